"""The SRGAN trainer's discriminator (SRGANDiscriminator, reference backend/trainingcode/srgan_code/sr_ganTrainGNew.py:54-80) without
a GPU: cid_srd_* (include/cid.h) and srgan_disc.py.  State-dict structure, checkpoint reading, the C ABI's host-side argument checks
in their documented order, the workspace formula, and the Python layer's input checks.  The GPU tests are in tests/test_srgan_disc.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import srgan_disc_oracle as oracle  # noqa: E402

ERR_INVALID, ERR_SHAPE, ERR_KEY, ERR_STATE, ERR_WORKSPACE = 1, 2, 3, 4, 5
SHAPES = [(2, 1, 1), (4, 7, 5), (8, 37, 53), (3, 41, 70)]
N_PARAMS = sum(cout * cin * k * k + cout for _, cin, cout, k in oracle.CONVS) + 2 * sum(c for _, c in oracle.BNS)


def test_state_dict_matches_the_stock_module():
    from celebrity_image_denoiser_amd.srgan_disc import SRGANDiscriminator

    torch.manual_seed(5)
    ours = SRGANDiscriminator().state_dict()
    torch.manual_seed(5)
    ref = oracle.StockSRGANDiscriminator().state_dict()
    assert list(ours) == list(ref)
    assert len(ours) == 14 + 5 * 4
    for k in ref:
        assert ours[k].shape == ref[k].shape and ours[k].dtype == ref[k].dtype, k
        assert torch.equal(ours[k], ref[k]), k   # same layers drawn in the same order: the same default initialisation
    for i, _ in oracle.BNS:
        assert ours[f"model.{i}.num_batches_tracked"].dtype == torch.int64
    n_params = sum(v.numel() for k, v in ours.items() if k.endswith(("weight", "bias")))
    n_stats = sum(v.numel() for k, v in ours.items() if k.endswith(("running_mean", "running_var")))
    assert (n_params, n_stats) == (N_PARAMS, 2 * (64 + 128 + 128 + 256))
    # the portable weight sets carry the same keys, shapes and dtypes in the same order
    for kind in oracle.WSETS:
        sd = synth.make_srgan_disc_state_dict(kind)
        assert list(sd) == list(ref)
        for k in ref:
            assert tuple(sd[k].shape) == tuple(ref[k].shape) and str(sd[k].dtype) == str(ref[k].dtype).replace("torch.", ""), k


def test_state_dict_round_trips_both_ways():
    from celebrity_image_denoiser_amd.srgan_disc import SRGANDiscriminator

    sd = oracle.weights("trained")
    ours, stock = SRGANDiscriminator(), oracle.StockSRGANDiscriminator()
    ours.load_state_dict(sd, strict=True)
    stock.load_state_dict(ours.state_dict(), strict=True)
    for k, v in stock.state_dict().items():
        assert v.dtype == sd[k].dtype and torch.equal(v, sd[k]), k
    back = SRGANDiscriminator()
    back.load_state_dict(stock.state_dict(), strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in back.state_dict().items())
    assert ours.training and not back.eval().training and all(not m.training for m in back.model)


def test_calibrated_logits_stay_out_of_saturation():
    z = oracle.calibration_logits(oracle.weights("trained"))
    assert z.shape == (16,) and float(z.abs().max()) <= oracle.LOGIT_RANGE
    assert float(z.abs().max()) > 0.9 * oracle.LOGIT_RANGE and float(z.std()) > 0.1   # and they are not all alike


def test_trainer_checkpoint_loads_through_the_torch_free_reader(tmp_path):
    from celebrity_image_denoiser_amd import api
    from celebrity_image_denoiser_amd.srgan_disc import SRGANDiscriminator

    gen = {k: torch.from_numpy(v) for k, v in synth.make_srgan_state_dict("default").items()}
    disc = oracle.weights("trained")
    path = str(tmp_path / "ckpt.pth")
    # the SRGAN trainer's checkpoint keys (sr_ganTrainGNew.py:342-353)
    torch.save({"epoch": 3, "generator": gen, "discriminator": disc, "optimizer_G": {}, "optimizer_D": {}, "g_loss": 0.5,
                "d_loss": 1.25, "psnr": np.float64(27.5), "ssim": 0.8, "lpips": 0.3}, path)
    sd = api._read_checkpoint_file(path, key_candidates=("discriminator",))
    assert list(sd) == list(disc)
    for k in disc:
        assert sd[k].dtype == disc[k].dtype and torch.equal(sd[k], disc[k]), k
    m = SRGANDiscriminator()
    m.load_state_dict(sd, strict=True)
    for k, v in m.state_dict().items():
        assert v.dtype == disc[k].dtype and torch.equal(v, disc[k]), k
    # DataParallel prefixes are stripped by the same rule
    path2 = str(tmp_path / "dp.pth")
    torch.save({"discriminator": {"module." + k: v for k, v in disc.items()}}, path2)
    sd2 = api._read_checkpoint_file(path2, key_candidates=("discriminator",))
    assert list(sd2) == list(disc) and all(torch.equal(sd2[k], disc[k]) for k in disc)


def test_load_without_a_gpu_raises_the_no_fallback_error(monkeypatch):
    from celebrity_image_denoiser_amd import load_srgan_discriminator

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # what a machine without a GPU answers
    with pytest.raises(RuntimeError, match="an AMD GPU is required \\(no CPU fallback\\)"):
        load_srgan_discriminator(oracle.weights("default"))
    with pytest.raises(RuntimeError, match="an AMD GPU is required \\(no CPU fallback\\)"):
        load_srgan_discriminator(oracle.weights("default"), device="cpu")


def _workspace_bytes(n, h, w, training):
    out = ctypes.c_size_t()
    rc = _lib.lib().cid_srd_workspace_bytes(n, h, w, training, ctypes.byref(out))
    return rc, out.value


def _expected_workspace(n, h, w, training):
    """The formula of include/cid.h (cid_srd_workspace_bytes)."""
    a256 = lambda v: (v + 255) // 256 * 256   # noqa: E731
    h2, w2 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    h4, w4 = (h2 - 1) // 2 + 1, (w2 - 1) // 2 + 1
    total = a256(4 * n * max(64 * h * w, 128 * h2 * w2, 256 * h4 * w4)) + a256(4 * n * max(64 * h2 * w2, 128 * h4 * w4))
    total += a256(4 * 4 * 256 * 2)
    if training:
        for (ho, wo, th, c) in ((h2, w2, 16, 64), (h2, w2, 8, 128), (h4, w4, 8, 128), (h4, w4, 8, 256)):
            total += a256(8 * c * 2 * n * -(-ho // th) * -(-wo // 16))
    return total


def _bn_array(eps=1e-5, momentum=0.1, ptr=1 << 20, nbt=True):
    from celebrity_image_denoiser_amd.discriminator import _BnArg

    arr = (_BnArg * 4)()
    for i in range(4):
        arr[i] = _BnArg(ptr, ptr, ptr, ptr, ptr if nbt else None, eps, momentum)
    return arr


@pytest.fixture()
def handle():
    L = _lib.lib()
    d = ctypes.c_void_p()
    assert L.cid_srd_create(ctypes.byref(d)) == 0
    yield d
    L.cid_srd_destroy(d)


FAKE = 1 << 20   # 256-byte aligned, never dereferenced: every forward call in this file must fail on the host


def _fwd(d, n=2, h=16, w=16, training=0, bn="ok", x=FAKE, fmt=0, out=FAKE, ws=FAKE, ws_bytes=1 << 40):
    return _lib.lib().cid_srd_forward(d, x, fmt, out, n, h, w, _bn_array() if isinstance(bn, str) else bn, training, ws, ws_bytes, None)


def test_cabi_argument_errors_come_before_any_launch(handle):
    d = handle
    L = _lib.lib()
    assert L.cid_srd_forward(None, FAKE, 0, FAKE, 2, 16, 16, _bn_array(), 0, FAKE, 1 << 40, None) == ERR_INVALID
    assert L.cid_srd_last_error(None) == b"null handle"
    # CID_ERR_INVALID
    assert _fwd(d, x=None) == ERR_INVALID and L.cid_srd_last_error(d) == b"cid_srd_forward: null pointer"
    assert _fwd(d, out=None) == ERR_INVALID
    assert _fwd(d, bn=None) == ERR_INVALID
    assert _fwd(d, ws=None) == ERR_INVALID
    assert _fwd(d, fmt=7) == ERR_INVALID
    assert _fwd(d, x=FAKE + 1) == ERR_INVALID                  # misaligned fp32 input
    assert _fwd(d, x=FAKE + 1, fmt=1, ws_bytes=0) == ERR_WORKSPACE   # a uint8 input has no alignment
    assert _fwd(d, out=FAKE + 2) == ERR_INVALID
    assert _fwd(d, training=2) == ERR_INVALID
    for eps in (float("nan"), float("inf"), -1e-5):
        assert _fwd(d, bn=_bn_array(eps=eps)) == ERR_INVALID
        assert _fwd(d, bn=_bn_array(eps=eps), training=1) == ERR_INVALID
    for mom in (float("nan"), float("inf"), -0.5):
        assert _fwd(d, bn=_bn_array(momentum=mom), training=1) == ERR_INVALID
    assert _fwd(d, bn=_bn_array(nbt=False), training=1) == ERR_INVALID
    for layer in range(4):                                     # all four BatchNorms are checked, the fourth included
        for field in ("gamma", "beta", "running_mean", "running_var"):
            arr = _bn_array()
            setattr(arr[layer], field, None)
            assert _fwd(d, bn=arr) == ERR_INVALID, (layer, field)
            assert L.cid_srd_last_error(d) == b"cid_srd_forward: null BatchNorm pointer"
        arr = _bn_array()
        arr[layer].eps = -1.0
        assert _fwd(d, bn=arr) == ERR_INVALID
        arr = _bn_array()
        arr[layer].num_batches_tracked = None
        assert _fwd(d, bn=arr, training=1) == ERR_INVALID and _fwd(d, bn=arr, ws_bytes=0) == ERR_WORKSPACE
    # momentum and num_batches_tracked are not read in eval mode; momentum=None is the sentinel
    assert _fwd(d, bn=_bn_array(nbt=False, momentum=-0.5), ws_bytes=0) == ERR_WORKSPACE
    assert _fwd(d, bn=_bn_array(momentum=_lib.CID_DISC_MOMENTUM_NONE), training=1, ws_bytes=0) == ERR_WORKSPACE
    # CID_ERR_SHAPE
    for n, h, w in ((0, 8, 8), (2, 0, 8), (2, 8, 0), (1, 65536, 32768)):
        assert _fwd(d, n=n, h=h, w=w) == ERR_SHAPE
        assert _fwd(d, n=n, h=h, w=w, training=1) == ERR_SHAPE
        assert b"input shape not accepted" in L.cid_srd_last_error(d)
    for h, w in ((1, 1), (2, 2), (4, 4), (3, 2), (1, 4)):      # train mode with one value per channel: N = 1, H, W <= 4
        assert _fwd(d, n=1, h=h, w=w, training=1) == ERR_SHAPE
        assert L.cid_srd_last_error(d) == b"Expected more than 1 value per channel when training"
        assert _fwd(d, n=1, h=h, w=w, training=0, ws_bytes=0) == ERR_WORKSPACE
        assert _workspace_bytes(1, h, w, 1)[0] == ERR_SHAPE
    assert _fwd(d, n=1, h=5, w=4, training=1, ws_bytes=0) == ERR_WORKSPACE   # H4 = 2
    assert _fwd(d, n=2, h=1, w=1, training=1, ws_bytes=0) == ERR_WORKSPACE   # two values per channel
    # CID_ERR_WORKSPACE: too small (by one byte) or misaligned; then CID_ERR_STATE, still before any launch
    for training in (0, 1):
        rc, need = _workspace_bytes(3, 37, 53, training)
        assert rc == 0
        assert _fwd(d, n=3, h=37, w=53, training=training, ws_bytes=need - 1) == ERR_WORKSPACE
        assert b"cid_srd_workspace_bytes" in L.cid_srd_last_error(d)
        assert _fwd(d, n=3, h=37, w=53, training=training, ws=FAKE + 16, ws_bytes=need) == ERR_WORKSPACE
        assert _fwd(d, n=3, h=37, w=53, training=training, ws_bytes=need) == ERR_STATE
        assert L.cid_srd_last_error(d) == b"cid_srd_forward: weights not uploaded"
    # cid_srd_losses
    assert L.cid_srd_losses(None, FAKE, 2, FAKE, None) == ERR_INVALID
    assert L.cid_srd_losses(FAKE, None, 2, FAKE, None) == ERR_INVALID
    assert L.cid_srd_losses(FAKE, FAKE, 2, None, None) == ERR_INVALID
    assert L.cid_srd_losses(FAKE + 2, FAKE, 2, FAKE, None) == ERR_INVALID
    assert L.cid_srd_losses(FAKE, FAKE, 2, FAKE + 4, None) == ERR_INVALID
    assert L.cid_srd_losses(FAKE, FAKE, 0, FAKE, None) == ERR_SHAPE


def test_cabi_checks_come_in_the_documented_order(handle):
    """INVALID (pointers, format, alignment, training, BatchNorm fields) before SHAPE before WORKSPACE before STATE: a call wrong
    in several ways reports the first of them."""
    d = handle
    bad_bn = _bn_array(eps=-1.0)
    assert _fwd(d, x=None, n=0, ws_bytes=0) == ERR_INVALID
    assert _fwd(d, fmt=9, n=0, ws_bytes=0) == ERR_INVALID
    assert _fwd(d, training=3, n=0, ws_bytes=0) == ERR_INVALID
    assert _fwd(d, bn=bad_bn, n=0, ws_bytes=0) == ERR_INVALID
    assert _fwd(d, n=0, ws_bytes=0) == ERR_SHAPE
    assert _fwd(d, n=1, h=1, w=1, training=1, ws_bytes=0) == ERR_SHAPE
    assert _fwd(d, ws_bytes=0) == ERR_WORKSPACE
    assert _fwd(d) == ERR_STATE


def test_workspace_bytes_equals_the_documented_formula():
    for shape in SHAPES + [(16, 256, 256), (1, 9, 300)]:
        for training in (0, 1):
            assert _workspace_bytes(*shape, training) == (0, _expected_workspace(*shape, training)), (shape, training)
    assert _workspace_bytes(3, 37, 53, 1)[1] > _workspace_bytes(3, 37, 53, 0)[1]
    # z11 is counted: of a 1x1 image it is the largest tensor of region A (256 floats against a0's 64 and z5's 128)
    assert _expected_workspace(1, 1, 1, 0) == 1024 + 512 + 8192
    assert _workspace_bytes(1, 1, 1, 0) == (0, 1024 + 512 + 8192)
    assert _workspace_bytes(2, 8, 8, 2)[0] == ERR_INVALID
    assert _lib.lib().cid_srd_workspace_bytes(2, 8, 8, 0, None) == ERR_INVALID


def test_weight_keys_shapes_and_upload_state(handle):
    d = handle
    L = _lib.lib()
    w = np.zeros((256, 128, 3, 3), np.float32)

    def put(key, shape):
        sh = (ctypes.c_int64 * len(shape))(*shape)
        return L.cid_srd_set_weight(d, key, w.ctypes.data, sh, len(shape))

    assert put(b"model.0.weight", (64, 3, 3, 3)) == 0
    for key in (b"model.3.weight", b"model.12.weight", b"model.12.running_mean", b"model.1.weight", b"model.18.weight", b"model.11"):
        assert put(key, (64, 3, 3, 3)) == ERR_KEY, key            # BatchNorm tensors are per call; the rest does not exist
    msg = L.cid_srd_last_error(d)
    assert msg.startswith(b"cid_srd_set_weight: unknown key 'model.11'") and b"model.3/6/9/12" in msg
    assert put(b"model.11.weight", (128, 256, 3, 3)) == ERR_SHAPE
    assert put(b"model.11.weight", (256, 128, 3)) == ERR_SHAPE
    assert put(b"model.15.weight", (512, 256)) == ERR_SHAPE
    assert put(b"model.17.bias", (512,)) == ERR_SHAPE
    assert L.cid_srd_last_error(d) == b"cid_srd_set_weight: size mismatch for model.17.bias"
    assert L.cid_srd_set_weight(d, None, w.ctypes.data, None, 0) == ERR_INVALID
    assert L.cid_srd_set_weight(d, b"model.0.bias", None, None, 0) == ERR_INVALID
    assert L.cid_srd_upload_weights(d, None, None) == ERR_INVALID
    assert L.cid_srd_upload_weights(d, FAKE + 64, None) == ERR_WORKSPACE
    # upload before every key is set: CID_ERR_STATE naming the first missing layer, whatever is still missing
    keys = [(f"model.{i}.weight".encode(), (cout, cin, k, k)) for i, cin, cout, k in oracle.CONVS]
    keys += [(f"model.{i}.bias".encode(), (cout,)) for i, cin, cout, k in oracle.CONVS]
    for key, shape in keys[:-1]:
        assert L.cid_srd_upload_weights(d, FAKE, None) == ERR_STATE
        assert put(key, shape) == 0, key
    assert L.cid_srd_upload_weights(d, FAKE, None) == ERR_STATE
    assert L.cid_srd_last_error(d) == b"cid_srd_upload_weights: model.17 not set"
    assert L.cid_srd_packed_weights_bytes() >= (N_PARAMS - 4 * (64 + 128 + 128 + 256)) * 4   # the convolutions; BatchNorm per call
    assert L.cid_srd_packed_weights_bytes() % 256 == 0


def test_python_layer_rejects_bad_inputs():
    from celebrity_image_denoiser_amd.srgan_disc import SRGANDiscriminator, srgan_trainer_losses

    m = SRGANDiscriminator()
    with pytest.raises(RuntimeError, match="CPU tensor"):
        m(torch.zeros(2, 3, 8, 8))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        m(torch.zeros(2, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="float32"):
        m(torch.zeros(2, 3, 8, 8, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"\[N,3,H,W\]"):
        m(torch.zeros(2, 4, 8, 8))
    with pytest.raises(RuntimeError, match=r"\[N,3,H,W\]"):
        m(torch.zeros(3, 8, 8))
    with pytest.raises(RuntimeError, match=r"\[N,H,W,3\]"):
        m(torch.zeros(2, 3, 8, 8, dtype=torch.uint8))
    with pytest.raises(TypeError):
        m(np.zeros((2, 3, 8, 8), np.float32))
    with pytest.raises(RuntimeError, match="differ in size"):
        srgan_trainer_losses(m, torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 9))
    with pytest.raises(RuntimeError, match="on the discriminator's GPU"):
        srgan_trainer_losses(m, torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8))
    with pytest.raises(RuntimeError, match=r"fp32 \[N,3,H,W\] or uint8 \[N,H,W,3\]"):
        srgan_trainer_losses(m, torch.zeros(2, 3, 8, 8, dtype=torch.float64), torch.zeros(2, 3, 8, 8))
