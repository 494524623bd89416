"""The ESRGAN trainer's discriminator (Discriminator, reference backend/trainingcode/esrgan_code/models.py:36-71) without a GPU:
cid_esd_* (include/cid.h) and esrgan_disc.py.  State-dict structure, checkpoint reading, the host pack (the fc permutation and the
convolution blocks), the C ABI's host-side argument checks, the workspace formula and the BCE-with-logits formula.  The GPU tests are
in tests/test_esrgan_disc.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth
from celebrity_image_denoiser_amd.esrgan_disc import ESRGANDiscriminator, feature_side, load_esrgan_discriminator

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import esrgan_disc_oracle as oracle  # noqa: E402
from esrgan_disc_oracle import bce_with_logits, expected_workspace as _expected_workspace  # noqa: E402

ERR_INVALID, ERR_SHAPE, ERR_KEY, ERR_STATE, ERR_WORKSPACE = 1, 2, 3, 4, 5
FAKE = 1 << 20   # 256-byte aligned, never dereferenced: every forward call in this file must fail on the host
SMALL = (3, 37, 53)


def test_state_dict_matches_the_stock_module():
    for shape in (SMALL, (3, 256, 256)):
        torch.manual_seed(5)
        ours = ESRGANDiscriminator(shape).state_dict()
        torch.manual_seed(5)
        ref = oracle.StockESRGANDiscriminator(shape).state_dict()
        assert list(ours) == list(ref) == [f"{l}.{k}" for l in ("conv1", "conv2", "conv3", "conv4", "fc") for k in ("weight", "bias")]
        for k in ref:
            assert ours[k].shape == ref[k].shape and ours[k].dtype == ref[k].dtype, k
            assert torch.equal(ours[k], ref[k]), k   # same layers drawn in the same order: the same default initialisation
        assert list(ESRGANDiscriminator(shape).buffers()) == []
        # the portable weight sets carry the same keys, shapes and dtypes in the same order
        assert {k: v[0] for k, v in synth.esrgan_disc_param_shapes(shape).items()} == {k: tuple(v.shape) for k, v in ref.items()}
        for kind in oracle.WSETS:
            sd = synth.make_esrgan_disc_state_dict(kind, shape)
            assert list(sd) == list(ref)
            assert all(tuple(sd[k].shape) == tuple(ref[k].shape) and sd[k].dtype == np.float32 for k in ref)
    assert ESRGANDiscriminator((3, 256, 256)).fc.weight.shape == (1, 512 * 16 * 16)
    assert [feature_side(v) for v in (1, 5, 7, 16, 37, 53, 256, 264)] == [1, 1, 1, 1, 3, 4, 16, 17]
    for bad in ((1, 8, 8), (3, 0, 8), (3, 8, _lib.CID_ESD_MAX_SIDE + 1), (3, 8)):
        with pytest.raises(ValueError):
            ESRGANDiscriminator(bad)


def test_state_dict_round_trips_both_ways():
    sd = oracle.weights("trained", SMALL[1:])
    ours, stock = ESRGANDiscriminator(SMALL), oracle.StockESRGANDiscriminator(SMALL)
    ours.load_state_dict(sd, strict=True)
    stock.load_state_dict(ours.state_dict(), strict=True)
    for k, v in stock.state_dict().items():
        assert v.dtype == sd[k].dtype and torch.equal(v, sd[k]), k
    back = ESRGANDiscriminator(SMALL)
    back.load_state_dict(stock.state_dict(), strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in back.state_dict().items())
    with pytest.raises(RuntimeError, match="size mismatch"):   # another input size has another fc.weight
        ESRGANDiscriminator((3, 64, 64)).load_state_dict(sd, strict=True)
    # the restatement is the stock module
    x = oracle.images(2, *SMALL[1:])[1]
    with torch.no_grad():
        assert float((stock(x) - oracle.restate(sd, x)[1]).abs().max()) <= 1e-6


def _save_trainer_checkpoint(path, disc):
    gen = {k: torch.from_numpy(np.array(v)) for k, v in synth.make_esrgan_state_dict("default").items()}
    # the ESRGAN trainer's checkpoint keys (esrgan_train.py:166-172)
    torch.save({"G": gen, "D": disc, "g_opt": {"state": {}, "param_groups": []}, "d_opt": {"state": {}, "param_groups": []},
                "epoch": 1}, path)


def test_loader_reads_the_trainer_checkpoint_through_the_safe_reader(tmp_path, monkeypatch):
    from celebrity_image_denoiser_amd import ckpt, esrgan_disc

    disc = oracle.weights("trained", (256, 256))
    path = str(tmp_path / "esrgan_epoch_1.pth")
    _save_trainer_checkpoint(path, disc)
    sd = ckpt.read_state_dict(path, key_candidates=("D", "discriminator", "state_dict"))
    assert list(sd) == list(disc) and all(np.array_equal(np.asarray(sd[k]), disc[k].numpy()) for k in disc)
    # the loader itself: stop it where it needs the GPU, after the state dict is in the module
    seen = {}

    def to(self, device):
        seen["sd"] = {k: v.clone() for k, v in self.state_dict().items()}
        seen["shape"] = self.input_shape
        raise InterruptedError

    monkeypatch.setattr(esrgan_disc._packed, "cuda_device", lambda device, who: torch.device("cuda", 0))
    monkeypatch.setattr(ESRGANDiscriminator, "to", to)
    for source in (path, {"D": disc, "epoch": 1}, {"module." + k: v for k, v in disc.items()}):
        seen.clear()
        with pytest.raises(InterruptedError):
            load_esrgan_discriminator(source)
        assert seen["shape"] == (3, 256, 256)   # inferred from fc.weight's width
        assert all(torch.equal(seen["sd"][k], disc[k]) for k in disc)
    # a checkpoint without a D entry is refused
    bad = str(tmp_path / "no_d.pth")
    torch.save({"G": {"initial.0.weight": torch.zeros(4)}, "g_opt": {}, "epoch": 1}, bad)
    with pytest.raises(KeyError, match="no discriminator state dict"):
        load_esrgan_discriminator(bad)
    with pytest.raises(KeyError, match="no discriminator state dict"):
        load_esrgan_discriminator({"G": {"initial.0.weight": torch.zeros(4)}, "epoch": 1})
    # a width that 256 x 256 does not give needs input_shape; with it, the size is the caller's
    small = oracle.weights("default", SMALL[1:])
    with pytest.raises(ValueError, match="pass input_shape"):
        load_esrgan_discriminator({"D": small})
    seen.clear()
    with pytest.raises(InterruptedError):
        load_esrgan_discriminator({"D": small}, input_shape=SMALL)
    assert seen["shape"] == SMALL and torch.equal(seen["sd"]["fc.weight"], small["fc.weight"])


def test_load_without_a_gpu_raises_the_no_fallback_error(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # what a machine without a GPU answers
    with pytest.raises(RuntimeError, match="an AMD GPU is required \\(no CPU fallback\\)"):
        load_esrgan_discriminator(oracle.weights("default", (256, 256)))
    with pytest.raises(RuntimeError, match="an AMD GPU is required \\(no CPU fallback\\)"):
        load_esrgan_discriminator(None, device="cpu")


# ------------------------------------------------------------------------------------------------------------ the host pack
def _align64(v):
    return (v + 63) // 64 * 64


def _expected_blob(sd, h, w):
    """The layout include/cid.h documents for cid_esd_packed_weights_bytes, restated in numpy."""
    parts = []
    for name, cin, cout in synth.ESRGAN_DISC_CONVS:
        wt, b = sd[name + ".weight"], sd[name + ".bias"]
        if name == "conv1":
            seg = np.concatenate([wt.reshape(-1), b])
        else:
            blocks = []
            for part in range(cout // 64):
                wp = wt[64 * part:64 * part + 64]                                    # [64, cin, 3, 3]
                wp = wp.reshape(64, cin // 8, 8, 9).transpose(1, 3, 2, 0)            # [cin/8, tap, ci%8, co%64]
                blocks += [wp.reshape(-1), b[64 * part:64 * part + 64]]
            seg = np.concatenate(blocks)
        parts.append(np.concatenate([seg, np.zeros(_align64(seg.size) - seg.size, np.float32)]))
    p = feature_side(h) * feature_side(w)
    fcw = sd["fc.weight"].reshape(512 // 8, 8, p).transpose(0, 2, 1).reshape(-1)      # feature c*P + p -> ((c/8)*P + p)*8 + c%8
    parts.append(np.concatenate([fcw, np.zeros(_align64(fcw.size) - fcw.size, np.float32)]))
    parts.append(np.concatenate([sd["fc.bias"], np.zeros(63, np.float32)]))
    return np.concatenate(parts)


def _fc_positions(p):
    """NCHW feature index -> C8 position, one by one."""
    return np.array([((f // p) // 8 * p + f % p) * 8 + (f // p) % 8 for f in range(512 * p)])


@pytest.mark.parametrize("hw", [(1, 1), (37, 53), (264, 24)], ids=lambda s: "x".join(map(str, s)))
def test_host_pack_layout(hw):
    """H4*W4 = 1, 12 (3x4) and 34 (17x2): every staged float is where include/cid.h says.  cid_esd_export_packed hands out the
    bytes cid_esd_upload_weights sends to the device."""
    h, w = hw
    p = feature_side(h) * feature_side(w)
    assert p == {(1, 1): 1, (37, 53): 12, (264, 24): 34}[hw]
    sd = {k: v.astype(np.float32) for k, v in synth.make_esrgan_disc_state_dict("trained", (3, h, w)).items()}
    want = _expected_blob(sd, h, w)
    L = _lib.lib()
    assert L.cid_esd_packed_weights_bytes(h, w) == want.size * 4
    # the fc permutation is the NCHW -> C8 map
    fcw_off = sum(_align64(cout * cin * 9 + cout) for _, cin, cout in synth.ESRGAN_DISC_CONVS)
    pos = _fc_positions(p)
    assert sorted(pos) == list(range(512 * p))
    assert np.array_equal(want[fcw_off + pos], sd["fc.weight"].reshape(-1))
    # and the library stages exactly these floats
    got = _staged_blob(sd, h, w)
    assert got.size == want.size and np.array_equal(got, want)


def _staged_blob(sd, h, w):
    """What a handle stages for `sd` (cid_esd_export_packed)."""
    L = _lib.lib()
    d = ctypes.c_void_p()
    assert L.cid_esd_create(ctypes.byref(d), h, w) == 0
    try:
        n = L.cid_esd_packed_weights_bytes(h, w) // 4
        out = np.zeros(n, np.float32)
        assert L.cid_esd_export_packed(d, out.ctypes.data, out.nbytes) == ERR_STATE   # nothing set yet
        for k, v in sd.items():
            a = np.ascontiguousarray(v)
            shape = (ctypes.c_int64 * a.ndim)(*a.shape)
            assert L.cid_esd_set_weight(d, k.encode(), a.ctypes.data, shape, a.ndim) == 0, k
        assert L.cid_esd_export_packed(d, out.ctypes.data, out.nbytes - 4) == ERR_WORKSPACE
        assert L.cid_esd_export_packed(d, out.ctypes.data, out.nbytes) == 0
        return out
    finally:
        L.cid_esd_destroy(d)


# ------------------------------------------------------------------------------------------------------------ the C ABI
@pytest.fixture()
def handle():
    L = _lib.lib()
    d = ctypes.c_void_p()
    assert L.cid_esd_create(ctypes.byref(d), 37, 53) == 0
    yield d
    L.cid_esd_destroy(d)


def _fwd(d, n=2, h=37, w=53, x=FAKE, fmt=0, out=FAKE, ws=FAKE, ws_bytes=1 << 40):
    return _lib.lib().cid_esd_forward(d, x, fmt, out, n, h, w, ws, ws_bytes, None)


def _workspace_bytes(n, h, w):
    out = ctypes.c_size_t()
    return _lib.lib().cid_esd_workspace_bytes(n, h, w, ctypes.byref(out)), out.value


def test_create_and_weight_errors(handle):
    L = _lib.lib()
    d = ctypes.c_void_p()
    assert L.cid_esd_create(None, 8, 8) == ERR_INVALID
    for h, w in ((0, 8), (8, 0), (-1, 8), (_lib.CID_ESD_MAX_SIDE + 1, 8), (8, _lib.CID_ESD_MAX_SIDE + 1)):
        assert L.cid_esd_create(ctypes.byref(d), h, w) == ERR_SHAPE and not d.value
        assert L.cid_esd_packed_weights_bytes(h, w) == 0
    assert L.cid_esd_last_error(None) == b"null handle"
    d = handle
    w = np.zeros(512 * 256 * 9, np.float32)

    def put(key, shape):
        sh = (ctypes.c_int64 * len(shape))(*shape)
        return L.cid_esd_set_weight(d, key, w.ctypes.data, sh, len(shape))

    assert put(b"conv1.weight", (64, 3, 3, 3)) == 0
    for key in (b"conv0.weight", b"conv5.weight", b"fc", b"leaky_relu.weight", b"model.0.weight", b"conv1.running_mean"):
        assert put(key, (64, 3, 3, 3)) == ERR_KEY, key
    assert L.cid_esd_last_error(d).startswith(b"cid_esd_set_weight: unknown key 'conv1.running_mean'")
    assert put(b"conv4.weight", (256, 512, 3, 3)) == ERR_SHAPE
    assert put(b"conv4.weight", (512, 256, 3)) == ERR_SHAPE
    assert put(b"conv3.bias", (128,)) == ERR_SHAPE
    assert L.cid_esd_last_error(d) == b"cid_esd_set_weight: size mismatch for conv3.bias"
    # fc.weight must be [1, 512 * H4 * W4] for the handle's input: 37 x 53 gives 3 x 4 features per channel
    assert put(b"fc.weight", (1, 512 * 12)) == 0
    for shape in ((1, 512 * 16 * 16), (512 * 12,), (512 * 12, 1), (1, 512 * 12 + 1)):
        assert put(b"fc.weight", shape) == ERR_SHAPE, shape
    assert b"[1, 6144]" in L.cid_esd_last_error(d)
    assert put(b"fc.bias", (1,)) == 0 and put(b"fc.bias", (2,)) == ERR_SHAPE
    assert L.cid_esd_set_weight(d, None, w.ctypes.data, None, 0) == ERR_INVALID
    assert L.cid_esd_set_weight(d, b"conv1.bias", None, None, 0) == ERR_INVALID
    assert L.cid_esd_upload_weights(d, None, None) == ERR_INVALID
    assert L.cid_esd_upload_weights(d, FAKE + 64, None) == ERR_WORKSPACE
    # upload before every key is set: CID_ERR_STATE naming the first missing layer
    assert L.cid_esd_upload_weights(d, FAKE, None) == ERR_STATE
    assert L.cid_esd_last_error(d) == b"cid_esd_upload_weights: conv1 not set"
    assert put(b"conv1.bias", (64,)) == 0
    assert L.cid_esd_upload_weights(d, FAKE, None) == ERR_STATE
    assert L.cid_esd_last_error(d) == b"cid_esd_upload_weights: conv2 not set"


def test_cabi_argument_errors_come_before_any_launch(handle):
    d = handle
    L = _lib.lib()
    assert L.cid_esd_forward(None, FAKE, 0, FAKE, 2, 37, 53, FAKE, 1 << 40, None) == ERR_INVALID
    # CID_ERR_INVALID
    assert _fwd(d, x=None) == ERR_INVALID and L.cid_esd_last_error(d) == b"cid_esd_forward: null pointer"
    assert _fwd(d, out=None) == ERR_INVALID
    assert _fwd(d, ws=None) == ERR_INVALID
    assert _fwd(d, fmt=7) == ERR_INVALID
    assert _fwd(d, x=FAKE + 1) == ERR_INVALID                        # misaligned fp32 input
    assert _fwd(d, x=FAKE + 1, fmt=1, ws_bytes=0) == ERR_WORKSPACE   # a uint8 input has no alignment
    assert _fwd(d, out=FAKE + 2) == ERR_INVALID
    # CID_ERR_SHAPE: N <= 0, H or W different from the handle's
    for n in (0, -3):
        assert _fwd(d, n=n) == ERR_SHAPE
    for h, w in ((53, 37), (37, 54), (36, 53), (256, 256), (0, 53)):
        assert _fwd(d, h=h, w=w) == ERR_SHAPE
        assert b"the handle was created for 37x53" in L.cid_esd_last_error(d)
    # CID_ERR_WORKSPACE: too small (by one byte) or misaligned; then CID_ERR_STATE, still before any launch
    rc, need = _workspace_bytes(2, 37, 53)
    assert rc == 0
    assert _fwd(d, ws_bytes=need - 1) == ERR_WORKSPACE
    assert b"cid_esd_workspace_bytes" in L.cid_esd_last_error(d)
    assert _fwd(d, ws=FAKE + 16, ws_bytes=need) == ERR_WORKSPACE
    assert _fwd(d, ws_bytes=need) == ERR_STATE
    assert L.cid_esd_last_error(d) == b"cid_esd_forward: weights not uploaded"
    # the first of several faults is the one reported
    assert _fwd(d, x=None, n=0, ws_bytes=0) == ERR_INVALID
    assert _fwd(d, n=0, ws_bytes=0) == ERR_SHAPE
    assert _fwd(d, h=5, ws_bytes=0) == ERR_SHAPE
    assert _fwd(d, ws_bytes=0) == ERR_WORKSPACE
    # cid_esd_losses / cid_esd_trainer_losses
    assert L.cid_esd_losses(None, FAKE, 2, FAKE, None) == ERR_INVALID
    assert L.cid_esd_losses(FAKE, None, 2, FAKE, None) == ERR_INVALID
    assert L.cid_esd_losses(FAKE, FAKE, 2, None, None) == ERR_INVALID
    assert L.cid_esd_losses(FAKE + 2, FAKE, 2, FAKE, None) == ERR_INVALID
    assert L.cid_esd_losses(FAKE, FAKE, 2, FAKE + 4, None) == ERR_INVALID
    assert L.cid_esd_losses(FAKE, FAKE, 0, FAKE, None) == ERR_SHAPE
    assert L.cid_esd_trainer_losses(FAKE, FAKE, None, 0, FAKE, 0, 2, 8, 8, FAKE, None) == ERR_INVALID
    assert L.cid_esd_trainer_losses(FAKE, FAKE, FAKE, 0, FAKE, 3, 2, 8, 8, FAKE, None) == ERR_INVALID
    assert L.cid_esd_trainer_losses(FAKE, FAKE, FAKE + 2, 0, FAKE, 0, 2, 8, 8, FAKE, None) == ERR_INVALID
    assert L.cid_esd_trainer_losses(FAKE, FAKE, FAKE, 0, FAKE, 0, 0, 8, 8, FAKE, None) == ERR_SHAPE
    assert L.cid_esd_trainer_losses(FAKE, FAKE, FAKE, 0, FAKE, 0, 2, 0, 8, FAKE, None) == ERR_SHAPE


def test_workspace_bytes_equals_the_documented_formula():
    for shape in [(2, 1, 1), (4, 7, 5), (3, 16, 16), (2, 37, 53), (1, 70, 130), (8, 256, 256), (65537, 1, 1)]:
        offs, total = _expected_workspace(*shape)
        assert _workspace_bytes(*shape) == (0, total), shape
    # four distinct regions: at 8 x 256 x 256 a1 is 32 MiB and a2 + a3 + a4 another 28 MiB
    offs, total = _expected_workspace(8, 256, 256)
    assert offs == [0, 32 << 20, 48 << 20, 56 << 20] and total == 60 << 20
    assert _expected_workspace(2, 1, 1) == ([0, 512, 1536, 3584], 7680)
    assert _workspace_bytes(0, 8, 8)[0] == ERR_SHAPE and _workspace_bytes(1, 0, 8)[0] == ERR_SHAPE
    assert _workspace_bytes(1, 8, _lib.CID_ESD_MAX_SIDE + 1)[0] == ERR_SHAPE
    assert _lib.lib().cid_esd_workspace_bytes(2, 8, 8, None) == ERR_INVALID


def test_python_layer_rejects_bad_inputs():
    from celebrity_image_denoiser_amd.esrgan_disc import esrgan_trainer_losses

    m = ESRGANDiscriminator((3, 8, 8))
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
        esrgan_trainer_losses(m, torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 9))
    with pytest.raises(RuntimeError, match="on the discriminator's GPU"):
        esrgan_trainer_losses(m, torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8))
    with pytest.raises(RuntimeError, match=r"fp32 \[N,3,H,W\] or uint8 \[N,H,W,3\]"):
        esrgan_trainer_losses(m, torch.zeros(2, 3, 8, 8, dtype=torch.float64), torch.zeros(2, 3, 8, 8))


# ------------------------------------------------------------------------------------------------------------ the BCE formula
def test_bce_formula_matches_torch_in_float64():
    x = np.array([-40.0, -1.0, 0.0, 1e-8, 3.0, 40.0])
    for y in (0.0, 1.0):
        got = bce_with_logits(x, y)
        want = torch.nn.BCEWithLogitsLoss(reduction="none")(torch.from_numpy(x), torch.full((6,), y, dtype=torch.float64)).numpy()
        # torch forms log(1 + exp(-|x|)) without log1p, so its own value is only good to one rounding of 1 + exp(-|x|), 2^-53 absolute
        # (at x = -40, y = 0 it returns exactly 0 where the term is exp(-40) = 4.2e-18): four such roundings of room, no more
        assert np.all(np.isfinite(got)) and np.allclose(got, want, rtol=1e-14, atol=4 * 2.0 ** -53), (y, got, want)
        mean = float(torch.nn.BCEWithLogitsLoss()(torch.from_numpy(x), torch.full((6,), y, dtype=torch.float64)))
        assert got.mean() == pytest.approx(mean, rel=1e-14)
    assert bce_with_logits(40.0, 0.0) == pytest.approx(40.0, rel=1e-15) and 0.0 < bce_with_logits(40.0, 1.0) < 1e-17
    assert bce_with_logits(0.0, 1.0) == np.log(2.0)
