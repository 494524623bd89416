"""The trainer's discriminator (DenoiseDiscriminator, reference backend/trainingcode/denoise_gan_code/training.py:77-98) on the GPU:
cid_disc_* (include/cid.h) and discriminator.py.

The reference for error is a CPU restatement written here with torch.nn.functional (conv2d, batch_norm, leaky_relu,
adaptive_avg_pool2d, sigmoid), run in float64; the same code in float32 stands for "ATen fp32".  Two weight sets: the default
initialisation (fresh BatchNorm buffers, where eval-mode BatchNorm is nearly the identity) and a "trained-like" set whose BatchNorm
parameters and buffers are far from it, so that a swapped or unused pointer shows.

CPU: state_dict structure and initialisation, checkpoint reading, the C ABI's host-side argument checks, the Python layer's input checks.
GPU: eval and train parity (probabilities, running buffers, num_batches_tracked), determinism, a 1440x1920 batch, a non-default stream,
trainer_losses and evaluate_noise_types(..., discriminator=D)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from celebrity_image_denoiser_amd import _lib, synth

DEV = "cuda:0"
TOL = 1e-5
ERR_INVALID, ERR_SHAPE, ERR_KEY, ERR_STATE, ERR_WORKSPACE = 1, 2, 3, 4, 5
SHAPES = [(16, 256, 256), (64, 128, 128), (8, 37, 53), (4, 7, 5), (2, 1, 1)]
WSETS = ("default", "trained")
CONVS = ((0, 3, 64, 3), (2, 64, 64, 3), (5, 64, 128, 3), (8, 128, 128, 3), (12, 128, 1, 1))
BNS = ((3, 64), (6, 128), (9, 128))


class StockDiscriminator(nn.Module):
    """The reference's structure (training.py:77-98) with stock layers."""

    def __init__(self):
        super().__init__()
        self.model = nn.Sequential(
            nn.Conv2d(3, 64, kernel_size=3, padding=1), nn.LeakyReLU(0.2),
            nn.Conv2d(64, 64, kernel_size=3, stride=2, padding=1), nn.BatchNorm2d(64), nn.LeakyReLU(0.2),
            nn.Conv2d(64, 128, kernel_size=3, padding=1), nn.BatchNorm2d(128), nn.LeakyReLU(0.2),
            nn.Conv2d(128, 128, kernel_size=3, stride=2, padding=1), nn.BatchNorm2d(128), nn.LeakyReLU(0.2),
            nn.AdaptiveAvgPool2d(1), nn.Conv2d(128, 1, kernel_size=1), nn.Sigmoid())

    def forward(self, x):
        return self.model(x).view(-1)


def restate(sd, x, training, momentum=0.1, logits=False):
    """The forward in x's dtype.  `sd` holds tensors of that dtype (num_batches_tracked int64); in train mode its running buffers
    and counters are updated in place, as nn.BatchNorm2d does."""
    def conv(t, i, stride=1, pad=1):
        return F.conv2d(t, sd[f"model.{i}.weight"], sd[f"model.{i}.bias"], stride=stride, padding=pad)

    def bn(t, i):
        m = 0.0
        if training:
            sd[f"model.{i}.num_batches_tracked"] += 1
            m = momentum if momentum is not None else 1.0 / float(sd[f"model.{i}.num_batches_tracked"])
        return F.batch_norm(t, sd[f"model.{i}.running_mean"], sd[f"model.{i}.running_var"], sd[f"model.{i}.weight"],
                            sd[f"model.{i}.bias"], training, m, 1e-5)

    act = lambda t: F.leaky_relu(t, 0.2)   # noqa: E731
    y = act(conv(x, 0))
    y = act(bn(conv(y, 2, stride=2), 3))
    y = act(bn(conv(y, 5), 6))
    y = act(bn(conv(y, 8, stride=2), 9))
    y = F.conv2d(F.adaptive_avg_pool2d(y, 1), sd["model.12.weight"], sd["model.12.bias"]).view(-1)
    return y if logits else torch.sigmoid(y)


def cast(sd, dtype):
    return {k: (v.clone() if v.dtype == torch.int64 else v.to(dtype).clone()) for k, v in sd.items()}


def images_u8(n, h, w, first_index=0):
    """Noisy face-like uint8 [n,h,w,3] batches (varied activations)."""
    return synth.add_gaussian_noise(synth.clean_images_u8(n, h, w, first_index), 25.0, first_index)


def images(n, h, w, first_index=0):
    u8 = images_u8(n, h, w, first_index)
    return u8, torch.from_numpy(synth.normalize_u8(u8))


def make_weights(kind):
    """state_dict (CPU fp32) of a weight set."""
    torch.manual_seed(20261016)
    m = StockDiscriminator()
    if kind == "trained":
        g = torch.Generator().manual_seed(7)
        with torch.no_grad():
            for i, c in BNS:
                bn = m.model[i]
                bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
                bn.bias.copy_((torch.rand(c, generator=g) - 0.5) * 0.6)
                bn.running_mean.copy_((torch.rand(c, generator=g) - 0.5) * 0.4)
                bn.running_var.copy_(torch.rand(c, generator=g) * 2.8 + 0.2)
                bn.num_batches_tracked.fill_(7)
        # scale the 1x1 layer so that the logits of a calibration batch stay within +-1.5 in both modes (no sigmoid saturation)
        sd = cast(m.state_dict(), torch.float64)
        x = images(8, 48, 48, first_index=500)[1].double()
        b = float(sd["model.12.bias"])
        z = torch.cat([restate(cast(sd, torch.float64), x, t, logits=True) - b for t in (False, True)])
        s = 1.5 / float(z.abs().max())
        with torch.no_grad():
            m.model[12].weight.mul_(s)
            m.model[12].bias.fill_(-float(z.mean()) * s)
    return {k: v.clone() for k, v in m.state_dict().items()}


_WEIGHTS = {}


def weights(kind):
    if kind not in _WEIGHTS:
        _WEIGHTS[kind] = make_weights(kind)
    return _WEIGHTS[kind]


# ------------------------------------------------------------------------------------------------------------------ CPU tests
def test_state_dict_matches_the_reference_structure():
    from celebrity_image_denoiser_amd.discriminator import DenoiseDiscriminator

    torch.manual_seed(5)
    ours = DenoiseDiscriminator().state_dict()
    torch.manual_seed(5)
    ref = StockDiscriminator().state_dict()
    assert list(ours) == list(ref)
    assert len(ours) == 25
    for k in ref:
        assert ours[k].shape == ref[k].shape and ours[k].dtype == ref[k].dtype, k
        assert torch.equal(ours[k], ref[k]), k   # same layers drawn in the same order: the same default initialisation
    assert ours["model.3.num_batches_tracked"].dtype == torch.int64
    n_params = sum(v.numel() for k, v in ours.items() if k.endswith(("weight", "bias")))
    n_stats = sum(v.numel() for k, v in ours.items() if k.endswith(("running_mean", "running_var")))
    assert (n_params, n_stats) == (260929, 640)
    expected = [f"model.{i}.{p}" for i, *_ in CONVS for p in ("weight", "bias")]
    expected += [f"model.{i}.{p}" for i, _ in BNS for p in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    assert sorted(ours) == sorted(expected)


def test_trainer_checkpoint_loads_through_the_torch_free_reader(tmp_path):
    from celebrity_image_denoiser_amd import api
    from celebrity_image_denoiser_amd.discriminator import DenoiseDiscriminator

    gen = {k: torch.from_numpy(v) for k, v in synth.make_state_dict("default").items()}
    disc = weights("trained")
    path = str(tmp_path / "ckpt.pth")
    torch.save({"generator": gen, "discriminator": disc, "epoch": 3, "best_psnr": np.float64(31.25)}, path)
    sd = api._read_checkpoint_file(path, key_candidates=("discriminator",))
    assert list(sd) == list(disc)
    for k in disc:
        assert sd[k].dtype == disc[k].dtype and torch.equal(sd[k], disc[k]), k
    m = DenoiseDiscriminator()
    m.load_state_dict(sd, strict=True)
    for k, v in m.state_dict().items():
        assert v.dtype == disc[k].dtype and torch.equal(v, disc[k]), k
    # the generator's reader of the same file is unchanged
    g = api._read_checkpoint_file(path)
    assert list(g) == list(gen) and all(torch.equal(g[k], gen[k]) for k in gen)
    # DataParallel prefixes are stripped by the same rule
    path2 = str(tmp_path / "dp.pth")
    torch.save({"discriminator": {"module." + k: v for k, v in disc.items()}}, path2)
    sd2 = api._read_checkpoint_file(path2, key_candidates=("discriminator",))
    assert list(sd2) == list(disc) and all(torch.equal(sd2[k], disc[k]) for k in disc)


def _workspace_bytes(n, h, w, training):
    out = ctypes.c_size_t()
    rc = _lib.lib().cid_disc_workspace_bytes(n, h, w, training, ctypes.byref(out))
    return rc, out.value


def _expected_workspace(n, h, w, training):
    a256 = lambda v: (v + 255) // 256 * 256   # noqa: E731
    h2, w2 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    h4, w4 = (h2 - 1) // 2 + 1, (w2 - 1) // 2 + 1
    total = a256(max(n * 64 * h * w, n * 128 * h2 * w2) * 4) + a256(max(n * 64 * h2 * w2, n * 128 * h4 * w4) * 4) + a256(3 * 128 * 2 * 4)
    if training:
        for (ho, wo, th, cout) in ((h2, w2, 16, 64), (h2, w2, 8, 128), (h4, w4, 8, 128)):
            tiles = -(-ho // th) * -(-wo // 16)
            total += a256(cout * 2 * n * tiles * 8)
    return total


def _bn_array(eps=1e-5, momentum=0.1, ptr=1 << 20, nbt=True):
    from celebrity_image_denoiser_amd.discriminator import _BnArg

    arr = (_BnArg * 3)()
    for i in range(3):
        arr[i] = _BnArg(ptr, ptr, ptr, ptr, ptr if nbt else None, eps, momentum)
    return arr


def test_cabi_argument_errors_come_before_any_launch():
    L = _lib.lib()
    d = ctypes.c_void_p()
    assert L.cid_disc_create(ctypes.byref(d)) == 0
    try:
        fake = 1 << 20          # 256-byte aligned, never dereferenced: every call below must fail on the host
        ok_bn = _bn_array()

        def fwd(n=2, h=16, w=16, training=0, bn=ok_bn, x=fake, fmt=0, out=fake, ws=fake, ws_bytes=1 << 40):
            return L.cid_disc_forward(d, x, fmt, out, n, h, w, bn, training, ws, ws_bytes, None)

        # CID_ERR_INVALID
        assert fwd(x=None) == ERR_INVALID
        assert fwd(out=None) == ERR_INVALID
        assert fwd(bn=None) == ERR_INVALID
        assert fwd(ws=None) == ERR_INVALID
        assert fwd(fmt=7) == ERR_INVALID
        assert fwd(x=fake + 1) == ERR_INVALID                  # misaligned fp32 input
        assert fwd(out=fake + 2) == ERR_INVALID
        assert fwd(training=2) == ERR_INVALID
        for eps in (float("nan"), float("inf"), -1e-5):
            assert fwd(bn=_bn_array(eps=eps)) == ERR_INVALID
            assert fwd(bn=_bn_array(eps=eps), training=1) == ERR_INVALID
        for mom in (float("nan"), float("inf"), -0.5):
            assert fwd(bn=_bn_array(momentum=mom), training=1) == ERR_INVALID
        assert fwd(bn=_bn_array(nbt=False), training=1) == ERR_INVALID
        arr = _bn_array()
        arr[1].gamma = None
        assert fwd(bn=arr) == ERR_INVALID
        # momentum and num_batches_tracked are not read in eval mode; momentum=None is the sentinel
        assert fwd(bn=_bn_array(nbt=False, momentum=-0.5), ws_bytes=0) == ERR_WORKSPACE
        assert fwd(bn=_bn_array(momentum=_lib.CID_DISC_MOMENTUM_NONE), training=1, ws_bytes=0) == ERR_WORKSPACE
        # CID_ERR_SHAPE
        for n, h, w in ((0, 8, 8), (2, 0, 8), (2, 8, 0), (1, 65536, 32768)):
            assert fwd(n=n, h=h, w=w) == ERR_SHAPE
            assert fwd(n=n, h=h, w=w, training=1) == ERR_SHAPE
        for h, w in ((1, 1), (4, 4), (3, 2), (1, 4)):       # train mode with one value per channel: N = 1, H, W <= 4
            assert fwd(n=1, h=h, w=w, training=1) == ERR_SHAPE
            assert fwd(n=1, h=h, w=w, training=0, ws_bytes=0) == ERR_WORKSPACE
            assert _workspace_bytes(1, h, w, 1)[0] == ERR_SHAPE
        assert fwd(n=1, h=5, w=4, training=1, ws_bytes=0) == ERR_WORKSPACE   # H4 = 2
        assert fwd(n=2, h=1, w=1, training=1, ws_bytes=0) == ERR_WORKSPACE   # two values per channel
        # CID_ERR_WORKSPACE: too small (by one byte) or misaligned
        for training in (0, 1):
            rc, need = _workspace_bytes(3, 37, 53, training)
            assert rc == 0 and need == _expected_workspace(3, 37, 53, training)
            assert fwd(n=3, h=37, w=53, training=training, ws_bytes=need - 1) == ERR_WORKSPACE
            assert fwd(n=3, h=37, w=53, training=training, ws=fake + 16, ws_bytes=need) == ERR_WORKSPACE
            # everything valid but no weights uploaded: CID_ERR_STATE, still before any launch
            assert fwd(n=3, h=37, w=53, training=training, ws_bytes=need) == ERR_STATE
        assert _workspace_bytes(3, 37, 53, 1)[1] > _workspace_bytes(3, 37, 53, 0)[1]
        assert _workspace_bytes(2, 8, 8, 2)[0] == ERR_INVALID
        for shape in ((16, 256, 256), (256, 128, 128), (2, 1, 1)):
            for training in (0, 1):
                assert _workspace_bytes(*shape, training) == (0, _expected_workspace(*shape, training))
        # weights
        w = np.zeros((64, 3, 3, 3), np.float32)
        sh = (ctypes.c_int64 * 4)(*w.shape)
        assert L.cid_disc_set_weight(d, b"model.0.weight", w.ctypes.data, sh, 4) == 0
        assert L.cid_disc_set_weight(d, b"model.3.weight", w.ctypes.data, sh, 4) == ERR_KEY       # BatchNorm: per call
        assert L.cid_disc_set_weight(d, b"model.1.weight", w.ctypes.data, sh, 4) == ERR_KEY
        assert L.cid_disc_set_weight(d, b"model.2.weight", w.ctypes.data, sh, 4) == ERR_SHAPE
        assert L.cid_disc_upload_weights(d, fake, None) == ERR_STATE                            # nine tensors missing
        assert L.cid_disc_upload_weights(d, None, None) == ERR_INVALID
        assert L.cid_disc_packed_weights_bytes() >= (260929 - 2 * (64 + 128 + 128)) * 4   # the convolutions; BatchNorm per call
        # losses
        assert L.cid_disc_losses(None, fake, fake, 0, fake, 0, 2, 8, 8, fake, None) == ERR_INVALID
        assert L.cid_disc_losses(fake, fake, fake, 3, fake, 0, 2, 8, 8, fake, None) == ERR_INVALID
        assert L.cid_disc_losses(fake, fake, fake + 1, 0, fake, 0, 2, 8, 8, fake, None) == ERR_INVALID
        assert L.cid_disc_losses(fake, fake, fake, 0, fake, 1, 0, 8, 8, fake, None) == ERR_SHAPE
    finally:
        L.cid_disc_destroy(d)


def test_python_layer_rejects_bad_inputs():
    from celebrity_image_denoiser_amd.discriminator import DenoiseDiscriminator

    m = DenoiseDiscriminator()
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


# ------------------------------------------------------------------------------------------------------------------ GPU tests
def _module(kind, training):
    from celebrity_image_denoiser_amd.discriminator import DenoiseDiscriminator

    m = DenoiseDiscriminator()
    m.load_state_dict(weights(kind), strict=True)
    m.to(DEV)
    return m.train(training)


_REF = {}


def _ref_eval(kind, shape):
    """(float64 probabilities, float32 restatement's probabilities) of images(shape) in eval mode."""
    key = (kind, shape)
    if key not in _REF:
        x = images(*shape, first_index=sum(shape))[1]
        sd = weights(kind)
        _REF[key] = (restate(cast(sd, torch.float64), x.double(), False), restate(cast(sd, torch.float32), x, False).double())
    return _REF[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", WSETS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_eval_parity(kind, shape):
    u8, x = images(*shape, first_index=sum(shape))
    m = _module(kind, False)
    p = m(x.to(DEV))
    p_u8 = m(torch.from_numpy(u8).to(DEV))
    torch.cuda.synchronize()
    ref64, ref32 = _ref_eval(kind, shape)
    err = float((p.cpu().double() - ref64).abs().max())
    err_aten = float((ref32 - ref64).abs().max())
    print(f"eval {kind} {shape}: max|p - ref64| = {err:.2e}   ATen fp32 (CPU): {err_aten:.2e}")
    assert p.shape == (shape[0],) and p.dtype == torch.float32 and not p.requires_grad
    assert err <= TOL
    assert torch.equal(p_u8, p)   # a u8 batch and its normalised fp32 copy give identical bits
    if kind == "trained" and min(shape[1:]) >= 37:   # the calibrated weight set does not saturate the sigmoid
        assert float(ref64.min()) > 0.02 and float(ref64.max()) < 0.98


def _check_train(kind, shape, momentum, calls=2, make=images):
    """Train-mode parity of `calls` successive calls; make(n, h, w, first_index=...) -> (u8, fp32) batches (default: images)."""
    from celebrity_image_denoiser_amd import discriminator

    m = _module(kind, True)
    for i in BNS:
        m.model[i[0]].momentum = momentum
    sd = cast(weights(kind), torch.float64)
    for call in range(calls):
        u8, x = make(*shape, first_index=sum(shape) + 31 * call)
        p = m(x.to(DEV))
        torch.cuda.synchronize()
        ref = restate(sd, x.double(), True, momentum)
        err = float((p.cpu().double() - ref).abs().max())
        print(f"train {kind} {shape} momentum={momentum} call {call}: max|p - ref64| = {err:.2e}")
        assert err <= TOL
        for i, _ in BNS:
            for b in ("running_mean", "running_var"):
                got = getattr(m.model[i], b).cpu().double()
                want = sd[f"model.{i}.{b}"]
                bound = TOL * torch.clamp(want.abs(), min=1.0)
                assert bool(((got - want).abs() <= bound).all()), (i, b, float((got - want).abs().max()))
            assert int(m.model[i].num_batches_tracked) == int(sd[f"model.{i}.num_batches_tracked"])
    assert isinstance(m, discriminator.DenoiseDiscriminator)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", WSETS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_train_parity(kind, shape):
    _check_train(kind, shape, 0.1)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_train_parity_momentum_none(shape):
    _check_train("trained", shape, None)


@pytest.mark.gpu
def test_train_mode_matches_a_stock_module_in_float64():
    """The restatement's train-mode BatchNorm is the stock module's (buffers and counter included)."""
    stock = StockDiscriminator().double()
    stock.load_state_dict(cast(weights("trained"), torch.float64))
    stock.train()
    m = _module("trained", True)
    x = images(4, 37, 29, first_index=3)[1]
    p = m(x.to(DEV)).cpu().double()
    with torch.no_grad():
        ref = stock(x.double())
    assert float((p - ref).abs().max()) <= TOL
    for i, _ in BNS:
        for b in ("running_mean", "running_var"):
            got, want = getattr(m.model[i], b).cpu().double(), getattr(stock.model[i], b)
            assert bool(((got - want).abs() <= TOL * torch.clamp(want.abs(), min=1.0)).all())
        assert int(m.model[i].num_batches_tracked) == int(stock.model[i].num_batches_tracked) == 8


@pytest.mark.gpu
def test_one_value_per_channel_raises_in_train_mode():
    m = _module("default", True)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m(torch.zeros(1, 3, 4, 4, device=DEV))
    m.eval()
    assert m(torch.zeros(1, 3, 4, 4, device=DEV)).shape == (1,)


@pytest.mark.gpu
def test_eval_is_batch_independent_and_train_is_deterministic():
    u8, x = images(64, 40, 48, first_index=900)
    m = _module("trained", False)
    xg = x.to(DEV)
    batch = m(xg)
    alone = torch.cat([m(xg[i:i + 1]) for i in range(64)])
    assert torch.equal(batch, alone)
    assert torch.equal(m(torch.from_numpy(u8).to(DEV)), batch)
    # train: the same call twice from the same state gives the same bits, outputs and buffers
    runs = []
    for _ in range(2):
        t = _module("trained", True)
        p = t(xg)
        runs.append([p] + [getattr(t.model[i], b).clone() for i, _ in BNS for b in ("running_mean", "running_var", "num_batches_tracked")])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.gpu
def test_large_image_batch():
    """1440x1920: the layer-0 tensor of this batch passes 2^31 bytes (64-bit offsets)."""
    u8, x = images(4, 1440, 1920, first_index=77)
    m = _module("trained", False)
    xg = x.to(DEV)
    p = m(xg)
    p3 = m(xg[3:4])
    torch.cuda.synchronize()
    assert torch.equal(p[3:4], p3)
    ref32 = restate(cast(weights("trained"), torch.float32), x[3:4], False)
    err = float((p3.cpu() - ref32).abs().max())
    print(f"1440x1920: max|p - ATen fp32| = {err:.2e}")
    assert err <= TOL


@pytest.mark.gpu
def test_runs_on_a_non_default_stream():
    x = images(8, 64, 64, first_index=11)[1].to(DEV)
    ref_eval = _module("trained", False)(x)
    t0 = _module("trained", True)
    ref_train = t0(x)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m = _module("trained", False)
        pe = m(x)
        t = _module("trained", True)
        pt = t(x)
    s.synchronize()
    assert torch.equal(pe, ref_eval) and torch.equal(pt, ref_train)
    assert torch.equal(t.model[9].running_var, t0.model[9].running_var)


def _bce(p, target):
    return float(nn.BCELoss()(p.double(), torch.full_like(p.double(), target)))


@pytest.mark.gpu
@pytest.mark.parametrize("training", (False, True))
def test_trainer_losses(training):
    from celebrity_image_denoiser_amd.discriminator import trainer_losses

    clean_u8, clean = images(8, 64, 64, first_index=40)
    den = (clean + 0.05 * torch.sin(torch.arange(clean.numel(), dtype=torch.float32).reshape(clean.shape))).clamp(-1, 1)
    m = _module("trained", training)
    lo = trainer_losses(m, den.to(DEV), clean.to(DEV))
    # the probabilities the two calls saw (in train mode they depend only on the batch, not on the running buffers)
    pr, pf = m(clean.to(DEV)).cpu(), m(den.to(DEV)).cpu()
    sd = cast(weights("trained"), torch.float64)
    assert float((pr.double() - restate(cast(sd, torch.float64), clean.double(), training)).abs().max()) <= TOL
    content = float(nn.MSELoss()(den.double(), clean.double()))
    want = {"d_loss": _bce(pr, 1.0) + _bce(pf, 0.0), "adv_loss": _bce(pf, 1.0), "content_loss": content}
    want["g_loss"] = content + 0.001 * want["adv_loss"]
    for k, v in want.items():
        assert lo[k] == pytest.approx(v, rel=1e-6), k
    # a u8 clean batch is read as its normalised fp32 copy
    m.eval()
    a = trainer_losses(m, den.to(DEV), clean.to(DEV))
    b = trainer_losses(m, den.to(DEV), torch.from_numpy(clean_u8).to(DEV))
    assert a == b
    # no autograd history: the trainer's backward on D's output raises torch's own error
    p = m(clean.to(DEV))
    assert not p.requires_grad and p.grad_fn is None
    with pytest.raises(RuntimeError, match="does not require grad"):
        nn.BCELoss()(p, torch.ones_like(p)).backward()


@pytest.mark.gpu
@pytest.mark.parametrize("bias", (1e4, -1e4))
def test_trainer_losses_clamp_saturated_logs(bias):
    from celebrity_image_denoiser_amd.discriminator import trainer_losses

    m = _module("trained", False)
    with torch.no_grad():
        m.model[12].bias.fill_(bias)
    clean = images(4, 16, 16, first_index=2)[1].to(DEV)
    p = m(clean)
    assert bool((p == (1.0 if bias > 0 else 0.0)).all())
    lo = trainer_losses(m, clean * 0.5, clean)
    pc = p.cpu()
    want_d = _bce(pc, 1.0) + _bce(pc, 0.0)
    assert want_d == 100.0
    assert lo["d_loss"] == pytest.approx(want_d, rel=1e-12)
    assert lo["adv_loss"] == pytest.approx(_bce(pc, 1.0), abs=1e-12)


@pytest.mark.gpu
def test_evaluate_noise_types_with_a_discriminator():
    import celebrity_image_denoiser_amd as cid
    from celebrity_image_denoiser_amd import noise
    from celebrity_image_denoiser_amd.discriminator import trainer_losses

    model = cid.load(synth.make_state_dict("default"), device=DEV, strict=True)
    d = _module("trained", False)
    clean = torch.from_numpy(synth.clean_images_u8(12, 64, 64, first_index=300)).to(DEV)
    base = noise.evaluate_noise_types(model, clean, max_batch=5)
    got = noise.evaluate_noise_types(model, clean, max_batch=5, discriminator=d)
    for kind in noise.NOISE_TYPES:
        assert set(base[kind]) == {"psnr_noisy", "psnr", "ssim"}
        assert set(got[kind]) == set(base[kind]) | {"d_loss", "g_loss"}
        assert all(got[kind][k] == v for k, v in base[kind].items())
        sums = {"d_loss": 0.0, "g_loss": 0.0}
        for i0 in range(0, 12, 5):
            c = clean[i0:i0 + 5]
            noisy = noise.add_noise(c, kind, first_index=i0)
            lo = trainer_losses(d, model.forward_u8(noisy, out_u8=False), c)
            for k in sums:
                sums[k] += lo[k] * c.shape[0]
        assert got[kind]["d_loss"] == sums["d_loss"] / 12 and got[kind]["g_loss"] == sums["g_loss"] / 12
