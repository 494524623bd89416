"""The SRGAN trainer's discriminator (SRGANDiscriminator, reference backend/trainingcode/srgan_code/sr_ganTrainGNew.py:54-80) on the GPU:
cid_srd_* (include/cid.h) and srgan_disc.py against tests/srgan_disc_oracle.py in float64.

Shapes (N, H, W), the smallest at which each mechanism can fail: (2,1,1) everything is padding, H4 = W4 = 1; (4,7,5) odd sides and
partial tiles everywhere; (8,37,53) H4 = 10, two tile rows of model.11's launch with the second partial; (3,41,70) H4 = 11, W4 = 18,
two tile rows and two tile columns of it, both partial.  Tolerances are those of tests/test_discriminator.py: 1e-5 absolute on
probabilities, 1e-5 * max(1, |want|) on running buffers."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from celebrity_image_denoiser_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import srgan_disc_oracle as oracle  # noqa: E402
from srgan_disc_oracle import BNS, cast, images, restate, weights  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
SHAPES = [(2, 1, 1), (4, 7, 5), (8, 37, 53), (3, 41, 70)]
WSETS = oracle.WSETS
BUFFERS = ("running_mean", "running_var", "num_batches_tracked")
ids = lambda s: "x".join(map(str, s))   # noqa: E731


def _module(kind, training, sd=None):
    from celebrity_image_denoiser_amd.srgan_disc import SRGANDiscriminator

    m = SRGANDiscriminator()
    m.load_state_dict(weights(kind) if sd is None else sd, strict=True)
    m.to(DEV)
    return m.train(training)


def _buffers(m):
    return [getattr(m.model[i], b).clone() for i, _ in BNS for b in BUFFERS]


_BATCH, _REF = {}, {}


def _batch(shape):
    """(uint8, fp32) CPU batch of a shape: drawn once, never modified."""
    if shape not in _BATCH:
        _BATCH[shape] = images(*shape, first_index=sum(shape))
    return _BATCH[shape]


def _ref_eval(kind, shape):
    """float64 eval-mode probabilities of _batch(shape): computed once, shared, never modified."""
    if (kind, shape) not in _REF:
        _REF[(kind, shape)] = restate(cast(weights(kind), torch.float64), _batch(shape)[1].double(), False)
    return _REF[(kind, shape)]


@pytest.mark.parametrize("kind", WSETS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_eval_parity(kind, shape):
    u8, x = _batch(shape)
    m = _module(kind, False)
    before = _buffers(m)
    p = m(x.to(DEV))
    p_u8 = m(torch.from_numpy(u8).to(DEV))
    torch.cuda.synchronize()
    ref64 = _ref_eval(kind, shape)
    err = float((p.cpu().double() - ref64).abs().max())
    print(f"eval {kind} {shape}: max|p - ref64| = {err:.2e}   p in [{float(ref64.min()):.3f}, {float(ref64.max()):.3f}]")
    assert p.shape == (shape[0],) and p.dtype == torch.float32 and not p.requires_grad and p.grad_fn is None
    assert err <= TOL
    assert torch.equal(p_u8, p)   # a u8 batch and its normalised fp32 copy give identical bits
    assert all(torch.equal(a, b) for a, b in zip(before, _buffers(m)))   # eval mode leaves the buffers alone
    if kind == "trained":         # the calibrated weight set does not saturate the sigmoid
        assert float(ref64.min()) > 0.02 and float(ref64.max()) < 0.98


def _check_buffers(m, sd):
    for i, _ in BNS:
        for b in ("running_mean", "running_var"):
            got = getattr(m.model[i], b).cpu().double()
            want = sd[f"model.{i}.{b}"]
            bound = TOL * torch.clamp(want.abs(), min=1.0)
            assert bool(((got - want).abs() <= bound).all()), (i, b, float((got - want).abs().max()))
        assert int(m.model[i].num_batches_tracked) == int(sd[f"model.{i}.num_batches_tracked"])


_TRAIN = {}
CONDITION = TOL / 10   # what the float32 restatement itself may differ from the float64 one for a draw to be used in train mode


def _train_case(kind, shape, momentum, calls=2):
    """[(fp32 batch, float64 probabilities, float64 state after the call)] of `calls` successive train-mode calls: computed once,
    shared, never modified.

    Which images a call gets is decided by the reference alone.  A BatchNorm over few values is ill-conditioned: over the two values
    of an N = 2, 1x1 batch it is y = beta +- gamma * d / sqrt(d^2 + 4 eps) with d the difference of the two, a step of slope
    gamma / (2 sqrt(eps)) = 158 gamma around d = 0, and four of them follow one another.  There the float32 rounding of a convolution
    output moves the probability by more than TOL whoever computes it: on the first draw of (2,1,1) with the "trained" set the
    restatement in float32 (ATen on the CPU) is 1.13e-5 from the float64 one and the HIP forward 3.16e-5, and over twelve draws the
    float32 restatement ranges from 6.5e-8 to 9.9e-5.  So a call takes the first draw of a fixed sequence on which the float32
    restatement is within CONDITION of the float64 one: the reference's own float32 error leaves nine tenths of TOL to the code
    under test.  At the three larger shapes every first draw qualifies."""
    key = (kind, shape, momentum)
    if key not in _TRAIN:
        sd64, sd32 = cast(weights(kind), torch.float64), cast(weights(kind), torch.float32)
        out = []
        for call in range(calls):
            for draw in range(16):
                x = images(*shape, first_index=sum(shape) + 31 * call + 1000 * draw)[1]
                t64, t32 = cast(sd64, torch.float64), cast(sd32, torch.float32)
                p64, p32 = restate(t64, x.double(), True, momentum), restate(t32, x, True, momentum)
                own = float((p64 - p32.double()).abs().max())
                if own <= CONDITION:
                    break
            else:
                raise AssertionError(f"no well-conditioned draw for {key}")
            print(f"train {kind} {shape} momentum={momentum} call {call}: draw {draw}, float32 restatement {own:.2e} from float64")
            sd64, sd32 = t64, t32
            out.append((x, p64, cast(t64, torch.float64)))
        _TRAIN[key] = out
    return _TRAIN[key]


def _check_train(kind, shape, momentum, calls=2):
    """Train-mode parity of `calls` successive calls: probabilities, then the buffers and counters of all four BatchNorms."""
    m = _module(kind, True)
    for i, _ in BNS:
        m.model[i].momentum = momentum
    for call, (x, ref, sd) in enumerate(_train_case(kind, shape, momentum, calls)):
        p = m(x.to(DEV))
        torch.cuda.synchronize()
        err = float((p.cpu().double() - ref).abs().max())
        print(f"train {kind} {shape} momentum={momentum} call {call}: max|p - ref64| = {err:.2e}")
        assert err <= TOL
        _check_buffers(m, sd)
    assert int(m.model[12].num_batches_tracked) == int(weights(kind)["model.12.num_batches_tracked"]) + calls


@pytest.mark.parametrize("kind", WSETS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_train_parity(kind, shape):
    _check_train(kind, shape, 0.1)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_train_parity_momentum_none(shape):
    _check_train("trained", shape, None)


def test_train_mode_matches_a_stock_module_in_float64():
    """The restatement's train-mode BatchNorm is the stock module's (buffers and counter included), through load_state_dict."""
    stock = oracle.StockSRGANDiscriminator().double()
    stock.load_state_dict(cast(weights("trained"), torch.float64))
    stock.train()
    m = _module("trained", True)
    x = images(4, 37, 29, first_index=3)[1]
    p = m(x.to(DEV)).cpu().double()
    with torch.no_grad():
        ref = stock(x.double())
    assert float((p - ref).abs().max()) <= TOL
    _check_buffers(m, stock.state_dict())
    assert all(int(m.model[i].num_batches_tracked) == 8 for i, _ in BNS)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 2, 2)], ids=ids)
def test_one_value_per_channel_raises_in_train_mode_and_launches_nothing(shape):
    m = _module("trained", True)
    before = _buffers(m)
    x = torch.zeros(shape[0], 3, shape[1], shape[2], device=DEV)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m(x)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m(torch.zeros(shape[0], shape[1], shape[2], 3, dtype=torch.uint8, device=DEV))
    # the C ABI refuses the same call itself (CID_ERR_SHAPE with PyTorch's wording), before any launch
    from celebrity_image_denoiser_amd.discriminator import bn_args

    out = torch.full((1,), 7.0, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    rc = _lib.lib().cid_srd_forward(m._cid, x.data_ptr(), 0, out.data_ptr(), *shape, bn_args(m.model, (3, 6, 9, 12), torch.device(DEV)), 1,
                                    ws.data_ptr(), ws.numel(), None)
    assert rc == 2 and _lib.lib().cid_srd_last_error(m._cid) == b"Expected more than 1 value per channel when training"
    torch.cuda.synchronize()
    assert float(out) == 7.0 and not bool(ws.any())
    assert all(torch.equal(a, b) for a, b in zip(before, _buffers(m)))
    m.eval()
    assert m(x).shape == (1,)


def test_eval_is_batch_independent():
    """Image i alone, and image i at another position of a larger batch, give the same bits."""
    shape = (3, 41, 70)
    xg = _batch(shape)[1].to(DEV)
    m = _module("trained", False)
    batch = m(xg)
    alone = torch.cat([m(xg[i:i + 1]) for i in range(shape[0])])
    assert torch.equal(batch, alone)
    more = images(4, 41, 70, first_index=7)[1].to(DEV)
    larger = m(torch.cat([more[:2], xg[2:3], more[2:], xg[0:2]]))   # 7 images: image 2 at position 2, images 0 and 1 at 5 and 6
    assert torch.equal(larger[2], batch[2]) and torch.equal(larger[5:7], batch[0:2])
    assert float((batch.cpu().double() - _ref_eval("trained", shape)).abs().max()) <= TOL


def test_train_is_deterministic():
    """The same call twice from the same state gives the same bits, outputs and buffers."""
    xg = _batch((3, 41, 70))[1].to(DEV)
    runs = []
    for _ in range(2):
        t = _module("trained", True)
        runs.append([t(xg)] + _buffers(t))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert not torch.equal(runs[0][-2], weights("trained")["model.12.running_var"].to(DEV))   # and the buffers did move


@pytest.mark.parametrize("zeroed", ("upper", "lower"))
def test_channel_halves_of_layer_11(zeroed):
    """model.11 runs as two 128-channel halves.  With one half's output channels, and what model.12 and model.15 make of them,
    zeroed in the restatement and in the module alike, parity still holds: a half that lands at the other half's offset, reads the
    other half's weights or sums into the other half's statistics does not survive either case."""
    shape = (3, 41, 70)
    half = slice(128, 256) if zeroed == "upper" else slice(0, 128)
    sd = weights("trained")
    for k in ("model.11.weight", "model.11.bias", "model.12.weight", "model.12.bias"):
        sd[k][half] = 0.0
    sd["model.15.weight"][:, half] = 0.0
    x = _batch(shape)[1]
    ref = restate(cast(sd, torch.float64), x.double(), False)
    full = _ref_eval("trained", shape)
    assert float((ref - full).abs().max()) > 100 * TOL   # the zeroed half mattered
    p = _module("trained", False, sd=sd)(x.to(DEV)).cpu().double()
    err = float((p - ref).abs().max())
    print(f"{zeroed} half zeroed: max|p - ref64| = {err:.2e}")
    assert err <= TOL


def test_launch_split_above_65535_images():
    """N = 65,535 + 9 images of 1x1 in eval mode: the images on both sides of the launch seam equal the same images run alone."""
    n = 65535 + 9
    u = synth.hash_uniform(20261019, 11, n * 3).astype(np.float32)
    x = torch.from_numpy(2.0 * u - 1.0).reshape(n, 3, 1, 1).to(DEV)
    m = _module("trained", False)
    p = m(x)
    seam = [0, 1, 65534, 65535, 65536, n - 1]
    for i in seam:
        assert torch.equal(m(x[i:i + 1]), p[i:i + 1]), i
    assert bool(torch.isfinite(p).all())
    ref = restate(cast(weights("trained"), torch.float64), x[seam].cpu().double(), False)
    assert float((p[seam].cpu().double() - ref).abs().max()) <= TOL
    # the seam images are told apart: their probabilities differ pairwise by more than ten float32 steps, so a neighbour's value would show
    gaps = (ref[:, None] - ref[None, :]).abs() + torch.eye(len(seam), dtype=torch.float64)
    assert float(gaps.min()) > 10 * 2.0 ** -24


def test_runs_on_a_non_default_stream():
    x = _batch((8, 37, 53))[1].to(DEV)
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
    assert all(torch.equal(a, b) for a, b in zip(_buffers(t), _buffers(t0)))


@pytest.mark.parametrize("training", (0, 1))
@pytest.mark.parametrize("shape", [(4, 7, 5), (3, 41, 70)], ids=ids)
def test_workspace_hygiene(shape, training):
    """A workspace full of NaN bytes gives the same result, and nothing is written past cid_srd_workspace_bytes."""
    from celebrity_image_denoiser_amd.discriminator import bn_args

    L = _lib.lib()
    x = _batch(shape)[1].to(DEV)
    want_m = _module("trained", bool(training))
    want = want_m(x)
    m = _module("trained", bool(training))
    m.pack_weights()
    need = ctypes.c_size_t()
    assert L.cid_srd_workspace_bytes(*shape, training, ctypes.byref(need)) == 0
    guard = 4096
    ws = torch.full((need.value + guard,), 0xFF, dtype=torch.uint8, device=DEV)   # 0xFFFFFFFF is a NaN in fp32 and in fp64
    assert ws.data_ptr() % 256 == 0 and need.value % 256 == 0
    out = torch.empty(shape[0], dtype=torch.float32, device=DEV)
    _lib.check_srd(m._cid, L.cid_srd_forward(m._cid, x.data_ptr(), 0, out.data_ptr(), *shape, bn_args(m.model, (3, 6, 9, 12), torch.device(DEV)),
                                             training, ws.data_ptr(), need.value, None))
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert bool((ws[need.value:] == 0xFF).all())
    assert all(torch.equal(a, b) for a, b in zip(_buffers(m), _buffers(want_m)))


def _bce(p, target):
    return float(nn.BCELoss()(p.double(), torch.full_like(p.double(), target)))


@pytest.mark.parametrize("training", (False, True))
def test_srgan_trainer_losses(training):
    from celebrity_image_denoiser_amd.srgan_disc import srgan_trainer_losses

    hr_u8, hr = _batch((8, 37, 53))
    fake = (hr + 0.05 * torch.sin(torch.arange(hr.numel(), dtype=torch.float32).reshape(hr.shape))).clamp(-1, 1)
    m = _module("trained", training)
    lo = srgan_trainer_losses(m, fake.to(DEV), hr.to(DEV))
    assert set(lo) == {"d_loss", "adv_loss", "content_loss", "g_loss"} and lo["content_loss"] is None and lo["g_loss"] is None
    # against the float64 restatement (in train mode the probabilities depend only on the batch, not on the running buffers)
    sd = weights("trained")
    pr = restate(cast(sd, torch.float64), hr.double(), training)
    pf = restate(cast(sd, torch.float64), fake.double(), training)
    got_r, got_f = m(hr.to(DEV)).cpu(), m(fake.to(DEV)).cpu()
    assert float((got_r.double() - pr).abs().max()) <= TOL and float((got_f.double() - pf).abs().max()) <= TOL
    # the BCE arithmetic itself, on the probabilities the device produced
    want = {"d_loss": _bce(got_r, 1.0) + _bce(got_f, 0.0), "adv_loss": _bce(got_f, 1.0)}
    for k, v in want.items():
        print(f"{k}: got {lo[k]!r} want {v!r} float64 restatement {(_bce(pr, 1.0) + _bce(pf, 0.0)) if k == 'd_loss' else _bce(pf, 1.0)!r}")
        assert lo[k] == pytest.approx(v, rel=1e-6), k
    # a u8 hr batch is read as its normalised fp32 copy
    m.eval()
    a = srgan_trainer_losses(m, fake.to(DEV), hr.to(DEV))
    b = srgan_trainer_losses(m, fake.to(DEV), torch.from_numpy(hr_u8).to(DEV))
    assert a == b
    # no autograd history: the trainer's backward on D's output raises torch's own error
    p = m(hr.to(DEV).requires_grad_(True))
    assert not p.requires_grad and p.grad_fn is None
    with pytest.raises(RuntimeError, match="does not require grad"):
        nn.BCELoss()(p, torch.ones_like(p)).backward()


@pytest.mark.parametrize("bias", (1e4, -1e4))
def test_srgan_trainer_losses_clamp_saturated_logs(bias):
    from celebrity_image_denoiser_amd.srgan_disc import srgan_trainer_losses

    m = _module("trained", False)
    with torch.no_grad():
        m.model[17].bias.fill_(bias)
    hr = _batch((4, 7, 5))[1].to(DEV)
    p = m(hr)
    assert bool((p == (1.0 if bias > 0 else 0.0)).all())
    lo = srgan_trainer_losses(m, hr * 0.5, hr)
    pc = p.cpu()
    want_d = _bce(pc, 1.0) + _bce(pc, 0.0)
    assert want_d == 100.0
    assert lo["d_loss"] == 100.0
    assert lo["adv_loss"] == (0.0 if bias > 0 else 100.0) == _bce(pc, 1.0)


def test_srgan_trainer_losses_with_the_vgg_content_loss():
    from celebrity_image_denoiser_amd.lpips import load_vgg_loss
    from celebrity_image_denoiser_amd.srgan_disc import srgan_trainer_losses

    np_sd = synth.vgg_loss_state_dict(synth.make_lpips_state_dict("default", net="vgg"))
    vgg = load_vgg_loss({k: torch.from_numpy(v) for k, v in np_sd.items()}, device=DEV)
    hr = images(4, 16, 16, first_index=21)[1]
    fake = (hr * 0.9 + 0.03).to(DEV)
    hr = hr.to(DEV)
    m = _module("trained", False)
    lo = srgan_trainer_losses(m, fake, hr, vgg_loss=vgg)
    base = srgan_trainer_losses(m, fake, hr)
    assert lo["content_loss"] == float(vgg(fake, hr)) and lo["content_loss"] > 0.0
    assert (lo["d_loss"], lo["adv_loss"]) == (base["d_loss"], base["adv_loss"])
    assert lo["g_loss"] == lo["content_loss"] + 0.001 * lo["adv_loss"]
