"""The ESRGAN trainer's discriminator (Discriminator, reference backend/trainingcode/esrgan_code/models.py:36-71) on the GPU:
cid_esd_* (include/cid.h) and esrgan_disc.py against tests/esrgan_disc_oracle.py in float64.

Shapes (N, H, W), the smallest at which each mechanism can fail.  The MFMA layers conv2, conv3, conv4 run on tiles of 16, 8 and 4
output rows by 16 columns (k_esd_conv, PT = 4, 2, 1), so every one of them sees two tiles in each direction with the last partial:
  (2,1,1)      everything is padding, 512 features
  (4,7,5)      odd sides all the way down (4x3, 2x2, 1x1, 1x1)
  (3,16,16)    exact halving to 1x1
  (2,37,53)    partial tiles in every layer, 3x4 features per channel
  (1,70,130)   conv2's output is 18x33 (tile rows 16 + 2, tile columns 16 + 16 + 1), conv3's 9x17 (8 + 1, 16 + 1), conv4's 5x9 (4 + 1)
  (1,24,264)   conv4's output is 2x17: a second tile column of the last MFMA layer with one pixel in it
  (1,264,24)   conv4's output is 17x2: five tile rows of it, the last with one pixel
Every stage a1 ... a4 (read from the workspace at the offsets include/cid.h documents) and the logits are within
1e-5 * max(1, max|ref64|) of the float64 restatement, the project's bound; the oracle asserts on the CPU that the float32
restatement itself is within a tenth of that for every stage of every case and that the "trained" logits lie in (-6, 6)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib
from celebrity_image_denoiser_amd.esrgan_disc import ESRGANDiscriminator, esrgan_trainer_losses

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import esrgan_disc_oracle as oracle  # noqa: E402
from esrgan_disc_oracle import TOL, bce_with_logits, case, weights  # noqa: E402
from esrgan_disc_oracle import expected_workspace as _expected_workspace  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(2, 1, 1), (4, 7, 5), (3, 16, 16), (2, 37, 53), (1, 70, 130), (1, 24, 264), (1, 264, 24)]
BATCH = (8, 37, 53)
ids = lambda s: "x".join(map(str, s))   # noqa: E731


def _module(kind, hw, sd=None):
    m = ESRGANDiscriminator((3, hw[0], hw[1]))
    m.load_state_dict(weights(kind, hw) if sd is None else sd, strict=True)
    return m.to(DEV)


def _stages_at_documented_offsets(m, shape):
    """a1 ... a4 of the module's last forward, read from its workspace by the formula of include/cid.h."""
    n, h, w = shape
    offs, total = _expected_workspace(n, h, w)
    assert m._ws.numel() >= total
    out = []
    for off, c in zip(offs, (64, 128, 256, 512)):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        flat = m._ws[off:off + 4 * n * c * h * w].view(torch.float32)
        out.append(oracle.c8_to_nchw(flat, n, c, h, w).cpu())
    return out


@pytest.mark.parametrize("kind", oracle.WSETS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_parity_stage_by_stage(kind, shape):
    u8, x, st64, lg64 = case(kind, shape)
    m = _module(kind, shape[1:])
    out = m(x.to(DEV))
    torch.cuda.synchronize()
    assert out.shape == (shape[0], 1) and out.dtype == torch.float32 and not out.requires_grad and out.grad_fn is None
    got = _stages_at_documented_offsets(m, shape) + [out.cpu()]
    errs = []
    for name, g, ref in zip(("a1", "a2", "a3", "a4", "logits"), got, st64 + [lg64]):
        assert g.shape == ref.shape, name
        errs.append((name, float((g.double() - ref).abs().max()), TOL * max(1.0, float(ref.abs().max()))))
    print(f"{kind} {shape}: " + "  ".join(f"{n} {e:.2e} (bound {b:.2e})" for n, e, b in errs)
          + f"  logits in [{float(lg64.min()):.3f}, {float(lg64.max()):.3f}]")
    for name, err, bound in errs:
        assert err <= bound, (name, err, bound)
    # a uint8 batch and its fp32 copy give equal bits, stage by stage
    out_u8 = m(torch.from_numpy(u8).to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(out_u8, out)
    assert all(torch.equal(a, b) for a, b in zip(_stages_at_documented_offsets(m, shape), got[:4]))
    assert all(torch.equal(a, b) for a, b in zip(m.stages(shape[0]), [g.to(DEV) for g in got[:4]]))


def test_matches_a_stock_module_and_train_mode_is_eval_mode():
    shape = (2, 37, 53)
    _, x, _, lg64 = case("trained", shape)
    stock = oracle.StockESRGANDiscriminator((3, 37, 53)).double()
    m = _module("trained", shape[1:])
    stock.load_state_dict({k: v.double() for k, v in m.state_dict().items()}, strict=True)
    with torch.no_grad():
        ref = stock(x.double())
    assert float((ref - lg64).abs().max()) <= 1e-12   # the restatement is the stock module
    a = m.train()(x.to(DEV))
    b = m.eval()(x.to(DEV))
    assert torch.equal(a, b) and float((a.cpu().double() - ref).abs().max()) <= TOL * max(1.0, float(ref.abs().max()))
    assert torch.ones_like(a).shape == (2, 1)
    # no autograd history: the trainer's backward on D's output raises torch's own error
    p = m(x.to(DEV).requires_grad_(True))
    assert not p.requires_grad and p.grad_fn is None
    with pytest.raises(RuntimeError, match="does not require grad"):
        torch.nn.BCEWithLogitsLoss()(p, torch.ones_like(p)).backward()


def test_batch_independence():
    """Image i of a batch gives the bits it gives alone and at another position."""
    _, x, _, lg64 = case("trained", BATCH)
    xg = x.to(DEV)
    m = _module("trained", BATCH[1:])
    batch = m(xg)
    stages = m.stages(BATCH[0])
    assert float((batch.cpu().double() - lg64).abs().max()) <= TOL * max(1.0, float(lg64.abs().max()))
    for i in (0, 3, 7):
        alone = m(xg[i:i + 1])
        assert torch.equal(alone, batch[i:i + 1]), i
        assert all(torch.equal(a[0], b[i]) for a, b in zip(m.stages(1), stages)), i
    moved = m(torch.cat([xg[5:6], xg[7:8], xg[0:1], xg[3:4], xg[3:4]]))   # images 7, 0, 3 at positions 1, 2, 3 (and 4)
    assert torch.equal(moved[:, 0], batch[[5, 7, 0, 3, 3], 0])


@pytest.mark.parametrize("shape", [(4, 7, 5), (1, 70, 130)], ids=ids)
def test_workspace_hygiene(shape):
    """A workspace full of NaN bytes gives the same bits, and nothing is written past cid_esd_workspace_bytes."""
    L = _lib.lib()
    _, x, _, _ = case("trained", shape)
    xg = x.to(DEV)
    m = _module("trained", shape[1:])
    want = m(xg)
    want_stages = m.stages(shape[0])
    need = ctypes.c_size_t()
    assert L.cid_esd_workspace_bytes(*shape, ctypes.byref(need)) == 0 and need.value == _expected_workspace(*shape)[1]
    guard = 4096
    ws = torch.full((need.value + guard,), 0xFF, dtype=torch.uint8, device=DEV)   # 0xFFFFFFFF is a NaN in fp32
    assert ws.data_ptr() % 256 == 0 and need.value % 256 == 0
    out = torch.empty((shape[0], 1), dtype=torch.float32, device=DEV)
    _lib.check_abi("esd", m._cid, L.cid_esd_forward(m._cid, xg.data_ptr(), 0, out.data_ptr(), *shape, ws.data_ptr(), need.value, None))
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert bool((ws[need.value:] == 0xFF).all())
    m._ws = ws   # read the stages of that call
    assert all(torch.equal(a, b) for a, b in zip(m.stages(shape[0]), want_stages))


def test_reload_of_a_second_weight_set_equals_a_fresh_module():
    shape = (2, 37, 53)
    x = case("trained", shape)[1].to(DEV)
    m = _module("default", shape[1:])
    first = m(x)
    second = weights("trained", shape[1:], seed=0xABCD)
    m.load_state_dict(second, strict=True)
    got = m(x)
    fresh = _module("trained", shape[1:], sd=second)(x)
    assert torch.equal(got, fresh) and not torch.equal(got, first)
    with torch.no_grad():                       # an in-place parameter change is repacked too
        m.fc.bias.add_(1.0)
    moved = m(x)
    assert float((moved - got - 1.0).abs().max()) < 1e-6 and not torch.equal(moved, got)


def test_launch_split_above_65535_images():
    """65,537 images of 1x1: image 0, 65,534, 65,535 and 65,536 on both sides of the launch seam equal the same images run alone."""
    n = 65537
    u8 = (np.arange(n * 3, dtype=np.int64) * 2654435761 % 251).astype(np.uint8).reshape(n, 1, 1, 3)
    x = torch.from_numpy(u8).to(DEV)
    m = _module("trained", (1, 1))
    out = m(x)
    assert out.shape == (n, 1) and bool(torch.isfinite(out).all())
    seam = [0, 65534, 65535, 65536]
    for i in seam:
        assert torch.equal(m(x[i:i + 1].contiguous()), out[i:i + 1]), i
    xf = torch.from_numpy(u8[seam]).permute(0, 3, 1, 2).double() / 255.0
    ref = oracle.restate(oracle.cast(weights("trained", (1, 1)), torch.float64), xf)[1]
    assert float((out[seam].cpu().double() - ref).abs().max()) <= TOL
    # the seam images are told apart: their logits differ pairwise by more than ten float32 steps, so a neighbour's value would show
    gaps = (ref - ref.t()).abs() + torch.eye(len(seam), dtype=torch.float64)
    assert float(gaps.min()) > 10 * 2.0 ** -24


def _want_losses(real, fake):
    r, f = real.cpu().numpy().reshape(-1), fake.cpu().numpy().reshape(-1)
    return bce_with_logits(r, 1.0).mean(), bce_with_logits(f, 0.0).mean(), bce_with_logits(f, 1.0).mean()


def test_cid_esd_losses_against_the_float64_restatement():
    L = _lib.lib()
    for n, seed in ((1, 3), (6, 5), (1500, 7)):
        g = torch.Generator().manual_seed(seed)
        real = (torch.randn(n, generator=g) * 3.0).to(DEV)
        fake = (torch.randn(n, generator=g) * 3.0).to(DEV)
        if n == 6:   # the stable form at its asymptotes
            real[:4] = torch.tensor([40.0, -40.0, 0.0, 1e-8], device=DEV)
            fake[:4] = torch.tensor([-40.0, 40.0, 1e-8, 0.0], device=DEV)
        out = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
        assert L.cid_esd_losses(real.data_ptr(), fake.data_ptr(), n, out.data_ptr(), None) == 0
        got, want = out.cpu().tolist(), _want_losses(real, fake)
        print(f"N={n}: got {got} want {list(want)}")
        for g_, w_ in zip(got, want):
            assert np.isfinite(g_) and g_ == pytest.approx(w_, rel=1e-6)
        ref = [float(torch.nn.BCEWithLogitsLoss()(t.cpu().double(), torch.full((n,), y, dtype=torch.float64)))
               for t, y in ((real, 1.0), (fake, 0.0), (fake, 1.0))]
        assert got == pytest.approx(ref, rel=1e-6)


def test_esrgan_trainer_losses():
    u8, clean, _, _ = case("trained", BATCH)
    den = (clean + 0.05 * torch.sin(torch.arange(clean.numel(), dtype=torch.float32).reshape(clean.shape))).clamp(0, 1)
    m = _module("trained", BATCH[1:])
    lo = esrgan_trainer_losses(m, den.to(DEV), clean.to(DEV))
    assert set(lo) == {"d_loss", "gan_loss", "pixel_loss", "g_loss"}
    assert all(v.device.type == "cuda" and v.dtype == torch.float64 and v.dim() == 0 for v in lo.values())   # they stay on the device
    real, fake = m(clean.to(DEV)), m(den.to(DEV))
    real1, fake0, fake1 = _want_losses(real, fake)   # the BCE arithmetic itself, on the logits the device produced
    pixel = float(((den.double() - clean.double()) ** 2).mean())
    want = {"d_loss": 0.5 * (real1 + fake0), "gan_loss": fake1, "pixel_loss": pixel, "g_loss": pixel + 1e-3 * fake1}
    for k, v in want.items():
        print(f"{k}: got {float(lo[k])!r} want {v!r}")
        assert float(lo[k]) == pytest.approx(v, rel=1e-6), k
    assert float(lo["g_loss"]) == float(lo["pixel_loss"]) + 1e-3 * float(lo["gan_loss"])   # the module's own arithmetic, to the bit
    assert float(lo["d_loss"]) != float(lo["gan_loss"]) and float(lo["pixel_loss"]) > 0.0
    # against the trainer's own lines in float64 on the float64 restatement's logits
    sd64 = oracle.cast(weights("trained", BATCH[1:]), torch.float64)
    r64, f64 = oracle.restate(sd64, clean.double())[1], oracle.restate(sd64, den.double())[1]
    bce = torch.nn.BCEWithLogitsLoss()
    d_ref = 0.5 * (bce(r64, torch.ones_like(r64)) + bce(f64, torch.zeros_like(f64)))
    assert float(lo["d_loss"]) == pytest.approx(float(d_ref), abs=2e-5)
    # a uint8 clean batch is read as its fp32 copy
    b = esrgan_trainer_losses(m, den.to(DEV), torch.from_numpy(u8).to(DEV))
    assert all(torch.equal(lo[k], b[k]) for k in lo)


def test_saturated_logits_stay_finite():
    """fc.bias = +-40: the stable form gives 40 and about e^-40, not inf and 0."""
    shape = (4, 7, 5)
    x = case("trained", shape)[1].to(DEV)
    for bias in (40.0, -40.0):
        m = _module("trained", shape[1:])
        with torch.no_grad():
            m.fc.bias.fill_(bias)
        logits = m(x)
        assert bool(((logits - bias).abs() < 1.0).all())
        lo = esrgan_trainer_losses(m, x * 0.5, x)
        real1, fake0, fake1 = _want_losses(logits, m(x * 0.5))
        assert all(bool(torch.isfinite(v)) for v in lo.values())
        assert float(lo["d_loss"]) == pytest.approx(0.5 * (real1 + fake0), rel=1e-6) and float(lo["d_loss"]) > 19.0
        assert float(lo["gan_loss"]) == pytest.approx(fake1, rel=1e-6)
        assert (float(lo["gan_loss"]) < 1e-15) == (bias > 0)


def test_rejections_leave_the_module_usable():
    shape = (2, 37, 53)
    x = case("trained", shape)[1].to(DEV)
    m = _module("trained", shape[1:])
    want = m(x)
    with pytest.raises(RuntimeError, match="built for input_shape"):
        m(torch.zeros(2, 3, 37, 54, device=DEV))
    with pytest.raises(RuntimeError, match="built for input_shape"):
        m(torch.zeros(2, 53, 37, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="float32"):
        m(x.double())
    with pytest.raises(RuntimeError, match="float32"):
        m(x.half())
    with pytest.raises(RuntimeError, match="contiguous"):
        m(torch.zeros(2, 37, 53, 3, device=DEV).permute(0, 3, 1, 2))
    with pytest.raises(RuntimeError, match="contiguous"):
        m(torch.zeros(2, 37, 53, 6, dtype=torch.uint8, device=DEV)[..., ::2])
    with pytest.raises(RuntimeError, match=r"\[N,3,H,W\]"):
        m(x[0])
    assert torch.equal(m(x), want)   # the next valid call still gives the right bits
    # the C ABI refuses a wrong size itself, before any launch
    out = torch.full((2, 1), 7.0, device=DEV)
    rc = _lib.lib().cid_esd_forward(m._cid, x.data_ptr(), 0, out.data_ptr(), 2, 53, 37, m._ws.data_ptr(), m._ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == 2 and bool((out == 7.0).all())
    assert torch.equal(m(x), want)


def test_runs_on_a_non_default_stream():
    shape = (2, 37, 53)
    x = case("trained", shape)[1].to(DEV)
    want = _module("trained", shape[1:])(x)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = _module("trained", shape[1:])(x)
    s.synchronize()
    assert torch.equal(got, want)
