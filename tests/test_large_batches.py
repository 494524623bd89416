"""Batches past 65,535 images: a grid's y dimension holds at most 65,535 images, so cid_disc_forward(_saved), cid_disc_backward,
cid_backward, cid_quality, cid_esr_forward and cid_sr_forward loop over launches of 65,535 images on the host (every kernel adds
the launch's first image to its block index), and cid_add_noise and cid_resize loop over the rest inside the kernel.  Every case
here runs N = 65,535 + 9 images of the smallest size its entry point accepts and makes two checks:

  (i)  every image's result in the one call is bit-equal to its result in two calls of at most 65,535 images, on [0, 32772) and
       [32772, N), compared on the device;
  (ii) the SEAM images (both ends of the batch, of the first launch and of the two smaller calls) match the high-precision CPU
       reference of the family's own test file at that file's own tolerance, which anchors (i).

All images are distinct (a seeded numpy generator; the first pixel of image n carries a 24-bit code unique to n), so an image read
or written at another image's index shows.  Gradients with respect to parameters sum over the batch: there grad_out (grad_prob) is
zero except on SEAM, zero rows contribute exact zeros, and the true gradient is that of the 10-image batch x[SEAM].  Train-mode
BatchNorm couples the whole batch; at 1 x 1 the whole batch runs through the float64 reference.

The train-mode entry points of the server's generators and of the SRGAN trainer (cid_esr_forward_train, cid_sr_forward_train,
cid_sr_forward_saved + cid_sr_backward), whose launches carry the first image into slab rows and reductions as well, take the same
split in tests/test_train_batches.py, over two seams (N = 2 * 65,535 + 9) and with the whole batch held to float64.

This file covers the axis N alone: at these sizes every tensor is a few MiB.  The large-tensor axis (an activation tensor of
cid_esr_*, cid_sr_*, cid_cg_*, cid_srd_* or cid_esd_* past 2^31 elements, where a narrow offset shows) is tests/test_wide_offsets.py's.

MS-SSIM is defined for min(H, W) > 160 only (cid_quality refuses smaller images), so the 7 x 7 case covers PSNR and SSIM and a
case of its own runs all three metrics at 161 x 161."""
import numpy as np
import pytest
import torch

import test_discriminator as TD
import test_discriminator_backward as TDB
import test_generator_backward as TGB
import test_quality as TQ
from celebrity_image_denoiser_amd import synth

DEV = "cuda:0"
TOL = 1e-5
N = 65535 + 9
CUT = 32772
PARTS = ((0, CUT), (CUT, N))
SEAM = (0, 1, 32771, 65533, 65534, 65535, 65536, 65537, N - 2, N - 1)


def distinct_u8(n, h, w, seed):
    """Seeded uint8 [n,h,w,3]; pixel (0, 0) of image i is a 24-bit code no other image has."""
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    code = rng.permutation(1 << 24)[:n]
    for c in range(3):
        u8[:, 0, 0, c] = (code >> (8 * c)) & 255
    return u8


def distinct_f32(n, h, w, seed):
    u8 = distinct_u8(n, h, w, seed)
    return u8, torch.from_numpy(synth.normalize_u8(u8))


def _in_parts(fn):
    """fn(lo, hi) on the two smaller calls, concatenated."""
    return torch.cat([fn(lo, hi) for lo, hi in PARTS])


# ------------------------------------------------------------------------------------------------------------------ cid_add_noise
@pytest.mark.gpu
@pytest.mark.parametrize("kind", synth.NOISE_TYPES)
def test_add_noise(kind):
    from celebrity_image_denoiser_amd import noise

    # salt & pepper needs H, W >= 2 (numpy's randint(0, i - 1)); at 2 x 2 the default 0.02 would draw nothing
    side, params = (2, dict(salt_prob=0.25, pepper_prob=0.25)) if kind == "salt_pepper" else (1, {})
    clean = distinct_u8(N, side, side, 11)
    d = torch.from_numpy(clean).to(DEV)
    big = noise.add_noise(d, kind, **params)
    parts = _in_parts(lambda lo, hi: noise.add_noise(d[lo:hi], kind, first_index=lo, **params))
    assert torch.equal(big, parts)
    got = big.cpu().numpy()
    assert not np.array_equal(got, clean)
    for i in SEAM:
        assert np.array_equal(got[i:i + 1], synth.add_noise_np(clean[i:i + 1], kind, first_index=i, **params)), (kind, i)


# --------------------------------------------------------------------------------------------------------------------- cid_resize
@pytest.mark.gpu
@pytest.mark.parametrize("out", ("u8", "f32"))
@pytest.mark.parametrize("src,dst", (((3, 3), (2, 2)), ((2, 2), (5, 5))), ids=("3x3-2x2", "2x2-5x5"))
def test_resize(src, dst, out):
    from celebrity_image_denoiser_amd import resize as R

    clean = distinct_u8(N, src[0], src[1], 12)
    d = torch.from_numpy(clean).to(DEV)
    size = (dst[1], dst[0])
    big = R.resize(d, size, out=out)
    parts = _in_parts(lambda lo, hi: R.resize(d[lo:hi].contiguous(), size, out=out))
    assert torch.equal(big.view(torch.uint8), parts.view(torch.uint8))
    idx = list(SEAM)
    ref = synth.resize_bicubic_np(clean[idx], size)
    got = big[torch.tensor(idx, device=DEV)].cpu().numpy()
    if out == "u8":
        assert np.array_equal(got, ref)
    else:
        assert np.array_equal(got.view(np.uint32), synth.normalize_u8(ref).view(np.uint32))


# -------------------------------------------------------------------------------------------------------------------- cid_quality
@pytest.mark.gpu
def test_quality():
    from celebrity_image_denoiser_amd import metrics as M

    names = ("psnr", "ssim")
    a_u8 = distinct_u8(N, 7, 7, 13)
    b = distinct_f32(N, 7, 7, 14)[1]
    ad, bd = torch.from_numpy(a_u8).to(DEV), b.to(DEV)
    for first, second in ((ad, bd), (bd, ad)):          # the u8 operand on either side
        big = M.quality(first, second, names)
        for m in names:
            part = _in_parts(lambda lo, hi: M.quality(first[lo:hi].contiguous(), second[lo:hi].contiguous(), names)[m])
            assert torch.equal(big[m].view(torch.int64), part.view(torch.int64)), m
    idx = list(SEAM)
    got = {m: v.cpu().numpy() for m, v in big.items()}
    TQ._check(got, TQ.oracle(b.numpy()[idx], synth.normalize_u8(a_u8[idx]), names), idx)


@pytest.mark.gpu
def test_quality_ms_ssim():
    """All three metrics at 161 x 161, the smallest size MS-SSIM takes: the four pooled pyramid levels are launches of their own
    and carry the launch's first image too.  The batch (5 GB uint8, 20 GB fp32, 15 GB of workspace) is put together on the device
    from two seeded numpy blocks of 512 images: image n is block image n mod 512 with n written into its first pixel, and the fp32
    operand is its normalised copy plus a tenth of another block image, so that MS-SSIM is neither 0 nor 1."""
    from celebrity_image_denoiser_amd import metrics as M

    side, blocks = 161, 512
    rng = np.random.default_rng(19)
    base = torch.from_numpy(rng.integers(0, 256, (2, blocks, side, side, 3), dtype=np.uint8)).to(DEV)
    n_all = torch.arange(N, device=DEV)
    a = base[0][n_all % blocks]
    for c in range(3):
        a[:, 0, 0, c] = ((n_all >> (8 * c)) & 255).to(torch.uint8)
    b = torch.empty((N, 3, side, side), dtype=torch.float32, device=DEV)
    for lo in range(0, N, 4096):
        hi = min(lo + 4096, N)
        other = base[1][(n_all[lo:hi] * 7 + 3) % blocks]
        b[lo:hi] = ((a[lo:hi].float() / 255 - 0.5) / 0.5 + 0.1 * ((other.float() / 255 - 0.5) / 0.5)).permute(0, 3, 1, 2)
    del other, base
    big = M.quality(a, b, TQ.ALL)
    for lo, hi in PARTS:
        part = M.quality(a[lo:hi], b[lo:hi], TQ.ALL)
        for m in TQ.ALL:
            assert torch.equal(big[m][lo:hi].view(torch.int64), part[m].view(torch.int64)), (m, lo)
        del part
    idx = list(SEAM)
    didx = torch.tensor(idx, device=DEV)
    got = {m: v.cpu().numpy() for m, v in big.items()}
    ref = TQ.oracle(synth.normalize_u8(a[didx].cpu().numpy()), b[didx].cpu().numpy())
    assert 0.2 < ref["ms_ssim"].min() and ref["ms_ssim"].max() < 0.999
    TQ._check(got, ref, idx)
    del a, b, big
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ the discriminator
DISC_EVAL = (("trained", 1, 1), ("default", 2, 3))


def _disc_ref_eval(kind, x, gp=None, masks=None, dtype=torch.float64):
    return TDB.ref_backward(TD.weights(kind), x, False, None, dtype, masks, grad_prob=gp)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,h,w", DISC_EVAL, ids=("trained-1x1", "default-2x3"))
def test_discriminator_eval_forward(kind, h, w):
    u8, x = distinct_f32(N, h, w, 15)
    m = TD._module(kind, False)
    xd = x.to(DEV)
    big = m(xd)
    assert torch.equal(big, _in_parts(lambda lo, hi: m(xd[lo:hi])))
    assert torch.equal(big, m(torch.from_numpy(u8).to(DEV)))          # the u8 input's launches take the same split
    idx = list(SEAM)
    ref = TD.restate(TD.cast(TD.weights(kind), torch.float64), x[idx].double(), False)
    err = float((big.cpu()[idx].double() - ref).abs().max())
    print(f"eval {kind} {N}x{h}x{w}: max|p - ref64| on SEAM = {err:.2e}")
    assert err <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("kind,h,w", DISC_EVAL, ids=("trained-1x1", "default-2x3"))
def test_discriminator_eval_backward(kind, h, w):
    x = distinct_f32(N, h, w, 16)[1]
    xd = x.to(DEV)
    idx = list(SEAM)
    didx = torch.tensor(idx, device=DEV)
    m = TDB._module(kind, False)
    dense = torch.randn(N, generator=torch.Generator().manual_seed(4321))
    sparse = torch.zeros(N)
    sparse[idx] = dense[idx]
    dd, sd_ = dense.to(DEV), sparse.to(DEV)

    # (i) a dense upstream gradient: forward_saved's probabilities and the input gradient, image by image
    p, _, gx, masks, _ = TDB.cabi_backward(m, xd, False, lambda q: dd, want=())
    runs = [TDB.cabi_backward(m, xd[lo:hi], False, lambda q, lo=lo, hi=hi: dd[lo:hi], want=(), with_masks=False) for lo, hi in PARTS]
    assert torch.equal(p, torch.cat([r[0] for r in runs]))
    assert torch.equal(gx, torch.cat([r[2] for r in runs]))
    del runs
    # (ii) ... and on SEAM against float64 with the device's masks
    ms = [t[didx].cpu().bool() for t in masks]
    _, gx64, ys64, p64 = _disc_ref_eval(kind, x[idx], dense[idx], ms)
    assert float((p[didx].cpu().double() - p64).abs().max()) <= TOL
    TDB.check_mask_cap(ms, ys64, "hip")
    _, gx32, ys32, _ = _disc_ref_eval(kind, x[idx], dense[idx], None, torch.float32)
    ms32 = [y > 0 for y in ys32]
    TDB.check_mask_cap(ms32, ys64, "aten")
    _, gx64a, _, _ = _disc_ref_eval(kind, x[idx], dense[idx], ms32)
    e_hip = float((gx[didx].cpu().double() - gx64).abs().max()) / float(gx64.abs().max())
    e_aten = float((gx32.double() - gx64a).abs().max()) / float(gx64a.abs().max())
    print(f"\ndiscriminator eval {kind} {N}x{h}x{w} dense grad_prob, input gradient on SEAM: e_hip {e_hip:.2e}  e_aten {e_aten:.2e}")
    assert e_hip <= max(TOL, 2 * e_aten)

    # grad_prob zero off SEAM: the parameter gradients are those of x[SEAM]
    _, grads, gxs, _, _ = TDB.cabi_backward(m, xd, False, lambda q: sd_, with_masks=False)
    off = torch.ones(N, dtype=torch.bool, device=DEV)
    off[didx] = False
    assert bool((gxs[off] == 0).all())
    assert torch.equal(gxs[didx], gx[didx])
    got = {k: v.cpu() for k, v in grads.items()}
    g64, gx64, _, _ = _disc_ref_eval(kind, x[idx], sparse[idx], ms)
    g32, gx32, _, _ = _disc_ref_eval(kind, x[idx], sparse[idx], None, torch.float32)
    g64a, gx64a, _, _ = _disc_ref_eval(kind, x[idx], sparse[idx], ms32)
    e_hip = TDB.rel_errors(got, gxs[didx].cpu(), g64, gx64, False)
    e_aten = TDB.rel_errors(g32, gx32, g64a, gx64a, False)
    print(f"discriminator eval {kind} {N}x{h}x{w} grad_prob zero off SEAM:   e_hip      e_aten(fp32, CPU)")
    for k in TDB.PARAMS + ["input"]:
        print(f"    {k:16s} {e_hip[k]:.2e}   {e_aten[k]:.2e}")
    for k in TDB.PARAMS + ["input"]:
        assert bool(torch.isfinite(got[k] if k != "input" else gxs).all()), k
        assert e_hip[k] <= max(TOL, 2 * e_aten[k]), (k, e_hip[k], e_aten[k])


def _train_images(n, h, w, first_index=0):
    return distinct_f32(n, h, w, 17 + first_index)


@pytest.mark.gpu
def test_discriminator_train_forward():
    """BatchNorm's statistics run over all 65,544 images: probabilities, running mean and variance, and the counter."""
    TD._check_train("default", (N, 1, 1), 0.1, calls=1, make=_train_images)


@pytest.mark.gpu
def test_discriminator_train_backward():
    TDB.gradient_parity("default", (N, 1, 1), True, "real1", x=_train_images(N, 1, 1)[1])


# ------------------------------------------------------------------------------------------- the server's ESRGAN and SRGAN generators
@pytest.mark.gpu
def test_esrgan_forward():
    """Two residual blocks on 1 x 1 images: the head's and the tail's launches and the trunk's three epilogues (PReLU, residual, the
    closing sum) each take the split.  x is the true /255 view of the uint8 batch, so the uint8 input must give its bits."""
    import test_esrgan as TE
    from celebrity_image_denoiser_amd.esrgan import load_esrgan

    r = 2
    u8 = distinct_u8(N, 1, 1, 20)
    x = np.ascontiguousarray((u8.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))
    m = load_esrgan(synth.make_esrgan_state_dict("hot", r), num_residuals=r, device=DEV, strict=True)   # not TE's cache: freed below
    xd = torch.from_numpy(x).to(DEV)
    big = m(xd)
    assert torch.equal(big.view(torch.int32), _in_parts(lambda lo, hi: m(xd[lo:hi])).view(torch.int32))
    assert torch.equal(big.view(torch.int32), m(torch.from_numpy(u8).to(DEV), out_dtype=torch.float32).view(torch.int32))
    idx = list(SEAM)
    ref = TE.esrgan_oracle.forward(synth.make_esrgan_state_dict("hot", r), x[idx], r)
    TE.check(f"esrgan hot r{r} {N}x1x1, out on SEAM", big.cpu().numpy()[idx], ref["out"])
    del m, big, xd
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_srgan_forward():
    """scale_factor 2 on 1 x 1 images: the head, the eleven trunk launches, one upscale stage (grid z = 2) and the tail each take the
    split.  As in test_srgan.py the output is held to the bound of the sums before tanh, which the raw call gives."""
    import test_srgan as TS
    from celebrity_image_denoiser_amd.srgan import load_srgan

    scale = 2
    u8 = distinct_u8(N, 1, 1, 21)
    x = TS.srgan_oracle.normalise_u8(u8)
    m = load_srgan(synth.make_srgan_state_dict("hot", scale), scale_factor=scale, device=DEV, strict=True)   # not TS's cache: freed below
    xd = torch.from_numpy(x).to(DEV)
    idx = list(SEAM)
    ref = TS.srgan_oracle.forward(synth.make_srgan_state_dict("hot", scale), x[idx])
    for raw, name in ((True, "pre"), (False, "out")):
        big = m(xd, raw=raw)
        assert big.shape == (N, 3, scale, scale)
        assert torch.equal(big.view(torch.int32), _in_parts(lambda lo, hi: m(xd[lo:hi], raw=raw)).view(torch.int32)), name
        assert torch.equal(big.view(torch.int32), m(torch.from_numpy(u8).to(DEV), out_dtype=torch.float32, raw=raw).view(torch.int32)), name
        TS.check(f"srgan hot s{scale} {N}x1x1, {name} on SEAM", big.cpu().numpy()[idx], ref[name], bound=TS.srgan_oracle.bound(ref["pre"]))
    del m, big, xd
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------ the generator
GEN_STAGES = TGB.RELU_STAGES + ("pool1", "pool2", "up2", "up1")


class _Gen:
    """The one big cid_forward_saved call (weights "hot", N x 3 x 4 x 4), shared by the three generator tests."""

    def __init__(self):
        self.m = TGB._module("hot")
        self.sd = {k: v.detach().cpu() for k, v in self.m.state_dict().items()}
        self.x = distinct_f32(N, 4, 4, 18)[1]
        self.xd = self.x.to(DEV)
        self.y, self.saved = TGB.forward_saved(self.m, self.xd)
        self.idx = list(SEAM)
        self.didx = torch.tensor(self.idx, device=DEV)
        self.masks, self.argmax = TGB.saved_masks_and_argmax(self.saved, N, 4, 4, self.didx)
        self._ref = {}

    def reference(self, name, grad_out):
        """float64 with the device's masks and routing, and ATen fp32 against float64 with ATen's, on x[SEAM]."""
        if name not in self._ref:
            xs, up = self.x[self.idx], ("grad", grad_out[self.idx])
            g64, gx64, pre64, pin64, own64, y64 = TGB.ref_backward(self.sd, xs, torch.float64, up, self.masks, self.argmax)
            TGB.check_caps(self.masks, self.argmax, pre64, pin64, own64, "hip")
            g32, gx32, pre32, _, own32, _ = TGB.ref_backward(self.sd, xs, torch.float32, up)
            masks32 = [t > 0 for t in pre32]
            TGB.check_caps(masks32, own32, pre64, pin64, own64, "aten")
            g64a, gx64a, _, _, _, _ = TGB.ref_backward(self.sd, xs, torch.float64, up, masks32, own32)
            self._ref[name] = (g64, gx64, y64, TGB.rel_errors(g32, gx32, g64a, gx64a))
        return self._ref[name]


@pytest.fixture(scope="module")
def gen():
    g = _Gen()
    yield g
    g.saved = g.y = g.xd = None
    g.m._ws = None
    del g
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_generator_forward_saved(gen):
    for lo, hi in PARTS:
        y, saved = TGB.forward_saved(gen.m, gen.xd[lo:hi])
        assert torch.equal(gen.y[lo:hi], y)
        for s in GEN_STAGES:
            assert torch.equal(TGB.stage(gen.saved, s, N, 4, 4)[lo:hi], TGB.stage(saved, s, hi - lo, 4, 4)), (lo, s)
        del y, saved
    y64 = gen.reference("dense", _dense_grad_out())[2]
    err = float((gen.y[gen.didx].cpu().double() - y64).abs().max())
    print(f"generator hot {N}x4x4: max|y - y64| on SEAM = {err:.2e}")
    assert err <= TOL


def _dense_grad_out():
    return torch.randn((N, 3, 4, 4), generator=torch.Generator().manual_seed(1234))


@pytest.mark.gpu
def test_generator_backward_input_gradient(gen):
    go = _dense_grad_out()
    god = go.to(DEV)
    _, _, gx, _, _ = TGB.cabi_backward(gen.m, gen.xd, lambda y: god, want=(), saved=gen.saved, y=gen.y)
    for lo, hi in PARTS:
        _, _, gxp, _, _ = TGB.cabi_backward(gen.m, gen.xd[lo:hi], lambda y, lo=lo, hi=hi: god[lo:hi], want=())
        assert torch.equal(gx[lo:hi], gxp), lo
        del gxp
    assert bool(torch.isfinite(gx).all())
    _, gx64, _, e_aten = gen.reference("dense", go)
    e_hip = float((gx[gen.didx].cpu().double() - gx64).abs().max()) / float(gx64.abs().max())
    print(f"\ngenerator hot {N}x4x4 dense grad_out, input gradient on SEAM: e_hip {e_hip:.2e}  e_aten {e_aten['input']:.2e}")
    assert e_hip <= max(TOL, 2 * e_aten["input"])


@pytest.mark.gpu
def test_generator_backward_parameter_gradients(gen):
    go = torch.zeros((N, 3, 4, 4))
    go[gen.idx] = _dense_grad_out()[gen.idx]
    god = go.to(DEV)
    _, grads, gx, _, _ = TGB.cabi_backward(gen.m, gen.xd, lambda y: god, saved=gen.saved, y=gen.y)
    off = torch.ones(N, dtype=torch.bool, device=DEV)
    off[gen.didx] = False
    assert bool((gx[off] == 0).all())
    got = {k: v.cpu() for k, v in grads.items()}
    g64, gx64, _, e_aten = gen.reference("sparse", go)
    e_hip = TGB.rel_errors(got, gx[gen.didx].cpu(), g64, gx64)
    print(f"\ngenerator hot {N}x4x4 grad_out zero off SEAM:   e_hip      e_aten(fp32, CPU)")
    for k in TGB.PARAMS + ["input"]:
        print(f"    {k:20s} {e_hip[k]:.2e}   {e_aten[k]:.2e}")
    for k in TGB.PARAMS:
        assert bool(torch.isfinite(got[k]).all()), k
    assert bool(torch.isfinite(gx).all())
    for k in TGB.PARAMS + ["input"]:
        assert e_hip[k] <= max(TOL, 2 * e_aten[k]), (k, e_hip[k], e_aten[k])
