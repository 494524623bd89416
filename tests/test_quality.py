"""Device image-quality metrics (cid_quality, metrics.quality / metrics.evaluate): PSNR, SSIM and MS-SSIM as the reference's
denoise trainer evaluates them (backend/trainingcode/denoise_gan_code/training.py:378-392).

The oracle below is a float64 restatement of the definitions in include/cid.h (skimage peak_signal_noise_ratio and
structural_similarity(channel_axis=2, data_range=2.0), pytorch_msssim.MS_SSIM(data_range=1.0) v1.0), on the CPU with numpy
and torch.  Tolerances against it: PSNR 1e-4 dB, SSIM and MS-SSIM 1e-5 per image."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from celebrity_image_denoiser_amd import _lib, synth

PSNR_TOL, SSIM_TOL = 1e-4, 1e-5
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
ERR_INVALID, ERR_SHAPE, ERR_WORKSPACE = 1, 2, 5
ALL = ("psnr", "ssim", "ms_ssim")


# ---------------------------------------------------------------- float64 oracle
def oracle_psnr(a, b):
    """d = a - b and d*d in fp32, the mean over 3*H*W in fp64, 10*log10(2^2 / mse) per image."""
    d = a.astype(np.float32) - b.astype(np.float32)
    mse = (d * d).reshape(d.shape[0], -1).astype(np.float64).mean(axis=1)
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(4.0 / mse)


def box_mean(x):
    """7x7 uniform mean at every interior pixel (skimage's crop(S, 3) region) of float64 [N,C,H,W]."""
    return F.avg_pool2d(x, 7, stride=1)


def oracle_ssim(a, b):
    X, Y = torch.from_numpy(np.asarray(a, np.float32)).double(), torch.from_numpy(np.asarray(b, np.float32)).double()
    cn = 49.0 / 48.0
    C1, C2 = (0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2
    ux, uy = box_mean(X), box_mean(Y)
    uxx, uyy, uxy = box_mean(X * X), box_mean(Y * Y), box_mean(X * Y)
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    S = (2 * ux * uy + C1) * (2 * vxy + C2) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return S.mean(dim=(2, 3)).mean(dim=1).numpy()


def gauss_window():
    """pytorch_msssim _fspecial_gauss_1d(11, 1.5): computed in float32 as torch does, then float64."""
    coords = torch.arange(11, dtype=torch.float32) - 5
    g = torch.exp(-(coords ** 2) / (2 * 1.5 ** 2))
    return (g / g.sum()).double()


def gauss_filter(x, g):
    c = x.shape[1]
    x = F.conv2d(x, g.view(1, 1, 1, 11).repeat(c, 1, 1, 1), groups=c)      # valid, no padding
    return F.conv2d(x, g.view(1, 1, 11, 1).repeat(c, 1, 1, 1), groups=c)


def pool2(x):
    """avg_pool2d(kernel 2, stride 2, padding (H%2, W%2), count_include_pad=True), written out in numpy: an odd side gets one
    zero on each end and becomes (s+1)/2."""
    x = np.asarray(x, np.float64)
    ph, pw = x.shape[-2] % 2, x.shape[-1] % 2
    x = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(ph, ph), (pw, pw)])
    ho, wo = (x.shape[-2] - 2) // 2 + 1, (x.shape[-1] - 2) // 2 + 1
    x = x[..., : 2 * ho, : 2 * wo]
    return (x[..., 0::2, 0::2] + x[..., 0::2, 1::2] + x[..., 1::2, 0::2] + x[..., 1::2, 1::2]) / 4.0


def oracle_msssim(a, b):
    half = np.float32(0.5)
    X = torch.from_numpy((np.asarray(a, np.float32) * half + half).astype(np.float32)).double()
    Y = torch.from_numpy((np.asarray(b, np.float32) * half + half).astype(np.float32)).double()
    g = gauss_window()
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    vals = []
    for level in range(5):
        mx, my = gauss_filter(X, g), gauss_filter(Y, g)
        sxx = gauss_filter(X * X, g) - mx * mx
        syy = gauss_filter(Y * Y, g) - my * my
        sxy = gauss_filter(X * Y, g) - mx * my
        cs_map = (2 * sxy + C2) / (sxx + syy + C2)
        ssim_map = (2 * mx * my + C1) / (mx * mx + my * my + C1) * cs_map
        if level < 4:
            vals.append(torch.relu(cs_map.mean(dim=(2, 3))))
            X, Y = torch.from_numpy(pool2(X.numpy())), torch.from_numpy(pool2(Y.numpy()))
        else:
            vals.append(torch.relu(ssim_map.mean(dim=(2, 3))))
    w = torch.tensor(MS_WEIGHTS, dtype=torch.float64)
    per_channel = torch.prod(torch.stack(vals) ** w.view(-1, 1, 1), dim=0)
    return per_channel.mean(dim=1).numpy()


def oracle(a, b, metrics=ALL):
    fns = {"psnr": oracle_psnr, "ssim": oracle_ssim, "ms_ssim": oracle_msssim}
    return {m: fns[m](a, b) for m in metrics}


# ---------------------------------------------------------------- no GPU: the oracle itself
def test_oracle_identities():
    x, clean, _ = synth.make_batch(2, 176, 168, first_index=40)
    np.testing.assert_allclose(oracle_ssim(x, x), 1.0, atol=1e-12)
    np.testing.assert_allclose(oracle_msssim(x, x), 1.0, atol=1e-12)
    xq = (np.round(x * 1024) / 1024).astype(np.float32)          # on a 2^-10 grid: x + d is exact in fp32
    for d in (0.5, 0.125, 2.0 ** -7):
        np.testing.assert_allclose(oracle_psnr(xq + np.float32(d), xq), 10 * np.log10(4.0 / d ** 2), rtol=1e-12)
    assert np.all(np.isinf(oracle_psnr(x, x)))
    s = oracle_ssim(x, clean)
    assert np.all((s > 0) & (s < 1))


def test_oracle_box_mean_is_uniform_filter_interior():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(7)
    x = rng.standard_normal((1, 1, 23, 31))
    ref = ndimage.uniform_filter(x[0, 0], size=7)[3:-3, 3:-3]
    np.testing.assert_allclose(box_mean(torch.from_numpy(x))[0, 0].numpy(), ref, rtol=1e-12, atol=1e-13)


def test_oracle_odd_pooling_is_avg_pool2d_with_padding():
    rng = np.random.default_rng(8)
    for h, w in ((161, 161), (161, 203), (81, 102), (200, 255), (12, 17)):
        x = rng.standard_normal((1, 3, h, w))
        ref = F.avg_pool2d(torch.from_numpy(x), kernel_size=2, padding=(h % 2, w % 2)).numpy()
        out = pool2(x)
        assert out.shape[-2:] == ((h + 1) // 2, (w + 1) // 2)
        np.testing.assert_allclose(out, ref, rtol=1e-14, atol=1e-15)


# ---------------------------------------------------------------- no GPU: the C ABI's host checks
def _ws(n, h, w, metrics):
    b = ctypes.c_size_t()
    rc = _lib.lib().cid_quality_workspace_bytes(n, h, w, metrics, ctypes.byref(b))
    return rc, b.value


def test_quality_workspace_bytes():
    assert _lib.CID_METRIC_PSNR | _lib.CID_METRIC_SSIM | _lib.CID_METRIC_MS_SSIM == 7
    rc, one = _ws(1, 256, 256, 3)
    assert rc == 0 and one > 0
    rc, many = _ws(256, 256, 256, 3)
    assert rc == 0 and many >= 256 * (one - 255)
    rc, ms = _ws(16, 256, 256, 7)
    # MS-SSIM keeps both images' pooled levels 1..4 in fp32
    pyr = sum(16 * 3 * (-(-256 // 2 ** l)) ** 2 * 4 for l in range(1, 5)) * 2
    assert rc == 0 and ms >= pyr
    assert _ws(1, 1, 1, 1)[0] == 0              # PSNR alone takes any size
    assert _ws(1, 7, 7, 2)[0] == 0
    assert _ws(1, 161, 161, 4)[0] == 0
    assert _ws(1, 6, 7, 2)[0] == ERR_SHAPE
    assert _ws(1, 7, 6, 3)[0] == ERR_SHAPE
    assert _ws(1, 160, 300, 4)[0] == ERR_SHAPE
    assert _ws(1, 300, 160, 5)[0] == ERR_SHAPE
    assert _ws(0, 64, 64, 1)[0] == ERR_SHAPE
    assert _ws(1, 65536, 65536, 1)[0] == ERR_SHAPE
    assert _ws(1, 64, 64, 0)[0] == ERR_INVALID
    assert _ws(1, 64, 64, 8)[0] == ERR_INVALID
    assert _lib.lib().cid_quality_workspace_bytes(1, 64, 64, 1, None) == ERR_INVALID


def test_quality_argument_errors_come_before_any_launch():
    """Every call here is invalid, so none reaches a launch: the dummy pointers are never dereferenced."""
    L = _lib.lib()
    P = ctypes.c_void_p(0x100000)           # dummy non-null, 256-byte aligned
    _, need = _ws(2, 200, 200, 7)
    big = need + (1 << 20)

    def q(a=P, fa=0, b=P, fb=0, n=2, h=200, w=200, m=7, out=P, ws=P, nbytes=big):
        return L.cid_quality(a, fa, b, fb, n, h, w, m, out, ws, nbytes, None)

    assert q(a=None) == ERR_INVALID
    assert q(b=None) == ERR_INVALID
    assert q(out=None) == ERR_INVALID
    assert q(ws=None) == ERR_INVALID
    assert q(fa=2) == ERR_INVALID
    assert q(fb=-1) == ERR_INVALID
    assert q(a=ctypes.c_void_p(0x100002)) == ERR_INVALID          # misaligned fp32 operand
    assert q(out=ctypes.c_void_p(0x100004)) == ERR_INVALID        # misaligned double output
    assert q(m=0) == ERR_INVALID
    assert q(m=8) == ERR_INVALID
    assert q(m=15) == ERR_INVALID
    assert q(n=0) == ERR_SHAPE
    assert q(n=-3) == ERR_SHAPE
    assert q(h=6, m=2) == ERR_SHAPE
    assert q(w=6, m=3) == ERR_SHAPE
    assert q(h=160, m=4) == ERR_SHAPE
    assert q(w=160, m=7) == ERR_SHAPE
    assert q(h=65536, w=65536, m=1) == ERR_SHAPE
    assert q(nbytes=need - 1) == ERR_WORKSPACE
    assert q(ws=ctypes.c_void_p(0x100008)) == ERR_WORKSPACE
    assert q(fa=1, a=ctypes.c_void_p(0x100001), nbytes=need - 1) == ERR_WORKSPACE   # u8 operands need no alignment


def test_quality_rejects_cpu_tensors_and_mismatched_shapes():
    from celebrity_image_denoiser_amd import metrics as M

    x = torch.zeros(2, 3, 16, 16)
    with pytest.raises(RuntimeError):
        M.quality(x, x)
    with pytest.raises(RuntimeError):
        M.evaluate(x, x, ms_ssim=False)
    with pytest.raises(ValueError, match="Input images must have the same dimensions."):
        M.quality(x, torch.zeros(2, 3, 16, 17))
    with pytest.raises(ValueError, match="Input images must have the same dimensions."):
        M.quality(x, torch.zeros(3, 16, 16, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        M.quality(x, x, metrics=("psnr", "lpips"))


# ---------------------------------------------------------------- on the MI355X
DEV = "cuda:0"


def _gpu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _run(a, b, metrics=ALL):
    from celebrity_image_denoiser_amd import metrics as M

    r = M.quality(_gpu(a) if isinstance(a, np.ndarray) else a, _gpu(b) if isinstance(b, np.ndarray) else b, metrics)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _check(got, ref, idx=None):
    for m, r in ref.items():
        g = got[m] if idx is None else got[m][idx]
        tol = PSNR_TOL if m == "psnr" else SSIM_TOL
        assert g.dtype == np.float64
        np.testing.assert_allclose(g, r, rtol=0, atol=tol, err_msg=m)


@pytest.mark.gpu
def test_synth_noisy_vs_clean_matches_oracle():
    x, clean, _ = synth.make_batch(4, 128, 128, first_index=300)
    got = _run(x, clean, ("psnr", "ssim"))
    assert set(got) == {"psnr", "ssim"}
    _check(got, oracle(x, clean, ("psnr", "ssim")))
    x, clean, _ = synth.make_batch(3, 256, 256, first_index=310)
    _check(_run(x, clean), oracle(x, clean))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["default", "hot"])
def test_forward_output_vs_clean_matches_oracle(kind, weight_sets):
    import celebrity_image_denoiser_amd as cid

    model = cid.load(weight_sets[kind], device=DEV, strict=True)
    x, clean, _ = synth.make_batch(4, 256, 256, first_index=320)
    y = model(_gpu(x))
    got = _run(y, _gpu(clean))
    _check(got, oracle(y.cpu().numpy(), clean))


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(7, 7), (13, 18), (161, 161), (161, 203), (200, 255)])
def test_odd_and_edge_sizes_match_oracle(hw):
    h, w = hw
    metrics = ALL if min(h, w) > 160 else ("psnr", "ssim")
    x, clean, _ = synth.make_batch(2, h, w, first_index=330)
    _check(_run(x, clean, metrics), oracle(x, clean, metrics))


@pytest.mark.gpu
def test_u8_operands_are_bit_identical_to_their_normalised_copy():
    _, clean, noisy_u8 = synth.make_batch(3, 176, 184, first_index=340)
    clean_u8 = synth.clean_images_u8(3, 176, 184, first_index=340)
    x = synth.normalize_u8(noisy_u8)
    f32 = _run(x, clean)
    mixed = _run(noisy_u8, clean)
    both_u8 = _run(noisy_u8, clean_u8)
    for m in ALL:
        assert np.array_equal(f32[m], mixed[m]), m
        assert np.array_equal(f32[m], both_u8[m]), m
    _check(mixed, oracle(x, clean))
    _check(_run(x, clean_u8), oracle(x, clean))


@pytest.mark.gpu
def test_identical_inputs():
    x, _, _ = synth.make_batch(2, 192, 200, first_index=350)
    got = _run(x, x)
    assert np.all(np.isinf(got["psnr"])) and np.all(got["psnr"] > 0)
    assert np.all(got["ssim"] == 1.0)
    assert np.all(np.abs(got["ms_ssim"] - 1.0) <= 1e-7)


@pytest.mark.gpu
def test_deterministic_and_independent_of_the_batch():
    x, clean, _ = synth.make_batch(37, 192, 192, first_index=360)
    a, b = _gpu(x), _gpu(clean)
    r1, r2 = _run(a, b), _run(a, b)
    for m in ALL:
        assert np.array_equal(r1[m], r2[m]), m
    for k in (0, 17, 36):
        alone = _run(a[k:k + 1].contiguous(), b[k:k + 1].contiguous())
        for m in ALL:
            assert np.array_equal(alone[m], r1[m][k:k + 1]), (m, k)


@pytest.mark.gpu
def test_nan_stays_in_its_image():
    x, clean, _ = synth.make_batch(4, 176, 176, first_index=370)
    ref = _run(x, clean)
    x[2, 1, 90, 50] = np.nan
    got = _run(x, clean)
    for m in ALL:
        assert np.isnan(got[m][2]), m
        keep = [0, 1, 3]
        assert np.array_equal(got[m][keep], ref[m][keep]), m


@pytest.mark.gpu
def test_batch_256_at_256():
    x, clean, _ = synth.make_batch(256, 256, 256, first_index=400)
    got = _run(x, clean)
    idx = [0, 1, 128, 255]
    _check(got, oracle(x[idx], clean[idx]), idx)


@pytest.mark.gpu
def test_full_hd_pair():
    x, clean, _ = synth.make_batch(1, 1440, 1920, first_index=700)
    _check(_run(x, clean), oracle(x, clean))


@pytest.mark.gpu
def test_evaluate_is_the_trainers_batch_means():
    from celebrity_image_denoiser_amd import metrics as M

    x, clean, _ = synth.make_batch(5, 176, 192, first_index=380)
    ref = oracle(x, clean)
    psnr, ssim, lpips, msssim = M.evaluate(_gpu(x), _gpu(clean))
    assert all(isinstance(v, float) for v in (psnr, ssim, lpips, msssim))
    assert lpips == 0.0
    assert abs(psnr - ref["psnr"].mean()) <= PSNR_TOL
    assert abs(ssim - ref["ssim"].mean()) <= SSIM_TOL
    assert abs(msssim - ref["ms_ssim"].mean()) <= SSIM_TOL
    x, clean, _ = synth.make_batch(2, 128, 128, first_index=390)
    with pytest.raises(ValueError):
        M.evaluate(_gpu(x), _gpu(clean))
    psnr, ssim, lpips, msssim = M.evaluate(_gpu(x), _gpu(clean), ms_ssim=False)
    assert lpips == 0.0 and msssim == 0.0
    ref = oracle(x, clean, ("psnr", "ssim"))
    assert abs(psnr - ref["psnr"].mean()) <= PSNR_TOL
    assert abs(ssim - ref["ssim"].mean()) <= SSIM_TOL
