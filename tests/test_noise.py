"""Noise synthesis (cid_add_noise, noise.add_noise / noise.evaluate_noise_types): the reference trainer's five noise kinds
(backend/trainingcode/denoise_gan_code/noise_generation.py:6-39) on device uint8 batches.

CPU: the numpy restatements in synth.py against the reference's own expressions run on np.random.default_rng (per-value means
and variances within 5 sigma on a ramp image holding every value 0..255), and the C ABI's host-side argument checks.
GPU: the device output equals the restatement bit for bit (gaussian and speckle: except where the float64 value lies within
1e-9 of an integer or a clip edge, where an ulp of log / cos could move the truncation; none are expected)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth

ERR_INVALID, ERR_SHAPE = 1, 2
KINDS = synth.NOISE_TYPES
B_STAT = 2000                      # ramp images per statistical test: 3*B_STAT samples per pixel value


def ramp(n):
    """[n,16,16,3] uint8: pixel (y, x) holds y*16 + x in all channels, so every value 0..255 occurs 3 times per image."""
    img = np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=2)
    return np.ascontiguousarray(np.broadcast_to(img, (n, 16, 16, 3)))


def per_value(x):
    """[256, samples]: the outputs at each clean value of a ramp batch."""
    return x.reshape(x.shape[0], 256, 3).transpose(1, 0, 2).reshape(256, -1).astype(np.float64)


def assert_same_distribution(a, b, what):
    """Per clean value: means and variances of two sample sets agree within 5 sigma of their difference."""
    a, b = per_value(a), per_value(b)
    na, nb = a.shape[1], b.shape[1]
    ma, mb = a.mean(1), b.mean(1)
    va, vb = a.var(1), b.var(1)
    tol_m = 5 * np.sqrt(va / na + vb / nb) + 1e-12
    bad = np.nonzero(np.abs(ma - mb) > tol_m)[0]
    assert bad.size == 0, f"{what}: means differ at values {bad[:8]}: {ma[bad[:8]]} vs {mb[bad[:8]]}"
    m4a = ((a - ma[:, None]) ** 4).mean(1)
    m4b = ((b - mb[:, None]) ** 4).mean(1)
    tol_v = 5 * np.sqrt(np.maximum(m4a - va ** 2, 0) / na + np.maximum(m4b - vb ** 2, 0) / nb) + 1e-9
    bad = np.nonzero(np.abs(va - vb) > tol_v)[0]
    assert bad.size == 0, f"{what}: variances differ at values {bad[:8]}: {va[bad[:8]]} vs {vb[bad[:8]]}"


# ---------------------------------------------------------------- no GPU: restatements against the reference's formulas
def test_gaussian_dispatch_is_add_gaussian_noise_bit_for_bit():
    clean = synth.clean_images_u8(3, 40, 56, first_index=11)
    for fi, sigma in ((11, 25.0), (0, 25.0), (500, 7.5)):
        ref = synth.add_gaussian_noise(clean, sigma, first_index=fi)
        assert np.array_equal(synth.add_noise_np(clean, "gaussian", first_index=fi, sigma=sigma), ref)
        assert np.array_equal(synth.add_noise_np(clean, "gaussian", synth.NOISE_SEED, fi, mean=0.0, sigma=sigma), ref)


@pytest.mark.parametrize("kind", ["gaussian", "speckle", "uniform"])
def test_additive_kinds_match_the_reference_distribution(kind):
    img = ramp(B_STAT)
    rng = np.random.default_rng({"gaussian": 1, "speckle": 2, "uniform": 3}[kind])
    if kind == "gaussian":      # noise_generation.py:6-10
        ref = np.clip(img + rng.normal(0, 25, img.shape), 0, 255).astype(np.uint8)
    elif kind == "speckle":     # :24-28
        ref = np.clip(img + img * rng.normal(0, 0.1, img.shape), 0, 255).astype(np.uint8)
    else:                       # :35-39
        ref = np.clip(img + rng.uniform(0, 25, img.shape), 0, 255).astype(np.uint8)
    ours = synth.add_noise_np(img, kind, seed=77, first_index=5)
    assert_same_distribution(ours, ref, kind)
    # the hash streams vary per image and per element
    assert not np.array_equal(ours[0], ours[1])


def poisson_tail(lam, k0):
    """P(k >= k0) for k ~ Poisson(lam), summed exactly in log space."""
    head = sum(math.exp(-lam + k * math.log(lam) - math.lgamma(k + 1)) for k in range(k0))
    return 1.0 - head


def test_poisson_matches_the_reference_including_its_uint8_wrap():
    img = ramp(B_STAT)
    rng = np.random.default_rng(4)
    ref = rng.poisson(img).astype(np.uint8)             # noise_generation.py:30-33: int64 -> uint8 wraps
    ours = synth.add_poisson_noise(img, seed=78, first_index=9)
    assert_same_distribution(ours, ref, "poisson")
    assert np.all(per_value(ours)[0] == 0)              # lambda = 0 gives k = 0
    # at lambda = 255, k >= 256 wraps to a dark value (k - 256 < 128); k < 128 has probability ~1e-20
    at255 = per_value(ours)[255]
    dark = float((at255 < 128).mean())
    p = poisson_tail(255.0, 256)
    assert 0.45 < p < 0.50
    assert abs(dark - p) <= 5 * math.sqrt(p * (1 - p) / at255.size), (dark, p)


def test_poisson_table_search_is_the_sequential_inversion():
    clean = synth.clean_images_u8(2, 24, 20, first_index=3)
    clean[1, :4] = 255
    clean[1, 4:6] = 0
    u = synth._image_uniforms(5, 3, 2, synth.NOISE_STREAMS["poisson"][0], 24 * 20 * 3)
    got = synth.add_poisson_noise(clean, seed=5, first_index=3).reshape(2, -1)
    lam = clean.reshape(2, -1)
    for i in range(2):
        for e in range(0, lam.shape[1], 7):
            L = float(lam[i, e])
            p = c = math.exp(-L)
            k = 0
            while u[i, e] >= c and k < 1023:
                k += 1
                p = (p * L) / k
                c = c + p
            assert got[i, e] == k % 256, (i, e, L)


def test_salt_pepper_matches_the_reference_counts():
    n, h, w = B_STAT, 32, 32
    img = np.full((n, h, w, 3), 128, np.uint8)
    ours = synth.add_salt_pepper_noise(img, seed=79, first_index=2)
    rng = np.random.default_rng(5)
    ref = img.copy()
    k = int(img[0].size * 0.02)                       # noise_generation.py:12-22, per image
    for i in range(n):
        coords = [rng.integers(0, s - 1, k) for s in img[i].shape]
        ref[i][coords[0], coords[1], :] = 255
        coords = [rng.integers(0, s - 1, k) for s in img[i].shape]
        ref[i][coords[0], coords[1], :] = 0
    cells = (h - 1) * (w - 1)
    q = 1.0 - 1.0 / cells
    expect = {255: cells * (1 - q ** k) * q ** k, 0: cells * (1 - q ** k)}   # salt less pepper collisions; pepper
    for x, name in ((ours, "ours"), (ref, "reference")):
        changed = x != 128
        assert np.all(changed.all(axis=3) == changed.any(axis=3)), name       # all 3 channels set together
        assert not changed[:, -1].any() and not changed[:, :, -1].any(), name  # never the last row or column
        for value, e in expect.items():
            cnt = (x[..., 0] == value).reshape(n, -1).sum(1)
            assert abs(cnt.mean() - e) <= 5 * cnt.std() / math.sqrt(n) + 1e-9, (name, value, cnt.mean(), e)


def test_salt_pepper_pepper_wins_and_counts_are_exact():
    h, w = 9, 7
    img = np.full((3, h, w, 3), 100, np.uint8)
    out = synth.add_salt_pepper_noise(img, 0.5, 0.4, seed=3, first_index=40)
    for i in range(3):
        (sr, sc), (pr, pc) = synth.salt_pepper_coords(h, w, 0.5, 0.4, seed=3, index=40 + i)
        assert sr.size == int(float(h * w * 3) * 0.5) and pr.size == int(float(h * w * 3) * 0.4)
        assert sr.max() <= h - 2 and sc.max() <= w - 2 and pr.max() <= h - 2 and pc.max() <= w - 2
        pepper = set(zip(pr.tolist(), pc.tolist()))
        salt = set(zip(sr.tolist(), sc.tolist())) - pepper
        assert salt and len(set(zip(sr.tolist(), sc.tolist())) & pepper) > 0      # collisions happen at these rates
        for (y, x) in pepper:
            assert np.all(out[i, y, x] == 0)
        for (y, x) in salt:
            assert np.all(out[i, y, x] == 255)
        assert int((out[i, ..., 0] == 0).sum()) == len(pepper)
        assert int((out[i, ..., 0] == 255).sum()) == len(salt)
    with pytest.raises(ValueError):
        synth.add_salt_pepper_noise(np.zeros((1, 1, 5, 3), np.uint8))


def test_mulhi_is_exact():
    z = synth._hash_u64(1, 2, 2000)
    for m in (1, 2, 30, 255, 1439, 65535, 2 ** 31 - 1):
        got = synth._mulhi64(z, m)
        assert all(int(g) == (int(v) * m) >> 64 for g, v in zip(got, z)), m


def test_restatement_images_depend_only_on_their_global_index():
    clean = synth.clean_images_u8(5, 20, 28, first_index=60)
    for kind in KINDS:
        full = synth.add_noise_np(clean, kind, seed=9, first_index=60)
        for k in (0, 3):
            alone = synth.add_noise_np(clean[k:k + 1], kind, seed=9, first_index=60 + k)
            assert np.array_equal(alone[0], full[k]), kind
        other = synth.add_noise_np(clean, kind, seed=10, first_index=60)
        assert not np.array_equal(other, full), kind


def test_restatement_rejects_unknown_names():
    x = np.zeros((1, 8, 8, 3), np.uint8)
    with pytest.raises(ValueError):
        synth.add_noise_np(x, "pink")
    with pytest.raises(TypeError):
        synth.add_noise_np(x, "uniform", sigma=3.0)
    with pytest.raises(TypeError):
        synth.add_noise_np(x, "poisson", lam=3.0)


# ---------------------------------------------------------------- no GPU: the C ABI's host checks
def test_noise_constants_and_streams():
    assert (_lib.CID_NOISE_GAUSSIAN, _lib.CID_NOISE_SALT_PEPPER, _lib.CID_NOISE_SPECKLE, _lib.CID_NOISE_POISSON,
            _lib.CID_NOISE_UNIFORM) == (0, 1, 2, 3, 4)
    assert KINDS == ("gaussian", "salt_pepper", "speckle", "poisson", "uniform")
    ids = [s for v in synth.NOISE_STREAMS.values() for s in v]
    assert len(set(ids)) == len(ids) and all(s > 2 for s in ids[2:])


def test_add_noise_argument_errors_come_before_any_launch():
    """Every call here is invalid, so none reaches a launch: the dummy pointers are never dereferenced."""
    L = _lib.lib()
    P = ctypes.c_void_p(0x100000)

    def call(kind=0, params=(0.0, 25.0), nparams=None, a=P, o=P, n=2, h=64, w=64, null_params=False):
        arr = None if null_params else (ctypes.c_double * max(len(params), 1))(*params)
        return L.cid_add_noise(a, o, n, h, w, kind, arr, len(params) if nparams is None else nparams, 1, 0, None)

    assert call(a=None) == ERR_INVALID
    assert call(o=None) == ERR_INVALID
    assert call(kind=-1) == ERR_INVALID
    assert call(kind=5) == ERR_INVALID
    assert call(nparams=1) == ERR_INVALID
    assert call(nparams=3) == ERR_INVALID
    assert call(kind=3, params=(1.0, 2.0)) == ERR_INVALID           # poisson takes no parameters
    assert call(null_params=True) == ERR_INVALID
    assert call(params=(0.0, float("nan"))) == ERR_INVALID
    assert call(params=(float("inf"), 1.0)) == ERR_INVALID
    assert call(kind=2, params=(0.0, -0.1)) == ERR_INVALID
    assert call(kind=0, params=(0.0, -1.0)) == ERR_INVALID
    assert call(kind=1, params=(1.5, 0.02)) == ERR_INVALID
    assert call(kind=1, params=(0.02, -0.01)) == ERR_INVALID
    assert call(kind=4, params=(5.0, 4.0)) == ERR_INVALID
    assert call(n=0) == ERR_SHAPE
    assert call(n=-1) == ERR_SHAPE
    assert call(h=0) == ERR_SHAPE
    assert call(w=0, kind=3, params=()) == ERR_SHAPE
    assert call(kind=1, params=(0.02, 0.02), h=1) == ERR_SHAPE
    assert call(kind=1, params=(0.02, 0.02), w=1) == ERR_SHAPE
    assert call(h=32768, w=32768) == ERR_SHAPE                        # H*W*3 >= 2^31
    assert call(h=1 << 14, w=43691) == ERR_SHAPE                      # 2^31 + 2^14 subpixels


def test_python_layer_rejects_cpu_tensors_and_unknown_names():
    from celebrity_image_denoiser_amd import noise

    x = torch.zeros(2, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        noise.add_noise(x, "gaussian")
    with pytest.raises(ValueError):
        noise.add_noise(x, "pink")
    with pytest.raises(TypeError):
        noise.add_noise(x, "gaussian", salt_prob=0.1)
    with pytest.raises(RuntimeError):
        noise.add_noise(torch.zeros(2, 3, 16, 16), "uniform")
    with pytest.raises(ValueError):
        noise.evaluate_noise_types(None, torch.zeros(2, 18, 16, 3, dtype=torch.uint8))
    import celebrity_image_denoiser_amd as cid

    assert cid.add_noise is noise.add_noise and cid.NOISE_TYPES == KINDS


# ---------------------------------------------------------------- on the MI355X
DEV = "cuda:0"


def _gpu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _inputs(n, h, w, first_index):
    """Smooth clean images, with every other image replaced by uniform random bytes (every value, both clip edges)."""
    x = synth.clean_images_u8(n, h, w, first_index)
    for i in range(1, n, 2):
        x[i] = np.floor(synth.hash_uniform(first_index + i, 99, h * w * 3) * 256).astype(np.uint8).reshape(h, w, 3)
    return x


def _device(clean, kind, **kw):
    from celebrity_image_denoiser_amd import noise

    out = noise.add_noise(_gpu(clean), kind, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _assert_matches(got, clean, kind, seed, first_index):
    ref = synth.add_noise_np(clean, kind, seed, first_index)
    diff = got != ref
    if kind in ("gaussian", "speckle"):
        v = synth.noise_values_np(clean, kind, seed, first_index)
        near = (np.abs(v - np.round(v)) < 1e-9) | (np.abs(v) < 1e-9) | (np.abs(v - 255.0) < 1e-9)
        assert not np.any(diff & ~near), f"{kind}: {int(diff.sum())} mismatches, {int((diff & ~near).sum())} away from an edge"
        assert int(diff.sum()) <= 4, f"{kind}: {int(diff.sum())} mismatches at near-integer values"
    else:
        assert not diff.any(), f"{kind}: {int(diff.sum())} of {diff.size} bytes differ"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(8, 128, 128), (8, 37, 53), (8, 256, 256), (1, 1440, 1920)])
@pytest.mark.parametrize("kind", KINDS)
def test_device_equals_restatement(kind, shape):
    n, h, w = shape
    clean = _inputs(n, h, w, 500 + h)
    for seed, fi in ((synth.NOISE_SEED, 0), (12345, 77), (2 ** 64 - 3, 1000)):
        got = _device(clean, kind, seed=seed, first_index=fi)
        _assert_matches(got, clean, kind, seed, fi)


@pytest.mark.gpu
def test_device_gaussian_is_the_bench_input():
    for fi in (0, 900):
        clean = synth.clean_images_u8(4, 96, 128, first_index=fi)
        assert np.array_equal(_device(clean, "gaussian", first_index=fi), synth.add_gaussian_noise(clean, 25.0, fi))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_non_default_parameters(kind):
    params = {"gaussian": dict(mean=3.5, sigma=40.0), "speckle": dict(mean=-0.2, sigma=0.5),
              "uniform": dict(low=-30.0, high=10.0), "salt_pepper": dict(salt_prob=0.3, pepper_prob=0.1), "poisson": {}}[kind]
    clean = _inputs(4, 64, 80, 50)
    got = _device(clean, kind, seed=8, first_index=3, **params)
    ref = synth.add_noise_np(clean, kind, 8, 3, **params)
    if kind in ("gaussian", "speckle"):
        v = synth.noise_values_np(clean, kind, 8, 3, **params)
        near = (np.abs(v - np.round(v)) < 1e-9) | (np.abs(v) < 1e-9) | (np.abs(v - 255.0) < 1e-9)
        assert not np.any((got != ref) & ~near)
    else:
        assert np.array_equal(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_batch_independence(kind):
    from celebrity_image_denoiser_amd import noise

    clean = _gpu(_inputs(64, 64, 48, 20))
    full = noise.add_noise(clean, kind, seed=5, first_index=100)
    for k in (0, 1, 37, 63):
        alone = noise.add_noise(clean[k:k + 1], kind, seed=5, first_index=100 + k)
        assert torch.equal(alone[0], full[k]), (kind, k)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_in_place_equals_out_of_place(kind):
    from celebrity_image_denoiser_amd import noise

    clean = _gpu(_inputs(6, 72, 88, 30))
    ref = noise.add_noise(clean, kind, first_index=4)
    buf = clean.clone()
    got = noise.add_noise(buf, kind, first_index=4, out=buf)
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(buf, ref)


@pytest.mark.gpu
def test_no_write_outside_the_output():
    from celebrity_image_denoiser_amd import noise

    n, h, w = 256, 256, 256
    total, guard = n * h * w * 3, 1 << 16
    clean = _gpu(_inputs(2, h, w, 40)).repeat(n // 2, 1, 1, 1).contiguous()
    for kind in KINDS:
        buf = torch.full((total + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
        out = buf[guard:guard + total].view(n, h, w, 3)
        noise.add_noise(clean, kind, out=out)
        inplace = torch.full((total + 2 * guard,), 0x5A, dtype=torch.uint8, device=DEV)
        view = inplace[guard:guard + total].view(n, h, w, 3)
        view.copy_(clean)
        noise.add_noise(view, kind, out=view)
        torch.cuda.synchronize()
        for g, val in ((buf, 0xA5), (inplace, 0x5A)):
            assert bool((g[:guard] == val).all()) and bool((g[guard + total:] == val).all()), kind
        assert torch.equal(out, view), kind
        for i in (0, 1, 255):
            _assert_matches(out[i:i + 1].cpu().numpy(), clean[i:i + 1].cpu().numpy(), kind, synth.NOISE_SEED, i)


@pytest.mark.gpu
def test_runs_on_a_non_default_stream():
    from celebrity_image_denoiser_amd import noise

    clean = _inputs(8, 128, 128, 60)
    x = _gpu(clean)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    outs = {}
    with torch.cuda.stream(s):
        for kind in KINDS:
            outs[kind] = noise.add_noise(x, kind, first_index=6)
    s.synchronize()
    for kind in KINDS:
        _assert_matches(outs[kind].cpu().numpy(), clean, kind, synth.NOISE_SEED, 6)


@pytest.mark.gpu
def test_evaluate_noise_types_is_the_hand_composed_loop(weight_sets):
    import celebrity_image_denoiser_amd as cid
    from celebrity_image_denoiser_amd import metrics, noise

    model = cid.load(weight_sets["default"], device=DEV, strict=True)
    clean = _gpu(synth.clean_images_u8(16, 256, 256, first_index=70))
    res = noise.evaluate_noise_types(model, clean, first_index=70)
    assert tuple(res) == KINDS
    for kind in KINDS:
        noisy = noise.add_noise(clean, kind, first_index=70)
        q = metrics.quality(model.forward_u8(noisy, out_u8=False), clean)
        ref = {m: float(q[m].cpu().numpy().mean()) for m in ("psnr", "ssim", "ms_ssim")}
        ref["psnr_noisy"] = float(metrics.quality(noisy, clean, ("psnr",))["psnr"].cpu().numpy().mean())
        assert res[kind] == ref, kind
        assert all(math.isfinite(v) for v in res[kind].values()), (kind, res[kind])
    split = noise.evaluate_noise_types(model, clean, kinds=("poisson",), first_index=70, max_batch=5)
    assert split["poisson"]["psnr_noisy"] == res["poisson"]["psnr_noisy"]      # the noise does not depend on the split
    small = noise.evaluate_noise_types(model, clean[:2, :128, :128].contiguous(), kinds="uniform")
    assert set(small["uniform"]) == {"psnr_noisy", "psnr", "ssim"}
