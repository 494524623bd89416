"""LPIPS(net='alex') on the GPU: cid_lpips (include/cid.h, which holds the definition), lpips.py and its users in metrics.py / noise.py.

The reference for error is tests/lpips_oracle.py in float64.  Bounds, as the feature's issue sets them:
  taps    relu1 ... relu5 through cid_lpips_stage_view: max|delta| <= 1e-5 * max(1, max|ref|) per tensor (lpips_oracle.bound)
  d_k, d  |delta| <= 1e-5 * |ref| per value: relative, because the distances are small (5e-4 ... 3e-2 here)
ATen fp32 on a plain torch.nn build of the same network stands at most 1.4e-6 of the tap scale and 3.8e-6 relative on the distances
over every case below (tests/golden/lpips_stats.json, asserted by make_lpips_golden.py at 5x inside the tap rule).

Shapes (lpips_oracle.CASES): 31x31 (every late map one pixel: the GEMM's column tiles run across images) at N = 1, 2, 5; 35x47 (maps
8x11 -> 3x5 -> 1x2, the pool drops a row, partial last column tile) at N = 3, 19; 67x33; 64x64; 128x128 (the trainers' size); 200x136
(more than one workgroup per map).  Operands: noisy / clean pairs (small distances) and unrelated pairs (ordinary ones)."""
import os
import sys

import numpy as np
import pytest
import torch

import celebrity_image_denoiser_amd as cid
from celebrity_image_denoiser_amd import metrics, synth
from celebrity_image_denoiser_amd.lpips import load_lpips

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = list(lpips_oracle.CASES)
_MODELS, _REFS, _PAIRS = {}, {}, {}


def model_of(wset):
    if wset not in _MODELS:
        sd = {k: torch.from_numpy(v) for k, v in synth.make_lpips_state_dict(wset).items()}
        _MODELS[wset] = load_lpips(sd, device=DEV, strict=True)
    return _MODELS[wset]


def first_index(h, w, n):
    return 5000 + 100 * h + w + n


def pairs_of(kind, case):
    key = (kind, case)
    if key not in _PAIRS:
        h, w, n = case
        _PAIRS[key] = lpips_oracle.pairs(kind, n, h, w, first_index(h, w, n))
        for v in _PAIRS[key]:
            v.setflags(write=False)
    return _PAIRS[key]


def reference(wset, kind, case, unit):
    """The float64 oracle of one case: computed once, shared, never modified."""
    key = (wset, kind, case, unit)
    if key not in _REFS:
        a, b, _, _ = pairs_of(kind, case)
        ref = lpips_oracle.forward(synth.make_lpips_state_dict(wset), a, b, unit)
        for v in ref.values():
            v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def check_taps(m, ref, case, what):
    h, w, n = case
    for name in lpips_oracle.TAPS:
        got = m.stage(name, n, h, w).cpu().numpy()
        bound = lpips_oracle.bound(ref[name])
        err = float(np.abs(got.astype(np.float64) - ref[name]).max())
        print(f"{what} {name}: max|delta| {err:.3e}, bound {bound:.3e} (margin {bound / max(err, 1e-300):.1f}x), max|ref| {np.abs(ref[name]).max():.4g}")
        assert got.shape == ref[name].shape, (what, name)
        assert np.isfinite(got).all(), (what, name)
        assert err <= bound, (what, name, err, bound)


def check_distances(d, layers, ref, what):
    rel_l = np.abs(layers - ref["layers"]) / np.abs(ref["layers"])
    rel_d = np.abs(d - ref["d"]) / np.abs(ref["d"])
    print(f"{what}: d in [{ref['d'].min():.3e}, {ref['d'].max():.3e}], max rel delta layers {rel_l.max():.3e}, d {rel_d.max():.3e} (bound 1e-5)")
    assert (np.abs(layers - ref["layers"]) <= 1e-5 * np.abs(ref["layers"])).all(), (what, rel_l.max())
    assert (np.abs(d - ref["d"]) <= 1e-5 * np.abs(ref["d"])).all(), (what, rel_d.max())


def run(wset, kind, case, unit):
    m = model_of(wset)
    a, b, _, _ = pairs_of(kind, case)
    d, layers = m.distances(dev(a), dev(b), unit_view=unit, per_layer=True)
    ref = reference(wset, kind, case, unit)
    what = f"{wset} {kind} {case} unit={int(unit)}"
    check_taps(m, ref, case, what)
    check_distances(d.cpu().numpy(), layers.cpu().numpy(), ref, what)


@pytest.mark.parametrize("wset", ["default", "hot"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}n{c[2]}")
def test_parity(case, wset):
    """Taps and distances of every shape: the trainers' call (x*0.5+0.5) on noisy / clean pairs, the plain call on unrelated pairs."""
    run(wset, "noisy", case, True)
    run(wset, "unrelated", case, False)


@pytest.mark.parametrize("wset", ["default", "hot"])
@pytest.mark.parametrize("case", [(35, 47, 3), (128, 128, 3)], ids=lambda c: f"{c[0]}x{c[1]}n{c[2]}")
def test_parity_other_flag(case, wset):
    """The other pairing of operands and flag."""
    run(wset, "noisy", case, False)
    run(wset, "unrelated", case, True)


@pytest.mark.parametrize("wset", ["default", "hot"])
def test_fixture_and_module_call(wset):
    """Against the recorded ATen fp32 values (two fp32 results: twice the bound), through the package's call signature."""
    m = model_of(wset)
    case = (64, 64, 2)
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"lpips_{wset}_unrelated_64x64_n2.npz"))
    assert not bool(fx["unit_view"]) and int(fx["first_index"]) == first_index(*case)
    a, b, _, _ = pairs_of("unrelated", case)
    out, per = m(dev(a), dev(b), retPerLayer=True)
    assert out.dtype == torch.float32 and tuple(out.shape) == (2, 1, 1, 1) and len(per) == 5 and tuple(per[0].shape) == (2, 1, 1, 1)
    ref = reference(wset, "unrelated", case, False)
    # the package's fp32 return value: the distance bound plus half an fp32 ulp of the cast
    assert (np.abs(out.cpu().numpy().reshape(-1).astype(np.float64) - ref["d"]) <= (1e-5 + 2.0 ** -24) * ref["d"]).all()
    assert (np.abs(out.cpu().numpy().reshape(-1).astype(np.float64) - fx["d"]) <= 2e-5 * np.abs(fx["d"])).all()
    got5 = m.stage("relu5", 2, 64, 64).cpu().numpy()
    assert np.abs(got5 - fx["relu5"]).max() <= 2 * lpips_oracle.bound(ref["relu5"])
    # normalize=True: [0,1] operands, 2*x - 1 first: the plain call on the same images up to the fp32 rounding of that round trip
    out_n = m(dev(a) * 0.5 + 0.5, dev(b) * 0.5 + 0.5, normalize=True)
    assert (np.abs(out_n.cpu().numpy().reshape(-1) - ref["d"]) <= 1e-4 * ref["d"]).all()


def test_identity_symmetry_and_formats():
    m = model_of("hot")
    case = (35, 47, 3)
    a, b, a8, b8 = pairs_of("noisy", case)
    ta, tb, ta8, tb8 = dev(a), dev(b), dev(a8), dev(b8)
    for unit in (False, True):
        d_aa, l_aa = m.distances(ta, ta, unit_view=unit, per_layer=True)
        assert np.array_equal(d_aa.cpu().numpy(), np.zeros(3)) and np.array_equal(l_aa.cpu().numpy(), np.zeros((3, 5)))     # exactly 0.0
        d_ab, l_ab = m.distances(ta, tb, unit_view=unit, per_layer=True)
        d_ba, l_ba = m.distances(tb, ta, unit_view=unit, per_layer=True)
        assert torch.equal(d_ab, d_ba) and torch.equal(l_ab, l_ba)                                                          # bit for bit
        # a uint8 operand is read as (u/255 - 0.5)/0.5: the same bits as its normalised fp32 copy, in every mix
        for x, y in ((ta8, tb), (ta, tb8), (ta8, tb8)):
            d, l = m.distances(x, y, unit_view=unit, per_layer=True)
            assert torch.equal(d, d_ab) and torch.equal(l, l_ab)
        check_distances(d_ab.cpu().numpy(), l_ab.cpu().numpy(), reference("hot", "noisy", case, unit), f"formats unit={int(unit)}")
    assert torch.equal(metrics.lpips(ta8, tb, m, unit_view=True), d_ab)


def test_batch_position_independence():
    """An image pair's result has the same bits alone and at any position of a 19-image batch."""
    m = model_of("default")
    case = (35, 47, 19)
    a, b, _, _ = pairs_of("unrelated", case)
    ta, tb = dev(a), dev(b)
    d19, l19 = m.distances(ta, tb, per_layer=True)
    taps19 = m.stage("relu5", 19, 35, 47)
    for i in (0, 7, 18):
        d1, l1 = m.distances(ta[i:i + 1], tb[i:i + 1], per_layer=True)
        assert torch.equal(d1[0], d19[i]) and torch.equal(l1[0], l19[i]), i
        t1 = m.stage("relu5", 1, 35, 47)
        assert torch.equal(t1[0], taps19[i]) and torch.equal(t1[1], taps19[19 + i]), i
    perm = torch.tensor([(7 * i + 3) % 19 for i in range(19)], device=DEV)
    dp = m.distances(ta[perm].contiguous(), tb[perm].contiguous())
    assert torch.equal(dp, d19[perm])
    d5 = m.distances(ta[11:16].contiguous(), tb[11:16].contiguous())
    assert torch.equal(d5, d19[11:16])


def test_workspace_hygiene():
    """Results do not depend on what the workspace held, and nothing past it is written."""
    import ctypes

    from celebrity_image_denoiser_amd import _lib

    m = model_of("default")
    case = (35, 47, 3)
    a, b, _, _ = pairs_of("noisy", case)
    ta, tb = dev(a), dev(b)
    want, want_l = m.distances(ta, tb, unit_view=True, per_layer=True)
    need = ctypes.c_size_t()
    assert _lib.lib().cid_lpips_workspace_bytes(3, 35, 47, ctypes.byref(need)) == 0
    guard = 4096
    buf = torch.empty(need.value + guard, dtype=torch.uint8, device=DEV)
    buf[:need.value].view(torch.float32).fill_(float("nan"))
    buf[need.value:] = 0xA5
    out = torch.empty(3, dtype=torch.float64, device=DEV)
    lay = torch.empty((3, 5), dtype=torch.float64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check_lpips(m._cid, _lib.lib().cid_lpips(m._cid, ta.data_ptr(), 0, tb.data_ptr(), 0, 3, 35, 47, _lib.CID_LPIPS_UNIT_VIEW,
                                                  out.data_ptr(), lay.data_ptr(), buf.data_ptr(), need.value, stream))
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(lay, want_l)
    assert bool((buf[need.value:] == 0xA5).all())


def test_dead_first_layer():
    """A first bias that drives relu1 to all zeros: 0 / (0 + 1e-10) = 0, so d_0 = 0 and the total is finite."""
    sd = {k: torch.from_numpy(v.copy()) for k, v in synth.make_lpips_state_dict("default").items()}
    sd["net.slice1.0.bias"] = torch.full((64,), -1e4)
    sd["net.slice2.3.bias"] = sd["net.slice2.3.bias"].abs() + 0.1     # relu2 lives on its bias alone
    m = load_lpips(sd, device=DEV, strict=True)
    a, b, _, _ = pairs_of("unrelated", (31, 31, 2))
    d, layers = m.distances(dev(a), dev(b), per_layer=True)
    assert float(m.stage("relu1", 2, 31, 31).abs().max()) == 0.0
    assert np.array_equal(layers[:, 0].cpu().numpy(), np.zeros(2))
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(layers).all())
    assert float(m.stage("relu2", 2, 31, 31).max()) > 0.0


def test_shape_errors():
    m = model_of("default")
    x = torch.zeros(1, 3, 30, 64, device=DEV)
    with pytest.raises(ValueError, match="31"):
        m.distances(x, x)
    with pytest.raises(ValueError, match="31"):
        metrics.lpips(torch.zeros(1, 64, 30, 3, dtype=torch.uint8, device=DEV), torch.zeros(1, 64, 30, 3, dtype=torch.uint8, device=DEV), m)
    with pytest.raises(ValueError):
        cid.quality(x, x, ("lpips",))


def test_evaluate_and_noise_types():
    m = model_of("default")
    case = (128, 128, 3)
    a, b, _, _ = pairs_of("noisy", case)
    ta, tb = dev(a), dev(b)
    ref = reference("default", "noisy", case, True)
    psnr, ssim, lp, ms = cid.evaluate(ta, tb, ms_ssim=False, lpips=m)
    want = float(ref["d"].mean())
    print(f"evaluate lpips {lp:.9e}, oracle mean {want:.9e}")
    assert abs(lp - want) <= 1e-5 * want and ms == 0.0
    base = cid.evaluate(ta, tb, ms_ssim=False)
    assert base[2] == 0.0 and base[0] == psnr and base[1] == ssim          # without a model it stays 0.0

    gen = cid.load(synth.make_state_dict("default"), device=DEV, strict=True)
    clean = dev(synth.clean_images_u8(2, 32, 32, 40))
    r = cid.evaluate_noise_types(gen, clean, kinds=("gaussian", "uniform"), lpips=m)
    r0 = cid.evaluate_noise_types(gen, clean, kinds=("gaussian", "uniform"))
    for kind in ("gaussian", "uniform"):
        assert "lpips" in r[kind] and "lpips" not in r0[kind] and np.isfinite(r[kind]["lpips"]) and r[kind]["lpips"] > 0
        assert {k: v for k, v in r[kind].items() if k != "lpips"} == r0[kind]
        noisy = cid.add_noise(clean, kind)
        den = gen.forward_u8(noisy, out_u8=False)
        assert r[kind]["lpips"] == float(metrics.lpips(den, clean, m, unit_view=True).cpu().numpy().mean())


def test_more_than_65535_images_in_one_call():
    """2 N = 65,540 images: the head's grid y is split after image 65,535 (tower b's image 32,767 of 32,770), as in the existing
    forwards.  The pairs repeat five base pairs, so every result must equal, bit for bit, the one a 5-pair call gives."""
    m = model_of("default")
    n = 32770
    a, b, _, _ = pairs_of("unrelated", (31, 31, 5))
    ta, tb = dev(a), dev(b)
    want = m.distances(ta, tb)
    idx = torch.arange(n, device=DEV) % 5
    got = m.distances(ta[idx].contiguous(), tb[idx].contiguous())
    assert torch.equal(got, want[idx])
    m._ws = None   # 1.5 GB: not kept for the rest of the session
