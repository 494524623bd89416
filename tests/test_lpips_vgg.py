"""VGG16 features on the GPU: cid_vgg_lpips and cid_vgg_content_loss (include/cid.h, which holds the definitions), LPIPS(net='vgg') and
VGGPerceptualLoss in lpips.py.

The reference for error is tests/lpips_vgg_oracle.py in float64.  Bounds, the project's own rules:
  taps         through cid_vgg_stage_view: max|delta| <= 1e-5 * max(1, max|ref|) per tensor (lpips_oracle.bound)
  d_k, d, loss |delta| <= 1e-5 * |ref| per value
ATen fp32 on a plain torch.nn build of the same network stands at most 8.6e-7 of the tap scale, 6.3e-6 relative on the distances and
1.1e-6 on the content loss over every case below (tests/golden/lpips_vgg_stats.json, asserted by make_lpips_vgg_golden.py at 5x inside
the tap rule).

Shapes (lpips_vgg_oracle.CASES): 16x16 (the smallest: relu5 is 1x1) at N = 1, 2 and 70 (one 128-column run of relu5 spans 128
images); 17x19 (odd floors at every pool); 35x47 at N = 3, 19 (runs that cross image boundaries); 64x64, 96x72, 128x128; 20x264 and
264x20 (past the 254-wide staging plane); 16x512 (the widest accepted map).  Content loss: 4x4 (the smallest), 5x7, 35x47, 64x64,
128x128."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import celebrity_image_denoiser_amd as cid
from celebrity_image_denoiser_amd import _lib, metrics, synth
from celebrity_image_denoiser_amd.lpips import load_lpips, load_vgg_loss

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_vgg_oracle as oracle  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_MODELS, _LOSSES, _REFS, _CREFS, _PAIRS = {}, {}, {}, {}, {}
case_id = lambda c: f"{c[0]}x{c[1]}n{c[2]}"   # noqa: E731


def model_of(wset):
    if wset not in _MODELS:
        sd = {k: torch.from_numpy(v) for k, v in oracle.weights(wset).items()}
        _MODELS[wset] = load_lpips(sd, device=DEV, strict=True, net="vgg")
    return _MODELS[wset]


def loss_of(wset):
    if wset not in _LOSSES:
        sd = {k: torch.from_numpy(v) for k, v in synth.vgg_loss_state_dict(oracle.weights(wset)).items()}
        _LOSSES[wset] = load_vgg_loss(sd, device=DEV)
    return _LOSSES[wset]


def pairs_of(kind, case):
    key = (kind, case)
    if key not in _PAIRS:
        h, w, n = case
        _PAIRS[key] = oracle.pairs(kind, n, h, w, oracle.first_index(h, w, n))
        for v in _PAIRS[key]:
            v.setflags(write=False)
    return _PAIRS[key]


def reference(wset, kind, case, unit):
    """The float64 oracle of one case: computed once, shared, never modified."""
    key = (wset, kind, case, unit)
    if key not in _REFS:
        a, b, _, _ = pairs_of(kind, case)
        ref = oracle.forward(oracle.weights(wset), a, b, unit)
        for v in ref.values():
            v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def content_reference(wset, kind, case):
    key = (wset, kind, case)
    if key not in _CREFS:
        a, b, _, _ = pairs_of(kind, case)
        ref = oracle.content(oracle.weights(wset), a, b)
        for v in ref.values():
            v.setflags(write=False)
        _CREFS[key] = ref
    return _CREFS[key]


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def check_taps(m, ref, case, what, names=oracle.TAPS):
    h, w, n = case
    for name in names:
        got = m.stage(name, n, h, w).cpu().numpy()
        bound = oracle.bound(ref[name])
        err = float(np.abs(got.astype(np.float64) - ref[name]).max())
        print(f"{what} {name}: max|delta| {err:.3e}, bound {bound:.3e} (margin {bound / max(err, 1e-300):.1f}x), max|ref| {np.abs(ref[name]).max():.4g}")
        assert got.shape == ref[name].shape, (what, name)
        assert np.isfinite(got).all(), (what, name)
        assert err <= bound, (what, name, err, bound)


def check_values(got, want, what):
    rel = np.abs(got - want) / np.abs(want)
    print(f"{what}: in [{want.min():.3e}, {want.max():.3e}], max rel delta {rel.max():.3e} (bound 1e-5)")
    assert (np.abs(got - want) <= 1e-5 * np.abs(want)).all(), (what, rel.max())


def run(wset, kind, case, unit):
    m = model_of(wset)
    a, b, _, _ = pairs_of(kind, case)
    d, layers = m.distances(dev(a), dev(b), unit_view=unit, per_layer=True)
    ref = reference(wset, kind, case, unit)
    what = f"{wset} {kind} {case} unit={int(unit)}"
    check_taps(m, ref, case, what)
    check_values(layers.cpu().numpy(), ref["layers"], what + " layers")
    check_values(d.cpu().numpy(), ref["d"], what + " d")


@pytest.mark.parametrize("wset", ["default", "hot"])
@pytest.mark.parametrize("case", oracle.CASES, ids=case_id)
def test_parity(case, wset):
    """Taps and distances of every shape: the trainer's call (x*0.5+0.5) on noisy / clean pairs, the plain call on unrelated pairs."""
    run(wset, "noisy", case, True)
    run(wset, "unrelated", case, False)


@pytest.mark.parametrize("wset", ["default", "hot"])
@pytest.mark.parametrize("case", oracle.CASES, ids=case_id)
def test_parity_other_flag(case, wset):
    """The other pairing of operands and flag."""
    run(wset, "noisy", case, False)
    run(wset, "unrelated", case, True)


@pytest.mark.parametrize("wset", ["default", "hot"])
@pytest.mark.parametrize("case", oracle.CONTENT_CASES, ids=case_id)
def test_content_loss_parity(case, wset):
    """relu1_2, relu2_2 and relu3_3 of the unscaled operands and the per-pair loss; forward() is the mean of per_image()."""
    m = loss_of(wset)
    h, w, n = case
    for kind in ("noisy", "unrelated"):
        a, b, _, _ = pairs_of(kind, case)
        ref = content_reference(wset, kind, case)
        per = m.per_image(dev(a), dev(b))
        what = f"content {wset} {kind} {case}"
        assert per.dtype == torch.float64 and tuple(per.shape) == (n,)
        check_taps(m, ref, case, what, oracle.TAPS[:3])
        check_values(per.cpu().numpy(), ref["loss"], what + " loss")
        out = m(dev(a), dev(b))
        assert out.dtype == torch.float32 and out.dim() == 0 and not out.requires_grad
        assert torch.equal(out, per.mean().to(torch.float32))
        with pytest.raises(KeyError):
            m.stage("relu4", n, h, w)


@pytest.mark.parametrize("wset", ["default", "hot"])
def test_fixture_and_module_call(wset):
    """Against the recorded ATen fp32 values (two fp32 results: twice the bound), through the package's call signature."""
    m = model_of(wset)
    case = (64, 64, 2)
    fx = np.load(os.path.join(GOLDEN, f"lpips_vgg_{wset}_unrelated_64x64_n2.npz"))
    assert not bool(fx["unit_view"]) and int(fx["first_index"]) == oracle.first_index(*case)
    a, b, _, _ = pairs_of("unrelated", case)
    out, per = m(dev(a), dev(b), retPerLayer=True)
    assert out.dtype == torch.float32 and tuple(out.shape) == (2, 1, 1, 1) and len(per) == 5 and tuple(per[0].shape) == (2, 1, 1, 1)
    ref = reference(wset, "unrelated", case, False)
    got = out.cpu().numpy().reshape(-1).astype(np.float64)
    # the package's fp32 return value: the distance bound plus half an fp32 ulp of the cast
    assert (np.abs(got - ref["d"]) <= (1e-5 + 2.0 ** -24) * ref["d"]).all()
    assert (np.abs(got - fx["d"]) <= 2e-5 * np.abs(fx["d"])).all()
    got_l = np.stack([p.cpu().numpy().reshape(-1) for p in per], axis=1).astype(np.float64)
    assert (np.abs(got_l - fx["layers"]) <= 2e-5 * np.abs(fx["layers"])).all()
    got5 = m.stage("relu5", 2, 64, 64).cpu().numpy()
    assert np.abs(got5 - fx["relu5"]).max() <= 2 * oracle.bound(ref["relu5"])
    # normalize=True: [0,1] operands, 2*x - 1 first: the plain call on the same images up to the fp32 rounding of that round trip
    out_n = m(dev(a) * 0.5 + 0.5, dev(b) * 0.5 + 0.5, normalize=True)
    assert (np.abs(out_n.cpu().numpy().reshape(-1) - ref["d"]) <= 1e-4 * ref["d"]).all()
    # the content loss of the same operands
    loss = loss_of(wset).per_image(dev(a), dev(b)).cpu().numpy()
    assert (np.abs(loss - fx["loss"]) <= 2e-5 * np.abs(fx["loss"])).all()


@pytest.mark.parametrize("wset", ["default", "hot"])
def test_packed_blob(wset):
    """The uploaded weight blob is the numpy restatement of the packed layout, word for word; the content-loss handle's blob has the
    same first seven convolutions and zeros elsewhere."""
    want = oracle.packed_blob(oracle.weights(wset))
    got = model_of(wset).pack_weights().view(torch.float32).cpu().numpy()
    assert np.array_equal(got, want)
    got_c = loss_of(wset).pack_weights().view(torch.float32).cpu().numpy()
    end = 27 * 64 + 128 + sum(co * ci * 9 + co for ci, co in ((64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256)))
    want_c = want.copy()
    want_c[27 * 64 + 64:27 * 64 + 128] = 0          # no scaling layer
    want_c[end:] = 0
    assert np.array_equal(got_c, want_c)


def test_identity_symmetry_and_formats():
    m, cl = model_of("hot"), loss_of("hot")
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
        check_values(d_ab.cpu().numpy(), reference("hot", "noisy", case, unit)["d"], f"formats unit={int(unit)}")
    assert torch.equal(metrics.lpips(ta8, tb, m, unit_view=True), d_ab)
    c_ab = cl.per_image(ta, tb)
    assert np.array_equal(cl.per_image(ta, ta).cpu().numpy(), np.zeros(3))
    assert torch.equal(cl.per_image(tb, ta), c_ab)
    for x, y in ((ta8, tb), (ta, tb8), (ta8, tb8)):
        assert torch.equal(cl.per_image(x, y), c_ab)


@pytest.mark.parametrize("case,picks", [((16, 16, 70), (0, 1, 63, 64, 69)), ((35, 47, 19), (0, 7, 18))], ids=["16x16n70", "35x47n19"])
def test_batch_position_independence(case, picks):
    """An image pair's result has the same bits alone and at any position of the batch.  At 16x16 relu5 is one pixel per image and
    relu4 four, relu3 sixteen: 128-column runs hold 128, 32 and 8 images and the 140 images cross their boundaries at different
    places; at 35x47 every map's runs cross image boundaries mid-row."""
    m = model_of("default")
    h, w, n = case
    a, b, _, _ = pairs_of("unrelated", case)
    ta, tb = dev(a), dev(b)
    dn, ln = m.distances(ta, tb, per_layer=True)
    taps_n = [m.stage(name, n, h, w) for name in ("relu3", "relu5")]
    for i in picks:
        d1, l1 = m.distances(ta[i:i + 1], tb[i:i + 1], per_layer=True)
        assert torch.equal(d1[0], dn[i]) and torch.equal(l1[0], ln[i]), i
        for name, tn in zip(("relu3", "relu5"), taps_n):
            t1 = m.stage(name, 1, h, w)
            assert torch.equal(t1[0], tn[i]) and torch.equal(t1[1], tn[n + i]), (i, name)
    perm = torch.tensor([(7 * i + 3) % n for i in range(n)], device=DEV)
    assert torch.equal(m.distances(ta[perm].contiguous(), tb[perm].contiguous()), dn[perm])
    assert torch.equal(m.distances(ta[11:16].contiguous(), tb[11:16].contiguous()), dn[11:16])
    cl = loss_of("default")
    cn = cl.per_image(ta, tb)
    assert torch.equal(cl.per_image(ta[perm].contiguous(), tb[perm].contiguous()), cn[perm])
    assert torch.equal(cl.per_image(ta[5:6], tb[5:6])[0], cn[5])


def test_workspace_hygiene():
    """Results do not depend on what the workspace or the LDS held, and nothing past the workspace is written."""
    m, cl = model_of("default"), loss_of("default")
    case = (35, 47, 3)
    a, b, _, _ = pairs_of("noisy", case)
    ta, tb = dev(a), dev(b)
    want, want_l = m.distances(ta, tb, unit_view=True, per_layer=True)
    want_c = cl.per_image(ta, tb)
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    guard = 4096
    for form in (_lib.CID_VGG_LPIPS, _lib.CID_VGG_CONTENT):
        need = ctypes.c_size_t()
        assert L.cid_vgg_workspace_bytes(form, 3, 35, 47, ctypes.byref(need)) == 0
        buf = torch.empty(need.value + guard, dtype=torch.uint8, device=DEV)
        buf[:need.value].view(torch.float32).fill_(float("nan"))
        buf[need.value:] = 0xA5
        out = torch.empty(3, dtype=torch.float64, device=DEV)
        lay = torch.empty((3, 5), dtype=torch.float64, device=DEV)
        assert L.cid_debug_poison_lds(stream) == 0
        if form == _lib.CID_VGG_LPIPS:
            _lib.check_vgg(m._cid, L.cid_vgg_lpips(m._cid, ta.data_ptr(), 0, tb.data_ptr(), 0, 3, 35, 47, _lib.CID_LPIPS_UNIT_VIEW,
                                                   out.data_ptr(), lay.data_ptr(), buf.data_ptr(), need.value, stream))
            torch.cuda.synchronize()
            assert torch.equal(out, want) and torch.equal(lay, want_l)
        else:
            _lib.check_vgg(cl._cid, L.cid_vgg_content_loss(cl._cid, ta.data_ptr(), 0, tb.data_ptr(), 0, 3, 35, 47, 0, out.data_ptr(),
                                                           buf.data_ptr(), need.value, stream))
            torch.cuda.synchronize()
            assert torch.equal(out, want_c)
        assert bool((buf[need.value:] == 0xA5).all())


def test_dead_first_layer():
    """A first bias that drives relu1_1 to all zeros, and a second one that does the same to relu1_2: 0 / (0 + 1e-10) = 0, so d_0 = 0
    and the total is finite; the later layers live on their biases."""
    sd = {k: torch.from_numpy(v.copy()) for k, v in oracle.weights("default").items()}
    sd["net.slice1.0.bias"] = torch.full((64,), -1e4)
    sd["net.slice1.2.bias"] = -sd["net.slice1.2.bias"].abs() - 0.1
    sd["net.slice2.5.bias"] = sd["net.slice2.5.bias"].abs() + 0.1
    m = load_lpips(sd, device=DEV, strict=True, net="vgg")
    a, b, _, _ = pairs_of("unrelated", (16, 16, 2))
    d, layers = m.distances(dev(a), dev(b), per_layer=True)
    assert float(m.stage("relu1", 2, 16, 16).abs().max()) == 0.0
    assert np.array_equal(layers[:, 0].cpu().numpy(), np.zeros(2))
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(layers).all())
    assert float(m.stage("relu2", 2, 16, 16).max()) > 0.0


def test_errors():
    m, cl = model_of("default"), loss_of("default")
    x = torch.zeros(1, 3, 15, 64, device=DEV)
    with pytest.raises(ValueError, match="16"):
        m.distances(x, x)
    with pytest.raises(ValueError, match="16"):
        metrics.lpips(torch.zeros(1, 64, 15, 3, dtype=torch.uint8, device=DEV), torch.zeros(1, 64, 15, 3, dtype=torch.uint8, device=DEV), m)
    wide = torch.zeros(1, 3, 16, 513, device=DEV)
    with pytest.raises(ValueError, match="512"):
        m.distances(wide, wide)
    with pytest.raises(ValueError, match="512"):
        cl(wide, wide)
    with pytest.raises(ValueError, match="4"):
        cl(torch.zeros(1, 3, 3, 8, device=DEV), torch.zeros(1, 3, 3, 8, device=DEV))
    assert float(cl(x, x)) == 0.0                       # side 15 is fine for the content loss
    with pytest.raises(RuntimeError, match="GPU-only"):
        m.distances(x.cpu(), x.cpu())
    with pytest.raises(RuntimeError, match="GPU-only"):
        cl(x.cpu(), x.cpu())
    with pytest.raises(ValueError, match="same dimensions"):
        cl(x, torch.zeros(1, 3, 16, 64, device=DEV))
    # a content-loss handle does not serve the metric: CID_ERR_STATE
    need = ctypes.c_size_t()
    L = _lib.lib()
    assert L.cid_vgg_workspace_bytes(_lib.CID_VGG_LPIPS, 1, 16, 16, ctypes.byref(need)) == 0
    buf = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    y = torch.zeros(1, 3, 16, 16, device=DEV)
    out = torch.empty(1, dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.CidError) as e:
        _lib.check_vgg(cl._cid, L.cid_vgg_lpips(cl._cid, y.data_ptr(), 0, y.data_ptr(), 0, 1, 16, 16, 0, out.data_ptr(), None, buf.data_ptr(),
                                                need.value, torch.cuda.current_stream().cuda_stream))
    assert e.value.code == 4
    with pytest.raises(KeyError):
        m.stage("relu6", 1, 16, 16)
    m.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            m.distances(y, y)
    finally:
        m.eval()


def test_evaluate_takes_the_vgg_model():
    m = model_of("default")
    case = (64, 64, 2)
    a, b, _, _ = pairs_of("noisy", case)
    want = float(reference("default", "noisy", case, True)["d"].mean())
    _, _, lp, _ = cid.evaluate(dev(a), dev(b), ms_ssim=False, lpips=m)
    assert abs(lp - want) <= 1e-5 * want
