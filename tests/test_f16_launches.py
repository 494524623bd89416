"""Every launch of the fp16-storage path (compute_dtype="f16") checked on its own inputs.

After one forward every launch's output is still in the arena (each writes a region of its own, cid_api.hip enum Buf); each is held
to oracle/f16_oracle.check against a float64 reference computed from the tensors that launch READ, so a rounding flip upstream
does not blur the check downstream.  A stored half must lie in [half(post(ref - B)), half(post(ref + B))] (B: the fp32
summation bound, c = 1), must be a half at all, and at least MIN_EXACT of a launch's elements must equal half(post(ref)).
The fused last layer's z is checked against the activations the tiled form stores in the same forward — the kernel comment's
claim that the fused epilogue contracts exactly the stored tensor.  profiles/f16_launch_check.txt records the numbers."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from celebrity_image_denoiser_amd import synth
from oracle import f16_oracle as fo
from oracle import torch_oracle

pytestmark = pytest.mark.gpu

MIN_EXACT = 0.99
# end to end against the fp32 ATen oracle, He-gain weights, white noise: the CPU stand-in's maximum over 64 images of 128 x 128 is
# 4.7e-3 (csrc/tools/f16_calibrate.py); the bound adds a margin of 1.5x for the tail of larger batches (include/cid.h, CID_DTYPE_F16)
F16_WHITE_NOISE_BOUND = 7e-3


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X (torch.cuda.is_available() is False)")


@pytest.fixture(scope="module")
def f16_models(weight_sets):
    _need_gpu()
    import celebrity_image_denoiser_amd as cid

    out = {}
    for k, v in weight_sets.items():
        m = cid.load(v, device="cuda:0", strict=True)
        m.compute_dtype = "f16"
        out[k] = m
    return out


def _inputs(kind, n, h, w, seed=0):
    if kind == "faces":
        return synth.make_batch(n, h, w, first_index=700 + seed)[0]
    if kind == "uniform":
        g = torch.Generator().manual_seed(seed)
        return (torch.rand((n, 3, h, w), generator=g) * 2 - 1).numpy()
    yy, xx = np.mgrid[0:h, 0:w]
    cb = np.stack([((yy + xx + c) % 2) * 2.0 - 1.0 for c in range(3)]).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(cb, (n, 3, h, w))).copy()


def _forward(m, x, in_u8=False, padding=None):
    xd = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    if padding is not None:
        y = m.forward_padded(xd, padding, out_u8=False)
    elif in_u8:
        y = m.forward_u8(xd, out_u8=False)
    else:
        y = m(xd)
    torch.cuda.synchronize()
    return y.cpu()


def _assert_pass(reports, ctx):
    for r in reports.values():
        assert r.ok, (ctx, r.line())
        if r.launch != "upconv1.2":
            assert r.exact >= MIN_EXACT, (ctx, r.line())


def _check_both_tails(m, sd, x, in_u8=False, images=None):
    """One forward with the tiled last layer, one with the fused one, on the same input: the ten launches before the last two are
    bit-equal between them; every launch of both passes; the pooled tensors equal the max-pool of the stored ones where covered.
    `images`: the subset of the batch the CPU checks (the launches are per image).  -> {tail: reports}"""
    n = x.shape[0]
    h, w = (x.shape[1], x.shape[2]) if in_u8 else (x.shape[2], x.shape[3])
    sel = list(range(n)) if images is None else list(images)
    xn = fo.network_input(x, in_u8)[sel]
    out = {}
    m.tail_algo = "tiles"
    y_t = _forward(m, x, in_u8)
    st_t = fo.stored_tensors(m, n, h, w)
    m.tail_algo = "fused"
    y_f = _forward(m, x, in_u8)
    st_f = fo.stored_tensors(m, n, h, w)
    for k in fo.STORED:
        assert torch.equal(st_t[k], st_f[k]), k
    e1, e2 = st_t["down1"], st_t["down2"]
    assert torch.equal(st_t["pool1"][:, :, :e1.shape[2] // 2, :e1.shape[3] // 2], F.max_pool2d(e1, 2, 2))
    assert torch.equal(st_t["pool2"], F.max_pool2d(e2, 2, 2))
    for tail, st, y in (("tiles", st_t, y_t), ("fused", st_f, y_f)):
        sub = {k: v[sel] for k, v in st.items()}
        sub["out"] = y[sel]
        out[tail] = fo.check_launches(sd, xn, sub, tail=tail, act10=st_t["upconv1.0"][sel])
        _assert_pass(out[tail], (tail, x.shape))
    return out


@pytest.mark.parametrize("wset", ["hot", "default"])
@pytest.mark.parametrize("kind", ["faces", "uniform", "checkerboard"])
def test_every_launch_at_128_batch_4(f16_models, weight_sets, wset, kind):
    """All 12 launches (both last-layer forms) on faces, uniform white noise and the +-1 checkerboard, 4 images of 128 x 128."""
    _check_both_tails(f16_models[wset], weight_sets[wset], _inputs(kind, 4, 128, 128, seed=1))


@pytest.mark.parametrize("shape", [(2, 37, 150), (1, 129, 67), (2, 13, 18), (3, 8, 8), (2, 100, 20)], ids=lambda s: "x".join(map(str, s)))
def test_every_launch_on_ragged_shapes(f16_models, weight_sets, shape):
    """Crops with Hu < H, widths that are not a multiple of 16 or 32 (partial tiles, MFMA column tiles across rows), tiny images."""
    n, h, w = shape
    for wset in ("hot", "default"):
        _check_both_tails(f16_models[wset], weight_sets[wset], _inputs("uniform", n, h, w, seed=h * w))


@pytest.mark.parametrize("kind", synth.NOISE_TYPES)
def test_every_launch_on_the_trainer_noise_kinds_u8(f16_models, weight_sets, kind):
    """The u8 front end (head: half((u8/255 - 0.5)/0.5)) on the trainer's five noise kinds, 2 faces of 96 x 112."""
    clean = synth.clean_images_u8(2, 96, 112, first_index=900)
    noisy = synth.add_noise_np(clean, kind, first_index=900)
    _check_both_tails(f16_models["hot"], weight_sets["hot"], noisy, in_u8=True)


def test_walking_and_one_item_per_workgroup_at_batch_64(f16_models, weight_sets):
    """One 128 x 128 batch of 64 images with the 3x3 launches' workgroups walking (three per CU) and with one item per workgroup:
    the same bits, and the launch checks pass on images at both ends of the batch."""
    from celebrity_image_denoiser_amd import _lib

    L = _lib.lib()
    m, sd = f16_models["hot"], weight_sets["hot"]
    x = _inputs("uniform", 64, 128, 128, seed=64)
    walkers = ("down2.0", "upconv2")                           # the MODE-0 launches with CIN <= 128 walk (upconv1.0 too: z, "out")
    prev = L.cid_debug_half_workgroups_per_cu(3)
    try:
        _check_both_tails(m, sd, x, images=(0, 1, 62, 63))
        y_walk = _forward(m, x)
        walk = {k: m.stage_output(k, 64, 128, 128).cpu() for k in walkers}
        L.cid_debug_half_workgroups_per_cu(0)
        y_one = _forward(m, x)
        one = {k: m.stage_output(k, 64, 128, 128).cpu() for k in walkers}
    finally:
        L.cid_debug_half_workgroups_per_cu(prev)
    assert torch.equal(y_walk, y_one)
    for k in walkers:
        assert torch.equal(walk[k], one[k]), k
    m._ws = None
    torch.cuda.empty_cache()


def test_head_window_of_the_padded_forward(f16_models, weight_sets):
    """forward_padded with non-zero top / left padding (u8 and fp32 callers): the head synthesises the -1 band, the zero padding
    beyond it; every launch up to upconv1[0] passes on the padded network input."""
    m, sd = f16_models["hot"], weight_sets["hot"]
    pad = (3, 2, 1, 2)                                         # left, top, right, bottom -> 33 x 48 network input from 29 x 44
    u8 = synth.add_noise_np(synth.clean_images_u8(2, 29, 44, first_index=950), "salt_pepper", first_index=950)
    for x, in_u8 in ((u8, True), (synth.normalize_u8(u8), False)):
        for tail in ("tiles", "fused"):
            m.tail_algo = tail
            _forward(m, x, padding=pad)
            st = fo.stored_tensors(m, 2, 33, 48)
            xn = fo.network_input(x, in_u8, pad)
            assert xn.shape == (2, 3, 33, 48)
            _assert_pass(fo.check_launches(sd, xn, st, tail=tail), (in_u8, tail))
    m.tail_algo = "fused"


def test_end_to_end_white_noise_and_noise_kinds_he_gain(f16_models, weight_sets):
    """End to end against the fp32 ATen oracle on He-gain weights: 64 white-noise images of 128 x 128 within F16_WHITE_NOISE_BOUND
    (calibrated on the CPU stand-in, see above), and the trainer's five noise kinds through the u8 front end within the benchmark
    distribution's 5e-3 (stand-in: <= 3.6e-3)."""
    m, sd = f16_models["hot"], weight_sets["hot"]
    m.tail_algo = "fused"
    g = torch.Generator().manual_seed(2024)
    x = (torch.rand((64, 3, 128, 128), generator=g) * 2 - 1).numpy()
    err = (_forward(m, x) - torch_oracle.forward(sd, x)).abs().flatten(1).max(1).values
    assert float(err.max()) <= F16_WHITE_NOISE_BOUND, (float(err.max()), float(err.median()))
    clean = synth.clean_images_u8(8, 128, 128, first_index=300)
    for kind in synth.NOISE_TYPES:
        noisy = synth.add_noise_np(clean, kind, first_index=300)
        e = float((_forward(m, noisy, in_u8=True) - torch_oracle.forward(sd, synth.normalize_u8(noisy))).abs().max())
        assert e <= 5e-3, (kind, e)
    m._ws = None
    torch.cuda.empty_cache()


def test_new_stage_rows_fp32_against_the_aten_intermediates(weight_sets):
    """The block-internal rows of cid_stage_view ("down1.0", "down2.0", "bottleneck.0", "upconv2.0") on the fp32 path, against the
    ATen oracle's intermediates under the per-stage rule max|delta| <= 1e-5 * max(1, max|s|), at a ragged size."""
    _need_gpu()
    import celebrity_image_denoiser_amd as cid

    for wset in ("default", "hot"):
        sd = weight_sets[wset]
        m = cid.load(sd, device="cuda:0", strict=True)
        x = _inputs("faces", 2, 37, 150)
        _forward(m, x)
        _, s = torch_oracle.forward(sd, x, return_stages=True)
        p = lambda k: torch.from_numpy(sd[k])  # noqa: E731
        blk0 = lambda t, k: F.relu(F.conv2d(t, p(k + ".0.weight"), p(k + ".0.bias"), padding=1))  # noqa: E731
        e2 = s["down2"][:, :, :s["up2"].shape[2], :s["up2"].shape[3]]
        want = {"down1.0": blk0(torch.from_numpy(x), "down1"), "down2.0": blk0(s["pool1"], "down2"),
                "bottleneck.0": blk0(s["pool2"], "bottleneck"), "upconv2.0": blk0(torch.cat([s["up2"], e2], 1), "upconv2")}
        for k, ref in want.items():
            got = m.stage_output(k, 2, 37, 150).cpu()
            assert got.shape == ref.shape, (k, got.shape, ref.shape)
            tol = 1e-5 * max(1.0, float(ref.abs().max()))
            assert float((got - ref).abs().max()) <= tol, (wset, k, float((got - ref).abs().max()))
