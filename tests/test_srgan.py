"""The server's SRGANGenerator (reference backend/app.py:145-186) on the GPU: cid_sr_forward (include/cid.h) and srgan.py.

The reference for error is tests/srgan_oracle.py in float64 (held to the fixtures recorded from the reference class by
test_srgan_host.py); where a fixture exists the result is compared with it as well.  The bound is the project's per-stage rule,
max|delta| <= 1e-5 * max(1, max|ref64|) per tensor: the reference's own ATen fp32 stands at 0.6-6.1e-7 of that scale on the "default"
weights and 0.2-2.0e-6 on "hot" (tests/golden/srgan_stats.json), a margin of 5x or more.  x0, the trunk, the first upscale stage and
the tensor the tail reads are compared through cid_sr_stage_view, and the sums before tanh through CID_SR_RAW, so that an error is
told from the stage after it.  tanh saturates, so `out` is held to the bound of the sums before it (tanh is 1-Lipschitz) and the
tanh step alone to 1e-6 against float64 tanh of the GPU's own sums."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth
from celebrity_image_denoiser_amd.srgan import load_srgan, srgan_padding, super_resolve, super_resolve_u8

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import srgan_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (N, H, W, scale).  1x1: every window is padding, the output is 4x4; 5x7: smaller than the 9x9 window and than any tile; 2x16x16: an
# exact trunk tile, batch stride; 13x18: partial tiles on both axes in every kernel; 3x8x12: a batch of three for the bit tests;
# 20x36: the output is 80x144, several tail tiles (16x64) on both axes with a partial one, the middle stage is 40x72; 13x18 at scale
# 2: one upscale stage; 5x7 at scale 1: none, tail_in is the trunk
SHAPES = [(1, 1, 1, 4), (1, 5, 7, 4), (2, 16, 16, 4), (1, 13, 18, 4), (3, 8, 12, 4), (1, 20, 36, 4), (1, 13, 18, 2), (1, 5, 7, 1)]
FIRST = {s: 2100 + 10 * i for i, s in enumerate(SHAPES)}
FIXTURES = {(1, 5, 7, 4), (2, 16, 16, 4), (1, 13, 18, 4)}

_MODELS, _REFS = {}, {}


def model_of(wset, scale=4):
    if (wset, scale) not in _MODELS:
        _MODELS[(wset, scale)] = load_srgan(synth.make_srgan_state_dict(wset, scale), scale_factor=scale, device=DEV, strict=True)
    return _MODELS[(wset, scale)]


def input_u8(shape):
    return synth.srgan_inputs_u8(*shape[:3], FIRST[shape])


def fixture_of(wset, shape):
    return np.load(os.path.join(GOLDEN, f"srgan_{wset}_s4_{shape[1]}x{shape[2]}.npz")) if shape in FIXTURES else None


def input_of(wset, shape):
    """The fixture's input where one exists, else the normalised view of this shape's uint8 batch.  fp32 [N,3,H,W] in [-1,1]."""
    fx = fixture_of(wset, shape)
    return fx["x"] if fx is not None else srgan_oracle.normalise_u8(input_u8(shape))


def reference(wset, shape, padding=(0, 0, 0, 0)):
    """The float64 oracle of one case (over the padded input): computed once, shared, never modified."""
    key = (wset, shape, tuple(padding))
    if key not in _REFS:
        taps = {}
        x = srgan_oracle.pad_input(input_of(wset, shape), padding)
        ref = srgan_oracle.forward(synth.make_srgan_state_dict(wset, shape[3]), x, taps=taps)
        ref.update(taps)
        for v in ref.values():
            v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def check(name, got, ref64, fixture=None, bound=None):
    bound = srgan_oracle.bound(ref64) if bound is None else bound
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    print(f"{name}: max|delta| {err:.3e}, bound {bound:.3e} (margin {bound / max(err, 1e-300):.1f}x), max|ref| {np.abs(ref64).max():.4g}")
    assert got.shape == ref64.shape, name
    assert np.isfinite(got).all(), name
    assert err <= bound, (name, err, bound)
    if fixture is not None:
        errf = float(np.abs(got.astype(np.float64) - fixture.astype(np.float64)).max())
        print(f"{name}: against the fixture {errf:.3e}")
        assert errf <= bound, (name, errf, bound)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:3])) + f"-s{s[3]}")
@pytest.mark.parametrize("wset", ["default", "hot"])
def test_parity_with_the_float64_oracle(wset, shape):
    n, h, w, scale = shape
    m = model_of(wset, scale)
    x = input_of(wset, shape)
    ref = reference(wset, shape)
    fx = fixture_of(wset, shape)
    full = fx is not None and "initial" in fx.files
    xd = torch.from_numpy(x).to(DEV)
    pre = m(xd, raw=True)
    out = super_resolve(m, xd)
    stages = {k: m.stage(k, n, h, w) for k in ("x0", "trunk", "tail_in") + (("up1",) if scale >= 4 else ())}
    torch.cuda.synchronize()
    assert out.shape == (n, 3, scale * h, scale * w) and out.dtype == torch.float32 and pre.shape == out.shape
    check("x0", stages["x0"].cpu().numpy(), ref["x0"], None if fx is None else fx["initial" if full else "x0"])
    check("trunk", stages["trunk"].cpu().numpy(), ref["trunk"], None if fx is None else (fx["mid"] + fx["initial"] if full else fx["trunk"]))
    if scale >= 4:
        check("up1", stages["up1"].cpu().numpy(), ref["up1"])
    if scale == 1:
        assert torch.equal(stages["tail_in"], stages["trunk"])
    check("tail_in", stages["tail_in"].cpu().numpy(), ref["tail_in"], fx["upscale"] if full else None)
    pre, out = pre.cpu().numpy(), out.cpu().numpy()
    check("pre", pre, ref["pre"], fx["final"] if full else None)
    # tanh is 1-Lipschitz and saturates: the output inherits the bound of the sums before it
    check("out", out, ref["out"], None if fx is None else fx["out"], bound=srgan_oracle.bound(ref["pre"]))
    tanh_err = float(np.abs(out.astype(np.float64) - np.tanh(pre.astype(np.float64))).max())
    print(f"tanh step alone: max|tanhf(pre) - tanh64(pre)| {tanh_err:.3e} over |pre| <= {np.abs(pre).max():.4g} (bound 1e-6; ATen fp32: 3.2e-8)")
    assert tanh_err <= 1e-6
    assert np.abs(out).max() <= 1.0


def u8_check(got, want, wset):
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    frac = float((d != 0).mean())
    sat = float(((want == 0) | (want == 255)).mean())
    print(f"uint8 {wset}: max|delta| {d.max()}, differing {frac:.2e}, expected bytes at 0 or 255 {sat:.3f}")
    assert got.shape == want.shape and got.dtype == want.dtype
    assert d.max() <= 1 and frac <= 1e-3            # the cap of test_gpu_parity.py
    if wset == "hot":
        assert 0.05 <= sat <= 0.90                  # the clamp is exercised and is not all there is
    else:
        assert sat == 0                             # every byte is mid-range


@pytest.mark.parametrize("wset", ["default", "hot"])
def test_uint8_server_path_against_the_server_fixture(wset):
    fx = np.load(os.path.join(GOLDEN, f"srgan_{wset}_u8_24x20.npz"))
    got = super_resolve_u8(model_of(wset), torch.from_numpy(fx["in_u8"]).to(DEV))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 128, 128, 3)
    u8_check(got.cpu().numpy(), fx["out_u8"], wset)


@pytest.mark.parametrize("wset", ["default", "hot"])
def test_uint8_server_path_against_the_oracle(wset):
    shape = (1, 13, 18, 4)
    pad = srgan_padding(13, 18, 4)
    got = super_resolve_u8(model_of(wset), torch.from_numpy(input_u8(shape)).to(DEV))
    assert tuple(got.shape) == (1, 64, 128, 3)
    x = srgan_oracle.pad_input(srgan_oracle.normalise_u8(input_u8(shape)), pad)
    ref = srgan_oracle.forward(synth.make_srgan_state_dict(wset, 4), x)
    u8_check(got.cpu().numpy(), srgan_oracle.to_u8(ref["out"]), wset)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_uint8_input_gives_the_bits_of_its_fp32_copy():
    m = model_of("hot")
    shape = (3, 8, 12, 4)
    u8 = torch.from_numpy(input_u8(shape)).to(DEV)
    # the normalised copy is made on the host with true divisions, as ToTensor() and Normalize() do
    xf = torch.from_numpy(srgan_oracle.normalise_u8(input_u8(shape))).to(DEV)
    for pad in ((0, 0, 0, 0), (2, 0, 1, 3)):
        assert torch.equal(_bits(m(u8, out_dtype=torch.float32, padding=pad)), _bits(m(xf, padding=pad))), pad
        assert torch.equal(m(xf, out_dtype=torch.uint8, padding=pad), m(u8, padding=pad)), pad
        assert torch.equal(_bits(m(u8, out_dtype=torch.float32, raw=True, padding=pad)), _bits(m(xf, raw=True, padding=pad))), pad


@pytest.mark.parametrize("pad", [(7, 1, 7, 2), (0, 3, 0, 0), (5, 0, 0, 0), (0, 0, 9, 11)], ids=lambda p: "-".join(map(str, p)))
def test_explicit_pads_give_the_bits_of_a_host_padded_input(pad):
    """The band is uint8 0, or -1.0 for fp32: index arithmetic in the head gives the bits of a padded copy run with all-zero pads."""
    m = model_of("hot")
    shape = (1, 13, 18, 4)
    pl, pt, pr, pb = pad
    u8 = input_u8(shape)
    xf = srgan_oracle.normalise_u8(u8)
    u8_padded = np.pad(u8, ((0, 0), (pt, pb), (pl, pr), (0, 0)))
    xf_padded = srgan_oracle.pad_input(xf, pad)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    a = m(dev(u8), padding=pad)
    assert tuple(a.shape) == (1, 4 * (13 + pt + pb), 4 * (18 + pl + pr), 3)
    assert torch.equal(a, m(dev(u8_padded)))
    b = m(dev(xf), padding=pad)
    assert torch.equal(_bits(b), _bits(m(dev(xf_padded))))
    assert torch.equal(_bits(b), _bits(m(dev(u8_padded), out_dtype=torch.float32)))
    x0 = m.stage("x0", 1, 13 + pt + pb, 18 + pl + pr)
    m(dev(xf), padding=pad)
    assert torch.equal(_bits(x0), _bits(m.stage("x0", 1, 13 + pt + pb, 18 + pl + pr)))


def test_an_image_alone_and_in_a_batch_and_two_calls_give_identical_bits():
    m = model_of("hot")
    shape = (3, 8, 12, 4)
    x = torch.from_numpy(input_of("hot", shape)).to(DEV)
    pad = (1, 2, 3, 0)
    for kw in ({}, {"padding": pad}, {"out_dtype": torch.uint8, "padding": pad}):
        full = m(x, **kw)
        again = m(x, **kw)
        assert torch.equal(_bits(full), _bits(again))
        for i in range(3):
            alone = m(x[i:i + 1].contiguous(), **kw)
            assert torch.equal(_bits(alone), _bits(full[i:i + 1])), (i, kw)


def test_crop_equals_slicing_the_uncropped_result():
    m = model_of("default")
    shape = (1, 13, 18, 4)
    u8 = torch.from_numpy(input_u8(shape)).to(DEV)
    pl, pt, pr, pb = srgan_padding(13, 18, 4)
    whole = super_resolve_u8(m, u8)
    part = super_resolve_u8(m, u8, crop=True)
    assert tuple(whole.shape) == (1, 64, 128, 3) and tuple(part.shape) == (1, 52, 72, 3)
    assert torch.equal(part, whole[:, 4 * pt:4 * (pt + 13), 4 * pl:4 * (pl + 18)])
    assert part._base is not None                                           # a view: no kernel, no copy
    # another divisor: 13 x 18 -> 16 x 24 at pad_divisor 2
    assert tuple(super_resolve_u8(m, u8, pad_divisor=2).shape) == (1, 64, 96, 3)


GUARD = 4096


def _guarded(nbytes, fill):
    buf = torch.full((nbytes + 2 * GUARD + 256,), fill, dtype=torch.uint8, device=DEV)
    start = (-buf.data_ptr() - GUARD) % 256 + GUARD      # 256-byte aligned, at least one guard past the start
    return buf, start


@pytest.mark.parametrize("out_u8", [False, True], ids=["f32", "u8"])
def test_nan_prefill_changes_nothing_and_guard_regions_stay_untouched(out_u8):
    """Workspace and output start as NaN bits (0xFF bytes), with 4 KiB guard regions of 0xA5 before and after each: the result is
    finite and equal to the module's, and no guard byte changes (no read of an unwritten word reaches a result, no write leaves
    its buffer)."""
    m = model_of("hot")
    shape = (1, 13, 18, 4)
    n, h, w, s = shape
    pl, pt, pr, pb = pad = (7, 1, 7, 2)
    hp, wp = h + pt + pb, w + pl + pr
    x = torch.from_numpy(input_of("hot", shape)).to(DEV)
    want = m(x, out_dtype=torch.uint8 if out_u8 else torch.float32, padding=pad)
    L = _lib.lib()
    need = ctypes.c_size_t()
    assert L.cid_sr_workspace_bytes(n, hp, wp, s, ctypes.byref(need)) == 0
    out_bytes = n * s * hp * s * wp * 3 * (1 if out_u8 else 4)
    bufs = []
    for nbytes in (need.value, out_bytes):
        buf, start = _guarded(nbytes, 0xA5)
        buf[start:start + nbytes] = 0xFF
        bufs.append((buf, start, nbytes))
    (wsb, ws0, _), (ob, o0, _) = bufs
    stream = torch.cuda.current_stream().cuda_stream
    rc = L.cid_sr_forward(m._cid, x.data_ptr(), _lib.CID_FMT_F32_NCHW, ob.data_ptr() + o0,
                          _lib.CID_FMT_U8_NHWC if out_u8 else _lib.CID_FMT_F32_NCHW, n, h, w, pl, pt, pr, pb, 0, wsb.data_ptr() + ws0,
                          need.value, stream)
    assert rc == 0, L.cid_sr_last_error(m._cid)
    torch.cuda.synchronize()
    got = ob[o0:o0 + out_bytes].clone()
    got = got.view(n, s * hp, s * wp, 3) if out_u8 else got.view(torch.float32).view(n, 3, s * hp, s * wp)
    if not out_u8:
        assert torch.isfinite(got).all()
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    for buf, start, nbytes in bufs:
        assert bool((buf[:start] == 0xA5).all()) and bool((buf[start + nbytes:] == 0xA5).all())


def test_the_unusual_prelu_slopes_of_hot_are_hit():
    """"hot" sets the slope of initial.1 to -0.3, that of the last block's PReLU to 1.5 and that of the first upscale stage to -0.3.
    The tensors they are applied to have more than 5 % negative entries, so the slopes reach the result.  A max-form PReLU
    (max(v, a*v)) is wrong for a > 1 and differs on the 1.5 tap by more than 1e-3; for a < 0 the max form equals the definition, and
    what differs there by more than 1e-3 is a form that takes the slope's magnitude or clamps it to [0, 1]."""
    sd = synth.make_srgan_state_dict("hot", 4)
    slopes = {"pre.initial": "initial.1.weight", "pre.4": "res_blocks.4.2.weight", "pre.up1": "upscale.2.weight"}
    assert [float(sd[k][0]) for k in slopes.values()] == pytest.approx([-0.3, 1.5, -0.3])
    ref = reference("hot", (1, 20, 36, 4))
    for tap, key in slopes.items():
        v, a = ref[tap], float(sd[key][0])
        frac = float((v < 0).mean())
        print(tap, "negative entries:", frac)
        assert frac > 0.05
        right = np.where(v > 0, v, a * v)
        if a > 1:
            assert np.abs(np.maximum(v, a * v) - right).max() > 1e-3          # the max form differs there
        else:
            assert np.abs(np.where(v > 0, v, abs(a) * v) - right).max() > 1e-3 and np.abs(np.maximum(v, 0) - right).max() > 1e-3


def test_load_srgan_reads_a_checkpoint_file(tmp_path):
    sd = {"module." + k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_srgan_state_dict("default", 2).items()}
    path = os.path.join(tmp_path, "srgan.pth")
    torch.save({"generator": sd, "epoch": 3}, path)
    m = load_srgan(path, scale_factor=2, device=DEV, strict=True)
    shape = (1, 13, 18, 2)
    x = torch.from_numpy(input_of("default", shape)).to(DEV)
    assert torch.equal(m(x), model_of("default", 2)(x))
    assert not m.training
