"""The server's ESRGANGenerator (reference backend/app.py:188-218) on the GPU: cid_esr_forward (include/cid.h) and esrgan.py.

The reference for error is tests/esrgan_oracle.py in float64 (held to the fixtures recorded from the reference class by
test_esrgan_host.py); where a fixture exists the result is compared with it as well.  The bound is the project's per-stage rule,
max|delta| <= 1e-5 * max(1, max|ref64|) per tensor: the reference's own ATen fp32 stands at 0.3-1.2e-6 of that scale on the "default"
weights and 1.4-1.9e-6 on "hot" (tests/golden/esrgan_stats.json), a margin of 5-13x.  x1 and the tensor the tail reads are compared
through cid_esr_stage_view, so that a trunk error is told from a tail error."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth
from celebrity_image_denoiser_amd.esrgan import enhance, enhance_u8, load_esrgan

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import esrgan_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# 1x1: the window is all padding; 5x7: smaller than the 9x9 window and than a tile; 16x16: an exact trunk tile; 13x18, 37x53: partial
# tiles on both axes, odd sizes; 3x24x40: batch stride, several tiles; 2x64x64: an exact tail tile row, several trunk tiles.
# The tail tiles 16 rows x 64 columns (E_TAIL_TH, E_TAIL_TW), a thread owning 8 consecutive pixels of one row; the last three are the
# shapes with more than one tail column (tx >= 1: the halo origin tx * 64 - 4, the store column tx * 64 + cx + j, tiles_x itself):
# 1x20x70: two tail columns, the second 6 wide, so `ox < W` cuts inside one thread's segment; two tail rows, the second 4 deep;
# 1x17x130: three tail columns, the last 2 wide; the second tail row is one image row; 9 trunk tile columns;
# 2x33x65: batch stride with a 1-pixel second column and a 1-row third tail row (test_esrgan_host.py holds the list to this coverage)
SHAPES = [(1, 1, 1), (1, 5, 7), (2, 16, 16), (1, 13, 18), (1, 37, 53), (3, 24, 40), (2, 64, 64), (1, 20, 70), (1, 17, 130), (2, 33, 65)]
FIRST = {s: 1100 + 10 * i for i, s in enumerate(SHAPES)}
# The uint8 cases: of the float64 oracle's own bytes ("default", R = 8) 51.8% are 0 or 255 at 1x37x53 (first index 1140) and 54.2% at
# 1x20x70 (first index 1170), inside u8_check's window [0.05, 0.60] before any kernel runs (test_esrgan_host.py asserts it).
U8_SHAPES = [(1, 37, 53), (1, 20, 70)]
FIXTURES = {("default", 8, (2, 16, 16)), ("hot", 8, (2, 16, 16)), ("default", 8, (1, 13, 18)), ("hot", 8, (1, 13, 18)),
            ("default", 1, (1, 5, 7)), ("hot", 1, (1, 5, 7)), ("default", 0, (1, 1, 1))}

_MODELS, _REFS = {}, {}


def model_of(wset, r):
    if (wset, r) not in _MODELS:
        _MODELS[(wset, r)] = load_esrgan(synth.make_esrgan_state_dict(wset, r), num_residuals=r, device=DEV, strict=True)
    return _MODELS[(wset, r)]


def input_u8(shape):
    return synth.esrgan_inputs_u8(*shape, FIRST[shape])


def input_of(wset, r, shape):
    """The fixture's input where one exists, else the /255 view of this shape's uint8 batch.  fp32 [N,3,H,W] in [0,1]."""
    if (wset, r, shape) in FIXTURES:
        return np.load(os.path.join(GOLDEN, f"esrgan_{wset}_r{r}_{shape[1]}x{shape[2]}.npz"))["x"]
    return np.ascontiguousarray((input_u8(shape).astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))


def reference(wset, r, shape):
    """The float64 oracle of one case: computed once, shared, never modified."""
    key = (wset, r, shape)
    if key not in _REFS:
        taps = {}
        ref = esrgan_oracle.forward(synth.make_esrgan_state_dict(wset, r), input_of(*key), r, taps=taps)
        ref.update(taps)
        for v in ref.values():
            v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def check(name, got, ref64, fixture=None):
    bound = esrgan_oracle.bound(ref64)
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    print(f"{name}: max|delta| {err:.3e}, bound {bound:.3e}, max|ref| {np.abs(ref64).max():.4g}")
    assert np.isfinite(got).all(), name
    assert err <= bound, (name, err, bound)
    if fixture is not None:
        errf = float(np.abs(got.astype(np.float64) - fixture.astype(np.float64)).max())
        print(f"{name}: against the fixture {errf:.3e}")
        assert errf <= bound, (name, errf, bound)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("r", [0, 1, 8])
@pytest.mark.parametrize("wset", ["default", "hot"])
def test_parity_with_the_float64_oracle(wset, r, shape):
    m = model_of(wset, r)
    x = input_of(wset, r, shape)
    ref = reference(wset, r, shape)
    out = enhance(m, torch.from_numpy(x).to(DEV))
    x1, tail_in = m.stage("x1", *shape), m.stage("tail_in", *shape)
    torch.cuda.synchronize()
    fx = np.load(os.path.join(GOLDEN, f"esrgan_{wset}_r{r}_{shape[1]}x{shape[2]}.npz")) if (wset, r, shape) in FIXTURES else None
    assert out.shape == x.shape and out.dtype == torch.float32
    check("x1", x1.cpu().numpy(), ref["x1"], None if fx is None else fx["x1"])
    check("tail_in", tail_in.cpu().numpy(), ref["tail_in"], None if fx is None else fx["x1"] + fx["x2"])
    check("out", out.cpu().numpy(), ref["out"], None if fx is None else fx["out"])


def u8_check(got, want):
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    frac = float((d != 0).mean())
    sat = float(((want == 0) | (want == 255)).mean())
    print(f"uint8: max|delta| {d.max()}, differing {frac:.2e}, expected bytes at 0 or 255 {sat:.3f}")
    assert d.max() <= 1 and frac <= 1e-3            # the cap of test_gpu_parity.py
    assert 0.05 <= sat <= 0.60                      # the clamp is exercised and is not all there is


def test_uint8_path_against_the_server_fixture():
    fx = np.load(os.path.join(GOLDEN, "esrgan_default_u8_24x20.npz"))
    got = enhance_u8(model_of("default", 8), torch.from_numpy(fx["in_u8"]).to(DEV))
    assert got.dtype == torch.uint8 and got.shape == fx["in_u8"].shape
    u8_check(got.cpu().numpy(), fx["out_u8"])


@pytest.mark.parametrize("shape", U8_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_uint8_path_against_the_oracle(shape):
    got = enhance_u8(model_of("default", 8), torch.from_numpy(input_u8(shape)).to(DEV))
    u8_check(got.cpu().numpy(), esrgan_oracle.to_u8(reference("default", 8, shape)["out"]))


def test_uint8_input_gives_the_bits_of_its_fp32_copy():
    m = model_of("hot", 8)
    shape = (3, 24, 40)
    u8 = torch.from_numpy(input_u8(shape)).to(DEV)
    # the fp32 copy is made on the host with a true division, as ToTensor() does (a device tensor / 255.0 multiplies by a reciprocal)
    xf = torch.from_numpy(np.ascontiguousarray((input_u8(shape).astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))).to(DEV)
    a = m(u8, out_dtype=torch.float32)
    b = m(xf)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(m(xf, out_dtype=torch.uint8), m(u8))


def test_an_image_alone_and_in_a_batch_and_two_calls_give_identical_bits():
    m = model_of("hot", 8)
    shape = (3, 24, 40)
    x = torch.from_numpy(input_of("hot", 8, shape)).to(DEV)
    full = m(x)
    again = m(x)
    assert torch.equal(full.view(torch.int32), again.view(torch.int32))
    for i in range(3):
        alone = m(x[i:i + 1].contiguous())
        assert torch.equal(alone.view(torch.int32), full[i:i + 1].view(torch.int32)), i


GUARD = 4096


def _guarded(nbytes, fill):
    buf = torch.full((nbytes + 2 * GUARD + 256,), fill, dtype=torch.uint8, device=DEV)
    start = (-buf.data_ptr() - GUARD) % 256 + GUARD      # 256-byte aligned, at least one guard past the start
    return buf, start


@pytest.mark.parametrize("shape", [(1, 37, 53), (1, 17, 130)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("out_u8", [False, True], ids=["f32", "u8"])
def test_nan_prefill_changes_nothing_and_guard_regions_stay_untouched(out_u8, shape):
    """Workspace and output start as NaN bits (0xFF bytes), with 4 KiB guard regions of 0xA5 before and after each: the result is
    finite and equal to the module's, and no guard byte changes (no read of an unwritten word reaches a result, no write leaves
    its buffer).  At 1x17x130 the last of three tail columns is 2 pixels wide: a tail store past the last column of the last
    row lands in the guard behind the output."""
    m = model_of("hot", 8)
    n, h, w = shape
    x = torch.from_numpy(input_of("hot", 8, shape)).to(DEV)
    want = m(x, out_dtype=torch.uint8 if out_u8 else torch.float32)
    L = _lib.lib()
    need = ctypes.c_size_t()
    assert L.cid_esr_workspace_bytes(n, h, w, ctypes.byref(need)) == 0
    out_bytes = n * h * w * 3 * (1 if out_u8 else 4)
    bufs = []
    for nbytes in (need.value, out_bytes):
        buf, start = _guarded(nbytes, 0xA5)
        buf[start:start + nbytes] = 0xFF
        bufs.append((buf, start, nbytes))
    (wsb, ws0, _), (ob, o0, _) = bufs
    stream = torch.cuda.current_stream().cuda_stream
    rc = L.cid_esr_forward(m._cid, x.data_ptr(), _lib.CID_FMT_F32_NCHW, ob.data_ptr() + o0,
                           _lib.CID_FMT_U8_NHWC if out_u8 else _lib.CID_FMT_F32_NCHW, n, h, w, wsb.data_ptr() + ws0, need.value, stream)
    assert rc == 0, L.cid_esr_last_error(m._cid)
    torch.cuda.synchronize()
    got = ob[o0:o0 + out_bytes].clone()
    got = got.view(n, h, w, 3) if out_u8 else got.view(torch.float32).view(n, 3, h, w)
    if not out_u8:
        assert torch.isfinite(got).all()
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    for buf, start, nbytes in bufs:
        assert bool((buf[:start] == 0xA5).all()) and bool((buf[start + nbytes:] == 0xA5).all())


def test_the_unusual_prelu_slopes_of_hot_are_hit():
    """"hot" sets the slope of initial.1 to -0.3 and that of the last block's PReLU to 1.5: the tensors they are applied to have
    negative entries, so a max-form PReLU (max(v, a*v)) would fail the parity test above on this set."""
    sd = synth.make_esrgan_state_dict("hot", 8)
    assert float(sd["initial.1.weight"][0]) == pytest.approx(-0.3) and float(sd["residuals.7.block.2.weight"][0]) == 1.5
    ref = reference("hot", 8, (1, 37, 53))
    for k in ("pre.initial", "pre.7"):
        frac = float((ref[k] < 0).mean())
        print(k, "negative entries:", frac)
        assert frac > 0.05
    v = ref["pre.7"]
    assert np.abs(np.maximum(v, 1.5 * v) - np.where(v > 0, v, 1.5 * v)).max() > 1e-3      # the max form differs there


def test_load_esrgan_reads_a_checkpoint_file(tmp_path):
    sd = {"module." + k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_esrgan_state_dict("default", 1).items()}
    path = os.path.join(tmp_path, "esrgan.pth")
    torch.save({"G": sd, "epoch": 3}, path)
    m = load_esrgan(path, num_residuals=1, device=DEV, strict=True)
    shape = (1, 5, 7)
    x = torch.from_numpy(input_of("default", 1, shape)).to(DEV)
    assert torch.equal(m(x), model_of("default", 1)(x))
    assert not m.training
