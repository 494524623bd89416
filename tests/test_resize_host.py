"""No-GPU checks of the bicubic resize: the numpy restatement (synth.resize_bicubic_np) against recorded and live Pillow results,
the plan's coefficient tables (cid_resize_plan_table) against synth.resize_tables_np, and the argument checks of the C ABI."""
import ctypes
import os

import numpy as np
import pytest

from celebrity_image_denoiser_amd import _lib, synth

# (Hs, Ws, Hd, Wd): the shapes of tests/golden/make_resize_golden.py, which records Pillow's results for them
SHAPES = [(218, 178, 256, 256), (37, 53, 16, 16), (16, 16, 37, 53), (5, 7, 16, 12), (3, 3, 8, 8), (300, 200, 131, 200),
          (256, 100, 256, 64), (256, 256, 256, 256), (1, 1, 4, 4), (64, 64, 1, 1), (512, 192, 8, 3), (300, 250, 131, 77)]
BIG = (1024, 1024, 256, 256)
INVALID, SHAPE = 1, 2   # CID_ERR_INVALID, CID_ERR_SHAPE


def _id(s):
    return f"{s[0]}x{s[1]}_{s[2]}x{s[3]}"


def _inputs(hs, ws):
    """make_resize_golden.py's three inputs: seeded noise, 0/255 checkerboard of period 3, constant 255."""
    noise = np.random.default_rng(hs * 100003 + ws).integers(0, 256, (hs, ws, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:hs, 0:ws]
    checker = np.repeat(((((yy // 3) + (xx // 3)) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    return np.stack([noise, checker, np.full((hs, ws, 3), 255, np.uint8)])


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_restatement_equals_recorded_pillow(golden_dir, shape):
    hs, ws, hd, wd = shape
    g = np.load(os.path.join(golden_dir, f"resize_{_id(shape)}.npz"))
    assert np.array_equal(g["x"], _inputs(hs, ws))
    got = synth.resize_bicubic_np(g["x"], (wd, hd))
    assert got.shape == (3, hd, wd, 3) and got.dtype == np.uint8
    assert np.array_equal(got, g["y"]), f"differs from Pillow {g['pillow_version']}"
    assert (got[2] == 255).all()                                             # a constant image stays constant
    assert np.array_equal(synth.resize_bicubic_np(g["x"][0], (wd, hd)), g["y"][0])   # [H,W,3] form
    if shape == (16, 16, 37, 53):
        assert got[1].min() == 0 and got[1].max() == 255                     # upscaled, the checkerboard's overshoot reaches both clamps


@pytest.mark.parametrize("shape", SHAPES + [BIG], ids=_id)
def test_restatement_equals_live_pillow(shape):
    Image = pytest.importorskip("PIL.Image")
    hs, ws, hd, wd = shape
    x = _inputs(hs, ws)
    ref = np.stack([np.asarray(Image.fromarray(im).resize((wd, hd), resample=Image.Resampling.BICUBIC)) for im in x])
    assert np.array_equal(synth.resize_bicubic_np(x, (wd, hd)), ref)


def _plan(hs, ws, hd, wd):
    p = ctypes.c_void_p()
    assert _lib.lib().cid_resize_plan_create(ctypes.byref(p), hs, ws, hd, wd, _lib.CID_RESAMPLE_BICUBIC) == 0
    return p


def _table(p, axis, out_size):
    L = _lib.lib()
    ks = ctypes.c_int()
    assert L.cid_resize_plan_table(p, axis, ctypes.byref(ks), None, None) == 0          # query ksize only
    bounds, coeffs = np.full((out_size, 2), -7, np.int32), np.full((out_size, ks.value), -7, np.int32)
    assert L.cid_resize_plan_table(p, axis, ctypes.byref(ks), bounds.ctypes.data, coeffs.ctypes.data) == 0
    return ks.value, bounds, coeffs


def _check_axis(p, axis, in_size, out_size):
    ks, bounds, coeffs = _table(p, axis, out_size)
    ks_np, bounds_np, coeffs_np = synth.resize_tables_np(in_size, out_size)
    assert ks == ks_np and np.array_equal(bounds, bounds_np) and np.array_equal(coeffs, coeffs_np), (axis, in_size, out_size)


@pytest.mark.parametrize("shape", SHAPES + [BIG], ids=_id)
def test_plan_tables_equal_the_restatement(shape):
    hs, ws, hd, wd = shape
    p = _plan(hs, ws, hd, wd)
    _check_axis(p, 0, hs, hd)     # axis 0: vertical
    _check_axis(p, 1, ws, wd)     # axis 1: horizontal
    _lib.lib().cid_resize_plan_destroy(p)


def test_plan_tables_one_dimensional_sweep():
    """1 -> 1 through 64 -> 1 (every downscale factor up to the limit, down to a single sample) and 1 -> 1 through 1 -> 64."""
    for s in range(1, 65):
        for in_size, out_size in ((s, 1), (1, s)):
            p = _plan(in_size, 1, out_size, 1)
            _check_axis(p, 0, in_size, out_size)
            _check_axis(p, 1, 1, 1)
            _lib.lib().cid_resize_plan_destroy(p)
    ks, bounds, coeffs = synth.resize_tables_np(64, 1)
    assert ks == 257 and tuple(bounds[0]) == (0, 64) and coeffs.sum() in range((1 << 22) - 64, (1 << 22) + 65)


def test_argument_errors():
    """Every error of include/cid.h's resize section, with host pointers: all are found before anything is launched."""
    L = _lib.lib()
    p = ctypes.c_void_p()
    create = lambda hs, ws, hd, wd, f=3: L.cid_resize_plan_create(ctypes.byref(p), hs, ws, hd, wd, f)   # noqa: E731
    assert L.cid_resize_plan_create(None, 8, 8, 4, 4, 3) == INVALID
    assert create(8, 8, 4, 4, 2) == INVALID and create(8, 8, 4, 4, 0) == INVALID                        # bilinear, nearest: unknown here
    for bad in ((0, 8, 4, 4), (8, 0, 4, 4), (8, 8, 0, 4), (8, 8, 4, -1)):                               # a side below 1
        assert create(*bad) == SHAPE, bad
    for bad in ((16385, 8, 4096, 8), (8, 16385, 8, 4096), (8, 8, 16385, 8), (8, 8, 8, 16385)):          # a side above 16384
        assert create(*bad) == SHAPE, bad
    assert create(65, 8, 1, 8) == SHAPE and create(8, 129, 8, 2) == SHAPE                               # factor above 64
    assert create(0, 8, 4, 4, 2) == INVALID                                                             # INVALID comes first
    assert p.value is None
    for good in ((64, 8, 1, 8), (8, 128, 8, 2), (1, 1, 16384, 3), (16384, 1, 256, 1)):                  # the limits themselves
        assert create(*good) == 0, good
        L.cid_resize_plan_destroy(p)
    assert create(8, 8, 4, 4) == 0
    ks = ctypes.c_int()
    assert L.cid_resize_plan_table(None, 0, ctypes.byref(ks), None, None) == INVALID
    assert L.cid_resize_plan_table(p, 0, None, None, None) == INVALID
    assert L.cid_resize_plan_table(p, 2, ctypes.byref(ks), None, None) == INVALID
    assert L.cid_resize_plan_table(p, -1, ctypes.byref(ks), None, None) == INVALID
    src, dst = np.zeros(8 * 8 * 3, np.uint8), np.zeros(4 * 4 * 3, np.float32)
    s, d = src.ctypes.data, dst.ctypes.data
    assert L.cid_resize(None, s, d, _lib.CID_FMT_U8_NHWC, 1, None) == INVALID
    assert L.cid_resize(p, None, d, _lib.CID_FMT_U8_NHWC, 1, None) == INVALID
    assert L.cid_resize(p, s, None, _lib.CID_FMT_U8_NHWC, 1, None) == INVALID
    assert L.cid_resize(p, s, d, 2, 1, None) == INVALID and L.cid_resize(p, s, d, -1, 1, None) == INVALID
    assert L.cid_resize(p, s, d, _lib.CID_FMT_F32_NCHW, 0, None) == INVALID
    assert L.cid_resize(p, s, d, _lib.CID_FMT_U8_NHWC, -3, None) == INVALID
    assert not dst.any()
    L.cid_resize_plan_destroy(p)
    L.cid_resize_plan_destroy(None)                                                                     # a no-op


def test_python_surface_refuses_what_the_kernel_does_not_take():
    import torch

    import celebrity_image_denoiser_amd as cid

    with pytest.raises(RuntimeError, match="CPU tensor"):
        cid.resize(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (4, 4))
    with pytest.raises(RuntimeError, match="uint8"):
        cid.resize(torch.zeros(1, 8, 8, 3), (4, 4))
    with pytest.raises(ValueError):
        cid.resize(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (4, 4), out="f16")
    with pytest.raises(ValueError):
        synth.resize_tables_np(0, 4)
