"""The server's ESRGANGenerator (reference backend/app.py:188-218) without a GPU: the module's state_dict against the keys recorded from
the reference class, the synthetic weight sets, the host side of cid_esr_* (include/cid.h) and tests/esrgan_oracle.py, the float64
restatement the GPU tests measure against, held to every fixture recorded from the reference."""
import ctypes
import glob
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth
from celebrity_image_denoiser_amd.esrgan import ESRGANGenerator

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import esrgan_oracle  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ERR_INVALID, ERR_SHAPE, ERR_KEY, ERR_STATE, ERR_WORKSPACE = 1, 2, 3, 4, 5


def _keys():
    return json.load(open(os.path.join(GOLDEN, "esrgan_keys.json")))


@pytest.mark.parametrize("r", [8, 1])
def test_state_dict_matches_the_reference_class(r):
    want = _keys()[f"r{r}"]
    sd = ESRGANGenerator(r).state_dict()
    assert [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()] == want
    assert len(want) == 5 + 15 * r
    shapes = synth.esrgan_param_shapes(r)
    assert [[k, list(s), d] for k, (s, d) in shapes.items()] == want


def test_state_dict_round_trip_is_lossless():
    sd = synth.make_esrgan_state_dict("hot", 8)
    m = ESRGANGenerator(8)
    res = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    back = m.state_dict()
    assert list(back) == list(sd)
    for k, v in sd.items():
        assert back[k].dtype == torch.from_numpy(np.asarray(v)).dtype and np.array_equal(back[k].numpy(), v), k
    assert m.eval() is m and not m.training
    m.train()
    with pytest.raises(RuntimeError, match="train mode"):
        m(torch.zeros(1, 3, 4, 4))
    with pytest.raises(ValueError):
        ESRGANGenerator(17)


def _digest(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def test_synthetic_weights_are_reproducible():
    digests = json.load(open(os.path.join(GOLDEN, "esrgan_synth_digests.json")))
    for kind in ("default", "hot"):
        for r in (8, 1, 0):
            sd = synth.make_esrgan_state_dict(kind, r)
            assert _digest(sd) == digests[f"{kind}_r{r}"], (kind, r)
            assert _digest(synth.make_esrgan_state_dict(kind, r)) == _digest(sd)
    d, h = synth.make_esrgan_state_dict("default", 8), synth.make_esrgan_state_dict("hot", 8)
    for sd, gain in ((d, 1.0), (h, 6.0)):
        for k, fan in (("initial.0.weight", 243), ("residuals.3.block.3.weight", 576), ("final.weight", 5184)):
            b = np.sqrt(gain / fan)
            assert 0.98 * b < np.abs(sd[k]).max() <= b
        for i in range(8):
            for j in (1, 4):
                p = f"residuals.{i}.block.{j}."
                assert 0.6 <= sd[p + "weight"].min() and sd[p + "weight"].max() <= 1.4 and np.abs(sd[p + "bias"]).max() <= 0.1
                assert np.abs(sd[p + "running_mean"]).max() <= 0.3 and 0.5 <= sd[p + "running_var"].min() and sd[p + "running_var"].max() <= 1.5
    slopes = lambda sd: [float(sd[k][0]) for k in sd if sd[k].shape == (1,)]   # noqa: E731
    assert all(0.05 <= s <= 0.45 for s in slopes(d)) and len(slopes(d)) == 9
    assert sorted(slopes(h))[0] == pytest.approx(-0.3) and sorted(slopes(h))[-1] == 1.5
    assert all(0.05 <= s <= 0.45 for s in sorted(slopes(h))[1:-1])
    with pytest.raises(ValueError):
        synth.make_esrgan_state_dict("warm")


def test_param_key_enumerates_exactly_the_keys():
    L = _lib.lib()
    for r in (8, 1, 0):
        h = ctypes.c_void_p()
        assert L.cid_esr_create(ctypes.byref(h), r) == 0
        keys = []
        while L.cid_esr_param_key(h, len(keys)) is not None:
            keys.append(L.cid_esr_param_key(h, len(keys)).decode())
        assert keys == list(synth.esrgan_param_shapes(r))
        if r in (8, 1):
            assert keys == [k for k, _, _ in _keys()[f"r{r}"]]
        assert L.cid_esr_param_key(h, -1) is None and L.cid_esr_param_key(None, 0) is None
        L.cid_esr_destroy(h)


def _set(L, h, key, a):
    a = np.ascontiguousarray(a) if np.ndim(a) else np.asarray(a)      # ascontiguousarray would make a 0-d array 1-d
    shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
    return L.cid_esr_set_weight(h, key.encode(), a.ctypes.data, shape, a.ndim)


def test_c_abi_argument_errors_need_no_gpu():
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.cid_esr_create(None, 8) == ERR_INVALID
    assert L.cid_esr_create(ctypes.byref(h), -1) == ERR_INVALID and L.cid_esr_create(ctypes.byref(h), 17) == ERR_INVALID
    assert L.cid_esr_create(ctypes.byref(h), 16) == 0
    L.cid_esr_destroy(h)
    assert L.cid_esr_create(ctypes.byref(h), 1) == 0
    assert L.cid_esr_last_error(None) == b"null handle"
    sd = synth.make_esrgan_state_dict("default", 1)
    miss = ctypes.c_int()
    assert L.cid_esr_missing_weights(h, ctypes.byref(miss)) == 0 and miss.value == 18      # 20 keys less 2 num_batches_tracked
    assert L.cid_esr_missing_weights(h, None) == ERR_INVALID and L.cid_esr_missing_weights(None, ctypes.byref(miss)) == ERR_INVALID
    w = sd["final.weight"]
    assert L.cid_esr_set_weight(None, b"final.weight", w.ctypes.data, (ctypes.c_int64 * 4)(*w.shape), 4) == ERR_INVALID
    assert L.cid_esr_set_weight(h, None, w.ctypes.data, (ctypes.c_int64 * 4)(*w.shape), 4) == ERR_INVALID
    assert L.cid_esr_set_weight(h, b"final.weight", None, (ctypes.c_int64 * 4)(*w.shape), 4) == ERR_INVALID
    assert L.cid_esr_set_weight(h, b"final.weight", w.ctypes.data, None, 4) == ERR_INVALID
    assert _set(L, h, "residuals.1.block.0.weight", sd["residuals.0.block.0.weight"]) == ERR_KEY        # R = 1 has no block 1
    assert b"unexpected key" in L.cid_esr_last_error(h)
    assert _set(L, h, "final.weight", sd["initial.0.weight"]) == ERR_SHAPE and b"size mismatch for final.weight" in L.cid_esr_last_error(h)
    assert _set(L, h, "initial.1.weight", np.zeros(2, np.float32)) == ERR_SHAPE
    assert _set(L, h, "residuals.0.block.1.num_batches_tracked", np.zeros(1, np.int64)) == ERR_SHAPE
    assert L.cid_esr_set_bn_eps(h, 1, 0, 1e-5) == ERR_INVALID and L.cid_esr_set_bn_eps(h, 0, 2, 1e-5) == ERR_INVALID
    assert L.cid_esr_set_bn_eps(h, 0, 0, -1.0) == ERR_INVALID and L.cid_esr_set_bn_eps(h, 0, 1, float("nan")) == ERR_INVALID
    assert L.cid_esr_set_bn_eps(h, 0, 1, 1e-3) == 0
    fake = ctypes.c_void_p(1 << 20)                                                          # aligned, never dereferenced
    assert L.cid_esr_upload_weights(h, None, None) == ERR_INVALID
    assert L.cid_esr_upload_weights(h, ctypes.c_void_p((1 << 20) + 64), None) == ERR_WORKSPACE
    assert L.cid_esr_upload_weights(h, fake, None) == ERR_STATE and b"initial.0.weight not set" in L.cid_esr_last_error(h)
    for k, v in sd.items():
        if not k.endswith("final.bias"):
            assert _set(L, h, k, v) == 0, k
    assert L.cid_esr_missing_weights(h, ctypes.byref(miss)) == 0 and miss.value == 1
    assert L.cid_esr_upload_weights(h, fake, None) == ERR_STATE and b"final.bias not set" in L.cid_esr_last_error(h)
    seg = lambda r: ((243 * 64 + 128) + 2 * r * (64 * 64 * 9 + 256) + (64 * 9 * 32 + 64)) * 4   # noqa: E731
    assert L.cid_esr_packed_weights_bytes(h) == seg(1) and L.cid_esr_packed_weights_bytes(None) == 0
    n = ctypes.c_size_t()
    assert L.cid_esr_workspace_bytes(2, 13, 18, ctypes.byref(n)) == 0 and n.value == 3 * ((2 * 64 * 13 * 18 * 4 + 255) // 256 * 256)
    assert L.cid_esr_workspace_bytes(2, 13, 18, None) == ERR_INVALID
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (1, 1 << 16, 1 << 15)):
        assert L.cid_esr_workspace_bytes(*bad, ctypes.byref(n)) == ERR_SHAPE, bad
    fwd = lambda hh, i, fi, o, fo, N, H, W, ws, nb: L.cid_esr_forward(hh, i, fi, o, fo, N, H, W, ws, nb, None)   # noqa: E731
    big = 1 << 40
    assert fwd(None, fake, 0, fake, 0, 1, 8, 8, fake, big) == ERR_INVALID
    assert fwd(h, None, 0, fake, 0, 1, 8, 8, fake, big) == ERR_INVALID and b"null pointer" in L.cid_esr_last_error(h)
    assert fwd(h, fake, 0, None, 0, 1, 8, 8, fake, big) == ERR_INVALID and fwd(h, fake, 0, fake, 0, 1, 8, 8, None, big) == ERR_INVALID
    assert fwd(h, fake, 2, fake, 0, 1, 8, 8, fake, big) == ERR_INVALID and fwd(h, fake, 0, fake, -1, 1, 8, 8, fake, big) == ERR_INVALID
    assert b"unknown format" in L.cid_esr_last_error(h)
    odd = ctypes.c_void_p((1 << 20) + 2)
    assert fwd(h, odd, 0, fake, 0, 1, 8, 8, fake, big) == ERR_INVALID and fwd(h, fake, 1, odd, 0, 1, 8, 8, fake, big) == ERR_INVALID
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-3, 8, 8)):
        assert fwd(h, fake, 0, fake, 0, *bad, fake, big) == ERR_SHAPE, bad
    assert fwd(h, fake, 0, fake, 0, 2, 13, 18, fake, n.value - 1) == ERR_WORKSPACE
    assert fwd(h, fake, 0, fake, 0, 2, 13, 18, ctypes.c_void_p((1 << 20) + 128), big) == ERR_WORKSPACE
    assert fwd(h, odd, 1, odd, 1, 2, 13, 18, fake, n.value) == ERR_STATE and b"weights not uploaded" in L.cid_esr_last_error(h)
    off, c, hs, ws, cb = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    refs = (ctypes.byref(off), ctypes.byref(c), ctypes.byref(hs), ctypes.byref(ws), ctypes.byref(cb))
    assert L.cid_esr_stage_view(b"x1", 2, 13, 18, *refs) == 0 and (off.value, c.value, hs.value, ws.value, cb.value) == (0, 64, 13, 18, 8)
    assert L.cid_esr_stage_view(b"tail_in", 2, 13, 18, *refs) == 0 and off.value == n.value // 3 * 2
    assert L.cid_esr_stage_view(b"x2", 2, 13, 18, *refs) == ERR_KEY and L.cid_esr_stage_view(None, 2, 13, 18, *refs) == ERR_INVALID
    assert L.cid_esr_stage_view(b"x1", 0, 13, 18, *refs) == ERR_SHAPE
    L.cid_esr_destroy(h)


def _fixtures():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "esrgan_*_r*_*x*.npz")))


def test_the_fixture_set_is_complete():
    assert _fixtures() == sorted([f"esrgan_{w}_r8_{s}" for w in ("default", "hot") for s in ("16x16", "13x18")]
                                 + [f"esrgan_{w}_r1_5x7" for w in ("default", "hot")] + ["esrgan_default_r0_1x1"])
    for p in glob.glob(os.path.join(GOLDEN, "esrgan_*")):
        assert os.path.getsize(p) < 400 * 1000, p


@pytest.mark.parametrize("name", _fixtures())
def test_oracle_agrees_with_every_fixture_tensor(name):
    """The fixtures are the reference class on ATen fp32; the oracle is float64.  Per tensor max|delta| <= 1e-5 * max(1, max|ref64|)."""
    _, wset, r, size = name.split("_")
    r = int(r[1:])
    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert fx["x"].shape[2:] == tuple(int(v) for v in size.split("x")) and fx["x"].min() >= 0 and fx["x"].max() <= 1
    ref = esrgan_oracle.forward(synth.make_esrgan_state_dict(wset, r), fx["x"], r)
    for k in ("x1", "x2", "out"):
        assert ref[k].shape == fx[k].shape
        assert np.abs(fx[k] - ref[k]).max() <= esrgan_oracle.bound(ref[k]), k
    assert np.array_equal(ref["tail_in"], ref["x1"] + ref["x2"])
    if r == 0:
        assert np.array_equal(ref["x2"], ref["x1"])          # the empty nn.Sequential is the identity: out = final(2 * x1)


def test_oracle_agrees_with_the_uint8_fixture():
    fx = np.load(os.path.join(GOLDEN, "esrgan_default_u8_24x20.npz"))
    x = (fx["in_u8"].astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2)
    ref = esrgan_oracle.forward(synth.make_esrgan_state_dict("default", 8), x, 8)
    assert np.abs(fx["out_f32"] - ref["out"]).max() <= esrgan_oracle.bound(ref["out"])
    got, want = esrgan_oracle.to_u8(ref["out"]), fx["out_u8"]
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert d.max() <= 1 and (d != 0).mean() <= 1e-3
    sat = ((want == 0) | (want == 255)).mean()
    assert 0.05 <= sat <= 0.60, sat


def test_the_parity_shapes_cross_every_tile_edge():
    """test_esrgan.SHAPES against the tiling of csrc/esrgan_kernels.h, restated here: k_esr_conv owns 16 x 16 output pixels (DiscGeom's
    TH and D_TW), k_esr_tail 16 rows x 64 columns (E_TAIL_TH, E_TAIL_TW) with 8 consecutive pixels of a row per thread (E_TAIL_PX).
    The list must keep a shape for every edge the tail's column index tx and the plan's tiles_x take part in, so that none of
    them can leave the list unnoticed."""
    import test_esrgan

    trunk, tail_h, tail_w, px = 16, 16, 64, 8
    cols = lambda w: -(-w // tail_w)   # noqa: E731
    rows = lambda h: -(-h // tail_h)   # noqa: E731
    shapes = test_esrgan.SHAPES
    assert len(set(shapes)) == len(shapes)
    # >= 2 tail columns, the last one partial and cut inside one thread's 8-pixel segment
    assert any(cols(w) >= 2 and w % tail_w and (w % tail_w) % px for _, h, w in shapes)
    assert any(cols(w) >= 3 for _, h, w in shapes)
    assert any(cols(w) >= 2 and w % tail_w == 1 for _, h, w in shapes)            # a last column of one pixel
    assert any(rows(h) >= 2 and h % tail_h for _, h, w in shapes)                 # a partial last tail row
    assert any(rows(h) >= 2 and h % tail_h == 1 for _, h, w in shapes)            # ... of a single image row
    assert any(h % tail_h == 0 and w % tail_w == 0 for _, h, w in shapes)         # an exact tail tile
    assert any(h < 9 and w < 9 for _, h, w in shapes)                             # smaller than the 9 x 9 window
    assert any(n > 1 and rows(h) * cols(w) > 1 for n, h, w in shapes)             # batch stride over several tail tiles
    assert any(n > 1 and cols(w) >= 2 for n, h, w in shapes)                      # ... and over several tail columns
    assert any(h % trunk == 0 and w % trunk == 0 for _, h, w in shapes)           # an exact trunk tile
    assert any(-(-w // trunk) >= 9 for _, h, w in shapes)                         # many trunk tile columns
    # the uint8 and guard cases reach tx >= 1 too
    assert any(cols(w) >= 2 for _, h, w in test_esrgan.U8_SHAPES)
    assert all(s in shapes for s in test_esrgan.U8_SHAPES)


def test_the_oracle_alone_meets_the_saturation_window_of_the_uint8_shapes():
    """u8_check wants 5-60% of the expected bytes at 0 or 255.  That is a property of the inputs and the weights: the float64 oracle
    alone must meet it for every shape of test_esrgan.U8_SHAPES, before any kernel runs."""
    import test_esrgan

    sd = synth.make_esrgan_state_dict("default", 8)
    for shape in test_esrgan.U8_SHAPES:
        want = esrgan_oracle.to_u8(esrgan_oracle.forward(sd, test_esrgan.input_of("default", 8, shape), 8)["out"])
        sat = float(((want == 0) | (want == 255)).mean())
        print(shape, test_esrgan.FIRST[shape], f"{sat:.4f}")
        assert 0.05 <= sat <= 0.60, (shape, sat)
