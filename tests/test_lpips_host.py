"""LPIPS(net='alex') without a GPU: the float64 oracle's identities and sizes, the synthetic weight sets, the key table, both loader
layouts, strict / missing-key errors, the host side of cid_lpips_* (include/cid.h) and evaluate() without a model."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib, metrics, synth
from celebrity_image_denoiser_amd.lpips import LPIPS, build_lpips, lpips_state_dict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_oracle  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ERR_INVALID, ERR_SHAPE, ERR_KEY, ERR_STATE, ERR_WORKSPACE = 1, 2, 3, 4, 5


def _tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


# ---------------------------------------------------------------------------------------------------------------- the oracle
def test_oracle_sizes_by_hand():
    assert lpips_oracle.sizes(31, 31) == ((7, 7), (3, 3), (1, 1))
    assert lpips_oracle.sizes(35, 47) == ((8, 11), (3, 5), (1, 2))
    assert lpips_oracle.sizes(128, 128) == ((31, 31), (15, 15), (7, 7))
    sd = synth.make_lpips_state_dict("default")
    a, b, _, _ = lpips_oracle.pairs("noisy", 1, 35, 47)
    r = lpips_oracle.forward(sd, a, b)
    assert [r[t].shape for t in lpips_oracle.TAPS] == [(2, 64, 8, 11), (2, 192, 3, 5), (2, 384, 1, 2), (2, 256, 1, 2), (2, 256, 1, 2)]
    assert r["layers"].shape == (1, 5) and r["d"].shape == (1,)


def test_oracle_identities():
    sd = synth.make_lpips_state_dict("hot")
    a, b, _, _ = lpips_oracle.pairs("unrelated", 2, 31, 31)
    ab, ba, aa = lpips_oracle.forward(sd, a, b), lpips_oracle.forward(sd, b, a), lpips_oracle.forward(sd, a, a)
    assert np.array_equal(aa["d"], np.zeros(2)) and np.array_equal(aa["layers"], np.zeros((2, 5)))
    assert np.array_equal(ab["d"], ba["d"]) and np.array_equal(ab["layers"], ba["layers"])
    assert (ab["d"] > 0).all()
    # the padded border of the first convolution is zero AFTER the scaling layer: a constant image at `shift` is all zeros scaled,
    # so relu1 is relu(bias) everywhere, border included
    x = np.tile(sd["scaling_layer.shift"].astype(np.float64), (1, 1, 31, 31))   # the fp32 shift the oracle subtracts
    t = lpips_oracle.taps(sd, x)[0].numpy()
    want = np.maximum(sd["net.slice1.0.bias"].astype(np.float64), 0).reshape(1, 64, 1, 1)
    assert np.abs(t - want).max() < 1e-12
    # unit_view is the same network on x*0.5+0.5
    u = lpips_oracle.forward(sd, a, b, unit_view=True)
    v = lpips_oracle.forward(sd, a.astype(np.float64) * 0.5 + 0.5, b.astype(np.float64) * 0.5 + 0.5)
    assert np.array_equal(u["d"], v["d"])


def test_oracle_agrees_with_the_recorded_aten_fp32():
    """The fixtures hold ATen fp32's values of a plain torch.nn build of the network (make_lpips_golden.py): the oracle stands inside
    the bounds the maker asserted."""
    stats = json.load(open(os.path.join(GOLDEN, "lpips_stats.json")))
    assert stats["worst_fp32_tap_error"] <= 2e-6 and stats["worst_fp32_distance_error"] <= 1e-5
    for wset in ("default", "hot"):
        sd = synth.make_lpips_state_dict(wset)
        for kind in ("noisy", "unrelated"):
            fx = np.load(os.path.join(GOLDEN, f"lpips_{wset}_{kind}_35x47_n3.npz"))
            a, b, _, _ = lpips_oracle.pairs(kind, 3, 35, 47, int(fx["first_index"]))
            r = lpips_oracle.forward(sd, a, b, bool(fx["unit_view"]))
            assert np.abs(fx["relu5"] - r["relu5"]).max() <= lpips_oracle.bound(r["relu5"]) / 5
            assert (np.abs(fx["d"] - r["d"]) <= 1e-5 * np.abs(r["d"])).all()
            assert (np.abs(fx["layers"] - r["layers"]) <= 1e-5 * np.abs(r["layers"])).all()


# ---------------------------------------------------------------------------------------------------------------- weights and keys
def test_synth_weights_are_reproducible():
    want = json.load(open(os.path.join(GOLDEN, "lpips_synth_digests.json")))
    for wset in ("default", "hot"):
        sd = synth.make_lpips_state_dict(wset)
        h = hashlib.sha256()
        for k, v in sd.items():
            h.update(k.encode())
            h.update(np.ascontiguousarray(v).tobytes())
        assert h.hexdigest() == want[wset]
        for k in range(5):
            w = sd[f"lin{k}.model.1.weight"]
            assert (w >= 0).all() and 0.7 < float(w.sum()) < 1.3
            assert sd[f"lins.{k}.model.1.weight"] is w
    with pytest.raises(ValueError):
        synth.make_lpips_state_dict("cold")


def test_key_table():
    shapes = synth.lpips_param_shapes()
    m = LPIPS()
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == list(shapes.items())
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.cid_lpips_create(ctypes.byref(h)) == 0
    keys = [L.cid_lpips_param_key(h, i).decode() for i in range(_lib.CID_LPIPS_NUM_WEIGHTS)]
    assert keys == [k for k in shapes if not k.startswith("lins.")]
    assert L.cid_lpips_param_key(h, 17) is None and L.cid_lpips_param_key(h, -1) is None
    L.cid_lpips_destroy(h)
    assert not m.training and not any(p.requires_grad for p in m.parameters())


def test_loader_layouts():
    sd = synth.make_lpips_state_dict("default")
    full = build_lpips(_tensors(sd))
    # the package's lin-only file + a torchvision AlexNet state dict
    lin_only = {k: v for k, v in _tensors(sd).items() if k.startswith("lin") and not k.startswith("lins.")}
    alex = {}
    for k, v in sd.items():
        if k.startswith("net.slice"):
            _, _, idx, leaf = k.split(".")
            alex[f"features.{idx}.{leaf}"] = torch.from_numpy(v)
    alex["classifier.1.weight"] = torch.zeros(4, 4)
    alex["classifier.1.bias"] = torch.zeros(4)
    split = build_lpips(lin_only, alex)
    # "module."-prefixed keys, lins.* only
    prefixed = {"module." + k: v for k, v in _tensors(sd).items() if not (k.startswith("lin") and not k.startswith("lins."))}
    pre = build_lpips(prefixed)
    for other in (split, pre):
        for (k, v), (k2, v2) in zip(full.state_dict().items(), other.state_dict().items()):
            assert k == k2 and torch.equal(v, v2), k
    for k, v in full.state_dict().items():
        assert np.array_equal(v.numpy(), sd[k]), k
    assert set(lpips_state_dict(lin_only, alex)) == set(sd) - {"scaling_layer.shift", "scaling_layer.scale"}


def test_loader_errors():
    sd = _tensors(synth.make_lpips_state_dict("default"))
    missing = {k: v for k, v in sd.items() if k != "net.slice3.6.bias"}
    with pytest.raises(RuntimeError, match="net.slice3.6.bias"):
        build_lpips(missing)
    assert build_lpips(missing, strict=False) is not None
    extra = dict(sd, **{"net.slice9.0.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="net.slice9.0.weight"):
        build_lpips(extra)
    with pytest.raises(KeyError, match="avgpool"):
        build_lpips(sd, {"avgpool.weight": torch.zeros(1)})
    bad = dict(sd, **{"lin2.model.1.weight": torch.zeros(1, 383, 1, 1), "lins.2.model.1.weight": torch.zeros(1, 383, 1, 1)})
    with pytest.raises(RuntimeError, match="size mismatch"):
        build_lpips(bad)


# ---------------------------------------------------------------------------------------------------------------- C ABI, host side
def _handle(sd=None):
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.cid_lpips_create(ctypes.byref(h)) == 0
    for k, v in (sd or {}).items():
        if k.startswith("lins."):
            continue
        a = np.ascontiguousarray(v, dtype=np.float32)
        shape = (ctypes.c_int64 * a.ndim)(*a.shape)
        assert L.cid_lpips_set_weight(h, k.encode(), a.ctypes.data, shape, a.ndim) == 0, k
    return L, h


def test_set_weight_and_missing():
    sd = synth.make_lpips_state_dict("default")
    L, h = _handle()
    n = ctypes.c_int(-1)
    assert L.cid_lpips_missing_weights(h, ctypes.byref(n)) == 0 and n.value == 17
    a = np.zeros((64, 3, 11, 11), dtype=np.float32)
    s4 = (ctypes.c_int64 * 4)(64, 3, 11, 11)
    assert L.cid_lpips_set_weight(h, b"net.slice1.0.weight", a.ctypes.data, s4, 4) == 0
    assert L.cid_lpips_set_weight(h, b"lins.0.model.1.weight", a.ctypes.data, s4, 4) == ERR_KEY
    assert L.cid_lpips_set_weight(h, b"features.0.weight", a.ctypes.data, s4, 4) == ERR_KEY
    assert b"features.0.weight" in L.cid_lpips_last_error(h)
    assert L.cid_lpips_set_weight(h, b"net.slice2.3.weight", a.ctypes.data, s4, 4) == ERR_SHAPE
    assert L.cid_lpips_set_weight(h, b"net.slice1.0.weight", a.ctypes.data, s4, 3) == ERR_SHAPE
    assert L.cid_lpips_set_weight(h, b"scaling_layer.shift", a.ctypes.data, (ctypes.c_int64 * 1)(3), 1) == ERR_SHAPE
    assert L.cid_lpips_set_weight(h, None, a.ctypes.data, s4, 4) == ERR_INVALID
    assert L.cid_lpips_set_weight(h, b"net.slice1.0.weight", None, s4, 4) == ERR_INVALID
    assert L.cid_lpips_missing_weights(h, ctypes.byref(n)) == 0 and n.value == 16
    # upload with a tensor missing, a null or misaligned blob: all found before any device call
    assert L.cid_lpips_upload_weights(h, ctypes.c_void_p(4096), None) == ERR_STATE
    assert L.cid_lpips_upload_weights(h, None, None) == ERR_INVALID
    assert L.cid_lpips_upload_weights(h, ctypes.c_void_p(4100), None) == ERR_WORKSPACE
    L.cid_lpips_destroy(h)
    L, h = _handle(sd)
    assert L.cid_lpips_missing_weights(h, ctypes.byref(n)) == 0 and n.value == 0
    floats = 363 * 64 + 128 + sum(co * ci * k * k + co for co, ci, k in ((192, 64, 5), (384, 192, 3), (256, 384, 3), (256, 256, 3))) + 1152
    assert L.cid_lpips_packed_weights_bytes(h) == 4 * floats     # every segment is already a multiple of 64 floats
    L.cid_lpips_destroy(h)
    assert L.cid_lpips_create(None) == ERR_INVALID
    assert L.cid_lpips_last_error(None) == b"null handle"


def test_workspace_bytes_and_stage_view():
    L = _lib.lib()
    nb = ctypes.c_size_t()

    def expect(n, h, w):
        total = 0
        s = lpips_oracle.sizes(h, w)
        for c, (hs, ws) in zip((64, 192, 384, 256, 256), (s[0], s[1], s[2], s[2], s[2])):
            total += (2 * n * c * hs * ws * 4 + 255) // 256 * 256
        return total

    for n, h, w in ((1, 31, 31), (3, 35, 47), (19, 128, 128), (1, 200, 136), (2, 512, 384), (1, 1024, 1024)):
        assert L.cid_lpips_workspace_bytes(n, h, w, ctypes.byref(nb)) == 0, (n, h, w)
        assert nb.value == expect(n, h, w)
    for n, h, w in ((1, 30, 31), (1, 31, 30), (0, 64, 64), (-1, 64, 64), (1, 30, 30), ((1 << 20) + 1, 31, 31), (1, 31, 1 << 30)):
        assert L.cid_lpips_workspace_bytes(n, h, w, ctypes.byref(nb)) == ERR_SHAPE, (n, h, w)
    assert L.cid_lpips_workspace_bytes(1, 64, 64, None) == ERR_INVALID
    off, c, hs, ws, cb = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    refs = [ctypes.byref(v) for v in (off, c, hs, ws, cb)]
    at = 0
    sz = lpips_oracle.sizes(35, 47)
    for k, (name, ch) in enumerate(zip(lpips_oracle.TAPS, (64, 192, 384, 256, 256))):
        assert L.cid_lpips_stage_view(name.encode(), 3, 35, 47, *refs) == 0
        assert (off.value, c.value, (hs.value, ws.value), cb.value) == (at, ch, sz[min(k, 2)], 8)
        at += (2 * 3 * ch * hs.value * ws.value * 4 + 255) // 256 * 256
    assert L.cid_lpips_stage_view(b"relu6", 3, 35, 47, *refs) == ERR_KEY
    assert L.cid_lpips_stage_view(b"pool1", 3, 35, 47, *refs) == ERR_KEY
    assert L.cid_lpips_stage_view(b"relu1", 3, 30, 47, *refs) == ERR_SHAPE
    assert L.cid_lpips_stage_view(None, 3, 35, 47, *refs) == ERR_INVALID


def test_forward_argument_errors_need_no_device():
    """Everything cid_lpips refuses is refused before any launch, so host addresses are enough."""
    L, h = _handle()
    nb = ctypes.c_size_t()
    assert L.cid_lpips_workspace_bytes(2, 35, 47, ctypes.byref(nb)) == 0
    A, B, OUT, LAY, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x100000

    def call(a=A, fa=0, b=B, fb=0, n=2, hh=35, ww=47, flags=0, out=OUT, lay=LAY, ws=WS, wsb=None, handle=h):
        return L.cid_lpips(handle, a, fa, b, fb, n, hh, ww, flags, out, lay, ws, nb.value if wsb is None else wsb, None)

    assert call(handle=None) == ERR_INVALID
    for kw in (dict(a=None), dict(b=None), dict(out=None), dict(ws=None), dict(fa=2), dict(fb=-1), dict(a=A + 2), dict(b=B + 1),
               dict(out=OUT + 4), dict(lay=LAY + 4), dict(flags=2), dict(flags=3)):
        assert call(**kw) == ERR_INVALID, kw
    assert call(a=A + 1, fa=1, b=B + 3, fb=1, lay=None) == ERR_STATE       # uint8 operands need no alignment, layers may be null
    for kw in (dict(n=0), dict(hh=30), dict(ww=30), dict(n=(1 << 20) + 1)):
        assert call(**kw) == ERR_SHAPE, kw
    assert call(wsb=nb.value - 1) == ERR_WORKSPACE
    assert call(ws=WS + 128) == ERR_WORKSPACE
    assert call() == ERR_STATE and b"not uploaded" in L.cid_lpips_last_error(h)
    L.cid_lpips_destroy(h)


def test_python_surface_without_a_model():
    import celebrity_image_denoiser_amd as cid

    assert cid.LPIPS is LPIPS and callable(cid.load_lpips)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(TypeError):
        metrics.lpips(x, x, model=None)
    with pytest.raises(ValueError):
        metrics._quality_table(x, x, ("lpips",))       # quality() keeps rejecting "lpips"
    m = LPIPS()
    with pytest.raises(RuntimeError, match="GPU-only"):
        m.distances(x, x)
    with pytest.raises(ValueError, match="same dimensions"):
        m.distances(x, torch.zeros(1, 3, 64, 60))
    with pytest.raises(RuntimeError, match="expected float32"):
        m.distances(x.double(), x.double())
    import inspect

    assert inspect.signature(metrics.evaluate).parameters["lpips"].default is None
    assert inspect.signature(cid.evaluate_noise_types).parameters["lpips"].default is None
