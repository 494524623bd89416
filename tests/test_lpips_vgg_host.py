"""VGG16 features without a GPU: the float64 oracle against the recorded ATen fp32 fixtures, the synthetic weight sets, the key table,
the upload states, both loader layouts, the host side of cid_vgg_* (include/cid.h) and the VGGPerceptualLoss container."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib, metrics, synth
from celebrity_image_denoiser_amd.lpips import LPIPS, VGGPerceptualLoss, build_lpips, build_vgg_loss, lpips_state_dict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_vgg_oracle as oracle  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ERR_INVALID, ERR_SHAPE, ERR_KEY, ERR_STATE, ERR_WORKSPACE = 1, 2, 3, 4, 5
LPIPS_FORM, CONTENT_FORM = 0, 1
CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (17, 256, 512),
         (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))
SLICE_OF = {0: 1, 2: 1, 5: 2, 7: 2, 10: 3, 12: 3, 14: 3, 17: 4, 19: 4, 21: 4, 24: 5, 26: 5, 28: 5}


def _tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _digest(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------- the oracle
def test_oracle_sizes_and_identities():
    assert oracle.sizes(16, 16) == ((16, 16), (8, 8), (4, 4), (2, 2), (1, 1))
    assert oracle.sizes(17, 19) == ((17, 19), (8, 9), (4, 4), (2, 2), (1, 1))
    assert oracle.sizes(35, 47) == ((35, 47), (17, 23), (8, 11), (4, 5), (2, 2))
    sd = oracle.weights("hot")
    a, b, _, _ = oracle.pairs("unrelated", 2, 17, 19)
    ab, ba, aa = oracle.forward(sd, a, b), oracle.forward(sd, b, a), oracle.forward(sd, a, a)
    assert [ab[t].shape for t in oracle.TAPS] == [(4, 64, 17, 19), (4, 128, 8, 9), (4, 256, 4, 4), (4, 512, 2, 2), (4, 512, 1, 1)]
    assert np.array_equal(aa["d"], np.zeros(2)) and np.array_equal(aa["layers"], np.zeros((2, 5)))
    assert np.array_equal(ab["d"], ba["d"]) and np.array_equal(ab["layers"], ba["layers"]) and (ab["d"] > 0).all()
    c = oracle.content(sd, a, b)
    assert c["loss"].shape == (2,) and (c["loss"] > 0).all() and c["relu3"].shape == (4, 256, 4, 4)
    assert np.array_equal(oracle.content(sd, a, a)["loss"], np.zeros(2))
    # the content loss reads its operands unscaled: it is not the LPIPS tower's relu3
    assert np.abs(c["relu3"] - ab["relu3"]).max() > 1e-3


def test_oracle_agrees_with_the_recorded_aten_fp32():
    """The fixtures hold ATen fp32's values of a plain torch.nn build of the network (make_lpips_vgg_golden.py): the oracle stands
    inside the bounds the maker asserted."""
    stats = json.load(open(os.path.join(GOLDEN, "lpips_vgg_stats.json")))
    assert stats["worst_fp32_tap_error"] <= 2e-6 and stats["worst_fp32_distance_error"] <= 1e-5 and stats["worst_fp32_loss_error"] <= 1e-5
    for wset in ("default", "hot"):
        sd = oracle.weights(wset)
        for kind in ("noisy", "unrelated"):
            fx = np.load(os.path.join(GOLDEN, f"lpips_vgg_{wset}_{kind}_35x47_n3.npz"))
            assert int(fx["first_index"]) == oracle.first_index(35, 47, 3)
            a, b, _, _ = oracle.pairs(kind, 3, 35, 47, int(fx["first_index"]))
            r = oracle.forward(sd, a, b, bool(fx["unit_view"]))
            assert np.abs(fx["relu5"] - r["relu5"]).max() <= oracle.bound(r["relu5"]) / 5
            assert (np.abs(fx["d"] - r["d"]) <= 1e-5 * np.abs(r["d"])).all()
            assert (np.abs(fx["layers"] - r["layers"]) <= 1e-5 * np.abs(r["layers"])).all()
            c = oracle.content(sd, a, b)
            assert (np.abs(fx["loss"] - c["loss"]) <= 1e-5 * np.abs(c["loss"])).all()


# ---------------------------------------------------------------------------------------------------------------- weights and keys
def test_synth_weights_are_reproducible():
    want = json.load(open(os.path.join(GOLDEN, "lpips_vgg_synth_digests.json")))
    alex = json.load(open(os.path.join(GOLDEN, "lpips_synth_digests.json")))
    for wset in ("default", "hot"):
        sd = synth.make_lpips_state_dict(wset, net="vgg")
        assert _digest(sd) == want[wset]
        assert _digest(synth.make_lpips_state_dict(wset)) == alex[wset]                 # the default output is unchanged
        assert _digest(synth.make_lpips_state_dict(wset, net="alex")) == alex[wset]
        for k, c in enumerate((64, 128, 256, 512, 512)):
            w = sd[f"lin{k}.model.1.weight"]
            assert w.shape == (1, c, 1, 1) and (w >= 0).all() and 0.7 < float(w.sum()) < 1.3
            assert sd[f"lins.{k}.model.1.weight"] is w
        w = sd["net.slice3.12.weight"]
        gain = 12.0 if wset == "hot" else 6.0
        assert w.shape == (256, 256, 3, 3) and np.abs(w).max() <= np.sqrt(gain / (256 * 9)) and np.abs(w).max() > 0.99 * np.sqrt(gain / (256 * 9))
        assert np.abs(sd["net.slice3.12.bias"]).max() <= (0.5 if wset == "hot" else 0.05)
    with pytest.raises(ValueError):
        synth.make_lpips_state_dict("cold", net="vgg")
    with pytest.raises(ValueError):
        synth.make_lpips_state_dict("default", net="squeeze")


def test_key_table():
    shapes = synth.lpips_param_shapes("vgg")
    want = ["scaling_layer.shift", "scaling_layer.scale"]
    for idx, cin, cout in CONVS:
        want += [f"net.slice{SLICE_OF[idx]}.{idx}.weight", f"net.slice{SLICE_OF[idx]}.{idx}.bias"]
    want += [f"lin{k}.model.1.weight" for k in range(5)]
    assert len(want) == 33 == _lib.CID_VGG_NUM_WEIGHTS
    m = LPIPS(net="vgg")
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == list(shapes.items())
    assert [k for k in shapes if not k.startswith("lins.")] == want
    assert [k for k in shapes if k.startswith("lins.")] == [f"lins.{k}.model.1.weight" for k in range(5)]      # the aliases
    assert all(m.lins[k] is getattr(m, f"lin{k}") for k in range(5))
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.cid_vgg_create(ctypes.byref(h)) == 0
    assert [L.cid_vgg_param_key(h, i).decode() for i in range(33)] == want
    assert L.cid_vgg_param_key(h, 33) is None and L.cid_vgg_param_key(h, -1) is None
    L.cid_vgg_destroy(h)
    assert not m.training and not any(p.requires_grad for p in m.parameters())
    # the default net is unchanged
    assert [(k, tuple(v.shape)) for k, v in LPIPS().state_dict().items()] == list(synth.lpips_param_shapes().items())
    with pytest.raises(ValueError):
        LPIPS(net="squeeze")


def _handle(sd=None, keep=lambda k: True):
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.cid_vgg_create(ctypes.byref(h)) == 0
    for k, v in (sd or {}).items():
        if k.startswith("lins.") or not keep(k):
            continue
        a = np.ascontiguousarray(v, dtype=np.float32)
        shape = (ctypes.c_int64 * a.ndim)(*a.shape)
        assert L.cid_vgg_set_weight(h, k.encode(), a.ctypes.data, shape, a.ndim) == 0, k
    return L, h


def test_set_weight_errors():
    L, h = _handle()
    n = ctypes.c_int(-1)
    assert L.cid_vgg_missing_weights(h, ctypes.byref(n)) == 0 and n.value == 33
    a = np.zeros((64, 3, 3, 3), dtype=np.float32)
    s4 = (ctypes.c_int64 * 4)(64, 3, 3, 3)
    assert L.cid_vgg_set_weight(h, b"net.slice1.0.weight", a.ctypes.data, s4, 4) == 0
    assert L.cid_vgg_set_weight(h, b"lins.0.model.1.weight", a.ctypes.data, s4, 4) == ERR_KEY
    assert L.cid_vgg_set_weight(h, b"features.0.weight", a.ctypes.data, s4, 4) == ERR_KEY
    assert b"features.0.weight" in L.cid_vgg_last_error(h)
    assert L.cid_vgg_set_weight(h, b"net.slice2.3.weight", a.ctypes.data, s4, 4) == ERR_KEY          # AlexNet's name
    assert L.cid_vgg_set_weight(h, b"net.slice1.2.weight", a.ctypes.data, s4, 4) == ERR_SHAPE
    assert L.cid_vgg_set_weight(h, b"net.slice1.0.weight", a.ctypes.data, s4, 3) == ERR_SHAPE
    assert L.cid_vgg_set_weight(h, b"lin4.model.1.weight", a.ctypes.data, (ctypes.c_int64 * 4)(1, 256, 1, 1), 4) == ERR_SHAPE
    assert L.cid_vgg_set_weight(h, None, a.ctypes.data, s4, 4) == ERR_INVALID
    assert L.cid_vgg_set_weight(h, b"net.slice1.0.weight", None, s4, 4) == ERR_INVALID
    assert L.cid_vgg_missing_weights(h, ctypes.byref(n)) == 0 and n.value == 32
    L.cid_vgg_destroy(h)
    assert L.cid_vgg_create(None) == ERR_INVALID
    assert L.cid_vgg_last_error(None) == b"null handle"


def test_upload_states():
    """All 33 tensors or exactly the 14 of slice1 ... slice3; the answer comes before any device call, so a host address that is
    null or misaligned tells which way the check went."""
    sd = oracle.weights("default")
    content = lambda k: k.startswith(("net.slice1.", "net.slice2.", "net.slice3."))   # noqa: E731
    n = ctypes.c_int(-1)

    def state(keep, want_missing):
        L, h = _handle(sd, keep)
        assert L.cid_vgg_missing_weights(h, ctypes.byref(n)) == 0 and n.value == want_missing
        rc = L.cid_vgg_upload_weights(h, ctypes.c_void_p(4100), None)     # a complete set reaches the alignment check
        assert L.cid_vgg_upload_weights(h, None, None) == ERR_INVALID
        L.cid_vgg_destroy(h)
        return rc

    assert state(lambda k: True, 0) == ERR_WORKSPACE                                      # 33: complete
    assert state(content, 19) == ERR_WORKSPACE                                            # 14: the content-loss handle
    assert state(lambda k: content(k) and k != "net.slice3.14.bias", 20) == ERR_STATE     # 13
    assert state(lambda k: content(k) or k == "lin0.model.1.weight", 18) == ERR_STATE     # 14 + one lin
    assert state(lambda k: content(k) or k.startswith("scaling_layer."), 17) == ERR_STATE
    assert state(lambda k: k != "lin3.model.1.weight", 1) == ERR_STATE                    # 32
    # 14 tensors, but not slice1 ... slice3
    assert state(lambda k: (content(k) and k != "net.slice1.0.bias") or k == "net.slice4.17.bias", 19) == ERR_STATE
    assert state(lambda k: False, 33) == ERR_STATE


def _expect_bytes(form, n, h, w):
    sz = oracle.sizes(h, w)
    a256 = lambda v: (v + 255) // 256 * 256   # noqa: E731
    total = a256(2 * n * 64 * h * w * 4) + a256(2 * n * 256 * sz[2][0] * sz[2][1] * 4)
    for c, (hs, ws) in list(zip(oracle.CHANNELS, sz))[:5 if form == LPIPS_FORM else 3]:
        total += a256(2 * n * c * hs * ws * 4)
    return total


def test_workspace_bytes_and_stage_view():
    L = _lib.lib()
    nb = ctypes.c_size_t()
    assert _lib.CID_VGG_MAX_SIDE == 512
    for form in (LPIPS_FORM, CONTENT_FORM):
        for n, h, w in ((1, 16, 16), (3, 35, 47), (19, 128, 128), (1, 20, 264), (1, 16, 512), (2, 512, 512), (1 << 20, 16, 16)):
            assert L.cid_vgg_workspace_bytes(form, n, h, w, ctypes.byref(nb)) == 0, (form, n, h, w)
            assert nb.value == _expect_bytes(form, n, h, w)
        for n, h, w in ((0, 64, 64), (-1, 64, 64), ((1 << 20) + 1, 16, 16), (1, 513, 16), (1, 16, 513), (1, 1024, 1024), (1, 16, 1 << 30),
                        (1 << 20, 512, 512)):
            assert L.cid_vgg_workspace_bytes(form, n, h, w, ctypes.byref(nb)) == ERR_SHAPE, (form, n, h, w)
    for h, w in ((15, 16), (16, 15), (15, 15)):
        assert L.cid_vgg_workspace_bytes(LPIPS_FORM, 1, h, w, ctypes.byref(nb)) == ERR_SHAPE
        assert L.cid_vgg_workspace_bytes(CONTENT_FORM, 1, h, w, ctypes.byref(nb)) == 0
    for h, w in ((3, 4), (4, 3), (3, 3)):
        assert L.cid_vgg_workspace_bytes(CONTENT_FORM, 1, h, w, ctypes.byref(nb)) == ERR_SHAPE
    assert L.cid_vgg_workspace_bytes(CONTENT_FORM, 2, 4, 4, ctypes.byref(nb)) == 0 and nb.value == _expect_bytes(CONTENT_FORM, 2, 4, 4)
    assert L.cid_vgg_workspace_bytes(LPIPS_FORM, 1, 64, 64, None) == ERR_INVALID
    assert L.cid_vgg_workspace_bytes(2, 1, 64, 64, ctypes.byref(nb)) == ERR_INVALID
    off, c, hs, ws, cb = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    refs = [ctypes.byref(v) for v in (off, c, hs, ws, cb)]
    sz = oracle.sizes(35, 47)
    a256 = lambda v: (v + 255) // 256 * 256   # noqa: E731
    for form, taps in ((LPIPS_FORM, 5), (CONTENT_FORM, 3)):
        at = a256(2 * 3 * 64 * 35 * 47 * 4) + a256(2 * 3 * 256 * 8 * 11 * 4)
        for k in range(taps):
            assert L.cid_vgg_stage_view(form, oracle.TAPS[k].encode(), 3, 35, 47, *refs) == 0
            assert (off.value, c.value, (hs.value, ws.value), cb.value) == (at, oracle.CHANNELS[k], sz[k], 8)
            at += a256(2 * 3 * oracle.CHANNELS[k] * hs.value * ws.value * 4)
        assert L.cid_vgg_workspace_bytes(form, 3, 35, 47, ctypes.byref(nb)) == 0 and nb.value == at
        assert L.cid_vgg_stage_view(form, b"relu6", 3, 35, 47, *refs) == ERR_KEY
        assert L.cid_vgg_stage_view(form, b"pool1", 3, 35, 47, *refs) == ERR_KEY
        assert L.cid_vgg_stage_view(form, None, 3, 35, 47, *refs) == ERR_INVALID
    assert L.cid_vgg_stage_view(CONTENT_FORM, b"relu4", 3, 35, 47, *refs) == ERR_KEY
    assert L.cid_vgg_stage_view(LPIPS_FORM, b"relu1", 3, 15, 47, *refs) == ERR_SHAPE


def test_forward_argument_errors_need_no_device():
    """Everything cid_vgg_lpips and cid_vgg_content_loss refuse is refused before any launch, so host addresses are enough."""
    L, h = _handle()
    nb = ctypes.c_size_t()
    assert L.cid_vgg_workspace_bytes(LPIPS_FORM, 2, 35, 47, ctypes.byref(nb)) == 0
    A, B, OUT, LAY, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x100000

    def lp(a=A, fa=0, b=B, fb=0, n=2, hh=35, ww=47, flags=0, out=OUT, lay=LAY, ws=WS, wsb=None, handle=h):
        return L.cid_vgg_lpips(handle, a, fa, b, fb, n, hh, ww, flags, out, lay, ws, nb.value if wsb is None else wsb, None)

    def cl(a=A, fa=0, b=B, fb=0, n=2, hh=35, ww=47, flags=0, out=OUT, ws=WS, wsb=None, handle=h):
        return L.cid_vgg_content_loss(handle, a, fa, b, fb, n, hh, ww, flags, out, ws, nb.value if wsb is None else wsb, None)

    for call in (lp, cl):
        assert call(handle=None) == ERR_INVALID
        for kw in (dict(a=None), dict(b=None), dict(out=None), dict(ws=None), dict(fa=2), dict(fb=-1), dict(a=A + 2), dict(b=B + 1),
                   dict(out=OUT + 4), dict(flags=2), dict(flags=3)):
            assert call(**kw) == ERR_INVALID, kw
        for kw in (dict(n=0), dict(hh=3), dict(ww=3), dict(hh=513), dict(ww=513), dict(n=(1 << 20) + 1)):
            assert call(**kw) == ERR_SHAPE, kw
        assert call(ws=WS + 128) == ERR_WORKSPACE
        assert call(wsb=1024) == ERR_WORKSPACE
        assert call(a=A + 1, fa=1, b=B + 3, fb=1) == ERR_STATE         # uint8 operands need no alignment
        assert call() == ERR_STATE and b"not uploaded" in L.cid_vgg_last_error(h)
    assert lp(lay=LAY + 4) == ERR_INVALID and lp(lay=None) == ERR_STATE
    assert lp(hh=15) == ERR_SHAPE and cl(hh=15) == ERR_STATE          # the two smallest sides: 16 and 4
    assert lp(wsb=nb.value - 1) == ERR_WORKSPACE
    L.cid_vgg_destroy(h)


def test_packed_weight_index():
    """The trunk's packed layout (lp_conv_windex), restated in numpy (lpips_vgg_oracle.windex, packed_blob): the blob's size and the
    index's shape here; the uploaded blob is compared with the restatement word for word in test_lpips_vgg.py."""
    L, h = _handle(oracle.weights("default"))
    floats = 27 * 64 + 128 + sum(co * ci * 9 + co for _, ci, co in CONVS[1:]) + 1472
    assert L.cid_vgg_packed_weights_bytes(h) == 4 * floats        # every segment is already a multiple of 64 floats
    L.cid_vgg_destroy(h)

    windex = oracle.windex
    assert oracle.packed_blob(oracle.weights("default")).size == floats
    for cin, cout in ((64, 128), (512, 512)):
        co, ci, kh, kw = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(3), np.arange(3), indexing="ij")
        idx = windex(cin, co, ci, kh, kw).reshape(-1)
        assert np.array_equal(np.sort(idx), np.arange(cout * cin * 9))       # a bijection onto the segment
    assert windex(64, 0, 0, 0, 0) == 0 and windex(64, 1, 0, 0, 0) == 1 and windex(64, 0, 1, 0, 0) == 64
    assert windex(64, 0, 0, 0, 1) == 256 and windex(64, 0, 4, 0, 0) == 9 * 256 and windex(64, 64, 0, 0, 0) == 16 * 9 * 256


# ---------------------------------------------------------------------------------------------------------------- loaders
def _vgg16_state_dict(sd):
    out = {}
    for k, v in sd.items():
        if k.startswith("net.slice"):
            _, _, idx, leaf = k.split(".")
            out[f"features.{idx}.{leaf}"] = torch.from_numpy(v)
    out["classifier.0.weight"] = torch.zeros(4, 4)
    out["classifier.0.bias"] = torch.zeros(4)
    return out


def test_loader_layouts():
    sd = oracle.weights("default")
    full = build_lpips(_tensors(sd), net="vgg")
    lin_only = {k: v for k, v in _tensors(sd).items() if k.startswith("lin") and not k.startswith("lins.")}
    vgg16 = _vgg16_state_dict(sd)
    split = build_lpips(lin_only, vgg16, net="vgg")
    prefixed = {"module." + k: v for k, v in _tensors(sd).items() if not (k.startswith("lin") and not k.startswith("lins."))}
    pre = build_lpips(prefixed, net="vgg")
    for other in (split, pre):
        for (k, v), (k2, v2) in zip(full.state_dict().items(), other.state_dict().items()):
            assert k == k2 and torch.equal(v, v2), k
    for k, v in full.state_dict().items():
        assert np.array_equal(v.numpy(), sd[k]), k
    for k in range(5):   # the lins.* aliases name the same tensors
        assert full.state_dict()[f"lins.{k}.model.1.weight"].data_ptr() == full.state_dict()[f"lin{k}.model.1.weight"].data_ptr()
    assert set(lpips_state_dict(lin_only, vgg16, "vgg")) == set(sd) - {"scaling_layer.shift", "scaling_layer.scale"}
    assert full.pnet_type == "vgg" and LPIPS().pnet_type == "alex"


def test_loader_errors():
    sd = _tensors(oracle.weights("default"))
    with pytest.raises(KeyError, match="avgpool"):
        build_lpips(sd, {"avgpool.weight": torch.zeros(1)}, net="vgg")
    with pytest.raises(KeyError, match="features.3"):
        build_lpips(sd, {"features.3.weight": torch.zeros(1)}, net="vgg")      # AlexNet's index: not a vgg16 convolution
    missing = {k: v for k, v in sd.items() if k != "net.slice3.12.bias"}
    with pytest.raises(RuntimeError, match="net.slice3.12.bias"):
        build_lpips(missing, net="vgg")
    with pytest.raises(RuntimeError, match="size mismatch"):
        build_lpips(_tensors(synth.make_lpips_state_dict("default")), net="vgg")     # AlexNet's tensors: lin widths differ
    with pytest.raises(RuntimeError):
        build_lpips(sd)                                                                # and the other way round


def test_vgg_perceptual_loss_container():
    import celebrity_image_denoiser_amd as cid

    assert cid.VGGPerceptualLoss is VGGPerceptualLoss and callable(cid.load_vgg_loss)
    m = VGGPerceptualLoss()
    want = []
    for idx, cin, cout in CONVS[:7]:
        want += [(f"slice.{idx}.weight", (cout, cin, 3, 3)), (f"slice.{idx}.bias", (cout,))]
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    assert not m.training and not any(p.requires_grad for p in m.parameters())
    sd = oracle.weights("hot")
    ref_names = synth.vgg_loss_state_dict(sd)
    assert list(ref_names) == [k for k, _ in want]
    for src in (_vgg16_state_dict(sd), {k[len("features."):]: v for k, v in _vgg16_state_dict(sd).items() if k.startswith("features.")},
                _tensors(ref_names)):
        got = build_vgg_loss(src).state_dict()
        for k, v in ref_names.items():
            assert np.array_equal(got[k].numpy(), v), k
    with pytest.raises(KeyError, match="avgpool"):
        build_vgg_loss({"avgpool.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="slice.14.bias"):
        build_vgg_loss({k: v for k, v in _tensors(ref_names).items() if k != "slice.14.bias"})
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(RuntimeError, match="GPU-only"):
        m(x, x)
    with pytest.raises(ValueError, match="same dimensions"):
        m(x, torch.zeros(1, 3, 64, 60))
    v = LPIPS(net="vgg")
    with pytest.raises(RuntimeError, match="GPU-only"):
        metrics.lpips(x, x, v)
