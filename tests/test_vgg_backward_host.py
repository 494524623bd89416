"""The VGG content loss's input gradient without a GPU: the backward weight pack against a numpy restatement, the saved arena's sizes
and views, the argument errors of cid_vgg_content_loss_saved and cid_vgg_content_backward (host addresses only: everything refused is
refused before any launch), the VGGPerceptualLoss(autograd=True) container, and the manual float64 backward the GPU tests use
(vgg_backward_ref.py) against torch autograd."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from celebrity_image_denoiser_amd import _lib
from celebrity_image_denoiser_amd.lpips import VGGPerceptualLoss, build_vgg_loss

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_vgg_oracle as oracle  # noqa: E402
import vgg_backward_ref as ref  # noqa: E402

ERR_INVALID, ERR_SHAPE, ERR_KEY, ERR_STATE, ERR_WORKSPACE = 1, 2, 3, 4, 5
CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256))
# the arena, in order: (name, images per pair-batch image, channels, level)
ARENA = ([(n, 2, c, k) for n, c, k in zip(ref.ACTS, (64, 64, 128, 128, 256, 256, 256), (0, 0, 1, 1, 2, 2, 2))] +
         [(n, 1, c, k) for n, c, k in zip(ref.GRADS, (256, 256, 256, 128, 128, 64, 64), (2, 2, 2, 2, 1, 1, 0))])


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


def backward_blob(sd):
    """The blob of cid_vgg_upload_backward_weights, restated: the head as hb[(t * 64 + co) * 3 + ci] = w[co][ci][2 - t/3][2 - t%3], then
    per trunk convolution (features 2, 5, 7, 10, 12, 14) the flipped, transposed weights w'[ci][co][kh][kw] = w[co][ci][2-kh][2-kw]
    packed as a convolution of co -> ci channels with oracle.windex."""
    w0 = np.asarray(sd["net.slice1.0.weight"])                      # [64,3,3,3]
    head = np.ascontiguousarray(w0[:, :, ::-1, ::-1].transpose(2, 3, 0, 1)).reshape(-1)      # [kh', kw', co, ci]
    parts = [head.astype(np.float32)]
    for idx, cin, cout in CONVS[1:]:
        w = np.asarray(sd[f"net.slice{ref.SLICE[ref.IDX.index(idx)]}.{idx}.weight"])          # [cout, cin, 3, 3]
        wt = np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))                 # w'[ci][co][kh][kw]
        o, i, kh, kw = np.meshgrid(np.arange(cin), np.arange(cout), np.arange(3), np.arange(3), indexing="ij")
        seg = np.empty(wt.size, dtype=np.float32)
        seg[oracle.windex(cout, o, i, kh, kw).reshape(-1)] = wt.reshape(-1)
        parts.append(seg)
    return np.concatenate(parts)


def test_backward_pack_matches_the_numpy_restatement():
    """cid_vgg_upload_backward_weights packs on the host before it copies; the staging copy is not reachable from here, so the pack is
    compared where it is visible: the blob's size here, the uploaded words in test_vgg_backward.py (which imports backward_blob)."""
    sd = oracle.weights("default")
    L, h = _handle(sd)
    floats = 9 * 64 * 3 + sum(co * ci * 9 for _, ci, co in CONVS[1:])
    assert L.cid_vgg_backward_weights_bytes(h) == 4 * floats
    assert L.cid_vgg_backward_weights_bytes(None) == 0
    want = backward_blob(sd)
    assert want.size == floats and want.dtype == np.float32
    # the restatement's own shape: the flip and the transpose, spot-checked against the definition
    w = np.asarray(sd["net.slice2.5.weight"])      # [128, 64, 3, 3]: gradient channels 128 -> input channels 64
    off = 9 * 64 * 3 + 64 * 64 * 9
    for co, ci, kh, kw in ((0, 0, 0, 0), (127, 63, 2, 1), (5, 9, 1, 2), (64, 33, 0, 2)):
        assert want[off + oracle.windex(128, ci, co, kh, kw)] == w[co, ci, 2 - kh, 2 - kw]
    w0 = np.asarray(sd["net.slice1.0.weight"])
    for t, co, ci in ((0, 0, 0), (8, 63, 2), (5, 17, 1)):
        assert want[(t * 64 + co) * 3 + ci] == w0[co, ci, 2 - t // 3, 2 - t % 3]
    # the packed blobs of the forward stay what lpips_vgg_oracle.packed_blob restates
    assert L.cid_vgg_packed_weights_bytes(h) == 4 * oracle.packed_blob(sd).size
    # upload: every answer below comes before any device call
    assert L.cid_vgg_upload_backward_weights(None, ctypes.c_void_p(4096), None) == ERR_INVALID
    assert L.cid_vgg_upload_backward_weights(h, None, None) == ERR_INVALID
    assert L.cid_vgg_upload_backward_weights(h, ctypes.c_void_p(4100), None) == ERR_WORKSPACE
    L.cid_vgg_destroy(h)
    L, h = _handle(sd, lambda k: k != "net.slice3.12.weight")
    assert L.cid_vgg_upload_backward_weights(h, ctypes.c_void_p(4096), None) == ERR_STATE
    assert b"net.slice3.12.weight" in L.cid_vgg_last_error(h)
    L.cid_vgg_destroy(h)
    # the 14 tensors of slice1 ... slice3 are enough
    L, h = _handle(sd, lambda k: k.startswith(("net.slice1.", "net.slice2.", "net.slice3.")))
    assert L.cid_vgg_upload_backward_weights(h, ctypes.c_void_p(4100), None) == ERR_WORKSPACE
    L.cid_vgg_destroy(h)


def _expect_arena(n, h, w):
    sz = oracle.sizes(h, w)
    a256 = lambda v: (v + 255) // 256 * 256   # noqa: E731
    at, out = 0, {}
    for name, towers, c, k in ARENA:
        out[name] = (at, towers * n, c, sz[k])
        at += a256(towers * n * c * sz[k][0] * sz[k][1] * 4)
    return out, at


def test_saved_bytes_and_view():
    L = _lib.lib()
    nb = ctypes.c_size_t()
    off, im, c, hs, ws, cb = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    refs = [ctypes.byref(v) for v in (off, im, c, hs, ws, cb)]
    for n, h, w in ((2, 4, 4), (130, 4, 4), (3, 5, 7), (3, 17, 19), (3, 35, 47), (2, 64, 64), (1, 4, 512), (16, 256, 256), (2, 512, 512)):
        want, total = _expect_arena(n, h, w)
        assert L.cid_vgg_saved_bytes(n, h, w, ctypes.byref(nb)) == 0 and nb.value == total, (n, h, w)
        assert len(want) == 14
        for name, (at, images, ch, (hh, ww)) in want.items():
            assert L.cid_vgg_saved_view(name.encode(), n, h, w, *refs) == 0, name
            assert (off.value, im.value, c.value, hs.value, ws.value, cb.value) == (at, images, ch, hh, ww, 8), name
            assert off.value % 256 == 0
        # the plain call's three taps are among them, at the plain call's sizes
        for tap, name in (("relu1", "relu1_2"), ("relu2", "relu2_2"), ("relu3", "relu3_3")):
            o2, c2, h2, w2, b2 = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            assert L.cid_vgg_stage_view(1, tap.encode(), n, h, w, *[ctypes.byref(v) for v in (o2, c2, h2, w2, b2)]) == 0
            assert (c2.value, (h2.value, w2.value)) == (want[name][2], want[name][3])
    for stage in (b"relu1", b"relu3_4", b"relu4_1", b"grad2_2", b"grad1_2", b"grad_x", b"pool1", b""):
        assert L.cid_vgg_saved_view(stage, 3, 35, 47, *refs) == ERR_KEY, stage
    assert L.cid_vgg_saved_view(None, 3, 35, 47, *refs) == ERR_INVALID
    assert L.cid_vgg_saved_view(b"relu1_1", 3, 35, 47, None, *refs[1:]) == ERR_INVALID
    assert L.cid_vgg_saved_bytes(3, 35, 47, None) == ERR_INVALID
    # the forward's shape limits: 4 <= H, W <= 512, 1 <= N <= 2^20
    for n, h, w in ((0, 64, 64), (-1, 64, 64), ((1 << 20) + 1, 16, 16), (1, 3, 4), (1, 4, 3), (1, 513, 16), (1, 16, 513), (1 << 20, 512, 512)):
        assert L.cid_vgg_saved_bytes(n, h, w, ctypes.byref(nb)) == ERR_SHAPE, (n, h, w)
        assert L.cid_vgg_saved_view(b"relu1_1", n, h, w, *refs) == ERR_SHAPE, (n, h, w)
    # the plain workspace's forms are unchanged
    assert L.cid_vgg_workspace_bytes(2, 1, 64, 64, ctypes.byref(nb)) == ERR_INVALID


def test_argument_errors_need_no_device():
    """Everything cid_vgg_content_loss_saved and cid_vgg_content_backward refuse is refused before any launch."""
    L, h = _handle()
    nb = ctypes.c_size_t()
    assert L.cid_vgg_saved_bytes(2, 35, 47, ctypes.byref(nb)) == 0
    A, B, OUT, GO, GA, SV = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x100000

    def fwd(a=A, fa=0, b=B, fb=0, n=2, hh=35, ww=47, flags=0, out=OUT, sv=SV, svb=None, handle=h):
        return L.cid_vgg_content_loss_saved(handle, a, fa, b, fb, n, hh, ww, flags, out, sv, nb.value if svb is None else svb, None)

    def bwd(go=GO, ga=GA, n=2, hh=35, ww=47, flags=0, sv=SV, svb=None, handle=h):
        return L.cid_vgg_content_backward(handle, go, ga, n, hh, ww, flags, sv, nb.value if svb is None else svb, None)

    assert fwd(handle=None) == ERR_INVALID and bwd(handle=None) == ERR_INVALID
    for kw in (dict(a=None), dict(b=None), dict(out=None), dict(sv=None), dict(fa=2), dict(fb=-1), dict(a=A + 2), dict(b=B + 1),
               dict(out=OUT + 4), dict(flags=2), dict(flags=3)):
        assert fwd(**kw) == ERR_INVALID, kw
    # operand a as uint8 has no gradient: refused; b may be uint8 (and then needs no alignment)
    assert fwd(fa=1) == ERR_INVALID and b"fp32" in L.cid_vgg_last_error(h)
    assert fwd(fa=1, fb=1) == ERR_INVALID
    assert fwd(b=B + 3, fb=1) == ERR_STATE
    for kw in (dict(go=None), dict(ga=None), dict(sv=None), dict(go=GO + 4), dict(ga=GA + 2), dict(flags=2), dict(flags=3)):
        assert bwd(**kw) == ERR_INVALID, kw
    for call in (fwd, bwd):
        for kw in (dict(n=0), dict(hh=3), dict(ww=3), dict(hh=513), dict(ww=513), dict(n=(1 << 20) + 1)):
            assert call(**kw) == ERR_SHAPE, kw
        assert call(sv=SV + 128) == ERR_WORKSPACE
        assert call(svb=nb.value - 1) == ERR_WORKSPACE
        assert call(svb=1024) == ERR_WORKSPACE
        assert call() == ERR_STATE and b"not uploaded" in L.cid_vgg_last_error(h)
        assert call(flags=1) == ERR_STATE
    # the plain workspace is smaller than the arena: a buffer sized for the plain call is refused
    ws = ctypes.c_size_t()
    assert L.cid_vgg_workspace_bytes(1, 2, 35, 47, ctypes.byref(ws)) == 0 and ws.value < nb.value
    assert fwd(svb=ws.value) == ERR_WORKSPACE
    L.cid_vgg_destroy(h)


def test_autograd_container():
    for m in (VGGPerceptualLoss(autograd=True), build_vgg_loss({k: torch.from_numpy(v) for k, v in _ref_names().items()}, autograd=True)):
        want = []
        for idx, cin, cout in CONVS:
            want += [(f"slice.{idx}.weight", (cout, cin, 3, 3)), (f"slice.{idx}.bias", (cout,))]
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
        assert not m.training and not any(p.requires_grad for p in m.parameters())
        assert m.autograd is True
    assert VGGPerceptualLoss().autograd is False and build_vgg_loss({k: torch.from_numpy(v) for k, v in _ref_names().items()}).autograd is False
    x = torch.zeros(1, 3, 8, 8, requires_grad=True)
    with pytest.raises(RuntimeError, match="GPU-only"):
        VGGPerceptualLoss(autograd=True)(x, torch.zeros(1, 3, 8, 8))


def _ref_names():
    from celebrity_image_denoiser_amd import synth

    return synth.vgg_loss_state_dict(oracle.weights("hot"))


@pytest.mark.parametrize("wset", ["default", "hot"])
@pytest.mark.parametrize("case", [(5, 7, 3), (17, 19, 2)], ids=lambda c: f"{c[0]}x{c[1]}n{c[2]}")
def test_manual_backward_is_autograd_in_float64(case, wset):
    """backward64 with its own masks and routing equals torch autograd of F.mse_loss(slice(x), slice(y)) in float64, to 1e-12
    relative; with per-image weights it equals autograd of the weighted sum, and the unit view carries the factor 0.5."""
    h, w, n = case
    sd = oracle.weights(wset)
    a, b, _, _ = oracle.pairs("unrelated", n, h, w, oracle.first_index(h, w, n))
    for unit, go in ((False, np.full(n, 1.0 / n)), (True, np.linspace(0.25, 1.75, n))):
        x = torch.from_numpy(a).double().requires_grad_(True)

        def slice64(v):
            v = v * 0.5 + 0.5 if unit else v
            for i in range(7):
                if ref.POOL_BEFORE[i]:
                    v = F.max_pool2d(v, 2, 2)
                wt, bias = ref.params(sd, i, torch.float64)
                v = F.relu(F.conv2d(v, wt, bias, padding=1))
            return v

        fb = slice64(torch.from_numpy(b).double()).detach()
        if unit:
            (((slice64(x) - fb) ** 2).mean(dim=(1, 2, 3)) * torch.from_numpy(go)).sum().backward()
        else:
            F.mse_loss(slice64(x), fb).backward()
        _, act = ref.forward64(sd, a, unit)
        _, act_b = ref.forward64(sd, b, unit)
        assert torch.equal(act_b[6], fb)
        masks, routes = ref.own_discontinuities(act)
        g = ref.backward64(sd, act, act_b[6], go, masks, routes, unit)
        assert g["grad_x"].shape == x.grad.shape and float(x.grad.abs().max()) > 0
        assert ref.rel_err(g["grad_x"], x.grad) <= 1e-12
