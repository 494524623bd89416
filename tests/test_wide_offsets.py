"""Activation tensors past 2^31 elements in the families that came after the denoiser: cid_esr_forward, cid_sr_forward, cid_cg_forward,
cid_srd_forward, cid_srd_forward_saved + cid_srd_backward and cid_esd_forward (include/cid.h).

Their kernels promise 64-bit offsets ("only a pixel index inside one image is an int") and tiles that depend only on (H, W).
tests/test_large_batches.py holds them to that past 65,535 images, at 1 x 1, where every tensor is a few MiB.  Here the images are small
but not tile multiples and the batch is chosen so that at least one C8 tensor of the family holds more than 2^31 elements (and so
passes 2^31, 2^32 and 2^33 bytes): an int product in ((n * C/8 + cb) * H + y) * W + x, a 32-bit blockIdx.x * ..., a narrow stage
offset or a narrow size on the host reads or writes another image's memory there.  Every case has four parts:

  (a) crossing(family) derives, on the host, each tensor's N * C * Hs * Ws from the family's stage views and workspace functions,
      asserts that the case crosses 2^31 elements, and derives the SEAM images: image 0, image N - 1 and, for each boundary B in
      {2^29, 2^30, 2^31} elements of each tensor, the images floor(B / per-image elements) - 1, that image and + 1.
      test_the_cases_cross_what_they_claim runs it without a GPU;
  (b) the inputs are distinct images made on the device from a seeded torch.Generator; only the seam images reach the host;
  (c) the C ABI is called directly on buffers prefilled with 0xFF bytes (NaN bits): workspace, saved buffer, outputs, gradients;
  (d) every seam image's result, and every stage view's tensor, is bit-equal to the same image run alone (N = 1) through the same
      entry point in a fresh 0xFF-filled workspace, and the seam image that holds the 2^31-element boundary is held to the family's
      float64 oracle under the family's own bound, which anchors the bit comparison to something other than the code under test.

Train-mode BatchNorm (cid_esr_forward_train, cid_sr_forward_train, cid_sr_forward_saved + cid_sr_backward, cid_srd_* with
training = 1) couples the whole batch: an image alone is another computation, so (d) does not apply.  Those calls are held past 2^31
elements by tests/test_train_batches.py, on batches that repeat a block of seven images (such a batch has the block's statistics,
so the block's float64 oracle is the oracle of every image).  The cases here cover eval mode: cid_sr_forward,
cid_srd_forward(training = 0) and cid_srd_forward_saved + cid_srd_backward(training = 0).  Parameter gradients sum over the batch:
there grad_prob is zero off the seam images and the gradients are those of the seam images as a small batch, under the rule of
tests/test_srgan_disc_backward.py.

Every case needs less than the 70 GiB of test_gpu_parity.py::test_batch_past_2_31_elements_per_buffer and skips below its need plus
that test's 20 GiB of headroom; each frees its buffers afterwards.

What would fail here (reasoned from the kernels, not run): an (int) on the image term of any of these kernels' offsets, e.g.
(int)((n * 8 + cb) * HW) in k_esr_head or k_esr_conv, wraps from image floor(2^31 / per-image elements) on, so the images at and
after the 2^31 seam are written over earlier images (or outside the buffer) and their own slices keep the 0xFF prefill: the stage
views of the anchor image and of image N - 1 differ from the image alone, and the anchor misses its oracle.  The same holds for the
staged reads (the result of those images changes), for a 32-bit n * plane in a tail's store, and for a stage offset or workspace size
narrowed on the host (crossing() compares them with the documented formulas).  k_esr_tail with tx forced to 0 leaves columns 64 and up
of every 48 x 80 output at the prefill here, and fails test_esrgan.py at 1x20x70, 1x17x130 and 2x33x65.

Measured on one MI355X, whole suite in one process: esr 0.42 s, sr 0.40 s, cg 0.31 s, esd 0.38 s, srd forward 0.37 s, srd backward
0.74 s, next to 1.75 s (winograd42) and 2.32 s (winograd64) of test_batch_past_2_31_elements_per_buffer.  Worst share of the oracle bound
at the anchor image: esr 0.14 (out), sr 0.16 (trunk), cg 0.08 (t2), esd 0.11 (a3), srd forward 0.001, srd backward 0.13."""
import ctypes
import functools
import gc
import os
import sys

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cgan_oracle  # noqa: E402
import esrgan_disc_oracle  # noqa: E402
import esrgan_oracle  # noqa: E402
import srgan_disc_oracle  # noqa: E402
import srgan_oracle  # noqa: E402

DEV = "cuda:0"
F32, U8 = _lib.CID_FMT_F32_NCHW, _lib.CID_FMT_U8_NHWC
BOUNDARIES = (1 << 29, 1 << 30, 1 << 31)
GIB = 1 << 30
MEMORY_CAP, HEADROOM = 70 * GIB, 20 * GIB
# Image sizes that are no multiple of any tile of their family (trunk 16 x 16, tails 16 x 64, discriminator layers 16 / 8 / 4 rows by
# 16 columns), N the starting points of the issue adjusted until crossing() holds.
#   esr  R = 2 runs EPI_PRELU, EPI_RES (in place) and EPI_SUM; x1, the middle tensor and the tail's input are 8750 * 64 * 48 * 80 each
#   sr   scale 4 on 15 x 17: only the 60 x 68 tensor the tail reads passes 2^31; the base-resolution tensors are 16 times smaller
#   cg   one launch (N < 65,535): t3 = N * 32 * 64 * 64
#   srd  24 x 40: the layer-0 tensor a0 = N * 64 * 24 * 40
#   esd  48 x 80: a1 = N * 64 * 24 * 40
CASES = {
    "esr": dict(n=8750, h=48, w=80, r=2, wset="hot"),
    "sr": dict(n=8232, h=15, w=17, scale=4, wset="hot"),
    "cg": dict(n=16400, wset="hot", n_classes=10),
    "srd": dict(n=35000, h=24, w=40, kind="trained"),
    "esd": dict(n=35000, h=48, w=80, kind="trained"),
}


# ------------------------------------------------------------------------------------------------------------------ (a) on the host
def _a256(v):
    return (v + 255) // 256 * 256


def _size(fn, *args):
    need = ctypes.c_size_t()
    assert fn(*args, ctypes.byref(need)) == 0, (fn.__name__, args)
    return need.value


def _view(fn, stage, *dims):
    """(offset in bytes, C, Hs, Ws) of a cid_<abi>_stage_view."""
    off, c, hs, ws, cb = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert fn(stage.encode(), *dims, ctypes.byref(off), ctypes.byref(c), ctypes.byref(hs), ctypes.byref(ws), ctypes.byref(cb)) == 0, stage
    assert cb.value == 8 and off.value % 256 == 0
    return off.value, c.value, hs.value, ws.value


def _side(s):
    return (s - 1) // 2 + 1


def tensors_of(family, n):
    """What a forward over `n` images of the family's case leaves behind, from the library's own host functions.
    -> ([(name, offset in the workspace or None where no view exists, C, Hs, Ws)], workspace bytes, other bytes of the call)"""
    L = _lib.lib()
    c = CASES[family]
    if family == "esr":
        h, w = c["h"], c["w"]
        need = _size(L.cid_esr_workspace_bytes, n, h, w)
        views = [(s,) + _view(L.cid_esr_stage_view, s, n, h, w) for s in ("x1", "tail_in")]
        assert need == 3 * _a256(4 * n * 64 * h * w)                       # x1, the blocks' middle tensor, the running sum
        views.insert(1, ("mid", None, 64, h, w))
        return views, need, n * h * w * 3 + 4 * n * 3 * h * w
    if family == "sr":
        h, w, s = c["h"], c["w"], c["scale"]
        need = _size(L.cid_sr_workspace_bytes, n, h, w, s)
        views = [(k,) + _view(L.cid_sr_stage_view, k, n, h, w, s) for k in ("x0", "trunk", "up1", "tail_in")]
        return views, need, n * h * w * 3 + 4 * n * 3 * s * h * s * w
    if family == "cg":
        need = _size(L.cid_cg_workspace_bytes, n)
        views = [(k,) + _view(L.cid_cg_stage_view, k, n) for k in ("l1", "t1", "t2", "t3")]
        return views, need, 4 * n * 100 + 8 * n + 4 * n * 3 * 64 * 64
    if family == "esd":
        h, w = c["h"], c["w"]
        need = _size(L.cid_esd_workspace_bytes, n, h, w)
        offs, total = esrgan_disc_oracle.expected_workspace(n, h, w)       # the formula of include/cid.h
        assert need == total
        views = []
        for name, off, ch in zip(("a1", "a2", "a3", "a4"), offs, (64, 128, 256, 512)):
            h, w = _side(h), _side(w)
            views.append((name, off, ch, h, w))
        return views, need, n * c["h"] * c["w"] * 3 + 4 * n
    assert family == "srd"
    h, w = c["h"], c["w"]
    h2, w2 = _side(h), _side(w)
    h4, w4 = _side(h2), _side(w2)
    # the forward's regions alias (a0, then z5, then z11 in region A), so there are no views: the five tensors of include/cid.h
    views = [("a0", None, 64, h, w), ("z2", None, 64, h2, w2), ("z5", None, 128, h2, w2), ("z8", None, 128, h4, w4), ("z11", None, 256, h4, w4)]
    fwd = _size(L.cid_srd_workspace_bytes, n, h, w, 0)
    assert fwd == (_a256(4 * n * max(64 * h * w, 128 * h2 * w2, 256 * h4 * w4)) + _a256(4 * n * max(64 * h2 * w2, 128 * h4 * w4))
                   + _a256(4 * 4 * 256 * 2))
    saved = _size(L.cid_srd_saved_bytes, n, h, w, 0)
    assert saved >= sum(_a256(4 * n * ch * hh * ww) for _, _, ch, hh, ww in views)
    bwd = _size(L.cid_srd_backward_workspace_bytes, n, h, w, 0)
    # the larger of the two tests: x, the saved buffer, the backward's workspace, two input gradients, the probabilities
    return views, max(fwd, saved + bwd), 3 * 4 * n * 3 * h * w + 8 * n


def seam_images(n, per_image):
    """Image 0, image n - 1, and for each boundary B of each tensor (`per_image`: its elements per image) the image that holds element
    B and its two neighbours, where the batch has them."""
    seam = {0, n - 1}
    for per in per_image:
        for b in BOUNDARIES:
            i = b // per
            seam.update(j for j in (i - 1, i, i + 1) if 0 <= j < n)
    return sorted(seam)


def crossing(family):
    """The host side of a case: which tensors pass 2^31 elements, the seam images, the anchor image (the one that holds element 2^31
    of the largest tensor) and the device memory the case needs."""
    n = CASES[family]["n"]
    views, ws_bytes, other = tensors_of(family, n)
    per = {name: ch * hs * ws for name, _, ch, hs, ws in views}
    past = [name for name in per if n * per[name] > 1 << 31]
    assert past, (family, {k: n * v for k, v in per.items()})
    for name in past:
        assert 4 * n * per[name] > 1 << 33 and (n - 1) * per[name] > 1 << 31        # the last image lies wholly past the boundary
    largest = max(per.values())
    anchor = (1 << 31) // largest
    seam = seam_images(n, per.values())
    assert anchor in seam and anchor * largest <= 1 << 31 < (anchor + 1) * largest
    need = ws_bytes + other
    assert ws_bytes > 1 << 33 and need < MEMORY_CAP
    return dict(n=n, views=views, per=per, past=past, seam=seam, anchor=anchor, need=need)


def test_the_cases_cross_what_they_claim():
    """crossing() of every family without a GPU, and its arithmetic against figures worked out by hand."""
    assert seam_images(10, [1 << 28]) == [0, 1, 2, 3, 4, 5, 7, 8, 9]                 # boundaries at images 2, 4 and 8
    assert seam_images(5, [3]) == [0, 4] and seam_images(1, [1 << 40]) == [0]
    got = {f: crossing(f) for f in CASES}
    for f, c in got.items():
        print(f, "past 2^31 elements:", {k: c["n"] * c["per"][k] for k in c["past"]}, "seam", c["seam"], "anchor", c["anchor"],
              f"need {c['need'] / GIB:.1f} GiB")
        assert c["seam"] == sorted(set(c["seam"])) and c["seam"][0] == 0 and c["seam"][-1] == c["n"] - 1 and len(c["seam"]) <= 16
    assert got["esr"]["past"] == ["x1", "mid", "tail_in"] and got["esr"]["per"]["x1"] == 64 * 48 * 80 == 245760
    assert got["esr"]["seam"] == [0, 2183, 2184, 2185, 4368, 4369, 4370, 8737, 8738, 8739, 8749] and got["esr"]["anchor"] == 8738
    assert got["sr"]["past"] == ["tail_in"] and got["sr"]["per"] == {"x0": 16320, "trunk": 16320, "up1": 65280, "tail_in": 261120}
    assert got["sr"]["seam"] == [0, 2055, 2056, 2057, 4111, 4112, 4113, 8223, 8224, 8225, 8231]   # up1 passes 2^29 in image 8224 too
    assert got["cg"]["past"] == ["t3"] and got["cg"]["per"]["t3"] == 32 * 64 * 64
    assert got["cg"]["seam"] == [0, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 16399] and got["cg"]["anchor"] == 16384
    assert got["srd"]["past"] == ["a0"] and got["esd"]["past"] == ["a1"]
    assert got["srd"]["per"]["a0"] == got["esd"]["per"]["a1"] == 61440 and got["srd"]["seam"] == got["esd"]["seam"]
    assert got["esd"]["seam"] == [0, 8737, 8738, 8739, 17475, 17476, 17477, 34951, 34952, 34953, 34999]
    # an image alone has the same per-image sizes: the comparison with N = 1 is slice against slice
    for f in CASES:
        assert [v[2:] for v in tensors_of(f, 1)[0]] == [v[2:] for v in got[f]["views"]]


# ------------------------------------------------------------------------------------------------------------------ (b), (c) helpers
def _skip_below(need):
    """The skip rule of every case here and in test_train_batches.py: the case's own bytes plus HEADROOM must be free."""
    free, _ = torch.cuda.mem_get_info()
    if free < need + HEADROOM:
        pytest.skip(f"needs {need / GIB:.0f} GiB of free device memory and {HEADROOM // GIB} GiB of headroom")


def _case(family):
    c = crossing(family)
    _skip_below(c["need"])
    print(f"\n{family}: N = {c['n']}, past 2^31 elements: " + ", ".join(f"{k} = {c['n'] * c['per'][k]}" for k in c["past"])
          + f"; seam {c['seam']}; anchor {c['anchor']}; {c['need'] / GIB:.1f} GiB")
    return c


def _frees_its_buffers(test):
    """Give the case's device memory back once its frame is gone, as test_batch_past_2_31_elements_per_buffer does."""
    @functools.wraps(test)
    def run():
        try:
            test()
        finally:
            gc.collect()
            torch.cuda.empty_cache()
    return run


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _poisoned(nbytes):
    """0xFF bytes: NaN bits as fp32 or fp64."""
    return torch.full((max(int(nbytes), 1),), 0xFF, dtype=torch.uint8, device=DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _stage_bits(ws, view, i, per):
    """The C8 bytes of image i of a stage view."""
    return ws[view[1] + 4 * per * i:view[1] + 4 * per * (i + 1)]


def _nchw(bits, view):
    """One image's C8 bytes -> fp32 [1,C,Hs,Ws] on the host."""
    _, _, ch, hs, ws = view
    return bits.view(torch.float32).view(1, ch // 8, hs, ws, 8).permute(0, 1, 4, 2, 3).reshape(1, ch, hs, ws).cpu().numpy()


def _same_bits(family, case, big_out, big_ws, alone):
    """(d, ii): alone(i) -> (output of image i run alone, its workspace); result and stage views bit-equal to the big call's."""
    one = tensors_of(family, 1)[0]
    for i in case["seam"]:
        out1, ws1 = alone(i)
        torch.cuda.synchronize()
        assert torch.equal(big_out[i:i + 1].reshape(-1).view(torch.uint8), out1.reshape(-1).view(torch.uint8)), (family, "out", i)
        for vb, v1 in zip(case["views"], one):
            if vb[1] is not None:
                per = case["per"][vb[0]]
                assert torch.equal(_stage_bits(big_ws, vb, i, per), _stage_bits(ws1, v1, 0, per)), (family, vb[0], i)


def _share(name, got, ref64, bound):
    """err / bound of one tensor against the float64 oracle, asserted to be at most 1."""
    ref64 = np.asarray(ref64, np.float64)
    got = np.asarray(got)
    assert got.shape == ref64.shape and np.isfinite(got).all(), name
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    print(f"    {name}: max|delta| {err:.3e}, bound {bound:.3e}, share {err / bound:.3f}")
    assert err <= bound, (name, err, bound)
    return err / bound


# ------------------------------------------------------------------------------------------------------------------ cid_esr_forward
def _esr_call(m, u8):
    L = _lib.lib()
    n, h, w, _ = u8.shape
    need = _size(L.cid_esr_workspace_bytes, n, h, w)
    ws, out = _poisoned(need), _poisoned(4 * n * 3 * h * w)
    _lib.check_abi("esr", m._cid, L.cid_esr_forward(m._cid, u8.data_ptr(), U8, out.data_ptr(), F32, n, h, w, ws.data_ptr(), need, _stream()))
    return out.view(torch.float32).view(n, 3, h, w), ws


@pytest.mark.gpu
@_frees_its_buffers
def test_esr_forward():
    from celebrity_image_denoiser_amd.esrgan import load_esrgan

    c = _case("esr")
    cfg = CASES["esr"]
    sd = synth.make_esrgan_state_dict(cfg["wset"], cfg["r"])
    m = load_esrgan(sd, num_residuals=cfg["r"], device=DEV, strict=True)
    u8 = torch.randint(0, 256, (c["n"], cfg["h"], cfg["w"], 3), dtype=torch.uint8, device=DEV, generator=_gen(41))
    out, ws = _esr_call(m, u8)
    torch.cuda.synchronize()
    _same_bits("esr", c, out, ws, lambda i: _esr_call(m, u8[i:i + 1]))
    a = c["anchor"]
    x = np.ascontiguousarray((u8[a:a + 1].cpu().numpy().astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))
    ref = esrgan_oracle.forward(sd, x, cfg["r"])
    views = {v[0]: v for v in c["views"]}
    shares = [_share(k, _nchw(_stage_bits(ws, views[k], a, c["per"][k]), views[k]), ref[k], esrgan_oracle.bound(ref[k]))
              for k in ("x1", "tail_in")]
    shares.append(_share("out", out[a:a + 1].cpu().numpy(), ref["out"], esrgan_oracle.bound(ref["out"])))
    print(f"esr: worst share of the oracle bound at image {a}: {max(shares):.3f}")


# ------------------------------------------------------------------------------------------------------------------- cid_sr_forward
def _sr_call(m, u8, scale):
    L = _lib.lib()
    n, h, w, _ = u8.shape
    need = _size(L.cid_sr_workspace_bytes, n, h, w, scale)
    ws, out = _poisoned(need), _poisoned(4 * n * 3 * scale * h * scale * w)
    _lib.check_abi("sr", m._cid, L.cid_sr_forward(m._cid, u8.data_ptr(), U8, out.data_ptr(), F32, n, h, w, 0, 0, 0, 0, 0, ws.data_ptr(),
                                                  need, _stream()))
    return out.view(torch.float32).view(n, 3, scale * h, scale * w), ws


@pytest.mark.gpu
@_frees_its_buffers
def test_sr_forward():
    """Eval mode (the module docstring says why).  As in test_srgan.py the output is held to the bound of the sums before tanh."""
    from celebrity_image_denoiser_amd.srgan import load_srgan

    c = _case("sr")
    cfg = CASES["sr"]
    s = cfg["scale"]
    sd = synth.make_srgan_state_dict(cfg["wset"], s)
    m = load_srgan(sd, scale_factor=s, device=DEV, strict=True)
    u8 = torch.randint(0, 256, (c["n"], cfg["h"], cfg["w"], 3), dtype=torch.uint8, device=DEV, generator=_gen(42))
    out, ws = _sr_call(m, u8, s)
    torch.cuda.synchronize()
    _same_bits("sr", c, out, ws, lambda i: _sr_call(m, u8[i:i + 1], s))
    a = c["anchor"]
    ref = srgan_oracle.forward(sd, srgan_oracle.normalise_u8(u8[a:a + 1].cpu().numpy()))
    shares = [_share(v[0], _nchw(_stage_bits(ws, v, a, c["per"][v[0]]), v), ref[v[0]], srgan_oracle.bound(ref[v[0]]))
              for v in c["views"]]
    shares.append(_share("out", out[a:a + 1].cpu().numpy(), ref["out"], srgan_oracle.bound(ref["pre"])))
    print(f"sr: worst share of the oracle bound at image {a}: {max(shares):.3f}")


# ------------------------------------------------------------------------------------------------------------------- cid_cg_forward
def _cg_call(m, z, labels):
    L = _lib.lib()
    n = z.shape[0]
    need = _size(L.cid_cg_workspace_bytes, n)
    ws, out = _poisoned(need), _poisoned(4 * n * 3 * 64 * 64)
    _lib.check_abi("cg", m._cid, L.cid_cg_forward(m._cid, z.data_ptr(), labels.data_ptr(), out.data_ptr(), F32, n, 0, ws.data_ptr(), need,
                                                  _stream()))
    return out.view(torch.float32).view(n, 3, 64, 64), ws


@pytest.mark.gpu
@_frees_its_buffers
def test_cg_forward():
    """One launch per layer (N < 65,535): t3 = N x 32 x 64 x 64 alone is the subject.  The output is held to the bound of the sums
    before tanh, as in test_cgan.py."""
    from celebrity_image_denoiser_amd.cgan import load_cgan

    c = _case("cg")
    cfg = CASES["cg"]
    sd = synth.make_cgan_state_dict(cfg["wset"], cfg["n_classes"])
    m = load_cgan(sd, n_classes=cfg["n_classes"], device=DEV, strict=True)
    z = torch.randn((c["n"], 100), dtype=torch.float32, device=DEV, generator=_gen(43))
    lab = torch.randint(0, cfg["n_classes"], (c["n"],), dtype=torch.int64, device=DEV, generator=_gen(44))
    out, ws = _cg_call(m, z, lab)
    torch.cuda.synchronize()
    _same_bits("cg", c, out, ws, lambda i: _cg_call(m, z[i:i + 1], lab[i:i + 1]))
    a = c["anchor"]
    ref = cgan_oracle.forward(sd, z[a:a + 1].cpu().numpy(), [int(lab[a])])
    shares = [_share(v[0], _nchw(_stage_bits(ws, v, a, c["per"][v[0]]), v), ref[v[0]], cgan_oracle.bound(ref[v[0]]))
              for v in c["views"]]
    shares.append(_share("out", out[a:a + 1].cpu().numpy(), ref["out"], cgan_oracle.bound(ref["pre"])))
    print(f"cg: worst share of the oracle bound at image {a}: {max(shares):.3f}")


# ------------------------------------------------------------------------------------------------------------------ cid_esd_forward
def _esd_call(m, u8):
    L = _lib.lib()
    n, h, w, _ = u8.shape
    need = _size(L.cid_esd_workspace_bytes, n, h, w)
    ws, out = _poisoned(need), _poisoned(4 * n)
    _lib.check_abi("esd", m._cid, L.cid_esd_forward(m._cid, u8.data_ptr(), U8, out.data_ptr(), n, h, w, ws.data_ptr(), need, _stream()))
    return out.view(torch.float32), ws


@pytest.mark.gpu
@_frees_its_buffers
def test_esd_forward():
    import test_esrgan_disc as TED

    c = _case("esd")
    cfg = CASES["esd"]
    hw = (cfg["h"], cfg["w"])
    m = TED._module(cfg["kind"], hw)
    m.pack_weights()
    u8 = torch.randint(0, 256, (c["n"],) + hw + (3,), dtype=torch.uint8, device=DEV, generator=_gen(45))
    out, ws = _esd_call(m, u8)
    torch.cuda.synchronize()
    _same_bits("esd", c, out, ws, lambda i: _esd_call(m, u8[i:i + 1]))
    a = c["anchor"]
    x = u8[a:a + 1].cpu().permute(0, 3, 1, 2).to(torch.float32) / 255.0                  # ToTensor(): a true division
    st64, lg64 = esrgan_disc_oracle.restate(esrgan_disc_oracle.cast(esrgan_disc_oracle.weights(cfg["kind"], hw), torch.float64), x.double())
    bound = lambda t: esrgan_disc_oracle.TOL * max(1.0, float(t.abs().max()))   # noqa: E731
    shares = [_share(v[0], _nchw(_stage_bits(ws, v, a, c["per"][v[0]]), v), r.numpy(), bound(r)) for v, r in zip(c["views"], st64)]
    shares.append(_share("logit", out[a:a + 1].cpu().numpy(), lg64.numpy().reshape(-1), bound(lg64)))
    print(f"esd: worst share of the oracle bound at image {a}: {max(shares):.3f}")


# --------------------------------------------------------------------------------------------- cid_srd_forward, cid_srd_backward (eval)
def _srd_bn(m):
    """cid_disc_bn[4] on the module's own tensors (eval mode reads the running statistics and writes nothing)."""
    from celebrity_image_denoiser_amd.discriminator import _BnArg

    bn = (_BnArg * 4)()
    for i, idx in enumerate((3, 6, 9, 12)):
        b = m.model[idx]
        bn[i] = _BnArg(b.weight.data_ptr(), b.bias.data_ptr(), b.running_mean.data_ptr(), b.running_var.data_ptr(),
                       b.num_batches_tracked.data_ptr(), float(b.eps), float(b.momentum))
    return bn


def _srd_images(n, h, w, seed):
    """Distinct fp32 [n,3,h,w] in [-1,1], the normalised view of a seeded uint8 batch, and that batch."""
    u8 = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=DEV, generator=_gen(seed))
    x = torch.empty((n, 3, h, w), dtype=torch.float32, device=DEV)
    for lo in range(0, n, 4096):
        x[lo:lo + 4096] = ((u8[lo:lo + 4096].to(torch.float32) / 255.0 - 0.5) / 0.5).permute(0, 3, 1, 2)
    return u8, x


def _srd_forward(m, inp):
    L = _lib.lib()
    fmt, n, h, w = (U8,) + tuple(inp.shape[:3]) if inp.dtype == torch.uint8 else (F32, inp.shape[0], inp.shape[2], inp.shape[3])
    need = _size(L.cid_srd_workspace_bytes, n, h, w, 0)
    ws, p = _poisoned(need), _poisoned(4 * n)
    _lib.check_srd(m._cid, L.cid_srd_forward(m._cid, inp.data_ptr(), fmt, p.data_ptr(), n, h, w, _srd_bn(m), 0, ws.data_ptr(), need, _stream()))
    return p.view(torch.float32), ws


@pytest.mark.gpu
@_frees_its_buffers
def test_srd_forward_eval():
    """The forward's regions alias, so the probabilities carry the comparison: every layer feeds them.  uint8 and fp32 input."""
    import test_srgan_disc as TSD

    c = _case("srd")
    cfg = CASES["srd"]
    m = TSD._module(cfg["kind"], False)
    m.pack_weights()
    u8, x = _srd_images(c["n"], cfg["h"], cfg["w"], 46)
    p, ws = _srd_forward(m, u8)
    torch.cuda.synchronize()
    _same_bits("srd", c, p, ws, lambda i: _srd_forward(m, u8[i:i + 1]))
    ws = None
    pf, ws = _srd_forward(m, x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(pf).all())
    _same_bits("srd", c, pf, ws, lambda i: _srd_forward(m, x[i:i + 1]))
    a = c["anchor"]
    sd64 = srgan_disc_oracle.cast(srgan_disc_oracle.weights(cfg["kind"]), torch.float64)
    for name, pp, xa in (("u8", p, torch.from_numpy(synth.normalize_u8(u8[a:a + 1].cpu().numpy()))), ("f32", pf, x[a:a + 1].cpu())):
        ref = srgan_disc_oracle.restate(sd64, xa.double(), False)
        share = _share(f"p ({name} input)", pp[a:a + 1].cpu().numpy(), ref.numpy(), 1e-5)      # test_srgan_disc.py: 1e-5 absolute
        print(f"srd forward, {name}: share of the oracle bound at image {a}: {share:.3f}")


def _srd_saved_forward(m, x):
    L = _lib.lib()
    n, _, h, w = x.shape
    saved, p = _poisoned(_size(L.cid_srd_saved_bytes, n, h, w, 0)), _poisoned(4 * n)
    _lib.check_srd(m._cid, L.cid_srd_forward_saved(m._cid, x.data_ptr(), F32, p.data_ptr(), n, h, w, _srd_bn(m), 0, saved.data_ptr(),
                                                   saved.numel(), _stream()))
    return p.view(torch.float32), saved


def _srd_backward(m, x, gp, saved, want):
    """cid_srd_backward in a 0xFF-filled workspace -> ({key: gradient}, input gradient), both prefilled with NaN bits."""
    import test_srgan_disc_backward as TSDB

    L = _lib.lib()
    n, _, h, w = x.shape
    shapes = {k: v.shape for k, v in m.named_parameters()}
    grads = {k: _poisoned(4 * shapes[k].numel()).view(torch.float32).view(shapes[k]) for k in want}
    g = TSDB.Grads()
    for k, t in grads.items():
        idx, kind = int(k.split(".")[1]), k.rsplit(".", 1)[1]
        if idx in TSDB.CONV_IDX:
            (g.w if kind == "weight" else g.b)[TSDB.CONV_IDX.index(idx)] = t.data_ptr()
        else:
            (g.gamma if kind == "weight" else g.beta)[TSDB.BN_IDX.index(idx)] = t.data_ptr()
    gx = _poisoned(4 * x.numel()).view(torch.float32).view(x.shape)
    g.input = gx.data_ptr()
    ws = _poisoned(_size(L.cid_srd_backward_workspace_bytes, n, h, w, 0))
    _lib.check_srd(m._cid, L.cid_srd_backward(m._cid, x.data_ptr(), F32, gp.data_ptr(), n, h, w, _srd_bn(m), 0, saved.data_ptr(),
                                              saved.numel(), ctypes.byref(g), ws.data_ptr(), ws.numel(), _stream()))
    torch.cuda.synchronize()
    return grads, gx


@pytest.mark.gpu
@_frees_its_buffers
def test_srd_backward_eval():
    """cid_srd_forward_saved keeps a0, z2, z5, z8, z11 without overlap: a0 passes 2^31 elements and the buffer 2^34 bytes.  With a dense
    grad_prob every seam image's probability and input gradient are the bits of that image alone.  The parameter gradients sum over
    the batch: with grad_prob = d BCE(p[SEAM], 1) / dp on the seam images and zero elsewhere they are those of the small batch x[SEAM],
    held to float64 under the rule of test_srgan_disc_backward.py (e_hip <= max(1e-5, 2 e_aten), LeakyReLU masks shared under its cap)."""
    import test_srgan_disc_backward as TSDB

    c = _case("srd")
    cfg = CASES["srd"]
    n = c["n"]
    m = TSDB._module(cfg["kind"], False)
    m.pack_weights()
    seam = c["seam"]
    didx = torch.tensor(seam, device=DEV)
    _, x = _srd_images(n, cfg["h"], cfg["w"], 47)
    p, saved = _srd_saved_forward(m, x)
    dense = torch.randn(n, dtype=torch.float32, device=DEV, generator=_gen(48))
    _, gx = _srd_backward(m, x, dense, saved, ())
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(gx).all())
    for i in seam:
        p1, saved1 = _srd_saved_forward(m, x[i:i + 1])
        _, gx1 = _srd_backward(m, x[i:i + 1], dense[i:i + 1], saved1, ())
        assert torch.equal(p1.view(torch.int32), p[i:i + 1].view(torch.int32)), i
        assert torch.equal(gx1.view(torch.int32), gx[i:i + 1].view(torch.int32)), i
    gx = None

    # grad_prob zero off the seam images: the parameter gradients are those of x[SEAM]
    sparse = torch.zeros(n, dtype=torch.float32, device=DEV)
    sparse[didx] = TSDB._bce_grad(p[didx], 1.0)
    grads, gxs = _srd_backward(m, x, sparse, saved, TSDB.PARAMS)
    off = torch.ones(n, dtype=torch.bool, device=DEV)
    off[didx] = False
    assert bool((gxs[off] == 0).all())
    xs = x[didx].contiguous()
    ps, _, gx_small, masks, _ = TSDB.cabi_backward(m, xs, False, lambda q: TSDB._bce_grad(q, 1.0))
    assert torch.equal(ps.view(torch.int32), p[didx].view(torch.int32))
    assert torch.equal(gx_small.view(torch.int32), gxs[didx].view(torch.int32))
    got = {k: v.cpu() for k, v in grads.items()}
    masks = [t.cpu().bool() for t in masks]
    sd, xc = srgan_disc_oracle.weights(cfg["kind"]), xs.cpu()
    g64, gx64, ys64, p64 = TSDB.ref_backward(sd, xc, False, 1.0, torch.float64, masks)
    e_p = float((ps.cpu().double() - p64).abs().max())
    assert e_p <= TSDB.TOL
    TSDB.check_mask_cap(masks, ys64, "hip")
    e_hip = TSDB.rel_errors(got, gxs[didx].cpu(), g64, gx64, False)
    g32, gx32, ys32, _ = TSDB.ref_backward(sd, xc, False, 1.0, torch.float32)
    masks32 = [y > 0 for y in ys32]
    TSDB.check_mask_cap(masks32, ys64, "aten")
    g64a, gx64a, _, _ = TSDB.ref_backward(sd, xc, False, 1.0, torch.float64, masks32)
    e_aten = TSDB.rel_errors(g32, gx32, g64a, gx64a, False)
    print(f"srd backward: max|p - p64| on SEAM {e_p:.2e} (share {e_p / TSDB.TOL:.3f});   e_hip      e_aten(fp32, CPU)")
    for k in TSDB.PARAMS + ["input"]:
        print(f"    {k:16s} {e_hip[k]:.2e}   {e_aten[k]:.2e}")
    print("srd backward: worst share of the bound max(1e-5, 2 e_aten): "
          f"{max(e_hip[k] / max(TSDB.TOL, 2 * e_aten[k]) for k in e_hip):.3f}")
    for k in TSDB.PARAMS + ["input"]:
        assert bool(torch.isfinite(got[k] if k != "input" else gxs).all()), k
        assert e_hip[k] <= max(TSDB.TOL, 2 * e_aten[k]), (k, e_hip[k], e_aten[k])
