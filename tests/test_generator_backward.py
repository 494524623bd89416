"""The backward pass of the denoising generator: cid_saved_bytes / cid_forward_saved / cid_backward_workspace_bytes / cid_backward
(include/cid.h) and DenoiseGenerator(autograd=True).

The reference for error is the stock structure (training.py:59-74) written with torch.nn.functional in float64 on the CPU, through torch
autograd; the same in float32 stands for "ATen fp32".  ReLU's derivative and max-pool's routing are discontinuous, so each fp32 run
(ours, ATen's) is compared with a float64 run whose ReLU backward takes that fp32 run's nine masks and whose pool backward takes that
fp32 run's two argmax maps; the forward of the float64 run is untouched.  For the device run both are derived from the saved buffer
through cid_stage_view: mask = stored activation > 0, argmax = the first element in window scan order (0,0), (0,1), (1,0), (1,1) whose
stored value equals the stored pooled value.

That sharing is capped (a condition, not a measurement): a mask may differ from y64 > 0 only where |y64| <= 1e-5 * max|y64|; an
argmax may differ from float64's only where the two candidates differ by <= 1e-5 * max|e64|; each at no more than ceil(1e-5 * units)
units per layer (MASK_CAP).

Error of a tensor: e(T) = max|g - g64| / max|g64|.  Bound: e_hip(T) <= max(1e-5, 2 * e_aten(T)), e_aten measured in the same test on
the same case: 1e-5 is the project's TOL; one tensor's fp32 error is a single draw of a rounding walk, so ATen's own error for the
same tensor is allowed twice."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from celebrity_image_denoiser_amd import _lib, synth

DEV = "cuda:0"
TOL = 1e-5
MASK_CAP = 1e-5
ERR_INVALID, ERR_SHAPE, ERR_STATE, ERR_WORKSPACE = 1, 2, 4, 5
LAYERS = ("down1.0", "down1.2", "down2.0", "down2.2", "bottleneck.0", "bottleneck.2", "up2", "upconv2.0", "upconv2.2", "up1",
          "upconv1.0", "upconv1.2")
PARAMS = [f"{l}.{k}" for l in LAYERS for k in ("weight", "bias")]   # nn.Module.parameters() order = cid_param_key order
DECODER = [k for k in PARAMS if k.split(".")[0] in ("up2", "upconv2", "up1", "upconv1")]
# the nine ReLUs in forward order, by the cid_stage_view stage that holds each one's output
RELU_STAGES = ("down1.0", "down1", "down2.0", "down2", "bottleneck.0", "bottleneck", "upconv2.0", "upconv2", "upconv1.0")
WSETS = ("default", "hot")


# ------------------------------------------------------------------------------------------------------------- float64 / fp32 reference
class _MaskedRelu(torch.autograd.Function):
    """Stock ReLU forward; backward g * mask with a given mask."""

    @staticmethod
    def forward(ctx, y, mask):
        ctx.save_for_backward(mask)
        return F.relu(y)

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return g * mask.to(g.dtype), None


def _own_argmax(e):
    """Window-local argmax (0..3 in scan order) of max_pool2d(e, 2) as ATen routes it."""
    _, idx = F.max_pool2d(e, 2, return_indices=True)
    w = e.shape[3]
    return ((idx // w) % 2) * 2 + (idx % w) % 2


class _RoutedPool(torch.autograd.Function):
    """Stock max_pool2d(2) forward; backward sends g to the window element `arg` (0..3 in scan order) of each window."""

    @staticmethod
    def forward(ctx, e, arg):
        ctx.save_for_backward(arg)
        return F.max_pool2d(e, 2)

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        n, c, hp, wp = g.shape
        ge = torch.zeros(n, c, 2 * hp, 2 * wp, dtype=g.dtype)
        for k in range(4):
            ge[:, :, k // 2::2, k % 2::2] = g * (arg == k).to(g.dtype)
        return ge, None


def ref_backward(sd, x, dtype, upstream, masks=None, argmax=None):
    """Gradients in `dtype` on the CPU.  upstream: ("mse", clean) for MSE(G(x), clean), or ("grad", grad_out).  masks: nine bool
    tensors for ReLU's backward / argmax: two window-local index maps for the pools' backward, or None for the run's own.
    -> (param grads by key, input grad, the nine ReLU pre-activations, the two pool inputs, the run's own argmax maps, y)"""
    P = {k: torch.as_tensor(sd[k]).to(dtype).clone().requires_grad_(True) for k in PARAMS}
    xx = torch.as_tensor(x).to(dtype).clone().requires_grad_(True)
    pre, pin, own = [], [], []

    def conv(t, name):
        return F.conv2d(t, P[name + ".weight"], P[name + ".bias"], padding=1)

    def relu(y):
        i = len(pre)
        pre.append(y.detach())
        return _MaskedRelu.apply(y, masks[i] if masks is not None else y.detach() > 0)

    def pool(e):
        i = len(pin)
        pin.append(e.detach())
        own.append(_own_argmax(e.detach()))
        return _RoutedPool.apply(e, argmax[i] if argmax is not None else own[i])

    def convt(t, name):
        return F.conv_transpose2d(t, P[name + ".weight"], P[name + ".bias"], stride=2)

    e1 = relu(conv(relu(conv(xx, "down1.0")), "down1.2"))
    e2 = relu(conv(relu(conv(pool(e1), "down2.0")), "down2.2"))
    b = relu(conv(relu(conv(pool(e2), "bottleneck.0")), "bottleneck.2"))
    d2 = relu(conv(relu(conv(torch.cat([convt(b, "up2"), e2], 1), "upconv2.0")), "upconv2.2"))
    t4 = relu(conv(torch.cat([convt(d2, "up1"), e1], 1), "upconv1.0"))
    y = torch.tanh(conv(t4, "upconv1.2"))
    if upstream[0] == "mse":
        F.mse_loss(y, torch.as_tensor(upstream[1]).to(dtype)).backward()
    else:
        y.backward(torch.as_tensor(upstream[1]).to(dtype))
    return {k: P[k].grad for k in PARAMS}, xx.grad, pre, pin, own, y.detach()


def rel_errors(got, got_x, ref, ref_x):
    out = {k: float((got[k].double() - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in PARAMS}
    out["input"] = float((got_x.double() - ref_x).abs().max()) / float(ref_x.abs().max())
    return out


def check_caps(masks, argmax, pre64, pin64, own64, who):
    """The sharing conditions of the module docstring; prints what differs."""
    for i, (m, y) in enumerate(zip(masks, pre64)):
        flips = m != (y > 0)
        nf = int(flips.sum())
        if nf:
            worst = float(y[flips].abs().max()) / float(y.abs().max())
            print(f"    {who} ReLU mask {i}: {nf} of {y.numel()} units differ from y64 > 0, all at |y64| <= {worst:.1e} * max|y64|")
            assert worst <= MASK_CAP, (who, i, worst)
        assert nf <= math.ceil(MASK_CAP * y.numel()), (who, "relu", i, nf)
    for i, (a, e, a64) in enumerate(zip(argmax, pin64, own64)):
        diff = a != a64
        nd = int(diff.sum())
        if nd:
            win = torch.stack([e[:, :, k // 2::2, k % 2::2] for k in range(4)], -1)
            gap = (win.gather(-1, a64.unsqueeze(-1)) - win.gather(-1, a.long().unsqueeze(-1))).squeeze(-1).abs()
            worst = float(gap[diff].max()) / float(e.abs().max())
            print(f"    {who} pool {i}: {nd} of {a.numel()} windows route elsewhere than float64, candidates within {worst:.1e} * max|e64|")
            assert worst <= MASK_CAP, (who, i, worst)
        assert nd <= math.ceil(MASK_CAP * a.numel()), (who, "pool", i, nd)


# ------------------------------------------------------------------------------------------------------------- the C ABI, directly
class _Grads(ctypes.Structure):
    _fields_ = [("w", ctypes.c_void_p * 12), ("b", ctypes.c_void_p * 12), ("input", ctypes.c_void_p)]


def _module(kind, autograd=False, conv_algo=None):
    from celebrity_image_denoiser_amd.generator import DenoiseGenerator

    m = DenoiseGenerator(autograd=autograd)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_state_dict(kind).items()}, strict=True)
    m.to(DEV)
    if conv_algo is not None:
        m.conv_algo = conv_algo
    return m


def _sizes(n, h, w):
    L = _lib.lib()
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.cid_saved_bytes(n, h, w, ctypes.byref(a)) == 0 and L.cid_backward_workspace_bytes(n, h, w, ctypes.byref(b)) == 0
    return a.value, b.value


def forward_saved(m, x):
    """cid_forward_saved at m's weights -> (y, saved buffer)"""
    L = _lib.lib()
    m.pack_weights()
    n, _, h, w = x.shape
    saved = torch.empty(_sizes(n, h, w)[0], dtype=torch.uint8, device=DEV)
    y = torch.empty((n, 3, h, w), dtype=torch.float32, device=DEV)
    _lib.check(m._cid, L.cid_forward_saved(m._cid, x.data_ptr(), y.data_ptr(), n, h, w, saved.data_ptr(), saved.numel(),
                                           torch.cuda.current_stream().cuda_stream))
    return y, saved


def stage(buf, name, n, h, w):
    """Stage `name` (cid_stage_view) of an arena-layout buffer as an fp32 NCHW tensor."""
    off, c, hs, ws, ps, coff = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert _lib.lib().cid_stage_view(name.encode(), n, h, w, ctypes.byref(off), ctypes.byref(c), ctypes.byref(hs), ctypes.byref(ws),
                                     ctypes.byref(ps), ctypes.byref(coff)) == 0
    flat = buf[off.value:off.value + 4 * n * hs.value * ws.value * ps.value].view(torch.float32)
    return flat.view(n, hs.value, ws.value, ps.value)[..., coff.value:coff.value + c.value].permute(0, 3, 1, 2).contiguous()


def saved_masks_and_argmax(saved, n, h, w, idx=None):
    """The nine ReLU masks and the two pool routings as cid_backward decides them, from the saved buffer (CPU tensors); of the
    images `idx` (a device index tensor) only, if given."""
    pick = (lambda t: t) if idx is None else (lambda t: t[idx])
    masks = [(pick(stage(saved, s, n, h, w)) > 0).cpu() for s in RELU_STAGES]
    argmax = []
    for e_name, p_name in (("down1", "pool1"), ("down2", "pool2")):
        e, p = pick(stage(saved, e_name, n, h, w)), pick(stage(saved, p_name, n, h, w))
        a = torch.full(p.shape, 3, dtype=torch.int64, device=e.device)
        for k in (2, 1, 0):   # the FIRST equal element in scan order wins
            a = torch.where(e[:, :, k // 2::2, k % 2::2] == p, torch.full_like(a, k), a)
        argmax.append(a.cpu())
    return masks, argmax


def cabi_backward(m, x, grad_fn, want=PARAMS, want_input=True, saved=None, y=None):
    """cid_forward_saved (unless given) + cid_backward at m's weights on the device batch x.  grad_fn(y) -> grad_out.
    -> (y, {key: grad}, grad_x or None, saved, grad_out); buffers not asked for keep their NaN prefill and are returned in `rest`."""
    L = _lib.lib()
    n, _, h, w = x.shape
    x = x.contiguous()
    if saved is None:
        y, saved = forward_saved(m, x)
    go = grad_fn(y).to(torch.float32).contiguous()
    shapes = {k: tuple(p.shape) for k, p in m.named_parameters()}
    grads = {k: torch.full(shapes[k], float("nan"), dtype=torch.float32, device=DEV) for k in want}
    g = _Grads()
    for k, t in grads.items():
        layer, kind = k.rsplit(".", 1)
        (g.w if kind == "weight" else g.b)[LAYERS.index(layer)] = t.data_ptr()
    gx = None
    if want_input:
        gx = torch.full((n, 3, h, w), float("nan"), dtype=torch.float32, device=DEV)
        g.input = gx.data_ptr()
    ws = torch.empty(_sizes(n, h, w)[1], dtype=torch.uint8, device=DEV)
    _lib.check(m._cid, L.cid_backward(m._cid, x.data_ptr(), y.data_ptr(), go.data_ptr(), n, h, w, saved.data_ptr(), saved.numel(),
                                      ctypes.byref(g), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return y, grads, gx, saved, go


def _mse_grad(y, clean):
    """d MSE(y, clean) / dy as torch computes it on the device."""
    leaf = y.detach().clone().requires_grad_(True)
    F.mse_loss(leaf, clean).backward()
    return leaf.grad


# ------------------------------------------------------------------------------------------------------------------ CPU tests
def test_saved_bytes_equals_workspace_bytes():
    L = _lib.lib()
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    for shape in ((1, 4, 4), (3, 12, 8), (16, 256, 256), (64, 128, 128), (2, 30, 45)):
        assert L.cid_saved_bytes(*shape, ctypes.byref(a)) == 0 and L.cid_workspace_bytes(*shape, ctypes.byref(b)) == 0
        assert a.value == b.value > 0
    assert L.cid_saved_bytes(2, 8, 8, None) == ERR_INVALID
    assert L.cid_saved_bytes(0, 8, 8, ctypes.byref(a)) == ERR_SHAPE and L.cid_saved_bytes(1, 3, 8, ctypes.byref(a)) == ERR_SHAPE
    assert L.cid_backward_workspace_bytes(2, 8, 8, None) == ERR_INVALID
    assert L.cid_backward_workspace_bytes(2, 30, 45, ctypes.byref(a)) == ERR_SHAPE
    assert L.cid_backward_workspace_bytes(0, 8, 8, ctypes.byref(a)) == ERR_SHAPE
    # the workspace holds at least the gradients of the two concat tensors
    assert L.cid_backward_workspace_bytes(3, 12, 8, ctypes.byref(a)) == 0 and a.value >= 3 * 12 * 8 * 128 * 4 + 3 * 6 * 4 * 256 * 4


def test_argument_errors_come_before_any_launch():
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.cid_create(ctypes.byref(h)) == 0
    try:
        fake = 1 << 20          # 256-byte aligned, never dereferenced: every call below must fail on the host
        ok_g = _Grads()
        ok_g.w[0] = fake
        ok_g.input = fake
        need_s, need_w = _sizes(3, 12, 8)

        def fwd(hh=h, x=fake, out=fake, n=3, hh_=12, w=8, sv=fake, sv_bytes=1 << 40):
            return L.cid_forward_saved(hh, x, out, n, hh_, w, sv, sv_bytes, None)

        def bwd(hh=h, x=fake, y=fake, go=fake, n=3, hh_=12, w=8, sv=fake, sv_bytes=1 << 40, g=ok_g, ws=fake, ws_bytes=1 << 40):
            return L.cid_backward(hh, x, y, go, n, hh_, w, sv, sv_bytes, ctypes.byref(g) if g is not None else None, ws, ws_bytes, None)

        assert fwd(hh=None) == ERR_INVALID and bwd(hh=None) == ERR_INVALID
        for kw in (dict(x=None), dict(out=None), dict(sv=None)):
            assert fwd(**kw) == ERR_INVALID, kw
        bad_g = _Grads()
        bad_g.b[7] = fake + 2
        for kw in (dict(x=None), dict(y=None), dict(go=None), dict(sv=None), dict(g=None), dict(ws=None), dict(x=fake + 1),
                   dict(go=fake + 2), dict(g=bad_g)):
            assert bwd(**kw) == ERR_INVALID, kw
        # H or W not a multiple of 4: the differentiable forward refuses what the plain forward accepts, and says why
        size = ctypes.c_size_t()
        for n, hh_, w in ((2, 30, 45), (2, 32, 45), (2, 30, 44), (1, 6, 8)):
            assert L.cid_workspace_bytes(n, hh_, w, ctypes.byref(size)) == 0
            assert fwd(n=n, hh_=hh_, w=w) == ERR_SHAPE
            assert b"multiples of 4" in L.cid_last_error(h)
            assert bwd(n=n, hh_=hh_, w=w) == ERR_SHAPE
            assert b"multiples of 4" in L.cid_last_error(h)
        for n, hh_, w in ((0, 8, 8), (2, 0, 8), (2, 8, 3)):
            assert fwd(n=n, hh_=hh_, w=w) == ERR_SHAPE and bwd(n=n, hh_=hh_, w=w) == ERR_SHAPE
        # short or misaligned buffers
        assert fwd(sv_bytes=need_s - 1) == ERR_WORKSPACE and fwd(sv=fake + 16, sv_bytes=need_s) == ERR_WORKSPACE
        assert bwd(sv_bytes=need_s - 1) == ERR_WORKSPACE and bwd(sv=fake + 16, sv_bytes=need_s) == ERR_WORKSPACE
        assert bwd(sv_bytes=need_s, ws_bytes=need_w - 1) == ERR_WORKSPACE and bwd(sv_bytes=need_s, ws=fake + 16, ws_bytes=need_w) == ERR_WORKSPACE
        # no weights attached: still before any launch
        assert fwd(sv_bytes=need_s) == ERR_STATE and bwd(sv_bytes=need_s, ws_bytes=need_w) == ERR_STATE
        assert b"weights" in L.cid_last_error(h)
        # fp16 storage has no backward
        assert L.cid_set_compute_dtype(h, _lib.CID_DTYPE_F16) == 0
        assert fwd(sv_bytes=need_s) == ERR_STATE and b"CID_DTYPE_F32" in L.cid_last_error(h)
        assert bwd(sv_bytes=need_s, ws_bytes=need_w) == ERR_STATE and b"CID_DTYPE_F32" in L.cid_last_error(h)
        tail = ctypes.c_int(-1)
        assert L.cid_get_tail_algo(h, ctypes.byref(tail)) == 0 and tail.value == _lib.CID_TAIL_FUSED
    finally:
        L.cid_destroy(h)


def test_autograd_flag_defaults_off_and_keeps_the_structure():
    from celebrity_image_denoiser_amd import load
    from celebrity_image_denoiser_amd.generator import DenoiseGenerator

    plain, auto = DenoiseGenerator(), DenoiseGenerator(autograd=True)
    assert plain._autograd is False and auto._autograd is True
    assert [k for k, _ in auto.named_parameters()] == PARAMS
    assert list(auto.state_dict()) == list(plain.state_dict()) == PARAMS
    assert inspect.signature(load).parameters["autograd"].default is False
    assert inspect.signature(DenoiseGenerator.__init__).parameters["autograd"].default is False
    assert [_lib.lib().cid_param_key(i).decode() for i in range(24)] == PARAMS


# ------------------------------------------------------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("algo", ("winograd42", "direct"))
def test_forward_saved_is_bit_identical_to_the_unfused_forward(algo):
    x = torch.from_numpy(synth.make_batch(3, 40, 56, first_index=11)[0]).to(DEV)
    n, _, h, w = x.shape
    for kind in WSETS:
        m = _module(kind, conv_algo=algo)
        before = m(x).clone()                     # the handle's own configuration (fused tail under winograd42)
        tail_before = m.tail_algo
        y, saved = forward_saved(m, x)
        assert m.tail_algo == tail_before == "fused"
        after = m(x)
        assert torch.equal(before, after)
        ref = _module(kind, conv_algo=algo)
        ref.tail_algo = "tiles"
        yr = ref(x)
        assert torch.equal(y, yr)
        for s in RELU_STAGES + ("pool1", "pool2", "up2", "up1"):
            assert torch.equal(stage(saved, s, n, h, w), ref.stage_output(s, n, h, w)), (kind, s)


PARITY_SHAPES = ((1, 4, 4), (3, 12, 8), (2, 20, 24), (16, 64, 64), (4, 128, 128), (2, 256, 256))
_ATEN = {}   # (kind, shape, upstream kind) -> ATen fp32's errors: they do not depend on the device run


def _parity(kind, algo, shape, random_upstream=False, m=None, x=None, clean=None, grad_out=None):
    """Gradient parity of one case -> (e_hip, e_aten); asserts the caps and the bound."""
    n, h, w = shape
    if x is None:
        xn, cn, _ = synth.make_batch(n, h, w, first_index=sum(shape))
        x, clean = torch.from_numpy(xn), torch.from_numpy(cn)
    sd = synth.make_state_dict(kind) if m is None else {k: v.detach().cpu() for k, v in m.state_dict().items()}
    m = m if m is not None else _module(kind, conv_algo=algo)
    if random_upstream:
        grad_out = torch.randn(x.shape, generator=torch.Generator().manual_seed(1234))
    if grad_out is not None:
        grad_fn, up = (lambda y: grad_out.to(DEV)), ("grad", grad_out)
    else:
        cd = clean.to(DEV)
        grad_fn, up = (lambda y: _mse_grad(y, cd)), ("mse", clean)
    y, grads, gx, saved, _ = cabi_backward(m, x.to(DEV), grad_fn)
    got = {k: v.cpu() for k, v in grads.items()}
    masks, argmax = saved_masks_and_argmax(saved, n, h, w)
    del saved
    g64, gx64, pre64, pin64, own64, y64 = ref_backward(sd, x, torch.float64, up, masks, argmax)
    assert float((y.cpu().double() - y64).abs().max()) <= TOL
    check_caps(masks, argmax, pre64, pin64, own64, "hip")
    e_hip = rel_errors(got, gx.cpu(), g64, gx64)
    key = (kind, shape, "rand" if random_upstream else "mse") if grad_out is None or random_upstream else None
    if key is None or key not in _ATEN:
        g32, gx32, pre32, _, own32, _ = ref_backward(sd, x, torch.float32, up)
        masks32 = [t > 0 for t in pre32]
        check_caps(masks32, own32, pre64, pin64, own64, "aten")
        g64a, gx64a, _, _, _, _ = ref_backward(sd, x, torch.float64, up, masks32, own32)
        e_aten = rel_errors(g32, gx32, g64a, gx64a)
        if key is not None:
            _ATEN[key] = e_aten
    else:
        e_aten = _ATEN[key]
    print(f"\ngenerator gradient parity {kind} {algo} {'x'.join(map(str, shape))} {'random grad_out' if random_upstream else up[0]}:"
          "   e_hip      e_aten(fp32, CPU)")
    for k in PARAMS + ["input"]:
        flag = "" if e_hip[k] <= TOL else ("  (2*e_aten branch)" if e_hip[k] <= 2 * e_aten[k] else "  FAIL")
        print(f"    {k:20s} {e_hip[k]:.2e}   {e_aten[k]:.2e}{flag}")
    for k in PARAMS:
        assert bool(torch.isfinite(got[k]).all()), k
    assert bool(torch.isfinite(gx).all())
    for k in PARAMS + ["input"]:
        assert e_hip[k] <= max(TOL, 2 * e_aten[k]), (k, e_hip[k], e_aten[k])
    return e_hip, e_aten


@pytest.mark.gpu
@pytest.mark.parametrize("kind", WSETS)
@pytest.mark.parametrize("shape", PARITY_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("algo", ("winograd42", "direct"))
def test_gradient_parity(kind, shape, algo):
    """MSE(G(x), clean): all 24 parameter gradients and the input gradient."""
    _parity(kind, algo, shape)


@pytest.mark.gpu
def test_gradient_parity_random_upstream():
    _parity("default", "winograd42", (3, 24, 20), random_upstream=True)


@pytest.mark.gpu
def test_backward_is_deterministic():
    xn, cn, _ = synth.make_batch(5, 36, 44, first_index=900)
    x, clean = torch.from_numpy(xn).to(DEV), torch.from_numpy(cn).to(DEV)
    m = _module("hot")
    runs = [cabi_backward(m, x, lambda y: _mse_grad(y, clean)) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2])
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in PARAMS)


@pytest.mark.gpu
def test_subsets_give_the_same_bits_and_leave_the_rest_untouched():
    xn, cn, _ = synth.make_batch(3, 28, 36, first_index=33)
    x, clean = torch.from_numpy(xn).to(DEV), torch.from_numpy(cn).to(DEV)
    m = _module("default")
    gfn = lambda y: _mse_grad(y, clean)   # noqa: E731
    y, full, gx_full, saved, _ = cabi_backward(m, x, gfn)
    assert all(bool(torch.isfinite(v).all()) for v in full.values()) and bool(torch.isfinite(gx_full).all())
    L = _lib.lib()
    n, _, h, w = x.shape
    for want, want_input in (((), True), (("down1.0.weight",), False), (tuple(DECODER), False)):
        # every buffer is passed around NaN-prefilled; only the ones asked for are handed to cid_backward
        bufs = {k: torch.full_like(full[k], float("nan")) for k in PARAMS}
        gx = torch.full_like(gx_full, float("nan"))
        g = _Grads()
        for k in want:
            layer, kind = k.rsplit(".", 1)
            (g.w if kind == "weight" else g.b)[LAYERS.index(layer)] = bufs[k].data_ptr()
        if want_input:
            g.input = gx.data_ptr()
        go = gfn(y).contiguous()
        ws = torch.empty(_sizes(n, h, w)[1], dtype=torch.uint8, device=DEV)
        _lib.check(m._cid, L.cid_backward(m._cid, x.data_ptr(), y.data_ptr(), go.data_ptr(), n, h, w, saved.data_ptr(), saved.numel(),
                                          ctypes.byref(g), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        for k in PARAMS:
            if k in want:
                assert torch.equal(bufs[k], full[k]), (want, k)
            else:
                assert bool(torch.isnan(bufs[k]).all()), (want, k)
        assert torch.equal(gx, gx_full) if want_input else bool(torch.isnan(gx).all())


@pytest.mark.gpu
def test_module_autograd():
    xn, cn, _ = synth.make_batch(4, 32, 24, first_index=7)
    x, clean = torch.from_numpy(xn).to(DEV), torch.from_numpy(cn).to(DEV)
    plain, auto = _module("default"), _module("default", autograd=True)
    # autograd=False: today's module
    yp = plain(x)
    assert yp.grad_fn is None and yp.requires_grad is False
    # autograd=True: loss.backward() fills .grad with cid_backward's bits
    _, want, want_x, _, _ = cabi_backward(plain, x, lambda y: _mse_grad(y, clean))
    xr = x.clone().requires_grad_(True)
    ya = auto(xr)
    assert ya.grad_fn is not None and ya.requires_grad
    assert auto.tail_algo == "fused"
    F.mse_loss(ya, clean).backward()
    for k, p in auto.named_parameters():
        assert p.grad is not None and torch.equal(p.grad, want[k]), k
    assert torch.equal(xr.grad, want_x)
    # a second backward accumulates
    F.mse_loss(auto(x), clean).backward()
    for k, p in auto.named_parameters():
        assert torch.equal(p.grad, want[k] + want[k]), k
    # under no_grad, and when nothing requires grad, the default path: fused tail included, bit for bit
    with torch.no_grad():
        yn = auto(x)
    assert yn.grad_fn is None and torch.equal(yn, yp)
    for p in auto.parameters():
        p.requires_grad_(False)
    yf = auto(x)
    assert yf.grad_fn is None and torch.equal(yf, yp)
    # only the input requires grad
    xr2 = x.clone().requires_grad_(True)
    F.mse_loss(auto(xr2), clean).backward()
    assert torch.equal(xr2.grad, want_x)
    for p in auto.parameters():
        p.requires_grad_(True)
    # an in-place parameter change between forward and backward raises
    loss = F.mse_loss(auto(x), clean)
    with torch.no_grad():
        auto.down2[0].weight.mul_(0.5)
    with pytest.raises(RuntimeError, match="modified in place"):
        loss.backward()
    # sizes that are not multiples of 4: a clear error with grad, today's forward without
    odd = torch.from_numpy(synth.make_batch(2, 30, 45, first_index=3)[0]).to(DEV)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        auto(odd)
    with torch.no_grad():
        yo = auto(odd)
    assert tuple(yo.shape) == (2, 3, 28, 44) and torch.equal(yo, _remake(auto)(odd))
    # fp16 storage has no backward
    auto.compute_dtype = "f16"
    with pytest.raises(RuntimeError, match="f32"):
        auto(x)
    with torch.no_grad():
        assert auto(x).grad_fn is None


def _remake(m):
    """A plain module at m's current weights."""
    from celebrity_image_denoiser_amd.generator import DenoiseGenerator

    r = DenoiseGenerator()
    r.load_state_dict(m.state_dict(), strict=True)
    return r.to(DEV)


class StockGenerator(nn.Module):
    """The reference's structure (training.py:59-74 / app.py:39-103) with stock layers."""

    def __init__(self):
        super().__init__()
        blk = lambda a, b, c, last=True: nn.Sequential(*([nn.Conv2d(a, b, 3, padding=1), nn.ReLU(), nn.Conv2d(b, c, 3, padding=1)]  # noqa: E731
                                                         + ([nn.ReLU()] if last else [])))
        self.down1, self.pool1 = blk(3, 64, 64), nn.MaxPool2d(2, 2)
        self.down2, self.pool2 = blk(64, 128, 128), nn.MaxPool2d(2, 2)
        self.bottleneck = blk(128, 256, 256)
        self.up2, self.upconv2 = nn.ConvTranspose2d(256, 128, 2, stride=2), blk(256, 128, 128)
        self.up1, self.upconv1 = nn.ConvTranspose2d(128, 64, 2, stride=2), blk(128, 64, 3, last=False)

    def forward(self, x):
        e1 = self.down1(x)
        e2 = self.down2(self.pool1(e1))
        b = self.bottleneck(self.pool2(e2))
        d2 = self.upconv2(torch.cat([self.up2(b), e2], 1))
        return torch.tanh(self.upconv1(torch.cat([self.up1(d2), e1], 1)))


def _trainer_loop(G, D, noisy, clean, steps, on_step=None):
    """training.py:410-426 on one fixed batch -> [(d_loss, g_loss, content_loss, adv_loss)] per step."""
    g_optimizer = torch.optim.Adam(G.parameters(), lr=1e-4)
    d_optimizer = torch.optim.Adam(D.parameters(), lr=1e-4)
    bce_loss, mse_loss = nn.BCELoss(), nn.MSELoss()
    out = []
    for step in range(steps):
        d_optimizer.zero_grad()
        denoised_img = G(noisy)
        real_pred = D(clean)
        fake_pred = D(denoised_img.detach())
        d_loss = bce_loss(real_pred, torch.ones_like(real_pred)) + bce_loss(fake_pred, torch.zeros_like(fake_pred))
        d_loss.backward()
        d_optimizer.step()

        g_optimizer.zero_grad()
        d_in = denoised_img.view_as(denoised_img)      # an alias, so that D's input gradient can be observed on its own
        seen = {}
        if on_step is not None and step == 0:
            d_in.register_hook(lambda t: seen.__setitem__("d_in", t.detach().clone()))
        fake_pred = D(d_in)
        content_loss = mse_loss(denoised_img, clean)
        adv_loss = bce_loss(fake_pred, torch.ones_like(fake_pred))
        g_loss = content_loss + 0.001 * adv_loss
        g_loss.backward()
        if on_step is not None and step == 0:
            on_step(denoised_img.detach(), seen["d_in"])
        g_optimizer.step()
        out.append(tuple(float(v.detach()) for v in (d_loss, g_loss, content_loss, adv_loss)))
    return out


@pytest.mark.gpu
def test_the_trainers_whole_step_on_both_modules():
    """training.py:410-426 with DenoiseGenerator(autograd=True) and DenoiseDiscriminator(autograd=True), two Adam(lr=1e-4), B = 4, 64 x 64."""
    from celebrity_image_denoiser_amd.discriminator import DenoiseDiscriminator
    from test_discriminator import StockDiscriminator
    from test_discriminator import weights as disc_weights

    B, S = 4, 64
    xn, cn, _ = synth.make_batch(B, S, S, first_index=321)
    noisy, clean = torch.from_numpy(xn), torch.from_numpy(cn)
    G = _module("default", autograd=True).train()
    D = DenoiseDiscriminator(autograd=True)
    D.load_state_dict(disc_weights("trained"), strict=True)
    D.to(DEV).train()
    nd, cd = noisy.to(DEV), clean.to(DEV)
    checked = {}

    def on_step(y, d_in_grad):
        # the generator gradients of step 1 are cid_backward's for grad_out = 2 (y - clean) / numel + 0.001 * d adv / d y, bit for bit
        mse_grad = _mse_grad(y, cd)
        formula = 2.0 * (y.double() - cd.double()) / y.numel()
        assert float((mse_grad.double() - formula).abs().max()) <= 4 * 2.0 ** -24 * float(formula.abs().max())
        grad_out = mse_grad + d_in_grad
        plain = _remake(G)
        _, want, _, _, _ = cabi_backward(plain, nd, lambda _y: grad_out, want_input=False)
        for k, p in G.named_parameters():
            assert p.grad is not None and torch.equal(p.grad, want[k]), k
        # ... and pass the parity bound with that grad_out
        _parity("default", "winograd42", (B, S, S), m=plain, x=noisy, grad_out=grad_out.cpu())
        checked["ok"] = True

    hip = _trainer_loop(G, D, nd, cd, 10, on_step)
    assert checked.get("ok")
    # the same loop with stock ATen modules on the CPU from the same initialisation: printed, not a gate
    Gc, Dc = StockGenerator(), StockDiscriminator()
    Gc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_state_dict("default").items()}, strict=True)
    Dc.load_state_dict(disc_weights("trained"), strict=True)
    cpu = _trainer_loop(Gc.train(), Dc.train(), noisy, clean, 10)
    print("\ntrainer step trajectory (B=4, 64x64, one fixed batch):  HIP d_loss g_loss content adv | ATen CPU d_loss g_loss content adv")
    for i, (a, b) in enumerate(zip(hip, cpu)):
        print(f"    step {i + 1:2d}: " + " ".join(f"{v:.6f}" for v in a) + " | " + " ".join(f"{v:.6f}" for v in b))
    assert all(math.isfinite(v) for row in hip for v in row)
    assert hip[-1][2] < hip[0][2], (hip[0][2], hip[-1][2])
