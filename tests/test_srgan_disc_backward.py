"""The backward pass of the SRGAN trainer's discriminator on the GPU: cid_srd_forward_saved / cid_srd_backward /
cid_srd_pack_weights_device / cid_srd_saved_masks (include/cid.h) and SRGANDiscriminator(autograd=True).

The rule of error is that of tests/test_discriminator_backward.py, taken over whole.  The reference is the stock structure in float64
on the CPU through torch autograd; the same in float32 stands for "ATen fp32".  LeakyReLU's derivative is discontinuous, so each fp32
run (ours, ATen's) is compared with a float64 run that takes LeakyReLU's backward masks from that fp32 run (six masks here: a0, the four
BatchNorm outputs, the hidden layer); the forward of the float64 run is untouched.  That sharing is capped: a device mask may differ
from `y64 > 0` only where |y64| <= 1e-5 * max|y64| of that tensor, at no more than ceil(1e-5 * units) units per layer.

Error of a tensor: e(T) = max|g - g64| / max|g64|; for model.2/5/8/11.bias in train mode, whose true value is 0 (BatchNorm removes the
mean), the denominator is max|g64| of the same layer's weight gradient.  Bound: e_hip(T) <= max(1e-5, 2 * e_aten(T)), e_aten measured
in the same test; probabilities within 1e-5 of float64.

Shapes: those of tests/test_srgan_disc.py, for its reasons ((3,41,70): quarter resolution 11 x 18 crosses model.11's 16-pixel tile
width and both of its gradients' tile heights), and (2,8,8) in train mode."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import celebrity_image_denoiser_amd as cid
from celebrity_image_denoiser_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import srgan_disc_oracle as oracle  # noqa: E402
from srgan_disc_oracle import BNS, cast, images, images_u8, restate, weights  # noqa: E402
from test_srgan_disc_backward_host import PARAMS, Grads  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
MASK_CAP = 1e-5
WSETS = oracle.WSETS
CONV_IDX = (0, 2, 5, 8, 11, 15, 17)
BN_IDX = (3, 6, 9, 12)
BN_BIASES = ("model.2.bias", "model.5.bias", "model.8.bias", "model.11.bias")   # true gradient 0 in train mode


# ------------------------------------------------------------------------------------------------------------- float64 / fp32 reference
class _MaskedLeaky(torch.autograd.Function):
    """Stock LeakyReLU(0.2) forward; backward g * where(mask, 1, 0.2) with a given mask."""

    @staticmethod
    def forward(ctx, y, mask):
        ctx.save_for_backward(mask)
        return F.leaky_relu(y, 0.2)

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return g * torch.where(mask, 1.0, 0.2).to(g.dtype), None


def ref_backward(sd, x, training, target, dtype, masks=None):
    """Gradients of BCE(D(x), target) in `dtype` on the CPU.  masks: six bool tensors for LeakyReLU's backward, or None for the run's
    own (y > 0).  -> (param grads by state_dict key, input grad, the six pre-activations y, probabilities)"""
    P = {k: sd[k].to(dtype).clone().requires_grad_(True) for k in PARAMS}
    xx = x.to(dtype).clone().requires_grad_(True)
    ys = []

    def act(y):
        i = len(ys)
        ys.append(y.detach())
        return _MaskedLeaky.apply(y, masks[i].reshape(y.shape) if masks is not None else y.detach() > 0)

    def conv(t, i, stride=1, pad=1):
        return F.conv2d(t, P[f"model.{i}.weight"], P[f"model.{i}.bias"], stride=stride, padding=pad)

    def bn(t, i):
        return F.batch_norm(t, sd[f"model.{i}.running_mean"].to(dtype).clone(), sd[f"model.{i}.running_var"].to(dtype).clone(),
                            P[f"model.{i}.weight"], P[f"model.{i}.bias"], training, 0.1, 1e-5)

    y = act(conv(xx, 0))
    y = act(bn(conv(y, 2, 2), 3))
    y = act(bn(conv(y, 5), 6))
    y = act(bn(conv(y, 8, 2), 9))
    y = act(bn(conv(y, 11), 12))
    y = act(conv(F.adaptive_avg_pool2d(y, 1), 15, pad=0))
    p = torch.sigmoid(conv(y, 17, pad=0).view(-1))
    F.binary_cross_entropy(p, torch.full_like(p, target)).backward()
    return {k: P[k].grad for k in PARAMS}, xx.grad, ys, p.detach()


def rel_errors(got, got_x, ref, ref_x, training):
    """e(T) of every parameter gradient and of the input gradient."""
    out = {}
    for k in PARAMS:
        den = float(ref[k].abs().max())
        if training and k in BN_BIASES:
            den = float(ref[k.replace("bias", "weight")].abs().max())
        out[k] = float((got[k].double() - ref[k]).abs().max()) / den
    if got_x is not None:
        out["input"] = float((got_x.double() - ref_x).abs().max()) / float(ref_x.abs().max())
    return out


def check_mask_cap(masks, ys, who):
    """A mask may differ from y64 > 0 only at |y64| <= 1e-5 * max|y64|, at no more than ceil(1e-5 * units) units per layer."""
    for i, (m, y) in enumerate(zip(masks, ys)):
        flips = m.reshape(y.shape) != (y > 0)
        nf = int(flips.sum())
        if nf:
            worst = float(y[flips].abs().max()) / float(y.abs().max())
            print(f"    {who} mask {i}: {nf} of {y.numel()} units differ from y64 > 0, all at |y64| <= {worst:.1e} * max|y64|")
            assert worst <= MASK_CAP, (who, i, worst)
        assert nf <= math.ceil(MASK_CAP * y.numel()), (who, i, nf)


# ------------------------------------------------------------------------------------------------------------- the C ABI, directly
def _module(kind, training, autograd=False, sd=None):
    from celebrity_image_denoiser_amd.srgan_disc import SRGANDiscriminator

    m = SRGANDiscriminator(autograd=autograd)
    m.load_state_dict(weights(kind) if sd is None else sd, strict=True)
    m.to(DEV)
    return m.train(training)


def _dims(x):
    if x.dtype == torch.uint8:
        return _lib.CID_FMT_U8_NHWC, x.shape[0], x.shape[1], x.shape[2]
    return _lib.CID_FMT_F32_NCHW, x.shape[0], x.shape[2], x.shape[3]


def _side(s):
    return (s - 1) // 2 + 1


def _bce_grad(p, target):
    """d BCE(p, target) / dp as torch computes it on the device."""
    leaf = p.clone().requires_grad_(True)
    nn.BCELoss()(leaf, torch.full_like(leaf, target)).backward()
    return leaf.grad


def cabi_backward(m, x, training, grad_fn, want=PARAMS, want_input=True, with_masks=True, ws_fill=None):
    """cid_srd_forward_saved + cid_srd_saved_masks + cid_srd_backward at m's weights on the device batch x, with clones of the running
    buffers (m is left as it was).  grad_fn(p) -> grad_prob; ws_fill: the byte the backward workspace is filled with first.
    -> (p, {key: grad}, grad_x or None, masks or None, grad_prob)"""
    from celebrity_image_denoiser_amd.discriminator import _BnArg

    L = _lib.lib()
    m.pack_weights()
    fmt, n, h, w = _dims(x)
    x = x.contiguous()
    keep = []
    bn = (_BnArg * 4)()
    for i, idx in enumerate(BN_IDX):
        b = m.model[idx]
        rm, rv, nbt = b.running_mean.clone(), b.running_var.clone(), b.num_batches_tracked.clone()
        keep += [rm, rv, nbt]
        bn[i] = _BnArg(b.weight.data_ptr(), b.bias.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), float(b.eps), float(b.momentum))
    need = ctypes.c_size_t()
    assert L.cid_srd_saved_bytes(n, h, w, int(training), ctypes.byref(need)) == 0
    saved = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    p = torch.empty(n, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check_srd(m._cid, L.cid_srd_forward_saved(m._cid, x.data_ptr(), fmt, p.data_ptr(), n, h, w, bn, int(training),
                                                   saved.data_ptr(), saved.numel(), stream))
    gp = grad_fn(p).to(torch.float32).contiguous()
    masks = None
    if with_masks:
        h2, w2 = _side(h), _side(w)
        h4, w4 = _side(h2), _side(w2)
        shapes = ((n, 64, h, w), (n, 64, h2, w2), (n, 128, h2, w2), (n, 128, h4, w4), (n, 256, h4, w4), (n, 512))
        masks = [torch.empty(s, dtype=torch.uint8, device=DEV) for s in shapes]
        ptrs = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in masks])
        assert L.cid_srd_saved_masks(saved.data_ptr(), saved.numel(), n, h, w, int(training), ptrs, stream) == 0
    sd = dict(m.named_parameters())
    grads = {k: torch.full(sd[k].shape, float("nan"), dtype=torch.float32, device=DEV) for k in want}
    g = Grads()
    for k, t in grads.items():
        idx, kind = int(k.split(".")[1]), k.rsplit(".", 1)[1]
        if idx in CONV_IDX:
            (g.w if kind == "weight" else g.b)[CONV_IDX.index(idx)] = t.data_ptr()
        else:
            (g.gamma if kind == "weight" else g.beta)[BN_IDX.index(idx)] = t.data_ptr()
    gx = None
    if want_input:
        gx = torch.full((n, 3, h, w), float("nan"), dtype=torch.float32, device=DEV)
        g.input = gx.data_ptr()
    assert L.cid_srd_backward_workspace_bytes(n, h, w, int(training), ctypes.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    _lib.check_srd(m._cid, L.cid_srd_backward(m._cid, x.data_ptr(), fmt, gp.data_ptr(), n, h, w, bn, int(training), saved.data_ptr(),
                                              saved.numel(), ctypes.byref(g), ws.data_ptr(), ws.numel(), stream))
    torch.cuda.synchronize()
    return p, grads, gx, masks, gp


# ------------------------------------------------------------------------------------------------------------------ gradient parity
PARITY_CASES = [((8, 37, 53), True), ((8, 37, 53), False), ((3, 41, 70), True), ((3, 41, 70), False), ((4, 7, 5), True),
                ((4, 7, 5), False), ((2, 8, 8), True), ((2, 1, 1), False)]   # (2,1,1) in train mode is ill-conditioned whoever computes it


@pytest.mark.parametrize("kind", WSETS)
@pytest.mark.parametrize("shape,training", PARITY_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("train" if v else "eval"))
@pytest.mark.parametrize("loss", ("real1", "fake0"))
def test_gradient_parity(kind, shape, training, loss):
    """BCE(D(x), 1) and BCE(D(perturbed x), 0), each on its own: all 22 parameter gradients and the input gradient."""
    x = images(*shape, first_index=sum(shape))[1]
    target = 1.0
    if loss == "fake0":
        x = (x + 0.05 * torch.sin(torch.arange(x.numel(), dtype=torch.float32).reshape(x.shape))).clamp(-1, 1)
        target = 0.0
    sd = weights(kind)
    m = _module(kind, training)
    p, grads, gx, masks, _ = cabi_backward(m, x.to(DEV), training, lambda q: _bce_grad(q, target))
    got = {k: v.cpu() for k, v in grads.items()}
    masks = [t.cpu().bool() for t in masks]
    # float64 with the device's masks
    g64, gx64, ys64, p64 = ref_backward(sd, x, training, target, torch.float64, masks)
    e_p = float((p.cpu().double() - p64).abs().max())
    print(f"\ngradient parity {kind} {shape} {'train' if training else 'eval'} {loss}: max|p - p64| = {e_p:.2e}")
    assert e_p <= TOL
    check_mask_cap(masks, ys64, "hip")
    e_hip = rel_errors(got, gx.cpu(), g64, gx64, training)
    # ATen fp32 with its own masks, against float64 with ATen's masks
    g32, gx32, ys32, _ = ref_backward(sd, x, training, target, torch.float32)
    masks32 = [y > 0 for y in ys32]
    check_mask_cap(masks32, ys64, "aten")
    g64a, gx64a, _, _ = ref_backward(sd, x, training, target, torch.float64, masks32)
    e_aten = rel_errors(g32, gx32, g64a, gx64a, training)
    print("                       e_hip      e_aten(fp32, CPU)")
    for k in PARAMS + ["input"]:
        flag = "" if e_hip[k] <= TOL else ("  (2*e_aten branch)" if e_hip[k] <= 2 * e_aten[k] else "  FAIL")
        print(f"    {k:16s} {e_hip[k]:.2e}   {e_aten[k]:.2e}{flag}")
    for k in PARAMS + ["input"]:
        assert all(bool(torch.isfinite(t).all()) for t in ([got[k]] if k != "input" else [gx]))
        assert e_hip[k] <= max(TOL, 2 * e_aten[k]), (k, e_hip[k], e_aten[k])


# ------------------------------------------------------------------------------------------------------------------ the saved forward
@pytest.mark.parametrize("training", (False, True))
def test_forward_saved_is_bit_identical_to_forward(training):
    """Probabilities and all BatchNorm buffers, fp32 and uint8 input, two consecutive calls."""
    for kind in WSETS:
        plain, auto = _module(kind, training), _module(kind, training, autograd=True)
        for call in range(2):
            u8, x = images(6, 45, 38, first_index=17 + call)
            for inp in (x.to(DEV), torch.from_numpy(u8).to(DEV)):
                pp, pa = plain(inp), auto(inp)
                assert pp.grad_fn is None and pa.grad_fn is not None
                assert torch.equal(pp, pa.detach())
                for i, _ in BNS:
                    for b in ("running_mean", "running_var", "num_batches_tracked"):
                        assert torch.equal(getattr(plain.model[i], b), getattr(auto.model[i], b)), (kind, call, i, b)
        assert int(auto.model[12].num_batches_tracked) == int(weights(kind)["model.12.num_batches_tracked"]) + (4 if training else 0)


@pytest.mark.parametrize("kind", WSETS)
def test_device_pack_equals_host_pack(kind):
    host, dev = _module(kind, False), _module(kind, False, autograd=True)
    a, b = host.pack_weights(), dev.pack_weights()
    torch.cuda.synchronize()
    assert a.numel() == b.numel() == _lib.lib().cid_srd_packed_weights_bytes()
    assert torch.equal(a, b)
    # after an in-place update the device pack follows, into the same blob; the host pack of the same tensors agrees again
    with torch.no_grad():
        for q1, q2 in zip(host.parameters(), dev.parameters()):
            q1.mul_(1.25)
            q2.mul_(1.25)
    a2, b2 = host.pack_weights(), dev.pack_weights()
    assert torch.equal(a2, b2) and b2.data_ptr() == b.data_ptr()
    assert not torch.equal(a, a2)


# ------------------------------------------------------------------------------------------------------------------ subsets, uint8
def test_subsets_and_uint8_input_give_the_same_bits():
    u8 = torch.from_numpy(images_u8(4, 24, 20, first_index=5)).to(DEV)
    x = images(4, 24, 20, first_index=5)[1].to(DEV)
    m = _module("trained", True)
    gfn = lambda q: _bce_grad(q, 1.0)   # noqa: E731
    p_u8, g_u8, gx_u8, _, _ = cabi_backward(m, u8, True, gfn, want_input=False, with_masks=False)
    p_f, g_f, gx_f, _, _ = cabi_backward(m, x, True, gfn, with_masks=False)
    assert gx_u8 is None and gx_f is not None and bool(torch.isfinite(gx_f).all())
    assert torch.equal(p_u8, p_f) and all(torch.equal(g_u8[k], g_f[k]) for k in PARAMS)   # u8 batch == its normalised copy
    # a subset: only what is asked for is written, and it has the same bits
    for sub in (("model.11.weight", "model.12.bias", "model.15.weight", "model.17.bias"), ("model.17.weight",), ("model.12.weight",),
                ("model.11.bias",), ("model.9.weight", "model.0.bias")):
        _, g_sub, _, _, _ = cabi_backward(m, x, True, gfn, want=sub, want_input=False, with_masks=False)
        assert set(g_sub) == set(sub) and all(torch.equal(g_sub[k], g_f[k]) for k in g_sub), sub
    _, g_low, gx_low, _, _ = cabi_backward(m, x, True, gfn, want=(), want_input=True, with_masks=False)
    assert g_low == {} and torch.equal(gx_low, gx_f)


def test_backward_is_deterministic_and_eval_input_gradient_is_batch_independent():
    x = images(8, 40, 48, first_index=900)[1].to(DEV)
    for training in (True, False):
        m = _module("trained", training)
        runs = [cabi_backward(m, x, training, lambda q: _bce_grad(q, 0.0), with_masks=False) for _ in range(2)]
        assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in PARAMS)
        assert torch.equal(runs[0][2], runs[1][2]) and torch.equal(runs[0][0], runs[1][0])
    gp = runs[0][4]
    for i in (0, 5):
        _, _, gxi, _, _ = cabi_backward(m, x[i:i + 1], False, lambda q: gp[i:i + 1], want=(), with_masks=False)
        assert torch.equal(gxi[0], runs[0][2][i])


@pytest.mark.parametrize("training", (False, True), ids=("eval", "train"))
def test_workspace_is_written_before_it_is_read(training):
    """The backward reads nothing it did not write: a workspace full of NaN bytes gives the bits a zeroed one gives."""
    x = images(3, 41, 70, first_index=114)[1].to(DEV)
    m = _module("trained", training)
    gfn = lambda q: _bce_grad(q, 1.0)   # noqa: E731
    _, g0, gx0, _, _ = cabi_backward(m, x, training, gfn, with_masks=False, ws_fill=0)
    _, g1, gx1, _, _ = cabi_backward(m, x, training, gfn, with_masks=False, ws_fill=0xFF)
    assert bool(torch.isfinite(gx1).all()) and torch.equal(gx0, gx1)
    for k in PARAMS:
        assert bool(torch.isfinite(g1[k]).all()) and torch.equal(g0[k], g1[k]), k


# ------------------------------------------------------------------------------------------------------------------ model.11's halves
@pytest.mark.parametrize("training", (False, True), ids=("eval", "train"))
@pytest.mark.parametrize("zeroed", ("upper", "lower"))
def test_channel_halves_of_layer_11(zeroed, training):
    """model.11's gradients run as two 128-channel halves (weight gradient: grid z; data gradient: two weight blocks).  On both sides
    model.15 ignores the half in question, so nothing flows back into it.  Zeroing that half's output channels of model.11 as well
    then leaves the other half's gradients, and everything below, with the same bits, and the zeroed half's own gradients exactly 0:
    a half that reads the other's dz, coefficients or weights, or writes at the other's offset, does not survive both cases."""
    half, other = (slice(128, 256), slice(0, 128)) if zeroed == "upper" else (slice(0, 128), slice(128, 256))
    base = weights("trained")
    base["model.15.weight"][:, half] = 0.0
    cut = {k: v.clone() for k, v in base.items()}
    cut["model.11.weight"][half] = 0.0
    cut["model.11.bias"][half] = 0.0
    x = images(3, 41, 70, first_index=114)[1].to(DEV)
    gfn = lambda q: _bce_grad(q, 1.0)   # noqa: E731
    p0, g0, gx0, _, _ = cabi_backward(_module("trained", training, sd=base), x, training, gfn, with_masks=False)
    p1, g1, gx1, _, _ = cabi_backward(_module("trained", training, sd=cut), x, training, gfn, with_masks=False)
    assert torch.equal(p0, p1)
    for k in ("model.11.weight", "model.11.bias", "model.12.weight", "model.12.bias"):
        assert torch.equal(g1[k][other], g0[k][other]), k
        assert k == "model.11.bias" or float(g0[k][other].abs().max()) > 0, k   # (a bias before a train-mode BatchNorm: true value 0)
    assert float(g1["model.12.weight"][half].abs().max()) == 0.0 and float(g1["model.11.weight"][half].abs().max()) == 0.0
    assert torch.equal(g1["model.15.weight"][:, other], g0["model.15.weight"][:, other])
    for k in PARAMS:
        if int(k.split(".")[1]) < 11:
            assert torch.equal(g1[k], g0[k]), k
    assert torch.equal(gx1, gx0) and float(gx0.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------ launch split
def test_launch_split_above_65535_images():
    """N = 65,537 images of 1x1 in eval mode: the input gradients on both sides of the launch seam equal one-image calls."""
    n = 65537
    u = synth.hash_uniform(20261019, 12, n * 3).astype(np.float32)
    x = torch.from_numpy(2.0 * u - 1.0).reshape(n, 3, 1, 1).to(DEV)
    m = _module("trained", False)
    p, grads, gx, _, gp = cabi_backward(m, x, False, lambda q: _bce_grad(q, 1.0), with_masks=False)
    for k in PARAMS:
        assert bool(torch.isfinite(grads[k]).all()) and float(grads[k].abs().max()) > 0, k
    assert bool(torch.isfinite(gx).all())
    for i in (0, 65534, 65535, 65536):
        pi, _, gxi, _, _ = cabi_backward(m, x[i:i + 1], False, lambda q: gp[i:i + 1], want=(), with_masks=False)
        assert torch.equal(pi[0], p[i]) and torch.equal(gxi[0], gx[i]), i
        assert float(gxi.abs().max()) > 0
    pd = p.double()
    assert float(grads["model.17.bias"][0]) == pytest.approx(float((gp.double() * pd * (1 - pd)).sum()), rel=1e-5)


# ------------------------------------------------------------------------------------------------------------------ the Python layer
def test_autograd_module_matches_the_c_abi_bit_for_bit():
    x = images(4, 24, 20, first_index=5)[1].to(DEV)
    u8 = torch.from_numpy(images_u8(4, 24, 20, first_index=5)).to(DEV)
    gfn = lambda q: _bce_grad(q, 1.0)   # noqa: E731
    _, g_f, gx_f, _, _ = cabi_backward(_module("trained", True), x, True, gfn, with_masks=False)
    a = _module("trained", True, autograd=True)
    pa = a(x)
    assert pa.grad_fn is not None and pa.requires_grad
    nn.BCELoss()(pa, torch.ones(4, device=DEV)).backward()
    assert [k for k, _ in a.named_parameters()] == PARAMS
    assert all(q.grad is not None and torch.equal(q.grad, g_f[k]) for k, q in a.named_parameters())
    # a uint8 batch: the same parameter gradients, no input gradient to give
    a.zero_grad()
    nn.BCELoss()(a(u8), torch.ones(4, device=DEV)).backward()
    assert all(torch.equal(q.grad, g_f[k]) for k, q in a.named_parameters())
    # the input gradient alone
    for q in a.parameters():
        q.requires_grad_(False)
    xr = x.clone().requires_grad_(True)
    nn.BCELoss()(a(xr), torch.ones(4, device=DEV)).backward()
    assert torch.equal(xr.grad, gx_f)
    assert a(x).grad_fn is None           # nothing requires grad: the plain forward


def test_in_place_parameter_change_between_forward_and_backward_raises():
    x = images(4, 16, 16, first_index=3)[1].to(DEV)
    m = _module("trained", True, autograd=True)
    loss = nn.BCELoss()(m(x), torch.ones(4, device=DEV))
    with torch.no_grad():
        m.model[11].weight.mul_(0.5)
    with pytest.raises(RuntimeError, match="modified in place"):
        loss.backward()
    with torch.no_grad():
        assert m(x).grad_fn is None
    # autograd=False keeps the forward-only behaviour
    plain = _module("trained", True)
    p = plain(x)
    assert not p.requires_grad and p.grad_fn is None
    with pytest.raises(RuntimeError, match="does not require grad"):
        nn.BCELoss()(p, torch.ones_like(p)).backward()


# ------------------------------------------------------------------------------------------------------------------ the trainer's steps
def _adv_gradient_check(D, sd_new, fake):
    """d BCE(D(fake), 1) / d fake at D's weights: (float64 gradient with the device's masks, e_hip, e_aten)."""
    _, _, gx, masks, _ = cabi_backward(D, fake, True, lambda q: _bce_grad(q, 1.0), want=())
    xc = fake.cpu()
    masks = [t.cpu().bool() for t in masks]
    _, gx64, ys64, _ = ref_backward(sd_new, xc, True, 1.0, torch.float64, masks)
    check_mask_cap(masks, ys64, "hip")
    _, gx32, ys32, _ = ref_backward(sd_new, xc, True, 1.0, torch.float32)
    _, gx64a, _, _ = ref_backward(sd_new, xc, True, 1.0, torch.float64, [y > 0 for y in ys32])
    e_aten = float((gx32.double() - gx64a).abs().max()) / float(gx64a.abs().max())
    e_hip = float((gx.cpu().double() - gx64).abs().max()) / float(gx64.abs().max())
    return gx64, e_hip, e_aten


def test_the_trainers_discriminator_and_generator_steps():
    """sr_ganTrainGNew.py:393-409 with a leaf tensor standing in for the generator's output."""
    import lpips_vgg_oracle
    from celebrity_image_denoiser_amd.lpips import load_vgg_loss

    B, S = 8, 32
    D = _module("trained", True, autograd=True)
    d_optimizer = torch.optim.Adam(D.parameters(), lr=1e-4)
    vgg_sd = {k: torch.from_numpy(v) for k, v in synth.vgg_loss_state_dict(lpips_vgg_oracle.weights("default")).items()}
    vgg_loss = load_vgg_loss(vgg_sd, device=DEV, autograd=True)
    bce_loss = nn.BCELoss()
    for step in range(2):
        hr_img = images(B, S, S, first_index=100 + 40 * step)[1].to(DEV)
        noise = 0.1 * torch.sin(torch.arange(hr_img.numel(), dtype=torch.float32, device=DEV).reshape(hr_img.shape) * (1 + step))
        fake_hr = (hr_img + noise).clamp(-1, 1).requires_grad_(True)      # the generator's output
        # the two single-loss gradients from the C ABI at the weights of this step
        _, g_real, _, _, _ = cabi_backward(D, hr_img, True, lambda q: _bce_grad(q, 1.0), want_input=False, with_masks=False)
        _, g_fake, _, _, _ = cabi_backward(D, fake_hr.detach(), True, lambda q: _bce_grad(q, 0.0), want_input=False, with_masks=False)

        d_optimizer.zero_grad()
        real_pred = D(hr_img)
        fake_pred = D(fake_hr.detach())
        d_loss = bce_loss(real_pred, torch.ones_like(real_pred)) + bce_loss(fake_pred, torch.zeros_like(fake_pred))
        d_loss.backward()
        assert fake_hr.grad is None
        for k, q in D.named_parameters():
            want = g_real[k].double() + g_fake[k].double()
            assert q.grad is not None and q.grad.shape == q.shape, k
            scale = float(torch.maximum(g_real[k].abs().max(), g_fake[k].abs().max()))
            assert float((q.grad.double() - want).abs().max()) <= 4 * 2.0 ** -24 * scale, k      # one fp32 addition of the two
        d_optimizer.step()

        # the next forward runs at the UPDATED weights (repacked on the device)
        sd_new = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
        fake_pred = D(fake_hr)
        ref = restate(cast(sd_new, torch.float64), fake_hr.detach().cpu().double(), True)
        assert float((fake_pred.detach().cpu().double() - ref).abs().max()) <= TOL
        content_loss = vgg_loss(fake_hr, hr_img)
        adv_loss = bce_loss(fake_pred, torch.ones_like(fake_pred))
        g_loss = content_loss + 0.001 * adv_loss
        g_loss.backward()
        # the VGG loss's own input gradient, from a separate call on a detached copy
        leaf = fake_hr.detach().clone().requires_grad_(True)
        vgg_loss(leaf, hr_img).backward()
        gx64, e_hip, e_aten = _adv_gradient_check(D, sd_new, fake_hr.detach())
        print(f"step {step}: d adv / d fake_hr  e_hip {e_hip:.2e}  e_aten {e_aten:.2e}")
        assert e_hip <= max(TOL, 2 * e_aten)
        want = leaf.grad.cpu().double() + 0.001 * gx64
        got = fake_hr.grad.cpu().double()
        e = float((got - want).abs().max()) / float(want.abs().max())
        print(f"step {step}: d g_loss / d fake_hr  e {e:.2e}")
        assert e <= max(TOL, 2 * e_aten)
    assert int(D.model[12].num_batches_tracked) == int(weights("trained")["model.12.num_batches_tracked"]) + 3 * 2

    # the device-side Adam takes the 22 tensors in one launch; the next forward follows it
    opt = cid.Adam(D.parameters(), lr=1e-4)
    before = [q.detach().clone() for q in D.parameters()]
    opt.zero_grad()
    bce_loss(D(hr_img), torch.ones(B, device=DEV)).backward()
    opt.step()
    assert len(before) == 22 and len(opt.state) == 22
    assert all(not torch.equal(b, q) for b, q in zip(before, D.parameters()) if bool(q.grad.any()))
    assert sum(bool(q.grad.any()) for q in D.parameters()) >= 18    # (the four biases in front of a BatchNorm may get an exact 0)
    sd_new = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
    got = D(hr_img).detach().cpu().double()
    ref = restate(cast(sd_new, torch.float64), hr_img.cpu().double(), True)
    assert float((got - ref).abs().max()) <= TOL
