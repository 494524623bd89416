"""Reference for the backward pass of the ESRGAN generator in train mode (cid_esr_backward): torch autograd on the CPU over the graph
of tests/esrgan_train_oracle.py with F.batch_norm(training=True), in float64 (the reference) or float32 (ATen fp32's own arithmetic).

The loss is (out * G).sum() with G a fixed seeded fp32 tensor in [-1, 1] divided by its element count, so grad_out = G.

PReLU's derivative is discontinuous, so a run can take the 1 + R PReLU backward masks (head, residuals.i.block.2) from another run:
the forward is untouched, the backward of a PReLU with mask m is g * where(m, 1, a) for its input and sum(g * v * ~m) for its slope.
The sharing is capped (check_mask_cap).

Error of a tensor T: e(T) = max|g - g64| / D(T), D(T) = max|g64| except
  * residuals.i.block.{0,3}.bias, whose true gradient under train-mode BatchNorm is 0: D = max|g64| of the same layer's weight gradient;
  * the PReLU slopes, sums with heavy cancellation: D = the float64 sum of |g * v| over the units with mask 0."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import esrgan_train_oracle as oracle

MASK_CAP = 1e-5
TOL = 1e-5


def param_names(num_residuals):
    names = ["initial.0.weight", "initial.0.bias", "initial.1.weight"]
    for i in range(num_residuals):
        b = f"residuals.{i}.block."
        names += [b + "0.weight", b + "0.bias", b + "1.weight", b + "1.bias", b + "2.weight", b + "3.weight", b + "3.bias", b + "4.weight",
                  b + "4.bias"]
    return names + ["final.weight", "final.bias"]


def slope_names(num_residuals):
    """The PReLUs in mask order."""
    return ["initial.1.weight"] + [f"residuals.{i}.block.2.weight" for i in range(num_residuals)]


def bn_biases(num_residuals):
    return tuple(f"residuals.{i}.block.{j}.bias" for i in range(num_residuals) for j in (0, 3))


# One more parity case, for an edge none of esrgan_train_oracle.PARITY_CASES crosses.  Every weight-gradient launch splits its items
# over a capped number of workgroups (128 for a trunk convolution's (image, 4 x 16 tile) items, 256 for the head's (image, row,
# 32-pixel segment) items, 512 for final's (image, 4 x 16 tile) items); on the six shapes above no launch has more items than its cap,
# so every workgroup runs ONE item.  66 images of 16 x 32 give 528, 1056 and 528 items: more than every cap by a fraction, so the
# ranges are uneven, a workgroup walks its item loop more than once, and ranges straddle two images in each launch (an image has 8, 16
# and 8 items).  It is the path the trainer's shape takes (8192 items over 128 workgroups at B=8, 256 x 256).
SPLIT_CASE = (66, 16, 32)
SPLIT_FIRST = 2700
# (R, (N, H, W)): the six shapes at R = 8, SMALL_CASES at R = 1, 2, 16 and at R = 0, and the split case
CASES = oracle.GPU_PARITY + [(0, c) for c in oracle.SMALL_CASES] + [(8, SPLIT_CASE)]


def case_id(rc):
    return f"R{rc[0]}-{oracle.case_id(rc[1])}"


def case_u8(case):
    from celebrity_image_denoiser_amd import synth

    return synth.esrgan_inputs_u8(*case, SPLIT_FIRST if case == SPLIT_CASE else oracle._FIRST[case])


def case_input(case):
    """fp32 [N,3,H,W] in [0,1] of the shape of a case of CASES: the /255 view of its synthetic uint8 batch."""
    if case != SPLIT_CASE:
        return oracle.case_input(case)
    return np.ascontiguousarray(case_u8(case).transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0)


def grad_out(n, h, w, seed=7):
    """G: fp32 [n,3,h,w] in [-1,1] / numel.  A bias or slope gradient under this loss is a sum of terms of random sign;
    test_esrgan_backward_host.py asserts that, with this seed, ATen fp32 is within 1e-5 of float64 on every tensor of every parity
    case, which is what makes max(1e-5, 2 * e_aten) a fair bound for another fp32 implementation."""
    g = np.random.default_rng(seed + 131 * n + 17 * h + w).uniform(-1.0, 1.0, (n, 3, h, w))
    return torch.from_numpy((g / g.size).astype(np.float32))


class _MaskedPReLU(torch.autograd.Function):
    """Stock PReLU forward; backward with a given mask.  Records sum |g * v| over the units with mask 0 in `book[name]`."""

    @staticmethod
    def forward(ctx, v, a, mask, book, name):
        ctx.save_for_backward(v, a, mask)
        ctx.book, ctx.name = book, name
        return torch.where(v > 0, v, a * v)

    @staticmethod
    def backward(ctx, g):
        v, a, mask = ctx.saved_tensors
        off = g * v * (~mask).to(g.dtype)
        ctx.book[ctx.name] = float(off.abs().double().sum())
        return g * torch.where(mask, torch.ones_like(a), a), off.sum().reshape(a.shape), None, None, None


def ref_backward(sd, x, G, num_residuals, dtype=torch.float64, masks=None):
    """sd: state_dict (numpy arrays or tensors); x fp32 [N,3,H,W]; G: grad_out.  masks: the 1 + R bool tensors for the PReLU backward,
    or None for the run's own (v > 0).
    -> (gradients by parameter name, the PReLU pre-activations in mask order, out, {slope name: sum |g * v| over mask 0})"""
    t = {k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}
    names = param_names(num_residuals)
    P = {k: t[k].to(dtype).clone().requires_grad_(True) for k in names}
    xx = torch.as_tensor(np.asarray(x)).to(dtype)
    pre, book = [], {}
    order = slope_names(num_residuals)

    def act(v, name):
        i = len(pre)
        assert order[i] == name
        pre.append(v.detach())
        m = masks[i].reshape(v.shape) if masks is not None else v.detach() > 0
        return _MaskedPReLU.apply(v, P[name], m, book, name)

    def bn(v, name):
        return F.batch_norm(v, t[name + ".running_mean"].to(dtype).clone(), t[name + ".running_var"].to(dtype).clone(), P[name + ".weight"],
                            P[name + ".bias"], True, oracle.MOMENTUM, oracle.EPS)

    x1 = act(F.conv2d(xx, P["initial.0.weight"], P["initial.0.bias"], padding=4), "initial.1.weight")
    cur = x1
    for i in range(num_residuals):
        b = f"residuals.{i}.block."
        y = bn(F.conv2d(cur, P[b + "0.weight"], P[b + "0.bias"], padding=1), b + "1")
        y = bn(F.conv2d(act(y, b + "2.weight"), P[b + "3.weight"], P[b + "3.bias"], padding=1), b + "4")
        cur = cur + y
    out = F.conv2d(x1 + cur, P["final.weight"], P["final.bias"], padding=4)
    (out * G.to(dtype)).sum().backward()
    return {k: P[k].grad for k in names}, pre, out.detach(), book


def rel_errors(got, ref, book):
    """e(T) of every parameter gradient; `book` is the float64 run's."""
    out = {}
    for k, r in ref.items():
        den = float(r.abs().max())
        if k.startswith("residuals.") and k.endswith((".0.bias", ".3.bias")):
            den = float(ref[k.replace("bias", "weight")].abs().max())
        elif k in book:
            den = book[k]
        out[k] = float((got[k].double().reshape(r.shape) - r).abs().max()) / den
    return out


def check_mask_cap(masks, pre64, who):
    """A mask may differ from v64 > 0 only at |v64| <= 1e-5 * max|v64|, at no more than ceil(1e-5 * units) units per layer.
    -> the number of differing units"""
    total = 0
    for i, (m, v) in enumerate(zip(masks, pre64)):
        flips = m.reshape(v.shape) != (v > 0)
        nf = int(flips.sum())
        total += nf
        if nf:
            worst = float(v[flips].abs().max()) / float(v.abs().max())
            print(f"    {who} mask {i}: {nf} of {v.numel()} units differ from v64 > 0, all at |v64| <= {worst:.1e} * max|v64|")
            assert worst <= MASK_CAP, (who, i, worst)
        assert nf <= math.ceil(MASK_CAP * v.numel()), (who, i, nf)
    return total


_ATEN = {}


def aten_errors(wset, rc, sd=None, tag=None):
    """ATen fp32 on one case of CASES against float64 with ATen's masks -> (e_aten per tensor, its flips).  Computed once per key."""
    from celebrity_image_denoiser_amd import synth

    key = (wset, rc, tag)
    if key not in _ATEN:
        r, case = rc
        n, h, w = case
        sd = synth.make_esrgan_state_dict(wset, r) if sd is None else sd
        x, G = case_input(case), grad_out(n, h, w)
        g32, pre32, _, _ = ref_backward(sd, x, G, r, torch.float32)
        m32 = [v > 0 for v in pre32]
        g64, pre64, _, book = ref_backward(sd, x, G, r, torch.float64, masks=m32)
        flips = check_mask_cap(m32, pre64, "ATen fp32")
        _ATEN[key] = (rel_errors(g32, g64, book), flips)
    return _ATEN[key]
