"""Reference for the backward pass of the SRGAN generator in train mode (cid_sr_backward): torch autograd on the CPU over the structure
of tests/srgan_train_oracle.py with F.batch_norm(training=True), in float64 (the reference) or float32 (ATen fp32's own arithmetic).

The loss is (out * G).sum() with G a fixed seeded fp32 tensor in [-1, 1] divided by its element count, so grad_out = G.

PReLU's derivative is discontinuous, so a run can take the 1 + 5 + stages PReLU backward masks (head, res_blocks.i.2, upscale.3k+2)
from another run: the forward is untouched, the backward of a PReLU with mask m is g * where(m, 1, a) for its input and
sum(g * v * ~m) for its slope.  The sharing is capped (check_mask_cap).

Error of a tensor T: e(T) = max|g - g64| / D(T), D(T) = max|g64| except
  * res_blocks.i.{0,3}.bias, whose true gradient under train-mode BatchNorm is 0: D = max|g64| of the same layer's weight gradient;
  * the PReLU slopes, sums with heavy cancellation: D = the float64 sum of |g * v| over the units with mask 0."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import srgan_train_oracle as oracle

NUM_BLOCKS = oracle.NUM_BLOCKS
MASK_CAP = 1e-5
TOL = 1e-5


def param_names(stages):
    names = ["initial.0.weight", "initial.0.bias", "initial.1.weight"]
    for i in range(NUM_BLOCKS):
        b = f"res_blocks.{i}."
        names += [b + "0.weight", b + "0.bias", b + "1.weight", b + "1.bias", b + "2.weight", b + "3.weight", b + "3.bias", b + "4.weight",
                  b + "4.bias"]
    names += ["mid.weight", "mid.bias"]
    for k in range(stages):
        names += [f"upscale.{3 * k}.weight", f"upscale.{3 * k}.bias", f"upscale.{3 * k + 2}.weight"]
    return names + ["final.weight", "final.bias"]


def slope_names(stages):
    """The PReLUs in mask order."""
    return ["initial.1.weight"] + [f"res_blocks.{i}.2.weight" for i in range(NUM_BLOCKS)] + [f"upscale.{3 * k + 2}.weight" for k in range(stages)]


BN_BIASES = tuple(f"res_blocks.{i}.{j}.bias" for i in range(NUM_BLOCKS) for j in (0, 3))


# One more parity case, for an edge none of srgan_train_oracle.PARITY_CASES crosses.  Every weight-gradient launch splits its (image,
# tile) items over a capped number of workgroups (128 for a trunk convolution, 32 for an upscale stage, 512 for final, 256 row
# segments for the head); on the six cases above no launch has more items than its cap, so every workgroup runs ONE item.  66 images
# of 8 x 16 at scale 2 give 132, 132, 528 and 528 items: more than every cap by a fraction, so the ranges are uneven (one or two, four
# or five items), a workgroup walks its item loop more than once, and ranges straddle two images in each of the four launches
# (an image has 2, 2, 8 and 8 items).  It is the path the trainer's shape takes (1024 items over 128 workgroups at B=16, 64 x 64).
SPLIT_CASE = (66, 8, 16, 2)
CASES = oracle.PARITY_CASES + [SPLIT_CASE]


def case_input(case):
    """fp32 [N,3,H,W] in [-1,1] of a case of CASES.  SPLIT_CASE's first image index is one at which ATen fp32 stands well inside 1e-5
    on every tensor (test_srgan_backward_host.py asserts it), as grad_out's seed is."""
    if case in oracle.PARITY_CASES:
        return oracle.case_input(case)
    from celebrity_image_denoiser_amd import synth

    return synth.normalize_u8(synth.srgan_inputs_u8(*case[:3], 2700))


def grad_out(n, scale, h, w, seed=7):
    """G: fp32 [n,3,scale*h,scale*w] in [-1,1] / numel.  A bias or slope gradient under this loss is a sum of terms of random sign;
    test_srgan_backward_host.py asserts that, with this seed, ATen fp32 is within 1e-5 of float64 on every tensor of every parity
    case, which is what makes max(1e-5, 2 * e_aten) a fair bound for another fp32 implementation."""
    g = np.random.default_rng(seed + 131 * n + 17 * h + w + 7 * scale).uniform(-1.0, 1.0, (n, 3, scale * h, scale * w))
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


def ref_backward(sd, x, G, dtype=torch.float64, masks=None, raw=False):
    """sd: state_dict (numpy arrays or tensors); x fp32 [N,3,H,W]; G: grad_out.  masks: the 1 + 5 + stages bool tensors for the PReLU
    backward, or None for the run's own (v > 0).
    -> (gradients by parameter name, the PReLU pre-activations in mask order, out, {slope name: sum |g * v| over mask 0})"""
    t = {k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}
    stages = sum(1 for k in t if k.startswith("upscale.") and k.endswith(".bias"))
    names = param_names(stages)
    P = {k: t[k].to(dtype).clone().requires_grad_(True) for k in names}
    xx = torch.as_tensor(np.asarray(x)).to(dtype)
    pre, book = [], {}
    order = slope_names(stages)

    def act(v, name):
        i = len(pre)
        assert order[i] == name
        pre.append(v.detach())
        m = masks[i].reshape(v.shape) if masks is not None else v.detach() > 0
        return _MaskedPReLU.apply(v, P[name], m, book, name)

    def bn(v, name):
        return F.batch_norm(v, t[name + ".running_mean"].to(dtype).clone(), t[name + ".running_var"].to(dtype).clone(), P[name + ".weight"],
                            P[name + ".bias"], True, oracle.MOMENTUM, oracle.EPS)

    x0 = act(F.conv2d(xx, P["initial.0.weight"], P["initial.0.bias"], padding=4), "initial.1.weight")
    cur = x0
    for i in range(NUM_BLOCKS):
        b = f"res_blocks.{i}."
        cur = bn(F.conv2d(cur, P[b + "0.weight"], P[b + "0.bias"], padding=1), b + "1")
        cur = bn(F.conv2d(act(cur, b + "2.weight"), P[b + "3.weight"], P[b + "3.bias"], padding=1), b + "4")
    u = F.conv2d(cur, P["mid.weight"], P["mid.bias"], padding=1) + x0
    for k in range(stages):
        u = act(F.pixel_shuffle(F.conv2d(u, P[f"upscale.{3 * k}.weight"], P[f"upscale.{3 * k}.bias"], padding=1), 2), f"upscale.{3 * k + 2}.weight")
    out = F.conv2d(u, P["final.weight"], P["final.bias"], padding=4)
    if not raw:
        out = torch.tanh(out)
    (out * G.to(dtype)).sum().backward()
    return {k: P[k].grad for k in names}, pre, out.detach(), book


def rel_errors(got, ref, book):
    """e(T) of every parameter gradient; `book` is the float64 run's."""
    out = {}
    for k, r in ref.items():
        den = float(r.abs().max())
        if k in BN_BIASES:
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


def aten_errors(wset, case, raw=False, sd=None, tag=None):
    """ATen fp32 on one parity case against float64 with ATen's masks -> (e_aten per tensor, its flips).  Computed once per key."""
    from celebrity_image_denoiser_amd import synth

    key = (wset, case, raw, tag)
    if key not in _ATEN:
        n, h, w, scale = case
        sd = synth.make_srgan_state_dict(wset, scale) if sd is None else sd
        x, G = case_input(case), grad_out(n, scale, h, w)
        g32, pre32, _, _ = ref_backward(sd, x, G, torch.float32, raw=raw)
        m32 = [v > 0 for v in pre32]
        g64, pre64, _, book = ref_backward(sd, x, G, torch.float64, masks=m32, raw=raw)
        flips = check_mask_cap(m32, pre64, "ATen fp32")
        _ATEN[key] = (rel_errors(g32, g64, book), flips)
    return _ATEN[key]
