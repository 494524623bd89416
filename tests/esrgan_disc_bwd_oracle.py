"""CPU autograd reference of the ESRGAN trainer's discriminator backward pass, for tests/test_esrgan_disc_backward_host.py and
tests/test_esrgan_disc_backward.py.  tests/esrgan_disc_oracle.py holds the forward's restatement, weights and images and is imported.

    ref_backward(sd, x, loss, dtype, masks)   gradients of the loss in `dtype` with given LeakyReLU masks (or the run's own, y > 0)
    reference(kind, shape, loss)              the shared runs of one case: float64 with its own masks, ATen fp32 and its errors
    rel_errors / check_mask_cap / bound       the rule of error of the sibling backward tests
    Grads                                     cid_esd_grads (include/cid.h)

Loss "real1" is BCEWithLogits(D(x), 1), "fake0" is BCEWithLogits(D(x), 0), both with mean reduction.

Rule of error.  Each fp32 run (the kernels', or ATen's on the CPU) is compared with a float64 run that takes THAT run's four masks
(conv1 ... conv4; the kernels' are a_l > 0 on the saved tensors).  A mask may differ from y64 > 0 only where |y64| <= 1e-5 * max|y64|
of that tensor, at no more than ceil(1e-5 * units) units per layer.  e(T) = max|g - g64| / max|g64|; the kernels must meet
e_hip(T) <= max(1e-5, 2 * e_aten(T)).
"""
import ctypes
import math

import torch
import torch.nn.functional as F

import esrgan_disc_oracle as oracle
from esrgan_disc_oracle import cast, weights  # noqa: F401

LAYERS = ("conv1", "conv2", "conv3", "conv4", "fc")
PARAMS = tuple(f"{l}.{k}" for l in LAYERS for k in ("weight", "bias"))
LOSSES = {"real1": 1.0, "fake0": 0.0}
# the forward's seven shapes; (5,40,24): conv4's weight-gradient workgroups walk item ranges that cross image boundaries; (1,66,258):
# two tiles with a partial last one in both directions for the kernels of conv4 (tests/test_esrgan_disc_backward.py's docstring)
ADDED = (1, 66, 258)
SHAPES = [(2, 1, 1), (4, 7, 5), (3, 16, 16), (2, 37, 53), (1, 70, 130), (1, 24, 264), (1, 264, 24), (5, 40, 24), ADDED]
TOL = 1e-5
MASK_CAP = 1e-5
# what the reference itself must satisfy for the first branch of the bound to govern (asserted in the host test)
# ATen fp32 on the CPU against float64.  What the condition is for is that the first branch of the bound governs, 2 * e_aten <= TOL,
# and that is what is asserted.  The figure itself is not portable: ATen's sums depend on the machine's threads.  The worst tensor of
# the issue's eight shapes measured 1.50e-6, 1.51e-6 and 1.56e-6 on three machines (conv1.bias / conv2.weight of (1,70,130)); the
# shape this pull request adds, the largest, 1.9e-6.
ATEN_ERR_MAX = TOL / 2
GRAD_FLOOR = 4.7e-5     # the smallest max|g64| of any tensor is 4.77e-5 (4.8e-5 to two digits), at (2,1,1) default real1
LOGIT_RANGE = (-1.0, 1.5)


class Grads(ctypes.Structure):
    """cid_esd_grads (include/cid.h)."""
    _fields_ = [("w", ctypes.c_void_p * 5), ("b", ctypes.c_void_p * 5), ("input", ctypes.c_void_p)]


class _MaskedLeaky(torch.autograd.Function):
    """Stock LeakyReLU(0.2) forward; backward g * where(mask, 1, 0.2) with a given mask."""

    @staticmethod
    def forward(ctx, y, mask):
        ctx.save_for_backward(mask)
        return F.leaky_relu(y, 0.2)

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        # the two slopes in g's dtype: torch.where on Python scalars would round 0.2 to float32 first
        return g * torch.where(mask, torch.ones((), dtype=g.dtype), torch.full((), 0.2, dtype=g.dtype)), None


def bce_grad(logits, loss):
    """d mean BCEWithLogits(logits, target) / d logits, as torch computes it where `logits` lives."""
    leaf = logits.detach().clone().requires_grad_(True)
    F.binary_cross_entropy_with_logits(leaf, torch.full_like(leaf, LOSSES[loss])).backward()
    return leaf.grad


def ref_backward(sd, x, loss, dtype, masks=None):
    """Gradients of the loss in `dtype` on the CPU.  masks: four bool tensors for LeakyReLU's backward, or None for the run's own
    (y > 0).  -> (param grads by state_dict key, input grad, the four pre-activations y, logits [N,1])"""
    P = {k: sd[k].to(dtype).clone().requires_grad_(True) for k in PARAMS}
    xx = x.to(dtype).clone().requires_grad_(True)
    ys = []
    y = xx
    for i, name in enumerate(LAYERS[:4]):
        y = F.conv2d(y, P[name + ".weight"], P[name + ".bias"], stride=2, padding=1)
        ys.append(y.detach())
        y = _MaskedLeaky.apply(y, masks[i].reshape(y.shape) if masks is not None else y.detach() > 0)
    logits = y.reshape(y.shape[0], -1) @ P["fc.weight"].t() + P["fc.bias"]
    F.binary_cross_entropy_with_logits(logits, torch.full_like(logits, LOSSES[loss])).backward()
    return {k: P[k].grad for k in PARAMS}, xx.grad, ys, logits.detach()


def rel_errors(got, got_x, ref, ref_x):
    """e(T) of every parameter gradient in `got` and of the input gradient."""
    out = {k: float((got[k].double() - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in got}
    if got_x is not None:
        out["input"] = float((got_x.double() - ref_x).abs().max()) / float(ref_x.abs().max())
    return out


def check_mask_cap(masks, ys, who):
    """A mask may differ from y64 > 0 only at |y64| <= 1e-5 * max|y64|, at no more than ceil(1e-5 * units) units per layer.
    -> the number of differing units."""
    total = 0
    for i, (m, y) in enumerate(zip(masks, ys)):
        flips = m.reshape(y.shape) != (y > 0)
        nf = int(flips.sum())
        if nf:
            worst = float(y[flips].abs().max()) / float(y.abs().max())
            print(f"    {who} mask {i}: {nf} of {y.numel()} units differ from y64 > 0, all at |y64| <= {worst:.1e} * max|y64|")
            assert worst <= MASK_CAP, (who, i, worst)
        assert nf <= math.ceil(MASK_CAP * y.numel()), (who, i, nf)
        total += nf
    return total


def bound(e_aten):
    return max(TOL, 2.0 * e_aten)


_REFS = {}


def reference(kind, shape, loss):
    """The shared CPU runs of one case, computed once and never modified:
        x       fp32 [N,3,H,W]          u8      its uint8 [N,H,W,3] source          sd    the weight set
        g64, gx64, ys64, logits64       float64 autograd with its own masks
        masks64                         ys64 > 0
        e_aten                          e(T) of ATen fp32 on the CPU against float64 with ATen's masks
        aten_flips                      mask units of the ATen run that differ from float64's"""
    key = (kind, tuple(shape), loss)
    if key not in _REFS:
        n, h, w = shape
        u8, x, _, _ = oracle.case(kind, shape)
        sd = weights(kind, (h, w))
        g64, gx64, ys64, lg64 = ref_backward(sd, x, loss, torch.float64)
        masks64 = [y > 0 for y in ys64]
        g32, gx32, ys32, _ = ref_backward(sd, x, loss, torch.float32)
        masks32 = [y > 0 for y in ys32]
        flips = check_mask_cap(masks32, ys64, "ATen")
        ga, gxa = (g64, gx64) if flips == 0 else ref_backward(sd, x, loss, torch.float64, masks32)[:2]
        _REFS[key] = dict(x=x, u8=u8, sd=sd, g64=g64, gx64=gx64, ys64=ys64, logits64=lg64, masks64=masks64,
                          e_aten=rel_errors(g32, gx32, ga, gxa), aten_flips=flips)
    return _REFS[key]


def ref_for_masks(ref, loss, masks):
    """(g64, gx64) of the float64 run that takes `masks`: the shared one where they are float64's own."""
    if all(torch.equal(m.reshape(m64.shape), m64) for m, m64 in zip(masks, ref["masks64"])):
        return ref["g64"], ref["gx64"]
    return ref_backward(ref["sd"], ref["x"], loss, torch.float64, masks)[:2]
