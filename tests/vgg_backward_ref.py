"""Float64 restatement of the VGG content loss's input gradient (cid_vgg_content_backward, include/cid.h), for the tests.

ReLU and max-pool make the gradient discontinuous, so an fp32 run is compared with a float64 backward that takes THAT run's
discontinuities: the seven ReLU masks (activation > 0) and the two pool routings (F.max_pool2d(..., return_indices=True) on that run's
relu1_2 and relu2_2).  The float64 forward itself is untouched.

    forward64(sd, x, unit)                     -> (pre[7], act[7]) of one tower, float64 tensors
    own_discontinuities(act)                   -> (masks[7], routes[2]) of any run's activations
    backward64(sd, act_a, f_b, grad_out, masks, routes, unit)   -> {"grad3_3", ..., "grad1_1", "grad_x"}: float64 tensors
    aten_fp32(sd, a, b, grad_out, unit)        -> (grads, masks, routes) of ATen fp32 autograd on the CPU
    check_masks / check_routing                the caps on sharing a run's discontinuities with the float64 reference
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

IDX = (0, 2, 5, 7, 10, 12, 14)                      # torchvision's features indices of the seven convolutions
SLICE = (1, 1, 2, 2, 3, 3, 3)
POOL_BEFORE = (False, False, True, False, True, False, False)
ACTS = ("relu1_1", "relu1_2", "relu2_1", "relu2_2", "relu3_1", "relu3_2", "relu3_3")
GRADS = ("grad3_3", "grad3_2", "grad3_1", "gradpool2", "grad2_1", "gradpool1", "grad1_1")
# the float64 quantity a stored gradient tensor holds: ("pre", i) = dL/d z_i, ("pool", k) = dL/d (output of pool k)
GRAD_OF = {"grad3_3": ("pre", 6), "grad3_2": ("pre", 5), "grad3_1": ("pre", 4), "gradpool2": ("pool", 1), "grad2_1": ("pre", 2),
           "gradpool1": ("pool", 0), "grad1_1": ("pre", 0)}


def params(sd, i, dtype):
    p = f"net.slice{SLICE[i]}.{IDX[i]}."
    return torch.from_numpy(np.asarray(sd[p + "weight"])).to(dtype), torch.from_numpy(np.asarray(sd[p + "bias"])).to(dtype)


def forward64(sd, x, unit=False):
    v = torch.from_numpy(np.asarray(x)).double()
    if unit:
        v = v * 0.5 + 0.5
    pre, act = [], []
    with torch.no_grad():
        for i in range(7):
            if POOL_BEFORE[i]:
                v = F.max_pool2d(v, 2, 2)
            w, b = params(sd, i, torch.float64)
            z = F.conv2d(v, w, b, padding=1)
            v = F.relu(z)
            pre.append(z)
            act.append(v)
    return pre, act


def own_discontinuities(act):
    masks = [a > 0 for a in act]
    routes = [F.max_pool2d(act[1], 2, 2, return_indices=True)[1], F.max_pool2d(act[3], 2, 2, return_indices=True)[1]]
    return masks, routes


def backward64(sd, act_a, f_b, grad_out, masks, routes, unit=False):
    """act_a: tower a's float64 activations, f_b: tower b's float64 relu3_3, grad_out: float64 [N]."""
    go = torch.as_tensor(np.asarray(grad_out), dtype=torch.float64).view(-1, 1, 1, 1)
    w = [params(sd, i, torch.float64)[0] for i in range(7)]
    m = [torch.as_tensor(np.asarray(k)).double() for k in masks]
    fa = act_a[6]
    count = fa[0].numel()
    g = {}
    d = go * (2.0 / count) * (fa - f_b) * m[6]
    g["grad3_3"] = d
    d = F.conv_transpose2d(d, w[6], padding=1) * m[5]
    g["grad3_2"] = d
    d = F.conv_transpose2d(d, w[5], padding=1) * m[4]
    g["grad3_1"] = d
    p = F.conv_transpose2d(d, w[4], padding=1)
    g["gradpool2"] = p
    d = F.max_unpool2d(p, torch.as_tensor(np.asarray(routes[1])), 2, 2, output_size=act_a[3].shape[-2:]) * m[3]
    d = F.conv_transpose2d(d, w[3], padding=1) * m[2]
    g["grad2_1"] = d
    p = F.conv_transpose2d(d, w[2], padding=1)
    g["gradpool1"] = p
    d = F.max_unpool2d(p, torch.as_tensor(np.asarray(routes[0])), 2, 2, output_size=act_a[1].shape[-2:]) * m[1]
    d = F.conv_transpose2d(d, w[1], padding=1) * m[0]
    g["grad1_1"] = d
    gx = F.conv_transpose2d(d, w[0], padding=1)
    g["grad_x"] = gx * 0.5 if unit else gx
    return g


def aten_fp32(sd, a, b, grad_out, unit=False):
    """ATen fp32 autograd of sum_n grad_out[n] * mean((slice(a_n) - slice(b_n))^2) on the CPU, with the gradients of the tensors
    the device stores, and that run's own masks and routings."""
    x = torch.from_numpy(np.array(a)).requires_grad_(True)
    y = torch.from_numpy(np.array(b))

    def tower(v, keep):
        pre, pooled, routes = [], [], []
        if unit:
            v = v * 0.5 + 0.5
        for i in range(7):
            if POOL_BEFORE[i]:
                v, idx = F.max_pool2d(v, 2, 2, return_indices=True)
                if keep:
                    v.retain_grad()
                pooled.append(v)
                routes.append(idx)
            w, bias = params(sd, i, torch.float32)
            z = F.conv2d(v, w, bias, padding=1)
            if keep:
                z.retain_grad()
            pre.append(z)
            v = F.relu(z)
        return v, pre, pooled, routes

    fa, pre, pooled, routes = tower(x, True)
    with torch.no_grad():
        fb = tower(y, False)[0]
    out = ((fa - fb) ** 2).mean(dim=(1, 2, 3))
    (out * torch.as_tensor(np.asarray(grad_out), dtype=torch.float32)).sum().backward()
    grads = {"grad_x": x.grad.double()}
    for name, (kind, i) in GRAD_OF.items():
        grads[name] = (pre[i] if kind == "pre" else pooled[i]).grad.double()
    return grads, [z.detach() > 0 for z in pre], [r.detach() for r in routes]


def cap(units):
    return max(2, math.ceil(1e-5 * units))


def check_masks(masks, pre64, what):
    """A run's ReLU masks may differ from the float64 forward's only where |pre64| <= 1e-5 max|pre64|, at no more than cap() units."""
    for name, m, z in zip(ACTS, masks, pre64):
        diff = torch.as_tensor(np.asarray(m)).bool() != (z > 0)
        n = int(diff.sum())
        assert n <= cap(z.numel()), (what, name, n)
        if n:
            assert float(z[diff].abs().max()) <= 1e-5 * float(z.abs().max()), (what, name, float(z[diff].abs().max()))


def check_routing(routes, act64, what):
    """A run's pool routings may differ from the float64 forward's only where the two candidates' float64 values differ by at most
    1e-5 max|y64|, at no more than cap() units."""
    for name, r, y in zip(("pool1", "pool2"), routes, (act64[1], act64[3])):
        r = torch.as_tensor(np.asarray(r))
        r64 = F.max_pool2d(y, 2, 2, return_indices=True)[1]
        diff = r != r64
        n = int(diff.sum())
        assert n <= cap(r64.numel()), (what, name, n)
        if n:
            flat = y.flatten(2)
            gap = (flat.gather(2, r.flatten(2)) - flat.gather(2, r64.flatten(2))).abs()
            assert float(gap.max()) <= 1e-5 * float(y.abs().max()), (what, name, float(gap.max()))


def rel_err(g, g64):
    """e(T) = max|g - g64| / max|g64|."""
    g, g64 = torch.as_tensor(np.asarray(g)).double(), torch.as_tensor(np.asarray(g64)).double()
    return float((g - g64).abs().max()) / float(g64.abs().max())
