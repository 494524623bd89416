"""Float64 restatement of LPIPS(net='alex') as include/cid.h defines it (cid_lpips), for the tests and the fixture maker.

forward(sd, a, b, unit_view=False) takes the state dict (numpy arrays, the package's names) and two fp32 [N,3,H,W] batches and
returns float64 arrays: relu1 ... relu5 ([2 N,C,Hs,Ws]: operand a's N images, then operand b's, as the workspace holds them),
layers [N,5] = d_0 ... d_4 and d [N].  Convolutions and pools are torch's, run in float64 on the CPU; the rest is written out.

CASES and pairs() are the shapes and operands the GPU tests and tests/golden/make_lpips_golden.py share."""
import numpy as np
import torch
import torch.nn.functional as F

from celebrity_image_denoiser_amd import synth

TAPS = ("relu1", "relu2", "relu3", "relu4", "relu5")
CONVS = (("net.slice1.0", 4, 2, False), ("net.slice2.3", 1, 2, True), ("net.slice3.6", 1, 1, True), ("net.slice4.8", 1, 1, False),
         ("net.slice5.10", 1, 1, False))   # (prefix, stride, padding, max-pool first)

# (H, W, N): the issue's table
CASES = ((31, 31, 1), (31, 31, 2), (31, 31, 5), (35, 47, 3), (35, 47, 19), (67, 33, 1), (64, 64, 2), (128, 128, 3), (200, 136, 1))


def sizes(h, w):
    """((H1, W1), (H2, W2), (H3, W3)) of an h x w input."""
    h1, w1 = (h - 7) // 4 + 1, (w - 7) // 4 + 1
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    h3, w3 = (h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1
    return (h1, w1), (h2, w2), (h3, w3)


def bound(ref):
    """The project's per-stage rule for a tap: max|delta| <= 1e-5 * max(1, max|ref|)."""
    return 1e-5 * max(1.0, float(np.abs(ref).max()))


def pairs(kind, n, h, w, first_index=0):
    """(a, b, a_u8, b_u8): fp32 [n,3,h,w] in [-1,1] and the uint8 [n,h,w,3] images they are the normalised copies of.
    "noisy": synth.make_batch's noisy / clean pairs (small distances); "unrelated": clean image i against clean image i + 1."""
    if kind == "noisy":
        x, clean, noisy_u8 = synth.make_batch(n, h, w, first_index=first_index)
        return x, clean, noisy_u8, synth.clean_images_u8(n, h, w, first_index)
    if kind == "unrelated":
        u8 = synth.clean_images_u8(n + 1, h, w, first_index)
        f = synth.normalize_u8(u8)
        return np.ascontiguousarray(f[:n]), np.ascontiguousarray(f[1:]), np.ascontiguousarray(u8[:n]), np.ascontiguousarray(u8[1:])
    raise ValueError(kind)


def taps(sd, x, unit_view=False):
    """The five taps of one tower, float64 tensors."""
    x = torch.from_numpy(np.asarray(x)).double()
    if unit_view:
        x = x * 0.5 + 0.5
    shift = torch.from_numpy(np.asarray(sd["scaling_layer.shift"])).double().view(1, 3, 1, 1)
    scale = torch.from_numpy(np.asarray(sd["scaling_layer.scale"])).double().view(1, 3, 1, 1)
    x = (x - shift) / scale
    out = []
    for prefix, stride, pad, pool in CONVS:
        if pool:
            x = F.max_pool2d(x, 3, 2)
        w = torch.from_numpy(np.asarray(sd[prefix + ".weight"])).double()
        b = torch.from_numpy(np.asarray(sd[prefix + ".bias"])).double()
        x = F.relu(F.conv2d(x, w, b, stride=stride, padding=pad))
        out.append(x)
    return out


def distance(sd, t0, t1):
    """(layers [N,5], d [N]) from the taps of the two towers (float64 arrays [N,C,Hs,Ws])."""
    layers = []
    for k, (x0, x1) in enumerate(zip(t0, t1)):
        x0, x1 = np.asarray(x0, dtype=np.float64), np.asarray(x1, dtype=np.float64)
        n0 = np.sqrt((x0 * x0).sum(axis=1, keepdims=True)) + 1e-10
        n1 = np.sqrt((x1 * x1).sum(axis=1, keepdims=True)) + 1e-10
        w = np.asarray(sd[f"lin{k}.model.1.weight"], dtype=np.float64).reshape(1, -1, 1, 1)
        layers.append((w * (x0 / n0 - x1 / n1) ** 2).sum(axis=1).mean(axis=(1, 2)))
    layers = np.stack(layers, axis=1)
    return layers, layers.sum(axis=1)


def forward(sd, a, b, unit_view=False):
    with torch.no_grad():
        t0 = [t.numpy() for t in taps(sd, a, unit_view)]
        t1 = [t.numpy() for t in taps(sd, b, unit_view)]
    layers, d = distance(sd, t0, t1)
    out = {name: np.concatenate([x0, x1], axis=0) for name, x0, x1 in zip(TAPS, t0, t1)}
    out["layers"], out["d"] = layers, d
    return out
