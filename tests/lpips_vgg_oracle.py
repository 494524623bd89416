"""Float64 restatement of VGG16 features as include/cid.h defines them (cid_vgg_lpips, cid_vgg_content_loss), for the tests and the
fixture maker.

forward(sd, a, b, unit_view=False) takes the state dict (numpy arrays, the lpips package's names) and two fp32 [N,3,H,W] batches and
returns float64 arrays: relu1 ... relu5 ([2 N,C,Hk,Wk]: operand a's N images, then operand b's, as the workspace holds them), layers
[N,5] = d_0 ... d_4 and d [N].  content(sd, a, b) returns relu1 ... relu3 of the UNSCALED operands and loss [N], the per-pair mean
squared difference of relu3.  Convolutions and pools are torch's, run in float64 on the CPU; the rest is written out.

CASES, CONTENT_CASES and pairs() are the shapes and operands the GPU tests and tests/golden/make_lpips_vgg_golden.py share."""
import numpy as np
import torch
import torch.nn.functional as F

from celebrity_image_denoiser_amd import synth

import lpips_oracle

TAPS = ("relu1", "relu2", "relu3", "relu4", "relu5")
CHANNELS = (64, 128, 256, 512, 512)
# per slice: the features indices of its convolutions; a 2x2 max-pool comes before every slice but the first
SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))

# (H, W, N): the issue's tables
CASES = ((16, 16, 1), (16, 16, 2), (16, 16, 70), (17, 19, 3), (35, 47, 3), (35, 47, 19), (64, 64, 2), (96, 72, 1), (128, 128, 2),
         (20, 264, 1), (264, 20, 1), (16, 512, 1))
CONTENT_CASES = ((4, 4, 2), (5, 7, 3), (35, 47, 3), (64, 64, 2), (128, 128, 2))

bound = lpips_oracle.bound
pairs = lpips_oracle.pairs
distance = lpips_oracle.distance


def first_index(h, w, n):
    return 7000 + 100 * h + w + n


def sizes(h, w):
    """((H1, W1), ..., (H5, W5)) of an h x w input."""
    out = [(h, w)]
    for _ in range(4):
        out.append((out[-1][0] // 2, out[-1][1] // 2))
    return tuple(out)


def taps(sd, x, unit_view=False, scaled=True, slices=5):
    """The taps of one tower, float64 tensors."""
    x = torch.from_numpy(np.asarray(x)).double()
    if unit_view:
        x = x * 0.5 + 0.5
    if scaled:
        shift = torch.from_numpy(np.asarray(sd["scaling_layer.shift"])).double().view(1, 3, 1, 1)
        scale = torch.from_numpy(np.asarray(sd["scaling_layer.scale"])).double().view(1, 3, 1, 1)
        x = (x - shift) / scale
    out = []
    for k, convs in enumerate(SLICES[:slices]):
        if k:
            x = F.max_pool2d(x, 2, 2)
        for idx in convs:
            w = torch.from_numpy(np.asarray(sd[f"net.slice{k + 1}.{idx}.weight"])).double()
            b = torch.from_numpy(np.asarray(sd[f"net.slice{k + 1}.{idx}.bias"])).double()
            x = F.relu(F.conv2d(x, w, b, padding=1))
        out.append(x)
    return out


def forward(sd, a, b, unit_view=False):
    with torch.no_grad():
        t0 = [t.numpy() for t in taps(sd, a, unit_view)]
        t1 = [t.numpy() for t in taps(sd, b, unit_view)]
    layers, d = distance(sd, t0, t1)
    out = {name: np.concatenate([x0, x1], axis=0) for name, x0, x1 in zip(TAPS, t0, t1)}
    out["layers"], out["d"] = layers, d
    return out


def content(sd, a, b):
    with torch.no_grad():
        t0 = [t.numpy() for t in taps(sd, a, scaled=False, slices=3)]
        t1 = [t.numpy() for t in taps(sd, b, scaled=False, slices=3)]
    out = {name: np.concatenate([x0, x1], axis=0) for name, x0, x1 in zip(TAPS, t0, t1)}
    out["loss"] = ((t0[2] - t1[2]) ** 2).mean(axis=(1, 2, 3))
    return out


def windex(cin, co, ci, kh, kw):
    """Packed index of w[co][ci][kh][kw] of a trunk convolution: channel group co / 64, chunk ci / 4, tap, ci % 4, co % 64."""
    return ((((co // 64) * (cin // 4) + ci // 4) * 9 + kh * 3 + kw) * 4 + ci % 4) * 64 + co % 64


def packed_blob(sd):
    """The device blob of cid_vgg_upload_weights for a full state dict, restated: the head as w[k][64] with k = (ci, kh, kw), its
    bias, shift at +64 and scale at +68 after it; per trunk convolution the packed weights then the biases; the five lin vectors."""
    head = np.zeros(27 * 64 + 128, dtype=np.float32)
    head[:27 * 64] = np.asarray(sd["net.slice1.0.weight"]).reshape(64, 27).T.reshape(-1)
    head[27 * 64:27 * 64 + 64] = sd["net.slice1.0.bias"]
    head[27 * 64 + 64:27 * 64 + 67] = np.asarray(sd["scaling_layer.shift"]).reshape(-1)
    head[27 * 64 + 68:27 * 64 + 71] = np.asarray(sd["scaling_layer.scale"]).reshape(-1)
    parts = [head]
    for k, convs in enumerate(SLICES):
        for idx in convs:
            if idx == 0:
                continue
            w = np.asarray(sd[f"net.slice{k + 1}.{idx}.weight"])
            cout, cin = w.shape[:2]
            co, ci, kh, kw = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(3), np.arange(3), indexing="ij")
            seg = np.empty(w.size, dtype=np.float32)
            seg[windex(cin, co, ci, kh, kw).reshape(-1)] = w.reshape(-1)
            parts += [seg, np.asarray(sd[f"net.slice{k + 1}.{idx}.bias"])]
    parts += [np.asarray(sd[f"lin{k}.model.1.weight"]).reshape(-1) for k in range(5)]
    return np.concatenate(parts)


_SD = {}


def weights(wset):
    """The synthetic VGG weight set, drawn once."""
    if wset not in _SD:
        _SD[wset] = synth.make_lpips_state_dict(wset, net="vgg")
    return _SD[wset]
