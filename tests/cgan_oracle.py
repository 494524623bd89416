"""Float64 restatement of the server's CGANGenerator forward (reference backend/app.py:105-143, the label branch, eval mode) in numpy:
the reference the GPU tests of cid_cg_forward measure against.  The transposed convolution is written as its scatter definition
(every input pixel adds its 4 x 4 stamp to the output), not as the four-parity gather the kernel uses; `conv_transpose_parity` is that
second form, kept here so that the host tests can hold the two against each other."""
import numpy as np

EPS = 1e-5   # nn.BatchNorm2d's default, which the reference keeps
TOL = 1e-5   # the project's per-stage rule: max|delta| <= TOL * max(1, max|ref64|) per tensor
UPS = ((2, 3), (5, 6), (8, 9))   # (ConvTranspose2d, BatchNorm2d) indices inside `model`


def conv_transpose_scatter(x, w, b=None):
    """ConvTranspose2d(4, stride 2, padding 1) by definition: x [N,CI,H,W], w [CI,CO,4,4] -> [N,CO,2H,2W];
    out[n, co, 2 iy - 1 + ky, 2 ix - 1 + kx] += x[n, ci, iy, ix] * w[ci, co, ky, kx]."""
    n, ci, h, wd = x.shape
    co = w.shape[1]
    full = np.zeros((n, co, 2 * h + 2, 2 * wd + 2), dtype=np.result_type(x, w))   # index = output index + 1
    for ky in range(4):
        for kx in range(4):
            full[:, :, ky:ky + 2 * h:2, kx:kx + 2 * wd:2] += np.einsum("nchw,cd->ndhw", x, w[:, :, ky, kx])
    out = full[:, :, 1:-1, 1:-1]
    return out if b is None else out + np.asarray(b).reshape(1, -1, 1, 1)


def conv_transpose_parity(x, w, b=None):
    """The same as four 2 x 2 convolutions, one per output parity (py, px): output (2m + py, 2n + px) gathers inputs
    (m - 1 + py + dy, n - 1 + px + dx), dy, dx in {0, 1}, through kernel taps (3 - py - 2 dy, 3 - px - 2 dx): k_cg_up's index
    arithmetic."""
    n, ci, h, wd = x.shape
    co = w.shape[1]
    xp = np.zeros((n, ci, h + 2, wd + 2), dtype=x.dtype)   # one-pixel halo of zeros: index = input index + 1
    xp[:, :, 1:-1, 1:-1] = x
    out = np.zeros((n, co, 2 * h, 2 * wd), dtype=np.result_type(x, w))
    for py in range(2):
        for px in range(2):
            for dy in range(2):
                for dx in range(2):
                    ky, kx = 3 - py - 2 * dy, 3 - px - 2 * dx
                    out[:, :, py::2, px::2] += np.einsum("nchw,cd->ndhw", xp[:, :, py + dy:py + dy + h, px + dx:px + dx + wd], w[:, :, ky, kx])
    return out if b is None else out + np.asarray(b).reshape(1, -1, 1, 1)


def conv3x3(x, w, b):
    """Conv2d(3, padding 1): x [N,CI,H,W], w [CO,CI,3,3]."""
    n, ci, h, wd = x.shape
    xp = np.zeros((n, ci, h + 2, wd + 2), dtype=x.dtype)
    xp[:, :, 1:-1, 1:-1] = x
    out = np.zeros((n, w.shape[0], h, wd), dtype=np.result_type(x, w))
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("nchw,dc->ndhw", xp[:, :, ky:ky + h, kx:kx + wd], w[:, :, ky, kx])
    return out + np.asarray(b).reshape(1, -1, 1, 1)


def forward(sd, z, labels, dtype=np.float64, eps=EPS):
    """sd: state_dict of numpy arrays or tensors; z: [N,100] or [N,100,1,1]; labels: N ints in [0, n_classes) ->
    {"l1", "t1", "t2", "t3", "pre", "out"} as numpy arrays of `dtype`: l1 = ReLU(BN(l1(cat(z, emb)))) as [N,128,8,8], t<k> the k-th
    ConvTranspose2d -> BatchNorm -> ReLU, pre the sums before tanh."""
    p = {k: np.asarray(v) for k, v in sd.items()}
    p = {k: (v.astype(dtype) if v.dtype.kind == "f" else v) for k, v in p.items()}
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    z = np.asarray(z).astype(dtype).reshape(len(labels), -1)
    if labels.min() < 0 or labels.max() >= p["label_emb.weight"].shape[0]:
        raise IndexError("label out of range")

    def bn_relu(v, i):
        s = p[f"model.{i}.weight"] / np.sqrt(p[f"model.{i}.running_var"] + dtype(eps))
        y = (v - p[f"model.{i}.running_mean"].reshape(1, -1, 1, 1)) * s.reshape(1, -1, 1, 1) + p[f"model.{i}.bias"].reshape(1, -1, 1, 1)
        return np.maximum(y, 0)

    out = {}
    x = np.concatenate([z, p["label_emb.weight"][labels]], axis=1)
    cur = bn_relu((x @ p["l1.weight"].T + p["l1.bias"]).reshape(-1, 128, 8, 8), 0)
    out["l1"] = cur
    for k, (ic, ib) in enumerate(UPS):
        cur = bn_relu(conv_transpose_scatter(cur, p[f"model.{ic}.weight"], p[f"model.{ic}.bias"]), ib)
        out[f"t{k + 1}"] = cur
    out["pre"] = conv3x3(cur, p["model.11.weight"], p["model.11.bias"])
    out["out"] = np.tanh(out["pre"])
    return out


def to_u8(out):
    """The server's view of an output (app.py:435, 472): y * 0.5 + 0.5 -> clamp(0,1) -> ToPILImage = mul(255).byte(), [N,H,W,3].
    The output is rounded to fp32 FIRST and the view applied in fp32, as the server does: in float64 tanh(10) * 0.5 + 0.5 stays below
    1 and truncates to 254 where fp32 gives 255."""
    t = np.asarray(out).astype(np.float32)
    v = np.clip(t * np.float32(0.5) + np.float32(0.5), np.float32(0), np.float32(1)) * np.float32(255)
    return np.ascontiguousarray(v.astype(np.uint8).transpose(0, 2, 3, 1))


def bound(ref64):
    return TOL * max(1.0, float(np.abs(ref64).max()))
