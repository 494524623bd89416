"""Portable synthetic weights and inputs for the denoise hot path.

The reference ships no trained denoise checkpoint in this tree and its server falls back to
random-init weights when the checkpoint is missing (reference backend/app.py:327-336), so every
parity test and the benchmark run on *seeded synthetic* weights.  Torch's RNG streams are not
portable between builds, so everything here comes from a counter-based splitmix64 hash: the same
(seed, key, index) gives the same float on every machine, with numpy only.

Inputs follow the reference's data recipe:
  * noisy = clip(clean + N(0, sigma=25), 0, 255).astype(uint8)
        reference backend/trainingcode/denoise_gan_code/noise_generation.py:6-10
  * x = (noisy/255 - 0.5)/0.5 as float32 NCHW
        reference backend/trainingcode/denoise_gan_code/training.py:152-155, backend/app.py:401-405
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)

WEIGHT_SEED = 0x5EED
CLEAN_SEED = 0xC0FFEE
NOISE_SEED = 0xBADD1E

# (key prefix, kind, Cin, Cout) in reference declaration order, backend/app.py:42-78.
LAYERS = (
    ("down1.0", "conv", 3, 64),
    ("down1.2", "conv", 64, 64),
    ("down2.0", "conv", 64, 128),
    ("down2.2", "conv", 128, 128),
    ("bottleneck.0", "conv", 128, 256),
    ("bottleneck.2", "conv", 256, 256),
    ("up2", "convT", 256, 128),
    ("upconv2.0", "conv", 256, 128),
    ("upconv2.2", "conv", 128, 128),
    ("up1", "convT", 128, 64),
    ("upconv1.0", "conv", 128, 64),
    ("upconv1.2", "conv", 64, 3),
)


def param_shapes() -> "OrderedDict[str, tuple]":
    """state_dict key -> shape, same names/shapes as the reference module (app.py:39-78)."""
    out: "OrderedDict[str, tuple]" = OrderedDict()
    for name, kind, cin, cout in LAYERS:
        if kind == "conv":
            out[name + ".weight"] = (cout, cin, 3, 3)  # nn.Conv2d: [Cout, Cin, kh, kw]
        else:
            out[name + ".weight"] = (cin, cout, 2, 2)  # nn.ConvTranspose2d: [Cin, Cout, kh, kw]
        out[name + ".bias"] = (cout,)
    return out


def splitmix64(x: np.ndarray) -> np.ndarray:
    """Vectorised splitmix64 finaliser on uint64 arrays (wrapping arithmetic)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def _fnv1a64(s: str) -> int:
    h = 0xCBF29CE484222325
    for b in s.encode("utf-8"):
        h ^= b
        h = (h * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def hash_uniform(seed: int, stream: int, n: int, offset: int = 0) -> np.ndarray:
    """n doubles in [0,1): element i = top 53 bits of splitmix64(splitmix64(seed^stream) + offset+i)."""
    base = splitmix64(np.array([(seed ^ stream) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))[0]
    idx = np.arange(offset, offset + n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = splitmix64(base + idx)
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def make_state_dict(kind: str = "default", seed: int = WEIGHT_SEED) -> "OrderedDict[str, np.ndarray]":
    """Synthetic float32 weights keyed like the reference state_dict.

    kind="default": U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weights and biases — the scale of
        PyTorch's default Conv2d init, i.e. of the server's random-init fallback (app.py:333-336).
    kind="hot": He-uniform weights U(+-sqrt(6/fan_in)), biases U(+-0.05): keeps activation
        variance through the ReLU stack so ReLU sparsity is ~50 % and tanh leaves its linear range.
    """
    if kind not in ("default", "hot"):
        raise ValueError(f"unknown weight set {kind!r}")
    sd: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for key, shape in param_shapes().items():
        n = int(np.prod(shape))
        layer = key.rsplit(".", 1)[0]
        wshape = param_shapes()[layer + ".weight"]
        fan_in = wshape[1] * wshape[2] * wshape[3]  # torch's rule, also for ConvTranspose2d
        if kind == "default":
            bound = 1.0 / math.sqrt(fan_in)
        elif key.endswith(".weight"):
            bound = math.sqrt(6.0 / fan_in)
        else:
            bound = 0.05
        u = hash_uniform(seed, _fnv1a64(kind + ":" + key), n)
        sd[key] = ((2.0 * u - 1.0) * bound).astype(np.float32).reshape(shape)
    return sd


def clean_images_u8(n: int, h: int, w: int, first_index: int = 0) -> np.ndarray:
    """[n,h,w,3] uint8 smooth "face-like" fields: an 8x8x3 hash grid, bilinearly upsampled."""
    out = np.empty((n, h, w, 3), dtype=np.uint8)
    ys = np.linspace(0.0, 7.0, h) if h > 1 else np.zeros(1)
    xs = np.linspace(0.0, 7.0, w) if w > 1 else np.zeros(1)
    y0 = np.minimum(ys.astype(np.int64), 6)
    x0 = np.minimum(xs.astype(np.int64), 6)
    fy = (ys - y0)[:, None, None]
    fx = (xs - x0)[None, :, None]
    for i in range(n):
        g = np.floor(hash_uniform(CLEAN_SEED + first_index + i, 0, 8 * 8 * 3) * 256.0).reshape(8, 8, 3)
        a = g[y0][:, x0]
        b = g[y0][:, x0 + 1]
        c = g[y0 + 1][:, x0]
        d = g[y0 + 1][:, x0 + 1]
        v = (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy
        out[i] = np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)
    return out


def add_gaussian_noise(clean_u8: np.ndarray, sigma: float = 25.0, first_index: int = 0) -> np.ndarray:
    """clip(img + N(0,sigma), 0, 255).astype(uint8) per image (noise_generation.py:6-10), with the
    normal deviates from Box-Muller on the hash stream so the result is machine-independent."""
    n = clean_u8.shape[0]
    per = int(np.prod(clean_u8.shape[1:]))
    out = np.empty_like(clean_u8)
    for i in range(n):
        u1 = hash_uniform(NOISE_SEED + first_index + i, 1, per)
        u2 = hash_uniform(NOISE_SEED + first_index + i, 2, per)
        z = np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)
        noisy = clean_u8[i].astype(np.float64).reshape(-1) + sigma * z
        out[i] = np.clip(noisy, 0, 255).astype(np.uint8).reshape(clean_u8.shape[1:])
    return out


def normalize_u8(img_u8_nhwc: np.ndarray) -> np.ndarray:
    """uint8 NHWC -> float32 NCHW in [-1,1]: ToTensor (/255) then Normalize(0.5,0.5)
    (app.py:401-405; training.py:152-155), both steps in float32 like torchvision."""
    t = img_u8_nhwc.astype(np.float32) / np.float32(255.0)
    t = (t - np.float32(0.5)) / np.float32(0.5)
    return np.ascontiguousarray(t.transpose(0, 3, 1, 2))


def make_batch(n: int, h: int, w: int, first_index: int = 0, sigma: float = 25.0):
    """(x_noisy f32 NCHW, clean f32 NCHW, noisy u8 NHWC) for images first_index..first_index+n-1."""
    clean = clean_images_u8(n, h, w, first_index)
    noisy = add_gaussian_noise(clean, sigma, first_index)
    return normalize_u8(noisy), normalize_u8(clean), noisy


# ---- the trainer's five noise kinds (noise_generation.py:6-39): bit-defined restatements of cid_add_noise ----
#
# Every draw comes from the hash streams above, never from np.random: image n of a call uses the seed
# seed + first_index + n, and element e = (y*W + x)*3 + c of an image is element e of each stream.  All arithmetic is
# float64 in the order written; results are np.clip(v, 0, 255).astype(np.uint8).  include/cid.h states the definitions and
# noise.add_noise computes the same bits on the GPU.

NOISE_TYPES = ("gaussian", "salt_pepper", "speckle", "poisson", "uniform")   # the trainer's list, training.py:247
NOISE_DEFAULTS = {                       # the reference's keyword defaults, in cid_add_noise's params order
    "gaussian": {"mean": 0.0, "sigma": 25.0},
    "salt_pepper": {"salt_prob": 0.02, "pepper_prob": 0.02},
    "speckle": {"mean": 0.0, "sigma": 0.1},
    "poisson": {},
    "uniform": {"low": 0.0, "high": 25.0},
}
NOISE_STREAMS = {
    "gaussian": (1, 2),                   # add_gaussian_noise's streams
    "speckle": (_fnv1a64("noise:speckle:u1"), _fnv1a64("noise:speckle:u2")),
    "uniform": (_fnv1a64("noise:uniform"),),
    "poisson": (_fnv1a64("noise:poisson"),),
    "salt_pepper": tuple(_fnv1a64("noise:salt_pepper:" + s) for s in ("salt_row", "salt_col", "pepper_row", "pepper_col")),
}
POISSON_KMAX = 1023


def _image_uniforms(seed: int, first_index: int, n: int, stream: int, per: int) -> np.ndarray:
    """[n, per] float64: row i is hash_uniform(seed + first_index + i, stream, per)."""
    return np.stack([hash_uniform(seed + first_index + i, stream, per) for i in range(n)]) if n else np.empty((0, per))


def _box_muller(u1: np.ndarray, u2: np.ndarray) -> np.ndarray:
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)


def noise_values_np(clean_u8: np.ndarray, kind: str, seed: int = NOISE_SEED, first_index: int = 0, **params) -> np.ndarray:
    """The float64 value v of every element before np.clip / uint8 truncation, for the kinds that have one (gaussian, speckle,
    uniform); [N,H,W,3] like the input."""
    if kind not in ("gaussian", "speckle", "uniform"):
        raise ValueError(f"{kind!r} has no float64 pre-clip value (poisson and salt_pepper are integer draws)")
    p = dict(NOISE_DEFAULTS[kind])
    unknown = set(params) - set(p)
    if unknown:
        raise TypeError(f"unknown parameter(s) {sorted(unknown)} for {kind!r} noise; expected {sorted(p)}")
    p.update(params)
    n = clean_u8.shape[0]
    per = int(np.prod(clean_u8.shape[1:]))
    img = clean_u8.reshape(n, per).astype(np.float64)
    streams = NOISE_STREAMS[kind]
    if kind == "uniform":
        u = _image_uniforms(seed, first_index, n, streams[0], per)
        v = img + (p["low"] + (p["high"] - p["low"]) * u)
    else:
        z = _box_muller(_image_uniforms(seed, first_index, n, streams[0], per),
                        _image_uniforms(seed, first_index, n, streams[1], per))
        noise = p["mean"] + p["sigma"] * z
        v = img + noise if kind == "gaussian" else img + img * noise
    return v.reshape(clean_u8.shape)


def _clip_u8(v: np.ndarray) -> np.ndarray:
    return np.clip(v, 0, 255).astype(np.uint8)


def add_speckle_noise(clean_u8: np.ndarray, mean: float = 0.0, sigma: float = 0.1, seed: int = NOISE_SEED,
                      first_index: int = 0) -> np.ndarray:
    """clip(img + img*(mean + sigma*z), 0, 255).astype(uint8) (noise_generation.py:24-28), z from Box-Muller on the speckle
    streams."""
    return _clip_u8(noise_values_np(clean_u8, "speckle", seed, first_index, mean=mean, sigma=sigma))


def add_uniform_noise(clean_u8: np.ndarray, low: float = 0.0, high: float = 25.0, seed: int = NOISE_SEED,
                      first_index: int = 0) -> np.ndarray:
    """clip(img + (low + (high-low)*u), 0, 255).astype(uint8) (noise_generation.py:35-39; numpy's uniform is low + (high-low)*u)."""
    return _clip_u8(noise_values_np(clean_u8, "uniform", seed, first_index, low=low, high=high))


def poisson_cdf_table() -> np.ndarray:
    """[256, POISSON_KMAX+1] float64: row lambda holds the running sums c_k of the inversion, p_0 = exp(-lambda) (math.exp: the
    host libm, as cid_add_noise uses std::exp), p_k = (p_{k-1}*lambda)/k, c_k = c_{k-1} + p_k.  Each row is non-decreasing."""
    lam = np.arange(256, dtype=np.float64)
    p = np.array([math.exp(-float(v)) for v in range(256)], dtype=np.float64)
    c = np.empty((256, POISSON_KMAX + 1), dtype=np.float64)
    c[:, 0] = p
    for k in range(1, POISSON_KMAX + 1):
        p = (p * lam) / float(k)
        c[:, k] = c[:, k - 1] + p
    return c


def add_poisson_noise(clean_u8: np.ndarray, seed: int = NOISE_SEED, first_index: int = 0) -> np.ndarray:
    """np.random.poisson(img).astype(np.uint8) (noise_generation.py:30-33) by inversion: lambda = the pixel value, k = 0, c = p =
    exp(-lambda); while u >= c and k < 1023: k += 1, p = (p*lambda)/k, c += p.  The result is k mod 256: the reference's cast
    wraps, so about 48 % of the pixels at 255 come out dark.  That quirk is kept on purpose.

    The loop stops at the first k with u < c_k, which for a non-decreasing row of the table is a binary search: the same bits,
    without a Python loop per element."""
    n = clean_u8.shape[0]
    per = int(np.prod(clean_u8.shape[1:]))
    lam = clean_u8.reshape(n, per)
    u = _image_uniforms(seed, first_index, n, NOISE_STREAMS["poisson"][0], per)
    table = poisson_cdf_table()
    lam, u = lam.reshape(-1), u.reshape(-1)
    order = np.argsort(lam, kind="stable")
    bounds = np.searchsorted(lam[order], np.arange(257))
    k = np.empty(lam.size, dtype=np.int64)
    for v in range(256):
        idx = order[bounds[v]:bounds[v + 1]]
        k[idx] = np.searchsorted(table[v], u[idx], side="right")
    k = np.minimum(k, POISSON_KMAX)
    return (k & 255).astype(np.uint8).reshape(clean_u8.shape)


def _mulhi64(z: np.ndarray, m: int) -> np.ndarray:
    """floor(z*m / 2^64) for uint64 z and 0 <= m < 2^32, exact (32-bit halves)."""
    assert 0 <= m < 2 ** 32
    mm = np.uint64(m)
    lo = (z & np.uint64(0xFFFFFFFF)) * mm
    hi = (z >> np.uint64(32)) * mm
    return (hi + (lo >> np.uint64(32))) >> np.uint64(32)


def _hash_u64(seed: int, stream: int, n: int) -> np.ndarray:
    """The full 64-bit draws z_j = splitmix64(splitmix64(seed ^ stream) + j), j < n (hash_uniform's integers)."""
    base = splitmix64(np.array([(seed ^ stream) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))[0]
    with np.errstate(over="ignore"):
        return splitmix64(base + np.arange(n, dtype=np.uint64))


def salt_pepper_coords(h: int, w: int, salt_prob: float = 0.02, pepper_prob: float = 0.02, seed: int = NOISE_SEED,
                       index: int = 0):
    """((salt_rows, salt_cols), (pepper_rows, pepper_cols)) of the image with global index `index`: n = int(float(h*w*3)*prob)
    draws each, row = floor(z*(h-1) / 2^64), col = floor(z*(w-1) / 2^64) (numpy's randint(0, h-1): the last row and column are
    never hit)."""
    if h < 2 or w < 2:
        raise ValueError(f"salt_pepper needs H, W >= 2 (numpy's randint(0, i-1) raises high <= low), got {h}x{w}")
    per = h * w * 3
    sr, sc, pr, pc = NOISE_STREAMS["salt_pepper"]
    s = seed + index
    out = []
    for prob, (rs, cs) in ((salt_prob, (sr, sc)), (pepper_prob, (pr, pc))):
        k = int(float(per) * prob)
        out.append((_mulhi64(_hash_u64(s, rs, k), h - 1).astype(np.int64), _mulhi64(_hash_u64(s, cs, k), w - 1).astype(np.int64)))
    return tuple(out)


def add_salt_pepper_noise(clean_u8: np.ndarray, salt_prob: float = 0.02, pepper_prob: float = 0.02, seed: int = NOISE_SEED,
                          first_index: int = 0) -> np.ndarray:
    """noise_generation.py:12-22: int(float(H*W*3)*prob) salt draws set all 3 channels of their pixel to 255, then as many pepper
    draws set theirs to 0 (pepper wins a collision).  The reference's third, channel coordinate is drawn but unused, so it is not
    drawn here."""
    n, h, w = clean_u8.shape[:3]
    out = clean_u8.copy()
    for i in range(n):
        (sr, sc), (pr, pc) = salt_pepper_coords(h, w, salt_prob, pepper_prob, seed, first_index + i)
        out[i, sr, sc, :] = 255
        out[i, pr, pc, :] = 0
    return out


def add_noise_np(clean_u8: np.ndarray, kind: str, seed: int = NOISE_SEED, first_index: int = 0, **params) -> np.ndarray:
    """uint8 [N,H,W,3] -> the same with `kind` noise (one of NOISE_TYPES, the reference's keyword names and defaults): the CPU
    restatement of noise.add_noise / cid_add_noise.  With kind="gaussian" and mean 0 this is add_gaussian_noise bit for bit."""
    if kind not in NOISE_DEFAULTS:
        raise ValueError(f"unknown noise kind {kind!r}; expected one of {NOISE_TYPES}")
    unknown = set(params) - set(NOISE_DEFAULTS[kind])
    if unknown:
        raise TypeError(f"unknown parameter(s) {sorted(unknown)} for {kind!r} noise; expected {sorted(NOISE_DEFAULTS[kind])}")
    clean_u8 = np.ascontiguousarray(clean_u8, dtype=np.uint8)
    if kind in ("gaussian", "speckle", "uniform"):
        return _clip_u8(noise_values_np(clean_u8, kind, seed, first_index, **params))
    if kind == "poisson":
        return add_poisson_noise(clean_u8, seed, first_index)
    return add_salt_pepper_noise(clean_u8, seed=seed, first_index=first_index, **params)


def adam_step_np(p, g, m, v, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """One torch.optim.Adam update (default flags: no amsgrad, no maximize, L2 weight decay) of one fp32 tensor -> (p', m', v'):
    the CPU restatement of k_adam_step / cid_adam_step, the expression tree of include/cid.h in float64 with one rounding to
    float32 per stored value.  `t` is the tensor's step number including this update (>= 1).  The inputs are not modified."""
    t = int(t)
    if t < 1:
        raise ValueError("adam_step_np: t counts this update, so it is at least 1")
    lr, beta1, beta2, eps, weight_decay = float(lr), float(beta1), float(beta2), float(eps), float(weight_decay)
    p64, m64, v64 = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (p, m, v))
    g64 = np.asarray(g, dtype=np.float32).astype(np.float64)
    if weight_decay != 0.0:
        g64 = g64 + weight_decay * p64
    m1 = (m64 * beta1 + (1.0 - beta1) * g64).astype(np.float32)
    v1 = (v64 * beta2 + ((1.0 - beta2) * g64) * g64).astype(np.float32)
    bc1 = 1.0 - math.pow(beta1, float(t))
    bc2 = 1.0 - math.pow(beta2, float(t))
    denom = np.sqrt(v1.astype(np.float64)) / math.sqrt(bc2) + eps
    p1 = (p64 - (lr / bc1) * (m1.astype(np.float64) / denom)).astype(np.float32)
    return p1, m1, v1


def _resize_cubic(t: np.ndarray) -> np.ndarray:
    """Pillow's bicubic filter (a = -0.5) in its evaluation order, float64."""
    a = -0.5
    t = np.abs(t)
    inner = ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0
    outer = (((t - 5.0) * t + 8.0) * t - 4.0) * a
    return np.where(t < 1.0, inner, np.where(t < 2.0, outer, 0.0))


def resize_tables_np(in_size: int, out_size: int):
    """(ksize, bounds int32 [out, 2] = (xmin, n), coeffs int32 [out, ksize]) of one axis of the bicubic resize: the CPU restatement
    of cid_resize_plan_table — the arithmetic of include/cid.h (Pillow's precompute_coeffs + normalize_coeffs_8bpc) in float64,
    every operation rounded on its own (numpy does not contract), casts truncating, the weights summed in index order."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("resize_tables_np: sizes must be >= 1")
    scale = float(in_size) / float(out_size)
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # astype truncates toward zero, like the C cast
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    live = x < n[:, None]
    w = _resize_cubic(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * (1.0 / fs))
    w = np.where(live, w, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for k in range(ksize):                                                   # w[0] + w[1] + ... in that order (np.sum is pairwise)
        ww = ww + w[:, k]
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    fixed = np.where(w < 0.0, -0.5 + w * 4194304.0, 0.5 + w * 4194304.0).astype(np.int64)
    coeffs = np.where(live, fixed, 0).astype(np.int32)
    bounds = np.stack([xmin, n], axis=1).astype(np.int32)
    return ksize, bounds, coeffs


def _resize_pass_np(img: np.ndarray, axis: int, out_size: int) -> np.ndarray:
    """One pass of the resize over `axis` of a uint8 [N,H,W,3] array: clamp((2^21 + sum in * k) >> 22, 0, 255) in integers."""
    in_size = img.shape[axis]
    ksize, bounds, coeffs = resize_tables_np(in_size, out_size)
    src = np.moveaxis(img, axis, -1).astype(np.int64)                        # [..., in]
    acc = np.full(src.shape[:-1] + (out_size,), 1 << 21, dtype=np.int64)
    for k in range(ksize):
        idx = np.minimum(bounds[:, 0].astype(np.int64) + k, in_size - 1)     # past n the coefficient is 0
        acc += src[..., idx] * coeffs[:, k].astype(np.int64)
    out = np.clip(acc >> 22, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.moveaxis(out, -1, axis))


def resize_bicubic_np(img_u8: np.ndarray, size) -> np.ndarray:
    """uint8 [H,W,3] or [N,H,W,3] -> the same resized to size = (width, height) as PIL's Image.resize(size, resample=BICUBIC)
    does, byte for byte, without PIL: the CPU restatement of resize.resize / cid_resize.  Horizontal pass first (if the width
    changes) into a uint8 intermediate, vertical pass second (if the height changes); a pass whose axis keeps its size is
    skipped."""
    img = np.ascontiguousarray(img_u8, dtype=np.uint8)
    single = img.ndim == 3
    if single:
        img = img[None]
    if img.ndim != 4 or img.shape[3] != 3:
        raise ValueError("resize_bicubic_np expects uint8 [H,W,3] or [N,H,W,3]")
    wd, hd = int(size[0]), int(size[1])
    if img.shape[2] != wd:
        img = _resize_pass_np(img, 2, wd)
    if img.shape[1] != hd:
        img = _resize_pass_np(img, 1, hd)
    if np.shares_memory(img, img_u8):                                        # neither pass ran: the result is a copy
        img = img.copy()
    return img[0] if single else img


# ---- the server's ESRGANGenerator (backend/app.py:188-218): parameter shapes and synthetic weights ----

def esrgan_param_shapes(num_residuals: int = 8) -> "OrderedDict[str, tuple]":
    """state_dict key -> (shape, dtype name) of ESRGANGenerator(num_residuals), in the module's own order, BatchNorm buffers and
    num_batches_tracked included."""
    out: "OrderedDict[str, tuple]" = OrderedDict()
    f = "float32"
    out["initial.0.weight"] = ((64, 3, 9, 9), f)
    out["initial.0.bias"] = ((64,), f)
    out["initial.1.weight"] = ((1,), f)
    for i in range(num_residuals):
        b = f"residuals.{i}.block."
        for c in (0, 3):
            out[f"{b}{c}.weight"] = ((64, 64, 3, 3), f)
            out[f"{b}{c}.bias"] = ((64,), f)
            for k in ("weight", "bias", "running_mean", "running_var"):
                out[f"{b}{c + 1}.{k}"] = ((64,), f)
            out[f"{b}{c + 1}.num_batches_tracked"] = ((), "int64")
            if c == 0:
                out[f"{b}2.weight"] = ((1,), f)
    out["final.weight"] = ((3, 64, 9, 9), f)
    out["final.bias"] = ((3,), f)
    return out


def make_esrgan_state_dict(kind: str = "default", num_residuals: int = 8, seed: int = WEIGHT_SEED) -> "OrderedDict[str, np.ndarray]":
    """Synthetic weights keyed like the reference's ESRGANGenerator state_dict, from the hash streams.

    Convolution weights and biases are U(+-sqrt(1/fan_in)) for kind="default" and U(+-sqrt(6/fan_in)) for kind="hot"; BatchNorm
    gamma in [0.6, 1.4], beta in +-0.1, running_mean in +-0.3, running_var in [0.5, 1.5], far enough from a fresh BatchNorm that a
    swapped or unused buffer shows; PReLU slopes in [0.05, 0.45].  In "hot" the slope of initial.1 is -0.3 and that of the last
    block's PReLU 1.5 (with no block, only the first): learned slopes may leave [0, 1], which a max-form PReLU gets wrong."""
    if kind not in ("default", "hot"):
        raise ValueError(f"unknown weight set {kind!r}")
    shapes = esrgan_param_shapes(num_residuals)
    sd: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for key, (shape, dtype) in shapes.items():
        if dtype == "int64":
            sd[key] = np.array(7, dtype=np.int64)
            continue
        n = int(np.prod(shape))
        u = hash_uniform(seed, _fnv1a64("esrgan:" + kind + ":" + key), n)
        layer, leaf = key.rsplit(".", 1)
        wshape = shapes[layer + ".weight"][0]
        if len(wshape) == 4:                                   # a convolution's weight or bias
            fan_in = wshape[1] * wshape[2] * wshape[3]
            bound = math.sqrt((1.0 if kind == "default" else 6.0) / fan_in)
            v = (2.0 * u - 1.0) * bound
        elif wshape == (1,):                                   # a PReLU slope
            v = 0.05 + 0.4 * u
        elif leaf == "weight":
            v = 0.6 + 0.8 * u
        elif leaf == "bias":
            v = (2.0 * u - 1.0) * 0.1
        elif leaf == "running_mean":
            v = (2.0 * u - 1.0) * 0.3
        else:                                                  # running_var
            v = 0.5 + u
        sd[key] = v.astype(np.float32).reshape(shape)
    if kind == "hot":
        sd["initial.1.weight"][...] = -0.3
        if num_residuals > 0:
            sd[f"residuals.{num_residuals - 1}.block.2.weight"][...] = 1.5
    return sd


def esrgan_inputs_u8(n: int, h: int, w: int, first_index: int = 0) -> np.ndarray:
    """uint8 [n,h,w,3] inputs for the ESRGAN tests: the noisy face-like fields of make_batch."""
    return add_gaussian_noise(clean_images_u8(n, h, w, first_index), 25.0, first_index)


# ---- the server's SRGANGenerator (backend/app.py:145-186): parameter shapes and synthetic weights ----

def _srgan_stages(scale_factor: int) -> int:
    s = int(scale_factor)
    if s < 1 or s & (s - 1):
        raise ValueError(f"scale_factor must be a power of two (got {scale_factor})")
    return s.bit_length() - 1


def srgan_param_shapes(scale_factor: int = 4) -> "OrderedDict[str, tuple]":
    """state_dict key -> (shape, dtype name) of SRGANGenerator(scale_factor), in the module's own order, BatchNorm buffers and
    num_batches_tracked included."""
    out: "OrderedDict[str, tuple]" = OrderedDict()
    f = "float32"
    out["initial.0.weight"] = ((64, 3, 9, 9), f)
    out["initial.0.bias"] = ((64,), f)
    out["initial.1.weight"] = ((1,), f)
    for i in range(5):
        b = f"res_blocks.{i}."
        for c in (0, 3):
            out[f"{b}{c}.weight"] = ((64, 64, 3, 3), f)
            out[f"{b}{c}.bias"] = ((64,), f)
            for k in ("weight", "bias", "running_mean", "running_var"):
                out[f"{b}{c + 1}.{k}"] = ((64,), f)
            out[f"{b}{c + 1}.num_batches_tracked"] = ((), "int64")
            if c == 0:
                out[f"{b}2.weight"] = ((1,), f)
    out["mid.weight"] = ((64, 64, 3, 3), f)
    out["mid.bias"] = ((64,), f)
    for u in range(_srgan_stages(scale_factor)):
        out[f"upscale.{3 * u}.weight"] = ((256, 64, 3, 3), f)
        out[f"upscale.{3 * u}.bias"] = ((256,), f)
        out[f"upscale.{3 * u + 2}.weight"] = ((1,), f)
    out["final.weight"] = ((3, 64, 9, 9), f)
    out["final.bias"] = ((3,), f)
    return out


def make_srgan_state_dict(kind: str = "default", scale_factor: int = 4, seed: int = WEIGHT_SEED) -> "OrderedDict[str, np.ndarray]":
    """Synthetic weights keyed like the reference's SRGANGenerator state_dict, from the hash streams "srgan:<kind>:<key>", with the
    distributions of make_esrgan_state_dict: convolutions U(+-sqrt(g/fan_in)), g = 1 for "default" and 6 for "hot"; BatchNorm gamma
    in [0.6, 1.4], beta in +-0.1, running_mean in +-0.3, running_var in [0.5, 1.5]; PReLU slopes in [0.05, 0.45].  In "hot" the
    slope of initial.1 is -0.3, that of the last block's PReLU (res_blocks.4.2) 1.5 and that of the first upscale stage -0.3."""
    if kind not in ("default", "hot"):
        raise ValueError(f"unknown weight set {kind!r}")
    shapes = srgan_param_shapes(scale_factor)
    sd: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for key, (shape, dtype) in shapes.items():
        if dtype == "int64":
            sd[key] = np.array(7, dtype=np.int64)
            continue
        n = int(np.prod(shape))
        u = hash_uniform(seed, _fnv1a64("srgan:" + kind + ":" + key), n)
        layer, leaf = key.rsplit(".", 1)
        wshape = shapes[layer + ".weight"][0]
        if len(wshape) == 4:                                   # a convolution's weight or bias
            fan_in = wshape[1] * wshape[2] * wshape[3]
            bound = math.sqrt((1.0 if kind == "default" else 6.0) / fan_in)
            v = (2.0 * u - 1.0) * bound
        elif wshape == (1,):                                   # a PReLU slope
            v = 0.05 + 0.4 * u
        elif leaf == "weight":
            v = 0.6 + 0.8 * u
        elif leaf == "bias":
            v = (2.0 * u - 1.0) * 0.1
        elif leaf == "running_mean":
            v = (2.0 * u - 1.0) * 0.3
        else:                                                  # running_var
            v = 0.5 + u
        sd[key] = v.astype(np.float32).reshape(shape)
    if kind == "hot":
        sd["initial.1.weight"][...] = -0.3
        sd["res_blocks.4.2.weight"][...] = 1.5
        if "upscale.2.weight" in sd:
            sd["upscale.2.weight"][...] = -0.3
    return sd


SRGAN_DISC_CONVS = ((0, 3, 64, 3), (2, 64, 64, 3), (5, 64, 128, 3), (8, 128, 128, 3), (11, 128, 256, 3), (15, 256, 512, 1), (17, 512, 1, 1))
SRGAN_DISC_BNS = ((3, 64), (6, 128), (9, 128), (12, 256))


def srgan_disc_param_shapes() -> "OrderedDict[str, tuple]":
    """state_dict key -> (shape, dtype name) of SRGANDiscriminator, in the module's own order, BatchNorm buffers and
    num_batches_tracked included."""
    layers = {i: ("conv", (cin, cout, k)) for i, cin, cout, k in SRGAN_DISC_CONVS}
    layers.update({i: ("bn", c) for i, c in SRGAN_DISC_BNS})
    out: "OrderedDict[str, tuple]" = OrderedDict()
    f = "float32"
    for i in sorted(layers):
        what, d = layers[i]
        if what == "conv":
            out[f"model.{i}.weight"] = ((d[1], d[0], d[2], d[2]), f)
            out[f"model.{i}.bias"] = ((d[1],), f)
        else:
            for k in ("weight", "bias", "running_mean", "running_var"):
                out[f"model.{i}.{k}"] = ((d,), f)
            out[f"model.{i}.num_batches_tracked"] = ((), "int64")
    return out


def make_srgan_disc_state_dict(kind: str = "default", seed: int = WEIGHT_SEED) -> "OrderedDict[str, np.ndarray]":
    """Synthetic weights keyed like the reference's SRGANDiscriminator state_dict, from the hash streams "srgan_disc:<kind>:<key>":
    convolution weights and biases U(+-1/sqrt(fan_in)), the scale of PyTorch's default Conv2d initialisation.
    kind="default": fresh BatchNorms (gamma 1, beta 0, running_mean 0, running_var 1, num_batches_tracked 0).
    kind="trained": BatchNorm values far from those, so that a swapped or unused pointer shows: gamma in [0.5, 1.5], beta in +-0.3,
        running_mean in +-0.2, running_var in [0.2, 3.0], num_batches_tracked 7."""
    if kind not in ("default", "trained"):
        raise ValueError(f"unknown weight set {kind!r}")
    shapes = srgan_disc_param_shapes()
    sd: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for key, (shape, dtype) in shapes.items():
        if dtype == "int64":
            sd[key] = np.array(7 if kind == "trained" else 0, dtype=np.int64)
            continue
        n = int(np.prod(shape))
        u = hash_uniform(seed, _fnv1a64("srgan_disc:" + kind + ":" + key), n)
        layer, leaf = key.rsplit(".", 1)
        wshape = shapes[layer + ".weight"][0]
        if len(wshape) == 4:
            v = (2.0 * u - 1.0) / math.sqrt(wshape[1] * wshape[2] * wshape[3])
        elif kind == "default":
            v = np.full(n, 1.0 if leaf in ("weight", "running_var") else 0.0)
        elif leaf == "weight":
            v = 0.5 + u
        elif leaf == "bias":
            v = (2.0 * u - 1.0) * 0.3
        elif leaf == "running_mean":
            v = (2.0 * u - 1.0) * 0.2
        else:                                                  # running_var
            v = 0.2 + 2.8 * u
        sd[key] = np.asarray(v).astype(np.float32).reshape(shape)
    return sd


def srgan_inputs_u8(n: int, h: int, w: int, first_index: int = 0) -> np.ndarray:
    """uint8 [n,h,w,3] inputs for the SRGAN tests: the noisy face-like fields of make_batch."""
    return add_gaussian_noise(clean_images_u8(n, h, w, first_index), 25.0, first_index)


# ---- the ESRGAN trainer's Discriminator (backend/trainingcode/esrgan_code/models.py:36-71) ----

ESRGAN_DISC_CONVS = (("conv1", 3, 64), ("conv2", 64, 128), ("conv3", 128, 256), ("conv4", 256, 512))
ESRGAN_DISC_TRAINED_CONV_GAIN = 1.5    # "trained": conv weights U(+-gain / sqrt(fan_in)), biases U(+-0.05)
ESRGAN_DISC_TRAINED_FC_GAIN = 12.0     # "trained": fc.weight U(+-gain / sqrt(features)), fc.bias 0.25


def esrgan_disc_param_shapes(input_shape=(3, 256, 256)) -> "OrderedDict[str, tuple]":
    """state_dict key -> (shape, dtype name) of the ESRGAN Discriminator(input_shape), in the module's own order.  No buffers."""
    h, w = int(input_shape[1]), int(input_shape[2])
    out: "OrderedDict[str, tuple]" = OrderedDict()
    for name, cin, cout in ESRGAN_DISC_CONVS:
        out[name + ".weight"] = ((cout, cin, 3, 3), "float32")
        out[name + ".bias"] = ((cout,), "float32")
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out["fc.weight"] = ((1, 512 * h * w), "float32")
    out["fc.bias"] = ((1,), "float32")
    return out


def make_esrgan_disc_state_dict(kind: str = "default", input_shape=(3, 256, 256), seed: int = WEIGHT_SEED) -> "OrderedDict[str, np.ndarray]":
    """Synthetic weights keyed like the reference's ESRGAN Discriminator state_dict, from the hash streams "esrgan_disc:<kind>:<key>".
    kind="default": every tensor U(+-1/sqrt(fan_in)), the scale of PyTorch's default Conv2d / Linear initialisation; four such layers
        shrink the signal, so the logits stay within a few hundredths of fc.bias.
    kind="trained": convolution weights 1.5 times that with biases U(+-0.05), and fc.weight U(+-12/sqrt(features)) with fc.bias 0.25:
        the logits of the noisy face-like test images differ from image to image and stay within about +-1.5 at every input size (well
        inside +-4), so BCE-with-logits runs on its curved part, not on its asymptotes, and the fc gain does not amplify the float32
        rounding of conv4's output beyond what the parity bound leaves."""
    if kind not in ("default", "trained"):
        raise ValueError(f"unknown weight set {kind!r}")
    sd: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for key, (shape, _) in esrgan_disc_param_shapes(input_shape).items():
        n = int(np.prod(shape))
        u = 2.0 * hash_uniform(seed, _fnv1a64("esrgan_disc:" + kind + ":" + key), n) - 1.0
        layer, leaf = key.rsplit(".", 1)
        fan_in = n if key == "fc.weight" else int(np.prod(esrgan_disc_param_shapes(input_shape)[layer + ".weight"][0][1:]))
        v = u / math.sqrt(fan_in)
        if kind == "trained":
            if layer == "fc":
                v = u * ESRGAN_DISC_TRAINED_FC_GAIN / math.sqrt(fan_in) if leaf == "weight" else np.full(n, 0.25)
            else:
                v = u * ESRGAN_DISC_TRAINED_CONV_GAIN / math.sqrt(fan_in) if leaf == "weight" else u * 0.05
        sd[key] = np.asarray(v).astype(np.float32).reshape(shape)
    return sd


# ---- the server's CGANGenerator (backend/app.py:105-143): parameter shapes, synthetic weights and the latent's streams ----

CGAN_LATENT_DIM = 100
CGAN_Z_STREAMS = (_fnv1a64("cgan:z:u1"), _fnv1a64("cgan:z:u2"))   # u1, u2 of the latent's Box-Muller (cid_cg_latent)
CGAN_HOT_GAIN = 14.0


def cgan_param_shapes(n_classes: int = 10) -> "OrderedDict[str, tuple]":
    """state_dict key -> (shape, dtype name) of CGANGenerator(n_classes), in the module's own order, BatchNorm buffers and
    num_batches_tracked included.  ConvTranspose2d weights are [Cin, Cout, 4, 4]."""
    if int(n_classes) < 1:
        raise ValueError(f"n_classes must be positive (got {n_classes})")
    out: "OrderedDict[str, tuple]" = OrderedDict()
    f = "float32"

    def bn(i, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            out[f"model.{i}.{k}"] = ((c,), f)
        out[f"model.{i}.num_batches_tracked"] = ((), "int64")

    out["label_emb.weight"] = ((int(n_classes), CGAN_LATENT_DIM), f)
    out["l1.weight"] = ((8192, 2 * CGAN_LATENT_DIM), f)
    out["l1.bias"] = ((8192,), f)
    bn(0, 128)
    for i, cin, cout in ((2, 128, 128), (5, 128, 64), (8, 64, 32)):
        out[f"model.{i}.weight"] = ((cin, cout, 4, 4), f)
        out[f"model.{i}.bias"] = ((cout,), f)
        bn(i + 1, cout)
    out["model.11.weight"] = ((3, 32, 3, 3), f)
    out["model.11.bias"] = ((3,), f)
    return out


def make_cgan_state_dict(kind: str = "default", n_classes: int = 10, seed: int = WEIGHT_SEED) -> "OrderedDict[str, np.ndarray]":
    """Synthetic weights keyed like the reference's CGANGenerator state_dict, from the hash streams "cgan:<kind>:<key>".
    "default" has the scale of PyTorch's initialisation: linear and convolutions U(+-1/sqrt(fan_in)) with torch's fan_in rule
    (shape[1] * kernel area, also for ConvTranspose2d), the embedding Box-Muller N(0, 1), BatchNorm gamma 1, beta 0, running_mean 0,
    running_var 1.  "hot": linear and convolutions U(+-sqrt(g/fan_in)) with g = CGAN_HOT_GAIN, which saturates tanh in part of the
    output; BatchNorm gamma in [0.6, 1.4], beta in +-0.1, running_mean in +-0.3, running_var in [0.5, 1.5]."""
    if kind not in ("default", "hot"):
        raise ValueError(f"unknown weight set {kind!r}")
    shapes = cgan_param_shapes(n_classes)
    sd: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for key, (shape, dtype) in shapes.items():
        if dtype == "int64":
            sd[key] = np.array(7, dtype=np.int64)
            continue
        n = int(np.prod(shape))
        stream = _fnv1a64("cgan:" + kind + ":" + key)
        u = hash_uniform(seed, stream, n)
        layer, leaf = key.rsplit(".", 1)
        wshape = shapes[layer + ".weight"][0]
        if key == "label_emb.weight":
            v = _box_muller(u, hash_uniform(seed, _fnv1a64("cgan:" + kind + ":" + key + ":u2"), n))
        elif len(wshape) >= 2:                                 # the linear's or a convolution's weight or bias
            fan_in = int(np.prod(wshape[1:]))
            bound = math.sqrt((1.0 if kind == "default" else CGAN_HOT_GAIN) / fan_in)
            v = (2.0 * u - 1.0) * bound
        elif kind == "default":                                # BatchNorm as constructed
            v = np.full(n, 1.0 if leaf in ("weight", "running_var") else 0.0)
        elif leaf == "weight":
            v = 0.6 + 0.8 * u
        elif leaf == "bias":
            v = (2.0 * u - 1.0) * 0.1
        elif leaf == "running_mean":
            v = (2.0 * u - 1.0) * 0.3
        else:                                                  # running_var
            v = 0.5 + u
        sd[key] = v.astype(np.float32).reshape(shape)
    return sd


def cgan_latent_np(n: int, seed: int, first_index: int = 0) -> np.ndarray:
    """fp32 [n,100]: row i is Box-Muller in float64 of the two streams CGAN_Z_STREAMS under seed (seed + first_index + i), rounded to
    fp32: the restatement of cid_cg_latent.  A row depends on (seed + first_index + i) alone."""
    z = _box_muller(_image_uniforms(seed, first_index, n, CGAN_Z_STREAMS[0], CGAN_LATENT_DIM),
                    _image_uniforms(seed, first_index, n, CGAN_Z_STREAMS[1], CGAN_LATENT_DIM))
    return z.astype(np.float32)


# ---- LPIPS(net='alex') (include/cid.h, cid_lpips): portable synthetic weights ----
LPIPS_CHANNELS = (64, 192, 384, 256, 256)
LPIPS_SHIFT = (-.030, -.088, -.188)
LPIPS_SCALE = (.458, .448, .450)
LPIPS_VGG_CHANNELS = (64, 128, 256, 512, 512)
# (slice, torchvision vgg16.features index, Cin, Cout, kernel)
LPIPS_VGG_CONVS = ((1, 0, 3, 64, 3), (1, 2, 64, 64, 3), (2, 5, 64, 128, 3), (2, 7, 128, 128, 3), (3, 10, 128, 256, 3), (3, 12, 256, 256, 3),
                   (3, 14, 256, 256, 3), (4, 17, 256, 512, 3), (4, 19, 512, 512, 3), (4, 21, 512, 512, 3), (5, 24, 512, 512, 3),
                   (5, 26, 512, 512, 3), (5, 28, 512, 512, 3))


def lpips_param_shapes(net: str = "alex") -> "OrderedDict[str, tuple]":
    """state_dict key -> shape of lpips.LPIPS(net=net) in the module's own order, the lins.* aliases of lin* last."""
    if net not in ("alex", "vgg"):
        raise ValueError(f"unknown net {net!r}")
    out: "OrderedDict[str, tuple]" = OrderedDict()
    out["scaling_layer.shift"] = (1, 3, 1, 1)
    out["scaling_layer.scale"] = (1, 3, 1, 1)
    convs = LPIPS_VGG_CONVS if net == "vgg" else ((1, 0, 3, 64, 11), (2, 3, 64, 192, 5), (3, 6, 192, 384, 3), (4, 8, 384, 256, 3), (5, 10, 256, 256, 3))
    channels = LPIPS_VGG_CHANNELS if net == "vgg" else LPIPS_CHANNELS
    for k, idx, cin, cout, ks in convs:
        out[f"net.slice{k}.{idx}.weight"] = (cout, cin, ks, ks)
        out[f"net.slice{k}.{idx}.bias"] = (cout,)
    for k, c in enumerate(channels):
        out[f"lin{k}.model.1.weight"] = (1, c, 1, 1)
    for k, c in enumerate(channels):
        out[f"lins.{k}.model.1.weight"] = (1, c, 1, 1)
    return out


def make_lpips_state_dict(kind: str = "default", seed: int = WEIGHT_SEED, net: str = "alex") -> "OrderedDict[str, np.ndarray]":
    """Synthetic weights keyed like lpips.LPIPS(net=net), from the hash streams "lpips:<kind>:<key>" (net="alex") or
    "lpips_vgg:<kind>:<key>" (net="vgg").  No pretrained weights ship
    with this package; these keep the activations alive through the ReLUs so that every tap carries signal.
    Convolutions are He-uniform, U(+-sqrt(6 / fan_in)); biases U(+-0.05) ("default") or U(+-0.5) ("hot", which also doubles the
    weights' gain: larger, sparser activations).  lin weights are non-negative, u / sum(u) * (1 + 0.25 (2 v - 1)) per layer: they sum
    to about 1.  shift / scale are the package's constants.  lins.* repeat lin*."""
    if kind not in ("default", "hot"):
        raise ValueError(f"unknown weight set {kind!r}")
    stream = ("lpips_vgg:" if net == "vgg" else "lpips:") + kind + ":"
    sd: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for key, shape in lpips_param_shapes(net).items():
        n = int(np.prod(shape))
        if key == "scaling_layer.shift":
            v = np.array(LPIPS_SHIFT)
        elif key == "scaling_layer.scale":
            v = np.array(LPIPS_SCALE)
        elif key.startswith("lins."):
            sd[key] = sd["lin" + key[len("lins."):]]
            continue
        else:
            u = hash_uniform(seed, _fnv1a64(stream + key), n)
            if key.startswith("lin"):
                g = hash_uniform(seed, _fnv1a64(stream + key + ":gain"), 1)[0]
                v = u / u.sum() * (1.0 + 0.25 * (2.0 * g - 1.0))
            elif key.endswith(".weight"):
                fan_in = shape[1] * shape[2] * shape[3]
                v = (2.0 * u - 1.0) * math.sqrt((6.0 if kind == "default" else 12.0) / fan_in)
            else:
                v = (2.0 * u - 1.0) * (0.05 if kind == "default" else 0.5)
        sd[key] = v.astype(np.float32).reshape(shape)
    return sd


def vgg_loss_state_dict(lpips_vgg_sd) -> "OrderedDict[str, np.ndarray]":
    """The reference VGGPerceptualLoss's state dict (slice.N.*) cut from a make_lpips_state_dict(net="vgg") one: slice1 ... slice3."""
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for k, idx, *_ in LPIPS_VGG_CONVS[:7]:
        for leaf in ("weight", "bias"):
            out[f"slice.{idx}.{leaf}"] = lpips_vgg_sd[f"net.slice{k}.{idx}.{leaf}"]
    return out
