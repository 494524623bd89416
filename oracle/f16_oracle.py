"""TEST INFRASTRUCTURE — an arithmetic model of the fp16-storage forward (compute_dtype="f16", BASELINE configs[4]), launch by launch.

Comparing the path's final output with an emulation of it cannot be tight: one rounding flip in an early layer cascades through the
eleven roundings to half that follow it.  What CAN be checked tightly is each launch on its own, fed with the tensors the GPU itself
stored: every launch of the path writes a region of the arena of its own, so after one forward all of them can be read back.

What the kernels compute (csrc/conv_kernels_f16.h, csrc/cid_api.hip), and what this module models:
  head      k_conv_head_h16   the network input to half (u8: half((u8/255.f - 0.5f)/0.5f) in fp32; the caller's padding band -1, outside the
                              network input the convolution's zero padding), weights to half, 27 products on one MFMA in fp32, + fp32 bias, ReLU,
                              ONE rounding to half at the store
  3x3       k_conv3x3_h16     half operands, fp32 accumulators over CIN x 9 products, + fp32 bias, ReLU, one rounding at the store.  The pooling
                              launches (down1.2, down2.2) also store the 2x2 max-pool of the fp32 values (+ bias, ReLU) over the COMPUTED region
                              2 (H/2) x 2 (W/2), rounded once; the full-size tensor is stored only over the top-left crop the concat keeps
  convT     k_convt_t16       CIN products per output pixel (one tap), + fp32 bias, no ReLU, rounded once, into the concat's channel slice
  fused     k_conv3x3_h16<ZOUT>  the operand is half(relu(acc + b)), the same value the unfused kernel stores; z[3 tap + co] =
                              half(sum_ci a * half(W2)) (fp32 accumulation of 64 products); k_conv_tail_zh then sums bias + the nine taps'
                              z in fp32, in tap order (zero outside the image), and applies tanhf
  tiles     k_conv_tail_h     fp32 accumulation of 576 half products per output + bias, tanhf

Rounding model.  half() is IEEE round-to-nearest-even with SUBNORMALS KEPT: the library is built without fast-math or denormal
flushing, so the fp16/fp64 denormal mode of its kernels is "preserve" and v_cvt_f16_f32 (what (_Float16)x compiles to) rounds into
the subnormal range like torch's float -> half conversion.  The GPU rounds fp32 values, so half() takes its argument to fp32 first
(which is also what torch does for a float64 tensor).

Bound.  For a stored value v = fl32(sum of K exact half products, + bias), |v - ref| <= B with
    B = c * K * 2^-24 * (|W| * |X|) + 2^-24 * |b|        (K = the number of fp32 additions, the bias add included)
which holds for ANY order of summation (fp32 recursive summation; half x half products are exact in fp32).  C_ACC = c = 1: the
guides do not document how the f16 MFMA accumulates inside one instruction; a larger c needs a recorded measurement.  ReLU, max-pool
and rounding to half are monotone, so the stored element must lie in [half(post(ref - B)), half(post(ref + B))].

Only tests/ and csrc/tools may import this module; the shipped package never does.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24            # unit roundoff of fp32
C_ACC = 1.0               # c of the bound
TANH_ABS = 4 * U          # tanhf's error allowance on outputs in (-1, 1): a few fp32 ulps
LAUNCHES = ("down1.0", "down1.2", "down2.0", "down2.2", "bottleneck.0", "bottleneck.2", "up2", "upconv2.0", "upconv2.2", "up1",
            "upconv1.0", "upconv1.2")


# ------------------------------------------------------------------ rounding
def half(t: torch.Tensor) -> torch.Tensor:
    """fp32 -> IEEE half, round to nearest even, subnormals kept; returned as float64 (exact)."""
    return t.to(torch.float32).to(torch.float16).to(torch.float64)


def half_rtz(t: torch.Tensor) -> torch.Tensor:
    """fp32 -> half rounded toward zero (mutation testing only)."""
    t32 = t.to(torch.float32)
    h = t32.to(torch.float16)
    away = h.to(torch.float32).abs() > t32.abs()
    bits = h.view(torch.int16)
    bits = torch.where(away, bits - 1, bits)            # one ulp toward zero on the magnitude (sign-magnitude format)
    return bits.view(torch.float16).to(torch.float64)


def _ordered(h: torch.Tensor) -> torch.Tensor:
    """half values -> integers that are consecutive for consecutive halfs (+0 and -0 both 0)."""
    b = h.to(torch.float16).view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(b >= 0x8000, -(b - 0x8000), b)


def ulp_distance(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """|a - b| in units of half ulps (both half-valued)."""
    return (_ordered(a) - _ordered(b)).abs()


def _t(sd, key) -> torch.Tensor:
    v = sd[key]
    if isinstance(v, np.ndarray):
        v = torch.from_numpy(np.ascontiguousarray(v))
    return v.detach().to("cpu", torch.float64)


# ------------------------------------------------------------------ network input of the head
def network_input(x, in_u8: bool = False, padding=(0, 0, 0, 0)) -> torch.Tensor:
    """What k_conv_head_h16 rounds to half: the caller's batch (fp32 NCHW, or u8 NHWC normalised in fp32 as the kernel does) inside a
    band of -1 (the black the server pads with, cid_forward_padded; padding = (left, top, right, bottom)).  float64 NCHW, not yet half."""
    x = torch.as_tensor(x)
    if in_u8:
        x = ((x.permute(0, 3, 1, 2).to(torch.float32) / 255.0 - 0.5) / 0.5)
    x = x.to(torch.float32)
    left, top, right, bottom = padding
    if left or top or right or bottom:
        x = F.pad(x, (left, right, top, bottom), value=-1.0)
    return x.to(torch.float64)


# ------------------------------------------------------------------ per-launch references
def _mag(fn, x, w, k):
    """|W| * |X| as an upper bound: computed in fp32 (all terms >= 0, relative error <= k u), then inflated by (1 + 2 k u)."""
    return fn(x.abs().float(), w.abs().float()).double() * (1.0 + 2 * k * U)


def launch_ref(kind: str, x: torch.Tensor, w: torch.Tensor = None, b: torch.Tensor = None, c: float = C_ACC):
    """One launch, given the (half-valued) tensors it read: -> (ref, B), the float64 value before the launch's rounding (and before
    its ReLU / pool) and the bound on the fp32 arithmetic's distance from it.  `w` / `b` are the layer's fp32 parameters (rounded
    to half here as the packing does).
      kind "conv3x3" (head, the eight 3x3 layers, the tiled tail's pre-tanh sum): x [N,CIN,H,W] -> [N,COUT,H,W], K = 9 CIN
      kind "convt": x [N,CIN,h,w] -> [N,COUT,2h,2w], K = CIN
      kind "z": x = upconv1[0]'s activations [N,64,H,W], w = upconv1[2].weight -> z [N,27,H,W] (row 3 tap + co), K = 64, no bias
      kind "zsum": x = z [N,27,H,W] (half-valued), b = upconv1[2].bias -> pre-tanh [N,3,H,W], K = 9"""
    x = x.to(torch.float64)
    if kind == "zsum":
        zp = F.pad(x, (1, 1, 1, 1))
        n, _, hh, ww = x.shape
        ref = b.to(torch.float64).view(1, 3, 1, 1).expand(n, 3, hh, ww).clone()
        mag = ref.abs().clone()
        for tap in range(9):
            ky, kx = divmod(tap, 3)
            sl = zp[:, 3 * tap:3 * tap + 3, ky:ky + hh, kx:kx + ww]
            ref = ref + sl
            mag = mag + sl.abs()
        return ref, c * 9 * U * mag
    wh = half(w.to(torch.float64))
    if kind == "z":
        wz = wh.permute(2, 3, 0, 1).reshape(27, 64)                 # row 3 (3 kh + kw) + co
        ref = torch.einsum("nchw,rc->nrhw", x, wz)
        mag = torch.einsum("nchw,rc->nrhw", x.abs().float(), wz.abs().float()).double() * (1.0 + 2 * 64 * U)
        return ref, c * 64 * U * mag
    bb = b.to(torch.float64)
    if kind == "conv3x3":
        k = 9 * x.shape[1]
        ref = F.conv2d(x, wh, bb, padding=1)
        mag = _mag(lambda a, v: F.conv2d(a, v, padding=1), x, wh, k)
    elif kind == "convt":
        k = x.shape[1]
        ref = F.conv_transpose2d(x, wh, bb, stride=2)
        mag = _mag(lambda a, v: F.conv_transpose2d(a, v, stride=2), x, wh, k)
    else:
        raise ValueError(kind)
    return ref, c * k * U * mag + U * bb.abs().view(1, -1, 1, 1)


# ------------------------------------------------------------------ checks
@dataclass
class Report:
    launch: str
    elements: int = 0
    violations: int = 0
    where: list = field(default_factory=list)     # up to 8 (n, c, y, x) of violating elements
    exact: float = 1.0                            # fraction equal to half(post(ref)) (fp32 outputs: within TANH_ABS of tanh(ref))
    worst_ulp: int = 0                            # worst distance from half(post(ref)) in half ulps (fp32 outputs: worst |err| / (B + TANH_ABS))
    not_half: int = 0                             # elements that are not half values at all

    def merge(self, o: "Report") -> "Report":
        n = self.elements + o.elements
        ex = (self.exact * self.elements + o.exact * o.elements) / max(n, 1)
        return Report(self.launch, n, self.violations + o.violations, (self.where + o.where)[:8], ex,
                      max(self.worst_ulp, o.worst_ulp), self.not_half + o.not_half)

    @property
    def ok(self) -> bool:
        return self.violations == 0 and self.not_half == 0

    def line(self) -> str:
        return (f"{self.launch:<14} n={self.elements:>10} violations={self.violations:<6} not_half={self.not_half:<5} "
                f"exact={self.exact:.5f} worst={self.worst_ulp}" + (f" first={self.where[:3]}" if self.where else ""))


def _post(t, relu):
    return t.clamp_min(0.0) if relu else t


def _maxpool(t):
    return F.max_pool2d(t, 2, 2)


def check(launch: str, got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, relu: bool = True, pool: bool = False,
          rnd=half) -> Report:
    """Every element of `got` (the GPU's stored half tensor, any float dtype, [N,C,h,w] with h, w <= ref's: a top-left crop)
    must lie in [half(post(ref - B)), half(post(ref + B))], post = the launch's ReLU (relu) after its 2x2 max-pool (pool)."""
    lo, hi, mid = ref - bound, ref + bound, ref
    if pool:
        hh, ww = 2 * (ref.shape[2] // 2), 2 * (ref.shape[3] // 2)
        lo, hi, mid = (_maxpool(t[:, :, :hh, :ww]) for t in (lo, hi, mid))
    h, w = got.shape[2], got.shape[3]
    lo, hi, mid = (rnd(_post(t[:, :, :h, :w], relu)) for t in (lo, hi, mid))
    g = got.to(torch.float64)
    r = Report(launch, g.numel())
    r.not_half = int((half(g) != g).sum())
    bad = (g < lo) | (g > hi) | (half(g) != g)
    r.violations = int(bad.sum())
    if r.violations:
        r.where = [tuple(int(v) for v in idx) for idx in bad.nonzero()[:8]]
    r.exact = float((g == mid).double().mean())
    r.worst_ulp = int(ulp_distance(half(g), mid).max()) if g.numel() else 0
    return r


def check_tanh(launch: str, got: torch.Tensor, pre: torch.Tensor, bound: torch.Tensor) -> Report:
    """The last launch's fp32 output: |got - tanh(pre)| <= B + TANH_ABS (tanh is 1-Lipschitz)."""
    g = got.to(torch.float64)
    err = (g - torch.tanh(pre)).abs()
    lim = bound + TANH_ABS
    r = Report(launch, g.numel())
    bad = err > lim
    r.violations = int(bad.sum())
    if r.violations:
        r.where = [tuple(int(v) for v in idx) for idx in bad.nonzero()[:8]]
    r.exact = float((err <= TANH_ABS).double().mean())
    r.worst_ulp = float((err / lim).max()) if g.numel() else 0.0
    return r


def z_from_groups(zg: torch.Tensor) -> torch.Tensor:
    """The fp16 fused tail's z layout [N][7][H][W][4] halfs -> [N,27,H,W] (row 3 tap + co = 4 group + slot)."""
    n, g, h, w, s = zg.shape
    assert g == 7 and s == 4
    return zg.permute(0, 1, 4, 2, 3).reshape(n, 28, h, w)[:, :27]


def check_launches(sd, x_net: torch.Tensor, st: dict, tail: str = "fused", c: float = C_ACC, act10: torch.Tensor = None,
                   rnd=half) -> "OrderedDict[str, Report]":
    """Check every launch of one forward on the tensors it stored.  x_net: network_input(...) (float64, not yet half);
    st: the stored tensors as float NCHW — "down1.0", "down1", "pool1", "down2.0", "down2", "pool2", "bottleneck.0",
    "bottleneck", "up2", "upconv2.0", "upconv2", "up1", then "upconv1.0" (tail "tiles") or "z" [N,27,Hu1,Wu1] (tail "fused"),
    and "out" (fp32 tanh output over the whole Hu1 x Wu1).  With the fused tail, upconv1[0]'s activations are never stored;
    `act10` (the same forward's "upconv1.0" under tail "tiles") lets the z check run on them, else z is not checked."""
    D = lambda k: st[k].to(torch.float64)  # noqa: E731
    P = lambda k: _t(sd, k)  # noqa: E731
    R = OrderedDict()

    def conv(name, inp, key, got, relu=True, pool_got=None, pool_name=None):
        ref, B = launch_ref("conv3x3", inp, P(key + ".weight"), P(key + ".bias"), c)
        R[name] = check(name, got, ref, B, relu=relu, rnd=rnd)
        if pool_got is not None:
            R[name] = R[name].merge(check(pool_name, pool_got, ref, B, relu=True, pool=True, rnd=rnd))
            R[name].launch = name

    conv("down1.0", half(x_net), "down1.0", D("down1.0"))
    conv("down1.2", D("down1.0"), "down1.2", D("down1"), pool_got=D("pool1"), pool_name="pool1")
    conv("down2.0", D("pool1"), "down2.0", D("down2.0"))
    conv("down2.2", D("down2.0"), "down2.2", D("down2"), pool_got=D("pool2"), pool_name="pool2")
    conv("bottleneck.0", D("pool2"), "bottleneck.0", D("bottleneck.0"))
    conv("bottleneck.2", D("bottleneck.0"), "bottleneck.2", D("bottleneck"))
    ref, B = launch_ref("convt", D("bottleneck"), P("up2.weight"), P("up2.bias"), c)
    R["up2"] = check("up2", D("up2"), ref, B, relu=False, rnd=rnd)
    conv("upconv2.0", torch.cat([D("up2"), D("down2")], 1), "upconv2.0", D("upconv2.0"))
    conv("upconv2.2", D("upconv2.0"), "upconv2.2", D("upconv2"))
    ref, B = launch_ref("convt", D("upconv2"), P("up1.weight"), P("up1.bias"), c)
    R["up1"] = check("up1", D("up1"), ref, B, relu=False, rnd=rnd)
    cat1 = torch.cat([D("up1"), D("down1")], 1)
    if tail == "tiles":
        conv("upconv1.0", cat1, "upconv1.0", D("upconv1.0"))
        pre, B = launch_ref("conv3x3", D("upconv1.0"), P("upconv1.2.weight"), P("upconv1.2.bias"), c)
    else:
        if act10 is not None:
            ref, B = launch_ref("z", act10.to(torch.float64), P("upconv1.2.weight"), None, c)
            R["upconv1.0"] = check("upconv1.0", D("z"), ref, B, relu=False, rnd=rnd)
        pre, B = launch_ref("zsum", D("z"), None, P("upconv1.2.bias"), c)
    if "out" in st:   # (a cropped output, forward_padded's, is not checked here)
        R["upconv1.2"] = check_tanh("upconv1.2", st["out"], pre, B)
    return R


STORED = ("down1.0", "down1", "pool1", "down2.0", "down2", "pool2", "bottleneck.0", "bottleneck", "up2", "upconv2.0", "upconv2", "up1")


def stored_tensors(model, n: int, h: int, w: int) -> "OrderedDict[str, torch.Tensor]":
    """What the last fp16 forward of an [n,3,h,w] network input left in `model`'s arena (cid_stage_view), as float32 NCHW CPU tensors
    (exact: they are halfs): the STORED tensors and "upconv1.0" (tail "tiles") or "z" [n,27,Hu1,Wu1] (tail "fused")."""
    import ctypes

    from celebrity_image_denoiser_amd import _lib

    st = OrderedDict((k, model.stage_output(k, n, h, w).cpu()) for k in STORED)
    if model.tail_algo == "fused":
        off, c, hs, ws, ps, co = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert _lib.lib().cid_stage_view(b"upconv1.0", n, h, w, *(ctypes.byref(v) for v in (off, c, hs, ws, ps, co))) == 0
        cnt = n * 7 * hs.value * ws.value * 4
        zg = model._ws[off.value:off.value + 2 * cnt].view(torch.float16).view(n, 7, hs.value, ws.value, 4)
        st["z"] = z_from_groups(zg.cpu()).to(torch.float32)
    else:
        st["upconv1.0"] = model.stage_output("upconv1.0", n, h, w).cpu()
    return st


# ------------------------------------------------------------------ whole-path stand-in
MUTANTS = ("drop_tap_right_edge", "bottom_halo", "concat_swap", "crop_shift", "rtz", "bias_missing", "convt_khkw", "z_fp32")
MUTANT_LAUNCH = {"drop_tap_right_edge": "down2.0", "bottom_halo": "upconv2.2", "concat_swap": "upconv2.0", "crop_shift": "down1.2",
                 "rtz": "upconv2.2", "bias_missing": "bottleneck.2", "convt_khkw": "up1", "z_fp32": "upconv1.0"}


def forward(sd, x, in_u8: bool = False, padding=(0, 0, 0, 0), acc_dtype=torch.float32, rounding: bool = True,
            shuffle_seed: int = None, tail: str = "fused", mutate: str = None):
    """A CPU stand-in for the fp16 path: the same rounding points as the kernels, the arithmetic between them in `acc_dtype`
    (ATen's convolutions; with `shuffle_seed` the input channels of every contraction are summed in a shuffled order).
    rounding=False drops every rounding to half (then, with acc_dtype float64, this is torch_oracle.forward(dtype=float64)).
    -> (out [N,3,Hu1,Wu1] float64 tanh output, the stored tensors as check_launches takes them, plus "upconv1.0" under either tail).
    `mutate`: one of MUTANTS — a deliberately wrong variant of one launch (tests of the checks' power)."""
    rnd = half if rounding else (lambda t: t.to(torch.float64))
    rng = np.random.default_rng(shuffle_seed) if shuffle_seed is not None else None
    P = lambda k: _t(sd, k)  # noqa: E731
    W = (lambda k: half(P(k))) if rounding else P

    def perm(cin):
        return torch.from_numpy(rng.permutation(cin)) if rng is not None else None

    def acc(op, inp, w, b=None, **kw):
        p = perm(inp.shape[1])
        if p is not None:
            inp = inp[:, p]
            w = w[:, p] if op is F.conv2d else w[p]
        y = op(inp.to(acc_dtype), w.to(acc_dtype), None if b is None else b.to(acc_dtype), **kw)
        return y.to(torch.float64)

    def store(t, name):
        if mutate == "rtz" and name == MUTANT_LAUNCH["rtz"] and rounding:
            return half_rtz(t)
        return rnd(t)

    def conv(name, inp, relu=True):
        w, b = W(name + ".weight"), P(name + ".bias")
        if mutate == "bias_missing" and name == MUTANT_LAUNCH["bias_missing"]:
            b = b.clone()
            b[7] = 0.0
        if mutate == "bottom_halo" and name == MUTANT_LAUNCH["bottom_halo"]:
            # the halo row below the image holds the last row again instead of zeros
            y = acc(F.conv2d, torch.cat([F.pad(inp, (1, 1, 1, 0)), F.pad(inp[:, :, -1:], (1, 1))], 2), w, b)
        else:
            y = acc(F.conv2d, inp, w, b, padding=1)
        if mutate == "drop_tap_right_edge" and name == MUTANT_LAUNCH["drop_tap_right_edge"]:
            w2 = w.clone()
            w2[:, :, :, 0] = 0.0                                                          # the left taps
            y[:, :, :, -1] = acc(F.conv2d, inp, w2, b, padding=1)[:, :, :, -1]
        return y.clamp_min(0.0) if relu else y

    st = OrderedDict()
    xn = network_input(x, in_u8, padding)
    n, _, H, Wd = xn.shape
    H1, W1 = H // 2, Wd // 2
    H2, W2 = H1 // 2, W1 // 2
    Hu2, Wu2, Hu1, Wu1 = 2 * H2, 2 * W2, 4 * H2, 4 * W2
    st["down1.0"] = t0 = store(conv("down1.0", rnd(xn)), "down1.0")
    a = conv("down1.2", t0)
    c0 = 1 if mutate == "crop_shift" and H > Hu1 else 0
    st["down1"] = e1 = store(a[:, :, c0:c0 + Hu1, :Wu1], "down1.2")
    st["pool1"] = p1 = store(_maxpool(a[:, :, :2 * H1, :2 * W1]), "pool1")
    st["down2.0"] = t1 = store(conv("down2.0", p1), "down2.0")
    a = conv("down2.2", t1)
    st["down2"] = e2 = store(a[:, :, :Hu2, :Wu2], "down2.2")
    st["pool2"] = p2 = store(_maxpool(a[:, :, :2 * H2, :2 * W2]), "pool2")
    st["bottleneck.0"] = t2 = store(conv("bottleneck.0", p2), "bottleneck.0")
    st["bottleneck"] = bt = store(conv("bottleneck.2", t2), "bottleneck.2")
    st["up2"] = u2 = store(acc(F.conv_transpose2d, bt, W("up2.weight"), P("up2.bias"), stride=2), "up2")
    cat2 = torch.cat([e2, u2] if mutate == "concat_swap" else [u2, e2], 1)
    st["upconv2.0"] = t3 = store(conv("upconv2.0", cat2), "upconv2.0")
    st["upconv2"] = d2 = store(conv("upconv2.2", t3), "upconv2.2")
    wt = W("up1.weight")
    if mutate == "convt_khkw":
        wt = wt.transpose(2, 3)
    st["up1"] = u1 = store(acc(F.conv_transpose2d, d2, wt, P("up1.bias"), stride=2), "up1")
    st["upconv1.0"] = t4 = store(conv("upconv1.0", torch.cat([u1, e1], 1)), "upconv1.0")
    w2, b2 = W("upconv1.2.weight"), P("upconv1.2.bias")
    if tail == "tiles":
        pre = conv("upconv1.2", t4, relu=False)
    else:
        wz = w2.permute(2, 3, 0, 1).reshape(27, 64)
        z = acc(F.conv2d, t4, wz.view(27, 64, 1, 1))
        st["z"] = z = z if mutate == "z_fp32" else rnd(z)
        if acc_dtype == torch.float32:   # k_conv_tail_zh: bias + nine taps, fp32, in tap order
            zp = F.pad(z, (1, 1, 1, 1)).to(torch.float32)
            pre = b2.to(torch.float32).view(1, 3, 1, 1).expand(n, 3, Hu1, Wu1).clone()
            for tap in range(9):
                ky, kx = divmod(tap, 3)
                pre = pre + zp[:, 3 * tap:3 * tap + 3, ky:ky + Hu1, kx:kx + Wu1]
            pre = pre.to(torch.float64)
        else:
            pre = launch_ref("zsum", z, None, b2)[0]
    out = torch.tanh(pre.to(acc_dtype)).to(torch.float64)
    st["out"] = out
    return out, st
