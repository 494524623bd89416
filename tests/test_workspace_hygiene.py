"""Reads of memory nobody wrote and writes outside a buffer, off the forward path: cid_forward_saved + cid_backward,
cid_disc_forward, cid_disc_forward_saved + cid_disc_backward, and cid_quality.

The Python layers keep their workspaces (torch.empty, reused), so in training a stale word is a plausible value of the previous
step and a kernel that reads a word it never wrote passes every parity test.  Here every buffer a call writes or scratches
(outputs, saved activations, workspaces, gradient buffers) is a 256-byte aligned payload between two 4 KiB guard regions of 0xA5.
Each case runs twice, once with the payloads prefilled with 0xFF bytes (NaN bits) and cid_debug_poison_lds issued on the same
stream right before every call, once with them zero-filled, in separate allocations: every result is bit-equal between the two
runs and finite, and every guard byte still holds 0xA5.  A stale-workspace test per family runs the largest shape and then a
smaller one in the same buffers without refilling them: the smaller one's results are the bits of a run in fresh NaN-filled buffers.

With them: the generator's backward on a non-default stream, and its input gradient image by image."""
import ctypes

import pytest
import torch

import test_discriminator as TD
import test_discriminator_backward as TDB
import test_generator_backward as TGB
from celebrity_image_denoiser_amd import _lib, synth

DEV = "cuda:0"
GUARD = 4096
NAN_BYTE, ZERO_BYTE, GUARD_BYTE = 0xFF, 0x00, 0xA5


class Guarded:
    """`nbytes` of device memory, 256-byte aligned and prefilled with `fill`, between two 4 KiB regions of 0xA5."""

    def __init__(self, nbytes, fill):
        self.nbytes = int(nbytes)
        self.buf = torch.full((self.nbytes + 2 * GUARD + 256,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.start = (-self.buf.data_ptr() - GUARD) % 256 + GUARD      # 256-byte aligned, at least one guard past the start
        self.buf[self.start:self.start + self.nbytes] = fill
        self.ptr = self.buf.data_ptr() + self.start
        assert self.ptr % 256 == 0

    def bits(self, nbytes=None):
        """A copy of the payload (its first `nbytes`)."""
        return self.buf[self.start:self.start + (self.nbytes if nbytes is None else nbytes)].clone()

    def tensor(self, dtype, shape):
        n = torch.tensor([], dtype=dtype).element_size()
        for s in shape:
            n *= s
        return self.bits(n).view(dtype).view(shape)

    def intact(self):
        return bool((self.buf[:self.start] == GUARD_BYTE).all()) and bool((self.buf[self.start + self.nbytes:] == GUARD_BYTE).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _poison(fill):
    if fill == NAN_BYTE:
        assert _lib.lib().cid_debug_poison_lds(_stream()) == 0


def _compare(runs, what):
    """Two {name: tensor} results: bit-equal, and finite where floating point."""
    a, b = runs
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8)), (what, k)
        if a[k].dtype.is_floating_point:
            assert bool(torch.isfinite(a[k]).all()), (what, k)


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


# ------------------------------------------------------------------------------------------------------------------ the generator
GEN_SHAPES = ((1, 4, 4), (3, 12, 8), (2, 20, 24), (2, 40, 72))
GEN_REQUESTS = {"all": (tuple(TGB.PARAMS), True), "input": ((), True), "down1.0.weight": (("down1.0.weight",), False),
                "decoder": (tuple(TGB.DECODER), False)}


@pytest.fixture(scope="module")
def gen_module():
    m = TGB._module("hot")
    m.pack_weights()
    return m


def _gen_inputs(shape):
    n, h, w = shape
    x = torch.from_numpy(synth.make_batch(n, h, w, first_index=sum(shape))[0]).to(DEV)
    go = torch.randn((n, 3, h, w), generator=torch.Generator().manual_seed(77)).to(DEV)
    return x, go


class GenBuffers:
    """Every buffer cid_forward_saved + cid_backward write or scratch for `shape` and the gradients `want`."""

    def __init__(self, m, shape, want, want_input, fill):
        n, h, w = shape
        saved_bytes, ws_bytes = TGB._sizes(n, h, w)
        self.shapes = {k: tuple(p.shape) for k, p in m.named_parameters()}
        self.y = Guarded(n * 3 * h * w * 4, fill)
        self.saved = Guarded(saved_bytes, fill)
        self.ws = Guarded(ws_bytes, fill)
        self.grads = {k: Guarded(_numel(self.shapes[k]) * 4, fill) for k in want}
        self.gx = Guarded(n * 3 * h * w * 4, fill) if want_input else None

    def all(self):
        return [self.y, self.saved, self.ws] + list(self.grads.values()) + ([self.gx] if self.gx is not None else [])


def _gen_run(m, shape, x, go, bufs, poison):
    """cid_forward_saved + cid_backward of `shape` in `bufs` (which may be larger) -> {name: result}"""
    L = _lib.lib()
    n, h, w = shape
    _poison(poison)
    _lib.check(m._cid, L.cid_forward_saved(m._cid, x.data_ptr(), bufs.y.ptr, n, h, w, bufs.saved.ptr, bufs.saved.nbytes, _stream()))
    g = TGB._Grads()
    for k, t in bufs.grads.items():
        layer, kind = k.rsplit(".", 1)
        (g.w if kind == "weight" else g.b)[TGB.LAYERS.index(layer)] = t.ptr
    if bufs.gx is not None:
        g.input = bufs.gx.ptr
    _poison(poison)
    _lib.check(m._cid, L.cid_backward(m._cid, x.data_ptr(), bufs.y.ptr, go.data_ptr(), n, h, w, bufs.saved.ptr, bufs.saved.nbytes,
                                      ctypes.byref(g), bufs.ws.ptr, bufs.ws.nbytes, _stream()))
    torch.cuda.synchronize()
    out = {"y": bufs.y.tensor(torch.float32, (n, 3, h, w))}
    for k, t in bufs.grads.items():
        out[k] = t.tensor(torch.float32, bufs.shapes[k])
    if bufs.gx is not None:
        out["input"] = bufs.gx.tensor(torch.float32, (n, 3, h, w))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("request_", GEN_REQUESTS, ids=lambda r: r)
@pytest.mark.parametrize("shape", GEN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_generator_backward_nan_prefill_and_guards(gen_module, shape, request_):
    want, want_input = GEN_REQUESTS[request_]
    x, go = _gen_inputs(shape)
    runs = []
    for fill in (NAN_BYTE, ZERO_BYTE):
        bufs = GenBuffers(gen_module, shape, want, want_input, fill)
        runs.append(_gen_run(gen_module, shape, x, go, bufs, fill))
        assert all(b.intact() for b in bufs.all()), (shape, request_, fill)
    _compare(runs, (shape, request_))
    assert set(runs[0]) == {"y"} | set(want) | ({"input"} if want_input else set())


@pytest.mark.gpu
def test_generator_backward_in_a_stale_workspace(gen_module):
    big, small = GEN_SHAPES[-1], GEN_SHAPES[1]
    want, want_input = GEN_REQUESTS["all"]
    bufs = GenBuffers(gen_module, big, want, want_input, NAN_BYTE)
    assert all(a >= b for a, b in zip(TGB._sizes(*big), TGB._sizes(*small))) and big[0] * big[1] * big[2] >= small[0] * small[1] * small[2]
    _gen_run(gen_module, big, *_gen_inputs(big), bufs, NAN_BYTE)
    x, go = _gen_inputs(small)
    stale = _gen_run(gen_module, small, x, go, bufs, ZERO_BYTE)
    assert all(b.intact() for b in bufs.all())
    fresh = _gen_run(gen_module, small, x, go, GenBuffers(gen_module, small, want, want_input, NAN_BYTE), NAN_BYTE)
    _compare((stale, fresh), "stale")


@pytest.mark.gpu
def test_generator_backward_runs_on_a_non_default_stream():
    x, go = _gen_inputs((3, 28, 36))
    y0, g0, gx0, _, _ = TGB.cabi_backward(TGB._module("hot"), x, lambda y: go)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y1, g1, gx1, _, _ = TGB.cabi_backward(TGB._module("hot"), x, lambda y: go)
    s.synchronize()
    assert torch.equal(y0, y1) and torch.equal(gx0, gx1)
    assert all(torch.equal(g0[k], g1[k]) for k in TGB.PARAMS)


@pytest.mark.gpu
def test_generator_input_gradient_is_batch_independent(gen_module):
    x, go = _gen_inputs((5, 36, 44))
    _, _, gx, _, _ = TGB.cabi_backward(gen_module, x, lambda y: go, want=())
    for i in range(5):
        _, _, gxi, _, _ = TGB.cabi_backward(gen_module, x[i:i + 1], lambda y, i=i: go[i:i + 1], want=())
        assert torch.equal(gxi[0], gx[i]), i


# ------------------------------------------------------------------------------------------------------------ the discriminator
DISC_CASES = [((2, 1, 1), False), ((4, 7, 5), False), ((4, 7, 5), True), ((3, 37, 53), False), ((3, 37, 53), True)]
DISC_INPUTS = (("f32", True), ("f32", False), ("u8", False))     # a uint8 input has no input gradient


@pytest.fixture(scope="module")
def disc_module():
    m = TDB._module("trained", True)
    m.pack_weights()
    return m


def _disc_inputs(shape, fmt):
    u8, x = TD.images(*shape, first_index=sum(shape))
    gp = torch.randn(shape[0], generator=torch.Generator().manual_seed(78)).to(DEV)
    return (torch.from_numpy(u8) if fmt == "u8" else x).to(DEV).contiguous(), gp


def _disc_sizes(shape, training):
    L = _lib.lib()
    out = []
    for fn in (L.cid_disc_workspace_bytes, L.cid_disc_saved_bytes, L.cid_disc_backward_workspace_bytes):
        need = ctypes.c_size_t()
        assert fn(*shape, int(training), ctypes.byref(need)) == 0
        out.append(need.value)
    return out


class DiscBuffers:
    def __init__(self, m, shape, training, want_input, fill, rows=0):
        """`rows`: images the two probability buffers hold, if more than shape's."""
        n, h, w = shape
        fwd_ws, saved, bwd_ws = _disc_sizes(shape, training)
        self.shapes = {k: tuple(p.shape) for k, p in m.named_parameters()}
        self.p_plain, self.p = Guarded(max(n, rows) * 4, fill), Guarded(max(n, rows) * 4, fill)
        self.fwd_ws, self.saved, self.bwd_ws = Guarded(fwd_ws, fill), Guarded(saved, fill), Guarded(bwd_ws, fill)
        self.grads = {k: Guarded(_numel(self.shapes[k]) * 4, fill) for k in TDB.PARAMS}
        self.gx = Guarded(n * 3 * h * w * 4, fill) if want_input else None

    def all(self):
        return [self.p_plain, self.p, self.fwd_ws, self.saved, self.bwd_ws] + list(self.grads.values()) + ([self.gx] if self.gx is not None else [])


def _disc_bn(m):
    """cid_disc_bn[3] on clones of m's running buffers -> (array, the clones by name)."""
    from celebrity_image_denoiser_amd.discriminator import _BnArg

    bn, clones = (_BnArg * 3)(), {}
    for i, (idx, _) in enumerate(TD.BNS):
        b = m.model[idx]
        rm, rv, nbt = b.running_mean.clone(), b.running_var.clone(), b.num_batches_tracked.clone()
        clones.update({f"model.{idx}.running_mean": rm, f"model.{idx}.running_var": rv, f"model.{idx}.num_batches_tracked": nbt})
        bn[i] = _BnArg(b.weight.data_ptr(), b.bias.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), float(b.eps), float(b.momentum))
    return bn, clones


def _disc_run(m, shape, training, x, gp, bufs, poison):
    """cid_disc_forward, then cid_disc_forward_saved + cid_disc_backward, of `shape` in `bufs` (which may be larger) -> {name: result}"""
    L = _lib.lib()
    n, h, w = shape
    fmt = TDB._dims(x)[0]
    out = {}
    bn, clones = _disc_bn(m)
    _poison(poison)
    _lib.check_disc(m._cid, L.cid_disc_forward(m._cid, x.data_ptr(), fmt, bufs.p_plain.ptr, n, h, w, bn, int(training), bufs.fwd_ws.ptr,
                                               bufs.fwd_ws.nbytes, _stream()))
    torch.cuda.synchronize()
    out.update({"forward." + k: v for k, v in clones.items()})
    bn, clones = _disc_bn(m)
    _poison(poison)
    _lib.check_disc(m._cid, L.cid_disc_forward_saved(m._cid, x.data_ptr(), fmt, bufs.p.ptr, n, h, w, bn, int(training), bufs.saved.ptr,
                                                     bufs.saved.nbytes, _stream()))
    g = TDB._Grads()
    for k, t in bufs.grads.items():
        layer, kind = k.rsplit(".", 1)
        if layer in TDB.CONV_KEYS:
            (g.w if kind == "weight" else g.b)[TDB.CONV_KEYS.index(layer)] = t.ptr
        else:
            (g.gamma if kind == "weight" else g.beta)[(3, 6, 9).index(int(layer.split(".")[1]))] = t.ptr
    if bufs.gx is not None:
        g.input = bufs.gx.ptr
    _poison(poison)
    _lib.check_disc(m._cid, L.cid_disc_backward(m._cid, x.data_ptr(), fmt, gp.data_ptr(), n, h, w, bn, int(training), bufs.saved.ptr,
                                                bufs.saved.nbytes, ctypes.byref(g), bufs.bwd_ws.ptr, bufs.bwd_ws.nbytes, _stream()))
    torch.cuda.synchronize()
    out.update({"saved." + k: v for k, v in clones.items()})
    out["p_plain"], out["p"] = bufs.p_plain.tensor(torch.float32, (n,)), bufs.p.tensor(torch.float32, (n,))
    for k, t in bufs.grads.items():
        out[k] = t.tensor(torch.float32, bufs.shapes[k])
    if bufs.gx is not None:
        out["input"] = bufs.gx.tensor(torch.float32, (n, 3, h, w))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,want_input", DISC_INPUTS, ids=("f32-input_grad", "f32", "u8"))
@pytest.mark.parametrize("shape,training", DISC_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("train" if v else "eval"))
def test_discriminator_nan_prefill_and_guards(disc_module, shape, training, fmt, want_input):
    x, gp = _disc_inputs(shape, fmt)
    runs = []
    for fill in (NAN_BYTE, ZERO_BYTE):
        bufs = DiscBuffers(disc_module, shape, training, want_input, fill)
        runs.append(_disc_run(disc_module, shape, training, x, gp, bufs, fill))
        assert all(b.intact() for b in bufs.all()), (shape, training, fmt, fill)
    _compare(runs, (shape, training, fmt))
    assert torch.equal(runs[0]["p"], runs[0]["p_plain"])
    assert ("input" in runs[0]) == want_input


@pytest.mark.gpu
@pytest.mark.parametrize("training", (False, True), ids=("eval", "train"))
def test_discriminator_in_a_stale_workspace(disc_module, training):
    big, small = (3, 37, 53), (4, 7, 5)
    bufs = DiscBuffers(disc_module, big, training, True, NAN_BYTE, rows=small[0])
    assert all(a >= b for a, b in zip(_disc_sizes(big, training), _disc_sizes(small, training)))
    _disc_run(disc_module, big, training, *_disc_inputs(big, "f32"), bufs, NAN_BYTE)
    x, gp = _disc_inputs(small, "f32")
    stale = _disc_run(disc_module, small, training, x, gp, bufs, ZERO_BYTE)
    assert all(b.intact() for b in bufs.all())
    fresh = _disc_run(disc_module, small, training, x, gp, DiscBuffers(disc_module, small, training, True, NAN_BYTE), NAN_BYTE)
    _compare((stale, fresh), ("stale", training))


# -------------------------------------------------------------------------------------------------------------------- cid_quality
QUALITY_SHAPES = ((2, 7, 7), (3, 13, 18), (2, 161, 203))
METRIC_BITS = {"psnr": 1, "ssim": 2, "ms_ssim": 4}


def _quality_requests(shape):
    """All the metrics the size admits together, and each alone (MS-SSIM is defined for min(H, W) > 160 only)."""
    names = ("psnr", "ssim", "ms_ssim") if min(shape[1:]) > 160 else ("psnr", "ssim")
    return [names] + [(m,) for m in names]


def _quality_inputs(shape):
    _, clean, noisy_u8 = synth.make_batch(*shape, first_index=sum(shape))
    return torch.from_numpy(noisy_u8).to(DEV), torch.from_numpy(clean).to(DEV)


class QualityBuffers:
    def __init__(self, shape, bits, fill, rows=0):
        """`rows`: images the output table holds, if more than shape's."""
        need = ctypes.c_size_t()
        assert _lib.lib().cid_quality_workspace_bytes(*shape, bits, ctypes.byref(need)) == 0
        self.out, self.ws = Guarded(max(shape[0], rows) * 3 * 8, fill), Guarded(max(need.value, 256), fill)

    def all(self):
        return [self.out, self.ws]


def _quality_run(shape, names, a, b, bufs, poison):
    n, h, w = shape
    bits = sum(METRIC_BITS[m] for m in names)
    _poison(poison)
    _lib.check(None, _lib.lib().cid_quality(a.data_ptr(), _lib.CID_FMT_U8_NHWC, b.data_ptr(), _lib.CID_FMT_F32_NCHW, n, h, w, bits,
                                            bufs.out.ptr, bufs.ws.ptr, bufs.ws.nbytes, _stream()))
    torch.cuda.synchronize()
    table = bufs.out.tensor(torch.float64, (n, 3))
    out = {m: table[:, c].contiguous() for c, m in enumerate(("psnr", "ssim", "ms_ssim")) if m in names}
    out["rest"] = torch.stack([table[:, c] for c, m in enumerate(("psnr", "ssim", "ms_ssim")) if m not in names] + [table[:, 0]]).view(torch.int64)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", QUALITY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_quality_nan_prefill_and_guards(shape):
    a, b = _quality_inputs(shape)
    for names in _quality_requests(shape):
        bits = sum(METRIC_BITS[m] for m in names)
        runs = []
        for fill in (NAN_BYTE, ZERO_BYTE):
            bufs = QualityBuffers(shape, bits, fill)
            runs.append(_quality_run(shape, names, a, b, bufs, fill))
            assert all(g.intact() for g in bufs.all()), (shape, names, fill)
        _compare(runs, (shape, names))


@pytest.mark.gpu
def test_quality_in_a_stale_workspace():
    big, small = QUALITY_SHAPES[2], QUALITY_SHAPES[1]
    bufs = QualityBuffers(big, 7, NAN_BYTE, rows=small[0])
    _quality_run(big, ("psnr", "ssim", "ms_ssim"), *_quality_inputs(big), bufs, NAN_BYTE)
    a, b = _quality_inputs(small)
    names = ("psnr", "ssim")
    stale = _quality_run(small, names, a, b, bufs, ZERO_BYTE)
    assert all(g.intact() for g in bufs.all())
    fresh = _quality_run(small, names, a, b, QualityBuffers(small, 3, NAN_BYTE), NAN_BYTE)
    _compare((stale, fresh), "stale")
