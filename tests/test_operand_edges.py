"""What a call READS from its caller: the neighbours of its read-only operands, the other images of its batch, and every alignment
the C ABI admits.  tests/test_workspace_hygiene.py and the families' own hygiene tests guard what a call writes (outputs, workspaces,
saved buffers: 0xFF prefill, 0xA5 guard regions, poisoned LDS); test_large_batches.py and test_wide_offsets.py cover the launch split
and 64-bit offsets.  None of them would notice a kernel that reads one element before or after an input, that multiplies a
neighbour's value by a zero where it should select, or that assumes the 16-byte alignment every torch allocation happens to have.

One TABLE (below) has one row per launching entry point of include/cid.h: its read-only device operands with their element type,
its outputs, whether its results are per image or couple the batch, and two shapes (the smallest the entry point accepts, and the
smallest ragged multi-tile shape of its family's parity list with N = 3).  tests/test_operand_edges_host.py holds the header to it
without a GPU: a function with a `void* stream` parameter is a row, or stands in EXEMPT with its reason.

Every check is a bit comparison with the PLAIN run: the same entry point through the C ABI on ordinary torch tensors, outputs and
workspaces 0xFF-prefilled between 0xA5 guard regions as the family tests have them.  The plain run of each (row, variant, shape) is
held once to the family's float64 oracle under that family's own bound (imported from its test file), so the bit comparisons rest
on something other than the code under test.

Part A  Every read-only operand lives in an allocation of its own: a payload of exactly nbytes directly between two 4 KiB guard
        regions (class ReadOnly).  Run with the guards 0xFF-filled (NaN bits as fp32 or fp64, 255 as uint8), then 0x00-filled: all
        results are bit-equal between the two, finite, bit-equal to the plain run, and the operand and its guards keep their bytes.
        A read outside the operand that is DISCARDED is not detectable this way; only one whose value reaches a result is.
        The BatchNorm tensors that cid_disc_bn hands over as device pointers at every call (cid_disc_*, cid_srd_*, cid_sr_forward_train,
        cid_sr_forward_saved, cid_sr_backward) are operands like the images: gamma and beta in every mode, the running statistics and
        the counter in eval mode, each in a guarded allocation of its own (_bn_ops, _bn_array); in train mode the running statistics
        and the counter are written, and are in/out buffers between 0xA5 guards that start at the loaded values, as cid_adam_step's state.
        Would catch: a weight-gradient kernel (k_disc_wgrad, k_gen_wgrad) that multiplies dz = 0 of a partial tile by
        whatever `a` holds past the last image: 0 * finite is an exact zero and passes every test on torch tensors, 0 * NaN is NaN
        and reaches the gradient; a tail lane of a vector load of grad_out whose value is masked by a product.
Part B  Per-image rows only.  In the N = 3 ragged batch, fp32 image k (k = 0, 1, 2) is overwritten entirely with quiet NaN
        (0x7FC00000), and in a second run with +Inf: every result of the OTHER images (outputs, stage views, input gradients) is
        bit-equal to the clean batch, and image k's own result differs in bits from its clean one (so the test is not vacuous;
        nothing else is asserted of image k: fmaxf-style activations legitimately turn NaN into 0).  One operand is poisoned at a
        time: backwards get a second variant with grad_out / grad_prob / grad_logit of image k poisoned, and the two-tower calls
        (LPIPS, VGG) one with image k of operand b, whose tower follows tower a in the workspace, so that b[0] is a[N - 1]'s next image.
        A result named in the table that a run does not produce is an error, not a skipped comparison.  The generator also runs the (37, 100, 76) batch of
        test_gpu_parity.py::test_walking_workgroups_equal_one_item_per_workgroup with images 0, 17 and 36 poisoned in turn, in f32
        and f16, compared on the device.  Would catch: the Winograd F(4x2) walk (wino42_kernels.h) prefetches the next tile's first
        chunk under the current tile's last one, and the next tile belongs to the next image at an image's last tile: a prefetched
        value that is masked by a multiplication, or that lands in an LDS slot the current tile still reads, turns the last tile
        of image k - 1 into NaN.  With finite data that product is an exact zero, and batch independence passes.
        Results that couple the batch by definition are exempt and marked so in the table (ROW.couples): train-mode BatchNorm
        (statistics over the batch), every parameter gradient (a sum over the batch), batch-mean losses, and cid_adam_step (which
        has no images).  They run Parts A and C.  uint8 operands have no NaN: Part A's 0xFF / 0x00 guards cover their neighbours.
Part C  Every caller-supplied pointer that is not a workspace, a saved buffer or a blob sits at a 256-byte aligned address plus
        +4 and +12 bytes (fp32), +1 and +3 bytes (uint8), +8 bytes (fp64 and int64), once with every pointer offset together and
        once with the read-only operands alone, between Part A's NaN guards (the bytes between the aligned address and the payload
        are guard bytes): results bit-equal to the plain run.  The BatchNorm pointers are among them: +4 / +12 for the fp32 arrays,
        +8 for the int64 counter (the host checks none of them for alignment; the kernels read them element by element and pass).  No header sentence documents a stricter requirement for these
        pointers (fp64 outputs and int64 labels are documented at 8 bytes, which +8 keeps), so no row asserts a refusal.
        Would catch: resize_stage_rows's `& 15` head and tail units (a uint8 source at +1 / +3 starts mid-unit), a 16-byte vector
        load of an fp32 input in the LPIPS / VGG and backward kernels, adam_item's s.off when the four arrays disagree.

Python layer: each module once on `big[1:]`, a contiguous view with storage offset 1 (data_ptr() 4-byte but not 16-byte aligned, odd
for uint8): results and, for the autograd modules, input and parameter gradients bit-equal to the same call on a clone of the view.

What does fail here (run once on a scratch build, not kept): k_esr_head's padding select `v = inside ? in[...] : 0` replaced by
`in[clamp(flat index)] * (inside ? 1 : 0)`, which reads the neighbouring channel's or image's pixel and multiplies it by zero.
test_esrgan.py passes on it (71 passed: parity, batch independence, NaN prefill); Part B fails esr_forward-f32-3x37x53 for NaN and for
Inf ("out image 1 changed when image 0 was poisoned").  Reasoned, not run: Part A's example needs a read before the operand, which a
plain run cannot be given safely; the same product without the clamp reads the guard region in front of image 0 and turns row 0 of
its output into NaN with 0xFF guards and leaves it with 0x00 guards.  No kernel bug was found by any of the 402 GPU cases.

Measured on one MI355X, whole suite in one process (call + setup, all cases of a row; the first case of a row pays its float64
anchor): forward_ex 0.62 s (56 cases), forward_padded 0.04, view_u8 0.00, forward_saved+backward 0.35, disc eval 0.24, disc train 0.21,
quality 0.00, losses 0.01, add_noise 0.02, resize 0.00, adam_step 0.00, esr_forward 0.18, sr_forward 0.30, cg_forward 0.32, esd_forward
0.04, esd backward 0.16, srd eval 0.33, srd train 0.37, lpips 0.12, vgg_lpips 0.25, vgg_content_loss 0.04, vgg backward 0.12,
sr_forward_train 0.29, sr backward 0.64, the five packs 2.31, the walk 0.11, the Python layer 0.09; 7.1 s in all, no case above 1.3 s.
Worst share of the oracle bound at the anchor: forward_ex 0.24, forward_padded 0.24, forward_saved+backward 0.13, disc eval 0.10, disc
train 0.21 ((2, 1, 1): 0.006, the forward and the running statistics only), quality 0.002, losses 0.03, esr 0.17, sr 0.19, cg 0.07, esd forward 0.18, esd backward 0.11, srd eval 0.003, srd train 0.08 (at (2, 1, 1), the probabilities only), lpips 0.14,
vgg_lpips 0.42, vgg_content_loss 0.06, vgg backward 0.06 (its loss; check_gradients prints the gradients' margins, 3.5x at least),
sr_forward_train 0.37, sr backward 0.34; exact (0): view_u8, add_noise, resize, adam_step's moments, the packs."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cgan_oracle  # noqa: E402
import esrgan_disc_oracle  # noqa: E402
import esrgan_oracle  # noqa: E402
import srgan_disc_oracle  # noqa: E402
import srgan_backward_ref as SBR  # noqa: E402
import srgan_oracle  # noqa: E402
import srgan_train_oracle as STO  # noqa: E402
import esrgan_disc_bwd_oracle as EBW  # noqa: E402
import test_adam as TA  # noqa: E402
import test_discriminator as TD  # noqa: E402
import test_discriminator_backward as TDB  # noqa: E402
import test_esrgan_disc as TED  # noqa: E402
import test_esrgan_disc_backward as TEDB  # noqa: E402
import test_generator_backward as TGB  # noqa: E402
import test_gpu_parity as TGP  # noqa: E402
import test_lpips as TL  # noqa: E402
import test_lpips_vgg as TLV  # noqa: E402
import test_quality as TQ  # noqa: E402
import test_resize as TR  # noqa: E402
import test_srgan_backward as TSB  # noqa: E402
import test_srgan_disc as TSD  # noqa: E402
import test_srgan_disc_backward as TSDB  # noqa: E402
import test_srgan_train as TST  # noqa: E402
import test_vgg_backward as TVB  # noqa: E402
import test_wide_offsets as WO  # noqa: E402
import test_workspace_hygiene as H  # noqa: E402

DEV = "cuda:0"
GUARD = H.GUARD
NAN_BYTE, ZERO_BYTE = H.NAN_BYTE, H.ZERO_BYTE
F32, U8 = _lib.CID_FMT_F32_NCHW, _lib.CID_FMT_U8_NHWC
QNAN_BITS, INF_BITS = 0x7FC00000, 0x7F800000
KIND = {torch.float32: "f32", torch.uint8: "u8", torch.float64: "f64", torch.int64: "i64"}
OFFSETS = {"f32": (4, 12), "u8": (1, 3), "f64": (8, 8), "i64": (8, 8), "ws": (0, 0)}     # Part C: bytes past a 256-byte boundary
F16_TOL = TGP.FP16_TOL                                                                   # {"default": 5e-4, "hot": 5e-3}
LOSS_REL = 1e-6     # the loss tests' pytest.approx(rel=1e-6): test_discriminator.py, test_srgan_disc.py, test_esrgan_disc.py


# ------------------------------------------------------------------------------------------------------------- placing the operands
class ReadOnly:
    """The read-only variant of test_workspace_hygiene.Guarded: a copy of tensor `t` whose payload, exactly nbytes long, starts
    `offset` bytes past a 256-byte boundary and lies directly between two guard regions of at least 4 KiB of `fill` bytes."""

    def __init__(self, t, fill, offset=0):
        raw = t.contiguous().reshape(-1).view(torch.uint8)
        self.nbytes = raw.numel()
        self.buf = torch.full((self.nbytes + 2 * GUARD + 512,), fill, dtype=torch.uint8, device=DEV)
        self.start = (-self.buf.data_ptr() - GUARD) % 256 + GUARD + offset
        self.buf[self.start:self.start + self.nbytes] = raw
        self.t = self.buf[self.start:self.start + self.nbytes].view(t.dtype).view(t.shape)
        assert self.t.data_ptr() % 256 == offset and self.t.is_contiguous()
        self.before = self.buf.clone()

    def unchanged(self):
        return torch.equal(self.buf, self.before)


class Shifted(H.Guarded):
    """test_workspace_hygiene.Guarded with the payload `offset` bytes past the 256-byte boundary (0: that class itself)."""

    def __init__(self, nbytes, fill, offset=0):
        self.nbytes = int(nbytes)
        self.buf = torch.full((self.nbytes + 2 * GUARD + 512,), H.GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.start = (-self.buf.data_ptr() - GUARD) % 256 + GUARD + offset
        self.buf[self.start:self.start + self.nbytes] = fill
        self.ptr = self.buf.data_ptr() + self.start
        assert self.ptr % 256 == offset


class Place:
    """Where a run's pointers go.  fill None: the operands as they are (the plain run).  Else every operand in a ReadOnly of that
    guard byte, at OFFSETS[kind][j] (j None: aligned); outputs at the same offsets if `outputs_too`."""

    def __init__(self, fill=None, j=None, outputs_too=False):
        self.fill, self.j, self.outputs_too = fill, j, outputs_too

    def operand_offset(self, kind):
        return 0 if self.j is None else OFFSETS[kind][self.j]

    def output_offset(self, kind):
        return OFFSETS[kind][self.j] if (self.j is not None and self.outputs_too) else 0


class Outs:
    """Allocates a run's outputs, workspaces and saved buffers: 0xFF-prefilled payloads between 0xA5 guard regions."""

    def __init__(self, place):
        self.place, self.bufs = place, []

    def __call__(self, nbytes, kind, init=None):
        b = Shifted(max(int(nbytes), 1), NAN_BYTE, self.place.output_offset(kind))
        if init is not None:                                             # an in/out tensor (cid_adam_step's state)
            b.buf[b.start:b.start + b.nbytes] = init.contiguous().reshape(-1).view(torch.uint8)
        self.bufs.append(b)
        return b

    def intact(self):
        return all(b.intact() for b in self.bufs)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.clone(memory_format=torch.contiguous_format).reshape(-1).view(torch.uint8)     # a [1] column keeps its stride otherwise


def _dev(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV).contiguous()


def _numel(shape):
    return int(np.prod(shape, dtype=np.int64))


def execute(row, ctx, ops, place):
    """One run of `row` with `ops` placed by `place` -> {name: result tensor}.  The operands and their guards keep their bytes and
    no output guard byte is written."""
    placed, held = {}, []
    for k, t in ops.items():
        if place.fill is None:
            placed[k] = t
        else:
            held.append(ReadOnly(t, place.fill, place.operand_offset(KIND[t.dtype])))
            placed[k] = held[-1].t
    outs = Outs(place)
    assert _lib.lib().cid_debug_poison_lds(_stream()) == 0
    res = row.run(ctx, placed, outs)
    torch.cuda.synchronize()
    assert outs.intact(), (row.name, "a guard region of an output was written")
    assert all(r.unchanged() for r in held), (row.name, "a read-only operand or its guard was written")
    return res


def same_bits(a, b, what, finite=True):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(_bits(a[k]), _bits(b[k])), (what, k)
        if finite and a[k].dtype.is_floating_point:
            assert bool(torch.isfinite(a[k]).all()), (what, k)


# ----------------------------------------------------------------------------------------------------------------- the generator
@functools.lru_cache(maxsize=None)
def _generator(dtype, algo):
    import celebrity_image_denoiser_amd as cid

    wset = "hot" if dtype == "f32" else "default"          # the f16 bound of test_gpu_parity.py is tightest on "default"
    m = cid.load(synth.make_state_dict(wset), device=DEV, strict=True)
    m.conv_algo = algo
    m.compute_dtype = dtype
    m.pack_weights()
    return m, wset


def _gen_ws(n, h, w):
    need = ctypes.c_size_t()
    assert _lib.lib().cid_workspace_bytes(n, h, w, ctypes.byref(need)) == 0
    return need.value


def _fwd_make(variant, shape):
    fmt, dtype, algo = variant
    m, wset = _generator(dtype, algo)
    x, _, u8 = synth.make_batch(*shape, first_index=sum(shape))
    return dict(m=m, wset=wset, fmt=fmt, dtype=dtype, x=x, shape=shape), {"in": _dev(u8 if fmt == "u8" else x)}


def _fwd_call(ctx, x, out_fmt, outs):
    n, h, w = ctx["shape"]
    m = ctx["m"]
    ws = outs(_gen_ws(n, h, w), "ws")
    out = outs(n * 3 * h * w * (1 if out_fmt == U8 else 4), "u8" if out_fmt == U8 else "f32")
    _lib.check(m._cid, _lib.lib().cid_forward_ex(m._cid, x.data_ptr(), U8 if x.dtype == torch.uint8 else F32, out.ptr, out_fmt, n, h, w,
                                                 ws.ptr, ws.nbytes, _stream()))
    torch.cuda.synchronize()
    return out.tensor(torch.uint8, (n, h, w, 3)) if out_fmt == U8 else out.tensor(torch.float32, (n, 3, h, w))


def _fwd_run(ctx, ops, outs):
    return {"out": _fwd_call(ctx, ops["in"], U8 if ctx["fmt"] == "u8" else F32, outs)}


def _fwd_anchor(ctx, ops, res):
    """fp32 output against the ATen float64-checked oracle of smoke() under test_gpu_parity's bound; a uint8 output is cid_view_u8
    (anchored in its own row) of the fp32 output of the same input, which is held to the oracle."""
    from oracle import torch_oracle

    y = res["out"] if ctx["fmt"] == "f32" else _fwd_call(ctx, ops["in"], F32, Outs(Place()))
    ref = torch_oracle.forward(synth.make_state_dict(ctx["wset"]), ctx["x"]).numpy()
    bound = TGP.TOL if ctx["dtype"] == "f32" else F16_TOL[ctx["wset"]]
    share = WO._share("out", y.cpu().numpy(), ref, bound)
    if ctx["fmt"] == "u8":
        n, h, w = ctx["shape"]
        img = torch.empty((n, h, w, 3), dtype=torch.uint8, device=DEV)
        assert _lib.lib().cid_view_u8(y.data_ptr(), img.data_ptr(), n, h, w, _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(img, res["out"])
    return share


PADS = {(1, 1, 1): (1, 1, 2, 2), (3, 18, 21): (1, 1, 2, 1)}      # (left, top, right, bottom): padded sizes 4 x 4 and 20 x 24


def _pad_make(variant, shape):
    ctx, ops = _fwd_make((variant, "f32", "winograd42"), shape)
    ctx["pads"] = PADS[shape]
    return ctx, ops


def _pad_run(ctx, ops, outs):
    n, h, w = ctx["shape"]
    left, top, right, bottom = ctx["pads"]
    m, x = ctx["m"], ops["in"]
    ws = outs(_gen_ws(n, h + top + bottom, w + left + right), "ws")
    out = outs(n * 3 * h * w * 4, "f32")
    _lib.check(m._cid, _lib.lib().cid_forward_padded(m._cid, x.data_ptr(), U8 if x.dtype == torch.uint8 else F32, out.ptr, F32, n, h, w,
                                                     left, top, right, bottom, ws.ptr, ws.nbytes, _stream()))
    torch.cuda.synchronize()
    return {"out": out.tensor(torch.float32, (n, 3, h, w))}


def _pad_anchor(ctx, ops, res):
    from oracle import torch_oracle

    n, h, w = ctx["shape"]
    left, top, right, bottom = ctx["pads"]
    xp = np.full((n, 3, h + top + bottom, w + left + right), -1.0, np.float32)       # the band is uint8 0 = -1.0
    xp[:, :, top:top + h, left:left + w] = ctx["x"]
    ref = torch_oracle.forward(synth.make_state_dict(ctx["wset"]), xp).numpy()[:, :, top:top + h, left:left + w]
    return WO._share("out", res["out"].cpu().numpy(), ref, TGP.TOL)


def _view_make(variant, shape):
    x, _, _ = synth.make_batch(*shape, first_index=sum(shape))
    return dict(shape=shape, y=(x * np.float32(1.25)).astype(np.float32)), {"in": _dev((x * np.float32(1.25)).astype(np.float32))}


def _view_run(ctx, ops, outs):
    n, h, w = ctx["shape"]
    img = outs(n * h * w * 3, "u8")
    assert _lib.lib().cid_view_u8(ops["in"].data_ptr(), img.ptr, n, h, w, _stream()) == 0
    torch.cuda.synchronize()
    return {"out": img.tensor(torch.uint8, (n, h, w, 3))}


def _view_anchor(ctx, ops, res):
    """include/cid.h states the arithmetic: (uint8)(clamp(y * 0.5 + 0.5, 0, 1) * 255), truncating, in fp32.  Exact."""
    y = ctx["y"]
    v = np.clip(y * np.float32(0.5) + np.float32(0.5), np.float32(0), np.float32(1)) * np.float32(255)
    want = v.astype(np.uint8).transpose(0, 2, 3, 1)
    assert np.array_equal(res["out"].cpu().numpy(), want)
    return 0.0


GEN_STAGES = TGB.RELU_STAGES + ("pool1", "pool2")


@functools.lru_cache(maxsize=None)
def _gen_module():
    m = TGB._module("hot")
    m.pack_weights()
    return m


def _bwd_make(variant, shape):
    x, go = H._gen_inputs(shape)
    return dict(m=_gen_module(), shape=shape), {"in": x, "grad_out": go}


def _bwd_run(ctx, ops, outs):
    m, shape = ctx["m"], ctx["shape"]
    n, h, w = shape
    saved_bytes, ws_bytes = TGB._sizes(n, h, w)
    b = object.__new__(H.GenBuffers)
    b.shapes = {k: tuple(p.shape) for k, p in m.named_parameters()}
    b.y, b.saved, b.ws = outs(n * 3 * h * w * 4, "f32"), outs(saved_bytes, "ws"), outs(ws_bytes, "ws")
    b.grads = {k: outs(_numel(b.shapes[k]) * 4, "f32") for k in TGB.PARAMS}
    b.gx = outs(n * 3 * h * w * 4, "f32")
    res = H._gen_run(m, shape, ops["in"], ops["grad_out"], b, NAN_BYTE)
    saved = b.saved.bits()
    for s in GEN_STAGES:
        res["stage." + s] = TGB.stage(saved, s, n, h, w)
    return res


def _bwd_anchor(ctx, ops, res):
    """The plain run has the bits of test_generator_backward.cabi_backward, which _parity holds to float64 under that file's rule."""
    m, shape = ctx["m"], ctx["shape"]
    x, go = ops["in"], ops["grad_out"]
    y, grads, gx, _, _ = TGB.cabi_backward(m, x, lambda y: go)
    assert torch.equal(y, res["y"]) and torch.equal(gx, res["input"]) and all(torch.equal(grads[k], res[k]) for k in TGB.PARAMS)
    e_hip, e_aten = TGB._parity("hot", None, shape, m=m, x=x.cpu(), grad_out=go.cpu())
    return max(e_hip[k] / max(TGB.TOL, 2 * e_aten[k]) for k in e_hip)


# ------------------------------------------------------------------------------- the BatchNorm tensors a call takes as pointers
BN_STATE = (("running_mean", "f32"), ("running_var", "f32"), ("num_batches_tracked", "i64"))


def _bn_ops(layers, training):
    """The tensors of cid_disc_bn that a call only reads, as operands {"<layer>.<field>": tensor}: gamma and beta in every mode, the
    running statistics and the counter in eval mode.  (Train mode updates those three: _bn_array places them as in/out buffers.)"""
    ops = {}
    for name, b in layers:
        ops[name + ".gamma"], ops[name + ".beta"] = b.weight.detach().clone(), b.bias.detach().clone()
        if not training:
            for f, _ in BN_STATE:
                ops[f"{name}.{f}"] = getattr(b, f).detach().clone()
    return ops


def _bn_array(layers, ops, outs, training, state=None):
    """cid_disc_bn[len(layers)] whose every device pointer is a placed operand or, in train mode for the running statistics and the
    counter, an in/out buffer of `outs` that starts at the layer's loaded value (`state`: a state dict to take it from instead).
    -> (the array, {"<layer>.<field>": in/out buffer})"""
    from celebrity_image_denoiser_amd.discriminator import _BnArg

    bn, inout = (_BnArg * len(layers))(), {}
    for i, (name, b) in enumerate(layers):
        ptrs = []
        for f, kind in BN_STATE:
            if training:
                start = getattr(b, f).detach() if state is None else _dev(np.asarray(state[f"{name}.{f}"]))
                inout[f"{name}.{f}"] = outs(start.numel() * start.element_size(), kind, init=start)
                ptrs.append(inout[f"{name}.{f}"].ptr)
            else:
                ptrs.append(ops[f"{name}.{f}"].data_ptr())
        bn[i] = _BnArg(ops[name + ".gamma"].data_ptr(), ops[name + ".beta"].data_ptr(), *ptrs, float(b.eps),
                       _lib.CID_DISC_MOMENTUM_NONE if b.momentum is None else float(b.momentum))
    return bn, inout


def _bn_results(prefix, layers, inout):
    out = {}
    for name, b in layers:
        for f, _ in BN_STATE:
            if f"{name}.{f}" in inout:
                t = getattr(b, f)
                out[f"{prefix}{name}.{f}"] = inout[f"{name}.{f}"].tensor(t.dtype, tuple(t.shape))
    return out


# ------------------------------------------------------------------------- DenoiseDiscriminator and SRGANDiscriminator (cid_srd_*)
def _disc_slot(g, k):
    layer, kind = k.rsplit(".", 1)
    if layer in TDB.CONV_KEYS:
        return (g.w if kind == "weight" else g.b), TDB.CONV_KEYS.index(layer)
    return (g.gamma if kind == "weight" else g.beta), [i for i, _ in TD.BNS].index(int(layer.split(".")[1]))


def _srd_slot(g, k):
    idx, kind = int(k.split(".")[1]), k.rsplit(".", 1)[1]
    if idx in TSDB.CONV_IDX:
        return (g.w if kind == "weight" else g.b), TSDB.CONV_IDX.index(idx)
    return (g.gamma if kind == "weight" else g.beta), TSDB.BN_IDX.index(idx)


BND = {"disc": dict(T=TDB, bns=[i for i, _ in TD.BNS], grads=TDB._Grads, slot=_disc_slot, check=_lib.check_disc),
       "srd": dict(T=TSDB, bns=list(TSDB.BN_IDX), grads=TSDB.Grads, slot=_srd_slot, check=_lib.check_srd)}
TRAIN_MIN = (2, 1, 1)      # the smallest batch train mode accepts: two values per channel


@functools.lru_cache(maxsize=None)
def _bnd_module(fam, training):
    m = BND[fam]["T"]._module("trained", training)
    m.pack_weights()
    return m


def _bnd_layers(fam, m):
    return [(f"model.{i}", m.model[i]) for i in BND[fam]["bns"]]


def _bnd_images(fam, shape, training):
    """(uint8, fp32) CPU batch: the family's own images of the shape.  At TRAIN_MIN the SRGAN discriminator's family takes the first
    well-conditioned draw of a fixed sequence (test_srgan_disc._train_case says why); so does this."""
    if fam == "disc":
        return TD.images(*shape, first_index=sum(shape))
    if training and shape == TRAIN_MIN:
        x = TSD._train_case("trained", shape, 0.1)[0][0]
        for draw in range(16):
            u8, xd = srgan_disc_oracle.images(*shape, first_index=sum(shape) + 1000 * draw)
            if torch.equal(xd, x):
                return u8, x
        raise AssertionError("the draw of _train_case was not found")
    return TSD._batch(shape)


def _bnd_make(variant, shape):
    fam, fmt, training = variant
    T, m = BND[fam]["T"], _bnd_module(fam, training)
    u8, x = _bnd_images(fam, shape, training)
    xin = _dev(u8 if fmt == "u8" else x)
    # grad_prob = d BCE(p, 1) / dp at the probabilities of this very batch, as the families' gradient parity has it
    _, _, _, _, gp = T.cabi_backward(m, xin, training, lambda q: T._bce_grad(q, 1.0), want=(), want_input=False, with_masks=False)
    ops = {"in": xin, "grad_prob": gp}
    ops.update(_bn_ops(_bnd_layers(fam, m), training))
    return dict(fam=fam, m=m, shape=shape, training=training, fmt=fmt, x=x), ops


def _bnd_run(ctx, ops, outs):
    """cid_<fam>_forward, then cid_<fam>_forward_saved + cid_<fam>_backward, every BatchNorm pointer a placed operand."""
    L, fam = _lib.lib(), ctx["fam"]
    cfg, m, training = BND[fam], ctx["m"], int(ctx["training"])
    fn = lambda name: getattr(L, f"cid_{fam}_{name}")   # noqa: E731
    n, h, w = ctx["shape"]
    x, layers = ops["in"], _bnd_layers(fam, m)
    fmt = U8 if x.dtype == torch.uint8 else F32
    sd = dict(m.named_parameters())
    fwd_ws, p_plain = outs(WO._size(fn("workspace_bytes"), n, h, w, training), "ws"), outs(4 * n, "f32")
    bn, state = _bn_array(layers, ops, outs, training)
    cfg["check"](m._cid, fn("forward")(m._cid, x.data_ptr(), fmt, p_plain.ptr, n, h, w, bn, training, fwd_ws.ptr, fwd_ws.nbytes, _stream()))
    torch.cuda.synchronize()
    res = _bn_results("forward.", layers, state)
    saved, p = outs(WO._size(fn("saved_bytes"), n, h, w, training), "ws"), outs(4 * n, "f32")
    bn, state = _bn_array(layers, ops, outs, training)
    assert L.cid_debug_poison_lds(_stream()) == 0
    cfg["check"](m._cid, fn("forward_saved")(m._cid, x.data_ptr(), fmt, p.ptr, n, h, w, bn, training, saved.ptr, saved.nbytes, _stream()))
    g = cfg["grads"]()
    grads = {k: outs(4 * sd[k].numel(), "f32") for k in cfg["T"].PARAMS}
    for k, b in grads.items():
        arr, i = cfg["slot"](g, k)
        arr[i] = b.ptr
    gx = outs(4 * n * 3 * h * w, "f32") if fmt == F32 else None                 # a uint8 input has no input gradient
    if gx is not None:
        g.input = gx.ptr
    bwd_ws = outs(WO._size(fn("backward_workspace_bytes"), n, h, w, training), "ws")
    assert L.cid_debug_poison_lds(_stream()) == 0
    cfg["check"](m._cid, fn("backward")(m._cid, x.data_ptr(), fmt, ops["grad_prob"].data_ptr(), n, h, w, bn, training, saved.ptr, saved.nbytes,
                                        ctypes.byref(g), bwd_ws.ptr, bwd_ws.nbytes, _stream()))
    torch.cuda.synchronize()
    res.update(_bn_results("saved.", layers, state))
    res["p_plain"], res["p"] = p_plain.tensor(torch.float32, (n,)), p.tensor(torch.float32, (n,))
    res.update({k: b.tensor(torch.float32, tuple(sd[k].shape)) for k, b in grads.items()})
    if gx is not None:
        res["input"] = gx.tensor(torch.float32, (n, 3, h, w))
    return res


def _bnd_anchor(ctx, ops, res):
    """The plain run has the bits of the family's cabi_backward on the same batch.  That is held to float64 by the family's gradient
    parity (same weights, same images, loss "real1"), and the probabilities by the float64 restatement.  At TRAIN_MIN the families
    hold only the forward (gradients over two values per channel are ill-conditioned whoever computes them; their parity lists leave
    the shape out): there the probabilities, and the DenoiseDiscriminator's running statistics, are held to the restatement under
    the rule of the family's train-mode parity, and the gradients only to cabi_backward's bits."""
    fam, m, shape, training = ctx["fam"], ctx["m"], ctx["shape"], ctx["training"]
    T = BND[fam]["T"]
    want_input = ctx["fmt"] == "f32"
    p, grads, gx, _, _ = T.cabi_backward(m, ops["in"], training, lambda q: ops["grad_prob"], want_input=want_input, with_masks=False)
    assert torch.equal(p, res["p"]) and torch.equal(p, res["p_plain"]) and all(torch.equal(grads[k], res[k]) for k in T.PARAMS)
    if not want_input:            # the uint8 batch is read as its normalised fp32 copy, whose variant is anchored
        return 0.0
    assert torch.equal(gx, res["input"])
    got_p = res["p"].cpu().numpy()
    if fam == "disc":
        sd64 = TD.cast(TD.weights("trained"), torch.float64)
        ref = TD.restate(sd64, ctx["x"].double(), training)                    # in train mode it moves sd64's running statistics
        share = WO._share("p", got_p, ref.numpy().reshape(-1), TD.TOL)
        if training:
            for i, _ in TD.BNS:
                for f in ("running_mean", "running_var"):
                    want = sd64[f"model.{i}.{f}"]
                    err = (res[f"forward.model.{i}.{f}"].cpu().double() - want).abs() / (TD.TOL * torch.clamp(want.abs(), min=1.0))
                    assert float(err.max()) <= 1.0, (i, f, float(err.max()))      # test_discriminator._check_train's rule
                    share = max(share, float(err.max()))
        if not (training and shape == TRAIN_MIN):
            e_hip, e_aten = TDB.gradient_parity("trained", shape, training, "real1")
            share = max(share, max(e_hip[k] / max(TDB.TOL, 2 * e_aten[k]) for k in e_hip))
        return share
    if training and shape == TRAIN_MIN:
        ref = TSD._train_case("trained", shape, 0.1)[0][1]
    else:
        TSDB.test_gradient_parity("trained", shape, training, "real1")         # asserts its rule; returns nothing
        ref = srgan_disc_oracle.restate(srgan_disc_oracle.cast(srgan_disc_oracle.weights("trained"), torch.float64), ctx["x"].double(), training)
    return WO._share("p", got_p, ref.numpy().reshape(-1), TSD.TOL)


# ------------------------------------------------------------------------------------------------------------------ cid_quality
def _quality_names(shape):
    return H._quality_requests(shape)[0]


def _quality_make(variant, shape):
    a, b = H._quality_inputs(shape)
    return dict(shape=shape), {"a": a, "b": b}


def _quality_run(ctx, ops, outs):
    shape = ctx["shape"]
    names = _quality_names(shape)
    bits = sum(H.METRIC_BITS[m] for m in names)
    need = ctypes.c_size_t()
    assert _lib.lib().cid_quality_workspace_bytes(*shape, bits, ctypes.byref(need)) == 0
    b = object.__new__(H.QualityBuffers)
    b.out, b.ws = outs(shape[0] * 3 * 8, "f64"), outs(max(need.value, 256), "ws")
    res = H._quality_run(shape, names, ops["a"], ops["b"], b, NAN_BYTE)
    res.pop("rest")          # the columns not asked for keep their prefill: not a result
    return res


def _quality_anchor(ctx, ops, res):
    a = synth.normalize_u8(ops["a"].cpu().numpy())
    names = _quality_names(ctx["shape"])
    got, ref = {k: res[k].cpu().numpy() for k in names}, TQ.oracle(a, ops["b"].cpu().numpy(), names)
    TQ._check(got, ref)
    return max(float(np.abs(got[k] - ref[k]).max()) / (TQ.PSNR_TOL if k == "psnr" else TQ.SSIM_TOL) for k in names)


# ----------------------------------------------------------------------------------------------------------------- the four losses
def _bce64(p, target):
    return TD._bce(p.cpu(), target)


def _loss_make(variant, shape):
    n, h, w = shape
    g = torch.Generator().manual_seed(100 + n)
    if variant in ("disc", "srd"):
        a, b = torch.rand(n, generator=g) * 0.98 + 0.01, torch.rand(n, generator=g) * 0.98 + 0.01       # probabilities
    else:
        a, b = torch.randn(n, generator=g) * 3.0, torch.randn(n, generator=g) * 3.0                     # logits
    ops = {"real": _dev(a), "fake": _dev(b)}
    if variant in ("disc", "esd_trainer"):
        u8, clean = TD.images(n, h, w, first_index=sum(shape))
        den = (clean + 0.05 * torch.sin(torch.arange(clean.numel(), dtype=torch.float32).reshape(clean.shape))).clamp(-1, 1)
        ops.update({"denoised": _dev(den), "clean": _dev(u8)})          # one fp32 and one uint8 image operand
    return dict(which=variant, shape=shape), ops


LOSS_OUT = {"disc": 4, "srd": 2, "esd": 3, "esd_trainer": 4}


def _loss_run(ctx, ops, outs):
    L, which = _lib.lib(), ctx["which"]
    n, h, w = ctx["shape"]
    out = outs(8 * LOSS_OUT[which], "f64")
    r, f = ops["real"].data_ptr(), ops["fake"].data_ptr()
    if which == "disc":
        rc = L.cid_disc_losses(r, f, ops["denoised"].data_ptr(), F32, ops["clean"].data_ptr(), U8, n, h, w, out.ptr, _stream())
    elif which == "srd":
        rc = L.cid_srd_losses(r, f, n, out.ptr, _stream())
    elif which == "esd":
        rc = L.cid_esd_losses(r, f, n, out.ptr, _stream())
    else:
        rc = L.cid_esd_trainer_losses(r, f, ops["denoised"].data_ptr(), F32, ops["clean"].data_ptr(), U8, n, h, w, out.ptr, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {"out": out.tensor(torch.float64, (LOSS_OUT[which],))}


def _loss_anchor(ctx, ops, res):
    """The float64 restatements of the loss tests of test_discriminator.py, test_srgan_disc.py and test_esrgan_disc.py."""
    which = ctx["which"]
    got = res["out"].cpu().tolist()
    r, f = ops["real"], ops["fake"]
    if which in ("disc", "srd"):
        want = [_bce64(r, 1.0) + _bce64(f, 0.0), _bce64(f, 1.0)]
    else:
        real1, fake0, fake1 = TED._want_losses(r, f)
        want = [real1, fake0, fake1]
    if which in ("disc", "esd_trainer"):
        den = ops["denoised"].cpu().double()
        u8 = ops["clean"].cpu().numpy()
        clean = torch.from_numpy(synth.normalize_u8(u8) if which == "disc" else
                                 np.ascontiguousarray((u8.astype(np.float64) / 255.0).transpose(0, 3, 1, 2))).double()
        mse = float(((den - clean) ** 2).mean())
        want = ([want[0], mse + 0.001 * want[1], mse, want[1]] if which == "disc" else
                [0.5 * (want[0] + want[1]), want[2], mse, mse + 1e-3 * want[2]])
    print(which, "got", got, "want", want)
    worst = 0.0
    for g_, w_ in zip(got, want):
        assert g_ == pytest.approx(w_, rel=LOSS_REL), (which, got, want)
        worst = max(worst, abs(g_ - w_) / (LOSS_REL * abs(w_)))
    return worst


# ----------------------------------------------------------------------------------------------- cid_add_noise, cid_resize, cid_adam
NOISE_KINDS = {"gaussian": _lib.CID_NOISE_GAUSSIAN, "salt_pepper": _lib.CID_NOISE_SALT_PEPPER, "poisson": _lib.CID_NOISE_POISSON}
NOISE_PARAMS = {"gaussian": (0.0, 25.0), "salt_pepper": (0.02, 0.02), "poisson": ()}


def _noise_make(variant, shape):
    import test_noise as TN

    clean = TN._inputs(*shape, 500 + shape[1])
    return dict(kind=variant, shape=shape, clean=clean), {"clean": _dev(clean)}


def _noise_run(ctx, ops, outs):
    n, h, w = ctx["shape"]
    out = outs(n * h * w * 3, "u8")
    p = NOISE_PARAMS[ctx["kind"]]
    params = (ctypes.c_double * max(len(p), 1))(*p)
    rc = _lib.lib().cid_add_noise(ops["clean"].data_ptr(), out.ptr, n, h, w, NOISE_KINDS[ctx["kind"]], params, len(p), 12345, 77, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {"out": out.tensor(torch.uint8, (n, h, w, 3))}


def _noise_anchor(ctx, ops, res):
    import test_noise as TN

    TN._assert_matches(res["out"].cpu().numpy(), ctx["clean"], ctx["kind"], 12345, 77)
    return 0.0


def _resize_make(variant, shape):
    x, ref = TR._case(shape)
    return dict(fmt=variant, shape=shape, ref=ref), {"src": _dev(np.array(x))}


def _resize_run(ctx, ops, outs):
    L = _lib.lib()
    hs, ws, hd, wd = ctx["shape"]
    n = ops["src"].shape[0]
    plan = ctypes.c_void_p()
    assert L.cid_resize_plan_create(ctypes.byref(plan), hs, ws, hd, wd, _lib.CID_RESAMPLE_BICUBIC) == 0
    try:
        u8 = ctx["fmt"] == "u8"
        dst = outs(n * hd * wd * 3 * (1 if u8 else 4), "u8" if u8 else "f32")
        rc = L.cid_resize(plan, ops["src"].data_ptr(), dst.ptr, U8 if u8 else F32, n, _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
    finally:
        L.cid_resize_plan_destroy(plan)
    return {"dst": dst.tensor(torch.uint8, (n, hd, wd, 3)) if u8 else dst.tensor(torch.float32, (n, 3, hd, wd))}


def _resize_anchor(ctx, ops, res):
    """Pillow's bytes (synth.resize_bicubic_np), exactly, as test_resize.py::test_resize_equals_the_restatement."""
    got = res["dst"].cpu().numpy()
    if ctx["fmt"] == "u8":
        assert np.array_equal(got, ctx["ref"])
    else:
        assert np.array_equal(got.view(np.uint32), TR._normalized(ctx["ref"]).view(np.uint32))
    return 0.0


ADAM_STATE = ("param", "exp_avg", "exp_avg_sq")


def _adam_make(variant, shape):
    rng = np.random.default_rng(7 + shape[0])
    n = shape[0]
    state = {"param": (rng.standard_normal(n) * 0.05).astype(np.float32), "exp_avg": (rng.standard_normal(n) * 1e-3).astype(np.float32),
             "exp_avg_sq": (rng.random(n) * 1e-5).astype(np.float32)}
    grad = TA._gradient(rng, n)
    return dict(n=n, state=state, grad=grad, wd=variant), {"grad": _dev(grad)}


def _adam_run(ctx, ops, outs):
    n = ctx["n"]
    bufs = {k: outs(4 * n, "f32", init=_dev(ctx["state"][k])) for k in ADAM_STATE}
    t = (_lib.AdamTensor * 1)()
    t[0].param, t[0].exp_avg, t[0].exp_avg_sq, t[0].grad = bufs["param"].ptr, bufs["exp_avg"].ptr, bufs["exp_avg_sq"].ptr, ops["grad"].data_ptr()
    t[0].count, t[0].step = n, 3
    TA._launch(t, TA._hyper(ctx["wd"]))
    torch.cuda.synchronize()
    return {k: bufs[k].tensor(torch.float32, (n,)) for k in ADAM_STATE}


def _adam_anchor(ctx, ops, res):
    """test_adam.py::test_identity_with_the_restatement's rule: exp_avg and exp_avg_sq bit for bit, the parameter within one ulp at
    no more than ceil(1e-6 count) elements."""
    s = ctx["state"]
    p1, m1, v1 = synth.adam_step_np(s["param"], ctx["grad"], s["exp_avg"], s["exp_avg_sq"], 3, lr=TA.LR, weight_decay=ctx["wd"])
    assert np.array_equal(TA._bits(res["exp_avg"].cpu().numpy()), TA._bits(m1))
    assert np.array_equal(TA._bits(res["exp_avg_sq"].cpu().numpy()), TA._bits(v1))
    d = TA._ulp_distance(res["param"].cpu().numpy(), p1)
    assert d.max() <= 1 and int((d > 0).sum()) <= int(np.ceil(1e-6 * ctx["n"]))
    return float(d.max())


# ------------------------------------------------------------------------- the server generators and the two newer discriminators
def _views(fn, stages, *dims):
    return [(s,) + WO._view(fn, s, *dims) for s in stages]


def _stage_results(res, raw, views, n):
    """Every stage view's tensor as [N, bytes of one image]: the C8 layout is image-major."""
    for name, off, c, hs, ws in views:
        res["stage." + name] = raw[off:off + 4 * n * c * hs * ws].view(n, -1)


def _stage_shares(res, views, ref, bound):
    """Each stage view of the whole batch against ref[name] (float64 NCHW) -> the worst share of bound(ref[name])."""
    worst = 0.0
    for v in views:
        got = np.concatenate([WO._nchw(res["stage." + v[0]][i], v) for i in range(res["stage." + v[0]].shape[0])])
        worst = max(worst, WO._share(v[0], got, ref[v[0]], bound(ref[v[0]])))
    return worst


ESR_R, ESR_STAGES = 2, ("x1", "tail_in")


@functools.lru_cache(maxsize=None)
def _esr_model():
    from celebrity_image_denoiser_amd.esrgan import load_esrgan

    sd = synth.make_esrgan_state_dict("hot", ESR_R)
    return load_esrgan(sd, num_residuals=ESR_R, device=DEV, strict=True), sd


def _esr_make(variant, shape):
    u8 = synth.esrgan_inputs_u8(*shape, 1100 + sum(shape))
    x = np.ascontiguousarray((u8.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))      # test_esrgan.input_of
    return dict(shape=shape, x=x), {"in": _dev(u8 if variant == "u8" else x)}


def _esr_run(ctx, ops, outs):
    L = _lib.lib()
    m, _ = _esr_model()
    n, h, w = ctx["shape"]
    x = ops["in"]
    ws, out = outs(WO._size(L.cid_esr_workspace_bytes, n, h, w), "ws"), outs(4 * n * 3 * h * w, "f32")
    _lib.check_abi("esr", m._cid, L.cid_esr_forward(m._cid, x.data_ptr(), U8 if x.dtype == torch.uint8 else F32, out.ptr, F32, n, h, w, ws.ptr,
                                                    ws.nbytes, _stream()))
    torch.cuda.synchronize()
    res = {"out": out.tensor(torch.float32, (n, 3, h, w))}
    _stage_results(res, ws.bits(), _views(L.cid_esr_stage_view, ESR_STAGES, n, h, w), n)
    return res


def _esr_anchor(ctx, ops, res):
    n, h, w = ctx["shape"]
    ref = esrgan_oracle.forward(_esr_model()[1], ctx["x"], ESR_R)
    share = _stage_shares(res, _views(_lib.lib().cid_esr_stage_view, ESR_STAGES, n, h, w), ref, esrgan_oracle.bound)
    return max(share, WO._share("out", res["out"].cpu().numpy(), ref["out"], esrgan_oracle.bound(ref["out"])))


SR_STAGES = ("x0", "trunk", "up1", "tail_in")


@functools.lru_cache(maxsize=None)
def _sr_model(scale):
    from celebrity_image_denoiser_amd.srgan import load_srgan

    sd = synth.make_srgan_state_dict("hot", scale)
    return load_srgan(sd, scale_factor=scale, device=DEV, strict=True), sd


def _sr_make(variant, shape):
    n, h, w, s = shape
    u8 = synth.srgan_inputs_u8(n, h, w, 2100 + sum(shape))
    x = srgan_oracle.normalise_u8(u8)
    return dict(shape=shape, x=x), {"in": _dev(u8 if variant == "u8" else x)}


def _sr_run(ctx, ops, outs):
    L = _lib.lib()
    n, h, w, s = ctx["shape"]
    m, _ = _sr_model(s)
    x = ops["in"]
    ws, out = outs(WO._size(L.cid_sr_workspace_bytes, n, h, w, s), "ws"), outs(4 * n * 3 * s * h * s * w, "f32")
    _lib.check_abi("sr", m._cid, L.cid_sr_forward(m._cid, x.data_ptr(), U8 if x.dtype == torch.uint8 else F32, out.ptr, F32, n, h, w,
                                                  0, 0, 0, 0, 0, ws.ptr, ws.nbytes, _stream()))
    torch.cuda.synchronize()
    res = {"out": out.tensor(torch.float32, (n, 3, s * h, s * w))}
    _stage_results(res, ws.bits(), _views(L.cid_sr_stage_view, SR_STAGES, n, h, w, s), n)
    return res


def _sr_anchor(ctx, ops, res):
    n, h, w, s = ctx["shape"]
    ref = srgan_oracle.forward(_sr_model(s)[1], ctx["x"])
    share = _stage_shares(res, _views(_lib.lib().cid_sr_stage_view, SR_STAGES, n, h, w, s), ref, srgan_oracle.bound)
    return max(share, WO._share("out", res["out"].cpu().numpy(), ref["out"], srgan_oracle.bound(ref["pre"])))   # as test_srgan.py


CG_STAGES, CG_CLASSES = ("l1", "t1", "t2", "t3"), 10


@functools.lru_cache(maxsize=None)
def _cg_model():
    from celebrity_image_denoiser_amd.cgan import load_cgan

    sd = synth.make_cgan_state_dict("hot", CG_CLASSES)
    return load_cgan(sd, n_classes=CG_CLASSES, device=DEV, strict=True), sd


def _cg_make(variant, shape):
    import test_cgan as TC

    n = shape[0]
    z, labels = synth.cgan_latent_np(n, TC.SEED, 100 * n), TC.labels_of(n, CG_CLASSES)
    return dict(shape=shape, z=z, labels=labels), {"z": _dev(z), "labels": _dev(np.asarray(labels, np.int64))}


def _cg_run(ctx, ops, outs):
    L = _lib.lib()
    m, _ = _cg_model()
    n = ctx["shape"][0]
    ws, out = outs(WO._size(L.cid_cg_workspace_bytes, n), "ws"), outs(4 * n * 3 * 64 * 64, "f32")
    _lib.check_abi("cg", m._cid, L.cid_cg_forward(m._cid, ops["z"].data_ptr(), ops["labels"].data_ptr(), out.ptr, F32, n, 0, ws.ptr, ws.nbytes,
                                                  _stream()))
    torch.cuda.synchronize()
    res = {"out": out.tensor(torch.float32, (n, 3, 64, 64))}
    _stage_results(res, ws.bits(), _views(L.cid_cg_stage_view, CG_STAGES, n), n)
    return res


def _cg_anchor(ctx, ops, res):
    n = ctx["shape"][0]
    ref = cgan_oracle.forward(_cg_model()[1], ctx["z"], ctx["labels"])
    share = _stage_shares(res, _views(_lib.lib().cid_cg_stage_view, CG_STAGES, n), ref, cgan_oracle.bound)
    return max(share, WO._share("out", res["out"].cpu().numpy(), ref["out"], cgan_oracle.bound(ref["pre"])))    # as test_cgan.py


@functools.lru_cache(maxsize=None)
def _esd_module(hw):
    m = TED._module("trained", hw)
    m.pack_weights()
    return m


def _esd_views(n, h, w):
    offs, _ = esrgan_disc_oracle.expected_workspace(n, h, w)                 # the formula of include/cid.h
    views = []
    for name, off, ch in zip(("a1", "a2", "a3", "a4"), offs, (64, 128, 256, 512)):
        h, w = WO._side(h), WO._side(w)
        views.append((name, off, ch, h, w))
    return views


def _esd_make(variant, shape):
    u8, x, st64, lg64 = esrgan_disc_oracle.case("trained", shape)
    return dict(shape=shape, st64=st64, lg64=lg64), {"in": _dev(u8 if variant == "u8" else x)}


def _esd_run(ctx, ops, outs):
    L = _lib.lib()
    n, h, w = ctx["shape"]
    m = _esd_module((h, w))
    x = ops["in"]
    ws, out = outs(WO._size(L.cid_esd_workspace_bytes, n, h, w), "ws"), outs(4 * n, "f32")
    _lib.check_abi("esd", m._cid, L.cid_esd_forward(m._cid, x.data_ptr(), U8 if x.dtype == torch.uint8 else F32, out.ptr, n, h, w, ws.ptr,
                                                    ws.nbytes, _stream()))
    torch.cuda.synchronize()
    res = {"logit": out.tensor(torch.float32, (n,))}
    _stage_results(res, ws.bits(), _esd_views(n, h, w), n)
    return res


def _esd_anchor(ctx, ops, res):
    n, h, w = ctx["shape"]
    bound = lambda t: esrgan_disc_oracle.TOL * max(1.0, float(np.abs(t).max()))   # noqa: E731
    ref = {v[0]: r.numpy() for v, r in zip(_esd_views(n, h, w), ctx["st64"])}
    share = _stage_shares(res, _esd_views(n, h, w), ref, bound)
    lg = ctx["lg64"].numpy().reshape(-1)
    return max(share, WO._share("logit", res["logit"].cpu().numpy(), lg, bound(lg)))


def _esdb_make(variant, shape):
    ref = EBW.reference("trained", shape, "real1")
    m = _esd_module(shape[1:])
    logits, _ = TEDB.forward_saved(m, _dev(ref["x"]))
    gl = EBW.bce_grad(logits, "real1")
    return dict(shape=shape, ref=ref, fmt=variant), {"in": _dev(ref["u8"] if variant == "u8" else ref["x"]), "grad_logit": gl}


def _esdb_run(ctx, ops, outs):
    L = _lib.lib()
    n, h, w = ctx["shape"]
    m = _esd_module((h, w))
    x = ops["in"]
    fmt = U8 if x.dtype == torch.uint8 else F32
    sd = m.state_dict()
    saved, out = outs(WO._size(L.cid_esd_saved_bytes, n, h, w), "ws"), outs(4 * n, "f32")
    _lib.check_abi("esd", m._cid, L.cid_esd_forward_saved(m._cid, x.data_ptr(), fmt, out.ptr, n, h, w, saved.ptr, saved.nbytes, _stream()))
    g = EBW.Grads()
    grads = {k: outs(4 * sd[k].numel(), "f32") for k in EBW.PARAMS}
    for k, b in grads.items():
        layer, kind = k.rsplit(".", 1)
        (g.w if kind == "weight" else g.b)[EBW.LAYERS.index(layer)] = b.ptr
    gx = outs(4 * n * 3 * h * w, "f32") if fmt == F32 else None                 # a uint8 input has no input gradient
    if gx is not None:
        g.input = gx.ptr
    ws = outs(WO._size(L.cid_esd_backward_workspace_bytes, n, h, w), "ws")
    assert L.cid_debug_poison_lds(_stream()) == 0
    _lib.check_abi("esd", m._cid, L.cid_esd_backward(m._cid, x.data_ptr(), fmt, ops["grad_logit"].data_ptr(), n, h, w, saved.ptr, saved.nbytes,
                                                     ctypes.byref(g), ws.ptr, ws.nbytes, _stream()))
    torch.cuda.synchronize()
    res = {"logit": out.tensor(torch.float32, (n,))}
    res.update({k: b.tensor(torch.float32, tuple(sd[k].shape)) for k, b in grads.items()})
    if gx is not None:
        res["input"] = gx.tensor(torch.float32, (n, 3, h, w))
    _stage_results(res, saved.bits(), _esd_views(n, h, w), n)
    return res


def _esdb_anchor(ctx, ops, res):
    """The plain run has the bits of test_esrgan_disc_backward's forward_saved + backward, held to float64 by that file's check_rule."""
    shape, ref = ctx["shape"], ctx["ref"]
    m = _esd_module(shape[1:])
    want_input = ctx["fmt"] == "f32"
    logits, saved = TEDB.forward_saved(m, ops["in"])
    grads, gx = TEDB.backward(m, ops["in"], saved, ops["grad_logit"], want_input=want_input, fill=NAN_BYTE)
    assert torch.equal(logits, res["logit"]) and all(torch.equal(grads[k], res[k]) for k in EBW.PARAMS)
    if not want_input:            # the uint8 batch is read as its fp32 copy, whose variant is anchored
        return 0.0
    assert torch.equal(gx, res["input"])
    return TEDB.check_rule(TEDB._cpu(grads), gx.cpu(), TEDB.saved_stages(saved, shape), ref, "real1", f"operand edges {shape}")


# ------------------------------------------------------------------------------------------------ the SRGAN generator in train mode
def _srt_u8(shape, backward):
    """The uint8 source of the family's fp32 input of a case (srgan_train_oracle.case_input / srgan_backward_ref.case_input)."""
    first = STO._FIRST[shape] if (shape in STO.PARITY_CASES or not backward) else 2700
    return synth.srgan_inputs_u8(*shape[:3], first)


@functools.lru_cache(maxsize=None)
def _srt_model(scale):
    sd = synth.make_srgan_state_dict("hot", scale)
    m = TSB.model_of(sd, scale)          # batch statistics, train mode
    m.pack_weights()
    return m, sd


def _srt_layers(m):
    return [(name, layer) for name, layer, _ in m._batchnorms()]


def _srt_load_running(m, res):
    """Put a run's running statistics into the module, for the family's checks that read them there."""
    with torch.no_grad():
        for name, b in _srt_layers(m):
            for f, _ in BN_STATE:
                getattr(b, f).copy_(res[f"{name}.{f}"].reshape(getattr(b, f).shape))


def _srt_make(variant, shape):
    u8 = _srt_u8(shape, False)
    x = STO.case_input(shape)
    assert np.array_equal(x, srgan_oracle.normalise_u8(u8))
    ops = {"in": _dev(u8 if variant == "u8" else x)}
    ops.update(_bn_ops(_srt_layers(_srt_model(shape[3])[0]), True))
    return dict(shape=shape), ops


SRT_STAGES = ("x0", "trunk", "tail_in")


def _srt_run(ctx, ops, outs):
    L = _lib.lib()
    n, h, w, s = ctx["shape"]
    m, sd = _srt_model(s)
    x, layers = ops["in"], _srt_layers(m)
    ws, out = outs(WO._size(L.cid_sr_train_workspace_bytes, n, h, w, s), "ws"), outs(4 * n * 3 * s * h * s * w, "f32")
    bn, state = _bn_array(layers, ops, outs, True, state=sd)         # every run starts from the loaded running statistics
    m._check(L.cid_sr_forward_train(m._cid, x.data_ptr(), U8 if x.dtype == torch.uint8 else F32, out.ptr, F32, n, h, w, 0, bn, ws.ptr,
                                    ws.nbytes, _stream()))
    torch.cuda.synchronize()
    res = {"out": out.tensor(torch.float32, (n, 3, s * h, s * w))}
    res.update(_bn_results("", layers, state))
    _stage_results(res, ws.bits(), _views(L.cid_sr_train_stage_view, SRT_STAGES, n, h, w, s), n)
    return res


def _srt_anchor(ctx, ops, res):
    """As test_srgan_train.py::test_parity_with_the_float64_oracle: stages and running statistics under the oracle's bound, the output
    under max(1e-5, 2 e_aten)."""
    shape = ctx["shape"]
    n, h, w, s = shape
    ref, r32 = STO.reference("hot", shape), STO.reference("hot", shape, torch.float32)
    share = _stage_shares(res, _views(_lib.lib().cid_sr_train_stage_view, SRT_STAGES, n, h, w, s), ref, STO.bound)
    _srt_load_running(_srt_model(s)[0], res)
    TST.check_buffers(_srt_model(s)[0], ref)
    e_aten = float(np.abs(r32["out"].astype(np.float64) - ref["out"]).max())
    return max(share, TST.check("out", res["out"].cpu().numpy(), ref["out"], bound=max(1e-5, 2 * e_aten)))


def _srb_make(variant, shape):
    n, h, w, s = shape
    u8, x = _srt_u8(shape, True), SBR.case_input(shape)
    assert np.array_equal(x, srgan_oracle.normalise_u8(u8))
    ops = {"in": _dev(u8 if variant == "u8" else x), "grad_out": _dev(SBR.grad_out(n, s, h, w))}
    ops.update(_bn_ops(_srt_layers(_srt_model(s)[0]), True))
    return dict(shape=shape, fmt=variant, x=x), ops


def _srb_run(ctx, ops, outs):
    """cid_sr_forward_saved + cid_sr_backward, as test_srgan_backward.cabi."""
    from celebrity_image_denoiser_amd.srgan import _GradsArg, _set_grad

    L = _lib.lib()
    n, h, w, s = ctx["shape"]
    m, sd = _srt_model(s)
    x, layers = ops["in"], _srt_layers(m)
    fmt = U8 if x.dtype == torch.uint8 else F32
    saved, fws = outs(WO._size(L.cid_sr_saved_bytes, n, h, w, s), "ws"), outs(WO._size(L.cid_sr_train_workspace_bytes, n, h, w, s), "ws")
    bws, out = outs(WO._size(L.cid_sr_backward_workspace_bytes, n, h, w, s), "ws"), outs(4 * n * 3 * s * h * s * w, "f32")
    bn, state = _bn_array(layers, ops, outs, True, state=sd)
    m._check(L.cid_sr_forward_saved(m._cid, x.data_ptr(), fmt, out.ptr, n, h, w, 0, bn, saved.ptr, saved.nbytes, fws.ptr, fws.nbytes, _stream()))
    g, grads = _GradsArg(), {}
    for k, p in m.named_parameters():
        grads[k] = outs(4 * p.numel(), "f32")
        _set_grad(g, k, grads[k].ptr)
    assert L.cid_debug_poison_lds(_stream()) == 0
    m._check(L.cid_sr_backward(m._cid, x.data_ptr(), fmt, ops["grad_out"].data_ptr(), n, h, w, 0, bn, saved.ptr, saved.nbytes, ctypes.byref(g),
                               bws.ptr, bws.nbytes, _stream()))
    torch.cuda.synchronize()
    res = {"out": out.tensor(torch.float32, (n, 3, s * h, s * w))}
    res.update(_bn_results("", layers, state))
    res.update({k: grads[k].tensor(torch.float32, tuple(p.shape)) for k, p in m.named_parameters()})
    return res


def _srb_anchor(ctx, ops, res):
    """The plain run has the bits of test_srgan_backward.cabi, running statistics included, held to float64 by that file's
    check_against_float64; the share is that rule's, computed once more here because the check returns none."""
    shape = ctx["shape"]
    m, sd = _srt_model(shape[3])
    TST.restore(m, sd)
    out, grads, masks = TSB.cabi(m, ops["in"], ops["grad_out"])
    assert torch.equal(out, res["out"]) and all(torch.equal(grads[k], res[k]) for k in grads) and len(grads) > 30
    assert all(torch.equal(_bits(v), _bits(res[k].reshape(v.shape))) for k, v in TSB.running(m).items())
    if ctx["fmt"] == "u8":            # the uint8 batch is read as its normalised fp32 copy, whose variant is anchored
        return 0.0
    e_aten, _ = SBR.aten_errors("hot", shape)
    TSB.check_against_float64(sd, ctx["x"], ops["grad_out"], grads, masks, e_aten)
    g64, _, _, book = SBR.ref_backward(sd, ctx["x"], ops["grad_out"].cpu(), torch.float64, masks=masks)
    errs = SBR.rel_errors({k: v.cpu() for k, v in grads.items()}, g64, book)
    return max(e / max(SBR.TOL, 2 * e_aten.get(k, 0.0)) for k, e in errs.items())


# -------------------------------------------------------------------------------------------------------- the five device packs
def _pack_modules(which, hw):
    """(a fresh module that packs on the device, a fresh one that packs on the host) of a family, same weights."""
    if which == "gen":
        return TGB._module("hot", autograd=True), TGB._module("hot")
    if which == "disc":
        return TDB._module("trained", False, autograd=True), TDB._module("trained", False)
    if which == "srd":
        return TSDB._module("trained", False, autograd=True), TSDB._module("trained", False)
    if which == "esd":
        return TEDB._module("trained", hw, autograd=True), TEDB._module("trained", hw)
    from celebrity_image_denoiser_amd.srgan import load_srgan

    sd = synth.make_srgan_state_dict("hot", 4)
    return TSB.model_of(sd, 4), load_srgan(sd, scale_factor=4, device=DEV, strict=True)


def _pack_make(variant, shape):
    m, _ = _pack_modules(variant, shape)
    ops = {k: p.detach().clone() for k, p in m.named_parameters()}
    ops.update({"buffer." + k: b.detach().clone() for k, b in m.named_buffers()})
    return dict(which=variant, hw=shape), ops


def _pack_run(ctx, ops, outs):
    """The module's own device pack (one cid_*_pack_weights_device call) with every parameter's storage replaced by the placed
    operand: the pointers of the call are the operands' own.  The blob is the module's (256-byte aligned by contract)."""
    m, _ = _pack_modules(ctx["which"], ctx["hw"])
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.data = ops[k]
        for k, b in m.named_buffers():
            b.data = ops["buffer." + k]
    blob = m.pack_weights()
    torch.cuda.synchronize()
    assert all(p.data_ptr() == ops[k].data_ptr() for k, p in m.named_parameters())
    assert all(b.data_ptr() == ops["buffer." + k].data_ptr() for k, b in m.named_buffers())
    return {"blob": blob.clone()}


def _pack_anchor(ctx, ops, res):
    """The host pack of the same weights, byte for byte (the families' test_device_pack_equals_*host_pack)."""
    _, host = _pack_modules(ctx["which"], ctx["hw"])
    want = host.pack_weights()
    torch.cuda.synchronize()
    assert want.numel() == res["blob"].numel() and torch.equal(want.view(torch.uint8), res["blob"].view(torch.uint8))
    return 0.0


# ------------------------------------------------------------------------------------------------------------ LPIPS and the VGG loss
PERCEPTUAL = {"lpips": (TL, "cid_lpips", 5), "vgg_lpips": (TLV, "cid_vgg_lpips", 5), "vgg_content": (TLV, "cid_vgg_content_loss", 3)}


def _perc_model(which):
    return TLV.loss_of("hot") if which == "vgg_content" else PERCEPTUAL[which][0].model_of("hot")


def _perc_views(which, n, h, w):
    """The taps' views in the workspace; both towers: 2 N images, tower b after tower a."""
    L = _lib.lib()
    names = TL.lpips_oracle.TAPS[:PERCEPTUAL[which][2]]
    if which == "lpips":
        return [(s,) + WO._view(L.cid_lpips_stage_view, s, n, h, w) for s in names]
    what = _lib.CID_VGG_CONTENT if which == "vgg_content" else _lib.CID_VGG_LPIPS
    return [(s,) + WO._view(lambda stage, *a: L.cid_vgg_stage_view(what, stage, *a), s, n, h, w) for s in names]


def _perc_make(variant, shape):
    which, fmt = variant
    n, h, w = shape
    a, b, a8, b8 = PERCEPTUAL[which][0].pairs_of("noisy", (h, w, n))
    return dict(which=which, shape=shape, a=a, b=b), {"a": _dev(np.array(a8 if fmt == "u8" else a)), "b": _dev(np.array(b8 if fmt == "u8" else b))}


def _perc_run(ctx, ops, outs):
    L, which = _lib.lib(), ctx["which"]
    n, h, w = ctx["shape"]
    m = _perc_model(which)
    a, b = ops["a"], ops["b"]
    fa, fb = (U8 if a.dtype == torch.uint8 else F32), (U8 if b.dtype == torch.uint8 else F32)
    out = outs(8 * n, "f64")
    if which == "lpips":
        ws, lay = outs(WO._size(L.cid_lpips_workspace_bytes, n, h, w), "ws"), outs(8 * n * 5, "f64")
        _lib.check_lpips(m._cid, L.cid_lpips(m._cid, a.data_ptr(), fa, b.data_ptr(), fb, n, h, w, _lib.CID_LPIPS_UNIT_VIEW, out.ptr, lay.ptr,
                                             ws.ptr, ws.nbytes, _stream()))
    elif which == "vgg_lpips":
        ws, lay = outs(WO._size(L.cid_vgg_workspace_bytes, _lib.CID_VGG_LPIPS, n, h, w), "ws"), outs(8 * n * 5, "f64")
        _lib.check_vgg(m._cid, L.cid_vgg_lpips(m._cid, a.data_ptr(), fa, b.data_ptr(), fb, n, h, w, _lib.CID_LPIPS_UNIT_VIEW, out.ptr, lay.ptr,
                                               ws.ptr, ws.nbytes, _stream()))
    else:
        ws, lay = outs(WO._size(L.cid_vgg_workspace_bytes, _lib.CID_VGG_CONTENT, n, h, w), "ws"), None
        _lib.check_vgg(m._cid, L.cid_vgg_content_loss(m._cid, a.data_ptr(), fa, b.data_ptr(), fb, n, h, w, 0, out.ptr, ws.ptr, ws.nbytes,
                                                      _stream()))
    torch.cuda.synchronize()
    res = {"out": out.tensor(torch.float64, (n,))}
    if lay is not None:
        res["layers"] = lay.tensor(torch.float64, (n, 5))
    raw = ws.bits()
    for name, off, c, hs, wss in _perc_views(which, n, h, w):
        both = raw[off:off + 4 * 2 * n * c * hs * wss].view(2, n, -1)          # tower b's N images follow tower a's
        res["stage." + name] = both.permute(1, 0, 2).contiguous()                # -> [N, tower, bytes]: an image's two taps together
    return res


def _rel_share(got, want):
    """The families' rule |got - want| <= 1e-5 |want| (test_lpips.check_distances, test_lpips_vgg.check_values) as a share."""
    return float((np.abs(got - want) / (1e-5 * np.abs(want))).max())


def _perc_anchor(ctx, ops, res):
    which = ctx["which"]
    if which == "vgg_content":
        ref = TLV.oracle.content(TLV.oracle.weights("hot"), ctx["a"], ctx["b"])
        TLV.check_values(res["out"].cpu().numpy(), ref["loss"], "content loss")
        return _rel_share(res["out"].cpu().numpy(), ref["loss"])
    d, layers = res["out"].cpu().numpy(), res["layers"].cpu().numpy()
    if which == "lpips":
        ref = TL.lpips_oracle.forward(synth.make_lpips_state_dict("hot"), ctx["a"], ctx["b"], True)
        TL.check_distances(d, layers, ref, "lpips")
    else:
        ref = TLV.oracle.forward(TLV.oracle.weights("hot"), ctx["a"], ctx["b"], True)
        TLV.check_values(layers, ref["layers"], "vgg layers")
        TLV.check_values(d, ref["d"], "vgg d")
    return max(_rel_share(d, ref["d"]), _rel_share(layers, ref["layers"]))


def _vggb_make(variant, shape):
    n, h, w = shape
    a, b, _, b8 = TVB.pairs_of("noisy", (h, w, n))
    go = torch.full((n,), 1.0 / n, dtype=torch.float64)               # the trainer's scalar: the mean over the batch
    return dict(shape=shape, fmt=variant, go=go), {"a": _dev(np.array(a)), "b": _dev(np.array(b8 if variant == "u8" else b)), "grad_out": _dev(go)}


def _vggb_run(ctx, ops, outs):
    L = _lib.lib()
    n, h, w = ctx["shape"]
    m = TVB.loss_of("hot")
    m.pack_weights()
    m._pack_backward_weights()
    a, b = ops["a"], ops["b"]
    arena, out, gx = outs(TVB.saved_bytes(n, h, w), "ws"), outs(8 * n, "f64"), outs(4 * n * 3 * h * w, "f32")
    _lib.check_vgg(m._cid, L.cid_vgg_content_loss_saved(m._cid, a.data_ptr(), F32, b.data_ptr(), U8 if b.dtype == torch.uint8 else F32, n, h, w, 0,
                                                        out.ptr, arena.ptr, arena.nbytes, _stream()))
    assert L.cid_debug_poison_lds(_stream()) == 0
    _lib.check_vgg(m._cid, L.cid_vgg_content_backward(m._cid, ops["grad_out"].data_ptr(), gx.ptr, n, h, w, 0, arena.ptr, arena.nbytes, _stream()))
    torch.cuda.synchronize()
    return {"out": out.tensor(torch.float64, (n,)), "grad_a": gx.tensor(torch.float32, (n, 3, h, w))}


def _vggb_anchor(ctx, ops, res):
    """The plain run has the bits of test_vgg_backward.cabi, and that file's check_gradients holds grad_a and the seven stored gradient
    tensors of the arena to float64 under its rule (it asserts and prints its margins; it returns no share)."""
    n, h, w = ctx["shape"]
    out, gx, arena = TVB.cabi(TVB.loss_of("hot"), ops["a"], ops["b"], ctx["go"], fmt_b=U8 if ctx["fmt"] == "u8" else F32)
    assert torch.equal(out, res["out"]) and torch.equal(gx, res["grad_a"])
    if ctx["fmt"] == "u8":
        return 0.0
    TVB.check_gradients("hot", "noisy", (h, w, n), False, ctx["go"].numpy(), gx, arena, f"operand edges {ctx['shape']}")
    ref = TLV.oracle.content(TLV.oracle.weights("hot"), *TVB.pairs_of("noisy", (h, w, n))[:2])
    return _rel_share(res["out"].cpu().numpy(), ref["loss"])


# ------------------------------------------------------------------------------------------------------------------------ the table
class Row:
    """One launching entry point (or a forward_saved + backward pair) of include/cid.h.
    entry     the functions of the header the row covers
    operands  {name: element type} of its read-only device operands; outputs likewise
    couples   None for a per-image row, else why its results couple the batch (Part B does not apply)
    shapes    (the smallest the entry point accepts, the smallest ragged multi-tile shape of the family's parity list with N = 3)
    variants  callers' formats, modes and algorithms the row runs in
    images    operands Part B poisons image by image; grads: the backward's upstream-gradient operands, poisoned in a second variant
    local     the results that belong to one image each (leading dimension N); grad_local: those a poisoned upstream gradient reaches
    make      (variant, shape) -> (context, {operand: plain device tensor}); run: (context, placed operands, Outs) -> {name: result};
    anchor    (context, operands, plain results) -> the worst share of the family's oracle bound, asserted to be at most 1"""

    def __init__(self, name, entry, operands, outputs, shapes, couples=None, variants=(None,), images=(), grads=(), local=(), grad_local=(),
                 make=None, run=None, anchor=None, note=""):
        self.name, self.entry, self.operands, self.outputs, self.shapes, self.couples = name, tuple(entry), operands, outputs, shapes, couples
        self.variants, self.images, self.grads, self.local, self.grad_local = variants, images, grads, local, grad_local
        self.make, self.run, self.anchor, self.note = make, run, anchor, note


BATCH_SUM = "a sum or mean over the batch"
GEN_SHAPES = ((1, 4, 4), (3, 20, 24))
DISC_SHAPES = ((1, 1, 1), (3, 37, 53))
_STAGES = lambda names: tuple("stage." + s for s in names)   # noqa: E731

TABLE = [
    Row("forward_ex", ["cid_forward_ex", "cid_forward"], {"in": "f32 | u8"}, {"out": "f32 | u8"}, GEN_SHAPES,
        variants=tuple((f, d, a) for f in ("f32", "u8") for d in ("f32", "f16") for a in ("winograd42", "direct")),
        images=("in",), local=("out",), make=_fwd_make, run=_fwd_run, anchor=_fwd_anchor,
        note="cid_forward is cid_forward_ex(F32_NCHW, F32_NCHW); the caller's format is that of both the input and the output"),
    Row("forward_padded", ["cid_forward_padded"], {"in": "f32 | u8"}, {"out": "f32"}, tuple(PADS), variants=("f32", "u8"),
        images=("in",), local=("out",), make=_pad_make, run=_pad_run, anchor=_pad_anchor),
    Row("view_u8", ["cid_view_u8"], {"in": "f32"}, {"out": "u8"}, GEN_SHAPES, images=("in",), local=("out",),
        make=_view_make, run=_view_run, anchor=_view_anchor),
    Row("forward_saved+backward", ["cid_forward_saved", "cid_backward"], {"in": "f32", "grad_out": "f32"},
        {"y": "f32", "input": "f32", "24 parameter gradients": "f32"}, GEN_SHAPES, images=("in",), grads=("grad_out",),
        local=("y", "input") + _STAGES(GEN_STAGES), grad_local=("input",), make=_bwd_make, run=_bwd_run, anchor=_bwd_anchor,
        note="the parameter gradients couple the batch (" + BATCH_SUM + "): Parts A and C only; y, the saved stages and the input "
             "gradient are per image"),
    Row("disc eval", ["cid_disc_forward", "cid_disc_forward_saved", "cid_disc_backward"],
        {"in": "f32 | u8", "grad_prob": "f32", "BatchNorm gamma, beta": "f32", "BatchNorm running_mean, running_var": "f32", "BatchNorm num_batches_tracked": "i64"},
        {"p": "f32", "input": "f32", "16 parameter gradients": "f32"}, DISC_SHAPES, variants=(("disc", "f32", False), ("disc", "u8", False)),
        images=("in",), grads=("grad_prob",), local=("p", "p_plain", "input"), grad_local=("input",),
        make=_bnd_make, run=_bnd_run, anchor=_bnd_anchor,
        note="training = 0; a uint8 input has no input gradient; every pointer of cid_disc_bn[3] is a placed operand"),
    Row("disc train", ["cid_disc_forward", "cid_disc_forward_saved", "cid_disc_backward"], {"in": "f32 | u8", "grad_prob": "f32", "BatchNorm gamma, beta": "f32"},
        {"p": "f32", "input": "f32", "16 parameter gradients": "f32", "BatchNorm running_mean, running_var (in/out)": "f32", "BatchNorm num_batches_tracked (in/out)": "i64"}, (TRAIN_MIN, (3, 37, 53)),
        couples="train-mode BatchNorm: statistics over the batch", variants=(("disc", "f32", True), ("disc", "u8", True)),
        make=_bnd_make, run=_bnd_run, anchor=_bnd_anchor,
        note="training = 1; the running statistics and the counter are in/out, placed like cid_adam_step's state; _bnd_anchor says what "
             "holds (2, 1, 1)"),
    Row("quality", ["cid_quality"], {"a": "u8", "b": "f32"}, {"out": "f64"}, ((1, 7, 7), (3, 13, 18)), images=("b",),
        local=("psnr", "ssim"), make=_quality_make, run=_quality_run, anchor=_quality_anchor,
        note="test_quality.py::test_nan_stays_in_its_image stays; this row adds the guards and the alignments"),
    Row("losses", ["cid_disc_losses", "cid_srd_losses", "cid_esd_losses", "cid_esd_trainer_losses"],
        {"real": "f32", "fake": "f32", "denoised": "f32", "clean": "u8"}, {"out": "f64"}, ((1, 1, 1), (3, 37, 53)), couples=BATCH_SUM,
        variants=("disc", "srd", "esd", "esd_trainer"), make=_loss_make, run=_loss_run, anchor=_loss_anchor),
    Row("add_noise", ["cid_add_noise"], {"clean": "u8"}, {"out": "u8"}, ((1, 2, 2), (3, 37, 53)), variants=tuple(NOISE_KINDS),
        make=_noise_make, run=_noise_run, anchor=_noise_anchor,
        note="per image (test_noise.py::test_batch_independence), but uint8 only: no NaN to poison an image with, so no Part B"),
    Row("resize", ["cid_resize"], {"src": "u8"}, {"dst": "u8 | f32"}, ((3, 3, 8, 8), (37, 53, 16, 16)), variants=("u8", "f32"),
        make=_resize_make, run=_resize_run, anchor=_resize_anchor,
        note="shapes are (Hs, Ws, Hd, Wd) of test_resize.py's fixtures, three images each; uint8 only, so no Part B"),
    Row("adam_step", ["cid_adam_step"], {"grad": "f32"}, {"param": "f32", "exp_avg": "f32", "exp_avg_sq": "f32"}, ((1,), (4097,)),
        couples="no images", variants=(0.0, 1e-2), make=_adam_make, run=_adam_run, anchor=_adam_anchor,
        note="test_adam.py's RESIDUES table runs every 4-byte residue, equal and mixed, between NaN canaries; this row adds the "
             "4 KiB guards and the residues +4 / +12 with the gradient alone offset (the scalar path)"),
    Row("esr_forward", ["cid_esr_forward"], {"in": "f32 | u8"}, {"out": "f32"}, ((1, 1, 1), (3, 37, 53)), variants=("f32", "u8"),
        images=("in",), local=("out",) + _STAGES(ESR_STAGES), make=_esr_make, run=_esr_run, anchor=_esr_anchor),
    Row("sr_forward", ["cid_sr_forward"], {"in": "f32 | u8"}, {"out": "f32"}, ((1, 1, 1, 4), (3, 13, 18, 4)), variants=("f32", "u8"),
        images=("in",), local=("out",) + _STAGES(SR_STAGES), make=_sr_make, run=_sr_run, anchor=_sr_anchor),
    Row("cg_forward", ["cid_cg_forward"], {"z": "f32", "labels": "i64"}, {"out": "f32"}, ((1,), (3,)),
        images=("z",), local=("out",) + _STAGES(CG_STAGES), make=_cg_make, run=_cg_run, anchor=_cg_anchor),
    Row("esd_forward", ["cid_esd_forward"], {"in": "f32 | u8"}, {"logit": "f32"}, ((1, 1, 1), (3, 37, 53)), variants=("f32", "u8"),
        images=("in",), local=("logit",) + _STAGES(("a1", "a2", "a3", "a4")), make=_esd_make, run=_esd_run, anchor=_esd_anchor),
    Row("esd_forward_saved+backward", ["cid_esd_forward_saved", "cid_esd_backward"], {"in": "f32 | u8", "grad_logit": "f32"},
        {"logit": "f32", "input": "f32", "10 parameter gradients": "f32"}, ((2, 1, 1), (3, 37, 53)), variants=("f32", "u8"),
        images=("in",), grads=("grad_logit",), local=("logit", "input") + _STAGES(("a1", "a2", "a3", "a4")), grad_local=("input",),
        make=_esdb_make, run=_esdb_run, anchor=_esdb_anchor,
        note="(2, 1, 1) is the smallest shape of the family's parity list; the parameter gradients couple the batch (" + BATCH_SUM + ")"),
    Row("srd eval", ["cid_srd_forward", "cid_srd_forward_saved", "cid_srd_backward"], {"in": "f32 | u8", "grad_prob": "f32", "BatchNorm gamma, beta": "f32", "BatchNorm running_mean, running_var": "f32", "BatchNorm num_batches_tracked": "i64"},
        {"p": "f32", "input": "f32", "22 parameter gradients": "f32"}, ((2, 1, 1), (3, 41, 70)),
        variants=(("srd", "f32", False), ("srd", "u8", False)),
        images=("in",), grads=("grad_prob",), local=("p", "p_plain", "input"), grad_local=("input",),
        make=_bnd_make, run=_bnd_run, anchor=_bnd_anchor,
        note="training = 0; (2, 1, 1) is the smallest shape of test_srgan_disc.py; every pointer of cid_disc_bn[4] is a placed operand"),
    Row("srd train", ["cid_srd_forward", "cid_srd_forward_saved", "cid_srd_backward"], {"in": "f32 | u8", "grad_prob": "f32", "BatchNorm gamma, beta": "f32"},
        {"p": "f32", "input": "f32", "22 parameter gradients": "f32", "BatchNorm running_mean, running_var (in/out)": "f32", "BatchNorm num_batches_tracked (in/out)": "i64"}, (TRAIN_MIN, (3, 41, 70)),
        couples="train-mode BatchNorm: statistics over the batch", variants=(("srd", "f32", True), ("srd", "u8", True)),
        make=_bnd_make, run=_bnd_run, anchor=_bnd_anchor,
        note="training = 1; at (2, 1, 1) the batch is the family's first well-conditioned draw (test_srgan_disc._train_case)"),
    Row("lpips", ["cid_lpips"], {"a": "f32 | u8", "b": "f32 | u8"}, {"out": "f64", "layers": "f64"}, ((1, 31, 31), (3, 35, 47)),
        variants=(("lpips", "f32"), ("lpips", "u8")), images=("a", "b"), local=("out", "layers") + _STAGES(TL.lpips_oracle.TAPS),
        make=_perc_make, run=_perc_run, anchor=_perc_anchor, note="CID_LPIPS_UNIT_VIEW, the trainers' call; image k of a, then of b, is poisoned: tower b follows tower a in the workspace"),
    Row("vgg_lpips", ["cid_vgg_lpips"], {"a": "f32 | u8", "b": "f32 | u8"}, {"out": "f64", "layers": "f64"}, ((1, 16, 16), (3, 17, 19)),
        variants=(("vgg_lpips", "f32"), ("vgg_lpips", "u8")), images=("a", "b"), local=("out", "layers") + _STAGES(TL.lpips_oracle.TAPS),
        make=_perc_make, run=_perc_run, anchor=_perc_anchor),
    Row("vgg_content_loss", ["cid_vgg_content_loss"], {"a": "f32 | u8", "b": "f32 | u8"}, {"out": "f64"}, ((1, 4, 4), (3, 5, 7)),
        variants=(("vgg_content", "f32"), ("vgg_content", "u8")), images=("a", "b"), local=("out",) + _STAGES(TL.lpips_oracle.TAPS[:3]),
        make=_perc_make, run=_perc_run, anchor=_perc_anchor, note="out holds one loss per image pair; the module takes their mean"),
    Row("vgg_content_loss_saved+backward", ["cid_vgg_content_loss_saved", "cid_vgg_content_backward"],
        {"a": "f32", "b": "f32 | u8", "grad_out": "f64"}, {"out": "f64", "grad_a": "f32"}, ((1, 4, 4), (3, 5, 7)), variants=("f32", "u8"),
        images=("a", "b"), grads=("grad_out",), local=("out", "grad_a"), grad_local=("grad_a",),
        make=_vggb_make, run=_vggb_run, anchor=_vggb_anchor, note="the variant is operand b's format; a is fp32 by the header"),
    Row("sr_forward_train", ["cid_sr_forward_train"], {"in": "f32 | u8", "BatchNorm gamma, beta": "f32"}, {"out": "f32", "BatchNorm running_mean, running_var (in/out)": "f32", "BatchNorm num_batches_tracked (in/out)": "i64"},
        ((1, 5, 7, 2), (3, 8, 12, 2)), couples="train-mode BatchNorm: statistics over the batch", variants=("f32", "u8"),
        make=_srt_make, run=_srt_run, anchor=_srt_anchor,
        note="(1, 5, 7, 2) is the smallest shape of the family's parity list; (1, 1, 2, 2) is accepted but has two values per channel, "
             "which test_srgan_train.py::test_two_values_per_channel holds under a rule of its own"),
    Row("sr_forward_saved+backward", ["cid_sr_forward_saved", "cid_sr_backward"], {"in": "f32 | u8", "grad_out": "f32", "BatchNorm gamma, beta": "f32"},
        {"out": "f32", "every parameter gradient": "f32", "BatchNorm running_mean, running_var (in/out)": "f32", "BatchNorm num_batches_tracked (in/out)": "i64"}, ((1, 5, 7, 2), (3, 8, 12, 2)),
        couples="train-mode BatchNorm: statistics over the batch", variants=("f32", "u8"),
        make=_srb_make, run=_srb_run, anchor=_srb_anchor, note="the entry points have no eval mode and no input gradient"),
    Row("pack_weights_device", ["cid_pack_weights_device", "cid_disc_pack_weights_device", "cid_srd_pack_weights_device",
                                "cid_esd_pack_weights_device", "cid_sr_pack_weights_device"], {"every parameter tensor": "f32", "BatchNorm buffers": "f32", "BatchNorm counters": "i64"},
        {"device_blob": "blob"}, ((1, 1), (37, 53)), couples="no images", variants=("gen", "disc", "srd", "esd", "sr"),
        make=_pack_make, run=_pack_run, anchor=_pack_anchor,
        note="the parameter tensors (BatchNorm's gamma and beta among them) and the modules' BatchNorm buffers, which "
             "cid_sr_pack_weights_device takes through its bn argument, are the read-only operands; "
             "the blob is documented at 256 bytes and stays there; the shapes are "
             "the ESRGAN discriminator's (H, W), the other four packs do not depend on one"),
]
ROWS = {r.name: r for r in TABLE}
assert len(ROWS) == len(TABLE)

# Functions of include/cid.h with a `void* stream` parameter that are no row, each with its reason.
EXEMPT = {
    "cid_upload_weights": "upload: host-staged weights to a 256-byte aligned blob, no caller-supplied device operand",
    "cid_disc_upload_weights": "upload, as cid_upload_weights",
    "cid_srd_upload_weights": "upload, as cid_upload_weights",
    "cid_esd_upload_weights": "upload, as cid_upload_weights",
    "cid_esr_upload_weights": "upload, as cid_upload_weights",
    "cid_sr_upload_weights": "upload, as cid_upload_weights",
    "cid_cg_upload_weights": "upload, as cid_upload_weights",
    "cid_lpips_upload_weights": "upload, as cid_upload_weights",
    "cid_vgg_upload_weights": "upload, as cid_upload_weights",
    "cid_vgg_upload_backward_weights": "upload, as cid_upload_weights",
    "cid_broadcast_weights": "RCCL broadcast of the attached blob: no kernel of this library reads a caller's operand",
    "cid_forward_timed": "cid_forward with events around its launches: the same kernels as the forward_ex row",
    "cid_timing_end": "reads back event times: no device operand",
    "cid_cg_latent": "writes z from (seed, index): no read-only operand",
    "cid_debug_poison_lds": "debug call: no operand",
    "cid_disc_saved_masks": "debug view of a saved buffer (256-byte aligned by contract) for the tests' float64 references",
    "cid_srd_saved_masks": "debug view of a saved buffer, as cid_disc_saved_masks",
    "cid_sr_saved_masks": "debug view of a saved buffer, as cid_disc_saved_masks",
}


CASES = [(r.name, v, s) for r in TABLE for v in r.variants for s in r.shapes]


def _id(case):
    name, v, s = case
    vs = "" if v is None else "-" + ("-".join(str(t) for t in v) if isinstance(v, tuple) else str(v))
    return f"{name.replace(' ', '_')}{vs}-{'x'.join(map(str, s))}"


@functools.lru_cache(maxsize=None)
def plain(case):
    """(ctx, operands, results, share) of the plain run of a case, anchored to the family's float64 oracle: made once, only read."""
    name, variant, shape = case
    row = ROWS[name]
    ctx, ops = row.make(variant, shape)
    res = execute(row, ctx, ops, Place())
    for k, t in res.items():
        assert not t.dtype.is_floating_point or bool(torch.isfinite(t).all()), (case, k)
    share = row.anchor(ctx, ops, res)
    print(f"\nanchor {_id(case)}: worst share of the oracle bound {share:.3f}")
    return ctx, ops, res, share


# --------------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_part_a_operands_between_nan_guards(case):
    ctx, ops, want, _ = plain(case)
    row = ROWS[case[0]]
    nan = execute(row, ctx, ops, Place(NAN_BYTE))
    zero = execute(row, ctx, ops, Place(ZERO_BYTE))
    same_bits(nan, zero, (case, "0xFF against 0x00 guards"))
    same_bits(nan, want, (case, "guarded against plain"))


@pytest.mark.gpu
@pytest.mark.parametrize("outputs_too", (True, False), ids=("all_pointers", "operands_only"))
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_part_c_every_admitted_alignment(case, outputs_too):
    ctx, ops, want, _ = plain(case)
    row = ROWS[case[0]]
    for j in (0, 1):
        got = execute(row, ctx, ops, Place(NAN_BYTE, j, outputs_too))
        same_bits(got, want, (case, "offsets", j, outputs_too))


B_CASES = [(r.name, v, r.shapes[1]) for r in TABLE if r.couples is None and r.images for v in r.variants
           if "u8" not in (v if isinstance(v, tuple) else (v,))]          # the fp32 callers: a uint8 image has no NaN


def _poisoned(t, k, bits):
    """`t` with image k all quiet NaN or +Inf (`bits`: the fp32 pattern; an fp64 operand takes the same value)."""
    out = t.clone()
    out[k] = torch.tensor(bits, dtype=torch.int32).view(torch.float32).item()
    if t.dtype == torch.float32:
        assert bool((out[k].reshape(-1).view(torch.int32) == bits).all())
    else:
        assert t.dtype == torch.float64 and not bool(torch.isfinite(out[k]).any())
    return out


def _others_equal(got, want, names, k, what):
    """Every image but k of the per-image results `names` has the clean bits; image k differs in at least one of them."""
    differs = False
    for name in names:
        assert name in want and name in got, (what, name, "is not a result of this row")
        n = want[name].shape[0]
        for i in range(n):
            eq = torch.equal(_bits(got[name][i]), _bits(want[name][i]))
            if i != k:
                assert eq, (what, name, "image", i, "changed when image", k, "was poisoned")
            differs = differs or not eq
    assert differs, (what, "image", k, "did not change: the case is vacuous")


@pytest.mark.gpu
@pytest.mark.parametrize("poison", (QNAN_BITS, INF_BITS), ids=("nan", "inf"))
@pytest.mark.parametrize("case", B_CASES, ids=_id)
def test_part_b_a_poisoned_image_stays_in_its_image(case, poison):
    ctx, ops, want, _ = plain(case)
    row = ROWS[case[0]]
    n = ops[row.images[0]].shape[0]
    assert n == 3
    for k in range(n):
        for name in row.images + row.grads:                      # one operand at a time
            if ops[name].dtype == torch.uint8:                   # operand b of the VGG backward's uint8 variant
                continue
            bad = dict(ops)
            bad[name] = _poisoned(ops[name], k, poison)
            _others_equal(execute(row, ctx, bad, Place()), want, row.grad_local if name in row.grads else row.local, k, (case, name))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ("f32", "f16"))
def test_part_b_poison_across_the_winograd_walk(dtype):
    """The (37, 100, 76) batch of test_gpu_parity.py::test_walking_workgroups_equal_one_item_per_workgroup (75 tiles per image, walkers
    straddle images): images 0, 17 and 36 poisoned in turn, compared on the device; only booleans reach the host.  The clean run is
    anchored by that test (f32) and by test_fp16_ragged_shapes_and_long_walks (f16); here its image 36 is held to the oracle again."""
    from oracle import torch_oracle

    m, wset = _generator(dtype, "winograd42")
    x, _, _ = synth.make_batch(37, 100, 76, first_index=8100)
    xd = _dev(x)
    clean = m(xd).clone()
    ref = torch_oracle.forward(synth.make_state_dict(wset), x[36:37]).numpy()
    WO._share("image 36", clean[36:37].cpu().numpy(), ref, TGP.TOL if dtype == "f32" else F16_TOL[wset])
    keep = torch.ones(37, dtype=torch.bool, device=DEV)
    for bits in (QNAN_BITS, INF_BITS):
        for k in (0, 17, 36):
            got = m(_poisoned(xd, k, bits))
            keep.fill_(True)
            keep[k] = False
            same = bool(torch.equal(got[keep].view(torch.int32), clean[keep].view(torch.int32)))
            changed = not bool(torch.equal(got[k].view(torch.int32), clean[k].view(torch.int32)))
            assert same, (dtype, hex(bits), "an image other than", k, "changed")
            assert changed, (dtype, hex(bits), k, "vacuous")


# ------------------------------------------------------------------------------------------------------------------ the Python layer
def _offset_view(t):
    """`big[1:]` for a flat `big` of t.numel() + 1 elements, shaped like t: a contiguous view with storage offset 1, whose data_ptr()
    is 4-byte but not 16-byte aligned (8-byte for int64, odd for uint8).  A module that passes the storage's base pointer, or that
    assumes torch's allocation alignment, computes something else on it than on its clone."""
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = big[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.storage_offset() == 1 and v.data_ptr() % 16 == t.element_size() % 16
    return v


def _with_grads(m, y, upstream, leaves):
    """Backward of `y` under `upstream` -> [y, the leaves' gradients, every parameter's gradient], all copies."""
    m.zero_grad(set_to_none=True)
    y.backward(upstream)
    return [y.detach().clone()] + [t.grad.clone() for t in leaves] + [p.grad.clone() for p in m.parameters() if p.grad is not None]


def _seeded(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV, dtype)


def _py_generator():
    m = TGB._module("hot", autograd=True)          # what cid.load(..., autograd=True) returns
    x = _dev(synth.make_batch(3, 20, 24, first_index=47)[0])

    def run(x):
        plain = _generator("f32", "winograd42")[0](x).clone()                   # cid.load(...): the serving forward
        leaf = x.detach().requires_grad_(True)
        assert leaf.data_ptr() == x.data_ptr()
        return [plain] + _with_grads(m, m(leaf), _seeded((3, 3, 20, 24), 1), [leaf])
    return run, [x]


def _py_disc(module, x):
    def run(x):
        leaf = x.detach().requires_grad_(True)
        assert leaf.data_ptr() == x.data_ptr()
        p = module(leaf)
        return _with_grads(module, p, _seeded(tuple(p.shape), 2), [leaf])
    return run, [x]


def _py_srgan_train():
    m, sd = _srt_model(2)
    x = _dev(STO.case_input((3, 8, 12, 2)))

    def run(x):
        TST.restore(m, sd)
        y = m(x)
        return _with_grads(m, y, _dev(SBR.grad_out(3, 2, 8, 12)), []) + list(TSB.running(m).values())
    return run, [x]


def _py_vgg_loss():
    m = TVB.loss_of("hot")
    a, b, _, _ = TVB.pairs_of("noisy", (5, 7, 3))

    def run(a, b):
        leaf = a.detach().requires_grad_(True)
        assert leaf.data_ptr() == a.data_ptr()
        loss = m(leaf, b)
        return _with_grads(m, loss, torch.ones_like(loss), [leaf])
    return run, [_dev(np.array(a)), _dev(np.array(b))]


def _py_pairs(mod, case):
    a, b, _, _ = mod.pairs_of("noisy", case)
    return [_dev(np.array(a)), _dev(np.array(b))]


def _py_cgan():
    import test_cgan as TC

    z, labels = synth.cgan_latent_np(3, TC.SEED, 300), TC.labels_of(3, CG_CLASSES)
    return (lambda z, lab: [_cg_model()[0](z, lab)]), [_dev(z), _dev(np.asarray(labels, np.int64))]


def _py_quality():
    from celebrity_image_denoiser_amd import metrics

    a, b = H._quality_inputs((3, 13, 18))
    return (lambda a, b: list(metrics.quality(a, b, ("psnr", "ssim")).values())), [a, b]


def _py_noise():
    from celebrity_image_denoiser_amd import noise
    import test_noise as TN

    return (lambda c: [noise.add_noise(c, "gaussian", seed=12345, first_index=77)]), [_dev(TN._inputs(3, 37, 53, 537))]


def _py_resize():
    import celebrity_image_denoiser_amd as cid

    x, _ = TR._case((37, 53, 16, 16))
    return (lambda s: [cid.resize(s, (16, 16), out="u8"), cid.resize(s, (16, 16), out="f32")]), [_dev(np.array(x))]


PY_MODULES = {
    "cid.load": _py_generator,
    "DenoiseDiscriminator": lambda: _py_disc(TDB._module("trained", False, autograd=True), _dev(TD.images(3, 37, 53, first_index=93)[1])),
    "SRGANDiscriminator": lambda: _py_disc(TSDB._module("trained", False, autograd=True), _dev(TSD._batch((3, 41, 70))[1])),
    "ESRGANDiscriminator": lambda: _py_disc(TEDB._module("trained", (37, 53), autograd=True),
                                            _dev(esrgan_disc_oracle.case("trained", (3, 37, 53))[1])),
    "ESRGANGenerator": lambda: ((lambda x: [_esr_model()[0](x)]), [_esr_make("f32", (3, 37, 53))[1]["in"]]),
    "SRGANGenerator": lambda: ((lambda x: [_sr_model(4)[0](x)]), [_sr_make("f32", (3, 13, 18, 4))[1]["in"]]),
    "SRGANGenerator-train": _py_srgan_train,
    "CGANGenerator": _py_cgan,
    "LPIPS-alex": lambda: ((lambda a, b: list(TL.model_of("hot").distances(a, b, unit_view=True, per_layer=True))), _py_pairs(TL, (35, 47, 3))),
    "LPIPS-vgg": lambda: ((lambda a, b: list(TLV.model_of("hot").distances(a, b, unit_view=True, per_layer=True))), _py_pairs(TLV, (17, 19, 3))),
    "VGGPerceptualLoss": _py_vgg_loss,
    "metrics.quality": _py_quality,
    "noise.add_noise": _py_noise,
    "resize.resize": _py_resize,
}


@pytest.mark.gpu
@pytest.mark.parametrize("module", PY_MODULES, ids=lambda s: s)
def test_python_layer_on_a_view_with_a_storage_offset(module):
    """Each Python module once on a contiguous view with a non-zero storage offset: the results, and for the autograd modules the
    input and parameter gradients, are the bits of the same call on a clone of that view.  (Each module's own tests anchor the call.)"""
    run, inputs = PY_MODULES[module]()
    views = [_offset_view(t) for t in inputs]
    got = [t.clone() for t in run(*views)]
    want = run(*[v.clone() for v in views])
    torch.cuda.synchronize()
    assert len(got) == len(want) and len(got) >= 1
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and torch.equal(_bits(g), _bits(w)), (module, i)
        assert not g.dtype.is_floating_point or bool(torch.isfinite(g).all()), (module, i)
