"""tests/test_operand_edges.py's Parts A and C for the ESRGAN generator's backward family: cid_esr_forward_saved + cid_esr_backward as one
row (train-mode BatchNorm couples the batch, so Part B does not apply) and cid_esr_pack_weights_device as another, on that file's
machinery (ReadOnly operands between NaN / zero guards, every admitted alignment, bit comparison with the plain run, which is anchored
to the family's float64 reference under the family's own rule, tests/test_esrgan_backward.py).

test_operand_edges_host.py asks every launching function of include/cid.h for a row of test_operand_edges.TABLE or a place in its
EXEMPT dict with a reason.  This module enters the four functions there when it is imported, which pytest does for every test module
before the first test runs: the reason of three is that their rows are here, of cid_esr_saved_masks that it is a debug view."""
import ctypes
import os
import sys

import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth
from celebrity_image_denoiser_amd.esrgan import _GradsArg, _set_grad, load_esrgan

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import esrgan_backward_ref as REF  # noqa: E402
import esrgan_train_oracle as ETO  # noqa: E402
import test_esrgan_backward as TEB  # noqa: E402
import test_operand_edges as OE  # noqa: E402

_HERE = "its row, with Parts A and C, is tests/test_operand_edges_esrgan_backward.py"
for _fn in ("cid_esr_forward_saved", "cid_esr_backward", "cid_esr_pack_weights_device"):
    OE.EXEMPT.setdefault(_fn, _HERE)
OE.EXEMPT.setdefault("cid_esr_saved_masks", "debug view of a saved buffer, as cid_disc_saved_masks")

R = 3                          # r_0 and r_1 are stored, both G tensors of the backward are in use
_MODEL = []


def _model():
    if not _MODEL:
        sd = synth.make_esrgan_state_dict("hot", R)
        m = TEB.model_of(sd, R)
        m.pack_weights()
        _MODEL.append((m, sd))
    return _MODEL[0]


def _layers(m):
    return [(name, layer) for name, layer, _ in m._batchnorms()]


def _make(variant, shape):
    n, h, w = shape
    ops = {"in": OE._dev(REF.case_u8(shape) if variant == "u8" else ETO.case_input(shape)), "grad_out": OE._dev(REF.grad_out(n, h, w))}
    ops.update(OE._bn_ops(_layers(_model()[0]), True))
    return dict(shape=shape, fmt=variant), ops


def _run(ctx, ops, outs):
    """cid_esr_forward_saved + cid_esr_backward, as test_esrgan_backward.cabi."""
    L = _lib.lib()
    n, h, w = ctx["shape"]
    m, sd = _model()
    x, layers = ops["in"], _layers(m)
    fmt = OE.U8 if x.dtype == torch.uint8 else OE.F32
    saved, fws = outs(OE.WO._size(L.cid_esr_saved_bytes, n, h, w, R), "ws"), outs(OE.WO._size(L.cid_esr_train_workspace_bytes, n, h, w, R), "ws")
    bws, out = outs(OE.WO._size(L.cid_esr_backward_workspace_bytes, n, h, w, R), "ws"), outs(4 * n * 3 * h * w, "f32")
    bn, state = OE._bn_array(layers, ops, outs, True, state=sd)       # every run starts from the loaded running statistics
    m._check(L.cid_esr_forward_saved(m._cid, x.data_ptr(), fmt, out.ptr, n, h, w, bn, saved.ptr, saved.nbytes, fws.ptr, fws.nbytes, OE._stream()))
    g, grads = _GradsArg(), {}
    for k, p in m.named_parameters():
        grads[k] = outs(4 * p.numel(), "f32")
        _set_grad(g, k, grads[k].ptr)
    assert L.cid_debug_poison_lds(OE._stream()) == 0
    m._check(L.cid_esr_backward(m._cid, x.data_ptr(), fmt, ops["grad_out"].data_ptr(), n, h, w, bn, saved.ptr, saved.nbytes, ctypes.byref(g),
                                bws.ptr, bws.nbytes, OE._stream()))
    torch.cuda.synchronize()
    res = {"out": out.tensor(torch.float32, (n, 3, h, w))}
    res.update(OE._bn_results("", layers, state))
    res.update({k: grads[k].tensor(torch.float32, tuple(p.shape)) for k, p in m.named_parameters()})
    return res


def _anchor(ctx, ops, res):
    """The plain run has the bits of test_esrgan_backward.cabi on a freshly loaded module, running statistics included; that run is
    held to float64 by that file's check_against_float64 (the uint8 batch is read as its /255 fp32 copy, whose variant is held)."""
    shape = ctx["shape"]
    _, sd = _model()
    m = TEB.model_of(sd, R)
    out, grads, masks = TEB.cabi(m, ops["in"], ops["grad_out"])
    assert torch.equal(out, res["out"]) and all(torch.equal(grads[k], res[k]) for k in grads) and len(grads) == 5 + 9 * R
    assert all(torch.equal(OE._bits(v), OE._bits(res[k].reshape(v.shape))) for k, v in TEB.running(m).items())
    if ctx["fmt"] == "u8":
        return 0.0
    e_aten, _ = REF.aten_errors("hot", (R, shape))
    TEB.check_against_float64(sd, ETO.case_input(shape), ops["grad_out"], R, grads, masks, e_aten)
    g64, _, _, book = REF.ref_backward(sd, ETO.case_input(shape), ops["grad_out"].cpu(), R, torch.float64, masks=masks)
    errs = REF.rel_errors({k: v.cpu() for k, v in grads.items()}, g64, book)
    return max(e / max(REF.TOL, 2 * e_aten.get(k, 0.0)) for k, e in errs.items())


def _pack_make(variant, shape):
    m = TEB.model_of(synth.make_esrgan_state_dict("hot", variant), variant)
    ops = {k: p.detach().clone() for k, p in m.named_parameters()}
    ops.update({"buffer." + k: b.detach().clone() for k, b in m.named_buffers()})
    return dict(r=variant), ops


def _pack_run(ctx, ops, outs):
    """The module's own device pack (one cid_esr_pack_weights_device call) with every parameter's and buffer's storage replaced by
    the placed operand: the pointers of the call are the operands' own.  The blob is the module's (256-byte aligned by contract)."""
    r = ctx["r"]
    m = TEB.model_of(synth.make_esrgan_state_dict("hot", r), r)
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.data = ops[k]
        for k, b in m.named_buffers():
            b.data = ops["buffer." + k]
    blob = m.pack_weights()
    torch.cuda.synchronize()
    assert all(p.data_ptr() == ops[k].data_ptr() for k, p in m.named_parameters())
    return {"blob": blob.clone()}


def _pack_anchor(ctx, ops, res):
    """The host pack of the same weights, byte for byte."""
    r = ctx["r"]
    want = load_esrgan(synth.make_esrgan_state_dict("hot", r), num_residuals=r, device=OE.DEV, strict=True).pack_weights()
    torch.cuda.synchronize()
    assert want.numel() == res["blob"].numel() and torch.equal(want.view(torch.uint8), res["blob"].view(torch.uint8))
    return 0.0


ROWS = [
    OE.Row("esr_forward_saved+backward", ["cid_esr_forward_saved", "cid_esr_backward"],
           {"in": "f32 | u8", "grad_out": "f32", "BatchNorm gamma, beta": "f32"},
           {"out": "f32", "every parameter gradient": "f32", "BatchNorm running_mean, running_var (in/out)": "f32",
            "BatchNorm num_batches_tracked (in/out)": "i64"}, ((1, 5, 7), (3, 8, 12)),
           couples="train-mode BatchNorm: statistics over the batch", variants=("f32", "u8"), make=_make, run=_run, anchor=_anchor,
           note="the entry points have no eval mode and no input gradient"),
    OE.Row("esr_pack_weights_device", ["cid_esr_pack_weights_device"],
           {"every parameter tensor": "f32", "BatchNorm buffers": "f32", "BatchNorm counters": "i64"}, {"device_blob": "blob"}, ((1, 1), (1, 1)),
           couples="no images", variants=(0, 3), make=_pack_make, run=_pack_run, anchor=_pack_anchor,
           note="the variant is the number of residual blocks; the pack does not depend on a shape"),
]
CASES = [(r.name, v, s) for r in ROWS for v in r.variants for s in dict.fromkeys(r.shapes)]
_BY_NAME = {r.name: r for r in ROWS}
_PLAIN = {}


def _id(case):
    return f"{case[0]}-{case[1]}-{'x'.join(map(str, case[2]))}"


def plain(case):
    """(row, ctx, operands, results) of the plain run of a case, anchored: made once, only read."""
    if case not in _PLAIN:
        row = _BY_NAME[case[0]]
        ctx, ops = row.make(case[1], case[2])
        res = OE.execute(row, ctx, ops, OE.Place())
        for k, t in res.items():
            assert not t.dtype.is_floating_point or bool(torch.isfinite(t).all()), (case, k)
        share = row.anchor(ctx, ops, res)
        print(f"\nanchor {_id(case)}: worst share of the reference's bound {share:.3f}")
        assert share <= 1.0
        _PLAIN[case] = (row, ctx, ops, res)
    return _PLAIN[case]


def test_the_entry_points_have_their_decision_and_the_rows_name_their_four_things():
    """What test_operand_edges_host.py asks of a row of the table, asked of these; no GPU."""
    covered = [fn for r in ROWS for fn in r.entry]
    assert sorted(covered) == ["cid_esr_backward", "cid_esr_forward_saved", "cid_esr_pack_weights_device"]
    assert all(fn in OE.EXEMPT and not any(fn in r.entry for r in OE.TABLE) for fn in covered + ["cid_esr_saved_masks"])
    kinds = ("f32", "u8", "f64", "i64", "f32|u8", "u8|f32", "blob")
    for r in ROWS:
        assert r.operands and r.outputs and len(r.shapes) == 2
        assert all(t.replace(" ", "") in kinds for t in list(r.operands.values()) + list(r.outputs.values()))
        assert isinstance(r.couples, str) and not r.images and not r.grads and not r.local      # Parts A and C only
        assert r.make is not None and r.run is not None and r.anchor is not None
    assert ROWS[0].shapes[0] == ETO.PARITY_CASES[0] and ROWS[0].shapes[1] in ETO.PARITY_CASES and ROWS[0].shapes[1][0] == 3


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_part_a_operands_between_nan_guards(case):
    row, ctx, ops, want = plain(case)
    nan = OE.execute(row, ctx, ops, OE.Place(OE.NAN_BYTE))
    zero = OE.execute(row, ctx, ops, OE.Place(OE.ZERO_BYTE))
    OE.same_bits(nan, zero, (case, "0xFF against 0x00 guards"))
    OE.same_bits(nan, want, (case, "guarded against plain"))


@pytest.mark.gpu
@pytest.mark.parametrize("outputs_too", (True, False), ids=("all_pointers", "operands_only"))
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_part_c_every_admitted_alignment(case, outputs_too):
    row, ctx, ops, want = plain(case)
    for j in (0, 1):
        got = OE.execute(row, ctx, ops, OE.Place(OE.NAN_BYTE, j, outputs_too))
        OE.same_bits(got, want, (case, "offsets", j, outputs_too))
