"""cid_esr_forward_train held to the operand contract of tests/test_operand_edges.py: the row that file's TABLE would carry, with its
Parts A and C, kept in a file of its own.

The entry point's caller-supplied operands are the image batch and, per BatchNorm, gamma and beta (read only) and running_mean,
running_var and num_batches_tracked (in/out).  Part A: every read-only operand directly between guard regions of 0xFF bytes and of
0x00 bytes, every output, workspace and in/out buffer 0xFF-prefilled between 0xA5 guards; all results bit-equal to the plain run, no
operand or guard byte written.  Part C: the same at every alignment the contract admits (fp32 4 and 12, uint8 1 and 3 bytes past a
256-byte boundary).  Part B (an image poisoned with NaN or Inf stays in its image) does not apply: train-mode BatchNorm takes its
statistics over the batch.  The plain run is anchored to tests/esrgan_train_oracle.py in float64 under the project's rule.

tests/test_operand_edges_host.py asks that every launching function of include/cid.h be a row of test_operand_edges.TABLE or stand in
its EXEMPT dict with a reason.  This module enters the function there when it is imported, which pytest does for every test module
before the first test runs: its reason is that its row is here."""
import os
import sys

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import esrgan_train_oracle as ETO  # noqa: E402
import test_operand_edges as OE  # noqa: E402

OE.EXEMPT.setdefault("cid_esr_forward_train", "its row, with Parts A and C, is tests/test_operand_edges_esrgan_train.py")

R = 3                          # both tensors the block outputs alternate between are in use
STAGES = ("x1", "tail_in")
_MODEL = []


def _model():
    if not _MODEL:
        from celebrity_image_denoiser_amd.esrgan import load_esrgan

        sd = synth.make_esrgan_state_dict("hot", R)
        m = load_esrgan(sd, num_residuals=R, device=OE.DEV, strict=True, batch_stats=True).train()
        m.pack_weights()
        _MODEL.append((m, sd))
    return _MODEL[0]


def _layers(m):
    return [(name, layer) for name, layer, _ in m._batchnorms()]


def _make(variant, shape):
    u8 = synth.esrgan_inputs_u8(*shape, ETO._FIRST[shape])
    x = ETO.case_input(shape)
    ops = {"in": OE._dev(u8 if variant == "u8" else x)}
    ops.update(OE._bn_ops(_layers(_model()[0]), True))
    return dict(shape=shape), ops


def _run(ctx, ops, outs):
    L = _lib.lib()
    n, h, w = ctx["shape"]
    m, sd = _model()
    x, layers = ops["in"], _layers(m)
    ws, out = outs(OE.WO._size(L.cid_esr_train_workspace_bytes, n, h, w, R), "ws"), outs(4 * n * 3 * h * w, "f32")
    bn, state = OE._bn_array(layers, ops, outs, True, state=sd)       # every run starts from the loaded running statistics
    m._check(L.cid_esr_forward_train(m._cid, x.data_ptr(), OE.U8 if x.dtype == torch.uint8 else OE.F32, out.ptr, OE.F32, n, h, w, bn,
                                     ws.ptr, ws.nbytes, OE._stream()))
    torch.cuda.synchronize()
    res = {"out": out.tensor(torch.float32, (n, 3, h, w))}
    res.update(OE._bn_results("", layers, state))
    OE._stage_results(res, ws.bits(), OE._views(L.cid_esr_train_stage_view, STAGES, n, h, w, R), n)
    return res


def _anchor(ctx, ops, res):
    """Stages, output and running statistics under the oracle's bound; the counters exact."""
    shape = ctx["shape"]
    n, h, w = shape
    ref = ETO.reference("hot", shape, R)
    share = OE._stage_shares(res, OE._views(_lib.lib().cid_esr_train_stage_view, STAGES, n, h, w, R), ref, ETO.bound)
    share = max(share, OE.WO._share("out", res["out"].cpu().numpy(), ref["out"], ETO.bound(ref["out"])))
    for name in ETO.BN_NAMES(R):
        for k in ("running_mean", "running_var"):
            share = max(share, OE.WO._share(f"{name}.{k}", res[f"{name}.{k}"].cpu().numpy(), ref[f"{name}.{k}"], ETO.bound(ref[f"{name}.{k}"])))
        assert int(res[name + ".num_batches_tracked"]) == int(ref[name + ".num_batches_tracked"]), name
    return share


ROW = OE.Row("esr_forward_train", ["cid_esr_forward_train"], {"in": "f32 | u8", "BatchNorm gamma, beta": "f32"},
             {"out": "f32", "BatchNorm running_mean, running_var (in/out)": "f32", "BatchNorm num_batches_tracked (in/out)": "i64"},
             ((1, 5, 7), (3, 8, 12)), couples="train-mode BatchNorm: statistics over the batch", variants=("f32", "u8"),
             make=_make, run=_run, anchor=_anchor,
             note="(1, 5, 7) is the smallest shape of the family's parity list; (2, 1, 1) is accepted but has two values per channel, "
                  "which no oracle bound holds for")
CASES = [(v, s) for v in ROW.variants for s in ROW.shapes]
_PLAIN = {}


def _id(case):
    return f"{case[0]}-{'x'.join(map(str, case[1]))}"


def plain(case):
    """(ctx, operands, results) of the plain run of a case, anchored to the float64 oracle: made once, only read."""
    if case not in _PLAIN:
        ctx, ops = ROW.make(*case)
        res = OE.execute(ROW, ctx, ops, OE.Place())
        for k, t in res.items():
            assert not t.dtype.is_floating_point or bool(torch.isfinite(t).all()), (case, k)
        share = ROW.anchor(ctx, ops, res)
        print(f"\nanchor {_id(case)}: worst share of the oracle bound {share:.3f}")
        assert share <= 1.0
        _PLAIN[case] = (ctx, ops, res)
    return _PLAIN[case]


def test_the_entry_point_has_its_decision_and_the_row_names_its_four_things():
    """What test_operand_edges_host.py asks of a row of the table, asked of this one; no GPU."""
    assert "cid_esr_forward_train" in OE.EXEMPT and not any("cid_esr_forward_train" in r.entry for r in OE.TABLE)
    assert ROW.operands and ROW.outputs and len(ROW.shapes) == 2
    kinds = ("f32", "u8", "f64", "i64", "f32|u8", "u8|f32", "blob")
    assert all(t.replace(" ", "") in kinds for t in list(ROW.operands.values()) + list(ROW.outputs.values()))
    assert isinstance(ROW.couples, str) and not ROW.images and not ROW.grads and not ROW.local      # Parts A and C only
    assert ROW.make is not None and ROW.run is not None and ROW.anchor is not None
    assert ROW.shapes[0] == ETO.PARITY_CASES[0] and ROW.shapes[1] in ETO.PARITY_CASES and ROW.shapes[1][0] == 3


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_part_a_operands_between_nan_guards(case):
    ctx, ops, want = plain(case)
    nan = OE.execute(ROW, ctx, ops, OE.Place(OE.NAN_BYTE))
    zero = OE.execute(ROW, ctx, ops, OE.Place(OE.ZERO_BYTE))
    OE.same_bits(nan, zero, (case, "0xFF against 0x00 guards"))
    OE.same_bits(nan, want, (case, "guarded against plain"))


@pytest.mark.gpu
@pytest.mark.parametrize("outputs_too", (True, False), ids=("all_pointers", "operands_only"))
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_part_c_every_admitted_alignment(case, outputs_too):
    ctx, ops, want = plain(case)
    for j in (0, 1):
        got = OE.execute(ROW, ctx, ops, OE.Place(OE.NAN_BYTE, j, outputs_too))
        OE.same_bits(got, want, (case, "offsets", j, outputs_too))
