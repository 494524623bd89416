"""The CPU pin of tests/test_operand_edges.py: every function of include/cid.h that takes a `void* stream` launches (or may launch)
work on the caller's operands, so each is a row of that file's TABLE or stands in its EXEMPT dict with a one-line reason.  A later
entry point cannot be added without a decision there."""
import os
import re

import test_operand_edges as OE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launching_entry_points():
    """The names of the header's functions with a `void* stream` parameter, comments stripped."""
    with open(os.path.join(ROOT, "include", "cid.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    found = []
    for name, params in re.findall(r"\b(cid_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        if re.search(r"\bvoid\s*\*\s*stream\b", params):
            found.append(name)
    return found


def test_the_parser_sees_the_header():
    names = launching_entry_points()
    assert len(names) == len(set(names)) and len(names) >= 50
    for known in ("cid_forward_ex", "cid_backward", "cid_adam_step", "cid_vgg_content_backward", "cid_esd_pack_weights_device", "cid_cg_latent"):
        assert known in names
    for host_only in ("cid_create", "cid_workspace_bytes", "cid_resize_plan_create", "cid_debug_adam_step_host", "cid_stage_view"):
        assert host_only not in names


def test_every_launching_entry_point_is_a_row_or_exempt():
    rows = {}
    for r in OE.TABLE:
        for e in r.entry:
            rows.setdefault(e, []).append(r.name)
    names = launching_entry_points()
    undecided = [n for n in names if n not in rows and n not in OE.EXEMPT]
    assert not undecided, f"no row of test_operand_edges.TABLE and no EXEMPT reason for: {undecided}"
    both = [n for n in names if n in rows and n in OE.EXEMPT]
    assert not both, both
    stale = [n for n in list(rows) + list(OE.EXEMPT) if n not in names]
    assert not stale, f"not a launching function of include/cid.h: {stale}"
    assert all(isinstance(v, str) and v and "\n" not in v for v in OE.EXEMPT.values())


def test_every_row_names_its_four_things():
    for r in OE.TABLE:
        assert r.operands and r.outputs and len(r.shapes) == 2, r.name
        assert all(t.replace(" ", "") in ("f32", "u8", "f64", "i64", "f32|u8", "u8|f32", "blob") for t in list(r.operands.values()) + list(r.outputs.values())), r.name
        assert r.couples is None or isinstance(r.couples, str)
        if r.couples is not None:            # a row that couples the batch runs Parts A and C only
            assert not r.images and not r.grads and not r.local, r.name
        assert r.make is not None and r.run is not None and r.anchor is not None, r.name
        if r.images:
            assert r.local and all(k in r.operands for k in r.images + r.grads), r.name
            assert r.shapes[1][0] == 3, (r.name, "Part B runs in a batch of three")


# The issue's list of Part B: eval-mode forwards of the four generators and the three discriminators, cid_forward_padded, the three
# perceptual calls, cid_quality, and the input gradient of every eval-mode backward.  -> the operands poisoned image by image.
PART_B = {
    "forward_ex": ("in",), "forward_padded": ("in",), "view_u8": ("in",), "esr_forward": ("in",), "sr_forward": ("in",), "cg_forward": ("z",),
    "esd_forward": ("in",), "quality": ("b",), "lpips": ("a", "b"), "vgg_lpips": ("a", "b"), "vgg_content_loss": ("a", "b"),
    "forward_saved+backward": ("in", "grad_out"), "disc eval": ("in", "grad_prob"), "srd eval": ("in", "grad_prob"),
    "esd_forward_saved+backward": ("in", "grad_logit"), "vgg_content_loss_saved+backward": ("a", "b", "grad_out"),
}


def test_part_b_runs_the_rows_the_issue_lists():
    """By name: a row that is later marked `couples`, or loses its `images`, drops out of Part B only with a change here."""
    got = {}
    for name, variant, shape in OE.B_CASES:
        row = OE.ROWS[name]
        got[name] = row.images + row.grads
        assert shape == row.shapes[1] and shape[0] == 3, name
    assert got == PART_B
    for name, operands in PART_B.items():                      # each has an fp32 caller among its variants, and results to compare
        row = OE.ROWS[name]
        assert row.couples is None and row.local and (not row.grads or row.grad_local), name
        if "input" in row.local:
            assert "input" in row.grad_local, name
    assert {r.name for r in OE.TABLE if r.couples is not None} == {
        "disc train", "srd train", "sr_forward_train", "sr_forward_saved+backward", "losses", "adam_step", "pack_weights_device"}
    assert {c[0] for c in OE.CASES} == {r.name for r in OE.TABLE}
