#!/usr/bin/env python3
"""Generate the SRGAN fixtures in tests/golden/ from the REFERENCE implementation itself.

Runs only where the reference tree is present.  Nothing of the reference is copied into this repo: the script parses
backend/app.py at run time, pulls out the ClassDef `SRGANGenerator` (app.py:145-186), instantiates it, loads the portable synthetic
weights of celebrity_image_denoiser_amd.synth.make_srgan_state_dict and records

  srgan_keys.json                        the state_dict keys, shapes and dtypes of the reference class for scale 4 and 2
  srgan_<wset>_s4_5x7.npz (N=1)          x and the forward hooks on initial, res_blocks, mid, upscale, final (= the sum before tanh),
                                         and out, float32
  srgan_<wset>_s4_16x16.npz (N=2), srgan_<wset>_s4_13x18.npz (N=1):
                                         x, x0 = initial(x), trunk = mid(res_blocks(x0)) + x0 and out only (a 64-channel tensor at
                                         4x size does not fit the size cap)
  srgan_<wset>_u8_24x20.npz (N=2)        a uint8 input, the padding and the server's uint8 output: get_padding(image, 4, 4) ->
                                         Pad(fill=0) -> ToTensor -> Normalize(0.5, 0.5) -> net -> y*0.5+0.5 -> clamp(0,1) ->
                                         ToPILImage = mul(255).byte() (app.py:276-281, 400-406, 434-435, 472; torchvision and PIL are
                                         not needed: these third-party steps are written out with numpy / torch ops)
  srgan_stats.json                       per fixture: the reference's own fp32 error against the same module in float64 per stage,
                                         relative to max(1, max|stage64|); the saturated share of the uint8 bytes; the share of
                                         bytes in which ATen fp32 and to_u8(oracle64) differ; ATen's fp32 tanh error over [-20, 20];
                                         and the fp32 margins at the oracle-only shapes of tests/test_srgan.py

with <wset> in {default, hot}.   Usage:  python tests/golden/make_srgan_golden.py
"""
import ast
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from celebrity_image_denoiser_amd import synth  # noqa: E402
import srgan_oracle  # noqa: E402

REF_APP = "/root/reference/backend/app.py"
STAGES = ("initial", "res_blocks", "mid", "upscale", "final")


def lift_reference_class(path=REF_APP):
    with open(path, "r") as f:
        tree = ast.parse(f.read(), path)
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "SRGANGenerator"]
    assert len(cls) == 1
    ns = {"torch": torch, "nn": nn, "np": np}
    exec(compile(ast.Module(body=cls, type_ignores=[]), path, "exec"), ns)
    return ns["SRGANGenerator"]


def build(cls, wset, scale, dtype=torch.float32):
    model = cls(scale_factor=scale)
    sd = synth.make_srgan_state_dict(wset, scale)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return model.to(dtype).eval()


def run(model, x):
    rec = {}
    hooks = [getattr(model, s).register_forward_hook(lambda m, i, o, s=s: rec.__setitem__(s, o.detach().clone())) for s in STAGES]
    with torch.no_grad():
        out = model(x)
    for h in hooks:
        h.remove()
    r = {s: rec[s].numpy() for s in STAGES}
    r["out"] = out.numpy()
    r["x0"], r["trunk"], r["pre"] = r["initial"], r["mid"] + r["initial"], r["final"]   # forward(): x = self.mid(res) + x0
    return r


def inputs(n, h, w, first):
    u8 = synth.srgan_inputs_u8(n, h, w, first)
    return u8, torch.from_numpy(srgan_oracle.normalise_u8(u8))


def rel_errors(rec, r64, keys):
    return {k: float(np.abs(rec[k] - r64[k]).max()) / max(1.0, float(np.abs(r64[k]).max())) for k in keys}


def margins(rec, r64):
    """The quantities tests/test_srgan.py bounds: every stage relative to its own scale, and `out` relative to max(1, max|pre64|)."""
    e = rel_errors(rec, r64, ("x0", "res_blocks", "trunk", "upscale", "pre"))
    e["out_abs"] = float(np.abs(rec["out"] - r64["out"]).max())
    e["out_rel_pre"] = e["out_abs"] / max(1.0, float(np.abs(r64["pre"]).max()))
    worst = max(v for k, v in e.items() if k != "out_abs")
    return {"fp32_vs_fp64_rel": e, "max_abs_pre": float(np.abs(r64["pre"]).max()), "beyond_0.999": float((np.abs(r64["out"]) > 0.999).mean()),
            "margin_under_1e-5": 1e-5 / worst if worst > 0 else None}


def main():
    torch.set_num_threads(8)
    cls = lift_reference_class()
    keys = {f"s{s}": [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in cls(scale_factor=s).state_dict().items()] for s in (4, 2)}
    with open(os.path.join(HERE, "srgan_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    stats = {"torch": torch.__version__, "reference": "backend/app.py:145-186 SRGANGenerator (lifted by AST)", "hot_gain": 6.0}
    g = torch.linspace(-20, 20, 4_000_001, dtype=torch.float64)
    stats["aten_tanh_fp32_max_err_-20_20"] = float((torch.tanh(g.float()).double() - torch.tanh(g.float().double())).abs().max())
    print("ATen fp32 tanh:", stats["aten_tanh_fp32_max_err_-20_20"])
    cases = [(ws, 1, 5, 7, 2000, True) for ws in ("default", "hot")] + [(ws, 2, 16, 16, 2010, False) for ws in ("default", "hot")]
    cases += [(ws, 1, 13, 18, 2020, False) for ws in ("default", "hot")]
    for wset, n, h, w, first, full in cases:
        _, x = inputs(n, h, w, first)
        rec = run(build(cls, wset, 4), x)
        r64 = run(build(cls, wset, 4, torch.float64), x.double())
        name = f"srgan_{wset}_s4_{h}x{w}"
        keep = STAGES + ("out",) if full else ("x0", "trunk", "out")
        np.savez_compressed(os.path.join(HERE, name + ".npz"), x=x.numpy(), **{k: rec[k] for k in keep})
        stats[name] = margins(rec, r64)
        print(name, os.path.getsize(os.path.join(HERE, name + ".npz")), stats[name])
    for wset in ("default", "hot"):
        u8, _ = inputs(2, 24, 20, 2040)
        pad = [int(v) for v in _get_padding(24, 20, 4, 4)]
        pl, pt, pr, pb = pad
        padded = np.pad(u8, ((0, 0), (pt, pb), (pl, pr), (0, 0)))                          # Pad(fill=0)
        x = torch.from_numpy(srgan_oracle.normalise_u8(padded))                            # ToTensor, Normalize(0.5, 0.5)
        with torch.no_grad():
            y = build(cls, wset, 4)(x)
            y64 = build(cls, wset, 4, torch.float64)(x.double())
        out_u8 = (y * 0.5 + 0.5).clamp(0, 1).mul(255).byte().permute(0, 2, 3, 1).contiguous().numpy()
        name = f"srgan_{wset}_u8_24x20"
        np.savez_compressed(os.path.join(HERE, name + ".npz"), in_u8=u8, out_u8=out_u8, padding=np.array(pad, dtype=np.int32))
        o64 = srgan_oracle.to_u8(y64.numpy())
        d = np.abs(o64.astype(np.int16) - out_u8.astype(np.int16))
        stats[name] = {"saturated_bytes": float(((out_u8 == 0) | (out_u8 == 255)).mean()), "bytes_at_0": float((out_u8 == 0).mean()),
                       "bytes_at_255": float((out_u8 == 255).mean()), "aten_vs_oracle64_max": int(d.max()),
                       "aten_vs_oracle64_differing": float((d != 0).mean())}
        print(name, os.path.getsize(os.path.join(HERE, name + ".npz")), stats[name])
    # the same margins at the shapes the GPU tests use beyond the fixtures (oracle-only cases there)
    for wset in ("default", "hot"):
        for scale, n, h, w, first in ((4, 1, 1, 1, 2100), (4, 3, 8, 12, 2140), (4, 1, 20, 36, 2150), (2, 1, 13, 18, 2160), (1, 1, 5, 7, 2170)):
            _, x = inputs(n, h, w, first)
            rec = run(build(cls, wset, scale), x)
            r64 = run(build(cls, wset, scale, torch.float64), x.double())
            if scale == 1:   # an empty nn.Sequential: the hook gives its input back
                rec["upscale"], r64["upscale"] = rec["trunk"], r64["trunk"]
            stats[f"margin_{wset}_s{scale}_{n}x{h}x{w}"] = margins(rec, r64)
            print(wset, scale, n, h, w, stats[f"margin_{wset}_s{scale}_{n}x{h}x{w}"])
    with open(os.path.join(HERE, "srgan_stats.json"), "w") as f:
        json.dump(stats, f, indent=1)
    print("wrote SRGAN fixtures to", HERE)


def _get_padding(h, w, divisor, scale, path=REF_APP):
    """The reference's own get_padding (app.py:276-281), lifted by AST and called with a stand-in for the PIL image (only .size is
    read): (left, top, right, bottom)."""
    import types
    import typing

    with open(path, "r") as f:
        tree = ast.parse(f.read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_padding"]
    assert len(fn) == 1
    ns = {"Image": types.SimpleNamespace(Image=object), "Tuple": typing.Tuple}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["get_padding"](types.SimpleNamespace(size=(w, h)), divisor, scale)


if __name__ == "__main__":
    main()
