#!/usr/bin/env python3
"""Generate the ESRGAN fixtures in tests/golden/ from the REFERENCE implementation itself.

Runs only where the reference tree is present.  Nothing of the reference is copied into this repo: the script parses
backend/app.py at run time, pulls out the two ClassDefs `ResidualBlock` and `ESRGANGenerator` (app.py:188-218), instantiates them,
loads the portable synthetic weights of celebrity_image_denoiser_amd.synth.make_esrgan_state_dict and records

  esrgan_keys.json                       the state_dict keys, shapes and dtypes of the reference class for R = 8 and R = 1
  esrgan_<wset>_r8_16x16.npz (N=2), esrgan_<wset>_r8_13x18.npz (N=1), esrgan_<wset>_r1_5x7.npz (N=1), esrgan_default_r0_1x1.npz:
                                         x, x1 = initial(x), x2 = residuals(x1) (forward hooks) and out, float32
  esrgan_default_u8_24x20.npz (N=2)      a uint8 input and the server's uint8 output: /255 (ToTensor) -> net -> clamp(0,1) ->
                                         ToPILImage = mul(255).byte() (app.py:243-254; torchvision is absent here, so these
                                         third-party steps are written out with torch ops)
  esrgan_stats.json                      the reference's own fp32 error against the same module in float64, per fixture, relative to
                                         max(1, max|out64|): what the 1e-5 parity bound of tests/test_esrgan.py is held against

with <wset> in {default, hot}.   Usage:  python tests/golden/make_esrgan_golden.py
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
from celebrity_image_denoiser_amd import synth  # noqa: E402

REF_APP = "/root/reference/backend/app.py"


def lift_reference_classes(path=REF_APP):
    with open(path, "r") as f:
        tree = ast.parse(f.read(), path)
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ("ResidualBlock", "ESRGANGenerator")]
    assert [c.name for c in cls] == ["ResidualBlock", "ESRGANGenerator"]
    ns = {"torch": torch, "nn": nn}
    exec(compile(ast.Module(body=cls, type_ignores=[]), path, "exec"), ns)
    return ns["ESRGANGenerator"]


def build(cls, wset, r, dtype=torch.float32):
    model = cls(num_residuals=r)
    sd = synth.make_esrgan_state_dict(wset, r)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return model.to(dtype).eval()


def run(model, x):
    rec = {}
    hooks = [getattr(model, s).register_forward_hook(lambda m, i, o, s=s: rec.__setitem__(s, o.detach().clone()))
             for s in ("initial", "residuals")]
    with torch.no_grad():
        out = model(x)
    for h in hooks:
        h.remove()
    return {"x1": rec["initial"].numpy(), "x2": rec["residuals"].numpy(), "out": out.numpy()}


def inputs(n, h, w, first):
    u8 = synth.esrgan_inputs_u8(n, h, w, first)
    return u8, torch.from_numpy(u8).permute(0, 3, 1, 2).to(torch.float32).div(255).contiguous()


def main():
    torch.set_num_threads(8)
    cls = lift_reference_classes()
    keys = {}
    for r in (8, 1):
        keys[f"r{r}"] = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in cls(num_residuals=r).state_dict().items()]
    with open(os.path.join(HERE, "esrgan_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    stats = {"torch": torch.__version__, "reference": "backend/app.py:188-218 ResidualBlock, ESRGANGenerator (lifted by AST)"}
    cases = [(ws, 8, 2, 16, 16, 1000) for ws in ("default", "hot")] + [(ws, 8, 1, 13, 18, 1010) for ws in ("default", "hot")]
    cases += [(ws, 1, 1, 5, 7, 1020) for ws in ("default", "hot")] + [("default", 0, 1, 1, 1, 1030)]
    for wset, r, n, h, w, first in cases:
        _, x = inputs(n, h, w, first)
        rec = run(build(cls, wset, r), x)
        r64 = run(build(cls, wset, r, torch.float64), x.double())
        name = f"esrgan_{wset}_r{r}_{h}x{w}"
        np.savez_compressed(os.path.join(HERE, name + ".npz"), x=x.numpy(), **rec)
        scale = max(1.0, float(np.abs(r64["out"]).max()))
        o = rec["out"]
        stats[name] = {"max_abs_out": float(np.abs(r64["out"]).max()), "outside_unit_range": float(((o < 0) | (o > 1)).mean()),
                       "fp32_vs_fp64_rel": {k: float(np.abs(rec[k] - r64[k]).max()) / max(1.0, float(np.abs(r64[k]).max())) for k in rec},
                       "margin_under_1e-5": 1e-5 / (float(np.abs(rec["out"] - r64["out"]).max()) / scale) if np.any(rec["out"] != r64["out"]) else None}
        print(name, stats[name])
    u8, x = inputs(2, 24, 20, 1040)
    model = build(cls, "default", 8)
    with torch.no_grad():
        y = model(x)
    out_u8 = y.clamp(0, 1).mul(255).byte().permute(0, 2, 3, 1).contiguous().numpy()
    np.savez_compressed(os.path.join(HERE, "esrgan_default_u8_24x20.npz"), in_u8=u8, out_u8=out_u8, out_f32=y.numpy())
    stats["esrgan_default_u8_24x20"] = {"saturated_bytes": float(((out_u8 == 0) | (out_u8 == 255)).mean())}
    print("u8 24x20 saturated:", stats["esrgan_default_u8_24x20"])
    # the same margin at the sizes the GPU tests use beyond the fixtures (oracle-only cases there)
    for wset in ("default", "hot"):
        for n, h, w, first in ((1, 37, 53, 1050), (2, 64, 64, 1070)):
            _, x = inputs(n, h, w, first)
            rec = run(build(cls, wset, 8), x)
            r64 = run(build(cls, wset, 8, torch.float64), x.double())
            scale = max(1.0, float(np.abs(r64["out"]).max()))
            err = float(np.abs(rec["out"] - r64["out"]).max()) / scale
            stats[f"margin_{wset}_r8_{n}x{h}x{w}"] = {"max_abs_out": scale, "fp32_vs_fp64_rel": err, "margin_under_1e-5": 1e-5 / err}
            print(wset, n, h, w, stats[f"margin_{wset}_r8_{n}x{h}x{w}"])
    with open(os.path.join(HERE, "esrgan_stats.json"), "w") as f:
        json.dump(stats, f, indent=1)
    print("wrote ESRGAN fixtures to", HERE)


if __name__ == "__main__":
    main()
