#!/usr/bin/env python3
"""Generate the LPIPS fixtures in tests/golden/.

There is no reference class to lift (the reference only imports the `lpips` package, which is not vendored): the network is
built here as plain torch.nn from the definition in include/cid.h and run in ATen fp32 on the portable synthetic weights of
celebrity_image_denoiser_amd.synth.make_lpips_state_dict.  It records

  lpips_<wset>_<kind>_<H>x<W>_n<N>.npz   for FIXTURES: d [N], layers [N,5] and relu5 [2 N,256,H3,W3] of ATen fp32 (float32), plus the
                                         unit_view flag; the operands come from lpips_oracle.pairs and are not stored
  lpips_synth_digests.json               sha256 of the synthetic weight sets
  lpips_stats.json                       per case of lpips_oracle.CASES, weight set, operand kind and flag: ATen fp32's error against
                                         the float64 oracle, per tap relative to max(1, max|tap64|) and per distance relative to it

and asserts what the tests rely on: ATen fp32 alone stays 5x inside the tap rule (1e-5 * max(1, max|ref|)) and inside the distance
bound (|delta| <= 1e-5 |ref| for d_0 ... d_4 and d) on every case.   Usage:  python tests/golden/make_lpips_golden.py
"""
import hashlib
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
import lpips_oracle  # noqa: E402

FIXTURES = ((31, 31, 2), (35, 47, 3), (64, 64, 2))
SIZE_CAP = 700 * 1000


class Net(nn.Module):
    """LPIPS(net='alex') in stock layers, fp32."""

    def __init__(self, sd):
        super().__init__()
        t = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
        self.shift, self.scale = t["scaling_layer.shift"], t["scaling_layer.scale"]
        self.convs = nn.ModuleList()
        self.pools = []
        for prefix, stride, pad, pool in lpips_oracle.CONVS:
            w = t[prefix + ".weight"]
            c = nn.Conv2d(w.shape[1], w.shape[0], w.shape[2], stride=stride, padding=pad)
            c.load_state_dict({"weight": w, "bias": t[prefix + ".bias"]})
            self.convs.append(c)
            self.pools.append(pool)
        self.lins = [t[f"lin{k}.model.1.weight"] for k in range(5)]

    def tower(self, x):
        x = (x - self.shift) / self.scale
        out = []
        for c, pool in zip(self.convs, self.pools):
            if pool:
                x = nn.functional.max_pool2d(x, 3, 2)
            x = torch.relu(c(x))
            out.append(x)
        return out

    def forward(self, a, b):
        t0, t1 = self.tower(a), self.tower(b)
        layers = []
        for x0, x1, w in zip(t0, t1, self.lins):
            n0 = x0 / (torch.sqrt(torch.sum(x0 ** 2, dim=1, keepdim=True)) + 1e-10)
            n1 = x1 / (torch.sqrt(torch.sum(x1 ** 2, dim=1, keepdim=True)) + 1e-10)
            layers.append(nn.functional.conv2d((n0 - n1) ** 2, w).mean(dim=(2, 3)).view(-1))
        layers = torch.stack(layers, dim=1)
        return [torch.cat([x0, x1]) for x0, x1 in zip(t0, t1)], layers, layers.sum(dim=1)


def digest(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def first_index(h, w, n):
    return 5000 + 100 * h + w + n


def main():
    torch.set_num_threads(8)
    with open(os.path.join(HERE, "lpips_synth_digests.json"), "w") as f:
        json.dump({k: digest(synth.make_lpips_state_dict(k)) for k in ("default", "hot")}, f, indent=1)
    stats = {"torch": torch.__version__, "network": "plain torch.nn restatement of include/cid.h's definition, ATen fp32 on the CPU"}
    worst_tap, worst_d = 0.0, 0.0
    for wset in ("default", "hot"):
        sd = synth.make_lpips_state_dict(wset)
        net = Net(sd).eval()
        for h, w, n in lpips_oracle.CASES:
            for kind in ("noisy", "unrelated"):
                a, b, _, _ = lpips_oracle.pairs(kind, n, h, w, first_index(h, w, n))
                for unit in (False, True):
                    ref = lpips_oracle.forward(sd, a, b, unit)
                    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
                    with torch.no_grad():
                        taps, layers, d = net(ta * 0.5 + 0.5, tb * 0.5 + 0.5) if unit else net(ta, tb)
                    e = {name: float(np.abs(t.numpy() - ref[name]).max()) / max(1.0, float(np.abs(ref[name]).max()))
                         for name, t in zip(lpips_oracle.TAPS, taps)}
                    e["layers_rel"] = float((np.abs(layers.numpy() - ref["layers"]) / np.abs(ref["layers"])).max())
                    e["d_rel"] = float((np.abs(d.numpy().astype(np.float64) - ref["d"]) / np.abs(ref["d"])).max())
                    e["d_min"], e["d_max"] = float(ref["d"].min()), float(ref["d"].max())
                    e["zero_share_relu5"] = float((ref["relu5"] == 0).mean())
                    name = f"{wset}_{kind}_{h}x{w}_n{n}_unit{int(unit)}"
                    stats[name] = e
                    tap_err = max(e[t] for t in lpips_oracle.TAPS)
                    worst_tap, worst_d = max(worst_tap, tap_err), max(worst_d, e["layers_rel"], e["d_rel"])
                    print(name, f"tap {tap_err:.2e} layers {e['layers_rel']:.2e} d {e['d_rel']:.2e} d in [{e['d_min']:.3g}, {e['d_max']:.3g}]")
                    assert tap_err <= 2e-6, (name, e)                       # 5x inside the tap rule
                    assert e["layers_rel"] <= 1e-5 and e["d_rel"] <= 1e-5, (name, e)   # inside the distance bound
                    if (h, w, n) in FIXTURES and unit == (kind == "noisy"):
                        np.savez_compressed(os.path.join(HERE, f"lpips_{wset}_{kind}_{h}x{w}_n{n}.npz"), d=d.numpy(), layers=layers.numpy(),
                                            relu5=taps[4].numpy(), unit_view=np.array(unit), first_index=np.array(first_index(h, w, n)))
    stats["worst_fp32_tap_error"], stats["worst_fp32_distance_error"] = worst_tap, worst_d
    print("worst ATen fp32 tap error", worst_tap, "distance error", worst_d)
    for p in os.listdir(HERE):
        if p.startswith("lpips_"):
            assert os.path.getsize(os.path.join(HERE, p)) < SIZE_CAP, p
    with open(os.path.join(HERE, "lpips_stats.json"), "w") as f:
        json.dump(stats, f, indent=1)
    print("wrote LPIPS fixtures to", HERE)


if __name__ == "__main__":
    main()
