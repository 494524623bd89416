#!/usr/bin/env python3
"""Generate the VGG16 fixtures (LPIPS(net='vgg') and the content loss) in tests/golden/.

There is no reference class to lift (the reference imports the `lpips` package and torchvision, neither vendored): the network is
built here as plain torch.nn from the definition in include/cid.h and run in ATen fp32 on the portable synthetic weights of
celebrity_image_denoiser_amd.synth.make_lpips_state_dict(net="vgg").  It records

  lpips_vgg_<wset>_<kind>_<H>x<W>_n<N>.npz   for FIXTURES: d [N], layers [N,5] and relu5 [2 N,512,H5,W5] of ATen fp32 (float32), the
                                             unit_view flag, and loss [N], the content loss of the same operands (unscaled, no
                                             unit view); the operands come from lpips_vgg_oracle.pairs and are not stored
  lpips_vgg_synth_digests.json               sha256 of the synthetic weight sets
  lpips_vgg_stats.json                       per case of lpips_vgg_oracle.CASES / CONTENT_CASES, weight set, operand kind and flag:
                                             ATen fp32's error against the float64 oracle, per tap relative to max(1, max|tap64|)
                                             and per distance / loss relative to the value

and asserts what the tests rely on: ATen fp32 alone stays 5x inside the tap rule (1e-5 * max(1, max|ref|)) and inside the value bound
(|delta| <= 1e-5 |ref| for d_0 ... d_4, d and the content loss) on every case.   Usage:  python tests/golden/make_lpips_vgg_golden.py
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
import lpips_vgg_oracle as oracle  # noqa: E402

FIXTURES = ((16, 16, 2), (35, 47, 3), (64, 64, 2))
SIZE_CAP = 700 * 1000


class Net(nn.Module):
    """vgg16.features with the LPIPS ends and the content-loss end, in stock layers, fp32."""

    def __init__(self, sd):
        super().__init__()
        t = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
        self.shift, self.scale = t["scaling_layer.shift"], t["scaling_layer.scale"]
        self.slices = nn.ModuleList()
        for k, convs in enumerate(oracle.SLICES):
            layers = [nn.MaxPool2d(2, 2)] if k else []
            for idx in convs:
                w = t[f"net.slice{k + 1}.{idx}.weight"]
                c = nn.Conv2d(w.shape[1], w.shape[0], 3, padding=1)
                c.load_state_dict({"weight": w, "bias": t[f"net.slice{k + 1}.{idx}.bias"]})
                layers += [c, nn.ReLU()]
            self.slices.append(nn.Sequential(*layers))
        self.lins = [t[f"lin{k}.model.1.weight"] for k in range(5)]

    def tower(self, x, scaled=True, slices=5):
        if scaled:
            x = (x - self.shift) / self.scale
        out = []
        for s in self.slices[:slices]:
            x = s(x)
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

    def content(self, a, b):
        """The reference class per image pair: MSELoss(reduction='none') of features[:16], averaged over each image."""
        t0, t1 = self.tower(a, False, 3), self.tower(b, False, 3)
        return [torch.cat([x0, x1]) for x0, x1 in zip(t0, t1)], nn.functional.mse_loss(t0[2], t1[2], reduction="none").mean(dim=(1, 2, 3))


def digest(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def tap_errors(taps, ref):
    return {name: float(np.abs(t.numpy() - ref[name]).max()) / max(1.0, float(np.abs(ref[name]).max())) for name, t in zip(oracle.TAPS, taps)}


def main():
    torch.set_num_threads(8)
    with open(os.path.join(HERE, "lpips_vgg_synth_digests.json"), "w") as f:
        json.dump({k: digest(synth.make_lpips_state_dict(k, net="vgg")) for k in ("default", "hot")}, f, indent=1)
    stats = {"torch": torch.__version__, "network": "plain torch.nn restatement of include/cid.h's definition, ATen fp32 on the CPU"}
    worst_tap, worst_d, worst_loss = 0.0, 0.0, 0.0
    for wset in ("default", "hot"):
        sd = oracle.weights(wset)
        net = Net(sd).eval()
        for h, w, n in oracle.CASES:
            for kind in ("noisy", "unrelated"):
                a, b, _, _ = oracle.pairs(kind, n, h, w, oracle.first_index(h, w, n))
                ta, tb = torch.from_numpy(a), torch.from_numpy(b)
                for unit in (False, True):
                    ref = oracle.forward(sd, a, b, unit)
                    with torch.no_grad():
                        taps, layers, d = net(ta * 0.5 + 0.5, tb * 0.5 + 0.5) if unit else net(ta, tb)
                    e = tap_errors(taps, ref)
                    e["layers_rel"] = float((np.abs(layers.numpy() - ref["layers"]) / np.abs(ref["layers"])).max())
                    e["d_rel"] = float((np.abs(d.numpy().astype(np.float64) - ref["d"]) / np.abs(ref["d"])).max())
                    e["d_min"], e["d_max"] = float(ref["d"].min()), float(ref["d"].max())
                    e["zero_share"] = [float((ref[t] == 0).mean()) for t in oracle.TAPS]
                    e["relu5_max"] = float(ref["relu5"].max())
                    name = f"{wset}_{kind}_{h}x{w}_n{n}_unit{int(unit)}"
                    stats[name] = e
                    tap_err = max(e[t] for t in oracle.TAPS)
                    worst_tap, worst_d = max(worst_tap, tap_err), max(worst_d, e["layers_rel"], e["d_rel"])
                    print(name, f"tap {tap_err:.2e} layers {e['layers_rel']:.2e} d {e['d_rel']:.2e} d in [{e['d_min']:.3g}, {e['d_max']:.3g}]",
                          flush=True)
                    assert tap_err <= 2e-6, (name, e)                       # 5x inside the tap rule
                    assert e["layers_rel"] <= 1e-5 and e["d_rel"] <= 1e-5, (name, e)   # inside the distance bound
                    assert e["relu5_max"] > 0 and min(e["zero_share"]) > 0.05 and max(e["zero_share"]) < 0.95, (name, e)   # every tap keeps signal
                    if (h, w, n) in FIXTURES and unit == (kind == "noisy"):
                        with torch.no_grad():
                            _, loss = net.content(ta, tb)
                        np.savez_compressed(os.path.join(HERE, f"lpips_vgg_{wset}_{kind}_{h}x{w}_n{n}.npz"), d=d.numpy(), layers=layers.numpy(),
                                            relu5=taps[4].numpy(), loss=loss.numpy(), unit_view=np.array(unit),
                                            first_index=np.array(oracle.first_index(h, w, n)))
        for h, w, n in oracle.CONTENT_CASES:
            for kind in ("noisy", "unrelated"):
                a, b, _, _ = oracle.pairs(kind, n, h, w, oracle.first_index(h, w, n))
                ref = oracle.content(sd, a, b)
                with torch.no_grad():
                    taps, loss = net.content(torch.from_numpy(a), torch.from_numpy(b))
                e = tap_errors(taps, ref)
                e["loss_rel"] = float((np.abs(loss.numpy().astype(np.float64) - ref["loss"]) / np.abs(ref["loss"])).max())
                e["loss_min"], e["loss_max"] = float(ref["loss"].min()), float(ref["loss"].max())
                name = f"content_{wset}_{kind}_{h}x{w}_n{n}"
                stats[name] = e
                tap_err = max(e[t] for t in oracle.TAPS[:3])
                worst_tap, worst_loss = max(worst_tap, tap_err), max(worst_loss, e["loss_rel"])
                print(name, f"tap {tap_err:.2e} loss {e['loss_rel']:.2e} loss in [{e['loss_min']:.3g}, {e['loss_max']:.3g}]", flush=True)
                assert tap_err <= 2e-6 and e["loss_rel"] <= 1e-5 and e["loss_min"] > 0, (name, e)
    stats["worst_fp32_tap_error"], stats["worst_fp32_distance_error"], stats["worst_fp32_loss_error"] = worst_tap, worst_d, worst_loss
    print("worst ATen fp32 tap error", worst_tap, "distance error", worst_d, "loss error", worst_loss)
    with open(os.path.join(HERE, "lpips_vgg_stats.json"), "w") as f:
        json.dump(stats, f, indent=1)
    for p in os.listdir(HERE):
        if p.startswith("lpips_vgg_"):
            assert os.path.getsize(os.path.join(HERE, p)) < SIZE_CAP, p
    print("wrote VGG fixtures to", HERE)


if __name__ == "__main__":
    main()
