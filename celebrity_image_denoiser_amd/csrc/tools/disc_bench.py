"""Times the discriminator forward (DenoiseDiscriminator, cid_disc_forward) on the GPU with device events after a warm-up, in eval and
train mode, next to the same network run by ATen/MIOpen fp32 in the same process and the generator's forward at the same shape.

Cases: B=16 256^2 (the trainer's batch, training.py:504-505) and B=256 128^2 (bench.py's shape).  For each: median ms per call over
--reps windows of --iters calls [min-max], images/s, algorithmic TFLOP/s (the four convolutions, 1.265 GFLOP per 128^2 image) and its
share of the 157.3 TFLOP/s fp32 MFMA peak.  The ATen baseline is the module's own stock nn.Sequential (the same weights and BatchNorm
containers) under torch.no_grad().

With --backward (train mode only) it also times one differentiable forward plus its backward, all 16 parameter gradients and the
input gradient: DenoiseDiscriminator(autograd=True) (cid_disc_forward_saved + cid_disc_backward) next to the stock nn.Sequential
through torch autograd (ATen/MIOpen).  The shares printed for these rows count 3x the forward's FLOPs (forward, data gradient,
weight gradient).

    python celebrity_image_denoiser_amd/csrc/tools/disc_bench.py [--reps 5] [--iters 20] [--case N,H,W ...] [--no-aten] [--no-gen]
                                                                 [--backward] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import celebrity_image_denoiser_amd as cid  # noqa: E402
from celebrity_image_denoiser_amd import synth  # noqa: E402

MFMA_F32_PEAK = 157.3e12
CASES = ((16, 256, 256), (256, 128, 128))


def disc_flops(n, h, w):
    """2 * MACs of layers 0, 2, 5, 8 and the 1x1 layer."""
    h2, w2 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    h4, w4 = (h2 - 1) // 2 + 1, (w2 - 1) // 2 + 1
    return 2.0 * n * (h * w * 64 * 27 + h2 * w2 * 64 * 576 + h2 * w2 * 128 * 576 + h4 * w4 * 128 * 1152 + 128)


def timed(fn, reps, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def summary(t, n, flops):
    med = statistics.median(t)
    return {"ms_median": med, "ms_min": min(t), "ms_max": max(t), "images_per_s": n / med * 1e3,
            "tflops": flops / med / 1e9, "mfma_share": flops / med / 1e-3 / MFMA_F32_PEAK}


def fmt(name, r):
    return (f"{name} {r['ms_median']:.3f} ms [{r['ms_min']:.3f}-{r['ms_max']:.3f}] {r['images_per_s']:.0f} img/s "
            f"{r['tflops']:.1f} TF/s {100 * r['mfma_share']:.0f}% of 157.3")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--case", action="append", default=None, help="N,H,W (repeatable); default: the two cases above")
    ap.add_argument("--no-aten", action="store_true", help="skip the ATen/MIOpen baseline")
    ap.add_argument("--no-gen", action="store_true", help="skip the generator's forward")
    ap.add_argument("--backward", action="store_true", help="also time forward_saved + backward (train mode) next to ATen's")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("disc_bench needs a GPU")
    dev = "cuda:0"
    cases = [tuple(int(v) for v in c.split(",")) for c in args.case] if args.case else CASES
    torch.manual_seed(0)
    disc = cid.load_discriminator(None, device=dev)
    disc_ag = cid.load_discriminator(disc.state_dict(), device=dev, autograd=True) if args.backward else None
    gen = None if args.no_gen else cid.load(synth.make_state_dict("default"), device=dev, strict=True)
    rows = []
    for n, h, w in cases:
        u8 = synth.add_gaussian_noise(synth.clean_images_u8(16, h, w), 25.0)
        x = torch.from_numpy(synth.normalize_u8(u8)).to(dev).repeat((n + 15) // 16, 1, 1, 1)[:n].contiguous()
        flops = disc_flops(n, h, w)
        row = {"N": n, "H": h, "W": w, "gflop": flops / 1e9}
        for mode in ("eval", "train"):
            disc.train(mode == "train")
            row[mode] = summary(timed(lambda: disc(x), args.reps, args.iters), n, flops)
            if not args.no_aten:
                with torch.no_grad():
                    row[mode + "_aten"] = summary(timed(lambda: disc.model(x).view(-1), args.reps, args.iters), n, flops)
        disc.eval()
        if args.backward:
            gp = torch.full((n,), -1.0 / n, device=dev)
            xg = x.clone().requires_grad_(True)

            def step(fwd, params):
                for q in params:
                    q.grad = None
                xg.grad = None
                fwd(xg).backward(gp)

            disc_ag.train()
            row["train_fwd_bwd"] = summary(timed(lambda: step(disc_ag, list(disc_ag.parameters())), args.reps, args.iters), n, 3 * flops)
            if not args.no_aten:
                disc.train()
                row["train_fwd_bwd_aten"] = summary(timed(lambda: step(lambda t: disc.model(t).view(-1), list(disc.parameters())),
                                                          args.reps, args.iters), n, 3 * flops)
                disc.eval()
            line = f"B={n:3d} {h}x{w} {3 * flops / 1e9:.0f} GFLOP train forward_saved + backward | " + fmt("hip", row["train_fwd_bwd"])
            if "train_fwd_bwd_aten" in row:
                line += " | " + fmt("aten", row["train_fwd_bwd_aten"]) + \
                    f" | hip/aten {row['train_fwd_bwd']['ms_median'] / row['train_fwd_bwd_aten']['ms_median']:.2f}"
            print(line, flush=True)
        if gen is not None:
            y = torch.empty_like(x)
            row["generator_ms_median"] = statistics.median(timed(lambda: gen(x, out=y), args.reps, max(1, args.iters // 4)))
        rows.append(row)
        for mode in ("eval", "train"):
            line = f"B={n:3d} {h}x{w} {flops / 1e9:.0f} GFLOP {mode:5s} | " + fmt("hip", row[mode])
            if mode + "_aten" in row:
                line += " | " + fmt("aten", row[mode + "_aten"]) + f" | hip/aten {row[mode]['ms_median'] / row[mode + '_aten']['ms_median']:.2f}"
            print(line, flush=True)
        if gen is not None:
            print(f"B={n:3d} {h}x{w} generator forward {row['generator_ms_median']:.3f} ms "
                  f"(train/eval {row['train']['ms_median'] / row['eval']['ms_median']:.2f})", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
