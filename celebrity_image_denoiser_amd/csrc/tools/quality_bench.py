"""Times metrics.quality() (cid_quality) on the GPU with device events after a warm-up, next to the forward at the same shape.

Cases: B=16 256^2 (the trainer's batch), B=256 128^2, B=256 256^2 (402 MB of fp32 input: more than the 256 MiB Infinity Cache).
For each: ms per call for PSNR+SSIM and (sides > 160) for all three metrics, GB/s of the compulsory input bytes (both fp32 operands read
once) and that rate's share of the 8 TB/s HBM peak.  Repeats: --reps timed windows of --iters calls; min / median / max reported.

    python celebrity_image_denoiser_amd/csrc/tools/quality_bench.py [--reps 5] [--iters 20] [--json out.json]
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
from celebrity_image_denoiser_amd import metrics, synth  # noqa: E402

HBM_PEAK = 8.0e12
CASES = ((16, 256, 256), (256, 128, 128), (256, 256, 256))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quality_bench needs a GPU")
    dev = "cuda:0"
    model = cid.load(synth.make_state_dict("default"), device=dev, strict=True)
    rows = []
    for n, h, w in CASES:
        x16, c16, _ = synth.make_batch(16, h, w, first_index=0)
        reps_n = (n + 15) // 16
        x = torch.from_numpy(x16).to(dev).repeat(reps_n, 1, 1, 1)[:n].contiguous()
        c = torch.from_numpy(c16).to(dev).repeat(reps_n, 1, 1, 1)[:n].contiguous()
        y = torch.empty_like(x)
        in_bytes = 2 * x.numel() * 4
        row = {"N": n, "H": h, "W": w, "input_MB": in_bytes / 1e6}
        sets = [("psnr_ssim", ("psnr", "ssim"))]
        if min(h, w) > 160:         # MS-SSIM needs min(H, W) > 160
            sets.append(("all", ("psnr", "ssim", "ms_ssim")))
        for name, ms in sets:
            t = timed(lambda: metrics.quality(x, c, ms), args.reps, args.iters)
            med = statistics.median(t)
            row[name] = {"ms_min": min(t), "ms_median": med, "ms_max": max(t), "GBps": in_bytes / med / 1e6,
                         "hbm_share": in_bytes / med / 1e-3 / HBM_PEAK}
        t = timed(lambda: model(x, out=y), args.reps, max(1, args.iters // 4))
        row["forward_ms_median"] = statistics.median(t)
        rows.append(row)
        print(f"B={n:3d} {h}x{w} input {row['input_MB']:.0f} MB | "
              + " | ".join(f"{k}: {row[k]['ms_median']:.4f} ms [{row[k]['ms_min']:.4f}-{row[k]['ms_max']:.4f}] "
                           f"{row[k]['GBps']:.0f} GB/s {100 * row[k]['hbm_share']:.0f}% of 8 TB/s" for k, _ in sets)
              + f" | forward {row['forward_ms_median']:.3f} ms", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
