"""Times noise.add_noise() (cid_add_noise) on the GPU with device events after a warm-up, next to the forward at the same shape
and next to the numpy restatement (synth.add_noise_np) on the host.

Cases: B=256 at 128^2 (12.6 M subpixels) and 256^2 (50.3 M).  For each kind: ms per call (min / median / max over --reps windows
of --iters calls), the share of one forward_u8 at that shape, GB/s of the compulsory bytes (read + write of the uint8 batch), and
the numpy restatement's time for the same batch (--cpu-images images timed, scaled to B).

    python celebrity_image_denoiser_amd/csrc/tools/noise_bench.py [--reps 5] [--iters 20] [--cpu-images 16] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import celebrity_image_denoiser_amd as cid  # noqa: E402
from celebrity_image_denoiser_amd import noise, synth  # noqa: E402

CASES = ((256, 128, 128), (256, 256, 256))


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
    ap.add_argument("--cpu-images", type=int, default=16)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("noise_bench needs a GPU")
    dev = "cuda:0"
    model = cid.load(synth.make_state_dict("default"), device=dev, strict=True)
    rows = []
    for n, h, w in CASES:
        clean16 = synth.clean_images_u8(16, h, w, first_index=0)
        clean = torch.from_numpy(clean16).to(dev).repeat((n + 15) // 16, 1, 1, 1)[:n].contiguous()
        out = torch.empty_like(clean)
        nbytes = 2 * clean.numel()
        t = timed(lambda: model.forward_u8(clean, out_u8=False), args.reps, max(1, args.iters // 4))
        fwd = statistics.median(t)
        row = {"N": n, "H": h, "W": w, "subpixels": clean.numel(), "forward_ms_median": fwd}
        for kind in noise.NOISE_TYPES:
            t = timed(lambda: noise.add_noise(clean, kind, out=out), args.reps, args.iters)
            med = statistics.median(t)
            c = clean16[:args.cpu_images]
            t0 = time.perf_counter()
            synth.add_noise_np(c, kind)
            cpu_ms = (time.perf_counter() - t0) * 1e3 * n / len(c)
            row[kind] = {"ms_min": min(t), "ms_median": med, "ms_max": max(t), "GBps": nbytes / med / 1e6,
                         "forward_share": med / fwd, "numpy_ms": cpu_ms}
            print(f"B={n} {h}x{w} {kind:12s} {med:.4f} ms [{min(t):.4f}-{max(t):.4f}] {nbytes / med / 1e6:6.0f} GB/s "
                  f"{100 * med / fwd:5.2f}% of a forward ({fwd:.3f} ms) | numpy {cpu_ms:.0f} ms", flush=True)
        rows.append(row)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
