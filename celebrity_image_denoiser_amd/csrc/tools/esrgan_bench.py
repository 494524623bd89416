"""Times the ESRGAN forward (ESRGANGenerator, cid_esr_forward) on the GPU with device events after a warm-up, next to the same network
restated with the module's own stock nn containers on ATen/MIOpen fp32 in the same process.

Cases: B=16 256^2 and B=256 128^2.  For each: median ms per call over --reps windows of --iters calls [min-max], images/s, algorithmic
TFLOP/s (2 * MACs of the 9x9 head, the 2 R trunk convolutions and the 9x9 tail: 1.242 MFLOP per pixel at R = 8) and its share of the
157.3 TFLOP/s fp32 MFMA peak.  --residuals 0 times head + tail alone; the trunk's time per launch is the difference to R = 8 over 16.

    python celebrity_image_denoiser_amd/csrc/tools/esrgan_bench.py [--reps 5] [--iters 10] [--case N,H,W ...] [--residuals 8]
                                                                   [--no-aten] [--u8] [--json out.json]
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


def esr_flops(n, h, w, r):
    return 2.0 * n * h * w * (243 * 64 + 2 * r * 64 * 576 + 5184 * 3)


def aten_forward(m, x):
    """The reference's forward (app.py:215-218, ResidualBlock :199-200) on the module's stock containers."""
    x1 = m.initial(x)
    cur = x1
    for blk in m.residuals:
        cur = cur + blk.block(cur)
    return m.final(x1 + cur)


def timed(fn, reps, iters):
    for _ in range(2):
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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--case", action="append", default=None, help="N,H,W (repeatable); default: the two cases above")
    ap.add_argument("--residuals", type=int, default=8)
    ap.add_argument("--no-aten", action="store_true", help="skip the ATen/MIOpen baseline")
    ap.add_argument("--u8", action="store_true", help="also time the uint8 -> uint8 path")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("esrgan_bench needs a GPU")
    dev = "cuda:0"
    cases = [tuple(int(v) for v in c.split(",")) for c in args.case] if args.case else CASES
    r = args.residuals
    model = cid.load_esrgan(synth.make_esrgan_state_dict("default", r), num_residuals=r, device=dev, strict=True)
    rows = []
    for n, h, w in cases:
        u8 = torch.from_numpy(synth.esrgan_inputs_u8(16, h, w)).to(dev).repeat((n + 15) // 16, 1, 1, 1)[:n].contiguous()
        x = u8.to(torch.float32).div(255.0).permute(0, 3, 1, 2).contiguous()
        flops = esr_flops(n, h, w, r)
        row = {"N": n, "H": h, "W": w, "R": r, "gflop": flops / 1e9}
        row["hip"] = summary(timed(lambda: model(x), args.reps, args.iters), n, flops)
        line = f"B={n:3d} {h}x{w} R={r} {flops / 1e9:.0f} GFLOP | " + fmt("hip", row["hip"])
        if args.u8:
            row["hip_u8"] = summary(timed(lambda: model(u8), args.reps, args.iters), n, flops)
            line += " | " + fmt("hip u8", row["hip_u8"])
        if not args.no_aten:
            with torch.no_grad():
                row["aten"] = summary(timed(lambda: aten_forward(model, x), args.reps, args.iters), n, flops)
            line += " | " + fmt("aten", row["aten"]) + f" | hip/aten {row['hip']['ms_median'] / row['aten']['ms_median']:.2f}"
        rows.append(row)
        print(line, flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
