"""Times the cGAN forward (CGANGenerator, cid_cg_forward) on the GPU with device events after a warm-up, next to the same network run
through the module's own stock nn containers on ATen/MIOpen fp32 in the same process.

Cases: N = 1, 16 and 256 images (the sizes are fixed by the model: 100 + label -> 3 x 64 x 64).  Each case runs in a process of its
own (this script starts one child per case).  For each: median ms per call over --reps windows of --iters calls [min-max], images/s,
algorithmic TFLOP/s (2 * 89,063,424 MACs per image: the linear, the three transposed convolutions and the tail) and its share of
the 157.3 TFLOP/s fp32 MFMA peak.

--trace starts ONE `rocprofv3 --kernel-trace` run (no counters in it) of a few forwards at the given N and prints per launch the
count, the mean and the minimum time, and the fp32-MFMA bound of the MFMA launches.

    python celebrity_image_denoiser_amd/csrc/tools/cgan_bench.py [--reps 5] [--iters 20] [--case N ...] [--no-aten] [--no-u8]
                                                                 [--json out.json] [--trace N]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

MFMA_F32_PEAK = 157.3e12
CASES = (1, 16, 256)
# MACs per image of each launch, in launch order
MACS = {"k_cg_linear": 200 * 8192, "k_cg_up<128, 128, 8>": 256 * 128 * 128 * 4, "k_cg_up<128, 64, 16>": 1024 * 64 * 128 * 4,
        "k_cg_up<64, 32, 32>": 4096 * 32 * 64 * 4, "k_cg_tail": 4096 * 3 * 32 * 9}


def cg_flops(n):
    return 2.0 * n * sum(MACS.values())


def aten_forward(m, z, labels):
    """The reference's label branch (app.py:132-138) on the module's stock containers."""
    import torch

    x = torch.cat([z, m.label_emb(labels)], dim=1)
    return torch.tanh(m.model(m.l1(x).view(z.size(0), 128, 8, 8)))


def timed(fn, reps, iters):
    import torch

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
    return (f"{name} {r['ms_median']:.4f} ms [{r['ms_min']:.4f}-{r['ms_max']:.4f}] {r['images_per_s']:.0f} img/s "
            f"{r['tflops']:.2f} TF/s {100 * r['mfma_share']:.1f}% of 157.3")


def setup(n):
    import torch

    import celebrity_image_denoiser_amd as cid
    from celebrity_image_denoiser_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("cgan_bench needs a GPU")
    dev = "cuda:0"
    model = cid.load_cgan(synth.make_cgan_state_dict("default"), device=dev, strict=True)
    z = cid.latent(n, 1, device=dev)
    labels = (torch.arange(n, device=dev) % 10).to(torch.int64)
    return model, z, labels


def run_case(n, args):
    import torch

    model, z, labels = setup(n)
    flops = cg_flops(n)
    row = {"N": n, "gflop": flops / 1e9}
    row["hip"] = summary(timed(lambda: model(z, labels), args.reps, args.iters), n, flops)
    line = f"N={n:3d} {flops / 1e9:.2f} GFLOP | " + fmt("hip", row["hip"])
    if not args.no_u8:
        row["hip_u8"] = summary(timed(lambda: model(z, labels, out_dtype=torch.uint8), args.reps, args.iters), n, flops)
        line += " | " + fmt("hip u8", row["hip_u8"])
    if not args.no_aten:
        with torch.no_grad():
            row["aten"] = summary(timed(lambda: aten_forward(model, z, labels), args.reps, args.iters), n, flops)
        line += " | " + fmt("aten", row["aten"]) + f" | hip/aten {row['hip']['ms_median'] / row['aten']['ms_median']:.2f}"
    print(line, flush=True)
    return row


def run_traced(n, args):
    """The child of --trace: a few plain forwards, nothing else."""
    import torch

    model, z, labels = setup(n)
    for _ in range(args.trace_calls):
        model(z, labels)
    torch.cuda.synchronize()


def short_name(k):
    k = k.split("(")[0].replace("void ", "").replace("cid::", "")
    return k.split("<")[0] if k.startswith("k_cg_tail") else k


def trace(n, args):
    """One rocprofv3 --kernel-trace run of this script's traced child; per kernel: launches, mean and min ms, in launch order."""
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--traced-child", str(n), "--trace-calls", str(args.trace_calls)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            raise SystemExit(f"rocprofv3 failed ({r.returncode}):\n{r.stderr[-2000:]}")
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise SystemExit("rocprofv3 wrote no kernel trace")
        rows = []
        for f in files:
            with open(f, newline="") as fh:
                rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = {}
    for r in rows:
        name = short_name(r["Kernel_Name"])
        if name.startswith("k_cg_") and "latent" not in name:
            per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    print(f"per launch at N={n} (one rocprofv3 --kernel-trace run of {args.trace_calls} forwards, the first dropped; mean / min ms)")
    out, total = {}, 0.0
    for name, t in per.items():
        t = t[len(t) // args.trace_calls:]                 # drop the first forward (it pays for code loading)
        mean, mn = statistics.mean(t), min(t)
        line = f"{name:24s} {len(t):3d} launches   {mean:.4f} / {mn:.4f}"
        if name in MACS and "tail" not in name:
            b = 2.0 * n * MACS[name] / MFMA_F32_PEAK * 1e3
            line += f"   fp32-MFMA bound {b:.4f} ms, share {b / mean:.2f}"
        print(line)
        out[name] = mean
        total += mean
    print(f"sum of one forward's launches {total:.4f} ms")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--case", action="append", type=int, default=None, help="N (repeatable); default: 1, 16 and 256, one process each")
    ap.add_argument("--no-aten", action="store_true", help="skip the ATen/MIOpen baseline")
    ap.add_argument("--no-u8", action="store_true", help="skip the uint8 output")
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace", type=int, default=None, help="N: per-launch times at this batch size from one rocprofv3 --kernel-trace run")
    ap.add_argument("--trace-calls", type=int, default=4)
    ap.add_argument("--traced-child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.traced_child:
        run_traced(args.traced_child, args)
        return
    rows = []
    if args.child:
        rows = [run_case(c, args) for c in args.case]
    elif args.case or not args.trace:
        for c in (args.case or CASES):
            # each case in a process of its own: allocator state and clocks of one do not reach the next
            with tempfile.NamedTemporaryFile(suffix=".json") as tf:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--case", str(c), "--reps", str(args.reps), "--iters", str(args.iters),
                       "--json", tf.name]
                cmd += ["--no-aten"] * args.no_aten + ["--no-u8"] * args.no_u8
                subprocess.run(cmd, check=True)
                rows += json.load(open(tf.name))
    if args.trace:
        rows.append({"trace": args.trace, "per_launch_ms": trace(args.trace, args)})
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
