"""Times LPIPS (lpips.LPIPS, cid_lpips) on the GPU with device events after a warm-up, next to a torch restatement of the same
network on ATen/MIOpen fp32 in the same process, on the same GPU and the same inputs.

Cases: the pair batch at 128 x 128 (the trainers' size) for N = 64 and 256 pairs, the trainers' call (x*0.5+0.5).  Each case runs in a
process of its own (this script starts one child per case).  For each: median ms per call over --reps windows of --iters calls
[min-max], pairs/s, algorithmic TFLOP/s of the five convolutions (2 towers) and its share of the 157.3 TFLOP/s fp32 MFMA peak; and,
as yardsticks at the same batch, one generator forward and one cid_quality call (PSNR + SSIM).

--trace starts ONE `rocprofv3 --kernel-trace` run (no counters in it) of a few calls at the given N and prints per launch the count,
the mean and the minimum time, and the fp32-MFMA bound of the MFMA launches.

    python celebrity_image_denoiser_amd/csrc/tools/lpips_bench.py [--reps 5] [--iters 10] [--case N ...] [--no-aten] [--json out.json]
                                                                  [--trace N]
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
CASES = (64, 256)
SIDE = 128
# MACs per image of each launch at 128 x 128 (maps 31, 15, 7), in launch order
MACS = {"k_lpips_head": 961 * 363 * 64, "k_lpips_conv<64, 192, 5, true>": 225 * 1600 * 192, "k_lpips_conv<192, 384, 3, true>": 49 * 1728 * 384,
        "k_lpips_conv<384, 256, 3, false>": 49 * 3456 * 256, "k_lpips_conv<256, 256, 3, false>": 49 * 2304 * 256}


def lp_flops(n):
    return 2.0 * 2 * n * sum(MACS.values())


def aten_lpips(sd, a, b):
    """The definition (include/cid.h) on ATen: both towers as one batch, the trainers' x*0.5+0.5 first."""
    import torch
    import torch.nn.functional as F

    x = torch.cat([a, b]) * 0.5 + 0.5
    x = (x - sd["scaling_layer.shift"]) / sd["scaling_layer.scale"]
    n = a.shape[0]
    d = 0
    for k, (prefix, stride, pad, pool) in enumerate((("net.slice1.0", 4, 2, False), ("net.slice2.3", 1, 2, True), ("net.slice3.6", 1, 1, True),
                                                     ("net.slice4.8", 1, 1, False), ("net.slice5.10", 1, 1, False))):
        if pool:
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, sd[prefix + ".weight"], sd[prefix + ".bias"], stride=stride, padding=pad))
        u = x / (torch.sqrt(torch.sum(x * x, dim=1, keepdim=True)) + 1e-10)
        d = d + F.conv2d((u[:n] - u[n:]) ** 2, sd[f"lin{k}.model.1.weight"]).mean(dim=(2, 3))
    return d


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


def summary(t, n, flops=None):
    med = statistics.median(t)
    r = {"ms_median": med, "ms_min": min(t), "ms_max": max(t), "per_s": n / med * 1e3}
    if flops:
        r.update({"tflops": flops / med / 1e9, "mfma_share": flops / med / 1e-3 / MFMA_F32_PEAK})
    return r


def fmt(name, r):
    s = f"{name} {r['ms_median']:.4f} ms [{r['ms_min']:.4f}-{r['ms_max']:.4f}] {r['per_s']:.0f}/s"
    if "tflops" in r:
        s += f" {r['tflops']:.2f} TF/s {100 * r['mfma_share']:.1f}% of 157.3"
    return s


def setup(n):
    import torch

    import celebrity_image_denoiser_amd as cid
    from celebrity_image_denoiser_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("lpips_bench needs a GPU")
    dev = "cuda:0"
    sd = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_lpips_state_dict("default").items()}
    model = cid.load_lpips(sd, device=dev, strict=True)
    x, clean, _ = synth.make_batch(min(n, 16), SIDE, SIDE)
    reps = (n + x.shape[0] - 1) // x.shape[0]
    a = torch.from_numpy(x).to(dev).repeat(reps, 1, 1, 1)[:n].contiguous()
    b = torch.from_numpy(clean).to(dev).repeat(reps, 1, 1, 1)[:n].contiguous()
    return model, sd, a, b


def run_case(n, args):
    import torch

    import celebrity_image_denoiser_amd as cid
    from celebrity_image_denoiser_amd import metrics, synth

    model, sd, a, b = setup(n)
    flops = lp_flops(n)
    row = {"N": n, "side": SIDE, "gflop": flops / 1e9}
    row["hip"] = summary(timed(lambda: metrics.lpips(a, b, model, unit_view=True), args.reps, args.iters), n, flops)
    line = f"N={n:3d} pairs {SIDE}x{SIDE} {flops / 1e9:.2f} GFLOP | " + fmt("hip", row["hip"])
    if not args.no_aten:
        with torch.no_grad():
            want = aten_lpips(sd, a, b).view(-1).double()
            got = metrics.lpips(a, b, model, unit_view=True)
            row["max_rel_delta_vs_aten"] = float(((got - want).abs() / want).max())
            row["aten"] = summary(timed(lambda: aten_lpips(sd, a, b), args.reps, args.iters), n, flops)
        line += " | " + fmt("aten", row["aten"]) + f" | hip/aten {row['hip']['ms_median'] / row['aten']['ms_median']:.2f}"
        line += f" | max rel delta {row['max_rel_delta_vs_aten']:.1e}"
    gen = cid.load(synth.make_state_dict("default"), device="cuda:0", strict=True)
    row["generator"] = summary(timed(lambda: gen(a), args.reps, args.iters), n)
    row["quality"] = summary(timed(lambda: metrics.quality(a, b, ("psnr", "ssim")), args.reps, args.iters), n)
    line += " | " + fmt("generator forward", row["generator"]) + " | " + fmt("cid_quality psnr+ssim", row["quality"])
    print(line, flush=True)
    return row


def run_traced(n, args):
    """The child of --trace: a few plain calls, nothing else."""
    import torch

    from celebrity_image_denoiser_amd import metrics

    model, _, a, b = setup(n)
    for _ in range(args.trace_calls):
        metrics.lpips(a, b, model, unit_view=True)
    torch.cuda.synchronize()


def short_name(k):
    return k.split("(")[0].replace("void ", "").replace("cid::", "")


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
        if name.startswith("k_lpips_"):
            per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    print(f"per launch at N={n} pairs (one rocprofv3 --kernel-trace run of {args.trace_calls} calls, the first dropped; mean / min ms)")
    out, total = {}, 0.0
    for name, t in per.items():
        t = t[len(t) // args.trace_calls:]                 # drop the first call (it pays for code loading)
        mean, mn = statistics.mean(t), min(t)
        line = f"{name:36s} {len(t):3d} launches   {mean:.4f} / {mn:.4f}"
        if name in MACS:
            bnd = 2.0 * 2 * n * MACS[name] / MFMA_F32_PEAK * 1e3
            line += f"   fp32-MFMA bound {bnd:.4f} ms, share {bnd / mean:.2f}" + (" (VALU kernel)" if "head" in name else "")
        print(line)
        out[name] = mean
        total += mean
    print(f"sum of one call's launches {total:.4f} ms")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--case", action="append", type=int, default=None, help="N pairs (repeatable); default: 64 and 256, one process each")
    ap.add_argument("--no-aten", action="store_true", help="skip the ATen/MIOpen baseline")
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
                cmd += ["--no-aten"] * args.no_aten
                subprocess.run(cmd, check=True)
                rows += json.load(open(tf.name))
    if args.trace:
        rows.append({"trace": args.trace, "per_launch_ms": trace(args.trace, args)})
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
