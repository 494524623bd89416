"""Times the two VGG16 entry points (LPIPS(net='vgg') -> cid_vgg_lpips, VGGPerceptualLoss -> cid_vgg_content_loss) on the GPU with
device events after a warm-up, next to a torch restatement of the same stack on ATen/MIOpen fp32 in the same process, on the same GPU
and the same inputs.

Cases: 64 pairs at 128 x 128 and 16 pairs at 256 x 256 (the trainers' size), the same number of pixels.  Each case runs in a process
of its own (this script starts one child per case).  For each entry point: the median ms per call over --iters individually timed
calls [min-max] after --warmup calls, the algorithmic TFLOP/s of the convolutions (2 towers) and that whole-call rate's share of the
157.3 TFLOP/s fp32 MFMA peak, hip and ATen alternating call by call in the same timed loop.

--trace starts ONE `rocprofv3 --kernel-trace` run (no counters in it) per case of a few cid_vgg_lpips calls and prints, per launch
in launch order, the mean and the minimum kernel time, the fp32-MFMA bound of the launch (its MACs over the peak) and the fraction of
the peak it reaches; the slowest launch is named.

--backward times the differentiable content loss instead: VGGPerceptualLoss(autograd=True)(x, y).backward() (cid_vgg_content_loss_saved
+ cid_vgg_content_backward, with torch's own mean / cast / accumulate around them) next to ATen fp32 autograd of the same slice with
x alone requiring grad, at 16 pairs of 256 x 256 (the SRGAN trainer's hr_size and batch_size) and 4 pairs of 128 x 128.  With --trace
the per-launch breakdown is that of the sixteen launches of one forward + backward.

    python celebrity_image_denoiser_amd/csrc/tools/vgg_bench.py [--iters 50] [--warmup 5] [--case N,SIDE ...] [--no-aten] [--trace]
                                                                [--backward] [--json out.json]
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
CASES = ((64, 128), (16, 256))
BWD_CASES = ((16, 256), (4, 128))
# (name, Cin, Cout, level): launch order of cid_vgg_lpips; the map of level k is (side >> k) squared
LAUNCHES = (("relu1_1 (head, VALU)", 3, 64, 0), ("relu1_2", 64, 64, 0), ("relu2_1", 64, 128, 1), ("relu2_2", 128, 128, 1), ("relu3_1", 128, 256, 2),
            ("relu3_2", 256, 256, 2), ("relu3_3", 256, 256, 2), ("relu4_1", 256, 512, 3), ("relu4_2", 512, 512, 3), ("relu4_3", 512, 512, 3),
            ("relu5_1", 512, 512, 4), ("relu5_2", 512, 512, 4), ("relu5_3", 512, 512, 4))


def macs(launch, side):
    _, cin, cout, level = launch
    return (side >> level) ** 2 * 9 * cin * cout


def flops(n, side, convs):
    """Both towers of n pairs through the first `convs` convolutions."""
    return 2.0 * 2 * n * sum(macs(l, side) for l in LAUNCHES[:convs])


def aten_features(sd, x, slices):
    import torch.nn.functional as F

    out = []
    for k, convs in enumerate(((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))[:slices]):
        if k:
            x = F.max_pool2d(x, 2, 2)
        for idx in convs:
            x = F.relu(F.conv2d(x, sd[f"net.slice{k + 1}.{idx}.weight"], sd[f"net.slice{k + 1}.{idx}.bias"], padding=1))
        out.append(x)
    return out


def aten_lpips(sd, a, b):
    """The definition (include/cid.h) on ATen: both towers as one batch, the trainers' x*0.5+0.5 first."""
    import torch
    import torch.nn.functional as F

    x = torch.cat([a, b]) * 0.5 + 0.5
    x = (x - sd["scaling_layer.shift"]) / sd["scaling_layer.scale"]
    n = a.shape[0]
    d = 0
    for k, t in enumerate(aten_features(sd, x, 5)):
        u = t / (torch.sqrt(torch.sum(t * t, dim=1, keepdim=True)) + 1e-10)
        d = d + F.conv2d((u[:n] - u[n:]) ** 2, sd[f"lin{k}.model.1.weight"]).mean(dim=(2, 3))
    return d


def aten_content(sd, a, b):
    import torch

    t = aten_features(sd, torch.cat([a, b]), 3)[2]
    n = a.shape[0]
    return ((t[:n] - t[n:]) ** 2).mean(dim=(1, 2, 3))


# launch order of the backward: (name, forward convolution whose data gradient it is, or None)
BWD_LAUNCHES = (("grad3_3 (seed)", None), ("grad3_2", 6), ("grad3_1", 5), ("gradpool2", 4), ("grad2_1", 3), ("gradpool1", 2), ("grad1_1", 1),
                ("grad_a (head, VALU)", 0))


def train_flops(n, side):
    """Forward of both towers and the data gradient of tower a through the seven convolutions."""
    return 2.0 * 3 * n * sum(macs(l, side) for l in LAUNCHES[:7])


def aten_content_train(sd, x, b):
    """ATen fp32 autograd of the trainer's scalar with x alone requiring grad."""
    import torch

    with torch.no_grad():
        fb = aten_features(sd, b, 3)[2]
    return ((aten_features(sd, x, 3)[2] - fb) ** 2).mean()


def timed_alternating(fns, warmup, iters):
    """Each function's per-call ms: every call between its own pair of events, the functions taking turns call by call."""
    import torch

    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[i].append(e0.elapsed_time(e1))
    return times


def summary(t, fl):
    med = statistics.median(t)
    return {"ms_median": med, "ms_min": min(t), "ms_max": max(t), "calls": len(t), "tflops": fl / med / 1e9,
            "mfma_share_whole_call": fl / med / 1e-3 / MFMA_F32_PEAK}


def fmt(name, r):
    return (f"{name} {r['ms_median']:.3f} ms [{r['ms_min']:.3f}-{r['ms_max']:.3f}] over {r['calls']} calls, {r['tflops']:.1f} TF/s = "
            f"{100 * r['mfma_share_whole_call']:.1f}% of 157.3 (whole call)")


def setup(n, side):
    import torch

    import celebrity_image_denoiser_amd as cid
    from celebrity_image_denoiser_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("vgg_bench needs a GPU")
    dev = "cuda:0"
    np_sd = synth.make_lpips_state_dict("default", net="vgg")
    sd = {k: torch.from_numpy(v).to(dev) for k, v in np_sd.items()}
    model = cid.load_lpips(sd, device=dev, strict=True, net="vgg")
    loss = cid.load_vgg_loss({k: torch.from_numpy(v) for k, v in synth.vgg_loss_state_dict(np_sd).items()}, device=dev)
    x, clean, _ = synth.make_batch(min(n, 8), side, side)
    reps = (n + x.shape[0] - 1) // x.shape[0]
    a = torch.from_numpy(x).to(dev).repeat(reps, 1, 1, 1)[:n].contiguous()
    b = torch.from_numpy(clean).to(dev).repeat(reps, 1, 1, 1)[:n].contiguous()
    return model, loss, sd, a, b


def run_case(n, side, args):
    import torch

    model, loss, sd, a, b = setup(n, side)
    row = {"N": n, "side": side}
    with torch.no_grad():
        for name, hip, aten, convs in (("lpips", lambda: model.distances(a, b, unit_view=True), lambda: aten_lpips(sd, a, b), 13),
                                       ("content_loss", lambda: loss.per_image(a, b), lambda: aten_content(sd, a, b), 7)):
            fl = flops(n, side, convs)
            fns = [hip] if args.no_aten else [hip, aten]
            t = timed_alternating(fns, args.warmup, args.iters)
            row[name] = {"gflop": fl / 1e9, "hip": summary(t[0], fl)}
            line = f"N={n:3d} pairs {side}x{side} {name:12s} {fl / 1e9:.1f} GFLOP | " + fmt("hip", row[name]["hip"])
            if not args.no_aten:
                want, got = aten().view(-1).double(), hip()
                row[name]["max_rel_delta_vs_aten"] = float(((got - want).abs() / want).max())
                row[name]["aten"] = summary(t[1], fl)
                line += " | " + fmt("aten", row[name]["aten"]) + f" | hip/aten {row[name]['hip']['ms_median'] / row[name]['aten']['ms_median']:.2f}"
                line += f" | max rel delta {row[name]['max_rel_delta_vs_aten']:.1e}"
            print(line, flush=True)
    return row


def setup_backward(n, side):
    import torch

    import celebrity_image_denoiser_amd as cid
    from celebrity_image_denoiser_amd import synth

    _, _, sd, a, b = setup(n, side)
    np_sd = synth.make_lpips_state_dict("default", net="vgg")
    loss = cid.load_vgg_loss({k: torch.from_numpy(v) for k, v in synth.vgg_loss_state_dict(np_sd).items()}, device="cuda:0", autograd=True)
    return loss, sd, a.requires_grad_(True), b


def run_backward_case(n, side, args):
    import torch

    loss, sd, a, b = setup_backward(n, side)
    a2 = a.detach().clone().requires_grad_(True)

    def hip():
        a.grad = None
        loss(a, b).backward()

    def aten():
        a2.grad = None
        aten_content_train(sd, a2, b).backward()

    fl = train_flops(n, side)
    t = timed_alternating([hip] if args.no_aten else [hip, aten], args.warmup, args.iters)
    row = {"N": n, "side": side, "content_loss_backward": {"gflop": fl / 1e9, "hip": summary(t[0], fl)}}
    r = row["content_loss_backward"]
    line = f"N={n:3d} pairs {side}x{side} loss + backward {fl / 1e9:.1f} GFLOP | " + fmt("hip", r["hip"])
    if not args.no_aten:
        hip(), aten()
        # two fp32 runs decide some of the 1e8 ReLU units and pool windows differently, and each such unit moves a few pixels of the
        # gradient by a visible amount: the maximum is theirs; the share of elements beyond 1e-5 of the scale says how few they are
        # (the accuracy claim is tests/test_vgg_backward.py's, against float64 with each run's own decisions)
        delta, scale = (a.grad - a2.grad).abs(), float(a2.grad.abs().max())
        r["max_delta_vs_aten_over_max"] = float(delta.max()) / scale
        r["share_beyond_1e-5_of_max"] = float((delta > 1e-5 * scale).double().mean())
        r["aten"] = summary(t[1], fl)
        line += " | " + fmt("aten", r["aten"]) + f" | hip/aten {r['hip']['ms_median'] / r['aten']['ms_median']:.2f}"
        line += f" | max|delta| / max|grad| {r['max_delta_vs_aten_over_max']:.1e}, {100 * r['share_beyond_1e-5_of_max']:.4f}% of the elements beyond 1e-5"
    print(line, flush=True)
    return row


def run_traced_backward(n, side, calls):
    """The child of --backward --trace: a few forward + backward calls, nothing else."""
    import torch

    loss, _, a, b = setup_backward(n, side)
    for _ in range(calls):
        a.grad = None
        loss(a, b).backward()
    torch.cuda.synchronize()


def trace_rows(n, side, args, extra, kernels):
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--traced-child", f"{n},{side}", "--trace-calls", str(args.trace_calls)] + extra
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            raise SystemExit(f"rocprofv3 failed ({r.returncode}):\n{r.stderr[-2000:]}")
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(f, newline="") as fh:
                rows += list(csv.DictReader(fh))
    if not rows:
        raise SystemExit("rocprofv3 wrote no kernel trace")
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [r for r in rows if any(k in r["Kernel_Name"] for k in kernels)]


def trace_backward(n, side, args):
    """Per launch of one forward + backward, in launch order: mean and min ms, the launch's fp32-MFMA bound and its fraction of peak."""
    ours = trace_rows(n, side, args, ["--backward"], ("k_vgg_head", "k_lpips_conv", "k_vgg_content", "k_vgg_seed", "k_vgg_dgrad"))
    names = [(l[0], 2 * macs(l, side)) for l in LAUNCHES[:7]] + [("loss (float64, VALU)", 0)]
    names += [(name, macs(LAUNCHES[conv], side) if conv is not None else 0) for name, conv in BWD_LAUNCHES]
    per_call = len(names)
    if len(ours) != per_call * args.trace_calls:
        raise SystemExit(f"expected {per_call * args.trace_calls} launches in the trace, found {len(ours)}")
    print(f"per launch of loss + backward at N={n} pairs {side}x{side} (one rocprofv3 --kernel-trace run of {args.trace_calls} calls, the first "
          "dropped; mean / min ms)")
    out, total = {}, 0.0
    for i, (name, m) in enumerate(names):
        t = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in ours[per_call + i::per_call]]
        mean, mn = statistics.mean(t), min(t)
        kernel = ours[i]["Kernel_Name"].split("(")[0].replace("void ", "").replace("cid::", "")
        line = f"{name:26s} {kernel:48s} {mean:8.4f} / {mn:8.4f}"
        if m:
            bnd = 2.0 * n * m / MFMA_F32_PEAK * 1e3
            line += f"   fp32-MFMA bound {bnd:7.4f} ms, fraction of peak {bnd / mean:.3f}"
        print(line)
        out[name] = {"kernel": kernel, "ms_mean": mean, "ms_min": mn}
        total += mean
    fwd = sum(v["ms_mean"] for v in list(out.values())[:8])
    print(f"sum of one call's launches {total:.4f} ms: forward {fwd:.4f}, backward {total - fwd:.4f}")
    return out


def run_traced(n, side, calls):
    """The child of --trace: a few plain cid_vgg_lpips calls, nothing else."""
    import torch

    model, _, _, a, b = setup(n, side)
    for _ in range(calls):
        model.distances(a, b, unit_view=True)
    torch.cuda.synchronize()


def trace(n, side, args):
    """One rocprofv3 --kernel-trace run of this script's traced child; per launch of one call, in launch order: mean and min ms."""
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--traced-child", f"{n},{side}", "--trace-calls", str(args.trace_calls)]
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
    ours = [r for r in rows if any(k in r["Kernel_Name"] for k in ("k_vgg_head", "k_lpips_conv", "k_lpips_dist"))]
    per_call = len(LAUNCHES) + 1                                   # + the distance kernel
    if len(ours) != per_call * args.trace_calls:
        raise SystemExit(f"expected {per_call * args.trace_calls} launches in the trace, found {len(ours)}")
    names = [l[0] for l in LAUNCHES] + ["distance (float64, VALU)"]
    print(f"per launch at N={n} pairs {side}x{side} (one rocprofv3 --kernel-trace run of {args.trace_calls} calls, the first dropped; mean / min ms)")
    out, total, slowest = {}, 0.0, None
    for i, name in enumerate(names):
        t = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in ours[per_call + i::per_call]]
        mean, mn = statistics.mean(t), min(t)
        kernel = ours[i]["Kernel_Name"].split("(")[0].replace("void ", "").replace("cid::", "")
        line = f"{name:26s} {kernel:44s} {mean:8.4f} / {mn:8.4f}"
        if i < len(LAUNCHES):
            bnd = 2.0 * 2 * n * macs(LAUNCHES[i], side) / MFMA_F32_PEAK * 1e3
            line += f"   fp32-MFMA bound {bnd:7.4f} ms, fraction of peak {bnd / mean:.3f}"
            if i and (slowest is None or mean > slowest[1]):
                slowest = (name, mean, bnd / mean)
        print(line)
        out[name] = {"kernel": kernel, "ms_mean": mean, "ms_min": mn}
        total += mean
    print(f"sum of one call's launches {total:.4f} ms; slowest trunk launch: {slowest[0]} at {slowest[1]:.4f} ms, {slowest[2]:.3f} of the peak")
    return out


def parse_case(s):
    n, side = s.split(",")
    return int(n), int(side)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--case", action="append", type=parse_case, default=None, help="N,SIDE (repeatable); default: 64,128 and 16,256")
    ap.add_argument("--no-aten", action="store_true", help="skip the ATen/MIOpen baseline")
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace", action="store_true", help="per-launch times of each case from one rocprofv3 --kernel-trace run")
    ap.add_argument("--trace-calls", type=int, default=4)
    ap.add_argument("--backward", action="store_true", help="time VGGPerceptualLoss(autograd=True) forward + backward against ATen autograd")
    ap.add_argument("--traced-child", type=parse_case, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.traced_child:
        (run_traced_backward if args.backward else run_traced)(*args.traced_child, args.trace_calls)
        return
    if args.child:
        rows = [(run_backward_case if args.backward else run_case)(n, side, args) for n, side in args.case]
    else:
        rows = []
        for n, side in (args.case or (BWD_CASES if args.backward else CASES)):
            # each case in a process of its own: allocator state and clocks of one do not reach the next
            with tempfile.NamedTemporaryFile(suffix=".json") as tf:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--case", f"{n},{side}", "--iters", str(args.iters),
                       "--warmup", str(args.warmup), "--json", tf.name]
                cmd += ["--no-aten"] * args.no_aten + ["--backward"] * args.backward
                subprocess.run(cmd, check=True)
                rows += json.load(open(tf.name))
            if args.trace:
                rows.append({"trace": [n, side], "per_launch": (trace_backward if args.backward else trace)(n, side, args)})
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
