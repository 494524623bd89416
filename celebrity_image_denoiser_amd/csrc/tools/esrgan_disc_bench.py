"""Times the ESRGAN discriminator forward (ESRGANDiscriminator, cid_esd_forward) on the GPU with device events after a warm-up, next
to the same network run by ATen/MIOpen fp32 in the same process.

Cases: B=8 and B=16 at 256^2 (the ESRGAN trainer's batch_size = 8, input_shape = (3, 256, 256)).  For each: median ms per call over
--reps windows of --iters calls [min-max] after 3 warm-up calls, images/s, algorithmic TFLOP/s (the four convolutions and the linear
layer) and its share of the 157.3 TFLOP/s fp32 MFMA peak, and the workgroups of each launch.  The ATen baseline is a stock nn.Module
of the reference's structure with the same weights under torch.no_grad().

Each launch's share of a forward comes from a kernel trace taken in a run of its own (tracing slows the host, so the timings above
are taken with the profiler off; no counters are collected in that run):

    python .../esrgan_disc_bench.py --shares [--case 8,256,256]

starts `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python .../esrgan_disc_bench.py --case ... --no-aten --reps 1
--iters 5` as a child process and prints, per kernel, its calls, average time, share of the traced time and, for the MFMA layers, the
share of the fp32 MFMA peak its average time amounts to.  --shares-csv PATH summarises an existing kernel_stats CSV (no GPU needed).

--backward times the differentiable path instead: cid_esd_forward_saved alone (next to cid_esd_forward: the same launches), and
cid_esd_forward_saved + cid_esd_backward with all ten parameter gradients and the input gradient, against ATen/MIOpen fp32 autograd of
the stock module (forward + torch.autograd.grad of the same eleven tensors) in the same process, the two alternating window by window.
--shares --backward traces such a run (in a child process of its own, no counters) and lists the backward launches too.

    python celebrity_image_denoiser_amd/csrc/tools/esrgan_disc_bench.py [--reps 5] [--iters 20] [--case N,H,W ...] [--no-aten] [--backward]
                                                                        [--json out.json]
"""
import argparse
import csv
import ctypes
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
CASES = ((8, 256, 256), (16, 256, 256))
CONVS = (("conv1", 3, 64), ("conv2", 64, 128), ("conv3", 128, 256), ("conv4", 256, 512))
TILE_ROWS = {"conv2": 16, "conv3": 8, "conv4": 4}   # k_esd_conv: 4 * PT output rows x 16 columns x 64 channels per workgroup


def half(v):
    return (v - 1) // 2 + 1


def layer_table(n, h, w):
    """name -> (2 * MACs, workgroups) of each launch of one forward."""
    out = {}
    for name, cin, cout in CONVS:
        h, w = half(h), half(w)
        flops = 2.0 * n * h * w * cout * cin * 9
        if name == "conv1":
            wgs = n * -(-h * w // 256)
        else:
            wgs = n * -(-h // TILE_ROWS[name]) * -(-w // 16) * (cout // 64)
        out[name] = (flops, wgs)
    out["fc"] = (2.0 * n * 512 * h * w, n)
    return out


# the backward's MFMA launches (api/esrgan_disc_backward.h): dz channels per weight-gradient workgroup and its target splits; input
# channels and class rows per data-gradient workgroup
BWD_WG = {"conv2": (128, 64), "conv3": (128, 16), "conv4": (64, 2)}
BWD_DG = {"conv2": (64, 16), "conv3": (128, 8), "conv4": (128, 4)}


def backward_table(n, h, w):
    """name -> (2 * MACs, workgroups) of each MFMA or VALU launch of one backward."""
    out = {}
    sides = [(h, w)]
    for _ in CONVS:
        sides.append((half(sides[-1][0]), half(sides[-1][1])))
    for i, (name, cin, cout) in enumerate(CONVS):
        (hi, wi), (ho, wo) = sides[i], sides[i + 1]
        flops = 2.0 * n * ho * wo * cout * cin * 9
        if name == "conv1":
            out["wgrad1"] = (flops, min(n * -(-ho * wo // 64), 256))
            out["dgrad1"] = (flops, n * 4 * -(-(-(-hi // 2) * -(-wi // 2)) // 256))
            continue
        cd, target = BWD_WG[name]
        items = n * -(-ho // 4) * -(-wo // 16)
        out["wgrad" + name[-1]] = (flops, min(items, max(target, -(-items // 2048))) * (cin // 16) * (cout // cd))
        cxw, th = BWD_DG[name]
        out["dgrad" + name[-1]] = (flops, n * -(-(-(-hi // 2)) // th) * -(-(-(-wi // 2)) // 16) * 4 * (cin // cxw))
    out["fc_bwd"] = (2.0 * n * 512 * sides[4][0] * sides[4][1], 512 * sides[4][0] * sides[4][1] // 256)
    return out


def esd_flops(n, h, w):
    return sum(f for f, _ in layer_table(n, h, w).values())


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


def timed_alternating(fns, reps, iters):
    """timed() of several callables whose windows alternate: window r of each before window r + 1 of any."""
    import torch

    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) / iters)
    return out


def summary(t, n, flops):
    med = statistics.median(t)
    return {"ms_median": med, "ms_min": min(t), "ms_max": max(t), "images_per_s": n / med * 1e3,
            "tflops": flops / med / 1e9, "mfma_share": flops / med / 1e-3 / MFMA_F32_PEAK}


def fmt(name, r):
    return (f"{name} {r['ms_median']:.3f} ms [{r['ms_min']:.3f}-{r['ms_max']:.3f}] {r['images_per_s']:.0f} img/s "
            f"{r['tflops']:.1f} TF/s {100 * r['mfma_share']:.0f}% of 157.3")


# kernel name prefix -> the launch it is, for --shares
LAUNCHES = (("k_esd_conv1", "conv1"), ("k_esd_conv<64, 128", "conv2"), ("k_esd_conv<128, 256", "conv3"), ("k_esd_conv<256, 512", "conv4"),
            ("k_esd_fc_bwd", "fc_bwd"), ("k_esd_fc(", "fc"), ("k_esd_trainer_losses", "losses"), ("k_esd_losses", "losses"),
            ("k_esd_wgrad<128, 64", "wgrad2"), ("k_esd_wgrad<128, 128", "wgrad3"), ("k_esd_wgrad<64, 256", "wgrad4"),
            ("k_esd_dgrad<128, 64", "dgrad2"), ("k_esd_dgrad<256, 128", "dgrad3"), ("k_esd_dgrad<512, 256", "dgrad4"),
            ("k_esd_wgrad1", "wgrad1"), ("k_esd_dgrad1", "dgrad1"), ("k_disc_wgrad_reduce", "reduce"), ("k_disc_wgrad0_reduce", "reduce1"))


def shares(path, case):
    """Per-launch share of the traced time from a rocprofv3 kernel_stats CSV."""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            hit = [launch for prefix, launch in LAUNCHES if "cid::" + prefix in name]
            if hit:
                rows.append((hit[0], name, int(r["Calls"]), float(r["TotalDurationNs"]), float(r["AverageNs"]), float(r["MinNs"]),
                             float(r["MaxNs"])))
    if not rows:
        raise SystemExit(f"{path}: no ESRGAN discriminator kernels in the trace")
    total = sum(r[3] for r in rows)
    table = dict(layer_table(*case), **backward_table(*case))
    print(f"# share of the traced discriminator kernel time ({total / 1e6:.3f} ms over all calls), case N,H,W = {case}")
    for launch, name, calls, tot, mean, lo, hi in sorted(rows, key=lambda r: -r[3]):
        short = name.split("(")[0].replace("void ", "")
        line = f"{launch:7s} {short:44s} calls {calls:4d}  avg {mean / 1e3:8.1f} us  min {lo / 1e3:8.1f}  max {hi / 1e3:8.1f}  share {100 * tot / total:5.1f}%"
        if launch in table:
            flops, wgs = table[launch]
            line += f"  workgroups {wgs:5d}"
            if launch[:5] in ("conv2", "conv3", "conv4", "wgrad", "dgrad") and not launch.endswith("1"):
                line += f"  MFMA share {flops / MFMA_F32_PEAK / (mean * 1e-9):.2f}"
        print(line)


def traced_shares(case, backward=False):
    """Run this program under rocprofv3 as a child process (kernel trace and statistics only) and summarise its CSV."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--case", ",".join(map(str, case)), "--no-aten", "--reps", "1", "--iters", "5"] + (["--backward"] if backward else [])
        print("# " + " ".join(cmd), flush=True)
        subprocess.run(cmd, check=True, timeout=600)
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise SystemExit("rocprofv3 wrote no kernel_stats CSV")
        shares(found[0], case)


def backward_case(cid, torch, sd, x, args):
    """One case of --backward -> the result row."""
    from celebrity_image_denoiser_amd import _lib
    from celebrity_image_denoiser_amd.esrgan_disc import _GradsArg

    n, _, h, w = x.shape
    dev = x.device
    L = _lib.lib()
    disc = cid.load_esrgan_discriminator(sd, device=dev, input_shape=(3, h, w))

    def size(fn):
        out = ctypes.c_size_t()
        disc._check(getattr(L, fn)(n, h, w, ctypes.byref(out)))
        return out.value

    saved = torch.empty(size("cid_esd_saved_bytes"), dtype=torch.uint8, device=dev)
    ws = torch.empty(size("cid_esd_backward_workspace_bytes"), dtype=torch.uint8, device=dev)
    logits = torch.empty(n, dtype=torch.float32, device=dev)
    gl = torch.linspace(0.02, 0.1, n, device=dev)   # one sign: no gradient is a sum that cancels
    grads = {k: torch.empty_like(p) for k, p in disc.named_parameters()}
    gx = torch.empty_like(x)
    g = _GradsArg()
    for i, layer in enumerate(("conv1", "conv2", "conv3", "conv4", "fc")):
        g.w[i], g.b[i] = grads[layer + ".weight"].data_ptr(), grads[layer + ".bias"].data_ptr()
    g.input = gx.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def fwd_saved():
        disc._check(L.cid_esd_forward_saved(disc._cid, x.data_ptr(), 0, logits.data_ptr(), n, h, w, saved.data_ptr(), saved.numel(), stream))

    def fwd_bwd():
        fwd_saved()
        disc._check(L.cid_esd_backward(disc._cid, x.data_ptr(), 0, gl.data_ptr(), n, h, w, saved.data_ptr(), saved.numel(), ctypes.byref(g),
                                       ws.data_ptr(), ws.numel(), stream))

    flops = esd_flops(n, h, w)
    fns = [lambda: disc(x), fwd_saved, fwd_bwd]
    if not args.no_aten:
        stock = torch.nn.ModuleDict({name: torch.nn.Conv2d(cin, cout, 3, stride=2, padding=1) for name, cin, cout in CONVS})
        stock["fc"] = torch.nn.Linear(sd["fc.weight"].shape[1], 1)
        stock.load_state_dict(sd, strict=True)
        stock.to(dev)
        xa = x.clone().requires_grad_(True)
        leaves = [xa] + list(stock.parameters())
        box = {}

        def aten():
            t = xa
            for name, _, _ in CONVS:
                t = torch.nn.functional.leaky_relu(stock[name](t), 0.2)
            out = stock["fc"](t.view(n, -1))
            box["grads"] = torch.autograd.grad(out, leaves, gl.view(n, 1))

        fns.append(aten)
    t = timed_alternating(fns, args.reps, args.iters)
    row = {"N": n, "H": h, "W": w, "forward": summary(t[0], n, flops), "forward_saved": summary(t[1], n, flops),
           "forward_backward": summary(t[2], n, 3 * flops), "workgroups": {k: v[1] for k, v in backward_table(n, h, w).items()}}
    print(f"B={n:3d} {h}x{w} | " + fmt("forward", row["forward"]) + " | " + fmt("forward_saved", row["forward_saved"]), flush=True)
    line = "    " + fmt("forward_saved + backward", row["forward_backward"])
    if not args.no_aten:
        row["aten_forward_backward"] = summary(t[3], n, 3 * flops)
        ours = [gx] + [grads[k] for k, _ in disc.named_parameters()]
        row["max_rel_diff"] = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(ours, box["grads"]))
        lo, hi = row["aten_forward_backward"]["ms_min"], row["aten_forward_backward"]["ms_max"]
        med = row["forward_backward"]["ms_median"]
        verdict = "below ATen's windows" if med < lo else ("inside ATen's windows" if med <= hi else "above ATen's windows")
        line += (" | " + fmt("aten autograd", row["aten_forward_backward"]) +
                 f" | hip/aten {med / row['aten_forward_backward']['ms_median']:.2f} ({verdict}) | max rel diff {row['max_rel_diff']:.1e}")
    print(line, flush=True)
    print("    workgroups per backward launch: " + ", ".join(f"{k} {v}" for k, v in row["workgroups"].items()), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--case", action="append", default=None, help="N,H,W (repeatable); default: the two cases above")
    ap.add_argument("--no-aten", action="store_true", help="skip the ATen/MIOpen baseline")
    ap.add_argument("--shares", action="store_true", help="trace a run of the last case under rocprofv3 and print each launch's share")
    ap.add_argument("--shares-csv", default=None, help="a rocprofv3 kernel_stats CSV of a traced run: print each launch's share and exit")
    ap.add_argument("--backward", action="store_true", help="time forward_saved and forward_saved + backward against ATen autograd")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    cases = [tuple(int(v) for v in c.split(",")) for c in args.case] if args.case else CASES
    if args.shares_csv:
        shares(args.shares_csv, cases[-1])
        return
    if args.shares:
        traced_shares(cases[0] if args.case else CASES[0], args.backward)
        return
    import torch

    import celebrity_image_denoiser_amd as cid
    from celebrity_image_denoiser_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("esrgan_disc_bench needs a GPU")
    dev = "cuda:0"
    rows = []
    for n, h, w in cases:
        sd = {k: torch.from_numpy(v) for k, v in synth.make_esrgan_disc_state_dict("trained", (3, h, w)).items()}
        u8 = synth.add_gaussian_noise(synth.clean_images_u8(min(n, 16), h, w), 25.0)
        x = (torch.from_numpy(u8).permute(0, 3, 1, 2).float() / 255.0).to(dev).repeat((n + 15) // 16, 1, 1, 1)[:n].contiguous()
        if args.backward:
            rows.append(backward_case(cid, torch, sd, x, args))
            continue
        disc = cid.load_esrgan_discriminator(sd, device=dev, input_shape=(3, h, w))
        table = layer_table(n, h, w)
        flops = esd_flops(n, h, w)
        row = {"N": n, "H": h, "W": w, "gflop": flops / 1e9, "workgroups": {k: v[1] for k, v in table.items()},
               "hip": summary(timed(lambda: disc(x), args.reps, args.iters), n, flops)}
        line = f"B={n:3d} {h}x{w} {flops / 1e9:.1f} GFLOP | " + fmt("hip", row["hip"])
        if not args.no_aten:
            stock = torch.nn.ModuleDict({name: torch.nn.Conv2d(cin, cout, 3, stride=2, padding=1) for name, cin, cout in CONVS})
            stock["fc"] = torch.nn.Linear(sd["fc.weight"].shape[1], 1)
            stock.load_state_dict(sd, strict=True)
            stock.to(dev)

            def aten(t=x, m=stock):
                for name, _, _ in CONVS:
                    t = torch.nn.functional.leaky_relu(m[name](t), 0.2, inplace=True)
                return m["fc"](t.view(t.size(0), -1))

            with torch.no_grad():
                row["aten"] = summary(timed(aten, args.reps, args.iters), n, flops)
                row["max_abs_diff"] = float((aten() - disc(x)).abs().max())
            line += " | " + fmt("aten", row["aten"]) + f" | hip/aten {row['hip']['ms_median'] / row['aten']['ms_median']:.2f}"
            line += f" | max|hip - aten| {row['max_abs_diff']:.1e}"
        rows.append(row)
        print(line, flush=True)
        print("    workgroups per launch: " + ", ".join(f"{k} {v[1]}" for k, v in table.items()), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
