"""Times the SRGAN discriminator forward (SRGANDiscriminator, cid_srd_forward) on the GPU with device events after a warm-up, in eval
and train mode, next to the same network run by ATen/MIOpen fp32 in the same process.

Cases: B=8 and B=16 at 256^2 (the SRGAN trainer's HR crops, sr_ganTrainGNew.py).  For each: median ms per call over --reps windows of
--iters calls [min-max], images/s, algorithmic TFLOP/s (the five 3x3 convolutions and the two 1x1 layers) and its share of the
157.3 TFLOP/s fp32 MFMA peak.  The ATen baseline is the module's own stock nn.Sequential (the same weights and BatchNorm containers)
under torch.no_grad().

Each launch's share of a forward comes from a kernel trace taken in a run of its own (tracing slows the host, so the timings above
are taken with the profiler off):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python .../srgan_disc_bench.py --case 16,256,256 --no-aten --reps 1 --iters 5
    python .../srgan_disc_bench.py --shares OUT/<host>/<pid>_kernel_stats.csv [--case 16,256,256]

--shares reads the kernel_stats CSV (no GPU needed) and prints, per kernel, its calls, average time and share of the traced time.
For model.11's launch (k_disc_conv<128, 128, 1, true, ., 256>, two channel halves that each stage the input halo) it also prints
the time next to that of k_disc_conv<64, 128, 1, ...> (model.5: half the contraction, four times the pixels, one staging): per
MFMA the two would cost the same if staging the halo twice were free.

--backward times one training call instead: forward_saved + backward (SRGANDiscriminator(autograd=True) in train mode, BCE against
ones, all 22 parameter gradients and the input gradient) next to the stock nn.Sequential under torch autograd (ATen/MIOpen fp32), in
the same process by the same method; FLOP are counted as three times the forward's.  --shares on a trace of such a run names the
backward's launches too; the two model.11 launches (the 256-channel k_disc_wgrad and k_disc_dgrad) are the ones to look at.

    python celebrity_image_denoiser_amd/csrc/tools/srgan_disc_bench.py [--reps 5] [--iters 20] [--case N,H,W ...] [--no-aten] [--backward] [--json out.json]
"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

MFMA_F32_PEAK = 157.3e12
CASES = ((8, 256, 256), (16, 256, 256))


def sides(h, w):
    h2, w2 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return h2, w2, (h2 - 1) // 2 + 1, (w2 - 1) // 2 + 1


def layer_flops(n, h, w):
    """2 * MACs of each layer of one forward, by the name of its launch."""
    h2, w2, h4, w4 = sides(h, w)
    return {"conv0": 2.0 * n * h * w * 64 * 27, "conv2": 2.0 * n * h2 * w2 * 64 * 576, "conv5": 2.0 * n * h2 * w2 * 128 * 576,
            "conv8": 2.0 * n * h4 * w4 * 128 * 1152, "conv11": 2.0 * n * h4 * w4 * 256 * 1152, "head": 2.0 * n * (256 * 512 + 512)}


def srd_flops(n, h, w):
    return sum(layer_flops(n, h, w).values())


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
    return (f"{name} {r['ms_median']:.3f} ms [{r['ms_min']:.3f}-{r['ms_max']:.3f}] {r['images_per_s']:.0f} img/s "
            f"{r['tflops']:.1f} TF/s {100 * r['mfma_share']:.0f}% of 157.3")


# kernel name prefix -> the launch it is, for --shares
LAUNCHES = (
    # the backward (--backward) first: the first match names the launch, so model.11's instantiations and the longer names lead
    ("k_disc_wgrad<128, 128, 1", "wgrad11"), ("k_disc_dgrad<256, 128, 1", "dgrad11"), ("k_disc_bn_bwd_part<256", "bn12 sums"),
    ("k_disc_wgrad<128, 128, 2", "wgrad8"), ("k_disc_dgrad<128, 128, 2", "dgrad8"), ("k_disc_wgrad<128, 64, 1", "wgrad5"),
    ("k_disc_dgrad<128, 64, 1", "dgrad5"), ("k_disc_wgrad<64, 64, 2", "wgrad2"), ("k_disc_dgrad<64, 64, 2", "dgrad2"),
    ("k_disc_wgrad0_reduce", "wgrad0 red"), ("k_disc_wgrad0", "wgrad0"), ("k_disc_dgrad0", "dgrad0"),
    ("k_disc_wgrad_reduce", "wgrad red"), ("k_disc_bn_bwd_part", "bn sums"), ("k_disc_bn_bwd_reduce", "bn reduce"),
    ("k_srd_head_bwd", "head bwd"), ("k_srd_head_reduce", "head red"), ("k_disc_pack", "pack"),
    ("k_disc_conv0", "conv0"), ("k_disc_conv<64, 64, 2", "conv2"), ("k_disc_conv<64, 128, 1", "conv5"),
    ("k_disc_conv<128, 128, 2", "conv8"), ("k_disc_conv<128, 128, 1", "conv11"), ("k_srd_head", "head"),
    ("k_disc_bn_stats", "bn stats"), ("k_disc_bn_eval", "bn eval"), ("k_disc_bn_count", "bn count"))


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
        raise SystemExit(f"{path}: no discriminator kernels in the trace")
    total = sum(r[3] for r in rows)
    flops = layer_flops(*case)
    print(f"# share of the traced discriminator kernel time ({total / 1e6:.3f} ms over all calls), case N,H,W = {case}")
    avg = {}
    for launch, name, calls, tot, mean, lo, hi in sorted(rows, key=lambda r: -r[3]):
        short = name.split("(")[0].replace("void ", "")
        line = f"{launch:10s} {short:66s} calls {calls:4d}  avg {mean / 1e3:9.1f} us  min {lo / 1e3:9.1f}  max {hi / 1e3:9.1f}  share {100 * tot / total:5.1f}%"
        if launch in flops and launch != "head":
            line += f"  MFMA share {flops[launch] / MFMA_F32_PEAK / (mean * 1e-9):.2f}" if launch != "conv0" else ""
        avg.setdefault(launch, []).append(mean)
        print(line)
    if "conv11" in avg and "conv5" in avg:
        t11, t5 = statistics.mean(avg["conv11"]), statistics.mean(avg["conv5"])
        per11, per5 = t11 / flops["conv11"], t5 / flops["conv5"]
        print(f"# conv11 (two halves, halo staged twice) {t11 / 1e3:.1f} us for {flops['conv11'] / 1e9:.1f} GFLOP; conv5 (one staging) "
              f"{t5 / 1e3:.1f} us for {flops['conv5'] / 1e9:.1f} GFLOP: time per FLOP conv11 / conv5 = {per11 / per5:.2f}")


def backward_cases(args, cases, disc, dev):
    """forward_saved + backward of one BCE loss in train mode, HIP next to ATen autograd on the same weights."""
    import copy

    import torch
    from celebrity_image_denoiser_amd import synth

    bce = torch.nn.BCELoss()
    rows = []
    for n, h, w in cases:
        u8 = synth.add_gaussian_noise(synth.clean_images_u8(min(n, 16), h, w), 25.0)
        x = torch.from_numpy(synth.normalize_u8(u8)).to(dev).repeat((n + 15) // 16, 1, 1, 1)[:n].contiguous().requires_grad_(True)
        ones = torch.ones(n, device=dev)
        flops = 3.0 * srd_flops(n, h, w)
        stock = copy.deepcopy(disc.model).train()   # its own parameters and BatchNorm buffers
        disc.train()

        def step(fwd, params):
            for q in params:
                q.grad = None
            x.grad = None
            bce(fwd(x), ones).backward()

        hip_params, aten_params = list(disc.parameters()), list(stock.parameters())
        row = {"N": n, "H": h, "W": w, "gflop": flops / 1e9,
               "train": summary(timed(lambda: step(disc, hip_params), args.reps, args.iters), n, flops)}
        if not args.no_aten:
            row["train_aten"] = summary(timed(lambda: step(lambda t: stock(t).view(-1), aten_params), args.reps, args.iters), n, flops)
        rows.append(row)
        line = f"B={n:3d} {h}x{w} forward_saved + backward, train | " + fmt("hip", row["train"])
        if "train_aten" in row:
            line += " | " + fmt("aten", row["train_aten"]) + f" | hip/aten {row['train']['ms_median'] / row['train_aten']['ms_median']:.2f}"
        print(line, flush=True)
    disc.eval()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--case", action="append", default=None, help="N,H,W (repeatable); default: the two cases above")
    ap.add_argument("--no-aten", action="store_true", help="skip the ATen/MIOpen baseline")
    ap.add_argument("--backward", action="store_true", help="time forward_saved + backward in train mode against ATen autograd")
    ap.add_argument("--shares", default=None, help="a rocprofv3 kernel_stats CSV of a traced run: print each launch's share and exit")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    cases = [tuple(int(v) for v in c.split(",")) for c in args.case] if args.case else CASES
    if args.shares:
        shares(args.shares, cases[-1])
        return
    import torch

    import celebrity_image_denoiser_amd as cid
    from celebrity_image_denoiser_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("srgan_disc_bench needs a GPU")
    dev = "cuda:0"
    sd = {k: torch.from_numpy(v) for k, v in synth.make_srgan_disc_state_dict("trained").items()}
    disc = cid.load_srgan_discriminator(sd, device=dev, strict=True, autograd=args.backward)
    rows = []
    if args.backward:
        backward_cases(args, cases, disc, dev)
        return
    for n, h, w in cases:
        u8 = synth.add_gaussian_noise(synth.clean_images_u8(min(n, 16), h, w), 25.0)
        x = torch.from_numpy(synth.normalize_u8(u8)).to(dev).repeat((n + 15) // 16, 1, 1, 1)[:n].contiguous()
        flops = srd_flops(n, h, w)
        row = {"N": n, "H": h, "W": w, "gflop": flops / 1e9}
        for mode in ("eval", "train"):
            disc.train(mode == "train")
            row[mode] = summary(timed(lambda: disc(x), args.reps, args.iters), n, flops)
            if not args.no_aten:
                with torch.no_grad():
                    row[mode + "_aten"] = summary(timed(lambda: disc.model(x).view(-1), args.reps, args.iters), n, flops)
        disc.eval()
        rows.append(row)
        for mode in ("eval", "train"):
            line = f"B={n:3d} {h}x{w} {flops / 1e9:.0f} GFLOP {mode:5s} | " + fmt("hip", row[mode])
            if mode + "_aten" in row:
                line += " | " + fmt("aten", row[mode + "_aten"]) + f" | hip/aten {row[mode]['ms_median'] / row[mode + '_aten']['ms_median']:.2f}"
            print(line, flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
