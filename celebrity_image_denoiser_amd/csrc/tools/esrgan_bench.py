"""Times the ESRGAN forward (ESRGANGenerator, cid_esr_forward) on the GPU with device events after a warm-up, next to the same network
restated with the module's own stock nn containers on ATen/MIOpen fp32 in the same process.

Cases: B=16 256^2 and B=256 128^2.  For each: median ms per call over --reps windows of --iters calls [min-max], images/s, algorithmic
TFLOP/s (2 * MACs of the 9x9 head, the 2 R trunk convolutions and the 9x9 tail: 1.242 MFLOP per pixel at R = 8) and its share of the
157.3 TFLOP/s fp32 MFMA peak.  --residuals 0 times head + tail alone; the trunk's time per launch is the difference to R = 8 over 16.

--train times the TRAIN-mode forward (ESRGANGenerator(batch_stats=True), cid_esr_forward_train) at the ESRGAN trainer's shape, B=8
256x256, and at B=16, next to this build's own eval forward and to a stock copy of the network in train mode on ATen/MIOpen (under
no_grad, as this forward has no autograd history either).  The three run in one process and take turns window by window: 3 warm-up
calls each, then the median of 5 windows of 20 calls [min-max], "default" weights, inputs resident.

--backward times the differentiable step (ESRGANGenerator(batch_stats=True, autograd=True): cid_esr_pack_weights_device +
cid_esr_forward_saved, then cid_esr_backward under loss.backward()) at the trainer's shape, B=8 256x256, R=8, next to the forward of
that step alone and to loss.backward() through a stock copy of the network on ATen/MIOpen autograd, in the same protocol: one process,
windows in turn, 3 warm-up steps each, the median of 5 windows of 5 steps [min-max].  A step is out = G(x); (out * g).sum().backward()
with .grad set to None before it.  It also prints what one call holds: the saved buffer is (3R+1) tensors of N*64*H*W*4 bytes plus
the BatchNorm tables, 3.36 GB at that shape, next to the train workspace and the backward workspace.

    python celebrity_image_denoiser_amd/csrc/tools/esrgan_bench.py [--reps 5] [--iters 10] [--case N,H,W ...] [--residuals 8]
                                                                   [--no-aten] [--u8] [--json out.json] [--train | --backward]
"""
import argparse
import copy
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
TRAIN_CASES = ((8, 256, 256), (16, 256, 256))


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


def timed_in_turn(fns, reps, iters, warmup=3):
    """timed() of several callables whose windows alternate: clocks and cache state of one window reach every contender alike."""
    for fn in fns:
        for _ in range(warmup):
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


def run_train_case(n, h, w, r, args):
    """One train forward: HIP, this build's eval forward, and the stock layers in train mode on ATen/MIOpen."""
    dev = "cuda:0"
    sd = synth.make_esrgan_state_dict("default", r)
    train = cid.load_esrgan(sd, num_residuals=r, device=dev, strict=True, batch_stats=True).train()
    evalm = cid.load_esrgan(sd, num_residuals=r, device=dev, strict=True)   # its own module: its fold never goes stale
    # the stock layers of the module, copied (their BatchNorm buffers move) and run as the reference's forward does
    stock = copy.deepcopy(torch.nn.ModuleDict({k: getattr(train, k) for k in ("initial", "residuals", "final")})).train()
    u8 = torch.from_numpy(synth.esrgan_inputs_u8(min(n, 16), h, w)).to(dev).repeat((n + 15) // 16, 1, 1, 1)[:n].contiguous()
    x = u8.to(torch.float32).div(255.0).permute(0, 3, 1, 2).contiguous()

    def stock_forward():
        with torch.no_grad():
            return aten_forward(stock, x)

    fns = [lambda: train(x), lambda: evalm(x)] + ([] if args.no_aten else [stock_forward])
    times = timed_in_turn(fns, args.reps, args.iters)
    flops = esr_flops(n, h, w, r)
    row = {"N": n, "H": h, "W": w, "R": r, "gflop": flops / 1e9, "mode": "train"}
    row["hip_train"], row["hip_eval"] = summary(times[0], n, flops), summary(times[1], n, flops)
    line = f"train B={n:3d} {h}x{w} R={r} | " + fmt("hip train", row["hip_train"]) + " | " + fmt("hip eval", row["hip_eval"])
    line += f" | train/eval {row['hip_train']['ms_median'] / row['hip_eval']['ms_median']:.2f}"
    if not args.no_aten:
        row["aten_train"] = summary(times[2], n, flops)
        line += " | " + fmt("aten train", row["aten_train"]) + f" | hip/aten {row['hip_train']['ms_median'] / row['aten_train']['ms_median']:.2f}"
    print(line, flush=True)
    return row


def run_backward_case(n, h, w, r, args):
    """One generator step: HIP forward with history, HIP forward + backward, and the stock layers under ATen autograd."""
    import ctypes

    from celebrity_image_denoiser_amd import _lib

    dev = "cuda:0"
    sd = synth.make_esrgan_state_dict("default", r)
    model = cid.load_esrgan(sd, num_residuals=r, device=dev, strict=True, batch_stats=True, autograd=True).train()
    stock = copy.deepcopy(torch.nn.ModuleDict({k: getattr(model, k) for k in ("initial", "residuals", "final")})).train()
    u8 = torch.from_numpy(synth.esrgan_inputs_u8(min(n, 16), h, w)).to(dev).repeat((n + 15) // 16, 1, 1, 1)[:n].contiguous()
    x = u8.to(torch.float32).div(255.0).permute(0, 3, 1, 2).contiguous()
    g = torch.rand((n, 3, h, w), device=dev, generator=torch.Generator(dev).manual_seed(7)).mul_(2).sub_(1).div_(n * 3 * h * w)

    def hip_forward():
        model(x)    # with grad enabled: pack on the device + cid_esr_forward_saved; the context is dropped with the result

    def hip_step():
        model.zero_grad(set_to_none=True)
        (model(x) * g).sum().backward()

    def aten_step():
        stock.zero_grad(set_to_none=True)
        (aten_forward(stock, x) * g).sum().backward()

    fns = [hip_forward, hip_step] + ([] if args.no_aten else [aten_step])
    times = timed_in_turn(fns, args.reps, args.iters)
    flops = 3.0 * esr_flops(n, h, w, r)   # forward + data gradient + weight gradient, the input gradient of the head aside
    row = {"N": n, "H": h, "W": w, "R": r, "mode": "backward", "gflop_step": flops / 1e9}
    need = ctypes.c_size_t()
    for key, fn in (("saved_bytes", "cid_esr_saved_bytes"), ("backward_workspace_bytes", "cid_esr_backward_workspace_bytes"),
                    ("train_workspace_bytes", "cid_esr_train_workspace_bytes")):
        assert getattr(_lib.lib(), fn)(n, h, w, r, ctypes.byref(need)) == 0
        row[key] = need.value
    row["hip_forward_saved"], row["hip_step"] = summary(times[0], n, flops / 3), summary(times[1], n, flops)
    line = (f"backward B={n:3d} {h}x{w} R={r} | saved {row['saved_bytes'] / 1e9:.2f} GB, backward workspace "
            f"{row['backward_workspace_bytes'] / 1e9:.2f} GB, train workspace {row['train_workspace_bytes'] / 1e9:.2f} GB\n  "
            + fmt("hip forward_saved", row["hip_forward_saved"]) + "\n  " + fmt("hip forward+backward", row["hip_step"]))
    if not args.no_aten:
        row["aten_step"] = summary(times[2], n, flops)
        line += "\n  " + fmt("aten forward+backward", row["aten_step"]) + f"\n  hip/aten {row['hip_step']['ms_median'] / row['aten_step']['ms_median']:.2f}"
    print(line, flush=True)
    return row


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
    ap.add_argument("--train", action="store_true", help="the train-mode forward at the trainer's shapes (B=8 and B=16, 256x256)")
    ap.add_argument("--backward", action="store_true", help="forward + backward of the generator step at the trainer's shape (B=8, 256x256)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("esrgan_bench needs a GPU")
    dev = "cuda:0"
    cases = [tuple(int(v) for v in c.split(",")) for c in args.case] if args.case else CASES
    r = args.residuals
    if args.backward:
        args.iters = 5 if args.iters == ap.get_default("iters") else args.iters
        rows = [run_backward_case(n, h, w, r, args) for n, h, w in (cases if args.case else TRAIN_CASES[:1])]
        if args.json:
            with open(args.json, "w") as f:
                json.dump(rows, f, indent=1)
        return
    if args.train:
        args.iters = 20 if args.iters == ap.get_default("iters") else args.iters
        rows = [run_train_case(n, h, w, r, args) for n, h, w in (cases if args.case else TRAIN_CASES)]
        if args.json:
            with open(args.json, "w") as f:
                json.dump(rows, f, indent=1)
        return
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
