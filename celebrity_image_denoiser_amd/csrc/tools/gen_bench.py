"""Times the generator's training step pieces on the GPU with device events after a warm-up:

    forward            cid_forward (DenoiseGenerator(), fused last layer)
    forward + backward DenoiseGenerator(autograd=True): cid_forward_saved + cid_backward, all 24 parameter gradients and the input gradient
    aten               the same network on the module's own stock nn layers through torch autograd (ATen/MIOpen fp32), same process
    repack             pack_weights() of a forward-only module after an in-place change of every parameter: the host path (24
                       device-to-host copies, the host repack, one upload)
    repack_device      the same on DenoiseGenerator(autograd=True): cid_pack_weights_device, one kernel that writes the whole blob
                       (what an optimizer step costs the trainer's next forward), with the blob's bytes against the 8 TB/s of HBM
    touch              the in-place change alone (24 elementwise launches), which both repack rows contain
    pack kernel        k_gen_pack by itself: forced packs queued behind a few forwards, so that the host has enqueued them all before
                       the first one starts and the events around them see the kernels back to back; the blob's bytes over that time
                       against the 8 TB/s of HBM
    adam               stock torch.optim.Adam(G.parameters(), lr=1e-4).step() on the 24 parameters
    adam_device        cid.Adam(G.parameters(), lr=1e-4).step(): one cid_adam_step launch; the same process and the same 24 gradients
    adam kernel        k_adam_step by itself, queued back to back behind a few forwards as `pack kernel` is: 28 bytes per element (four
                       loads, three stores) over that time against the 8 TB/s of HBM

Cases: B=16 256^2 (the trainer's batch, training.py:504-505) and B=64 128^2.  For each: median ms per call over --reps windows of
--iters calls [min-max], images/s, algorithmic TFLOP/s and its share of the 157.3 TFLOP/s fp32 MFMA peak; the forward + backward rows
count 3x the forward's algorithmic FLOPs (forward, data gradient, weight gradient).

    python celebrity_image_denoiser_amd/csrc/tools/gen_bench.py [--reps 5] [--iters 20] [--case N,H,W ...] [--no-aten] [--json out.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import celebrity_image_denoiser_amd as cid  # noqa: E402
from celebrity_image_denoiser_amd import _lib, synth  # noqa: E402
from celebrity_image_denoiser_amd.generator import launch_table  # noqa: E402

MFMA_F32_PEAK = 157.3e12
HBM_PEAK = 8.0e12
CASES = ((16, 256, 256), (64, 128, 128))


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


def stock_forward(m, x):
    """The reference forward (app.py:80-103) on the module's stock nn layers: ATen/MIOpen."""
    e1 = m.down1(x)
    e2 = m.down2(m.pool1(e1))
    b = m.bottleneck(m.pool2(e2))
    d2 = m.upconv2(torch.cat([m.up2(b), e2], 1))
    return torch.tanh(m.upconv1(torch.cat([m.up1(d2), e1], 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--case", action="append", default=None, help="N,H,W (repeatable); default: the two cases above")
    ap.add_argument("--no-aten", action="store_true", help="skip the ATen/MIOpen baseline")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gen_bench needs a GPU")
    dev = "cuda:0"
    cases = [tuple(int(v) for v in c.split(",")) for c in args.case] if args.case else CASES
    sd = synth.make_state_dict("default")
    gen = cid.load(sd, device=dev, strict=True)
    gen_ag = cid.load(sd, device=dev, strict=True, autograd=True)
    rows = []
    for n, h, w in cases:
        u8 = synth.add_gaussian_noise(synth.clean_images_u8(16, h, w), 25.0)
        x = torch.from_numpy(synth.normalize_u8(u8)).to(dev).repeat((n + 15) // 16, 1, 1, 1)[:n].contiguous()
        flops = sum(r[2] for r in launch_table(n, h, w))
        row = {"N": n, "H": h, "W": w, "gflop": flops / 1e9}
        y = torch.empty_like(x)
        row["forward"] = summary(timed(lambda: gen(x, out=y), args.reps, args.iters), n, flops)
        go = torch.randn(x.shape, device=dev, generator=torch.Generator(dev).manual_seed(1)) / x.numel()
        xg = x.clone().requires_grad_(True)

        def step(fwd, params):
            for q in params:
                q.grad = None
            xg.grad = None
            fwd(xg).backward(go)

        row["fwd_bwd"] = summary(timed(lambda: step(gen_ag, list(gen_ag.parameters())), args.reps, args.iters), n, 3 * flops)
        if not args.no_aten:
            with torch.no_grad():
                row["forward_aten"] = summary(timed(lambda: stock_forward(gen, x), args.reps, args.iters), n, flops)
            row["fwd_bwd_aten"] = summary(timed(lambda: step(lambda t: stock_forward(gen, t), list(gen.parameters())), args.reps, args.iters),
                                          n, 3 * flops)
        rows.append(row)
        for key, label, f in (("forward", "forward", flops), ("fwd_bwd", "forward_saved + backward", 3 * flops)):
            line = f"B={n:3d} {h}x{w} {f / 1e9:.0f} GFLOP {label} | " + fmt("hip", row[key])
            if key + "_aten" in row:
                line += " | " + fmt("aten", row[key + "_aten"]) + f" | hip/aten {row[key]['ms_median'] / row[key + '_aten']['ms_median']:.2f}"
            print(line, flush=True)

    # the repack after an optimizer step: every parameter changed in place, then pack_weights()
    def repack(m, pack=True):
        with torch.no_grad():
            for q in m.parameters():
                q.mul_(1.0)
        if pack:
            m.pack_weights()

    blob_bytes = gen.pack_weights().numel()
    it = max(1, args.iters // 4)
    t = timed(lambda: repack(gen), args.reps, it)
    td = timed(lambda: repack(gen_ag), args.reps, it)
    t0 = timed(lambda: repack(gen_ag, pack=False), args.reps, it)
    med, medd, med0 = statistics.median(t), statistics.median(td), statistics.median(t0)

    def pack_kernel(n=20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(8):          # ~20 ms of queued work: the host is done enqueuing long before the packs start
            gen(x, out=y)
        e0.record()
        for _ in range(n):
            gen_ag.pack_weights(force=True)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    tk = [pack_kernel() for _ in range(args.reps)]
    medk = statistics.median(tk)
    rows.append({"repack_ms_median": med, "repack_ms_min": min(t), "repack_ms_max": max(t),
                 "repack_device_ms_median": medd, "repack_device_ms_min": min(td), "repack_device_ms_max": max(td),
                 "touch_ms_median": med0, "touch_ms_min": min(t0), "touch_ms_max": max(t0),
                 "pack_kernel_ms_median": medk, "pack_kernel_ms_min": min(tk), "pack_kernel_ms_max": max(tk),
                 "blob_bytes": blob_bytes, "device_over_host": medd / med, "pack_kernel_hbm_share": blob_bytes / (medk * 1e-3) / HBM_PEAK})
    print(f"repack after an optimizer step (pack_weights, host path, autograd=False): {med:.3f} ms [{min(t):.3f}-{max(t):.3f}]", flush=True)
    print(f"repack_device (pack_weights, device path, autograd=True): {medd:.4f} ms [{min(td):.4f}-{max(td):.4f}] = {medd / med:.5f} of the host path", flush=True)
    print(f"touch (the in-place change of the 24 parameters alone): {med0:.4f} ms [{min(t0):.4f}-{max(t0):.4f}]", flush=True)
    print(f"pack kernel (k_gen_pack back to back): {medk:.4f} ms [{min(tk):.4f}-{max(tk):.4f}] for the {blob_bytes / 1e6:.1f} MB blob: "
          f"{blob_bytes / (medk * 1e-3) / 1e12:.2f} TB/s written, {blob_bytes / (medk * 1e-3) / HBM_PEAK:.3f} of 8 TB/s", flush=True)
    adam_rows(args, gen, gen_ag, x, y, rows)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


def adam_rows(args, gen, gen_ag, x, y, rows):
    """The optimizer step: stock torch.optim.Adam on `gen`'s parameters, cid.Adam on `gen_ag`'s, both reading the same 24 gradients."""
    dev = x.device
    rng = torch.Generator(dev).manual_seed(2)
    grads = [torch.randn(p.shape, device=dev, generator=rng) * 1e-3 for p in gen.parameters()]
    for m in (gen, gen_ag):
        for p, g in zip(m.parameters(), grads):
            p.grad = g
    stock = torch.optim.Adam(gen.parameters(), lr=1e-4)
    device = cid.Adam(gen_ag.parameters(), lr=1e-4)
    ts = timed(stock.step, args.reps, args.iters)
    td = timed(device.step, args.reps, args.iters)
    # the kernel alone through the C ABI with a fixed table, behind ~20 ms of queued work so that the host is ahead of the device
    params = list(gen_ag.parameters())
    table = (_lib.AdamTensor * len(params))()
    for e, p, g in zip(table, params, grads):
        st = device.state[p]
        e.param, e.grad, e.exp_avg, e.exp_avg_sq = p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
        e.count, e.step = p.numel(), 1000
    hp = _lib.AdamHyper(1e-4, 0.9, 0.999, 1e-8, 0.0)
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def adam_kernel(n=args.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(8):
            gen(x, out=y)
        e0.record()
        for _ in range(n):
            if L.cid_adam_step(table, len(params), ctypes.byref(hp), stream) != 0:
                raise SystemExit("cid_adam_step failed")
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    adam_kernel()
    tk = [adam_kernel() for _ in range(args.reps)]
    meds, medd, medk = statistics.median(ts), statistics.median(td), statistics.median(tk)
    nbytes = 28 * sum(p.numel() for p in params)
    rows.append({"adam_ms_median": meds, "adam_ms_min": min(ts), "adam_ms_max": max(ts),
                 "adam_device_ms_median": medd, "adam_device_ms_min": min(td), "adam_device_ms_max": max(td),
                 "adam_kernel_ms_median": medk, "adam_kernel_ms_min": min(tk), "adam_kernel_ms_max": max(tk),
                 "adam_bytes": nbytes, "adam_device_over_stock": medd / meds, "adam_kernel_hbm_share": nbytes / (medk * 1e-3) / HBM_PEAK})
    print(f"adam (torch.optim.Adam(G.parameters(), lr=1e-4).step(), 24 tensors): {meds:.4f} ms [{min(ts):.4f}-{max(ts):.4f}]", flush=True)
    print(f"adam_device (cid.Adam(G.parameters(), lr=1e-4).step(), one launch): {medd:.4f} ms [{min(td):.4f}-{max(td):.4f}] = "
          f"{medd / meds:.3f} of the stock step", flush=True)
    print(f"adam kernel (k_adam_step back to back): {medk:.4f} ms [{min(tk):.4f}-{max(tk):.4f}] for {nbytes / 1e6:.1f} MB moved: "
          f"{nbytes / (medk * 1e-3) / 1e12:.2f} TB/s, {nbytes / (medk * 1e-3) / HBM_PEAK:.3f} of 8 TB/s", flush=True)


if __name__ == "__main__":
    main()
