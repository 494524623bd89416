"""Times resize.resize() (cid_resize) on the GPU next to Pillow's Image.resize(BICUBIC) in a 16-thread pool, in the same run.

Cases: 1024x1024 -> 256x256 and 218x178 (CelebA) -> 256x256, at N = 64 and N = 256.  Per case:
  kernel    median ms per cid_resize call (device events around --iters calls, --reps windows, after a warm-up) and the achieved
            GB/s against the source bytes read (N*Hs*Ws*3; the kernel's compulsory traffic is that plus the N*Hd*Wd*3 written)
  device    images/s of upload + resize + synchronise, from a pageable and from a pinned host batch (wall clock, median of --reps)
  pillow    images/s and ms per image per thread of Image.resize in a ThreadPoolExecutor(16) over the same N images (wall clock)
The acceptance line compares the device path (upload included, pageable) with the Pillow pool at 1024x1024 -> 256x256, N = 64.

    python celebrity_image_denoiser_amd/csrc/tools/resize_bench.py [--reps 5] [--iters 20] [--out profiles/resize_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from celebrity_image_denoiser_amd import resize as rz  # noqa: E402

CASES = ((1024, 1024, 256, 256), (218, 178, 256, 256))
BATCHES = (64, 256)
POOL = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resize_bench needs a GPU")
    from PIL import Image
    import PIL

    dev = "cuda:0"
    lines = [f"resize_bench: {torch.cuda.get_device_name(0)}, Pillow {PIL.__version__}, pool of {POOL} threads, "
             f"reps {args.reps}, iters {args.iters}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    accept = None
    for hs, ws, hd, wd in CASES:
        base = np.random.default_rng(hs).integers(0, 256, (16, hs, ws, 3), dtype=np.uint8)
        for n in BATCHES:
            host = np.ascontiguousarray(np.tile(base, ((n + 15) // 16, 1, 1, 1))[:n])
            pinned = torch.from_numpy(host).pin_memory()
            xd = torch.from_numpy(host).to(dev)
            for _ in range(3):
                rz.resize(xd, (wd, hd))
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    rz.resize(xd, (wd, hd))
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / args.iters)
            med = statistics.median(ms)
            src_bytes = host.nbytes

            def device_path(src):
                t = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    rz.resize(src.to(dev, non_blocking=True), (wd, hd))
                    torch.cuda.synchronize()
                    t.append(time.perf_counter() - t0)
                return n / statistics.median(t)

            ips_pageable, ips_pinned = device_path(torch.from_numpy(host)), device_path(pinned)
            imgs = [Image.fromarray(host[k]) for k in range(n)]
            with ThreadPoolExecutor(POOL) as pool:
                list(pool.map(lambda im: im.resize((wd, hd), resample=Image.Resampling.BICUBIC), imgs[:POOL]))   # warm the pool
                t0 = time.perf_counter()
                list(pool.map(lambda im: im.resize((wd, hd), resample=Image.Resampling.BICUBIC), imgs))
                pil_s = time.perf_counter() - t0
            ips_pil = n / pil_s
            say(f"{hs}x{ws} -> {hd}x{wd} N={n}: kernel {med:.4f} ms [{min(ms):.4f}-{max(ms):.4f}] = {n / med * 1e3:.0f} img/s, "
                f"{src_bytes / med / 1e6:.0f} GB/s of source read | device path with upload {ips_pageable:.0f} img/s pageable, "
                f"{ips_pinned:.0f} img/s pinned | Pillow x{POOL} {ips_pil:.0f} img/s ({pil_s / n * POOL * 1e3:.2f} ms per image per thread)")
            if (hs, ws, n) == (1024, 1024, 64):
                accept = (ips_pageable, ips_pil)
            del xd, pinned
    if accept:
        say(f"acceptance (1024x1024 -> 256x256, N=64, upload counted): device {accept[0]:.0f} img/s vs Pillow x{POOL} {accept[1]:.0f} img/s: "
            f"{'PASS' if accept[0] > accept[1] else 'FAIL'} ({accept[0] / accept[1]:.1f}x)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
