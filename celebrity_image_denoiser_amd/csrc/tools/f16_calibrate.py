"""CPU calibration of the fp16-storage path's end-to-end error (oracle/f16_oracle.py's stand-in: the kernels' rounding points, fp32
arithmetic between them, channels summed in a shuffled order) against the fp32 ATen oracle, He-gain weights, per image:
uniform white noise in [-1, 1] at 128 x 128 (64 images by default), the benchmark's faces, and the trainer's five noise kinds on the
faces through the u8 front end.  The white-noise maximum plus a margin is the bound tests/test_f16_launches.py holds the GPU to
(include/cid.h, CID_DTYPE_F16).  Usage: python f16_calibrate.py [white-noise images]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)) + "/../../..")
from celebrity_image_denoiser_amd import synth  # noqa: E402
from oracle import f16_oracle, torch_oracle  # noqa: E402


def errs(sd, x, in_u8=False, seed=0):
    out, _ = f16_oracle.forward(sd, x, in_u8=in_u8, shuffle_seed=seed)
    xf = synth.normalize_u8(x) if in_u8 else x
    ref = torch_oracle.forward(sd, xf).double()
    return (out - ref).abs().flatten(1).max(1).values.numpy()


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = synth.make_state_dict("hot")
    g = torch.Generator().manual_seed(2024)
    e = np.concatenate([errs(sd, (torch.rand((4, 3, 128, 128), generator=g) * 2 - 1).numpy(), seed=i) for i in range(0, n, 4)])
    print(f"white noise 128x128, {len(e)} images: max {e.max():.3e}  p50 {np.median(e):.3e}  p90 {np.quantile(e, 0.9):.3e}  mean {e.mean():.3e}")
    x, _, _ = synth.make_batch(16, 128, 128, first_index=100)
    e = errs(sd, x)
    print(f"faces (benchmark batch) 128x128, 16 images: max {e.max():.3e}  p50 {np.median(e):.3e}")
    clean = synth.clean_images_u8(8, 128, 128, first_index=300)
    for kind in synth.NOISE_TYPES:
        e = errs(sd, synth.add_noise_np(clean, kind, first_index=300), in_u8=True)
        print(f"{kind:<12} on faces 128x128, 8 images (u8 in): max {e.max():.3e}  p50 {np.median(e):.3e}")


if __name__ == "__main__":
    main()
