"""Per launch x input class on the GPU: violations, exact-match fraction and worst distance (half ulps) of every launch of the
fp16-storage path against oracle/f16_oracle.check on the tensors the GPU stored; then the end-to-end white-noise error against the
fp32 ATen oracle (He-gain weights).  The numbers behind profiles/f16_launch_check.txt."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)) + "/../../..")
import celebrity_image_denoiser_amd as cid  # noqa: E402
from celebrity_image_denoiser_amd import synth  # noqa: E402
from oracle import f16_oracle as fo, torch_oracle  # noqa: E402


def run(m, x, in_u8=False):
    y = (m.forward_u8 if in_u8 else m)(*([torch.from_numpy(x).to("cuda:0")] + ([False] if in_u8 else [])))
    torch.cuda.synchronize()
    return y.cpu()


def main():
    torch.set_num_threads(16)
    g = torch.Generator().manual_seed(7)
    yy, xx = np.mgrid[0:128, 0:128]
    cb = np.stack([((yy + xx + c) % 2) * 2.0 - 1.0 for c in range(3)]).astype(np.float32)
    inputs = {"faces": (synth.make_batch(4, 128, 128, first_index=100)[0], False),
              "white": ((torch.rand((4, 3, 128, 128), generator=g) * 2 - 1).numpy(), False),
              "checker": (np.ascontiguousarray(np.broadcast_to(cb, (4, 3, 128, 128))).copy(), False),
              "white37x150": ((torch.rand((2, 3, 37, 150), generator=g) * 2 - 1).numpy(), False)}
    clean = synth.clean_images_u8(2, 128, 128, first_index=300)
    for kind in synth.NOISE_TYPES:
        inputs["u8_" + kind] = (synth.add_noise_np(clean, kind, first_index=300), True)
    for wset in ("hot", "default"):
        sd = synth.make_state_dict(wset)
        m = cid.load(sd, device="cuda:0", strict=True)
        m.compute_dtype = "f16"
        for name, (x, in_u8) in inputs.items():
            n = x.shape[0]
            h, w = (x.shape[1], x.shape[2]) if in_u8 else (x.shape[2], x.shape[3])
            m.tail_algo = "tiles"
            y = run(m, x, in_u8)
            st_t = fo.stored_tensors(m, n, h, w)
            st_t["out"] = y
            m.tail_algo = "fused"
            y = run(m, x, in_u8)
            st_f = fo.stored_tensors(m, n, h, w)
            st_f["out"] = y
            xn = fo.network_input(x, in_u8)
            rt = fo.check_launches(sd, xn, st_t, tail="tiles")
            rf = fo.check_launches(sd, xn, st_f, tail="fused", act10=st_t["upconv1.0"])
            print(f"== {wset} weights, {name} [{n},3,{h},{w}]")
            for k in fo.LAUNCHES:
                print("  tiles " + rt[k].line())
            for k in ("upconv1.0", "upconv1.2"):
                print("  fused " + rf[k].line().replace("upconv1.0     ", "upconv1.0 (z) "))
            sys.stdout.flush()
    sd = synth.make_state_dict("hot")
    m = cid.load(sd, device="cuda:0", strict=True)
    m.compute_dtype = "f16"
    g = torch.Generator().manual_seed(2024)      # the CPU calibration's images (csrc/tools/f16_calibrate.py)
    errs = []
    for i in range(0, 64, 16):
        x = (torch.rand((16, 3, 128, 128), generator=g) * 2 - 1).numpy()
        errs.append((run(m, x) - torch_oracle.forward(sd, x)).abs().flatten(1).max(1).values.numpy())
    e = np.concatenate(errs)
    print(f"== end to end, He-gain, white noise 128x128, 64 images, GPU (fused tail) vs fp32 ATen: max {e.max():.3e}  p50 {np.median(e):.3e}  "
          f"p90 {np.quantile(e, 0.9):.3e}  mean {e.mean():.3e}")


if __name__ == "__main__":
    main()
