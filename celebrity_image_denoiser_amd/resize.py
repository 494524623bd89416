"""PIL's bicubic resize on device uint8 batches, bit for bit.

Every reference entry point starts with Image.resize(image_size, resample=BICUBIC) (noise_generation.py:61, denoisegan_eval.py,
denoise_eavl_iter.py:89, training.py:303-304).  Pillow's 8-bit resampler is integer arithmetic (22-bit fixed-point coefficients, a
uint8 intermediate between the horizontal and the vertical pass), so a HIP kernel (cid_resize, include/cid.h) equals it exactly;
synth.resize_bicubic_np is the bit-defined CPU restatement.  There is no CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import ctypes
import sys
import types

_FMT = {"f32": 0, "u8": 1}   # CID_FMT_F32_NCHW, CID_FMT_U8_NHWC


class _PlanCache(dict):
    """cid_resize_plan_t per (device index, Hs, Ws, Hd, Wd); the plans are destroyed with the cache."""

    def clear(self):
        from . import _lib

        for plan in self.values():
            _lib.lib().cid_resize_plan_destroy(plan)
        super().clear()

    def __del__(self):
        try:
            self.clear()
        except Exception:   # noqa: BLE001 - interpreter shutdown: the library may be gone already
            pass


_plans = _PlanCache()


def _plan(device, hs: int, ws: int, hd: int, wd: int):
    import torch

    from . import _lib

    key = (device.index if device.index is not None else torch.cuda.current_device(), hs, ws, hd, wd)
    plan = _plans.get(key)
    if plan is None:
        p = ctypes.c_void_p()
        with torch.cuda.device(key[0]):
            rc = _lib.lib().cid_resize_plan_create(ctypes.byref(p), hs, ws, hd, wd, _lib.CID_RESAMPLE_BICUBIC)
        if rc == 2:   # CID_ERR_SHAPE
            raise ValueError(f"resize {hs}x{ws} -> {hd}x{wd} not accepted: sides 1..16384, downscale factor at most 64 per axis")
        _lib.check(None, rc)
        plan = _plans[key] = p
    return plan


def resize(src_u8, size, out: str = "u8"):
    """uint8 [N,H,W,3] on the GPU -> the batch resized to size = (width, height) (PIL's order, as the reference passes it) by one
    HIP kernel on torch's current stream: uint8 [N,height,width,3] (out="u8") or the normalised fp32 [N,3,height,width]
    (out="f32": (u8/255 - 0.5)/0.5, what the forward makes of the uint8 result).  Equals
    synth.resize_bicubic_np(src_u8.cpu().numpy(), size), i.e. PIL's Image.resize(size, resample=BICUBIC) of every image, byte for
    byte.  Downscale factors up to 64 per axis.  The plan of a (device, source size, size) is built on first use and cached."""
    import torch

    from . import _lib

    if out not in _FMT:
        raise ValueError(f"out must be 'u8' or 'f32', got {out!r}")
    if not isinstance(src_u8, torch.Tensor) or src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3:
        raise RuntimeError("resize expects a uint8 tensor of shape [N,H,W,3]")
    if not src_u8.is_cuda:
        raise RuntimeError("got a CPU tensor: the resize is GPU-only; there is no CPU fallback (synth.resize_bicubic_np is the "
                           "CPU restatement used by the tests)")
    if not src_u8.is_contiguous():
        raise RuntimeError("resize expects a contiguous tensor")
    n, hs, ws, _ = src_u8.shape
    wd, hd = int(size[0]), int(size[1])
    if n < 1:
        raise ValueError("resize expects at least one image")
    plan = _plan(src_u8.device, hs, ws, hd, wd)
    if out == "u8":
        dst = torch.empty((n, hd, wd, 3), dtype=torch.uint8, device=src_u8.device)
    else:
        dst = torch.empty((n, 3, hd, wd), dtype=torch.float32, device=src_u8.device)
    with torch.cuda.device(src_u8.device):
        stream = torch.cuda.current_stream(src_u8.device).cuda_stream
        rc = _lib.lib().cid_resize(plan, src_u8.data_ptr(), dst.data_ptr(), _FMT[out], n, stream)
    _lib.check(None, rc)
    return dst


def resize_images(images, size, device="cuda:0"):
    """A ragged list of uint8 [H,W,3] images (numpy arrays or tensors) -> uint8 [len(images),height,width,3] on `device`, in list
    order: the images are grouped by source size, each group is uploaded as one batch and resized by one launch, and the results
    are scattered back into list order."""
    import numpy as np
    import torch

    wd, hd = int(size[0]), int(size[1])
    dev = torch.device(device)
    groups = {}
    for i, im in enumerate(images):
        t = im if isinstance(im, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(im))
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise RuntimeError(f"image {i}: expected uint8 [H,W,3], got {t.dtype} {list(t.shape)}")
        groups.setdefault((t.shape[0], t.shape[1]), []).append((i, t))
    out = torch.empty((len(images), hd, wd, 3), dtype=torch.uint8, device=dev)
    for members in groups.values():
        batch = torch.stack([t for _, t in members]).to(dev).contiguous()
        index = torch.tensor([i for i, _ in members], dtype=torch.int64).to(dev)
        out.index_copy_(0, index, resize(batch, (wd, hd)))
    return out


class _CallableModule(types.ModuleType):
    """Importing this submodule binds the package attribute `resize` to the module, which would shadow the package's lazy export of
    the function of the same name; calling the module is calling the function, so `cid.resize(x, size)` works either way."""

    def __call__(self, *args, **kwargs):
        return resize(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule
