"""What the modules over a cid_<abi>_* weight-store handle share (ESRGANGenerator, SRGANGenerator, CGANGenerator, LPIPS,
VGGPerceptualLoss, DenoiseDiscriminator, SRGANDiscriminator, ESRGANDiscriminator): the handle, the packed blob, the grow-only workspace and the decode of a stored stage.

A subclass sets `_abi`, builds its layers, calls `_create(...)`, and keeps its forward and its shape errors.  Where it differs it
overrides `_batchnorms()` (BatchNorm layers whose eps the library needs), `_key()` (state_dict key -> library key) and `_tensors()`
(which tensors are sent).
"""
from __future__ import annotations

import ctypes
import numpy as np
import torch
import torch.nn as nn

from . import _lib


def cuda_device(device, who: str) -> torch.device:
    """`device`, or the current GPU when it is None; anything but a GPU raises for the public function `who`."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if device is None or torch.device(device).type != "cuda":
        raise RuntimeError(f"celebrity_image_denoiser_amd.{who}: an AMD GPU is required (no CPU fallback)")
    return torch.device(device)


def image_operand(x):
    """(CID format, (N, H, W)) of an fp32 [N,3,H,W] or uint8 [N,H,W,3] tensor; None for anything else."""
    if isinstance(x, torch.Tensor) and x.dim() == 4:
        if x.dtype == torch.float32 and x.shape[1] == 3:
            return _lib.CID_FMT_F32_NCHW, (x.shape[0], x.shape[2], x.shape[3])
        if x.dtype == torch.uint8 and x.shape[3] == 3:
            return _lib.CID_FMT_U8_NHWC, (x.shape[0], x.shape[1], x.shape[2])
    return None


def image_output(out_dtype, n: int, h: int, w: int, device):
    """(CID format, the empty output tensor): uint8 [n,h,w,3] or float32 [n,3,h,w]."""
    if out_dtype == torch.uint8:
        return _lib.CID_FMT_U8_NHWC, torch.empty((n, h, w, 3), dtype=torch.uint8, device=device)
    if out_dtype == torch.float32:
        return _lib.CID_FMT_F32_NCHW, torch.empty((n, 3, h, w), dtype=torch.float32, device=device)
    raise RuntimeError(f"out_dtype must be torch.float32 or torch.uint8, got {out_dtype}")


def load_into(model, source, device, strict: bool, key_candidates=None):
    """The body of load_esrgan / load_srgan / load_cgan and of the BatchNorm discriminators' loaders: `source` (a checkpoint path, a
    checkpoint dict, a state_dict or None) into `model`, the model to `device` in eval mode, weights packed.  `key_candidates`: where
    the state_dict sits in a checkpoint dict, where that is not the generators' default (api.extract_state_dict)."""
    from .api import _read_checkpoint_file, extract_state_dict

    where = () if key_candidates is None else (key_candidates,)
    if isinstance(source, str):
        model.load_state_dict(_read_checkpoint_file(source, *where), strict=strict)
    elif source is not None:
        sd = {k: (v if isinstance(v, torch.Tensor) else torch.as_tensor(v)) for k, v in extract_state_dict(source, *where).items()}
        model.load_state_dict(sd, strict=strict)
    model.to(device).eval()
    model.pack_weights()
    return model


class PackedModule(nn.Module):
    _abi = ""     # the C ABI family: "esr", "sr", "cg", "lpips", "vgg", "disc", "srd" or "esd"
    _form = ()    # the leading `what` argument of cid_vgg_workspace_bytes / cid_vgg_stage_view; the other families have none

    def _create(self, *args) -> None:
        """cid_<abi>_create(&handle, *args); call it last in __init__."""
        self._cid = ctypes.c_void_p()
        self._check(self._fn("create")(ctypes.byref(self._cid), *args), handle=False)
        self._blob = None          # packed weights on the device (uint8 tensor, owns the memory)
        self._packed_sig = None
        self._ws = None            # workspace (uint8 tensor, grow-only)

    def __del__(self):
        try:
            if getattr(self, "_cid", None):
                self._fn("destroy")(self._cid)
                self._cid = None
        except Exception:
            pass

    def _fn(self, name: str):
        return getattr(_lib.lib(), f"cid_{self._abi}_{name}")

    def _check(self, rc: int, handle: bool = True) -> None:
        _lib.check_abi(self._abi, self._cid if handle else None, rc)

    # ------------------------------------------------------------------ weights
    def _device(self) -> torch.device:
        return next(self.parameters()).device

    def _tensors(self):
        """The (key, tensor) pairs the library gets."""
        return list(self.state_dict(keep_vars=True).items())

    def _key(self, key: str) -> str:
        """The library's name of state_dict key `key`."""
        return key

    def _batchnorms(self):
        """(name, BatchNorm2d, its leading arguments of cid_<abi>_set_bn_eps) of every BatchNorm the pack folds."""
        return ()

    def _blob_bytes(self) -> int:
        """Size of the packed blob (a family whose layout does not depend on the handle takes no argument and overrides this)."""
        return self._fn("packed_weights_bytes")(self._cid)

    def _signature(self):
        eps = tuple(float(bn.eps) for _, bn, _ in self._batchnorms())
        return tuple((k, t.data_ptr(), t._version, str(t.device)) for k, t in self._tensors()) + eps

    def pack_weights(self, force: bool = False) -> torch.Tensor:
        """Pack the state_dict into the kernels' layout on the module's GPU, BatchNorm (where the model has any) folded (if anything
        changed since the last call)."""
        sig = self._signature()
        if not force and self._blob is not None and sig == self._packed_sig:
            return self._blob
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs only on an AMD GPU (HIP kernels behind libcid.so); move it with "
                               ".to('cuda') first. There is no CPU fallback.")
        for name, bn, where in self._batchnorms():
            if not (bn.affine and bn.track_running_stats):
                raise NotImplementedError(f"{name}: only BatchNorm2d(affine=True, track_running_stats=True)")
            self._check(self._fn("set_bn_eps")(self._cid, *where, float(bn.eps)))
        for key, t in self._tensors():
            if key.endswith("num_batches_tracked"):
                a = t.detach().cpu().numpy()   # 0-d int64: accepted and ignored by the library
            else:
                a = np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())
            shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
            self._check(self._fn("set_weight")(self._cid, self._key(key).encode(), a.ctypes.data, shape, a.ndim))
        blob = torch.empty(self._blob_bytes(), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self._check(self._fn("upload_weights")(self._cid, blob.data_ptr(), stream))
        self._blob, self._packed_sig = blob, sig
        return blob

    # ------------------------------------------------------------------ forward
    def _image_input(self, x):
        """(CID format, (N, H, W)) of the image batch a generator's forward got; its TypeError / RuntimeError otherwise."""
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"{type(self).__name__} expects a torch.Tensor")
        got = image_operand(x)
        if got is None:
            if x.dtype == torch.uint8:
                raise RuntimeError(f"expected a uint8 input of shape [N,H,W,3], got {list(x.shape)}")
            if x.dtype == torch.float32:
                raise RuntimeError(f"expected a float32 input of shape [N,3,H,W], got {list(x.shape)}")
            raise RuntimeError(f"expected float32 [N,3,H,W] or uint8 [N,H,W,3] input, got {x.dtype}")
        return got

    def _input_device(self, x: torch.Tensor) -> torch.device:
        """The module's device, once `x` is known to be on it."""
        if x.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__}.forward got a CPU tensor: this implementation is GPU-only (hand-written HIP "
                               "kernels); there is no CPU fallback. Move the input with .to('cuda').")
        dev = self._device()
        if x.device != dev:
            raise RuntimeError(f"input on {x.device} but module parameters on {dev}")
        return dev

    def _ensure_workspace(self, device: torch.device, *dims, needs: str = "", sizer: str = "workspace_bytes") -> None:
        """The workspace of cid_<abi>_<sizer>(*dims) on `device`, grow-only.  With `needs` (LPIPS and the VGG loss, dims =
        (n, h, w)) a shape the library does not accept raises the ValueError that says what the model needs."""
        need = ctypes.c_size_t()
        rc = self._fn(sizer)(*self._form, *dims, ctypes.byref(need))
        if rc == 2 and needs:   # CID_ERR_SHAPE
            raise ValueError(f"image size {dims[1]}x{dims[2]} (N={dims[0]}) not accepted: {needs}")
        self._check(rc)
        need = need.value
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            if self._ws is not None:
                torch.cuda.synchronize(self._ws.device)   # kernels of an earlier call may still use the old workspace
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)

    def _stage(self, images: int, name: str, what: str, *dims, view: str = "stage_view") -> torch.Tensor:
        """The C8 tensor cid_<abi>_<view>(name, *dims) names, out of the workspace, as fp32 [images,C,Hs,Ws] (a copy)."""
        off, c, hs, ws, cb = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        rc = self._fn(view)(*self._form, name.encode(), *dims, ctypes.byref(off), ctypes.byref(c), ctypes.byref(hs),
                            ctypes.byref(ws), ctypes.byref(cb))
        if rc != _lib.CID_OK:
            raise KeyError(f"no stored stage {name!r} for {what} (cid_{self._abi}_{view} -> {rc})")
        count = images * c.value * hs.value * ws.value
        t = self._ws[off.value:off.value + 4 * count].view(torch.float32)
        t = t.view(images, c.value // cb.value, hs.value, ws.value, cb.value).permute(0, 1, 4, 2, 3)
        return t.reshape(images, c.value, hs.value, ws.value).clone()
