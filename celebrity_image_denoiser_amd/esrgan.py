"""The server's second model (`ESRGANGenerator`, reference backend/app.py:188-218, the "esrgan" branch of /enhance, :387-397) on the GPU.

    ESRGANGenerator(num_residuals=8)          nn.Module with the reference's parameter names (initial.*, residuals.i.block.*, final.*,
                                              BatchNorm buffers included); forward(x) in eval mode
    load_esrgan(path_or_state_dict)           -> ESRGANGenerator from a checkpoint (its "generator" / "state_dict" / "G" entry)
    enhance(model, x)                         fp32 [N,3,H,W] in [0,1] -> the raw fp32 output [N,3,H,W] (no tanh, no clamp)
    enhance_u8(model, u8_nhwc)                uint8 [N,H,W,3] -> uint8 [N,H,W,3]: ToTensor() in, clamp(0,1) -> ToPILImage out
                                              (preprocess_image / postprocess_tensor, app.py:243-254), fused into the first / last kernel

Everything numeric runs in HIP kernels behind cid_esr_* (include/cid.h).  Eval mode only: BatchNorm uses its running statistics,
folded once per weight upload; calling the module in train mode raises.  There is no CPU fallback.

The server crops this model's UNPADDED output with the padding's offsets (app.py:474-480, while its esrgan branch never pads), which
shifts the image by pad//2 pixels whenever a size is not a multiple of 4.  That is not reproduced: the output here has the input's size.
"""
from __future__ import annotations

import ctypes
from typing import Mapping, Optional, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib

MAX_RESIDUALS = 16


class ResidualBlock(nn.Module):
    """conv -> BatchNorm -> PReLU -> conv -> BatchNorm under the reference's name `block` (a parameter container here)."""

    def __init__(self, channels: int):
        super().__init__()
        self.block = nn.Sequential(
            nn.Conv2d(channels, channels, 3, 1, 1),
            nn.BatchNorm2d(channels),
            nn.PReLU(),
            nn.Conv2d(channels, channels, 3, 1, 1),
            nn.BatchNorm2d(channels),
        )


class ESRGANGenerator(nn.Module):
    """The reference's ESRGAN generator.  `initial`, `residuals` and `final` are stock layers used as parameter containers, so
    state_dict keys, .to(), load_state_dict(), .train() and .eval() behave as in the reference.  forward(x):
      fp32 [N,3,H,W] in [0,1]  ->  the raw fp32 [N,3,H,W]
      uint8 [N,H,W,3]          ->  uint8 [N,H,W,3], the server's view of the output
    (`out_dtype` picks the other output format for either input),
    asynchronous on the current stream, without autograd history.  Weight changes are found by the tensors' version counters and
    repacked at the next call (after writes through `.data` call pack_weights(force=True))."""

    def __init__(self, num_residuals: int = 8):
        super().__init__()
        if not 0 <= int(num_residuals) <= MAX_RESIDUALS:
            raise ValueError(f"num_residuals must be in [0, {MAX_RESIDUALS}], got {num_residuals}")
        self.num_residuals = int(num_residuals)
        self.initial = nn.Sequential(nn.Conv2d(3, 64, 9, 1, 4), nn.PReLU())
        self.residuals = nn.Sequential(*[ResidualBlock(64) for _ in range(self.num_residuals)])
        self.final = nn.Conv2d(64, 3, 9, 1, 4)
        self._cid = ctypes.c_void_p()
        _lib.check_esr(None, _lib.lib().cid_esr_create(ctypes.byref(self._cid), self.num_residuals))
        self._blob = None          # packed weights on the device (uint8 tensor, owns the memory)
        self._packed_sig = None
        self._ws = None            # workspace (uint8 tensor, grow-only)

    def __del__(self):
        try:
            if getattr(self, "_cid", None):
                _lib.lib().cid_esr_destroy(self._cid)
                self._cid = None
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def _device(self) -> torch.device:
        return next(self.parameters()).device

    def _tensors(self):
        return list(self.state_dict(keep_vars=True).items())

    def _signature(self):
        eps = tuple(float(b.block[i].eps) for b in self.residuals for i in (1, 4))
        return tuple((k, t.data_ptr(), t._version, str(t.device)) for k, t in self._tensors()) + eps

    def pack_weights(self, force: bool = False) -> torch.Tensor:
        """Pack the state_dict into the kernels' layout on the module's GPU, BatchNorm folded (if anything changed since the last
        call)."""
        sig = self._signature()
        if not force and self._blob is not None and sig == self._packed_sig:
            return self._blob
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("ESRGANGenerator runs only on an AMD GPU (HIP kernels behind libcid.so); move it with .to('cuda') "
                               "first. There is no CPU fallback.")
        L = _lib.lib()
        for i, blk in enumerate(self.residuals):
            for which, idx in enumerate((1, 4)):
                bn = blk.block[idx]
                if not (bn.affine and bn.track_running_stats):
                    raise NotImplementedError(f"residuals.{i}.block.{idx}: only BatchNorm2d(affine=True, track_running_stats=True)")
                _lib.check_esr(self._cid, L.cid_esr_set_bn_eps(self._cid, i, which, float(bn.eps)))
        for key, t in self._tensors():
            if key.endswith("num_batches_tracked"):
                a = t.detach().cpu().numpy()   # 0-d int64: accepted and ignored by the library
            else:
                a = np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())
            shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
            _lib.check_esr(self._cid, L.cid_esr_set_weight(self._cid, key.encode(), a.ctypes.data, shape, a.ndim))
        blob = torch.empty(L.cid_esr_packed_weights_bytes(self._cid), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check_esr(self._cid, L.cid_esr_upload_weights(self._cid, blob.data_ptr(), stream))
        self._blob, self._packed_sig = blob, sig
        return blob

    # ------------------------------------------------------------------ forward
    def _ensure_workspace(self, n: int, h: int, w: int, device: torch.device) -> None:
        need = ctypes.c_size_t()
        _lib.check_esr(self._cid, _lib.lib().cid_esr_workspace_bytes(n, h, w, ctypes.byref(need)))
        if self._ws is None or self._ws.numel() < need.value or self._ws.device != device:
            if self._ws is not None:
                torch.cuda.synchronize(self._ws.device)   # kernels of an earlier call may still use the old workspace
            self._ws = None
            self._ws = torch.empty(need.value, dtype=torch.uint8, device=device)

    def forward(self, x: torch.Tensor, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        if self.training:
            raise RuntimeError("ESRGANGenerator is in train mode: train-mode BatchNorm (batch statistics) is not implemented; call "
                               ".eval() first, as the server does (app.py:240)")
        if not isinstance(x, torch.Tensor):
            raise TypeError("ESRGANGenerator expects a torch.Tensor")
        if x.dtype == torch.uint8:
            if x.dim() != 4 or x.shape[3] != 3:
                raise RuntimeError(f"expected a uint8 input of shape [N,H,W,3], got {list(x.shape)}")
            fmt, (n, h, w) = _lib.CID_FMT_U8_NHWC, (x.shape[0], x.shape[1], x.shape[2])
        elif x.dtype == torch.float32:
            if x.dim() != 4 or x.shape[1] != 3:
                raise RuntimeError(f"expected a float32 input of shape [N,3,H,W], got {list(x.shape)}")
            fmt, (n, h, w) = _lib.CID_FMT_F32_NCHW, (x.shape[0], x.shape[2], x.shape[3])
        else:
            raise RuntimeError(f"expected float32 [N,3,H,W] or uint8 [N,H,W,3] input, got {x.dtype}")
        if x.device.type != "cuda":
            raise RuntimeError("ESRGANGenerator.forward got a CPU tensor: this implementation is GPU-only (hand-written HIP kernels); "
                               "there is no CPU fallback. Move the input with .to('cuda').")
        dev = self._device()
        if x.device != dev:
            raise RuntimeError(f"input on {x.device} but module parameters on {dev}")
        if n < 1 or h < 1 or w < 1:
            raise RuntimeError(f"empty input {list(x.shape)}")
        self.pack_weights()
        self._ensure_workspace(n, h, w, dev)
        x = x.contiguous()
        out_dtype = x.dtype if out_dtype is None else out_dtype
        if out_dtype == torch.uint8:
            out_fmt, out = _lib.CID_FMT_U8_NHWC, torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
        elif out_dtype == torch.float32:
            out_fmt, out = _lib.CID_FMT_F32_NCHW, torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
        else:
            raise RuntimeError(f"out_dtype must be torch.float32 or torch.uint8, got {out_dtype}")
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check_esr(self._cid, _lib.lib().cid_esr_forward(self._cid, x.data_ptr(), fmt, out.data_ptr(), out_fmt, n, h, w,
                                                                 self._ws.data_ptr(), self._ws.numel(), stream))
        return out

    def stage(self, name: str, n: int, h: int, w: int) -> torch.Tensor:
        """What the last forward of an [n,3,h,w] input left in the workspace as fp32 [n,64,h,w] (a copy): "x1", or "tail_in", the
        tensor the last launch read (cid_esr_stage_view)."""
        off, c, hs, ws, cb = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        rc = _lib.lib().cid_esr_stage_view(name.encode(), n, h, w, ctypes.byref(off), ctypes.byref(c), ctypes.byref(hs), ctypes.byref(ws),
                                           ctypes.byref(cb))
        if rc != _lib.CID_OK:
            raise KeyError(f"no stored stage {name!r} for input [{n},3,{h},{w}] (cid_esr_stage_view -> {rc})")
        count = n * c.value * hs.value * ws.value
        t = self._ws[off.value:off.value + 4 * count].view(torch.float32)
        t = t.view(n, c.value // cb.value, hs.value, ws.value, cb.value).permute(0, 1, 4, 2, 3)
        return t.reshape(n, c.value, hs.value, ws.value).clone()


def load_esrgan(source: Union[str, Mapping, None] = None, num_residuals: int = 8,
                device: Optional[Union[str, torch.device]] = None, strict: bool = False) -> ESRGANGenerator:
    """Build an ESRGANGenerator on `device` (default: current GPU) from a checkpoint path (read with the torch-free reader), a
    checkpoint dict or a state_dict: the state_dict is looked up under "generator", "state_dict" and "G" (the server's own loader
    reads checkpoint['G'], app.py:236-241) and "module." prefixes are stripped, as load_state_safely does.  `source=None` keeps the
    default initialisation.  Returns the module in eval mode."""
    from .api import _read_checkpoint_file, extract_state_dict

    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if device is None or torch.device(device).type != "cuda":
        raise RuntimeError("celebrity_image_denoiser_amd.load_esrgan: an AMD GPU is required (no CPU fallback)")
    model = ESRGANGenerator(num_residuals)
    if isinstance(source, str):
        model.load_state_dict(_read_checkpoint_file(source), strict=strict)
    elif source is not None:
        sd = {k: (v if isinstance(v, torch.Tensor) else torch.as_tensor(v)) for k, v in extract_state_dict(source).items()}
        model.load_state_dict(sd, strict=strict)
    model.to(device).eval()
    model.pack_weights()
    return model


def enhance(model: ESRGANGenerator, x: torch.Tensor) -> torch.Tensor:
    """fp32 [N,3,H,W] in [0,1] on the model's GPU -> the network's raw fp32 output [N,3,H,W] (the reference's model(tensor))."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise RuntimeError("enhance expects a float32 [N,3,H,W] tensor; for uint8 images use enhance_u8")
    return model(x)


def enhance_u8(model: ESRGANGenerator, images_u8: torch.Tensor) -> torch.Tensor:
    """uint8 [N,H,W,3] on the model's GPU -> uint8 [N,H,W,3]: /255 -> network -> clamp(0,1).mul(255).byte(), the server's
    preprocess_image / postprocess_tensor around the model (app.py:243-254), in the first and last kernel."""
    if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8:
        raise RuntimeError("enhance_u8 expects a uint8 [N,H,W,3] tensor")
    return model(images_u8)
