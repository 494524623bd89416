"""The server's third model (`SRGANGenerator`, reference backend/app.py:145-186, the "srgan" branch of /enhance) on the GPU.

    SRGANGenerator(scale_factor=4)            nn.Module with the reference's parameter names (initial.*, res_blocks.i.j.*, mid.*,
                                              upscale.*, final.*, BatchNorm buffers included); forward(x) in eval mode
    load_srgan(path_or_state_dict)            -> SRGANGenerator from a checkpoint (its "generator" / "state_dict" / "G" entry)
    super_resolve(model, x)                   fp32 [N,3,H,W] in [-1,1] -> fp32 [N,3,sH,sW] = tanh(.)
    super_resolve_u8(model, u8_nhwc)          uint8 [N,H,W,3] -> uint8 [N,s*Hp,s*Wp,3], the server's branch: pad to a multiple of
                                              4*s -> ToTensor -> Normalize(0.5, 0.5) -> network -> y*0.5+0.5 -> clamp -> ToPILImage,
                                              with padding and both conversions inside the first / last kernel

Everything numeric runs in HIP kernels behind cid_sr_* (include/cid.h).  Eval mode only: BatchNorm uses its running statistics,
folded once per weight upload; calling the module in train mode raises.  There is no CPU fallback.

The server shows this model's whole padded output and crops only the input's picture (app.py:481-485); `crop=True` gives the part of
the output that belongs to the unpadded image instead.
"""
from __future__ import annotations

import ctypes
from typing import Mapping, Optional, Sequence, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib

MAX_SCALE = 8
NUM_BLOCKS = 5


def _stages(scale_factor: int) -> int:
    s = int(scale_factor)
    if s < 1 or s & (s - 1):
        raise ValueError(f"scale_factor must be a power of two (got {scale_factor})")
    if s > MAX_SCALE:
        raise ValueError(f"scale_factor above {MAX_SCALE} is not implemented (got {scale_factor})")
    return s.bit_length() - 1


class SRGANGenerator(nn.Module):
    """The reference's SRGAN generator.  `initial`, `res_blocks`, `mid`, `upscale` and `final` are stock layers used as parameter
    containers, so state_dict keys, .to(), load_state_dict(), .train() and .eval() behave as in the reference.  forward(x):
      fp32 [N,3,H,W] in [-1,1]  ->  fp32 [N,3,s*Hp,s*Wp] = tanh(.)   (`raw=True`: the sums before tanh)
      uint8 [N,H,W,3]           ->  uint8 [N,s*Hp,s*Wp,3], the server's view of the output
    (`out_dtype` picks the other output format for either input), where `padding` = (left, top, right, bottom) is the server's
    Pad(fill=0) of the input, done as index arithmetic in the first kernel, and Hp x Wp the padded size.  Asynchronous on the current
    stream, without autograd history.  Weight changes are found by the tensors' version counters and repacked at the next call
    (after writes through `.data` call pack_weights(force=True))."""

    def __init__(self, scale_factor: int = 4):
        super().__init__()
        self.num_upsamples = _stages(scale_factor)
        self.scale_factor = int(scale_factor)
        self.initial = nn.Sequential(nn.Conv2d(3, 64, 9, 1, 4), nn.PReLU())
        self.res_blocks = nn.Sequential(*[
            nn.Sequential(nn.Conv2d(64, 64, 3, 1, 1), nn.BatchNorm2d(64), nn.PReLU(), nn.Conv2d(64, 64, 3, 1, 1), nn.BatchNorm2d(64))
            for _ in range(NUM_BLOCKS)])
        self.mid = nn.Conv2d(64, 64, 3, 1, 1)
        upscale = []
        for _ in range(self.num_upsamples):
            upscale += [nn.Conv2d(64, 256, 3, 1, 1), nn.PixelShuffle(2), nn.PReLU()]
        self.upscale = nn.Sequential(*upscale)
        self.final = nn.Conv2d(64, 3, 9, 1, 4)
        self._cid = ctypes.c_void_p()
        _lib.check_sr(None, _lib.lib().cid_sr_create(ctypes.byref(self._cid), self.scale_factor))
        self._blob = None          # packed weights on the device (uint8 tensor, owns the memory)
        self._packed_sig = None
        self._ws = None            # workspace (uint8 tensor, grow-only)

    def __del__(self):
        try:
            if getattr(self, "_cid", None):
                _lib.lib().cid_sr_destroy(self._cid)
                self._cid = None
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def _device(self) -> torch.device:
        return next(self.parameters()).device

    def _tensors(self):
        return list(self.state_dict(keep_vars=True).items())

    def _signature(self):
        eps = tuple(float(b[i].eps) for b in self.res_blocks for i in (1, 4))
        return tuple((k, t.data_ptr(), t._version, str(t.device)) for k, t in self._tensors()) + eps

    def pack_weights(self, force: bool = False) -> torch.Tensor:
        """Pack the state_dict into the kernels' layout on the module's GPU, BatchNorm folded (if anything changed since the last
        call)."""
        sig = self._signature()
        if not force and self._blob is not None and sig == self._packed_sig:
            return self._blob
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("SRGANGenerator runs only on an AMD GPU (HIP kernels behind libcid.so); move it with .to('cuda') "
                               "first. There is no CPU fallback.")
        L = _lib.lib()
        for i, blk in enumerate(self.res_blocks):
            for which, idx in enumerate((1, 4)):
                bn = blk[idx]
                if not (bn.affine and bn.track_running_stats):
                    raise NotImplementedError(f"res_blocks.{i}.{idx}: only BatchNorm2d(affine=True, track_running_stats=True)")
                _lib.check_sr(self._cid, L.cid_sr_set_bn_eps(self._cid, i, which, float(bn.eps)))
        for key, t in self._tensors():
            if key.endswith("num_batches_tracked"):
                a = t.detach().cpu().numpy()   # 0-d int64: accepted and ignored by the library
            else:
                a = np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())
            shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
            _lib.check_sr(self._cid, L.cid_sr_set_weight(self._cid, key.encode(), a.ctypes.data, shape, a.ndim))
        blob = torch.empty(L.cid_sr_packed_weights_bytes(self._cid), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check_sr(self._cid, L.cid_sr_upload_weights(self._cid, blob.data_ptr(), stream))
        self._blob, self._packed_sig = blob, sig
        return blob

    # ------------------------------------------------------------------ forward
    def _ensure_workspace(self, n: int, hp: int, wp: int, device: torch.device) -> None:
        need = ctypes.c_size_t()
        _lib.check_sr(self._cid, _lib.lib().cid_sr_workspace_bytes(n, hp, wp, self.scale_factor, ctypes.byref(need)))
        if self._ws is None or self._ws.numel() < need.value or self._ws.device != device:
            if self._ws is not None:
                torch.cuda.synchronize(self._ws.device)   # kernels of an earlier call may still use the old workspace
            self._ws = None
            self._ws = torch.empty(need.value, dtype=torch.uint8, device=device)

    def forward(self, x: torch.Tensor, out_dtype: Optional[torch.dtype] = None, raw: bool = False,
                padding: Sequence[int] = (0, 0, 0, 0)) -> torch.Tensor:
        if self.training:
            raise RuntimeError("SRGANGenerator is in train mode: train-mode BatchNorm (batch statistics) is not implemented; call "
                               ".eval() first, as the server does (app.py:273)")
        if not isinstance(x, torch.Tensor):
            raise TypeError("SRGANGenerator expects a torch.Tensor")
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
            raise RuntimeError("SRGANGenerator.forward got a CPU tensor: this implementation is GPU-only (hand-written HIP kernels); "
                               "there is no CPU fallback. Move the input with .to('cuda').")
        dev = self._device()
        if x.device != dev:
            raise RuntimeError(f"input on {x.device} but module parameters on {dev}")
        if n < 1 or h < 1 or w < 1:
            raise RuntimeError(f"empty input {list(x.shape)}")
        pl, pt, pr, pb = (int(v) for v in padding)
        if min(pl, pt, pr, pb) < 0 or max(pl, pt, pr, pb) > 4096:
            raise ValueError(f"padding must be four values in [0, 4096] (left, top, right, bottom), got {tuple(padding)}")
        out_dtype = x.dtype if out_dtype is None else out_dtype
        if raw and out_dtype != torch.float32:
            raise ValueError("raw=True gives the fp32 sums before tanh: it needs out_dtype=torch.float32")
        hp, wp, s = h + pt + pb, w + pl + pr, self.scale_factor
        self.pack_weights()
        self._ensure_workspace(n, hp, wp, dev)
        x = x.contiguous()
        if out_dtype == torch.uint8:
            out_fmt, out = _lib.CID_FMT_U8_NHWC, torch.empty((n, s * hp, s * wp, 3), dtype=torch.uint8, device=dev)
        elif out_dtype == torch.float32:
            out_fmt, out = _lib.CID_FMT_F32_NCHW, torch.empty((n, 3, s * hp, s * wp), dtype=torch.float32, device=dev)
        else:
            raise RuntimeError(f"out_dtype must be torch.float32 or torch.uint8, got {out_dtype}")
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check_sr(self._cid, _lib.lib().cid_sr_forward(self._cid, x.data_ptr(), fmt, out.data_ptr(), out_fmt, n, h, w, pl, pt, pr, pb,
                                                               _lib.CID_SR_RAW if raw else 0, self._ws.data_ptr(), self._ws.numel(), stream))
        return out

    def stage(self, name: str, n: int, hp: int, wp: int) -> torch.Tensor:
        """What the last forward over a padded [n,3,hp,wp] input left in the workspace, as fp32 [n,64,Hs,Ws] (a copy): "x0", "trunk",
        "up1", or "tail_in", the tensor the last launch read (cid_sr_stage_view)."""
        off, c, hs, ws, cb = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        rc = _lib.lib().cid_sr_stage_view(name.encode(), n, hp, wp, self.scale_factor, ctypes.byref(off), ctypes.byref(c), ctypes.byref(hs),
                                          ctypes.byref(ws), ctypes.byref(cb))
        if rc != _lib.CID_OK:
            raise KeyError(f"no stored stage {name!r} for input [{n},3,{hp},{wp}] (cid_sr_stage_view -> {rc})")
        count = n * c.value * hs.value * ws.value
        t = self._ws[off.value:off.value + 4 * count].view(torch.float32)
        t = t.view(n, c.value // cb.value, hs.value, ws.value, cb.value).permute(0, 1, 4, 2, 3)
        return t.reshape(n, c.value, hs.value, ws.value).clone()


def load_srgan(source: Union[str, Mapping, None] = None, scale_factor: int = 4,
               device: Optional[Union[str, torch.device]] = None, strict: bool = False) -> SRGANGenerator:
    """Build an SRGANGenerator on `device` (default: current GPU) from a checkpoint path (read with the torch-free reader), a
    checkpoint dict or a state_dict: the state_dict is looked up under "generator", "state_dict" and "G" and "module." prefixes are
    stripped, as load_state_safely does (app.py:257-274).  `source=None` keeps the default initialisation.  Returns the module in
    eval mode."""
    from .api import _read_checkpoint_file, extract_state_dict

    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if device is None or torch.device(device).type != "cuda":
        raise RuntimeError("celebrity_image_denoiser_amd.load_srgan: an AMD GPU is required (no CPU fallback)")
    model = SRGANGenerator(scale_factor)
    if isinstance(source, str):
        model.load_state_dict(_read_checkpoint_file(source), strict=strict)
    elif source is not None:
        sd = {k: (v if isinstance(v, torch.Tensor) else torch.as_tensor(v)) for k, v in extract_state_dict(source).items()}
        model.load_state_dict(sd, strict=strict)
    model.to(device).eval()
    model.pack_weights()
    return model


def srgan_padding(h: int, w: int, scale_factor: int, pad_divisor: int = 4):
    """The server's get_padding(image, pad_divisor, scale) (app.py:276-281) as (left, top, right, bottom): each side is padded to a
    multiple of pad_divisor * scale, the left / top share being pad // 2."""
    d = int(pad_divisor) * int(scale_factor)
    if d < 1:
        raise ValueError("pad_divisor must be positive")
    pw, ph = (d - w % d) % d, (d - h % d) % d
    return pw // 2, ph // 2, pw - pw // 2, ph - ph // 2


def super_resolve(model: SRGANGenerator, x: torch.Tensor) -> torch.Tensor:
    """fp32 [N,3,H,W] in [-1,1] on the model's GPU -> fp32 [N,3,sH,sW] in [-1,1] (the reference's model(tensor))."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise RuntimeError("super_resolve expects a float32 [N,3,H,W] tensor; for uint8 images use super_resolve_u8")
    return model(x)


def super_resolve_u8(model: SRGANGenerator, images_u8: torch.Tensor, pad_divisor: int = 4, crop: bool = False) -> torch.Tensor:
    """uint8 [N,H,W,3] on the model's GPU -> uint8 [N,s*Hp,s*Wp,3], the server's "srgan" branch: get_padding(image, 4, scale) ->
    Pad(fill=0) -> ToTensor -> Normalize(0.5, 0.5) -> network -> y*0.5+0.5 -> clamp(0,1) -> ToPILImage, all inside the first and last
    kernel.  `crop=True` returns the view [s*pt : s*(pt+H), s*pl : s*(pl+W)] of that result: the unpadded image's part."""
    if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4:
        raise RuntimeError("super_resolve_u8 expects a uint8 [N,H,W,3] tensor")
    h, w, s = images_u8.shape[1], images_u8.shape[2], model.scale_factor
    pl, pt, pr, pb = srgan_padding(h, w, s, pad_divisor)
    out = model(images_u8, padding=(pl, pt, pr, pb))
    return out[:, s * pt:s * (pt + h), s * pl:s * (pl + w)] if crop else out
