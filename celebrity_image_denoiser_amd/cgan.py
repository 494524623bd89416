"""The server's fourth model (`CGANGenerator`, reference backend/app.py:105-143, the "cgan" branch of /enhance) on the GPU.

    CGANGenerator(n_classes=10)               nn.Module with the reference's parameter names (label_emb.*, l1.*, model.i.*, BatchNorm
                                              buffers included); forward(z, labels) in eval mode
    load_cgan(path_or_state_dict)             -> CGANGenerator from a checkpoint (its "generator" / "state_dict" / "G" entry)
    latent(n, seed)                           fp32 [n,100] standard normal deviates from the package's counter-based hash streams,
                                              drawn on the device (the server draws torch.randn(N,100,1,1), app.py:428)
    generate(model, labels, seed=... | z=...) -> fp32 [N,3,64,64] = tanh(.)
    generate_u8(model, labels, ...)           -> uint8 [N,64,64,3], the server's view y*0.5+0.5 -> clamp -> *255 -> byte

Everything numeric runs in HIP kernels behind cid_cg_* (include/cid.h).  Eval mode only: BatchNorm uses its running statistics,
folded once per weight upload; calling the module in train mode raises.  There is no CPU fallback.

Only the label-conditioned branch exists.  The reference's image-conditioned branch (a 4-D `cond`, app.py:139-143) concatenates two
3-channel images and feeds the 6 channels to BatchNorm2d(128): it raises for every input in the reference itself.
"""
from __future__ import annotations

import ctypes
from typing import Mapping, Optional, Sequence, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib

LATENT_DIM = 100
OUT_SIZE = 64
_BN = (0, 3, 6, 9)


class CGANGenerator(nn.Module):
    """The reference's cGAN generator.  `label_emb`, `l1` and `model` are stock layers used as parameter containers, so state_dict
    keys, .to(), load_state_dict(), .train() and .eval() behave as in the reference.  forward(z, cond):
      z     fp32 [N,100] or [N,100,1,1] on the module's GPU
      cond  the class labels: a 1-D int64 tensor on the GPU (not range-checked: an invalid label gives an all-NaN image, or all-zero
            bytes, at its position and leaves the others alone) or on the host, or a sequence of ints (range-checked: IndexError, as
            nn.Embedding)
      ->    fp32 [N,3,64,64] = tanh(.)   (`raw=True`: the sums before tanh), or with out_dtype=torch.uint8 the server's view
            uint8 [N,64,64,3].
    Asynchronous on the current stream, without autograd history.  Weight changes are found by the tensors' version counters and
    repacked at the next call (after writes through `.data` call pack_weights(force=True))."""

    def __init__(self, n_classes: int = 10, latent_dim: int = LATENT_DIM):
        super().__init__()
        if int(latent_dim) != LATENT_DIM:
            raise ValueError(f"latent_dim must be {LATENT_DIM} (got {latent_dim}): the reference's forward hard-codes "
                             "label_emb(cond).view(-1, 100, 1, 1) (app.py:133), so no other value runs there either")
        if int(n_classes) < 1:
            raise ValueError(f"n_classes must be positive (got {n_classes})")
        self.n_classes = int(n_classes)
        self.latent_dim = LATENT_DIM
        self.init_size = 8
        self.label_emb = nn.Embedding(self.n_classes, LATENT_DIM)
        self.l1 = nn.Linear(2 * LATENT_DIM, 128 * self.init_size * self.init_size)
        self.model = nn.Sequential(
            nn.BatchNorm2d(128), nn.ReLU(inplace=True), nn.ConvTranspose2d(128, 128, 4, stride=2, padding=1),
            nn.BatchNorm2d(128), nn.ReLU(inplace=True), nn.ConvTranspose2d(128, 64, 4, stride=2, padding=1),
            nn.BatchNorm2d(64), nn.ReLU(inplace=True), nn.ConvTranspose2d(64, 32, 4, stride=2, padding=1),
            nn.BatchNorm2d(32), nn.ReLU(inplace=True), nn.Conv2d(32, 3, 3, stride=1, padding=1))
        self._cid = ctypes.c_void_p()
        _lib.check_cg(None, _lib.lib().cid_cg_create(ctypes.byref(self._cid), self.n_classes))
        self._blob = None          # packed weights on the device (uint8 tensor, owns the memory)
        self._packed_sig = None
        self._ws = None            # workspace (uint8 tensor, grow-only)

    def __del__(self):
        try:
            if getattr(self, "_cid", None):
                _lib.lib().cid_cg_destroy(self._cid)
                self._cid = None
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def _device(self) -> torch.device:
        return next(self.parameters()).device

    def _tensors(self):
        return list(self.state_dict(keep_vars=True).items())

    def _signature(self):
        eps = tuple(float(self.model[i].eps) for i in _BN)
        return tuple((k, t.data_ptr(), t._version, str(t.device)) for k, t in self._tensors()) + eps

    def pack_weights(self, force: bool = False) -> torch.Tensor:
        """Pack the state_dict into the kernels' layout on the module's GPU, BatchNorm folded (if anything changed since the last
        call)."""
        sig = self._signature()
        if not force and self._blob is not None and sig == self._packed_sig:
            return self._blob
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("CGANGenerator runs only on an AMD GPU (HIP kernels behind libcid.so); move it with .to('cuda') "
                               "first. There is no CPU fallback.")
        L = _lib.lib()
        for which, i in enumerate(_BN):
            bn = self.model[i]
            if not (bn.affine and bn.track_running_stats):
                raise NotImplementedError(f"model.{i}: only BatchNorm2d(affine=True, track_running_stats=True)")
            _lib.check_cg(self._cid, L.cid_cg_set_bn_eps(self._cid, which, float(bn.eps)))
        for key, t in self._tensors():
            if key.endswith("num_batches_tracked"):
                a = t.detach().cpu().numpy()   # 0-d int64: accepted and ignored by the library
            else:
                a = np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())
            shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
            _lib.check_cg(self._cid, L.cid_cg_set_weight(self._cid, key.encode(), a.ctypes.data, shape, a.ndim))
        blob = torch.empty(L.cid_cg_packed_weights_bytes(self._cid), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check_cg(self._cid, L.cid_cg_upload_weights(self._cid, blob.data_ptr(), stream))
        self._blob, self._packed_sig = blob, sig
        return blob

    # ------------------------------------------------------------------ forward
    def _ensure_workspace(self, n: int, device: torch.device) -> None:
        need = ctypes.c_size_t()
        _lib.check_cg(self._cid, _lib.lib().cid_cg_workspace_bytes(n, ctypes.byref(need)))
        if self._ws is None or self._ws.numel() < need.value or self._ws.device != device:
            if self._ws is not None:
                torch.cuda.synchronize(self._ws.device)   # kernels of an earlier call may still use the old workspace
            self._ws = None
            self._ws = torch.empty(need.value, dtype=torch.uint8, device=device)

    def _labels(self, cond, n: int, dev: torch.device) -> torch.Tensor:
        if isinstance(cond, torch.Tensor):
            if cond.dim() == 4:
                raise NotImplementedError(
                    "the image-conditioned branch (a 4-D cond) is not built: the reference concatenates two 3-channel images and feeds "
                    "6 channels to BatchNorm2d(128), which raises for every input (\"running_mean should contain 6 elements not 128\", "
                    "app.py:139-143)")
            if cond.dim() != 1 or cond.dtype != torch.int64:
                raise RuntimeError(f"cond must be a 1-D int64 tensor of class labels, got {cond.dtype} {list(cond.shape)}")
        else:
            if cond is None:
                raise ValueError("cGAN requires a condition (label or tensor)")
            cond = torch.as_tensor(np.asarray(list(cond), dtype=np.int64).reshape(-1))
        if cond.shape[0] != n:
            raise RuntimeError(f"{n} latent vectors but {cond.shape[0]} labels")
        if cond.device.type != "cuda":
            if n and (int(cond.min()) < 0 or int(cond.max()) >= self.n_classes):
                raise IndexError(f"label out of range: labels must lie in [0, {self.n_classes})")
            cond = cond.to(dev)
        elif cond.device != dev:
            raise RuntimeError(f"labels on {cond.device} but module parameters on {dev}")
        return cond.contiguous()

    def forward(self, z: torch.Tensor, cond=None, out_dtype: torch.dtype = torch.float32, raw: bool = False) -> torch.Tensor:
        if self.training:
            raise RuntimeError("CGANGenerator is in train mode: train-mode BatchNorm (batch statistics) is not implemented; call "
                               ".eval() first, as the server does (app.py:273)")
        if not isinstance(z, torch.Tensor):
            raise TypeError("CGANGenerator expects a torch.Tensor")
        if z.dtype != torch.float32 or z.dim() not in (2, 4) or tuple(z.shape[1:]) not in ((LATENT_DIM,), (LATENT_DIM, 1, 1)):
            raise RuntimeError(f"expected a float32 latent of shape [N,{LATENT_DIM}] or [N,{LATENT_DIM},1,1], got {z.dtype} {list(z.shape)}")
        if z.device.type != "cuda":
            raise RuntimeError("CGANGenerator.forward got a CPU tensor: this implementation is GPU-only (hand-written HIP kernels); "
                               "there is no CPU fallback. Move the input with .to('cuda').")
        dev = self._device()
        if z.device != dev:
            raise RuntimeError(f"input on {z.device} but module parameters on {dev}")
        n = z.shape[0]
        if n < 1:
            raise RuntimeError(f"empty input {list(z.shape)}")
        labels = self._labels(cond, n, dev)
        if raw and out_dtype != torch.float32:
            raise ValueError("raw=True gives the fp32 sums before tanh: it needs out_dtype=torch.float32")
        self.pack_weights()
        self._ensure_workspace(n, dev)
        z = z.reshape(n, LATENT_DIM).contiguous()
        if out_dtype == torch.uint8:
            out_fmt, out = _lib.CID_FMT_U8_NHWC, torch.empty((n, OUT_SIZE, OUT_SIZE, 3), dtype=torch.uint8, device=dev)
        elif out_dtype == torch.float32:
            out_fmt, out = _lib.CID_FMT_F32_NCHW, torch.empty((n, 3, OUT_SIZE, OUT_SIZE), dtype=torch.float32, device=dev)
        else:
            raise RuntimeError(f"out_dtype must be torch.float32 or torch.uint8, got {out_dtype}")
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check_cg(self._cid, _lib.lib().cid_cg_forward(self._cid, z.data_ptr(), labels.data_ptr(), out.data_ptr(), out_fmt, n,
                                                               _lib.CID_CG_RAW if raw else 0, self._ws.data_ptr(), self._ws.numel(), stream))
        return out

    def stage(self, name: str, n: int) -> torch.Tensor:
        """What the last forward over n images left in the workspace, as fp32 [n,C,Hs,Ws] (a copy): "l1" ([n,128,8,8]), "t1"
        ([n,128,16,16]), "t2" ([n,64,32,32]) or "t3" ([n,32,64,64]), each after its BatchNorm and ReLU (cid_cg_stage_view)."""
        off, c, hs, ws, cb = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        rc = _lib.lib().cid_cg_stage_view(name.encode(), n, ctypes.byref(off), ctypes.byref(c), ctypes.byref(hs), ctypes.byref(ws),
                                          ctypes.byref(cb))
        if rc != _lib.CID_OK:
            raise KeyError(f"no stored stage {name!r} for {n} images (cid_cg_stage_view -> {rc})")
        count = n * c.value * hs.value * ws.value
        t = self._ws[off.value:off.value + 4 * count].view(torch.float32)
        t = t.view(n, c.value // cb.value, hs.value, ws.value, cb.value).permute(0, 1, 4, 2, 3)
        return t.reshape(n, c.value, hs.value, ws.value).clone()


def load_cgan(source: Union[str, Mapping, None] = None, n_classes: int = 10,
              device: Optional[Union[str, torch.device]] = None, strict: bool = False) -> CGANGenerator:
    """Build a CGANGenerator on `device` (default: current GPU) from a checkpoint path (read with the torch-free reader), a
    checkpoint dict or a state_dict: the state_dict is looked up under "generator", "state_dict" and "G" and "module." prefixes are
    stripped, as load_state_safely does (app.py:257-274).  `source=None` keeps the default initialisation.  Returns the module in
    eval mode."""
    from .api import _read_checkpoint_file, extract_state_dict

    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if device is None or torch.device(device).type != "cuda":
        raise RuntimeError("celebrity_image_denoiser_amd.load_cgan: an AMD GPU is required (no CPU fallback)")
    model = CGANGenerator(n_classes)
    if isinstance(source, str):
        model.load_state_dict(_read_checkpoint_file(source), strict=strict)
    elif source is not None:
        sd = {k: (v if isinstance(v, torch.Tensor) else torch.as_tensor(v)) for k, v in extract_state_dict(source).items()}
        model.load_state_dict(sd, strict=strict)
    model.to(device).eval()
    model.pack_weights()
    return model


def latent(n: int, seed: int, first_index: int = 0, device: Optional[Union[str, torch.device]] = None) -> torch.Tensor:
    """fp32 [n,100] on `device` (default: current GPU): row i is the latent of image (first_index + i) under `seed`, Box-Muller of the
    hash streams "cgan:z:u1" / "cgan:z:u2" in float64, rounded to fp32 (cid_cg_latent; synth.cgan_latent_np is the restatement).  A row
    depends on (seed + first_index + i) alone, never on the batch."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if device is None or torch.device(device).type != "cuda":
        raise RuntimeError("celebrity_image_denoiser_amd.latent: an AMD GPU is required (no CPU fallback)")
    device = torch.device(device)
    if int(n) < 1:
        raise ValueError(f"n must be positive (got {n})")
    z = torch.empty((int(n), LATENT_DIM), dtype=torch.float32, device=device)
    mask = 0xFFFFFFFFFFFFFFFF
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        rc = _lib.lib().cid_cg_latent(int(seed) & mask, int(first_index) & mask, int(n), z.data_ptr(), stream)
    if rc != _lib.CID_OK:
        raise _lib.CidError(rc, f"cid_cg_latent -> {rc}")
    return z


def _latent_of(model: CGANGenerator, n: int, seed, z) -> torch.Tensor:
    if (seed is None) == (z is None):
        raise ValueError("give exactly one of seed and z")
    return latent(n, seed, device=model._device()) if z is None else z


def _count(labels) -> int:
    return int(labels.shape[0]) if isinstance(labels, torch.Tensor) else len(labels)


def generate(model: CGANGenerator, labels: Union[torch.Tensor, Sequence[int]], seed: Optional[int] = None,
             z: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One image per label: fp32 [N,3,64,64] in [-1,1] (the reference's model(z, labels)).  The latent is `z`, or is drawn from
    `seed` (image i uses seed + i): exactly one of the two."""
    return model(_latent_of(model, _count(labels), seed, z), labels)


def generate_u8(model: CGANGenerator, labels: Union[torch.Tensor, Sequence[int]], seed: Optional[int] = None,
                z: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [N,64,64,3]: the server's view of generate() (y*0.5+0.5 -> clamp(0,1) -> ToPILImage, app.py:435, 472), made inside the
    last kernel."""
    return model(_latent_of(model, _count(labels), seed, z), labels, out_dtype=torch.uint8)
