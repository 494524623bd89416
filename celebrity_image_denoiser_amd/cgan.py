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

from typing import Mapping, Optional, Sequence, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib, _packed

LATENT_DIM = 100
OUT_SIZE = 64
_BN = (0, 3, 6, 9)


class CGANGenerator(_packed.PackedModule):
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

    _abi = "cg"

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
        self._create(self.n_classes)

    def _batchnorms(self):
        return [(f"model.{i}", self.model[i], (which,)) for which, i in enumerate(_BN)]

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
        dev = self._input_device(z)
        n = z.shape[0]
        if n < 1:
            raise RuntimeError(f"empty input {list(z.shape)}")
        labels = self._labels(cond, n, dev)
        if raw and out_dtype != torch.float32:
            raise ValueError("raw=True gives the fp32 sums before tanh: it needs out_dtype=torch.float32")
        self.pack_weights()
        self._ensure_workspace(dev, n)
        z = z.reshape(n, LATENT_DIM).contiguous()
        out_fmt, out = _packed.image_output(out_dtype, n, OUT_SIZE, OUT_SIZE, dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self._check(self._fn("forward")(self._cid, z.data_ptr(), labels.data_ptr(), out.data_ptr(), out_fmt, n,
                                             _lib.CID_CG_RAW if raw else 0, self._ws.data_ptr(), self._ws.numel(), stream))
        return out

    def stage(self, name: str, n: int) -> torch.Tensor:
        """What the last forward over n images left in the workspace, as fp32 [n,C,Hs,Ws] (a copy): "l1" ([n,128,8,8]), "t1"
        ([n,128,16,16]), "t2" ([n,64,32,32]) or "t3" ([n,32,64,64]), each after its BatchNorm and ReLU (cid_cg_stage_view)."""
        return self._stage(n, name, f"{n} images", n)


def load_cgan(source: Union[str, Mapping, None] = None, n_classes: int = 10,
              device: Optional[Union[str, torch.device]] = None, strict: bool = False) -> CGANGenerator:
    """Build a CGANGenerator on `device` (default: current GPU) from a checkpoint path (read with the torch-free reader), a
    checkpoint dict or a state_dict: the state_dict is looked up under "generator", "state_dict" and "G" and "module." prefixes are
    stripped, as load_state_safely does (app.py:257-274).  `source=None` keeps the default initialisation.  Returns the module in
    eval mode."""
    device = _packed.cuda_device(device, "load_cgan")
    return _packed.load_into(CGANGenerator(n_classes), source, device, strict)


def latent(n: int, seed: int, first_index: int = 0, device: Optional[Union[str, torch.device]] = None) -> torch.Tensor:
    """fp32 [n,100] on `device` (default: current GPU): row i is the latent of image (first_index + i) under `seed`, Box-Muller of the
    hash streams "cgan:z:u1" / "cgan:z:u2" in float64, rounded to fp32 (cid_cg_latent; synth.cgan_latent_np is the restatement).  A row
    depends on (seed + first_index + i) alone, never on the batch."""
    device = _packed.cuda_device(device, "latent")
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
