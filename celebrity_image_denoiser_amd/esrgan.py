"""The server's second model (`ESRGANGenerator`, reference backend/app.py:188-218, the "esrgan" branch of /enhance, :387-397) on the GPU.

    ESRGANGenerator(num_residuals=8)          nn.Module with the reference's parameter names (initial.*, residuals.i.block.*, final.*,
                                              BatchNorm buffers included); forward(x) in eval mode
    ESRGANGenerator(8, batch_stats=True)      the same module with a train-mode forward as well: BatchNorm on batch statistics,
                                              running buffers updated in place (the trainer's denoised = G(noisy) after G.train())
    load_esrgan(path_or_state_dict)           -> ESRGANGenerator from a checkpoint (its "generator" / "state_dict" / "G" entry)
    enhance(model, x)                         fp32 [N,3,H,W] in [0,1] -> the raw fp32 output [N,3,H,W] (no tanh, no clamp)
    enhance_u8(model, u8_nhwc)                uint8 [N,H,W,3] -> uint8 [N,H,W,3]: ToTensor() in, clamp(0,1) -> ToPILImage out
                                              (preprocess_image / postprocess_tensor, app.py:243-254), fused into the first / last kernel

Everything numeric runs in HIP kernels behind cid_esr_* (include/cid.h).  In eval mode BatchNorm uses its running statistics,
folded once per weight upload.  Calling the default module in train mode raises; with batch_stats=True the train-mode forward runs
cid_esr_forward_train (forward only: no autograd history).  There is no CPU fallback.

The server crops this model's UNPADDED output with the padding's offsets (app.py:474-480, while its esrgan branch never pads), which
shifts the image by pad//2 pixels whenever a size is not a multiple of 4.  That is not reproduced: the output here has the input's size.
"""
from __future__ import annotations

from typing import Mapping, Optional, Union

import torch
import torch.nn as nn

from . import _packed
from .discriminator import named_bn_args

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


class ESRGANGenerator(_packed.PackedModule):
    """The reference's ESRGAN generator.  `initial`, `residuals` and `final` are stock layers used as parameter containers, so
    state_dict keys, .to(), load_state_dict(), .train() and .eval() behave as in the reference.  forward(x):
      fp32 [N,3,H,W] in [0,1]  ->  the raw fp32 [N,3,H,W]
      uint8 [N,H,W,3]          ->  uint8 [N,H,W,3], the server's view of the output
    (`out_dtype` picks the other output format for either input),
    asynchronous on the current stream, without autograd history.  Weight changes are found by the tensors' version counters and
    repacked at the next call (after writes through `.data` call pack_weights(force=True)).

    With batch_stats=True forward dispatches on self.training.  Eval mode is the path above.  Train mode normalises every BatchNorm
    with the statistics of the batch and updates running_mean, running_var and num_batches_tracked of the module's own BatchNorm2d
    layers in place on the device, as nn.BatchNorm2d does (eps and momentum, None included, are read from the layers at every
    call).  Its output carries no autograd history either.  The next eval forward folds the updated running statistics again."""

    _abi = "esr"

    def __init__(self, num_residuals: int = 8, batch_stats: bool = False):
        super().__init__()
        if not 0 <= int(num_residuals) <= MAX_RESIDUALS:
            raise ValueError(f"num_residuals must be in [0, {MAX_RESIDUALS}], got {num_residuals}")
        self._batch_stats = bool(batch_stats)
        self._fold_stale = False   # a train forward changed the running statistics behind the tensors' version counters
        self._train_ws = False     # the workspace holds a train forward's tensors (stage)
        self.num_residuals = int(num_residuals)
        self.initial = nn.Sequential(nn.Conv2d(3, 64, 9, 1, 4), nn.PReLU())
        self.residuals = nn.Sequential(*[ResidualBlock(64) for _ in range(self.num_residuals)])
        self.final = nn.Conv2d(64, 3, 9, 1, 4)
        self._create(self.num_residuals)

    def _batchnorms(self):
        return [(f"residuals.{i}.block.{idx}", blk.block[idx], (i, which))
                for i, blk in enumerate(self.residuals) for which, idx in enumerate((1, 4))]

    def pack_weights(self, force: bool = False) -> torch.Tensor:
        """PackedModule.pack_weights; after a train forward the fold of the running statistics is stale and the pack runs again."""
        blob = super().pack_weights(force or self._fold_stale)
        self._fold_stale = False
        return blob

    def forward(self, x: torch.Tensor, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        if self.training and not self._batch_stats:
            raise RuntimeError("ESRGANGenerator is in train mode: train-mode BatchNorm (batch statistics) is not implemented; call "
                               ".eval() first, as the server does (app.py:240)")
        fmt, (n, h, w) = self._image_input(x)
        dev = self._input_device(x)
        if n < 1 or h < 1 or w < 1:
            raise RuntimeError(f"empty input {list(x.shape)}")
        if self.training:
            return self._forward_train(x, fmt, n, h, w, dev, x.dtype if out_dtype is None else out_dtype)
        self.pack_weights()
        self._ensure_workspace(dev, n, h, w)
        x = x.contiguous()
        out_dtype = x.dtype if out_dtype is None else out_dtype
        out_fmt, out = _packed.image_output(out_dtype, n, h, w, dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self._check(self._fn("forward")(self._cid, x.data_ptr(), fmt, out.data_ptr(), out_fmt, n, h, w, self._ws.data_ptr(),
                                             self._ws.numel(), stream))
        self._train_ws = False
        return out

    def _forward_train(self, x, fmt, n, h, w, dev, out_dtype) -> torch.Tensor:
        """cid_esr_forward_train on the module's own BatchNorm2d layers."""
        r = self.num_residuals
        if r and n * h * w == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {torch.Size([n, 64, 1, 1])}")
        bn = named_bn_args([(name, layer) for name, layer, _ in self._batchnorms()], dev)
        # convolution weights and slopes come from the blob; a fold that is already stale stays so until the next eval forward
        _packed.PackedModule.pack_weights(self)
        self._ensure_workspace(dev, n, h, w, r, sizer="train_workspace_bytes")
        x = x.detach().contiguous()
        out_fmt, out = _packed.image_output(out_dtype, n, h, w, dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self._check(self._fn("forward_train")(self._cid, x.data_ptr(), fmt, out.data_ptr(), out_fmt, n, h, w, bn if r else None,
                                                   self._ws.data_ptr(), self._ws.numel(), stream))
        # the kernels wrote the running buffers through raw pointers: no version counter moved, so the pack cannot see it
        self._fold_stale = True
        self._train_ws = True
        return out

    def stage(self, name: str, n: int, h: int, w: int) -> torch.Tensor:
        """What the last forward of an [n,3,h,w] input left in the workspace as fp32 [n,64,h,w] (a copy): "x1", or "tail_in", the
        tensor the last launch read (cid_esr_stage_view; after a train-mode forward cid_esr_train_stage_view)."""
        if self._train_ws:
            return self._stage(n, name, f"input [{n},3,{h},{w}]", n, h, w, self.num_residuals, view="train_stage_view")
        return self._stage(n, name, f"input [{n},3,{h},{w}]", n, h, w)


def load_esrgan(source: Union[str, Mapping, None] = None, num_residuals: int = 8,
                device: Optional[Union[str, torch.device]] = None, strict: bool = False, batch_stats: bool = False) -> ESRGANGenerator:
    """Build an ESRGANGenerator on `device` (default: current GPU) from a checkpoint path (read with the torch-free reader), a
    checkpoint dict or a state_dict: the state_dict is looked up under "generator", "state_dict" and "G" (the server's own loader
    reads checkpoint['G'], app.py:236-241) and "module." prefixes are stripped, as load_state_safely does.  `source=None` keeps the
    default initialisation.  `batch_stats=True` gives the module a train-mode forward (ESRGANGenerator).  Returns the module in eval
    mode."""
    device = _packed.cuda_device(device, "load_esrgan")
    return _packed.load_into(ESRGANGenerator(num_residuals, batch_stats=batch_stats), source, device, strict)


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
