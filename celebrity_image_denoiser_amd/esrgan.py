"""The server's second model (`ESRGANGenerator`, reference backend/app.py:188-218, the "esrgan" branch of /enhance, :387-397) on the GPU.

    ESRGANGenerator(num_residuals=8)          nn.Module with the reference's parameter names (initial.*, residuals.i.block.*, final.*,
                                              BatchNorm buffers included); forward(x) in eval mode
    ESRGANGenerator(8, batch_stats=True)      the same module with a train-mode forward as well: BatchNorm on batch statistics,
                                              running buffers updated in place (the trainer's denoised = G(noisy) after G.train())
    ESRGANGenerator(8, batch_stats=True, autograd=True)   that train-mode forward with autograd history: g_loss.backward() fills the
                                              .grad of every parameter (cid_esr_forward_saved / cid_esr_backward)
    load_esrgan(path_or_state_dict)           -> ESRGANGenerator from a checkpoint (its "generator" / "state_dict" / "G" entry)
    enhance(model, x)                         fp32 [N,3,H,W] in [0,1] -> the raw fp32 output [N,3,H,W] (no tanh, no clamp)
    enhance_u8(model, u8_nhwc)                uint8 [N,H,W,3] -> uint8 [N,H,W,3]: ToTensor() in, clamp(0,1) -> ToPILImage out
                                              (preprocess_image / postprocess_tensor, app.py:243-254), fused into the first / last kernel

Everything numeric runs in HIP kernels behind cid_esr_* (include/cid.h).  In eval mode BatchNorm uses its running statistics,
folded once per weight upload.  Calling the default module in train mode raises; with batch_stats=True the train-mode forward runs
cid_esr_forward_train (forward only: no autograd history) and, with autograd=True, the differentiable pair cid_esr_forward_saved /
cid_esr_backward.  There is no CPU fallback.

The server crops this model's UNPADDED output with the padding's offsets (app.py:474-480, while its esrgan branch never pads), which
shifts the image by pad//2 pixels whenever a size is not a multiple of 4.  That is not reproduced: the output here has the input's size.
"""
from __future__ import annotations

import ctypes
from typing import Mapping, Optional, Union

import torch
import torch.nn as nn

from . import _lib, _packed
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
    call).  Its output carries no autograd history either.  The next eval forward folds the updated running statistics again.

    With autograd=True as well (it needs batch_stats=True) a train-mode forward with an fp32 output records a
    torch.autograd.Function when grad is enabled and a parameter requires grad: forward is cid_esr_forward_saved into a buffer owned
    by that call, backward cid_esr_backward, which gives every parameter that requires grad its gradient.  There is no input
    gradient (an input with requires_grad gets None), a uint8 output has no history, and eval mode is unchanged."""

    _abi = "esr"

    def __init__(self, num_residuals: int = 8, batch_stats: bool = False, autograd: bool = False):
        super().__init__()
        if not 0 <= int(num_residuals) <= MAX_RESIDUALS:
            raise ValueError(f"num_residuals must be in [0, {MAX_RESIDUALS}], got {num_residuals}")
        if autograd and not batch_stats:
            raise ValueError("ESRGANGenerator(autograd=True) needs batch_stats=True: the backward pass is the train-mode one "
                             "(BatchNorm on batch statistics); autograd in eval mode is not implemented")
        self._batch_stats = bool(batch_stats)
        self._autograd = bool(autograd)
        self._bws = None           # backward workspace (uint8 tensor, grow-only)
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
        """PackedModule.pack_weights; after a train forward the fold of the running statistics is stale and the pack runs again.
        With autograd=True in train mode the pack runs on the device instead (cid_esr_pack_weights_device, one launch, every call:
        a trainer changes the weights at every step) into one blob that stays in place."""
        if self._autograd and self.training:
            return self._pack_device()
        blob = super().pack_weights(force or self._fold_stale)
        self._fold_stale = False
        return blob

    def _pack_device(self) -> torch.Tensor:
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs only on an AMD GPU (HIP kernels behind libcid.so); move it with "
                               ".to('cuda') first. There is no CPU fallback.")
        params = list(self.parameters())
        if any(p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev for p in params):
            raise RuntimeError("ESRGANGenerator(autograd=True): parameters must be contiguous float32 tensors on one GPU")
        bn = self._bn_args(dev)
        if self._blob is None or self._blob.device != dev:
            self._blob = torch.empty(self._blob_bytes(), dtype=torch.uint8, device=dev)
        self._packed_sig = None    # the host pack's signature no longer describes the blob: the next eval forward packs again
        ptrs = (ctypes.c_void_p * len(params))(*[p.data_ptr() for p in params])
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self._check(self._fn("pack_weights_device")(self._cid, ptrs, bn, self._blob.data_ptr(), stream))
        return self._blob

    def _bn_args(self, dev):
        """The cid_disc_bn array of the module's own BatchNorm2d layers; None where there is no block."""
        return named_bn_args([(name, layer) for name, layer, _ in self._batchnorms()], dev) if self.num_residuals else None

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
        bn = self._bn_args(dev)
        # convolution weights and slopes come from the blob; a fold that is already stale stays so until the next eval forward
        if self._autograd:
            self._pack_device()
        else:
            _packed.PackedModule.pack_weights(self)
        self._ensure_workspace(dev, n, h, w, r, sizer="train_workspace_bytes")
        if (self._autograd and out_dtype == torch.float32 and torch.is_grad_enabled()
                and any(p.requires_grad for p in self.parameters())):
            out = _EsrFunction.apply(self, fmt, (n, h, w), bn, x, *self.parameters())
            self._fold_stale = True
            self._train_ws = True
            return out
        x = x.detach().contiguous()
        out_fmt, out = _packed.image_output(out_dtype, n, h, w, dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self._check(self._fn("forward_train")(self._cid, x.data_ptr(), fmt, out.data_ptr(), out_fmt, n, h, w, bn,
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


class _GradsArg(ctypes.Structure):
    """cid_esr_grads (include/cid.h)."""
    _fields_ = [("head_w", ctypes.c_void_p), ("head_b", ctypes.c_void_p), ("head_slope", ctypes.c_void_p),
                ("conv_w", ctypes.c_void_p * (2 * MAX_RESIDUALS)), ("conv_b", ctypes.c_void_p * (2 * MAX_RESIDUALS)),
                ("gamma", ctypes.c_void_p * (2 * MAX_RESIDUALS)), ("beta", ctypes.c_void_p * (2 * MAX_RESIDUALS)),
                ("slope", ctypes.c_void_p * MAX_RESIDUALS), ("final_w", ctypes.c_void_p), ("final_b", ctypes.c_void_p)]


def _set_grad(g: _GradsArg, name: str, ptr: int) -> None:
    """Put the gradient tensor of parameter `name` into its slot of cid_esr_grads."""
    parts = name.split(".")
    weight = parts[-1] == "weight"
    if parts[0] == "initial":
        setattr(g, "head_slope" if parts[1] == "1" else ("head_w" if weight else "head_b"), ptr)
    elif parts[0] == "residuals":
        i, j = int(parts[1]), int(parts[3])
        if j == 2:
            g.slope[i] = ptr
        elif j in (0, 3):
            (g.conv_w if weight else g.conv_b)[2 * i + (j == 3)] = ptr
        else:
            (g.gamma if weight else g.beta)[2 * i + (j == 4)] = ptr
    else:
        setattr(g, "final_w" if weight else "final_b", ptr)


class _EsrFunction(torch.autograd.Function):
    """forward = cid_esr_forward_saved into a buffer owned by this call's context, backward = cid_esr_backward."""

    @staticmethod
    def forward(ctx, module, fmt, shape, bn, x, *params):
        n, h, w = shape
        dev = x.device
        L = _lib.lib()
        need = ctypes.c_size_t()
        module._check(L.cid_esr_saved_bytes(n, h, w, module.num_residuals, ctypes.byref(need)))
        saved = torch.empty(need.value, dtype=torch.uint8, device=dev)
        xc = x.detach().contiguous()
        out = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            module._check(L.cid_esr_forward_saved(module._cid, xc.data_ptr(), fmt, out.data_ptr(), n, h, w, bn, saved.data_ptr(),
                                                  saved.numel(), module._ws.data_ptr(), module._ws.numel(), stream))
        ctx.module, ctx.fmt, ctx.shape = module, fmt, shape
        ctx.saved, ctx.x = saved, xc
        ctx.names = [k for k, _ in module.named_parameters()]
        ctx.versions = [p._version for p in params]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        module = ctx.module
        if ctx.saved is None:
            raise RuntimeError("ESRGANGenerator: this call's saved activations were released by its first backward")
        params = list(module.parameters())
        for name, p, v in zip(ctx.names, params, ctx.versions):
            if p._version != v:
                raise RuntimeError(f"ESRGANGenerator: parameter {name} was modified in place between a forward and its backward "
                                   f"(version {p._version}, expected {v}); the gradient would be taken at the wrong weights")
        n, h, w = ctx.shape
        dev = ctx.x.device
        L = _lib.lib()
        needs = ctx.needs_input_grad
        g = _GradsArg()
        grads = [None] * len(params)
        for i, (name, p) in enumerate(zip(ctx.names, params)):
            if needs[5 + i]:
                grads[i] = torch.empty(p.shape, dtype=torch.float32, device=dev)
                _set_grad(g, name, grads[i].data_ptr())
        need = ctypes.c_size_t()
        module._check(L.cid_esr_backward_workspace_bytes(n, h, w, module.num_residuals, ctypes.byref(need)))
        if module._bws is None or module._bws.numel() < need.value or module._bws.device != dev:
            module._bws = None
            module._bws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        go = grad_out.to(torch.float32).contiguous()
        bn = module._bn_args(dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            module._check(L.cid_esr_backward(module._cid, ctx.x.data_ptr(), ctx.fmt, go.data_ptr(), n, h, w, bn, ctx.saved.data_ptr(),
                                             ctx.saved.numel(), ctypes.byref(g), module._bws.data_ptr(), module._bws.numel(), stream))
        ctx.saved = None
        return (None, None, None, None, None, *grads)


def load_esrgan(source: Union[str, Mapping, None] = None, num_residuals: int = 8,
                device: Optional[Union[str, torch.device]] = None, strict: bool = False, batch_stats: bool = False,
                autograd: bool = False) -> ESRGANGenerator:
    """Build an ESRGANGenerator on `device` (default: current GPU) from a checkpoint path (read with the torch-free reader), a
    checkpoint dict or a state_dict: the state_dict is looked up under "generator", "state_dict" and "G" (the server's own loader
    reads checkpoint['G'], app.py:236-241) and "module." prefixes are stripped, as load_state_safely does.  `source=None` keeps the
    default initialisation.  `batch_stats=True` gives the module a train-mode forward, `autograd=True` with it a differentiable one
    (ESRGANGenerator).  Returns the module in eval mode."""
    device = _packed.cuda_device(device, "load_esrgan")
    return _packed.load_into(ESRGANGenerator(num_residuals, batch_stats=batch_stats, autograd=autograd), source, device, strict)


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
