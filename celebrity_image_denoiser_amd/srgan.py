"""The server's third model (`SRGANGenerator`, reference backend/app.py:145-186, the "srgan" branch of /enhance) on the GPU.

    SRGANGenerator(scale_factor=4)            nn.Module with the reference's parameter names (initial.*, res_blocks.i.j.*, mid.*,
                                              upscale.*, final.*, BatchNorm buffers included); forward(x) in eval mode
    SRGANGenerator(4, batch_stats=True)       the same module with a train-mode forward as well: BatchNorm on batch statistics,
                                              running buffers updated in place (the trainer's fake_hr = self.generator(lr_img))
    SRGANGenerator(4, batch_stats=True, autograd=True)   that train-mode forward with autograd history: loss.backward() fills the
                                              .grad of every parameter (cid_sr_forward_saved / cid_sr_backward)
    load_srgan(path_or_state_dict)            -> SRGANGenerator from a checkpoint (its "generator" / "state_dict" / "G" entry)
    super_resolve(model, x)                   fp32 [N,3,H,W] in [-1,1] -> fp32 [N,3,sH,sW] = tanh(.)
    super_resolve_u8(model, u8_nhwc)          uint8 [N,H,W,3] -> uint8 [N,s*Hp,s*Wp,3], the server's branch: pad to a multiple of
                                              4*s -> ToTensor -> Normalize(0.5, 0.5) -> network -> y*0.5+0.5 -> clamp -> ToPILImage,
                                              with padding and both conversions inside the first / last kernel

Everything numeric runs in HIP kernels behind cid_sr_* (include/cid.h).  In eval mode BatchNorm uses its running statistics,
folded once per weight upload.  Calling the default module in train mode raises; with batch_stats=True the train-mode forward runs
cid_sr_forward_train (forward only: no autograd history) and, with autograd=True, the differentiable pair cid_sr_forward_saved /
cid_sr_backward.  There is no CPU fallback.

The server shows this model's whole padded output and crops only the input's picture (app.py:481-485); `crop=True` gives the part of
the output that belongs to the unpadded image instead.
"""
from __future__ import annotations

import ctypes
from typing import Mapping, Optional, Sequence, Union

import torch
import torch.nn as nn

from . import _lib, _packed
from .discriminator import named_bn_args

MAX_SCALE = 8
NUM_BLOCKS = 5


def _stages(scale_factor: int) -> int:
    s = int(scale_factor)
    if s < 1 or s & (s - 1):
        raise ValueError(f"scale_factor must be a power of two (got {scale_factor})")
    if s > MAX_SCALE:
        raise ValueError(f"scale_factor above {MAX_SCALE} is not implemented (got {scale_factor})")
    return s.bit_length() - 1


class SRGANGenerator(_packed.PackedModule):
    """The reference's SRGAN generator.  `initial`, `res_blocks`, `mid`, `upscale` and `final` are stock layers used as parameter
    containers, so state_dict keys, .to(), load_state_dict(), .train() and .eval() behave as in the reference.  forward(x):
      fp32 [N,3,H,W] in [-1,1]  ->  fp32 [N,3,s*Hp,s*Wp] = tanh(.)   (`raw=True`: the sums before tanh)
      uint8 [N,H,W,3]           ->  uint8 [N,s*Hp,s*Wp,3], the server's view of the output
    (`out_dtype` picks the other output format for either input), where `padding` = (left, top, right, bottom) is the server's
    Pad(fill=0) of the input, done as index arithmetic in the first kernel, and Hp x Wp the padded size.  Asynchronous on the current
    stream, without autograd history.  Weight changes are found by the tensors' version counters and repacked at the next call
    (after writes through `.data` call pack_weights(force=True)).

    With batch_stats=True forward dispatches on self.training.  Eval mode is the path above.  Train mode normalises every BatchNorm
    with the statistics of the batch and updates running_mean, running_var and num_batches_tracked of the module's own BatchNorm2d
    layers in place on the device, as nn.BatchNorm2d does (eps and momentum, None included, are read from the layers at every
    call).  It takes no `padding` (the trainer does not pad) and its output carries no autograd history either: it is the fake_hr
    the discriminator step consumes through .detach().  The next eval forward folds the updated running statistics again.

    With autograd=True as well (it needs batch_stats=True) a train-mode forward with an fp32 output records a
    torch.autograd.Function when grad is enabled and a parameter requires grad: forward is cid_sr_forward_saved into a buffer owned
    by that call, backward cid_sr_backward, which gives every parameter that requires grad its gradient (`raw=True` included).
    There is no input gradient (an input with requires_grad gets None), a uint8 output has no history, and eval mode is unchanged."""

    _abi = "sr"

    def __init__(self, scale_factor: int = 4, batch_stats: bool = False, autograd: bool = False):
        super().__init__()
        if autograd and not batch_stats:
            raise ValueError("SRGANGenerator(autograd=True) needs batch_stats=True: the backward pass is the train-mode one "
                             "(BatchNorm on batch statistics); autograd in eval mode is not implemented")
        self._batch_stats = bool(batch_stats)
        self._autograd = bool(autograd)
        self._bws = None           # backward workspace (uint8 tensor, grow-only)
        self._fold_stale = False   # a train forward changed the running statistics behind the tensors' version counters
        self._train_ws = False     # the workspace holds a train forward's tensors (stage)
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
        self._create(self.scale_factor)

    def _batchnorms(self):
        return [(f"res_blocks.{i}.{idx}", blk[idx], (i, which)) for i, blk in enumerate(self.res_blocks) for which, idx in enumerate((1, 4))]

    def pack_weights(self, force: bool = False) -> torch.Tensor:
        """PackedModule.pack_weights; after a train forward the fold of the running statistics is stale and the pack runs again.
        With autograd=True in train mode the pack runs on the device instead (cid_sr_pack_weights_device, one launch, every call:
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
            raise RuntimeError("SRGANGenerator(autograd=True): parameters must be contiguous float32 tensors on one GPU")
        bn = named_bn_args([(name, layer) for name, layer, _ in self._batchnorms()], dev)
        if self._blob is None or self._blob.device != dev:
            self._blob = torch.empty(self._blob_bytes(), dtype=torch.uint8, device=dev)
        self._packed_sig = None    # the host pack's signature no longer describes the blob: the next eval forward packs again
        ptrs = (ctypes.c_void_p * len(params))(*[p.data_ptr() for p in params])
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self._check(self._fn("pack_weights_device")(self._cid, ptrs, bn, self._blob.data_ptr(), stream))
        return self._blob

    def forward(self, x: torch.Tensor, out_dtype: Optional[torch.dtype] = None, raw: bool = False,
                padding: Sequence[int] = (0, 0, 0, 0)) -> torch.Tensor:
        if self.training and not self._batch_stats:
            raise RuntimeError("SRGANGenerator is in train mode: train-mode BatchNorm (batch statistics) is not implemented; call "
                               ".eval() first, as the server does (app.py:273)")
        fmt, (n, h, w) = self._image_input(x)
        dev = self._input_device(x)
        if n < 1 or h < 1 or w < 1:
            raise RuntimeError(f"empty input {list(x.shape)}")
        pl, pt, pr, pb = (int(v) for v in padding)
        if min(pl, pt, pr, pb) < 0 or max(pl, pt, pr, pb) > 4096:
            raise ValueError(f"padding must be four values in [0, 4096] (left, top, right, bottom), got {tuple(padding)}")
        out_dtype = x.dtype if out_dtype is None else out_dtype
        if raw and out_dtype != torch.float32:
            raise ValueError("raw=True gives the fp32 sums before tanh: it needs out_dtype=torch.float32")
        hp, wp, s = h + pt + pb, w + pl + pr, self.scale_factor
        if self.training:
            if (pl, pt, pr, pb) != (0, 0, 0, 0):
                raise ValueError(f"padding is not implemented in train mode (got {tuple(padding)}): the trainer does not pad")
            return self._forward_train(x, fmt, n, h, w, dev, out_dtype, raw)
        self.pack_weights()
        self._ensure_workspace(dev, n, hp, wp, s)
        x = x.contiguous()
        out_fmt, out = _packed.image_output(out_dtype, n, s * hp, s * wp, dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self._check(self._fn("forward")(self._cid, x.data_ptr(), fmt, out.data_ptr(), out_fmt, n, h, w, pl, pt, pr, pb,
                                             _lib.CID_SR_RAW if raw else 0, self._ws.data_ptr(), self._ws.numel(), stream))
        self._train_ws = False
        return out

    def _forward_train(self, x, fmt, n, h, w, dev, out_dtype, raw) -> torch.Tensor:
        """cid_sr_forward_train on the module's own BatchNorm2d layers."""
        if n * h * w == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {torch.Size([n, 64, 1, 1])}")
        bn = named_bn_args([(name, layer) for name, layer, _ in self._batchnorms()], dev)
        # convolution weights and slopes come from the blob; a fold that is already stale stays so until the next eval forward
        if self._autograd:
            self._pack_device()
        else:
            _packed.PackedModule.pack_weights(self)
        s = self.scale_factor
        self._ensure_workspace(dev, n, h, w, s, sizer="train_workspace_bytes")
        if (self._autograd and out_dtype == torch.float32 and torch.is_grad_enabled()
                and any(p.requires_grad for p in self.parameters())):
            out = _SrFunction.apply(self, fmt, (n, h, w), bool(raw), bn, x, *self.parameters())
            self._fold_stale = True
            self._train_ws = True
            return out
        x = x.detach().contiguous()
        out_fmt, out = _packed.image_output(out_dtype, n, s * h, s * w, dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self._check(self._fn("forward_train")(self._cid, x.data_ptr(), fmt, out.data_ptr(), out_fmt, n, h, w,
                                                   _lib.CID_SR_RAW if raw else 0, bn, self._ws.data_ptr(), self._ws.numel(), stream))
        # the kernels wrote the running buffers through raw pointers: no version counter moved, so the pack cannot see it
        self._fold_stale = True
        self._train_ws = True
        return out

    def stage(self, name: str, n: int, hp: int, wp: int) -> torch.Tensor:
        """What the last forward over a padded [n,3,hp,wp] input left in the workspace, as fp32 [n,64,Hs,Ws] (a copy): "x0", "trunk",
        "up1", or "tail_in", the tensor the last launch read (cid_sr_stage_view)."""
        return self._stage(n, name, f"input [{n},3,{hp},{wp}]", n, hp, wp, self.scale_factor,
                           view="train_stage_view" if self._train_ws else "stage_view")


class _GradsArg(ctypes.Structure):
    """cid_sr_grads (include/cid.h)."""
    _fields_ = [("head_w", ctypes.c_void_p), ("head_b", ctypes.c_void_p), ("head_slope", ctypes.c_void_p),
                ("conv_w", ctypes.c_void_p * 10), ("conv_b", ctypes.c_void_p * 10), ("gamma", ctypes.c_void_p * 10),
                ("beta", ctypes.c_void_p * 10), ("slope", ctypes.c_void_p * NUM_BLOCKS), ("mid_w", ctypes.c_void_p),
                ("mid_b", ctypes.c_void_p), ("up_w", ctypes.c_void_p * 3), ("up_b", ctypes.c_void_p * 3),
                ("up_slope", ctypes.c_void_p * 3), ("final_w", ctypes.c_void_p), ("final_b", ctypes.c_void_p)]


def _set_grad(g: _GradsArg, name: str, ptr: int) -> None:
    """Put the gradient tensor of parameter `name` into its slot of cid_sr_grads."""
    parts = name.split(".")
    weight = parts[-1] == "weight"
    if parts[0] == "initial":
        setattr(g, "head_slope" if parts[1] == "1" else ("head_w" if weight else "head_b"), ptr)
    elif parts[0] == "res_blocks":
        i, j = int(parts[1]), int(parts[2])
        if j == 2:
            g.slope[i] = ptr
        elif j in (0, 3):
            (g.conv_w if weight else g.conv_b)[2 * i + (j == 3)] = ptr
        else:
            (g.gamma if weight else g.beta)[2 * i + (j == 4)] = ptr
    elif parts[0] == "upscale":
        k, j = divmod(int(parts[1]), 3)
        if j == 2:
            g.up_slope[k] = ptr
        else:
            (g.up_w if weight else g.up_b)[k] = ptr
    else:
        setattr(g, ("mid_" if parts[0] == "mid" else "final_") + ("w" if weight else "b"), ptr)


class _SrFunction(torch.autograd.Function):
    """forward = cid_sr_forward_saved into a buffer owned by this call's context, backward = cid_sr_backward."""

    @staticmethod
    def forward(ctx, module, fmt, shape, raw, bn, x, *params):
        n, h, w = shape
        dev = x.device
        L = _lib.lib()
        s = module.scale_factor
        need = ctypes.c_size_t()
        module._check(L.cid_sr_saved_bytes(n, h, w, s, ctypes.byref(need)))
        saved = torch.empty(need.value, dtype=torch.uint8, device=dev)
        xc = x.detach().contiguous()
        out = torch.empty((n, 3, s * h, s * w), dtype=torch.float32, device=dev)
        flags = _lib.CID_SR_RAW if raw else 0
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            module._check(L.cid_sr_forward_saved(module._cid, xc.data_ptr(), fmt, out.data_ptr(), n, h, w, flags, bn, saved.data_ptr(),
                                                 saved.numel(), module._ws.data_ptr(), module._ws.numel(), stream))
        ctx.module, ctx.fmt, ctx.shape, ctx.flags = module, fmt, shape, flags
        ctx.saved, ctx.x = saved, xc
        ctx.names = [k for k, _ in module.named_parameters()]
        ctx.versions = [p._version for p in params]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        module = ctx.module
        if ctx.saved is None:
            raise RuntimeError("SRGANGenerator: this call's saved activations were released by its first backward")
        params = list(module.parameters())
        for name, p, v in zip(ctx.names, params, ctx.versions):
            if p._version != v:
                raise RuntimeError(f"SRGANGenerator: parameter {name} was modified in place between a forward and its backward "
                                   f"(version {p._version}, expected {v}); the gradient would be taken at the wrong weights")
        n, h, w = ctx.shape
        dev = ctx.x.device
        L = _lib.lib()
        needs = ctx.needs_input_grad
        g = _GradsArg()
        grads = [None] * len(params)
        for i, (name, p) in enumerate(zip(ctx.names, params)):
            if needs[6 + i]:
                grads[i] = torch.empty(p.shape, dtype=torch.float32, device=dev)
                _set_grad(g, name, grads[i].data_ptr())
        need = ctypes.c_size_t()
        module._check(L.cid_sr_backward_workspace_bytes(n, h, w, module.scale_factor, ctypes.byref(need)))
        if module._bws is None or module._bws.numel() < need.value or module._bws.device != dev:
            module._bws = None
            module._bws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        go = grad_out.to(torch.float32).contiguous()
        bn = named_bn_args([(name, layer) for name, layer, _ in module._batchnorms()], dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            module._check(L.cid_sr_backward(module._cid, ctx.x.data_ptr(), ctx.fmt, go.data_ptr(), n, h, w, ctx.flags, bn,
                                            ctx.saved.data_ptr(), ctx.saved.numel(), ctypes.byref(g), module._bws.data_ptr(),
                                            module._bws.numel(), stream))
        ctx.saved = None
        return (None, None, None, None, None, None, *grads)


def load_srgan(source: Union[str, Mapping, None] = None, scale_factor: int = 4,
               device: Optional[Union[str, torch.device]] = None, strict: bool = False, batch_stats: bool = False,
               autograd: bool = False) -> SRGANGenerator:
    """Build an SRGANGenerator on `device` (default: current GPU) from a checkpoint path (read with the torch-free reader), a
    checkpoint dict or a state_dict: the state_dict is looked up under "generator", "state_dict" and "G" and "module." prefixes are
    stripped, as load_state_safely does (app.py:257-274).  `source=None` keeps the default initialisation.  `batch_stats=True` gives
    the module a train-mode forward, `autograd=True` with it a differentiable one (SRGANGenerator).  Returns the module in eval mode."""
    device = _packed.cuda_device(device, "load_srgan")
    return _packed.load_into(SRGANGenerator(scale_factor, batch_stats=batch_stats, autograd=autograd), source, device, strict)


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
