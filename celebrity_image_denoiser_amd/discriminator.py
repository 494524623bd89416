"""The trainer's discriminator (`DenoiseDiscriminator`, reference backend/trainingcode/denoise_gan_code/training.py:77-98) on the GPU.

    DenoiseDiscriminator(autograd=False)     nn.Module with the reference's parameter names (model.0 ... model.12, BatchNorm buffers
                                             included); forward(x) -> fp32 [N] probabilities, eval or train mode
    load_discriminator(path_or_state_dict)   -> DenoiseDiscriminator from the "discriminator" entry of a trainer checkpoint
    trainer_losses(D, denoised, clean)       -> the trainer's d_loss / g_loss / content_loss / adv_loss of one batch

Everything numeric runs in HIP kernels behind cid_disc_* (include/cid.h).  By default the module is forward only: the output carries
no autograd history, so the trainer's d_loss.backward() on it raises torch's own "does not require grad" error.  With autograd=True
the forward records a torch.autograd.Function whose backward is cid_disc_backward: the trainer's discriminator step
(training.py:410-417) and the adversarial half of its generator step (:421-425) then run on these kernels, with a stock
torch.optim optimizer doing the update.  No double backward.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Mapping, Optional, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib, _packed


class _BnArg(ctypes.Structure):
    """cid_disc_bn (include/cid.h)."""
    _fields_ = [("gamma", ctypes.c_void_p), ("beta", ctypes.c_void_p), ("running_mean", ctypes.c_void_p),
                ("running_var", ctypes.c_void_p), ("num_batches_tracked", ctypes.c_void_p), ("eps", ctypes.c_double),
                ("momentum", ctypes.c_double)]


def _grads_arg(convs: int, bns: int):
    """cid_disc_grads / cid_srd_grads (include/cid.h): the struct of a discriminator with that many convolutions and BatchNorms."""
    class _GradsArg(ctypes.Structure):
        _fields_ = [("w", ctypes.c_void_p * convs), ("b", ctypes.c_void_p * convs), ("gamma", ctypes.c_void_p * bns),
                    ("beta", ctypes.c_void_p * bns), ("input", ctypes.c_void_p)]
    return _GradsArg()


def _out_side(s: int) -> int:
    return (s - 1) // 2 + 1


def bn_args(model: nn.Sequential, indices, dev: torch.device):
    """The cid_disc_bn array of the BatchNorm2d containers model[i], i in `indices` (named_bn_args)."""
    return named_bn_args([(f"model.{idx}", model[idx]) for idx in indices], dev)


def named_bn_args(named, dev: torch.device):
    """The cid_disc_bn array of the (name, BatchNorm2d) pairs `named`, whose tensors live on `dev`: device pointers of the affine
    parameters, the running buffers and the counter, with eps and momentum as the containers hold them now."""
    arr = (_BnArg * len(named))()
    for i, (name, bn) in enumerate(named):
        if not (bn.affine and bn.track_running_stats):
            raise NotImplementedError(f"{name}: only BatchNorm2d(affine=True, track_running_stats=True) is supported")
        ts = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
        if any(t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() for t in ts):
            raise RuntimeError(f"{name}: BatchNorm tensors must be contiguous float32 on {dev}")
        nbt = bn.num_batches_tracked
        if nbt.device != dev or nbt.dtype != torch.int64:
            raise RuntimeError(f"{name}.num_batches_tracked must be int64 on {dev}")
        mom = bn.momentum
        arr[i] = _BnArg(bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                        nbt.data_ptr(), float(bn.eps), _lib.CID_DISC_MOMENTUM_NONE if mom is None else float(mom))
        if mom is not None and (not np.isfinite(mom) or mom < 0):
            raise ValueError(f"{name}.momentum must be finite and >= 0 or None, got {mom}")
        if not np.isfinite(bn.eps) or bn.eps < 0:
            raise ValueError(f"{name}.eps must be finite and >= 0, got {bn.eps}")
    return arr


def device_pack(module, what: str, force: bool = False) -> torch.Tensor:
    """pack_weights() of a differentiable module (the BatchNorm discriminators, ESRGANDiscriminator): the tensors of
    `module._tensors()`, in that order, repacked by cid_<abi>_pack_weights_device on the module's GPU into one blob that stays in
    place (if they changed since the last call).  `what` names the tensors in the error text."""
    sig = module._signature()
    if not force and module._blob is not None and sig == module._packed_sig:
        return module._blob
    dev = module._device()
    if dev.type != "cuda":
        raise RuntimeError(f"{type(module).__name__} runs only on an AMD GPU (HIP kernels behind libcid.so); move it with "
                           ".to('cuda') first. There is no CPU fallback.")
    ts = [t.detach() for _, t in module._tensors()]
    if any(t.dtype != torch.float32 or t.device != dev for t in ts):
        raise RuntimeError(f"{type(module).__name__}: {what} must be float32 on {dev}")
    ts = [t.contiguous() for t in ts]
    if module._blob is None or module._blob.device != dev:
        module._blob = torch.empty(module._blob_bytes(), dtype=torch.uint8, device=dev)
    ptrs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        module._check(module._fn("pack_weights_device")(module._cid, ptrs, module._blob.data_ptr(), stream))
    module._packed_sig = sig
    return module._blob


class BatchNormDiscriminator(_packed.PackedModule):
    """What DenoiseDiscriminator and SRGANDiscriminator (srgan_disc.py) share: a Sequential `self.model` of stock layers whose
    convolutions `_CONVS` are packed into the blob and whose BatchNorms `_BNS` are call arguments (indices into the Sequential).
    A subclass sets `_abi` and the two tuples, builds `self.model`, calls `_create()`, and names the BatchNorm that first sees a
    single value (`_single_value_channels`).
    forward dispatches on self.training:
      eval   BatchNorm with the running buffers;
      train  BatchNorm with batch statistics, and the running buffers and num_batches_tracked are updated in place on the device,
             as nn.BatchNorm2d does (momentum and eps are read from the containers at every call).
    The forward is asynchronous on the current stream.  With autograd=False (the default) it carries no autograd history.  With
    autograd=True, grad mode on and a parameter or the input requiring grad, it is differentiable once: each call keeps its own
    activations (cid_<abi>_saved_bytes per call) until its backward has run, and weight changes are repacked on the device."""

    _CONVS = ()
    _BNS = ()

    def __init__(self, autograd: bool = False):
        super().__init__()
        self._autograd = bool(autograd)
        self._bws = None           # backward workspace (uint8 tensor, grow-only)

    # ------------------------------------------------------------------ weights
    def _tensors(self):
        # the convolution tensors; the BatchNorm tensors are call arguments.  p._version counts in-place updates made through the
        # tensor API; after writes through `p.data` call pack_weights(force=True)
        return [(f"model.{i}.{kind}", getattr(self.model[i], kind)) for i in self._CONVS for kind in ("weight", "bias")]

    def _blob_bytes(self) -> int:
        return self._fn("packed_weights_bytes")()

    def pack_weights(self, force: bool = False) -> torch.Tensor:
        """Repack the convolution tensors into the kernels' layout on the module's GPU (if they changed since the last call).
        With autograd=True the pack runs on the device, into one blob that stays in place: a training loop changes the weights at
        every step."""
        if not self._autograd:
            return super().pack_weights(force)
        return device_pack(self, "convolution parameters", force)

    # ------------------------------------------------------------------ forward
    def _bn_args(self, dev: torch.device):
        return bn_args(self.model, self._BNS, dev)

    def _single_value_channels(self, h: int, w: int) -> int:
        """Channels of the first BatchNorm that sees one value per channel, for an N = 1 input whose last map is 1 x 1."""
        raise NotImplementedError

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """fp32 [N,3,H,W] in [-1,1] or uint8 [N,H,W,3] on the GPU -> fp32 [N] probabilities on the same GPU (the reference's
        forward).  In train mode the BatchNorm running buffers are updated in place."""
        fmt, (n, h, w) = self._image_input(x)
        dev = self._input_device(x)
        if n < 1 or h < 1 or w < 1:
            raise RuntimeError(f"empty input {list(x.shape)}")
        training = self.training
        if training and n * _out_side(_out_side(h)) * _out_side(_out_side(w)) == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size "
                             f"{torch.Size([n, self._single_value_channels(h, w), 1, 1])}")
        bn = self._bn_args(dev)
        self.pack_weights()
        if self._autograd and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return _DiscFunction.apply(self, fmt, (n, h, w), training, x, *self.parameters())
        self._ensure_workspace(dev, n, h, w, int(training))
        x = x.detach().contiguous()
        out = torch.empty(n, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self._check(self._fn("forward")(self._cid, x.data_ptr(), fmt, out.data_ptr(), n, h, w, bn, int(training),
                                            self._ws.data_ptr(), self._ws.numel(), stream))
        return out


class _DiscFunction(torch.autograd.Function):
    """forward = cid_<abi>_forward_saved into a buffer owned by this call's context, backward = cid_<abi>_backward, for a
    BatchNormDiscriminator `module`."""

    @staticmethod
    def forward(ctx, module, fmt, shape, training, x, *params):
        n, h, w = shape
        dev = x.device
        need = ctypes.c_size_t()
        module._check(module._fn("saved_bytes")(n, h, w, int(training), ctypes.byref(need)))
        saved = torch.empty(need.value, dtype=torch.uint8, device=dev)
        xc = x.detach().contiguous()
        out = torch.empty(n, dtype=torch.float32, device=dev)
        bn = module._bn_args(dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            module._check(module._fn("forward_saved")(module._cid, xc.data_ptr(), fmt, out.data_ptr(), n, h, w, bn, int(training),
                                                      saved.data_ptr(), saved.numel(), stream))
        ctx.module, ctx.fmt, ctx.shape, ctx.training = module, fmt, shape, training
        ctx.saved, ctx.x = saved, xc
        ctx.names = [k for k, _ in module.named_parameters()]
        ctx.versions = [p._version for p in params]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_prob):
        module = ctx.module
        convs, bns = module._CONVS, module._BNS
        params = list(module.parameters())
        for name, p, v in zip(ctx.names, params, ctx.versions):
            if p._version != v:
                raise RuntimeError(f"{type(module).__name__}: parameter {name} was modified in place between a forward and its "
                                   f"backward (version {p._version}, expected {v}); the gradient would be taken at the wrong weights")
        n, h, w = ctx.shape
        dev = ctx.x.device
        needs = ctx.needs_input_grad
        g = _grads_arg(len(convs), len(bns))
        grads = [None] * len(params)
        for i, (name, p) in enumerate(zip(ctx.names, params)):
            if not needs[5 + i]:
                continue
            grads[i] = torch.empty(p.shape, dtype=torch.float32, device=dev)
            idx, kind = int(name.split(".")[1]), name.rsplit(".", 1)[1]
            if idx in convs:
                (g.w if kind == "weight" else g.b)[convs.index(idx)] = grads[i].data_ptr()
            else:
                (g.gamma if kind == "weight" else g.beta)[bns.index(idx)] = grads[i].data_ptr()
        grad_x = None
        if needs[4] and ctx.fmt == _lib.CID_FMT_F32_NCHW:
            grad_x = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
            g.input = grad_x.data_ptr()
        need = ctypes.c_size_t()
        module._check(module._fn("backward_workspace_bytes")(n, h, w, int(ctx.training), ctypes.byref(need)))
        if module._bws is None or module._bws.numel() < need.value or module._bws.device != dev:
            module._bws = None
            module._bws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        gp = grad_prob.to(torch.float32).contiguous()
        bn = module._bn_args(dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            module._check(module._fn("backward")(module._cid, ctx.x.data_ptr(), ctx.fmt, gp.data_ptr(), n, h, w, bn, int(ctx.training),
                                                 ctx.saved.data_ptr(), ctx.saved.numel(), ctypes.byref(g), module._bws.data_ptr(),
                                                 module._bws.numel(), stream))
        ctx.saved = None
        return (None, None, None, None, grad_x, *grads)


class DenoiseDiscriminator(BatchNormDiscriminator):
    """The reference's discriminator (BatchNormDiscriminator: state_dict keys, .to(), load_state_dict(), .train() and .eval() behave
    as in the reference; train mode updates model.3 / model.6 / model.9 in place)."""

    _abi = "disc"
    _CONVS = (0, 2, 5, 8, 12)
    _BNS = (3, 6, 9)

    def __init__(self, autograd: bool = False):
        super().__init__(autograd)
        self.model = nn.Sequential(
            nn.Conv2d(3, 64, kernel_size=3, padding=1),
            nn.LeakyReLU(0.2),
            nn.Conv2d(64, 64, kernel_size=3, stride=2, padding=1),
            nn.BatchNorm2d(64),
            nn.LeakyReLU(0.2),
            nn.Conv2d(64, 128, kernel_size=3, padding=1),
            nn.BatchNorm2d(128),
            nn.LeakyReLU(0.2),
            nn.Conv2d(128, 128, kernel_size=3, stride=2, padding=1),
            nn.BatchNorm2d(128),
            nn.LeakyReLU(0.2),
            nn.AdaptiveAvgPool2d(1),
            nn.Conv2d(128, 1, kernel_size=1),
            nn.Sigmoid(),
        )
        self._create()

    def _single_value_channels(self, h: int, w: int) -> int:
        return 128


def load_discriminator(source: Union[str, Mapping, None] = None, device: Optional[Union[str, torch.device]] = None,
                       strict: bool = False, autograd: bool = False) -> DenoiseDiscriminator:
    """Build a DenoiseDiscriminator on `device` (default: current GPU) from a trainer checkpoint path (its "discriminator" entry,
    training.py:362, read with the torch-free reader), a checkpoint dict or a state_dict; "module." prefixes are stripped as for
    the generator.  `source=None` keeps the default initialisation.  `autograd=True` makes the forward differentiable
    (DenoiseDiscriminator).  Returns the module in eval mode."""
    device = _packed.cuda_device(device, "load_discriminator")
    return _packed.load_into(DenoiseDiscriminator(autograd=autograd), source, device, strict, key_candidates=("discriminator",))


def _image_operand(x: torch.Tensor, what: str):
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise RuntimeError(f"{what}: expected fp32 [N,3,H,W] or uint8 [N,H,W,3]")
    if x.dtype == torch.float32 and x.shape[1] == 3:
        return x.contiguous(), _lib.CID_FMT_F32_NCHW, (x.shape[0], x.shape[2], x.shape[3])
    if x.dtype == torch.uint8 and x.shape[3] == 3:
        return x.contiguous(), _lib.CID_FMT_U8_NHWC, (x.shape[0], x.shape[1], x.shape[2])
    raise RuntimeError(f"{what}: expected fp32 [N,3,H,W] or uint8 [N,H,W,3], got {x.dtype} {list(x.shape)}")


def trainer_losses(discriminator: DenoiseDiscriminator, denoised: torch.Tensor, clean: torch.Tensor) -> dict:
    """The trainer's losses of one batch (training.py:412-424) -> {"d_loss", "g_loss", "content_loss", "adv_loss"} as floats:
        p_real = D(clean), p_fake = D(denoised)
        d_loss = BCE(p_real, 1) + BCE(p_fake, 0)      content_loss = MSE(denoised, clean)
        adv_loss = BCE(p_fake, 1)                     g_loss = content_loss + 0.001 * adv_loss
    BCE clamps its logs at -100 as nn.BCELoss does; the reductions run in one HIP kernel in fp64 (one device-to-host copy).
    Each operand is fp32 [N,3,H,W] in [-1,1] or uint8 [N,H,W,3] (read as the forward reads it).  Two differences from the trainer:
    D is evaluated twice at its current weights (the trainer evaluates :421 after D's optimizer step), and in train mode each of
    the two calls updates the BatchNorm running statistics."""
    den, fd, sd = _image_operand(denoised, "denoised")
    cln, fc, sc = _image_operand(clean, "clean")
    if sd != sc:
        raise RuntimeError(f"denoised and clean differ in size: {sd} vs {sc}")
    if den.device != cln.device or den.device.type != "cuda":
        raise RuntimeError("trainer_losses: both batches must be on the discriminator's GPU")
    p_real = discriminator(cln)
    p_fake = discriminator(den)
    out = torch.empty(4, dtype=torch.float64, device=den.device)
    n, h, w = sd
    with torch.cuda.device(den.device):
        stream = torch.cuda.current_stream(den.device).cuda_stream
        _lib.check(None, _lib.lib().cid_disc_losses(p_real.data_ptr(), p_fake.data_ptr(), den.data_ptr(), fd, cln.data_ptr(), fc,
                                                     n, h, w, out.data_ptr(), stream))
    d_loss, g_loss, content, adv = out.cpu().tolist()
    return {"d_loss": d_loss, "g_loss": g_loss, "content_loss": content, "adv_loss": adv}
