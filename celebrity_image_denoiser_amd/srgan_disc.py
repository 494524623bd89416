"""The SRGAN trainer's discriminator (`SRGANDiscriminator`, reference backend/trainingcode/srgan_code/sr_ganTrainGNew.py:54-80) on the GPU.

    SRGANDiscriminator(autograd=False)         nn.Module with the reference's parameter names (model.0 ... model.17, BatchNorm
                                               buffers included); forward(x) -> fp32 [N] probabilities, eval or train mode
    load_srgan_discriminator(path_or_sd)       -> SRGANDiscriminator from the "discriminator" entry of an SRGAN trainer checkpoint
    srgan_trainer_losses(D, fake_hr, hr_img)   -> the trainer's d_loss / adv_loss (and, with a VGGPerceptualLoss, content_loss / g_loss)

Everything numeric runs in HIP kernels behind cid_srd_* (include/cid.h).  By default the module is forward only: the output carries
no autograd history, so the trainer's d_loss.backward() on it raises torch's own "does not require grad" error.  With autograd=True
the forward records a torch.autograd.Function whose backward is cid_srd_backward: the trainer's discriminator step
(sr_ganTrainGNew.py:393-400) and the adversarial half of its generator step (:403-409) then run on these kernels, with a stock
torch.optim optimizer or cid.Adam doing the update.  No double backward.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Mapping, Optional, Union

import torch
import torch.nn as nn

from . import _lib, _packed
from .discriminator import _out_side, bn_args

_CONVS = (0, 2, 5, 8, 11, 15, 17)
_BNS = (3, 6, 9, 12)


class _GradsArg(ctypes.Structure):
    """cid_srd_grads (include/cid.h)."""
    _fields_ = [("w", ctypes.c_void_p * 7), ("b", ctypes.c_void_p * 7), ("gamma", ctypes.c_void_p * 4),
                ("beta", ctypes.c_void_p * 4), ("input", ctypes.c_void_p)]


class SRGANDiscriminator(_packed.PackedModule):
    """The reference's SRGAN discriminator.  `self.model` is a Sequential of stock layers used as parameter containers, so state_dict
    keys, buffers, .to(), load_state_dict(), .train() and .eval() behave as in the reference.  forward dispatches on self.training:
      eval   BatchNorm with the running buffers;
      train  BatchNorm with batch statistics, and the running buffers and num_batches_tracked of model.3 / 6 / 9 / 12 are updated
             in place on the device, as nn.BatchNorm2d does (momentum and eps are read from the containers at every call).
    The forward is asynchronous on the current stream.  With autograd=False (the default) it carries no autograd history.  With
    autograd=True, grad mode on and a parameter or the input requiring grad, it is differentiable once: each call keeps its own
    activations (cid_srd_saved_bytes per call) until its backward has run, and weight changes are repacked on the device."""

    _abi = "srd"

    def __init__(self, autograd: bool = False):
        super().__init__()
        self._autograd = bool(autograd)
        self._bws = None           # backward workspace (uint8 tensor, grow-only)
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
            nn.Conv2d(128, 256, kernel_size=3, padding=1),
            nn.BatchNorm2d(256),
            nn.LeakyReLU(0.2),
            nn.AdaptiveAvgPool2d(1),
            nn.Conv2d(256, 512, kernel_size=1),
            nn.LeakyReLU(0.2),
            nn.Conv2d(512, 1, kernel_size=1),
            nn.Sigmoid(),
        )
        self._create()

    # ------------------------------------------------------------------ weights
    def _tensors(self):
        # the fourteen convolution tensors; the BatchNorm tensors are call arguments.  p._version counts in-place updates made
        # through the tensor API; after writes through `p.data` call pack_weights(force=True)
        return [(f"model.{i}.{kind}", getattr(self.model[i], kind)) for i in _CONVS for kind in ("weight", "bias")]

    def _blob_bytes(self) -> int:
        return _lib.lib().cid_srd_packed_weights_bytes()

    def pack_weights(self, force: bool = False) -> torch.Tensor:
        """Repack the fourteen convolution tensors into the kernels' layout on the module's GPU (if they changed since the last
        call).  With autograd=True the pack runs on the device, into one blob that stays in place: a training loop changes the
        weights at every step."""
        if not self._autograd:
            return super().pack_weights(force)
        sig = self._signature()
        if not force and self._blob is not None and sig == self._packed_sig:
            return self._blob
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("SRGANDiscriminator runs only on an AMD GPU (HIP kernels behind libcid.so); move it with "
                               ".to('cuda') first. There is no CPU fallback.")
        ts = [t.detach() for _, t in self._tensors()]
        if any(t.dtype != torch.float32 or t.device != dev for t in ts):
            raise RuntimeError(f"SRGANDiscriminator: convolution parameters must be float32 on {dev}")
        ts = [t.contiguous() for t in ts]
        if self._blob is None or self._blob.device != dev:
            self._blob = torch.empty(self._blob_bytes(), dtype=torch.uint8, device=dev)
        ptrs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self._check(self._fn("pack_weights_device")(self._cid, ptrs, self._blob.data_ptr(), stream))
        self._packed_sig = sig
        return self._blob

    # ------------------------------------------------------------------ forward
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """fp32 [N,3,H,W] in [-1,1] or uint8 [N,H,W,3] on the GPU -> fp32 [N] probabilities on the same GPU (reference forward,
        sr_ganTrainGNew.py:79-80).  In train mode the BatchNorm running buffers are updated in place."""
        fmt, (n, h, w) = self._image_input(x)
        dev = self._input_device(x)
        if n < 1 or h < 1 or w < 1:
            raise RuntimeError(f"empty input {list(x.shape)}")
        training = self.training
        if training and n * _out_side(_out_side(h)) * _out_side(_out_side(w)) == 1:
            first = 64 if _out_side(h) * _out_side(w) == 1 else 128   # the first BatchNorm that sees one value: model.3 or model.9
            raise ValueError(f"Expected more than 1 value per channel when training, got input size "
                             f"{torch.Size([n, first, 1, 1])}")
        bn = bn_args(self.model, _BNS, dev)
        self.pack_weights()
        if self._autograd and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return _SrdFunction.apply(self, fmt, (n, h, w), training, x, *self.parameters())
        self._ensure_workspace(dev, n, h, w, int(training))
        x = x.detach().contiguous()
        out = torch.empty(n, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self._check(_lib.lib().cid_srd_forward(self._cid, x.data_ptr(), fmt, out.data_ptr(), n, h, w, bn, int(training),
                                                   self._ws.data_ptr(), self._ws.numel(), stream))
        return out


class _SrdFunction(torch.autograd.Function):
    """forward = cid_srd_forward_saved into a buffer owned by this call's context, backward = cid_srd_backward."""

    @staticmethod
    def forward(ctx, module, fmt, shape, training, x, *params):
        n, h, w = shape
        dev = x.device
        L = _lib.lib()
        need = ctypes.c_size_t()
        module._check(L.cid_srd_saved_bytes(n, h, w, int(training), ctypes.byref(need)))
        saved = torch.empty(need.value, dtype=torch.uint8, device=dev)
        xc = x.detach().contiguous()
        out = torch.empty(n, dtype=torch.float32, device=dev)
        bn = bn_args(module.model, _BNS, dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            module._check(L.cid_srd_forward_saved(module._cid, xc.data_ptr(), fmt, out.data_ptr(), n, h, w, bn, int(training),
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
        params = list(module.parameters())
        for name, p, v in zip(ctx.names, params, ctx.versions):
            if p._version != v:
                raise RuntimeError(f"SRGANDiscriminator: parameter {name} was modified in place between a forward and its backward "
                                   f"(version {p._version}, expected {v}); the gradient would be taken at the wrong weights")
        n, h, w = ctx.shape
        dev = ctx.x.device
        L = _lib.lib()
        needs = ctx.needs_input_grad
        g = _GradsArg()
        grads = [None] * len(params)
        for i, (name, p) in enumerate(zip(ctx.names, params)):
            if not needs[5 + i]:
                continue
            grads[i] = torch.empty(p.shape, dtype=torch.float32, device=dev)
            idx, kind = int(name.split(".")[1]), name.rsplit(".", 1)[1]
            if idx in _CONVS:
                (g.w if kind == "weight" else g.b)[_CONVS.index(idx)] = grads[i].data_ptr()
            else:
                (g.gamma if kind == "weight" else g.beta)[_BNS.index(idx)] = grads[i].data_ptr()
        grad_x = None
        if needs[4] and ctx.fmt == _lib.CID_FMT_F32_NCHW:
            grad_x = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
            g.input = grad_x.data_ptr()
        need = ctypes.c_size_t()
        module._check(L.cid_srd_backward_workspace_bytes(n, h, w, int(ctx.training), ctypes.byref(need)))
        if module._bws is None or module._bws.numel() < need.value or module._bws.device != dev:
            module._bws = None
            module._bws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        gp = grad_prob.to(torch.float32).contiguous()
        bn = bn_args(module.model, _BNS, dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            module._check(L.cid_srd_backward(module._cid, ctx.x.data_ptr(), ctx.fmt, gp.data_ptr(), n, h, w, bn, int(ctx.training),
                                             ctx.saved.data_ptr(), ctx.saved.numel(), ctypes.byref(g), module._bws.data_ptr(),
                                             module._bws.numel(), stream))
        ctx.saved = None
        return (None, None, None, None, grad_x, *grads)


def load_srgan_discriminator(source: Union[str, Mapping, None] = None, device: Optional[Union[str, torch.device]] = None,
                             strict: bool = False, autograd: bool = False) -> SRGANDiscriminator:
    """Build an SRGANDiscriminator on `device` (default: current GPU) from an SRGAN trainer checkpoint path (its "discriminator"
    entry, sr_ganTrainGNew.py:342-353, read with the torch-free reader), a checkpoint dict or a state_dict; "module." prefixes are
    stripped as for the generators.  `source=None` keeps the default initialisation.  `autograd=True` makes the forward differentiable
    (SRGANDiscriminator).  Returns the module in eval mode."""
    from .api import _read_checkpoint_file, extract_state_dict

    device = _packed.cuda_device(device, "load_srgan_discriminator")
    model = SRGANDiscriminator(autograd=autograd)
    if isinstance(source, str):
        model.load_state_dict(_read_checkpoint_file(source, key_candidates=("discriminator",)), strict=strict)
    elif source is not None:
        sd = {k: (v if isinstance(v, torch.Tensor) else torch.as_tensor(v))
              for k, v in extract_state_dict(source, ("discriminator",)).items()}
        model.load_state_dict(sd, strict=strict)
    model.to(device).eval()
    model.pack_weights()
    return model


def srgan_trainer_losses(discriminator: SRGANDiscriminator, fake_hr: torch.Tensor, hr_img: torch.Tensor, vgg_loss=None) -> dict:
    """The SRGAN trainer's losses of one batch (sr_ganTrainGNew.py:395-407) -> {"d_loss", "adv_loss", "content_loss", "g_loss"}:
        p_real = D(hr_img), p_fake = D(fake_hr)
        d_loss = BCE(p_real, 1) + BCE(p_fake, 0)      adv_loss = BCE(p_fake, 1)
        content_loss = vgg_loss(fake_hr, hr_img)      g_loss = content_loss + 0.001 * adv_loss
    as floats; without a VGGPerceptualLoss, content_loss and g_loss are None.  BCE clamps its logs at -100 as nn.BCELoss does; the
    two BCE reductions run in one HIP kernel in fp64 in a fixed order (one device-to-host copy).  Each operand is fp32 [N,3,H,W] in
    [-1,1] or uint8 [N,H,W,3] (read as the forward reads it).  Two differences from the trainer: D is evaluated twice at its current
    weights (the trainer evaluates :404 after D's optimizer step), and in train mode each of the two calls updates the BatchNorm
    running statistics."""
    shapes = [_packed.image_operand(t) for t in (fake_hr, hr_img)]
    if shapes[0] is None or shapes[1] is None:
        raise RuntimeError("srgan_trainer_losses: expected fp32 [N,3,H,W] or uint8 [N,H,W,3] batches")
    if shapes[0][1] != shapes[1][1]:
        raise RuntimeError(f"fake_hr and hr_img differ in size: {shapes[0][1]} vs {shapes[1][1]}")
    if fake_hr.device != hr_img.device or fake_hr.device.type != "cuda":
        raise RuntimeError("srgan_trainer_losses: both batches must be on the discriminator's GPU")
    p_real = discriminator(hr_img)
    p_fake = discriminator(fake_hr)
    dev = fake_hr.device
    out = torch.empty(2, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(None, _lib.lib().cid_srd_losses(p_real.data_ptr(), p_fake.data_ptr(), p_real.shape[0], out.data_ptr(), stream))
    content = None if vgg_loss is None else vgg_loss(fake_hr, hr_img)
    d_loss, adv = out.cpu().tolist()
    content = None if content is None else float(content)
    return {"d_loss": d_loss, "adv_loss": adv, "content_loss": content,
            "g_loss": None if content is None else content + 0.001 * adv}
