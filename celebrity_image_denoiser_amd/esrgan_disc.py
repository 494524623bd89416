"""The ESRGAN trainer's discriminator (`Discriminator`, reference backend/trainingcode/esrgan_code/models.py:36-71) on the GPU.

    ESRGANDiscriminator(input_shape=(3, 256, 256),      nn.Module with the reference's parameter names (conv1 ... conv4, fc);
                        autograd=False)                 forward(x) -> fp32 [N,1] logits (no sigmoid: the trainer uses BCEWithLogitsLoss)
    load_esrgan_discriminator(path_or_sd)               -> ESRGANDiscriminator from the "D" entry of an ESRGAN trainer checkpoint
    esrgan_trainer_losses(D, denoised, clean)           -> the trainer's d_loss / gan_loss / pixel_loss / g_loss, on the device

Everything numeric runs in HIP kernels behind cid_esd_* (include/cid.h).  By default the module is forward only: the output carries
no autograd history, so the trainer's d_loss.backward() on it raises torch's own "does not require grad" error.  With autograd=True
the forward records a torch.autograd.Function whose backward is cid_esd_backward: the trainer's discriminator step
(esrgan_train.py:101-109) and the adversarial half of its generator step (:112-121) then run on these kernels, with a stock
torch.optim optimizer or cid.Adam doing the update.  No double backward.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Mapping, Optional, Sequence, Union

import torch
import torch.nn as nn

from . import _lib, _packed
from .discriminator import device_pack


def _half(v: int) -> int:
    """Output side of a 3x3 stride-2 padding-1 convolution."""
    return (v - 1) // 2 + 1


def feature_side(v: int) -> int:
    """Side of conv4's output for an input side `v`."""
    for _ in range(4):
        v = _half(v)
    return v


def _check_input_shape(input_shape: Sequence[int]):
    shape = tuple(int(v) for v in input_shape)
    if len(shape) != 3 or shape[0] != 3:
        raise ValueError(f"input_shape must be (3, H, W), got {tuple(input_shape)}")
    if not (1 <= shape[1] <= _lib.CID_ESD_MAX_SIDE and 1 <= shape[2] <= _lib.CID_ESD_MAX_SIDE):
        raise ValueError(f"input_shape {shape}: H and W must be within 1 ... {_lib.CID_ESD_MAX_SIDE}")
    return shape


class ESRGANDiscriminator(_packed.PackedModule):
    """The reference's ESRGAN discriminator.  conv1 ... conv4 and fc are stock layers used as parameter containers, so state_dict
    keys, .to() and load_state_dict() behave as in the reference: a stock state dict loads with strict=True and this module's loads
    back into a stock module.  There are no buffers, and train and eval mode behave the same.  The linear layer fixes the input size
    (`input_shape`, as in the reference).  The forward is asynchronous on the current stream.  With autograd=False (the default) it
    carries no autograd history.  With autograd=True, grad mode on and a parameter or the input requiring grad, it is differentiable
    once: each call keeps its own activations (cid_esd_saved_bytes per call) until its backward has run, and weight changes are
    repacked on the device."""

    _abi = "esd"

    def __init__(self, input_shape: Sequence[int] = (3, 256, 256), autograd: bool = False):
        super().__init__()
        self._autograd = bool(autograd)
        self._bws = None           # backward workspace (uint8 tensor, grow-only)
        self.input_shape = _check_input_shape(input_shape)
        self.conv1 = nn.Conv2d(3, 64, kernel_size=3, stride=2, padding=1)
        self.leaky_relu = nn.LeakyReLU(0.2, inplace=True)
        self.conv2 = nn.Conv2d(64, 128, kernel_size=3, stride=2, padding=1)
        self.conv3 = nn.Conv2d(128, 256, kernel_size=3, stride=2, padding=1)
        self.conv4 = nn.Conv2d(256, 512, kernel_size=3, stride=2, padding=1)
        self._shape = 512 * feature_side(self.input_shape[1]) * feature_side(self.input_shape[2])
        self.fc = nn.Linear(self._shape, 1)
        self._create(self.input_shape[1], self.input_shape[2])

    def _blob_bytes(self) -> int:
        return _lib.lib().cid_esd_packed_weights_bytes(self.input_shape[1], self.input_shape[2])

    def pack_weights(self, force: bool = False) -> torch.Tensor:
        """Repack the ten tensors into the kernels' layout on the module's GPU (if they changed since the last call).  With
        autograd=True the pack runs on the device, into one blob that stays in place: a training loop changes the weights at every
        step."""
        if not self._autograd:
            return super().pack_weights(force)
        return device_pack(self, "parameters", force)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """fp32 [N,3,H,W] in [0,1] or uint8 [N,H,W,3] on the GPU -> fp32 [N,1] logits on the same GPU (reference forward,
        models.py:67-71).  H and W must be input_shape's; the input must be contiguous."""
        fmt, (n, h, w) = self._image_input(x)
        dev = self._input_device(x)
        if n < 1:
            raise RuntimeError(f"empty input {list(x.shape)}")
        if (h, w) != self.input_shape[1:]:
            raise RuntimeError(f"input is {h}x{w} but this discriminator was built for input_shape={self.input_shape}: the linear "
                               f"layer takes {self._shape} features")
        if not x.is_contiguous():
            raise RuntimeError(f"ESRGANDiscriminator expects a contiguous input, got strides {tuple(x.stride())}")
        self.pack_weights()
        if self._autograd and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return _EsdFunction.apply(self, fmt, (n, h, w), x, *self.parameters())
        self._ensure_workspace(dev, n, h, w)
        x = x.detach()
        out = torch.empty((n, 1), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self._check(_lib.lib().cid_esd_forward(self._cid, x.data_ptr(), fmt, out.data_ptr(), n, h, w, self._ws.data_ptr(),
                                                   self._ws.numel(), stream))
        return out

    def stages(self, n: int):
        """The four activated tensors a1 ... a4 the last forward of `n` images left in the workspace, as fp32 [n,C,Hs,Ws] copies
        (the offsets of cid_esd_workspace_bytes, include/cid.h)."""
        out, off, h, w = [], 0, self.input_shape[1], self.input_shape[2]
        for c in (64, 128, 256, 512):
            h, w = _half(h), _half(w)
            count = n * c * h * w
            t = self._ws[off:off + 4 * count].view(torch.float32).view(n, c // 8, h, w, 8).permute(0, 1, 4, 2, 3)
            out.append(t.reshape(n, c, h, w).clone())
            off += (4 * count + 255) // 256 * 256
        return out


class _EsdFunction(torch.autograd.Function):
    """forward = cid_esd_forward_saved into a buffer owned by this call's context, backward = cid_esd_backward (the counterpart of
    discriminator._DiscFunction for a model without BatchNorm)."""

    _LAYERS = ("conv1", "conv2", "conv3", "conv4", "fc")

    @staticmethod
    def forward(ctx, module, fmt, shape, x, *params):
        n, h, w = shape
        dev = x.device
        need = ctypes.c_size_t()
        module._check(_lib.lib().cid_esd_saved_bytes(n, h, w, ctypes.byref(need)))
        saved = torch.empty(need.value, dtype=torch.uint8, device=dev)
        xc = x.detach()
        out = torch.empty((n, 1), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            module._check(_lib.lib().cid_esd_forward_saved(module._cid, xc.data_ptr(), fmt, out.data_ptr(), n, h, w, saved.data_ptr(),
                                                           saved.numel(), stream))
        ctx.module, ctx.fmt, ctx.shape = module, fmt, shape
        ctx.saved, ctx.x = saved, xc
        ctx.names = [k for k, _ in module.named_parameters()]
        ctx.versions = [p._version for p in params]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_logit):
        module = ctx.module
        params = list(module.parameters())
        for name, p, v in zip(ctx.names, params, ctx.versions):
            if p._version != v:
                raise RuntimeError(f"{type(module).__name__}: parameter {name} was modified in place between a forward and its "
                                   f"backward (version {p._version}, expected {v}); the gradient would be taken at the wrong weights")
        n, h, w = ctx.shape
        dev = ctx.x.device
        needs = ctx.needs_input_grad
        g = _GradsArg()
        grads = [None] * len(params)
        for i, (name, p) in enumerate(zip(ctx.names, params)):
            if not needs[4 + i]:
                continue   # a frozen parameter: a null pointer, and no work that only it needs
            grads[i] = torch.empty(p.shape, dtype=torch.float32, device=dev)
            layer, kind = name.rsplit(".", 1)
            (g.w if kind == "weight" else g.b)[_EsdFunction._LAYERS.index(layer)] = grads[i].data_ptr()
        grad_x = None
        if needs[3] and ctx.fmt == _lib.CID_FMT_F32_NCHW:
            grad_x = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
            g.input = grad_x.data_ptr()
        need = ctypes.c_size_t()
        module._check(_lib.lib().cid_esd_backward_workspace_bytes(n, h, w, ctypes.byref(need)))
        if module._bws is None or module._bws.numel() < need.value or module._bws.device != dev:
            module._bws = None
            module._bws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        gl = grad_logit.to(torch.float32).contiguous()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            module._check(_lib.lib().cid_esd_backward(module._cid, ctx.x.data_ptr(), ctx.fmt, gl.data_ptr(), n, h, w, ctx.saved.data_ptr(),
                                                      ctx.saved.numel(), ctypes.byref(g), module._bws.data_ptr(), module._bws.numel(),
                                                      stream))
        ctx.saved = None
        return (None, None, None, grad_x, *grads)


class _GradsArg(ctypes.Structure):
    """cid_esd_grads (include/cid.h)."""
    _fields_ = [("w", ctypes.c_void_p * 5), ("b", ctypes.c_void_p * 5), ("input", ctypes.c_void_p)]


def infer_input_shape(fc_features: int):
    """input_shape of a checkpoint from the width of its fc.weight: 512 * H4 * W4 features.  The trainer's images are square 256 x 256
    (esrgan_train.py: input_shape=(3, 256, 256)), which is the only size the width can tell: anything else needs input_shape."""
    want = 512 * feature_side(256) ** 2
    if fc_features != want:
        raise ValueError(f"fc.weight has {fc_features} features, the trainer's 256 x 256 input gives {want}: pass input_shape=(3, H, W) "
                         "for a discriminator trained at another size")
    return (3, 256, 256)


def load_esrgan_discriminator(source: Union[str, Mapping, None] = None, device: Optional[Union[str, torch.device]] = None,
                              input_shape: Optional[Sequence[int]] = None, autograd: bool = False) -> ESRGANDiscriminator:
    """Build an ESRGANDiscriminator on `device` (default: current GPU) from an ESRGAN trainer checkpoint path (its "D" entry,
    esrgan_train.py:166-172, read with the torch-free reader), a checkpoint dict or a state_dict; "module." prefixes are stripped.
    Without `input_shape` it is inferred from fc.weight's width (infer_input_shape).  `source=None` keeps the default initialisation.
    The state dict is loaded with strict=True.  `autograd=True` makes the forward differentiable (ESRGANDiscriminator)."""
    from . import ckpt
    from .api import extract_state_dict

    device = _packed.cuda_device(device, "load_esrgan_discriminator")
    sd = None
    candidates = ("D", "discriminator", "state_dict")
    if isinstance(source, str):
        sd = ckpt.read_state_dict(source, key_candidates=candidates)
    elif source is not None:
        sd = extract_state_dict(source, candidates)
    if sd is not None:
        # a checkpoint without a discriminator entry comes back whole (its "G", "g_opt", ... entries): not a state dict of this model
        if "fc.weight" not in sd or getattr(sd["fc.weight"], "ndim", 0) != 2:
            raise KeyError(f"no discriminator state dict found (looked under {candidates}; got keys {sorted(map(str, sd))[:8]})")
        sd = {k: (v if isinstance(v, torch.Tensor) else torch.as_tensor(v)) for k, v in sd.items()}
        if input_shape is None:
            input_shape = infer_input_shape(int(sd["fc.weight"].shape[1]))
    model = ESRGANDiscriminator((3, 256, 256) if input_shape is None else input_shape, autograd=autograd)
    if sd is not None:
        model.load_state_dict(sd, strict=True)
    model.to(device).eval()
    model.pack_weights()
    return model


def esrgan_trainer_losses(discriminator: ESRGANDiscriminator, denoised: torch.Tensor, clean: torch.Tensor) -> dict:
    """The ESRGAN trainer's losses of one batch (esrgan_train.py:104-119) -> {"d_loss", "gan_loss", "pixel_loss", "g_loss"}:
        real = D(clean), fake = D(denoised)
        d_loss = 0.5 * (BCEWithLogits(real, 1) + BCEWithLogits(fake, 0))      gan_loss = BCEWithLogits(fake, 1)
        pixel_loss = MSE(denoised, clean)                                     g_loss = pixel_loss + 1e-3 * gan_loss
    as 0-dim float64 tensors ON THE DEVICE: nothing is copied to the host and nothing waits.  The four values come from one HIP
    kernel in fp64 in a fixed order.  Each operand is fp32 [N,3,H,W] in [0,1] or uint8 [N,H,W,3] (read as the forward reads it).
    One difference from the trainer: D is evaluated twice at its current weights (the trainer evaluates :116 after D's
    optimizer step)."""
    shapes = [_packed.image_operand(t) for t in (denoised, clean)]
    if shapes[0] is None or shapes[1] is None:
        raise RuntimeError("esrgan_trainer_losses: expected fp32 [N,3,H,W] or uint8 [N,H,W,3] batches")
    if shapes[0][1] != shapes[1][1]:
        raise RuntimeError(f"denoised and clean differ in size: {shapes[0][1]} vs {shapes[1][1]}")
    if denoised.device != clean.device or denoised.device.type != "cuda":
        raise RuntimeError("esrgan_trainer_losses: both batches must be on the discriminator's GPU")
    real = discriminator(clean)
    fake = discriminator(denoised)
    dev = denoised.device
    n, h, w = shapes[0][1]
    out = torch.empty(4, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(None, _lib.lib().cid_esd_trainer_losses(real.data_ptr(), fake.data_ptr(), denoised.data_ptr(), shapes[0][0],
                                                           clean.data_ptr(), shapes[1][0], n, h, w, out.data_ptr(), stream))
    return {"d_loss": out[0], "gan_loss": out[1], "pixel_loss": out[2], "g_loss": out[3]}
