"""LPIPS — the third number of the reference trainers' evaluation (training.py:282,389; net='alex') and the ESRGAN trainer's
perceptual metric (esrgan_train.py:65,133; net='vgg') — and the trainers' VGGPerceptualLoss, on the GPU.

    LPIPS(net="alex")                     nn.Module with the package's state_dict names (scaling_layer.*, net.slice*.*, lin*.*, and
                                          the lins.* aliases); forward(in0, in1, retPerLayer=False, normalize=False) -> fp32 [N,1,1,1]
    load_lpips(lin_ckpt, backbone=None, net="alex")   -> LPIPS from a full LPIPS state dict, or from the package's lin*-only weight
                                          file together with a torchvision AlexNet / vgg16 state dict
    metrics.lpips(a, b, model)            float64 [N] on the device (metrics.py)
    VGGPerceptualLoss(autograd=False)     the trainers' content loss: MSE of vgg16.features[:16]; forward(x, y) -> fp32 scalar,
                                          per_image(x, y) -> float64 [N]; with autograd=True differentiable with respect to x
                                          (cid_vgg_content_loss_saved / cid_vgg_content_backward), else no autograd history
    load_vgg_loss(backbone, autograd=False)   -> VGGPerceptualLoss from a torchvision vgg16 (or features-only) state dict

The definitions are stated once, in the header comments of include/cid.h (cid_lpips, cid_vgg_lpips, cid_vgg_content_loss).
Everything numeric runs in HIP kernels behind cid_lpips_* and cid_vgg_*; there is no CPU fallback.  No weights ship with this package: synth.make_lpips_state_dict draws portable synthetic
ones, and INTEGRATION.md says how to obtain and pass the real ones.
"""
from __future__ import annotations

import ctypes
from typing import Mapping, Optional, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib, _packed

CHANNELS = (64, 192, 384, 256, 256)
MIN_SIDE = 31
# net.slice<k+1>.<index>: torchvision's alexnet.features indices of the five convolutions
_CONVS = ((1, 0, 3, 64, 11, 4, 2), (2, 3, 64, 192, 5, 1, 2), (3, 6, 192, 384, 3, 1, 1), (4, 8, 384, 256, 3, 1, 1),
          (5, 10, 256, 256, 3, 1, 1))
VGG_CHANNELS = (64, 128, 256, 512, 512)
VGG_MIN_SIDE, VGG_LOSS_MIN_SIDE, VGG_MAX_SIDE = 16, 4, _lib.CID_VGG_MAX_SIDE
# torchvision's vgg16.features indices of the thirteen convolutions, by slice
_VGG_CONVS = tuple((k, idx, cin, cout, 3, 1, 1) for k, idx, cin, cout in (
    (1, 0, 3, 64), (1, 2, 64, 64), (2, 5, 64, 128), (2, 7, 128, 128), (3, 10, 128, 256), (3, 12, 256, 256), (3, 14, 256, 256),
    (4, 17, 256, 512), (4, 19, 512, 512), (4, 21, 512, 512), (5, 24, 512, 512), (5, 26, 512, 512), (5, 28, 512, 512)))
_NETS = {"alex": (_CONVS, CHANNELS, "lpips"), "vgg": (_VGG_CONVS, VGG_CHANNELS, "vgg")}


class _ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer("scale", torch.tensor([.458, .448, .450])[None, :, None, None])


class _LinLayer(nn.Module):
    def __init__(self, chn_in: int):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(chn_in, 1, 1, stride=1, padding=0, bias=False))


def operand(x, what: str = "lpips"):
    """(CID format, (N, H, W)) of an fp32 [N,3,H,W] or uint8 [N,H,W,3] tensor."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise RuntimeError(f"{what}() expects 4-d torch tensors: float32 [N,3,H,W] or uint8 [N,H,W,3]")
    got = _packed.image_operand(x)
    if got is None:
        raise RuntimeError(f"expected float32 [N,3,H,W] or uint8 [N,H,W,3], got {x.dtype} {list(x.shape)}")
    return got


class LPIPS(_packed.PackedModule):
    """lpips.LPIPS(net='alex' or 'vgg') as a parameter container plus the HIP forward.  `scaling_layer`, `net`, `lin0` ... `lin4` and `lins`
    are stock layers, so state_dict keys, .to() and load_state_dict() behave as in the package.  Eval mode only (dropout is inert).
    Asynchronous on the current stream, without autograd history.  Weight changes are found by the tensors' version counters and
    repacked at the next call (after writes through `.data` call pack_weights(force=True))."""

    def __init__(self, net: str = "alex"):
        super().__init__()
        if net not in _NETS:
            raise ValueError(f"unknown net {net!r}: 'alex' or 'vgg'")
        self.pnet_type = net
        convs, self.chns, self._abi = _NETS[net]
        self._form = (_lib.CID_VGG_LPIPS,) if self._abi == "vgg" else ()
        self.scaling_layer = _ScalingLayer()
        self.net = nn.Module()
        for k in range(1, 6):
            self.net.add_module(f"slice{k}", nn.Sequential())
        for k, idx, cin, cout, ks, stride, pad in convs:
            getattr(self.net, f"slice{k}").add_module(str(idx), nn.Conv2d(cin, cout, ks, stride=stride, padding=pad))
        for k, c in enumerate(self.chns):
            setattr(self, f"lin{k}", _LinLayer(c))
        self.lins = nn.ModuleList([getattr(self, f"lin{k}") for k in range(5)])
        for p in self.parameters():
            p.requires_grad_(False)
        self.eval()
        self._create()

    def _tensors(self):
        return [(k, t) for k, t in self.state_dict(keep_vars=True).items() if not k.startswith("lins.")]

    def distances(self, a: torch.Tensor, b: torch.Tensor, unit_view: bool = False, per_layer: bool = False):
        """cid_lpips on the current stream: float64 [N] on the device, with per_layer also float64 [N,5] = d_0 ... d_4.  Each operand
        is float32 [N,3,H,W] or uint8 [N,H,W,3] (read as (u/255-0.5)/0.5); unit_view applies v*0.5+0.5 to both (the trainers' call)."""
        if self.training:
            raise RuntimeError("LPIPS is in train mode: the metric is defined in eval mode (dropout inert); call .eval()")
        dev = self._device()
        (fa, fb), (n, h, w) = _check_pair(a, b, dev, "LPIPS")
        if self._abi == "vgg":
            needs = f"LPIPS(net='vgg') needs {VGG_MIN_SIDE} <= H, W <= {VGG_MAX_SIDE} (four 2x2 pools down to 1x1)"
        else:
            needs = f"LPIPS needs H, W >= {MIN_SIDE} (AlexNet's maps 7 -> 3 -> 1) and sides of at most 1024"
        self._ensure_workspace(dev, n, h, w, needs=needs)
        self.pack_weights()
        a, b = a.contiguous(), b.contiguous()
        out = torch.empty((n,), dtype=torch.float64, device=dev)
        layers = torch.empty((n, 5), dtype=torch.float64, device=dev) if per_layer else None
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self._check((_lib.lib().cid_vgg_lpips if self._abi == "vgg" else _lib.lib().cid_lpips)(
                self._cid, a.data_ptr(), fa, b.data_ptr(), fb, n, h, w, _lib.CID_LPIPS_UNIT_VIEW if unit_view else 0, out.data_ptr(),
                layers.data_ptr() if per_layer else None, self._ws.data_ptr(), self._ws.numel(), stream))
        return (out, layers) if per_layer else out

    def forward(self, in0: torch.Tensor, in1: torch.Tensor, retPerLayer: bool = False, normalize: bool = False):
        """The package's call: fp32 [N,1,1,1]; with retPerLayer also the list of the five layer tensors ([N,1,1,1] each).
        normalize=True takes [0,1] inputs (2*x - 1 first): an fp32 copy is made, since the kernels' own input view is the opposite
        one."""
        if normalize:
            in0, in1 = (2.0 * t - 1.0 if t.dtype == torch.float32 else t for t in (in0, in1))
            if in0.dtype != torch.float32 or in1.dtype != torch.float32:
                raise RuntimeError("normalize=True needs float32 operands in [0,1]")
        if retPerLayer:
            d, layers = self.distances(in0, in1, per_layer=True)
            return d.to(torch.float32).view(-1, 1, 1, 1), [layers[:, k].to(torch.float32).view(-1, 1, 1, 1) for k in range(5)]
        return self.distances(in0, in1).to(torch.float32).view(-1, 1, 1, 1)

    def stage(self, name: str, n: int, h: int, w: int) -> torch.Tensor:
        """What the last call over n pairs of h x w images left in the workspace, as fp32 [2 n,C,Hs,Ws] (a copy): "relu1" ... "relu5";
        operand a's n images, then operand b's (cid_lpips_stage_view)."""
        return self._stage(2 * n, name, f"{n} pairs of {h}x{w}", n, h, w)


def _check_pair(a, b, dev, what: str):
    """The operand checks distances() and per_image() share: ((fmt_a, fmt_b), (n, h, w))."""
    fa, shape_a = operand(a)
    fb, shape_b = operand(b)
    if shape_a != shape_b:
        raise ValueError("Input images must have the same dimensions.")
    if not (a.is_cuda and b.is_cuda):
        raise RuntimeError(f"got a CPU tensor: {what} is GPU-only (hand-written HIP kernels); there is no CPU fallback")
    if a.device != dev or b.device != dev:
        raise RuntimeError(f"operands on {a.device} and {b.device} but module parameters on {dev}")
    if shape_a[0] < 1:
        raise RuntimeError(f"empty input {list(a.shape)}")
    return (fa, fb), shape_a


_VGG_LOSS_IDX = (0, 2, 5, 7, 10, 12, 14)
_VGG_SLICE_OF = {idx: k for k, idx, *_ in _VGG_CONVS}


class _VGGLossFunction(torch.autograd.Function):
    """forward = cid_vgg_content_loss_saved into an arena owned by this call's context, backward = cid_vgg_content_backward."""

    @staticmethod
    def forward(ctx, module, fy, shape, unit_view, x, y):
        n, h, w = shape
        dev = x.device
        L = _lib.lib()
        need = ctypes.c_size_t()
        module._check(L.cid_vgg_saved_bytes(n, h, w, ctypes.byref(need)))
        saved = torch.empty(need.value, dtype=torch.uint8, device=dev)
        out = torch.empty((n,), dtype=torch.float64, device=dev)
        flags = _lib.CID_LPIPS_UNIT_VIEW if unit_view else 0
        xc, yc = x.detach().contiguous(), y.detach().contiguous()
        with torch.cuda.device(dev):
            module._check(L.cid_vgg_content_loss_saved(
                module._cid, xc.data_ptr(), _lib.CID_FMT_F32_NCHW, yc.data_ptr(), fy, n, h, w, flags, out.data_ptr(), saved.data_ptr(),
                saved.numel(), torch.cuda.current_stream(dev).cuda_stream))
        ctx.module, ctx.shape, ctx.flags, ctx.saved = module, shape, flags, saved
        ctx.save_for_backward(torch.empty(0, device=dev))   # freed with the graph: a second backward() raises torch's own error
        ctx.names = [k for k, _ in module.named_parameters()]
        ctx.versions = [p._version for p in module.parameters()]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        module = ctx.module
        ctx.saved_tensors   # raises torch's "backward through the graph a second time" once the graph was freed
        if ctx.saved is None:   # retain_graph=True
            raise RuntimeError("VGGPerceptualLoss: this call's saved activations were released by its first backward")
        for name, p, v in zip(ctx.names, module.parameters(), ctx.versions):
            if p._version != v:
                raise RuntimeError(f"VGGPerceptualLoss: parameter {name} was modified in place between a forward and its backward "
                                   f"(version {p._version}, expected {v}); the gradient would be taken at the wrong weights")
        n, h, w = ctx.shape
        dev = ctx.saved.device
        grad_x = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
        go = grad_out.to(torch.float64).contiguous()
        with torch.cuda.device(dev):
            module._pack_backward_weights()
            module._check(_lib.lib().cid_vgg_content_backward(
                module._cid, go.data_ptr(), grad_x.data_ptr(), n, h, w, ctx.flags, ctx.saved.data_ptr(), ctx.saved.numel(),
                torch.cuda.current_stream(dev).cuda_stream))
        ctx.saved = None
        return None, None, None, None, grad_x, None


class VGGPerceptualLoss(_packed.PackedModule):
    """The reference trainers' VGGPerceptualLoss (sr_ganTrainGNew.py:83-94, training.py:101-111): MSELoss of vgg16.features[:16] on
    the two operands as they are, with the reference's parameter names slice.{0,2,5,7,10,12,14}.weight / .bias, frozen, eval mode.
    The forward runs in HIP kernels (cid_vgg_content_loss) on the current stream.

    autograd=False (default): no autograd history.  autograd=True: when grad mode is on and `x` requires grad, per_image records a
    torch.autograd.Function whose backward is cid_vgg_content_backward (HIP kernels, d loss / d x through the seven frozen
    convolutions), so the trainer's `g_loss = vgg(fake, hr) + ...; g_loss.backward()` reaches the generator; the activations live in a
    per-call arena that is released after the backward.  `y` gets no gradient (y.requires_grad raises NotImplementedError); a uint8 `x`
    has none and takes the plain path.  The weights stay frozen."""

    _abi = "vgg"
    _form = (_lib.CID_VGG_CONTENT,)

    def __init__(self, autograd: bool = False):
        super().__init__()
        self.autograd = bool(autograd)
        self.slice = nn.Sequential()
        for k, idx, cin, cout, ks, stride, pad in _VGG_CONVS[:7]:
            self.slice.add_module(str(idx), nn.Conv2d(cin, cout, ks, stride=stride, padding=pad))
        for p in self.parameters():
            p.requires_grad_(False)
        self.eval()
        self._create()
        self._bwd_blob = None      # the data-gradient weights on the device, packed at the first differentiable call
        self._bwd_of = None        # the forward blob they were packed with

    def _key(self, key: str) -> str:
        _, idx, leaf = key.split(".")
        return f"net.slice{_VGG_SLICE_OF[int(idx)]}.{idx}.{leaf}"

    def _pack_backward_weights(self) -> torch.Tensor:
        """The backward blob (cid_vgg_upload_backward_weights) of the packed forward weights; rebuilt when pack_weights rebuilt those."""
        blob = self.pack_weights()
        if self._bwd_blob is None or self._bwd_of is not blob:
            dev = blob.device
            bwd = torch.empty(_lib.lib().cid_vgg_backward_weights_bytes(self._cid), dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                self._check(_lib.lib().cid_vgg_upload_backward_weights(self._cid, bwd.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
            self._bwd_blob, self._bwd_of = bwd, blob
        return self._bwd_blob

    def per_image(self, x: torch.Tensor, y: torch.Tensor, unit_view: bool = False) -> torch.Tensor:
        """cid_vgg_content_loss on the current stream: float64 [N] on the device, the mean squared difference of relu3_3 per pair.
        With autograd=True, grad mode on and x requiring grad, the result carries the history of x."""
        if self.training:
            raise RuntimeError("VGGPerceptualLoss is in train mode: the reference keeps it in eval mode; call .eval()")
        dev = self._device()
        (fx, fy), (n, h, w) = _check_pair(x, y, dev, "VGGPerceptualLoss")
        needs = f"VGGPerceptualLoss needs {VGG_LOSS_MIN_SIDE} <= H, W <= {VGG_MAX_SIDE}"
        if self.autograd and torch.is_grad_enabled():
            if y.requires_grad:
                raise NotImplementedError("VGGPerceptualLoss(autograd=True): no gradient for the second operand (the reference's "
                                          "hr_img never requires one); detach it")
            if x.requires_grad and fx == _lib.CID_FMT_F32_NCHW:
                need = ctypes.c_size_t()
                if _lib.lib().cid_vgg_saved_bytes(n, h, w, ctypes.byref(need)) == 2:   # CID_ERR_SHAPE
                    raise ValueError(f"image size {h}x{w} (N={n}) not accepted: {needs}")
                self._pack_backward_weights()
                return _VGGLossFunction.apply(self, fy, (n, h, w), bool(unit_view), x, y)
        self._ensure_workspace(dev, n, h, w, needs=needs)
        self.pack_weights()
        x, y = x.detach().contiguous(), y.detach().contiguous()
        out = torch.empty((n,), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            self._check(_lib.lib().cid_vgg_content_loss(
                self._cid, x.data_ptr(), fx, y.data_ptr(), fy, n, h, w, _lib.CID_LPIPS_UNIT_VIEW if unit_view else 0, out.data_ptr(),
                self._ws.data_ptr(), self._ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
        return out

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """The reference's call: the fp32 scalar MSELoss()(slice(x), slice(y)), the mean of per_image (torch's own differentiable
        ops over the float64 [N], so with autograd=True the scalar trains through)."""
        return self.per_image(x, y).mean().to(torch.float32)

    def stage(self, name: str, n: int, h: int, w: int) -> torch.Tensor:
        """ "relu1" ... "relu3" (relu1_2, relu2_2, relu3_3) of the last call, fp32 [2 n,C,Hs,Ws] (a copy): x's n images, then y's."""
        return self._stage(2 * n, name, f"{n} pairs of {h}x{w}", n, h, w)


def vgg_loss_state_dict(backbone_sd: Mapping) -> dict:
    """slice.N.* from a torchvision vgg16 state dict (features.N.*, later features and classifier.* dropped), a features-only one
    (N.*) or the class's own (slice.N.*).  Any other key raises KeyError."""
    from .api import extract_state_dict

    out = {}
    for k, v in extract_state_dict(backbone_sd).items():
        parts = k.split(".")
        if parts[0] in ("features", "slice"):
            parts = parts[1:]
        elif parts[0] == "classifier":
            continue
        if len(parts) != 2 or not parts[0].isdigit() or parts[1] not in ("weight", "bias") or int(parts[0]) not in [c[1] for c in _VGG_CONVS]:
            raise KeyError(f"unexpected key {k!r} in the vgg16 state dict (expected features.N.weight / .bias and classifier.*)")
        if int(parts[0]) in _VGG_LOSS_IDX:
            out[f"slice.{parts[0]}.{parts[1]}"] = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
    return out


def build_vgg_loss(backbone, reader=None, autograd: bool = False) -> VGGPerceptualLoss:
    """load_vgg_loss without the move to the GPU."""
    if reader is None:
        from .api import _read_checkpoint_file as reader
    model = VGGPerceptualLoss(autograd=autograd)
    model.load_state_dict(vgg_loss_state_dict(reader(backbone) if isinstance(backbone, str) else backbone), strict=True)
    return model


def load_vgg_loss(backbone: Union[str, Mapping], device: Optional[Union[str, torch.device]] = None,
                  autograd: bool = False) -> VGGPerceptualLoss:
    """A VGGPerceptualLoss on `device` (default: current GPU) from a torchvision vgg16 state dict or a features-only one, a path or
    a mapping.  `autograd=True` makes it differentiable with respect to its first operand (VGGPerceptualLoss)."""
    device = _packed.cuda_device(device, "load_vgg_loss")
    model = build_vgg_loss(backbone, autograd=autograd)
    model.to(device).eval()
    model.pack_weights()
    return model


def lpips_state_dict(lin_sd: Mapping, backbone_sd: Optional[Mapping] = None, net: str = "alex") -> dict:
    """The module's state dict from either layout: a full LPIPS state dict, or the package's lin*-only file plus a torchvision
    AlexNet / vgg16 state dict (features.N.* -> net.sliceK.N.*, classifier.* dropped).  "module." prefixes are stripped; lins.* aliases are
    filled from lin* (or the other way round)."""
    from .api import extract_state_dict

    features = {f"features.{idx}.": f"net.slice{k}.{idx}." for k, idx, *_ in _NETS[net][0]}
    out = {}
    for k, v in extract_state_dict(lin_sd).items():
        out[k] = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
    if backbone_sd is not None:
        for k, v in extract_state_dict(backbone_sd).items():
            if k.startswith("classifier."):
                continue
            for old, new in features.items():
                if k.startswith(old):
                    out[new + k[len(old):]] = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
                    break
            else:
                name = "AlexNet" if net == "alex" else "vgg16"
                want = ",".join(str(c[1]) for c in _NETS[net][0])
                raise KeyError(f"unexpected key {k!r} in the {name} state dict (expected features.{{{want}}}.* and classifier.*)")
    for k in range(5):
        a, b = f"lin{k}.model.1.weight", f"lins.{k}.model.1.weight"
        if a in out and b not in out:
            out[b] = out[a]
        elif b in out and a not in out:
            out[a] = out[b]
    return out


def load_lpips(lin_ckpt: Union[str, Mapping], backbone: Union[str, Mapping, None] = None,
               device: Optional[Union[str, torch.device]] = None, strict: bool = True, net: str = "alex") -> LPIPS:
    """Build an LPIPS on `device` (default: current GPU).  `lin_ckpt` is a full LPIPS state dict, or the package's weight file
    (lin* keys only) with `backbone` a torchvision AlexNet (net="alex") or vgg16 (net="vgg") state dict; each a path (read with the torch-free reader) or a mapping.
    The module's own shift / scale buffers stand in when a file leaves them out.  strict=True raises for any other missing or
    unexpected key, as load_state_dict does."""
    from .api import _read_checkpoint_file

    device = _packed.cuda_device(device, "load_lpips")
    model = build_lpips(lin_ckpt, backbone, strict, _read_checkpoint_file, net=net)
    model.to(device).eval()
    model.pack_weights()
    return model


def build_lpips(lin_ckpt, backbone=None, strict: bool = True, reader=None, net: str = "alex") -> LPIPS:
    """load_lpips without the move to the GPU: the module on the CPU, weights loaded (the loader's key handling, testable anywhere)."""
    if reader is None:
        from .api import _read_checkpoint_file as reader
    lin_sd = reader(lin_ckpt) if isinstance(lin_ckpt, str) else lin_ckpt
    back_sd = reader(backbone) if isinstance(backbone, str) else backbone
    model = LPIPS(net)
    sd = lpips_state_dict(lin_sd, back_sd, net)
    for k, v in model.scaling_layer.state_dict(prefix="scaling_layer.").items():
        sd.setdefault(k, v)
    model.load_state_dict(sd, strict=strict)
    return model
