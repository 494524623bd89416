"""The server's third model (`SRGANGenerator`, reference backend/app.py:145-186, the "srgan" branch of /enhance) on the GPU.

    SRGANGenerator(scale_factor=4)            nn.Module with the reference's parameter names (initial.*, res_blocks.i.j.*, mid.*,
                                              upscale.*, final.*, BatchNorm buffers included); forward(x) in eval mode
    SRGANGenerator(4, batch_stats=True)       the same module with a train-mode forward as well: BatchNorm on batch statistics,
                                              running buffers updated in place (the trainer's fake_hr = self.generator(lr_img))
    load_srgan(path_or_state_dict)            -> SRGANGenerator from a checkpoint (its "generator" / "state_dict" / "G" entry)
    super_resolve(model, x)                   fp32 [N,3,H,W] in [-1,1] -> fp32 [N,3,sH,sW] = tanh(.)
    super_resolve_u8(model, u8_nhwc)          uint8 [N,H,W,3] -> uint8 [N,s*Hp,s*Wp,3], the server's branch: pad to a multiple of
                                              4*s -> ToTensor -> Normalize(0.5, 0.5) -> network -> y*0.5+0.5 -> clamp -> ToPILImage,
                                              with padding and both conversions inside the first / last kernel

Everything numeric runs in HIP kernels behind cid_sr_* (include/cid.h).  In eval mode BatchNorm uses its running statistics,
folded once per weight upload.  Calling the default module in train mode raises; with batch_stats=True the train-mode forward runs
cid_sr_forward_train (forward only: no autograd history).  There is no CPU fallback.

The server shows this model's whole padded output and crops only the input's picture (app.py:481-485); `crop=True` gives the part of
the output that belongs to the unpadded image instead.
"""
from __future__ import annotations

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
    the discriminator step consumes through .detach().  The next eval forward folds the updated running statistics again."""

    _abi = "sr"

    def __init__(self, scale_factor: int = 4, batch_stats: bool = False):
        super().__init__()
        self._batch_stats = bool(batch_stats)
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
        """PackedModule.pack_weights; after a train forward the fold of the running statistics is stale and the pack runs again."""
        blob = super().pack_weights(force or self._fold_stale)
        self._fold_stale = False
        return blob

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
        _packed.PackedModule.pack_weights(self)
        s = self.scale_factor
        self._ensure_workspace(dev, n, h, w, s, sizer="train_workspace_bytes")
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


def load_srgan(source: Union[str, Mapping, None] = None, scale_factor: int = 4,
               device: Optional[Union[str, torch.device]] = None, strict: bool = False, batch_stats: bool = False) -> SRGANGenerator:
    """Build an SRGANGenerator on `device` (default: current GPU) from a checkpoint path (read with the torch-free reader), a
    checkpoint dict or a state_dict: the state_dict is looked up under "generator", "state_dict" and "G" and "module." prefixes are
    stripped, as load_state_safely does (app.py:257-274).  `source=None` keeps the default initialisation.  `batch_stats=True` gives
    the module a train-mode forward (SRGANGenerator).  Returns the module in eval mode."""
    device = _packed.cuda_device(device, "load_srgan")
    return _packed.load_into(SRGANGenerator(scale_factor, batch_stats=batch_stats), source, device, strict)


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
