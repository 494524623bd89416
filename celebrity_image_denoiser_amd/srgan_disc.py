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

from typing import Mapping, Optional, Union

import torch
import torch.nn as nn

from . import _lib, _packed
from .discriminator import BatchNormDiscriminator, _out_side


class SRGANDiscriminator(BatchNormDiscriminator):
    """The reference's SRGAN discriminator (BatchNormDiscriminator: state_dict keys, buffers, .to(), load_state_dict(), .train() and
    .eval() behave as in the reference; train mode updates model.3 / 6 / 9 / 12 in place)."""

    _abi = "srd"
    _CONVS = (0, 2, 5, 8, 11, 15, 17)
    _BNS = (3, 6, 9, 12)

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

    def _single_value_channels(self, h: int, w: int) -> int:
        return 64 if _out_side(h) * _out_side(w) == 1 else 128   # the first BatchNorm that sees one value: model.3 or model.9


def load_srgan_discriminator(source: Union[str, Mapping, None] = None, device: Optional[Union[str, torch.device]] = None,
                             strict: bool = False, autograd: bool = False) -> SRGANDiscriminator:
    """Build an SRGANDiscriminator on `device` (default: current GPU) from an SRGAN trainer checkpoint path (its "discriminator"
    entry, sr_ganTrainGNew.py:342-353, read with the torch-free reader), a checkpoint dict or a state_dict; "module." prefixes are
    stripped as for the generators.  `source=None` keeps the default initialisation.  `autograd=True` makes the forward differentiable
    (SRGANDiscriminator).  Returns the module in eval mode."""
    device = _packed.cuda_device(device, "load_srgan_discriminator")
    return _packed.load_into(SRGANDiscriminator(autograd=autograd), source, device, strict, key_candidates=("discriminator",))


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
