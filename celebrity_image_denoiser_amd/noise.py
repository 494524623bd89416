"""The reference trainer's five noise kinds on device uint8 batches, and the evaluation loop over them.

The reference trains its denoiser on gaussian, salt & pepper, speckle, Poisson and uniform noise (DenoiseDataset over
['gaussian', 'salt_pepper', 'speckle', 'poisson', 'uniform'], backend/trainingcode/denoise_gan_code/training.py:247), each made
from a clean uint8 image by noise_generation.py:6-39.  add_noise computes them in HIP kernels (cid_add_noise, include/cid.h) with
the reference's formulas and defaults; the draws come from the counter-based hash streams of synth.py instead of np.random, so
synth.add_noise_np is a bit-defined CPU restatement and an image's noise depends only on (seed, its global index, its size).
There is no CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import ctypes

from . import synth

NOISE_TYPES = synth.NOISE_TYPES
_KIND_IDS = {"gaussian": 0, "salt_pepper": 1, "speckle": 2, "poisson": 3, "uniform": 4}   # CID_NOISE_*
_M64 = 0xFFFFFFFFFFFFFFFF


def add_noise(clean_u8, kind: str, *, seed: int = synth.NOISE_SEED, first_index: int = 0, out=None, **params):
    """uint8 [N,H,W,3] on the GPU -> the same batch with `kind` noise (one of NOISE_TYPES), computed by HIP kernels on torch's
    current stream.  Parameters take the reference's names and defaults: gaussian (mean=0, sigma=25), salt_pepper
    (salt_prob=0.02, pepper_prob=0.02), speckle (mean=0, sigma=0.1), poisson (none), uniform (low=0, high=25).  Image n is noised
    as global image first_index + n, so splitting a batch does not change its bits.  `out` (uint8, same shape, contiguous) may be
    `clean_u8` itself.  Equals synth.add_noise_np(clean_u8.cpu().numpy(), kind, seed, first_index, **params)."""
    import torch

    from . import _lib

    if kind not in _KIND_IDS:
        raise ValueError(f"unknown noise kind {kind!r}; expected one of {NOISE_TYPES}")
    defaults = synth.NOISE_DEFAULTS[kind]
    unknown = set(params) - set(defaults)
    if unknown:
        raise TypeError(f"unknown parameter(s) {sorted(unknown)} for {kind!r} noise; expected {sorted(defaults)}")
    if not isinstance(clean_u8, torch.Tensor) or clean_u8.dtype != torch.uint8 or clean_u8.dim() != 4 or clean_u8.shape[3] != 3:
        raise RuntimeError("add_noise expects a uint8 tensor of shape [N,H,W,3]")
    if not clean_u8.is_cuda:
        raise RuntimeError("got a CPU tensor: noise synthesis is GPU-only; there is no CPU fallback (synth.add_noise_np is the "
                           "CPU restatement used by the tests)")
    n, h, w, _ = clean_u8.shape
    clean_u8 = clean_u8.contiguous()
    if out is None:
        out = torch.empty_like(clean_u8)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.shape != clean_u8.shape
          or out.device != clean_u8.device or not out.is_contiguous()):
        raise RuntimeError(f"out must be a contiguous uint8 tensor of shape {list(clean_u8.shape)} on {clean_u8.device}")
    values = [float(params.get(k, v)) for k, v in defaults.items()]
    arr = (ctypes.c_double * max(len(values), 1))(*values)
    with torch.cuda.device(clean_u8.device):
        stream = torch.cuda.current_stream(clean_u8.device).cuda_stream
        rc = _lib.lib().cid_add_noise(clean_u8.data_ptr(), out.data_ptr(), n, h, w, _KIND_IDS[kind], arr, len(values),
                                      seed & _M64, first_index & _M64, stream)
    if rc == 1:   # CID_ERR_INVALID: the pointers are checked above, so a parameter value
        raise ValueError(f"invalid parameters for {kind!r} noise: {dict(zip(defaults, values))} (finite; sigma >= 0; "
                         "probabilities in [0, 1]; low <= high)")
    if rc == 2:   # CID_ERR_SHAPE
        raise ValueError(f"image batch {list(clean_u8.shape)} not accepted for {kind!r} noise: N, H, W >= 1 (H, W >= 2 for "
                         "salt_pepper), H*W*3 < 2^31")
    _lib.check(None, rc)
    return out


def evaluate_noise_types(model, clean_u8, kinds=NOISE_TYPES, seed: int = synth.NOISE_SEED, first_index: int = 0,
                         max_batch: int = None, discriminator=None, lpips=None) -> dict:
    """How well `model` denoises each noise kind, all on the GPU: per kind, add_noise -> model.forward_u8(noisy, out_u8=False) ->
    metrics.quality(denoised, clean_u8), plus metrics.quality(noisy, clean_u8) for the input's own PSNR.

    clean_u8 is a device uint8 [N,H,W,3] batch with H and W multiples of 4 (so that the forward's output matches it).  Returns
    {kind: {"psnr_noisy", "psnr", "ssim", "ms_ssim"}}: float64 means over the batch of the per-image values (numpy's mean of
    the values copied to the host).  "ms_ssim" is left out when min(H, W) <= 160, where MS-SSIM is not defined.  max_batch
    bounds the images per forward; the results do not depend on it beyond the forward's own batch independence.

    With a `discriminator` (discriminator.DenoiseDiscriminator), each kind's dict also holds "d_loss" and "g_loss": the trainer's
    two per-epoch numbers (training.py:455) from discriminator.trainer_losses(discriminator, denoised, clean), here per noise kind
    on held-out images; with max_batch they are averaged over the chunks weighted by chunk size.

    With an `lpips` model (lpips.LPIPS), each kind's dict also holds "lpips": the batch mean of the trainer's call on the denoised and
    the clean images (metrics.lpips(..., unit_view=True), training.py:389)."""
    import numpy as np
    import torch

    from . import metrics

    if not isinstance(clean_u8, torch.Tensor) or clean_u8.dtype != torch.uint8 or clean_u8.dim() != 4 or clean_u8.shape[3] != 3:
        raise RuntimeError("evaluate_noise_types expects a uint8 tensor of shape [N,H,W,3]")
    n, h, w, _ = clean_u8.shape
    if h % 4 or w % 4:
        raise ValueError(f"H and W must be multiples of 4 so that the denoised output matches the clean batch, got {h}x{w}")
    kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
    for k in kinds:
        if k not in _KIND_IDS:
            raise ValueError(f"unknown noise kind {k!r}; expected one of {NOISE_TYPES}")
    names = ("psnr", "ssim", "ms_ssim") if min(h, w) > 160 else ("psnr", "ssim")
    step = n if max_batch is None else int(max_batch)
    if step < 1:
        raise ValueError(f"max_batch must be >= 1, got {max_batch}")
    clean_u8 = clean_u8.contiguous()
    if discriminator is not None:
        from .discriminator import trainer_losses
    result = {}
    for kind in kinds:
        vals = {m: [] for m in ("psnr_noisy",) + names + (("lpips",) if lpips is not None else ())}
        losses = {"d_loss": 0.0, "g_loss": 0.0}
        for i0 in range(0, n, step):
            clean = clean_u8[i0:i0 + step]
            noisy = add_noise(clean, kind, seed=seed, first_index=first_index + i0)
            denoised = model.forward_u8(noisy, out_u8=False)
            q = metrics.quality(denoised, clean, names)
            vals["psnr_noisy"].append(metrics.quality(noisy, clean, ("psnr",))["psnr"].cpu().numpy())
            for m in names:
                vals[m].append(q[m].cpu().numpy())
            if lpips is not None:
                vals["lpips"].append(metrics.lpips(denoised, clean, lpips, unit_view=True).cpu().numpy())
            if discriminator is not None:
                lo = trainer_losses(discriminator, denoised, clean)
                for m in losses:
                    losses[m] += lo[m] * clean.shape[0]
        result[kind] = {m: float(np.concatenate(v).mean()) for m, v in vals.items()}
        if discriminator is not None:
            result[kind].update({m: v / n for m, v in losses.items()})
    return result
