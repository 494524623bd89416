"""CPU restatement of the ESRGAN trainer's discriminator (Discriminator, reference backend/trainingcode/esrgan_code/models.py:36-71)
for tests/test_esrgan_disc_host.py and tests/test_esrgan_disc.py.

    StockESRGANDiscriminator(input_shape)   the reference's structure with stock layers
    restate(sd, x)                          ([a1, a2, a3, a4], logits [N,1]) with torch.nn.functional in x's dtype
    weights(kind, shape)                    "default" / "trained" state_dict (CPU fp32 tensors) for input (H, W), built once
    images(N, H, W)                         (uint8 [N,H,W,3], fp32 [N,3,H,W] in [0,1]): ToTensor()'s range, the ESRGAN trainer's
    c8_to_nchw(flat, N, C, H, W)            a C8 workspace region as [N,C,H,W]
    expected_workspace(N, H, W)             the workspace formula of include/cid.h: (offsets of a1 ... a4, total)
    bce_with_logits(x, y)                   the stable BCE-with-logits term in numpy float64
    case(kind, shape)                       the shared float64 reference of one parity case, with the two conditions on its inputs

Both weight sets come from synth.make_esrgan_disc_state_dict (hash streams, no RNG of a stock module).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from celebrity_image_denoiser_amd import synth

WSETS = ("default", "trained")
TOL = 1e-5               # the project's bound (DESIGN sections 15-17): |got - ref64| <= TOL * max(1, max|ref64|) per stage
CONDITION = TOL / 10     # what the float32 restatement itself may differ from the float64 one, per stage, for a case to be used
LOGIT_BOUND = 6.0        # "trained" logits lie in (-6, 6): BCE on its curved part


class StockESRGANDiscriminator(nn.Module):
    """The reference's structure (models.py:36-71) with stock layers."""

    def __init__(self, input_shape=(3, 256, 256)):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, kernel_size=3, stride=2, padding=1)
        self.leaky_relu = nn.LeakyReLU(0.2, inplace=True)
        self.conv2 = nn.Conv2d(64, 128, kernel_size=3, stride=2, padding=1)
        self.conv3 = nn.Conv2d(128, 256, kernel_size=3, stride=2, padding=1)
        self.conv4 = nn.Conv2d(256, 512, kernel_size=3, stride=2, padding=1)
        with torch.no_grad():
            self._shape = self._features(torch.zeros(1, *input_shape)).view(1, -1).size(1)
        self.fc = nn.Linear(self._shape, 1)

    def _features(self, x):
        for conv in (self.conv1, self.conv2, self.conv3, self.conv4):
            x = self.leaky_relu(conv(x))
        return x

    def forward(self, x):
        x = self._features(x)
        return self.fc(x.view(x.size(0), -1))


def restate(sd, x):
    """The forward in x's dtype: the four activated stages and the logits [N,1]."""
    stages = []
    y = x
    for name in ("conv1", "conv2", "conv3", "conv4"):
        y = F.leaky_relu(F.conv2d(y, sd[name + ".weight"], sd[name + ".bias"], stride=2, padding=1), 0.2)
        stages.append(y)
    logits = y.reshape(y.shape[0], -1) @ sd["fc.weight"].t() + sd["fc.bias"]
    return stages, logits


def cast(sd, dtype):
    return {k: v.to(dtype).clone() for k, v in sd.items()}


def images(n, h, w, first_index=0):
    """Noisy face-like batches: uint8 [n,h,w,3] and its ToTensor() copy, fp32 [n,3,h,w] = u / 255 with a true division."""
    u8 = synth.add_gaussian_noise(synth.clean_images_u8(n, h, w, first_index), 25.0, first_index)
    x = torch.from_numpy(u8).permute(0, 3, 1, 2).to(torch.float32) / 255.0
    return u8, x.contiguous()


def c8_to_nchw(flat, n, c, h, w):
    """fp32 C8 region (element (n, c, y, x) at (((n * (C/8) + c/8) * H + y) * W + x) * 8 + c % 8) -> [n,c,h,w]."""
    return flat[:n * c * h * w].view(n, c // 8, h, w, 8).permute(0, 1, 4, 2, 3).reshape(n, c, h, w)


def expected_workspace(n, h, w):
    """The formula of include/cid.h (cid_esd_workspace_bytes): (offsets of a1 ... a4, total)."""
    offs, at = [], 0
    for c in (64, 128, 256, 512):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        offs.append(at)
        at += (4 * n * c * h * w + 255) // 256 * 256
    return offs, at


def bce_with_logits(x, y):
    """The stable form the kernels use, in numpy float64: max(x, 0) - x*y + log1p(exp(-|x|))."""
    x = np.asarray(x, np.float64)
    return np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))


_WEIGHTS = {}


def weights(kind, shape, seed=synth.WEIGHT_SEED):
    """state_dict (CPU fp32 tensors) of a weight set for input (H, W) = shape; a fresh copy each call."""
    key = (kind, tuple(shape), seed)
    if key not in _WEIGHTS:
        sd = synth.make_esrgan_disc_state_dict(kind, (3, shape[0], shape[1]), seed)
        _WEIGHTS[key] = {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    return {k: v.clone() for k, v in _WEIGHTS[key].items()}


_CASES = {}


def case(kind, shape):
    """(uint8 batch, fp32 batch, float64 stages, float64 logits) of a parity case (N, H, W): computed once, shared, never modified.
    The reference alone decides whether the case can carry the bound: the float32 restatement (ATen on the CPU) must be within
    CONDITION * max(1, max|ref64|) of the float64 one at every stage, which leaves nine tenths of TOL to the code under test, and the
    "trained" logits must lie in (-LOGIT_BOUND, LOGIT_BOUND)."""
    key = (kind, tuple(shape))
    if key not in _CASES:
        n, h, w = shape
        u8, x = images(n, h, w, first_index=n + h + w)
        sd = weights(kind, (h, w))
        st64, lg64 = restate(cast(sd, torch.float64), x.double())
        st32, lg32 = restate(sd, x)
        for name, a, b in zip(("a1", "a2", "a3", "a4", "logits"), st64 + [lg64], st32 + [lg32]):
            own = float((a - b.double()).abs().max())
            bound = CONDITION * max(1.0, float(a.abs().max()))
            assert own <= bound, f"{key} {name}: the float32 restatement is {own:.2e} from float64, above {bound:.2e}"
        if kind == "trained":
            assert float(lg64.abs().max()) < LOGIT_BOUND, f"{key}: trained logits reach {float(lg64.abs().max()):.2f}"
        _CASES[key] = (u8, x, st64, lg64)
    return _CASES[key]
