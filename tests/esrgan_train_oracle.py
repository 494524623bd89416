"""Float64 restatement of the ESRGAN generator's forward in TRAIN mode (reference backend/trainingcode/esrgan_code/models.py:6-45 as the
trainer calls it, esrgan_train.py:89-121 after G.train()) with torch.nn.functional on the CPU: every BatchNorm runs
F.batch_norm(..., training=True, momentum, eps), which normalises with the batch statistics and updates the running buffers, and every
block adds its input (ResidualBlock.forward is x + block(x)).  The reference the GPU tests of cid_esr_forward_train measure against;
`dtype=torch.float32` gives the same graph on ATen fp32, the reference's own arithmetic."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import esrgan_oracle

EPS = 1e-5        # nn.BatchNorm2d's defaults, which the reference's blocks keep
MOMENTUM = 0.1
STAGES = ("x1", "tail_in", "out")


def BN_NAMES(num_residuals):
    return tuple(f"residuals.{i}.block.{j}" for i in range(num_residuals) for j in (1, 4))


def running_keys(num_residuals):
    return [f"{b}.{k}" for b in BN_NAMES(num_residuals) for k in ("running_mean", "running_var")]


def forward(sd, x, num_residuals, dtype=torch.float64, bn=None, skip=True):
    """sd: state_dict of numpy arrays or tensors; x: [N,3,H,W] in [0,1]; bn: {"residuals.i.block.j": {"eps": e, "momentum": m}} for the
    layers that do not keep the defaults (momentum None: the cumulative average, factor 1 / num_batches_tracked after the increment)
    -> {"x1", "tail_in", "out"}, every block's output as "r.<i>" and, under their state_dict keys, the updated running tensors (numpy
    arrays of `dtype`) and num_batches_tracked (int64).  `skip=False` drops the blocks' skips (a plain nn.Sequential trunk): what a
    test of the skip compares with."""
    bn = bn or {}
    t = {k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}
    p = {k: (v.to(dtype).clone() if v.dtype.is_floating_point else v.clone()) for k, v in t.items()}
    prelu = lambda v, a: torch.where(v > 0, v, a * v)   # noqa: E731
    x = torch.from_numpy(np.array(x)).to(dtype)
    out = {}

    def batch_norm(v, name):
        cfg = bn.get(name, {})
        count = p[name + ".num_batches_tracked"] + 1
        momentum = cfg.get("momentum", MOMENTUM)
        factor = 1.0 / float(count) if momentum is None else float(momentum)
        y = F.batch_norm(v, p[name + ".running_mean"], p[name + ".running_var"], p[name + ".weight"], p[name + ".bias"], True, factor,
                         cfg.get("eps", EPS))
        p[name + ".num_batches_tracked"] = count
        return y

    with torch.no_grad():
        x1 = prelu(F.conv2d(x, p["initial.0.weight"], p["initial.0.bias"], padding=4), p["initial.1.weight"])
        cur = x1
        for i in range(num_residuals):
            b = f"residuals.{i}.block."
            y = batch_norm(F.conv2d(cur, p[b + "0.weight"], p[b + "0.bias"], padding=1), b + "1")
            y = batch_norm(F.conv2d(prelu(y, p[b + "2.weight"]), p[b + "3.weight"], p[b + "3.bias"], padding=1), b + "4")
            cur = cur + y if skip else y
            out[f"r.{i}"] = cur.numpy()
        tail_in = x1 + cur
        out["x1"], out["tail_in"] = x1.numpy(), tail_in.numpy()
        out["out"] = F.conv2d(tail_in, p["final.weight"], p["final.bias"], padding=4).numpy()
    for name in BN_NAMES(num_residuals):
        for k in ("running_mean", "running_var", "num_batches_tracked"):
            out[f"{name}.{k}"] = p[f"{name}.{k}"].numpy()
    return out


def next_state_dict(sd, result, num_residuals):
    """`sd` with the running tensors and counters a forward returned: the state the next train call starts from."""
    nxt = dict(sd)
    for name in BN_NAMES(num_residuals):
        for k in ("running_mean", "running_var", "num_batches_tracked"):
            nxt[f"{name}.{k}"] = result[f"{name}.{k}"]
    return nxt


class _Block(nn.Module):
    """The reference's ResidualBlock: stock layers under `block`, forward x + block(x)."""

    def __init__(self):
        super().__init__()
        self.block = nn.Sequential(nn.Conv2d(64, 64, 3, 1, 1), nn.BatchNorm2d(64), nn.PReLU(), nn.Conv2d(64, 64, 3, 1, 1),
                                   nn.BatchNorm2d(64))

    def forward(self, x):
        return x + self.block(x)


def stock_generator(sd, num_residuals, bn=None):
    """The reference class restated with stock torch.nn layers (the reference's names), fp32 on the CPU, loaded with `sd`, in train
    mode: what ATen itself computes.  Returns (module, forward function)."""
    bn = bn or {}
    m = nn.Module()
    m.initial = nn.Sequential(nn.Conv2d(3, 64, 9, 1, 4), nn.PReLU())
    m.residuals = nn.Sequential(*[_Block() for _ in range(num_residuals)])
    m.final = nn.Conv2d(64, 3, 9, 1, 4)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    for name, cfg in bn.items():
        layer = m.get_submodule(name)
        layer.eps = cfg.get("eps", layer.eps)
        layer.momentum = cfg.get("momentum", layer.momentum)
    m.train()

    def run(x):
        with torch.no_grad():
            x1 = m.initial(x)
            tail_in = x1 + m.residuals(x1)
            return {"x1": x1, "tail_in": tail_in, "out": m.final(tail_in)}

    return m, run


def bound(ref64):
    return esrgan_oracle.bound(ref64)


# The parity cases of the GPU tests, (N, H, W), whose conditioning test_esrgan_train_host.py asserts without a GPU.  5x7: one partial
# tile; 2x16x16: an exact tile, two slab rows; 13x18: two tiles across; 3x8x12: three images; 20x36: 2 x 3 tiles; 2x17x33: one-pixel
# remnants on both axes, two images.  R = 8 runs all six; R = 1, 2 and 16 run SMALL_CASES (R = 1 also the last one on the host).
PARITY_CASES = [(1, 5, 7), (2, 16, 16), (1, 13, 18), (3, 8, 12), (1, 20, 36), (2, 17, 33)]
SMALL_CASES = [(1, 5, 7), (3, 8, 12)]
GPU_PARITY = [(8, c) for c in PARITY_CASES] + [(r, c) for r in (1, 2, 16) for c in SMALL_CASES]
_FIRST = {c: 2600 + 10 * i for i, c in enumerate(PARITY_CASES + [(2, 1, 1), (1, 1, 2), (1, 2, 2)])}
_REFS = {}


def case_id(case):
    return "x".join(map(str, case))


def case_input(case):
    """fp32 [N,3,H,W] in [0,1]: the /255 view of the case's synthetic uint8 batch."""
    from celebrity_image_denoiser_amd import synth

    u8 = synth.esrgan_inputs_u8(*case, _FIRST[case])
    return np.ascontiguousarray(u8.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0)


def reference(wset, case, num_residuals=8, dtype=torch.float64):
    """forward() of one case on the synthetic weight set `wset`: computed once, shared, never modified."""
    from celebrity_image_denoiser_amd import synth

    key = (wset, case, num_residuals, dtype)
    if key not in _REFS:
        ref = forward(synth.make_esrgan_state_dict(wset, num_residuals), case_input(case), num_residuals, dtype=dtype)
        for v in ref.values():
            v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]
