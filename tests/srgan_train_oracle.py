"""Float64 restatement of the SRGAN generator's forward in TRAIN mode (reference backend/trainingcode/srgan_code/sr_ganTrainGNew.py:19-51
after self.generator.train()) with torch.nn.functional on the CPU: every BatchNorm runs F.batch_norm(..., training=True, momentum,
eps), which normalises with the batch statistics and updates the running buffers.  The reference the GPU tests of
cid_sr_forward_train measure against; `dtype=torch.float32` gives the same graph on ATen fp32, the reference's own arithmetic."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import srgan_oracle

EPS = 1e-5        # nn.BatchNorm2d's defaults, which the reference's blocks keep
MOMENTUM = 0.1
NUM_BLOCKS = srgan_oracle.NUM_BLOCKS
BN_NAMES = tuple(f"res_blocks.{i}.{j}" for i in range(NUM_BLOCKS) for j in (1, 4))
STAGES = ("x0", "trunk", "tail_in", "pre", "out")


def running_keys():
    return [f"{b}.{k}" for b in BN_NAMES for k in ("running_mean", "running_var")]


def forward(sd, x, dtype=torch.float64, bn=None):
    """sd: state_dict of numpy arrays or tensors; x: [N,3,H,W] in [-1,1]; bn: {"res_blocks.i.j": {"eps": e, "momentum": m}} for the
    layers that do not keep the defaults (momentum None: the cumulative average, factor 1 / num_batches_tracked after the increment)
    -> {"x0", "trunk", "tail_in", "pre", "out"} and, under their state_dict keys, the twenty updated running tensors (numpy arrays of
    `dtype`) and the ten updated num_batches_tracked (int64)."""
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
        x0 = prelu(F.conv2d(x, p["initial.0.weight"], p["initial.0.bias"], padding=4), p["initial.1.weight"])
        cur = x0
        for i in range(NUM_BLOCKS):   # plain nn.Sequential blocks: no skip
            b = f"res_blocks.{i}."
            cur = batch_norm(F.conv2d(cur, p[b + "0.weight"], p[b + "0.bias"], padding=1), b + "1")
            cur = batch_norm(F.conv2d(prelu(cur, p[b + "2.weight"]), p[b + "3.weight"], p[b + "3.bias"], padding=1), b + "4")
        u = F.conv2d(cur, p["mid.weight"], p["mid.bias"], padding=1) + x0
        out["x0"], out["trunk"] = x0.numpy(), u.numpy()
        for k in range(srgan_oracle.stages_of(sd)):
            u = prelu(F.pixel_shuffle(F.conv2d(u, p[f"upscale.{3 * k}.weight"], p[f"upscale.{3 * k}.bias"], padding=1), 2),
                      p[f"upscale.{3 * k + 2}.weight"])
        out["tail_in"] = u.numpy()
        pre = F.conv2d(u, p["final.weight"], p["final.bias"], padding=4)
        out["pre"], out["out"] = pre.numpy(), torch.tanh(pre).numpy()
    for name in BN_NAMES:
        for k in ("running_mean", "running_var", "num_batches_tracked"):
            out[f"{name}.{k}"] = p[f"{name}.{k}"].numpy()
    return out


def next_state_dict(sd, result):
    """`sd` with the running tensors and counters a forward returned: the state the next train call starts from."""
    nxt = dict(sd)
    for name in BN_NAMES:
        for k in ("running_mean", "running_var", "num_batches_tracked"):
            nxt[f"{name}.{k}"] = result[f"{name}.{k}"]
    return nxt


def stock_generator(sd, scale, bn=None):
    """The reference class restated with stock torch.nn layers (nn.Sequential parts under the reference's names), fp32 on the CPU,
    loaded with `sd`, in train mode: what ATen itself computes.  Returns (module, forward function)."""
    bn = bn or {}
    m = nn.Module()
    m.initial = nn.Sequential(nn.Conv2d(3, 64, 9, 1, 4), nn.PReLU())
    m.res_blocks = nn.Sequential(*[
        nn.Sequential(nn.Conv2d(64, 64, 3, 1, 1), nn.BatchNorm2d(64), nn.PReLU(), nn.Conv2d(64, 64, 3, 1, 1), nn.BatchNorm2d(64))
        for _ in range(NUM_BLOCKS)])
    m.mid = nn.Conv2d(64, 64, 3, 1, 1)
    up = []
    for _ in range(scale.bit_length() - 1):
        up += [nn.Conv2d(64, 256, 3, 1, 1), nn.PixelShuffle(2), nn.PReLU()]
    m.upscale = nn.Sequential(*up)
    m.final = nn.Conv2d(64, 3, 9, 1, 4)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    for name, cfg in bn.items():
        layer = m.get_submodule(name)
        layer.eps = cfg.get("eps", layer.eps)
        layer.momentum = cfg.get("momentum", layer.momentum)
    m.train()

    def run(x):
        with torch.no_grad():
            x0 = m.initial(x)
            trunk = m.mid(m.res_blocks(x0)) + x0
            tail_in = m.upscale(trunk)
            pre = m.final(tail_in)
            return {"x0": x0, "trunk": trunk, "tail_in": tail_in, "pre": pre, "out": torch.tanh(pre)}

    return m, run


def bound(ref64):
    return srgan_oracle.bound(ref64)


# The parity cases of the GPU tests, (N, H, W, scale), whose conditioning test_srgan_train_host.py asserts without a GPU.  5x7: one
# partial tile; 2x16x16: an exact tile, two slab rows; 13x18 at scale 4: two tiles across, both upscale stages; 3x8x12; 20x36: 2 x 3
# tiles; 2x17x33: one-pixel remnants on both axes, two images.
PARITY_CASES = [(1, 5, 7, 2), (2, 16, 16, 1), (1, 13, 18, 4), (3, 8, 12, 2), (1, 20, 36, 1), (2, 17, 33, 1)]
_FIRST = {c: 2300 + 10 * i for i, c in enumerate(PARITY_CASES + [(2, 1, 1, 1), (1, 1, 2, 2)])}
_REFS = {}


def case_id(case):
    return "x".join(map(str, case[:3])) + f"-s{case[3]}"


def case_input(case):
    """fp32 [N,3,H,W] in [-1,1]: the normalised view of the case's synthetic uint8 batch."""
    from celebrity_image_denoiser_amd import synth

    return srgan_oracle.normalise_u8(synth.srgan_inputs_u8(*case[:3], _FIRST[case]))


def reference(wset, case, dtype=torch.float64):
    """forward() of one case on the synthetic weight set `wset`: computed once, shared, never modified."""
    from celebrity_image_denoiser_amd import synth

    key = (wset, case, dtype)
    if key not in _REFS:
        ref = forward(synth.make_srgan_state_dict(wset, case[3]), case_input(case), dtype=dtype)
        for v in ref.values():
            v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]
