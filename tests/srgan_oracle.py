"""Float64 restatement of the server's SRGANGenerator forward (reference backend/app.py:145-186, eval mode) with torch.nn.functional
on the CPU: the reference the GPU tests of cid_sr_forward measure against.  `dtype=torch.float32` gives the same graph on ATen fp32,
the reference's own arithmetic."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5   # nn.BatchNorm2d's default, which the reference's blocks keep
TOL = 1e-5   # the project's per-stage rule: max|delta| <= TOL * max(1, max|ref64|) per tensor
NUM_BLOCKS = 5


def stages_of(sd):
    return sum(1 for k in sd if k.startswith("upscale.") and k.endswith(".bias"))


def forward(sd, x, dtype=torch.float64, eps=EPS, taps=None):
    """sd: state_dict of numpy arrays or tensors (the number of upscale stages is read from its keys); x: [N,3,H,W] in [-1,1], already
    padded -> {"x0", "res", "trunk", "up1", ..., "tail_in", "pre", "out"} as numpy arrays of `dtype`: res = res_blocks(x0),
    trunk = mid(res) + x0, up<k> the k-th upscale stage's output, tail_in the last of them (trunk with no stage), pre the sum before
    tanh.  `taps`, if a dict, receives the tensors each PReLU is applied to: "pre.initial", "pre.<i>" (block i), "pre.up<k>"."""
    t = {k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}
    p = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in t.items()}
    prelu = lambda v, a: torch.where(v > 0, v, a * v)   # noqa: E731
    x = torch.from_numpy(np.array(x)).to(dtype)
    out = {}
    with torch.no_grad():
        pre = F.conv2d(x, p["initial.0.weight"], p["initial.0.bias"], padding=4)
        if taps is not None:
            taps["pre.initial"] = pre.numpy()
        x0 = prelu(pre, p["initial.1.weight"])
        cur = x0
        for i in range(NUM_BLOCKS):   # plain nn.Sequential blocks: no skip
            b = f"res_blocks.{i}."
            bn = lambda v, j: F.batch_norm(v, p[f"{b}{j}.running_mean"], p[f"{b}{j}.running_var"], p[f"{b}{j}.weight"],   # noqa: E731
                                           p[f"{b}{j}.bias"], False, 0.0, eps)
            pre = bn(F.conv2d(cur, p[b + "0.weight"], p[b + "0.bias"], padding=1), 1)
            if taps is not None:
                taps[f"pre.{i}"] = pre.numpy()
            cur = bn(F.conv2d(prelu(pre, p[b + "2.weight"]), p[b + "3.weight"], p[b + "3.bias"], padding=1), 4)
        out["x0"], out["res"] = x0.numpy(), cur.numpy()
        u = F.conv2d(cur, p["mid.weight"], p["mid.bias"], padding=1) + x0
        out["trunk"] = u.numpy()
        for k in range(stages_of(sd)):
            pre = F.pixel_shuffle(F.conv2d(u, p[f"upscale.{3 * k}.weight"], p[f"upscale.{3 * k}.bias"], padding=1), 2)
            if taps is not None:
                taps[f"pre.up{k + 1}"] = pre.numpy()
            u = prelu(pre, p[f"upscale.{3 * k + 2}.weight"])
            out[f"up{k + 1}"] = u.numpy()
        out["tail_in"] = u.numpy()
        pre = F.conv2d(u, p["final.weight"], p["final.bias"], padding=4)
        out["pre"] = pre.numpy()
        out["out"] = torch.tanh(pre).numpy()
    return out


def pad_input(x, padding, fill=-1.0):
    """[N,3,H,W] -> the server's Pad(fill=0) after Normalize(0.5, 0.5): a band of -1.0; padding = (left, top, right, bottom)."""
    pl, pt, pr, pb = padding
    return np.pad(np.asarray(x), ((0, 0), (0, 0), (pt, pb), (pl, pr)), constant_values=fill)


def normalise_u8(u8):
    """uint8 [N,H,W,3] -> fp32 [N,3,H,W]: ToTensor + Normalize(0.5, 0.5) with true divisions in fp32."""
    x = (u8.astype(np.float32) / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def to_u8(out):
    """The server's view of an output (app.py:435, 472): y * 0.5 + 0.5 -> clamp(0,1) -> ToPILImage = mul(255).byte(), [N,H,W,3].
    The output is rounded to fp32 FIRST and the view applied in fp32, as the server does: in float64 tanh(10) * 0.5 + 0.5 stays below
    1 and truncates to 254 where fp32 gives 255."""
    t = torch.from_numpy(np.array(out).astype(np.float32))
    return (t * 0.5 + 0.5).clamp(0, 1).mul(255).byte().permute(0, 2, 3, 1).contiguous().numpy()


def bound(ref64):
    return TOL * max(1.0, float(np.abs(ref64).max()))
