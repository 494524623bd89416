"""Float64 restatement of the server's ESRGANGenerator forward (reference backend/app.py:188-218, eval mode) with torch.nn.functional
on the CPU: the reference the GPU tests of cid_esr_forward measure against.  `dtype=torch.float32` gives the same graph on ATen fp32,
the reference's own arithmetic."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5   # nn.BatchNorm2d's default, which the reference's blocks keep
TOL = 1e-5   # the project's per-stage rule: max|delta| <= TOL * max(1, max|ref64|) per tensor


def forward(sd, x, num_residuals, dtype=torch.float64, eps=EPS, taps=None):
    """sd: state_dict of numpy arrays or tensors; x: [N,3,H,W] in [0,1] -> {"x1", "x2", "tail_in", "out"} as numpy arrays of `dtype`.
    `taps`, if a dict, receives "pre.initial" and "pre.<i>": the tensors each PReLU is applied to."""
    t = {k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}
    p = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in t.items()}
    prelu = lambda v, a: torch.where(v > 0, v, a * v)   # noqa: E731
    x = torch.from_numpy(np.array(x)).to(dtype)
    with torch.no_grad():
        pre = F.conv2d(x, p["initial.0.weight"], p["initial.0.bias"], padding=4)
        if taps is not None:
            taps["pre.initial"] = pre.numpy()
        x1 = prelu(pre, p["initial.1.weight"])
        cur = x1
        for i in range(num_residuals):
            b = f"residuals.{i}.block."
            bn = lambda v, j: F.batch_norm(v, p[f"{b}{j}.running_mean"], p[f"{b}{j}.running_var"], p[f"{b}{j}.weight"],   # noqa: E731
                                           p[f"{b}{j}.bias"], False, 0.0, eps)
            pre = bn(F.conv2d(cur, p[b + "0.weight"], p[b + "0.bias"], padding=1), 1)
            if taps is not None:
                taps[f"pre.{i}"] = pre.numpy()
            mid = prelu(pre, p[b + "2.weight"])
            cur = cur + bn(F.conv2d(mid, p[b + "3.weight"], p[b + "3.bias"], padding=1), 4)
        tail_in = x1 + cur
        out = F.conv2d(tail_in, p["final.weight"], p["final.bias"], padding=4)
    return {"x1": x1.numpy(), "x2": cur.numpy(), "tail_in": tail_in.numpy(), "out": out.numpy()}


def to_u8(out):
    """The server's view of an output (postprocess_tensor, app.py:251-254): clamp(0,1) -> ToPILImage = mul(255).byte(), [N,H,W,3]."""
    t = torch.from_numpy(np.array(out, dtype=np.float32))
    return t.clamp(0, 1).mul(255).byte().permute(0, 2, 3, 1).contiguous().numpy()


def bound(ref64):
    return TOL * max(1.0, float(np.abs(ref64).max()))
