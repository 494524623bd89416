"""The trainer's optimizer (reference training.py:239-242: torch.optim.Adam, default flags) on the device: one cid_adam_step launch
per parameter group instead of torch's multi-tensor launches, with a fixed expression tree (include/cid.h; synth.adam_step_np
restates it)."""
from __future__ import annotations

import ctypes
from collections.abc import Mapping

import numpy as np
import torch

from . import _lib

__all__ = ["Adam"]

# the flags of torch.optim.Adam this optimizer does not implement; they stay in the groups with torch's defaults so that a
# state_dict moves between the two classes in both directions
_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")


def _to_tensors(obj):
    """A state_dict read by ckpt.read_checkpoint holds numpy arrays where torch.load gives tensors."""
    if isinstance(obj, np.ndarray):
        return torch.from_numpy(np.array(obj))   # own, writable copy
    if isinstance(obj, Mapping):
        return {k: _to_tensors(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_tensors(v) for v in obj)
    return obj


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) with default flags (no amsgrad, no maximize, L2 weight decay) for
    contiguous float32 parameters on the GPU.  step() is one kernel per parameter group on the current stream and makes no host
    synchronisation; it bumps the updated parameters' version counters, so DenoiseGenerator / DenoiseDiscriminator repack at
    their next forward and a step between a differentiable forward and its backward raises as for a stock optimizer.
    Per-parameter state is torch's (`step`: float32 scalar on the CPU; `exp_avg`, `exp_avg_sq`: float32 on the parameter's device):
    state_dict() / load_state_dict() interchange with torch.optim.Adam, and load_state_dict also takes the numpy arrays of
    ckpt.read_checkpoint(path)["g_optimizer"]."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        if isinstance(lr, torch.Tensor) or any(isinstance(b, torch.Tensor) for b in betas):
            raise ValueError("cid.Adam: lr and betas are Python numbers (tensor hyper-parameters belong to torch's capturable path)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": weight_decay, "amsgrad": False, "maximize": False,
                    "foreach": None, "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": False}
        super().__init__(params, defaults)

    def load_state_dict(self, state_dict):
        super().load_state_dict(_to_tensors(state_dict))
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)
                if not st:
                    continue
                step = st["step"]   # a Python number in checkpoints of torch < 1.12, a device tensor from a capturable optimizer
                st["step"] = torch.tensor(float(step), dtype=torch.float32)
                for key in ("exp_avg", "exp_avg_sq"):
                    st[key] = st[key].to(device=p.device, dtype=torch.float32).contiguous()

    def _plan(self):
        """-> [(group, device, [(param, grad, state)])] of at most CID_ADAM_MAX_TENSORS tensors each; raises before anything is
        launched or any state is touched."""
        calls = []
        for group in self.param_groups:
            on = [k for k in _UNSUPPORTED if group.get(k)]
            if on:
                raise NotImplementedError(f"cid.Adam: {', '.join(on)} not supported (the update is torch.optim.Adam's with default flags)")
            by_dev = {}
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("cid.Adam does not support sparse gradients")
                if p.dtype != torch.float32 or p.device.type != "cuda" or not p.is_contiguous():
                    raise RuntimeError(f"cid.Adam: parameters must be contiguous float32 tensors on the GPU, got {p.dtype} "
                                       f"{tuple(p.shape)} on {p.device}{'' if p.is_contiguous() else ' (not contiguous)'}")
                if g.dtype != torch.float32 or g.device != p.device or not g.is_contiguous() or g.shape != p.shape:
                    raise RuntimeError(f"cid.Adam: a gradient must be a contiguous float32 tensor of its parameter's shape and device, "
                                       f"got {g.dtype} {tuple(g.shape)} on {g.device} for {tuple(p.shape)} on {p.device}")
                by_dev.setdefault(p.device, []).append((p, g))
            for dev, items in by_dev.items():
                for i in range(0, len(items), _lib.CID_ADAM_MAX_TENSORS):
                    calls.append((group, dev, items[i:i + _lib.CID_ADAM_MAX_TENSORS]))
        return calls

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise RuntimeError("cid.Adam.step does not take a closure")
        L = _lib.lib()
        for group, dev, items in self._plan():
            beta1, beta2 = group["betas"]
            hp = _lib.AdamHyper(float(group["lr"]), float(beta1), float(beta2), float(group["eps"]), float(group["weight_decay"]))
            table = (_lib.AdamTensor * len(items))()
            steps, params = [], []
            for i, (p, g) in enumerate(items):
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                m, v = st["exp_avg"], st["exp_avg_sq"]
                e = table[i]
                e.param, e.grad, e.exp_avg, e.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
                e.count, e.step = p.numel(), int(st["step"].item()) + 1
                steps.append(st["step"])
                params.append(p)
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                rc = L.cid_adam_step(table, len(items), ctypes.byref(hp), stream)
            if rc != _lib.CID_OK:
                raise _lib.CidError(rc, f"cid_adam_step failed with code {rc}")
            torch._foreach_add_(steps, 1)
            # the kernel wrote through raw pointers: tell autograd and the modules' _signature() that the parameters changed
            torch.autograd.graph.increment_version(params)
        return None
