"""The SRGAN generator in train mode without a GPU: tests/srgan_train_oracle.py (the float64 restatement the GPU tests of
cid_sr_forward_train measure against) held to a stock train-mode nn.Sequential restatement on ATen fp32, the conditioning of the GPU
parity inputs, the host argument checks of cid_sr_train_* (include/cid.h) and the opt-in flag of the module."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth
from celebrity_image_denoiser_amd.discriminator import _BnArg
from celebrity_image_denoiser_amd.srgan import SRGANGenerator

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import srgan_train_oracle as oracle  # noqa: E402

ERR_INVALID, ERR_SHAPE, ERR_KEY, ERR_STATE, ERR_WORKSPACE = 1, 2, 3, 4, 5
CUSTOM_BN = {"res_blocks.1.4": {"eps": 1e-3, "momentum": 0.4}, "res_blocks.3.1": {"momentum": None}}


@pytest.mark.parametrize("bn", [None, CUSTOM_BN], ids=["defaults", "custom"])
@pytest.mark.parametrize("wset", ["default", "hot"])
def test_fp32_oracle_is_the_stock_train_mode_module(wset, bn):
    """Two consecutive train calls.  The oracle on fp32 and the stock layers run the same ATen kernels on the same operands (PReLU
    written as a select is exact either way), so they agree to the last bit: outputs, running tensors and counters."""
    case = (3, 8, 12, 2)
    sd = synth.make_srgan_state_dict(wset, case[3])
    x = oracle.case_input(case)
    module, run = oracle.stock_generator(sd, case[3], bn)
    before = {name: int(sd[name + ".num_batches_tracked"]) for name in oracle.BN_NAMES}
    for call in (1, 2):
        got = oracle.forward(sd, x, dtype=torch.float32, bn=bn)
        want = run(torch.from_numpy(x))
        for k in oracle.STAGES:
            assert got[k].dtype == np.float32 and np.array_equal(got[k], want[k].numpy()), (call, k)
        state = module.state_dict()
        for name in oracle.BN_NAMES:
            for k in ("running_mean", "running_var", "num_batches_tracked"):
                assert np.array_equal(got[f"{name}.{k}"], state[f"{name}.{k}"].numpy()), (call, name, k)
            assert int(got[name + ".num_batches_tracked"]) == before[name] + call
        sd = oracle.next_state_dict(sd, got)
    assert got["out"].shape == (3, 3, 16, 24) and got["tail_in"].shape == (3, 64, 16, 24)


def test_the_oracle_normalises_by_the_batch_and_tracks_the_unbiased_variance():
    """One layer by hand: res_blocks.0.1 sees z = conv(x0); its running buffers move by momentum towards the batch mean and the
    unbiased batch variance."""
    case = (3, 8, 12, 2)
    sd = synth.make_srgan_state_dict("default", 2)
    ref = oracle.reference("default", case)
    import torch.nn.functional as F

    z = F.conv2d(torch.from_numpy(ref["x0"].copy()), torch.from_numpy(sd["res_blocks.0.0.weight"]).double(),
                 torch.from_numpy(sd["res_blocks.0.0.bias"]).double(), padding=1)
    mean, var_u = z.mean((0, 2, 3)).numpy(), z.var((0, 2, 3), unbiased=True).numpy()
    old_mean, old_var = (sd[f"res_blocks.0.1.{k}"].astype(np.float64) for k in ("running_mean", "running_var"))
    assert np.allclose(ref["res_blocks.0.1.running_mean"], 0.9 * old_mean + 0.1 * mean, rtol=0, atol=1e-12)
    assert np.allclose(ref["res_blocks.0.1.running_var"], 0.9 * old_var + 0.1 * var_u, rtol=0, atol=1e-12)
    assert int(ref["res_blocks.0.1.num_batches_tracked"]) == int(sd["res_blocks.0.1.num_batches_tracked"]) + 1


@pytest.mark.parametrize("case", oracle.PARITY_CASES, ids=oracle.case_id)
@pytest.mark.parametrize("wset", ["default", "hot"])
def test_parity_inputs_are_well_conditioned(wset, case):
    """The condition under which 1e-5 * max(1, max|ref64|) is a fair bound for an fp32 implementation: ATen fp32 itself meets it on
    every GPU parity case, on x0, trunk, tail_in, pre and every running tensor.  (Batches with two values per channel do not: their
    batch variance is far below eps; they are not parity cases.)"""
    ref, r32 = oracle.reference(wset, case), oracle.reference(wset, case, torch.float32)
    worst = 0.0
    for k in ("x0", "trunk", "tail_in", "pre") + tuple(oracle.running_keys()):
        err = float(np.abs(r32[k].astype(np.float64) - ref[k]).max())
        worst = max(worst, err / oracle.bound(ref[k]))
        assert err <= oracle.bound(ref[k]), (k, err, oracle.bound(ref[k]))
    print(f"{wset} {oracle.case_id(case)}: ATen fp32 at {worst:.3f} of the bound at worst")
    sd = synth.make_srgan_state_dict(wset, case[3])
    for name in oracle.BN_NAMES:
        assert int(ref[name + ".num_batches_tracked"]) == int(sd[name + ".num_batches_tracked"]) + 1


def test_default_module_still_raises_and_the_flag_opts_in():
    m = SRGANGenerator(2)
    m.train()
    with pytest.raises(RuntimeError, match="train mode: train-mode BatchNorm \\(batch statistics\\) is not implemented"):
        m(torch.zeros(1, 3, 4, 4))
    t = SRGANGenerator(2, batch_stats=True)
    assert list(t.state_dict()) == list(m.state_dict())
    t.train()
    with pytest.raises(RuntimeError, match="GPU-only"):          # past the mode check: the CPU tensor is what is refused
        t(torch.zeros(1, 3, 4, 4))
    assert not SRGANGenerator(2, batch_stats=True).eval().training


def _handle(L, scale, sd=None):
    h = ctypes.c_void_p()
    assert L.cid_sr_create(ctypes.byref(h), scale) == 0
    for k, v in (sd or {}).items():
        a = np.ascontiguousarray(v) if np.ndim(v) else np.asarray(v)
        assert L.cid_sr_set_weight(h, k.encode(), a.ctypes.data, (ctypes.c_int64 * max(a.ndim, 1))(*a.shape), a.ndim) == 0, k
    return h


def test_c_abi_argument_errors_need_no_gpu():
    L = _lib.lib()
    h = _handle(L, 2)
    n = ctypes.c_size_t()
    a256 = lambda v: (v + 255) // 256 * 256   # noqa: E731
    t = a256(2 * 64 * 13 * 18 * 4)
    tables = a256(64 * 2 * 2 * 2 * 8) + a256(10 * 64 * 2 * 4)          # 13 x 18: 1 x 2 tiles, two images
    assert L.cid_sr_train_workspace_bytes(2, 13, 18, 1, ctypes.byref(n)) == 0 and n.value == 4 * t + tables
    assert L.cid_sr_train_workspace_bytes(2, 13, 18, 2, ctypes.byref(n)) == 0 and n.value == 4 * t + a256(4 * 2 * 64 * 13 * 18 * 4) + tables
    assert L.cid_sr_train_workspace_bytes(2, 13, 18, 4, ctypes.byref(n)) == 0
    assert n.value == 4 * t + a256(4 * 2 * 64 * 13 * 18 * 4) + a256(16 * 2 * 64 * 13 * 18 * 4) + tables
    assert L.cid_sr_train_workspace_bytes(2, 17, 33, 1, ctypes.byref(n)) == 0
    assert n.value == 4 * a256(2 * 64 * 17 * 33 * 4) + a256(64 * 2 * 2 * 6 * 8) + a256(10 * 64 * 2 * 4)   # 2 x 3 tiles
    assert L.cid_sr_train_workspace_bytes(2, 13, 18, 2, None) == ERR_INVALID
    assert L.cid_sr_train_workspace_bytes(2, 13, 18, 3, ctypes.byref(n)) == ERR_INVALID
    for bad in ((0, 8, 8, 2), (1, 0, 8, 2), (1, 8, -1, 2), (1, 1 << 15, 1 << 13, 4), (1, 1, 1, 1), (1, 1, 1, 4)):
        assert L.cid_sr_train_workspace_bytes(*bad, ctypes.byref(n)) == ERR_SHAPE, bad
    assert L.cid_sr_train_workspace_bytes(2, 1, 1, 1, ctypes.byref(n)) == 0 and L.cid_sr_train_workspace_bytes(1, 1, 2, 2, ctypes.byref(n)) == 0
    assert L.cid_sr_train_workspace_bytes(2, 13, 18, 2, ctypes.byref(n)) == 0

    fake = ctypes.c_void_p(1 << 20)                                   # aligned, never dereferenced
    odd = ctypes.c_void_p((1 << 20) + 2)
    big = 1 << 40

    def bns(**change):
        arr = (_BnArg * 10)()
        for i in range(10):
            arr[i] = _BnArg(1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1e-5, 0.1)
        for k, v in change.items():
            setattr(arr[int(k[1:].split("_", 1)[0])], k.split("_", 1)[1], v)
        return arr

    def fwd(hh, i, fi, o, fo, N, H, W, ws, nb, bn=None, flags=0):
        return L.cid_sr_forward_train(hh, i, fi, o, fo, N, H, W, flags, bns() if bn is None else bn, ws, nb, None)

    err = lambda: L.cid_sr_last_error(h)   # noqa: E731
    assert fwd(None, fake, 0, fake, 0, 1, 8, 8, fake, big) == ERR_INVALID
    assert fwd(h, None, 0, fake, 0, 1, 8, 8, fake, big) == ERR_INVALID and b"cid_sr_forward_train: null pointer" in err()
    assert fwd(h, fake, 0, None, 0, 1, 8, 8, fake, big) == ERR_INVALID and fwd(h, fake, 0, fake, 0, 1, 8, 8, None, big) == ERR_INVALID
    assert L.cid_sr_forward_train(h, fake, 0, fake, 0, 1, 8, 8, 0, None, fake, big, None) == ERR_INVALID and b"null pointer" in err()
    for layer in (0, 4, 9):                                           # each of a layer's five pointers
        for field in ("gamma", "beta", "running_mean", "running_var", "num_batches_tracked"):
            assert fwd(h, fake, 0, fake, 0, 1, 8, 8, fake, big, bn=bns(**{f"l{layer}_{field}": None})) == ERR_INVALID, (layer, field)
            assert b"null BatchNorm pointer" in err()
    for eps in (-1.0, float("nan"), float("inf")):
        assert fwd(h, fake, 0, fake, 0, 1, 8, 8, fake, big, bn=bns(l7_eps=eps)) == ERR_INVALID and b"eps" in err(), eps
    for mom in (-0.5, float("nan"), float("inf")):
        assert fwd(h, fake, 0, fake, 0, 1, 8, 8, fake, big, bn=bns(l3_momentum=mom)) == ERR_INVALID and b"momentum" in err(), mom
    assert fwd(h, fake, 2, fake, 0, 1, 8, 8, fake, big) == ERR_INVALID and fwd(h, fake, 0, fake, -1, 1, 8, 8, fake, big) == ERR_INVALID
    assert b"unknown format" in err()
    assert fwd(h, odd, 0, fake, 0, 1, 8, 8, fake, big) == ERR_INVALID and fwd(h, fake, 1, odd, 0, 1, 8, 8, fake, big) == ERR_INVALID
    assert fwd(h, fake, 0, fake, 0, 1, 8, 8, fake, big, flags=2) == ERR_INVALID and b"unknown flags" in err()
    assert fwd(h, fake, 0, fake, 1, 1, 8, 8, fake, big, flags=_lib.CID_SR_RAW) == ERR_INVALID and b"CID_SR_RAW" in err()
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-3, 8, 8)):
        assert fwd(h, fake, 0, fake, 0, *bad, fake, big) == ERR_SHAPE, bad
    assert fwd(h, fake, 0, fake, 0, 1, 1 << 15, 1 << 15, fake, big) == ERR_SHAPE          # 4 * 2^30 pixels at scale 2
    assert fwd(h, fake, 0, fake, 0, 1, 1, 1, fake, big) == ERR_SHAPE
    assert err() == b"Expected more than 1 value per channel when training"               # torch's own text
    assert fwd(h, fake, 0, fake, 0, 2, 13, 18, fake, n.value - 1) == ERR_WORKSPACE and b"cid_sr_train_workspace_bytes" in err()
    assert fwd(h, fake, 0, fake, 0, 2, 13, 18, ctypes.c_void_p((1 << 20) + 128), big) == ERR_WORKSPACE
    # the eval plan is smaller: its size does not do
    e = ctypes.c_size_t()
    assert L.cid_sr_workspace_bytes(2, 13, 18, 2, ctypes.byref(e)) == 0 and e.value < n.value
    assert fwd(h, fake, 0, fake, 0, 2, 13, 18, fake, e.value) == ERR_WORKSPACE
    assert fwd(h, odd, 1, odd, 1, 2, 13, 18, fake, n.value) == ERR_STATE and b"weights not uploaded" in err()
    assert fwd(h, fake, 0, fake, 0, 2, 13, 18, fake, n.value, bn=bns(l2_momentum=_lib.CID_DISC_MOMENTUM_NONE, l5_eps=0.0, l6_momentum=0.0),
               flags=_lib.CID_SR_RAW) == ERR_STATE
    L.cid_sr_destroy(h)


def test_train_stage_view():
    L = _lib.lib()
    off, c, hs, ws, cb = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    refs = (ctypes.byref(off), ctypes.byref(c), ctypes.byref(hs), ctypes.byref(ws), ctypes.byref(cb))
    view = lambda: (off.value, c.value, hs.value, ws.value, cb.value)   # noqa: E731
    a256 = lambda v: (v + 255) // 256 * 256   # noqa: E731
    t = a256(2 * 64 * 13 * 18 * 4)
    sv = L.cid_sr_train_stage_view
    assert sv(b"x0", 2, 13, 18, 4, *refs) == 0 and view() == (0, 64, 13, 18, 8)
    assert sv(b"trunk", 2, 13, 18, 4, *refs) == 0 and view() == (3 * t, 64, 13, 18, 8)
    assert sv(b"up1", 2, 13, 18, 4, *refs) == 0 and view() == (4 * t, 64, 26, 36, 8)
    assert sv(b"tail_in", 2, 13, 18, 4, *refs) == 0 and view() == (4 * t + a256(4 * 2 * 64 * 13 * 18 * 4), 64, 52, 72, 8)
    assert sv(b"tail_in", 2, 13, 18, 2, *refs) == 0 and view() == (4 * t, 64, 26, 36, 8)
    assert sv(b"tail_in", 2, 13, 18, 1, *refs) == 0 and view() == (3 * t, 64, 13, 18, 8)          # no stage: the trunk
    assert sv(b"up2", 2, 13, 18, 8, *refs) == 0 and view()[1:] == (64, 52, 72, 8)
    assert sv(b"up1", 2, 13, 18, 2, *refs) == ERR_KEY and sv(b"up2", 2, 13, 18, 4, *refs) == ERR_KEY
    assert sv(b"z", 2, 13, 18, 4, *refs) == ERR_KEY and sv(None, 2, 13, 18, 4, *refs) == ERR_INVALID
    assert sv(b"x0", 2, 13, 18, 4, None, *refs[1:]) == ERR_INVALID
    assert sv(b"x0", 0, 13, 18, 4, *refs) == ERR_SHAPE and sv(b"x0", 1, 1, 1, 4, *refs) == ERR_SHAPE
    assert sv(b"x0", 2, 13, 18, 5, *refs) == ERR_INVALID
