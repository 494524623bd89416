"""The ESRGAN generator in train mode without a GPU: tests/esrgan_train_oracle.py (the float64 restatement the GPU tests of
cid_esr_forward_train measure against) held to a stock train-mode restatement on ATen fp32, the conditioning of the GPU parity
inputs, the host argument checks of cid_esr_train_* (include/cid.h) and the opt-in flag of the module."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth
from celebrity_image_denoiser_amd.discriminator import _BnArg
from celebrity_image_denoiser_amd.esrgan import ESRGANGenerator

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import esrgan_train_oracle as oracle  # noqa: E402

ERR_INVALID, ERR_SHAPE, ERR_KEY, ERR_STATE, ERR_WORKSPACE = 1, 2, 3, 4, 5
CUSTOM_BN = {"residuals.1.block.4": {"eps": 1e-3, "momentum": 0.4}, "residuals.2.block.1": {"momentum": None}}
CAP = 1.0 / 3.0   # ATen fp32's share of the bound on a GPU parity case: the project's 3x margin


@pytest.mark.parametrize("bn", [None, CUSTOM_BN], ids=["defaults", "custom"])
@pytest.mark.parametrize("wset", ["default", "hot"])
def test_fp32_oracle_is_the_stock_train_mode_module(wset, bn):
    """Two consecutive train calls.  The oracle on fp32 and the stock layers run the same ATen kernels on the same operands (PReLU
    written as a select is exact either way), so they agree to the last bit: outputs, running tensors and counters."""
    case, R = (3, 8, 12), 3
    sd = synth.make_esrgan_state_dict(wset, R)
    x = oracle.case_input(case)
    module, run = oracle.stock_generator(sd, R, bn)
    names = oracle.BN_NAMES(R)
    before = {name: int(sd[name + ".num_batches_tracked"]) for name in names}
    for call in (1, 2):
        got = oracle.forward(sd, x, R, dtype=torch.float32, bn=bn)
        want = run(torch.from_numpy(x))
        for k in oracle.STAGES:
            assert got[k].dtype == np.float32 and np.array_equal(got[k], want[k].numpy()), (call, k)
        state = module.state_dict()
        for name in names:
            for k in ("running_mean", "running_var", "num_batches_tracked"):
                assert np.array_equal(got[f"{name}.{k}"], state[f"{name}.{k}"].numpy()), (call, name, k)
            assert int(got[name + ".num_batches_tracked"]) == before[name] + call
        sd = oracle.next_state_dict(sd, got, R)
    assert got["out"].shape == (3, 3, 8, 12) and got["tail_in"].shape == (3, 64, 8, 12)
    assert len(names) == 2 * R and names[:3] == ("residuals.0.block.1", "residuals.0.block.4", "residuals.1.block.1")


def test_the_oracle_normalises_by_the_batch_and_tracks_the_unbiased_variance():
    """One layer by hand: residuals.0.block.1 sees z = conv(x1); its running buffers move by momentum towards the batch mean and the
    unbiased batch variance.  And the skip is in the graph: without it the tail's input is another tensor."""
    case = (3, 8, 12)
    sd = synth.make_esrgan_state_dict("default", 8)
    ref = oracle.reference("default", case)
    import torch.nn.functional as F

    z = F.conv2d(torch.from_numpy(ref["x1"].copy()), torch.from_numpy(sd["residuals.0.block.0.weight"]).double(),
                 torch.from_numpy(sd["residuals.0.block.0.bias"]).double(), padding=1)
    mean, var_u = z.mean((0, 2, 3)).numpy(), z.var((0, 2, 3), unbiased=True).numpy()
    old_mean, old_var = (sd[f"residuals.0.block.1.{k}"].astype(np.float64) for k in ("running_mean", "running_var"))
    assert np.allclose(ref["residuals.0.block.1.running_mean"], 0.9 * old_mean + 0.1 * mean, rtol=0, atol=1e-12)
    assert np.allclose(ref["residuals.0.block.1.running_var"], 0.9 * old_var + 0.1 * var_u, rtol=0, atol=1e-12)
    assert int(ref["residuals.0.block.1.num_batches_tracked"]) == int(sd["residuals.0.block.1.num_batches_tracked"]) + 1
    plain = oracle.forward(sd, oracle.case_input(case), 8, skip=False)
    assert np.abs(plain["tail_in"] - ref["tail_in"]).max() > 100 * oracle.bound(ref["tail_in"])


@pytest.mark.parametrize("rc", oracle.GPU_PARITY + [(1, (2, 17, 33))], ids=lambda rc: f"R{rc[0]}-{oracle.case_id(rc[1])}")
@pytest.mark.parametrize("wset", ["default", "hot"])
def test_parity_inputs_are_well_conditioned(wset, rc):
    """The condition under which 1e-5 * max(1, max|ref64|) is a fair bound for an fp32 implementation: ATen fp32 itself stays within
    a third of it on every GPU parity case, on x1, every block's output, tail_in, out and every running tensor.  (Batches with two
    values per channel do not: they are not parity cases.)"""
    R, case = rc
    ref, r32 = oracle.reference(wset, case, R), oracle.reference(wset, case, R, torch.float32)
    worst = 0.0
    for k in ("x1", "tail_in", "out") + tuple(f"r.{i}" for i in range(R)) + tuple(oracle.running_keys(R)):
        err = float(np.abs(r32[k].astype(np.float64) - ref[k]).max())
        worst = max(worst, err / oracle.bound(ref[k]))
        assert err <= CAP * oracle.bound(ref[k]), (k, err, oracle.bound(ref[k]))
    print(f"{wset} R={R} {oracle.case_id(case)}: ATen fp32 at {worst:.3f} of the bound at worst")
    sd = synth.make_esrgan_state_dict(wset, R)
    for name in oracle.BN_NAMES(R):
        assert int(ref[name + ".num_batches_tracked"]) == int(sd[name + ".num_batches_tracked"]) + 1


def test_default_module_still_raises_and_the_flag_opts_in():
    m = ESRGANGenerator(2)
    m.train()
    with pytest.raises(RuntimeError, match="train mode: train-mode BatchNorm \\(batch statistics\\) is not implemented"):
        m(torch.zeros(1, 3, 4, 4))
    t = ESRGANGenerator(2, batch_stats=True)
    assert list(t.state_dict()) == list(m.state_dict())
    t.train()
    with pytest.raises(RuntimeError, match="GPU-only"):          # past the mode check: the CPU tensor is what is refused
        t(torch.zeros(1, 3, 4, 4))
    assert not ESRGANGenerator(2, batch_stats=True).eval().training


def _handle(L, R):
    h = ctypes.c_void_p()
    assert L.cid_esr_create(ctypes.byref(h), R) == 0
    return h


def test_c_abi_argument_errors_need_no_gpu():
    L = _lib.lib()
    R = 3
    h = _handle(L, R)
    n = ctypes.c_size_t()
    a256 = lambda v: (v + 255) // 256 * 256   # noqa: E731
    size = lambda N, H, W, tiles, r: 5 * a256(N * 64 * H * W * 4) + a256(64 * 2 * N * tiles * 8) + 2 * r * a256(64 * 2 * 4)   # noqa: E731
    wb = L.cid_esr_train_workspace_bytes
    assert wb(2, 13, 18, 3, ctypes.byref(n)) == 0 and n.value == size(2, 13, 18, 2, 3)            # 1 x 2 tiles, two images
    assert wb(2, 17, 33, 16, ctypes.byref(n)) == 0 and n.value == size(2, 17, 33, 6, 16)          # 2 x 3 tiles
    assert wb(1, 5, 7, 0, ctypes.byref(n)) == 0 and n.value == size(1, 5, 7, 1, 0)
    assert wb(1, 5, 7, 1, ctypes.byref(n)) == 0 and n.value == size(1, 5, 7, 1, 1)
    assert wb(2, 13, 18, 3, None) == ERR_INVALID
    assert wb(2, 13, 18, -1, ctypes.byref(n)) == ERR_INVALID and wb(2, 13, 18, 17, ctypes.byref(n)) == ERR_INVALID
    for bad in ((0, 8, 8, 3), (1, 0, 8, 3), (1, 8, -1, 3), (1, 1 << 16, 1 << 15, 3), (1, 1, 1, 1), (1, 1, 1, 16)):
        assert wb(*bad, ctypes.byref(n)) == ERR_SHAPE, bad
    assert wb(1, 1, 1, 0, ctypes.byref(n)) == 0                       # no block, no BatchNorm: one value per channel is fine
    assert wb(2, 1, 1, 3, ctypes.byref(n)) == 0 and wb(1, 1, 2, 3, ctypes.byref(n)) == 0
    assert wb(2, 13, 18, 3, ctypes.byref(n)) == 0

    fake = ctypes.c_void_p(1 << 20)                                   # aligned, never dereferenced
    odd = ctypes.c_void_p((1 << 20) + 2)
    big = 1 << 40

    def bns(**change):
        arr = (_BnArg * (2 * R))()
        for i in range(2 * R):
            arr[i] = _BnArg(1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1e-5, 0.1)
        for k, v in change.items():
            setattr(arr[int(k[1:].split("_", 1)[0])], k.split("_", 1)[1], v)
        return arr

    def fwd(hh, i, fi, o, fo, N, H, W, ws, nb, bn=None):
        return L.cid_esr_forward_train(hh, i, fi, o, fo, N, H, W, bns() if bn is None else bn, ws, nb, None)

    err = lambda: L.cid_esr_last_error(h)   # noqa: E731
    assert fwd(None, fake, 0, fake, 0, 1, 8, 8, fake, big) == ERR_INVALID
    assert fwd(h, None, 0, fake, 0, 1, 8, 8, fake, big) == ERR_INVALID and b"cid_esr_forward_train: null pointer" in err()
    assert fwd(h, fake, 0, None, 0, 1, 8, 8, fake, big) == ERR_INVALID and fwd(h, fake, 0, fake, 0, 1, 8, 8, None, big) == ERR_INVALID
    assert L.cid_esr_forward_train(h, fake, 0, fake, 0, 1, 8, 8, None, fake, big, None) == ERR_INVALID and b"null pointer" in err()
    for layer in (0, 3, 5):                                           # each of a layer's five pointers
        for field in ("gamma", "beta", "running_mean", "running_var", "num_batches_tracked"):
            assert fwd(h, fake, 0, fake, 0, 1, 8, 8, fake, big, bn=bns(**{f"l{layer}_{field}": None})) == ERR_INVALID, (layer, field)
            assert b"null BatchNorm pointer" in err()
    for eps in (-1.0, float("nan"), float("inf")):
        assert fwd(h, fake, 0, fake, 0, 1, 8, 8, fake, big, bn=bns(l4_eps=eps)) == ERR_INVALID and b"eps" in err(), eps
    for mom in (-0.5, float("nan"), float("inf")):
        assert fwd(h, fake, 0, fake, 0, 1, 8, 8, fake, big, bn=bns(l3_momentum=mom)) == ERR_INVALID and b"momentum" in err(), mom
    assert fwd(h, fake, 2, fake, 0, 1, 8, 8, fake, big) == ERR_INVALID and fwd(h, fake, 0, fake, -1, 1, 8, 8, fake, big) == ERR_INVALID
    assert b"unknown format" in err()
    assert fwd(h, odd, 0, fake, 0, 1, 8, 8, fake, big) == ERR_INVALID and fwd(h, fake, 1, odd, 0, 1, 8, 8, fake, big) == ERR_INVALID
    assert b"misaligned fp32 operand" in err()
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-3, 8, 8)):
        assert fwd(h, fake, 0, fake, 0, *bad, fake, big) == ERR_SHAPE, bad
    assert fwd(h, fake, 0, fake, 0, 1, 1 << 16, 1 << 15, fake, big) == ERR_SHAPE          # 2^31 pixels
    assert fwd(h, fake, 0, fake, 0, 1, 1, 1, fake, big) == ERR_SHAPE
    assert err() == b"Expected more than 1 value per channel when training"               # torch's own text
    assert fwd(h, fake, 0, fake, 0, 2, 13, 18, fake, n.value - 1) == ERR_WORKSPACE and b"cid_esr_train_workspace_bytes" in err()
    assert fwd(h, fake, 0, fake, 0, 2, 13, 18, ctypes.c_void_p((1 << 20) + 128), big) == ERR_WORKSPACE
    # the eval plan is smaller: its size does not do
    e = ctypes.c_size_t()
    assert L.cid_esr_workspace_bytes(2, 13, 18, ctypes.byref(e)) == 0 and e.value < n.value
    assert fwd(h, fake, 0, fake, 0, 2, 13, 18, fake, e.value) == ERR_WORKSPACE
    assert fwd(h, odd, 1, odd, 1, 2, 13, 18, fake, n.value) == ERR_STATE and b"weights not uploaded" in err()
    assert fwd(h, fake, 0, fake, 0, 2, 13, 18, fake, n.value,
               bn=bns(l2_momentum=_lib.CID_DISC_MOMENTUM_NONE, l5_eps=0.0, l1_momentum=0.0)) == ERR_STATE
    L.cid_esr_destroy(h)

    # no block: no BatchNorm to describe, and one value per channel passes the checks
    h0 = _handle(L, 0)
    assert wb(1, 1, 1, 0, ctypes.byref(n)) == 0
    assert L.cid_esr_forward_train(h0, fake, 0, fake, 0, 1, 1, 1, None, fake, n.value, None) == ERR_STATE
    assert L.cid_esr_forward_train(h0, fake, 0, fake, 0, 1, 1, 1, None, fake, n.value - 1, None) == ERR_WORKSPACE
    L.cid_esr_destroy(h0)


def test_train_stage_view():
    L = _lib.lib()
    off, c, hs, ws, cb = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    refs = (ctypes.byref(off), ctypes.byref(c), ctypes.byref(hs), ctypes.byref(ws), ctypes.byref(cb))
    view = lambda: (off.value, c.value, hs.value, ws.value, cb.value)   # noqa: E731
    a256 = lambda v: (v + 255) // 256 * 256   # noqa: E731
    t = a256(2 * 64 * 13 * 18 * 4)
    sv = L.cid_esr_train_stage_view
    assert sv(b"x1", 2, 13, 18, 8, *refs) == 0 and view() == (0, 64, 13, 18, 8)
    # the tail's input takes the tensor the last block's input is not in: r[(R - 1) % 2]
    for R, slot in ((0, 0), (1, 0), (2, 1), (3, 0), (8, 1), (16, 1)):
        assert sv(b"tail_in", 2, 13, 18, R, *refs) == 0 and view() == ((3 + slot) * t, 64, 13, 18, 8), R
    assert sv(b"x2", 2, 13, 18, 8, *refs) == ERR_KEY and sv(b"z", 2, 13, 18, 8, *refs) == ERR_KEY
    assert sv(None, 2, 13, 18, 8, *refs) == ERR_INVALID and sv(b"x1", 2, 13, 18, 8, None, *refs[1:]) == ERR_INVALID
    assert sv(b"x1", 0, 13, 18, 8, *refs) == ERR_SHAPE and sv(b"x1", 1, 1, 1, 8, *refs) == ERR_SHAPE
    assert sv(b"x1", 1, 1, 1, 0, *refs) == 0
    assert sv(b"x1", 2, 13, 18, 17, *refs) == ERR_INVALID
