"""The ESRGAN generator in train mode on the GPU: ESRGANGenerator(batch_stats=True) and cid_esr_forward_train (include/cid.h).

The reference for error is tests/esrgan_train_oracle.py in float64 (held to a stock train-mode module by test_esrgan_train_host.py,
which also asserts that ATen fp32 itself stays within a third of the bound on every parity case here).  The bound is the project's
per-stage rule, max|delta| <= 1e-5 * max(1, max|ref64|) per tensor, for x1 and tail_in (through cid_esr_train_stage_view), the output
(the raw sum: there is no tanh) and every running tensor; num_batches_tracked is exact.  Every check prints its share of the bound.

Measured on an MI355X, the largest share of the bound over the 24 parity cases: x1 0.101, tail_in 0.144, out 0.129, running tensors
0.051."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth
from celebrity_image_denoiser_amd.discriminator import named_bn_args
from celebrity_image_denoiser_amd.esrgan import load_esrgan

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import esrgan_oracle  # noqa: E402
import esrgan_train_oracle as oracle  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def train_model(sd, R, bn=None):
    """A fresh module on the GPU (each test mutates its buffers), in train mode, with the BatchNorm settings of `bn`."""
    m = load_esrgan(sd, num_residuals=R, device=DEV, strict=True, batch_stats=True)
    for name, cfg in (bn or {}).items():
        layer = m.get_submodule(name)
        layer.eps = cfg.get("eps", layer.eps)
        layer.momentum = cfg.get("momentum", layer.momentum)
    return m.train()


def buffers(m):
    sd = m.state_dict()
    return {f"{name}.{k}": sd[f"{name}.{k}"].cpu().numpy().copy() for name in oracle.BN_NAMES(m.num_residuals) for k in BUFFERS}


def restore(m, sd):
    with torch.no_grad():
        for name in oracle.BN_NAMES(m.num_residuals):
            for k in BUFFERS:
                m.get_submodule(name).get_buffer(k).copy_(torch.from_numpy(np.asarray(sd[f"{name}.{k}"])))


def check(name, got, ref64, bound=None):
    bound = oracle.bound(ref64) if bound is None else bound
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    print(f"{name}: max|delta| {err:.3e}, bound {bound:.3e} (share {err / bound:.3f}), max|ref| {np.abs(ref64).max():.4g}")
    assert got.shape == ref64.shape, name
    assert np.isfinite(got).all(), name
    assert err <= bound, (name, err, bound)
    return err / bound


def check_buffers(m, ref, names=None):
    names = oracle.BN_NAMES(m.num_residuals) if names is None else names
    got = buffers(m)
    worst = 0.0
    for name in names:
        for k in ("running_mean", "running_var"):
            err = float(np.abs(got[f"{name}.{k}"].astype(np.float64) - ref[f"{name}.{k}"]).max())
            worst = max(worst, err / oracle.bound(ref[f"{name}.{k}"]))
            assert err <= oracle.bound(ref[f"{name}.{k}"]), (name, k, err)
        assert int(got[name + ".num_batches_tracked"]) == int(ref[name + ".num_batches_tracked"]), name
    print(f"running tensors: worst share of the bound {worst:.3f}")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_buffers(a, b):
    for k, v in a.items():
        as_bits = np.int32 if v.dtype == np.float32 else v.dtype
        assert np.array_equal(v.view(as_bits), b[k].view(as_bits)), k


@pytest.mark.parametrize("rc", oracle.GPU_PARITY, ids=lambda rc: f"R{rc[0]}-{oracle.case_id(rc[1])}")
@pytest.mark.parametrize("wset", ["default", "hot"])
def test_parity_with_the_float64_oracle(wset, rc):
    """R = 8 on every case; R = 1 (no ping-pong, res = x1 everywhere), 2 and 16 (32 counters and tables) on two of them."""
    R, case = rc
    n, h, w = case
    m = train_model(synth.make_esrgan_state_dict(wset, R), R)
    ref = oracle.reference(wset, case, R)
    x = torch.from_numpy(oracle.case_input(case)).to(DEV)
    out = m(x)
    stages = {k: m.stage(k, n, h, w).cpu().numpy() for k in ("x1", "tail_in")}
    torch.cuda.synchronize()
    check_buffers(m, ref)                      # after ONE call
    assert out.shape == (n, 3, h, w) and out.dtype == torch.float32
    assert not out.requires_grad and out.grad_fn is None
    for k in ("x1", "tail_in"):
        check(k, stages[k], ref[k])
    check("out", out.cpu().numpy(), ref["out"])


@pytest.mark.parametrize("wset,case", [("default", (2, 1, 1)), ("default", (1, 1, 2)), ("hot", (1, 2, 2))],
                         ids=["2x1x1", "1x1x2", "hot-1x2x2"])
def test_ill_conditioned_batches(wset, case):
    """Not parity cases: with two values per channel the batch variance of later layers is far below eps and ATen fp32 itself is
    thousands of bounds from float64; 1x2x2 on "hot" is at 1.5.  The first BatchNorm still sees well-scaled data: its running
    buffers meet the rule; the output is finite and two calls give the same bits."""
    n, h, w = case
    sd = synth.make_esrgan_state_dict(wset, 8)
    m = train_model(sd, 8)
    x = torch.from_numpy(oracle.case_input(case)).to(DEV)
    a = m(x)
    check_buffers(m, oracle.forward(sd, oracle.case_input(case), 8), names=("residuals.0.block.1",))
    b = m(x)
    assert a.shape == (n, 3, h, w) and bool(torch.isfinite(a).all())
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("bn", [{"residuals.2.block.1": {"momentum": None}}, {"residuals.1.block.4": {"eps": 1e-3, "momentum": 0.4}}],
                         ids=["momentum-none", "eps-momentum"])
def test_two_consecutive_calls_match_the_oracle_iterated_twice(bn):
    """The running buffers are read, modified and written in place, the counter ends two higher; one layer with momentum=None (the
    cumulative average 1 / num_batches_tracked, which differs between the calls) or with its own eps and momentum."""
    case, R = (3, 8, 12), 3
    n, h, w = case
    sd = synth.make_esrgan_state_dict("hot", R)
    x = oracle.case_input(case)
    first = oracle.forward(sd, x, R, bn=bn)
    second = oracle.forward(oracle.next_state_dict(sd, first, R), x, R, bn=bn)
    m = train_model(sd, R, bn)
    xd = torch.from_numpy(x).to(DEV)
    m(xd)
    check_buffers(m, first)
    out = m(xd)
    check_buffers(m, second)
    check("tail_in", m.stage("tail_in", n, h, w).cpu().numpy(), second["tail_in"])
    check("out", out.cpu().numpy(), second["out"])
    for name in oracle.BN_NAMES(R):
        assert int(m.state_dict()[name + ".num_batches_tracked"]) == int(sd[name + ".num_batches_tracked"]) + 2
    # the changed layer's settings reach the result: the defaults give other buffers there
    (name, _), = bn.items()
    plain = oracle.forward(sd, x, R)
    for key in (f"{name}.running_mean", f"{name}.running_var"):
        assert np.abs(plain[key] - first[key]).max() > 100 * oracle.bound(first[key]), key


def test_the_skip_is_live():
    """R = 2 on 2 x 3 tiles: block 0's output is formed and stored by the staging of block 1's first convolution, block 1's by the sum
    launch.  Without the skips the tail's input is more than 100 bounds away."""
    case, R = (1, 20, 36), 2
    sd = synth.make_esrgan_state_dict("default", R)
    x = oracle.case_input(case)
    ref = oracle.reference("default", case, R)
    plain = oracle.forward(sd, x, R, skip=False)
    m = train_model(sd, R)
    m(torch.from_numpy(x).to(DEV))
    got = m.stage("tail_in", *case).cpu().numpy()
    moved = float(np.abs(got - plain["tail_in"]).max())
    print(f"without the skips tail_in is {moved:.3e} away; bound {oracle.bound(ref['tail_in']):.3e}")
    assert moved > 100 * oracle.bound(ref["tail_in"])
    check("tail_in", got, ref["tail_in"])


def test_uint8_paths_and_repeatability():
    """uint8 input gives the bits of its /255 fp32 copy; the uint8 output is the server's view of the fp32 output; the same call twice
    from restored buffers gives identical bits of output and buffers."""
    case, R = (3, 8, 12), 3
    sd = synth.make_esrgan_state_dict("hot", R)
    m = train_model(sd, R)
    u8_host = synth.esrgan_inputs_u8(*case, 2700)
    u8 = torch.from_numpy(u8_host).to(DEV)
    xf = torch.from_numpy(np.ascontiguousarray(u8_host.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0)).to(DEV)
    out = m(xf)
    after = buffers(m)
    restore(m, sd)
    again = m(xf)
    assert torch.equal(_bits(out), _bits(again))
    _same_buffers(buffers(m), after)
    assert torch.equal(_bits(m(u8, out_dtype=torch.float32)), _bits(out))
    view = out.clamp(0, 1).mul(255).byte().permute(0, 2, 3, 1).contiguous()
    got = m(xf, out_dtype=torch.uint8)
    assert got.dtype == torch.uint8 and torch.equal(got, view) and torch.equal(m(u8), view)
    assert np.array_equal(view.cpu().numpy(), esrgan_oracle.to_u8(out.cpu().numpy()))
    sat = float(((view == 0) | (view == 255)).float().mean())
    print("bytes at 0 or 255:", sat)
    assert 0 < sat < 1                                     # the clamp is exercised and is not all there is


def test_the_prelu_on_the_staging_path_is_live():
    """"hot" sets the slope of the last block's PReLU to 1.5 (a max-form PReLU is wrong above 1).  In train mode that PReLU runs while
    the block's second convolution stages its input: with the slope swapped for 0.25 tail_in moves by more than 100 times the bound."""
    case, R = (3, 8, 12), 2
    n, h, w = case
    sd = synth.make_esrgan_state_dict("hot", R)
    key = f"residuals.{R - 1}.block.2.weight"
    assert float(sd[key][0]) == pytest.approx(1.5)
    other = dict(sd)
    other[key] = np.full(1, 0.25, np.float32)
    x = torch.from_numpy(oracle.case_input(case)).to(DEV)
    tails = []
    for weights in (sd, other):
        m = train_model(weights, R)
        m(x)
        tails.append(m.stage("tail_in", n, h, w).cpu().numpy())
    ref = oracle.reference("hot", case, R)
    check("tail_in", tails[0], ref["tail_in"])
    moved = float(np.abs(tails[0] - tails[1]).max())
    print(f"slope 1.5 -> 0.25 moves tail_in by {moved:.3e}; bound {oracle.bound(ref['tail_in']):.3e}")
    assert moved > 100 * oracle.bound(ref["tail_in"])
    check("tail_in, slope 0.25", tails[1], oracle.forward(other, oracle.case_input(case), R)["tail_in"])


def test_eval_after_training_folds_the_updated_running_statistics():
    """A kernel writing through a raw pointer bumps no version counter: after two train calls .eval() must still give the bits of a
    module freshly loaded from the trained state_dict, not those of the fold made before training."""
    case, R = (3, 8, 12), 3
    sd = synth.make_esrgan_state_dict("hot", R)
    x = torch.from_numpy(oracle.case_input(case)).to(DEV)
    m = train_model(sd, R)
    m.eval()
    before = m(x)                                          # folds the initial statistics
    m.train()
    m(x)
    m(x)
    m.eval()
    got = m(x)
    fresh = load_esrgan(m.state_dict(), num_residuals=R, device=DEV, strict=True)
    assert not fresh.training
    assert torch.equal(_bits(got), _bits(fresh(x)))
    assert not torch.equal(_bits(got), _bits(before))      # the statistics moved, and the result with them
    assert torch.equal(_bits(m.stage("tail_in", *case)), _bits(fresh.stage("tail_in", *case)))   # the eval layout again


def test_eval_mode_of_a_batch_stats_module_is_the_default_modules():
    case, R = (1, 13, 18), 8
    sd = synth.make_esrgan_state_dict("hot", R)
    x = torch.from_numpy(oracle.case_input(case)).to(DEV)
    a = load_esrgan(sd, num_residuals=R, device=DEV, strict=True, batch_stats=True)
    b = load_esrgan(sd, num_residuals=R, device=DEV, strict=True)
    assert not a.training
    assert torch.equal(_bits(a(x)), _bits(b(x)))
    assert torch.equal(a(x, out_dtype=torch.uint8), b(x, out_dtype=torch.uint8))
    b.train()
    with pytest.raises(RuntimeError, match="train mode"):
        b(x)


def test_no_block_train_mode_is_eval_mode():
    """R = 0 has no BatchNorm: the train call runs the eval launches, one value per channel included."""
    sd = synth.make_esrgan_state_dict("hot", 0)
    m = load_esrgan(sd, num_residuals=0, device=DEV, strict=True, batch_stats=True)
    for case in ((2, 17, 33), (1, 1, 1)):
        x = torch.rand(case[0], 3, case[1], case[2], device=DEV)
        want, want_tail = m(x), m.stage("tail_in", *case)
        m.train()
        got = m(x)
        assert torch.equal(_bits(got), _bits(want))
        assert torch.equal(_bits(m.stage("tail_in", *case)), _bits(want_tail))
        assert torch.equal(m(x, out_dtype=torch.uint8), m.eval()(x, out_dtype=torch.uint8))


def test_shapes_and_arguments_that_raise():
    m = train_model(synth.make_esrgan_state_dict("default", 2), 2)
    before = buffers(m)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m(torch.zeros(1, 3, 1, 1, device=DEV))
    with pytest.raises(RuntimeError, match="out_dtype"):
        m(torch.zeros(1, 3, 8, 8, device=DEV), out_dtype=torch.float16)
    with pytest.raises(RuntimeError, match="expected a float32 input"):
        m(torch.zeros(1, 4, 8, 8, device=DEV))
    torch.cuda.synchronize()
    _same_buffers(buffers(m), before)                      # a refused call updates nothing
    assert tuple(m(torch.zeros(2, 3, 1, 1, device=DEV)).shape) == (2, 3, 1, 1)
    assert int(m.state_dict()["residuals.1.block.4.num_batches_tracked"]) == int(before["residuals.1.block.4.num_batches_tracked"]) + 1


GUARD = 4096


def _guarded(nbytes, fill):
    buf = torch.full((nbytes + 2 * GUARD + 256,), fill, dtype=torch.uint8, device=DEV)
    start = (-buf.data_ptr() - GUARD) % 256 + GUARD      # 256-byte aligned, at least one guard past the start
    return buf, start


@pytest.mark.parametrize("out_u8", [False, True], ids=["f32", "u8"])
def test_nan_prefill_changes_nothing_and_guard_regions_stay_untouched(out_u8):
    """The interior-only, write-once store of the block outputs, at one-pixel remnants on both axes and R = 3 (both r tensors in use).
    Workspace and output start as NaN bits (0xFF bytes), with 4 KiB guard regions of 0xA5 before and after each: the result is finite
    and equal to the module's, and no guard byte changes (no read of an unwritten word reaches a result or a statistic, no write
    leaves its buffer)."""
    case, R = (2, 17, 33), 3
    n, h, w = case
    sd = synth.make_esrgan_state_dict("hot", R)
    m = train_model(sd, R)
    x = torch.from_numpy(oracle.case_input(case)).to(DEV)
    want = m(x, out_dtype=torch.uint8 if out_u8 else torch.float32)
    want_buffers = buffers(m)
    restore(m, sd)
    L = _lib.lib()
    need = ctypes.c_size_t()
    assert L.cid_esr_train_workspace_bytes(n, h, w, R, ctypes.byref(need)) == 0
    out_bytes = n * h * w * 3 * (1 if out_u8 else 4)
    bufs = []
    for nbytes in (need.value, out_bytes):
        buf, start = _guarded(nbytes, 0xA5)
        buf[start:start + nbytes] = 0xFF
        bufs.append((buf, start, nbytes))
    (wsb, ws0, _), (ob, o0, _) = bufs
    bn = named_bn_args([(name, m.get_submodule(name)) for name in oracle.BN_NAMES(R)], torch.device(DEV))
    stream = torch.cuda.current_stream().cuda_stream
    rc = L.cid_esr_forward_train(m._cid, x.data_ptr(), _lib.CID_FMT_F32_NCHW, ob.data_ptr() + o0,
                                 _lib.CID_FMT_U8_NHWC if out_u8 else _lib.CID_FMT_F32_NCHW, n, h, w, bn, wsb.data_ptr() + ws0,
                                 need.value, stream)
    assert rc == 0, L.cid_esr_last_error(m._cid)
    torch.cuda.synchronize()
    got = ob[o0:o0 + out_bytes].clone()
    got = got.view(n, h, w, 3) if out_u8 else got.view(torch.float32).view(n, 3, h, w)
    if not out_u8:
        assert torch.isfinite(got).all()
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    for k, v in buffers(m).items():
        assert np.isfinite(v).all() and np.array_equal(v, want_buffers[k]), k
    for buf, start, nbytes in bufs:
        assert bool((buf[:start] == 0xA5).all()) and bool((buf[start + nbytes:] == 0xA5).all())
