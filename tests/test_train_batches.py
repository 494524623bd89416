"""Train-mode BatchNorm on the two axes where a batch-coupled kernel has failure modes of its own: more than 65,535 images, and
tensors past 2^31 elements.  Entry points: cid_esr_forward_train, cid_sr_forward_train, cid_sr_forward_saved + cid_sr_backward,
cid_srd_forward(training = 1) and cid_srd_forward_saved + cid_srd_backward(training = 1) (include/cid.h).  The batches, the cases'
arithmetic and every condition on the references are tests/test_train_batches_host.py's, which proves them without a GPU; every bound
here is the family's own (tests/test_esrgan_train.py, test_srgan_train.py, test_srgan_backward.py, test_srgan_disc.py,
test_srgan_disc_backward.py).  Every call goes through the C ABI on buffers prefilled with 0xFF bytes (NaN bits) between 4 KiB guard
regions of 0xA5: workspace, saved buffer, outputs, gradients.

Part A: the launch split.  N = 2 * 65,535 + 9 = 131,079 distinct 1 x 1 images, so every grid runs as two full launches and one of
nine images, and the three launches draw from three value ranges: statistics that lose a launch, count one twice or divide by one
launch's image count move `out` by 24,000 bounds or more (the host file).  A slab row written at blockIdx.y without the launch's
first image leaves the later launches' rows at the NaN prefill, and the statistics with them.  The whole batch runs through the float64
oracle: x1 / x0, trunk, tail_in, the output, the running buffers and counters; the uint8 batch gives the bits of its fp32 view;
cid_sr_forward_saved gives cid_sr_forward_train's bits, and cid_sr_backward's parameter gradients under a dense grad_out meet
e_hip <= max(1e-5, 2 * e_aten) with e_aten measured on this batch.  (At 1 x 1 every pixel sees the same padding, so the gradient of
res_blocks.0-3.4.bias, a per-channel shift in front of a convolution and a train-mode BatchNorm, is exactly 0 like that of the
convolution biases: float64 gives 1e-19, ATen fp32 and the device rounding noise, and the rule's 2 * e_aten branch decides.)

Part B: past 2^31 elements, on periodic batches.  Image n is image n mod 7 of a block made on the device by
periodic_block_u8 (7 is odd, coprime to 65,535, and 65,535 mod 7 = 1: an index off by a launch or a power of two lands in another
residue class).  Such a batch has the block's mean and biased variance exactly, so for each case
  (a) train_crossing() (host file) says which tensors pass 2^30, 2^31 and 2^32 elements and in which periods;
  (b) all buffers are prefilled and guarded as above;
  (c) every tensor the call leaves behind (stage views, the raw z tensors, the block output r.0, saved tensors, masks) and the
      output / input gradient, reshaped to (q, 7, ...), is bit-equal across q, compared on the device;
  (d) the first period, the last, and every period that holds element 2^30, 2^31 or 2^32 of a tensor are held to the float64 oracle
      of the 7-image block under the family's bound;
  (e) running mean, running variance and counter are held to that oracle under the family's rule, the running variance with the
      unbiased factor M / (M - 1) at the big batch's M = N * H * W, derived from the oracle's biased variance.  The block's own
      running_var is 3.57 bounds from that reference on the sr case and 0.87 on the esr case (the host file asserts both): on sr
      (e) tells the big batch's M from the block's, on esr it holds the statistics but could not tell the two counts apart.
Cases: esr N = 8750 = 7 * 1250 of 48 x 80 at R = 2 (x1, z0, z1, r.0 and tail_in hold 2,150,400,000 elements each; launch 2 forms r.0
from x1 and BN(z1) while it stages, and the sum launch reads z3, r.0 and x1; 40.6 GiB); sr N = 17500 = 7 * 2500 of 24 x 40 (1.5 x
2.5 tiles) at scale 2: the stage output holds 4,300,800,000 elements (past 2^32), x0, z0, z1 and trunk 1,075,200,000 each (past
2^30, 2^32 bytes), 33.7 GiB; srd N = 35000 = 7 * 5000 of 24 x 40 (a0 past 2^31, z5 past 2^30; 33.3 GiB), forward and backward: with
a periodic grad_prob the input gradient is periodic and every parameter gradient is q times the block's, held to
max(1e-5, 2 * e_aten) with e_aten measured on the block.
Out of scope: cid_sr_forward_saved + cid_sr_backward past 2^31 elements (its saved buffer gives each of the ten z a tensor of its
own: 12 + 4 base tensors next to the forward's workspace do not fit under the 70 GiB cap at a size where one passes 2^31; Part A
and the kernels shared with cid_sr_forward_train cover what can be covered), and cid_esd_*, whose train mode is its eval mode.

What fails here, each tried once on a scratch build and not kept: the slab row of the train tile taken from
blockIdx.y without n0 (Part A's three tests: NaN statistics; Part B and the family files stay green); the statistics launch of
esr_train_run given one launch's image count, min(N, 65535) (Part A's esr test: tail_in 3.2e8 away; Part B's esr case is one launch,
whose count is N, and stays green); the image term of the r_out offset in the ST_IN_RES_BN staging masked to 31 bits, which wraps
inside the buffer (Part B's esr case: the twelve images from 8738 on, the one that holds element 2^31, land on periods 0 and 1 of
r.0 and leave periods 1248 and 1249 at the NaN prefill, so (c) reports periods 1, 2, 1248 and 1249 of r.0 and of tail_in, and (d)
period 0 at 124,000 bounds on r.0 and 81,000 on out and periods 1248 and 1249 as not finite, while period 624 and x1 pass;
Part A's esr test, tests/test_esrgan_train.py, tests/test_wide_offsets.py, tests/test_operand_edges_esrgan_train.py and
test_large_batches.py::test_esrgan_forward stay green).

A finding of this file: k_disc_wgrad accumulated a workgroup's whole range of items in one fp32 chain, whose length grows with N
(1640 items at 35,000 images): model.2 / 5 / 8 / 11.weight of the srd backward stood at 2.1 - 2.4 bounds.  It now folds every 64 items
(csrc/disc_bwd_kernels.h, D_WG_CHUNK), and they stand at 0.19 - 0.21.

Measured on one MI355X, whole suite in one process: worst share of the bound (e_hip / bound), device time of a call, time of the test.
  A esr          x1 0.004, tail_in 0.130, out 0.179, running tensors 0.005                            0.154 s   2.8 s
  A sr           x0 0.004, trunk 0.093, tail_in 0.088, pre 0.099, out 0.103, running tensors 0.005    0.328 s   7.6 s
  A sr backward  0.657 of max(1e-5, 2 e_aten), 33 mask flips inside the cap                           0.79 s    53 s
  B esr          x1 0.087, r.0 0.078, tail_in 0.074, out 0.081, running tensors 0.004                 0.154 s   under 1.8 s
  B sr           x0 0.081, trunk 0.081, tail_in 0.112, pre 0.102, out 0.412, running tensors 0.004    0.316 s   under 1.8 s
  B srd forward  p 0.015                                                                              0.076 s   under 1.8 s
  B srd backward 0.265 of max(1e-5, 2 e_aten) (model.9.weight), p 0.015                               0.081 + 0.263 s   under 1.8 s
The sr backward of Part A is not quick: about 50 of its 53 s are the reference's three autograd runs over 131,079 images on the CPU
(float64 with the device's masks, fp32, float64 with ATen's masks), which the rule's "e_aten on the same batch" asks for; the device
calls come first, so a broken build fails within seconds."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib
from celebrity_image_denoiser_amd.discriminator import named_bn_args

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import esrgan_train_oracle  # noqa: E402
import srgan_backward_ref  # noqa: E402
import srgan_train_oracle  # noqa: E402
import test_esrgan_train as TET  # noqa: E402
import test_srgan_backward as TSB  # noqa: E402
import test_srgan_disc as TSD  # noqa: E402
import test_srgan_disc_backward as TSDB  # noqa: E402
import test_srgan_train as TST  # noqa: E402
import test_train_batches_host as H  # noqa: E402
import test_wide_offsets as TWO  # noqa: E402

DEV = "cuda:0"
F32, U8 = _lib.CID_FMT_F32_NCHW, _lib.CID_FMT_U8_NHWC
GUARD = 4096
K = H.K


# ----------------------------------------------------------------------------------------------------------------------- buffers
class _Buf:
    """`nbytes` of 0xFF on a 256-byte boundary between two guard regions of 0xA5."""

    def __init__(self, nbytes):
        self.n = max(int(nbytes), 4)
        self.raw = torch.full((self.n + 2 * GUARD + 256,), 0xA5, dtype=torch.uint8, device=DEV)
        self.start = (-self.raw.data_ptr() - GUARD) % 256 + GUARD
        self.t = self.raw[self.start:self.start + self.n]
        self.t.fill_(0xFF)
        self.ptr = self.t.data_ptr()
        assert self.ptr % 256 == 0

    def f32(self, *shape):
        return self.t.view(torch.float32).view(*shape)

    def intact(self):
        return bool((self.raw[:self.start] == 0xA5).all()) and bool((self.raw[self.start + self.n:] == 0xA5).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dims(x):
    return (U8, x.shape[0], x.shape[1], x.shape[2]) if x.dtype == torch.uint8 else (F32, x.shape[0], x.shape[2], x.shape[3])


def _bits(t):
    return t.reshape(-1).view(torch.int32)


def _images(buf, view, lo, hi):
    """Images [lo, hi) of a C8 tensor at `view` = (name, offset, C, Hs, Ws) of a buffer -> fp32 [hi-lo,C,Hs,Ws] on the host."""
    _, off, ch, hs, ws = view
    per = 4 * ch * hs * ws
    t = buf[off + per * lo:off + per * hi].view(torch.float32).view(hi - lo, ch // 8, hs, ws, 8)
    return t.permute(0, 1, 4, 2, 3).reshape(hi - lo, ch, hs, ws).cpu().numpy()


def _periodic(name, t, q, found=None):
    """(c): `t`, a tensor whose leading axis runs over q periods, has the same bits in every period.  With `found`, a list, a
    difference is recorded there and the test goes on to its next check."""
    v = t.reshape(-1)
    v = (v.view(torch.int32) if v.dtype == torch.float32 or (v.dtype == torch.uint8 and v.numel() % (4 * q) == 0) else v).view(q, -1)
    differs = (v[1:] != v[:-1]).any(dim=1).nonzero().view(-1) + 1
    what = ("(c)", name, f"{differs.numel()} periods differ from the one before them, the first four:", differs[:4].tolist())
    if found is None:
        assert differs.numel() == 0, what
    elif differs.numel():
        found.append(what)


def _tensor_bytes(buf, view, n):
    _, off, ch, hs, ws = view
    return buf[off:off + 4 * n * ch * hs * ws]


def _share(name, got, ref64, bound, shares, found=None, period=None):
    """(d): one tensor against the float64 oracle under its bound.  With `found`, a miss is recorded there with its period."""
    try:
        shares[name] = max(shares.get(name, 0.0), TWO._share(name, got, ref64, bound))
    except AssertionError as e:
        if found is None:
            raise
        found.append(("(d)", f"period {period}", str(e)[:120]))


def _buffer_shares(got, ref, names, bound):
    """Worst |running - ref| / bound over the running tensors of `names` (the assertion is the family's check_buffers)."""
    return max(float(np.abs(got[f"{b}.{k}"].astype(np.float64) - ref[f"{b}.{k}"]).max()) / bound(ref[f"{b}.{k}"])
               for b in names for k in ("running_mean", "running_var"))


def _case(family):
    c = H.train_crossing(family)
    TWO._skip_below(c["need"])
    print(f"\n{family}: N = {c['n']} = {K} * {c['q']}, past 2^31 elements: " + ", ".join(f"{k} = {c['n'] * c['per'][k]}" for k in c["past"][1 << 31])
          + f"; periods held to the oracle {c['blocks']}; {c['need'] / TWO.GIB:.1f} GiB")
    return c


def _periodic_batch(family):
    """The case's block made on the device (the host's bytes, asserted) and its q-fold repetition, uint8 [N,h,w,3]."""
    cfg, blk = H.TRAIN_CASES[family], H.block_case(family)
    block = H.periodic_block_u8(K, cfg["h"], cfg["w"], cfg["seed"], DEV)
    assert np.array_equal(block.cpu().numpy(), blk["u8"])
    return blk, block.repeat(blk["q"], 1, 1, 1)


# --------------------------------------------------------------------------------------------------------- cid_esr_forward_train
def _esr_train(m, x):
    """cid_esr_forward_train on module m's handle and BatchNorm tensors -> (out fp32 [N,3,H,W], the workspace's bytes, seconds)."""
    L = _lib.lib()
    fmt, n, h, w = _dims(x)
    r = m.num_residuals
    m.pack_weights()
    need = TWO._size(L.cid_esr_train_workspace_bytes, n, h, w, r)
    ws, out = _Buf(need), _Buf(4 * n * 3 * h * w)
    bn = named_bn_args([(name, m.get_submodule(name)) for name in esrgan_train_oracle.BN_NAMES(r)], torch.device(DEV))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _lib.check_abi("esr", m._cid, L.cid_esr_forward_train(m._cid, x.data_ptr(), fmt, out.ptr, F32, n, h, w, bn, ws.ptr, need, _stream()))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert ws.intact() and out.intact(), "a guard region changed"
    return out.f32(n, 3, h, w), ws.t, dt


@pytest.mark.gpu
def test_esr_forward_train_across_the_launch_split():
    a = H.part_a("esr")
    ref, sd, r = a["ref"], a["sd"], H.R_A
    n = H.N_A
    m = TET.train_model(sd, r)
    x = torch.from_numpy(a["x"]).to(DEV)
    out, ws, dt = _esr_train(m, x)
    views = {s: (s,) + TWO._view(_lib.lib().cid_esr_train_stage_view, s, n, 1, 1, r) for s in ("x1", "tail_in")}
    got = {s: _images(ws, v, 0, n) for s, v in views.items()}
    got["out"] = out.cpu().numpy()
    running = TET.buffers(m)
    for k, v in {**got, **running}.items():
        assert np.isfinite(v).all(), f"{k} is not finite: a slab row or an image the launches after the first did not write"
    shares = {}
    for k in ("x1", "tail_in", "out"):
        _share(k, got[k], ref[k], esrgan_train_oracle.bound(ref[k]), shares)
    TET.check_buffers(m, ref)
    shares["running"] = _buffer_shares(running, ref, esrgan_train_oracle.BN_NAMES(r), esrgan_train_oracle.bound)
    # the uint8 batch gives the bits of its /255 view, from the same starting buffers
    TET.restore(m, sd)
    out8, _, _ = _esr_train(m, torch.from_numpy(a["u8"]).to(DEV))
    assert torch.equal(_bits(out8), _bits(out))
    TET._same_buffers(TET.buffers(m), running)
    print(f"esr train {n}x1x1: {dt:.3f} s a call; worst shares of the bounds " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))


@pytest.mark.gpu
@TWO._frees_its_buffers
def test_esr_forward_train_past_2_31_elements():
    c = _case("esr")
    cfg = H.TRAIN_CASES["esr"]
    blk, u8 = _periodic_batch("esr")
    n, q, ref = c["n"], c["q"], blk["ref"]
    m = TET.train_model(blk["sd"], cfg["r"])
    out, ws, dt = _esr_train(m, u8)
    found = []                                                                     # (c) and (d) both run before either fails the test
    for v in c["views"]:                                                           # (c)
        _periodic(v[0], _tensor_bytes(ws, v, n).view(torch.float32), q, found)
    _periodic("out", out, q, found)
    shares = {}
    for b in c["blocks"]:                                                          # (d)
        for v in c["views"]:
            if v[0] in ref:
                _share(v[0], _images(ws, v, b * K, (b + 1) * K), ref[v[0]], esrgan_train_oracle.bound(ref[v[0]]), shares, found, b)
        _share("out", out[b * K:(b + 1) * K].cpu().numpy(), ref["out"], esrgan_train_oracle.bound(ref["out"]), shares, found, b)
    print(*found, sep="\n")
    assert not found, found
    TET.check_buffers(m, ref)                                                      # (e)
    shares["running"] = _buffer_shares(TET.buffers(m), ref, esrgan_train_oracle.BN_NAMES(cfg["r"]), esrgan_train_oracle.bound)
    print(f"esr train {n}x{cfg['h']}x{cfg['w']}: {dt:.3f} s a call; worst shares of the bounds "
          + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))


# ---------------------------------------------------------------------------------------------------------- cid_sr_forward_train
def _sr_train(m, x, raw=False):
    """cid_sr_forward_train on module m's handle and BatchNorm tensors -> (out fp32 [N,3,sH,sW], the workspace's bytes, seconds)."""
    L = _lib.lib()
    fmt, n, h, w = _dims(x)
    s = m.scale_factor
    m.pack_weights()
    need = TWO._size(L.cid_sr_train_workspace_bytes, n, h, w, s)
    ws, out = _Buf(need), _Buf(4 * n * 3 * s * h * s * w)
    bn = named_bn_args([(name, m.get_submodule(name)) for name in srgan_train_oracle.BN_NAMES], torch.device(DEV))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _lib.check_abi("sr", m._cid, L.cid_sr_forward_train(m._cid, x.data_ptr(), fmt, out.ptr, F32, n, h, w, _lib.CID_SR_RAW if raw else 0, bn,
                                                        ws.ptr, need, _stream()))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert ws.intact() and out.intact(), "a guard region changed"
    return out.f32(n, 3, s * h, s * w), ws.t, dt


def _sr_same_buffers(a, b):
    for k, v in a.items():
        as_bits = np.int32 if v.dtype == np.float32 else v.dtype
        assert np.array_equal(v.view(as_bits), b[k].view(as_bits)), k


@pytest.mark.gpu
def test_sr_forward_train_across_the_launch_split():
    """The sums before tanh (CID_SR_RAW) and the stages from one call, `out` from a second one that starts from the same buffers:
    tests/test_srgan_train.py's rule, `out` under max(1e-5, 2 * e_aten) with e_aten measured on this batch."""
    a = H.part_a("sr")
    ref, sd, s = a["ref"], a["sd"], H.SCALE_A
    n = H.N_A
    m = TST.train_model(sd, s)
    x = torch.from_numpy(a["x"]).to(DEV)
    pre, ws, dt = _sr_train(m, x, raw=True)
    views = {k: (k,) + TWO._view(_lib.lib().cid_sr_train_stage_view, k, n, 1, 1, s) for k in ("x0", "trunk", "tail_in")}
    got = {k: _images(ws, v, 0, n) for k, v in views.items()}
    got["pre"] = pre.cpu().numpy()
    running = TST.buffers(m)
    for k, v in {**got, **running}.items():
        assert np.isfinite(v).all(), f"{k} is not finite: a slab row or an image the launches after the first did not write"
    shares = {}
    for k in ("x0", "trunk", "tail_in", "pre"):
        _share(k, got[k], ref[k], srgan_train_oracle.bound(ref[k]), shares)
    TST.check_buffers(m, ref)
    shares["running"] = _buffer_shares(running, ref, srgan_train_oracle.BN_NAMES, srgan_train_oracle.bound)
    TST.restore(m, sd)
    out, _, _ = _sr_train(m, x)
    _share("out", out.cpu().numpy(), ref["out"], H.sr_out_bound(ref, a["r32"]), shares)
    _sr_same_buffers(TST.buffers(m), running)
    TST.restore(m, sd)
    out8, _, _ = _sr_train(m, torch.from_numpy(a["u8"]).to(DEV))                   # the uint8 batch gives its normalised view's bits
    assert torch.equal(_bits(out8), _bits(out))
    print(f"sr train {n}x1x1 s{s}: {dt:.3f} s a call; worst shares of the bounds " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))


@pytest.mark.gpu
def test_sr_backward_across_the_launch_split():
    """cid_sr_forward_saved + cid_sr_backward through test_srgan_backward.cabi (NaN-filled saved buffer and workspaces, guards)."""
    a = H.part_a("sr")
    sd, s, n = a["sd"], H.SCALE_A, H.N_A
    x = torch.from_numpy(a["x"]).to(DEV)
    plain = TSB.model_of(sd, s, autograd=False)
    want_out, _, _ = _sr_train(plain, x)
    m = TSB.model_of(sd, s)
    G = srgan_backward_ref.grad_out(n, s, 1, 1)
    t0 = time.perf_counter()
    out, grads, masks = TSB.cabi(m, x, G.to(DEV))
    t1 = time.perf_counter()
    assert bool(torch.isfinite(out).all()) and torch.equal(_bits(out), _bits(want_out))   # cid_sr_forward_train's bits
    got, want = TSB.running(m), TSB.running(plain)
    assert len(want) == 30 and all(torch.equal(TSB._bits(got[k]), TSB._bits(want[k])) for k in want)
    assert list(grads) == srgan_backward_ref.param_names(1)
    e_aten, G_ref = H.part_a_sr_backward_aten()                                    # the references come last: they take a minute
    assert torch.equal(G, G_ref)
    t2 = time.perf_counter()
    TSB.check_against_float64(sd, a["x"], G, grads, masks, e_aten)
    print(f"sr backward {n}x1x1 s{s}: forward_saved + masks + backward {t1 - t0:.2f} s; the references on the CPU {t2 - t1:.0f} s "
          f"and {time.perf_counter() - t2:.0f} s")


@pytest.mark.gpu
@TWO._frees_its_buffers
def test_sr_forward_train_past_2_31_elements():
    c = _case("sr")
    cfg = H.TRAIN_CASES["sr"]
    blk, u8 = _periodic_batch("sr")
    n, q, ref, s = c["n"], c["q"], blk["ref"], cfg["scale"]
    m = TST.train_model(blk["sd"], s)
    pre, ws, dt = _sr_train(m, u8, raw=True)
    found = []                                                                     # (c) and (d) both run before either fails the test
    for v in c["views"]:                                                           # (c)
        _periodic(v[0], _tensor_bytes(ws, v, n).view(torch.float32), q, found)
    _periodic("pre", pre, q, found)
    shares = {}
    for b in c["blocks"]:                                                          # (d)
        for v in c["views"]:
            if v[0] in ref:
                _share(v[0], _images(ws, v, b * K, (b + 1) * K), ref[v[0]], srgan_train_oracle.bound(ref[v[0]]), shares, found, b)
        _share("pre", pre[b * K:(b + 1) * K].cpu().numpy(), ref["pre"], srgan_train_oracle.bound(ref["pre"]), shares, found, b)
    print(*found, sep="\n")
    assert not found, found
    TST.check_buffers(m, ref)                                                      # (e)
    running = TST.buffers(m)
    shares["running"] = _buffer_shares(running, ref, srgan_train_oracle.BN_NAMES, srgan_train_oracle.bound)
    # the same batch through tanh, from the same buffers: periodic, inside `out`'s bound, and the same statistics bit for bit
    pre = ws = None
    torch.cuda.empty_cache()
    TST.restore(m, blk["sd"])
    out, ws, _ = _sr_train(m, u8)
    _periodic("out", out, q)
    for b in c["blocks"]:
        _share("out", out[b * K:(b + 1) * K].cpu().numpy(), ref["out"], blk["bounds"]["out"], shares)
    _sr_same_buffers(TST.buffers(m), running)
    print(f"sr train {n}x{cfg['h']}x{cfg['w']} s{s}: {dt:.3f} s a call; worst shares of the bounds "
          + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))


# ------------------------------------------------------------------------------------- cid_srd_forward, cid_srd_backward (train)
def _srd_module(family="srd"):
    m = TSD._module(H.TRAIN_CASES[family]["kind"], True)
    m.pack_weights()
    return m


@pytest.mark.gpu
@TWO._frees_its_buffers
def test_srd_forward_train_past_2_31_elements():
    """The forward's regions alias (a0, then z5, then z11 in region A), so the probabilities and the statistics carry the comparison:
    every layer feeds them."""
    c = _case("srd")
    cfg = H.TRAIN_CASES["srd"]
    blk, u8 = _periodic_batch("srd")
    n, q, h, w = c["n"], c["q"], cfg["h"], cfg["w"]
    x = blk["x"].to(DEV).repeat(q, 1, 1, 1)                                       # synth.normalize_u8 of the block, as the oracle has it
    L = _lib.lib()
    need = TWO._size(L.cid_srd_workspace_bytes, n, h, w, 1)
    results = []
    for inp in (x, u8):
        m = _srd_module()
        ws, p = _Buf(need), _Buf(4 * n)
        fmt = _dims(inp)[0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.check_srd(m._cid, L.cid_srd_forward(m._cid, inp.data_ptr(), fmt, p.ptr, n, h, w, TWO._srd_bn(m), 1, ws.ptr, need, _stream()))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert ws.intact() and p.intact(), "a guard region changed"
        p = p.f32(n)
        _periodic("p", p, q)                                                       # (c)
        share = max(TWO._share(f"p, period {b}", p[b * K:(b + 1) * K].cpu().numpy(), blk["p64"].numpy(), TSD.TOL) for b in c["blocks"])   # (d)
        TSD._check_buffers(m, blk["state"])                                        # (e)
        results.append((p, TSD._buffers(m)))
        ws = None
    assert torch.equal(_bits(results[0][0]), _bits(results[1][0]))                 # a uint8 batch and its normalised copy: the same bits
    assert all(torch.equal(a, b) for a, b in zip(results[0][1], results[1][1]))
    print(f"srd train forward {n}x{h}x{w}: {dt:.3f} s a call; worst share of the bound on p {share:.3f}")


def _srd_train_backward(m, x, q, views):
    """cid_srd_forward_saved + cid_srd_saved_masks + cid_srd_backward in train mode on the q-fold repetition x of a block, with
    grad_prob the repetition of d BCE(p, 1) / dp of the first period; check (c) on everything the calls leave behind.
    -> (p, input gradient, {key: gradient / q} in float64 on the host, the first period's masks, seconds of the two calls)"""
    L = _lib.lib()
    n, _, h, w = x.shape
    bn = TWO._srd_bn(m)
    saved, p = _Buf(TWO._size(L.cid_srd_saved_bytes, n, h, w, 1)), _Buf(4 * n)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _lib.check_srd(m._cid, L.cid_srd_forward_saved(m._cid, x.data_ptr(), F32, p.ptr, n, h, w, bn, 1, saved.ptr, saved.n, _stream()))
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    pf = p.f32(n)
    _periodic("p", pf, q)
    for v in views:
        _periodic(v[0], _tensor_bytes(saved.t, v, n).view(torch.float32), q)
    h2, w2 = H._side(h), H._side(w)
    h4, w4 = H._side(h2), H._side(w2)
    shapes = ((n, 64, h, w), (n, 64, h2, w2), (n, 128, h2, w2), (n, 128, h4, w4), (n, 256, h4, w4), (n, 512))
    masks = [torch.full(s, 7, dtype=torch.uint8, device=DEV) for s in shapes]
    assert L.cid_srd_saved_masks(saved.ptr, saved.n, n, h, w, 1, (ctypes.c_void_p * 6)(*[t.data_ptr() for t in masks]), _stream()) == 0
    for i, t in enumerate(masks):
        _periodic(f"mask {i}", t, q)
    block_masks = [t[:K].cpu() for t in masks]
    assert all(bool(((t == 0) | (t == 1)).all()) for t in block_masks)
    block_masks = [t.bool() for t in block_masks]
    masks = None
    gp = TSDB._bce_grad(pf[:K].clone(), 1.0).repeat(q).contiguous()
    params = dict(m.named_parameters())
    grads = {k: _Buf(4 * params[k].numel()) for k in TSDB.PARAMS}
    g = TSDB.Grads()
    for k, t in grads.items():
        idx, kind = int(k.split(".")[1]), k.rsplit(".", 1)[1]
        if idx in TSDB.CONV_IDX:
            (g.w if kind == "weight" else g.b)[TSDB.CONV_IDX.index(idx)] = t.ptr
        else:
            (g.gamma if kind == "weight" else g.beta)[TSDB.BN_IDX.index(idx)] = t.ptr
    gx, ws = _Buf(4 * x.numel()), _Buf(TWO._size(L.cid_srd_backward_workspace_bytes, n, h, w, 1))
    g.input = gx.ptr
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    _lib.check_srd(m._cid, L.cid_srd_backward(m._cid, x.data_ptr(), F32, gp.data_ptr(), n, h, w, bn, 1, saved.ptr, saved.n, ctypes.byref(g),
                                              ws.ptr, ws.n, _stream()))
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    assert all(b.intact() for b in (saved, p, gx, ws, *grads.values())), "a guard region changed"
    gxf = gx.f32(*x.shape)
    _periodic("input gradient", gxf, q)
    got = {k: (grads[k].f32(*params[k].shape).cpu().double() / q) for k in TSDB.PARAMS}          # q times the block's
    for k in TSDB.PARAMS:
        assert bool(torch.isfinite(got[k]).all()), k
    return pf, gxf, got, block_masks, (t1 - t0, t3 - t2)


@pytest.mark.gpu
@TWO._frees_its_buffers
def test_srd_backward_train_past_2_31_elements():
    """cid_srd_forward_saved keeps a0, z2, z5, z8 and z11 without overlap (a0 past 2^31 elements, the buffer past 2^34 bytes).  grad_prob
    repeats d BCE(p, 1) / dp of the first period: the probabilities, the five saved tensors, the six masks and the input gradient are
    periodic, and every parameter gradient is q times the block's."""
    c = _case("srd")
    cfg = H.TRAIN_CASES["srd"]
    blk = H.block_case("srd")
    n, q, h, w = c["n"], c["q"], cfg["h"], cfg["w"]
    x = blk["x"].to(DEV).repeat(q, 1, 1, 1)
    m = _srd_module()
    pf, gxf, got, block_masks, (t_fwd, t_bwd) = _srd_train_backward(m, x, q, c["views"])
    e_p = max(float((pf[b * K:(b + 1) * K].cpu().double() - blk["p64"]).abs().max()) for b in c["blocks"])
    assert e_p <= TSDB.TOL
    TSD._check_buffers(m, blk["state"])
    assert bool(torch.isfinite(gxf[:K]).all())
    g64, gx64, ys64, p64 = TSDB.ref_backward(blk["sd"], blk["x"], True, 1.0, torch.float64, block_masks)
    TSDB.check_mask_cap(block_masks, ys64, "hip")
    e_aten = blk["e_aten"]
    worst, bad = 0.0, []
    for b in c["blocks"]:
        e_hip = TSDB.rel_errors(got, gxf[b * K:(b + 1) * K].cpu(), g64, gx64, True)
        for k in TSDB.PARAMS + ["input"]:
            bound = max(TSDB.TOL, 2 * e_aten[k])
            if b == 0:
                print(f"    {k:16s} e_hip {e_hip[k]:.2e}   e_aten {e_aten[k]:.2e}   share {e_hip[k] / bound:.3f}")
            worst = max(worst, e_hip[k] / bound)
            if not e_hip[k] <= bound:
                bad.append((b, k, e_hip[k], e_aten[k]))
    print(f"srd train backward {n}x{h}x{w}: forward_saved {t_fwd:.3f} s, backward {t_bwd:.3f} s; max|p - p64| {e_p:.2e} "
          f"(share {e_p / TSDB.TOL:.3f}); worst share of max(1e-5, 2 e_aten) {worst:.3f}")
    assert not bad, bad
