"""The backward pass of the SRGAN generator without a GPU: tests/srgan_backward_ref.py (the reference the GPU tests of
cid_sr_backward measure against) held to the stock nn layers under autograd, the conditioning of the GPU parity cases under the rule
of error stated there, the host argument checks and size formulas of cid_sr_saved_bytes / cid_sr_forward_saved /
cid_sr_backward_workspace_bytes / cid_sr_backward / cid_sr_saved_masks (include/cid.h), and the module's opt-in flags."""
import ctypes
import os
import sys

import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth
from celebrity_image_denoiser_amd.discriminator import _BnArg
from celebrity_image_denoiser_amd.srgan import SRGANGenerator, _GradsArg, _set_grad, load_srgan

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import srgan_backward_ref as ref  # noqa: E402
import srgan_train_oracle as oracle  # noqa: E402

ERR_INVALID, ERR_SHAPE, ERR_KEY, ERR_STATE, ERR_WORKSPACE = 1, 2, 3, 4, 5


@pytest.mark.parametrize("raw", [False, True], ids=["tanh", "raw"])
@pytest.mark.parametrize("wset", ["default", "hot"])
def test_fp32_reference_is_the_stock_module_under_autograd(wset, raw):
    """The reference on fp32 with its own masks against loss.backward() through stock nn.Conv2d / BatchNorm2d / PReLU / PixelShuffle
    in train mode.  Both run ATen fp32 on the same operands; only PReLU's backward is written by hand here, so every tensor agrees
    to well inside the rule's 1e-5 (the slopes' sums are taken in another order)."""
    case = (3, 8, 12, 2)
    n, h, w, scale = case
    sd = synth.make_srgan_state_dict(wset, scale)
    x, G = oracle.case_input(case), ref.grad_out(n, scale, h, w)
    got, pre, out, book = ref.ref_backward(sd, x, G, torch.float32, raw=raw)
    m, _ = oracle.stock_generator(sd, scale)
    x0 = m.initial(torch.from_numpy(x))
    y = m.final(m.upscale(m.mid(m.res_blocks(x0)) + x0))
    y = y if raw else torch.tanh(y)
    (y * G).sum().backward()
    assert torch.equal(y.detach(), out)
    want = {k: p.grad for k, p in m.named_parameters()}
    assert list(want) == ref.param_names(1) == list(got)
    assert len(pre) == 1 + 5 + 1 and set(book) == set(ref.slope_names(1))
    errs = ref.rel_errors(got, {k: v.double() for k, v in want.items()}, book)
    worst = max(errs, key=errs.get)
    print(f"{wset} raw={raw}: worst {worst} at {errs[worst]:.2e}")
    assert errs[worst] <= 1e-6, (worst, errs[worst])


@pytest.mark.parametrize("case", ref.CASES, ids=oracle.case_id)
@pytest.mark.parametrize("wset", ["default", "hot"])
def test_parity_inputs_are_well_conditioned(wset, case):
    """ATen fp32 itself is within the mask cap (asserted inside aten_errors) and within the plain 1e-5 on every tensor of every
    GPU parity case, under the rule of error of srgan_backward_ref."""
    errs, flips = ref.aten_errors(wset, case)
    worst = max(errs, key=errs.get)
    print(f"{wset} {oracle.case_id(case)}: ATen fp32 {flips} mask flips, worst {worst} at {errs[worst]:.2e}")
    assert errs[worst] <= ref.TOL, (worst, errs[worst])


def test_the_split_case_exceeds_every_cap_of_the_weight_gradients():
    """srgan_backward_ref.SPLIT_CASE against the caps in csrc/api/srgan_backward.h (kSrWgSplits, kSrWgUpSplits, kSrTwSplits,
    kSrW9Splits) and the kernels' item geometry: more items than workgroups in all four launches, an uneven partition, and in each
    launch a workgroup whose range [items*k/splits, items*(k+1)/splits) holds items of two images.  No other case has more items than
    a cap."""
    def launches(n, h, w, s):
        tiles = lambda hh, ww: -(-hh // 4) * -(-ww // 16)   # noqa: E731
        out = [(n * tiles(h, w), tiles(h, w), 128), (n * h * -(-w // 32), h * -(-w // 32), 256), (n * tiles(s * h, s * w), tiles(s * h, s * w), 512)]
        return out + [(n * tiles(h << k, w << k), tiles(h << k, w << k), 32) for k in range(s.bit_length() - 1)]

    for case in oracle.PARITY_CASES:
        assert all(items <= cap for items, _, cap in launches(*case)), case
    got = launches(*ref.SPLIT_CASE)
    assert len(got) == 4
    for items, per_image, cap in got:
        assert items > cap and items % cap
        ranges = [(items * k // cap, items * (k + 1) // cap) for k in range(cap)]
        assert any(b - a >= 2 and a // per_image != (b - 1) // per_image for a, b in ranges), (items, per_image, cap)


def test_masked_prelu_takes_the_given_mask():
    """A mask that differs from v > 0 changes both gradients of that PReLU and nothing of the forward."""
    v = torch.tensor([[-1.0, 2.0, 0.5]], dtype=torch.float64, requires_grad=True)
    a = torch.tensor([0.25], dtype=torch.float64, requires_grad=True)
    book = {}
    y = ref._MaskedPReLU.apply(v, a, torch.tensor([[False, True, False]]), book, "s")
    assert torch.equal(y.detach(), torch.tensor([[-0.25, 2.0, 0.5]], dtype=torch.float64))
    (y * torch.tensor([[1.0, 10.0, 100.0]], dtype=torch.float64)).sum().backward()
    assert torch.equal(v.grad, torch.tensor([[0.25, 10.0, 25.0]], dtype=torch.float64))
    assert float(a.grad) == -1.0 + 50.0 and book["s"] == 51.0


def test_opt_in_flags():
    with pytest.raises(ValueError, match="autograd=True\\) needs batch_stats=True"):
        SRGANGenerator(2, autograd=True)
    with pytest.raises(ValueError, match="needs batch_stats=True"):
        SRGANGenerator(2, False, True)
    assert "autograd" in load_srgan.__code__.co_varnames
    m = SRGANGenerator(4, batch_stats=True, autograd=True)
    assert list(m.state_dict()) == list(SRGANGenerator(4).state_dict())
    assert [k for k, _ in m.named_parameters()] == ref.param_names(2)
    m.train()
    with pytest.raises(RuntimeError, match="GPU-only"):
        m(torch.zeros(1, 3, 4, 4))


def test_every_parameter_has_its_slot_in_cid_sr_grads():
    names = ref.param_names(3)
    g = _GradsArg()
    for i, k in enumerate(names):
        _set_grad(g, k, 4 * (i + 1))
    flat = (ctypes.c_void_p * (ctypes.sizeof(g) // ctypes.sizeof(ctypes.c_void_p))).from_buffer(g)
    assert sorted(flat) == [4 * (i + 1) for i in range(len(names))] and len(flat) == 3 + 4 * 10 + 5 + 2 + 3 * 3 + 2
    assert g.head_w == 4 and g.head_slope == 12 and g.conv_w[0] == 16 and g.gamma[0] == 24 and g.slope[0] == 32 and g.conv_w[1] == 36
    assert g.beta[9] == 4 * (names.index("res_blocks.4.4.bias") + 1) and g.up_slope[2] == 4 * (names.index("upscale.8.weight") + 1)
    assert g.final_b == 4 * len(names) and g.mid_w == 4 * (names.index("mid.weight") + 1)


def _handle(L, scale):
    h = ctypes.c_void_p()
    assert L.cid_sr_create(ctypes.byref(h), scale) == 0
    return h


def test_size_formulas_are_exact_and_monotone():
    L = _lib.lib()
    n = ctypes.c_size_t()
    a256 = lambda v: (v + 255) // 256 * 256   # noqa: E731

    def saved(N, H, W, s):
        assert L.cid_sr_saved_bytes(N, H, W, s, ctypes.byref(n)) == 0
        return n.value

    def work(N, H, W, s):
        assert L.cid_sr_backward_workspace_bytes(N, H, W, s, ctypes.byref(n)) == 0
        return n.value

    for (N, H, W, s) in oracle.PARITY_CASES + [(16, 64, 64, 4), (2, 3, 5, 8)]:
        t = N * 64 * H * W * 4
        stages = s.bit_length() - 1
        want = 12 * a256(t) + sum(a256(t * 4 ** k) for k in range(1, stages + 1)) + a256(10 * 128 * 4) + a256(10 * 128 * 8) + a256(N * 3 * s * s * H * W * 4)
        assert saved(N, H, W, s) == want, (N, H, W, s)
        strips = (s * s * H * W + 511) // 512
        want = (a256(t * 4 ** stages) + (a256(t * 4 ** (stages - 1)) if stages else 0) + 2 * a256(t) + a256(64 * 8 * 4) + a256(64 * 3 * N * strips * 8)
                + a256(64 * 8) + a256(128 * 4 * 64 * 144 * 4) + a256(32 * 256 * 8) + a256(512 * 64 * 244 * 8))
        assert work(N, H, W, s) == want, (N, H, W, s)
    for f in (saved, work):
        assert f(2, 16, 16, 2) < f(3, 16, 16, 2) and f(2, 16, 16, 2) < f(2, 17, 16, 2) < f(2, 17, 17, 2) and f(2, 16, 16, 2) < f(2, 16, 16, 4)
    for fn in (L.cid_sr_saved_bytes, L.cid_sr_backward_workspace_bytes):
        assert fn(2, 8, 8, 2, None) == ERR_INVALID and fn(2, 8, 8, 3, ctypes.byref(n)) == ERR_INVALID
        for bad in ((0, 8, 8, 2), (1, 0, 8, 2), (1, 8, -1, 2), (1, 1 << 15, 1 << 13, 4), (1, 1, 1, 1)):
            assert fn(*bad, ctypes.byref(n)) == ERR_SHAPE, bad


def test_c_abi_argument_errors_need_no_gpu():
    L = _lib.lib()
    h = _handle(L, 2)
    fake, odd = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 2)
    off = ctypes.c_void_p((1 << 20) + 128)
    big = 1 << 40
    sv, ws, tw = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    assert L.cid_sr_saved_bytes(2, 13, 18, 2, ctypes.byref(sv)) == 0 and L.cid_sr_backward_workspace_bytes(2, 13, 18, 2, ctypes.byref(ws)) == 0
    assert L.cid_sr_train_workspace_bytes(2, 13, 18, 2, ctypes.byref(tw)) == 0
    err = lambda: L.cid_sr_last_error(h)   # noqa: E731

    def bns(**change):
        arr = (_BnArg * 10)()
        for i in range(10):
            arr[i] = _BnArg(1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1e-5, 0.1)
        for k, v in change.items():
            setattr(arr[int(k[1:].split("_", 1)[0])], k.split("_", 1)[1], v)
        return arr

    def fwd(hh=h, i=fake, fi=0, o=fake, N=2, H=13, W=18, flags=0, bn=None, s=fake, sb=big, w=fake, wb=big):
        return L.cid_sr_forward_saved(hh, i, fi, o, N, H, W, flags, bns() if bn is None else bn, s, sb, w, wb, None)

    assert fwd(hh=None) == ERR_INVALID
    for kw in ({"i": None}, {"o": None}, {"s": None}, {"w": None}):
        assert fwd(**kw) == ERR_INVALID and b"cid_sr_forward_saved" in err(), kw
    assert L.cid_sr_forward_saved(h, fake, 0, fake, 2, 13, 18, 0, None, fake, big, fake, big, None) == ERR_INVALID
    assert fwd(bn=bns(l4_running_var=None)) == ERR_INVALID and b"null BatchNorm pointer" in err()
    assert fwd(bn=bns(l4_eps=-1.0)) == ERR_INVALID and fwd(bn=bns(l4_momentum=float("nan"))) == ERR_INVALID
    assert fwd(fi=2) == ERR_INVALID and fwd(i=odd) == ERR_INVALID and fwd(o=odd) == ERR_INVALID
    assert fwd(flags=2) == ERR_INVALID and b"unknown flags" in err()
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0)):
        assert fwd(N=bad[0], H=bad[1], W=bad[2]) == ERR_SHAPE, bad
    assert fwd(N=1, H=1, W=1) == ERR_SHAPE and err() == b"Expected more than 1 value per channel when training"
    assert fwd(N=1, H=1 << 15, W=1 << 15) == ERR_SHAPE
    assert fwd(sb=sv.value - 1) == ERR_WORKSPACE and b"cid_sr_saved_bytes" in err() and b"saved buffer" in err()
    assert fwd(s=off) == ERR_WORKSPACE
    assert fwd(wb=tw.value - 1) == ERR_WORKSPACE and b"cid_sr_train_workspace_bytes" in err()
    assert fwd(w=off) == ERR_WORKSPACE
    assert fwd(sb=sv.value, wb=tw.value) == ERR_STATE and b"weights not uploaded" in err()
    assert fwd(i=odd, fi=1, flags=_lib.CID_SR_RAW, sb=sv.value, wb=tw.value) == ERR_STATE

    def bwd(hh=h, i=fake, fi=0, go=fake, N=2, H=13, W=18, flags=0, bn=None, s=fake, sb=big, g=None, w=fake, wb=big, null_g=False):
        gr = _GradsArg() if g is None else g
        return L.cid_sr_backward(hh, i, fi, go, N, H, W, flags, bns() if bn is None else bn, s, sb, None if null_g else ctypes.byref(gr), w, wb,
                                 None)

    assert bwd(hh=None) == ERR_INVALID
    for kw in ({"i": None}, {"go": None}, {"s": None}, {"w": None}, {"null_g": True}):
        assert bwd(**kw) == ERR_INVALID and b"cid_sr_backward: null pointer" in err(), kw
    assert L.cid_sr_backward(h, fake, 0, fake, 2, 13, 18, 0, None, fake, big, ctypes.byref(_GradsArg()), fake, big, None) == ERR_INVALID
    assert bwd(bn=bns(l7_gamma=None)) == ERR_INVALID and b"null BatchNorm pointer" in err()
    assert bwd(bn=bns(l7_beta=None, l2_running_mean=None, l0_num_batches_tracked=None), sb=sv.value, wb=ws.value) == ERR_STATE   # only gamma is read
    assert bwd(fi=2) == ERR_INVALID and bwd(i=odd) == ERR_INVALID and bwd(go=odd) == ERR_INVALID
    assert bwd(flags=4) == ERR_INVALID and b"unknown flags" in err()
    g = _GradsArg()
    g.up_w[1] = (1 << 20) + 1
    assert bwd(g=g) == ERR_INVALID and b"misaligned gradient tensor" in err()
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0)):
        assert bwd(N=bad[0], H=bad[1], W=bad[2]) == ERR_SHAPE, bad
    assert bwd(N=1, H=1, W=1) == ERR_SHAPE and err() == b"Expected more than 1 value per channel when training"
    assert bwd(sb=sv.value - 1) == ERR_WORKSPACE and b"cid_sr_saved_bytes" in err()
    assert bwd(s=off) == ERR_WORKSPACE
    assert bwd(wb=ws.value - 1) == ERR_WORKSPACE and b"cid_sr_backward_workspace_bytes" in err()
    assert bwd(w=off) == ERR_WORKSPACE
    assert bwd(sb=sv.value, wb=ws.value) == ERR_STATE and b"weights not uploaded" in err()
    assert bwd(i=odd, fi=1, flags=_lib.CID_SR_RAW, sb=sv.value, wb=ws.value) == ERR_STATE
    L.cid_sr_destroy(h)

    masks = (ctypes.c_void_p * 9)(*([1 << 20] * 9))
    mk = lambda *a: L.cid_sr_saved_masks(*a, None)   # noqa: E731
    assert mk(None, big, 2, 13, 18, 2, masks) == ERR_INVALID and mk(fake, big, 2, 13, 18, 2, None) == ERR_INVALID
    assert mk(fake, big, 2, 13, 18, 3, masks) == ERR_INVALID and mk(fake, big, 0, 13, 18, 2, masks) == ERR_SHAPE
    assert mk(fake, sv.value - 1, 2, 13, 18, 2, masks) == ERR_WORKSPACE and mk(off, big, 2, 13, 18, 2, masks) == ERR_WORKSPACE
    short = (ctypes.c_void_p * 9)(*([1 << 20] * 6 + [None] * 3))
    assert mk(fake, big, 2, 13, 18, 2, short) == ERR_INVALID        # scale 2 has a seventh mask


def test_device_pack_argument_errors_need_no_gpu():
    L = _lib.lib()
    fake = 1 << 20
    for scale, count in ((1, 52), (2, 55), (8, 61)):
        h = _handle(L, scale)
        bn = (_BnArg * 10)(*[_BnArg(fake, fake, fake, fake, fake, 1e-5, 0.1) for _ in range(10)])
        ptrs = (ctypes.c_void_p * count)(*([fake] * count))
        assert count == len(ref.param_names(scale.bit_length() - 1))
        pack = lambda hh=h, p=ptrs, b=bn, blob=ctypes.c_void_p(fake): L.cid_sr_pack_weights_device(hh, p, b, blob, None)   # noqa: E731
        assert pack(hh=None) == ERR_INVALID and pack(p=None) == ERR_INVALID and pack(b=None) == ERR_INVALID and pack(blob=None) == ERR_INVALID
        assert b"cid_sr_pack_weights_device: null pointer" in L.cid_sr_last_error(h)
        for i in (0, count // 2, count - 1):
            for bad in (None, fake + 2):
                q = (ctypes.c_void_p * count)(*([fake] * count))
                q[i] = bad
                assert pack(p=q) == ERR_INVALID and b"null or misaligned parameter pointer" in L.cid_sr_last_error(h), (i, bad)
        for field in ("gamma", "beta", "running_mean", "running_var"):
            b2 = (_BnArg * 10)(*[_BnArg(fake, fake, fake, fake, fake, 1e-5, 0.1) for _ in range(10)])
            setattr(b2[6], field, None)
            assert pack(b=b2) == ERR_INVALID and b"null BatchNorm pointer" in L.cid_sr_last_error(h), field
        b2 = (_BnArg * 10)(*[_BnArg(fake, fake, fake, fake, fake, float("nan") if i == 3 else 1e-5, 0.1) for i in range(10)])
        assert pack(b=b2) == ERR_INVALID and b"eps" in L.cid_sr_last_error(h)
        assert pack(blob=ctypes.c_void_p(fake + 128)) == ERR_WORKSPACE and b"256-byte aligned" in L.cid_sr_last_error(h)
        L.cid_sr_destroy(h)
