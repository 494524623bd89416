"""The backward pass of the ESRGAN generator without a GPU: tests/esrgan_backward_ref.py (the reference the GPU tests of
cid_esr_backward measure against) held to the stock nn layers under autograd, the conditioning of the GPU parity cases under the rule
of error stated there, the host argument checks and size formulas of cid_esr_saved_bytes / cid_esr_forward_saved /
cid_esr_backward_workspace_bytes / cid_esr_backward / cid_esr_pack_weights_device / cid_esr_saved_masks (include/cid.h), and the
module's opt-in flags."""
import ctypes
import os
import sys

import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth
from celebrity_image_denoiser_amd.discriminator import _BnArg
from celebrity_image_denoiser_amd.esrgan import ESRGANGenerator, _GradsArg, _set_grad, load_esrgan

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import esrgan_backward_ref as ref  # noqa: E402
import esrgan_train_oracle as oracle  # noqa: E402

ERR_INVALID, ERR_SHAPE, ERR_KEY, ERR_STATE, ERR_WORKSPACE = 1, 2, 3, 4, 5


@pytest.mark.parametrize("wset", ["default", "hot"])
def test_fp32_reference_is_the_stock_module_under_autograd(wset):
    """The reference on fp32 with its own masks against loss.backward() through stock nn.Conv2d / BatchNorm2d / PReLU in train mode,
    the blocks' skips and the outer skip included.  Both run ATen fp32 on the same operands; only PReLU's backward is written by hand
    here, so every tensor agrees to well inside the rule's 1e-5 (the slopes' sums are taken in another order)."""
    case, r = (3, 8, 12), 2
    n, h, w = case
    sd = synth.make_esrgan_state_dict(wset, r)
    x, G = oracle.case_input(case), ref.grad_out(n, h, w)
    got, pre, out, book = ref.ref_backward(sd, x, G, r, torch.float32)
    m, _ = oracle.stock_generator(sd, r)
    x1 = m.initial(torch.from_numpy(x))
    y = m.final(x1 + m.residuals(x1))
    (y * G).sum().backward()
    assert torch.equal(y.detach(), out)
    want = {k: p.grad for k, p in m.named_parameters()}
    assert list(want) == ref.param_names(r) == list(got)
    assert len(pre) == 1 + r and set(book) == set(ref.slope_names(r))
    errs = ref.rel_errors(got, {k: v.double() for k, v in want.items()}, book)
    worst = max(errs, key=errs.get)
    print(f"{wset}: worst {worst} at {errs[worst]:.2e}")
    assert errs[worst] <= 1e-6, (worst, errs[worst])


@pytest.mark.parametrize("rc", ref.CASES, ids=ref.case_id)
@pytest.mark.parametrize("wset", ["default", "hot"])
def test_parity_inputs_are_well_conditioned(wset, rc):
    """ATen fp32 itself is within the mask cap (asserted inside aten_errors) and within the plain 1e-5 on every tensor of every
    GPU parity case, under the rule of error of esrgan_backward_ref."""
    errs, flips = ref.aten_errors(wset, rc)
    worst = max(errs, key=errs.get)
    print(f"{wset} {ref.case_id(rc)}: ATen fp32 {flips} mask flips, worst {worst} at {errs[worst]:.2e}")
    assert errs[worst] <= ref.TOL, (worst, errs[worst])


@pytest.mark.parametrize("slope", [0.0, -0.5])
def test_slope_cases_are_well_conditioned(slope):
    case, r = (3, 8, 12), 2
    sd = dict(synth.make_esrgan_state_dict("default", r))
    for k in ref.slope_names(r):
        sd[k] = sd[k] * 0 + slope
    errs, _ = ref.aten_errors("default", (r, case), sd=sd, tag=slope)
    assert max(errs.values()) <= ref.TOL


def test_the_split_case_exceeds_every_cap_of_the_weight_gradients():
    """esrgan_backward_ref.SPLIT_CASE against the caps cid_esr_backward uses (kSrWgSplits = 128, kSrW9Splits = 256, kSrTwSplits = 512
    of csrc/api/srgan_backward.h) and the kernels' item geometry: 528, 1056 and 528 items, more than the cap in all three launches, an
    uneven partition, and in each launch a workgroup whose range [items*k/splits, items*(k+1)/splits) holds items of two images.  No
    other shape has more items than a cap."""
    def launches(n, h, w):
        tiles = -(-h // 4) * -(-w // 16)
        return [(n * tiles, tiles, 128), (n * h * -(-w // 32), h * -(-w // 32), 256), (n * tiles, tiles, 512)]

    for case in oracle.PARITY_CASES:
        assert all(items <= cap for items, _, cap in launches(*case)), case
    got = launches(*ref.SPLIT_CASE)
    assert [items for items, _, _ in got] == [528, 1056, 528]
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
        ESRGANGenerator(2, autograd=True)
    with pytest.raises(ValueError, match="needs batch_stats=True"):
        ESRGANGenerator(2, False, True)
    assert "autograd" in load_esrgan.__code__.co_varnames
    m = ESRGANGenerator(3, batch_stats=True, autograd=True)
    assert list(m.state_dict()) == list(ESRGANGenerator(3).state_dict())
    assert [k for k, _ in m.named_parameters()] == ref.param_names(3)
    m.train()
    with pytest.raises(RuntimeError, match="GPU-only"):
        m(torch.zeros(1, 3, 4, 4))


def test_every_parameter_has_its_slot_in_cid_esr_grads():
    names = ref.param_names(16)
    g = _GradsArg()
    for i, k in enumerate(names):
        _set_grad(g, k, 4 * (i + 1))
    flat = (ctypes.c_void_p * (ctypes.sizeof(g) // ctypes.sizeof(ctypes.c_void_p))).from_buffer(g)
    assert sorted(flat) == [4 * (i + 1) for i in range(len(names))] and len(flat) == 3 + 4 * 32 + 16 + 2 == len(names)
    assert g.head_w == 4 and g.head_b == 8 and g.head_slope == 12 and g.conv_w[0] == 16 and g.conv_b[0] == 20 and g.gamma[0] == 24
    assert g.beta[0] == 28 and g.slope[0] == 32 and g.conv_w[1] == 36 and g.conv_b[1] == 40 and g.gamma[1] == 44 and g.beta[1] == 48
    assert g.beta[31] == 4 * (names.index("residuals.15.block.4.bias") + 1) and g.slope[15] == 4 * (names.index("residuals.15.block.2.weight") + 1)
    assert g.final_w == 4 * (len(names) - 1) and g.final_b == 4 * len(names)


def _handle(L, r):
    h = ctypes.c_void_p()
    assert L.cid_esr_create(ctypes.byref(h), r) == 0
    return h


def test_size_formulas_are_exact_and_monotone():
    L = _lib.lib()
    n = ctypes.c_size_t()
    a256 = lambda v: (v + 255) // 256 * 256   # noqa: E731

    def saved(N, H, W, r):
        assert L.cid_esr_saved_bytes(N, H, W, r, ctypes.byref(n)) == 0
        return n.value

    def work(N, H, W, r):
        assert L.cid_esr_backward_workspace_bytes(N, H, W, r, ctypes.byref(n)) == 0
        return n.value

    for r, (N, H, W) in ref.CASES + [(8, (8, 256, 256)), (3, (2, 3, 5)), (0, (1, 1, 1))]:
        t = N * 64 * H * W * 4
        assert saved(N, H, W, r) == (3 * r + 1 if r else 2) * a256(t) + a256(2 * r * 128 * 4) + a256(2 * r * 128 * 8), (r, N, H, W)
        strips = (H * W + 511) // 512
        want = ((4 if r else 2) * a256(t) + a256(64 * 8 * 4) + a256(64 * 3 * N * strips * 8) + a256(64 * 8) + a256(128 * 4 * 64 * 144 * 4)
                + a256(128 * 64 * 8) + a256(512 * 64 * 244 * 8))
        assert work(N, H, W, r) == want, (r, N, H, W)
    assert saved(8, 256, 256, 8) == 25 * 8 * 64 * 256 * 256 * 4 + 2 * 8 * 128 * 12          # 3.36 GB at the trainer's shape
    for f in (saved, work):
        assert f(2, 16, 16, 2) < f(3, 16, 16, 2) and f(2, 16, 16, 2) < f(2, 17, 16, 2) < f(2, 17, 17, 2)
    assert saved(2, 16, 16, 0) < saved(2, 16, 16, 1) < saved(2, 16, 16, 2) < saved(2, 16, 16, 16)
    assert work(2, 16, 16, 0) < work(2, 16, 16, 1) == work(2, 16, 16, 16)
    for fn in (L.cid_esr_saved_bytes, L.cid_esr_backward_workspace_bytes):
        assert fn(2, 8, 8, 2, None) == ERR_INVALID and fn(2, 8, 8, 17, ctypes.byref(n)) == ERR_INVALID and fn(2, 8, 8, -1, ctypes.byref(n)) == ERR_INVALID
        for bad in ((0, 8, 8, 2), (1, 0, 8, 2), (1, 8, -1, 2), (1, 1 << 16, 1 << 15, 2), (1, 1, 1, 1)):
            assert fn(*bad, ctypes.byref(n)) == ERR_SHAPE, bad
        assert fn(1, 1, 1, 0, ctypes.byref(n)) == 0


def test_c_abi_argument_errors_need_no_gpu():
    L = _lib.lib()
    R = 2
    h = _handle(L, R)
    fake, odd = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 2)
    off = ctypes.c_void_p((1 << 20) + 128)
    big = 1 << 40
    sv, ws, tw = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    assert L.cid_esr_saved_bytes(2, 13, 18, R, ctypes.byref(sv)) == 0 and L.cid_esr_backward_workspace_bytes(2, 13, 18, R, ctypes.byref(ws)) == 0
    assert L.cid_esr_train_workspace_bytes(2, 13, 18, R, ctypes.byref(tw)) == 0
    err = lambda: L.cid_esr_last_error(h)   # noqa: E731

    def bns(**change):
        arr = (_BnArg * (2 * R))()
        for i in range(2 * R):
            arr[i] = _BnArg(1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1e-5, 0.1)
        for k, v in change.items():
            setattr(arr[int(k[1:].split("_", 1)[0])], k.split("_", 1)[1], v)
        return arr

    def fwd(hh=h, i=fake, fi=0, o=fake, N=2, H=13, W=18, bn=None, s=fake, sb=big, w=fake, wb=big):
        return L.cid_esr_forward_saved(hh, i, fi, o, N, H, W, bns() if bn is None else bn, s, sb, w, wb, None)

    assert fwd(hh=None) == ERR_INVALID
    for kw in ({"i": None}, {"o": None}, {"s": None}, {"w": None}):
        assert fwd(**kw) == ERR_INVALID and b"cid_esr_forward_saved: null pointer" in err(), kw
    assert L.cid_esr_forward_saved(h, fake, 0, fake, 2, 13, 18, None, fake, big, fake, big, None) == ERR_INVALID
    assert fwd(bn=bns(l3_running_var=None)) == ERR_INVALID and b"null BatchNorm pointer" in err()
    assert fwd(bn=bns(l1_eps=-1.0)) == ERR_INVALID and fwd(bn=bns(l2_momentum=float("nan"))) == ERR_INVALID
    assert fwd(fi=2) == ERR_INVALID and fwd(i=odd) == ERR_INVALID and fwd(o=odd) == ERR_INVALID
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0)):
        assert fwd(N=bad[0], H=bad[1], W=bad[2]) == ERR_SHAPE, bad
    assert fwd(N=1, H=1, W=1) == ERR_SHAPE and err() == b"Expected more than 1 value per channel when training"
    assert fwd(N=1, H=1 << 16, W=1 << 15) == ERR_SHAPE
    assert fwd(sb=sv.value - 1) == ERR_WORKSPACE and b"cid_esr_saved_bytes" in err() and b"saved buffer" in err()
    assert fwd(s=off) == ERR_WORKSPACE
    assert fwd(wb=tw.value - 1) == ERR_WORKSPACE and b"cid_esr_train_workspace_bytes" in err()
    assert fwd(w=off) == ERR_WORKSPACE
    assert fwd(sb=sv.value, wb=tw.value) == ERR_STATE and b"weights not uploaded" in err()
    assert fwd(i=odd, fi=1, sb=sv.value, wb=tw.value) == ERR_STATE

    def bwd(hh=h, i=fake, fi=0, go=fake, N=2, H=13, W=18, bn=None, s=fake, sb=big, g=None, w=fake, wb=big, null_g=False):
        gr = _GradsArg() if g is None else g
        return L.cid_esr_backward(hh, i, fi, go, N, H, W, bns() if bn is None else bn, s, sb, None if null_g else ctypes.byref(gr), w, wb, None)

    assert bwd(hh=None) == ERR_INVALID
    for kw in ({"i": None}, {"go": None}, {"s": None}, {"w": None}, {"null_g": True}):
        assert bwd(**kw) == ERR_INVALID and b"cid_esr_backward: null pointer" in err(), kw
    assert L.cid_esr_backward(h, fake, 0, fake, 2, 13, 18, None, fake, big, ctypes.byref(_GradsArg()), fake, big, None) == ERR_INVALID
    assert b"cid_esr_backward: null pointer" in err()
    assert bwd(bn=bns(l3_gamma=None)) == ERR_INVALID and b"null BatchNorm pointer" in err()
    assert bwd(bn=bns(l3_beta=None, l2_running_mean=None, l0_num_batches_tracked=None), sb=sv.value, wb=ws.value) == ERR_STATE   # only gamma is read
    assert bwd(fi=2) == ERR_INVALID and b"unknown format or misaligned fp32 operand" in err()
    assert bwd(i=odd) == ERR_INVALID and bwd(go=odd) == ERR_INVALID and b"misaligned grad_out" in err()
    g = _GradsArg()
    g.gamma[31] = (1 << 20) + 1
    assert bwd(g=g) == ERR_INVALID and b"misaligned gradient tensor" in err()
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0)):
        assert bwd(N=bad[0], H=bad[1], W=bad[2]) == ERR_SHAPE and b"input shape not accepted" in err(), bad
    assert bwd(N=1, H=1, W=1) == ERR_SHAPE and err() == b"Expected more than 1 value per channel when training"
    assert bwd(sb=sv.value - 1) == ERR_WORKSPACE and b"cid_esr_saved_bytes" in err() and b"saved buffer" in err()
    assert bwd(s=off) == ERR_WORKSPACE
    assert bwd(wb=ws.value - 1) == ERR_WORKSPACE and b"cid_esr_backward_workspace_bytes" in err()
    assert bwd(w=off) == ERR_WORKSPACE
    assert bwd(sb=sv.value, wb=ws.value) == ERR_STATE and b"weights not uploaded" in err()
    assert bwd(i=odd, fi=1, sb=sv.value, wb=ws.value) == ERR_STATE
    L.cid_esr_destroy(h)

    # R = 0: no BatchNorm, bn may be null, one value per channel is accepted
    h0 = _handle(L, 0)
    assert L.cid_esr_saved_bytes(1, 1, 1, 0, ctypes.byref(sv)) == 0 and L.cid_esr_backward_workspace_bytes(1, 1, 1, 0, ctypes.byref(ws)) == 0
    assert L.cid_esr_forward_saved(h0, fake, 0, fake, 1, 1, 1, None, fake, sv.value, fake, big, None) == ERR_STATE
    assert L.cid_esr_backward(h0, fake, 0, fake, 1, 1, 1, None, fake, sv.value, ctypes.byref(_GradsArg()), fake, ws.value, None) == ERR_STATE
    L.cid_esr_destroy(h0)

    masks = (ctypes.c_void_p * 3)(*([1 << 20] * 3))
    mk = lambda *a: L.cid_esr_saved_masks(*a, None)   # noqa: E731
    assert L.cid_esr_saved_bytes(2, 13, 18, R, ctypes.byref(sv)) == 0
    assert mk(None, big, 2, 13, 18, R, masks) == ERR_INVALID and mk(fake, big, 2, 13, 18, R, None) == ERR_INVALID
    assert mk(fake, big, 2, 13, 18, 17, masks) == ERR_INVALID and mk(fake, big, 0, 13, 18, R, masks) == ERR_SHAPE
    assert mk(fake, sv.value - 1, 2, 13, 18, R, masks) == ERR_WORKSPACE and mk(off, big, 2, 13, 18, R, masks) == ERR_WORKSPACE
    short = (ctypes.c_void_p * 3)(*([1 << 20] * 2 + [None]))
    assert mk(fake, big, 2, 13, 18, R, short) == ERR_INVALID        # R = 2 has a third mask


def test_device_pack_argument_errors_need_no_gpu():
    L = _lib.lib()
    fake = 1 << 20
    for r, count in ((0, 5), (1, 14), (16, 149)):
        h = _handle(L, r)
        nb = max(2 * r, 1)
        bn = (_BnArg * nb)(*[_BnArg(fake, fake, fake, fake, fake, 1e-5, 0.1) for _ in range(nb)])
        ptrs = (ctypes.c_void_p * count)(*([fake] * count))
        assert count == len(ref.param_names(r))
        pack = lambda hh=h, p=ptrs, b=bn, blob=ctypes.c_void_p(fake): L.cid_esr_pack_weights_device(hh, p, b, blob, None)   # noqa: E731
        assert pack(hh=None) == ERR_INVALID and pack(p=None) == ERR_INVALID and pack(blob=None) == ERR_INVALID
        assert b"cid_esr_pack_weights_device: null pointer" in L.cid_esr_last_error(h)
        for i in (0, count // 2, count - 1):
            for bad in (None, fake + 2):
                q = (ctypes.c_void_p * count)(*([fake] * count))
                q[i] = bad
                assert pack(p=q) == ERR_INVALID and b"null or misaligned parameter pointer" in L.cid_esr_last_error(h), (i, bad)
        if r:
            assert pack(b=None) == ERR_INVALID and b"null pointer" in L.cid_esr_last_error(h)
            for field in ("gamma", "beta", "running_mean", "running_var"):
                b2 = (_BnArg * nb)(*[_BnArg(fake, fake, fake, fake, fake, 1e-5, 0.1) for _ in range(nb)])
                setattr(b2[nb - 1], field, None)
                assert pack(b=b2) == ERR_INVALID and b"null BatchNorm pointer" in L.cid_esr_last_error(h), field
            b2 = (_BnArg * nb)(*[_BnArg(fake, fake, fake, fake, fake, float("nan") if i == 1 else 1e-5, 0.1) for i in range(nb)])
            assert pack(b=b2) == ERR_INVALID and b"eps" in L.cid_esr_last_error(h)
        assert pack(blob=ctypes.c_void_p(fake + 128)) == ERR_WORKSPACE and b"256-byte aligned" in L.cid_esr_last_error(h)
        L.cid_esr_destroy(h)
