"""The VGG content loss's input gradient on the GPU: cid_vgg_content_loss_saved and cid_vgg_content_backward (include/cid.h, which
holds the definitions) and VGGPerceptualLoss(autograd=True) in lpips.py.

The reference is vgg16.features[:16] in float64 on the CPU, from lpips_vgg_oracle.weights(wset).  ReLU and max-pool make the gradient
discontinuous, so each fp32 run (the device's and ATen's) is compared with a float64 backward that takes THAT run's discontinuities
(vgg_backward_ref.py): the seven ReLU masks and the two pool routings; the device's come out of the arena through cid_vgg_saved_view.
The sharing is capped (vgg_backward_ref.check_masks, check_routing): a mask may differ from float64's only where |pre64| <= 1e-5 max,
a routing only where the two candidates' float64 values differ by <= 1e-5 max, each at no more than max(2, ceil(1e-5 units)) units.

Error e(T) = max|g - g64| / max|g64|; bound e_hip(T) <= max(1e-5, 2 e_aten(T)) for grad_x and for every stored gradient tensor, with
e_aten measured in the same test on ATen fp32 autograd (CPU) against float64 with ATen's own masks and routing.

Shapes (H, W, N): (4,4,2) the smallest, relu3 is 1x1; (4,4,130) a 128-column run of 1x1 maps spans 128 images and a second workgroup
starts mid-batch; (5,7,3) and (17,19,3) odd floors at both pools, the unrouted last row and column; (35,47,3) runs that cross image
boundaries; (64,64,2); (4,512,1) the wide plane in the full-resolution data gradient."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import celebrity_image_denoiser_amd as cid
from celebrity_image_denoiser_amd import _lib, synth
from celebrity_image_denoiser_amd.lpips import load_vgg_loss

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_vgg_oracle as oracle  # noqa: E402
import vgg_backward_ref as ref  # noqa: E402
from test_vgg_backward_host import backward_blob  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ((4, 4, 2), (4, 4, 130), (5, 7, 3), (17, 19, 3), (35, 47, 3), (64, 64, 2), (4, 512, 1))
_LOSSES, _PAIRS, _F64 = {}, {}, {}
case_id = lambda c: f"{c[0]}x{c[1]}n{c[2]}"   # noqa: E731


def loss_of(wset, autograd=True):
    key = (wset, autograd)
    if key not in _LOSSES:
        sd = {k: torch.from_numpy(v) for k, v in synth.vgg_loss_state_dict(oracle.weights(wset)).items()}
        _LOSSES[key] = load_vgg_loss(sd, device=DEV, autograd=autograd)
    return _LOSSES[key]


def pairs_of(kind, case):
    key = (kind, case)
    if key not in _PAIRS:
        h, w, n = case
        _PAIRS[key] = oracle.pairs(kind, n, h, w, oracle.first_index(h, w, n))
        for v in _PAIRS[key]:
            v.setflags(write=False)
    return _PAIRS[key]


def forward64_of(wset, kind, case, unit=False):
    """The float64 forward of both towers: computed once, shared, never modified."""
    key = (wset, kind, case, unit)
    if key not in _F64:
        a, b, _, _ = pairs_of(kind, case)
        _F64[key] = (ref.forward64(oracle.weights(wset), a, unit), ref.forward64(oracle.weights(wset), b, unit))
    return _F64[key]


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


def saved_bytes(n, h, w):
    need = ctypes.c_size_t()
    assert _lib.lib().cid_vgg_saved_bytes(n, h, w, ctypes.byref(need)) == 0
    return need.value


def view(arena, name, n, h, w):
    """A tensor of the arena as fp32 [images,C,Hs,Ws] on the CPU (a copy), through cid_vgg_saved_view."""
    off, im, c, hs, ws, cb = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert _lib.lib().cid_vgg_saved_view(name.encode(), n, h, w, *[ctypes.byref(v) for v in (off, im, c, hs, ws, cb)]) == 0
    count = im.value * c.value * hs.value * ws.value
    t = arena[off.value:off.value + 4 * count].view(torch.float32)
    t = t.view(im.value, c.value // cb.value, hs.value, ws.value, cb.value).permute(0, 1, 4, 2, 3)
    return t.reshape(im.value, c.value, hs.value, ws.value).cpu()


def cabi(m, a, b, grad_out, unit=False, arena=None, fmt_b=0):
    """cid_vgg_content_loss_saved + cid_vgg_content_backward at m's weights -> (out, grad_x, arena), device tensors."""
    L = _lib.lib()
    n, _, h, w = a.shape
    m.pack_weights()
    m._pack_backward_weights()
    if arena is None:
        arena = torch.empty(saved_bytes(n, h, w), dtype=torch.uint8, device=DEV)
    out = torch.empty(n, dtype=torch.float64, device=DEV)
    gx = torch.empty((n, 3, h, w), dtype=torch.float32, device=DEV)
    flags = _lib.CID_LPIPS_UNIT_VIEW if unit else 0
    _lib.check_vgg(m._cid, L.cid_vgg_content_loss_saved(m._cid, a.data_ptr(), 0, b.data_ptr(), fmt_b, n, h, w, flags, out.data_ptr(),
                                                        arena.data_ptr(), arena.numel(), stream()))
    go = grad_out.to(DEV, torch.float64).contiguous()
    _lib.check_vgg(m._cid, L.cid_vgg_content_backward(m._cid, go.data_ptr(), gx.data_ptr(), n, h, w, flags, arena.data_ptr(), arena.numel(),
                                                      stream()))
    torch.cuda.synchronize()
    return out, gx, arena


def device_discontinuities(arena, n, h, w):
    """Tower a's masks (saved activation > 0) and routings (max_pool2d's indices on the saved fp32 relu1_2 and relu2_2)."""
    acts = [view(arena, name, n, h, w)[:n] for name in ref.ACTS]
    return ref.own_discontinuities(acts)


def check_gradients(wset, kind, case, unit, grad_out, gx, arena, what):
    """grad_x and the seven stored gradient tensors against float64 with the device's discontinuities, under the bound measured on
    ATen fp32 with its own."""
    h, w, n = case
    sd = oracle.weights(wset)
    a, b, _, _ = pairs_of(kind, case)
    (pre_a, act_a), (_, act_b) = forward64_of(wset, kind, case, unit)
    masks, routes = device_discontinuities(arena, n, h, w)
    ref.check_masks(masks, pre_a, what)
    ref.check_routing(routes, act_a, what)
    g64 = ref.backward64(sd, act_a, act_b[6], grad_out, masks, routes, unit)
    g_aten, m_aten, r_aten = ref.aten_fp32(sd, a, b, grad_out, unit)
    g64_aten = ref.backward64(sd, act_a, act_b[6], grad_out, m_aten, r_aten, unit)
    got = {name: view(arena, name, n, h, w) for name in ref.GRADS}
    got["grad_x"] = gx.cpu()
    for name in ("grad_x",) + ref.GRADS:
        assert got[name].shape == g64[name].shape, (what, name)
        assert bool(torch.isfinite(got[name]).all()), (what, name)
        e_hip, e_aten = ref.rel_err(got[name], g64[name]), ref.rel_err(g_aten[name], g64_aten[name])
        bound = max(1e-5, 2 * e_aten)
        print(f"{what} {name}: e_hip {e_hip:.3e}, e_aten {e_aten:.3e}, bound {bound:.3e} (margin {bound / max(e_hip, 1e-300):.1f}x), "
              f"max|g64| {float(g64[name].abs().max()):.4g}")
        assert e_hip <= bound, (what, name, e_hip, bound)


@pytest.mark.parametrize("wset", ["default", "hot"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gradient_parity(case, wset):
    """The trainer's scalar (the mean over the batch: grad_out = 1 / N) on noisy / clean and on unrelated pairs."""
    m = loss_of(wset)
    h, w, n = case
    for kind in ("noisy", "unrelated"):
        a, b, _, _ = pairs_of(kind, case)
        go = torch.full((n,), 1.0 / n, dtype=torch.float64)
        out, gx, arena = cabi(m, dev(a), dev(b), go)
        check_gradients(wset, kind, case, False, go.numpy(), gx, arena, f"{wset} {kind} {case}")


@pytest.mark.parametrize("wset", ["default", "hot"])
@pytest.mark.parametrize("case", [(4, 4, 2), (5, 7, 3), (35, 47, 3), (4, 512, 1)], ids=case_id)
def test_saved_forward_is_the_plain_forward(case, wset):
    """cid_vgg_content_loss_saved gives the bits of cid_vgg_content_loss, in both views and with a uint8 second operand; the seven
    saved activations of both towers stand within the tap bound of the float64 forward, and the three the plain call keeps are its
    bits."""
    m = loss_of(wset)
    h, w, n = case
    a, b, _, b8 = pairs_of("noisy", case)
    ta, tb = dev(a), dev(b)
    go = torch.ones(n, dtype=torch.float64)
    for unit in (False, True):
        want = m.per_image(ta, tb, unit_view=unit)
        assert not want.requires_grad
        out, _, arena = cabi(m, ta, tb, go, unit)
        assert torch.equal(out, want)
        out8, _, _ = cabi(m, ta, dev(b8), go, unit, fmt_b=1)
        assert torch.equal(out8, want)
        (_, act_a), (_, act_b) = forward64_of(wset, "noisy", case, unit)
        for i, name in enumerate(ref.ACTS):
            got = view(arena, name, n, h, w).double()
            want64 = torch.cat([act_a[i], act_b[i]], dim=0)
            bound = oracle.bound(want64.numpy())
            err = float((got - want64).abs().max())
            print(f"saved {wset} {case} unit={int(unit)} {name}: max|delta| {err:.3e}, bound {bound:.3e} (margin {bound / max(err, 1e-300):.1f}x)")
            assert got.shape == want64.shape and err <= bound, (name, err, bound)
        for tap, name in (("relu1", "relu1_2"), ("relu2", "relu2_2"), ("relu3", "relu3_3")):
            assert torch.equal(m.stage(tap, n, h, w).cpu(), view(arena, name, n, h, w)), name


@pytest.mark.parametrize("wset", ["default", "hot"])
def test_backward_blob(wset):
    """The uploaded backward blob is the numpy restatement of the pack (the flip, the transpose, oracle.windex), word for word, and
    the forward blob is still what lpips_vgg_oracle.packed_blob restates."""
    m = loss_of(wset)
    m.pack_weights()
    got = m._pack_backward_weights().view(torch.float32).cpu().numpy()
    assert np.array_equal(got, backward_blob(oracle.weights(wset)))
    want = oracle.packed_blob(oracle.weights(wset))
    fwd = m.pack_weights().view(torch.float32).cpu().numpy()
    end = 27 * 64 + 64
    assert np.array_equal(fwd[:end], want[:end])
    off = 27 * 64 + 128
    size = sum(co * ci * 9 + co for ci, co in ((64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256)))
    assert np.array_equal(fwd[off:off + size], want[off:off + size])


@pytest.mark.parametrize("case", [(17, 19, 5), (35, 47, 5)], ids=case_id)
def test_batch_and_position_independence(case):
    """grad_x of a pair is bit-identical alone, in a batch of 5 at positions 0 and 4, and whatever grad_out the other images have;
    two runs are bit-identical."""
    m = loss_of("default")
    h, w, n = case
    a, b, _, _ = pairs_of("unrelated", case)
    ta, tb = dev(a), dev(b)
    go = torch.tensor([0.7, -1.3, 2.0, 0.01, 5.5], dtype=torch.float64)
    out, gx, _ = cabi(m, ta, tb, go)
    out2, gx2, _ = cabi(m, ta, tb, go)
    assert torch.equal(gx, gx2) and torch.equal(out, out2)
    for i in (0, 2, 4):
        _, g1, _ = cabi(m, ta[i:i + 1].contiguous(), tb[i:i + 1].contiguous(), go[i:i + 1])
        assert torch.equal(g1[0], gx[i]), i
    perm = torch.tensor([4, 1, 2, 3, 0], device=DEV)
    go_other = torch.tensor([0.7, 9.0, -4.0, 100.0, 5.5], dtype=torch.float64)
    _, gp, _ = cabi(m, ta[perm].contiguous(), tb[perm].contiguous(), go_other[perm.cpu()])
    assert torch.equal(gp[4], gx[0]) and torch.equal(gp[0], gx[4])
    # a zero grad_out gives an exactly zero gradient for that image alone
    gz = go.clone()
    gz[2] = 0.0
    _, g0, _ = cabi(m, ta, tb, gz)
    assert float(g0[2].abs().max()) == 0.0 and torch.equal(g0[[0, 1, 3, 4]], gx[[0, 1, 3, 4]])


@pytest.mark.parametrize("wset", ["default", "hot"])
def test_non_uniform_grad_out_through_the_module(wset):
    """(loss.per_image(x, y) * weights).sum().backward() meets the same bound, stored tensors included."""
    m = loss_of(wset)
    case = (17, 19, 3)
    h, w, n = case
    a, b, _, _ = pairs_of("unrelated", case)
    weights = torch.tensor([0.25, 3.0, -1.5], dtype=torch.float64)
    x = dev(a).requires_grad_(True)
    per = m.per_image(x, dev(b))
    assert per.requires_grad and per.dtype == torch.float64
    arena = per.grad_fn.saved
    (per * weights.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    check_gradients(wset, "unrelated", case, False, weights.numpy(), x.grad, arena, f"module weights {wset}")


def test_unit_view_carries_the_half_exactly():
    """Under unit_view=True the gradient is, bit for bit, 0.5 times that of a call whose operands are x*0.5+0.5."""
    m = loss_of("hot")
    case = (17, 19, 3)
    a, b, _, _ = pairs_of("noisy", case)
    ta, tb = dev(a), dev(b)
    go = torch.tensor([1.0, 0.3, 2.5], dtype=torch.float64)
    out_u, g_u, _ = cabi(m, ta, tb, go, unit=True)
    out_p, g_p, _ = cabi(m, ta * 0.5 + 0.5, tb * 0.5 + 0.5, go, unit=False)
    assert torch.equal(out_u, out_p)
    assert float(g_p.abs().max()) > 0 and torch.equal(g_u, g_p * 0.5)
    check_gradients("hot", "noisy", case, True, go.numpy(), g_u, cabi(m, ta, tb, go, unit=True)[2], "unit view")
    # and through the module
    x = ta.clone().requires_grad_(True)
    (m.per_image(x, tb, unit_view=True) * go.to(DEV)).sum().backward()
    assert torch.equal(x.grad, g_u)


def test_module_behaviour():
    plain, auto = loss_of("default", autograd=False), loss_of("default")
    case = (17, 19, 3)
    h, w, n = case
    a, b, a8, _ = pairs_of("noisy", case)
    ta, tb = dev(a), dev(b)
    want = plain(ta, tb)
    x = ta.clone().requires_grad_(True)
    # the default has no history, whatever the operand asks for
    assert not plain(x, tb).requires_grad and plain(x, tb).grad_fn is None and torch.equal(plain(x, tb), want)
    # autograd=True: the plain path under no_grad, for an operand that does not require grad and for a uint8 one: the same bits
    with torch.no_grad():
        out = auto(x, tb)
    assert out.grad_fn is None and torch.equal(out, want)
    out = auto(ta, tb)
    assert out.grad_fn is None and not out.requires_grad and torch.equal(out, want)
    assert auto.per_image(dev(a8), tb).grad_fn is None
    # the differentiable path: the same bits, fp32 scalar, history
    loss = auto(x, tb)
    assert loss.requires_grad and loss.dtype == torch.float32 and loss.dim() == 0 and torch.equal(loss.detach(), want)
    per = auto.per_image(x, tb)
    ctx = per.grad_fn
    assert ctx.saved is not None and ctx.saved.numel() == saved_bytes(n, h, w)
    per.mean().backward()
    assert ctx.saved is None                                   # the arena is released after backward
    g_first = x.grad.clone()
    assert bool(torch.isfinite(g_first).all()) and float(g_first.abs().max()) > 0
    with pytest.raises(RuntimeError, match="second time"):     # torch's own error
        per.mean().backward()
    # the scalar path gives the same gradient as the mean of per_image
    x.grad = None
    loss.backward()
    # (its grad_out is fp32's 1/3 widened, not float64's: 3e-8 relative on the seed, fp32 roundings of the perturbed sums after it)
    assert float((x.grad - g_first).abs().max()) <= 1e-5 * float(g_first.abs().max())
    # no gradient for the second operand
    with pytest.raises(NotImplementedError, match="second operand"):
        auto(x, tb.clone().requires_grad_(True))
    # shape errors are the plain path's
    with pytest.raises(ValueError, match="512"):
        auto(torch.zeros(1, 3, 16, 513, device=DEV, requires_grad=True), torch.zeros(1, 3, 16, 513, device=DEV))
    with pytest.raises(ValueError, match="4"):
        auto(torch.zeros(1, 3, 3, 8, device=DEV, requires_grad=True), torch.zeros(1, 3, 3, 8, device=DEV))


def test_parameter_changed_between_forward_and_backward():
    sd = {k: torch.from_numpy(v) for k, v in synth.vgg_loss_state_dict(oracle.weights("default")).items()}
    m = load_vgg_loss(sd, device=DEV, autograd=True)
    a, b, _, _ = pairs_of("noisy", (5, 7, 3))
    x = dev(a).requires_grad_(True)
    loss = m(x, dev(b))
    with torch.no_grad():
        getattr(m.slice, "5").bias.add_(0.5)
    with pytest.raises(RuntimeError, match="slice.5.bias was modified in place"):
        loss.backward()
    # the next call repacks both blobs: its gradient is the changed weights'
    x2 = dev(a).requires_grad_(True)
    m(x2, dev(b)).backward()
    sd2 = dict(sd)
    sd2["slice.5.bias"] = sd["slice.5.bias"] + 0.5
    fresh = load_vgg_loss(sd2, device=DEV, autograd=True)
    x3 = dev(a).requires_grad_(True)
    fresh(x3, dev(b)).backward()
    assert torch.equal(x2.grad, x3.grad)
    assert np.array_equal(m._bwd_blob.cpu().numpy(), fresh._bwd_blob.cpu().numpy())


@pytest.mark.parametrize("wset", ["default", "hot"])
def test_the_trainers_call_composes(wset):
    """fake = tanh(leaf); g_loss = vgg(fake, hr) + 0.001 * other; g_loss.backward(): leaf.grad is the chain rule on the float64
    reference, within the bound."""
    m = loss_of(wset)
    case = (35, 47, 3)
    h, w, n = case
    sd = oracle.weights(wset)
    a, b, _, _ = pairs_of("unrelated", case)
    leaf = (dev(a) * 1.5).requires_grad_(True)
    fake = torch.tanh(leaf)
    other = (fake ** 2).mean()
    vgg = m.per_image(fake, dev(b))
    arena = vgg.grad_fn.saved
    g_loss = vgg.mean().to(torch.float32) + 0.001 * other
    g_loss.backward()
    torch.cuda.synchronize()
    # float64: the same graph on the CPU, the VGG part by backward64 with the device's discontinuities
    fake_np = fake.detach().cpu().numpy()
    pre_a, act_a = ref.forward64(sd, fake_np)
    _, act_b = ref.forward64(sd, b)
    masks, routes = device_discontinuities(arena, n, h, w)
    ref.check_masks(masks, pre_a, "trainer")
    ref.check_routing(routes, act_a, "trainer")
    go = np.full(n, 1.0 / n)
    g64 = ref.backward64(sd, act_a, act_b[6], go, masks, routes)["grad_x"]
    f64 = torch.from_numpy(fake_np).double()
    l64 = torch.from_numpy(np.array(a)).double() * 1.5
    want = (g64 + 0.001 * 2.0 * f64 / f64.numel()) * (1.0 - torch.tanh(l64) ** 2)
    g_aten, m_aten, r_aten = ref.aten_fp32(sd, fake_np, b, go)
    e_aten = ref.rel_err(g_aten["grad_x"], ref.backward64(sd, act_a, act_b[6], go, m_aten, r_aten)["grad_x"])
    e = ref.rel_err(leaf.grad.cpu(), want)
    bound = max(1e-5, 2 * e_aten)
    print(f"trainer {wset}: e {e:.3e}, e_aten {e_aten:.3e}, bound {bound:.3e} (margin {bound / max(e, 1e-300):.1f}x)")
    assert e <= bound


def test_composes_with_the_generator():
    """Through DenoiseGenerator(autograd=True) at 16x16: the parameter gradients of vgg(G(noisy), clean).backward() are, bit for bit,
    those of feeding the same VGG input gradient into G(noisy).backward(gradient=...)."""
    m = loss_of("default")
    g = cid.DenoiseGenerator(autograd=True)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict("default").items()})
    g.to(DEV)
    for p in g.parameters():
        p.requires_grad_(True)
    noisy, clean, _ = synth.make_batch(2, 16, 16, first_index=4321)
    tn, tc = dev(noisy), dev(clean)
    out = g(tn)
    assert out.requires_grad
    m(out, tc).backward()
    first = {k: p.grad.clone() for k, p in g.named_parameters()}
    assert all(bool(torch.isfinite(v).all()) for v in first.values()) and any(float(v.abs().max()) > 0 for v in first.values())
    # the VGG input gradient on its own, then into the generator
    y = g(tn).detach().requires_grad_(True)
    m(y, tc).backward()
    for p in g.parameters():
        p.grad = None
    g(tn).backward(gradient=y.grad)
    for k, p in g.named_parameters():
        assert torch.equal(p.grad, first[k]), k


def test_workspace_hygiene():
    """Results do not depend on what the arena, grad_a or the LDS held; nothing past cid_vgg_saved_bytes or around grad_a is written."""
    m = loss_of("default")
    case = (35, 47, 3)
    h, w, n = case
    a, b, _, _ = pairs_of("noisy", case)
    ta, tb = dev(a), dev(b)
    go = torch.tensor([1.0, -0.5, 2.0], dtype=torch.float64)
    want_out, want_gx, want_arena = cabi(m, ta, tb, go)
    L = _lib.lib()
    need, guard = saved_bytes(n, h, w), 4096
    for fill in (0xFF, 0x00):
        buf = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=DEV)
        buf[:need] = fill
        gbytes = n * 3 * h * w * 4
        gbuf = torch.full((gbytes + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
        gbuf[guard:guard + gbytes] = fill
        gx = gbuf[guard:guard + gbytes].view(torch.float32).view(n, 3, h, w)
        out = torch.empty(n, dtype=torch.float64, device=DEV)
        gd = go.to(DEV)
        assert L.cid_debug_poison_lds(stream()) == 0
        _lib.check_vgg(m._cid, L.cid_vgg_content_loss_saved(m._cid, ta.data_ptr(), 0, tb.data_ptr(), 0, n, h, w, 0, out.data_ptr(), buf.data_ptr(),
                                                            need, stream()))
        assert L.cid_debug_poison_lds(stream()) == 0
        _lib.check_vgg(m._cid, L.cid_vgg_content_backward(m._cid, gd.data_ptr(), gx.data_ptr(), n, h, w, 0, buf.data_ptr(), need, stream()))
        torch.cuda.synchronize()
        assert torch.equal(out, want_out) and torch.equal(gx, want_gx)
        for name in ref.ACTS + ref.GRADS:
            assert torch.equal(view(buf, name, n, h, w), view(want_arena, name, n, h, w)), name
        assert bool((buf[need:] == 0xA5).all())
        assert bool((gbuf[:guard] == 0xA5).all()) and bool((gbuf[guard + gbytes:] == 0xA5).all())


def test_state_errors():
    """A backward before the backward blob is uploaded is CID_ERR_STATE; uploading the forward blob again drops the backward blob."""
    sd = {k: torch.from_numpy(v) for k, v in synth.vgg_loss_state_dict(oracle.weights("default")).items()}
    m = load_vgg_loss(sd, device=DEV, autograd=True)
    L = _lib.lib()
    n, h, w = 1, 8, 8
    x = torch.zeros(n, 3, h, w, device=DEV)
    arena = torch.empty(saved_bytes(n, h, w), dtype=torch.uint8, device=DEV)
    out = torch.empty(n, dtype=torch.float64, device=DEV)
    go = torch.ones(n, dtype=torch.float64, device=DEV)
    gx = torch.empty_like(x)

    def fwd(fa=0):
        return L.cid_vgg_content_loss_saved(m._cid, x.data_ptr(), fa, x.data_ptr(), 0, n, h, w, 0, out.data_ptr(), arena.data_ptr(), arena.numel(), stream())

    def bwd():
        return L.cid_vgg_content_backward(m._cid, go.data_ptr(), gx.data_ptr(), n, h, w, 0, arena.data_ptr(), arena.numel(), stream())

    assert fwd() == 0
    assert fwd(fa=1) == 1                       # CID_ERR_INVALID: a uint8 operand a
    assert bwd() == 4 and b"backward weights" in L.cid_vgg_last_error(m._cid)
    m._pack_backward_weights()
    assert bwd() == 0
    m.pack_weights(force=True)
    assert bwd() == 4
    m._pack_backward_weights()
    assert bwd() == 0
    torch.cuda.synchronize()
    assert float(gx.abs().max()) == 0.0          # identical operands: the seed is exactly zero
