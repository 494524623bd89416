"""The ESRGAN discriminator's backward pass on the GPU: cid_esd_forward_saved, cid_esd_backward, cid_esd_pack_weights_device
(include/cid.h) and ESRGANDiscriminator(autograd=True).  The rule of error, the reference and the shapes are in
tests/esrgan_disc_bwd_oracle.py; its conditions on the reference are asserted in tests/test_esrgan_disc_backward_host.py.

Which shape gives each new kernel two tiles with a partial last one (rows x columns of the tiled map in brackets):
  k_esd_wgrad, items of 4 x 16 output pixels      conv2 [18 x 33] and conv3 [9 x 17] at (1,70,130); conv4 [5 x 17] at (1,66,258)
  k_esd_dgrad conv2, class tiles of 16 x 16        class (0,0) of a1 [18 x 33] at (1,70,130)
  k_esd_dgrad conv3, class tiles of 8 x 16         class (0,0) of a2 [9 x 17] at (1,70,130)
  k_esd_dgrad conv4, class tiles of 4 x 16         class (0,0) of a3 [5 x 17] at (1,66,258); (1,24,264) and (1,264,24) give one direction each
  k_esd_wgrad1, strips of 64 pixels of a1          513 pixels at (2,37,53): nine strips, one pixel in the last
  k_esd_dgrad1, blocks of 256 pixels of a class    class (0,0) of the input, 513 pixels at (2,37,53)
  k_esd_fc_bwd, blocks of 256 features             512 * H4 * W4 is a multiple of 256: it has no partial block; (2,37,53) has 24 blocks
  k_esd_pack, blocks of 256 floats                 the blob of (37,53) ends 64 floats into its last block
A weight-gradient workgroup's item range crosses image boundaries at (5,40,24) for conv4 (five items, two splits) and for conv2,
conv3, conv4 and conv1 in the launch-split test (65,537 items over 64, 33, 33 and 256 splits).  Odd sides give parity classes of
unequal size in every data gradient; (2,1,1) and (4,7,5) have classes with no pixel at all.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import celebrity_image_denoiser_amd as cid
from celebrity_image_denoiser_amd import _lib
from celebrity_image_denoiser_amd.esrgan_disc import ESRGANDiscriminator

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import esrgan_disc_oracle as oracle  # noqa: E402
import esrgan_disc_bwd_oracle as bwd  # noqa: E402
from esrgan_disc_bwd_oracle import PARAMS, Grads, weights  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256          # guard bytes on each side of every output and of the workspace
GUARD_BYTE = 0xA5
ids = lambda s: "x".join(map(str, s))   # noqa: E731


def _module(kind, hw, autograd=False, sd=None):
    m = ESRGANDiscriminator((3, hw[0], hw[1]), autograd=autograd)
    m.load_state_dict(weights(kind, hw) if sd is None else sd, strict=True)
    return m.to(DEV)


def _dims(x):
    if x.dtype == torch.uint8:
        return _lib.CID_FMT_U8_NHWC, x.shape[0], x.shape[1], x.shape[2]
    return _lib.CID_FMT_F32_NCHW, x.shape[0], x.shape[2], x.shape[3]


def _size(fn, n, h, w):
    out = ctypes.c_size_t()
    assert getattr(_lib.lib(), fn)(n, h, w, ctypes.byref(out)) == 0
    return out.value


class _Guarded:
    """`nbytes` of device memory between two runs of guard bytes, filled with `fill` first."""

    def __init__(self, nbytes, fill):
        self.raw = torch.full((nbytes + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.body = self.raw[GUARD:GUARD + nbytes]
        self.body.fill_(fill)
        assert self.body.data_ptr() % 256 == 0

    def intact(self):
        return bool((self.raw[:GUARD] == GUARD_BYTE).all()) and bool((self.raw[GUARD + self.body.numel():] == GUARD_BYTE).all())


def forward_saved(m, x):
    """cid_esd_forward_saved at m's weights -> (logits [N] on the device, the saved buffer)."""
    m.pack_weights()
    fmt, n, h, w = _dims(x)
    saved = torch.empty(_size("cid_esd_saved_bytes", n, h, w), dtype=torch.uint8, device=DEV)
    out = torch.empty(n, dtype=torch.float32, device=DEV)
    m._check(_lib.lib().cid_esd_forward_saved(m._cid, x.data_ptr(), fmt, out.data_ptr(), n, h, w, saved.data_ptr(), saved.numel(), None))
    return out, saved


def saved_stages(saved, shape):
    """a1 ... a4 out of a saved buffer at the documented offsets, as [N,C,H,W] on the CPU."""
    n, h, w = shape
    offs, _ = oracle.expected_workspace(n, h, w)
    out = []
    for off, c in zip(offs, (64, 128, 256, 512)):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        out.append(oracle.c8_to_nchw(saved[off:off + 4 * n * c * h * w].view(torch.float32), n, c, h, w).cpu())
    return out


def backward(m, x, saved, grad_logit, want=PARAMS, want_input=True, fill=0):
    """cid_esd_backward into guarded buffers filled with `fill` -> ({key: grad}, grad_x or None); the guards are checked."""
    fmt, n, h, w = _dims(x)
    sd = m.state_dict()
    g = Grads()
    bufs = {}
    for k in want:
        bufs[k] = _Guarded(4 * sd[k].numel(), fill)
        layer, kind = k.rsplit(".", 1)
        (g.w if kind == "weight" else g.b)[bwd.LAYERS.index(layer)] = bufs[k].body.data_ptr()
    if want_input:
        bufs["input"] = _Guarded(4 * n * 3 * h * w, fill)
        g.input = bufs["input"].body.data_ptr()
    ws = _Guarded(_size("cid_esd_backward_workspace_bytes", n, h, w), fill)
    gl = grad_logit.contiguous()
    m._check(_lib.lib().cid_esd_backward(m._cid, x.data_ptr(), fmt, gl.data_ptr(), n, h, w, saved.data_ptr(), saved.numel(), ctypes.byref(g),
                                         ws.body.data_ptr(), ws.body.numel(), None))
    torch.cuda.synchronize()
    assert ws.intact(), "workspace guard"
    for k, b in bufs.items():
        assert b.intact(), f"guard of {k}"
    grads = {k: bufs[k].body.view(torch.float32).view(sd[k].shape).clone() for k in want}
    gx = bufs["input"].body.view(torch.float32).view(n, 3, h, w).clone() if want_input else None
    return grads, gx


def _cpu(grads):
    return {k: v.cpu() for k, v in grads.items()}


def check_rule(got, got_x, stages, ref, loss, who):
    """The rule of error on one run; -> the worst share of the bound."""
    masks = [a > 0 for a in stages]
    bwd.check_mask_cap(masks, ref["ys64"], who)
    g64, gx64 = bwd.ref_for_masks(ref, loss, masks)
    e = bwd.rel_errors(got, got_x, g64, gx64)
    worst = 0.0
    for k, v in e.items():
        share = v / bwd.bound(ref["e_aten"][k])
        worst = max(worst, share)
        assert np.isfinite(v) and share <= 1.0, (who, k, v, ref["e_aten"][k])
    return worst


# ------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("loss", list(bwd.LOSSES))
@pytest.mark.parametrize("kind", oracle.WSETS)
@pytest.mark.parametrize("shape", bwd.SHAPES, ids=ids)
def test_gradient_parity(shape, kind, loss):
    ref = bwd.reference(kind, shape, loss)
    m = _module(kind, shape[1:])
    x = ref["x"].to(DEV)
    logits, saved = forward_saved(m, x)
    assert float((logits.cpu().double() - ref["logits64"].view(-1)).abs().max()) <= oracle.TOL * max(1.0, float(ref["logits64"].abs().max()))
    gl = bwd.bce_grad(logits, loss)
    grads, gx = backward(m, x, saved, gl)
    worst = check_rule(_cpu(grads), gx.cpu(), saved_stages(saved, shape), ref, loss, f"{shape} {kind} {loss}")
    print(f"{shape} {kind} {loss}: worst share of the bound {worst:.3f}")


def test_saved_forward_is_the_forward_byte_for_byte():
    for shape, kind in (((2, 37, 53), "trained"), ((1, 70, 130), "default")):
        for x in (oracle.case(kind, shape)[1].to(DEV), torch.from_numpy(oracle.case(kind, shape)[0]).to(DEV)):
            m = _module(kind, shape[1:])
            want = m(x)
            total = oracle.expected_workspace(*shape)[1]
            logits, saved = forward_saved(m, x)
            assert torch.equal(logits, want.view(-1))
            assert saved.numel() == total and torch.equal(saved, m._ws[:total])


@pytest.mark.parametrize("kind", oracle.WSETS)
@pytest.mark.parametrize("hw", [(37, 53), (264, 24)], ids=ids)
def test_device_pack_equals_the_host_pack(hw, kind):
    """The synthetic weight sets have no two equal values in a tensor, so a wrong permutation shows."""
    L = _lib.lib()
    h, w = hw
    sd = weights(kind, hw)
    assert all(v.unique().numel() >= min(v.numel(), 64) for v in sd.values())
    m = _module(kind, hw)
    m.pack_weights()
    nbytes = L.cid_esd_packed_weights_bytes(h, w)
    host = np.zeros(nbytes // 4, np.float32)
    assert L.cid_esd_export_packed(m._cid, host.ctypes.data, host.nbytes) == 0
    assert torch.equal(m._blob.cpu().view(torch.float32), torch.from_numpy(host))   # the upload is the export
    params = [p.detach().contiguous() for p in m.parameters()]
    ptrs = (ctypes.c_void_p * 10)(*[p.data_ptr() for p in params])
    blob = _Guarded(nbytes, 0xFF)
    m._check(L.cid_esd_pack_weights_device(m._cid, ptrs, blob.body.data_ptr(), None))
    torch.cuda.synchronize()
    assert blob.intact()
    assert np.array_equal(blob.body.cpu().numpy().view(np.uint32), host.view(np.uint32))
    # the handle now runs on that blob
    x = oracle.images(2, h, w)[1].to(DEV)
    want = _module(kind, hw)(x)
    m._blob = blob.body
    assert torch.equal(m(x), want)


def _one_case(shape=(2, 37, 53), kind="trained", loss="real1"):
    ref = bwd.reference(kind, shape, loss)
    m = _module(kind, shape[1:])
    x = ref["x"].to(DEV)
    logits, saved = forward_saved(m, x)
    return ref, m, x, saved, bwd.bce_grad(logits, loss)


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_subsets_determinism_and_buffer_hygiene():
    ref, m, x, saved, gl = _one_case()
    full, gx = backward(m, x, saved, gl)
    # determinism, and nothing is read before it is written: 0xFF in the workspace and in every output changes no bit
    again, gx2 = backward(m, x, saved, gl, fill=0xFF)
    assert _same(gx, gx2) and all(_same(full[k], again[k]) for k in PARAMS)
    assert all(bool(torch.isfinite(v).all()) for v in again.values()) and bool(torch.isfinite(gx2).all())
    # every single-output call and an input-only call
    for k in PARAMS:
        one, none = backward(m, x, saved, gl, want=(k,), want_input=False, fill=0xFF)
        assert none is None and _same(one[k], full[k]), k
    only, gx3 = backward(m, x, saved, gl, want=(), want_input=True, fill=0xFF)
    assert only == {} and _same(gx3, gx)
    # nothing asked for: no launch, no error
    assert backward(m, x, saved, gl, want=(), want_input=False) == ({}, None)


def test_uint8_input_gives_the_gradients_of_its_fp32_copy():
    shape, kind = (2, 37, 53), "trained"
    u8, xf = oracle.case(kind, shape)[:2]
    m = _module(kind, shape[1:])
    xu, xf = torch.from_numpy(u8).to(DEV), xf.to(DEV)
    lu, su = forward_saved(m, xu)
    lf, sf = forward_saved(m, xf)
    assert torch.equal(lu, lf) and torch.equal(su, sf)
    gl = bwd.bce_grad(lf, "fake0")
    gu, none = backward(m, xu, su, gl, want_input=False)
    gf, _ = backward(m, xf, sf, gl)
    assert none is None and all(_same(gu[k], gf[k]) for k in PARAMS)
    g = Grads()
    g.input = xf.data_ptr()
    assert _lib.lib().cid_esd_backward(m._cid, xu.data_ptr(), 1, gl.data_ptr(), 2, 37, 53, su.data_ptr(), su.numel(), ctypes.byref(g),
                                       su.data_ptr(), su.numel(), None) == 1   # CID_ERR_INVALID, before any launch


def test_batch_independence_of_the_input_gradient():
    n, h, w = 5, 37, 53
    x = oracle.images(n, h, w, first_index=3)[1].to(DEV)
    m = _module("trained", (h, w))
    gl = torch.tensor([0.3, -0.2, 0.05, 0.3, -1.0], device=DEV)
    _, saved = forward_saved(m, x)
    _, gx = backward(m, x, saved, gl, want=())
    for i in range(n):
        xi = x[i:i + 1].contiguous()
        _, si = forward_saved(m, xi)
        _, gi = backward(m, xi, si, gl[i:i + 1], want=())
        assert _same(gi, gx[i:i + 1]), i
    # at another position of another batch
    perm = [3, 0, 4, 1]
    xp = x[perm].contiguous()
    _, sp = forward_saved(m, xp)
    _, gp = backward(m, xp, sp, gl[perm].contiguous(), want=())
    assert _same(gp, gx[perm])


def test_zero_gradient_gives_zeros():
    ref, m, x, saved, gl = _one_case()
    grads, gx = backward(m, x, saved, torch.zeros_like(gl), fill=0xFF)
    for k, v in list(grads.items()) + [("input", gx)]:
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) == 0.0, k


def test_launch_split_above_65535_images():
    """65,537 images of 1x1: the seam images' input gradients equal the image run alone; the parameter gradients against float64."""
    n = 65537
    u8 = (np.arange(n * 3, dtype=np.int64) * 2654435761 % 251).astype(np.uint8).reshape(n, 1, 1, 3)
    xf = (torch.from_numpy(u8).permute(0, 3, 1, 2).to(torch.float32) / 255.0).contiguous()
    x = xf.to(DEV)
    m = _module("trained", (1, 1))
    logits, saved = forward_saved(m, x)
    gl = bwd.bce_grad(logits, "real1") * n   # per-image values of ordinary size: the mean's 1/n taken out
    grads, gx = backward(m, x, saved, gl)
    for i in (0, 65534, 65535, 65536):
        xi = x[i:i + 1].contiguous()
        _, si = forward_saved(m, xi)
        _, gi = backward(m, xi, si, gl[i:i + 1].contiguous(), want=())
        assert _same(gi, gx[i:i + 1]), i
        assert float(gi.abs().max()) > 0
    # float64 with the kernels' masks, on the same grad_logit; ATen fp32 on the CPU measures the reference's own error
    sd = weights("trained", (1, 1))
    stages = saved_stages(saved, (n, 1, 1))
    masks = [a > 0 for a in stages]
    glc = gl.cpu()

    def run(dtype, mk):
        # at 1x1 only the centre tap meets the image: each layer is a matrix product with W[:, :, 1, 1], every other tap's gradient 0
        P = {k: sd[k].to(dtype).clone().requires_grad_(True) for k in PARAMS}
        y, ys = xf.to(dtype).view(n, 3), []
        for l, name in enumerate(bwd.LAYERS[:4]):
            y = y @ P[name + ".weight"][:, :, 1, 1].t() + P[name + ".bias"]
            ys.append(y.detach())
            y = bwd._MaskedLeaky.apply(y, mk[l].reshape(y.shape) if mk is not None else y.detach() > 0)
        out = y @ P["fc.weight"].t() + P["fc.bias"]
        out.backward(glc.to(dtype).view(n, 1))
        return {k: P[k].grad for k in PARAMS}, ys

    g64, ys64 = run(torch.float64, masks)
    bwd.check_mask_cap(masks, ys64, "hip")
    g32, ys32 = run(torch.float32, None)
    m32 = [y > 0 for y in ys32]
    ga = g64 if all(torch.equal(a.reshape(b.shape), b) for a, b in zip(masks, m32)) else run(torch.float64, m32)[0]
    e_aten = bwd.rel_errors(g32, None, ga, None)
    e_hip = bwd.rel_errors(_cpu(grads), None, g64, None)
    for k in PARAMS:
        print(f"  {k}: e_hip {e_hip[k]:.2e} e_aten {e_aten[k]:.2e}")
        assert e_hip[k] <= bwd.bound(e_aten[k]), (k, e_hip[k], e_aten[k])


# ------------------------------------------------------------------------------------------------------------- the module
def _loss(out, target):
    return nn.BCEWithLogitsLoss()(out, torch.full_like(out, target))


def test_module_gives_the_cabi_bits_and_grad_accumulates():
    shape, kind = (2, 37, 53), "trained"
    ref = bwd.reference(kind, shape, "real1")
    x = ref["x"].to(DEV)
    m = _module(kind, shape[1:], autograd=True)
    xr = x.clone().requires_grad_(True)
    out = m(xr)
    assert out.shape == (2, 1) and out.grad_fn is not None and out.dtype == torch.float32
    _loss(out, 1.0).backward()
    plain = _module(kind, shape[1:])
    logits, saved = forward_saved(plain, x)
    assert torch.equal(out.detach().view(-1), logits)
    want, wx = backward(plain, x, saved, bwd.bce_grad(logits, "real1"))
    assert _same(xr.grad, wx)
    for k, p in m.named_parameters():
        assert _same(p.grad, want[k]), k
    # the trainer's two D(.) calls before one backward: .grad accumulates over both
    m.zero_grad()
    x2 = oracle.images(2, 37, 53, first_index=11)[1].to(DEV)
    (0.5 * (_loss(m(x), 1.0) + _loss(m(x2), 0.0))).backward()
    l1, s1 = forward_saved(plain, x)
    l2, s2 = forward_saved(plain, x2)
    g1, _ = backward(plain, x, s1, 0.5 * bwd.bce_grad(l1, "real1"), want_input=False)
    g2, _ = backward(plain, x2, s2, 0.5 * bwd.bce_grad(l2, "fake0"), want_input=False)
    for k, p in m.named_parameters():
        assert _same(p.grad, g1[k] + g2[k]) or _same(p.grad, g2[k] + g1[k]), k
    # once differentiable
    out = m(xr)
    (gx,) = torch.autograd.grad(out.sum(), xr, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


def test_frozen_parameters_inplace_changes_and_the_default_module():
    shape, kind = (2, 37, 53), "trained"
    x = oracle.case(kind, shape)[1].to(DEV)
    m = _module(kind, shape[1:], autograd=True)
    for k, p in m.named_parameters():
        p.requires_grad_(k in ("conv3.weight", "fc.bias"))
    _loss(m(x), 0.0).backward()
    plain = _module(kind, shape[1:])
    logits, saved = forward_saved(plain, x)
    want, _ = backward(plain, x, saved, bwd.bce_grad(logits, "fake0"), want=("conv3.weight", "fc.bias"), want_input=False)
    for k, p in m.named_parameters():
        assert (p.grad is None) if k not in want else _same(p.grad, want[k]), k
    # every parameter frozen, only the input: the generator's adversarial half
    for p in m.parameters():
        p.requires_grad_(False)
    xr = x.clone().requires_grad_(True)
    _loss(m(xr), 1.0).backward()
    assert xr.grad is not None and all(p.grad is None or k in want for k, p in m.named_parameters())
    # nothing requires grad, or grad mode off: no history
    assert m(x).grad_fn is None
    for p in m.parameters():
        p.requires_grad_(True)
    with torch.no_grad():
        assert m(x).grad_fn is None
    # an in-place change between a forward and its backward
    out = m(x)
    with torch.no_grad():
        m.conv2.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="conv2.bias was modified in place"):
        _loss(out, 1.0).backward()
    # the default module: no grad_fn, and backward raises torch's own error
    out = plain(x)
    assert out.grad_fn is None and not out.requires_grad
    with pytest.raises(RuntimeError, match="does not require grad"):
        _loss(out, 1.0).backward()


def test_module_runs_on_a_non_default_stream():
    shape, kind = (2, 37, 53), "trained"
    x = oracle.case(kind, shape)[1].to(DEV)
    m = _module(kind, shape[1:], autograd=True)
    _loss(m(x), 1.0).backward()
    want = {k: p.grad.clone() for k, p in m.named_parameters()}
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        m2 = _module(kind, shape[1:], autograd=True)
        _loss(m2(x), 1.0).backward()
    s.synchronize()
    for k, p in m2.named_parameters():
        assert _same(p.grad, want[k]), k


class _TinyG(nn.Module):
    """A small differentiable stand-in for the generator: one 3x3 convolution and a sigmoid, output in [0,1]."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 3, 3, padding=1)

    def forward(self, x):
        return torch.sigmoid(self.conv(x))


@pytest.mark.parametrize("opt", ["torch", "cid"])
def test_the_trainers_two_steps(opt):
    """esrgan_train.py:101-121 with D on the HIP kernels, against the float64 stock run under the rule."""
    shape, kind = (2, 37, 53), "trained"
    n, h, w = shape
    sd = weights(kind, (h, w))
    clean = oracle.images(n, h, w, first_index=5)[1]
    noisy = oracle.case(kind, shape)[1]
    torch.manual_seed(3)
    G = _TinyG()
    g_sd = {k: v.clone() for k, v in G.state_dict().items()}
    G = G.to(DEV)
    D = _module(kind, (h, w), autograd=True)
    d_opt = (torch.optim.Adam if opt == "torch" else cid.Adam)(D.parameters(), lr=1e-4, betas=(0.9, 0.999))
    bce, mse = nn.BCEWithLogitsLoss(), nn.MSELoss()
    cl, no = clean.to(DEV), noisy.to(DEV)

    denoised = G(no)
    real_out, fake_out = D(cl), D(denoised.detach())
    d_loss = 0.5 * (bce(real_out, torch.ones_like(real_out)) + bce(fake_out, torch.zeros_like(fake_out)))
    d_opt.zero_grad()
    d_loss.backward()
    d_grads = {k: p.grad.detach().cpu().clone() for k, p in D.named_parameters()}
    d_opt.step()
    stepped = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
    denoised.retain_grad()
    fake_out_g = D(denoised)
    # the repack happened: this forward is a fresh module's at the stepped weights
    assert torch.equal(fake_out_g.detach(), _module(kind, (h, w), sd=stepped)(denoised.detach()))
    assert any(not torch.equal(stepped[k], sd[k]) for k in sd)
    g_loss = mse(denoised, cl) + 1e-3 * bce(fake_out_g, torch.ones_like(fake_out_g))
    G.zero_grad()
    g_loss.backward()
    den_grad = denoised.grad.detach().cpu()

    # float64 stock run of the same two steps (D's step taken from the device: `stepped`)
    G64 = _TinyG().double()
    G64.load_state_dict({k: v.double() for k, v in g_sd.items()})
    den64 = G64(noisy.double())
    den32 = denoised.detach().cpu()
    assert float((den32.double() - den64.detach()).abs().max()) <= 1e-6

    def run(dtype, state, xs, targets, scale, pixel=None, masks=None):
        """Gradients of scale * sum_i BCE(D(xs[i]), targets[i]) (+ MSE(xs[-1], pixel)) at `state`; masks per call, or None for the
        run's own."""
        P = {k: state[k].to(dtype).clone().requires_grad_(True) for k in PARAMS}
        leaves, ys, total = [], [], 0
        for j, (xi, t) in enumerate(zip(xs, targets)):
            y = xi.to(dtype).clone().requires_grad_(True)
            leaves.append(y)
            ys.append([])
            for l, name in enumerate(bwd.LAYERS[:4]):
                y = torch.nn.functional.conv2d(y, P[name + ".weight"], P[name + ".bias"], stride=2, padding=1)
                ys[j].append(y.detach())
                y = bwd._MaskedLeaky.apply(y, masks[j][l] if masks is not None else y.detach() > 0)
            out = y.reshape(n, -1) @ P["fc.weight"].t() + P["fc.bias"]
            total = total + scale * bce(out, torch.full_like(out, t))
        if pixel is not None:
            total = total + mse(leaves[-1], pixel.to(dtype))
        total.backward()
        return {k: P[k].grad for k in PARAMS}, leaves[-1].grad, ys

    def check(state, xs, targets, scale, pixel, got, got_x, who):
        # the kernels' masks: a_l > 0 of the forward at `state` (the plain forward's workspace holds the saved forward's bytes)
        plain = _module(kind, (h, w), sd=state)
        hip_masks = []
        for xi in xs:
            plain(xi.to(DEV))
            hip_masks.append([a > 0 for a in saved_stages(plain._ws, shape)])
        g64, x64, ys64 = run(torch.float64, state, xs, targets, scale, pixel, hip_masks)
        g32, x32, ys32 = run(torch.float32, state, xs, targets, scale, pixel)
        aten_masks = [[y > 0 for y in ys] for ys in ys32]
        for j in range(len(xs)):
            bwd.check_mask_cap(hip_masks[j], ys64[j], "hip")
            bwd.check_mask_cap(aten_masks[j], ys64[j], "ATen")
        same = all(torch.equal(a, b) for ma, mb in zip(aten_masks, hip_masks) for a, b in zip(ma, mb))
        ga, xa = (g64, x64) if same else run(torch.float64, state, xs, targets, scale, pixel, aten_masks)[:2]
        e_aten = bwd.rel_errors(g32, x32, ga, xa)
        e_hip = bwd.rel_errors(got, got_x, g64, x64)
        for k, v in e_hip.items():
            print(f"  {who} {k}: e_hip {v:.2e} e_aten {e_aten[k]:.2e}")
            assert v <= bwd.bound(e_aten[k]), (who, k, v, e_aten[k])

    check(sd, [clean, den32], [1.0, 0.0], 0.5, None, d_grads, None, "d step")
    # the generator step: the gradient of g_loss with respect to denoised, through D at the stepped weights
    check(stepped, [den32], [1.0], 1e-3, clean, {}, den_grad, "g step")
