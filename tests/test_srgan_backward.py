"""The backward pass of the SRGAN generator in train mode on the GPU: cid_sr_forward_saved / cid_sr_backward / cid_sr_saved_masks
(include/cid.h) and SRGANGenerator(batch_stats=True, autograd=True).

Reference and rule of error are those of tests/srgan_backward_ref.py (held to the stock layers and checked for conditioning by
test_srgan_backward_host.py): float64 autograd on the CPU that takes the 1 + 5 + stages PReLU masks from the fp32 run it is compared
with (capped), e(T) = max|g - g64| / D(T), and the bound e_hip(T) <= max(1e-5, 2 * e_aten(T)) with e_aten measured on the same case.
The forward's output and running buffers are bit-identical to cid_sr_forward_train.

Cases: srgan_train_oracle.PARITY_CASES on both weight sets, and srgan_backward_ref.SPLIT_CASE (66 x 8 x 16 at scale 2), which is
there for the weight gradients' item loops: on the six cases no weight-gradient launch has more items than workgroups; on this one
all four do, unevenly, with ranges that straddle two images (the reasons and the arithmetic are with SPLIT_CASE and in
test_srgan_backward_host.py).  The backward's tiles are 16 x 16 (data gradients, final's included),
4 x 16 (the 3x3 weight gradients and final's), 32-pixel row segments (the head's weight gradient) and 512-pixel strips (sums);
13 x 18 at scale 4 (52 x 72 at the output) crosses the first two in both directions at every size they run at, 20 x 36 and 17 x 33 the
32-pixel segment, 2 x 17 x 33 and 52 x 72 the strip, so no shape is added for those.
Every call here has guard regions after the saved buffer, the workspace and each gradient tensor, and a NaN-filled workspace and
saved buffer.

Measured on an MI355X over every check of this file: at most 4 mask flips in a check, all inside the cap; largest e_hip 5.7e-6
(res_blocks.i.4.bias; ATen fp32 5.3e-6 at its worst on that kind), convolution weights 3.6e-6, slopes 1.4e-7; worst share of the
bound 0.57, and no tensor needs the 2 * e_aten branch
(DESIGN.md, section 24)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from celebrity_image_denoiser_amd import _lib, synth
from celebrity_image_denoiser_amd.discriminator import named_bn_args
from celebrity_image_denoiser_amd.srgan import _GradsArg, _set_grad, load_srgan

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import srgan_backward_ref as ref  # noqa: E402
import srgan_train_oracle as oracle  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256          # bytes after the saved buffer and the workspace, floats' worth after each gradient tensor
SENTINEL = 0x5A


def model_of(sd, scale, autograd=True):
    return load_srgan(sd, scale_factor=scale, device=DEV, strict=True, batch_stats=True, autograd=autograd).train()


def running(m):
    sd = m.state_dict()
    return {k: sd[k].clone() for k in sd if "running" in k or "num_batches" in k}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def cabi(m, x, G, raw=False, want=None, masks=True):
    """One cid_sr_forward_saved + cid_sr_saved_masks + cid_sr_backward on module m's handle and BatchNorm tensors, NaN-filled saved
    buffer and workspace, guards checked.  x: fp32 [N,3,H,W] or uint8 [N,H,W,3] on the device.
    -> (out, {name: gradient} for the names in `want` (default: all), the masks as bool tensors on the CPU)"""
    L = _lib.lib()
    u8 = x.dtype == torch.uint8
    n, h, w = (x.shape[0], x.shape[1], x.shape[2]) if u8 else (x.shape[0], x.shape[2], x.shape[3])
    fmt = _lib.CID_FMT_U8_NHWC if u8 else _lib.CID_FMT_F32_NCHW
    s = m.scale_factor
    stages = m.num_upsamples
    flags = _lib.CID_SR_RAW if raw else 0
    m.pack_weights()
    need = ctypes.c_size_t()

    def buffer(sizer):
        assert sizer(n, h, w, s, ctypes.byref(need)) == 0
        t = torch.full((need.value + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
        t[:need.value].view(torch.float32).fill_(float("nan"))
        return t, need.value

    saved, nsaved = buffer(L.cid_sr_saved_bytes)
    fws, nfws = buffer(L.cid_sr_train_workspace_bytes)
    bws, nbws = buffer(L.cid_sr_backward_workspace_bytes)
    out = torch.empty((n, 3, s * h, s * w), dtype=torch.float32, device=DEV)
    bn = named_bn_args([(name, layer) for name, layer, _ in m._batchnorms()], torch.device(DEV))
    x = x.contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    m._check(L.cid_sr_forward_saved(m._cid, x.data_ptr(), fmt, out.data_ptr(), n, h, w, flags, bn, saved.data_ptr(), nsaved, fws.data_ptr(),
                                    nfws, stream))
    got_masks = []
    if masks:
        sizes = [(n, 64, h, w)] * 6 + [(n, 64, h << (k + 1), w << (k + 1)) for k in range(stages)]
        mt = [torch.full(sz, 7, dtype=torch.uint8, device=DEV) for sz in sizes]
        arr = (ctypes.c_void_p * len(mt))(*[t.data_ptr() for t in mt])
        assert L.cid_sr_saved_masks(saved.data_ptr(), nsaved, n, h, w, s, arr, stream) == 0
        got_masks = [t.cpu() for t in mt]
        assert all(bool(((t == 0) | (t == 1)).all()) for t in got_masks)
        got_masks = [t.bool() for t in got_masks]
    names = [k for k, _ in m.named_parameters()]
    want = names if want is None else want
    g = _GradsArg()
    store = {}
    for k, p in m.named_parameters():
        if k in want:
            store[k] = torch.full((p.numel() + GUARD,), -77.0, dtype=torch.float32, device=DEV)
            _set_grad(g, k, store[k].data_ptr())
    m._check(L.cid_sr_backward(m._cid, x.data_ptr(), fmt, G.data_ptr(), n, h, w, flags, bn, saved.data_ptr(), nsaved, ctypes.byref(g),
                               bws.data_ptr(), nbws, stream))
    torch.cuda.synchronize()
    for t, used in ((saved, nsaved), (fws, nfws), (bws, nbws)):
        assert bool((t[used:] == SENTINEL).all()), "guard after a buffer"
    grads = {}
    for k, p in m.named_parameters():
        if k in want:
            assert bool((store[k][p.numel():] == -77.0).all()), ("guard after", k)
            grads[k] = store[k][:p.numel()].reshape(p.shape).clone()
            assert bool(torch.isfinite(grads[k]).all()), k
    return out, grads, got_masks


def check_against_float64(sd, x32, G, grads, masks, e_aten, raw=False, who="HIP"):
    """The rule of error: float64 with the device's masks (capped); e_hip(T) <= max(1e-5, 2 * e_aten(T)).  Prints every figure first."""
    g64, pre64, _, book = ref.ref_backward(sd, x32, G.cpu(), torch.float64, masks=masks, raw=raw)
    flips = ref.check_mask_cap(masks, pre64, who)
    errs = ref.rel_errors({k: v.cpu() for k, v in grads.items()}, g64, book)
    bad = []
    for k, e in errs.items():
        bound = max(ref.TOL, 2 * e_aten.get(k, 0.0))
        print(f"    {k:28s} e_hip {e:.2e}  e_aten {e_aten.get(k, float('nan')):.2e}  bound {bound:.2e}")
        if not e <= bound:
            bad.append((k, e, bound))
    print(f"  {who}: {flips} mask flips, worst share of the bound {max(e / max(ref.TOL, 2 * e_aten.get(k, 0.0)) for k, e in errs.items()):.3f}")
    assert not bad, bad


# --------------------------------------------------------------------------------------------------------------- parity, C ABI
@pytest.mark.parametrize("case", ref.CASES, ids=oracle.case_id)
@pytest.mark.parametrize("wset", ["default", "hot"])
def test_gradient_parity_through_the_c_abi(wset, case):
    n, h, w, scale = case
    sd = synth.make_srgan_state_dict(wset, scale)
    x32 = ref.case_input(case)
    x, G = torch.from_numpy(x32).to(DEV), ref.grad_out(n, scale, h, w).to(DEV)
    e_aten, _ = ref.aten_errors(wset, case)
    plain = model_of(sd, scale, autograd=False)
    with torch.no_grad():
        want_out = plain(x)
    m = model_of(sd, scale)
    out, grads, masks = cabi(m, x, G)
    assert torch.equal(_bits(out), _bits(want_out))                      # bit-identical to cid_sr_forward_train
    got, want = running(m), running(plain)
    assert all(torch.equal(_bits(got[k]), _bits(want[k])) for k in want) and len(want) == 30
    assert list(grads) == ref.param_names(scale.bit_length() - 1)
    check_against_float64(sd, x32, G, grads, masks, e_aten)


def test_repeatability_and_raw():
    """Two calls give identical bits (NaN-filled buffers both times); with CID_SR_RAW the gradient belongs to the sums before tanh."""
    case, wset = (3, 8, 12, 2), "hot"
    n, h, w, scale = case
    sd = synth.make_srgan_state_dict(wset, scale)
    x32 = oracle.case_input(case)
    x, G = torch.from_numpy(x32).to(DEV), ref.grad_out(n, scale, h, w).to(DEV)
    m = model_of(sd, scale)
    out1, g1, _ = cabi(m, x, G, masks=False)
    out2, g2, _ = cabi(m, x, G, masks=False)
    assert torch.equal(_bits(out1), _bits(out2)) and all(torch.equal(_bits(g1[k]), _bits(g2[k])) for k in g1)
    e_aten, _ = ref.aten_errors(wset, case, raw=True)
    pre, graw, masks = cabi(m, x, G, raw=True)
    assert float((torch.tanh(pre) - out1).abs().max()) <= 1e-6 and float(pre.abs().max()) > 1.0
    check_against_float64(sd, x32, G, graw, masks, e_aten, raw=True)


@pytest.mark.parametrize("slope", [0.0, -0.5])
def test_slopes_zero_and_negative(slope):
    """Every PReLU slope (head, blocks, stage) set by hand: with a <= 0 the sign of an activated value says nothing about its
    pre-activation (a = 0 even erases it), so masks and slope gradients must come from what the forward saw."""
    case = (3, 8, 12, 2)
    n, h, w, scale = case
    sd = dict(synth.make_srgan_state_dict("default", scale))
    for k in ref.slope_names(1):
        sd[k] = np.full_like(sd[k], slope)
    x32 = oracle.case_input(case)
    x, G = torch.from_numpy(x32).to(DEV), ref.grad_out(n, scale, h, w).to(DEV)
    e_aten, _ = ref.aten_errors("default", case, sd=sd, tag=slope)
    assert max(e_aten.values()) <= ref.TOL                                 # the reference is well-conditioned here as well
    m = model_of(sd, scale)
    _, grads, masks = cabi(m, x, G)
    _, pre64, _, _ = ref.ref_backward(sd, x32, G.cpu(), torch.float64)
    for i, (mk, v) in enumerate(zip(masks, pre64)):
        assert 0.05 < float(mk.float().mean()) < 0.95, i                   # both branches are taken
    check_against_float64(sd, x32, G, grads, masks, e_aten)
    assert all(float(grads[k].abs().max()) > 0 for k in ref.slope_names(1))


# --------------------------------------------------------------------------------------------------------------- the module
def module_grads(m, x, G, raw=False, out_dtype=None):
    m.zero_grad(set_to_none=True)
    out = m(x, raw=raw) if out_dtype is None else m(x, out_dtype=out_dtype, raw=raw)
    assert out.requires_grad and out.grad_fn is not None
    (out * G).sum().backward()
    return out.detach(), {k: p.grad for k, p in m.named_parameters()}


@pytest.mark.parametrize("raw", [False, True], ids=["tanh", "raw"])
def test_module_backward_is_the_c_abi(raw):
    """loss.backward() through the module gives the bits of cid_sr_backward called directly (whose parity the tests above hold)."""
    case = (1, 13, 18, 4)
    n, h, w, scale = case
    sd = synth.make_srgan_state_dict("hot", scale)
    x, G = torch.from_numpy(oracle.case_input(case)).to(DEV), ref.grad_out(n, scale, h, w).to(DEV)
    m = model_of(sd, scale)
    want_out, want, _ = cabi(model_of(sd, scale), x, G, raw=raw, masks=False)
    xin = x.clone().requires_grad_(True)
    out, got = module_grads(m, xin, G, raw=raw)
    assert xin.grad is None                                               # lr_img is data
    assert torch.equal(_bits(out), _bits(want_out))
    for k in want:
        assert got[k] is not None and got[k].shape == want[k].shape and torch.equal(_bits(got[k]), _bits(want[k])), k
    # the saved buffer is released by the backward; a second forward / backward accumulates into .grad
    out2 = m(x, raw=raw)
    (out2 * G).sum().backward()
    k = "mid.weight"
    assert torch.equal(m.get_parameter(k).grad, want[k] + want[k])
    # eval mode, no_grad and a uint8 output carry no history
    with torch.no_grad():
        assert m(x).grad_fn is None
    assert m(x, out_dtype=torch.uint8).grad_fn is None
    assert m.eval()(x).grad_fn is None


def test_uint8_input_and_frozen_parameters():
    case = (3, 8, 12, 2)
    n, h, w, scale = case
    sd = synth.make_srgan_state_dict("default", scale)
    u8 = synth.srgan_inputs_u8(n, h, w, 2330)
    x32 = synth.normalize_u8(u8)
    G = ref.grad_out(n, scale, h, w).to(DEV)
    m = model_of(sd, scale)
    out, got = module_grads(m, torch.from_numpy(u8).to(DEV), G, out_dtype=torch.float32)
    g32, pre32, _, _ = ref.ref_backward(sd, x32, G.cpu(), torch.float32)
    g64, pre64, _, book = ref.ref_backward(sd, x32, G.cpu(), torch.float64, masks=[v > 0 for v in pre32])
    e_aten = ref.rel_errors(g32, g64, book)
    _, _, masks = cabi(model_of(sd, scale), torch.from_numpy(u8).to(DEV), G, want=[])
    check_against_float64(sd, x32, G, got, masks, e_aten)
    # frozen parameters get no gradient; the others keep their bits
    frozen = ("initial.0.weight", "res_blocks.2.1.weight", "res_blocks.2.2.weight", "upscale.0.bias", "final.weight")
    f = model_of(sd, scale)
    for k in frozen:
        f.get_parameter(k).requires_grad_(False)
    _, part = module_grads(f, torch.from_numpy(u8).to(DEV), G, out_dtype=torch.float32)
    for k in got:
        if k in frozen:
            assert part[k] is None, k
        else:
            assert torch.equal(_bits(part[k]), _bits(got[k])), k


def test_in_place_change_between_forward_and_backward_raises():
    sd = synth.make_srgan_state_dict("default", 2)
    m = model_of(sd, 2)
    x = torch.from_numpy(oracle.case_input((1, 5, 7, 2))).to(DEV)
    out = m(x)
    with torch.no_grad():
        m.mid.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="parameter mid.bias was modified in place"):
        out.sum().backward()


def test_a_second_backward_through_one_forward_raises():
    """The saved buffer belongs to one backward; retain_graph=True does not keep it."""
    m = model_of(synth.make_srgan_state_dict("default", 2), 2)
    out = m(torch.from_numpy(oracle.case_input((1, 5, 7, 2))).to(DEV))
    out.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="saved activations were released by its first backward"):
        out.sum().backward()


def test_an_optimizer_step_reaches_the_next_forwards():
    """Adam step, train forward at the new weights, then .eval(): the eval forward folds the UPDATED running statistics and equals a
    freshly loaded module's, bit for bit."""
    sd = synth.make_srgan_state_dict("default", 2)
    m = model_of(sd, 2)
    x = torch.from_numpy(oracle.case_input((2, 16, 16, 1))).to(DEV)      # the input does not depend on the case's scale
    G = ref.grad_out(2, 2, 16, 16).to(DEV)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    (m(x) * G).sum().backward()
    opt.step()
    out = m(x)
    fresh = model_of({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, 2, autograd=False)
    assert torch.equal(_bits(m.eval()(x)), _bits(fresh.eval()(x)))
    assert not torch.equal(out.detach(), m(x))                            # train and eval differ, the fold was not reused


@pytest.mark.parametrize("scale", [1, 2, 4, 8])
@pytest.mark.parametrize("wset", ["default", "hot"])
def test_device_pack_equals_the_host_pack(wset, scale):
    """cid_sr_pack_weights_device against cid_sr_upload_weights: byte equality of the whole blob (a NaN-filled blob before the
    call, so every float is written), at the loaded state and again after a train forward has moved the running statistics."""
    sd = synth.make_srgan_state_dict(wset, scale)
    want = load_srgan(sd, scale_factor=scale, device=DEV, strict=True).pack_weights()
    m = model_of(sd, scale)
    m._blob.fill_(0xFF)
    got = m.pack_weights()
    assert got.data_ptr() == m._blob.data_ptr() and got.numel() == want.numel()
    assert torch.equal(got, want)
    with torch.no_grad():
        m(torch.from_numpy(oracle.case_input((1, 5, 7, 2))).to(DEV))
    state = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    assert not np.array_equal(state["res_blocks.3.4.running_var"], sd["res_blocks.3.4.running_var"])
    ptr = m._blob.data_ptr()
    m._blob.fill_(0xFF)
    got = m.pack_weights()
    assert got.data_ptr() == ptr                                          # one blob that stays in place
    assert torch.equal(got, load_srgan(state, scale_factor=scale, device=DEV, strict=True).pack_weights())


def test_composition_with_discriminator_and_vgg_loss():
    """The generator step of the SRGAN trainer on one small batch: the parameter gradients of vgg_loss(fake, hr) + 0.001 *
    BCE(D(fake), 1) through autograd are, bit for bit, cid_sr_backward called with the grad_out that D and VGG produce for `fake`
    taken as a leaf.  Plumbing only."""
    import lpips_vgg_oracle
    import srgan_disc_oracle
    from celebrity_image_denoiser_amd.lpips import load_vgg_loss
    from celebrity_image_denoiser_amd.srgan_disc import SRGANDiscriminator

    case = (2, 16, 16, 4)
    n, h, w, scale = case
    sd = synth.make_srgan_state_dict("default", scale)
    x = torch.from_numpy(synth.normalize_u8(synth.srgan_inputs_u8(n, h, w, 2400))).to(DEV)
    hr = torch.from_numpy(synth.normalize_u8(synth.srgan_inputs_u8(n, scale * h, scale * w, 2410))).to(DEV)
    D = SRGANDiscriminator(autograd=True)
    D.load_state_dict(srgan_disc_oracle.weights("default"), strict=True)
    D.to(DEV).train()
    vgg = load_vgg_loss({k: torch.from_numpy(v) for k, v in synth.vgg_loss_state_dict(lpips_vgg_oracle.weights("default")).items()},
                        device=DEV, autograd=True)
    bce = nn.BCELoss()

    def g_loss(fake):
        pred = D(fake)
        return vgg(fake, hr) + 0.001 * bce(pred, torch.ones_like(pred))

    m = model_of(sd, scale)
    d_buffers = {k: v.clone() for k, v in D.state_dict().items()}
    g_loss(m(x)).backward()
    got = {k: p.grad.clone() for k, p in m.named_parameters()}
    # the same step with fake as a leaf (D's train-mode statistics do not read its running buffers; restore them all the same)
    D.load_state_dict(d_buffers)
    D.zero_grad(set_to_none=True)
    with torch.no_grad():
        fake = model_of(sd, scale, autograd=False)(x)
    leaf = fake.clone().requires_grad_(True)
    g_loss(leaf).backward()
    _, want, _ = cabi(model_of(sd, scale), x, leaf.grad.contiguous(), masks=False)
    for k in want:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k
