"""The backward pass of the ESRGAN generator in train mode on the GPU: cid_esr_forward_saved / cid_esr_backward / cid_esr_saved_masks /
cid_esr_pack_weights_device (include/cid.h) and ESRGANGenerator(batch_stats=True, autograd=True).

Reference and rule of error are those of tests/esrgan_backward_ref.py (held to the stock layers and checked for conditioning by
test_esrgan_backward_host.py): float64 autograd on the CPU that takes the 1 + R PReLU masks from the fp32 run it is compared with
(capped), e(T) = max|g - g64| / D(T), and the bound e_hip(T) <= max(1e-5, 2 * e_aten(T)) with e_aten measured on the same case.
The forward's output and running buffers are bit-identical to cid_esr_forward_train.

Cases (esrgan_backward_ref.CASES): esrgan_train_oracle.GPU_PARITY (the six shapes at R = 8, SMALL_CASES at R = 1, 2, 16), SMALL_CASES
at R = 0, and SPLIT_CASE (66 x 16 x 32 at R = 8), which is there for the weight gradients' item loops: on the six shapes no
weight-gradient launch has more items than workgroups; on this one all three do, unevenly, with ranges that straddle two images (the
arithmetic is in test_esrgan_backward_host.py).  The backward's tiles are 16 x 16 (data gradients, final's included), 4 x 16 (the 3x3
weight gradients and final's), 32-pixel row segments (the head's weight gradient) and 512-pixel strips (sums); 13 x 18 and 20 x 36
cross the first two in both directions, 20 x 36 and 17 x 33 the 32-pixel segment, 2 x 17 x 33 and 20 x 36 the strip.
Every C-ABI call here has guard regions after the saved buffer, the workspaces and each gradient tensor, and NaN-filled buffers.

Measured on an MI355X over every check of this file: at most 5 mask flips in a check (the split case; ATen fp32 has 7 there), all
inside the cap; largest e_hip 4.6e-6 (residuals.i.block.0.weight and .bias on the split case; ATen fp32 4.5e-6 and 5.6e-6 at its
worst on those kinds, 6.0e-6 on final.bias), BatchNorm weights and biases 4.0e-6, the head 3.5e-6, final 1.3e-6, slopes 1.1e-7;
worst share of the bound 0.46, and no tensor needs the 2 * e_aten branch."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from celebrity_image_denoiser_amd import _lib, synth
from celebrity_image_denoiser_amd.esrgan import _GradsArg, _set_grad, load_esrgan

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import esrgan_backward_ref as ref  # noqa: E402
import esrgan_train_oracle as oracle  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256          # bytes after the saved buffer and the workspaces, floats' worth after each gradient tensor
SENTINEL = 0x5A


def model_of(sd, r, autograd=True):
    return load_esrgan(sd, num_residuals=r, device=DEV, strict=True, batch_stats=True, autograd=autograd).train()


def running(m):
    sd = m.state_dict()
    return {k: sd[k].clone() for k in sd if "running" in k or "num_batches" in k}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def cabi(m, x, G, want=None, masks=True):
    """One cid_esr_forward_saved + cid_esr_saved_masks + cid_esr_backward on module m's handle and BatchNorm tensors, NaN-filled saved
    buffer and workspaces, guards checked.  x: fp32 [N,3,H,W] or uint8 [N,H,W,3] on the device.
    -> (out, {name: gradient} for the names in `want` (default: all), the masks as bool tensors on the CPU)"""
    L = _lib.lib()
    u8 = x.dtype == torch.uint8
    n, h, w = (x.shape[0], x.shape[1], x.shape[2]) if u8 else (x.shape[0], x.shape[2], x.shape[3])
    fmt = _lib.CID_FMT_U8_NHWC if u8 else _lib.CID_FMT_F32_NCHW
    r = m.num_residuals
    m.pack_weights()
    need = ctypes.c_size_t()

    def buffer(sizer):
        assert sizer(n, h, w, r, ctypes.byref(need)) == 0
        t = torch.full((need.value + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
        t[:need.value].view(torch.float32).fill_(float("nan"))
        return t, need.value

    saved, nsaved = buffer(L.cid_esr_saved_bytes)
    fws, nfws = buffer(L.cid_esr_train_workspace_bytes)
    bws, nbws = buffer(L.cid_esr_backward_workspace_bytes)
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=DEV)
    bn = m._bn_args(torch.device(DEV))
    x = x.contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    m._check(L.cid_esr_forward_saved(m._cid, x.data_ptr(), fmt, out.data_ptr(), n, h, w, bn, saved.data_ptr(), nsaved, fws.data_ptr(), nfws,
                                     stream))
    got_masks = []
    if masks:
        mt = [torch.full((n, 64, h, w), 7, dtype=torch.uint8, device=DEV) for _ in range(1 + r)]
        arr = (ctypes.c_void_p * len(mt))(*[t.data_ptr() for t in mt])
        assert L.cid_esr_saved_masks(saved.data_ptr(), nsaved, n, h, w, r, arr, stream) == 0
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
    m._check(L.cid_esr_backward(m._cid, x.data_ptr(), fmt, G.data_ptr(), n, h, w, bn, saved.data_ptr(), nsaved, ctypes.byref(g),
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


def check_against_float64(sd, x32, G, r, grads, masks, e_aten, who="HIP"):
    """The rule of error: float64 with the device's masks (capped); e_hip(T) <= max(1e-5, 2 * e_aten(T)).  Prints every figure first."""
    g64, pre64, _, book = ref.ref_backward(sd, x32, G.cpu(), r, torch.float64, masks=masks)
    flips = ref.check_mask_cap(masks, pre64, who)
    errs = ref.rel_errors({k: v.cpu() for k, v in grads.items()}, g64, book)
    bad = []
    for k, e in errs.items():
        bound = max(ref.TOL, 2 * e_aten.get(k, 0.0))
        print(f"    {k:32s} e_hip {e:.2e}  e_aten {e_aten.get(k, float('nan')):.2e}  bound {bound:.2e}")
        if not e <= bound:
            bad.append((k, e, bound))
    print(f"  {who}: {flips} mask flips, worst e_hip {max(errs.values()):.2e}, "
          f"worst share of the bound {max(e / max(ref.TOL, 2 * e_aten.get(k, 0.0)) for k, e in errs.items()):.3f}")
    assert not bad, bad


# --------------------------------------------------------------------------------------------------------------- parity, C ABI
@pytest.mark.parametrize("rc", ref.CASES, ids=ref.case_id)
@pytest.mark.parametrize("wset", ["default", "hot"])
def test_gradient_parity_through_the_c_abi(wset, rc):
    r, case = rc
    n, h, w = case
    sd = synth.make_esrgan_state_dict(wset, r)
    x32 = ref.case_input(case)
    x, G = torch.from_numpy(x32).to(DEV), ref.grad_out(n, h, w).to(DEV)
    e_aten, _ = ref.aten_errors(wset, rc)
    plain = model_of(sd, r, autograd=False)
    with torch.no_grad():
        want_out = plain(x)
    m = model_of(sd, r)
    out, grads, masks = cabi(m, x, G)
    assert torch.equal(_bits(out), _bits(want_out))                      # bit-identical to cid_esr_forward_train
    got, want = running(m), running(plain)
    assert all(torch.equal(_bits(got[k]), _bits(want[k])) for k in want) and len(want) == 6 * r
    assert list(grads) == ref.param_names(r) and len(masks) == 1 + r
    check_against_float64(sd, x32, G, r, grads, masks, e_aten)


def test_repeatability():
    """Two calls give identical bits (NaN-filled buffers both times)."""
    case, r = (3, 8, 12), 2
    sd = synth.make_esrgan_state_dict("hot", r)
    x, G = torch.from_numpy(oracle.case_input(case)).to(DEV), ref.grad_out(*case).to(DEV)
    m = model_of(sd, r)
    out1, g1, _ = cabi(m, x, G, masks=False)
    out2, g2, _ = cabi(m, x, G, masks=False)
    assert torch.equal(_bits(out1), _bits(out2)) and all(torch.equal(_bits(g1[k]), _bits(g2[k])) for k in g1)


@pytest.mark.parametrize("slope", [0.0, -0.5])
def test_slopes_zero_and_negative(slope):
    """Every PReLU slope (head, blocks) set by hand: with a <= 0 the sign of an activated value says nothing about its
    pre-activation (a = 0 even erases it), so masks and slope gradients must come from what the forward saw."""
    case, r = (3, 8, 12), 2
    n, h, w = case
    sd = dict(synth.make_esrgan_state_dict("default", r))
    for k in ref.slope_names(r):
        sd[k] = np.full_like(sd[k], slope)
    x32 = oracle.case_input(case)
    x, G = torch.from_numpy(x32).to(DEV), ref.grad_out(n, h, w).to(DEV)
    e_aten, _ = ref.aten_errors("default", (r, case), sd=sd, tag=slope)
    assert max(e_aten.values()) <= ref.TOL                                 # the reference is well-conditioned here as well
    m = model_of(sd, r)
    _, grads, masks = cabi(m, x, G)
    for i, mk in enumerate(masks):
        assert 0.05 < float(mk.float().mean()) < 0.95, i                   # both branches are taken
    check_against_float64(sd, x32, G, r, grads, masks, e_aten)
    assert all(float(grads[k].abs().max()) > 0 for k in ref.slope_names(r))


# --------------------------------------------------------------------------------------------------------------- the module
def module_grads(m, x, G, out_dtype=None):
    m.zero_grad(set_to_none=True)
    out = m(x) if out_dtype is None else m(x, out_dtype=out_dtype)
    assert out.requires_grad and out.grad_fn is not None
    (out * G).sum().backward()
    return out.detach(), {k: p.grad for k, p in m.named_parameters()}


def test_module_backward_is_the_c_abi():
    """loss.backward() through the module gives the bits of cid_esr_backward called directly (whose parity the tests above hold)."""
    case, r = (1, 13, 18), 8
    sd = synth.make_esrgan_state_dict("hot", r)
    x, G = torch.from_numpy(oracle.case_input(case)).to(DEV), ref.grad_out(*case).to(DEV)
    m = model_of(sd, r)
    want_out, want, _ = cabi(model_of(sd, r), x, G, masks=False)
    xin = x.clone().requires_grad_(True)
    out, got = module_grads(m, xin, G)
    assert xin.grad is None                                               # noisy is data
    assert torch.equal(_bits(out), _bits(want_out))
    for k in want:
        assert got[k] is not None and got[k].shape == want[k].shape and torch.equal(_bits(got[k]), _bits(want[k])), k
    # the saved buffer is released by the backward; a second forward / backward accumulates into .grad (the running statistics, which
    # the second forward starts from, do not enter a train-mode gradient)
    out2 = m(x)
    (out2 * G).sum().backward()
    k = "residuals.3.block.3.weight"
    assert torch.equal(m.get_parameter(k).grad, want[k] + want[k])
    # eval mode, no_grad and a uint8 output carry no history
    with torch.no_grad():
        assert m(x).grad_fn is None
    assert m(x, out_dtype=torch.uint8).grad_fn is None
    assert m.eval()(x).grad_fn is None


def test_uint8_input_and_frozen_parameters():
    case, r = (3, 8, 12), 2
    n, h, w = case
    sd = synth.make_esrgan_state_dict("default", r)
    u8 = ref.case_u8(case)
    x32 = oracle.case_input(case)
    G = ref.grad_out(n, h, w).to(DEV)
    m = model_of(sd, r)
    out, got = module_grads(m, torch.from_numpy(u8).to(DEV), G, out_dtype=torch.float32)
    e_aten, _ = ref.aten_errors("default", (r, case))
    _, _, masks = cabi(model_of(sd, r), torch.from_numpy(u8).to(DEV), G, want=[])
    check_against_float64(sd, x32, G, r, got, masks, e_aten)
    # frozen parameters get no gradient; the others keep their bits
    frozen = ("initial.0.weight", "residuals.1.block.1.weight", "residuals.1.block.2.weight", "residuals.0.block.3.bias", "final.weight")
    f = model_of(sd, r)
    for k in frozen:
        f.get_parameter(k).requires_grad_(False)
    _, part = module_grads(f, torch.from_numpy(u8).to(DEV), G, out_dtype=torch.float32)
    for k in got:
        if k in frozen:
            assert part[k] is None, k
        else:
            assert torch.equal(_bits(part[k]), _bits(got[k])), k


def test_in_place_change_between_forward_and_backward_raises():
    m = model_of(synth.make_esrgan_state_dict("default", 1), 1)
    out = m(torch.from_numpy(oracle.case_input((1, 5, 7))).to(DEV))
    with torch.no_grad():
        m.final.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="parameter final.bias was modified in place"):
        out.sum().backward()


def test_a_second_backward_through_one_forward_raises():
    """The saved buffer belongs to one backward; retain_graph=True does not keep it."""
    m = model_of(synth.make_esrgan_state_dict("default", 1), 1)
    out = m(torch.from_numpy(oracle.case_input((1, 5, 7))).to(DEV))
    out.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="saved activations were released by its first backward"):
        out.sum().backward()


def test_an_optimizer_step_reaches_the_next_forwards():
    """Adam step, train forward at the new weights, then .eval(): the eval forward folds the UPDATED running statistics and equals a
    freshly loaded module's, bit for bit."""
    r, case = 2, (2, 16, 16)
    m = model_of(synth.make_esrgan_state_dict("default", r), r)
    x, G = torch.from_numpy(oracle.case_input(case)).to(DEV), ref.grad_out(*case).to(DEV)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    (m(x) * G).sum().backward()
    opt.step()
    out = m(x)
    fresh = model_of({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, r, autograd=False)
    assert torch.equal(_bits(m.eval()(x)), _bits(fresh.eval()(x)))
    assert not torch.equal(out.detach(), m(x))                            # train and eval differ, the fold was not reused


@pytest.mark.parametrize("r", [0, 1, 8, 16])
@pytest.mark.parametrize("wset", ["default", "hot"])
def test_device_pack_equals_the_host_pack(wset, r):
    """cid_esr_pack_weights_device against cid_esr_upload_weights: byte equality of the whole blob (an 0xFF-filled blob before the
    call, so every float is written), at the loaded state and again after a train forward has moved the running statistics."""
    sd = synth.make_esrgan_state_dict(wset, r)
    want = load_esrgan(sd, num_residuals=r, device=DEV, strict=True).pack_weights()
    m = model_of(sd, r)
    m._blob.fill_(0xFF)
    got = m.pack_weights()
    assert got.data_ptr() == m._blob.data_ptr() and got.numel() == want.numel()
    assert torch.equal(got, want)
    with torch.no_grad():
        m(torch.from_numpy(oracle.case_input((1, 5, 7))).to(DEV))
    state = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    if r:
        key = f"residuals.{r - 1}.block.4.running_var"
        assert not np.array_equal(state[key], sd[key])
    ptr = m._blob.data_ptr()
    m._blob.fill_(0xFF)
    got = m.pack_weights()
    assert got.data_ptr() == ptr                                          # one blob that stays in place
    assert torch.equal(got, load_esrgan(state, num_residuals=r, device=DEV, strict=True).pack_weights())


def test_composition_with_the_discriminator():
    """The generator step of the ESRGAN trainer on one small batch: the parameter gradients of MSE(denoised, clean) + 1e-3 *
    BCEWithLogits(D(denoised), 1) through autograd are, bit for bit, cid_esr_backward called with the grad_out that D and the MSE
    produce for `denoised` taken as a leaf.  Plumbing only."""
    from celebrity_image_denoiser_amd.esrgan_disc import ESRGANDiscriminator

    r, (n, h, w) = 2, (2, 16, 16)
    sd = synth.make_esrgan_state_dict("default", r)
    x = torch.from_numpy(oracle.case_input((n, h, w))).to(DEV)
    clean = torch.from_numpy(synth.clean_images_u8(n, h, w, oracle._FIRST[(n, h, w)]).transpose(0, 3, 1, 2).astype(np.float32) / 255).to(DEV)
    D = ESRGANDiscriminator((3, h, w), autograd=True)
    D.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_esrgan_disc_state_dict("default", (3, h, w)).items()}, strict=True)
    D.to(DEV).train()
    mse, bce = nn.MSELoss(), nn.BCEWithLogitsLoss()

    def g_loss(denoised):
        pred = D(denoised)
        return mse(denoised, clean) + 1e-3 * bce(pred, torch.ones_like(pred))

    m = model_of(sd, r)
    g_loss(m(x)).backward()
    got = {k: p.grad.clone() for k, p in m.named_parameters()}
    D.zero_grad(set_to_none=True)
    with torch.no_grad():
        denoised = model_of(sd, r, autograd=False)(x)
    leaf = denoised.clone().requires_grad_(True)
    g_loss(leaf).backward()
    _, want, _ = cabi(model_of(sd, r), x, leaf.grad.contiguous(), masks=False)
    assert len(want) == len(ref.param_names(r))
    for k in want:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k
