"""What the backward kernels decide AT a discontinuity: exact zeros, exact ties, degenerate BatchNorm statistics, byte boundaries.

The parity suites of the six backward families share each fp32 run's ReLU / LeakyReLU / PReLU masks and pool routings with the
float64 reference under a cap, which is right for random data and leaves the decision at the discontinuity itself unpinned: an
exactly zero pre-activation and an exactly tied window sit inside the cap whatever the kernel does there.  The cases here are
constructed (tests/test_discontinuities_host.py builds them and proves their preconditions on ATen alone), so the zero and the tie
are exact in float64, in ATen fp32 and in the device's stored tensors, and the reference takes ATen's decision there:

  * a mask is False at an exact zero (ReLU's derivative 0, LeakyReLU(0.2)'s 0.2, PReLU's slope);
  * a pool window routes to F.max_pool2d(stored, 2, return_indices=True)'s index, ATen's rule applied to the device's stored
    activation (cid_stage_view / cid_vgg_saved_view): the first maximum in scan order;
  * everywhere else the device's masks are shared under the families' existing caps, unchanged.

Reference: float64 autograd on the CPU, the families' own (ref_backward, vgg_backward_ref, ...).  Error e(T) and its denominators are
the families'; bound e_hip(T) <= max(1e-5, 2 e_aten(T)) with e_aten from ATen fp32 on the CPU for the same case.  The host file
asserts e_aten <= 0.5e-5 for every tensor of every case, so 1e-5 governs.  Each case asserts that its constructed units are exactly
0.0 (either sign), or exactly tied, in the device's stored tensors as well.

Part A (ties), construction per family.  Generator (3,32,16) and VGG (32,16,2), (18,22,2): STRIPES, an image constant along y gives
bit-equal rows of a 3x3 convolution away from the border for any arithmetic that does not depend on the pixel's position, hence
windows [a b; a b] (winner 0 or 1); the generator runs it under conv_algo="direct" (the rows of a Winograd tile are not computed with
the same arithmetic), the VGG tower's k_lpips_conv sums a column's neighbourhood alone.  Generator (3,16,32) and VGG (16,32,2): the
LATTICE, a channel that copies a plane drawn from {0, 1/4, 1/2, 3/4, 1} through identity-tap weights in both convolutions of both
blocks; every sum is exact in fp32 and float64 and every 2x2 tie pattern occurs (winners 0, 1 and 2).  It stands in for the image
constant along x: there the device's columns are bit-equal, but ATen's float64 convolution (an im2col GEMM over the pixels of a row)
gives its remainder columns another summation order, and the reference has to have the tie.  Dead-weight channels with
bias 0.25 add four-way ties in every case and run under both generator algorithms.  Floor on the device's stored tensor: half the
share the host file measures with ATen fp32, per pool, and the winners above among the tied windows.

    share of windows with an exact positive tie (striped images / lattice channel)    ATen fp32 (host)   floor           MI355X
    generator  stripes  (3,32,16)   pool1 / pool2                                   0.547 / 0.326      0.270 / 0.160   0.547 / 0.326
    generator  lattice  (3,16,32)   pool1 / pool2                                   0.365 / 0.833      0.180 / 0.415   0.365 / 0.833
    VGG        stripes  (32,16,2)   pool1 / pool2                                   0.589 / 0.336      0.290 / 0.165   0.589 / 0.336
    VGG        lattice  (16,32,2)   pool1 / pool2                                   0.336 / 0.844      0.165 / 0.420   0.336 / 0.844
    VGG        stripes  (18,22,2)   pool1 / pool2                                   0.508 / 0.163      0.250 / 0.080   0.508 / 0.163
On the device every striped tensor's interior rows are bit-equal and every share is ATen's.

Parts B and C on the BatchNorm discriminators take their masks from cid_disc_saved_masks / cid_srd_saved_masks as the families' suites
do and set them False at the constructed units, whatever those routines say; the stored a0, raw z and hidden pre-activations are read
out of the saved buffer (include/cid.h's layout) for the preconditions.  Their large shape for the e_aten <= 0.5e-5 assertion is
(4,19,37); (8,37,53), where ATen's own error is above that with untouched weights, runs too (host file).

Measured on an MI355X, worst e_hip / bound per family (1e-5 governs everywhere but at (8,37,53)):
    generator                 0.123  (pixel-sparse zeros; ties 0.104, zero channels 0.096)
    VGG content loss          0.202  (zero channels; ties 0.140)
    DenoiseDiscriminator      0.368  (part C, (8,37,53); part B 0.308)          max|p - p64| 7.7e-7
    SRGANDiscriminator        0.344  (part B, (8,37,53) train; part C 0.263)    max|p - p64| 4.4e-7
    ESRGANDiscriminator       0.180
    SRGANGenerator (train)    0.333  (part B; part C 0.313)
Worst forward error in part C: SRGANGenerator 0.132 of 1e-5 max(1, max|ref|) over its five stages; probabilities 1.2e-7
(DenoiseDiscriminator) and 3.4e-8 (SRGANDiscriminator) against a bound of 1e-5.
Part D: cid_view_u8 and the ESRGAN tail give torch fp32's bytes at every boundary; the SRGAN and cGAN tails differ by one byte at
some boundaries (tanhf against ATen's tanh), never by two.
"""
import os
import sys

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import synth
from celebrity_image_denoiser_amd.generator import DenoiseGenerator
from celebrity_image_denoiser_amd.lpips import load_vgg_loss

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_discontinuities_host as host  # noqa: E402
import test_generator_backward as gen  # noqa: E402
import test_vgg_backward as vgg  # noqa: E402
import vgg_backward_ref as vref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5


def _report(what, e_hip, e_aten):
    """Prints every figure, then asserts the bound."""
    worst = 0.0
    for k in e_hip:
        bound = max(TOL, 2 * e_aten[k])
        worst = max(worst, e_hip[k] / bound)
        print(f"    {what} {k:20s} e_hip {e_hip[k]:.2e}  e_aten {e_aten[k]:.2e}  e_hip/bound {e_hip[k] / bound:.3f}")
    print(f"{what}: worst e_hip / bound {worst:.3f}")
    for k in e_hip:
        assert e_hip[k] <= max(TOL, 2 * e_aten[k]), (what, k, e_hip[k], e_aten[k])


def _check_ties(what, stored, key, kind):
    """The floor on the part of the device's stored pool inputs that carries the constructed ties: the share of exactly tied positive
    windows, the winners; for a lattice channel, the stored values themselves."""
    for k, e in enumerate(stored):
        share, winners = host.tie_stats(e)
        floor = 0.5 * host.TIE_SHARE[key][k]
        equal = f", interior rows bit-equal: {host.interior_equal(e, 'y', 2 + k)}" if kind == "y" else ""
        print(f"{what} pool{k + 1}: device tie share {share:.3f} (floor {floor:.3f}), winners {sorted(winners)}{equal}")
        assert share >= floor, (what, k, share, floor)
        assert winners >= host.WINNERS[kind], (what, k, winners)


# ------------------------------------------------------------------------------------------------------------------- generator
def _gen_module(sd, algo):
    m = DenoiseGenerator()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m.to(DEV)
    m.conv_algo = algo
    return m


def _gen_run(name, algo):
    """One generator case on the device against float64 with ATen's decisions on the device's stored tensors.
    -> (case, device grads on the CPU, stored stages by name)"""
    c = host.gen_reference(name)
    n, _, h, w = c["x"].shape
    clean = torch.from_numpy(c["clean"]).to(DEV)
    m = _gen_module(c["sd"], algo)
    y, grads, gx, saved, _ = gen.cabi_backward(m, torch.from_numpy(c["x"]).to(DEV), lambda out: gen._mse_grad(out, clean))
    stages = {s: gen.stage(saved, s, n, h, w).cpu() for s in gen.RELU_STAGES}
    masks = [stages[s] > 0 for s in gen.RELU_STAGES]                      # False at a stored 0.0 or -0.0: ATen's ReLU derivative
    argmax = [host.aten_winner(stages["down1"]), host.aten_winner(stages["down2"])]   # ATen's routing of the stored activation
    g64, gx64, pre64, pin64, own64, y64 = gen.ref_backward(c["sd"], c["x"], torch.float64, ("mse", torch.from_numpy(c["clean"])), masks, argmax)
    assert float((y.cpu().double() - y64).abs().max()) <= TOL
    gen.check_caps(masks, argmax, pre64, pin64, own64, "hip")
    got = {k: v.cpu() for k, v in grads.items()}
    assert all(bool(torch.isfinite(v).all()) for v in got.values()) and bool(torch.isfinite(gx).all())
    _report(f"generator {name} {algo}", gen.rel_errors(got, gx.cpu(), g64, gx64), c["e_aten"])
    return c, got, stages


@pytest.mark.parametrize("kind", ("y", "lattice"))
def test_generator_pool_routing_on_exact_ties(kind):
    """Part A: both pools of cid_backward (k_gen_pool_bwd) on two-way ties ([a b; a b] rows of a striped image, every pattern on the
    lattice channel) and on four-way ties, under conv_algo="direct"."""
    c, _, stages = _gen_run("tie-" + kind, "direct")
    pin = [stages["down1"], stages["down2"]]
    if kind == "lattice":
        plane = torch.from_numpy(c["x"][:, 0])
        assert torch.equal(pin[0][:, host.GEN_LATTICE[1][1]], plane)
        assert torch.equal(pin[1][:, host.GEN_LATTICE[3][1]], torch.nn.functional.max_pool2d(plane, 2))
    _check_ties(f"generator {kind}", host.tied_part(kind, pin), ("gen", kind), kind)
    for s, layer in (("down1", "down1.2"), ("down2", "down2.2")):
        for ch in host.GEN_CONST[layer]:
            assert bool((stages[s][:, ch] == host.CONST_BIAS).all()), (layer, ch)


@pytest.mark.parametrize("algo", ("winograd42", "direct"))
def test_generator_pool_routing_on_constant_channels(algo):
    """Part A: a dead-weight channel with bias 0.25 is a four-way tie in every window; index 0 wins."""
    _, _, stages = _gen_run("const", algo)
    for s, layer in (("down1", "down1.2"), ("down2", "down2.2")):
        for ch in host.GEN_CONST[layer]:
            assert bool((stages[s][:, ch] == host.CONST_BIAS).all()), (layer, ch)


@pytest.mark.parametrize("algo", ("winograd42", "direct"))
def test_generator_relu_mask_at_exactly_zero(algo):
    """Part B: dead channels (zero weights, zero bias) in down1.0, down2.2, bottleneck.0 and upconv2.0: ReLU's derivative at 0 is 0, so
    their bias gradients and weight-gradient rows are exactly 0.0."""
    _, got, stages = _gen_run("zero", algo)
    stage_of = {"down1.0": "down1.0", "down2.2": "down2", "bottleneck.0": "bottleneck.0", "upconv2.0": "upconv2.0"}
    for layer, ch in host.GEN_ZERO.items():
        assert host.is_zero(stages[stage_of[layer]][:, ch]), layer
        assert host.is_zero(got[layer + ".bias"][ch]) and host.is_zero(got[layer + ".weight"][ch]), layer


def test_generator_relu_mask_at_pixel_sparse_zeros():
    """Part B: a head channel that copies input channel 0, whose pixels are exactly 0.0 at 10 % and -0.0 at 5 %."""
    c, _, stages = _gen_run("sparse", "direct")
    assert bool(((stages["down1.0"][:, host.GEN_HEAD_TAP] == 0) == torch.from_numpy(c["zero"])).all())


# ------------------------------------------------------------------------------------------------------------------------- VGG
def _vgg_run(case, axis=None):
    c = host.vgg_reference(case, axis)
    h, w, n = case
    sd = c["sd"]
    m = load_vgg_loss({k: torch.from_numpy(v) for k, v in synth.vgg_loss_state_dict(sd).items()}, device=DEV, autograd=True)
    go = torch.from_numpy(c["go"])
    _, gx, arena = vgg.cabi(m, vgg.dev(c["a"]), vgg.dev(c["b"]), go)
    acts = [vgg.view(arena, name, n, h, w)[:n] for name in vref.ACTS]
    masks, routes = vref.own_discontinuities(acts)          # stored > 0 and F.max_pool2d's indices on the stored activations
    vref.check_masks(masks, c["pre_a"], "hip")
    vref.check_routing(routes, c["act_a"], "hip")
    g64 = vref.backward64(sd, c["act_a"], c["act_b"][6], c["go"], masks, routes)
    got = {name: vgg.view(arena, name, n, h, w) for name in vref.GRADS}
    got["grad_x"] = gx.cpu()
    for name in got:
        assert got[name].shape == g64[name].shape and bool(torch.isfinite(got[name]).all()), name
    _report(f"VGG {case} {axis or 'zero channels'}", {k: vref.rel_err(got[k], g64[k]) for k in ("grad_x",) + vref.GRADS}, c["e_aten"])
    return c, got, acts


@pytest.mark.parametrize("case,axis", host.VGG_TIE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_vgg_pool_routing_on_exact_ties(case, axis):
    """Part A: both pools of cid_vgg_content_backward (the UNPOOL staging) on tied windows; (18,22) adds the rows and columns past
    2 floor(size / 2), which get zero."""
    c, _, acts = _vgg_run(case, axis)
    if axis == "lattice":
        plane = torch.from_numpy(c["a"][:, 0])
        assert torch.equal(acts[1][:, host.VGG_LATTICE[1][1]], plane)
        assert torch.equal(acts[3][:, host.VGG_LATTICE[3][1]], torch.nn.functional.max_pool2d(plane, 2))
    _check_ties(f"VGG {case}", host.vgg_tied_part(axis, acts), ("vgg", case), axis)
    for i, layer in ((1, "net.slice1.2"), (3, "net.slice2.7")):
        assert bool((acts[i][:, host.VGG_CONST[layer]] == host.CONST_BIAS).all()), layer


def test_vgg_relu_mask_at_exactly_zero():
    """Part B: dead channels in conv1_1, conv2_2 and conv3_2; the stored gradients of the two that are kept are exactly 0.0 there."""
    _, got, acts = _vgg_run(host.VGG_ZERO_CASE)
    for layer, ch in host.VGG_ZERO.items():
        assert host.is_zero(acts[host.VGG_ZERO_ACT[layer]][:, ch]), layer
    assert host.is_zero(got["grad1_1"][:, host.VGG_ZERO["net.slice1.0"]]) and host.is_zero(got["grad3_2"][:, host.VGG_ZERO["net.slice3.12"]])


# ------------------------------------------------------------------------------------------------- the BatchNorm discriminators
def _bn_class(name):
    if name == "denoise":
        from celebrity_image_denoiser_amd.discriminator import DenoiseDiscriminator
        return DenoiseDiscriminator
    from celebrity_image_denoiser_amd.srgan_disc import SRGANDiscriminator
    return SRGANDiscriminator


def _a256(v):
    return (v + 255) // 256 * 256


def _bn_saved_tensors(fam, saved, n, h, w):
    """a0 and the raw z of every BatchNorm'd convolution out of a cid_disc / cid_srd saved buffer (the layout of include/cid.h), as
    [N,C,Hs,Ws] on the CPU, and the SRGAN head's fp64 hidden pre-activations [N,512] (or None)."""
    from esrgan_disc_oracle import c8_to_nchw

    side = lambda s: (s - 1) // 2 + 1   # noqa: E731
    sizes = [(h, w), (side(h), side(w)), (side(h), side(w)), (side(side(h)), side(side(w))), (side(side(h)), side(side(w)))]
    out, at = [], 0
    for (_, _, c), (hs, ws) in zip(fam.leaky, sizes):
        out.append(c8_to_nchw(saved[at:at + 4 * n * c * hs * ws].view(torch.float32), n, c, hs, ws).cpu())
        at += _a256(4 * n * c * hs * ws)
    hidden = None
    if fam.hidden is not None:
        at += _a256(4 * 4 * 256 * 2) + _a256(8 * 4 * 256 * 2) + _a256(8 * n * 256)
        hidden = saved[at:at + 8 * n * 512].view(torch.float64).view(n, 512).cpu()
    return out, hidden


@pytest.mark.parametrize("case", host.BN_CASES, ids=host.bn_case_id)
@pytest.mark.parametrize("name", ("denoise", "srgan"))
def test_batchnorm_discriminators_at_exact_zeros_and_degenerate_statistics(name, case):
    """Parts B and C on cid_disc_* and cid_srd_*.  B: a dead channel in every LeakyReLU'd convolution (beta 0 behind a BatchNorm), a
    dead hidden unit, pixel-sparse zeros: the float64 reference uses slope 0.2 there.  C (train mode): a channel with |mean| / std =
    32 and a constant channel (bias 2^-5, so y = 0 exactly with beta = 0) in every BatchNorm'd convolution: probabilities, running
    buffers and every gradient."""
    part, shape, training, _ = case
    c = host.bn_reference(name, case)
    fam = host.bn_family(name)
    bwd, cls = fam.bwd, _bn_class(name)
    n, h, w = shape
    x = c["x"].to(DEV)

    def module(autograd):
        m = cls(autograd=autograd)
        m.load_state_dict(c["sd"], strict=True)
        return m.to(DEV).train(training)

    p, grads, gx, masks, _ = bwd.cabi_backward(module(False), x, training, lambda q: bwd._bce_grad(q, c["target"]))
    # the saved buffer of the same forward, and the BatchNorm buffers after it, through the differentiable module
    ma = module(True)
    pa = ma(x)
    assert torch.equal(pa.detach(), p)
    stored, hidden = _bn_saved_tensors(fam, pa.grad_fn.saved, n, h, w)
    masks = [t.cpu().bool() for t in masks]
    for i, ch, pixels in c["forced"]:
        if i == len(fam.leaky):
            assert host.is_zero(hidden[:, ch]), "hidden unit"
        elif part == "C":
            assert bool((stored[i][:, ch] == host.DISC_CONST_BIAS).all()), (i, ch)
        else:
            assert host.is_zero(host.forced_units(stored[i], ch, pixels)), (i, ch)
            if pixels is not None:
                assert bool(((stored[i][:, ch] == 0) == pixels).all())
        # ATen's decision at an exact zero: slope 0.2
        unit = masks[i].reshape(masks[i].shape[0], masks[i].shape[1], -1)[:, ch]
        if pixels is None:
            unit[:] = False
        else:
            unit[pixels.reshape(pixels.shape[0], -1)] = False
    g64, gx64, ys64, p64 = bwd.ref_backward(c["sd"], c["x"], training, c["target"], torch.float64, masks)
    e_p = float((p.cpu().double() - p64).abs().max())
    print(f"{name} {host.bn_case_id(case)}: max|p - p64| {e_p:.2e}")
    assert e_p <= TOL
    bwd.check_mask_cap(masks, ys64, "hip")
    if training:
        for idx in [bn for _, bn, _ in fam.leaky if bn is not None]:
            for b in ("running_mean", "running_var"):
                got, want = getattr(ma.model[idx], b).cpu().double(), c["running"][f"model.{idx}.{b}"]
                assert bool(((got - want).abs() <= TOL * torch.clamp(want.abs(), min=1.0)).all()), (idx, b, float((got - want).abs().max()))
            assert int(ma.model[idx].num_batches_tracked) == int(c["running"][f"model.{idx}.num_batches_tracked"])
    got = {k: v.cpu() for k, v in grads.items()}
    assert all(bool(torch.isfinite(v).all()) for v in got.values()) and bool(torch.isfinite(gx).all())
    _report(f"{name} {host.bn_case_id(case)}", bwd.rel_errors(got, gx.cpu(), g64, gx64, training), c["e_aten"])


# ------------------------------------------------------------------------------------------------------ the ESRGAN discriminator
@pytest.mark.parametrize("case", host.ESD_CASES, ids=lambda c: "x".join(map(str, c[0])) + "-" + c[1])
def test_esrgan_discriminator_at_exact_zeros(case):
    """Part B on cid_esd_*: a dead channel in each of conv1 ... conv4 and pixel-sparse zeros behind conv1; the backward's a > 0 staging
    must take slope 0.2 at a stored 0.0."""
    import esrgan_disc_bwd_oracle as bwd
    import test_esrgan_disc_backward as esd

    shape, _ = case
    c = host.esd_reference(case)
    m = esd._module("trained", shape[1:], sd=c["sd"])
    x = c["x"].to(DEV)
    logits, saved = esd.forward_saved(m, x)
    assert float((logits.cpu().double() - c["logits64"].view(-1)).abs().max()) <= TOL * max(1.0, float(c["logits64"].abs().max()))
    grads, gx = esd.backward(m, x, saved, bwd.bce_grad(logits, c["loss"]))
    stages = esd.saved_stages(saved, shape)
    for i, ch, pixels in c["forced"]:
        assert host.is_zero(host.forced_units(stages[i], ch, pixels)), (i, ch)
        if pixels is not None:
            assert bool(((stages[i][:, ch] == 0) == pixels).all())
    masks = [a > 0 for a in stages]                 # False at a stored 0.0 or -0.0
    bwd.check_mask_cap(masks, c["ys64"], "hip")
    g64, gx64 = bwd.ref_backward(c["sd"], c["x"], c["loss"], torch.float64, masks)[:2]
    got = {k: v.cpu() for k, v in grads.items()}
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    _report(f"ESRGAN discriminator {case}", bwd.rel_errors(got, gx.cpu(), g64, gx64), c["e_aten"])


# ------------------------------------------------------------------------------------------- part D: uint8 truncation boundaries
def test_view_u8_at_every_truncation_boundary():
    """cid_view_u8 on the smallest fp32 pre-image of every byte 1 ... 255, its three neighbours on each side, +-1 and their neighbours
    and +-0, in one 1x3x25x25 launch: the bytes of (x*0.5+0.5).clamp(0,1).mul(255).byte() in torch fp32."""
    from celebrity_image_denoiser_amd import _lib

    vals, count = host.boundary_values()
    want = host.view_u8_expr(torch.from_numpy(vals)).permute(0, 2, 3, 1).contiguous()
    x = torch.from_numpy(vals).to(DEV)
    out = torch.full((1, 25, 25, 3), 77, dtype=torch.uint8, device=DEV)
    assert _lib.lib().cid_view_u8(x.data_ptr(), out.data_ptr(), 1, 25, 25, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    diff = (out.cpu() != want)
    assert not bool(diff.any()), (int(diff.sum()), vals.transpose(0, 2, 3, 1)[diff.numpy()][:8])


# ----------------------------------------------------------------------------------------- the SRGAN generator in train mode
@pytest.mark.parametrize("case", host.SR_CASES, ids=lambda c: "x".join(map(str, c)))
def test_srgan_generator_prelu_mask_at_exactly_zero(case):
    """Part B on cid_sr_forward_saved / cid_sr_backward: dead channels in initial.0, res_blocks.0.0, res_blocks.2.0 and upscale.0 (scale
    2); at v = 0 PReLU's input derivative is its slope and v adds nothing to the slope's own gradient.  The head's and the stage's
    zeros are read back from the stored x0 and tail_in; the trunk's have no view and are read from cid_sr_saved_masks."""
    import test_srgan_backward as srb

    n, h, w, scale = case
    c = host.sr_reference("B", case)
    x, G = torch.from_numpy(c["x"]).to(DEV), c["G"].to(DEV)
    plain = srb.model_of(c["sd"], scale, autograd=False)
    with torch.no_grad():
        want = plain(x)
    assert host.is_zero(plain.stage("x0", n, h, w).cpu()[:, host.SR_ZERO[0][2]])
    if scale > 1:
        assert host.is_zero(host.sr_units(plain.stage("tail_in", n, h, w).cpu(), host.SR_ZERO[3][4]))
    out, grads, masks = srb.cabi(srb.model_of(c["sd"], scale), x, G)
    assert torch.equal(out, want)
    for i, where in c["forced"]:
        assert not bool(host.sr_units(masks[i], where).any()), (i, where)
        host.sr_units(masks[i], where)[:] = False        # ATen's decision at an exact zero: the slope
    srb.check_against_float64(c["sd"], c["x"], G, grads, masks, c["e_aten"], who=f"SRGAN generator B {case}")


def test_srgan_generator_on_degenerate_batch_statistics():
    """Part C on cid_sr_forward_train / cid_sr_forward_saved / cid_sr_backward at (2,16,16,1): a channel with |mean| / std = 32 and a
    constant channel in each of the ten BatchNorm'd convolutions: every stage of the forward, the running buffers, every gradient."""
    import test_srgan_backward as srb
    import test_srgan_train as srt

    n, h, w, scale = case = host.SR_C_CASE
    c = host.sr_reference("C", case)
    x, G = torch.from_numpy(c["x"]).to(DEV), c["G"].to(DEV)
    ref = c["fwd64"]
    plain = srb.model_of(c["sd"], scale, autograd=False)
    with torch.no_grad():
        pre = plain(x, raw=True)
        stages = {k: plain.stage(k, n, h, w).cpu().numpy() for k in ("x0", "trunk", "tail_in")}
        srt.check_buffers(plain, ref)
        out = plain(x)
    worst = max(srt.check(k, stages[k], ref[k]) for k in ("x0", "trunk", "tail_in"))
    worst = max(worst, srt.check("pre", pre.cpu().numpy(), ref["pre"]), srt.check("out", out.cpu().numpy(), ref["out"]))
    print(f"SRGAN generator C: worst forward error / bound {worst:.3f}")
    out2, grads, masks = srb.cabi(srb.model_of(c["sd"], scale), x, G)
    assert torch.equal(out2, out)
    srb.check_against_float64(c["sd"], c["x"], G, grads, masks, c["e_aten"], who="SRGAN generator C")


@pytest.mark.parametrize("model", ("esrgan", "srgan", "cgan"))
def test_server_tails_at_truncation_boundaries(model):
    """The uint8 output of cid_esr_forward, cid_sr_forward and cid_cg_forward with a zero-weight tail convolution whose three biases sit
    on (or one fp32 value below) a truncation boundary: 8 triples per model, 1x8x8 (N = 1 for the cGAN).  ESRGAN's tail has no tanh and
    its bytes equal torch fp32's v.clamp(0,1).mul(255).byte().  The tanh tails take fp32(atanh(boundary)) as bias; ATen's tanh and
    tanhf differ in the last bit, which at a boundary is one byte, so there |byte - torch's| <= 1 is asserted."""
    from celebrity_image_denoiser_amd.cgan import load_cgan
    from celebrity_image_denoiser_amd.esrgan import load_esrgan
    from celebrity_image_denoiser_amd.srgan import load_srgan

    if model == "esrgan":
        sd, tail = synth.make_esrgan_state_dict("default", 1), "final"
        triples = host.tail_bias_triples(host.unit_u8_expr, 0.0)
        x = torch.from_numpy(synth.esrgan_inputs_u8(1, 8, 8, 3)).to(DEV)
        run = lambda s: load_esrgan(s, num_residuals=1, device=DEV, strict=True)(x)                     # noqa: E731
        want_of = lambda b: host.unit_u8_expr(b)                                                         # noqa: E731
    elif model == "srgan":
        sd, tail = synth.make_srgan_state_dict("default", 1), "final"
        triples = host.tail_bias_triples(through_tanh=True)
        x = torch.from_numpy(synth.srgan_inputs_u8(1, 8, 8, 3)).to(DEV)
        run = lambda s: load_srgan(s, scale_factor=1, device=DEV, strict=True)(x)                        # noqa: E731
        want_of = lambda b: host.view_u8_expr(torch.tanh(b))                                             # noqa: E731
    else:
        sd, tail = synth.make_cgan_state_dict("default", 10), "model.11"
        triples = host.tail_bias_triples(through_tanh=True)
        z, lab = torch.from_numpy(synth.cgan_latent_np(1, 5, 0)).to(DEV), torch.tensor([3], device=DEV)
        run = lambda s: load_cgan(s, n_classes=10, device=DEV, strict=True)(z, lab, out_dtype=torch.uint8)   # noqa: E731
        want_of = lambda b: host.view_u8_expr(torch.tanh(b))                                             # noqa: E731
    sd = {k: np.array(v) for k, v in sd.items()}
    sd[tail + ".weight"][:] = 0.0
    worst = 0
    for triple in triples:
        sd[tail + ".bias"][:] = triple
        got = run(sd)
        assert got.dtype == torch.uint8 and got.shape[0] == 1 and got.shape[3] == 3
        want = want_of(torch.from_numpy(triple)).view(1, 1, 1, 3).expand(got.shape)
        delta = int((got.cpu().int() - want.int()).abs().max())
        worst = max(worst, delta)
        print(f"{model} tail, biases {triple.tolist()}: bytes {got[0, 0, 0].tolist()}, torch fp32 {want[0, 0, 0].tolist()}")
        assert bool((got == got[:, :1, :1, :]).all())                  # one value per channel, whatever the pixel
        assert delta <= (0 if model == "esrgan" else 1), (model, triple, delta)
    print(f"{model} tail: worst |byte - torch fp32| {worst}")
