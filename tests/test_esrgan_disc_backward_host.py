"""The ESRGAN discriminator's backward pass without a GPU: the host side of cid_esd_saved_bytes, cid_esd_forward_saved,
cid_esd_backward and cid_esd_pack_weights_device (include/cid.h), the autograd flag of esrgan_disc.py, and the conditions the CPU
reference of tests/esrgan_disc_bwd_oracle.py must meet for the GPU tests' bound to mean what it says.  The GPU tests are in
tests/test_esrgan_disc_backward.py."""
import ctypes
import os
import sys

import pytest
import torch

from celebrity_image_denoiser_amd import _lib
from celebrity_image_denoiser_amd.esrgan_disc import ESRGANDiscriminator, load_esrgan_discriminator

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import esrgan_disc_oracle as oracle  # noqa: E402
import esrgan_disc_bwd_oracle as bwd  # noqa: E402
from esrgan_disc_bwd_oracle import Grads  # noqa: E402

ERR_INVALID, ERR_SHAPE, ERR_KEY, ERR_STATE, ERR_WORKSPACE = 1, 2, 3, 4, 5
FAKE = 1 << 20   # 256-byte aligned, never dereferenced: every call in this file must fail on the host
H, W = 37, 53


def _size(fn, n, h, w):
    out = ctypes.c_size_t()
    return getattr(_lib.lib(), fn)(n, h, w, ctypes.byref(out)), out.value


def test_saved_bytes_is_the_workspace_formula():
    for shape in bwd.SHAPES + [(8, 256, 256), (65537, 1, 1)]:
        _, total = oracle.expected_workspace(*shape)
        assert _size("cid_esd_saved_bytes", *shape) == (0, total) == _size("cid_esd_workspace_bytes", *shape), shape
    assert _size("cid_esd_saved_bytes", 0, 8, 8)[0] == ERR_SHAPE and _size("cid_esd_saved_bytes", 1, 0, 8)[0] == ERR_SHAPE
    assert _lib.lib().cid_esd_saved_bytes(2, 8, 8, None) == ERR_INVALID


def _a256(v):
    return (v + 255) // 256 * 256


def test_backward_workspace_bytes_is_the_documented_formula():
    for n, h, w in bwd.SHAPES + [(8, 256, 256), (65537, 1, 1)]:
        side = [(h, w)]
        for _ in range(4):
            side.append(((side[-1][0] - 1) // 2 + 1, (side[-1][1] - 1) // 2 + 1))
        want = sum(_a256(4 * n * c * side[l][0] * side[l][1]) for l, c in ((1, 64), (2, 128), (3, 256)))
        items = [n * -(-side[l][0] // 4) * -(-side[l][1] // 16) for l in (2, 3, 4)]
        splits = [min(it, max(s, -(-it // 2048))) for it, s in zip(items, (64, 16, 2))]
        want += _a256(4 * 9 * max(splits[0] * 128 * 64, splits[1] * 256 * 128, splits[2] * 512 * 256))
        want += _a256(8 * max(splits[0] * 128, splits[1] * 256, splits[2] * 512))
        want += _a256(8 * 64 * 28 * min(n * -(-side[1][0] * side[1][1] // 64), 256))
        assert _size("cid_esd_backward_workspace_bytes", n, h, w) == (0, want), (n, h, w)
    assert _size("cid_esd_backward_workspace_bytes", 0, 8, 8)[0] == ERR_SHAPE
    assert _size("cid_esd_backward_workspace_bytes", 1, 8, _lib.CID_ESD_MAX_SIDE + 1)[0] == ERR_SHAPE
    assert _lib.lib().cid_esd_backward_workspace_bytes(2, 8, 8, None) == ERR_INVALID


@pytest.fixture()
def handle():
    L = _lib.lib()
    d = ctypes.c_void_p()
    assert L.cid_esd_create(ctypes.byref(d), H, W) == 0
    yield d
    L.cid_esd_destroy(d)


def _fwd(d, n=2, h=H, w=W, x=FAKE, fmt=0, out=FAKE, sv=FAKE, sv_bytes=1 << 40):
    return _lib.lib().cid_esd_forward_saved(d, x, fmt, out, n, h, w, sv, sv_bytes, None)


def test_forward_saved_argument_errors_come_before_any_launch(handle):
    d = handle
    L = _lib.lib()
    assert L.cid_esd_forward_saved(None, FAKE, 0, FAKE, 2, H, W, FAKE, 1 << 40, None) == ERR_INVALID
    assert _fwd(d, x=None) == ERR_INVALID and L.cid_esd_last_error(d) == b"cid_esd_forward_saved: null pointer"
    assert _fwd(d, out=None) == ERR_INVALID
    assert _fwd(d, sv=None) == ERR_INVALID
    assert _fwd(d, fmt=7) == ERR_INVALID
    assert _fwd(d, x=FAKE + 1) == ERR_INVALID
    assert _fwd(d, x=FAKE + 1, fmt=1, sv_bytes=0) == ERR_WORKSPACE   # a uint8 input has no alignment
    assert _fwd(d, out=FAKE + 2) == ERR_INVALID
    for n in (0, -3):
        assert _fwd(d, n=n) == ERR_SHAPE
    for h, w in ((53, 37), (37, 54), (256, 256), (0, 53)):
        assert _fwd(d, h=h, w=w) == ERR_SHAPE
        assert b"the handle was created for 37x53" in L.cid_esd_last_error(d)
    need = _size("cid_esd_saved_bytes", 2, H, W)[1]
    assert _fwd(d, sv_bytes=need - 1) == ERR_WORKSPACE
    assert L.cid_esd_last_error(d) == b"cid_esd_forward_saved: saved buffer smaller than cid_esd_saved_bytes() or not 256-byte aligned"
    assert _fwd(d, sv=FAKE + 16, sv_bytes=need) == ERR_WORKSPACE
    assert _fwd(d, sv_bytes=need) == ERR_STATE
    assert L.cid_esd_last_error(d) == b"cid_esd_forward_saved: weights not uploaded"
    # the first of several faults is the one reported
    assert _fwd(d, x=None, n=0, sv_bytes=0) == ERR_INVALID
    assert _fwd(d, n=0, sv_bytes=0) == ERR_SHAPE
    assert _fwd(d, h=5, sv_bytes=0) == ERR_SHAPE


def _all_grads(**over):
    g = Grads()
    for i in range(5):
        g.w[i] = FAKE
        g.b[i] = FAKE
    g.input = FAKE
    for k, v in over.items():
        if k == "input":
            g.input = v
        else:
            getattr(g, k[0])[int(k[1])] = v
    return g


def _bwd(d, n=2, h=H, w=W, x=FAKE, fmt=0, gl=FAKE, sv=FAKE, sv_bytes=1 << 40, g="all", ws=FAKE, ws_bytes=1 << 40):
    if isinstance(g, str):
        g = _all_grads() if fmt == 0 else _all_grads(input=None)
    gp = None if g is None else ctypes.byref(g)
    return _lib.lib().cid_esd_backward(d, x, fmt, gl, n, h, w, sv, sv_bytes, gp, ws, ws_bytes, None)


def test_backward_argument_errors_come_before_any_launch(handle):
    d = handle
    L = _lib.lib()
    g = _all_grads()
    assert L.cid_esd_backward(None, FAKE, 0, FAKE, 2, H, W, FAKE, 1 << 40, ctypes.byref(g), FAKE, 1 << 40, None) == ERR_INVALID
    # CID_ERR_INVALID
    for kw in (dict(x=None), dict(gl=None), dict(sv=None), dict(g=None), dict(ws=None)):
        assert _bwd(d, **kw) == ERR_INVALID, kw
        assert L.cid_esd_last_error(d) == b"cid_esd_backward: null pointer"
    assert _bwd(d, fmt=7) == ERR_INVALID
    assert _bwd(d, x=FAKE + 1) == ERR_INVALID and _bwd(d, gl=FAKE + 2) == ERR_INVALID
    assert L.cid_esd_last_error(d) == b"cid_esd_backward: misaligned fp32 operand"
    for k in [f"{kind}{i}" for kind in "wb" for i in range(5)] + ["input"]:
        assert _bwd(d, g=_all_grads(**{k: FAKE + 2})) == ERR_INVALID, k
        assert L.cid_esd_last_error(d) == b"cid_esd_backward: misaligned gradient pointer"
    assert _bwd(d, fmt=1, g=_all_grads()) == ERR_INVALID   # a uint8 input has no gradient
    assert b"a uint8 input has no gradient" in L.cid_esd_last_error(d)
    assert _bwd(d, fmt=1, x=FAKE + 1, ws_bytes=0, sv_bytes=0) == ERR_WORKSPACE   # but it is accepted, at any alignment
    # CID_ERR_SHAPE
    for n in (0, -1):
        assert _bwd(d, n=n) == ERR_SHAPE
    for h, w in ((53, 37), (37, 54), (256, 256), (0, 53)):
        assert _bwd(d, h=h, w=w) == ERR_SHAPE
        assert b"the handle was created for 37x53 (the linear layer fixes it)" in L.cid_esd_last_error(d)
    # CID_ERR_WORKSPACE: the saved buffer, then the workspace; then CID_ERR_STATE
    sv_need = _size("cid_esd_saved_bytes", 2, H, W)[1]
    ws_need = _size("cid_esd_backward_workspace_bytes", 2, H, W)[1]
    assert _bwd(d, sv_bytes=sv_need - 1) == ERR_WORKSPACE
    assert L.cid_esd_last_error(d) == b"cid_esd_backward: saved buffer smaller than cid_esd_saved_bytes() or not 256-byte aligned"
    assert _bwd(d, sv=FAKE + 64, sv_bytes=sv_need) == ERR_WORKSPACE
    assert _bwd(d, sv_bytes=sv_need, ws_bytes=ws_need - 1) == ERR_WORKSPACE
    assert L.cid_esd_last_error(d) == (b"cid_esd_backward: workspace smaller than cid_esd_backward_workspace_bytes() or not 256-byte "
                                       b"aligned")
    assert _bwd(d, sv_bytes=sv_need, ws=FAKE + 128, ws_bytes=ws_need) == ERR_WORKSPACE
    assert _bwd(d, sv_bytes=sv_need, ws_bytes=ws_need) == ERR_STATE
    assert L.cid_esd_last_error(d) == b"cid_esd_backward: weights not uploaded"
    # nothing asked for is still checked the same way
    assert _bwd(d, g=Grads(), sv_bytes=sv_need, ws_bytes=ws_need) == ERR_STATE
    # the first of several faults is the one reported
    assert _bwd(d, x=None, n=0, sv_bytes=0) == ERR_INVALID
    assert _bwd(d, n=0, sv_bytes=0, ws_bytes=0) == ERR_SHAPE
    assert _bwd(d, sv_bytes=0, ws_bytes=0) == ERR_WORKSPACE and b"saved buffer" in L.cid_esd_last_error(d)


def test_pack_weights_device_argument_errors(handle):
    d = handle
    L = _lib.lib()
    ptrs = (ctypes.c_void_p * 10)(*[FAKE] * 10)
    assert L.cid_esd_pack_weights_device(None, ptrs, FAKE, None) == ERR_INVALID
    assert L.cid_esd_pack_weights_device(d, None, FAKE, None) == ERR_INVALID
    assert L.cid_esd_pack_weights_device(d, ptrs, None, None) == ERR_INVALID
    assert L.cid_esd_last_error(d) == b"cid_esd_pack_weights_device: null pointer"
    for i in range(10):
        for bad in (None, FAKE + 2):
            p = (ctypes.c_void_p * 10)(*[FAKE] * 10)
            p[i] = bad
            assert L.cid_esd_pack_weights_device(d, p, FAKE, None) == ERR_INVALID, (i, bad)
    assert L.cid_esd_pack_weights_device(d, ptrs, FAKE + 64, None) == ERR_WORKSPACE
    # none of these attached a blob
    assert _fwd(d, sv_bytes=1 << 40) == ERR_STATE


def test_autograd_flag_defaults_off_and_keeps_the_state_dict():
    shape = (3, H, W)
    sd = oracle.weights("trained", (H, W))
    plain, diff = ESRGANDiscriminator(shape), ESRGANDiscriminator(shape, autograd=True)
    assert plain._autograd is False and diff._autograd is True
    assert ESRGANDiscriminator(shape, False)._autograd is False
    assert list(plain.state_dict()) == list(diff.state_dict()) == list(oracle.StockESRGANDiscriminator(shape).state_dict())
    diff.load_state_dict(sd, strict=True)
    stock = oracle.StockESRGANDiscriminator(shape)
    stock.load_state_dict(diff.state_dict(), strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in stock.state_dict().items())
    assert list(diff.buffers()) == [] and [k for k, _ in diff.named_parameters()] == list(bwd.PARAMS)
    import inspect
    assert inspect.signature(load_esrgan_discriminator).parameters["autograd"].default is False
    assert inspect.signature(ESRGANDiscriminator.__init__).parameters["autograd"].default is False


@pytest.mark.parametrize("shape", bwd.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_reference_meets_its_conditions(shape):
    """What the bound e_hip <= max(1e-5, 2 * e_aten) rests on, so that a later change of inputs cannot weaken it silently: ATen fp32
    is within half the bound's first branch of float64 on every tensor (1.5e-6 ... 1.9e-6 measured: esrgan_disc_bwd_oracle.ATEN_ERR_MAX),
    not one of its mask units differs from float64's, no gradient tensor is smaller
    than 4.8e-5 (4.77e-5 before rounding) at its largest element, and the logits lie in (-1, 1.5)."""
    for kind in oracle.WSETS:
        for loss in bwd.LOSSES:
            r = bwd.reference(kind, shape, loss)
            worst = max(r["e_aten"].items(), key=lambda kv: kv[1])
            floor = min([float(g.abs().max()) for g in r["g64"].values()] + [float(r["gx64"].abs().max())])
            lo, hi = float(r["logits64"].min()), float(r["logits64"].max())
            print(f"{shape} {kind} {loss}: worst e_aten {worst[1]:.2e} ({worst[0]}), smallest max|g64| {floor:.2e}, logits [{lo:.3f}, {hi:.3f}]")
            assert worst[1] <= bwd.ATEN_ERR_MAX, worst
            assert r["aten_flips"] == 0
            assert floor >= bwd.GRAD_FLOOR
            assert bwd.LOGIT_RANGE[0] < lo and hi < bwd.LOGIT_RANGE[1]


def test_masked_reference_with_its_own_masks_is_plain_autograd():
    n, h, w = 2, H, W
    for kind in oracle.WSETS:
        for loss, target in bwd.LOSSES.items():
            r = bwd.reference(kind, (n, h, w), loss)
            stock = oracle.StockESRGANDiscriminator((3, h, w)).double()
            stock.load_state_dict(oracle.cast(r["sd"], torch.float64), strict=True)
            x = r["x"].double().requires_grad_(True)
            out = stock(x)
            torch.nn.BCEWithLogitsLoss()(out, torch.full_like(out, target)).backward()
            assert torch.equal(out.detach(), r["logits64"]) or float((out.detach() - r["logits64"]).abs().max()) <= 1e-14
            for k, p in stock.named_parameters():
                assert float((p.grad - r["g64"][k]).abs().max()) <= 1e-13 * float(r["g64"][k].abs().max()), k
            assert float((x.grad - r["gx64"]).abs().max()) <= 1e-13 * float(r["gx64"].abs().max())
            # and other masks change it: the masks are really used
            flipped = [~m for m in r["masks64"]]
            g2, _ = bwd.ref_for_masks(r, loss, flipped)
            assert float((g2["conv1.weight"] - r["g64"]["conv1.weight"]).abs().max()) > 0
