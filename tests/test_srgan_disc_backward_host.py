"""The backward pass of the SRGAN trainer's discriminator without a GPU: the host-side argument checks of cid_srd_saved_bytes,
cid_srd_forward_saved, cid_srd_backward_workspace_bytes, cid_srd_backward, cid_srd_pack_weights_device and cid_srd_saved_masks
(include/cid.h) in their documented order, the saved-bytes formula, and the `autograd` argument of the Python layer.  Every call
below hands the library pointers that are never dereferenced: it must fail on the host, before any launch.  The GPU tests are in
tests/test_srgan_disc_backward.py."""
import ctypes
import inspect

from celebrity_image_denoiser_amd import _lib
from test_srgan_disc_host import ERR_INVALID, ERR_SHAPE, ERR_STATE, ERR_WORKSPACE, FAKE, _bn_array

PARAMS = [f"model.{i}.{k}" for i in (0, 2, 3, 5, 6, 8, 9, 11, 12, 15, 17) for k in ("weight", "bias")]   # nn.Module.parameters() order


class Grads(ctypes.Structure):
    """cid_srd_grads (include/cid.h)."""
    _fields_ = [("w", ctypes.c_void_p * 7), ("b", ctypes.c_void_p * 7), ("gamma", ctypes.c_void_p * 4), ("beta", ctypes.c_void_p * 4),
                ("input", ctypes.c_void_p)]


def _side(s):
    return (s - 1) // 2 + 1


def expected_saved(n, h, w, training):
    """The formula of include/cid.h (cid_srd_saved_bytes)."""
    a256 = lambda v: (v + 255) // 256 * 256   # noqa: E731
    h2, w2 = _side(h), _side(w)
    h4, w4 = _side(h2), _side(w2)
    total = sum(a256(4 * n * c * hh * ww) for c, hh, ww in ((64, h, w), (64, h2, w2), (128, h2, w2), (128, h4, w4), (256, h4, w4)))
    total += a256(4 * 4 * 256 * 2) + a256(8 * 4 * 256 * 2)
    total += a256(8 * n * 256) + a256(8 * n * 512)
    if training:
        for (ho, wo, th, c) in ((h2, w2, 16, 64), (h2, w2, 8, 128), (h4, w4, 8, 128), (h4, w4, 8, 256)):
            total += a256(8 * c * 2 * n * -(-ho // th) * -(-wo // 16))
    return total


def test_saved_bytes_equals_the_documented_formula():
    L = _lib.lib()
    size = ctypes.c_size_t()
    for shape in ((16, 256, 256), (3, 37, 53), (2, 1, 1)):
        for training in (0, 1):
            assert L.cid_srd_saved_bytes(*shape, training, ctypes.byref(size)) == 0
            assert size.value == expected_saved(*shape, training), (shape, training)
    # the five tensors do not overlap: more than the forward's two regions
    ws = ctypes.c_size_t()
    assert L.cid_srd_workspace_bytes(16, 256, 256, 1, ctypes.byref(ws)) == 0
    assert L.cid_srd_saved_bytes(16, 256, 256, 1, ctypes.byref(size)) == 0 and size.value > ws.value
    assert size.value >= 4 * 16 * (64 * 256 * 256 + 64 * 128 * 128 + 128 * 128 * 128 + 128 * 64 * 64 + 256 * 64 * 64)


def test_backward_argument_errors_come_before_any_launch():
    L = _lib.lib()
    d = ctypes.c_void_p()
    assert L.cid_srd_create(ctypes.byref(d)) == 0
    try:
        fake = FAKE
        ok_bn = _bn_array()
        ok_g = Grads()
        ok_g.w[0] = fake
        ok_g.input = fake
        size = ctypes.c_size_t()

        # cid_srd_saved_bytes / cid_srd_backward_workspace_bytes
        for fn in (L.cid_srd_saved_bytes, L.cid_srd_backward_workspace_bytes):
            assert fn(2, 8, 8, 0, None) == ERR_INVALID
            assert fn(2, 8, 8, 2, ctypes.byref(size)) == ERR_INVALID
            for n, h, w in ((0, 8, 8), (2, 0, 8), (2, 8, 0), (1, 65536, 32768)):
                assert fn(n, h, w, 0, ctypes.byref(size)) == ERR_SHAPE
            for h, w in ((1, 1), (4, 4), (3, 2)):
                assert fn(1, h, w, 1, ctypes.byref(size)) == ERR_SHAPE      # one value per channel in train mode
            assert fn(1, 4, 4, 0, ctypes.byref(size)) == 0 and size.value > 0
            assert fn(2, 1, 1, 1, ctypes.byref(size)) == 0 and size.value > 0

        # cid_srd_forward_saved: the forward's checks, the saved buffer in the workspace's place
        def fwd(n=2, h=16, w=16, training=0, bn=ok_bn, x=fake, fmt=0, out=fake, sv=fake, sv_bytes=1 << 40):
            return L.cid_srd_forward_saved(d, x, fmt, out, n, h, w, bn, training, sv, sv_bytes, None)

        assert L.cid_srd_forward_saved(None, fake, 0, fake, 2, 16, 16, ok_bn, 0, fake, 1 << 40, None) == ERR_INVALID
        no_rv = _bn_array()
        no_rv[3].running_var = None            # the fourth BatchNorm is checked too
        for kw in (dict(x=None), dict(out=None), dict(bn=None), dict(sv=None), dict(fmt=7), dict(x=fake + 1), dict(out=fake + 2),
                   dict(training=2), dict(bn=_bn_array(eps=float("nan"))), dict(bn=_bn_array(momentum=-0.5), training=1),
                   dict(bn=_bn_array(nbt=False), training=1), dict(bn=no_rv)):
            assert fwd(**kw) == ERR_INVALID, kw
        assert L.cid_srd_last_error(d) == b"cid_srd_forward_saved: null BatchNorm pointer"
        assert fwd(n=0) == ERR_SHAPE and fwd(n=1, h=4, w=4, training=1) == ERR_SHAPE
        assert L.cid_srd_last_error(d) == b"Expected more than 1 value per channel when training"
        assert fwd(x=None, n=0, sv_bytes=0) == ERR_INVALID and fwd(n=0, sv_bytes=0) == ERR_SHAPE      # the documented order
        for training in (0, 1):
            need = expected_saved(3, 37, 53, training)
            assert fwd(n=3, h=37, w=53, training=training, sv_bytes=need - 1) == ERR_WORKSPACE
            assert b"cid_srd_saved_bytes" in L.cid_srd_last_error(d)
            assert fwd(n=3, h=37, w=53, training=training, sv=fake + 16, sv_bytes=need) == ERR_WORKSPACE
            assert fwd(n=3, h=37, w=53, training=training, sv_bytes=need) == ERR_STATE     # no weights: still before any launch

        # cid_srd_backward
        def bwd(n=3, h=37, w=53, training=0, bn=ok_bn, x=fake, fmt=0, gp=fake, sv=fake, sv_bytes=1 << 40, g=ok_g, ws=fake, ws_bytes=1 << 40):
            return L.cid_srd_backward(d, x, fmt, gp, n, h, w, bn, training, sv, sv_bytes, ctypes.byref(g) if g is not None else None,
                                      ws, ws_bytes, None)

        assert L.cid_srd_backward(None, fake, 0, fake, 3, 37, 53, ok_bn, 0, fake, 1 << 40, ctypes.byref(ok_g), fake, 1 << 40, None) == ERR_INVALID
        bad = []
        for field, i in (("b", 3), ("w", 6), ("b", 5), ("gamma", 3), ("beta", 0)):
            g = Grads()
            getattr(g, field)[i] = fake + 2
            bad.append(g)
        bad_in = Grads()
        bad_in.input = fake + 1
        no_gamma = _bn_array()
        no_gamma[3].gamma = None
        for kw in [dict(x=None), dict(gp=None), dict(bn=None), dict(sv=None), dict(g=None), dict(ws=None), dict(fmt=7), dict(x=fake + 1),
                   dict(gp=fake + 2), dict(training=2), dict(bn=no_gamma), dict(g=bad_in), dict(fmt=1)] + [dict(g=g) for g in bad]:
            assert bwd(**kw) == ERR_INVALID, kw                  # fmt=1: uint8 input with g.input
        assert bwd(fmt=1) == ERR_INVALID and b"uint8 input has no gradient" in L.cid_srd_last_error(d)
        u8_g = Grads()
        u8_g.w[4] = fake
        assert bwd(fmt=1, g=u8_g) == ERR_STATE                   # uint8 input without an input gradient is accepted
        assert bwd(g=Grads()) == ERR_STATE                       # nothing asked for is not an error of its own
        for n, h, w in ((0, 8, 8), (2, 0, 8), (2, 8, 0), (1, 65536, 32768)):
            assert bwd(n=n, h=h, w=w) == ERR_SHAPE
        assert bwd(n=1, h=4, w=4, training=1) == ERR_SHAPE
        # the order: INVALID before SHAPE before WORKSPACE before STATE
        assert bwd(x=None, n=0, sv_bytes=0) == ERR_INVALID and bwd(training=3, n=0) == ERR_INVALID
        assert bwd(n=0, sv_bytes=0, ws_bytes=0) == ERR_SHAPE and bwd(sv_bytes=0) == ERR_WORKSPACE
        for training in (0, 1):
            need_s = expected_saved(3, 37, 53, training)
            assert L.cid_srd_backward_workspace_bytes(3, 37, 53, training, ctypes.byref(size)) == 0
            need_w = size.value
            assert bwd(training=training, sv_bytes=need_s - 1) == ERR_WORKSPACE
            assert b"cid_srd_saved_bytes" in L.cid_srd_last_error(d)
            assert bwd(training=training, sv=fake + 16, sv_bytes=need_s) == ERR_WORKSPACE
            assert bwd(training=training, sv_bytes=need_s, ws_bytes=need_w - 1) == ERR_WORKSPACE
            assert b"cid_srd_backward_workspace_bytes" in L.cid_srd_last_error(d)
            assert bwd(training=training, sv_bytes=need_s, ws=fake + 16, ws_bytes=need_w) == ERR_WORKSPACE
            assert bwd(training=training, sv_bytes=need_s, ws_bytes=need_w) == ERR_STATE
            assert L.cid_srd_last_error(d) == b"cid_srd_backward: weights not uploaded"
        # the workspace holds at least the two gradient tensors the data-gradient chain passes on, and model.11's data gradient
        assert L.cid_srd_backward_workspace_bytes(3, 37, 53, 0, ctypes.byref(size)) == 0
        assert size.value >= 3 * 64 * 37 * 53 * 4 + 3 * 64 * 19 * 27 * 4
        assert L.cid_srd_backward_workspace_bytes(2, 1, 1, 0, ctypes.byref(size)) == 0 and size.value >= 2 * 128 * 4 + 2 * 128 * 4

        # cid_srd_pack_weights_device
        ptrs = (ctypes.c_void_p * 14)(*([fake] * 14))
        assert L.cid_srd_pack_weights_device(None, ptrs, fake, None) == ERR_INVALID
        assert L.cid_srd_pack_weights_device(d, None, fake, None) == ERR_INVALID
        assert L.cid_srd_pack_weights_device(d, ptrs, None, None) == ERR_INVALID
        assert L.cid_srd_pack_weights_device(d, ptrs, fake + 16, None) == ERR_WORKSPACE
        for i in (7, 13):
            ptrs[i] = None
            assert L.cid_srd_pack_weights_device(d, ptrs, fake, None) == ERR_INVALID
            ptrs[i] = fake + 2
            assert L.cid_srd_pack_weights_device(d, ptrs, fake, None) == ERR_INVALID
            ptrs[i] = fake

        # cid_srd_saved_masks
        mk = (ctypes.c_void_p * 6)(*([fake] * 6))
        assert L.cid_srd_saved_masks(None, 1 << 40, 2, 8, 8, 0, mk, None) == ERR_INVALID
        assert L.cid_srd_saved_masks(fake, 1 << 40, 2, 8, 8, 0, None, None) == ERR_INVALID
        assert L.cid_srd_saved_masks(fake, 1 << 40, 2, 8, 8, 2, mk, None) == ERR_INVALID
        assert L.cid_srd_saved_masks(fake, 1 << 40, 0, 8, 8, 0, mk, None) == ERR_SHAPE
        assert L.cid_srd_saved_masks(fake, 1 << 40, 1, 4, 4, 1, mk, None) == ERR_SHAPE
        assert L.cid_srd_saved_masks(fake, expected_saved(2, 8, 8, 0) - 1, 2, 8, 8, 0, mk, None) == ERR_WORKSPACE
        assert L.cid_srd_saved_masks(fake + 16, 1 << 40, 2, 8, 8, 0, mk, None) == ERR_WORKSPACE
        for i in (2, 5):
            mk[i] = None
            assert L.cid_srd_saved_masks(fake, 1 << 40, 2, 8, 8, 0, mk, None) == ERR_INVALID
            mk[i] = fake
    finally:
        L.cid_srd_destroy(d)


def test_autograd_flag_defaults_off_and_keeps_the_structure():
    from celebrity_image_denoiser_amd.srgan_disc import SRGANDiscriminator, load_srgan_discriminator

    assert SRGANDiscriminator()._autograd is False and SRGANDiscriminator(autograd=True)._autograd is True
    assert [k for k, _ in SRGANDiscriminator(autograd=True).named_parameters()] == PARAMS
    assert [k for k, _ in SRGANDiscriminator().named_parameters()] == PARAMS
    assert list(SRGANDiscriminator(autograd=True).state_dict()) == list(SRGANDiscriminator().state_dict())
    assert inspect.signature(load_srgan_discriminator).parameters["autograd"].default is False
    assert inspect.signature(SRGANDiscriminator.__init__).parameters["autograd"].default is False
