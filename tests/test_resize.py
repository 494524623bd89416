"""GPU checks of the bicubic resize (resize.resize / cid_resize): every byte against the numpy restatement
(synth.resize_bicubic_np, itself held against Pillow in test_resize_host.py), the float form against the forward's uint8 input
arithmetic, batch independence, guard bytes around the destination, stream-asynchrony, the ragged-list form and the harness."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth

pytestmark = pytest.mark.gpu

# (Hs, Ws, Hd, Wd): tests/golden/make_resize_golden.py's shapes (inputs from its fixtures) and the sized shape (N = 2, generated here)
SHAPES = [(218, 178, 256, 256), (37, 53, 16, 16), (16, 16, 37, 53), (5, 7, 16, 12), (3, 3, 8, 8), (300, 200, 131, 200),
          (256, 100, 256, 64), (256, 256, 256, 256), (1, 1, 4, 4), (64, 64, 1, 1), (512, 192, 8, 3), (300, 250, 131, 77)]
BIG = (1024, 1024, 256, 256)
DEV = "cuda:0"
GUARD = 64


def _id(s):
    return f"{s[0]}x{s[1]}_{s[2]}x{s[3]}"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("this test needs a GPU (run the suite with -m 'not gpu' on a machine without one)")


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(inputs uint8 [N,Hs,Ws,3], the restatement's result) of a shape, computed once and shared; both are only read."""
    hs, ws, hd, wd = shape
    if shape == BIG:
        noise = np.random.default_rng(1024).integers(0, 256, (hs, ws, 3), dtype=np.uint8)
        yy, xx = np.mgrid[0:hs, 0:ws]
        checker = np.repeat(((((yy // 3) + (xx // 3)) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
        x = np.stack([noise, checker])
    else:
        golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        x = np.load(os.path.join(golden, f"resize_{_id(shape)}.npz"))["x"]       # noise, checkerboard of period 3, constant 255
    ref = synth.resize_bicubic_np(x, (wd, hd))
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


def _normalized(u8_nhwc):
    """The forward's uint8 input arithmetic in numpy float32: (u/255 - 0.5)/0.5, NCHW."""
    f = u8_nhwc.astype(np.float32)
    return np.ascontiguousarray((((f / np.float32(255.0)) - np.float32(0.5)) / np.float32(0.5)).transpose(0, 3, 1, 2))


@pytest.mark.parametrize("shape", SHAPES + [BIG], ids=_id)
def test_resize_equals_the_restatement(shape):
    _need_gpu()
    import celebrity_image_denoiser_amd as cid

    hs, ws, hd, wd = shape
    x, ref = _case(shape)
    xd = torch.from_numpy(np.array(x)).to(DEV)
    got = cid.resize(xd, (wd, hd), out="u8")
    assert got.dtype == torch.uint8 and tuple(got.shape) == (x.shape[0], hd, wd, 3) and got.is_contiguous()
    got = got.cpu().numpy()
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} of {ref.size} bytes differ"
    if shape != BIG:
        assert (got[2] == 255).all()                                     # the constant image
    f = cid.resize(xd, (wd, hd), out="f32")
    assert f.dtype == torch.float32 and tuple(f.shape) == (x.shape[0], 3, hd, wd)
    assert np.array_equal(f.cpu().numpy().view(np.uint32), _normalized(ref).view(np.uint32))
    assert torch.equal(cid.resize(xd, (wd, hd)), torch.from_numpy(got).to(DEV))      # the same plan again: the same bytes


def test_float_result_feeds_the_forward_like_the_uint8_result(weight_sets):
    _need_gpu()
    import celebrity_image_denoiser_amd as cid

    x, _ = _case((37, 53, 16, 16))
    xd = torch.from_numpy(np.array(x)).to(DEV)
    G = cid.load(weight_sets["hot"], device=DEV, strict=True)
    y_f = G(cid.resize(xd, (16, 16), out="f32"))
    y_u = G.forward_u8(cid.resize(xd, (16, 16)), out_u8=False)
    assert torch.equal(y_f, y_u)


@pytest.mark.parametrize("shape", [(300, 250, 131, 77), (218, 178, 256, 256), (300, 200, 131, 200), (256, 100, 256, 64)], ids=_id)
def test_result_does_not_depend_on_the_batch(shape):
    _need_gpu()
    import celebrity_image_denoiser_amd as cid

    hs, ws, hd, wd = shape
    x, _ = _case(shape)
    xd = torch.from_numpy(np.array(x)).to(DEV)
    full = cid.resize(xd, (wd, hd))
    for k in (0, 2):
        assert torch.equal(cid.resize(xd[k:k + 1].contiguous(), (wd, hd))[0], full[k])


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_nothing_is_written_outside_the_destination(shape):
    """The destination sits between 64 guard bytes of 0xA5 on each side; the source is the tail of its allocation."""
    _need_gpu()
    from celebrity_image_denoiser_amd import resize as rz

    hs, ws, hd, wd = shape
    x, ref = _case(shape)
    n = x.shape[0]
    xd = torch.from_numpy(np.array(x)).to(DEV)
    plan = rz._plan(xd.device, hs, ws, hd, wd)
    stream = torch.cuda.current_stream(xd.device).cuda_stream
    for fmt, elem in ((_lib.CID_FMT_U8_NHWC, 1), (_lib.CID_FMT_F32_NCHW, 4)):
        nbytes = n * hd * wd * 3 * elem
        buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        assert _lib.lib().cid_resize(plan, xd.data_ptr(), buf.data_ptr() + GUARD, fmt, n, stream) == 0
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:GUARD] == 0xA5).all() and (host[GUARD + nbytes:] == 0xA5).all()
        body = host[GUARD:GUARD + nbytes]
        if elem == 1:
            assert np.array_equal(body.reshape(ref.shape), ref)
        else:
            assert np.array_equal(body.view(np.uint32), _normalized(ref).reshape(-1).view(np.uint32))


def test_resize_makes_no_host_synchronisation_once_its_plan_is_cached():
    _need_gpu()
    import celebrity_image_denoiser_amd as cid

    x, ref = _case((37, 53, 16, 16))
    xd = torch.from_numpy(np.array(x)).to(DEV)
    cid.resize(xd, (16, 16))                                             # builds and caches the plan (may synchronise)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = cid.resize(xd, (16, 16))
        b = cid.resize(xd, (16, 16), out="f32")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(a.cpu().numpy(), ref) and tuple(b.shape) == (3, 3, 16, 16)


def test_resize_images_keeps_list_order_over_mixed_sizes():
    _need_gpu()
    import celebrity_image_denoiser_amd as cid

    rng = np.random.default_rng(77)
    sizes = [(20, 30), (33, 17), (20, 30), (16, 16)]                     # two 20x30, one 33x17, one 16x16 (a copy)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    got = cid.resize_images(images, (16, 16), DEV)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (4, 16, 16, 3) and got.is_cuda
    for k, im in enumerate(images):
        assert np.array_equal(got[k].cpu().numpy(), synth.resize_bicubic_np(im, (16, 16))), k
    mixed = [images[0], torch.from_numpy(images[1]), images[2], torch.from_numpy(images[3])]
    assert torch.equal(cid.resize_images(mixed, (16, 16), DEV), got)


def test_python_surface_errors_on_the_device():
    _need_gpu()
    import celebrity_image_denoiser_amd as cid

    xd = torch.zeros(1, 130, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="factor"):
        cid.resize(xd, (8, 2))                                           # 130 rows -> 2: factor 65
    with pytest.raises(RuntimeError, match="contiguous"):
        cid.resize(torch.zeros(1, 8, 16, 3, dtype=torch.uint8, device=DEV)[:, :, ::2], (4, 4))


def test_harness_device_resize_writes_the_same_files(tmp_path, weight_sets):
    """enhance_images(resize="device") against resize="host": byte-identical PNGs (the existing harness test's recipe at 32x48)."""
    _need_gpu()
    from PIL import Image

    import celebrity_image_denoiser_amd as cid

    src, dst_h, dst_d = tmp_path / "testNoise", tmp_path / "host", tmp_path / "device"
    src.mkdir()
    _, _, noisy = synth.make_batch(3, 40, 52, first_index=8000)
    for k in range(3):
        Image.fromarray(noisy[k]).save(src / f"img{k}.png")
    m = cid.load(weight_sets["hot"], device=DEV, strict=True)
    wh = cid.enhance_images(None, str(src), str(dst_h), image_size=(32, 48), batch_size=2, model=m)
    wd = cid.enhance_images(None, str(src), str(dst_d), image_size=(32, 48), batch_size=2, model=m, resize="device")
    assert sorted(map(os.path.basename, wh)) == sorted(map(os.path.basename, wd)) == [f"img{k}.png" for k in range(3)]
    for k in range(3):
        assert (dst_h / f"img{k}.png").read_bytes() == (dst_d / f"img{k}.png").read_bytes(), k
        assert np.asarray(Image.open(dst_d / f"img{k}.png")).shape == (48, 32, 3)
