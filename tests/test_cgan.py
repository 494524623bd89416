"""The server's CGANGenerator (reference backend/app.py:105-143, the label branch) on the GPU: cid_cg_forward / cid_cg_latent
(include/cid.h) and cgan.py.

The reference for error is tests/cgan_oracle.py in float64 (held to the fixtures recorded from the reference class by
test_cgan_host.py); where a fixture exists the result is compared with it as well.  The bound is the project's per-stage rule,
max|delta| <= 1e-5 * max(1, max|ref64|) per tensor: the reference's own ATen fp32 stands at 0.1-5.1e-7 of that scale on the "default"
weights and 1.4-6.9e-7 on "hot" (tests/golden/cgan_stats.json), a margin of 14x or more.  The linear's output, the three transposed
convolutions' outputs (each after BatchNorm and ReLU) are compared through cid_cg_stage_view and the sums before tanh through
CID_CG_RAW, so that an error is told from the stage after it.  tanh saturates, so `out` is held to the bound of the sums before it
(tanh is 1-Lipschitz) and the tanh step alone to 1e-6 against float64 tanh of the GPU's own sums.

The spatial sizes are fixed by the model, so the shapes are batch sizes: 1 (a single column of the linear's 16-image MFMA tile),
2, 3 and 5 (odd tails), 19 (more than one column tile with a partial last one)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth
from celebrity_image_denoiser_amd.cgan import CGANGenerator, generate, generate_u8, latent, load_cgan

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cgan_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BATCHES = [1, 2, 3, 5, 19]
FIXTURES = {1, 3}
SEED = 777

_MODELS, _REFS = {}, {}


def model_of(wset, n_classes=10):
    if (wset, n_classes) not in _MODELS:
        _MODELS[(wset, n_classes)] = load_cgan(synth.make_cgan_state_dict(wset, n_classes), n_classes=n_classes, device=DEV, strict=True)
    return _MODELS[(wset, n_classes)]


def fixture_of(wset, n):
    return np.load(os.path.join(GOLDEN, f"cgan_{wset}_n{n}.npz")) if n in FIXTURES else None


def labels_of(n, n_classes=10):
    """Covers 0 and n_classes - 1 from N = 2 on; N = 1 takes the last class."""
    return [(n_classes - 1, 0, 3 % n_classes, 3 % n_classes, 1)[i % 5] for i in range(n)]


def inputs_of(wset, n, n_classes=10):
    """(z fp32 [N,100], labels): the fixture's where one exists (n_classes 10), else the latent's restatement and labels_of."""
    fx = fixture_of(wset, n) if n_classes == 10 else None
    if fx is not None:
        return fx["z"], [int(v) for v in fx["labels"]]
    return synth.cgan_latent_np(n, SEED, 100 * n), labels_of(n, n_classes)


def reference(wset, n, n_classes=10):
    """The float64 oracle of one case: computed once, shared, never modified."""
    key = (wset, n, n_classes)
    if key not in _REFS:
        z, labels = inputs_of(wset, n, n_classes)
        ref = cgan_oracle.forward(synth.make_cgan_state_dict(wset, n_classes), z, labels)
        for v in ref.values():
            v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def check(name, got, ref64, fixture=None, bound=None):
    bound = cgan_oracle.bound(ref64) if bound is None else bound
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    print(f"{name}: max|delta| {err:.3e}, bound {bound:.3e} (margin {bound / max(err, 1e-300):.1f}x), max|ref| {np.abs(ref64).max():.4g}")
    assert got.shape == ref64.shape, name
    assert np.isfinite(got).all(), name
    assert err <= bound, (name, err, bound)
    if fixture is not None:
        errf = float(np.abs(got.astype(np.float64) - fixture.astype(np.float64)).max())
        print(f"{name}: against the fixture {errf:.3e}")
        assert errf <= bound, (name, errf, bound)


def run_parity(wset, n, n_classes=10):
    m = model_of(wset, n_classes)
    z, labels = inputs_of(wset, n, n_classes)
    ref = reference(wset, n, n_classes)
    fx = fixture_of(wset, n) if n_classes == 10 else None
    zd = torch.from_numpy(z).to(DEV)
    lab = torch.tensor(labels, dtype=torch.int64, device=DEV)
    pre = m(zd, lab, raw=True)
    out = m(zd.view(n, 100, 1, 1), labels)                       # the server's latent shape, host labels
    stages = {k: m.stage(k, n) for k in ("l1", "t1", "t2", "t3")}
    torch.cuda.synchronize()
    assert out.shape == (n, 3, 64, 64) and out.dtype == torch.float32 and pre.shape == out.shape
    for k in ("l1", "t1", "t2", "t3"):
        check(k, stages[k].cpu().numpy(), ref[k], fx[k] if fx is not None and k in fx.files else None)
    pre, out = pre.cpu().numpy(), out.cpu().numpy()
    check("pre", pre, ref["pre"], fx["pre"] if fx is not None and "pre" in fx.files else None)
    # tanh is 1-Lipschitz and saturates: the output inherits the bound of the sums before it
    check("out", out, ref["out"], None if fx is None else fx["out"], bound=cgan_oracle.bound(ref["pre"]))
    tanh_err = float(np.abs(out.astype(np.float64) - np.tanh(pre.astype(np.float64))).max())
    print(f"tanh step alone: max|tanhf(pre) - tanh64(pre)| {tanh_err:.3e} over |pre| <= {np.abs(pre).max():.4g} (bound 1e-6)")
    assert tanh_err <= 1e-6
    assert np.abs(out).max() <= 1.0


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("wset", ["default", "hot"])
def test_parity_with_the_float64_oracle(wset, n):
    run_parity(wset, n)


@pytest.mark.parametrize("wset", ["default", "hot"])
def test_parity_with_three_classes(wset):
    assert set(labels_of(5, 3)) >= {0, 2}
    run_parity(wset, 5, n_classes=3)


def u8_check(got, want, wset):
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    frac = float((d != 0).mean())
    sat = float(((want == 0) | (want == 255)).mean())
    print(f"uint8 {wset}: max|delta| {d.max()}, differing {frac:.2e}, expected bytes at 0 or 255 {sat:.3f}")
    assert got.shape == want.shape and got.dtype == want.dtype
    assert d.max() <= 1 and frac <= 1e-3            # the cap of test_gpu_parity.py
    if wset == "hot":
        assert 0.05 <= sat <= 0.90                  # the clamp is exercised and is not all there is
    else:
        assert sat == 0                             # every byte is mid-range


@pytest.mark.parametrize("wset", ["default", "hot"])
def test_uint8_server_path_against_the_server_fixture(wset):
    fx = np.load(os.path.join(GOLDEN, f"cgan_{wset}_u8_n2.npz"))
    got = generate_u8(model_of(wset), [int(v) for v in fx["labels"]], z=torch.from_numpy(fx["z"]).to(DEV))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 64, 64, 3)
    u8_check(got.cpu().numpy(), fx["out_u8"], wset)


@pytest.mark.parametrize("wset", ["default", "hot"])
def test_uint8_server_path_against_the_oracle(wset):
    z, labels = inputs_of(wset, 5)
    got = generate_u8(model_of(wset), labels, z=torch.from_numpy(z).to(DEV))
    u8_check(got.cpu().numpy(), cgan_oracle.to_u8(reference(wset, 5)["out"]), wset)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_an_image_alone_and_in_a_batch_and_two_calls_give_identical_bits():
    m = model_of("hot")
    z, labels = inputs_of("hot", 19)
    zd, lab = torch.from_numpy(z).to(DEV), torch.tensor(labels, device=DEV)
    for kw in ({}, {"raw": True}, {"out_dtype": torch.uint8}):
        full = m(zd, lab, **kw)
        assert torch.equal(_bits(full), _bits(m(zd, lab, **kw)))
        for i in (0, 1, 15, 16, 18):                  # both sides of the linear's column-tile edge, and the last
            alone = m(zd[i:i + 1].contiguous(), lab[i:i + 1].contiguous(), **kw)
            assert torch.equal(_bits(alone), _bits(full[i:i + 1])), (i, kw)
        # the same image at every position of a batch of three
        for pos in range(3):
            idx = [4, 5, 6]
            idx[pos] = 17
            part = m(zd[idx].contiguous(), lab[idx].contiguous(), **kw)
            assert torch.equal(_bits(part[pos:pos + 1]), _bits(full[17:18])), (pos, kw)


def test_latent_matches_its_restatement():
    n, seed, first = 37, 12345, 11
    got = latent(n, seed, first, device=DEV)
    assert got.shape == (n, 100) and got.dtype == torch.float32
    want = synth.cgan_latent_np(n, seed, first)
    g = got.cpu().numpy()
    d = np.abs(g.astype(np.float64) - want.astype(np.float64))
    print(f"latent: {int((g != want).sum())} of {g.size} elements differ from the restatement; worst {float((d / np.spacing(np.abs(want))).max()):.2f} ulp")
    assert np.isfinite(g).all()
    assert (d <= np.spacing(np.abs(want))).all()      # both are fp32 roundings of doubles a few double ulps apart
    for k in (0, 5, 36):                              # image k alone, first_index shifted: identical bits
        assert torch.equal(_bits(latent(1, seed, first + k, device=DEV)), _bits(got[k:k + 1]))
        assert torch.equal(_bits(latent(1, seed + first + k, 0, device=DEV)), _bits(got[k:k + 1]))
    assert torch.equal(_bits(latent(4, seed, first + 30, device=DEV)), _bits(got[30:34]))


def test_generate_from_a_seed_equals_the_forward_of_its_latent():
    m = model_of("hot")
    labels = labels_of(5)
    a = generate(m, labels, seed=31)
    b = m(latent(5, 31, device=DEV), labels)
    assert a.shape == (5, 3, 64, 64) and torch.equal(_bits(a), _bits(b))
    assert torch.equal(generate_u8(m, labels, seed=31), m(latent(5, 31, device=DEV), labels, out_dtype=torch.uint8))
    assert torch.equal(_bits(generate(m, labels, z=latent(5, 31, device=DEV))), _bits(a))
    with pytest.raises(ValueError, match="exactly one"):
        generate(m, labels)
    with pytest.raises(ValueError, match="exactly one"):
        generate(m, labels, seed=1, z=latent(5, 31, device=DEV))


@pytest.mark.parametrize("bad", [-1, 10])
def test_an_invalid_device_label_gives_nan_at_its_position_only(bad):
    """An input check, not a fault: the kernel reads row 0 of the table for that image and replaces its outputs."""
    m = model_of("hot")
    z, labels = inputs_of("hot", 5)
    zd = torch.from_numpy(z).to(DEV)
    good = m(zd, torch.tensor(labels, device=DEV))
    good_u8 = m(zd, torch.tensor(labels, device=DEV), out_dtype=torch.uint8)
    for pos in (0, 2, 4):
        lab = list(labels)
        lab[pos] = bad
        got = m(zd, torch.tensor(lab, device=DEV))
        got_u8 = m(zd, torch.tensor(lab, device=DEV), out_dtype=torch.uint8)
        raw = m(zd, torch.tensor(lab, device=DEV), raw=True)
        assert bool(torch.isnan(got[pos]).all()) and bool(torch.isnan(raw[pos]).all()) and bool((got_u8[pos] == 0).all())
        keep = [i for i in range(5) if i != pos]
        assert torch.equal(_bits(got[keep]), _bits(good[keep])) and torch.equal(got_u8[keep], good_u8[keep])
        with pytest.raises(IndexError):
            m(zd, lab)                                # the same labels on the host are range-checked
        with pytest.raises(IndexError):
            m(zd, torch.tensor(lab))


GUARD = 4096


def _guarded(nbytes, fill):
    buf = torch.full((nbytes + 2 * GUARD + 256,), fill, dtype=torch.uint8, device=DEV)
    start = (-buf.data_ptr() - GUARD) % 256 + GUARD      # 256-byte aligned, at least one guard past the start
    return buf, start


@pytest.mark.parametrize("out_u8", [False, True], ids=["f32", "u8"])
def test_nan_prefill_changes_nothing_and_guard_regions_stay_untouched(out_u8):
    """Workspace and output start as NaN bits (0xFF bytes), with 4 KiB guard regions of 0xA5 before and after each: the result is
    finite and equal to the module's, and no guard byte changes (no read of an unwritten word reaches a result, no write leaves
    its buffer)."""
    m = model_of("hot")
    n = 3
    z, labels = inputs_of("hot", n)
    zd, lab = torch.from_numpy(z).to(DEV), torch.tensor(labels, device=DEV)
    want = m(zd, lab, out_dtype=torch.uint8 if out_u8 else torch.float32)
    L = _lib.lib()
    need = ctypes.c_size_t()
    assert L.cid_cg_workspace_bytes(n, ctypes.byref(need)) == 0
    out_bytes = n * 64 * 64 * 3 * (1 if out_u8 else 4)
    bufs = []
    for nbytes in (need.value, out_bytes):
        buf, start = _guarded(nbytes, 0xA5)
        buf[start:start + nbytes] = 0xFF
        bufs.append((buf, start, nbytes))
    (wsb, ws0, _), (ob, o0, _) = bufs
    stream = torch.cuda.current_stream().cuda_stream
    rc = L.cid_cg_forward(m._cid, zd.data_ptr(), lab.data_ptr(), ob.data_ptr() + o0,
                          _lib.CID_FMT_U8_NHWC if out_u8 else _lib.CID_FMT_F32_NCHW, n, 0, wsb.data_ptr() + ws0, need.value, stream)
    assert rc == 0, L.cid_cg_last_error(m._cid)
    torch.cuda.synchronize()
    got = ob[o0:o0 + out_bytes].clone()
    got = got.view(n, 64, 64, 3) if out_u8 else got.view(torch.float32).view(n, 3, 64, 64)
    if not out_u8:
        assert torch.isfinite(got).all()
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    for buf, start, nbytes in bufs:
        assert bool((buf[:start] == 0xA5).all()) and bool((buf[start + nbytes:] == 0xA5).all())


def test_errors_raised():
    m = model_of("default")
    z = torch.zeros(2, 100, device=DEV)
    with pytest.raises(NotImplementedError, match="app.py:139-143"):
        m(z, torch.zeros(2, 3, 64, 64, device=DEV))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        m(z.cpu(), [0, 1])
    with pytest.raises(RuntimeError, match="latent of shape"):
        m(torch.zeros(2, 99, device=DEV), [0, 1])
    with pytest.raises(RuntimeError, match="latent of shape"):
        m(torch.zeros(2, 100, 1, device=DEV), [0, 1])
    with pytest.raises(RuntimeError, match="labels"):
        m(z, [0, 1, 2])
    with pytest.raises(ValueError, match="raw=True"):
        m(z, [0, 1], out_dtype=torch.uint8, raw=True)
    with pytest.raises(ValueError):
        m(z, None)
    with pytest.raises(ValueError, match="hard-codes"):
        CGANGenerator(10, latent_dim=7)
    t = CGANGenerator(3).to(DEV)
    assert t.training
    with pytest.raises(RuntimeError, match="train mode"):
        t(z, [0, 1])


def test_load_cgan_reads_a_checkpoint_file(tmp_path):
    sd = {"module." + k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_cgan_state_dict("default", 3).items()}
    path = os.path.join(tmp_path, "cgan.pth")
    torch.save({"generator": sd, "epoch": 3}, path)
    m = load_cgan(path, n_classes=3, device=DEV, strict=True)
    z = latent(2, 5, device=DEV)
    assert torch.equal(m(z, [0, 2]), model_of("default", 3)(z, [0, 2]))
    assert not m.training
