"""The server's CGANGenerator (reference backend/app.py:105-143) without a GPU: the module's state_dict against the keys recorded from
the reference class, the synthetic weight sets, the latent's restatement, the host side of cid_cg_* (include/cid.h), the index
arithmetic of the four-parity transposed convolution, and tests/cgan_oracle.py, the float64 restatement the GPU tests measure against,
held to every fixture recorded from the reference."""
import ctypes
import glob
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth
from celebrity_image_denoiser_amd.cgan import CGANGenerator

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cgan_oracle  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ERR_INVALID, ERR_SHAPE, ERR_KEY, ERR_STATE, ERR_WORKSPACE = 1, 2, 3, 4, 5
SIZE_CAP = 700 * 1000   # the largest fixture already in tests/golden


def _keys():
    return json.load(open(os.path.join(GOLDEN, "cgan_keys.json")))


@pytest.mark.parametrize("n_classes", [10, 3])
def test_state_dict_matches_the_reference_class(n_classes):
    want = _keys()[f"c{n_classes}"]
    sd = CGANGenerator(n_classes).state_dict()
    assert [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()] == want
    assert len(want) == 31
    shapes = synth.cgan_param_shapes(n_classes)
    assert [[k, list(s), d] for k, (s, d) in shapes.items()] == want
    assert shapes["model.2.weight"][0] == (128, 128, 4, 4) and shapes["model.5.weight"][0] == (128, 64, 4, 4)   # [Cin,Cout,4,4]


def test_state_dict_round_trip_is_lossless():
    sd = synth.make_cgan_state_dict("hot")
    m = CGANGenerator()
    res = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    back = m.state_dict()
    assert list(back) == list(sd)
    for k, v in sd.items():
        assert back[k].dtype == torch.from_numpy(np.asarray(v)).dtype and np.array_equal(back[k].numpy(), v), k


def test_errors_that_need_no_gpu():
    m = CGANGenerator(3)
    assert m.eval() is m and not m.training
    m.train()
    with pytest.raises(RuntimeError, match="train mode"):
        m(torch.zeros(1, 100), torch.zeros(1, dtype=torch.int64))
    m.eval()
    with pytest.raises(RuntimeError, match="CPU tensor"):
        m(torch.zeros(1, 100), [0])
    with pytest.raises(RuntimeError, match="latent of shape"):
        m(torch.zeros(1, 99), [0])
    with pytest.raises(ValueError, match="hard-codes"):
        CGANGenerator(10, latent_dim=7)
    with pytest.raises(ValueError):
        CGANGenerator(0)
    with pytest.raises(ValueError):
        synth.make_cgan_state_dict("warm")


def _digest(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def test_synthetic_weights_are_reproducible():
    digests = json.load(open(os.path.join(GOLDEN, "cgan_synth_digests.json")))
    for kind in ("default", "hot"):
        for c in (10, 3):
            sd = synth.make_cgan_state_dict(kind, c)
            assert _digest(sd) == digests[f"{kind}_c{c}"], (kind, c)
    d, h = synth.make_cgan_state_dict("default"), synth.make_cgan_state_dict("hot")
    assert json.load(open(os.path.join(GOLDEN, "cgan_stats.json")))["hot_gain"] == synth.CGAN_HOT_GAIN
    for sd, gain in ((d, 1.0), (h, synth.CGAN_HOT_GAIN)):
        for k, fan in (("l1.weight", 200), ("model.2.weight", 128 * 16), ("model.5.weight", 64 * 16), ("model.8.weight", 32 * 16),
                       ("model.11.weight", 288)):
            b = np.sqrt(gain / fan)
            assert 0.98 * b < np.abs(sd[k]).max() <= b, k
        assert 0.8 < sd["label_emb.weight"].std() < 1.2
    for i in (0, 3, 6, 9):
        p = f"model.{i}."
        assert (d[p + "weight"] == 1).all() and (d[p + "bias"] == 0).all() and (d[p + "running_mean"] == 0).all() and (d[p + "running_var"] == 1).all()
        assert 0.6 <= h[p + "weight"].min() and h[p + "weight"].max() <= 1.4 and 0 < np.abs(h[p + "bias"]).max() <= 0.1
        assert 0 < np.abs(h[p + "running_mean"]).max() <= 0.3 and 0.5 <= h[p + "running_var"].min() and h[p + "running_var"].max() <= 1.5


def test_stream_constants_and_latent_restatement():
    assert synth.CGAN_Z_STREAMS == (synth._fnv1a64("cgan:z:u1"), synth._fnv1a64("cgan:z:u2"))
    assert len(set(synth.CGAN_Z_STREAMS) | {s for v in synth.NOISE_STREAMS.values() for s in v}) == 2 + 10
    z = synth.cgan_latent_np(7, 99, 5)
    assert z.shape == (7, 100) and z.dtype == np.float32 and np.isfinite(z).all()
    # an image alone and in a batch: a row depends on seed + first_index + i alone
    for k in range(7):
        assert np.array_equal(synth.cgan_latent_np(1, 99, 5 + k)[0], z[k])
        assert np.array_equal(synth.cgan_latent_np(1, 99 + 5 + k, 0)[0], z[k])
    assert np.array_equal(synth.cgan_latent_np(3, 99, 7), z[2:5])
    big = synth.cgan_latent_np(400, 1)
    assert abs(float(big.mean())) < 0.02 and abs(float(big.std()) - 1) < 0.02
    assert not np.array_equal(synth.cgan_latent_np(1, 100, 5), z[:1])


@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (8, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_four_parity_form_equals_the_scatter_definition_exactly(hw):
    """Small integers stored as floats: every product and sum is exact, so the two forms must agree to the bit.  This is the index
    arithmetic k_cg_up rests on: oy = 2 iy - 1 + ky, parity (py, px) gathers inputs (m - 1 + py + dy, n - 1 + px + dx) through taps
    (3 - py - 2 dy, 3 - px - 2 dx)."""
    rng = np.random.RandomState(hw[0] * 10 + hw[1])
    x = rng.randint(-4, 5, size=(2, 3) + hw).astype(np.float64)
    w = rng.randint(-4, 5, size=(3, 2, 4, 4)).astype(np.float64)
    b = rng.randint(-4, 5, size=2).astype(np.float64)
    a, p = cgan_oracle.conv_transpose_scatter(x, w, b), cgan_oracle.conv_transpose_parity(x, w, b)
    assert a.shape == (2, 2, 2 * hw[0], 2 * hw[1]) and np.array_equal(a, p)
    want = torch.nn.functional.conv_transpose2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), stride=2, padding=1).numpy()
    assert np.array_equal(a, want)


def test_param_key_enumerates_exactly_the_keys():
    L = _lib.lib()
    for c in (10, 3):
        h = ctypes.c_void_p()
        assert L.cid_cg_create(ctypes.byref(h), c) == 0
        keys = []
        while L.cid_cg_param_key(h, len(keys)) is not None:
            keys.append(L.cid_cg_param_key(h, len(keys)).decode())
        assert keys == list(synth.cgan_param_shapes(c)) == [k for k, _, _ in _keys()[f"c{c}"]]
        assert L.cid_cg_param_key(h, -1) is None and L.cid_cg_param_key(None, 0) is None
        L.cid_cg_destroy(h)


def _set(L, h, key, a):
    a = np.ascontiguousarray(a) if np.ndim(a) else np.asarray(a)      # ascontiguousarray would make a 0-d array 1-d
    shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
    return L.cid_cg_set_weight(h, key.encode(), a.ctypes.data, shape, a.ndim)


def test_c_abi_argument_errors_need_no_gpu():
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.cid_cg_create(None, 10) == ERR_INVALID
    for bad in (0, -1, (1 << 20) + 1):
        assert L.cid_cg_create(ctypes.byref(h), bad) == ERR_INVALID, bad
    assert L.cid_cg_create(ctypes.byref(h), 3) == 0
    assert L.cid_cg_last_error(None) == b"null handle"
    sd = synth.make_cgan_state_dict("default", 3)
    miss = ctypes.c_int()
    assert L.cid_cg_missing_weights(h, ctypes.byref(miss)) == 0 and miss.value == 31 - 4      # less the num_batches_tracked
    assert L.cid_cg_missing_weights(h, None) == ERR_INVALID and L.cid_cg_missing_weights(None, ctypes.byref(miss)) == ERR_INVALID
    w = sd["model.11.weight"]
    s4 = (ctypes.c_int64 * 4)(*w.shape)
    assert L.cid_cg_set_weight(None, b"model.11.weight", w.ctypes.data, s4, 4) == ERR_INVALID
    assert L.cid_cg_set_weight(h, None, w.ctypes.data, s4, 4) == ERR_INVALID
    assert L.cid_cg_set_weight(h, b"model.11.weight", None, s4, 4) == ERR_INVALID
    assert L.cid_cg_set_weight(h, b"model.11.weight", w.ctypes.data, None, 4) == ERR_INVALID
    assert _set(L, h, "model.12.weight", w) == ERR_KEY and b"unexpected key" in L.cid_cg_last_error(h)
    assert _set(L, h, "model.11.weight", sd["model.8.weight"]) == ERR_SHAPE and b"size mismatch for model.11.weight" in L.cid_cg_last_error(h)
    assert _set(L, h, "label_emb.weight", synth.make_cgan_state_dict("default", 10)["label_emb.weight"]) == ERR_SHAPE   # 10 classes into 3
    assert _set(L, h, "model.5.weight", np.ascontiguousarray(sd["model.5.weight"].transpose(1, 0, 2, 3))) == ERR_SHAPE  # [Cout,Cin,4,4]
    assert _set(L, h, "l1.weight", sd["l1.weight"].reshape(-1)) == ERR_SHAPE
    assert _set(L, h, "model.0.num_batches_tracked", np.zeros(1, np.int64)) == ERR_SHAPE
    assert L.cid_cg_set_bn_eps(h, 4, 1e-5) == ERR_INVALID and L.cid_cg_set_bn_eps(h, -1, 1e-5) == ERR_INVALID
    assert L.cid_cg_set_bn_eps(h, 0, -1.0) == ERR_INVALID and L.cid_cg_set_bn_eps(h, 1, float("nan")) == ERR_INVALID
    assert L.cid_cg_set_bn_eps(None, 0, 1e-5) == ERR_INVALID and L.cid_cg_set_bn_eps(h, 3, 1e-3) == 0
    fake = ctypes.c_void_p(1 << 20)                                                          # aligned, never dereferenced
    assert L.cid_cg_upload_weights(h, None, None) == ERR_INVALID
    assert L.cid_cg_upload_weights(h, ctypes.c_void_p((1 << 20) + 64), None) == ERR_WORKSPACE
    assert L.cid_cg_upload_weights(h, fake, None) == ERR_STATE and b"label_emb.weight not set" in L.cid_cg_last_error(h)
    for k, v in sd.items():
        if k != "model.11.bias":
            assert _set(L, h, k, v) == 0, k
    assert L.cid_cg_missing_weights(h, ctypes.byref(miss)) == 0 and miss.value == 1
    assert L.cid_cg_upload_weights(h, fake, None) == ERR_STATE and b"model.11.bias not set" in L.cid_cg_last_error(h)
    a64 = lambda v: (v + 63) // 64 * 64   # noqa: E731
    floats = a64(512 * 64 * 52 + 8192 + 256) + sum(a64(16 * ci * co + 3 * co) for ci, co in ((128, 128), (128, 64), (64, 32))) + 896 + a64(300)
    assert L.cid_cg_packed_weights_bytes(h) == 4 * floats and L.cid_cg_packed_weights_bytes(None) == 0
    n = ctypes.c_size_t()
    per = (8192 + 128 * 256 + 64 * 1024 + 32 * 4096) * 4
    assert L.cid_cg_workspace_bytes(3, ctypes.byref(n)) == 0 and n.value == 3 * per
    assert L.cid_cg_workspace_bytes(3, None) == ERR_INVALID
    for bad in (0, -1, (1 << 18) + 1):
        assert L.cid_cg_workspace_bytes(bad, ctypes.byref(n)) == ERR_SHAPE, bad
    assert L.cid_cg_workspace_bytes(3, ctypes.byref(n)) == 0

    def fwd(hh, z, lab, o, fo, N, ws, nb, flags=0):
        return L.cid_cg_forward(hh, z, lab, o, fo, N, flags, ws, nb, None)

    big = 1 << 40
    odd = ctypes.c_void_p((1 << 20) + 2)
    assert fwd(None, fake, fake, fake, 0, 1, fake, big) == ERR_INVALID
    assert fwd(h, None, fake, fake, 0, 1, fake, big) == ERR_INVALID and b"null pointer" in L.cid_cg_last_error(h)
    assert fwd(h, fake, None, fake, 0, 1, fake, big) == ERR_INVALID and fwd(h, fake, fake, None, 0, 1, fake, big) == ERR_INVALID
    assert fwd(h, fake, fake, fake, 0, 1, None, big) == ERR_INVALID
    assert fwd(h, fake, fake, fake, 2, 1, fake, big) == ERR_INVALID and b"unknown format" in L.cid_cg_last_error(h)
    assert fwd(h, odd, fake, fake, 0, 1, fake, big) == ERR_INVALID and fwd(h, fake, odd, fake, 0, 1, fake, big) == ERR_INVALID
    assert fwd(h, fake, fake, odd, 0, 1, fake, big) == ERR_INVALID and b"misaligned" in L.cid_cg_last_error(h)
    assert fwd(h, fake, fake, fake, 0, 1, fake, big, flags=2) == ERR_INVALID and b"unknown flags" in L.cid_cg_last_error(h)
    assert fwd(h, fake, fake, fake, 1, 1, fake, big, flags=_lib.CID_CG_RAW) == ERR_INVALID and b"CID_CG_RAW" in L.cid_cg_last_error(h)
    for bad in (0, -3, (1 << 18) + 1):
        assert fwd(h, fake, fake, fake, 0, bad, fake, big) == ERR_SHAPE, bad
    assert fwd(h, fake, fake, fake, 0, 3, fake, n.value - 1) == ERR_WORKSPACE
    assert fwd(h, fake, fake, fake, 0, 3, ctypes.c_void_p((1 << 20) + 128), big) == ERR_WORKSPACE
    assert fwd(h, fake, fake, odd, 1, 3, fake, n.value) == ERR_STATE and b"weights not uploaded" in L.cid_cg_last_error(h)
    assert L.cid_cg_latent(1, 0, 4, None, None) == ERR_INVALID and L.cid_cg_latent(1, 0, 4, odd, None) == ERR_INVALID
    assert L.cid_cg_latent(1, 0, 0, fake, None) == ERR_SHAPE and L.cid_cg_latent(1, 0, (1 << 18) + 1, fake, None) == ERR_SHAPE
    off, c, hs, ws, cb = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    refs = (ctypes.byref(off), ctypes.byref(c), ctypes.byref(hs), ctypes.byref(ws), ctypes.byref(cb))
    view = lambda: (off.value, c.value, hs.value, ws.value, cb.value)   # noqa: E731
    assert L.cid_cg_stage_view(b"l1", 3, *refs) == 0 and view() == (0, 128, 8, 8, 8)
    assert L.cid_cg_stage_view(b"t1", 3, *refs) == 0 and view() == (3 * 8192 * 4, 128, 16, 16, 8)
    assert L.cid_cg_stage_view(b"t2", 3, *refs) == 0 and view() == (3 * (8192 + 32768) * 4, 64, 32, 32, 8)
    assert L.cid_cg_stage_view(b"t3", 3, *refs) == 0 and view() == (3 * (8192 + 32768 + 65536) * 4, 32, 64, 64, 8)
    assert L.cid_cg_stage_view(b"t4", 3, *refs) == ERR_KEY and L.cid_cg_stage_view(None, 3, *refs) == ERR_INVALID
    assert L.cid_cg_stage_view(b"l1", 0, *refs) == ERR_SHAPE
    L.cid_cg_destroy(h)


def _fixtures():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "cgan_*_n[0-9].npz")) if "_u8_" not in p)


def test_the_fixture_set_is_complete_and_small():
    assert _fixtures() == sorted(f"cgan_{w}_n{n}" for w in ("default", "hot") for n in (1, 3))
    for w in ("default", "hot"):
        assert os.path.exists(os.path.join(GOLDEN, f"cgan_{w}_u8_n2.npz"))
    for p in glob.glob(os.path.join(GOLDEN, "cgan_*")):
        assert os.path.getsize(p) < SIZE_CAP, p


def test_the_reference_alone_stays_inside_the_caps():
    st = json.load(open(os.path.join(GOLDEN, "cgan_stats.json")))
    assert st["worst_fp32_stage_error"] <= 2e-6            # 5x under the 1e-5 rule
    for w in ("default", "hot"):
        u = st[f"cgan_{w}_u8_n2"]
        assert u["aten_vs_oracle64_max"] <= 1 and u["aten_vs_oracle64_differing"] <= 1e-3
        assert (0.05 <= u["saturated_bytes"] <= 0.90) if w == "hot" else u["saturated_bytes"] == 0
    assert "running_mean should contain 6 elements not 128" in st["image_branch_error"]


@pytest.mark.parametrize("name", _fixtures())
def test_oracle_agrees_with_every_fixture_tensor(name):
    """The fixtures are the reference class on ATen fp32; the oracle runs in float64.  Per stage
    max|delta| <= 1e-5 * max(1, max|ref64|); `out` is bounded by the scale of the sums before tanh (tanh is 1-Lipschitz)."""
    _, wset, nn_ = name.split("_")
    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    n = int(nn_[1:])
    assert fx["z"].shape == (n, 100) and fx["labels"].shape == (n,) and fx["labels"].dtype == np.int64
    if n == 3:
        assert fx["labels"].tolist() == [0, 9, 3]
    ref = cgan_oracle.forward(synth.make_cgan_state_dict(wset), fx["z"], fx["labels"])
    r32 = cgan_oracle.forward(synth.make_cgan_state_dict(wset), fx["z"], fx["labels"], dtype=np.float32)
    shapes = {"l1": (n, 128, 8, 8), "t1": (n, 128, 16, 16), "t2": (n, 64, 32, 32), "t3": (n, 32, 64, 64), "pre": (n, 3, 64, 64), "out": (n, 3, 64, 64)}
    for k, s in shapes.items():
        assert ref[k].shape == s and ref[k].dtype == np.float64, k
    for k in ("l1", "t1", "t2", "pre"):
        if k in fx.files:
            for got in (fx[k], r32[k]):
                assert got.shape == ref[k].shape
                assert np.abs(got - ref[k]).max() <= cgan_oracle.bound(ref[k]), k
    assert set(fx.files) == ({"z", "labels", "l1", "t1", "t2", "pre", "out"} if n == 1 else {"z", "labels", "l1", "out"})
    for got in (fx["out"], r32["out"]):
        assert np.abs(got - ref["out"]).max() <= cgan_oracle.bound(ref["pre"])
    assert np.abs(ref["out"]).max() <= 1.0 and (ref["l1"] >= 0).all() and 0.2 < (ref["t2"] == 0).mean() < 0.8
    # the batch does not enter an image's result
    one = cgan_oracle.forward(synth.make_cgan_state_dict(wset), fx["z"][-1:], fx["labels"][-1:])
    assert np.abs(one["out"] - ref["out"][-1:]).max() <= 1e-12
    with pytest.raises(IndexError):
        cgan_oracle.forward(synth.make_cgan_state_dict(wset), fx["z"][:1], [10])


@pytest.mark.parametrize("wset", ["default", "hot"])
def test_oracle_agrees_with_the_uint8_fixture(wset):
    fx = np.load(os.path.join(GOLDEN, f"cgan_{wset}_u8_n2.npz"))
    assert fx["out_u8"].shape == (2, 64, 64, 3) and fx["out_u8"].dtype == np.uint8
    ref = cgan_oracle.forward(synth.make_cgan_state_dict(wset), fx["z"], fx["labels"])
    got, want = cgan_oracle.to_u8(ref["out"]), fx["out_u8"]
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert d.max() <= 1 and (d != 0).mean() <= 1e-3
    sat = ((want == 0) | (want == 255)).mean()
    if wset == "hot":
        assert 0.05 <= sat <= 0.90, sat
    else:
        assert sat == 0, sat


def test_to_u8_rounds_to_fp32_before_the_view():
    v = np.full((1, 3, 1, 1), np.tanh(10.0))
    assert v.max() < 1.0 and int(((v * 0.5 + 0.5) * 255).astype(np.uint8).max()) == 254
    assert cgan_oracle.to_u8(v).max() == 255 and cgan_oracle.to_u8(-v).max() == 0
