"""What tests/test_train_batches.py rests on, shown without a GPU: the batches it builds, the arithmetic that lets a small float64
oracle stand for a batch past 2^31 elements, and the conditions its references have to meet.  The GPU file imports its batches,
cases and references from here, so both files speak of the same objects and each reference is computed once per process.

Part A (the 65,535-image launch split under batch statistics).  launch_batch_u8() is one 1 x 1 image per index of
N = 2 * 65,535 + 9, all distinct, the three launches drawn from [0, 64), [96, 160) and [192, 256).  The ranges are there so that
statistics which lose a launch, count one twice or divide by one launch's image count are far from the true ones:
test_part_a_wrong_statistics_move_the_result_by_100_bounds runs the two generator oracles with exactly those statistics (a stand-in
for torch.nn.functional whose batch_norm weighs the images and takes the count it is given, with the device's clamp of a negative
variance) and asserts that `out` moves by at least 100 times the family's bound.  Those runs are in the oracle's float32 and are
compared with its float32 run under the true statistics: the moves are four orders above fp32 rounding, and float64 would triple the
time of this file for the same verdict.  The stand-in with every weight 1 and the true count is held to the float64 oracle under
the family's bound, as ATen fp32 is.

Part B (tensors past 2^31 elements).  A batch that repeats a block of k images q times has the block's batch mean and biased
variance exactly, so the float64 result of the block is the result of every period of the big batch, its gradients are q times the
block's at equal grad_out (or grad_prob) per image, and only running_var differs: it takes the unbiased factor M / (M - 1) at the
big batch's M = q * k * H * W.  big_batch_running_var() derives the big batch's value from the block's, through the biased variance;
the tests below hold all of that on small shapes for esrgan_train_oracle, srgan_train_oracle, srgan_disc_oracle and the two
backward references, and assert that the unrescaled running_var misses the big batch's by more than the GPU test's tolerance, so
that the GPU test's check (e) is not vacuous.  train_crossing() is tests/test_wide_offsets.py's crossing() for the train workspaces:
which tensors pass 2^30, 2^31 and 2^32 elements, and in which periods.  block_case() holds ATen fp32 on each GPU case's own block to
the family's bound and mask caps: conditions on the reference, proved here and not on the device.

The blocks come from periodic_block_u8(): integer arithmetic in torch on whichever device it is given, so the GPU test makes its
block on the device and this file sees the same bytes on the CPU (the GPU test asserts the equality)."""
import contextlib
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

from celebrity_image_denoiser_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import esrgan_train_oracle  # noqa: E402
import srgan_backward_ref  # noqa: E402
import srgan_disc_oracle  # noqa: E402
import srgan_oracle  # noqa: E402
import srgan_train_oracle  # noqa: E402
import test_srgan_disc_backward as TSDB  # noqa: E402
import test_wide_offsets as TWO  # noqa: E402
from test_large_batches import distinct_u8  # noqa: E402

# ------------------------------------------------------------------------------------------------------------------------- Part A
LAUNCH = 65535
N_A = 2 * LAUNCH + 9
LAUNCHES = ((0, LAUNCH), (LAUNCH, 2 * LAUNCH), (2 * LAUNCH, N_A))
RANGES = ((0, 64), (96, 160), (192, 256))
R_A, SCALE_A, WSET_A = 2, 2, "hot"


def launch_batch_u8(seed):
    """uint8 [N_A,1,1,3]: launch j's images have every channel in RANGES[j], and no two images are equal.  The codes are
    distinct_u8's: within a launch an image's rank among them, four times over plus two of its bits and spread by an odd factor
    (a bijection of 18 bits), gives its three 6-bit channels."""
    u8 = distinct_u8(N_A, 1, 1, seed)
    code = u8[:, 0, 0, 0].astype(np.int64) | (u8[:, 0, 0, 1].astype(np.int64) << 8) | (u8[:, 0, 0, 2].astype(np.int64) << 16)
    out = np.empty_like(u8)
    for (lo, _), (a, b) in zip(RANGES, LAUNCHES):
        c = code[a:b]
        v = ((np.argsort(np.argsort(c)) * 4 + (c & 3)) * 40503) & ((1 << 18) - 1)
        for ch in range(3):
            out[a:b, 0, 0, ch] = lo + ((v >> (6 * ch)) & 63)
    return out


def wrong_statistics():
    """{what a kernel would get wrong: (weight of every image in the sums, image count the sums are divided by)}"""
    one = np.ones(N_A)
    lost, twice = one.copy(), one.copy()
    lost[LAUNCH:2 * LAUNCH] = 0.0
    twice[LAUNCH:2 * LAUNCH] = 2.0
    return {"loses the second launch": (lost, lost.sum()), "counts the second launch twice": (twice, twice.sum()),
            "divides by one launch's images": (one, float(LAUNCH))}


class _Functional:
    """torch.nn.functional with train-mode batch_norm on given statistics: per-image weights in the two sums and a given image count,
    then what k_disc_bn_stats does with sums and a count (mean, biased variance clamped at 0, unbiased factor M / (M - 1))."""

    def __init__(self, weight, count):
        self.weight, self.count = torch.as_tensor(weight), float(count)

    def __getattr__(self, name):
        return getattr(F, name)

    def batch_norm(self, v, running_mean, running_var, gamma, beta, training, momentum, eps):
        assert training
        wt, v64 = self.weight.double().view(-1, 1, 1, 1), v.double()          # the device's sums are fp64 too
        M = self.count * v.shape[2] * v.shape[3]
        mean = (v64 * wt).sum((0, 2, 3)) / M
        var = ((v64 * v64 * wt).sum((0, 2, 3)) / M - mean * mean).clamp_min(0.0)
        mean, var = mean.to(v.dtype), var.to(v.dtype)
        running_mean.mul_(1.0 - momentum).add_(momentum * mean)
        running_var.mul_(1.0 - momentum).add_(momentum * var * (M / (M - 1.0)))
        c = lambda t: t.view(1, -1, 1, 1)   # noqa: E731
        return (v - c(mean)) / torch.sqrt(c(var) + eps) * c(gamma) + c(beta)


@contextlib.contextmanager
def statistics(oracle, weight, count):
    """Run `oracle`'s forward with the statistics of _Functional(weight, count)."""
    real = oracle.F
    oracle.F = _Functional(weight, count)
    try:
        yield
    finally:
        oracle.F = real


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _oracle_run(family, sd, x, dtype=torch.float64):
    if family == "esr":
        return esrgan_train_oracle.forward(sd, x, R_A, dtype=dtype)
    return srgan_train_oracle.forward(sd, x, dtype=dtype)


def _normalised(family, u8):
    if family == "esr":
        return np.ascontiguousarray(u8.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0)   # ToTensor(): a true division
    return srgan_oracle.normalise_u8(u8)


@functools.lru_cache(maxsize=None)
def part_a(family):
    """Part A's batch of a generator family ("esr" or "sr"), its weights, the float64 oracle of the WHOLE batch and the oracle's own
    float32 run: computed once, shared, never modified."""
    u8 = launch_batch_u8(31 if family == "esr" else 32)
    x = _normalised(family, u8)
    sd = synth.make_esrgan_state_dict(WSET_A, R_A) if family == "esr" else synth.make_srgan_state_dict(WSET_A, SCALE_A)
    u8.setflags(write=False)
    x.setflags(write=False)
    return dict(u8=u8, x=x, sd=sd, ref=_frozen(_oracle_run(family, sd, x)), r32=_frozen(_oracle_run(family, sd, x, torch.float32)))


def _bound(family, ref, key):
    """The family's bound of one stage (tests/test_esrgan_train.py, tests/test_srgan_train.py); srgan's `out` is held to
    max(1e-5, 2 * e_aten), which needs the fp32 run and is formed where it is used."""
    return (esrgan_train_oracle if family == "esr" else srgan_train_oracle).bound(ref[key])


def sr_out_bound(ref, r32):
    return max(1e-5, 2 * float(np.abs(r32["out"].astype(np.float64) - ref["out"]).max()))


@functools.lru_cache(maxsize=None)
def part_a_sr_backward_aten():
    """e_aten of tests/test_srgan_backward.py's rule on Part A's srgan batch with the dense grad_out of srgan_backward_ref.grad_out:
    ATen fp32 against float64 with ATen's masks (capped).  Two autograd runs over 131,079 images: only the GPU test asks for it."""
    a = part_a("sr")
    G = srgan_backward_ref.grad_out(N_A, SCALE_A, 1, 1)
    g32, pre32, _, _ = srgan_backward_ref.ref_backward(a["sd"], a["x"], G, torch.float32)
    m32 = [v > 0 for v in pre32]
    g64, pre64, _, book = srgan_backward_ref.ref_backward(a["sd"], a["x"], G, torch.float64, masks=m32)
    srgan_backward_ref.check_mask_cap(m32, pre64, "ATen fp32")
    return srgan_backward_ref.rel_errors(g32, g64, book), G


def test_part_a_batch_is_distinct_and_keeps_its_ranges():
    u8 = launch_batch_u8(31)
    assert u8.shape == (N_A, 1, 1, 3) and u8.dtype == np.uint8 and N_A == 131079
    assert len(np.unique(u8.reshape(N_A, 3), axis=0)) == N_A
    for (lo, hi), (a, b) in zip(RANGES, LAUNCHES):
        assert lo <= int(u8[a:b].min()) and int(u8[a:b].max()) < hi
    for (lo, hi), (a, b) in zip(RANGES[:2], LAUNCHES[:2]):          # the full launches fill their range in every channel
        assert all(int(u8[a:b, 0, 0, ch].min()) == lo and int(u8[a:b, 0, 0, ch].max()) == hi - 1 for ch in range(3))
    assert [b - a for a, b in LAUNCHES] == [65535, 65535, 9]
    assert not np.array_equal(u8, launch_batch_u8(32))


def test_part_a_wrong_statistics_move_the_result_by_100_bounds():
    """For both generators: the stand-in with the true statistics meets the oracle's bound; ATen fp32 on the batch is inside every bound; each
    of the three wrong statistics moves `out` (and srgan's sums before tanh) by at least 100 bounds."""
    for family, oracle, keys in (("esr", esrgan_train_oracle, ("out",)), ("sr", srgan_train_oracle, ("pre", "out"))):
        a = part_a(family)
        ref, r32 = a["ref"], a["r32"]
        bounds = {k: _bound(family, ref, k) for k in oracle.STAGES}
        if family == "sr":
            bounds["out"] = sr_out_bound(ref, r32)
        for k in oracle.STAGES:
            share = float(np.abs(r32[k].astype(np.float64) - ref[k]).max()) / bounds[k]
            print(f"{family} {k}: ATen fp32 at {share:.3f} of the bound {bounds[k]:.3e}")
            assert share <= 1.0, (family, k, share)
        with statistics(oracle, np.ones(N_A), N_A):
            same = _oracle_run(family, a["sd"], a["x"], torch.float32)
        for k in keys + tuple(k for k in ref if k.endswith("running_var")):
            assert float(np.abs(same[k].astype(np.float64) - ref[k]).max()) <= bounds.get(k, oracle.bound(ref[k])), (family, k)
        for what, (weight, count) in wrong_statistics().items():
            with statistics(oracle, weight, count):
                wrong = _oracle_run(family, a["sd"], a["x"], torch.float32)
            for k in keys:
                moved = float(np.abs(wrong[k].astype(np.float64) - r32[k]).max())
                print(f"{family}: a kernel that {what} moves {k} by {moved:.3e} = {moved / bounds[k]:.0f} bounds")
                assert moved >= 100 * bounds[k], (family, what, k, moved, bounds[k])


# ------------------------------------------------------------------------------------------------------------------------- Part B
K = 7        # odd, coprime to 65,535, and 65,535 mod 7 = 1: an index off by a launch or a power of two lands in another residue class
BOUNDARIES = (1 << 30, 1 << 31, 1 << 32)
TRAIN_CASES = {
    "esr": dict(n=8750, h=48, w=80, r=2, wset="hot", seed=51),
    # up[0] = 17500 * 64 * 48 * 80 = 4,300,800,000 elements (past 2^32), each base tensor 1,075,200,000 (past 2^30, 2^32 bytes),
    # 24 x 40 is 1.5 x 2.5 tiles of 16 x 16; the workspace is 32.1 GiB
    "sr": dict(n=17500, h=24, w=40, scale=2, wset="hot", seed=52),
    "srd": dict(n=35000, h=24, w=40, kind="trained", seed=53),
}


def periodic_block_u8(k, h, w, seed, device="cpu"):
    """uint8 [k,h,w,3] from a seeded integer mix in torch on `device`: the same bytes on every device."""
    i = torch.arange(k * h * w * 3, dtype=torch.int64, device=device)
    v = (i + seed * 1000003) * 6364136223846793005 + 1442695040888963407
    v = (v ^ (v >> 31)) * 2685821657736338717
    v = v ^ (v >> 29)
    return ((v >> 24) & 255).to(torch.uint8).view(k, h, w, 3)


def big_batch_running_var(rv_block, rv_before, momentum, m_block, m_big):
    """running_var after one train call on the periodic batch (m_big values per channel) from the block's (m_block values): the
    biased variance is the same, the unbiased factor is not."""
    biased = (np.asarray(rv_block, np.float64) - (1.0 - momentum) * np.asarray(rv_before, np.float64)) / momentum * ((m_block - 1.0) / m_block)
    return (1.0 - momentum) * np.asarray(rv_before, np.float64) + momentum * biased * (m_big / (m_big - 1.0))


def big_batch_reference(ref_block, sd, bn_names, momentum, m_block, q):
    """A generator oracle's result on the block, as the reference of its q-fold repetition: only the running_var entries change."""
    big = dict(ref_block)
    for name in bn_names:
        key = name + ".running_var"
        big[key] = big_batch_running_var(ref_block[key], np.asarray(sd[key]), momentum, m_block, q * m_block)
    return big


def _side(s):
    return (s - 1) // 2 + 1


def srd_values_per_channel(h, w):
    """H * W of the four BatchNorm inputs of the SRGAN discriminator (model.3, 6, 9, 12)."""
    h2, w2 = _side(h), _side(w)
    h4, w4 = _side(h2), _side(w2)
    return {3: h2 * w2, 6: h2 * w2, 9: h4 * w4, 12: h4 * w4}


def srd_big_batch_state(sd_block, sd_before, k, q, h, w, momentum=0.1):
    """srgan_disc_oracle.restate's state after one train call on the block -> after one call on its q-fold repetition."""
    big = {key: v.clone() for key, v in sd_block.items()}
    for i, pix in srd_values_per_channel(h, w).items():
        key = f"model.{i}.running_var"
        big[key] = torch.from_numpy(big_batch_running_var(sd_block[key].numpy(), sd_before[key].double().numpy(), momentum, k * pix, q * k * pix))
    return big


def train_tensors_of(family, n):
    """tests/test_wide_offsets.py's tensors_of for the train-mode calls: every tensor of the family's case that holds one value per
    (image, channel, pixel), with its offset in the workspace (srd: in the saved buffer), from the library's own host functions and
    the layouts include/cid.h documents.  -> ([(name, offset, C, Hs, Ws)], bytes of that buffer, other bytes of the case)"""
    L = _lib.lib()
    c = TRAIN_CASES[family]
    h, w = c["h"], c["w"]
    a256 = TWO._a256
    t = a256(4 * n * 64 * h * w)
    tiles = -(-h // 16) * -(-w // 16)
    if family == "esr":
        need = TWO._size(L.cid_esr_train_workspace_bytes, n, h, w, c["r"])
        assert c["r"] == 2 and need == 5 * t + a256(64 * 2 * n * tiles * 8) + 2 * c["r"] * a256(64 * 2 * 4)
        view = lambda s: TWO._view(L.cid_esr_train_stage_view, s, n, h, w, c["r"])   # noqa: E731
        assert view("x1") == (0, 64, h, w) and view("tail_in") == (4 * t, 64, h, w)
        # x1, the two raw z tensors, r[0] (block 0's output, which block 1's first convolution forms) and r[1], the tail's input
        views = [(name, i * t, 64, h, w) for i, name in enumerate(("x1", "z0", "z1", "r.0", "tail_in"))]
        return views, need, n * h * w * 3 + 4 * n * 3 * h * w
    if family == "sr":
        s = c["scale"]
        need = TWO._size(L.cid_sr_train_workspace_bytes, n, h, w, s)
        assert s == 2 and need == 4 * t + a256(4 * 4 * n * 64 * h * w) + a256(64 * 2 * n * tiles * 8) + a256(10 * 64 * 2 * 4)
        view = lambda k: TWO._view(L.cid_sr_train_stage_view, k, n, h, w, s)   # noqa: E731
        assert view("x0") == (0, 64, h, w) and view("trunk") == (3 * t, 64, h, w) and view("tail_in") == (4 * t, 64, 2 * h, 2 * w)
        views = [(name, i * t, 64, h, w) for i, name in enumerate(("x0", "z0", "z1", "trunk"))] + [("tail_in", 4 * t, 64, 2 * h, 2 * w)]
        return views, need, n * h * w * 3 + 2 * 4 * n * 3 * s * h * s * w
    assert family == "srd"
    h2, w2 = _side(h), _side(w)
    h4, w4 = _side(h2), _side(w2)
    views, at = [], 0
    for name, ch, hh, ww in (("a0", 64, h, w), ("z2", 64, h2, w2), ("z5", 128, h2, w2), ("z8", 128, h4, w4), ("z11", 256, h4, w4)):
        views.append((name, at, ch, hh, ww))
        at += a256(4 * n * ch * hh * ww)
    fwd = TWO._size(L.cid_srd_workspace_bytes, n, h, w, 1)
    saved = TWO._size(L.cid_srd_saved_bytes, n, h, w, 1)
    slabs = fwd - TWO._size(L.cid_srd_workspace_bytes, n, h, w, 0)
    assert saved == at + a256(4 * 4 * 256 * 2) + a256(8 * 4 * 256 * 2) + a256(8 * n * 256) + a256(8 * n * 512) + slabs
    bwd = TWO._size(L.cid_srd_backward_workspace_bytes, n, h, w, 1)
    # the larger of the two tests: x, the saved buffer, the backward's workspace, the input gradient, the six masks
    masks = n * (64 * h * w + (64 + 128) * h2 * w2 + (128 + 256) * h4 * w4 + 512)
    return views, saved, bwd + 2 * 4 * n * 3 * h * w + masks + n * h * w * 3 + 16 * n


def train_crossing(family):
    """crossing() for a train case: which tensors pass 2^31 (and 2^30, 2^32) elements, and the periods (blocks of K images) the GPU
    test holds to the oracle: the first, the last, and every period that holds element 2^30, 2^31 or 2^32 of a tensor."""
    n = TRAIN_CASES[family]["n"]
    assert n % K == 0
    q = n // K
    views, buf_bytes, other = train_tensors_of(family, n)
    per = {name: ch * hs * ws for name, _, ch, hs, ws in views}
    past = {b: [name for name in per if n * per[name] > b] for b in BOUNDARIES}
    assert past[1 << 31], (family, {k: n * v for k, v in per.items()})
    blocks = {0, q - 1}
    for name, p in per.items():
        for b in BOUNDARIES:
            if n * p > b:
                assert (n - K) * p > b or b != 1 << 31                      # the last period lies wholly past 2^31
                blocks.add(b // p // K)
    largest = max(per.values())
    anchor = (1 << 31) // largest // K
    assert anchor in blocks and anchor * K * largest <= 1 << 31 < (anchor + 1) * K * largest
    need = buf_bytes + other
    assert buf_bytes > 1 << 33 and need < TWO.MEMORY_CAP
    return dict(n=n, q=q, views=views, per=per, past=past, blocks=sorted(blocks), anchor=anchor, need=need)


def test_the_train_cases_cross_what_they_claim():
    got = {f: train_crossing(f) for f in TRAIN_CASES}
    for f, c in got.items():
        print(f, {b.bit_length() - 1: v for b, v in c["past"].items()}, "periods", c["blocks"], f"need {c['need'] / TWO.GIB:.1f} GiB")
    e, s, d = got["esr"], got["sr"], got["srd"]
    five = ["x1", "z0", "z1", "r.0", "tail_in"]
    assert e["past"][1 << 31] == five and e["past"][1 << 32] == [] and e["per"]["r.0"] == 245760 and 8750 * 245760 == 2150400000
    assert (e["q"], e["blocks"], e["anchor"]) == (1250, [0, 624, 1248, 1249], 1248)      # element 2^31 lies in image 8738 = 7 * 1248 + 2
    assert s["past"][1 << 30] == ["x0", "z0", "z1", "trunk", "tail_in"] and s["past"][1 << 31] == s["past"][1 << 32] == ["tail_in"]
    assert s["per"] == {"x0": 61440, "z0": 61440, "z1": 61440, "trunk": 61440, "tail_in": 245760} and 17500 * 61440 == 1075200000
    # tail_in's elements 2^30, 2^31 and 2^32 lie in images 4369, 8738 and 17476; the base tensors' element 2^30 in image 17476
    assert (s["q"], s["blocks"], s["anchor"]) == (2500, [0, 624, 1248, 2496, 2499], 1248)
    assert d["past"][1 << 31] == ["a0"] and d["past"][1 << 30] == ["a0", "z5"] and d["per"]["a0"] == 61440 and d["per"]["z5"] == 30720
    assert (d["q"], d["blocks"], d["anchor"]) == (5000, [0, 2496, 4993, 4999], 4993)
    assert all(c["need"] < TWO.MEMORY_CAP for c in got.values()) and 30 * TWO.GIB < e["need"] < 50 * TWO.GIB
    # 24 x 40 and 48 x 80 are no multiples of the 16 x 16 trunk tile in one direction each (and 80 is none of the tail's 64 columns)
    assert 24 % 16 and 40 % 16 and 80 % 16 == 0 and 80 % 64


def _tile(a, q):
    return np.ascontiguousarray(np.tile(a, (q,) + (1,) * (a.ndim - 1)))


def _periodic_generator_check(family, oracle, sd, bn_names, k, q, h, w, seed, **kw):
    u8 = periodic_block_u8(k, h, w, seed).numpy()
    xb = _normalised(family, u8)
    run = (lambda x: oracle.forward(sd, x, R_A, **kw)) if family == "esr" else (lambda x: oracle.forward(sd, x, **kw))
    blk, full = run(xb), run(_tile(xb, q))
    stages = [key for key in blk if not key.startswith(("residuals.", "res_blocks."))]
    assert set(oracle.STAGES) <= set(stages)
    for key in stages:
        per = full[key].reshape((q,) + blk[key].shape)
        err = float(np.abs(per - blk[key][None]).max())
        assert err <= 1e-12 * max(1.0, float(np.abs(blk[key]).max())), (family, key, err)
    big = big_batch_reference(blk, sd, bn_names, oracle.MOMENTUM, k * h * w, q)
    worst = 0.0
    for name in bn_names:
        assert int(full[name + ".num_batches_tracked"]) == int(blk[name + ".num_batches_tracked"])
        assert float(np.abs(full[name + ".running_mean"] - blk[name + ".running_mean"]).max()) <= 1e-13
        rv = name + ".running_var"
        assert float(np.abs(full[rv] - big[rv]).max()) <= 1e-13 * max(1.0, float(np.abs(full[rv]).max())), (family, rv)
        worst = max(worst, float(np.abs(full[rv] - blk[rv]).max()) / oracle.bound(full[rv]))
    print(f"{family}: the block's own running_var is up to {worst:.1f} bounds from the periodic batch's")
    assert worst > 1.0                                                      # the M / (M - 1) of the big batch is needed
    return worst


def test_a_periodic_batch_has_its_blocks_result_in_the_generator_oracles():
    """q = 6 periods of K = 7 images of 5 x 9, "hot" weights: every stage and every block output of the periodic batch equals the
    block's to 1e-12, running_mean to 1e-13, running_var once the unbiased factor is taken at the big batch's M; without that it is
    more than a bound away."""
    _periodic_generator_check("esr", esrgan_train_oracle, synth.make_esrgan_state_dict(WSET_A, R_A), esrgan_train_oracle.BN_NAMES(R_A),
                              K, 6, 5, 9, 61)
    _periodic_generator_check("sr", srgan_train_oracle, synth.make_srgan_state_dict(WSET_A, SCALE_A), srgan_train_oracle.BN_NAMES,
                              K, 6, 5, 9, 62)


def test_a_periodic_batch_has_q_times_its_blocks_gradients_in_the_srgan_backward_reference():
    k, q, h, w = K, 3, 5, 9
    sd = synth.make_srgan_state_dict(WSET_A, SCALE_A)
    xb = srgan_oracle.normalise_u8(periodic_block_u8(k, h, w, 63).numpy())
    G = srgan_backward_ref.grad_out(k, SCALE_A, h, w)
    gb, preb, outb, _ = srgan_backward_ref.ref_backward(sd, xb, G)
    gf, pref, outf, _ = srgan_backward_ref.ref_backward(sd, _tile(xb, q), torch.from_numpy(_tile(G.numpy(), q)))
    assert float((outf.reshape((q,) + outb.shape) - outb[None]).abs().max()) <= 1e-12
    scale = {key: float(v.abs().max()) for key, v in gb.items()}
    for key in gb:
        den = scale[key.replace("bias", "weight")] if key in srgan_backward_ref.BN_BIASES else scale[key]
        assert float((gf[key] - q * gb[key]).abs().max()) <= 1e-10 * q * den, key


def test_a_periodic_batch_has_its_blocks_result_in_the_srgan_discriminator_references():
    """Probabilities, running statistics (running_var through big_batch_running_var, per layer's own H * W) and, with the mean BCE of
    tests/test_srgan_disc_backward.py's reference, the gradients: the loss's 1 / N gives every image 1 / q of the grad_prob it has in
    the block, so the sums over q periods are the block's gradients; at EQUAL grad_prob per image they are q times the block's,
    which is what the GPU test feeds."""
    k, q, h, w = K, 3, 9, 10
    x = torch.from_numpy(synth.normalize_u8(periodic_block_u8(k, h, w, 64).numpy()))
    xf = x.repeat(q, 1, 1, 1)
    before = srgan_disc_oracle.cast(srgan_disc_oracle.weights("trained"), torch.float64)
    sb, sf = srgan_disc_oracle.cast(before, torch.float64), srgan_disc_oracle.cast(before, torch.float64)
    pb, pf = srgan_disc_oracle.restate(sb, x.double(), True), srgan_disc_oracle.restate(sf, xf.double(), True)
    assert float((pf.view(q, k) - pb[None]).abs().max()) <= 1e-13
    big = srd_big_batch_state(sb, before, k, q, h, w)
    worst = 0.0
    for i in srd_values_per_channel(h, w):
        assert int(sf[f"model.{i}.num_batches_tracked"]) == int(sb[f"model.{i}.num_batches_tracked"])
        assert float((sf[f"model.{i}.running_mean"] - sb[f"model.{i}.running_mean"]).abs().max()) <= 1e-13
        rv = f"model.{i}.running_var"
        assert float((sf[rv] - big[rv]).abs().max()) <= 1e-13 * max(1.0, float(sf[rv].abs().max())), rv
        worst = max(worst, float(((sf[rv] - sb[rv]).abs() / (1e-5 * sf[rv].abs().clamp(min=1.0))).max()))   # test_srgan_disc.py's rule
    print(f"srd: the block's own running_var is up to {worst:.1f} bounds from the periodic batch's")
    assert worst > 1.0
    sd = srgan_disc_oracle.weights("trained")
    gb, gxb, _, _ = TSDB.ref_backward(sd, x, True, 1.0, torch.float64)
    gf, gxf, _, _ = TSDB.ref_backward(sd, xf, True, 1.0, torch.float64)
    assert float((q * gxf.view((q,) + gxb.shape) - gxb[None]).abs().max()) <= 1e-10 * float(gxb.abs().max())
    for key in TSDB.PARAMS:
        den = float(gb[key.replace("bias", "weight")].abs().max()) if key in TSDB.BN_BIASES else float(gb[key].abs().max())
        assert float((gf[key] - gb[key]).abs().max()) <= 1e-10 * den, key


# --------------------------------------------------------------------------------------------- the GPU cases' blocks and references
@functools.lru_cache(maxsize=None)
def block_case(family):
    """The block of a GPU case of Part B, the float64 reference of its periodic batch, and ATen fp32 held to the family's bounds and
    mask caps on that block: computed once, shared, never modified."""
    c = TRAIN_CASES[family]
    n, h, w = c["n"], c["h"], c["w"]
    q = n // K
    u8 = periodic_block_u8(K, h, w, c["seed"]).numpy()
    u8.setflags(write=False)
    if family in ("esr", "sr"):
        oracle = esrgan_train_oracle if family == "esr" else srgan_train_oracle
        names = oracle.BN_NAMES(c["r"]) if family == "esr" else oracle.BN_NAMES
        sd = synth.make_esrgan_state_dict(c["wset"], c["r"]) if family == "esr" else synth.make_srgan_state_dict(c["wset"], c["scale"])
        x = _normalised(family, u8)
        ref, r32 = _oracle_run(family, sd, x), _oracle_run(family, sd, x, torch.float32)
        bounds = {k: oracle.bound(ref[k]) for k in oracle.STAGES}
        if family == "sr":
            bounds["out"] = sr_out_bound(ref, r32)
        for k in oracle.STAGES:
            share = float(np.abs(r32[k].astype(np.float64) - ref[k]).max()) / bounds[k]
            print(f"{family} block, {k}: ATen fp32 at {share:.3f} of the bound {bounds[k]:.3e}")
            assert share <= 1.0, (family, k, share)
        big = big_batch_reference(ref, sd, names, oracle.MOMENTUM, K * h * w, q)
        unscaled = max(float(np.abs(big[b + ".running_var"] - ref[b + ".running_var"]).max()) / oracle.bound(big[b + ".running_var"]) for b in names)
        return dict(u8=u8, x=x, sd=sd, ref=_frozen(big), bounds=bounds, q=q, unscaled=unscaled)
    assert family == "srd"
    x = torch.from_numpy(synth.normalize_u8(u8))
    sd = srgan_disc_oracle.weights(c["kind"])
    before = srgan_disc_oracle.cast(sd, torch.float64)
    s64, s32 = srgan_disc_oracle.cast(sd, torch.float64), srgan_disc_oracle.cast(sd, torch.float32)
    p64, p32 = srgan_disc_oracle.restate(s64, x.double(), True), srgan_disc_oracle.restate(s32, x, True)
    own = float((p64 - p32.double()).abs().max())
    print(f"srd block: ATen fp32 probabilities {own:.2e} from float64")
    assert own <= TSDB.TOL / 10                                             # tests/test_srgan_disc.py's CONDITION
    assert 0.02 < float(p64.min()) and float(p64.max()) < 0.98             # the sigmoid is not saturated
    # the backward: ATen fp32 with its own masks against float64 with ATen's masks, both capped
    g32, gx32, ys32, _ = TSDB.ref_backward(sd, x, True, 1.0, torch.float32)
    masks32 = [y > 0 for y in ys32]
    g64a, gx64a, ys64, _ = TSDB.ref_backward(sd, x, True, 1.0, torch.float64, masks32)
    TSDB.check_mask_cap(masks32, ys64, "aten")
    e_aten = TSDB.rel_errors(g32, gx32, g64a, gx64a, True)
    print("srd block: e_aten " + ", ".join(f"{k} {v:.1e}" for k, v in e_aten.items() if v > 1e-6))
    return dict(u8=u8, x=x, sd=sd, p64=p64, state=srd_big_batch_state(s64, before, K, q, h, w), e_aten=e_aten, q=q)


def test_aten_fp32_meets_the_bounds_on_every_block_of_part_b():
    """block_case() asserts the bounds and caps while it builds each reference.  Check (e) of the GPU file tells the big batch's M from
    the block's only where the two running_var lie more than a bound apart: on the sr case they do (3.57 bounds), on the esr case they
    do not (0.87: M = 26,880 values per channel in the block already, and variances near 1), so there (e) holds the statistics but
    not the count; the small shapes above and the sr case carry that."""
    for family in TRAIN_CASES:
        b = block_case(family)
        assert b["q"] * K == TRAIN_CASES[family]["n"]
        if family != "srd":
            print(f"{family}: without the big batch's M / (M - 1) running_var would be {b['unscaled']:.2f} bounds off")
    assert block_case("sr")["unscaled"] > 1.0 > block_case("esr")["unscaled"] > 0.0
    # the mix is integer arithmetic, identical wherever it runs: bytes pinned here, and the GPU file compares its device block with the host's
    pinned = periodic_block_u8(2, 3, 4, 5).view(-1)
    assert pinned[:8].tolist() == [178, 212, 58, 15, 98, 3, 166, 228] and pinned[-4:].tolist() == [116, 6, 74, 81]
    block = periodic_block_u8(K, 24, 40, 53)
    assert block.view(-1)[:8].tolist() == [2, 254, 252, 181, 194, 138, 103, 135] and int(block.long().sum()) == 2563403
    assert len(set(block.view(K, -1).sum(1).tolist())) == K                                     # seven different images
