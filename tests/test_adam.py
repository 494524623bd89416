"""The device Adam step (cid_adam_step / k_adam_step, cid.Adam) on the GPU.

References: synth.adam_step_np, the numpy restatement of the kernel's expression tree (tests/test_adam_host.py holds it against
torch.optim.Adam), for the bit-level tests; torch.optim.Adam on float64 CPU copies for the trajectory tests, with the bound
e <= max(1e-6, 2 e(torch fp32 on the CPU)), e(T) = max|T - T64| / max|T64|, per tensor and state entry.
"""
import copy
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import celebrity_image_denoiser_amd as cid
from celebrity_image_denoiser_amd import _lib, ckpt, synth

DEV = "cuda:0"
SIZES = (1, 3, 63, 64, 65, 257, 4097, 36864, 36865)
# element offset mod 4 of (param, grad, exp_avg, exp_avg_sq) inside a 16-byte-aligned flat buffer: (0, 0, 0, 0) is the 16-byte path
# with neither head nor tail phantom elements, (r, r, r, r) the 16-byte path behind a 4-byte head, anything else 4-byte accesses only
RESIDUES = ((0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 2, 0), (0, 0, 0, 0), (3, 3, 3, 3), (0, 1, 2, 3), (1, 1, 1, 1), (0, 0, 0, 0), (2, 2, 2, 2))
LR = 1e-4
KEYS = ("param", "exp_avg", "exp_avg_sq")


def _hyper(weight_decay=0.0, lr=LR):
    return _lib.AdamHyper(lr, 0.9, 0.999, 1e-8, weight_decay)


def _layout():
    """-> ([(param, grad, exp_avg, exp_avg_sq) element offsets per tensor], total elements): every array at its residue, at least one
    canary element between neighbours and at both ends."""
    cur, out = 1, []
    for n, res in zip(SIZES, RESIDUES):
        offs = []
        for r in res:
            cur += (r - cur) % 4
            offs.append(cur)
            cur += n + 1
        out.append(tuple(offs))
    return out, cur + 3


def _gradient(rng, n):
    g = (rng.standard_normal(n) * 10.0 ** int(rng.integers(-6, 1))).astype(np.float32)
    g[:2] = (0.0, -0.0)[:n]          # exact zeros of both signs at both ends
    g[-2:] = (0.0, -0.0)[-n:]
    return g


@functools.lru_cache(maxsize=None)
def _case():
    rng = np.random.default_rng(77)
    offs, total = _layout()
    flat = np.full(total, np.nan, np.float32)
    for n, (po, go, mo, vo) in zip(SIZES, offs):
        flat[po:po + n] = rng.standard_normal(n) * 0.05
        flat[mo:mo + n] = 0.0
        flat[vo:vo + n] = 0.0
    grads = [[_gradient(rng, n) for n in SIZES] for _ in range(3)]
    return offs, flat, grads


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _table(flat_dev, offs, order, steps):
    t = (_lib.AdamTensor * len(order))()
    base = flat_dev.data_ptr()
    assert base % 16 == 0
    for e, i in zip(t, order):
        po, go, mo, vo = offs[i]
        e.param, e.grad, e.exp_avg, e.exp_avg_sq = base + 4 * po, base + 4 * go, base + 4 * mo, base + 4 * vo
        e.count, e.step = SIZES[i], steps
    return t


def _launch(table, hp):
    rc = _lib.lib().cid_adam_step(table, len(table), ctypes.byref(hp), torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.CID_OK, rc


def _ulp_distance(a, b):
    """Distance in fp32 units in the last place between same-shaped finite arrays (monotone integer map of the bit patterns)."""
    def key(x):
        i = _bits(x).astype(np.int64)
        return np.where(i & 0x80000000, 0x80000000 - i, i)
    return np.abs(key(a) - key(b))


@pytest.mark.gpu
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_identity_with_the_restatement(weight_decay):
    """Three consecutive steps over nine tensors carved out of one flat buffer.  Each step is compared with the restatement applied to
    the state the device held before it: exp_avg and exp_avg_sq bit for bit, the parameter within one fp32 ulp at no more than
    ceil(1e-6 count) elements of a tensor and equal elsewhere.  The NaN canaries between the tensors and the gradients keep their bits."""
    offs, flat0, grads = _case()
    flat = torch.from_numpy(flat0.copy()).to(DEV)
    inside = np.zeros(flat0.size, bool)
    for n, o4 in zip(SIZES, offs):
        assert len({o % 4 for o in o4}) == len(set(RESIDUES[SIZES.index(n)]))
        for o in o4:
            assert not inside[o - 1:o + n + 1].any()      # no two arrays touch
            inside[o:o + n] = True
    before = flat0.copy()
    for s in range(3):
        for i, (n, o4) in enumerate(zip(SIZES, offs)):
            before[o4[1]:o4[1] + n] = grads[s][i]
        flat.copy_(torch.from_numpy(before))
        _launch(_table(flat, offs, range(len(SIZES)), s + 1), _hyper(weight_decay))
        after = flat.cpu().numpy()
        assert np.array_equal(_bits(after)[~inside], _bits(flat0)[~inside]), "a canary was written"
        for i, (n, (po, go, mo, vo)) in enumerate(zip(SIZES, offs)):
            sl = lambda a, o: a[o:o + n]   # noqa: E731
            assert np.array_equal(_bits(sl(after, go)), _bits(grads[s][i])), f"gradient of tensor {n} changed"
            p1, m1, v1 = synth.adam_step_np(sl(before, po), grads[s][i], sl(before, mo), sl(before, vo), s + 1, lr=LR,
                                            weight_decay=weight_decay)
            assert np.array_equal(_bits(sl(after, mo)), _bits(m1)), f"step {s + 1} size {n}: exp_avg"
            assert np.array_equal(_bits(sl(after, vo)), _bits(v1)), f"step {s + 1} size {n}: exp_avg_sq"
            d = _ulp_distance(sl(after, po), p1)
            print(f"wd={weight_decay} step {s + 1} size {n}: {int((d > 0).sum())} parameter element(s) off, max {int(d.max())} ulp")
            assert d.max() <= 1 and int((d > 0).sum()) <= math.ceil(1e-6 * n), f"step {s + 1} size {n}: parameter"
            assert np.isfinite(sl(after, po)).all()
        before = after.copy()


@pytest.mark.gpu
def test_independence_of_table_and_position():
    """A tensor's three results have the same bits whether it is updated alone or among the other eight, first or last in the table."""
    offs, flat0, grads = _case()
    start = flat0.copy()
    for i, (n, o4) in enumerate(zip(SIZES, offs)):
        start[o4[1]:o4[1] + n] = grads[0][i]
    hp = _hyper(1e-2)

    def run(order):
        flat = torch.from_numpy(start).to(DEV)
        _launch(_table(flat, offs, order, 2), hp)
        return _bits(flat.cpu().numpy())

    together = run(range(len(SIZES)))
    backwards = run(range(len(SIZES) - 1, -1, -1))
    assert np.array_equal(together, backwards)
    untouched = _bits(start)
    for i, (n, o4) in enumerate(zip(SIZES, offs)):
        alone = run([i])
        mine = np.zeros(start.size, bool)
        for o in (o4[0], o4[2], o4[3]):
            mine[o:o + n] = True
        assert np.array_equal(alone[mine], together[mine]), f"size {n}"
        assert not np.array_equal(alone[mine], untouched[mine])
        assert np.array_equal(alone[~mine], untouched[~mine]), f"size {n}: a tensor that was not in the table changed"


@pytest.mark.gpu
def test_empty_entry_shared_gradient_and_per_tensor_step():
    """count == 0 entries (null pointers) between real ones, two tensors reading ONE gradient, and different step numbers in one call."""
    rng = np.random.default_rng(5)
    n = 1500
    host = {k: (rng.standard_normal(n) * s).astype(np.float32) for k, s in (("a", 0.05), ("b", 0.05), ("g", 1e-3))}
    m0, v0 = (np.abs(rng.standard_normal(n)) * 1e-3).astype(np.float32), (np.abs(rng.standard_normal(n)) * 1e-6).astype(np.float32)
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in host.items()}
    st = {k: (torch.from_numpy(m0).to(DEV), torch.from_numpy(v0).to(DEV)) for k in "ab"}
    t = (_lib.AdamTensor * 4)()
    t[0].count, t[0].step = 0, 1
    for e, k, step in ((t[1], "a", 4), (t[3], "b", 9)):
        e.param, e.grad, e.exp_avg, e.exp_avg_sq = dev[k].data_ptr(), dev["g"].data_ptr(), st[k][0].data_ptr(), st[k][1].data_ptr()
        e.count, e.step = n, step
    t[2].count, t[2].step = 0, 7
    _launch(t, _hyper())
    for k, step in (("a", 4), ("b", 9)):
        p1, m1, v1 = synth.adam_step_np(host[k], host["g"], m0, v0, step, lr=LR)
        assert np.array_equal(_bits(st[k][0].cpu().numpy()), _bits(m1)) and np.array_equal(_bits(st[k][1].cpu().numpy()), _bits(v1))
        assert _ulp_distance(dev[k].cpu().numpy(), p1).max() <= 1
    assert np.array_equal(_bits(dev["g"].cpu().numpy()), _bits(host["g"]))


@pytest.mark.gpu
def test_a_tensor_past_2_to_31_elements():
    """Element indices beyond 2^31 and a grid of more than 2^21 work items: every element of a constant tensor gets the one expected
    value (an element that was skipped or updated twice would not), behind a 4-byte head, and the guard elements around it stay."""
    n = (1 << 31) + 5
    vals = {"param": 0.5, "grad": 0.25, "exp_avg": 0.125, "exp_avg_sq": 0.0625}
    bufs = {k: torch.full((n + 8,), v, dtype=torch.float32, device=DEV) for k, v in vals.items()}
    t = (_lib.AdamTensor * 1)()
    e = t[0]
    e.param, e.grad, e.exp_avg, e.exp_avg_sq = (bufs[k].data_ptr() + 4 for k in ("param", "grad", "exp_avg", "exp_avg_sq"))
    e.count, e.step = n, 3
    _launch(t, _hyper(1e-2))
    one = lambda k: np.array([vals[k]], np.float32)   # noqa: E731
    p1, m1, v1 = synth.adam_step_np(one("param"), one("grad"), one("exp_avg"), one("exp_avg_sq"), 3, lr=LR, weight_decay=1e-2)
    for k, want in (("exp_avg", m1), ("exp_avg_sq", v1), ("param", p1), ("grad", one("grad"))):
        body = bufs[k][1:1 + n]
        lo, hi = float(body.min()), float(body.max())
        assert lo == hi, (k, lo, hi)
        assert _ulp_distance(np.array([lo], np.float32), want).max() <= (1 if k == "param" else 0), (k, lo, float(want[0]))
        guards = torch.cat([bufs[k][:1], bufs[k][1 + n:]]).cpu().numpy()
        assert (guards == np.float32(vals[k])).all(), k
    del bufs
    torch.cuda.empty_cache()


# ---- trajectories against torch.optim.Adam ----
def _err(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    top = np.abs(ref).max()
    if top == 0.0:      # an all-zero gradient history (a convolution bias in front of a train-mode BatchNorm): the state stays zero
        return 0.0 if not a.any() else math.inf
    return float(np.abs(a - ref).max() / top)


def _state_of(opt, params):
    """[{param, exp_avg, exp_avg_sq}] as float64 numpy arrays."""
    out = []
    for p in params:
        st = opt.state[p]
        out.append({"param": p.detach().cpu().numpy().astype(np.float64), "exp_avg": st["exp_avg"].cpu().numpy().astype(np.float64),
                    "exp_avg_sq": st["exp_avg_sq"].cpu().numpy().astype(np.float64)})
    return out


def _assert_bound(got, t32, t64, what):
    worst_g, worst_t = 0.0, 0.0
    for i, (g, a, r) in enumerate(zip(got, t32, t64)):
        for k in KEYS:
            e_g, e_t = _err(g[k], r[k]), _err(a[k], r[k])
            worst_g, worst_t = max(worst_g, e_g), max(worst_t, e_t)
            assert e_g <= max(1e-6, 2 * e_t), (what, i, k, e_g, e_t)
    print(f"{what}: worst e_hip={worst_g:.2e} e_torch32={worst_t:.2e}")


def _cpu_adam(values, grad_steps, dtype, sched=False, **kw):
    ps = [nn.Parameter(torch.from_numpy(np.array(v, np.float32)).to(dtype)) for v in values]
    opt = torch.optim.Adam(ps, foreach=False, **kw)
    sc = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.1) if sched else None
    for grads in grad_steps:
        for p, g in zip(ps, grads):
            p.grad = None if g is None else torch.from_numpy(g).to(dtype).reshape(p.shape)
        opt.step()
        if sc:
            sc.step()
    return opt, ps


def _seeded_grads(rng, values, steps):
    return [[(rng.standard_normal(v.shape) * 10.0 ** int(rng.integers(-6, 1))).astype(np.float32) for v in values] for _ in range(steps)]


def _disc_values():
    from test_discriminator import weights as disc_weights

    D = cid.DenoiseDiscriminator()
    D.load_state_dict(disc_weights("trained"), strict=True)
    return [p.detach().numpy().copy() for p in D.parameters()]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["generator", "discriminator"])
def test_the_real_parameter_sets(which):
    """Ten steps of cid.Adam(lr=1e-4) over the generator's 24 tensors / the discriminator's 16 with seeded gradients, against
    torch.optim.Adam on float64 and fp32 CPU copies."""
    if which == "generator":
        values = [np.array(v, np.float32) for v in synth.make_state_dict("default").values()]
        assert len(values) == 24 and sum(v.size for v in values) == 1827587      # CID_NUM_PARAM_ELEMS
    else:
        values = _disc_values()
        assert len(values) == 16
    grads = _seeded_grads(np.random.default_rng(11), values, 10)
    ps = [nn.Parameter(torch.from_numpy(v.copy()).to(DEV)) for v in values]
    opt = cid.Adam(ps, lr=LR)
    dev_grads = [[torch.from_numpy(g).to(DEV) for g in gs] for gs in grads]
    for gs in dev_grads:
        for p, g in zip(ps, gs):
            p.grad = g
        opt.step()
    assert all(float(opt.state[p]["step"]) == 10 for p in ps)
    o64, p64 = _cpu_adam(values, grads, torch.float64, lr=LR)
    o32, p32 = _cpu_adam(values, grads, torch.float32, lr=LR)
    _assert_bound(_state_of(opt, ps), _state_of(o32, p32), _state_of(o64, p64), which)


SMALL = ((7, 3, 3, 3), (65,), (64, 16, 2, 2), (4097,))


def _small_values():
    rng = np.random.default_rng(3)
    return [(rng.standard_normal(s) * 0.05).astype(np.float32) for s in SMALL]


def _gpu_run(opt_cls, values, grad_steps, load=None, **kw):
    """Steps of `opt_cls` on GPU copies under StepLR(step_size=2, gamma=0.1); `load` = (optimizer state_dict, scheduler state_dict)."""
    ps = [nn.Parameter(torch.from_numpy(np.array(v, np.float32)).to(DEV)) for v in values]
    opt = opt_cls(ps, **kw)
    sc = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.1)
    if load is not None:
        opt.load_state_dict(load[0])
        sc.load_state_dict(load[1])
    for grads in grad_steps:
        for p, g in zip(ps, grads):
            p.grad = torch.from_numpy(g).to(DEV)
        opt.step()
        sc.step()
    return opt, sc, ps


@pytest.mark.gpu
@pytest.mark.parametrize("direction", ["to_torch", "from_torch", "from_numpy"])
def test_state_dict_interchange(direction, tmp_path):
    """Three steps with one class, its state_dict loaded into the other, two more steps under StepLR(step_size=2, gamma=0.1) (the
    learning rates 1e-4, 1e-4, 1e-5, 1e-5, 1e-6 reach the kernel through the group); from_numpy: the state goes through a checkpoint
    file written as the trainer's save_checkpoint does and read by ckpt.read_checkpoint, whose tensors are numpy arrays."""
    values = _small_values()
    grads = _seeded_grads(np.random.default_rng(21), values, 5)
    first, second = (cid.Adam, torch.optim.Adam) if direction == "to_torch" else (torch.optim.Adam, cid.Adam)
    o1, s1, p1 = _gpu_run(first, values, grads[:3], lr=LR, weight_decay=1e-2)
    assert o1.param_groups[0]["lr"] == pytest.approx(1e-5)
    sd = copy.deepcopy(o1.state_dict())      # load_state_dict does not copy tensors that already have the right type and device
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values())
    if direction == "to_torch":
        ref = torch.optim.Adam([nn.Parameter(torch.zeros(1, device=DEV))], lr=LR, weight_decay=1e-2)
        ref.zero_grad()
        ref.param_groups[0]["params"][0].grad = torch.zeros(1, device=DEV)
        ref.step()
        (rst,), (st, *_) = ref.state_dict()["state"].values(), sd["state"].values()
        for k in ("step", "exp_avg", "exp_avg_sq"):     # types and devices are what the installed torch.optim.Adam uses
            assert st[k].dtype == rst[k].dtype and st[k].device.type == rst[k].device.type and st[k].dim() == (0 if k == "step" else st[k].dim())
        assert set(sd["param_groups"][0]) - {"initial_lr"} == set(ref.state_dict()["param_groups"][0])
    if direction == "from_numpy":
        path = str(tmp_path / "denoise_epoch_3.pth")
        torch.save({"g_optimizer": sd, "epoch": 3}, path)
        sd = ckpt.read_checkpoint(path)["g_optimizer"]
        assert isinstance(sd["state"][0]["exp_avg"], np.ndarray) and isinstance(sd["state"][0]["step"], np.ndarray)
    mid = [p.detach().cpu().numpy() for p in p1]
    o2, s2, p2 = _gpu_run(second, mid, grads[3:], load=(sd, s1.state_dict()), lr=LR, weight_decay=1e-2)
    assert o2.param_groups[0]["lr"] == pytest.approx(1e-6)
    assert all(float(o2.state[p]["step"]) == 5 for p in p2)
    st = o2.state[p2[0]]
    assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and st["exp_avg"].device.type == "cuda"
    # the one that kept going
    o1c, _, p1c = _gpu_run(first, mid, grads[3:], load=(copy.deepcopy(o1.state_dict()), s1.state_dict()), lr=LR, weight_decay=1e-2)
    o64, p64 = _cpu_adam(values, grads, torch.float64, sched=True, lr=LR, weight_decay=1e-2)
    o32, p32 = _cpu_adam(values, grads, torch.float32, sched=True, lr=LR, weight_decay=1e-2)
    _assert_bound(_state_of(o2, p2), _state_of(o32, p32), _state_of(o64, p64), f"{direction}: loaded")
    _assert_bound(_state_of(o1c, p1c), _state_of(o32, p32), _state_of(o64, p64), f"{direction}: continued")


@pytest.mark.gpu
def test_step_skips_parameters_without_gradient_and_reads_lr_every_call():
    values = _small_values()
    grads = _seeded_grads(np.random.default_rng(8), values, 4)
    grads[1][2] = None
    grads[2][2] = None
    ps = [nn.Parameter(torch.from_numpy(v.copy()).to(DEV)) for v in values]
    opt = cid.Adam([{"params": ps[:2]}, {"params": ps[2:], "lr": 3e-4}], lr=LR)
    lrs = (1.0, 0.5, 2.0, 1.0)
    for s, gs in enumerate(grads):
        for p, g in zip(ps, gs):
            p.grad = None if g is None else torch.from_numpy(g).to(DEV)
        opt.param_groups[0]["lr"] = LR * lrs[s]
        held = ps[2].detach().clone()
        opt.step()
        if gs[2] is None:
            assert torch.equal(ps[2].detach(), held)
    assert [float(opt.state[p]["step"]) for p in ps] == [4, 4, 2, 4]
    want = []
    for i, v in enumerate(values):
        p, m, w, t = v.copy(), np.zeros_like(v), np.zeros_like(v), 0
        for s in range(4):
            if grads[s][i] is None:
                continue
            t += 1
            p, m, w = synth.adam_step_np(p, grads[s][i], m, w, t, lr=LR * lrs[s] if i < 2 else 3e-4)
        want.append(p)
    for p, w in zip(ps, want):
        np.testing.assert_allclose(p.detach().cpu().numpy(), w, rtol=0, atol=float(np.abs(w).max()) * 1e-6)


@pytest.mark.gpu
def test_step_refuses_before_any_launch():
    good = nn.Parameter(torch.ones(8, device=DEV))
    good.grad = torch.ones(8, device=DEV)

    def unchanged(opt):
        return torch.equal(good.detach(), torch.ones(8, device=DEV)) and not opt.state[good]

    with pytest.raises(RuntimeError, match="closure"):
        cid.Adam([good]).step(lambda: 0.0)
    for bad in (nn.Parameter(torch.ones(8, device=DEV, dtype=torch.float64)), nn.Parameter(torch.ones(8)),
                nn.Parameter(torch.ones(4, 8, device=DEV).t())):
        bad.grad = torch.ones_like(bad)
        opt = cid.Adam([good, bad])
        with pytest.raises(RuntimeError, match="contiguous float32"):
            opt.step()
        assert unchanged(opt)
    emb = nn.Embedding(4, 2, sparse=True).to(DEV)
    emb(torch.tensor([1], device=DEV)).sum().backward()
    opt = cid.Adam([good, emb.weight])
    with pytest.raises(RuntimeError, match="sparse"):
        opt.step()
    assert unchanged(opt)
    with pytest.raises(ValueError):
        cid.Adam([good], betas=(0.9, 1.0))


# ---- with the modules: training.py:410-426 ----
def _modules(seed=0):
    torch.manual_seed(seed)
    G = cid.load(None, autograd=True).train()
    D = cid.load_discriminator(None, autograd=True).train()
    xn, cn, _ = synth.make_batch(2, 32, 32, first_index=60)
    return G, D, torch.from_numpy(xn).to(DEV), torch.from_numpy(cn).to(DEV)


def _trainer_step(G, D, g_optimizer, d_optimizer, noisy_img, clean_img, before_step=None):
    bce_loss, mse_loss = nn.BCELoss(), nn.MSELoss()
    d_optimizer.zero_grad()
    denoised_img = G(noisy_img)
    real_pred = D(clean_img)
    fake_pred = D(denoised_img.detach())
    d_loss = bce_loss(real_pred, torch.ones_like(real_pred)) + bce_loss(fake_pred, torch.zeros_like(fake_pred))
    d_loss.backward()
    if before_step:
        before_step("d")
    d_optimizer.step()

    g_optimizer.zero_grad()
    fake_pred = D(denoised_img)
    content_loss = mse_loss(denoised_img, clean_img)
    adv_loss = bce_loss(fake_pred, torch.ones_like(fake_pred))
    g_loss = content_loss + 0.001 * adv_loss
    g_loss.backward()
    if before_step:
        before_step("g")
    g_optimizer.step()
    return content_loss, d_loss


@pytest.mark.gpu
def test_one_trainer_step_with_the_modules():
    G, D, noisy, clean = _modules()
    g_opt, d_opt = cid.Adam(G.parameters(), lr=LR), cid.Adam(D.parameters(), lr=LR)
    G(noisy), D(clean)                       # workspaces and first packs exist before the synchronisation watch below
    snap = {}

    def before_step(which):
        mod = G if which == "g" else D
        snap[which] = ([p.detach().clone() for p in mod.parameters()], [p.grad.detach().clone() for p in mod.parameters()],
                       [p._version for p in mod.parameters()])
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")     # only the optimizer step runs under it: the next module call resets it

    mode = torch.cuda.get_sync_debug_mode()
    real_g, real_d = g_opt.step, d_opt.step

    def watched(real):
        def step():
            try:
                real()
            finally:
                torch.cuda.set_sync_debug_mode(mode)
        return step

    g_opt.step, d_opt.step = watched(real_g), watched(real_d)
    try:
        _trainer_step(G, D, g_opt, d_opt, noisy, clean, before_step)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
        g_opt.step, d_opt.step = real_g, real_d
    for which, mod, n in (("g", G, 24), ("d", D, 16)):
        params = list(mod.parameters())
        values, grads, versions = snap[which]
        assert len(params) == n and all(p._version > v for p, v in zip(params, versions))
        vals, gs = [v.cpu().numpy() for v in values], [[g.cpu().numpy() for g in grads]]
        o64, p64 = _cpu_adam(vals, gs, torch.float64, lr=LR)
        o32, p32 = _cpu_adam(vals, gs, torch.float32, lr=LR)
        opt = g_opt if which == "g" else d_opt
        _assert_bound(_state_of(opt, params), _state_of(o32, p32), _state_of(o64, p64), f"module step 1 ({which})")
    # the repack saw the update: the next forward equals a fresh module's at the same state_dict, bit for bit
    with torch.no_grad():
        y = G(noisy)
        fresh = cid.load({k: v.detach().cpu() for k, v in G.state_dict().items()})
        assert torch.equal(y, fresh(noisy))
        D.eval()
        pd = D(clean)
        fresh_d = cid.load_discriminator({k: v.detach().cpu() for k, v in D.state_dict().items()})
        assert torch.equal(pd, fresh_d(clean))
        D.train()
    # a step between a differentiable forward and its backward
    loss = nn.MSELoss()(G(noisy), clean)
    g_opt.step()
    with pytest.raises(RuntimeError, match="modified in place"):
        loss.backward()
    loss = D(clean).sum()
    d_opt.step()
    with pytest.raises(RuntimeError, match="modified in place"):
        loss.backward()


@pytest.mark.gpu
def test_ten_trainer_steps_lower_the_content_loss():
    G, D, noisy, clean = _modules()
    g_opt, d_opt = cid.Adam(G.parameters(), lr=LR), cid.Adam(D.parameters(), lr=LR)
    content, dl = [], []
    for _ in range(10):
        c, d = _trainer_step(G, D, g_opt, d_opt, noisy, clean)
        content.append(float(c))
        dl.append(float(d))
    print("content_loss", " ".join(f"{v:.6f}" for v in content))
    print("d_loss", " ".join(f"{v:.6f}" for v in dl))
    assert all(math.isfinite(v) for v in content + dl)
    assert content[-1] < content[0]
