"""No-GPU checks of the device Adam step: the numpy restatement of its expression tree (synth.adam_step_np) against torch.optim.Adam on
the CPU, and every argument error of cid_adam_step, which is found before anything is launched."""
import ctypes
import math

import numpy as np
import pytest
import torch

from celebrity_image_denoiser_amd import _lib, synth

SIZES = (1, 3, 63, 64, 65, 257, 4097, 36864)
STEPS = 10
SKIP = {3: (3, 4)}   # tensor index -> the (1-based) steps at which it has no gradient


def _case(seed=20240):
    rng = np.random.default_rng(seed)
    params = [(rng.standard_normal(n) * 0.05).astype(np.float32) for n in SIZES]
    grads = [[(rng.standard_normal(n) * 10.0 ** int(rng.integers(-6, 1))).astype(np.float32) for n in SIZES] for _ in range(STEPS)]
    return params, grads


def _torch_adam(params, grads, dtype, weight_decay):
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(dtype)) for p in params]
    opt = torch.optim.Adam(ps, lr=1e-4, weight_decay=weight_decay, foreach=False)
    for s in range(STEPS):
        for i, p in enumerate(ps):
            p.grad = None if (s + 1) in SKIP.get(i, ()) else torch.from_numpy(grads[s][i]).to(dtype)
        opt.step()
    return [{"param": p.detach().numpy().astype(np.float64), "exp_avg": opt.state[p]["exp_avg"].numpy().astype(np.float64),
             "exp_avg_sq": opt.state[p]["exp_avg_sq"].numpy().astype(np.float64), "step": float(opt.state[p]["step"])} for p in ps]


def _err(a, ref):
    return float(np.abs(a - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_restatement_against_torch(weight_decay):
    """e(T) = max|T - T64| / max|T64| against torch.optim.Adam on float64 copies: the restatement's error is within
    max(1e-6, 2 e(torch fp32)) for every parameter, exp_avg and exp_avg_sq after ten steps."""
    params, grads = _case()
    t64 = _torch_adam(params, grads, torch.float64, weight_decay)
    t32 = _torch_adam(params, grads, torch.float32, weight_decay)
    worst = {"restatement": 0.0, "torch32": 0.0}
    for i, p0 in enumerate(params):
        p, m, v, t = p0.copy(), np.zeros_like(p0), np.zeros_like(p0), 0
        for s in range(STEPS):
            if (s + 1) in SKIP.get(i, ()):
                continue
            t += 1
            p, m, v = synth.adam_step_np(p, grads[s][i], m, v, t, lr=1e-4, weight_decay=weight_decay)
            assert p.dtype == m.dtype == v.dtype == np.float32
        assert t == t64[i]["step"] == t32[i]["step"] == (8 if i in SKIP else 10)
        for key, val in (("param", p), ("exp_avg", m), ("exp_avg_sq", v)):
            e_r, e_t = _err(val.astype(np.float64), t64[i][key]), _err(t32[i][key], t64[i][key])
            worst["restatement"], worst["torch32"] = max(worst["restatement"], e_r), max(worst["torch32"], e_t)
            assert e_r <= max(1e-6, 2 * e_t), (SIZES[i], key, e_r, e_t)
    print(f"weight_decay={weight_decay}: worst e_restatement={worst['restatement']:.2e} e_torch32={worst['torch32']:.2e}")


def test_restatement_leaves_inputs_and_checks_t():
    p = np.full(5, 0.25, np.float32)
    g, m, v = np.full(5, 0.5, np.float32), np.zeros(5, np.float32), np.zeros(5, np.float32)
    p1, m1, v1 = synth.adam_step_np(p, g, m, v, 1, lr=1e-3)
    assert (p == 0.25).all() and (m == 0).all() and (v == 0).all()
    # step 1 of Adam moves every element by lr against the gradient's sign (up to eps)
    np.testing.assert_allclose(p1, 0.25 - 1e-3, rtol=1e-6)
    assert m1[0] == np.float32(0.5 * (1.0 - 0.9)) and v1[0] == np.float32((1.0 - 0.999) * 0.5 * 0.5)
    with pytest.raises(ValueError):
        synth.adam_step_np(p, g, m, v, 0)


# ---- cid_adam_step's argument errors: host pointers that are never dereferenced, no GPU ----
A = 1 << 20   # a 16-byte-aligned fake address


def _table(*entries):
    t = (_lib.AdamTensor * len(entries))()
    for e, (param, grad, m, v, count, step) in zip(t, entries):
        e.param, e.grad, e.exp_avg, e.exp_avg_sq, e.count, e.step = param, grad, m, v, count, step
    return t


def _entry(i=0, count=100, step=1, **over):
    base = A + i * 0x10000
    d = {"param": base, "grad": base + 0x1000, "m": base + 0x2000, "v": base + 0x3000}
    d.update(over)
    return (d["param"], d["grad"], d["m"], d["v"], count, step)


def _hyper(**over):
    d = {"lr": 1e-4, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "weight_decay": 0.0}
    d.update(over)
    return _lib.AdamHyper(d["lr"], d["beta1"], d["beta2"], d["eps"], d["weight_decay"])


def _call(table, n=None, hp=None):
    return _lib.lib().cid_adam_step(table, len(table) if n is None else n, ctypes.byref(hp or _hyper()), None)


INVALID = 1


def test_null_arguments_and_tensor_count():
    L = _lib.lib()
    t = _table(_entry())
    assert L.cid_adam_step(None, 1, ctypes.byref(_hyper()), None) == INVALID
    assert L.cid_adam_step(t, 1, None, None) == INVALID
    assert _call(t, n=0) == INVALID and _call(t, n=-1) == INVALID
    big = _table(*[_entry(i) for i in range(_lib.CID_ADAM_MAX_TENSORS + 1)])
    assert _call(big) == INVALID


@pytest.mark.parametrize("field", ["param", "grad", "m", "v"])
def test_null_or_misaligned_pointer(field):
    assert _call(_table(_entry(**{field: None}))) == INVALID
    for mis in (1, 2, 3):
        assert _call(_table(_entry(**{field: A + 0x8000 + mis}))) == INVALID
    assert _call(_table(_entry(0), _entry(1, **{field: None}))) == INVALID      # in a later entry


def test_count_and_step():
    assert _call(_table(_entry(count=-1))) == INVALID
    assert _call(_table(_entry(step=0))) == INVALID
    assert _call(_table(_entry(step=-3))) == INVALID
    assert _call(_table(_entry(count=0, step=0, param=None, grad=None, m=None, v=None))) == INVALID   # step counts even where count == 0
    assert _call(_table(_entry(0), _entry(1, count=-5))) == INVALID


def test_empty_entries_launch_nothing():
    """count == 0 is a no-op entry whose pointers are not looked at: a table of them returns CID_OK without a launch (no GPU here)."""
    t = _table(_entry(count=0, param=None, grad=None, m=None, v=None), _entry(count=0, param=3, grad=5, m=7, v=9))
    assert _call(t) == _lib.CID_OK


@pytest.mark.parametrize("over", [
    {"lr": -1e-4}, {"lr": math.nan}, {"lr": math.inf},
    {"beta1": 1.0}, {"beta1": -0.1}, {"beta1": math.nan}, {"beta1": 1.5},
    {"beta2": 1.0}, {"beta2": -1e-9}, {"beta2": math.inf},
    {"eps": -1e-8}, {"eps": math.nan}, {"eps": math.inf},
    {"weight_decay": -1e-2}, {"weight_decay": math.nan}, {"weight_decay": math.inf},
])
def test_hyper_parameters(over):
    assert _call(_table(_entry()), hp=_hyper(**over)) == INVALID


def test_overlapping_ranges():
    n = 100   # 400 bytes per range
    assert _call(_table(_entry(m=A))) == INVALID                                       # exp_avg is the parameter
    assert _call(_table(_entry(v=A + 0x2000 + 396))) == INVALID                        # exp_avg_sq starts in exp_avg's last element
    assert _call(_table(_entry(grad=A + 200))) == INVALID                              # the gradient lies inside the parameter
    assert _call(_table(_entry(grad=A - 396))) == INVALID                              # the gradient's last element is the parameter's first
    assert _call(_table(_entry(0), _entry(1, param=A + 0x3000 + 4 * (n - 1)))) == INVALID   # across entries: written / written
    assert _call(_table(_entry(0), _entry(1, grad=A + 0x2000))) == INVALID             # across entries: a gradient on another tensor's exp_avg
    assert _call(_table(_entry(0), _entry(0))) == INVALID                              # the same tensor twice
    assert _call(_table(_entry(0, count=0x5000))) == INVALID                           # long enough to run into its own gradient


# ---- the kernel's own table and work-item code on the CPU (cid_debug_adam_step_host) against the restatement ----
class _HostFlat:
    """A 16-byte-aligned float32 host buffer with the data_ptr() the GPU tests' table builder asks of a device tensor."""

    def __init__(self, values):
        raw = np.empty(values.size + 8, np.float32)
        first = (-raw.ctypes.data % 16) // 4
        self.a = raw[first:first + values.size]
        self.a[:] = values

    def data_ptr(self):
        return self.a.ctypes.data


def _host_step(flat, offs, order, step, weight_decay):
    import test_adam as T

    t = T._table(flat, offs, order, step)
    hp = T._hyper(weight_decay)
    assert _lib.lib().cid_debug_adam_step_host(t, len(t), ctypes.byref(hp)) == _lib.CID_OK


@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_work_item_code_on_the_host_equals_the_restatement(weight_decay):
    """tests/test_adam.py's identity case (nine tensors at mixed alignments in one flat buffer, NaN canaries, three steps) through
    the kernel's __host__ __device__ code on the CPU: exp_avg and exp_avg_sq bit for bit, the parameter under the GPU test's
    condition (one ulp at no more than ceil(1e-6 count) elements), canaries and gradients untouched."""
    import test_adam as T

    offs, flat0, grads = T._case()
    inside = np.zeros(flat0.size, bool)
    for n, o4 in zip(T.SIZES, offs):
        for o in o4:
            inside[o:o + n] = True
    before = flat0.copy()
    for s in range(3):
        for i, (n, o4) in enumerate(zip(T.SIZES, offs)):
            before[o4[1]:o4[1] + n] = grads[s][i]
        flat = _HostFlat(before)
        _host_step(flat, offs, range(len(T.SIZES)), s + 1, weight_decay)
        after = flat.a.copy()
        assert np.array_equal(T._bits(after)[~inside], T._bits(flat0)[~inside]), "a canary was written"
        for i, (n, (po, go, mo, vo)) in enumerate(zip(T.SIZES, offs)):
            assert np.array_equal(T._bits(after[go:go + n]), T._bits(grads[s][i]))
            p1, m1, v1 = synth.adam_step_np(before[po:po + n], grads[s][i], before[mo:mo + n], before[vo:vo + n], s + 1, lr=T.LR,
                                            weight_decay=weight_decay)
            assert np.array_equal(T._bits(after[mo:mo + n]), T._bits(m1)), (s + 1, n, "exp_avg")
            assert np.array_equal(T._bits(after[vo:vo + n]), T._bits(v1)), (s + 1, n, "exp_avg_sq")
            d = T._ulp_distance(after[po:po + n], p1)
            assert d.max() <= 1 and int((d > 0).sum()) <= math.ceil(1e-6 * n), (s + 1, n, "param")
        before = after


def test_work_item_code_on_the_host_is_independent_of_the_table():
    import test_adam as T

    offs, flat0, grads = T._case()
    start = flat0.copy()
    for i, (n, o4) in enumerate(zip(T.SIZES, offs)):
        start[o4[1]:o4[1] + n] = grads[0][i]

    def run(order):
        flat = _HostFlat(start)
        _host_step(flat, offs, order, 2, 1e-2)
        return T._bits(flat.a.copy())

    together = run(range(len(T.SIZES)))
    assert np.array_equal(together, run(range(len(T.SIZES) - 1, -1, -1)))
    for i, (n, o4) in enumerate(zip(T.SIZES, offs)):
        alone = run([i])
        mine = np.zeros(start.size, bool)
        for o in (o4[0], o4[2], o4[3]):
            mine[o:o + n] = True
        assert np.array_equal(alone[mine], together[mine]) and np.array_equal(alone[~mine], T._bits(start)[~mine]), n
