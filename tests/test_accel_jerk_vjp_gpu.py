"""The differentiable Hermite force on the GPU (csrc/direct_hermite_grad.hip, nbd.autograd.direct_accel_jerk,
HermiteSimulator.compute_accelerations_and_jerks() under autograd) against the fp64 closed form of
tests/accel_jerk_vjp_oracle.py.

float64: inside the bar of tests/hermite_f64_oracle.py, |got - ref| <= (T + 32) 2^-53 sum|terms|, T = 44 n for a component
of dL/dx, 8 n for dL/dv and 15 n for dL/dm; no input is fp32-representable.
float32: on fp32-representable inputs against the same oracle; the yardstick is torch's CPU fp32 autograd through the
dense statement of (a, j), computed here, and the bars are four times max(the yardstick's own figure, 2^-23) -- in
global_rel and row_rel of dL/dx and dL/dv, global_rel of dL/dm and, elementwise, max |err| / sum|terms| of dL/dm -- next
to the project's 1e-5 (global) / 1e-4 (row).
Every workspace is NaN-filled before each call. Measured on the MI355X: NOTES.md, "K-HVJP"."""
import functools

import numpy as np
import pytest
import torch

import accel_jerk_vjp_oracle as jo
import hermite_f64_oracle as fo
from conftest import global_rel, load_golden, row_rel

pytestmark = pytest.mark.gpu

G, EPS = 1.0, 0.05
SIZES_F64 = [1, 2, 3, 63, 64, 65, 130, 448, 449, 1000, 5000]      # 448 / 449: one slab -> two (nbd_hermite_f64_plan)
SIZES_F32 = [1, 2, 63, 64, 65, 127, 129, 500, 2048]
U23 = 2.0 ** -23
F32, F64 = torch.float32, torch.float64
NAMES = ("dL/dx", "dL/dv", "dL/dm")
TERMS = (jo.T_POS, jo.T_VEL, jo.T_MASS)


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, device, dtype=F64):
    return torch.tensor(np.asarray(a, np.float64), dtype=dtype, device=device)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _case(name, eps=EPS, fp32=False):
    """(x, v, m, cota, cotj, g, eps, (dL/dx, dL/dv, dL/dm), (sum|terms| of each)), computed once and never written to.
    name: a size (Plummer, masses U(0.5, 1.5) / n, velocities N(0, 0.3^2), N(0, 1) cotangents) or a golden case
    (perturbed, so not fp32-representable)."""
    if isinstance(name, int):
        x, v, m, ca, cj = jo.case(name, seed=200 + name, fp32=fp32)
        g = G
    else:
        gd = load_golden(name)
        x, v, m = fo.perturbed(gd["pos"], gd["vel"], gd["mass"], 5)
        rng = np.random.default_rng(6)
        ca, cj = rng.standard_normal(x.shape), rng.standard_normal(x.shape)
        g, eps = float(gd["g_const"]), float(gd["softening"])
    out = jo.accel_jerk_vjp(x, v, m, ca, cj, g, eps * eps)
    return _frozen(x, v, m, ca, cj) + (g, eps, _frozen(*out[:3]), _frozen(*out[3:]))


@functools.lru_cache(maxsize=None)
def _partial(name, which):
    """The oracle of case `name` (float64) with one cotangent only: (values, sum|terms|)."""
    x, v, m, ca, cj, g, eps = _case(name)[:7]
    out = jo.accel_jerk_vjp(x, v, m, ca if which == "alpha" else None, cj if which == "beta" else None, g, eps * eps)
    return _frozen(*out[:3]), _frozen(*out[3:])


def _figures(got, ref, sm):
    """(global_rel, row_rel of dL/dx; of dL/dv; global_rel of dL/dm; max |err| / sum|terms| of dL/dm)"""
    live = sm > 0
    elem = float((np.abs(got[2] - ref[2])[live] / sm[live]).max()) if live.any() else 0.0
    return (global_rel(got[0], ref[0]), row_rel(got[0], ref[0]), global_rel(got[1], ref[1]), row_rel(got[1], ref[1]),
            global_rel(got[2], ref[2]), elem)


FIGURES = ("dL/dx global_rel", "dL/dx row_rel", "dL/dv global_rel", "dL/dv row_rel", "dL/dm global_rel",
           "dL/dm max|err|/sum|terms|")
PROJECT = (1e-5, 1e-4, 1e-5, 1e-4, 1e-5, None)


@functools.lru_cache(maxsize=None)
def _yardstick(n, eps=EPS):
    """The figures of torch's CPU fp32 autograd through the dense statement on the fp32 case n, against the oracle (the
    statement keeps its diagonal finite, so eps = 0 is finite too)."""
    x, v, m, ca, cj, g, eps, ref, sums = _case(n, eps, True)
    return _figures(jo.torch_vjp(x, v, m, ca, cj, g, eps, F32), ref, sums[2])


def _pack(dtype, x, v, m, ca, cj, device):
    """(rows, vrows, cota rows, cotj rows): the pack entry of the dtype, a cotangent passed as the velocities."""
    from nbd import direct
    n = x.shape[0]
    alloc = direct.alloc_rows_f64 if dtype == F64 else (lambda k, d: torch.zeros_like(direct.alloc_posm(k, d)))
    pack = direct.hermite_f64_pack if dtype == F64 else direct.hermite_pack
    xt, vt, mt = (_dev(a, device, dtype) for a in (x, v, m))
    rows, vrows, spare = alloc(n, device), alloc(n, device), alloc(n, device)
    pack(xt, vt, mt, rows, vrows)
    cots = []
    for c in (ca, cj):
        if c is None:
            cots.append(None)
            continue
        crow = alloc(n, device)
        pack(xt, _dev(c, device, dtype), mt, spare, crow)
        cots.append(crow)
    return rows, vrows, cots[0], cots[1]


def _vjp64(x, v, m, ca, cj, g, eps2, device, slabs=0, fill=float("nan"), **want):
    from nbd import direct
    n = x.shape[0]
    rows = _pack(F64, x, v, m, ca, cj, device)
    ws = direct.accel_jerk_vjp_f64_workspace(n, device, slabs)
    ws.view(F64).fill_(fill)
    return direct.accel_jerk_vjp_f64(*rows, n, eps2, g, workspace=ws, slabs=slabs, **want)


def _vjp32(x, v, m, ca, cj, g, eps2, device, fill=float("nan"), **want):
    from nbd import direct
    n = x.shape[0]
    rows = _pack(F32, x, v, m, ca, cj, device)
    ws = direct.accel_jerk_vjp_workspace(n, device)
    ws.view(F32).fill_(fill)
    return direct.accel_jerk_vjp(*rows, n, direct.f32(eps2), direct.f32(g), workspace=ws, **want)


def _check64(tag, got, ref, sums, n):
    fig = []
    for k in range(3):
        ok, f = fo.within(_np(got[k]), ref[k], TERMS[k] * n, sums[k])
        fig.append((ok, f))
    print(f"{tag}: |got - ref| / bar: " + ", ".join(f"{NAMES[k]} {fig[k][1]:.3f}" for k in range(3)))
    assert all(ok for ok, _ in fig), (tag, fig)


def _check32(tag, got, case, yard):
    """The project's bars and, with a yardstick, four times max(its own figure, 2^-23) in each measure."""
    ref, sums = case[7], case[8]
    arrays = [_np(t).astype(np.float64) for t in got]
    ours = _figures(arrays, ref, sums[2])
    for k, nm in enumerate(FIGURES):
        line = f"{tag}: {nm}: ours {ours[k]:.2e}"
        if yard is not None:
            line += f", torch fp32 {yard[k]:.2e}, ratio to the bar {ours[k] / (4 * max(yard[k], U23)):.3f}"
        print(line)
    assert all(np.isfinite(a).all() for a in arrays)
    for k, nm in enumerate(FIGURES):
        if PROJECT[k] is not None:
            assert ours[k] <= PROJECT[k], (tag, nm, ours[k])
    if yard is not None:
        for k, nm in enumerate(FIGURES):
            assert ours[k] <= 4 * max(yard[k], U23), (tag, nm, ours[k], yard[k])


# ---------------------------------------------------------------- the kernels against the oracle
@pytest.mark.parametrize("name", SIZES_F64 + ["direct_plummer_n300_ragged_mass", "direct_spiral_n25"])
def test_f64_at_the_bar(gpu_device, name):
    case = _case(name)
    x, v, m, ca, cj, g, eps, ref, sums = case
    for a in (x, v, m[m != 0]):
        assert not np.any(a.astype(np.float32).astype(np.float64) == a)
    if not isinstance(name, int):
        assert (m == 0).any() == ("ragged_mass" in name)
    got = _vjp64(x, v, m, ca, cj, g, eps * eps, gpu_device)
    assert all(t.dtype == F64 for t in got)
    assert got[0].shape == x.shape and got[1].shape == x.shape and got[2].shape == m.shape
    _check64(f"f64 n={name}", got, ref, sums, x.shape[0])
    if name == 1:
        assert not any(_np(t).any() for t in got)               # no partner: exact zeros


@pytest.mark.parametrize("n,slabs", [(130, 1), (1000, 1), (1000, 3), (5000, 64)])
def test_f64_with_an_explicit_split(gpu_device, n, slabs):
    """Several chunks per wave (both staging buffers and the three-load wait count reused: 1000 / 1 gives 4 chunks per
    wave, 1000 / 3 an uneven split), waves without a chunk (130 / 1; 5000 / 64)."""
    x, v, m, ca, cj, g, eps, ref, sums = _case(n)
    got = _vjp64(x, v, m, ca, cj, g, eps * eps, gpu_device, slabs)
    _check64(f"f64 n={n} slabs={slabs}", got, ref, sums, n)


@pytest.mark.parametrize("n", SIZES_F32)
def test_f32_against_the_oracle_and_the_yardstick(gpu_device, n):
    case = _case(n, EPS, True)
    x, v, m, ca, cj, g, eps = case[:7]
    for a in (x, v, m, ca, cj):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    got = _vjp32(x, v, m, ca, cj, g, eps * eps, gpu_device)
    assert all(t.dtype == F32 for t in got)
    _check32(f"f32 n={n}", got, case, _yardstick(n))
    if n == 1:
        assert not any(_np(t).any() for t in got)


def test_f32_n5000_against_the_oracle(gpu_device):
    """The project's bars only: the dense yardstick is too large here. 79 chunks, 40 groups."""
    case = _case(5000, EPS, True)
    x, v, m, ca, cj, g, eps = case[:7]
    _check32("f32 n=5000", _vjp32(x, v, m, ca, cj, g, eps * eps, gpu_device), case, None)


@pytest.mark.parametrize("n", [65, 130])
def test_no_self_term_leaks_at_a_tiny_softening(gpu_device, n):
    """eps = 1e-6: the un-masked path with s^3 up to 1e18 on the diagonal. A residual h_ii in dL/dv, or an i == j term of
    any other sum, would miss the bars by many orders of magnitude."""
    eps = 1e-6
    x, v, m, ca, cj, g, _, ref, sums = _case(n, eps)
    _check64(f"f64 n={n} eps=1e-6", _vjp64(x, v, m, ca, cj, g, eps * eps, gpu_device), ref, sums, n)
    case32 = _case(n, eps, True)
    x, v, m, ca, cj, g = case32[:6]
    _check32(f"f32 n={n} eps=1e-6", _vjp32(x, v, m, ca, cj, g, eps * eps, gpu_device), case32, _yardstick(n, eps))


@pytest.mark.parametrize("n", [64, 130])
def test_zero_softening_is_the_closed_form_over_the_other_bodies(gpu_device, n):
    """eps = 0 (every chunk index-masked): finite, and the sum over j != i."""
    x, v, m, ca, cj, g, _, ref, sums = _case(n, 0.0)
    assert np.unique(x, axis=0).shape[0] == n
    got = _vjp64(x, v, m, ca, cj, g, 0.0, gpu_device)
    assert all(torch.isfinite(t).all() for t in got)
    _check64(f"f64 n={n} eps=0", got, ref, sums, n)
    case32 = _case(n, 0.0, True)
    x, v, m, ca, cj, g = case32[:6]
    assert np.unique(x, axis=0).shape[0] == n
    _check32(f"f32 n={n} eps=0", _vjp32(x, v, m, ca, cj, g, 0.0, gpu_device), case32, _yardstick(n, 0.0))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_without_the_jerk_cotangent_the_bits_are_accel_vjp(gpu_device, dtype):
    from nbd import direct
    n = 1000
    x, v, m, ca, cj, g, eps = _case(n, EPS, dtype == F32)[:7]
    run = _vjp32 if dtype == F32 else _vjp64
    gp, gv, gm = run(x, v, m, ca, None, g, eps * eps, gpu_device)
    rows, _, crow, _ = _pack(dtype, x, v, m, ca, None, gpu_device)
    if dtype == F32:
        rp, rm = direct.accel_vjp(rows, crow, n, direct.f32(eps * eps), direct.f32(g))
    else:
        rp, rm = direct.accel_vjp_f64(rows, crow, n, eps * eps, g)
    assert torch.equal(gp, rp) and torch.equal(gm, rm)
    assert not _np(gv).any()
    # only dL/dv asked for, and no beta: zeros, nothing else formed
    only = run(x, v, m, ca, None, g, eps * eps, gpu_device, want_pos=False, want_mass=False)
    assert only[0] is None and only[2] is None and not _np(only[1]).any()


@pytest.mark.parametrize("n,slabs", [(130, 0), (1000, 3)])
def test_without_the_acceleration_cotangent(gpu_device, n, slabs):
    """cota = None: only the new kernel runs. Against the oracle with beta alone at the bar, and equal to the full call
    minus the alpha call: full = fl(beta part + alpha part), so the difference is within 2^-53 (|full| + |alpha part|)
    <= 2 2^-53 sum|terms| of the full call, far inside its bar."""
    x, v, m, ca, cj, g, eps, ref, sums = _case(n)
    beta = _vjp64(x, v, m, None, cj, g, eps * eps, gpu_device, slabs)
    bref, bsums = _partial(n, "beta")
    _check64(f"f64 n={n} slabs={slabs} beta only", beta, bref, bsums, n)
    full = _vjp64(x, v, m, ca, cj, g, eps * eps, gpu_device, slabs)
    alpha = _vjp64(x, v, m, ca, None, g, eps * eps, gpu_device, slabs)
    assert torch.equal(beta[1], full[1])                         # dL/dv has no alpha part
    diff = [_np(full[k]) - _np(alpha[k]) for k in range(3)]
    _check64(f"f64 n={n} slabs={slabs} full - alpha against beta only", [torch.tensor(d) for d in diff],
             [_np(t) for t in beta], sums, n)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_deterministic_with_any_workspace(gpu_device, dtype):
    """Two calls whose workspaces hold different things give the same bits."""
    x, v, m, ca, cj, g, eps = _case(1000, EPS, dtype == F32)[:7]
    run = _vjp32 if dtype == F32 else _vjp64
    a = run(x, v, m, ca, cj, g, eps * eps, gpu_device, fill=float("nan"))
    b = run(x, v, m, ca, cj, g, eps * eps, gpu_device, fill=-3.25e7)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_entry_is_capturable(gpu_device, dtype):
    """Both cotangents (the alpha entry, the walk and the finish: five launches) captured once into a graph and replayed
    into outputs that were overwritten in between: the eager bits."""
    from nbd import direct
    n = 300
    x, v, m, ca, cj, g, eps = _case("direct_plummer_n300_ragged_mass")[:7]
    rows = _pack(dtype, x, v, m, ca, cj, gpu_device)
    if dtype == F32:
        ws, call = direct.accel_jerk_vjp_workspace(n, gpu_device), direct.accel_jerk_vjp
        eps2, g = direct.f32(eps * eps), direct.f32(g)
    else:
        ws, call, eps2 = direct.accel_jerk_vjp_f64_workspace(n, gpu_device), direct.accel_jerk_vjp_f64, eps * eps
    outs = [torch.empty((n, 3), dtype=dtype, device=gpu_device), torch.empty((n, 3), dtype=dtype, device=gpu_device),
            torch.empty((n,), dtype=dtype, device=gpu_device)]
    eager = [t.clone() for t in call(*rows, n, eps2, g, *outs, workspace=ws)]
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        call(*rows, n, eps2, g, *outs, workspace=ws)
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(*rows, n, eps2, g, *outs, workspace=ws)
    for t in outs:
        t.fill_(float("nan"))
    ws.fill_(255)
    graph.replay()
    torch.cuda.synchronize(gpu_device)
    assert all(torch.equal(p, q) for p, q in zip(outs, eager))


def test_translation_and_boost_invariance(gpu_device):
    """sum_i dL/dx_i = 0 and sum_i dL/dv_i = 0: L depends on differences of positions and of velocities only. Each row is
    within bar(T n, its sum|terms|) of its exact value and the fp64 sum of the n rows adds at most n 2^-53 sum of all
    |terms|: T + 1 terms per source over the summed |terms|."""
    n = 1000
    x, v, m, ca, cj, g, eps, ref, sums = _case(n)
    got = _vjp64(x, v, m, ca, cj, g, eps * eps, gpu_device)
    for k in range(2):
        total = _np(got[k]).sum(0)
        b = fo.bar((TERMS[k] + 1) * n, sums[k].sum(0))
        print(f"sum of {NAMES[k]}: |sum| / bar = {(np.abs(total) / b).max():.3f}")
        assert np.all(np.abs(total) <= b)


# ---------------------------------------------------------------- the autograd surface
def _sim(dtype, x, v, m, **kw):
    from galaxify import simulation
    kw.setdefault("g_const", G); kw.setdefault("softening", EPS); kw.setdefault("calc_energy", False)
    return simulation.HermiteSimulator(positions=x, velocities=v, masses=m, device="cuda", dtype=dtype, **kw)


def _state(n, seed, dtype):
    return jo.case(n, seed=seed, fp32=dtype == F32)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_forward_is_the_simulators_force(gpu_device, dtype):
    from nbd import autograd
    x, v, m, _, _ = _state(300, 41, dtype)
    sim = _sim(dtype, x, v, m, g_const=1.5, softening=0.07)
    ra, rj = sim.compute_accelerations_and_jerks()
    assert ra.grad_fn is None and rj.grad_fn is None and not ra.requires_grad          # nothing requires grad: today's path
    a, j = autograd.direct_accel_jerk(sim.positions, sim.velocities, sim.masses, 1.5, 0.07)
    assert a.dtype == dtype and torch.equal(a, ra) and torch.equal(j, rj) and a.grad_fn is None and j.grad_fn is None
    for name in ("positions", "velocities", "masses"):
        t = getattr(sim, name)
        t.requires_grad_()
        b, k = sim.compute_accelerations_and_jerks()
        assert b.grad_fn is not None and k.grad_fn is not None and torch.equal(b, ra) and torch.equal(k, rj)
        with torch.no_grad():
            c, l = sim.compute_accelerations_and_jerks()
        assert c.grad_fn is None and l.grad_fn is None and torch.equal(c, ra) and torch.equal(l, rj)
        t.requires_grad_(False)
    assert sim.compute_accelerations_and_jerks()[0].grad_fn is None


def test_block_simulator_inherits(gpu_device):
    from galaxify import simulation
    from nbd import autograd
    x, v, m, _, _ = _state(130, 43, F64)
    sim = simulation.BlockHermiteSimulator(positions=x, velocities=v, masses=m, device="cuda", dtype=F64, g_const=G,
                                           softening=EPS, calc_energy=False)
    ra, rj = sim.compute_accelerations_and_jerks()
    sim.velocities.requires_grad_()
    a, j = sim.compute_accelerations_and_jerks()
    assert type(a.grad_fn).__name__ == autograd.DirectAccelJerkFn.__name__ + "Backward" and torch.equal(a, ra) and torch.equal(j, rj)


@pytest.mark.parametrize("n", [5, 67])
def test_gradcheck_float64(gpu_device, n):
    from nbd import autograd
    x, v, m, _, _ = jo.case(n, seed=50 + n)
    xt, vt, mt = (_dev(a, gpu_device).requires_grad_() for a in (x, v, m))
    assert torch.autograd.gradcheck(lambda p, q, r: autograd.direct_accel_jerk(p, q, r, 1.3, 0.2), (xt, vt, mt))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_backward_once_and_only_what_is_asked(gpu_device, dtype):
    from nbd import autograd
    n = 130
    x, v, m, ca, cj = _state(n, 61, dtype)
    xt, vt, mt, at, jt = (_dev(a, gpu_device, dtype) for a in (x, v, m, ca, cj))
    xg, vg, mg = (t.clone().requires_grad_() for t in (xt, vt, mt))
    a, j = autograd.direct_accel_jerk(xg, vg, mg, G, EPS)
    torch.autograd.backward((a, j), (at, jt))
    with pytest.raises(RuntimeError):
        torch.autograd.backward((a, j), (at, jt))                                # once: the packed copy is released
    # against the kernels driven directly, bit for bit
    run = _vjp32 if dtype == F32 else _vjp64
    gp, gv, gm = run(x, v, m, ca, cj, G, EPS * EPS, gpu_device)
    assert torch.equal(xg.grad, gp) and torch.equal(vg.grad, gv) and torch.equal(mg.grad, gm)
    # one input at a time: the others have no edge and get no gradient
    for k, ref in enumerate((gp, gv, gm)):
        ins = [xt, vt, mt]
        ins[k] = ins[k].clone().requires_grad_()
        a, j = autograd.direct_accel_jerk(*ins, G, EPS)
        edges = a.grad_fn.next_functions
        assert all((edges[q][0] is not None) == (q == k) for q in range(3))
        torch.autograd.backward((a, j), (at, jt))
        assert torch.equal(ins[k].grad, ref)
        assert all(t.grad is None for q, t in enumerate(ins) if q != k)
    # non-contiguous cotangents
    xs = xt.clone().requires_grad_()
    wide = torch.zeros((2, n, 6), dtype=dtype, device=gpu_device)
    wide[0, :, ::2], wide[1, :, ::2] = at, jt
    assert not wide[0, :, ::2].is_contiguous()
    a, j = autograd.direct_accel_jerk(xs, vt, mt, G, EPS)
    torch.autograd.backward((a, j), (wide[0, :, ::2], wide[1, :, ::2]))
    assert torch.equal(xs.grad, gp)
    # an output that is not used: the bits of a zero cotangent
    zero = torch.zeros_like(at)
    for use, cots in ((0, (at, zero)), (1, (zero, jt))):
        ins = [t.clone().requires_grad_() for t in (xt, vt, mt)]
        autograd.direct_accel_jerk(*ins, G, EPS)[use].backward(cots[use])
        refs = [t.clone().requires_grad_() for t in (xt, vt, mt)]
        torch.autograd.backward(autograd.direct_accel_jerk(*refs, G, EPS), cots)
        assert all(torch.equal(p.grad, q.grad) for p, q in zip(ins, refs))
    # n = 0
    e3, e1 = torch.zeros((0, 3), dtype=dtype, device=gpu_device), torch.zeros((0,), dtype=dtype, device=gpu_device)
    e3.requires_grad_()
    a, j = autograd.direct_accel_jerk(e3, e3.detach(), e1, G, EPS)
    assert a.shape == (0, 3) and j.shape == (0, 3)
    (a.sum() + j.sum()).backward()
    assert e3.grad.shape == (0, 3)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_state_is_snapshotted_at_the_forward(gpu_device, dtype):
    """step() writes positions and velocities through raw pointers, which torch's version counters do not see: the node
    must have packed its own copy."""
    from nbd import autograd
    x, v, m, ca, cj = _state(200, 71, dtype)
    sim = _sim(dtype, x, v, m, dt=0.05)
    at, jt = _dev(ca, gpu_device, dtype), _dev(cj, gpu_device, dtype)
    for t in (sim.positions, sim.velocities, sim.masses):
        t.requires_grad_()
    saved = [t.detach().clone() for t in (sim.positions, sim.velocities, sim.masses)]
    a, j = sim.compute_accelerations_and_jerks()
    sim.step()
    sim.step()
    assert not torch.equal(sim.positions.detach(), saved[0]) and not torch.equal(sim.velocities.detach(), saved[1])
    torch.autograd.backward((a, j), (at, jt))
    fresh = [t.clone().requires_grad_() for t in saved]
    torch.autograd.backward(autograd.direct_accel_jerk(*fresh, G, EPS), (at, jt))
    for t, f in zip((sim.positions, sim.velocities, sim.masses), fresh):
        assert torch.equal(t.grad, f.grad)


def test_three_hermite_steps_compose(gpu_device):
    """Three predict-evaluate-correct steps in torch ops around direct_accel_jerk, float64, n = 33:
    d sum(x_final^2) / d (x0, v0, m) against CPU fp64 autograd of the dense statement, to 1e-10 global_rel (the leapfrog
    composition test's bound; the measured figure is in NOTES.md)."""
    from nbd import autograd
    n, dt, g, eps = 33, 0.02, 1.0, 0.05
    x, v, m, _, _ = _state(n, 81, F64)

    def rollout(force, x0, v0, mm):
        xx, vv = x0, v0
        a0, j0 = force(xx, vv, mm)
        for _ in range(3):
            xp = xx + vv * dt + a0 * (dt * dt / 2) + j0 * (dt ** 3 / 6)
            vp = vv + a0 * dt + j0 * (dt * dt / 2)
            a1, j1 = force(xp, vp, mm)
            v1 = vv + (a0 + a1) * (dt / 2) + (j0 - j1) * (dt * dt / 12)
            xx = xx + (vv + v1) * (dt / 2) + (a0 - a1) * (dt * dt / 12)
            vv, a0, j0 = v1, a1, j1
        return (xx * xx).sum()

    grads = []
    for device, force in ((gpu_device, lambda p, q, r: autograd.direct_accel_jerk(p, q, r, g, eps)),
                          ("cpu", lambda p, q, r: jo.dense_accel_jerk(p, q, r, g, eps))):
        ins = [torch.tensor(a, dtype=F64, device=device, requires_grad=True) for a in (x, v, m)]
        rollout(force, *ins).backward()
        grads.append([_np(t.grad) for t in ins])
    errs = [global_rel(p, q) for p, q in zip(*grads)]
    print(f"three Hermite steps: d/dx0 {errs[0]:.2e}, d/dv0 {errs[1]:.2e}, d/dm {errs[2]:.2e}")
    assert max(errs) <= 1e-10


def test_sharded_simulator_refuses(gpu_device, tmp_path, monkeypatch):
    import torch.distributed as dist
    x, v, m, _, _ = _state(300, 91, F32)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        monkeypatch.setenv("NBD_FORCE_SHARDED", "1")
        sim = _sim(F32, x, v, m, process_group=dist.group.WORLD)
        monkeypatch.delenv("NBD_FORCE_SHARDED")
        assert sim._sharded
        assert sim.compute_accelerations_and_jerks()[0].grad_fn is None
        sim.velocities.requires_grad_()
        with pytest.raises(ValueError, match="process_group is not supported"):
            sim.compute_accelerations_and_jerks()
        with torch.no_grad():
            assert sim.compute_accelerations_and_jerks()[1].grad_fn is None
    finally:
        dist.destroy_process_group()
