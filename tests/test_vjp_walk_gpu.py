"""The two fp32 force backward kernels (nbd_accel_vjp_f32 of csrc/direct_grad.hip, nbd_accel_jerk_vjp_f32 of
csrc/direct_hermite_grad.hip: accel_jerk_body of csrc/hermite_kernels.h with another pair policy, the second with three
streamed rows and the vmcnt(3) wait) on the MI355X at every edge of the chunk walk and where a wave walks three chunks and
more -- buffer 0 of the two-buffer LDS-DMA ring refilled behind the counted vmcnt -- against the fp64 rows of
tests/vjp_rows_oracle.py, through nbd.direct.hermite_pack, accel_vjp and accel_jerk_vjp; plus the units pinned to these
kernels bit for bit, at a long walk. What each size stands for: WALKS of test_hermite_walk_host.py; the entries have no
slab argument, so the default plan's n = 5633 is the smallest three-chunk walk.

The bars, on the checked rows (all rows up to n = 1100, else vjp_rows_oracle.sample_rows), each output on its own:
  F       <= 4 F_yardstick            F = max |got - ref| / (2^-24 sum|terms|); dL/dx, dL/dv and dL/dm
  row_rel <= max(1e-4, 4 row_rel_yardstick)                                     dL/dx and dL/dv
The yardstick is the plain float32 evaluation in the kernel's summation order (vjp_rows_oracle.yardstick_*), on the same
rows; 4 is the project's margin for v_rsq_f32 (test_hermite_walk_gpu.py), 1e-4 the row bar of the existing backward tests.
Both sides round the same fp32 terms in the same order, so the ratio sits near 1; a dropped chunk moves a row by about
64 / n of sum|terms| (test_vjp_walk_host.py shows the miss on the CPU). Where the yardstick's F is 0 the kernel matches
exactly.
Long sizes, all rows, against the project's fp64 backward (whose sampled rows are first held to the fp64 bar of
hermite_f64_oracle, T n terms): row_rel of dL/dx and dL/dv, global_rel of dL/dm, inside vjp_rows_oracle.NET_* -- a net
for gross errors in the groups the sample does not visit, not an accuracy claim (how it was set: NOTES.md, "T-VJPWALK").
Every workspace and output is filled with NaN bytes before each call. Every figure is printed before it is asserted.
Measured on the MI355X: NOTES.md, "T-VJPWALK"."""
import functools

import numpy as np
import pytest
import torch

import accel_jerk_vjp_oracle as jo
import hermite_f64_oracle as fo
import hermite_rows_oracle as hr
import vjp_rows_oracle as vr
from conftest import global_rel, row_rel

pytestmark = pytest.mark.gpu

G, EPS = 1.0, 0.05
F32, F64 = torch.float32, torch.float64
LONG = [(n, eps) for n in hr.LONG_SIZES for eps in ((EPS, 0.0) if n in hr.LONG_EPS0 else (EPS,))]
ACCEL_NAMES, JERK_NAMES = ("dL/dx", "dL/dm"), ("dL/dx", "dL/dv", "dL/dm")
ACCEL_TERMS, JERK_TERMS = (8, 3), (jo.T_POS, jo.T_VEL, jo.T_MASS)          # terms per source of the fp64 bar
COTS = {"both": (True, True), "alpha": (True, False), "beta": (False, True)}


def _np(t):
    return t.detach().cpu().numpy()


def _eps2(eps):
    return float(np.float32(eps * eps))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _nan_bytes(*tensors):
    for t in tensors:
        t.view(torch.uint8).fill_(255)
    return tensors


@functools.lru_cache(maxsize=None)
def _case(n):
    case = _frozen(*vr.case(n))
    for a in case:
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)      # fp32-representable, every value
    return case


@functools.lru_cache(maxsize=None)
def _plan(n):
    from nbd import direct
    return hr.chunk_plan(n, direct.accel_plan(n, n))


@functools.lru_cache(maxsize=None)
def _reference(op, n, eps, cots="both"):
    """(rows, the fp64 values of those rows, their sum|terms|, the yardstick's (row_rel, F) of every output), computed
    once and never written to. op "accel": (dL/dx, dL/dm); "jerk": (dL/dx, dL/dv, dL/dm) with the cotangents `cots`."""
    x, v, m, ca, cj = _case(n)
    rows = vr.sample_rows(n)
    if op == "accel":
        ref = vr.accel_vjp_rows(x, m, ca, G, _eps2(eps), rows)
        yard = vr.yardstick_accel_vjp_rows(x, m, ca, G, _eps2(eps), rows, _plan(n))
    else:
        ca, cj = (c if use else None for c, use in zip((ca, cj), COTS[cots]))
        ref = vr.accel_jerk_vjp_rows(x, v, m, ca, cj, G, _eps2(eps), rows)
        yard = vr.yardstick_accel_jerk_vjp_rows(x, v, m, ca, cj, G, _eps2(eps), rows, _plan(n))
    k = len(yard)
    assert all(y.dtype == np.float32 and np.isfinite(y).all() for y in yard)
    return (_frozen(rows)[0], _frozen(*ref[:k]), _frozen(*ref[k:]),
            tuple(vr.figures(y, r, s) for y, r, s in zip(yard, ref[:k], ref[k:])))


def _packed32(n, device):
    """(posm, velp, cota rows, cotj rows) through hermite_pack, a cotangent packed as the velocities; every buffer starts
    as NaN bytes."""
    from nbd import direct
    x, v, m, ca, cj = (torch.tensor(t, dtype=F32, device=device) for t in _case(n))
    posm, velp, arow, jrow, spare = _nan_bytes(*(direct.alloc_posm(n, device) for _ in range(5)))
    direct.hermite_pack(x, v, m, posm, velp)
    direct.hermite_pack(x, ca, m, spare, arow)
    direct.hermite_pack(x, cj, m, spare, jrow)
    return posm, velp, arow, jrow


def _accel32(n, eps, device, packed):
    """(dL/dx, dL/dm) as float32 tensors from accel_vjp; workspace and outputs start as NaN bytes."""
    from nbd import direct
    ws, gp, gm = _nan_bytes(direct.accel_vjp_workspace(n, device), torch.empty((n, 3), dtype=F32, device=device),
                            torch.empty((n,), dtype=F32, device=device))
    return direct.accel_vjp(packed[0], packed[2], n, _eps2(eps), G, gp, gm, workspace=ws)


def _jerk32(n, eps, device, packed, cots="both"):
    """(dL/dx, dL/dv, dL/dm) as float32 tensors from accel_jerk_vjp, all three asked for; workspace and outputs start as
    NaN bytes."""
    from nbd import direct
    ws, gp, gv, gm = _nan_bytes(direct.accel_jerk_vjp_workspace(n, device), torch.empty((n, 3), dtype=F32, device=device),
                                torch.empty((n, 3), dtype=F32, device=device), torch.empty((n,), dtype=F32, device=device))
    ca, cj = (c if use else None for c, use in zip(packed[2:], COTS[cots]))
    return direct.accel_jerk_vjp(packed[0], packed[1], ca, cj, n, _eps2(eps), G, gp, gv, gm, workspace=ws)


def _backward64(op, n, eps, device):
    """The project's fp64 backward of all rows on the same inputs, as numpy arrays; the workspace starts as NaN bytes."""
    from nbd import direct
    x, v, m, ca, cj = (torch.tensor(t, dtype=F64, device=device) for t in _case(n))
    posd, veld, arow, jrow, spare = (direct.alloc_rows_f64(n, device) for _ in range(5))
    direct.hermite_f64_pack(x, v, m, posd, veld)
    direct.hermite_f64_pack(x, ca, m, spare, arow)
    if op == "accel":
        ws = _nan_bytes(direct.accel_vjp_f64_workspace(n, device))[0]
        return [_np(t) for t in direct.accel_vjp_f64(posd, arow, n, _eps2(eps), G, workspace=ws)]
    direct.hermite_f64_pack(x, cj, m, spare, jrow)
    ws = _nan_bytes(direct.accel_jerk_vjp_f64_workspace(n, device))[0]
    return [_np(t) for t in direct.accel_jerk_vjp_f64(posd, veld, arow, jrow, n, _eps2(eps), G, workspace=ws)]


def _check_rows(tag, names, got, ref, sums, yard):
    """The sampled-row bars: got, ref and sums hold the checked rows of every output; yard its yardstick (row_rel, F)."""
    figs = []
    for name, g, r, s, (yr, yf) in zip(names, got, ref, sums, yard):
        assert g.shape == r.shape, (tag, name)
        rr, f = vr.figures(g, r, s)
        print(f"{tag}: {name}: F {f:.2f} (yardstick {yf:.2f}, ratio {f / yf if yf else float(f != 0):.2f}), "
              f"row_rel {rr:.2e} (yardstick {yr:.2e}, ratio {rr / yr if yr else float(rr != 0):.2f})")
        figs.append((name, rr, f, yr, yf))
    assert all(np.isfinite(g).all() for g in got), tag
    for name, rr, f, yr, yf in figs:
        assert f <= vr.MARGIN * yf, (tag, name, "F", f, yf)
        if name != "dL/dm":
            assert rr <= max(vr.ROW_BAR, vr.MARGIN * yr), (tag, name, "row_rel", rr, yr)


def _check_net(tag, names, terms, got, got64, n, rows, ref, sums, net):
    """The fp64 kernel's sampled rows at the fp64 bar, then every row of the fp32 result against it."""
    fig = [fo.within(g[rows], r, t * n, s) for g, r, t, s in zip(got64, ref, terms, sums)]
    print(f"{tag}: the fp64 kernel, |got - ref| / bar: " + ", ".join(f"{nm} {f:.3f}" for nm, (_, f) in zip(names, fig)))
    assert all(ok for ok, _ in fig), (tag, fig)
    nets = [(global_rel if nm == "dL/dm" else row_rel)(g, g64) for nm, g, g64 in zip(names, got, got64)]
    print(f"{tag}: all rows against the fp64 kernel: " + ", ".join(
        f"{nm} {'global_rel' if nm == 'dL/dm' else 'row_rel'} {e:.2e} (bar {b:.0e})" for nm, e, b in zip(names, nets, net)))
    for nm, e, b in zip(names, nets, net):
        assert e <= b, (tag, nm, e, b)


# ---------------------------------------------------------------- the kernels against the fp64 rows
@pytest.mark.parametrize("n", hr.EDGE_SIZES)
def test_accel_backward_edge_sizes_all_rows(gpu_device, n):
    """eps = 0.05 (the un-masked block loop, the group's two own chunks masked) and eps = 0 (the index-masked instance)."""
    packed = _packed32(n, gpu_device)
    for eps in (EPS, 0.0):
        rows, ref, sums, yard = _reference("accel", n, eps)
        assert rows.size == n
        got = [_np(t) for t in _accel32(n, eps, gpu_device, packed)]
        _check_rows(f"accel backward n={n} eps={eps}", ACCEL_NAMES, got, ref, sums, yard)
        if n == 1:
            assert not any(g.any() for g in got)                         # no partner: exact zeros


@pytest.mark.parametrize("n", hr.EDGE_SIZES)
def test_jerk_backward_edge_sizes_all_rows(gpu_device, n):
    """Both cotangents (the alpha part through the workspace, behind the beta block), both softenings."""
    packed = _packed32(n, gpu_device)
    for eps in (EPS, 0.0):
        rows, ref, sums, yard = _reference("jerk", n, eps)
        assert rows.size == n
        got = [_np(t) for t in _jerk32(n, eps, gpu_device, packed)]
        _check_rows(f"jerk backward n={n} eps={eps}", JERK_NAMES, got, ref, sums, yard)
        if n == 1:
            assert not any(g.any() for g in got)


@pytest.mark.parametrize("n,eps", LONG)
def test_accel_backward_long_walks(gpu_device, n, eps):
    """Two chunks per wave and more (5633: the first refill of buffer 0; 32193: 21 chunks per wave): the sampled rows at
    the bars, and all rows inside the net around the fp64 kernel."""
    rows, ref, sums, yard = _reference("accel", n, eps)
    assert rows.size < n
    tag = f"accel backward n={n} eps={eps}"
    got = [_np(t) for t in _accel32(n, eps, gpu_device, _packed32(n, gpu_device))]
    _check_rows(tag, ACCEL_NAMES, [g[rows] for g in got], ref, sums, yard)
    _check_net(tag, ACCEL_NAMES, ACCEL_TERMS, got, _backward64("accel", n, eps, gpu_device), n, rows, ref, sums,
               vr.NET_ACCEL)


@pytest.mark.parametrize("n,eps", LONG)
def test_jerk_backward_long_walks(gpu_device, n, eps):
    """The three-row form (six staging quads per buffer, vmcnt(3)) at the same walks, both cotangents."""
    rows, ref, sums, yard = _reference("jerk", n, eps)
    assert rows.size < n
    tag = f"jerk backward n={n} eps={eps}"
    got = [_np(t) for t in _jerk32(n, eps, gpu_device, _packed32(n, gpu_device))]
    _check_rows(tag, JERK_NAMES, [g[rows] for g in got], ref, sums, yard)
    _check_net(tag, JERK_NAMES, JERK_TERMS, got, _backward64("jerk", n, eps, gpu_device), n, rows, ref, sums, vr.NET_JERK)


@pytest.mark.parametrize("cots", ["beta", "alpha"])
def test_jerk_backward_one_cotangent_at_a_long_walk(gpu_device, cots):
    """n = 5633, all three outputs asked for. beta only: the walk's sums are the result. alpha only: the acceleration
    backward writes the outputs in place from its workspace behind the (multi-slab) beta block, and dL/dv is zeros."""
    n = 5633
    rows, ref, sums, yard = _reference("jerk", n, EPS, cots)
    got = [_np(t) for t in _jerk32(n, EPS, gpu_device, _packed32(n, gpu_device), cots)]
    _check_rows(f"jerk backward n={n} {cots} only", JERK_NAMES, [g[rows] for g in got], ref, sums, yard)
    if cots == "alpha":
        assert not got[1].any()


# ---------------------------------------------------------------- the units pinned to these kernels, at a long walk
PINNED_N = 5633


def _tensors(n, device):
    return tuple(torch.tensor(t, dtype=F32, device=device) for t in _case(n))


def test_direct_accel_backward_is_accel_vjps_bits(gpu_device):
    from nbd import autograd
    n = PINNED_N
    x, _, m, ca, _ = _tensors(n, gpu_device)
    xg, mg = x.clone().requires_grad_(), m.clone().requires_grad_()
    autograd.direct_accel(xg, mg, G, EPS).backward(ca)
    gp, gm = _accel32(n, EPS, gpu_device, _packed32(n, gpu_device))
    assert torch.isfinite(gp).all() and torch.isfinite(gm).all()
    assert torch.equal(xg.grad, gp) and torch.equal(mg.grad, gm)


def test_direct_accel_jerk_backward_is_accel_jerk_vjps_bits(gpu_device):
    from nbd import autograd
    n = PINNED_N
    x, v, m, ca, cj = _tensors(n, gpu_device)
    ins = [t.clone().requires_grad_() for t in (x, v, m)]
    torch.autograd.backward(autograd.direct_accel_jerk(*ins, G, EPS), (ca, cj))
    want = _jerk32(n, EPS, gpu_device, _packed32(n, gpu_device))
    for t, w in zip(ins, want):
        assert torch.isfinite(w).all()
        assert torch.equal(t.grad, w)


def test_hermite_simulator_under_autograd_gives_the_same_bits(gpu_device):
    from galaxify import simulation
    n = PINNED_N
    x, v, m, ca, cj = _tensors(n, gpu_device)
    sim = simulation.HermiteSimulator(positions=_case(n)[0].astype(np.float32), velocities=_case(n)[1].astype(np.float32),
                                      masses=_case(n)[2].astype(np.float32), g_const=G, softening=EPS,
                                      calc_energy=False, device="cuda")
    state = (sim.positions, sim.velocities, sim.masses)
    assert all(torch.equal(s, t) for s, t in zip(state, (x, v, m)))
    for t in state:
        t.requires_grad_()
    torch.autograd.backward(sim.compute_accelerations_and_jerks(), (ca, cj))
    want = _jerk32(n, EPS, gpu_device, _packed32(n, gpu_device))
    for t, w in zip(state, want):
        assert torch.equal(t.grad, w)


def test_without_the_jerk_cotangent_the_bits_are_accel_vjp_at_a_long_walk(gpu_device):
    n = PINNED_N
    packed = _packed32(n, gpu_device)
    gp, gv, gm = _jerk32(n, EPS, gpu_device, packed, "alpha")
    rp, rm = _accel32(n, EPS, gpu_device, packed)
    assert torch.isfinite(rp).all() and torch.isfinite(rm).all()
    assert torch.equal(gp, rp) and torch.equal(gm, rm) and not _np(gv).any()
