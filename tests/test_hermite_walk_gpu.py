"""The fp32 Hermite force (accel_jerk_body of csrc/hermite_kernels.h, through nbd.direct.hermite_pack / accel_jerk, both
variants) on the MI355X at every edge of its chunk walk and where a wave walks three chunks and more -- buffer 0 of the
two-buffer LDS-DMA ring refilled behind the counted vmcnt -- against the fp64 rows of tests/hermite_rows_oracle.py, plus
one step at a long walk and the units that are pinned to this kernel bit for bit (a scene of a batch, block level 0, the
active-subset force) at a long walk. What each size stands for: WALKS of test_hermite_walk_host.py, which holds the
launch plan to it.

The bars, on the checked rows (all rows up to n = 1100, else hermite_rows_oracle.sample_rows), acceleration and jerk each:
  F       <= 4 F_yardstick,                F = max |got - ref| / (2^-24 sum|terms|), sum|terms| as hermite_f64_oracle has it
  row_rel <= max(1e-5, 4 row_rel_yardstick)
The yardstick is the plain float32 evaluation in the kernel's summation order of hermite_rows_oracle.yardstick_rows, on
the same rows in the same call; the factor 4 is the margin test_accel_jerk_vjp_gpu.py gives a kernel over its fp32
yardstick (v_rsq_f32 is good to 1 ulp, not correctly rounded, and enters cubed and to the fifth power). Both sides form
the same fp32 differences of the same fp32 inputs, so the ratio sits near 1; a dropped or stale source moves a
component by about 1 / n of sum|terms|, hundreds of times the bar at every size here. The jerk is not held to the flat
1e-5 of the golden states: its terms cancel 10-20 times and plain fp32 reaches 3e-5 over all rows of these inputs
(NOTES.md, "T-WALK").
Long sizes, all rows, against the project's own fp64 kernel (whose sampled rows are first held to the fp64 bar of
hermite_f64_oracle): acceleration row_rel <= 1e-5, jerk row_rel <= 3e-4 -- a net for gross errors in the groups the
sample does not visit (a dropped chunk costs about 64 / n of sum|terms|, 2e-3 or more), not an accuracy claim.
Every workspace and output is filled with NaN bytes before each call. Every figure is printed before it is asserted.
Measured on the MI355X: NOTES.md, "T-WALK"."""
import functools

import numpy as np
import pytest
import torch

import hermite_f64_oracle as fo
import hermite_rows_oracle as hr
from conftest import row_rel

pytestmark = pytest.mark.gpu

G, EPS, DT = 1.0, 0.05, 1.0 / 64
TOL = 1e-5                              # the project's bar (TOL of test_hermite_gpu.py)
NET_ACC, NET_JERK = 1e-5, 3e-4          # all rows of a long size against the fp64 kernel
F32, F64 = torch.float32, torch.float64


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
    return _frozen(*hr.case(n))


@functools.lru_cache(maxsize=None)
def _plan(n):
    from nbd import direct
    return hr.chunk_plan(n, direct.accel_plan(n, n))


@functools.lru_cache(maxsize=None)
def _reference(n, eps):
    """(rows, (a, j, sum|a terms|, sum|j terms|) of those rows in fp64, the yardstick's (row_rel, F) of a and of j),
    computed once and never written to."""
    x, v, m = _case(n)
    rows = hr.sample_rows(n)
    ref = hr.accel_jerk_rows(x, v, m, G, _eps2(eps), rows)
    ya, yj = hr.yardstick_rows(x, v, m, G, _eps2(eps), rows, _plan(n))
    assert np.isfinite(ya).all() and np.isfinite(yj).all()
    return _frozen(rows)[0], _frozen(*ref), (hr.figures(ya, ref[0], ref[2]), hr.figures(yj, ref[1], ref[3]))


def _state32(n, device):
    x, v, m = _case(n)
    return tuple(torch.tensor(t, dtype=F32, device=device) for t in (x, v, m))


def _packed32(n, device):
    from nbd import direct
    pos, vel, mass = _state32(n, device)
    posm, velp = _nan_bytes(direct.alloc_posm(n, device), direct.alloc_posm(n, device))
    direct.hermite_pack(pos, vel, mass, posm, velp)
    return posm, velp


def _force32(n, eps, variant, device, packed=None):
    """(acc, jerk) as numpy float32 through hermite_pack and accel_jerk; workspace and outputs start as NaN bytes."""
    from nbd import direct
    posm, velp = packed if packed is not None else _packed32(n, device)
    ws, acc, jerk = _nan_bytes(direct.hermite_workspace(n, device), torch.empty((n, 3), dtype=F32, device=device),
                               torch.empty((n, 3), dtype=F32, device=device))
    direct.accel_jerk(posm, velp, n, _eps2(eps), G, acc, jerk, workspace=ws, variant=variant)
    return _np(acc), _np(jerk)


def _force64(x, v, m, eps, device):
    """(acc, jerk) of all rows as float64 tensors from the project's fp64 kernel."""
    from nbd import direct
    n = x.shape[0]
    xt, vt, mt = (torch.tensor(np.asarray(t), dtype=F64, device=device) for t in (x, v, m))
    posd, veld = direct.alloc_rows_f64(n, device), direct.alloc_rows_f64(n, device)
    direct.hermite_f64_pack(xt, vt, mt, posd, veld)
    ws = direct.hermite_f64_workspace(n, device)
    _nan_bytes(ws)
    return direct.accel_jerk_f64(posd, veld, n, _eps2(eps), G, workspace=ws)


def _check_rows(tag, acc, jerk, ref, yard):
    """The sampled-row bars: acc, jerk are the checked rows (k, 3); ref = (a, j, sum|a terms|, sum|j terms|) of them;
    yard = the yardstick's ((row_rel, F) of a, (row_rel, F) of j)."""
    assert acc.shape == ref[0].shape and jerk.shape == ref[1].shape
    figs = []
    for name, got, want, terms, (yr, yf) in (("acc", acc, ref[0], ref[2], yard[0]), ("jerk", jerk, ref[1], ref[3], yard[1])):
        rr, f = hr.figures(got, want, terms)
        print(f"{tag}: {name}: F {f:.2f} (yardstick {yf:.2f}, ratio {f / yf if yf else float(f != 0):.2f}), "
              f"row_rel {rr:.2e} (yardstick {yr:.2e}, ratio {rr / yr if yr else float(rr != 0):.2f})")
        figs.append((name, rr, f, yr, yf))
    assert np.isfinite(acc).all() and np.isfinite(jerk).all(), tag
    for name, rr, f, yr, yf in figs:
        assert f <= 4 * yf, (tag, name, "F", f, yf)
        assert rr <= max(TOL, 4 * yr), (tag, name, "row_rel", rr, yr)


def _eps_of(n):
    return (EPS, 0.0) if n <= 1100 or n in hr.LONG_EPS0 else (EPS,)


# ---------------------------------------------------------------- the force against the fp64 rows
@pytest.mark.parametrize("n", hr.EDGE_SIZES)
def test_edge_sizes_all_rows(gpu_device, n):
    """eps = 0.05 (the un-masked block loop) and eps = 0 (the index-masked loop), variants 0 and 1."""
    packed = _packed32(n, gpu_device)
    for eps in _eps_of(n):
        rows, ref, yard = _reference(n, eps)
        assert rows.size == n
        for variant in (0, 1):
            acc, jerk = _force32(n, eps, variant, gpu_device, packed)
            _check_rows(f"n={n} eps={eps} variant={variant}", acc, jerk, ref, yard)
            if n == 1:
                assert not acc.any() and not jerk.any()                  # no partner: exact zeros


@pytest.mark.parametrize("n", hr.LONG_SIZES)
def test_long_walks(gpu_device, n):
    """Two chunks per wave and more (5633: the first refill of buffer 0; 32193: 21 chunks per wave): the sampled rows at
    the bars, and all rows inside the net around the fp64 kernel."""
    x, v, m = _case(n)
    packed = _packed32(n, gpu_device)
    for eps in _eps_of(n):
        rows, ref, yard = _reference(n, eps)
        assert rows.size < n
        a64, j64 = (_np(t) for t in _force64(x, v, m, eps, gpu_device))
        ok_a, fa = fo.within(a64[rows], ref[0], n, ref[2])
        ok_j, fj = fo.within(j64[rows], ref[1], 4 * n, ref[3])
        print(f"n={n} eps={eps}: the fp64 kernel, |got - ref| / bar: acc {fa:.3f}, jerk {fj:.3f}")
        assert ok_a and ok_j, (n, eps, fa, fj)
        for variant in (0, 1):
            tag = f"n={n} eps={eps} variant={variant}"
            acc, jerk = _force32(n, eps, variant, gpu_device, packed)
            _check_rows(tag, acc[rows], jerk[rows], ref, yard)
            net_a, net_j = row_rel(acc, a64), row_rel(jerk, j64)
            print(f"{tag}: all rows against the fp64 kernel: acc row_rel {net_a:.2e}, jerk row_rel {net_j:.2e}")
            assert np.isfinite(acc).all() and np.isfinite(jerk).all(), tag
            assert net_a <= NET_ACC, (tag, net_a)
            assert net_j <= NET_JERK, (tag, net_j)


@pytest.mark.parametrize("n", hr.STEP_SIZES)
def test_one_step_at_a_long_walk(gpu_device, n):
    """nbd_hermite_step_f32 from (x, v, a0, j0), dt = 1/64, with a0, j0 the fp64 kernel's force rounded to fp32. Sampled
    rows: x1, v1 against the fp64 corrector fed by the fp64 rows at the fp64 predicted state, row_rel < 1e-5; acc_out and
    jerk_out against those rows at the sampled-row bars, the yardstick evaluated where the kernel evaluates -- at the
    fp32 predicted state (hermite_rows_oracle.predict32, the bits hermite_pack gives) -- so that both carry the rounding
    of the predicted state."""
    from nbd import direct
    x, v, m = _case(n)
    eps2 = _eps2(EPS)
    rows = hr.sample_rows(n)
    a0t, j0t = (t.to(F32) for t in _force64(x, v, m, EPS, gpu_device))
    a0, j0 = _np(a0t).astype(np.float64), _np(j0t).astype(np.float64)
    # the reference
    xp = x + v * DT + a0 * (DT * DT / 2) + j0 * (DT ** 3 / 6)
    vp = v + a0 * DT + j0 * (DT * DT / 2)
    ref = hr.accel_jerk_rows(xp, vp, m, G, eps2, rows)
    v1 = v[rows] + (a0[rows] + ref[0]) * (DT / 2) + (j0[rows] - ref[1]) * (DT * DT / 12)
    x1 = x[rows] + (v[rows] + v1) * (DT / 2) + (a0[rows] - ref[0]) * (DT * DT / 12)
    # the yardstick
    xp32, vp32 = hr.predict32(x, v, a0, j0, DT)
    ya, yj = hr.yardstick_rows(xp32, vp32, m, G, eps2, rows, _plan(n))
    yard = (hr.figures(ya, ref[0], ref[2]), hr.figures(yj, ref[1], ref[3]))
    # the predicted rows the kernel works from are the yardstick's
    pos, vel, mass = _state32(n, gpu_device)
    posm, velp = _nan_bytes(direct.alloc_posm(n, gpu_device), direct.alloc_posm(n, gpu_device))
    direct.hermite_pack(pos, vel, mass, posm, velp, a0t, j0t, DT)
    assert np.array_equal(_np(posm)[:n, :3], xp32) and np.array_equal(_np(velp)[:n, :3], vp32)
    # the step
    ws, acc1, jerk1, posm = _nan_bytes(direct.hermite_workspace(n, gpu_device), torch.empty_like(a0t),
                                       torch.empty_like(j0t), posm)
    direct.hermite_step(pos, vel, a0t, j0t, acc1, jerk1, mass, DT, eps2, G, posm, ws)
    got = [_np(t) for t in (pos, vel, acc1, jerk1)]
    assert all(np.isfinite(t).all() for t in got)
    ex, ev = row_rel(got[0][rows], x1), row_rel(got[1][rows], v1)
    print(f"step n={n}: x1 row_rel {ex:.2e}, v1 row_rel {ev:.2e}")
    _check_rows(f"step n={n}", got[2][rows], got[3][rows], ref, yard)
    assert ex < TOL and ev < TOL, (n, ex, ev)
    assert np.array_equal(_np(posm)[:n, :3], got[0])                     # posm = {x1, m}


# ---------------------------------------------------------------- the units pinned to this kernel, at a long walk
def _sim(cls, n, **kw):
    from galaxify import simulation
    x, v, m = _case(n)
    return getattr(simulation, cls)(positions=x.astype(np.float32), velocities=v.astype(np.float32),
                                    masses=m.astype(np.float32), g_const=G, softening=EPS, dt=DT, calc_energy=False,
                                    device="cuda", **kw)


def _state(sim):
    return (sim.positions, sim.velocities, sim.accelerations, sim.jerks)


def test_scenes_of_a_batch_are_the_lone_simulators_bits(gpu_device):
    from galaxify import simulation
    sizes = hr.PINNED_SCENES
    cases = [tuple(t.astype(np.float32) for t in _case(n)) for n in sizes]
    batch = simulation.BatchedSimulator(systems=cases, integrator="hermite", g_const=G, softening=EPS, dt=DT,
                                        calc_energy=False, device="cuda")
    lones = [_sim("HermiteSimulator", n) for n in sizes]

    def compare(what, names):
        for i, lone in enumerate(lones):
            lo, hi = int(batch.offsets[i]), int(batch.offsets[i + 1])
            assert hi - lo == sizes[i]
            for nm in names:
                p, q = getattr(batch, nm)[lo:hi], getattr(lone, nm)
                assert torch.isfinite(q).all(), (what, sizes[i], nm)
                assert torch.equal(p, q), (what, sizes[i], nm, float((p - q).abs().max()))
    compare("construction", ("accelerations", "jerks"))
    for _ in range(2):
        batch.step()
        for lone in lones:
            lone.step()
    compare("2 steps", ("positions", "velocities", "accelerations", "jerks"))


def test_block_level_zero_is_the_shared_step_bit_for_bit(gpu_device):
    n = hr.ACTIVE_N
    shared, block = _sim("HermiteSimulator", n), _sim("BlockHermiteSimulator", n, max_level=0)
    for _ in range(2):
        shared.step()
        block.step()
    for nm, p, q in zip(("pos", "vel", "acc", "jerk"), _state(shared), _state(block)):
        assert torch.isfinite(p).all(), nm
        assert torch.equal(p, q), (nm, float((p - q).abs().max()))
    assert block.block_steps == 2


def test_active_list_of_all_bodies_shuffled_gives_accel_jerks_bits(gpu_device):
    from nbd import direct
    n = hr.ACTIVE_N
    posm, velp = _packed32(n, gpu_device)
    order = np.random.default_rng(n).permutation(n)
    act = torch.tensor(order, dtype=torch.int32, device=gpu_device)
    for eps in (EPS, 0.0):
        ws = _nan_bytes(direct.hblock_workspace(n, gpu_device))[0]
        acc, jerk = direct.accel_jerk_active(posm, velp, n, act, _eps2(eps), G, workspace=ws)
        full_a, full_j = direct.accel_jerk(posm, velp, n, _eps2(eps), G)
        back_a, back_j = torch.empty_like(full_a), torch.empty_like(full_j)
        back_a[act.long()], back_j[act.long()] = acc, jerk
        assert torch.isfinite(full_a).all() and torch.isfinite(full_j).all()
        assert torch.equal(back_a, full_a) and torch.equal(back_j, full_j), eps


def test_active_list_of_130_under_the_raised_slab_plan(gpu_device):
    """130 random targets under 5633 sources: plan_active raises the slab count, another split of the same chunks. The
    workspace is exactly what the entry checks; the yardstick takes the split of plan_active."""
    from nbd import direct
    n, k = hr.ACTIVE_N, hr.ACTIVE_LIST
    x, v, m = _case(n)
    rows = np.random.default_rng(k).choice(n, k, replace=False)
    plan = hr.active_plan(n, k, direct.accel_plan(n, k))
    assert plan["slabs"] > _plan(n)["slabs"]
    posm, velp = _packed32(n, gpu_device)
    act = torch.tensor(rows, dtype=torch.int32, device=gpu_device)
    need = -(-n // 4) * 16 + plan["slabs"] * 6 * k * 4
    for eps in (EPS, 0.0):
        ref = hr.accel_jerk_rows(x, v, m, G, _eps2(eps), rows)
        ya, yj = hr.yardstick_rows(x, v, m, G, _eps2(eps), rows, plan)
        yard = (hr.figures(ya, ref[0], ref[2]), hr.figures(yj, ref[1], ref[3]))
        ws = _nan_bytes(torch.empty(need, dtype=torch.uint8, device=gpu_device))[0]
        acc, jerk = direct.accel_jerk_active(posm, velp, n, act, _eps2(eps), G, workspace=ws)
        _check_rows(f"active {k} of {n} eps={eps}", _np(acc), _np(jerk), ref, yard)
