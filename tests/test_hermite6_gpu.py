"""Hermite6Simulator on the GPU (csrc/direct_hermite_f64.hip) against the fp64 oracle of tests/hermite6_oracle.py.

The acceleration and the jerk of the three-array evaluation are held to the BITS of direct.accel_jerk_f64 on the same
packed rows at the same slab count (that entry has its own accuracy tests); the snap to the accuracy bar of
tests/hermite_f64_oracle.py, |got - ref| <= (T + 32) 2^-53 sum|terms| with T = 19 n, against the oracle evaluated on the
inputs the kernel was given. No input is fp32-representable, and every workspace is NaN-filled before a call."""
import functools

import numpy as np
import pytest
import torch

import hermite6_oracle as h6
import hermite_f64_oracle as fo
import hermite_oracle as ho
from conftest import load_golden

pytestmark = pytest.mark.gpu

G, EPS = 1.0, 0.05


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, device):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, device=device)


def _nan_bytes(nbytes, device):
    return torch.full((nbytes // 8 + 2,), float("nan"), dtype=torch.float64, device=device).view(torch.uint8)


def _sim(x, v, m, **kw):
    from galaxify import simulation
    kw.setdefault("g_const", G); kw.setdefault("softening", EPS); kw.setdefault("calc_energy", False)
    sim = simulation.Hermite6Simulator(positions=x, velocities=v, masses=m, device="cuda", **kw)
    sim._hws.view(torch.float64).fill_(float("nan"))
    return sim


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, v, m, g, eps, a of the oracle), computed once and never written to."""
    if isinstance(name, int):
        x, v, m = fo.plummer_case(name, seed=600 + name)
        g, eps = G, EPS
    else:
        gd = load_golden(name)
        x, v, m = fo.perturbed(gd["pos"], gd["vel"], gd["mass"], 5)
        g, eps = float(gd["g_const"]), float(gd["softening"])
    a = ho.accel_jerk(x, v, m, g, eps * eps)[0]
    for arr in (x, v, m, a):
        arr.setflags(write=False)
    return x, v, m, g, eps, a


@functools.lru_cache(maxsize=None)
def _snap_of_case(n):
    """(the oracle's snap, its sum|terms|) of _case(n) on the oracle's acceleration rows: once for every split of n."""
    x, v, m, g, eps, a = _case(n)
    ref, s_abs = h6.snap_and_abs(x, v, a, m, g, eps * eps)
    ref.setflags(write=False); s_abs.setflags(write=False)
    return ref, s_abs


def _check_snap(tag, got, x, v, a_rows, m, g, eps2, ref=None):
    """The snap at the bar, against the oracle on the rows the kernel was given."""
    n = x.shape[0]
    ref, s_abs = ref if ref is not None else h6.snap_and_abs(x, v, a_rows, m, g, eps2)
    ok, frac = fo.within(got, ref, 19 * n, s_abs)
    print(f"{tag}: |s - ref| / bar = {frac:.4f}")
    assert ok, (tag, frac)


def _force(x, v, a, m, g, eps2, device, slabs=0):
    """(a, j, s) of direct.accel_jerk_snap_f64 and (a, j) of direct.accel_jerk_f64 on the same packed rows, at `slabs`,
    NaN-filled workspaces."""
    from nbd import direct
    n = x.shape[0]
    posd, veld, accd = (direct.alloc_rows_f64(n, device) for _ in range(3))
    direct.hermite6_pack(_dev(x, device), _dev(v, device), _dev(m, device), posd, veld, accd, acc=_dev(a, device))
    assert np.array_equal(_np(accd[:n, :3]), a) and not _np(accd[n:]).any() and not _np(accd[:, 3]).any()
    ws = _nan_bytes(direct.hermite6_workspace(n, device, slabs).numel(), device)
    got = direct.accel_jerk_snap_f64(posd, veld, accd, n, eps2, g, workspace=ws, slabs=slabs)
    ws4 = _nan_bytes(direct.hermite_f64_workspace(n, device, slabs).numel(), device)
    ref = direct.accel_jerk_f64(posd, veld, n, eps2, g, workspace=ws4, slabs=slabs)
    ws.view(torch.float64).fill_(float("nan"))
    again = direct.accel_jerk_snap_f64(posd, veld, accd, n, eps2, g, workspace=ws, slabs=slabs)
    assert all(torch.equal(p, q) for p, q in zip(got, again))
    return got, ref


@pytest.mark.parametrize("name", [3, 64, 65, 130, 1000, "direct_plummer_n64_eps0", "direct_plummer_n300_ragged_mass"])
def test_force_at_the_bar(gpu_device, name):
    """Through the simulator's construction (the plan's split): two passes, the acceleration first. The goldens add the
    index-masked path (softening 0) and a massless body."""
    from nbd import direct
    x, v, m, g, eps, _ = _case(name)
    if not isinstance(name, int):
        assert (eps == 0.0) == name.endswith("eps0") and ((m == 0).any() == ("ragged_mass" in name))
    sim = _sim(x, v, m, g_const=g, softening=eps)
    n = sim.n
    state = (sim.positions, sim.velocities, sim.masses, sim.accelerations, sim.jerks, sim.snaps, sim.crackles)
    assert all(t.dtype == torch.float64 and t.is_cuda for t in state)
    assert all(t.shape == (n, 3) for t in state[3:]) and not sim.crackles.any()
    assert np.array_equal(_np(sim.positions), x) and np.array_equal(_np(sim.masses), m)      # not through fp32
    assert np.array_equal(_np(sim._posd[:n, :3]), x) and np.array_equal(_np(sim._veld[:n, :3]), v)
    a4, j4 = direct.accel_jerk_f64(sim._posd, sim._veld, n, eps * eps, g,
                                   workspace=_nan_bytes(direct.hermite_f64_workspace(n, gpu_device).numel(), gpu_device))
    assert torch.equal(sim.accelerations, a4) and torch.equal(sim.jerks, j4)
    assert torch.equal(sim._accd[:n, :3], a4)                    # the second pass ran on the first pass's acceleration
    _check_snap(f"n={name}", _np(sim.snaps), x, v, _np(a4), m, g, eps * eps)
    sim._hws.view(torch.float64).fill_(float("nan"))
    a2, j2, s2 = sim.compute_accelerations_jerks_and_snaps()     # NaN workspace, same bits, new tensors
    assert torch.equal(a2, sim.accelerations) and torch.equal(j2, sim.jerks) and torch.equal(s2, sim.snaps)
    assert a2.data_ptr() != sim.accelerations.data_ptr() and s2.data_ptr() != sim.snaps.data_ptr()
    a3, j3 = sim.compute_accelerations_and_jerks()               # the inherited two
    assert torch.equal(a3, a4) and torch.equal(j3, j4) and torch.equal(sim.compute_accelerations(), a4)


@pytest.mark.parametrize("n,slabs", [(130, 1), (1000, 1), (1000, 3), (5000, 1), (5000, 64)])
def test_force_with_an_explicit_split(gpu_device, n, slabs):
    """Several chunks per wave (both LDS buffers reused: 1000 / 1 -> 4 chunks, 5000 / 1 -> 19 or 20), waves without a
    chunk (130 / 1: three chunks on four waves; 5000 / 64: 79 chunks on 256 waves), an uneven split (1000 / 3)."""
    x, v, m, g, eps, a = _case(n)
    (a6, j6, s6), (a4, j4) = _force(x, v, a, m, g, eps * eps, gpu_device, slabs)
    assert torch.equal(a6, a4) and torch.equal(j6, j4)
    _check_snap(f"n={n} slabs={slabs}", _np(s6), x, v, a, m, g, eps * eps, ref=_snap_of_case(n))


def test_cancellation_case(gpu_device):
    """Two bodies 2e-9 apart at x = 1 with eps = 1e-10 and a third far away, the acceleration rows from the oracle: an
    fp32 difference, or a reciprocal square root left at its hardware estimate, misses the bar by many orders."""
    rng = np.random.default_rng(3)
    x = np.array([[1.0 - 1e-9, 0.0, 0.0], [1.0 + 1e-9, 0.0, 0.0], [-50.0, 3.0, 2.0]])
    v = rng.uniform(-1, 1, (3, 3))
    m = np.array([0.3, 0.5, 0.2]) + rng.uniform(-1, 1, 3) * 1e-9
    eps = 1e-10
    a = ho.accel_jerk(x, v, m, G, eps * eps)[0]
    assert np.abs(a[:2]).max() > 1e16                     # the close pair dominates: s^3 ~ 1e26
    (a6, j6, s6), (a4, j4) = _force(x, v, a, m, G, eps * eps, gpu_device)
    assert torch.equal(a6, a4) and torch.equal(j6, j4)
    _check_snap("cancellation", _np(s6), x, v, a, m, G, eps * eps)


def _oracle_states(x, v, m, dt, g, eps2, marks):
    """The oracle's (x, v, a, j, s, c) after each step count of `marks`, from one run."""
    state = (np.array(x), np.array(v)) + h6.start(x, v, m, g, eps2)
    out = {}
    for k in range(1, max(marks) + 1):
        state = h6.hermite6_step(*state, m, dt, g, eps2)
        if k in marks:
            out[k] = state
    return out


def test_steps_against_the_oracle(gpu_device):
    """n = 1000, dt = 0.01, after 1 and 10 steps: within 8 s_k + 8 * 2^-53 max|value| of hermite6_run, s_k = the largest
    difference between that run and the same run with the bodies permuted (measured here, on the CPU): the float64
    4th-order step test's rule and factor. The crackle of every step is the c1 formula on the simulator's own (a, j, s)
    before and after the step, componentwise within 16 * 2^-53 of the sum of its |terms|."""
    n, dt = 1000, 0.01
    x, v, m, g, eps, _ = _case(n)
    perm = np.random.default_rng(11).permutation(n)
    back = np.empty_like(perm)
    back[perm] = np.arange(n)
    ref = _oracle_states(x, v, m, dt, g, eps * eps, (1, 10))
    prm = _oracle_states(x[perm], v[perm], m[perm], dt, g, eps * eps, (1, 10))
    sim = _sim(x, v, m, dt=dt)
    done = 0
    for k in (1, 10):
        while done < k:
            before = [_np(t) for t in (sim.accelerations, sim.jerks, sim.snaps)]
            old = (sim.accelerations, sim.jerks, sim.snaps, sim.crackles)
            sim.step()
            done += 1
            assert all(new is not o for new, o in zip((sim.accelerations, sim.jerks, sim.snaps, sim.crackles), old))
            after = [_np(t) for t in (sim.accelerations, sim.jerks, sim.snaps)]
            c_err = np.abs(_np(sim.crackles) - h6.crackle(*before, *after, dt))
            c_tol = 16 * fo.U53 * h6.crackle_abs(*before, *after, dt)
            assert np.all(c_err <= c_tol), (done, float((c_err / c_tol).max()))
        got = [_np(t) for t in (sim.positions, sim.velocities, sim.accelerations, sim.jerks, sim.snaps)]
        for name, r, p, q in zip(("pos", "vel", "acc", "jerk", "snap"), ref[k], prm[k], got):
            s_k = np.abs(r - p[back]).max()
            dist = np.abs(q - r).max()
            tol = 8 * s_k + 8 * fo.U53 * np.abs(r).max()
            print(f"steps={k} {name}: s_k = {s_k:.3e}, |gpu - oracle| = {dist:.3e}, tolerance {tol:.3e}")
            assert dist <= tol, (k, name, dist, tol)


@functools.lru_cache(maxsize=None)
def _orbit():
    x, v, m, period = ho.two_body(0.5)
    x, v, m = fo.perturbed(x, v, m, 9)                   # (the orbit's zeros too: no input is fp32-representable)
    return x, v, m, period


@pytest.mark.parametrize("steps", [64, 128, 256, 512])
def test_two_body_orbit(gpu_device, steps):
    """e = 0.5, eps = 0.1, one period in `steps` steps: the final positions within 1e-10 of hermite6_run with the same
    steps, and the relative energy error of compute_invariants() equal to the oracle's own to 1 % or 1e-13. At 256 steps
    the error is at least 100 times below HermiteSimulator(dtype=torch.float64)'s on the same device (the oracles: 546)."""
    from galaxify import simulation
    x, v, m, period = _orbit()
    eps, dt = 0.1, period / steps
    ref = h6.hermite6_run(x, v, m, dt, 1.0, eps * eps, steps)
    sim = _sim(x, v, m, softening=eps, dt=dt)
    e0_gpu = sim.compute_invariants().energy
    for _ in range(steps):
        sim.step()
    dist = ho.orbit_error(_np(sim.positions), ref[0])
    e0 = fo.energy(x, v, m, 1.0, eps * eps)
    err_ref = abs(fo.energy(ref[0], ref[1], m, 1.0, eps * eps) - e0) / abs(e0)
    err_gpu = abs(sim.compute_invariants().energy - e0_gpu) / abs(e0_gpu)
    print(f"S={steps}: |x_gpu - x_oracle| = {dist:.3e}, energy error gpu {err_gpu:.6e} oracle {err_ref:.6e}")
    assert dist <= 1e-10, dist
    assert abs(err_gpu - err_ref) <= max(0.01 * err_ref, 1e-13), (err_gpu, err_ref)
    if steps == 256:
        four = simulation.HermiteSimulator(positions=x, velocities=v, masses=m, g_const=1.0, softening=eps, dt=dt,
                                           calc_energy=False, device="cuda", dtype=torch.float64)
        e0_four = four.compute_invariants().energy
        for _ in range(steps):
            four.step()
        err_four = abs(four.compute_invariants().energy - e0_four) / abs(e0_four)
        print(f"S={steps}: 4th-order energy error {err_four:.6e}, ratio {err_four / err_gpu:.1f}")
        assert err_four >= 100.0 * err_gpu, (err_four, err_gpu)


def test_run_is_eager_float64_and_bit_identical_to_steps(gpu_device):
    n, steps = 130, 12
    x, v, m, *_ = _case(n)
    kw = dict(dt=0.01, calc_energy=True, calc_invariants=True)
    ran, twin, again = (_sim(x, v, m, **kw) for _ in range(3))
    assert not ran._graph_run_ok(steps) and not ran._graph_run_ok(64)
    states = ran.run(steps)
    assert len(states) == steps and [s.step for s in states] == list(range(steps))
    for s in states:
        twin.step()
        for got, want in ((s.positions, twin.positions), (s.velocities, twin.velocities),
                          (s.accelerations, twin.accelerations)):
            assert got.dtype == torch.float64 and not got.is_cuda and torch.equal(got, want.cpu())
        assert (s.u_energy, s.k_energy) == twin.compute_energies()
        assert s.invariants == twin.compute_invariants()
    assert ran._run_stage[0].dtype == torch.float64 and ran._run_stage[0].is_pinned()
    for name in ("positions", "velocities", "accelerations", "jerks", "snaps", "crackles"):
        assert torch.equal(getattr(ran, name), getattr(twin, name)), name
    assert torch.equal(ran.gather("positions"), ran.positions)
    for s, t in zip(states, again.run(steps)):
        assert torch.equal(s.positions, t.positions) and torch.equal(s.velocities, t.velocities)
        assert torch.equal(s.accelerations, t.accelerations)
        assert (s.u_energy, s.k_energy, s.invariants) == (t.u_energy, t.k_energy, t.invariants)


def test_the_fourth_order_simulators_are_untouched(gpu_device):
    """A default HermiteSimulator and a HermiteSimulator(dtype=torch.float64) built beside a Hermite6Simulator: their
    first step is nbd_hermite_step_f32 resp. nbd_hermite_step_f64 driven directly, bit for bit."""
    from galaxify import simulation
    from nbd import direct
    g = load_golden("direct_plummer_n300_ragged_mass")
    dt, gc, soft = float(g["dt"]), float(g["g_const"]), float(g["softening"])
    kw = dict(positions=g["pos"], velocities=g["vel"], masses=g["mass"], g_const=gc, softening=soft, dt=dt,
              calc_energy=False, device="cuda")
    six = simulation.Hermite6Simulator(**kw)
    plain = simulation.HermiteSimulator(**kw)
    wide = simulation.HermiteSimulator(dtype=torch.float64, **kw)
    assert six.snaps.dtype == torch.float64 and not hasattr(plain, "snaps") and not hasattr(wide, "snaps")
    n = plain.n
    for sim, dtype in ((plain, torch.float32), (wide, torch.float64)):
        assert all(t.dtype == dtype for t in (sim.positions, sim.velocities, sim.masses, sim.accelerations, sim.jerks))
    six.step(); plain.step(); wide.step(); six.step()
    # fp32, as test_hermite_f64_gpu drives it
    pos, vel, mass = (torch.tensor(np.asarray(g[k]), dtype=torch.float32, device=gpu_device)
                      for k in ("pos", "vel", "mass"))
    eps2, gcf = direct.f32(soft ** 2), direct.f32(gc)
    posm, velp = direct.alloc_posm(n, gpu_device), direct.alloc_posm(n, gpu_device)
    hws = direct.hermite_workspace(n, gpu_device)
    direct.hermite_pack(pos, vel, mass, posm, velp)
    acc, jerk = direct.accel_jerk(posm, velp, n, eps2, gcf, workspace=hws)
    direct.hermite_step(pos, vel, acc, jerk, acc, jerk, mass, dt, eps2, gcf, posm, hws)
    for got, want in ((plain.positions, pos), (plain.velocities, vel), (plain.accelerations, acc), (plain.jerks, jerk)):
        assert got.dtype == torch.float32 and torch.equal(got, want)
    # float64
    pos, vel, mass = (_dev(g[k], gpu_device) for k in ("pos", "vel", "mass"))
    posd, veld = direct.alloc_rows_f64(n, gpu_device), direct.alloc_rows_f64(n, gpu_device)
    ws = direct.hermite_f64_workspace(n, gpu_device)
    direct.hermite_f64_pack(pos, vel, mass, posd, veld)
    acc, jerk = direct.accel_jerk_f64(posd, veld, n, soft ** 2, gc, workspace=ws)
    direct.hermite_step_f64(pos, vel, acc, jerk, acc, jerk, mass, dt, soft ** 2, gc, posd, veld, ws)
    for got, want in ((wide.positions, pos), (wide.velocities, vel), (wide.accelerations, acc), (wide.jerks, jerk)):
        assert got.dtype == torch.float64 and torch.equal(got, want)
