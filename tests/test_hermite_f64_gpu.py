"""HermiteSimulator(dtype=torch.float64) on the GPU (csrc/direct_hermite_f64.hip) against the fp64 oracles at the
accuracy bar of tests/hermite_f64_oracle.py: |got - ref| <= (T + 32) 2^-53 sum|terms| for a sum of T terms. No input is
fp32-representable, and every workspace is NaN-filled before a call.

Measured on the MI355X (largest |got - ref| / bar per test, and the step distances) are in NOTES.md, "K-H64"."""
import functools

import numpy as np
import pytest
import torch

import hermite_f64_oracle as fo
import hermite_oracle as ho
from conftest import load_golden

pytestmark = pytest.mark.gpu

G, EPS = 1.0, 0.05
SIZES = [1, 2, 3, 63, 64, 65, 130, 448, 449, 1000, 5000]      # 448 / 449: one slab -> two (nbd_hermite_f64_plan)


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, device):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, device=device)


def _nan_bytes(nbytes, device):
    return torch.full((nbytes // 8 + 2,), float("nan"), dtype=torch.float64, device=device).view(torch.uint8)


def _sim(x, v, m, device, **kw):
    from galaxify import simulation
    kw.setdefault("g_const", G); kw.setdefault("softening", EPS); kw.setdefault("calc_energy", False)
    sim = simulation.HermiteSimulator(positions=x, velocities=v, masses=m, device="cuda", dtype=torch.float64, **kw)
    sim._hws.view(torch.float64).fill_(float("nan"))
    return sim


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, v, m, g, eps, a, j, sum|a terms|, sum|j terms|), computed once and never written to."""
    if isinstance(name, int):
        x, v, m = fo.plummer_case(name, seed=100 + name)
        g, eps = G, EPS
    else:
        gd = load_golden(name)
        x, v, m = fo.perturbed(gd["pos"], gd["vel"], gd["mass"], 5)
        g, eps = float(gd["g_const"]), float(gd["softening"])
    a, j = fo.accel_jerk(x, v, m, g, eps * eps)
    sa, sj = fo.accel_jerk_abs(x, v, m, g, eps * eps)
    for arr in (x, v, m, a, j, sa, sj):
        arr.setflags(write=False)
    return x, v, m, g, eps, a, j, sa, sj


def _force(x, v, m, g, eps2, device, slabs=0):
    from nbd import direct
    n = x.shape[0]
    posd, veld = direct.alloc_rows_f64(n, device), direct.alloc_rows_f64(n, device)
    direct.hermite_f64_pack(_dev(x, device), _dev(v, device), _dev(m, device), posd, veld)
    ws = _nan_bytes(direct.hermite_f64_workspace(n, device, slabs).numel(), device)
    a, j = direct.accel_jerk_f64(posd, veld, n, eps2, g, workspace=ws, slabs=slabs)
    return _np(a), _np(j)


def _check_force(tag, got_a, got_j, a, j, sa, sj):
    n = a.shape[0]
    ok_a, fa = fo.within(got_a, a, n, sa)
    ok_j, fj = fo.within(got_j, j, 4 * n, sj)
    print(f"{tag}: |a - ref| / bar = {fa:.3f}, |j - ref| / bar = {fj:.3f}")
    assert ok_a and ok_j, (tag, fa, fj)


@pytest.mark.parametrize("name", SIZES + ["direct_plummer_n64_eps0", "direct_plummer_n300_ragged_mass"])
def test_force_and_jerk_at_the_bar(gpu_device, name):
    """Through the simulator (the plan's split) for every size; the goldens add the index-masked path (softening 0) and a
    massless body."""
    x, v, m, g, eps, a, j, sa, sj = _case(name)
    if not isinstance(name, int):
        assert (eps == 0.0) == name.endswith("eps0") and ((m == 0).any() == ("ragged_mass" in name))
    sim = _sim(x, v, m, gpu_device, g_const=g, softening=eps)
    assert all(t.dtype == torch.float64 and t.is_cuda for t in
               (sim.positions, sim.velocities, sim.masses, sim.accelerations, sim.jerks))
    assert np.array_equal(_np(sim.positions), x) and np.array_equal(_np(sim.masses), m)      # not through fp32
    _check_force(f"n={name}", _np(sim.accelerations), _np(sim.jerks), a, j, sa, sj)
    a2, j2 = sim.compute_accelerations_and_jerks()
    assert torch.equal(a2, sim.accelerations) and torch.equal(j2, sim.jerks)                 # NaN workspace, same bits
    assert torch.equal(sim.compute_accelerations(), sim.accelerations)


@pytest.mark.parametrize("n,slabs", [(130, 1), (1000, 1), (1000, 3), (5000, 1), (5000, 64)])
def test_force_with_an_explicit_split(gpu_device, n, slabs):
    """Several chunks per wave (both LDS buffers reused: 1000 / 1 -> 4 chunks, 5000 / 1 -> 19 or 20), waves without a
    chunk (130 / 1: three chunks on four waves; 5000 / 64: 79 chunks on 256 waves), an uneven split (1000 / 3)."""
    x, v, m, g, eps, a, j, sa, sj = _case(n)
    got_a, got_j = _force(x, v, m, g, eps * eps, gpu_device, slabs)
    _check_force(f"n={n} slabs={slabs}", got_a, got_j, a, j, sa, sj)


def test_cancellation_case(gpu_device):
    """Two bodies 2e-9 apart at x = 1 with eps = 1e-10 and a third far away: an fp32 difference, or a reciprocal square
    root left at its hardware estimate, misses the bar by many orders of magnitude."""
    rng = np.random.default_rng(3)
    x = np.array([[1.0 - 1e-9, 0.0, 0.0], [1.0 + 1e-9, 0.0, 0.0], [-50.0, 3.0, 2.0]])
    v = rng.uniform(-1, 1, (3, 3))
    m = np.array([0.3, 0.5, 0.2]) + rng.uniform(-1, 1, 3) * 1e-9
    eps = 1e-10
    a, j = fo.accel_jerk(x, v, m, G, eps * eps)
    sa, sj = fo.accel_jerk_abs(x, v, m, G, eps * eps)
    assert np.abs(a[:2]).max() > 1e16                     # the close pair dominates: s^3 ~ 1e26
    sim = _sim(x, v, m, gpu_device, softening=eps)
    _check_force("cancellation", _np(sim.accelerations), _np(sim.jerks), a, j, sa, sj)


@pytest.mark.parametrize("n", [2, 65, 1000])
def test_potential_invariants_and_energies_at_the_bar(gpu_device, n):
    x, v, m, g, eps, *_ = _case(n)
    sim = _sim(x, v, m, gpu_device)
    phi_gpu = sim.compute_potentials()
    assert phi_gpu.dtype == torch.float64 and phi_gpu.shape == (n,)
    phi, sp = fo.potentials(x, m, g, eps * eps)
    ok, f_phi = fo.within(_np(phi_gpu), phi, n, sp)
    assert ok, f_phi
    # the row: its 12 sums against the oracle's from the GPU's own phi (phi itself is checked above), each at the bar
    sim._hws.view(torch.float64).fill_(float("nan"))
    inv = sim.compute_invariants()
    row = np.array(inv.row())
    s, s_abs = fo.sums(x, v, m, _np(phi_gpu))
    b = fo.bar(n, s_abs)
    M, K, U = s[0], s[10], 0.5 * s[11]
    assert abs(row[0] - M) <= b[0]
    assert np.all(np.abs(row[1:4] * row[0] - s[1:4]) <= b[1:4] + np.abs(row[1:4]) * b[0] + 4 * fo.U53 * np.abs(s[1:4]))
    assert np.all(np.abs(row[4:10] - s[4:10]) <= b[4:10])
    assert abs(row[10] - K) <= b[10] and abs(row[11] - U) <= 0.5 * b[11]
    assert row[12] == row[10] + row[11] and row[13] == -2.0 * row[10] / row[11] and row[14] == row[15] == 0.0
    f_row = max(abs(row[0] - M) / b[0], abs(row[10] - K) / b[10], abs(row[11] - U) / (0.5 * b[11]))
    # (U, K) of compute_energies(): the reference's convention, T = the number of pair terms
    sim._hws.view(torch.float64).fill_(float("nan"))
    u_gpu, k_gpu = sim.compute_energies()
    u, k, ua, ka = fo.reference_energies(x, v, m, g, eps)
    ok_u, f_u = fo.within(u_gpu, u, n * (n - 1) // 2, ua)
    ok_k, f_k = fo.within(k_gpu, k, n, ka)
    print(f"n={n}: / bar: phi {f_phi:.3f}, row {f_row:.3f}, U {f_u:.4f}, K {f_k:.3f}")
    assert ok_u and ok_k, (f_u, f_k)
    assert u_gpu != inv.u_energy                          # two conventions, as in fp32


def test_steps_against_the_oracle(gpu_device):
    """n = 1000, dt = 0.01, after 1 and 10 steps: within 8 s_k + 8 * 2^-53 max|value| of hermite_run, s_k = the largest
    difference between that run and the same run with the bodies permuted (measured here, on the CPU): the factor 8 is
    for a different reciprocal square root and a different summation order."""
    n, dt = 1000, 0.01
    x, v, m, g, eps, *_ = _case(n)
    perm = np.random.default_rng(11).permutation(n)
    back = np.empty_like(perm)
    back[perm] = np.arange(n)
    sim = _sim(x, v, m, gpu_device, dt=dt)
    done = 0
    for k in (1, 10):
        ref = ho.hermite_run(x, v, m, dt, g, eps * eps, k)
        prm = [q[back] for q in ho.hermite_run(x[perm], v[perm], m[perm], dt, g, eps * eps, k)]
        while done < k:
            sim.step()
            done += 1
        got = [_np(t) for t in (sim.positions, sim.velocities, sim.accelerations, sim.jerks)]
        for name, r, p, q in zip(("pos", "vel", "acc", "jerk"), ref, prm, got):
            s_k = np.abs(r - p).max()
            dist = np.abs(q - r).max()
            tol = 8 * s_k + 8 * fo.U53 * np.abs(r).max()
            print(f"steps={k} {name}: s_k = {s_k:.3e}, |gpu - oracle| = {dist:.3e}, tolerance {tol:.3e}")
            assert dist <= tol, (k, name, dist, tol)


@pytest.mark.parametrize("steps", [256, 512, 1024, 2048])
def test_two_body_orbit(gpu_device, steps):
    """e = 0.5, eps = 0.1, one period in `steps` steps: the final positions within 1e-10 of hermite_run with the same
    steps, and the relative energy error of compute_invariants() equal to the oracle's own to 1 % or 1e-13. (That the
    oracle is in its convergent regime at these step counts is test_hermite_f64_host's; repeated here for the runs used.)"""
    x, v, m, period = ho.two_body(0.5)
    x, v, m = fo.perturbed(x, v, m, 9)                   # (the orbit's zeros too: no input is fp32-representable)
    eps, dt = 0.1, period / steps
    ref = ho.hermite_run(x, v, m, dt, 1.0, eps * eps, steps)
    half = ho.hermite_run(x, v, m, dt / 2, 1.0, eps * eps, 2 * steps)
    quarter = ho.hermite_run(x, v, m, dt / 4, 1.0, eps * eps, 4 * steps)
    ratio = np.abs(ref[0] - half[0]).max() / np.abs(half[0] - quarter[0]).max()
    assert 12.0 < ratio < 20.0, ratio
    sim = _sim(x, v, m, gpu_device, softening=eps, dt=dt)
    e0_gpu = sim.compute_invariants().energy
    for _ in range(steps):
        sim.step()
    dist = ho.orbit_error(_np(sim.positions), ref[0])
    e0 = fo.energy(x, v, m, 1.0, eps * eps)
    err_ref = abs(fo.energy(ref[0], ref[1], m, 1.0, eps * eps) - e0) / abs(e0)
    err_gpu = abs(sim.compute_invariants().energy - e0_gpu) / abs(e0_gpu)
    print(f"S={steps}: |x_gpu - x_oracle| = {dist:.3e}, energy error gpu {err_gpu:.6e} oracle {err_ref:.6e}, "
          f"oracle position-error ratio {ratio:.2f}")
    assert dist <= 1e-10, dist
    assert abs(err_gpu - err_ref) <= max(0.01 * err_ref, 1e-13), (err_gpu, err_ref)


def test_run_is_eager_float64_and_bit_identical_to_steps(gpu_device):
    n, steps = 130, 12
    x, v, m, *_ = _case(n)
    kw = dict(dt=0.01, calc_energy=True, calc_invariants=True)
    ran, twin, again = (_sim(x, v, m, gpu_device, **kw) for _ in range(3))
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
    assert torch.equal(ran.positions, twin.positions) and torch.equal(ran.jerks, twin.jerks)
    for s, t in zip(states, again.run(steps)):
        assert torch.equal(s.positions, t.positions) and torch.equal(s.velocities, t.velocities)
        assert torch.equal(s.accelerations, t.accelerations)
        assert (s.u_energy, s.k_energy, s.invariants) == (t.u_energy, t.k_energy, t.invariants)


def test_default_dtype_is_untouched(gpu_device):
    """A default-dtype simulator built beside a float64 one keeps float32 tensors, and its first step is
    nbd_hermite_step_f32 driven directly, bit for bit."""
    from galaxify import simulation
    from nbd import direct
    g = load_golden("direct_plummer_n300_ragged_mass")
    dt, gc, soft = float(g["dt"]), float(g["g_const"]), float(g["softening"])
    kw = dict(positions=g["pos"], velocities=g["vel"], masses=g["mass"], g_const=gc, softening=soft, dt=dt,
              calc_energy=False, device="cuda")
    wide = simulation.HermiteSimulator(dtype=torch.float64, **kw)
    plain = simulation.HermiteSimulator(**kw)
    named = simulation.HermiteSimulator(dtype=torch.float32, **kw)
    assert wide.positions.dtype == torch.float64 and not plain._f64
    for sim in (plain, named):
        assert all(t.dtype == torch.float32 for t in
                   (sim.positions, sim.velocities, sim.masses, sim.accelerations, sim.jerks))
    n = plain.n
    f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=gpu_device)      # noqa: E731
    pos, vel, mass = f32(g["pos"]), f32(g["vel"]), f32(g["mass"])
    eps2, gcf = direct.f32(soft ** 2), direct.f32(gc)
    posm, velp = direct.alloc_posm(n, gpu_device), direct.alloc_posm(n, gpu_device)
    hws = direct.hermite_workspace(n, gpu_device)
    direct.hermite_pack(pos, vel, mass, posm, velp)
    acc, jerk = direct.accel_jerk(posm, velp, n, eps2, gcf, workspace=hws)
    assert torch.equal(acc, plain.accelerations) and torch.equal(jerk, plain.jerks)
    wide.step(); plain.step(); named.step()
    direct.hermite_step(pos, vel, acc, jerk, acc, jerk, mass, dt, eps2, gcf, posm, hws)
    for sim in (plain, named):
        for got, want in ((sim.positions, pos), (sim.velocities, vel), (sim.accelerations, acc), (sim.jerks, jerk)):
            assert got.dtype == torch.float32 and torch.equal(got, want)
    assert plain._graph_run_ok(64) and not wide._graph_run_ok(64)
