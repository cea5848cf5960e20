"""LeapFrogSimulator / EulerSimulator(dtype=torch.float64) and nbd_accel_f64 on the GPU (csrc/direct_leapfrog_f64.hip)
against the fp64 oracles at the accuracy bar of tests/hermite_f64_oracle.py, |got - ref| <= (T + 32) 2^-53 sum|terms|, and
bit for bit against nbd_accel_jerk_f64's acceleration and against numpy's float64 update formulas. No input is
fp32-representable, and every workspace is NaN-filled before a call."""
import functools

import numpy as np
import pytest
import torch

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


def _sim(x, v, m, device, cls="LeapFrogSimulator", **kw):
    from galaxify import simulation
    kw.setdefault("g_const", G); kw.setdefault("softening", EPS); kw.setdefault("calc_energy", False)
    sim = getattr(simulation, cls)(positions=x, velocities=v, masses=m, device="cuda", dtype=torch.float64, **kw)
    sim._hws.view(torch.float64).fill_(float("nan"))
    return sim


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, v, m, g, eps, a, sum|a terms|), computed once and never written to."""
    if isinstance(name, int):
        x, v, m = fo.plummer_case(name, seed=300 + name)
        g, eps = G, EPS
    else:
        gd = load_golden(name)
        x, v, m = fo.perturbed(gd["pos"], gd["vel"], gd["mass"], 5)
        g, eps = float(gd["g_const"]), float(gd["softening"])
    a, _ = fo.accel_jerk(x, v, m, g, eps * eps)
    sa, _ = fo.accel_jerk_abs(x, v, m, g, eps * eps)
    for arr in (x, v, m, a, sa):
        arr.setflags(write=False)
    return x, v, m, g, eps, a, sa


def _check_accel(tag, got, a, sa):
    ok, frac = fo.within(got, a, a.shape[0], sa)
    print(f"{tag}: |a - ref| / bar = {frac:.3f}")
    assert ok, (tag, frac)


@pytest.mark.parametrize("name", [1, 2, 63, 64, 65, 129, 448, 449, 1000, "direct_plummer_n64_eps0",
                                  "direct_plummer_n300_ragged_mass"])
def test_acceleration_at_the_bar(gpu_device, name):
    """Through the simulator (the plan's split); the goldens add the index-masked path (softening 0) and a massless body."""
    x, v, m, g, eps, a, sa = _case(name)
    if not isinstance(name, int):
        assert (eps == 0.0) == name.endswith("eps0") and ((m == 0).any() == ("ragged_mass" in name))
    sim = _sim(x, v, m, gpu_device, g_const=g, softening=eps)
    assert all(t.dtype == torch.float64 and t.is_cuda for t in
               (sim.positions, sim.velocities, sim.masses, sim.accelerations))
    assert np.array_equal(_np(sim.positions), x) and np.array_equal(_np(sim.masses), m)      # not through fp32
    _check_accel(f"n={name}", _np(sim.accelerations), a, sa)
    sim._hws.view(torch.float64).fill_(float("nan"))
    assert torch.equal(sim.compute_accelerations(), sim.accelerations)                       # NaN workspace, same bits


def test_cancellation_case(gpu_device):
    """Two bodies 2e-9 apart at x = 1 with eps = 1e-10 and a third far away: an fp32 difference, or a reciprocal square
    root left at its hardware estimate, misses the bar by many orders of magnitude."""
    rng = np.random.default_rng(3)
    x = np.array([[1.0 - 1e-9, 0.0, 0.0], [1.0 + 1e-9, 0.0, 0.0], [-50.0, 3.0, 2.0]])
    v = rng.uniform(-1, 1, (3, 3))
    m = np.array([0.3, 0.5, 0.2]) + rng.uniform(-1, 1, 3) * 1e-9
    eps = 1e-10
    a, _ = fo.accel_jerk(x, v, m, G, eps * eps)
    sa, _ = fo.accel_jerk_abs(x, v, m, G, eps * eps)
    assert np.abs(a[:2]).max() > 1e16                     # the close pair dominates: s^3 ~ 1e26
    sim = _sim(x, v, m, gpu_device, softening=eps)
    _check_accel("cancellation", _np(sim.accelerations), a, sa)


@pytest.mark.parametrize("n,slabs", [(n, s) for n in (65, 449, 1000) for s in (0, 1, 3)] + [(2100, 1), (65, 8)])
def test_acceleration_is_bit_identical_to_the_hermite_force(gpu_device, n, slabs):
    """nbd_accel_f64 against nbd_accel_jerk_f64's acc_out at the same slab count, each with a NaN-filled workspace, and
    run twice. 2100 / 1: 33 chunks over 4 waves, 9/8/8/8 -- a wave walks many chunks; 65 / 8: waves without a chunk."""
    from nbd import direct
    x, v, m = fo.plummer_case(n, seed=500 + n)
    posd, veld = direct.alloc_rows_f64(n, gpu_device), direct.alloc_rows_f64(n, gpu_device)
    direct.hermite_f64_pack(_dev(x, gpu_device), _dev(v, gpu_device), _dev(m, gpu_device), posd, veld)
    want = direct.accel_jerk_f64(posd, veld, n, EPS * EPS, G, slabs=slabs,
                                 workspace=_nan_bytes(direct.hermite_f64_workspace(n, gpu_device, slabs).numel(),
                                                      gpu_device))[0]
    need = direct.accel_f64_workspace(n, gpu_device, slabs).numel()
    first = direct.accel_f64(posd, n, EPS * EPS, G, workspace=_nan_bytes(need, gpu_device), slabs=slabs)
    again = direct.accel_f64(posd, n, EPS * EPS, G, workspace=_nan_bytes(need, gpu_device), slabs=slabs)
    assert not torch.isnan(first).any()
    assert torch.equal(first, want) and torch.equal(again, first)
    if slabs == 0:                                       # ... and a Hermite workspace serves the plan's split
        ws = _nan_bytes(direct.hermite_f64_workspace(n, gpu_device).numel(), gpu_device)
        assert torch.equal(direct.accel_f64(posd, n, EPS * EPS, G, workspace=ws), want)


@pytest.mark.parametrize("cls", ["LeapFrogSimulator", "EulerSimulator"])
def test_one_step_is_bit_equal_to_numpy_float64(gpu_device, cls):
    """n = 130: with the GPU's own a0 and a1, x1 and v1 are numpy float64's, every product and sum rounded on its own."""
    n, dt = 130, 0.01
    x, v, m = fo.plummer_case(n, seed=430)
    sim = _sim(x, v, m, gpu_device, cls=cls, dt=dt)
    a0 = _np(sim.accelerations)
    sim.step()
    a1 = _np(sim.accelerations)
    assert sim.accelerations.dtype == torch.float64
    if cls == "LeapFrogSimulator":
        vh = v + (0.5 * dt) * a0
        x1 = x + dt * vh
        v1 = vh + (0.5 * dt) * a1
        assert np.array_equal(_np(sim._posd)[:n, :3], x1) and np.array_equal(_np(sim._posd)[:n, 3], m)
    else:
        assert np.array_equal(a1, a0)                    # a(t) of the unchanged positions: the same bits
        v1 = v + dt * a1
        x1 = x + dt * v1
        assert np.array_equal(_np(sim._posd)[:n, :3], x)                         # the pre-drift positions
    assert np.all(_np(sim._posd)[n:] == 0.0)
    assert np.array_equal(_np(sim.positions), x1) and np.array_equal(_np(sim.velocities), v1)


def test_steps_against_the_oracle(gpu_device):
    """n = 1000, dt = 0.01, after 1 and 10 steps: within 8 s_k + 8 * 2^-53 max|value| of leapfrog_run, s_k = the largest
    difference between that run and the same run with the bodies permuted (the rule of test_hermite_f64_gpu.py)."""
    n, dt = 1000, 0.01
    x, v, m, g, eps, *_ = _case(n)
    perm = np.random.default_rng(11).permutation(n)
    back = np.empty_like(perm)
    back[perm] = np.arange(n)
    sim = _sim(x, v, m, gpu_device, dt=dt)
    done = 0
    for k in (1, 10):
        ref = ho.leapfrog_run(x, v, m, dt, g, eps * eps, k)
        prm = [q[back] for q in ho.leapfrog_run(x[perm], v[perm], m[perm], dt, g, eps * eps, k)]
        while done < k:
            sim.step()
            done += 1
        for name, r, p, q in zip(("pos", "vel"), ref, prm, (_np(sim.positions), _np(sim.velocities))):
            s_k = np.abs(r - p).max()
            dist = np.abs(q - r).max()
            tol = 8 * s_k + 8 * fo.U53 * np.abs(r).max()
            print(f"steps={k} {name}: s_k = {s_k:.3e}, |gpu - oracle| = {dist:.3e}, tolerance {tol:.3e}")
            assert dist <= tol, (k, name, dist, tol)


@pytest.mark.parametrize("steps", [256, 1024, 4096])
def test_two_body_orbit(gpu_device, steps):
    """e = 0.5, eps = 0.1, one period in `steps` steps: the final positions within 1e-10 of leapfrog_run with the same
    steps, and the relative energy error of compute_invariants() equal to the oracle's own to 1 % or 1e-13 (1.8e-9 at 256
    steps, 1.1e-10 at 1024, 7.1e-12 at 4096: second order, far below what an fp32 state can show)."""
    x, v, m, period = ho.two_body(0.5)
    x, v, m = fo.perturbed(x, v, m, 9)                   # (the orbit's zeros too: no input is fp32-representable)
    eps, dt = 0.1, period / steps
    ref = ho.leapfrog_run(x, v, m, dt, 1.0, eps * eps, steps)
    sim = _sim(x, v, m, gpu_device, softening=eps, dt=dt)
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


@pytest.mark.parametrize("cls", ["LeapFrogSimulator", "EulerSimulator"])
def test_run_is_eager_float64_and_bit_identical_to_steps(gpu_device, cls):
    n, steps = 130, 12
    x, v, m = fo.plummer_case(n, seed=430)
    kw = dict(cls=cls, dt=0.01, calc_energy=True, calc_invariants=True)
    ran, twin = (_sim(x, v, m, gpu_device, **kw) for _ in range(2))
    assert ran.n == n and not ran._graph_run_ok(steps) and not ran._graph_run_ok(64)
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
    assert torch.equal(ran.positions, twin.positions) and torch.equal(ran.accelerations, twin.accelerations)
    # the energies are those of the fp64 oracle on the final state
    xs, vs = _np(ran.positions), _np(ran.velocities)
    u, k, ua, ka = fo.reference_energies(xs, vs, m, G, EPS)
    assert fo.within(states[-1].u_energy, u, n * (n - 1) // 2, ua)[0] and fo.within(states[-1].k_energy, k, n, ka)[0]


def test_default_dtype_is_untouched(gpu_device):
    """A default-dtype LeapFrogSimulator built beside a float64 one keeps float32 tensors, and its first step is
    nbd_leapfrog_step_f32 driven directly, bit for bit."""
    from galaxify import simulation
    from nbd import direct
    g = load_golden("direct_plummer_n300_ragged_mass")
    dt, gc, soft = float(g["dt"]), float(g["g_const"]), float(g["softening"])
    kw = dict(positions=g["pos"], velocities=g["vel"], masses=g["mass"], g_const=gc, softening=soft, dt=dt,
              calc_energy=False, device="cuda")
    wide = simulation.LeapFrogSimulator(dtype=torch.float64, **kw)
    plain = simulation.LeapFrogSimulator(**kw)
    named = simulation.LeapFrogSimulator(dtype=torch.float32, **kw)
    assert wide.positions.dtype == wide.accelerations.dtype == torch.float64
    for sim in (plain, named):
        assert all(t.dtype == torch.float32 for t in (sim.positions, sim.velocities, sim.masses, sim.accelerations))
        assert sim._fmt is simulation._FORMATS[torch.float32] and not hasattr(sim, "_posd")
    n = plain.n
    f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=gpu_device)      # noqa: E731
    pos, vel, mass = f32(g["pos"]), f32(g["vel"]), f32(g["mass"])
    eps2, gcf = direct.f32(soft ** 2), direct.f32(gc)
    posm = direct.pack_posm(pos, mass)
    ws = direct.step_workspace(n, gpu_device)
    acc = direct.accel(posm, n, posm, n, 0, eps2, gcf)
    assert torch.equal(acc, plain.accelerations)
    wide.step(); plain.step(); named.step()
    new_acc = torch.empty_like(acc)
    direct.leapfrog_step(pos, vel, acc, new_acc, mass, direct.f32(0.5 * dt), direct.f32(dt), eps2, gcf, posm, ws,
                         uniform=plain._uniform)
    for sim in (plain, named):
        for got, want in ((sim.positions, pos), (sim.velocities, vel), (sim.accelerations, new_acc)):
            assert got.dtype == torch.float32 and torch.equal(got, want)
    assert plain._graph_run_ok(64) and not wide._graph_run_ok(64)


def test_direct_accel_float64_returns_the_simulators_bits(gpu_device):
    from galaxify import simulation
    from nbd.autograd import direct_accel
    n = 449
    x, v, m, g, eps, a, sa = _case(n)
    kw = dict(positions=x, velocities=v, masses=m, g_const=g, softening=eps, calc_energy=False, device="cuda",
              dtype=torch.float64)
    leap = simulation.LeapFrogSimulator(**kw)
    herm = simulation.HermiteSimulator(**kw)
    pos = _dev(x, gpu_device).requires_grad_(True)
    acc = direct_accel(pos, _dev(m, gpu_device), g, eps)
    assert acc.dtype == torch.float64 and acc.grad_fn is not None
    assert torch.equal(acc.detach(), leap.compute_accelerations())
    assert torch.equal(acc.detach(), herm.compute_accelerations()) and torch.equal(acc.detach(), herm.accelerations)
    _check_accel("direct_accel", _np(acc), a, sa)
    acc.sum().backward()                                  # the backward is what it was: a float64 gradient arrives
    assert pos.grad.dtype == torch.float64 and torch.isfinite(pos.grad).all()
