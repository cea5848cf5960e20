"""BatchedSimulator(integrator="hermite", dtype=torch.float64) on the MI355X (csrc/direct_batch_hermite_f64.hip): every
scene is bit-identical to a HermiteSimulator(dtype=torch.float64) of that scene alone -- state, force, energies,
potentials, invariants -- at every size at which the float64 plan takes another shape, whatever its companions; the
batch against the fp64 oracles, independently of the one-system path; captured run() == eager run() == step(); a
two-body orbit past the fp32 floor through a captured run(); NaN isolation; the float32 default untouched.

No input is fp32-representable (hermite_f64_oracle.perturbed) and every workspace is NaN-filled before each call."""
import functools

import numpy as np
import pytest
import torch

import hermite_f64_oracle as fo
import hermite_oracle as ho
from conftest import load_golden

pytestmark = pytest.mark.gpu

F64 = torch.float64
# 448 -> 449: one slab -> two (plan_f64); 1000: waves walk several chunks, both LDS buffers reused; 130: a wave without a
# chunk; 63 / 64 / 65: around one target group; 0: an empty scene, here in the middle
SIZES = [1, 2, 3, 63, 64, 65, 0, 130, 448, 449, 1000]


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _scene(name, g=1.0, eps=0.05, dt=0.01):
    """A scene as a dict, built once and never written to. name: a body count (a perturbed Plummer sphere; 0: empty) or a
    golden (perturbed, with its own parameters)."""
    if isinstance(name, int):
        if name == 0:
            x, v, m = np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0)
        else:
            x, v, m = fo.plummer_case(name, seed=300 + name)
    else:
        gd = load_golden(name)
        x, v, m = fo.perturbed(gd["pos"], gd["vel"], gd["mass"], 5)
        g, eps, dt = float(gd["g_const"]), float(gd["softening"]), float(gd["dt"])
    for arr in (x, v, m):
        arr.setflags(write=False)
    return dict(pos=x, vel=v, mass=m, g=g, eps=eps, dt=dt)


def _mixed_scenes():
    """Every size, g_const, softening and dt different per scene, then the two goldens: softening 0 (the index-masked
    walk) and a massless body."""
    sc = [_scene(n, g=1.0 + 0.07 * k, eps=0.03 + 0.011 * k, dt=0.004 + 0.0007 * k) for k, n in enumerate(SIZES)]
    sc += [_scene("direct_plummer_n64_eps0"), _scene("direct_plummer_n300_ragged_mass")]
    assert sc[-2]["eps"] == 0.0 and (sc[-1]["mass"] == 0).any()
    return sc


def _nan_fill(sim):
    """NaN into everything a call may only write before it reads: the partial sums and the packed rows."""
    for name in ("_ws", "_hws", "_posd", "_veld"):       # (a batch has _ws, a lone simulator _hws)
        t = getattr(sim, name, None)
        if t is not None:
            t.view(F64).fill_(float("nan"))


def _batch(scenes, **kw):
    from galaxify import simulation
    kw.setdefault("calc_energy", False)
    sim = simulation.BatchedSimulator(systems=[(s["pos"], s["vel"], s["mass"]) for s in scenes], integrator="hermite",
                                      g_const=[s["g"] for s in scenes], softening=[s["eps"] for s in scenes],
                                      dt=[s["dt"] for s in scenes], device="cuda", dtype=F64, **kw)
    _nan_fill(sim)
    return sim


def _lone(s, **kw):
    from galaxify import simulation
    kw.setdefault("calc_energy", False)
    sim = simulation.HermiteSimulator(positions=s["pos"], velocities=s["vel"], masses=s["mass"], g_const=s["g"],
                                      softening=s["eps"], dt=s["dt"], device="cuda", dtype=F64, **kw)
    _nan_fill(sim)
    return sim


def _rows(sim, i):
    lo, hi = int(sim.offsets[i]), int(sim.offsets[i + 1])
    return (sim.positions[lo:hi], sim.velocities[lo:hi], sim.accelerations[lo:hi], sim.jerks[lo:hi])


def _state(sim):
    return (sim.positions, sim.velocities, sim.accelerations, sim.jerks)


def _assert_equal(batch, i, lone, what):
    for nm, x, y in zip(("pos", "vel", "acc", "jerk"), _rows(batch, i), _state(lone)):
        assert x.dtype == F64 and y.dtype == F64
        assert torch.equal(x, y), (what, i, nm, float((x - y).abs().max()))


# ------------------------------------------------------------------ 1. bit-identity with the one-system simulator
def test_every_scene_is_bit_identical_to_the_lone_simulator(gpu_device):
    sc = _mixed_scenes()
    assert len({(s["g"], s["eps"], s["dt"]) for s in sc}) == len(sc)
    sim = _batch(sc)
    lones = [_lone(s) for s in sc]
    for t in (sim.positions, sim.velocities, sim.masses, sim.accelerations, sim.jerks):
        assert t.dtype == F64 and t.is_cuda
    assert np.array_equal(_np(sim.masses), np.concatenate([s["mass"] for s in sc]))           # not through fp32
    assert np.array_equal(_np(sim.positions), np.concatenate([s["pos"] for s in sc]))
    for i in range(len(sc)):
        p, v, a = sim.scene(i)
        assert p.dtype == F64 and p.data_ptr() == _rows(sim, i)[0].data_ptr() and a.shape == (len(sc[i]["mass"]), 3)
    for i, lone in enumerate(lones):
        _assert_equal(sim, i, lone, "construction")
    # the force on its own, from NaN-filled scratch: the same bits, and compute_accelerations() is its first part
    _nan_fill(sim)
    a2, j2 = sim.compute_accelerations_and_jerks()
    assert torch.equal(a2, sim.accelerations) and torch.equal(j2, sim.jerks)
    _nan_fill(sim)
    assert torch.equal(sim.compute_accelerations(), sim.accelerations)
    for k in range(10):
        _nan_fill(sim)
        sim.step()
        for lone in lones:
            _nan_fill(lone)
            lone.step()
        if k in (0, 9):
            for i, lone in enumerate(lones):
                _assert_equal(sim, i, lone, f"step {k + 1}")
    assert not torch.isnan(sim.positions).any() and not torch.isnan(sim.jerks).any()


# ------------------------------------------------------------------ 2. companions do not matter
def test_companions_and_position_do_not_matter(gpu_device):
    target = _scene(449, g=0.9, eps=0.04, dt=0.006)

    def run(scenes, idx):
        sim = _batch(scenes)
        for _ in range(5):
            _nan_fill(sim)
            sim.step()
        return [t.clone() for t in _rows(sim, idx)]
    alone = run([target], 0)
    first = run([target, _scene(65), _scene(1000, eps=0.0)], 0)
    last = run([_scene(3), _scene(0), _scene(130), target], 3)
    middle = run([_scene(1000), _scene(1), target, _scene(0), _scene(64, g=2.0)], 2)
    for other in (first, last, middle, run([target], 0)):
        for x, y in zip(alone, other):
            assert torch.equal(x, y)


# ------------------------------------------------------------------ 3. independent of the one-system path
def test_batch_against_the_oracle(gpu_device):
    """n = 3, 65, 449 in one batch. The initial (a, j) at the bar of hermite_f64_oracle ((T + 32) 2^-53 sum|terms|); after 10
    steps within 8 s_k + 8 * 2^-53 max|value| of hermite_run, s_k = the largest difference between that run and the same
    run with the bodies permuted (measured here, on the CPU) -- test_steps_against_the_oracle's tolerance."""
    sc = [_scene(3, eps=0.05, dt=0.01), _scene(65, g=1.3, eps=0.07, dt=0.008), _scene(449, g=0.8, eps=0.04, dt=0.005)]
    sim = _batch(sc)
    for i, s in enumerate(sc):
        x, v, m, g, e2, n = s["pos"], s["vel"], s["mass"], s["g"], s["eps"] ** 2, len(s["mass"])
        a, j = fo.accel_jerk(x, v, m, g, e2)
        sa, sj = fo.accel_jerk_abs(x, v, m, g, e2)
        _, _, ga, gj = _rows(sim, i)
        ok_a, f_a = fo.within(_np(ga), a, n, sa)
        ok_j, f_j = fo.within(_np(gj), j, 4 * n, sj)
        print(f"n={n}: |a - ref| / bar = {f_a:.3f}, |j - ref| / bar = {f_j:.3f}")
        assert ok_a and ok_j, (n, f_a, f_j)
    for _ in range(10):
        _nan_fill(sim)
        sim.step()
    for i, s in enumerate(sc):
        x, v, m, n = s["pos"], s["vel"], s["mass"], len(s["mass"])
        perm = np.random.default_rng(11 + n).permutation(n)
        back = np.empty_like(perm)
        back[perm] = np.arange(n)
        ref = ho.hermite_run(x, v, m, s["dt"], s["g"], s["eps"] ** 2, 10)
        prm = [q[back] for q in ho.hermite_run(x[perm], v[perm], m[perm], s["dt"], s["g"], s["eps"] ** 2, 10)]
        for name, r, p, q in zip(("pos", "vel", "acc", "jerk"), ref, prm, _rows(sim, i)):
            s_k = np.abs(r - p).max()
            dist = np.abs(_np(q) - r).max()
            tol = 8 * s_k + 8 * fo.U53 * np.abs(r).max()
            print(f"n={n} {name}: s_k = {s_k:.3e}, |gpu - oracle| = {dist:.3e}, tolerance {tol:.3e}")
            assert dist <= tol, (n, name, dist, tol)


# ------------------------------------------------------------------ 4. diagnostics
def test_diagnostics_are_the_lone_simulators_bit_for_bit(gpu_device):
    sc = _mixed_scenes()
    sim = _batch(sc)
    lones = [_lone(s) for s in sc]
    for _ in range(2):                                     # not the initial state only
        sim.step()
        for lone in lones:
            lone.step()
    _nan_fill(sim)
    u, k = sim.compute_energies()
    _nan_fill(sim)
    phi = sim.compute_potentials()
    _nan_fill(sim)
    inv = sim.compute_invariants()
    assert phi.dtype == F64 and phi.shape == (sim.n,) and len(u) == len(k) == len(inv) == len(sc)
    from galaxify.simulation import Invariants
    for i, (s, lone) in enumerate(zip(sc, lones)):
        lo, hi = int(sim.offsets[i]), int(sim.offsets[i + 1])
        _nan_fill(lone)
        assert (u[i], k[i]) == lone.compute_energies(), (i, u[i], k[i])
        _nan_fill(lone)
        assert torch.equal(phi[lo:hi], lone.compute_potentials()), i
        _nan_fill(lone)
        assert inv[i] == lone.compute_invariants(), i
        if hi == lo:
            assert (u[i], k[i]) == (0.0, 0.0) and inv[i] == Invariants.from_row([0.0] * 16)
    # n = 65: U and K against the oracle at the bar, from the state the batch holds
    i = SIZES.index(65)
    s = sc[i]
    x, v = (_np(t) for t in _rows(sim, i)[:2])
    ur, kr, ua, ka = fo.reference_energies(x, v, s["mass"], s["g"], s["eps"])
    ok_u, f_u = fo.within(u[i], ur, 65 * 64 // 2, ua)
    ok_k, f_k = fo.within(k[i], kr, 65, ka)
    print(f"n=65: |U - ref| / bar = {f_u:.4f}, |K - ref| / bar = {f_k:.3f}")
    assert ok_u and ok_k, (f_u, f_k)


# ------------------------------------------------------------------ 5. run()
def _same_states(a, b):
    assert len(a) == len(b)
    for sa, sb in zip(a, b):
        assert len(sa) == len(sb)
        for x, y in zip(sa, sb):
            for p, q in ((x.positions, y.positions), (x.velocities, y.velocities), (x.accelerations, y.accelerations)):
                assert p.dtype == F64 and not p.is_cuda and torch.equal(p, q)
            assert (x.step, x.u_energy, x.k_energy, x.invariants) == (y.step, y.u_energy, y.k_energy, y.invariants)


@pytest.mark.parametrize("calc_energy", [True, False])
def test_run_captured_eager_and_steps_agree(gpu_device, monkeypatch, calc_energy):
    sc = [_scene(3), _scene(0), _scene(65, g=1.2, eps=0.06, dt=0.007), _scene(449, eps=0.04), _scene(1)]
    kw = dict(calc_energy=calc_energy, calc_invariants=calc_energy)
    steps = 20                                             # captured: 8 + 8, then 4 eager
    ran, eager, twin = (_batch(sc, **kw) for _ in range(3))
    monkeypatch.setenv("NBD_RUN_GRAPH", "1")
    assert ran._chunk_len() >= 8
    captured = ran.run(steps)
    assert len(ran._run_graphs) >= 1                       # chunks were captured and replayed
    monkeypatch.setenv("NBD_RUN_GRAPH", "0")
    plain = eager.run(steps)
    assert not getattr(eager, "_run_graphs", None)
    _same_states(captured, plain)
    assert all(len(s) == steps for s in captured) and [s.step for s in captured[2]] == list(range(steps))
    for k in range(steps):
        _nan_fill(twin)
        twin.step()
        if calc_energy:
            u, kin = twin.compute_energies()
            inv = twin.compute_invariants()
        for i in range(len(sc)):
            st = captured[i][k]
            for got, want in zip((st.positions, st.velocities, st.accelerations), _rows(twin, i)):
                assert torch.equal(got, want.cpu()), (k, i)
            if calc_energy:
                assert (st.u_energy, st.k_energy, st.invariants) == (u[i], kin[i], inv[i]), (k, i)
            else:
                assert st.u_energy is None and st.k_energy is None and st.invariants is None
    for a, b in zip(_state(ran), _state(twin)):
        assert torch.equal(a, b)


def test_changing_dt_between_runs_takes_effect(gpu_device, monkeypatch):
    monkeypatch.setenv("NBD_RUN_GRAPH", "1")
    sc = [_scene(65, eps=0.06, dt=0.007), _scene(130, g=1.1, dt=0.005)]
    sim = _batch(sc)
    lones = [_lone(s) for s in sc]
    sim.run(8)
    sim.dt = [0.003, 0.011]
    sim.softening = [0.05, 0.02]
    out = sim.run(9)                                       # a new table, the same buffer: 8 captured + 1 eager
    for lone, dt, eps in zip(lones, sim.dt, sim.softening):
        for _ in range(8):
            lone.step()
        lone.dt, lone.softening = dt, eps
        for _ in range(9):
            lone.step()
    for i, lone in enumerate(lones):
        _assert_equal(sim, i, lone, "after the change")
        assert torch.equal(out[i][-1].positions, lone.positions.cpu())


# ------------------------------------------------------------------ 6. past the fp32 floor
def test_two_body_orbit_through_a_captured_run(gpu_device, monkeypatch):
    """e = 0.5, eps = 0.1, one period in 2048 steps as one scene among two Plummer companions: test_two_body_orbit's
    bounds for the one-system path, which this is bit-identical to."""
    monkeypatch.setenv("NBD_RUN_GRAPH", "1")
    steps = 2048
    x, v, m, period = ho.two_body(0.5)
    x, v, m = fo.perturbed(x, v, m, 9)
    eps, dt = 0.1, period / steps
    orbit = dict(pos=x, vel=v, mass=m, g=1.0, eps=eps, dt=dt)
    sim = _batch([_scene(65), orbit, _scene(130, dt=0.002)])
    e0_gpu = sim.compute_invariants()[1].energy
    states = sim.run(steps)
    assert states[1][0].u_energy is None and len(sim._run_graphs) >= 1
    ref = ho.hermite_run(x, v, m, dt, 1.0, eps * eps, steps)
    dist = ho.orbit_error(_np(_rows(sim, 1)[0]), ref[0])
    e0 = fo.energy(x, v, m, 1.0, eps * eps)
    err_ref = abs(fo.energy(ref[0], ref[1], m, 1.0, eps * eps) - e0) / abs(e0)
    err_gpu = abs(sim.compute_invariants()[1].energy - e0_gpu) / abs(e0_gpu)
    print(f"|x_gpu - x_oracle| = {dist:.3e}, energy error gpu {err_gpu:.6e} oracle {err_ref:.6e}")
    assert torch.equal(states[1][-1].positions, _rows(sim, 1)[0].cpu())
    assert dist <= 1e-10, dist
    assert abs(err_gpu - err_ref) <= max(0.01 * err_ref, 1e-13), (err_gpu, err_ref)


# ------------------------------------------------------------------ 7. poison stays in its scene
def test_nan_stays_in_its_scene(gpu_device):
    healthy = _scene(130, eps=0.04)
    x = np.array(_scene(3)["pos"])
    x[1] = x[0]                                            # two coincident bodies at softening 0: 0 * inf
    poison = dict(_scene(3), pos=x, eps=0.0)
    sim = _batch([healthy, poison, _scene(65)])
    alone = _batch([healthy])
    for _ in range(3):
        sim.step()
        alone.step()
    assert torch.isnan(_rows(sim, 1)[2]).any()
    for i in (0, 2):
        assert not any(torch.isnan(t).any() for t in _rows(sim, i))
    for a, b in zip(_rows(sim, 0), _rows(alone, 0)):
        assert torch.equal(a, b)
    u, k = sim.compute_energies()
    assert u[0] == alone.compute_energies()[0][0] and np.isfinite(u[2])


# ------------------------------------------------------------------ 8. the default is untouched
def test_default_dtype_is_untouched(gpu_device):
    """A default-dtype batch built beside a float64 one keeps float32 tensors, and its first step is
    direct.batch_hermite_step driven directly, bit for bit."""
    from galaxify import simulation
    from nbd import direct
    g = [load_golden("direct_plummer_n300_ragged_mass"), load_golden("direct_plummer_n64_eps0")]
    kw = dict(systems=[(q["pos"], q["vel"], q["mass"]) for q in g], integrator="hermite",
              g_const=[float(q["g_const"]) for q in g], softening=[float(q["softening"]) for q in g],
              dt=[float(q["dt"]) for q in g], calc_energy=False, device="cuda")
    wide = simulation.BatchedSimulator(dtype=F64, **kw)
    plain = simulation.BatchedSimulator(**kw)
    named = simulation.BatchedSimulator(dtype=torch.float32, **kw)
    assert wide.positions.dtype == F64 and wide._params.dtype == F64
    for sim in (plain, named):
        assert all(t.dtype == torch.float32 for t in
                   (sim.positions, sim.velocities, sim.masses, sim.accelerations, sim.jerks, sim._params))
    f32 = lambda k: torch.tensor(np.concatenate([np.asarray(q[k]) for q in g]), dtype=torch.float32,      # noqa: E731
                                 device=gpu_device)
    pos, vel, mass = f32("pos"), f32("vel"), f32("mass")
    plan = direct.BatchPlan([len(q["mass"]) for q in g], gpu_device)
    P = torch.tensor([[direct.f32(float(q["g_const"])) for q in g], [direct.f32(float(q["softening"]) ** 2) for q in g]]
                     + [[direct.f32(c(float(q["dt"]))) for q in g] for c in
                        (lambda d: d, lambda d: 0.5 * d, lambda d: 0.5 * d * d, lambda d: d * d * d / 6.0,
                         lambda d: d * d / 12.0)], dtype=torch.float32, device=gpu_device)
    posm, hws = plan.alloc_posm(), plan.hermite_workspace()
    acc, jerk = torch.zeros_like(pos), torch.zeros_like(pos)
    direct.batch_accel_jerk(plan, pos, vel, mass, P[1], P[0], acc, jerk, posm, hws)
    assert torch.equal(acc, plain.accelerations) and torch.equal(jerk, plain.jerks)
    wide.step(); plain.step(); named.step()
    direct.batch_hermite_step(plan, pos, vel, acc, jerk, acc, jerk, mass, P[2:7], P[1], P[0], posm, hws)
    for sim in (plain, named):
        for got, want in ((sim.positions, pos), (sim.velocities, vel), (sim.accelerations, acc), (sim.jerks, jerk)):
            assert got.dtype == torch.float32 and torch.equal(got, want)
