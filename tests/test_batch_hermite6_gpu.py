"""BatchedSimulator(integrator="hermite6") on the MI355X (csrc/direct_batch_hermite_f64.hip): every scene is bit-identical
to a Hermite6Simulator of that scene alone -- construction, steps, captured run(), energies, invariants -- whatever its
companions and its place in the batch; the batch against the fp64 oracle of tests/hermite6_oracle.py, independently of
the one-system path; a two-body orbit through a captured run(); the existing modes untouched.

The standard ensemble is [3, 0, 64, 65, 1, 130, 520, 1000] with every scalar different per scene and one softening 0 (the
index-masked walk): an empty scene, a single body, the chunk edge 64 / 65, one slab with idle waves (130), two ragged
slabs (520), four slabs (1000). No input is fp32-representable (hermite_f64_oracle.perturbed) and every workspace is
NaN-filled before a call."""
import functools

import numpy as np
import pytest
import torch

import hermite6_oracle as h6
import hermite_f64_oracle as fo
import hermite_oracle as ho

pytestmark = pytest.mark.gpu

F64 = torch.float64
SIZES = [3, 0, 64, 65, 1, 130, 520, 1000]
CARRIED = ("accelerations", "jerks", "snaps", "crackles")
STATE = ("positions", "velocities") + CARRIED


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _scene(n, g=1.0, eps=0.05, dt=0.01):
    """A perturbed Plummer sphere of n bodies (0: empty) as a dict, built once and never written to."""
    if n == 0:
        x, v, m = np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0)
    else:
        x, v, m = fo.plummer_case(n, seed=700 + n)
    for arr in (x, v, m):
        arr.setflags(write=False)
    return dict(pos=x, vel=v, mass=m, g=g, eps=eps, dt=dt)


def _ensemble():
    """The standard ensemble: g_const, softening and dt different per scene; n = 65 at softening 0."""
    sc = [_scene(n, g=1.0 + 0.07 * k, eps=0.0 if n == 65 else 0.03 + 0.011 * k, dt=0.004 + 0.0007 * k)
          for k, n in enumerate(SIZES)]
    assert [s["eps"] for s in sc].count(0.0) == 1
    return sc


def _nan_fill(sim):
    """NaN into everything a call may only write before it reads: the partial sums and the packed rows."""
    for name in ("_ws", "_hws", "_posd", "_veld", "_accd"):      # (a batch has _ws, a lone simulator _hws)
        t = getattr(sim, name, None)
        if t is not None:
            t.view(F64).fill_(float("nan"))


def _batch(scenes, integrator="hermite6", **kw):
    from galaxify import simulation
    kw.setdefault("calc_energy", False)
    sim = simulation.BatchedSimulator(systems=[(s["pos"], s["vel"], s["mass"]) for s in scenes], integrator=integrator,
                                      g_const=[s["g"] for s in scenes], softening=[s["eps"] for s in scenes],
                                      dt=[s["dt"] for s in scenes], device="cuda", **kw)
    _nan_fill(sim)
    return sim


def _lone(s, **kw):
    from galaxify import simulation
    kw.setdefault("calc_energy", False)
    sim = simulation.Hermite6Simulator(positions=s["pos"], velocities=s["vel"], masses=s["mass"], g_const=s["g"],
                                       softening=s["eps"], dt=s["dt"], device="cuda", **kw)
    _nan_fill(sim)
    return sim


def _rows(sim, i, names=STATE):
    lo, hi = int(sim.offsets[i]), int(sim.offsets[i + 1])
    return [getattr(sim, nm)[lo:hi] for nm in names]


def _assert_equal(batch, i, lone, what, names=STATE):
    for nm, x in zip(names, _rows(batch, i, names)):
        y = getattr(lone, nm)
        assert x.dtype == F64 and y.dtype == F64 and x.shape == y.shape
        assert torch.equal(x, y), (what, i, nm, float((x - y).abs().max()))


# ------------------------------------------------------------------ 1. construction
def test_construction_is_the_lone_simulators_bit_for_bit(gpu_device):
    sc = _ensemble()
    assert len({(s["g"], s["eps"], s["dt"]) for s in sc}) == len(sc)
    sim = _batch(sc)
    assert sim._params.shape == (13, len(sc)) and sim._plan.order == 6
    lones = [_lone(s) for s in sc]
    for nm in STATE + ("masses",):
        t = getattr(sim, nm)
        assert t.dtype == F64 and t.is_cuda and t.shape == ((sim.n,) if nm == "masses" else (sim.n, 3)), nm
    assert np.array_equal(_np(sim.positions), np.concatenate([s["pos"] for s in sc]))           # not through fp32
    assert np.array_equal(_np(sim.masses), np.concatenate([s["mass"] for s in sc]))
    assert not sim.crackles.any()
    for i, lone in enumerate(lones):
        _assert_equal(sim, i, lone, "construction")
    # the evaluation on its own, from NaN-filled scratch: the same bits in new tensors; the inherited ones are its parts
    _nan_fill(sim)
    a2, j2, s2 = sim.compute_accelerations_jerks_and_snaps()
    assert torch.equal(a2, sim.accelerations) and torch.equal(j2, sim.jerks) and torch.equal(s2, sim.snaps)
    assert a2.data_ptr() != sim.accelerations.data_ptr() and s2.data_ptr() != sim.snaps.data_ptr()
    _nan_fill(sim)
    a3, j3 = sim.compute_accelerations_and_jerks()
    assert torch.equal(a3, sim.accelerations) and torch.equal(j3, sim.jerks)
    assert torch.equal(sim.compute_accelerations(), sim.accelerations)
    # an anchor that does not pass through the lone kernel: the snap of the two-slab scene at the project's fp64 bar,
    # against the oracle on the rows the kernel was given
    i = SIZES.index(520)
    s = sc[i]
    _, _, a, _, snap, _ = (_np(t) for t in _rows(sim, i))
    ref, s_abs = h6.snap_and_abs(s["pos"], s["vel"], a, s["mass"], s["g"], s["eps"] ** 2)
    ok, frac = fo.within(snap, ref, 19 * 520, s_abs)
    print(f"n=520: |s - ref| / bar = {frac:.4f}")
    assert ok, frac


# ------------------------------------------------------------------ 2. steps
@functools.lru_cache(maxsize=None)
def _lone_after_five_steps(k):
    """Scene k of the ensemble alone, after 5 steps: clones of its six arrays, computed once."""
    lone = _lone(_ensemble()[k])
    for _ in range(5):
        _nan_fill(lone)
        lone.step()
    return [getattr(lone, nm).clone() for nm in STATE]


def _five_steps(scenes):
    sim = _batch(scenes)
    for _ in range(5):
        old = [getattr(sim, nm) for nm in CARRIED]
        _nan_fill(sim)
        sim.step()
        assert all(getattr(sim, nm) is not o for nm, o in zip(CARRIED, old))       # rebound
    return sim


def test_steps_are_the_lone_simulators_bit_for_bit(gpu_device):
    sc = _ensemble()
    sim = _five_steps(sc)
    for k in range(len(sc)):
        for nm, x, y in zip(STATE, _rows(sim, k), _lone_after_five_steps(k)):
            assert torch.equal(x, y), ("forward", k, nm)
    assert not any(torch.isnan(getattr(sim, nm)).any() for nm in STATE)
    again = _five_steps(sc)                                 # NaN-refilled workspace, a second simulator: the same bits
    for nm in STATE:
        assert torch.equal(getattr(sim, nm), getattr(again, nm)), nm


def test_companions_and_position_do_not_matter(gpu_device):
    sc = _ensemble()
    S = len(sc)
    back = _five_steps(sc[::-1])
    for k in range(S):
        for nm, x, y in zip(STATE, _rows(back, S - 1 - k), _lone_after_five_steps(k)):
            assert torch.equal(x, y), ("reversed", k, nm)
    for k in (SIZES.index(65), SIZES.index(520), SIZES.index(1000)):
        alone = _five_steps([sc[k]])
        for nm, x, y in zip(STATE, _rows(alone, 0), _lone_after_five_steps(k)):
            assert torch.equal(x, y), ("alone", k, nm)


# ------------------------------------------------------------------ 3. independent of the one-system path
def _oracle_states(x, v, m, dt, g, eps2, marks):
    """The oracle's (x, v, a, j, s, c) after each step count of `marks`, from one run."""
    state = (np.array(x), np.array(v)) + h6.start(x, v, m, g, eps2)
    out = {}
    for k in range(1, max(marks) + 1):
        state = h6.hermite6_step(*state, m, dt, g, eps2)
        if k in marks:
            out[k] = state
    return out


def test_batch_against_the_oracle(gpu_device):
    """n = 65, 130, 520 in one batch, each with its own G, softening and dt, after 1 and 10 steps: within
    8 s_k + 8 * 2^-53 max|value| of hermite6_run, s_k = the largest difference between that run and the same run with the
    bodies permuted (measured here, on the CPU) -- test_hermite6_gpu.py::test_steps_against_the_oracle's marks and bound.
    The crackle of every step is the c1 formula on the batch's own (a, j, s) before and after the step, componentwise
    within 16 * 2^-53 of the sum of its |terms|, as there."""
    sc = [_scene(65, g=1.3, eps=0.07, dt=0.008), _scene(130, eps=0.05, dt=0.01), _scene(520, g=0.8, eps=0.04, dt=0.005)]
    marks = (1, 10)
    refs, prms, backs = [], [], []
    for s in sc:
        x, v, m, n = s["pos"], s["vel"], s["mass"], len(s["mass"])
        perm = np.random.default_rng(11 + n).permutation(n)
        back = np.empty_like(perm)
        back[perm] = np.arange(n)
        refs.append(_oracle_states(x, v, m, s["dt"], s["g"], s["eps"] ** 2, marks))
        prms.append(_oracle_states(x[perm], v[perm], m[perm], s["dt"], s["g"], s["eps"] ** 2, marks))
        backs.append(back)
    sim = _batch(sc)
    done = 0
    for k in marks:
        while done < k:
            before = [[_np(t) for t in _rows(sim, i, CARRIED[:3])] for i in range(len(sc))]
            _nan_fill(sim)
            sim.step()
            done += 1
            for i, s in enumerate(sc):
                after = [_np(t) for t in _rows(sim, i, CARRIED[:3])]
                c_err = np.abs(_np(_rows(sim, i, ("crackles",))[0]) - h6.crackle(*before[i], *after, s["dt"]))
                c_tol = 16 * fo.U53 * h6.crackle_abs(*before[i], *after, s["dt"])
                assert np.all(c_err <= c_tol), (done, i, float((c_err / c_tol).max()))
        for i, s in enumerate(sc):
            n = len(s["mass"])
            got = [_np(t) for t in _rows(sim, i, STATE[:5])]
            for name, r, p, q in zip(("pos", "vel", "acc", "jerk", "snap"), refs[i][k], prms[i][k], got):
                s_k = np.abs(r - p[backs[i]]).max()
                dist = np.abs(q - r).max()
                tol = 8 * s_k + 8 * fo.U53 * np.abs(r).max()
                print(f"n={n} steps={k} {name}: s_k = {s_k:.3e}, |gpu - oracle| = {dist:.3e}, tolerance {tol:.3e}")
                assert dist <= tol, (n, k, name, dist, tol)


# ------------------------------------------------------------------ 4. run()
def _same_states(a, b, what):
    assert len(a) == len(b)
    for sa, sb in zip(a, b):
        assert len(sa) == len(sb)
        for x, y in zip(sa, sb):
            for p, q in ((x.positions, y.positions), (x.velocities, y.velocities), (x.accelerations, y.accelerations)):
                assert p.dtype == F64 and not p.is_cuda and torch.equal(p, q), what
            assert (x.step, x.u_energy, x.k_energy, x.invariants) == (y.step, y.u_energy, y.k_energy, y.invariants), what


def test_run_captured_eager_steps_and_lone_runs_agree(gpu_device, monkeypatch):
    sc = _ensemble()
    kw = dict(calc_energy=True, calc_invariants=True)
    steps = 45                                             # captured: 32 + 8, then 5 eager
    ran, eager, twin = (_batch(sc, **kw) for _ in range(3))
    monkeypatch.setenv("NBD_RUN_GRAPH", "1")
    assert ran._chunk_len() == 32
    captured = ran.run(steps)
    assert sorted(k[0] for k in ran._run_graphs) == [8, 32]                  # both chunk lengths captured and replayed
    assert all(len(s) == steps for s in captured) and [s.step for s in captured[3]] == list(range(steps))
    monkeypatch.setenv("NBD_RUN_GRAPH", "0")
    plain = eager.run(steps)
    assert not getattr(eager, "_run_graphs", None)
    _same_states(captured, plain, "NBD_RUN_GRAPH=0")
    for k in range(steps):
        _nan_fill(twin)
        twin.step()
        u, kin = twin.compute_energies()
        inv = twin.compute_invariants()
        for i in range(len(sc)):
            st = captured[i][k]
            for got, want in zip((st.positions, st.velocities, st.accelerations), _rows(twin, i)):
                assert torch.equal(got, want.cpu()), (k, i)
            assert (st.u_energy, st.k_energy, st.invariants) == (u[i], kin[i], inv[i]), (k, i)
    for nm in STATE:
        assert torch.equal(getattr(ran, nm), getattr(twin, nm)), nm
    # the lone simulators' own run(45)
    for i, s in enumerate(sc):
        lone = _lone(s, **kw)
        if SIZES[i] == 0:                                  # (nothing to run alone: the batch's states of it are empty)
            assert all(st.positions.shape == (0, 3) and (st.u_energy, st.k_energy) == (0.0, 0.0) for st in captured[i])
            continue
        _same_states([captured[i]], [lone.run(steps)], f"lone run, scene {i}")
        _assert_equal(ran, i, lone, "after run()")


def test_changing_dt_between_runs_takes_effect(gpu_device, monkeypatch):
    monkeypatch.setenv("NBD_RUN_GRAPH", "1")
    sc = [_scene(65, eps=0.06, dt=0.007), _scene(130, g=1.1, dt=0.005), _scene(3, dt=0.002)]
    sim = _batch(sc)
    lones = [_lone(s) for s in sc]
    sim.run(8)
    table = sim._params.data_ptr()
    keys = set(sim._run_graphs)
    sim.dt = [0.003, 0.011, 0.0045]
    out = sim.run(8)
    assert sim._params.data_ptr() == table and len(set(sim._run_graphs) - keys) == 1    # rewritten in place, a new key
    assert _np(sim._params[3]).tolist() == sim.dt
    for lone, dt in zip(lones, sim.dt):
        for _ in range(8):
            lone.step()
        lone.dt = dt
        for _ in range(8):
            lone.step()
    for i, lone in enumerate(lones):
        _assert_equal(sim, i, lone, "after the change")
        assert torch.equal(out[i][-1].positions, lone.positions.cpu())


# ------------------------------------------------------------------ 5. a two-body orbit through a captured run()
def test_two_body_orbit_through_a_captured_run(gpu_device, monkeypatch):
    """e = 0.5, eps = 0.1, one period in 512 steps as one scene among two Plummer companions:
    test_hermite6_gpu.py::test_two_body_orbit's criterion at 512 steps -- the final positions within 1e-10 of hermite6_run
    with the same steps, the relative energy error of compute_invariants() equal to the oracle's own to 1 % or 1e-13."""
    monkeypatch.setenv("NBD_RUN_GRAPH", "1")
    steps = 512
    x, v, m, period = ho.two_body(0.5)
    x, v, m = fo.perturbed(x, v, m, 9)
    eps, dt = 0.1, period / steps
    orbit = dict(pos=x, vel=v, mass=m, g=1.0, eps=eps, dt=dt)
    sim = _batch([_scene(65), orbit, _scene(130, dt=0.002)])
    e0_gpu = sim.compute_invariants()[1].energy
    states = sim.run(steps)
    assert states[1][0].u_energy is None and len(sim._run_graphs) >= 1
    ref = h6.hermite6_run(x, v, m, dt, 1.0, eps * eps, steps)
    dist = ho.orbit_error(_np(_rows(sim, 1)[0]), ref[0])
    e0 = fo.energy(x, v, m, 1.0, eps * eps)
    err_ref = abs(fo.energy(ref[0], ref[1], m, 1.0, eps * eps) - e0) / abs(e0)
    err_gpu = abs(sim.compute_invariants()[1].energy - e0_gpu) / abs(e0_gpu)
    print(f"S={steps}: |x_gpu - x_oracle| = {dist:.3e}, energy error gpu {err_gpu:.6e} oracle {err_ref:.6e}")
    assert torch.equal(states[1][-1].positions, _rows(sim, 1)[0].cpu())
    assert dist <= 1e-10, dist
    assert abs(err_gpu - err_ref) <= max(0.01 * err_ref, 1e-13), (err_gpu, err_ref)


# ------------------------------------------------------------------ 6. what was there is untouched
def test_integrator_cannot_switch_into_out_of_or_between_the_hermites(gpu_device):
    sc = [_scene(3), _scene(65)]
    six = _batch(sc)
    four = _batch(sc, integrator="hermite", dtype=F64)
    assert four.snaps is None and four.crackles is None and four._plan.order == 4
    for sim, other in ((six, "hermite"), (six, "leapfrog"), (four, "hermite6")):
        was = sim.integrator
        sim.integrator = other
        with pytest.raises(ValueError, match="hermite6"):
            sim.step()
        with pytest.raises(ValueError, match="hermite6"):
            sim.run(1)
        sim.integrator = was
        sim.step()
    with pytest.raises(ValueError, match="hermite6"):
        four.compute_accelerations_jerks_and_snaps()


def test_existing_modes_are_untouched(gpu_device):
    """A float64 4th-order batch and a lone Hermite6Simulator built beside a 6th-order batch: their first step is the
    unchanged one-system entries (nbd_hermite_step_f64 resp. nbd_hermite6_step_f64) driven directly, bit for bit."""
    from galaxify import simulation
    from nbd import direct
    s = _scene(130, g=1.1, eps=0.04, dt=0.006)
    n, g, eps2, dt = 130, s["g"], s["eps"] ** 2, s["dt"]
    six = _batch([_scene(3), s])
    four = _batch([_scene(3), s], integrator="hermite", dtype=F64)
    lone = _lone(s)
    assert four._params.shape == (8, 2) and not hasattr(four, "_accd")
    six.step(); four.step(); lone.step()
    dev = lambda a: torch.tensor(np.asarray(a), dtype=F64, device=gpu_device)          # noqa: E731
    # the 4th-order float64 step, as test_hermite6_gpu drives it
    pos, vel, mass = dev(s["pos"]), dev(s["vel"]), dev(s["mass"])
    posd, veld = direct.alloc_rows_f64(n, gpu_device), direct.alloc_rows_f64(n, gpu_device)
    ws = direct.hermite_f64_workspace(n, gpu_device)
    direct.hermite_f64_pack(pos, vel, mass, posd, veld)
    acc, jerk = direct.accel_jerk_f64(posd, veld, n, eps2, g, workspace=ws)
    direct.hermite_step_f64(pos, vel, acc, jerk, acc, jerk, mass, dt, eps2, g, posd, veld, ws)
    for got, want in zip(_rows(four, 1, STATE[:4]), (pos, vel, acc, jerk)):
        assert got.dtype == F64 and torch.equal(got, want)
    # the 6th-order one-system step
    pos, vel = dev(s["pos"]), dev(s["vel"])
    accd = direct.alloc_rows_f64(n, gpu_device)
    hws = direct.hermite6_workspace(n, gpu_device)
    direct.hermite_f64_pack(pos, vel, mass, posd, veld)
    a0 = direct.accel_jerk_f64(posd, veld, n, eps2, g, workspace=ws)[0]
    direct.hermite6_pack(pos, vel, mass, posd, veld, accd, acc=a0)
    a, j, sn = direct.accel_jerk_snap_f64(posd, veld, accd, n, eps2, g, workspace=hws)
    c = torch.zeros_like(a)
    direct.hermite6_step_f64(pos, vel, a, j, sn, c, a, j, sn, c, mass, dt, eps2, g, posd, veld, accd, hws)
    for nm, want in zip(STATE, (pos, vel, a, j, sn, c)):
        assert torch.equal(getattr(lone, nm), want), nm
    _assert_equal(six, 1, lone, "beside the others")
