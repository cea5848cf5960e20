"""BlockHermiteSimulator and the nbd_hblock_* / nbd_accel_jerk_active_f32 kernels on the MI355X: max_level 0 is the shared
step bit for bit, the active-subset force against the fp64 restatement and against the all-bodies kernel, the level
schedule and state against the fp64 block oracle (block_hermite_oracle.py), that block steps pay on an eccentric orbit
and a planted binary, run() against eager steps, determinism, re-levelling, NaN termination and the dataset CLI."""
import csv
import importlib.util
import os

import numpy as np
import pytest
import torch

import block_hermite_oracle as bo
import hermite_oracle as ho
from conftest import PKG, golden_cases, load_golden, row_rel

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _np(t):
    return t.detach().cpu().numpy()


def _f32(x):
    return float(np.float32(x))


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _sim(cls, x, v, m, **kw):
    from galaxify import simulation
    kw.setdefault("device", "cuda")
    return getattr(simulation, cls)(positions=np.asarray(x, np.float32), velocities=np.asarray(v, np.float32),
                                    masses=np.asarray(m, np.float32), **kw)


def _golden_kw(g):
    return dict(g_const=float(g["g_const"]), softening=float(g["softening"]), dt=float(g["dt"]), calc_energy=True)


@pytest.mark.parametrize("name", golden_cases())
def test_max_level_zero_is_the_shared_step_bit_for_bit(name, gpu_device):
    g = load_golden(name)
    n = g["pos"].shape[0]
    for steps in (1, 10):
        shared = _sim("HermiteSimulator", g["pos"], g["vel"], g["mass"], **_golden_kw(g))
        block = _sim("BlockHermiteSimulator", g["pos"], g["vel"], g["mass"], max_level=0, **_golden_kw(g))
        want, got = shared.run(steps), block.run(steps)
        for a, b in zip(want, got):
            for f in ("positions", "velocities", "accelerations"):
                assert torch.equal(getattr(a, f), getattr(b, f)), (name, steps, a.step, f)
            assert (a.u_energy, a.k_energy) == (b.u_energy, b.k_energy), (name, steps, a.step)
        assert torch.equal(shared.jerks, block.jerks) and torch.equal(shared.accelerations, block.accelerations)
        assert block.pair_interactions == steps * n * n and block.block_steps == steps


def _active_cases():
    from nbd.plummer import generate_plummer
    for name in golden_cases():
        g = load_golden(name)
        yield name, g["pos"], g["vel"], g["mass"], float(g["g_const"]), float(g["softening"]) ** 2
    p, v, m = generate_plummer(5000, seed=3)
    for eps in (0.0, 0.01):
        yield f"plummer5000_eps{eps}", p, v, m, 1.0, eps ** 2


@pytest.mark.parametrize("case", list(range(len(golden_cases()) + 2)))
def test_active_subset_force(case, gpu_device):
    from nbd import direct
    name, p, v, m, gc, eps2 = list(_active_cases())[case]
    n = p.shape[0]
    pos = torch.tensor(p, dtype=torch.float32, device=gpu_device)
    vel = torch.tensor(v, dtype=torch.float32, device=gpu_device)
    mass = torch.tensor(m, dtype=torch.float32, device=gpu_device)
    posm, velp = direct.alloc_posm(n, gpu_device), direct.alloc_posm(n, gpu_device)
    direct.hermite_pack(pos, vel, mass, posm, velp)
    eps2 = _f32(eps2)
    a_ref, j_ref = ho.accel_jerk(_f64(p), _f64(v), _f64(m), _f32(gc), eps2)
    rng = np.random.default_rng(case)
    lists = {"empty": np.zeros(0, np.int64), "one": np.array([n // 2]),
             "ragged": np.sort(rng.choice(n, size=max(1, (n * 3) // 7) if n > 1 else 1, replace=False)),
             "unordered": rng.permutation(n)[: max(1, n - n // 5)], "all": np.arange(n)}
    ws = direct.hblock_workspace(n, gpu_device)
    for kind, idx in lists.items():
        act = torch.tensor(idx, dtype=torch.int32, device=gpu_device)
        acc, jerk = direct.accel_jerk_active(posm, velp, n, act, eps2, _f32(gc), workspace=ws)
        assert acc.shape == (idx.size, 3) and jerk.shape == (idx.size, 3)
        if idx.size == 0:
            continue
        assert row_rel(_np(acc), a_ref[idx]) < TOL, (name, kind, row_rel(_np(acc), a_ref[idx]))
        assert row_rel(_np(jerk), j_ref[idx]) < TOL, (name, kind, row_rel(_np(jerk), j_ref[idx]))
    all_acc, all_jerk = direct.accel_jerk_active(posm, velp, n, torch.arange(n, dtype=torch.int32, device=gpu_device),
                                                 eps2, _f32(gc), workspace=ws)
    full_acc, full_jerk = direct.accel_jerk(posm, velp, n, eps2, _f32(gc))
    assert torch.equal(all_acc, full_acc) and torch.equal(all_jerk, full_jerk), name


# seeds of the planted-binary sphere whose fp64 criterion values all miss a level boundary by >= 1e-3 over one output
# step (dt = 1/32, eta = 0.02, max_level 10): fp32 and fp64 must then choose the same levels
PLANTED = {0.0: 93, 0.01: 38}
DT = 1.0 / 32


@pytest.mark.parametrize("eps", [0.0, 0.01])
def test_levels_and_state_match_the_fp64_oracle(eps, gpu_device):
    x, v, m = (_f64(t) for t in bo.planted_binary_sphere(256, PLANTED[eps]))
    eps2 = _f32(eps ** 2)
    want = bo.block_run(x, v, m, DT, 1.0, eps2, 1)
    assert want["margin"] >= 1e-3, want["margin"]
    sim = _sim("BlockHermiteSimulator", x, v, m, softening=eps, dt=DT, calc_energy=False)
    sim.level_history = []
    sim.step()
    assert sim.block_steps == want["block_steps"] and sim.pair_interactions == want["pair_interactions"]
    assert len(sim.level_history) == len(want["history"])
    for k, (a, b) in enumerate(zip(sim.level_history, want["history"])):
        assert np.array_equal(a.numpy(), b), k
    assert row_rel(_np(sim.positions), want["x"]) < TOL and row_rel(_np(sim.velocities), want["v"]) < TOL
    levels = _np(sim.levels)
    assert levels[:2].min() > np.median(levels)                 # the binary runs deeper than the median body
    assert sim.clamped == want["clamped"] == 0

    # 8 output steps: no further from the oracle than 10x the shared step's fp32-vs-fp64 distance on the same case (at
    # the block run's finest step over the binary, dt / 2^levels[0])
    sim.level_history = None
    for _ in range(7):
        sim.step()
    want8 = bo.block_run(x, v, m, DT, 1.0, eps2, 8)
    err_block = max(row_rel(_np(sim.positions), want8["x"]), row_rel(_np(sim.velocities), want8["v"]))
    fine = DT / 2 ** int(want["levels"][0])
    shared = _sim("HermiteSimulator", x, v, m, softening=eps, dt=fine, calc_energy=False)
    steps = round(8 * DT / fine)
    for _ in range(steps):
        shared.step()
    sx, sv, _, _ = ho.hermite_run(x, v, m, fine, 1.0, eps2, steps)
    err_shared = max(row_rel(_np(shared.positions), sx), row_rel(_np(shared.velocities), sv))
    assert err_block <= 10 * err_shared, (err_block, err_shared)


def _orbit_block(eta, max_level=12, history=False):
    x0, v0, m, period = ho.two_body(0.9)
    sim = _sim("BlockHermiteSimulator", x0, v0, m, softening=0.0, dt=period / 4, calc_energy=False, eta=eta,
               max_level=max_level)
    if history:
        sim.level_history = []
    for _ in range(4):
        sim.step()
    return sim, ho.orbit_error(_np(sim.positions), x0.astype(np.float32))


def test_block_steps_pay_on_the_eccentric_orbit(gpu_device):
    """e = 0.9, eps = 0, one period, against shared Hermite with at least as many pair interactions.
    1. Block eta = 0.16 against shared steps of equal cost: fp64 oracle 1.75e-3 at 356 pairs against 4.1 for 89 shared
       steps (at this cost the shared orbit is lost), a factor of 2 300; the GPU factor must be at least the oracle's.
    2. Where the shared orbit is not lost: block eta = 0.01 (1 412 pairs, near the fp32 floor of the orbit, ~1e-5)
       against 1 024 shared steps (4 096 pairs, 2.9e-3): at least 10x smaller at under half the pairs."""
    x0, v0, m, period = ho.two_body(0.9)
    block, err_block = _orbit_block(0.16, history=True)
    lv = np.array([h.numpy()[0] for h in block.level_history])
    assert lv.max() >= lv.min() + 3, (lv.min(), lv.max())       # pericentre runs deeper than apocentre
    # started at apocentre (the first level is the (eta/2)|a|/|j| estimate, one level off at most); by symmetry the
    # middle block step lies at pericentre
    assert lv[0] <= lv.min() + 1 and lv[len(lv) // 2] >= lv.max() - 1, lv
    steps = -(-block.pair_interactions // 4)
    shared = _sim("HermiteSimulator", x0, v0, m, softening=0.0, dt=period / steps, calc_energy=False)
    for _ in range(steps):
        shared.step()
    err_shared = ho.orbit_error(_np(shared.positions), x0.astype(np.float32))
    assert steps * 4 >= block.pair_interactions
    ref = bo.block_run(x0, v0, m, period / 4, 1.0, 0.0, 4, eta=0.16, max_level=12)
    assert ref["pair_interactions"] == block.pair_interactions
    oracle_factor = ho.orbit_error(ho.hermite_run(x0, v0, m, period / steps, 1.0, 0.0, steps)[0], x0) / \
        ho.orbit_error(ref["x"], x0)
    factor = err_shared / err_block
    print(f"e=0.9 orbit: block {err_block:.3e} shared {err_shared:.3e} factor {factor:.1f} (fp64 {oracle_factor:.1f})")
    assert factor >= 10 and factor >= oracle_factor, (factor, oracle_factor, err_block, err_shared)

    fine, err_fine = _orbit_block(0.01)
    shared = _sim("HermiteSimulator", x0, v0, m, softening=0.0, dt=period / 1024, calc_energy=False)
    for _ in range(1024):
        shared.step()
    err_1024 = ho.orbit_error(_np(shared.positions), x0.astype(np.float32))
    assert 4 * 1024 >= fine.pair_interactions and err_1024 < 0.1           # the shared orbit is kept
    print(f"e=0.9 orbit: block eta=0.01 {err_fine:.3e} at {fine.pair_interactions} pairs, shared 1024 steps "
          f"{err_1024:.3e}, factor {err_1024 / err_fine:.0f}")
    assert err_1024 / err_fine >= 10, (err_fine, err_1024)


@pytest.mark.parametrize("calc_energy", [True, False])
def test_run_is_bit_identical_to_eager_steps_and_deterministic(calc_energy, gpu_device):
    x, v, m = bo.planted_binary_sphere(300, 5)
    kw = dict(softening=0.01, dt=DT, calc_energy=calc_energy, max_level=8)
    ran = _sim("BlockHermiteSimulator", x, v, m, **kw)
    assert not ran._graph_run_ok(12)
    states = ran.run(12)
    again = _sim("BlockHermiteSimulator", x, v, m, **kw).run(12)
    eager = _sim("BlockHermiteSimulator", x, v, m, **kw)
    assert len(states) == 12
    for k, (st, st2) in enumerate(zip(states, again)):
        eager.step()
        assert st.step == k
        for f in ("positions", "velocities", "accelerations"):
            assert torch.equal(getattr(st, f), getattr(eager, f).cpu()), (k, f)
            assert torch.equal(getattr(st, f), getattr(st2, f)), (k, f)
        if calc_energy:
            assert (st.u_energy, st.k_energy) == eager.compute_energies(), k
            assert (st.u_energy, st.k_energy) == (st2.u_energy, st2.k_energy)
        else:
            assert st.u_energy is None and st.k_energy is None
    assert torch.equal(ran.jerks, eager.jerks) and torch.equal(ran.levels, eager.levels)
    assert (ran.block_steps, ran.pair_interactions, ran.clamped) == (eager.block_steps, eager.pair_interactions,
                                                                     eager.clamped)
    with pytest.raises(ValueError):
        _sim("BlockHermiteSimulator", x, v, m, process_group=object())


def test_changing_dt_re_derives_the_levels(gpu_device):
    x, v, m = bo.planted_binary_sphere(200, 7)
    K = 8
    sim = _sim("BlockHermiteSimulator", x, v, m, softening=0.01, dt=DT, calc_energy=False, max_level=K)
    sim.run(2)
    before = _np(sim.levels).copy()
    sim.dt = 8 * DT
    a, j = _f64(_np(sim.accelerations)), _f64(_np(sim.jerks))
    crit = 0.5 * sim.eta * np.linalg.norm(a, axis=1) / np.linalg.norm(j, axis=1)
    expect = np.minimum([bo.wanted_level(c, sim.dt, K) for c in crit], K)
    assert not np.array_equal(expect, before)
    sim.level_history = []
    sim.run(1)
    first = sim.level_history[0].numpy()
    inactive = expect < expect.max()                          # the first block step moves the deepest level only
    assert inactive.any() and np.array_equal(first[inactive], expect[inactive])
    assert sim._leveled_for == (8 * DT, sim.eta, K)


def test_a_lone_body_takes_one_block_step_per_interval(gpu_device):
    """n = 1: a = j = 0, the criterion allows any step (+inf, not 0/0): level 0, nothing clamped, one block step per
    output step, and the free drift x + v t."""
    sim = _sim("BlockHermiteSimulator", [[0.3, 0.1, 0.0]], [[0.0, 0.25, 0.0]], [1.0], softening=0.0, dt=0.125,
               calc_energy=False, max_level=6)
    states = sim.run(3)
    assert sim.block_steps == 3 and sim.clamped == 0 and sim.pair_interactions == 3
    assert _np(sim.levels).tolist() == [0]
    assert np.allclose(states[-1].positions.numpy(), [[0.3, 0.1 + 3 * 0.125 * 0.25, 0.0]], rtol=0, atol=1e-6)


def test_coincident_bodies_finish_the_interval(gpu_device):
    """Two coincident bodies at eps = 0: the force is NaN, the criterion is NaN, the level is clamped to max_level and
    counted; the interval still ends within its 2^max_level block steps (the NaN spreads to the whole system after one
    evaluation, as in the other paths)."""
    rng = np.random.default_rng(2)
    x = rng.normal(size=(20, 3))
    x[5] = x[4]
    v = 0.1 * rng.normal(size=(20, 3))
    m = np.full(20, 1.0 / 20)
    sim = _sim("BlockHermiteSimulator", x, v, m, softening=0.0, dt=0.01, calc_energy=False, max_level=4)
    sim.step()
    assert sim.block_steps <= 16 and sim.clamped > 0
    sim.step()
    assert sim.block_steps <= 32


def test_dataset_cli_hermite_block_writes_the_rows_of_a_direct_run(tmp_path, gpu_device):
    from galaxify import simulation
    spec = importlib.util.spec_from_file_location("s01_hblock_gpu", os.path.join(PKG, "s01-dataset-generation.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    argv = ["--integrator", "hermite-block", "--n-bodies", "5", "8", "--sim-type", "spiral", "--steps", "6",
            "--seed", "42", "--device", "cuda"]
    out = tmp_path / "cli.csv"
    cli.main([*argv, "--output", str(out)])
    args = cli.build_parser().parse_args([*argv, "--output", "unused"])
    ref = tmp_path / "direct.csv"
    with open(ref, "wb") as f:
        f.write((",".join(cli.FIELDNAMES) + "\r\n").encode())
        for scene_id, n in enumerate((5, 8)):
            c = dict(vars(args), n_bodies=n, sim_type="spiral")
            pos, vel, masses = cli.initial_conditions(c)
            sim = simulation.BlockHermiteSimulator(positions=pos, velocities=vel, masses=masses, g_const=c["g"],
                                                   softening=c["softening"], dt=c["dt"], calc_energy=True,
                                                   device="cuda")
            cli.write_states(f, scene_id, "spiral", sim.run(c["steps"]), masses)
    got = list(csv.DictReader(open(out, newline="").read().splitlines()))
    want = list(csv.DictReader(open(ref, newline="").read().splitlines()))
    assert len(got) == len(want) == (5 + 8) * 6
    for a, b in zip(got, want):
        a.pop("step_time"); b.pop("step_time")
        assert a == b
