"""HermiteSimulator and the nbd_accel_jerk_f32 / nbd_hermite_step_f32 kernels on the MI355X against the fp64 restatement
in hermite_oracle.py: the force and jerk of every golden initial state, 1 and 10 steps, 4th-order convergence on an
eccentric two-body orbit (masked path) and on a softened Plummer sphere, captured run() against eager steps, momentum,
determinism and the dataset CLI."""
import csv
import importlib.util
import os

import numpy as np
import pytest
import torch

import hermite_oracle as ho
from conftest import PKG, golden_cases, load_golden, row_rel

pytestmark = pytest.mark.gpu

TOL = 1e-5          # per-particle relative (north_star), as tests/test_direct_gpu.py


def _np(t):
    return t.detach().cpu().numpy()


def _f32(x):
    return float(np.float32(x))


def _golden_sim(g, cls="HermiteSimulator", **over):
    from galaxify import simulation
    kw = dict(positions=g["pos"], velocities=g["vel"], masses=g["mass"], g_const=float(g["g_const"]),
              softening=float(g["softening"]), dt=float(g["dt"]), calc_energy=True, device="cuda")
    kw.update(over)
    return getattr(simulation, cls)(**kw)


def _oracle_args(g):
    """The fp32 state and constants the simulator works from, in fp64."""
    return (g["pos"].astype(np.float32).astype(np.float64), g["vel"].astype(np.float32).astype(np.float64),
            g["mass"].astype(np.float32).astype(np.float64), _f32(g["g_const"]), _f32(float(g["softening"]) ** 2))


@pytest.mark.parametrize("name", golden_cases())
def test_accel_jerk_golden_initial_states(name, gpu_device):
    from nbd import direct
    g = load_golden(name)
    n = g["pos"].shape[0]
    pos = torch.tensor(g["pos"], dtype=torch.float32, device=gpu_device)
    vel = torch.tensor(g["vel"], dtype=torch.float32, device=gpu_device)
    mass = torch.tensor(g["mass"], dtype=torch.float32, device=gpu_device)
    posm, velp = direct.alloc_posm(n, gpu_device), direct.alloc_posm(n, gpu_device)
    direct.hermite_pack(pos, vel, mass, posm, velp)
    x, v, m, gc, eps2 = _oracle_args(g)
    a_ref, j_ref = ho.accel_jerk(x, v, m, gc, eps2)
    for variant in (0, 1):
        acc, jerk = direct.accel_jerk(posm, velp, n, _f32(float(g["softening"]) ** 2), gc, variant=variant)
        acc, jerk = _np(acc), _np(jerk)
        assert np.isfinite(acc).all() and np.isfinite(jerk).all()
        assert row_rel(acc, g["acc0"]) < TOL, variant
        assert row_rel(jerk, j_ref) < TOL, (variant, row_rel(jerk, j_ref))


@pytest.mark.parametrize("name", [n for n in golden_cases() if "4096" not in n])
def test_hermite_steps_match_f64_oracle(name, gpu_device):
    g = load_golden(name)
    sim = _golden_sim(g)
    x, v, m, gc, eps2 = _oracle_args(g)
    dt = float(g["dt"])
    a, j = ho.accel_jerk(x, v, m, gc, eps2)
    assert row_rel(_np(sim.accelerations), a) < TOL and row_rel(_np(sim.jerks), j) < TOL
    for k in range(10):
        sim.step()
        x, v, a, j = ho.hermite_step(x, v, a, j, m, dt, gc, eps2)
        if k == 0:
            assert row_rel(_np(sim.positions), x) < TOL and row_rel(_np(sim.velocities), v) < TOL
    assert row_rel(_np(sim.positions), x) < 10 * TOL and row_rel(_np(sim.velocities), v) < 10 * TOL
    assert row_rel(_np(sim.accelerations), a) < 10 * TOL


def _orbit(cls, steps, e=0.5):
    from galaxify import simulation
    x0, v0, m, period = ho.two_body(e)
    sim = getattr(simulation, cls)(positions=x0, velocities=v0, masses=m, g_const=1.0, softening=0.0,
                                   dt=period / steps, calc_energy=False, device="cuda")
    for _ in range(steps):
        sim.step()
    return ho.orbit_error(_np(sim.positions), x0.astype(np.float32))


def test_two_body_orbit_converges_at_fourth_order(gpu_device):
    """e = 0.5, eps = 0 (the index-masked path), one period. fp64 oracle: 5.1e-3, 2.6e-4, 1.4e-5."""
    e64, e128, e256 = (_orbit("HermiteSimulator", k) for k in (64, 128, 256))
    assert e64 / e128 >= 12 and e128 / e256 >= 10, (e64, e128, e256)
    assert e128 < _orbit("LeapFrogSimulator", 512), e128


def test_plummer_converges_at_fourth_order(gpu_device):
    """Softened Plummer N = 256 (un-masked path) over one time unit at dt = 1/16 and 1/32 against the fp64 oracle at
    dt = 1/256."""
    from galaxify import simulation
    from nbd.plummer import generate_plummer
    p, v, m = (np.asarray(t, np.float32) for t in generate_plummer(256, seed=5))
    eps = 0.05
    x, _, _, _ = ho.hermite_run(p.astype(np.float64), v.astype(np.float64), m.astype(np.float64), 1.0 / 256, 1.0,
                                _f32(eps ** 2), 256)
    errs = []
    for k in (16, 32):
        sim = simulation.HermiteSimulator(positions=p, velocities=v, masses=m, softening=eps, dt=1.0 / k,
                                          calc_energy=False, device="cuda")
        for _ in range(k):
            sim.step()
        errs.append(float(np.linalg.norm(_np(sim.positions) - x, axis=1).max()))
    assert errs[0] / errs[1] >= 12 and errs[1] < 3e-4, errs


@pytest.mark.parametrize("n", [100, 2000])
@pytest.mark.parametrize("calc_energy", [True, False])
def test_run_is_bit_identical_to_eager_steps(n, calc_energy, gpu_device):
    """43 steps: captured chunks of 32 and 8, then an eager tail of 3."""
    from galaxify import simulation
    from nbd.plummer import generate_plummer
    p, v, m = generate_plummer(n, seed=11)
    kw = dict(positions=p, velocities=v, masses=m, softening=0.05, dt=1e-3, calc_energy=calc_energy, device="cuda")
    ran = simulation.HermiteSimulator(**kw)
    assert ran._graph_run_ok(43)
    states = ran.run(43)
    eager = simulation.HermiteSimulator(**kw)
    assert len(states) == 43
    for k, st in enumerate(states):
        eager.step()
        assert st.step == k
        assert torch.equal(st.positions, eager.positions.cpu()), k
        assert torch.equal(st.velocities, eager.velocities.cpu()), k
        assert torch.equal(st.accelerations, eager.accelerations.cpu()), k
        if calc_energy:
            assert (st.u_energy, st.k_energy) == eager.compute_energies(), k
        else:
            assert st.u_energy is None and st.k_energy is None
    assert torch.equal(ran.jerks, eager.jerks) and torch.equal(ran.accelerations, eager.accelerations)
    assert torch.equal(ran.positions, eager.positions)


def test_momentum_and_determinism(gpu_device):
    from galaxify import simulation
    g = load_golden("direct_plummer_n300_ragged_mass")
    runs = []
    for _ in range(2):
        sim = _golden_sim(g)
        m = sim.masses[:, None].double()
        for t in (sim.accelerations, sim.jerks):
            scale = (m * t.double().abs()).sum(0).max()
            assert (m * t.double()).sum(0).abs().max() <= 1e-6 * scale
        for _ in range(5):
            sim.step()
        runs.append([t.clone() for t in (sim.positions, sim.velocities, sim.accelerations, sim.jerks)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        simulation.HermiteSimulator(positions=g["pos"], velocities=g["vel"], masses=g["mass"], device="cuda",
                                    process_group=object())
    assert sim._uniform is None


def test_dataset_cli_hermite_writes_the_rows_of_a_direct_run(tmp_path, gpu_device):
    from galaxify import simulation
    spec = importlib.util.spec_from_file_location("s01_hermite_gpu", os.path.join(PKG, "s01-dataset-generation.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    argv = ["--integrator", "hermite", "--n-bodies", "5", "8", "--sim-type", "spiral", "--steps", "12", "--seed", "42",
            "--device", "cuda"]
    out = tmp_path / "cli.csv"
    cli.main([*argv, "--output", str(out)])
    args = cli.build_parser().parse_args([*argv, "--output", "unused"])
    ref = tmp_path / "direct.csv"
    with open(ref, "wb") as f:
        f.write((",".join(cli.FIELDNAMES) + "\r\n").encode())
        for scene_id, n in enumerate((5, 8)):
            c = dict(vars(args), n_bodies=n, sim_type="spiral")
            pos, vel, masses = cli.initial_conditions(c)
            sim = simulation.HermiteSimulator(positions=pos, velocities=vel, masses=masses, g_const=c["g"],
                                              softening=c["softening"], dt=c["dt"], calc_energy=True, device="cuda")
            cli.write_states(f, scene_id, "spiral", sim.run(c["steps"]), masses)
    got = list(csv.DictReader(open(out, newline="").read().splitlines()))
    want = list(csv.DictReader(open(ref, newline="").read().splitlines()))
    assert len(got) == len(want) == (5 + 8) * 12
    for a, b in zip(got, want):
        a.pop("step_time"); b.pop("step_time")                 # a GPU timing
        assert a == b
