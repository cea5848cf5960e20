"""galaxify.simulation.BatchedSimulator on the MI355X: many independent scenes advanced by one set of launches
(csrc/direct_batch.hip). Every golden scene inside ONE batch against its own reference vectors, bit-identical results
alone / with companions / at any position / run to run, captured run() == eager steps, rows against the fp64 C oracle,
NaN isolation at softening 0, and the dataset CLI's --batch-scenes path against the reference CSV."""
import numpy as np
import pytest
import torch

from conftest import global_rel, golden_cases, load_golden, row_rel

pytestmark = pytest.mark.gpu

TOL = 1e-5
TOL_ACC_GLOBAL = 1e-6


def _np(t):
    return t.detach().cpu().numpy()


def _batch(scenes, integrator="leapfrog", calc_energy=True, **kw):
    from galaxify import simulation
    args = dict(g_const=[s.get("g", 1.0) for s in scenes], softening=[s.get("eps", 0.1) for s in scenes],
                dt=[s.get("dt", 0.01) for s in scenes])
    args.update(kw)
    return simulation.BatchedSimulator(systems=[(s["pos"], s["vel"], s["mass"]) for s in scenes], integrator=integrator,
                                       calc_energy=calc_energy, device="cuda", **args)


def _golden_scenes():
    out = []
    for name in golden_cases():
        g = load_golden(name)
        out.append(dict(name=name, gold=g, pos=g["pos"], vel=g["vel"], mass=g["mass"], g=float(g["g_const"]),
                        eps=float(g["softening"]), dt=float(g["dt"])))
    return out


def test_all_goldens_in_one_leapfrog_batch(gpu_device):
    sc = _golden_scenes()
    assert len(sc) == 12 and len({(s["g"], s["eps"], s["dt"]) for s in sc}) == 3
    sim = _batch(sc)
    for i, s in enumerate(sc):
        gd = s["gold"]
        acc = _np(sim.scene(i)[2])
        assert np.isfinite(acc).all()
        assert row_rel(acc, gd["acc0"]) < TOL and global_rel(acc, gd["acc0"]) < TOL_ACC_GLOBAL, s["name"]
    us, ks = sim.compute_energies()
    for i, s in enumerate(sc):
        u0, k0 = s["gold"]["energy0"]
        assert abs(us[i] - u0) <= 2e-5 * abs(u0) + 1e-30 and abs(ks[i] - k0) <= 2e-6 * abs(k0) + 1e-30, s["name"]
    sim.step()
    for i, s in enumerate(sc):
        for key, t in zip(("pos", "vel", "acc"), sim.scene(i)):
            assert row_rel(_np(t), s["gold"][f"lf1_{key}"]) < TOL, (s["name"], key)
    for _ in range(9):
        sim.step()
    for i, s in enumerate(sc):
        if "lf10_pos" not in s["gold"] or "4096" in s["name"]:
            continue
        for key, t in zip(("pos", "vel", "acc"), sim.scene(i)):
            assert row_rel(_np(t), s["gold"][f"lf10_{key}"]) < 10 * TOL, (s["name"], key)


def test_all_goldens_in_one_euler_batch(gpu_device):
    sc = _golden_scenes()
    sim = _batch(sc, integrator="euler")
    sim.step()
    for i, s in enumerate(sc):
        for key, t in zip(("pos", "vel", "acc"), sim.scene(i)):
            assert row_rel(_np(t), s["gold"][f"eu1_{key}"]) < TOL, (s["name"], key)


def _spiral(n, seed):
    from galaxify import galaxies
    p, v, m = galaxies.generate_spiral(n_bodies=n, total_mass=1.0, radial_scale=3.0, height_scale=0.3, g_const=4.5e-6,
                                       black_hole_mass=0.01, seed=seed)
    return dict(pos=p, vel=v, mass=m, g=4.5e-6, eps=0.05, dt=1e-4)


def _plummer(n, seed, g=1.0, eps=0.1, dt=0.01):
    from nbd.plummer import generate_plummer
    p, v, m = generate_plummer(n, seed=seed)
    return dict(pos=p, vel=v, mass=m, g=g, eps=eps, dt=dt)


def _advance(scenes, steps, integrator="leapfrog"):
    sim = _batch(scenes, integrator=integrator)
    for _ in range(steps):
        sim.step()
    us, ks = sim.compute_energies()
    return [tuple(t.clone() for t in sim.scene(i)) + (us[i], ks[i]) for i in range(len(scenes))]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:]


@pytest.mark.parametrize("integrator", ["leapfrog", "euler"])
def test_scene_is_bit_identical_alone_and_with_any_companions(integrator, gpu_device):
    target = _spiral(300, 7)
    alone = _advance([target], 20, integrator)[0]
    with_a = _advance([_plummer(64, 1), target, _spiral(2000, 3)], 20, integrator)[1]
    with_b = _advance([_plummer(5000, 2), _spiral(3, 4), _plummer(129, 5, eps=0.0, dt=1e-3), target], 20, integrator)[3]
    again = _advance([target], 20, integrator)[0]
    assert _same(alone, with_a) and _same(alone, with_b) and _same(alone, again)
    assert np.isfinite(_np(alone[0])).all()


@pytest.mark.parametrize("integrator,energy", [("leapfrog", True), ("leapfrog", False), ("euler", True),
                                               ("euler", False)])
def test_captured_run_equals_eager_steps(integrator, energy, gpu_device):
    scenes = [_spiral(100, 1), _plummer(64, 2), _spiral(500, 3), dict(pos=np.zeros((0, 3)), vel=np.zeros((0, 3)),
                                                                        mass=np.zeros(0)), _plummer(1, 4)]
    a = _batch(scenes, integrator=integrator, calc_energy=energy)
    b = _batch(scenes, integrator=integrator, calc_energy=energy)
    acc_before = a.accelerations
    acc_copy = acc_before.clone()
    ra = a.run(45)                                          # 32 + 8 captured, a tail of 5 eager
    assert len(ra) == len(scenes) and all(len(r) == 45 for r in ra)
    for s_ in range(45):
        b.step()
        ub, kb = b.compute_energies() if energy else (None, None)
        for i in range(len(scenes)):
            st = ra[i][s_]
            assert st.step == s_ and st.step_time > 0
            for x, y in zip((st.positions, st.velocities, st.accelerations), b.scene(i)):
                assert torch.equal(x, y.cpu()), (s_, i)
            if energy:
                assert (st.u_energy, st.k_energy) == (ub[i], kb[i]), (s_, i)
            else:
                assert st.u_energy is None and st.k_energy is None
    assert ra[3][0].positions.shape == (0, 3)
    for key in ("positions", "velocities", "accelerations"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    assert torch.equal(acc_before, acc_copy) and a.accelerations.data_ptr() != acc_before.data_ptr()
    # a changed dt captures afresh instead of replaying the old graph
    n_graphs = len(a._run_graphs)
    a.dt = [2e-4, 5e-3, 1e-4, 1e-4, 0.02]; b.dt = list(a.dt)
    ra2 = a.run(10)
    assert len(a._run_graphs) > n_graphs
    for _ in range(10):
        b.step()
    for i in range(len(scenes)):
        assert torch.equal(ra2[i][-1].positions, b.scene(i)[0].cpu()) and torch.equal(ra2[i][-1].velocities,
                                                                                      b.scene(i)[1].cpu())


def test_ragged_batch_against_fp64_c_oracle(gpu_device):
    from oracle import c_oracle
    from nbd.plummer import generate_plummer
    sizes = [1, 2, 63, 64, 65, 127, 129, 4097]
    rng = np.random.default_rng(17)
    scenes = []
    for k, n in enumerate(sizes):
        p, v, m = generate_plummer(n, seed=200 + n)
        m = m * rng.uniform(0.5, 2.0, n)
        scenes.append(dict(pos=p, vel=v, mass=m, g=[1.0, 4.5e-6][k % 2], eps=[0.1, 0.05, 1e-3][k % 3], dt=0.01))
    sim = _batch(scenes)
    for i, s in enumerate(scenes):
        got = _np(sim.scene(i)[2]).astype(np.float64)
        ref = c_oracle.acc_f64(s["pos"], s["mass"], s["g"], s["eps"])
        scale = np.linalg.norm(ref, axis=1).max() if len(ref) else 0.0
        assert np.linalg.norm(got - ref, axis=1).max() <= 2e-6 * max(scale, 1e-30), (i, sizes[i])
        mf = np.asarray(s["mass"], dtype=np.float32).astype(np.float64)
        net = (mf[:, None] * got).sum(0)
        assert np.abs(net).max() <= 1e-5 * max((mf[:, None] * np.abs(got)).sum(0).max(), 1e-30), (i, net)


def test_coincident_bodies_at_eps0_poison_their_scene_only(gpu_device):
    bad = dict(pos=np.array([[0., 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0]]), vel=np.zeros((4, 3)), mass=np.ones(4),
               g=1.0, eps=0.0, dt=0.01)
    others = [_spiral(25, 1), _plummer(64, 2, eps=0.0, dt=1e-3), _plummer(300, 3)]
    with_bad = _batch([others[0], bad, others[1], others[2]])
    without = _batch(others)
    acc = _np(with_bad.scene(1)[2])
    assert np.isnan(acc[1]).any() and np.isnan(acc[2]).any()
    assert np.isfinite(acc[0]).all() and np.isfinite(acc[3]).all()
    for _ in range(3):
        with_bad.step(); without.step()
    for j, i in enumerate((0, 2, 3)):
        for x, y in zip(with_bad.scene(i), without.scene(j)):
            assert torch.isfinite(x).all() and torch.equal(x, y)
    ua, ka = with_bad.compute_energies()
    ub, kb = without.compute_energies()
    assert [ua[i] for i in (0, 2, 3)] == ub and [ka[i] for i in (0, 2, 3)] == kb


def test_dataset_cli_batch_scenes_reproduces_the_reference_csv(tmp_path, gpu_device):
    """--batch-scenes with the golden CLI arguments: the checks of test_dataset_cli_reproduces_the_reference_csv."""
    import csv
    import importlib.util
    import os
    import sys
    from conftest import PKG
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden_cli import ARGS
    spec = importlib.util.spec_from_file_location("s01", f"{PKG}/s01-dataset-generation.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    out = str(tmp_path / "out.csv")
    cli.main([*ARGS, "--device", "cuda", "--output", out, "--batch-scenes"])
    ref_raw = open(os.path.join(os.path.dirname(__file__), "golden", "ref_cli_spiral_n5_n8.csv"), newline="").read()
    got_raw = open(out, newline="").read()
    assert ref_raw.split("\r\n")[0] == got_raw.split("\r\n")[0] and ref_raw.endswith("\r\n") == got_raw.endswith("\r\n")
    ref = list(csv.DictReader(ref_raw.splitlines()))
    got = list(csv.DictReader(got_raw.splitlines()))
    assert len(ref) == len(got) == (5 + 8) * 3
    f32_cols = ["x", "y", "z", "vx", "vy", "vz", "ax", "ay", "az"]
    for a, b in zip(ref, got):
        assert (a["scene"], a["scene_type"], a["step"]) == (b["scene"], b["scene_type"], b["step"])
        assert a["mass"] == b["mass"]
        for c in f32_cols:
            x, y = float(a[c]), float(b[c])
            assert str(np.float32(y)) == b[c]
            assert abs(x - y) <= 1e-5 * max(abs(x), 1e-30) + 1e-12, (c, a[c], b[c])
        for c in ("u", "k"):
            assert abs(float(a[c]) - float(b[c])) <= 2e-5 * abs(float(a[c])), (c, a[c], b[c])
        assert float(b["step_time"]) >= 0.0


def test_cpu_device_raises_and_bad_shapes_raise(gpu_device):
    from galaxify import simulation
    s = _plummer(10, 1)
    with pytest.raises(RuntimeError):
        simulation.BatchedSimulator(systems=[(s["pos"], s["vel"], s["mass"])], device="cpu")
    with pytest.raises(ValueError):
        simulation.BatchedSimulator(systems=[(s["pos"], s["vel"], s["mass"][:5])], device="cuda")
    with pytest.raises(ValueError):
        simulation.BatchedSimulator(systems=[(s["pos"], s["vel"], s["mass"])] * 2, dt=[0.1, 0.2, 0.3], device="cuda")
