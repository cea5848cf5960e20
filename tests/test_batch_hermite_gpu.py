"""BatchedSimulator(integrator="hermite") on the MI355X (csrc/direct_batch_hermite.hip): every scene's positions,
velocities, accelerations and jerks are bit-identical to a HermiteSimulator of that scene alone, at construction and
after every step, on the masked and the un-masked path, alone / with companions / at any position; 10 steps against
the fp64 oracle; 4th-order convergence; captured run() == eager steps; empty and one-body scenes; NaN isolation at
softening 0; per-scene energies; the integrator cannot switch into or out of Hermite."""
import numpy as np
import pytest
import torch

import hermite_oracle as ho
from conftest import golden_cases, load_golden, row_rel

pytestmark = pytest.mark.gpu

TOL = 1e-5          # as test_hermite_steps_match_f64_oracle


def _np(t):
    return t.detach().cpu().numpy()


def _f32(x):
    return float(np.float32(x))


def _batch(scenes, calc_energy=True, integrator="hermite"):
    from galaxify import simulation
    return simulation.BatchedSimulator(systems=[(s["pos"], s["vel"], s["mass"]) for s in scenes], integrator=integrator,
                                       g_const=[s["g"] for s in scenes], softening=[s["eps"] for s in scenes],
                                       dt=[s["dt"] for s in scenes], calc_energy=calc_energy, device="cuda")


def _lone(s, calc_energy=True):
    from galaxify import simulation
    return simulation.HermiteSimulator(positions=s["pos"], velocities=s["vel"], masses=s["mass"], g_const=s["g"],
                                       softening=s["eps"], dt=s["dt"], calc_energy=calc_energy, device="cuda")


def _golden_scenes():
    out = []
    for name in golden_cases():
        g = load_golden(name)
        out.append(dict(name=name, pos=g["pos"], vel=g["vel"], mass=g["mass"], g=float(g["g_const"]),
                        eps=float(g["softening"]), dt=float(g["dt"])))
    return out


def _plummer(n, seed, g=1.0, eps=0.1, dt=0.01):
    from nbd.plummer import generate_plummer
    p, v, m = generate_plummer(n, seed=seed)
    return dict(pos=p, vel=v, mass=m, g=g, eps=eps, dt=dt)


def _spiral(n, seed):
    from galaxify import galaxies
    p, v, m = galaxies.generate_spiral(n_bodies=n, total_mass=1.0, radial_scale=3.0, height_scale=0.3, g_const=4.5e-6,
                                       black_hole_mass=0.01, seed=seed)
    return dict(pos=p, vel=v, mass=m, g=4.5e-6, eps=0.05, dt=1e-4)


def _rows(sim, i):
    lo, hi = int(sim.offsets[i]), int(sim.offsets[i + 1])
    return (sim.positions[lo:hi], sim.velocities[lo:hi], sim.accelerations[lo:hi], sim.jerks[lo:hi])


def _state(sim):
    return (sim.positions, sim.velocities, sim.accelerations, sim.jerks)


def _assert_equal(batch, i, lone, what):
    for nm, x, y in zip(("pos", "vel", "acc", "jerk"), _rows(batch, i), _state(lone)):
        assert torch.equal(x, y), (what, i, nm, float((x - y).abs().max()))


def test_all_goldens_bit_identical_to_lone_hermite(gpu_device):
    sc = _golden_scenes()
    names = [s["name"] for s in sc]
    assert "direct_plummer_n64_eps0" in names and "direct_plummer_n300_ragged_mass" in names
    assert len({(s["g"], s["eps"], s["dt"]) for s in sc}) >= 3
    sim = _batch(sc)
    lones = [_lone(s) for s in sc]
    assert sim.jerks is not None and tuple(sim.jerks.shape) == (sim.n, 3)
    for i, lone in enumerate(lones):
        _assert_equal(sim, i, lone, "construction")
    for k in range(10):
        sim.step()
        for lone in lones:
            lone.step()
        if k in (0, 9):
            for i, lone in enumerate(lones):
                _assert_equal(sim, i, lone, f"step {k + 1}")
    assert len(sim.scene(0)) == 3


def test_scene_is_bit_identical_alone_and_with_any_companions(gpu_device):
    target = _plummer(300, 7, eps=0.05, dt=2e-3)
    masked = _plummer(129, 5, eps=0.0, dt=1e-3)

    def run(scenes, idx):
        sim = _batch(scenes)
        for _ in range(12):
            sim.step()
        return [t.clone() for t in _rows(sim, idx)]
    alone = run([target], 0)
    with_a = run([_plummer(64, 1), target, _spiral(2000, 3)], 1)
    with_b = run([_plummer(5000, 2), _spiral(3, 4), masked, target], 3)
    again = run([target], 0)
    for other in (with_a, with_b, again):
        for x, y in zip(alone, other):
            assert torch.equal(x, y)
    m_alone = run([masked], 0)
    m_with = run([target, _spiral(25, 9), masked], 2)
    for x, y in zip(m_alone, m_with):
        assert torch.equal(x, y)


def test_ten_steps_match_f64_oracle(gpu_device):
    sc = [s for s in _golden_scenes() if "4096" not in s["name"]]
    sim = _batch(sc)
    for i, s in enumerate(sc):
        x = s["pos"].astype(np.float32).astype(np.float64)
        v = s["vel"].astype(np.float32).astype(np.float64)
        m = s["mass"].astype(np.float32).astype(np.float64)
        s["ora"] = [x, v, m, *ho.accel_jerk(x, v, m, _f32(s["g"]), _f32(s["eps"] ** 2))]
        pos, vel, acc, jerk = (_np(t) for t in _rows(sim, i))
        assert row_rel(acc, s["ora"][3]) < TOL and row_rel(jerk, s["ora"][4]) < TOL, s["name"]
    for k in range(10):
        sim.step()
        for i, s in enumerate(sc):
            x, v, m, a, j = s["ora"]
            x, v, a, j = ho.hermite_step(x, v, a, j, m, s["dt"], _f32(s["g"]), _f32(s["eps"] ** 2))
            s["ora"] = [x, v, m, a, j]
            if k == 0:
                pos, vel, _, _ = (_np(t) for t in _rows(sim, i))
                assert row_rel(pos, x) < TOL and row_rel(vel, v) < TOL, s["name"]
    for i, s in enumerate(sc):
        x, v, _, a, _ = s["ora"]
        pos, vel, acc, _ = (_np(t) for t in _rows(sim, i))
        assert row_rel(pos, x) < 10 * TOL and row_rel(vel, v) < 10 * TOL and row_rel(acc, a) < 10 * TOL, s["name"]


def test_fourth_order_convergence_in_one_batch(gpu_device):
    """The e = 0.5 two-body orbit (eps = 0, masked path) and a softened Plummer sphere (un-masked path) in one batch,
    with the step counts and ratios of test_hermite_gpu.py."""
    from nbd.plummer import generate_plummer
    x0, v0, m2, period = ho.two_body(0.5)
    p, v, m = (np.asarray(t, np.float32) for t in generate_plummer(256, seed=5))
    eps = 0.05
    ref, _, _, _ = ho.hermite_run(p.astype(np.float64), v.astype(np.float64), m.astype(np.float64), 1.0 / 256, 1.0,
                                  _f32(eps ** 2), 256)
    orbit, plum = {}, {}
    for k_orb, k_pl in ((64, 16), (128, 32), (256, None)):
        scenes = [dict(pos=x0, vel=v0, mass=m2, g=1.0, eps=0.0, dt=period / k_orb)]
        if k_pl:
            scenes.append(dict(pos=p, vel=v, mass=m, g=1.0, eps=eps, dt=1.0 / k_pl))
        sim = _batch(scenes, calc_energy=False)
        for s in range(k_orb):
            if k_pl and s == k_pl:
                plum[k_pl] = float(np.linalg.norm(_np(_rows(sim, 1)[0]) - ref, axis=1).max())
            sim.step()
        orbit[k_orb] = ho.orbit_error(_np(_rows(sim, 0)[0]), x0.astype(np.float32))
    assert orbit[64] / orbit[128] >= 12 and orbit[128] / orbit[256] >= 10, orbit
    assert plum[16] / plum[32] >= 12 and plum[32] < 3e-4, plum


@pytest.mark.parametrize("calc_energy", [True, False])
def test_captured_run_equals_eager_steps(calc_energy, gpu_device):
    """43 steps: captured chunks of 32 and 8, then an eager tail of 3."""
    scenes = [_plummer(100, 11, eps=0.05, dt=1e-3), _spiral(25, 2), _plummer(64, 3, eps=0.0, dt=1e-3),
              _plummer(2000, 4, eps=0.05, dt=5e-4)]
    ran = _batch(scenes, calc_energy=calc_energy)
    eager = _batch(scenes, calc_energy=calc_energy)
    assert ran._chunk_len() >= 8
    old_acc = ran.accelerations
    old_acc_copy = old_acc.clone()
    out = ran.run(43)
    assert len(out) == len(scenes) and all(len(o) == 43 for o in out)
    for k in range(43):
        eager.step()
        if calc_energy:
            us, ks = eager.compute_energies()
        for i in range(len(scenes)):
            st = out[i][k]
            pos, vel, acc = eager.scene(i)
            assert st.step == k
            assert torch.equal(st.positions, pos.cpu()) and torch.equal(st.velocities, vel.cpu()), (k, i)
            assert torch.equal(st.accelerations, acc.cpu()), (k, i)
            if calc_energy:
                assert (st.u_energy, st.k_energy) == (us[i], ks[i]), (k, i)
            else:
                assert st.u_energy is None and st.k_energy is None
    for x, y in zip(_state(ran), _state(eager)):
        assert torch.equal(x, y)
    assert torch.equal(old_acc, old_acc_copy)           # the caller's handle on the old accelerations is untouched


def test_empty_and_one_body_scenes(gpu_device):
    one = dict(pos=np.array([[0.5, -1.0, 2.0]]), vel=np.array([[0.1, 0.2, -0.3]]), mass=np.array([2.0]), g=1.0,
               eps=0.0, dt=0.01)
    empty = dict(pos=np.zeros((0, 3)), vel=np.zeros((0, 3)), mass=np.zeros(0), g=1.0, eps=0.1, dt=0.01)
    other = _plummer(70, 8, eps=0.05, dt=1e-3)
    sim = _batch([empty, one, other, empty])
    lone = _lone(other)
    for k in range(3):
        _, _, a, j = _rows(sim, 1)
        assert torch.equal(a, torch.zeros_like(a)) and torch.equal(j, torch.zeros_like(j)), k
        _assert_equal(sim, 2, lone, k)
        sim.step(); lone.step()
    x = _np(_rows(sim, 1)[0])[0]
    assert np.allclose(x, np.float32(one["pos"][0]) + 3 * np.float32(0.01) * np.float32(one["vel"][0]), rtol=1e-6)
    us, ks = sim.compute_energies()
    assert us[0] == 0.0 and ks[0] == 0.0 and us[3] == 0.0 and us[1] == 0.0
    only_empty = _batch([empty, empty])
    assert tuple(only_empty.jerks.shape) == (0, 3)
    only_empty.step()
    assert len(only_empty.run(9)[1]) == 9


def test_coincident_bodies_at_eps0_poison_their_scene_only(gpu_device):
    bad = dict(pos=np.array([[0., 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0]]), vel=np.zeros((4, 3)), mass=np.ones(4),
               g=1.0, eps=0.0, dt=0.01)
    others = [_spiral(25, 1), _plummer(64, 2, eps=0.0, dt=1e-3), _plummer(300, 3)]
    with_bad = _batch([others[0], bad, others[1], others[2]])
    without = _batch(others)
    _, _, acc, jerk = (_np(t) for t in _rows(with_bad, 1))
    assert np.isnan(acc[1]).any() and np.isnan(acc[2]).any() and np.isnan(jerk[1]).any()
    assert np.isfinite(acc[0]).all() and np.isfinite(acc[3]).all()
    for _ in range(3):
        with_bad.step(); without.step()
    for j, i in enumerate((0, 2, 3)):
        for x, y in zip(_rows(with_bad, i), _rows(without, j)):
            assert torch.isfinite(x).all() and torch.equal(x, y)


def test_energies_match_lone_hermite(gpu_device):
    sc = [s for s in _golden_scenes() if "4096" not in s["name"]]
    sim = _batch(sc)
    lones = [_lone(s) for s in sc]
    for _ in range(5):
        sim.step()
        for lone in lones:
            lone.step()
    us, ks = sim.compute_energies()
    for i, lone in enumerate(lones):
        u, k = lone.compute_energies()
        assert abs(us[i] - u) <= 2e-5 * abs(u) + 1e-30 and abs(ks[i] - k) <= 2e-5 * abs(k) + 1e-30, sc[i]["name"]


def test_integrator_cannot_switch_into_or_out_of_hermite(gpu_device):
    from galaxify import simulation
    scenes = [_plummer(40, 1), _plummer(70, 2)]
    with pytest.raises(ValueError):
        _batch(scenes, integrator="hermite-block")
    with pytest.raises(ValueError):
        _batch(scenes, integrator="rk4")
    h = _batch(scenes)
    h.integrator = "leapfrog"
    with pytest.raises(ValueError):
        h.step()
    with pytest.raises(ValueError):
        h.run(10)
    h.integrator = "hermite"
    h.step()
    lf = _batch(scenes, integrator="leapfrog")
    assert lf.jerks is None
    lf.integrator = "euler"
    lf.step()
    lf.integrator = "hermite"
    with pytest.raises(ValueError):
        lf.step()
    with pytest.raises(ValueError):
        lf.run(10)
    assert isinstance(h, simulation.BatchedSimulator)
