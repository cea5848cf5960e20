"""The tree force on the GPU (csrc/tree_force.hip, nbd/tree.py, TreeLeapFrogSimulator) against the fp64 restatement of
tests/tree_oracle.py fed the GPU's own body order, and against the fp64 direct sum. Inputs A-D and the softening are
tree_oracle.case's; every reference is computed once and shared."""
import numpy as np
import pytest
import torch

import tree_oracle as to
from conftest import row_rel

pytestmark = pytest.mark.gpu

CASES = ["A", "B", "C", "D"]
_refs = {}


def _np(t):
    return t.detach().cpu().numpy()


def _sim(name_or_arrays, theta, quadrupole=True, cls="TreeLeapFrogSimulator", softening=to.SOFTENING, **kw):
    from galaxify import simulation
    p, v, m = to.case(name_or_arrays) if isinstance(name_or_arrays, str) else name_or_arrays
    extra = dict(theta=theta, quadrupole=quadrupole) if cls == "TreeLeapFrogSimulator" else {}
    return getattr(simulation, cls)(positions=p, velocities=v, masses=m, g_const=1.0, softening=softening, dt=0.01,
                                    calc_energy=False, device="cuda", **extra, **kw)


def _direct(key, arrays=None):
    if ("direct", key) not in _refs:
        p, _, m = to.case(key) if arrays is None else arrays
        _refs[("direct", key)] = to.direct_accel(p, m, to.SOFTENING)
    return _refs[("direct", key)]


def _own_order_counters(key, theta, arrays=None):
    if ("own", key, theta) not in _refs:
        p, _, m = to.case(key) if arrays is None else arrays
        _refs[("own", key, theta)] = to.tree_accel(p, m, theta, to.SOFTENING)[1]
    return _refs[("own", key, theta)]


def _rms(e):
    return float(np.sqrt((e ** 2).mean())) if e.size else 0.0


def _same_tree_same_answer(key, arrays, theta, quadrupole):
    """The bars of 'same tree, same answer' for one simulator: rows and counters against the oracle on the GPU's order,
    errors against the fp64 direct sum no worse than twice the oracle's own."""
    sim = _sim(arrays, theta, quadrupole)
    acc, order, counters = _np(sim.accelerations), _np(sim.tree_order()), sim.tree_counters()
    p, _, m = arrays
    ref, ref_counters = to.tree_accel(p, m, theta, to.SOFTENING, quadrupole=quadrupole, order=order)
    rows = to.row_errors(acc, ref)
    direct = _direct(key, arrays)
    e_gpu, e_ref = to.row_errors(acc, direct), to.row_errors(ref, direct)
    print(f"{key} theta={theta} quad={quadrupole}: rows within 3e-6 of the oracle {np.mean(rows < 3e-6):.4f} (max "
          f"{rows.max():.2e}), counters {counters} vs {ref_counters}, vs direct max {e_gpu.max():.3e} (oracle "
          f"{e_ref.max():.3e}), rms {_rms(e_gpu):.3e} (oracle {_rms(e_ref):.3e})")
    assert np.isfinite(acc).all()
    assert np.mean(rows < 3e-6) >= 0.99
    for got, want in zip(counters, ref_counters):
        assert abs(got - want) <= 0.01 * want
    assert e_gpu.max() <= 2 * e_ref.max() + 3e-6 and _rms(e_gpu) <= 2 * _rms(e_ref) + 3e-6


@pytest.mark.parametrize("name", CASES)
def test_theta0_is_the_direct_sum(name, gpu_device):
    sim = _sim(name, 0.0)
    n = sim.n
    err = row_rel(_np(sim.accelerations), _direct(name))
    print(f"{name}: theta = 0 row_rel against the fp64 direct sum {err:.3e}")
    assert err < 3e-6
    assert sim.tree_counters() == (0, -(-n // 8) * -(-n // 64))


def test_theta0_at_a_deeper_split_level(gpu_device):
    """n = 40 000: 5 000 / 625 / 79 / 10 / 2 / 1 nodes per level, so the waves that share a group divide the tree two
    levels above the bodies' nodes (A-D divide it at level 0 or 1, 65 bodies and fewer use one wave). At theta = 0
    every level-0 node must be summed exactly once: the counter says so, and sampled rows equal the fp64 direct sum."""
    from nbd.plummer import generate_plummer
    n = 40000
    p, v, m = (np.asarray(t, dtype=np.float32) for t in generate_plummer(n, seed=5))
    sim = _sim((p, v, m), 0.0)
    assert sim.tree_counters() == (0, -(-n // 8) * -(-n // 64))
    rows = np.random.default_rng(1).choice(n, 64, replace=False)
    pf, mf = p.astype(np.float64), m.astype(np.float64)
    d = pf[None, :, :] - pf[rows, None, :]
    w = ((d * d).sum(2) + to.SOFTENING ** 2) ** -1.5
    w[np.arange(64), rows] = 0.0
    ref = (d * (w * mf[None, :])[:, :, None]).sum(1)
    err = row_rel(_np(sim.accelerations)[rows], ref)
    print(f"n = {n}, theta = 0: row_rel of 64 sampled rows against the fp64 direct sum {err:.3e}")
    assert err < 3e-6


@pytest.mark.parametrize("quadrupole", [True, False])
@pytest.mark.parametrize("theta", [0.5, 0.75])
@pytest.mark.parametrize("name", CASES)
def test_same_tree_same_answer(name, theta, quadrupole, gpu_device):
    _same_tree_same_answer(name, to.case(name), theta, quadrupole)


@pytest.mark.parametrize("name", CASES)
def test_order_is_a_permutation_and_spatially_as_good(name, gpu_device):
    sim = _sim(name, 0.5)
    order = _np(sim.tree_order())
    assert order.dtype == np.int32 and sorted(order.tolist()) == list(range(sim.n))
    p, _, m = to.case(name)
    with_gpu_order = to.tree_accel(p, m, 0.5, to.SOFTENING, order=order)[1]
    own = _own_order_counters(name, 0.5)
    print(f"{name}: rejected level-0 nodes with the GPU's order {with_gpu_order[1]}, with the fp64 Morton order {own[1]}")
    assert with_gpu_order[1] <= 1.05 * own[1]


def _small(n):
    from nbd.plummer import generate_plummer
    p, v, m = generate_plummer(n, seed=11)
    return p.astype(np.float32), v.astype(np.float32), m.astype(np.float32)


def test_one_body_feels_nothing(gpu_device):
    sim = _sim(_small(1), 0.5)
    assert torch.equal(sim.accelerations, torch.zeros((1, 3), device="cuda"))
    assert sim.tree_counters() == (0, 1) and _np(sim.tree_order()).tolist() == [0]
    sim.step()
    assert torch.isfinite(sim.positions).all() and torch.equal(sim.accelerations, torch.zeros((1, 3), device="cuda"))


@pytest.mark.parametrize("n", [3, 65])
@pytest.mark.parametrize("theta", [0.5, 0.75])
def test_small_systems_hold_the_same_bars(n, theta, gpu_device):
    _same_tree_same_answer(("E", n), _small(n), theta, True)


def test_ragged_last_group_is_finite(gpu_device):
    """B: 1000 = 15 x 64 + 40 bodies -- the lanes behind the last body take part in nothing."""
    sim = _sim("B", 0.5)
    order = _np(sim.tree_order()).astype(np.int64)
    last = order[15 * 64:]
    acc = _np(sim.accelerations)
    assert len(last) == 40 and np.isfinite(acc).all() and (np.linalg.norm(acc[last], axis=1) > 0).all()


def test_empty_system_constructs_and_steps(gpu_device):
    z = np.zeros((0, 3), dtype=np.float32)
    sim = _sim((z, z, np.zeros(0, dtype=np.float32)), 0.5)
    sim.step()
    assert sim.accelerations.shape == (0, 3) and sim.tree_counters() == (0, 0) and sim.tree_order().shape == (0,)
    assert sim.run(2)[1].positions.shape == (0, 3)


def test_eps0_coincident_bodies_behave_like_the_direct_kernel(gpu_device):
    """softening = 0, theta = 0: j == i is excluded by index, so two distinct bodies at one point give the NaNs
    LeapFrogSimulator.compute_accelerations() gives, and the other rows stay finite."""
    pos = np.array([[0., 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0]], dtype=np.float32)
    arrays = (pos, np.zeros((4, 3), dtype=np.float32), np.ones(4, dtype=np.float32))
    tree = _np(_sim(arrays, 0.0, softening=0.0).accelerations)
    direct = _np(_sim(arrays, 0.0, cls="LeapFrogSimulator", softening=0.0).accelerations)
    assert np.array_equal(np.isnan(tree), np.isnan(direct)) and np.array_equal(np.isinf(tree), np.isinf(direct))
    assert np.isnan(tree[1]).any() and np.isnan(tree[2]).any()
    ok = np.isfinite(direct)
    assert np.allclose(tree[ok], direct[ok], rtol=3e-6, atol=0)


def test_bit_identical_from_run_to_run_and_independent_of_the_callers_order(gpu_device):
    a, b = _sim("A", 0.5), _sim("A", 0.5)
    for _ in range(3):
        a.step(); b.step()
    for key in ("positions", "velocities", "accelerations"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    assert torch.equal(a.tree_order(), b.tree_order()) and a.tree_counters() == b.tree_counters()
    p, v, m = to.case("A")
    perm = np.random.default_rng(4).permutation(len(p))
    shuffled = _sim((p[perm], v[perm], m[perm]), 0.5)
    ref = _np(_sim("A", 0.5).accelerations)
    err = row_rel(_np(shuffled.accelerations), ref[perm])
    print(f"A shuffled in the caller's order: row_rel {err:.3e}")
    assert err < 3e-6


def test_step_follows_the_direct_leapfrog(gpu_device):
    K, dt = 5, 0.01
    direct = _sim("A", 0.0, cls="LeapFrogSimulator")
    exact = _sim("A", 0.0)
    tree = _sim("A", 0.5)
    force_err = float(np.linalg.norm(_np(tree.accelerations).astype(np.float64) - _np(direct.accelerations), axis=1).max())
    for _ in range(K):
        direct.step(); exact.step(); tree.step()
    for key in ("positions", "velocities"):
        err = row_rel(_np(getattr(exact, key)), _np(getattr(direct, key)))
        print(f"theta = 0, {K} steps, {key}: row_rel against LeapFrogSimulator {err:.3e}")
        assert err < 2e-6, key
    drift = float(np.linalg.norm(_np(tree.positions).astype(np.float64) - _np(direct.positions), axis=1).max())
    bound = 2 * ((K * dt) ** 2 / 2) * force_err + 1e-6
    print(f"theta = 0.5, {K} steps: max |x_tree - x_direct| {drift:.3e}, bound {bound:.3e} (force error {force_err:.3e})")
    assert drift <= bound


def test_linearity_in_mass_and_g(gpu_device):
    """Scaling the masses by 2 and G by 1/2 changes no bit: powers of two are exact through the fp64 node sums, the
    fp32 node records and the walk."""
    from nbd import tree
    p, _, m = to.case("A")
    n = len(p)
    pos, m1 = torch.tensor(p).cuda(), torch.tensor(m).cuda()
    ws = tree.workspace(n, "cuda")
    counters = torch.zeros(2, dtype=torch.int64, device="cuda")
    order_a = tree.build(pos, m1, ws)
    a = tree.accel(ws, n, 0.5, 0.01, 1.0, counters=counters)
    seen = counters.cpu().tolist()
    order_b = tree.build(pos, 2 * m1, ws)
    b = tree.accel(ws, n, 0.5, 0.01, 0.5)                  # counters are optional
    assert torch.equal(order_a, order_b) and torch.equal(a, b)
    assert seen[0] > 0 and 0 < seen[1] < (n // 8) * (n // 64)


def test_run_is_eager_and_reports_states(gpu_device):
    from galaxify import simulation
    p, v, m = to.case("B")
    kw = dict(positions=p, velocities=v, masses=m, softening=to.SOFTENING, dt=0.01, device="cuda", theta=0.5)
    a = simulation.TreeLeapFrogSimulator(calc_energy=True, **kw)
    b = simulation.TreeLeapFrogSimulator(calc_energy=False, **kw)
    assert not a._graph_run_ok(8)
    states = a.run(8)
    for _ in range(8):
        b.step()
    assert len(states) == 8 and torch.equal(states[-1].positions, b.positions.cpu())
    assert torch.equal(states[-1].accelerations, b.accelerations.cpu())
    u, k = a.compute_energies()
    assert states[-1].u_energy == u and states[-1].k_energy == k and u < 0 < k
