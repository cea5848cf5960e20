"""The tree potential on the GPU (csrc/tree_force.hip, nbd/tree.py, TreeLeapFrogSimulator(potential="tree")) against the
fp64 restatement of tests/tree_potential_oracle.py fed the GPU's own body order, against the fp64 all-pairs sum and
against the walks it shares its kernel with. Inputs A-D and the softening are tree_oracle.case's; every reference is
computed once and shared."""
import numpy as np
import pytest
import torch

import tree_oracle as to
import tree_potential_oracle as tpo

pytestmark = pytest.mark.gpu

CASES = ["A", "B", "C", "D"]
# theta = 0, every row: 6 roundings of the pair term, an fp32 chain of at most 7 adds (the 8 bodies of a level-0 node;
# everything above is fp64), the fp32 -> fp64 step, and a margin of 2 -- the form of test_diagnostics_gpu.PHI_TOL
PHI_TOL = 16 * 2.0 ** -24
_refs = {}


def _np(t):
    return t.detach().cpu().numpy()


def _rms(e):
    return float(np.sqrt((e ** 2).mean())) if e.size else 0.0


def _sim(arrays, theta=0.5, quadrupole=True, cls="TreeLeapFrogSimulator", softening=to.SOFTENING, **kw):
    from galaxify import simulation
    p, v, m = to.case(arrays) if isinstance(arrays, str) else arrays
    extra = dict(theta=theta, quadrupole=quadrupole) if cls == "TreeLeapFrogSimulator" else {}
    kw.setdefault("calc_energy", False)
    return getattr(simulation, cls)(positions=p, velocities=v, masses=m, g_const=1.0, softening=softening, dt=0.01,
                                    device="cuda", **extra, **kw)


def _direct(key, arrays=None):
    if ("direct", key) not in _refs:
        p, _, m = to.case(key) if arrays is None else arrays
        _refs[("direct", key)] = tpo.direct_potential(p, m, to.SOFTENING)
    return _refs[("direct", key)]


def _small(n):
    from nbd.plummer import generate_plummer
    p, v, m = generate_plummer(n, seed=11)
    return p.astype(np.float32), v.astype(np.float32), m.astype(np.float32)


def _built(arrays):
    """(workspace, order, n) of one build through nbd.tree."""
    from nbd import tree
    p, _, m = arrays
    n = len(p)
    ws = tree.workspace(n, "cuda")
    order = tree.build(torch.tensor(p).cuda(), torch.tensor(m).cuda(), ws)
    return ws, order, n


def _counters():
    return torch.zeros(2, dtype=torch.int64, device="cuda")


# ---------------------------------------------------------------- 1. theta = 0 is the all-pairs sum

@pytest.mark.parametrize("name", CASES)
def test_theta0_is_the_direct_sum(name, gpu_device):
    sim = _sim(name, 0.0, potential="tree")
    phi, ref = _np(sim.compute_potentials()), _direct(name)
    err = tpo.row_errors(phi, ref)
    print(f"{name}: theta = 0 max row error against the fp64 all-pairs sum {err.max():.3e} (bar {PHI_TOL:.3e})")
    assert phi.dtype == np.float64 and phi.shape == (sim.n,)
    assert (np.abs(phi - ref) <= PHI_TOL * np.abs(ref)).all()


@pytest.mark.parametrize("n", [1, 3, 65])
def test_theta0_on_one_wave_without_slabs(n, gpu_device):
    arrays = _small(n)
    phi = _np(_sim(arrays, 0.0, potential="tree").compute_potentials())
    ref = tpo.direct_potential(arrays[0], arrays[2], to.SOFTENING)
    if n == 1:
        assert phi.tolist() == [0.0]
    print(f"n = {n}: max row error {tpo.row_errors(phi, ref).max() if n > 1 else 0.0:.3e}")
    assert (np.abs(phi - ref) <= PHI_TOL * np.abs(ref)).all()


def test_theta0_at_a_deeper_split_level(gpu_device):
    """n = 40 000: the waves that share a group divide the tree at level 2. Every level-0 node is summed exactly once
    (the counter), and sampled rows equal the fp64 all-pairs rows."""
    from nbd import tree
    from nbd.plummer import generate_plummer
    n = 40000
    p, v, m = (np.asarray(t, dtype=np.float32) for t in generate_plummer(n, seed=5))
    sim = _sim((p, v, m), 0.0, potential="tree")
    phi = _np(sim.compute_potentials())
    counters = _counters()
    again = tree.potential(sim._tree_ws, n, 0.0, sim._eps2, sim._g, counters=counters)
    assert tuple(counters.cpu().tolist()) == (0, -(-n // 8) * -(-n // 64))
    assert torch.equal(again.cpu(), torch.from_numpy(phi))
    rows = np.random.default_rng(1).choice(n, 64, replace=False)
    pf, mf = p.astype(np.float64), m.astype(np.float64)
    d = pf[None, :, :] - pf[rows, None, :]
    w = ((d * d).sum(2) + to.SOFTENING ** 2) ** -0.5
    w[np.arange(64), rows] = 0.0
    ref = -(w * mf[None, :]).sum(1)
    print(f"n = {n}, theta = 0: max error of 64 sampled rows {tpo.row_errors(phi[rows], ref).max():.3e}")
    assert (np.abs(phi[rows] - ref) <= PHI_TOL * np.abs(ref)).all()


# ---------------------------------------------------------------- 2. same tree, same answer

@pytest.mark.parametrize("quadrupole", [True, False])
@pytest.mark.parametrize("theta", [0.5, 0.75])
@pytest.mark.parametrize("name", CASES)
def test_same_tree_same_answer(name, theta, quadrupole, gpu_device):
    from nbd import tree
    arrays = to.case(name)
    p, _, m = arrays
    ws, order, n = _built(arrays)
    c_phi, c_acc = _counters(), _counters()
    phi = _np(tree.potential(ws, n, theta, to.SOFTENING ** 2, 1.0, quadrupole, counters=c_phi))
    tree.accel(ws, n, theta, to.SOFTENING ** 2, 1.0, quadrupole, counters=c_acc)
    ref, ref_counters = tpo.tree_potential(p, m, theta, to.SOFTENING, quadrupole=quadrupole, order=_np(order))
    rows = tpo.row_errors(phi, ref)
    direct = _direct(name)
    e_gpu, e_ref = tpo.row_errors(phi, direct), tpo.row_errors(ref, direct)
    print(f"{name} theta={theta} quad={quadrupole}: rows within 3e-6 of the oracle {np.mean(rows < 3e-6):.4f} (max "
          f"{rows.max():.2e}), counters {c_phi.cpu().tolist()} (oracle {ref_counters}), vs direct max {e_gpu.max():.3e} "
          f"(oracle {e_ref.max():.3e}), rms {_rms(e_gpu):.3e} (oracle {_rms(e_ref):.3e})")
    assert np.isfinite(phi).all()
    assert np.mean(rows < 3e-6) >= 0.99
    assert c_phi.cpu().tolist() == c_acc.cpu().tolist()
    assert e_gpu.max() <= 2 * e_ref.max() + 3e-6 and _rms(e_gpu) <= 2 * _rms(e_ref) + 3e-6


# ---------------------------------------------------------------- 3. fused = separate

@pytest.mark.parametrize("key", ["A", 65])
@pytest.mark.parametrize("quadrupole", [True, False])
def test_fused_walk_is_the_two_walks(key, quadrupole, gpu_device):
    """A: 8 waves per group and slabs; 65 bodies: one wave, no slabs."""
    from nbd import tree
    ws, _, n = _built(to.case(key) if isinstance(key, str) else _small(key))
    walk = (ws, n, 0.5, to.SOFTENING ** 2, 1.0, quadrupole)
    c = [_counters() for _ in range(3)]
    acc = tree.accel(*walk, counters=c[0])
    phi = tree.potential(*walk, counters=c[1])
    acc2, phi2 = tree.accel_potential(*walk, counters=c[2])
    assert torch.equal(acc, acc2) and torch.equal(phi, phi2)
    assert c[0].cpu().tolist() == c[1].cpu().tolist() == c[2].cpu().tolist() and c[0].sum().item() > 0
    # and into the caller's buffers
    out = (torch.full((n, 3), float("nan"), device="cuda"),
           torch.full((n,), float("nan"), dtype=torch.float64, device="cuda"))
    got = tree.accel_potential(*walk, out=out)
    assert got[0] is out[0] and got[1] is out[1] and torch.equal(out[0], acc) and torch.equal(out[1], phi)


# ---------------------------------------------------------------- 4. potential="direct" is today's behaviour

def test_direct_and_no_keyword_are_the_all_pairs_potential(gpu_device):
    want = _sim("B", cls="LeapFrogSimulator").compute_potentials()
    assert torch.equal(_sim("B").compute_potentials(), want)
    assert torch.equal(_sim("B", potential="direct").compute_potentials(), want)
    assert _sim("B").potential == "direct"


# ---------------------------------------------------------------- 5. invariants

@pytest.mark.parametrize("theta", [0.5, 0.75])
@pytest.mark.parametrize("name", ["A", "B"])
def test_invariants_differ_in_the_potential_energy_alone(name, theta, gpu_device):
    p, _, m = to.case(name)
    t_sim = _sim(name, theta, potential="tree")
    t, d = t_sim.compute_invariants().row(), _sim(name, theta, potential="direct").compute_invariants().row()
    assert t[:11] == d[:11]                                   # M, C, P, L, K: identical bits
    ref = tpo.tree_potential(p, m, theta, to.SOFTENING, order=_np(t_sim.tree_order()))[0]
    u_ref, u_dir = tpo.potential_energy(m, ref), tpo.potential_energy(m, _direct(name))
    own = abs(u_ref - u_dir) / abs(u_dir)
    got = abs(t[11] - d[11]) / abs(d[11])
    print(f"{name} theta={theta}: |U_tree - U_direct| / |U_direct| {got:.3e} (the oracle's own {own:.3e})")
    assert got <= 2 * own + 1e-6
    assert t[12] == t[10] + t[11] and t[13] == -2.0 * t[10] / t[11]


# ---------------------------------------------------------------- 6. run() with calc_invariants

def test_run_takes_the_invariants_from_the_steps_own_walk(gpu_device):
    fused = _sim("B", calc_invariants=True, potential="tree")
    plain = _sim("B", calc_invariants=False, potential="tree")
    states = fused.run(5)
    for _ in range(5):
        plain.step()
    for key in ("positions", "velocities", "accelerations"):
        assert torch.equal(getattr(fused, key), getattr(plain, key)), key
        assert torch.equal(getattr(states[-1], key), getattr(plain, key).cpu()), key
    assert fused.tree_counters() == plain.tree_counters()
    assert all(s.invariants is not None for s in states)
    # the fused walk's phi against a fresh build and the phi-only walk's
    assert states[-1].invariants.row() == fused.compute_invariants().row()
    assert fused.tree_counters() == plain.tree_counters()


# ---------------------------------------------------------------- 7. edges

def test_empty_system(gpu_device):
    z = np.zeros((0, 3), dtype=np.float32)
    sim = _sim((z, z, np.zeros(0, dtype=np.float32)), calc_invariants=True, potential="tree")
    phi = sim.compute_potentials()
    assert phi.shape == (0,) and phi.dtype == torch.float64
    assert sim.compute_invariants().row() == [0.0] * 16
    assert sim.run(2)[1].positions.shape == (0, 3)


def test_eps0_coincident_bodies_behave_like_the_direct_kernel(gpu_device):
    pos = np.array([[0., 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0]], dtype=np.float32)
    arrays = (pos, np.zeros((4, 3), dtype=np.float32), np.ones(4, dtype=np.float32))
    tree = _np(_sim(arrays, 0.0, softening=0.0, potential="tree").compute_potentials())
    direct = _np(_sim(arrays, cls="LeapFrogSimulator", softening=0.0).compute_potentials())
    assert np.array_equal(np.isneginf(tree), np.isneginf(direct)) and np.isneginf(tree).tolist() == [False, True, True, False]
    assert not np.isnan(tree).any() and not np.isposinf(tree).any()
    ok = np.isfinite(direct)
    assert np.allclose(tree[ok], direct[ok], rtol=3e-6, atol=0)


def test_eps0_body_at_the_origin_ignores_the_padding(gpu_device):
    """n = 9: the second level-0 node holds one body and 7 zero rows of padding, which sit at the origin -- where body 0
    is. Without the j < n mask its row would take 0 * inf."""
    rng = np.random.default_rng(2)
    pos = rng.uniform(0.5, 2.0, (9, 3)).astype(np.float32)
    pos[0] = 0.0
    arrays = (pos, np.zeros((9, 3), dtype=np.float32), rng.uniform(0.5, 1.5, 9).astype(np.float32))
    for theta in (0.0, 0.5):
        phi = _np(_sim(arrays, theta, softening=0.0, potential="tree").compute_potentials())
        assert np.isfinite(phi).all()
    ref = tpo.direct_potential(arrays[0], arrays[2], 0.0)
    phi = _np(_sim(arrays, 0.0, softening=0.0, potential="tree").compute_potentials())
    assert (np.abs(phi - ref) <= PHI_TOL * np.abs(ref)).all()


def test_bit_identical_and_independent_of_the_callers_order(gpu_device):
    a, b = _sim("A", potential="tree"), _sim("A", potential="tree")
    ref = a.compute_potentials()
    assert torch.equal(ref, b.compute_potentials()) and torch.equal(ref, a.compute_potentials())
    p, v, m = to.case("A")
    perm = np.random.default_rng(4).permutation(len(p))
    shuffled = _np(_sim((p[perm], v[perm], m[perm]), potential="tree").compute_potentials())
    err = tpo.row_errors(shuffled, _np(ref)[perm]).max()
    print(f"A shuffled in the caller's order: max row error {err:.3e}")
    assert err < 3e-6


def test_compute_potentials_rebuilds_on_assigned_positions(gpu_device):
    sim = _sim("B", potential="tree")
    before = sim.compute_potentials()
    sim.positions = sim.positions * 1.5
    after = sim.compute_potentials()
    p, v, m = to.case("B")
    fresh = _sim((p * np.float32(1.5), v, m), potential="tree").compute_potentials()
    assert torch.equal(after, fresh) and not torch.equal(after, before)


def test_linearity_in_mass_and_g(gpu_device):
    """Scaling the masses by 2 and G by 1/2 changes no bit of phi."""
    from nbd import tree
    p, _, m = to.case("A")
    n = len(p)
    pos, m1 = torch.tensor(p).cuda(), torch.tensor(m).cuda()
    ws = tree.workspace(n, "cuda")
    tree.build(pos, m1, ws)
    a = tree.potential(ws, n, 0.5, 0.01, 1.0)
    tree.build(pos, 2 * m1, ws)
    b = tree.potential(ws, n, 0.5, 0.01, 0.5)
    assert torch.equal(a, b) and (a < 0).all()
