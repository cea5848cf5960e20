"""The tree potential without a GPU: the fp64 restatement (tests/tree_potential_oracle.py) against the fp64 all-pairs sum
on the inputs the GPU tests use, its consistency with the tree force, the argument checks of the two C entries, the
workspace's growth and the refusal of TreeLeapFrogSimulator(potential=...). No kernel is launched here."""
import ctypes

import numpy as np
import pytest

import tree_oracle as to
import tree_potential_oracle as tpo
from nbd import _lib

CASES = ["A", "B", "C", "D"]
# what a prototype of the restatement gave with the fp64 Morton order (theta = 0.5, quadrupoles): max and rms relative
# row error against the fp64 all-pairs sum, |U_tree - U_direct| / |U|. They fix the magnitude (max < 4 x, rms < 2 x: the
# margins of test_tree_host.py), not the digits.
EXPECTED = {"A": (4.2e-5, 4.0e-6, 1.2e-6), "B": (2.9e-5, 7.1e-6, 3.0e-6),
            "C": (6.5e-5, 1.0e-5, 6.2e-6), "D": (3.1e-4, 2.3e-5, 1.2e-6)}

_cache = {}


def oracle_run(name, theta, quadrupole=True, **kw):
    key = (name, theta, quadrupole, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _cache:
        p, _, m = to.case(name)
        _cache[key] = tpo.tree_potential(p, m, theta, to.SOFTENING, quadrupole=quadrupole, **kw)
    return _cache[key]


def direct(name):
    if ("direct", name) not in _cache:
        p, _, m = to.case(name)
        _cache[("direct", name)] = tpo.direct_potential(p, m, to.SOFTENING)
    return _cache[("direct", name)]


def _rms(e):
    return float(np.sqrt((e ** 2).mean()))


@pytest.mark.parametrize("name", CASES)
def test_oracle_theta0_is_the_direct_sum(name):
    """D holds 16 coincident copies of each body: a self term excluded by position instead of by index would drop
    15 m / eps from every row."""
    phi, (cells, leaves) = oracle_run(name, 0.0)
    n = len(phi)
    assert tpo.row_errors(phi, direct(name)).max() < 1e-12
    assert (cells, leaves) == (0, -(-n // 8) * -(-n // 64))


@pytest.mark.parametrize("theta", [0.0, 0.5, 0.75])
@pytest.mark.parametrize("name", CASES)
def test_oracle_walks_like_the_force_oracle(name, theta):
    p, _, m = to.case(name)
    assert oracle_run(name, theta)[1] == to.tree_accel(p, m, theta, to.SOFTENING)[1]


def test_cell_potential_is_the_potential_of_the_cell_force():
    """16 random cells {r, M, Q}, eps = 0.1: the central difference of the cell potential (step 1e-6) is the cell term
    of the force to 1e-7 of its norm -- with and without the quadrupole."""
    rng = np.random.default_rng(0)
    h, eps2 = 1e-6, to.SOFTENING ** 2
    for k in range(16):
        c = rng.uniform(-2.0, 2.0, 3)
        c *= max(1.0, 0.5 / np.linalg.norm(c))
        x = np.zeros(3)
        M = rng.uniform(0.5, 2.0)
        d = rng.normal(size=(8, 3)) * 0.2
        w = rng.uniform(0.0, 0.25, 8)
        Q = np.einsum("k,kab->ab", w, 3.0 * d[:, :, None] * d[:, None, :] - (d * d).sum(1)[:, None, None] * np.eye(3))
        for quad in (True, False):
            grad = np.array([(tpo.cell_potential(x + h * e, c, M, Q, eps2, quad) -
                              tpo.cell_potential(x - h * e, c, M, Q, eps2, quad)) / (2 * h) for e in np.eye(3)])
            a = tpo.cell_accel(x, c, M, Q, eps2, quad)
            assert np.linalg.norm(-grad - a) <= 1e-7 * np.linalg.norm(a), (k, quad)


def test_cell_terms_restated_here_are_the_oracles():
    """cell_accel is tree_oracle.tree_accel's cell term and cell_potential this oracle's: 64 bodies about the origin and
    a lone 65th far away, in index order. The last group is that body alone and its walk accepts exactly one cell, the
    level-1 node of the other 64 (its own nodes have s = 0 and d = 0: opened, and j == i leaves nothing)."""
    rng = np.random.default_rng(1)
    pos = np.vstack([rng.normal(size=(64, 3)) * 0.3, [[40.0, 1.0, -2.0]]])
    mass = rng.uniform(0.5, 1.5, 65)
    eps2 = to.SOFTENING ** 2
    for quad in (True, False):
        acc, _ = to.tree_accel(pos, mass, 0.75, to.SOFTENING, quadrupole=quad, order=np.arange(65))
        phi, _ = tpo.tree_potential(pos, mass, 0.75, to.SOFTENING, quadrupole=quad, order=np.arange(65))
        L1 = to.build_nodes(pos, mass)[1]
        cell = (L1["c"][0], L1["M"][0], L1["Q"][0], eps2, quad)
        assert np.allclose(acc[64], tpo.cell_accel(pos[64], *cell), rtol=1e-13, atol=0)
        assert np.isclose(phi[64], tpo.cell_potential(pos[64], *cell), rtol=1e-13, atol=0)


@pytest.mark.parametrize("name", CASES)
def test_oracle_against_the_direct_sum(name):
    phi, _ = oracle_run(name, 0.5)
    _, _, m = to.case(name)
    err = tpo.row_errors(phi, direct(name))
    u_tree, u_dir = tpo.potential_energy(m, phi), tpo.potential_energy(m, direct(name))
    du = abs(u_tree - u_dir) / abs(u_dir)
    e_max, e_rms, _ = EXPECTED[name]
    print(f"{name}: max {err.max():.3e} rms {_rms(err):.3e} |dU|/|U| {du:.3e}")
    assert err.max() < 4 * e_max and _rms(err) < 2 * e_rms


def test_oracle_monopole_only_is_coarser():
    mono = tpo.row_errors(oracle_run("C", 0.5, quadrupole=False)[0], direct("C"))
    quad = tpo.row_errors(oracle_run("C", 0.5)[0], direct("C"))
    assert quad.max() < mono.max() and _rms(quad) < _rms(mono)
    assert oracle_run("C", 0.5, quadrupole=False)[1] == oracle_run("C", 0.5)[1]       # the same walk


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("theta", [0.5, 0.75])
def test_float32_opening_test_decides_like_float64(name, theta):
    """What the GPU tests lean on: the opening test in float32 flips (almost) no decision -- both counters within 1 %
    and at least 99 % of the rows within 3e-6 |phi| of the float64 walk's."""
    p64, c64 = oracle_run(name, theta)
    p32, c32 = oracle_run(name, theta, opening_dtype=np.float32)
    for got, want in zip(c32, c64):
        assert abs(got - want) <= 0.01 * want
    assert (tpo.row_errors(p32, p64) < 3e-6).mean() >= 0.99


def test_oracle_small_systems():
    p, _, m = to.case("B")
    phi, counters = tpo.tree_potential(p[:1], m[:1], 0.5, to.SOFTENING)
    assert np.array_equal(phi, np.zeros(1)) and counters == (0, 1)
    assert tpo.tree_potential(p[:0], m[:0], 0.5, to.SOFTENING)[1] == (0, 0)
    for n in (3, 65):
        phi, _ = tpo.tree_potential(p[:n], m[:n], 0.5, to.SOFTENING)
        assert tpo.row_errors(phi, tpo.direct_potential(p[:n], m[:n], to.SOFTENING)).max() < 1e-3
    # eps = 0: a coincident distinct body is kept (-inf), the self term is not
    pos = np.array([[0., 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0]])
    phi, _ = tpo.tree_potential(pos, np.ones(4), 0.0, 0.0, order=np.arange(4))
    assert np.isneginf(phi).tolist() == [False, True, True, False]
    assert np.array_equal(phi, tpo.direct_potential(pos, np.ones(4), 0.0))


# ---------------------------------------------------------------- the C entries

def _entries():
    L = _lib.lib()
    pot = lambda ws, n, theta, out: L.nbd_tree_potential_f32(ws, n, theta, 0.01, 1.0, 1, out, None, None)
    both = lambda ws, n, theta, out: L.nbd_tree_accel_potential_f32(ws, n, theta, 0.01, 1.0, 1, out, out, None, None)
    return [("nbd_tree_potential_f32", pot), ("nbd_tree_accel_potential_f32", both)]


@pytest.mark.parametrize("which", [0, 1])
def test_bad_arguments_are_rejected_without_touching_the_gpu(which):
    """The table of test_tree_bad_arguments_are_rejected_without_touching_the_gpu for nbd_tree_accel_f32, on the two
    new entries."""
    name, call = _entries()[which]
    assert call(None, -1, 0.5, None) == -1, name
    assert call(None, 5, 0.5, None) == -1
    assert call(0x1000, 5, 0.5, None) == -1                        # no output
    assert call(0x1000, 5, -0.5, 0x1000) == -1                     # theta < 0
    assert call(0x1000, 5, float("nan"), 0x1000) == -1
    assert call(0x1010, 5, 0.5, 0x1000) == -1                      # misaligned workspace
    assert call(0x1000, (1 << 24) + 1, 0.5, 0x1000) == -3
    assert call(None, 0, 0.5, None) == 0                           # n == 0 is a no-op


def test_fused_entry_wants_both_outputs():
    L = _lib.lib()
    assert L.nbd_tree_accel_potential_f32(0x1000, 5, 0.5, 0.01, 1.0, 1, None, 0x1000, None, None) == -1     # no acc_out
    assert L.nbd_tree_accel_potential_f32(0x1000, 5, 0.5, 0.01, 1.0, 1, 0x1000, None, None, None) == -1     # no phi_out


@pytest.mark.parametrize("n", [1, 8, 9, 64, 65, 511, 512, 513, 4096, 40000, 1 << 24])
def test_workspace_holds_the_potential_slabs(n):
    """Where the plan splits a group's walk over 8 waves (a level with 64 nodes or more: n > 504), the workspace also
    holds 8 slabs of n doubles."""
    L = _lib.lib()
    total = ctypes.c_int(-1)
    assert L.nbd_tree_plan(n, None, total) == 0
    splits = max(to.plan(n)[2]) >= 64
    assert splits == (n > 504)
    assert L.nbd_tree_workspace_bytes(n) >= total.value * 48 + n * 16 + (8 * 8 * n if splits else 0)
    if splits:      # every region of the force included: sorted bodies, nodes, moments, boxes, fp32 slabs, sort keys
        assert L.nbd_tree_workspace_bytes(n) >= total.value * (48 + 13 * 8 + 32) + n * (16 + 24 + 8 * 12) + 8 * 8 * n


def test_simulator_refuses_an_unknown_potential():
    """Before a device is resolved: it holds on a box without a GPU."""
    from galaxify import simulation
    z = np.zeros((4, 3))
    kw = dict(positions=z, velocities=z, masses=np.ones(4))
    for bad in ("nonsense", "Tree", None, ""):
        with pytest.raises(ValueError, match="potential"):
            simulation.TreeLeapFrogSimulator(potential=bad, **kw)
