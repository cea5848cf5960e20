"""The tree force without a GPU: the fp64 restatement (tests/tree_oracle.py) against the fp64 direct sum on the inputs the
GPU tests use, the host arithmetic of nbd_tree_plan, the argument checks of the C entries and the refusals of
TreeLeapFrogSimulator. No kernel is launched here."""
import ctypes

import numpy as np
import pytest
import torch

import tree_oracle as to
from nbd import _lib

# what the fp64 restatement gave when the inputs were chosen (theta = 0.5, quadrupole): max and rms row error against
# the fp64 direct sum, accepted cells, rejected level-0 nodes
EXPECTED = {"A": (4.0e-4, 2.4e-5, 1407, 4944), "B": (6.2e-4, 4.9e-5, 362, 1463),
            "C": (8.0e-4, 1.0e-4, 6460, 26154), "D": (1.8e-3, 1.5e-4, 887, 648)}

_cache = {}


def oracle_run(name, theta, quadrupole=True, **kw):
    key = (name, theta, quadrupole, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _cache:
        p, _, m = to.case(name)
        _cache[key] = to.tree_accel(p, m, theta, to.SOFTENING, quadrupole=quadrupole, **kw)
    return _cache[key]


def direct(name):
    if ("direct", name) not in _cache:
        p, _, m = to.case(name)
        _cache[("direct", name)] = to.direct_accel(p, m, to.SOFTENING)
    return _cache[("direct", name)]


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_oracle_theta0_is_the_direct_sum(name):
    acc, (cells, leaves) = oracle_run(name, 0.0)
    n = len(acc)
    assert to.row_errors(acc, direct(name)).max() < 1e-12
    assert (cells, leaves) == (0, -(-n // 8) * -(-n // 64))


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_oracle_against_the_direct_sum(name):
    """theta = 0.5 with quadrupoles: a truncation error of a few 1e-4 at the worst row, and the walk does a fraction of
    the direct sum's work. EXPECTED holds the figures of the prototype the inputs were chosen with: the same
    constructions, not the same realisation bit for bit (its draws of the mass factors and its tie order are not
    recorded), so they fix the magnitude, not the digits: the rms error within a factor 2 upwards, the maximum -- one
    row out of thousands, the tail of a skewed distribution -- within a factor 4, the counters within 15 %."""
    acc, (cells, leaves) = oracle_run(name, 0.5)
    err = to.row_errors(acc, direct(name))
    e_max, e_rms, want_cells, want_leaves = EXPECTED[name]
    print(name, err.max(), np.sqrt((err ** 2).mean()), cells, leaves)
    assert err.max() < 4 * e_max and np.sqrt((err ** 2).mean()) < 2 * e_rms
    assert abs(cells - want_cells) <= 0.15 * want_cells and abs(leaves - want_leaves) <= 0.15 * want_leaves
    n = len(acc)
    assert leaves < 0.85 * (-(-n // 8) * -(-n // 64))


def test_oracle_monopole_only_is_coarser():
    mono = to.row_errors(oracle_run("C", 0.5, quadrupole=False)[0], direct("C"))
    quad = to.row_errors(oracle_run("C", 0.5)[0], direct("C"))
    assert quad.max() < mono.max() < 1e-2 and np.sqrt((mono ** 2).mean()) < 2e-3
    assert oracle_run("C", 0.5, quadrupole=False)[1] == oracle_run("C", 0.5)[1]       # the same walk


@pytest.mark.parametrize("name", sorted(EXPECTED))
@pytest.mark.parametrize("theta", [0.5, 0.75])
def test_float32_opening_test_decides_like_float64(name, theta):
    """What the GPU tests lean on: deciding s^2 < theta^2 d^2 in float32, from float32 c and s, flips (almost) no
    decision -- both counters within 1 % and at least 99 % of the rows within 3e-6 of the float64 walk's."""
    a64, c64 = oracle_run(name, theta)
    a32, c32 = oracle_run(name, theta, opening_dtype=np.float32)
    for got, want in zip(c32, c64):
        assert abs(got - want) <= 0.01 * want
    assert (to.row_errors(a32, a64) < 3e-6).mean() >= 0.99


def test_oracle_accepts_an_order_and_small_systems():
    p, _, m = to.case("B")
    own = to.morton_order(p)
    assert sorted(own.tolist()) == list(range(len(p)))
    a, c = to.tree_accel(p, m, 0.5, to.SOFTENING, order=own)
    b, d = oracle_run("B", 0.5)
    assert np.array_equal(a, b) and c == d
    # an arbitrary order is a worse tree, not a wrong one
    shuffled = np.random.default_rng(0).permutation(len(p))
    a, c = to.tree_accel(p, m, 0.5, to.SOFTENING, order=shuffled)
    assert to.row_errors(a, direct("B")).max() < 5e-3 and c[1] > d[1]
    acc, counters = to.tree_accel(p[:1], m[:1], 0.5, to.SOFTENING)
    assert np.array_equal(acc, np.zeros((1, 3))) and counters == (0, 1)
    for n in (3, 65):
        acc, _ = to.tree_accel(p[:n], m[:n], 0.5, to.SOFTENING)
        assert to.row_errors(acc, to.direct_accel(p[:n], m[:n], to.SOFTENING)).max() < 5e-3
    # a massless node takes the mean of its bodies as its centre and contributes nothing
    acc, _ = to.tree_accel(p[:100], np.zeros(100), 0.5, to.SOFTENING)
    assert np.array_equal(acc, np.zeros((100, 3)))


@pytest.mark.parametrize("n", [1, 8, 9, 64, 65, 513, 4096, 1 << 24])
def test_tree_plan_arithmetic(n):
    L = _lib.lib()
    levels, total = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.nbd_tree_plan(n, levels, total) == 0
    want = {1: (1, 1), 8: (1, 1), 9: (2, 3), 64: (2, 9), 65: (3, 12), 513: (4, 77), 4096: (4, 585),
            1 << 24: (8, (8 ** 8 - 1) // 7)}[n]
    assert (levels.value, total.value) == want == to.plan(n)[:2]
    assert L.nbd_tree_plan(n, None, None) == 0
    assert L.nbd_tree_workspace_bytes(n) >= total.value * 48 + n * 16
    from nbd import tree
    assert tree.plan(n) == {"levels": want[0], "nodes_total": want[1]}


def test_tree_plan_refuses_what_it_cannot_hold():
    L = _lib.lib()
    levels, total = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.nbd_tree_plan(0, levels, total) == 0 and (levels.value, total.value) == (0, 0)
    assert L.nbd_tree_plan((1 << 24) + 1, levels, total) == -3
    assert L.nbd_tree_plan(-1, levels, total) == -1
    assert L.nbd_tree_workspace_bytes((1 << 24) + 1) == 0 and L.nbd_tree_workspace_bytes(0) == 0
    assert L.nbd_tree_workspace_bytes(-5) == 0
    from nbd import tree
    with pytest.raises(_lib.NbdUnsupported):
        tree.plan((1 << 24) + 1)


def test_tree_bad_arguments_are_rejected_without_touching_the_gpu():
    L = _lib.lib()
    assert L.nbd_tree_build_f32(None, None, -1, None, None, 0, None) == -1
    assert L.nbd_tree_build_f32(None, None, 5, None, None, 0, None) == -1
    assert L.nbd_tree_build_f32(0x1000, 0x1000, 5, 0x1000, None, 0, None) == -1            # no workspace
    assert L.nbd_tree_build_f32(0x1000, 0x1000, 5, 0x1000, 0x1010, 1 << 30, None) == -1    # misaligned workspace
    assert L.nbd_tree_build_f32(0x1000, 0x1000, 5, 0x1000, 0x1000, 16, None) == -2         # too small
    assert L.nbd_tree_build_f32(0x1000, 0x1000, (1 << 24) + 1, 0x1000, 0x1000, 1 << 40, None) == -3
    assert L.nbd_tree_build_f32(None, None, 0, None, None, 0, None) == 0                   # n == 0 is a no-op
    assert L.nbd_tree_accel_f32(None, -1, 0.5, 0.01, 1.0, 1, None, None, None) == -1
    assert L.nbd_tree_accel_f32(None, 5, 0.5, 0.01, 1.0, 1, None, None, None) == -1
    assert L.nbd_tree_accel_f32(0x1000, 5, 0.5, 0.01, 1.0, 1, None, None, None) == -1      # no output
    assert L.nbd_tree_accel_f32(0x1000, 5, -0.5, 0.01, 1.0, 1, 0x1000, None, None) == -1   # theta < 0
    assert L.nbd_tree_accel_f32(0x1000, 5, float("nan"), 0.01, 1.0, 1, 0x1000, None, None) == -1
    assert L.nbd_tree_accel_f32(0x1000, (1 << 24) + 1, 0.5, 0.01, 1.0, 1, 0x1000, None, None) == -3
    assert L.nbd_tree_accel_f32(None, 0, 0.5, 0.01, 1.0, 1, None, None, None) == 0


def test_simulator_refusals():
    """Every refusal comes before a device is resolved or anything is allocated: it holds on a box without a GPU."""
    from galaxify import simulation
    z = np.zeros((4, 3))
    kw = dict(positions=z, velocities=z, masses=np.ones(4))
    with pytest.raises(ValueError, match="float32"):
        simulation.TreeLeapFrogSimulator(dtype=torch.float64, **kw)
    with pytest.raises(ValueError, match="process_group"):
        simulation.TreeLeapFrogSimulator(process_group=object(), **kw)
    with pytest.raises(ValueError, match="theta"):
        simulation.TreeLeapFrogSimulator(theta=-0.1, **kw)
    with pytest.raises(ValueError, match="theta"):
        simulation.TreeLeapFrogSimulator(theta=float("nan"), **kw)
    grad = torch.zeros((4, 3), requires_grad=True)
    with pytest.raises(ValueError, match="requires grad"):
        simulation.TreeLeapFrogSimulator(positions=grad, velocities=z, masses=np.ones(4))
    with pytest.raises(ValueError, match="requires grad"):
        simulation.TreeLeapFrogSimulator(positions=z, velocities=z, masses=torch.ones(4, requires_grad=True))
    with pytest.raises(RuntimeError):                       # as every simulator of this build: there is no CPU path
        simulation.TreeLeapFrogSimulator(device="cpu", **kw)
    assert issubclass(simulation.TreeLeapFrogSimulator, simulation.LeapFrogSimulator)
    assert not simulation.TreeLeapFrogSimulator._capturable() and simulation.LeapFrogSimulator._capturable()
