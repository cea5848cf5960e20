"""What tests/test_tree_build_gpu.py leans on, without a GPU: the host-only layout query nbd_tree_regions, the fp32 key
restatement against the fp64 Morton order, the oracle's groups= / cond= additions, the claim that a float32 opening test
decides exactly like a float64 one on the inputs off the Plummer path, and the node bounds. No kernel is launched here."""
import ctypes

import numpy as np
import pytest

import tree_build_oracle as tbo
import tree_oracle as to
import tree_potential_oracle as tpo
from nbd import _lib


def _regions(n):
    a, b, c = ctypes.c_size_t(7), ctypes.c_size_t(7), ctypes.c_size_t(7)
    return _lib.lib().nbd_tree_regions(n, a, b, c), (a.value, b.value, c.value)


@pytest.mark.parametrize("n", [1, 8, 9, 64, 65, 513, 33025, 1 << 24])
def test_regions_arithmetic(n):
    L = _lib.lib()
    code, (order, posm, nodes) = _regions(n)
    total = L.nbd_tree_workspace_bytes(n)
    pad = (n + 63) // 64 * 64
    assert code == 0
    assert order % 256 == posm % 256 == nodes % 256 == 0
    # each region ends before the next begins, the node records before the workspace does
    assert 0 < order and order + 4 * n <= posm and posm + 16 * pad <= nodes and nodes + 48 * to.plan(n)[1] <= total
    # the order follows the sort's two key arrays and its index array; the regions follow each other without a gap
    assert order >= 2 * 8 * n + 4 * n
    assert posm == (order + 4 * n + 255) // 256 * 256 and nodes == (posm + 16 * pad + 255) // 256 * 256


def test_regions_refusals():
    L = _lib.lib()
    assert _regions(0) == (0, (0, 0, 0))
    assert _regions(-1) == (-1, (7, 7, 7))
    assert _regions((1 << 24) + 1) == (-3, (7, 7, 7))
    a = ctypes.c_size_t()
    assert L.nbd_tree_regions(64, None, a, a) == -1 and L.nbd_tree_regions(64, a, None, a) == -1
    assert L.nbd_tree_regions(64, a, a, None) == -1 and L.nbd_tree_regions(64, None, None, None) == -1
    from nbd import tree
    with pytest.raises(_lib.NbdUnsupported):
        tree.views(None, (1 << 24) + 1)


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_keys_f32_against_the_fp64_morton_order(name):
    """How far the fp32 keys are from the fp64 ones: the bodies whose place differs are reported, equality is not asked
    for. What is asked: both are permutations, the fp32 keys are sorted along their own order with ties in index order."""
    p = to.case(name)[0]
    o32, o64 = tbo.order_f32(p), to.morton_order(p)
    moved = np.flatnonzero(o32 != o64)
    print(f"{name}: {len(moved)} of {len(p)} sorted positions hold another body than under the fp64 keys: {moved[:16].tolist()}")
    assert sorted(o32.tolist()) == sorted(o64.tolist()) == list(range(len(p)))
    k = tbo.keys_f32(p)[o32]
    assert (np.diff(k.astype(np.int64)) >= 0).all() and (np.diff(o32)[np.diff(k.astype(np.int64)) == 0] > 0).all()
    if name == "D":                            # 16 copies of a body share a key (65 bodies, one of them cut in two by the
        assert len(np.unique(k)) <= 66         # shift of the second half): the tie order is the index order


def test_keys_f32_edges():
    assert (tbo.keys_f32(tbo.inputs("point")[0]) == 0).all()
    assert tbo.order_f32(tbo.inputs("point")[0]).tolist() == list(range(100))
    p = tbo.inputs("faces")[0]
    k = tbo.keys_f32(p)
    top = (1 << 63) - 1                                            # all 63 bits: cell 2^21 - 1 on every axis
    assert int(k[3]) == top and int(k[4]) == 0 and tbo.order_f32(p)[-1] == 3 and tbo.order_f32(p)[0] == 4
    for body, shift in ((0, 2), (1, 1), (2, 0)):                   # the maximum face of one axis: every bit of that axis
        assert int(k[body]) >> shift & 0x1249249249249249 == 0x1249249249249249
    p = tbo.inputs("nan")[0]
    assert int(tbo.keys_f32(p)[37]) >> 1 & 0x1249249249249249 == 0  # the NaN coordinate: cell 0 on its axis
    assert sorted(tbo.order_f32(p).tolist()) == list(range(100))
    assert len(tbo.keys_f32(np.zeros((0, 3)))) == 0


def test_outlier_ties_most_keys():
    """One body at 1e6 makes a cell of the 21-bit grid 2e6 / 2^21 = 0.95 wide: most bodies of the unit-sized cluster share
    their key with another, and only the stable sort's index order separates them."""
    p = tbo.inputs("outlier")[0]
    _, inverse, counts = np.unique(tbo.keys_f32(p), return_inverse=True, return_counts=True)
    tied = int((counts[inverse] > 1).sum())
    print(f"outlier: {len(counts)} distinct keys among {len(p)} bodies, {tied} bodies share theirs, the largest tie {counts.max()}")
    assert tied > len(p) // 2 and tbo.order_f32(p)[-1] == 999


def test_groups_and_cond_are_additions():
    """groups= returns the rows and counters the full walk gives those groups; cond= changes no row and bounds it."""
    p, m = tbo.inputs("masses")
    full, counters = to.tree_accel(p, m, 0.5, to.SOFTENING)
    again, counters2, S = to.tree_accel(p, m, 0.5, to.SOFTENING, cond=True)
    assert np.array_equal(full, again) and counters == counters2
    assert S.shape == (1000, 2) and (np.linalg.norm(full, axis=1) <= S.sum(1) * (1 + 1e-12)).all() and (S.sum(1) > 0).all()
    order = to.morton_order(p)
    picked = [15, 0, 7]                                            # 15: the ragged last group (40 bodies)
    rows, per_group, S_rows = to.tree_accel(p, m, 0.5, to.SOFTENING, groups=picked, cond=True)
    idx = np.concatenate([order[64 * g:64 * g + 64] for g in picked])
    assert rows.shape == (64 + 64 + 40, 3) and np.array_equal(rows, full[idx]) and np.array_equal(S_rows, S[idx])
    every = to.tree_accel(p, m, 0.5, to.SOFTENING, groups=range(16))[1]
    assert tuple(np.sum(every, axis=0)) == counters and [every[g] for g in picked] == per_group
    phi, phi_counters = tpo.tree_potential(p, m, 0.5, to.SOFTENING)
    phi_rows, phi_groups = tpo.tree_potential(p, m, 0.5, to.SOFTENING, groups=picked)
    assert np.array_equal(phi_rows, phi[idx]) and phi_groups == per_group and phi_counters == counters
    assert to.tree_accel(p[:0], m[:0], 0.5, 0.1, groups=[], cond=True)[1] == []


@pytest.mark.parametrize("theta", tbo.THETAS)
@pytest.mark.parametrize("name", tbo.WALKED)
def test_float32_opening_test_decides_exactly_like_float64(name, theta):
    """On these inputs no decision flips: the GPU tests ask for EQUAL counters, with no allowance for flips."""
    p, m = tbo.inputs(name)
    order = tbo.order_f32(p)
    a64, c64 = to.tree_accel(p, m, theta, to.SOFTENING, order=order)
    a32, c32 = to.tree_accel(p, m, theta, to.SOFTENING, order=order, opening_dtype=np.float32)
    assert c32 == c64 and np.array_equal(a32, a64)


def test_float32_opening_test_decides_exactly_like_float64_on_deep():
    p, m = tbo.inputs("deep")
    order, groups = tbo.order_f32(p), tbo.deep_groups()
    assert len(groups) == 24 and len(set(groups)) == 24 and groups[:2] == [0, 516] and to.plan(len(p))[2] == [4129, 517, 65, 9, 2, 1]
    a64, c64 = to.tree_accel(p, m, 0.5, to.SOFTENING, order=order, groups=groups)
    a32, c32 = to.tree_accel(p, m, 0.5, to.SOFTENING, order=order, groups=groups, opening_dtype=np.float32)
    assert c32 == c64 and np.array_equal(a32, a64) and len(a64) == 23 * 64 + 1
    # cells are accepted above, at and below the level the waves divide the tree at: some group accepts many
    assert max(c for c, _ in c64) > 100 and min(l for _, l in c64) > 0


@pytest.mark.parametrize("name", tbo.WALKED + ["n513", "point", "D"])
def test_node_tolerances(name):
    p, m = tbo.inputs(name)
    order = tbo.order_f32(p)
    x, w = p[order].astype(np.float64), m[order].astype(np.float64)
    tol = tbo.node_tolerances(x, w, tbo.box_f32(p)[3])
    ref = to.build_nodes(x, w)
    assert len(tol) == len(ref) == to.plan(len(p))[0]
    massless_nodes = 0
    for T, L in zip(tol, ref):
        for k in ("M", "c", "s", "Q"):
            assert np.isfinite(T[k]).all() and T[k].shape == L[k].shape[:T[k].ndim] and (T[k] >= 0).all()
        massless = L["M"] == 0
        massless_nodes += int(massless.sum())
        assert (T["M"][massless] == 0).all() and (T["Q"][massless] == 0).all()
        assert (T["M"][~massless] > 0).all()
        if name != "point":                    # (at one point R = 0 and Q = 0: nothing to allow for)
            assert (T["Q"][~massless] > 0).all() and (T["c"] > 0).any() and (T["s"] > 0).all()
        # a bound of the roundings, far below the quantities themselves
        assert (T["s"] <= 1e-6 * np.maximum(L["s"], np.abs(L["c"]).max(1)) + 1e-30).all()
    if name == "masses":
        assert massless_nodes >= 5             # the 40 massless bodies of the corner: whole level-0 nodes without mass
