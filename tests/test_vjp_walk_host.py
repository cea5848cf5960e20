"""The helper of the chunk-edge and long-walk tests of the two fp32 force backward kernels (tests/vjp_rows_oracle.py)
without a GPU: its fp64 rows are the project's backward oracles, its float32 yardsticks are fp32 evaluations (finite at
eps = 0) whose chunk order changes the roundings and not the terms, every size of test_vjp_walk_gpu.py still gets from the
launch plan the walk it is listed for (WALKS of test_hermite_walk_host.py, and the entries' workspace sizes, through the
built library), and the GPU test's bars can fail: a yardstick that leaves one chunk of a long walk out misses them."""
import numpy as np
import pytest

import accel_jerk_vjp_oracle as jo
import accel_vjp_oracle as vo
import hermite_rows_oracle as hr
import vjp_rows_oracle as vr
from conftest import global_rel, row_rel
from nbd import _lib
from test_hermite_walk_host import WALKS

G, EPS = 1.0, 0.05
COTS = {"both": (True, True), "alpha": (True, False), "beta": (False, True)}


def _eps2(eps):
    return float(np.float32(eps * eps))


def _plan(n, slabs=None):
    return {"groups": -(-n // hr.GROUP), "slabs": WALKS[n][0] if slabs is None else slabs, "chunks": -(-n // hr.CHUNK)}


# ---------------------------------------------------------------- the fp64 rows
@pytest.mark.parametrize("n", [130, 449])
@pytest.mark.parametrize("eps", [EPS, 0.0])
def test_rows_are_the_projects_oracles(n, eps):
    """All rows in order: the full oracles' bits (they are the row form on 0 .. n - 1). Any rows in any order, more than
    one block: the same values and sums of |terms| to 1e-13 of the sum of |terms| (another blocking of the same
    matrix-vector products). Both cotangents, alpha only, beta only."""
    x, v, m, ca, cj = vr.case(n)
    for t in (x, v, m, ca, cj):
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t)
    eps2 = _eps2(eps)
    rows = np.random.default_rng(n).permutation(n)[:n - 7]
    full = vo.accel_vjp(x, m, ca, 1.3, eps2)
    assert all(np.array_equal(p, q) for p, q in zip(vr.accel_vjp_rows(x, m, ca, 1.3, eps2, np.arange(n)), full))
    got = vr.accel_vjp_rows(x, m, ca, 1.3, eps2, rows)
    for g_, want, terms in zip(got, full, (full[2], full[3]) * 2):
        assert g_.shape == want[rows].shape
        assert np.all(np.abs(g_ - want[rows]) <= 1e-13 * terms[rows])
    for use_a, use_j in COTS.values():
        a, b = (ca if use_a else None), (cj if use_j else None)
        full = jo.accel_jerk_vjp(x, v, m, a, b, 1.3, eps2)
        same = vr.accel_jerk_vjp_rows(x, v, m, a, b, 1.3, eps2, np.arange(n))
        assert all(np.array_equal(p, q) for p, q in zip(same, full))
        got = vr.accel_jerk_vjp_rows(x, v, m, a, b, 1.3, eps2, rows)
        for g_, want, terms in zip(got, full, full[3:] * 2):
            assert g_.shape == want[rows].shape
            assert np.all(np.abs(g_ - want[rows]) <= 1e-13 * terms[rows])
        assert (not full[1].any()) == (b is None)                        # dL/dv comes from beta alone


def test_reduced_row_sample_holds_the_first_and_the_ragged_last_group():
    for n in (5057, 5633, 8385, 11649):
        assert np.array_equal(vr.sample_rows(n), hr.sample_rows(n))
    n = 32193
    rows = vr.sample_rows(n)
    last = (-(-n // 128) - 1) * 128
    assert np.array_equal(rows, np.unique(rows)) and rows.min() == 0 and rows.max() == n - 1
    assert set(range(128)) <= set(rows) and set(range(last, n)) <= set(rows) and 0 < n - last < 128
    assert 16 <= rows.size - 128 - (n - last) <= 32                     # the seeded random rows outside those groups
    assert np.array_equal(rows, vr.sample_rows(n))


# ---------------------------------------------------------------- the yardsticks
def _both(n, eps, rows, plan, cots="both", **kw):
    """[(name, yardstick, fp64 value, sum|terms|)] of the two operations' outputs on `rows`."""
    x, v, m, ca, cj = vr.case(n)
    eps2 = _eps2(eps)
    a, b = (c if use else None for c, use in zip((ca, cj), COTS[cots]))
    out = []
    if a is not None:
        ref = vr.accel_vjp_rows(x, m, a, G, eps2, rows)
        y = vr.yardstick_accel_vjp_rows(x, m, a, G, eps2, rows, plan, **kw)
        out += [("accel " + nm, y[i], ref[i], ref[2 + i]) for i, nm in enumerate(("dL/dx", "dL/dm"))]
    ref = vr.accel_jerk_vjp_rows(x, v, m, a, b, G, eps2, rows)
    y = vr.yardstick_accel_jerk_vjp_rows(x, v, m, a, b, G, eps2, rows, plan, **kw)
    return out + [("jerk " + nm, y[i], ref[i], ref[3 + i]) for i, nm in enumerate(("dL/dx", "dL/dv", "dL/dm"))]


@pytest.mark.parametrize("n,slabs", [(1, 1), (2, 1), (65, 1), (193, 1), (449, 2), (769, 2), (1025, 3), (1025, 7)])
@pytest.mark.parametrize("eps", [EPS, 0.0])
def test_yardsticks_are_float32_evaluations(n, slabs, eps):
    """float32, finite at eps = 0, and an fp32 sum: within 2^-24 sum|terms| times (the longest chain, 32 sources per chunk
    in each of the two sets, + the wave, slab and output additions + at most 40 roundings inside a term) of the fp64 rows
    -- and not fp64 in disguise: above 2^-30 sum|terms| somewhere. Any split gives a value inside the same bound."""
    plan = _plan(n, slabs)
    q, _ = hr.split(plan)
    rows = np.arange(n) if n <= 500 else np.arange(0, n, 4)               # a row's sums do not depend on the other rows
    for cots in COTS:
        for name, y, ref, terms in _both(n, eps, rows, plan, cots):
            assert y.dtype == np.float32 and y.shape == ref.shape and np.isfinite(y).all(), name
            _, f = vr.figures(y, ref, terms)
            assert f <= 32 * (q + 1) + 8 + slabs + 40, (name, n, slabs, eps, cots, f)
            if n == 1 or (cots == "alpha" and name == "jerk dL/dv"):
                assert not y.any() and not ref.any()                     # no partner, or no beta: exact zeros
            elif n >= 65:
                assert f > 2.0 ** -6, (name, f)


@pytest.mark.parametrize("n", [449, 769, 1025])
def test_a_permuted_chunk_order_changes_the_roundings_not_the_terms(n):
    """The same chunks walked in a seeded permuted order: some bits differ, and no component by more than the two
    evaluations' summation errors together -- a changed, lost or doubled term would show at 1 / n of sum|terms|."""
    plan = _plan(n)
    q, _ = hr.split(plan)
    rows = np.arange(0, n, 8)
    perm = np.random.default_rng(n).permutation(plan["chunks"])
    assert not np.array_equal(perm, np.arange(plan["chunks"]))
    bound = 2 * (32 * (q + 1) + 8 + plan["slabs"]) * hr.U24
    for (name, y, _, terms), (_, yp, _, _) in zip(_both(n, EPS, rows, plan), _both(n, EPS, rows, plan, chunk_order=perm)):
        assert not np.array_equal(y, yp), name
        d = np.abs(y.astype(np.float64) - yp)
        print(f"n={n} {name}: permuted order, max |difference| / (2^-24 sum|terms|) = {(d / (hr.U24 * terms)).max():.2f}")
        assert np.all(d <= bound * terms), name
        assert 64.0 / n > 50 * bound                                     # a chunk's share of sum|terms| is far above it


# ---------------------------------------------------------------- the sizes and the plan
def test_the_gpu_test_runs_these_sizes():
    assert sorted(hr.EDGE_SIZES + hr.LONG_SIZES) == sorted(WALKS)
    assert hr.LONG_SIZES == [5057, 5633, 8385, 11649, 32193] and hr.LONG_EPS0 == [5633, 11649]
    assert {128, 192, 193, 256, 257, 448, 449, 513, 705, 769, 1025} <= set(hr.EDGE_SIZES)
    longest = {n: WALKS[n][2] + (1 if WALKS[n][3] else 0) for n in hr.LONG_SIZES}
    assert longest == {5057: 2, 5633: 3, 8385: 3, 11649: 5, 32193: 21}
    assert min(n for n in hr.LONG_SIZES if longest[n] >= 3) == 5633


@pytest.mark.parametrize("n", sorted(WALKS))
def test_workspaces_are_the_layout_of_the_listed_walk(n):
    """The backward entries take the forward force's plan: their workspace sizes are the slab count of WALKS[n] -- a
    retuned plan fails here, by size (then pick sizes with the listed walks, test_hermite_walk_host.py). Acceleration
    backward: float[slabs][4][n]. Jerk backward: float[slabs][7][n] rounded up to a multiple of 4 floats, the acceleration
    backward's workspace, its dL/dx (3 n) and its dL/dm (n)."""
    slabs = WALKS[n][0]
    L = _lib.lib()
    assert L.nbd_accel_vjp_workspace_bytes(n) == slabs * 4 * n * 4
    assert L.nbd_accel_jerk_vjp_workspace_bytes(n) == (-(-slabs * 7 * n // 4) * 4 + slabs * 4 * n + 4 * n) * 4


# ---------------------------------------------------------------- the bars of the GPU test can fail
def _miss(y, ref, terms, yard, with_row):
    """How far the values y miss the sampled-row bars of test_vjp_walk_gpu.py given the yardstick `yard`: the largest
    figure / bar."""
    rr, f = vr.figures(y, ref, terms)
    yr, yf = vr.figures(yard, ref, terms)
    miss = f / (vr.MARGIN * yf) if yf else (float("inf") if f else 0.0)
    return max(miss, rr / max(vr.ROW_BAR, vr.MARGIN * yr)) if with_row else miss


@pytest.mark.parametrize("n", [5633, 11649])
def test_a_dropped_third_chunk_misses_the_sampled_row_bars(n):
    """Wave 0 walks three chunks or more at both sizes (5633: exactly three); its third chunk (sources 128 .. 191), the
    first one that lands in the refilled buffer 0, is left out of the yardstick. That must miss the bars by 10 x or more on
    at least one output of each operation."""
    slabs, _, q, r = WALKS[n]
    assert q + (1 if r else 0) >= 3 and (n != 5633 or (q, r > 0) == (2, True))
    rows = vr.sample_rows(n)[::8]
    good, bad = _both(n, EPS, rows, _plan(n)), _both(n, EPS, rows, _plan(n), drop_chunk=2)
    worst = {"accel": 0.0, "jerk": 0.0}
    for (name, y, ref, terms), (_, yd, _, _) in zip(good, bad):
        miss = _miss(yd, ref, terms, y, "dL/dm" not in name)
        print(f"n={n} {name}: a dropped chunk misses the bars by a factor {miss:.3g}")
        worst[name.split()[0]] = max(worst[name.split()[0]], miss)
    assert worst["accel"] >= 10 and worst["jerk"] >= 10, worst


def test_the_net_bars_are_a_quarter_of_a_dropped_chunk_at_most():
    """n = 32193, where a chunk is the smallest share of a row (64 / n of sum|terms|): the shift one dropped chunk causes,
    in the net's own measures (row_rel of dL/dx and dL/dv, global_rel of dL/dm) on 24 rows, is more than four times every
    net bar."""
    n = 32193
    rows = vr.sample_rows(n)[::8][:24]
    good, bad = _both(n, EPS, rows, _plan(n)), _both(n, EPS, rows, _plan(n), drop_chunk=2)
    bars = dict(zip(("accel dL/dx", "accel dL/dm", "jerk dL/dx", "jerk dL/dv", "jerk dL/dm"), vr.NET_ACCEL + vr.NET_JERK))
    for (name, y, _, _), (_, yd, _, _) in zip(good, bad):
        shift = global_rel(yd, y) if "dL/dm" in name else row_rel(yd, y)
        print(f"n={n} {name}: a dropped chunk shifts by {shift:.2e}, the net bar is {bars[name]:.0e}")
        assert bars[name] < shift / 4, (name, shift, bars[name])
