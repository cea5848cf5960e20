"""The helper of the chunk-edge and long-walk tests of the fp32 Hermite force (tests/hermite_rows_oracle.py) without a
GPU: its fp64 rows are the project's oracles, its float32 yardstick is an fp32 evaluation (and finite at eps = 0), the row
sample holds the ragged last group, and every size of test_hermite_walk_gpu.py still gets from the launch plan
(nbd_accel_plan, through the built library) the chunk walk it is listed for."""
import ctypes

import numpy as np
import pytest

import hermite_f64_oracle as fo
import hermite_oracle as ho
import hermite_rows_oracle as hr
from nbd import _lib

# n: (slabs, chunks, q, r) -- every wave walks q chunks of 64 sources, the first r of the 4 x slabs waves one more.
# What each size is in the GPU test for:
WALKS = {
    1: (1, 1, 0, 1), 2: (1, 1, 0, 1), 63: (1, 1, 0, 1), 64: (1, 1, 0, 1),      # one chunk, three idle waves
    65: (1, 2, 0, 2), 127: (1, 2, 0, 2), 128: (1, 2, 0, 2),                    # two chunks, two idle waves
    129: (1, 3, 0, 3), 192: (1, 3, 0, 3),                                      # a second group; three chunks, one idle wave
    193: (1, 4, 1, 0), 256: (1, 4, 1, 0),                                      # four chunks, q = 1
    257: (1, 5, 1, 1), 448: (1, 7, 1, 3),                                      # the last one-slab size
    449: (2, 8, 1, 0), 513: (2, 9, 1, 1),                                      # two slabs
    705: (3, 12, 1, 0),                                                        # three slabs
    769: (2, 13, 1, 5), 1025: (3, 17, 1, 5),                                   # ragged splits: a slab of two-chunk waves
    5057: (10, 80, 2, 0),                                                      # every wave walks exactly two chunks
    5633: (9, 89, 2, 17),                                                      # 17 waves walk three: buffer 0 refilled
    8385: (11, 132, 3, 0),
    11649: (11, 183, 4, 7),
    32193: (6, 504, 21, 0),                                                    # the longest chains below the large-N plan
}
G, EPS = 1.0, 0.05


def _accel_plan(n_src, n_tgt):
    g, s, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert _lib.lib().nbd_accel_plan(n_src, n_tgt, g, s, c) == 0
    return {"groups": g.value, "slabs": s.value, "chunks_per_wave": c.value}


@pytest.mark.parametrize("n", sorted(WALKS))
def test_every_size_still_gets_the_walk_it_is_listed_for(n):
    """A retuned plan fails here, by size: pick another size with the listed walk (and update WALKS and the GPU test's
    lists together) -- the GPU test must never silently lose its long walks."""
    ap = _accel_plan(n, n)
    plan = hr.chunk_plan(n, ap)
    slabs, chunks, q, r = WALKS[n]
    assert (plan["slabs"], plan["chunks"]) + hr.split(plan) == (slabs, chunks, q, r), (n, plan, hr.split(plan))
    assert plan["groups"] == -(-n // hr.GROUP)
    assert ap["chunks_per_wave"] == q + (1 if r else 0)                # the library's own longest walk


def test_the_gpu_test_runs_these_sizes():
    assert sorted(hr.EDGE_SIZES + hr.LONG_SIZES) == sorted(WALKS)
    assert all(n <= 1100 for n in hr.EDGE_SIZES) and all(n > 1100 for n in hr.LONG_SIZES)
    longest = {n: WALKS[n][2] + (1 if WALKS[n][3] else 0) for n in hr.LONG_SIZES}
    assert sorted(longest.values()) == [2, 3, 3, 5, 21]
    assert set(hr.STEP_SIZES) <= set(hr.LONG_SIZES) and all(longest[n] >= 3 for n in hr.STEP_SIZES)
    assert set(hr.PINNED_SCENES) <= set(WALKS) and hr.ACTIVE_N in WALKS


def test_active_plan_is_the_entrys_workspace_check():
    """active_plan restates plan_active (csrc/direct_hermite_block.hip): the entry accepts a workspace of exactly the bytes
    it gives and refuses one float less (the argument checks run before any GPU call)."""
    n, n_act = 5633, 130
    plan = hr.active_plan(n, n_act, _accel_plan(n, n_act))
    assert plan["slabs"] == 22 and hr.split(plan) == (1, 1)
    assert plan["slabs"] != hr.chunk_plan(n, _accel_plan(n, n))["slabs"]            # another split of the same chunks
    need = -(-n // 4) * 16 + plan["slabs"] * 6 * n_act * 4
    L = _lib.lib()
    args = (0x1000, 0x2000, n, 0x3000, n_act, 0.0025, 1.0, 0x4000, 0x5000, 0x6000)
    assert L.nbd_accel_jerk_active_f32(*args, need - 4, None) == -2
    assert hr.active_plan(n, n, _accel_plan(n, n)) == hr.chunk_plan(n, _accel_plan(n, n))      # all bodies: the shared plan


@pytest.mark.parametrize("n", [130, 449])
@pytest.mark.parametrize("eps", [EPS, 0.0])
def test_rows_are_the_projects_oracles(n, eps):
    x, v, m = hr.case(n)
    for t in (x, v, m):
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t)
    eps2 = float(np.float32(eps * eps))
    a, j = ho.accel_jerk(x, v, m, 1.3, eps2)
    sa, sj = fo.accel_jerk_abs(x, v, m, 1.3, eps2)
    rows = np.random.default_rng(n).permutation(n)[:n - 7]             # any rows, any order, more than one block
    got = hr.accel_jerk_rows(x, v, m, 1.3, eps2, rows)
    for g_, want, terms in zip(got, (a, j, sa, sj), (sa, sj, sa, sj)):
        assert g_.shape == (rows.size, 3)
        assert np.all(np.abs(g_ - want[rows]) <= 1e-13 * terms[rows])          # relative to the sum of |terms|, by component


@pytest.mark.parametrize("n,slabs", [(2, 1), (65, 1), (193, 1), (449, 2), (769, 2), (1025, 3), (1025, 7)])
@pytest.mark.parametrize("eps", [EPS, 0.0])
def test_yardstick_is_a_float32_evaluation(n, slabs, eps):
    """Finite at eps = 0; an fp32 sum: within 2^-24 sum|terms| times (the longest chain + a few roundings per term) of the
    fp64 rows -- and not fp64 in disguise: its error is above 2^-30 sum|terms| somewhere. Any split gives a value inside
    the same bound."""
    x, v, m = hr.case(n)
    eps2 = float(np.float32(eps * eps))
    rows = hr.sample_rows(n)
    assert rows.size == n
    a, j, sa, sj = hr.accel_jerk_rows(x, v, m, G, eps2, rows)
    plan = {"groups": -(-n // 128), "slabs": slabs, "chunks": -(-n // 64)}
    ya, yj = hr.yardstick_rows(x, v, m, G, eps2, rows, plan)
    assert ya.dtype == np.float32 and yj.dtype == np.float32 and ya.shape == (n, 3) and yj.shape == (n, 3)
    assert np.isfinite(ya).all() and np.isfinite(yj).all()
    q, r = hr.split(plan)
    chain = 64 * (q + 1) + 4 + slabs
    for got, ref, sm, per_term in ((ya, a, sa, 8), (yj, j, sj, 14)):
        rr, f = hr.figures(got, ref, sm)
        assert f <= chain + per_term, (n, slabs, eps, f)
        assert n < 65 or f > 2.0 ** -6
        assert rr < 1e-4


def test_yardstick_split_changes_the_order_not_the_terms():
    """One slab against three at n = 1025: different roundings (some bits differ) of the same sum (both inside the bound
    above, and within 2^-24 sum|terms| x the chain length of each other)."""
    n = 1025
    x, v, m = hr.case(n)
    eps2 = float(np.float32(EPS * EPS))
    rows = np.arange(0, n, 8)
    _, _, sa, sj = hr.accel_jerk_rows(x, v, m, G, eps2, rows)
    one = hr.yardstick_rows(x, v, m, G, eps2, rows, {"groups": 9, "slabs": 1, "chunks": 17})
    three = hr.yardstick_rows(x, v, m, G, eps2, rows, {"groups": 9, "slabs": 3, "chunks": 17})
    for p, q_, sm in zip(one, three, (sa, sj)):
        assert not np.array_equal(p, q_)
        assert np.all(np.abs(p.astype(np.float64) - q_) <= 5 * 64 * hr.U24 * sm)


def test_yardstick_drops_nothing_and_adds_nothing():
    """A source moved past the end of its wave's walk would be lost: the sum over one slab of a system whose last chunk
    holds a single heavy body far away sees that body."""
    n = 193
    x, v, m = hr.case(n)
    m = m.copy(); m[-1] = 1.0
    eps2 = float(np.float32(EPS * EPS))
    rows = np.arange(n)
    a, j, sa, sj = hr.accel_jerk_rows(x, v, m, G, eps2, rows)
    ya, yj = hr.yardstick_rows(x, v, m, G, eps2, rows, {"groups": 2, "slabs": 1, "chunks": 4})
    assert hr.figures(ya, a, sa)[1] < 80 and hr.figures(yj, j, sj)[1] < 80
    m[-1] = 0.0
    a0 = hr.accel_jerk_rows(x, v, m, G, eps2, rows)[0]
    assert hr.figures(ya, a0, sa)[1] > 1e4                             # the heavy body matters at this scale


def test_row_sample_holds_the_ragged_last_group():
    for n in (5057, 5633, 8385, 11649, 32193):
        rows = hr.sample_rows(n)
        last = (-(-n // 128) - 1) * 128
        mid = (-(-n // 128) // 2) * 128
        assert np.array_equal(rows, np.unique(rows)) and rows.min() == 0 and rows.max() == n - 1
        assert set(range(last, n)) <= set(rows) and n - last < 128                     # ragged, and whole
        assert set(range(128)) <= set(rows) and set(range(mid, mid + 128)) <= set(rows)
        extra = rows.size - 256 - (n - last)
        assert 32 <= extra <= 64                                       # the seeded random rows outside those groups
        assert np.array_equal(rows, hr.sample_rows(n))
    assert np.array_equal(hr.sample_rows(1025), np.arange(1025))


def test_figures():
    ref = np.array([[1.0, 2.0, 0.0]])
    sm = np.array([[4.0, 4.0, 0.0]])
    rr, f = hr.figures(ref + np.array([[0.0, 4 * hr.U24 * 3, 0.0]]), ref, sm)
    assert f == pytest.approx(3.0) and rr == pytest.approx(12 * hr.U24 / np.sqrt(5.0))
    assert hr.figures(ref + np.array([[0.0, 0.0, 1e-30]]), ref, sm)[1] == float("inf")     # no terms: exact
    assert hr.figures(np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 3))) == (0.0, 0.0)
    assert hr.figures(np.array([[np.nan, 2.0, 0.0]]), ref, sm)[1] == float("inf")


def test_predict32_rounds_every_operation():
    rng = np.random.default_rng(3)
    x, v, a, j = (rng.standard_normal((50, 3)).astype(np.float32) for _ in range(4))
    dt = 1.0 / 64
    xp, vp = hr.predict32(x, v, a, j, dt)
    assert xp.dtype == np.float32 and vp.dtype == np.float32
    x64 = x.astype(np.float64) + v * dt + a * (dt * dt / 2) + j * (dt ** 3 / 6)
    assert np.abs(xp - x64).max() < 4 * 2.0 ** -24 * np.abs(x64).max() + 1e-7
    h = np.float32(dt)
    assert np.array_equal(vp, (v + a * h) + j * np.float32(0.5 * dt * dt))
