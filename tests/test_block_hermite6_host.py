"""BlockHermite6Simulator without a GPU: the block oracle (tests/block_hermite6_oracle.py) is the shared 6th-order oracle
at max_level 0, its criterion's derivative formulas are those of a quintic, the fixtures of test_block_hermite6_gpu.py are
pinned on the CPU (their criterion values keep clear of every level boundary by a thousand times what a permutation of
the bodies moves them, so the GPU must choose the oracle's levels), the eccentric orbit shows what the order buys, and the
refusals of the class and of the new C-ABI entries come before any device work."""
import ctypes
import re
import os

import numpy as np
import pytest
import torch

import block_hermite6_cases as c6
import block_hermite6_oracle as b6
import block_hermite_f64_cases as bc
import hermite6_oracle as h6
import hermite_f64_oracle as fo
from conftest import ROOT
from nbd import _lib

ENTRIES = ("nbd_hblock6_f64_workspace_bytes", "nbd_hblock6_predict_f64", "nbd_hblock6_force_f64",
           "nbd_hblock6_correct_f64", "nbd_hblock6_step_f64", "nbd_accel_jerk_snap_active_f64")

# measured on the CPU (the printed figures): {(eps, output steps): margin}; the floors below are half of them
MARGINS = {(0.0, 1): 1.259e-4, (0.0, 4): 8.554e-5, (0.01, 1): 7.836e-4, (0.01, 4): 3.102e-4}
# {eta: (orbit error, pair interactions)} of the e = 0.9 orbit at max_level 16
ORBIT = {0.01: (9.396e-11, 1984), 0.0025: (1.5005e-12, 3968)}


@pytest.mark.parametrize("n", [1, 2, 65])
def test_max_level_zero_is_the_shared_oracle_bit_for_bit(n):
    x, v, m = fo.plummer_case(n, seed=260 + n)
    got = b6.block6_run(x, v, m, 0.01, 1.0, 0.05 ** 2, 3, eta=0.02, max_level=0)
    want = h6.hermite6_run(x, v, m, 0.01, 1.0, 0.05 ** 2, 3)
    for key, ref in zip("xvajsc", want):
        assert np.array_equal(got[key], ref), (n, key)
    assert got["block_steps"] == 3 and got["pair_interactions"] == 3 * n * n and got["levels"].max() == 0


def test_criterion_derivatives_are_those_of_a_quintic():
    """a(t) a random quintic per component, sampled (a, j, s) at t0 and t1 = t0 + h: a3(t1), a4(t1) and a5 of the oracle
    against numpy.polynomial's derivatives, to 1e-9 relative (of the largest component). The steps are of order one:
    the formulas divide differences of O(1) samples by h^4 and h^5, so fp64 rounding alone is ~720 * 2^-53 / h^5 of a
    coefficient -- 1e-13 at h = 1/2, and past the 1e-9 of this check below h ~ 1/16, whatever the formula."""
    rng = np.random.default_rng(6)
    for h in (0.5, 0.25, 1.7):
        t0 = rng.uniform(-1, 1)
        polys = [[np.polynomial.Polynomial(rng.uniform(-1, 1, 6)) for _ in range(3)] for _ in range(5)]

        def at(t, order):
            return np.array([[p.deriv(order)(t) if order else p(t) for p in row] for row in polys])
        ends = [at(t, k) for t in (t0, t0 + h) for k in (0, 1, 2)]
        got = b6.derivatives(*ends, np.full(5, h))
        for order, g in zip((3, 4, 5), got):
            ref = at(t0 + h, order)
            assert np.abs(g - ref).max() <= 1e-9 * np.abs(ref).max(), (h, order)
        assert np.array_equal(got[0], h6.crackle(*ends, h))           # a3(t1) is the crackle the corrector forms


@pytest.mark.parametrize("eps", [0.0, 0.01])
def test_fixture_margins_and_permuted_level_histories(eps):
    """dt = 1/32, eta = 0.02, max_level 10, seeds block_hermite6_cases.PLANTED. Measured: margin 1.26e-4 (eps = 0) /
    7.84e-4 (eps = 0.01) over one output step, 8.55e-5 / 3.10e-4 over four; the three permutations move the margin by at
    most 1.1e-8 / 1.1e-9 resp. 1.5e-8 / 2.7e-8, keep every level history, and nothing is clamped; the deepest level is 9."""
    for steps in (1, 4):
        ref = c6.planted_run(eps, steps)
        assert ref["clamped"] == 0
        shift = 0.0
        for seed in c6.PERM_SEEDS:
            prm = c6.planted_run_permuted(eps, steps, seed)
            assert prm["clamped"] == 0
            assert prm["block_steps"] == ref["block_steps"] and prm["pair_interactions"] == ref["pair_interactions"]
            assert len(prm["history"]) == len(ref["history"])
            assert all(np.array_equal(a, b) for a, b in zip(prm["history"], ref["history"])), (eps, steps, seed)
            shift = max(shift, abs(prm["margin"] - ref["margin"]))
        print(f"eps={eps} steps={steps}: margin {ref['margin']:.4e}, largest shift {shift:.3e}, deepest level "
              f"{max(h.max() for h in ref['history'])}, {ref['block_steps']} block steps")
        assert ref["margin"] >= 1000 * shift, (eps, steps, ref["margin"], shift)
        assert ref["margin"] >= 0.5 * MARGINS[eps, steps], (eps, steps, ref["margin"])
    x, v, m = c6.planted(eps)
    for a in (x, v, m):
        assert not np.any(a.astype(np.float32).astype(np.float64) == a)
    assert ref["levels"][:2].min() > np.median(ref["levels"])           # the binary runs deeper than the median body


def test_the_order_pays_on_the_eccentric_orbit():
    """e = 0.9, eps = 0, one period as 4 output steps, max_level 16. Measured: eta = 0.01 -> 9.396e-11 at 1 984 pair
    interactions, eta = 0.0025 -> 1.5005e-12 at 3 968; the 4th-order block oracle at its eta = 0.000625: 5.07e-9 at
    5 668 (54 times the error at 2.9 times the pairs)."""
    for eta, (err, pairs) in ORBIT.items():
        r = c6.orbit_run(eta)
        print(f"eta={eta}: err {r['err']:.4e}, {r['pair_interactions']} pairs, margin {r['margin']:.3e}")
        assert r["clamped"] == 0 and r["levels"].max() <= c6.ORBIT_K
        assert r["pair_interactions"] == pairs
        assert abs(r["err"] - err) <= 0.01 * err, (eta, r["err"])
    six, four = c6.orbit_run(0.01), bc.orbit_run()
    assert 10 * six["err"] <= four["err"], (six["err"], four["err"])
    assert six["pair_interactions"] < four["pair_interactions"]


def test_refusals_come_before_any_device_work():
    from galaxify import simulation
    cls = simulation.BlockHermite6Simulator
    z = np.zeros((4, 3))
    kw = dict(positions=z, velocities=z, masses=np.ones(4), device="cpu")
    for bad in (torch.float32, torch.float16, "float64", None):
        with pytest.raises(ValueError, match="dtype"):
            cls(dtype=bad, **kw)
    with pytest.raises(ValueError, match="process_group"):
        cls(process_group=object(), **kw)
    with pytest.raises(ValueError, match="process_group"):
        cls(dtype=torch.float64, process_group=object(), **kw)
    with pytest.raises(TypeError, match="no_such_keyword"):
        cls(no_such_keyword=1, **kw)
    with pytest.raises(RuntimeError, match="cpu"):               # with everything in order, the project's usual rule
        cls(**kw)
    assert issubclass(cls, simulation.Hermite6Simulator) and not issubclass(cls, simulation.BlockHermiteSimulator)
    block = simulation.BlockHermiteSimulator
    for name in ("step", "_set_levels", "_check_params", "_read_clamped", "MAX_LEVEL_LIMIT"):     # one copy of the loop
        assert getattr(cls, name) is getattr(block, name), name
    assert cls.MAX_LEVEL_LIMIT == 20 and not cls._capturable()
    for name in ("run", "compute_energies", "compute_invariants", "compute_accelerations_jerks_and_snaps"):
        assert getattr(cls, name) is getattr(simulation.Hermite6Simulator, name), name
    sim = object.__new__(cls)
    sim.dt, sim.eta, sim.max_level = 0.01, 0.02, 21
    with pytest.raises(ValueError, match="BlockHermite6Simulator: max_level"):
        sim._check_params()
    sim.max_level, sim.eta = 4, 0.0
    with pytest.raises(ValueError, match="BlockHermite6Simulator: dt and eta"):
        sim._check_params()
    old = object.__new__(block)
    old.dt, old.eta, old.max_level = 0.01, 0.02, -1
    with pytest.raises(ValueError, match=r"BlockHermiteSimulator: max_level must be an int in \[0, 20\]"):
        old._check_params()


def test_new_symbols_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbd.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared in include/nbd.h"
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert L.nbd_abi_version() == _lib.ABI_VERSION == 2          # entries were added, nothing else changed


def _plan_slabs(n, n_act):
    """The plan of n_act targets under n sources, restated: ~1024 workgroups, every wave keeps a chunk, at most 64 slabs."""
    groups, chunks = -(-n_act // 64), -(-n // 64)
    return max(1, min(-(-1024 // groups), chunks // 4, 64))


def test_workspace_sizes_without_a_gpu():
    L = _lib.lib()
    assert L.nbd_hblock6_f64_workspace_bytes(0) == 0 and L.nbd_hblock6_f64_workspace_bytes(-3) == 0
    for n in (1, 2, 63, 64, 65, 130, 449, 1000, 5000):
        act = -(-n // 8) * 32                                    # the list, padded so that the slab part is 32-byte aligned
        most = max(_plan_slabs(n, n_act) * n_act for n_act in range(1, n + 1))
        assert L.nbd_hblock6_f64_workspace_bytes(n) == act + most * 9 * 8, n
        assert L.nbd_hblock6_f64_workspace_bytes(n) >= act + L.nbd_hermite6_f64_workspace_bytes(n)


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    L = _lib.lib()
    n = 100
    ws_n = L.nbd_hblock6_f64_workspace_bytes(n)
    fake = ctypes.c_void_p(1 << 20)                     # never dereferenced: every call below fails its host checks
    odd = ctypes.c_void_p((1 << 20) + 16)               # 16-byte aligned only: rows and workspace need 32
    f8, f9 = [fake] * 8, [fake] * 9
    predict, force, correct = L.nbd_hblock6_predict_f64, L.nbd_hblock6_force_f64, L.nbd_hblock6_correct_f64
    step, active = L.nbd_hblock6_step_f64, L.nbd_accel_jerk_snap_active_f64
    assert predict(*f8, -1, 4, 0.1, fake, fake, fake, fake, None) == -1
    assert predict(*f8, n, 21, 0.1, fake, fake, fake, fake, None) == -1
    assert predict(*f8, n, -1, 0.1, fake, fake, fake, fake, None) == -1
    assert predict(*f8, n, 4, 0.0, fake, fake, fake, fake, None) == -1
    assert predict(*([None] * 8), n, 4, 0.1, None, None, None, None, None) == -1
    assert predict(*[fake] * 5, None, fake, fake, n, 4, 0.1, fake, fake, fake, fake, None) == -1      # no crackle
    assert predict(*f8, n, 4, 0.1, fake, fake, fake, odd, None) == -1
    assert force(fake, fake, fake, -1, 0, 0.01, fake, ws_n, None) == -1
    assert force(fake, fake, fake, n, n + 1, 0.01, fake, ws_n, None) == -1             # n_act > n
    assert force(fake, fake, None, n, n, 0.01, fake, ws_n, None) == -1
    assert force(fake, fake, odd, n, n, 0.01, fake, ws_n, None) == -1
    assert force(fake, fake, fake, n, n, 0.01, fake, 64, None) == -2
    assert force(fake, fake, fake, n, n, 0.01, odd, ws_n, None) == -2
    assert force(fake, fake, fake, n, 0, 0.01, fake, ws_n, None) == 0                  # nothing listed: a no-op
    assert correct(*f9, -1, 0, 4, 0.1, 0.02, 1.0, fake, fake, fake, ws_n, None) == -1
    assert correct(*f9, n, n + 1, 4, 0.1, 0.02, 1.0, fake, fake, fake, ws_n, None) == -1
    assert correct(*f9, n, n, 21, 0.1, 0.02, 1.0, fake, fake, fake, ws_n, None) == -1
    assert correct(*f9, n, n, 4, 0.1, 0.0, 1.0, fake, fake, fake, ws_n, None) == -1
    assert correct(*[fake] * 4, None, *[fake] * 4, n, n, 4, 0.1, 0.02, 1.0, fake, fake, fake, ws_n, None) == -1     # no snap
    assert correct(*f9, n, n, 4, 0.1, 0.02, 1.0, fake, odd, fake, ws_n, None) == -1
    assert correct(*f9, n, n, 4, 0.1, 0.02, 1.0, fake, fake, None, ws_n, None) == -2
    assert correct(*f9, n, 0, 4, 0.1, 0.02, 1.0, fake, fake, fake, ws_n, None) == 0
    tail = (fake, fake, fake, fake, fake, ws_n, None)                                  # sched, posd, veld, accd, workspace
    assert step(*f9, -1, 1, 4, 0.1, 0.02, 0.01, 1.0, *tail) == -1
    assert step(*f9, n, 0, 4, 0.1, 0.02, 0.01, 1.0, *tail) == -1                       # nothing active
    assert step(*f9, n, n, 21, 0.1, 0.02, 0.01, 1.0, *tail) == -1
    assert step(*([None] * 9), n, n, 4, 0.1, 0.02, 0.01, 1.0, *tail) == -1
    assert step(*f9, n, n, 4, 0.1, 0.02, 0.01, 1.0, fake, fake, fake, odd, fake, ws_n, None) == -1
    assert step(*f9, n, n, 4, 0.1, 0.02, 0.01, 1.0, fake, fake, fake, None, fake, ws_n, None) == -1
    assert step(*f9, n, n, 4, 0.1, 0.02, 0.01, 1.0, fake, fake, fake, fake, fake, 64, None) == -2     # before the predictor
    out = (fake, fake, fake)
    assert active(fake, fake, fake, -1, fake, 0, 0.01, 1.0, *out, fake, ws_n, 0, None) == -1
    assert active(fake, fake, fake, n, fake, n + 1, 0.01, 1.0, *out, fake, ws_n, 0, None) == -1
    assert active(fake, fake, fake, n, None, 5, 0.01, 1.0, *out, fake, ws_n, 0, None) == -1
    assert active(fake, fake, None, n, fake, 5, 0.01, 1.0, *out, fake, ws_n, 0, None) == -1
    assert active(fake, fake, fake, n, fake, 5, 0.01, 1.0, fake, fake, None, fake, ws_n, 0, None) == -1
    assert active(fake, fake, fake, n, fake, 5, 0.01, 1.0, *out, fake, ws_n, 65, None) == -1
    assert active(fake, fake, fake, n, fake, 5, 0.01, 1.0, *out, fake, ws_n, -1, None) == -1
    assert active(fake, fake, fake, n, fake, 5, 0.01, 1.0, *out, fake, 64, 0, None) == -2
    assert active(fake, fake, fake, n, fake, 5, 0.01, 1.0, *out, fake, 416 + 2 * 9 * 5 * 8 - 1, 2, None) == -2
    assert active(None, None, None, n, None, 0, 0.01, 1.0, None, None, None, None, 0, 0, None) == 0
