"""The symmetric equal-mass force with the slot count read off the workspace it is handed (plan_sym: K = the widest plan
that fits, at most min(M, 64)). With one slot per round (K = M) every round stores and all M (M - 1) / 2 tile pairs go in
ONE launch; with 16 < K < M the first K - 1 rounds store and launches of K rounds add; with the workspace of the existing
queries the plan is the 16-slot one. Through nbd_accel_sym_uniform_f32 (variants 2 and 0) with a workspace of a stated
number of slots: rows against fp64 and against the 16-slot plan at the 2e-6 of the existing tests, run-to-run bit identity,
net momentum, nothing written behind the stated size; the size checks; and one LeapFrogSimulator at n = 65 536 + 37 with
the preferred workspace against NBD_SYM_SLOTS=16."""
import functools

import numpy as np
import pytest
import torch

from conftest import row_rel
from test_direct_sym_gpu import EPS2, _f64_rows, _state, _sym

pytestmark = pytest.mark.gpu

K_PREF = 64          # slots of the preferred step workspace at M >= 64 tiles (kSymSlotsPref of csrc/direct_force.hip)

# (n, slots handed in): M + 1 = 21 (one launch of 190 workgroups, ragged slot stride, remainder slot); 24 + 1 (23 storing
# rounds, then 10 adding ones); 34 + 1 (one launch); M = 2 (wide and narrow plan coincide)
CASES = [(20 * 1024 + 37, 21), (34 * 1024 + 4, 25), (34 * 1024 + 4, 35), (2048, 2)]
GUARD = 4096         # sentinel floats behind the stated workspace size


def _core(n):
    return (n // 1024 & ~1) * 1024


def _sym_ws(posm, n, mass_value, variant, nbytes, expect=0):
    """nbd_accel_sym_uniform_f32 on a workspace of exactly nbytes; the floats behind it must stay untouched."""
    from nbd import _lib
    L = _lib.lib()
    assert nbytes % 4 == 0 or expect != 0
    buf = torch.full(((nbytes + 3) // 4 + GUARD,), 12345.0, dtype=torch.float32, device=posm.device)
    out = torch.empty((n, 3), dtype=torch.float32, device=posm.device)
    rc = L.nbd_accel_sym_uniform_f32(posm.data_ptr(), n, EPS2, 1.0, mass_value, out.data_ptr(), buf.data_ptr(), nbytes,
                                     variant, _lib.current_stream(posm.device))
    assert rc == expect, _lib.lib().nbd_strerror(rc)
    assert bool((buf[(nbytes + 3) // 4:] == 12345.0).all())
    return out if rc == 0 else None


@functools.lru_cache(maxsize=None)
def _case(n):
    """State, sampled rows and their fp64 reference of one size: computed once, shared by the tests, never written."""
    p, m, posm = _state(n, seed=n + 3)
    mv = float(np.float32(m[0]))
    assert np.all(m.astype(np.float32) == np.float32(mv))
    core = _core(n)
    rng = np.random.default_rng(2)
    edges = [0, 63, 64, 511, 512, 1023, 1024, 2047, core - 1024, core - 1, core, n - 1]
    rows = np.unique(np.concatenate([rng.choice(n, 96, replace=False), edges]))
    rows = rows[rows < n]
    for r in (0, 1023, 1024, core - 1, min(core, n - 1), n - 1):
        assert r in rows
    ref = _f64_rows(p, m, rows)
    ref.setflags(write=False)
    return posm, mv, rows, ref


@pytest.mark.parametrize("variant", [2, 0])
@pytest.mark.parametrize("n,slots", CASES)
def test_sym_wide_rows_against_f64_and_16_slot_plan(n, slots, variant, gpu_device):
    posm, mv, rows, ref = _case(n)
    acc = _sym_ws(posm, n, mv, variant, slots * n * 12)
    assert torch.isfinite(acc).all()
    a = acc.cpu().numpy()
    rel64 = row_rel(a[rows], ref)
    print(f"n = {n}, {slots} slots, variant {variant}: against fp64 on {len(rows)} rows, row_rel = {rel64:.3e}")
    assert rel64 < 2e-6
    narrow = _sym(posm, n, mv, variant=variant).cpu().numpy()      # the workspace of the existing query: 16-slot plan
    rel16 = row_rel(a, narrow)
    print(f"n = {n}, {slots} slots, variant {variant}: against the 16-slot plan, row_rel = {rel16:.3e}")
    assert rel16 < 2e-6
    if n == 2048:
        assert np.array_equal(a, narrow)                           # M = 2: one plan, the same bits


@pytest.mark.parametrize("variant", [2, 0])
@pytest.mark.parametrize("n,slots", CASES)
def test_sym_wide_bit_identical_run_to_run_and_momentum(n, slots, variant, gpu_device):
    posm, mv, _, _ = _case(n)
    a1 = _sym_ws(posm, n, mv, variant, slots * n * 12)
    a2 = _sym_ws(posm, n, mv, variant, slots * n * 12)
    assert torch.equal(a1, a2)
    acc = a1.cpu().numpy().astype(np.float64)
    net = acc.sum(0)
    print(f"n = {n}, {slots} slots, variant {variant}: net / sum |a| = {np.abs(net).max() / np.abs(acc).sum(0).max():.3e}")
    assert np.abs(net).max() < 1e-6 * np.abs(acc).sum(0).max()


def test_sym_wide_workspace_sizes(gpu_device):
    from nbd import _lib
    L = _lib.lib()
    # the existing queries keep their values: every caller that allocates by them gets the 16-slot plan
    assert L.nbd_step_workspace_bytes(65536) == 16 * 65536 * 12
    assert L.nbd_accel_sym_workspace_bytes(65536) == 16 * 65536 * 12
    assert L.nbd_accel_sym_workspace_bytes(16384 + 37) == 17 * (16384 + 37) * 12
    # the preferred size: K_PREF slots (+ the remainder's) where the step takes the symmetric force, else the plain size
    assert L.nbd_step_workspace_pref_bytes(65536) == K_PREF * 65536 * 12
    assert L.nbd_step_workspace_pref_bytes(65536 + 37) == (K_PREF + 1) * (65536 + 37) * 12
    for n in (0, 1, 1000, 2048, 16384 + 37, 65535):
        assert L.nbd_step_workspace_pref_bytes(n) == L.nbd_step_workspace_bytes(n)
    assert L.nbd_step_workspace_pref_bytes(-5) == 0

    n = 20 * 1024 + 37
    posm, mv, rows, ref = _case(n)
    # one slot short of one-slot-per-round: the next narrower plan (K = 19: 18 storing rounds, one adding), no error
    a = _sym_ws(posm, n, mv, 2, 20 * n * 12).cpu().numpy()
    assert row_rel(a[rows], ref) < 2e-6
    # a few bytes short of a slot count round down to the slots that are whole
    b = _sym_ws(posm, n, mv, 2, 21 * n * 12 - 4).cpu().numpy()
    assert np.array_equal(a, b)
    # more than the widest plan takes: the widest plan
    c = _sym_ws(posm, n, mv, 2, 30 * n * 12).cpu().numpy()
    assert np.array_equal(c, _sym_ws(posm, n, mv, 2, 21 * n * 12).cpu().numpy())
    # the 16-slot minimum (16 + the remainder's slot) still holds: exactly that runs, one byte less does not
    least = L.nbd_accel_sym_workspace_bytes(n)
    assert least == 17 * n * 12
    d = _sym_ws(posm, n, mv, 2, least).cpu().numpy()
    assert np.array_equal(d, _sym(posm, n, mv, variant=2).cpu().numpy())
    assert _sym_ws(posm, n, mv, 2, least - 1, expect=-2) is None


def test_sym_wide_step_against_16_slot_step_and_captured_run(gpu_device, monkeypatch):
    """n = 65 536 + 37, the smallest size at which the step takes the symmetric force with a remainder: the simulator's
    preferred workspace (one launch of 2016 tile pairs) against NBD_SYM_SLOTS=16 (the four launches), and run() replayed
    from captured chunks against the eager run (8 steps: run() captures from 8 steps on, a run(4) would be eager twice)."""
    from galaxify import simulation
    from nbd import _lib
    from nbd.plummer import generate_plummer
    L = _lib.lib()
    n = 65536 + 37
    p, v, m = generate_plummer(n, seed=4321)
    kw = dict(positions=p, velocities=v, masses=m, g_const=1.0, softening=0.1, dt=0.01, device="cuda")
    monkeypatch.delenv("NBD_SYM_SLOTS", raising=False)
    a = simulation.LeapFrogSimulator(**kw)
    assert a._uniform is not None
    assert a._ws.numel() * a._ws.element_size() == L.nbd_step_workspace_pref_bytes(n) == (K_PREF + 1) * n * 12
    monkeypatch.setenv("NBD_SYM_SLOTS", "16")
    b = simulation.LeapFrogSimulator(**kw)
    assert b._ws.numel() * b._ws.element_size() == L.nbd_step_workspace_bytes(n) == 17 * n * 12
    monkeypatch.delenv("NBD_SYM_SLOTS")
    a.step(); b.step()
    rel_a = row_rel(a.accelerations.cpu().numpy(), b.accelerations.cpu().numpy())
    rel_p = row_rel(a.positions.cpu().numpy(), b.positions.cpu().numpy())
    print(f"n = {n}: preferred against 16 slots after one step, accelerations {rel_a:.3e}, positions {rel_p:.3e}")
    assert rel_a < 2e-6
    assert rel_p < 1e-6

    monkeypatch.setattr(simulation.LeapFrogSimulator, "GRAPH_RUN_MAX_BODIES", n, raising=False)
    c = simulation.LeapFrogSimulator(**kw)
    d = simulation.LeapFrogSimulator(**kw)
    assert c._graph_run_ok(8)
    sc = c.run(8)
    monkeypatch.setenv("NBD_RUN_GRAPH", "0")
    assert not d._graph_run_ok(8)
    sd = d.run(8)
    for x, y in zip(sc, sd):
        assert torch.equal(x.positions, y.positions) and torch.equal(x.accelerations, y.accelerations)
    assert torch.equal(c.velocities, d.velocities)
