"""The symmetric equal-mass force with the diagonal blocks as the trailing workgroups of the one pair launch
(accel_sym2_tail_kernel, through nbd_accel_sym_tail_uniform_f32 and through the uniform-mass leapfrog step). Every row's
slot values and the finish order are those of variant 2 of nbd_accel_sym_uniform_f32, so the results are the same BITS on
the same workspace size: with a slot per round (K = M: the merged launch), with the remainder launches behind it, and
with K < M (an adding round reads slot 0: the diagonal launch stays in front, the path IS variant 2). Rows against fp64 at
the 2e-6 of the existing tests, nothing written behind the stated workspace size, run-to-run identity, the rejections of
the old entry, one LeapFrogSimulator step at n = 65 536 + 37 and its captured run."""
import functools

import numpy as np
import pytest
import torch

from conftest import row_rel
from test_direct_sym_gpu import EPS2, _f64_rows, _state

pytestmark = pytest.mark.gpu

# (n, slots handed in): M = 2 (one pair job and the trailing diagonal jobs); K = M = 6 with the remainder slot; n / 1024
# odd (M = 6, remainder longer than a tile); the wide case of test_direct_sym_wide_gpu; K = 24 < M = 34 (the fallback)
CASES = [(2048, 2), (6 * 1024 + 37, 7), (7 * 1024 + 5, 7), (20 * 1024 + 37, 21), (34 * 1024 + 4, 25)]
GUARD = 4096         # sentinel floats behind the stated workspace size


def _force(posm, n, mass_value, nbytes, tail, eps2=EPS2, g=1.0, expect=0):
    """The tail entry (tail) or variant 2 of the old one on a workspace of exactly nbytes, guard floats behind it."""
    from nbd import _lib
    L = _lib.lib()
    buf = torch.full(((nbytes + 3) // 4 + GUARD,), 12345.0, dtype=torch.float32, device=posm.device)
    out = torch.empty((n, 3), dtype=torch.float32, device=posm.device)
    head = (posm.data_ptr(), n, eps2, g, mass_value, out.data_ptr(), buf.data_ptr(), nbytes)
    st = _lib.current_stream(posm.device)
    rc = L.nbd_accel_sym_tail_uniform_f32(*head, st) if tail else L.nbd_accel_sym_uniform_f32(*head, 2, st)
    assert rc == expect, L.nbd_strerror(rc)
    assert bool((buf[(nbytes + 3) // 4:] == 12345.0).all())
    return out if rc == 0 else None


@functools.lru_cache(maxsize=None)
def _case(n):
    """State, sampled rows and their fp64 reference of one size: computed once, shared by the tests, never written."""
    p, m, posm = _state(n, seed=n + 5)
    mv = float(np.float32(m[0]))
    assert np.all(m.astype(np.float32) == np.float32(mv))
    core = (n // 1024 & ~1) * 1024
    rng = np.random.default_rng(3)
    # the first and last row of a diagonal group (128 rows), of a half workgroup's pair of them, of a tile, of the core
    edges = [0, 127, 128, 255, 256, 1023, 1024, 1151, core - 1024, core - 129, core - 128, core - 1, core, n - 1]
    rows = np.unique(np.concatenate([rng.choice(n, 96, replace=False), edges]))
    rows = rows[rows < n]
    ref = _f64_rows(p, m, rows)
    ref.setflags(write=False)
    return posm, mv, rows, ref


@pytest.mark.parametrize("n,slots", CASES)
def test_sym_tail_same_bits_as_variant_2_and_rows_against_f64(n, slots, gpu_device):
    posm, mv, rows, ref = _case(n)
    new = _force(posm, n, mv, slots * n * 12, tail=True)
    old = _force(posm, n, mv, slots * n * 12, tail=False)
    assert torch.isfinite(new).all()
    assert torch.equal(new, old)
    rel = row_rel(new.cpu().numpy()[rows], ref)
    print(f"n = {n}, {slots} slots: against fp64 on {len(rows)} rows, row_rel = {rel:.3e}")
    assert rel < 2e-6


@pytest.mark.parametrize("n,slots", CASES)
def test_sym_tail_bit_identical_run_to_run(n, slots, gpu_device):
    posm, mv, _, _ = _case(n)
    assert torch.equal(_force(posm, n, mv, slots * n * 12, tail=True), _force(posm, n, mv, slots * n * 12, tail=True))


def test_sym_tail_rejects_what_the_old_entry_rejects(gpu_device):
    from nbd import _lib
    L = _lib.lib()
    _, m, posm = _state(1000, seed=1)
    assert _force(posm, 1000, 1.0, 1 << 20, tail=True, expect=-3) is None             # fewer than two tiles
    posm, mv, _, _ = _case(2048)
    assert _force(posm, 2048, mv, 2 * 2048 * 12, tail=True, eps2=0.0, expect=-3) is None   # unsoftened
    n = 6 * 1024 + 37
    posm, mv, _, _ = _case(n)
    least = L.nbd_accel_sym_workspace_bytes(n)
    assert least == 7 * n * 12
    assert _force(posm, n, mv, least - 1, tail=True, expect=-2) is None               # short workspace
    assert _force(posm, n, mv, least - 1, tail=False, expect=-2) is None


def test_sym_tail_step_same_bits_as_variant_2_and_captured_run(gpu_device, monkeypatch):
    """n = 65 536 + 37, the smallest size at which the step takes the symmetric force with a remainder: the accelerations
    of one step are the bits of variant 2 on the step's own packed bodies and a workspace of the step's size; run()
    replayed from captured chunks equals the eager run (8 steps: run() captures from 8 steps on)."""
    from galaxify import simulation
    from nbd import _lib
    from nbd.plummer import generate_plummer
    L = _lib.lib()
    n = 65536 + 37
    p, v, m = generate_plummer(n, seed=4321)
    kw = dict(positions=p, velocities=v, masses=m, g_const=1.0, softening=0.1, dt=0.01, device="cuda")
    monkeypatch.delenv("NBD_SYM_SLOTS", raising=False)
    sim = simulation.LeapFrogSimulator(**kw)
    assert sim._uniform is not None
    nbytes = L.nbd_step_workspace_pref_bytes(n)
    assert sim._ws.numel() * sim._ws.element_size() == nbytes == 65 * n * 12
    sim.step()
    ref = _force(sim._posm, n, sim._uniform, nbytes, tail=False, eps2=sim._eps2, g=sim._g)
    assert torch.equal(sim.accelerations, ref)

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
