"""The symmetric equal-mass force (accel_sym_kernel: every off-diagonal pair evaluated once, Newton's third law) through
its force-only entry point nbd_accel_sym_uniform_f32 and through the uniform-mass leapfrog step that takes it from
N = 65 536 on: rows against fp64 and against the all-pairs kernel, run-to-run bit identity, net momentum, and a
captured run() equal to the eager one."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import row_rel

pytestmark = pytest.mark.gpu

EPS2 = float(np.float32(0.1 ** 2))


def _state(n, seed):
    from nbd import direct
    from nbd.plummer import generate_plummer
    p, v, m = generate_plummer(n, seed=seed)
    pos = torch.tensor(p, dtype=torch.float32).cuda()
    mass = torch.tensor(m, dtype=torch.float32).cuda()
    return p, m, direct.pack_posm(pos, mass)


def _sym(posm, n, mass_value, variant=0, g=1.0):
    from nbd import _lib, direct
    L = _lib.lib()
    ws = direct.alloc_bytes(L.nbd_accel_sym_workspace_bytes(n), posm.device)
    out = torch.empty((n, 3), dtype=torch.float32, device=posm.device)
    _lib.check(L.nbd_accel_sym_uniform_f32(posm.data_ptr(), n, EPS2, g, mass_value, out.data_ptr(), ws.data_ptr(),
                                           ws.numel(), variant, _lib.current_stream(posm.device)),
               "nbd_accel_sym_uniform_f32")
    return out


def _f64_rows(p, m, rows):
    pf, mf = p.astype(np.float32).astype(np.float64), m.astype(np.float32).astype(np.float64)
    d = pf[None, :, :] - pf[rows, None, :]
    inv = ((d * d).sum(2) + EPS2) ** -1.5
    inv[np.arange(len(rows)), rows] = 0.0
    return (d * (inv * mf[None, :])[:, :, None]).sum(1)


@pytest.mark.parametrize("n", [2048, 16384 + 37, 65536])
def test_sym_force_rows_against_f64_and_all_pairs(n, gpu_device):
    from nbd import direct
    p, m, posm = _state(n, seed=n)
    mv = float(np.float32(m[0]))
    assert np.all(m.astype(np.float32) == np.float32(mv))
    acc = _sym(posm, n, mv)
    ref_gpu = direct.accel(posm, n, posm, n, 0, EPS2, 1.0)
    assert torch.isfinite(acc).all()
    a = acc.cpu().numpy()
    assert row_rel(a, ref_gpu.cpu().numpy()) < 2e-6
    # rows from every tile, the tile edges and the ragged remainder
    rng = np.random.default_rng(0)
    rows = np.unique(np.concatenate([rng.choice(n, 96, replace=False), [0, 1023, 1024, n - 1, n - 37, n - 38]]))
    rows = rows[(rows >= 0) & (rows < n)]
    assert row_rel(a[rows], _f64_rows(p, m, rows)) < 2e-6
    # both register shapes compute the same sums in another order
    assert row_rel(_sym(posm, n, mv, variant=1).cpu().numpy(), a) < 2e-6


@pytest.mark.parametrize("n", [2048, 16384 + 37, 65536])
def test_sym_force_bit_identical_run_to_run_and_momentum(n, gpu_device):
    p, m, posm = _state(n, seed=7)
    mv = float(np.float32(m[0]))
    a1 = _sym(posm, n, mv)
    a2 = _sym(posm, n, mv)
    assert torch.equal(a1, a2)
    acc = a1.cpu().numpy().astype(np.float64)
    net = acc.sum(0)                              # equal masses: sum_i m a_i = m sum_i a_i
    assert np.abs(net).max() < 1e-6 * np.abs(acc).sum(0).max()


def test_sym_force_rejects_what_it_does_not_cover(gpu_device):
    from nbd import _lib, direct
    L = _lib.lib()
    _, m, posm = _state(1000, seed=1)
    ws = direct.alloc_bytes(1 << 20, posm.device)
    out = torch.empty((1000, 3), dtype=torch.float32, device="cuda")
    st = _lib.current_stream(posm.device)
    assert L.nbd_accel_sym_uniform_f32(posm.data_ptr(), 1000, EPS2, 1.0, 1.0, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                       0, st) == -3                      # fewer than two tiles
    _, m, posm = _state(4096, seed=1)
    out = torch.empty((4096, 3), dtype=torch.float32, device="cuda")
    assert L.nbd_accel_sym_uniform_f32(posm.data_ptr(), 4096, 0.0, 1.0, 1.0, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                       0, st) == -3                      # unsoftened: the index-masked kernel's case
    assert L.nbd_accel_sym_uniform_f32(posm.data_ptr(), 4096, EPS2, 1.0, 1.0, out.data_ptr(), ws.data_ptr(), 16,
                                       0, st) == -2
    assert L.nbd_accel_sym_workspace_bytes(65536) == L.nbd_step_workspace_bytes(65536) == 16 * 65536 * 12
    assert L.nbd_accel_sym_workspace_bytes(16384 + 37) == 17 * (16384 + 37) * 12


def test_uniform_step_on_symmetric_path_matches_all_pairs_and_captured_run(gpu_device, monkeypatch):
    """N = 65 536 equal masses: the step takes the symmetric force; its accelerations match the general-mass step (the
    all-pairs kernel) to summation-order rounding, and run() replayed from captured chunks equals the eager run bit for
    bit."""
    from galaxify import simulation
    from nbd.plummer import generate_plummer
    n = 65536
    p, v, m = generate_plummer(n, seed=1234)
    kw = dict(positions=p, velocities=v, masses=m, g_const=1.0, softening=0.1, dt=0.01, device="cuda")
    a = simulation.LeapFrogSimulator(**kw)
    assert a._uniform is not None
    b = simulation.LeapFrogSimulator(**kw)
    b._uniform = None                                     # the general-mass step: all-pairs kernel
    a.step(); b.step()
    assert row_rel(a.accelerations.cpu().numpy(), b.accelerations.cpu().numpy()) < 2e-6
    assert row_rel(a.positions.cpu().numpy(), b.positions.cpu().numpy()) < 1e-6

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
