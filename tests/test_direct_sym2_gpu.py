"""Variant 2 of the symmetric equal-mass force (accel_sym2_kernel: two sources per step, packed by source) through
nbd_accel_sym_uniform_f32: rows against fp64, against variant 0 and against the all-pairs kernel, including the tile edges
and the ragged remainder; run-to-run bit identity; net momentum; and the uniform-mass step, which takes this variant from
N = 65 536 on, replayed from captured chunks equal to the eager run."""
import numpy as np
import pytest
import torch

from conftest import row_rel
from test_direct_sym_gpu import EPS2, _f64_rows, _state, _sym

pytestmark = pytest.mark.gpu

SIZES = [2048, 16384 + 37, 65536]


@pytest.mark.parametrize("n", SIZES)
def test_sym2_rows_against_f64_variant0_and_all_pairs(n, gpu_device):
    from nbd import direct
    p, m, posm = _state(n, seed=n + 1)
    mv = float(np.float32(m[0]))
    acc = _sym(posm, n, mv, variant=2)
    assert torch.isfinite(acc).all()
    a = acc.cpu().numpy()
    assert row_rel(a, _sym(posm, n, mv, variant=0).cpu().numpy()) < 2e-6
    assert row_rel(a, direct.accel(posm, n, posm, n, 0, EPS2, 1.0).cpu().numpy()) < 2e-6
    # rows from every tile, both chunks of each chunk pair (c, c + 8), the tile edges and the ragged remainder
    rng = np.random.default_rng(1)
    edges = [0, 63, 64, 511, 512, 575, 1023, 1024, 2047, n - 1, n - 37, n - 38]
    rows = np.unique(np.concatenate([rng.choice(n, 96, replace=False), edges]))
    rows = rows[(rows >= 0) & (rows < n)]
    assert row_rel(a[rows], _f64_rows(p, m, rows)) < 2e-6


@pytest.mark.parametrize("n", SIZES)
def test_sym2_bit_identical_run_to_run_and_momentum(n, gpu_device):
    p, m, posm = _state(n, seed=11)
    mv = float(np.float32(m[0]))
    a1 = _sym(posm, n, mv, variant=2)
    a2 = _sym(posm, n, mv, variant=2)
    assert torch.equal(a1, a2)
    acc = a1.cpu().numpy().astype(np.float64)
    net = acc.sum(0)
    assert np.abs(net).max() < 1e-6 * np.abs(acc).sum(0).max()


def test_sym2_rejects_unknown_variant(gpu_device):
    from nbd import _lib, direct
    L = _lib.lib()
    _, _, posm = _state(4096, seed=1)
    ws = direct.alloc_bytes(L.nbd_accel_sym_workspace_bytes(4096), posm.device)
    out = torch.empty((4096, 3), dtype=torch.float32, device="cuda")
    assert L.nbd_accel_sym_uniform_f32(posm.data_ptr(), 4096, EPS2, 1.0, 1.0, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                       3, _lib.current_stream(posm.device)) == -1


def test_sym2_step_captured_run_equals_eager(gpu_device, monkeypatch):
    from galaxify import simulation
    from nbd.plummer import generate_plummer
    n = 65536
    p, v, m = generate_plummer(n, seed=99)
    kw = dict(positions=p, velocities=v, masses=m, g_const=1.0, softening=0.1, dt=0.01, device="cuda")
    monkeypatch.setattr(simulation.LeapFrogSimulator, "GRAPH_RUN_MAX_BODIES", n, raising=False)
    c = simulation.LeapFrogSimulator(**kw)
    d = simulation.LeapFrogSimulator(**kw)
    assert c._uniform is not None and c._graph_run_ok(8)
    sc = c.run(8)
    monkeypatch.setenv("NBD_RUN_GRAPH", "0")
    assert not d._graph_run_ok(8)
    sd = d.run(8)
    for x, y in zip(sc, sd):
        assert torch.equal(x.positions, y.positions) and torch.equal(x.accelerations, y.accelerations)
    assert torch.equal(c.velocities, d.velocities)
