"""Variant 2 of the symmetric equal-mass force (accel_sym2_kernel) where a ragged n meets an ADDING launch: the launches
after the first add to the slot rows an earlier launch stored, and fetch those rows before the pair walk. The sizes of
test_direct_sym2_gpu.py never combine the two (16 384 + 37 has the storing launch only). Here:
n = 20 * 1024 + 37: 20 tiles, 19 rounds = a storing launch of 15 + an adding launch of 4, a slot stride n * 12 that is no
multiple of 16 bytes, 37 remainder rows; n = 34 * 1024 + 4: 34 tiles, 33 rounds = 15 + 16 + a partial adding launch of 2.
Rows against fp64 and against variant 0 at the 2e-6 of the existing tests, run-to-run bit identity, net momentum."""
import numpy as np
import pytest
import torch

from conftest import row_rel
from test_direct_sym_gpu import _f64_rows, _state, _sym

pytestmark = pytest.mark.gpu

SIZES = [20 * 1024 + 37, 34 * 1024 + 4]


def _core(n):
    return (n // 1024 & ~1) * 1024


@pytest.mark.parametrize("n", SIZES)
def test_sym2_adding_launch_rows_against_f64_and_variant0(n, gpu_device):
    p, m, posm = _state(n, seed=n + 1)
    mv = float(np.float32(m[0]))
    acc = _sym(posm, n, mv, variant=2)
    assert torch.isfinite(acc).all()
    a = acc.cpu().numpy()
    rel0 = row_rel(a, _sym(posm, n, mv, variant=0).cpu().numpy())
    print(f"n = {n}: variant 2 against variant 0, row_rel = {rel0:.3e}")
    assert rel0 < 2e-6
    core = _core(n)
    assert 0 < core < n
    rng = np.random.default_rng(2)
    edges = [0, 63, 64, 511, 512, 1023, 1024, 2047, core - 1024, core - 1, core, n - 1]
    rows = np.unique(np.concatenate([rng.choice(n, 96, replace=False), edges]))
    for r in (0, 1023, 1024, core - 1, core, n - 1):
        assert r in rows
    rel64 = row_rel(a[rows], _f64_rows(p, m, rows))
    print(f"n = {n}: variant 2 against fp64 on {len(rows)} rows, row_rel = {rel64:.3e}")
    assert rel64 < 2e-6


@pytest.mark.parametrize("n", SIZES)
def test_sym2_adding_launch_bit_identical_run_to_run_and_momentum(n, gpu_device):
    p, m, posm = _state(n, seed=11)
    mv = float(np.float32(m[0]))
    a1 = _sym(posm, n, mv, variant=2)
    a2 = _sym(posm, n, mv, variant=2)
    assert torch.equal(a1, a2)
    acc = a1.cpu().numpy().astype(np.float64)
    net = acc.sum(0)
    print(f"n = {n}: net / sum |a| = {np.abs(net).max() / np.abs(acc).sum(0).max():.3e}")
    assert np.abs(net).max() < 1e-6 * np.abs(acc).sum(0).max()
