"""Consistent-potential diagnostics without a GPU: the fp64 oracle (tests/diag_oracle.py) pinned to real reference
output where the two potential conventions coincide, Invariants.from_row, the argument checks of the new C-ABI entries,
and the refusal of range-sharded simulators."""
import ctypes

import numpy as np
import pytest

import diag_oracle as do
from conftest import load_golden
from nbd import _lib


def test_oracle_matches_reference_energies_where_the_conventions_coincide():
    """Softening 0: -G m_i m_j / (|r| + 0) is the Plummer pair potential at eps = 0, so the oracle's U = 1/2 sum m phi and K
    are the reference's recorded energy0 (tolerances of test_golden_energies)."""
    g = load_golden("direct_plummer_n64_eps0")
    assert float(g["softening"]) == 0.0
    phi = do.potentials(g["pos"], g["mass"], float(g["g_const"]), 0.0)
    row = do.invariants_row(g["pos"], g["vel"], g["mass"], phi)
    u0, k0 = (float(x) for x in g["energy0"])
    assert u0 < 0 < k0
    assert abs(row[11] - u0) <= 2e-5 * abs(u0) + 1e-30
    assert abs(row[10] - k0) <= 2e-6 * abs(k0) + 1e-30
    assert row[12] == row[10] + row[11] and row[13] == -2.0 * row[10] / row[11]
    u_ref, k_ref = do.reference_energies(g["pos"], g["vel"], g["mass"], float(g["g_const"]), 0.0)
    assert abs(u_ref - row[11]) <= 1e-12 * abs(u_ref) and abs(k_ref - row[10]) <= 1e-12 * abs(k_ref)


def test_conventions_differ_with_softening():
    g = load_golden("direct_plummer_n64")
    eps = float(g["softening"])
    assert eps > 0
    phi = do.potentials(g["pos"], g["mass"], float(g["g_const"]), eps * eps)
    row = do.invariants_row(g["pos"], g["vel"], g["mass"], phi)
    u_ref, _ = do.reference_energies(g["pos"], g["vel"], g["mass"], float(g["g_const"]), eps)
    assert abs(row[11] - u_ref) > 1e-3 * abs(u_ref)          # 1 / sqrt(r^2 + eps^2) > 1 / (r + eps) for every pair
    assert row[11] < u_ref < 0


def test_oracle_row_of_a_hand_system():
    x = np.array([[1.0, 0, 0], [-1.0, 0, 0]])
    v = np.array([[0, 0.5, 0], [0, -0.5, 0]])
    m = np.array([2.0, 2.0])
    phi = do.potentials(x, m, 1.0, 0.0)
    assert np.array_equal(phi, [-1.0, -1.0])
    row = do.invariants_row(x, v, m, phi)
    #                          M    C          P          L            K    U     E     Q
    assert row.tolist() == [4.0, 0, 0, 0, 0, 0, 0, 0, 0, 2.0, 0.5, -2.0, -1.5, 0.5, 0, 0]
    assert do.invariants_row(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), np.zeros(0)).tolist() == [0.0] * 16


def test_invariants_from_row_round_trips():
    from galaxify.simulation import Invariants, SimulationState
    row = [3.0, 0.1, 0.2, 0.3, 1.0, 2.0, 3.0, -1.0, -2.0, -3.0, 0.25, -0.5, -0.25, 1.0, 0.0, 0.0]
    inv = Invariants.from_row(row)
    assert inv.mass == 3.0 and inv.com == (0.1, 0.2, 0.3) and inv.momentum == (1.0, 2.0, 3.0)
    assert inv.angular_momentum == (-1.0, -2.0, -3.0)
    assert (inv.k_energy, inv.u_energy, inv.energy, inv.virial_ratio) == (0.25, -0.5, -0.25, 1.0)
    assert inv.row() == row and Invariants.from_row(inv.row()) == inv
    assert Invariants.from_row(np.array(row)) == inv
    import torch
    assert Invariants.from_row(torch.tensor(row, dtype=torch.float64)) == inv
    assert all(isinstance(x, float) for x in (inv.mass, *inv.com, inv.energy))
    with pytest.raises(ValueError):
        Invariants.from_row(row[:13])
    z = torch.zeros((2, 3))
    st = SimulationState(0, 0.0, z, z, z)
    assert st.invariants is None and st.u_energy is None
    assert SimulationState(0, 0.0, z, z, z, 1.0, 2.0, inv).invariants is inv      # the new field is the last one


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    L = _lib.lib()
    assert L.nbd_potential_workspace_bytes(0, 5) == 0 and L.nbd_potential_workspace_bytes(5, -1) == 0
    g, s, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for n_src, n_tgt in [(1, 1), (300, 300), (8257, 8257), (65536, 65536), (65536, 8192)]:
        assert L.nbd_accel_plan(n_src, n_tgt, g, s, c) == 0
        assert L.nbd_potential_workspace_bytes(n_src, n_tgt) == s.value * n_tgt * 8        # one fp64 slab per source split
    assert L.nbd_potential_f32(None, -1, None, 1, 0, 0.01, 1.0, None, None, 0, None) == -1
    assert L.nbd_potential_f32(None, 4, None, -4, 0, 0.01, 1.0, None, None, 0, None) == -1
    assert L.nbd_potential_f32(None, 4, None, 4, 0, 0.01, 1.0, None, None, 0, None) == -1       # null buffers
    assert L.nbd_potential_f32(0x1000, 4, 0x1000, 4, -1, 0.01, 1.0, 0x2000, 0x3000, 1 << 20, None) == -1
    assert L.nbd_potential_f32(0x1000, 4, 0x1008, 4, 0, 0.01, 1.0, 0x2000, 0x3000, 1 << 20, None) == -1   # misaligned
    assert L.nbd_potential_f32(0x1000, 4, 0x1000, 4, 0, 0.01, 1.0, 0x2004, 0x3000, 1 << 20, None) == -1   # phi: 8 bytes
    assert L.nbd_potential_f32(0x1000, 4, 0x1000, 4, 0, 0.01, 1.0, 0x2000, None, 0, None) == -2
    assert L.nbd_potential_f32(0x1000, 4, 0x1000, 4, 0, 0.01, 1.0, 0x2000, 0x3000, 31, None) == -2
    assert L.nbd_potential_f32(None, 4, None, 0, 0, 0.01, 1.0, None, None, 0, None) == 0        # no targets: a no-op
    assert L.nbd_invariants_f64(None, None, None, -1, 0x1000, None) == -1
    assert L.nbd_invariants_f64(None, None, None, 0, None, None) == -1                          # the row is always written
    assert L.nbd_invariants_f64(None, None, None, 4, 0x1000, None) == -1
    assert L.nbd_invariants_f64(0x1008, 0x2000, 0x3000, 4, 0x1000, None) == -1
    # batched: the host offsets and the plan are validated first
    off = (ctypes.c_int * 3)(0, 5, 70)
    bad = (ctypes.c_int * 3)(0, 5, 3)
    items, rows = ctypes.c_int(), ctypes.c_int()
    pb, wb = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.nbd_batch_plan(off, 2, items, rows, pb, wb) == 0
    addr = lambda a: ctypes.cast(a, ctypes.c_void_p).value                                      # noqa: E731
    assert L.nbd_batch_potential_f32(addr(bad), 2, 0x1000, pb.value, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, wb.value,
                                     None) == -1
    assert L.nbd_batch_potential_f32(addr(off), 2, None, pb.value, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, wb.value,
                                     None) == -1
    assert L.nbd_batch_potential_f32(addr(off), 2, 0x1000, pb.value + 4, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, wb.value,
                                     None) == -1
    assert L.nbd_batch_potential_f32(addr(off), 2, 0x1000, pb.value, None, 0x1000, 0x1000, 0x1000, 0x1000, wb.value,
                                     None) == -1
    assert L.nbd_batch_potential_f32(addr(off), 2, 0x1000, pb.value, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 8, None) == -2
    assert L.nbd_batch_invariants_f64(addr(bad), 2, 0x1000, pb.value, 0x1000, 0x1000, 0x1000, 0x1000, None) == -1
    assert L.nbd_batch_invariants_f64(addr(off), 2, 0x1000, pb.value, 0x1000, 0x1000, 0x1000, None, None) == -1
    assert L.nbd_batch_invariants_f64(addr(off), 2, 0x1000, pb.value, 0x1000, None, 0x1000, 0x1000, None) == -1


def test_range_sharded_simulators_refuse_diagnostics():
    """The refusal itself, on a stub that only says it is sharded (the GPU suite runs it on a real one-rank group)."""
    from galaxify import simulation
    sim = object.__new__(simulation.LeapFrogSimulator)
    sim._sharded, sim.n, sim.calc_invariants = True, 8, True
    with pytest.raises(ValueError):
        sim.compute_potentials()
    with pytest.raises(ValueError):
        sim.compute_invariants()
    with pytest.raises(ValueError):
        sim.run(3)
