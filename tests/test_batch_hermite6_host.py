"""BatchedSimulator(integrator="hermite6") without a GPU: the new entries are in the header and the ctypes table with the
declared signatures, the parameter rows are hermite6_step_constants' expressions bit for bit, the 9-row work list is the
float64 one with nine doubles per body and slab, every launching entry rejects bad arguments before anything reaches the
device, and the constructor refuses what there is no form of before it resolves a device."""
import ctypes
import os
import re
from ctypes import c_int, c_size_t, c_void_p, POINTER

import numpy as np
import pytest
import torch

from conftest import ROOT
from nbd import _lib

E_BADARG, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -3
HEAD = [c_void_p, c_int, c_void_p, c_size_t]
# symbol -> (return type, argument types), written out from include/nbd.h
NEW = {
    "nbd_batch_hermite6_f64_plan_fill": (c_int, HEAD),
    "nbd_batch_hermite6_f64_workspace_bytes": (c_int, [c_void_p, c_int, POINTER(c_size_t)]),
    "nbd_batch_hermite6_pack_f64": (c_int, HEAD + [c_void_p] * 7 + [c_void_p]),
    "nbd_batch_accel_jerk_snap_f64": (c_int, HEAD + [c_void_p] * 7 + [c_void_p, c_size_t, c_void_p]),
    "nbd_batch_hermite6_step_f64": (c_int, HEAD + [c_void_p] * 15 + [c_void_p, c_size_t, c_void_p]),
}
SIZES = [3, 0, 64, 65, 1, 130, 520, 1000]
SLABS = [1, None, 1, 1, 1, 1, 2, 4]       # plan_f64: min(ceil(1024 / groups), n_chunks / 4, max), at least 1


def _off(sizes):
    off = np.zeros(len(sizes) + 1, dtype=np.int32)
    np.cumsum(sizes, out=off[1:])
    return off


def _plan(sizes, order):
    """(offsets, items, rows, plan bytes, workspace bytes, item records (k, 4), scene records (S, 8), row_scene, buffer)
    of the 6-row float64 plan (order 4) or the 9-row one (order 6)."""
    L = _lib.lib()
    off = _off(sizes)
    items, rows, pb, wb = c_int(), c_int(), c_size_t(), c_size_t()
    assert L.nbd_batch_f64_plan(off.ctypes.data, len(sizes), items, rows, pb) == 0
    ws_bytes, fill = ((L.nbd_batch_f64_workspace_bytes, L.nbd_batch_f64_plan_fill) if order == 4 else
                      (L.nbd_batch_hermite6_f64_workspace_bytes, L.nbd_batch_hermite6_f64_plan_fill))
    assert ws_bytes(off.ctypes.data, len(sizes), wb) == 0
    buf = np.zeros((pb.value + 15) // 16 * 4, dtype=np.int32)
    assert fill(off.ctypes.data, len(sizes), buf.ctypes.data, pb.value) == 0
    k, S = items.value, len(sizes)
    return (off, k, rows.value, pb.value, wb.value, buf[:4 * k].reshape(k, 4), buf[4 * k:4 * k + 8 * S].reshape(S, 8),
            buf[4 * k + 8 * S:4 * k + 8 * S + rows.value], buf)


def test_new_symbols_are_declared_and_bound_with_their_signatures():
    header = open(os.path.join(ROOT, "include", "nbd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(nbd_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    for sym, (restype, argtypes) in NEW.items():
        assert sym in declared and hasattr(L, sym), sym
        assert _lib.SIGNATURES[sym] == (restype, argtypes), sym
        # the count of parameters the header declares
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % sym, text).group(1)
        assert len(decl.split(",")) == len(argtypes), sym
    assert "#define NBD_ABI_VERSION 2" in header and L.nbd_abi_version() == 2
    assert "#define NBD_BATCH_H6_PARAM_ROWS 13" in header


@pytest.mark.parametrize("dts", [[0.01, 1.0 / 3.0, 2.0 ** -7]])
def test_parameter_rows_are_the_one_system_expressions(dts):
    from nbd import direct
    g, eps = [1.0, 0.7, 2.5], [0.1, 0.0, 1.0 / 7.0]
    rows = direct.batch_h6_params(g, eps, dts)
    assert len(rows) == direct.BATCH_H6_PARAM_ROWS == 13 and all(len(r) == 3 for r in rows)
    assert rows[:3] == direct.batch_f64_params(g, eps, dts)[:3]
    for s, dt in enumerate(dts):
        # hermite6_step_constants, written out
        dt2 = dt * dt
        dt3 = dt2 * dt
        want = [g[s], float(eps[s]) ** 2, eps[s], dt, 0.5 * dt, 0.5 * dt2, dt3 / 6.0, dt2 * dt2 / 24.0,
                dt2 * dt3 / 120.0, dt2 / 10.0, dt3 / 120.0, dt2, dt3]
        assert [float(r[s]).hex() for r in rows] == [float(w).hex() for w in want]


def test_plan_is_the_float64_plan_with_nine_rows_per_slab():
    off4, k4, rows4, pb4, wb4, items4, scenes4, row_scene4, _ = _plan(SIZES, 4)
    off6, k6, rows6, pb6, wb6, items6, scenes6, row_scene6, _ = _plan(SIZES, 6)
    assert (k6, rows6, pb6) == (k4, rows4, pb4) and 2 * wb6 == 3 * wb4 and wb4 > 0
    assert np.array_equal(items6, items4) and np.array_equal(row_scene6, row_scene4)
    ws_off = 0
    for s, n in enumerate(SIZES):
        assert int(scenes6[s][3]) == ws_off, s
        rest = [0, 1, 2, 4, 5, 6, 7]                      # every field but ws_off is the 6-row plan's
        assert np.array_equal(scenes6[s][rest], scenes4[s][rest])
        if n == 0:
            assert int(scenes6[s][5]) == 0
            continue
        assert int(scenes6[s][5]) == SLABS[s], (s, n)
        ws_off += SLABS[s] * 9 * n
    assert wb6 == 8 * ws_off
    # through the Python plan
    from nbd import direct
    p4 = direct.BatchPlan(SIZES, "cpu", dtype=torch.float64)
    p6 = direct.BatchPlan(SIZES, "cpu", dtype=torch.float64, order=6)
    assert (p6.n_items, p6.posm_rows, p6.plan_bytes) == (p4.n_items, p4.posm_rows, p4.plan_bytes) == (k4, rows4, pb4)
    assert (p4.workspace_bytes, p6.workspace_bytes) == (wb4, wb6)
    assert (p4.param_rows, p6.param_rows) == (8, 13) and (p4.order, p6.order) == (4, 6)
    with pytest.raises(_lib.NbdError):
        direct.BatchPlan(SIZES, "cpu", order=6)           # there is no fp32 form


def test_plan_of_empty_scenes_and_bad_offsets():
    L = _lib.lib()
    _, k, rows, pb, wb, *_ = _plan([0, 0], 6)
    assert (k, rows, wb, pb) == (0, 0, 0, 64)
    n = c_size_t()
    for bad, S in ((np.array([0, 5, 2], dtype=np.int32), 2), (np.array([1, 5], dtype=np.int32), 1),
                   (np.array([0, 5], dtype=np.int32), 0)):
        assert L.nbd_batch_hermite6_f64_workspace_bytes(bad.ctypes.data, S, n) == E_BADARG
        assert L.nbd_batch_hermite6_f64_plan_fill(bad.ctypes.data, S, bad.ctypes.data, 64) == E_BADARG
    off = _off([5, 7])
    assert L.nbd_batch_hermite6_f64_workspace_bytes(off.ctypes.data, 2, None) == E_BADARG
    assert L.nbd_batch_hermite6_f64_workspace_bytes(None, 2, n) == E_BADARG
    _, _, _, pb, _, _, _, _, host = _plan([5, 7], 6)
    assert L.nbd_batch_hermite6_f64_plan_fill(off.ctypes.data, 2, None, pb) == E_BADARG
    assert L.nbd_batch_hermite6_f64_plan_fill(off.ctypes.data, 2, host.ctypes.data, pb - 16) == E_BADARG
    # the partial sums counted in doubles must stay within the int offsets: 1 slab x 9 x 3e8 bodies does not, where the
    # 6-row plan of the same size still does
    big = _off([300_000_000])
    assert L.nbd_batch_f64_workspace_bytes(big.ctypes.data, 1, n) == 0
    assert L.nbd_batch_hermite6_f64_workspace_bytes(big.ctypes.data, 1, n) == E_UNSUPPORTED


# entry -> (device pointers between the plan head and the tail, the packed rows among them, those that may be NULL,
# takes a workspace)
SHAPE = {"nbd_batch_hermite6_pack_f64": (7, (4, 5, 6), (2,), False),
         "nbd_batch_accel_jerk_snap_f64": (7, (0, 1, 2), (), True),
         "nbd_batch_hermite6_step_f64": (15, (12, 13, 14), (), True)}


def _call(name, head, ptrs, ws=None, wsb=0):
    tail = (ws, wsb, None) if SHAPE[name][3] else (None,)
    return getattr(_lib.lib(), name)(*head, *ptrs, *tail)


@pytest.mark.parametrize("name", sorted(SHAPE))
def test_bad_arguments_are_rejected_without_touching_the_gpu(name):
    sizes = [5, 0, 70]
    off, _, _, pb, need, _, _, _, host = _plan(sizes, 6)
    S, p = len(sizes), host.ctypes.data
    assert p % 16 == 0 and need == 8 * 9 * 75
    keep = np.zeros(64, dtype=np.float64)
    A = (keep.ctypes.data + 31) // 32 * 32                  # a 32-byte aligned host address; no entry dereferences it
    k, rows_at, optional, has_ws = SHAPE[name]
    head = (off.ctypes.data, S, p, pb)
    # every device pointer NULL, then one NULL among the rest
    assert _call(name, head, [None] * k, A, need) == E_BADARG
    for i in range(k):
        if i in optional:
            continue
        q = [A] * k
        q[i] = None
        assert _call(name, head, q, A, need) == E_BADARG, i
    # each of the three packed arrays needs 32-byte alignment
    for i in rows_at:
        q = [A] * k
        q[i] = A + 16
        assert _call(name, head, q, A, need) == E_BADARG, i
    # the plan: 16-byte aligned, its byte count the reported one, offsets and scene count valid
    for bad_head in ((off.ctypes.data, S, p, pb + 16), (off.ctypes.data, S, None, pb), (off.ctypes.data, S, p + 4, pb),
                     (off.ctypes.data, 0, p, pb), (None, S, p, pb)):
        assert _call(name, bad_head, [A] * k, A, need) == E_BADARG, bad_head
    if has_ws:
        # arrays given but no workspace, a misaligned one, one a byte short, or the 6-row plan's: NBD_E_WORKSPACE
        for ws, wsb in ((None, need), (A + 4, need), (A, need - 1), (A, need * 2 // 3), (A, 0)):
            assert _call(name, head, [A] * k, ws, wsb) == E_WORKSPACE, (ws, wsb)


def test_an_all_empty_batch_is_a_no_op_without_a_gpu():
    off, _, _, pb, _, _, _, _, host = _plan([0, 0], 6)
    head = (off.ctypes.data, 2, host.ctypes.data, pb)
    for name, (k, _, _, _) in SHAPE.items():
        assert _call(name, head, [None] * k) == 0, name


def test_the_float64_diagnostics_accept_the_nine_row_plan():
    """Their host checks on the 9-row plan with its workspace pass up to the launch (an all-NULL call still fails on its
    pointers, not on the plan), and they refuse the 6-row plan's smaller workspace only when it is smaller than THEIR need:
    the 9-row workspace is larger than what they ask for."""
    sizes = [5, 0, 70]
    off, _, _, pb, need6, _, _, _, host = _plan(sizes, 6)
    _, _, _, pb4, need4, *_ = _plan(sizes, 4)
    assert pb == pb4 and need6 > need4
    L = _lib.lib()
    keep = np.zeros(64, dtype=np.float64)
    A = (keep.ctypes.data + 31) // 32 * 32
    head = (off.ctypes.data, len(sizes), host.ctypes.data, pb)
    # the plan is accepted (an argument error would be BADARG): with good pointers, only a short workspace is refused
    assert L.nbd_batch_potential_f64(*head, A, A, A, A, need4 - 1, None) == E_WORKSPACE
    assert L.nbd_batch_energies_f64(*head, A, A, A, A, A, need4 - 1, None) == E_WORKSPACE
    assert L.nbd_batch_accel_jerk_f64(*head, *[A] * 8, A, need4 - 1, None) == E_WORKSPACE


def test_constructor_refuses_before_any_device_is_resolved():
    from galaxify import simulation
    z = np.zeros((4, 3))
    scene = (z, z, np.ones(4))
    # device="tpu" would raise ValueError("device debe ser ...") and device="cpu" RuntimeError: the refusals come first
    with pytest.raises(ValueError, match="hermite6.*float64"):
        simulation.BatchedSimulator(systems=[scene], integrator="hermite6", dtype=torch.float32, device="tpu")
    with pytest.raises(ValueError, match="dtype must be"):
        simulation.BatchedSimulator(systems=[scene], integrator="hermite6", dtype=torch.float16, device="tpu")
    with pytest.raises(TypeError, match="no_such_keyword"):
        simulation.BatchedSimulator(systems=[scene], integrator="hermite6", no_such_keyword=1, device="tpu")
    with pytest.raises(ValueError, match="integrator must be"):
        simulation.BatchedSimulator(systems=[scene], integrator="hermite8", device="tpu")
    # a valid combination reaches the device rule: float64 is the default, and may be spelled
    for kw in ({}, {"dtype": torch.float64}):
        with pytest.raises(RuntimeError, match="cpu"):
            simulation.BatchedSimulator(systems=[scene], integrator="hermite6", device="cpu", **kw)
    assert simulation._batch_format(torch.float64, "hermite6") is not simulation._batch_format(torch.float64, "hermite")
    assert isinstance(simulation._batch_format(torch.float64, "hermite6"), simulation._BatchFloat64)
