"""The range-sharded tree force without a GPU: the argument checks of the ranged walks, the packed-row build and the
scatter (every refusal and every no-op returns before anything is launched), tree.groups, the two partitions of a
sharded TreeLeapFrogSimulator and the validation of its process_group. No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from nbd import _lib
from nbd.dist import RangePartition

WS, OUT = 0x1000, 0x2000          # aligned, never dereferenced: every call below returns from its host checks
NEW = ["nbd_tree_build_posm_f32", "nbd_tree_accel_groups_f32", "nbd_tree_potential_groups_f32",
       "nbd_tree_accel_potential_groups_f32", "nbd_tree_scatter_f32"]


def _walks():
    L = _lib.lib()
    acc = lambda ws, n, lo, hi, theta, out: L.nbd_tree_accel_groups_f32(ws, n, lo, hi, theta, 0.01, 1.0, 1, out, None, None)
    pot = lambda ws, n, lo, hi, theta, out: L.nbd_tree_potential_groups_f32(ws, n, lo, hi, theta, 0.01, 1.0, 1, out, None,
                                                                             None)
    both = lambda ws, n, lo, hi, theta, out: L.nbd_tree_accel_potential_groups_f32(ws, n, lo, hi, theta, 0.01, 1.0, 1, out,
                                                                                    out, None, None)
    return [acc, pot, both]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_ranged_walks_reject_bad_arguments(which):
    call = _walks()[which]
    n = 1000                                                     # 16 groups
    for lo, hi in ((-1, 4), (5, 4), (0, 17), (17, 17), (16, 18), (-2, -1)):
        assert call(WS, n, lo, hi, 0.5, OUT) == -1, (lo, hi)
    assert call(WS, 65, 0, 3, 0.5, OUT) == -1                    # 65 bodies are two groups
    assert call(WS, 64, 0, 2, 0.5, OUT) == -1
    assert call(WS, 0, 0, 1, 0.5, OUT) == -1                     # no bodies, no groups
    assert call(WS, -1, 0, 0, 0.5, OUT) == -1
    assert call(WS, n, 0, 16, -0.5, OUT) == -1                   # theta < 0
    assert call(WS, n, 0, 16, float("nan"), OUT) == -1
    assert call(None, n, 0, 16, 0.5, OUT) == -1                  # no workspace
    assert call(WS, n, 0, 16, 0.5, None) == -1                   # no output
    assert call(WS + 16, n, 0, 16, 0.5, OUT) == -1               # misaligned workspace
    assert call(WS, (1 << 24) + 1, 0, 1, 0.5, OUT) == -3
    assert call(WS, (1 << 24) + 1, 0, 0, 0.5, OUT) == -3


@pytest.mark.parametrize("which", [0, 1, 2])
def test_an_empty_range_is_a_no_op(which):
    call = _walks()[which]
    for n, g in ((1000, 0), (1000, 5), (1000, 16), (65, 2), (1, 1), (0, 0), (1 << 24, 1 << 18)):
        assert call(WS, n, g, g, 0.5, OUT) == 0, (n, g)
        assert call(None, n, g, g, 0.5, None) == 0, (n, g)       # nothing is asked of the pointers


def test_fused_ranged_walk_wants_both_outputs():
    L = _lib.lib()
    assert L.nbd_tree_accel_potential_groups_f32(WS, 100, 0, 2, 0.5, 0.01, 1.0, 1, None, OUT, None, None) == -1
    assert L.nbd_tree_accel_potential_groups_f32(WS, 100, 0, 2, 0.5, 0.01, 1.0, 1, OUT, None, None, None) == -1


def test_build_posm_rejects_bad_arguments():
    build = _lib.lib().nbd_tree_build_posm_f32
    big = 1 << 40
    assert build(None, 5, OUT, WS, big, None) == -1              # no rows
    assert build(OUT, 5, None, WS, big, None) == -1              # no order
    assert build(OUT, -1, OUT, WS, big, None) == -1
    assert build(OUT, 5, OUT, None, big, None) == -1             # no workspace
    assert build(OUT, 5, OUT, WS + 16, big, None) == -1          # misaligned workspace
    assert build(OUT + 4, 5, OUT, WS, big, None) == -1           # rows that are not 16-byte aligned
    assert build(OUT, 5, OUT, WS, 16, None) == -2                # a workspace that is too small
    assert build(OUT, 5, OUT, WS, _lib.lib().nbd_tree_workspace_bytes(5) - 1, None) == -2
    assert build(OUT, (1 << 24) + 1, OUT, WS, big, None) == -3
    assert build(None, 0, None, None, 0, None) == 0              # n == 0 is a no-op


def test_scatter_rejects_bad_arguments():
    scatter = _lib.lib().nbd_tree_scatter_f32
    n = 1000
    for lo, hi in ((-1, 5), (6, 5), (0, n + 1), (n + 1, n + 1)):
        assert scatter(WS, n, lo, hi, OUT, None, OUT, None, None) == -1, (lo, hi)
    assert scatter(WS, -1, 0, 0, OUT, None, OUT, None, None) == -1
    assert scatter(WS, n, 0, n, None, None, OUT, OUT, None) == -1            # nothing to place
    assert scatter(WS, n, 0, n, OUT, None, None, None, None) == -1           # rows of a without a place for them
    assert scatter(WS, n, 0, n, None, OUT, OUT, None, None) == -1            # ... of phi
    assert scatter(WS, n, 0, n, OUT, OUT, OUT, None, None) == -1
    assert scatter(None, n, 0, n, OUT, None, OUT, None, None) == -1          # no workspace
    assert scatter(WS + 16, n, 0, n, OUT, None, OUT, None, None) == -1       # misaligned workspace
    assert scatter(WS, (1 << 24) + 1, 0, 1, OUT, None, OUT, None, None) == -3
    for lo in (0, 333, n):                                                   # an empty range is a no-op
        assert scatter(WS, n, lo, lo, OUT, OUT, None, None, None) == 0
    assert scatter(None, 0, 0, 0, OUT, None, None, None, None) == 0


def test_groups():
    from nbd import tree
    assert [tree.groups(n) for n in (0, 1, 63, 64, 65, 128, 1000, 1001, 1 << 24)] == \
        [0, 1, 1, 1, 2, 2, 16, 16, 1 << 18]
    assert tree.GROUP == 64


@pytest.mark.parametrize("n,world", [(1000, 3), (65, 3), (64, 2), (1, 2), (0, 2)])
def test_partitions_cover_bodies_and_groups_once(n, world):
    """What a sharded TreeLeapFrogSimulator divides: the bodies by caller index, the target groups by group index.
    Contiguous, in rank order, balanced to one; the group ranges are valid arguments of the ranged walks (checked
    through the C entry: an empty one returns 0 before any pointer is looked at, a bad one -1)."""
    from nbd import tree
    groups = tree.groups(n)
    call = _walks()[0]
    for total in (n, groups):
        parts = [RangePartition(total, world, r) for r in range(world)]
        covered = np.zeros(total, np.int64)
        at = 0
        for p in parts:
            assert p.lo == at and p.hi - p.lo == p.n_local
            covered[p.lo:p.hi] += 1
            at = p.hi
        assert at == total and (covered == 1).all()
        counts = [p.n_local for p in parts]
        assert max(counts) - min(counts) <= 1 and counts == sorted(counts, reverse=True)
    for p in (RangePartition(groups, world, r) for r in range(world)):
        if p.n_local == 0:
            assert call(None, n, p.lo, p.hi, 0.5, None) == 0
        else:
            assert call(None, n, p.lo, p.hi, 0.5, OUT) == -1      # a valid range: refused only for the missing workspace
    if (n, world) == (65, 3):
        assert [RangePartition(groups, world, r).n_local for r in range(3)] == [1, 1, 0]       # a rank with no groups
    if (n, world) == (1, 2):
        assert [RangePartition(n, world, r).n_local for r in range(2)] == [1, 0]               # a rank with no bodies


def test_process_group_is_validated_before_a_device_is_resolved():
    from galaxify import simulation
    z = np.zeros((4, 3))
    kw = dict(positions=z, velocities=z, masses=np.ones(4))
    for bad in (object(), "world", 0, [None]):
        with pytest.raises(ValueError, match=r"TreeLeapFrogSimulator: process_group must be a "
                                             r"torch\.distributed\.ProcessGroup, got "):
            simulation.TreeLeapFrogSimulator(process_group=bad, **kw)
    # the refusals that stay, with a process_group beside them or not
    with pytest.raises(ValueError, match="float32"):
        simulation.TreeLeapFrogSimulator(dtype=torch.float64, process_group=object(), **kw)
    with pytest.raises(ValueError, match="theta"):
        simulation.TreeLeapFrogSimulator(theta=-0.1, **kw)
    grad = torch.zeros((4, 3), requires_grad=True)
    with pytest.raises(ValueError, match="requires grad"):
        simulation.TreeLeapFrogSimulator(positions=grad, velocities=z, masses=np.ones(4))


def test_signatures_hold_the_new_entries_as_the_header_declares_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbd.h")).read(), flags=re.S)
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, f"{name} is not declared in include/nbd.h"
        want = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            kind = arg.rsplit(" ", 1)[0]
            want.append(ctypes.c_void_p if "*" in arg or kind == "nbd_stream_t" else ctype[kind])
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == want, name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    declared = sorted(set(re.findall(r"\b(nbd_[a-z0-9_]+)\s*\(", text)))
    assert sorted(_lib.SIGNATURES) == declared
