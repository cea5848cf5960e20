"""Typed wrappers over the tree-code entry points of libnbd_hip.so (csrc/tree_force.hip).

build() orders the bodies along a Morton curve and fills a workspace with the sorted bodies and every node of the implicit
octree-like hierarchy over that order; walk() walks it for a, phi or both, over all target groups, a range of them or a
list of bodies, and holds every check, allocation and launch of a walk: accel(), potential(), accel_potential() and the
*_groups() / accel_active() names below are each one call of it. All check dtype / shape / contiguity on the host and
launch on torch's current stream; none allocates unless the caller leaves an output out. views() shows what a build left:
the order, the sorted bodies and the node records, as views of the workspace.

For several ranks ("Several ranks"): build_posm() is build() from packed {x, y, z, m} rows, accel_groups(),
potential_groups() and accel_potential_groups() walk the target groups [group_lo, group_hi) of groups(n) alone and leave
their rows in TREE order, scatter() places tree-order rows into a range of the caller's order.

For block timesteps ("Block timesteps"): select_active() compacts the flagged bodies into a list of sorted
positions, accel_active() walks the tree for the listed bodies alone and writes only their rows; block_*() are the O(N)
stages of csrc/tree_block.hip.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .direct import _chk, alloc_bytes


def plan(n: int) -> dict:
    """{"levels", "nodes_total"} of the hierarchy over n bodies (host arithmetic; NbdUnsupported above 2**24 bodies)."""
    levels, total = ctypes.c_int(), ctypes.c_int()
    _lib.call("nbd_tree_plan", int(n), levels, total)
    return {"levels": levels.value, "nodes_total": total.value}


def workspace_bytes(n: int) -> int:
    return _lib.lib().nbd_tree_workspace_bytes(int(n))


def workspace(n: int, device) -> torch.Tensor:
    """The buffer build() fills and the walks read for n bodies (the radix sort's scratch included)."""
    plan(n)                                    # refuses what the library refuses, with its message
    return alloc_bytes(workspace_bytes(n), device)


def _nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


def build(pos: torch.Tensor, mass: torch.Tensor, ws: torch.Tensor, order: torch.Tensor | None = None) -> torch.Tensor:
    """Sort pos (n,3) / mass (n,) by Morton key and build every node into `ws`; returns order (n,) int32: order[k] is the
    caller's index of the k-th body of the tree order."""
    n = pos.shape[0]
    _chk(pos, (n, 3), "pos"); _chk(mass, (n,), "mass")
    _chk(ws, None, "workspace", torch.uint8)
    if order is None:
        order = torch.empty((n,), dtype=torch.int32, device=pos.device)
    _chk(order, (n,), "order", torch.int32)
    _lib.launch("nbd_tree_build_f32", pos.device, pos.data_ptr(), mass.data_ptr(), n, order.data_ptr(), ws.data_ptr(),
                _nbytes(ws))
    return order


GROUP = 64                       # sorted bodies per target group (one wave of the walk)


def groups(n: int) -> int:
    """Target groups of the walk over n bodies: ceil(n / 64)."""
    return (int(n) + GROUP - 1) // GROUP


def _ws_checks(ws: torch.Tensor, n: int):
    _chk(ws, None, "workspace", torch.uint8)
    if _nbytes(ws) < workspace_bytes(n):
        raise _lib.NbdError(f"workspace: {_nbytes(ws)} bytes, the tree of {n} bodies takes {workspace_bytes(n)}")


def walk(ws: torch.Tensor, n: int, theta: float, softening_sq: float, g_const: float, quadrupole: bool = True, *,
         acc: bool = True, phi: bool = False, groups: tuple | None = None, active: tuple | None = None,
         out: tuple | None = None, counters: torch.Tensor | None = None) -> tuple:
    """One walk of the tree build() left in `ws` -> (acc or None, phi or None): the acceleration (n,3) float32, the
    potential (n,) float64 whose gradient it is, or both from ONE walk, in the caller's order. Every simulator and every
    named wrapper below goes through here.
    groups (lo, hi): of the target groups [lo, hi) of groups(n) alone; the outputs then hold (hi - lo) 64 rows in TREE
    order, row t = sorted body 64 lo + t, the rows behind body n - 1 as 0. An empty range launches nothing.
    active (list, n_act): of the n_act sorted positions of `list` (select_active()'s) alone; acc is in the caller's order
    and only the rows order[list[t]] are written (an acc allocated here holds 0 elsewhere). The list has no phi.
    out: None or (acc, phi), None for what is to be allocated. counters: None or a (2,) int64 device tensor that receives
    {accepted cells, rejected level-0 nodes} summed over the walked groups (0 where nothing is walked)."""
    n, acc, phi, ranged, listed = int(n), bool(acc), bool(phi), groups is not None, active is not None
    if not (acc or phi):
        raise _lib.NbdError("walk: nothing asked for, give acc, phi or both")
    if ranged and listed:
        raise _lib.NbdError("walk: give groups or active, not both")
    if listed and phi:
        raise _lib.NbdError("walk: the listed walk sums the acceleration alone, there is no phi of a list")
    _ws_checks(ws, n)
    if counters is not None:
        _chk(counters, (2,), "counters", torch.int64)
    rows, tag, head = n, "", (ws.data_ptr(), n)
    if ranged:
        (lo, hi), n_groups = (int(g) for g in groups), (n + GROUP - 1) // GROUP
        if not 0 <= lo <= hi <= n_groups:
            raise _lib.NbdError(f"groups [{lo}, {hi}) outside [0, {n_groups}] of {n} bodies")
        if lo == hi and counters is not None:
            counters.zero_()
        rows, tag, head = (hi - lo) * GROUP, "_sorted", head + (lo, hi)
    if listed:
        lst, n_act = active[0], int(active[1])
        if lst is not None:
            _chk(lst, None, "list", torch.int32)
            if lst.dim() != 1 or lst.shape[0] < n_act:
                raise _lib.NbdError(f"list: {n_act} entries asked for, it holds {tuple(lst.shape)}")
        head = (ws.data_ptr(), _nbytes(ws), n, _lib.ptr(lst), n_act)
    a, p = out if out is not None else (None, None)
    if acc:
        if a is None:                            # (the unlisted rows of a listed walk are not written: they are 0)
            a = (torch.zeros if listed else torch.empty)((rows, 3), dtype=torch.float32, device=ws.device)
        _chk(a, (rows, 3), f"acc{tag}_out")
    if phi:
        if p is None:
            p = torch.empty((rows,), dtype=torch.float64, device=ws.device)
        _chk(p, (rows,), f"phi{tag}_out", torch.float64)
    outs = ((a,) if acc else ()) + ((p,) if phi else ())
    entry = "_".join(("accel",) * acc + ("potential",) * phi + ("groups",) * ranged + ("active",) * listed)
    _lib.launch(f"nbd_tree_{entry}_f32", ws.device, *head, float(theta), float(softening_sq), float(g_const),
                int(bool(quadrupole)), *(t.data_ptr() for t in outs), _lib.ptr(counters))
    return (a if acc else None), (p if phi else None)


def views(ws: torch.Tensor, n: int) -> dict:
    """What build() left in `ws` and the walks read, as zero-copy views of it (nbd_tree_regions): {"order": (n,) int32,
    sorted position -> caller's index; "posm": (n rounded up to 64, 4) float32, the sorted rows {x, y, z, m}, zeros
    behind body n - 1; "nodes": one (count, 12) float32 per level, level 0 first, a row {c (3), s, M, Qxx, Qxy, Qxz,
    Qyy, Qyz, Qzz, 0}}."""
    n = int(n)
    offs = [ctypes.c_size_t() for _ in range(3)]
    _lib.call("nbd_tree_regions", n, *offs)
    if n == 0:
        return {"order": ws[:0].view(torch.int32), "posm": ws[:0].view(torch.float32).view(0, 4), "nodes": []}
    _ws_checks(ws, n)
    order_off, posm_off, nodes_off = (o.value for o in offs)
    rows = groups(n) * GROUP
    counts = [(n + 7) // 8]
    while counts[-1] > 1:
        counts.append((counts[-1] + 7) // 8)
    assert len(counts) == plan(n)["levels"] and sum(counts) == plan(n)["nodes_total"]
    nodes, at = [], nodes_off
    for count in counts:
        nodes.append(ws[at:at + 48 * count].view(torch.float32).view(count, 12))
        at += 48 * count
    return {"order": ws[order_off:order_off + 4 * n].view(torch.int32),
            "posm": ws[posm_off:posm_off + 16 * rows].view(torch.float32).view(rows, 4), "nodes": nodes}


def accel(ws: torch.Tensor, n: int, theta: float, softening_sq: float, g_const: float, quadrupole: bool = True,
          out: torch.Tensor | None = None, counters: torch.Tensor | None = None) -> torch.Tensor:
    """acc (n,3) in the caller's order from the tree build() left in `ws`. counters: None or a (2,) int64 device tensor
    that receives {accepted cells, rejected level-0 nodes} summed over the target groups."""
    return walk(ws, n, theta, softening_sq, g_const, quadrupole, out=(out, None), counters=counters)[0]


def potential(ws: torch.Tensor, n: int, theta: float, softening_sq: float, g_const: float, quadrupole: bool = True,
              out: torch.Tensor | None = None, counters: torch.Tensor | None = None) -> torch.Tensor:
    """phi (n,) float64 in the caller's order from the tree build() left in `ws`: the potential whose gradient accel()
    is, summed over the same accepted cells and rejected level-0 nodes (fp32 terms, fp64 sums). counters as in accel()."""
    return walk(ws, n, theta, softening_sq, g_const, quadrupole, acc=False, phi=True, out=(None, out),
                counters=counters)[1]


def accel_potential(ws: torch.Tensor, n: int, theta: float, softening_sq: float, g_const: float, quadrupole: bool = True,
                    out: tuple | None = None, counters: torch.Tensor | None = None) -> tuple:
    """(acc, phi) from ONE walk: acc bit for bit accel()'s, phi bit for bit potential()'s. out: None or (acc, phi)."""
    return walk(ws, n, theta, softening_sq, g_const, quadrupole, phi=True, out=out, counters=counters)


# ---------------------------------------------------------------- a range of the target groups (several ranks)
def build_posm(posm: torch.Tensor, n: int, ws: torch.Tensor, order: torch.Tensor | None = None) -> torch.Tensor:
    """build() from packed rows: posm (>= n, 4) {x, y, z, m} (what pack_posm, kick_drift and the all-gather of a sharded
    step leave). order and everything the walks read are bit for bit build()'s for the same values."""
    n = int(n)
    _chk(posm, None, "posm")
    if posm.dim() != 2 or posm.shape[1] != 4 or posm.shape[0] < n:
        raise _lib.NbdError(f"posm: expected at least ({n}, 4) rows, got {tuple(posm.shape)}")
    _chk(ws, None, "workspace", torch.uint8)
    if order is None:
        order = torch.empty((n,), dtype=torch.int32, device=posm.device)
    _chk(order, (n,), "order", torch.int32)
    _lib.launch("nbd_tree_build_posm_f32", posm.device, posm.data_ptr(), n, order.data_ptr(), ws.data_ptr(), _nbytes(ws))
    return order


def accel_groups(ws: torch.Tensor, n: int, group_lo: int, group_hi: int, theta: float, softening_sq: float,
                 g_const: float, quadrupole: bool = True, out: torch.Tensor | None = None,
                 counters: torch.Tensor | None = None) -> torch.Tensor:
    """accel() for the target groups [group_lo, group_hi) alone -> ((group_hi - group_lo) 64, 3) in TREE order: row t is
    sorted body 64 group_lo + t and equals accel()'s row order[64 group_lo + t] bit for bit; rows behind body n - 1 are
    0. counters: the sums over these groups."""
    return walk(ws, n, theta, softening_sq, g_const, quadrupole, groups=(group_lo, group_hi), out=(out, None),
                counters=counters)[0]


def potential_groups(ws: torch.Tensor, n: int, group_lo: int, group_hi: int, theta: float, softening_sq: float,
                     g_const: float, quadrupole: bool = True, out: torch.Tensor | None = None,
                     counters: torch.Tensor | None = None) -> torch.Tensor:
    """potential() for the target groups [group_lo, group_hi) alone -> ((group_hi - group_lo) 64,) float64 in tree order."""
    return walk(ws, n, theta, softening_sq, g_const, quadrupole, acc=False, phi=True, groups=(group_lo, group_hi),
                out=(None, out), counters=counters)[1]


def accel_potential_groups(ws: torch.Tensor, n: int, group_lo: int, group_hi: int, theta: float, softening_sq: float,
                           g_const: float, quadrupole: bool = True, out: tuple | None = None,
                           counters: torch.Tensor | None = None) -> tuple:
    """(acc, phi) of the target groups [group_lo, group_hi) from ONE walk, both in tree order. out: None or (acc, phi)."""
    return walk(ws, n, theta, softening_sq, g_const, quadrupole, phi=True, groups=(group_lo, group_hi), out=out,
                counters=counters)


def scatter(ws: torch.Tensor, n: int, lo: int, hi: int, acc_sorted: torch.Tensor | None = None,
            phi_sorted: torch.Tensor | None = None, out: tuple | None = None) -> tuple:
    """Tree order -> the bodies [lo, hi) of the caller's order, by the order build() left in `ws`: acc (hi - lo, 3) from
    acc_sorted (64 groups(n), 3) and / or phi (hi - lo,) from phi_sorted (64 groups(n),). Returns (acc, phi), None for
    what was not given. out: None or (acc, phi)."""
    _ws_checks(ws, n)
    if not 0 <= lo <= hi <= n:
        raise _lib.NbdError(f"bodies [{lo}, {hi}) outside [0, {n}]")
    if acc_sorted is None and phi_sorted is None:
        raise _lib.NbdError("scatter: give acc_sorted, phi_sorted or both")
    rows, dev = groups(n) * GROUP, ws.device
    acc, phi = out if out is not None else (None, None)
    if acc_sorted is not None:
        _chk(acc_sorted, (rows, 3), "acc_sorted")
        if acc is None:
            acc = torch.empty((hi - lo, 3), dtype=torch.float32, device=dev)
        _chk(acc, (hi - lo, 3), "acc_out")
    if phi_sorted is not None:
        _chk(phi_sorted, (rows,), "phi_sorted", torch.float64)
        if phi is None:
            phi = torch.empty((hi - lo,), dtype=torch.float64, device=dev)
        _chk(phi, (hi - lo,), "phi_out", torch.float64)
    _lib.launch("nbd_tree_scatter_f32", dev, ws.data_ptr(), int(n), int(lo), int(hi), _lib.ptr(acc_sorted),
                _lib.ptr(phi_sorted), _lib.ptr(acc if acc_sorted is not None else None),
                _lib.ptr(phi if phi_sorted is not None else None))
    return (acc if acc_sorted is not None else None), (phi if phi_sorted is not None else None)


# ---------------------------------------------------------------- listed targets (block timesteps)
def active_workspace_bytes(n: int) -> int:
    return _lib.lib().nbd_tree_active_workspace_bytes(int(n))


def active_workspace(n: int, device) -> torch.Tensor:
    """The buffer select_active() works in for n bodies: the list, its count, the flags in tree order and the
    compaction's scratch."""
    plan(n)
    return alloc_bytes(active_workspace_bytes(n), device)


def _active_views(active_ws: torch.Tensor, n: int) -> tuple:
    """(list (n,), n_act (1,)) int32 views of the active workspace: the list at byte 0, the count at 4 n rounded up to 256."""
    ints = active_ws.view(torch.int32)
    at = (4 * n + 255) // 256 * 64
    return ints[:n], ints[at:at + 1]


def select_active(ws: torch.Tensor, n: int, flags: torch.Tensor, list_out: torch.Tensor | None = None, *,
                  active_ws: torch.Tensor | None = None, n_act_out: torch.Tensor | None = None) -> tuple:
    """(list, n_act): list[:n_act] = the sorted positions k, ascending, with flags[order[k]] != 0 -- the flagged bodies in
    tree order, `order` the one build() left in `ws`. flags (n,) int32 in the caller's order. An ordered compaction: the
    same list from run to run. n_act is a (1,) int32 DEVICE tensor: the caller reads it back. active_ws: the buffer of
    active_workspace(n) (None: one is allocated here; with it given nothing is allocated and nothing synchronises).
    list_out (n,) int32 and n_act_out (1,) int32: None for the active workspace's own."""
    n = int(n)
    _chk(flags, (n,), "flags", torch.int32)
    if n == 0:
        return (list_out if list_out is not None else torch.empty((0,), dtype=torch.int32, device=flags.device),
                n_act_out.zero_() if n_act_out is not None else torch.zeros((1,), dtype=torch.int32, device=flags.device))
    _ws_checks(ws, n)
    if active_ws is None:
        active_ws = active_workspace(n, ws.device)
    _chk(active_ws, None, "active workspace", torch.uint8)
    own_list, own_count = _active_views(active_ws, n) if _nbytes(active_ws) >= active_workspace_bytes(n) else (None, None)
    if list_out is not None:
        _chk(list_out, (n,), "list_out", torch.int32)
    if n_act_out is not None:
        _chk(n_act_out, (1,), "n_act_out", torch.int32)
    _lib.launch("nbd_tree_select_active", ws.device, ws.data_ptr(), n, flags.data_ptr(), _lib.ptr(list_out),
                _lib.ptr(n_act_out), active_ws.data_ptr(), _nbytes(active_ws))
    return (list_out if list_out is not None else own_list), (n_act_out if n_act_out is not None else own_count)


def accel_active(ws: torch.Tensor, n: int, list: torch.Tensor, n_act: int, theta: float, softening_sq: float,
                 g_const: float, quadrupole: bool = True, out: torch.Tensor | None = None,
                 counters: torch.Tensor | None = None) -> torch.Tensor:
    """The tree force on the n_act bodies of `list` (select_active()'s; n_act the host's copy of its count) against the
    tree of all n bodies in `ws`: target groups of 64 consecutive list entries, each with the box of its own bodies.
    Written: the rows order[list[t]], t < n_act, of out (n,3) in the caller's order, and NO other row (out None: the others
    are 0). With every body listed, out and counters equal accel()'s bit for bit. n_act = 0 launches nothing and zeroes
    the counters."""
    return walk(ws, n, theta, softening_sq, g_const, quadrupole, active=(list, n_act), out=(out, None),
                counters=counters)[0]


# ---------------------------------------------------------------- the O(N) stages of a block step (csrc/tree_block.hip)
BLOCK_SCHED_INTS = 8             # NBD_TBLOCK_SCHED_INTS: {t_next, n_act, clamped, t_cur, the min being reduced, ...}


def block_init_levels(acc: torch.Tensor, dt: float, eta: float, softening: float, max_level: int, ticks: torch.Tensor,
                      levels: torch.Tensor, sched: torch.Tensor) -> None:
    """levels = the criterion's on acc (n,3), ticks = 0; sched[2] grows by the levels wanted deeper than max_level."""
    n = acc.shape[0]
    _chk(acc, (n, 3), "acc"); _chk(ticks, (n,), "ticks", torch.int32); _chk(levels, (n,), "levels", torch.int32)
    _chk(sched, (BLOCK_SCHED_INTS,), "sched", torch.int32)
    _lib.launch("nbd_tblock_init_levels", acc.device, acc.data_ptr(), n, float(dt), float(eta), float(softening),
                int(max_level), ticks.data_ptr(), levels.data_ptr(), sched.data_ptr())


def block_open(vel, acc, levels, ticks, residual, max_level: int, dt: float, sched) -> None:
    """The opening kick of an interval: v += a h_i / 2 for every body, ticks = 0, the drift's residual (n,3) = 0."""
    n = vel.shape[0]
    _chk(vel, (n, 3), "vel"); _chk(acc, (n, 3), "acc"); _chk(residual, (n, 3), "residual")
    _chk(ticks, (n,), "ticks", torch.int32); _chk(levels, (n,), "levels", torch.int32)
    _lib.launch("nbd_tblock_open", vel.device, vel.data_ptr(), acc.data_ptr(), levels.data_ptr(), ticks.data_ptr(),
                residual.data_ptr(), n, int(max_level), float(dt), sched.data_ptr())


def block_drift(pos, vel, mass, levels, ticks, residual, max_level: int, dt: float, sched, posm) -> None:
    """t_next = min (ticks + d) on the device; every body drifts there (a compensated sum: `residual` (n,3) carries the
    rounding of a position between the block steps of an interval); posm = the packed rows build_posm() takes."""
    n = pos.shape[0]
    _chk(pos, (n, 3), "pos"); _chk(vel, (n, 3), "vel"); _chk(mass, (n,), "mass"); _chk(residual, (n, 3), "residual")
    _chk(ticks, (n,), "ticks", torch.int32); _chk(levels, (n,), "levels", torch.int32)
    _chk(posm, None, "posm")
    if posm.dim() != 2 or posm.shape[1] != 4 or posm.shape[0] < _lib.lib().nbd_posm_padded_len(n):
        raise _lib.NbdError(f"posm: need (>= padded_len({n}), 4), got {tuple(posm.shape)}")
    _lib.launch("nbd_tblock_drift", pos.device, pos.data_ptr(), vel.data_ptr(), mass.data_ptr(), levels.data_ptr(),
                ticks.data_ptr(), residual.data_ptr(), n, int(max_level), float(dt), sched.data_ptr(), posm.data_ptr())


def block_flag(levels, ticks, max_level: int, sched, flags) -> None:
    """flags[i] = body i is due at t_next; sched[0] = t_next."""
    n = levels.shape[0]
    _chk(ticks, (n,), "ticks", torch.int32); _chk(levels, (n,), "levels", torch.int32)
    _chk(flags, (n,), "flags", torch.int32)
    _lib.launch("nbd_tblock_flag", levels.device, levels.data_ptr(), ticks.data_ptr(), n, int(max_level), sched.data_ptr(),
                flags.data_ptr())


def block_close(vel, acc, flags, levels, ticks, max_level: int, dt: float, eta: float, softening: float, sched) -> None:
    """The flagged bodies: closing kick, new level, and (inside the interval) the opening kick of the next step."""
    n = vel.shape[0]
    _chk(vel, (n, 3), "vel"); _chk(acc, (n, 3), "acc"); _chk(flags, (n,), "flags", torch.int32)
    _chk(ticks, (n,), "ticks", torch.int32); _chk(levels, (n,), "levels", torch.int32)
    _lib.launch("nbd_tblock_close", vel.device, vel.data_ptr(), acc.data_ptr(), flags.data_ptr(), levels.data_ptr(),
                ticks.data_ptr(), n, int(max_level), float(dt), float(eta), float(softening), sched.data_ptr())
