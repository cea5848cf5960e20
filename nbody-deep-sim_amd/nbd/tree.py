"""Typed wrappers over the tree-code entry points of libnbd_hip.so (csrc/tree_force.hip).

build() orders the bodies along a Morton curve and fills a workspace with the sorted bodies and every node of the implicit
octree-like hierarchy over that order; accel(), potential() and accel_potential() walk it. All check dtype / shape / contiguity on the host and launch on
torch's current stream; none allocates unless the caller leaves an output out.
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


def _walk_checks(ws: torch.Tensor, n: int, counters: torch.Tensor | None):
    _chk(ws, None, "workspace", torch.uint8)
    if _nbytes(ws) < workspace_bytes(n):
        raise _lib.NbdError(f"workspace: {_nbytes(ws)} bytes, the tree of {n} bodies takes {workspace_bytes(n)}")
    if counters is not None:
        _chk(counters, (2,), "counters", torch.int64)


def accel(ws: torch.Tensor, n: int, theta: float, softening_sq: float, g_const: float, quadrupole: bool = True,
          out: torch.Tensor | None = None, counters: torch.Tensor | None = None) -> torch.Tensor:
    """acc (n,3) in the caller's order from the tree build() left in `ws`. counters: None or a (2,) int64 device tensor
    that receives {accepted cells, rejected level-0 nodes} summed over the target groups."""
    _walk_checks(ws, n, counters)
    if out is None:
        out = torch.empty((n, 3), dtype=torch.float32, device=ws.device)
    _chk(out, (n, 3), "acc_out")
    _lib.launch("nbd_tree_accel_f32", ws.device, ws.data_ptr(), int(n), float(theta), float(softening_sq), float(g_const),
                int(bool(quadrupole)), out.data_ptr(), _lib.ptr(counters))
    return out


def potential(ws: torch.Tensor, n: int, theta: float, softening_sq: float, g_const: float, quadrupole: bool = True,
              out: torch.Tensor | None = None, counters: torch.Tensor | None = None) -> torch.Tensor:
    """phi (n,) float64 in the caller's order from the tree build() left in `ws`: the potential whose gradient accel()
    is, summed over the same accepted cells and rejected level-0 nodes (fp32 terms, fp64 sums). counters as in accel()."""
    _walk_checks(ws, n, counters)
    if out is None:
        out = torch.empty((n,), dtype=torch.float64, device=ws.device)
    _chk(out, (n,), "phi_out", torch.float64)
    _lib.launch("nbd_tree_potential_f32", ws.device, ws.data_ptr(), int(n), float(theta), float(softening_sq),
                float(g_const), int(bool(quadrupole)), out.data_ptr(), _lib.ptr(counters))
    return out


def accel_potential(ws: torch.Tensor, n: int, theta: float, softening_sq: float, g_const: float, quadrupole: bool = True,
                    out: tuple | None = None, counters: torch.Tensor | None = None) -> tuple:
    """(acc, phi) from ONE walk: acc bit for bit accel()'s, phi bit for bit potential()'s. out: None or (acc, phi)."""
    _walk_checks(ws, n, counters)
    acc, phi = out if out is not None else (None, None)
    if acc is None:
        acc = torch.empty((n, 3), dtype=torch.float32, device=ws.device)
    if phi is None:
        phi = torch.empty((n,), dtype=torch.float64, device=ws.device)
    _chk(acc, (n, 3), "acc_out"); _chk(phi, (n,), "phi_out", torch.float64)
    _lib.launch("nbd_tree_accel_potential_f32", ws.device, ws.data_ptr(), int(n), float(theta), float(softening_sq),
                float(g_const), int(bool(quadrupole)), acc.data_ptr(), phi.data_ptr(), _lib.ptr(counters))
    return acc, phi
