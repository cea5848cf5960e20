"""Typed wrappers over the direct-force entry points of libnbd_hip.so.

Every function takes torch CUDA(=HIP) tensors, checks dtype/shape/contiguity on the host (a
wrong shape must never reach a hand-written kernel) and launches on torch's current stream.
A float64 wrapper that repeats a float32 one is a second binding of the same private body: the
body takes the dtype, the C entry's name and, where an error names the caller, the public name.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _lib


def _chk(t: torch.Tensor, shape, name: str, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.NbdError(f"{name}: expected a CUDA/HIP tensor (no CPU fallback on this path)")
    if t.dtype != dtype or not t.is_contiguous():
        raise _lib.NbdError(f"{name}: expected contiguous {dtype}, got {t.dtype} contiguous={t.is_contiguous()}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise _lib.NbdError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")


def _chk_n3(dtype, n: int, names, *tensors):
    """The tensors, under the names the messages use, are all (n, 3) of `dtype`. (Positional: this runs in every eager
    step, and a call with keywords costs a measurable part of one.)"""
    shape = (n, 3)
    for name, t in zip(names, tensors):
        _chk(t, shape, name, dtype)


def _chk_together(who: str, text: str, dtype, n: int, names, *tensors):
    """Optional (n, 3) inputs that come together: all of them, and then checked, or none; else '`who`: give `text`'."""
    given = [t is not None for t in tensors]
    if any(given) != all(given):
        raise _lib.NbdError(f"{who}: give {text}")
    if given[0]:
        _chk_n3(dtype, n, names, *tensors)


def _chk_min_rows(t: torch.Tensor, rows: int, width: int, name: str, dtype=torch.float32):
    """An array of `width`-element rows of `dtype` that holds at least `rows` of them."""
    _chk(t, None, name, dtype)
    if t.dim() != 2 or t.shape[1] != width or t.shape[0] < rows:
        raise _lib.NbdError(f"{name}: need >= {rows} rows of {width}, got {tuple(t.shape)}")


def padded_len(n: int) -> int:
    return _lib.lib().nbd_posm_padded_len(int(n))


def _chk_packed(dtype, pos_rows, vel_rows, n: int):
    """The packed (padded_len(n), 4) rows of n bodies in `dtype`; vel_rows None where the entry takes none."""
    for t, name in zip((pos_rows, vel_rows), ("posm", "velp") if dtype == torch.float32 else ("posd", "veld")):
        if t is not None:
            _chk(t, (padded_len(n), 4), name, dtype)


_PLAN3 = ("groups", "slabs", "chunks_per_wave")
_PLAN4 = ("slabs_local", "chunks_per_wave_local", "slabs_remote", "chunks_per_wave_remote")


def _plan(entry: str, keys, *args) -> dict:
    """The ints a *_plan entry writes behind `args`, under `keys`."""
    out = [ctypes.c_int() for _ in keys]
    _lib.call(entry, *args, *out)
    return {k: v.value for k, v in zip(keys, out)}


def accel_plan(n_src: int, n_tgt: int) -> dict:
    return _plan("nbd_accel_plan", _PLAN3, n_src, n_tgt)


def alloc_posm(n: int, device) -> torch.Tensor:
    return torch.empty((padded_len(n), 4), dtype=torch.float32, device=device)


def alloc_bytes(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def pack_posm(pos: torch.Tensor, mass: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    n = pos.shape[0]
    _chk(pos, (n, 3), "pos"); _chk(mass, (n,), "mass")
    if out is None:
        out = alloc_posm(n, pos.device)
    _chk(out, (padded_len(n), 4), "posm")
    _lib.launch("nbd_pack_posm_f32", pos.device, pos.data_ptr(), mass.data_ptr(), n, out.data_ptr())
    return out


def accel_workspace(n_src: int, n_tgt: int, device) -> torch.Tensor:
    return alloc_bytes(_lib.lib().nbd_accel_workspace_bytes(n_src, n_tgt), device)


def accel(posm_src: torch.Tensor, n_src: int, posm_tgt: torch.Tensor, n_tgt: int, tgt_offset: int,
          softening_sq: float, g_const: float, out: torch.Tensor | None = None,
          workspace: torch.Tensor | None = None) -> torch.Tensor:
    """acc (n_tgt,3) of targets posm_tgt[:n_tgt] under sources posm_src[:n_src] (simulation.py:71-89)."""
    _chk(posm_src, (padded_len(n_src), 4), "posm_src") if n_src > 0 else None
    _chk_min_rows(posm_tgt, n_tgt, 4, "posm_tgt")
    dev = posm_tgt.device
    if out is None:
        out = torch.empty((n_tgt, 3), dtype=torch.float32, device=dev)
    _chk(out, (n_tgt, 3), "acc_out")
    need = _lib.lib().nbd_accel_workspace_bytes(n_src, n_tgt)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = alloc_bytes(need, dev)
    _lib.launch("nbd_accel_f32", dev, posm_src.data_ptr() if n_src > 0 else None, n_src, posm_tgt.data_ptr(), n_tgt,
                tgt_offset, float(softening_sq), float(g_const), out.data_ptr(), workspace.data_ptr(),
                workspace.numel() * workspace.element_size())
    return out


def accel_tuned(posm_src: torch.Tensor, n_src: int, posm_tgt: torch.Tensor, n_tgt: int, tgt_offset: int,
                softening_sq: float, g_const: float, slabs: int, variant: int = 0, exclude=(0, 0),
                out: torch.Tensor | None = None, workspace: torch.Tensor | None = None) -> torch.Tensor:
    """`accel` with an explicit launch geometry and an optional excluded source range (tuning hook)."""
    _chk(posm_src, (padded_len(n_src), 4), "posm_src")
    _chk_min_rows(posm_tgt, n_tgt, 4, "posm_tgt")
    dev = posm_tgt.device
    if out is None:
        out = torch.empty((n_tgt, 3), dtype=torch.float32, device=dev)
    _chk(out, (n_tgt, 3), "acc_out")
    need = _lib.lib().nbd_accel_tuned_workspace_bytes(n_tgt, slabs)
    if workspace is None or _nbytes(workspace) < need:
        workspace = alloc_bytes(need, dev)
    _lib.launch("nbd_accel_tuned_f32", dev, posm_src.data_ptr(), n_src, int(exclude[0]), int(exclude[1]),
                posm_tgt.data_ptr(), n_tgt, tgt_offset, float(softening_sq), float(g_const), out.data_ptr(),
                workspace.data_ptr(), _nbytes(workspace), int(slabs), int(variant))
    return out


def shard_plan(n_total: int, lo: int, n_local: int) -> dict:
    return _plan("nbd_shard_plan", _PLAN4, n_total, lo, n_local)


def shard_workspace(n_total: int, lo: int, n_local: int, device) -> torch.Tensor:
    return alloc_bytes(_lib.lib().nbd_shard_workspace_bytes(n_total, lo, n_local), device)


def shard_force_local(posm_local: torch.Tensor, n_local: int, n_total: int, lo: int, softening_sq: float,
                      workspace: torch.Tensor, uniform=None) -> None:
    """First launch of the sharded force: own bodies as sources (runs while the all-gather is in flight).
    uniform: the bodies' common mass (uniform_mass) -> the kernel without its per-pair mass multiply."""
    _chk(posm_local, (padded_len(n_local), 4), "posm_local")
    _lib.launch("nbd_shard_force_local_f32" if uniform is None else "nbd_shard_force_local_uniform_f32",
                posm_local.device, posm_local.data_ptr(), n_local, float(softening_sq), workspace.data_ptr(),
                _nbytes(workspace), n_total, lo)


def shard_force_remote(posm_all: torch.Tensor, n_total: int, posm_local: torch.Tensor, n_local: int, lo: int,
                       softening_sq: float, g_const: float, acc_out: torch.Tensor, vel: torch.Tensor | None,
                       c_kick: float, workspace: torch.Tensor, uniform=None) -> None:
    """Second launch: every other body as a source, then acc = G * sum(slabs) and v += c_kick * acc."""
    _chk(posm_all, (padded_len(n_total), 4), "posm_all")
    _chk(posm_local, (padded_len(n_local), 4), "posm_local")
    _chk(acc_out, (n_local, 3), "acc_out")
    if vel is not None:
        _chk(vel, (n_local, 3), "vel")
    head = (posm_all.data_ptr(), n_total, posm_local.data_ptr(), n_local, lo, float(softening_sq), float(g_const))
    tail = (acc_out.data_ptr(), _lib.ptr(vel), float(c_kick), workspace.data_ptr(), _nbytes(workspace))
    if uniform is not None:
        _lib.launch("nbd_shard_force_remote_uniform_f32", posm_all.device, *head, float(uniform), *tail)
        return
    _lib.launch("nbd_shard_force_remote_f32", posm_all.device, *head, *tail)


def f32(x: float) -> float:
    """The value torch uses when a Python double scalar meets an fp32 tensor."""
    return float(np.float32(x))


def _nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


def step_workspace(n: int, device) -> torch.Tensor:
    """Scratch of the fused step at its preferred plan (nbd_step_workspace_pref_bytes). The step reads its plan off the
    size it is handed: NBD_SYM_SLOTS=K (read here, at allocation) caps the symmetric force's partial-sum slots at K -- the
    A/B switch for measurements and the way back to the 16-slot plan (NBD_SYM_SLOTS=16); never below what the step needs."""
    L = _lib.lib()
    least, pref = L.nbd_step_workspace_bytes(n), L.nbd_step_workspace_pref_bytes(n)
    cap = os.environ.get("NBD_SYM_SLOTS")
    if cap is not None and pref > least:
        # one slot = n rows of 3 floats; the slot of the rows behind the last whole tile comes on top of the K
        pref = min(pref, (max(int(cap), 0) + (1 if n % 2048 else 0)) * n * 12)
    return alloc_bytes(max(least, pref), device)


def kick_drift(pos, vel, acc, mass, c_kick: float, c_drift: float, posm=None) -> None:
    """v += c_kick*a ; x += c_drift*v ; posm[:n] = {x,m} (simulation.py:164,166). In place."""
    n = pos.shape[0]
    _chk(pos, (n, 3), "pos"); _chk(vel, (n, 3), "vel")
    if acc is not None:
        _chk(acc, (n, 3), "acc")
    if posm is not None:
        _chk(mass, (n,), "mass")
        if posm.dtype != torch.float32 or not posm.is_contiguous() or posm.shape[0] < padded_len(n):
            raise _lib.NbdError("posm: need contiguous fp32 (>= padded_len(n), 4)")
    _lib.launch("nbd_kick_drift_f32", pos.device, pos.data_ptr(), vel.data_ptr(), _lib.ptr(acc), _lib.ptr(mass), n,
                c_kick, c_drift, _lib.ptr(posm))


def kick(vel, acc, c: float) -> None:
    n = vel.shape[0]
    _chk(vel, (n, 3), "vel"); _chk(acc, (n, 3), "acc")
    _lib.launch("nbd_kick_f32", vel.device, vel.data_ptr(), acc.data_ptr(), n, c)


def drift(pos, vel, c: float) -> None:
    n = pos.shape[0]
    _chk(pos, (n, 3), "pos"); _chk(vel, (n, 3), "vel")
    _lib.launch("nbd_drift_f32", pos.device, pos.data_ptr(), vel.data_ptr(), n, c)


def _snapshot(dtype, entry: str, pos, vel, acc, out) -> None:
    n = pos.shape[0]
    _chk_n3(dtype, n, ("pos", "vel", "acc"), pos, vel, acc)
    _chk(out, (3, n, 3), "out", dtype)
    _lib.launch(entry, pos.device, pos.data_ptr(), vel.data_ptr(), acc.data_ptr(), n, out.data_ptr())


def snapshot(pos, vel, acc, out) -> None:
    """out (3, n, 3) = [pos, vel, acc]: one launch (a slot of run()'s device ring)."""
    _snapshot(torch.float32, "nbd_snapshot_f32", pos, vel, acc, out)


def snapshot_f64(pos, vel, acc, out) -> None:
    """snapshot of a float64 state: out (3, n, 3) float64 = [pos, vel, acc], one launch."""
    _snapshot(F64, "nbd_snapshot_f64", pos, vel, acc, out)


def uniform_mass(mass: torch.Tensor):
    """The common mass as a Python float when every body has the same, finite, positive mass -- what
    nbd_leapfrog_step_uniform_f32 asks its caller to vouch for -- else None. One device read-back: call it once."""
    if mass.numel() == 0:
        return None
    lo, hi = torch.aminmax(mass)
    lo, hi = float(lo), float(hi)
    return lo if (lo == hi and lo > 0.0 and lo != float("inf")) else None


def leapfrog_step(pos, vel, acc_in, acc_out, mass, dt_half: float, dt: float, softening_sq: float,
                  g_const: float, posm, workspace, ev_begin=None, ev_end=None, uniform=None) -> None:
    """One fused step; ev_begin/ev_end: optional torch.cuda.Event (already recorded once, so the
    handle exists) recorded around the force kernel -- bench.py's roofline hook. uniform: the bodies' common mass
    (uniform_mass(mass)) -> the force kernel without its per-pair mass multiply (nbd_leapfrog_step_uniform_f32)."""
    n = pos.shape[0]
    _chk_n3(torch.float32, n, ("pos", "vel", "acc_in", "acc_out"), pos, vel, acc_in, acc_out)
    _chk(mass, (n,), "mass"); _chk(posm, (padded_len(n), 4), "posm")
    events = (None if ev_begin is None else ev_begin.cuda_event, None if ev_end is None else ev_end.cuda_event)
    if uniform is not None:
        _lib.launch("nbd_leapfrog_step_uniform_f32", pos.device, pos.data_ptr(), vel.data_ptr(), acc_in.data_ptr(),
                    acc_out.data_ptr(), mass.data_ptr(), float(uniform), n, dt_half, dt, softening_sq, g_const,
                    posm.data_ptr(), workspace.data_ptr(), _nbytes(workspace), after=events)
        return
    # the failure has always been reported under the name of the entry without events; callers may match on that text
    _lib.launch("nbd_leapfrog_step_ev_f32", pos.device, pos.data_ptr(), vel.data_ptr(), acc_in.data_ptr(),
                acc_out.data_ptr(), mass.data_ptr(), n, dt_half, dt, softening_sq, g_const, posm.data_ptr(),
                workspace.data_ptr(), _nbytes(workspace), after=events, what="nbd_leapfrog_step_f32")


def euler_step(pos, vel, acc_out, mass, dt: float, softening_sq: float, g_const: float, posm,
               workspace) -> None:
    n = pos.shape[0]
    _chk_n3(torch.float32, n, ("pos", "vel", "acc_out"), pos, vel, acc_out)
    _chk(mass, (n,), "mass"); _chk(posm, (padded_len(n), 4), "posm")
    _lib.launch("nbd_euler_step_f32", pos.device, pos.data_ptr(), vel.data_ptr(), acc_out.data_ptr(), mass.data_ptr(),
                n, dt, softening_sq, g_const, posm.data_ptr(), workspace.data_ptr(), _nbytes(workspace))


def _energy_out(dtype, rows, vel, n: int, out_uk):
    """The checks energy and energy_f64 share; out_uk, new when None."""
    _chk_packed(dtype, rows, None, n); _chk(vel, (n, 3), "vel", dtype)
    if out_uk is None:
        out_uk = torch.empty(2, dtype=torch.float64, device=vel.device)
    _chk(out_uk, (2,), "out_uk", torch.float64)
    return out_uk


def energy(posm, vel, n: int, softening: float, g_const: float, out_uk=None, workspace=None):
    """Device double[2] = {U, K} (simulation.py:91-115); asynchronous."""
    out_uk = _energy_out(torch.float32, posm, vel, n, out_uk)
    need = _lib.lib().nbd_energy_workspace_bytes(n)
    if workspace is None or _nbytes(workspace) < need:
        workspace = alloc_bytes(need, vel.device)
    _lib.launch("nbd_energy_f32", vel.device, posm.data_ptr(), vel.data_ptr(), n, softening, g_const,
                out_uk.data_ptr(), workspace.data_ptr(), _nbytes(workspace))
    return out_uk


# ---------------------------------------------------------------- consistent-potential diagnostics (csrc/direct_diag.hip)
INVARIANT_ROW = 16              # doubles per row: {M, C (3), P (3), L (3), K, U, E, Q, 0, 0}


def potential_workspace(n_src: int, n_tgt: int, device) -> torch.Tensor:
    return alloc_bytes(_lib.lib().nbd_potential_workspace_bytes(int(n_src), int(n_tgt)), device)


def potential(posm_src: torch.Tensor, n_src: int, posm_tgt: torch.Tensor, n_tgt: int, tgt_offset: int,
              softening_sq: float, g_const: float, out: torch.Tensor | None = None,
              workspace: torch.Tensor | None = None) -> torch.Tensor:
    """phi (n_tgt,) float64 of targets posm_tgt[:n_tgt] under sources posm_src[:n_src]:
    phi_i = -G sum_{j != i} m_j (|r_ij|^2 + eps^2)^(-1/2), the potential the force of `accel` derives from (j == tgt_offset
    + i excluded by index). Asynchronous, deterministic."""
    _chk(posm_src, (padded_len(n_src), 4), "posm_src") if n_src > 0 else None
    _chk_min_rows(posm_tgt, n_tgt, 4, "posm_tgt")
    dev = posm_tgt.device
    if out is None:
        out = torch.empty((n_tgt,), dtype=torch.float64, device=dev)
    _chk(out, (n_tgt,), "phi_out", torch.float64)
    need = _lib.lib().nbd_potential_workspace_bytes(n_src, n_tgt)
    if workspace is None or _nbytes(workspace) < need:
        workspace = alloc_bytes(need, dev)
    _lib.launch("nbd_potential_f32", dev, posm_src.data_ptr() if n_src > 0 else None, n_src, posm_tgt.data_ptr(), n_tgt,
                int(tgt_offset), float(softening_sq), float(g_const), out.data_ptr(), workspace.data_ptr(),
                _nbytes(workspace))
    return out


def invariants(posm, vel, phi, n: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """Device double[16] = {M, C, P, L, K, U, E, Q, 0, 0} of the n bodies of posm / vel with their potentials phi (as
    `potential` returns them); every product in fp64 from the fp32 state, fixed summation order. Asynchronous."""
    _chk(posm, (padded_len(n), 4), "posm"); _chk(vel, (n, 3), "vel"); _chk(phi, (n,), "phi", torch.float64)
    dev = vel.device
    if out is None:
        out = torch.empty(INVARIANT_ROW, dtype=torch.float64, device=dev)
    _chk(out, (INVARIANT_ROW,), "out_row", torch.float64)
    _lib.launch("nbd_invariants_f64", dev, posm.data_ptr(), vel.data_ptr(), phi.data_ptr(), n, out.data_ptr())
    return out


# ---------------------------------------------------------------- 4th-order Hermite integrator (csrc/direct_hermite.hip)
def hermite_workspace(n: int, device) -> torch.Tensor:
    return alloc_bytes(_lib.lib().nbd_hermite_workspace_bytes(int(n)), device)


def _hermite_pack(dtype, entry: str, who: str, pos, vel, mass, rows, vrows, acc, jerk, dt) -> None:
    n = pos.shape[0]
    _chk_n3(dtype, n, ("pos", "vel"), pos, vel); _chk(mass, (n,), "mass", dtype)
    _chk_packed(dtype, rows, vrows, n)
    _chk_together(who, "both acc and jerk, or neither", dtype, n, ("acc", "jerk"), acc, jerk)
    _lib.launch(entry, pos.device, pos.data_ptr(), vel.data_ptr(), _lib.ptr(acc), _lib.ptr(jerk), mass.data_ptr(), n,
                float(dt), rows.data_ptr(), vrows.data_ptr())


def hermite_pack(pos, vel, mass, posm, velp, acc=None, jerk=None, dt: float = 0.0) -> None:
    """posm = {x_p, m}, velp = {v_p, 0} (padded_len(n) rows each): the predicted state after dt from (acc, jerk), or a
    plain pack of (pos, vel) when both are None."""
    _hermite_pack(torch.float32, "nbd_hermite_pack_f32", "hermite_pack", pos, vel, mass, posm, velp, acc, jerk, dt)


def accel_jerk(posm, velp, n: int, softening_sq: float, g_const: float, acc_out=None, jerk_out=None, workspace=None,
               variant: int = 0):
    """(acc, jerk), each (n,3), of all n bodies of posm / velp (as hermite_pack leaves them):
    a_i = G sum_j m_j r_ij s^3, j_i = G sum_j m_j (v_ij s^3 - 3 (r_ij.v_ij) s^5 r_ij), s = (|r_ij|^2 + eps^2)^(-1/2)."""
    _chk_packed(torch.float32, posm, velp, n)
    dev = posm.device
    if acc_out is None:
        acc_out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    if jerk_out is None:
        jerk_out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    _chk_n3(torch.float32, n, ("acc_out", "jerk_out"), acc_out, jerk_out)
    need = _lib.lib().nbd_hermite_workspace_bytes(n)
    if workspace is None or _nbytes(workspace) < need:
        workspace = alloc_bytes(need, dev)
    _lib.launch("nbd_accel_jerk_f32", dev, posm.data_ptr(), velp.data_ptr(), n, float(softening_sq), float(g_const),
                acc_out.data_ptr(), jerk_out.data_ptr(), workspace.data_ptr(), _nbytes(workspace), int(variant))
    return acc_out, jerk_out


def _hermite_step(dtype, entry: str, pos, vel, acc_in, jerk_in, acc_out, jerk_out, mass, dt, softening_sq, g_const,
                  rows, vrows, workspace) -> None:
    """vrows: the packed velocities where the entry takes them as scratch (float64), else None."""
    n = pos.shape[0]
    _chk_n3(dtype, n, ("pos", "vel", "acc_in", "jerk_in", "acc_out", "jerk_out"), pos, vel, acc_in, jerk_in, acc_out,
            jerk_out)
    _chk(mass, (n,), "mass", dtype); _chk_packed(dtype, rows, vrows, n)
    _lib.launch(entry, pos.device, pos.data_ptr(), vel.data_ptr(), acc_in.data_ptr(), jerk_in.data_ptr(),
                acc_out.data_ptr(), jerk_out.data_ptr(), mass.data_ptr(), n, float(dt), float(softening_sq),
                float(g_const), *(t.data_ptr() for t in (rows, vrows) if t is not None), workspace.data_ptr(),
                _nbytes(workspace))


def hermite_step(pos, vel, acc_in, jerk_in, acc_out, jerk_out, mass, dt: float, softening_sq: float, g_const: float,
                 posm, workspace) -> None:
    """One predictor-corrector step (three launches): pos, vel in place; acc_out, jerk_out = a, j at the predicted state
    (may be acc_in, jerk_in); posm = {x1, m}. dt is the Python double: the fp32 step constants are formed from it."""
    _hermite_step(torch.float32, "nbd_hermite_step_f32", pos, vel, acc_in, jerk_in, acc_out, jerk_out, mass, dt,
                  softening_sq, g_const, posm, None, workspace)


# ------------------------------------------------------ range-sharded Hermite step (csrc/direct_hermite_shard.hip)
HERMITE_ROW = 8                 # floats per exchanged row: {x_p, y_p, z_p, m, vx_p, vy_p, vz_p, 0}


def alloc_hermite_rows(n: int, device) -> torch.Tensor:
    """Zeroed (padded_len(n), 8) rows: a rank's send buffer, or the gathered array of all n bodies."""
    return torch.zeros((padded_len(n), HERMITE_ROW), dtype=torch.float32, device=device)


def hermite_shard_plan(n_total: int, lo: int, n_local: int) -> dict:
    return _plan("nbd_hermite_shard_plan", _PLAN4, n_total, lo, n_local)


def hermite_shard_workspace(n_total: int, lo: int, n_local: int, device) -> torch.Tensor:
    return alloc_bytes(_lib.lib().nbd_hermite_shard_workspace_bytes(n_total, lo, n_local), device)


def _chk_rows(t: torch.Tensor, n: int, name: str, dtype=torch.float32, width: int = HERMITE_ROW):
    """An array of `width`-element exchanged rows of `dtype` that holds at least padded_len(n) of them."""
    _chk_min_rows(t, padded_len(n), width, name, dtype)


def _hermite_shard_predict(dtype, entry: str, who: str, pos, vel, mass, send, acc, jerk, dt) -> None:
    n = pos.shape[0]
    _chk_n3(dtype, n, ("pos", "vel"), pos, vel); _chk(mass, (n,), "mass", dtype)
    _chk_rows(send, n, "send", dtype)
    _chk_together(who, "both acc and jerk, or neither", dtype, n, ("acc", "jerk"), acc, jerk)
    _lib.launch(entry, send.device, pos.data_ptr(), vel.data_ptr(), _lib.ptr(acc), _lib.ptr(jerk), mass.data_ptr(), n,
                float(dt), send.data_ptr(), send.shape[0])


def _hermite_shard_force_local(dtype, entry: str, send, n_local, n_total, lo, softening_sq, workspace, *slabs,
                               width: int = HERMITE_ROW) -> None:
    _chk_rows(send, n_local, "send", dtype, width)
    _lib.launch(entry, send.device, send.data_ptr(), n_local, float(softening_sq), workspace.data_ptr(),
                _nbytes(workspace), n_total, lo, *map(int, slabs))


def _hermite_shard_force_remote(dtype, entry: str, who: str, rows_all, n_total, send, n_local, lo, softening_sq, g_const,
                                acc_out, jerk_out, workspace, pos, vel, acc_in, jerk_in, dt, *slabs) -> None:
    _chk_rows(rows_all, n_total, "rows_all", dtype)
    _chk_rows(send, n_local, "send", dtype)
    _chk_n3(dtype, n_local, ("acc_out", "jerk_out"), acc_out, jerk_out)
    _chk_together(who, "pos, vel, acc_in and jerk_in, or none of them", dtype, n_local,
                  ("pos", "vel", "acc_in", "jerk_in"), pos, vel, acc_in, jerk_in)
    _lib.launch(entry, rows_all.device, rows_all.data_ptr(), n_total, send.data_ptr(), n_local, lo, float(softening_sq),
                float(g_const), _lib.ptr(pos), _lib.ptr(vel), _lib.ptr(acc_in), _lib.ptr(jerk_in), acc_out.data_ptr(),
                jerk_out.data_ptr(), float(dt), workspace.data_ptr(), _nbytes(workspace), *map(int, slabs))


def hermite_shard_predict(pos, vel, mass, send, acc=None, jerk=None, dt: float = 0.0) -> None:
    """First launch of the sharded Hermite step: send[:n_local] = {x_p, m, v_p, 0} of the rank's bodies predicted over dt
    from (acc, jerk) -- a plain pack of (pos, vel) when both are None -- and zeros in every row behind n_local."""
    _hermite_shard_predict(torch.float32, "nbd_hermite_shard_predict_f32", "hermite_shard_predict", pos, vel, mass, send,
                           acc, jerk, dt)


def hermite_shard_force_local(send: torch.Tensor, n_local: int, n_total: int, lo: int, softening_sq: float,
                              workspace: torch.Tensor) -> None:
    """Second launch: acceleration + jerk partial sums of the own bodies under the own bodies (reads `send` only, so it
    runs while the all-gather is in flight)."""
    _hermite_shard_force_local(torch.float32, "nbd_hermite_shard_force_local_f32", send, n_local, n_total, lo,
                               softening_sq, workspace)


def hermite_shard_force_remote(rows_all: torch.Tensor, n_total: int, send: torch.Tensor, n_local: int, lo: int,
                               softening_sq: float, g_const: float, acc_out: torch.Tensor, jerk_out: torch.Tensor,
                               workspace: torch.Tensor, pos=None, vel=None, acc_in=None, jerk_in=None,
                               dt: float = 0.0) -> None:
    """Third and fourth launch: every other body of the gathered rows as a source, then a1, j1 = G * sum(slabs) into
    acc_out, jerk_out. With pos, vel, acc_in, jerk_in and dt also the corrector of the own rows (pos, vel in place;
    acc_out may be acc_in and jerk_out jerk_in); with none of them the force on its own."""
    _hermite_shard_force_remote(torch.float32, "nbd_hermite_shard_force_remote_f32", "hermite_shard_force_remote",
                                rows_all, n_total, send, n_local, lo, softening_sq, g_const, acc_out, jerk_out, workspace,
                                pos, vel, acc_in, jerk_in, dt)


# ---------------------------------------------------------- double-precision Hermite (csrc/direct_hermite_f64.hip)
F64 = torch.float64


def alloc_rows_f64(n: int, device) -> torch.Tensor:
    """Zeroed (padded_len(n), 4) float64 rows: posd = {x, y, z, m} or veld = {vx, vy, vz, 0}."""
    return torch.zeros((padded_len(n), 4), dtype=F64, device=device)


def hermite_f64_plan(n: int) -> dict:
    return _plan("nbd_hermite_f64_plan", _PLAN3, int(n))


def hermite_f64_workspace(n: int, device, slabs: int = 0) -> torch.Tensor:
    """The partial sums of every f64 entry at n bodies (or of accel_jerk_f64 with an explicit slab count)."""
    need = _lib.lib().nbd_hermite_f64_workspace_bytes(int(n))
    return alloc_bytes(max(need, int(slabs) * 6 * int(n) * 8), device)


def hermite_f64_pack(pos, vel, mass, posd, veld, acc=None, jerk=None, dt: float = 0.0) -> None:
    """hermite_pack in float64: posd = {x_p, m}, veld = {v_p, 0}, predicted over dt from (acc, jerk) or a plain pack."""
    _hermite_pack(F64, "nbd_hermite_f64_pack", "hermite_f64_pack", pos, vel, mass, posd, veld, acc, jerk, dt)


def accel_jerk_f64(posd, veld, n: int, softening_sq: float, g_const: float, workspace=None, slabs: int = 0):
    """accel_jerk in float64: new (acc, jerk), each (n,3) float64. slabs: 0 = the plan's source split, else that many."""
    _chk_packed(F64, posd, veld, n)
    dev = posd.device
    acc_out = torch.empty((n, 3), dtype=F64, device=dev)
    jerk_out = torch.empty((n, 3), dtype=F64, device=dev)
    if workspace is None:                       # a given workspace is checked by the entry, against what this call uses
        workspace = hermite_f64_workspace(n, dev, slabs)
    _lib.launch("nbd_accel_jerk_f64", dev, posd.data_ptr(), veld.data_ptr(), n, float(softening_sq), float(g_const),
                acc_out.data_ptr(), jerk_out.data_ptr(), workspace.data_ptr(), _nbytes(workspace), int(slabs))
    return acc_out, jerk_out


def hermite_step_f64(pos, vel, acc_in, jerk_in, acc_out, jerk_out, mass, dt: float, softening_sq: float,
                     g_const: float, posd, veld, workspace) -> None:
    """hermite_step in float64 (three launches): pos, vel in place; acc_out, jerk_out may be acc_in, jerk_in;
    posd = {x1, m}; veld is scratch. dt, softening_sq and g_const go in as the Python doubles."""
    _hermite_step(F64, "nbd_hermite_step_f64", pos, vel, acc_in, jerk_in, acc_out, jerk_out, mass, dt, softening_sq,
                  g_const, posd, veld, workspace)


def energy_f64(posd, vel, n: int, softening: float, g_const: float, workspace, out_uk=None):
    """Device double[2] = {U, K} in the reference's convention from a float64 state; asynchronous."""
    out_uk = _energy_out(F64, posd, vel, n, out_uk)
    _lib.launch("nbd_energy_f64", vel.device, posd.data_ptr(), vel.data_ptr(), n, float(softening), float(g_const),
                out_uk.data_ptr(), workspace.data_ptr(), _nbytes(workspace))
    return out_uk


def potential_f64(posd, n: int, softening_sq: float, g_const: float, workspace, out=None) -> torch.Tensor:
    """phi (n,) float64 of the n bodies of posd under each other, pair terms in float64; asynchronous."""
    _chk_packed(F64, posd, None, n)
    if out is None:
        out = torch.empty((n,), dtype=F64, device=posd.device)
    _chk(out, (n,), "phi_out", F64)
    _lib.launch("nbd_potential_f64", posd.device, posd.data_ptr(), n, float(softening_sq), float(g_const),
                out.data_ptr(), workspace.data_ptr(), _nbytes(workspace))
    return out


def invariants_state_f64(pos, vel, mass, phi, out=None) -> torch.Tensor:
    """`invariants` from a float64 state (pos, vel (n,3), mass (n)) and its potentials phi; asynchronous."""
    n = pos.shape[0]
    _chk_n3(F64, n, ("pos", "vel"), pos, vel); _chk(mass, (n,), "mass", F64)
    _chk(phi, (n,), "phi", F64)
    if out is None:
        out = torch.empty(INVARIANT_ROW, dtype=F64, device=vel.device)
    _chk(out, (INVARIANT_ROW,), "out_row", F64)
    _lib.launch("nbd_invariants_state_f64", vel.device, pos.data_ptr(), vel.data_ptr(), mass.data_ptr(), phi.data_ptr(),
                n, out.data_ptr())
    return out


# ---------------------------------------------------------- 6th-order Hermite, float64 (csrc/direct_hermite_f64.hip)
def _chk_accd(accd, n: int):
    """The third packed array {ax, ay, az, 0}: laid out like veld."""
    _chk(accd, (padded_len(n), 4), "accd", F64)


def hermite6_workspace(n: int, device, slabs: int = 0) -> torch.Tensor:
    """The partial sums of the 6th-order entries at n bodies: 9 doubles per body and slab (or of accel_jerk_snap_f64
    with an explicit slab count)."""
    need = _lib.lib().nbd_hermite6_f64_workspace_bytes(int(n))
    return alloc_bytes(max(need, int(slabs) * 9 * int(n) * 8), device)


def hermite6_pack(pos, vel, mass, posd, veld, accd, acc=None, jerk=None, snap=None, crackle=None,
                  dt: float = 0.0) -> None:
    """posd = {x_p, m}, veld = {v_p, 0}, accd = {a_p, 0}, predicted over dt from (acc, jerk, snap, crackle); with jerk,
    snap and crackle all None a plain pack of (pos, vel, acc), and acc None gives zero rows."""
    n = pos.shape[0]
    _chk_n3(F64, n, ("pos", "vel"), pos, vel); _chk(mass, (n,), "mass", F64)
    _chk_packed(F64, posd, veld, n); _chk_accd(accd, n)
    higher = (jerk, snap, crackle)
    if len({t is None for t in higher}) != 1 or (jerk is not None and acc is None):
        raise _lib.NbdError("hermite6_pack: give acc, jerk, snap and crackle, or acc alone, or none of them")
    for t, nm in ((acc, "acc"), (jerk, "jerk"), (snap, "snap"), (crackle, "crackle")):
        if t is not None:
            _chk(t, (n, 3), nm, F64)
    _lib.launch("nbd_hermite6_f64_pack", pos.device, pos.data_ptr(), vel.data_ptr(), _lib.ptr(acc), _lib.ptr(jerk),
                _lib.ptr(snap), _lib.ptr(crackle), mass.data_ptr(), n, float(dt), posd.data_ptr(), veld.data_ptr(),
                accd.data_ptr())


def accel_jerk_snap_f64(posd, veld, accd, n: int, softening_sq: float, g_const: float, workspace=None, slabs: int = 0):
    """New (acc, jerk, snap), each (n,3) float64, of the n bodies of the packed rows; acc and jerk are accel_jerk_f64's
    bits at the same slab count. slabs: 0 = the plan's source split, else that many."""
    _chk_packed(F64, posd, veld, n); _chk_accd(accd, n)
    dev = posd.device
    acc_out, jerk_out, snap_out = (torch.empty((n, 3), dtype=F64, device=dev) for _ in range(3))
    if workspace is None:                       # a given workspace is checked by the entry, against what this call uses
        workspace = hermite6_workspace(n, dev, slabs)
    _lib.launch("nbd_accel_jerk_snap_f64", dev, posd.data_ptr(), veld.data_ptr(), accd.data_ptr(), n,
                float(softening_sq), float(g_const), acc_out.data_ptr(), jerk_out.data_ptr(), snap_out.data_ptr(),
                workspace.data_ptr(), _nbytes(workspace), int(slabs))
    return acc_out, jerk_out, snap_out


def hermite6_step_f64(pos, vel, acc_in, jerk_in, snap_in, crackle_in, acc_out, jerk_out, snap_out, crackle_out, mass,
                      dt: float, softening_sq: float, g_const: float, posd, veld, accd, workspace) -> None:
    """One 6th-order Hermite step (three launches): pos, vel in place; every output may be its input; posd = {x1, m};
    veld and accd are scratch. dt, softening_sq and g_const go in as the Python doubles."""
    n = pos.shape[0]
    state = (pos, vel, acc_in, jerk_in, snap_in, crackle_in, acc_out, jerk_out, snap_out, crackle_out)
    _chk_n3(F64, n, ("pos", "vel", "acc_in", "jerk_in", "snap_in", "crackle_in", "acc_out", "jerk_out", "snap_out",
                     "crackle_out"), *state)
    _chk(mass, (n,), "mass", F64)
    _chk_packed(F64, posd, veld, n); _chk_accd(accd, n)
    _lib.launch("nbd_hermite6_step_f64", pos.device, *(t.data_ptr() for t in state), mass.data_ptr(), n, float(dt),
                float(softening_sq), float(g_const), posd.data_ptr(), veld.data_ptr(), accd.data_ptr(),
                workspace.data_ptr(), _nbytes(workspace))


# ---------------------------------------------------------- double-precision leapfrog (csrc/direct_leapfrog_f64.hip)
def accel_f64_workspace(n: int, device, slabs: int = 0) -> torch.Tensor:
    """The partial sums of accel_f64 at n bodies: 3 doubles per body and slab (slabs: 0 = the plan's)."""
    return alloc_bytes(_lib.lib().nbd_accel_f64_workspace_bytes(int(n), int(slabs)), device)


def accel_f64(posd, n: int, softening_sq: float, g_const: float, workspace=None, slabs: int = 0, out=None):
    """The all-pairs acceleration in float64: new (n,3) float64, the bits of accel_jerk_f64's acceleration at the same
    slab count, from posd alone. slabs: 0 = the plan's source split, else that many."""
    _chk_packed(F64, posd, None, n)
    dev = posd.device
    if out is None:
        out = torch.empty((n, 3), dtype=F64, device=dev)
    _chk(out, (n, 3), "acc_out", F64)
    if workspace is None:                       # a given workspace is checked by the entry, against what this call uses
        workspace = accel_f64_workspace(n, dev, slabs)
    _lib.launch("nbd_accel_f64", dev, posd.data_ptr(), n, float(softening_sq), float(g_const), out.data_ptr(),
                workspace.data_ptr(), _nbytes(workspace), int(slabs))
    return out


def leapfrog_step_f64(pos, vel, acc_in, acc_out, mass, dt_half: float, dt: float, softening_sq: float, g_const: float,
                      posd, workspace) -> None:
    """leapfrog_step in float64 (three launches): pos, vel in place; acc_out may be acc_in; posd = {x1, m}. dt_half, dt,
    softening_sq and g_const go in as the Python doubles."""
    n = pos.shape[0]
    _chk_n3(F64, n, ("pos", "vel", "acc_in", "acc_out"), pos, vel, acc_in, acc_out)
    _chk(mass, (n,), "mass", F64)
    _chk_packed(F64, posd, None, n)
    _lib.launch("nbd_leapfrog_step_f64", pos.device, pos.data_ptr(), vel.data_ptr(), acc_in.data_ptr(),
                acc_out.data_ptr(), mass.data_ptr(), n, float(dt_half), float(dt), float(softening_sq), float(g_const),
                posd.data_ptr(), workspace.data_ptr(), _nbytes(workspace))


def euler_step_f64(pos, vel, acc_out, mass, dt: float, softening_sq: float, g_const: float, posd, workspace) -> None:
    """euler_step in float64 (three launches): acc_out = a(x), v += dt a, x += dt v; posd keeps the positions from before
    the drift."""
    n = pos.shape[0]
    _chk_n3(F64, n, ("pos", "vel", "acc_out"), pos, vel, acc_out)
    _chk(mass, (n,), "mass", F64)
    _chk_packed(F64, posd, None, n)
    _lib.launch("nbd_euler_step_f64", pos.device, pos.data_ptr(), vel.data_ptr(), acc_out.data_ptr(), mass.data_ptr(),
                n, float(dt), float(softening_sq), float(g_const), posd.data_ptr(), workspace.data_ptr(),
                _nbytes(workspace))


# ----------------------- double-precision range-sharded Hermite step (csrc/direct_hermite_shard_f64.hip: the 4th order)
def alloc_hermite_rows_f64(n: int, device) -> torch.Tensor:
    """alloc_hermite_rows in float64: zeroed (padded_len(n), 8) rows of 64 bytes, {x_p, y_p, z_p, m, vx_p, vy_p, vz_p, 0}."""
    return torch.zeros((padded_len(n), HERMITE_ROW), dtype=F64, device=device)


def hermite_shard_f64_plan(n_total: int, lo: int, n_local: int) -> dict:
    return _plan("nbd_hermite_shard_f64_plan", _PLAN4, n_total, lo, n_local)


def hermite_shard_f64_workspace(n_total: int, lo: int, n_local: int, device, slabs_local: int = 0,
                                slabs_remote: int = 0) -> torch.Tensor:
    """The partial sums of a rank's two force launches; slab counts: 0 = the plan's, else that many."""
    return alloc_bytes(_lib.lib().nbd_hermite_shard_f64_workspace_bytes(n_total, lo, n_local, int(slabs_local),
                                                                        int(slabs_remote)), device)


def hermite_shard_predict_f64(pos, vel, mass, send, acc=None, jerk=None, dt: float = 0.0) -> None:
    """hermite_shard_predict in float64: send[:n_local] = {x_p, m, v_p, 0} of the rank's bodies predicted over dt from
    (acc, jerk) -- a plain pack of (pos, vel) when both are None -- and zeros in every row behind n_local."""
    _hermite_shard_predict(F64, "nbd_hermite_shard_predict_f64", "hermite_shard_predict_f64", pos, vel, mass, send, acc,
                           jerk, dt)


def hermite_shard_force_local_f64(send: torch.Tensor, n_local: int, n_total: int, lo: int, softening_sq: float,
                                  workspace: torch.Tensor, slabs: int = 0) -> None:
    """hermite_shard_force_local in float64. slabs: 0 = the plan's split of the own chunks, else that many slabs."""
    _hermite_shard_force_local(F64, "nbd_hermite_shard_force_local_f64", send, n_local, n_total, lo, softening_sq,
                               workspace, slabs)


def hermite_shard_force_remote_f64(rows_all: torch.Tensor, n_total: int, send: torch.Tensor, n_local: int, lo: int,
                                   softening_sq: float, g_const: float, acc_out: torch.Tensor, jerk_out: torch.Tensor,
                                   workspace: torch.Tensor, pos=None, vel=None, acc_in=None, jerk_in=None,
                                   dt: float = 0.0, slabs_local: int = 0, slabs_remote: int = 0) -> None:
    """hermite_shard_force_remote in float64: every other body of the gathered rows as a source, then a1, j1 =
    G * sum(slabs) into acc_out, jerk_out, and with pos, vel, acc_in, jerk_in and dt the corrector of the own rows.
    slabs_local: what the local call was given; slabs_remote: 0 = the plan's split of the remote chunks."""
    _hermite_shard_force_remote(F64, "nbd_hermite_shard_force_remote_f64", "hermite_shard_force_remote_f64", rows_all,
                                n_total, send, n_local, lo, softening_sq, g_const, acc_out, jerk_out, workspace, pos, vel,
                                acc_in, jerk_in, dt, slabs_local, slabs_remote)


# ----------------------- range-sharded 6th-order Hermite step, float64 (csrc/direct_hermite_shard_f64.hip: the 6th order)
HERMITE6_ROW = 12               # doubles per exchanged row: {x_p, y_p, z_p, m, vx_p, vy_p, vz_p, 0, ax_p, ay_p, az_p, 0}


def alloc_hermite6_rows_f64(n: int, device) -> torch.Tensor:
    """Zeroed (padded_len(n), 12) float64 rows of 96 bytes: a rank's send buffer, or the gathered array of all n bodies.
    The force kernels fetch whole 64-row chunks, so both are allocated to the padded length."""
    return torch.zeros((padded_len(n), HERMITE6_ROW), dtype=F64, device=device)


def hermite6_shard_f64_plan(n_total: int, lo: int, n_local: int) -> dict:
    return _plan("nbd_hermite6_shard_f64_plan", _PLAN4, n_total, lo, n_local)


def hermite6_shard_f64_workspace(n_total: int, lo: int, n_local: int, device, slabs_local: int = 0,
                                 slabs_remote: int = 0) -> torch.Tensor:
    """The partial sums of a rank's two force launches, 9 doubles per body and slab; slab counts: 0 = the plan's, else
    that many."""
    return alloc_bytes(_lib.lib().nbd_hermite6_shard_f64_workspace_bytes(n_total, lo, n_local, int(slabs_local),
                                                                         int(slabs_remote)), device)


def hermite6_shard_predict_f64(pos, vel, mass, send, acc=None, jerk=None, snap=None, crackle=None,
                               dt: float = 0.0) -> None:
    """First launch of the sharded 6th-order step: send[:n_local] = {x_p, m, v_p, 0, a_p, 0} of the rank's bodies
    predicted over dt from (acc, jerk, snap, crackle) -- with jerk, snap and crackle all None a plain pack of (pos, vel,
    acc), and acc None gives a zero third quad pair -- and zeros in every row behind n_local."""
    n = pos.shape[0]
    _chk_n3(F64, n, ("pos", "vel"), pos, vel); _chk(mass, (n,), "mass", F64)
    _chk_rows(send, n, "send", F64, HERMITE6_ROW)
    higher = (jerk, snap, crackle)
    if len({t is None for t in higher}) != 1 or (jerk is not None and acc is None):
        raise _lib.NbdError("hermite6_shard_predict_f64: give acc, jerk, snap and crackle, or acc alone, or none of them")
    for t, nm in ((acc, "acc"), (jerk, "jerk"), (snap, "snap"), (crackle, "crackle")):
        if t is not None:
            _chk(t, (n, 3), nm, F64)
    _lib.launch("nbd_hermite6_shard_predict_f64", send.device, pos.data_ptr(), vel.data_ptr(), _lib.ptr(acc),
                _lib.ptr(jerk), _lib.ptr(snap), _lib.ptr(crackle), mass.data_ptr(), n, float(dt), send.data_ptr(),
                send.shape[0])


def hermite6_shard_force_local_f64(send: torch.Tensor, n_local: int, n_total: int, lo: int, softening_sq: float,
                                   workspace: torch.Tensor, slabs: int = 0) -> None:
    """Second launch: acceleration + jerk + snap partial sums of the own bodies under the own bodies (reads `send` only,
    so it runs while the all-gather is in flight). slabs: 0 = the plan's split of the own chunks, else that many slabs."""
    _hermite_shard_force_local(F64, "nbd_hermite6_shard_force_local_f64", send, n_local, n_total, lo, softening_sq,
                               workspace, slabs, width=HERMITE6_ROW)


def hermite6_shard_force_remote_f64(rows_all: torch.Tensor, n_total: int, send: torch.Tensor, n_local: int, lo: int,
                                    softening_sq: float, g_const: float, acc_out: torch.Tensor, jerk_out: torch.Tensor,
                                    snap_out: torch.Tensor, workspace: torch.Tensor, pos=None, vel=None, acc_in=None,
                                    jerk_in=None, snap_in=None, crackle_out=None, dt: float = 0.0, slabs_local: int = 0,
                                    slabs_remote: int = 0) -> None:
    """Third and fourth launch: every other body of the gathered rows as a source, then a1, j1, s1 = G * sum(slabs) into
    acc_out, jerk_out, snap_out. With pos, vel, acc_in, jerk_in, snap_in, crackle_out and dt also the corrector of the own
    rows (pos, vel in place; every output may be its input) and c1 into crackle_out; with none of them the force on its
    own. slabs_local: what the local call was given; slabs_remote: 0 = the plan's split of the remote chunks."""
    _chk_rows(rows_all, n_total, "rows_all", F64, HERMITE6_ROW)
    _chk_rows(send, n_local, "send", F64, HERMITE6_ROW)
    _chk_n3(F64, n_local, ("acc_out", "jerk_out", "snap_out"), acc_out, jerk_out, snap_out)
    _chk_together("hermite6_shard_force_remote_f64", "pos, vel, acc_in, jerk_in, snap_in and crackle_out, or none of them",
                  F64, n_local, ("pos", "vel", "acc_in", "jerk_in", "snap_in", "crackle_out"), pos, vel, acc_in, jerk_in,
                  snap_in, crackle_out)
    _lib.launch("nbd_hermite6_shard_force_remote_f64", rows_all.device, rows_all.data_ptr(), n_total, send.data_ptr(),
                n_local, lo, float(softening_sq), float(g_const), _lib.ptr(pos), _lib.ptr(vel), _lib.ptr(acc_in),
                _lib.ptr(jerk_in), _lib.ptr(snap_in), acc_out.data_ptr(), jerk_out.data_ptr(), snap_out.data_ptr(),
                _lib.ptr(crackle_out), float(dt), workspace.data_ptr(), _nbytes(workspace), int(slabs_local),
                int(slabs_remote))


# ------------------------------------------------ backward of the all-pairs acceleration (csrc/direct_grad.hip)
def accel_vjp_workspace(n: int, device) -> torch.Tensor:
    return alloc_bytes(_lib.lib().nbd_accel_vjp_workspace_bytes(int(n)), device)


def _chk_grads(n: int, dtype, dev, grad_pos, grad_mass, want_pos: bool, want_mass: bool):
    if not (want_pos or want_mass):
        raise _lib.NbdError("accel_vjp: neither gradient is asked for")
    if want_pos and grad_pos is None:
        grad_pos = torch.empty((n, 3), dtype=dtype, device=dev)
    if want_mass and grad_mass is None:
        grad_mass = torch.empty((n,), dtype=dtype, device=dev)
    if want_pos:
        _chk(grad_pos, (n, 3), "grad_pos", dtype)
    if want_mass:
        _chk(grad_mass, (n,), "grad_mass", dtype)
    return (grad_pos if want_pos else None), (grad_mass if want_mass else None)


def _accel_vjp(dtype, entry: str, who: str, rows, cot, n, softening_sq, g_const, grad_pos, grad_mass, workspace,
               want_pos, want_mass, need_entry: str, *slabs):
    """What accel_vjp and accel_vjp_f64 share behind their own checks of the packed rows: the outputs that are asked
    for, the workspace (need_entry(n, *slabs) bytes) and the launch."""
    dev = rows.device
    grad_pos, grad_mass = _chk_grads(n, dtype, dev, grad_pos, grad_mass, want_pos, want_mass)
    need = getattr(_lib.lib(), need_entry)(n, *slabs)
    if workspace is None:
        workspace = alloc_bytes(need, dev)
    if _nbytes(workspace) < need:
        raise _lib.NbdError(f"{who}: workspace of {_nbytes(workspace)} bytes, {need} needed")
    _lib.launch(entry, dev, rows.data_ptr(), cot.data_ptr(), n, float(softening_sq), float(g_const), _lib.ptr(grad_pos),
                _lib.ptr(grad_mass), workspace.data_ptr(), *slabs)
    return grad_pos, grad_mass


def accel_vjp(posm, cot, n: int, softening_sq: float, g_const: float, grad_pos=None, grad_mass=None, workspace=None,
              want_pos: bool = True, want_mass: bool = True):
    """(grad_pos (n,3), grad_mass (n,)) of L with respect to the positions and masses packed in posm, for the cotangent
    dL/da packed in cot = {gx, gy, gz, 0} (hermite_pack with the cotangent as the velocities), a the acceleration of
    `accel`: dL/dx_i = G sum_j [s^3 h - 3 s^5 d (d.h)], h = m_i g_j - m_j g_i; dL/dm_i = -G sum_j s^3 (d.g_j).
    A gradient that is not wanted is None and is not written."""
    _chk(posm, (padded_len(n), 4), "posm"); _chk(cot, (padded_len(n), 4), "cot")
    return _accel_vjp(torch.float32, "nbd_accel_vjp_f32", "accel_vjp", posm, cot, n, softening_sq, g_const, grad_pos,
                      grad_mass, workspace, want_pos, want_mass, "nbd_accel_vjp_workspace_bytes")


def accel_vjp_f64_workspace(n: int, device, slabs: int = 0) -> torch.Tensor:
    return alloc_bytes(_lib.lib().nbd_accel_vjp_f64_workspace_bytes(int(n), int(slabs)), device)


def accel_vjp_f64(posd, cotd, n: int, softening_sq: float, g_const: float, grad_pos=None, grad_mass=None,
                  workspace=None, slabs: int = 0, want_pos: bool = True, want_mass: bool = True):
    """accel_vjp in float64 (posd, cotd as hermite_f64_pack leaves them). slabs: 0 = the plan's source split."""
    _chk_packed(F64, posd, cotd, n)
    if not 0 <= int(slabs) <= 64:
        raise _lib.NbdError(f"accel_vjp_f64: slabs must be in [0, 64], got {slabs}")
    return _accel_vjp(F64, "nbd_accel_vjp_f64", "accel_vjp_f64", posd, cotd, n, softening_sq, g_const, grad_pos,
                      grad_mass, workspace, want_pos, want_mass, "nbd_accel_vjp_f64_workspace_bytes", int(slabs))


# ------------------------------------------------ backward of the Hermite force (csrc/direct_hermite_grad.hip)
def accel_jerk_vjp_workspace(n: int, device) -> torch.Tensor:
    return alloc_bytes(_lib.lib().nbd_accel_jerk_vjp_workspace_bytes(int(n)), device)


def accel_jerk_vjp_f64_workspace(n: int, device, slabs: int = 0) -> torch.Tensor:
    return alloc_bytes(_lib.lib().nbd_accel_jerk_vjp_f64_workspace_bytes(int(n), int(slabs)), device)


def _accel_jerk_vjp(dtype, entry: str, name: str, rows, vrows, cota, cotj, n, softening_sq, g_const, grads, wants,
                    workspace, need, *slabs):
    """What accel_jerk_vjp and accel_jerk_vjp_f64 share: the checks, the outputs that are asked for, the workspace of
    `need` bytes and the launch."""
    _chk_packed(dtype, rows, vrows, n)
    if cota is None and cotj is None:
        raise _lib.NbdError(f"{name}: neither cotangent is given")
    for t, nm in ((cota, "cota"), (cotj, "cotj")):
        if t is not None:
            _chk(t, (padded_len(n), 4), nm, dtype)
    if not any(wants):
        raise _lib.NbdError(f"{name}: no gradient is asked for")
    dev = rows.device
    out = []
    for g, want, nm, shape in zip(grads, wants, ("grad_pos", "grad_vel", "grad_mass"), ((n, 3), (n, 3), (n,))):
        if want and g is None:
            g = torch.empty(shape, dtype=dtype, device=dev)
        if want:
            _chk(g, shape, nm, dtype)
        out.append(g if want else None)
    if workspace is None:
        workspace = alloc_bytes(need, dev)
    if _nbytes(workspace) < need:
        raise _lib.NbdError(f"{name}: workspace of {_nbytes(workspace)} bytes, {need} needed")
    if n:
        _lib.launch(entry, dev, rows.data_ptr(), vrows.data_ptr(), _lib.ptr(cota), _lib.ptr(cotj), n,
                    float(softening_sq), float(g_const), *map(_lib.ptr, out), workspace.data_ptr(), _nbytes(workspace),
                    *slabs)
    return tuple(out)


def accel_jerk_vjp(posm, velp, cota, cotj, n: int, softening_sq: float, g_const: float, grad_pos=None, grad_vel=None,
                   grad_mass=None, workspace=None, want_pos: bool = True, want_vel: bool = True, want_mass: bool = True):
    """(grad_pos (n,3), grad_vel (n,3), grad_mass (n,)) of L with respect to the positions, velocities and masses packed in
    posm / velp (as hermite_pack leaves them), for the cotangents dL/da and dL/dj of `accel_jerk`, packed in cota and
    cotj = {gx, gy, gz, 0} (hermite_pack with a cotangent as the velocities). Either cotangent may be None: with cotj None
    the results are accel_vjp's bits and grad_vel is zeros. A gradient that is not wanted is None and is not written.
    The formulas: csrc/direct_hermite_grad.hip."""
    return _accel_jerk_vjp(torch.float32, "nbd_accel_jerk_vjp_f32", "accel_jerk_vjp", posm, velp, cota, cotj, n,
                           softening_sq, g_const, (grad_pos, grad_vel, grad_mass), (want_pos, want_vel, want_mass),
                           workspace, _lib.lib().nbd_accel_jerk_vjp_workspace_bytes(int(n)))


def accel_jerk_vjp_f64(posd, veld, cota, cotj, n: int, softening_sq: float, g_const: float, grad_pos=None,
                       grad_vel=None, grad_mass=None, workspace=None, slabs: int = 0, want_pos: bool = True,
                       want_vel: bool = True, want_mass: bool = True):
    """accel_jerk_vjp in float64 (rows as hermite_f64_pack leaves them). slabs: 0 = the plan's source split."""
    if not 0 <= int(slabs) <= 64:
        raise _lib.NbdError(f"accel_jerk_vjp_f64: slabs must be in [0, 64], got {slabs}")
    return _accel_jerk_vjp(F64, "nbd_accel_jerk_vjp_f64", "accel_jerk_vjp_f64", posd, veld, cota, cotj, n, softening_sq,
                           g_const, (grad_pos, grad_vel, grad_mass), (want_pos, want_vel, want_mass), workspace,
                           _lib.lib().nbd_accel_jerk_vjp_f64_workspace_bytes(int(n), int(slabs)), int(slabs))


# ---------------------------------------------------- block-timestep Hermite integrator (csrc/direct_hermite_block.hip)
HBLOCK_SCHED_INTS = 32          # NBD_HBLOCK_SCHED_INTS: {t_next, n_act, clamped, ...} of the block schedule


def _chk_sched(n: int, ticks, levels, sched):
    """The int32 schedule arrays of a block step; ticks None where the entry takes none."""
    if ticks is not None:
        _chk(ticks, (n,), "ticks", torch.int32)
    _chk(levels, (n,), "levels", torch.int32)
    _chk(sched, (HBLOCK_SCHED_INTS,), "sched", torch.int32)


_HBLOCK_STATE = ("pos", "vel", "acc", "jerk", "snap", "crackle")      # the 4th order carries the first four


def _chk_block_rows(dtype, n: int, rows):
    """The packed source arrays a block entry takes, (pos_rows[, vel_rows[, accd]]), as _chk_packed and _chk_accd check
    them."""
    shape = (padded_len(n), 4)
    for t, name in zip(rows, ("posm", "velp") if dtype == torch.float32 else ("posd", "veld", "accd")):
        _chk(t, shape, name, dtype)


def _ptrs(tensors):
    """The device pointers of a state or row tuple, for a launch's argument list. (A map, not a generator expression: this
    runs in every eager block step, and the generator's frames cost a measurable part of one.)"""
    return map(torch.Tensor.data_ptr, tensors)


def _chk_hblock(dtype, state, mass, ticks, levels, sched, rows) -> int:
    """The arguments of a block step in `dtype`: state = the (n,3) arrays (pos, vel, acc, jerk[, snap, crackle]), rows =
    the packed rows the entry takes (pos_rows[, vel_rows[, accd]]), the int32 schedule arrays; returns n."""
    n = state[0].shape[0]
    _chk_n3(dtype, n, _HBLOCK_STATE, *state)
    _chk(mass, (n,), "mass", dtype)
    _chk_block_rows(dtype, n, rows)
    _chk_sched(n, ticks, levels, sched)
    return n


def hblock_workspace(n: int, device) -> torch.Tensor:
    """Active list + partial sums of one block step (nbd_hblock_workspace_bytes)."""
    return alloc_bytes(_lib.lib().nbd_hblock_workspace_bytes(int(n)), device)


def _hblock_init_levels(dtype, entry: str, acc, jerk, dt, eta, max_level, ticks, levels, sched) -> None:
    n = acc.shape[0]
    _chk_n3(dtype, n, ("acc", "jerk"), acc, jerk)
    _chk_sched(n, ticks, levels, sched)
    _lib.launch(entry, acc.device, acc.data_ptr(), jerk.data_ptr(), n, float(dt), float(eta), int(max_level),
                ticks.data_ptr(), levels.data_ptr(), sched.data_ptr())


def hblock_init_levels(acc, jerk, dt: float, eta: float, max_level: int, ticks, levels, sched) -> None:
    """ticks = 0, levels from dt_i = (eta / 2) |a| / |j| quantised to dt 2^-k (k in [0, max_level]; deeper ones are
    clamped and counted in sched[2]); starts a new interval."""
    _hblock_init_levels(torch.float32, "nbd_hblock_init_levels", acc, jerk, dt, eta, max_level, ticks, levels, sched)


def hblock_schedule(levels, max_level: int, sched, workspace, host_sched=None) -> None:
    """t_next and the active list of the next block step (sched[0], sched[1]; the list into the workspace). host_sched: an
    int32 CPU tensor of at least 4 elements (pinned is fastest) that receives sched[0..4) after a stream sync."""
    n = levels.shape[0]
    _chk_sched(n, None, levels, sched)
    if host_sched is not None and (host_sched.is_cuda or host_sched.dtype != torch.int32 or host_sched.numel() < 4):
        raise _lib.NbdError("hblock_schedule: host_sched must be an int32 CPU tensor of 4 elements")
    _lib.launch("nbd_hblock_schedule", levels.device, levels.data_ptr(), n, int(max_level), sched.data_ptr(),
                workspace.data_ptr(), _nbytes(workspace), _lib.ptr(host_sched))


def _hblock_step(dtype, entry: str, state, mass, ticks, levels, n_act, max_level, dt, eta, softening_sq, g_const, sched,
                 rows, workspace) -> None:
    """A whole block step of either order and format: the state tuple gives the leading pointers, the row tuple the
    trailing ones."""
    n = _chk_hblock(dtype, state, mass, ticks, levels, sched, rows)
    _lib.launch(entry, state[0].device, *_ptrs(state), mass.data_ptr(), ticks.data_ptr(), levels.data_ptr(), n, int(n_act),
                int(max_level), float(dt), float(eta), float(softening_sq), float(g_const), sched.data_ptr(),
                *_ptrs(rows), workspace.data_ptr(), _nbytes(workspace))


def hblock_step(pos, vel, acc, jerk, mass, ticks, levels, n_act: int, max_level: int, dt: float, eta: float,
                softening_sq: float, g_const: float, sched, posm, velp, workspace) -> None:
    """Predict all bodies to t_next, evaluate the n_act listed ones, correct and re-level them (three launches). pos, vel,
    acc, jerk, ticks, levels in place for the active bodies; posm = {x1, m} for them, predicted rows for the rest."""
    _hblock_step(torch.float32, "nbd_hblock_step_f32", (pos, vel, acc, jerk), mass, ticks, levels, n_act, max_level, dt,
                 eta, softening_sq, g_const, sched, (posm, velp), workspace)


def _accel_jerk_active(dtype, entry: str, rows, n, act, softening_sq, g_const, workspace, new_workspace, *slabs):
    """The force of a list on its own: one (len(act), 3) output per packed source array of `rows` (acc, jerk[, snap]).
    new_workspace(device, n_act): the workspace where none is given."""
    _chk_block_rows(dtype, n, rows)
    _chk(act, None, "act", torch.int32)
    n_act = act.numel()
    dev = rows[0].device
    outs = tuple(torch.empty((n_act, 3), dtype=dtype, device=dev) for _ in rows)
    if workspace is None:                       # a given workspace is checked by the entry, against what this call uses
        workspace = new_workspace(dev, n_act)
    _lib.launch(entry, dev, *_ptrs(rows), n, act.data_ptr(), n_act, float(softening_sq), float(g_const), *_ptrs(outs),
                workspace.data_ptr(), _nbytes(workspace), *map(int, slabs))
    return outs


def accel_jerk_active(posm, velp, n: int, act, softening_sq: float, g_const: float, workspace=None):
    """(acc, jerk), each (len(act), 3), of the bodies act (a device int32 list, any order) under all n bodies of posm /
    velp, in list order. The all-bodies list gives accel_jerk's bits."""
    return _accel_jerk_active(torch.float32, "nbd_accel_jerk_active_f32", (posm, velp), n, act, softening_sq, g_const,
                              workspace, lambda dev, n_act: hblock_workspace(n, dev))


# ---------------- double-precision block-timestep Hermite, 4th and 6th order (csrc/direct_hermite_block_f64.hip)
def _hblock_f64_workspace(entry: str, sums: int, n, device, slabs, n_act) -> torch.Tensor:
    """`entry`(n) bytes, or the list and `sums` doubles per slab and target of an explicit slab count on n_act targets."""
    need = getattr(_lib.lib(), entry)(int(n))
    return alloc_bytes(max(need, (int(n) + 7) // 8 * 32 + int(slabs) * sums * int(n_act) * 8), device)


def _hblock_predict(entry: str, state, mass, ticks, levels, max_level, dt, sched, rows) -> None:
    n = _chk_hblock(F64, state, mass, ticks, levels, sched, rows)
    _lib.launch(entry, state[0].device, *_ptrs(state), mass.data_ptr(), ticks.data_ptr(), n, int(max_level), float(dt),
                sched.data_ptr(), *_ptrs(rows))


def _hblock_force(entry: str, rows, n, n_act, softening_sq, workspace) -> None:
    _chk_block_rows(F64, n, rows)
    _lib.launch(entry, rows[0].device, *_ptrs(rows), n, int(n_act), float(softening_sq), workspace.data_ptr(),
                _nbytes(workspace))


def _hblock_correct(entry: str, state, mass, ticks, levels, n_act, max_level, dt, eta, g_const, sched, posd,
                    workspace) -> None:
    n = _chk_hblock(F64, state, mass, ticks, levels, sched, (posd,))
    _lib.launch(entry, state[0].device, *_ptrs(state), mass.data_ptr(), ticks.data_ptr(), levels.data_ptr(), n, int(n_act),
                int(max_level), float(dt), float(eta), float(g_const), sched.data_ptr(), posd.data_ptr(),
                workspace.data_ptr(), _nbytes(workspace))


def hblock_f64_workspace(n: int, device, slabs: int = 0, n_act: int = 0) -> torch.Tensor:
    """Active list + float64 partial sums of one block step (nbd_hblock_f64_workspace_bytes), or of accel_jerk_active_f64
    with an explicit slab count on n_act targets."""
    return _hblock_f64_workspace("nbd_hblock_f64_workspace_bytes", 6, n, device, slabs, n_act)


def hblock_init_levels_f64(acc, jerk, dt: float, eta: float, max_level: int, ticks, levels, sched) -> None:
    """hblock_init_levels from float64 acc, jerk."""
    _hblock_init_levels(F64, "nbd_hblock_init_levels_f64", acc, jerk, dt, eta, max_level, ticks, levels, sched)


def hblock_predict_f64(pos, vel, acc, jerk, mass, ticks, levels, max_level: int, dt: float, sched, posd, veld) -> None:
    """First launch of a float64 block step: every body predicted to t_next = sched[0] into posd / veld."""
    _hblock_predict("nbd_hblock_predict_f64", (pos, vel, acc, jerk), mass, ticks, levels, max_level, dt, sched,
                    (posd, veld))


def hblock_force_f64(posd, veld, n: int, n_act: int, softening_sq: float, workspace) -> None:
    """Second launch: the partial sums of the n_act bodies the schedule listed in the workspace."""
    _hblock_force("nbd_hblock_force_f64", (posd, veld), n, n_act, softening_sq, workspace)


def hblock_correct_f64(pos, vel, acc, jerk, mass, ticks, levels, n_act: int, max_level: int, dt: float, eta: float,
                       g_const: float, sched, posd, workspace) -> None:
    """Third launch: slab sum, corrector and new level of the listed bodies; posd = {x1, m} for them."""
    _hblock_correct("nbd_hblock_correct_f64", (pos, vel, acc, jerk), mass, ticks, levels, n_act, max_level, dt, eta,
                    g_const, sched, posd, workspace)


def hblock_step_f64(pos, vel, acc, jerk, mass, ticks, levels, n_act: int, max_level: int, dt: float, eta: float,
                    softening_sq: float, g_const: float, sched, posd, veld, workspace) -> None:
    """hblock_step in float64 (three launches): dt, eta, softening_sq and g_const go in as the Python doubles."""
    _hblock_step(F64, "nbd_hblock_step_f64", (pos, vel, acc, jerk), mass, ticks, levels, n_act, max_level, dt, eta,
                 softening_sq, g_const, sched, (posd, veld), workspace)


def accel_jerk_active_f64(posd, veld, n: int, act, softening_sq: float, g_const: float, workspace=None, slabs: int = 0):
    """accel_jerk_active in float64: (acc, jerk), each (len(act), 3) float64, in list order. slabs: 0 = the plan's source
    split, else that many. The all-bodies list gives accel_jerk_f64's bits at the same slab count."""
    return _accel_jerk_active(F64, "nbd_accel_jerk_active_f64", (posd, veld), n, act, softening_sq, g_const, workspace,
                              lambda dev, n_act: hblock_f64_workspace(n, dev, slabs, n_act), slabs)


def hblock6_workspace(n: int, device, slabs: int = 0, n_act: int = 0) -> torch.Tensor:
    """Active list + float64 partial sums of one 6th-order block step (nbd_hblock6_f64_workspace_bytes), or of
    accel_jerk_snap_active_f64 with an explicit slab count on n_act targets."""
    return _hblock_f64_workspace("nbd_hblock6_f64_workspace_bytes", 9, n, device, slabs, n_act)


def hblock6_predict_f64(pos, vel, acc, jerk, snap, crackle, mass, ticks, levels, max_level: int, dt: float, sched, posd,
                        veld, accd) -> None:
    """First launch of a 6th-order block step: every body predicted to t_next = sched[0] into posd / veld / accd."""
    _hblock_predict("nbd_hblock6_predict_f64", (pos, vel, acc, jerk, snap, crackle), mass, ticks, levels, max_level, dt,
                    sched, (posd, veld, accd))


def hblock6_force_f64(posd, veld, accd, n: int, n_act: int, softening_sq: float, workspace) -> None:
    """Second launch: the partial sums of the n_act bodies the schedule listed in the workspace."""
    _hblock_force("nbd_hblock6_force_f64", (posd, veld, accd), n, n_act, softening_sq, workspace)


def hblock6_correct_f64(pos, vel, acc, jerk, snap, crackle, mass, ticks, levels, n_act: int, max_level: int, dt: float,
                        eta: float, g_const: float, sched, posd, workspace) -> None:
    """Third launch: slab sum, corrector, crackle and new level of the listed bodies; posd = {x1, m} for them."""
    _hblock_correct("nbd_hblock6_correct_f64", (pos, vel, acc, jerk, snap, crackle), mass, ticks, levels, n_act,
                    max_level, dt, eta, g_const, sched, posd, workspace)


def hblock6_step_f64(pos, vel, acc, jerk, snap, crackle, mass, ticks, levels, n_act: int, max_level: int, dt: float,
                     eta: float, softening_sq: float, g_const: float, sched, posd, veld, accd, workspace) -> None:
    """Predict all bodies to t_next, evaluate the n_act listed ones, correct and re-level them (three launches). pos, vel,
    acc, jerk, snap, crackle, ticks, levels in place for the active bodies; posd = {x1, m} for them, predicted rows for
    the rest. dt, eta, softening_sq and g_const go in as the Python doubles."""
    _hblock_step(F64, "nbd_hblock6_step_f64", (pos, vel, acc, jerk, snap, crackle), mass, ticks, levels, n_act,
                 max_level, dt, eta, softening_sq, g_const, sched, (posd, veld, accd), workspace)


def accel_jerk_snap_active_f64(posd, veld, accd, n: int, act, softening_sq: float, g_const: float, workspace=None,
                               slabs: int = 0):
    """(acc, jerk, snap), each (len(act), 3) float64, of the bodies act (a device int32 list, any order) under all n
    bodies of posd / veld / accd, in list order. slabs: 0 = the plan's source split, else that many. The all-bodies list
    gives accel_jerk_snap_f64's bits at the same slab count."""
    return _accel_jerk_active(F64, "nbd_accel_jerk_snap_active_f64", (posd, veld, accd), n, act, softening_sq, g_const,
                              workspace, lambda dev, n_act: hblock6_workspace(n, dev, slabs, n_act), slabs)


# ---------------- a block step divided over the ranks of a process group (csrc/direct_hermite_block_split_f64.hip)
HBLOCK_SPLIT_ROW = 16           # NBD_HBLOCK_SPLIT_ROW: x1 v1 a1 j1, three spare doubles, {new level, clamped}
HBLOCK6_SPLIT_ROW = 20          # NBD_HBLOCK6_SPLIT_ROW: x1 v1 a1 j1 s1 c1, one spare double, {new level, clamped}
HBLOCK_SCHED_DIVERGED = 6       # the int of the schedule record a split apply raises when the pieces' headers disagree


def hblock_split_slices(n_act: int, world: int) -> list:
    """[(first, count)] * world: the slices of an ordered active list of n_act entries the ranks of a group evaluate.
    Rank r takes [r q, min((r + 1) q, n_act)) with q = 64 ceil(ceil(n_act / world) / 64), so that no group of 64 targets
    is cut; slices behind the list are (n_act, 0). q is formed here and nowhere else: hblock_split_q reads it off the
    first slice."""
    n_act, world = int(n_act), int(world)
    if n_act < 1 or world < 1:
        raise ValueError(f"hblock_split_slices: n_act={n_act} and world={world} must be at least 1")
    q = 64 * -(-(-(-n_act // world)) // 64)
    firsts = [min(r * q, n_act) for r in range(world + 1)]
    return [(firsts[r], firsts[r + 1] - firsts[r]) for r in range(world)]


def hblock_split_q(slices) -> int:
    """The piece length q of hblock_split_slices(n_act, world): the first slice's count rounded up to a group of 64 (the
    first slice is [0, min(q, n_act)))."""
    return -(-slices[0][1] // 64) * 64


def hblock_split_workspace(n: int, device, order: int = 4) -> torch.Tensor:
    """The ordered list, the ordering's scratch and a slice's block workspace (nbd_hblock_split_f64_workspace_bytes, or
    the hblock6 twin for order 6). Its head is a block workspace's: hblock_schedule and hblock*_step_f64 run on it too."""
    entry = "nbd_hblock_split_f64_workspace_bytes" if order == 4 else "nbd_hblock6_split_f64_workspace_bytes"
    return alloc_bytes(getattr(_lib.lib(), entry)(int(n)), device)


def hblock_order_list(levels, max_level: int, sched, workspace) -> None:
    """The list hblock_schedule has just written, in ascending body index (two launches, no readback)."""
    n = levels.shape[0]
    _chk_sched(n, None, levels, sched)
    _lib.launch("nbd_hblock_order_list", levels.device, levels.data_ptr(), n, int(max_level), sched.data_ptr(),
                workspace.data_ptr(), _nbytes(workspace))


def hblock_split_rows(state, levels, n_act: int, first: int, count: int, max_level: int, dt: float, eta: float,
                      softening_sq: float, g_const: float, sched, rows, rows_out, workspace) -> None:
    """The header and the result rows of entries [first, first + count) of the ordered list into rows_out ((>= 1 + count,
    row) float64), nothing of the state written. state = (pos, vel, acc, jerk) with rows = (posd, veld) for the 4th order,
    (pos, vel, acc, jerk, snap) with (posd, veld, accd) for the 6th."""
    n = state[0].shape[0]
    six = len(rows) == 3
    _chk_n3(F64, n, _HBLOCK_STATE, *state)
    _chk_block_rows(F64, n, rows)
    _chk_sched(n, None, levels, sched)
    if len(state) != (5 if six else 4):
        raise _lib.NbdError("hblock_split_rows: state is (pos, vel, acc, jerk) with two row arrays, or those and snap "
                            "with three")
    width = HBLOCK6_SPLIT_ROW if six else HBLOCK_SPLIT_ROW
    if (rows_out.dtype != F64 or rows_out.dim() != 2 or rows_out.shape[1] != width or not rows_out.is_contiguous()
            or rows_out.shape[0] < 1 + int(count) or rows_out.device != state[0].device):
        raise _lib.NbdError(f"hblock_split_rows: rows_out must be a contiguous float64 (>= {1 + int(count)}, {width}) "
                            "tensor on the state's device")
    _lib.launch("nbd_hblock6_split_rows_f64" if six else "nbd_hblock_split_rows_f64", state[0].device, *_ptrs(state),
                levels.data_ptr(), n, int(n_act), int(first), int(count), int(max_level), float(dt), float(eta),
                float(softening_sq), float(g_const), sched.data_ptr(), *_ptrs(rows), rows_out.data_ptr(),
                workspace.data_ptr(), _nbytes(workspace))


def hblock_split_apply(rows_all, world: int, q: int, n_act: int, state, mass, ticks, levels, max_level: int, sched, posd,
                       workspace) -> None:
    """All n_act rows of rows_all (world pieces of 1 + q rows, contiguous) into state = (pos, vel, acc, jerk[, snap,
    crackle]) with the block step's bookkeeping; posd = {x1, m} for them. A piece whose header disagrees with this
    rank's record raises sched[HBLOCK_SCHED_DIVERGED]."""
    n = _chk_hblock(F64, state, mass, ticks, levels, sched, (posd,))
    six = len(state) == 6
    width = HBLOCK6_SPLIT_ROW if six else HBLOCK_SPLIT_ROW
    if len(state) not in (4, 6):
        raise _lib.NbdError("hblock_split_apply: state is (pos, vel, acc, jerk) or those with snap and crackle")
    if (rows_all.dtype != F64 or rows_all.dim() != 2 or rows_all.shape[1] != width or not rows_all.is_contiguous()
            or rows_all.shape[0] < int(world) * (1 + int(q)) or rows_all.device != state[0].device):
        raise _lib.NbdError(f"hblock_split_apply: rows_all must be a contiguous float64 (>= world (1 + q), {width}) "
                            "tensor on the state's device")
    _lib.launch("nbd_hblock6_split_apply_f64" if six else "nbd_hblock_split_apply_f64", state[0].device,
                rows_all.data_ptr(), int(world), int(q), int(n_act), *_ptrs(state), mass.data_ptr(), ticks.data_ptr(),
                levels.data_ptr(), n, int(max_level), sched.data_ptr(), posd.data_ptr(), workspace.data_ptr(),
                _nbytes(workspace))


# ---------------------------------------------------------------- batched direct integrator (csrc/direct_batch.hip)
class BatchPlan:
    """The host offsets of an ensemble of scenes and the device work list built from them (nbd_batch_plan /
    nbd_batch_plan_fill): built once per set of scene sizes, passed to every batch_* call. dtype=torch.float64: the work
    list of the batch_*_f64 calls instead (nbd_batch_f64_plan / nbd_batch_f64_plan_fill: groups of 64 targets, the
    float64 step's slabs); `posm_rows` then counts the rows of posd / veld and `workspace_bytes` is the one workspace of
    every float64 call. A plan serves the calls of its own dtype only. order=6 (float64 only): the same work list with
    room for the 6th-order step's partial sums (nbd_batch_hermite6_f64_plan_fill: 9 doubles per body and slab where the
    4th-order step has 6) for the batch_hermite6_* calls; the float64 diagnostics, batch_pack_f64 and batch_accel_jerk_f64
    run on it too, with its workspace and a BATCH_H6_PARAM_ROWS table."""

    def __init__(self, sizes, device, dtype=torch.float32, order: int = 4):
        sizes = [int(n) for n in sizes]
        if not sizes or min(sizes) < 0:
            raise _lib.NbdError("batch: need at least one scene and no negative size")
        if dtype not in (torch.float32, F64):
            raise _lib.NbdError(f"batch: dtype must be torch.float32 or torch.float64, got {dtype!r}")
        if order not in (4, 6) or (order == 6 and dtype != F64):
            raise _lib.NbdError(f"batch: order must be 4, or 6 with dtype=torch.float64, got order={order!r}")
        self.dtype, self.order = dtype, order
        self.param_rows = None if dtype == torch.float32 else (BATCH_F64_PARAM_ROWS, BATCH_H6_PARAM_ROWS)[order == 6]
        self.offsets = np.zeros(len(sizes) + 1, dtype=np.int32)
        np.cumsum(sizes, out=self.offsets[1:])
        self.n_scenes, self.n_total = len(sizes), int(self.offsets[-1])
        items, rows = ctypes.c_int(), ctypes.c_int()
        pb, wb = ctypes.c_size_t(), ctypes.c_size_t()
        scenes = (self._off(), self.n_scenes)
        if dtype == torch.float32:
            _lib.call("nbd_batch_plan", *scenes, items, rows, pb, wb)
            fill = "nbd_batch_plan_fill"
        else:
            _lib.call("nbd_batch_f64_plan", *scenes, items, rows, pb)
            _lib.call("nbd_batch_f64_workspace_bytes", *scenes, wb)
            fill = "nbd_batch_f64_plan_fill"
            if order == 6:                    # items, rows and bytes are the float64 plan's
                _lib.call("nbd_batch_hermite6_f64_workspace_bytes", *scenes, wb)
                fill = "nbd_batch_hermite6_f64_plan_fill"
        self.n_items, self.posm_rows, self.plan_bytes, self.workspace_bytes = items.value, rows.value, pb.value, wb.value
        host = np.zeros((self.plan_bytes + 15) // 16 * 4, dtype=np.int32)
        _lib.call(fill, *scenes, host.ctypes.data, self.plan_bytes)
        self.plan = torch.from_numpy(host).to(device)
        self.device = self.plan.device

    def _off(self) -> int:
        return self.offsets.ctypes.data

    def head(self):
        """The leading arguments of every batch entry point."""
        return (self._off(), self.n_scenes, self.plan.data_ptr(), self.plan_bytes)

    def workspace(self) -> torch.Tensor:
        return alloc_bytes(self.workspace_bytes, self.device)

    def alloc_posm(self) -> torch.Tensor:
        return torch.zeros((max(self.posm_rows, 1), 4), dtype=torch.float32, device=self.device)

    def hermite_workspace_bytes(self) -> int:
        if getattr(self, "_hws_bytes", None) is None:          # asked on every step: one host query per plan
            nb = ctypes.c_size_t()
            _lib.call("nbd_batch_hermite_workspace_bytes", self._off(), self.n_scenes, nb)
            self._hws_bytes = nb.value
        return self._hws_bytes

    def hermite_workspace(self) -> torch.Tensor:
        """Packed velocities + acceleration-and-jerk partial sums of the batch_hermite_* calls (the energies keep using
        workspace())."""
        return alloc_bytes(self.hermite_workspace_bytes(), self.device)

    def check_state(self, posm, ws, *arrays):
        if self.dtype != torch.float32:
            raise _lib.NbdError("batch float32 call: the plan was built for float64")
        n = self.n_total
        for t, nm in arrays:
            _chk(t, (n, 3) if nm != "mass" else (n,), nm)
        _chk_min_rows(posm, self.posm_rows, 4, "posm")
        if ws is not None and _nbytes(ws) < self.workspace_bytes:
            raise _lib.NbdError("batch workspace too small")


def _param(p: torch.Tensor, plan: BatchPlan, name: str) -> int:
    _chk(p, (plan.n_scenes,), name)
    return p.data_ptr()


def batch_pack_posm(plan: BatchPlan, pos, mass, posm) -> None:
    plan.check_state(posm, None, (pos, "pos"), (mass, "mass"))
    _lib.launch("nbd_batch_pack_posm_f32", pos.device, *plan.head(), pos.data_ptr(), mass.data_ptr(), posm.data_ptr())


def batch_accel(plan: BatchPlan, pos, mass, eps2, g, acc_out, posm, ws) -> None:
    """acc_out = the force of every scene on its own bodies (packs posm first). eps2, g: device fp32 (S,)."""
    plan.check_state(posm, ws, (pos, "pos"), (mass, "mass"), (acc_out, "acc_out"))
    _lib.launch("nbd_batch_accel_f32", pos.device, *plan.head(), pos.data_ptr(), mass.data_ptr(),
                _param(eps2, plan, "softening_sq"), _param(g, plan, "g_const"), acc_out.data_ptr(), posm.data_ptr(),
                ws.data_ptr(), _nbytes(ws))


def batch_leapfrog_step(plan: BatchPlan, pos, vel, acc_in, acc_out, mass, dt_half, dt, eps2, g, posm, ws) -> None:
    plan.check_state(posm, ws, (pos, "pos"), (vel, "vel"), (acc_in, "acc_in"), (acc_out, "acc_out"), (mass, "mass"))
    _lib.launch("nbd_batch_leapfrog_step_f32", pos.device, *plan.head(), pos.data_ptr(), vel.data_ptr(),
                acc_in.data_ptr(), acc_out.data_ptr(), mass.data_ptr(), _param(dt_half, plan, "dt_half"),
                _param(dt, plan, "dt"), _param(eps2, plan, "softening_sq"), _param(g, plan, "g_const"), posm.data_ptr(),
                ws.data_ptr(), _nbytes(ws))


def batch_euler_step(plan: BatchPlan, pos, vel, acc_out, mass, dt, eps2, g, posm, ws) -> None:
    plan.check_state(posm, ws, (pos, "pos"), (vel, "vel"), (acc_out, "acc_out"), (mass, "mass"))
    _lib.launch("nbd_batch_euler_step_f32", pos.device, *plan.head(), pos.data_ptr(), vel.data_ptr(),
                acc_out.data_ptr(), mass.data_ptr(), _param(dt, plan, "dt"), _param(eps2, plan, "softening_sq"),
                _param(g, plan, "g_const"), posm.data_ptr(), ws.data_ptr(), _nbytes(ws))


def batch_energies(plan: BatchPlan, posm, vel, soft, g, out_uk, ws) -> torch.Tensor:
    """out_uk (S, 2) float64 = {U_s, K_s} from posm (as the batch entries leave it) and vel; asynchronous."""
    plan.check_state(posm, ws, (vel, "vel"))
    _chk(out_uk, (plan.n_scenes, 2), "out_uk", torch.float64)
    _lib.launch("nbd_batch_energies", vel.device, *plan.head(), posm.data_ptr(), vel.data_ptr(),
                _param(soft, plan, "softening"), _param(g, plan, "g_const"), out_uk.data_ptr(), ws.data_ptr(),
                _nbytes(ws))
    return out_uk


def batch_potential(plan: BatchPlan, posm, eps2, g, phi_out, ws) -> torch.Tensor:
    """phi_out (N_total,) float64 = every body's potential under the bodies of its own scene (`potential` per scene, bit
    for bit) from posm as the batch entries leave it. eps2, g: device fp32 (S,); ws: plan.workspace(). Asynchronous."""
    plan.check_state(posm, ws)
    _chk(phi_out, (plan.n_total,), "phi_out", torch.float64)
    _lib.launch("nbd_batch_potential_f32", posm.device, *plan.head(), posm.data_ptr(),
                _param(eps2, plan, "softening_sq"), _param(g, plan, "g_const"), phi_out.data_ptr(), ws.data_ptr(),
                _nbytes(ws))
    return phi_out


def batch_invariants(plan: BatchPlan, posm, vel, phi, out_rows) -> torch.Tensor:
    """out_rows (S, 16) float64 = `invariants` of every scene (bit for bit) from posm, vel and phi (batch_potential)."""
    plan.check_state(posm, None, (vel, "vel"))
    _chk(phi, (plan.n_total,), "phi", torch.float64)
    _chk(out_rows, (plan.n_scenes, INVARIANT_ROW), "out_rows", torch.float64)
    _lib.launch("nbd_batch_invariants_f64", vel.device, *plan.head(), posm.data_ptr(), vel.data_ptr(), phi.data_ptr(),
                out_rows.data_ptr())
    return out_rows


# ---------------------------------------------------------------- Hermite per scene (csrc/direct_batch_hermite.hip)
def _hws(plan: BatchPlan, ws) -> None:
    if _nbytes(ws) < plan.hermite_workspace_bytes():
        raise _lib.NbdError("batch Hermite workspace too small")


def batch_accel_jerk(plan: BatchPlan, pos, vel, mass, eps2, g, acc_out, jerk_out, posm, hws) -> None:
    """acc_out, jerk_out = the acceleration and jerk of every scene's current state (a plain pack first; leaves
    posm = {x, m}). eps2, g: device fp32 (S,); hws: plan.hermite_workspace()."""
    plan.check_state(posm, None, (pos, "pos"), (vel, "vel"), (mass, "mass"), (acc_out, "acc_out"),
                     (jerk_out, "jerk_out"))
    _hws(plan, hws)
    _lib.launch("nbd_batch_accel_jerk_f32", pos.device, *plan.head(), pos.data_ptr(), vel.data_ptr(), mass.data_ptr(),
                _param(eps2, plan, "softening_sq"), _param(g, plan, "g_const"), acc_out.data_ptr(), jerk_out.data_ptr(),
                posm.data_ptr(), hws.data_ptr(), _nbytes(hws))


def batch_hermite_step(plan: BatchPlan, pos, vel, acc_in, jerk_in, acc_out, jerk_out, mass, hdt, eps2, g, posm,
                       hws) -> None:
    """One Hermite step of every scene: pos, vel in place; acc_out, jerk_out (may be acc_in, jerk_in); posm = {x1, m}.
    hdt: device fp32 (5, S) rows dt, dt/2, dt^2/2, dt^3/6, dt^2/12, each formed from the double dt and rounded once."""
    plan.check_state(posm, None, (pos, "pos"), (vel, "vel"), (acc_in, "acc_in"), (jerk_in, "jerk_in"),
                     (acc_out, "acc_out"), (jerk_out, "jerk_out"), (mass, "mass"))
    _chk(hdt, (5, plan.n_scenes), "hdt")
    _hws(plan, hws)
    _lib.launch("nbd_batch_hermite_step_f32", pos.device, *plan.head(), pos.data_ptr(), vel.data_ptr(),
                acc_in.data_ptr(), jerk_in.data_ptr(), acc_out.data_ptr(), jerk_out.data_ptr(), mass.data_ptr(),
                hdt.data_ptr(), _param(eps2, plan, "softening_sq"), _param(g, plan, "g_const"), posm.data_ptr(),
                hws.data_ptr(), _nbytes(hws))


# ------------------------------------------- double-precision Hermite per scene (csrc/direct_batch_hermite_f64.hip)
BATCH_F64_PARAM_ROWS = 8        # NBD_BATCH_F64_PARAM_ROWS: G, eps^2, eps, dt, dt/2, dt^2/2, dt^3/6, dt^2/12
BATCH_H6_PARAM_ROWS = 13        # NBD_BATCH_H6_PARAM_ROWS: G, eps^2, eps, then Hermite6Step's ten members


def batch_f64_params(g, eps, dt) -> list:
    """The rows of the float64 calls' parameter table from each scene's Python doubles (g, eps, dt: S floats each), formed
    by the expressions of the one-system float64 path: eps ** 2, and hermite_step_constants<double>'s 0.5 * dt,
    0.5 * dt * dt, dt * dt * dt / 6.0, dt * dt / 12.0. -> BATCH_F64_PARAM_ROWS lists of S floats."""
    return [[float(x) for x in g], [float(e) ** 2 for e in eps], [float(e) for e in eps], [float(d) for d in dt],
            [0.5 * d for d in dt], [0.5 * d * d for d in dt], [d * d * d / 6.0 for d in dt], [d * d / 12.0 for d in dt]]


def _chk_f64_batch(plan: BatchPlan, posd, veld, ws, params, *arrays):
    """The checks every batch_*_f64 call makes: a float64 plan, the state arrays, the packed rows, the workspace and the
    parameter table (each None where the call takes none)."""
    if plan.dtype != F64:
        raise _lib.NbdError("batch float64 call: the plan was built for float32 (BatchPlan(..., dtype=torch.float64))")
    n = plan.n_total
    for t, nm in arrays:
        _chk(t, (n,) if nm in ("mass", "phi") else (n, 3), nm, F64)
    for t, nm in ((posd, "posd"), (veld, "veld")):
        if t is not None:
            _chk_min_rows(t, plan.posm_rows, 4, nm, F64)
    if ws is not None and _nbytes(ws) < plan.workspace_bytes:
        raise _lib.NbdError("batch float64 workspace too small")
    if params is not None:                 # the plan's own table: the 6th-order plan's is taller, rows 0-2 the same
        _chk(params, (plan.param_rows, plan.n_scenes), "params", F64)


def alloc_batch_rows_f64(plan: BatchPlan) -> torch.Tensor:
    """Zeroed (rows, 4) float64 rows of a float64 plan: posd or veld."""
    return torch.zeros((max(plan.posm_rows, 1), 4), dtype=F64, device=plan.device)


def batch_pack_f64(plan: BatchPlan, pos, vel, mass, posd, veld) -> None:
    """posd = {x, m}, veld = {v, 0} of every scene."""
    _chk_f64_batch(plan, posd, veld, None, None, (pos, "pos"), (vel, "vel"), (mass, "mass"))
    _lib.launch("nbd_batch_pack_f64", pos.device, *plan.head(), pos.data_ptr(), vel.data_ptr(), mass.data_ptr(),
                posd.data_ptr(), veld.data_ptr())


def batch_accel_jerk_f64(plan: BatchPlan, pos, vel, mass, params, acc_out, jerk_out, posd, veld, ws) -> None:
    """batch_accel_jerk in float64 (accel_jerk_f64 per scene, bit for bit). params: device float64
    (BATCH_F64_PARAM_ROWS, S) as batch_f64_params forms it; ws: plan.workspace()."""
    _chk_f64_batch(plan, posd, veld, ws, params, (pos, "pos"), (vel, "vel"), (mass, "mass"), (acc_out, "acc_out"),
                   (jerk_out, "jerk_out"))
    _lib.launch("nbd_batch_accel_jerk_f64", pos.device, *plan.head(), pos.data_ptr(), vel.data_ptr(), mass.data_ptr(),
                params.data_ptr(), acc_out.data_ptr(), jerk_out.data_ptr(), posd.data_ptr(), veld.data_ptr(),
                ws.data_ptr(), _nbytes(ws))


def batch_hermite_step_f64(plan: BatchPlan, pos, vel, acc_in, jerk_in, acc_out, jerk_out, mass, params, posd, veld,
                           ws) -> None:
    """batch_hermite_step in float64 (hermite_step_f64 per scene, bit for bit): pos, vel in place; acc_out, jerk_out (may
    be acc_in, jerk_in); posd = {x1, m}; veld is scratch."""
    _chk_f64_batch(plan, posd, veld, ws, params, (pos, "pos"), (vel, "vel"), (acc_in, "acc_in"), (jerk_in, "jerk_in"),
                   (acc_out, "acc_out"), (jerk_out, "jerk_out"), (mass, "mass"))
    _lib.launch("nbd_batch_hermite_step_f64", pos.device, *plan.head(), pos.data_ptr(), vel.data_ptr(),
                acc_in.data_ptr(), jerk_in.data_ptr(), acc_out.data_ptr(), jerk_out.data_ptr(), mass.data_ptr(),
                params.data_ptr(), posd.data_ptr(), veld.data_ptr(), ws.data_ptr(), _nbytes(ws))


def batch_energies_f64(plan: BatchPlan, posd, vel, params, out_uk, ws) -> torch.Tensor:
    """out_uk (S, 2) float64 = {U_s, K_s} (energy_f64 per scene, bit for bit) from posd and vel; asynchronous."""
    _chk_f64_batch(plan, posd, None, ws, params, (vel, "vel"))
    _chk(out_uk, (plan.n_scenes, 2), "out_uk", F64)
    _lib.launch("nbd_batch_energies_f64", vel.device, *plan.head(), posd.data_ptr(), vel.data_ptr(), params.data_ptr(),
                out_uk.data_ptr(), ws.data_ptr(), _nbytes(ws))
    return out_uk


def batch_potential_f64(plan: BatchPlan, posd, params, phi_out, ws) -> torch.Tensor:
    """phi_out (N_total,) float64 (potential_f64 per scene, bit for bit) from posd; asynchronous."""
    _chk_f64_batch(plan, posd, None, ws, params, (phi_out, "phi"))
    _lib.launch("nbd_batch_potential_f64", posd.device, *plan.head(), posd.data_ptr(), params.data_ptr(),
                phi_out.data_ptr(), ws.data_ptr(), _nbytes(ws))
    return phi_out


def batch_invariants_state_f64(plan: BatchPlan, pos, vel, mass, phi, out_rows) -> torch.Tensor:
    """out_rows (S, 16) float64 = invariants_state_f64 of every scene (bit for bit) from the state and phi."""
    _chk_f64_batch(plan, None, None, None, None, (pos, "pos"), (vel, "vel"), (mass, "mass"), (phi, "phi"))
    _chk(out_rows, (plan.n_scenes, INVARIANT_ROW), "out_rows", F64)
    _lib.launch("nbd_batch_invariants_state_f64", vel.device, *plan.head(), pos.data_ptr(), vel.data_ptr(),
                mass.data_ptr(), phi.data_ptr(), out_rows.data_ptr())
    return out_rows


# ------------------------------------------------- 6th-order Hermite per scene (csrc/direct_batch_hermite_f64.hip)
def batch_h6_params(g, eps, dt) -> list:
    """The rows of the 6th-order calls' parameter table from each scene's Python doubles (g, eps, dt: S floats each):
    batch_f64_params' first three rows, then hermite6_step_constants' expressions (dt2 = dt * dt, dt3 = dt2 * dt).
    -> BATCH_H6_PARAM_ROWS lists of S floats."""
    dt = [float(d) for d in dt]
    dt2 = [d * d for d in dt]
    dt3 = [d2 * d for d2, d in zip(dt2, dt)]
    return [[float(x) for x in g], [float(e) ** 2 for e in eps], [float(e) for e in eps], dt,
            [0.5 * d for d in dt], [0.5 * d2 for d2 in dt2], [d3 / 6.0 for d3 in dt3], [d2 * d2 / 24.0 for d2 in dt2],
            [d2 * d3 / 120.0 for d2, d3 in zip(dt2, dt3)], [d2 / 10.0 for d2 in dt2], [d3 / 120.0 for d3 in dt3],
            dt2, dt3]


def _chk_h6_batch(plan: BatchPlan, posd, veld, accd, ws, params, *arrays):
    """_chk_f64_batch for a 6th-order plan, and the third packed array."""
    if plan.dtype != F64 or plan.order != 6:
        raise _lib.NbdError("batch 6th-order call: the plan was not built for it "
                            "(BatchPlan(..., dtype=torch.float64, order=6))")
    _chk_f64_batch(plan, posd, veld, ws, params, *arrays)
    _chk_min_rows(accd, plan.posm_rows, 4, "accd", F64)


def batch_hermite6_pack_f64(plan: BatchPlan, pos, vel, mass, posd, veld, accd, acc=None) -> None:
    """posd = {x, m}, veld = {v, 0}, accd = {a, 0} of every scene (acc None: zero rows)."""
    _chk_h6_batch(plan, posd, veld, accd, None, None, (pos, "pos"), (vel, "vel"), (mass, "mass"),
                  *(((acc, "acc"),) if acc is not None else ()))
    _lib.launch("nbd_batch_hermite6_pack_f64", pos.device, *plan.head(), pos.data_ptr(), vel.data_ptr(), _lib.ptr(acc),
                mass.data_ptr(), posd.data_ptr(), veld.data_ptr(), accd.data_ptr())


def batch_accel_jerk_snap_f64(plan: BatchPlan, posd, veld, accd, params, acc_out, jerk_out, snap_out, ws) -> None:
    """acc_out, jerk_out, snap_out of every scene from the packed rows (accel_jerk_snap_f64 per scene, bit for bit).
    params: device float64 (BATCH_H6_PARAM_ROWS, S) as batch_h6_params forms it; ws: plan.workspace()."""
    _chk_h6_batch(plan, posd, veld, accd, ws, params, (acc_out, "acc_out"), (jerk_out, "jerk_out"),
                  (snap_out, "snap_out"))
    _lib.launch("nbd_batch_accel_jerk_snap_f64", posd.device, *plan.head(), posd.data_ptr(), veld.data_ptr(),
                accd.data_ptr(), params.data_ptr(), acc_out.data_ptr(), jerk_out.data_ptr(), snap_out.data_ptr(),
                ws.data_ptr(), _nbytes(ws))


def batch_hermite6_step_f64(plan: BatchPlan, pos, vel, acc_in, jerk_in, snap_in, crackle_in, acc_out, jerk_out, snap_out,
                            crackle_out, mass, params, posd, veld, accd, ws) -> None:
    """One 6th-order Hermite step of every scene (hermite6_step_f64 per scene, bit for bit): pos, vel in place; every
    output may be its input; posd = {x1, m}; veld and accd are scratch."""
    _chk_h6_batch(plan, posd, veld, accd, ws, params, (pos, "pos"), (vel, "vel"), (acc_in, "acc_in"),
                  (jerk_in, "jerk_in"), (snap_in, "snap_in"), (crackle_in, "crackle_in"), (acc_out, "acc_out"),
                  (jerk_out, "jerk_out"), (snap_out, "snap_out"), (crackle_out, "crackle_out"), (mass, "mass"))
    _lib.launch("nbd_batch_hermite6_step_f64", pos.device, *plan.head(), pos.data_ptr(), vel.data_ptr(),
                acc_in.data_ptr(), jerk_in.data_ptr(), snap_in.data_ptr(), crackle_in.data_ptr(), acc_out.data_ptr(),
                jerk_out.data_ptr(), snap_out.data_ptr(), crackle_out.data_ptr(), mass.data_ptr(), params.data_ptr(),
                posd.data_ptr(), veld.data_ptr(), accd.data_ptr(), ws.data_ptr(), _nbytes(ws))


# ------------------------- block-timestep Hermite per scene, 4th and 6th order (csrc/direct_batch_hermite_block_f64.hip)
BATCH_HBLOCK_PARAM_ROWS = 5     # NBD_BATCH_HBLOCK_PARAM_ROWS: G, eps^2, eps, dt, eta


def batch_hblock_params(g, eps, dt, eta) -> list:
    """The rows of the batched block step's parameter table from each scene's Python doubles, formed as the one-system
    block simulators hand them to their entries: float(g), float(eps) ** 2, float(dt), float(eta).
    -> BATCH_HBLOCK_PARAM_ROWS lists of S floats."""
    return [[float(x) for x in g], [float(e) ** 2 for e in eps], [float(e) for e in eps], [float(d) for d in dt],
            [float(x) for x in eta]]


class BatchBlockPlan:
    """The static work list of the batched block-timestep step (nbd_batch_hblock_f64_plan and the order's plan_fill),
    next to a float64 BatchPlan of the same scenes: `n_items` workgroups per force launch (every scene's worst case),
    `workspace_bytes` for the active lists and the partial sums (order 4: 6 doubles per listed body and slab; 6: 9)."""

    def __init__(self, sizes, device, order: int = 4):
        sizes = [int(n) for n in sizes]
        if not sizes or min(sizes) < 0:
            raise _lib.NbdError("batch: need at least one scene and no negative size")
        if order not in (4, 6):
            raise _lib.NbdError(f"batch block plan: order must be 4 or 6, got {order!r}")
        self.order = order
        self.offsets = np.zeros(len(sizes) + 1, dtype=np.int32)
        np.cumsum(sizes, out=self.offsets[1:])
        self.n_scenes, self.n_total = len(sizes), int(self.offsets[-1])
        items, rows = ctypes.c_int(), ctypes.c_int()
        pb, wb = ctypes.c_size_t(), ctypes.c_size_t()
        scenes = (self.offsets.ctypes.data, self.n_scenes)
        tag = "hblock" if order == 4 else "hblock6"
        _lib.call("nbd_batch_hblock_f64_plan", *scenes, items, rows, pb)
        _lib.call(f"nbd_batch_{tag}_f64_workspace_bytes", *scenes, wb)
        self.n_items, self.posm_rows, self.plan_bytes, self.workspace_bytes = items.value, rows.value, pb.value, wb.value
        self.host = np.zeros((self.plan_bytes + 15) // 16 * 4, dtype=np.int32)
        _lib.call(f"nbd_batch_{tag}_f64_plan_fill", *scenes, self.host.ctypes.data, self.plan_bytes)
        self.plan = torch.from_numpy(self.host).to(device) if device is not None else None
        self.device = self.plan.device if self.plan is not None else None

    def head(self):
        return (self.offsets.ctypes.data, self.n_scenes, self.plan.data_ptr(), self.plan_bytes)

    def workspace(self) -> torch.Tensor:
        return alloc_bytes(self.workspace_bytes, self.device)

    def sched(self) -> torch.Tensor:
        """The zeroed device records: the ensemble's, then one per scene."""
        return torch.zeros((self.n_scenes + 1, HBLOCK_SCHED_INTS), dtype=torch.int32, device=self.device)

    def counters(self) -> torch.Tensor:
        """The zeroed per-scene {block steps, pair interactions}."""
        return torch.zeros((self.n_scenes, 2), dtype=torch.int64, device=self.device)


def _chk_bblock(plan: BatchBlockPlan, state, mass, ticks, levels, params, bsched, rows, ws):
    """The arguments of a batched block call, each None where the call takes none: the (N_total, 3) state arrays, the int32
    schedule arrays, the parameter table, the records, the packed rows and the workspace."""
    n = plan.n_total
    _chk_n3(F64, n, _HBLOCK_STATE, *state)
    if mass is not None:
        _chk(mass, (n,), "mass", F64)
    for t, nm in ((ticks, "ticks"), (levels, "levels")):
        if t is not None:
            _chk(t, (n,), nm, torch.int32)
    _chk(params, (BATCH_HBLOCK_PARAM_ROWS, plan.n_scenes), "params", F64)
    _chk(bsched, (plan.n_scenes + 1, HBLOCK_SCHED_INTS), "bsched", torch.int32)
    for t, nm in zip(rows, ("posd", "veld", "accd")):
        _chk_min_rows(t, plan.posm_rows, 4, nm, F64)
    if ws is not None and _nbytes(ws) < plan.workspace_bytes:
        raise _lib.NbdError("batch block workspace too small")


def batch_hblock_init_levels(plan: BatchBlockPlan, acc, jerk, params, max_level: int, ticks, levels, bsched,
                             mask=None) -> None:
    """ticks = 0 and levels from dt_i = (eta_s / 2) |a| / |j| quantised to dt_s 2^-k for every scene (mask: a device int32
    (S,), only the scenes it marks); the scenes' clamp counts and histograms, the ensemble's histogram, tick 0."""
    _chk_bblock(plan, (acc, jerk), None, ticks, levels, params, bsched, (), None)
    if mask is not None:
        _chk(mask, (plan.n_scenes,), "mask", torch.int32)
    _lib.launch("nbd_batch_hblock_init_levels_f64", bsched.device, *plan.head(), acc.data_ptr(), jerk.data_ptr(),
                params.data_ptr(), int(max_level), _lib.ptr(mask), ticks.data_ptr(), levels.data_ptr(), bsched.data_ptr())


def batch_hblock_schedule(plan: BatchBlockPlan, levels, max_level: int, bsched, counters, workspace,
                          host_sched=None) -> None:
    """t_next and every scene's active list of the next block step (bsched, the workspace), the per-scene counters.
    host_sched: an int32 CPU tensor of at least 4 elements that receives {t_next, n_act_total, ...} after a stream sync."""
    _chk(levels, (plan.n_total,), "levels", torch.int32)
    _chk(bsched, (plan.n_scenes + 1, HBLOCK_SCHED_INTS), "bsched", torch.int32)
    _chk(counters, (plan.n_scenes, 2), "counters", torch.int64)
    if host_sched is not None and (host_sched.is_cuda or host_sched.dtype != torch.int32 or host_sched.numel() < 4):
        raise _lib.NbdError("batch_hblock_schedule: host_sched must be an int32 CPU tensor of 4 elements")
    _lib.launch("nbd_batch_hblock_schedule", levels.device, *plan.head(), levels.data_ptr(), int(max_level),
                bsched.data_ptr(), counters.data_ptr(), workspace.data_ptr(), _nbytes(workspace), _lib.ptr(host_sched))


def _bblock_entry(plan: BatchBlockPlan, stage: str) -> str:
    return f"nbd_batch_{'hblock' if plan.order == 4 else 'hblock6'}_{stage}_f64"


def batch_hblock_predict(plan: BatchBlockPlan, state, mass, ticks, params, max_level: int, bsched, rows) -> None:
    """First launch of a batched block step: every body predicted to t_next into the packed rows. state: (pos, vel, acc,
    jerk[, snap, crackle]); rows: (posd, veld[, accd])."""
    _chk_bblock(plan, state, mass, ticks, None, params, bsched, rows, None)
    _lib.launch(_bblock_entry(plan, "predict"), bsched.device, *plan.head(), *_ptrs(state), mass.data_ptr(),
                ticks.data_ptr(), params.data_ptr(), int(max_level), bsched.data_ptr(), *_ptrs(rows))


def batch_hblock_force(plan: BatchBlockPlan, rows, params, bsched, workspace) -> None:
    """Second launch: the partial sums of every scene's listed bodies."""
    _chk_bblock(plan, (), None, None, None, params, bsched, rows, workspace)
    _lib.launch(_bblock_entry(plan, "force"), bsched.device, *plan.head(), *_ptrs(rows), params.data_ptr(),
                bsched.data_ptr(), workspace.data_ptr(), _nbytes(workspace))


def batch_hblock_correct(plan: BatchBlockPlan, state, mass, ticks, levels, params, max_level: int, bsched, posd,
                         workspace) -> None:
    """Third launch: slab sum, corrector and new level of every listed body; posd = {x1, m} for them."""
    _chk_bblock(plan, state, mass, ticks, levels, params, bsched, (posd,), workspace)
    _lib.launch(_bblock_entry(plan, "correct"), bsched.device, *plan.head(), *_ptrs(state), mass.data_ptr(),
                ticks.data_ptr(), levels.data_ptr(), params.data_ptr(), int(max_level), bsched.data_ptr(),
                posd.data_ptr(), workspace.data_ptr(), _nbytes(workspace))


def batch_hblock_step(plan: BatchBlockPlan, state, mass, ticks, levels, params, max_level: int, bsched, rows,
                      workspace) -> None:
    """Predict, force and correct of the block step batch_hblock_schedule has just listed (three launches), in place."""
    _chk_bblock(plan, state, mass, ticks, levels, params, bsched, rows, workspace)
    _lib.launch(_bblock_entry(plan, "step"), bsched.device, *plan.head(), *_ptrs(state), mass.data_ptr(),
                ticks.data_ptr(), levels.data_ptr(), params.data_ptr(), int(max_level), bsched.data_ptr(), *_ptrs(rows),
                workspace.data_ptr(), _nbytes(workspace))
