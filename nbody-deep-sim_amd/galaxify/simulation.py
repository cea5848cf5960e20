"""MI355X drop-in for the reference integrator module (src/galaxify/simulation.py).

Same public surface -- SimulationState, BaseSimulator, LeapFrogSimulator, EulerSimulator with
the kw-only constructor, attributes (positions, velocities, accelerations, masses, n, dt,
g_const, softening, calc_energy, device) and methods step()/run()/compute_accelerations()/
compute_energies() -- but every O(N^2)/O(N) update runs in hand-written HIP kernels
(csrc/direct_force.hip) through the C-ABI of include/nbd.h. There is no CPU path: device="cpu"
or a missing libnbd_hip.so raises.

Addition over the reference (which has no distributed code): `process_group=` range-partitions
the bodies over the ranks of a torch.distributed group (one process per GPU, RCCL over xGMI);
positions/velocities/accelerations then hold the local shard [lo, hi) and `gather()` assembles
the global arrays. See nbd/dist.py and DESIGN.md.

Second addition: `BatchedSimulator` advances many independent systems with one set of launches per step
(csrc/direct_batch.hip).

Third addition: `HermiteSimulator`, the shared-timestep 4th-order Hermite predictor-corrector (one acceleration + jerk
evaluation per step; csrc/direct_hermite.hip).

Fourth addition: `BlockHermiteSimulator`, the same scheme with individual block timesteps inside each output interval
(csrc/direct_hermite_block.hip).

Sixth addition: `HermiteSimulator(dtype=torch.float64)`, the same scheme with float64 state, scalars and pair arithmetic
(csrc/direct_hermite_f64.hip). The default stays float32 and takes the paths it took.

Seventh addition: `BlockHermiteSimulator(dtype=torch.float64)`, block timesteps in that float64 format
(csrc/direct_hermite_block_f64.hip). Again the default is float32 and takes the paths it took.

Fifth addition: `compute_potentials()` / `compute_invariants()` and `calc_invariants=`: the per-body potential of the
softening the force uses and the conserved quantities formed from it (`Invariants`; csrc/direct_diag.hip).
`compute_energies()`, `u_energy` and `k_energy` keep the reference's convention.

Eighth addition: `compute_accelerations()` is differentiable. When torch records a graph and `positions` or `masses`
requires grad, its result carries a grad_fn whose backward is a HIP kernel (csrc/direct_grad.hip; `nbd.autograd.direct_accel`
is the function form; DESIGN.md K-VJP), as the reference's nine lines of torch do by themselves. Otherwise nothing changes.

Ninth addition: `BatchedSimulator(integrator="hermite", dtype=torch.float64)`, the float64 Hermite step on every scene of
a batch with one set of launches, each scene bit-identical to `HermiteSimulator(dtype=torch.float64)` of that scene alone,
and run() in captured chunks (csrc/direct_batch_hermite_f64.hip). The default stays float32.

Tenth addition: `HermiteSimulator.compute_accelerations_and_jerks()` is differentiable in the same way, with respect to
`positions`, `velocities` and `masses` (csrc/direct_hermite_grad.hip; `nbd.autograd.direct_accel_jerk` is the function form;
DESIGN.md K-HVJP). `BlockHermiteSimulator` inherits it; `BatchedSimulator` does not have it.

Eleventh addition: `LeapFrogSimulator(dtype=torch.float64)` and `EulerSimulator(dtype=torch.float64)`, the reference's two
schemes with float64 state, scalars and pair arithmetic (csrc/direct_leapfrog_f64.hip): un-sharded, run()
eager. The default stays float32 and takes the paths it took. The float64 `compute_accelerations()` of every simulator is
that unit's acceleration-only kernel, bit-identical to the acceleration of the Hermite force.

Twelfth addition: `TreeLeapFrogSimulator`, the leapfrog step with a Barnes-Hut force in O(N log N) (csrc/tree_force.hip;
DESIGN.md K-T): float32, one GPU. `LeapFrogSimulator` is untouched.
"""
from __future__ import annotations

import os
import time
from dataclasses import dataclass

import numpy as np
import torch

from nbd import _lib, direct
from nbd import dist as nbd_dist


@dataclass
class Invariants:
    """The conserved quantities of one system (a row of nbd_invariants_f64): total mass, centre of mass, linear and
    angular momentum, kinetic energy K = sum 1/2 m |v|^2, potential energy U = 1/2 sum m_i phi_i of the Plummer potential
    the force derives from (phi_i = -G sum_{j != i} m_j (r_ij^2 + eps^2)^(-1/2)), E = K + U and the virial ratio
    Q = -2 K / U (0 when U = 0). Every product is formed in fp64 from the fp32 state, so k_energy differs from
    compute_energies()'s K (fp32 products) in the last digits; u_energy differs from compute_energies()'s U by
    construction wherever the softening is not 0 (that one is the reference's -G m_i m_j / (|r| + eps))."""

    mass: float
    com: tuple
    momentum: tuple
    angular_momentum: tuple
    k_energy: float
    u_energy: float
    energy: float
    virial_ratio: float

    @classmethod
    def from_row(cls, row) -> "Invariants":
        """From the 16 doubles {M, C (3), P (3), L (3), K, U, E, Q, 0, 0} (a list, array or CPU tensor)."""
        r = [float(x) for x in (row.tolist() if hasattr(row, "tolist") else row)]
        if len(r) != direct.INVARIANT_ROW:
            raise ValueError(f"Invariants.from_row: expected {direct.INVARIANT_ROW} values, got {len(r)}")
        return cls(mass=r[0], com=tuple(r[1:4]), momentum=tuple(r[4:7]), angular_momentum=tuple(r[7:10]),
                   k_energy=r[10], u_energy=r[11], energy=r[12], virial_ratio=r[13])

    def row(self) -> list:
        """The 16 doubles from_row() takes."""
        return [self.mass, *self.com, *self.momentum, *self.angular_momentum, self.k_energy, self.u_energy, self.energy,
                self.virial_ratio, 0.0, 0.0]


@dataclass
class SimulationState:
    """Snapshot of one step; field names and order as simulation.py:8-18, then `invariants` (an addition: the
    Invariants of the state after the step when the simulator was built with calc_invariants=True, else None)."""

    step: int
    step_time: float
    positions: torch.Tensor
    velocities: torch.Tensor
    accelerations: torch.Tensor
    u_energy: float = None
    k_energy: float = None
    invariants: Invariants = None


def _to_device(x, device, dtype) -> torch.Tensor:
    """A device copy in `dtype`, converted directly (float64 never through float32); simulation.py:58-65 makes its fp32
    copies with torch.tensor(...)."""
    if isinstance(x, torch.Tensor):
        return x.detach().to(device=device, dtype=dtype, copy=True).contiguous()
    return torch.tensor(np.asarray(x), dtype=dtype, device=device).contiguous()


def _resolve_device(device) -> torch.device:
    """Device rule of simulation.py:46-51 ("cuda" is PyTorch-ROCm's name for the MI355X), minus
    the CPU branch: this build has no CPU compute path."""
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("galaxify (MI355X build): no GPU visible and there is no CPU path")
        return torch.device("cuda", torch.cuda.current_device())
    if device == "cuda":
        return torch.device("cuda", torch.cuda.current_device())
    if device == "cpu":
        raise RuntimeError("galaxify (MI355X build): device='cpu' is not provided by this build; "
                           "the HIP kernels are the only compute path (use the reference for CPU)")
    raise ValueError("device debe ser 'cuda', 'cpu' o None")


class _ChunkedRun:
    """run() in captured chunks, for BaseSimulator and BatchedSimulator. Below ~16 k bodies a step is a handful of
    microseconds of GPU work and run() is bound by its per-step host work (events, seven ctypes launches, three staged
    copies, a state object): 110-280 us per step wall for 15-25 us of GPU time at the reference's dataset sizes (100-2000
    bodies x 1000 steps, s01-dataset-generation.py:192-214). Those systems run in CHUNKS captured into a hipGraph: per
    step the integrator's launches, the energy launches and ONE snapshot launch into a device ring; per chunk one replay,
    one sync, one device->host copy. Same kernels in the same order as step(): bit-identical states (tested).

    The simulator supplies: `_carried`, the public arrays a step rebinds paired with the static buffers a captured step
    updates in place; `_chunk_scalars()`, every scalar the body bakes into its launches; `_chunk_body(m)` -> (body(count),
    device buffers to copy per chunk); `_emit_states(host buffers, m, first, GPU seconds of each step, out)`; and
    `_run_eager(steps, first, out)` for the tail."""

    GRAPH_RUN_CHUNK = 32
    _carried = (("accelerations", "_acc_g"),)

    def _statics(self) -> list:
        """The static buffers of the carried arrays, allocated on first use."""
        for public, static in self._carried:
            if getattr(self, static, None) is None:
                setattr(self, static, torch.empty_like(getattr(self, public)))
        return [getattr(self, static) for _, static in self._carried]

    def _chunk_graph(self, m: int):
        """(graph, device buffers) for a chunk of m steps; captured once per key and kept."""
        cache = self.__dict__.setdefault("_run_graphs", {})
        statics = self._statics()
        # a graph bakes in buffer addresses and scalar arguments: every array that can be rebound after construction
        # and every scalar the caller may have changed is in the key (the scratch is allocated once and never rebound)
        key = (m, *(t.data_ptr() for t in (self.positions, self.velocities, self.masses, *statics)),
               *self._chunk_scalars())
        if key in cache:
            return cache[key]
        if len(cache) > 8:
            cache.clear()
        body, bufs = self._chunk_body(m)
        dev = self.device
        # capture on a side stream; the state is saved and restored around the (executed) warm-up pass
        saved = [self.positions, self.velocities, *statics]
        keep = [t.clone() for t in saved]

        def restore():
            for t, k in zip(saved, keep):
                t.copy_(k)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            body(1)                                          # every kernel of a step once (lazy initialisations)
        torch.cuda.current_stream(dev).wait_stream(side)
        restore()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            body(m)
        restore()
        cache[key] = (graph, bufs)
        return cache[key]

    def _run_chunked(self, steps: int, big: int, out):
        """Chunks of `big` steps, then of 8; the last < 8 steps run eagerly."""
        done = 0
        while steps - done >= 8:
            m = big if steps - done >= big else 8
            graph, bufs = self._chunk_graph(m)              # (capture leaves the state untouched)
            if done == 0:                                    # a caller's handle on the old accelerations stays valid
                for (public, _), static in zip(self._carried, self._statics()):
                    static.copy_(getattr(self, public))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            host = [b.cpu() for b in bufs]                   # one device->host copy per buffer (synchronises)
            self._emit_states(host, m, done, [e0.elapsed_time(e1) * 1e-3 / m] * m, out)   # the chunk's GPU time, spread
            done += m
        if done:
            for (public, _), static in zip(self._carried, self._statics()):
                setattr(self, public, static.clone())        # rebound, as step() does (simulation.py:168)
        if done < steps:
            self._run_eager(steps - done, done, out)


def _hermite_shard_scratch(s, alloc_rows, workspace, width, dtype, own_mass):
    """The range-sharded Hermite scratch of simulator `s`, from what a number format names (its row allocator, workspace
    function, row width and dtype): the rank's own predicted rows -- source of its local block and send buffer of the
    gather, max_count of them so that ragged shards send equal, zero-padded pieces --, the gathered rows of all bodies,
    the partial sums of the two force launches, the gather, and with own_mass the rank's masses (BaseSimulator's scratch
    has them for _Float32)."""
    part = s.part
    s._rows_local = alloc_rows(part.max_count, s.device)
    s._rows_all = alloc_rows(s.n, s.device)
    s._hws = workspace(s.n, part.lo, part.n_local, s.device) if part.n_local else None
    s._hgather = nbd_dist.RowGather(part, width, dtype, s.device, s.process_group, collective=True)
    if own_mass:
        s._mass_local = s.masses[part.lo:part.hi].contiguous()


class _Float32:
    """The float32 number format: every nbd.direct call of a simulator `s` that depends on the format (the object keeps no
    state of its own). BaseSimulator uses the diagnostics, LeapFrogSimulator and EulerSimulator the scratch and the step
    of theirs as well (`_base_scratch`, `_leapfrog_step`, `_euler_step`), the Hermite simulators the rest; `_Float64` has
    the same methods. Packed sources: `s._posm` = {x, y, z, m} (BaseSimulator's) and `s._velp` = {vx, vy, vz, 0}.
    Scalars: eps^2 and G are the fp32 values formed AT CONSTRUCTION (`s._eps2`, `s._g`: a later change of `softening` or
    `g_const` does not reach the force); the energies read `s.softening`, and the step `s.dt`, at the launch. _Float64 reads
    all three at every launch. A quirk, kept as it was found: unifying it would change results."""

    dtype = torch.float32
    capturable = True               # run() may capture chunks of steps
    shardable = True                # there is a range-sharded step
    leapfrog_shardable = True       # ... and a range-sharded leapfrog / Euler step

    def bind_scalars(self, s):
        # fp32 scalars exactly as torch forms them from the Python doubles (simulation.py:82,88,164)
        s._eps2 = direct.f32(s.softening ** 2)
        s._g = direct.f32(s.g_const)

    def hermite_scratch(self, s):
        """BaseSimulator's scratch with its plain all-pairs force launch, then what the Hermite step adds."""
        s._init_scratch()
        if not s._sharded:
            s._velp = direct.alloc_posm(s.n, s.device)
            s._hws = direct.hermite_workspace(max(s.n, 1), s.device)
        else:
            _hermite_shard_scratch(s, direct.alloc_hermite_rows, direct.hermite_shard_workspace, direct.HERMITE_ROW,
                                   self.dtype, own_mass=False)

    def _base_scratch(self, s):
        """BaseSimulator's scratch (LeapFrogSimulator, EulerSimulator) and the first force."""
        s._init_scratch()

    # the un-sharded leapfrog and Euler steps (LeapFrogSimulator, EulerSimulator): acc_out may be acc_in
    def _leapfrog_step(self, s, acc_in, acc_out):
        direct.leapfrog_step(s.positions, s.velocities, acc_in, acc_out, s.masses, direct.f32(0.5 * s.dt),
                             direct.f32(s.dt), s._eps2, s._g, s._posm, s._ws, uniform=s._uniform)

    def _euler_step(self, s, acc_out):
        direct.euler_step(s.positions, s.velocities, acc_out, s.masses, direct.f32(s.dt), s._eps2, s._g, s._posm, s._ws)

    def pack(self, s):
        """posm[:n] = {x,y,z,m} of ALL bodies in global order (one all-gather when sharded)."""
        if not s._sharded:
            direct.pack_posm(s.positions, s.masses, out=s._posm)
        else:
            s._pack_local()
            s._gather.finish(s._gather.start(s._posm_local, s._posm), s._posm)

    def accel(self, s):
        if not s._sharded:
            direct.pack_posm(s.positions, s.masses, out=s._posm)
            return direct.accel(s._posm, s.n, s._posm, s.n, 0, s._eps2, s._g, workspace=s._ws)
        s._pack_local()
        return s._force_sharded()

    def accel_jerk(self, s):
        direct.hermite_pack(s.positions, s.velocities, s.masses, s._posm, s._velp)
        return direct.accel_jerk(s._posm, s._velp, s.n, s._eps2, s._g, workspace=s._hws)

    def hermite_step(self, s, acc, jerk, new_acc, new_jerk):
        direct.hermite_step(s.positions, s.velocities, acc, jerk, new_acc, new_jerk, s.masses, s.dt, s._eps2, s._g,
                            s._posm, s._hws)

    def energies(self, s, vel, out_uk=None, workspace=None):
        return direct.energy(s._posm, vel, s.n, direct.f32(s.softening), s._g, out_uk=out_uk, workspace=workspace)

    def potentials(self, s, phi):
        if getattr(s, "_diag_ws", None) is None:
            s._diag_ws = direct.potential_workspace(s.n, s.n, s.device)
        return direct.potential(s._posm, s.n, s._posm, s.n, 0, s._eps2, s._g, out=phi, workspace=s._diag_ws)

    def invariants(self, s, phi, out=None):
        return direct.invariants(s._posm, s.velocities, phi, s.n, out=out)

    # the range-sharded step's three calls on the scratch of hermite_scratch (HermiteSimulator._sharded_launches; carried
    # = the carried derivatives or None, new = the outputs, `_shard_force_outputs` of them for the force on its own); the
    # wrappers are looked up on nbd.direct when a call is made
    _shard_force_outputs = 2        # a, j

    def _shard_predict(self, s, carried):
        acc, jerk = carried or (None, None)
        direct.hermite_shard_predict(s.positions, s.velocities, s._mass_local, s._rows_local, acc, jerk, s.dt)

    def _shard_local(self, s):
        p = s.part
        direct.hermite_shard_force_local(s._rows_local, p.n_local, s.n, p.lo, s._eps2, s._hws)

    def _shard_remote(self, s, carried, new, **step):
        p = s.part
        direct.hermite_shard_force_remote(s._rows_all, s.n, s._rows_local, p.n_local, p.lo, s._eps2, s._g, *new,
                                          s._hws, **step)

    block_workspace = staticmethod(direct.hblock_workspace)
    block_init_levels = staticmethod(direct.hblock_init_levels)

    def block_step(self, s, n_act: int):
        direct.hblock_step(s.positions, s.velocities, s.accelerations, s.jerks, s.masses, s._ticks, s.levels, n_act,
                           s.max_level, s.dt, s.eta, s._eps2, s._g, s._sched, s._posm, s._velp, s._bws)


class _Float64:
    """The float64 number format of the Hermite simulators (csrc/direct_hermite_f64.hip, direct_hermite_block_f64.hip,
    direct_hermite_shard_f64.hip) and of LeapFrogSimulator and EulerSimulator (csrc/direct_leapfrog_f64.hip): `_Float32`'s methods over the float64 entries; nothing of the fp32 paths is allocated
    or launched. Packed sources: `s._posd` = {x, y, z, m}, `s._veld` = {vx, vy, vz, 0}; a step leaves `_posd` at the
    post-step state, and the invariants come from the state arrays. Sharded, the step works on 8-double rows
    (`_rows_local`, `_rows_all`) and only the energies pack `posd` rows, of the gathered state, per call. Scalars:
    softening, g_const and dt are read as the Python doubles AT EVERY LAUNCH, sharded or not (_Float32 forms eps^2 and G
    once, at construction). A quirk, kept as it was found."""

    dtype = torch.float64
    capturable = False              # run() is eager: there is no captured form
    shardable = True                # there is a range-sharded step
    leapfrog_shardable = False      # ... but no range-sharded leapfrog or Euler step

    def bind_scalars(self, s):           # nothing is formed at construction
        pass

    def _scalars(self, s):               # (softening^2, G) as the Python doubles, read when a launch is made
        return float(s.softening) ** 2, float(s.g_const)

    def hermite_scratch(self, s):
        if not s._sharded:
            s._posd, s._veld = direct.alloc_rows_f64(s.n, s.device), direct.alloc_rows_f64(s.n, s.device)
            s._hws = direct.hermite_f64_workspace(max(s.n, 1), s.device)
        else:
            self._shard_scratch(s)

    def _shard_scratch(self, s):
        _hermite_shard_scratch(s, direct.alloc_hermite_rows_f64, direct.hermite_shard_f64_workspace, direct.HERMITE_ROW,
                               self.dtype, own_mass=True)

    def pack(self, s):
        if not s._sharded:          # (sharded, only the energies read packed rows of all bodies: they pack them)
            direct.hermite_f64_pack(s.positions, s.velocities, s.masses, s._posd, s._veld)

    def _base_scratch(self, s):
        """The un-sharded scratch of hermite_scratch (`_posd`, `_veld`, `_hws`: the pack, the energies, the potentials and
        the invariants work on it as they are) and the first force."""
        self.hermite_scratch(s)
        s.accelerations = s.compute_accelerations()

    # csrc/direct_leapfrog_f64.hip; dt/2 is formed here, in Python
    def _leapfrog_step(self, s, acc_in, acc_out):
        direct.leapfrog_step_f64(s.positions, s.velocities, acc_in, acc_out, s.masses, 0.5 * s.dt, s.dt,
                                 *self._scalars(s), s._posd, s._hws)

    def _euler_step(self, s, acc_out):
        direct.euler_step_f64(s.positions, s.velocities, acc_out, s.masses, s.dt, *self._scalars(s), s._posd, s._hws)

    def accel(self, s):
        if s._sharded:              # (the sharded Hermite step's force; there is no sharded leapfrog in this format)
            return s.compute_accelerations_and_jerks()[0]
        self.pack(s)
        return direct.accel_f64(s._posd, s.n, *self._scalars(s), workspace=s._hws)

    def accel_jerk(self, s):
        self.pack(s)
        return direct.accel_jerk_f64(s._posd, s._veld, s.n, *self._scalars(s), workspace=s._hws)

    def hermite_step(self, s, acc, jerk, new_acc, new_jerk):
        direct.hermite_step_f64(s.positions, s.velocities, acc, jerk, new_acc, new_jerk, s.masses, s.dt,
                                *self._scalars(s), s._posd, s._veld, s._hws)

    def energies(self, s, vel, out_uk=None, workspace=None):
        if not s._sharded:
            return direct.energy_f64(s._posd, vel, s.n, s.softening, s.g_const, s._hws, out_uk=out_uk)
        # occasional use: `vel` is the gathered velocities; a blocking gather of the positions, one pack of the gathered
        # state with the replicated masses, the un-sharded entry. Scratch per call. Every rank gets the global sums.
        posd, veld = direct.alloc_rows_f64(s.n, s.device), direct.alloc_rows_f64(s.n, s.device)
        direct.hermite_f64_pack(s.gather("positions"), vel, s.masses, posd, veld)
        return direct.energy_f64(posd, vel, s.n, s.softening, s.g_const, direct.hermite_f64_workspace(s.n, s.device),
                                 out_uk=out_uk)

    def potentials(self, s, phi):
        return direct.potential_f64(s._posd, s.n, *self._scalars(s), s._hws, out=phi)

    def invariants(self, s, phi, out=None):
        return direct.invariants_state_f64(s.positions, s.velocities, s.masses, phi, out=out)

    _shard_force_outputs = 2        # a, j

    def _shard_predict(self, s, carried):
        acc, jerk = carried or (None, None)
        direct.hermite_shard_predict_f64(s.positions, s.velocities, s._mass_local, s._rows_local, acc, jerk, s.dt)

    def _shard_local(self, s):
        p = s.part
        direct.hermite_shard_force_local_f64(s._rows_local, p.n_local, s.n, p.lo, self._scalars(s)[0], s._hws)

    def _shard_remote(self, s, carried, new, **step):
        p = s.part
        direct.hermite_shard_force_remote_f64(s._rows_all, s.n, s._rows_local, p.n_local, p.lo, *self._scalars(s),
                                              *new, s._hws, **step)

    block_workspace = staticmethod(direct.hblock_f64_workspace)
    block_init_levels = staticmethod(direct.hblock_init_levels_f64)

    def block_step(self, s, n_act: int):
        direct.hblock_step_f64(s.positions, s.velocities, s.accelerations, s.jerks, s.masses, s._ticks, s.levels, n_act,
                               s.max_level, s.dt, s.eta, *self._scalars(s), s._sched, s._posd, s._veld, s._bws)

    # a block step divided over the ranks of a group (csrc/direct_hermite_block_split_f64.hip; _BlockSteps._split_step):
    # the order, the predictor of all bodies, the state arrays a result row carries and the ones the rows are formed from
    block_order = 4
    split_row = direct.HBLOCK_SPLIT_ROW

    def _block_predict(self, s):
        direct.hblock_predict_f64(s.positions, s.velocities, s.accelerations, s.jerks, s.masses, s._ticks, s.levels,
                                  s.max_level, s.dt, s._sched, s._posd, s._veld)

    def _block_state(self, s):
        return s.positions, s.velocities, s.accelerations, s.jerks

    def _block_rows_in(self, s):
        return self._block_state(s), (s._posd, s._veld)


class _Hermite6Float64(_Float64):
    """The number format of Hermite6Simulator: `_Float64` with the calls that differ for the 6th order
    (csrc/direct_hermite_f64.hip; sharded, the 6th-order entries of csrc/direct_hermite_shard_f64.hip). Un-sharded, a
    third source array `s._accd` = {ax, ay, az, 0} and one workspace for every entry: 9 doubles per body and slab, where
    the inherited force and the diagnostics need at most 6. Sharded, 12-double rows {x_p, m, v_p, 0, a_p, 0}, 9 doubles per
    body and slab, the snap as a third output and the crackle as the fourth of a step."""

    def hermite_scratch(self, s):
        super().hermite_scratch(s)
        if not s._sharded:
            s._accd = direct.alloc_rows_f64(s.n, s.device)
            s._hws = direct.hermite6_workspace(max(s.n, 1), s.device)

    def _shard_scratch(self, s):
        _hermite_shard_scratch(s, direct.alloc_hermite6_rows_f64, direct.hermite6_shard_f64_workspace,
                               direct.HERMITE6_ROW, self.dtype, own_mass=True)

    _shard_force_outputs = 3        # a, j, s

    def _shard_predict(self, s, carried, acc=None):
        """carried None: a plain pack, with `acc` (or zeros) as the third quad pair."""
        if carried:
            direct.hermite6_shard_predict_f64(s.positions, s.velocities, s._mass_local, s._rows_local, *carried, dt=s.dt)
        else:
            direct.hermite6_shard_predict_f64(s.positions, s.velocities, s._mass_local, s._rows_local, acc=acc)

    def _shard_local(self, s):
        p = s.part
        direct.hermite6_shard_force_local_f64(s._rows_local, p.n_local, s.n, p.lo, self._scalars(s)[0], s._hws)

    def _shard_remote(self, s, carried, new, **step):
        p = s.part
        if carried:
            step.update(snap_in=carried[2], crackle_out=new[3])
        direct.hermite6_shard_force_remote_f64(s._rows_all, s.n, s._rows_local, p.n_local, p.lo, *self._scalars(s),
                                               *new[:3], s._hws, **step)

    # BlockHermite6Simulator (the 6th order of csrc/direct_hermite_block_f64.hip): 9 doubles per listed body and slab; the
    # initial levels are the inherited block_init_levels, from a and j
    block_workspace = staticmethod(direct.hblock6_workspace)

    def block_step(self, s, n_act: int):
        direct.hblock6_step_f64(s.positions, s.velocities, s.accelerations, s.jerks, s.snaps, s.crackles, s.masses,
                                s._ticks, s.levels, n_act, s.max_level, s.dt, s.eta, *self._scalars(s), s._sched,
                                s._posd, s._veld, s._accd, s._bws)

    block_order = 6
    split_row = direct.HBLOCK6_SPLIT_ROW

    def _block_predict(self, s):
        direct.hblock6_predict_f64(s.positions, s.velocities, s.accelerations, s.jerks, s.snaps, s.crackles, s.masses,
                                   s._ticks, s.levels, s.max_level, s.dt, s._sched, s._posd, s._veld, s._accd)

    def _block_state(self, s):
        return s.positions, s.velocities, s.accelerations, s.jerks, s.snaps, s.crackles

    def _block_rows_in(self, s):             # the crackle is formed, never read
        return self._block_state(s)[:5], (s._posd, s._veld, s._accd)


_FORMATS = {fmt.dtype: fmt for fmt in (_Float32(), _Float64())}
_HERMITE6 = _Hermite6Float64()


class BaseSimulator(_ChunkedRun):
    # What an integrator class states next to its step(): `_step_in_place()`, the same step on the static buffers of
    # `_carried` without rebinding anything (capturable); `_carried` itself when the step carries more than the
    # accelerations; and
    _posm_after_step = False        # step() leaves _posm at the post-step positions (else the energies repack first)
    _equal_mass_step = False        # the un-sharded step() has an equal-mass form (`_uniform`)
    _fmt = _FORMATS[torch.float32]  # the number format; the constructors choose it from `dtype`

    def __init__(self, *, positions, velocities, masses, g_const: float = 1.0, softening: float = 0.1,
                 dt: float = 0.01, calc_energy: bool = True, device: str = None, process_group=None,
                 calc_invariants: bool = False, **format_kw):
        # format_kw: `dtype` (default torch.float32), the one keyword of the number format, taken as BatchedSimulator
        # takes it; any other name is refused as an unknown keyword is.
        dtype = format_kw.pop("dtype", torch.float32)
        if format_kw:
            raise TypeError(f"{type(self).__name__}.__init__() got an unexpected keyword argument "
                            f"{next(iter(format_kw))!r}")
        self._check_format(dtype, process_group)         # before anything is resolved, allocated or launched
        self._fmt = _FORMATS[dtype]                      # the only place the format is chosen
        self._init_state(positions, velocities, masses, g_const, softening, dt, calc_energy, device, process_group,
                         calc_invariants)
        self._fmt._base_scratch(self)

    @classmethod
    def _check_format(cls, dtype, process_group):
        if dtype not in _FORMATS:
            raise ValueError(f"{cls.__name__}: dtype must be torch.float32 or torch.float64, got {dtype!r}")
        if process_group is not None and not _FORMATS[dtype].leapfrog_shardable:
            raise ValueError(f"{cls.__name__}: dtype={dtype} has no range-sharded form; process_group is not supported "
                             "with it")

    def _init_state(self, positions, velocities, masses, g_const, softening, dt, calc_energy, device, process_group,
                    calc_invariants):
        """Device, scalars, the state in the format's dtype and the partition: no scratch, no launch."""
        self.device = _resolve_device(device)
        _lib.lib()  # fail now, loudly, if the extension is not built

        self.dt = dt
        self.g_const = g_const
        self.softening = softening
        self.calc_energy = calc_energy
        self.calc_invariants = calc_invariants
        self._fmt.bind_scalars(self)

        full_pos, full_vel, self.masses = (_to_device(x, self.device, self._fmt.dtype)
                                           for x in (positions, velocities, masses))
        self.n = full_pos.shape[0]
        if full_pos.shape != (self.n, 3) or full_vel.shape != (self.n, 3) or self.masses.shape != (self.n,):
            raise ValueError("positions/velocities must be (n,3) and masses (n,)")

        world, rank = nbd_dist.group_info(process_group) if process_group is not None else (1, 0)
        self.process_group = process_group
        self.part = nbd_dist.RangePartition(self.n, world, rank)
        lo, hi = self.part.lo, self.part.hi
        # the range-sharded code path: more than one rank, or a one-rank group with NBD_FORCE_SHARDED=1 (rehearsal
        # of the RCCL calls, the asynchronous gather and the split force on a single GPU)
        self._sharded = world > 1 or (process_group is not None and os.environ.get("NBD_FORCE_SHARDED") == "1")
        self.positions = full_pos[lo:hi].clone() if self._sharded else full_pos
        self.velocities = full_vel[lo:hi].clone() if self._sharded else full_vel
        self.accelerations = None
        self._uniform = None

    def _init_scratch(self):
        """The fp32 scratch: packed sources (all ranks' bodies), slabs, energy partials; then the first force."""
        self._posm = direct.alloc_posm(self.n, self.device)
        self._posm.zero_()
        # equal masses (the published configurations): the force kernel without its per-pair mass multiply, the common
        # factor applied once to the finished sum -- in the fused leapfrog step and in both launches of the
        # range-sharded force. Checked here, once (the masses are replicated on every rank: all ranks decide alike);
        # NBD_UNIFORM_MASS=0 keeps the general kernel. The un-sharded Euler step and compute_accelerations() use the
        # general kernel.
        self._uniform = (direct.uniform_mass(self.masses)
                         if ((self._sharded or self._equal_mass_step)
                             and os.environ.get("NBD_UNIFORM_MASS", "1") != "0") else None)
        if not self._sharded:
            # sized for the step's preferred plan (the equal-mass symmetric force: one partial-sum slot per round of its
            # tile tournament, all rounds in one launch); NBD_SYM_SLOTS=16 keeps the 16-slot plan, as NBD_UNIFORM_MASS=0
            # keeps the general kernel
            self._ws = direct.step_workspace(max(self.n, 1), self.device)
            self._posm_local, self._mass_local, self._gather = self._posm, self.masses, None
        else:
            # the rank's own packed bodies: source of its local force block and send buffer of the gather
            # (max_count rows so that ragged shards send equal, zero-padded pieces)
            self._posm_local = direct.alloc_posm(self.part.max_count, self.device)
            self._posm_local.zero_()
            self._mass_local = self.masses[self.part.lo:self.part.hi].contiguous()
            self._ws = direct.shard_workspace(self.n, self.part.lo, self.part.n_local, self.device) \
                if self.part.n_local else None
            self._gather = nbd_dist.RowGather(self.part, 4, torch.float32, self.device, self.process_group,
                                              collective=True)

        self.accelerations = self.compute_accelerations()

    # ------------------------------------------------------------------ force
    def _pack_local(self):
        n_loc = self.part.n_local
        if n_loc:
            direct.pack_posm(self.positions, self._mass_local, out=self._posm_local[:direct.padded_len(n_loc)])

    def _force_sharded(self, vel=None, c_kick: float = 0.0, ev=None) -> torch.Tensor:
        """Force on the rank's bodies from `_posm_local` (already packed): start the all-gather, run the
        local x local block while it is in flight, then the remote block + slab sum (+ fused kick).
        `ev`: events recorded after the gather's start (ev[1]), the local block, the gather's end and the remote block."""
        def mark(i):
            if ev is not None:
                ev[i].record()
        p = self.part
        handle = self._gather.start(self._posm_local, self._posm)
        acc = torch.empty((p.n_local, 3), dtype=torch.float32, device=self.device)
        mark(1)
        if p.n_local:
            local = self._posm_local[:direct.padded_len(p.n_local)]
            direct.shard_force_local(local, p.n_local, self.n, p.lo, self._eps2, self._ws, uniform=self._uniform)
        mark(2)
        self._gather.finish(handle, self._posm)
        mark(3)
        if p.n_local:
            direct.shard_force_remote(self._posm, self.n, local, p.n_local, p.lo, self._eps2, self._g, acc,
                                      vel, c_kick, self._ws, uniform=self._uniform)
        mark(4)
        return acc

    def compute_accelerations(self) -> torch.Tensor:
        """a_i = G sum_{j!=i} m_j (r_j - r_i)/(|r_j - r_i|^2 + eps^2)^(3/2) -> new (n_local,3) tensor
        (simulation.py:71-89)."""
        if self.n == 0:
            return torch.zeros((0, 3), dtype=self._fmt.dtype, device=self.device)
        if self._wants_grad():
            return self._accelerations_with_grad()
        return self._fmt.accel(self)

    def _wants_grad(self) -> bool:
        return torch.is_grad_enabled() and (self.positions.requires_grad or self.masses.requires_grad)

    def _accelerations_with_grad(self) -> torch.Tensor:
        """compute_accelerations() as a node of torch's graph (nbd.autograd.direct_accel: the same forward bits, and a
        HIP backward with respect to positions and masses). The node packs its own copy of the state, so a later step()
        does not change what backward() differentiates."""
        self._refuse_sharded("compute_accelerations() with requires_grad")
        from nbd.autograd import direct_accel
        return direct_accel(self.positions, self.masses, self.g_const, self.softening)

    def compute_energies(self):
        """(U, K) as Python floats (simulation.py:91-115). Sharded: every rank evaluates the
        global sums from the gathered state (velocities are gathered for this call)."""
        if self.n == 0:
            return 0.0, 0.0
        self._fmt.pack(self)
        vel = self.gather("velocities") if self._sharded else self.velocities
        return tuple(self._fmt.energies(self, vel).cpu().tolist())

    # ------------------------------------------------------------------ consistent-potential diagnostics
    def _refuse_sharded(self, what: str):
        if self._sharded:
            raise ValueError(f"{type(self).__name__}.{what}: there are no range-sharded diagnostics; process_group is not "
                             "supported here")

    def _potentials_into(self, phi):
        """phi (n,) float64 from the packed sources (already packed), asynchronous."""
        return self._fmt.potentials(self, phi)

    def compute_potentials(self) -> torch.Tensor:
        """phi_i = -G sum_{j != i} m_j (|r_ij|^2 + eps^2)^(-1/2) -> new (n,) float64 device tensor: the potential the force
        of compute_accelerations() is the gradient of (pair terms in fp32, sums in fp64; csrc/direct_diag.hip). Coincident
        distinct bodies at softening 0 give -inf."""
        self._refuse_sharded("compute_potentials()")
        if self.n == 0:
            return torch.zeros((0,), dtype=torch.float64, device=self.device)
        self._fmt.pack(self)
        return self._potentials_into(None)

    def compute_invariants(self) -> Invariants:
        """Mass, centre of mass, momentum, angular momentum, K, U = 1/2 sum m phi, E = K + U and the virial ratio of the
        current state (see Invariants). compute_energies() is untouched: it keeps the reference's potential."""
        self._refuse_sharded("compute_invariants()")
        if self.n == 0:
            return Invariants.from_row([0.0] * direct.INVARIANT_ROW)
        phi = self.compute_potentials()
        return Invariants.from_row(self._fmt.invariants(self, phi).cpu())

    def _invariants_into(self, out_row):
        """Invariants row of the state AFTER an un-sharded step, asynchronous (phi into a buffer kept by the simulator)."""
        if getattr(self, "_phi", None) is None:
            self._phi = torch.empty((self.n,), dtype=torch.float64, device=self.device)
        if not self._posm_after_step:
            self._fmt.pack(self)
        self._potentials_into(self._phi)
        self._fmt.invariants(self, self._phi, out_row)

    def gather(self, name: str) -> torch.Tensor:
        """Global (n,3) copy of a sharded state array on every rank ('positions', ...)."""
        local = getattr(self, name)
        if not self._sharded:
            return local
        out = torch.empty((self.n, 3), dtype=local.dtype, device=self.device)
        return nbd_dist.allgather_rows(local, self.part, out, group=self.process_group)

    # ------------------------------------------------------------------ run loop
    def run(self, steps: int) -> list[SimulationState]:
        """Run `steps` steps and return one SimulationState per step (simulation.py:117-146):
        CPU clones of the state after the step, the step's time and (if calc_energy) U and K.
        step_time is the GPU time of step() from HIP events (the reference's un-synchronised
        time.time() bracket would only time the launches)."""
        states = []
        if steps <= 0:
            return states
        if self.calc_invariants:
            self._refuse_sharded("run() with calc_invariants")
        if self._graph_run_ok(steps):
            self._run_chunked(steps, self.GRAPH_RUN_CHUNK, states)
        else:
            self._run_eager(steps, 0, states)
        return states

    def _energies_into(self, out_uk, workspace=None):
        """Energies of the state AFTER an un-sharded step (simulation.py:131-133), asynchronous."""
        if not self._posm_after_step:
            self._fmt.pack(self)
        self._fmt.energies(self, self.velocities, out_uk, workspace)

    def _run_eager(self, steps: int, first_index: int, states):
        n_loc = self.part.n_local
        dtype = self.positions.dtype                     # float32, or float64 for HermiteSimulator(dtype=torch.float64)
        per_step = 3 * n_loc * 3 * self.positions.element_size()
        chunk = max(1, min(max(steps, 32), (64 << 20) // max(per_step, 1)))
        # pinned staging is expensive to create (page-locking): keep it across run() calls
        cached = getattr(self, "_run_stage", None)
        if cached is None or cached[0].shape[0] < chunk:
            cached = (torch.empty((chunk, 3, n_loc, 3), dtype=dtype).pin_memory(),
                      torch.empty((chunk, 2), dtype=torch.float64).pin_memory())
            self._run_stage = cached
        stage, uk_host = cached
        chunk = stage.shape[0]
        uk_dev = torch.zeros((chunk, 2), dtype=torch.float64, device=self.device)
        inv_dev = (torch.zeros((chunk, direct.INVARIANT_ROW), dtype=torch.float64, device=self.device)
                   if self.calc_invariants else None)
        done = 0
        while done < steps:
            m = min(chunk, steps - done)
            events = []
            for s in range(m):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                self.step()
                e1.record()
                events.append((e0, e1))
                if self.calc_energy:
                    if not self._sharded:
                        self._energies_into(uk_dev[s])
                    else:
                        u, k = self.compute_energies()
                        uk_dev[s, 0], uk_dev[s, 1] = u, k
                if self.calc_invariants and self.n:
                    self._invariants_into(inv_dev[s])
                stage[s, 0].copy_(self.positions, non_blocking=True)
                stage[s, 1].copy_(self.velocities, non_blocking=True)
                stage[s, 2].copy_(self.accelerations, non_blocking=True)
            uk_host[:m].copy_(uk_dev[:m], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            # one pageable copy of the whole chunk (the pinned staging is reused); the states' tensors are
            # views into it -- 3 m small clones cost several times more in allocation and page faults
            host = [stage[:m].clone()] + ([uk_host[:m]] if self.calc_energy else []) + \
                ([inv_dev[:m].cpu()] if self.calc_invariants else [])
            self._emit_states(host, m, first_index + done, [e0.elapsed_time(e1) * 1e-3 for e0, e1 in events], states)
            done += m

    def _emit_states(self, host, m, first, t_steps, states):
        """m states from host copies of a chunk's ring (m, 3, n, 3), then (with calc_energy) its energies (m, 2), then
        (with calc_invariants) its invariant rows (m, 16): views, no copies."""
        rest = iter(host[1:])
        ring = host[0]
        uk = next(rest).tolist() if self.calc_energy else None
        inv = next(rest).tolist() if self.calc_invariants else None
        for s in range(m):
            u, k = (uk[s][0], uk[s][1]) if self.calc_energy else (None, None)
            states.append(SimulationState(step=first + s, step_time=t_steps[s], positions=ring[s, 0],
                                          velocities=ring[s, 1], accelerations=ring[s, 2], u_energy=u, k_energy=k,
                                          invariants=Invariants.from_row(inv[s]) if inv is not None else None))

    # ------------------------------------------------------------------ run(): captured chunks (_ChunkedRun)
    GRAPH_RUN_MAX_BODIES = 16384

    @classmethod
    def _capturable(cls) -> bool:
        """The class that defines step() also defines _step_in_place(): an overriding step() is never replaced by an
        inherited in-place step, it runs eagerly."""
        owner = next(k for k in cls.__mro__ if "step" in vars(k))
        return "_step_in_place" in vars(owner)

    def _graph_run_ok(self, steps: int) -> bool:
        return (self._fmt.capturable and not self._sharded and 0 < self.n <= self.GRAPH_RUN_MAX_BODIES and steps >= 8 and
                self._capturable() and os.environ.get("NBD_RUN_GRAPH", "1") != "0")

    def _chunk_scalars(self):
        return (float(self.dt), float(self.softening), bool(self.calc_energy), self._eps2, self._g, self._uniform,
                bool(self.calc_invariants))

    def _chunk_body(self, m: int):
        n, dev = self.n, self.device
        if getattr(self, "_energy_ws", None) is None:
            self._energy_ws = direct.alloc_bytes(_lib.lib().nbd_energy_workspace_bytes(n), dev)
        ring = torch.empty((m, 3, n, 3), dtype=torch.float32, device=dev)
        uk = torch.zeros((m, 2), dtype=torch.float64, device=dev)
        inv = torch.zeros((m, direct.INVARIANT_ROW), dtype=torch.float64, device=dev) if self.calc_invariants else None

        def body(count):
            for s_ in range(count):
                self._step_in_place()
                if self.calc_energy:
                    self._energies_into(uk[s_], self._energy_ws)
                if self.calc_invariants:
                    self._invariants_into(inv[s_])
                direct.snapshot(self.positions, self.velocities, self._acc_g, ring[s_])
        return body, (ring,) + ((uk,) if self.calc_energy else ()) + ((inv,) if self.calc_invariants else ())

    def step(self):
        raise NotImplementedError("El método step debe ser implementado en la subclase")


class LeapFrogSimulator(BaseSimulator):
    """The reference's kick-drift-kick integrator. With `dtype=torch.float64` (csrc/direct_leapfrog_f64.hip; DESIGN.md
    K-L64) positions, velocities, masses and accelerations are float64 device tensors (the inputs are converted directly,
    not through float32), g_const, softening ** 2, dt and dt / 2 go to the kernels as the Python doubles, and step(), the
    compute_*() methods and run() are float64 end to end; run() is eager and there is no range-sharded form in this mode."""

    def step(self):
        """Kick-drift-kick (simulation.py:153-170); one force evaluation per step; positions and
        velocities are updated in place, `accelerations` is rebound to a new tensor (:168)."""
        if self.n == 0:
            return
        if not self._sharded:
            new_acc = torch.empty_like(self.accelerations)
            self._fmt._leapfrog_step(self, self.accelerations, new_acc)
            self.accelerations = new_acc
            return
        half = direct.f32(0.5 * self.dt)
        dt = direct.f32(self.dt)
        # sharded: kick+drift+pack of the own bodies -> all-gather in flight || own x own force block ->
        # own x remote block + slab sum + second kick. Four launches and one collective.
        if self._step_graph is not None:                 # capture_step(): the same launches and the collective, replayed
            self._step_graph.replay()
            return
        self.accelerations = self._sharded_launches(self.accelerations, half, dt)

    _posm_after_step = True
    _equal_mass_step = True

    def _step_in_place(self):
        self._fmt._leapfrog_step(self, self._acc_g, self._acc_g)

    def _sharded_launches(self, acc, half, dt, ev=None) -> torch.Tensor:
        """The range-sharded step's launches from the accelerations `acc`; returns the new ones. `ev`: five events, ev[0]
        recorded before the kick-drift and the others between the phases of _force_sharded()."""
        if ev is not None:
            ev[0].record()
        if self.part.n_local:
            direct.kick_drift(self.positions, self.velocities, acc, self._mass_local, half, dt, posm=self._posm_local)
        return self._force_sharded(self.velocities, half, ev)

    _step_graph = None

    def capture_step(self, warmup: int = 3) -> bool:
        """Capture the range-sharded leapfrog step -- kick-drift, the all-gather, both force blocks, the second kick -- into
        ONE hipGraph (torch's NCCL backend = RCCL records its collective into a capturing stream): a rank's step at the
        strong-scaled size is ~136 us of kernels behind ~28 us of host enqueue (profiles/r02_shard_rank_of_8.json), and the
        enqueue is what a replay removes. `accelerations` becomes a static buffer (the graph copies the new values into
        it: 12 B per body). Returns False -- and step() stays eager -- when the runtime refuses the capture; every rank
        must call this together (the warm-up steps run the collective)."""
        if not self._sharded or self.n == 0 or self._step_graph is not None:
            return self._step_graph is not None
        try:
            for _ in range(warmup):                      # communicator, allocator pools, hipFuncSetAttribute calls
                self.step()
            torch.cuda.synchronize(self.device)
            half, dt = direct.f32(0.5 * self.dt), direct.f32(self.dt)
            acc_static = self.accelerations.clone()
            self.accelerations = acc_static
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(graph, stream=side):
                    new_acc = self._sharded_launches(acc_static, half, dt)
                    acc_static.copy_(new_acc)
            torch.cuda.current_stream(self.device).wait_stream(side)
            torch.cuda.synchronize(self.device)
            self._step_graph, self._step_graph_keep = graph, (new_acc, acc_static, side)
            return True
        except Exception as exc:                          # pragma: no cover - depends on the runtime's capture support
            import warnings
            warnings.warn(f"hipGraph capture of the range-sharded step failed ({exc}); the step stays eager")
            try:
                torch.cuda.synchronize(self.device)
            except Exception:
                pass
            self._step_graph = None
            return False

    def step_phases(self):
        """One EAGER range-sharded step with HIP events between its phases: {"local_force_ms", "gather_wait_ms",
        "remote_force_ms", "kick_drift_ms", "host_enqueue_ms"} -- gather_wait = the launch stream idle between the end of
        the own x own block and the completion of the all-gather (what the overlap does not cover). Synchronises."""
        if not self._sharded or self.n == 0:
            raise _lib.NbdError("step_phases(): only the range-sharded step has phases")
        half, dt = direct.f32(0.5 * self.dt), direct.f32(self.dt)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        t0 = time.perf_counter()
        acc = self._sharded_launches(self.accelerations, half, dt, ev)
        host = (time.perf_counter() - t0) * 1e3
        if self._step_graph is not None:
            self.accelerations.copy_(acc)                # the captured step's static buffer
        else:
            self.accelerations = acc
        torch.cuda.synchronize(self.device)
        return {"kick_drift_ms": ev[0].elapsed_time(ev[1]), "local_force_ms": ev[1].elapsed_time(ev[2]),
                "gather_wait_ms": ev[2].elapsed_time(ev[3]), "remote_force_ms": ev[3].elapsed_time(ev[4]),
                "host_enqueue_ms": host}


class TreeLeapFrogSimulator(LeapFrogSimulator):
    """LeapFrogSimulator with a Barnes-Hut force in place of the all-pairs sum (csrc/tree_force.hip):
    O(N log N) per step, for softened collisionless systems where a relative force error of ~1e-3 is below the
    discreteness noise. `theta` is the opening angle (0.5; 0 opens every node and is the direct sum in tree order),
    `quadrupole` keeps the cells' quadrupole term (True). float32 only, no gradients: `dtype=torch.float64` and inputs
    that require grad are refused.

    positions, velocities and accelerations stay in the caller's order; the bodies are re-sorted along a Morton curve
    and the tree rebuilt inside every force evaluation (`tree_order()` is that permutation, `tree_counters()` the walk's
    work). step() is kick-drift, sort + build, tree force, kick; run() is eager.

    `potential` chooses what compute_potentials(), compute_invariants() and run() with calc_invariants=True sum:
      "direct" (the default)  the all-pairs O(N^2) potential of LeapFrogSimulator, bit for bit;
      "tree"                  the tree's own potential, O(N log N): over the accepted cells and rejected level-0 nodes
                              of the force walk, phi_cell = -(M u + 1/2 (r.Qr) u^5) and -m_j (|d|^2 + eps^2)^(-1/2) per
                              body (fp32 terms, fp64 sums) -- the function whose gradient the tree force is, so
                              E = K + 1/2 sum m phi is the figure of merit of this integrator. compute_potentials()
                              sorts and builds on the current positions and walks for phi alone; while calc_invariants
                              is True, step() takes a and phi from ONE walk and the invariants row of run() uses that
                              phi: no second build, no second walk. a and tree_counters() are the plain step's.
    compute_energies() and calc_energy keep the reference's all-pairs -G m m / (|r| + eps) kernel under either value:
    that number has to be the reference's, and its pair term is not the one the cell records expand. It is O(N^2):
    construct large systems with calc_energy=False.

    `process_group` ("Several ranks"): a rank owns the bodies of its RangePartition of the caller's order,
    as in every sharded simulator here, and walks the target groups (64 consecutive bodies of the Morton order) of a
    second RangePartition over the ceil(n/64) groups. The step is kick-drift of the own bodies, the all-gather of the
    packed rows, sort + build of the WHOLE tree on every rank, the walk of the rank's groups, one all-gather of the
    finished rows in tree order (two with phi) and a scatter of the own bodies' rows: the results are bit for bit those
    of one GPU, whatever the number of ranks. compute_accelerations(), compute_potentials() and compute_invariants()
    (potential="tree") and compute_energies() are collective; compute_potentials() returns the rank's (n_local,) phi,
    compute_invariants() the global row on every rank, tree_order() the global order, tree_counters() the rank's own
    walk. potential="direct" diagnostics and run() with calc_invariants stay refused as for every sharded simulator;
    capture_step() returns False (the step stays eager)."""

    def __init__(self, *, theta: float = 0.5, quadrupole: bool = True, potential: str = "direct", **kw):
        name = type(self).__name__
        if potential not in ("direct", "tree"):
            raise ValueError(f"{name}: potential must be 'direct' or 'tree', got {potential!r}")
        if kw.get("dtype", torch.float32) != torch.float32:
            raise ValueError(f"{name}: the tree force is float32 only, got dtype={kw['dtype']!r}")
        group = kw.get("process_group")                  # checked here: before a device is resolved
        if group is not None and not (torch.distributed.is_available()
                                      and isinstance(group, torch.distributed.ProcessGroup)):
            raise ValueError(f"{name}: process_group must be a torch.distributed.ProcessGroup, got {group!r}")
        for key in ("positions", "velocities", "masses"):
            if isinstance(kw.get(key), torch.Tensor) and kw[key].requires_grad:
                raise ValueError(f"{name}: the tree force has no backward; {key} requires grad")
        if not float(theta) >= 0.0:
            raise ValueError(f"{name}: theta must be >= 0, got {theta!r}")
        self.theta = float(theta)
        self.quadrupole = bool(quadrupole)
        self.potential = potential
        super().__init__(**kw)

    def _init_scratch(self):
        """The packed sources the energy kernels read, the tree's workspace and outputs; then the first force. (None of
        the all-pairs step's slabs: they are 16 n rows and this class never launches that step.)"""
        from nbd import tree
        self._posm = direct.alloc_posm(self.n, self.device)
        self._posm.zero_()
        self._uniform, self._ws, self._gather = None, None, None
        self._posm_local, self._mass_local = self._posm, self.masses
        self._tree_ws = tree.workspace(self.n, self.device) if self.n else None
        self._order = torch.empty((self.n,), dtype=torch.int32, device=self.device)
        self._counters = torch.zeros((2,), dtype=torch.int64, device=self.device)
        self._phi, self._phi_of_step = None, False       # phi of the last step's walk (potential="tree")
        if self._sharded:
            self._init_shard_scratch()
        self.accelerations = self.compute_accelerations()

    def _init_shard_scratch(self):
        """Several ranks: the rank's packed bodies and their gather (as BaseSimulator's), the partition of the target
        groups, and per exchanged quantity a send buffer of the rank's groups and the array of all groups, both in tree
        order, with the RowGather that moves one row per GROUP (192 floats of a, 64 doubles of phi) between them."""
        from nbd import tree
        p, dev = self.part, self.device
        self._posm_local = direct.alloc_posm(p.max_count, dev)
        self._posm_local.zero_()
        self._mass_local = self.masses[p.lo:p.hi].contiguous()
        self._gather = nbd_dist.RowGather(p, 4, torch.float32, dev, self.process_group, collective=True)
        g = self._gpart = nbd_dist.RangePartition(tree.groups(self.n), p.world_size, p.rank)
        self._acc_send = torch.zeros((g.max_count * tree.GROUP, 3), dtype=torch.float32, device=dev)
        self._acc_sorted = torch.zeros((g.n * tree.GROUP, 3), dtype=torch.float32, device=dev)
        self._acc_gather = nbd_dist.RowGather(g, 3 * tree.GROUP, torch.float32, dev, self.process_group, collective=True)
        self._phi_send = self._phi_sorted = self._phi_gather = None      # made by the first walk that sums phi

    def _phi_exchange(self):
        from nbd import tree
        if self._phi_gather is None:
            g, dev = self._gpart, self.device
            self._phi_send = torch.zeros((g.max_count * tree.GROUP,), dtype=torch.float64, device=dev)
            self._phi_sorted = torch.zeros((g.n * tree.GROUP,), dtype=torch.float64, device=dev)
            self._phi_gather = nbd_dist.RowGather(g, tree.GROUP, torch.float64, dev, self.process_group, collective=True)
        return self._phi_gather

    def _exchange_groups(self, gather, send, out, cols):
        """One all-gather of the rank's group rows `send` into `out` (all groups, tree order)."""
        g = self._gpart
        send, out = send.view(g.max_count, cols), out.view(g.n, cols)
        gather.finish(gather.start(send, out), out)

    def _sharded_walk(self, acc: bool, phi: bool, lo: int, hi: int, ev=None) -> tuple:
        """Several ranks, `_posm_local` already packed: all-gather of the packed rows, sort + build of the whole tree,
        the walk of the rank's groups for a, phi or both (the fused walk), one all-gather per quantity of the finished
        rows in tree order, and their scatter to the bodies [lo, hi) of the caller's order -> (acc or None, phi or None).
        `ev`: events recorded after the gather's start (ev[1]), its end, the build, the walk and the scatter."""
        from nbd import tree
        def mark(i):
            if ev is not None:
                ev[i].record()
        n, g, ws = self.n, self._gpart, self._tree_ws
        handle = self._gather.start(self._posm_local, self._posm)
        mark(1)
        self._gather.finish(handle, self._posm)
        mark(2)
        tree.build_posm(self._posm, n, ws, self._order)
        mark(3)
        rows = g.n_local * tree.GROUP
        if phi:
            self._phi_exchange()
        tree.walk(ws, n, self.theta, self._eps2, self._g, self.quadrupole, acc=acc, phi=phi, groups=(g.lo, g.hi),
                  out=(self._acc_send[:rows] if acc else None, self._phi_send[:rows] if phi else None),
                  counters=self._counters if acc else None)          # (phi alone: they keep the last FORCE walk's)
        mark(4)
        if acc:
            self._exchange_groups(self._acc_gather, self._acc_send, self._acc_sorted, 3 * tree.GROUP)
        if phi:
            self._exchange_groups(self._phi_gather, self._phi_send, self._phi_sorted, tree.GROUP)
        out = tree.scatter(ws, n, lo, hi, self._acc_sorted if acc else None, self._phi_sorted if phi else None)
        mark(5)
        return out

    def compute_accelerations(self) -> torch.Tensor:
        """The tree force on the current positions -> new (n_local,3) tensor in the caller's order (collective when
        sharded)."""
        return self._tree_force(None)

    def _tree_force(self, phi) -> torch.Tensor:
        """Sort + build, then the walk: for a alone, or (phi: (n,) float64) the fused one that also leaves phi there."""
        if self.n == 0:
            return torch.zeros((0, 3), dtype=torch.float32, device=self.device)
        if self._wants_grad():
            raise ValueError(f"{type(self).__name__}.compute_accelerations(): the tree force has no backward")
        from nbd import tree
        if self._sharded:                                # (only for a: the sharded step() walks by itself)
            self._pack_local()
            return self._sharded_walk(True, False, self.part.lo, self.part.hi)[0]
        tree.build(self.positions, self.masses, self._tree_ws, self._order)
        return tree.walk(self._tree_ws, self.n, self.theta, self._eps2, self._g, self.quadrupole, phi=phi is not None,
                         out=(None, phi), counters=self._counters)[0]

    def _phi_buffer(self) -> torch.Tensor:
        """(n,) float64 for the phi a step's own walk leaves, made by the first step that wants it."""
        if self._phi is None:
            self._phi = torch.empty((self.n,), dtype=torch.float64, device=self.device)
        return self._phi

    def compute_potentials(self) -> torch.Tensor:
        """potential="direct": LeapFrogSimulator.compute_potentials(). potential="tree": sort + build on the current
        positions, then the phi-only walk -> new (n,) float64 device tensor (coincident distinct bodies at softening 0
        give -inf here too). tree_counters() keeps the last FORCE evaluation's figures."""
        if self.potential != "tree":
            return super().compute_potentials()
        if self.n == 0:
            return torch.zeros((0,), dtype=torch.float64, device=self.device)
        if self._sharded:                                # collective; the rank's own (n_local,) rows
            return self._potentials_sharded(self.part.lo, self.part.hi)
        from nbd import tree
        self._fmt.pack(self)                             # compute_invariants() reads the packed bodies next to phi
        tree.build(self.positions, self.masses, self._tree_ws, self._order)
        return tree.walk(self._tree_ws, self.n, self.theta, self._eps2, self._g, self.quadrupole, acc=False, phi=True)[1]

    def _potentials_sharded(self, lo: int, hi: int) -> torch.Tensor:
        """phi of the bodies [lo, hi) of the caller's order from the phi-only walk of the rank's groups; `_posm` is left
        at the current positions of all bodies."""
        self._pack_local()
        return self._sharded_walk(False, True, lo, hi)[1]

    def compute_invariants(self) -> Invariants:
        """As BaseSimulator.compute_invariants(). Sharded with potential="tree": collective, the global row on every rank
        (phi of all bodies from the exchanged tree-order rows, the velocities gathered for this call)."""
        if not self._sharded or self.potential != "tree":
            return super().compute_invariants()
        if self.n == 0:
            return Invariants.from_row([0.0] * direct.INVARIANT_ROW)
        phi = self._potentials_sharded(0, self.n)
        vel = self.gather("velocities")
        return Invariants.from_row(direct.invariants(self._posm, vel, phi, self.n).cpu())

    def _invariants_into(self, out_row):
        """potential="tree": the row from the phi the step's own walk left (step() packed `_posm` in its kick-drift)."""
        if self.potential != "tree" or not self._phi_of_step:
            return super()._invariants_into(out_row)
        self._fmt.invariants(self, self._phi, out_row)

    def _potentials_into(self, phi):
        if self.potential != "tree":
            return super()._potentials_into(phi)
        return phi.copy_(self.compute_potentials())      # (only a row asked for without a fused step before it)

    def tree_order(self) -> torch.Tensor:
        """order (n,) int32 of the last force evaluation: order[k] is the index of the k-th body along the Morton curve."""
        return self._order.clone()

    def tree_counters(self) -> tuple:
        """(accepted cells, rejected level-0 nodes) of the last force evaluation, summed over the target groups."""
        if self.n == 0:
            return 0, 0
        c = self._counters.cpu().tolist()
        return int(c[0]), int(c[1])

    def step(self):
        """Kick-drift (the direct integrator's kernel), sort + build, tree force, kick. With potential="tree" and
        calc_invariants the force walk is the fused one and leaves phi of the new positions for the invariants."""
        if self.n == 0:
            return
        if self._sharded:
            self._sharded_step()
            return
        half, dt = direct.f32(0.5 * self.dt), direct.f32(self.dt)
        direct.kick_drift(self.positions, self.velocities, self.accelerations, self.masses, half, dt, posm=self._posm)
        self._phi_of_step = self.potential == "tree" and bool(self.calc_invariants)
        self.accelerations = self._tree_force(self._phi_buffer() if self._phi_of_step else None)
        direct.kick(self.velocities, self.accelerations, half)

    def _sharded_step(self, ev=None):
        """The step on several ranks: kick-drift of the own bodies into `_posm_local`, `_sharded_walk` (the fused one with
        potential="tree" and calc_invariants: `_phi` is then the rank's (n_local,) phi of the new positions), kick. Two
        collectives (three with phi). `ev`: six events, ev[0] before the kick-drift, the others as `_sharded_walk`."""
        p = self.part
        half, dt = direct.f32(0.5 * self.dt), direct.f32(self.dt)
        if ev is not None:
            ev[0].record()
        if p.n_local:
            direct.kick_drift(self.positions, self.velocities, self.accelerations, self._mass_local, half, dt,
                              posm=self._posm_local)
        self._phi_of_step = self.potential == "tree" and bool(self.calc_invariants)
        self.accelerations, phi = self._sharded_walk(True, self._phi_of_step, p.lo, p.hi, ev)
        if self._phi_of_step:
            self._phi = phi
        if p.n_local:
            direct.kick(self.velocities, self.accelerations, half)

    def capture_step(self, warmup: int = 3) -> bool:
        """False, and nothing is captured: the tree step stays eager, alone or sharded (out of scope)."""
        return False

    def step_phases(self):
        """One EAGER sharded step with HIP events between its phases: {"kick_drift_ms", "gather_wait_ms" (the all-gather
        of the packed rows: nothing overlaps it), "build_ms", "walk_ms", "exchange_ms" (the all-gathers of the finished
        rows and the scatter), "host_enqueue_ms"}. Synchronises; collective."""
        if not self._sharded or self.n == 0:
            raise _lib.NbdError("step_phases(): only the range-sharded step has phases")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        t0 = time.perf_counter()
        self._sharded_step(ev)
        host = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize(self.device)
        return {"kick_drift_ms": ev[0].elapsed_time(ev[1]), "gather_wait_ms": ev[1].elapsed_time(ev[2]),
                "build_ms": ev[2].elapsed_time(ev[3]), "walk_ms": ev[3].elapsed_time(ev[4]),
                "exchange_ms": ev[4].elapsed_time(ev[5]), "host_enqueue_ms": host}


class BlockTreeLeapFrogSimulator(TreeLeapFrogSimulator):
    """TreeLeapFrogSimulator with individual block timesteps: a hierarchical kick-drift-kick with power-of-two steps, as in
    GADGET-2 (csrc/tree_block.hip, the listed-target walk of csrc/tree_force.hip; DESIGN.md K-T, "Block timesteps"), an
    extension the reference does not have. `dt` is the output interval and the longest step: one step() advances every
    body by dt, in 2^max_level ticks. Body i moves with its own step h_i = dt 2^-k_i, k_i = levels[i] in [0, max_level],
    from the criterion of softened collisionless runs, h_i <= sqrt(2 eta softening / |a_i|) (the level may deepen at any
    block step and rises by one where the block allows). step() gives every body the opening kick of its step and then
    runs block steps: ALL bodies drift to the next due time (a compensated fp32 sum: within an interval a position takes
    one rounding however many block steps drift it), the tree is sorted and rebuilt on all of them, the force is
    walked for the due bodies alone (target groups of 64 due bodies in tree order), and those get the closing kick, a
    new level and the opening kick of their next step. At the end of the interval every body is due and the state is
    synchronised, so run() keeps returning one state per dt, compute_*() are TreeLeapFrogSimulator's, and with
    potential="tree" and calc_invariants the invariants row still comes from the phi of the step's own last walk.
    Initial levels (at construction, and after dt, eta, softening or max_level change) come from the same criterion.

    Counters (cumulative Python ints): `block_steps`, `active_targets` (the sum of n_act) and `clamped` (levels the
    criterion wanted deeper than max_level, NaN criteria included). `levels` is int32 on the device; setting
    `level_history` to a list records a CPU copy of it after every block step. `accelerations` is updated in place.
    tree_order() and tree_counters() are those of the last force evaluation. Eager-only: every block step reads
    {t_next, n_act} back to the host; capture_step() returns False. With max_level=0 it is TreeLeapFrogSimulator bit for
    bit. float32 only, no process_group, softening > 0 (the criterion needs it): each refusal is a ValueError before a
    device is resolved."""

    MAX_LEVEL_LIMIT = 20

    def __init__(self, *, eta: float = 0.025, max_level: int = 10, **kw):
        name = type(self).__name__
        self.eta, self.max_level = eta, max_level
        self.dt, self.softening = kw.get("dt", 0.01), kw.get("softening", 0.1)
        self._check_block_params()
        if kw.get("process_group") is not None:
            raise ValueError(f"{name}: there is no range-sharded block step; process_group is not supported")
        self.levels = None
        self.block_steps = self.active_targets = self.clamped = 0
        self.level_history = None
        super().__init__(**kw)

    def _check_block_params(self):
        name = type(self).__name__
        if not (type(self.max_level) is int and 0 <= self.max_level <= self.MAX_LEVEL_LIMIT):
            raise ValueError(f"{name}: max_level must be an int in [0, {self.MAX_LEVEL_LIMIT}], got {self.max_level!r}")
        if not (self.eta > 0 and self.dt > 0):
            raise ValueError(f"{name}: dt and eta must be positive, got dt={self.dt!r}, eta={self.eta!r}")
        if not self.softening > 0:
            raise ValueError(f"{name}: the step criterion needs softening > 0, got {self.softening!r}")

    def _init_scratch(self):
        from nbd import tree
        super()._init_scratch()                          # (ends with the construction-time force)
        n, dev = self.n, self.device
        self.levels = torch.zeros(n, dtype=torch.int32, device=dev)
        self._ticks = torch.zeros(n, dtype=torch.int32, device=dev)
        self._flags = torch.zeros(n, dtype=torch.int32, device=dev)
        self._sched = torch.zeros(tree.BLOCK_SCHED_INTS, dtype=torch.int32, device=dev)
        self._sched_host = torch.zeros(tree.BLOCK_SCHED_INTS, dtype=torch.int32).pin_memory()
        self._act_ws = tree.active_workspace(n, dev) if n else None
        self._act_list = torch.zeros(n, dtype=torch.int32, device=dev)
        self._residual = torch.zeros((n, 3), dtype=torch.float32, device=dev)      # the drift's rounding, per interval
        self._leveled_for = None
        self._set_levels()

    def _set_levels(self):
        from nbd import tree
        self._check_block_params()
        self._leveled_for = (self.dt, self.eta, self.softening, self.max_level)
        if self.n == 0:
            return
        tree.block_init_levels(self.accelerations, self.dt, self.eta, self.softening, self.max_level, self._ticks,
                               self.levels, self._sched)
        self._sched_host.copy_(self._sched)
        self.clamped = int(self._sched_host[2])

    def step(self):
        """One output interval: the opening kick of every body, then block steps until every body is back at tick
        2^max_level (at most 2^max_level of them)."""
        if self.n == 0:
            return
        if self._leveled_for != (self.dt, self.eta, self.softening, self.max_level):
            self._set_levels()
        from nbd import tree
        who = type(self).__name__
        n, K, ws, host = self.n, self.max_level, self._tree_ws, self._sched_host
        end, t_prev = 1 << K, 0
        walk = (self.theta, self._eps2, self._g, self.quadrupole)
        want_phi = self.potential == "tree" and bool(self.calc_invariants)
        self._phi_of_step = False
        tree.block_open(self.velocities, self.accelerations, self.levels, self._ticks, self._residual, K, self.dt,
                        self._sched)
        for _ in range(end):
            tree.block_drift(self.positions, self.velocities, self.masses, self.levels, self._ticks, self._residual, K,
                             self.dt, self._sched, self._posm)
            tree.build_posm(self._posm, n, ws, self._order)
            tree.block_flag(self.levels, self._ticks, K, self._sched, self._flags)
            tree.select_active(ws, n, self._flags, self._act_list, active_ws=self._act_ws, n_act_out=self._sched[1:2])
            host.copy_(self._sched)                      # the one readback of a block step
            t_next, n_act = int(host[0]), int(host[1])
            if not (t_prev < t_next <= end and 1 <= n_act <= n):
                raise RuntimeError(f"{who}: corrupt schedule (t_next={t_next}, n_act={n_act}, previous tick {t_prev})")
            # the interval's last walk, of every body, leaves phi for the invariants
            fused = want_phi and t_next == end and n_act == n
            tree.walk(ws, n, *walk, phi=fused, active=(self._act_list, n_act) if n_act < n else None,
                      out=(self.accelerations, self._phi_buffer() if fused else None), counters=self._counters)
            self._phi_of_step = fused
            tree.block_close(self.velocities, self.accelerations, self._flags, self.levels, self._ticks, K, self.dt,
                             self.eta, self.softening, self._sched)
            self.block_steps += 1
            self.active_targets += n_act
            if self.level_history is not None:
                self.level_history.append(self.levels.cpu())
            if t_next == end:
                break
            t_prev = t_next
        else:
            raise RuntimeError(f"{who}: interval not finished within {end} block steps")
        host.copy_(self._sched)
        self.clamped = int(host[2])


class EulerSimulator(BaseSimulator):
    """The reference's Euler integrator; `dtype=torch.float64` as in LeapFrogSimulator."""

    def step(self):
        """a(t) -> v += dt a -> x += dt v (simulation.py:173-187)."""
        if self.n == 0:
            return
        if not self._sharded:
            new_acc = torch.empty_like(self.accelerations)
            self._fmt._euler_step(self, new_acc)
            self.accelerations = new_acc
            return
        dt = direct.f32(self.dt)
        self._pack_local()
        self.accelerations = self._force_sharded(self.velocities, dt)        # a(t), v += dt a fused
        if self.part.n_local:
            direct.drift(self.positions, self.velocities, dt)

    def _step_in_place(self):           # (packs _posm before its drift: _posm_after_step stays False)
        self._fmt._euler_step(self, self._acc_g)


class HermiteSimulator(BaseSimulator):
    """Shared-timestep 4th-order Hermite predictor-corrector (Makino & Aarseth 1992), an extension the reference does not
    have. With a0, j0 the acceleration and jerk carried from the previous step:
        predict  x_p = x + v dt + a0 dt^2/2 + j0 dt^3/6,  v_p = v + a0 dt + j0 dt^2/2
        evaluate a1, j1 at (x_p, v_p)
        correct  v1 = v + (a0 + a1) dt/2 + (j0 - j1) dt^2/12,  x1 = x + (v + v1) dt/2 + (a0 - a1) dt^2/12
    One acceleration + jerk evaluation per step (csrc/direct_hermite.hip), fp32 state. `jerks` (n,3) is public next to
    `accelerations`; both hold the values evaluated at the last predicted state (PEC) and are rebound by step(). No
    equal-mass specialisation.

    With `process_group=` the bodies are range-sharded as for LeapFrogSimulator (csrc/direct_hermite_shard.hip; DESIGN.md
    §8): positions, velocities, accelerations and jerks hold the rank's rows [lo, hi), `gather()` assembles any of them,
    and a step is predict + pack of the own bodies -> ONE all-gather of 8-float rows {x_p, m, v_p, 0} in flight || own x
    own block -> own x others block + slab sum + corrector. Eager only: there is no captured form of the sharded step.

    With `dtype=torch.float64` (csrc/direct_hermite_f64.hip) positions, velocities, masses,
    accelerations and jerks are float64 device tensors (the inputs are converted directly, not through float32), g_const,
    softening ** 2, dt and the step constants go to the kernels as the Python doubles, and step(), the compute_*() methods
    and run() -- its states, energies and invariants -- are float64 end to end: there is no fp32 pair term anywhere.
    run() is eager in this mode. With `process_group=` as well (csrc/direct_hermite_shard_f64.hip) the
    sharded step above runs in float64: the exchanged rows are 8 doubles, still ONE all-gather per step, and
    compute_energies() gathers the float64 state on every rank."""

    _f64 = property(lambda self: self._fmt.dtype == torch.float64)       # read-only: tests and tools read it

    @staticmethod
    def _check_dtype(dtype, process_group):
        if dtype not in _FORMATS:
            raise ValueError(f"HermiteSimulator: dtype must be torch.float32 or torch.float64, got {dtype!r}")
        if process_group is not None and not _FORMATS[dtype].shardable:
            raise ValueError(f"HermiteSimulator: dtype={dtype} has no range-sharded form; process_group is not "
                             "supported with it")

    def __init__(self, *, positions, velocities, masses, g_const: float = 1.0, softening: float = 0.1,
                 dt: float = 0.01, calc_energy: bool = True, device: str = None, process_group=None,
                 calc_invariants: bool = False, dtype=torch.float32):
        self._check_dtype(dtype, process_group)                  # before anything is resolved, allocated or launched
        if process_group is not None and not (torch.distributed.is_available() and
                                              isinstance(process_group, torch.distributed.ProcessGroup)):
            raise ValueError("HermiteSimulator: process_group must be a torch.distributed process group, got "
                             f"{type(process_group).__name__} (dtype={dtype})")
        self.jerks = None
        self._fmt = _FORMATS[dtype]          # the only place the format is chosen; no method below asks which it is
        self._init_state(positions, velocities, masses, g_const, softening, dt, calc_energy, device, process_group,
                         calc_invariants)
        self._fmt.hermite_scratch(self)
        self.accelerations, self.jerks = self.compute_accelerations_and_jerks()

    def compute_accelerations_and_jerks(self):
        """(a, j) of the current state as new (n,3) tensors -- (n_local,3), the rank's rows, when sharded:
        a_i = G sum_{j!=i} m_j r_ij s^3, j_i = G sum_{j!=i} m_j (v_ij s^3 - 3 (r_ij.v_ij) s^5 r_ij),
        s = (|r_ij|^2 + eps^2)^(-1/2).
        With grad enabled and positions, velocities or masses requiring grad, the pair are nodes of torch's graph
        (nbd.autograd.direct_accel_jerk: the same forward bits, and a HIP backward, csrc/direct_hermite_grad.hip); the node
        packs its own copy of the state. step() and run() stay non-differentiable in-place kernels."""
        if self.n == 0:
            z = torch.zeros((0, 3), dtype=self.positions.dtype, device=self.device)
            return z, z.clone()
        if torch.is_grad_enabled() and (self.positions.requires_grad or self.velocities.requires_grad or
                                        self.masses.requires_grad):
            self._refuse_sharded("compute_accelerations_and_jerks() with requires_grad")
            from nbd.autograd import direct_accel_jerk
            return direct_accel_jerk(self.positions, self.velocities, self.masses, self.g_const, self.softening)
        if self._sharded:
            return self._sharded_launches()[:2]       # (the 6th-order format's force has the snap behind them)
        return self._fmt.accel_jerk(self)

    def _sharded_launches(self, carried=None, **pack):
        """The range-sharded launches from the carried derivatives, (acc, jerk) or the format's longer tuple: predict +
        pack of the own bodies, ONE all-gather in flight during the own x own block, then the own x others block, the
        slab sum and the corrector; returns as many new (n_local,3) tensors. With carried None the force of the current
        state on its own (a plain pack -- `pack` goes to the format's predictor --, no corrector): the format's
        `_shard_force_outputs` tensors."""
        fmt, n_loc = self._fmt, self.part.n_local
        new = tuple(torch.empty((n_loc, 3), dtype=fmt.dtype, device=self.device)
                    for _ in range(len(carried) if carried else fmt._shard_force_outputs))
        fmt._shard_predict(self, carried, **pack)
        handle = self._hgather.start(self._rows_local, self._rows_all)
        if n_loc:
            fmt._shard_local(self)
        self._hgather.finish(handle, self._rows_all)
        if n_loc:
            step = dict(pos=self.positions, vel=self.velocities, acc_in=carried[0], jerk_in=carried[1],
                        dt=self.dt) if carried else {}
            fmt._shard_remote(self, carried, new, **step)
        return new

    def step(self):
        """One predictor-corrector step: positions and velocities in place, `accelerations` and `jerks` rebound."""
        if self.n == 0:
            return
        if self._sharded:
            self.accelerations, self.jerks = self._sharded_launches((self.accelerations, self.jerks))
            return
        new_acc = torch.empty_like(self.accelerations)
        new_jerk = torch.empty_like(self.jerks)
        self._fmt.hermite_step(self, self.accelerations, self.jerks, new_acc, new_jerk)
        self.accelerations, self.jerks = new_acc, new_jerk

    _carried = BaseSimulator._carried + (("jerks", "_jerk_g"),)
    _posm_after_step = True

    def _step_in_place(self):
        self._fmt.hermite_step(self, self._acc_g, self._jerk_g, self._acc_g, self._jerk_g)


class Hermite6Simulator(HermiteSimulator):
    """Shared-timestep 6th-order Hermite predictor-corrector (Nitadori & Makino 2008) in float64
    (csrc/direct_hermite_f64.hip), an extension the reference does not have. The force evaluation carries
    one more derivative than HermiteSimulator's, the snap s = d^2 a / dt^2, and still runs once per step. With a0, j0, s0
    and the crackle c0 = d^3 a / dt^3 carried from the previous step:
        predict  x_p = x + v dt + a0 dt^2/2 + j0 dt^3/6 + s0 dt^4/24 + c0 dt^5/120
                 v_p = v + a0 dt + j0 dt^2/2 + s0 dt^3/6 + c0 dt^4/24
                 a_p = a0 + j0 dt + s0 dt^2/2 + c0 dt^3/6
        evaluate a1, j1, s1 at (x_p, v_p, a_p)
        correct  v1 = v + (a0 + a1) dt/2 - (j1 - j0) dt^2/10 + (s0 + s1) dt^3/120
                 x1 = x + (v + v1) dt/2 - (a1 - a0) dt^2/10 + (j0 + j1) dt^3/120
                 c1 = [60 (a1 - a0) - dt (36 j1 + 24 j0) + dt^2 (9 s1 - 3 s0)] / dt^3
    At construction the acceleration comes first (the inherited evaluation), then the evaluation with that acceleration
    as the third source array gives the snap, and c = 0.

    `accelerations`, `jerks`, `snaps` and `crackles` are (n,3) float64 device tensors that hold the values at the last
    predicted state; step() rebinds them. positions, velocities and masses are float64 as for
    HermiteSimulator(dtype=torch.float64), whose compute_energies(), compute_potentials(), compute_invariants(), gather()
    and eager run() work here unchanged. The only number format is float64 (`dtype` defaults to it): the fp32 Hermite run
    already sits on the fp32 floor at a few dozen steps, so a higher order buys nothing there. There is no differentiable
    form. Individual block timesteps are BlockHermite6Simulator (with max_level=0 this simulator bit for bit); many systems
    stepped together, with a captured run(), are BatchedSimulator(integrator="hermite6"), each scene bit-identical to this
    simulator on it alone.

    With `process_group=` the bodies are range-sharded as for HermiteSimulator(dtype=torch.float64)
    (the 6th-order entries of csrc/direct_hermite_shard_f64.hip): positions, velocities, accelerations,
    jerks, snaps and crackles hold the rank's rows [lo, hi), `gather()` assembles any of them, and a step is
    HermiteSimulator's sequence through the 6th-order format object: predict + pack of the own bodies -> ONE all-gather of
    12-double rows {x_p, m, v_p, 0, a_p, 0} in flight || own x own block -> own x others block + slab sum + corrector.
    Construction takes two exchanges (the acceleration, then the snap from it). run() is eager,
    compute_energies() gathers the float64 state on every rank, and compute_potentials(), compute_invariants() and
    run() with calc_invariants are refused as they are for the sharded HermiteSimulator."""

    def __init__(self, *, positions, velocities, masses, g_const: float = 1.0, softening: float = 0.1,
                 dt: float = 0.01, calc_energy: bool = True, device: str = None, process_group=None,
                 calc_invariants: bool = False, **format_kw):
        # all refusals before anything is resolved, allocated or launched
        dtype = format_kw.pop("dtype", torch.float64)
        if format_kw:
            raise TypeError(f"{type(self).__name__}.__init__() got an unexpected keyword argument "
                            f"{next(iter(format_kw))!r}")
        if dtype is not torch.float64:
            raise ValueError(f"Hermite6Simulator: dtype must be torch.float64, got {dtype!r}: the 4th-order fp32 run "
                             "already sits on the fp32 floor, so there is no fp32 form of the 6th-order scheme")
        if process_group is not None and not (torch.distributed.is_available() and
                                              isinstance(process_group, torch.distributed.ProcessGroup)):
            raise ValueError("Hermite6Simulator: process_group must be a torch.distributed process group, got "
                             f"{type(process_group).__name__}")
        self.jerks = self.snaps = self.crackles = None
        self._fmt = _HERMITE6                # the only place the format is chosen
        self._init_state(positions, velocities, masses, g_const, softening, dt, calc_energy, device, process_group,
                         calc_invariants)
        self._fmt.hermite_scratch(self)
        self.accelerations, self.jerks, self.snaps = self.compute_accelerations_jerks_and_snaps()
        self.crackles = torch.zeros_like(self.snaps)

    def compute_accelerations_jerks_and_snaps(self):
        """(a, j, s) of the current state as new (n,3) float64 tensors, in two passes: the acceleration first, then the
        evaluation that takes it as the third source array,
            s_i = G sum_{j!=i} m_j s^3 (a_ij - 6 alpha v_ij + (15 alpha^2 - 3 gamma) r_ij),
            alpha = (r_ij.v_ij) s^2, gamma = (v_ij.v_ij + r_ij.a_ij) s^2, s = (|r_ij|^2 + eps^2)^(-1/2).
        a and j are compute_accelerations_and_jerks()'s bits. Not differentiable. Sharded: the rank's rows, from two
        exchanges."""
        if torch.is_grad_enabled() and (self.positions.requires_grad or self.velocities.requires_grad or
                                        self.masses.requires_grad):
            raise RuntimeError("Hermite6Simulator.compute_accelerations_jerks_and_snaps(): there is no differentiable "
                               "form of the snap evaluation; call it under torch.no_grad() or on a detached state")
        if self.n == 0:
            z = torch.zeros((0, 3), dtype=torch.float64, device=self.device)
            return z, z.clone(), z.clone()
        if self._sharded:           # two exchanges: the rows with a zero third quad pair give a, the rows with that a give s
            return self._sharded_launches(acc=self._sharded_launches()[0])
        acc = self._fmt.accel(self)
        direct.hermite6_pack(self.positions, self.velocities, self.masses, self._posd, self._veld, self._accd, acc=acc)
        return direct.accel_jerk_snap_f64(self._posd, self._veld, self._accd, self.n, *self._fmt._scalars(self),
                                          workspace=self._hws)

    def step(self):
        """One predictor-corrector step: positions and velocities in place, `accelerations`, `jerks`, `snaps` and
        `crackles` rebound."""
        if self.n == 0:
            return
        cur = (self.accelerations, self.jerks, self.snaps, self.crackles)
        if self._sharded:
            self.accelerations, self.jerks, self.snaps, self.crackles = self._sharded_launches(cur)
            return
        new = tuple(torch.empty_like(t) for t in cur)
        direct.hermite6_step_f64(self.positions, self.velocities, *cur, *new, self.masses, self.dt,
                                 *self._fmt._scalars(self), self._posd, self._veld, self._accd, self._hws)
        self.accelerations, self.jerks, self.snaps, self.crackles = new


class _BlockSteps:
    """What the block-timestep simulators share (BlockHermiteSimulator, BlockHermite6Simulator), mixed in in front of the
    shared-timestep class whose scheme they run: the parameters `eta` and `max_level`, the int32 schedule state, the
    counters, the initial levels, the loop of block steps that makes one step(), and `process_group`: its refusals and
    the block step divided over its ranks (`_split_step`; float64, state replicated on every rank). The
    class's format object gives the workspace (`block_workspace`), the initial levels (`block_init_levels`, from
    `accelerations` and `jerks`) and `block_step(sim, n_act)`: the predict, force and correct of the block step the
    schedule has just listed, over the simulator's own state arrays."""

    MAX_LEVEL_LIMIT = 20

    @classmethod
    def _check_group(cls, process_group, split_min_active, dtype):
        """The refusals of `process_group` and `split_min_active`, before anything is resolved or allocated."""
        who = cls.__name__
        if process_group is None:
            if split_min_active is not None:
                raise ValueError(f"{who}: split_min_active is the threshold of the block steps divided over a "
                                 "process_group; there is none")
            return
        import torch.distributed as dist
        if not (dist.is_available() and isinstance(process_group, dist.ProcessGroup)):
            raise ValueError(f"{who}: process_group must be a torch.distributed.ProcessGroup, got "
                             f"{type(process_group).__name__}")
        if dtype is not torch.float64:
            raise ValueError(f"{who}: block steps are divided over a process_group in float64 only (dtype={dtype})")
        if split_min_active is None:
            raise ValueError(f"{who}: a process_group divides the block steps with at least split_min_active active "
                             f"bodies, and no exchange has been measured to set that threshold by default: pass "
                             f"split_min_active (an int >= 1; {who}.default_split_min_active(n, world) is the "
                             "provisional model)")
        if not (type(split_min_active) is int and split_min_active >= 1):
            raise ValueError(f"{who}: split_min_active must be an int >= 1, got {split_min_active!r}")

    @staticmethod
    def default_split_min_active(n: int, world: int) -> int:
        """A provisional threshold to pass as `split_min_active` (the constructors take none by themselves: a group
        without a threshold is refused): max(64 world, ceil(2^25 / n)) active bodies. On one GPU, one of 8 emulated ranks and
        no transport, the rank's share of a divided step first beats the un-divided step at n_act = 512 (n = 65 536) and
        512 to 1 024 (n = 16 384); at this threshold it is 10 to 30 us ahead, which is what is left for an exchange that
        nobody has measured (DESIGN.md K-HBS, NOTES.md; tools/bench_hermite_block_split.py)."""
        return max(64 * world, -(-(1 << 25) // max(n, 1)))

    def _init_block(self, eta, max_level, process_group=None, split_min_active=None):
        self.eta = eta
        self.max_level = max_level
        self.levels = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        self._ticks = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        self._sched = torch.zeros(direct.HBLOCK_SCHED_INTS, dtype=torch.int32, device=self.device)
        self._sched_host = torch.zeros(8, dtype=torch.int32).pin_memory()
        # the group of the divided block steps, in an attribute of its own: the state is replicated, so nothing of
        # BaseSimulator's range-sharded path (`_sharded`, `part`) is used
        self.process_group = self._split_group = process_group
        world, self._split_rank = nbd_dist.group_info(process_group) if process_group is not None else (1, 0)
        self._split_world = world
        forced = os.environ.get("NBD_FORCE_SHARDED") == "1"
        self._split = process_group is not None and self.n > 0 and (world > 1 or forced)
        self.split_min_active = split_min_active      # (_check_group: an int with a group, None without)
        self.split_block_steps = 0
        self.exchanged_rows = 0
        if self._split:
            self._bws = direct.hblock_split_workspace(self.n, self.device, self._fmt.block_order)
            q_max = direct.hblock_split_q(direct.hblock_split_slices(self.n, world))
            self._pieces = nbd_dist.PieceExchange(world, q_max, self._fmt.split_row, self.device, process_group,
                                                  collective=forced)
        else:
            self._bws = self._fmt.block_workspace(max(self.n, 1), self.device)
        self.block_steps = 0
        self.pair_interactions = 0
        self.clamped = 0
        self.level_history = None
        self._leveled_for = None
        self._set_levels()

    def _check_params(self):
        who = type(self).__name__
        if not (isinstance(self.max_level, int) and 0 <= self.max_level <= self.MAX_LEVEL_LIMIT):
            raise ValueError(f"{who}: max_level must be an int in [0, {self.MAX_LEVEL_LIMIT}]")
        if not (self.dt > 0 and self.eta > 0):
            raise ValueError(f"{who}: dt and eta must be positive")

    def _set_levels(self):
        self._check_params()
        self._leveled_for = (self.dt, self.eta, self.max_level)
        if self.n == 0:
            return
        self._fmt.block_init_levels(self.accelerations, self.jerks, self.dt, self.eta, self.max_level, self._ticks,
                                    self.levels, self._sched)
        self._read_clamped()

    def _read_clamped(self):
        self._sched_host.copy_(self._sched[:8])
        self.clamped = int(self._sched_host[2])
        if int(self._sched_host[direct.HBLOCK_SCHED_DIVERGED]):
            raise RuntimeError(f"{type(self).__name__}: the replicas diverged: a rank's piece of a divided block step "
                               "did not carry this rank's t_next, n_act or slice")

    def _split_step(self, n_act: int):
        """The block step the schedule has just listed, divided over the ranks: the list in index order, every body
        predicted, this rank's slice into its piece, one exchange, all rows applied."""
        fmt, K = self._fmt, self.max_level
        slices = direct.hblock_split_slices(n_act, self._split_world)
        q = direct.hblock_split_q(slices)
        first, count = slices[self._split_rank]
        direct.hblock_order_list(self.levels, K, self._sched, self._bws)
        fmt._block_predict(self)
        state, rows = fmt._block_rows_in(self)
        direct.hblock_split_rows(state, self.levels, n_act, first, count, K, self.dt, self.eta, *fmt._scalars(self),
                                 self._sched, rows, self._pieces.send, self._bws)
        direct.hblock_split_apply(self._pieces.exchange(q), self._split_world, q, n_act, fmt._block_state(self),
                                  self.masses, self._ticks, self.levels, K, self._sched, self._posd, self._bws)
        self.split_block_steps += 1
        self.exchanged_rows += n_act

    def step(self):
        """One output interval: block steps until every body is back at tick 2^max_level (at most 2^max_level of them)."""
        if self.n == 0:
            return
        if self._leveled_for != (self.dt, self.eta, self.max_level):
            self._set_levels()
        who = type(self).__name__
        K = self.max_level
        end = 1 << K
        host = self._sched_host
        t_prev = 0
        for _ in range(end):
            direct.hblock_schedule(self.levels, K, self._sched, self._bws, host_sched=host)
            t_next, n_act = int(host[0]), int(host[1])
            if not (t_prev < t_next <= end and 1 <= n_act <= self.n):
                raise RuntimeError(f"{who}: corrupt schedule (t_next={t_next}, n_act={n_act}, previous tick {t_prev})")
            if self._split and n_act >= self.split_min_active:
                self._split_step(n_act)
            else:
                self._fmt.block_step(self, n_act)
            self.block_steps += 1
            self.pair_interactions += n_act * self.n
            if self.level_history is not None:
                self.level_history.append(self.levels.cpu())
            if t_next == end:
                break
            t_prev = t_next
        else:
            raise RuntimeError(f"{who}: interval not finished within {end} block steps")
        self._read_clamped()


class BlockHermiteSimulator(_BlockSteps, HermiteSimulator):
    """HermiteSimulator with individual block timesteps (Makino & Aarseth 1992), an extension the reference does not have.
    `dt` is the output interval and the longest step: one step() advances every body by dt, in 2^max_level ticks. Body i
    moves with its own step dt 2^-k_i, k_i = levels[i] in [0, max_level], chosen by the Aarseth criterion
        dt_i = sqrt(eta (|a||a2| + |j|^2) / (|j||a3| + |a2|^2))
    (levels may deepen at any block step and rise by one where the block allows). On each block step only the bodies that
    are due are evaluated, against all bodies predicted to that time; every body is back in step at the end of the
    interval, so run() keeps returning one state per dt. Initial levels (at construction, and after dt, eta or max_level
    change) come from dt_i = (eta / 2) |a| / |j|.

    Counters (cumulative Python ints): `block_steps`, `pair_interactions` (sum of n_act * n over block steps) and `clamped`
    (levels the criterion wanted deeper than max_level, NaN criteria included). `accelerations` and `jerks` are updated in
    place. Eager-only: every block step reads {t_next, n_act} back to the host (csrc/direct_hermite_block.hip). Setting
    `level_history` to a list records a CPU copy of `levels` after every block step (tests, diagnostics).

    `dtype` is HermiteSimulator's keyword and is handed on to it (default torch.float32; anything but float32 or float64
    raises ValueError before anything is allocated).
    With `dtype=torch.float64` (csrc/direct_hermite_block_f64.hip) the same scheme runs in the number
    format of HermiteSimulator(dtype=torch.float64): positions, velocities, masses, accelerations and jerks are float64
    device tensors, g_const, softening ** 2, dt and every body's own step constants go to the kernels as doubles, and the
    pair arithmetic and all sums are float64; levels, ticks and the schedule stay int32. An fp32 block run stops gaining
    from a smaller eta at the fp32 floor of the orbit; this mode follows the criterion down to float64 rounding. With
    max_level=0 it is HermiteSimulator(dtype=torch.float64) bit for bit. compute_*() and run() are that class's.

    `process_group` (float64 only; csrc/direct_hermite_block_split_f64.hip, DESIGN.md K-HBS) divides the large block steps
    over the ranks of a torch.distributed.ProcessGroup. Unlike the other `process_group=` simulators, which hold their own
    rows, the state here is REPLICATED: positions, velocities, accelerations, jerks, masses and levels are the full arrays
    on every rank, bit for bit the same, construction (first force, initial levels) runs redundantly on every rank, and
    gather(), compute_energies(), compute_potentials(), compute_invariants() and run() (calc_invariants too) work unchanged
    on every rank with no communication. A block step with at least `split_min_active` active bodies is divided: each
    rank evaluates and corrects its slice of the index-ordered active list, one all_gather_into_tensor carries the
    corrected rows (n_act of them, never n) and every rank applies all of them; smaller block steps run redundantly with
    no collective. `split_min_active` (a keyword beside `dtype`; an int >= 1) is REQUIRED with a group and refused
    without one: no exchange has been measured here, so there is no default, and a group without a threshold raises
    ValueError as it did before this mode existed. `default_split_min_active(n, world)` = max(64 world, ceil(2^25 / n))
    is a PROVISIONAL value to pass: it rests on a one-GPU measurement without transport. Counters: `split_block_steps` and `exchanged_rows` (sum of n_act over divided steps). The results are
    the un-divided simulator's bit for bit wherever a slice and the whole block get the same slab count (every n <= 448;
    always with one rank), and to rounding elsewhere. A one-rank group divides only with NBD_FORCE_SHARDED=1. step() raises
    RuntimeError if the ranks' pieces ever disagree about t_next, n_act or the slices ("replicas diverged"). Anything that
    is not a ProcessGroup, float32 with a group, a group without `split_min_active`, and a `split_min_active` without a
    group or not an int >= 1 raise ValueError before a device is resolved."""

    def __init__(self, *, positions, velocities, masses, g_const: float = 1.0, softening: float = 0.1,
                 dt: float = 0.01, calc_energy: bool = True, device: str = None, process_group=None,
                 eta: float = 0.02, max_level: int = 10, calc_invariants: bool = False, **hermite_kw):
        # hermite_kw: `split_min_active` (_BlockSteps; required with a group, refused without), taken out here, and the keywords that are
        # HermiteSimulator's own and mean here what they mean there -- `dtype` (default torch.float32). Those go to
        # HermiteSimulator.__init__ as given, which refuses a name it does not know.
        split_min_active = hermite_kw.pop("split_min_active", None)
        self._check_dtype(hermite_kw.get("dtype", torch.float32), None)     # before anything is resolved or allocated
        self._check_group(process_group, split_min_active, hermite_kw.get("dtype", torch.float32))
        # the state is replicated: HermiteSimulator is built without the group, on all n bodies, on every rank
        super().__init__(positions=positions, velocities=velocities, masses=masses, g_const=g_const,
                         softening=softening, dt=dt, calc_energy=calc_energy, device=device,
                         calc_invariants=calc_invariants, **hermite_kw)
        self._init_block(eta, max_level, process_group, split_min_active)


class BlockHermite6Simulator(_BlockSteps, Hermite6Simulator):
    """Hermite6Simulator with individual block timesteps, the form Nitadori & Makino (2008) wrote the scheme for
    (csrc/direct_hermite_block_f64.hip at the 6th order), an extension the reference does not have.
    `dt` is the output interval and the longest step: one step() advances every body by dt, in 2^max_level ticks. Body i carries x, v, a, j,
    s and the crackle c at its last correction and moves with its own step h_i = dt 2^-k_i, k_i = levels[i] in
    [0, max_level]. A block step predicts every body to the next due time by Hermite6Simulator's Taylor series over its
    own elapsed time, evaluates a1, j1, s1 of the due bodies against all predicted bodies, corrects them with their own
    h_i and re-levels them from the generalised Aarseth criterion for p = 6,
        dt_i = (eta^3 (|a1||s1| + |j1|^2) / (|c1||a5| + |a4|^2))^(1/6),
    a4 (at the end of the step) and a5 from the quintic through (a, j, s) at both ends, c1 the crackle just formed; eta
    keeps BlockHermiteSimulator's convention (dt_i = sqrt(eta ...) there). Levels may deepen at any block step and rise
    by one where the block allows. Initial levels (at construction, and after dt, eta or max_level change) come from
    dt_i = (eta / 2) |a| / |j|; the start is Hermite6Simulator's (a first, then the snap from it, c = 0).

    The public surface is BlockHermiteSimulator's: `eta`, `max_level`, `levels`, the cumulative counters `block_steps`,
    `pair_interactions` and `clamped`, `level_history`, MAX_LEVEL_LIMIT. `accelerations`, `jerks`, `snaps` and `crackles`
    are updated in place. Float64 only and eager-only (every block step reads {t_next, n_act} back to the host); there is
    no captured or differentiable form; BatchedSimulator(integrator="block_hermite6") is the batched one.
    With max_level=0 it is Hermite6Simulator bit for bit.
    compute_*() and run() are that class's.

    `process_group` and `split_min_active` are BlockHermiteSimulator's (DESIGN.md K-HBS): the state (with `snaps` and
    `crackles`) is REPLICATED on every rank -- not the rank's own rows, as in the other `process_group=` simulators -- so
    gather(), compute_*() and run() work unchanged on every rank without communication; block steps with at least
    `split_min_active` active bodies (required with a group; `default_split_min_active(n, world)` is a provisional value
    to pass) are divided over the ranks, one
    all_gather_into_tensor of the corrected rows each; `split_block_steps` and `exchanged_rows` count them. The same
    refusals, each a ValueError before a device is resolved."""

    def __init__(self, *, positions, velocities, masses, g_const: float = 1.0, softening: float = 0.1,
                 dt: float = 0.01, calc_energy: bool = True, device: str = None, process_group=None,
                 eta: float = 0.02, max_level: int = 10, calc_invariants: bool = False,
                 split_min_active: int = None, **format_kw):
        # all refusals before anything is resolved, allocated or launched; format_kw is Hermite6Simulator's (`dtype`)
        unknown = [k for k in format_kw if k != "dtype"]
        if unknown:
            raise TypeError(f"{type(self).__name__}.__init__() got an unexpected keyword argument {unknown[0]!r}")
        dtype = format_kw.get("dtype", torch.float64)
        if dtype is not torch.float64:
            raise ValueError(f"BlockHermite6Simulator: dtype must be torch.float64, got {dtype!r}: there is no fp32 form "
                             "of the 6th-order scheme")
        self._check_group(process_group, split_min_active, dtype)
        # the state is replicated: Hermite6Simulator is built without the group, on all n bodies, on every rank
        super().__init__(positions=positions, velocities=velocities, masses=masses, g_const=g_const,
                         softening=softening, dt=dt, calc_energy=calc_energy, device=device,
                         calc_invariants=calc_invariants, **format_kw)
        self._init_block(eta, max_level, process_group, split_min_active)


def _per_scene(x, n_scenes: int, name: str) -> list:
    """A scalar, or one value per scene -> list of S Python floats."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().tolist()
    if np.ndim(x) == 0:
        return [float(x)] * n_scenes
    vals = [float(v) for v in np.asarray(x, dtype=np.float64).reshape(-1)]
    if len(vals) != n_scenes:
        raise ValueError(f"{name}: expected a scalar or {n_scenes} values, got {len(vals)}")
    return vals


def _batch_chunk_layout(m: int, n: int, n_scenes: int, dtype=torch.float32):
    """A batch's chunk buffer, in bytes: ring (m, 3, n, 3) of the state's dtype | energies (m, S, 2) fp64 from the next
    multiple of 16 -> (ring bytes, energies' offset, size)."""
    ring_b = m * 9 * n * dtype.itemsize
    uk_at = (ring_b + 15) // 16 * 16
    return ring_b, uk_at, uk_at + m * n_scenes * 16


def _batch_chunk_views(buf, m: int, n: int, n_scenes: int, dtype=torch.float32):
    """(ring, energies) views of a chunk buffer, on the device or in its host copy."""
    ring_b, uk_at, size = _batch_chunk_layout(m, n, n_scenes, dtype)
    return (buf[:ring_b].view(dtype).view(m, 3, n, 3),
            buf[uk_at:size].view(torch.float64).view(m, n_scenes, 2))


def _batch_states(host, m: int, offsets: list, calc_energy: bool, first: int, t_steps, out, inv=None,
                  dtype=torch.float32):
    """Append m states per scene to `out` from a host copy of a chunk buffer (views into it, no copies). inv: a host copy
    of the chunk's invariant rows (m, S, 16), or None."""
    n_scenes = len(offsets) - 1
    ring, uk = _batch_chunk_views(host, m, offsets[-1], n_scenes, dtype)
    uk = uk.tolist() if calc_energy else None
    inv = inv.tolist() if inv is not None else None
    for s_ in range(m):
        for i in range(n_scenes):
            lo, hi = offsets[i], offsets[i + 1]
            u, k = (uk[s_][i][0], uk[s_][i][1]) if calc_energy else (None, None)
            out[i].append(SimulationState(step=first + s_, step_time=t_steps[s_], positions=ring[s_, 0, lo:hi],
                                          velocities=ring[s_, 1, lo:hi], accelerations=ring[s_, 2, lo:hi],
                                          u_energy=u, k_energy=k,
                                          invariants=Invariants.from_row(inv[s_][i]) if inv is not None else None))


class _BatchFormat:
    """What every format object of BatchedSimulator shares: the parameter table's upkeep (`extra_params`, `write_params`),
    one step() of the shared-timestep integrators (`advance`: new carried arrays, rebound) and the flags `capturable`
    (run() may capture its chunks) and `block` (a block-timestep format, `_BatchBlock`)."""

    capturable = True
    block = False

    def extra_params(self, s) -> tuple:
        """Per-scene parameter lists beyond (g_const, softening, dt); they join the key of the table."""
        return ()

    def write_params(self, s, g, eps, dt):
        s._params.copy_(torch.tensor(self.param_rows(g, eps, dt), dtype=self.dtype))

    def start(self, s):
        """What the format sets up once the first forces are known (nothing for a shared timestep)."""

    def advance(self, s):
        cur = [getattr(s, public) for public, _ in s._carried]
        new = [torch.empty_like(t) for t in cur]
        s._step_into(cur, new)
        for (public, _), t in zip(s._carried, new):
            setattr(s, public, t)


class _BatchFloat32(_BatchFormat):
    """The float32 number format of BatchedSimulator: every allocation and nbd.direct call of a batch `s` that depends on
    the format (the object keeps no state of its own); `_BatchFloat64` has the same methods. Packed sources: `s._posm` =
    {x, y, z, m}; the Hermite calls keep their packed velocities inside `s._hws`, allocated on first use. Parameter table
    `s._params`: rows g, eps^2, eps, dt / 2, dt, as torch forms the fp32 scalars from the Python doubles
    (simulation.py:82,88,164), then the Hermite step constants dt, dt/2, dt^2/2, dt^3/6, dt^2/12, each formed in double
    and rounded once (as HermiteSimulator's)."""

    dtype = torch.float32
    integrators = ("leapfrog", "euler", "hermite")

    def scratch(self, s):
        s._plan = direct.BatchPlan(s.sizes, s.device)
        s._posm = s._plan.alloc_posm()
        s._ws = s._plan.workspace()
        s._params = torch.zeros((10, s.n_scenes), dtype=torch.float32, device=s.device)
        s._hws = None

    def param_rows(self, g, eps, dt) -> list:
        f32 = direct.f32
        return [[f32(x) for x in g], [f32(e ** 2) for e in eps], [f32(e) for e in eps],
                [f32(0.5 * d) for d in dt], [f32(d) for d in dt],
                [f32(d) for d in dt], [f32(0.5 * d) for d in dt], [f32(0.5 * d * d) for d in dt],
                [f32(d * d * d / 6.0) for d in dt], [f32(d * d / 12.0) for d in dt]]

    def _hermite_ws(self, s) -> torch.Tensor:
        if s._hws is None:
            s._hws = s._plan.hermite_workspace()
        return s._hws

    def accel(self, s):
        acc = torch.zeros((s.n, 3), dtype=torch.float32, device=s.device)
        P = s._params
        direct.batch_accel(s._plan, s.positions, s.masses, P[1], P[0], acc, s._posm, s._ws)
        return acc

    def accel_jerk(self, s, acc, jerk):
        P = s._params
        direct.batch_accel_jerk(s._plan, s.positions, s.velocities, s.masses, P[1], P[0], acc, jerk, s._posm,
                                self._hermite_ws(s))

    def hermite_step(self, s, cur, new):
        P = s._params
        direct.batch_hermite_step(s._plan, s.positions, s.velocities, cur[0], cur[1], new[0], new[1], s.masses, P[5:10],
                                  P[1], P[0], s._posm, s._hws)

    def pack(self, s):
        direct.batch_pack_posm(s._plan, s.positions, s.masses, s._posm)

    def energies(self, s, out_uk):
        P = s._params
        direct.batch_energies(s._plan, s._posm, s.velocities, P[2], P[0], out_uk, s._ws)

    def potentials(self, s, phi):
        P = s._params
        return direct.batch_potential(s._plan, s._posm, P[1], P[0], phi, s._ws)

    def invariants(self, s, phi, out_rows):
        return direct.batch_invariants(s._plan, s._posm, s.velocities, phi, out_rows)

    snapshot = staticmethod(direct.snapshot)


class _BatchFloat64(_BatchFormat):
    """The float64 number format of BatchedSimulator (csrc/direct_batch_hermite_f64.hip): `_BatchFloat32`'s methods over the
    float64 entries, Hermite only; nothing of the fp32 paths is allocated or launched. Packed sources: `s._posd` =
    {x, y, z, m}, `s._veld` = {vx, vy, vz, 0}; ONE workspace `s._ws` for the step and the diagnostics. Parameter table
    `s._params`: the doubles G, eps^2, eps and the five step constants, formed by the expressions of
    HermiteSimulator(dtype=torch.float64)'s path (direct.batch_f64_params): the kernels read every per-scene scalar from
    it, which is what lets run() capture the float64 step."""

    dtype = torch.float64
    integrators = ("hermite",)

    def scratch(self, s):
        s._plan = direct.BatchPlan(s.sizes, s.device, dtype=torch.float64)
        s._posd = direct.alloc_batch_rows_f64(s._plan)
        s._veld = direct.alloc_batch_rows_f64(s._plan)
        s._ws = s._plan.workspace()
        s._params = torch.zeros((direct.BATCH_F64_PARAM_ROWS, s.n_scenes), dtype=torch.float64, device=s.device)

    def param_rows(self, g, eps, dt) -> list:
        return direct.batch_f64_params(g, eps, dt)

    def accel(self, s):
        return s.compute_accelerations_and_jerks()[0]

    def accel_jerk(self, s, acc, jerk):
        direct.batch_accel_jerk_f64(s._plan, s.positions, s.velocities, s.masses, s._params, acc, jerk, s._posd, s._veld,
                                    s._ws)

    def hermite_step(self, s, cur, new):
        direct.batch_hermite_step_f64(s._plan, s.positions, s.velocities, cur[0], cur[1], new[0], new[1], s.masses,
                                      s._params, s._posd, s._veld, s._ws)

    def pack(self, s):
        direct.batch_pack_f64(s._plan, s.positions, s.velocities, s.masses, s._posd, s._veld)

    def energies(self, s, out_uk):
        direct.batch_energies_f64(s._plan, s._posd, s.velocities, s._params, out_uk, s._ws)

    def potentials(self, s, phi):
        return direct.batch_potential_f64(s._plan, s._posd, s._params, phi, s._ws)

    def invariants(self, s, phi, out_rows):
        return direct.batch_invariants_state_f64(s._plan, s.positions, s.velocities, s.masses, phi, out_rows)

    snapshot = staticmethod(direct.snapshot_f64)


class _BatchHermite6(_BatchFloat64):
    """The float64 format of BatchedSimulator(integrator="hermite6") (csrc/direct_batch_hermite_f64.hip): `_BatchFloat64`
    with the 9-row plan and its workspace, the third packed array `s._accd` = {ax, ay, az, 0} and the taller parameter
    table (direct.batch_h6_params: G, eps^2, eps, then Hermite6Step's constants). The carried arrays are
    (accelerations, jerks, snaps, crackles). The inherited pack, acceleration + jerk, energies, potentials and invariants
    run on the same plan, workspace and table: they read a scene's workspace offset from the plan and rows 0..2 of the
    table."""

    integrators = ("hermite6",)

    def scratch(self, s):
        s._plan = direct.BatchPlan(s.sizes, s.device, dtype=torch.float64, order=6)
        s._posd, s._veld, s._accd = (direct.alloc_batch_rows_f64(s._plan) for _ in range(3))
        s._ws = s._plan.workspace()
        s._params = torch.zeros((direct.BATCH_H6_PARAM_ROWS, s.n_scenes), dtype=torch.float64, device=s.device)

    def param_rows(self, g, eps, dt) -> list:
        return direct.batch_h6_params(g, eps, dt)

    def accel_jerk_snap(self, s, acc, jerk, snap):
        """Hermite6Simulator's two passes: the acceleration first (acc, jerk serve as its outputs), then the evaluation
        that takes it as the third source array."""
        self.accel_jerk(s, acc, jerk)
        direct.batch_hermite6_pack_f64(s._plan, s.positions, s.velocities, s.masses, s._posd, s._veld, s._accd, acc=acc)
        direct.batch_accel_jerk_snap_f64(s._plan, s._posd, s._veld, s._accd, s._params, acc, jerk, snap, s._ws)

    def hermite_step(self, s, cur, new):
        direct.batch_hermite6_step_f64(s._plan, s.positions, s.velocities, *cur, *new, s.masses, s._params, s._posd,
                                       s._veld, s._accd, s._ws)


class _BatchBlock:
    """The block-timestep part of a batch format (csrc/direct_batch_hermite_block_f64.hip; DESIGN.md K-BHB), mixed in in
    front of the shared-timestep float64 format whose scheme it runs (`_BatchFloat64`: "block_hermite"; `_BatchHermite6`:
    "block_hermite6"). That format keeps the plan, the packed rows, the first forces and the diagnostics. Added here: the
    static work list and workspace of the block step (`s._bplan`, `s._bws`), the int32 schedule state (`s.levels`,
    `s._ticks`, the device records `s._bsched`), the per-scene counters `s._counters`, a second parameter table
    `s._bparams` (G, eps^2, eps, dt, eta), the initial levels and the loop of ensemble block steps that makes one
    step() -- `_BlockSteps.step` with ONE schedule and one host read for all scenes."""

    capturable = False
    block = True
    order = 4
    integrators = ("block_hermite",)
    state_names = ("positions", "velocities", "accelerations", "jerks")
    row_names = ("_posd", "_veld")

    def scratch(self, s):
        super().scratch(s)
        s._bplan = direct.BatchBlockPlan(s.sizes, s.device, order=self.order)
        s._bws = s._bplan.workspace()
        s._bsched = s._bplan.sched()
        s._counters = s._bplan.counters()
        s._bparams = torch.zeros((direct.BATCH_HBLOCK_PARAM_ROWS, s.n_scenes), dtype=torch.float64, device=s.device)
        s.levels = torch.zeros(s.n, dtype=torch.int32, device=s.device)
        s._ticks = torch.zeros(s.n, dtype=torch.int32, device=s.device)
        s._sched_host = torch.zeros(4, dtype=torch.int32).pin_memory()
        s._leveled_for = None

    def extra_params(self, s) -> tuple:
        return (_per_scene(s.eta, s.n_scenes, "eta"),)

    def write_params(self, s, g, eps, dt, eta):
        super().write_params(s, g, eps, dt)
        s._bparams.copy_(torch.tensor(direct.batch_hblock_params(g, eps, dt, eta), dtype=torch.float64))

    @staticmethod
    def check_level(max_level):
        limit = _BlockSteps.MAX_LEVEL_LIMIT
        if not (isinstance(max_level, int) and 0 <= max_level <= limit):
            raise ValueError(f"BatchedSimulator: max_level must be an int in [0, {limit}]")

    @classmethod
    def check_params(cls, s, dt, eta):
        cls.check_level(s.max_level)
        if not (all(d > 0 for d in dt) and all(e > 0 for e in eta)):
            raise ValueError("BatchedSimulator: dt and eta must be positive")

    def start(self, s):
        s._sync_params()
        self.set_levels(s)

    def set_levels(self, s):
        """`_BlockSteps._set_levels` per scene: the initial levels of the scenes whose dt or eta changed (all of them the
        first time and after max_level changed), from the batch's accelerations and jerks. Parameters in sync."""
        dt, eta = s._params_key[2], s._params_key[3]
        new = (dt, eta, s.max_level)
        old = s._leveled_for
        if new == old:
            return
        self.check_params(s, dt, eta)
        s._leveled_for = new
        if s.n == 0:
            return
        mask = None
        if old is not None and old[2] == s.max_level:
            mask = torch.tensor([int(a != b or c != d) for a, b, c, d in zip(dt, old[0], eta, old[1])],
                                dtype=torch.int32).to(s.device)
        direct.batch_hblock_init_levels(s._bplan, s.accelerations, s.jerks, s._bparams, s.max_level, s._ticks, s.levels,
                                        s._bsched, mask=mask)

    def advance(self, s):
        """One output interval of every scene: ensemble block steps until every body is back at tick 2^max_level."""
        self.set_levels(s)
        K = s.max_level
        end = 1 << K
        host = s._sched_host
        state = tuple(getattr(s, name) for name in self.state_names)
        rows = tuple(getattr(s, name) for name in self.row_names)
        t_prev = 0
        for _ in range(end):
            direct.batch_hblock_schedule(s._bplan, s.levels, K, s._bsched, s._counters, s._bws, host_sched=host)
            t_next, n_act = int(host[0]), int(host[1])
            if not (t_prev < t_next <= end and 1 <= n_act <= s.n):
                raise RuntimeError(f"BatchedSimulator: corrupt schedule (t_next={t_next}, n_act={n_act}, previous tick "
                                   f"{t_prev})")
            direct.batch_hblock_step(s._bplan, state, s.masses, s._ticks, s.levels, s._bparams, K, s._bsched, rows,
                                     s._bws)
            s.block_steps += 1
            if s.tick_history is not None:
                s.tick_history.append((t_next, n_act))
            if s.level_history is not None:
                s.level_history.append(s.levels.cpu())
            if t_next == end:
                break
            t_prev = t_next
        else:
            raise RuntimeError(f"BatchedSimulator: interval not finished within {end} block steps")


class _BatchBlockHermite(_BatchBlock, _BatchFloat64):
    """BatchedSimulator(integrator="block_hermite"): BlockHermiteSimulator(dtype=torch.float64)'s scheme per scene."""


class _BatchBlockHermite6(_BatchBlock, _BatchHermite6):
    """BatchedSimulator(integrator="block_hermite6"): BlockHermite6Simulator's scheme per scene."""

    order = 6
    integrators = ("block_hermite6",)
    state_names = _BatchBlock.state_names + ("snaps", "crackles")
    row_names = _BatchBlock.row_names + ("_accd",)


_BATCH_FORMATS = {fmt.dtype: fmt for fmt in (_BatchFloat32(), _BatchFloat64())}
# the integrators with a float64-only format of their own
_BATCH_OWN_FORMATS = {"hermite6": _BatchHermite6(), "block_hermite": _BatchBlockHermite(),
                      "block_hermite6": _BatchBlockHermite6()}
_BATCH_INTEGRATORS = ("leapfrog", "euler", "hermite", "hermite6", "block_hermite", "block_hermite6")
_BATCH_BLOCK_INTEGRATORS = ("block_hermite", "block_hermite6")


def _batch_format(dtype, integrator):
    """The format object of a batch: by dtype, and the 6th-order and the block schemes have one of their own."""
    return _BATCH_OWN_FORMATS.get(integrator) or _BATCH_FORMATS[dtype]


class BatchedSimulator(_ChunkedRun):
    """S independent systems ("scenes") advanced together: one set of launches per step for all of them
    (csrc/direct_batch.hip). Each body feels only the bodies of its own scene, with that scene's g_const, softening
    and dt (scalars, or one value per scene). The scenes are stored back to back: `positions`, `velocities`,
    `accelerations` are (N_total, 3) and `masses` (N_total,), scene s owning rows offsets[s]:offsets[s + 1];
    `scene(s)` returns views of them. A scene's results do not depend on its companions or its position in the batch
    (bit for bit). There is no CPU path and no multi-GPU sharding: the batch runs on one device.

    integrator="hermite" is HermiteSimulator's shared-timestep predictor-corrector on every scene
    (csrc/direct_batch_hermite.hip): `jerks` (N_total, 3) is public next to `accelerations`, both rebound by step(), and
    each scene's positions, velocities, accelerations and jerks are bit-identical to a HermiteSimulator of that scene
    alone. `jerks` is None for leapfrog and Euler. The integrator may switch between leapfrog and Euler after
    construction, but not into or out of Hermite.

    With `dtype=torch.float64` (integrator="hermite" only; csrc/direct_batch_hermite_f64.hip) every
    scene runs HermiteSimulator(dtype=torch.float64)'s step: positions, velocities, masses, accelerations and jerks are
    float64 device tensors (the inputs are converted directly, not through float32), each scene's g_const, softening ** 2,
    dt and step constants reach the kernels as doubles through a device table, and step(), the compute_*() methods and
    run() -- its states, energies and invariants -- are float64 end to end, each scene bit-identical to a
    HermiteSimulator(dtype=torch.float64) of that scene alone. Because the table, not a kernel argument, carries the
    scalars, run() captures its chunks in this mode too. The default stays float32 and takes the paths it took.

    integrator="hermite6" (csrc/direct_batch_hermite_f64.hip) is Hermite6Simulator's 6th-order step on
    every scene, float64 only (`dtype` then defaults to torch.float64; torch.float32 is refused): `accelerations`,
    `jerks`, `snaps` and `crackles` are (N_total, 3) float64 tensors rebound by step(), built as Hermite6Simulator builds
    them (the acceleration first, then the evaluation with it as the third source array, crackle 0), and each scene's
    state is bit-identical to a Hermite6Simulator of that scene alone. run() captures its chunks as for the float64
    4th-order mode, the four arrays stepped in place; energies, potentials and invariants are that mode's. The
    integrator cannot switch into or out of "hermite6", nor between "hermite" and "hermite6".

    integrator="block_hermite" and "block_hermite6" (csrc/direct_batch_hermite_block_f64.hip; DESIGN.md K-BHB) run
    BlockHermiteSimulator(dtype=torch.float64)'s resp. BlockHermite6Simulator's individual block timesteps on every scene,
    float64 only. All scenes share one grid of 2^max_level ticks per output interval (`max_level`: one int for the batch, in
    [0, MAX_LEVEL_LIMIT]); `eta` is a float or one value per scene. Under the block condition the union of the scenes'
    schedules is itself a block schedule, so ONE scheduler launch, one host read of {t_next, n_act_total} and one predict /
    force / correct launch set serve all scenes per ensemble block step, and every scene still takes exactly the block
    steps it would take alone: its positions, velocities, accelerations, jerks (snaps, crackles), `levels` and counters
    are bit-identical to the one-system block simulator of that scene, whatever its companions. `levels` is an
    (N_total,) int32 device tensor; `block_steps` counts the ensemble's block steps; `scene_counters()` reads the per-scene
    counters the kernels keep on the device; `tick_history` (set to a list) receives (t_next, n_act_total) per ensemble
    block step and `level_history` a CPU copy of `levels`. The carried arrays are updated in place. Changing dt, eta or
    max_level re-derives the initial levels of the scenes concerned before the next step(). Eager-only; with max_level=0
    the modes are "hermite" (float64) and "hermite6" bit for bit. The integrator cannot change into, out of or between
    the block modes; `eta` and `max_level` are refused with any other integrator."""

    RING_BYTES = 64 << 20                                # the eager run()'s staging cap, per chunk of states

    @staticmethod
    def _check_dtype(dtype, integrator):
        if dtype not in _BATCH_FORMATS:
            raise ValueError(f"BatchedSimulator: dtype must be torch.float32 or torch.float64, got {dtype!r}")
        if integrator in _BATCH_OWN_FORMATS:
            if dtype is not torch.float64:
                raise ValueError(f"BatchedSimulator: integrator={integrator!r} is float64 only (dtype must be "
                                 f"torch.float64, got {dtype!r}): there is no fp32 form of "
                                 + ("the 6th-order scheme" if integrator == "hermite6" else "the batched block schemes"))
        elif integrator not in _BATCH_FORMATS[dtype].integrators:
            raise ValueError(f"BatchedSimulator: dtype={dtype} has integrator='hermite' only (there is no float64 "
                             f"leapfrog or Euler), got {integrator!r}")

    def __init__(self, *, systems, integrator: str = "leapfrog", g_const=1.0, softening=0.1, dt=0.01,
                 calc_energy: bool = True, device: str = None, calc_invariants: bool = False, eta=None,
                 max_level: int = None, **format_kw):
        # format_kw: `dtype` (default torch.float32; torch.float64 for "hermite6" and the block modes), the one keyword of
        # the number format. As in BlockHermiteSimulator it is not a named parameter: HermiteSimulator's signature stays the only one that spells it (tested); any other
        # name is refused as an unknown keyword is.
        dtype = format_kw.pop("dtype", torch.float64 if integrator in _BATCH_OWN_FORMATS else torch.float32)
        if format_kw:
            raise TypeError(f"BatchedSimulator.__init__() got an unexpected keyword argument {next(iter(format_kw))!r}")
        if integrator not in _BATCH_INTEGRATORS:
            raise ValueError("integrator must be 'leapfrog', 'euler', 'hermite', 'hermite6', 'block_hermite' or "
                             "'block_hermite6'")
        self._check_dtype(dtype, integrator)             # before anything is resolved, allocated or launched
        if integrator in _BATCH_BLOCK_INTEGRATORS:
            self.eta = 0.02 if eta is None else eta      # the defaults of the one-system block simulators
            self.max_level = 10 if max_level is None else max_level
            _BatchBlock.check_level(self.max_level)
        elif eta is not None or max_level is not None:
            raise ValueError(f"BatchedSimulator: eta and max_level belong to the block integrators "
                             f"{_BATCH_BLOCK_INTEGRATORS}, not to integrator={integrator!r}")
        self._fmt = _batch_format(dtype, integrator)     # the only place the format is chosen
        self.device = _resolve_device(device)
        _lib.lib()
        systems = list(systems)
        if not systems:
            raise ValueError("systems: need at least one (positions, velocities, masses) scene")
        self.integrator = self._built_as = integrator
        self.calc_energy = calc_energy
        self.calc_invariants = calc_invariants
        self.n_scenes = len(systems)
        self.block_steps = 0                             # the block modes' public state; `levels` is theirs alone
        self.levels = self.tick_history = self.level_history = None
        pos, vel, mass = [], [], []
        for i, sysm in enumerate(systems):
            p, v, m = (_to_device(x, self.device, dtype) for x in sysm)
            n = p.shape[0]
            if p.shape != (n, 3) or v.shape != (n, 3) or m.shape != (n,):
                raise ValueError(f"scene {i}: positions/velocities must be (n,3) and masses (n,)")
            pos.append(p); vel.append(v); mass.append(m)
        self.sizes = [p.shape[0] for p in pos]
        self.positions = torch.cat(pos).contiguous()
        self.velocities = torch.cat(vel).contiguous()
        self.masses = torch.cat(mass).contiguous()
        self.n = self.positions.shape[0]
        self._fmt.scratch(self)                          # the plan, the packed rows, the workspace, the parameter table
        self.offsets = torch.tensor(self._plan.offsets, dtype=torch.int64)
        self.g_const, self.softening, self.dt = g_const, softening, dt
        self._params_key = None
        self._hermite = integrator not in ("leapfrog", "euler")   # fixed at construction: the state carries jerks or not
        self._order6 = integrator in ("hermite6", "block_hermite6")         # ... and snaps and crackles
        self._phi = None
        self.jerks = self.snaps = self.crackles = None
        if self._order6:
            self._carried = self._carried + (("jerks", "_jerk_g"), ("snaps", "_snap_g"), ("crackles", "_crackle_g"))
            self.accelerations, self.jerks, self.snaps = self.compute_accelerations_jerks_and_snaps()
            self.crackles = torch.zeros_like(self.snaps)
        elif self._hermite:
            self._carried = self._carried + (("jerks", "_jerk_g"),)
            self.accelerations, self.jerks = self.compute_accelerations_and_jerks()
        else:
            self.accelerations = self.compute_accelerations()
        self._fmt.start(self)                            # a block format: the initial levels

    MAX_LEVEL_LIMIT = _BlockSteps.MAX_LEVEL_LIMIT

    def scene_counters(self) -> list:
        """The block modes' counters per scene, cumulative, as the one-system block simulator of that scene reports them:
        dicts of `block_steps` (the ensemble block steps in which the scene had an active body), `pair_interactions` (sum of
        n_act_s * n_s) and `clamped`. Read from the device tables here, and only here."""
        if not self._fmt.block:
            raise ValueError("BatchedSimulator.scene_counters(): the block integrators only")
        counts = self._counters.cpu().tolist()
        clamped = self._bsched[1:, 2].cpu().tolist()
        return [{"block_steps": c[0], "pair_interactions": c[1], "clamped": k} for c, k in zip(counts, clamped)]

    # ------------------------------------------------------------------ per-scene parameters
    def _sync_params(self):
        """The device parameter table in the format's own rows (`_BatchFloat32`, `_BatchFloat64`), rewritten IN PLACE when
        an attribute changed (captured graphs keep reading the same buffer). Returns the per-scene values (the graph
        cache key)."""
        S = self.n_scenes
        g = _per_scene(self.g_const, S, "g_const")
        eps = _per_scene(self.softening, S, "softening")
        dt = _per_scene(self.dt, S, "dt")
        extra = self._fmt.extra_params(self)
        key = (tuple(g), tuple(eps), tuple(dt)) + tuple(tuple(x) for x in extra)
        if key != self._params_key:
            self._fmt.write_params(self, g, eps, dt, *extra)
            self._params_key = key
        return key

    def scene(self, i: int):
        """(positions, velocities, accelerations) views of scene i."""
        if not -self.n_scenes <= i < self.n_scenes:
            raise IndexError(f"scene {i} of {self.n_scenes}")
        i %= self.n_scenes
        lo, hi = int(self.offsets[i]), int(self.offsets[i + 1])
        return self.positions[lo:hi], self.velocities[lo:hi], self.accelerations[lo:hi]

    # ------------------------------------------------------------------ force, energies, step
    def compute_accelerations(self) -> torch.Tensor:
        """Force of every scene on its own bodies -> new (N_total, 3) tensor (simulation.py:71-89 per scene)."""
        self._sync_params()
        return self._fmt.accel(self)

    def compute_accelerations_and_jerks(self):
        """(a, j) of every scene's current state as new (N_total, 3) tensors (HermiteSimulator's per scene)."""
        self._sync_params()
        acc = torch.zeros((self.n, 3), dtype=self._fmt.dtype, device=self.device)
        jerk = torch.zeros((self.n, 3), dtype=self._fmt.dtype, device=self.device)
        self._fmt.accel_jerk(self, acc, jerk)
        return acc, jerk

    def compute_accelerations_jerks_and_snaps(self):
        """(a, j, s) of every scene's current state as new (N_total, 3) float64 tensors, in Hermite6Simulator's two
        passes per scene (integrator="hermite6" only)."""
        if not self._order6:
            raise ValueError("BatchedSimulator.compute_accelerations_jerks_and_snaps(): integrator='hermite6' (or "
                             "'block_hermite6') only")
        self._sync_params()
        acc, jerk, snap = (torch.zeros((self.n, 3), dtype=torch.float64, device=self.device) for _ in range(3))
        self._fmt.accel_jerk_snap(self, acc, jerk, snap)
        return acc, jerk, snap

    def _check_integrator(self):
        if self._fmt.block or self.integrator in _BATCH_BLOCK_INTEGRATORS:
            if self.integrator != self._built_as:
                raise ValueError("BatchedSimulator: the integrator cannot change into, out of or between the block "
                                 "modes after construction (their schedule state, plan and tables are their own); "
                                 "build a new simulator")
            return
        if (self.integrator == "hermite6") != self._order6:
            raise ValueError("BatchedSimulator: the integrator cannot change into or out of 'hermite6' after "
                             "construction (the state carries snaps and crackles only for the 6th-order scheme, and "
                             "its plan and parameter table are its own); build a new simulator")
        if (self.integrator == "hermite") != (self._hermite and not self._order6):
            raise ValueError("BatchedSimulator: the integrator cannot change into or out of 'hermite' after "
                             "construction (the state carries jerks only for Hermite); build a new simulator")

    def _energies_into(self, out_uk):
        self._fmt.energies(self, out_uk)

    def compute_energies(self):
        """(u, k): two lists of S Python floats (simulation.py:91-115 per scene)."""
        self._sync_params()
        self._fmt.pack(self)
        uk = torch.empty((self.n_scenes, 2), dtype=torch.float64, device=self.device)
        self._energies_into(uk)
        uk = uk.cpu()
        return uk[:, 0].tolist(), uk[:, 1].tolist()

    # ------------------------------------------------------------------ consistent-potential diagnostics
    def _potentials_into(self, phi):
        """phi (N_total,) float64 from the packed sources (already packed, parameters in sync), asynchronous."""
        return self._fmt.potentials(self, phi)

    def _invariants_into(self, out_rows):
        """(S, 16) invariant rows of the state a step left (packed sources = its positions), asynchronous."""
        if self._phi is None:
            self._phi = torch.zeros((self.n,), dtype=torch.float64, device=self.device)
        self._potentials_into(self._phi)
        self._fmt.invariants(self, self._phi, out_rows)

    def compute_potentials(self) -> torch.Tensor:
        """Every body's potential under the bodies of its own scene, with the scene's softening and g_const -> new
        (N_total,) float64 device tensor in scene order (BaseSimulator.compute_potentials per scene, bit for bit)."""
        self._sync_params()
        self._fmt.pack(self)
        return self._potentials_into(torch.zeros((self.n,), dtype=torch.float64, device=self.device))

    def compute_invariants(self) -> list:
        """One Invariants per scene (BaseSimulator.compute_invariants per scene, bit for bit; zeros for an empty scene)."""
        phi = self.compute_potentials()
        rows = torch.zeros((self.n_scenes, direct.INVARIANT_ROW), dtype=torch.float64, device=self.device)
        self._fmt.invariants(self, phi, rows)
        return [Invariants.from_row(r) for r in rows.cpu().tolist()]

    def _step_into(self, cur, new):
        """One step from the carried arrays `cur` into `new` (lists in the order of `_carried`; may be the same)."""
        P = self._params
        if self._hermite:
            self._fmt.hermite_step(self, cur, new)
        elif self.integrator == "leapfrog":
            direct.batch_leapfrog_step(self._plan, self.positions, self.velocities, cur[0], new[0], self.masses,
                                       P[3], P[4], P[1], P[0], self._posm, self._ws)
        else:
            direct.batch_euler_step(self._plan, self.positions, self.velocities, new[0], self.masses, P[4], P[1],
                                    P[0], self._posm, self._ws)

    def step(self):
        """One step of every scene; positions and velocities in place, `accelerations` (for Hermite `jerks`, for the
        6th-order scheme `snaps` and `crackles` as well) rebound to new tensors. The block modes advance every scene by its
        own dt in ensemble block steps and update the carried arrays in place."""
        self._check_integrator()
        if self.n == 0:
            return
        self._sync_params()
        self._fmt.advance(self)

    # ------------------------------------------------------------------ run()
    def _chunk_len(self) -> int:
        return max(1, min(self.GRAPH_RUN_CHUNK, self.RING_BYTES // max(9 * self._fmt.dtype.itemsize * self.n, 1)))

    def run(self, steps: int) -> list[list[SimulationState]]:
        """Run `steps` steps of every scene: S lists of reference-shaped SimulationState (simulation.py:117-146).
        step_time is the GPU time of the batched step divided by S. Chunks of >= 8 steps replay a captured hipGraph
        (the steps, the energies and one snapshot launch per step; one device->host copy per chunk); the last < 8 steps
        run eagerly -- the same launches in the same order, so the states are bit-identical either way."""
        out = [[] for _ in range(self.n_scenes)]
        if steps <= 0:
            return out
        self._check_integrator()
        if self.n == 0:
            uk = (0.0, 0.0) if self.calc_energy else (None, None)
            empty = torch.zeros((0, 3), dtype=self._fmt.dtype)
            for i in range(self.n_scenes):
                out[i] = [SimulationState(step=s, step_time=0.0, positions=empty, velocities=empty, accelerations=empty,
                                          u_energy=uk[0], k_energy=uk[1],
                                          invariants=(Invariants.from_row([0.0] * direct.INVARIANT_ROW)
                                                      if self.calc_invariants else None)) for s in range(steps)]
            return out
        self._sync_params()
        big = self._chunk_len()
        if big >= 8 and self._fmt.capturable and os.environ.get("NBD_RUN_GRAPH", "1") != "0":
            self._run_chunked(steps, big, out)
        else:
            self._run_eager(steps, 0, out)
        return out

    def _chunk_buffers(self, m: int):
        """One device buffer = ring | energies (_batch_chunk_layout): ONE device->host copy per chunk."""
        size = _batch_chunk_layout(m, self.n, self.n_scenes, self._fmt.dtype)[2]
        buf = torch.empty(size, dtype=torch.uint8, device=self.device)
        return (buf,) + _batch_chunk_views(buf, m, self.n, self.n_scenes, self._fmt.dtype)

    def _inv_buffer(self, m: int):
        """The chunk's invariant rows (m, S, 16), a second device buffer next to ring | energies; None without the flag."""
        if not self.calc_invariants:
            return None
        return torch.zeros((m, self.n_scenes, direct.INVARIANT_ROW), dtype=torch.float64, device=self.device)

    def _emit_states(self, host, m, first, t_steps, out):
        _batch_states(host[0], m, self.offsets.tolist(), self.calc_energy, first,
                      [t / self.n_scenes for t in t_steps], out,       # the batched step's GPU time, spread over S
                      inv=host[1] if self.calc_invariants else None, dtype=self._fmt.dtype)

    def _run_eager(self, steps: int, first: int, out):
        done = 0
        while done < steps:
            m = min(self._chunk_len(), steps - done)
            buf, ring, uk = self._chunk_buffers(m)
            inv = self._inv_buffer(m)
            events = []
            for s_ in range(m):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                self.step()
                e1.record()
                events.append((e0, e1))
                if self.calc_energy:
                    self._energies_into(uk[s_])
                if inv is not None:
                    self._invariants_into(inv[s_])
                self._fmt.snapshot(self.positions, self.velocities, self.accelerations, ring[s_])
            host = [buf.cpu()] + ([inv.cpu()] if inv is not None else [])
            self._emit_states(host, m, first + done, [a.elapsed_time(b) * 1e-3 for a, b in events], out)
            done += m

    def _chunk_scalars(self):
        return (self._params_key, bool(self.calc_energy), self.integrator, bool(self.calc_invariants))

    def _chunk_body(self, m: int):
        buf, ring, uk = self._chunk_buffers(m)
        inv = self._inv_buffer(m)
        statics = self._statics()

        def body(count):
            for s_ in range(count):
                self._step_into(statics, statics)
                if self.calc_energy:
                    self._energies_into(uk[s_])
                if inv is not None:
                    self._invariants_into(inv[s_])
                self._fmt.snapshot(self.positions, self.velocities, statics[0], ring[s_])
        return body, (buf,) + ((inv,) if inv is not None else ())
