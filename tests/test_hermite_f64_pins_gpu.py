"""The shared-step float64 Hermite units on the MI355X, pinned to recorded bits: SHA-256 digests of the output bytes of
HermiteSimulator(dtype=torch.float64) and Hermite6Simulator -- the force on its own and the state after two steps --
recorded once by tests/golden/make_hermite_f64_pins.py (tests/golden/hermite_f64_pins.json; digests only) and recomputed
here with the tree's own library. A BatchedSimulator of either order must give each of its scenes the lone simulator's
digests, so the fixture has no batched entries. No oracle runs: a case is a few launches.

The inputs are a closed-form integer recipe (no random generator): body i sits at the lattice point (i % 32, i // 32 % 32,
i // 1024) plus a jitter below 2^-8 per coordinate, a 32-bit hash of (i, coordinate) with its top and bottom bits set,
scaled by 2^-40 -- so no two bodies coincide and every coordinate has 32 to 45 significant bits: exact in fp64, not
fp32-representable. Velocities are centred hashes scaled by 2^-33; mass i is (2^32 + (a hash with its low 13 bits replaced
by i)) 2^-32 / 2^ceil(log2 n): pairwise different for n <= 8192.

The sizes are the smallest at which the pair kernels' geometry differs (hermite_f64_kernels.h: groups of 64 targets,
chunks of 64 sources, 4 waves per workgroup, slabs = min(ceil(1024 / groups), chunks / 4, 64), at least 1):
  n = 1     one valid lane
  n = 65    two groups, the second with one lane
  n = 130   three chunks on one slab: one wave of a workgroup has none
  n = 513   9 chunks: the first size with two slabs (9 // 4) and an uneven split (8 waves: one walks two chunks), one lane
            in the last group
  n = 8192  128 chunks on 8 slabs: the first size where every wave walks 4 chunks, so the double buffer wraps
each at eps = 0.01 and at eps = 0 (every chunk walked index-masked)."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F64 = torch.float64
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hermite_f64_pins.json")
SIZES = (1, 65, 130, 513, 8192)
SOFTENINGS = (0.01, 0.0)
ORDERS = (4, 6)
G, DT, STEPS = 1.0, 2.0 ** -7, 2
BATCH = ((65, 0.01), (0, 0.01), (513, 0.0), (1, 0.0), (130, 0.01))       # (scene size, softening)
STATE = {4: ("positions", "velocities", "accelerations", "jerks"),
         6: ("positions", "velocities", "accelerations", "jerks", "snaps", "crackles")}
FORCE = {4: ("accelerations", "jerks"), 6: ("accelerations", "jerks", "snaps")}


def _hash32(k):
    """A 32-bit mix of the integers k (an int64 array): multiply, then the xor-shift-multiply rounds of a finaliser, all
    in uint64 arithmetic masked to 32 bits."""
    m = np.uint64(0xFFFFFFFF)
    x = (k.astype(np.uint64) * np.uint64(2654435761) + np.uint64(0x9E3779B9)) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & m
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & m
    x ^= x >> np.uint64(16)
    return x.astype(np.int64)


@functools.lru_cache(maxsize=None)
def inputs(n):
    """(positions (n, 3), velocities (n, 3), masses (n,)) of the recipe above, float64, read-only."""
    assert 0 <= n <= 8192
    i = np.arange(n, dtype=np.int64)
    lattice = np.stack([i % 32, i // 32 % 32, i // 1024], axis=1)
    h = _hash32(i[:, None] * 7 + np.arange(7)[None, :])
    pos = np.ldexp((lattice * 2 ** 40 + (h[:, 0:3] | 0x80000001)).astype(np.float64), -40)
    vel = np.ldexp(((h[:, 3:6] | 1) - 2 ** 31).astype(np.float64), -33)
    mass = np.ldexp((2 ** 32 + (h[:, 6] >> 13 << 13) + i).astype(np.float64), -32 - max(n - 1, 0).bit_length())
    assert np.all(pos.astype(np.float32).astype(np.float64) != pos) and len(set(mass.tolist())) == n
    assert len({tuple(r) for r in lattice.tolist()}) == n
    for a in (pos, vel, mass):
        a.setflags(write=False)
    return pos, vel, mass


def _digest(t):
    a = t.detach().cpu().contiguous().numpy()
    assert a.dtype == np.float64
    return hashlib.sha256(a.tobytes()).hexdigest()


def _nan_fill(sim):
    """NaN into everything a call may only write before it reads: the partial sums and the packed rows."""
    for name in ("_ws", "_hws", "_posd", "_veld", "_accd"):
        t = getattr(sim, name, None)
        if t is not None:
            t.view(F64).fill_(float("nan"))


def _force(sim, order):
    _nan_fill(sim)
    return (sim.compute_accelerations_and_jerks() if order == 4 else sim.compute_accelerations_jerks_and_snaps())


def _steps(sim):
    for _ in range(STEPS):
        _nan_fill(sim)
        sim.step()


def key(order, n, eps):
    return f"order{order}/n{n}/eps{eps!r}"


def lone_digests(order, n, eps):
    """{"force/<array>": digest, "steps/<array>": digest} of the lone simulator of `order` on inputs(n)."""
    from galaxify import simulation
    pos, vel, mass = inputs(n)
    kw = dict(positions=pos, velocities=vel, masses=mass, g_const=G, softening=eps, dt=DT, calc_energy=False,
              device="cuda")
    sim = simulation.HermiteSimulator(dtype=F64, **kw) if order == 4 else simulation.Hermite6Simulator(**kw)
    out = {"force/" + nm: _digest(t) for nm, t in zip(FORCE[order], _force(sim, order))}
    _steps(sim)
    out.update({"steps/" + nm: _digest(getattr(sim, nm)) for nm in STATE[order]})
    return out


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(FIXTURE) as f:
        return json.load(f)["digests"]


@pytest.mark.parametrize("eps", SOFTENINGS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("order", ORDERS)
def test_lone_simulator_has_the_recorded_bits(gpu_device, order, n, eps):
    got, want = lone_digests(order, n, eps), _recorded()[key(order, n, eps)]
    assert sorted(got) == sorted(want)
    assert got == want, sorted(k for k in got if got[k] != want[k])


@pytest.mark.parametrize("order", ORDERS)
def test_every_scene_of_a_batch_has_the_lone_simulators_recorded_bits(gpu_device, order):
    from galaxify import simulation
    kw = dict(integrator="hermite", dtype=F64) if order == 4 else dict(integrator="hermite6")
    sim = simulation.BatchedSimulator(systems=[inputs(n) for n, _ in BATCH], g_const=[G] * len(BATCH),
                                      softening=[eps for _, eps in BATCH], dt=[DT] * len(BATCH), calc_energy=False,
                                      device="cuda", **kw)
    force = _force(sim, order)
    _steps(sim)
    for s, (n, eps) in enumerate(BATCH):
        lo, hi = int(sim.offsets[s]), int(sim.offsets[s + 1])
        assert hi - lo == n
        if n == 0:
            continue
        got = {"force/" + nm: _digest(t[lo:hi]) for nm, t in zip(FORCE[order], force)}
        got.update({"steps/" + nm: _digest(getattr(sim, nm)[lo:hi]) for nm in STATE[order]})
        want = _recorded()[key(order, n, eps)]
        assert got == want, (s, n, eps, sorted(k for k in got if got[k] != want.get(k)))
