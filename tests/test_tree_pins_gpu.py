"""The tree code on the MI355X, pinned to recorded bits: SHA-256 digests of what every walk of nbd.tree -- all groups, a
range of groups, listed targets; a, phi and both -- and the two tree simulators leave, recorded once by
tests/golden/make_tree_pins.py (tests/golden/tree_pins.json; digests only) and recomputed here with the tree's own
library. The other tree tests compare one path of a build with another path of the same build or with an fp64 oracle
within a tolerance; these compare a build with an earlier one, to the bit. Only public names are used: nbd.tree's
wrappers and the simulators. No oracle runs: the module is a few dozen launches.

The inputs are test_hermite_f64_pins_gpu.inputs(n) (a closed-form integer recipe: no random generator, no libm) rounded
to float32, with softening 0.1 and G = 1. Every output is pre-filled with a sentinel, so the rows a walk must leave
unwritten are pinned with the rows it writes.

The sizes are the smallest at which the walk's geometry differs (csrc/tree_force.hip: level-0 nodes of 8 bodies, target
groups of 64, 8 waves share a group once a level has 64 nodes):
  n = 65    two groups, the second holds one body; one wave per group
  n = 300   38 level-0 nodes: one wave per group, a ragged last group
  n = 1000  125 level-0 nodes: 8 waves share a group at level 0; 16 groups, the last holds 40 bodies
  n = 5000  79 level-1 nodes: the waves divide the tree at level 1
each at theta = 0.5 with and without the quadrupole term; n = 300 at theta = 0 (every node opened) as well."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from test_hermite_f64_pins_gpu import inputs

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_pins.json")
SIZES = (65, 300, 1000, 5000)
CASES = [(n, 0.5, quad) for n in SIZES for quad in (True, False)] + [(300, 0.0, True)]      # (n, theta, quadrupole)
SOFTENING, G = 0.1, 1.0
EPS2 = SOFTENING * SOFTENING
SENTINEL = -12345.0
SIM_N, SIM_DT, SIM_STEPS = 300, 2.0 ** -4, 2
BLOCK_DT, BLOCK_MAX_LEVEL = 4.0, 3            # the criterion puts these bodies on all four levels at this interval


def _digest(*tensors):
    """One digest of the bytes of several tensors or arrays, each behind its dtype and shape."""
    h = hashlib.sha256()
    for t in tensors:
        a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
        h.update(f"{a.dtype}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def arrays(n):
    """(positions, velocities, masses) of inputs(n), rounded to float32."""
    return tuple(a.astype(np.float32) for a in inputs(n))


def _acc(rows):
    return torch.full((rows, 3), SENTINEL, dtype=torch.float32, device="cuda")


def _phi(rows):
    return torch.full((rows,), SENTINEL, dtype=torch.float64, device="cuda")


def _counters():
    return torch.full((2,), -1, dtype=torch.int64, device="cuda")


def key(n, theta, quadrupole):
    return f"n{n}/theta{theta!r}/quad{int(quadrupole)}"


def walk_digests(n, theta, quadrupole):
    """{name: digest} of the order and of every walk over the tree of arrays(n)."""
    from nbd import tree
    pos, _, mass = arrays(n)
    ws = tree.workspace(n, "cuda")
    order = tree.build(torch.tensor(pos).cuda(), torch.tensor(mass).cuda(), ws)
    walk = (theta, EPS2, G, quadrupole)
    out = {"order": _digest(order)}

    a, c = _acc(n), _counters()
    tree.accel(ws, n, *walk, out=a, counters=c)
    out["accel"] = _digest(a, c)
    p, c = _phi(n), _counters()
    tree.potential(ws, n, *walk, out=p, counters=c)
    out["potential"] = _digest(p, c)
    a, p, c = _acc(n), _phi(n), _counters()
    tree.accel_potential(ws, n, *walk, out=(a, p), counters=c)
    out["accel_potential"] = _digest(a, p, c)

    groups = tree.groups(n)
    ranges = {"middle": (groups // 3, groups - groups // 3),       # the middle third of the groups
              "last": (groups - 1, groups)}                        # the ragged group: its rows behind body n - 1 are 0
    for name, (lo, hi) in ranges.items():
        rows = (hi - lo) * tree.GROUP
        a, c = _acc(rows), _counters()
        tree.accel_groups(ws, n, lo, hi, *walk, out=a, counters=c)
        out[f"accel_groups/{name}"] = _digest(a, c)
        p, c = _phi(rows), _counters()
        tree.potential_groups(ws, n, lo, hi, *walk, out=p, counters=c)
        out[f"potential_groups/{name}"] = _digest(p, c)
        a, p, c = _acc(rows), _phi(rows), _counters()
        tree.accel_potential_groups(ws, n, lo, hi, *walk, out=(a, p), counters=c)
        out[f"accel_potential_groups/{name}"] = _digest(a, p, c)

    flags = torch.zeros(n, dtype=torch.int32, device="cuda")
    flags[order[::3].long()] = 1                                   # every third sorted position
    lst, n_act_dev = tree.select_active(ws, n, flags)
    n_act = int(n_act_dev.item())
    assert n_act == (n + 2) // 3
    out["select_active"] = _digest(lst[:n_act], n_act_dev)
    a, c = _acc(n), _counters()
    tree.accel_active(ws, n, lst, n_act, *walk, out=a, counters=c)
    out["accel_active"] = _digest(a, c)
    return out


def _sim_kw(dt):
    pos, vel, mass = arrays(SIM_N)
    return dict(positions=pos, velocities=vel, masses=mass, g_const=G, softening=SOFTENING, dt=dt, calc_energy=False,
                device="cuda")


def leapfrog_digests():
    """The state after two steps of the tree leapfrog whose steps take a and phi from one walk, and the invariants row."""
    from galaxify import simulation
    sim = simulation.TreeLeapFrogSimulator(potential="tree", calc_invariants=True, **_sim_kw(SIM_DT))
    states = sim.run(SIM_STEPS)
    out = {name: _digest(getattr(sim, name)) for name in ("positions", "velocities", "accelerations")}
    out["invariants"] = _digest(np.array(states[-1].invariants.row(), dtype=np.float64))
    return out


def block_digests():
    """The state and the levels after one output interval of the block-timestep tree leapfrog."""
    from galaxify import simulation
    sim = simulation.BlockTreeLeapFrogSimulator(max_level=BLOCK_MAX_LEVEL, **_sim_kw(BLOCK_DT))
    sim.step()
    assert sim.active_targets < sim.block_steps * SIM_N            # some block steps walked a list
    return {name: _digest(getattr(sim, name)) for name in ("positions", "velocities", "accelerations", "levels")}


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(FIXTURE) as f:
        return json.load(f)["digests"]


def _check(got, want):
    assert sorted(got) == sorted(want)
    assert got == want, sorted(k for k in got if got[k] != want[k])


@pytest.mark.parametrize("n, theta, quadrupole", CASES)
def test_every_walk_has_the_recorded_bits(gpu_device, n, theta, quadrupole):
    _check(walk_digests(n, theta, quadrupole), _recorded()[key(n, theta, quadrupole)])


def test_tree_leapfrog_has_the_recorded_bits(gpu_device):
    _check(leapfrog_digests(), _recorded()["leapfrog"])


def test_block_tree_leapfrog_has_the_recorded_bits(gpu_device):
    _check(block_digests(), _recorded()["block"])
