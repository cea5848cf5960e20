"""BlockTreeLeapFrogSimulator next to TreeLeapFrogSimulator on the MI355X, in one process.

  python tools/bench_tree_block.py [--out FILE] [--sizes N ...]          (default: profiles/r32_tree_block.json)

Per N (Plummer sphere, theta = 0.5, eps = 0.1, G = 1, quadrupoles on), over one time unit (1 / dt output intervals):
  block     BlockTreeLeapFrogSimulator(dt, eta, max_level): the level histogram at the end, the deepest level any body
            had at the end of an interval, block_steps, active_targets, clamped, and the walk's terms summed over the
            block steps of the last round (cells + 8 x level-0 nodes, per 64 targets of a group: x 64)
  shared    TreeLeapFrogSimulator at the shared step dt 2^-deepest: what the block run's smallest step costs when every
            body takes it; its terms per time unit
  ms        GPU time per time unit of both (HIP events around the step() calls), in alternating rounds; the median
  energy    |E(1) - E(0)| / |E(0)|, E = K + 1/2 sum m phi_tree (compute_invariants() with potential="tree"), for both
  floor     what a block step costs outside its walk, measured at n_act = 1: drift + build + flag + select + readback,
            and the walk of that one body
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-deep-sim_amd"))

from galaxify import simulation  # noqa: E402
from nbd import tree  # noqa: E402
from nbd.plummer import generate_plummer  # noqa: E402

THETA, EPS, DT, ETA, MAX_LEVEL, ROUNDS = 0.5, 0.1, 0.5, 0.025, 6, 3


def _sim(cls, arrays, dt, **kw):
    p, v, m = arrays
    return cls(positions=p, velocities=v, masses=m, g_const=1.0, softening=EPS, dt=dt, calc_energy=False, device="cuda",
               theta=THETA, potential="tree", **kw)


def _unit(sim, steps):
    """GPU ms of `steps` step() calls (the counters are summed in a round of their own: reading them synchronises)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        sim.step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _terms_shared(sim, steps):
    total = 0
    for _ in range(steps):
        sim.step()
        c, l = sim.tree_counters()
        total += (c + 8 * l) * 64
    return total


def _terms_block(sim, steps):
    """Sum of (cells + 8 leaves) x 64 over every block step: level_history's hook is the one place step() calls back."""
    total = [0]

    class Hook(list):
        def append(self, item):
            c, l = sim.tree_counters()
            total[0] += (c + 8 * l) * 64
    sim.level_history = Hook()
    for _ in range(steps):
        sim.step()
    sim.level_history = None
    return total[0]


def _floor(arrays, reps=20):
    """One block step at n_act = 1: every body at level 0 but one at MAX_LEVEL."""
    sim = _sim(simulation.BlockTreeLeapFrogSimulator, arrays, DT, eta=ETA, max_level=MAX_LEVEL)
    n, K = sim.n, MAX_LEVEL
    host = sim._sched_host
    around, walk = [], []
    for _ in range(reps):
        sim.levels.zero_()
        sim.levels[0] = K
        tree.block_open(sim.velocities, sim.accelerations, sim.levels, sim._ticks, sim._residual, K, sim.dt, sim._sched)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        tree.block_drift(sim.positions, sim.velocities, sim.masses, sim.levels, sim._ticks, sim._residual, K, sim.dt,
                         sim._sched, sim._posm)
        tree.build_posm(sim._posm, n, sim._tree_ws, sim._order)
        tree.block_flag(sim.levels, sim._ticks, K, sim._sched, sim._flags)
        tree.select_active(sim._tree_ws, n, sim._flags, sim._act_list, active_ws=sim._act_ws, n_act_out=sim._sched[1:2])
        host.copy_(sim._sched)
        ev[1].record()
        assert int(host[1]) == 1 and int(host[0]) == 1, host.tolist()
        tree.accel_active(sim._tree_ws, n, sim._act_list, 1, THETA, EPS * EPS, 1.0, True, out=sim.accelerations,
                          counters=sim._counters)
        ev[2].record()
        torch.cuda.synchronize()
        around.append(ev[0].elapsed_time(ev[1])); walk.append(ev[1].elapsed_time(ev[2]))
    return {"drift_build_select_readback_ms": float(np.median(around)), "walk_one_body_ms": float(np.median(walk))}


def bench(n):
    arrays = tuple(np.asarray(t, dtype=np.float32) for t in generate_plummer(n, seed=1))
    intervals = int(round(1.0 / DT))
    rec = {"n": n, "theta": THETA, "eps": EPS, "dt": DT, "eta": ETA, "max_level": MAX_LEVEL, "intervals": intervals}
    # a first block run finds the deepest populated level
    probe = _sim(simulation.BlockTreeLeapFrogSimulator, arrays, DT, eta=ETA, max_level=MAX_LEVEL)
    deepest = int(probe.levels.max())
    for _ in range(intervals):
        probe.step()
        deepest = max(deepest, int(probe.levels.max()))
    h = DT * 2.0 ** -deepest
    shared_steps = intervals << deepest
    rec["deepest_level"] = deepest
    rec["shared_dt"] = h
    block_ms, shared_ms = [], []
    for r in range(ROUNDS):
        block = _sim(simulation.BlockTreeLeapFrogSimulator, arrays, DT, eta=ETA, max_level=MAX_LEVEL)
        shared = _sim(simulation.TreeLeapFrogSimulator, arrays, h)
        if r == 0:
            e_block0, e_shared0 = block.compute_invariants().energy, shared.compute_invariants().energy
        block_ms.append(_unit(block, intervals))
        shared_ms.append(_unit(shared, shared_steps))
    rec["block"] = {
        "ms_per_time_unit": float(np.median(block_ms)), "ms_rounds": block_ms,
        "level_histogram": np.bincount(block.levels.cpu().numpy(), minlength=MAX_LEVEL + 1).tolist(),
        "block_steps": block.block_steps, "active_targets": block.active_targets, "clamped": block.clamped,
        "mean_active_fraction": block.active_targets / (block.block_steps * n),
        "energy_drift": abs(block.compute_invariants().energy - e_block0) / abs(e_block0)}
    rec["shared"] = {
        "ms_per_time_unit": float(np.median(shared_ms)), "ms_rounds": shared_ms, "steps": shared_steps,
        "energy_drift": abs(shared.compute_invariants().energy - e_shared0) / abs(e_shared0)}
    rec["block"]["ms_per_dt"] = rec["block"]["ms_per_time_unit"] / intervals
    rec["shared"]["ms_per_dt"] = rec["shared"]["ms_per_time_unit"] / intervals
    rec["block_over_shared"] = rec["block"]["ms_per_time_unit"] / rec["shared"]["ms_per_time_unit"]
    # the walk's terms, in a round of their own (the counter reads synchronise)
    rec["block"]["terms"] = _terms_block(_sim(simulation.BlockTreeLeapFrogSimulator, arrays, DT, eta=ETA,
                                              max_level=MAX_LEVEL), intervals)
    rec["shared"]["terms"] = _terms_shared(_sim(simulation.TreeLeapFrogSimulator, arrays, h), shared_steps)
    rec["terms_block_over_shared"] = rec["block"]["terms"] / rec["shared"]["terms"]
    rec["floor"] = _floor(arrays)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32_tree_block.json"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 262144, 524288])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    out = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "sizes": []}
    for n in args.sizes:
        rec = bench(n)
        out["sizes"].append(rec)
        print(json.dumps(rec), flush=True)
        with open(args.out, "w") as f:                  # (after every size: a long run leaves what it finished)
            json.dump(out, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
