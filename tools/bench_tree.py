"""The tree force (csrc/tree_force.hip) next to the all-pairs kernel on the MI355X, in one process.

  python tools/bench_tree.py [--out FILE] [--sizes N ...]          (default: profiles/r28_tree.json)

Per N (Plummer sphere, eps = 0.1, G = 1, quadrupoles on) and theta in {0.5, 0.75}:
  build_ms    nbd_tree_build_f32: bounding box, Morton keys, radix sort, gather, every node
  walk_ms     nbd_tree_accel_f32 with the counters
  direct_ms   nbd_accel_f32 on the same bodies (packed once, outside the window)
  counters    accepted cells and rejected level-0 nodes over all target groups, and what they come to per body:
              interactions_per_body = (cells + 8 x level-0 nodes) x 64 / n against the n of the direct sum
  row errors  256 sampled rows of the tree force, and of nbd_accel_f32, against float64 all-pairs rows (torch on the
              device: a reference, not a product path), measured like conftest.row_rel
Times are HIP events around `reps` calls; the three are measured in alternating rounds and the median round is kept.

  python tools/bench_tree.py --potential [--out FILE] [--sizes N ...]     (default: profiles/r30_tree_potential.json)

The tree potential next to the all-pairs potential of csrc/direct_diag.hip, same inputs, same alternating rounds:
  build_ms, walk_ms, direct_ms   as above
  phi_walk_ms, fused_walk_ms     nbd_tree_potential_f32 and nbd_tree_accel_potential_f32 with the counters
  direct_phi_ms                  nbd_potential_f32 on the same bodies
  fused_over_walk                (a) what phi costs a force walk
  tree_phi_over_direct_phi       (b) (build + phi-only walk) / all-pairs potential
  run_step_ms                    (c) TreeLeapFrogSimulator.run() per step with calc_invariants=True, calc_energy=False,
                                 potential="tree" and "direct" (HIP events around run(4), host copies of the states included)
  phi_row_error                  256 sampled rows of the tree phi, and of nbd_potential_f32, against float64 all-pairs rows:
                                 |phi - ref| / |ref|
  u_rel_diff                     |U_tree - U_direct| / |U_direct|, U = 1/2 sum m phi in float64 from the two device phi

  python tools/bench_tree.py --ranks [--out FILE] [--sizes N ...] [--worlds W ...]   (default: profiles/r31_tree_ranks.json)

The range-sharded tree force with its ranks EMULATED on one GPU (N = 262 144 and 524 288, theta = 0.5, world 2, 4, 8):
  full_walk_ms                   nbd_tree_accel_f32 with the counters
  build_ms, build_posm_ms        nbd_tree_build_f32 and nbd_tree_build_posm_f32 (every rank runs the latter on all bodies)
  scatter_ms                     nbd_tree_scatter_f32 of rank 0's bodies from the rows of all groups
  per rank                       the groups [lo, hi) of RangePartition(groups, world, rank), walk_ms of
                                 nbd_tree_accel_groups_f32 over them alone on the otherwise idle GPU, its counters
  balance                        slowest rank's walk_ms / (full_walk_ms / world): the partition balances the number of
                                 groups, not their cost
No collective runs here: the all-gather and exchange times of a real group are TreeLeapFrogSimulator.step_phases().
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-deep-sim_amd"))

from nbd import direct, tree  # noqa: E402
from nbd.plummer import generate_plummer  # noqa: E402

EPS, ROUNDS, SAMPLED = 0.1, 5, 256


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _f64_rows(pos, mass, rows, eps2):
    """float64 all-pairs accelerations of the sampled rows (G = 1), 16 rows at a time."""
    p, m = pos.double(), mass.double()
    out = torch.empty((len(rows), 3), dtype=torch.float64, device=pos.device)
    for k in range(0, len(rows), 16):
        r = rows[k:k + 16]
        d = p[None, :, :] - p[r][:, None, :]
        w = ((d * d).sum(2) + eps2) ** -1.5
        w[torch.arange(len(r), device=pos.device), r] = 0.0
        out[k:k + 16] = ((m[None, :] * w)[:, :, None] * d).sum(1)
    return out.cpu().numpy()


def _row_errors(a, ref):
    nrm = np.linalg.norm(ref, axis=1)
    floor = 1e-3 * np.sqrt((nrm ** 2).mean())
    e = np.linalg.norm(a - ref, axis=1) / np.maximum(nrm, floor)
    return {"max": float(e.max()), "rms": float(np.sqrt((e ** 2).mean()))}


def _f64_phi_rows(pos, mass, rows, eps2):
    """float64 all-pairs potentials of the sampled rows (G = 1), 16 rows at a time."""
    p, m = pos.double(), mass.double()
    out = torch.empty((len(rows),), dtype=torch.float64, device=pos.device)
    for k in range(0, len(rows), 16):
        r = rows[k:k + 16]
        d = p[None, :, :] - p[r][:, None, :]
        w = ((d * d).sum(2) + eps2) ** -0.5
        w[torch.arange(len(r), device=pos.device), r] = 0.0
        out[k:k + 16] = -(m[None, :] * w).sum(1)
    return out.cpu().numpy()


def _phi_errors(phi, ref):
    e = np.abs(phi - ref) / np.abs(ref)
    return {"max": float(e.max()), "rms": float(np.sqrt((e ** 2).mean()))}


def _run_step_ms(p, m, theta, potential, steps=4):
    """Per step of run(steps) with the invariants on, after one warm-up run (staging buffers, first launches)."""
    from galaxify import simulation
    v = np.zeros_like(p)
    sim = simulation.TreeLeapFrogSimulator(positions=p, velocities=v, masses=m, g_const=1.0, softening=EPS, dt=1e-3,
                                           calc_energy=False, calc_invariants=True, device="cuda", theta=theta,
                                           potential=potential)
    sim.run(2)
    return _timed(lambda: sim.run(steps), 1) / steps


def potential_case(n, thetas):
    p, _, m = generate_plummer(n, seed=1)
    p, m = np.asarray(p, np.float32), np.asarray(m, np.float32)
    dev = torch.device("cuda", torch.cuda.current_device())
    pos, mass = torch.tensor(p, device=dev), torch.tensor(m, device=dev)
    eps2 = direct.f32(EPS ** 2)
    posm = direct.pack_posm(pos, mass)
    dws = direct.accel_workspace(n, n, dev)
    pws = direct.potential_workspace(n, n, dev)
    dacc = torch.empty((n, 3), dtype=torch.float32, device=dev)
    dphi = torch.empty((n,), dtype=torch.float64, device=dev)
    tws = tree.workspace(n, dev)
    order = torch.empty((n,), dtype=torch.int32, device=dev)
    tacc = torch.empty((n, 3), dtype=torch.float32, device=dev)
    tphi = torch.empty((n,), dtype=torch.float64, device=dev)
    counters = torch.zeros((2,), dtype=torch.int64, device=dev)
    rows = torch.tensor(np.random.default_rng(0).choice(n, min(SAMPLED, n), replace=False), device=dev)
    ref = _f64_phi_rows(pos, mass, rows, float(eps2))

    runs = {"direct_ms": lambda: direct.accel(posm, n, posm, n, 0, eps2, 1.0, out=dacc, workspace=dws),
            "direct_phi_ms": lambda: direct.potential(posm, n, posm, n, 0, eps2, 1.0, out=dphi, workspace=pws),
            "build_ms": lambda: tree.build(pos, mass, tws, order)}
    reps_direct = max(2, min(50, int(4e10 / n / n)))
    reps_tree = max(5, min(50, int(4e6 / n) * 5))
    res = {"n": n, "plan": tree.plan(n), "workspace_bytes": tree.workspace_bytes(n), "reps_direct": reps_direct,
           "reps_tree": reps_tree, "thetas": []}
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    res["direct_phi_row_error"] = _phi_errors(dphi[rows].cpu().numpy(), ref)
    u_direct = 0.5 * float((mass.double() * dphi).sum())
    for theta in thetas:
        walk = (tws, n, theta, eps2, 1.0, True)
        runs["walk_ms"] = lambda: tree.accel(*walk, out=tacc, counters=counters)
        runs["phi_walk_ms"] = lambda: tree.potential(*walk, out=tphi, counters=counters)
        runs["fused_walk_ms"] = lambda: tree.accel_potential(*walk, out=(tacc, tphi), counters=counters)
        for key in ("walk_ms", "fused_walk_ms", "phi_walk_ms"):
            runs[key]()
        torch.cuda.synchronize()
        t = {key: [] for key in runs}
        for _ in range(ROUNDS):
            for key, fn in runs.items():
                t[key].append(_timed(fn, reps_direct if key.startswith("direct") else reps_tree))
        row = {"theta": theta}
        for key, vals in t.items():
            row[key] = float(np.median(vals))
            row[key + "_min"] = float(np.min(vals))
        row["fused_over_walk"] = row["fused_walk_ms"] / row["walk_ms"]
        row["phi_walk_over_walk"] = row["phi_walk_ms"] / row["walk_ms"]
        row["tree_phi_ms"] = row["build_ms"] + row["phi_walk_ms"]
        row["tree_phi_over_direct_phi"] = row["tree_phi_ms"] / row["direct_phi_ms"]
        cells, leaves = counters.cpu().tolist()
        row["accepted_cells"], row["rejected_level0_nodes"] = int(cells), int(leaves)
        row["phi_row_error"] = _phi_errors(tphi[rows].cpu().numpy(), ref)
        u_tree = 0.5 * float((mass.double() * tphi).sum())
        row["u_tree"], row["u_direct"] = u_tree, u_direct
        row["u_rel_diff"] = abs(u_tree - u_direct) / abs(u_direct)
        steps = {"tree": [], "direct": []}
        for which in ("tree", "direct", "tree", "direct"):
            steps[which].append(_run_step_ms(p, m, theta, which))
        row["run_step_ms"] = {which: float(np.min(vals)) for which, vals in steps.items()}
        row["run_step_ms_all"] = steps
        row["run_step_tree_over_direct"] = row["run_step_ms"]["tree"] / row["run_step_ms"]["direct"]
        res["thetas"].append(row)
        print(json.dumps({"n": n, **row}), flush=True)
    return res


def case(n, thetas):
    p, _, m = generate_plummer(n, seed=1)
    dev = torch.device("cuda", torch.cuda.current_device())
    pos = torch.tensor(np.asarray(p, np.float32), device=dev)
    mass = torch.tensor(np.asarray(m, np.float32), device=dev)
    eps2 = direct.f32(EPS ** 2)
    posm = direct.pack_posm(pos, mass)
    dws = direct.accel_workspace(n, n, dev)
    dacc = torch.empty((n, 3), dtype=torch.float32, device=dev)
    tws = tree.workspace(n, dev)
    order = torch.empty((n,), dtype=torch.int32, device=dev)
    tacc = torch.empty((n, 3), dtype=torch.float32, device=dev)
    counters = torch.zeros((2,), dtype=torch.int64, device=dev)
    rows = torch.tensor(np.random.default_rng(0).choice(n, min(SAMPLED, n), replace=False), device=dev)
    ref = _f64_rows(pos, mass, rows, float(eps2))

    def run_direct():
        direct.accel(posm, n, posm, n, 0, eps2, 1.0, out=dacc, workspace=dws)

    def run_build():
        tree.build(pos, mass, tws, order)

    reps_direct = max(2, min(50, int(4e10 / n / n)))
    reps_tree = max(5, min(50, int(4e6 / n) * 5))
    res = {"n": n, "plan": tree.plan(n), "workspace_bytes": tree.workspace_bytes(n), "reps_direct": reps_direct,
           "reps_tree": reps_tree, "thetas": []}
    run_direct(); run_build()
    torch.cuda.synchronize()
    res["direct_row_error"] = _row_errors(dacc[rows].cpu().numpy().astype(np.float64), ref)
    for theta in thetas:
        def run_walk():
            tree.accel(tws, n, theta, eps2, 1.0, True, out=tacc, counters=counters)
        run_walk()
        torch.cuda.synchronize()
        t = {"direct_ms": [], "build_ms": [], "walk_ms": []}
        for _ in range(ROUNDS):
            t["direct_ms"].append(_timed(run_direct, reps_direct))
            t["build_ms"].append(_timed(run_build, reps_tree))
            t["walk_ms"].append(_timed(run_walk, reps_tree))
        row = {"theta": theta}
        for key, vals in t.items():
            row[key] = float(np.median(vals))
            row[key + "_min"] = float(np.min(vals))
        row["tree_ms"] = row["build_ms"] + row["walk_ms"]
        row["direct_over_tree"] = row["direct_ms"] / row["tree_ms"]
        row["tree_faster_than_direct"] = bool(row["tree_ms"] < row["direct_ms"])
        cells, leaves = counters.cpu().tolist()
        row["accepted_cells"], row["rejected_level0_nodes"] = int(cells), int(leaves)
        row["interactions_per_body"] = (cells + 8 * leaves) * 64 / n
        row["tree_row_error"] = _row_errors(tacc[rows].cpu().numpy().astype(np.float64), ref)
        res["thetas"].append(row)
        print(json.dumps({"n": n, **row}), flush=True)
    return res


def ranks_case(n, theta, worlds):
    from nbd.dist import RangePartition
    p, _, m = generate_plummer(n, seed=1)
    dev = torch.device("cuda", torch.cuda.current_device())
    pos = torch.tensor(np.asarray(p, np.float32), device=dev)
    mass = torch.tensor(np.asarray(m, np.float32), device=dev)
    eps2 = direct.f32(EPS ** 2)
    posm = direct.pack_posm(pos, mass)
    tws = tree.workspace(n, dev)
    order = torch.empty((n,), dtype=torch.int32, device=dev)
    tacc = torch.empty((n, 3), dtype=torch.float32, device=dev)
    groups = tree.groups(n)
    sorted_acc = torch.zeros((groups * tree.GROUP, 3), dtype=torch.float32, device=dev)
    counters = torch.zeros((2,), dtype=torch.int64, device=dev)
    reps = max(5, min(50, int(4e6 / n) * 5))
    own = RangePartition(n, max(worlds), 0)
    own_acc = torch.empty((own.n_local, 3), dtype=torch.float32, device=dev)
    runs = {"full_walk_ms": lambda: tree.accel(tws, n, theta, eps2, 1.0, True, out=tacc, counters=counters),
            "build_ms": lambda: tree.build(pos, mass, tws, order),
            "build_posm_ms": lambda: tree.build_posm(posm, n, tws, order),
            "scatter_ms": lambda: tree.scatter(tws, n, own.lo, own.hi, sorted_acc, None, out=(own_acc, None))}
    ranges = {}
    for world in worlds:
        for rank in range(world):
            g = RangePartition(groups, world, rank)
            out = sorted_acc[g.lo * tree.GROUP:g.hi * tree.GROUP]
            ranges[(world, rank)] = (g.lo, g.hi)
            runs[f"w{world}r{rank}"] = (lambda lo=g.lo, hi=g.hi, out=out:
                                        tree.accel_groups(tws, n, lo, hi, theta, eps2, 1.0, True, out=out, counters=counters))
    runs["build_posm_ms"]()
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    t = {key: [] for key in runs}
    for _ in range(ROUNDS):
        for key, fn in runs.items():
            t[key].append(_timed(fn, reps))
    med = {key: float(np.median(vals)) for key, vals in t.items()}
    runs["full_walk_ms"]()
    full_counters = [int(c) for c in counters.cpu().tolist()]
    res = {"n": n, "theta": theta, "groups": groups, "reps": reps, "plan": tree.plan(n),
           **{key: med[key] for key in ("full_walk_ms", "build_ms", "build_posm_ms", "scatter_ms")},
           "scatter_rows": own.n_local, "accepted_cells": full_counters[0], "rejected_level0_nodes": full_counters[1],
           "worlds": []}
    for world in worlds:
        per = []
        for rank in range(world):
            runs[f"w{world}r{rank}"]()
            c = [int(x) for x in counters.cpu().tolist()]
            lo, hi = ranges[(world, rank)]
            per.append({"rank": rank, "groups": [lo, hi], "walk_ms": med[f"w{world}r{rank}"],
                        "walk_ms_min": float(np.min(t[f"w{world}r{rank}"])), "accepted_cells": c[0],
                        "rejected_level0_nodes": c[1]})
        slowest = max(r["walk_ms"] for r in per)
        row = {"world": world, "ranks": per, "slowest_walk_ms": slowest, "sum_walk_ms": sum(r["walk_ms"] for r in per),
               "balance": slowest / (med["full_walk_ms"] / world),
               "counters_sum_to_the_full_walk": [sum(r["accepted_cells"] for r in per) == full_counters[0],
                                                 sum(r["rejected_level0_nodes"] for r in per) == full_counters[1]],
               "rank_step_ms": med["build_posm_ms"] + slowest + med["scatter_ms"],
               "one_gpu_step_ms": med["build_ms"] + med["full_walk_ms"]}
        res["worlds"].append(row)
        print(json.dumps({"n": n, **{k: v for k, v in row.items() if k != "ranks"}}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", action="store_true", help="the ranged walks of emulated ranks next to the full walk")
    ap.add_argument("--worlds", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--potential", action="store_true", help="the tree potential next to the all-pairs potential")
    ap.add_argument("--out", default=None, help="profiles/r28_tree.json, or profiles/r30_tree_potential.json")
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 262144, 524288])
    ap.add_argument("--thetas", type=float, nargs="+", default=[0.5, 0.75])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "r30_tree_potential.json" if args.potential else "r28_tree.json")
    if args.ranks:
        if args.out == os.path.join(ROOT, "profiles", "r28_tree.json"):
            args.out = os.path.join(ROOT, "profiles", "r31_tree_ranks.json")
        sizes = args.sizes if args.sizes != ap.get_default("sizes") else [262144, 524288]
        res = {"device": torch.cuda.get_device_name(0), "softening": EPS, "quadrupole": True, "rounds": ROUNDS,
               "cases": [ranks_case(n, 0.5, args.worlds) for n in sizes]}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        return
    one = potential_case if args.potential else case
    res = {"device": torch.cuda.get_device_name(0), "softening": EPS, "quadrupole": True, "sampled_rows": SAMPLED,
           "rounds": ROUNDS, "cases": [one(n, args.thetas) for n in args.sizes]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
