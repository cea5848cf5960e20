"""Block-timestep Hermite (BlockHermiteSimulator) on the MI355X, in one run.

  python tools/bench_hermite_block.py [--out FILE] [--dtype float64]

1. The active-subset force at n = 65 536 sources: nbd_accel_jerk_active_f32 (kernel + slab sum) for n_act = 65 536,
   8 192, 1 024, 128, interleaved with nbd_accel_jerk_f32 on the same state; time and pair rate of each.
2. Block-step cost at n = 65 536: levels planted so that the first block step has n_act active bodies (max_level 10),
   then schedule + readback + predict + force + correct timed wall-clock with a sync; a least-squares fit
   T(n_act) = (n_act / n) T_full + F, with T_full the HermiteSimulator step.
3. Accuracy per time. (a) One period of the e = 0.9 two-body orbit (eps = 0): shared Hermite step sweep against block eta
   sweep; error against the exact closed orbit and the wall time of the steps (all launch-bound at n = 2). (b) A Plummer
   sphere of n = 16 384, eps = 0.01, one time unit: shared dt = 1/64 ... 1/1024 and block eta sweeps (dt = 1/16,
   max_level 10), max-body and 99.9th-percentile position error against a block run at eta = 0.0025, with wall time.

With --dtype float64 (BlockHermiteSimulator(dtype=torch.float64), csrc/direct_hermite_block_f64.hip), all in one process:
1. nbd_accel_jerk_active_f64 with every body listed against nbd_accel_jerk_f64 (the same wave body and plan), and shorter
   lists, interleaved as above.
2. The block-step cost fit of both precisions, from the same run.
3. The e = 0.9 orbit (eps = 0, one period as 4 output steps, max_level 16): eta = 0.01 ... 0.000625 in float64 beside
   float32; error, pair interactions, clamped levels and wall time per eta.
The default output is profiles/r13_hermite_block_f64.json.

With --order 6 (BlockHermite6Simulator, the 6th order of csrc/direct_hermite_block_f64.hip; float64), all in one process:
1. nbd_accel_jerk_snap_active_f64 with every body listed against nbd_accel_jerk_snap_f64 (the same wave body and plan),
   and shorter lists, interleaved as above.
2. The block-step cost fit of the 6th order (T_full the Hermite6Simulator step) beside the float64 4th order's.
3. The e = 0.9 orbit (eps = 0, one period as 4 output steps, max_level 16): eta = 0.01 ... 0.000625 at the 6th order
   beside BlockHermiteSimulator(dtype=torch.float64); error, pair interactions, clamped levels, wall time and the GPU
   time of the four output steps (HIP events) per eta.
The default output is profiles/r23_hermite6_block.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-deep-sim_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from galaxify import simulation  # noqa: E402
from nbd import direct  # noqa: E402
from nbd.plummer import generate_plummer  # noqa: E402
import hermite_oracle as ho  # noqa: E402


def _event_ms(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def active_force(n=65536, reps=20):
    p, v, m = generate_plummer(n, seed=1)
    dev = torch.device("cuda")
    pos, vel = torch.tensor(p, dtype=torch.float32, device=dev), torch.tensor(v, dtype=torch.float32, device=dev)
    mass = torch.tensor(m, dtype=torch.float32, device=dev)
    posm, velp = direct.alloc_posm(n, dev), direct.alloc_posm(n, dev)
    direct.hermite_pack(pos, vel, mass, posm, velp)
    eps2 = direct.f32(0.01 ** 2)
    hws, bws = direct.hermite_workspace(n, dev), direct.hblock_workspace(n, dev)
    a, j = torch.empty((n, 3), device=dev), torch.empty((n, 3), device=dev)
    rng = np.random.default_rng(0)
    rows = []
    for n_act in (65536, 8192, 1024, 128):
        act = torch.tensor(np.sort(rng.permutation(n)[:n_act]), dtype=torch.int32, device=dev)
        f_all = (lambda: direct.accel_jerk(posm, velp, n, eps2, 1.0, a, j, hws))
        f_act = (lambda: direct.accel_jerk_active(posm, velp, n, act, eps2, 1.0, bws))
        for _ in range(3):
            f_all(); f_act()
        full, part = [], []
        for _ in range(3):                                   # interleaved rounds
            full.append(_event_ms(f_all, reps)); part.append(_event_ms(f_act, reps))
        full_ms, act_ms = float(np.median(full)), float(np.median(part))
        rows.append({"n": n, "n_act": n_act, "accel_jerk_ms": full_ms, "active_ms": act_ms,
                     "ratio_to_full": act_ms / full_ms,
                     "pair_rate_fraction": (n_act / act_ms) / (n / full_ms)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def active_force_f64(n=65536, reps=10):
    p, v, m = generate_plummer(n, seed=1)
    dev = torch.device("cuda")
    f64 = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, device=dev)      # noqa: E731
    posd, veld = direct.alloc_rows_f64(n, dev), direct.alloc_rows_f64(n, dev)
    direct.hermite_f64_pack(f64(p), f64(v), f64(m), posd, veld)
    eps2 = 0.01 ** 2
    hws, bws = direct.hermite_f64_workspace(n, dev), direct.hblock_f64_workspace(n, dev)
    rng = np.random.default_rng(0)
    rows = []
    for n_act in (65536, 8192, 1024, 128):
        act = torch.tensor(np.sort(rng.permutation(n)[:n_act]), dtype=torch.int32, device=dev)
        f_all = (lambda: direct.accel_jerk_f64(posd, veld, n, eps2, 1.0, workspace=hws))
        f_act = (lambda: direct.accel_jerk_active_f64(posd, veld, n, act, eps2, 1.0, workspace=bws))
        for _ in range(2):
            f_all(); f_act()
        full, part = [], []
        for _ in range(3):                                   # interleaved rounds
            full.append(_event_ms(f_all, reps)); part.append(_event_ms(f_act, reps))
        full_ms, act_ms = float(np.median(full)), float(np.median(part))
        rows.append({"n": n, "n_act": n_act, "accel_jerk_f64_ms": full_ms, "active_f64_ms": act_ms,
                     "ratio_to_full": act_ms / full_ms,
                     "pair_rate_fraction": (n_act / act_ms) / (n / full_ms)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def active_force6(n=65536, reps=10):
    p, v, m = generate_plummer(n, seed=1)
    dev = torch.device("cuda")
    f64 = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, device=dev)      # noqa: E731
    posd, veld, accd = (direct.alloc_rows_f64(n, dev) for _ in range(3))
    eps2 = 0.01 ** 2
    hws, bws = direct.hermite6_workspace(n, dev), direct.hblock6_workspace(n, dev)
    direct.hermite6_pack(f64(p), f64(v), f64(m), posd, veld, accd)
    acc = direct.accel_jerk_snap_f64(posd, veld, accd, n, eps2, 1.0, workspace=hws)[0]
    direct.hermite6_pack(f64(p), f64(v), f64(m), posd, veld, accd, acc=acc)
    rng = np.random.default_rng(0)
    rows = []
    for n_act in (65536, 8192, 1024, 128):
        act = torch.tensor(np.sort(rng.permutation(n)[:n_act]), dtype=torch.int32, device=dev)
        f_all = (lambda: direct.accel_jerk_snap_f64(posd, veld, accd, n, eps2, 1.0, workspace=hws))
        f_act = (lambda: direct.accel_jerk_snap_active_f64(posd, veld, accd, n, act, eps2, 1.0, workspace=bws))
        for _ in range(2):
            f_all(); f_act()
        full, part = [], []
        for _ in range(3):                                   # interleaved rounds
            full.append(_event_ms(f_all, reps)); part.append(_event_ms(f_act, reps))
        full_ms, act_ms = float(np.median(full)), float(np.median(part))
        rows.append({"n": n, "n_act": n_act, "accel_jerk_snap_f64_ms": full_ms, "active_snap_f64_ms": act_ms,
                     "ratio_to_full": act_ms / full_ms,
                     "pair_rate_fraction": (n_act / act_ms) / (n / full_ms)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def block_step_cost(n=65536, K=10, reps=15, dtype=torch.float32, order=4):
    p, v, m = generate_plummer(n, seed=1)
    kw = dict(positions=p, velocities=v, masses=m, softening=0.01, dt=1e-3, calc_energy=False, device="cuda",
              dtype=dtype)
    shared, block = ((simulation.HermiteSimulator, simulation.BlockHermiteSimulator) if order == 4 else
                     (simulation.Hermite6Simulator, simulation.BlockHermite6Simulator))
    he = shared(**kw)
    for _ in range(3):
        he.step()
    torch.cuda.synchronize()
    t_full = _event_ms(he.step, reps)
    sim = block(max_level=K, **kw)
    host = sim._sched_host
    pts = []
    for n_act in (128, 1024, 8192, 32768, 65536):
        wall = []
        for r in range(reps + 2):
            # plant n_act bodies at level K and the rest at 0, at tick 0: levels, ticks, and the schedule's current
            # tick, cursor and level histogram (sched[3:], include/nbd.h)
            sim.levels.zero_(); sim.levels[:n_act] = K; sim._ticks.zero_(); sim._sched[3:] = 0
            sim._sched[8] = n - n_act; sim._sched[8 + K] = n_act
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            direct.hblock_schedule(sim.levels, K, sim._sched, sim._bws, host_sched=host)
            got = int(host[1])
            sim._fmt.block_step(sim, got)
            torch.cuda.synchronize()
            if r >= 2:
                wall.append((time.perf_counter() - t0) * 1e3)
            assert got == (n_act if n_act < n else n)
        pts.append({"n_act": n_act, "block_step_ms": float(np.median(wall))})
        print(json.dumps(pts[-1]), flush=True)
    f = np.array([q["n_act"] / n for q in pts])
    t = np.array([q["block_step_ms"] for q in pts])
    slope, icpt = np.polyfit(f, t, 1)
    return {"n": n, "max_level": K, "dtype": str(dtype), "order": order, "hermite_step_ms": t_full, "points": pts,
            "fit_T_full_ms": float(slope), "fit_F_us": float(icpt * 1e3)}


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def orbit(e=0.9):
    x0, v0, m, period = ho.two_body(e)
    out = {"shared": [], "block": []}
    for steps in (256, 512, 1024, 2048, 4096):
        sim = simulation.HermiteSimulator(positions=x0, velocities=v0, masses=m, softening=0.0, dt=period / steps,
                                          calc_energy=False, device="cuda")
        sim.step()                                              # warm
        sim = simulation.HermiteSimulator(positions=x0, velocities=v0, masses=m, softening=0.0, dt=period / steps,
                                          calc_energy=False, device="cuda")
        s = _wall(lambda: [sim.step() for _ in range(steps)])
        out["shared"].append({"steps": steps, "pairs": 4 * steps, "wall_s": s,
                              "err": ho.orbit_error(sim.positions.cpu().numpy(), x0.astype(np.float32))})
        print(json.dumps(out["shared"][-1]), flush=True)
    for eta in (0.16, 0.08, 0.04, 0.02, 0.01):
        sim = simulation.BlockHermiteSimulator(positions=x0, velocities=v0, masses=m, softening=0.0, dt=period / 4,
                                               calc_energy=False, device="cuda", eta=eta, max_level=12)
        s = _wall(lambda: [sim.step() for _ in range(4)])
        out["block"].append({"eta": eta, "block_steps": sim.block_steps, "pairs": sim.pair_interactions, "wall_s": s,
                             "err": ho.orbit_error(sim.positions.cpu().numpy(), x0.astype(np.float32))})
        print(json.dumps(out["block"][-1]), flush=True)
    return out


def orbit_f64(e=0.9, K=16):
    """The eta sweep of the eccentric orbit in both precisions: the fp32 run stops gaining at its floor, fp64 does not."""
    x0, v0, m, period = ho.two_body(e)
    out = []
    for eta in (0.01, 0.0025, 0.000625):
        row = {"eta": eta, "max_level": K}
        for name, dtype, ref in (("float64", torch.float64, x0), ("float32", torch.float32, x0.astype(np.float32))):
            kw = dict(positions=x0, velocities=v0, masses=m, softening=0.0, dt=period / 4, calc_energy=False,
                      device="cuda", eta=eta, max_level=K, dtype=dtype)
            simulation.BlockHermiteSimulator(**kw).step()       # warm
            sim = simulation.BlockHermiteSimulator(**kw)
            s = _wall(lambda: [sim.step() for _ in range(4)])
            row[name] = {"err": ho.orbit_error(sim.positions.cpu().numpy(), ref), "pairs": sim.pair_interactions,
                         "block_steps": sim.block_steps, "clamped": sim.clamped, "wall_s": s}
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def orbit6(e=0.9, K=16):
    """The eta sweep of the eccentric orbit at the 6th order beside the float64 4th order."""
    x0, v0, m, period = ho.two_body(e)
    out = []
    for eta in (0.01, 0.0025, 0.000625):
        row = {"eta": eta, "max_level": K}
        for name, cls, fmt in (("order6", simulation.BlockHermite6Simulator, {}),
                               ("order4_float64", simulation.BlockHermiteSimulator, {"dtype": torch.float64})):
            kw = dict(positions=x0, velocities=v0, masses=m, softening=0.0, dt=period / 4, calc_energy=False,
                      device="cuda", eta=eta, max_level=K, **fmt)
            cls(**kw).step()                                    # warm
            sim = cls(**kw)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s = _wall(lambda: [sim.step() for _ in range(4)])
            e1.record()
            torch.cuda.synchronize()
            row[name] = {"err": ho.orbit_error(sim.positions.cpu().numpy(), x0), "pairs": sim.pair_interactions,
                         "block_steps": sim.block_steps, "clamped": sim.clamped, "wall_s": s,
                         "gpu_ms": e0.elapsed_time(e1)}
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def plummer(n=16384, eps=0.01):
    p, v, m = generate_plummer(n, seed=3)
    kw = dict(positions=p, velocities=v, masses=m, softening=eps, calc_energy=False, device="cuda")

    def block(eta):
        sim = simulation.BlockHermiteSimulator(dt=1.0 / 16, eta=eta, max_level=10, **kw)
        s = _wall(lambda: [sim.step() for _ in range(16)])
        return sim, s

    ref, ref_s = block(0.0025)
    xr = ref.positions.cpu().numpy().astype(np.float64)

    def errs(sim):
        d = np.linalg.norm(sim.positions.cpu().numpy().astype(np.float64) - xr, axis=1)
        return float(d.max()), float(np.percentile(d, 99.9))

    out = {"n": n, "eps": eps, "reference": {"eta": 0.0025, "wall_s": ref_s, "block_steps": ref.block_steps,
                                             "pairs": ref.pair_interactions}, "shared": [], "block": []}
    for k in (64, 128, 256, 512, 1024):
        sim = simulation.HermiteSimulator(dt=1.0 / k, **kw)
        s = _wall(lambda: [sim.step() for _ in range(k)])
        mx, p999 = errs(sim)
        out["shared"].append({"dt": 1.0 / k, "wall_s": s, "pairs": k * n * n, "max_err": mx, "p999_err": p999})
        print(json.dumps(out["shared"][-1]), flush=True)
    for eta in (0.04, 0.02, 0.01):
        sim, s = block(eta)
        mx, p999 = errs(sim)
        out["block"].append({"eta": eta, "wall_s": s, "block_steps": sim.block_steps, "pairs": sim.pair_interactions,
                             "clamped": sim.clamped, "max_err": mx, "p999_err": p999,
                             "levels_hist": np.bincount(sim.levels.cpu().numpy(), minlength=11).tolist()})
        print(json.dumps(out["block"][-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="force,cost,orbit,plummer")
    ap.add_argument("--dtype", default="float32", choices=["float32", "float64"])
    ap.add_argument("--order", type=int, default=4, choices=[4, 6])
    args = ap.parse_args()
    parts = args.only.split(",")
    res = {"device": torch.cuda.get_device_name(0)}
    if args.order == 6:                                         # float64 only, whatever --dtype says
        args.dtype = "order6"
        args.out = args.out or os.path.join(ROOT, "profiles", "r23_hermite6_block.json")
        if "force" in parts:
            res["active_force_snap_f64"] = active_force6()
        if "cost" in parts:
            res["block_step_cost_order6"] = block_step_cost(dtype=torch.float64, order=6)
            res["block_step_cost_f64"] = block_step_cost(dtype=torch.float64)
        if "orbit" in parts:
            res["orbit_e09"] = orbit6()
    elif args.dtype == "float64":
        args.out = args.out or os.path.join(ROOT, "profiles", "r13_hermite_block_f64.json")
        if "force" in parts:
            res["active_force_f64"] = active_force_f64()
        if "cost" in parts:
            res["block_step_cost_f64"] = block_step_cost(dtype=torch.float64)
            res["block_step_cost_f32"] = block_step_cost(dtype=torch.float32)
        if "orbit" in parts:
            res["orbit_e09"] = orbit_f64()
    elif "force" in parts:
        res["active_force"] = active_force()
    if args.dtype == "float32" and "cost" in parts:
        res["block_step_cost"] = block_step_cost()
    if args.dtype == "float32" and "orbit" in parts:
        res["orbit_e09"] = orbit()
    if args.dtype == "float32" and "plummer" in parts:
        res["plummer16k"] = plummer()
    txt = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
