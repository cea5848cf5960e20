"""Hermite6Simulator next to HermiteSimulator(dtype=torch.float64) on the MI355X, in one process.

  python tools/bench_hermite6.py [--out FILE]          (default: profiles/r20_hermite6.json)

1. The force alone, nbd_accel_jerk_snap_f64 against nbd_accel_jerk_f64 on the same packed rows, and the step of the two
   simulators (HIP events around repeated calls, median of 5 batches) at N = 4 096, 16 384, 65 536, with their ratios.
   The pair functor of the 6th order holds about 1.7 times the fp64 operations of the 4th order's (an instruction count).
2. One period of the e = 0.5 two-body orbit at eps = 0.1: |E1 - E0| / |E0| from compute_invariants() per step count for
   both orders with the GPU time of the run, the fp64 oracles' own errors, and the figure of merit: the GPU time of the
   shortest run of each order that reaches an energy error <= 1e-10.
3. A softened Plummer sphere of N = 4 096 over one time unit: the median per-body position error per step count for both
   orders, against a 6th-order run at dt = 1/1024, with the GPU time of each run.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-deep-sim_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from galaxify import simulation  # noqa: E402
from nbd import direct  # noqa: E402
from nbd.plummer import generate_plummer  # noqa: E402
import hermite6_oracle as h6  # noqa: E402
import hermite_f64_oracle as fo  # noqa: E402
import hermite_oracle as ho  # noqa: E402

MODEL_OPS_RATIO = 1.7           # fp64 operations of AccelJerkSnapPair::pair over AccelJerkPair::pair, counted
TARGET = 1e-10


def _sim(order, **kw):
    if order == 6:
        return simulation.Hermite6Simulator(**kw)
    return simulation.HermiteSimulator(dtype=torch.float64, **kw)


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _median(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return float(np.median([_timed(fn, reps) for _ in range(5)]))


def force_and_step_times(n):
    p, v, m = generate_plummer(n, seed=1)
    m = np.asarray(m) * np.random.default_rng(2).uniform(0.5, 1.5, n)
    kw = dict(positions=p, velocities=v, masses=m, softening=0.05, dt=1e-4, calc_energy=False, device="cuda")
    reps = max(3, min(100, int(1e10 / n / n)))
    res = {"n": n, "reps": reps, "model_ops_ratio": MODEL_OPS_RATIO}
    six, four = _sim(6, **kw), _sim(4, **kw)
    eps2, g = six._fmt._scalars(six)
    ws6, ws4 = direct.hermite6_workspace(n, six.device), direct.hermite_f64_workspace(n, six.device)
    res["force4_ms"] = _median(lambda: direct.accel_jerk_f64(six._posd, six._veld, n, eps2, g, workspace=ws4), reps)
    res["force6_ms"] = _median(
        lambda: direct.accel_jerk_snap_f64(six._posd, six._veld, six._accd, n, eps2, g, workspace=ws6), reps)
    res["force6_over_force4"] = res["force6_ms"] / res["force4_ms"]
    res["step4_ms"] = _median(four.step, reps)
    res["step6_ms"] = _median(six.step, reps)
    res["step6_over_step4"] = res["step6_ms"] / res["step4_ms"]
    for k in ("force4", "force6", "step4", "step6"):
        res[f"{k}_gpairs_per_s"] = n * n / res[f"{k}_ms"] / 1e6
    return res


def _orbit_run(order, x, v, m, eps, period, steps):
    sim = _sim(order, positions=x, velocities=v, masses=m, softening=eps, dt=period / steps, calc_energy=False,
               device="cuda")
    e_start = sim.compute_invariants().energy
    ms = _timed(sim.step, steps) * steps                 # (the callers warm both paths up first)
    return abs(sim.compute_invariants().energy - e_start) / abs(e_start), ms


def two_body(sweep=(64, 128, 256, 512, 1024, 2048), fine6=(320, 352, 384, 416, 448, 480),
             fine4=(1280, 1408, 1536, 1664, 1792, 1920)):
    x, v, m, period = ho.two_body(0.5)
    x, v, m = fo.perturbed(x, v, m, 9)
    eps = 0.1
    e0 = fo.energy(x, v, m, 1.0, eps * eps)
    _orbit_run(6, x, v, m, eps, period, 64); _orbit_run(4, x, v, m, eps, period, 64)          # warm-up of both paths

    def oracle(run, s):
        r = run(x, v, m, period / s, 1.0, eps * eps, s)
        return abs(fo.energy(r[0], r[1], m, 1.0, eps * eps) - e0) / abs(e0)
    rows = []
    for s in sweep:
        row = {"steps": s}
        for order, run in ((6, h6.hermite6_run), (4, ho.hermite_run)):
            err, ms = _orbit_run(order, x, v, m, eps, period, s)
            row[f"order{order}_energy_error"], row[f"order{order}_gpu_ms"] = err, ms
            row[f"order{order}_oracle_energy_error"] = oracle(run, s)
        rows.append(row)
    merit = {"target_energy_error": TARGET}
    for order, fine in ((6, fine6), (4, fine4)):
        tried = []
        for s in sorted(set(fine) | set(sweep)):
            err, ms = _orbit_run(order, x, v, m, eps, period, s)
            tried.append({"steps": s, "energy_error": err, "gpu_ms": ms})
        reached = [t for t in tried if t["energy_error"] <= TARGET]
        merit[f"order{order}"] = {"tried": tried, "first_to_reach": min(reached, key=lambda t: t["steps"]) if reached
                                  else None}
    a, b = merit["order6"]["first_to_reach"], merit["order4"]["first_to_reach"]
    if a and b:
        merit["gpu_time_order4_over_order6"] = b["gpu_ms"] / a["gpu_ms"]
    return {"rows": rows, "time_to_target": merit}


def plummer(n=4096, steps_list=(4, 8, 16, 32, 64, 128, 256), ref_steps=1024):
    p, v, m = generate_plummer(n, seed=7)
    kw = dict(positions=p, velocities=v, masses=m, softening=0.05, calc_energy=False, device="cuda")

    def final(order, steps):
        sim = _sim(order, dt=1.0 / steps, **kw)
        ms = _timed(sim.step, steps) * steps
        return sim.positions.cpu().numpy(), ms
    final(6, 4); final(4, 4)
    ref, _ = final(6, ref_steps)
    out = []
    for s in steps_list:
        row = {"steps": s}
        for order in (6, 4):
            x, ms = final(order, s)
            row[f"order{order}_median_error"] = float(np.median(np.linalg.norm(x - ref, axis=1)))
            row[f"order{order}_gpu_ms"] = ms
        out.append(row)
    return {"n": n, "reference": f"6th order, {ref_steps} steps", "rows": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_hermite6.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    res = {"device": torch.cuda.get_device_name(0),
           "force_and_step_times": [force_and_step_times(n) for n in (4096, 16384, 65536)],
           "two_body_e0.5_eps0.1": two_body(),
           "plummer": plummer()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
