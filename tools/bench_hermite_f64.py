"""HermiteSimulator(dtype=torch.float64) next to the fp32 HermiteSimulator on the MI355X, in one process.

  python tools/bench_hermite_f64.py [--out FILE]          (default: profiles/r12_hermite_f64.json)

1. Step time (HIP events around repeated step() calls, median of 5 batches) at N = 4 096, 16 384, 65 536 in both
   precisions, and their ratio.
2. One period of the e = 0.5 two-body orbit at eps = 0.1: |E1 - E0| / |E0| from compute_invariants() per step count, in
   both precisions, and the fp64 oracle's own.
3. A softened Plummer sphere of N = 4 096 over one time unit: the median per-body position error per step count in both
   precisions, against a float64 run at dt = 1/1024.
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
from nbd.plummer import generate_plummer  # noqa: E402
import hermite_f64_oracle as fo  # noqa: E402
import hermite_oracle as ho  # noqa: E402

DTYPES = (("f32", torch.float32), ("f64", torch.float64))


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def step_times(n, warmup=3):
    p, v, m = generate_plummer(n, seed=1)
    m = np.asarray(m) * np.random.default_rng(2).uniform(0.5, 1.5, n)
    kw = dict(positions=p, velocities=v, masses=m, softening=0.05, dt=1e-4, calc_energy=False, device="cuda")
    reps = max(3, min(100, int(1e10 / n / n)))
    res = {"n": n, "reps": reps}
    for name, dtype in DTYPES:
        sim = simulation.HermiteSimulator(dtype=dtype, **kw)
        for _ in range(warmup):
            sim.step()
        torch.cuda.synchronize()
        res[f"{name}_step_ms"] = float(np.median([_timed(sim.step, reps) for _ in range(5)]))
        res[f"{name}_gpairs_per_s"] = n * n / res[f"{name}_step_ms"] / 1e6
    res["f64_over_f32"] = res["f64_step_ms"] / res["f32_step_ms"]
    return res


def two_body(steps_list=(64, 128, 256, 512, 1024, 2048, 4096)):
    x, v, m, period = ho.two_body(0.5)
    eps = 0.1
    e0 = fo.energy(x, v, m, 1.0, eps * eps)
    out = []
    for s in steps_list:
        row = {"steps": s}
        for name, dtype in DTYPES:
            sim = simulation.HermiteSimulator(positions=x, velocities=v, masses=m, softening=eps, dt=period / s,
                                              calc_energy=False, device="cuda", dtype=dtype)
            e_start = sim.compute_invariants().energy
            for _ in range(s):
                sim.step()
            row[f"{name}_energy_error"] = abs(sim.compute_invariants().energy - e_start) / abs(e_start)
        xr, vr, _, _ = ho.hermite_run(x, v, m, period / s, 1.0, eps * eps, s)
        row["oracle_energy_error"] = abs(fo.energy(xr, vr, m, 1.0, eps * eps) - e0) / abs(e0)
        out.append(row)
    return out


def plummer(n=4096, steps_list=(4, 8, 16, 32, 64, 128, 256), ref_steps=1024):
    p, v, m = generate_plummer(n, seed=7)
    kw = dict(positions=p, velocities=v, masses=m, softening=0.05, calc_energy=False, device="cuda")

    def final(dtype, steps):
        sim = simulation.HermiteSimulator(dt=1.0 / steps, dtype=dtype, **kw)
        for _ in range(steps):
            sim.step()
        return sim.positions.double().cpu().numpy()
    ref = final(torch.float64, ref_steps)
    out = []
    for s in steps_list:
        row = {"steps": s}
        for name, dtype in DTYPES:
            row[f"{name}_median_error"] = float(np.median(np.linalg.norm(final(dtype, s) - ref, axis=1)))
        out.append(row)
    return {"n": n, "reference": f"float64, {ref_steps} steps", "rows": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_hermite_f64.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    res = {"device": torch.cuda.get_device_name(0),
           "step_times": [step_times(n) for n in (4096, 16384, 65536)],
           "two_body_e0.5_eps0.1": two_body(),
           "plummer": plummer()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
