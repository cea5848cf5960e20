"""LeapFrogSimulator(dtype=torch.float64) next to K-H64's Hermite step and the fp32 leapfrog on the MI355X, in one process.

  python tools/bench_leapfrog_f64.py [--out FILE]          (default: profiles/r19_leapfrog_f64.json)

1. Step time (HIP events around repeated step() calls, median of 5 batches) at N = 4 096, 16 384, 65 536: the float64
   leapfrog step, HermiteSimulator(dtype=torch.float64)'s step and the fp32 general-mass leapfrog step (unequal masses:
   no equal-mass specialisation).
2. The force alone at the same sizes: nbd_accel_f64 against nbd_accel_jerk_f64 on the same packed rows, and their ratio
   (the instruction model: 22 against 36 fp64 operations per pair, 0.6-0.65).
3. One period of the e = 0.5 two-body orbit at eps = 0.1: |E1 - E0| / |E0| from compute_invariants() per step count, in
   both precisions, and the fp64 oracle's own.
4. A softened Plummer sphere of N = 4 096 over one time unit: per step count the median per-body distance of the fp32
   run from the float64 run of the SAME dt (what fp32 adds to the scheme's own error), and of both from a float64
   leapfrog run at dt = 1/4096 (the scheme's error).
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


def _median(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return float(np.median([_timed(fn, reps) for _ in range(5)]))


def _unequal(n):
    p, v, m = generate_plummer(n, seed=1)
    return p, v, np.asarray(m) * np.random.default_rng(2).uniform(0.5, 1.5, n)


def step_times(n):
    p, v, m = _unequal(n)
    kw = dict(positions=p, velocities=v, masses=m, softening=0.05, dt=1e-4, calc_energy=False, device="cuda")
    reps = max(3, min(100, int(1e10 / n / n)))
    res = {"n": n, "reps": reps}
    sims = (("leapfrog_f64", simulation.LeapFrogSimulator(dtype=torch.float64, **kw)),
            ("hermite_f64", simulation.HermiteSimulator(dtype=torch.float64, **kw)),
            ("leapfrog_f32", simulation.LeapFrogSimulator(**kw)))
    assert sims[2][1]._uniform is None
    for name, sim in sims:
        res[f"{name}_step_ms"] = _median(sim.step, reps)
        res[f"{name}_gpairs_per_s"] = n * n / res[f"{name}_step_ms"] / 1e6
    res["leapfrog_f64_over_hermite_f64"] = res["leapfrog_f64_step_ms"] / res["hermite_f64_step_ms"]
    res["leapfrog_f64_over_leapfrog_f32"] = res["leapfrog_f64_step_ms"] / res["leapfrog_f32_step_ms"]
    return res


def force_times(n):
    p, v, m = _unequal(n)
    dev = torch.device("cuda", torch.cuda.current_device())
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, device=dev)      # noqa: E731
    posd, veld = direct.alloc_rows_f64(n, dev), direct.alloc_rows_f64(n, dev)
    direct.hermite_f64_pack(t64(p), t64(v), t64(m), posd, veld)
    ws = direct.hermite_f64_workspace(n, dev)
    out = torch.empty((n, 3), dtype=torch.float64, device=dev)
    reps = max(3, min(100, int(1e10 / n / n)))
    eps2 = 0.05 ** 2
    res = {"n": n, "reps": reps, "slabs": direct.hermite_f64_plan(n)["slabs"]}
    res["accel_f64_ms"] = _median(lambda: direct.accel_f64(posd, n, eps2, 1.0, workspace=ws, out=out), reps)
    res["accel_jerk_f64_ms"] = _median(lambda: direct.accel_jerk_f64(posd, veld, n, eps2, 1.0, workspace=ws), reps)
    res["accel_over_accel_jerk"] = res["accel_f64_ms"] / res["accel_jerk_f64_ms"]
    assert torch.equal(out, direct.accel_jerk_f64(posd, veld, n, eps2, 1.0, workspace=ws)[0])
    return res


def two_body(steps_list=(256, 512, 1024, 2048, 4096, 8192)):
    x, v, m, period = ho.two_body(0.5)
    eps = 0.1
    e0 = fo.energy(x, v, m, 1.0, eps * eps)
    out = []
    for s in steps_list:
        row = {"steps": s}
        for name, dtype in DTYPES:
            sim = simulation.LeapFrogSimulator(positions=x, velocities=v, masses=m, softening=eps, dt=period / s,
                                               calc_energy=False, device="cuda", dtype=dtype)
            e_start = sim.compute_invariants().energy
            for _ in range(s):
                sim.step()
            row[f"{name}_energy_error"] = abs(sim.compute_invariants().energy - e_start) / abs(e_start)
        xr, vr = ho.leapfrog_run(x, v, m, period / s, 1.0, eps * eps, s)
        row["oracle_energy_error"] = abs(fo.energy(xr, vr, m, 1.0, eps * eps) - e0) / abs(e0)
        out.append(row)
    return out


def plummer(n=4096, steps_list=(16, 32, 64, 128, 256, 512, 1024), ref_steps=4096):
    p, v, m = generate_plummer(n, seed=7)
    kw = dict(positions=p, velocities=v, masses=m, softening=0.05, calc_energy=False, device="cuda")

    def final(dtype, steps):
        sim = simulation.LeapFrogSimulator(dt=1.0 / steps, dtype=dtype, **kw)
        for _ in range(steps):
            sim.step()
        return sim.positions.double().cpu().numpy()

    def dist(a, b):
        return float(np.median(np.linalg.norm(a - b, axis=1)))
    ref = final(torch.float64, ref_steps)
    out = []
    for s in steps_list:
        x32, x64 = final(torch.float32, s), final(torch.float64, s)
        out.append({"steps": s, "f32_from_f64_same_dt": dist(x32, x64), "f32_median_error": dist(x32, ref),
                    "f64_median_error": dist(x64, ref)})
    return {"n": n, "reference": f"float64 leapfrog, {ref_steps} steps", "rows": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_leapfrog_f64.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    sizes = (4096, 16384, 65536)
    res = {"device": torch.cuda.get_device_name(0),
           "step_times": [step_times(n) for n in sizes],
           "force_times": [force_times(n) for n in sizes],
           "two_body_e0.5_eps0.1": two_body(),
           "plummer": plummer()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
