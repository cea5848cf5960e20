"""4th-order Hermite step against the general-mass leapfrog step on the MI355X, in one run.

  python tools/bench_hermite.py [--out FILE]

1. Step time (HIP events around repeated step() calls) and force time at N = 4 096, 16 384, 65 536: the Hermite step
   (HermiteSimulator) and the leapfrog step with the general kernel (NBD_UNIFORM_MASS=0, LeapFrogSimulator); pairs/s of
   each. The force alone: nbd_accel_jerk_f32 (kernel + slab sum) against the leapfrog step's force kernel (the step's
   event hooks around accel_kernel<false, ...>).
2. Error against GPU time for both integrators: one period of the e = 0.5 two-body orbit (eps = 0, error against the
   exact closed orbit) and a softened Plummer sphere of N = 4 096 over one time unit (median per-body position error
   against a Hermite run at dt = 1/1024).
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
os.environ["NBD_UNIFORM_MASS"] = "0"          # the leapfrog side runs the general (per-pair mass) kernel

from galaxify import simulation  # noqa: E402
from nbd import direct  # noqa: E402
from nbd.plummer import generate_plummer  # noqa: E402
import hermite_oracle as ho  # noqa: E402


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
    m = np.asarray(m) * np.random.default_rng(2).uniform(0.5, 1.5, n)     # unequal masses
    kw = dict(positions=p, velocities=v, masses=m, softening=0.05, dt=1e-4, calc_energy=False, device="cuda")
    reps = max(5, min(200, int(4e10 / n / n)))
    lf, he = simulation.LeapFrogSimulator(**kw), simulation.HermiteSimulator(**kw)
    assert lf._uniform is None
    for _ in range(warmup):
        lf.step(); he.step()
    torch.cuda.synchronize()
    lf_ms = _timed(lf.step, reps)
    he_ms = _timed(he.step, reps)
    # force alone: the leapfrog step's event hooks around its force kernel; nbd_accel_jerk_f32 for Hermite
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    acc = torch.empty_like(lf.accelerations)
    for b, e in evs:
        b.record(); e.record()
    torch.cuda.synchronize()
    for b, e in evs:
        direct.leapfrog_step(lf.positions, lf.velocities, lf.accelerations, acc, lf.masses, direct.f32(0.5 * lf.dt),
                             direct.f32(lf.dt), lf._eps2, lf._g, lf._posm, lf._ws, ev_begin=b, ev_end=e)
    torch.cuda.synchronize()
    lf_force = float(np.median([b.elapsed_time(e) for b, e in evs]))
    direct.hermite_pack(he.positions, he.velocities, he.masses, he._posm, he._velp)
    res = {"n": n, "reps": reps, "leapfrog_step_ms": lf_ms, "hermite_step_ms": he_ms,
           "leapfrog_force_kernel_ms": lf_force}
    for variant in (0, 1):
        a, j = torch.empty_like(acc), torch.empty_like(acc)
        f = (lambda: direct.accel_jerk(he._posm, he._velp, n, he._eps2, he._g, a, j, he._hws, variant=variant))
        f()
        res[f"hermite_force_ms_variant{variant}"] = _timed(f, reps)
    res["step_ratio"] = he_ms / lf_ms
    res["force_ratio"] = res["hermite_force_ms_variant0"] / lf_force
    res["leapfrog_pairs_per_s"] = n * n / (lf_ms * 1e-3)
    res["hermite_pairs_per_s"] = n * n / (he_ms * 1e-3)
    return res


def run_gpu_ms(sim, steps):
    torch.cuda.synchronize()
    return _timed(sim.step, steps) * steps


def two_body_error_vs_time():
    x0, v0, m, period = ho.two_body(0.5)
    out = []
    for cls, ks in (("HermiteSimulator", (32, 64, 128, 256, 512)), ("LeapFrogSimulator", (128, 256, 512, 1024, 2048))):
        for k in ks:
            sim = getattr(simulation, cls)(positions=x0, velocities=v0, masses=m, g_const=1.0, softening=0.0,
                                           dt=period / k, calc_energy=False, device="cuda")
            ms = run_gpu_ms(sim, k)
            err = ho.orbit_error(sim.positions.cpu().numpy(), x0.astype(np.float32))
            out.append({"integrator": cls, "steps": k, "gpu_ms": ms, "error": err})
    return out


def plummer_error_vs_time(n=4096):
    p, v, m = generate_plummer(n, seed=3)
    kw = dict(positions=p, velocities=v, masses=m, softening=0.05, calc_energy=False, device="cuda")
    ref = simulation.HermiteSimulator(dt=1.0 / 1024, **kw)
    for _ in range(1024):
        ref.step()
    x_ref = ref.positions.cpu().double()
    out = []
    for cls, ks in (("HermiteSimulator", (16, 32, 64, 128)), ("LeapFrogSimulator", (32, 64, 128, 256, 512))):
        for k in ks:
            sim = getattr(simulation, cls)(dt=1.0 / k, **kw)
            ms = run_gpu_ms(sim, k)
            row = (sim.positions.cpu().double() - x_ref).norm(dim=1)
            # the median body: the largest row error comes from a few close encounters and sits at the same level for
            # every step size tried
            out.append({"integrator": cls, "steps": k, "gpu_ms": ms, "error": float(row.median()),
                        "max_error": float(row.max())})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 16384, 65536])
    ap.add_argument("--steps-only", action="store_true", help="step and force times only (for a profiler pass)")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "steps": [step_times(n) for n in args.sizes]}
    if not args.steps_only:
        res["two_body_e0.5"] = two_body_error_vs_time()
        res["plummer_n4096"] = plummer_error_vs_time()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
