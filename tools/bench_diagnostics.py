"""Consistent-potential diagnostics on the MI355X (csrc/direct_diag.hip), in one run.

  python tools/bench_diagnostics.py [--out profiles/r09_diagnostics.json]

1. GPU time (HIP events around repeated calls, state already packed) of the invariants pipeline -- potential kernel +
   slab sum + invariants kernel, what compute_invariants() and a calc_invariants step add -- next to the energy pipeline
   of compute_energies() at N = 4 096, 16 384, 65 536; the potential alone; pairs/s of both.
2. Worst per-body relative error of phi at each N against fp64 rows (a contiguous block of rows from the middle of the
   system and the last, padded, group, all sources: the restriction oracle/c_oracle.py uses for large N).
3. Energy error of Hermite against leapfrog on two_body(0.5) (eps = 0.1, one period) and a Plummer sphere of N = 256
   (eps = 0.05, one time unit): max |E - E0| / |E0| of the consistent energy from calc_invariants, next to the same
   figure for the reference-convention u_energy + k_energy of the same states.
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
from nbd import _lib, direct  # noqa: E402
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


def _phi_rows_f64(pos, mass, g, eps2, lo, hi):
    x = np.asarray(pos, np.float32).astype(np.float64)
    m = np.asarray(mass, np.float32).astype(np.float64)
    out = np.empty(hi - lo)
    for a in range(lo, hi, 256):
        b = min(hi, a + 256)
        d = x[None, :, :] - x[a:b, None, :]
        r2 = (d * d).sum(-1) + eps2
        idx = np.arange(a, b)
        r2[idx - a, idx] = 1.0
        s = 1.0 / np.sqrt(r2)
        s[idx - a, idx] = 0.0
        out[a - lo:b - lo] = -g * (m[None, :] * s).sum(1)
    return out


def times_and_error(n, eps=0.05, rows=1024):
    p, v, m = generate_plummer(n, seed=1)
    m = np.asarray(m) * np.random.default_rng(2).uniform(0.5, 1.5, n)     # unequal masses
    sim = simulation.LeapFrogSimulator(positions=p, velocities=v, masses=m, softening=eps, dt=1e-4, calc_energy=False,
                                       device="cuda")
    reps = max(5, min(200, int(4e10 / n / n)))
    dev = sim.device
    phi = sim.compute_potentials()                  # packs _posm, allocates the workspace
    row = torch.empty(direct.INVARIANT_ROW, dtype=torch.float64, device=dev)
    uk = torch.empty(2, dtype=torch.float64, device=dev)
    ews = direct.alloc_bytes(_lib.lib().nbd_energy_workspace_bytes(n), dev)
    soft = direct.f32(sim.softening)

    def potential():
        sim._potentials_into(phi)

    def invariants():
        sim._potentials_into(phi)
        direct.invariants(sim._posm, sim.velocities, phi, n, out=row)

    def energies():
        direct.energy(sim._posm, sim.velocities, n, soft, sim._g, out_uk=uk, workspace=ews)
    for f in (potential, invariants, energies):
        f()
    torch.cuda.synchronize()
    res = {"n": n, "reps": reps, "potential_ms": _timed(potential, reps), "invariants_ms": _timed(invariants, reps),
           "energies_ms": _timed(energies, reps)}
    res["invariants_over_energies"] = res["invariants_ms"] / res["energies_ms"]
    res["potential_pairs_per_s"] = n * n / (res["potential_ms"] * 1e-3)
    res["energies_pairs_per_s"] = n * (n - 1) / 2 / (res["energies_ms"] * 1e-3)
    # phi against fp64 rows: a block from the middle and the last group
    got = phi.cpu().numpy()
    pos32, m32 = sim.positions.cpu().numpy(), sim.masses.cpu().numpy()
    worst = 0.0
    for lo, hi in ((n // 2, min(n, n // 2 + rows)), (max(0, n - 128), n)):
        ref = _phi_rows_f64(pos32, m32, sim._g, sim._eps2, lo, hi)
        worst = max(worst, float((np.abs(got[lo:hi] - ref) / np.abs(ref)).max()))
    res["phi_rows_checked"] = min(n, rows) + min(n, 128)
    res["phi_max_rel_err_vs_f64_rows"] = worst
    return res


def _drifts(sim, steps):
    e0 = sim.compute_invariants().energy
    u0, k0 = sim.compute_energies()
    states = sim.run(steps)
    return (max(abs(s.invariants.energy - e0) for s in states) / abs(e0),
            max(abs(s.u_energy + s.k_energy - (u0 + k0)) for s in states) / abs(u0 + k0))


def energy_errors():
    x0, v0, m2, period = ho.two_body(0.5)
    p, v, m = generate_plummer(256, seed=5)
    cases = (("two_body_e0.5_eps0.1_one_period", dict(positions=x0, velocities=v0, masses=m2, softening=0.1),
              period, (128, 256, 512)),
             ("plummer_n256_eps0.05_one_time_unit", dict(positions=p, velocities=v, masses=m, softening=0.05),
              1.0, (64, 128, 256)))
    out = []
    for name, kw, span, ks in cases:
        for cls in ("HermiteSimulator", "LeapFrogSimulator"):
            for k in ks:
                sim = getattr(simulation, cls)(g_const=1.0, dt=span / k, calc_energy=True, calc_invariants=True,
                                               device="cuda", **kw)
                good, naive = _drifts(sim, k)
                out.append({"case": name, "integrator": cls, "steps": k, "consistent_energy_error": good,
                            "reference_convention_energy_error": naive})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 16384, 65536])
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "sizes": [times_and_error(n) for n in args.sizes],
           "energy_errors": energy_errors()}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
