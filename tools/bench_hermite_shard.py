"""One rank's share of the range-sharded Hermite step, emulated on ONE GPU, against the un-sharded Hermite kernels measured
in the same process (the yardstick; there is no gate). Rank `--rank` of `--world` owns n / world bodies of an n-body
Plummer sphere and runs, per step, exactly the launches the sharded HermiteSimulator issues --

    predict + pack (own rows) | [gather: here a device copy of the own rows into the gathered array]
    a, j (own x own)          | a, j (own x others) + slab sum + corrector

-- with HIP-event times per phase: medians over windows, after a time-based warm-up. Writes
profiles/r11_hermite_shard.json:   python tools/bench_hermite_shard.py [--n 65536 --world 8 --rank 3] [--big]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "nbody-deep-sim_amd"), ROOT):
    sys.path.insert(0, _p)
import torch
from nbd import direct
from nbd.plummer import generate_plummer

EPS2, G, DT = direct.f32(0.01), 1.0, 1e-3


def warm(fn, seconds=0.5):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:                   # clock ramp
        for _ in range(10):
            fn()
        torch.cuda.synchronize()


def window_ms(fn, reps, windows):
    """Median over `windows` of the HIP-event time of `reps` back-to-back calls, per call."""
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return statistics.median(out)


def unsharded(n, dev, windows):
    """nbd_accel_jerk_f32 and nbd_hermite_step_f32 at n bodies: (force ms, step ms)."""
    p, v, m = generate_plummer(n, seed=1234)
    pos, vel, mass = (torch.tensor(a, dtype=torch.float32, device=dev) for a in (p, v, m))
    posm, velp = direct.alloc_posm(n, dev), direct.alloc_posm(n, dev)
    hws = direct.hermite_workspace(n, dev)
    direct.hermite_pack(pos, vel, mass, posm, velp)
    acc, jerk = direct.accel_jerk(posm, velp, n, EPS2, G, workspace=hws)
    force = lambda: direct.accel_jerk(posm, velp, n, EPS2, G, acc_out=acc, jerk_out=jerk, workspace=hws)
    step = lambda: direct.hermite_step(pos, vel, acc, jerk, acc, jerk, mass, DT, EPS2, G, posm, hws)
    warm(force)
    reps = max(2, min(20, int(40e-3 / (2.0e-3 * (n / 65536) ** 2))))
    f_ms = window_ms(force, reps, windows)
    warm(step, 0.2)
    return f_ms, window_ms(step, reps, windows)


def rank_of(n, world, rank, dev, windows):
    """The emulated rank's phases at n bodies over `world` ranks, in ms."""
    n_loc = n // world
    lo = rank * n_loc
    p, v, m = generate_plummer(n, seed=1234)
    pos_all, vel_all, mass_all = (torch.tensor(a, dtype=torch.float32, device=dev) for a in (p, v, m))
    rows_all = direct.alloc_hermite_rows(n, dev)
    direct.hermite_shard_predict(pos_all, vel_all, mass_all, rows_all)        # every body's rows, as gathered
    pos, vel = pos_all[lo:lo + n_loc].clone(), vel_all[lo:lo + n_loc].clone()
    mass = mass_all[lo:lo + n_loc].contiguous()
    send = direct.alloc_hermite_rows(n_loc, dev)
    ws = direct.hermite_shard_workspace(n, lo, n_loc, dev)
    acc = torch.zeros((n_loc, 3), device=dev)
    jerk = torch.zeros((n_loc, 3), device=dev)
    direct.hermite_shard_predict(pos, vel, mass, send)
    direct.hermite_shard_force_local(send, n_loc, n, lo, EPS2, ws)
    direct.hermite_shard_force_remote(rows_all, n, send, n_loc, lo, EPS2, G, acc, jerk, ws)

    def step(ev=None):
        if ev: ev[0].record()
        direct.hermite_shard_predict(pos, vel, mass, send, acc, jerk, DT)
        if ev: ev[1].record()
        rows_all[lo:lo + n_loc].copy_(send[:n_loc])                # stands in for the all-gather's arrival
        if ev: ev[2].record()
        direct.hermite_shard_force_local(send, n_loc, n, lo, EPS2, ws)
        if ev: ev[3].record()
        direct.hermite_shard_force_remote(rows_all, n, send, n_loc, lo, EPS2, G, acc, jerk, ws, pos=pos, vel=vel,
                                          acc_in=acc, jerk_in=jerk, dt=DT)
        if ev: ev[4].record()

    warm(step)
    reps = max(2, min(20, int(40e-3 / (2.0e-3 / world * (n / 65536) ** 2))))
    step_ms = window_ms(step, reps, windows)
    names = ["predict", "gather_stand_in_copy", "force_local", "force_remote_finish_correct"]
    samples = {k: [] for k in names}
    for _ in range(max(windows * 4, 20)):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        step(ev)
        torch.cuda.synchronize()
        for i, k in enumerate(names):
            samples[k].append(ev[i].elapsed_time(ev[i + 1]))
    phase = {k: statistics.median(s) for k, s in samples.items()}
    return {"n": n, "world": world, "rank": rank, "n_local": n_loc, "plan": direct.hermite_shard_plan(n, lo, n_loc),
            "rank_step_ms": step_ms, "phase_ms": phase}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rank", type=int, default=3)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--big", action="store_true", help="also BASELINE configs[4]'s rank shape: 65 536 of 524 288")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_hermite_shard.json"))
    args = ap.parse_args()
    dev = "cuda"
    results = []
    for n in [args.n] + ([args.n * args.world] if args.big else []):
        windows = args.windows if n == args.n else 3
        f_ms, s_ms = unsharded(n, dev, windows)
        r = rank_of(n, args.world, args.rank, dev, windows)
        ph = r["phase_ms"]
        r["unsharded_force_ms"], r["unsharded_step_ms"] = f_ms, s_ms
        r["force_ratio"] = (ph["force_local"] + ph["force_remote_finish_correct"]) / (f_ms / args.world)
        r["step_ratio"] = r["rank_step_ms"] / (s_ms / args.world)
        results.append(r)
        print(json.dumps(r), flush=True)
    out = {"tool": "tools/bench_hermite_shard.py", "device": torch.cuda.get_device_name(0),
           "what": "one emulated rank of the range-sharded Hermite step; force_ratio = (local + remote) / (unsharded "
                   "force / world), step_ratio = rank step / (unsharded step / world), same process", "results": results}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
