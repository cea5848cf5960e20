"""One rank's share of the range-sharded Hermite step, emulated on ONE GPU, against the un-sharded Hermite kernels measured
in the same process (the yardstick; there is no gate). Rank `--rank` of `--world` owns n / world bodies of an n-body
Plummer sphere and runs, per step, exactly the launches the sharded HermiteSimulator issues --

    predict + pack (own rows) | [gather: here a device copy of the own rows into the gathered array]
    a, j (own x own)          | a, j (own x others) + slab sum + corrector

-- with HIP-event times per phase: medians over windows, after a time-based warm-up. Writes
profiles/r11_hermite_shard.json:   python tools/bench_hermite_shard.py [--n 65536 --world 8 --rank 3] [--big]
--dtype float64 runs the same launches of the float64 step (csrc/direct_hermite_shard_f64.hip) against the un-sharded
float64 kernels and writes profiles/r16_hermite_shard_f64.json:   python tools/bench_hermite_shard.py --dtype float64 --big
--integrator hermite6 runs the launches of the sharded Hermite6Simulator (the same unit's 6th-order entries, 12-double
rows) against the un-sharded 6th-order kernels and writes profiles/r22_hermite6_shard.json:
    python tools/bench_hermite_shard.py --integrator hermite6 --big
No multi-rank transport is in any of these numbers: the all-gather is a device copy of the rank's own rows."""
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

G, DT = 1.0, 1e-3


class _Fourth:
    """What the two measurements call, on the 4th-order entries a subclass names: the carried derivatives (acc, jerk), the
    un-sharded (force, step) calls and the three calls of a rank's step."""
    integrator = "hermite"

    @classmethod
    def new_state(cls, n, dev):
        return [torch.zeros((n, 3), dtype=cls.dtype, device=dev) for _ in range(2)]

    @classmethod
    def unsharded_calls(cls, n, dev, pos, vel, mass):
        posm, velp = cls.alloc_packed(n, dev), cls.alloc_packed(n, dev)
        hws = cls.workspace(n, dev)
        cls.pack(pos, vel, mass, posm, velp)
        acc, jerk = cls.new_state(n, dev)
        return (lambda: cls.force(posm, velp, n, acc, jerk, hws),
                lambda: cls.step(pos, vel, acc, jerk, mass, posm, velp, hws))

    @classmethod
    def pack_rows(cls, pos, vel, mass, rows):
        cls.predict(pos, vel, mass, rows)

    @classmethod
    def predict_step(cls, pos, vel, mass, send, state):
        cls.predict(pos, vel, mass, send, *state, DT)

    @classmethod
    def remote_force(cls, rows_all, n, send, n_loc, lo, ws, state):
        cls.remote(rows_all, n, send, n_loc, lo, cls.eps2, G, *state, ws)

    @classmethod
    def remote_step(cls, rows_all, n, send, n_loc, lo, ws, pos, vel, state):
        acc, jerk = state
        cls.remote(rows_all, n, send, n_loc, lo, cls.eps2, G, acc, jerk, ws, pos=pos, vel=vel, acc_in=acc, jerk_in=jerk,
                   dt=DT)


class Fmt32(_Fourth):
    """The float32 entries the two measurements call; Fmt64 names the float64 ones."""
    dtype, eps2, out = torch.float32, direct.f32(0.01), "r11_hermite_shard.json"
    alloc_packed, workspace, pack = direct.alloc_posm, direct.hermite_workspace, direct.hermite_pack
    rows, plan, shard_workspace = direct.alloc_hermite_rows, direct.hermite_shard_plan, direct.hermite_shard_workspace
    predict, local, remote = (direct.hermite_shard_predict, direct.hermite_shard_force_local,
                              direct.hermite_shard_force_remote)

    @staticmethod
    def force(posm, velp, n, acc, jerk, hws):
        direct.accel_jerk(posm, velp, n, Fmt32.eps2, G, acc_out=acc, jerk_out=jerk, workspace=hws)

    @staticmethod
    def step(pos, vel, acc, jerk, mass, posm, velp, hws):
        direct.hermite_step(pos, vel, acc, jerk, acc, jerk, mass, DT, Fmt32.eps2, G, posm, hws)


class Fmt64(_Fourth):
    dtype, eps2, out = torch.float64, 0.01, "r16_hermite_shard_f64.json"
    alloc_packed, workspace, pack = direct.alloc_rows_f64, direct.hermite_f64_workspace, direct.hermite_f64_pack
    rows, plan, shard_workspace = (direct.alloc_hermite_rows_f64, direct.hermite_shard_f64_plan,
                                   direct.hermite_shard_f64_workspace)
    predict, local, remote = (direct.hermite_shard_predict_f64, direct.hermite_shard_force_local_f64,
                              direct.hermite_shard_force_remote_f64)

    @staticmethod
    def force(posd, veld, n, acc, jerk, hws):               # (allocates its outputs: two cached (n,3) blocks per call)
        direct.accel_jerk_f64(posd, veld, n, Fmt64.eps2, G, workspace=hws)

    @staticmethod
    def step(pos, vel, acc, jerk, mass, posd, veld, hws):
        direct.hermite_step_f64(pos, vel, acc, jerk, acc, jerk, mass, DT, Fmt64.eps2, G, posd, veld, hws)


class Fmt6(_Fourth):
    """The 6th-order entries: float64, rows of 12 doubles, (acc, jerk, snap, crackle) carried."""
    integrator = "hermite6"
    dtype, eps2, out = torch.float64, 0.01, "r22_hermite6_shard.json"
    rows, plan, shard_workspace = (direct.alloc_hermite6_rows_f64, direct.hermite6_shard_f64_plan,
                                   direct.hermite6_shard_f64_workspace)
    predict, local = direct.hermite6_shard_predict_f64, direct.hermite6_shard_force_local_f64

    @classmethod
    def new_state(cls, n, dev):
        return [torch.zeros((n, 3), dtype=cls.dtype, device=dev) for _ in range(4)]

    @classmethod
    def unsharded_calls(cls, n, dev, pos, vel, mass):
        posd, veld, accd = (direct.alloc_rows_f64(n, dev) for _ in range(3))
        hws = direct.hermite6_workspace(n, dev)
        state = cls.new_state(n, dev)
        direct.hermite6_pack(pos, vel, mass, posd, veld, accd, acc=state[0])
        return (lambda: direct.accel_jerk_snap_f64(posd, veld, accd, n, cls.eps2, G, workspace=hws),
                lambda: direct.hermite6_step_f64(pos, vel, *state, *state, mass, DT, cls.eps2, G, posd, veld, accd, hws))

    @classmethod
    def remote_force(cls, rows_all, n, send, n_loc, lo, ws, state):
        direct.hermite6_shard_force_remote_f64(rows_all, n, send, n_loc, lo, cls.eps2, G, *state[:3], ws)

    @classmethod
    def remote_step(cls, rows_all, n, send, n_loc, lo, ws, pos, vel, state):
        acc, jerk, snap, crackle = state
        direct.hermite6_shard_force_remote_f64(rows_all, n, send, n_loc, lo, cls.eps2, G, acc, jerk, snap, ws, pos=pos,
                                               vel=vel, acc_in=acc, jerk_in=jerk, snap_in=snap, crackle_out=crackle,
                                               dt=DT)


FORMATS = {"float32": Fmt32, "float64": Fmt64}


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


def unsharded(fmt, n, dev, windows):
    """The un-sharded force (nbd_accel_jerk_f32 / _f64) and step (nbd_hermite_step_f32 / _f64) at n bodies:
    (force ms, step ms)."""
    p, v, m = generate_plummer(n, seed=1234)
    pos, vel, mass = (torch.tensor(a, dtype=fmt.dtype, device=dev) for a in (p, v, m))
    force, step = fmt.unsharded_calls(n, dev, pos, vel, mass)
    force()
    warm(force)
    reps = max(2, min(20, int(40e-3 / (2.0e-3 * (n / 65536) ** 2))))
    f_ms = window_ms(force, reps, windows)
    warm(step, 0.2)
    return f_ms, window_ms(step, reps, windows)


def rank_of(fmt, n, world, rank, dev, windows):
    """The emulated rank's phases at n bodies over `world` ranks, in ms."""
    n_loc = n // world
    lo = rank * n_loc
    eps2 = fmt.eps2
    p, v, m = generate_plummer(n, seed=1234)
    pos_all, vel_all, mass_all = (torch.tensor(a, dtype=fmt.dtype, device=dev) for a in (p, v, m))
    rows_all = fmt.rows(n, dev)
    fmt.pack_rows(pos_all, vel_all, mass_all, rows_all)             # every body's rows, as gathered
    pos, vel = pos_all[lo:lo + n_loc].clone(), vel_all[lo:lo + n_loc].clone()
    mass = mass_all[lo:lo + n_loc].contiguous()
    send = fmt.rows(n_loc, dev)
    ws = fmt.shard_workspace(n, lo, n_loc, dev)
    state = fmt.new_state(n_loc, dev)
    fmt.pack_rows(pos, vel, mass, send)
    fmt.local(send, n_loc, n, lo, eps2, ws)
    fmt.remote_force(rows_all, n, send, n_loc, lo, ws, state)

    def step(ev=None):
        if ev: ev[0].record()
        fmt.predict_step(pos, vel, mass, send, state)
        if ev: ev[1].record()
        rows_all[lo:lo + n_loc].copy_(send[:n_loc])                # stands in for the all-gather's arrival
        if ev: ev[2].record()
        fmt.local(send, n_loc, n, lo, eps2, ws)
        if ev: ev[3].record()
        fmt.remote_step(rows_all, n, send, n_loc, lo, ws, pos, vel, state)
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
    return {"n": n, "world": world, "rank": rank, "n_local": n_loc, "plan": fmt.plan(n, lo, n_loc),
            "rank_step_ms": step_ms, "phase_ms": phase}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rank", type=int, default=3)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--big", action="store_true", help="also BASELINE configs[4]'s rank shape: 65 536 of 524 288")
    ap.add_argument("--dtype", choices=sorted(FORMATS), default="float32")
    ap.add_argument("--integrator", choices=("hermite", "hermite6"), default="hermite",
                    help="hermite6: the 6th-order step (float64 only; --dtype is then float64)")
    ap.add_argument("--out", default=None, help="default: profiles/r11_hermite_shard.json, or "
                                                "profiles/r16_hermite_shard_f64.json with --dtype float64, or "
                                                "profiles/r22_hermite6_shard.json with --integrator hermite6")
    args = ap.parse_args()
    if args.integrator == "hermite6":
        args.dtype = "float64"
    fmt = Fmt6 if args.integrator == "hermite6" else FORMATS[args.dtype]
    out_path = args.out or os.path.join(ROOT, "profiles", fmt.out)
    dev = "cuda"
    results = []
    for n in [args.n] + ([args.n * args.world] if args.big else []):
        windows = args.windows if n == args.n else 3
        f_ms, s_ms = unsharded(fmt, n, dev, windows)
        r = rank_of(fmt, n, args.world, args.rank, dev, windows)
        r["dtype"], r["integrator"] = args.dtype, fmt.integrator
        ph = r["phase_ms"]
        r["unsharded_force_ms"], r["unsharded_step_ms"] = f_ms, s_ms
        r["force_ratio"] = (ph["force_local"] + ph["force_remote_finish_correct"]) / (f_ms / args.world)
        r["step_ratio"] = r["rank_step_ms"] / (s_ms / args.world)
        results.append(r)
        print(json.dumps(r), flush=True)
    out = {"tool": "tools/bench_hermite_shard.py", "device": torch.cuda.get_device_name(0),
           "what": "one emulated rank of the range-sharded Hermite step, no multi-rank transport (the all-gather is a "
                   "device copy); force_ratio = (local + remote) / (unsharded "
                   "force / world), step_ratio = rank step / (unsharded step / world), same process", "results": results}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
