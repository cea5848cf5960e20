"""One rank's share of a block step divided over 8 ranks (csrc/direct_hermite_block_split_f64.hip), emulated on ONE GPU,
against the un-divided float64 block step measured in the same process (the yardstick; there is no gate). For n bodies of a
Plummer sphere and n_act of them due, the un-divided step is nbd_hblock_step_f64 / nbd_hblock6_step_f64 (predict, force,
correct); the rank's share of the divided one is what BlockHermiteSimulator._split_step issues --

    order list | predict | header + slice list, force of the slice, rows | [exchange: here a device copy] | apply

-- for rank 0, whose slice is never shorter than another's. HIP-event times, medians over windows, after a time-based
warm-up. The schedule is planted: max_level = 1, the first n_act bodies at level 1, the rest at level 0, tick 0, so the block
step to tick 1 lists exactly n_act bodies; eta is huge, so no level ever moves and every repetition does the same work.
Writes profiles/r26_hermite_block_split.json:   python tools/bench_hermite_block_split.py [--n 16384 65536] [--fine]
No multi-rank transport is in any of these numbers: the all-gather is a device copy of the rank's own piece."""
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
from galaxify.simulation import BlockHermiteSimulator
from nbd import direct
from nbd.plummer import generate_plummer

G, EPS2, DT, ETA, K, WORLD = 1.0, 0.01, 1e-3, 1e12, 1, 8
F64 = torch.float64


def warm(fn, seconds=0.3):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:                   # clock ramp
        for _ in range(5):
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


class Planted:
    """State, levels and a schedule record with exactly n_act bodies due at tick 1, and both forms of that block step."""

    def __init__(self, order, n, n_act, dev):
        self.order, self.n, self.n_act = order, n, n_act
        p, v, m = generate_plummer(n, seed=1234)
        self.state = [torch.tensor(a, dtype=F64, device=dev) for a in (p, v)]
        self.state += [torch.zeros((n, 3), dtype=F64, device=dev) for _ in range(2 if order == 4 else 4)]
        self.mass = torch.tensor(m, dtype=F64, device=dev)
        self.rows = tuple(direct.alloc_rows_f64(n, dev) for _ in range(2 if order == 4 else 3))
        self.levels = torch.zeros(n, dtype=torch.int32, device=dev)
        self.levels[:n_act] = 1
        self.ticks = torch.zeros(n, dtype=torch.int32, device=dev)
        sched = torch.zeros(direct.HBLOCK_SCHED_INTS, dtype=torch.int32)
        sched[8], sched[9] = n - n_act, n_act
        self.sched = sched.to(dev)
        self.ws = direct.hblock_split_workspace(n, dev, order)
        host = torch.zeros(4, dtype=torch.int32).pin_memory()
        direct.hblock_schedule(self.levels, K, self.sched, self.ws, host_sched=host)
        assert (int(host[0]), int(host[1])) == (1, n_act), host
        self.slices = direct.hblock_split_slices(n_act, WORLD)
        self.q = direct.hblock_split_q(self.slices)
        width = direct.HBLOCK_SPLIT_ROW if order == 4 else direct.HBLOCK6_SPLIT_ROW
        self.send = torch.zeros((1 + self.q, width), dtype=F64, device=dev)
        self.recv = torch.zeros((WORLD * (1 + self.q), width), dtype=F64, device=dev)
        self.step_entry = direct.hblock_step_f64 if order == 4 else direct.hblock6_step_f64
        self.predict_entry = direct.hblock_predict_f64 if order == 4 else direct.hblock6_predict_f64
        # every piece once, so that the apply reads sound rows of all ranks
        direct.hblock_order_list(self.levels, K, self.sched, self.ws)
        self.predict()
        for r, (first, count) in enumerate(self.slices):
            self.rows_of(first, count, self.recv[r * (1 + self.q):(r + 1) * (1 + self.q)])

    def predict(self):
        self.predict_entry(*self.state, self.mass, self.ticks, self.levels, K, DT, self.sched, *self.rows)

    def rows_of(self, first, count, out):
        direct.hblock_split_rows(tuple(self.state[:4 if self.order == 4 else 5]), self.levels, self.n_act, first, count,
                                 K, DT, ETA, EPS2, G, self.sched, self.rows, out, self.ws)

    def undivided(self):
        self.step_entry(*self.state, self.mass, self.ticks, self.levels, self.n_act, K, DT, ETA, EPS2, G, self.sched,
                        *self.rows, self.ws)

    def divided(self, ev=None):
        first, count = self.slices[0]
        if ev: ev[0].record()
        direct.hblock_order_list(self.levels, K, self.sched, self.ws)
        if ev: ev[1].record()
        self.predict()
        if ev: ev[2].record()
        self.rows_of(first, count, self.send)
        if ev: ev[3].record()
        self.recv[:1 + self.q].copy_(self.send)                    # stands in for the all-gather's arrival
        if ev: ev[4].record()
        direct.hblock_split_apply(self.recv, WORLD, self.q, self.n_act, tuple(self.state), self.mass, self.ticks,
                                  self.levels, K, self.sched, self.rows[0], self.ws)
        if ev: ev[5].record()


PHASES = ["order_list", "predict", "header_force_rows", "exchange_stand_in_copy", "apply"]


def measure(order, n, n_act, dev, windows):
    case = Planted(order, n, n_act, dev)
    est_ms = 0.1 + 6.0 * (n / 65536) * (n_act / 65536) * (1.5 if order == 6 else 1.0)
    reps = max(2, min(50, int(40.0 / est_ms)))
    warm(case.undivided)
    undivided_ms = window_ms(case.undivided, reps, windows)
    case = Planted(order, n, n_act, dev)                          # a fresh state for the other form
    warm(case.divided)
    divided_ms = window_ms(case.divided, reps, windows)
    samples = {k: [] for k in PHASES}
    for _ in range(max(windows * 3, 15)):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        case.divided(ev)
        torch.cuda.synchronize()
        for i, k in enumerate(PHASES):
            samples[k].append(ev[i].elapsed_time(ev[i + 1]))
    flag = int(case.sched.cpu()[direct.HBLOCK_SCHED_DIVERGED])
    assert flag == 0, "the planted pieces' headers disagree with the record"
    return {"order": order, "n": n, "n_act": n_act, "world": WORLD, "rank": 0, "slice": list(case.slices[0]),
            "q": case.q, "undivided_ms": undivided_ms, "rank_share_ms": divided_ms,
            "ratio_to_undivided_over_world": divided_ms / (undivided_ms / WORLD),
            "divided_wins": divided_ms < undivided_ms,
            "phase_ms": {k: statistics.median(s) for k, s in samples.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[16384, 65536])
    ap.add_argument("--orders", type=int, nargs="+", default=[4, 6], choices=(4, 6))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--fine", action="store_true", help="also n_act = 256, 512, 2048, 4096: where the crossover lies")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_hermite_block_split.json"))
    args = ap.parse_args()
    dev = "cuda"
    results, crossover = [], {}
    for order in args.orders:
        for n in args.n:
            counts = sorted({128, 1024, 8192, n} | ({256, 512, 2048, 4096} if args.fine else set()))
            rows = [measure(order, n, n_act, dev, args.windows) for n_act in counts if n_act <= n]
            for r in rows:
                print(json.dumps(r), flush=True)
            wins = [r["n_act"] for r in rows if r["divided_wins"]]
            crossover[f"order{order}_n{n}"] = {
                "smallest_measured_n_act_where_divided_wins": min(wins) if wins else None,
                "default_split_min_active": BlockHermiteSimulator.default_split_min_active(n, WORLD),
                "issue_model_max_64P_2p26_over_n": max(64 * WORLD, -(-(1 << 26) // n))}
            results += rows
    out = {"tool": "tools/bench_hermite_block_split.py", "device": torch.cuda.get_device_name(0),
           "what": "rank 0 of 8 emulated ranks of a divided float64 block step against the un-divided block step, same "
                   "process; no multi-rank transport (the all-gather is a device copy of the rank's piece); "
                   "ratio_to_undivided_over_world = rank share / (un-divided / 8); divided_wins = rank share < "
                   "un-divided, i.e. before any exchange latency", "crossover": crossover, "results": results}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
