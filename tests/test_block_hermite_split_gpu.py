"""Block steps divided over the ranks of a process group on the MI355X (csrc/direct_hermite_block_split_f64.hip;
BlockHermiteSimulator(dtype=torch.float64, process_group=) and BlockHermite6Simulator(process_group=)): the ordered list,
emulated ranks through nbd.direct bit for bit against the un-divided simulators where one slab serves every count
(n = 256), slices at their own slab count at the fp64 oracles' bars, the rows entry read-only and deterministic, the header
guard, the one-rank group and two real ranks over gloo. Every workspace and row buffer is NaN-filled before a call."""
import functools
import os
import time

import numpy as np
import pytest
import torch

import block_hermite6_cases as c6
import block_hermite_f64_cases as bc
import hermite6_oracle as h6
import hermite_f64_oracle as fo
import test_hermite6_shard_gpu as shard6
import test_hermite_shard_f64_gpu as shard4

pytestmark = pytest.mark.gpu

F64 = torch.float64
NAN = float("nan")
G, EPS = 1.0, 0.05
T_NEXT, N_ACT, CLAMPED, T_CUR, CURSOR, DONE, DIVERGED, HIST = 0, 1, 2, 3, 4, 5, 6, 8      # the schedule record
STATE = {4: ("positions", "velocities", "accelerations", "jerks"),
         6: ("positions", "velocities", "accelerations", "jerks", "snaps", "crackles")}
CASES = {4: bc, 6: c6}
CLS = {4: "BlockHermiteSimulator", 6: "BlockHermite6Simulator"}


def _np(t):
    return t.detach().cpu().numpy()


def _nan_fill(ws):
    ws[: ws.numel() // 8 * 8].view(F64).fill_(NAN)
    return ws


def _sim(order, x, v, m, **kw):
    from galaxify import simulation
    kw.setdefault("g_const", G); kw.setdefault("softening", EPS); kw.setdefault("calc_energy", False)
    if order == 4:
        kw.setdefault("dtype", F64)
    sim = getattr(simulation, CLS[order])(positions=x, velocities=v, masses=m, device="cuda", **kw)
    _nan_fill(sim._hws)
    _nan_fill(sim._bws)
    return sim


def _planted_sim(order, eps, **kw):
    x, v, m = CASES[order].planted(eps)
    return _sim(order, x, v, m, g_const=1.0, softening=eps, dt=bc.DT, eta=bc.ETA, max_level=bc.K, **kw)


class Hand:
    """The state of a freshly built un-divided simulator, copied, and the block steps driven by hand through nbd.direct
    with `world` emulated ranks: all slices of a block step from the same pre-step state into one buffer, then apply."""

    def __init__(self, order, sim):
        from nbd import direct
        self.direct, self.order, self.n, self.dev = direct, order, sim.n, sim.device
        self.state = tuple(getattr(sim, name).clone() for name in STATE[order])
        self.mass, self.levels, self.ticks, self.sched = sim.masses, sim.levels.clone(), sim._ticks.clone(), sim._sched.clone()
        self.K, self.dt, self.eta = sim.max_level, sim.dt, sim.eta
        self.eps2, self.g = float(sim.softening) ** 2, float(sim.g_const)
        self.rows = tuple(direct.alloc_rows_f64(self.n, self.dev) for _ in range(2 if order == 4 else 3))
        self.width = direct.HBLOCK_SPLIT_ROW if order == 4 else direct.HBLOCK6_SPLIT_ROW
        self.ws = _nan_fill(direct.hblock_split_workspace(self.n, self.dev, order))
        self.host = torch.zeros(4, dtype=torch.int32).pin_memory()
        self.block_steps = 0

    def rows_in(self):
        return self.state[:4] if self.order == 4 else self.state[:5]

    def schedule(self):
        """schedule + order + predict of the next block step -> (t_next, n_act)."""
        d = self.direct
        d.hblock_schedule(self.levels, self.K, self.sched, self.ws, host_sched=self.host)
        d.hblock_order_list(self.levels, self.K, self.sched, self.ws)
        if self.order == 4:
            d.hblock_predict_f64(*self.state, self.mass, self.ticks, self.levels, self.K, self.dt, self.sched, *self.rows)
        else:
            d.hblock6_predict_f64(*self.state, self.mass, self.ticks, self.levels, self.K, self.dt, self.sched, *self.rows)
        return int(self.host[0]), int(self.host[1])

    def slice_rows(self, n_act, first, count, out=None, fill=NAN):
        out = torch.full((1 + count, self.width), fill, dtype=F64, device=self.dev) if out is None else out
        self.direct.hblock_split_rows(self.rows_in(), self.levels, n_act, first, count, self.K, self.dt, self.eta,
                                      self.eps2, self.g, self.sched, self.rows, out, self.ws)
        return out

    def pieces(self, n_act, world):
        d = self.direct
        slices = d.hblock_split_slices(n_act, world)
        q = d.hblock_split_q(slices)
        buf = torch.full((world * (1 + q), self.width), NAN, dtype=F64, device=self.dev)
        for r, (first, count) in enumerate(slices):
            self.slice_rows(n_act, first, count, out=buf[r * (1 + q):(r + 1) * (1 + q)])
        return buf, q

    def apply(self, buf, world, q, n_act):
        self.direct.hblock_split_apply(buf, world, q, n_act, self.state, self.mass, self.ticks, self.levels, self.K,
                                       self.sched, self.rows[0], self.ws)
        self.block_steps += 1

    def interval(self, world, before_last=None):
        end = 1 << self.K
        for _ in range(end):
            t_next, n_act = self.schedule()
            if t_next == end and before_last is not None:
                before_last(n_act)
            buf, q = self.pieces(n_act, world)
            self.apply(buf, world, q, n_act)
            if t_next == end:
                return
        raise AssertionError("interval not finished")

    def same_as(self, sim, tag):
        for name, mine in zip(STATE[self.order], self.state):
            assert torch.equal(mine, getattr(sim, name)), (tag, name)
        assert torch.equal(self.levels, sim.levels) and torch.equal(self.ticks, sim._ticks), tag
        mine, theirs = _np(self.sched), _np(sim._sched)
        assert mine[CLAMPED] == theirs[CLAMPED] and np.array_equal(mine[HIST:], theirs[HIST:]), tag
        assert mine[T_CUR] == theirs[T_CUR] and mine[DIVERGED] == 0 and theirs[DIVERGED] == 0, tag
        assert mine[CURSOR] == 0 and mine[DONE] == 0, tag
        assert self.block_steps == sim.block_steps, (tag, self.block_steps, sim.block_steps)


# ---------------------------------------------------------------- 1. the ordered list
@pytest.mark.parametrize("tick", [0, 6])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000, 5000])
def test_the_list_is_put_in_ascending_index(gpu_device, n, tick):
    from nbd import direct
    K = 4
    levels = np.random.default_rng(1000 * n + tick).integers(0, K + 1, n).astype(np.int32)
    sched = np.zeros(direct.HBLOCK_SCHED_INTS, np.int32)
    sched[T_CUR] = tick
    sched[HIST:HIST + K + 1] = np.bincount(levels, minlength=K + 1)
    t_next = min((tick // (1 << (K - k)) + 1) * (1 << (K - k)) for k in range(K + 1) if sched[HIST + k])
    thr = max(0, K - ((t_next & -t_next).bit_length() - 1))
    want = np.flatnonzero(levels >= thr).astype(np.int32)
    lev, rec = torch.tensor(levels, device=gpu_device), torch.tensor(sched, device=gpu_device)
    ws = _nan_fill(direct.hblock_split_workspace(n, gpu_device))
    host = torch.zeros(4, dtype=torch.int32).pin_memory()
    for again in (False, True):                         # the second round: the cursor and the finished count were left clean
        direct.hblock_schedule(lev, K, rec, ws, host_sched=host)
        assert (int(host[0]), int(host[1])) == (t_next, want.size)
        listed = _np(ws[:4 * want.size].view(torch.int32))
        assert np.array_equal(np.sort(listed), want), (n, tick, again)
        after_schedule = _np(rec)
        direct.hblock_order_list(lev, K, rec, ws)
        assert np.array_equal(_np(ws[:4 * want.size].view(torch.int32)), want), (n, tick, again)
        assert np.array_equal(_np(rec), after_schedule)                  # the record is read only
        assert after_schedule[CURSOR] == 0 and after_schedule[DONE] == 0 and after_schedule[DIVERGED] == 0
    assert np.array_equal(_np(lev), levels)


# ---------------------------------------------------------------- 2. emulated ranks, bit for bit (n = 256: one slab)
@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("eps", [0.0, 0.01])
@pytest.mark.parametrize("order", [4, 6])
def test_emulated_ranks_have_the_undivided_bits(gpu_device, order, eps, world):
    """One output step of the planted fixture: block steps with n_act = 2 (most slices empty) up to the full block."""
    plain = _planted_sim(order, eps)
    hand = Hand(order, plain)
    hand.same_as(plain, "start")
    seen = []
    real_schedule = hand.schedule

    def schedule():
        t_next, n_act = real_schedule()
        seen.append(n_act)
        return t_next, n_act
    hand.schedule = schedule
    hand.interval(world)
    plain.step()
    hand.same_as(plain, (order, eps, world))
    assert min(seen) == 2 and max(seen) == plain.n == 256 and sum(seen) * 256 == plain.pair_interactions
    assert all(torch.equal(hand.rows[0][i, :3], hand.state[0][i]) for i in (0, 255))          # posd = {x1, m}
    assert torch.equal(hand.rows[0][:256, 3], hand.mass)


@pytest.mark.parametrize("order", [4, 6])
def test_explicit_slices_of_a_full_block(gpu_device, order):
    """count in {0, 1, 63, 64, 65} at first in {0, 64, n_act - count} on the last block step of the interval, where every
    body is due: each piece is its header and the whole list's rows [first, first + count), bit for bit."""
    hand = Hand(order, _planted_sim(order, 0.01))
    checked = []

    def slices(n_act):
        assert n_act == 256
        whole = _np(hand.slice_rows(n_act, 0, n_act))
        assert not np.isnan(whole).any()
        for count in (0, 1, 63, 64, 65):
            for first in (0, 64, n_act - count):
                got = _np(hand.slice_rows(n_act, first, count))
                head = got[0].view(np.int32)
                assert list(head[:4]) == [1 << hand.K, n_act, first, count] and not got[0, 2:].any()
                assert np.array_equal(got[1:].view(np.int64), whole[1 + first:1 + first + count].view(np.int64))
                checked.append((first, count))
        slot = whole[1:, -1].copy().view(np.int32).reshape(-1, 2)
        assert (slot[:, 0] >= 0).all() and (slot[:, 0] <= hand.K).all() and set(slot[:, 1]) <= {0, 1}
        spare = whole[1:, 12:15] if order == 4 else whole[1:, 18:19]
        assert not spare.any()
    hand.interval(2, before_last=slices)
    assert len(checked) == 15


# ---------------------------------------------------------------- 3. the rows entry is read-only and deterministic
@pytest.mark.parametrize("order", [4, 6])
def test_rows_leave_the_state_alone_and_do_not_depend_on_the_buffers(gpu_device, order):
    hand = Hand(order, _planted_sim(order, 0.01))
    t_next, n_act = hand.schedule()
    assert 2 <= n_act < 256
    kept = [t.clone() for t in hand.state + (hand.levels, hand.ticks, hand.sched) + hand.rows]
    first = hand.slice_rows(n_act, 0, n_act, fill=NAN)
    hand.ws[_act_bytes(hand.n):].zero_()                # everything behind the ordered list: scratch, slice list, slabs
    second = hand.slice_rows(n_act, 0, n_act, fill=0.0)
    third = hand.slice_rows(n_act, 0, n_act, fill=0.0)
    assert np.array_equal(_np(first).view(np.int64), _np(second).view(np.int64))
    assert np.array_equal(_np(second).view(np.int64), _np(third).view(np.int64))
    for before, after in zip(kept, hand.state + (hand.levels, hand.ticks, hand.sched) + hand.rows):
        assert torch.equal(before.view(torch.int32 if before.dtype == torch.int32 else torch.int64),
                           after.view(torch.int32 if after.dtype == torch.int32 else torch.int64))


def _act_bytes(n):
    return -(-n // 8) * 32


# ---------------------------------------------------------------- 4. slices at their own slab count
@functools.lru_cache(maxsize=None)
def _sphere(n):
    x, v, m = fo.plummer_case(n, seed=900 + n)
    for arr in (x, v, m):
        arr.setflags(write=False)
    return x, v, m


@functools.lru_cache(maxsize=None)
def _bars(order, n, dt, steps):
    """The step bars of the range-sharded tests (8 s_k + 8 * 2^-53 max|value|), built once per order and size."""
    x, v, m = _sphere(n)
    if order == 4:
        return shard4._step_bars(x, v, m, G, EPS * EPS, dt, (steps,))
    return shard6._step_bars(x, v, m, EPS * EPS, dt, (steps,))


_FORCE_REF = {}     # (order, n) -> the predicted rows of the first step and the oracles' sums on them, computed once


def _check_force_rows(tag, order, whole, x_p, v_p, a_p, m):
    """a1, j1 (s1) of every row against the fp64 oracles on the predicted rows the kernel read, at their bars. The
    predicted rows do not depend on the rank count, so the oracles run once per order and size."""
    n = m.shape[0]
    if (order, n) not in _FORCE_REF:
        ref = [x_p, v_p, a_p, *fo.accel_jerk(x_p, v_p, m, G, EPS * EPS), *fo.accel_jerk_abs(x_p, v_p, m, G, EPS * EPS)]
        if order == 6:
            ref += list(h6.snap_and_abs(x_p, v_p, a_p, m, G, EPS * EPS))
        _FORCE_REF[order, n] = ref
    x_r, v_r, a_r, a, j, sa, sj, *snap = _FORCE_REF[order, n]
    assert np.array_equal(x_r, x_p) and np.array_equal(v_r, v_p) and (order == 4 or np.array_equal(a_r, a_p))
    ok_a, fa = fo.within(whole[:, 6:9], a, n, sa)
    ok_j, fj = fo.within(whole[:, 9:12], j, 4 * n, sj)
    print(f"{tag}: |a - ref| / bar = {fa:.3f}, |j - ref| / bar = {fj:.3f}")
    assert ok_a and ok_j, (tag, fa, fj)
    if order == 6:
        ok_s, fs = fo.within(whole[:, 12:15], snap[0], 19 * n, snap[1])
        print(f"{tag}: |s - ref| / bar = {fs:.3f}")
        assert ok_s, (tag, fs)


@pytest.mark.parametrize("world", [2, 8])
@pytest.mark.parametrize("n", [1000, 5000])
@pytest.mark.parametrize("order", [4, 6])
def test_slices_at_their_own_slab_count(gpu_device, order, n, world):
    """max_level = 0: every step is one full block, the list is 0..n-1, and a slice's plan has more slabs than the whole
    block's. The forces of the first step at the oracles' bars; the state after 3 steps at the step bars."""
    dt, steps = 0.01, 3
    x, v, m = _sphere(n)
    hand = Hand(order, _sim(order, x, v, m, dt=dt, max_level=0))
    for k in range(1, steps + 1):
        t_next, n_act = hand.schedule()
        assert (t_next, n_act) == (1, n)
        buf, q = hand.pieces(n_act, world)
        if k == 1:
            rows = _np(buf).reshape(world, 1 + q, -1)[:, 1:].reshape(world * q, -1)[:n]
            pred = [_np(r)[:n] for r in hand.rows]
            assert np.array_equal(pred[0][:, 3], m)
            _check_force_rows(f"order {order} n={n} P={world}", order, rows, pred[0][:, :3], pred[1][:, :3],
                              pred[2][:, :3] if order == 6 else None, m)
        hand.apply(buf, world, q, n_act)
        assert _np(hand.sched)[DIVERGED] == 0
    names = ("pos", "vel", "acc", "jerk", "snap")[:4 if order == 4 else 5]
    check = shard4._check_steps if order == 4 else shard6._check_steps
    check(f"order {order} n={n} P={world}", steps, _bars(order, n, dt, steps), [_np(t) for t in hand.state[:len(names)]])
    assert _np(hand.levels).max() == 0 and not _np(hand.ticks).any()


# ---------------------------------------------------------------- 5. the header guard
@pytest.mark.parametrize("order", [4, 6])
def test_a_doctored_header_raises_the_flag(gpu_device, order):
    hand = Hand(order, _planted_sim(order, 0.01))
    t_next, n_act = hand.schedule()
    buf, q = hand.pieces(n_act, 2)
    assert _np(hand.sched)[DIVERGED] == 0
    head = buf[1 + q].view(torch.int32)
    assert head[:4].tolist() == [t_next, n_act, min(q, n_act), max(0, n_act - q)]
    head[1] = n_act + 1
    hand.apply(buf, 2, q, n_act)
    assert _np(hand.sched)[DIVERGED] != 0
    assert _np(hand.ticks).max() == t_next                               # the state is written all the same


@pytest.fixture
def one_rank_group(tmp_path, monkeypatch):
    """A one-rank gloo group with NBD_FORCE_SHARDED=1: the divided block step end to end in this process, the exchange
    through the collective."""
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    monkeypatch.setenv("NBD_FORCE_SHARDED", "1")
    try:
        yield dist.group.WORLD
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("order", [4, 6])
def test_step_raises_when_the_replicas_diverge(gpu_device, order, one_rank_group, monkeypatch):
    from nbd import direct
    sim = _planted_sim(order, 0.01, process_group=one_rank_group, split_min_active=1)
    real = direct.hblock_split_rows

    def doctored(state, levels, n_act, first, count, *rest):
        real(state, levels, n_act, first, count, *rest)
        rows_out = rest[-2]
        rows_out[0].view(torch.int32)[0] += 1                            # another rank's t_next
    monkeypatch.setattr(direct, "hblock_split_rows", doctored)
    with pytest.raises(RuntimeError, match="replicas"):
        sim.step()


# ---------------------------------------------------------------- 6. the one-rank group
def _same_run(a, b):
    assert len(a) == len(b)
    for p, q in zip(a, b):
        for name in ("positions", "velocities", "accelerations"):
            assert torch.equal(getattr(p, name), getattr(q, name)), name
        assert (p.u_energy, p.k_energy, p.invariants) == (q.u_energy, q.k_energy, q.invariants)
        assert p.u_energy is not None and p.invariants is not None


@pytest.mark.parametrize("order", [4, 6])
def test_one_rank_group_has_the_undivided_bits(gpu_device, order, one_rank_group, monkeypatch):
    kw = dict(calc_energy=True, calc_invariants=True)
    plain = _planted_sim(order, 0.01, **kw)
    split = _planted_sim(order, 0.01, process_group=one_rank_group, split_min_active=1, **kw)
    assert split._split and split._pieces.collective and not split._sharded and not plain._split
    assert split.process_group is one_rank_group and plain.split_min_active is None

    def same(tag):
        for name in STATE[order] + ("levels", "_ticks"):
            assert torch.equal(getattr(split, name), getattr(plain, name)), (tag, name)
            assert getattr(split, name).shape[0] == 256                  # the full arrays on the rank
        for name in ("block_steps", "pair_interactions", "clamped"):
            assert getattr(split, name) == getattr(plain, name), (tag, name)
        assert split.split_block_steps == split.block_steps and split.exchanged_rows * 256 == split.pair_interactions
        assert torch.equal(split.gather("positions"), plain.positions)
        assert split.compute_energies() == plain.compute_energies()
        assert torch.equal(split.compute_potentials(), plain.compute_potentials())
        assert split.compute_invariants() == plain.compute_invariants()
    same("start")
    for k in range(2):
        plain.step()
        split.step()
        same(k)
    _same_run(split.run(3), plain.run(3))
    same("run")
    assert plain.split_block_steps == 0 and plain.exchanged_rows == 0

    # a threshold no block reaches: no collective is ever called, and the bits are the un-divided ones again
    import torch.distributed as dist

    def never(*a, **k):
        raise AssertionError("all_gather_into_tensor was called")
    lazy = _planted_sim(order, 0.01, process_group=one_rank_group, split_min_active=257, **kw)
    fresh = _planted_sim(order, 0.01, **kw)
    monkeypatch.setattr(dist, "all_gather_into_tensor", never)
    for _ in range(2):
        lazy.step()
        fresh.step()
    for name in STATE[order] + ("levels", "_ticks"):
        assert torch.equal(getattr(lazy, name), getattr(fresh, name)), name
    assert lazy.split_block_steps == 0 and lazy.exchanged_rows == 0 and lazy.block_steps == fresh.block_steps
    assert lazy.split_min_active == 257 and lazy._split


# ---------------------------------------------------------------- 7. two real ranks
COUNTERS = ("block_steps", "pair_interactions", "clamped", "split_block_steps", "exchanged_rows")


def _inputs(order, n):
    if n == 256:
        x, v, m = CASES[order].planted(0.01)
        return x, v, m, dict(g_const=1.0, softening=0.01, dt=bc.DT, eta=bc.ETA, max_level=bc.K)
    x, v, m = _sphere(n)
    return x, v, m, dict(g_const=G, softening=EPS, dt=0.01, max_level=0)


def _saved(sim, order):
    out = {name: _np(getattr(sim, name)) for name in STATE[order] + ("levels",)}
    out.update({name: np.int64(getattr(sim, name)) for name in COUNTERS})
    return out


def _two_rank_worker(rank, world, port, order, n, steps, out_dir):
    import datetime
    import sys
    import torch.distributed as dist
    from conftest import PKG, ROOT
    for p in (PKG, ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=120))
    try:
        x, v, m, kw = _inputs(order, n)
        sim = _sim(order, x, v, m, process_group=dist.group.WORLD, split_min_active=1, **kw)
        assert sim._split and not sim._sharded and sim.positions.shape == (n, 3) and sim._split_world == 2
        for _ in range(steps):
            sim.step()
        np.savez(os.path.join(out_dir, f"split{rank}.npz"), **_saved(sim, order))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n", [256, 1001])
@pytest.mark.parametrize("order", [4, 6])
def test_two_rank_block_steps_on_gpu(order, n, tmp_path, gpu_device):
    """The real path (HIP kernels, PieceExchange, one all-gather per divided block step) with two processes sharing this
    GPU over gloo. n = 256 (the planted fixture, two output steps): one slab for every count, so both ranks hold the
    un-divided run's bits. n = 1001, max_level = 0, 3 steps: the ranks equal each other, the state at the step bars."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    steps = 2 if n == 256 else 3
    x, v, m, kw = _inputs(order, n)
    bars = None if n == 256 else _bars(order, n, 0.01, steps)
    ctx = mp.spawn(_two_rank_worker, args=(2, port, order, n, steps, str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + 240.0
    try:
        while not ctx.join(timeout=5.0):                       # returns as soon as a worker ends; raises if one failed
            assert time.monotonic() < deadline, "the two ranks did not finish in time"
    finally:
        for proc in ctx.processes:
            if proc.is_alive():
                proc.kill()
    got = [np.load(tmp_path / f"split{r}.npz") for r in (0, 1)]
    keys = STATE[order] + ("levels",) + COUNTERS
    for key in keys:
        assert np.array_equal(got[0][key], got[1][key]), key              # every rank holds the same arrays and counters
    assert got[0]["split_block_steps"] == got[0]["block_steps"] > 0
    if n == 256:
        plain = _sim(order, x, v, m, **kw)
        for _ in range(steps):
            plain.step()
        want = _saved(plain, order)
        for key in STATE[order] + ("levels", "block_steps", "pair_interactions", "clamped"):
            assert np.array_equal(got[0][key], want[key]), key
    else:
        assert got[0]["split_block_steps"] == 3 and got[0]["exchanged_rows"] == 3 * n
        names = ("pos", "vel", "acc", "jerk", "snap")[:4 if order == 4 else 5]
        check = shard4._check_steps if order == 4 else shard6._check_steps
        check(f"two ranks order {order} n={n}", steps, bars, [got[0][key] for key in STATE[order][:len(names)]])
