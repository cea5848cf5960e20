"""Range-sharded 6th-order Hermite step (csrc/direct_hermite_shard_f64.hip, Hermite6Simulator(process_group=...)) on the
GPU against the fp64 oracles. The force at the bars of tests/hermite_f64_oracle.py and tests/hermite6_oracle.py:
|got - ref| <= (T + 32) 2^-53 sum|terms|, T = n_total for the acceleration, 4 n_total for the jerk and 19 n_total for the
snap -- any-order bounds, so they hold for the sharded order (own block, then the others) as for the un-sharded one. The
step at the project's step bar, 8 s_k + 8 * 2^-53 max|ref|, s_k = the largest difference between the oracle run and the
oracle run on permuted bodies. No input is fp32-representable, masses are ragged, G = 1, eps = 0.05 unless stated, and
every workspace is NaN-filled before a call. Emulated ranks through the C-ABI in one process (force, explicit splits,
masks, determinism, the un-sharded kernel's and the 4th-order sharded kernels' bits, the full step), two real processes
over gloo, and the one-rank group."""
import functools
import os
import time

import numpy as np
import pytest
import torch

import hermite6_oracle as h6
import hermite_f64_oracle as fo
import hermite_oracle as ho

pytestmark = pytest.mark.gpu

G, EPS = 1.0, 0.05
F64 = torch.float64
NAMES = ("pos", "vel", "acc", "jerk", "snap")


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, device):
    return torch.tensor(np.asarray(a, np.float64), dtype=F64, device=device)


def _ragged(n, seed):
    x, v, m = fo.plummer_case(n, seed=seed)
    return x, v, m * np.random.default_rng(1).uniform(0.5, 2.0, n)


@functools.lru_cache(maxsize=None)
def _case(n):
    """(x, v, m, a, j, s, sum|a terms|, sum|j terms|, sum|s terms|) of the oracles, the snap on the oracle's a as the
    third row pair; computed once and never written to."""
    x, v, m = _ragged(n, 700 + n)
    a, j = fo.accel_jerk(x, v, m, G, EPS * EPS)
    sa, sj = fo.accel_jerk_abs(x, v, m, G, EPS * EPS)
    s, ss = h6.snap_and_abs(x, v, a, m, G, EPS * EPS)
    out = (x, v, m, a, j, s, sa, sj, ss)
    for arr in out:
        arr.setflags(write=False)
    return out


def _gathered_rows(x, v, a, m, device):
    """The array every rank holds after the exchange, built with the un-sharded pack and device copies."""
    from nbd import direct
    n = x.shape[0]
    posd, veld, accd = (direct.alloc_rows_f64(n, device) for _ in range(3))
    direct.hermite6_pack(_dev(x, device), _dev(v, device), _dev(m, device), posd, veld, accd,
                         acc=None if a is None else _dev(a, device))
    rows = direct.alloc_hermite6_rows_f64(n, device)
    assert rows.shape == (direct.padded_len(n), 12) and not rows.any()
    rows[:, 0:4].copy_(posd)
    rows[:, 4:8].copy_(veld)
    rows[:, 8:12].copy_(accd)
    return rows


def _send_of(rows_all, part):
    from nbd import direct
    send = direct.alloc_hermite6_rows_f64(part.n_local, rows_all.device)
    send[:part.n_local].copy_(rows_all[part.lo:part.hi])
    return send


def _parts(n, world):
    from nbd.dist import RangePartition
    return [RangePartition(n, world, r) for r in range(world)]


def _ws_bytes(n, part, sl=0, sr=0):
    from nbd import direct
    return direct._lib.lib().nbd_hermite6_shard_f64_workspace_bytes(n, part.lo, part.n_local, sl, sr)


def _nan_ws(nbytes, device):
    return torch.full((nbytes // 8 + 2,), float("nan"), dtype=F64, device=device).view(torch.uint8)


def _nan3(n, device, count=3):
    return tuple(torch.full((n, 3), float("nan"), dtype=F64, device=device) for _ in range(count))


def _rank_force(rows_all, n, part, ws=None, send=None, sl=0, sr=0):
    """(a, j, s) of one emulated rank: local then remote, force only, the workspace NaN-filled unless one is given."""
    from nbd import direct
    dev = rows_all.device
    send = _send_of(rows_all, part) if send is None else send
    ws = _nan_ws(_ws_bytes(n, part, sl, sr), dev) if ws is None else ws
    out = _nan3(part.n_local, dev)
    direct.hermite6_shard_force_local_f64(send, part.n_local, n, part.lo, EPS * EPS, ws, slabs=sl)
    direct.hermite6_shard_force_remote_f64(rows_all, n, send, part.n_local, part.lo, EPS * EPS, G, *out, ws,
                                           slabs_local=sl, slabs_remote=sr)
    return out


def _rank_force4(rows_all, n, part, sl=0, sr=0):
    """(a, j) of the 4th-order sharded entries on the first two quad pairs of the same rows, at the same slab counts."""
    from nbd import direct
    dev = rows_all.device
    rows8 = direct.alloc_hermite_rows_f64(n, dev)
    rows8.copy_(rows_all[:, 0:8])
    send = direct.alloc_hermite_rows_f64(part.n_local, dev)
    send[:part.n_local].copy_(rows8[part.lo:part.hi])
    ws = _nan_ws(direct._lib.lib().nbd_hermite_shard_f64_workspace_bytes(n, part.lo, part.n_local, sl, sr), dev)
    acc, jerk = _nan3(part.n_local, dev, 2)
    direct.hermite_shard_force_local_f64(send, part.n_local, n, part.lo, EPS * EPS, ws, slabs=sl)
    direct.hermite_shard_force_remote_f64(rows8, n, send, part.n_local, part.lo, EPS * EPS, G, acc, jerk, ws,
                                          slabs_local=sl, slabs_remote=sr)
    return acc, jerk


def _check_rank(tag, part, got, case):
    x, v, m, a, j, s, sa, sj, ss = case
    n = x.shape[0]
    own = slice(part.lo, part.hi)
    acc, jerk, snap = (_np(t) for t in got)
    assert np.isfinite(acc).all() and np.isfinite(jerk).all() and np.isfinite(snap).all(), tag
    ok_a, fa = fo.within(acc, a[own], n, sa[own])
    ok_j, fj = fo.within(jerk, j[own], 4 * n, sj[own])
    ok_s, fs = fo.within(snap, s[own], 19 * n, ss[own])
    print(f"{tag} rank={part.rank} lo={part.lo} n_local={part.n_local}: / bar: a {fa:.3f}, j {fj:.3f}, s {fs:.3f}")
    assert ok_a and ok_j and ok_s, (tag, part.rank, fa, fj, fs)


def _check_ranks(n, world, device, sl=0, sr=0, predict=True, fourth=False):
    from nbd import direct
    case = _case(n)
    x, v, m, a = case[:4]
    rows_all = _gathered_rows(x, v, a, m, device)
    pos, vel, mass, acc0 = (_dev(t, device) for t in (x, v, m, a))
    for part in _parts(n, world):
        own = slice(part.lo, part.hi)
        send = None
        if predict:
            # the predict entry with no derivatives is the plain pack of the rank's rows, zero behind them
            send = direct.alloc_hermite6_rows_f64(part.n_local, device)
            send.fill_(float("nan"))
            direct.hermite6_shard_predict_f64(pos[own].contiguous(), vel[own].contiguous(), mass[own].contiguous(), send,
                                              acc=acc0[own].contiguous())
            assert torch.equal(send[:part.n_local], rows_all[own]) and not send[part.n_local:].any()
        if part.n_local == 0:
            # a no-op returning success, workspace or not
            empty = direct.alloc_hermite6_rows_f64(0, device)
            out = _nan3(0, device)
            direct.hermite6_shard_force_local_f64(empty, 0, n, part.lo, EPS * EPS, _nan_ws(16, device))
            direct.hermite6_shard_force_remote_f64(rows_all, n, empty, 0, part.lo, EPS * EPS, G, *out,
                                                   _nan_ws(16, device))
            continue
        got = _rank_force(rows_all, n, part, send=send, sl=sl, sr=sr)
        _check_rank(f"n={n} P={world} slabs=({sl},{sr})", part, got, case)
        if fourth:
            a4, j4 = _rank_force4(rows_all, n, part, sl, sr)
            assert torch.equal(got[0], a4) and torch.equal(got[1], j4), (part.rank, sl, sr)


# n, P: 64/2 own range inside one chunk; 65/2 straddle + tail chunk of one body; 130/3 lo unaligned on every rank; 200/1
# no remote chunks; 3/8 ranks with n_local = 0; 1000/3 whole chunks skipped, both ends masked; 5000/3 several chunks around
# the skipped run
@pytest.mark.parametrize("n,world", [(64, 2), (65, 2), (130, 3), (200, 1), (3, 8), (1000, 3), (5000, 3)])
def test_emulated_ranks_force_at_the_bar(n, world, gpu_device):
    _check_ranks(n, world, gpu_device, fourth=(world == 3))


def test_predict_without_an_acceleration_leaves_a_zero_third_pair(gpu_device):
    from nbd import direct
    n = 130
    x, v, m = _case(n)[:3]
    rows = _gathered_rows(x, v, None, m, gpu_device)
    assert not rows[:, 8:12].any() and np.array_equal(_np(rows[:n, 0:3]), x)
    send = direct.alloc_hermite6_rows_f64(n, gpu_device)
    send.fill_(float("nan"))
    direct.hermite6_shard_predict_f64(_dev(x, gpu_device), _dev(v, gpu_device), _dev(m, gpu_device), send)
    assert torch.equal(send, rows)


# remote slabs 1: 130/3 waves without a chunk; 1000/3 a wave walks across the skipped run, both LDS buffers reused; 5000/3
# about 13 chunks per wave around the gap. 64 slabs at 5000: more waves than chunks. Local slabs: 1, and 3. The a and j of
# every rank are the 4th-order sharded entries' bits at the same split.
@pytest.mark.parametrize("n,world,sl,sr", [(130, 3, 1, 1), (1000, 3, 1, 1), (1000, 3, 3, 1), (1000, 3, 1, 3),
                                           (5000, 3, 1, 1), (5000, 3, 3, 1), (5000, 3, 1, 3), (5000, 3, 1, 64)])
def test_force_with_explicit_splits(n, world, sl, sr, gpu_device):
    _check_ranks(n, world, gpu_device, sl=sl, sr=sr, predict=False, fourth=True)


def test_plan_matches_the_workspace(gpu_device):
    from nbd import direct
    lib = direct._lib.lib()
    for n, lo, n_local in ((1000, 334, 333), (200, 0, 200), (524288, 196608, 65536), (65536, 8192, 8192)):
        p = direct.hermite6_shard_f64_plan(n, lo, n_local)
        assert p == direct.hermite_shard_f64_plan(n, lo, n_local)
        assert p["slabs_local"] >= 1 and (p["slabs_remote"] >= 1) == (n_local < n)
        need = (p["slabs_local"] + p["slabs_remote"]) * 9 * n_local * 8
        assert lib.nbd_hermite6_shard_f64_workspace_bytes(n, lo, n_local, 0, 0) == need
        assert direct.hermite6_shard_f64_workspace(n, lo, n_local, gpu_device).numel() >= need


@pytest.mark.parametrize("n", [130, 1000])
def test_own_rows_of_the_gathered_array_are_never_sources(n, gpu_device):
    """Mask by select, skip by chunk: the remote block gives the same bits whether rows [lo, hi) of the gathered array
    hold the real values, zeros or NaN; the padding behind n_total stays the zeros it was."""
    x, v, m, a = _case(n)[:4]
    rows_all = _gathered_rows(x, v, a, m, gpu_device)
    for part in _parts(n, 3):
        send = _send_of(rows_all, part)
        base = _rank_force(rows_all, n, part, send=send)
        for fill in (0.0, float("nan")):
            other = rows_all.clone()
            other[part.lo:part.hi] = fill
            got = _rank_force(other, n, part, send=send)
            assert all(torch.equal(g_, b) for g_, b in zip(got, base)), (part.rank, fill)
            assert not other[n:].any()
        assert all(torch.isfinite(b).all() for b in base)
        assert not rows_all[n:].any()


def test_deterministic_and_independent_of_rank_order(gpu_device):
    """The same call twice gives the same bits, and a rank's output does not depend on which ranks used the (shared,
    NaN-filled at first) workspace before it."""
    n, world = 1000, 3
    x, v, m, a = _case(n)[:4]
    rows_all = _gathered_rows(x, v, a, m, gpu_device)
    parts = _parts(n, world)
    ws = _nan_ws(max(_ws_bytes(n, p) for p in parts), gpu_device)
    first = {p.rank: _rank_force(rows_all, n, p, ws=ws) for p in parts}
    again = {p.rank: _rank_force(rows_all, n, p, ws=ws) for p in reversed(parts)}
    alone = {p.rank: _rank_force(rows_all, n, p) for p in parts}
    for r in first:
        for other in (again, alone):
            assert all(torch.equal(p, q) for p, q in zip(first[r], other[r])), r


@pytest.mark.parametrize("n,slabs", [(130, 1), (1000, 3)])
def test_a_rank_that_owns_everything_has_the_unsharded_bits(n, slabs, gpu_device):
    """n_local = n_total, lo = 0: local + finish only, against nbd_accel_jerk_snap_f64 at the same explicit slab count on
    rows packed from the same state -- one copy of every rounded operation, so the same bits."""
    from nbd import direct
    x, v, m, a = _case(n)[:4]
    posd, veld, accd = (direct.alloc_rows_f64(n, gpu_device) for _ in range(3))
    direct.hermite6_pack(_dev(x, gpu_device), _dev(v, gpu_device), _dev(m, gpu_device), posd, veld, accd,
                         acc=_dev(a, gpu_device))
    ref = direct.accel_jerk_snap_f64(posd, veld, accd, n, EPS * EPS, G, slabs=slabs,
                                     workspace=_nan_ws(slabs * 9 * n * 8, gpu_device))
    rows_all = _gathered_rows(x, v, a, m, gpu_device)
    part = _parts(n, 1)[0]
    assert _ws_bytes(n, part, slabs, 0) == slabs * 9 * n * 8                    # no remote slabs
    got = _rank_force(rows_all, n, part, sl=slabs)
    assert all(torch.equal(p, q) for p, q in zip(got, ref))


def _oracle_states(x, v, m, dt, eps2, marks):
    state = (np.array(x), np.array(v)) + h6.start(x, v, m, G, eps2)
    out = {}
    for k in range(1, max(marks) + 1):
        state = h6.hermite6_step(*state, m, dt, G, eps2)
        if k in marks:
            out[k] = state
    return out


def _step_bars(x, v, m, eps2, dt, counts, seed=11):
    """{k: [(name, reference, tolerance)]}: test_hermite6_gpu.py's step bar, 8 s_k + 8 * 2^-53 max|value|, s_k = the largest
    difference between the oracle run and the same run with the bodies permuted (measured here, on the CPU)."""
    n = x.shape[0]
    perm = np.random.default_rng(seed).permutation(n)
    back = np.empty_like(perm)
    back[perm] = np.arange(n)
    ref = _oracle_states(x, v, m, dt, eps2, counts)
    prm = _oracle_states(x[perm], v[perm], m[perm], dt, eps2, counts)
    return {k: [(name, r, 8 * np.abs(r - p[back]).max() + 8 * fo.U53 * np.abs(r).max())
                for name, r, p in zip(NAMES, ref[k], prm[k])] for k in counts}


def _check_steps(tag, k, bars, got):
    for (name, ref, tol), q in zip(bars[k], got):
        dist = np.abs(np.asarray(q) - ref).max()
        print(f"{tag} steps={k} {name}: |gpu - oracle| = {dist:.3e}, tolerance {tol:.3e}")
        assert dist <= tol, (tag, k, name, dist, tol)


def test_full_sharded_step_through_the_c_abi(gpu_device):
    """The oracle's start (a from rows with a zero third pair, then a, j, s from rows with that a; c = 0), then predict,
    local, remote + corrector for every emulated rank of n = 1000, P = 3, the exchange by device copies: after 1 and 10
    steps at the un-sharded 6th-order step's bar, the crackle of every step at its own."""
    from nbd import direct
    n, world, dt = 1000, 3, 0.01
    x, v, m = _case(n)[:3]
    dev = gpu_device
    bars = _step_bars(x, v, m, EPS * EPS, dt, (1, 10))
    pos, vel, mass = _dev(x, dev), _dev(v, dev), _dev(m, dev)
    parts = _parts(n, world)
    rows_all = _gathered_rows(x, v, None, m, dev)
    a0 = torch.cat([_rank_force(rows_all, n, p)[0] for p in parts])
    rows_all[:n, 8:11].copy_(a0)
    ranks = []
    for p in parts:
        acc, jerk, snap = _rank_force(rows_all, n, p)
        assert torch.equal(acc, a0[p.lo:p.hi])
        ranks.append(dict(part=p, pos=pos[p.lo:p.hi].clone(), vel=vel[p.lo:p.hi].clone(),
                          mass=mass[p.lo:p.hi].contiguous(), acc=acc, jerk=jerk, snap=snap,
                          crackle=torch.zeros_like(acc), send=direct.alloc_hermite6_rows_f64(p.n_local, dev),
                          ws=_nan_ws(_ws_bytes(n, p), dev)))

    def cat(key):
        return _np(torch.cat([r[key] for r in ranks]))
    for k in range(1, 11):
        before = [cat(key) for key in ("acc", "jerk", "snap")]
        for r in ranks:
            direct.hermite6_shard_predict_f64(r["pos"], r["vel"], r["mass"], r["send"], r["acc"], r["jerk"], r["snap"],
                                              r["crackle"], dt)
        for r in ranks:                                        # the exchange
            p = r["part"]
            rows_all[p.lo:p.hi].copy_(r["send"][:p.n_local])
        for r in ranks:
            p = r["part"]
            direct.hermite6_shard_force_local_f64(r["send"], p.n_local, n, p.lo, EPS * EPS, r["ws"])
            direct.hermite6_shard_force_remote_f64(rows_all, n, r["send"], p.n_local, p.lo, EPS * EPS, G, r["acc"],
                                                   r["jerk"], r["snap"], r["ws"], pos=r["pos"], vel=r["vel"],
                                                   acc_in=r["acc"], jerk_in=r["jerk"], snap_in=r["snap"],
                                                   crackle_out=r["crackle"], dt=dt)
        after = [cat(key) for key in ("acc", "jerk", "snap")]
        c_err = np.abs(cat("crackle") - h6.crackle(*before, *after, dt))
        c_tol = 16 * fo.U53 * h6.crackle_abs(*before, *after, dt)
        assert np.all(c_err <= c_tol), (k, float((c_err / c_tol).max()))
        if k in bars:
            _check_steps("emulated", k, bars, [cat(key) for key in NAMES])


KEYS = ("positions", "velocities", "accelerations", "jerks", "snaps")


def _two_rank_worker(rank, world, port, n, steps, out_dir):
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
        from galaxify import simulation
        x, v, m = _ragged(n, 700 + n)
        sim = simulation.Hermite6Simulator(positions=x, velocities=v, masses=m, dt=0.01, g_const=G, softening=EPS,
                                           calc_energy=True, device="cuda", process_group=dist.group.WORLD)
        assert sim._sharded and sim.snaps.shape == (sim.part.n_local, 3) and sim.snaps.dtype == torch.float64
        assert sim._rows_all.dtype == torch.float64 and sim._rows_all.shape[1] == 12 and not sim.crackles.any()
        for _ in range(steps):
            sim.step()
        u, k = sim.compute_energies()
        full = {key: sim.gather(key) for key in KEYS + ("crackles",)}
        assert all(t.dtype == torch.float64 for t in full.values())
        np.savez(os.path.join(out_dir, f"sharded{rank}.npz"), u=u, k=k, **{key: _np(t) for key, t in full.items()})
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n", [1024, 1001])
def test_two_rank_hermite6_on_gpu(n, tmp_path, gpu_device):
    """The real sharded path (HIP kernels, RowGather of 12-double rows, one all-gather per step) with two processes sharing
    this GPU over gloo: 3 steps at the step bar, the same global arrays on both ranks; compute_energies() against the fp64
    energies of the gathered state itself."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    steps = 3
    x, v, m = _ragged(n, 700 + n)
    bars = _step_bars(x, v, m, EPS * EPS, 0.01, (steps,))
    ctx = mp.spawn(_two_rank_worker, args=(2, port, n, steps, str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + 240.0
    try:
        while not ctx.join(timeout=5.0):                       # returns as soon as a worker ends; raises if one failed
            assert time.monotonic() < deadline, "the two ranks did not finish in time"
    finally:
        for proc in ctx.processes:
            if proc.is_alive():
                proc.kill()
    got = [np.load(tmp_path / f"sharded{r}.npz") for r in (0, 1)]
    for key in KEYS + ("crackles", "u", "k"):
        assert np.array_equal(got[0][key], got[1][key]), key              # every rank holds the same global arrays
    assert all(got[0][key].dtype == np.float64 and got[0][key].shape == (n, 3) for key in KEYS)
    _check_steps(f"two ranks n={n}", steps, bars, [got[0][key] for key in KEYS])
    u, k, ua, ka = fo.reference_energies(got[0]["positions"], got[0]["velocities"], m, G, EPS)
    ok_u, f_u = fo.within(got[0]["u"], u, n * (n - 1) // 2, ua)
    ok_k, f_k = fo.within(got[0]["k"], k, n, ka)
    print(f"n={n}: / bar: U {f_u:.4f}, K {f_k:.3f}")
    assert ok_u and ok_k, (f_u, f_k)


@pytest.fixture
def one_rank_group(tmp_path, monkeypatch):
    """A one-rank gloo group with NBD_FORCE_SHARDED=1: the sharded path end to end in this process (the collective with
    an async handle, no remote launch)."""
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    monkeypatch.setenv("NBD_FORCE_SHARDED", "1")
    try:
        yield dist.group.WORLD
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n", [130, 1000])
def test_forced_sharded_one_rank_group_has_the_unsharded_bits(n, gpu_device, one_rank_group):
    """x, v, a, j, s, c of the forced-sharded simulator are the un-sharded Hermite6Simulator's bits after 10 steps, and
    compute_energies() equals it; what HermiteSimulator refuses when sharded is refused here."""
    from galaxify import simulation
    x, v, m = _case(n)[:3]
    kw = dict(positions=x, velocities=v, masses=m, g_const=G, softening=EPS, dt=0.01, calc_energy=True, device="cuda")
    plain = simulation.Hermite6Simulator(**kw)
    forced = simulation.Hermite6Simulator(process_group=one_rank_group, **kw)
    assert forced._sharded and forced._hgather.collective and not plain._sharded
    assert not forced._graph_run_ok(64) and (forced.part.lo, forced.part.n_local) == (0, n)
    assert forced._rows_all.shape[1] == 12 and np.array_equal(_np(forced.positions), x)          # not through fp32
    forced._hws.view(F64).fill_(float("nan"))
    names = ("positions", "velocities", "accelerations", "jerks", "snaps", "crackles")
    for name in names:
        assert torch.equal(getattr(forced, name), getattr(plain, name)), ("start", name)
    a, j = forced.compute_accelerations_and_jerks()              # the inherited method on the sharded launches
    assert torch.equal(a, plain.accelerations) and torch.equal(j, plain.jerks)
    assert torch.equal(forced.compute_accelerations(), plain.accelerations)
    for _ in range(10):
        plain.step()
        forced.step()
    for name in names:
        assert torch.equal(getattr(forced, name), getattr(plain, name)), name
        assert torch.equal(forced.gather(name), getattr(plain, name)), name
    assert forced.compute_energies() == plain.compute_energies()
    states = forced.run(2)                                       # the eager engine
    plain.step(); plain.step()
    assert len(states) == 2 and torch.equal(states[-1].positions, plain.positions.cpu())
    assert (states[-1].u_energy, states[-1].k_energy) == plain.compute_energies()
    for call in (forced.compute_potentials, forced.compute_invariants):
        with pytest.raises(ValueError, match="range-sharded"):
            call()
    with pytest.raises(ValueError, match="range-sharded"):
        simulation.Hermite6Simulator(process_group=one_rank_group, calc_invariants=True, **kw).run(1)


def test_two_body_orbit_on_the_sharded_path(gpu_device, one_rank_group):
    """e = 0.5, eps = 0.1, one period in 256 steps as the n = 2 problem on the one-rank sharded path: the relative energy
    error (fp64, on the host, of the gathered state) within a factor 2 of the float64 oracle's own at that step count."""
    from galaxify import simulation
    steps, eps = 256, 0.1
    x, v, m, period = ho.two_body(0.5)
    x, v, m = fo.perturbed(x, v, m, 9)                   # (the orbit's zeros too: no input is fp32-representable)
    dt = period / steps
    ref = h6.hermite6_run(x, v, m, dt, 1.0, eps * eps, steps)
    e0 = fo.energy(x, v, m, 1.0, eps * eps)
    err_ref = abs(fo.energy(ref[0], ref[1], m, 1.0, eps * eps) - e0) / abs(e0)
    sim = simulation.Hermite6Simulator(positions=x, velocities=v, masses=m, g_const=1.0, softening=eps, dt=dt,
                                       calc_energy=False, device="cuda", process_group=one_rank_group)
    assert sim._sharded
    for _ in range(steps):
        sim.step()
    e1 = fo.energy(_np(sim.gather("positions")), _np(sim.gather("velocities")), m, 1.0, eps * eps)
    err_gpu = abs(e1 - e0) / abs(e0)
    print(f"S={steps}: energy error sharded {err_gpu:.6e}, oracle {err_ref:.6e}")
    assert err_ref > 0 and 0.5 * err_ref <= err_gpu <= 2.0 * err_ref, (err_gpu, err_ref)
