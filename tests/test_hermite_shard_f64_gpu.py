"""Range-sharded Hermite step in float64 (csrc/direct_hermite_shard_f64.hip, HermiteSimulator(dtype=torch.float64,
process_group=...)) on the GPU against the fp64 oracles, at the bar of tests/hermite_f64_oracle.py:
|got - ref| <= (T + 32) 2^-53 sum|terms|, T = n_total for the acceleration and 4 n_total for the jerk -- an any-order
bound, so it holds for the sharded order (own block, then the others) as it does for the un-sharded one. No input is
fp32-representable, masses are ragged, and every workspace is NaN-filled before a call. Emulated ranks through the C-ABI
in one process (force, explicit splits, masks, determinism, the un-sharded kernel's bits, the full step), two real
processes over gloo, and the one-rank group."""
import functools
import os

import numpy as np
import pytest
import torch

import hermite_f64_oracle as fo
import hermite_oracle as ho
from conftest import load_golden

pytestmark = pytest.mark.gpu

G, EPS = 1.0, 0.05
F64 = torch.float64


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, device):
    return torch.tensor(np.asarray(a, np.float64), dtype=F64, device=device)


def _ragged(n, seed):
    x, v, m = fo.plummer_case(n, seed=seed)
    return x, v, m * np.random.default_rng(1).uniform(0.5, 2.0, n)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, v, m, g, eps, a, j, sum|a terms|, sum|j terms|), computed once and never written to."""
    if isinstance(name, int):
        x, v, m = _ragged(name, 200 + name)
        g, eps = G, EPS
    else:
        gd = load_golden(name)
        x, v, m = fo.perturbed(gd["pos"], gd["vel"], gd["mass"], 5)
        g, eps = float(gd["g_const"]), float(gd["softening"])
    a, j = fo.accel_jerk(x, v, m, g, eps * eps)
    sa, sj = fo.accel_jerk_abs(x, v, m, g, eps * eps)
    for arr in (x, v, m, a, j, sa, sj):
        arr.setflags(write=False)
    return x, v, m, g, eps, a, j, sa, sj


def _packed(x, v, m, device):
    from nbd import direct
    n = x.shape[0]
    posd, veld = direct.alloc_rows_f64(n, device), direct.alloc_rows_f64(n, device)
    direct.hermite_f64_pack(_dev(x, device), _dev(v, device), _dev(m, device), posd, veld)
    return posd, veld


def _gathered_rows(x, v, m, device):
    """The array every rank holds after the exchange, built with the un-sharded pack and device copies."""
    from nbd import direct
    posd, veld = _packed(x, v, m, device)
    rows = direct.alloc_hermite_rows_f64(x.shape[0], device)
    rows[:, 0:4].copy_(posd)
    rows[:, 4:8].copy_(veld)
    return rows


def _send_of(rows_all, part):
    from nbd import direct
    send = direct.alloc_hermite_rows_f64(part.n_local, rows_all.device)
    send[:part.n_local].copy_(rows_all[part.lo:part.hi])
    return send


def _parts(n, world):
    from nbd.dist import RangePartition
    return [RangePartition(n, world, r) for r in range(world)]


def _ws_bytes(n, part, sl=0, sr=0):
    from nbd import direct
    return direct._lib.lib().nbd_hermite_shard_f64_workspace_bytes(n, part.lo, part.n_local, sl, sr)


def _nan_ws(nbytes, device):
    return torch.full((nbytes // 8 + 2,), float("nan"), dtype=F64, device=device).view(torch.uint8)


def _rank_force(rows_all, n, part, eps2, g, ws=None, send=None, sl=0, sr=0):
    """(a, j) of one emulated rank: local then remote, force only, the workspace NaN-filled unless one is given."""
    from nbd import direct
    dev = rows_all.device
    send = _send_of(rows_all, part) if send is None else send
    ws = _nan_ws(_ws_bytes(n, part, sl, sr), dev) if ws is None else ws
    acc = torch.full((part.n_local, 3), float("nan"), dtype=F64, device=dev)
    jerk = torch.full((part.n_local, 3), float("nan"), dtype=F64, device=dev)
    direct.hermite_shard_force_local_f64(send, part.n_local, n, part.lo, eps2, ws, slabs=sl)
    direct.hermite_shard_force_remote_f64(rows_all, n, send, part.n_local, part.lo, eps2, g, acc, jerk, ws,
                                          slabs_local=sl, slabs_remote=sr)
    return acc, jerk


def _check_rank(tag, part, acc, jerk, a, j, sa, sj):
    n = a.shape[0]
    own = slice(part.lo, part.hi)
    acc, jerk = _np(acc), _np(jerk)
    assert np.isfinite(acc).all() and np.isfinite(jerk).all(), tag
    ok_a, fa = fo.within(acc, a[own], n, sa[own])
    ok_j, fj = fo.within(jerk, j[own], 4 * n, sj[own])
    print(f"{tag} rank={part.rank} lo={part.lo} n_local={part.n_local}: |a - ref| / bar = {fa:.3f}, "
          f"|j - ref| / bar = {fj:.3f}")
    assert ok_a and ok_j, (tag, part.rank, fa, fj)


def _check_ranks(name, world, device, sl=0, sr=0, predict=True):
    from nbd import direct
    x, v, m, g, eps, a, j, sa, sj = _case(name)
    n = x.shape[0]
    rows_all = _gathered_rows(x, v, m, device)
    pos, vel, mass = _dev(x, device), _dev(v, device), _dev(m, device)
    for part in _parts(n, world):
        send = None
        if predict:
            # the predict entry with no (acc, jerk) is the plain pack of the rank's rows, zero behind them
            send = direct.alloc_hermite_rows_f64(part.n_local, device)
            send.fill_(float("nan"))
            direct.hermite_shard_predict_f64(pos[part.lo:part.hi].contiguous(), vel[part.lo:part.hi].contiguous(),
                                             mass[part.lo:part.hi].contiguous(), send)
            assert torch.equal(send[:part.n_local], rows_all[part.lo:part.hi]) and not send[part.n_local:].any()
        if part.n_local == 0:
            # a no-op returning success, workspace or not
            empty = direct.alloc_hermite_rows_f64(0, device)
            out = torch.empty((0, 3), dtype=F64, device=device)
            direct.hermite_shard_force_local_f64(empty, 0, n, part.lo, eps * eps, _nan_ws(16, device))
            direct.hermite_shard_force_remote_f64(rows_all, n, empty, 0, part.lo, eps * eps, g, out, out.clone(),
                                                  _nan_ws(16, device))
            continue
        acc, jerk = _rank_force(rows_all, n, part, eps * eps, g, send=send, sl=sl, sr=sr)
        _check_rank(f"n={name} P={world} slabs=({sl},{sr})", part, acc, jerk, a, j, sa, sj)


# n, P: 64/2 own range inside one chunk; 65/2 straddle + tail chunk of one body; 130/3 lo unaligned on every rank; 200/1
# no remote chunks; 3/8 ranks with n_local = 0; 1000/3 whole chunks skipped, both ends masked; 5000/3 several chunks around
# the skipped run
@pytest.mark.parametrize("n,world", [(64, 2), (65, 2), (130, 3), (200, 1), (3, 8), (1000, 3), (5000, 3)])
def test_emulated_ranks_force_at_the_bar(n, world, gpu_device):
    _check_ranks(n, world, gpu_device)


@pytest.mark.parametrize("name,world", [("direct_plummer_n64_eps0", 2), ("direct_plummer_n64_eps0", 3),
                                        ("direct_plummer_n300_ragged_mass", 3)])
def test_emulated_ranks_force_golden(name, world, gpu_device):
    """Softening 0 (index-masked everywhere, in both blocks) and a massless body."""
    x, v, m, g, eps, *_ = _case(name)
    assert (eps == 0.0) == name.endswith("eps0") and ((m == 0).any() == ("ragged_mass" in name))
    _check_ranks(name, world, gpu_device)


# remote slabs 1: 130/3 waves without a chunk; 1000/3 a wave walks across the skipped run, both LDS buffers reused; 5000/3
# about 13 chunks per wave around the gap. 64 slabs at 5000: more waves than chunks. Local slabs: 1, and 3 at n = 1000
@pytest.mark.parametrize("n,world,sl,sr", [(130, 3, 1, 1), (1000, 3, 1, 1), (1000, 3, 3, 1), (5000, 3, 1, 1),
                                           (5000, 3, 1, 64)])
def test_force_with_explicit_splits(n, world, sl, sr, gpu_device):
    _check_ranks(n, world, gpu_device, sl=sl, sr=sr, predict=False)


def test_plan_matches_the_workspace(gpu_device):
    from nbd import direct
    lib = direct._lib.lib()
    for n, lo, n_local in ((1000, 334, 333), (200, 0, 200), (524288, 196608, 65536), (65536, 8192, 8192)):
        p = direct.hermite_shard_f64_plan(n, lo, n_local)
        assert p["slabs_local"] >= 1 and (p["slabs_remote"] >= 1) == (n_local < n)
        assert lib.nbd_hermite_shard_f64_workspace_bytes(n, lo, n_local, 0, 0) == \
            (p["slabs_local"] + p["slabs_remote"]) * 6 * n_local * 8
        assert direct.hermite_shard_f64_workspace(n, lo, n_local, gpu_device).numel() >= \
            (p["slabs_local"] + p["slabs_remote"]) * 6 * n_local * 8


@pytest.mark.parametrize("n", [130, 1000])
def test_own_rows_of_the_gathered_array_are_never_sources(n, gpu_device):
    """Mask by select, skip by chunk: the remote block gives the same bits whether rows [lo, hi) of the gathered array
    hold the real values, zeros or NaN; the padding behind n_total stays the zeros it was."""
    x, v, m, g, eps, *_ = _case(n)
    rows_all = _gathered_rows(x, v, m, gpu_device)
    for part in _parts(n, 3):
        send = _send_of(rows_all, part)
        base = _rank_force(rows_all, n, part, eps * eps, g, send=send)
        for fill in (0.0, float("nan")):
            other = rows_all.clone()
            other[part.lo:part.hi] = fill
            got = _rank_force(other, n, part, eps * eps, g, send=send)
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), (part.rank, fill)
            assert not other[n:].any()
        assert torch.isfinite(base[0]).all() and torch.isfinite(base[1]).all()
        assert not rows_all[n:].any()


def test_deterministic_and_independent_of_rank_order(gpu_device):
    """The same call twice gives the same bits, and a rank's output does not depend on which ranks used the (shared,
    NaN-filled at first) workspace before it."""
    n, world = 1000, 3
    x, v, m, g, eps, *_ = _case(n)
    rows_all = _gathered_rows(x, v, m, gpu_device)
    parts = _parts(n, world)
    ws = _nan_ws(max(_ws_bytes(n, p) for p in parts), gpu_device)
    first = {p.rank: _rank_force(rows_all, n, p, eps * eps, g, ws=ws) for p in parts}
    again = {p.rank: _rank_force(rows_all, n, p, eps * eps, g, ws=ws) for p in reversed(parts)}
    alone = {p.rank: _rank_force(rows_all, n, p, eps * eps, g) for p in parts}
    for r in first:
        for other in (again, alone):
            assert torch.equal(first[r][0], other[r][0]) and torch.equal(first[r][1], other[r][1]), r


@pytest.mark.parametrize("n,slabs", [(130, 1), (1000, 3)])
def test_a_rank_that_owns_everything_has_the_unsharded_bits(n, slabs, gpu_device):
    """n_local = n_total, lo = 0: local + finish only, against nbd_accel_jerk_f64 at the same explicit slab count on rows
    packed from the same state -- one copy of every rounded operation, so the same bits."""
    from nbd import direct
    x, v, m, g, eps, *_ = _case(n)
    posd, veld = _packed(x, v, m, gpu_device)
    ref_a, ref_j = direct.accel_jerk_f64(posd, veld, n, eps * eps, g, slabs=slabs,
                                         workspace=_nan_ws(slabs * 6 * n * 8, gpu_device))
    rows_all = _gathered_rows(x, v, m, gpu_device)
    part = _parts(n, 1)[0]
    assert _ws_bytes(n, part, slabs, 0) == slabs * 6 * n * 8                    # no remote slabs
    acc, jerk = _rank_force(rows_all, n, part, eps * eps, g, sl=slabs)
    assert torch.equal(acc, ref_a) and torch.equal(jerk, ref_j)


def _step_bars(x, v, m, g, eps2, dt, counts, seed=11):
    """{k: [(name, reference, tolerance)]}: test_hermite_f64_gpu.py's step bar, 8 s_k + 8 * 2^-53 max|value|, s_k = the
    largest difference between hermite_run and the same run with the bodies permuted (measured here, on the CPU)."""
    n = x.shape[0]
    perm = np.random.default_rng(seed).permutation(n)
    back = np.empty_like(perm)
    back[perm] = np.arange(n)
    bars = {}
    for k in counts:
        ref = ho.hermite_run(x, v, m, dt, g, eps2, k)
        prm = [q[back] for q in ho.hermite_run(x[perm], v[perm], m[perm], dt, g, eps2, k)]
        bars[k] = [(name, r, 8 * np.abs(r - p).max() + 8 * fo.U53 * np.abs(r).max())
                   for name, r, p in zip(("pos", "vel", "acc", "jerk"), ref, prm)]
    return bars


def _check_steps(tag, k, bars, got):
    for (name, ref, tol), q in zip(bars[k], got):
        dist = np.abs(np.asarray(q) - ref).max()
        print(f"{tag} steps={k} {name}: |gpu - oracle| = {dist:.3e}, tolerance {tol:.3e}")
        assert dist <= tol, (tag, k, name, dist, tol)


def test_full_sharded_step_through_the_c_abi(gpu_device):
    """predict, local, remote + corrector for every emulated rank of n = 1000, P = 3, the exchange by device copies:
    after 1 and 10 steps at the un-sharded float64 step's bar."""
    from nbd import direct
    n, world, dt = 1000, 3, 0.01
    x, v, m, g, eps, *_ = _case(n)
    dev = gpu_device
    bars = _step_bars(x, v, m, g, eps * eps, dt, (1, 10))
    pos, vel, mass = _dev(x, dev), _dev(v, dev), _dev(m, dev)
    rows_all = _gathered_rows(x, v, m, dev)
    ranks = []
    for p in _parts(n, world):
        acc, jerk = _rank_force(rows_all, n, p, eps * eps, g)
        ranks.append(dict(part=p, pos=pos[p.lo:p.hi].clone(), vel=vel[p.lo:p.hi].clone(),
                          mass=mass[p.lo:p.hi].contiguous(), acc=acc, jerk=jerk,
                          send=direct.alloc_hermite_rows_f64(p.n_local, dev), ws=_nan_ws(_ws_bytes(n, p), dev)))

    def cat(key):
        return _np(torch.cat([r[key] for r in ranks]))
    for k in range(1, 11):
        for r in ranks:
            direct.hermite_shard_predict_f64(r["pos"], r["vel"], r["mass"], r["send"], r["acc"], r["jerk"], dt)
        for r in ranks:                                        # the exchange
            p = r["part"]
            rows_all[p.lo:p.hi].copy_(r["send"][:p.n_local])
        for r in ranks:
            p = r["part"]
            direct.hermite_shard_force_local_f64(r["send"], p.n_local, n, p.lo, eps * eps, r["ws"])
            direct.hermite_shard_force_remote_f64(rows_all, n, r["send"], p.n_local, p.lo, eps * eps, g, r["acc"],
                                                  r["jerk"], r["ws"], pos=r["pos"], vel=r["vel"], acc_in=r["acc"],
                                                  jerk_in=r["jerk"], dt=dt)
        if k in bars:
            _check_steps("emulated", k, bars, [cat(key) for key in ("pos", "vel", "acc", "jerk")])


def _two_rank_worker(rank, world, port, n, steps, out_dir):
    import sys
    import torch.distributed as dist
    from conftest import PKG, ROOT
    for p in (PKG, ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        from galaxify import simulation
        x, v, m = _ragged(n, 200 + n)
        sim = simulation.HermiteSimulator(positions=x, velocities=v, masses=m, dt=0.01, g_const=G, softening=EPS,
                                          calc_energy=True, device="cuda", process_group=dist.group.WORLD,
                                          dtype=torch.float64)
        assert sim._sharded and sim.jerks.shape == (sim.part.n_local, 3) and sim.jerks.dtype == torch.float64
        assert sim._rows_all.dtype == torch.float64 and sim._rows_all.shape[1] == 8
        for _ in range(steps):
            sim.step()
        u, k = sim.compute_energies()
        full = {key: sim.gather(key) for key in ("positions", "velocities", "accelerations", "jerks")}
        assert all(t.dtype == torch.float64 for t in full.values())
        np.savez(os.path.join(out_dir, f"sharded{rank}.npz"), u=u, k=k, **{key: _np(t) for key, t in full.items()})
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n", [1024, 1001])
def test_two_rank_f64_hermite_on_gpu(n, tmp_path, gpu_device):
    """The real sharded path (HIP kernels, RowGather of 8-double rows, one all-gather per step) with two processes sharing
    this GPU over gloo: 10 steps at the step bar; compute_energies() against the fp64 energies of the gathered state
    itself, the same on both ranks."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    steps = 10
    x, v, m = _ragged(n, 200 + n)
    bars = _step_bars(x, v, m, G, EPS * EPS, 0.01, (steps,))
    mp.spawn(_two_rank_worker, args=(2, port, n, steps, str(tmp_path)), nprocs=2, join=True)
    got = [np.load(tmp_path / f"sharded{r}.npz") for r in (0, 1)]
    keys = ("positions", "velocities", "accelerations", "jerks")
    for key in keys + ("u", "k"):
        assert np.array_equal(got[0][key], got[1][key]), key              # every rank holds the same global arrays
    assert all(got[0][key].dtype == np.float64 and got[0][key].shape == (n, 3) for key in keys)
    _check_steps(f"two ranks n={n}", steps, bars, [got[0][key] for key in keys])
    u, k, ua, ka = fo.reference_energies(got[0]["positions"], got[0]["velocities"], m, G, EPS)
    ok_u, f_u = fo.within(got[0]["u"], u, n * (n - 1) // 2, ua)
    ok_k, f_k = fo.within(got[0]["k"], k, n, ka)
    print(f"n={n}: / bar: U {f_u:.4f}, K {f_k:.3f}")
    assert ok_u and ok_k, (f_u, f_k)


def test_forced_sharded_one_rank_group(gpu_device, tmp_path, monkeypatch):
    """A one-rank process group with NBD_FORCE_SHARDED=1: the float64 sharded path end to end in this process (the
    collective with an async handle, no remote launch) on two golden cases: the force at the bar, run() against eager
    steps bit for bit, and what stays refused."""
    import torch.distributed as dist
    from galaxify import simulation
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        monkeypatch.setenv("NBD_FORCE_SHARDED", "1")
        for name in ("direct_plummer_n64_eps0", "direct_disk_n1024"):
            x, v, m, g, eps, a, j, sa, sj = _case(name)
            n = x.shape[0]
            kw = dict(positions=x, velocities=v, masses=m, g_const=g, softening=eps, dt=float(load_golden(name)["dt"]),
                      calc_energy=True, device="cuda", process_group=dist.group.WORLD)
            forced = simulation.HermiteSimulator(dtype=torch.float64, **kw)
            ran = simulation.HermiteSimulator(dtype=torch.float64, **kw)
            eager = simulation.HermiteSimulator(dtype=torch.float64, **kw)
            for dtype in (torch.float32, torch.float64):
                with pytest.raises(ValueError, match="BlockHermiteSimulator"):
                    simulation.BlockHermiteSimulator(dtype=dtype, **kw)
            with pytest.raises(ValueError):              # a sharded run with calc_invariants stays refused
                simulation.HermiteSimulator(dtype=torch.float64, calc_invariants=True, **kw).run(1)
            for call in (forced.compute_potentials, forced.compute_invariants):
                with pytest.raises(ValueError, match="range-sharded"):
                    call()
            assert forced._sharded and forced._hgather.collective and forced._f64
            assert not forced._graph_run_ok(64)
            assert forced.jerks.dtype == torch.float64 and forced.accelerations.dtype == torch.float64
            assert np.array_equal(_np(forced.positions), x)                      # not through fp32
            part = forced.part
            assert (part.lo, part.n_local) == (0, n)
            _check_rank(name, part, forced.accelerations, forced.jerks, a, j, sa, sj)

            # run() is the eager engine here: five states = five step()s of a second forced-sharded simulator
            states = ran.run(5)
            assert len(states) == 5
            for st in states:
                eager.step()
                assert st.positions.dtype == st.velocities.dtype == st.accelerations.dtype == torch.float64
                assert torch.equal(st.positions, eager.positions.cpu())
                assert torch.equal(st.velocities, eager.velocities.cpu())
                assert torch.equal(st.accelerations, eager.accelerations.cpu())
                assert (st.u_energy, st.k_energy) == eager.compute_energies()
            assert torch.equal(ran.jerks, eager.jerks) and ran.jerks.dtype == torch.float64
    finally:
        dist.destroy_process_group()
