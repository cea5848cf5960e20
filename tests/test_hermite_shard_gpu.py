"""Range-sharded 4th-order Hermite step (csrc/direct_hermite_shard.hip, HermiteSimulator(process_group=...)) on the GPU
against the fp64 restatement in hermite_oracle.py, at the bars of tests/test_hermite_gpu.py: emulated ranks through the
C-ABI in one process (force, masks, determinism, the full step), two real processes over gloo, and the one-rank group."""
import functools
import os

import numpy as np
import pytest
import torch

import hermite_oracle as ho
from conftest import load_golden, row_rel

pytestmark = pytest.mark.gpu

TOL = 1e-5          # per-particle relative, as tests/test_hermite_gpu.py


def _np(t):
    return t.detach().cpu().numpy()


def _f32(x):
    return float(np.float32(x))


def _as64(a):
    return np.asarray(a, np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _plummer(n):
    """Plummer state with ragged masses (the recipe of the existing sharded tests), softening 0.1, G = 1, and its fp64
    force: computed once per size and shared, never modified."""
    from nbd.plummer import generate_plummer
    p, v, m = generate_plummer(n, seed=77)
    m = m * np.random.default_rng(1).uniform(0.5, 2.0, n)
    case = dict(pos=p, vel=v, mass=m, g_const=1.0, softening=0.1, dt=0.01)
    return case, _reference(n)


def _reference_of(g):
    return ho.accel_jerk(_as64(g["pos"]), _as64(g["vel"]), _as64(g["mass"]), _f32(g["g_const"]),
                         _f32(float(g["softening"]) ** 2))


def _reference(n):
    from nbd.plummer import generate_plummer
    p, v, m = generate_plummer(n, seed=77)
    m = m * np.random.default_rng(1).uniform(0.5, 2.0, n)
    return ho.accel_jerk(_as64(p), _as64(v), _as64(m), 1.0, _f32(0.1 ** 2))


def _dev(g, dev):
    return tuple(torch.tensor(np.asarray(g[k]), dtype=torch.float32, device=dev) for k in ("pos", "vel", "mass"))


def _gathered_rows(pos, vel, mass):
    """The array every rank holds after the exchange, built with the existing pack and device copies."""
    from nbd import direct
    n = pos.shape[0]
    posm, velp = direct.alloc_posm(n, pos.device), direct.alloc_posm(n, pos.device)
    direct.hermite_pack(pos, vel, mass, posm, velp)
    rows = direct.alloc_hermite_rows(n, pos.device)
    rows[:, 0:4].copy_(posm)
    rows[:, 4:8].copy_(velp)
    return rows


def _send_of(rows_all, part, rows=None):
    from nbd import direct
    send = direct.alloc_hermite_rows(max(part.n_local, rows or 0), rows_all.device)
    send[:part.n_local].copy_(rows_all[part.lo:part.hi])
    return send


def _parts(n, world):
    from nbd.dist import RangePartition
    return [RangePartition(n, world, r) for r in range(world)]


def _nan_ws(nbytes, dev):
    return torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device=dev)        # every float a NaN


def _rank_force(rows_all, n, part, eps2, g, ws=None, send=None):
    """(a, j) of one emulated rank: local then remote, force only."""
    from nbd import direct
    dev = rows_all.device
    send = _send_of(rows_all, part) if send is None else send
    if ws is None:
        ws = direct.hermite_shard_workspace(n, part.lo, part.n_local, dev)
    acc = torch.full((part.n_local, 3), float("nan"), device=dev)
    jerk = torch.full((part.n_local, 3), float("nan"), device=dev)
    direct.hermite_shard_force_local(send, part.n_local, n, part.lo, eps2, ws)
    direct.hermite_shard_force_remote(rows_all, n, send, part.n_local, part.lo, eps2, g, acc, jerk, ws)
    return acc, jerk


def _check_ranks(g, ref, world, dev):
    from nbd import direct
    pos, vel, mass = _dev(g, dev)
    n = pos.shape[0]
    eps2, gc = _f32(float(g["softening"]) ** 2), _f32(g["g_const"])
    rows_all = _gathered_rows(pos, vel, mass)
    a_ref, j_ref = ref
    worst = 0.0
    for part in _parts(n, world):
        # the predict entry with no (acc, jerk) is the plain pack of the rank's rows, zero behind them
        send = direct.alloc_hermite_rows(part.n_local, dev)
        send.fill_(float("nan"))
        direct.hermite_shard_predict(pos[part.lo:part.hi].contiguous(), vel[part.lo:part.hi].contiguous(),
                                     mass[part.lo:part.hi].contiguous(), send)
        assert torch.equal(send[:part.n_local], rows_all[part.lo:part.hi]) and not send[part.n_local:].any()
        if part.n_local == 0:
            # a no-op returning success, workspace or not
            direct.hermite_shard_force_local(send, 0, n, part.lo, eps2, _nan_ws(16, dev))
            continue
        nbytes = direct._lib.lib().nbd_hermite_shard_workspace_bytes(n, part.lo, part.n_local)
        acc, jerk = _rank_force(rows_all, n, part, eps2, gc, ws=_nan_ws(nbytes, dev), send=send)
        acc, jerk = _np(acc), _np(jerk)
        assert np.isfinite(acc).all() and np.isfinite(jerk).all(), part.rank
        ea, ej = row_rel(acc, a_ref[part.lo:part.hi]), row_rel(jerk, j_ref[part.lo:part.hi])
        print(f"n={n} P={world} rank={part.rank} lo={part.lo} n_local={part.n_local} a {ea:.2e} j {ej:.2e}")
        worst = max(worst, ea, ej)
        assert ea < TOL and ej < TOL, (part.rank, ea, ej)
    return worst


# n, P: 64/2 own range inside one chunk, both straddles in the same chunk; 65/2 straddle + tail chunk of one body; 130/3
# lo unaligned on every rank; 200/1 remote walk with zero chunks; 3/8 ranks with n_local = 0; 1000/3 whole chunks skipped,
# both ends masked; 5000/3 waves that walk several chunks around a skipped run
@pytest.mark.parametrize("n,world", [(64, 2), (65, 2), (130, 3), (200, 1), (3, 8), (1000, 3), (5000, 3)])
def test_emulated_ranks_force_matches_f64(n, world, gpu_device):
    g, ref = _plummer(n)
    _check_ranks(g, ref, world, gpu_device)


@pytest.mark.parametrize("name,world", [("direct_plummer_n64_eps0", 2), ("direct_plummer_n64_eps0", 3),
                                        ("direct_plummer_n300_ragged_mass", 3)])
def test_emulated_ranks_force_golden(name, world, gpu_device):
    """Softening 0 (the index-masked i == j path in both blocks) and a massless body."""
    g = load_golden(name)
    _check_ranks(g, _reference_of(g), world, gpu_device)


def test_plan_and_workspace(gpu_device):
    from nbd import direct
    lib = direct._lib.lib()
    for n, lo, n_local in ((1000, 334, 333), (200, 0, 200), (524288, 196608, 65536), (65536, 8192, 8192)):
        p = direct.hermite_shard_plan(n, lo, n_local)
        assert p["slabs_local"] >= 1 and (p["slabs_remote"] >= 1) == (n_local < n)
        # a wave's sequential fp32 chain stays <= 64 chunks of 64 sources
        assert p["chunks_per_wave_local"] <= 64 and p["chunks_per_wave_remote"] <= 64, p
        assert lib.nbd_hermite_shard_workspace_bytes(n, lo, n_local) == \
            (p["slabs_local"] + p["slabs_remote"]) * 6 * n_local * 4
    assert lib.nbd_hermite_shard_workspace_bytes(100, 90, 20) == 0


@pytest.mark.parametrize("n", [130, 1000])
def test_own_rows_of_the_gathered_array_are_never_sources(n, gpu_device):
    """Mask by select, skip by chunk: the remote block gives the same bits whether rows [lo, hi) of the gathered array
    hold the real values, zeros or NaN; the padding behind n_total stays the zeros it was."""
    g, _ = _plummer(n)
    pos, vel, mass = _dev(g, gpu_device)
    eps2 = _f32(0.1 ** 2)
    rows_all = _gathered_rows(pos, vel, mass)
    for part in _parts(n, 3):
        send = _send_of(rows_all, part)
        base = _rank_force(rows_all, n, part, eps2, 1.0, send=send)
        for fill in (0.0, float("nan")):
            other = rows_all.clone()
            other[part.lo:part.hi] = fill
            got = _rank_force(other, n, part, eps2, 1.0, send=send)
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), (part.rank, fill)
            assert not other[n:].any()
        assert torch.isfinite(base[0]).all() and torch.isfinite(base[1]).all()


def test_deterministic_and_independent_of_rank_order(gpu_device):
    """The same call twice gives the same bits, and a rank's output does not depend on which ranks used the (shared,
    NaN-filled at first) workspace before it."""
    from nbd import direct
    n, world = 1000, 3
    g, _ = _plummer(n)
    pos, vel, mass = _dev(g, gpu_device)
    eps2 = _f32(0.1 ** 2)
    rows_all = _gathered_rows(pos, vel, mass)
    parts = _parts(n, world)
    lib = direct._lib.lib()
    ws = _nan_ws(max(lib.nbd_hermite_shard_workspace_bytes(n, p.lo, p.n_local) for p in parts), gpu_device)
    first = {p.rank: _rank_force(rows_all, n, p, eps2, 1.0, ws=ws) for p in parts}
    again = {p.rank: _rank_force(rows_all, n, p, eps2, 1.0, ws=ws) for p in reversed(parts)}
    alone = {p.rank: _rank_force(rows_all, n, p, eps2, 1.0) for p in parts}
    for r in first:
        for other in (again, alone):
            assert torch.equal(first[r][0], other[r][0]) and torch.equal(first[r][1], other[r][1]), r


def test_full_sharded_step_through_the_c_abi(gpu_device):
    """predict, local, remote + corrector for every emulated rank of n = 1000, P = 3, the exchange by device copies:
    10 steps against the fp64 Hermite step."""
    from nbd import direct
    n, world, dt = 1000, 3, 0.01
    g, (a, j) = _plummer(n)
    dev = gpu_device
    pos, vel, mass = _dev(g, dev)
    eps2 = _f32(0.1 ** 2)
    x, v, m = _as64(g["pos"]), _as64(g["vel"]), _as64(g["mass"])
    parts = _parts(n, world)
    rows_all = _gathered_rows(pos, vel, mass)
    ranks = []
    for p in parts:
        acc, jerk = _rank_force(rows_all, n, p, eps2, 1.0)
        ranks.append(dict(part=p, pos=pos[p.lo:p.hi].clone(), vel=vel[p.lo:p.hi].clone(),
                          mass=mass[p.lo:p.hi].contiguous(), acc=acc, jerk=jerk,
                          send=direct.alloc_hermite_rows(p.n_local, dev),
                          ws=direct.hermite_shard_workspace(n, p.lo, p.n_local, dev)))

    def cat(key):
        return _np(torch.cat([r[key] for r in ranks]))
    for k in range(10):
        for r in ranks:
            direct.hermite_shard_predict(r["pos"], r["vel"], r["mass"], r["send"], r["acc"], r["jerk"], dt)
        for r in ranks:                                        # the exchange
            p = r["part"]
            rows_all[p.lo:p.hi].copy_(r["send"][:p.n_local])
        for r in ranks:
            p = r["part"]
            direct.hermite_shard_force_local(r["send"], p.n_local, n, p.lo, eps2, r["ws"])
            direct.hermite_shard_force_remote(rows_all, n, r["send"], p.n_local, p.lo, eps2, 1.0, r["acc"], r["jerk"],
                                              r["ws"], pos=r["pos"], vel=r["vel"], acc_in=r["acc"], jerk_in=r["jerk"],
                                              dt=dt)
        x, v, a, j = ho.hermite_step(x, v, a, j, m, dt, 1.0, eps2)
        if k == 0:
            e1 = (row_rel(cat("pos"), x), row_rel(cat("vel"), v))
            print("1 step: pos %.2e vel %.2e" % e1)
            assert e1[0] < TOL and e1[1] < TOL, e1
    e10 = (row_rel(cat("pos"), x), row_rel(cat("vel"), v), row_rel(cat("acc"), a))
    print("10 steps: pos %.2e vel %.2e acc %.2e" % e10)
    assert max(e10) < 10 * TOL, e10


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
        from nbd.plummer import generate_plummer
        p, v, m = generate_plummer(n, seed=77)
        m = m * np.random.default_rng(1).uniform(0.5, 2.0, n)
        sim = simulation.HermiteSimulator(positions=p, velocities=v, masses=m, dt=0.01, calc_energy=True,
                                          device="cuda", process_group=dist.group.WORLD)
        assert sim.jerks.shape == (sim.part.n_local, 3)
        for _ in range(steps):
            sim.step()
        u, k = sim.compute_energies()
        full = {key: sim.gather(key).cpu().numpy() for key in ("positions", "velocities", "accelerations", "jerks")}
        if rank == 0:
            np.savez(os.path.join(out_dir, "sharded.npz"), u=u, k=k, **full)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n", [1024, 1001])
def test_two_rank_hermite_on_gpu_matches_f64(n, tmp_path, gpu_device):
    """The real sharded path (HIP kernels, RowGather of 8-float rows, one all-gather per step) with two processes
    sharing this GPU over gloo (RCCL needs distinct devices): 10 steps against the fp64 oracle, energies against the
    un-sharded simulator."""
    import socket
    import torch.multiprocessing as mp
    from galaxify import simulation
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    steps = 10
    mp.spawn(_two_rank_worker, args=(2, port, n, steps, str(tmp_path)), nprocs=2, join=True)
    got = np.load(tmp_path / "sharded.npz")
    g, _ = _plummer(n)
    x, v, a, j = ho.hermite_run(_as64(g["pos"]), _as64(g["vel"]), _as64(g["mass"]), 0.01, 1.0, _f32(0.1 ** 2), steps)
    err = {k: row_rel(got[k], ref) for k, ref in (("positions", x), ("velocities", v), ("accelerations", a))}
    print(n, err)
    assert max(err.values()) < 10 * TOL, err
    assert got["jerks"].shape == (n, 3) and np.isfinite(got["jerks"]).all()
    sim = simulation.HermiteSimulator(positions=g["pos"], velocities=g["vel"], masses=g["mass"], dt=0.01,
                                      calc_energy=True, device="cuda")
    for _ in range(steps):
        sim.step()
    u, k = sim.compute_energies()
    assert abs(got["u"] - u) < 1e-6 * abs(u) and abs(got["k"] - k) < 1e-6 * abs(k)


def test_forced_sharded_one_rank_group(gpu_device, tmp_path, monkeypatch):
    """A one-rank process group with NBD_FORCE_SHARDED=1: the sharded Hermite path end to end in this process (the
    collective with an async handle, a remote walk with zero chunks) on three golden cases: the step bars, run() against
    eager steps bit for bit, and the un-sharded simulator built beside it against nbd_hermite_step_f32 driven directly."""
    import torch.distributed as dist
    from galaxify import simulation
    from nbd import direct
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        for name in ("direct_plummer_n64_eps0", "direct_plummer_n300_ragged_mass", "direct_disk_n1024"):
            g = load_golden(name)
            dt = float(g["dt"])
            kw = dict(positions=g["pos"], velocities=g["vel"], masses=g["mass"], g_const=float(g["g_const"]),
                      softening=float(g["softening"]), dt=dt, calc_energy=True, device="cuda")
            monkeypatch.setenv("NBD_FORCE_SHARDED", "1")
            forced = simulation.HermiteSimulator(process_group=dist.group.WORLD, **kw)
            ran = simulation.HermiteSimulator(process_group=dist.group.WORLD, **kw)
            eager = simulation.HermiteSimulator(process_group=dist.group.WORLD, **kw)
            with pytest.raises(ValueError, match="BlockHermiteSimulator"):
                simulation.BlockHermiteSimulator(process_group=dist.group.WORLD, **kw)
            with pytest.raises(ValueError):              # a sharded run with calc_invariants stays refused
                simulation.HermiteSimulator(process_group=dist.group.WORLD, calc_invariants=True, **kw).run(1)
            monkeypatch.delenv("NBD_FORCE_SHARDED")
            plain = simulation.HermiteSimulator(**kw)
            assert forced._sharded and forced._hgather.collective and not plain._sharded
            assert not forced._graph_run_ok(64)

            # the step bars
            x, v, m = _as64(g["pos"]), _as64(g["vel"]), _as64(g["mass"])
            gc, eps2 = _f32(g["g_const"]), _f32(float(g["softening"]) ** 2)
            a, j = ho.accel_jerk(x, v, m, gc, eps2)
            assert row_rel(_np(forced.accelerations), a) < TOL and row_rel(_np(forced.jerks), j) < TOL, name
            # the un-sharded code path, driven directly
            n = x.shape[0]
            pos, vel, mass = _dev(g, gpu_device)
            posm, velp = direct.alloc_posm(n, gpu_device), direct.alloc_posm(n, gpu_device)
            hws = direct.hermite_workspace(n, gpu_device)
            direct.hermite_pack(pos, vel, mass, posm, velp)
            acc, jerk = direct.accel_jerk(posm, velp, n, eps2, gc, workspace=hws)
            for k in range(10):
                forced.step(); plain.step()
                direct.hermite_step(pos, vel, acc, jerk, acc, jerk, mass, dt, eps2, gc, posm, hws)
                x, v, a, j = ho.hermite_step(x, v, a, j, m, dt, gc, eps2)
                if k == 0:
                    assert row_rel(_np(forced.positions), x) < TOL and row_rel(_np(forced.velocities), v) < TOL, name
            e10 = (row_rel(_np(forced.positions), x), row_rel(_np(forced.velocities), v),
                   row_rel(_np(forced.accelerations), a))
            print(name, "10 steps: pos %.2e vel %.2e acc %.2e" % e10)
            assert max(e10) < 10 * TOL, (name, e10)
            for got, ref in ((plain.positions, pos), (plain.velocities, vel), (plain.accelerations, acc),
                             (plain.jerks, jerk)):
                assert torch.equal(got, ref), name
            uf, kf = forced.compute_energies(); up, kp = plain.compute_energies()
            assert abs(uf - up) < 1e-6 * abs(up) and abs(kf - kp) < 1e-6 * abs(kp)

            # run() is the eager engine here: five states = five step()s of a second forced-sharded simulator
            states = ran.run(5)
            assert len(states) == 5
            for st in states:
                eager.step()
                assert torch.equal(st.positions, eager.positions.cpu())
                assert torch.equal(st.velocities, eager.velocities.cpu())
                assert torch.equal(st.accelerations, eager.accelerations.cpu())
                assert (st.u_energy, st.k_energy) == eager.compute_energies()
            assert torch.equal(ran.jerks, eager.jerks)
    finally:
        dist.destroy_process_group()
