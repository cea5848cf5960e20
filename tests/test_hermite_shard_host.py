"""world_size-2, -3 and -8 gloo runs of the range-sharded HermiteSimulator on CPU.

What is exercised is the PRODUCT's distributed control flow: nbd/dist.py (partition, ONE all-gather of 8-float rows per
step) and the sharded branches of galaxify.simulation.HermiteSimulator (predict + pack of the own bodies -> asynchronous
exchange || own x own block -> own x others block + corrector). The HIP entry points are replaced, in this test only, by
CPU stand-ins: test_dist_gloo's for what the base constructor calls, and fp64 ones built on hermite_oracle's formulas for
nbd_hermite_shard_*, which also assert the protocol. The sharded result is compared with the un-sharded fp64 oracle."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import hermite_oracle as ho
from conftest import PKG, ROOT, row_rel
from test_dist_gloo import _free_port, _install_cpu_standins

TOL = 1e-5          # per-particle relative, as tests/test_hermite_gpu.py
STEPS = 5
DT, G, SOFT = 0.01, 1.0, 0.1


def _state(n):
    from nbd.plummer import generate_plummer
    p, v, m = generate_plummer(n, seed=77)
    return p, v, m * np.random.default_rng(1).uniform(0.5, 2.0, n)


def _partial(src, tgt, drop_diag):
    """Unscaled (a, j) sums of the 8-float target rows under the 8-float source rows, in fp64 (hermite_oracle's terms)."""
    src, tgt = src.double().numpy(), tgt.double().numpy()
    d = src[None, :, 0:3] - tgt[:, None, 0:3]
    dv = src[None, :, 4:7] - tgt[:, None, 4:7]
    r2 = (d * d).sum(-1) + state["eps2"]
    if drop_diag:
        np.fill_diagonal(r2, 1.0)
    s = 1.0 / np.sqrt(r2)
    if drop_diag:
        np.fill_diagonal(s, 0.0)
    w = src[None, :, 3] * s ** 3
    rv = (d * dv).sum(-1)
    return (w[..., None] * d).sum(1), (w[..., None] * dv - 3.0 * (rv * s * s * w)[..., None] * d).sum(1)


state = {"local": None, "eps2": None, "gathers": 0, "predicts": 0}


def _install_hermite_standins():
    """nbd.direct's nbd_hermite_shard_* wrappers on CPU tensors, with the order of a step asserted."""
    from nbd import direct

    def padded(n):
        return (n + 63) // 64 * 64

    def alloc_hermite_rows(n, device):
        return torch.zeros((padded(n), 8), dtype=torch.float32)

    def hermite_shard_predict(pos, vel, mass, send, acc=None, jerk=None, dt=0.0):
        assert state["local"] is None, "predict issued between a local and a remote block"
        n = pos.shape[0]
        assert send.shape[0] >= padded(n) and send.shape[1] == 8 and (acc is None) == (jerk is None)
        x, v = pos.double(), vel.double()
        if acc is not None:
            a, j = acc.double(), jerk.double()
            x, v = x + v * dt + a * (dt * dt / 2) + j * (dt ** 3 / 6), v + a * dt + j * (dt * dt / 2)
        send.zero_()
        send[:n, 0:3] = x.float(); send[:n, 3] = mass; send[:n, 4:7] = v.float()
        state["predicts"] += 1

    def hermite_shard_force_local(send, n_local, n_total, lo, eps2, ws):
        assert state["local"] is None, "local block issued twice without a remote block"
        assert not send[n_local:].any(), "padding rows of the send buffer must be zero"
        state["eps2"] = float(np.float32(eps2))
        state["local"] = _partial(send[:n_local], send[:n_local], True)

    def hermite_shard_force_remote(rows_all, n_total, send, n_local, lo, eps2, g, acc_out, jerk_out, ws, pos=None,
                                   vel=None, acc_in=None, jerk_in=None, dt=0.0):
        assert state["local"] is not None, "remote block issued before the local block"
        assert torch.equal(rows_all[lo:lo + n_local], send[:n_local]), "gather must have completed"
        assert not rows_all[n_total:].any() and not send[n_local:].any(), "padding must stay zero"
        assert acc_out.shape == (n_local, 3) and jerk_out.shape == (n_local, 3), "n_local rows come out"
        keep = torch.ones(n_total, dtype=torch.bool); keep[lo:lo + n_local] = False
        ar, jr = _partial(rows_all[:n_total][keep], send[:n_local], False)
        a1, j1 = g * (state["local"][0] + ar), g * (state["local"][1] + jr)
        state["local"] = None
        if pos is not None:
            x, v, a0, j0 = (t.double().numpy() for t in (pos, vel, acc_in, jerk_in))
            v1 = v + (a0 + a1) * (dt / 2) + (j0 - j1) * (dt * dt / 12)
            x1 = x + (v + v1) * (dt / 2) + (a0 - a1) * (dt * dt / 12)
            pos.copy_(torch.from_numpy(x1).float()); vel.copy_(torch.from_numpy(v1).float())
        acc_out.copy_(torch.from_numpy(a1).float()); jerk_out.copy_(torch.from_numpy(j1).float())

    dummy = lambda *a, **k: torch.zeros(16, dtype=torch.uint8)
    for name, fn in dict(alloc_hermite_rows=alloc_hermite_rows, hermite_shard_workspace=dummy,
                         hermite_shard_predict=hermite_shard_predict,
                         hermite_shard_force_local=hermite_shard_force_local,
                         hermite_shard_force_remote=hermite_shard_force_remote).items():
        setattr(direct, name, fn)

    # count the collectives: every all_gather_into_tensor of the process goes through here
    real = dist.all_gather_into_tensor

    def counted(*a, **k):
        state["gathers"] += 1
        return real(*a, **k)
    dist.all_gather_into_tensor = counted


def _worker(rank, world, port, n, out_dir):
    for p in (PKG, ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        _install_cpu_standins()
        _install_hermite_standins()
        from galaxify import simulation
        p, v, m = _state(n)
        sim = simulation.HermiteSimulator(positions=p, velocities=v, masses=m, dt=DT, g_const=G, softening=SOFT,
                                          calc_energy=False, process_group=dist.group.WORLD)
        part = sim.part
        assert part.world_size == world and sim._sharded
        for key in ("positions", "velocities", "accelerations", "jerks"):
            assert getattr(sim, key).shape == (part.n_local, 3), key
        a, j = sim.compute_accelerations_and_jerks()
        assert a.shape == (part.n_local, 3) and j.shape == (part.n_local, 3)
        assert not sim._graph_run_ok(64), "a sharded simulator must not be picked up by the chunked engine"
        for _ in range(STEPS):
            before = dict(state)
            pos_id, vel_id, acc_old, jerk_old = sim.positions, sim.velocities, sim.accelerations, sim.jerks
            sim.step()
            assert state["gathers"] == before["gathers"] + 1, "exactly one all_gather_into_tensor per step()"
            assert state["predicts"] == before["predicts"] + 1 and state["local"] is None
            assert sim.positions is pos_id and sim.velocities is vel_id, "positions and velocities update in place"
            assert sim.accelerations is not acc_old and sim.jerks is not jerk_old, "accelerations and jerks are rebound"
        full = {k: sim.gather(k).numpy() for k in ("positions", "velocities", "accelerations", "jerks")}
        with pytest.raises(ValueError, match="BlockHermiteSimulator"):
            simulation.BlockHermiteSimulator(positions=p, velocities=v, masses=m, process_group=dist.group.WORLD)
        if rank == 0:
            np.savez(os.path.join(out_dir, "sharded.npz"), **full)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n", [(2, 512), (2, 301), (3, 301), (8, 67)])
def test_sharded_hermite_steps_match_unsharded_f64_oracle(world, n, tmp_path):
    """5 steps of HermiteSimulator(process_group=WORLD): equal shards (world 2, n 512), ragged ones (301 over 2 and 3; 67
    over 8: ranks of 9 and of 8 bodies). Positions, velocities, accelerations and jerks against the un-sharded fp64 oracle
    at the 10-step bar of tests/test_hermite_gpu.py (10 TOL; positions and velocities at TOL: the stand-ins are fp64
    arithmetic on the fp32 state)."""
    mp.spawn(_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
    got = np.load(tmp_path / "sharded.npz")
    p, v, m = _state(n)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    x, v, a, j = ho.hermite_run(f32(p), f32(v), f32(m), DT, float(np.float32(G)), float(np.float32(SOFT ** 2)), STEPS)
    assert got["positions"].shape == (n, 3)
    err = {k: row_rel(got[k], ref) for k, ref in (("positions", x), ("velocities", v), ("accelerations", a),
                                                   ("jerks", j))}
    print(world, n, err)
    assert err["positions"] < TOL and err["velocities"] < TOL, err
    assert err["accelerations"] < 10 * TOL and err["jerks"] < 10 * TOL, err
