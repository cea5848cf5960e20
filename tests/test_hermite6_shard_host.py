"""Hermite6Simulator(process_group=...) without a GPU (the 6th-order entries and kernels of
csrc/direct_hermite_shard_f64.hip).

World_size-2, -3 and -8 gloo runs on CPU of the PRODUCT's distributed control flow: nbd/dist.py (partition, ONE all-gather
of 12-double rows per step, two at construction) and the sharded branches of galaxify.simulation.Hermite6Simulator. The
HIP entry points are replaced, in the spawned processes only, by float64 CPU stand-ins built on hermite6_oracle's
formulas, which also assert the protocol (predict -> local -> remote, zero padding rows, float64 rows of 12 columns).
Beside that: the new C-ABI entries are declared and bound and check their arguments before any launch, the remote plan
keeps every wave of a slab a chunk, the constructor's refusals come before any device work, and the new kernels have no
scratch, no spills, 48 KiB of LDS within the register budget of three workgroups per CU, and no fp32 intermediate."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import hermite6_oracle as h6
import hermite_f64_oracle as fo
from conftest import PKG, ROOT
from nbd import _lib
from test_dist_gloo import _free_port, _install_cpu_standins
from test_hermite_shard_f64_host import _kernel, _no_scratch_no_spills, asm  # noqa: F401  (asm: the unit's assembly)

STEPS = 5
DT, G, SOFT = 0.01, 1.0, 0.05
ENTRIES = ("nbd_hermite6_shard_f64_plan", "nbd_hermite6_shard_f64_workspace_bytes", "nbd_hermite6_shard_predict_f64",
           "nbd_hermite6_shard_force_local_f64", "nbd_hermite6_shard_force_remote_f64")
KEYS = ("positions", "velocities", "accelerations", "jerks", "snaps")


def _state(n):
    """Nothing fp32-representable, ragged masses as in the 4th-order shard tests."""
    x, v, m = fo.plummer_case(n, seed=77)
    return x, v, m * np.random.default_rng(1).uniform(0.5, 2.0, n)


def _partial(src, tgt, eps2, drop_diag):
    """Unscaled (a, j, s) sums of the 12-double target rows under the 12-double source rows (hermite6_oracle's terms)."""
    src, tgt = src.numpy(), tgt.numpy()
    d = src[None, :, 0:3] - tgt[:, None, 0:3]
    dv = src[None, :, 4:7] - tgt[:, None, 4:7]
    da = src[None, :, 8:11] - tgt[:, None, 8:11]
    r2 = (d * d).sum(-1) + eps2
    if drop_diag:
        np.fill_diagonal(r2, 1.0)
    s = 1.0 / np.sqrt(r2)
    if drop_diag:
        np.fill_diagonal(s, 0.0)
    w = src[None, :, 3] * s ** 3
    s2 = s * s
    rv = (d * dv).sum(-1)
    al = rv * s2
    alw = rv * s * s * w
    gm = ((dv * dv).sum(-1) + (d * da).sum(-1)) * s2
    return ((w[..., None] * d).sum(1), (w[..., None] * dv - 3.0 * alw[..., None] * d).sum(1),
            (w[..., None] * da - 6.0 * alw[..., None] * dv + ((15.0 * al * al - 3.0 * gm) * w)[..., None] * d).sum(1))


state = {"local": None, "gathers": 0, "predicts": 0, "order": []}


def _install_h6_standins():
    """nbd.direct's wrappers the sharded 6th-order simulator calls, on CPU tensors, with the order of a step and the
    format of every exchanged array asserted."""
    from nbd import direct

    def padded(n):
        return (n + 63) // 64 * 64

    def rows_ok(t, n):
        assert t.dtype == torch.float64 and t.dim() == 2 and t.shape[1] == 12 and t.shape[0] >= padded(n)

    def alloc_hermite6_rows_f64(n, device):
        return torch.zeros((padded(n), 12), dtype=torch.float64)

    def hermite6_shard_predict_f64(pos, vel, mass, send, acc=None, jerk=None, snap=None, crackle=None, dt=0.0):
        assert state["local"] is None, "predict issued between a local and a remote block"
        n = pos.shape[0]
        rows_ok(send, n)
        assert (jerk is None) == (snap is None) == (crackle is None) and (jerk is None or acc is not None)
        assert all(t.dtype == torch.float64 for t in (pos, vel, mass)) and isinstance(dt, float)
        x, v, a = pos, vel, (torch.zeros_like(pos) if acc is None else acc)
        if jerk is not None:
            assert acc.dtype == jerk.dtype == snap.dtype == crackle.dtype == torch.float64
            j, s, c = jerk, snap, crackle
            x = x + v * dt + a * (dt ** 2 / 2) + j * (dt ** 3 / 6) + s * (dt ** 4 / 24) + c * (dt ** 5 / 120)
            v = v + a * dt + j * (dt ** 2 / 2) + s * (dt ** 3 / 6) + c * (dt ** 4 / 24)
            a = a + j * dt + s * (dt ** 2 / 2) + c * (dt ** 3 / 6)
        send.zero_()
        send[:n, 0:3] = x; send[:n, 3] = mass; send[:n, 4:7] = v; send[:n, 8:11] = a
        state["predicts"] += 1
        state["order"].append("predict")

    def hermite6_shard_force_local_f64(send, n_local, n_total, lo, eps2, ws, slabs=0):
        assert state["local"] is None, "local block issued twice without a remote block"
        rows_ok(send, n_local)
        assert not send[n_local:].any(), "padding rows of the send buffer must be zero"
        assert isinstance(eps2, float) and eps2 == SOFT ** 2, "softening^2 as the Python double"
        state["local"] = _partial(send[:n_local], send[:n_local], eps2, True)
        state["order"].append("local")

    def hermite6_shard_force_remote_f64(rows_all, n_total, send, n_local, lo, eps2, g, acc_out, jerk_out, snap_out, ws,
                                        pos=None, vel=None, acc_in=None, jerk_in=None, snap_in=None, crackle_out=None,
                                        dt=0.0, slabs_local=0, slabs_remote=0):
        assert state["local"] is not None, "remote block issued before the local block"
        rows_ok(rows_all, n_total); rows_ok(send, n_local)
        assert torch.equal(rows_all[lo:lo + n_local], send[:n_local]), "gather must have completed"
        assert not rows_all[n_total:].any() and not send[n_local:].any(), "padding must stay zero"
        assert all(t.shape == (n_local, 3) and t.dtype == torch.float64 for t in (acc_out, jerk_out, snap_out))
        assert isinstance(eps2, float) and isinstance(g, float) and (eps2, g) == (SOFT ** 2, G)
        keep = torch.ones(n_total, dtype=torch.bool); keep[lo:lo + n_local] = False
        rem = _partial(rows_all[:n_total][keep], send[:n_local], eps2, False)
        a1, j1, s1 = (g * (l + r) for l, r in zip(state["local"], rem))
        state["local"] = None
        given = [t is not None for t in (pos, vel, acc_in, jerk_in, snap_in, crackle_out)]
        assert all(given) or not any(given)
        if pos is not None:
            x, v, a0, j0, s0 = (t.numpy().copy() for t in (pos, vel, acc_in, jerk_in, snap_in))
            v1 = v + (a0 + a1) * (dt / 2) - (j1 - j0) * (dt ** 2 / 10) + (s0 + s1) * (dt ** 3 / 120)
            x1 = x + (v + v1) * (dt / 2) - (a1 - a0) * (dt ** 2 / 10) + (j0 + j1) * (dt ** 3 / 120)
            pos.copy_(torch.from_numpy(x1)); vel.copy_(torch.from_numpy(v1))
            crackle_out.copy_(torch.from_numpy(h6.crackle(a0, j0, s0, a1, j1, s1, dt)))
        acc_out.copy_(torch.from_numpy(a1)); jerk_out.copy_(torch.from_numpy(j1)); snap_out.copy_(torch.from_numpy(s1))
        state["order"].append("remote")

    # the sharded energies: one pack of the gathered state, then the un-sharded entry
    def alloc_rows_f64(n, device):
        return torch.zeros((padded(n), 4), dtype=torch.float64)

    def hermite_f64_pack(pos, vel, mass, posd, veld, acc=None, jerk=None, dt=0.0):
        n = pos.shape[0]
        assert pos.dtype == vel.dtype == mass.dtype == torch.float64 and mass.shape == (n,) and acc is None
        posd.zero_(); veld.zero_()
        posd[:n, 0:3] = pos; posd[:n, 3] = mass; veld[:n, 0:3] = vel

    def energy_f64(posd, vel, n, softening, g_const, workspace, out_uk=None):
        assert posd.dtype == vel.dtype == torch.float64 and vel.shape == (n, 3)
        u, k, _, _ = fo.reference_energies(posd[:n, 0:3].numpy(), vel.numpy(), posd[:n, 3].numpy(), g_const, softening)
        out_uk = torch.empty(2, dtype=torch.float64) if out_uk is None else out_uk
        out_uk[0], out_uk[1] = u, k
        return out_uk

    dummy = lambda *a, **k: torch.zeros(16, dtype=torch.uint8)
    for name, fn in dict(alloc_hermite6_rows_f64=alloc_hermite6_rows_f64, hermite6_shard_f64_workspace=dummy,
                         hermite6_shard_predict_f64=hermite6_shard_predict_f64,
                         hermite6_shard_force_local_f64=hermite6_shard_force_local_f64,
                         hermite6_shard_force_remote_f64=hermite6_shard_force_remote_f64, alloc_rows_f64=alloc_rows_f64,
                         hermite_f64_pack=hermite_f64_pack, hermite_f64_workspace=dummy, energy_f64=energy_f64).items():
        setattr(direct, name, fn)

    # count the collectives: every all_gather_into_tensor of the process goes through here
    real = dist.all_gather_into_tensor

    def counted(out, inp, *a, **k):
        state["gathers"] += 1
        state["gathered"] = (inp.dtype, tuple(inp.shape[1:]))
        return real(out, inp, *a, **k)
    dist.all_gather_into_tensor = counted


def _setup(rank, world, port):
    for p in (PKG, ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    _install_cpu_standins()
    _install_h6_standins()


def _worker(rank, world, port, n, out_dir):
    _setup(rank, world, port)
    try:
        from galaxify import simulation
        p, v, m = _state(n)
        kw = dict(positions=p, velocities=v, masses=m, dt=DT, g_const=G, softening=SOFT, calc_energy=False,
                  process_group=dist.group.WORLD)
        sim = simulation.Hermite6Simulator(**kw)
        part = sim.part
        assert part.world_size == world and sim._sharded and sim._f64
        assert state["gathers"] == 2 and state["order"] == ["predict", "local", "remote"] * 2, "two exchanges at the start"
        assert state["gathered"] == (torch.float64, (12,))
        for key in KEYS + ("crackles",):
            assert getattr(sim, key).shape == (part.n_local, 3) and getattr(sim, key).dtype == torch.float64, key
        assert not sim.crackles.any(), "c = 0 at the start"
        assert torch.equal(sim.positions, torch.from_numpy(p[part.lo:part.hi])), "converted directly, not through fp32"
        assert sim._rows_local.dtype == sim._rows_all.dtype == torch.float64
        assert sim._rows_local.shape[1] == sim._rows_all.shape[1] == 12
        before = state["gathers"]
        a, j = sim.compute_accelerations_and_jerks()                # the inherited method: one exchange, the rank's rows
        assert state["gathers"] == before + 1
        assert a.shape == (part.n_local, 3) and j.shape == (part.n_local, 3) and a.dtype == j.dtype == torch.float64
        assert torch.equal(a, sim.accelerations) and torch.equal(j, sim.jerks)
        assert sim.compute_accelerations().dtype == torch.float64
        assert not sim._graph_run_ok(64), "a sharded simulator must not be picked up by the chunked engine"
        for _ in range(STEPS):
            before = dict(state, order=list(state["order"]))
            pos_id, vel_id = sim.positions, sim.velocities
            old = (sim.accelerations, sim.jerks, sim.snaps, sim.crackles)
            ajs0 = [t.numpy().copy() for t in old[:3]]
            sim.step()
            assert state["gathers"] == before["gathers"] + 1, "exactly one all_gather_into_tensor per step()"
            assert state["gathered"] == (torch.float64, (12,)), "the exchanged rows are 12 doubles"
            assert state["predicts"] == before["predicts"] + 1 and state["local"] is None
            done = state["order"][len(before["order"]):]
            assert done == ["predict", "local", "remote"], done
            assert sim.positions is pos_id and sim.velocities is vel_id, "positions and velocities update in place"
            new = (sim.accelerations, sim.jerks, sim.snaps, sim.crackles)
            assert all(t is not o for t, o in zip(new, old)), "a, j, s and c are rebound"
        # the crackle of the last step: the c1 formula on the simulator's own (a, j, s) before and after it
        ajs1 = [t.numpy() for t in new[:3]]
        c_err = np.abs(sim.crackles.numpy() - h6.crackle(*ajs0, *ajs1, DT))
        assert np.all(c_err <= 16 * fo.U53 * h6.crackle_abs(*ajs0, *ajs1, DT)), rank
        full = {k: sim.gather(k) for k in KEYS + ("crackles",)}
        assert all(t.dtype == torch.float64 and t.shape == (n, 3) for t in full.values())
        # the energies: blocking gathers of positions and velocities, the global sums on every rank
        before = state["gathers"]
        u, k = sim.compute_energies()
        assert state["gathers"] == before + 2 and state["gathered"] == (torch.float64, (3,))
        u_ref, k_ref, _, _ = fo.reference_energies(full["positions"].numpy(), full["velocities"].numpy(), m, G, SOFT)
        assert (u, k) == (u_ref, k_ref), rank
        # what stays refused
        for call in (sim.compute_potentials, sim.compute_invariants):
            with pytest.raises(ValueError, match="range-sharded"):
                call()
        with pytest.raises(ValueError, match="range-sharded"):
            simulation.Hermite6Simulator(calc_invariants=True, **kw).run(1)
        if rank == 0:
            np.savez(os.path.join(out_dir, "sharded.npz"), **{k: t.numpy() for k, t in full.items()})
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n", [(2, 130), (3, 130), (3, 1001), (8, 1001)])
def test_sharded_steps_match_the_oracle(world, n, tmp_path):
    """5 steps of Hermite6Simulator(process_group=WORLD) at dt = 0.01: 130 = 65 + 65 and 44 + 43 + 43, 1001 over 3 (ragged)
    and over 8 (one rank of 126, seven of 125). The gathered x, v, a, j, s against hermite6_run at the project's step bar,
    8 s_k + 8 * 2^-53 max|ref|, s_k = the largest difference between the oracle run and the oracle run on permuted
    bodies."""
    mp.spawn(_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
    got = np.load(tmp_path / "sharded.npz")
    p, v, m = _state(n)
    perm = np.random.default_rng(11).permutation(n)
    back = np.empty_like(perm)
    back[perm] = np.arange(n)
    ref = h6.hermite6_run(p, v, m, DT, G, SOFT ** 2, STEPS)
    prm = h6.hermite6_run(p[perm], v[perm], m[perm], DT, G, SOFT ** 2, STEPS)
    for key, r, q in zip(KEYS, ref, prm):
        assert got[key].dtype == np.float64 and got[key].shape == (n, 3), key
        s_k = np.abs(r - q[back]).max()
        dist_ = np.abs(got[key] - r).max()
        tol = 8 * s_k + 8 * fo.U53 * np.abs(r).max()
        print(f"P={world} n={n} {key}: s_k = {s_k:.3e}, |sharded - oracle| = {dist_:.3e}, tolerance {tol:.3e}")
        assert dist_ <= tol, (key, dist_, tol)


def test_refusals_and_a_real_group_before_any_device_work(tmp_path):
    """Anything that is no ProcessGroup raises ValueError naming process_group before a device is resolved; a real
    one-rank gloo group gets past that check and reaches the project's usual refusal of device='cpu'."""
    from galaxify import simulation
    z = np.zeros((4, 3))
    kw = dict(positions=z, velocities=z, masses=np.ones(4), device="cpu")
    for bad in (object(), "WORLD", 0):
        with pytest.raises(ValueError, match="process_group"):
            simulation.Hermite6Simulator(process_group=bad, **kw)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        with pytest.raises(RuntimeError, match="cpu"):
            simulation.Hermite6Simulator(process_group=dist.group.WORLD, **kw)
    finally:
        dist.destroy_process_group()


def test_new_symbols_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbd.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared in include/nbd.h"
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    from nbd import direct
    assert direct.HERMITE6_ROW == 12
    for name in ("alloc_hermite6_rows_f64", "hermite6_shard_f64_workspace", "hermite6_shard_predict_f64",
                 "hermite6_shard_force_local_f64", "hermite6_shard_force_remote_f64"):
        assert callable(getattr(direct, name)), name


def _plan(L, n, lo, n_local):
    a, b, c, d = (ctypes.c_int() for _ in range(4))
    assert L.nbd_hermite6_shard_f64_plan(n, lo, n_local, a, b, c, d) == 0
    return a.value, b.value, c.value, d.value


def test_plan_workspace_and_argument_checks_without_a_gpu():
    L = _lib.lib()
    ws = L.nbd_hermite6_shard_f64_workspace_bytes
    g, s, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for n, lo, n_local in ((64, 0, 32), (65, 33, 32), (130, 44, 43), (200, 0, 200), (1000, 334, 333), (5000, 1667, 1667),
                           (65536, 8192, 8192), (524288, 196608, 65536)):
        sl, cl, sr, cr = _plan(L, n, lo, n_local)
        # the local block follows the un-sharded plan at n_local
        assert L.nbd_hermite_f64_plan(n_local, g, s, c) == 0 and (sl, cl) == (s.value, c.value)
        # the remote block: the logical chunks of everything but [lo, lo + n_local), covered and balanced to within one:
        # no wave of a slab is left without a chunk while another has two or more
        phys = (n + 63) // 64
        inside = max(0, (phys if lo + n_local >= n else (lo + n_local) // 64) - (lo + 63) // 64)
        chunks = phys - inside if n_local < n else 0
        assert (sr >= 1) == (chunks > 0) and 0 <= sr <= 64
        if chunks:
            assert sr * 4 * cr >= chunks and (cr - 1) * sr * 4 < chunks
            assert chunks >= sr * 4 or cr == 1
            assert sr == 1 or sr * 4 <= chunks
            assert sr == max(1, min(64, chunks // 4, -(-1024 // g.value)))
        assert ws(n, lo, n_local, 0, 0) == (sl + sr) * 9 * n_local * 8
        assert ws(n, lo, n_local, 3, 0) == (3 + sr) * 9 * n_local * 8
        assert ws(n, lo, n_local, 1, 64) == (1 + (64 if chunks else 0)) * 9 * n_local * 8
    assert ws(100, 90, 20, 0, 0) == 0 and ws(100, 0, 0, 0, 0) == 0 and ws(100, 0, 50, 65, 0) == 0 and ws(100, 0, 50, 0, -1) == 0
    assert L.nbd_hermite6_shard_f64_plan(100, 90, 20, None, None, None, None) == -1
    assert L.nbd_hermite6_shard_f64_plan(100, 0, 0, None, None, None, None) == -1
    big = 1 << 30
    A, S = 0x10000, 0x20000                                     # 32-byte aligned stand-ins: nothing is launched
    pred = L.nbd_hermite6_shard_predict_f64
    assert pred(A, A, None, None, None, None, A, 10, 0.1, S, 63, None) == -1        # fewer rows than padded_len(n_local)
    assert pred(A, A, A, A, None, None, A, 10, 0.1, S, 64, None) == -1              # jerk without snap and crackle
    assert pred(A, A, A, A, A, None, A, 10, 0.1, S, 64, None) == -1
    assert pred(A, A, None, A, A, A, A, 10, 0.1, S, 64, None) == -1                 # the higher ones without acc
    assert pred(A, A, None, None, None, None, A, 10, 0.1, S + 16, 64, None) == -1   # 32-byte alignment
    assert pred(A, A, None, None, None, None, A, 10, 0.1, None, 64, None) == -1
    assert pred(None, A, None, None, None, None, A, 10, 0.1, S, 64, None) == -1
    assert pred(None, None, None, None, None, None, None, 0, 0.1, None, 0, None) == 0
    loc = L.nbd_hermite6_shard_force_local_f64
    assert loc(S, 50, 0.01, A, big, 100, 60, 0, None) == -1                         # [lo, lo + n_local) outside n_total
    assert loc(S, 50, 0.01, A, big, 100, 0, 65, None) == -1 and loc(S, 50, 0.01, A, big, 100, 0, -1, None) == -1
    assert loc(S + 16, 50, 0.01, A, big, 100, 0, 0, None) == -1 and loc(None, 50, 0.01, A, big, 100, 0, 0, None) == -1
    assert loc(S, 50, 0.01, None, big, 100, 0, 0, None) == -2 and loc(S, 50, 0.01, A + 4, big, 100, 0, 0, None) == -2
    assert loc(S, 50, 0.01, A, 9 * 50 * 8 - 1, 100, 0, 0, None) == -2
    assert loc(S, 50, 0.01, A, 9 * 50 * 8, 100, 0, 2, None) == -2
    assert loc(None, 0, 0.01, None, 0, 100, 0, 0, None) == 0                        # n_local == 0: a no-op
    rem = L.nbd_hermite6_shard_force_remote_f64
    ok = dict(all=S, n_total=100, send=S, n_local=50, lo=0, eps2=0.01, g=1.0, pos=None, vel=None, acc_in=None,
              jerk_in=None, snap_in=None, acc_out=A, jerk_out=A, snap_out=A, crackle_out=None, dt=0.0, ws=A,
              ws_bytes=big, sl=0, sr=0, stream=None)
    full = ws(100, 0, 50, 0, 0)
    for change, rc in ((dict(lo=60), -1), (dict(sl=65), -1), (dict(sr=-1), -1), (dict(all=None), -1),
                       (dict(all=S + 16), -1), (dict(send=S + 16), -1), (dict(send=None), -1), (dict(acc_out=None), -1),
                       (dict(jerk_out=None), -1), (dict(snap_out=None), -1), (dict(pos=A), -1),
                       (dict(pos=A, vel=A, acc_in=A, jerk_in=A, snap_in=A), -1),        # the corrector without crackle_out
                       (dict(ws=None), -2), (dict(ws=A + 4), -2), (dict(ws_bytes=full - 1), -2),
                       (dict(ws_bytes=full, sr=2), -2), (dict(n_local=0), 0)):
        assert rem(*{**ok, **change}.values()) == rc, change


@pytest.mark.parametrize("kernel", ["shard_pair_f64_kernelINS_6Order6ELb0E", "shard_pair_f64_kernelINS_6Order6ELb1E"])
def test_pair_kernels_resources_and_instructions(asm, kernel):
    """The local (RANGE = false) and remote (RANGE = true) pair kernels: no scratch, no spills, exactly 48 KiB of LDS --
    three workgroups per CU, 3 waves per SIMD -- and at most 168 VGPRs, the register budget at that occupancy (the
    un-sharded kernel's own condition); LDS-DMA loads, the fp64 reciprocal square root and the counted wait of three
    streamed arrays; no fp32 intermediate and no atomics."""
    meta, desc, body = _kernel(asm, kernel)
    _no_scratch_no_spills(meta)
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1)) == 48 * 1024
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
    print(kernel, "VGPRs", vgprs)
    assert vgprs <= 168
    for need in ("global_load_lds_dwordx4", "v_rsq_f64", "vmcnt(6)"):
        assert need in body, need
    for bad in ("v_cvt_f32_f64", "v_rsq_f32"):
        assert bad not in body, bad
    assert not re.search(r"\b(global|flat|ds|buffer)_atomic", body)


@pytest.mark.parametrize("kernel", ["hermite6_predict_kernelILi3E", "hermite6_finish_kernelILb0E"])
def test_row_kernels_have_no_lds_and_no_spills(asm, kernel):
    """hermite6_predict_kernel<3> (the send buffer's three-piece stride) and hermite6_finish_kernel<false> (no packed row)"""
    meta, desc, body = _kernel(asm, kernel)
    _no_scratch_no_spills(meta)
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1)) == 0
    assert "v_cvt_f32_f64" not in body and not re.search(r"\b(global|flat|ds|buffer)_atomic", body)
