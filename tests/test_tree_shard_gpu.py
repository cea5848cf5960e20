"""The range-sharded tree force on the GPU (csrc/tree_force.hip: the ranged walks, the packed-row build, the scatter;
TreeLeapFrogSimulator(process_group=...)). Every comparison is exact: the reference is the full walk over the same
workspace, or the un-sharded simulator, in the same process -- which tests/test_tree_gpu.py and
tests/test_tree_potential_gpu.py hold to the fp64 oracles. A target group's walk reads nothing of another group's, so a
rank's rows are the one-GPU rows bit for bit, whatever the number of ranks."""
import functools
import os

import numpy as np
import pytest
import torch

import tree_oracle as to

pytestmark = pytest.mark.gpu

EPS2, G = float(np.float32(to.SOFTENING ** 2)), 1.0
WORLDS = (1, 2, 3, 8)


def _np(t):
    return t.detach().cpu().numpy()


def _plummer(n, seed=11):
    from nbd.plummer import generate_plummer
    p, v, m = generate_plummer(n, seed=seed)
    return p.astype(np.float32), v.astype(np.float32), m.astype(np.float32)


def _arrays(key):
    return to.case(key) if isinstance(key, str) else _plummer(key)


@functools.lru_cache(maxsize=None)
def _built(key):
    """(workspace, order, n) of one build through nbd.tree: made once per input and only read afterwards."""
    from nbd import tree
    p, _, m = _arrays(key)
    n = len(p)
    ws = tree.workspace(n, "cuda")
    order = tree.build(torch.tensor(p).cuda(), torch.tensor(m).cuda(), ws)
    return ws, order, n


def _counters():
    return torch.full((2,), -1, dtype=torch.int64, device="cuda")


def _ranges(total, world):
    from nbd.dist import RangePartition
    return [(p.lo, p.hi) for p in (RangePartition(total, world, r) for r in range(world))]


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _emulated(ws, n, world, theta, quad):
    """Every rank's ranged walks, one after another, into NaN-filled arrays of all groups in tree order: {"acc", "phi",
    "acc2", "phi2" (the fused walk's)} and the counters of the three walks summed over the ranks."""
    from nbd import tree
    rows = tree.groups(n) * tree.GROUP
    out = dict(acc=_nan((rows, 3), torch.float32), phi=_nan((rows,), torch.float64),
               acc2=_nan((rows, 3), torch.float32), phi2=_nan((rows,), torch.float64))
    sums = np.zeros((3, 2), np.int64)
    for lo, hi in _ranges(tree.groups(n), world):
        r = slice(lo * tree.GROUP, hi * tree.GROUP)
        c = [_counters() for _ in range(3)]
        walk = (ws, n, lo, hi, theta, EPS2, G, quad)
        tree.accel_groups(*walk, out=out["acc"][r], counters=c[0])
        tree.potential_groups(*walk, out=out["phi"][r], counters=c[1])
        tree.accel_potential_groups(*walk, out=(out["acc2"][r], out["phi2"][r]), counters=c[2])
        sums += np.stack([_np(x) for x in c])
    return out, sums


# ---------------------------------------------------------------- 1. emulated ranks through nbd.tree

# 300: split = 1, ragged last group; B (1000): split = 8 at level 0, 16 groups, the last one holding 40 bodies; 5000:
# 625 / 79 level-0 / level-1 nodes, the waves divide the tree at level 1; 65: the second group holds one body, and
# world = 3 leaves a rank with no groups
@pytest.mark.parametrize("quad", [True, False])
@pytest.mark.parametrize("theta", [0.0, 0.5])
@pytest.mark.parametrize("key", [300, "B", 5000, 65])
def test_emulated_ranks_give_the_full_walks_rows(key, theta, quad, gpu_device):
    from nbd import tree
    ws, order, n = _built(key)
    idx = order.long()
    cf = [_counters() for _ in range(3)]
    walk = (ws, n, theta, EPS2, G, quad)
    acc = tree.accel(*walk, counters=cf[0])
    phi = tree.potential(*walk, counters=cf[1])
    acc2, phi2 = tree.accel_potential(*walk, counters=cf[2])
    full = dict(acc=acc, phi=phi, acc2=acc2, phi2=phi2)
    want = np.stack([_np(x) for x in cf])
    assert (want[0] == want[1]).all() and (want[0] == want[2]).all() and want[0, 1] > 0
    if key == 65:
        assert _ranges(tree.groups(n), 3)[2] == (2, 2)
    for world in WORLDS:
        got, sums = _emulated(ws, n, world, theta, quad)
        for name, ref in full.items():
            rows = got[name]
            placed = torch.empty_like(ref)
            placed[idx] = rows[:n]                               # acc_full[order[k]] == acc_sorted[k]
            assert torch.equal(placed, ref), (key, world, name)
            assert rows.shape[0] == tree.groups(n) * 64 and (rows[n:] == 0).all(), (key, world, name)
        assert (sums == want).all(), (key, world, sums, want)


def test_a_group_range_in_the_middle(gpu_device):
    """n = 1000, the groups [5, 9) into a NaN-filled buffer with guard rows on both sides: only its 256 rows change,
    and they are the full walk's."""
    from nbd import tree
    ws, order, n = _built("B")
    idx = order.long()
    acc, phi = tree.accel_potential(ws, n, 0.5, EPS2, G, True)
    lo, hi, guard = 5, 9, 64
    rows = (hi - lo) * 64
    want_acc, want_phi = acc[idx[lo * 64:hi * 64]], phi[idx[lo * 64:hi * 64]]
    for fused in (False, True):
        buf_a, buf_p = _nan((rows + 2 * guard, 3), torch.float32), _nan((rows + 2 * guard,), torch.float64)
        mid = slice(guard, guard + rows)
        if fused:
            tree.accel_potential_groups(ws, n, lo, hi, 0.5, EPS2, G, True, out=(buf_a[mid], buf_p[mid]))
        else:
            tree.accel_groups(ws, n, lo, hi, 0.5, EPS2, G, True, out=buf_a[mid])
            tree.potential_groups(ws, n, lo, hi, 0.5, EPS2, G, True, out=buf_p[mid])
        assert torch.equal(buf_a[mid], want_acc) and torch.equal(buf_p[mid], want_phi)
        for buf in (buf_a, buf_p):
            assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + rows:]).all()
    # the full walk over the same workspace still gives its rows: the ranged walks left nothing behind
    again = tree.accel_potential(ws, n, 0.5, EPS2, G, True)
    assert torch.equal(again[0], acc) and torch.equal(again[1], phi)


# ---------------------------------------------------------------- 2. build_posm, scatter

@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_build_posm_is_build(name, gpu_device):
    """D: 16 coincident copies per body, tied keys -- the stable sort keeps them in index order under either layout."""
    from nbd import direct, tree
    ws, order, n = _built(name)
    p, _, m = to.case(name)
    posm = direct.pack_posm(torch.tensor(p).cuda(), torch.tensor(m).cuda())
    ws2 = tree.workspace(n, "cuda")
    order2 = tree.build_posm(posm, n, ws2)
    assert order2.dtype == torch.int32 and torch.equal(order2, order)
    for theta in (0.0, 0.5):
        c1, c2 = _counters(), _counters()
        a1, p1 = tree.accel_potential(ws, n, theta, EPS2, G, True, counters=c1)
        a2, p2 = tree.accel_potential(ws2, n, theta, EPS2, G, True, counters=c2)
        assert torch.equal(a1, a2) and torch.equal(p1, p2) and torch.equal(c1, c2)


def test_scatter_against_numpy(gpu_device):
    from nbd import tree
    ws, order, n = _built("B")
    o = _np(order).astype(np.int64)
    rng = np.random.default_rng(5)
    acc_s = rng.normal(size=(1024, 3)).astype(np.float32)
    phi_s = rng.normal(size=1024)
    acc_d, phi_d = torch.tensor(acc_s).cuda(), torch.tensor(phi_s).cuda()
    for lo, hi in ((0, n), (0, 0), (333, 667), (n - 1, n)):
        k = np.nonzero((o >= lo) & (o < hi))[0]
        want_a = np.full((hi - lo, 3), np.nan, np.float32); want_a[o[k] - lo] = acc_s[k]
        want_p = np.full((hi - lo,), np.nan); want_p[o[k] - lo] = phi_s[k]
        assert not np.isnan(want_a).any() and not np.isnan(want_p).any()        # order is a permutation
        for use_a, use_p in ((True, False), (False, True), (True, True)):
            out = (_nan((hi - lo, 3), torch.float32), _nan((hi - lo,), torch.float64))
            a, p = tree.scatter(ws, n, lo, hi, acc_d if use_a else None, phi_d if use_p else None, out=out)
            assert (a is out[0]) == use_a and (p is out[1]) == use_p
            if use_a:
                assert np.array_equal(_np(a), want_a), (lo, hi)
            else:
                assert torch.isnan(out[0]).all()
            if use_p:
                assert np.array_equal(_np(p), want_p), (lo, hi)
            else:
                assert torch.isnan(out[1]).all()


# ---------------------------------------------------------------- 3. the simulator: a forced one-rank group

def _kw(arrays, **kw):
    p, v, m = arrays
    kw.setdefault("calc_energy", False)
    return dict(positions=p, velocities=v, masses=m, g_const=1.0, softening=to.SOFTENING, dt=0.01, device="cuda", **kw)


def _same_state(a, b):
    for name in ("positions", "velocities", "accelerations"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.tree_order(), b.tree_order())
    assert a.tree_counters() == b.tree_counters()


def test_forced_sharded_one_rank_group(gpu_device, tmp_path, monkeypatch):
    """A one-rank gloo group with NBD_FORCE_SHARDED=1: the sharded step end to end in this process (both collectives,
    the packed-row build, the ranged walk of all groups, the scatter) equals the plain simulator bit for bit."""
    import torch.distributed as dist
    from galaxify.simulation import TreeLeapFrogSimulator as Sim
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        for arrays, potential in ((to.case("B"), "direct"), (_plummer(300), "tree")):
            kw = _kw(arrays, potential=potential)
            monkeypatch.setenv("NBD_FORCE_SHARDED", "1")
            forced = Sim(process_group=dist.group.WORLD, **kw)
            ran = Sim(process_group=dist.group.WORLD, **dict(kw, calc_energy=True))
            fused = Sim(process_group=dist.group.WORLD, **dict(kw, calc_invariants=True))
            monkeypatch.delenv("NBD_FORCE_SHARDED")
            plain, plain_ran, plain_fused = Sim(**kw), Sim(**dict(kw, calc_energy=True)), Sim(**dict(kw, calc_invariants=True))
            assert forced._sharded and forced._gather.collective and forced._acc_gather.collective
            assert not plain._sharded and Sim(process_group=dist.group.WORLD, **kw)._sharded is False
            assert forced.capture_step() is False and forced._step_graph is None
            _same_state(forced, plain)
            for _ in range(5):
                forced.step(); plain.step()
            _same_state(forced, plain)
            assert torch.equal(forced.compute_accelerations(), plain.compute_accelerations())
            assert forced.compute_energies() == plain.compute_energies()
            if potential == "tree":
                assert torch.equal(forced.compute_potentials(), plain.compute_potentials())
                assert forced.compute_invariants().row() == plain.compute_invariants().row()
                _same_state(forced, plain)               # the diagnostics leave the state and the force's counters alone
            else:
                with pytest.raises(ValueError, match="range-sharded diagnostics"):
                    forced.compute_potentials()
                with pytest.raises(ValueError, match="range-sharded diagnostics"):
                    forced.compute_invariants()
            # with calc_invariants the step's walk is the fused one (potential="tree"): the same a, and its phi
            for _ in range(2):
                fused.step(); plain_fused.step()
            _same_state(fused, plain_fused)
            assert fused._phi_of_step == plain_fused._phi_of_step == (potential == "tree")
            if potential == "tree":
                assert torch.equal(fused._phi, plain_fused._phi)
            with pytest.raises(ValueError, match="calc_invariants"):
                fused.run(1)
            # run() is the eager engine
            for got, ref in zip(ran.run(3), plain_ran.run(3)):
                assert torch.equal(got.positions, ref.positions) and torch.equal(got.velocities, ref.velocities)
                assert torch.equal(got.accelerations, ref.accelerations)
                assert (got.u_energy, got.k_energy) == (ref.u_energy, ref.k_energy)
            phases = forced.step_phases()
            plain.step()
            _same_state(forced, plain)
            assert sorted(phases) == ["build_ms", "exchange_ms", "gather_wait_ms", "host_enqueue_ms", "kick_drift_ms",
                                      "walk_ms"]
            assert all(v >= 0.0 for v in phases.values())
    finally:
        dist.destroy_process_group()


def test_forced_sharded_without_bodies(gpu_device, tmp_path, monkeypatch):
    import torch.distributed as dist
    from galaxify.simulation import TreeLeapFrogSimulator as Sim
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        monkeypatch.setenv("NBD_FORCE_SHARDED", "1")
        z = np.zeros((0, 3), np.float32)
        sim = Sim(process_group=dist.group.WORLD, potential="tree", **_kw((z, z, np.zeros(0, np.float32))))
        assert sim._sharded and sim.accelerations.shape == (0, 3)
        sim.step()
        assert sim.compute_accelerations().shape == (0, 3) and sim.compute_potentials().shape == (0,)
        assert sim.tree_counters() == (0, 0) and sim.tree_order().shape == (0,)
        assert sim.compute_energies() == (0.0, 0.0) and sim.compute_invariants().row() == [0.0] * 16
    finally:
        dist.destroy_process_group()


# ---------------------------------------------------------------- 4. two processes sharing the GPU over gloo

N_TWO, STEPS_TWO = 1001, 5       # 501 + 500 bodies, 16 groups of which the last holds 41: bodies and groups are ragged


def _two_rank_worker(rank, world, port, out_dir):
    import sys
    import torch.distributed as dist
    from conftest import PKG, ROOT
    for p in (PKG, ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        from galaxify.simulation import TreeLeapFrogSimulator as Sim
        sim = Sim(process_group=dist.group.WORLD, potential="tree", **_kw(_plummer(N_TWO), calc_energy=True))
        assert sim.accelerations.shape == (sim.part.n_local, 3)
        for _ in range(STEPS_TWO):
            sim.step()
        counters = sim.tree_counters()
        full = {key: sim.gather(key).cpu().numpy() for key in ("positions", "velocities", "accelerations")}
        phi = sim.compute_potentials()
        assert phi.shape == (sim.part.n_local,)
        inv = sim.compute_invariants().row()
        u, k = sim.compute_energies()
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), u=u, k=k, inv=np.array(inv), counters=np.array(counters),
                 order=sim.tree_order().cpu().numpy(), phi=phi.cpu().numpy(), lo=sim.part.lo, **full)
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_equal_one_rank(tmp_path, gpu_device):
    import socket
    import torch.multiprocessing as mp
    from galaxify.simulation import TreeLeapFrogSimulator as Sim
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_two_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    sim = Sim(potential="tree", **_kw(_plummer(N_TWO), calc_energy=True))
    for _ in range(STEPS_TWO):
        sim.step()
    counters = np.array(sim.tree_counters())
    ref = {key: _np(getattr(sim, key)) for key in ("positions", "velocities", "accelerations")}
    order = _np(sim.tree_order())
    phi = _np(sim.compute_potentials())
    inv = np.array(sim.compute_invariants().row())
    u, k = sim.compute_energies()
    got = [np.load(tmp_path / f"rank{r}.npz") for r in range(2)]
    for g in got:
        for key, want in ref.items():
            assert np.array_equal(g[key], want), key
        assert np.array_equal(g["order"], order)
        assert np.array_equal(g["inv"], inv) and (float(g["u"]), float(g["k"])) == (u, k)
        lo = int(g["lo"])
        assert np.array_equal(g["phi"], phi[lo:lo + len(g["phi"])])
    assert [int(g["lo"]) for g in got] == [0, 501] and len(got[1]["phi"]) == 500
    assert (got[0]["counters"] + got[1]["counters"] == counters).all() and (got[1]["counters"] > 0).all()


# ---------------------------------------------------------------- 5. empty and tiny systems through the C ABI

def test_no_bodies_and_one_body(gpu_device):
    from nbd import direct, tree
    # n = 0: every entry is a no-op
    ws0 = tree.workspace(0, "cuda")
    posm0 = direct.alloc_posm(0, "cuda")
    assert tree.build_posm(posm0, 0, ws0).shape == (0,)
    c = _counters()
    assert tree.accel_groups(ws0, 0, 0, 0, 0.5, EPS2, G, counters=c).shape == (0, 3) and c.tolist() == [0, 0]
    assert tree.potential_groups(ws0, 0, 0, 0, 0.5, EPS2, G).shape == (0,)
    a, p = tree.scatter(ws0, 0, 0, 0, torch.zeros((0, 3), device="cuda"), torch.zeros((0,), dtype=torch.float64,
                                                                                      device="cuda"))
    assert a.shape == (0, 3) and p.shape == (0,)
    # n = 1 on two ranks: rank 0 holds the body and the group, rank 1 neither
    pos, mass = torch.tensor([[0.5, -1.0, 2.0]]).cuda(), torch.tensor([3.0]).cuda()
    ws = tree.workspace(1, "cuda")
    order = tree.build_posm(direct.pack_posm(pos, mass), 1, ws)
    assert order.tolist() == [0]
    acc, phi = tree.accel_potential(ws, 1, 0.5, EPS2, G)
    assert acc.tolist() == [[0.0, 0.0, 0.0]] and phi.tolist() == [0.0]
    assert _ranges(1, 2) == [(0, 1), (1, 1)]
    sorted_acc, sorted_phi = _nan((64, 3), torch.float32), _nan((64,), torch.float64)
    for lo, hi in _ranges(tree.groups(1), 2):
        c = _counters()
        tree.accel_potential_groups(ws, 1, lo, hi, 0.5, EPS2, G, out=(sorted_acc[lo * 64:hi * 64], sorted_phi[lo * 64:hi * 64]),
                                    counters=c)
        assert c.tolist() == ([0, 1] if hi > lo else [0, 0])
    assert (sorted_acc == 0).all() and (sorted_phi == 0).all()
    for lo, hi in _ranges(1, 2):
        a, p = tree.scatter(ws, 1, lo, hi, sorted_acc, sorted_phi)
        assert a.shape == (hi - lo, 3) and p.shape == (hi - lo,)
        assert torch.equal(a, acc[lo:hi]) and torch.equal(p, phi[lo:hi])
