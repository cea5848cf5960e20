"""BatchedSimulator(integrator="block_hermite" / "block_hermite6") on the MI355X (csrc/direct_batch_hermite_block_f64.hip):
every scene is bit-identical to the one-system block simulator of that scene alone -- state, levels, counters, run() --
whatever its companions and its place in the batch, while the ensemble takes one schedule, one host read and one launch
set per block step; max_level = 0 is the shared-timestep batch; the slab count of a scene follows its active count; the
ensemble's ticks are the union of the scenes' own; the e = 0.9 orbit at the one-system tests' bound.

The standard ensemble is batch_block_cases.ensemble(): 0, 1, 2, 3, 63, 64, 65, 130 and 520 bodies with dt, softening and
eta different per scene and one softening 0 (the index-masked walk beside the un-masked one in one launch). Every
workspace is NaN-filled before a call."""
import functools

import numpy as np
import pytest
import torch

import batch_block_cases as cases
import block_hermite6_cases as c6
import block_hermite_f64_cases as bc
import hermite_oracle as ho

pytestmark = pytest.mark.gpu

F64 = torch.float64
ORDERS = cases.ORDERS
COUNTERS = ("block_steps", "pair_interactions", "clamped")


def _np(t):
    return t.detach().cpu().numpy()


def _nan_fill(sim, byte=None):
    """NaN (or a byte pattern) into everything a call may only write before it reads: the partial sums, the active
    lists and the packed rows."""
    for name in ("_ws", "_hws", "_bws", "_posd", "_veld", "_accd"):
        t = getattr(sim, name, None)
        if t is None:
            continue
        if byte is None:
            flat = t.view(torch.uint8).view(-1)
            flat[: flat.numel() // 8 * 8].view(F64).fill_(float("nan"))
        else:
            t.view(torch.uint8).fill_(byte)


def _batch(scenes, order, max_level=cases.K, integrator=None, **kw):
    from galaxify import simulation
    kw.setdefault("calc_energy", False)
    integrator = integrator or cases.INTEGRATOR[order]
    if integrator in cases.INTEGRATOR.values():
        kw.update(eta=[s["eta"] for s in scenes], max_level=max_level)
    sim = simulation.BatchedSimulator(systems=[(s["pos"], s["vel"], s["mass"]) for s in scenes], integrator=integrator,
                                      g_const=[s["g"] for s in scenes], softening=[s["eps"] for s in scenes],
                                      dt=[s["dt"] for s in scenes], device="cuda", **kw)
    _nan_fill(sim)
    return sim


def _lone(s, order, max_level=cases.K, **kw):
    from galaxify import simulation
    kw.setdefault("calc_energy", False)
    if order == 4:
        kw["dtype"] = F64
    sim = getattr(simulation, cases.LONE[order])(positions=s["pos"], velocities=s["vel"], masses=s["mass"],
                                                 g_const=s["g"], softening=s["eps"], dt=s["dt"], eta=s["eta"],
                                                 max_level=max_level, device="cuda", **kw)
    _nan_fill(sim)
    return sim


def _lone_result(lone, order, initial_levels=None, history=None, K=cases.K):
    out = {nm: getattr(lone, nm).clone() for nm in cases.STATE[order]}
    out["levels"] = lone.levels.clone()
    out["counters"] = {c: getattr(lone, c) for c in COUNTERS}
    if history is not None:
        out["ticks"] = cases.ticks_of(initial_levels, [h.numpy() for h in history], K)
    return out


@functools.lru_cache(maxsize=None)
def _lone_after(order, k, steps=3):
    """Scene k of the standard ensemble alone after `steps` output steps at max_level = K: clones of its state, its levels
    and counters, and the ticks of its block steps; computed once."""
    s = cases.ensemble()[k]
    if s["pos"].shape[0] == 0:
        return None
    lone = _lone(s, order)
    initial = _np(lone.levels).copy()
    lone.level_history = []
    for _ in range(steps):
        _nan_fill(lone)
        lone.step()
    return _lone_result(lone, order, initial, lone.level_history)


def _assert_scene(sim, i, want, order, what):
    lo, hi = int(sim.offsets[i]), int(sim.offsets[i + 1])
    if want is None:
        assert lo == hi
        return
    for nm in cases.STATE[order] + ("levels",):
        x, y = getattr(sim, nm)[lo:hi], want[nm]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, i, nm)
        assert torch.equal(x, y), (what, i, nm, float((x.double() - y.double()).abs().max()))
    assert sim.scene_counters()[i] == want["counters"], (what, i)


def _three_steps(scenes, order, fill=_nan_fill):
    sim = _batch(scenes, order)
    sim.tick_history = []
    for _ in range(3):
        fill(sim)
        sim.step()
    return sim


# ------------------------------------------------------------------ 1. bit-identity per scene
@pytest.mark.parametrize("order", ORDERS)
def test_every_scene_is_the_lone_simulator_bit_for_bit(gpu_device, order):
    sc = cases.ensemble()
    assert len({(s["eps"], s["dt"], s["eta"]) for s in sc}) == len(sc)
    sim = _batch(sc, order)
    assert sim.levels.dtype == torch.int32 and sim.levels.shape == (sim.n,) and sim.levels.is_cuda
    assert sim._bparams.shape == (5, len(sc)) and sim.block_steps == 0
    for i, s in enumerate(sc):                                           # construction: the initial levels and clamps
        if s["pos"].shape[0]:
            lone = _lone(s, order)
            lo, hi = int(sim.offsets[i]), int(sim.offsets[i + 1])
            assert torch.equal(sim.levels[lo:hi], lone.levels), i
            assert sim.scene_counters()[i] == dict(block_steps=0, pair_interactions=0, clamped=lone.clamped)
    sim = _three_steps(sc, order)
    for i in range(len(sc)):
        _assert_scene(sim, i, _lone_after(order, i), order, "three steps")
    levels = _np(sim.levels)
    assert levels.min() >= 0 and levels.max() <= cases.K and len(set(levels.tolist())) > 1


# ------------------------------------------------------------------ 2. the slab count follows the active count
@pytest.mark.parametrize("order", ORDERS)
def test_the_slab_count_follows_the_active_count(gpu_device, order):
    """4608 bodies are 72 chunks: 18 slabs for an active set of at most 56 groups (3584 bodies), 15 with every body
    listed. Both occur in the run, and the scene is the lone simulator's bit for bit through both."""
    assert cases.slabs_f64(56, 72) == 18 and cases.slabs_f64(72, 72) == 15
    sc = [cases.big_scene(), cases.ensemble()[cases.SIZES.index(65)]]
    sim = _batch(sc, order)
    sim.tick_history = []
    lones = [_lone(s, order) for s in sc]
    for _ in range(2):
        sim.step()
        for lone in lones:
            lone.step()
    for i, lone in enumerate(lones):
        _assert_scene(sim, i, _lone_result(lone, order), order, "big scene")
    n_big, n_all = 4608, 4608 + 65
    counts = [n for _, n in sim.tick_history]
    print(f"order {order}: {len(counts)} ensemble block steps, n_act from {min(counts)} to {max(counts)}")
    assert min(counts) < 3584 and max(counts) == n_all
    assert lones[0].pair_interactions < lones[0].block_steps * n_big * n_big          # ... and the big scene had small sets


# ------------------------------------------------------------------ 3. companions do not matter
@pytest.mark.parametrize("order", ORDERS)
def test_companions_and_position_do_not_matter(gpu_device, order):
    sc = cases.ensemble()
    order_of = [7, 2, 8, 0, 5, 3, 1, 6]                                  # a permutation of the scenes without scene 4 (63)
    sim = _three_steps([sc[k] for k in order_of], order)
    for i, k in enumerate(order_of):
        _assert_scene(sim, i, _lone_after(order, k), order, f"scene {k} at {i}")


# ------------------------------------------------------------------ 4. max_level = 0 is the shared-timestep batch
@pytest.mark.parametrize("order", ORDERS)
def test_max_level_zero_is_the_shared_timestep_batch(gpu_device, order):
    sc = [cases.scene(n, eps=0.0 if n == 65 else 0.03, dt=0.004 + 0.001 * k, eta=0.02) for k, n in
          enumerate([1, 2, 65, 449])]
    blk = _batch(sc, order, max_level=0)
    shared = _batch(sc, order, integrator=cases.SHARED[order], dtype=F64)
    for nm in cases.STATE[order]:
        assert torch.equal(getattr(blk, nm), getattr(shared, nm)), ("construction", nm)
    for step in range(3):
        _nan_fill(blk)
        _nan_fill(shared)
        blk.step()
        shared.step()
        for nm in cases.STATE[order]:
            assert torch.equal(getattr(blk, nm), getattr(shared, nm)), (step, nm)
    assert blk.block_steps == 3 and not blk.levels.any()
    assert [c["block_steps"] for c in blk.scene_counters()] == [3] * 4


# ------------------------------------------------------------------ 5. the ensemble's schedule
@pytest.mark.parametrize("order", ORDERS)
def test_the_ensemble_schedule_is_the_union_of_the_scenes(gpu_device, order):
    sc = cases.ensemble()
    sim = _three_steps(sc, order)
    end = 1 << cases.K
    ticks = [t for t, _ in sim.tick_history]
    intervals, cur = [], []
    for t in ticks:
        cur.append(t)
        if t == end:
            intervals.append(cur)
            cur = []
    assert not cur and len(intervals) == 3
    for iv in intervals:
        assert all(a < b for a, b in zip(iv, iv[1:])) and iv[0] > 0 and iv[-1] == end
    lone_ticks = [_lone_after(order, k)["ticks"] for k in range(len(sc)) if _lone_after(order, k) is not None]
    per_scene = [c["block_steps"] for c in sim.scene_counters()]
    assert per_scene == [0] + [len(t) for t in lone_ticks]
    assert max(per_scene) <= sim.block_steps <= sum(per_scene)
    # the union of the lone runs' tick sets, interval by interval
    want = []
    for k in range(3):
        own = []
        for t in lone_ticks:
            ends = [i for i, x in enumerate(t) if x == end]
            own.append(t[(ends[k - 1] + 1) if k else 0: ends[k] + 1])
        want.append(sorted(set().union(*own)))
    assert intervals == want and sim.block_steps == sum(map(len, want)) == len(sim.tick_history)
    for (t, n_act) in sim.tick_history:
        assert 1 <= n_act <= sim.n
    assert sim.tick_history[-1][1] == sim.n


# ------------------------------------------------------------------ 6. accuracy
@pytest.mark.parametrize("order", ORDERS)
def test_the_eccentric_orbit_as_one_scene_of_three(gpu_device, order):
    """e = 0.9, eps = 0, one period as 4 output steps at max_level 16, with the eta of the one-system tests (4th order:
    bc.ORBIT_ETA; 6th: 0.01): the scene has the lone simulator's bits, so its energy error; and it holds those tests' bound
    against the fp64 host oracle: the oracle's pair interactions, no clamp, an orbit error within 2x the oracle's own."""
    x0, v0, m, dt = bc.orbit()
    eta = bc.ORBIT_ETA if order == 4 else 0.01
    want = bc.orbit_run() if order == 4 else c6.orbit_run(0.01)
    orbit = cases.frozen(x0.copy(), v0.copy(), m.copy(), 1.0, 0.0, dt, eta)
    sc = [cases.scene(3, eps=0.05, dt=0.01), orbit, cases.scene(65, eps=0.03, dt=0.02)]
    sim = _batch(sc, order, max_level=bc.ORBIT_K)
    lone = _lone(orbit, order, max_level=bc.ORBIT_K)
    e0 = sum(lone.compute_energies())
    u0, k0 = sim.compute_energies()
    assert u0[1] + k0[1] == e0
    for _ in range(4):
        sim.step()
        lone.step()
    _assert_scene(sim, 1, _lone_result(lone, order), order, "orbit")
    u1, k1 = sim.compute_energies()
    de_batch, de_lone = (u1[1] + k1[1]) - e0, sum(lone.compute_energies()) - e0
    assert de_batch == de_lone
    lo, hi = int(sim.offsets[1]), int(sim.offsets[2])
    err = ho.orbit_error(_np(sim.positions[lo:hi]), x0)
    got = sim.scene_counters()[1]
    print(f"order {order}: e=0.9 orbit eta={eta}: orbit error {err:.3e} (oracle {want['err']:.3e}), energy error "
          f"{de_batch:.3e}, {got['pair_interactions']} pairs, {sim.block_steps} ensemble block steps")
    assert got["pair_interactions"] == want["pair_interactions"] and got["clamped"] == 0
    assert err <= 2 * want["err"], (err, want["err"])


# ------------------------------------------------------------------ 7. run()
@pytest.mark.parametrize("order", ORDERS)
def test_run_is_the_lone_run_per_scene_and_three_steps(gpu_device, order):
    sc = [s for s in cases.ensemble() if s["pos"].shape[0] in (0, 2, 65, 130)]
    kw = dict(calc_energy=True, calc_invariants=True)
    ran, twin = _batch(sc, order, **kw), _batch(sc, order, **kw)
    states = ran.run(3)
    for _ in range(3):
        twin.step()
    for nm in cases.STATE[order] + ("levels",):
        assert torch.equal(getattr(ran, nm), getattr(twin, nm)), nm
    assert ran.scene_counters() == twin.scene_counters() and ran.block_steps == twin.block_steps > 3
    assert len(states) == len(sc) and all(len(s) == 3 for s in states)
    for i, s in enumerate(sc):
        if not s["pos"].shape[0]:
            continue
        lone_states = _lone(s, order, **kw).run(3)
        for got, want in zip(states[i], lone_states):
            assert got.step == want.step
            for nm in ("positions", "velocities", "accelerations"):
                a, b = getattr(got, nm), getattr(want, nm)
                assert a.dtype == F64 and torch.equal(a, b), (i, got.step, nm)
            assert (got.u_energy, got.k_energy) == (want.u_energy, want.k_energy), (i, got.step)
            assert got.invariants == want.invariants, (i, got.step)


# ------------------------------------------------------------------ 8. the workspace may hold anything
@pytest.mark.parametrize("order", ORDERS)
def test_results_do_not_depend_on_what_the_workspace_held(gpu_device, order):
    sc = cases.ensemble()
    runs = [_three_steps(sc, order, fill=functools.partial(_nan_fill, byte=0x7f)), _three_steps(sc, order)]
    for sim in runs:
        for i in range(len(sc)):
            _assert_scene(sim, i, _lone_after(order, i), order, "garbage workspace")
    for nm in cases.STATE[order] + ("levels",):
        assert torch.equal(getattr(runs[0], nm), getattr(runs[1], nm)), nm
    assert runs[0].tick_history == runs[1].tick_history and runs[0].scene_counters() == runs[1].scene_counters()


# ------------------------------------------------------------------ 9. degenerate scenes
@pytest.mark.parametrize("order", ORDERS)
def test_a_lone_body_and_coincident_bodies_beside_others(gpu_device, order):
    one = cases.frozen(np.array([[0.3 + 1e-10, 0.1, 1e-11]]), np.array([[1e-11, 0.25 + 1e-10, 1e-12]]),
                       np.array([1.0 + 1e-10]), 1.0, 0.0, 0.125, 0.02)
    rng = np.random.default_rng(2)
    x = rng.normal(size=(20, 3))
    x[5] = x[4]
    twins = cases.frozen(x, 0.1 * rng.normal(size=(20, 3)), np.full(20, 1.0 / 20) + rng.uniform(-1, 1, 20) * 1e-9, 1.0,
                         0.0, 0.01, 0.02)
    sc = [one, twins, cases.scene(65, eps=0.03, dt=0.02), cases.scene(3, eps=0.05, dt=0.01)]
    sim = _batch(sc, order, max_level=3)
    lones = [_lone(s, order, max_level=3) for s in sc]
    for _ in range(3):
        sim.step()
        for lone in lones:
            lone.step()
    got = sim.scene_counters()
    assert got[0] == dict(block_steps=3, pair_interactions=3, clamped=0)          # one block step per interval
    assert _np(sim.levels[:1]).tolist() == [0]
    assert np.allclose(_np(sim.positions[:1]), one["pos"] + 3 * 0.125 * one["vel"], rtol=0, atol=1e-15)
    assert got[1]["clamped"] == lones[1].clamped > 0 and got[1]["block_steps"] <= 3 * 8
    for i in (2, 3):                                                              # the clamps stay with their scene
        assert got[i]["clamped"] == lones[i].clamped != got[1]["clamped"]
    for i, lone in enumerate(lones):
        assert got[i] == {c: getattr(lone, c) for c in COUNTERS}, i
        lo, hi = int(sim.offsets[i]), int(sim.offsets[i + 1])
        assert torch.equal(sim.levels[lo:hi], lone.levels), i
        if i != 1:                                                                # (NaN state where the bodies coincide)
            _assert_scene(sim, i, _lone_result(lone, order), order, "degenerate companions")
    assert sim.block_steps <= 3 * 8


# ------------------------------------------------------------------ 10. re-levelling
@pytest.mark.parametrize("order", ORDERS)
def test_changing_one_scenes_dt_re_derives_its_levels(gpu_device, order):
    sc = [cases.ensemble()[k] for k in (3, 6, 7)]
    dt_new = 8 * sc[1]["dt"]
    # before the first step: every scene equals a lone simulator built with the new values
    sim = _batch(sc, order)
    sim.dt = [sc[0]["dt"], dt_new, sc[2]["dt"]]
    built = [_lone(dict(s, dt=d), order) for s, d in zip(sc, sim.dt)]
    sim.step()
    assert sim._leveled_for[0] == tuple(sim.dt)
    for i, lone in enumerate(built):
        lone.step()
        want = _lone_result(lone, order)
        if i == 1:                                                              # (levelled twice here: its clamps count twice)
            assert sim.scene_counters()[1]["clamped"] >= want["counters"]["clamped"]
            want["counters"]["clamped"] = sim.scene_counters()[1]["clamped"]
        _assert_scene(sim, i, want, order, "new dt at the start")
    # between steps: the scene concerned is re-levelled as the lone simulator re-levels itself, the others are left alone
    sim, lones = _batch(sc, order), [_lone(s, order) for s in sc]
    sim.step()
    for lone in lones:
        lone.step()
    before = sim.levels.clone()
    sim.dt = [sc[0]["dt"], dt_new, sc[2]["dt"]]
    lones[1].dt = dt_new
    sim.level_history = []
    sim.step()
    for lone in lones:
        lone.step()
    lo, hi = int(sim.offsets[1]), int(sim.offsets[2])
    assert not torch.equal(sim.level_history[0][lo:hi], before[lo:hi].cpu())
    for i, lone in enumerate(lones):
        _assert_scene(sim, i, _lone_result(lone, order), order, "new dt between steps")
    sim.max_level = 21
    with pytest.raises(ValueError, match="max_level"):
        sim.step()
    sim.max_level, sim.eta = cases.K, [0.02, -1.0, 0.02]
    with pytest.raises(ValueError, match="positive"):
        sim.step()


# ------------------------------------------------------------------ 11. refusals
@pytest.mark.parametrize("order", ORDERS)
def test_a_corrupt_schedule_record_stops_the_step(gpu_device, order, monkeypatch):
    """The host record is doctored on its way to the Python step; nothing on the device is."""
    from nbd import direct
    sc = [cases.ensemble()[k] for k in (3, 6)]
    sim, twin = _batch(sc, order), _batch(sc, order)
    real = direct.batch_hblock_schedule
    for doctor, text in ((lambda h: h.__setitem__(0, 0), "t_next=0"),
                         (lambda h: h.__setitem__(0, (1 << cases.K) + 1), "t_next=17"),
                         (lambda h: h.__setitem__(1, 0), "n_act=0"),
                         (lambda h: h.__setitem__(1, sim.n + 1), f"n_act={sim.n + 1}")):
        def doctored(*args, host_sched=None, **kw):
            real(*args, host_sched=host_sched, **kw)
            doctor(host_sched)
        fresh = _batch(sc, order)
        monkeypatch.setattr(direct, "batch_hblock_schedule", doctored)
        with pytest.raises(RuntimeError, match=f"corrupt schedule.*{text}"):
            fresh.step()
        monkeypatch.setattr(direct, "batch_hblock_schedule", real)
        for nm in cases.STATE[order]:                                   # refused before the block step's launches
            assert torch.equal(getattr(fresh, nm), getattr(twin, nm)), nm
    sim.integrator = cases.SHARED[order]
    with pytest.raises(ValueError, match="block"):
        sim.step()
    sim.integrator = cases.INTEGRATOR[10 - order]
    with pytest.raises(ValueError, match="block"):
        sim.run(1)
    sim.integrator = cases.INTEGRATOR[order]
    shared = _batch(sc, order, integrator=cases.SHARED[order], dtype=F64)
    shared.integrator = cases.INTEGRATOR[order]
    with pytest.raises(ValueError, match="block"):
        shared.step()
    with pytest.raises(ValueError, match="block integrators only"):
        _batch(sc, order, integrator="hermite", dtype=F64).scene_counters()
    if order == 4:
        with pytest.raises(ValueError, match="hermite6"):
            sim.compute_accelerations_jerks_and_snaps()
    else:
        a, j, s = sim.compute_accelerations_jerks_and_snaps()
        assert torch.equal(a, sim.accelerations) and torch.equal(s, sim.snaps)


# ------------------------------------------------------------------ 12. the other simulators are untouched
def test_the_other_simulators_are_untouched(gpu_device):
    """The one-system block simulators (both orders) and the shared-timestep float64 batches, built and stepped beside the
    two batched block modes, give what a second instance of each gives on its own, bit for bit."""
    sc = [cases.ensemble()[k] for k in (3, 6, 7)]

    def others():
        return ([_lone(sc[2], o) for o in ORDERS] +
                [_batch(sc, o, integrator=cases.SHARED[o], dtype=F64) for o in ORDERS] +
                [_batch(sc, 4, integrator="leapfrog")])

    first = others()
    blocks = [_batch(sc, o) for o in ORDERS]
    for _ in range(2):
        for sim in blocks + first:
            sim.step()
    second = others()
    for a, b in zip(first, second):
        b.step(); b.step()
        for nm in cases.STATE[6]:
            x, y = getattr(a, nm, None), getattr(b, nm, None)
            if x is not None:
                assert x.dtype == y.dtype and torch.equal(x, y), (type(a).__name__, a.__dict__.get("integrator"), nm)
        if getattr(a, "levels", None) is not None:
            assert torch.equal(a.levels, b.levels) and a.block_steps == b.block_steps > 2
    assert all(b.block_steps > 2 and b.positions.dtype == F64 for b in blocks)
