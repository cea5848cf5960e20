"""BlockHermiteSimulator(dtype=torch.float64) and the nbd_hblock_*_f64 / nbd_accel_jerk_active_f64 kernels on the MI355X
(csrc/direct_hermite_block_f64.hip): max_level 0 is HermiteSimulator(dtype=torch.float64) bit for bit, the active-subset
force at the accuracy bar of tests/hermite_f64_oracle.py and bit-equal to the all-bodies kernel, levels and state against
the fp64 block oracle, the eccentric orbit below the fp32 floor, run() against eager steps, and the edge cases of the fp32
mode. No input is fp32-representable (the orbit: see block_hermite_f64_cases.orbit), and every workspace is NaN-filled
before a call.

Measured on the MI355X (the printed figures) are in NOTES.md, "K-HB64"."""
import functools

import numpy as np
import pytest
import torch

import block_hermite_f64_cases as bc
import block_hermite_oracle as bo
import hermite_f64_oracle as fo
import hermite_oracle as ho
from conftest import load_golden

pytestmark = pytest.mark.gpu

G, EPS = 1.0, 0.05
F64 = torch.float64
GOLDENS = ["direct_plummer_n64_eps0", "direct_plummer_n300_ragged_mass"]
NAN = float("nan")


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, device):
    return torch.tensor(np.asarray(a, np.float64), dtype=F64, device=device)


def _nan_fill(ws):
    ws[: ws.numel() // 8 * 8].view(F64).fill_(NAN)
    return ws


def _sim(cls, x, v, m, **kw):
    """A float64 simulator with NaN in every workspace it owns."""
    from galaxify import simulation
    kw.setdefault("g_const", G); kw.setdefault("softening", EPS); kw.setdefault("calc_energy", False)
    kw.setdefault("dtype", F64)
    sim = getattr(simulation, cls)(positions=x, velocities=v, masses=m, device="cuda", **kw)
    if sim._f64:
        _nan_fill(sim._hws)
        if cls == "BlockHermiteSimulator":
            _nan_fill(sim._bws)
    return sim


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, v, m, g, eps, a, j, sum|a terms|, sum|j terms|), computed once and never written to."""
    if isinstance(name, int):
        x, v, m = fo.plummer_case(name, seed=200 + name)
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


# ---------------------------------------------------------------- 1. max_level = 0 is the shared fp64 step
@pytest.mark.parametrize("name", [1, 2, 65, 449, 1000] + GOLDENS)
def test_max_level_zero_is_the_shared_f64_step_bit_for_bit(gpu_device, name):
    x, v, m, g, eps, *_ = _case(name)
    n = x.shape[0]
    kw = dict(g_const=g, softening=eps, dt=0.01, calc_energy=True)
    for steps in (1, 10):
        shared = _sim("HermiteSimulator", x, v, m, **kw)
        block = _sim("BlockHermiteSimulator", x, v, m, max_level=0, **kw)
        assert torch.equal(shared.accelerations, block.accelerations) and torch.equal(shared.jerks, block.jerks)
        for k in range(steps):
            shared.step()
            _nan_fill(block._bws)
            block.step()
            for f in ("positions", "velocities", "accelerations", "jerks"):
                a, b = getattr(shared, f), getattr(block, f)
                assert b.dtype == F64 and torch.equal(a, b), (name, steps, k, f)
        assert shared.compute_energies() == block.compute_energies(), (name, steps)
        assert block.pair_interactions == steps * n * n and block.block_steps == steps
        assert _np(block.levels).max() == 0


# ---------------------------------------------------------------- 2. the active-subset force
def _rows(x, v, m, device):
    from nbd import direct
    n = x.shape[0]
    posd, veld = direct.alloc_rows_f64(n, device), direct.alloc_rows_f64(n, device)
    direct.hermite_f64_pack(_dev(x, device), _dev(v, device), _dev(m, device), posd, veld)
    return posd, veld


def _active(posd, veld, n, idx, eps2, g, device, slabs=0):
    from nbd import direct
    act = torch.tensor(np.asarray(idx), dtype=torch.int32, device=device)
    ws = _nan_fill(direct.hblock_f64_workspace(n, device, slabs, act.numel()))
    a, j = direct.accel_jerk_active_f64(posd, veld, n, act, eps2, g, workspace=ws, slabs=slabs)
    assert a.dtype == F64 and a.shape == (len(idx), 3) and j.shape == (len(idx), 3)
    return _np(a), _np(j)


def _full(posd, veld, n, eps2, g, device, slabs=0):
    from nbd import direct
    ws = _nan_fill(direct.hermite_f64_workspace(n, device, slabs))
    a, j = direct.accel_jerk_f64(posd, veld, n, eps2, g, workspace=ws, slabs=slabs)
    return _np(a), _np(j)


def _check_rows(tag, got_a, got_j, idx, a, j, sa, sj):
    n = a.shape[0]
    ok_a, fa = fo.within(got_a, a[idx], n, sa[idx])
    ok_j, fj = fo.within(got_j, j[idx], 4 * n, sj[idx])
    print(f"{tag}: |a - ref| / bar = {fa:.3f}, |j - ref| / bar = {fj:.3f}")
    assert ok_a and ok_j, (tag, fa, fj)


def _all_shuffled_is_the_full_kernel(tag, posd, veld, n, eps2, g, device, rng, case, slabs=0):
    order = rng.permutation(n)
    got_a, got_j = _active(posd, veld, n, order, eps2, g, device, slabs)
    _check_rows(f"{tag} all", got_a, got_j, order, *case)
    back_a, back_j = np.empty_like(got_a), np.empty_like(got_j)
    back_a[order], back_j[order] = got_a, got_j
    full_a, full_j = _full(posd, veld, n, eps2, g, device, slabs)
    assert np.array_equal(back_a, full_a) and np.array_equal(back_j, full_j), tag      # bit-equal, in any list order


@pytest.mark.parametrize("name", [1, 2, 63, 64, 65, 130, 449, 1000, 5000] + GOLDENS)
def test_active_subset_force_at_the_bar(gpu_device, name):
    """The goldens add the index-masked walk (softening 0) and a massless body; n_act crosses 64 between the lists."""
    x, v, m, g, eps, a, j, sa, sj = _case(name)
    if not isinstance(name, int):
        assert (eps == 0.0) == name.endswith("eps0") and ((m == 0).any() == ("ragged_mass" in name))
    n = x.shape[0]
    posd, veld = _rows(x, v, m, gpu_device)
    rng = np.random.default_rng(n)
    lists = {"one": np.array([n // 2]), "ragged": np.sort(rng.choice(n, size=max(1, (3 * n) // 7), replace=False)),
             "unordered": rng.permutation(n)[: max(1, n - n // 5)]}
    for kind, idx in lists.items():
        got_a, got_j = _active(posd, veld, n, idx, eps * eps, g, gpu_device)
        _check_rows(f"n={name} {kind} ({idx.size})", got_a, got_j, idx, a, j, sa, sj)
    _all_shuffled_is_the_full_kernel(f"n={name}", posd, veld, n, eps * eps, g, gpu_device, rng, (a, j, sa, sj))


@pytest.mark.parametrize("n,slabs", [(1000, 3), (5000, 1), (130, 1)])
def test_active_force_with_an_explicit_split(gpu_device, n, slabs):
    """An uneven split (1000 / 3), 19 to 20 chunks per wave with both LDS buffers reused (5000 / 1), a wave without a
    chunk (130 / 1: three chunks on four waves); the shuffled all-bodies list is nbd_accel_jerk_f64 at the same split."""
    x, v, m, g, eps, a, j, sa, sj = _case(n)
    posd, veld = _rows(x, v, m, gpu_device)
    rng = np.random.default_rng(slabs)
    idx = np.sort(rng.choice(n, size=(3 * n) // 7, replace=False))
    got_a, got_j = _active(posd, veld, n, idx, eps * eps, g, gpu_device, slabs)
    _check_rows(f"n={n} slabs={slabs} ragged", got_a, got_j, idx, a, j, sa, sj)
    _all_shuffled_is_the_full_kernel(f"n={n} slabs={slabs}", posd, veld, n, eps * eps, g, gpu_device, rng,
                                     (a, j, sa, sj), slabs)


def test_active_force_of_a_short_list_on_many_slabs(gpu_device):
    """70 entries at n = 5000 with slabs = 64: two groups (the second of 6 entries), 79 chunks on 256 waves."""
    n = 5000
    x, v, m, g, eps, a, j, sa, sj = _case(n)
    posd, veld = _rows(x, v, m, gpu_device)
    idx = np.random.default_rng(70).permutation(n)[:70]
    got_a, got_j = _active(posd, veld, n, idx, eps * eps, g, gpu_device, 64)
    _check_rows("n=5000 n_act=70 slabs=64", got_a, got_j, idx, a, j, sa, sj)


def test_cancellation_case(gpu_device):
    """test_hermite_f64_gpu.py's: two bodies 2e-9 apart at x = 1 with eps = 1e-10 and a third far away, listed [1, 0]."""
    rng = np.random.default_rng(3)
    x = np.array([[1.0 - 1e-9, 0.0, 0.0], [1.0 + 1e-9, 0.0, 0.0], [-50.0, 3.0, 2.0]])
    v = rng.uniform(-1, 1, (3, 3))
    m = np.array([0.3, 0.5, 0.2]) + rng.uniform(-1, 1, 3) * 1e-9
    eps = 1e-10
    a, j = fo.accel_jerk(x, v, m, G, eps * eps)
    sa, sj = fo.accel_jerk_abs(x, v, m, G, eps * eps)
    assert np.abs(a[:2]).max() > 1e16                     # the close pair dominates: s^3 ~ 1e26
    posd, veld = _rows(x, v, m, gpu_device)
    idx = np.array([1, 0])
    got_a, got_j = _active(posd, veld, 3, idx, eps * eps, G, gpu_device)
    _check_rows("cancellation", got_a, got_j, idx, a, j, sa, sj)


# ---------------------------------------------------------------- 3. levels and state against the fp64 oracle
@pytest.mark.parametrize("eps", [0.0, 0.01])
def test_levels_and_state_match_the_fp64_oracle(gpu_device, eps):
    """One output step: the oracle's level history, block steps, pair interactions, nothing clamped -- exactly. Four: pos,
    vel, acc, jerk within 8 s_k + 8 * 2^-53 max|value| of the oracle, s_k = the largest difference between the oracle run
    and the same run under three fixed permutations of the bodies (test_steps_against_the_oracle's rule: the factor 8 is
    for another reciprocal square root and another order of the sums)."""
    x, v, m = bc.planted(eps)
    want = bc.planted_run(eps, 1)
    sim = _sim("BlockHermiteSimulator", x, v, m, softening=eps, dt=bc.DT, eta=bc.ETA, max_level=bc.K)
    sim.level_history = []
    sim.step()
    assert sim.block_steps == want["block_steps"] and sim.pair_interactions == want["pair_interactions"]
    assert len(sim.level_history) == len(want["history"])
    for k, (a, b) in enumerate(zip(sim.level_history, want["history"])):
        assert np.array_equal(a.numpy(), b), k
    assert sim.clamped == want["clamped"] == 0
    sim.level_history = None
    for _ in range(3):
        sim.step()
    want4, spread = bc.planted_run(eps, 4), bc.permutation_spread(eps, 4)
    assert sim.block_steps == want4["block_steps"] and np.array_equal(_np(sim.levels), want4["levels"])
    failed = []
    for name, key, got in (("pos", "x", sim.positions), ("vel", "v", sim.velocities), ("acc", "a", sim.accelerations),
                           ("jerk", "j", sim.jerks)):
        ref = want4[key]
        dist = np.abs(_np(got) - ref).max()
        tol = 8 * spread[name] + 8 * fo.U53 * np.abs(ref).max()
        print(f"eps={eps} 4 steps {name}: s_k = {spread[name]:.3e}, |gpu - oracle| = {dist:.3e}, tolerance {tol:.3e}")
        if not dist <= tol:
            failed.append((name, dist, tol))
    assert not failed, failed


# ---------------------------------------------------------------- 4. the reason for the feature
def test_eccentric_orbit_goes_below_the_fp32_floor(gpu_device):
    """e = 0.9, eps = 0, one period as 4 output steps, eta = 0.000625, max_level 16. The fp64 run takes the oracle's pair
    interactions and ends within 2x the oracle's own orbit error (truncation, ~5e-9: fp64 rounding is orders below it, so
    the 2 only absorbs a different last digit), at least 100x below the fp32 mode at the same eta."""
    x0, v0, m, dt = bc.orbit()
    want = bc.orbit_run()
    kw = dict(softening=0.0, dt=dt, eta=bc.ORBIT_ETA, max_level=bc.ORBIT_K)
    wide = _sim("BlockHermiteSimulator", x0, v0, m, **kw)
    narrow = _sim("BlockHermiteSimulator", x0, v0, m, dtype=torch.float32, **kw)
    for _ in range(4):
        wide.step()
        narrow.step()
    err64 = ho.orbit_error(_np(wide.positions), x0)
    err32 = ho.orbit_error(_np(narrow.positions), x0.astype(np.float32))
    print(f"e=0.9 orbit eta={bc.ORBIT_ETA}: fp64 {err64:.3e} at {wide.pair_interactions} pairs (oracle {want['err']:.3e} "
          f"at {want['pair_interactions']}), fp32 {err32:.3e} at {narrow.pair_interactions} pairs, "
          f"clamped {wide.clamped} / {narrow.clamped}")
    assert wide.pair_interactions == want["pair_interactions"] and wide.clamped == 0
    assert err64 <= 2 * want["err"], (err64, want["err"])
    assert err32 >= 100 * err64, (err32, err64)


# ---------------------------------------------------------------- 5. other checks
def test_run_is_eager_float64_and_bit_identical_to_steps(gpu_device):
    n, steps = 130, 6
    x, v, m, *_ = _case(n)
    kw = dict(dt=bc.DT, softening=0.01, calc_energy=True, calc_invariants=True, max_level=6)
    ran, twin, again = (_sim("BlockHermiteSimulator", x, v, m, **kw) for _ in range(3))
    assert not ran._graph_run_ok(steps) and not ran._graph_run_ok(64)
    states = ran.run(steps)
    assert len(states) == steps and [s.step for s in states] == list(range(steps))
    for s in states:
        twin.step()
        for got, want in ((s.positions, twin.positions), (s.velocities, twin.velocities),
                          (s.accelerations, twin.accelerations)):
            assert got.dtype == F64 and not got.is_cuda and torch.equal(got, want.cpu())
        assert (s.u_energy, s.k_energy) == twin.compute_energies()
        assert s.invariants == twin.compute_invariants()
    assert ran._run_stage[0].dtype == F64 and ran._run_stage[0].is_pinned()
    assert torch.equal(ran.positions, twin.positions) and torch.equal(ran.jerks, twin.jerks)
    assert torch.equal(ran.levels, twin.levels) and ran.block_steps == twin.block_steps > steps
    for s, t in zip(states, again.run(steps)):
        assert torch.equal(s.positions, t.positions) and torch.equal(s.velocities, t.velocities)
        assert torch.equal(s.accelerations, t.accelerations)
        assert (s.u_energy, s.k_energy, s.invariants) == (t.u_energy, t.k_energy, t.invariants)
    assert (ran.block_steps, ran.pair_interactions, ran.clamped) == (again.block_steps, again.pair_interactions,
                                                                     again.clamped)


def test_changing_dt_re_derives_the_levels(gpu_device):
    x, v, m = fo.perturbed(*bo.planted_binary_sphere(200, 7), 3)
    K = 8
    sim = _sim("BlockHermiteSimulator", x, v, m, softening=0.01, dt=bc.DT, max_level=K)
    sim.run(2)
    before = _np(sim.levels).copy()
    sim.dt = 8 * bc.DT
    a, j = _np(sim.accelerations), _np(sim.jerks)
    crit = 0.5 * sim.eta * np.linalg.norm(a, axis=1) / np.linalg.norm(j, axis=1)
    expect = np.minimum([bo.wanted_level(c, sim.dt, K) for c in crit], K)
    assert not np.array_equal(expect, before)
    sim.level_history = []
    sim.run(1)
    first = sim.level_history[0].numpy()
    inactive = expect < expect.max()                          # the first block step moves the deepest level only
    assert inactive.any() and np.array_equal(first[inactive], expect[inactive])
    assert sim._leveled_for == (8 * bc.DT, sim.eta, K)


def test_a_lone_body_takes_one_block_step_per_interval(gpu_device):
    x, v = np.array([[0.3 + 1e-10, 0.1, 1e-11]]), np.array([[1e-11, 0.25 + 1e-10, 1e-12]])
    sim = _sim("BlockHermiteSimulator", x, v, np.array([1.0 + 1e-10]), softening=0.0, dt=0.125, max_level=6)
    states = sim.run(3)
    assert sim.block_steps == 3 and sim.clamped == 0 and sim.pair_interactions == 3
    assert _np(sim.levels).tolist() == [0]
    assert states[-1].positions.dtype == F64
    assert np.allclose(states[-1].positions.numpy(), x + 3 * 0.125 * v, rtol=0, atol=1e-15)


def test_coincident_bodies_finish_the_interval(gpu_device):
    """Two coincident bodies at eps = 0: NaN force, NaN criterion, the level clamped to max_level and counted; the interval
    still ends within its 2^max_level block steps."""
    rng = np.random.default_rng(2)
    x = rng.normal(size=(20, 3))
    x[5] = x[4]
    v = 0.1 * rng.normal(size=(20, 3))
    m = np.full(20, 1.0 / 20) + rng.uniform(-1, 1, 20) * 1e-9
    sim = _sim("BlockHermiteSimulator", x, v, m, softening=0.0, dt=0.01, max_level=3)
    sim.step()
    assert sim.block_steps <= 8 and sim.clamped > 0
    sim.step()
    assert sim.block_steps <= 16


def test_default_dtype_is_untouched(gpu_device):
    """A default-dtype simulator built beside a float64 one keeps float32 tensors, and its first interval is
    nbd_hblock_schedule + nbd_hblock_step_f32 driven directly, bit for bit."""
    from galaxify import simulation
    from nbd import direct
    x, v, m = bo.planted_binary_sphere(300, 5)
    K, dt, eta, soft = 8, bc.DT, 0.02, 0.01
    kw = dict(positions=x, velocities=v, masses=m, softening=soft, dt=dt, eta=eta, max_level=K, calc_energy=False,
              device="cuda")
    wide = simulation.BlockHermiteSimulator(dtype=F64, **kw)
    plain = simulation.BlockHermiteSimulator(**kw)
    named = simulation.BlockHermiteSimulator(dtype=torch.float32, **kw)
    assert wide._f64 and wide.positions.dtype == F64 and wide.levels.dtype == torch.int32 and not plain._f64
    for sim in (plain, named):
        assert all(t.dtype == torch.float32 for t in
                   (sim.positions, sim.velocities, sim.masses, sim.accelerations, sim.jerks))
    n = plain.n
    f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=gpu_device)      # noqa: E731
    pos, vel, mass = f32(x), f32(v), f32(m)
    eps2, gcf = direct.f32(soft ** 2), direct.f32(1.0)
    posm, velp = direct.alloc_posm(n, gpu_device), direct.alloc_posm(n, gpu_device)
    direct.hermite_pack(pos, vel, mass, posm, velp)
    acc, jerk = direct.accel_jerk(posm, velp, n, eps2, gcf, workspace=direct.hermite_workspace(n, gpu_device))
    assert torch.equal(acc, plain.accelerations) and torch.equal(jerk, plain.jerks)
    ticks = torch.zeros(n, dtype=torch.int32, device=gpu_device)
    levels = torch.zeros(n, dtype=torch.int32, device=gpu_device)
    sched = torch.zeros(direct.HBLOCK_SCHED_INTS, dtype=torch.int32, device=gpu_device)
    host = torch.zeros(4, dtype=torch.int32).pin_memory()
    bws = direct.hblock_workspace(n, gpu_device)
    direct.hblock_init_levels(acc, jerk, dt, eta, K, ticks, levels, sched)
    assert torch.equal(levels, plain.levels)
    wide.step(); plain.step(); named.step()
    block_steps = 0
    while True:
        direct.hblock_schedule(levels, K, sched, bws, host_sched=host)
        direct.hblock_step(pos, vel, acc, jerk, mass, ticks, levels, int(host[1]), K, dt, eta, eps2, gcf, sched, posm,
                           velp, bws)
        block_steps += 1
        assert block_steps <= 1 << K
        if int(host[0]) == 1 << K:
            break
    for sim in (plain, named):
        assert sim.block_steps == block_steps > 1
        for got, want in ((sim.positions, pos), (sim.velocities, vel), (sim.accelerations, acc), (sim.jerks, jerk),
                          (sim.levels, levels)):
            assert torch.equal(got, want)
    assert wide.positions.dtype == F64 and wide.block_steps >= 1


@pytest.mark.parametrize("order", [4, 6])
def test_a_refused_step_launches_nothing(gpu_device, order):
    """n = 65 with all 65 listed (two target groups, the second ragged) and a workspace 32 bytes short of
    nbd_hblock(6)_f64_workspace_bytes(65), still 32-byte aligned: the step is refused for the size (-2) before its first
    launch, so the packed rows the predictor would overwrite keep their sentinel, bit for bit."""
    from nbd import _lib, direct
    n, K, sentinel = 65, 4, -1234.5625
    rng = np.random.default_rng(65)
    state = [_dev(rng.standard_normal((n, 3)) + 0.1, gpu_device) for _ in range(order)]
    mass = _dev(rng.uniform(0.5, 1.5, n), gpu_device)
    ticks, levels = (torch.zeros(n, dtype=torch.int32, device=gpu_device) for _ in range(2))
    sched = torch.zeros(direct.HBLOCK_SCHED_INTS, dtype=torch.int32, device=gpu_device)
    sched[0], sched[1] = 1 << K, n
    rows = [direct.alloc_rows_f64(n, gpu_device).fill_(sentinel) for _ in range(order // 2)]
    size, step = ((_lib.lib().nbd_hblock_f64_workspace_bytes, direct.hblock_step_f64) if order == 4 else
                  (_lib.lib().nbd_hblock6_f64_workspace_bytes, direct.hblock6_step_f64))
    ws = _nan_fill(torch.empty(size(n) - 32, dtype=torch.uint8, device=gpu_device))
    assert ws.data_ptr() % 32 == 0
    with pytest.raises(_lib.NbdError, match="code -2"):
        step(*state, mass, ticks, levels, n, K, 1.0 / 32, 0.02, EPS * EPS, G, sched, *rows, ws)
    torch.cuda.synchronize()
    want = torch.full_like(rows[0], sentinel).view(torch.int64)
    for r in rows:
        assert torch.equal(r.view(torch.int64), want)


def test_unsupported_dtype_raises(gpu_device):
    from galaxify import simulation
    z = np.zeros((4, 3))
    with pytest.raises(ValueError, match="dtype"):
        simulation.BlockHermiteSimulator(positions=z, velocities=z, masses=np.ones(4), dtype=torch.float16, device="cuda")
