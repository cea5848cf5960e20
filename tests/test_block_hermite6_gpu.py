"""BlockHermite6Simulator and the nbd_hblock6_*_f64 / nbd_accel_jerk_snap_active_f64 kernels on the MI355X
(the 6th order of csrc/direct_hermite_block_f64.hip): max_level 0 is Hermite6Simulator bit for bit, the active-subset
force at the accuracy bars of tests/hermite_f64_oracle.py and bit-equal to the all-bodies kernel, levels and state against the fp64 block oracle
(tests/block_hermite6_oracle.py), the eccentric orbit the order pays on, run() against eager steps and the edge cases of
the 4th-order block mode. No input is fp32-representable (the orbit: see block_hermite_f64_cases.orbit), and every
workspace is NaN-filled before a call."""
import functools

import numpy as np
import pytest
import torch

import block_hermite6_cases as c6
import block_hermite_f64_cases as bc
import block_hermite_oracle as bo
import hermite6_oracle as h6
import hermite_f64_oracle as fo
import hermite_oracle as ho
from conftest import load_golden

pytestmark = pytest.mark.gpu

G, EPS = 1.0, 0.05
F64 = torch.float64
GOLDENS = ["direct_plummer_n64_eps0", "direct_plummer_n300_ragged_mass"]
NAN = float("nan")
STATE = ("positions", "velocities", "accelerations", "jerks", "snaps", "crackles")


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
    if cls == "BlockHermiteSimulator":
        kw.setdefault("dtype", F64)
    sim = getattr(simulation, cls)(positions=x, velocities=v, masses=m, device="cuda", **kw)
    if sim._f64:
        _nan_fill(sim._hws)
        if cls.startswith("Block"):
            _nan_fill(sim._bws)
    return sim


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, v, m, g, eps, a, j, s, sum|a terms|, sum|j terms|, sum|s terms|), the snap on the oracle's acceleration rows;
    computed once and never written to."""
    if isinstance(name, int):
        x, v, m = fo.plummer_case(name, seed=700 + name)
        g, eps = G, EPS
    else:
        gd = load_golden(name)
        x, v, m = fo.perturbed(gd["pos"], gd["vel"], gd["mass"], 5)
        g, eps = float(gd["g_const"]), float(gd["softening"])
    a, j = fo.accel_jerk(x, v, m, g, eps * eps)
    sa, sj = fo.accel_jerk_abs(x, v, m, g, eps * eps)
    s, ss = h6.snap_and_abs(x, v, a, m, g, eps * eps)
    out = (x, v, m, g, eps, a, j, s, sa, sj, ss)
    for arr in out:
        if isinstance(arr, np.ndarray):
            arr.setflags(write=False)
    return out


# ---------------------------------------------------------------- 1. max_level = 0 is the shared 6th-order step
@pytest.mark.parametrize("name", [1, 2, 65, 449, 1000] + GOLDENS)
def test_max_level_zero_is_the_shared_step_bit_for_bit(gpu_device, name):
    x, v, m, g, eps, *_ = _case(name)
    n = x.shape[0]
    kw = dict(g_const=g, softening=eps, dt=0.01, calc_energy=True)
    for steps in (1, 10):
        shared = _sim("Hermite6Simulator", x, v, m, **kw)
        block = _sim("BlockHermite6Simulator", x, v, m, max_level=0, **kw)
        for f in STATE:
            assert torch.equal(getattr(shared, f), getattr(block, f)), (name, f)
        for k in range(steps):
            shared.step()
            _nan_fill(block._bws)
            held = [getattr(block, f).data_ptr() for f in STATE]
            block.step()
            assert held == [getattr(block, f).data_ptr() for f in STATE]          # updated in place
            for f in STATE:
                a, b = getattr(shared, f), getattr(block, f)
                assert b.dtype == F64 and torch.equal(a, b), (name, steps, k, f)
        assert shared.compute_energies() == block.compute_energies(), (name, steps)
        assert block.pair_interactions == steps * n * n and block.block_steps == steps
        assert _np(block.levels).max() == 0      # (bodies that want a deeper level are clamped to it, and counted)


# ---------------------------------------------------------------- 2. the active-subset force
def _rows(x, v, a, m, device):
    from nbd import direct
    n = x.shape[0]
    posd, veld, accd = (direct.alloc_rows_f64(n, device) for _ in range(3))
    direct.hermite6_pack(_dev(x, device), _dev(v, device), _dev(m, device), posd, veld, accd, acc=_dev(a, device))
    return posd, veld, accd


def _active(rows, n, idx, eps2, g, device, slabs=0):
    from nbd import direct
    act = torch.tensor(np.asarray(idx), dtype=torch.int32, device=device)
    ws = _nan_fill(direct.hblock6_workspace(n, device, slabs, act.numel()))
    out = direct.accel_jerk_snap_active_f64(*rows, n, act, eps2, g, workspace=ws, slabs=slabs)
    assert all(t.dtype == F64 and t.shape == (len(idx), 3) for t in out)
    return tuple(_np(t) for t in out)


def _full(rows, n, eps2, g, device, slabs=0):
    from nbd import direct
    ws = _nan_fill(direct.hermite6_workspace(n, device, slabs))
    return tuple(_np(t) for t in direct.accel_jerk_snap_f64(*rows, n, eps2, g, workspace=ws, slabs=slabs))


def _check_rows(tag, got, idx, a, j, s, sa, sj, ss):
    """The bars of the float64 block test for a and j (T = n, 4 n) and of test_hermite6_gpu.py for the snap (T = 19 n)."""
    n = a.shape[0]
    ok_a, fa = fo.within(got[0], a[idx], n, sa[idx])
    ok_j, fj = fo.within(got[1], j[idx], 4 * n, sj[idx])
    ok_s, fs = fo.within(got[2], s[idx], 19 * n, ss[idx])
    print(f"{tag}: |a - ref| / bar = {fa:.3f}, |j - ref| / bar = {fj:.3f}, |s - ref| / bar = {fs:.3f}")
    assert ok_a and ok_j and ok_s, (tag, fa, fj, fs)


def _all_shuffled_is_the_full_kernel(tag, rows, n, eps2, g, device, rng, case, slabs=0):
    order = rng.permutation(n)
    got = _active(rows, n, order, eps2, g, device, slabs)
    _check_rows(f"{tag} all", got, order, *case)
    full = _full(rows, n, eps2, g, device, slabs)
    for name, part, whole in zip("ajs", got, full):
        back = np.empty_like(part)
        back[order] = part
        assert np.array_equal(back, whole), (tag, name)      # bit-equal, in any list order


@pytest.mark.parametrize("name", [1, 2, 63, 64, 65, 130, 449, 1000, 5000] + GOLDENS)
def test_active_subset_force_at_the_bar(gpu_device, name):
    """The goldens add the index-masked walk (softening 0) and a massless body; n_act crosses 64 between the lists."""
    x, v, m, g, eps, a, *case = _case(name)
    if not isinstance(name, int):
        assert (eps == 0.0) == name.endswith("eps0") and ((m == 0).any() == ("ragged_mass" in name))
    n = x.shape[0]
    rows = _rows(x, v, a, m, gpu_device)
    rng = np.random.default_rng(n)
    lists = {"one": np.array([n // 2]), "ragged": np.sort(rng.choice(n, size=max(1, (3 * n) // 7), replace=False)),
             "unordered": rng.permutation(n)[: max(1, n - n // 5)]}
    for kind, idx in lists.items():
        got = _active(rows, n, idx, eps * eps, g, gpu_device)
        _check_rows(f"n={name} {kind} ({idx.size})", got, idx, a, *case)
    _all_shuffled_is_the_full_kernel(f"n={name}", rows, n, eps * eps, g, gpu_device, rng, (a, *case))


@pytest.mark.parametrize("n,slabs", [(1000, 3), (5000, 1), (130, 1)])
def test_active_force_with_an_explicit_split(gpu_device, n, slabs):
    """An uneven split (1000 / 3), 19 to 20 chunks per wave with both LDS buffers reused (5000 / 1), a wave without a
    chunk (130 / 1: three chunks on four waves); the shuffled all-bodies list is nbd_accel_jerk_snap_f64 at the same
    split."""
    x, v, m, g, eps, a, *case = _case(n)
    rows = _rows(x, v, a, m, gpu_device)
    rng = np.random.default_rng(slabs)
    idx = np.sort(rng.choice(n, size=(3 * n) // 7, replace=False))
    got = _active(rows, n, idx, eps * eps, g, gpu_device, slabs)
    _check_rows(f"n={n} slabs={slabs} ragged", got, idx, a, *case)
    _all_shuffled_is_the_full_kernel(f"n={n} slabs={slabs}", rows, n, eps * eps, g, gpu_device, rng, (a, *case), slabs)


def test_active_force_of_a_short_list_on_many_slabs(gpu_device):
    """70 entries at n = 5000 with slabs = 64: two groups (the second of 6 entries), 79 chunks on 256 waves."""
    n = 5000
    x, v, m, g, eps, a, *case = _case(n)
    rows = _rows(x, v, a, m, gpu_device)
    idx = np.random.default_rng(70).permutation(n)[:70]
    got = _active(rows, n, idx, eps * eps, g, gpu_device, 64)
    _check_rows("n=5000 n_act=70 slabs=64", got, idx, a, *case)


def test_cancellation_case(gpu_device):
    """test_block_hermite_f64_gpu.py's: two bodies 2e-9 apart at x = 1 with eps = 1e-10 and a third far away, listed
    [1, 0], the acceleration rows (non-zero: ~1e16 for the pair) from the oracle."""
    rng = np.random.default_rng(3)
    x = np.array([[1.0 - 1e-9, 0.0, 0.0], [1.0 + 1e-9, 0.0, 0.0], [-50.0, 3.0, 2.0]])
    v = rng.uniform(-1, 1, (3, 3))
    m = np.array([0.3, 0.5, 0.2]) + rng.uniform(-1, 1, 3) * 1e-9
    eps = 1e-10
    a, j = fo.accel_jerk(x, v, m, G, eps * eps)
    sa, sj = fo.accel_jerk_abs(x, v, m, G, eps * eps)
    s, ss = h6.snap_and_abs(x, v, a, m, G, eps * eps)
    assert np.abs(a[:2]).max() > 1e16                     # the close pair dominates: s^3 ~ 1e26
    rows = _rows(x, v, a, m, gpu_device)
    assert _np(rows[2][:3, :3]).any()
    idx = np.array([1, 0])
    got = _active(rows, 3, idx, eps * eps, G, gpu_device)
    _check_rows("cancellation", got, idx, a, j, s, sa, sj, ss)


# ---------------------------------------------------------------- 3. levels and state against the fp64 oracle
def _watch_crackles(sim, failed):
    """Wrap the block step of sim's format object (which is returned, to be put back): after every block step the crackle
    of each listed body is the c1 formula on the simulator's own (a, j, s) before and after, with the body's own step,
    componentwise within 16 * 2^-53 of the sum of its |terms| (test_hermite6_gpu.py's bar and factor)."""
    inner = sim._fmt

    def step(fmt, s, n_act):
        act = _np(sim._bws[: 4 * n_act].view(torch.int32)).astype(np.int64)
        h = (sim.dt * 2.0 ** -_np(sim.levels)[act].astype(np.float64))[:, None]
        before = [_np(t)[act] for t in (sim.accelerations, sim.jerks, sim.snaps)]
        inner.block_step(s, n_act)
        after = [_np(t)[act] for t in (sim.accelerations, sim.jerks, sim.snaps)]
        err = np.abs(_np(sim.crackles)[act] - h6.crackle(*before, *after, h))
        tol = 16 * fo.U53 * h6.crackle_abs(*before, *after, h)
        if not np.all(err <= tol):
            failed.append((sim.block_steps, float((err / tol).max())))
    sim._fmt = type("Watched", (type(inner),), {"block_step": step})()
    return inner


@pytest.mark.parametrize("eps", [0.0, 0.01])
def test_levels_and_state_match_the_fp64_oracle(gpu_device, eps):
    """One output step: the oracle's level history, block steps, pair interactions, nothing clamped -- exactly; the crackle
    of every block step at its own bar (_watch_crackles: it divides rounding differences by h^3, so it is not compared
    across runs). Four: pos, vel, acc, jerk, snap within 8 s_k + 8 * 2^-53 max|value| of the oracle, s_k = the largest
    difference between the oracle run and the same run under three fixed permutations of the bodies (the float64 block
    test's rule), and the oracle's levels."""
    x, v, m = c6.planted(eps)
    want = c6.planted_run(eps, 1)
    sim = _sim("BlockHermite6Simulator", x, v, m, softening=eps, dt=c6.DT, eta=c6.ETA, max_level=c6.K)
    sim.level_history = []
    bad_crackles = []
    fmt = _watch_crackles(sim, bad_crackles)
    sim.step()
    sim._fmt = fmt
    assert sim.block_steps == want["block_steps"] and sim.pair_interactions == want["pair_interactions"]
    assert len(sim.level_history) == len(want["history"])
    for k, (a, b) in enumerate(zip(sim.level_history, want["history"])):
        assert np.array_equal(a.numpy(), b), k
    assert sim.clamped == want["clamped"] == 0
    assert not bad_crackles, bad_crackles
    sim.level_history = None
    for _ in range(3):
        sim.step()
    want4, spread = c6.planted_run(eps, 4), c6.permutation_spread(eps, 4)
    assert sim.block_steps == want4["block_steps"] and np.array_equal(_np(sim.levels), want4["levels"])
    assert sim.clamped == 0
    failed = []
    for name, key in zip(STATE[:5], "xvajs"):
        ref = want4[key]
        dist = np.abs(_np(getattr(sim, name)) - ref).max()
        tol = 8 * spread[key] + 8 * fo.U53 * np.abs(ref).max()
        print(f"eps={eps} 4 steps {name}: s_k = {spread[key]:.3e}, |gpu - oracle| = {dist:.3e}, tolerance {tol:.3e}")
        if not dist <= tol:
            failed.append((name, dist, tol))
    assert not failed, failed


# ---------------------------------------------------------------- 4. the reason for the feature
def test_the_order_pays_on_the_eccentric_orbit(gpu_device):
    """e = 0.9, eps = 0, one period as 4 output steps, eta = 0.01, max_level 16. The run takes the oracle's pair
    interactions and ends within 2x the oracle's own orbit error (truncation, ~1e-10: fp64 rounding is orders below it),
    at least 10x below BlockHermiteSimulator(dtype=torch.float64) at its eta = 0.000625, with fewer pair interactions."""
    x0, v0, m, dt = bc.orbit()
    want = c6.orbit_run(0.01)
    six = _sim("BlockHermite6Simulator", x0, v0, m, softening=0.0, dt=dt, eta=0.01, max_level=c6.ORBIT_K)
    four = _sim("BlockHermiteSimulator", x0, v0, m, softening=0.0, dt=dt, eta=bc.ORBIT_ETA, max_level=bc.ORBIT_K)
    for _ in range(4):
        six.step()
        four.step()
    err6 = ho.orbit_error(_np(six.positions), x0)
    err4 = ho.orbit_error(_np(four.positions), x0)
    print(f"e=0.9 orbit: 6th order eta=0.01 {err6:.3e} at {six.pair_interactions} pairs (oracle {want['err']:.3e} at "
          f"{want['pair_interactions']}), 4th order eta={bc.ORBIT_ETA} {err4:.3e} at {four.pair_interactions} pairs, "
          f"clamped {six.clamped} / {four.clamped}")
    assert six.pair_interactions == want["pair_interactions"] and six.clamped == 0
    assert err6 <= 2 * want["err"], (err6, want["err"])
    assert err4 >= 10 * err6, (err4, err6)
    assert six.pair_interactions < four.pair_interactions


# ---------------------------------------------------------------- 5. behaviour
def test_run_is_eager_float64_and_bit_identical_to_steps(gpu_device):
    n, steps = 130, 6
    x, v, m, *_ = _case(n)
    kw = dict(dt=c6.DT, softening=0.01, calc_energy=True, calc_invariants=True, max_level=6)
    ran, twin, again = (_sim("BlockHermite6Simulator", x, v, m, **kw) for _ in range(3))
    _nan_fill(again._bws).view(torch.uint8)[again._bws.numel() // 2:] = 0x5A      # other garbage than the first run's
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
    for f in STATE:
        assert torch.equal(getattr(ran, f), getattr(twin, f)), f
    assert torch.equal(ran.levels, twin.levels) and ran.block_steps == twin.block_steps > steps
    for s, t in zip(states, again.run(steps)):                # deterministic, whatever the workspace held
        assert torch.equal(s.positions, t.positions) and torch.equal(s.velocities, t.velocities)
        assert torch.equal(s.accelerations, t.accelerations)
        assert (s.u_energy, s.k_energy, s.invariants) == (t.u_energy, t.k_energy, t.invariants)
    for f in STATE:
        assert torch.equal(getattr(ran, f), getattr(again, f)), f
    assert (ran.block_steps, ran.pair_interactions, ran.clamped) == (again.block_steps, again.pair_interactions,
                                                                     again.clamped)


def test_changing_dt_re_derives_the_levels(gpu_device):
    x, v, m = fo.perturbed(*bo.planted_binary_sphere(200, 7), 3)
    K = 8
    sim = _sim("BlockHermite6Simulator", x, v, m, softening=0.01, dt=c6.DT, max_level=K)
    sim.run(2)
    before = _np(sim.levels).copy()
    sim.dt = 8 * c6.DT
    a, j = _np(sim.accelerations), _np(sim.jerks)
    crit = 0.5 * sim.eta * np.linalg.norm(a, axis=1) / np.linalg.norm(j, axis=1)
    expect = np.minimum([bo.wanted_level(c, sim.dt, K) for c in crit], K)
    assert not np.array_equal(expect, before)
    sim.level_history = []
    sim.run(1)
    first = sim.level_history[0].numpy()
    inactive = expect < expect.max()                          # the first block step moves the deepest level only
    assert inactive.any() and np.array_equal(first[inactive], expect[inactive])
    assert sim._leveled_for == (8 * c6.DT, sim.eta, K)
    sim.max_level = 21
    with pytest.raises(ValueError, match="max_level"):
        sim.step()


def test_a_lone_body_takes_one_block_step_per_interval(gpu_device):
    """No force and no derivative of it: den == 0, the criterion is +inf, level 0."""
    x, v = np.array([[0.3 + 1e-10, 0.1, 1e-11]]), np.array([[1e-11, 0.25 + 1e-10, 1e-12]])
    sim = _sim("BlockHermite6Simulator", x, v, np.array([1.0 + 1e-10]), softening=0.0, dt=0.125, max_level=6)
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
    sim = _sim("BlockHermite6Simulator", x, v, m, softening=0.0, dt=0.01, max_level=3)
    sim.step()
    assert sim.block_steps <= 8 and sim.clamped > 0
    sim.step()
    assert sim.block_steps <= 16


def test_the_other_simulators_are_untouched(gpu_device):
    """BlockHermiteSimulator (both formats) and Hermite6Simulator built and stepped beside a BlockHermite6Simulator give
    what a second instance of each gives on its own, bit for bit."""
    x, v, m = fo.perturbed(*bo.planted_binary_sphere(300, 5), 3)
    kw = dict(softening=0.01, dt=c6.DT)
    blk = dict(eta=0.02, max_level=8, **kw)
    first = [_sim("BlockHermiteSimulator", x, v, m, **blk), _sim("BlockHermiteSimulator", x, v, m, dtype=torch.float32, **blk),
             _sim("Hermite6Simulator", x, v, m, **kw)]
    six = _sim("BlockHermite6Simulator", x, v, m, **blk)
    for _ in range(2):
        six.step()
        for sim in first:
            sim.step()
    second = [_sim("BlockHermiteSimulator", x, v, m, **blk), _sim("BlockHermiteSimulator", x, v, m, dtype=torch.float32, **blk),
              _sim("Hermite6Simulator", x, v, m, **kw)]
    for a, b in zip(first, second):
        b.step(); b.step()
        names = STATE if hasattr(a, "snaps") else STATE[:4]
        for f in names:
            assert getattr(a, f).dtype == getattr(b, f).dtype and torch.equal(getattr(a, f), getattr(b, f)), (type(a), f)
        if hasattr(a, "levels"):
            assert torch.equal(a.levels, b.levels) and a.block_steps == b.block_steps > 2
    assert six.block_steps > 2 and six.positions.dtype == F64 and first[1].positions.dtype == torch.float32
