"""Block timesteps over the tree force without a GPU: the fp64 restatements of tests/tree_block_oracle.py against
tests/tree_oracle.py and a plain leapfrog, the schedule the GPU trajectory test will demand, the argument checks of the
new C entries and the refusals of BlockTreeLeapFrogSimulator. No kernel is launched here."""
import ctypes

import numpy as np
import pytest
import torch

import tree_block_oracle as tb
import tree_oracle as to
from nbd import _lib

_cache = {}


def trajectory(max_level):
    """block_leapfrog on the trajectory input with the fp64 direct-sum force, once per max_level."""
    if max_level not in _cache:
        p, v, m = tb.trajectory_case()
        T = tb.TRAJ
        _cache[max_level] = tb.block_leapfrog(p, v, m, T["dt"], T["eta"], max_level, T["steps"], tb.direct_force(m))
    return _cache[max_level]


@pytest.mark.parametrize("theta", [0.0, 0.5])
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_everything_listed_is_the_full_walk_exactly(name, theta):
    p, _, m = to.case(name)
    order = to.morton_order(p)
    full, full_counters = to.tree_accel(p, m, theta, to.SOFTENING, order=order)
    rows, counters = tb.tree_accel_active(p, m, theta, to.SOFTENING, 1.0, True, order, np.arange(len(p)))
    assert counters == full_counters
    assert np.array_equal(rows, full[order])


def test_a_subset_is_one_group_with_its_own_box():
    """One body per full-walk group of case B: 16 targets in ONE group. At theta = 0 that group opens every node once and
    every row is the direct sum; at theta = 0.5 its box spans the system, so nothing that holds a target is accepted."""
    p, _, m = to.case("B")
    order = to.morton_order(p)
    act = np.arange(0, len(p), 64)
    direct = to.direct_accel(p, m, to.SOFTENING)
    exact, counters = tb.tree_accel_active(p, m, 0.0, to.SOFTENING, 1.0, True, order, act)
    assert counters == (0, -(-len(p) // 8)) and to.row_errors(exact, direct[order[act]]).max() < 1e-12
    rows, (cells, leaves) = tb.tree_accel_active(p, m, 0.5, to.SOFTENING, 1.0, True, order, act)
    assert leaves >= len(act) and np.isfinite(rows).all()        # at least the targets' own level-0 nodes are opened


def test_max_level_0_is_the_plain_leapfrog_exactly():
    p, v, m = to.case("B")
    force = tb.direct_force(m)
    block = tb.block_leapfrog(p, v, m, 0.01, 0.025, 0, 3, force)
    plain = tb.plain_leapfrog(p, v, 0.01, 3, force)
    assert block["n_act"] == [len(p)] * 3 and all((lv == 0).all() for lv in block["levels"])
    for got, want in zip(block["states"], plain):
        for a, b in zip(got, want):
            assert np.array_equal(a, b)


def test_the_trajectory_input_has_a_schedule_a_gpu_can_follow():
    """max_level = 4 on the trajectory input: the levels span three values, every body is back in step after each
    step(), and no level decision is closer than 1e-3 (relative) to the edge of its level -- 500 times what the fp32 tree
    force at theta = 0 is from the fp64 direct sum -- so the GPU run must take the same levels at the same block steps."""
    r = trajectory(tb.TRAJ["max_level"])
    n = tb.TRAJ["n"]
    seen = np.unique(np.concatenate(r["levels"]))
    print(f"levels seen {seen}, {len(r['n_act'])} block steps, sum n_act {sum(r['n_act'])}, margin {r['margin']:.3e}")
    assert len(seen) >= 3
    assert len(r["states"]) == tb.TRAJ["steps"] and sum(k == n for k in r["n_act"]) >= tb.TRAJ["steps"]
    assert r["clamped"] == 0
    assert r["margin"] >= 1e-3
    assert sum(r["n_act"]) < n * len(r["n_act"])                 # some block steps evaluate a subset


def test_the_clamp_input_clamps_with_the_same_margin():
    r = trajectory(1)
    print(f"max_level = 1: clamped {r['clamped']}, block steps {len(r['n_act'])}, margin {r['margin']:.3e}")
    assert r["clamped"] > 0 and len(r["n_act"]) <= 2 * tb.TRAJ["steps"] and r["margin"] >= 1e-3


def test_wanted_level_edges():
    acc = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [1e6, 0, 0]], dtype=np.float32)
    # (2 eta eps)^2 = 2.5e-5 with eta = 0.025, eps = 0.1; dt = 0.1: h_k^4 = 1e-4 16^-k, so |a| = 1 wants k = 1
    level, over, _ = tb.wanted_level(acc, 0.1, 0.025, 0.1, 4)
    assert level.tolist() == [0, 1, 4, 4] and over.tolist() == [False, False, True, True]


# ---------------------------------------------------------------- the C entries' argument checks (no launch)

def test_active_workspace_query():
    L = _lib.lib()
    assert L.nbd_tree_active_workspace_bytes(0) == 0 and L.nbd_tree_active_workspace_bytes(-1) == 0
    assert L.nbd_tree_active_workspace_bytes((1 << 24) + 1) == 0
    small, big = L.nbd_tree_active_workspace_bytes(300), L.nbd_tree_active_workspace_bytes(100000)
    assert 300 * 5 < small < big and small % 256 == 0 and big >= 100000 * 5


def test_listed_walk_refusals_launch_nothing():
    L = _lib.lib()
    n = 300
    fake = ctypes.c_void_p(256 * 4096)                   # never dereferenced: every case below returns before a launch
    ws_n = L.nbd_tree_workspace_bytes(n)
    args = (0.5, 0.01, 1.0, 1, fake, None, None)
    assert L.nbd_tree_accel_active_f32(fake, ws_n, n, fake, n + 1, *args) == -1          # n_act > n
    assert L.nbd_tree_accel_active_f32(fake, ws_n, n, None, 5, *args) == -1              # no list
    assert L.nbd_tree_accel_active_f32(fake, ws_n - 1, n, fake, 5, *args) == -1          # short workspace
    assert L.nbd_tree_accel_active_f32(fake, ws_n, n, fake, -1, *args) == -1
    assert L.nbd_tree_accel_active_f32(fake, ws_n, -1, fake, 0, *args) == -1
    assert L.nbd_tree_accel_active_f32(None, ws_n, n, fake, 5, *args) == -1
    assert L.nbd_tree_accel_active_f32(fake, ws_n, n, fake, 5, 0.5, 0.01, 1.0, 1, None, None, None) == -1
    assert L.nbd_tree_accel_active_f32(fake, ws_n, n, fake, 5, -0.5, 0.01, 1.0, 1, fake, None, None) == -1
    assert L.nbd_tree_accel_active_f32(fake, ws_n, (1 << 24) + 1, fake, 5, *args) == -3
    assert L.nbd_tree_accel_active_f32(None, 0, n, None, 0, 0.5, 0.01, 1.0, 1, None, None, None) == 0   # nothing listed
    act_n = L.nbd_tree_active_workspace_bytes(n)
    assert L.nbd_tree_select_active(None, n, fake, None, None, fake, act_n, None) == -1
    assert L.nbd_tree_select_active(fake, n, None, None, None, fake, act_n, None) == -1
    assert L.nbd_tree_select_active(fake, n, fake, None, None, None, act_n, None) == -1
    assert L.nbd_tree_select_active(fake, -1, fake, None, None, fake, act_n, None) == -1
    assert L.nbd_tree_select_active(fake, n, fake, None, None, fake, act_n - 1, None) == -2
    assert L.nbd_tree_select_active(fake, n, fake, None, None, ctypes.c_void_p(256 * 4096 + 16), act_n, None) == -1
    assert L.nbd_tree_select_active(fake, (1 << 24) + 1, fake, None, None, fake, act_n, None) == -3
    assert L.nbd_tree_select_active(None, 0, None, None, None, None, 0, None) == 0


def test_block_stage_refusals_launch_nothing():
    L = _lib.lib()
    f = ctypes.c_void_p(256 * 4096)
    assert L.nbd_tblock_init_levels(f, -1, 0.1, 0.02, 0.1, 4, f, f, f, None) == -1
    assert L.nbd_tblock_init_levels(f, 8, 0.1, 0.02, 0.1, 21, f, f, f, None) == -1
    assert L.nbd_tblock_init_levels(f, 8, 0.0, 0.02, 0.1, 4, f, f, f, None) == -1
    assert L.nbd_tblock_init_levels(f, 8, 0.1, 0.0, 0.1, 4, f, f, f, None) == -1
    assert L.nbd_tblock_init_levels(f, 8, 0.1, 0.02, 0.0, 4, f, f, f, None) == -1
    assert L.nbd_tblock_init_levels(f, 8, 0.1, 0.02, 0.1, 4, f, None, f, None) == -1
    assert L.nbd_tblock_init_levels(f, 8, 0.1, 0.02, 0.1, 4, f, f, None, None) == -1
    assert L.nbd_tblock_open(f, f, f, f, f, 0, 4, 0.1, f, None) == -1
    assert L.nbd_tblock_open(f, None, f, f, f, 8, 4, 0.1, f, None) == -1
    assert L.nbd_tblock_open(f, f, f, f, None, 8, 4, 0.1, f, None) == -1
    assert L.nbd_tblock_open(f, f, f, f, f, 8, -1, 0.1, f, None) == -1
    assert L.nbd_tblock_drift(f, f, f, f, f, f, 8, 4, 0.1, f, None, None) == -1
    assert L.nbd_tblock_drift(f, f, f, f, f, None, 8, 4, 0.1, f, f, None) == -1
    assert L.nbd_tblock_drift(f, f, f, f, f, f, 8, 4, 0.1, f, ctypes.c_void_p(256 * 4096 + 4), None) == -1
    assert L.nbd_tblock_drift(f, f, f, f, f, f, 8, 4, float("nan"), f, f, None) == -1
    assert L.nbd_tblock_flag(f, f, 8, 4, f, None, None) == -1
    assert L.nbd_tblock_flag(f, f, 0, 4, f, f, None) == -1
    assert L.nbd_tblock_close(f, f, None, f, f, 8, 4, 0.1, 0.02, 0.1, f, None) == -1
    assert L.nbd_tblock_close(f, f, f, f, f, 8, 4, 0.1, -0.02, 0.1, f, None) == -1
    assert L.nbd_tblock_close(f, f, f, f, f, 8, 4, 0.1, 0.02, 0.0, f, None) == -1


# ---------------------------------------------------------------- the simulator's refusals (before a device is resolved)

def _kw(**over):
    p, v, m = to.case("B")
    kw = dict(positions=p, velocities=v, masses=m, softening=to.SOFTENING, dt=0.01, device="cuda", calc_energy=False)
    kw.update(over)
    return kw


@pytest.mark.parametrize("over, word", [
    (dict(max_level=-1), "max_level"), (dict(max_level=21), "max_level"), (dict(max_level=2.0), "max_level"),
    (dict(max_level=True), "max_level"), (dict(eta=0.0), "eta"), (dict(eta=-1.0), "eta"), (dict(dt=0.0), "dt"),
    (dict(dt=-0.01), "dt"), (dict(softening=0.0), "softening"), (dict(softening=-0.1), "softening"),
    (dict(process_group=object()), "process_group"), (dict(dtype=torch.float64), "float32"),
    (dict(theta=-0.5), "theta"), (dict(potential="mesh"), "potential")])
def test_refusals_come_before_a_device_is_resolved(over, word, monkeypatch):
    from galaxify import simulation

    def no_device(*a, **k):
        raise AssertionError("a device was resolved before the refusal")
    monkeypatch.setattr(simulation, "_resolve_device", no_device)
    with pytest.raises(ValueError, match=word):
        simulation.BlockTreeLeapFrogSimulator(**_kw(**over))


def test_inputs_that_require_grad_are_refused(monkeypatch):
    from galaxify import simulation
    monkeypatch.setattr(simulation, "_resolve_device", lambda *a, **k: pytest.fail("a device was resolved"))
    p, v, m = to.case("B")
    with pytest.raises(ValueError, match="requires grad"):
        simulation.BlockTreeLeapFrogSimulator(**_kw(positions=torch.tensor(p, requires_grad=True)))


def test_defaults_and_surface():
    import inspect
    from galaxify import simulation
    cls = simulation.BlockTreeLeapFrogSimulator
    sig = inspect.signature(cls.__init__)
    assert sig.parameters["eta"].default == 0.025 and sig.parameters["max_level"].default == 10
    assert issubclass(cls, simulation.TreeLeapFrogSimulator) and cls.MAX_LEVEL_LIMIT == 20
    assert not cls._capturable()
