"""BatchedSimulator(integrator="block_hermite" / "block_hermite6") without a GPU: the refusals that come before any device
is resolved, the host-only plan and workspace entries of csrc/direct_batch_hermite_block_f64.hip against a Python
restatement of the float64 launch plan, and the argument the implementation rests on, on the CPU oracles alone: the
sorted union of independent scenes' block schedules is itself a block schedule, and the pooled scheduler gives every
scene exactly its own active set at every tick of the union."""
import ctypes

import numpy as np
import pytest
import torch

import batch_block_cases as cases

Z = np.zeros((4, 3))
SYSTEMS = [(Z, Z, np.ones(4))]


def _build(**kw):
    from galaxify import simulation
    return simulation.BatchedSimulator(systems=SYSTEMS, device="no-such-device", **kw)


@pytest.mark.parametrize("integrator", cases.INTEGRATOR.values())
def test_float32_is_refused_before_a_device_is_resolved(integrator):
    with pytest.raises(ValueError, match="float64 only"):
        _build(integrator=integrator, dtype=torch.float32)
    with pytest.raises(ValueError, match="dtype must be"):
        _build(integrator=integrator, dtype=torch.float16)


@pytest.mark.parametrize("integrator", ["leapfrog", "euler", "hermite", "hermite6"])
@pytest.mark.parametrize("kw", [dict(eta=0.02), dict(max_level=4), dict(eta=0.02, max_level=4)])
def test_eta_and_max_level_belong_to_the_block_integrators(integrator, kw):
    with pytest.raises(ValueError, match="eta and max_level"):
        _build(integrator=integrator, **kw)


@pytest.mark.parametrize("integrator", cases.INTEGRATOR.values())
def test_bad_keywords_and_levels_are_refused_first(integrator):
    with pytest.raises(TypeError, match="unexpected keyword argument 'etas'"):
        _build(integrator=integrator, etas=0.1)
    for bad in (-1, 21, 2.0):
        with pytest.raises(ValueError, match="max_level"):
            _build(integrator=integrator, max_level=bad)
    with pytest.raises(ValueError, match="integrator must be"):
        _build(integrator="block_hermite8")


# ------------------------------------------------------------------ the host plan entries
PLAN_SIZES = [1, 2, 64, 65, 130, 520, 4608, 0]


def test_the_python_restatement_knows_the_issue_figures():
    """4608 bodies: 72 chunks, 18 slabs up to 56 target groups and 15 with all 72."""
    assert {cases.slabs_f64(g, 72) for g in range(1, 57)} == {18} and cases.slabs_f64(72, 72) == 15
    assert cases.slabs_f64(1, 1) == 1 and cases.slabs_f64(9, 9) == 2


@pytest.mark.parametrize("order", cases.ORDERS)
def test_plan_items_and_workspace(order):
    from nbd import direct
    plan = direct.BatchBlockPlan(PLAN_SIZES, None, order=order)
    assert plan.n_items == sum(cases.scene_items(n) for n in PLAN_SIZES)
    assert plan.posm_rows == sum(-(-n // 64) * 64 for n in PLAN_SIZES)
    sums = sum(cases.scene_sum_rows(n) for n in PLAN_SIZES) * cases.K_OUT[order] * 8
    lists = -(-sum(PLAN_SIZES) // 8) * 8 * 4
    assert plan.workspace_bytes >= lists + sums
    for n in PLAN_SIZES:                                     # scene by scene: the list never falls short of a block step
        one = direct.BatchBlockPlan([n], None, order=order)
        assert one.n_items == cases.scene_items(n)
        assert one.workspace_bytes >= -(-n // 8) * 32 + cases.scene_sum_rows(n) * cases.K_OUT[order] * 8
        chunks = -(-n // 64)
        for n_act in range(1, n + 1, 7):
            g = -(-n_act // 64)
            assert g * cases.slabs_f64(g, chunks) <= one.n_items
    # the work list: every scene's items numbered from 0, each once
    items = plan.host[: 4 * plan.n_items].reshape(-1, 4)
    for s, n in enumerate(PLAN_SIZES):
        assert sorted(items[items[:, 0] == s][:, 1].tolist()) == list(range(cases.scene_items(n)))


def test_malformed_offsets_are_refused():
    from nbd import _lib, direct
    L = _lib.lib()
    items, rows, nb = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()

    def plan(offsets):
        arr = np.asarray(offsets, np.int32)
        return [L.nbd_batch_hblock_f64_plan(arr.ctypes.data, len(offsets) - 1, items, rows, nb),
                L.nbd_batch_hblock_f64_workspace_bytes(arr.ctypes.data, len(offsets) - 1, nb),
                L.nbd_batch_hblock6_f64_workspace_bytes(arr.ctypes.data, len(offsets) - 1, nb)]

    assert plan([0, 3, 10]) == [0, 0, 0]
    assert plan([1, 3, 10]) == [-1] * 3                      # does not start at 0
    assert plan([0, 5, 3]) == [-1] * 3                       # decreasing
    assert plan([0]) == [-1] * 3                             # no scene
    assert L.nbd_batch_hblock_f64_plan(None, 2, items, rows, nb) == -1
    good = np.asarray([0, 3, 10], np.int32)
    buf = np.zeros(1 << 12, np.int32)
    assert L.nbd_batch_hblock_f64_plan(good.ctypes.data, 2, items, rows, nb) == 0
    assert L.nbd_batch_hblock_f64_plan_fill(good.ctypes.data, 2, buf.ctypes.data, nb.value - 4) == -1
    assert L.nbd_batch_hblock6_f64_plan_fill(good.ctypes.data, 2, None, nb.value) == -1
    assert L.nbd_batch_hblock_f64_plan_fill(good.ctypes.data, 2, buf.ctypes.data, nb.value) == 0
    with pytest.raises(_lib.NbdError):
        direct.BatchBlockPlan([3, -1], None)
    with pytest.raises(_lib.NbdError):
        direct.BatchBlockPlan([3], None, order=5)
    # the launching entries refuse before any launch: a bad level, a missing plan
    assert L.nbd_batch_hblock_schedule(good.ctypes.data, 2, None, nb.value, None, 4, None, None, None, 0, None, None) == -1
    assert L.nbd_batch_hblock_step_f64(good.ctypes.data, 2, buf.ctypes.data, nb.value, *[None] * 8, 21, *[None] * 4, 0,
                                       None) == -1


# ------------------------------------------------------------------ one schedule serves all scenes
@pytest.mark.parametrize("order", cases.ORDERS)
def test_the_union_of_the_scenes_schedules_is_a_block_schedule(order):
    K = cases.bc.K
    end = 1 << K
    scenes = cases.oracle_scenes(order)
    assert len(scenes) == 3 and [len(s[0]) for s in scenes] == [2, 256, 256]
    own_ticks = [[t for t, _, _ in steps] for _, steps in scenes]
    for ticks in own_ticks:
        assert ticks == sorted(set(ticks)) and ticks[-1] == end
    union = sorted(set().union(*own_ticks))
    assert len({tuple(t) for t in own_ticks}) == 3 and min(map(len, own_ticks)) < len(union)    # three schedules, and a
    #                                                          scene that sits out some of the union's ticks
    levels = [np.asarray(initial) for initial, _ in scenes]
    at = [0] * len(scenes)
    T, taken = 0, []
    while True:
        t_next, active = cases.next_tick(np.concatenate(levels), T, K)
        taken.append(t_next)
        lo = 0
        for s, (_, steps) in enumerate(scenes):
            mine = active[lo:lo + len(levels[s])]
            lo += len(levels[s])
            if at[s] < len(steps) and steps[at[s]][0] == t_next:
                assert np.array_equal(mine, steps[at[s]][1]), (s, t_next)      # exactly its own active set
                d = 1 << (K - levels[s][mine])
                assert np.all(t_next % d == 0)
                levels[s] = np.asarray(steps[at[s]][2])
                at[s] += 1
            else:
                assert not mine.any(), (s, t_next)                               # not its tick: nothing of it is due
        if t_next == end:
            break
        T = t_next
    assert taken == union and at == [len(steps) for _, steps in scenes]
    assert all(a < b for a, b in zip(taken, taken[1:]))
