"""What the host and the GPU tests of BatchedSimulator(integrator="block_hermite" / "block_hermite6") share: the Python
restatement of the float64 launch plan (slabs_f64 of csrc/hermite_f64_kernels.h), the block scheduler as integers (the
next tick and the active set of a pool of levels), the scenes of the standard ensemble and the three oracle scenes of
the union-schedule test. Every fixture is computed once per process and never written to."""
import functools

import numpy as np

import block_hermite6_cases as c6
import block_hermite6_oracle as b6
import block_hermite_f64_cases as bc
import block_hermite_oracle as bo
import hermite_f64_oracle as fo

K_TARGET_WGS, K_WAVES, K_MAX_SLABS = 1024, 4, 64
ORDERS = (4, 6)
INTEGRATOR = {4: "block_hermite", 6: "block_hermite6"}
SHARED = {4: "hermite", 6: "hermite6"}
LONE = {4: "BlockHermiteSimulator", 6: "BlockHermite6Simulator"}
K_OUT = {4: 6, 6: 9}
STATE = {4: ("positions", "velocities", "accelerations", "jerks"),
         6: ("positions", "velocities", "accelerations", "jerks", "snaps", "crackles")}

SIZES = [0, 1, 2, 3, 63, 64, 65, 130, 520]
K = 4


def slabs_f64(groups, n_chunks):
    slabs = -(-K_TARGET_WGS // groups)
    slabs = min(slabs, n_chunks // K_WAVES, K_MAX_SLABS)
    return max(slabs, 1)


def scene_items(n):
    """max over g in [1, ceil(n / 64)] of g * slabs_f64(g, chunks): the scene's share of the static work list."""
    chunks = -(-n // 64)
    return max((g * slabs_f64(g, chunks) for g in range(1, chunks + 1)), default=0)


def scene_sum_rows(n):
    """The largest slabs * n_act over every active count of n bodies."""
    chunks = -(-n // 64)
    return max((slabs_f64(-(-a // 64), chunks) * a for a in range(1, n + 1)), default=0)


def next_tick(levels, T, K):
    """(t_next, active mask) of a pool of bodies at `levels` that has reached tick T: the first multiple after T of any
    step present, and the bodies whose step divides it."""
    d = 1 << (K - np.asarray(levels, np.int64))
    t_next = int(((T // d + 1) * d).min())
    return t_next, t_next % d == 0


def ticks_of(initial_levels, history, K):
    """The ticks of one scene's block steps, from its levels before the first one and after every one."""
    ticks, T, levels = [], 0, np.asarray(initial_levels)
    for after in history:
        t, _ = next_tick(levels, T, K)
        ticks.append(t)
        T = 0 if t == 1 << K else t
        levels = np.asarray(after)
    return ticks


@functools.lru_cache(maxsize=None)
def scene(n, g=1.0, eps=0.05, dt=0.01, eta=0.02, seed=None):
    """A perturbed Plummer sphere of n bodies (0: empty) with its parameters, as a dict."""
    if n == 0:
        x, v, m = np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0)
    else:
        x, v, m = fo.plummer_case(n, seed=(700 + n) if seed is None else seed)
    return frozen(x, v, m, g, eps, dt, eta)


def frozen(x, v, m, g, eps, dt, eta):
    for arr in (x, v, m):
        arr.setflags(write=False)
    return dict(pos=x, vel=v, mass=m, g=g, eps=eps, dt=dt, eta=eta)


def ensemble():
    """The standard ensemble: dt, softening and eta different per scene; n = 65 at softening 0 beside softened ones."""
    sc = [scene(n, eps=0.0 if n == 65 else 0.02 + 0.004 * k, dt=0.02 + 0.003 * k, eta=0.01 + 0.002 * k)
          for k, n in enumerate(SIZES)]
    assert [s["eps"] for s in sc].count(0.0) == 1
    return sc


@functools.lru_cache(maxsize=None)
def big_scene():
    """A Plummer sphere of 4608 bodies (72 chunks) with two planted close pairs: a few bodies far deeper than the rest."""
    x, v, m = (a.copy() for a in fo.plummer_case(4608, seed=4608))
    for a, b, sep in ((0, 1, 2e-3), (2, 3, 3e-3)):
        x[b] = x[a] + np.array([sep, 0.37 * sep, -0.21 * sep])
        v[b] = v[a] + np.array([0.0, 0.5, 0.1])
    return frozen(x, v, m, 1.0, 1e-3, 1.0 / 64, 0.02)


@functools.lru_cache(maxsize=None)
def oracle_scenes(order):
    """Three oracle runs on one tick grid (K = bc.K): the e = 0.9 two-body orbit and the two planted-binary spheres, one
    output step each. -> [(initial levels, [(tick, active mask, levels after)])]."""
    Kk = bc.K
    x0, v0, m0, dt0 = bc.orbit()
    run = bo.block_run if order == 4 else b6.block6_run
    planted = bc.planted if order == 4 else c6.planted
    cases = [(x0, v0, m0, dt0, 0.0, 0.01)] + [planted(eps) + (bc.DT, eps, bc.ETA) for eps in (0.0, 0.01)]
    out = []
    for x, v, m, dt, eps, eta in cases:
        r = run(x, v, m, dt, 1.0, eps * eps, 1, eta=eta, max_level=Kk)
        a, j = fo.accel_jerk(x, v, m, 1.0, eps * eps)
        na, nj = np.linalg.norm(a, axis=1), np.linalg.norm(j, axis=1)
        crit = np.where(nj == 0, np.inf, 0.5 * eta * na / np.where(nj == 0, 1.0, nj))
        initial = np.minimum([bo.wanted_level(c, dt, Kk) for c in crit], Kk)
        steps = []
        for ticks, levels in zip(r["tick_history"], r["history"]):
            t = int(ticks.max())
            steps.append((t if t else 1 << Kk, ticks == t, levels))
        out.append((initial, steps))
    return out
