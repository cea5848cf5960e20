"""What the host and the GPU tests of BlockHermiteSimulator(dtype=torch.float64) share: the two planted-binary fixtures
(no input fp32-representable), their fp64 block-oracle runs -- as they are and under three fixed permutations of the
bodies -- and the eccentric orbit. Every oracle run is computed once per process and never written to."""
import functools

import numpy as np

import block_hermite_oracle as bo
import hermite_f64_oracle as fo
import hermite_oracle as ho

# seeds of the planted-binary sphere whose criterion values keep clear of every level boundary (test_block_hermite_gpu.py
# found them for one output step; test_block_hermite_f64_host.py pins the margins of the perturbed fixtures)
PLANTED = {0.0: 93, 0.01: 38}
DT, ETA, K = 1.0 / 32, 0.02, 10
PERM_SEEDS = (21, 22, 23)

ORBIT_ETA, ORBIT_K = 0.000625, 16


def _freeze(run):
    for v in run.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return run


@functools.lru_cache(maxsize=None)
def planted(eps):
    """(x, v, m) of the fixture at softening eps: the planted-binary sphere with 1e-9 of noise on every input."""
    x, v, m = fo.perturbed(*bo.planted_binary_sphere(256, PLANTED[eps]), 7)
    for a in (x, v, m):
        a.setflags(write=False)
    return x, v, m


@functools.lru_cache(maxsize=None)
def planted_run(eps, steps):
    x, v, m = planted(eps)
    return _freeze(bo.block_run(x, v, m, DT, 1.0, eps * eps, steps, eta=ETA, max_level=K))


@functools.lru_cache(maxsize=None)
def planted_run_permuted(eps, steps, seed):
    """The same run with the bodies permuted on the way in and every per-body result put back in body order."""
    x, v, m = planted(eps)
    perm = np.random.default_rng(seed).permutation(x.shape[0])
    back = np.empty_like(perm)
    back[perm] = np.arange(perm.size)
    r = bo.block_run(x[perm], v[perm], m[perm], DT, 1.0, eps * eps, steps, eta=ETA, max_level=K)
    for key in ("x", "v", "a", "j", "levels"):
        r[key] = r[key][back]
    r["history"] = [h[back] for h in r["history"]]
    return _freeze(r)


def permutation_spread(eps, steps):
    """{name: s_k}: the largest difference of pos / vel / acc / jerk between the oracle run and the three permuted ones."""
    ref = planted_run(eps, steps)
    return {name: max(np.abs(planted_run_permuted(eps, steps, s)[key] - ref[key]).max() for s in PERM_SEEDS)
            for name, key in (("pos", "x"), ("vel", "v"), ("acc", "a"), ("jerk", "j"))}


def orbit():
    """The e = 0.9 orbit (eps = 0), one period as 4 output steps: (x0, v0, m, dt). Its coordinates (0.95) and velocities
    are not fp32-representable; its zeros and the masses 1/2 are exact in any format."""
    x0, v0, m, period = ho.two_body(0.9)
    assert not np.any(x0[:, 0].astype(np.float32) == x0[:, 0]) and not np.any(v0[:, 1].astype(np.float32) == v0[:, 1])
    return x0, v0, m, period / 4


@functools.lru_cache(maxsize=None)
def orbit_run(eta=ORBIT_ETA, max_level=ORBIT_K):
    x0, v0, m, dt = orbit()
    r = bo.block_run(x0, v0, m, dt, 1.0, 0.0, 4, eta=eta, max_level=max_level)
    r["err"] = ho.orbit_error(r["x"], x0)
    return _freeze(r)
