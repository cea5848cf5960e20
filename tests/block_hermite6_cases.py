"""What the host and the GPU tests of BlockHermite6Simulator share: the planted-binary fixtures of
block_hermite_f64_cases (same seeds, DT, ETA, K and permutations), their runs through the 6th-order block oracle -- as
they are and under the three fixed permutations of the bodies -- and the eccentric orbit at the 6th order. Every oracle
run is computed once per process and never written to."""
import functools

import numpy as np

import block_hermite6_oracle as b6
import block_hermite_f64_cases as bc
import block_hermite_oracle as bo
import hermite_f64_oracle as fo
import hermite_oracle as ho

DT, ETA, K, PERM_SEEDS = bc.DT, bc.ETA, bc.K, bc.PERM_SEEDS
# seeds of the planted-binary sphere. eps = 0: block_hermite_f64_cases's. eps = 0.01: that one (38) has a criterion value
# of the 6th-order scheme 6.8e-4 from a level boundary that a permutation of the bodies moves by 7.9e-7, 858 times less
# where the fixture condition asks for 1000 (test_block_hermite6_host.py); of the seeds 0..47, searched on the CPU, 14
# keeps the widest margins (7.8e-4 over one output step, 3.1e-4 over four; shifts 1.1e-9 and 2.7e-8).
PLANTED = {0.0: bc.PLANTED[0.0], 0.01: 14}

ORBIT_K = bc.ORBIT_K
ORBIT_ETAS = (0.01, 0.0025)
PER_BODY = ("x", "v", "a", "j", "s", "c", "levels")


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
    return bc._freeze(b6.block6_run(x, v, m, DT, 1.0, eps * eps, steps, eta=ETA, max_level=K))


@functools.lru_cache(maxsize=None)
def planted_run_permuted(eps, steps, seed):
    """The same run with the bodies permuted on the way in and every per-body result put back in body order."""
    x, v, m = planted(eps)
    perm = np.random.default_rng(seed).permutation(x.shape[0])
    back = np.empty_like(perm)
    back[perm] = np.arange(perm.size)
    r = b6.block6_run(x[perm], v[perm], m[perm], DT, 1.0, eps * eps, steps, eta=ETA, max_level=K)
    for key in PER_BODY:
        r[key] = r[key][back]
    r["history"] = [h[back] for h in r["history"]]
    return bc._freeze(r)


def permutation_spread(eps, steps):
    """{key: s_k}: the largest difference of x / v / a / j / s / c between the oracle run and the three permuted ones."""
    ref = planted_run(eps, steps)
    return {key: max(np.abs(planted_run_permuted(eps, steps, sd)[key] - ref[key]).max() for sd in PERM_SEEDS)
            for key in PER_BODY[:-1]}


@functools.lru_cache(maxsize=None)
def orbit_run(eta, max_level=ORBIT_K):
    """The e = 0.9 orbit of block_hermite_f64_cases.orbit() at the 6th order: block6_run's dict plus `err`."""
    x0, v0, m, dt = bc.orbit()
    r = b6.block6_run(x0, v0, m, dt, 1.0, 0.0, 4, eta=eta, max_level=max_level)
    r["err"] = ho.orbit_error(r["x"], x0)
    return bc._freeze(r)
