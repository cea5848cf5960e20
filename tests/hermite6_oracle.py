"""fp64 numpy restatement of the 6th-order Hermite integrator (Nitadori & Makino 2008) that Hermite6Simulator runs in
float64 (csrc/direct_hermite_f64.hip), row-blocked like hermite_oracle.

Pair terms for target i and source j, with r = x_j - x_i, v = v_j - v_i, a = a_j - a_i, s = (|r|^2 + eps^2)^(-1/2):
    w = m_j s^3,  alpha = (r.v) s^2,  gamma = (v.v + r.a) s^2
    A_ij = w r,  J_ij = w v - 3 alpha w r,  S_ij = w a - 6 alpha w v + (15 alpha^2 - 3 gamma) w r
    a_i = G sum_j A_ij,  j_i = G sum_j J_ij,  s_i = G sum_j S_ij,  j != i (by index, whatever the softening)
One step in PEC form, with a0, j0, s0 and the crackle c0 = d^3 a / dt^3 carried:
    predict   x_p = x + v dt + a0 dt^2/2 + j0 dt^3/6 + s0 dt^4/24 + c0 dt^5/120
              v_p = v + a0 dt + j0 dt^2/2 + s0 dt^3/6 + c0 dt^4/24
              a_p = a0 + j0 dt + s0 dt^2/2 + c0 dt^3/6
    evaluate  a1, j1, s1 at (x_p, v_p, a_p)
    correct   v1 = v + (a0 + a1) dt/2 - (j1 - j0) dt^2/10 + (s0 + s1) dt^3/120
              x1 = x + (v + v1) dt/2 - (a1 - a0) dt^2/10 + (j0 + j1) dt^3/120
              c1 = [60 (a1 - a0) - dt (36 j1 + 24 j0) + dt^2 (9 s1 - 3 s0)] / dt^3
At the start: a from the acceleration + jerk evaluation, then s from the evaluation with that a, and c = 0.

The accuracy bar of the snap (hermite_f64_oracle.bar): T = 19 n terms per component, and sum|terms| per component k
    sum_j |w| [ |a_k| + 6 s^2 P |v_k| + (3 s^2 Q + 15 s^4 P^2) |r_k| ],  P = sum_l |r_l||v_l|,  Q = sum_l (v_l^2 + |r_l||a_l|):
the scalar products may cancel, so their products are the terms, not their sums."""
import numpy as np

_ROWS = 128


def _pairs(x, v, a, m, lo, hi, eps2):
    d = x[None, :, :] - x[lo:hi, None, :]
    dv = v[None, :, :] - v[lo:hi, None, :]
    da = a[None, :, :] - a[lo:hi, None, :]
    r2 = (d * d).sum(-1) + eps2
    idx = np.arange(lo, hi)
    r2[idx - lo, idx] = 1.0                      # any finite value: the term is zeroed below
    s = 1.0 / np.sqrt(r2)
    s[idx - lo, idx] = 0.0
    return d, dv, da, s, m[None, :] * s ** 3


def _evaluate(x, v, a, m, g, eps2, want_abs):
    """(a, j, s) and, with want_abs, sum|terms| of the snap (else None), from one pass over the pairs."""
    x = np.asarray(x, np.float64); v = np.asarray(v, np.float64); a = np.asarray(a, np.float64)
    m = np.asarray(m, np.float64)
    n = x.shape[0]
    acc = np.zeros((n, 3)); jerk = np.zeros((n, 3)); snap = np.zeros((n, 3))
    sab = np.zeros((n, 3)) if want_abs else None
    for lo in range(0, n, _ROWS):
        hi = min(n, lo + _ROWS)
        d, dv, da, s, w = _pairs(x, v, a, m, lo, hi, eps2)
        s2 = s * s
        rv = (d * dv).sum(-1)
        al = rv * s2
        alw = rv * s * s * w                     # hermite_oracle.accel_jerk's product, in its order: the same a and j
        gm = ((dv * dv).sum(-1) + (d * da).sum(-1)) * s2
        acc[lo:hi] = (w[..., None] * d).sum(1)
        jerk[lo:hi] = (w[..., None] * dv - 3.0 * alw[..., None] * d).sum(1)
        snap[lo:hi] = (w[..., None] * da - 6.0 * alw[..., None] * dv
                       + ((15.0 * al * al - 3.0 * gm) * w)[..., None] * d).sum(1)
        if want_abs:
            d, dv, da, w = np.abs(d), np.abs(dv), np.abs(da), np.abs(w)
            p = (d * dv).sum(-1)
            q = (dv * dv).sum(-1) + (d * da).sum(-1)
            sab[lo:hi] = (w[..., None] * (da + (6.0 * s2 * p)[..., None] * dv
                                          + (3.0 * s2 * q + 15.0 * s2 * s2 * p * p)[..., None] * d)).sum(1)
    return g * acc, g * jerk, g * snap, abs(g) * sab if want_abs else None


def accel_jerk_snap(x, v, a, m, g, eps2):
    """(a, j, s), each (n,3), of the state (x, v) with the accelerations `a` as the rows the snap differences."""
    return _evaluate(x, v, a, m, g, eps2, False)[:3]


def snap_abs(x, v, a, m, g, eps2):
    """sum|terms| of every component of the snap, (n,3) (see the module text)."""
    return _evaluate(x, v, a, m, g, eps2, True)[3]


def snap_and_abs(x, v, a, m, g, eps2):
    """(the snap, its sum|terms|) from one pass: accel_jerk_snap(...)[2] and snap_abs(...)."""
    return _evaluate(x, v, a, m, g, eps2, True)[2:]


def crackle(a0, j0, s0, a1, j1, s1, dt):
    """c1: the third derivative at t1 of the quintic through (a, j, s) at t0 and t1 = t0 + dt."""
    return (60.0 * (a1 - a0) - dt * (36.0 * j1 + 24.0 * j0) + dt * dt * (9.0 * s1 - 3.0 * s0)) / dt ** 3


def crackle_abs(a0, j0, s0, a1, j1, s1, dt):
    """sum|terms| of `crackle`, componentwise."""
    a0, j0, s0, a1, j1, s1 = (np.abs(t) for t in (a0, j0, s0, a1, j1, s1))
    return (60.0 * (a1 + a0) + dt * (36.0 * j1 + 24.0 * j0) + dt * dt * (9.0 * s1 + 3.0 * s0)) / dt ** 3


def start(x, v, m, g, eps2):
    """(a, j, s, c) at the start: two passes, c = 0."""
    a, _, _ = accel_jerk_snap(x, v, np.zeros_like(np.asarray(x, np.float64)), m, g, eps2)
    a, j, s = accel_jerk_snap(x, v, a, m, g, eps2)
    return a, j, s, np.zeros_like(a)


def hermite6_step(x, v, a0, j0, s0, c0, m, dt, g, eps2):
    xp = x + v * dt + a0 * (dt ** 2 / 2) + j0 * (dt ** 3 / 6) + s0 * (dt ** 4 / 24) + c0 * (dt ** 5 / 120)
    vp = v + a0 * dt + j0 * (dt ** 2 / 2) + s0 * (dt ** 3 / 6) + c0 * (dt ** 4 / 24)
    ap = a0 + j0 * dt + s0 * (dt ** 2 / 2) + c0 * (dt ** 3 / 6)
    a1, j1, s1 = accel_jerk_snap(xp, vp, ap, m, g, eps2)
    v1 = v + (a0 + a1) * (dt / 2) - (j1 - j0) * (dt ** 2 / 10) + (s0 + s1) * (dt ** 3 / 120)
    x1 = x + (v + v1) * (dt / 2) - (a1 - a0) * (dt ** 2 / 10) + (j0 + j1) * (dt ** 3 / 120)
    return x1, v1, a1, j1, s1, crackle(a0, j0, s0, a1, j1, s1, dt)


def hermite6_run(x, v, m, dt, g, eps2, steps):
    """State after `steps` steps from (x, v): (x, v, a, j, s, c)."""
    x = np.array(x, np.float64); v = np.array(v, np.float64); m = np.asarray(m, np.float64)
    a, j, s, c = start(x, v, m, g, eps2)
    for _ in range(steps):
        x, v, a, j, s, c = hermite6_step(x, v, a, j, s, c, m, dt, g, eps2)
    return x, v, a, j, s, c
