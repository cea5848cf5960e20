"""fp64 numpy restatement of the 4th-order Hermite integrator (Makino & Aarseth 1992) that HermiteSimulator runs in fp32
(csrc/direct_hermite.hip), plus the leapfrog restatement and the two-body orbit the convergence tests use.

    a_i = G sum_{j!=i} m_j r_ij s^3
    j_i = G sum_{j!=i} m_j (v_ij s^3 - 3 (r_ij.v_ij) s^5 r_ij),   r_ij = x_j - x_i, v_ij = v_j - v_i,
                                                                s = (|r_ij|^2 + eps^2)^(-1/2)
    predict:  x_p = x + v dt + a0 dt^2/2 + j0 dt^3/6,  v_p = v + a0 dt + j0 dt^2/2
    correct:  v1 = v + (a0 + a1) dt/2 + (j0 - j1) dt^2/12,  x1 = x + (v + v1) dt/2 + (a0 - a1) dt^2/12
The i == j term is excluded by index (fill_diagonal_), whatever the softening."""
import numpy as np

_ROWS = 512


def accel_jerk(x, v, m, g, eps2):
    x = np.asarray(x, np.float64); v = np.asarray(v, np.float64); m = np.asarray(m, np.float64)
    n = x.shape[0]
    a = np.zeros((n, 3)); j = np.zeros((n, 3))
    for lo in range(0, n, _ROWS):
        hi = min(n, lo + _ROWS)
        d = x[None, :, :] - x[lo:hi, None, :]
        dv = v[None, :, :] - v[lo:hi, None, :]
        r2 = (d * d).sum(-1) + eps2
        idx = np.arange(lo, hi)
        r2[idx - lo, idx] = 1.0                      # any finite value: the term is zeroed below
        s = 1.0 / np.sqrt(r2)
        s[idx - lo, idx] = 0.0
        w = m[None, :] * s ** 3
        rv = (d * dv).sum(-1)
        a[lo:hi] = (w[..., None] * d).sum(1)
        j[lo:hi] = (w[..., None] * dv - 3.0 * (rv * s * s * w)[..., None] * d).sum(1)
    return g * a, g * j


def hermite_step(x, v, a0, j0, m, dt, g, eps2):
    xp = x + v * dt + a0 * (dt * dt / 2) + j0 * (dt ** 3 / 6)
    vp = v + a0 * dt + j0 * (dt * dt / 2)
    a1, j1 = accel_jerk(xp, vp, m, g, eps2)
    v1 = v + (a0 + a1) * (dt / 2) + (j0 - j1) * (dt * dt / 12)
    x1 = x + (v + v1) * (dt / 2) + (a0 - a1) * (dt * dt / 12)
    return x1, v1, a1, j1


def hermite_run(x, v, m, dt, g, eps2, steps):
    """State after `steps` steps from (x, v): (x, v, a, j)."""
    x = np.array(x, np.float64); v = np.array(v, np.float64)
    a, j = accel_jerk(x, v, m, g, eps2)
    for _ in range(steps):
        x, v, a, j = hermite_step(x, v, a, j, m, dt, g, eps2)
    return x, v, a, j


def leapfrog_run(x, v, m, dt, g, eps2, steps):
    x = np.array(x, np.float64); v = np.array(v, np.float64)
    a, _ = accel_jerk(x, v, m, g, eps2)
    for _ in range(steps):
        v = v + 0.5 * dt * a
        x = x + dt * v
        a, _ = accel_jerk(x, v, m, g, eps2)
        v = v + 0.5 * dt * a
    return x, v


def two_body(e=0.5):
    """Equal masses 1/2, G = 1, semi-major axis 1 (period 2 pi), started at apocentre, centre of mass at rest at the
    origin: (x, v, m, period)."""
    r = 1.0 + e
    vrel = np.sqrt((1.0 - e) / (1.0 + e))
    x = np.array([[-r / 2, 0.0, 0.0], [r / 2, 0.0, 0.0]])
    v = np.array([[0.0, -vrel / 2, 0.0], [0.0, vrel / 2, 0.0]])
    return x, v, np.array([0.5, 0.5]), 2.0 * np.pi


def orbit_error(x, x0):
    """Largest position error of a body after whole periods, relative to the semi-major axis (1)."""
    return float(np.linalg.norm(np.asarray(x, np.float64) - x0, axis=1).max())
