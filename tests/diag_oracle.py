"""fp64 numpy restatement of the consistent-potential diagnostics (csrc/direct_diag.hip), from the fp32 state promoted to
fp64:

    phi_i = -G sum_{j != i} m_j (|r_j - r_i|^2 + eps^2)^(-1/2)          (i == j excluded by index)
    row   = {M, C (3), P (3), L (3), K, U, E, Q, 0, 0},  C = sum m x / M, P = sum m v, L = sum m x cross v,
            K = sum 1/2 m |v|^2, U = 1/2 sum m phi, E = K + U, Q = -2 K / U  (C = 0 when M = 0, Q = 0 when U = 0)

`reference_energies` is the reference's own convention, U = sum_{i<j} -G m_i m_j / (|r| + eps): at eps = 0 the two agree."""
import numpy as np

_ROWS = 512


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def potentials(x, m, g, eps2):
    x, m = _f64(x), _f64(m)
    n = x.shape[0]
    phi = np.zeros(n)
    for lo in range(0, n, _ROWS):
        hi = min(n, lo + _ROWS)
        d = x[None, :, :] - x[lo:hi, None, :]
        r2 = (d * d).sum(-1) + eps2
        idx = np.arange(lo, hi)
        r2[idx - lo, idx] = 1.0                      # any finite value: the term is zeroed below
        s = 1.0 / np.sqrt(r2)
        s[idx - lo, idx] = 0.0
        phi[lo:hi] = (m[None, :] * s).sum(1)
    return -g * phi


def sums(x, v, m, phi):
    """(the 12 sums M, m x, m v, m x cross v, K, sum m phi; the sum of |terms| of each): the second bounds how far two
    fp64 summation orders of the first can differ."""
    x, v, m = _f64(x), _f64(v), _f64(m)
    cross = np.cross(x, v) if x.shape[0] else np.zeros((0, 3))
    terms = np.concatenate([m[:, None], m[:, None] * x, m[:, None] * v, m[:, None] * cross,
                            (0.5 * m * (v * v).sum(1))[:, None], (m * np.asarray(phi, np.float64))[:, None]], axis=1)
    return terms.sum(0), np.abs(terms).sum(0)


def invariants_row(x, v, m, phi):
    s, _ = sums(x, v, m, phi)
    M, K, U = s[0], s[10], 0.5 * s[11]
    row = np.zeros(16)
    row[0] = M
    row[1:4] = s[1:4] / M if M != 0 else 0.0
    row[4:10] = s[4:10]
    row[10], row[11], row[12] = K, U, K + U
    row[13] = -2.0 * K / U if U != 0 else 0.0
    return row


def reference_energies(x, v, m, g, eps):
    """(U, K) of the reference's compute_energies: U = sum_{i<j} -G m_i m_j / (|r_ij| + eps)."""
    x, v, m = _f64(x), _f64(v), _f64(m)
    n = x.shape[0]
    u = 0.0
    for lo in range(0, n, _ROWS):
        hi = min(n, lo + _ROWS)
        d = np.sqrt(((x[None, :, :] - x[lo:hi, None, :]) ** 2).sum(-1)) + eps
        with np.errstate(divide="ignore", invalid="ignore"):     # the diagonal at eps = 0: dropped by triu below
            w = m[lo:hi, None] * m[None, :] / d
        u += np.triu(w, k=lo + 1).sum()
    return -g * u, float((0.5 * m * (v * v).sum(1)).sum())
