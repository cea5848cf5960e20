"""What the float64 tests of HermiteSimulator(dtype=torch.float64) (csrc/direct_hermite_f64.hip) share: inputs that are
not fp32-representable, the fp64 numpy oracles with the sum of |terms| of every sum they form, and the accuracy bar.

The force, the steps and the orbit come from hermite_oracle (generic fp64). diag_oracle rounds its inputs to fp32 first
(it checks the fp32 diagnostics), so the potential, the 12 sums of the invariants row and the reference-convention
energies are restated here on the fp64 inputs as they are; the host test pins them to diag_oracle on fp32 inputs.

The bar, for a result that is a sum of T terms:   |got - ref| <= (T + 32) 2^-53 sum|terms|,  componentwise:
the worst-case bound of an fp64 sum in any order, plus a few ulp per term. Any fp32 intermediate misses it by ~10^6.
T and the terms of each sum:
  acceleration  n terms per component, w d_k                                   (w = G m_j s^3)
  jerk          4 n: w dv_k and the three products of -3 s^2 w d_k (d.dv) -- the scalar product may cancel, so its
                products are the terms, not their sum
  phi           n terms G m_j s;   the invariants' sums: n terms each;   U of compute_energies(): n (n - 1) / 2 pair terms
"""
import numpy as np

import hermite_oracle as ho

U53 = 2.0 ** -53
_ROWS = 512


def bar(t_terms, sum_abs):
    return (t_terms + 32) * U53 * np.asarray(sum_abs, np.float64)


def within(got, ref, t_terms, sum_abs):
    """(ok, the largest |got - ref| / bar over the components whose bar is not 0; those must match exactly)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    b = np.broadcast_to(bar(t_terms, sum_abs), ref.shape)
    err = np.abs(got - ref)
    ok = bool(np.all(err <= b))
    pos = b > 0
    return ok, float((err[pos] / b[pos]).max()) if pos.any() else 0.0


def perturbed(x, v, m, seed):
    """The case in fp64 with uniform(-1, 1) * 1e-9 added to every coordinate, velocity and mass: nothing is
    fp32-representable any more, so a kernel that rounded its inputs to fp32 misses the bar. A massless body stays
    massless (0 is what makes it the case it is, and rounding would not change it)."""
    rng = np.random.default_rng(seed)
    x = np.asarray(x, np.float64) + rng.uniform(-1, 1, np.shape(x)) * 1e-9
    v = np.asarray(v, np.float64) + rng.uniform(-1, 1, np.shape(v)) * 1e-9
    m = np.asarray(m, np.float64)
    m = np.where(m == 0, 0.0, m + rng.uniform(-1, 1, m.shape) * 1e-9)
    for a in (x, v, m[m != 0]):
        assert not np.any(a.astype(np.float32).astype(np.float64) == a)
    return x, v, m


def plummer_case(n, seed):
    from nbd.plummer import generate_plummer
    p, v, m = generate_plummer(n, seed=seed)
    return perturbed(np.asarray(p), np.asarray(v), np.asarray(m), seed + 1)


def accel_jerk(x, v, m, g, eps2, order=None):
    """hermite_oracle.accel_jerk with the sources summed in the order `order` (a permutation of the bodies; None: as
    they are): the bodies are permuted on the way in and the rows put back on the way out."""
    if order is None:
        return ho.accel_jerk(x, v, m, g, eps2)
    order = np.asarray(order)
    a, j = ho.accel_jerk(x[order], v[order], m[order], g, eps2)
    back = np.empty_like(order)
    back[order] = np.arange(order.size)
    return a[back], j[back]


def accel_jerk_abs(x, v, m, g, eps2):
    """sum|terms| of every component of the acceleration and of the jerk, (n,3) each (see the module text)."""
    x = np.asarray(x, np.float64); v = np.asarray(v, np.float64); m = np.abs(np.asarray(m, np.float64))
    n = x.shape[0]
    sa = np.zeros((n, 3)); sj = np.zeros((n, 3))
    for lo in range(0, n, _ROWS):
        hi = min(n, lo + _ROWS)
        d = np.abs(x[None, :, :] - x[lo:hi, None, :])
        dv = np.abs(v[None, :, :] - v[lo:hi, None, :])
        r2 = (d * d).sum(-1) + eps2
        idx = np.arange(lo, hi)
        r2[idx - lo, idx] = 1.0
        s = 1.0 / np.sqrt(r2)
        s[idx - lo, idx] = 0.0
        w = m[None, :] * s ** 3
        sa[lo:hi] = (w[..., None] * d).sum(1)
        sj[lo:hi] = (w[..., None] * dv + 3.0 * ((d * dv).sum(-1) * s * s * w)[..., None] * d).sum(1)
    return abs(g) * sa, abs(g) * sj


def potentials(x, m, g, eps2, order=None):
    """(phi, sum|terms|): diag_oracle.potentials on the fp64 inputs as they are, sources in the order `order`."""
    x = np.asarray(x, np.float64); m = np.asarray(m, np.float64)
    n = x.shape[0]
    order = np.arange(n) if order is None else np.asarray(order)
    xs, ms = x[order], m[order]
    phi = np.zeros(n); sab = np.zeros(n)
    for lo in range(0, n, _ROWS):
        hi = min(n, lo + _ROWS)
        d = xs[None, :, :] - x[lo:hi, None, :]
        r2 = (d * d).sum(-1) + eps2
        own = order[None, :] == np.arange(lo, hi)[:, None]
        r2[own] = 1.0
        s = 1.0 / np.sqrt(r2)
        s[own] = 0.0
        phi[lo:hi] = (ms[None, :] * s).sum(1)
        sab[lo:hi] = (np.abs(ms)[None, :] * s).sum(1)
    return -g * phi, abs(g) * sab


def sums(x, v, m, phi):
    """diag_oracle.sums on the fp64 inputs as they are: (the 12 sums, the sum of |terms| of each)."""
    x = np.asarray(x, np.float64); v = np.asarray(v, np.float64); m = np.asarray(m, np.float64)
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
    """diag_oracle.reference_energies on the fp64 inputs as they are: (U, K, sum|terms| of U, sum|terms| of K)."""
    x = np.asarray(x, np.float64); v = np.asarray(v, np.float64); m = np.asarray(m, np.float64)
    n = x.shape[0]
    u = ua = 0.0
    for lo in range(0, n, _ROWS):
        hi = min(n, lo + _ROWS)
        d = np.sqrt(((x[None, :, :] - x[lo:hi, None, :]) ** 2).sum(-1)) + eps
        with np.errstate(divide="ignore", invalid="ignore"):     # the diagonal at eps = 0: dropped by triu below
            w = m[lo:hi, None] * m[None, :] / d
        u += np.triu(w, k=lo + 1).sum()
        ua += np.abs(np.triu(w, k=lo + 1)).sum()
    k = 0.5 * m * (v * v).sum(1)
    return -g * u, float(k.sum()), abs(g) * ua, float(np.abs(k).sum())


def energy(x, v, m, g, eps2):
    """E = K + 1/2 sum m phi of the Plummer potential, in fp64."""
    phi, _ = potentials(x, m, g, eps2)
    s, _ = sums(x, v, m, phi)
    return s[10] + 0.5 * s[11]
