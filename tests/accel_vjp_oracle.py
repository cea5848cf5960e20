"""What the tests of the differentiable direct force (csrc/direct_grad.hip, nbd.autograd.direct_accel) share: the fp64
numpy closed form of the vector-Jacobian product of the all-pairs acceleration with the sum of |terms| of every component
it forms, a dense torch statement of the force for torch's own autograd, and the inputs.

    a_i = G sum_{j != i} m_j d s^3,   d = x_j - x_i,   s = (|d|^2 + eps^2)^(-1/2),   cotangent g = dL/da (n, 3)
    h_ij      = m_i g_j - m_j g_i
    dL/dx_i   =  G sum_{j != i} [ s^3 h_ij - 3 s^5 d (d . h_ij) ]
    dL/dm_i   = -G sum_{j != i}   s^3 (d . g_j)
The i == j term is excluded by index, whatever the softening (at eps = 0 torch's autograd gives NaN instead).

The terms of the sums, for the bar of hermite_f64_oracle (|got - ref| <= (T + 32) 2^-53 sum|terms|):
  position gradient, component k: 8 per source -- s^3 m_i g_j,k; s^3 m_j g_i,k; and the six products of
      3 s^5 d_k d_l h_l (l = 0, 1, 2) split by the two parts of h -- so T = 8 n (h and d . h may cancel, so their
      products are the terms, not their sums);
  mass gradient: 3 per source, s^3 d_l g_j,l, so T = 3 n.
accel_vjp_of_rows is the same arithmetic for a subset of the target rows (tests/vjp_rows_oracle.py).
"""
import numpy as np

_ROWS = 128


def accel_vjp(x, m, cot, g, eps2, order=None):
    """(dL/dx (n,3), dL/dm (n,), sum|terms| of dL/dx (n,3), sum|terms| of dL/dm (n,)) in fp64, the sources summed in
    the order `order` (a permutation of the bodies; None: as they are). Blocks of target rows against all sources, one
    (rows, n) array per scalar of a pair; with h = m_i g_j - m_j g_i split as stated, d . h = m_i (d . g_j) - m_j (d . g_i)
    and the sums over j of s^3 times a factor of j alone are matrix-vector products."""
    return accel_vjp_of_rows(x, m, cot, g, eps2, order, np.arange(np.asarray(x).shape[0]))


def accel_vjp_of_rows(x, m, cot, g, eps2, order, rows):
    """accel_vjp for the target rows `rows` (any indices, any order) under all n sources: the four results have
    len(rows) rows. accel_vjp is this with rows = 0 .. n - 1."""
    x = np.asarray(x, np.float64); m = np.asarray(m, np.float64); cot = np.asarray(cot, np.float64)
    n = x.shape[0]
    order = np.arange(n) if order is None else np.asarray(order)
    rows = np.asarray(rows, np.int64)
    xs, ms, gs = x[order], m[order], cot[order]
    ams, ags = np.abs(ms), np.abs(gs)
    nr = rows.size
    gx = np.zeros((nr, 3)); gm = np.zeros(nr); sx = np.zeros((nr, 3)); sm = np.zeros(nr)
    for lo in range(0, nr, _ROWS):
        hi = min(nr, lo + _ROWS)
        rr = rows[lo:hi]
        mi, gi = m[rr, None], cot[rr]
        d = [xs[None, :, k] - x[rr, None, k] for k in range(3)]                  # x_j - x_i, by component
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + eps2
        own = order[None, :] == rr[:, None]
        r2[own] = 1.0                                                            # any finite value: zeroed below
        s = 1.0 / np.sqrt(r2)
        s[own] = 0.0
        s2 = s * s
        s3 = s2 * s
        s5 = s3 * s2
        ad = [np.abs(c) for c in d]
        dgj = d[0] * gs[None, :, 0] + d[1] * gs[None, :, 1] + d[2] * gs[None, :, 2]          # d . g_j
        dgi = d[0] * gi[:, None, 0] + d[1] * gi[:, None, 1] + d[2] * gi[:, None, 2]          # d . g_i
        c5 = s5 * (mi * dgj - ms[None, :] * dgi)                                 # s^5 (d . h)
        a_dgj = [ad[l] * ags[None, :, l] for l in range(3)]                      # |d_l g_j,l|
        adgj = a_dgj[0] + a_dgj[1] + a_dgj[2]
        adgi = ad[0] * np.abs(gi[:, None, 0]) + ad[1] * np.abs(gi[:, None, 1]) + ad[2] * np.abs(gi[:, None, 2])
        q5 = s5 * (np.abs(mi) * adgj + ams[None, :] * adgi)                      # s^5 sum_l |d_l| (|m_i g_j,l| + |m_j g_i,l|)
        s3m, s3am = s3 @ ms, s3 @ ams
        for k in range(3):
            gx[lo:hi, k] = mi[:, 0] * (s3 @ gs[:, k]) - gi[:, k] * s3m - 3.0 * (c5 * d[k]).sum(1)
            sx[lo:hi, k] = np.abs(mi[:, 0]) * (s3 @ ags[:, k]) + np.abs(gi[:, k]) * s3am + 3.0 * (q5 * ad[k]).sum(1)
        gm[lo:hi] = -(s3 * dgj).sum(1)
        sm[lo:hi] = (s3 * adgj).sum(1)
    return g * gx, g * gm, abs(g) * sx, abs(g) * sm


def dense_accel(x, m, g, eps):
    """The all-pairs acceleration as a dense torch expression (what a user of the reference differentiates): every
    pair's weight (|d|^2 + eps^2)^(-3/2), the diagonal set to zero, one sum over the sources."""
    import torch
    n = x.shape[0]
    d = x.unsqueeze(0) - x.unsqueeze(1)
    w = (d.pow(2).sum(-1) + eps ** 2).pow(-1.5)
    w = w.masked_fill(torch.eye(n, dtype=torch.bool, device=x.device), 0.0)
    return g * (w.unsqueeze(-1) * d * m.view(1, n, 1)).sum(1)


def torch_vjp(x, m, cot, g, eps, dtype):
    """(dL/dx, dL/dm) as numpy float64 from torch's CPU autograd through dense_accel in `dtype`."""
    import torch
    xt = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    mt = torch.tensor(np.asarray(m), dtype=dtype, requires_grad=True)
    a = dense_accel(xt, mt, g, eps)
    a.backward(torch.tensor(np.asarray(cot), dtype=dtype))
    return xt.grad.double().numpy(), mt.grad.double().numpy()


def case(n, seed, fp32=False, zero_mass=False):
    """A Plummer sphere with unequal masses U(0.5, 1.5) / n and an N(0, 1) cotangent: (x, m, cot) in fp64. fp32: every
    value is fp32-representable; else 1e-9 perturbations make sure none is. zero_mass: body n // 2 is massless."""
    from nbd.plummer import generate_plummer
    rng = np.random.default_rng(seed)
    p, _, _ = generate_plummer(n, seed=seed)
    x = np.asarray(p, np.float64).reshape(n, 3)
    m = rng.uniform(0.5, 1.5, n) / n
    cot = rng.standard_normal((n, 3))
    if fp32:
        x, m, cot = (a.astype(np.float32).astype(np.float64) for a in (x, m, cot))
    else:
        x = x + rng.uniform(-1, 1, x.shape) * 1e-9
        m = m + rng.uniform(-1, 1, m.shape) * 1e-9 / n
    if zero_mass and n > 1:
        m[n // 2] = 0.0
    return x, m, cot
