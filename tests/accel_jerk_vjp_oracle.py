"""What the tests of the differentiable Hermite force (csrc/direct_hermite_grad.hip, nbd.autograd.direct_accel_jerk) share:
the fp64 numpy closed form of the vector-Jacobian product of (acceleration, jerk) with the sum of |terms| of every
component it forms, a dense torch statement of the pair for torch's own autograd, and the inputs.

    d = x_j - x_i,   w = v_j - v_i,   s = (|d|^2 + eps^2)^(-1/2)
    a_i = G sum_{j != i} m_j s^3 d,   j_i = G sum_{j != i} m_j [ s^3 w - 3 s^5 (d . w) d ]
    cotangents alpha = dL/da, beta = dL/dj (n, 3);   h^alpha = m_i alpha_j - m_j alpha_i,   h = m_i beta_j - m_j beta_i
    dL/dv_i =  G sum_j [ s^3 h - 3 s^5 d (d . h) ]
    dL/dx_i =  G sum_j [ s^3 h^alpha - 3 s^5 d (d . h^alpha) ]
             + G sum_j { -3 s^5 [ (h . w) d + (d . h) w + (d . w) h ] + 15 s^7 (d . w)(d . h) d }
    dL/dm_i = -G sum_j   s^3 (d . alpha_j)
             - G sum_j [ s^3 (beta_j . w) - 3 s^5 (d . w)(d . beta_j) ]
The i == j term is excluded by index, whatever the softening. The alpha lines, and dL/dv (the alpha line of dL/dx with
beta in the place of alpha), are accel_vjp_oracle.accel_vjp; the beta lines of dL/dx and dL/dm are formed here.

The terms of the sums, for the bar of hermite_f64_oracle (|got - ref| <= (T + 32) 2^-53 sum|terms|), by the rule of
accel_vjp_oracle.py -- where sums may cancel (h, and every dot product), the products are the terms:
  dL/dv, component k: 8 per source (accel_vjp_oracle), T = 8 n;
  dL/dx, component k: 8 (alpha) + 6 ((h . w) d_k: h_l w_l d_k, h in its two parts) + 6 ((d . h) w_k) + 6 ((d . w) h_k)
      + 18 ((d . w)(d . h) d_k: d_l w_l d_p h_p d_k, h in its two parts) = 44 per source, T = 44 n;
  dL/dm: 3 (alpha) + 3 (beta_j,l w_l) + 9 (d_l w_l d_p beta_j,p) = 15 per source, T = 15 n.
accel_jerk_vjp_of_rows is the same arithmetic for a subset of the target rows (tests/vjp_rows_oracle.py).
"""
import numpy as np

import accel_vjp_oracle as vo

_ROWS = 128
T_VEL, T_POS, T_MASS = 8, 44, 15            # terms per source


def _beta_lines(x, v, m, cot, g, eps2, order, rows):
    """The beta lines of dL/dx (len(rows),3) and dL/dm (len(rows),) of the target rows `rows` and the sum of |terms| of
    each, sources in the order `order`."""
    nr = rows.size
    xs, vs, ms, bs = x[order], v[order], m[order], cot[order]
    ams, abs_ = np.abs(ms), np.abs(bs)
    gx = np.zeros((nr, 3)); gm = np.zeros(nr); sx = np.zeros((nr, 3)); sm = np.zeros(nr)
    for lo in range(0, nr, _ROWS):
        hi = min(nr, lo + _ROWS)
        rr = rows[lo:hi]
        mi, bi = m[rr, None], cot[rr]
        d = [xs[None, :, k] - x[rr, None, k] for k in range(3)]
        w = [vs[None, :, k] - v[rr, None, k] for k in range(3)]
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + eps2
        own = order[None, :] == rr[:, None]
        r2[own] = 1.0                                                            # any finite value: zeroed below
        s = 1.0 / np.sqrt(r2)
        s[own] = 0.0
        s2 = s * s
        s3 = s2 * s
        s5 = s3 * s2
        s7 = s5 * s2
        ad, aw = [np.abs(c) for c in d], [np.abs(c) for c in w]
        h = [mi * bs[None, :, k] - ms[None, :] * bi[:, None, k] for k in range(3)]
        ah = [np.abs(mi) * abs_[None, :, k] + ams[None, :] * np.abs(bi[:, None, k]) for k in range(3)]
        dh = d[0] * h[0] + d[1] * h[1] + d[2] * h[2]
        dw = d[0] * w[0] + d[1] * w[1] + d[2] * w[2]
        hw = h[0] * w[0] + h[1] * w[1] + h[2] * w[2]
        adh = ad[0] * ah[0] + ad[1] * ah[1] + ad[2] * ah[2]
        adw = ad[0] * aw[0] + ad[1] * aw[1] + ad[2] * aw[2]
        ahw = ah[0] * aw[0] + ah[1] * aw[1] + ah[2] * aw[2]
        db = d[0] * bs[None, :, 0] + d[1] * bs[None, :, 1] + d[2] * bs[None, :, 2]           # d . beta_j
        bw = bs[None, :, 0] * w[0] + bs[None, :, 1] * w[1] + bs[None, :, 2] * w[2]           # beta_j . w
        adb = ad[0] * abs_[None, :, 0] + ad[1] * abs_[None, :, 1] + ad[2] * abs_[None, :, 2]
        abw = abs_[None, :, 0] * aw[0] + abs_[None, :, 1] * aw[1] + abs_[None, :, 2] * aw[2]
        for k in range(3):
            gx[lo:hi, k] = (-3.0 * s5 * (hw * d[k] + dh * w[k] + dw * h[k]) + 15.0 * s7 * dw * dh * d[k]).sum(1)
            sx[lo:hi, k] = (3.0 * s5 * (ahw * ad[k] + adh * aw[k] + adw * ah[k]) + 15.0 * s7 * adw * adh * ad[k]).sum(1)
        gm[lo:hi] = -(s3 * bw - 3.0 * s5 * dw * db).sum(1)
        sm[lo:hi] = (s3 * abw + 3.0 * s5 * adw * adb).sum(1)
    return g * gx, g * gm, abs(g) * sx, abs(g) * sm


def accel_jerk_vjp(x, v, m, cota, cotj, g, eps2, order=None):
    """(dL/dx (n,3), dL/dv (n,3), dL/dm (n,), sum|terms| of dL/dx, of dL/dv, of dL/dm) in fp64, the sources summed in the
    order `order` (a permutation of the bodies; None: as they are). cota or cotj None: that cotangent is zero."""
    return accel_jerk_vjp_of_rows(x, v, m, cota, cotj, g, eps2, order, np.arange(np.asarray(x).shape[0]))


def accel_jerk_vjp_of_rows(x, v, m, cota, cotj, g, eps2, order, rows):
    """accel_jerk_vjp for the target rows `rows` (any indices, any order) under all n sources: the six results have
    len(rows) rows. accel_jerk_vjp is this with rows = 0 .. n - 1."""
    x = np.asarray(x, np.float64); v = np.asarray(v, np.float64); m = np.asarray(m, np.float64)
    n = x.shape[0]
    rows = np.asarray(rows, np.int64)
    nr = rows.size
    gx = np.zeros((nr, 3)); gv = np.zeros((nr, 3)); gm = np.zeros(nr)
    sx = np.zeros((nr, 3)); sv = np.zeros((nr, 3)); sm = np.zeros(nr)
    if cota is not None:
        ax, am, asx, asm = vo.accel_vjp_of_rows(x, m, cota, g, eps2, order, rows)
        gx, gm, sx, sm = gx + ax, gm + am, sx + asx, sm + asm
    if cotj is not None:
        cotj = np.asarray(cotj, np.float64)
        gv, _, sv, _ = vo.accel_vjp_of_rows(x, m, cotj, g, eps2, order, rows)
        bx, bm, bsx, bsm = _beta_lines(x, v, m, cotj, g, eps2, np.arange(n) if order is None else np.asarray(order), rows)
        gx, gm, sx, sm = gx + bx, gm + bm, sx + bsx, sm + bsm
    return gx, gv, gm, sx, sv, sm


def dense_accel_jerk(x, v, m, g, eps):
    """(a, j) as a dense torch expression: every pair's powers of s with the diagonal made finite before the power and
    zeroed after it, one sum over the sources each."""
    import torch
    n = x.shape[0]
    d = x.unsqueeze(0) - x.unsqueeze(1)
    w = v.unsqueeze(0) - v.unsqueeze(1)
    eye = torch.eye(n, dtype=torch.bool, device=x.device)
    r2 = (d.pow(2).sum(-1) + eps ** 2).masked_fill(eye, 1.0)
    s3 = r2.pow(-1.5).masked_fill(eye, 0.0)
    s5 = r2.pow(-2.5).masked_fill(eye, 0.0)
    mj = m.view(1, n, 1)
    a = g * (s3.unsqueeze(-1) * d * mj).sum(1)
    dw = (d * w).sum(-1)
    j = g * ((s3.unsqueeze(-1) * w - 3.0 * (s5 * dw).unsqueeze(-1) * d) * mj).sum(1)
    return a, j


def torch_vjp(x, v, m, cota, cotj, g, eps, dtype):
    """(dL/dx, dL/dv, dL/dm) as numpy float64 from torch's CPU autograd through dense_accel_jerk in `dtype`."""
    import torch
    xt, vt, mt = (torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in (x, v, m))
    a, j = dense_accel_jerk(xt, vt, mt, g, eps)
    loss = 0.0
    if cota is not None:
        loss = loss + (a * torch.tensor(np.asarray(cota), dtype=dtype)).sum()
    if cotj is not None:
        loss = loss + (j * torch.tensor(np.asarray(cotj), dtype=dtype)).sum()
    loss.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return tuple(zero(t).double().numpy() for t in (xt, vt, mt))


def case(n, seed, fp32=False, zero_mass=False):
    """accel_vjp_oracle.case with velocities N(0, 0.3^2) and a second N(0, 1) cotangent: (x, v, m, cota, cotj) in fp64.
    fp32: every value is fp32-representable; else none is."""
    x, m, cota = vo.case(n, seed, fp32=fp32, zero_mass=zero_mass)
    rng = np.random.default_rng(seed + 7919)
    v = rng.standard_normal((n, 3)) * 0.3
    cotj = rng.standard_normal((n, 3))
    if fp32:
        v, cotj = (a.astype(np.float32).astype(np.float64) for a in (v, cotj))
    return x, v, m, cota, cotj
