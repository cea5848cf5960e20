"""fp64 numpy restatement of the tree potential of csrc/tree_force.hip (include/nbd.h, "tree-code gravity").

The walk is tree_oracle.tree_accel's, pass for pass: the same nodes (tree_oracle.build_nodes), the same opening test, the
same breadth-first pass per target group, so the accepted cells and the rejected level-0 nodes -- and the counters -- are
the ones the force sums. Only the terms differ: with r = c - x and u = (r.r + eps^2)^(-1/2) an accepted cell adds
    phi_cell = -( M u + 1/2 (r.Qr) u^5 )          (quadrupole off: -M u)
and a body j of a rejected level-0 node adds -m_j (d.d + eps^2)^(-1/2), j == i excluded by INDEX (a coincident distinct
body is kept: -inf at eps = 0). -grad phi_cell is tree_accel's cell term (d u / d x = u^3 r).
"""
import numpy as np

import tree_oracle as to


def cell_potential(x, c, M, Q, eps2, quadrupole=True):
    """phi_cell at the target x (3,) of one cell {c, M, Q}, G = 1."""
    r = np.asarray(c, dtype=np.float64) - np.asarray(x, dtype=np.float64)
    u = (r @ r + eps2) ** -0.5
    phi = M * u
    if quadrupole:
        phi += 0.5 * (r @ (np.asarray(Q) @ r)) * u ** 5
    return -phi


def cell_accel(x, c, M, Q, eps2, quadrupole=True):
    """The term tree_oracle.tree_accel adds for the same cell (restated for one target)."""
    r = np.asarray(c, dtype=np.float64) - np.asarray(x, dtype=np.float64)
    u = (r @ r + eps2) ** -0.5
    a = M * r * u ** 3
    if quadrupole:
        qr = np.asarray(Q) @ r
        a += -qr * u ** 5 + 2.5 * (r @ qr) * u ** 7 * r
    return a


def tree_potential(pos, mass, theta, softening, g_const=1.0, quadrupole=True, order=None, opening_dtype=np.float64,
                   groups=None):
    """(phi (n,) in the caller's order, (accepted cells, rejected level-0 nodes)); arguments as tree_oracle.tree_accel.
    groups: a list of target groups to walk alone -> (the rows of the listed groups one after another in TREE order,
    [(cells, leaves) per listed group]), as tree_oracle.tree_accel(groups=) gives them."""
    pos = np.asarray(pos, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    n = len(pos)
    phi = np.zeros(n)
    if n == 0:
        return (np.zeros(0), []) if groups is not None else (phi, (0, 0))
    order = to.morton_order(pos) if order is None else np.asarray(order, dtype=np.int64)
    assert sorted(order.tolist()) == list(range(n)), "order is not a permutation"
    x, m = pos[order], mass[order]
    levels = to.build_nodes(x, m)
    counts = [len(L["M"]) for L in levels]
    eps2 = float(softening) ** 2
    od = opening_dtype
    n_cells = n_leaves = 0
    out, per_group = np.zeros(n), []
    walked = range(-(-n // to.GROUP)) if groups is None else [int(g) for g in groups]
    assert all(0 <= g < -(-n // to.GROUP) for g in walked), "group outside the tree"
    for g0 in (g * to.GROUP for g in walked):
        g1 = min(n, g0 + to.GROUP)
        xt = x[g0:g1]
        tlo, thi = xt.min(0).astype(od), xt.max(0).astype(od)
        f = np.zeros(g1 - g0)
        before = (n_cells, n_leaves)
        front = np.array([0])
        for lvl in range(len(levels) - 1, -1, -1):
            L = levels[lvl]
            c = L["c"][front].astype(od)
            s = L["s"][front].astype(od)
            gap = np.maximum(np.maximum(tlo - c, c - thi), od(0))
            d2 = (gap * gap).sum(1, dtype=od)
            th2 = od(od(theta) * od(theta))
            accept = (s * s < th2 * d2) if theta > 0 else np.zeros(len(front), dtype=bool)
            cells, rest = front[accept], front[~accept]
            n_cells += len(cells)
            if len(cells):
                r = L["c"][cells][None, :, :] - xt[:, None, :]                      # (t, k, 3)
                u = ((r * r).sum(2) + eps2) ** -0.5
                term = L["M"][cells][None, :] * u
                if quadrupole:
                    qr = np.einsum("kab,tkb->tka", L["Q"][cells], r)
                    term += 0.5 * (r * qr).sum(2) * u ** 5
                f -= term.sum(1)
            if lvl > 0:
                kids = (rest[:, None] * to.LEAF + np.arange(to.LEAF)[None, :]).ravel()
                front = kids[kids < counts[lvl - 1]]
            else:
                n_leaves += len(rest)
                j = (rest[:, None] * to.LEAF + np.arange(to.LEAF)[None, :]).ravel()
                j = j[j < n]
                d = x[j][None, :, :] - xt[:, None, :]
                with np.errstate(divide="ignore", invalid="ignore"):
                    w = ((d * d).sum(2) + eps2) ** -0.5
                    w[np.arange(g0, g1)[:, None] == j[None, :]] = 0.0               # j == i by index
                    f -= (m[j][None, :] * w).sum(1)
        out[g0:g1] = f
        per_group.append((n_cells - before[0], n_leaves - before[1]))
    if groups is not None:
        rows = np.concatenate([np.arange(g * to.GROUP, min(n, g * to.GROUP + to.GROUP)) for g in walked]) if walked \
            else np.zeros(0, dtype=np.int64)
        return g_const * out[rows], per_group
    phi[order] = g_const * out
    return phi, (n_cells, n_leaves)


def direct_potential(pos, mass, softening, g_const=1.0):
    """The fp64 all-pairs sum phi_i = -G sum_{j != i} m_j (|r_ij|^2 + eps^2)^(-1/2), row block by row block."""
    pos = np.asarray(pos, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    n = len(pos)
    phi = np.zeros(n)
    eps2 = float(softening) ** 2
    for i0 in range(0, n, 512):
        i1 = min(n, i0 + 512)
        d = pos[None, :, :] - pos[i0:i1, None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            w = ((d * d).sum(2) + eps2) ** -0.5
            w[np.arange(i1 - i0), np.arange(i0, i1)] = 0.0
            phi[i0:i1] = -(mass[None, :] * w).sum(1)
    return g_const * phi


def potential_energy(mass, phi):
    """U = 1/2 sum m phi."""
    return 0.5 * float(np.asarray(mass, dtype=np.float64) @ np.asarray(phi, dtype=np.float64))


def row_errors(phi, ref):
    """|phi_i - ref_i| / |ref_i| (every body of a system of two or more has phi < 0)."""
    phi, ref = np.asarray(phi, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(phi - ref) / np.maximum(np.abs(ref), 1e-300)
