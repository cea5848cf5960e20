"""fp64 numpy restatement of the tree force of csrc/tree_force.hip (include/nbd.h, "tree-code gravity").

The body ORDER is an input (feed it a simulator's tree_order() to get the very tree the GPU walked) or computed here as
the stable order of fp64 Morton keys. Everything else -- nodes, opening test, accepted-cell term, direct part -- is
float64, written for clarity: a breadth-first pass per target group (the GPU walks depth-first; the set of accepted
cells and rejected level-0 nodes of a group does not depend on the traversal).
"""
import numpy as np

LEAF = 8
GROUP = 64


def plan(n):
    """(levels, nodes_total, [count per level]) of the implicit hierarchy over n bodies."""
    if n == 0:
        return 0, 0, []
    counts = [-(-n // LEAF)]
    while counts[-1] > 1:
        counts.append(-(-counts[-1] // LEAF))
    return len(counts), sum(counts), counts


def _spread21(v):
    x = v.astype(np.uint64) & np.uint64(0x1fffff)
    for shift, mask in ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f),
                        (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(shift))) & np.uint64(mask)
    return x


def morton_order(pos):
    """Stable order of the 3 x 21-bit Morton keys of pos on the bounding cube of all bodies (fp64 quantisation)."""
    pos = np.asarray(pos, dtype=np.float64)
    if len(pos) == 0:
        return np.zeros(0, dtype=np.int64)
    lo = pos.min(0)
    side = (pos.max(0) - lo).max()
    scale = 2097152.0 / side if side > 0 else 0.0
    q = np.clip(np.floor((pos - lo) * scale), 0, 2097151).astype(np.uint64)
    key = (_spread21(q[:, 0]) << np.uint64(2)) | (_spread21(q[:, 1]) << np.uint64(1)) | _spread21(q[:, 2])
    return np.argsort(key, kind="stable")


def build_nodes(x, m):
    """Per level (0 first): dict of M (k,), c (k,3), Q (k,3,3), s (k,) for the nodes over the SORTED bodies x, m."""
    n = len(x)
    levels = []
    for lvl, count in enumerate(plan(n)[2]):
        span = LEAF ** (lvl + 1)
        starts = np.arange(count) * span
        sizes = np.minimum(n, starts + span) - starts
        owner = np.repeat(np.arange(count), sizes)
        M = np.add.reduceat(m, starts)
        mx = np.add.reduceat(m[:, None] * x, starts, axis=0)
        mean = np.add.reduceat(x, starts, axis=0) / sizes[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where((M != 0)[:, None], mx / M[:, None], mean)
        d = x - c[owner]
        outer = 3.0 * d[:, :, None] * d[:, None, :] - (d * d).sum(1)[:, None, None] * np.eye(3)
        Q = np.add.reduceat(m[:, None, None] * outer, starts, axis=0)
        blo = np.minimum.reduceat(x, starts, axis=0)
        bhi = np.maximum.reduceat(x, starts, axis=0)
        s = (bhi - blo).max(1) + np.abs(c - 0.5 * (blo + bhi)).max(1)
        levels.append(dict(M=M, c=c, Q=Q, s=s))
    return levels


def tree_accel(pos, mass, theta, softening, g_const=1.0, quadrupole=True, order=None, opening_dtype=np.float64,
               groups=None, cond=False):
    """(acc (n,3) in the caller's order, (accepted cells, rejected level-0 nodes)).

    opening_dtype=np.float32 makes the opening decision the way an fp32 walk does (c, s and the group boxes rounded to
    float32, the comparison s^2 < theta^2 d^2 in float32); the forces stay float64.
    groups: a list of target groups (group g = the sorted bodies [64 g, min(n, 64 g + 64))) to walk alone. The result is
    then (rows, [(cells, leaves) per listed group]): the rows of the listed groups one after another in TREE order,
    without padding.
    cond=True appends the condition sums (rows, 2), ordered as the rows: the sum over everything added to the row of the
    Euclidean norm of each addend, times |g_const| -- column 0 over the pair terms m w d, column 1 over the accepted
    cells, each the three vectors it is made of, M r u^3, (Q r) u^5 and 2.5 (r.Qr) u^7 r. S_i is the sum of the two: an
    fp32 sum of the same addends is within a small multiple of 2^-24 S_i of the exact one, however much they cancel."""
    pos = np.asarray(pos, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    n = len(pos)
    acc = np.zeros((n, 3))
    if n == 0:
        empty = (np.zeros((0, 3)), []) if groups is not None else (acc, (0, 0))
        return empty + ((np.zeros((0, 2)),) if cond else ())
    order = morton_order(pos) if order is None else np.asarray(order, dtype=np.int64)
    assert sorted(order.tolist()) == list(range(n)), "order is not a permutation"
    x, m = pos[order], mass[order]
    levels = build_nodes(x, m)
    counts = [len(L["M"]) for L in levels]
    eps2 = float(softening) ** 2
    od = opening_dtype
    n_cells = n_leaves = 0
    out, cond_out, per_group = np.zeros((n, 3)), np.zeros((n, 2)), []
    walked = range(-(-n // GROUP)) if groups is None else [int(g) for g in groups]
    assert all(0 <= g < -(-n // GROUP) for g in walked), "group outside the tree"
    for g0 in (g * GROUP for g in walked):
        g1 = min(n, g0 + GROUP)
        xt = x[g0:g1]
        tlo, thi = xt.min(0).astype(od), xt.max(0).astype(od)
        a, S = np.zeros((g1 - g0, 3)), np.zeros((g1 - g0, 2))
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
                term = L["M"][cells][None, :, None] * r * (u ** 3)[:, :, None]
                if quadrupole:
                    qr = np.einsum("kab,tkb->tka", L["Q"][cells], r)
                    rqr = (r * qr).sum(2)
                    term += -qr * (u ** 5)[:, :, None] + 2.5 * (rqr * u ** 7)[:, :, None] * r
                a += term.sum(1)
                if cond:
                    rn = np.linalg.norm(r, axis=2)
                    S[:, 1] += (np.abs(L["M"][cells])[None, :] * rn * u ** 3).sum(1)
                    if quadrupole:
                        S[:, 1] += (np.linalg.norm(qr, axis=2) * u ** 5 + 2.5 * np.abs(rqr) * u ** 7 * rn).sum(1)
            if lvl > 0:
                kids = (rest[:, None] * LEAF + np.arange(LEAF)[None, :]).ravel()
                front = kids[kids < counts[lvl - 1]]
            else:
                n_leaves += len(rest)
                j = (rest[:, None] * LEAF + np.arange(LEAF)[None, :]).ravel()
                j = j[j < n]
                d = x[j][None, :, :] - xt[:, None, :]
                with np.errstate(divide="ignore", invalid="ignore"):
                    w = ((d * d).sum(2) + eps2) ** -1.5
                    w[np.arange(g0, g1)[:, None] == j[None, :]] = 0.0               # j == i by index
                    a += ((m[j][None, :] * w)[:, :, None] * d).sum(1)
                    if cond:
                        S[:, 0] += (np.abs(m[j])[None, :] * w * np.linalg.norm(d, axis=2)).sum(1)
        out[g0:g1], cond_out[g0:g1] = a, S
        per_group.append((n_cells - before[0], n_leaves - before[1]))
    if groups is not None:
        rows = np.concatenate([np.arange(g * GROUP, min(n, g * GROUP + GROUP)) for g in walked]) if walked else \
            np.zeros(0, dtype=np.int64)
        return (g_const * out[rows], per_group) + ((abs(g_const) * cond_out[rows],) if cond else ())
    acc[order] = g_const * out
    if cond:
        S_caller = np.zeros((n, 2))
        S_caller[order] = abs(g_const) * cond_out
        return acc, (n_cells, n_leaves), S_caller
    return acc, (n_cells, n_leaves)


def direct_accel(pos, mass, softening, g_const=1.0):
    """The fp64 all-pairs sum, row block by row block."""
    pos = np.asarray(pos, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    n = len(pos)
    acc = np.zeros((n, 3))
    eps2 = float(softening) ** 2
    for i0 in range(0, n, 512):
        i1 = min(n, i0 + 512)
        d = pos[None, :, :] - pos[i0:i1, None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            w = ((d * d).sum(2) + eps2) ** -1.5
            w[np.arange(i1 - i0), np.arange(i0, i1)] = 0.0
            acc[i0:i1] = ((mass[None, :] * w)[:, :, None] * d).sum(1)
    return g_const * acc


def row_errors(a, ref):
    """Per-row |a_i - ref_i| / max(|ref_i|, 1e-3 RMS row norm): the rows behind conftest.row_rel's maximum."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return np.zeros(0)
    nrm = np.linalg.norm(ref, axis=-1)
    floor = max(1e-3 * np.sqrt((nrm ** 2).mean()), 1e-300)
    return np.linalg.norm(a - ref, axis=-1) / np.maximum(nrm, floor)


# ---------------------------------------------------------------- the inputs the tree tests share (softening 0.1)

SHIFT = np.array([12.0, 3.0, -2.0])
SOFTENING = 0.1


def case(name):
    """(pos, vel, mass) float32 arrays of input A, B, C or D."""
    from nbd.plummer import generate_plummer
    if name == "A":
        p, v, m = generate_plummer(2048, seed=1)
    elif name == "B":
        p, v, m = generate_plummer(1000, seed=3)
        m = m * np.random.default_rng(3).uniform(0.2, 5.0, len(m))
    elif name == "C":
        p, v, m = generate_plummer(4096, seed=2)
    elif name == "D":
        p, v, m = generate_plummer(1027, seed=7)
        idx = np.minimum(np.arange(1027) // 16, 64)               # the first 65 bodies, 16 copies each (the last: 3)
        p, v, m = p[idx], v[idx], m[idx]
    else:
        raise KeyError(name)
    p, v, m = (np.array(t, dtype=np.float64) for t in (p, v, m))
    if name != "C":
        p[len(p) // 2:] += SHIFT
    return p.astype(np.float32), v.astype(np.float32), m.astype(np.float32)
