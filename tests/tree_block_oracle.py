"""fp64 numpy restatement of the listed-target walk of csrc/tree_force.hip and of the block-timestep scheme of
csrc/tree_block.hip (include/nbd.h, "Listed targets" and "block timesteps over the tree force"; DESIGN.md K-T, "Block
timesteps").

tree_accel_active() is tree_oracle.tree_accel() with its target groups taken from a list of sorted positions: the same
nodes (tree_oracle.build_nodes), the same breadth-first pass, the same terms in the same order, so that with every body
listed it returns tree_accel()'s numbers exactly. block_leapfrog() is the hierarchical kick-drift-kick in float64 with
a pluggable force; the level arithmetic (wanted_level) is the device's, operation for operation.
"""
import numpy as np

import tree_oracle as to

LEAF, GROUP = to.LEAF, to.GROUP


def tree_accel_active(pos, mass, theta, softening, g_const, quadrupole, order, active_sorted, opening_dtype=np.float64):
    """(rows (len(active_sorted), 3), (accepted cells, rejected level-0 nodes)): row t is the acceleration of the body at
    sorted position active_sorted[t] (the caller's body order[active_sorted[t]]), from target groups of 64 consecutive
    entries of active_sorted, each with the box of its own bodies. opening_dtype as in tree_oracle.tree_accel."""
    pos = np.asarray(pos, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    n = len(pos)
    act = np.asarray(active_sorted, dtype=np.int64)
    out = np.zeros((len(act), 3))
    if n == 0 or len(act) == 0:
        return out, (0, 0)
    order = np.asarray(order, dtype=np.int64)
    assert sorted(order.tolist()) == list(range(n)), "order is not a permutation"
    assert (np.diff(act) > 0).all() and act[0] >= 0 and act[-1] < n, "active_sorted is not ascending sorted positions"
    x, m = pos[order], mass[order]
    levels = to.build_nodes(x, m)
    counts = [len(L["M"]) for L in levels]
    eps2 = float(softening) ** 2
    od = opening_dtype
    n_cells = n_leaves = 0
    for g0 in range(0, len(act), GROUP):
        idx = act[g0:g0 + GROUP]
        xt = x[idx]
        tlo, thi = xt.min(0).astype(od), xt.max(0).astype(od)
        a = np.zeros((len(idx), 3))
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
                    w[idx[:, None] == j[None, :]] = 0.0                             # j == i by sorted index
                    a += ((m[j][None, :] * w)[:, :, None] * d).sum(1)
        out[g0:g0 + GROUP] = a
    return g_const * out, (n_cells, n_leaves)


# ---------------------------------------------------------------- the block scheme

def wanted_level(acc, dt, eta, softening, max_level):
    """(level (n,), over (n,) bool, margin): the smallest k in [0, K] with (dt 2^-k)^4 (a.a) <= (2 eta eps)^2 from the
    float32 acceleration, in float64 with the device's operation order; over where no level up to K satisfies it (a NaN
    too), and then the level is K. margin: the smallest |ratio - 1| over the bodies, ratio = h_k^4 (a.a) / (2 eta eps)^2
    at the chosen level and at the one above it (the coarser one, where there is one)."""
    a = np.asarray(acc, dtype=np.float32).astype(np.float64)
    K = int(max_level)
    aa = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]
    c = 2.0 * float(eta) * float(softening)
    lim = c * c
    level = np.full(len(a), K, dtype=np.int64)
    found = np.zeros(len(a), dtype=bool)
    ratio = np.empty((K + 1, len(a)))
    for k in range(K + 1):
        h = float(dt) * 2.0 ** -k
        h2 = h * h
        h4 = h2 * h2
        with np.errstate(invalid="ignore"):
            ok = (h4 * aa <= lim) & ~found
        level[ok] = k
        found |= ok
        ratio[k] = h4 * aa / lim
    margin = np.inf
    if len(a):
        rows = np.arange(len(a))
        at = np.abs(ratio[level, rows] - 1.0)
        above = np.where(level > 0, np.abs(ratio[np.maximum(level - 1, 0), rows] - 1.0), np.inf)
        margin = float(np.nanmin(np.minimum(at, above))) if np.isfinite(np.minimum(at, above)).any() else np.inf
    return level, ~found, margin


def block_leapfrog(pos, vel, mass, dt, eta, max_level, steps, force, softening=to.SOFTENING, acc_dtype=np.float32):
    """The scheme of csrc/tree_block.hip in float64. force(pos) -> acc (n,3) of all bodies (the rows of the bodies that
    are not due are not used). The level decisions read the acceleration rounded to acc_dtype, as the device reads its
    fp32 force. Returns a dict: states [(pos, vel, acc) after every step], levels [the levels after every block step],
    n_act [per block step], clamped (every decision that wanted a level deeper than max_level, the initial ones
    included), margin (the smallest relative margin of any level decision: see wanted_level)."""
    x = np.array(pos, dtype=np.float64)
    v = np.array(vel, dtype=np.float64)
    n, K = len(x), int(max_level)
    end = 1 << K
    out = dict(states=[], levels=[], n_act=[], clamped=0, margin=np.inf)
    a = np.array(force(x), dtype=np.float64)
    level, over, margin = wanted_level(a.astype(acc_dtype), dt, eta, softening, K)
    out["clamped"] += int(over.sum())
    out["margin"] = min(out["margin"], margin)
    out["initial_levels"] = level.copy()
    for _ in range(steps):
        if n == 0:
            out["states"].append((x.copy(), v.copy(), a.copy()))
            continue
        half = 0.5 * dt * 2.0 ** -level
        v += a * half[:, None]
        s = np.zeros(n, dtype=np.int64)
        t_cur = 0
        while True:
            d = 1 << (K - level)
            t_next = int((s + d).min())
            x += v * (dt * (t_next - t_cur) * 2.0 ** -K)
            due = s + d == t_next
            a[due] = np.asarray(force(x), dtype=np.float64)[due]
            v[due] += a[due] * (0.5 * dt * 2.0 ** -level[due])[:, None]
            want, over, margin = wanted_level(a[due].astype(acc_dtype), dt, eta, softening, K)
            out["clamped"] += int(over.sum())
            out["margin"] = min(out["margin"], margin)
            cur = level[due]
            rise = (want < cur) & (t_next % (1 << (K - np.maximum(cur, 1) + 1)) == 0)
            new = np.where(want > cur, want, np.where(rise, cur - 1, cur))
            level[due] = new
            if t_next < end:
                v[due] += a[due] * (0.5 * dt * 2.0 ** -new)[:, None]
                s[due] = t_next
            out["levels"].append(level.copy())
            out["n_act"].append(int(due.sum()))
            t_cur = t_next
            if t_next == end:
                break
        assert due.all(), "the interval ended with a body that was not due"
        out["states"].append((x.copy(), v.copy(), a.copy()))
    return out


def plain_leapfrog(pos, vel, dt, steps, force):
    """The shared-step kick-drift-kick in float64: [(pos, vel, acc) after every step]."""
    x = np.array(pos, dtype=np.float64)
    v = np.array(vel, dtype=np.float64)
    a = np.array(force(x), dtype=np.float64)
    half = 0.5 * dt
    states = []
    for _ in range(steps):
        v += a * half
        x += v * dt
        a = np.array(force(x), dtype=np.float64)
        v += a * half
        states.append((x.copy(), v.copy(), a.copy()))
    return states


# ---------------------------------------------------------------- the input of the trajectory tests

TRAJ = dict(n=600, seed=34, dt=0.1, eta=0.002, max_level=4, steps=2)


def trajectory_case():
    """(pos, vel, mass) float32: a Plummer sphere whose accelerations span three levels and more under TRAJ."""
    from nbd.plummer import generate_plummer
    p, v, m = generate_plummer(TRAJ["n"], seed=TRAJ["seed"])
    return (np.asarray(p, dtype=np.float32), np.asarray(v, dtype=np.float32), np.asarray(m, dtype=np.float32))


def direct_force(mass, softening=to.SOFTENING, g_const=1.0):
    """force(pos) of block_leapfrog: the fp64 direct sum."""
    return lambda x: to.direct_accel(x, mass, softening, g_const)
