"""What a build of csrc/tree_force.hip must leave, restated: the fp32 Morton keys bit for bit (keys_f32), the bounds of a
node record against the fp64 nodes of tree_oracle.build_nodes (node_tolerances), and the inputs off the Plummer path that
tests/test_tree_build_gpu.py and tests/test_tree_build_host.py share (softening 0.1, G = 1, float32 after construction).
"""
import numpy as np

import tree_oracle as to

F = np.float32
CELLS = 2097152                      # 2^21 cells per axis of the bounding cube


def box_f32(pos):
    """(lo (3,), hi (3,), scale, centre (3,)) as box_partial / box_final leave them, float32: fmin / fmax reductions (a
    NaN coordinate is skipped), the cube's side the longest edge, scale = 2^21 / side (0 for a point), centre = lo / 2 +
    hi / 2."""
    pos = np.asarray(pos, dtype=F)
    lo, hi = np.fmin.reduce(pos, axis=0), np.fmax.reduce(pos, axis=0)
    side = F(0)
    for a in range(3):
        side = np.fmax(side, F(hi[a] - lo[a]))
    with np.errstate(over="ignore"):
        scale = F(CELLS) / side if side > 0 else F(0)
    return lo, hi, F(scale), F(0.5) * lo + F(0.5) * hi


def keys_f32(pos):
    """The uint64 keys of key_kernel: q = uint32(clip((pos - lo) * scale, 0, 2^21 - 1)) with every operation rounded to
    float32 (a NaN lands in cell 0, as fmaxf(NaN, 0) = 0 does), key = spread(x) << 2 | spread(y) << 1 | spread(z). The
    library is built without fast-math and with -ffp-contract=off, its fp32 division is correctly rounded: the same bits."""
    pos = np.asarray(pos, dtype=F)
    if len(pos) == 0:
        return np.zeros(0, dtype=np.uint64)
    lo, _, scale, _ = box_f32(pos)
    with np.errstate(invalid="ignore", over="ignore"):
        f = (pos - lo[None, :]).astype(F) * scale
        q = np.fmin(np.fmax(f.astype(F), F(0)), F(CELLS - 1)).astype(np.uint32)
    return (to._spread21(q[:, 0]) << np.uint64(2)) | (to._spread21(q[:, 1]) << np.uint64(1)) | to._spread21(q[:, 2])


def order_f32(pos):
    """The order a stable sort of keys_f32 leaves: equal keys in index order."""
    return np.argsort(keys_f32(pos), kind="stable")


# ---------------------------------------------------------------- node records against the fp64 nodes
#
# The build (csrc/tree_force.hip: leaf_kernel, upper_kernel, finish_node) sums in fp64, level by level, a node's mass, its
# first moments and the sum of its positions about `centre`, the centre of the bounding box of ALL bodies (a leaf adds up
# to 8 bodies, a parent up to 8 children: at most 8 (L + 1) adds per sum of a level-L node, and a few more roundings per
# addend for the products), and its second moments about the node's OWN centre of mass (a leaf from its bodies, a parent
# from its children by the parallel-axis theorem); the record is stored fp32.
# With y_j = x_j - centre (exact in fp64), R = max |y_j| over the node's bodies, A = sum |m_j| and
#     E = (8 (L + 1) + 8) 2^-53
# the mass and the first moments are within E A and E A R of their exact values. From these:
#   M   2^-24 |M| (the fp32 store) + E A.
#   c   c = m1 / M: |delta c| <= (delta m1 + |c| delta M) / |M| <= 2 E A R / |M|, the same again for the quotient and the
#       sum centre + c: delta = 4 E A R / |M| per component, + 2^-24 |c| for the store. A massless node takes the mean of
#       its bodies, sum y / count: delta = E R.
#   s   the AABB is exact in fp32, so s = edge + shift errs by the c bound (shift is a max-norm of c - AABB centre) and
#       by its own store, 2^-24 s.
#   Q   C = sum m d d^T with d = y - c of size rho = r + delta at most, r the node's largest |x_j - c|: the sums' own
#       roundings are E A rho^2 per entry. The centres carry delta each (the node's and, in a parent, each child's: the
#       largest delta of the node and everything below it is taken), and a parent's M_k d_k d_k^T moves by 2 M_k |d_k| 2
#       delta: 4 A rho delta per entry. 3 C - tr takes both to 12 (E A rho^2 + 4 A rho delta) in Frobenius norm; the fp32
#       store adds 2^-24 per entry and the fp64 reference 3 d d - |d|^2 about its own c is good to the same order: 2^-23
#       |Q|_F. What a far outlier costs is the delta term alone: it moves `centre`, R grows to the size of the cube for
#       EVERY node, and a small node's Q keeps E R / r relative accuracy -- 1e-8 for a cluster of size 1 and a body at 1e6.
#       (Central moments taken from RAW second moments about `centre`, m2 - m1 c - c m1 + M c c, would keep 12 E A R^2: a
#       relative E R^2 / r^2, 1e-2 on that input. The build did that once; the walks of test_tree_build_gpu.py showed it.)
# Each bound is doubled, no more. A massless node has M and Q exactly 0 (every moment is a sum of exact zeros).
MARGIN = 2.0


def node_tolerances(x_sorted, m_sorted, centre):
    """Per level (0 first) a dict of the bounds above for the nodes over the sorted bodies: M (k,), c (k,3) per component,
    s (k,), Q (k,) in Frobenius norm of the 3 x 3 error; `centre` the centre of the bounding box of all bodies."""
    x, m = np.asarray(x_sorted, dtype=np.float64), np.asarray(m_sorted, dtype=np.float64)
    n = len(x)
    ref = to.build_nodes(x, m)
    dist = np.linalg.norm(x - np.asarray(centre, dtype=np.float64)[None, :], axis=1)
    out, delta_below = [], None
    for lvl, count in enumerate(to.plan(n)[2]):
        span = to.LEAF ** (lvl + 1)
        starts = np.arange(count) * span
        R = np.maximum.reduceat(dist, starts)
        A = np.add.reduceat(np.abs(m), starts)
        E = (8 * (lvl + 1) + 8) * 2.0 ** -53
        M, c, s, Q = (ref[lvl][k] for k in ("M", "c", "s", "Q"))
        massless = M == 0
        with np.errstate(divide="ignore", invalid="ignore"):
            delta = np.where(massless, E * R, 4 * E * A * R / np.abs(M))
        c_tol = 2.0 ** -24 * np.abs(c) + delta[:, None]
        owner = np.repeat(np.arange(count), np.minimum(n, starts + span) - starts)
        r = np.maximum.reduceat(np.linalg.norm(x - c[owner], axis=1), starts)
        if delta_below is not None:
            delta = np.maximum(delta, np.maximum.reduceat(delta_below, np.arange(count) * to.LEAF))
        rho = r + delta
        out.append(dict(M=MARGIN * (2.0 ** -24 * np.abs(M) + E * A),
                        c=MARGIN * c_tol,
                        s=MARGIN * (2.0 ** -24 * s + c_tol.max(1)),
                        Q=MARGIN * np.where(massless, 0.0, 2.0 ** -23 * np.linalg.norm(Q, axis=(1, 2))
                                            + 12 * (E * A * rho * rho + 4 * A * rho * delta))))
        delta_below = delta
    return out


def unpack_nodes(rows):
    """(M, c, s, Q (k,3,3)) float64 of one level's (k, 12) float32 records {c, s}, {M, Qxx, Qxy, Qxz}, {Qyy, Qyz, Qzz, 0}."""
    r = np.asarray(rows, dtype=np.float64)
    Q = np.empty((len(r), 3, 3))
    Q[:, 0, 0], Q[:, 0, 1], Q[:, 0, 2], Q[:, 1, 1], Q[:, 1, 2], Q[:, 2, 2] = r[:, 5], r[:, 6], r[:, 7], r[:, 8], r[:, 9], r[:, 10]
    Q[:, 1, 0], Q[:, 2, 0], Q[:, 2, 1] = Q[:, 0, 1], Q[:, 0, 2], Q[:, 1, 2]
    return r[:, 4], r[:, 0:3], r[:, 3], Q


# ---------------------------------------------------------------- inputs

WALKED = ["line", "sheet", "outlier", "masses"]
THETAS = [0.05, 0.5, 0.75, 1.5]
DEEP_N = 33025                       # 32 768 + 257: 4129 / 517 / 65 / 9 / 2 / 1 nodes, the waves divide the tree at level 2
_inputs = {}


def plummer(n, seed):
    from nbd.plummer import generate_plummer
    p, _, m = generate_plummer(n, seed=seed)
    return np.array(p, dtype=np.float64), np.array(m, dtype=np.float64)


def _make():
    rng = np.random.default_rng(20)          # draws in this order
    # line: zero-thickness boxes on two axes
    x = np.sort(rng.uniform(-1, 1, 1000) ** 3 * 4); p = np.zeros((1000, 3)); p[:, 0] = x
    perm = rng.permutation(1000)
    _inputs["line"] = (p[perm], rng.uniform(0.5, 2, 1000) / 1000)
    # sheet: a jittered 32 x 32 lattice in the plane z = 0.25
    g = np.stack(np.meshgrid(np.arange(32), np.arange(32), indexing="ij"), -1).reshape(-1, 2) / 8.0
    p = np.zeros((1024, 3)); p[:, :2] = g + rng.normal(0, 1e-3, g.shape); p[:, 2] = 0.25
    _inputs["sheet"] = (p, np.full(1024, 1 / 1024))
    # outlier: one body at 1e6 -- grid cells ~0.5 wide, almost every key tied, order ~ index order
    p, m = plummer(1000, seed=5); p[-1] = [1e6, -1e6, 5e5]
    _inputs["outlier"] = (p, m)
    # masses: 6 decades, every 7th body massless, and 40 massless bodies in a far corner (whole massless leaf nodes)
    p, m = plummer(1000, seed=6); m = m * 10 ** rng.uniform(-3, 3, 1000); m[::7] = 0
    p[960:] = p[960:] * 0.05 + [9, 9, 9]; m[960:] = 0
    _inputs["masses"] = (p, m)
    for k, (p, m) in _inputs.items():
        _inputs[k] = (p.astype(F), m.astype(F))


def inputs(name):
    """(pos (n,3), mass (n,)) float32 of line, sheet, outlier, masses, deep, or a build-only input (BUILD_ONLY)."""
    if not _inputs:
        _make()
    if name not in _inputs:
        _inputs[name] = _other(name)
    return _inputs[name]


BUILD_ONLY = ["n1", "n7", "n8", "n9", "n64", "n65", "n513", "point", "faces", "D", "nan"]


def _other(name):
    if name == "deep":
        p, m = plummer(DEEP_N, seed=9); p[DEEP_N // 2:] += to.SHIFT
    elif name == "D":
        p, _, m = to.case("D")
    elif name == "point":                      # every body at one point: side = 0, scale = 0, every key 0
        p, m = np.tile([0.3, -1.7, 2.5], (100, 1)), np.linspace(1, 2, 100) / 100
    elif name == "faces":                      # a body exactly on each maximum face of the cube: clamped to 2^21 - 1
        p, m = plummer(200, seed=8)
        p = np.clip(p, -2, 2)
        p[0], p[1], p[2], p[3], p[4] = [2, 0.1, 0.2], [0.3, 2, -0.4], [-0.5, 0.6, 2], [2, 2, 2], [-2, -2, -2]
    elif name == "nan":                        # one NaN coordinate: cell 0 on that axis; checked for its order only
        p, m = plummer(100, seed=4)
        p[37, 1] = np.nan
    elif name[0] == "n":
        p, m = plummer(int(name[1:]), seed=11)
    else:
        raise KeyError(name)
    return np.asarray(p, dtype=F), np.asarray(m, dtype=F)


def deep_groups():
    """The 24 target groups of `deep` that are walked on their own: the first, the last (ONE body) and 22 seeded ones."""
    last = -(-DEEP_N // to.GROUP) - 1
    rest = np.random.default_rng(21).choice(np.arange(1, last), 22, replace=False)
    return [0, last] + sorted(int(g) for g in rest)
