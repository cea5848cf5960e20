"""What the tests of the fp32 Hermite force at chunk edges and long chunk walks share (test_hermite_walk_host.py,
test_hermite_walk_gpu.py): the inputs, a row sample, the fp64 force of a few target rows under all n sources with the sum
of |terms| of every component, and a plain float32 evaluation of the same rows in the kernel's summation order -- the
yardstick an fp32 kernel is held to where the flat 1e-5 of the golden states does not apply. Plain numpy, no GPU.

The walk of accel_jerk_body (csrc/hermite_kernels.h), restated: the n sources are ceil(n / 64) chunks of 64 (zero rows
behind n); with `slabs` slabs of 4 waves each, q = chunks // (4 slabs), r = chunks % (4 slabs), wave jw = 4 slab + wave
walks the chunks [jw q + min(jw, r), ... + q + (jw < r)) as ONE sequential fp32 chain of fused multiply-adds into nine
sums per target (w d, w dv, c d with w = m s^3, c = (d . dv) s^2 w), a = the first three, j = (w dv) - 3 (c d); the four
waves of a slab are added in wave order; the slabs are added as hermite_slab_sum adds them (the partial p_w = slab w +
slab w + 4 + ..., then (p0 + p1) + (p2 + p3), which is slab order up to four slabs); G is applied last.
The yardstick differs from the kernel in one place only: its 1 / sqrt is correctly rounded, v_rsq_f32 is good to 1 ulp.
Its fused multiply-add is the exact product plus the sum in fp64, rounded to fp32."""
import numpy as np

import accel_jerk_vjp_oracle as jo

CHUNK, WAVES, GROUP = 64, 4, 128
U24 = 2.0 ** -24
_ROWS = 128
_F = np.float32

# The sizes test_hermite_walk_gpu.py runs; what each stands for is WALKS of test_hermite_walk_host.py, which holds the
# launch plan to it.
EDGE_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 256, 257, 448, 449, 513, 705, 769, 1025]      # all rows
LONG_SIZES = [5057, 5633, 8385, 11649, 32193]                          # sampled rows and the all-rows net
LONG_EPS0 = [5633, 11649]                                              # the long sizes that also run eps = 0
STEP_SIZES = [5633, 32193]
PINNED_SCENES = [65, 5633, 8385]
ACTIVE_N, ACTIVE_LIST = 5633, 130


def case(n):
    """(x, v, m) in fp64, every value fp32-representable: a Plummer sphere, masses U(0.5, 1.5) / n, velocities
    N(0, 0.3^2) -- the fp32 case n of test_accel_jerk_vjp_gpu.py."""
    return jo.case(n, seed=200 + n, fp32=True)[:3]


def sample_rows(n):
    """All rows when n <= 1100; else the first target group of 128, the middle group, the whole last (ragged) group and
    64 seeded random rows, sorted, no row twice."""
    if n <= 1100:
        return np.arange(n)
    groups = -(-n // GROUP)
    mid = (groups // 2) * GROUP
    rnd = np.random.default_rng(n).choice(n, 64, replace=False)
    return np.unique(np.concatenate([np.arange(GROUP), np.arange(mid, mid + GROUP),
                                     np.arange((groups - 1) * GROUP, n), rnd]))


def chunk_plan(n, accel_plan):
    """{groups, slabs, chunks} from what nbd.direct.accel_plan(n, n_tgt) reports for n sources."""
    return {"groups": accel_plan["groups"], "slabs": accel_plan["slabs"], "chunks": -(-n // CHUNK)}


def split(plan):
    """(q, r): every wave walks q chunks, the first r waves one more."""
    return divmod(plan["chunks"], WAVES * plan["slabs"])


def active_plan(n, n_act, accel_plan):
    """plan_active of csrc/direct_hermite_block.hip: accel_plan = nbd.direct.accel_plan(n, n_act); fewer targets than
    sources get the slab count raised until groups x slabs reaches 512 (at least one chunk per wave, at most 256)."""
    p = chunk_plan(n, accel_plan)
    if n_act < n and p["groups"] * p["slabs"] < 512:
        s = min(-(-512 // p["groups"]), p["chunks"] // WAVES, 256)
        p["slabs"] = max(p["slabs"], s)
    return p


def accel_jerk_rows(x, v, m, g, eps2, rows):
    """(a, j, sum|a terms|, sum|j terms|), each (len(rows), 3) in fp64, of the target rows `rows` under all n sources; the
    self term is dropped by index. hermite_oracle.accel_jerk and hermite_f64_oracle.accel_jerk_abs on those rows."""
    x = np.asarray(x, np.float64); v = np.asarray(v, np.float64); m = np.asarray(m, np.float64)
    rows = np.asarray(rows, np.int64)
    k = rows.size
    a = np.zeros((k, 3)); j = np.zeros((k, 3)); sa = np.zeros((k, 3)); sj = np.zeros((k, 3))
    am = np.abs(m)
    for lo in range(0, k, _ROWS):
        rr = rows[lo:lo + _ROWS]
        own = (np.arange(rr.size), rr)
        d = x[None, :, :] - x[rr, None, :]
        dv = v[None, :, :] - v[rr, None, :]
        r2 = (d * d).sum(-1) + eps2
        r2[own] = 1.0                                # any finite value: the term is zeroed below
        s = 1.0 / np.sqrt(r2)
        s[own] = 0.0
        s3 = s ** 3
        w = m[None, :] * s3
        rv = (d * dv).sum(-1)
        a[lo:lo + rr.size] = (w[..., None] * d).sum(1)
        j[lo:lo + rr.size] = (w[..., None] * dv - 3.0 * (rv * s * s * w)[..., None] * d).sum(1)
        ad, adv = np.abs(d), np.abs(dv)
        aw = am[None, :] * s3
        sa[lo:lo + rr.size] = (aw[..., None] * ad).sum(1)
        sj[lo:lo + rr.size] = (aw[..., None] * adv + 3.0 * ((ad * adv).sum(-1) * s * s * aw)[..., None] * ad).sum(1)
    return g * a, g * j, abs(g) * sa, abs(g) * sj


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(_F)


def predict32(x, v, a0, j0, dt):
    """The fp32 predictor of hermite_predict (each product and sum rounded on its own, the step constants formed in
    double and rounded once): (x_p, v_p) as float32 arrays."""
    x, v, a0, j0 = (np.asarray(t, _F) for t in (x, v, a0, j0))
    h, h2, h3 = _F(dt), _F(0.5 * dt * dt), _F(dt * dt * dt / 6.0)
    return ((x + v * h) + a0 * h2) + j0 * h3, (v + a0 * h) + j0 * h2


def yardstick_rows(x, v, m, g, eps2, rows, plan):
    """(a, j), each (len(rows), 3) float32: the float32 evaluation of the module text for the target rows `rows`, with
    the chunk split of plan = {groups, slabs, chunks}."""
    x = np.asarray(x, _F); v = np.asarray(v, _F); m = np.asarray(m, _F)
    rows = np.asarray(rows, np.int64)
    n, chunks, slabs = x.shape[0], plan["chunks"], plan["slabs"]
    assert chunks == -(-n // CHUNK) and slabs >= 1
    waves = WAVES * slabs
    q, r = split(plan)
    npad = chunks * CHUNK
    xs = np.zeros((npad, 3), _F); vs = np.zeros((npad, 3), _F); ms = np.zeros(npad, _F)
    xs[:n], vs[:n], ms[:n] = x, v, m
    jw = np.arange(waves)
    length = q + (1 if r else 0)                                       # chunks of the longest walk
    at = ((jw * q + np.minimum(jw, r)) * CHUNK)[:, None] + np.arange(length * CHUNK)[None, :]       # (waves, steps)
    live = np.arange(length * CHUNK)[None, :] < ((q + (jw < r)) * CHUNK)[:, None]
    at = np.where(live, at, 0)
    e2 = np.full((), eps2, _F)
    out_a = np.zeros((rows.size, 3), _F); out_j = np.zeros((rows.size, 3), _F)
    for lo in range(0, rows.size, _ROWS):
        rr = rows[lo:lo + _ROWS]
        k = rr.size
        d = [xs[None, :, c] - xs[rr, None, c] for c in range(3)]       # float32 differences, (k, npad)
        d += [vs[None, :, c] - vs[rr, None, c] for c in range(3)]
        r2 = _fma(d[2], d[2], _fma(d[1], d[1], _fma(d[0], d[0], e2)))
        rv = _fma(d[2], d[5], _fma(d[1], d[4], d[0] * d[3]))
        drop = np.broadcast_to(np.arange(npad) >= n, (k, npad)).copy() # the padding and the target itself: s = 0
        drop[np.arange(k), rr] = True
        with np.errstate(divide="ignore"):
            s = (1.0 / np.sqrt(r2.astype(np.float64))).astype(_F)      # correctly rounded (to a double rounding)
        s[drop] = 0.0
        s2 = s * s
        w = (s2 * s) * ms[None, :]
        c = (rv * s2) * w
        # every wave's chain, all waves and rows at once: (steps, k, waves) per factor; a step past a wave's end adds 0
        fac = np.stack([np.where(live[None], t[:, at], _F(0)) for t in (w, c)]).transpose(3, 0, 1, 2)
        dd = np.stack([t[:, at] for t in d]).transpose(3, 0, 1, 2)
        acc = np.zeros((9, k, waves), _F)
        for t in range(at.shape[1]):
            f, e = fac[t].astype(np.float64), dd[t].astype(np.float64)
            acc[:6] = (f[0][None] * e + acc[:6]).astype(_F)
            acc[6:] = (f[1][None] * e[:3] + acc[6:]).astype(_F)
        part = np.concatenate([acc[:3], acc[3:6] - _F(3.0) * acc[6:]])             # (6, k, waves): a wave's a and j
        part = part.reshape(6, k, slabs, WAVES)
        slab = ((part[..., 0] + part[..., 1]) + part[..., 2]) + part[..., 3]       # (6, k, slabs), wave order
        p = np.zeros((6, k, 4), _F)
        for sl in range(slabs):                                                    # hermite_slab_sum
            p[..., sl % 4] = p[..., sl % 4] + slab[..., sl]
        total = _F(g) * ((p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3]))
        out_a[lo:lo + k] = total[:3].T
        out_j[lo:lo + k] = total[3:].T
    return out_a, out_j


def figures(got, ref, sum_abs):
    """(row_rel, F): conftest.row_rel, and F = the largest |got - ref| / (2^-24 sum|terms|) over the components; a
    component whose sum|terms| is 0 must match exactly (F = inf otherwise)."""
    from conftest import row_rel
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64); sum_abs = np.asarray(sum_abs, np.float64)
    err = np.abs(got - ref)
    pos = sum_abs > 0
    f = float((err[pos] / (U24 * sum_abs[pos])).max()) if pos.any() else 0.0
    if np.any(err[~pos] != 0) or not np.isfinite(got).all():
        f = float("inf")
    return row_rel(got, ref), f
