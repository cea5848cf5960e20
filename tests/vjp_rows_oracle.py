"""What the tests of the two fp32 force backward kernels at chunk edges and long chunk walks share
(test_vjp_walk_host.py, test_vjp_walk_gpu.py): the inputs, the row sample, the fp64 gradients of a few target rows under
all n sources with the sum of |terms| of every component -- the arithmetic of accel_vjp_oracle.py and
accel_jerk_vjp_oracle.py, which take the rows -- and a plain float32 evaluation of the same rows in the kernels'
summation order, the yardstick an fp32 kernel is held to. Plain numpy, no GPU.

The kernels restated. nbd_accel_vjp_f32 (csrc/direct_grad.hip, AccelVjpPolicy) and nbd_accel_jerk_vjp_f32
(csrc/direct_hermite_grad.hip, AccelJerkVjpPolicy, three streamed rows) are accel_jerk_body (csrc/hermite_kernels.h) with
another pair policy and the plan of the forward force: the walk of hermite_rows_oracle's module text, wave
jw = 4 slab + wave over the chunks [jw q + min(jw, r), ... + q + (jw < r)). Per wave TWO sets of sums, one for the even
sources and one for the odd, every sum one sequential fp32 chain of fused multiply-adds; a wave's outputs are formed from
the two sets as the policy's out() forms them; the four waves of a slab are added in wave order, the slabs as
hermite_slab_sum adds them, G is applied once, the mass gradient takes its sign after that, and the jerk backward adds
the acceleration backward's finished result (the alpha part) last. Per pair: fp32 differences of the fp32 inputs,
h = m_i c_j - m_j c_i by one product and one fused multiply-add, every dot product one product and two fused multiply-adds.
The one stated difference from the kernels: 1 / sqrt is correctly rounded here. The kernels take v_rsq_f32 (1 ulp), and the
jerk backward refines it by a Newton step, which is not modelled. A fused multiply-add is hermite_rows_oracle._fma: the
exact product plus the sum in fp64, rounded to fp32."""
import numpy as np

import accel_jerk_vjp_oracle as jo
import accel_vjp_oracle as vo
import hermite_rows_oracle as hr

CHUNK, WAVES, GROUP = hr.CHUNK, hr.WAVES, hr.GROUP
FULL_SAMPLE_UP_TO = 11649                  # above: the reduced row sample
_F = np.float32
_fma = hr._fma
MARGIN, ROW_BAR = 4, 1e-4                 # the sampled-row bars: F <= 4 F_yardstick, row_rel <= max(1e-4, 4 row_rel_yardstick)
# The all-rows net of the long sizes around the fp64 kernel: row_rel of dL/dx (and dL/dv), global_rel of dL/dm. Ten times
# what the yardstick gives over ALL rows of n = 5633 against the fp64 rows (the larger of eps = 0.05 and eps = 0),
# rounded up to one digit: acceleration backward 1.69e-5, 2.19e-7; jerk backward 4.27e-6, 7.81e-6, 2.93e-7 (NOTES.md,
# "T-VJPWALK"). test_vjp_walk_host.py holds each below a quarter of what one dropped chunk shifts at n = 32193.
NET_ACCEL = (2e-4, 3e-6)
NET_JERK = (5e-5, 8e-5, 3e-6)
_PAIRS = 1 << 16                          # row-source pairs of one block of the yardstick (the arrays it holds at once)


def case(n):
    """(x, v, m, cota, cotj) in fp64, every value fp32-representable: the fp32 case n of test_accel_vjp_gpu.py (x, m,
    cota) and test_accel_jerk_vjp_gpu.py, and the (x, v, m) of hermite_rows_oracle.case."""
    return jo.case(n, seed=200 + n, fp32=True)


def sample_rows(n):
    """hermite_rows_oracle.sample_rows up to n = 11649; above, the first target group of 128, the whole last (ragged)
    group and 32 seeded random rows, sorted, no row twice (the fp64 rows of the jerk backward cost 0.5 us per pair)."""
    if n <= FULL_SAMPLE_UP_TO:
        return hr.sample_rows(n)
    groups = -(-n // GROUP)
    rnd = np.random.default_rng(n).choice(n, 32, replace=False)
    return np.unique(np.concatenate([np.arange(GROUP), np.arange((groups - 1) * GROUP, n), rnd]))


def accel_vjp_rows(x, m, cot, g, eps2, rows):
    """(dL/dx (k,3), dL/dm (k,), sum|terms| of dL/dx, of dL/dm) in fp64 of the target rows `rows` under all n sources,
    the self term dropped by index: accel_vjp_oracle.accel_vjp on those rows."""
    return vo.accel_vjp_of_rows(x, m, cot, g, eps2, None, rows)


def accel_jerk_vjp_rows(x, v, m, cota, cotj, g, eps2, rows):
    """(dL/dx (k,3), dL/dv (k,3), dL/dm (k,), sum|terms| of each) in fp64 of the target rows `rows` under all n sources:
    accel_jerk_vjp_oracle.accel_jerk_vjp on those rows. cota or cotj None: that cotangent is zero."""
    return jo.accel_jerk_vjp_of_rows(x, v, m, cota, cotj, g, eps2, None, rows)


# ---------------------------------------------------------------- the float32 yardsticks
def _walk(plan, chunk_order):
    """(at, live), each (waves, steps): the source index of step t of wave jw's chain, and whether the wave has that step
    (a wave one chunk shorter than the longest adds zeros there). chunk_order: the physical chunk at every place of the
    walk (None: the chunks as they are)."""
    chunks, waves = plan["chunks"], WAVES * plan["slabs"]
    q, r = hr.split(plan)
    jw = np.arange(waves)
    length = q + (1 if r else 0)
    live = np.arange(length)[None, :] < (q + (jw < r))[:, None]
    place = np.where(live, (jw * q + np.minimum(jw, r))[:, None] + np.arange(length)[None, :], 0)
    assert place.max() < chunks and np.array_equal(np.sort(place[live]), np.arange(chunks))      # every chunk once
    pc = place if chunk_order is None else np.asarray(chunk_order)[place]
    at = (pc[:, :, None] * CHUNK + np.arange(CHUNK)[None, None, :]).reshape(waves, length * CHUNK)
    return at, np.repeat(live, CHUNK, axis=1)


def _chains(prod, at, live):
    """prod (K, k, npad) float64, the exact products of the K fused multiply-adds of every pair -> (2, K, k, waves)
    float32: every wave's even-source and odd-source sums, each one sequential chain acc = fl32(product + acc) (_fma
    with its product already formed). A chunk starts at a multiple of 64, so step t is an even source when t is even."""
    seq = np.ascontiguousarray(np.where(live[None, None], prod[:, :, at], 0.0).transpose(3, 0, 1, 2))
    acc = np.zeros((2,) + seq.shape[1:], _F)
    for t in range(seq.shape[0]):
        acc[t & 1] = (seq[t] + acc[t & 1]).astype(_F)
    return acc


def _reduce(part, slabs):
    """part (K, k, waves) float32, a wave's outputs -> (K, k): the four waves of a slab in wave order, then the slabs as
    hermite_slab_sum and the two finishing kernels add them."""
    part = part.reshape(part.shape[:2] + (slabs, WAVES))
    slab = ((part[..., 0] + part[..., 1]) + part[..., 2]) + part[..., 3]
    p = np.zeros(part.shape[:2] + (4,), _F)
    for sl in range(slabs):
        p[..., sl % 4] = p[..., sl % 4] + slab[..., sl]
    return (p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])


def _dot(a, b):
    return _fma(a[2], b[2], _fma(a[1], b[1], a[0] * b[0]))


class _Blocks:
    """The row blocks of a yardstick: the padded float32 sources, and per block of target rows the differences d, r^2
    and the masked correctly rounded s = 1 / sqrt(r^2) (0 for the target itself, the padding behind n and the sources
    of `drop_chunk`)."""

    def __init__(self, x, m, eps2, rows, plan, chunk_order, drop_chunk, *more):
        self.n, self.plan = np.asarray(x).shape[0], plan
        assert plan["chunks"] == -(-self.n // CHUNK) and plan["slabs"] >= 1
        self.npad = plan["chunks"] * CHUNK
        self.x, self.m = self.pad(x), self.pad(m)
        self.more = [self.pad(t) for t in more]
        self.rows = np.asarray(rows, np.int64)
        self.e2 = np.full((), eps2, _F)
        self.at, self.live = _walk(plan, chunk_order)
        self.dropped = np.arange(self.npad) >= self.n
        if drop_chunk is not None:
            self.dropped[drop_chunk * CHUNK:(drop_chunk + 1) * CHUNK] = True
        self.step = max(1, _PAIRS // self.npad)

    def pad(self, t):
        t = np.asarray(t, _F)
        out = np.zeros((self.npad,) + t.shape[1:], _F)
        out[:self.n] = t
        return out

    def __iter__(self):
        for lo in range(0, self.rows.size, self.step):
            rr = self.rows[lo:lo + self.step]
            d = [self.x[None, :, c] - self.x[rr, None, c] for c in range(3)]       # float32 differences, (k, npad)
            r2 = _fma(d[2], d[2], _fma(d[1], d[1], _fma(d[0], d[0], self.e2)))
            with np.errstate(divide="ignore"):
                s = (1.0 / np.sqrt(r2.astype(np.float64))).astype(_F)             # correctly rounded (to a double rounding)
            s[np.broadcast_to(self.dropped, s.shape)] = 0.0
            s[np.arange(rr.size), rr] = 0.0
            yield slice(lo, lo + rr.size), rr, d, s

    def sums(self, fac, elem):
        """The chains of the fused multiply-adds acc = fma(fac[i], elem[i], acc): (2, K, k, waves) float32."""
        prod = np.stack([f.astype(np.float64) * e.astype(np.float64) for f, e in zip(fac, elem)])
        return _chains(prod, self.at, self.live)


def _h(mi, cj, mj, ci):
    """h = m_i c_j - m_j c_i by component: one product and one fused multiply-add (h_of of both policies)."""
    return [_fma(mi, cj[c], -(mj * ci[c])) for c in range(3)]


def yardstick_accel_vjp_rows(x, m, cot, g, eps2, rows, plan, chunk_order=None, drop_chunk=None):
    """(dL/dx (k,3), dL/dm (k,)) float32: nbd_accel_vjp_f32 restated (the module text) for the target rows `rows`, with
    the chunk split of plan = {groups, slabs, chunks}. chunk_order: a permutation of the chunks, the walk takes chunk
    chunk_order[c] where it would take c (another order of the same terms). drop_chunk: a physical chunk whose sources
    are left out (a mutation, for the tests of the bars)."""
    b = _Blocks(x, m, eps2, rows, plan, chunk_order, drop_chunk, cot)
    gs, = b.more
    gp = np.zeros((b.rows.size, 3), _F); gm = np.zeros(b.rows.size, _F)
    for sl, rr, d, s in b:
        mi, mj = b.m[rr, None], b.m[None, :]
        gj = [gs[None, :, c] for c in range(3)]
        h = _h(mi, gj, mj, [gs[rr, None, c] for c in range(3)])
        dh, dg = _dot(d, h), _dot(d, gj)
        s2 = s * s
        s3 = s2 * s
        c5 = (dh * s2) * s3
        acc = b.sums([s3] * 3 + [c5] * 3 + [s3], h + d + [dg])
        a = acc[0] + acc[1]                                                       # out(): the two sets, then the outputs
        part = np.concatenate([a[:3] - _F(3.0) * a[3:6], a[6:]])
        total = _reduce(part, plan["slabs"])
        gp[sl] = (_F(g) * total[:3]).T
        gm[sl] = _F(0.0) - _F(g) * total[3]
    return gp, gm


def yardstick_accel_jerk_vjp_rows(x, v, m, cota, cotj, g, eps2, rows, plan, chunk_order=None, drop_chunk=None):
    """(dL/dx (k,3), dL/dv (k,3), dL/dm (k,)) float32: nbd_accel_jerk_vjp_f32 restated for the target rows `rows`; the
    arguments of yardstick_accel_vjp_rows. cota given: the acceleration backward's finished result is added last, or, with
    cotj None, is the result (dL/dv = 0)."""
    k = np.asarray(rows).size
    alpha = None if cota is None else yardstick_accel_vjp_rows(x, m, cota, g, eps2, rows, plan, chunk_order, drop_chunk)
    if cotj is None:
        return alpha[0], np.zeros((k, 3), _F), alpha[1]
    b = _Blocks(x, m, eps2, rows, plan, chunk_order, drop_chunk, v, cotj)
    vs, bs = b.more
    gp = np.zeros((k, 3), _F); gv = np.zeros((k, 3), _F); gm = np.zeros(k, _F)
    for sl, rr, d, s in b:
        mi, mj = b.m[rr, None], b.m[None, :]
        w = [vs[None, :, c] - vs[rr, None, c] for c in range(3)]
        bj = [bs[None, :, c] for c in range(3)]
        h = _h(mi, bj, mj, [bs[rr, None, c] for c in range(3)])
        dh, dw, hw, db, bw = _dot(d, h), _dot(d, w), _dot(h, w), _dot(d, bj), _dot(bj, w)
        s2 = s * s
        s3 = s2 * s
        s5 = s3 * s2
        cdh, cdw = s5 * dh, s5 * dw
        e = _fma(_F(-5.0) * (s2 * dw), dh, hw)
        t = [_fma(e, d[c], _fma(dh, w[c], dw * h[c])) for c in range(3)]
        acc = b.sums([s3] * 3 + [cdh] * 3 + [s5] * 3 + [s3, cdw], h + d + t + [bw, db])
        a = acc[0] + acc[1]
        part = np.concatenate([_F(-3.0) * a[6:9], a[:3] - _F(3.0) * a[3:6], a[9:10] - _F(3.0) * a[10:11]])
        total = _F(g) * _reduce(part, plan["slabs"])
        gp[sl], gv[sl], gm[sl] = total[:3].T, total[3:6].T, _F(0.0) - total[6]
    if alpha is not None:
        gp, gm = gp + alpha[0], gm + alpha[1]
    return gp, gv, gm


def figures(got, ref, sum_abs):
    """hermite_rows_oracle.figures, a mass gradient (k,) held as (k, 1)."""
    got, ref, sum_abs = (np.asarray(t) for t in (got, ref, sum_abs))
    if ref.ndim == 1:
        got, ref, sum_abs = got[:, None], ref[:, None], sum_abs[:, None]
    return hr.figures(got, ref, sum_abs)
