"""fp64 numpy restatement of the block-timestep Hermite integrator that BlockHermiteSimulator runs in fp32
(csrc/direct_hermite_block.hip), built on hermite_oracle.accel_jerk.

One output interval dt is 2^K ticks (K = max_level). Body i keeps x, v, a, j at its last correction tick t_i and a level
k_i in [0, K]; its step is d_i = 2^(K - k_i) ticks. A block step goes to t_next = min_i (t_i + d_i): every body is
predicted over its own (t_next - t_i) ticks, the active ones {i : t_i + d_i = t_next} are evaluated against all predicted
bodies and corrected with h = d_i, then re-levelled from the Aarseth criterion
    a3 = (12 (a0 - a1) + 6 h (j0 + j1)) / h^3,  a2 = (-6 (a0 - a1) - h (4 j0 + 2 j1)) / h^2 + h a3,
    dt_i = sqrt(eta (|a1||a2| + |j1|^2) / (|j1||a3| + |a2|^2)),
quantised to the smallest k >= 0 with dt 2^-k <= dt_i: deeper is always allowed, one level up only where t_next is a
multiple of 2 d_i, deeper than K (or NaN) is clamped to K and counted. Initial levels: dt_i = (eta / 2) |a| / |j|.
A zero denominator (j = 0 and no higher derivative, e.g. a lone body) gives dt_i = +inf: any step.
The step constants of a body are formed exactly as hermite_oracle.hermite_step forms them from its own step, so K = 0
reproduces hermite_oracle.hermite_run bit for bit."""
import numpy as np

import hermite_oracle as ho


def wanted_level(crit, dt, K):
    """Smallest k >= 0 with dt 2^-k <= crit, or K + 1 (also for NaN)."""
    k, step = 0, dt
    while k <= K and not (step <= crit):
        k += 1
        step *= 0.5
    return k


def _margin(crit, dt, K):
    """Relative distance of a criterion value from the nearest boundary dt 2^-k that decides a level (k = 0..K)."""
    if not np.isfinite(crit):
        return np.inf
    return min(abs(crit - dt * 2.0 ** -k) / (dt * 2.0 ** -k) for k in range(K + 1))


def _norm(t):
    return np.sqrt((t * t).sum(-1))


def _consts(h_of, ticks):
    """Per-row (h, h^2/2, h^3/6, h/2, h^2/12) as hermite_oracle forms them from a Python-float step."""
    out = np.empty((ticks.shape[0], 5))
    for t in np.unique(ticks):
        h = h_of(int(t))
        out[ticks == t] = (h, h * h / 2, h ** 3 / 6, h / 2, h * h / 12)
    return out


def aarseth(a0, j0, a1, j1, h, eta):
    """The criterion per row; h is a per-row step."""
    h = np.asarray(h, np.float64)[:, None]
    da = a0 - a1
    a3 = (12.0 * da + 6.0 * h * (j0 + j1)) / (h * h * h)
    a2 = (-6.0 * da - h * (4.0 * j0 + 2.0 * j1)) / (h * h) + h * a3
    num = _norm(a1) * _norm(a2) + _norm(j1) ** 2
    den = _norm(j1) * _norm(a3) + _norm(a2) ** 2
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.where(den == 0.0, np.inf, np.sqrt(eta * num / den))   # den = 0 (a lone body): any step


def block_run(x, v, m, dt, g, eps2, steps, eta=0.02, max_level=10):
    """`steps` output intervals from (x, v). Returns a dict: x, v, a, j, levels (after the last step), states (x, v after
    each output step), history (levels after every block step), block_steps, pair_interactions, clamped, margin (the
    smallest relative margin of any finite criterion value from a level boundary) and tick_history (every body's last
    correction tick after every block step, before the wrap to 0 at the end of an interval)."""
    K, end = max_level, 1 << max_level
    x = np.array(x, np.float64); v = np.array(v, np.float64); m = np.asarray(m, np.float64)
    n = x.shape[0]
    a, j = ho.accel_jerk(x, v, m, g, eps2)
    with np.errstate(divide="ignore", invalid="ignore"):
        crit0 = np.where(_norm(j) == 0.0, np.inf, 0.5 * eta * _norm(a) / _norm(j))
    want = np.array([wanted_level(c, dt, K) for c in crit0], np.int64)
    clamped = int((want > K).sum())
    margin = min([_margin(c, dt, K) for c in crit0] + [np.inf])
    levels = np.minimum(want, K)
    ticks = np.zeros(n, np.int64)
    history, tick_history, states = [], [], []
    block_steps = pairs = 0
    for _ in range(steps):
        for _ in range(end):
            d = np.left_shift(1, K - levels)
            tn = int((ticks + d).min())
            act = np.nonzero(ticks + d == tn)[0]
            c = _consts(lambda t: dt * t / end, tn - ticks)
            xp = x + v * c[:, :1] + a * c[:, 1:2] + j * c[:, 2:3]
            vp = v + a * c[:, :1] + j * c[:, 1:2]
            a1, j1 = ho.accel_jerk(xp, vp, m, g, eps2)
            a1, j1 = a1[act], j1[act]
            a0, j0 = a[act], j[act]
            ca = _consts(lambda t: dt * t / end, d[act])
            v1 = v[act] + (a0 + a1) * ca[:, 3:4] + (j0 - j1) * ca[:, 4:5]
            x1 = x[act] + (v[act] + v1) * ca[:, 3:4] + (a0 - a1) * ca[:, 4:5]
            x[act], v[act], a[act], j[act] = x1, v1, a1, j1
            crit = aarseth(a0, j0, a1, j1, ca[:, 0], eta)
            for r, i in enumerate(act):
                w = wanted_level(crit[r], dt, K)
                margin = min(margin, _margin(crit[r], dt, K))
                if w > levels[i]:
                    if w > K:
                        clamped += 1
                    levels[i] = min(w, K)
                elif w < levels[i] and tn % (2 * d[i]) == 0:
                    levels[i] -= 1
            ticks[act] = tn
            block_steps += 1
            pairs += act.size * n
            history.append(levels.copy())
            tick_history.append(ticks.copy())
            if tn == end:
                break
        else:
            raise RuntimeError("block_run: interval not finished within 2^K block steps")
        ticks[:] = 0
        states.append((x.copy(), v.copy()))
    return dict(x=x, v=v, a=a, j=j, levels=levels, states=states, history=history, block_steps=block_steps,
                pair_interactions=pairs, clamped=clamped, margin=margin, tick_history=tick_history)


def planted_binary_sphere(n=256, seed=0, sep=0.01):
    """A Plummer sphere (G = 1, total mass 1, scale radius 1, ragged masses) with its first two bodies replaced by a tight
    circular binary of separation `sep` near the centre, moving with the centre's velocity: (x, v, m)."""
    rng = np.random.default_rng(seed)
    r = 1.0 / np.sqrt(rng.uniform(0.05, 0.95, n) ** (-2.0 / 3.0) - 1.0)
    u = rng.normal(size=(n, 3))
    x = r[:, None] * u / _norm(u)[:, None]
    sig = np.sqrt(1.0 / (6.0 * np.sqrt(1.0 + r * r)))
    v = sig[:, None] * rng.normal(size=(n, 3))
    m = rng.uniform(0.5, 1.5, n)
    m /= m.sum()
    mb = m[0] + m[1]
    vc = np.sqrt(mb / sep)
    x[0] = [0.1 - sep * m[1] / mb, 0.0, 0.0]
    x[1] = [0.1 + sep * m[0] / mb, 0.0, 0.0]
    v[0] = [0.0, -vc * m[1] / mb, 0.0]
    v[1] = [0.0, vc * m[0] / mb, 0.0]
    x -= (m[:, None] * x).sum(0)
    v -= (m[:, None] * v).sum(0)
    return x, v, m
