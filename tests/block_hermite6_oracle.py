"""fp64 numpy restatement of the block-timestep 6th-order Hermite integrator that BlockHermite6Simulator runs
(csrc/direct_hermite_block_f64.hip), built on hermite6_oracle (the pair sums, the start, the crackle) and
block_hermite_oracle (wanted_level, _margin, the level rules, the planted-binary sphere).

One output interval dt is 2^K ticks (K = max_level). Body i keeps x, v, a, j, s and the crackle c at its last correction
tick t_i and a level k_i in [0, K]; its step is d_i = 2^(K - k_i) ticks. A block step goes to t_next = min_i (t_i + d_i):
every body is predicted over its own (t_next - t_i) ticks by hermite6_oracle's Taylor series, the active ones
{i : t_i + d_i = t_next} are evaluated (a1, j1, s1) against all predicted bodies and corrected with h = d_i, c1 formed,
then re-levelled from the generalised Aarseth criterion of Nitadori & Makino (2008) for p = 6, with eta in the 4th-order
convention (dt_i = sqrt(eta ...) there):
    a5     = (720 (a1 - a0) - 360 h (j1 + j0) + 60 h^2 (s1 - s0)) / h^5
    a4(t1) = (-360 (a1 - a0) + h (168 j1 + 192 j0) + h^2 (-24 s1 + 36 s0)) / h^4 + h a5,    a3(t1) = c1
    dt_i = (eta^3 (|a1||s1| + |j1|^2) / (|c1||a5| + |a4(t1)|^2))^(1/6) = cbrt(sqrt(eta^3 num / den)),  den = 0 -> +inf
quantised and applied by block_hermite_oracle's rules. Initial levels: dt_i = (eta / 2) |a| / |j|. The start is
hermite6_oracle.start. The step constants of a body are formed exactly as hermite6_oracle.hermite6_step forms them from
its own step, so K = 0 reproduces hermite6_oracle.hermite6_run bit for bit."""
import numpy as np

import block_hermite_oracle as bo
import hermite6_oracle as h6

_norm = bo._norm


def derivatives(a0, j0, s0, a1, j1, s1, h):
    """(a3, a4, a5) at t1 of the quintic through (a, j, s) at t0 and t1 = t0 + h; h is a per-row step, (rows,) or scalar."""
    h = np.asarray(h, np.float64).reshape(-1, 1)
    da = a1 - a0
    a5 = (720.0 * da - 360.0 * h * (j1 + j0) + 60.0 * (h * h) * (s1 - s0)) / ((h * h) * (h * h) * h)
    a4 = (-360.0 * da + h * (168.0 * j1 + 192.0 * j0) + (h * h) * (-24.0 * s1 + 36.0 * s0)) / ((h * h) * (h * h)) + h * a5
    a3 = (60.0 * da - h * (36.0 * j1 + 24.0 * j0) + (h * h) * (9.0 * s1 - 3.0 * s0)) / (h * h * h)
    return a3, a4, a5


def aarseth6(a0, j0, s0, a1, j1, s1, c1, h, eta):
    """The criterion per row; h is a per-row step, c1 the crackle the corrector formed (a3 at t1)."""
    _, a4, a5 = derivatives(a0, j0, s0, a1, j1, s1, h)
    num = _norm(a1) * _norm(s1) + _norm(j1) ** 2
    den = _norm(c1) * _norm(a5) + _norm(a4) ** 2
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.where(den == 0.0, np.inf, np.cbrt(np.sqrt(eta * eta * eta * num / den)))


def _consts(h_of, ticks):
    """Per-row (h, h^2/2, h^3/6, h^4/24, h^5/120, h/2, h^2/10, h^3/120) as hermite6_oracle.hermite6_step forms them from a
    Python-float step."""
    out = np.empty((ticks.shape[0], 8))
    for t in np.unique(ticks):
        h = h_of(int(t))
        out[ticks == t] = (h, h ** 2 / 2, h ** 3 / 6, h ** 4 / 24, h ** 5 / 120, h / 2, h ** 2 / 10, h ** 3 / 120)
    return out


def _crackle(a0, j0, s0, a1, j1, s1, h_of, ticks):
    """hermite6_oracle.crackle per row, each row with the Python-float step of its tick count."""
    out = np.empty_like(a0)
    for t in np.unique(ticks):
        r = ticks == t
        out[r] = h6.crackle(a0[r], j0[r], s0[r], a1[r], j1[r], s1[r], h_of(int(t)))
    return out


def block6_run(x, v, m, dt, g, eps2, steps, eta=0.02, max_level=10):
    """`steps` output intervals from (x, v). Returns block_hermite_oracle.block_run's dict (x, v, a, j, levels, states,
    history, block_steps, pair_interactions, clamped, margin, tick_history) plus s and c."""
    K, end = max_level, 1 << max_level
    x = np.array(x, np.float64); v = np.array(v, np.float64); m = np.asarray(m, np.float64)
    n = x.shape[0]
    a, j, s, c = h6.start(x, v, m, g, eps2)
    with np.errstate(divide="ignore", invalid="ignore"):
        crit0 = np.where(_norm(j) == 0.0, np.inf, 0.5 * eta * _norm(a) / _norm(j))
    want = np.array([bo.wanted_level(q, dt, K) for q in crit0], np.int64)
    clamped = int((want > K).sum())
    margin = min([bo._margin(q, dt, K) for q in crit0] + [np.inf])
    levels = np.minimum(want, K)
    ticks = np.zeros(n, np.int64)
    history, tick_history, states = [], [], []
    block_steps = pairs = 0

    def h_of(t):
        return dt * t / end

    for _ in range(steps):
        for _ in range(end):
            d = np.left_shift(1, K - levels)
            tn = int((ticks + d).min())
            act = np.nonzero(ticks + d == tn)[0]
            p = _consts(h_of, tn - ticks)
            xp = x + v * p[:, :1] + a * p[:, 1:2] + j * p[:, 2:3] + s * p[:, 3:4] + c * p[:, 4:5]
            vp = v + a * p[:, :1] + j * p[:, 1:2] + s * p[:, 2:3] + c * p[:, 3:4]
            ap = a + j * p[:, :1] + s * p[:, 1:2] + c * p[:, 2:3]
            a1, j1, s1 = h6.accel_jerk_snap(xp, vp, ap, m, g, eps2)
            a1, j1, s1 = a1[act], j1[act], s1[act]
            a0, j0, s0 = a[act], j[act], s[act]
            q = _consts(h_of, d[act])
            v1 = v[act] + (a0 + a1) * q[:, 5:6] - (j1 - j0) * q[:, 6:7] + (s0 + s1) * q[:, 7:8]
            x1 = x[act] + (v[act] + v1) * q[:, 5:6] - (a1 - a0) * q[:, 6:7] + (j0 + j1) * q[:, 7:8]
            c1 = _crackle(a0, j0, s0, a1, j1, s1, h_of, d[act])
            x[act], v[act], a[act], j[act], s[act], c[act] = x1, v1, a1, j1, s1, c1
            crit = aarseth6(a0, j0, s0, a1, j1, s1, c1, q[:, 0], eta)
            for r, i in enumerate(act):
                w = bo.wanted_level(crit[r], dt, K)
                margin = min(margin, bo._margin(crit[r], dt, K))
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
            raise RuntimeError("block6_run: interval not finished within 2^K block steps")
        ticks[:] = 0
        states.append((x.copy(), v.copy()))
    return dict(x=x, v=v, a=a, j=j, s=s, c=c, levels=levels, states=states, history=history, block_steps=block_steps,
                pair_interactions=pairs, clamped=clamped, margin=margin, tick_history=tick_history)
