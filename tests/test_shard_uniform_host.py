"""What the equal-mass range-sharded force tests (tests/test_shard_uniform_gpu.py) need without a GPU: the rows-only fp64
reference they compare with, pinned here to oracle.galaxify_oracle.accelerations_f64, and the argument checks of the four
fp32 shard force entries (nbd_shard_force_{local,remote}{,_uniform}_f32) on stand-in addresses, nothing launched."""
import numpy as np
import pytest

from conftest import row_rel


def _f32(x):
    return float(np.float32(x))


def rows_f64(pos, mass, g_const, eps2, lo, n_loc, rows=None):
    """fp64 acceleration of the rows [lo, lo + n_loc) (or of the index array `rows`) against all n bodies, in blocks of 256
    rows. pos and mass are rounded to fp32 and then widened (what the kernel is handed), eps2 is softening^2 as the fp32
    value the kernel is handed, the diagonal is dropped by index."""
    p = np.asarray(pos, np.float32).astype(np.float64)
    m = np.asarray(mass, np.float32).astype(np.float64)
    idx = np.arange(lo, lo + n_loc) if rows is None else np.asarray(rows)
    out = np.empty((idx.size, 3))
    for b0 in range(0, idx.size, 256):
        i = idx[b0:b0 + 256]
        d = p[None, :, :] - p[i, None, :]
        q = (d * d).sum(2) + float(eps2)
        with np.errstate(divide="ignore"):
            inv = q ** -1.5
        inv[np.arange(i.size), i] = 0.0
        out[b0:b0 + i.size] = g_const * (d * (inv * m[None, :])[:, :, None]).sum(1)
    return out


@pytest.mark.parametrize("eps", [0.1, 0.0])
def test_rows_helper_equals_the_oracle(eps):
    """rows_f64 == accelerations_f64(...)[lo:hi] to 1e-13 per row, softening 0.1 and 0, rows and sampled rows."""
    from nbd.plummer import generate_plummer
    from oracle import galaxify_oracle as go
    n, lo, n_loc = 1001, 100, 333
    p, _, m = generate_plummer(n, seed=5)
    p32, m32 = p.astype(np.float32), m.astype(np.float32)
    g, eps2 = _f32(0.7), _f32(eps ** 2)
    # the oracle squares the softening it is given: hand it the root of the fp32 eps^2 (its square is 1 ulp of fp64 away)
    want = go.accelerations_f64(p32, m32, g, np.sqrt(eps2), block=256)
    assert np.isfinite(want).all()
    assert row_rel(rows_f64(p, m, g, eps2, lo, n_loc), want[lo:lo + n_loc]) < 1e-13
    pick = np.random.default_rng(0).choice(n, 300, replace=False)
    assert row_rel(rows_f64(p, m, g, eps2, 0, 0, rows=pick), want[pick]) < 1e-13
    # rounding to fp32 is part of the helper: a perturbation below half an fp32 ulp changes nothing, the diagonal is
    # dropped by index (a coincident pair at eps = 0 would be inf, not 0)
    assert np.array_equal(rows_f64(p32.astype(np.float64) * (1 + 1e-9), m, g, eps2, lo, n_loc),
                          rows_f64(p, m, g, eps2, lo, n_loc))


def test_shard_force_argument_checks_without_a_gpu():
    """local / remote x general / uniform: bad ranges, null and misaligned arrays -> -1; null or short workspace -> the
    workspace code; n_local == 0 -> 0 with every pointer null; the uniform entry answers as the general one."""
    from nbd import _lib
    L = _lib.lib()
    E_ARG, E_WS = -1, -2
    assert b"workspace" in L.nbd_strerror(E_WS).lower()
    A, S = 0x10000, 0x20000                                     # aligned stand-ins: nothing is launched
    big = 1 << 30
    n, lo, n_loc = 100, 10, 50
    full = L.nbd_shard_workspace_bytes(n, lo, n_loc)
    assert full > 0

    def local(uni, posm=S, n_local=n_loc, ws=A, ws_bytes=big, n_total=n, lo_=lo):
        fn = L.nbd_shard_force_local_uniform_f32 if uni else L.nbd_shard_force_local_f32
        return fn(posm, n_local, 0.01, ws, ws_bytes, n_total, lo_, None)

    def remote(uni, posm_all=S, n_total=n, posm_local=S, n_local=n_loc, lo_=lo, acc=A, vel=None, ws=A, ws_bytes=big):
        if uni:
            return L.nbd_shard_force_remote_uniform_f32(posm_all, n_total, posm_local, n_local, lo_, 0.01, 1.0, 0.01, acc,
                                                        vel, 0.0, ws, ws_bytes, None)
        return L.nbd_shard_force_remote_f32(posm_all, n_total, posm_local, n_local, lo_, 0.01, 1.0, acc, vel, 0.0, ws,
                                            ws_bytes, None)

    local_cases = ((dict(lo_=60), E_ARG), (dict(lo_=-1), E_ARG), (dict(n_local=-1), E_ARG), (dict(posm=None), E_ARG),
                   (dict(posm=S + 8), E_ARG), (dict(ws=None), E_WS), (dict(ws_bytes=full - 1), E_WS),
                   (dict(posm=None, n_local=0, ws=None, ws_bytes=0), 0))
    remote_cases = ((dict(lo_=60), E_ARG), (dict(lo_=-1), E_ARG), (dict(n_local=-1), E_ARG), (dict(posm_all=None), E_ARG),
                    (dict(posm_all=S + 8), E_ARG), (dict(posm_local=None), E_ARG), (dict(posm_local=S + 8), E_ARG),
                    (dict(acc=None), E_ARG), (dict(ws=None), E_WS), (dict(ws_bytes=full - 1), E_WS),
                    (dict(posm_all=None, posm_local=None, n_local=0, acc=None, ws=None, ws_bytes=0), 0))
    for fn, cases in ((local, local_cases), (remote, remote_cases)):
        for change, rc in cases:
            got = fn(False, **change), fn(True, **change)
            assert got == (rc, rc), (fn.__name__, change, got)
