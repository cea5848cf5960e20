"""Deterministic inputs and bars of the ContinuousConv pin (tests/golden/surrogate_ref_contconv_forward*.npz), shared by the
generator (tests/golden/make_golden_surrogate.py: contconv_forward_vectors) and by the host and GPU tests.

Every value is an integer hash on uint64 (wrap-around multiply / xor-shift, numpy integer arithmetic only: no RNG whose
stream could change between versions) mapped to a dyadic lattice:

  pos      multiples of 1/64 with |x| <= 4. Every pos[col] - pos[row] is a multiple of 1/64 with |.| <= 8 and every dist2 a
           multiple of 1/4096 below 192 < 2^24 / 4096: both EXACT in fp32, so the inside-the-radius decision is the same in
           the reference's fp32 run, its fp64 run and the kernels, and no case depends on a rounding of dist2. (For r = 0.8
           no lattice value lies between fp32(0.64) and 0.64.) Two tight clusters (offsets within +-1/4 of a centre: every
           member inside r = 1 of every other) hold 5/8 of the bodies, three quarters of those the first, so the
           radius-graph in-degrees reach the cap there; the rest is spread over the whole cube and has 0-2 neighbours.
  feat, filters, dout   multiples of 2^-8 in [-2, 2]: exact in fp32 and fp64. The filters (14 MB at D = 6, 128 -> 128) are
           regenerated, never stored; the fixture holds a sha256 of every input array's bytes.

Special bodies: 1 coincides with 0 (r = 0 off the diagonal); where the radius lies on the lattice (0.5, 1.0, 3.0) body 3 sits
at exactly dist2 == radius ** 2 from body 2 (strictly-less-than: outside).

Edge list of a case (edges()): oracle radius_graph(loop, cap) + n // 4 extra directed edges (the exact-radius pair in both
directions first, the others hashed: most of them beyond the radius) + two exact duplicates of radius-graph edges, all in a
fixed hashed permutation, so rows are not sorted by target. Row 0 = aggregation target, row 1 = feature source."""
import glob
import hashlib
import os

import numpy as np

_M = np.uint64(0xFFFFFFFFFFFFFFFF)

#        n    D  I    O    agg     radius cap  loop
CASES = {
    "f0": (160, 2, 1, 5, "sum", 1.0, 32, True),        # I % 4 != 0, one product per output
    "f1": (160, 6, 128, 128, "mean", 1.0, 32, True),   # published layer 1 shape
    "f2": (160, 4, 128, 128, "mean", 1.0, 32, True),   # published layer 2 shape
    "f3": (128, 3, 70, 40, "sum", 0.8, 32, True),      # radius ** 2 not exact in fp32, odd D, padded channels
    "f4": (96, 5, 4, 130, "sum", 3.0, 200, True),      # uncapped, samples near the grid faces, O off the matrix tile
    "f5": (128, 4, 32, 64, "mean", 0.5, 32, True),     # the reference's default radius
    "f6": (128, 4, 8, 16, "max", 1.0, 32, False),      # no self loops: rows without edges
    "g0": (96, 2, 1, 5, "sum", 1.0, 32, True),         # gradients
    "g1": (96, 4, 8, 16, "mean", 1.0, 32, True),       # gradients, fused training path
    "g2": (96, 3, 12, 20, "sum", 0.8, 32, True),       # gradients
}
F_CASES = [c for c in CASES if c.startswith("f")]
G_CASES = [c for c in CASES if c.startswith("g")]
GRAD_CASES = G_CASES + ["f2"]            # f2: feature gradient only (its filter gradient is 8 MB)
LISTS_CASES = ["f1", "f2", "f5"]         # also pinned on the pure radius graph (out64_lists)
EXACT_RADIUS = (0.5, 1.0, 3.0)           # radii that lie on the 1/64 lattice
TOL = 1e-5                               # the project's bar: global_rel < TOL, row_rel < 10 * TOL
FACTOR = 4.0                             # two bits over the reference's own fp32 error (floor: one fp32 unit, 2^-23)


def _hash(count, salt):
    """uint64[count]: splitmix64's finaliser over salt * 2^32 + index."""
    with np.errstate(over="ignore"):
        z = (np.arange(count, dtype=np.uint64) + np.uint64(salt) * np.uint64(1 << 32) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return (z ^ (z >> np.uint64(31))) & _M


def _salt(case, what):
    return (list(CASES).index(case) + 1) * 16 + what


def _dyadic(shape, salt):
    """float32, multiples of 2^-8 in [-2, 2]."""
    k = (_hash(int(np.prod(shape)), salt) % np.uint64(1025)).astype(np.int64) - 512
    return (k.astype(np.float32) / np.float32(256.0)).reshape(shape)


_CENTRES = np.array([[-128, 96, 32], [80, -64, 112]], dtype=np.int64)        # in units of 1/64


def _positions(case):
    n, radius = CASES[case][0], CASES[case][5]
    k = np.empty((n, 3), dtype=np.int64)
    h = _hash(3 * n, _salt(case, 0)).reshape(n, 3)
    dense = (5 * n) // 8
    k[:dense] = _CENTRES[(np.arange(dense) % 4 == 3).astype(np.int64)] + (h[:dense] % np.uint64(33)).astype(np.int64) - 16
    k[dense:] = (h[dense:] % np.uint64(513)).astype(np.int64) - 256
    k[1] = k[0]                                                             # coincident pair
    if radius in EXACT_RADIUS:
        k[3] = k[2] + np.array([int(radius * 64), 0, 0])                    # dist2 == radius ** 2 exactly
    assert np.abs(k).max() <= 256
    return (k.astype(np.float32) / np.float32(64.0))


def inputs(case):
    """pos [n, 3], feat [n, I], filters [D, D, D, I, O], dout [n, O]: float32, C-contiguous."""
    n, d, i, o = CASES[case][:4]
    return {"pos": _positions(case), "feat": _dyadic((n, i), _salt(case, 1)),
            "filters": _dyadic((d, d, d, i, o), _salt(case, 2)), "dout": _dyadic((n, o), _salt(case, 3))}


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def edges(case, pos):
    """(edge_index int32 [2, E], radius_at int32 [E0]): the case's edge list and where its radius-graph edges sit in it, in
    radius_graph's own order (edge_index[:, radius_at] IS the radius graph)."""
    import torch
    from oracle import surrogate_oracle as so
    n, _, _, _, _, radius, cap, loop = CASES[case]
    rg = so.radius_graph(torch.from_numpy(pos), radius, loop=loop, max_num_neighbors=cap).numpy().astype(np.int64)
    e0, extra = rg.shape[1], n // 4
    h = _hash(2 * extra + 2, _salt(case, 4))
    add = (h[:2 * extra] % np.uint64(n)).astype(np.int64).reshape(2, extra)
    if radius in EXACT_RADIUS:
        add[:, 0], add[:, 1] = (2, 3), (3, 2)
    dup = rg[:, (h[2 * extra:] % np.uint64(e0)).astype(np.int64)]
    ei = np.concatenate([rg, add, dup], axis=1)
    perm = np.argsort(_hash(ei.shape[1], _salt(case, 5)), kind="stable")
    where = np.empty(ei.shape[1], dtype=np.int64)
    where[perm] = np.arange(ei.shape[1])
    return ei[:, perm].astype(np.int32), where[:e0].astype(np.int32)


_FIXTURE = None


def fixture():
    """Every array of tests/golden/surrogate_ref_contconv_forward*.npz, keyed "<case>_<name>" (loaded once)."""
    global _FIXTURE
    if _FIXTURE is None:
        out = {}
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        for path in sorted(glob.glob(os.path.join(here, "surrogate_ref_contconv_forward*.npz"))):
            with np.load(path, allow_pickle=False) as z:
                out.update({k: z[k] for k in z.files})
        for v in out.values():
            v.setflags(write=False)
        _FIXTURE = out
    return _FIXTURE


def checked_inputs(case):
    """inputs(case) after asserting that they hash to the digests the fixture stores, plus the stored edge list (int64)."""
    fx, inp = fixture(), inputs(case)
    for name, a in inp.items():
        assert a.dtype == np.float32 and digest(a) == str(fx[f"{case}_sha_{name}"]), (case, name)
    inp["edge_index"] = fx[f"{case}_edge_index"].astype(np.int64)
    return inp


def ratios(got, case, what="out"):
    """(global_rel, row_rel) of `got` against the fp64 fixture `what`, each divided by max(the reference's own fp32 figure,
    2^-23), and the two raw figures."""
    from conftest import global_rel, row_rel
    fx = fixture()
    ref = np.tanh(fx[f"{case}_out64"]) if what == "tanh" else fx[f"{case}_{what}64"]
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    g, r = global_rel(got, ref), row_rel(got, ref)
    floor = 2.0 ** -23
    return (g / max(float(fx[f"{case}_{what}_ref32_global"]), floor), r / max(float(fx[f"{case}_{what}_ref32_row"]), floor), g, r)


def check(got, case, what="out", label=""):
    """The bars of the pin: the project's own (global_rel < 1e-5, row_rel < 1e-4) and four times the reference's own fp32 error
    against its fp64 run. Prints the measured figures before it asserts."""
    qg, qr, g, r = ratios(got, case, what)
    print(f"contconv-pin {case} {what} {label}: global_rel {g:.3e} ({qg:.2f} x ref32)  row_rel {r:.3e} ({qr:.2f} x ref32)")
    assert g < TOL and r < 10 * TOL, (case, what, label, g, r)
    assert qg <= FACTOR and qr <= FACTOR, (case, what, label, qg, qr)
    return qg, qr
