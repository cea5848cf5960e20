"""What a build of csrc/tree_force.hip leaves -- the order, the sorted bodies, every node record, read through
nbd.tree.views() -- against its specification (tests/tree_build_oracle.py), and walks of inputs off the Plummer path: bodies
on a line and in a plane, a far outlier that ties most keys, masses over six decades with whole massless nodes, opening
angles from 0.05 to 1.5, and theta > 0 where the 8 waves of a group divide the tree at level 2. Every build and every
reference is made once per module."""
import numpy as np
import pytest
import torch

import tree_build_oracle as tbo
import tree_oracle as to
import tree_potential_oracle as tpo

pytestmark = pytest.mark.gpu

EPS2 = to.SOFTENING ** 2
U = 2.0 ** -24                       # the relative rounding of one fp32 operation
BUILT = tbo.WALKED + ["deep"] + tbo.BUILD_ONLY
CHECKED = [name for name in BUILT if name != "nan"]          # the NaN input is checked for its order only, never walked

# Acceleration rows: |a_gpu - a_ref| <= MARGIN U (K_PAIR S_pair + K_CELL S_cell), S the oracle's condition sums
# (tree_oracle.tree_accel(cond=True)): the norms of the pair terms and of the three vectors of every accepted cell. The
# counts are of the roundings of tree_walk_kernel, each in units of U relative to the addend (or to a partial sum, which
# the condition sum bounds), worst case added up:
#   pair term     d = p - x: 1.  r2 = eps2 + dx^2 + dy^2 + dz^2, 3 FMAs: 3, + 2 from the squares of d: 5.  s = v_rsq_f32
#                 (1 ulp = 2 U) of it: 2 + 5/2 = 4.5.  w = m ((s s) s): 3 x 4.5 + 3 = 16.5.  w d: + 1 = 17.5.
#   node sum      the FMA chain over the 8 bodies of a level-0 node: 8.
#   outer sums    add_comp (compensated, over nodes and passes): 2.  The 8 slabs of a split group, plain adds: 7.  g: 1.
#   K_PAIR = 17.5 + 8 + 2 + 7 + 1 = 35.5 -> 36
#   cell term     r = c - x: 1, + 1 for c stored as fp32 (relative to |c|, counted as if to |r|): 2.  r2: 3 + 4 = 7.
#                 u = rsq: 2 + 3.5 = 5.5.  u2: 12.  u3: 18.5.  u5 = u3 u2: 31.5.  u7 = u5 u2: 44.5.
#                 M u3 (M stored: 1): 20.5, the FMA that adds the quadrupole's share of w: 1, times r: 2 -> 23.5.
#                 q = Q r (Q stored: 1, r: 2, 3 roundings): 6; u5 q: 37.5.  r.q: 6 + 2 + 3 = 11; 2.5 (r.q): 12; times u7:
#                 56.5; the FMA: 1; times r: 2 -> 59.5, the largest of the three vectors.
#   pass sum      the FMA chain of flush_cells, 2 FMAs per cell and component, at most 95 cells in a pass (a list is
#                 flushed at >= 64 entries and grows by <= 32 per iteration): 190.
#   K_CELL = 59.5 + 190 + 2 + 7 + 1 = 259.5 -> 260
# A row without an accepted cell (theta = 0.05 on the small inputs) is held to 2 x 36 U = 4.3e-6 of its condition sum.
K_PAIR, K_CELL, MARGIN = 36, 260, 2
# Potential rows at theta = 0.05, where (almost) nothing is accepted and the sum has one sign: 6 roundings of the pair
# term, an fp32 chain of at most 7 adds, the fp32 -> fp64 step, margin 2 -- test_tree_potential_gpu.PHI_TOL.
PHI_TOL = 16 * U

_cache = {}


def _np(t):
    return t.detach().cpu().numpy()


def _rms(e):
    return float(np.sqrt((e ** 2).mean())) if e.size else 0.0


def _ratio(err, bound):
    """The largest err / bound; an error where the bound is 0 is infinite, 0 / 0 is 0."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def _built(name, how="build"):
    """One build per input and entry: the workspace, the returned order and the three regions as numpy arrays."""
    if (name, how) not in _cache:
        from nbd import tree
        p, m = tbo.inputs(name)
        n = len(p)
        ws = tree.workspace(n, "cuda")
        ws.fill_(0xA5)                                        # whatever the workspace held: no region depends on it
        if how == "build":
            order = tree.build(torch.tensor(p).cuda(), torch.tensor(m).cuda(), ws)
        else:
            rows = torch.tensor(np.concatenate([p, m[:, None]], axis=1)).cuda()
            order = tree.build_posm(rows, n, ws)
        v = tree.views(ws, n)
        assert v["order"].data_ptr() > ws.data_ptr() and v["nodes"][0].data_ptr() > v["posm"].data_ptr()   # views, no copies
        _cache[(name, how)] = dict(ws=ws, n=n, order=_np(order), v_order=_np(v["order"]), posm=_np(v["posm"]),
                                   nodes=[_np(t) for t in v["nodes"]])
    return _cache[(name, how)]


# ---------------------------------------------------------------- a. the order

@pytest.mark.parametrize("how", ["build", "build_posm"])
@pytest.mark.parametrize("name", BUILT)
def test_order_is_the_stable_order_of_the_restated_keys(name, how, gpu_device):
    b = _built(name, how)
    p = tbo.inputs(name)[0]
    keys, want = tbo.keys_f32(p), tbo.order_f32(p)
    order = b["order"].astype(np.int64)
    assert b["order"].dtype == np.int32 and np.array_equal(b["order"], b["v_order"])
    assert sorted(order.tolist()) == list(range(len(p)))
    along = keys[order].astype(np.int64)                      # 63-bit keys
    exact = np.array_equal(order, want)
    print(f"{name} ({how}): order equals the stable order of the restated keys: {exact}; "
          f"{int((np.diff(along) == 0).sum())} ties among {len(p)} bodies")
    # the weaker property first: restated keys never decrease along the order, ties in ascending index
    assert (np.diff(along) >= 0).all() and (np.diff(order)[np.diff(along) == 0] > 0).all()
    assert exact, np.flatnonzero(order != want)[:16]


# ---------------------------------------------------------------- b. the sorted bodies

@pytest.mark.parametrize("name", CHECKED)
def test_sorted_bodies_are_the_gathered_rows_bit_for_bit(name, gpu_device):
    b, (p, m) = _built(name), tbo.inputs(name)
    n, order = b["n"], b["order"]
    posm = b["posm"]
    assert posm.shape == ((n + 63) // 64 * 64, 4) and posm.dtype == np.float32
    want = np.concatenate([p[order], m[order][:, None]], axis=1)
    assert np.array_equal(posm[:n].view(np.uint32), want.view(np.uint32))
    assert (posm[n:].view(np.uint32) == 0).all()
    other = _built(name, "build_posm")
    assert np.array_equal(other["order"], order) and np.array_equal(other["posm"].view(np.uint32), posm.view(np.uint32))
    assert len(other["nodes"]) == len(b["nodes"])
    for mine, theirs in zip(b["nodes"], other["nodes"]):
        assert np.array_equal(mine.view(np.uint32), theirs.view(np.uint32))


# ---------------------------------------------------------------- c. the node records

@pytest.mark.parametrize("name", CHECKED)
def test_node_records_against_the_fp64_nodes(name, gpu_device):
    """Every node of every level against tree_oracle.build_nodes on the GPU's own sorted bodies, within the bounds of
    tree_build_oracle.node_tolerances (derived there from finish_node; margin 2). s may not be too SMALL by more than
    its bound either: that is the direction that accepts cells it should open."""
    b = _built(name)
    n = b["n"]
    x, m = b["posm"][:n, :3].astype(np.float64), b["posm"][:n, 3].astype(np.float64)
    ref = to.build_nodes(x, m)
    tol = tbo.node_tolerances(x, m, tbo.box_f32(tbo.inputs(name)[0])[3])
    assert [len(t) for t in b["nodes"]] == to.plan(n)[2]
    worst = dict(M=0.0, c=0.0, s=0.0, Q=0.0)
    failures = []
    for lvl, (rec, L, T) in enumerate(zip(b["nodes"], ref, tol)):
        M, c, s, Q = tbo.unpack_nodes(rec)
        assert np.isfinite(rec).all() and (rec[:, 11] == 0).all()
        massless = L["M"] == 0
        assert (M[massless] == 0).all() and (rec[massless, 5:11] == 0).all()
        err = dict(M=np.abs(M - L["M"]), c=np.abs(c - L["c"]), s=np.abs(s - L["s"]),
                   Q=np.linalg.norm(Q - L["Q"], axis=(1, 2)))
        for k in worst:
            worst[k] = max(worst[k], _ratio(err[k], T[k]))
            if not (err[k] <= T[k]).all():
                failures.append((lvl, k, np.flatnonzero(~(err[k] <= T[k]).reshape(len(M), -1).all(1))[:8].tolist()))
        if not (s >= L["s"] - T["s"]).all():
            failures.append((lvl, "s too small", np.flatnonzero(s < L["s"] - T["s"])[:8].tolist()))
    print(f"{name}: largest error / bound over {sum(len(t) for t in b['nodes'])} nodes: "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not failures, failures


# ---------------------------------------------------------------- d. walks off the Plummer path

def _direct(name):
    if ("direct", name) not in _cache:
        p, m = tbo.inputs(name)
        _cache[("direct", name)] = (to.direct_accel(p, m, to.SOFTENING), tpo.direct_potential(p, m, to.SOFTENING))
    return _cache[("direct", name)]


def _acc_bound(S):
    return MARGIN * U * (K_PAIR * S[:, 0] + K_CELL * S[:, 1])


@pytest.mark.parametrize("theta,quadrupole", [(0.05, True), (0.5, True), (0.5, False), (1.5, True)])
@pytest.mark.parametrize("name", tbo.WALKED)
def test_walk_off_the_plummer_path(name, theta, quadrupole, gpu_device):
    """a and phi from ONE walk against the oracle on the GPU's order. Counters EQUAL (a float32 opening test flips no
    decision on these inputs: test_tree_build_host.py). Every acceleration row within MARGIN U (K_PAIR S_pair + K_CELL
    S_cell), K_PAIR = 36, K_CELL = 260, MARGIN = 2 (the counts, rounding by rounding, stand at the head of this file:
    17.5 for a pair term, 59.5 for a cell term with quadrupole, 8 and 190 for the fp32 chains of a node and of a list pass,
    2 + 7 + 1 for the compensated sums, the 8 slabs and G) -- not within 3e-6 of its norm: the forces on a body in the middle
    of a line or a sheet cancel, and an honest fp32 sum may miss that. Every potential row within PHI_TOL at theta = 0.05
    and within 3e-6 |phi_ref| elsewhere (one sign, no cancellation). Against the fp64 direct sums: no worse than twice the
    oracle's own error (+ 3e-6); at theta = 1.5 that error is of order 1 on line and sheet, which is the specification."""
    from nbd import tree
    b, (p, m) = _built(name), tbo.inputs(name)
    n, order = b["n"], b["order"]
    counters = torch.zeros(2, dtype=torch.int64, device="cuda")
    acc, phi = tree.accel_potential(b["ws"], n, theta, EPS2, 1.0, quadrupole, counters=counters)
    acc, phi, counters = _np(acc), _np(phi), tuple(counters.cpu().tolist())
    ref, ref_counters, S = to.tree_accel(p, m, theta, to.SOFTENING, quadrupole=quadrupole, order=order, cond=True)
    ref_phi, phi_counters = tpo.tree_potential(p, m, theta, to.SOFTENING, quadrupole=quadrupole, order=order)
    err, bound = np.linalg.norm(acc - ref, axis=1), _acc_bound(S)
    phi_err, phi_bound = np.abs(phi - ref_phi), (PHI_TOL if theta == 0.05 else 3e-6) * np.abs(ref_phi)
    d_acc, d_phi = _direct(name)
    e_gpu, e_ref = to.row_errors(acc, d_acc), to.row_errors(ref, d_acc)
    f_gpu, f_ref = tpo.row_errors(phi, d_phi), tpo.row_errors(ref_phi, d_phi)
    print(f"{name} theta={theta} quad={quadrupole}: counters {counters} (oracle {ref_counters}); largest row error / bound: "
          f"a {_ratio(err, bound):.3f}, phi {_ratio(phi_err, phi_bound):.3f}; a vs direct max {e_gpu.max():.3e} (oracle "
          f"{e_ref.max():.3e}) rms {_rms(e_gpu):.3e} ({_rms(e_ref):.3e}); phi vs direct max {f_gpu.max():.3e} "
          f"({f_ref.max():.3e}) rms {_rms(f_gpu):.3e} ({_rms(f_ref):.3e})")
    assert np.isfinite(acc).all() and np.isfinite(phi).all() and phi.dtype == np.float64
    assert counters == ref_counters == phi_counters
    assert (err <= bound).all(), np.flatnonzero(~(err <= bound))[:16]
    assert (phi_err <= phi_bound).all(), np.flatnonzero(~(phi_err <= phi_bound))[:16]
    assert e_gpu.max() <= 2 * e_ref.max() + 3e-6 and _rms(e_gpu) <= 2 * _rms(e_ref) + 3e-6
    assert f_gpu.max() <= 2 * f_ref.max() + 3e-6 and _rms(f_gpu) <= 2 * _rms(f_ref) + 3e-6
    if name == "outlier" and theta == 0.05:
        # the oracle accepts no cell here, so every row but the outlier's is the direct sum, to the pair term's count
        assert ref_counters[0] == 0 and (S[:, 1] == 0).all()
        rest = np.arange(n) != n - 1
        d_err = np.linalg.norm(acc - d_acc, axis=1)
        print(f"outlier theta=0.05 against the fp64 direct sum: largest row error / bound {_ratio(d_err[rest], bound[rest]):.3f}")
        assert (d_err[rest] <= bound[rest]).all()


# ---------------------------------------------------------------- e. theta > 0 where the tree divides at level 2

def test_theta_half_where_the_waves_divide_the_tree_at_level_2(gpu_device):
    """deep: 33 025 bodies, 4129 / 517 / 65 / 9 / 2 / 1 nodes, so the 8 waves of a group own the subtrees of the 65
    level-2 nodes by index mod 8, cells are accepted above, at and below that level and a wave's stack carries two levels
    below it; the last node of levels 0, 1 and 2 is ragged and group 516 holds ONE body. 24 groups are walked on their
    own: counters equal the oracle's, rows within the bars of the walks above, group 516's 63 padding rows exactly 0; the
    full walk gives the same bits, and its counters are the sum of all 517 per-group ones."""
    from nbd import tree
    b, (p, m) = _built("deep"), tbo.inputs("deep")
    n, order, ws = b["n"], b["order"].astype(np.int64), b["ws"]
    groups, n_groups = tbo.deep_groups(), tree.groups(n)
    assert n_groups == 517 and [len(t) for t in b["nodes"]] == [4129, 517, 65, 9, 2, 1]
    ref, ref_counters, S = to.tree_accel(p, m, 0.5, to.SOFTENING, order=order, groups=groups, cond=True)
    ref_phi, _ = tpo.tree_potential(p, m, 0.5, to.SOFTENING, order=order, groups=groups)

    total = torch.zeros(2, dtype=torch.int64, device="cuda")
    full = tree.accel(ws, n, 0.5, EPS2, 1.0, True, counters=total)
    per_group = torch.zeros((n_groups, 2), dtype=torch.int64, device="cuda")
    rows_a = torch.empty((n_groups, 64, 3), dtype=torch.float32, device="cuda")
    rows_phi = torch.empty((n_groups, 64), dtype=torch.float64, device="cuda")
    for g in range(n_groups):
        tree.accel_potential_groups(ws, n, g, g + 1, 0.5, EPS2, 1.0, True, out=(rows_a[g], rows_phi[g]),
                                    counters=per_group[g])
    full, total, per_group, rows_a, rows_phi = _np(full), total.cpu().tolist(), _np(per_group), _np(rows_a), _np(rows_phi)

    assert per_group.sum(0).tolist() == total
    tree_order_rows = rows_a.reshape(-1, 3)[:n]
    assert np.array_equal(full[order].view(np.uint32), tree_order_rows.view(np.uint32))       # every group, bit for bit
    assert (rows_a[516, 1:].view(np.uint32) == 0).all() and (rows_phi[516, 1:].view(np.uint64) == 0).all()
    at, worst_a, worst_phi = 0, 0.0, 0.0
    for g, want in zip(groups, ref_counters):
        k = min(n, 64 * g + 64) - 64 * g
        err = np.linalg.norm(rows_a[g, :k] - ref[at:at + k], axis=1)
        phi_err, phi_bound = np.abs(rows_phi[g, :k] - ref_phi[at:at + k]), 3e-6 * np.abs(ref_phi[at:at + k])
        bound = _acc_bound(S[at:at + k])
        worst_a, worst_phi = max(worst_a, _ratio(err, bound)), max(worst_phi, _ratio(phi_err, phi_bound))
        assert tuple(per_group[g].tolist()) == want, (g, per_group[g].tolist(), want)
        assert (err <= bound).all() and (phi_err <= phi_bound).all(), g
        at += k
    assert at == len(ref) == 23 * 64 + 1
    print(f"deep theta=0.5: counters of the full walk {total}; of the 24 sampled groups "
          f"{per_group[groups].sum(0).tolist()} (oracle {np.sum(ref_counters, axis=0).tolist()}); largest row error / bound: "
          f"a {worst_a:.3f}, phi {worst_phi:.3f}")
