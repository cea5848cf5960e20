"""The equal-mass range-sharded force (nbd_shard_force_local_uniform_f32 + nbd_shard_force_remote_uniform_f32: what every
rank of a multi-GPU run of equal masses executes) against an fp64 evaluation of the same rows, on every edge of the source
view: own range inside one chunk, first / last rank, both ends unaligned, the padded tail chunk walked masked or skipped,
waves that walk across the skipped run, fully aligned ranges. One process, emulated ranks through nbd.direct.

No tolerance here is new:
  BAR_EPS = 2e-6, BAR_EPS0 = 3e-6   tests/test_direct_gpu.py::test_split_force_matches_one_launch (split force against the
                                    one-launch force with softening; against fp64 without)
  BAR_NET = 2e-6                    tests/test_direct_gpu.py::test_config5_size_on_one_gpu_properties_and_rank_split
                                    (|sum_i m_i a_i| over sum_i |m_i a_i|)
The general-mass entries run on the same inputs and their error is printed beside the equal-mass one: they are not under
test, they tell an ill-conditioned input from a wrong kernel. Inputs: generate_plummer(n, seed=5) unmodified."""
import functools

import numpy as np
import pytest
import torch

from conftest import row_rel
from test_shard_uniform_host import rows_f64

pytestmark = pytest.mark.gpu

BAR_EPS, BAR_EPS0, BAR_NET = 2e-6, 3e-6, 2e-6
SEED = 5
GUARD = 4096


def _np(t):
    return t.detach().cpu().numpy()


def _bar(eps):
    return BAR_EPS if eps > 0 else BAR_EPS0


@functools.lru_cache(maxsize=4)
def _system(n):
    """(pos, mass) as numpy fp32 and on the device, the packed bodies and the common mass: made once per size, never
    modified."""
    from nbd import direct
    from nbd.plummer import generate_plummer
    p, _, m = generate_plummer(n, seed=SEED)
    assert m.min() == m.max()
    p32, m32 = p.astype(np.float32), m.astype(np.float32)
    pos, mass = torch.tensor(p32, device="cuda"), torch.tensor(m32, device="cuda")
    uniform = direct.uniform_mass(mass)
    assert uniform == float(m32[0])
    return p32, m32, pos, mass, direct.pack_posm(pos, mass), uniform


def _local_rows(pos, mass, lo, n_loc):
    from nbd import direct
    return direct.pack_posm(pos[lo:lo + n_loc].contiguous(), mass[lo:lo + n_loc].contiguous())


def _guarded_ws(n, lo, n_loc):
    """Exactly nbd_shard_workspace_bytes of NaN bytes, then GUARD bytes of a sentinel the launches must leave alone."""
    from nbd import direct
    nbytes = direct._lib.lib().nbd_shard_workspace_bytes(n, lo, n_loc)
    assert nbytes >= 12 * n_loc
    buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device="cuda")
    buf[:nbytes] = 0xFF                                          # every float a NaN
    buf[nbytes:] = 0xA5
    return buf[:nbytes], buf[nbytes:]


def _force(posm_all, posm_local, n, lo, n_loc, eps2, g, uniform, vel=None, c_kick=0.0):
    """One emulated rank: local then remote launch into a NaN-filled workspace and output; the guard stays untouched."""
    from nbd import direct
    ws, guard = _guarded_ws(n, lo, n_loc)
    acc = torch.full((n_loc, 3), float("nan"), device="cuda")
    direct.shard_force_local(posm_local, n_loc, n, lo, eps2, ws, uniform=uniform)
    direct.shard_force_remote(posm_all, n, posm_local, n_loc, lo, eps2, g, acc, vel, c_kick, ws, uniform=uniform)
    assert bool((guard == 0xA5).all()), "wrote behind nbd_shard_workspace_bytes"
    return acc


# (n, lo, n_loc): what the case reaches, and the plan properties (direct.shard_plan, lower bounds or exact zero) and view
# properties (plain index arithmetic) it relies on. tail: the padded last chunk of the gathered array is walked (masked,
# in the equal-mass kernel only) / skipped (the own range reaches the end) / absent (n a multiple of 64). The rank's own
# packed rows have a padded tail chunk of their own whenever n_loc is no multiple of 64 (the local launch walks it masked).
CASES = [
    ((64, 0, 32), dict(tail="absent")),                  # own range inside the only chunk
    ((64, 32, 32), dict(tail="absent")),
    ((65, 0, 33), dict(tail="walked")),                  # first rank; tail chunk of one body; edge1 = 0
    ((65, 33, 32), dict(tail="skipped")),                # last rank: ex_hi == n, no edge1
    ((130, 44, 43), dict(tail="walked")),                # both ends unaligned (edges 0 and 1), tail chunk 2
    ((130, 10, 119), dict(tail="walked", edge1_is_tail=True)),      # hi = 129: the edge1 chunk is also the tail chunk
    ((130, 64, 64), dict(tail="walked", aligned=True)),  # the gathered array's tail alone: no edge, no padding in the own rows
    ((300, 10, 5), dict(tail="walked", cr=2)),           # both edges in chunk 0, remote waves walk 2 chunks
    ((200, 0, 200), dict(tail="skipped", sr=0)),         # nothing remote
    ((1001, 100, 333), dict(tail="walked", sr=2, skipped=3)),       # whole chunks skipped between the edges
    ((1001, 500, 501), dict(tail="skipped", sl=2)),      # last ragged rank
    ((5000, 1667, 1667), dict(tail="walked", sl=2, cl=2, sr=2, cr=2, skipped=20)),  # waves walk across the skipped run
    ((5000, 4937, 63), dict(tail="skipped", sr=2, cr=2)),           # one-chunk last rank, many remote slabs
    ((4096, 3584, 512), dict(tail="absent", aligned=True)),         # no masked chunk in either launch (with softening)
    ((8192, 1024, 1024), dict(tail="absent", aligned=True)),
    ((16384, 6000, 2049), dict(tail="absent", sl=2, cl=2, sr=2, cr=2)),
    ((65535, 21845, 21845), dict(tail="walked", sl=2, cl=2, sr=2, cr=2)),
]


def _check_case_properties(n, lo, n_loc, want):
    from nbd import direct
    hi = lo + n_loc
    plan = direct.shard_plan(n, lo, n_loc)
    for key, name in (("sl", "slabs_local"), ("cl", "chunks_per_wave_local"), ("sr", "slabs_remote"),
                      ("cr", "chunks_per_wave_remote")):
        if key in want:
            assert (plan[name] == 0) if want[key] == 0 else (plan[name] >= want[key]), (name, plan)
    assert plan["slabs_local"] >= 1 and (plan["slabs_remote"] >= 1) == (n_loc < n), plan
    tail = "absent" if n % 64 == 0 else ("skipped" if hi == n else "walked")
    assert tail == want["tail"]
    if want.get("edge1_is_tail"):
        assert hi % 64 and hi // 64 == n // 64
    if want.get("aligned"):
        assert lo % 64 == 0 and hi % 64 == 0
    if "skipped" in want:
        assert hi // 64 - (lo + 63) // 64 >= want["skipped"]
    return plan


# softening 0.1 for every case; softening 0 (the index-masked kernel on every chunk) for every case with n <= 5000
RUNS = [pytest.param(c, w, eps, id="-".join(map(str, c)) + f"-eps{eps}")
        for c, w in CASES for eps in (0.1, 0.0) if eps > 0 or c[0] <= 5000]


@pytest.mark.parametrize("case,want,eps", RUNS)
def test_equal_mass_shard_force_matches_f64(case, want, eps, gpu_device):
    """Measured on the MI355X (equal-mass | general entries against fp64, per case and softening): NOTES.md, "Equal-mass
    range-sharded force against fp64"."""
    from nbd import direct
    n, lo, n_loc = case
    plan = _check_case_properties(n, lo, n_loc, want)
    p32, m32, pos, mass, posm, uniform = _system(n)
    eps2, g = direct.f32(eps ** 2), direct.f32(0.7)
    posm_local = _local_rows(pos, mass, lo, n_loc)
    vel = torch.full((n_loc, 3), 0.5, device="cuda")
    acc = _force(posm, posm_local, n, lo, n_loc, eps2, g, uniform, vel, 0.25)
    gen = _force(posm, posm_local, n, lo, n_loc, eps2, g, None)
    assert torch.isfinite(acc).all() and torch.isfinite(gen).all()
    if n < 65535:
        rows = np.arange(n_loc)
    else:
        rows = np.sort(np.random.default_rng(0).choice(n_loc, 256, replace=False))
    ref = rows_f64(p32, m32, g, eps2, 0, 0, rows=lo + rows)
    e_uni, e_gen = row_rel(_np(acc)[rows], ref), row_rel(_np(gen)[rows], ref)
    e_pair = row_rel(_np(acc), _np(gen))
    print(f"shard-uniform n={n} lo={lo} n_loc={n_loc} eps={eps} plan={plan['slabs_local']}x{plan['chunks_per_wave_local']}"
          f"+{plan['slabs_remote']}x{plan['chunks_per_wave_remote']} rows={rows.size} "
          f"uniform {e_uni:.2e} general {e_gen:.2e} uniform-vs-general {e_pair:.2e}")
    assert e_uni < _bar(eps), (e_uni, e_gen)
    if n == 65535:
        assert e_pair < BAR_EPS, e_pair            # all rows, against the general entries
    assert torch.equal(vel, torch.full_like(vel, 0.5) + 0.25 * acc)
    again = _force(posm, posm_local, n, lo, n_loc, eps2, g, uniform, None, 0.0)
    assert torch.equal(acc, again)


@pytest.mark.parametrize("eps", [0.1, 0.0])
def test_own_range_is_excluded_by_index(eps, gpu_device):
    """The rank's own rows of the gathered array are skipped or masked, never read into the sum: moving them (and giving
    them a huge mass) changes nothing. Under the equal-mass kernel the mass column is never read, so the moved positions
    are what proves it."""
    from nbd import direct
    n, lo, n_loc = 1000, 130, 301                      # both ends inside a 64-chunk, whole chunks between them
    _, _, pos, mass, posm, uniform = _system(n)
    eps2, g = direct.f32(eps ** 2), direct.f32(0.7)
    posm_local = _local_rows(pos, mass, lo, n_loc)
    moved = posm.clone()
    moved[lo:lo + n_loc, :3] += 3.0
    moved[lo:lo + n_loc, 3] = 1e30
    a = _force(posm, posm_local, n, lo, n_loc, eps2, g, uniform)
    b = _force(moved, posm_local, n, lo, n_loc, eps2, g, uniform)
    assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("eps", [0.1, 0.0])
@pytest.mark.parametrize("n", [200, 1000, 4096])
def test_rank_that_owns_everything_equals_the_unsharded_equal_mass_step(n, eps, gpu_device):
    """lo = 0, n_local = n: the local launch is the un-sharded equal-mass force (same plan, same view, same finishing
    kernel with the same g * m in fp32), nothing is remote: bit-identical to nbd_leapfrog_step_uniform_f32 at dt = 0."""
    from nbd import direct
    _, _, pos, mass, posm, uniform = _system(n)
    eps2, g = direct.f32(eps ** 2), direct.f32(0.7)
    assert direct.shard_plan(n, 0, n)["slabs_remote"] == 0
    a = _force(posm, posm, n, 0, n, eps2, g, uniform)
    x, v = pos.clone(), torch.zeros_like(pos)
    acc_out = torch.full((n, 3), float("nan"), device="cuda")
    direct.leapfrog_step(x, v, torch.zeros_like(pos), acc_out, mass, 0.0, 0.0, eps2, g, direct.alloc_posm(n, "cuda"),
                         direct.step_workspace(n, "cuda"), uniform=uniform)
    assert torch.equal(x, pos) and torch.isfinite(a).all()
    assert torch.equal(a, acc_out)


@pytest.mark.parametrize("n,world", [(1001, 3), (5000, 7), (130, 8)])
def test_all_ranks_of_a_partition(n, world, gpu_device):
    """Every rank of RangePartition(n, P, .): the assembled rows against fp64, and Newton's third law on them ((130, 8):
    ranks of 16-17 bodies whose whole range lies inside one chunk)."""
    from nbd import direct
    from nbd.dist import RangePartition
    p32, m32, pos, mass, posm, uniform = _system(n)
    eps2, g = direct.f32(0.1 ** 2), direct.f32(0.7)
    parts = []
    for r in range(world):
        part = RangePartition(n, world, r)
        parts.append(_force(posm, _local_rows(pos, mass, part.lo, part.n_local), n, part.lo, part.n_local, eps2, g,
                            uniform))
    acc = torch.cat(parts)
    assert acc.shape == (n, 3) and torch.isfinite(acc).all()
    err = row_rel(_np(acc), rows_f64(p32, m32, g, eps2, 0, n))
    a64 = acc.double()
    net = float(a64.sum(0).norm() / a64.norm(dim=1).sum())      # equal masses: sum_i a_i = 0
    print(f"shard-uniform partition n={n} P={world} rows {err:.2e} net {net:.2e}")
    assert err < BAR_EPS and net < BAR_NET


def test_error_names_the_entry_that_ran(gpu_device):
    """A workspace one byte short is refused before anything is launched, and the message names the entry called."""
    from nbd import _lib, direct
    n, lo, n_loc = 130, 44, 43
    _, _, pos, mass, posm, uniform = _system(n)
    posm_local = _local_rows(pos, mass, lo, n_loc)
    ws, _ = _guarded_ws(n, lo, n_loc)
    acc = torch.empty((n_loc, 3), device="cuda")
    for uni, tag in ((uniform, "_uniform_f32"), (None, "_f32")):
        with pytest.raises(_lib.NbdError, match="nbd_shard_force_local" + tag):
            direct.shard_force_local(posm_local, n_loc, n, lo, 0.01, ws[:-1], uniform=uni)
        with pytest.raises(_lib.NbdError, match="nbd_shard_force_remote" + tag):
            direct.shard_force_remote(posm, n, posm_local, n_loc, lo, 0.01, 1.0, acc, None, 0.0, ws[:-1], uniform=uni)
