"""Hermite6Simulator without a GPU: the 6th-order oracle (tests/hermite6_oracle.py) is what it says it is -- its snap is
the derivative of its jerk along the flow, its a and j are hermite_oracle's, it converges at 6th order and reproduces the
two-body energy errors the scheme was chosen for --, the new C-ABI entries are declared, bound and refuse bad arguments
on the host, the pair kernel keeps the occupancy its LDS allows, and the constructor's refusals come before anything
touches a device."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import hermite6_oracle as h6
import hermite_f64_oracle as fo
import hermite_oracle as ho
from conftest import ROOT
from nbd import _lib

SRC = os.path.join(ROOT, "nbody-deep-sim_amd", "csrc", "direct_hermite_f64.hip")       # both orders' unit
FORCE6 = "force_f64_kernelINS_6Order6E"                  # the mangled name carries the order
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S"]
ENTRIES = ("nbd_hermite6_f64_workspace_bytes", "nbd_hermite6_f64_pack", "nbd_accel_jerk_snap_f64",
           "nbd_hermite6_step_f64")
# relative energy error after one period of the e = 0.5 orbit (eps = 0.1), by steps per period: (6th order, 4th order)
TABLE = {64: (2.2e-5, 9.1e-4), 128: (2.0e-7, 2.9e-5), 256: (1.6e-9, 8.9e-7), 512: (1.3e-11, 2.8e-8),
         1024: (1.1e-13, 8.7e-10)}


def _random_case(n, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 3)), rng.normal(size=(n, 3)), rng.uniform(0.5, 1.0, n)


def test_snap_is_the_derivative_of_the_jerk_along_the_flow():
    """Central difference of the oracle's jerk at x +- v d + a d^2/2, v +- a d + j d^2/2 (n = 5, d = 1e-5): the
    truncation is O(d^2) ~ 1e-10 and the rounding 2^-53 / d ~ 1e-11 of the jerk; measured 5e-9 relative."""
    x, v, m = _random_case(5, 0)
    g, eps2, d = 1.0, 0.01, 1e-5
    a, j, s, c = h6.start(x, v, m, g, eps2)
    assert not c.any()
    jp = ho.accel_jerk(x + v * d + a * (d * d / 2), v + a * d + j * (d * d / 2), m, g, eps2)[1]
    jm = ho.accel_jerk(x - v * d + a * (d * d / 2), v - a * d + j * (d * d / 2), m, g, eps2)[1]
    rel = np.abs((jp - jm) / (2 * d) - s).max() / np.abs(s).max()
    print(f"snap against the central difference of the jerk: relative {rel:.3e}")
    assert rel <= 1e-7, rel


@pytest.mark.parametrize("n", [5, 130, 700])
def test_acceleration_and_jerk_are_hermite_oracles(n):
    x, v, m = fo.plummer_case(n, seed=60 + n)
    a, j = ho.accel_jerk(x, v, m, 1.0, 0.05 ** 2)
    a6, j6, s6 = h6.accel_jerk_snap(x, v, a, m, 1.0, 0.05 ** 2)
    assert np.array_equal(a6, a) and np.array_equal(j6, j)
    assert np.all(np.abs(s6) <= h6.snap_abs(x, v, a, m, 1.0, 0.05 ** 2))      # a sum is no larger than its |terms|


def test_the_snap_bar_is_not_tighter_than_fp64_allows():
    """The oracle against itself with the sources permuted, at the bar the GPU is held to (T = 19 n); an fp32
    intermediate misses it by orders of magnitude."""
    n = 130
    x, v, m = fo.plummer_case(n, seed=77)
    g, eps2 = 1.0, 0.1 ** 2
    a = ho.accel_jerk(x, v, m, g, eps2)[0]
    s = h6.accel_jerk_snap(x, v, a, m, g, eps2)[2]
    s_abs = h6.snap_abs(x, v, a, m, g, eps2)
    order = np.random.default_rng(n).permutation(n)
    back = np.empty_like(order)
    back[order] = np.arange(n)
    s2 = h6.accel_jerk_snap(x[order], v[order], a[order], m[order], g, eps2)[2][back]
    ok, frac = fo.within(s2, s, 19 * n, s_abs)
    assert ok and frac < 0.01, frac
    s32 = h6.accel_jerk_snap(x.astype(np.float32).astype(np.float64), v, a, m, g, eps2)[2]
    assert fo.within(s32, s, 19 * n, s_abs)[1] > 1e3


@pytest.fixture(scope="module")
def two_body_runs():
    x, v, m, period = ho.two_body(0.5)
    x, v, m = fo.perturbed(x, v, m, 9)
    eps2 = 0.1 ** 2
    runs = {s: h6.hermite6_run(x, v, m, period / s, 1.0, eps2, s) for s in (64, 128, 256, 512, 1024)}
    return x, v, m, period, eps2, runs


def test_two_body_oracle_converges_at_sixth_order(two_body_runs):
    """Halving dt divides the position error (the difference to the run with half the step) by 2^6 = 64; measured 75.2 at
    128 steps and 71.6 at 256. The first step's predictor has c = 0 and does not cost the order."""
    *_, runs = two_body_runs
    for s in (128, 256):
        ratio = np.abs(runs[s][0] - runs[2 * s][0]).max() / np.abs(runs[2 * s][0] - runs[4 * s][0]).max()
        print(f"S={s}: position-error ratio {ratio:.2f}")
        assert 48.0 < ratio < 96.0, (s, ratio)


def test_two_body_energy_errors(two_body_runs):
    """The errors the scheme was chosen for, both orders, to 5 %: 512 6th-order steps do what takes the 4th order 2048."""
    x, v, m, period, eps2, runs = two_body_runs
    e0 = fo.energy(x, v, m, 1.0, eps2)
    for s, (want6, want4) in TABLE.items():
        r4 = ho.hermite_run(x, v, m, period / s, 1.0, eps2, s)
        err6 = abs(fo.energy(runs[s][0], runs[s][1], m, 1.0, eps2) - e0) / abs(e0)
        err4 = abs(fo.energy(r4[0], r4[1], m, 1.0, eps2) - e0) / abs(e0)
        print(f"S={s}: energy error 6th order {err6:.3e}, 4th order {err4:.3e}")
        assert abs(err6 - want6) <= 0.05 * want6 and abs(err4 - want4) <= 0.05 * want4, (s, err6, err4)


def test_crackle_is_the_third_derivative_of_the_quintic():
    """On a polynomial a(t) of degree 5 the formula is exact: c1 = a'''(t1)."""
    rng = np.random.default_rng(4)
    coef = rng.normal(size=(6, 3))
    poly = [np.polynomial.Polynomial(coef[:, k]) for k in range(3)]
    at = lambda d, t: np.array([p.deriv(d)(t) if d else p(t) for p in poly])      # noqa: E731
    t0, dt = 0.3, 0.25
    c1 = h6.crackle(at(0, t0), at(1, t0), at(2, t0), at(0, t0 + dt), at(1, t0 + dt), at(2, t0 + dt), dt)
    assert np.allclose(c1, at(3, t0 + dt), rtol=1e-10, atol=0)


def test_new_symbols_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbd.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared in include/nbd.h"
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert L.nbd_abi_version() == _lib.ABI_VERSION == 2          # entries were added, nothing else changed


def test_argument_checks_without_a_gpu():
    L = _lib.lib()
    import ctypes
    g, s, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert L.nbd_hermite6_f64_workspace_bytes(0) == 0 and L.nbd_hermite6_f64_workspace_bytes(-3) == 0
    for n in (1, 64, 65, 448, 449, 1000, 5000, 65536):
        assert L.nbd_hermite_f64_plan(n, g, s, c) == 0
        assert L.nbd_hermite6_f64_workspace_bytes(n) == s.value * 9 * n * 8
    big = 1 << 30
    p, q, r, a, j, sn, ws = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000
    # the force
    f = L.nbd_accel_jerk_snap_f64
    assert f(None, None, None, 0, 0.01, 1.0, None, None, None, None, 0, 0, None) == 0
    assert f(None, None, None, -1, 0.01, 1.0, None, None, None, None, 0, 0, None) == -1
    assert f(None, None, None, 4, 0.01, 1.0, None, None, None, None, 0, 0, None) == -1
    for bad in range(6):                                         # every pointer NULL in turn
        args = [p, q, r, a, j, sn]
        args[bad] = None
        assert f(*args[:3], 4, 0.01, 1.0, *args[3:], ws, big, 0, None) == -1, bad
    for bad in range(3):                                         # every packed array off its 32 bytes in turn
        args = [p, q, r]
        args[bad] += 16
        assert f(*args, 4, 0.01, 1.0, a, j, sn, ws, big, 0, None) == -1, bad
    assert f(p, q, r, 4, 0.01, 1.0, a, j, sn, ws, big, 65, None) == -1
    assert f(p, q, r, 4, 0.01, 1.0, a, j, sn, ws, big, -1, None) == -1
    assert f(p, q, r, 4, 0.01, 1.0, a, j, sn, None, big, 0, None) == -2
    assert f(p, q, r, 4, 0.01, 1.0, a, j, sn, ws + 4, big, 0, None) == -2
    assert f(p, q, r, 4, 0.01, 1.0, a, j, sn, ws, 4 * 9 * 8 - 1, 0, None) == -2
    assert f(p, q, r, 4, 0.01, 1.0, a, j, sn, ws, 4 * 9 * 8, 2, None) == -2
    # the pack
    f = L.nbd_hermite6_f64_pack
    assert f(*([None] * 7), 0, 0.1, None, None, None, None) == 0
    assert f(*([None] * 7), -1, 0.1, None, None, None, None) == -1
    assert f(*([None] * 7), 4, 0.1, None, None, None, None) == -1
    good = [p, p, None, None, None, None, p, 4, 0.1, p, q, r, None]
    for bad in (0, 1, 6, 9, 10, 11):
        args = list(good)
        args[bad] = None
        assert f(*args) == -1, bad
    for bad in (9, 10, 11):
        args = list(good)
        args[bad] += 8
        assert f(*args) == -1, bad
    for acc, jerk, snap, crk in ((None, p, p, p), (p, p, None, None), (p, None, p, None), (p, None, None, p),
                                 (p, p, p, None)):               # jerk, snap and crackle together, and only with acc
        assert f(p, p, acc, jerk, snap, crk, p, 4, 0.1, p, q, r, None) == -1
    # the step
    f = L.nbd_hermite6_step_f64
    tail = (4, 0.1, 0.01, 1.0)
    assert f(*([None] * 11), 0, 0.1, 0.01, 1.0, None, None, None, None, 0, None) == 0
    assert f(*([None] * 11), -1, 0.1, 0.01, 1.0, None, None, None, None, 0, None) == -1
    assert f(*([None] * 11), *tail, None, None, None, None, 0, None) == -1
    for bad in range(14):
        args = [p] * 11 + [p, q, r]
        args[bad] = None
        assert f(*args[:11], *tail, *args[11:], ws, big, None) == -1, bad
    for bad in range(3):
        args = [p, q, r]
        args[bad] += 16
        assert f(*([p] * 11), *tail, *args, ws, big, None) == -1, bad
    assert f(*([p] * 11), *tail, p, q, r, None, big, None) == -2
    assert f(*([p] * 11), *tail, p, q, r, ws + 4, big, None) == -2
    assert f(*([p] * 11), *tail, p, q, r, ws, 4 * 9 * 8 - 1, None) == -2


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "direct_hermite_f64.s")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-o", out, SRC], check=True, capture_output=True)
    return open(out).read()


@pytest.mark.parametrize("kernel", [FORCE6, "hermite6_predict_kernel", "hermite6_finish_kernel"])
def test_kernels_have_no_scratch_and_keep_their_occupancy(asm, kernel):
    """No scratch and no spills anywhere. The pair kernel holds 4 x stage_quads_n<3>() = 48 KiB of LDS, three workgroups
    (12 waves) per CU, which 168 VGPRs still allow; it streams by LDS-DMA and has no fp32 intermediate."""
    names = re.findall(r"\.name:\s+(\S*" + kernel + r"\S*)", asm)
    assert len(names) == 1
    meta = asm[asm.index(".name:           " + names[0]):]
    meta = meta[:meta.index(".name:           ", 20) if ".name:           " in meta[20:] else len(meta)]
    num = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", meta).group(1))      # noqa: E731
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
        assert num(key) == 0, key
    desc = asm[asm.index(".amdhsa_kernel " + names[0]):]
    lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1))
    body = asm[asm.index(names[0] + ":"):]
    body = body[:body.index(".Lfunc_end")]
    assert "v_cvt_f32_f64" not in body and "v_rsq_f32" not in body
    assert not re.search(r"\b(global|flat|ds|buffer)_atomic", body)
    if kernel == FORCE6:
        assert lds == 48 * 1024
        assert num("vgpr_count") <= 168
        assert "global_load_lds_dwordx4" in body and "v_rsq_f64" in body and "vmcnt(6)" in body
    else:
        assert lds == 0


def test_refusals_come_before_any_device_work():
    from galaxify import simulation
    cls = simulation.Hermite6Simulator
    z = np.zeros((4, 3))
    kw = dict(positions=z, velocities=z, masses=np.ones(4), device="cpu")
    for bad in (torch.float32, torch.float16, torch.bfloat16, torch.int32, "float64", None):
        with pytest.raises(ValueError, match="dtype.*fp32 floor"):
            cls(dtype=bad, **kw)
    with pytest.raises(ValueError, match="process_group"):
        cls(process_group=object(), **kw)
    with pytest.raises(ValueError, match="process_group"):
        cls(dtype=torch.float64, process_group=object(), **kw)
    with pytest.raises(TypeError, match="no_such_keyword"):
        cls(no_such_keyword=1, **kw)
    with pytest.raises(RuntimeError, match="cpu"):               # with everything in order, the project's usual rule
        cls(**kw)
    with pytest.raises(RuntimeError, match="cpu"):
        cls(dtype=torch.float64, **kw)
    params = inspect.signature(cls.__init__).parameters
    assert list(params) == ["self", "positions", "velocities", "masses", "g_const", "softening", "dt", "calc_energy",
                            "device", "process_group", "calc_invariants", "format_kw"]
    assert params["format_kw"].kind is inspect.Parameter.VAR_KEYWORD
    assert issubclass(cls, simulation.HermiteSimulator) and not issubclass(cls, simulation.BlockHermiteSimulator)
    # eager run(): the class states its own step() and no in-place twin of it, and its format has no captured form
    sim = object.__new__(cls)
    sim._fmt, sim._sharded, sim.n = simulation._FORMATS[torch.float64], False, 100
    assert sim._f64 is True and not sim._graph_run_ok(64) and not cls._capturable()
    for name in ("compute_accelerations", "compute_accelerations_and_jerks"):        # inherited as they are
        assert getattr(cls, name) is getattr(simulation.HermiteSimulator, name)
    assert "compute_accelerations_jerks_and_snaps" in vars(cls)


def test_the_snap_refuses_autograd_before_any_launch():
    from galaxify import simulation
    sim = object.__new__(simulation.Hermite6Simulator)
    sim.n = 4
    sim.positions = torch.zeros((4, 3), dtype=torch.float64, requires_grad=True)
    sim.velocities = torch.zeros((4, 3), dtype=torch.float64)
    sim.masses = torch.ones(4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="differentiable"):
        sim.compute_accelerations_jerks_and_snaps()
