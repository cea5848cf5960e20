"""The differentiable Hermite force without a GPU: the numpy oracle of its vector-Jacobian product
(accel_jerk_vjp_oracle.py) pinned to torch's fp64 autograd and to the acceleration's backward it contains, the condition
under which the oracle alone stays inside the fp64 bar, the argument checks of the nbd_accel_jerk_vjp_* entry points, and
the resources of the kernels in the gfx950 assembly of csrc/direct_hermite_grad.hip (hipcc cross-compiles)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import accel_jerk_vjp_oracle as jo
import accel_vjp_oracle as vo
import hermite_f64_oracle as fo
from conftest import ROOT, global_rel

G, EPS = 1.0, 0.05
SIZES = [1, 2, 3, 65, 130]


@pytest.mark.parametrize("n", SIZES)
def test_oracle_matches_torch_fp64_autograd(n):
    """Unequal masses, one of them zero (n > 1), both cotangents and each alone. 1e-12 leaves room for other BLAS and
    threading orders."""
    x, v, m, ca, cj = jo.case(n, seed=10 + n, zero_mass=True)
    assert n == 1 or (m == 0).sum() == 1
    for tag, a, b in (("both", ca, cj), ("alpha", ca, None), ("beta", None, cj)):
        got = jo.accel_jerk_vjp(x, v, m, a, b, G, EPS * EPS)[:3]
        ref = jo.torch_vjp(x, v, m, a, b, G, EPS, torch.float64)
        errs = [global_rel(p, q) for p, q in zip(got, ref)]
        print(f"n={n} {tag}: oracle vs torch fp64 autograd: dL/dx {errs[0]:.2e}, dL/dv {errs[1]:.2e}, dL/dm {errs[2]:.2e}")
        assert max(errs) <= 1e-12
        if n == 1 or tag == "alpha":
            assert not got[1].any()                     # no partner, or no beta: dL/dv is exact zeros
        if n == 1:
            assert not got[0].any() and not got[2].any()


@pytest.mark.parametrize("n", SIZES)
def test_velocity_gradient_is_the_accelerations_position_gradient(n):
    """dL/dv of (alpha, beta) is dL/dx of the acceleration's backward with cot = beta, terms included."""
    x, v, m, ca, cj = jo.case(n, seed=20 + n)
    out = jo.accel_jerk_vjp(x, v, m, ca, cj, G, EPS * EPS)
    gx, _, sx, _ = vo.accel_vjp(x, m, cj, G, EPS * EPS)
    assert np.array_equal(out[1], gx) and np.array_equal(out[4], sx)


@pytest.mark.parametrize("n", [3, 65, 130, 1000])
def test_oracle_in_another_source_order_stays_inside_the_bar(n):
    """What the bar has to grant to any correct fp64 evaluation: the oracle itself, its sources permuted, is within
    bar(T n, sum|terms|) of its natural order, T = 44, 8, 15."""
    x, v, m, ca, cj = jo.case(n, seed=30 + n, zero_mass=True)
    nat = jo.accel_jerk_vjp(x, v, m, ca, cj, G, EPS * EPS)
    order = np.random.default_rng(n).permutation(n)
    per = jo.accel_jerk_vjp(x, v, m, ca, cj, G, EPS * EPS, order=order)
    for k, (nm, t) in enumerate((("dL/dx", jo.T_POS), ("dL/dv", jo.T_VEL), ("dL/dm", jo.T_MASS))):
        ok, f = fo.within(per[k], nat[k], t * n, nat[3 + k])
        print(f"n={n}: permuted sources: {nm} {f:.3f} of the bar")
        assert ok, (nm, f)
        assert np.allclose(per[3 + k], nat[3 + k], rtol=1e-12)


def _f32_bytes(n, slabs):
    return (((slabs * 7 * n + 3) & ~3) + slabs * 4 * n + 4 * n) * 4


def _f64_bytes(n, slabs):
    return (((slabs * 7 * n + 3) & ~3) + slabs * 4 * n + 4 * n) * 8


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    from nbd import _lib
    L = _lib.lib()
    ok16, ok32, odd = 0x10000, 0x20000, 0x10004               # never dereferenced: every call below is refused first
    nan, inf, big = float("nan"), float("inf"), 1 << 40
    f32, f64 = L.nbd_accel_jerk_vjp_f32, L.nbd_accel_jerk_vjp_f64
    # float32: (posm, velp, cota, cotj, n, eps2, g, grad_pos, grad_vel, grad_mass, workspace, workspace_bytes, stream)
    assert f32(None, None, None, None, -1, 0.01, 1.0, None, None, None, None, 0, None) == -1
    assert f32(None, None, None, None, 5, 0.01, 1.0, None, None, None, None, 0, None) == -1
    assert f32(ok16, ok16, None, None, 5, 0.01, 1.0, ok16, ok16, ok16, ok16, big, None) == -1       # no cotangent at all
    assert f32(ok16, ok16, ok16, ok16, 5, 0.01, 1.0, None, None, None, ok16, big, None) == -1       # no output at all
    assert f32(ok16, ok16, ok16, ok16, 5, 0.01, 1.0, ok16, ok16, ok16, None, big, None) == -1       # no workspace
    need = L.nbd_accel_jerk_vjp_workspace_bytes(5)
    assert need > 0
    assert f32(ok16, ok16, ok16, ok16, 5, 0.01, 1.0, ok16, ok16, ok16, ok16, need - 1, None) == -1  # too small
    assert f32(ok16, ok16, ok16, ok16, 5, 0.01, 1.0, ok16, ok16, ok16, ok16, 0, None) == -1
    for k in range(4):                                                                              # rows: 16 bytes
        rows = [ok16] * 4
        rows[k] = odd
        assert f32(*rows, 5, 0.01, 1.0, ok16, ok16, ok16, ok16, big, None) == -1
    assert f32(None, ok16, ok16, ok16, 5, 0.01, 1.0, ok16, ok16, ok16, ok16, big, None) == -1
    assert f32(ok16, None, ok16, ok16, 5, 0.01, 1.0, ok16, ok16, ok16, ok16, big, None) == -1
    for k in range(3):                                                                              # outputs: 4 bytes
        outs = [ok16] * 3
        outs[k] = ok16 + 2
        assert f32(ok16, ok16, ok16, ok16, 5, 0.01, 1.0, *outs, ok16, big, None) == -1
    assert f32(ok16, ok16, ok16, ok16, 5, 0.01, 1.0, ok16, ok16, ok16, odd, big, None) == -1
    for eps2, g in ((nan, 1.0), (inf, 1.0), (0.01, nan), (0.01, -inf)):
        assert f32(ok16, ok16, ok16, ok16, 5, eps2, g, ok16, ok16, ok16, ok16, big, None) == -1
    assert f32(None, None, None, None, 0, 0.01, 1.0, None, None, None, None, 0, None) == 0          # n = 0: nothing to do
    assert L.nbd_accel_jerk_vjp_workspace_bytes(0) == 0 and L.nbd_accel_jerk_vjp_workspace_bytes(-3) == 0
    g_, s_, c_ = (ctypes.c_int() for _ in range(3))
    for n in (5, 130, 5000):
        assert L.nbd_accel_plan(n, n, g_, s_, c_) == 0
        assert L.nbd_accel_jerk_vjp_workspace_bytes(n) == _f32_bytes(n, s_.value)
        assert _f32_bytes(n, s_.value) >= 7 * s_.value * n * 4 + L.nbd_accel_vjp_workspace_bytes(n) + 16 * n
    # float64: ... workspace_bytes, slabs, stream
    assert f64(None, None, None, None, -1, 0.01, 1.0, None, None, None, None, 0, 0, None) == -1
    assert f64(None, None, None, None, 5, 0.01, 1.0, None, None, None, None, 0, 0, None) == -1
    assert f64(ok32, ok32, None, None, 5, 0.01, 1.0, ok32, ok32, ok32, ok32, big, 0, None) == -1
    assert f64(ok32, ok32, ok32, ok32, 5, 0.01, 1.0, None, None, None, ok32, big, 0, None) == -1
    assert f64(ok32, ok32, ok32, ok32, 5, 0.01, 1.0, ok32, ok32, ok32, None, big, 0, None) == -1
    need = L.nbd_accel_jerk_vjp_f64_workspace_bytes(5, 0)
    assert need > 0
    assert f64(ok32, ok32, ok32, ok32, 5, 0.01, 1.0, ok32, ok32, ok32, ok32, need - 1, 0, None) == -1
    assert f64(ok32, ok32, ok32, ok32, 5, 0.01, 1.0, ok32, ok32, ok32, ok32,
               L.nbd_accel_jerk_vjp_f64_workspace_bytes(5, 3) - 1, 3, None) == -1
    for k in range(4):                                                                              # rows: 32 bytes
        rows = [ok32] * 4
        rows[k] = ok32 + 16
        assert f64(*rows, 5, 0.01, 1.0, ok32, ok32, ok32, ok32, big, 0, None) == -1
    assert f64(None, ok32, ok32, ok32, 5, 0.01, 1.0, ok32, ok32, ok32, ok32, big, 0, None) == -1
    assert f64(ok32, None, ok32, ok32, 5, 0.01, 1.0, ok32, ok32, ok32, ok32, big, 0, None) == -1
    for k in range(3):                                                                              # outputs: 8 bytes
        outs = [ok32] * 3
        outs[k] = ok32 + 4
        assert f64(ok32, ok32, ok32, ok32, 5, 0.01, 1.0, *outs, ok32, big, 0, None) == -1
    assert f64(ok32, ok32, ok32, ok32, 5, 0.01, 1.0, ok32, ok32, ok32, ok32 + 4, big, 0, None) == -1
    assert f64(ok32, ok32, ok32, ok32, 5, 0.01, 1.0, ok32, ok32, ok32, ok32, big, -1, None) == -1
    assert f64(ok32, ok32, ok32, ok32, 5, 0.01, 1.0, ok32, ok32, ok32, ok32, big, 65, None) == -1
    for eps2, g in ((nan, 1.0), (-inf, 1.0), (0.01, nan), (0.01, inf)):
        assert f64(ok32, ok32, ok32, ok32, 5, eps2, g, ok32, ok32, ok32, ok32, big, 0, None) == -1
    assert f64(None, None, None, None, 0, 0.01, 1.0, None, None, None, None, 0, 0, None) == 0
    wb = L.nbd_accel_jerk_vjp_f64_workspace_bytes
    assert wb(0, 0) == 0 and wb(100, 65) == 0 and wb(100, -1) == 0
    assert wb(448, 0) == _f64_bytes(448, 1)                                                         # nbd_hermite_f64_plan:
    assert wb(449, 0) == _f64_bytes(449, 2)                                                         # one slab -> two
    assert wb(1000, 3) == _f64_bytes(1000, 3)
    for n, slabs in ((448, 0), (449, 0), (1000, 3)):
        assert wb(n, slabs) >= (slabs or (1 if n == 448 else 2)) * 7 * n * 8 + L.nbd_accel_vjp_f64_workspace_bytes(n, slabs)


def test_wrappers_refuse_cpu_tensors():
    from nbd import _lib, autograd, direct
    x, m = torch.zeros((4, 3)), torch.ones(4)
    with pytest.raises(_lib.NbdError):
        autograd.direct_accel_jerk(x, x.clone(), m)
    with pytest.raises(_lib.NbdError):
        autograd.direct_accel_jerk(x.double(), x.double(), m.double())
    rows = torch.zeros((64, 4))
    with pytest.raises(_lib.NbdError):
        direct.accel_jerk_vjp(rows, rows, rows, rows, 4, 0.01, 1.0)
    rows = rows.double()
    with pytest.raises(_lib.NbdError):
        direct.accel_jerk_vjp_f64(rows, rows, rows, rows, 4, 0.01, 1.0)


# ---- kernel resources, from the assembly
SRC = os.path.join(ROOT, "nbody-deep-sim_amd", "csrc", "direct_hermite_grad.hip")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S"]
WALKS = ["accel_jerk_vjp_kernelILb0E", "accel_jerk_vjp_kernelILb1E", "accel_jerk_vjp_f64_kernel"]
UNMASKED = ["accel_jerk_vjp_kernelILb0E", "accel_jerk_vjp_f64_kernel"]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa_hvjp") / "direct_hermite_grad.s")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-o", out, SRC], check=True, capture_output=True)
    return open(out).read()


def _kernels(asm):
    """{kernel symbol: (vgpr_count, private_segment_fixed_size)} from the metadata."""
    out = {}
    for blk in asm[asm.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                     int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    return out


def _pair_loops(asm, name):
    """The innermost loops of kernel `name` that hold a reciprocal square root: lists of instructions."""
    i = asm.index(name + ":")
    parts = re.split(r"\n(\.LBB\d+_\d+):", asm[i:asm.index(".Lfunc_end", i)])
    loops = []
    for label, block in zip(parts[1::2], parts[2::2]):
        ins = [ln.strip() for ln in block.split("\n")]
        ins = [ln for ln in ins if ln and not ln.startswith((";", "."))]
        back = [k for k, ln in enumerate(ins) if ln.startswith("s_cbranch") and ln.endswith(" " + label)]
        if back and any(ln.startswith("v_rsq_") for ln in ins[:back[0] + 1]):
            loops.append(ins[:back[0] + 1])
    return loops


def test_kernel_resources(asm):
    """A zero private segment for every kernel; the VGPR counts are reported, not capped."""
    kernels = _kernels(asm)
    assert len(kernels) == 5, sorted(kernels)           # two fp32 walks, the fp64 walk, two finishing kernels
    for name, (vgpr, scratch) in kernels.items():
        print(f"{name}: {vgpr} VGPRs, {scratch} bytes of scratch")
        assert scratch == 0, (name, vgpr, scratch)
    for key in WALKS:
        assert sum(key in name for name in kernels) == 1, key


def test_unmasked_loops_stay_in_registers(asm):
    kernels = _kernels(asm)
    for key in UNMASKED:
        name = next(k for k in kernels if key in k)
        loops = [ins for ins in _pair_loops(asm, name) if not any(ln.startswith("v_cndmask") for ln in ins)]
        assert len(loops) == 1, (name, len(loops))      # the un-masked loop: the one without the index select
        assert not any("scratch_" in ln or "buffer_" in ln for ln in loops[0]), name
        packed = sum(ln.startswith("v_pk_") for ln in loops[0])
        print(f"{name}: {len(loops[0])} instructions in the un-masked loop, {packed} of them packed")
