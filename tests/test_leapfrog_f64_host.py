"""LeapFrogSimulator / EulerSimulator(dtype=torch.float64) without a GPU: the C-ABI entries of csrc/direct_leapfrog_f64.hip
are declared and bound, their argument and workspace rules hold, the constructors' errors come before anything touches a
device, the two format classes answer the same calls, accel_f64_kernel has no scratch, no spills and no fp32
intermediate, and the fp64 leapfrog oracle is second order where the GPU test compares with it."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import hermite_f64_oracle as fo
import hermite_oracle as ho
from conftest import ROOT
from nbd import _lib

SRC = os.path.join(ROOT, "nbody-deep-sim_amd", "csrc", "direct_leapfrog_f64.hip")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S"]
ENTRIES = {"nbd_accel_f64_workspace_bytes": 2, "nbd_accel_f64": 9, "nbd_leapfrog_step_f64": 14, "nbd_euler_step_f64": 12}


def test_new_symbols_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbd.h")).read(), flags=re.S)
    L = _lib.lib()
    for name, n_args in ENTRIES.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert decl, f"{name} not declared in include/nbd.h"
        assert len(decl.group(1).split(",")) == n_args
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
        assert len(_lib.SIGNATURES[name][1]) == n_args
    assert L.nbd_abi_version() == _lib.ABI_VERSION == 2          # entries were added, nothing else changed
    from nbd import direct
    for name in ("accel_f64", "leapfrog_step_f64", "euler_step_f64", "accel_f64_workspace"):
        assert callable(getattr(direct, name))


def test_workspace_and_argument_checks_without_a_gpu():
    L = _lib.lib()
    g, s, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for n in (1, 2, 63, 64, 65, 130, 448, 449, 1000, 2100, 5000, 8192, 65536):
        assert L.nbd_hermite_f64_plan(n, g, s, c) == 0
        assert L.nbd_accel_f64_workspace_bytes(n, 0) == s.value * 3 * n * 8
        assert L.nbd_accel_f64_workspace_bytes(n, 0) <= L.nbd_hermite_f64_workspace_bytes(n)   # a simulator's _hws serves
        for slabs in (1, 3, 64):
            assert L.nbd_accel_f64_workspace_bytes(n, slabs) == slabs * 3 * n * 8
    for n, slabs in ((0, 0), (-1, 0), (4, -1), (4, 65)):
        assert L.nbd_accel_f64_workspace_bytes(n, slabs) == 0
    big = 1 << 30
    # nbd_accel_f64(posd, n, eps2, g, acc_out, workspace, bytes, slabs, stream)
    assert L.nbd_accel_f64(None, -1, 0.01, 1.0, None, None, 0, 0, None) == -1
    assert L.nbd_accel_f64(None, 4, 0.01, 1.0, 0x3000, 0x5000, big, 0, None) == -1
    assert L.nbd_accel_f64(0x1010, 4, 0.01, 1.0, 0x3000, 0x5000, big, 0, None) == -1           # 32 bytes
    assert L.nbd_accel_f64(0x1000, 4, 0.01, 1.0, 0x3000, 0x5000, big, 65, None) == -1
    assert L.nbd_accel_f64(0x1000, 4, 0.01, 1.0, 0x3000, 0x5000, big, -1, None) == -1
    assert L.nbd_accel_f64(0x1000, 4, 0.01, 1.0, 0x3000, None, big, 0, None) == -2
    assert L.nbd_accel_f64(0x1000, 4, 0.01, 1.0, 0x3000, 0x5004, big, 0, None) == -2           # 8 bytes
    assert L.nbd_accel_f64(0x1000, 4, 0.01, 1.0, 0x3000, 0x5000, 4 * 3 * 8 - 1, 0, None) == -2
    assert L.nbd_accel_f64(0x1000, 4, 0.01, 1.0, 0x3000, 0x5000, 4 * 3 * 8, 2, None) == -2
    assert L.nbd_accel_f64(None, 0, 0.01, 1.0, None, None, 0, 0, None) == 0
    # nbd_leapfrog_step_f64(pos, vel, acc_in, acc_out, mass, n, dt_half, dt, eps2, g, posd, workspace, bytes, stream)
    assert L.nbd_leapfrog_step_f64(*([None] * 5), 4, 0.05, 0.1, 0.01, 1.0, None, None, 0, None) == -1
    assert L.nbd_leapfrog_step_f64(*([0x1000] * 5), -1, 0.05, 0.1, 0.01, 1.0, 0x1000, 0x1000, big, None) == -1
    assert L.nbd_leapfrog_step_f64(*([0x1000] * 5), 4, 0.05, 0.1, 0.01, 1.0, 0x1010, 0x1000, big, None) == -1
    assert L.nbd_leapfrog_step_f64(*([0x1000] * 5), 4, 0.05, 0.1, 0.01, 1.0, 0x1000, None, 0, None) == -2
    assert L.nbd_leapfrog_step_f64(*([0x1000] * 5), 4, 0.05, 0.1, 0.01, 1.0, 0x1000, 0x1000, 4 * 3 * 8 - 1, None) == -2
    assert L.nbd_leapfrog_step_f64(*([None] * 5), 0, 0.05, 0.1, 0.01, 1.0, None, None, 0, None) == 0
    # nbd_euler_step_f64(pos, vel, acc_out, mass, n, dt, eps2, g, posd, workspace, bytes, stream)
    assert L.nbd_euler_step_f64(*([None] * 4), 4, 0.1, 0.01, 1.0, None, None, 0, None) == -1
    assert L.nbd_euler_step_f64(*([0x1000] * 4), -1, 0.1, 0.01, 1.0, 0x1000, 0x1000, big, None) == -1
    assert L.nbd_euler_step_f64(*([0x1000] * 4), 4, 0.1, 0.01, 1.0, 0x1010, 0x1000, big, None) == -1
    assert L.nbd_euler_step_f64(*([0x1000] * 4), 4, 0.1, 0.01, 1.0, 0x1000, 0x1004, big, None) == -2
    assert L.nbd_euler_step_f64(*([0x1000] * 4), 4, 0.1, 0.01, 1.0, 0x1000, 0x1000, 4 * 3 * 8 - 1, None) == -2
    assert L.nbd_euler_step_f64(*([None] * 4), 0, 0.1, 0.01, 1.0, None, None, 0, None) == 0


def test_constructor_errors_come_before_any_device_work():
    """device="cpu" raises RuntimeError when it is resolved: every error here is raised before that."""
    from galaxify import simulation
    z = np.zeros((4, 3))
    kw = dict(positions=z, velocities=z, masses=np.ones(4), device="cpu")
    for cls in (simulation.LeapFrogSimulator, simulation.EulerSimulator):
        for bad in (torch.float16, torch.bfloat16, torch.int32, "float64", None):
            with pytest.raises(ValueError, match=cls.__name__ + ".*dtype must be"):
                cls(dtype=bad, **kw)
        with pytest.raises(ValueError, match="float64.*process_group"):
            cls(dtype=torch.float64, process_group=object(), **kw)
        with pytest.raises(TypeError, match="unexpected keyword argument 'precision'"):
            cls(precision=torch.float64, **kw)
        with pytest.raises(TypeError, match="unexpected keyword argument 'precision'"):
            cls(dtype=torch.float64, precision=1, **kw)
        for good in (torch.float32, torch.float64):              # the format is accepted; the device is what fails
            with pytest.raises(RuntimeError, match="cpu"):
                cls(dtype=good, **kw)
        # the keyword arrives through **format_kw, it is not a named parameter
        params = inspect.signature(cls.__init__).parameters
        assert "dtype" not in params and params["format_kw"].kind is inspect.Parameter.VAR_KEYWORD
        cls._check_format(torch.float32, object())               # the fp32 step has a range-sharded form
        cls._check_format(torch.float64, None)
        sim = object.__new__(cls)
        assert sim._fmt is simulation._FORMATS[torch.float32]
        sim._fmt, sim._sharded, sim.n = simulation._FORMATS[torch.float64], False, 100
        assert not sim._graph_run_ok(64)                         # run() is eager in float64


def test_format_classes_keep_equal_method_sets():
    from galaxify import simulation
    f32, f64 = simulation._FORMATS[torch.float32], simulation._FORMATS[torch.float64]

    def callables(obj, private):
        return {name for name in dir(type(obj)) if name.startswith("_") == private and not name.startswith("__")
                and callable(getattr(obj, name))}
    assert callables(f32, False) == callables(f64, False) and len(callables(f32, False)) == 12
    for name in ("_base_scratch", "_leapfrog_step", "_euler_step"):
        assert name in callables(f32, True) and name in callables(f64, True)
    assert callables(f32, True) <= callables(f64, True)          # (_Float64 adds its own _scalars)
    assert not f64.capturable and f32.capturable
    # the simulator classes do not ask which format they have
    for cls in (simulation.LeapFrogSimulator, simulation.EulerSimulator):
        text = inspect.getsource(cls)
        for pattern in (r"dtype\s*(==|!=|is\b)", r"(==|!=|\bis|\bis not)\s*torch\.float(32|64)\b",
                        r"isinstance\([^)]*_Float", r"_fmt\s*(==|!=|is\b)", r"(==|!=|\bis|\bis not)\s*_Float"):
            assert not re.search(pattern, text), (cls.__name__, pattern)


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "direct_leapfrog_f64.s")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-o", out, SRC], check=True, capture_output=True)
    return open(out).read()


def _kernel(asm, pattern):
    """(metadata, kernel descriptor, code) of the one kernel whose mangled name matches."""
    names = sorted(set(re.findall(r"\.name:\s+(\S*" + pattern + r"\S*)", asm)))
    names = [nm for nm in names if not nm.endswith(".kd")]
    assert len(names) == 1, names
    meta = asm[asm.index(".name:           " + names[0]):]
    meta = meta[:meta.index(".name:           ", 20) if ".name:           " in meta[20:] else len(meta)]
    desc = asm[asm.index(".amdhsa_kernel " + names[0]):]
    body = asm[asm.index(names[0] + ":"):]
    return meta, desc, body[:body.index(".Lfunc_end")]


def test_accel_kernel_has_no_scratch_and_half_the_lds(asm):
    meta, desc, body = _kernel(asm, "accel_f64_kernel")
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
        assert int(re.search(r"\." + key + r":\s+(\d+)", meta).group(1)) == 0, key
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1)) == 16384     # one streamed array
    assert "v_cvt_f32_f64" not in body                                      # no fp32 intermediate
    assert "v_rsq_f64" in body and "v_fma_f64" in body


@pytest.mark.parametrize("kernel", ["leapfrog_pack_f64_kernel", "leapfrog_finish_f64_kernelILb0E",
                                    "leapfrog_finish_f64_kernelILb1E"])
def test_step_kernels_have_no_scratch_and_round_every_operation(asm, kernel):
    meta, desc, body = _kernel(asm, kernel)
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
        assert int(re.search(r"\." + key + r":\s+(\d+)", meta).group(1)) == 0, key
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1)) == 0
    assert "v_cvt_f32_f64" not in body
    assert "v_fma_f64" not in body and "v_mul_f64" in body and "v_add_f64" in body      # a*b + c rounds twice


def test_leapfrog_oracle_is_second_order_on_the_two_body_orbit():
    """e = 0.5, eps = 0.1, one period: the relative energy error of E = K + 1/2 sum m phi after leapfrog_run falls by
    3.9 to 4.1 per halving of dt from 256 to 4096 steps, and is still far above fp64 rounding at the last."""
    x, v, m, period = ho.two_body(0.5)
    eps2 = 0.1 ** 2
    e0 = fo.energy(x, v, m, 1.0, eps2)
    err = []
    for steps in (256, 512, 1024, 2048, 4096):
        xs, vs = ho.leapfrog_run(x, v, m, period / steps, 1.0, eps2, steps)
        err.append(abs(fo.energy(xs, vs, m, 1.0, eps2) - e0) / abs(e0))
    for k in range(4):
        assert 3.9 < err[k] / err[k + 1] < 4.1, err
    assert 1e-9 < err[0] < 3e-9 and err[-1] > 1e-12
