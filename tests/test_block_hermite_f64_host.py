"""BlockHermiteSimulator(dtype=torch.float64) without a GPU: the fixtures of test_block_hermite_f64_gpu.py are pinned on the
CPU (their criterion values keep clear of every level boundary, so the GPU must choose the oracle's levels; permuting
the bodies never changes a level history), the fp64 block oracle reaches the error on the eccentric orbit that the fp32
mode cannot, the new C-ABI entries are declared, bound and refuse bad arguments before any launch, the new kernels have
no scratch, no spills and no float atomics, and the constructor's dtype check comes before any device work."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import block_hermite_f64_cases as bc
from conftest import ROOT
from nbd import _lib

ENTRIES = ("nbd_hblock_f64_workspace_bytes", "nbd_hblock_init_levels_f64", "nbd_hblock_predict_f64",
           "nbd_hblock_force_f64", "nbd_hblock_correct_f64", "nbd_hblock_step_f64", "nbd_accel_jerk_active_f64")
SRC = os.path.join(ROOT, "nbody-deep-sim_amd", "csrc", "direct_hermite_block_f64.hip")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S"]
# the two instantiations of the force kernel (the mangled name carries the order), the double instantiations of
# hermite_block_kernels.h's templates (the float ones: test_block_hermite_host.py) and the 6th order's O(N) kernels
FORCE4, FORCE6 = "active_force_f64_kernelINS_6Order4E", "active_force_f64_kernelINS_6Order6E"
KERNELS = (FORCE4, FORCE6, "hblock_init_kernelId", "hblock_predict_kernelId", "hblock_correct_kernelId",
           "hblock6_predict_kernel", "hblock6_correct_kernel")
# int[21] of level counts; one thread per row: none; [wave][buffer][array][128] quads of two resp. three source arrays
LDS = {"hblock_init_kernelId": 84, "hblock_correct_kernelId": 0, FORCE4: 32768, FORCE6: 49152}


@pytest.mark.parametrize("eps", [0.0, 0.01])
def test_fixture_margins_and_permuted_level_histories(eps):
    """dt = 1/32, eta = 0.02, max_level 10. Measured: margin 2.5e-3 (eps = 0) / 1.9e-3 (eps = 0.01) over one output step,
    9.4e-5 / 1.3e-4 over four; a permutation moves a criterion value by ~1e-11 of itself, far inside those margins."""
    for steps, floor in ((1, 1e-3), (4, 1e-5)):
        ref = bc.planted_run(eps, steps)
        assert ref["margin"] >= floor, (eps, steps, ref["margin"])
        assert ref["clamped"] == 0
        for seed in bc.PERM_SEEDS:
            prm = bc.planted_run_permuted(eps, steps, seed)
            assert prm["block_steps"] == ref["block_steps"] and prm["pair_interactions"] == ref["pair_interactions"]
            assert len(prm["history"]) == len(ref["history"])
            assert all(np.array_equal(a, b) for a, b in zip(prm["history"], ref["history"])), (eps, steps, seed)
            assert abs(prm["margin"] - ref["margin"]) <= 1e-6 * ref["margin"]
    x, v, m = bc.planted(eps)
    for a in (x, v, m):
        assert not np.any(a.astype(np.float32).astype(np.float64) == a)
    assert ref["levels"][:2].min() > np.median(ref["levels"])           # the binary runs deeper than the median body


def test_oracle_on_the_eccentric_orbit_goes_below_the_fp32_floor():
    """e = 0.9, eps = 0, one period as 4 output steps, eta = 0.000625, max_level 16: 5.1e-9 at 5 668 pair interactions,
    nothing clamped, every criterion value at least 1e-4 (relative) from a level boundary. The fp32 mode's floor on this
    orbit is ~1e-5 (test_block_hermite_gpu.py)."""
    r = bc.orbit_run()
    assert r["err"] < 1e-8, r["err"]
    assert r["clamped"] == 0 and r["margin"] >= 1e-6, (r["clamped"], r["margin"])
    assert r["pair_interactions"] == 5668 and r["levels"].max() <= bc.ORBIT_K


def test_new_symbols_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbd.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared in include/nbd.h"
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert L.nbd_abi_version() == _lib.ABI_VERSION == 2          # entries were added, nothing else changed


def _plan_slabs(n, n_act):
    """The plan of n_act targets under n sources, restated: ~1024 workgroups, every wave keeps a chunk, at most 64 slabs."""
    groups, chunks = -(-n_act // 64), -(-n // 64)
    return max(1, min(-(-1024 // groups), chunks // 4, 64))


def test_workspace_sizes_without_a_gpu():
    L = _lib.lib()
    g, s, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert L.nbd_hblock_f64_workspace_bytes(0) == 0 and L.nbd_hblock_f64_workspace_bytes(-3) == 0
    for n in (1, 2, 63, 64, 65, 130, 449, 1000, 5000, 65536):
        act = -(-n // 8) * 32                                    # the list, padded so that the slab part is 32-byte aligned
        most = max(_plan_slabs(n, n_act) * n_act for n_act in range(1, n + 1))
        assert L.nbd_hblock_f64_workspace_bytes(n) == act + most * 6 * 8, n
        assert L.nbd_hermite_f64_plan(n, g, s, c) == 0 and s.value == _plan_slabs(n, n)      # all active: the shared plan
        assert L.nbd_hblock_f64_workspace_bytes(n) >= act + L.nbd_hermite_f64_workspace_bytes(n)
    assert _plan_slabs(5000, 70) == 19 and _plan_slabs(65536, 128) == 64 and _plan_slabs(130, 1) == 1


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    L = _lib.lib()
    n = 100
    ws_n = L.nbd_hblock_f64_workspace_bytes(n)
    fake = ctypes.c_void_p(1 << 20)                     # never dereferenced: every call below fails its host checks
    odd = ctypes.c_void_p((1 << 20) + 16)               # 16-byte aligned only: rows and workspace need 32
    assert L.nbd_hblock_init_levels_f64(None, None, n, 0.1, 0.02, 4, None, None, None, None) == -1
    assert L.nbd_hblock_init_levels_f64(fake, fake, n, 0.1, 0.02, 21, fake, fake, fake, None) == -1
    assert L.nbd_hblock_init_levels_f64(fake, fake, n, 0.1, 0.02, -1, fake, fake, fake, None) == -1
    assert L.nbd_hblock_init_levels_f64(fake, fake, n, 0.0, 0.02, 4, fake, fake, fake, None) == -1
    assert L.nbd_hblock_init_levels_f64(fake, fake, n, 0.1, 0.0, 4, fake, fake, fake, None) == -1
    assert L.nbd_hblock_init_levels_f64(None, None, 0, 0.1, 0.02, 4, None, None, fake, None) == 0
    assert L.nbd_hblock_predict_f64(fake, fake, fake, fake, fake, fake, n, 4, 0.1, fake, odd, fake, None) == -1
    assert L.nbd_hblock_predict_f64(fake, fake, fake, fake, fake, fake, n, 4, 0.1, fake, fake, odd, None) == -1
    assert L.nbd_hblock_predict_f64(fake, None, fake, fake, fake, fake, n, 4, 0.1, fake, fake, fake, None) == -1
    assert L.nbd_hblock_predict_f64(fake, fake, fake, fake, fake, fake, n, 21, 0.1, fake, fake, fake, None) == -1
    assert L.nbd_hblock_force_f64(fake, fake, n, n + 1, 0.01, fake, ws_n, None) == -1             # n_act > n
    assert L.nbd_hblock_force_f64(odd, fake, n, n, 0.01, fake, ws_n, None) == -1
    assert L.nbd_hblock_force_f64(fake, fake, n, n, 0.01, fake, 64, None) == -2
    assert L.nbd_hblock_force_f64(fake, fake, n, n, 0.01, odd, ws_n, None) == -2
    assert L.nbd_hblock_force_f64(fake, fake, n, 0, 0.01, fake, ws_n, None) == 0                  # nothing listed: a no-op
    assert L.nbd_hblock_correct_f64(fake, fake, fake, fake, fake, fake, fake, n, n + 1, 4, 0.1, 0.02, 1.0, fake,
                                    fake, fake, ws_n, None) == -1
    assert L.nbd_hblock_correct_f64(fake, fake, fake, fake, fake, fake, None, n, n, 4, 0.1, 0.02, 1.0, fake,
                                    fake, fake, ws_n, None) == -1
    assert L.nbd_hblock_correct_f64(fake, fake, fake, fake, fake, fake, fake, n, n, 4, 0.1, 0.02, 1.0, fake,
                                    odd, fake, ws_n, None) == -1
    assert L.nbd_hblock_correct_f64(fake, fake, fake, fake, fake, fake, fake, n, n, 4, 0.1, 0.02, 1.0, fake,
                                    fake, None, ws_n, None) == -2
    assert L.nbd_hblock_correct_f64(fake, fake, fake, fake, fake, fake, fake, n, 0, 4, 0.1, 0.02, 1.0, fake,
                                    fake, fake, ws_n, None) == 0
    assert L.nbd_hblock_step_f64(fake, fake, fake, fake, fake, fake, fake, n, 0, 4, 0.1, 0.02, 0.01, 1.0, fake,
                                 fake, fake, fake, ws_n, None) == -1                              # nothing active
    assert L.nbd_hblock_step_f64(fake, fake, fake, fake, fake, fake, fake, n, n, 4, 0.1, 0.02, 0.01, 1.0, fake,
                                 fake, odd, fake, ws_n, None) == -1
    assert L.nbd_accel_jerk_active_f64(fake, fake, n, fake, n + 1, 0.01, 1.0, fake, fake, fake, ws_n, 0, None) == -1
    assert L.nbd_accel_jerk_active_f64(fake, fake, n, None, 5, 0.01, 1.0, fake, fake, fake, ws_n, 0, None) == -1
    assert L.nbd_accel_jerk_active_f64(fake, fake, n, fake, 5, 0.01, 1.0, fake, fake, fake, ws_n, 65, None) == -1
    assert L.nbd_accel_jerk_active_f64(fake, fake, n, fake, 5, 0.01, 1.0, fake, fake, fake, ws_n, -1, None) == -1
    assert L.nbd_accel_jerk_active_f64(fake, fake, n, fake, 5, 0.01, 1.0, fake, fake, fake, 64, 0, None) == -2
    assert L.nbd_accel_jerk_active_f64(fake, fake, n, fake, 5, 0.01, 1.0, fake, fake, fake, 416 + 2 * 6 * 5 * 8 - 1, 2,
                                       None) == -2                                                # the explicit split's need
    assert L.nbd_accel_jerk_active_f64(None, None, n, None, 0, 0.01, 1.0, None, None, None, 0, 0, None) == 0


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "direct_hermite_block_f64.s")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-o", out, SRC], check=True, capture_output=True)
    return open(out).read()


def _meta(asm, kernel):
    names = re.findall(r"\.name:\s+(\S*" + kernel + r"\S*)", asm)
    assert len(names) == 1, (kernel, names)
    meta = asm[asm.index(".name:           " + names[0]):]
    return names[0], meta[:meta.index(".name:           ", 20) if ".name:           " in meta[20:] else len(meta)]


@pytest.mark.parametrize("kernel", KERNELS)
def test_new_kernels_have_no_scratch_and_no_spills(asm, kernel):
    name, meta = _meta(asm, kernel)
    num = lambda key: int(re.search(key + r":\s+(\d+)", meta).group(1))      # noqa: E731
    assert num(r"\.private_segment_fixed_size") == 0 and num(r"\.vgpr_spill_count") == 0
    assert num(r"\.sgpr_spill_count") == 0
    if kernel in LDS:
        desc = asm[asm.index(".amdhsa_kernel " + name):]
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1)) == LDS[kernel]
    if kernel == FORCE6:
        assert num(r"\.vgpr_count") <= 168              # 3 workgroups per CU (48 KiB of LDS each), as force_f64_kernel<Order6>
    if kernel == FORCE4:
        assert num(r"\.vgpr_count") <= 96               # 5 workgroups per CU (32 KiB of LDS each), as force_f64_kernel<Order4>
        body = asm[asm.index(name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "global_load_lds_dwordx4" in body and "v_rsq_f64" in body
        assert "v_rsq_f32" not in body and "v_cvt_f32_f64" not in body           # no fp32 intermediate


def test_no_float_atomics_and_one_copy_of_the_wave_body(asm):
    atomics = [ln.split()[0] for ln in asm.split("\n") if re.match(r"\s*(global|flat|ds|buffer)_atomic", ln)]
    assert atomics and all(not re.search(r"_f32|_f64|_pk_", op) for op in atomics), atomics
    csrc = os.path.dirname(SRC)
    units = {f: open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith((".hip", ".h"))}
    for what in ("void walk_f64(", "struct AccelJerkPair", "double rsqrt_f64(", "F64Plan plan_f64(int n, int n_tgt)"):
        assert [f for f, text in units.items() if what in text] == ["hermite_f64_kernels.h"], what
    for what in ("double criterion(", "int wanted_level(", "double norm3(", "enum { kTNext", "void hblock_relevel(",
                 "void hblock_init_kernel(", "void hblock_predict_kernel(", "void hblock_correct_kernel("):
        assert [f for f, text in units.items() if what in text] == ["hermite_block_kernels.h"], what
    # the O(N) stages of both formats: one row predictor, one row corrector, one slab-order sum, two templated kernels
    for what in ("PosVel3<T> hermite_predict_row(", "Corrected<T> hermite_correct_row(", "void slab_order_sum(",
                 "void hermite_predict_kernel(", "void hermite_correct_kernel(", "struct HermiteFmt<double>"):
        assert [f for f, text in units.items() if what in text] == ["hermite_kernels.h"], what
    # ... which the range-sharded units launch too (with a row stride, without the packed store): their only kernel is
    # the pair kernel, and one struct describes a rank's plan in both formats
    for f in ("direct_hermite_shard.hip", "direct_hermite_shard_f64.hip"):
        assert units[f].count("__global__") == 1, f
    assert sum(text.count("struct HShardPlan") for text in units.values()) == 1
    # the 6th order's two O(N) kernels sit beside their row functions, for the un-sharded and the sharded unit
    for what in ("void hermite6_predict_kernel(", "void hermite6_finish_kernel("):
        assert [f for f, text in units.items() if what in text] == ["hermite6_f64_kernels.h"], what
    # the batched shared-step units: one templated predictor and one corrector for both formats, and no shard or batch
    # unit calls the row predictor from a kernel of its own
    for what in ("void batch_hermite_predict_kernel(", "void batch_hermite_correct_kernel("):
        assert [f for f, text in units.items() if what in text] == ["hermite_batch_kernels.h"], what
        assert units["hermite_batch_kernels.h"].count(what) == 1, what
    for f in ("direct_hermite_shard.hip", "direct_hermite_shard_f64.hip", "direct_batch_hermite.hip",
              "direct_batch_hermite_f64.hip"):
        assert "hermite_predict_row(" not in units[f], f
    # the two orders as types and the check of an order's packed arrays: the order header's, for every float64 unit
    for what in ("struct Order4", "struct Order6", "bool bad_rows("):
        assert [f for f, text in units.items() if what in text] == ["hermite_orders_f64.h"], what
    # the shared-step batched unit states its parameter rows once, for both orders (the block-timestep batched unit has
    # a table of its own, NBD_BATCH_HBLOCK_PARAM_ROWS)
    assert units["direct_batch_hermite_f64.hip"].count("enum ParamRow") == 1
    assert sorted(f for f, text in units.items() if "enum ParamRow" in text) == [
        "direct_batch_hermite_block_f64.hip", "direct_batch_hermite_f64.hip"]
    for f in ("direct_hermite_f64.hip", "direct_hermite_block_f64.hip"):      # no slab loop written out in an fp64 unit
        assert "+= slabs[" not in units[f], f
    # one float64 block unit for both orders, and one copy of its workspace arithmetic and of the force launch: each is
    # defined once, under no other spelling (the fp32 unit, direct_hermite_block.hip, has a step_bytes and a launch_active
    # of its own, over its own plan and wave body, and no slab_rows)
    for what in ("slab_rows", "step_bytes", "launch_active"):
        defs = {f: re.findall(r"^(?:inline )?(?:size_t|int) (%s\w*)\(" % what, text, flags=re.M)
                for f, text in units.items() if f != "direct_hermite_block.hip"}
        assert {f: d for f, d in defs.items() if d} == {"direct_hermite_block_f64.hip": [what]}, (what, defs)


def test_dtype_errors_come_before_any_device_work():
    from galaxify import simulation
    z = np.zeros((4, 3))
    kw = dict(positions=z, velocities=z, masses=np.ones(4))
    for bad in (torch.float16, torch.bfloat16, torch.int32, "float64", None):
        with pytest.raises(ValueError, match="dtype"):
            simulation.BlockHermiteSimulator(dtype=bad, **kw)
    for dtype in (torch.float32, torch.float64):
        with pytest.raises(ValueError, match="process_group"):
            simulation.BlockHermiteSimulator(dtype=dtype, process_group=object(), **kw)
    # the keyword is HermiteSimulator's: the block class hands it on, with that class's default, and so does not accept
    # a name HermiteSimulator does not know
    params = inspect.signature(simulation.BlockHermiteSimulator.__init__).parameters
    assert any(q.kind is inspect.Parameter.VAR_KEYWORD for q in params.values())
    assert inspect.signature(simulation.HermiteSimulator.__init__).parameters["dtype"].default is torch.float32
    with pytest.raises(TypeError, match="no_such_keyword"):
        simulation.BlockHermiteSimulator(no_such_keyword=1, **kw)
    sim = object.__new__(simulation.BlockHermiteSimulator)
    sim._fmt, sim._sharded, sim.n = simulation._FORMATS[torch.float64], False, 100
    assert not sim._graph_run_ok(64)                     # run() stays eager in this mode too
