"""The block-timestep Hermite integrator without a GPU: the fp64 oracle reduces to the shared-step oracle at max_level 0,
keeps the block condition, and its error falls with eta at the expected rate; the new kernels (gfx950 assembly, hipcc
cross-compiles) keep accel_jerk_kernel's packed-fp32 inner loop with no scratch, no spills and no float atomics; bad C-ABI
arguments are refused before any launch; the dataset CLI accepts --integrator hermite-block and refuses it with
--batch-scenes."""
import ctypes
import importlib.util
import os
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

import block_hermite_oracle as bo
import hermite_oracle as ho
from conftest import PKG, ROOT

SRC = os.path.join(ROOT, "nbody-deep-sim_amd", "csrc", "direct_hermite_block.hip")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S"]
KERNEL = "_ZN12_GLOBAL__N_124accel_jerk_active_kernelILb{m}EEEvPKDv4_fS3_iPKiiiifPf"
PER_SOURCE = {"v_pk_add_f32": 6, "v_pk_fma_f32": 14, "v_pk_mul_f32": 6, "v_rsq_f32_e32": 2}


def test_oracle_max_level_zero_is_the_shared_step():
    for e, eps2 in ((0.5, 0.0), (0.9, 0.0)):
        x, v, m, period = ho.two_body(e)
        got = bo.block_run(x, v, m, period / 64, 1.0, eps2, 12, eta=0.02, max_level=0)
        want = ho.hermite_run(x, v, m, period / 64, 1.0, eps2, 12)
        for a, b in zip((got["x"], got["v"], got["a"], got["j"]), want):
            assert np.array_equal(a, b)
        assert got["block_steps"] == 12 and got["pair_interactions"] == 12 * 4
    x, v, m = bo.planted_binary_sphere(48, 3)
    got = bo.block_run(x, v, m, 1 / 64, 1.0, 1e-4, 3, max_level=0)
    want = ho.hermite_run(x, v, m, 1 / 64, 1.0, 1e-4, 3)
    assert np.array_equal(got["x"], want[0]) and np.array_equal(got["v"], want[1])


def test_oracle_lets_a_lone_body_take_the_whole_interval():
    """n = 1 has a = j = 0: the criterion is +inf (any step), not 0/0 = NaN, so nothing is clamped."""
    r = bo.block_run([[0.3, 0.1, 0.0]], [[0.0, 0.25, 0.0]], [1.0], 0.125, 1.0, 0.0, 3, max_level=6)
    assert r["block_steps"] == 3 and r["clamped"] == 0 and r["levels"].tolist() == [0]
    assert np.array_equal(r["x"], [[0.3, 0.1 + 3 * 0.125 * 0.25, 0.0]])
    assert np.isinf(bo.aarseth(np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 3)), [0.5], 0.02)[0])


def test_oracle_keeps_the_block_condition_with_a_planted_binary():
    K = 8
    x, v, m = bo.planted_binary_sphere(64, 1)
    r = bo.block_run(x, v, m, 1 / 16, 1.0, 0.0, 3, eta=0.02, max_level=K)
    assert len(r["history"]) == r["block_steps"] == len(r["tick_history"])
    ends = 0
    for levels, ticks in zip(r["history"], r["tick_history"]):
        assert levels.min() >= 0 and levels.max() <= K
        assert (ticks % np.left_shift(1, K - levels) == 0).all()          # t_i is a multiple of d_i
        if ticks.min() == 1 << K:
            ends += 1
            assert (ticks == 1 << K).all()
    assert ends == 3 and r["tick_history"][-1].min() == 1 << K              # every body back at 2^K per output step
    assert r["levels"][:2].min() > np.median(r["levels"])                  # the binary runs deeper than the median body


def test_oracle_error_falls_with_eta_on_the_eccentric_orbit():
    """e = 0.9, eps = 0, one period as 4 output steps, max_level 12. The fp64 oracle: 6.0e-5, 2.8e-6, 9.8e-8 at
    eta = 0.04, 0.01, 0.0025 -- a factor of 22 and 28 per 4x in eta (the step ~ sqrt(eta), 4th order: 16 asymptotically)."""
    x0, v0, m, period = ho.two_body(0.9)
    errs = [ho.orbit_error(bo.block_run(x0, v0, m, period / 4, 1.0, 0.0, 4, eta=eta, max_level=12)["x"], x0)
            for eta in (0.04, 0.01, 0.0025)]
    for coarse, fine in zip(errs, errs[1:]):
        assert 18.0 < coarse / fine < 35.0, errs


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "direct_hermite_block.s")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-o", out, SRC], check=True, capture_output=True)
    return open(out).read()


def _function(asm, name):
    i = asm.index(name + ":")
    return asm[i:asm.index(".Lfunc_end", i)]


def _meta(asm, name):
    meta = asm[asm.index(".name:           " + name):]
    return meta[:meta.index(".name:           ", 20) if ".name:           " in meta[20:] else len(meta)]


def _loops(body):
    parts = re.split(r"\n(\.LBB\d+_\d+):", body)
    out = []
    for block in parts[2::2]:
        lines = [ln.strip() for ln in block.split("\n")]
        ins = [ln for ln in lines if ln and not ln.startswith((";", "."))]
        if any(ln.startswith("v_rsq_f32") for ln in ins):
            out.append(ins)
    return out


def test_active_kernel_inner_loop_instruction_mix(asm):
    loops = _loops(_function(asm, KERNEL.format(m=0)))
    assert len(loops) == 1
    ops = Counter(ln.split()[0] for ln in loops[0])
    sources = ops["v_rsq_f32_e32"] // 2
    assert sources == 2
    for op, n in PER_SOURCE.items():
        assert ops[op] == n * sources, (op, ops[op], sources)
    assert ops["s_nop"] == 0 and ops["v_mov_b32_e32"] == 0, ops


@pytest.mark.parametrize("masked", [0, 1])
def test_active_kernel_resources(asm, masked):
    name = KERNEL.format(m=masked)
    meta = _meta(asm, name)
    vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
    spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
    assert scratch == 0 and spill == 0 and vgpr <= 80, (vgpr, spill, scratch)
    assert "global_load_lds_dwordx4" in _function(asm, name)


@pytest.mark.parametrize("kernel", ["hblock_init_kernel", "hblock_schedule_kernel", "hblock_predict_kernel",
                                    "hblock_correct_kernel"])
def test_other_kernels_have_no_scratch(asm, kernel):
    """The scheduler, and the float instantiations (mangled ...kernelIfE...) of hermite_block_kernels.h's templates; the
    double ones: test_block_hermite_f64_host.py. LDS: int[21] of level counts in init, the slab sum's float[4][6][64] in
    the corrector."""
    lds = {"hblock_init_kernel": 84, "hblock_correct_kernel": 6144}.get(kernel)
    suffix = "" if kernel == "hblock_schedule_kernel" else "If"
    names = re.findall(r"\.name:\s+(\S*" + kernel + suffix + r"\S*)", asm)
    assert len(names) == 1
    meta = _meta(asm, names[0])
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1)) == 0
    if lds is not None:
        desc = asm[asm.index(".amdhsa_kernel " + names[0]):]
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1)) == lds


def test_no_float_atomics(asm):
    atomics = [ln.split()[0] for ln in asm.split("\n") if re.match(r"\s*(global|flat|ds|buffer)_atomic", ln)]
    assert all(not re.search(r"_f32|_f64|_pk_", op) for op in atomics), atomics


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    from nbd import _lib
    L = _lib.lib()
    n = 100
    ws_n = L.nbd_hblock_workspace_bytes(n)
    assert ws_n > 0 and L.nbd_hblock_workspace_bytes(0) == 0
    assert L.nbd_hblock_workspace_bytes(2 * n) >= ws_n
    fake = ctypes.c_void_p(1 << 20)                     # never dereferenced: every call below fails its host checks
    odd = ctypes.c_void_p((1 << 20) + 4)
    # null pointers, K outside [0, 20], bad dt / eta
    assert L.nbd_hblock_init_levels(None, None, n, 0.1, 0.02, 4, None, None, None, None) == -1
    assert L.nbd_hblock_init_levels(fake, fake, n, 0.1, 0.02, 21, fake, fake, fake, None) == -1
    assert L.nbd_hblock_init_levels(fake, fake, n, 0.1, 0.02, -1, fake, fake, fake, None) == -1
    assert L.nbd_hblock_init_levels(fake, fake, n, 0.0, 0.02, 4, fake, fake, fake, None) == -1
    assert L.nbd_hblock_schedule(None, n, 4, fake, fake, ws_n, None, None) == -1
    assert L.nbd_hblock_schedule(fake, n, 21, fake, fake, ws_n, None, None) == -1
    assert L.nbd_hblock_schedule(fake, n, 4, None, fake, ws_n, None, None) == -1
    assert L.nbd_hblock_schedule(fake, n, 4, fake, fake, 64, None, None) == -2                    # short workspace
    assert L.nbd_hblock_schedule(fake, n, 4, fake, odd, ws_n, None, None) == -2                   # misaligned workspace
    assert L.nbd_hblock_predict_f32(fake, fake, fake, fake, fake, fake, n, 4, 0.1, fake, odd, fake, None) == -1
    assert L.nbd_hblock_predict_f32(fake, fake, fake, fake, fake, fake, n, 4, 0.1, fake, fake, odd, None) == -1
    assert L.nbd_hblock_predict_f32(fake, None, fake, fake, fake, fake, n, 4, 0.1, fake, fake, fake, None) == -1
    assert L.nbd_hblock_force_f32(fake, fake, n, n + 1, 0.01, fake, ws_n, None) == -1             # n_act > n
    assert L.nbd_hblock_force_f32(odd, fake, n, n, 0.01, fake, ws_n, None) == -1
    assert L.nbd_hblock_force_f32(fake, fake, n, n, 0.01, fake, 64, None) == -2
    assert L.nbd_hblock_correct_f32(fake, fake, fake, fake, fake, fake, fake, n, n + 1, 4, 0.1, 0.02, 1.0, fake,
                                    fake, fake, ws_n, None) == -1
    assert L.nbd_hblock_correct_f32(fake, fake, fake, fake, fake, fake, None, n, n, 4, 0.1, 0.02, 1.0, fake,
                                    fake, fake, ws_n, None) == -1
    assert L.nbd_hblock_correct_f32(fake, fake, fake, fake, fake, fake, fake, n, n, 4, 0.1, 0.02, 1.0, fake,
                                    odd, fake, ws_n, None) == -1
    assert L.nbd_hblock_correct_f32(fake, fake, fake, fake, fake, fake, fake, n, n, 4, 0.1, 0.02, 1.0, fake,
                                    fake, None, ws_n, None) == -2
    assert L.nbd_hblock_step_f32(fake, fake, fake, fake, fake, fake, fake, n, 0, 4, 0.1, 0.02, 0.01, 1.0, fake,
                                 fake, fake, fake, ws_n, None) == -1                              # nothing active
    assert L.nbd_hblock_step_f32(fake, fake, fake, fake, fake, fake, fake, n, n, 4, 0.1, 0.02, 0.01, 1.0, fake,
                                 fake, odd, fake, ws_n, None) == -1
    assert L.nbd_accel_jerk_active_f32(fake, fake, n, fake, n + 1, 0.01, 1.0, fake, fake, fake, ws_n, None) == -1
    assert L.nbd_accel_jerk_active_f32(fake, fake, n, None, 5, 0.01, 1.0, fake, fake, fake, ws_n, None) == -1
    assert L.nbd_accel_jerk_active_f32(fake, fake, n, fake, 5, 0.01, 1.0, fake, fake, fake, 64, None) == -2
    # an empty active list is a no-op
    assert L.nbd_accel_jerk_active_f32(None, None, n, None, 0, 0.01, 1.0, None, None, None, 0, None) == 0


def _cli():
    spec = importlib.util.spec_from_file_location("s01_hblock", os.path.join(PKG, "s01-dataset-generation.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_accepts_hermite_block():
    args = _cli().build_parser().parse_args(["--n-bodies", "5", "--integrator", "hermite-block", "--output", "x.csv"])
    assert args.integrator == "hermite-block"


def test_cli_refuses_hermite_block_with_batch_scenes(tmp_path, capsys):
    out = tmp_path / "x.csv"
    with pytest.raises(SystemExit) as exc:
        _cli().main(["--n-bodies", "5", "--integrator", "hermite-block", "--output", str(out), "--batch-scenes"])
    assert exc.value.code == 2
    assert "--integrator hermite-block cannot be combined with --batch-scenes" in capsys.readouterr().err
    assert not out.exists()
