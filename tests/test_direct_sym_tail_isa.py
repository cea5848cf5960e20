"""accel_sym2_tail_kernel (the tile pairs of accel_sym2_kernel with the diagonal blocks as trailing workgroups of the same
launch) in the gfx950 assembly of csrc/direct_force.hip (no GPU needed: hipcc cross-compiles): its one wave_rol loop is the
step loop of accel_sym2_kernel with the same per-step mix (24 v_pk_add_f32, 72 v_pk_fma_f32, 16 v_pk_mul_f32, 16
v_rsq_f32, 6 DPP wave_rol:1 moves, two LDS reads, at most 2 s_nop states) and no global load in it; at most 128 VGPRs (4
waves per SIMD), no scratch, at most 80 KiB of LDS (two workgroups per CU)."""
import os
import re
import subprocess
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "nbody-deep-sim_amd", "csrc", "direct_force.hip")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S"]
KERNEL = "_ZN12_GLOBAL__N_122accel_sym2_tail_kernelEPKDv4_fiifPf"
PER_STEP = {"v_pk_add_f32": 24, "v_pk_fma_f32": 72, "v_pk_mul_f32": 16, "v_rsq_f32_e32": 16, "v_mov_b32_dpp": 6}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa_tail") / "direct_force.s")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-o", out, SRC], check=True, capture_output=True)
    return open(out).read()


def _function(asm, name):
    i = asm.index(name + ":")
    return asm[i:asm.index(".Lfunc_end", i)]


def _loops(asm):
    """[(instructions up to the loop's own back branch)] of every single-block loop of the kernel"""
    parts = re.split(r"\n(\.LBB\d+_\d+):", _function(asm, KERNEL))
    loops = []
    for label, block in zip(parts[1::2], parts[2::2]):
        ins = [ln.strip() for ln in block.split("\n")]
        ins = [ln for ln in ins if ln and not ln.startswith((";", "."))]
        back = [k for k, ln in enumerate(ins) if ln.startswith("s_cbranch") and ln.endswith(" " + label)]
        if back:
            loops.append(ins[:back[0] + 1])
    return loops


def test_sym_tail_step_instruction_mix(asm):
    loops = [ins for ins in _loops(asm) if any("wave_rol:1" in ln for ln in ins)]
    assert len(loops) == 1, "one step loop with wave_rol moves: one copy of the walk"
    ins = loops[0]
    ops = Counter(ln.split()[0] for ln in ins)
    assert ops["v_rsq_f32_e32"] == 16, "one step per loop trip"
    for op, n in PER_STEP.items():
        assert ops[op] == n, (op, ops[op])
    assert all("wave_rol:1" in ln for ln in ins if ln.startswith("v_mov_b32_dpp"))
    assert sum("neg_lo:[1,0,0] neg_hi:[1,0,0]" in ln for ln in ins if ln.startswith("v_pk_fma_f32")) == 24
    assert ops["ds_read_b128"] == 1 and ops["ds_read_b64"] == 1
    assert sum(ln.startswith("ds_") for ln in ins) == 2
    assert not any(ln.startswith(("v_mov_b32_e32", "v_pk_mov_b32")) for ln in ins)
    assert sum(int(ln.split()[1]) + 1 for ln in ins if ln.startswith("s_nop")) <= 2
    assert not any(ln.startswith(("global_load", "flat_load")) for ln in ins), "no global load in the step loop"
    assert not any("scratch_" in ln or "buffer_" in ln for ln in ins)


def test_sym_tail_diagonal_walk_is_the_unmasked_block_loop(asm):
    """The trailing workgroups run accel_body<8, true> unmasked: every other loop with a v_rsq_f32 (hipcc may unroll the
    walk over a wave's four chunks) is the block loop of 8 sources x 2 targets (16 v_rsq_f32, 11 packed ops per source: no
    per-source mass multiply) and none is the index-masked loop (no v_cndmask)."""
    loops = [ins for ins in _loops(asm) if not any("wave_rol:1" in ln for ln in ins)
             and any(ln.startswith("v_rsq_f32") for ln in ins)]
    assert loops, "the source loop of the diagonal blocks"
    for ins in loops:
        ops = Counter(ln.split()[0] for ln in ins)
        assert ops["v_rsq_f32_e32"] == 16
        assert ops["v_pk_add_f32"] + ops["v_pk_fma_f32"] + ops["v_pk_mul_f32"] == 8 * 11
        assert not any(ln.startswith("v_cndmask") for ln in ins)


def test_sym_tail_kernel_resources(asm):
    meta = asm[asm.index(".name:           " + KERNEL):]
    meta = meta[:meta.index(".name:           ", 20) if ".name:           " in meta[20:] else len(meta)]
    vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
    # the metadata keys of a kernel are sorted: its .group_segment_fixed_size is the last one in front of its .name
    before = asm[:asm.index(".name:           " + KERNEL)]
    lds = int(re.match(r"\.group_segment_fixed_size:\s+(\d+)", before[before.rindex(".group_segment_fixed_size:"):]).group(1))
    assert scratch == 0 and vgpr <= 128, (vgpr, scratch)
    assert 0 < lds <= 80 * 1024, lds
    assert "scratch_store" not in _function(asm, KERNEL)
