"""The step loop of variant 2 of the symmetric force (accel_sym2_kernel) in the gfx950 assembly of csrc/direct_force.hip
(no GPU needed: hipcc cross-compiles): per step, 8 targets x 2 sources = 24 v_pk_add_f32, 72 v_pk_fma_f32 (24 of them
the reaction, negated by the modifier), 16 v_pk_mul_f32, 16 v_rsq_f32 and 6 DPP wave_rol:1 moves, at most 2 LDS reads,
next to no s_nop; at most 128 VGPRs (4 waves per SIMD) and no scratch."""
import os
import re
import subprocess
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "nbody-deep-sim_amd", "csrc", "direct_force.hip")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S"]
KERNEL = "_ZN12_GLOBAL__N_117accel_sym2_kernelEPKDv4_fiiiifPf"
PER_STEP = {"v_pk_add_f32": 24, "v_pk_fma_f32": 72, "v_pk_mul_f32": 16, "v_rsq_f32_e32": 16, "v_mov_b32_dpp": 6}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa2") / "direct_force.s")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-o", out, SRC], check=True, capture_output=True)
    return open(out).read()


def _function(asm, name):
    i = asm.index(name + ":")
    return asm[i:asm.index(".Lfunc_end", i)]


def test_sym2_step_instruction_mix(asm):
    parts = re.split(r"\n(\.LBB\d+_\d+):", _function(asm, KERNEL))
    loops = []
    for label, block in zip(parts[1::2], parts[2::2]):
        ins = [ln.strip() for ln in block.split("\n")]
        ins = [ln for ln in ins if ln and not ln.startswith((";", "."))]
        back = [k for k, ln in enumerate(ins) if ln.startswith("s_cbranch") and ln.endswith(" " + label)]
        if back and any("wave_rol:1" in ln for ln in ins):
            loops.append(ins[:back[0] + 1])          # the loop body: up to its own back branch
    assert len(loops) == 1, "one step loop with wave_rol moves"
    ins = loops[0]
    ops = Counter(ln.split()[0] for ln in ins)
    assert ops["v_rsq_f32_e32"] == 16, "one step per loop trip"
    for op, n in PER_STEP.items():
        assert ops[op] == n, (op, ops[op])
    assert all("wave_rol:1" in ln for ln in ins if ln.startswith("v_mov_b32_dpp"))
    assert sum("neg_lo:[1,0,0] neg_hi:[1,0,0]" in ln for ln in ins if ln.startswith("v_pk_fma_f32")) == 24
    assert ops["ds_read_b128"] == 1 and ops["ds_read_b64"] == 1
    assert sum(ln.startswith("ds_") for ln in ins) == 2
    # the targets reach the halves of the packed ops by op_sel, never by copies
    assert not any(ln.startswith(("v_mov_b32_e32", "v_pk_mov_b32")) for ln in ins)
    assert sum(int(ln.split()[1]) + 1 for ln in ins if ln.startswith("s_nop")) <= 2
    assert not any("scratch_" in ln or "buffer_" in ln for ln in ins)


def test_sym2_kernel_resources(asm):
    meta = asm[asm.index(".name:           " + KERNEL):]
    meta = meta[:meta.index(".name:           ", 20) if ".name:           " in meta[20:] else len(meta)]
    vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
    assert scratch == 0 and vgpr <= 128, (vgpr, scratch)
    assert "scratch_store" not in _function(asm, KERNEL)
