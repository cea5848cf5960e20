"""The 4th-order Hermite integrator without a GPU: the fp64 oracle's jerk is the time derivative of its acceleration and
the oracle converges at 4th order; the new kernels (gfx950 assembly, hipcc cross-compiles) keep the packed-fp32 inner
loop with no scratch and no spills; the dataset CLI accepts --integrator hermite and refuses it with --batch-scenes."""
import importlib.util
import os
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

import hermite_oracle as ho
from conftest import PKG, ROOT

SRC = os.path.join(ROOT, "nbody-deep-sim_amd", "csrc", "direct_hermite.hip")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S"]
KERNEL = "_ZN12_GLOBAL__N_117accel_jerk_kernelILb{m}ELi{ku}EEEvPKDv4_fS3_iiifPf"
# per source and pair of targets in the un-masked loop: 6 differences (add), r^2 and r.v (5 fma + 1 mul), s^2, s^3, the
# mass splat, r.v s^2 and c (5 mul), a, w dv and c dr (9 fma): 26 packed ops
PER_SOURCE = {"v_pk_add_f32": 6, "v_pk_fma_f32": 14, "v_pk_mul_f32": 6, "v_rsq_f32_e32": 2}


def _plummer(n, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 3)), 0.3 * rng.normal(size=(n, 3)), rng.uniform(0.5, 1.5, n) / n


@pytest.mark.parametrize("eps2", [0.0, 0.01])
def test_oracle_jerk_is_derivative_of_acceleration(eps2):
    x, v, m = _plummer(40, 3)
    _, j = ho.accel_jerk(x, v, m, 1.3, eps2)
    h = 1e-4
    ap, _ = ho.accel_jerk(x + h * v, v, m, 1.3, eps2)
    am, _ = ho.accel_jerk(x - h * v, v, m, 1.3, eps2)
    fd = (ap - am) / (2 * h)
    assert np.abs(fd - j).max() < 1e-6 * np.abs(j).max()


def test_oracle_converges_at_fourth_order_on_two_body_orbit():
    x0, v0, m, period = ho.two_body(0.5)
    errs = [ho.orbit_error(ho.hermite_run(x0, v0, m, period / k, 1.0, 0.0, k)[0], x0) for k in (128, 256, 512)]
    for coarse, fine in zip(errs, errs[1:]):
        assert 14.0 < coarse / fine < 22.0, errs           # 2^4 = 16


def test_oracle_hermite_step_conserves_momentum():
    x, v, m = _plummer(64, 4)
    a, j = ho.accel_jerk(x, v, m, 1.0, 0.01)
    assert np.abs((m[:, None] * a).sum(0)).max() < 1e-12 and np.abs((m[:, None] * j).sum(0)).max() < 1e-12
    x1, v1, _, _ = ho.hermite_step(x, v, a, j, m, 0.01, 1.0, 0.01)
    assert np.abs((m[:, None] * (v1 - v)).sum(0)).max() < 1e-14


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "direct_hermite.s")
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


def test_accel_jerk_inner_loop_instruction_mix(asm):
    """The default (KU = 2) un-masked loop: 26 packed ops + 2 v_rsq_f32 per source, the mass splat folded into op_sel,
    the rsq's back to back with no s_nop padding, one position and one velocity LDS read per source."""
    loops = _loops(_function(asm, KERNEL.format(m=0, ku=2)))
    assert len(loops) == 1
    ins = loops[0]
    ops = Counter(ln.split()[0] for ln in ins)
    sources = ops["v_rsq_f32_e32"] // 2
    assert sources == 2
    for op, n in PER_SOURCE.items():
        assert ops[op] == n * sources, (op, ops[op], sources)
    assert ops["s_nop"] == 0 and ops["v_mov_b32_e32"] == 0, ops
    assert sum("op_sel:[1,0] op_sel_hi:[1,1]" in ln for ln in ins if ln.startswith("v_pk_mul_f32")) == sources
    assert sum(ln.startswith("ds_read") for ln in ins) == 2 * sources
    assert not any("scratch_" in ln or "buffer_" in ln for ln in ins)


@pytest.mark.parametrize("masked", [0, 1])
@pytest.mark.parametrize("ku,max_vgpr", [(2, 80), (4, 96)])
def test_accel_jerk_kernel_resources(asm, masked, ku, max_vgpr):
    name = KERNEL.format(m=masked, ku=ku)
    meta = _meta(asm, name)
    vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
    spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
    desc = asm[asm.index(".amdhsa_kernel " + name):]
    lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1))
    assert scratch == 0 and spill == 0 and vgpr <= max_vgpr, (vgpr, spill, scratch)
    assert lds == 16384
    body = _function(asm, name)
    assert "scratch_store" not in body and "global_load_lds_dwordx4" in body
    if masked == 0 or ku == 2:
        assert any(ln.split()[0] == "v_pk_fma_f32" for ins in _loops(body) for ln in ins)


@pytest.mark.parametrize("kernel", ["hermite_predict_kernel", "hermite_correct_kernel"])
def test_step_kernels_have_no_scratch(asm, kernel):
    """The float instantiations (mangled ...kernelIfE...) of hermite_kernels.h's two O(N) kernels; the double ones:
    test_hermite_f64_host.py. The corrector's LDS is the slab sum's float[4][6][64]."""
    lds = {"hermite_predict_kernel": 0, "hermite_correct_kernel": 6144}[kernel]
    names = re.findall(r"\.name:\s+(\S*" + kernel + r"If\S*)", asm)
    assert len(names) == 1
    meta = _meta(asm, names[0])
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1)) == 0
    desc = asm[asm.index(".amdhsa_kernel " + names[0]):]
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1)) == lds


def _cli():
    spec = importlib.util.spec_from_file_location("s01_hermite", os.path.join(PKG, "s01-dataset-generation.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_accepts_hermite():
    args = _cli().build_parser().parse_args(["--n-bodies", "5", "--integrator", "hermite", "--output", "x.csv"])
    assert args.integrator == "hermite"


def test_cli_refuses_hermite_with_batch_scenes(tmp_path, capsys):
    out = tmp_path / "x.csv"
    with pytest.raises(SystemExit) as exc:
        _cli().main(["--n-bodies", "5", "--integrator", "hermite", "--output", str(out), "--batch-scenes"])
    assert exc.value.code == 2
    assert "--batch-scenes" in capsys.readouterr().err
    assert not out.exists()
