"""The backward of the Hermite force (csrc/direct_hermite_grad.hip) next to the force itself and to the backward of the
acceleration on the MI355X, in one process.

  python tools/bench_accel_jerk_vjp.py [--out FILE]            (default: profiles/r18_accel_jerk_vjp.json)

1. HIP-event times (median of 5 batches) at N = 4 096, 16 384, 65 536, float32 and float64: nbd_accel_jerk_vjp_* with
   both cotangents, with the jerk's alone (only the new kernels run) and with the acceleration's alone (nbd_accel_vjp_*
   and nothing else), all three gradients asked for; the force nbd_accel_jerk_* and nbd_accel_vjp_* of the same dtype; the
   ratios to the force next to the instruction model's (packed ops + v_rsq_f32 per source and pair of targets in the
   un-masked fp32 loops, counted on the gfx950 assembly).
2. VGPRs, waves per SIMD, scratch and LDS of the new kernels, and the instruction count of the un-masked fp32 loop, read
   from the gfx950 assembly (hipcc -S).
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nbody-deep-sim_amd")
CSRC = os.path.join(PKG, "csrc")
sys.path.insert(0, PKG)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off"]
SIZES = (4096, 16384, 65536)
KU = 2                                    # sources per trip of the un-masked fp32 loop (kHvjpKU)
PACKED_FORCE, PACKED_VJP = 26, 29         # K-H's force and the acceleration's backward (their header comments)


def assembly():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "direct_hermite_grad.s")
        subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-S", "-o", out,
                        os.path.join(CSRC, "direct_hermite_grad.hip")], check=True, capture_output=True)
        return open(out).read()


def resources(asm):
    """{kernel: {vgprs, waves_per_simd, scratch_bytes, lds_bytes}} of csrc/direct_hermite_grad.hip."""
    res = {}
    for blk in asm[asm.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
        short = re.search(r"(accel_jerk_vjp\w*?kernel)(ILb([01])E)?", name)
        key = short.group(1) + ({"0": "<unmasked>", "1": "<masked>"}.get(short.group(3), ""))
        res[key] = {"vgprs": vgpr, "waves_per_simd": min(8, 512 // (-(-vgpr // 8) * 8)),
                    "scratch_bytes": int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)),
                    "lds_bytes": int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))}
    return res


def unmasked_loop(asm):
    """The un-masked pair loop of the fp32 walk (the innermost loop with a v_rsq_f32 and no index select): instruction
    counts per source and pair of targets."""
    name = next(re.search(r"\.name:\s+(\S+)", ln).group(1) for ln in asm.splitlines()
                if ".name:" in ln and "accel_jerk_vjp_kernelILb0E" in ln)
    i = asm.index(name + ":")
    parts = re.split(r"\n(\.LBB\d+_\d+):", asm[i:asm.index(".Lfunc_end", i)])
    for label, block in zip(parts[1::2], parts[2::2]):
        ins = [ln.strip() for ln in block.split("\n")]
        ins = [ln for ln in ins if ln and not ln.startswith((";", "."))]
        back = [k for k, ln in enumerate(ins) if ln.startswith("s_cbranch") and ln.endswith(" " + label)]
        if not back:
            continue
        ins = ins[:back[0] + 1]
        if any(ln.startswith("v_rsq_") for ln in ins) and not any(ln.startswith("v_cndmask") for ln in ins):
            count = lambda p: sum(ln.startswith(p) for ln in ins) / KU      # noqa: E731
            return {"instructions": len(ins) / KU, "v_pk_fma_f32": count("v_pk_fma_f32"),
                    "v_pk_mul_f32": count("v_pk_mul_f32"), "v_pk_add_f32": count("v_pk_add_f32"),
                    "packed": count("v_pk_"), "v_rsq_f32": count("v_rsq_f32"), "ds_read": count("ds_read"),
                    "v_mov_and_other_valu": sum(ln.startswith("v_") and not ln.startswith(("v_pk_", "v_rsq_"))
                                                for ln in ins) / KU}
    raise AssertionError("no un-masked loop found")


def _timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _median_ms(fn, reps, warmup=3):
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return float(np.median([_timed(fn, reps) for _ in range(5)]))


def _inputs(n, dtype):
    import numpy as np
    import torch
    from nbd.plummer import generate_plummer
    p, v, m = generate_plummer(n, seed=1)
    rng = np.random.default_rng(2)
    m = np.asarray(m) * rng.uniform(0.5, 1.5, n)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype, device=dev)      # noqa: E731
    return (t(np.asarray(p).reshape(n, 3)), t(np.asarray(v).reshape(n, 3)), t(m), t(rng.standard_normal((n, 3))),
            t(rng.standard_normal((n, 3))))


def times(n):
    import torch
    from nbd import direct
    eps2, g = 0.05 ** 2, 1.0
    reps = max(3, min(100, int(5e9 / n / n)))
    res = {"n": n, "reps": reps}
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        f64 = dtype == torch.float64
        pos, vel, mass, ca, cj = _inputs(n, dtype)
        alloc = direct.alloc_rows_f64 if f64 else direct.alloc_posm
        pack = direct.hermite_f64_pack if f64 else direct.hermite_pack
        rows, vrows, arows, jrows, spare = (alloc(n, pos.device) for _ in range(5))
        pack(pos, vel, mass, rows, vrows)
        pack(pos, ca, mass, spare, arows)
        pack(pos, cj, mass, spare, jrows)
        gp, gv, gm = torch.empty_like(pos), torch.empty_like(pos), torch.empty_like(mass)
        if f64:
            ws = direct.accel_jerk_vjp_f64_workspace(n, pos.device)
            ws_a = direct.accel_vjp_f64_workspace(n, pos.device)
            ws_h = direct.hermite_f64_workspace(n, pos.device)
            vjp = lambda a, b: direct.accel_jerk_vjp_f64(rows, vrows, a, b, n, eps2, g, gp, gv, gm, ws)      # noqa: E731
            avjp = lambda: direct.accel_vjp_f64(rows, arows, n, eps2, g, gp, gm, ws_a)                       # noqa: E731
            force = lambda: direct.accel_jerk_f64(rows, vrows, n, eps2, g, workspace=ws_h)                   # noqa: E731
        else:
            ws = direct.accel_jerk_vjp_workspace(n, pos.device)
            ws_a = direct.accel_vjp_workspace(n, pos.device)
            ws_h = direct.hermite_workspace(n, pos.device)
            acc, jerk = torch.empty_like(pos), torch.empty_like(pos)
            vjp = lambda a, b: direct.accel_jerk_vjp(rows, vrows, a, b, n, eps2, g, gp, gv, gm, ws)          # noqa: E731
            avjp = lambda: direct.accel_vjp(rows, arows, n, eps2, g, gp, gm, ws_a)                           # noqa: E731
            force = lambda: direct.accel_jerk(rows, vrows, n, eps2, g, acc, jerk, ws_h)                      # noqa: E731
        r = {"force_ms": _median_ms(force, reps), "accel_vjp_ms": _median_ms(avjp, reps),
             "both_ms": _median_ms(lambda: vjp(arows, jrows), reps),
             "beta_only_ms": _median_ms(lambda: vjp(None, jrows), reps),
             "alpha_only_ms": _median_ms(lambda: vjp(arows, None), reps)}
        for k in ("both", "beta_only", "alpha_only", "accel_vjp"):
            r[k + "_over_force"] = r[k + "_ms"] / r["force_ms"]
        res[tag] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_accel_jerk_vjp.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    asm = assembly()
    loop = unmasked_loop(asm)
    model = {"packed_ops_force": PACKED_FORCE, "packed_ops_accel_vjp": PACKED_VJP, "packed_ops_beta_walk": loop["packed"],
             "rsq": loop["v_rsq_f32"],
             "predicted_beta_only_over_force": (loop["packed"] + loop["v_rsq_f32"]) / (PACKED_FORCE + 2),
             "predicted_both_over_force": (loop["packed"] + PACKED_VJP + 2 * loop["v_rsq_f32"]) / (PACKED_FORCE + 2)}
    res = {"device": torch.cuda.get_device_name(0), "instruction_model": model, "unmasked_fp32_loop_per_source": loop,
           "times": [times(n) for n in SIZES], "resources": resources(asm)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
