"""The backward of the all-pairs acceleration (csrc/direct_grad.hip) next to its forward and to K-H's force on the
MI355X, in one process.

  python tools/bench_accel_vjp.py [--out FILE]            (default: profiles/r14_accel_vjp.json)
  python tools/bench_accel_vjp.py --build-variant         (no GPU: builds the measurement variant beside the library)

1. HIP-event times (median of 5 batches) at N = 4 096, 16 384, 65 536, float32 and float64: the forward of
   nbd.autograd.direct_accel (nbd_accel_f32, resp. nbd_accel_jerk_f64), the backward launch pair (nbd_accel_vjp_*), and
   K-H's force of that dtype (nbd_accel_jerk_f32 / _f64), with backward / K-H next to the instruction model's ratio
   (29 packed ops + 2 v_rsq_f32 against 26 + 2 per source and pair of targets in fp32; the issue's model, 30-32 + 2,
   predicts 1.15-1.2).
2. VGPRs, waves per SIMD and scratch of the new kernels, read from the gfx950 assembly (hipcc -S).
3. If tools/_trace/libnbd_hip_vjp_two_products.so exists (--build-variant made it: csrc/direct_grad.hip with
   -DNBD_VJP_OWN_MASKED=0, i.e. h by two separately rounded products and a subtraction and no chunk index-masked for the
   workgroup's own indices), the fp32 backward of that build, timed by a fresh child process with NBD_LIB_OVERRIDE, and
   its resources.
"""
import argparse
import glob
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
VARIANT_LIB = os.path.join(ROOT, "tools", "_trace", "libnbd_hip_vjp_two_products.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off"]
SIZES = (4096, 16384, 65536)
MODEL = {"packed_ops_vjp": 29, "packed_ops_vjp_two_products_variant": 32, "packed_ops_kh": 26, "rsq": 2,
         "predicted_ratio": [1.15, 1.2]}


def build_variant():
    """direct_grad.hip with h from two products, linked with the library's other objects (make them first)."""
    objs = [o for o in glob.glob(os.path.join(CSRC, "*.o")) if os.path.basename(o) != "direct_grad.o"]
    assert objs, "build the library first (make -C nbody-deep-sim_amd/csrc)"
    os.makedirs(os.path.dirname(VARIANT_LIB), exist_ok=True)
    obj = os.path.join(os.path.dirname(VARIANT_LIB), "direct_grad_two_products.o")
    subprocess.run([HIPCC, *FLAGS, "-fPIC", "-DNBD_VJP_OWN_MASKED=0", "-c", os.path.join(CSRC, "direct_grad.hip"), "-o", obj],
                   check=True)
    subprocess.run([HIPCC, "-shared", "-fPIC", "--offload-arch=gfx950", *objs, obj, "-o", VARIANT_LIB], check=True)
    print(VARIANT_LIB)


def resources(defines=()):
    """{kernel: {vgprs, waves_per_simd, scratch_bytes, lds_bytes}} of csrc/direct_grad.hip from its assembly."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "direct_grad.s")
        subprocess.run([HIPCC, *FLAGS, *defines, "--cuda-device-only", "-S", "-o", out,
                        os.path.join(CSRC, "direct_grad.hip")], check=True, capture_output=True)
        asm = open(out).read()
    res = {}
    for blk in asm[asm.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
        short = re.search(r"(accel_vjp\w*?kernel)(ILb([01])E)?", name)
        key = short.group(1) + ({"0": "<unmasked>", "1": "<masked>"}.get(short.group(3), ""))
        res[key] = {"vgprs": vgpr, "waves_per_simd": min(8, 512 // (-(-vgpr // 8) * 8)),
                    "scratch_bytes": int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)),
                    "lds_bytes": int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))}
    return res


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
    p, _, m = generate_plummer(n, seed=1)
    rng = np.random.default_rng(2)
    m = np.asarray(m) * rng.uniform(0.5, 1.5, n)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype, device=dev)      # noqa: E731
    return t(p), t(m), t(rng.standard_normal((n, 3)))


def times(n, only_f32_backward=False):
    import torch
    from nbd import direct
    eps2, g = 0.05 ** 2, 1.0
    reps = max(3, min(100, int(1e10 / n / n)))
    res = {"n": n, "reps": reps}
    # float32
    pos, mass, cot = _inputs(n, torch.float32)
    posm, cotm = direct.alloc_posm(n, pos.device), direct.alloc_posm(n, pos.device)
    direct.hermite_pack(pos, cot, mass, posm, cotm)
    gp, gm = torch.empty_like(pos), torch.empty_like(mass)
    ws = direct.accel_vjp_workspace(n, pos.device)
    res["f32_backward_ms"] = _median_ms(lambda: direct.accel_vjp(posm, cotm, n, eps2, g, gp, gm, ws), reps)
    if only_f32_backward:
        return res
    acc, jerk = torch.empty_like(pos), torch.empty_like(pos)
    ws_a, ws_h = direct.accel_workspace(n, n, pos.device), direct.hermite_workspace(n, pos.device)
    res["f32_forward_ms"] = _median_ms(lambda: direct.accel(posm, n, posm, n, 0, eps2, g, out=acc, workspace=ws_a), reps)
    res["f32_kh_force_ms"] = _median_ms(lambda: direct.accel_jerk(posm, cotm, n, eps2, g, acc, jerk, ws_h), reps)
    res["f32_backward_over_kh"] = res["f32_backward_ms"] / res["f32_kh_force_ms"]
    res["f32_backward_over_forward"] = res["f32_backward_ms"] / res["f32_forward_ms"]
    # float64: the forward of direct_accel IS K-H64's force (acceleration + jerk, the jerk dropped)
    pos, mass, cot = _inputs(n, torch.float64)
    posd, cotd = direct.alloc_rows_f64(n, pos.device), direct.alloc_rows_f64(n, pos.device)
    direct.hermite_f64_pack(pos, cot, mass, posd, cotd)
    gp, gm = torch.empty_like(pos), torch.empty_like(mass)
    ws = direct.accel_vjp_f64_workspace(n, pos.device)
    ws_h = direct.hermite_f64_workspace(n, pos.device)
    res["f64_backward_ms"] = _median_ms(lambda: direct.accel_vjp_f64(posd, cotd, n, eps2, g, gp, gm, ws), reps)
    res["f64_forward_ms"] = res["f64_kh_force_ms"] = _median_ms(
        lambda: direct.accel_jerk_f64(posd, cotd, n, eps2, g, workspace=ws_h), reps)
    res["f64_backward_over_kh"] = res["f64_backward_ms"] / res["f64_kh_force_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_accel_vjp.json"))
    ap.add_argument("--build-variant", action="store_true")
    ap.add_argument("--child-f32-backward", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.build_variant:
        return build_variant()
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    if args.child_f32_backward:
        print("CHILD " + json.dumps([times(n, only_f32_backward=True) for n in SIZES]))
        return
    res = {"device": torch.cuda.get_device_name(0), "instruction_model": MODEL,
           "times": [times(n) for n in SIZES], "resources": resources()}
    if os.path.exists(VARIANT_LIB):
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-f32-backward"], check=True,
                               capture_output=True, text=True, timeout=300, env=dict(os.environ, NBD_LIB_OVERRIDE=VARIANT_LIB))
        rows = json.loads(next(ln for ln in child.stdout.splitlines() if ln.startswith("CHILD "))[6:])
        res["two_products_variant"] = {"f32_backward_ms": {str(r["n"]): r["f32_backward_ms"] for r in rows},
                                            "resources": resources(["-DNBD_VJP_OWN_MASKED=0"])}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
