// direct_hermite.hip -- shared-timestep 4th-order Hermite predictor-corrector (Makino & Aarseth 1992) for the direct
// force path on gfx950 (MI355X). An extension: the reference has Euler and kick-drift-kick leapfrog only. C-ABI: the
// nbd_hermite_* / nbd_accel_jerk_f32 entries of include/nbd.h; Python: galaxify.simulation.HermiteSimulator.
//
// One step is three launches (PEC form; a0, j0 carried from the previous step):
//   predict  : x_p = x + v dt + a0 dt^2/2 + j0 dt^3/6, v_p = v + a0 dt + j0 dt^2/2 -> posm = {x_p, m}, velp = {v_p, 0}
//              (64-source chunk layout, zero padding)
//   evaluate : accel_jerk_kernel -- a_i = G sum_j m_j r_ij s^3, j_i = G sum_j m_j (v_ij s^3 - 3 (r_ij.v_ij) s^5 r_ij)
//              into float[slabs][6][n] partial sums (unscaled)
//   correct  : fixed-order slab sum, a1 = G sum, j1 = G sum, then
//              v1 = v + (a0 + a1) dt/2 + (j0 - j1) dt^2/12,  x1 = x + (v + v1) dt/2 + (a0 - a1) dt^2/12,
//              posm = {x1, m} (energies after the step need no extra pack)
// The arithmetic of all three (hermite_predict_row, accel_jerk_body, hermite_slab_sum, hermite_correct_row), the step
// constants (hermite_dt) and the two O(N) kernels themselves (hermite_predict_kernel<T>, hermite_correct_kernel<T>, here
// at T = float) live in hermite_kernels.h, shared with the block-timestep, the batched, the sharded and the float64
// units.
// No atomics, no memsets, no host syncs: deterministic and capturable.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_kernels.h"
#include "hermite_kernels.h"

namespace {

// Acceleration + jerk of all n bodies under all n bodies: accel_jerk_body (hermite_kernels.h) with grid = (target groups
// of 128, slabs), the chunks spread over all slabs x 4 waves to within one. out: float[slab][6][n].
// KU = 2 (the default): 76 VGPRs, 6 waves per SIMD, and hipcc issues each pair of rsq's back to back with no s_nop in
// the loop; KU = 4: 88 VGPRs, 5 waves per SIMD, but hipcc interleaves the rsq's with their consumers and pads the
// transcendental hazards with s_nop (14-19 per 4 sources). 16 KiB of LDS per workgroup (the partials reuse each wave's
// own staging buffers), so LDS does not cap either below 10 workgroups per CU.
template <bool MASKED, int KU>
__global__ __launch_bounds__(64 * kWaves, KU == 2 ? 6 : 5) void accel_jerk_kernel(
    const f4* __restrict__ posm, const f4* __restrict__ velp, int n, int cpw_q, int cpw_r, float eps2,
    float* __restrict__ out) {
  __shared__ f4 lds[kWaves * 4 * kChunk];
  const Group128<unsigned> g(blockIdx.x, blockIdx.y, n);
  const ChunkRange c = wave_chunks(g.jw(), cpw_q, cpw_r);
  accel_jerk_body<MASKED, KU>(posm, velp, n, posm, velp, g.r0(), g.r1(), g.i0, g.i1, c.begin, c.end, eps2, lds,
                              g.dst(out), n, g.n_valid());
}

constexpr int kSumRows = HermiteFmt<float>::kSumRows;      // bodies per workgroup of the corrector launch

size_t velp_bytes(int n) { return (size_t)ceil_div(n, kChunk) * kChunk * sizeof(f4); }

// the unscaled partial sums of every body into float[slabs][6][n]
int launch_jerk(const float* posm, const float* velp, int n, float eps2, float* slabs, const JerkPlan& p, int variant,
                hipStream_t st) {
  dim3 grid(p.groups, p.slabs), block(64 * kWaves);
  const ChunkSplit c = chunk_split(p.n_chunks, p.slabs);
  const f4* pm = reinterpret_cast<const f4*>(posm);
  const f4* vp = reinterpret_cast<const f4*>(velp);
  const bool masked = eps2 < kEps2Masked;
#define NBD_LAUNCH(M, K) accel_jerk_kernel<M, K><<<grid, block, 0, st>>>(pm, vp, n, c.q, c.r, eps2, slabs)
  if (variant == 1) { if (masked) NBD_LAUNCH(true, 4); else NBD_LAUNCH(false, 4); }
  else              { if (masked) NBD_LAUNCH(true, 2); else NBD_LAUNCH(false, 2); }
#undef NBD_LAUNCH
  return launch_status();
}

}  // namespace

extern "C" {

size_t nbd_hermite_workspace_bytes(int n) {
  if (n <= 0) return 0;
  return velp_bytes(n) + (size_t)plan_jerk(n, n).slabs * 6 * n * sizeof(float);
}

int nbd_hermite_pack_f32(const float* pos, const float* vel, const float* acc, const float* jerk, const float* mass,
                         int n, double dt, float* posm, float* velp, nbd_stream_t stream) {
  if (n < 0 || (n > 0 && (!pos || !vel || !mass || !posm || !velp)) || (!acc != !jerk)) return NBD_E_BADARG;
  if (misaligned16(posm) || misaligned16(velp)) return NBD_E_BADARG;
  if (n == 0) return 0;
  const int n_pad = nbd_posm_padded_len(n);
  hermite_predict_kernel<float><<<ceil_div(n_pad, 256), 256, 0, (hipStream_t)stream>>>(
      pos, vel, acc, jerk, mass, n, n_pad, hermite_dt(dt), reinterpret_cast<f4*>(posm), reinterpret_cast<f4*>(velp));
  return launch_status();
}

int nbd_accel_jerk_f32(const float* posm, const float* velp, int n, float softening_sq, float g_const, float* acc_out,
                       float* jerk_out, void* workspace, size_t workspace_bytes, int variant, nbd_stream_t stream) {
  if (n < 0 || variant < 0 || variant > 1) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (!posm || !velp || !acc_out || !jerk_out || misaligned16(posm) || misaligned16(velp)) return NBD_E_BADARG;
  if (!workspace || workspace_bytes < nbd_hermite_workspace_bytes(n)) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const JerkPlan p = plan_jerk(n, n);
  float* slabs = static_cast<float*>(workspace);
  int rc = launch_jerk(posm, velp, n, softening_sq, slabs, p, variant, st);
  if (rc) return rc;
  hermite_correct_kernel<float><<<ceil_div(n, kSumRows), 256, 0, st>>>(slabs, p.slabs, n, g_const, hermite_dt(0.0),
                                                                       nullptr, nullptr, nullptr, nullptr, acc_out,
                                                                       jerk_out, nullptr, nullptr);
  return launch_status();
}

int nbd_hermite_step_f32(float* pos, float* vel, const float* acc_in, const float* jerk_in, float* acc_out,
                         float* jerk_out, const float* mass, int n, double dt, float softening_sq, float g_const,
                         float* posm, void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  if (n < 0) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (!pos || !vel || !acc_in || !jerk_in || !acc_out || !jerk_out || !mass || !posm || misaligned16(posm))
    return NBD_E_BADARG;
  if (!workspace || misaligned16(workspace) || workspace_bytes < nbd_hermite_workspace_bytes(n)) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const HermiteDt h = hermite_dt(dt);
  const JerkPlan p = plan_jerk(n, n);
  float* velp = static_cast<float*>(workspace);
  float* slabs = reinterpret_cast<float*>(static_cast<char*>(workspace) + velp_bytes(n));
  const int n_pad = nbd_posm_padded_len(n);
  hermite_predict_kernel<float><<<ceil_div(n_pad, 256), 256, 0, st>>>(
      pos, vel, acc_in, jerk_in, mass, n, n_pad, h, reinterpret_cast<f4*>(posm), reinterpret_cast<f4*>(velp));
  int rc = launch_status();
  if (rc) return rc;
  if ((rc = launch_jerk(posm, velp, n, softening_sq, slabs, p, 0, st))) return rc;
  hermite_correct_kernel<float><<<ceil_div(n, kSumRows), 256, 0, st>>>(
      slabs, p.slabs, n, g_const, h, pos, vel, acc_in, jerk_in, acc_out, jerk_out, mass, reinterpret_cast<f4*>(posm));
  return launch_status();
}

}  // extern "C"
