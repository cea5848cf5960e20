// direct_batch_hermite.hip -- the shared-timestep 4th-order Hermite predictor-corrector of direct_hermite.hip, applied to
// every scene of an ensemble of independent systems by one set of launches (gfx950). C-ABI: the nbd_batch_hermite_* /
// nbd_batch_accel_jerk_f32 entries of include/nbd.h; Python: galaxify.simulation.BatchedSimulator(integrator="hermite").
//
// The scenes, the packed rows and the work list are those of direct_batch.hip (direct_batch_plan.h, unchanged): one item
// per (scene, target group of 128, slab), the slab count of a scene being the single-system plan for its size. One step
// is three launches for all scenes:
//   predict  : batch_hermite_predict_kernel<float> (hermite_batch_kernels.h, shared with the float64 unit): one thread
//              per packed row: posm = {x_p, m}, velp = {v_p, 0} (zeros in each scene's padding), the row predictor of
//              hermite_kernels.h with the scene's own fp32 step constants (hdt[5][S], HermiteStepRow's rows; the caller
//              forms each in double and rounds it once, as hermite_dt() does)
//   evaluate : one workgroup per item: accel_jerk_body (hermite_kernels.h, KU = 2) on the item's scene, masked or not per scene
//              from its softening^2; unscaled partial sums into float[slabs][6][n_s] at float 2 * ws_off of the slabs
//   correct  : batch_hermite_correct_kernel<float> (the same header): one workgroup per 64 packed rows (never across
//              scenes): hermite_slab_sum and hermite_correct_row with the scene's G and constants; posm = {x1, m} for the
//              energies after the step
// A scene's work, its split of the sources and its slab sum depend on n_s and its own parameters alone, and its arithmetic
// is the single-system kernels' own functions: its results are bit-identical to nbd_hermite_step_f32 on that scene alone.
// No atomics, no memsets, no host syncs: deterministic and capturable.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_batch_plan.h"
#include "direct_kernels.h"
#include "hermite_batch_kernels.h"
#include "hermite_kernels.h"

namespace {

// One workgroup per item (s, g, k): targets [128 g, 128 g + 128) of scene s (its packed rows of posm / velp) against the
// chunks that wave 4 k + w owns in the scene's own plan: accel_jerk_kernel<MASKED, 2>'s geometry read from the scene
// record, then the same accel_jerk_body. softening^2 < kEps2Masked takes the index-masked loop for the whole scene; the
// branch is taken once, at the top, so that each path keeps its own registers. out: the scene's float[slabs][6][n] at
// ws + 2 * ws_off (the leapfrog plan's float[slabs][n][3] offsets, doubled).
__global__ __launch_bounds__(64 * kWaves, 5) void batch_accel_jerk_kernel(const f4* __restrict__ posm,
                                                                          const f4* __restrict__ velp,
                                                                          const int4* __restrict__ items,
                                                                          const SceneRec* __restrict__ scenes,
                                                                          const float* __restrict__ eps2_s,
                                                                          float* __restrict__ ws) {
  __shared__ f4 lds[kWaves * 4 * kChunk];
  const Item w = load_item(items, scenes);
  const float eps2 = eps2_s[w.s];
  const Group128<int> g(w.grp, w.slab, w.n);
  const ChunkSplit sp = chunk_split(w.n_chunks, w.slabs);
  const ChunkRange c = wave_chunks(g.jw(), sp.q, sp.r);
  float* dst = g.dst(ws + 2 * (size_t)w.sc.ws_off);
  const int n_valid = g.n_valid();
  if (eps2 < kEps2Masked)
    accel_jerk_body<true, 2>(posm + w.poff, velp + w.poff, w.n, posm + w.poff, velp + w.poff, g.r0(), g.r1(), g.i0, g.i1,
                             c.begin, c.end, eps2, lds, dst, w.n, n_valid);
  else
    accel_jerk_body<false, 2>(posm + w.poff, velp + w.poff, w.n, posm + w.poff, velp + w.poff, g.r0(), g.r1(), g.i0, g.i1,
                              c.begin, c.end, eps2, lds, dst, w.n, n_valid);
}

// workspace: velp float4[posm_rows] | slabs fp32[2 * ws_floats] (16-byte aligned: posm_rows * 16 bytes come first)
size_t hws_slab_offset(const BatchTotals& t) { return (size_t)t.n_rows * sizeof(f4); }
size_t hws_bytes_of(const BatchTotals& t) { return hws_slab_offset(t) + (size_t)(2 * t.ws_floats) * sizeof(float); }
// The slabs of a scene start at float 2 * ws_off; the whole slab area must stay within the int range the plan's own
// offsets live in.
bool hws_fits(const BatchTotals& t) { return 2 * t.ws_floats <= (int64_t)INT_MAX; }

int launch_predict(const DevPlan& d, const BatchTotals& t, const float* pos, const float* vel, const float* acc,
                   const float* jerk, const float* mass, const float* hdt, int n_scenes, float* posm, void* workspace,
                   hipStream_t st) {
  batch_hermite_predict_kernel<float><<<ceil_div(t.n_rows, 256), 256, 0, st>>>(
      d.row_scene, d.scenes, t.n_rows, pos, vel, acc, jerk, mass, hdt, n_scenes, reinterpret_cast<f4*>(posm),
      static_cast<f4*>(workspace));
  return launch_status();
}

// the force of every scene at posm / velp, then the slab sum (+ the corrector when pos is given)
int launch_force_correct(const DevPlan& d, const BatchTotals& t, float* posm, const float* eps2, const float* g,
                         const float* hdt, int n_scenes, float* pos, float* vel, const float* acc_in,
                         const float* jerk_in, float* acc_out, float* jerk_out, const float* mass, void* workspace,
                         hipStream_t st) {
  const f4* velp = static_cast<const f4*>(workspace);
  float* slabs = reinterpret_cast<float*>(static_cast<char*>(workspace) + hws_slab_offset(t));
  batch_accel_jerk_kernel<<<t.n_items, 64 * kWaves, 0, st>>>(reinterpret_cast<const f4*>(posm), velp, d.items,
                                                             d.scenes, eps2, slabs);
  int rc = launch_status();
  if (rc) return rc;
  batch_hermite_correct_kernel<float><<<ceil_div(t.n_rows, HermiteFmt<float>::kSumRows), 256, 0, st>>>(
      d.row_scene, d.scenes, t.n_rows, slabs, g, hdt, n_scenes, pos, vel, acc_in, jerk_in, acc_out, jerk_out, mass,
      reinterpret_cast<f4*>(posm));
  return launch_status();
}

}  // namespace

extern "C" {

int nbd_batch_hermite_workspace_bytes(const int* offsets, int n_scenes, size_t* bytes) {
  BatchTotals t;
  const int rc = batch_totals(offsets, n_scenes, &t);
  if (rc) return rc;
  if (!bytes) return NBD_E_BADARG;
  if (!hws_fits(t)) return NBD_E_UNSUPPORTED;
  *bytes = hws_bytes_of(t);
  return 0;
}

int nbd_batch_accel_jerk_f32(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const float* pos,
                             const float* vel, const float* mass, const float* softening_sq, const float* g_const,
                             float* acc_out, float* jerk_out, float* posm, void* workspace, size_t workspace_bytes,
                             nbd_stream_t stream) {
  BatchTotals t;
  int rc = batch_prologue(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc) return rc;
  if (!hws_fits(t)) return NBD_E_UNSUPPORTED;
  if (t.n_total == 0) return 0;
  if (!pos || !vel || !mass || !softening_sq || !g_const || !acc_out || !jerk_out || !posm || misaligned16(posm))
    return NBD_E_BADARG;
  if (!workspace || misaligned16(workspace) || workspace_bytes < hws_bytes_of(t)) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const DevPlan d = dev_plan(plan, t);
  if ((rc = launch_predict(d, t, pos, vel, nullptr, nullptr, mass, nullptr, n_scenes, posm, workspace, st))) return rc;
  return launch_force_correct(d, t, posm, softening_sq, g_const, nullptr, n_scenes, nullptr, nullptr, nullptr, nullptr,
                              acc_out, jerk_out, nullptr, workspace, st);
}

int nbd_batch_hermite_step_f32(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, float* pos,
                               float* vel, const float* acc_in, const float* jerk_in, float* acc_out, float* jerk_out,
                               const float* mass, const float* hdt, const float* softening_sq, const float* g_const,
                               float* posm, void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  BatchTotals t;
  int rc = batch_prologue(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc) return rc;
  if (!hws_fits(t)) return NBD_E_UNSUPPORTED;
  if (t.n_total == 0) return 0;
  if (!pos || !vel || !acc_in || !jerk_in || !acc_out || !jerk_out || !mass || !hdt || !softening_sq || !g_const ||
      !posm || misaligned16(posm))
    return NBD_E_BADARG;
  if (!workspace || misaligned16(workspace) || workspace_bytes < hws_bytes_of(t)) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const DevPlan d = dev_plan(plan, t);
  if ((rc = launch_predict(d, t, pos, vel, acc_in, jerk_in, mass, hdt, n_scenes, posm, workspace, st))) return rc;
  return launch_force_correct(d, t, posm, softening_sq, g_const, hdt, n_scenes, pos, vel, acc_in, jerk_in, acc_out,
                              jerk_out, mass, workspace, st);
}

}  // extern "C"
