// direct_batch_hermite.hip -- the shared-timestep 4th-order Hermite predictor-corrector of direct_hermite.hip, applied to
// every scene of an ensemble of independent systems by one set of launches (gfx950). C-ABI: the nbd_batch_hermite_* /
// nbd_batch_accel_jerk_f32 entries of include/nbd.h; Python: galaxify.simulation.BatchedSimulator(integrator="hermite").
//
// The scenes, the packed rows and the work list are those of direct_batch.hip (direct_batch_plan.h, unchanged): one item
// per (scene, target group of 128, slab), the slab count of a scene being the single-system plan for its size. One step
// is three launches for all scenes:
//   predict  : one thread per packed row: posm = {x_p, m}, velp = {v_p, 0} (zeros in each scene's padding):
//              hermite_predict_row (hermite_kernels.h) with the scene's own fp32 step constants
//   evaluate : one workgroup per item: accel_jerk_body (hermite_kernels.h, KU = 2) on the item's scene, masked or not per scene
//              from its softening^2; unscaled partial sums into float[slabs][6][n_s] at float 2 * ws_off of the slabs
//   correct  : one workgroup per 64 packed rows (never across scenes): hermite_slab_sum and hermite_correct_row with the
//              scene's G and constants; posm = {x1, m} for the energies after the step
// A scene's work, its split of the sources and its slab sum depend on n_s and its own parameters alone, and its arithmetic
// is the single-system kernels' own functions: its results are bit-identical to nbd_hermite_step_f32 on that scene alone.
// No atomics, no memsets, no host syncs: deterministic and capturable.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_batch_plan.h"
#include "direct_kernels.h"
#include "hermite_kernels.h"

namespace {

// rows of the per-scene step-constant table hdt[5][S], HermiteDt's fields in order (the caller forms each in double and
// rounds it once, as hermite_dt() does)
enum { kDt = 0, kDtHalf = 1, kDt2Half = 2, kDt3Sixth = 3, kDt2Twelfth = 4 };

// posm[r] = {x_p, m}, velp[r] = {v_p, 0} for every packed row r (zeros behind each scene's last body). acc == nullptr:
// a plain pack of (x, v).
__global__ __launch_bounds__(256) void batch_hermite_predict_kernel(const int* __restrict__ row_scene,
                                                                    const SceneRec* __restrict__ scenes, int n_rows,
                                                                    const float* __restrict__ pos,
                                                                    const float* __restrict__ vel,
                                                                    const float* __restrict__ acc,
                                                                    const float* __restrict__ jerk,
                                                                    const float* __restrict__ mass,
                                                                    const float* __restrict__ hdt, int n_scenes,
                                                                    f4* __restrict__ posm, f4* __restrict__ velp) {
  PlanRow w;
  if (!load_row(row_scene, scenes, n_rows, w)) return;
  f4 pm = HermiteFmt<float>::zero(), vp = HermiteFmt<float>::zero();
  if (w.i() < w.sc.n) {
    const int b = w.sc.off + w.i();
    const float dt = acc ? hdt[kDt * n_scenes + w.s] : 0.f;
    const float dt2_half = acc ? hdt[kDt2Half * n_scenes + w.s] : 0.f;
    const float dt3_sixth = acc ? hdt[kDt3Sixth * n_scenes + w.s] : 0.f;
    const PosVel3<float> p = hermite_predict_row(pos, vel, acc, jerk, (size_t)b, dt, dt2_half, dt3_sixth, acc != nullptr);
    pm = hermite_row(p.x, mass[b]);
    vp = hermite_row(p.v, 0.f);
  }
  posm[w.r] = pm;
  velp[w.r] = vp;
}

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

// One workgroup per 64 packed rows (a scene's rows are whole chunks of 64, so a block never spans two scenes): a1, j1 =
// hermite_slab_sum of the body's row in its scene's slabs, scaled by G_s. pos == nullptr: write a1, j1 only. Else
// hermite_correct_row: reads a0, j0 (acc_in / jerk_in may alias acc_out / jerk_out: each element is read before it is
// written, by the same thread), x, v; writes x1, v1, a1, j1 and posm = {x1, m}.
__global__ __launch_bounds__(256) void batch_hermite_correct_kernel(const int* __restrict__ row_scene,
                                                                    const SceneRec* __restrict__ scenes,
                                                                    const float* __restrict__ ws,
                                                                    const float* __restrict__ g_s,
                                                                    const float* __restrict__ hdt, int n_scenes,
                                                                    float* pos, float* vel, const float* acc_in,
                                                                    const float* jerk_in, float* acc_out,
                                                                    float* jerk_out, const float* __restrict__ mass,
                                                                    f4* __restrict__ posm) {
  const int lane = threadIdx.x & 63;
  const int r0 = blockIdx.x * 64;
  const int s = row_scene[r0];
  const SceneRec sc = load_scene(scenes, s);
  const int i = r0 - sc.poff + lane;
  float a1[3], j1[3];
  if (!hermite_slab_sum(ws + 2 * (size_t)sc.ws_off, sc.slabs, sc.n, (size_t)i, i < sc.n, g_s[s], a1, j1)) return;
  const size_t b = (size_t)sc.off + i;
  if (pos) {
    const Corrected<float> c = hermite_correct_row(pos, vel, acc_in, jerk_in, b, a1, j1, hdt[kDtHalf * n_scenes + s],
                                                   hdt[kDt2Twelfth * n_scenes + s]);
    posm[r0 + lane] = hermite_row(c.x1, mass[b]);
  }
  hermite_store_force(acc_out, jerk_out, b, a1, j1);
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
  batch_hermite_predict_kernel<<<ceil_div(t.n_rows, 256), 256, 0, st>>>(
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
  batch_hermite_correct_kernel<<<t.n_rows / kChunk, 256, 0, st>>>(d.row_scene, d.scenes, slabs, g, hdt, n_scenes,
                                                                   pos, vel, acc_in, jerk_in, acc_out, jerk_out, mass,
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
