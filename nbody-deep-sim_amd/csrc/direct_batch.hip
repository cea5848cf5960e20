// direct_batch.hip -- an ensemble of S independent systems ("scenes") advanced by one set of launches (gfx950).
//
// The scenes are stored back to back: bodies [off_s, off_s + n_s) of pos / vel / acc / mass belong to scene s, and
// the packed sources {x, y, z, m} of scene s sit at rows [poff_s, poff_s + pad64(n_s)) of one posm array (every scene
// padded to whole 64-body chunks with zero entries). Each body feels only the bodies of its own scene, with the
// scene's own G, softening^2 and dt. C-ABI: include/nbd.h (nbd_batch_*).
//
// Work list (built once on the host, nbd_batch_plan / nbd_batch_plan_fill, uploaded by the caller): one item per
// (scene, target group of 128, slab), a workgroup each. Item (s, g, k) runs the wave body of
// accel_kernel (accel_body of direct_kernels.h: two targets per lane, v_pk_fma_f32 + v_rsq_f32,
// LDS-DMA staged 64-body chunks, the same code the one-system kernel calls) on targets [128 g, 128 g + 128) of scene s against the chunks of ITS scene that
// wave k * 4 + w owns. The slab count of a scene is the single-system plan for its size (nbd_accel_plan(n, n)), so
// a scene's items, their split of the sources and the fixed-order slab sum depend on n_s alone: a scene's results
// are bit-identical whether it runs alone or with any companions, at any position of the batch. Items are
// dispatched largest first (the order of the work, never of any sum). No float atomics, no host syncs, no memset:
// every launch here can be captured into a graph.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_batch_plan.h"
#include "direct_kernels.h"

namespace {

// workspace: slabs (fp32) | energy partials (fp64, 8-byte aligned)
size_t ws_u_offset(const BatchTotals& t) { return ((size_t)t.ws_floats * 4 + 15) & ~(size_t)15; }
size_t ws_bytes_of(const BatchTotals& t) { return ws_u_offset(t) + (size_t)t.u_doubles * 8; }

// ---- segmented force: one workgroup per item; accel_kernel's body (accel_body, KU = 8, the scene's full view) on the
// item's scene, masked or not for the whole scene by an argument the compiler tests once per chunk. Unscaled
// sums into slab k of the scene: ws[ws_off + (k * n + i) * 3 + c]. softening^2 < kEps2Masked takes the index-masked
// path for the whole scene (fill_diagonal_, simulation.py:85: the i == j term and the padding are dropped by index,
// coincident bodies give NaN in that scene only). Otherwise r^2 >= softening^2 >= 1e-24 keeps s^3 finite, and a
// padding entry (m = 0) adds w d = 0 exactly, as in accel_kernel's general-mass path.
__global__ __launch_bounds__(64 * kWaves, 5) void batch_accel_kernel(const f4* __restrict__ posm,
                                                                     const int4* __restrict__ items,
                                                                     const SceneRec* __restrict__ scenes,
                                                                     const float* __restrict__ eps2_s,
                                                                     float* __restrict__ ws) {
  __shared__ f4 lds[kAccelLdsF4];
  const Item w = load_item(items, scenes);
  const f4* src = posm + w.poff;
  const float eps2 = eps2_s[w.s];
  const int t_base = w.grp * kTgtPerWG;
  accel_body<8, false>(src, full_view(w.n, w.n_chunks, w.slabs), eps2 < kEps2Masked, src, w.n, 0, t_base, w.slab, eps2,
                       1.0f, lds, ws + w.sc.ws_off + ((size_t)w.slab * w.n + t_base) * 3);
}

// ---- per packed row r: scene s = row_scene[r], body i = r - poff_s. Optional kick v += ck_s a, optional drift
// x += cd_s v, then posm[r] = {x, m} (zeros behind the scene's last body). mul and add round separately (the torch
// eager order of kick_drift_kernel): given the same accelerations the update is bit-exact with the one-system step.
__global__ __launch_bounds__(256) void batch_update_kernel(const int* __restrict__ row_scene,
                                                           const SceneRec* __restrict__ scenes, int n_rows,
                                                           float* __restrict__ pos, float* __restrict__ vel,
                                                           const float* __restrict__ acc, const float* __restrict__ mass,
                                                           const float* __restrict__ ck_s, const float* __restrict__ cd_s,
                                                           f4* __restrict__ posm) {
  PlanRow w;
  if (!load_row(row_scene, scenes, n_rows, w)) return;
  f4 pm = {0.f, 0.f, 0.f, 0.f};
  if (w.i() < w.sc.n) {
    const int b = w.sc.off + w.i();
    const float ck = acc ? ck_s[w.s] : 0.f, cd = cd_s ? cd_s[w.s] : 0.f;
    float x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      x[k] = pos[3 * b + k];
      if (vel) {
        float v = vel[3 * b + k];
        if (acc) { v = __fadd_rn(v, __fmul_rn(ck, acc[3 * b + k])); vel[3 * b + k] = v; }
        if (cd_s) { x[k] = __fadd_rn(x[k], __fmul_rn(cd, v)); pos[3 * b + k] = x[k]; }
      }
    }
    pm = f4{x[0], x[1], x[2], mass[b]};
  }
  posm[w.r] = pm;
}

// ---- fixed-order slab sum: acc = G_s * (slab_0 + slab_1 + ...) in slab order, optional fused kick v += ck_s acc.
// One thread per (packed row, component): coalesced over the scene's rows of each slab.
__global__ __launch_bounds__(256) void batch_finish_kernel(const int* __restrict__ row_scene,
                                                           const SceneRec* __restrict__ scenes, int n_rows,
                                                           const float* __restrict__ ws, const float* __restrict__ g_s,
                                                           float* __restrict__ acc, float* __restrict__ vel,
                                                           const float* __restrict__ ck_s) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 3 * n_rows) return;
  const int r = e / 3, comp = e - 3 * r;
  const PlanRow w = row_of(row_scene, scenes, r);
  if (w.i() >= w.sc.n) return;
  const float* p = ws + w.sc.ws_off + (size_t)w.i() * 3 + comp;
  const size_t stride = (size_t)w.sc.n * 3;
  float sum = p[0];
  for (int k = 1; k < w.sc.slabs; ++k) sum += p[k * stride];
  const float a = __fmul_rn(g_s[w.s], sum);
  const size_t o = (size_t)(w.sc.off + w.i()) * 3 + comp;
  acc[o] = a;
  if (vel) vel[o] = __fadd_rn(vel[o], __fmul_rn(ck_s[w.s], a));
}

// ---- segmented potential energy: one workgroup per item, energy_kernel's body (energy_body) on the item's scene (upper triangle,
// |r| + eps, fp32 lanes, fp64 across lanes); the item's partial goes to pu[u_off + g * slabs + k].
__global__ __launch_bounds__(64 * kWaves) void batch_energy_kernel(const f4* __restrict__ posm,
                                                                   const int4* __restrict__ items,
                                                                   const SceneRec* __restrict__ scenes,
                                                                   const float* __restrict__ soft_s,
                                                                   double* __restrict__ pu) {
  __shared__ f4 lds[kEnergyLdsF4];
  const Item w = load_item(items, scenes);
  const float soft = soft_s[w.s];
  energy_body(posm + w.poff, w.n, w.n_chunks, w.grp * kTgtPerWG, w.slab, w.slabs, soft, !(soft > 0.f), lds,
              pu + (size_t)w.sc.u_off + (size_t)w.grp * w.slabs + w.slab);
}

// one workgroup per scene: U_s = -G_s * (sum of its partials), K_s = sum 0.5 m v^2 (fp32 terms as kinetic_kernel,
// fp64 sums); thread-strided then a fixed shuffle / LDS tree. out_uk[2 s] = U_s, out_uk[2 s + 1] = K_s.
__global__ __launch_bounds__(256) void batch_energy_final_kernel(const SceneRec* __restrict__ scenes,
                                                                 const f4* __restrict__ posm,
                                                                 const float* __restrict__ vel,
                                                                 const double* __restrict__ pu,
                                                                 const float* __restrict__ g_s,
                                                                 double* __restrict__ out_uk) {
  __shared__ double ru[4], rk[4];
  const int s = blockIdx.x;
  const SceneRec sc = load_scene(scenes, s);
  double u = 0.0, k = 0.0;
  const int nu = sc.n > 0 ? sc.groups * sc.slabs : 0;
  for (int b = threadIdx.x; b < nu; b += 256) u += pu[(size_t)sc.u_off + b];
  for (int i = threadIdx.x; i < sc.n; i += 256) {
    const size_t b = (size_t)(sc.off + i) * 3;
    const float vx = vel[b], vy = vel[b + 1], vz = vel[b + 2];
    const float v2 = __fadd_rn(__fadd_rn(__fmul_rn(vx, vx), __fmul_rn(vy, vy)), __fmul_rn(vz, vz));
    k += (double)__fmul_rn(__fmul_rn(0.5f, posm[sc.poff + i].w), v2);       // 0.5 * m * |v|^2 (simulation.py:100)
  }
  for (int off = 32; off > 0; off >>= 1) { u += __shfl_down(u, off); k += __shfl_down(k, off); }
  if ((threadIdx.x & 63) == 0) { ru[threadIdx.x >> 6] = u; rk[threadIdx.x >> 6] = k; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double us = (ru[0] + ru[1]) + (ru[2] + ru[3]);
    out_uk[2 * s] = sc.n > 0 ? -(double)g_s[s] * us : 0.0;
    out_uk[2 * s + 1] = (rk[0] + rk[1]) + (rk[2] + rk[3]);
  }
}

int launch_update(const DevPlan& d, const BatchTotals& t, float* pos, float* vel, const float* acc, const float* mass,
                  const float* ck, const float* cd, float* posm, hipStream_t st) {
  batch_update_kernel<<<ceil_div(t.n_rows, 256), 256, 0, st>>>(d.row_scene, d.scenes, t.n_rows, pos, vel, acc, mass,
                                                               ck, cd, reinterpret_cast<f4*>(posm));
  return launch_status();
}

int launch_force(const DevPlan& d, const BatchTotals& t, const float* posm, const float* eps2, const float* g,
                 float* acc_out, float* vel, const float* ck, void* workspace, hipStream_t st) {
  float* ws = static_cast<float*>(workspace);
  batch_accel_kernel<<<t.n_items, 64 * kWaves, 0, st>>>(reinterpret_cast<const f4*>(posm), d.items, d.scenes, eps2, ws);
  int rc = launch_status();
  if (rc) return rc;
  batch_finish_kernel<<<ceil_div(3 * t.n_rows, 256), 256, 0, st>>>(d.row_scene, d.scenes, t.n_rows, ws, g, acc_out,
                                                                   vel, ck);
  return launch_status();
}

}  // namespace

extern "C" {

int nbd_batch_plan(const int* offsets, int n_scenes, int* n_items, int* posm_rows, size_t* plan_bytes,
                   size_t* workspace_bytes) {
  BatchTotals t;
  const int rc = batch_totals(offsets, n_scenes, &t);
  if (rc) return rc;
  if (n_items) *n_items = t.n_items;
  if (posm_rows) *posm_rows = t.n_rows;
  if (plan_bytes) *plan_bytes = plan_bytes_of(t);
  if (workspace_bytes) *workspace_bytes = ws_bytes_of(t);
  return 0;
}

int nbd_batch_plan_fill(const int* offsets, int n_scenes, void* plan, size_t plan_bytes) {
  BatchTotals t;
  const int rc = batch_totals(offsets, n_scenes, &t);
  if (rc) return rc;
  if (!plan || plan_bytes != plan_bytes_of(t)) return NBD_E_BADARG;
  batch_plan_fill(offsets, n_scenes, t, plan, scene_geom_f32);
  return 0;
}

int nbd_batch_pack_posm_f32(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const float* pos,
                            const float* mass, float* posm, nbd_stream_t stream) {
  BatchTotals t;
  int rc = batch_prologue(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc) return rc;
  if (t.n_total == 0) return 0;
  if (!pos || !mass || !posm || misaligned16(posm)) return NBD_E_BADARG;
  return launch_update(dev_plan(plan, t), t, const_cast<float*>(pos), nullptr, nullptr, mass, nullptr, nullptr, posm,
                       (hipStream_t)stream);
}

int nbd_batch_accel_f32(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const float* pos,
                        const float* mass, const float* softening_sq, const float* g_const, float* acc_out,
                        float* posm, void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  BatchTotals t;
  int rc = batch_prologue(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc) return rc;
  if (t.n_total == 0) return 0;
  if (!pos || !mass || !softening_sq || !g_const || !acc_out || !posm || misaligned16(posm)) return NBD_E_BADARG;
  if (!workspace || workspace_bytes < ws_bytes_of(t)) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const DevPlan d = dev_plan(plan, t);
  if ((rc = launch_update(d, t, const_cast<float*>(pos), nullptr, nullptr, mass, nullptr, nullptr, posm, st))) return rc;
  return launch_force(d, t, posm, softening_sq, g_const, acc_out, nullptr, nullptr, workspace, st);
}

int nbd_batch_leapfrog_step_f32(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, float* pos,
                                float* vel, const float* acc_in, float* acc_out, const float* mass, const float* dt_half,
                                const float* dt, const float* softening_sq, const float* g_const, float* posm,
                                void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  BatchTotals t;
  int rc = batch_prologue(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc) return rc;
  if (t.n_total == 0) return 0;
  if (!pos || !vel || !acc_in || !acc_out || !mass || !dt_half || !dt || !softening_sq || !g_const || !posm ||
      misaligned16(posm))
    return NBD_E_BADARG;
  if (!workspace || workspace_bytes < ws_bytes_of(t)) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const DevPlan d = dev_plan(plan, t);
  if ((rc = launch_update(d, t, pos, vel, acc_in, mass, dt_half, dt, posm, st))) return rc;
  return launch_force(d, t, posm, softening_sq, g_const, acc_out, vel, dt_half, workspace, st);
}

int nbd_batch_euler_step_f32(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, float* pos,
                             float* vel, float* acc_out, const float* mass, const float* dt, const float* softening_sq,
                             const float* g_const, float* posm, void* workspace, size_t workspace_bytes,
                             nbd_stream_t stream) {
  BatchTotals t;
  int rc = batch_prologue(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc) return rc;
  if (t.n_total == 0) return 0;
  if (!pos || !vel || !acc_out || !mass || !dt || !softening_sq || !g_const || !posm || misaligned16(posm))
    return NBD_E_BADARG;
  if (!workspace || workspace_bytes < ws_bytes_of(t)) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const DevPlan d = dev_plan(plan, t);
  if ((rc = launch_update(d, t, pos, nullptr, nullptr, mass, nullptr, nullptr, posm, st))) return rc;
  if ((rc = launch_force(d, t, posm, softening_sq, g_const, acc_out, vel, dt, workspace, st))) return rc;
  // drift x += dt v, and posm = the moved bodies (what the energies of the new state read)
  return launch_update(d, t, pos, vel, nullptr, mass, nullptr, dt, posm, st);
}

int nbd_batch_energies(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const float* posm,
                       const float* vel, const float* softening, const float* g_const, double* out_uk, void* workspace,
                       size_t workspace_bytes, nbd_stream_t stream) {
  BatchTotals t;
  int rc = batch_prologue(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc) return rc;
  if (!out_uk || !g_const || !softening) return NBD_E_BADARG;
  if (t.n_total > 0 && (!posm || !vel || misaligned16(posm))) return NBD_E_BADARG;
  if (!workspace || workspace_bytes < ws_bytes_of(t)) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const DevPlan d = dev_plan(plan, t);
  double* pu = reinterpret_cast<double*>(static_cast<char*>(workspace) + ws_u_offset(t));
  if (t.n_items > 0) {
    batch_energy_kernel<<<t.n_items, 64 * kWaves, 0, st>>>(reinterpret_cast<const f4*>(posm), d.items, d.scenes,
                                                          softening, pu);
    if ((rc = launch_status())) return rc;
  }
  batch_energy_final_kernel<<<n_scenes, 256, 0, st>>>(d.scenes, reinterpret_cast<const f4*>(posm), vel, pu, g_const,
                                                      out_uk);
  return launch_status();
}

}  // extern "C"
