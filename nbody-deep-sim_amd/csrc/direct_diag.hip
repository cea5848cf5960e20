// direct_diag.hip -- diagnostics of the direct integrators on the device (gfx950): the per-body potential of the softening
// the FORCE uses, and the conserved quantities of a system formed from it.
//
// The force is Plummer-softened, a_i = G sum_j m_j r_ij (r^2 + eps^2)^(-3/2); it is the gradient of
//     phi_i = -G sum_{j != i} m_j (r_ij^2 + eps^2)^(-1/2),
// not of the reference's energy convention -G m_i m_j / (|r| + eps) that nbd_energy_f32 reproduces. Only
// E = K + 1/2 sum m_i phi_i is conserved by the equations of motion the integrators solve, so only its drift measures an
// integrator. Both exist: nbd_energy_f32 stays the drop-in for compute_energies(), this file is the figure of merit.
//
// potential_kernel: potential_body of direct_kernels.h (accel_body's geometry and LDS-DMA chunk walk; per pair 5 packed
// fp32 ops + 2 v_rsq_f32; fp32 sums of at most one 64-source chunk, everything above that in fp64) into one fp64 slab per
// source split; potential_finish_kernel adds the slabs in slab order and applies -G in fp64. invariants_kernel: one
// workgroup per system (invariants_body of direct_kernels.h), every product formed in fp64 from the fp32 state,
// thread-strided sums and a fixed shuffle / LDS tree. The batched kernels are a prologue that reads the scene record (direct_batch_plan.h) and the same bodies: a scene
// of a batch is bit-identical to the same system alone. No atomics, no memsets, no host syncs: deterministic, capturable.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_batch_plan.h"
#include "direct_kernels.h"

namespace {

__global__ __launch_bounds__(64 * kWaves) void potential_kernel(const f4* __restrict__ src, int n_src, int n_chunks,
                                                                int all_masked, const f4* __restrict__ tgt, int n_tgt,
                                                                int tgt_off, float eps2, double* __restrict__ slabs) {
  __shared__ f4 lds[kPotLdsF4];
  const int t_base = blockIdx.x * kTgtPerWG;
  potential_body(src, n_src, n_chunks, gridDim.y, all_masked != 0, tgt, n_tgt, tgt_off, t_base, blockIdx.y, eps2, lds,
                 slabs + (size_t)blockIdx.y * n_tgt + t_base);
}

// phi[i] = -G (slab_0[i] + slab_1[i] + ...) in slab order, all in fp64 (0 - G sum: a body without partners gets +0).
__device__ __forceinline__ double finish_phi(const double* __restrict__ p, int n_slabs, size_t stride, float g) {
  double sum = 0.0;
  for (int k = 0; k < n_slabs; ++k) sum += p[k * stride];
  return 0.0 - (double)g * sum;
}

__global__ __launch_bounds__(256) void potential_finish_kernel(const double* __restrict__ slabs, int n_slabs, int n_tgt,
                                                               float g, double* __restrict__ phi) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_tgt) phi[i] = finish_phi(slabs + i, n_slabs, (size_t)n_tgt, g);
}

// A body of the fp32 state for invariants_body (direct_kernels.h): posm rows and vel (n,3), promoted to fp64.
struct PackedF32State {
  const f4* __restrict__ posm;
  const float* __restrict__ vel;
  __device__ __forceinline__ void operator()(int i, double& m, double* x, double* v) const {
    const f4 p = posm[i];
    m = p.w; x[0] = p.x; x[1] = p.y; x[2] = p.z;
    v[0] = vel[3 * (size_t)i]; v[1] = vel[3 * (size_t)i + 1]; v[2] = vel[3 * (size_t)i + 2];
  }
};

__global__ __launch_bounds__(kInvThreads) void invariants_kernel(const f4* __restrict__ posm,
                                                                 const float* __restrict__ vel,
                                                                 const double* __restrict__ phi, int n,
                                                                 double* __restrict__ row) {
  __shared__ double red[kInvSums][kInvWaves];
  invariants_body(PackedF32State{posm, vel}, phi, n, row, red);
}

// ---- the batched forms: the scene's geometry from its record, then the same bodies
// potential partials of scene s: double[slabs][n] from double index ws_off / 3 of the workspace (ws_off counts the fp32
// force slabs float[slabs][n][3] of the scenes in front: 12 bytes per entry there, 8 here)
__global__ __launch_bounds__(64 * kWaves) void batch_potential_kernel(const f4* __restrict__ posm,
                                                                      const int4* __restrict__ items,
                                                                      const SceneRec* __restrict__ scenes,
                                                                      const float* __restrict__ eps2_s,
                                                                      double* __restrict__ ws) {
  __shared__ f4 lds[kPotLdsF4];
  const Item w = load_item(items, scenes);
  const f4* src = posm + w.poff;
  const float eps2 = eps2_s[w.s];
  const int t_base = w.grp * kTgtPerWG;
  potential_body(src, w.n, w.n_chunks, w.slabs, eps2 < kEps2Masked, src, w.n, 0, t_base, w.slab, eps2, lds,
                 ws + w.sc.ws_off / 3 + (size_t)w.slab * w.n + t_base);
}

__global__ __launch_bounds__(256) void batch_potential_finish_kernel(const int* __restrict__ row_scene,
                                                                     const SceneRec* __restrict__ scenes, int n_rows,
                                                                     const double* __restrict__ ws,
                                                                     const float* __restrict__ g_s,
                                                                     double* __restrict__ phi) {
  PlanRow w;
  if (!load_row(row_scene, scenes, n_rows, w) || w.i() >= w.sc.n) return;
  phi[w.sc.off + w.i()] = finish_phi(ws + w.sc.ws_off / 3 + w.i(), w.sc.slabs, (size_t)w.sc.n, g_s[w.s]);
}

__global__ __launch_bounds__(kInvThreads) void batch_invariants_kernel(const SceneRec* __restrict__ scenes,
                                                                       const f4* __restrict__ posm,
                                                                       const float* __restrict__ vel,
                                                                       const double* __restrict__ phi,
                                                                       double* __restrict__ rows) {
  __shared__ double red[kInvSums][kInvWaves];
  const SceneRec sc = load_scene(scenes, blockIdx.x);
  invariants_body(PackedF32State{posm + sc.poff, vel + (size_t)sc.off * 3}, phi + sc.off, sc.n,
                  rows + (size_t)blockIdx.x * 16, red);
}

inline int potential_slabs(int n_src, int n_tgt) {
  int s = 1;
  if (nbd_accel_plan(n_src, n_tgt, nullptr, &s, nullptr) != 0 || s < 1) s = 1;
  return s;
}

}  // namespace

extern "C" {

size_t nbd_potential_workspace_bytes(int n_src, int n_tgt) {
  if (n_src <= 0 || n_tgt <= 0) return 0;
  return (size_t)potential_slabs(n_src, n_tgt) * n_tgt * sizeof(double);
}

int nbd_potential_f32(const float* posm_src, int n_src, const float* posm_tgt, int n_tgt, int tgt_global_offset,
                      float softening_sq, float g_const, double* phi_out, void* workspace, size_t workspace_bytes,
                      nbd_stream_t stream) {
  if (n_src < 0 || n_tgt < 0 || tgt_global_offset < 0) return NBD_E_BADARG;
  if (n_tgt == 0) return 0;
  if (!phi_out || misaligned8(phi_out) || !posm_tgt || misaligned16(posm_tgt)) return NBD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (n_src == 0) {                            // no partners: zero slabs summed
    potential_finish_kernel<<<ceil_div(n_tgt, 256), 256, 0, st>>>(nullptr, 0, n_tgt, g_const, phi_out);
    return launch_status();
  }
  if (!posm_src || misaligned16(posm_src)) return NBD_E_BADARG;
  if (!workspace || misaligned8(workspace) || workspace_bytes < nbd_potential_workspace_bytes(n_src, n_tgt))
    return NBD_E_WORKSPACE;
  const int slabs = potential_slabs(n_src, n_tgt);
  double* ws = static_cast<double*>(workspace);
  potential_kernel<<<dim3(ceil_div(n_tgt, kTgtPerWG), slabs), 64 * kWaves, 0, st>>>(
      reinterpret_cast<const f4*>(posm_src), n_src, ceil_div(n_src, kChunk), softening_sq < kEps2Masked ? 1 : 0,
      reinterpret_cast<const f4*>(posm_tgt), n_tgt, tgt_global_offset, softening_sq, ws);
  const int rc = launch_status();
  if (rc) return rc;
  potential_finish_kernel<<<ceil_div(n_tgt, 256), 256, 0, st>>>(ws, slabs, n_tgt, g_const, phi_out);
  return launch_status();
}

int nbd_invariants_f64(const float* posm, const float* vel, const double* phi, int n, double* out_row,
                       nbd_stream_t stream) {
  if (n < 0 || !out_row || misaligned8(out_row)) return NBD_E_BADARG;
  if (n > 0 && (!posm || !vel || !phi || misaligned16(posm) || misaligned8(phi))) return NBD_E_BADARG;
  invariants_kernel<<<1, kInvThreads, 0, (hipStream_t)stream>>>(reinterpret_cast<const f4*>(posm), vel, phi, n, out_row);
  return launch_status();
}

int nbd_batch_potential_f32(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const float* posm,
                            const float* softening_sq, const float* g_const, double* phi_out, void* workspace,
                            size_t workspace_bytes, nbd_stream_t stream) {
  BatchTotals t;
  int rc = batch_prologue(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc) return rc;
  if (t.n_total == 0) return 0;
  if (!posm || misaligned16(posm) || !softening_sq || !g_const || !phi_out || misaligned8(phi_out)) return NBD_E_BADARG;
  if (!workspace || misaligned8(workspace) || workspace_bytes < (size_t)(t.ws_floats / 3) * sizeof(double))
    return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const DevPlan d = dev_plan(plan, t);
  double* ws = static_cast<double*>(workspace);
  batch_potential_kernel<<<t.n_items, 64 * kWaves, 0, st>>>(reinterpret_cast<const f4*>(posm), d.items, d.scenes,
                                                           softening_sq, ws);
  if ((rc = launch_status())) return rc;
  batch_potential_finish_kernel<<<ceil_div(t.n_rows, 256), 256, 0, st>>>(d.row_scene, d.scenes, t.n_rows, ws, g_const,
                                                                        phi_out);
  return launch_status();
}

int nbd_batch_invariants_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const float* posm,
                             const float* vel, const double* phi, double* out_rows, nbd_stream_t stream) {
  BatchTotals t;
  const int rc = batch_prologue(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc) return rc;
  if (!out_rows || misaligned8(out_rows)) return NBD_E_BADARG;
  if (t.n_total > 0 && (!posm || !vel || !phi || misaligned16(posm) || misaligned8(phi))) return NBD_E_BADARG;
  batch_invariants_kernel<<<n_scenes, kInvThreads, 0, (hipStream_t)stream>>>(
      dev_plan(plan, t).scenes, reinterpret_cast<const f4*>(posm), vel, phi, out_rows);
  return launch_status();
}

}  // extern "C"
