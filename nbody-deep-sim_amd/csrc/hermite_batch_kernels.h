// hermite_batch_kernels.h -- what the two batched shared-timestep Hermite translation units share
// (direct_batch_hermite.hip: fp32 state; direct_batch_hermite_f64.hip: fp64 state, its 4th order): the two O(N) kernels of
// a step of every scene, templates of the state's scalar type T (batch_hermite_predict_kernel<T>,
// batch_hermite_correct_kernel<T>), each unit instantiating its own. They are the shared step's two kernels
// (hermite_predict_kernel<T>, hermite_correct_kernel<T> of hermite_kernels.h) with the prologue of a batch: the row's
// scene from the plan (direct_batch_plan.h) and the scene's own scalars from device tables, given as typed pointers to
// table rows -- step: T[HermiteStepRow::kRows][S], field k of scene s at step[k * S + s] (the fp32 entries' hdt; rows
// kStep.. of the fp64 entries' par); g: T[S], G_s (the fp32 entries' g_const; row kG of par). The per-body arithmetic is
// hermite_kernels.h's (hermite_predict_row, hermite_slab_sum, hermite_correct_row), so a scene has the one-system step's
// bits in either format. The 6th order's two kernels have no fp32 form and stay in direct_batch_hermite_f64.hip.
// The definitions sit in an anonymous namespace: every translation unit that includes this file gets its own inlined copies.
#pragma once
#include "direct_batch_plan.h"
#include "hermite_kernels.h"

namespace {

// Where a scene's slabs T[slabs][6][n] start, in units of its record's ws_off: the fp32 plan counts the leapfrog's
// float[slabs][n][3] and the Hermite slabs lie at twice that; an fp64 plan counts the doubles themselves.
template <class T> constexpr int kSlabsPerWsOff = 1;
template <> constexpr int kSlabsPerWsOff<float> = 2;

// posm[r] = {x_p, m}, velp[r] = {v_p, 0} for every packed row r (zero rows behind each scene's last body), one thread per
// row. acc == nullptr: a plain pack of (x, v); step is not read.
template <class T>
__global__ __launch_bounds__(256) void batch_hermite_predict_kernel(const int* __restrict__ row_scene,
                                                                    const SceneRec* __restrict__ scenes, int n_rows,
                                                                    const T* __restrict__ pos, const T* __restrict__ vel,
                                                                    const T* __restrict__ acc, const T* __restrict__ jerk,
                                                                    const T* __restrict__ mass,
                                                                    const T* __restrict__ step, int n_scenes,
                                                                    typename HermiteFmt<T>::Row* __restrict__ posm,
                                                                    typename HermiteFmt<T>::Row* __restrict__ velp) {
  PlanRow w;
  if (!load_row(row_scene, scenes, n_rows, w)) return;
  typename HermiteFmt<T>::Row pm = HermiteFmt<T>::zero(), vp = HermiteFmt<T>::zero();
  if (w.i() < w.sc.n) {
    const size_t b = (size_t)w.sc.off + w.i();
    const T dt = acc ? step[HermiteStepRow::kDt * n_scenes + w.s] : (T)0;
    const T dt2_half = acc ? step[HermiteStepRow::kDt2Half * n_scenes + w.s] : (T)0;
    const T dt3_sixth = acc ? step[HermiteStepRow::kDt3Sixth * n_scenes + w.s] : (T)0;
    const PosVel3<T> p = hermite_predict_row(pos, vel, acc, jerk, b, dt, dt2_half, dt3_sixth, acc != nullptr);
    pm = hermite_row(p.x, mass[b]);
    vp = hermite_row(p.v, (T)0);
  }
  posm[w.r] = pm;
  velp[w.r] = vp;
}

// One workgroup per HermiteFmt<T>::kSumRows packed rows (grid = ceil(n_rows / kSumRows)), row = hermite_sum_row<T>():
// a1, j1 = hermite_slab_sum of the body's row in its scene's slabs (ws + kSlabsPerWsOff<T> * ws_off), scaled by G_s.
// pos == nullptr: write a1, j1 only. Else hermite_correct_row: reads a0, j0 (acc_in / jerk_in may alias acc_out /
// jerk_out: each element is read before it is written, by the same thread), x, v; writes x1, v1, a1, j1 and posm =
// {x1, m} for the energies after the step.
// float : 64 rows per workgroup, one chunk: a scene's rows are whole chunks, so the workgroup lies in one scene and reads
//         it at its first row (once, into SGPRs), and n_rows is a whole number of workgroups: no thread leaves before
//         the barrier of hermite_slab_sum.
// double: 256 rows per workgroup, each thread its own row's scene; n_rows is a multiple of 64, not of 256, so the
//         threads behind the last row leave at once (there is no barrier).
template <class T>
__global__ __launch_bounds__(256) void batch_hermite_correct_kernel(const int* __restrict__ row_scene,
                                                                    const SceneRec* __restrict__ scenes, int n_rows,
                                                                    const T* __restrict__ ws, const T* __restrict__ g,
                                                                    const T* __restrict__ step, int n_scenes, T* pos,
                                                                    T* vel, const T* acc_in, const T* jerk_in,
                                                                    T* acc_out, T* jerk_out, const T* __restrict__ mass,
                                                                    typename HermiteFmt<T>::Row* __restrict__ posm) {
  constexpr int kRows = HermiteFmt<T>::kSumRows;
  static_assert(kRows % kChunk == 0, "a workgroup covers whole chunks");
  PlanRow w;
  w.r = (int)hermite_sum_row<T>();
  if constexpr (kRows > kChunk) {
    if (w.r >= n_rows) return;
  }
  w.s = row_scene[kRows == kChunk ? (int)blockIdx.x * kChunk : w.r];
  w.sc = load_scene(scenes, w.s);
  T a1[3], j1[3];
  if (!hermite_slab_sum(ws + kSlabsPerWsOff<T> * (size_t)w.sc.ws_off, w.sc.slabs, w.sc.n, (size_t)w.i(),
                        w.i() < w.sc.n, g[w.s], a1, j1))
    return;
  const size_t b = (size_t)w.sc.off + w.i();
  if (pos) {
    const Corrected<T> c =
        hermite_correct_row(pos, vel, acc_in, jerk_in, b, a1, j1, step[HermiteStepRow::kDtHalf * n_scenes + w.s],
                            step[HermiteStepRow::kDt2Twelfth * n_scenes + w.s]);
    posm[w.r] = hermite_row(c.x1, mass[b]);
  }
  hermite_store_force(acc_out, jerk_out, b, a1, j1);
}

}  // namespace
