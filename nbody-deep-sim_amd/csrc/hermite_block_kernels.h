// hermite_block_kernels.h -- what the two block-timestep translation units share (direct_hermite_block.hip: fp32 state;
// direct_hermite_block_f64.hip: fp64 state, 4th and 6th order): the layout of the schedule record, the level arithmetic
// (criterion, wanted_level, norm3), the re-levelling of a corrected body (hblock_relevel), the three O(N) kernels as
// templates of the state's scalar type T (hblock_init_kernel<T>, hblock_predict_kernel<T>, hblock_correct_kernel<T>), each
// unit instantiating its own, and the host body of the initial-levels entries (hblock_init_levels<T>). Levels, ticks and
// the schedule are integers and the criterion is evaluated in fp64 in both modes, so there is one copy of each; the
// scheduler itself (hblock_schedule_kernel, direct_hermite_block.hip) looks at nothing else and serves both. The per-body
// arithmetic is hermite_kernels.h's (hermite_predict_row, hermite_slab_sum, hermite_correct_row), the step constants
// hermite_step_constants<T> of the body's own fp64 step: a body whose step is the whole interval gets the shared step's
// bits.
// direct_batch_hermite_block_f64.hip (both orders for every scene of a batch) takes the record's layout, the level
// arithmetic, hblock_ticks_len, hblock_initial_level and the two re-levelling functions from here and has kernels of its own.
// The 6th order of the fp64 unit takes the record, the level arithmetic, the initial levels, hblock_move_level and
// hblock6_relevel from here and has O(N) kernels of its own, in that unit, over hermite6_f64_kernels.h's rows.
// direct_hermite_block_split_f64.hip (a block step divided over the ranks of a process group) corrects a slice without
// touching the state and books all rows in a launch of its own, so the re-levelling is stated in its parts: the
// criterion's wanted level (hblock_wanted, hblock6_wanted), the level rules (hblock_next_level, pure) and the bookkeeping
// (hblock_book_level); hblock_move_level, hblock_relevel and hblock6_relevel are their compositions.
// The definitions sit in an anonymous namespace: every translation unit that includes this file gets its own inlined copies.
#pragma once
#include <math.h>

#include "direct_kernels.h"
#include "hermite_kernels.h"

namespace {

constexpr int kMaxLevel = 20;        // 2^20 ticks per interval: the tick count fits an int32 with room for t_i + d_i

// sched[NBD_HBLOCK_SCHED_INTS]: t_next and n_act of the block step being taken, the cumulative clamp count, the tick T
// every body has reached (the last t_next, 0 at the start of an interval), the compaction's write cursor and its count
// of finished workgroups (both 0 between launches), the flag a split block step raises when the ranks' headers disagree
// (direct_hermite_block_split_f64.hip; 0 otherwise), and the level histogram (bin k: bodies at level k)
enum { kTNext = 0, kNAct = 1, kClamped = 2, kTCur = 3, kCursor = 4, kDone = 5, kDiverged = 6, kHist = 8 };
static_assert(kHist + kMaxLevel + 1 <= NBD_HBLOCK_SCHED_INTS, "sched holds the level histogram");

inline bool bad_level(int K) { return K < 0 || K > kMaxLevel; }

// The Aarseth criterion sqrt(eta num / den). den = 0 (no jerk and no higher derivative: a lone body, or one in a
// uniform field) allows any step: +inf, not the NaN of 0/0. A NaN that comes from NaN forces stays NaN (clamped).
__device__ __forceinline__ double criterion(double eta, double num, double den) {
  return den == 0.0 ? INFINITY : sqrt(eta * num / den);
}

// The level a criterion value asks for: the smallest k >= 0 with dt 2^-k <= crit, compared against the exact powers of
// two. K + 1 means "deeper than K" (also for NaN, which no comparison accepts); +inf gives 0.
__device__ __forceinline__ int wanted_level(double crit, double dt, int K) {
  int k = 0;
  double step = dt;
  while (k <= K && !(step <= crit)) {
    ++k;
    step *= 0.5;
  }
  return k;
}

__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// The length of `ticks` ticks of an interval dt of 2^K ticks (tick = 2^-K): a body's elapsed time since its last
// correction (the predictors) and its own step (the correctors), in the one-system units and in the batched one
// (direct_batch_hermite_block_f64.hip, where dt is the scene's).
__device__ __forceinline__ double hblock_ticks_len(double dt, int ticks, double tick) { return dt * (double)ticks * tick; }

// The initial level of body i from dt_i = (eta / 2) |a| / |j| in fp64 (+inf where j = 0): K + 1 where deeper than K.
template <class T>
__device__ __forceinline__ int hblock_initial_level(const T* __restrict__ acc, const T* __restrict__ jerk, size_t i,
                                                    int K, double dt, double eta) {
  const double a = norm3(acc[3 * i], acc[3 * i + 1], acc[3 * i + 2]);
  const double j = norm3(jerk[3 * i], jerk[3 * i + 1], jerk[3 * i + 2]);
  return wanted_level(j == 0.0 ? INFINITY : 0.5 * eta * a / j, dt, K);
}

// Initial levels from dt_i = (eta / 2) |a| / |j| in fp64 (+inf where j = 0); every tick to 0. Levels deeper than K are
// clamped and counted.
template <class T>
__global__ __launch_bounds__(256) void hblock_init_kernel(const T* __restrict__ acc, const T* __restrict__ jerk, int n,
                                                          int K, double dt, double eta, int* __restrict__ ticks,
                                                          int* __restrict__ levels, int* __restrict__ sched) {
  __shared__ int hist[kMaxLevel + 1];
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x <= K) hist[threadIdx.x] = 0;
  __syncthreads();
  if (i < (size_t)n) {
    int k = hblock_initial_level(acc, jerk, i, K, dt, eta);
    if (k > K) {
      k = K;
      atomicAdd(&sched[kClamped], 1);
    }
    ticks[i] = 0;
    levels[i] = k;
    atomicAdd(&hist[k], 1);
  }
  __syncthreads();
  if (threadIdx.x <= K && hist[threadIdx.x]) atomicAdd(&sched[kHist + threadIdx.x], hist[threadIdx.x]);
}

// The host body of nbd_hblock_init_levels (T = float) and nbd_hblock_init_levels_f64 (T = double).
template <class T>
int hblock_init_levels(const T* acc, const T* jerk, int n, double dt, double eta, int max_level, int* ticks, int* levels,
                       int* sched, hipStream_t st) {
  if (n < 0 || bad_level(max_level) || !(dt > 0.0) || !(eta > 0.0)) return NBD_E_BADARG;
  if (!sched) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (!acc || !jerk || !ticks || !levels) return NBD_E_BADARG;
  // T, the cursor and the histogram start from zero; t_next, n_act and the clamp count are left as they are
  hipError_t e = hipMemsetAsync(sched + kTCur, 0, (NBD_HBLOCK_SCHED_INTS - kTCur) * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  hblock_init_kernel<T><<<ceil_div(n, 256), 256, 0, st>>>(acc, jerk, n, max_level, dt, eta, ticks, levels, sched);
  return launch_status();
}

// posm = {x_p, m}, velp = {v_p, 0} for rows [0, n_pad) (zero rows behind n): every body predicted from its last
// correction to t_next = sched[kTNext] by hermite_predict_row over Delta_i = (t_next - t_i) dt / 2^K, its constants from
// hermite_step_constants<T> (dt, dt2_half and dt3_sixth are used).
template <class T>
__global__ __launch_bounds__(256) void hblock_predict_kernel(const T* __restrict__ pos, const T* __restrict__ vel,
                                                             const T* __restrict__ acc, const T* __restrict__ jerk,
                                                             const T* __restrict__ mass, const int* __restrict__ ticks,
                                                             int n, int n_pad, double dt, double tick,
                                                             const int* __restrict__ sched,
                                                             typename HermiteFmt<T>::Row* __restrict__ posm,
                                                             typename HermiteFmt<T>::Row* __restrict__ velp) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n_pad) return;
  typename HermiteFmt<T>::Row pm = HermiteFmt<T>::zero(), vp = HermiteFmt<T>::zero();
  if (i < (size_t)n) {
    const HermiteStep<T> h = hermite_step_constants<T>(hblock_ticks_len(dt, sched[kTNext] - ticks[i], tick));
    const PosVel3<T> p = hermite_predict_row(pos, vel, acc, jerk, i, h.dt, h.dt2_half, h.dt3_sixth, true);
    pm = hermite_row(p.x, mass[i]);
    vp = hermite_row(p.v, (T)0);
  }
  posm[i] = pm;
  velp[i] = vp;
}

// The level rules of a corrected body at level lev (step d ticks) whose criterion wants level `want`, at the block step
// to t_next: shrink freely; grow by one level where t_next is a multiple of 2 d; deeper than K (NaN included) clamped,
// which `clamped` reports. Pure: direct_hermite_block_split_f64.hip forms a result row from it and books it elsewhere.
__device__ __forceinline__ int hblock_next_level(int want, int K, int lev, int d, int t_next, bool& clamped) {
  int nl = lev;
  clamped = false;
  if (want > lev) {
    nl = want;
    if (nl > K) {
      nl = K;
      clamped = true;
    }
  } else if (want < lev && (t_next & (2 * d - 1)) == 0) {
    nl = lev - 1;
  }
  return nl;
}

// The bookkeeping of a corrected body i that goes from level lev to nl at the block step to t_next: a clamp is counted,
// the body moves in the level histogram, t_i = t_next (0 at 2^K); `first` (one thread of the launch) publishes that tick
// as sched[kTCur].
__device__ __forceinline__ void hblock_book_level(int nl, bool clamped, int K, int lev, int t_next, int i, bool first,
                                                  int* __restrict__ ticks, int* __restrict__ levels,
                                                  int* __restrict__ sched) {
  if (clamped) atomicAdd(&sched[kClamped], 1);
  if (nl != lev) {
    atomicSub(&sched[kHist + lev], 1);
    atomicAdd(&sched[kHist + nl], 1);
  }
  levels[i] = nl;
  const int t_now = t_next == (1 << K) ? 0 : t_next;
  ticks[i] = t_now;
  if (first) sched[kTCur] = t_now;
}

// Both for a body corrected in place: hblock_next_level's rules, then hblock_book_level.
__device__ __forceinline__ void hblock_move_level(int want, int K, int lev, int d, int i, bool first,
                                                  int* __restrict__ ticks, int* __restrict__ levels,
                                                  int* __restrict__ sched) {
  const int t_next = sched[kTNext];
  bool clamped;
  const int nl = hblock_next_level(want, K, lev, d, t_next, clamped);
  hblock_book_level(nl, clamped, K, lev, t_next, i, first, ticks, levels, sched);
}

// The new level of body i, corrected from (a0, j0) to (a1, j1) over its step h = d ticks at level lev, from the Aarseth
// criterion in fp64, by hblock_move_level's rules.
//   a3 =(12 (a0 - a1) + 6 h (j0 + j1)) / h^3, a2(t1) = (-6 (a0 - a1) - h (4 j0 + 2 j1)) / h^2 + h a3
template <class T>
__device__ __forceinline__ int hblock_wanted(const T* a0, const T* j0, const T* a1, const T* j1, double h, double dt,
                                             double eta, int K) {
  double a3[3], a2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double da = (double)a0[k] - (double)a1[k];
    a3[k] = (12.0 * da + 6.0 * h * ((double)j0[k] + (double)j1[k])) / (h * h * h);
    a2[k] = (-6.0 * da - h * (4.0 * (double)j0[k] + 2.0 * (double)j1[k])) / (h * h) + h * a3[k];
  }
  const double na1 = norm3(a1[0], a1[1], a1[2]), nj1 = norm3(j1[0], j1[1], j1[2]);
  const double na2 = norm3(a2[0], a2[1], a2[2]), na3 = norm3(a3[0], a3[1], a3[2]);
  return wanted_level(criterion(eta, na1 * na2 + nj1 * nj1, nj1 * na3 + na2 * na2), dt, K);
}

template <class T>
__device__ __forceinline__ void hblock_relevel(const T* a0, const T* j0, const T* a1, const T* j1, double h, double dt,
                                               double eta, int K, int lev, int d, int i, bool first,
                                               int* __restrict__ ticks, int* __restrict__ levels,
                                               int* __restrict__ sched) {
  hblock_move_level(hblock_wanted(a0, j0, a1, j1, h, dt, eta, K), K, lev, d, i, first, ticks, levels, sched);
}

// ... and of a 6th-order body (direct_hermite_block_f64.hip), corrected from (a0, j0, s0) to (a1, j1, s1) with the
// crackle c1 just formed: the generalised criterion of Nitadori & Makino (2008) for p = 6, with eta in the 4th-order
// convention (dt_i = sqrt(eta ...) there),
//   dt_i = (eta^3 (|a1||s1| + |j1|^2) / (|c1||a5| + |a4(t1)|^2))^(1/6)  = cbrt(criterion(eta^3, num, den)),
// from the derivatives of the quintic through both ends,
//   a5 = (720 (a1 - a0) - 360 h (j1 + j0) + 60 h^2 (s1 - s0)) / h^5
//   a4(t1) = (-360 (a1 - a0) + h (168 j1 + 192 j0) + h^2 (-24 s1 + 36 s0)) / h^4 + h a5,   a3(t1) = c1.
// Every operation rounds on its own (the build has -ffp-contract=off). The level rules are hblock_move_level's.
__device__ __forceinline__ int hblock6_wanted(const double* a0, const double* j0, const double* s0, const double* a1,
                                              const double* j1, const double* s1, const double* c1, double h, double dt,
                                              double eta, int K) {
  double a4[3], a5[3];
  const double h2 = h * h, h4 = h2 * h2, h5 = h4 * h;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double da = a1[k] - a0[k];
    a5[k] = ((720.0 * da - 360.0 * h * (j1[k] + j0[k])) + 60.0 * h2 * (s1[k] - s0[k])) / h5;
    a4[k] = ((-360.0 * da + h * (168.0 * j1[k] + 192.0 * j0[k])) + h2 * (-24.0 * s1[k] + 36.0 * s0[k])) / h4 + h * a5[k];
  }
  const double na1 = norm3(a1[0], a1[1], a1[2]), nj1 = norm3(j1[0], j1[1], j1[2]), ns1 = norm3(s1[0], s1[1], s1[2]);
  const double nc1 = norm3(c1[0], c1[1], c1[2]), na4 = norm3(a4[0], a4[1], a4[2]), na5 = norm3(a5[0], a5[1], a5[2]);
  return wanted_level(cbrt(criterion(eta * eta * eta, na1 * ns1 + nj1 * nj1, nc1 * na5 + na4 * na4)), dt, K);
}

__device__ __forceinline__ void hblock6_relevel(const double* a0, const double* j0, const double* s0, const double* a1,
                                                const double* j1, const double* s1, const double* c1, double h,
                                                double dt, double eta, int K, int lev, int d, int i, bool first,
                                                int* __restrict__ ticks, int* __restrict__ levels,
                                                int* __restrict__ sched) {
  hblock_move_level(hblock6_wanted(a0, j0, s0, a1, j1, s1, c1, h, dt, eta, K), K, lev, d, i, first, ticks, levels,
                    sched);
}

// The active bodies' corrector, one workgroup per HermiteFmt<T>::kSumRows consecutive list entries: a1, j1 =
// hermite_slab_sum of the entry's row p. pos == nullptr: write a1, j1 in list order only (the force on its own). Else, for
// body i = act[p] with its own step h = dt 2^-k_i: hermite_correct_row with hermite_step_constants<T>(h) (only dt_half and
// dt2_twelfth are used; the other three are never formed), a1, j1, posm = {x1, m}, then hblock_relevel.
template <class T>
__global__ __launch_bounds__(256) void hblock_correct_kernel(const T* __restrict__ slabs, int n_slabs,
                                                             const int* __restrict__ act, int n_act, T g, int K,
                                                             double dt, double tick, double eta, T* pos, T* vel, T* acc,
                                                             T* jerk, const T* __restrict__ mass, int* __restrict__ ticks,
                                                             int* __restrict__ levels, int* __restrict__ sched,
                                                             typename HermiteFmt<T>::Row* __restrict__ posm) {
  const size_t p = hermite_sum_row<T>();
  T a1[3], j1[3];
  if (!hermite_slab_sum(slabs, n_slabs, n_act, p, p < (size_t)n_act, g, a1, j1)) return;
  if (!pos) {
    hermite_store_force(acc, jerk, p, a1, j1);
    return;
  }
  const int i = act[p];
  const int lev = levels[i];
  const int d = 1 << (K - lev);
  const double h = hblock_ticks_len(dt, d, tick);
  const HermiteStep<T> hc = hermite_step_constants<T>(h);
  const Corrected<T> c = hermite_correct_row(pos, vel, acc, jerk, (size_t)i, a1, j1, hc.dt_half, hc.dt2_twelfth);
  hermite_store_force(acc, jerk, (size_t)i, a1, j1);
  posm[i] = hermite_row(c.x1, mass[i]);
  hblock_relevel(c.a0, c.j0, a1, j1, h, dt, eta, K, lev, d, i, p == 0, ticks, levels, sched);
}

}  // namespace
