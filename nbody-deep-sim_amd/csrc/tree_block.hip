// tree_block.hip -- the O(N) stages of block timesteps over the tree force ("Block timesteps"): a
// hierarchical kick-drift-kick with individual power-of-two steps, as in GADGET-2. C-ABI: the nbd_tblock_* entries of
// include/nbd.h; Python: galaxify.simulation.BlockTreeLeapFrogSimulator.
//
// One output interval dt is 2^K ticks (K = max_level). Body i has a level k_i in [0, K], the step h_i = dt 2^-k_i =
// d_i = 2^(K - k_i) ticks, and the tick s_i at which its current step began (always a multiple of d_i). Its velocity is
// the mid-step one between the opening kick of a step and its closing kick. One step():
//   open    every body: v += a h_i / 2, s_i = 0, and the drift's rounding residual = 0
//   then, until t_next = 2^K, one block step:
//   drift   t_next = min_i (s_i + d_i) by an integer atomic min; every body: x += v (t_next - t_cur) dt / 2^K, and the
//           packed {x, y, z, m} rows the tree is built from, in the same launch. A body at a coarse level is drifted at
//           every block step with the SAME mid-step velocity, so the fp32 roundings of its position do not average out:
//           they repeat (measured: 3.3e-6 after 8 drifts where the shared step's 8 leave 1.1e-6; at K = 10 there are up
//           to 1024 per interval). The drift therefore carries its rounding residual from one block step to the next
//           (a compensated sum, one float per coordinate, zero at the start of every interval): over an interval a
//           position takes one rounding, as the shared step's does. The first drift of an interval has no residual:
//           it is x += c v as nbd_kick_drift_f32 forms it, to the bit
//   flag    flags[i] = (s_i + d_i == t_next): what nbd_tree_select_active compacts in tree order
//   (force on the listed bodies: csrc/tree_force.hip)
//   close   every flagged body: v += a h_i / 2, the new level from the criterion, and, unless the interval ends here, the
//           opening kick of the next step v += a h'_i / 2 and s_i = t_next
// The constants are formed in fp64 and rounded once to fp32 -- (float)(0.5 dt 2^-k) and (float)(dt ticks 2^-K), what a
// Python double gives when it meets an fp32 tensor -- and every update is v += c a; x += c v with the product and the sum
// rounded separately, as nbd_kick_drift_f32 and nbd_kick_f32 round them: with K = 0 the step is the shared-step tree
// leapfrog bit for bit.
// The criterion is the one of softened collisionless runs, h_i <= sqrt(2 eta eps / |a_i|), evaluated without a square
// root: the wanted level is the smallest k with h_k^4 (a.a) <= (2 eta eps)^2, in fp64 from the fp32 acceleration, a.a
// summed x, y, z with separate multiplies and adds (-ffp-contract=off), so that a host restatement reproduces it exactly.
// A level may deepen at any block step; it rises by one, and only when t_next is a multiple of the coarser step's ticks.
// A level wanted deeper than K is clamped and counted, a NaN criterion too. No float atomics: the results are the same
// from run to run.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nbd.h"

namespace {

// the schedule record (device int[NBD_TBLOCK_SCHED_INTS])
constexpr int kTNext = 0;      // the tick of the block step that is running (flag writes it)
constexpr int kNAct = 1;       // its active bodies (nbd_tree_select_active writes it: the caller points it here)
constexpr int kClamped = 2;    // cumulative
constexpr int kTCur = 3;       // the tick every position is at
constexpr int kTMin = 4;       // min_i (s_i + d_i) while it is being reduced; INT_MAX between block steps

constexpr int kMaxLevel = 20;

inline bool bad_level(int K) { return K < 0 || K > kMaxLevel; }
inline int blocks_of(int n) { return (n + 255) / 256; }
inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// the smallest k in [0, K] with (dt 2^-k)^4 (a.a) <= lim; none (or a NaN): K, and `over` is set
__device__ inline int level_wanted(const float* a, double dt, double lim, int K, bool& over) {
  const double x = a[0], y = a[1], z = a[2];
  const double aa = x * x + y * y + z * z;
  for (int k = 0; k <= K; ++k) {
    const double h = dt * ldexp(1.0, -k), h2 = h * h, h4 = h2 * h2;
    if (h4 * aa <= lim) { over = false; return k; }
  }
  over = true;
  return K;
}

__device__ inline float half_step(double dt, int k) { return (float)(0.5 * dt * ldexp(1.0, -k)); }

// v += c a, product and sum rounded separately
__device__ inline void kick3(float* v, const float* a, float c) {
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = __fadd_rn(v[k], __fmul_rn(c, a[k]));
}

__device__ inline void count_clamped(bool over, int* sched) {
  const unsigned long long m = __ballot(over);
  if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(&sched[kClamped], __popcll(m));
}

__global__ __launch_bounds__(256) void tblock_init_kernel(const float* __restrict__ acc, int n, double dt, double lim, int K,
                                                          int* __restrict__ ticks, int* __restrict__ levels,
                                                          int* __restrict__ sched) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool over = false;
  if (i < n) {
    const float a[3] = {acc[3 * i], acc[3 * i + 1], acc[3 * i + 2]};
    levels[i] = level_wanted(a, dt, lim, K, over);
    ticks[i] = 0;
  }
  count_clamped(over, sched);
  if (i == 0) { sched[kTNext] = 0; sched[kNAct] = 0; sched[kTCur] = 0; sched[kTMin] = INT_MAX; }
}

__global__ __launch_bounds__(256) void tblock_open_kernel(float* __restrict__ vel, const float* __restrict__ acc,
                                                          const int* __restrict__ levels, int* __restrict__ ticks,
                                                          float* __restrict__ residual, int n, double dt,
                                                          int* __restrict__ sched) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) { sched[kTCur] = 0; sched[kTMin] = INT_MAX; }
  if (i >= n) return;
  float v[3] = {vel[3 * i], vel[3 * i + 1], vel[3 * i + 2]};
  const float a[3] = {acc[3 * i], acc[3 * i + 1], acc[3 * i + 2]};
  kick3(v, a, half_step(dt, levels[i]));
  for (int k = 0; k < 3; ++k) { vel[3 * i + k] = v[k]; residual[3 * i + k] = 0.f; }
  ticks[i] = 0;
}

// sched[kTMin] = min(sched[kTMin], min_i (s_i + d_i)): one integer atomic per wave
__global__ __launch_bounds__(256) void tblock_min_kernel(const int* __restrict__ levels, const int* __restrict__ ticks, int n,
                                                         int K, int* __restrict__ sched) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  int t = i < n ? ticks[i] + (1 << (K - levels[i])) : INT_MAX;
  for (int d = 32; d > 0; d >>= 1) t = min(t, __shfl_xor(t, d));
  if ((threadIdx.x & 63) == 0 && t != INT_MAX) atomicMin(&sched[kTMin], t);
}

// x += c v with c = (float)(dt (t_next - t_cur) 2^-K), compensated: y = c v - r; t = x + y; r = (t - x) - y; x = t (every
// operation rounded by itself; r = 0 makes it x += c v); posm = {x, m}, zeros behind body n - 1
__global__ __launch_bounds__(256) void tblock_drift_kernel(float* __restrict__ pos, const float* __restrict__ vel,
                                                           const float* __restrict__ mass, float* __restrict__ residual,
                                                           int n, int n_pad, double dt, int K,
                                                           const int* __restrict__ sched, float4* __restrict__ posm) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pad) return;
  float4 pm = {0.f, 0.f, 0.f, 0.f};
  if (i < n) {
    const float c = (float)(dt * (double)(sched[kTMin] - sched[kTCur]) * ldexp(1.0, -K));
    float x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float x0 = pos[3 * i + k];
      const float y = __fsub_rn(__fmul_rn(c, vel[3 * i + k]), residual[3 * i + k]);
      x[k] = __fadd_rn(x0, y);
      residual[3 * i + k] = __fsub_rn(__fsub_rn(x[k], x0), y);
      pos[3 * i + k] = x[k];
    }
    pm = float4{x[0], x[1], x[2], mass[i]};
  }
  posm[i] = pm;
}

__global__ __launch_bounds__(256) void tblock_flag_kernel(const int* __restrict__ levels, const int* __restrict__ ticks, int n,
                                                          int K, int* __restrict__ sched, int* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int t_next = sched[kTMin];
  if (i == 0) sched[kTNext] = t_next;
  if (i < n) flags[i] = ticks[i] + (1 << (K - levels[i])) == t_next;
}

__global__ __launch_bounds__(256) void tblock_close_kernel(float* __restrict__ vel, const float* __restrict__ acc,
                                                           const int* __restrict__ flags, int* __restrict__ levels,
                                                           int* __restrict__ ticks, int n, int K, double dt, double lim,
                                                           int* __restrict__ sched) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int t_next = sched[kTNext], end = 1 << K;
  bool over = false;
  if (i < n && flags[i]) {
    float v[3] = {vel[3 * i], vel[3 * i + 1], vel[3 * i + 2]};
    const float a[3] = {acc[3 * i], acc[3 * i + 1], acc[3 * i + 2]};
    int k = levels[i];
    kick3(v, a, half_step(dt, k));                           // the step that ends here
    const int want = level_wanted(a, dt, lim, K, over);
    if (want > k) k = want;
    else if (want < k && t_next % (1 << (K - k + 1)) == 0) k -= 1;
    if (t_next < end) kick3(v, a, half_step(dt, k));         // the step that begins here
    for (int c = 0; c < 3; ++c) vel[3 * i + c] = v[c];
    levels[i] = k;
    ticks[i] = t_next < end ? t_next : 0;
  }
  count_clamped(over, sched);
  // (every thread of this launch reads kTNext alone; kTCur and kTMin are read by the next block step's launches)
  if (i == 0) { sched[kTCur] = t_next < end ? t_next : 0; sched[kTMin] = INT_MAX; }
}

}  // namespace

extern "C" {

int nbd_tblock_init_levels(const float* acc, int n, double dt, double eta, double softening, int max_level, int* ticks,
                           int* levels, int* sched, nbd_stream_t stream) {
  if (n < 0 || bad_level(max_level) || !(dt > 0.0) || !(eta > 0.0) || !(softening > 0.0) || !sched) return NBD_E_BADARG;
  if (n > 0 && (!acc || !ticks || !levels)) return NBD_E_BADARG;
  const double c = 2.0 * eta * softening;
  tblock_init_kernel<<<blocks_of(n > 0 ? n : 1), 256, 0, (hipStream_t)stream>>>(acc, n, dt, c * c, max_level, ticks, levels,
                                                                                sched);
  return launch_status();
}

int nbd_tblock_open(float* vel, const float* acc, const int* levels, int* ticks, float* residual, int n, int max_level,
                    double dt, int* sched, nbd_stream_t stream) {
  if (n <= 0 || bad_level(max_level) || !(dt > 0.0) || !vel || !acc || !levels || !ticks || !residual || !sched)
    return NBD_E_BADARG;
  tblock_open_kernel<<<blocks_of(n), 256, 0, (hipStream_t)stream>>>(vel, acc, levels, ticks, residual, n, dt, sched);
  return launch_status();
}

int nbd_tblock_drift(float* pos, const float* vel, const float* mass, const int* levels, const int* ticks, float* residual,
                     int n, int max_level, double dt, int* sched, float* posm, nbd_stream_t stream) {
  if (n <= 0 || bad_level(max_level) || !(dt > 0.0)) return NBD_E_BADARG;
  if (!pos || !vel || !mass || !levels || !ticks || !residual || !sched || !posm ||
      (reinterpret_cast<uintptr_t>(posm) & 15))
    return NBD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  tblock_min_kernel<<<blocks_of(n), 256, 0, st>>>(levels, ticks, n, max_level, sched);
  const int n_pad = nbd_posm_padded_len(n);
  tblock_drift_kernel<<<blocks_of(n_pad), 256, 0, st>>>(pos, vel, mass, residual, n, n_pad, dt, max_level, sched,
                                                        reinterpret_cast<float4*>(posm));
  return launch_status();
}

int nbd_tblock_flag(const int* levels, const int* ticks, int n, int max_level, int* sched, int* flags, nbd_stream_t stream) {
  if (n <= 0 || bad_level(max_level) || !levels || !ticks || !sched || !flags) return NBD_E_BADARG;
  tblock_flag_kernel<<<blocks_of(n), 256, 0, (hipStream_t)stream>>>(levels, ticks, n, max_level, sched, flags);
  return launch_status();
}

int nbd_tblock_close(float* vel, const float* acc, const int* flags, int* levels, int* ticks, int n, int max_level, double dt,
                     double eta, double softening, int* sched, nbd_stream_t stream) {
  if (n <= 0 || bad_level(max_level) || !(dt > 0.0) || !(eta > 0.0) || !(softening > 0.0)) return NBD_E_BADARG;
  if (!vel || !acc || !flags || !levels || !ticks || !sched) return NBD_E_BADARG;
  const double c = 2.0 * eta * softening;
  tblock_close_kernel<<<blocks_of(n), 256, 0, (hipStream_t)stream>>>(vel, acc, flags, levels, ticks, n, max_level, dt, c * c,
                                                                     sched);
  return launch_status();
}

}  // extern "C"
