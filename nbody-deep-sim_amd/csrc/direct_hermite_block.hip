// direct_hermite_block.hip -- block-timestep 4th-order Hermite integration (Makino & Aarseth 1992) for the direct force
// path on gfx950 (MI355X). An extension: the reference has Euler and kick-drift-kick leapfrog only. C-ABI: the
// nbd_hblock_* / nbd_accel_jerk_active_f32 entries of include/nbd.h; Python: galaxify.simulation.BlockHermiteSimulator.
//
// One output interval dt is 2^K integer ticks (K = max_level). Body i carries x, v, a, j at its last correction tick
// t_i and a level k_i in [0, K]: its step is d_i = 2^(K - k_i) ticks, and t_i is always a multiple of d_i. One block step:
//   schedule : t_next = min_i (t_i + d_i), the active list {i : t_i + d_i = t_next}. Under the block condition every
//              body at level k is due at the first multiple of d_k after the current tick T, so t_next is the integer
//              min of that over the levels present (a device histogram of the levels), and the active bodies are those
//              whose d_i divides t_next: level >= K - ctz(t_next). A multi-block compaction writes the list.
//   predict  : every body to t_next with its own Delta_i = t_next - t_i ticks -> posm = {x_p, m}, velp = {v_p, 0}
//   evaluate : accel_jerk_active_kernel -- a1, j1 of the active targets under all n predicted sources, into
//              float[slabs][6][n_act] partial sums (accel_jerk_kernel's arithmetic and source order)
//   correct  : fixed-order slab sum, the corrector with the body's own step h = d_i, the Aarseth criterion in fp64 for the
//              new level, t_i = t_next (0 at the end of the interval), posm = {x1, m}
// Predictor, force body, slab sum and corrector are the shared step's own functions (hermite_kernels.h), and the fp32
// step constants come from hermite_dt() on the body's fp64 step (dt times its tick count): a body whose Delta is the
// whole interval gets the shared step's bits. No float atomics (the clamp counter is an integer
// atomic); the host reads {t_next, n_act} once per block step, so the path is eager-only.
// The schedule record's layout and the level arithmetic (criterion, wanted_level, norm3) live in hermite_block_kernels.h,
// shared with the float64 form of this unit, direct_hermite_block_f64.hip; hblock_schedule_kernel serves both.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_kernels.h"
#include "hermite_block_kernels.h"
#include "hermite_kernels.h"

namespace {

constexpr int kActSlabTarget = 512;  // small active sets: raise the slab count until groups x slabs reaches ~2 per CU
constexpr int kActMaxSlabs = 256;

// Acceleration + jerk of the n_act targets act[0..n_act) under all n sources: accel_jerk_kernel<MASKED, 2> with its
// targets gathered through the index list (the same accel_jerk_body, so the same chunk stream and wave reduction).
// Grid = (ceil(n_act / 128), slabs), block = 4 waves. The lanes behind n_act repeat the last target and store nothing.
// out: float[slab][6][n_act], in list order. A target's sums depend only on n and the slab count, not on where it sits
// in the list.
template <bool MASKED>
__global__ __launch_bounds__(64 * kWaves, 6) void accel_jerk_active_kernel(
    const f4* __restrict__ posm, const f4* __restrict__ velp, int n, const int* __restrict__ act, int n_act, int cpw_q,
    int cpw_r, float eps2, float* __restrict__ out) {
  __shared__ f4 lds[kWaves * 4 * kChunk];
  const int t_base = blockIdx.x * kTgtPerWG;
  const int l0 = t_base + (threadIdx.x & 63);
  const int i0 = act[min(l0, n_act - 1)], i1 = act[min(l0 + 64, n_act - 1)];
  const int jw = blockIdx.y * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int c_begin, c_end;
  wave_chunk_range(jw, cpw_q, cpw_r, c_begin, c_end);
  accel_jerk_body<MASKED, 2>(posm, velp, n, posm, velp, i0, i1, i0, i1, c_begin, c_end, eps2, lds,
                             out + (size_t)blockIdx.y * 6 * n_act + t_base, n_act, min(kTgtPerWG, n_act - t_base));
}

// Initial levels from dt_i = (eta / 2) |a| / |j| in fp64 (+inf where j = 0); every tick to 0. Levels deeper than K are clamped and counted.
__global__ __launch_bounds__(256) void hblock_init_kernel(const float* __restrict__ acc, const float* __restrict__ jerk,
                                                          int n, int K, double dt, double eta, int* __restrict__ ticks,
                                                          int* __restrict__ levels, int* __restrict__ sched) {
  __shared__ int hist[kMaxLevel + 1];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x <= K) hist[threadIdx.x] = 0;
  __syncthreads();
  if (i < n) {
    const double a = norm3(acc[3 * i], acc[3 * i + 1], acc[3 * i + 2]);
    const double j = norm3(jerk[3 * i], jerk[3 * i + 1], jerk[3 * i + 2]);
    int k = wanted_level(j == 0.0 ? INFINITY : 0.5 * eta * a / j, dt, K);
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

// t_next from the level histogram and the current tick T = sched[kTCur]; every block derives it alike. Each wave appends
// its active bodies at one integer atomic on the cursor, so the list order varies from run to run; a body's sums do not
// depend on its place in the list. Block 0 publishes t_next and n_act. The last workgroup to finish sets the cursor and
// the finished count back to 0, so every launch starts from a clean cursor.
__global__ __launch_bounds__(256) void hblock_schedule_kernel(const int* __restrict__ levels, int n, int K,
                                                              int* __restrict__ sched, int* __restrict__ act) {
  const int T = sched[kTCur];
  int t_next = INT_MAX;
  for (int k = 0; k <= K; ++k)
    if (sched[kHist + k] > 0) {
      const int d = 1 << (K - k);
      t_next = min(t_next, (T / d + 1) * d);
    }
  const int thr = max(0, K - __builtin_ctz(t_next));          // active: d_i divides t_next
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool on = i < n && levels[i] >= thr;
  const unsigned long long mask = __ballot(on);
  if (mask) {
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)mask) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&sched[kCursor], __popcll(mask));
    base = __shfl(base, leader);
    if (on) act[base + __popcll(mask & __lanemask_lt())] = i;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int n_act = 0;
    for (int k = thr; k <= K; ++k) n_act += sched[kHist + k];
    sched[kTNext] = t_next;
    sched[kNAct] = n_act;
  }
  __syncthreads();                                             // every wave of this workgroup has taken its places
  if (threadIdx.x == 0) {
    __threadfence();
    if (atomicAdd(&sched[kDone], 1) == (int)gridDim.x - 1) {   // the last workgroup: no cursor update can follow
      sched[kCursor] = 0;
      sched[kDone] = 0;
    }
  }
}

// posm = {x_p, m}, velp = {v_p, 0} for rows [0, n_pad) (zero padding behind n): every body predicted from its last
// correction to t_next = sched[0] by hermite_predict over Delta_i = (t_next - t_i) dt / 2^K, its constants from
// hermite_dt().
__global__ __launch_bounds__(256) void hblock_predict_kernel(const float* __restrict__ pos, const float* __restrict__ vel,
                                                             const float* __restrict__ acc, const float* __restrict__ jerk,
                                                             const float* __restrict__ mass, const int* __restrict__ ticks,
                                                             int n, int n_pad, double dt, double tick,
                                                             const int* __restrict__ sched, f4* __restrict__ posm,
                                                             f4* __restrict__ velp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pad) return;
  f4 pm = {0.f, 0.f, 0.f, 0.f}, vp = {0.f, 0.f, 0.f, 0.f};
  if (i < n) {
    const HermiteDt h = hermite_dt(dt * (double)(sched[kTNext] - ticks[i]) * tick);  // dt, dt2_half, dt3_sixth used
    float x[3], v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const PosVel p = hermite_predict(pos[3 * i + k], vel[3 * i + k], acc[3 * i + k], jerk[3 * i + k], h.dt, h.dt2_half,
                                       h.dt3_sixth);
      x[k] = p.x;
      v[k] = p.v;
    }
    pm = f4{x[0], x[1], x[2], mass[i]};
    vp = f4{v[0], v[1], v[2], 0.f};
  }
  posm[i] = pm;
  velp[i] = vp;
}

// The active bodies' corrector, one workgroup per 64 consecutive list entries: a1, j1 = hermite_slab_sum of the entry's
// row. pos == nullptr: write a1, j1 in list order only (the force on its own). Else, for body i = act[p] with its own step
// h = dt 2^-k_i: hermite_correct with hermite_dt(h), then the new level from the Aarseth criterion in fp64 (shrink freely;
// grow by one level where t_next is a multiple of 2 d_i; deeper than K clamped and counted), t_i = t_next (0 at 2^K),
// posm = {x1, m}.
__global__ __launch_bounds__(256) void hblock_correct_kernel(const float* __restrict__ slabs, int n_slabs,
                                                             const int* __restrict__ act, int n_act, float g, int K,
                                                             double dt, double tick, double eta, float* pos, float* vel,
                                                             float* acc, float* jerk, const float* __restrict__ mass,
                                                             int* __restrict__ ticks, int* __restrict__ levels,
                                                             int* __restrict__ sched, f4* __restrict__ posm) {
  __shared__ float part[4][6][64];
  const int p = blockIdx.x * 64 + (threadIdx.x & 63);
  float a1[3], j1[3];
  if (!hermite_slab_sum(slabs, n_slabs, n_act, p, p < n_act, g, part, a1, j1)) return;
  if (!pos) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      acc[3 * p + k] = a1[k];
      jerk[3 * p + k] = j1[k];
    }
    return;
  }
  const int i = act[p];
  const int lev = levels[i];
  const int d = 1 << (K - lev);
  const double h = dt * (double)d * tick;
  const HermiteDt hc = hermite_dt(h);  // only dt_half and dt2_twelfth are used; the other three are never formed
  float x1[3];
  double a0d[3], j0d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float a0 = acc[3 * i + k], j0 = jerk[3 * i + k];
    float x = pos[3 * i + k], v = vel[3 * i + k];
    hermite_correct(x, v, a0, j0, a1[k], j1[k], hc.dt_half, hc.dt2_twelfth);
    vel[3 * i + k] = v;
    pos[3 * i + k] = x1[k] = x;
    acc[3 * i + k] = a1[k];
    jerk[3 * i + k] = j1[k];
    a0d[k] = a0;
    j0d[k] = j0;
  }
  posm[i] = f4{x1[0], x1[1], x1[2], mass[i]};

  // Aarseth: a3 = (12 (a0 - a1) + 6 h (j0 + j1)) / h^3, a2(t1) = (-6 (a0 - a1) - h (4 j0 + 2 j1)) / h^2 + h a3
  double a3[3], a2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double da = a0d[k] - (double)a1[k];
    a3[k] = (12.0 * da + 6.0 * h * (j0d[k] + (double)j1[k])) / (h * h * h);
    a2[k] = (-6.0 * da - h * (4.0 * j0d[k] + 2.0 * (double)j1[k])) / (h * h) + h * a3[k];
  }
  const double na1 = norm3(a1[0], a1[1], a1[2]), nj1 = norm3(j1[0], j1[1], j1[2]);
  const double na2 = norm3(a2[0], a2[1], a2[2]), na3 = norm3(a3[0], a3[1], a3[2]);
  const double crit = criterion(eta, na1 * na2 + nj1 * nj1, nj1 * na3 + na2 * na2);
  const int want = wanted_level(crit, dt, K);
  const int t_next = sched[kTNext];
  int nl = lev;
  if (want > lev) {
    nl = want;
    if (nl > K) {
      nl = K;
      atomicAdd(&sched[kClamped], 1);
    }
  } else if (want < lev && (t_next & (2 * d - 1)) == 0) {
    nl = lev - 1;
  }
  if (nl != lev) {
    atomicSub(&sched[kHist + lev], 1);
    atomicAdd(&sched[kHist + nl], 1);
  }
  levels[i] = nl;
  const int t_now = t_next == (1 << K) ? 0 : t_next;
  ticks[i] = t_now;
  if (p == 0) sched[kTCur] = t_now;
}

// All targets active: the shared step's plan, nbd_accel_plan(n, n), so that the sums are bit-identical to it. Fewer: the
// plan of n_act targets, with the slab count raised until groups x slabs reaches kActSlabTarget (at least one chunk per
// wave, at most kActMaxSlabs).
JerkPlan plan_active(int n, int n_act) {
  JerkPlan p = plan_jerk(n, n_act);
  if (n_act < n && p.groups * p.slabs < kActSlabTarget) {
    int s = ceil_div(kActSlabTarget, p.groups);
    const int cap = p.n_chunks / kWaves < kActMaxSlabs ? p.n_chunks / kWaves : kActMaxSlabs;
    if (s > cap) s = cap;
    if (s > p.slabs) p.slabs = s;
  }
  return p;
}

size_t act_bytes(int n) { return (size_t)ceil_div(n, 4) * 4 * sizeof(int); }

// what one block step with n_act targets uses of the workspace: the list and its partial sums (O(1): one plan)
size_t step_bytes(int n, int n_act) {
  return act_bytes(n) + (n_act > 0 ? (size_t)plan_active(n, n_act).slabs * 6 * n_act * sizeof(float) : 0);
}

// the largest slabs x n_act any active set of n sources can need
size_t slab_floats(int n) {
  size_t most = 0;
  const int g_all = ceil_div(n, kTgtPerWG);
  for (int g = 1; g <= g_all; ++g) {
    const int n_act = g == g_all ? n : g * kTgtPerWG;
    size_t rows = (size_t)plan_active(n, n_act).slabs * n_act;
    if (g == g_all && n_act > 1) {                      // a ragged last group below n uses the n_act < n plan
      const size_t r2 = (size_t)plan_active(n, n_act - 1).slabs * (n_act - 1);
      if (r2 > rows) rows = r2;
    }
    if (rows > most) most = rows;
  }
  return most * 6;
}

int launch_active(const float* posm, const float* velp, int n, const int* act, int n_act, float eps2, float* slabs,
                  const JerkPlan& p, hipStream_t st) {
  dim3 grid(p.groups, p.slabs), block(64 * kWaves);
  const ChunkSplit c = chunk_split(p.n_chunks, p.slabs);
  const f4* pm = reinterpret_cast<const f4*>(posm);
  const f4* vp = reinterpret_cast<const f4*>(velp);
  if (eps2 < kEps2Masked)
    accel_jerk_active_kernel<true><<<grid, block, 0, st>>>(pm, vp, n, act, n_act, c.q, c.r, eps2, slabs);
  else
    accel_jerk_active_kernel<false><<<grid, block, 0, st>>>(pm, vp, n, act, n_act, c.q, c.r, eps2, slabs);
  return launch_status();
}

int* ws_act(void* ws) { return static_cast<int*>(ws); }
float* ws_slabs(void* ws, int n) { return reinterpret_cast<float*>(static_cast<char*>(ws) + act_bytes(n)); }

}  // namespace

extern "C" {

size_t nbd_hblock_workspace_bytes(int n) {
  if (n <= 0) return 0;
  return act_bytes(n) + slab_floats(n) * sizeof(float);
}

int nbd_hblock_init_levels(const float* acc, const float* jerk, int n, double dt, double eta, int max_level, int* ticks,
                           int* levels, int* sched, nbd_stream_t stream) {
  if (n < 0 || bad_level(max_level) || !(dt > 0.0) || !(eta > 0.0)) return NBD_E_BADARG;
  if (!sched) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (!acc || !jerk || !ticks || !levels) return NBD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  // T, the cursor and the histogram start from zero; t_next, n_act and the clamp count are left as they are
  hipError_t e = hipMemsetAsync(sched + kTCur, 0, (NBD_HBLOCK_SCHED_INTS - kTCur) * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  hblock_init_kernel<<<ceil_div(n, 256), 256, 0, st>>>(acc, jerk, n, max_level, dt, eta, ticks, levels, sched);
  return launch_status();
}

int nbd_hblock_schedule(const int* levels, int n, int max_level, int* sched, void* workspace, size_t workspace_bytes,
                        int* host_sched, nbd_stream_t stream) {
  if (n <= 0 || bad_level(max_level) || !levels || !sched) return NBD_E_BADARG;
  if (!workspace || misaligned16(workspace) || workspace_bytes < act_bytes(n)) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  hblock_schedule_kernel<<<ceil_div(n, 256), 256, 0, st>>>(levels, n, max_level, sched, ws_act(workspace));
  int rc = launch_status();
  if (rc || !host_sched) return rc;
  hipError_t e = hipMemcpyAsync(host_sched, sched, 4 * sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e == hipSuccess ? 0 : (int)e;
}

int nbd_hblock_predict_f32(const float* pos, const float* vel, const float* acc, const float* jerk, const float* mass,
                           const int* ticks, int n, int max_level, double dt, int* sched, float* posm, float* velp,
                           nbd_stream_t stream) {
  if (n <= 0 || bad_level(max_level) || !(dt > 0.0)) return NBD_E_BADARG;
  if (!pos || !vel || !acc || !jerk || !mass || !ticks || !sched || !posm || !velp) return NBD_E_BADARG;
  if (misaligned16(posm) || misaligned16(velp)) return NBD_E_BADARG;
  const int n_pad = nbd_posm_padded_len(n);
  hblock_predict_kernel<<<ceil_div(n_pad, 256), 256, 0, (hipStream_t)stream>>>(
      pos, vel, acc, jerk, mass, ticks, n, n_pad, dt, ldexp(1.0, -max_level), sched, reinterpret_cast<f4*>(posm),
      reinterpret_cast<f4*>(velp));
  return launch_status();
}

int nbd_hblock_force_f32(const float* posm, const float* velp, int n, int n_act, float softening_sq, void* workspace,
                         size_t workspace_bytes, nbd_stream_t stream) {
  if (n <= 0 || n_act < 0 || n_act > n || !posm || !velp || misaligned16(posm) || misaligned16(velp))
    return NBD_E_BADARG;
  if (!workspace || misaligned16(workspace) || workspace_bytes < step_bytes(n, n_act)) return NBD_E_WORKSPACE;
  if (n_act == 0) return 0;
  return launch_active(posm, velp, n, ws_act(workspace), n_act, softening_sq, ws_slabs(workspace, n),
                       plan_active(n, n_act), (hipStream_t)stream);
}

int nbd_hblock_correct_f32(float* pos, float* vel, float* acc, float* jerk, const float* mass, int* ticks, int* levels,
                           int n, int n_act, int max_level, double dt, double eta, float g_const, int* sched, float* posm,
                           void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  if (n <= 0 || n_act < 0 || n_act > n || bad_level(max_level) || !(dt > 0.0) || !(eta > 0.0)) return NBD_E_BADARG;
  if (!pos || !vel || !acc || !jerk || !mass || !ticks || !levels || !sched || !posm || misaligned16(posm))
    return NBD_E_BADARG;
  if (!workspace || misaligned16(workspace) || workspace_bytes < step_bytes(n, n_act)) return NBD_E_WORKSPACE;
  if (n_act == 0) return 0;
  const JerkPlan p = plan_active(n, n_act);
  hblock_correct_kernel<<<ceil_div(n_act, 64), 256, 0, (hipStream_t)stream>>>(
      ws_slabs(workspace, n), p.slabs, ws_act(workspace), n_act, g_const, max_level, dt, ldexp(1.0, -max_level), eta,
      pos, vel, acc, jerk, mass, ticks, levels, sched, reinterpret_cast<f4*>(posm));
  return launch_status();
}

int nbd_hblock_step_f32(float* pos, float* vel, float* acc, float* jerk, const float* mass, int* ticks, int* levels,
                        int n, int n_act, int max_level, double dt, double eta, float softening_sq, float g_const,
                        int* sched, float* posm, float* velp, void* workspace, size_t workspace_bytes,
                        nbd_stream_t stream) {
  if (n <= 0 || n_act < 1 || n_act > n || bad_level(max_level) || !(dt > 0.0) || !(eta > 0.0)) return NBD_E_BADARG;
  if (!velp || misaligned16(velp)) return NBD_E_BADARG;
  int rc = nbd_hblock_predict_f32(pos, vel, acc, jerk, mass, ticks, n, max_level, dt, sched, posm, velp, stream);
  if (rc) return rc;
  rc = nbd_hblock_force_f32(posm, velp, n, n_act, softening_sq, workspace, workspace_bytes, stream);
  if (rc) return rc;
  return nbd_hblock_correct_f32(pos, vel, acc, jerk, mass, ticks, levels, n, n_act, max_level, dt, eta, g_const, sched,
                                posm, workspace, workspace_bytes, stream);
}

int nbd_accel_jerk_active_f32(const float* posm, const float* velp, int n, const int* act, int n_act,
                              float softening_sq, float g_const, float* acc_out, float* jerk_out, void* workspace,
                              size_t workspace_bytes, nbd_stream_t stream) {
  if (n < 0 || n_act < 0 || n_act > n) return NBD_E_BADARG;
  if (n_act == 0) return 0;
  if (!posm || !velp || !act || !acc_out || !jerk_out || misaligned16(posm) || misaligned16(velp)) return NBD_E_BADARG;
  if (!workspace || misaligned16(workspace) || workspace_bytes < step_bytes(n, n_act)) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const JerkPlan p = plan_active(n, n_act);
  float* slabs = ws_slabs(workspace, n);
  int rc = launch_active(posm, velp, n, act, n_act, softening_sq, slabs, p, st);
  if (rc) return rc;
  hblock_correct_kernel<<<ceil_div(n_act, 64), 256, 0, st>>>(slabs, p.slabs, act, n_act, g_const, 0, 1.0, 1.0, 1.0,
                                                             nullptr, nullptr, acc_out, jerk_out, nullptr, nullptr,
                                                             nullptr, nullptr, nullptr);
  return launch_status();
}

}  // extern "C"
