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
// The schedule record's layout, the level arithmetic (criterion, wanted_level, norm3, hblock_relevel) and the O(N)
// kernels (hblock_init_kernel<T>, hblock_predict_kernel<T>, hblock_correct_kernel<T>, here at T = float) live in
// hermite_block_kernels.h, shared with the float64 form of this unit, direct_hermite_block_f64.hip; hblock_schedule_kernel
// serves both.
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
constexpr int kSumRows = HermiteFmt<float>::kSumRows;      // list entries per workgroup of the corrector launch

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
  return hblock_init_levels(acc, jerk, n, dt, eta, max_level, ticks, levels, sched, (hipStream_t)stream);
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
  hblock_predict_kernel<float><<<ceil_div(n_pad, 256), 256, 0, (hipStream_t)stream>>>(
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
  hblock_correct_kernel<float><<<ceil_div(n_act, kSumRows), 256, 0, (hipStream_t)stream>>>(
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
  hblock_correct_kernel<float><<<ceil_div(n_act, kSumRows), 256, 0, st>>>(
      slabs, p.slabs, act, n_act, g_const, 0, 1.0, 1.0, 1.0, nullptr, nullptr, acc_out, jerk_out, nullptr, nullptr,
      nullptr, nullptr, nullptr);
  return launch_status();
}

}  // extern "C"
