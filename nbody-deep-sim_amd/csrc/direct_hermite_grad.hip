// direct_hermite_grad.hip -- the backward of the Hermite force for gfx950 (MI355X): the vector-Jacobian product of
//   a_i = G sum_{j != i} m_j s^3 d,   j_i = G sum_{j != i} m_j [ s^3 w - 3 s^5 (d . w) d ],
//   d = x_j - x_i,   w = v_j - v_i,   s = (|d|^2 + eps^2)^(-1/2)
// with the cotangents alpha = dL/da and beta = dL/dj (n, 3 each), with respect to positions, velocities and masses. With
// h = m_i beta_j - m_j beta_i (and h^alpha likewise from alpha):
//   dL/dv_i =  G sum_j [ s^3 h - 3 s^5 d (d . h) ]
//   dL/dx_i =  G sum_j [ s^3 h^alpha - 3 s^5 d (d . h^alpha) ]
//            + G sum_j { -3 s^5 [ (h . w) d + (d . h) w + (d . w) h ] + 15 s^7 (d . w)(d . h) d }
//   dL/dm_i = -G sum_j   s^3 (d . alpha_j)
//            - G sum_j [ s^3 (beta_j . w) - 3 s^5 (d . w)(d . beta_j) ]
// An extension: the reference has no Hermite integrator. C-ABI: the nbd_accel_jerk_vjp_* entries of include/nbd.h; Python:
// nbd.autograd.direct_accel_jerk and HermiteSimulator.compute_accelerations_and_jerks() under autograd.
//
// The alpha lines are the backward of the acceleration: when alpha is given, the host side of an entry calls
// nbd_accel_vjp_f32 / nbd_accel_vjp_f64 (direct_grad.hip), whose kernels stay the only copy of that arithmetic. This file
// holds the beta lines, one walk for all of them (dL/dv is the position-gradient arithmetic of direct_grad.hip with
// cot = beta; the walk already holds d, h and the powers of s, so it costs six more FMAs per source, not a launch):
//   fp32: accel_jerk_body (hermite_kernels.h) with THREE streamed rows per source, {x, m}, {v, 0}, {beta, 0}, and the pair
//         policy AccelJerkVjpPolicy: two targets per lane, 128 per workgroup, plan_jerk(n, n); float[slabs][7][n] partial
//         sums {dL/dx (3), dL/dv (3), dL/dm}, then accel_jerk_vjp_finish_kernel (hermite_slab_sum's 4-wave order, G once,
//         beta part + alpha part).
//   fp64: walk_f64 (hermite_f64_kernels.h) with the pair functor AccelJerkVjpPair (kStreams = 3), plan_f64(n);
//         double[slabs][7][n], then accel_jerk_vjp_finish_f64_kernel (slab_order_sum).
// No atomics, no memsets, no host syncs: deterministic run to run with a workspace that may hold anything, and capturable.
// An output that is not wanted is a null pointer and is not written.
//
// The i == j term, as in direct_grad.hip: every new beta term carries a factor d or w, exact zeros at i == j, but s^3 h of
// dL/dv does not -- fma(m_i, beta_i, -round(m_i beta_i)) survives and eps^-3 multiplies it. So the chunks that hold a
// workgroup's own indices (two in fp32, one in fp64) take the index-masked pair whatever the softening, and below
// eps^2 = 1e-24 every chunk does: the closed form over j != i. A padding row (m = 0, v = 0, beta = 0) gives h = 0,
// beta_j . w = 0 and d . beta_j = 0 with a finite s: every term it adds is an exact zero.
//
// The un-masked fp32 loop, per source and pair of targets, counted on the gfx950 assembly: 6 v_pk_add (d, w), 36 v_pk_fma
// (3 r^2, 3 h, 10 in the five dot products d.h, d.w, h.w, d.beta_j, beta_j.w, 2 in the Newton step on s, 1 in
// e = h.w - 5 s^2 d.w d.h, 6 in the bracket of dL/dx, 11 sums), 20 v_pk_mul (3 h, 5 dot products, 2 in the Newton step,
// s^2, s^3, s^5, s^5 d.h, s^5 d.w, 2 for e, 3 in the bracket), 2 v_rsq_f32: 62 packed ops against 26 for the force and
// 29 for the acceleration's backward, 71.5 instructions with 3 ds_read_b128 and 2.5 other VALU. Registers: 200 VGPRs for
// the un-masked kernel (both pair loops live in one kernel; 2 waves per SIMD), 122 for the masked one, 150 for fp64, no
// scratch in any (reported, not capped: DESIGN.md, "K-HVJP").
// Two accumulator sets per lane, one for the even and one for the odd sources, as AccelVjpPolicy has and for its reason:
// the error of these gradients is the error of the fp32 chains, the acceleration's backward missed four times torch's
// fp32 figures in a row of its n = 65 test with one chain per wave, and dL/dv here IS that arithmetic. The second set
// costs 11 registers per target pair and no instruction in the loop; it was taken over, not measured against one set.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_kernels.h"
#include "hermite_f64_kernels.h"
#include "hermite_kernels.h"

namespace {

constexpr int kHvjpOut = 7;      // dL/dx (3), dL/dv (3), dL/dm

// ---- fp32: the pair policy of accel_jerk_body with NS = 3 (what a policy is: AccelJerkPolicy, hermite_kernels.h)
// One set of sums: V1[0..2] s^3 h, V2[3..5] (s^5 d.h) d, X[6..8] s^5 (e d + (d.h) w + (d.w) h) with
// e = h.w - 5 s^2 d.w d.h, M1[9] s^3 beta_j.w, M2[10] (s^5 d.w) d.beta_j.
// out = {-3 X, V1 - 3 V2, M1 - 3 M2}; the finishing kernel multiplies by G (and by -1 for the mass).
struct AccelJerkVjpPolicy {
  static constexpr int kSet = 11, kAcc = 2 * kSet, kOut = kHvjpOut;
  f2 xi, yi, zi, mi, ui, vi, wi, bxi, byi, bzi;

  // t: the targets' {x, m} rows, u: their {v, 0} rows, b: their {beta, 0} rows
  __device__ __forceinline__ AccelJerkVjpPolicy(const f4 t0, const f4 t1, const f4 u0, const f4 u1, const f4 b0,
                                                const f4 b1)
      : xi{t0.x, t1.x}, yi{t0.y, t1.y}, zi{t0.z, t1.z}, mi{t0.w, t1.w}, ui{u0.x, u1.x}, vi{u0.y, u1.y},
        wi{u0.z, u1.z}, bxi{b0.x, b1.x}, byi{b0.y, b1.y}, bzi{b0.z, b1.z} {}

  __device__ __forceinline__ bool own(int pc, int i0) const {
    return (pc >> 1) == __builtin_amdgcn_readfirstlane(i0 >> 7);
  }

  // h = m_i beta_j - m_j beta_i for one component, one product and one fma (AccelVjpPolicy::h_of, OWN)
  __device__ __forceinline__ f2 h_of(const f2 bj, const f2 mj, const f2 bi) const {
    return __builtin_elementwise_fma(mi, bj, -(mj * bi));
  }

  static __device__ __forceinline__ f2 dot(const f2 ax, const f2 ay, const f2 az, const f2 bx, const f2 by, const f2 bz) {
    f2 t = ax * bx;
    t = __builtin_elementwise_fma(ay, by, t);
    return __builtin_elementwise_fma(az, bz, t);
  }

  // everything of one source that does not need s
  struct Pre { f2 dx, dy, dz, wx, wy, wz, hx, hy, hz, dh, dw, hw, db, bw, r2; };

  __device__ __forceinline__ Pre pre(const f4 p, const f4 q, const f4 r, const f2 e2) const {
    Pre t;
    t.dx = f2{p.x, p.x} - xi; t.dy = f2{p.y, p.y} - yi; t.dz = f2{p.z, p.z} - zi;
    t.wx = f2{q.x, q.x} - ui; t.wy = f2{q.y, q.y} - vi; t.wz = f2{q.z, q.z} - wi;
    f2 r2 = __builtin_elementwise_fma(t.dx, t.dx, e2);
    r2 = __builtin_elementwise_fma(t.dy, t.dy, r2);
    t.r2 = __builtin_elementwise_fma(t.dz, t.dz, r2);
    const f2 bx = {r.x, r.x}, by = {r.y, r.y}, bz = {r.z, r.z}, mj = {p.w, p.w};
    t.hx = h_of(bx, mj, bxi); t.hy = h_of(by, mj, byi); t.hz = h_of(bz, mj, bzi);
    t.dh = dot(t.dx, t.dy, t.dz, t.hx, t.hy, t.hz);
    t.dw = dot(t.dx, t.dy, t.dz, t.wx, t.wy, t.wz);
    t.hw = dot(t.hx, t.hy, t.hz, t.wx, t.wy, t.wz);
    t.db = dot(t.dx, t.dy, t.dz, bx, by, bz);
    t.bw = dot(bx, by, bz, t.wx, t.wy, t.wz);
    return t;
  }

  // the sums of one source, from what pre() left and s0 = v_rsq_f32 of r^2 (masked or not).
  // One Newton step first, s = s0 + (s0 / 2)(1 - r^2 s0^2) with the residual by one fma: s^5 multiplies the relative
  // error of s by 5, which with the 1-ulp v_rsq_f32 is by itself the room a pair that carries the norm has under four
  // times torch's fp32 figure. A masked s0 = 0 stays 0.
  // The beta part of dL/dx is s^5 TIMES the bracket T = (h.w - 5 s^2 d.w d.h) d + (d.h) w + (d.w) h: the terms of the
  // bracket cancel (to a quarter where d, w and h are parallel), and formed this way only the error of s^2 is amplified by
  // that, not the errors of s^5 and s^7. With s^5 and s^7 carried into the terms (e = s^5 h.w - 5 s^7 d.w d.h, then
  // e d + s^5 d.h w + s^5 d.w h) dL/dx sat at 1.10 of the bar at n = 65, where one pair carries the norm (NOTES "K-HVJP").
  __device__ __forceinline__ void add(f2* acc, const Pre& t, const f2 s0) const {
    const f2 res = __builtin_elementwise_fma(-(t.r2 * s0), s0, f2{1.0f, 1.0f});
    const f2 s = __builtin_elementwise_fma(0.5f * s0, res, s0);
    const f2 s2 = s * s;
    const f2 s3 = s2 * s;
    const f2 s5 = s3 * s2;
    const f2 cdh = s5 * t.dh;
    const f2 cdw = s5 * t.dw;
    const f2 e = __builtin_elementwise_fma(-5.0f * (s2 * t.dw), t.dh, t.hw);
    acc[0] = __builtin_elementwise_fma(s3, t.hx, acc[0]);
    acc[1] = __builtin_elementwise_fma(s3, t.hy, acc[1]);
    acc[2] = __builtin_elementwise_fma(s3, t.hz, acc[2]);
    acc[3] = __builtin_elementwise_fma(cdh, t.dx, acc[3]);
    acc[4] = __builtin_elementwise_fma(cdh, t.dy, acc[4]);
    acc[5] = __builtin_elementwise_fma(cdh, t.dz, acc[5]);
    f2 x = __builtin_elementwise_fma(t.dh, t.wx, t.dw * t.hx);
    acc[6] = __builtin_elementwise_fma(s5, __builtin_elementwise_fma(e, t.dx, x), acc[6]);
    x = __builtin_elementwise_fma(t.dh, t.wy, t.dw * t.hy);
    acc[7] = __builtin_elementwise_fma(s5, __builtin_elementwise_fma(e, t.dy, x), acc[7]);
    x = __builtin_elementwise_fma(t.dh, t.wz, t.dw * t.hz);
    acc[8] = __builtin_elementwise_fma(s5, __builtin_elementwise_fma(e, t.dz, x), acc[8]);
    acc[9] = __builtin_elementwise_fma(s3, t.bw, acc[9]);
    acc[10] = __builtin_elementwise_fma(cdw, t.db, acc[10]);
  }

  // One source against the lane's two targets, index-masked: only j == i and the padding behind n are dropped, by a
  // select on s.
  __device__ __forceinline__ void masked(const f4 p, const f4 q, const f4 r, const f2 e2, f2* acc, int j, int i0, int i1,
                                         int n) const {
    const Pre t = pre(p, q, r, e2);
    f2 s = {__builtin_amdgcn_rsqf(t.r2.x), __builtin_amdgcn_rsqf(t.r2.y)};
    s.x = (j < n && j != i0) ? s.x : 0.0f;
    s.y = (j < n && j != i1) ? s.y : 0.0f;
    if (j & 1) add(acc + kSet, t, s);      // j is uniform: a branch, never an indexed register
    else add(acc, t, s);
  }

  // KU sources at once, un-masked: jerk_block's shape (the 2 KU v_rsq_f32 issued back to back; every consumer of an
  // rsq result is plain C++, so hipcc pads the transcendental hazard itself).
  template <int KU>
  __device__ __forceinline__ void block(const f4* __restrict__ bp, const f4* __restrict__ bv, const f4* __restrict__ bb,
                                        const f2 e2, f2* acc) const {
    static_assert(KU % 2 == 0, "the two accumulator sets alternate inside a block");
    Pre t[KU];
    f2 s[KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) t[u] = pre(bp[u], bv[u], bb[u], e2);
#pragma unroll
    for (int u = 0; u < KU; ++u) s[u] = f2{__builtin_amdgcn_rsqf(t[u].r2.x), __builtin_amdgcn_rsqf(t[u].r2.y)};
    __builtin_amdgcn_sched_group_barrier(0x400, 2 * KU, 0);      // 0x400 = TRANS: keep the rsq's together
#pragma unroll
    for (int u = 0; u < KU; ++u) add(acc + (u & 1) * kSet, t[u], s[u]);      // a block starts at an even source
  }

  __device__ __forceinline__ f2 out(const f2* acc, int k) const {
    if (k < 3) return -3.0f * (acc[6 + k] + acc[kSet + 6 + k]);
    if (k < 6) return (acc[k - 3] + acc[kSet + k - 3]) - 3.0f * (acc[k] + acc[kSet + k]);
    return (acc[9] + acc[kSet + 9]) - 3.0f * (acc[10] + acc[kSet + 10]);
  }
};

constexpr int kHvjpKU = 2;

// The partial sums of all n bodies under all n bodies: accel_vjp_kernel's geometry (direct_grad.hip), grid = (target
// groups of 128, slabs), the chunks spread over all slabs x 4 waves to within one. out: float[slab][7][n].
template <bool MASKED>
__global__ __launch_bounds__(64 * kWaves) void accel_jerk_vjp_kernel(const f4* __restrict__ posm,
                                                                     const f4* __restrict__ velp,
                                                                     const f4* __restrict__ cotj, int n, int cpw_q,
                                                                     int cpw_r, float eps2, float* __restrict__ out) {
  __shared__ f4 lds[kWaves * 6 * kChunk];
  const int t_base = blockIdx.x * kTgtPerWG;
  const int i0 = t_base + (threadIdx.x & 63), i1 = i0 + 64;
  const int jw = blockIdx.y * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int c_begin, c_end;
  wave_chunk_range(jw, cpw_q, cpw_r, c_begin, c_end);
  accel_jerk_body<MASKED, kHvjpKU, 1, false, AccelJerkVjpPolicy, 3>(
      posm, velp, n, posm, velp, min(i0, n - 1), min(i1, n - 1), i0, i1, c_begin, c_end, eps2, lds,
      out + (size_t)blockIdx.y * kHvjpOut * n + t_base, n, min(kTgtPerWG, n - t_base), nullptr, cotj, cotj);
}

// One workgroup per 64 consecutive bodies: the slabs of float[n_slabs][7][n] in hermite_slab_sum's order (wave w sums
// slabs w, w + 4, ... of its lane's row, the four partials combined as (p0 + p1) + (p2 + p3)), then G, once, then the
// alpha part (a_pos (n, 3), a_mass (n,): what nbd_accel_vjp_f32 left, G applied; null: none) added last:
// grad_pos = g sum + a_pos, grad_vel = g sum, grad_mass = (0 - g sum) + a_mass. n_slabs = 0: zeros (no beta).
__global__ __launch_bounds__(256) void accel_jerk_vjp_finish_kernel(const float* __restrict__ slabs, int n_slabs, int n,
                                                                    float g, const float* __restrict__ a_pos,
                                                                    const float* __restrict__ a_mass,
                                                                    float* __restrict__ grad_pos,
                                                                    float* __restrict__ grad_vel,
                                                                    float* __restrict__ grad_mass) {
  __shared__ float part[4][kHvjpOut][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  float sum[kHvjpOut];
#pragma unroll
  for (int k = 0; k < kHvjpOut; ++k) sum[k] = 0.f;
  if (i < n)
    for (int s = w; s < n_slabs; s += 4)
#pragma unroll
      for (int k = 0; k < kHvjpOut; ++k) sum[k] += slabs[((size_t)s * kHvjpOut + k) * n + i];
#pragma unroll
  for (int k = 0; k < kHvjpOut; ++k) part[w][k][lane] = sum[k];
  __syncthreads();
  if (w != 0 || i >= n) return;
  auto total = [&](int k) {
    const float t = (part[0][k][lane] + part[1][k][lane]) + (part[2][k][lane] + part[3][k][lane]);
    return n_slabs ? g * t : 0.0f;
  };
  if (grad_pos) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float b = total(k);
      grad_pos[3 * (size_t)i + k] = a_pos ? b + a_pos[3 * (size_t)i + k] : b;
    }
  }
  if (grad_vel) {
#pragma unroll
    for (int k = 0; k < 3; ++k) grad_vel[3 * (size_t)i + k] = total(3 + k);
  }
  if (grad_mass) {
    const float b = 0.0f - total(6);
    grad_mass[i] = a_mass ? b + a_mass[i] : b;
  }
}

// ---- fp64: the pair functor of walk_f64 with three streamed arrays (what a functor is: hermite_f64_kernels.h).
// p = {x, y, z, m}, q = {vx, vy, vz, 0}, r = {beta_x, beta_y, beta_z, 0} of source j: AccelJerkVjpPolicy's operations one
// for one, one target per lane, one set of sums. walk_f64 walks the chunk of the group's own rows MASKED whatever the
// softening, so i == j never reaches the un-masked pair.
struct AccelJerkVjpPair {
  static constexpr int kStreams = 3;
  static constexpr int kOut = kHvjpOut;
  double xi, yi, zi, mi, ui, vi, wi, bxi, byi, bzi, e2;
  double acc[11];
  int i, n;

  __device__ __forceinline__ AccelJerkVjpPair(const d4 tp, const d4 tv, const d4 tb, double eps2, int i_, int n_)
      : xi(tp.x), yi(tp.y), zi(tp.z), mi(tp.w), ui(tv.x), vi(tv.y), wi(tv.z), bxi(tb.x), byi(tb.y), bzi(tb.z),
        e2(eps2), i(i_), n(n_) {
#pragma unroll
    for (int k = 0; k < 11; ++k) acc[k] = 0.0;
  }

  static __device__ __forceinline__ double dot(double ax, double ay, double az, double bx, double by, double bz) {
    double t = ax * bx;
    t = __builtin_fma(ay, by, t);
    return __builtin_fma(az, bz, t);
  }

  template <bool MASKED>
  __device__ __forceinline__ void pair(const d4 p, const d4 q, const d4 r, int j) {
    const double dx = p.x - xi, dy = p.y - yi, dz = p.z - zi;      // x_j - x_i
    const double wx = q.x - ui, wy = q.y - vi, wz = q.z - wi;      // v_j - v_i
    double r2 = __builtin_fma(dx, dx, e2);
    r2 = __builtin_fma(dy, dy, r2);
    r2 = __builtin_fma(dz, dz, r2);
    const double hx = __builtin_fma(mi, r.x, -(p.w * bxi));
    const double hy = __builtin_fma(mi, r.y, -(p.w * byi));
    const double hz = __builtin_fma(mi, r.z, -(p.w * bzi));
    const double dh = dot(dx, dy, dz, hx, hy, hz);
    const double dw = dot(dx, dy, dz, wx, wy, wz);
    const double hw = dot(hx, hy, hz, wx, wy, wz);
    const double db = dot(dx, dy, dz, r.x, r.y, r.z);
    const double bw = dot(r.x, r.y, r.z, wx, wy, wz);
    double s = rsqrt_f64(r2);
    if (MASKED) s = (j < n && j != i) ? s : 0.0;
    const double s2 = s * s;
    const double s3 = s2 * s;
    const double s5 = s3 * s2;
    const double cdh = s5 * dh;
    const double cdw = s5 * dw;
    const double e = __builtin_fma(-5.0 * (s2 * dw), dh, hw);
    acc[0] = __builtin_fma(s3, hx, acc[0]);
    acc[1] = __builtin_fma(s3, hy, acc[1]);
    acc[2] = __builtin_fma(s3, hz, acc[2]);
    acc[3] = __builtin_fma(cdh, dx, acc[3]);
    acc[4] = __builtin_fma(cdh, dy, acc[4]);
    acc[5] = __builtin_fma(cdh, dz, acc[5]);
    acc[6] = __builtin_fma(s5, __builtin_fma(e, dx, __builtin_fma(dh, wx, dw * hx)), acc[6]);
    acc[7] = __builtin_fma(s5, __builtin_fma(e, dy, __builtin_fma(dh, wy, dw * hy)), acc[7]);
    acc[8] = __builtin_fma(s5, __builtin_fma(e, dz, __builtin_fma(dh, wz, dw * hz)), acc[8]);
    acc[9] = __builtin_fma(s3, bw, acc[9]);
    acc[10] = __builtin_fma(cdw, db, acc[10]);
  }

  __device__ __forceinline__ double out(int k) const {
    if (k < 3) return -3.0 * acc[6 + k];
    if (k < 6) return acc[k - 3] - 3.0 * acc[k];
    return acc[9] - 3.0 * acc[10];
  }
};

// accel_vjp_f64_kernel's geometry (direct_grad.hip): grid = (groups of 64 targets, slabs). out: double[slab][7][n].
__global__ __launch_bounds__(64 * kWaves) void accel_jerk_vjp_f64_kernel(const d4* __restrict__ posd,
                                                                         const d4* __restrict__ veld,
                                                                         const d4* __restrict__ cotj, int n, int cpw_q,
                                                                         int cpw_r, double eps2, int all_masked,
                                                                         double* __restrict__ out) {
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads_n<3>()];
  const Group64<unsigned> g(blockIdx.x, blockIdx.y, n);
  const ChunkRange c = wave_chunks(g.jw(), cpw_q, cpw_r);
  AccelJerkVjpPair pr(posd[g.row()], veld[g.row()], cotj[g.row()], eps2, g.i, n);
  walk_f64(pr, posd, veld, c.begin, c.end, all_masked != 0, blockIdx.x, lds, g.dst<AccelJerkVjpPair>(out), (size_t)n,
           g.n_valid(), nullptr, cotj);
}

// One thread per body: the slabs of double[n_slabs][7][n] in slab order (slab_order_sum, hermite_kernels.h), then G, once,
// then the alpha part added last (accel_jerk_vjp_finish_kernel's statement). n_slabs = 0: zeros.
__global__ __launch_bounds__(256) void accel_jerk_vjp_finish_f64_kernel(const double* __restrict__ slabs, int n_slabs,
                                                                        int n, double g,
                                                                        const double* __restrict__ a_pos,
                                                                        const double* __restrict__ a_mass,
                                                                        double* __restrict__ grad_pos,
                                                                        double* __restrict__ grad_vel,
                                                                        double* __restrict__ grad_mass) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double sum[kHvjpOut];
  slab_order_sum<kHvjpOut>(slabs, n_slabs, (size_t)n, (size_t)i, sum);
  auto total = [&](int k) { return n_slabs ? g * sum[k] : 0.0; };
  if (grad_pos) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double b = total(k);
      grad_pos[3 * (size_t)i + k] = a_pos ? b + a_pos[3 * (size_t)i + k] : b;
    }
  }
  if (grad_vel) {
#pragma unroll
    for (int k = 0; k < 3; ++k) grad_vel[3 * (size_t)i + k] = total(3 + k);
  }
  if (grad_mass) {
    const double b = 0.0 - total(6);
    grad_mass[i] = a_mass ? b + a_mass[i] : b;
  }
}

// The workspace of an entry, in elements of its scalar type: [beta slabs: slabs x 7 x n, rounded up to a multiple of 4 so
// that what follows keeps the alignment the alpha entry asks for][the alpha entry's own workspace: slabs x 4 x n]
// [alpha's grad_pos: 3 n][alpha's grad_mass: n].
struct Layout { size_t alpha_ws, alpha_pos, alpha_mass, total; };

inline Layout layout(int n, int slabs) {
  Layout l;
  l.alpha_ws = ((size_t)slabs * kHvjpOut * n + 3) & ~(size_t)3;
  l.alpha_pos = l.alpha_ws + (size_t)slabs * 4 * n;
  l.alpha_mass = l.alpha_pos + 3 * (size_t)n;
  l.total = l.alpha_mass + (size_t)n;
  return l;
}

}  // namespace

extern "C" {

size_t nbd_accel_jerk_vjp_workspace_bytes(int n) {
  if (n <= 0) return 0;
  return layout(n, plan_jerk(n, n).slabs).total * sizeof(float);
}

int nbd_accel_jerk_vjp_f32(const float* posm, const float* velp, const float* cota, const float* cotj, int n,
                           float softening_sq, float g_const, float* grad_pos, float* grad_vel, float* grad_mass,
                           void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  if (n < 0 || !isfinite(softening_sq) || !isfinite(g_const)) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (!posm || !velp || misaligned16(posm) || misaligned16(velp) || misaligned16(cota) || misaligned16(cotj))
    return NBD_E_BADARG;
  if ((!cota && !cotj) || (!grad_pos && !grad_vel && !grad_mass)) return NBD_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(grad_pos) | reinterpret_cast<uintptr_t>(grad_vel) |
       reinterpret_cast<uintptr_t>(grad_mass)) & 3)
    return NBD_E_BADARG;
  const JerkPlan p = plan_jerk(n, n);
  const Layout l = layout(n, p.slabs);
  if (!workspace || misaligned16(workspace) || workspace_bytes < l.total * sizeof(float)) return NBD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  const bool alpha = cota && (grad_pos || grad_mass);
  float* a_pos = alpha && cotj && grad_pos ? ws + l.alpha_pos : nullptr;      // with beta: alpha goes through the workspace
  float* a_mass = alpha && cotj && grad_mass ? ws + l.alpha_mass : nullptr;
  if (alpha) {
    const int rc = nbd_accel_vjp_f32(posm, cota, n, softening_sq, g_const, cotj ? a_pos : grad_pos,
                                     cotj ? a_mass : grad_mass, ws + l.alpha_ws, stream);
    if (rc) return rc;
  }
  const dim3 fgrid(ceil_div(n, 64)), fblock(256);
  if (!cotj) {      // no beta: alpha's bits are in place (or zeros where there is no alpha either), dL/dv = 0
    float* zp = alpha ? nullptr : grad_pos;
    float* zm = alpha ? nullptr : grad_mass;
    if (!zp && !zm && !grad_vel) return 0;
    accel_jerk_vjp_finish_kernel<<<fgrid, fblock, 0, st>>>(ws, 0, n, g_const, nullptr, nullptr, zp, grad_vel, zm);
    return launch_status();
  }
  const ChunkSplit c = chunk_split(p.n_chunks, p.slabs);
  const dim3 grid(p.groups, p.slabs), block(64 * kWaves);
  const f4* pm = reinterpret_cast<const f4*>(posm);
  const f4* vp = reinterpret_cast<const f4*>(velp);
  const f4* cj = reinterpret_cast<const f4*>(cotj);
  if (softening_sq < kEps2Masked) accel_jerk_vjp_kernel<true><<<grid, block, 0, st>>>(pm, vp, cj, n, c.q, c.r, softening_sq, ws);
  else accel_jerk_vjp_kernel<false><<<grid, block, 0, st>>>(pm, vp, cj, n, c.q, c.r, softening_sq, ws);
  const int rc = launch_status();
  if (rc) return rc;
  accel_jerk_vjp_finish_kernel<<<fgrid, fblock, 0, st>>>(ws, p.slabs, n, g_const, a_pos, a_mass, grad_pos, grad_vel,
                                                         grad_mass);
  return launch_status();
}

size_t nbd_accel_jerk_vjp_f64_workspace_bytes(int n, int slabs) {
  if (n <= 0 || slabs < 0 || slabs > kMaxSlabs) return 0;
  if (slabs == 0) slabs = plan_f64(n).slabs;
  return layout(n, slabs).total * sizeof(double);
}

int nbd_accel_jerk_vjp_f64(const double* posd, const double* veld, const double* cota, const double* cotj, int n,
                           double softening_sq, double g_const, double* grad_pos, double* grad_vel, double* grad_mass,
                           void* workspace, size_t workspace_bytes, int slabs, nbd_stream_t stream) {
  if (n < 0 || slabs < 0 || slabs > kMaxSlabs || !isfinite(softening_sq) || !isfinite(g_const)) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (!posd || !veld || misaligned32(posd) || misaligned32(veld) || misaligned32(cota) || misaligned32(cotj))
    return NBD_E_BADARG;
  if ((!cota && !cotj) || (!grad_pos && !grad_vel && !grad_mass)) return NBD_E_BADARG;
  if (misaligned8(grad_pos) || misaligned8(grad_vel) || misaligned8(grad_mass)) return NBD_E_BADARG;
  const F64Plan p = plan_f64(n);
  if (slabs == 0) slabs = p.slabs;
  const Layout l = layout(n, slabs);
  if (!workspace || misaligned8(workspace) || workspace_bytes < l.total * sizeof(double)) return NBD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  double* ws = static_cast<double*>(workspace);
  const bool alpha = cota && (grad_pos || grad_mass);
  double* a_pos = alpha && cotj && grad_pos ? ws + l.alpha_pos : nullptr;
  double* a_mass = alpha && cotj && grad_mass ? ws + l.alpha_mass : nullptr;
  if (alpha) {
    const int rc = nbd_accel_vjp_f64(posd, cota, n, softening_sq, g_const, cotj ? a_pos : grad_pos,
                                     cotj ? a_mass : grad_mass, ws + l.alpha_ws, slabs, stream);
    if (rc) return rc;
  }
  const dim3 fgrid(ceil_div(n, 256)), fblock(256);
  if (!cotj) {
    double* zp = alpha ? nullptr : grad_pos;
    double* zm = alpha ? nullptr : grad_mass;
    if (!zp && !zm && !grad_vel) return 0;
    accel_jerk_vjp_finish_f64_kernel<<<fgrid, fblock, 0, st>>>(ws, 0, n, g_const, nullptr, nullptr, zp, grad_vel, zm);
    return launch_status();
  }
  const ChunkSplit c = chunk_split(p.n_chunks, slabs);
  accel_jerk_vjp_f64_kernel<<<dim3(p.groups, slabs), 64 * kWaves, 0, st>>>(
      reinterpret_cast<const d4*>(posd), reinterpret_cast<const d4*>(veld), reinterpret_cast<const d4*>(cotj), n, c.q,
      c.r, softening_sq, softening_sq < kEps2MaskedF64 ? 1 : 0, ws);
  const int rc = launch_status();
  if (rc) return rc;
  accel_jerk_vjp_finish_f64_kernel<<<fgrid, fblock, 0, st>>>(ws, slabs, n, g_const, a_pos, a_mass, grad_pos, grad_vel,
                                                             grad_mass);
  return launch_status();
}

}  // extern "C"
