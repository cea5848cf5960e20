// direct_grad.hip -- the backward of the all-pairs acceleration for gfx950 (MI355X): the vector-Jacobian product of
//   a_i = G sum_{j != i} m_j d s^3,   d = x_j - x_i,   s = (|d|^2 + eps^2)^(-1/2)
// with a cotangent g = dL/da (n, 3), with respect to positions and masses. With h_ij = m_i g_j - m_j g_i:
//   dL/dx_i =  G sum_{j != i} [ s^3 h_ij - 3 s^5 d (d . h_ij) ]
//   dL/dm_i = -G sum_{j != i}   s^3 (d . g_j)
// An extension: the reference gets these from torch's autograd through its nine lines of torch. C-ABI: the nbd_accel_vjp_*
// entries of include/nbd.h; Python: nbd.autograd.direct_accel and the simulators' compute_accelerations() under autograd.
//
// The position gradient has the shape of the jerk (s^3 dv - 3 s^5 d (d . dv), with h in the place of m_j dv), so both
// kernels are the Hermite kernels' chunk walks with another pair arithmetic:
//   fp32: accel_jerk_body (hermite_kernels.h) with the pair policy AccelVjpPolicy. Sources are posm rows {x, y, z, m} and
//         cotangent rows {gx, gy, gz, 0} (nbd_hermite_pack_f32 with the cotangent as the velocities), two targets per
//         lane, 128 per workgroup, plan_jerk(n, n); float[slabs][4][n] partial sums, then accel_vjp_finish_kernel.
//   fp64: walk_f64 (hermite_f64_kernels.h) with the pair functor AccelVjpPair, plan_f64(n); double[slabs][4][n], then
//         accel_vjp_finish_f64_kernel.
// No atomics, no memsets, no host syncs: deterministic run to run with a workspace that may hold anything, and capturable.
//
// The i == j term. The force kernels leave it to d = 0 on the un-masked path; here s^3 h_ii survives unless h_ii is an
// exact zero, and s^3 = eps^-3 multiplies whatever is left: fma(m_i, g_i, -round(m_i g_i)) is the rounding residual of
// the product. So the chunks that hold a group's own indices -- two in fp32, one in fp64 -- go through the index-masked
// pair whatever the softening, as potential_body and walk_f64 do, and h is one product and one fma everywhere. (The other
// way, h from two separately rounded products and one subtraction, which is an exact zero at j == i, is kept as a
// measurement variant: 3 packed ops more per source, 3-5 % slower on the MI355X.) A padding row (m = 0, g = 0) gives h = 0
// and d . g_j = 0 with a finite s. Below eps^2 = 1e-24 every chunk is index-masked and the result is the closed form over
// j != i (torch's autograd gives NaN for every row at eps = 0).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_kernels.h"
#include "hermite_f64_kernels.h"
#include "hermite_kernels.h"

namespace {

// ---- fp32: the pair policy of accel_jerk_body (what a policy is: AccelJerkPolicy, hermite_kernels.h)
// acc[0..2] accumulates s^3 h, acc[3..5] (d . h s^2) s^3 d, acc[6] s^3 (d . g_j); out = {acc[0..2] - 3 acc[3..5], acc[6]}.
// Two such sets, acc[0..6] for the even sources and acc[7..13] for the odd ones, added when the outputs are formed: the
// error of these gradients is the error of the fp32 chains (with exact sums the kernel's terms give torch's fp32 figures;
// one chain per wave misses four times those figures in a row of the n = 65 test, NOTES), and a second set halves every
// chain for 14 registers and no instruction in the loop.
// Per source and pair of targets: 3 v_pk_add (d), 3 v_pk_fma (r^2), 2 v_rsq_f32, 3 v_pk_mul + 3 v_pk_fma (h), 2 v_pk_mul +
// 4 v_pk_fma (d . h, d . g_j), 4 v_pk_mul (s^2, s^3, d . h s^2, c), 7 v_pk_fma (the sums): 29 packed ops.
// OWN (what the library builds): h by one product and one fma, and the two chunks that hold the workgroup's own indices
// go through the index-masked pair. !OWN (the measurement variant, NBD_VJP_OWN_MASKED=0): h by two products and one
// subtraction, an exact zero at j == i, no chunk masked for its indices: 32 packed ops.
template <bool OWN>
struct AccelVjpPolicyT {
  static constexpr int kSet = 7, kAcc = 2 * kSet, kOut = 4;
  f2 xi, yi, zi, gxi, gyi, gzi, mi;

  __device__ __forceinline__ AccelVjpPolicyT(const f4 t0, const f4 t1, const f4 u0, const f4 u1)
      : xi{t0.x, t1.x}, yi{t0.y, t1.y}, zi{t0.z, t1.z}, gxi{u0.x, u1.x}, gyi{u0.y, u1.y}, gzi{u0.z, u1.z},
        mi{t0.w, t1.w} {}

  __device__ __forceinline__ bool own(int pc, int i0) const {
    return OWN && (pc >> 1) == __builtin_amdgcn_readfirstlane(i0 >> 7);
  }

  // h = m_i g_j - m_j g_i for one component: gj = g_j splat, mj = m_j splat, gi = the targets' own. Plain C++: with
  // interact()'s asm multiply for the m_j splat hipcc pads the asm operands with s_nop and still copies a register per
  // source in the two-product form (85 instructions per two sources against 81, counted on the gfx950 assembly).
  __device__ __forceinline__ f2 h_of(const f2 gj, const f2 mj, const f2 gi) const {
    if (OWN) return __builtin_elementwise_fma(mi, gj, -(mj * gi));
    return mi * gj - mj * gi;
  }

  // the sums of one source, from d, h, d . g_j and s (masked or not)
  __device__ __forceinline__ void add(f2* acc, const f2 dx, const f2 dy, const f2 dz, const f2 hx, const f2 hy,
                                      const f2 hz, const f2 dh, const f2 dg, const f2 s) const {
    const f2 s2 = s * s;
    const f2 s3 = s2 * s;
    const f2 c = (dh * s2) * s3;
    acc[0] = __builtin_elementwise_fma(s3, hx, acc[0]);
    acc[1] = __builtin_elementwise_fma(s3, hy, acc[1]);
    acc[2] = __builtin_elementwise_fma(s3, hz, acc[2]);
    acc[3] = __builtin_elementwise_fma(c, dx, acc[3]);
    acc[4] = __builtin_elementwise_fma(c, dy, acc[4]);
    acc[5] = __builtin_elementwise_fma(c, dz, acc[5]);
    acc[6] = __builtin_elementwise_fma(s3, dg, acc[6]);
  }

  // One source against the lane's two targets, index-masked: only j == i and the padding behind n are dropped, by a
  // select on s. (There is no range-sharded form: RANGE and the excluded range are ignored.)
  template <bool RANGE>
  __device__ __forceinline__ void masked(const f4 p, const f4 q, const f2 e2, f2* acc, int j, int i0, int i1, int n,
                                         int = 0, int = 0) const {
    const f2 dx = f2{p.x, p.x} - xi, dy = f2{p.y, p.y} - yi, dz = f2{p.z, p.z} - zi;
    f2 r2 = __builtin_elementwise_fma(dx, dx, e2);
    r2 = __builtin_elementwise_fma(dy, dy, r2);
    r2 = __builtin_elementwise_fma(dz, dz, r2);
    const f2 gx = {q.x, q.x}, gy = {q.y, q.y}, gz = {q.z, q.z}, mj = {p.w, p.w};
    const f2 hx = h_of(gx, mj, gxi), hy = h_of(gy, mj, gyi), hz = h_of(gz, mj, gzi);
    f2 dh = dx * hx;
    dh = __builtin_elementwise_fma(dy, hy, dh);
    dh = __builtin_elementwise_fma(dz, hz, dh);
    f2 dg = dx * gx;
    dg = __builtin_elementwise_fma(dy, gy, dg);
    dg = __builtin_elementwise_fma(dz, gz, dg);
    f2 s = {__builtin_amdgcn_rsqf(r2.x), __builtin_amdgcn_rsqf(r2.y)};
    s.x = (j < n && j != i0) ? s.x : 0.0f;
    s.y = (j < n && j != i1) ? s.y : 0.0f;
    if (j & 1) add(acc + kSet, dx, dy, dz, hx, hy, hz, dh, dg, s);      // j is uniform: a branch, never an indexed register
    else add(acc, dx, dy, dz, hx, hy, hz, dh, dg, s);
  }

  // KU sources at once, un-masked: jerk_block's shape (the 2 KU v_rsq_f32 issued back to back; every consumer of an
  // rsq result is plain C++, so hipcc pads the transcendental hazard itself).
  template <int KU>
  __device__ __forceinline__ void block(const f4* __restrict__ bp, const f4* __restrict__ bv, const f2 e2, f2* acc) const {
    static_assert(KU % 2 == 0, "the two accumulator sets alternate inside a block");
    f2 dx[KU], dy[KU], dz[KU], hx[KU], hy[KU], hz[KU], dh[KU], dg[KU], s[KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const f4 p = bp[u], q = bv[u];
      dx[u] = f2{p.x, p.x} - xi; dy[u] = f2{p.y, p.y} - yi; dz[u] = f2{p.z, p.z} - zi;
      f2 r2 = __builtin_elementwise_fma(dx[u], dx[u], e2);
      r2 = __builtin_elementwise_fma(dy[u], dy[u], r2);
      s[u] = __builtin_elementwise_fma(dz[u], dz[u], r2);
      const f2 gx = {q.x, q.x}, gy = {q.y, q.y}, gz = {q.z, q.z}, mj = {p.w, p.w};
      hx[u] = h_of(gx, mj, gxi); hy[u] = h_of(gy, mj, gyi); hz[u] = h_of(gz, mj, gzi);
      f2 t = dx[u] * hx[u];
      t = __builtin_elementwise_fma(dy[u], hy[u], t);
      dh[u] = __builtin_elementwise_fma(dz[u], hz[u], t);
      t = dx[u] * gx;
      t = __builtin_elementwise_fma(dy[u], gy, t);
      dg[u] = __builtin_elementwise_fma(dz[u], gz, t);
    }
#pragma unroll
    for (int u = 0; u < KU; ++u) s[u] = f2{__builtin_amdgcn_rsqf(s[u].x), __builtin_amdgcn_rsqf(s[u].y)};
    __builtin_amdgcn_sched_group_barrier(0x400, 2 * KU, 0);      // 0x400 = TRANS: keep the rsq's together
#pragma unroll
    for (int u = 0; u < KU; ++u)      // a block starts at an even source (KU is even)
      add(acc + (u & 1) * kSet, dx[u], dy[u], dz[u], hx[u], hy[u], hz[u], dh[u], dg[u], s[u]);
  }

  __device__ __forceinline__ f2 out(const f2* acc, int k) const {
    if (k < 3) return (acc[k] + acc[kSet + k]) - 3.0f * (acc[k + 3] + acc[kSet + k + 3]);
    return acc[6] + acc[kSet + 6];
  }
};

#ifndef NBD_VJP_OWN_MASKED
#define NBD_VJP_OWN_MASKED 1      // 0: the measurement variant (tools/bench_accel_vjp.py builds it beside the library)
#endif
using AccelVjpPolicy = AccelVjpPolicyT<NBD_VJP_OWN_MASKED != 0>;

constexpr int kVjpKU = 2;

// The partial sums of all n bodies under all n bodies: accel_jerk_kernel's geometry (direct_hermite.hip), grid = (target
// groups of 128, slabs), the chunks spread over all slabs x 4 waves to within one. out: float[slab][4][n].
template <bool MASKED>
__global__ __launch_bounds__(64 * kWaves) void accel_vjp_kernel(const f4* __restrict__ posm, const f4* __restrict__ cot,
                                                                int n, int cpw_q, int cpw_r, float eps2,
                                                                float* __restrict__ out) {
  __shared__ f4 lds[kWaves * 4 * kChunk];
  const int t_base = blockIdx.x * kTgtPerWG;
  const int i0 = t_base + (threadIdx.x & 63), i1 = i0 + 64;
  const int jw = blockIdx.y * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int c_begin, c_end;
  wave_chunk_range(jw, cpw_q, cpw_r, c_begin, c_end);
  accel_jerk_body<MASKED, kVjpKU, 1, false, AccelVjpPolicy>(
      posm, cot, n, posm, cot, min(i0, n - 1), min(i1, n - 1), i0, i1, c_begin, c_end, eps2, lds,
      out + (size_t)blockIdx.y * AccelVjpPolicy::kOut * n + t_base, n, min(kTgtPerWG, n - t_base));
}

// One workgroup per 64 consecutive bodies: the slabs of float[n_slabs][4][n] in hermite_slab_sum's order (wave w sums
// slabs w, w + 4, ... of its lane's row, the four partials combined as (p0 + p1) + (p2 + p3)), then G, once:
// grad_pos[i] = g * sum (3 components), grad_mass[i] = -g * sum. Either output may be null.
__global__ __launch_bounds__(256) void accel_vjp_finish_kernel(const float* __restrict__ slabs, int n_slabs, int n,
                                                               float g, float* __restrict__ grad_pos,
                                                               float* __restrict__ grad_mass) {
  __shared__ float part[4][4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
  if (i < n)
    for (int s = w; s < n_slabs; s += 4)
#pragma unroll
      for (int k = 0; k < 4; ++k) sum[k] += slabs[((size_t)s * 4 + k) * n + i];
#pragma unroll
  for (int k = 0; k < 4; ++k) part[w][k][lane] = sum[k];
  __syncthreads();
  if (w != 0 || i >= n) return;
  auto total = [&](int k) { return (part[0][k][lane] + part[1][k][lane]) + (part[2][k][lane] + part[3][k][lane]); };
  if (grad_pos) {
#pragma unroll
    for (int k = 0; k < 3; ++k) grad_pos[3 * (size_t)i + k] = g * total(k);
  }
  if (grad_mass) grad_mass[i] = 0.0f - g * total(3);
}

// ---- fp64: the pair functor of walk_f64 (what a functor is: hermite_f64_kernels.h). p = {x, y, z, m} of source j,
// q = {gx, gy, gz, 0} of source j. walk_f64 walks the chunk of the group's own rows MASKED whatever the softening, so
// i == j never reaches the un-masked pair and h is one product and one fma.
struct AccelVjpPair {
  static constexpr bool kVel = true;
  static constexpr int kOut = 4;
  double xi, yi, zi, gxi, gyi, gzi, mi, e2;
  double acc[7];
  int i, n;

  __device__ __forceinline__ AccelVjpPair(const d4 tp, const d4 tg, double eps2, int i_, int n_)
      : xi(tp.x), yi(tp.y), zi(tp.z), gxi(tg.x), gyi(tg.y), gzi(tg.z), mi(tp.w), e2(eps2), i(i_), n(n_) {
#pragma unroll
    for (int k = 0; k < 7; ++k) acc[k] = 0.0;
  }

  template <bool MASKED>
  __device__ __forceinline__ void pair(const d4 p, const d4 q, int j) {
    const double dx = p.x - xi, dy = p.y - yi, dz = p.z - zi;      // x_j - x_i
    double r2 = __builtin_fma(dx, dx, e2);
    r2 = __builtin_fma(dy, dy, r2);
    r2 = __builtin_fma(dz, dz, r2);
    const double hx = __builtin_fma(mi, q.x, -(p.w * gxi));
    const double hy = __builtin_fma(mi, q.y, -(p.w * gyi));
    const double hz = __builtin_fma(mi, q.z, -(p.w * gzi));
    double dh = dx * hx;
    dh = __builtin_fma(dy, hy, dh);
    dh = __builtin_fma(dz, hz, dh);
    double dg = dx * q.x;
    dg = __builtin_fma(dy, q.y, dg);
    dg = __builtin_fma(dz, q.z, dg);
    double s = rsqrt_f64(r2);
    if (MASKED) s = (j < n && j != i) ? s : 0.0;
    const double s2 = s * s;
    const double s3 = s2 * s;
    const double c = (dh * s2) * s3;
    acc[0] = __builtin_fma(s3, hx, acc[0]);
    acc[1] = __builtin_fma(s3, hy, acc[1]);
    acc[2] = __builtin_fma(s3, hz, acc[2]);
    acc[3] = __builtin_fma(c, dx, acc[3]);
    acc[4] = __builtin_fma(c, dy, acc[4]);
    acc[5] = __builtin_fma(c, dz, acc[5]);
    acc[6] = __builtin_fma(s3, dg, acc[6]);
  }

  __device__ __forceinline__ double out(int k) const { return k < 3 ? acc[k] - 3.0 * acc[k + 3] : acc[6]; }
};

// force_f64_kernel's geometry (direct_hermite_f64.hip): grid = (groups of 64 targets, slabs). out: double[slab][4][n].
__global__ __launch_bounds__(64 * kWaves) void accel_vjp_f64_kernel(const d4* __restrict__ posd,
                                                                    const d4* __restrict__ cotd, int n, int cpw_q,
                                                                    int cpw_r, double eps2, int all_masked,
                                                                    double* __restrict__ out) {
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads<true>()];
  const Group64<unsigned> g(blockIdx.x, blockIdx.y, n);
  const ChunkRange c = wave_chunks(g.jw(), cpw_q, cpw_r);
  AccelVjpPair pr(posd[g.row()], cotd[g.row()], eps2, g.i, n);
  walk_f64(pr, posd, cotd, c.begin, c.end, all_masked != 0, blockIdx.x, lds, g.dst<AccelVjpPair>(out), (size_t)n,
           g.n_valid());
}

// One thread per body: the slabs of double[n_slabs][4][n] in slab order (slab_order_sum, hermite_kernels.h), then G,
// once. Either output may be null.
__global__ __launch_bounds__(256) void accel_vjp_finish_f64_kernel(const double* __restrict__ slabs, int n_slabs, int n,
                                                                   double g, double* __restrict__ grad_pos,
                                                                   double* __restrict__ grad_mass) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double sum[4];
  slab_order_sum<4>(slabs, n_slabs, (size_t)n, (size_t)i, sum);
  if (grad_pos) {
#pragma unroll
    for (int k = 0; k < 3; ++k) grad_pos[3 * (size_t)i + k] = g * sum[k];
  }
  if (grad_mass) grad_mass[i] = 0.0 - g * sum[3];
}

}  // namespace

extern "C" {

size_t nbd_accel_vjp_workspace_bytes(int n) {
  if (n <= 0) return 0;
  return (size_t)plan_jerk(n, n).slabs * AccelVjpPolicy::kOut * n * sizeof(float);
}

int nbd_accel_vjp_f32(const float* posm, const float* cot, int n, float softening_sq, float g_const, float* grad_pos,
                      float* grad_mass, void* workspace, nbd_stream_t stream) {
  if (n < 0 || !isfinite(softening_sq) || !isfinite(g_const)) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (!posm || !cot || misaligned16(posm) || misaligned16(cot) || (!grad_pos && !grad_mass)) return NBD_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(grad_pos) | reinterpret_cast<uintptr_t>(grad_mass)) & 3) return NBD_E_BADARG;
  if (!workspace || misaligned16(workspace)) return NBD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const JerkPlan p = plan_jerk(n, n);
  const ChunkSplit c = chunk_split(p.n_chunks, p.slabs);
  const dim3 grid(p.groups, p.slabs), block(64 * kWaves);
  const f4* pm = reinterpret_cast<const f4*>(posm);
  const f4* ct = reinterpret_cast<const f4*>(cot);
  float* slabs = static_cast<float*>(workspace);
  if (softening_sq < kEps2Masked) accel_vjp_kernel<true><<<grid, block, 0, st>>>(pm, ct, n, c.q, c.r, softening_sq, slabs);
  else accel_vjp_kernel<false><<<grid, block, 0, st>>>(pm, ct, n, c.q, c.r, softening_sq, slabs);
  const int rc = launch_status();
  if (rc) return rc;
  accel_vjp_finish_kernel<<<ceil_div(n, 64), 256, 0, st>>>(slabs, p.slabs, n, g_const, grad_pos, grad_mass);
  return launch_status();
}

size_t nbd_accel_vjp_f64_workspace_bytes(int n, int slabs) {
  if (n <= 0 || slabs < 0 || slabs > kMaxSlabs) return 0;
  if (slabs == 0) slabs = plan_f64(n).slabs;
  return (size_t)slabs * AccelVjpPair::kOut * n * sizeof(double);
}

int nbd_accel_vjp_f64(const double* posd, const double* cotd, int n, double softening_sq, double g_const,
                      double* grad_pos, double* grad_mass, void* workspace, int slabs, nbd_stream_t stream) {
  if (n < 0 || slabs < 0 || slabs > kMaxSlabs || !isfinite(softening_sq) || !isfinite(g_const)) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (!posd || !cotd || misaligned32(posd) || misaligned32(cotd) || (!grad_pos && !grad_mass)) return NBD_E_BADARG;
  if (misaligned8(grad_pos) || misaligned8(grad_mass) || !workspace || misaligned8(workspace)) return NBD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const F64Plan p = plan_f64(n);
  if (slabs == 0) slabs = p.slabs;
  const ChunkSplit c = chunk_split(p.n_chunks, slabs);
  double* part = static_cast<double*>(workspace);
  accel_vjp_f64_kernel<<<dim3(p.groups, slabs), 64 * kWaves, 0, st>>>(
      reinterpret_cast<const d4*>(posd), reinterpret_cast<const d4*>(cotd), n, c.q, c.r, softening_sq,
      softening_sq < kEps2MaskedF64 ? 1 : 0, part);
  const int rc = launch_status();
  if (rc) return rc;
  accel_vjp_finish_f64_kernel<<<ceil_div(n, 256), 256, 0, st>>>(part, slabs, n, g_const, grad_pos, grad_mass);
  return launch_status();
}

}  // extern "C"
