// direct_kernels.h -- what the direct-path translation units share (direct_force.hip: one system; direct_batch.hip: many
// independent systems back to back; direct_diag.hip: the diagnostics of both; through hermite_kernels.h the three Hermite
// units): the host helpers of their entry
// points (ceil_div, misaligned8 / 16 / 32, shard_args_ok, launch_status) and the device building blocks: the pair arithmetic (interact, interact_block,
// energy_pair, potential_pair) and, one level up, the wave bodies that walk the source chunks with it (accel_body, energy_body, potential_body: target
// loads, LDS-DMA chunk walk, pair loop, four-wave reduction, store), and the sums of the conserved quantities (invariants_body). A force or energy kernel of either unit is a
// prologue that reads its geometry (from blockIdx and arguments, or from a scene record) and one call of the body: that
// is what keeps a scene of a batch bit-identical to the same system run alone.
// The definitions sit in an anonymous namespace: every translation unit that includes this file gets its own inlined copies.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbd.h"

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef double d4 __attribute__((ext_vector_type(4)));      // the packed row of the float64 Hermite units

#define GPTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define LPTR(p) ((__attribute__((address_space(3))) void*)(p))

namespace {

constexpr int kWaves = 4;                  // waves per workgroup (J-split inside the workgroup)
constexpr int kTgtPerLane = 2;             // packed pair of targets per lane
constexpr int kTgtPerWG = 64 * kTgtPerLane;  // 128 targets per workgroup
constexpr int kChunk = NBD_SRC_PAD;        // 64 sources = one 1-KiB LDS-DMA piece
constexpr int kMaxSlabs = 64;
// below this softening^2 the cube of rsq overflows fp32 for coincident bodies (and the i==j
// term), so the index-masked kernel is used (fill_diagonal_ semantics, simulation.py:85)
constexpr float kEps2Masked = 1e-24f;

__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
inline bool misaligned32(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 31) != 0; }
inline bool misaligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) != 0; }
// a rank's bodies [lo, lo + n_local) lie within the n_total of a range partition (every range-sharded entry point; no
// sum that could overflow)
inline bool shard_args_ok(int n_total, int lo, int n_local) {
  return n_total >= 0 && lo >= 0 && n_local >= 0 && lo <= n_total && n_local <= n_total - lo;
}
// 0 or the HIP error of the last launch, as the C-ABI returns it
inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// Which sources a launch walks: the 64-source chunks of `src` minus a run of skipped physical chunks,
// with an element-wise exclusion in the (at most two) chunks that hold a partial piece of the excluded
// index range. The un-sharded force uses the trivial view; the range-sharded step (nbd_shard_*) walks
// "all bodies except my own [lo, hi)" with it while its own block runs from a separate launch.
struct SrcView {
  int n_src;           // real entries; the padding behind them is zero-mass
  int n_chunks;        // logical chunks walked (physical chunks minus the skipped run)
  int cpw_q, cpw_r;    // balanced split: every wave walks cpw_q chunks, the first cpw_r waves one more
  int skip_c0, skip_cn;  // physical chunks [skip_c0, skip_c0 + skip_cn) are not visited
  int ex_lo, ex_hi;    // source indices [ex_lo, ex_hi) contribute nothing (checked only where needed)
  int edge0, edge1;    // physical chunks that straddle ex_lo / ex_hi (-1: none): these take the masked path
  int tail;            // uniform-mass kernels only: the physical chunk that holds padding behind n_src (-1: none); it takes
                       // the masked path too (without the per-source mass factor a padding entry is not a zero any more)
};

// the balanced split of a view's n_chunks logical chunks over slabs x 4 waves
__host__ __device__ inline void split_chunks(SrcView& v, int n_chunks, int slabs) {
  v.n_chunks = n_chunks;
  v.cpw_q = n_chunks / (slabs * kWaves); v.cpw_r = n_chunks % (slabs * kWaves);
}

// all sources of an n_src array (n_chunks = ceil(n_src / 64)), split over `slabs` slabs
__host__ __device__ inline SrcView full_view(int n_src, int n_chunks, int slabs) {
  SrcView v;
  v.n_src = n_src;
  split_chunks(v, n_chunks, slabs);
  v.skip_c0 = n_chunks; v.skip_cn = 0; v.ex_lo = 0; v.ex_hi = 0; v.edge0 = -1; v.edge1 = -1;
  v.tail = (n_src % kChunk) ? n_src / kChunk : -1;
  return v;
}

// logical chunk count of "n_src sources without the indices [ex_lo, ex_hi)": whole chunks inside the
// excluded range are hopped over, chunks that straddle one of its ends are walked with the element mask
inline int excluded_view(int n_src, int ex_lo, int ex_hi, SrcView* v) {
  const int phys = ceil_div(n_src, kChunk);
  int c0 = ceil_div(ex_lo, kChunk), c1 = ex_hi / kChunk;      // whole chunks [c0, c1) lie inside
  if (ex_hi >= n_src) c1 = phys;                               // the tail chunk holds padding only beyond ex_hi
  if (c1 < c0) c1 = c0;
  if (v) {
    v->n_src = n_src; v->skip_c0 = c0; v->skip_cn = c1 - c0; v->ex_lo = ex_lo; v->ex_hi = ex_hi;
    v->edge0 = (ex_lo % kChunk) ? ex_lo / kChunk : -1;
    v->edge1 = (ex_hi % kChunk && ex_hi < n_src) ? ex_hi / kChunk : -1;
    if (ex_hi <= ex_lo) { v->skip_c0 = phys; v->skip_cn = 0; v->edge0 = v->edge1 = -1; }
    v->tail = (n_src % kChunk) ? n_src / kChunk : -1;
  }
  return ex_hi <= ex_lo ? phys : phys - (c1 - c0);
}

// One source against the lane's two targets. 12 packed ops + 2 v_rsq_f32 (UNI: 11, see accel_kernel).
template <bool MASKED, bool UNI = false>
__device__ __forceinline__ void interact(const f4 p, const f2 xi, const f2 yi, const f2 zi,
                                         const f2 e2, f2& ax, f2& ay, f2& az, int j, int i0,
                                         int i1, const SrcView& sv) {
  const f2 dx = f2{p.x, p.x} - xi, dy = f2{p.y, p.y} - yi, dz = f2{p.z, p.z} - zi;  // r_j - r_i
  f2 r2 = __builtin_elementwise_fma(dx, dx, e2);
  r2 = __builtin_elementwise_fma(dy, dy, r2);
  r2 = __builtin_elementwise_fma(dz, dz, r2);
  f2 s = {__builtin_amdgcn_rsqf(r2.x), __builtin_amdgcn_rsqf(r2.y)};
  if (MASKED) {  // exact fill_diagonal_(0): only j == i is dropped; padding and the excluded range too
    const bool live = j < sv.n_src && (unsigned)(j - sv.ex_lo) >= (unsigned)(sv.ex_hi - sv.ex_lo);
    s.x = (live && j != i0) ? s.x : 0.0f;
    s.y = (live && j != i1) ? s.y : 0.0f;
  }
  // w = m_j * s^3 with m_j broadcast from the HIGH half of the {z,m} register pair; hipcc does not
  // fold that splat into op_sel by itself (it inserts a v_mov), hence the one asm line. The asm
  // multiply takes s^3 (an ordinary VALU result), never s itself: gfx950 needs a wait state between
  // a transcendental result and its VALU consumer, and hipcc pads that only for instructions it
  // can see (an asm consumer right behind v_rsq_f32/v_rcp_f32 reads a stale register).
  const f2 zm = {p.z, p.w};
  const f2 s3 = (s * s) * s;
  f2 w;  // m_j (r^2 + eps^2)^(-3/2)
  if (UNI) w = s3;               // equal masses: the common factor is applied once, to the finished sum
  else asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(w) : "v"(zm), "v"(s3));
  ax = __builtin_elementwise_fma(w, dx, ax);
  ay = __builtin_elementwise_fma(w, dy, ay);
  az = __builtin_elementwise_fma(w, dz, az);
}

// KU sources at once for the un-masked path: same arithmetic as interact(), with the 2*KU v_rsq_f32
// issued back to back (__builtin_amdgcn_sched_group_barrier on the TRANS class). Switching between the
// quarter-rate transcendental unit and the packed-math stream costs issue cycles on gfx950 (3 fma : 1
// rsq mixes run ~10 % under the sum of their parts, tools/ubench_valu.hip), so the switches are
// batched; the rsq stays a compiler builtin so that hipcc fills the transcendental -> VALU wait state
// with independent work instead of the s_nop it must put behind an opaque asm block. Measured
// (tools/k1_variants.hip, N = 65 536): KU = 8 at 90 VGPRs / 5 waves per SIMD beats KU = 4 at 58 VGPRs /
// 8 waves (1.004 vs 1.010 ms) and an inline-asm rsq block (1.021 ms).
template <int KU, bool UNI = false>
__device__ __forceinline__ void interact_block(const f4* __restrict__ buf, const f2 xi, const f2 yi, const f2 zi,
                                               const f2 e2, f2& ax, f2& ay, f2& az) {
  f4 p[KU];
  f2 dx[KU], dy[KU], dz[KU], s[KU];
#pragma unroll
  for (int u = 0; u < KU; ++u) {
    p[u] = buf[u];
    if (UNI) asm("" : "+v"(p[u]));      // keep the source a whole 4-register tuple: with the mass unused hipcc loads 96 bits
                                        // and then copies z out of its odd register to splat it (a v_mov per source)
    dx[u] = f2{p[u].x, p[u].x} - xi; dy[u] = f2{p[u].y, p[u].y} - yi; dz[u] = f2{p[u].z, p[u].z} - zi;
    f2 r2 = __builtin_elementwise_fma(dx[u], dx[u], e2);
    r2 = __builtin_elementwise_fma(dy[u], dy[u], r2);
    s[u] = __builtin_elementwise_fma(dz[u], dz[u], r2);
  }
#pragma unroll
  for (int u = 0; u < KU; ++u) s[u] = f2{__builtin_amdgcn_rsqf(s[u].x), __builtin_amdgcn_rsqf(s[u].y)};
  __builtin_amdgcn_sched_group_barrier(0x400, 2 * KU, 0);      // 0x400 = TRANS: keep the rsq's together
#pragma unroll
  for (int u = 0; u < KU; ++u) {
    const f2 zm = {p[u].z, p[u].w};
    const f2 s3 = (s[u] * s[u]) * s[u];          // compiler-visible consumers of the rsq results (hazard-padded)
    f2 w;
    if (UNI) w = s3;
    else asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(w) : "v"(zm), "v"(s3));
    ax = __builtin_elementwise_fma(w, dx[u], ax);
    ay = __builtin_elementwise_fma(w, dy[u], ay);
    az = __builtin_elementwise_fma(w, dz[u], az);
  }
}

// The wave body of the all-pairs force kernels. A workgroup is 4 waves on the 128 targets tgt[t_base ..] (two per lane in
// packed fp32; global index tgt_off + row, what the masked loop takes for the lane's own source). Wave jw = slab * 4 + w
// walks the logical source chunks [jw*q + min(jw, r), ... + q (+1 if jw < r)) of the view: all chunks are spread over all
// waves to within one chunk (no idle tail waves). Each chunk comes HBM/L2 -> LDS by LDS-DMA, double-buffered behind a
// counted vmcnt; `masked` (or an edge chunk of the view, or the padded tail of a UNI walk) takes the index-masked loop,
// every other chunk interact_block<KU>. `masked` is a bool known at run time (a scene of a batch: tested once per chunk)
// or a std::integral_constant where the kernel's template parameter decides (the dead loop is never emitted). The 4 waves' partials are reduced through LDS ([wave][comp*2+half][64]) in wave
// order into one coalesced store dst[t * 3 + comp] = scale * sum for the valid targets. lds: the workgroup's
// f4[kAccelLdsF4]: [wave][buffer][64] staging + [wave][6][64] partials, ONE object (keeps hipcc's waits sane).
// tid: the thread's index among the 4 waves (threadIdx.x, or its low 8 bits where a 512-thread workgroup runs two groups
// side by side, each on its own lds region: both halves then meet at the one __syncthreads()).
constexpr int kAccelLdsF4 = kWaves * 2 * kChunk + kWaves * 6 * 64 / 4;

template <int KU, bool UNI, class Masked>
__device__ __forceinline__ void accel_body(const f4* __restrict__ src, const SrcView& sv, const Masked masked,
                                           const f4* __restrict__ tgt, int n_tgt, int tgt_off, int t_base, int slab,
                                           float eps2, float scale, f4* lds, float* __restrict__ dst, const int tid) {
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i0 = t_base + lane, i1 = t_base + 64 + lane;
  const f4 t0 = tgt[min(i0, n_tgt - 1)], t1 = tgt[min(i1, n_tgt - 1)];
  const f2 xi = {t0.x, t1.x}, yi = {t0.y, t1.y}, zi = {t0.z, t1.z};
  f2 ax = {0.f, 0.f}, ay = {0.f, 0.f}, az = {0.f, 0.f};
  f2 e2 = {eps2, eps2};
  asm volatile("" : "+v"(e2));  // keep eps^2 in VGPRs: an SGPR operand halves v_pk_fma issue

  const int jw = slab * kWaves + wave;
  const int c_begin = jw * sv.cpw_q + min(jw, sv.cpw_r), c_end = c_begin + sv.cpw_q + (jw < sv.cpw_r ? 1 : 0);
  f4* stage = &lds[wave * 2 * kChunk];
  const f4* s_lane = src + lane;
  // logical -> physical chunk: hop over the skipped run
  auto phys = [&](int c) { return c + (c >= sv.skip_c0 ? sv.skip_cn : 0); };
  if (c_begin < c_end)
    __builtin_amdgcn_global_load_lds(GPTR(s_lane + (size_t)phys(c_begin) * kChunk), LPTR(stage), 16, 0, 0);
  for (int c = c_begin; c < c_end; ++c) {
    const int b = (c - c_begin) & 1;
    if (c + 1 < c_end) {
      __builtin_amdgcn_global_load_lds(GPTR(s_lane + (size_t)phys(c + 1) * kChunk),
                                       LPTR(stage + (b ^ 1) * kChunk), 16, 0, 0);
      asm volatile("s_waitcnt vmcnt(1)" ::: "memory");  // chunk c has landed, c+1 in flight
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const f4* buf = stage + b * kChunk;
    const int pc = phys(c);
    const int j0 = pc * kChunk;
    if (masked || pc == sv.edge0 || pc == sv.edge1 || (UNI && pc == sv.tail)) {
#pragma unroll 4
      for (int j = 0; j < kChunk; ++j)
        interact<true, UNI>(buf[j], xi, yi, zi, e2, ax, ay, az, j0 + j, tgt_off + i0, tgt_off + i1, sv);
    } else {
#pragma unroll 1
      for (int j = 0; j < kChunk; j += KU) interact_block<KU, UNI>(buf + j, xi, yi, zi, e2, ax, ay, az);
    }
  }

  // wavefront partials -> LDS -> one coalesced (128 x 3) store per workgroup, waves added in fixed order
  float* red = reinterpret_cast<float*>(&lds[kWaves * 2 * kChunk]);  // [wave][comp*2+half][64]
  float* mine = red + wave * 6 * 64;
  mine[0 * 64 + lane] = ax.x; mine[1 * 64 + lane] = ax.y;
  mine[2 * 64 + lane] = ay.x; mine[3 * 64 + lane] = ay.y;
  mine[4 * 64 + lane] = az.x; mine[5 * 64 + lane] = az.y;
  __syncthreads();
  const int n_valid = min(kTgtPerWG, n_tgt - t_base) * 3;
  for (int o = tid; o < n_valid; o += 64 * kWaves) {
    const int lt = o / 3, comp = o - lt * 3;
    const int idx = (comp * 2 + (lt >> 6)) * 64 + (lt & 63);
    float sum = red[idx];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) sum += red[w * 6 * 64 + idx];
    dst[o] = __fmul_rn(scale, sum);
  }
}

// the workgroup IS the 4 waves
template <int KU, bool UNI, class Masked>
__device__ __forceinline__ void accel_body(const f4* __restrict__ src, const SrcView& sv, const Masked masked,
                                           const f4* __restrict__ tgt, int n_tgt, int tgt_off, int t_base, int slab,
                                           float eps2, float scale, f4* lds, float* __restrict__ dst) {
  accel_body<KU, UNI>(src, sv, masked, tgt, n_tgt, tgt_off, t_base, slab, eps2, scale, lds, dst, threadIdx.x);
}

// ---- energies (simulation.py:91-115). U = sum_{i<j} -G m_i m_j / (|r_ij| + eps), K = sum 0.5 m v^2.
// Same streaming structure as K1 (two targets per lane in packed registers, wave-private LDS-DMA
// chunks, J-split over waves and slabs) restricted to the upper triangle: a target group only
// walks the source chunks at or above its own first index; the (at most three) chunks that
// straddle the diagonal take the masked path (j > i), the rest run mask-free. Per pair
// 8 packed ops + 1 v_mov + 2 v_sqrt_f32 + 2 v_rcp_f32. fp32 per-lane partial sums, fp64 across lanes/blocks.
template <bool MASKED>
__device__ __forceinline__ void energy_pair(const f4 p, const f2 xi, const f2 yi, const f2 zi, const f2 soft,
                                            f2& u, int j, int i0, int i1, int n) {
  const f2 dx = f2{p.x, p.x} - xi, dy = f2{p.y, p.y} - yi, dz = f2{p.z, p.z} - zi;
  f2 d2 = dx * dx;
  d2 = __builtin_elementwise_fma(dy, dy, d2);
  d2 = __builtin_elementwise_fma(dz, dz, d2);
  const f2 den = f2{__builtin_amdgcn_sqrtf(d2.x), __builtin_amdgcn_sqrtf(d2.y)} + soft;   // |r| + eps (:105)
  const f2 inv = {__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
  f2 t = f2{p.w, p.w} * inv;                  // m_j / den (plain C: the consumer of v_rcp_f32 must be
                                              // visible to hipcc's hazard padding -- see interact())
  if (MASKED) {                               // triu(1): strictly above the diagonal (:113)
    t.x = (j > i0 && j < n) ? t.x : 0.f;
    t.y = (j > i1 && j < n) ? t.y : 0.f;
  }
  u += t;
}

// The wave body of the potential-energy kernels: targets [t_base, t_base + 128) of the n bodies in posm against this
// workgroup's share of the chunks [first chunk of the group, n_chunks), split over slabs x 4 waves; the diagonal chunks
// and the padded tail (every chunk when all_masked: no softening) take the masked pair. *dst = the workgroup's
// sum_i m_i u_i in fp64 (the -G factor is applied by the final kernel). lds: the workgroup's f4[kEnergyLdsF4].
constexpr int kEnergyLdsF4 = kWaves * 2 * kChunk + 8;

__device__ __forceinline__ void energy_body(const f4* __restrict__ posm, int n, int n_chunks, int t_base, int slab,
                                            int slabs, float soft_, const bool all_masked, f4* lds,
                                            double* __restrict__ dst) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i0 = t_base + lane, i1 = t_base + 64 + lane;
  const f4 t0 = posm[min(i0, n - 1)], t1 = posm[min(i1, n - 1)];
  const f2 xi = {t0.x, t1.x}, yi = {t0.y, t1.y}, zi = {t0.z, t1.z};
  f2 u = {0.f, 0.f};
  f2 soft = {soft_, soft_};
  asm volatile("" : "+v"(soft));
  const int c_lo = t_base / kChunk;
  const int span = n_chunks - c_lo;
  const int parts = slabs * kWaves;
  const int cpw = (span + parts - 1) / parts;
  const int jw = slab * kWaves + wave;
  const int c_begin = min(c_lo + jw * cpw, n_chunks), c_end = min(c_begin + cpw, n_chunks);
  const int c_diag_end = (t_base + kTgtPerWG + kChunk - 1) / kChunk;      // chunks below this touch j <= i
  f4* stage = &lds[wave * 2 * kChunk];
  const f4* s_lane = posm + lane;
  if (c_begin < c_end)
    __builtin_amdgcn_global_load_lds(GPTR(s_lane + (size_t)c_begin * kChunk), LPTR(stage), 16, 0, 0);
  for (int c = c_begin; c < c_end; ++c) {
    const int b = (c - c_begin) & 1;
    if (c + 1 < c_end) {
      __builtin_amdgcn_global_load_lds(GPTR(s_lane + (size_t)(c + 1) * kChunk), LPTR(stage + (b ^ 1) * kChunk), 16, 0, 0);
      asm volatile("s_waitcnt vmcnt(1)" ::: "memory");  // chunk c has landed, c+1 in flight
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const f4* buf = stage + b * kChunk;
    const int j0 = c * kChunk;
    if (all_masked || c < c_diag_end || c == n_chunks - 1) {     // diagonal chunks and the padded tail
#pragma unroll 4
      for (int j = 0; j < kChunk; ++j) energy_pair<true>(buf[j], xi, yi, zi, soft, u, j0 + j, i0, i1, n);
    } else {
#pragma unroll 4
      for (int j = 0; j < kChunk; ++j) energy_pair<false>(buf[j], xi, yi, zi, soft, u, j0 + j, i0, i1, n);
    }
  }
  double acc = 0.0;
  if (i0 < n) acc += (double)t0.w * (double)u.x;
  if (i1 < n) acc += (double)t1.w * (double)u.y;
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  double* red = reinterpret_cast<double*>(&lds[kWaves * 2 * kChunk]);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) *dst = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- per-body potential of the softening the FORCE uses (csrc/direct_diag.hip): u_i = sum_{j != i} m_j (|r_ij|^2 + eps^2)^(-1/2),
// the sum whose gradient interact() evaluates (energy_pair above is the reference's |r| + eps instead). One source
// against the lane's two targets: exact fp32 differences, fma for r^2 + eps^2, v_rsq_f32, fma with m_j -- 5 packed ops
// + 2 v_rsq_f32. MASKED drops j == i and the padding by index (the i == j term is m_i / eps, not 0, so it can never be
// left to the arithmetic); un-masked, a padding entry (m = 0) adds 0 exactly as long as eps^2 >= kEps2Masked keeps s
// finite. Coincident distinct bodies at eps = 0 give +inf here (phi = -inf).
template <bool MASKED>
__device__ __forceinline__ void potential_pair(const f4 p, const f2 xi, const f2 yi, const f2 zi, const f2 e2, f2& u,
                                               int j, int i0, int i1, int n_src) {
  const f2 dx = f2{p.x, p.x} - xi, dy = f2{p.y, p.y} - yi, dz = f2{p.z, p.z} - zi;
  f2 r2 = __builtin_elementwise_fma(dx, dx, e2);
  r2 = __builtin_elementwise_fma(dy, dy, r2);
  r2 = __builtin_elementwise_fma(dz, dz, r2);
  f2 s = {__builtin_amdgcn_rsqf(r2.x), __builtin_amdgcn_rsqf(r2.y)};
  if (MASKED) {
    s.x = (j < n_src && j != i0) ? s.x : 0.0f;
    s.y = (j < n_src && j != i1) ? s.y : 0.0f;
  }
  u = __builtin_elementwise_fma(f2{p.w, p.w}, s, u);      // plain C consumer of v_rsq_f32 (see interact())
}

// The wave body of the potential kernels. Geometry as accel_body: 4 waves on the 128 targets tgt[t_base ..] (global index
// tgt_off + row), wave jw = slab * 4 + w walks the chunks [jw*q + min(jw, r), ... + q (+1 if jw < r)) of the n_chunks
// source chunks, q = n_chunks / (slabs * 4), r the remainder, each chunk through the double-buffered LDS-DMA stage. The
// chunks that hold one of the group's own indices take the masked pair (every chunk when all_masked: eps^2 < kEps2Masked).
// Precision: an fp32 sum never runs past one chunk (64 terms of one sign); the chunk sums are added in fp64, in chunk
// order, then the four waves as (w0 + w1) + (w2 + w3) through LDS. dst[row] = this slab's fp64 partial for the valid
// rows of the group (no G, no sign: the finishing pass adds the slabs in slab order). lds: the workgroup's f4[kPotLdsF4].
constexpr int kPotLdsF4 = kWaves * 2 * kChunk + kWaves * 2 * 64 / 2;

__device__ __forceinline__ void potential_body(const f4* __restrict__ src, int n_src, int n_chunks, int slabs,
                                               const bool all_masked, const f4* __restrict__ tgt, int n_tgt, int tgt_off,
                                               int t_base, int slab, float eps2, f4* lds, double* __restrict__ dst) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i0 = t_base + lane, i1 = t_base + 64 + lane;
  const f4 t0 = tgt[min(i0, n_tgt - 1)], t1 = tgt[min(i1, n_tgt - 1)];
  const f2 xi = {t0.x, t1.x}, yi = {t0.y, t1.y}, zi = {t0.z, t1.z};
  f2 e2 = {eps2, eps2};
  asm volatile("" : "+v"(e2));  // keep eps^2 in VGPRs: an SGPR operand halves v_pk_fma issue
  double phi0 = 0.0, phi1 = 0.0;

  const int parts = slabs * kWaves, cpw_q = n_chunks / parts, cpw_r = n_chunks % parts;
  const int jw = slab * kWaves + wave;
  const int c_begin = jw * cpw_q + min(jw, cpw_r), c_end = c_begin + cpw_q + (jw < cpw_r ? 1 : 0);
  const int g_lo = tgt_off + t_base, g_hi = g_lo + kTgtPerWG;      // the group's own source indices
  f4* stage = &lds[wave * 2 * kChunk];
  const f4* s_lane = src + lane;
  if (c_begin < c_end)
    __builtin_amdgcn_global_load_lds(GPTR(s_lane + (size_t)c_begin * kChunk), LPTR(stage), 16, 0, 0);
  for (int c = c_begin; c < c_end; ++c) {
    const int b = (c - c_begin) & 1;
    if (c + 1 < c_end) {
      __builtin_amdgcn_global_load_lds(GPTR(s_lane + (size_t)(c + 1) * kChunk), LPTR(stage + (b ^ 1) * kChunk), 16, 0, 0);
      asm volatile("s_waitcnt vmcnt(1)" ::: "memory");  // chunk c has landed, c+1 in flight
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const f4* buf = stage + b * kChunk;
    const int j0 = c * kChunk;
    f2 u = {0.f, 0.f};
    if (all_masked || (j0 < g_hi && j0 + kChunk > g_lo)) {
#pragma unroll 4
      for (int j = 0; j < kChunk; ++j)
        potential_pair<true>(buf[j], xi, yi, zi, e2, u, j0 + j, tgt_off + i0, tgt_off + i1, n_src);
    } else {
#pragma unroll 8
      for (int j = 0; j < kChunk; ++j) potential_pair<false>(buf[j], xi, yi, zi, e2, u, j0 + j, 0, 0, n_src);
    }
    phi0 += (double)u.x;
    phi1 += (double)u.y;
  }

  double* red = reinterpret_cast<double*>(&lds[kWaves * 2 * kChunk]);  // [wave][half][64]
  red[(wave * 2 + 0) * 64 + lane] = phi0;
  red[(wave * 2 + 1) * 64 + lane] = phi1;
  __syncthreads();
  const int n_valid = min(kTgtPerWG, n_tgt - t_base);
  if ((int)threadIdx.x < n_valid) {
    const double* r = red + threadIdx.x;          // row lt = half * 64 + lane sits at [wave][lt]
    dst[threadIdx.x] = (r[0] + r[2 * 64]) + (r[4 * 64] + r[6 * 64]);
  }
}

// ---- conserved quantities (csrc/direct_diag.hip from the fp32 state, csrc/direct_hermite_f64.hip from an fp64 one).
// The body of the invariants kernels: the workgroup's 1024 threads over the n bodies of one system -- state(i, m, x, v)
// gives body i's mass, position and velocity as doubles -- and phi (n); row = {M, C (3), P (3), L (3), K, U, E, Q, 0, 0}.
// Thread t sums bodies t, t + 1024, ... in index order, then a shuffle tree per wave and the 16 wave sums in wave order.
// C = 0 when M = 0, Q = 0 when U = 0.
constexpr int kInvThreads = 1024;            // one workgroup per system: 16 waves
constexpr int kInvWaves = kInvThreads / 64;
constexpr int kInvSums = 12;                 // M, m x (3), m v (3), m x cross v (3), K, sum m phi

template <class State>
__device__ __forceinline__ void invariants_body(const State state, const double* __restrict__ phi, int n,
                                                double* __restrict__ row, double (*red)[kInvWaves]) {
  double a[kInvSums];
#pragma unroll
  for (int q = 0; q < kInvSums; ++q) a[q] = 0.0;
  for (int i = threadIdx.x; i < n; i += kInvThreads) {
    double m, xs[3], vs[3];
    state(i, m, xs, vs);
    const double x = xs[0], y = xs[1], z = xs[2], vx = vs[0], vy = vs[1], vz = vs[2];
    a[0] += m;
    a[1] += m * x; a[2] += m * y; a[3] += m * z;
    a[4] += m * vx; a[5] += m * vy; a[6] += m * vz;
    a[7] += m * (y * vz - z * vy); a[8] += m * (z * vx - x * vz); a[9] += m * (x * vy - y * vx);
    a[10] += 0.5 * m * ((vx * vx + vy * vy) + vz * vz);
    a[11] += m * phi[i];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < kInvSums; ++q) {
    for (int off = 32; off > 0; off >>= 1) a[q] += __shfl_down(a[q], off);
    if (lane == 0) red[q][wave] = a[q];
  }
  __syncthreads();
  if (threadIdx.x < kInvSums) {
    double s = red[threadIdx.x][0];
    for (int w = 1; w < kInvWaves; ++w) s += red[threadIdx.x][w];
    red[threadIdx.x][0] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double M = red[0][0], K = red[10][0], U = 0.5 * red[11][0];
    row[0] = M;
    for (int q = 1; q <= 3; ++q) row[q] = M != 0.0 ? red[q][0] / M : 0.0;
    for (int q = 4; q <= 9; ++q) row[q] = red[q][0];
    row[10] = K; row[11] = U; row[12] = K + U;
    row[13] = U != 0.0 ? -2.0 * K / U : 0.0;
    row[14] = 0.0; row[15] = 0.0;
  }
}

}  // namespace
