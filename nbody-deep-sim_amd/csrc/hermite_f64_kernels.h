// hermite_f64_kernels.h -- what the double-precision translation units share (direct_hermite_f64.hip: all targets,
// shared timestep, and the diagnostics; direct_hermite_block_f64.hip: an active list of targets, block timesteps;
// direct_batch_hermite_block_f64.hip: the active lists of every scene of a batch;
// direct_hermite_shard_f64.hip: one rank's bodies of a range partition, 4th and 6th order;
// direct_batch_hermite_f64.hip: many independent systems, shared timestep per system, and their diagnostics;
// direct_leapfrog_f64.hip: the acceleration alone, for the leapfrog and Euler steps; direct_grad.hip and direct_hermite_grad.hip: the float64 backward kernels): the reciprocal
// square root (rsqrt_f64), the pair functors (AccelJerkPair: acceleration plus jerk; AccelPair: its acceleration alone;
// PotentialPair, EnergyPair: the diagnostics), the finishing sums of the diagnostics (potential_finish_f64,
// energy_finish_f64, F64State), the wave body that walks the source chunks with a functor (walk_f64), the prologue of a
// kernel that calls it (Group64: the workgroup's targets, the wave's place in the chunk split, the slab destination;
// wave_chunks_upper: the upper-triangle chunk range of the energies) and the geometry of a pair launch (F64Plan,
// plan_f64). As in hermite_kernels.h there is one copy of every rounded operation and of every prologue line: a block
// step whose active list is every body, a rank that owns every body, or a scene of a batch, has the shared step's bits
// because the kernels are the same Group64 and a call of the same walk_f64.
// The definitions sit in an anonymous namespace: every translation unit that includes this file gets its own inlined copies.
#pragma once
#include "direct_kernels.h"
#include "hermite_kernels.h"

namespace {

constexpr int kTgtF64 = 64;                      // targets per workgroup: one per lane, = one source chunk
constexpr int kRowQuads = 2;                     // 16-byte LDS-DMA pieces per 32-byte row
constexpr int kChunkQuads = kChunk * kRowQuads;  // 128 quads = 2 KiB per chunk and array
constexpr double kEps2MaskedF64 = 1e-24;         // the fp32 kernels' rule (kEps2Masked): below it i == j goes by index
constexpr int kTargetWGs = 1024;                 // ~4 workgroups per CU (32 KiB of LDS each: at most 5 fit)
constexpr int kNoBody = 0x7fffffff;              // a source index that is behind every n and is no target's own

// x^(-1/2) to about 1 ulp. y0 = v_rsq_f64 (a compiler builtin: hipcc pads the transcendental -> VALU wait state for its
// consumers). With h = 1 - x y^2 formed by one fma from the rounded x y (its absolute error is 2^-53, and h is what the
// correction is proportional to): y1 = y0 (1 + h/2 + 3 h^2/8) leaves O(h^3), y2 = y1 (1 + h/2) squares that.
__device__ __forceinline__ double rsqrt_f64(const double x) {
  const double y0 = __builtin_amdgcn_rsq(x);
  double t = x * y0;
  double h = __builtin_fma(-t, y0, 1.0);
  const double y1 = __builtin_fma(y0 * h, __builtin_fma(0.375, h, 0.5), y0);
  t = x * y1;
  h = __builtin_fma(-t, y1, 1.0);
  return __builtin_fma(0.5 * y1, h, y1);
}

// ---- the pair functors. A functor holds its lane's target and partial sums; pair<MASKED>(p, q, j) adds source j (row p
// of posd, row q of veld where kVel; with kStreams = 3, pair<MASKED>(p, q, r, j) with row r of a third array) -- MASKED:
// exclusions by index, else by the arithmetic; out(k) is partial sum k of kOut.

// a_i = sum_j m_j r_ij s^3, j_i = sum_j m_j (v_ij s^3 - 3 (r_ij.v_ij) s^5 r_ij), s = (|r_ij|^2 + eps^2)^(-1/2): the
// operations of AccelJerkPolicy::masked / ::block (hermite_kernels.h) one for one. acc[3..5] accumulates w dv, acc[6..8]
// (r.v s^2) w dr; j = acc[3..5] - 3 acc[6..8]. MASKED drops j == i and the padding behind n by a select on s (after the
// refinement: whatever the dropped r^2 gave, NaN included, never reaches a sum). Un-masked, i == j and a padding row add
// exact zeros: dr = dv = 0 resp. m = 0, with s finite because eps^2 >= kEps2MaskedF64.
struct AccelJerkPair {
  static constexpr bool kVel = true;
  static constexpr int kOut = 6;
  double xi, yi, zi, ui, vi, wi, e2;
  double acc[9];
  int i, n;

  __device__ __forceinline__ AccelJerkPair(const d4 tp, const d4 tv, double eps2, int i_, int n_)
      : xi(tp.x), yi(tp.y), zi(tp.z), ui(tv.x), vi(tv.y), wi(tv.z), e2(eps2), i(i_), n(n_) {
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
  }

  template <bool MASKED>
  __device__ __forceinline__ void pair(const d4 p, const d4 q, int j) {
    const double dx = p.x - xi, dy = p.y - yi, dz = p.z - zi;      // r_j - r_i
    const double du = q.x - ui, dv = q.y - vi, dw = q.z - wi;
    double r2 = __builtin_fma(dx, dx, e2);
    r2 = __builtin_fma(dy, dy, r2);
    r2 = __builtin_fma(dz, dz, r2);
    double rv = dx * du;
    rv = __builtin_fma(dy, dv, rv);
    rv = __builtin_fma(dz, dw, rv);
    double s = rsqrt_f64(r2);
    if (MASKED) s = (j < n && j != i) ? s : 0.0;
    const double s2 = s * s;
    const double w = (s2 * s) * p.w;
    const double c = (rv * s2) * w;
    acc[0] = __builtin_fma(w, dx, acc[0]);
    acc[1] = __builtin_fma(w, dy, acc[1]);
    acc[2] = __builtin_fma(w, dz, acc[2]);
    acc[3] = __builtin_fma(w, du, acc[3]);
    acc[4] = __builtin_fma(w, dv, acc[4]);
    acc[5] = __builtin_fma(w, dw, acc[5]);
    acc[6] = __builtin_fma(c, dx, acc[6]);
    acc[7] = __builtin_fma(c, dy, acc[7]);
    acc[8] = __builtin_fma(c, dz, acc[8]);
  }

  __device__ __forceinline__ double out(int k) const { return k < 3 ? acc[k] : acc[k] - 3.0 * acc[k + 3]; }
};

// a_i = sum_j m_j r_ij s^3 alone (direct_leapfrog_f64.hip): AccelJerkPair::pair's operations for acc[0..2], one for one
// and in the same order, so the sums are that functor's bits; no velocity row is loaded and no second array streamed.
struct AccelPair {
  static constexpr bool kVel = false;
  static constexpr int kOut = 3;
  double xi, yi, zi, e2;
  double acc[3];
  int i, n;

  __device__ __forceinline__ AccelPair(const d4 tp, double eps2, int i_, int n_)
      : xi(tp.x), yi(tp.y), zi(tp.z), e2(eps2), acc{0.0, 0.0, 0.0}, i(i_), n(n_) {}

  template <bool MASKED>
  __device__ __forceinline__ void pair(const d4 p, const d4, int j) {
    const double dx = p.x - xi, dy = p.y - yi, dz = p.z - zi;      // r_j - r_i
    double r2 = __builtin_fma(dx, dx, e2);
    r2 = __builtin_fma(dy, dy, r2);
    r2 = __builtin_fma(dz, dz, r2);
    double s = rsqrt_f64(r2);
    if (MASKED) s = (j < n && j != i) ? s : 0.0;
    const double s2 = s * s;
    const double w = (s2 * s) * p.w;
    acc[0] = __builtin_fma(w, dx, acc[0]);
    acc[1] = __builtin_fma(w, dy, acc[1]);
    acc[2] = __builtin_fma(w, dz, acc[2]);
  }

  __device__ __forceinline__ double out(int k) const { return acc[k]; }
};

// ---- the pair functors of the diagnostics

// u_i = sum_{j != i} m_j (|r_ij|^2 + eps^2)^(-1/2): potential_pair (direct_kernels.h) in fp64. The i == j term is
// m_i / eps, never a zero: the chunk that holds the group's own indices is always walked MASKED.
struct PotentialPair {
  static constexpr bool kVel = false;
  static constexpr int kOut = 1;
  double xi, yi, zi, e2, u;
  int i, n;

  __device__ __forceinline__ PotentialPair(const d4 tp, double eps2, int i_, int n_)
      : xi(tp.x), yi(tp.y), zi(tp.z), e2(eps2), u(0.0), i(i_), n(n_) {}

  template <bool MASKED>
  __device__ __forceinline__ void pair(const d4 p, const d4, int j) {
    const double dx = p.x - xi, dy = p.y - yi, dz = p.z - zi;
    double r2 = __builtin_fma(dx, dx, e2);
    r2 = __builtin_fma(dy, dy, r2);
    r2 = __builtin_fma(dz, dz, r2);
    double s = rsqrt_f64(r2);
    if (MASKED) s = (j < n && j != i) ? s : 0.0;
    u = __builtin_fma(p.w, s, u);
  }

  __device__ __forceinline__ double out(int) const { return u; }
};

// u_i = sum_{j > i} m_j / (|r_ij| + eps), the reference's convention (energy_pair, direct_kernels.h): the square root and
// the quotient are the compiler's fp64 expansions (correctly rounded; |r| = 0 is an ordinary input to them). Always by
// index (j > i and j < n): the kernel walks it MASKED in every chunk.
struct EnergyPair {
  static constexpr bool kVel = false;
  static constexpr int kOut = 1;
  double xi, yi, zi, soft, u;
  int i, n;

  __device__ __forceinline__ EnergyPair(const d4 tp, double soft_, int i_, int n_)
      : xi(tp.x), yi(tp.y), zi(tp.z), soft(soft_), u(0.0), i(i_), n(n_) {}

  template <bool MASKED>
  __device__ __forceinline__ void pair(const d4 p, const d4, int j) {
    const double dx = p.x - xi, dy = p.y - yi, dz = p.z - zi;
    double d2 = dx * dx;
    d2 = __builtin_fma(dy, dy, d2);
    d2 = __builtin_fma(dz, dz, d2);
    const double t = p.w / (__builtin_sqrt(d2) + soft);
    u += (j > i && j < n) ? t : 0.0;
  }

  __device__ __forceinline__ double out(int) const { return u; }
};

// ---- the finishing sums of the diagnostics: the bodies of direct_hermite_f64.hip's finishing kernels (one system) and of
// direct_batch_hermite_f64.hip's (one scene of a batch)

constexpr int kSumThreads = 1024;                // the one-workgroup sums (energy_finish_f64): 16 waves
constexpr int kSumWaves = kSumThreads / 64;

// phi_i = -G (slab 0 + slab 1 + ...) in slab order (0 - G sum: a body without partners gets +0)
__device__ __forceinline__ double potential_finish_f64(const double* __restrict__ slabs, int n_slabs, int n, int i,
                                                       double g) {
  double sum;
  slab_order_sum<1>(slabs, n_slabs, (size_t)n, (size_t)i, &sum);
  return 0.0 - g * sum;
}

// {U, K} = {-G sum_i m_i u_i, sum_i 1/2 m_i |v_i|^2}, u_i = the slabs in slab order: one workgroup of kSumThreads, thread
// t over the bodies t, t + 1024, ... in index order, then a shuffle tree per wave and the 16 wave sums in wave order.
__device__ __forceinline__ void energy_finish_f64(const double* __restrict__ slabs, int n_slabs, int n,
                                                  const d4* __restrict__ posd, const double* __restrict__ vel, double g,
                                                  double* __restrict__ out_uk, double (*red)[kSumWaves]) {
  double a[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < n; i += kSumThreads) {
    double u;
    slab_order_sum<1>(slabs, n_slabs, (size_t)n, (size_t)i, &u);
    const double m = posd[i].w;
    const double vx = vel[3 * (size_t)i], vy = vel[3 * (size_t)i + 1], vz = vel[3 * (size_t)i + 2];
    a[0] += m * u;
    a[1] += 0.5 * m * ((vx * vx + vy * vy) + vz * vz);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    for (int off = 32; off > 0; off >>= 1) a[q] += __shfl_down(a[q], off);
    if (lane == 0) red[q][wave] = a[q];
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double s = red[threadIdx.x][0];
    for (int w = 1; w < kSumWaves; ++w) s += red[threadIdx.x][w];
    out_uk[threadIdx.x] = threadIdx.x == 0 ? 0.0 - g * s : s;
  }
}

// A body of the fp64 state for invariants_body (direct_kernels.h)
struct F64State {
  const double* __restrict__ pos;
  const double* __restrict__ vel;
  const double* __restrict__ mass;
  __device__ __forceinline__ void operator()(int i, double& m, double* x, double* v) const {
    m = mass[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      x[k] = pos[3 * (size_t)i + k];
      v[k] = vel[3 * (size_t)i + k];
    }
  }
};

// LDS of a workgroup, in 16-byte quads: [wave][buffer][pos (| vel)][128]
template <bool VEL>
constexpr int stage_quads() { return 2 * (VEL ? 2 : 1) * kChunkQuads; }

// ... and with NS arrays streamed: [wave][buffer][array][128]
template <int NS>
constexpr int stage_quads_n() { return 2 * NS * kChunkQuads; }

// The arrays a functor streams per source: kVel ? 2 : 1, or the functor's own kStreams (3: direct_hermite_grad.hip's
// {x, m}, {v, 0} and a cotangent row; pair<MASKED>(p, q, r, j) then takes the third row after the second).
template <class Pair, class = void>
struct PairStreams { static constexpr int value = Pair::kVel ? 2 : 1; };
template <class Pair>
struct PairStreams<Pair, decltype((void)Pair::kStreams)> { static constexpr int value = Pair::kStreams; };

// The wave body. The wave walks the chunks [c_begin, c_end) of posd (and veld): chunk c = rows [64 c, 64 c + 64), 2 KiB per
// array, fetched as two 1-KiB LDS-DMA pieces (lane l brings quads l and 64 + l of the chunk, so the rows land as they lie
// in memory), the next chunk in flight while this one is used. all_masked, or the chunk own_chunk (the one that holds the
// group's own indices; -1 for gathered targets, which have none), takes pair<true>, every other chunk pair<false>. Then
// the 4 waves' kOut partials per lane go through LDS -- a wave's staging is free after its last chunk: its loads have
// landed and its reads precede these writes -- and are added in wave order into dst[k * stride + t], t < n_valid.
// A functor with kStreams = 3 (PairStreams above) streams `third` as well: two more loads per chunk, [pos | vel | third][128]
// staging, the counted wait at six loads; with RANGE the edge chunks put three zero rows in for an excluded source.
// Compile-time shape, the defaults = two arrays of 32-byte rows, every chunk where it lies:
//   RQ    : 16-byte quads from one source row to the next. 2: posd and veld as above. 4: ONE array of 64-byte rows
//           {x, y, z, m, vx, vy, vz, 0} (veld = posd + 2 quads), what a range-sharded rank sends and gathers
//           (direct_hermite_shard_f64.hip). Lane l then brings quad l & 1 of the rows l >> 1 and 32 + (l >> 1) of the
//           chunk, the velocity quads two further on: the chunk lands in the same [pos | vel][128] image either way, and
//           the pair loops do not know the difference. 6 (three arrays only): ONE array of 96-byte rows
//           {x, y, z, m | vx, vy, vz, 0 | ax, ay, az, 0} (veld = posd + 2 quads, third = posd + 4 quads), the 6th-order
//           rank's row (the same unit): the same lane mapping at a six-quad row stride, the second piece
//           kChunk * RQ / 2 quads on, into the same [pos | vel | third][128] image; the counted wait stays vmcnt(6).
//   RANGE : the walk is over the view *sv (direct_kernels.h): [c_begin, c_end) are LOGICAL chunks that hop over the run of
//           physical chunks lying wholly inside [ex_lo, ex_hi), and the (at most two) chunks that straddle an end of that
//           range take pair<true> with the range mask: a source inside the range goes in as a zero row with an index no
//           body has (a select on the row and on j: whatever such a row holds, NaN included, never reaches a sum). own_chunk
//           and the index a pair is given are physical.
template <class Pair, int RQ = kRowQuads, bool RANGE = false>
__device__ __forceinline__ void walk_f64(Pair& pr, const d4* __restrict__ posd, const d4* __restrict__ veld, int c_begin,
                                         int c_end, bool all_masked, int own_chunk, f4* lds, double* __restrict__ dst,
                                         size_t stride, int n_valid, const SrcView* sv = nullptr,
                                         const d4* __restrict__ third = nullptr) {
  constexpr int kArr = PairStreams<Pair>::value;
  constexpr bool VEL = kArr >= 2;
  static_assert(kArr >= 1 && kArr <= 3, "one to three streamed arrays");
  static_assert(kArr < 3 || (RQ == kRowQuads && !RANGE) || RQ == 3 * kRowQuads,
                "three arrays: un-sharded 32-byte rows, or {pos, vel, third} rows");
  constexpr int kSrcQuads = kChunk * RQ;           // quads from one chunk to the next in memory
  constexpr int kPiece = kSrcQuads / 2;            // and from the first LDS-DMA piece of a chunk to the second
  static_assert(RQ == kRowQuads || (RQ == 2 * kRowQuads && kArr < 3) || (RQ == 3 * kRowQuads && kArr == 3),
                "rows of posd / veld / third, {pos, vel} rows, or {pos, vel, third} rows");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  f4* stage = &lds[wave * stage_quads_n<kArr>()];
  const int lane_quad = RQ == kRowQuads ? lane : (lane >> 1) * RQ + (lane & 1);
  const f4* p_lane = reinterpret_cast<const f4*>(posd) + lane_quad;
  const f4* v_lane = reinterpret_cast<const f4*>(veld) + lane_quad;
  const f4* b_lane = reinterpret_cast<const f4*>(third) + lane_quad;
  // logical -> physical chunk: hop over the skipped run
  auto phys = [&](int c) { return RANGE ? c + (c >= sv->skip_c0 ? sv->skip_cn : 0) : c; };
  auto fetch = [&](int c, int b) {
    const size_t at = (size_t)phys(c) * kSrcQuads;
    f4* to = stage + b * kArr * kChunkQuads;
    __builtin_amdgcn_global_load_lds(GPTR(p_lane + at), LPTR(to), 16, 0, 0);
    __builtin_amdgcn_global_load_lds(GPTR(p_lane + at + kPiece), LPTR(to + 64), 16, 0, 0);
    if (VEL) {
      __builtin_amdgcn_global_load_lds(GPTR(v_lane + at), LPTR(to + kChunkQuads), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(GPTR(v_lane + at + kPiece), LPTR(to + kChunkQuads + 64), 16, 0, 0);
    }
    if constexpr (kArr == 3) {
      __builtin_amdgcn_global_load_lds(GPTR(b_lane + at), LPTR(to + 2 * kChunkQuads), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(GPTR(b_lane + at + kPiece), LPTR(to + 2 * kChunkQuads + 64), 16, 0, 0);
    }
  };
  if (c_begin < c_end) fetch(c_begin, 0);
  for (int c = c_begin; c < c_end; ++c) {
    const int b = (c - c_begin) & 1;
    if (c + 1 < c_end) {
      fetch(c + 1, b ^ 1);
      // chunk c has landed, c + 1 (2 loads per array) in flight
      if constexpr (kArr == 3) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      else if (VEL) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const d4* bp = reinterpret_cast<const d4*>(stage + b * kArr * kChunkQuads);
    const d4* bv = VEL ? bp + kChunk : bp;
    const int pc = phys(c);
    const int j0 = pc * kChunk;
    if constexpr (kArr == 3) {
      const d4* bb = bv + kChunk;
      if (RANGE && (pc == sv->edge0 || pc == sv->edge1)) {
        const d4 none = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
        for (int j = 0; j < kChunk; ++j) {
          const bool ex = (unsigned)(j0 + j - sv->ex_lo) < (unsigned)(sv->ex_hi - sv->ex_lo);
          pr.template pair<true>(ex ? none : bp[j], ex ? none : bv[j], ex ? none : bb[j], ex ? kNoBody : j0 + j);
        }
      } else if (all_masked || pc == own_chunk) {
#pragma unroll 2
        for (int j = 0; j < kChunk; ++j) pr.template pair<true>(bp[j], bv[j], bb[j], j0 + j);
      } else {
#pragma unroll 2
        for (int j = 0; j < kChunk; ++j) pr.template pair<false>(bp[j], bv[j], bb[j], j0 + j);
      }
    } else if (RANGE && (pc == sv->edge0 || pc == sv->edge1)) {
      const d4 none = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
      for (int j = 0; j < kChunk; ++j) {
        const bool ex = (unsigned)(j0 + j - sv->ex_lo) < (unsigned)(sv->ex_hi - sv->ex_lo);
        pr.template pair<true>(ex ? none : bp[j], ex ? none : bv[j], ex ? kNoBody : j0 + j);
      }
    } else if (all_masked || pc == own_chunk) {
#pragma unroll 2
      for (int j = 0; j < kChunk; ++j) pr.template pair<true>(bp[j], bv[j], j0 + j);
    } else {
#pragma unroll 4
      for (int j = 0; j < kChunk; ++j) pr.template pair<false>(bp[j], bv[j], j0 + j);
    }
  }

  constexpr int kPart = stage_quads_n<kArr>() * 2;                     // doubles per wave; [k][64] in the first kOut * 64
  static_assert(Pair::kOut * 64 <= kPart, "the partials must fit a wave's staging");
  double* red = reinterpret_cast<double*>(lds);
#pragma unroll
  for (int k = 0; k < Pair::kOut; ++k) red[wave * kPart + k * 64 + lane] = pr.out(k);
  __syncthreads();
  for (int o = threadIdx.x; o < Pair::kOut * 64; o += 64 * kWaves) {
    const int k = o >> 6, t = o & 63;
    if (t >= n_valid) continue;
    double sum = red[o];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) sum += red[w * kPart + o];
    dst[(size_t)k * stride + t] = sum;
  }
}

// The prologue of every walk_f64 kernel: Group128 (hermite_kernels.h) with one target per lane, i (behind n it repeats
// row n - 1 and stores nothing). One copy of these lines is what keeps a scene of a batch, or a rank that owns every
// body, on the one-system kernel's geometry. A kernel is then: the group, the wave's chunks (wave_chunks /
// wave_chunks_of, hermite_kernels.h, or wave_chunks_upper), the pair functor, one walk_f64.
template <class I>
struct Group64 {
  I slab;
  int n, t_base, i;

  __device__ __forceinline__ Group64(I grp, I slab_, int n_)
      : slab(slab_), n(n_), t_base(grp * kTgtF64), i(t_base + (threadIdx.x & 63)) {}
  __device__ __forceinline__ int row() const { return min(i, n - 1); }
  __device__ __forceinline__ int jw() const { return slab * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }
  __device__ __forceinline__ int n_valid() const { return min(kTgtF64, n - t_base); }
  // the group's place in the slab of base = double[slabs][Pair::kOut][n]: walk_f64's dst (with stride n)
  template <class Pair>
  __device__ __forceinline__ double* dst(double* __restrict__ base) const {
    return base + (size_t)slab * Pair::kOut * n + t_base;
  }
};

// The chunks of wave jw in the upper triangle (the pair energies): group grp needs the chunks [grp, n_chunks) only, chunk
// grp being its own rows. The balanced split of that span over slabs x 4 waves, COUNTED FROM grp: the kernel walks
// [grp + begin, grp + end). (The sum is left to the kernel: formed here, the compiler orders the additions of grp + end
// another way than the kernels had.) I: as in Group64.
template <class I>
__device__ __forceinline__ ChunkRange wave_chunks_upper(int jw, int n_chunks, I grp, I slabs) {
  const int span = n_chunks - (int)grp, parts = slabs * kWaves;
  return wave_chunks(jw, span / parts, span % parts);
}

// The geometry of a pair launch: groups of 64 targets, and enough slabs for ~kTargetWGs workgroups as long as every wave
// of a slab still has a chunk to walk. n_tgt targets under n sources; n_tgt = n is the shared step's plan.
struct F64Plan { int groups, slabs, n_chunks; };

// the slab count of `groups` target groups under n_chunks source chunks (at least 1: a wave may then be left without one).
// On the device too: a scene of a batched block step (direct_batch_hermite_block_f64.hip) forms it from its own active count.
__host__ __device__ inline int slabs_f64(int groups, int n_chunks) {
  int slabs = ceil_div(kTargetWGs, groups);
  const int cap = n_chunks / kWaves;
  slabs = slabs > cap ? cap : slabs;
  slabs = slabs > kMaxSlabs ? kMaxSlabs : slabs;
  return slabs < 1 ? 1 : slabs;
}

inline F64Plan plan_f64(int n, int n_tgt) {
  F64Plan p;
  p.n_chunks = ceil_div(n, kChunk);
  p.groups = ceil_div(n_tgt, kTgtF64);
  p.slabs = slabs_f64(p.groups, p.n_chunks);
  return p;
}

inline F64Plan plan_f64(int n) { return plan_f64(n, n); }

// The geometry of a range-sharded rank's two force launches (direct_hermite_shard_f64.hip, the same for the 4th and the
// 6th order) as an HShardPlan (hermite_kernels.h). The local block is plan_f64(n_local); the remote block has the same target
// groups and slabs_f64's count for its logical chunks (none, and no launch, where the rank owns every body). An explicit
// slab count in [1, kMaxSlabs] replaces either. The view's chunk counts come from n_total: no logical chunk maps behind
// the padded length of the gathered array.
inline bool slab_arg_ok(int slabs) { return slabs >= 0 && slabs <= kMaxSlabs; }

// n_local > 0; slabs_local, slabs_remote: 0 = the plan's
inline HShardPlan plan_hshard_f64(int n_total, int lo, int n_local, int slabs_local, int slabs_remote) {
  HShardPlan p;
  const F64Plan local = plan_f64(n_local);
  p.groups = local.groups;
  p.chunks_local = local.n_chunks;
  p.slabs_local = slabs_local ? slabs_local : local.slabs;
  p.chunks_remote = excluded_view(n_total, lo, lo + n_local, &p.remote);
  p.slabs_remote = p.chunks_remote == 0 ? 0 : slabs_remote ? slabs_remote : slabs_f64(p.groups, p.chunks_remote);
  split_chunks(p.remote, p.chunks_remote, p.slabs_remote > 0 ? p.slabs_remote : 1);
  return p;
}

}  // namespace
