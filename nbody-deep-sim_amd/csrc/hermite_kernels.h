// hermite_kernels.h -- everything the Hermite translation units share (direct_hermite.hip: all targets, shared timestep;
// direct_hermite_block.hip: an active list of targets, block timesteps; direct_batch_hermite.hip: many independent
// systems, shared timestep per system; direct_hermite_shard.hip: one rank's bodies of a range partition; and their
// float64 forms):
//   - the acceleration-plus-jerk wave body (accel_jerk_body: target loads, LDS-DMA chunk walk, pair loop, four-wave
//     reduction, store; its compile-time parameters also give direct_hermite_shard.hip's range-sharded blocks: targets
//     apart from the sources, 8-float rows, a skipped source range), the split of the chunks over the waves (chunk_split
//     on the host or from a scene record, wave_chunk_range / wave_chunks in a kernel) and the prologue of a kernel that
//     calls the body (Group128: the workgroup's two targets per lane, the wave's place in the split, the slab destination);
//   - the O(N) stages, templates of the scalar type T of the state (float; double for direct_hermite_f64.hip and
//     direct_hermite_block_f64.hip): what the format fixes (HermiteFmt<T>: the packed row, the rows per workgroup of a
//     finishing launch), the step constants (hermite_step_constants; hermite_dt for fp32; HermiteStepRow: their rows in
//     a per-scene table), the predictor of one component and of one body (hermite_predict, hermite_predict_row), the
//     fixed-order slab sum (hermite_slab_sum: the 4-wave scheme for float, slab_order_sum for double -- two orders, each
//     format keeps its own), the corrector of one component and of one body (hermite_correct, hermite_correct_row), and
//     the shared step's two O(N) kernels: hermite_predict_kernel<T, SS> (SS: the row stride of the packed rows) and
//     hermite_correct_kernel<T, POSM> (POSM: whether it stores the packed row). direct_hermite.hip and
//     direct_hermite_f64.hip instantiate <T, 1> and <T, true>; the range-sharded units, direct_hermite_shard.hip and
//     direct_hermite_shard_f64.hip, launch the same two on a rank's own bodies as <T, 2> (posm = send, velp = send + 1)
//     and <T, false>, and have no O(N) kernel of their own. The batched units' two (hermite_batch_kernels.h) are these
//     with a scene's prologue;
//   - the launch plan of a force launch (JerkPlan, plan_jerk) and of a range-sharded rank's two (HShardPlan,
//     hshard_plan_out).
// A kernel of one of the units is a prologue that says which targets, which chunks, which rows and which constants, and
// calls of these: a scene of a batch, or a block step at level 0, is bit-identical to the shared-timestep step because
// there is one copy of every rounded operation, in either format, not because copies are kept alike.
// The definitions sit in an anonymous namespace: every translation unit that includes this file gets its own inlined copies.
#pragma once
#include "direct_kernels.h"

namespace {

// The pair policy of accel_jerk_body: what a target loads from its two rows, the masked pair, the un-masked block of KU
// sources, the number of per-lane accumulators and of outputs, and how an output is formed from the accumulators. This one
// is acceleration plus jerk; direct_grad.hip states the vector-Jacobian product of the acceleration as a second one and
// walks the chunks with the same body. own(pc, i0): the physical chunk pc holds indices of the workgroup's own targets
// and takes the masked pair for that reason alone (never, here: i == j is an exact zero).
struct AccelJerkPolicy {
  static constexpr int kAcc = 9, kOut = 6;
  f2 xi, yi, zi, ui, vi, wi;

  // t0, t1: the position rows of the lane's two targets, u0, u1: their velocity rows
  __device__ __forceinline__ AccelJerkPolicy(const f4 t0, const f4 t1, const f4 u0, const f4 u1)
      : xi{t0.x, t1.x}, yi{t0.y, t1.y}, zi{t0.z, t1.z}, ui{u0.x, u1.x}, vi{u0.y, u1.y}, wi{u0.z, u1.z} {}

  __device__ __forceinline__ bool own(int, int) const { return false; }

  // One source against the lane's two targets, index-masked (softening^2 below kEps2Masked): accel_kernel's rule, only
  // j == i and the padding behind n are dropped. ja accumulates w dv, jb accumulates (r.v s^2) w dr; j = ja - 3 jb.
  // RANGE (an edge chunk of a range-sharded walk, direct_hermite_shard.hip): the sources [ex_lo, ex_hi) are dropped too,
  // by the same select on s, and their rows are replaced by zeros before any arithmetic (a select, not a product:
  // whatever such a row holds, NaN included, never reaches a sum).
  template <bool RANGE>
  __device__ __forceinline__ void masked(f4 p, f4 q, const f2 e2, f2* acc, int j, int i0, int i1, int n, int ex_lo = 0,
                                         int ex_hi = 0) const {
    bool live = j < n;
    if (RANGE) {
      const bool ex = (unsigned)(j - ex_lo) < (unsigned)(ex_hi - ex_lo);
      p = ex ? f4{0.f, 0.f, 0.f, 0.f} : p;
      q = ex ? f4{0.f, 0.f, 0.f, 0.f} : q;
      live = live && !ex;
    }
    const f2 dx = f2{p.x, p.x} - xi, dy = f2{p.y, p.y} - yi, dz = f2{p.z, p.z} - zi;
    const f2 du = f2{q.x, q.x} - ui, dv = f2{q.y, q.y} - vi, dw = f2{q.z, q.z} - wi;
    f2 r2 = __builtin_elementwise_fma(dx, dx, e2);
    r2 = __builtin_elementwise_fma(dy, dy, r2);
    r2 = __builtin_elementwise_fma(dz, dz, r2);
    f2 rv = dx * du;
    rv = __builtin_elementwise_fma(dy, dv, rv);
    rv = __builtin_elementwise_fma(dz, dw, rv);
    f2 s = {__builtin_amdgcn_rsqf(r2.x), __builtin_amdgcn_rsqf(r2.y)};
    s.x = (live && j != i0) ? s.x : 0.0f;
    s.y = (live && j != i1) ? s.y : 0.0f;
    const f2 s2 = s * s;
    const f2 w = (s2 * s) * f2{p.w, p.w};
    const f2 c = (rv * s2) * w;
    acc[0] = __builtin_elementwise_fma(w, dx, acc[0]);
    acc[1] = __builtin_elementwise_fma(w, dy, acc[1]);
    acc[2] = __builtin_elementwise_fma(w, dz, acc[2]);
    acc[3] = __builtin_elementwise_fma(w, du, acc[3]);
    acc[4] = __builtin_elementwise_fma(w, dv, acc[4]);
    acc[5] = __builtin_elementwise_fma(w, dw, acc[5]);
    acc[6] = __builtin_elementwise_fma(c, dx, acc[6]);
    acc[7] = __builtin_elementwise_fma(c, dy, acc[7]);
    acc[8] = __builtin_elementwise_fma(c, dz, acc[8]);
  }

  // KU sources at once, un-masked: interact_block's shape (the 2 KU v_rsq_f32 issued back to back, the mass splat folded
  // into op_sel by one asm multiply that consumes s^3, never the rsq result itself -- see interact()). Per source and pair
  // of targets: 6 v_pk_add (differences), 5 v_pk_fma + 1 v_pk_mul (r^2, r.v), 2 v_rsq_f32, 5 v_pk_mul (s^2, s^3, w, r.v s^2,
  // c = (r.v s^2) w), 9 v_pk_fma (a, w dv, c dr): 26 packed ops (the factor -3 of the jerk's second sum is applied once, to
  // the finished per-lane sum).
  template <int KU>
  __device__ __forceinline__ void block(const f4* __restrict__ bp, const f4* __restrict__ bv, const f2 e2, f2* acc) const {
    f2 zm[KU], dx[KU], dy[KU], dz[KU], du[KU], dv[KU], dw[KU], s[KU], rv[KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const f4 p = bp[u], q = bv[u];
      zm[u] = f2{p.z, p.w};
      dx[u] = f2{p.x, p.x} - xi; dy[u] = f2{p.y, p.y} - yi; dz[u] = f2{p.z, p.z} - zi;
      du[u] = f2{q.x, q.x} - ui; dv[u] = f2{q.y, q.y} - vi; dw[u] = f2{q.z, q.z} - wi;
      f2 r2 = __builtin_elementwise_fma(dx[u], dx[u], e2);
      r2 = __builtin_elementwise_fma(dy[u], dy[u], r2);
      s[u] = __builtin_elementwise_fma(dz[u], dz[u], r2);
      f2 t = dx[u] * du[u];
      t = __builtin_elementwise_fma(dy[u], dv[u], t);
      rv[u] = __builtin_elementwise_fma(dz[u], dw[u], t);
    }
#pragma unroll
    for (int u = 0; u < KU; ++u) s[u] = f2{__builtin_amdgcn_rsqf(s[u].x), __builtin_amdgcn_rsqf(s[u].y)};
    __builtin_amdgcn_sched_group_barrier(0x400, 2 * KU, 0);      // 0x400 = TRANS: keep the rsq's together
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const f2 s2 = s[u] * s[u];
      const f2 s3 = s2 * s[u];
      f2 w;
      asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(w) : "v"(zm[u]), "v"(s3));
      const f2 c = (rv[u] * s2) * w;
      acc[0] = __builtin_elementwise_fma(w, dx[u], acc[0]);
      acc[1] = __builtin_elementwise_fma(w, dy[u], acc[1]);
      acc[2] = __builtin_elementwise_fma(w, dz[u], acc[2]);
      acc[3] = __builtin_elementwise_fma(w, du[u], acc[3]);
      acc[4] = __builtin_elementwise_fma(w, dv[u], acc[4]);
      acc[5] = __builtin_elementwise_fma(w, dw[u], acc[5]);
      acc[6] = __builtin_elementwise_fma(c, dx[u], acc[6]);
      acc[7] = __builtin_elementwise_fma(c, dy[u], acc[7]);
      acc[8] = __builtin_elementwise_fma(c, dz[u], acc[8]);
    }
  }

  // j = (w dv) - 3 (r.v s^2 w dr)
  __device__ __forceinline__ f2 out(const f2* acc, int k) const { return k < 3 ? acc[k] : acc[k] - 3.0f * acc[k + 3]; }
};

// The wave body of every acceleration-plus-jerk kernel. accel_kernel's structure: a workgroup is 4 waves on 128 targets,
// two per lane in packed fp32 (rows r0, r1 of tpos / tvel; i0, i1 are the source indices the masked loop takes for the
// lane's own); every wave streams its chunks [c_begin, c_end) of the n sources, each chunk = 64 positions + 64 velocities
// (2 KiB; a third row with NS = 3) by LDS-DMA, double-buffered behind a counted vmcnt; the 4 waves' partials are reduced through LDS in wave order
// into one coalesced store of 6 x n_valid floats: dst[comp * stride + t], t < n_valid. lds: the workgroup's
// f4[kWaves * 4 * kChunk] (16 KiB), [wave][buffer][pos | vel][64] staging; after its last chunk a wave puts its [12][64]
// partials into its own part. (6 and 12: P::kOut and twice that, for the policy P.)
// Compile-time shape, all defaults = the un-sharded kernels (targets and sources in the same two arrays):
//   SS    : quads between consecutive rows of spos / svel and of tpos / tvel. 1: two arrays of float4 (posm, velp);
//           2: one array of 8-float rows {x, y, z, m, vx, vy, vz, 0} (svel = spos + 1), the layout a range-sharded rank
//           sends and gathers. A lane's LDS-DMA fetches its own row's quad, so the chunk lands de-interleaved in the same
//           [pos | vel][64] staging either way and the pair loops do not know the difference.
//   RANGE : the walk is over the view *sv (direct_kernels.h): [c_begin, c_end) are LOGICAL chunks that hop over the run of
//           physical chunks lying wholly inside [ex_lo, ex_hi), and the (at most two) chunks that straddle an end of that
//           range take the masked loop with the range mask; every other chunk takes the loop MASKED says.
//   P     : the pair policy (above).
//   NS    : the rows streamed per source and loaded per target, 2 or 3. 3 (direct_hermite_grad.hip: {x, m}, {v, 0} and a
//           cotangent row): sthird / tthird are the third arrays, every chunk is one more LDS-DMA, a wave's staging is
//           [buffer][pos | vel | third][64] -- 6 kChunk quads instead of 4 --, the counted wait is vmcnt(3), and the
//           policy's constructor and pair functions take the third row after the second.
template <bool MASKED, int KU, int SS = 1, bool RANGE = false, class P = AccelJerkPolicy, int NS = 2>
__device__ __forceinline__ void accel_jerk_body(const f4* __restrict__ spos, const f4* __restrict__ svel, int n,
                                                const f4* __restrict__ tpos, const f4* __restrict__ tvel, int r0,
                                                int r1, int i0, int i1, int c_begin, int c_end, float eps2, f4* lds,
                                                float* __restrict__ dst, int stride, int n_valid,
                                                const SrcView* sv = nullptr,
                                                const f4* __restrict__ sthird = nullptr,
                                                const f4* __restrict__ tthird = nullptr) {
  static_assert(NS == 2 || NS == 3, "two or three rows per source");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const f4 t0 = tpos[r0 * SS], t1 = tpos[r1 * SS];
  const f4 u0 = tvel[r0 * SS], u1 = tvel[r1 * SS];
  const P pol = [&] {
    if constexpr (NS == 3) return P(t0, t1, u0, u1, tthird[r0 * SS], tthird[r1 * SS]);
    else return P(t0, t1, u0, u1);
  }();
  f2 acc[P::kAcc];
#pragma unroll
  for (int k = 0; k < P::kAcc; ++k) acc[k] = f2{0.f, 0.f};
  f2 e2 = {eps2, eps2};
  asm volatile("" : "+v"(e2));  // keep eps^2 in VGPRs: an SGPR operand halves v_pk_fma issue

  f4* stage = &lds[wave * 2 * NS * kChunk];
  const f4* p_lane = spos + lane * SS;
  const f4* v_lane = svel + lane * SS;
  const f4* b_lane = NS == 3 ? sthird + lane * SS : nullptr;
  // logical -> physical chunk: hop over the skipped run
  auto phys = [&](int c) { return RANGE ? c + (c >= sv->skip_c0 ? sv->skip_cn : 0) : c; };
  auto fetch = [&](int c, int b) {
    const size_t at = (size_t)phys(c) * (kChunk * SS);
    __builtin_amdgcn_global_load_lds(GPTR(p_lane + at), LPTR(stage + b * NS * kChunk), 16, 0, 0);
    __builtin_amdgcn_global_load_lds(GPTR(v_lane + at), LPTR(stage + b * NS * kChunk + kChunk), 16, 0, 0);
    if constexpr (NS == 3)
      __builtin_amdgcn_global_load_lds(GPTR(b_lane + at), LPTR(stage + b * NS * kChunk + 2 * kChunk), 16, 0, 0);
  };
  if (c_begin < c_end) fetch(c_begin, 0);
  for (int c = c_begin; c < c_end; ++c) {
    const int b = (c - c_begin) & 1;
    if (c + 1 < c_end) {
      fetch(c + 1, b ^ 1);
      // chunk c has landed, c+1 (NS loads) in flight
      if constexpr (NS == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const f4* bp = stage + b * NS * kChunk;
    const f4* bv = bp + kChunk;
    const int pc = phys(c);
    if constexpr (NS == 3) {      // no range-sharded form: the masked pair or the un-masked block, with the third row
      const f4* bb = bv + kChunk;
      if (MASKED || pol.own(pc, i0)) {
        const int j0 = pc * kChunk;
#pragma unroll 2
        for (int j = 0; j < kChunk; ++j) pol.masked(bp[j], bv[j], bb[j], e2, acc, j0 + j, i0, i1, n);
      } else {
#pragma unroll 1
        for (int j = 0; j < kChunk; j += KU) pol.template block<KU>(bp + j, bv + j, bb + j, e2, acc);
      }
    } else if (RANGE && (pc == sv->edge0 || pc == sv->edge1)) {
      const int j0 = pc * kChunk;
#pragma unroll 2
      for (int j = 0; j < kChunk; ++j)
        pol.template masked<true>(bp[j], bv[j], e2, acc, j0 + j, i0, i1, n, sv->ex_lo, sv->ex_hi);
    } else if (MASKED || pol.own(pc, i0)) {
      const int j0 = pc * kChunk;
#pragma unroll 2
      for (int j = 0; j < kChunk; ++j)
        pol.template masked<false>(bp[j], bv[j], e2, acc, j0 + j, i0, i1, n);
    } else {
#pragma unroll 1
      for (int j = 0; j < kChunk; j += KU) pol.template block<KU>(bp + j, bv + j, e2, acc);
    }
  }

  // wavefront partials (P::out) -> LDS -> one coalesced (kOut x 128) store per workgroup. A wave's staging is free
  // here: its loads have landed (vmcnt(0) on the last chunk) and its reads precede these writes.
  constexpr int kPart = 2 * NS * kChunk * 4;              // floats per wave: [comp*2+half][64] in the first kOut * 128
  static_assert(P::kOut * 128 <= kPart, "the partials must fit a wave's staging");
  float* red = reinterpret_cast<float*>(lds);
  float* mine = red + wave * kPart;
#pragma unroll
  for (int k = 0; k < P::kOut; ++k) {
    const f2 v = pol.out(acc, k);
    mine[(2 * k) * 64 + lane] = v.x;
    mine[(2 * k + 1) * 64 + lane] = v.y;
  }
  __syncthreads();
  for (int o = threadIdx.x; o < P::kOut * kTgtPerWG; o += 64 * kWaves) {
    const int comp = o >> 7, lt = o & 127;
    if (lt >= n_valid) continue;
    const int idx = (comp * 2 + (lt >> 6)) * 64 + (lt & 63);
    float sum = red[idx];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) sum += red[w * kPart + idx];
    dst[(size_t)comp * stride + lt] = sum;
  }
}

// The balanced split of n_chunks source chunks over slabs x 4 waves: every wave walks q chunks, the first r waves one more.
struct ChunkSplit { int q, r; };

__host__ __device__ inline ChunkSplit chunk_split(int n_chunks, int slabs) {
  return ChunkSplit{n_chunks / (slabs * kWaves), n_chunks % (slabs * kWaves)};
}

// the chunks [c_begin, c_end) of wave jw = slab * 4 + wave under that split
__device__ __forceinline__ void wave_chunk_range(int jw, int q, int r, int& c_begin, int& c_end) {
  c_begin = jw * q + min(jw, r);
  c_end = c_begin + q + (jw < r ? 1 : 0);
}

// ... as a value: from the launch's (q, r), or with (q, r) formed from a scene's n_chunks and slabs (a batch item)
struct ChunkRange { int begin, end; };

__device__ __forceinline__ ChunkRange wave_chunks(int jw, int q, int r) {
  ChunkRange c;
  wave_chunk_range(jw, q, r, c.begin, c.end);
  return c;
}

__device__ __forceinline__ ChunkRange wave_chunks_of(int jw, int n_chunks, int slabs) {
  const int parts = slabs * kWaves;
  return wave_chunks(jw, n_chunks / parts, n_chunks % parts);
}

// The prologue of every accel_jerk_body kernel: what workgroup (grp, slab) of n targets and its lanes work on. t_base is
// the group's first target; i0 and i1 = i0 + 64 are the lane's two (either may lie behind n: it then repeats row n - 1
// and stores nothing), r0() and r1() their rows; jw() is the wave's place in the split of the chunks, slab * 4 + wave;
// n_valid() the targets of the group that exist. grp and slab come from blockIdx (one system, a rank's block:
// I = unsigned) or from a work item (a scene of a batch, load_item of direct_batch_plan.h: I = int) and keep their type;
// what is not a member is formed where the kernel asks for it. Both so that every kernel compiles to the instructions
// it had with these lines written out in it.
template <class I>
struct Group128 {
  I slab;
  int n, t_base, i0, i1;

  __device__ __forceinline__ Group128(I grp, I slab_, int n_)
      : slab(slab_), n(n_), t_base(grp * kTgtPerWG), i0(t_base + (threadIdx.x & 63)), i1(i0 + 64) {}
  __device__ __forceinline__ int jw() const { return slab * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }
  __device__ __forceinline__ int r0() const { return min(i0, n - 1); }
  __device__ __forceinline__ int r1() const { return min(i1, n - 1); }
  __device__ __forceinline__ int n_valid() const { return min(kTgtPerWG, n - t_base); }
  // the group's place in the slab of base = float[slabs][P::kOut][n]: accel_jerk_body's dst (with stride n)
  template <class P = AccelJerkPolicy>
  __device__ __forceinline__ float* dst(float* __restrict__ base) const {
    return base + (size_t)slab * P::kOut * n + t_base;
  }
};

// The geometry of a force launch: the all-pairs force's plan (nbd_accel_plan) for n_tgt targets under n sources -- same
// targets, same chunks, the same balance problem.
struct JerkPlan { int groups, slabs, n_chunks; };

inline JerkPlan plan_jerk(int n, int n_tgt) {
  JerkPlan p;
  int cpw = 0;
  nbd_accel_plan(n, n_tgt, &p.groups, &p.slabs, &cpw);
  p.n_chunks = ceil_div(n, kChunk);
  return p;
}

// The geometry of a range-sharded rank's two force launches, in either format (direct_hermite_shard.hip: plan_hshard;
// hermite_f64_kernels.h: plan_hshard_f64 -- two plan functions, which choose their slab counts differently), and what a
// plan entry writes out of it.
struct HShardPlan { int groups, slabs_local, chunks_local, slabs_remote, chunks_remote; SrcView remote; };

inline void hshard_plan_out(const HShardPlan& p, int* slabs_local, int* chunks_per_wave_local, int* slabs_remote,
                            int* chunks_per_wave_remote) {
  if (slabs_local) *slabs_local = p.slabs_local;
  if (chunks_per_wave_local) *chunks_per_wave_local = ceil_div(p.chunks_local, p.slabs_local * kWaves);
  if (slabs_remote) *slabs_remote = p.slabs_remote;
  if (chunks_per_wave_remote)
    *chunks_per_wave_remote = p.slabs_remote ? ceil_div(p.chunks_remote, p.slabs_remote * kWaves) : 0;
}

// fp32 step constants, each formed in double and rounded once. On the device too: a block-timestep body forms them from
// its own fp64 step, so one whose step is the whole interval gets the shared step's bits.
// (T = double, direct_hermite_f64.hip and direct_hermite_block_f64.hip: the same five doubles, not rounded again.)
template <class T>
struct HermiteStep { T dt, dt_half, dt2_half, dt3_sixth, dt2_twelfth; };
using HermiteDt = HermiteStep<float>;

// ... as the rows of a per-scene table T[kRows][S] (the batched units: field k of scene s at step[k * S + s])
struct HermiteStepRow { enum { kDt, kDtHalf, kDt2Half, kDt3Sixth, kDt2Twelfth, kRows }; };
static_assert(sizeof(HermiteStep<double>) == HermiteStepRow::kRows * sizeof(double), "one row per field, in its order");

template <class T>
__host__ __device__ inline HermiteStep<T> hermite_step_constants(double dt) {
  return HermiteStep<T>{(T)dt, (T)(0.5 * dt), (T)(0.5 * dt * dt), (T)(dt * dt * dt / 6.0), (T)(dt * dt / 12.0)};
}

__host__ __device__ inline HermiteDt hermite_dt(double dt) { return hermite_step_constants<float>(dt); }

// What a number format (the scalar type T of the state) fixes for the O(N) stages: the packed row {x, y, z, w} the force
// kernels read, its zero (the padding behind n), and the geometry of the finishing launch that adds the slabs
// (hermite_slab_sum below) -- the rows a 256-thread workgroup covers; a launch site takes its grid from it.
template <class T> struct HermiteFmt;
template <> struct HermiteFmt<float> {
  using Row = f4;
  static __device__ __forceinline__ Row zero() { return Row{0.f, 0.f, 0.f, 0.f}; }
  static constexpr int kSumRows = 64;       // 4 waves on the same 64 rows
};
template <> struct HermiteFmt<double> {
  using Row = d4;
  static __device__ __forceinline__ Row zero() { return Row{0.0, 0.0, 0.0, 0.0}; }
  static constexpr int kSumRows = 256;      // one thread per row
};

template <class T>
__device__ __forceinline__ typename HermiteFmt<T>::Row hermite_row(const T* x, const T w) {
  return typename HermiteFmt<T>::Row{x[0], x[1], x[2], w};
}

// the row of the finishing launch this thread works on
template <class T>
__device__ __forceinline__ size_t hermite_sum_row() {
  return (size_t)blockIdx.x * HermiteFmt<T>::kSumRows + threadIdx.x % HermiteFmt<T>::kSumRows;
}

// One component of the predictor, each product and sum rounded on its own (the build has -ffp-contract=off):
// x_p = x + v dt + a dt^2/2 + j dt^3/6, v_p = v + a dt + j dt^2/2.
template <class T>
struct PosVelT { T x, v; };

template <class T>
__device__ __forceinline__ PosVelT<T> hermite_predict(const T x, const T v, const T a, const T j, const T dt,
                                                      const T dt2_half, const T dt3_sixth) {
  return PosVelT<T>{((x + v * dt) + a * dt2_half) + j * dt3_sixth, (v + a * dt) + j * dt2_half};
}

// The predictor of body i of pos, vel, acc, jerk (n, 3): its three components of x_p and of v_p. predict == false: x and
// v as they are (a plain pack; acc and jerk are not read). (Two local arrays, copied out at the end: filled in place, the
// returned struct makes hipcc pair the fp32 additions of x_p and v_p into v_pk_add_f32 -- the same bits, another kernel.)
template <class T>
struct PosVel3 { T x[3], v[3]; };

template <class T>
__device__ __forceinline__ PosVel3<T> hermite_predict_row(const T* __restrict__ pos, const T* __restrict__ vel,
                                                          const T* __restrict__ acc, const T* __restrict__ jerk,
                                                          const size_t i, const T dt, const T dt2_half,
                                                          const T dt3_sixth, const bool predict) {
  T x[3], v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    x[k] = pos[3 * i + k];
    v[k] = vel[3 * i + k];
    if (predict) {
      const PosVelT<T> p = hermite_predict(x[k], v[k], acc[3 * i + k], jerk[3 * i + k], dt, dt2_half, dt3_sixth);
      x[k] = p.x;
      v[k] = p.v;
    }
  }
  return PosVel3<T>{{x[0], x[1], x[2]}, {v[0], v[1], v[2]}};
}

// posm = {x_p, m}, velp = {v_p, 0} for rows [0, n_pad) (zero rows behind n). acc == nullptr: plain pack (x, v).
// SS: the rows between consecutive bodies of posm and of velp, accel_jerk_body's SS. 1: two arrays; 2: the send buffer of
// a range-sharded rank, one array of rows {x_p, m | v_p, 0} (posm = send, velp = send + 1).
template <class T, int SS = 1>
__global__ __launch_bounds__(256) void hermite_predict_kernel(const T* __restrict__ pos, const T* __restrict__ vel,
                                                              const T* __restrict__ acc, const T* __restrict__ jerk,
                                                              const T* __restrict__ mass, int n, int n_pad,
                                                              HermiteStep<T> h,
                                                              typename HermiteFmt<T>::Row* __restrict__ posm,
                                                              typename HermiteFmt<T>::Row* __restrict__ velp) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n_pad) return;
  typename HermiteFmt<T>::Row pm = HermiteFmt<T>::zero(), vp = HermiteFmt<T>::zero();
  if (i < (size_t)n) {
    const PosVel3<T> p = hermite_predict_row(pos, vel, acc, jerk, i, h.dt, h.dt2_half, h.dt3_sixth, acc != nullptr);
    pm = hermite_row(p.x, mass[i]);
    vp = hermite_row(p.v, (T)0);
  }
  posm[SS * i] = pm;
  velp[SS * i] = vp;
}

// sum[k] = slab 0 + slab 1 + ... of row `row`, component k < K, of slabs = double[n_slabs][K][stride], in slab order:
// the fp64 units' sum, one thread per row.
template <int K>
__device__ __forceinline__ void slab_order_sum(const double* __restrict__ slabs, int n_slabs, size_t stride, size_t row,
                                               double* sum) {
#pragma unroll
  for (int k = 0; k < K; ++k) sum[k] = 0.0;
  for (int s = 0; s < n_slabs; ++s)
#pragma unroll
    for (int k = 0; k < K; ++k) sum[k] += slabs[((size_t)s * K + k) * stride + row];
}

// a1 = g * sum of the slabs of slabs = T[n_slabs][6][stride], j1 likewise, in a fixed order, by a 256-thread workgroup on
// HermiteFmt<T>::kSumRows consecutive rows; row = hermite_sum_row<T>(). Every thread of the workgroup calls it (the fp32
// form holds a barrier); a row that is not valid reads nothing. True for the one thread per valid row that holds a1, j1.
// The two formats add in different orders, and each keeps its own:
//   float : finish_kernel's scheme, 4 waves on 64 rows: wave w sums slabs w, w+4, ... of its lane's row, the four
//           partials combined through LDS as (p0 + p1) + (p2 + p3); wave 0 holds the result.
//   double: slab_order_sum, one thread per row.
__device__ __forceinline__ bool hermite_slab_sum(const float* __restrict__ slabs, int n_slabs, int stride, size_t row,
                                                 bool valid, float g, float* a1, float* j1) {
  __shared__ float part[4][6][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float sum[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (valid)
    for (int s = w; s < n_slabs; s += 4)
#pragma unroll
      for (int k = 0; k < 6; ++k) sum[k] += slabs[((size_t)s * 6 + k) * stride + row];
#pragma unroll
  for (int k = 0; k < 6; ++k) part[w][k][lane] = sum[k];
  __syncthreads();
  if (w != 0 || !valid) return false;
  auto total = [&](int k) {
    return g * ((part[0][k][lane] + part[1][k][lane]) + (part[2][k][lane] + part[3][k][lane]));
  };
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a1[k] = total(k);
    j1[k] = total(k + 3);
  }
  return true;
}

__device__ __forceinline__ bool hermite_slab_sum(const double* __restrict__ slabs, int n_slabs, int stride, size_t row,
                                                 bool valid, double g, double* a1, double* j1) {
  if (!valid) return false;
  double sum[6];
  slab_order_sum<6>(slabs, n_slabs, (size_t)stride, row, sum);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a1[k] = g * sum[k];
    j1[k] = g * sum[k + 3];
  }
  return true;
}

// One component of the corrector, each product and sum rounded on its own:
// v1 = v + (a0 + a1) dt/2 + (j0 - j1) dt^2/12, x1 = x + (v + v1) dt/2 + (a0 - a1) dt^2/12.
template <class T>
__device__ __forceinline__ void hermite_correct(T& x, T& v, const T a0, const T j0, const T a1, const T j1,
                                                const T dt_half, const T dt2_twelfth) {
  const T v1 = (v + (a0 + a1) * dt_half) + (j0 - j1) * dt2_twelfth;
  x = (x + (v + v1) * dt_half) + (a0 - a1) * dt2_twelfth;
  v = v1;
}

// The corrector of body i: reads a0, j0 (acc_in / jerk_in, which may alias the arrays a1, j1 are stored to afterwards:
// each element is read before it is written, by the same thread), x, v; writes x1, v1. Returns x1 and the a0, j0 it read.
template <class T>
struct Corrected { T x1[3], a0[3], j0[3]; };

template <class T>
__device__ __forceinline__ Corrected<T> hermite_correct_row(T* pos, T* vel, const T* acc_in, const T* jerk_in,
                                                            const size_t i, const T* a1, const T* j1, const T dt_half,
                                                            const T dt2_twelfth) {
  Corrected<T> c;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c.a0[k] = acc_in[3 * i + k];
    c.j0[k] = jerk_in[3 * i + k];
    T x = pos[3 * i + k], v = vel[3 * i + k];
    hermite_correct(x, v, c.a0[k], c.j0[k], a1[k], j1[k], dt_half, dt2_twelfth);
    vel[3 * i + k] = v;
    pos[3 * i + k] = c.x1[k] = x;
  }
  return c;
}

// acc[i] = a1, jerk[i] = j1
template <class T>
__device__ __forceinline__ void hermite_store_force(T* acc, T* jerk, const size_t i, const T* a1, const T* j1) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    acc[3 * i + k] = a1[k];
    jerk[3 * i + k] = j1[k];
  }
}

// One workgroup per HermiteFmt<T>::kSumRows consecutive bodies: a1, j1 = hermite_slab_sum of the body's row. pos ==
// nullptr: write a1, j1 only (the force on its own). Else hermite_correct_row, then a1, j1 and posm = {x1, m} (energies
// after the step need no extra pack). POSM = false (a range-sharded rank: its packed rows are rebuilt by the next
// predictor): posm and mass are not used.
template <class T, bool POSM = true>
__global__ __launch_bounds__(256) void hermite_correct_kernel(const T* __restrict__ slabs, int n_slabs, int n, T g,
                                                              HermiteStep<T> h, T* pos, T* vel, const T* acc_in,
                                                              const T* jerk_in, T* acc_out, T* jerk_out,
                                                              const T* __restrict__ mass,
                                                              typename HermiteFmt<T>::Row* __restrict__ posm) {
  const size_t i = hermite_sum_row<T>();
  T a1[3], j1[3];
  if (!hermite_slab_sum(slabs, n_slabs, n, i, i < (size_t)n, g, a1, j1)) return;
  if (pos) {
    const Corrected<T> c = hermite_correct_row(pos, vel, acc_in, jerk_in, i, a1, j1, h.dt_half, h.dt2_twelfth);
    if constexpr (POSM) posm[i] = hermite_row(c.x1, mass[i]);
  }
  hermite_store_force(acc_out, jerk_out, i, a1, j1);
}

}  // namespace
