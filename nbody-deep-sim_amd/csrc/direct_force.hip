// direct_force.hip -- all-pairs softened gravity + leapfrog/Euler updates for gfx950 (MI355X).
//
// Replaces the arithmetic of the reference's BaseSimulator.compute_accelerations
// (src/galaxify/simulation.py:71-89), LeapFrogSimulator.step (:153-170),
// EulerSimulator.step (:173-187) and compute_energies (:91-115). C-ABI: include/nbd.h.
//
// K1 design:
//   * the kernel is VALU-issue bound (16 FMA-slot equivalents per pair, v_rsq_f32 = 4 of them),
//     so everything is arranged to keep the four SIMDs of a CU issuing packed fp32 math:
//     each lane owns TWO targets held as float2 register pairs, so one broadcast source feeds
//     v_pk_add/v_pk_fma/v_pk_mul on both; two register shapes of the same code are built: eight
//     sources in flight per wave (86-96 VGPRs, 5 waves/SIMD: best issue rate, the default) and four
//     (<=64 VGPRs, 8 waves/SIMD: more, smaller workgroup slots for launches with few targets);
//   * every wave is autonomous: it streams its own slice of the source array in 64-body
//     (1 KiB) chunks HBM/L2 -> LDS by LDS-DMA (global_load_lds_dwordx4: coalesced float4
//     loads, no VGPR staging), double-buffered behind a counted vmcnt, and reads the chunk
//     back with wave-uniform ds_read_b128 (LDS broadcast). No workgroup barrier in the loop;
//   * the 4 waves of a workgroup share the same 128 targets and split the sources (J-split);
//     their partial forces are reduced through LDS (wavefront-level partials -> one coalesced
//     store per workgroup). A second J-split across workgroups (gridDim.y slabs) fills the
//     256 CUs when there are few targets; slabs are summed in fixed order by the finishing
//     kernel, so results are bit-reproducible (no float atomics).
#include <hip/hip_runtime.h>
#include <string.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/nbd.h"
#include "direct_kernels.h"

namespace {

// grid = (target groups of 128, slabs); block = 256: accel_body (direct_kernels.h) on group blockIdx.x, slab blockIdx.y.
// KU = 8: 96 VGPRs (UNI: 86), 5 waves/SIMD. KU = 4: capped at 64 VGPRs, 8 waves/SIMD.
// UNI (round 3): every body has the SAME mass -- the published configurations (Plummer, m = 1 / N) among them. The mass
// then factors out of the whole sum, a = (G m) sum_j d_ij s_ij^3: the per-pair multiply by m_j goes (11 packed ops +
// 2 v_rsq_f32 per source and pair of targets instead of 12 + 2: 60 issue cycles per 128 pairs instead of 64), the
// differences stay the exact fp32 subtractions of the reference, and the only change in rounding is ONE multiplication
// of the finished sum instead of one per term. (Folding unequal masses into the coordinates -- c_j = m_j^(-1/2) scales
// source j so that rsq^3 carries m_j -- also reaches 11 ops and was built first; it gives up the exact difference
// c_j r_j - c_j r_i rounds the product c_j r_j -- and a close pair amplifies that half-ulp shift of the source:
// 1.8e-4 on one row of the Plummer N = 1000 golden, against the 1e-5 bar. Rejected; measured +2.9 %.) Padding entries
// are no zeros without the mass factor: the chunk that holds them (sv.tail) takes the masked path.
// out_rows: rows between slabs of `out` (n_tgt, or the system size when the launch fills rows of a wider slot array).
// tile_len: gridDim.z > 1 runs independent diagonal blocks, block z taking targets AND sources [z*tile_len, +n_tgt)
// (the diagonal blocks of the symmetric step, see accel_sym_kernel); 0 for every other launch.
template <bool MASKED, int KU, bool UNI = false>
__global__ __launch_bounds__(64 * kWaves, KU == 4 ? 8 : 5) void accel_kernel(
    const f4* __restrict__ src, const SrcView sv, const f4* __restrict__ tgt,
    int n_tgt, int tgt_off, float eps2, float scale, float* __restrict__ out, int out_rows, int tile_len) {
  __shared__ f4 lds[kAccelLdsF4];
  const int tz = blockIdx.z * tile_len;
  const int t_base = blockIdx.x * kTgtPerWG;
  accel_body<KU, UNI>(src + tz, sv, std::integral_constant<bool, MASKED>{}, tgt + tz, n_tgt, tgt_off, t_base, blockIdx.y, eps2, scale, lds,
                      out + (size_t)tz * 3 + ((size_t)blockIdx.y * out_rows + t_base) * 3);
}

// ---- symmetric force for EQUAL masses: every off-diagonal pair evaluated once (Newton's third law).
// The term of j on i is the exact negative of the term of i on j (r_j - r_i and r_i - r_j are exact negatives in fp32,
// r^2 and rsq come out bit-identical), so one evaluation feeds both rows; only the order of summation changes.
//
// The first core = M * S bodies (M even) are cut into M super-tiles of S = 1024. The M (M - 1) / 2 off-diagonal tile
// pairs are the M - 1 rounds of a round-robin tournament (circle method): round r pairs every tile with exactly one
// other, so one round writes each core row exactly once. Round r writes slot (r + 1) % K of the float[K][n][3] partial
// array; the diagonal blocks (accel_kernel, one launch) write slot 0. The rounds go in launches of at most K: the first
// launch (rounds 0 .. K-2) stores, every later one adds to what an earlier launch stored, so no two workgroups of one
// launch touch the same (slot, row) and the per-row sums have a fixed order: deterministic, no atomics, every slot written
// every step (no zero fill: capturable). K is read off the workspace (plan_sym): min(M, 16) in the 16 slots the all-pairs
// step needs at N = 65 536, up to min(M, 64) in a larger one. With K = M no round shares a slot: every round stores, the
// fetch of an adding launch never runs and all M (M - 1) / 2 tile pairs go in ONE launch (N = 65 536: 2016 workgroups,
// 3.94 residency rounds instead of four launches of one; 627.7 against 648.8 us, profiles/r15_sym_wide.txt). The step's
// form of that launch (accel_sym2_tail_kernel) carries the diagonal blocks too, as its highest-numbered workgroups: same
// slot 0, same arithmetic and order as the diagonal launch, one launch less (599.6 against 20.3 + 587.4 us,
// profiles/r25_sym_tail.txt).
//
// One workgroup = one tile pair (a, b): 4 target groups x SG source groups of waves. Wave (tg, sg) holds targets
// a*S + tg*256 + 64 t + lane (t = 0..3, as the packed pairs {t0, t1}, {t2, t3}) and walks the 16 / SG 64-body chunks
// of source group sg of tile b. Step k of a chunk: lane l takes source (l + k) & 63 (a lane-varying ds_read_b128 from a
// chunk stored twice, so the address is the immediate offset k * 16 and never wraps), adds w d to its own sums and
// -w d to the reaction registers of that source, then the 6 reaction VGPRs move one lane down (DPP wave_rol:1): after
// 64 steps lane l holds the reaction on source l from the wave's 256 targets. At the end of a chunk the 4 target groups
// add their reactions through LDS in wave order (one barrier per chunk); at the end of the tile pair the SG source
// groups add their own sums through LDS in order. Per step and pair of targets: 14 packed ops + 2 v_rsq_f32; per step
// 6 DPP moves for 4 targets.
constexpr int kSymTile = 1024;                   // S
constexpr int kSymChunks = kSymTile / kChunk;    // 16
constexpr int kSymSlots = 16;                    // K of the narrow plan: the workspace of the all-pairs step at N = 65 536
constexpr int kSymSlotsCap = 64;                 // K at most, whatever the workspace holds (memory at K = M grows as N^2)
constexpr int kSymSlotsPref = 64;                // K of the preferred workspace (nbd_step_workspace_pref_bytes)

__device__ __forceinline__ float rol1(float x) {  // lane l <- lane (l + 1) & 63
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x134 /* wave_rol:1 */, 0xf, 0xf, false));
}

// one source against two targets: own sums += w d, reaction -= w d (the neg modifier of v_pk_fma)
__device__ __forceinline__ void sym_pair(const f4 p, const f2 xi, const f2 yi, const f2 zi, const f2 e2,
                                         f2& ax, f2& ay, f2& az, f2& rx, f2& ry, f2& rz) {
  const f2 dx = f2{p.x, p.x} - xi, dy = f2{p.y, p.y} - yi, dz = f2{p.z, p.z} - zi;  // r_j - r_i
  f2 r2 = __builtin_elementwise_fma(dx, dx, e2);
  r2 = __builtin_elementwise_fma(dy, dy, r2);
  r2 = __builtin_elementwise_fma(dz, dz, r2);
  const f2 s = {__builtin_amdgcn_rsqf(r2.x), __builtin_amdgcn_rsqf(r2.y)};
  const f2 w = (s * s) * s;
  ax = __builtin_elementwise_fma(w, dx, ax);
  ay = __builtin_elementwise_fma(w, dy, ay);
  az = __builtin_elementwise_fma(w, dz, az);
  rx = __builtin_elementwise_fma(-w, dx, rx);
  ry = __builtin_elementwise_fma(-w, dy, ry);
  rz = __builtin_elementwise_fma(-w, dz, rz);
}

// tile pair (ta, tb) of workgroup wg of the launch that starts at round r0: round r of the circle method, match i
__device__ __forceinline__ void sym_round_match(int wg, int m, int r0, int n_slots, int& ta, int& tb, int& slot,
                                                bool& init) {
  const int half = m >> 1, mm = m - 1;
  const int rr = wg / half, i = wg - rr * half, r = r0 + rr;
  ta = i == 0 ? r % mm : (r + i) % mm;
  tb = i == 0 ? mm : (r - i + mm) % mm;
  slot = (r + 1) % n_slots;
  init = r + 1 < n_slots;
}

// grid = (rounds of this launch) x M/2 workgroups; block = 256 * SG. Unscaled sums (finish_kernel applies G m).
template <int SG>
__global__ __launch_bounds__(256 * SG, 2 * SG) void accel_sym_kernel(const f4* __restrict__ posm, int n, int m,
                                                                     int r0, int n_slots, float eps2,
                                                                     float* __restrict__ out) {
  constexpr int CPS = kSymChunks / SG;           // chunks per source group
  constexpr int kStageF4 = SG * 2 * 2 * kChunk;  // [sg][buffer][copy][64] f4
  constexpr int kRedF = 2 * 4 * SG * 3 * 64;     // [parity][wave][comp][lane] floats
  constexpr int kOwnF = SG * 4 * 12 * 64;        // [sg][tg][comp * 4 + t][lane] floats
  constexpr int kLdsF = (kStageF4 * 4 + kRedF > kOwnF) ? kStageF4 * 4 + kRedF : kOwnF;
  __shared__ f4 lds[kLdsF / 4];                  // ONE object (keeps hipcc's waits sane)
  float* const ldsf = reinterpret_cast<float*>(lds);

  int ta, tb, slot;
  bool init;
  sym_round_match(blockIdx.x, m, r0, n_slots, ta, tb, slot, init);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tg = wave & 3, sg = wave >> 2;
  const int row0 = ta * kSymTile + tg * 256 + lane;
  const f4 q0 = posm[row0], q1 = posm[row0 + 64], q2 = posm[row0 + 128], q3 = posm[row0 + 192];
  const f2 xa = {q0.x, q1.x}, ya = {q0.y, q1.y}, za = {q0.z, q1.z};
  const f2 xb = {q2.x, q3.x}, yb = {q2.y, q3.y}, zb = {q2.z, q3.z};
  f2 axa = {0.f, 0.f}, aya = {0.f, 0.f}, aza = {0.f, 0.f}, axb = {0.f, 0.f}, ayb = {0.f, 0.f}, azb = {0.f, 0.f};
  f2 e2 = {eps2, eps2};
  asm volatile("" : "+v"(e2));  // keep eps^2 in VGPRs: an SGPR operand halves v_pk_fma issue

  // sources: the chunks of source group sg of tile b, staged by target group 3 (not a reducer: its vmcnt counts only
  // the staging loads) into a buffer the 4 target groups share; the per-chunk barrier publishes and releases it
  f4* const stage = &lds[sg * 4 * kChunk];
  const int c0 = tb * kSymChunks + sg * CPS;
  const f4* const s_lane = posm + lane + (size_t)c0 * kChunk;
  auto fetch = [&](int c, int b) {
    __builtin_amdgcn_global_load_lds(GPTR(s_lane + c * kChunk), LPTR(stage + b * 2 * kChunk), 16, 0, 0);
    __builtin_amdgcn_global_load_lds(GPTR(s_lane + c * kChunk), LPTR(stage + b * 2 * kChunk + kChunk), 16, 0, 0);
  };
  if (tg == 3) {
    fetch(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();

  for (int c = 0; c < CPS; ++c) {
    const int b = c & 1;
    if (tg == 3 && c + 1 < CPS) fetch(c + 1, b ^ 1);
    // reducer tg (< 3) adds component tg of this chunk's reaction to what an earlier launch stored: fetch it now
    float* const o_react = out + ((size_t)slot * n + (size_t)(c0 + c) * kChunk + lane) * 3 + tg;
    float old = 0.f;
    if (!init && tg < 3) old = *o_react;
    const f4* buf = stage + b * 2 * kChunk + lane;
    f2 rx = {0.f, 0.f}, ry = {0.f, 0.f}, rz = {0.f, 0.f};
#pragma unroll 2
    for (int k = 0; k < kChunk; ++k) {
      const f4 p = buf[k];
      sym_pair(p, xa, ya, za, e2, axa, aya, aza, rx, ry, rz);
      sym_pair(p, xb, yb, zb, e2, axb, ayb, azb, rx, ry, rz);
      rx = f2{rol1(rx.x), rol1(rx.y)};
      ry = f2{rol1(ry.x), rol1(ry.y)};
      rz = f2{rol1(rz.x), rol1(rz.y)};
    }
    float* const red = ldsf + kStageF4 * 4 + b * (4 * SG * 3 * 64);
    float* const mine = red + wave * 3 * 64;
    mine[lane] = rx.x + rx.y;
    mine[64 + lane] = ry.x + ry.y;
    mine[128 + lane] = rz.x + rz.y;
    if (tg == 3 && c + 1 < CPS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // chunk c + 1 has landed
    __syncthreads();
    if (tg < 3) {
      const float* rs = red + (sg * 4) * 3 * 64 + tg * 64 + lane;
      const float v = ((rs[0] + rs[3 * 64]) + rs[6 * 64]) + rs[9 * 64];
      *o_react = init ? v : old + v;
    }
  }

  // own sums: the SG source groups of a target group in order, through LDS (staging and reaction space are free)
  float* const o_own = out + ((size_t)slot * n + row0) * 3;
  const f2 own[6] = {axa, aya, aza, axb, ayb, azb};
  if (SG == 1) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int comp = 0; comp < 3; ++comp) {
        const f2 v2 = own[(t >> 1) * 3 + comp];
        const float v = (t & 1) ? v2.y : v2.x;
        float* o = o_own + t * 64 * 3 + comp;
        *o = init ? v : *o + v;
      }
    return;
  }
  __syncthreads();  // every reduction read of the last chunk is done
  float* const mo = ldsf + (sg * 4 + tg) * 12 * 64;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const f2 v2 = own[(t >> 1) * 3 + comp];
      mo[(comp * 4 + t) * 64 + lane] = (t & 1) ? v2.y : v2.x;
    }
  __syncthreads();
  if (sg != 0) return;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const float* src = ldsf + tg * 12 * 64 + (comp * 4 + t) * 64 + lane;
      float v = src[0];
#pragma unroll
      for (int g = 1; g < SG; ++g) v += src[g * 4 * 12 * 64];
      float* o = o_own + t * 64 * 3 + comp;
      *o = init ? v : *o + v;
    }
}

// ---- variant 2 of the symmetric force: the packed halves of the VALU hold two SOURCES instead of two targets.
// accel_sym_kernel packs by target, so both halves of its reaction registers act on the one source of the step and each
// source pays 6 DPP moves. Here a step takes source s of chunk c in the .x halves and source s of chunk c + 8 in the .y
// halves; a target's coordinate is broadcast into both halves (op_sel), the own sums are {from c, from c + 8} (added once
// at the end) and the reaction {R_c, R_c+8} covers both sources: 6 DPP moves per two sources.
//
// One workgroup = one tile pair (a, b) of the same circle-method rounds as accel_sym_kernel (same slots, store/add rule).
// 8 waves: target group tg = wave & 1 holds the 512 targets a*S + tg*512 + 64 t + lane (t = 0..7) in registers, source
// group sg = wave >> 1 walks the chunk pairs (p, p + 8), p = 2 sg, 2 sg + 1, of tile b. Tile b is staged once, at the
// start, into an interleaved LDS image: per chunk pair, [128] {x_c, x_c+8, y_c, y_c+8} and [128] {z_c, z_c+8}, each chunk
// stored twice so that step k of lane l reads entry l + k at immediate offset k (one ds_read_b128 + one ds_read_b64, no
// wrap, no repacking). Per step and lane: 8 targets x 2 sources = 24 v_pk_add + 72 v_pk_fma + 16 v_pk_mul + 16 v_rsq +
// 6 DPP moves (37.5 issue cycles per lane-pair against 42 for accel_sym_kernel). The reactions of a chunk pair go to LDS
// without a barrier; after the walk the 2 target groups' reactions are added in order, then the 4 source groups' own
// sums, each row written once per (slot, row). Unscaled sums; needs the tile pair in the core (m >= 2).
constexpr int kSym2Pairs = kSymChunks / 2;   // chunk pairs (p, p + 8) of a tile
constexpr int kSym2T = 8;                    // targets per lane
constexpr int kSym2G = 2;                    // targets per scheduling group of the step (4: 128 VGPRs, 3 s_nop)
constexpr int kSym2XyF = kSym2Pairs * 128 * 4;   // [pair][128] {x, x', y, y'}
constexpr int kSym2ZF = kSym2Pairs * 128 * 2;    // [pair][128] {z, z'}
constexpr int kSym2ReactF = 2 * 8 * 6 * 64;      // [j][wave][comp * 2 + half][lane]
constexpr int kSym2OwnF = 8 * 3 * kSym2T * 64;   // [sg][tg][comp][t][lane], over all of the above after the walk
static_assert(kSym2XyF + kSym2ZF + kSym2ReactF == kSym2OwnF, "one 48-KiB LDS image");
constexpr int kSym2LdsF4 = kSym2OwnF / 4;        // the workgroup's f4[kSym2LdsF4], ONE object (keeps hipcc's waits sane)

// The tile pair of workgroup wg of the launch that starts at round r0, by the 512 threads of a workgroup: the body of
// accel_sym2_kernel and of the leading workgroups of accel_sym2_tail_kernel.
__device__ __forceinline__ void sym2_body(const f4* __restrict__ posm, int n, int m, int r0, int n_slots, int wg,
                                          float eps2, float* __restrict__ out, f4* lds) {
  constexpr int kXyF = kSym2XyF, kZF = kSym2ZF;
  float* const ldsf = reinterpret_cast<float*>(lds);
  f4* const xy = lds;
  f2* const zz = reinterpret_cast<f2*>(ldsf + kXyF);
  float* const react = ldsf + kXyF + kZF;

  int ta, tb, slot;
  bool init;
  sym_round_match(wg, m, r0, n_slots, ta, tb, slot, init);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tg = wave & 1, sg = wave >> 1;
  {  // stage tile b: thread (p = wave, lane) takes source lane of chunks p and p + 8
    const f4 u = posm[tb * kSymTile + wave * kChunk + lane];
    const f4 v = posm[tb * kSymTile + (wave + kSym2Pairs) * kChunk + lane];
    const f4 q = {u.x, v.x, u.y, v.y};
    const f2 z = {u.z, v.z};
    xy[wave * 128 + lane] = q; xy[wave * 128 + 64 + lane] = q;
    zz[wave * 128 + lane] = z; zz[wave * 128 + 64 + lane] = z;
  }
  const int row0 = ta * kSymTile + tg * 512 + lane;
  // targets as register pairs {x_t, y_t} and {z_t, z_t+1}: a coordinate reaches both halves of a packed op by op_sel
  f2 txy[kSym2T], tzz[kSym2T / 2];
  f2 ax[kSym2T], ay[kSym2T], az[kSym2T];
#pragma unroll
  for (int t = 0; t < kSym2T; ++t) {
    const f4 q = posm[row0 + t * 64];
    txy[t] = f2{q.x, q.y};
    if (t & 1) tzz[t >> 1].y = q.z; else tzz[t >> 1].x = q.z;
    ax[t] = ay[t] = az[t] = f2{0.f, 0.f};
  }
  f2 e2 = {eps2, eps2};
  asm volatile("" : "+v"(e2));  // keep eps^2 in VGPRs: an SGPR operand halves v_pk_fma issue
  __syncthreads();

#pragma unroll 1
  for (int j = 0; j < 2; ++j) {
    const int p = sg * 2 + j;
    const f4* const bxy = xy + p * 128 + lane;
    const f2* const bz = zz + p * 128 + lane;
    f2 rx = {0.f, 0.f}, ry = {0.f, 0.f}, rz = {0.f, 0.f};
#pragma unroll 1
    for (int k = 0; k < kChunk; ++k) {
      const f4 a = bxy[k];
      const f2 sx = {a.x, a.y}, sy = {a.z, a.w}, sz = bz[k];
      // opaque per step, or hipcc hoists the splats {x_t, x_t} out of the loop (24 more VGPRs)
#pragma unroll
      for (int t = 0; t < kSym2T; ++t) asm volatile("" : "+v"(txy[t]));
#pragma unroll
      for (int t = 0; t < kSym2T / 2; ++t) asm volatile("" : "+v"(tzz[t]));
#pragma unroll
      for (int g = 0; g < kSym2T; g += kSym2G) {
        // each stage over the whole group, fenced by sched_barrier: left alone, hipcc runs each target's chain back to back
        // and pads a wait state (s_nop) between every dependent packed op or rsq and its producer, 31 per step
        f2 dx[kSym2G], dy[kSym2G], dz[kSym2G], s[kSym2G], w[kSym2G];
#pragma unroll
        for (int u = 0; u < kSym2G; ++u) {
          const int t = g + u;
          const float tz = (t & 1) ? tzz[t >> 1].y : tzz[t >> 1].x;
          dx[u] = sx - f2{txy[t].x, txy[t].x}; dy[u] = sy - f2{txy[t].y, txy[t].y}; dz[u] = sz - f2{tz, tz};  // r_j - r_i
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kSym2G; ++u) s[u] = __builtin_elementwise_fma(dx[u], dx[u], e2);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kSym2G; ++u) s[u] = __builtin_elementwise_fma(dy[u], dy[u], s[u]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kSym2G; ++u) s[u] = __builtin_elementwise_fma(dz[u], dz[u], s[u]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kSym2G; ++u) s[u] = f2{__builtin_amdgcn_rsqf(s[u].x), __builtin_amdgcn_rsqf(s[u].y)};
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kSym2G; ++u) w[u] = s[u] * s[u];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kSym2G; ++u) w[u] = w[u] * s[u];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kSym2G; ++u) {
          const int t = g + u;
          ax[t] = __builtin_elementwise_fma(w[u], dx[u], ax[t]);
          ay[t] = __builtin_elementwise_fma(w[u], dy[u], ay[t]);
          az[t] = __builtin_elementwise_fma(w[u], dz[u], az[t]);
          rx = __builtin_elementwise_fma(-w[u], dx[u], rx);
          ry = __builtin_elementwise_fma(-w[u], dy[u], ry);
          rz = __builtin_elementwise_fma(-w[u], dz[u], rz);
        }
      }
      rx = f2{rol1(rx.x), rol1(rx.y)};
      ry = f2{rol1(ry.x), rol1(ry.y)};
      rz = f2{rol1(rz.x), rol1(rz.y)};
    }
    float* const mine = react + (j * 8 + wave) * 6 * 64 + lane;
    mine[0 * 64] = rx.x; mine[1 * 64] = rx.y;
    mine[2 * 64] = ry.x; mine[3 * 64] = ry.y;
    mine[4 * 64] = rz.x; mine[5 * 64] = rz.y;
  }
  // An adding launch needs what an earlier launch stored in its rows (written from other XCDs: they come from the
  // Infinity Cache or HBM, not the local L2). The walk's registers are dead here, so all twelve values of a thread are
  // requested at once, in front of the barrier: one exposed round trip. (Fetched trip by trip inside the two passes
  // below -- load, wait, add, store, six times each -- they cost 3.7 us of a 156-us launch, now 1.3 us.)
  float* const o_b = out + ((size_t)slot * n + (size_t)tb * kSymTile) * 3;
  float* const o_a = out + ((size_t)slot * n + (size_t)ta * kSymTile) * 3;
  float oldb[6], olda[6];
  if (!init) {
#pragma unroll
    for (int i = 0; i < 6; ++i) oldb[i] = o_b[threadIdx.x + i * 512];
#pragma unroll
    for (int i = 0; i < 6; ++i) olda[i] = o_a[threadIdx.x + i * 512];
  }
  __syncthreads();

  // reactions: rows of tile b, target group 0 + target group 1; one coalesced pass over the tile's 1024 x 3 floats
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int o = threadIdx.x + i * 512;
    const int row = o / 3, comp = o - row * 3;
    const int c = row >> 6, l = row & 63, p = c & (kSym2Pairs - 1), hf = c / kSym2Pairs;
    const float* rs = react + ((p & 1) * 8 + (p >> 1) * 2) * 6 * 64 + (comp * 2 + hf) * 64 + l;
    const float v = rs[0] + rs[6 * 64];
    o_b[o] = init ? v : oldb[i] + v;
  }
  __syncthreads();  // every reaction read is done: the LDS image takes the own sums
#pragma unroll
  for (int t = 0; t < kSym2T; ++t) {
    float* const mo = ldsf + ((sg * 2 + tg) * 3 * kSym2T + t) * 64 + lane;
    mo[0 * kSym2T * 64] = ax[t].x + ax[t].y;
    mo[1 * kSym2T * 64] = ay[t].x + ay[t].y;
    mo[2 * kSym2T * 64] = az[t].x + az[t].y;
  }
  __syncthreads();
  // own sums: rows of tile a, the 4 source groups in order
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int o = threadIdx.x + i * 512;
    const int row = o / 3, comp = o - row * 3;
    const int g = row >> 9, t = (row >> 6) & (kSym2T - 1), l = row & 63;
    const float* os = ldsf + ((g * 3 + comp) * kSym2T + t) * 64 + l;
    constexpr int kSg = 2 * 3 * kSym2T * 64;
    const float v = ((os[0] + os[kSg]) + os[2 * kSg]) + os[3 * kSg];
    o_a[o] = init ? v : olda[i] + v;
  }
}

__global__ __launch_bounds__(512, 4) void accel_sym2_kernel(const f4* __restrict__ posm, int n, int m, int r0,
                                                            int n_slots, float eps2, float* __restrict__ out) {
  __shared__ f4 lds[kSym2LdsF4];
  sym2_body(posm, n, m, r0, n_slots, blockIdx.x, eps2, out, lds);
}

// ---- the whole core in ONE launch, for the plan with a slot per round (K = M): workgroups [0, M (M - 1) / 2) are the
// tile pairs of accel_sym2_kernel, all rounds storing into slots 1 .. M - 1; the 4 M workgroups behind them run the
// diagonal blocks into slot 0, with the arithmetic and the summation order of the diagonal launch of launch_sym
// (accel_kernel<false, 8, true> on 8 groups x 1 slab per tile: accel_body<8, true> and the plan of 16 chunks over 4
// waves). A trailing workgroup is two such groups of 4 waves side by side, group 2 d + h of the M x 8 in half h of
// workgroup d, each half on its own accel_body LDS region of the 48-KiB object (2 x 14 KiB); both halves walk 4 chunks
// per wave and meet at accel_body's one barrier. Workgroups are handed out in index order, so the diagonal groups come
// last: they take the slots the fourth residency round leaves empty (N = 65 536: 2016 pair jobs in 4 x 512 slots) and
// the slots that finished pair jobs free, where a launch of their own ran at 2 waves per SIMD behind a launch boundary.
// No two workgroups write the same (slot, row): no order between them is needed.
__global__ __launch_bounds__(512, 4) void accel_sym2_tail_kernel(const f4* __restrict__ posm, int n, int m, float eps2,
                                                                 float* __restrict__ out) {
  __shared__ f4 lds[kSym2LdsF4];
  static_assert(2 * kAccelLdsF4 <= kSym2LdsF4, "two accel_body regions in the tile-pair image");
  const int pairs = (m >> 1) * (m - 1);
  if ((int)blockIdx.x < pairs) {
    sym2_body(posm, n, m, 0, m, blockIdx.x, eps2, out, lds);
    return;
  }
  const int half = __builtin_amdgcn_readfirstlane(threadIdx.x >> 8);
  const int g = ((int)blockIdx.x - pairs) * 2 + half;          // group g of the M x 8 diagonal groups
  constexpr int kGroups = kSymTile / kTgtPerWG;
  const int tz = (g / kGroups) * kSymTile, t_base = (g % kGroups) * kTgtPerWG;
  const SrcView sv = full_view(kSymTile, kSymChunks, 1);
  accel_body<8, true>(posm + tz, sv, std::false_type{}, posm + tz, kSymTile, 0, t_base, 0, eps2, 1.0f,
                      lds + half * kAccelLdsF4, out + ((size_t)tz + t_base) * 3, (int)(threadIdx.x & 255));
}

// acc = g * (slab_0 + slab_1 + ...), optional fused kick v += c * acc (simulation.py:88,170).
// Block = 4 waves on 64 consecutive outputs: wave w sums slabs w, w+4, w+8, ... (coalesced 256-B loads, all
// in flight), the four partial sums are combined as (p0 + p1) + (p2 + p3) through LDS -- a fixed association,
// so the result is bit-reproducible. One thread per output summing every slab serially took 9 us for the
// 28 slabs x 24 576 outputs of a sharded rank (96 workgroups, one dependent chain each); this form 3 us.
__global__ __launch_bounds__(256) void finish_kernel(const float* __restrict__ slabs, int n_slabs,
                                                     size_t slab_stride, float g, float* __restrict__ acc,
                                                     float* __restrict__ vel, float c_kick, int n3) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  float sum = 0.f;
  if (i < n3)
    for (int s = w; s < n_slabs; s += 4) sum += slabs[s * slab_stride + i];
  part[w][lane] = sum;
  __syncthreads();
  if (w != 0 || i >= n3) return;
  const float a = __fmul_rn(g, (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]));
  acc[i] = a;
  if (vel) vel[i] = __fadd_rn(vel[i], __fmul_rn(c_kick, a));
}

__global__ __launch_bounds__(256) void pack_kernel(const float* __restrict__ pos,
                                                   const float* __restrict__ mass, int n, int n_pad,
                                                   f4* __restrict__ posm) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pad) return;
  f4 v = {0.f, 0.f, 0.f, 0.f};
  if (i < n) v = f4{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], mass[i]};
  posm[i] = v;
}

// v += ck*a ; x += cd*v ; posm = {x, m}. mul and add round separately (torch eager order).
__global__ __launch_bounds__(256) void kick_drift_kernel(float* __restrict__ pos, float* __restrict__ vel,
                                                         const float* __restrict__ acc,
                                                         const float* __restrict__ mass, int n, int n_pad,
                                                         float ck, float cd, f4* __restrict__ posm) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pad) return;
  f4 pm = {0.f, 0.f, 0.f, 0.f};
  if (i < n) {
    float x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float v = vel[3 * i + k];
      if (acc) { v = __fadd_rn(v, __fmul_rn(ck, acc[3 * i + k])); vel[3 * i + k] = v; }
      x[k] = __fadd_rn(pos[3 * i + k], __fmul_rn(cd, v));
      pos[3 * i + k] = x[k];
    }
    pm = f4{x[0], x[1], x[2], mass ? mass[i] : 0.f};
  }
  if (posm) posm[i] = pm;
}

// zero fill by kernel, not hipMemsetAsync: memset nodes captured into a hipGraph were observed not to
// re-execute on replay on this stack (see csrc/graph.hip), and every entry point here must be capturable
__global__ __launch_bounds__(256) void zero_f32_kernel(float* __restrict__ p, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0.f;
}

// state snapshot of one step into a device ring slot: out = [pos | vel | acc], each (n,3) -- BaseSimulator.run's
// per-step clones (simulation.py:135-139) as ONE launch that a captured chunk of steps can contain
// (T = float, or double for the float64 Hermite simulators)
template <class T>
__global__ __launch_bounds__(256) void snapshot_kernel(const T* __restrict__ pos, const T* __restrict__ vel,
                                                       const T* __restrict__ acc, int n3, T* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n3) return;
  out[i] = pos[i]; out[n3 + i] = vel[i]; out[2 * n3 + i] = acc[i];
}

__global__ __launch_bounds__(256) void axpy_kernel(float* __restrict__ y, const float* __restrict__ x,
                                                   float c, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = __fadd_rn(y[i], __fmul_rn(c, x[i]));
}

__global__ __launch_bounds__(64 * kWaves) void energy_kernel(const f4* __restrict__ posm, int n, int n_chunks,
                                                             float soft_, int all_masked,
                                                             double* __restrict__ partial_u) {
  __shared__ f4 lds[kEnergyLdsF4];
  energy_body(posm, n, n_chunks, blockIdx.x * kTgtPerWG, blockIdx.y, gridDim.y, soft_, all_masked, lds,
              partial_u + (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

__global__ __launch_bounds__(256) void kinetic_kernel(const f4* __restrict__ posm, const float* __restrict__ vel,
                                                      int n, double* __restrict__ partial_k) {
  __shared__ double red[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double k = 0.0;
  if (i < n) {
    const float vx = vel[3 * i], vy = vel[3 * i + 1], vz = vel[3 * i + 2];
    const float v2 = __fadd_rn(__fadd_rn(__fmul_rn(vx, vx), __fmul_rn(vy, vy)), __fmul_rn(vz, vz));
    k = (double)__fmul_rn(__fmul_rn(0.5f, posm[i].w), v2);                // 0.5 * m * |v|^2 (:100)
  }
  for (int off = 32; off > 0; off >>= 1) k += __shfl_down(k, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = k;
  __syncthreads();
  if (threadIdx.x == 0) partial_k[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void energy_final_kernel(const double* __restrict__ pu, int nu,
                                                           const double* __restrict__ pk, int nk, float g,
                                                           double* __restrict__ out) {
  __shared__ double ru[4], rk[4];
  double u = 0.0, k = 0.0;
  for (int b = threadIdx.x; b < nu; b += 256) u += pu[b];
  for (int b = threadIdx.x; b < nk; b += 256) k += pk[b];
  for (int off = 32; off > 0; off >>= 1) { u += __shfl_down(u, off); k += __shfl_down(k, off); }
  if ((threadIdx.x & 63) == 0) { ru[threadIdx.x >> 6] = u; rk[threadIdx.x >> 6] = k; }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = -(double)g * ((ru[0] + ru[1]) + (ru[2] + ru[3]));
    out[1] = (rk[0] + rk[1]) + (rk[2] + rk[3]);
  }
}

inline int energy_slabs(int groups) {
  int s = (4096 + groups - 1) / groups;        // ~2 residency rounds; the triangle is balanced dynamically
  return s < 1 ? 1 : (s > 32 ? 32 : s);
}

struct AccelPlan { int groups, slabs, n_chunks, cpw, variant; };   // cpw = the LARGEST chunk count of a wave

// an explicit geometry: groups x slabs workgroups on n_chunks logical source chunks
AccelPlan make_plan(int groups, int slabs, int n_chunks, int variant = 0) {
  return AccelPlan{groups, slabs, n_chunks, ceil_div(n_chunks, slabs * kWaves), variant};
}

// Launch geometry for `n_chunks` logical source chunks against n_tgt targets.
//
// A workgroup is 4 waves (one per SIMD of its CU) on 128 targets; the kernel is VALU-issue bound, so a
// launch costs (to first order) the largest number of chunk-times any SIMD is handed:
//     cost(slabs) = [workgroups per CU] x [chunks per wave]       (workgroups go to the CUs round-robin)
// divided by the issue efficiency at that many waves per SIMD and plus a per-workgroup prologue/epilogue
// term. Fitted to the hardware sweep of every slab count (nbd_accel_tuned_f32, tools/sweep_accel_plan.py,
// profiles/r02_plan_sweep*.jsonl): e.g. 8192 targets x 57 344 sources (the remote block of one of 8 ranks):
// 2/3/4/>=5 workgroups per CU at equal chunk totals ran at 0.935/0.975/0.99/1.0 of the best rate, a slab
// count that leaves the work uneven across CUs (9 slabs: 576 workgroups) 30 % slower. Large launches keep
// ~32 workgroups per CU with >= 16 chunks (1024 sources) per wave: the tail then balances dynamically.
constexpr int kCUs = 256;
double plan_cost(int groups, int n_chunks, int slabs) {
  static const double eff[6] = {1.0, 0.70, 0.935, 0.975, 0.99, 1.0};
  const int waves = slabs * kWaves, q = n_chunks / waves, r = n_chunks % waves;
  const int wgs = groups * slabs, per_cu = ceil_div(wgs, kCUs);
  const int heavy_per_cu = ceil_div(groups * ceil_div(r, kWaves), kCUs);   // workgroups holding a (q+1)-chunk wave
  const double chunks = (double)per_cu * q + (heavy_per_cu < per_cu ? heavy_per_cu : per_cu);
  // exactly one residency round (<= 5 workgroups per CU) has no slack for uneven placement: +3 % measured
  // (128 groups x 10 slabs: 268 us, x 20 slabs: 261 us); 0.25 chunk-times of prologue/epilogue per workgroup
  return chunks / eff[per_cu < 5 ? per_cu : 5] * (per_cu <= 5 ? 1.03 : 1.0) + 0.25 * per_cu;
}

AccelPlan plan_chunks(int n_chunks, int n_tgt) {
  AccelPlan p;
  p.variant = 0;
  p.groups = ceil_div(n_tgt, kTgtPerWG);
  p.n_chunks = n_chunks;
  int cap = n_chunks / kWaves;                     // at least one chunk per wave
  cap = cap < 1 ? 1 : (cap > kMaxSlabs ? kMaxSlabs : cap);
  int slabs;
  const int pref = ceil_div(8192, p.groups), cap_pref = n_chunks / (16 * kWaves);
  if ((pref < cap_pref ? pref : cap_pref) * p.groups >= 10 * kCUs) {
    slabs = pref < cap_pref ? pref : cap_pref;
    // accuracy: a wave adds its sources in one sequential fp32 chain, so very large systems get enough slabs to keep
    // a chain <= 64 chunks (4096 sources): at N = 524 288 two slabs (65 536-source chains) measured 3e-6 per-row
    // against fp64, 32 slabs 1e-6; the extra slab traffic is < 0.1 % of such a step
    const int min_slabs = ceil_div(n_chunks, kWaves * 64);
    if (slabs < min_slabs) slabs = min_slabs;
  } else {
    slabs = 1;
    double best = plan_cost(p.groups, n_chunks, 1);
    for (int s = 2; s <= cap; ++s) {
      const double c = plan_cost(p.groups, n_chunks, s);
      if (c < best * 0.999) { best = c; slabs = s; }       // ties: fewer slabs to sum
    }
  }
  if (slabs > kMaxSlabs) slabs = kMaxSlabs;
  if (slabs < 1) slabs = 1;
  p.slabs = slabs;
  p.cpw = ceil_div(n_chunks, p.slabs * kWaves);
  return p;
}

AccelPlan plan_accel(int n_src, int n_tgt) { return plan_chunks(ceil_div(n_src, kChunk), n_tgt); }

inline int check(hipError_t e) { return e == hipSuccess ? 0 : (int)e; }

// all sources of an n_src array, split as the plan says
SrcView full_view(int n_src, const AccelPlan& p) { return full_view(n_src, p.n_chunks, p.slabs); }

// force into slabs (or straight into acc_out when one slab), no finishing pass
int launch_accel(const float* posm_src, SrcView sv, const float* posm_tgt, int n_tgt, int off,
                 float eps2, float direct_scale, float* slabs_or_acc, const AccelPlan& p,
                 hipStream_t st, bool uniform = false, int out_rows = 0, int tiles = 1, int tile_len = 0) {
  dim3 grid(p.groups, p.slabs, tiles), block(64 * kWaves);
  if (out_rows <= 0) out_rows = n_tgt;
  const f4* s = reinterpret_cast<const f4*>(posm_src);
  const f4* t = reinterpret_cast<const f4*>(posm_tgt);
  split_chunks(sv, p.n_chunks, p.slabs);
  const bool masked = eps2 < kEps2Masked;
#define NBD_LAUNCH(M, K, U) accel_kernel<M, K, U><<<grid, block, 0, st>>>(s, sv, t, n_tgt, off, eps2, direct_scale, slabs_or_acc, out_rows, tile_len)
  if (uniform) {
    if (p.variant == 1) { if (masked) NBD_LAUNCH(true, 4, true); else NBD_LAUNCH(false, 4, true); }
    else                { if (masked) NBD_LAUNCH(true, 8, true); else NBD_LAUNCH(false, 8, true); }
  } else {
    if (p.variant == 1) { if (masked) NBD_LAUNCH(true, 4, false); else NBD_LAUNCH(false, 4, false); }
    else                { if (masked) NBD_LAUNCH(true, 8, false); else NBD_LAUNCH(false, 8, false); }
  }
#undef NBD_LAUNCH
  return launch_status();
}

// ---- the symmetric force's launch plan (accel_sym_kernel): M even tiles of kSymTile, K slots, the remainder rows
// [core, n) in one more slot
struct SymPlan { int m, core, rem, slots, total_slots; };

// K = the widest plan that slots_avail slots of n rows hold: min(M, kSymSlotsCap, slots_avail less the remainder's slot),
// and never below the narrow plan's min(M, kSymSlots), which is what the callers check the workspace against. With
// K = M every round has a slot of its own: all rounds store, in ONE launch; with K < M the first K - 1 rounds store and
// launches of K rounds add.
SymPlan plan_sym(int n, int slots_avail = 0) {
  SymPlan p;
  p.m = n / kSymTile;
  p.m &= ~1;                                  // the circle method pairs an even number of tiles
  p.core = p.m * kSymTile;
  p.rem = n - p.core;
  const int narrow = p.m < kSymSlots ? p.m : kSymSlots, wide = p.m < kSymSlotsCap ? p.m : kSymSlotsCap;
  const int avail = slots_avail - (p.rem > 0 ? 1 : 0);
  p.slots = avail < narrow ? narrow : (avail < wide ? avail : wide);
  p.total_slots = p.slots + (p.rem > 0 ? 1 : 0);
  return p;
}

// the narrow plan's workspace: the least a symmetric call takes
size_t sym_workspace_bytes(int n) {
  const SymPlan p = plan_sym(n);
  return p.m < 2 ? 0 : (size_t)p.total_slots * n * 3 * sizeof(float);
}

// how many slots of n rows a workspace holds (capped: the plan never uses more than kSymSlotsCap + 1)
int sym_slots_avail(int n, size_t workspace_bytes) {
  const size_t s = workspace_bytes / ((size_t)n * 3 * sizeof(float));
  return s > (size_t)kSymSlotsCap + 1 ? kSymSlotsCap + 1 : (int)s;
}

// the workspace of the preferred plan: K = min(M, kSymSlotsPref)
size_t sym_workspace_pref_bytes(int n) {
  const SymPlan p = plan_sym(n);
  if (p.m < 2) return 0;
  const int k = p.m < kSymSlotsPref ? p.m : kSymSlotsPref;
  return (size_t)(k + (p.rem > 0 ? 1 : 0)) * n * 3 * sizeof(float);
}

// the uniform-mass leapfrog step takes the symmetric force from this size on
constexpr int kSymStepMinN = 65536;
bool sym_step(int n, float eps2) { return n >= kSymStepMinN && eps2 >= kEps2Masked; }

// unscaled sum_j d_ij s_ij^3 of every row into slots [0, total_slots) of float[total_slots][n][3]; needs m >= 2 and
// eps2 >= kEps2Masked (the i == j term of a diagonal block is then an exact zero)
// variant 0: 4 source groups (16-wave workgroups, 64 VGPRs, 2 per CU: 8 waves per SIMD); 1: 2 source groups (8 waves,
// 86 VGPRs: 4 waves per SIMD); 2: accel_sym2_kernel (two sources per step, 8 waves, <= 128 VGPRs: 4 waves per SIMD)
// kSymTailVariant (no number of the C-ABI): variant 2 with the diagonal blocks as the trailing workgroups of the one
// pair launch where every round has its own slot (accel_sym2_tail_kernel); with K < M an adding round reads slot 0, the
// diagonal launch has to come first and this IS variant 2.
constexpr int kSymTailVariant = 3;
int launch_sym(const float* posm, int n, float eps2, float* slots, const SymPlan& sp, hipStream_t st, int variant = 0) {
  const f4* pm = reinterpret_cast<const f4*>(posm);
  const bool tail = variant == kSymTailVariant && sp.slots == sp.m;
  if (variant == kSymTailVariant) variant = 2;
  int rc = 0;
  if (tail) {
    accel_sym2_tail_kernel<<<(sp.m / 2) * (sp.m - 1) + sp.m * (kSymTile / kTgtPerWG) / 2, 512, 0, st>>>(pm, n, sp.m,
                                                                                                      eps2, slots);
    if ((rc = launch_status())) return rc;
  } else {
    // the diagonal blocks (a, a): the all-pairs kernel on each tile, slot 0
    const AccelPlan dp = make_plan(kSymTile / kTgtPerWG, 1, kSymChunks);
    rc = launch_accel(posm, full_view(kSymTile, dp), posm, kSymTile, 0, eps2, 1.0f, slots, dp, st, true, n, sp.m,
                      kSymTile);
    if (rc) return rc;
  }
  // the off-diagonal rounds: [0, K-1) stores, then launches of K rounds add (the tail launch has run them all)
  const int rounds = sp.m - 1;
  for (int r0 = tail ? rounds : 0; r0 < rounds;) {
    const int r1 = r0 == 0 ? (sp.slots - 1 < rounds ? sp.slots - 1 : rounds) : (r0 + sp.slots < rounds ? r0 + sp.slots : rounds);
    const int wgs = (r1 - r0) * (sp.m / 2);
    if (variant == 2) accel_sym2_kernel<<<wgs, 512, 0, st>>>(pm, n, sp.m, r0, sp.slots, eps2, slots);
    else if (variant == 1) accel_sym_kernel<2><<<wgs, 512, 0, st>>>(pm, n, sp.m, r0, sp.slots, eps2, slots);
    else accel_sym_kernel<4><<<wgs, 1024, 0, st>>>(pm, n, sp.m, r0, sp.slots, eps2, slots);
    if ((rc = launch_status())) return rc;
    r0 = r1;
  }
  if (sp.rem == 0) return 0;
  // remainder rows [core, n) against all n sources, split over every slot (the symmetric launches never write them)
  const AccelPlan tp = make_plan(ceil_div(sp.rem, kTgtPerWG), sp.total_slots, ceil_div(n, kChunk));
  rc = launch_accel(posm, full_view(n, tp), posm + (size_t)sp.core * 4, sp.rem, sp.core, eps2, 1.0f,
                    slots + (size_t)sp.core * 3, tp, st, true, n);
  if (rc) return rc;
  // core rows against the remainder sources: the last slot
  SrcView sv;
  const AccelPlan cp = make_plan(sp.core / kTgtPerWG, 1, excluded_view(n, 0, sp.core, &sv));
  return launch_accel(posm, sv, posm, sp.core, 0, eps2, 1.0f, slots + (size_t)sp.slots * n * 3, cp, st, true, n);
}

}  // namespace

extern "C" {

int nbd_abi_version(void) { return NBD_ABI_VERSION; }

size_t nbd_struct_size(const char* name) {
  if (!name) return 0;
#define NBD_SZ(T) if (!strcmp(name, #T)) return sizeof(T);
  NBD_SZ(nbd_gnn_layer_args) NBD_SZ(nbd_gnn_forward_args) NBD_SZ(nbd_knn_pq_args) NBD_SZ(nbd_gnn_train_args)
  NBD_SZ(nbd_gnn_train_grads) NBD_SZ(nbd_cc_train_args) NBD_SZ(nbd_cc_train_grads) NBD_SZ(nbd_cc_pairs_job)
#undef NBD_SZ
  return 0;
}

const char* nbd_strerror(int code) {
  if (code == 0) return "ok";
  if (code == NBD_E_BADARG) return "nbd: bad argument (null/negative/misaligned)";
  if (code == NBD_E_WORKSPACE) return "nbd: workspace too small";
  if (code == NBD_E_UNSUPPORTED) return "nbd: unsupported configuration";
  if (code > 0) return hipGetErrorString((hipError_t)code);
  return "nbd: unknown error";
}

int nbd_posm_padded_len(int n) { return n <= 0 ? 0 : ceil_div(n, kChunk) * kChunk; }

int nbd_pack_posm_f32(const float* pos, const float* mass, int n, float* posm, nbd_stream_t stream) {
  if (n < 0 || (n > 0 && (!pos || !mass || !posm)) || misaligned16(posm)) return NBD_E_BADARG;
  if (n == 0) return 0;
  const int n_pad = nbd_posm_padded_len(n);
  pack_kernel<<<ceil_div(n_pad, 256), 256, 0, (hipStream_t)stream>>>(pos, mass, n, n_pad,
                                                                    reinterpret_cast<f4*>(posm));
  return launch_status();
}

size_t nbd_accel_workspace_bytes(int n_src, int n_tgt) {
  if (n_src <= 0 || n_tgt <= 0) return 0;
  const AccelPlan p = plan_accel(n_src, n_tgt);
  return p.slabs > 1 ? (size_t)p.slabs * n_tgt * 3 * sizeof(float) : 0;
}

int nbd_accel_plan(int n_src, int n_tgt, int* groups, int* slabs, int* chunks_per_wave) {
  if (n_src <= 0 || n_tgt <= 0) return NBD_E_BADARG;
  const AccelPlan p = plan_accel(n_src, n_tgt);
  if (groups) *groups = p.groups;
  if (slabs) *slabs = p.slabs;
  if (chunks_per_wave) *chunks_per_wave = p.cpw;
  return 0;
}

size_t nbd_step_workspace_bytes(int n) {
  if (n <= 0) return 0;
  const size_t all_pairs = (size_t)plan_accel(n, n).slabs * n * 3 * sizeof(float);
  const size_t sym = sym_step(n, kEps2Masked) ? sym_workspace_bytes(n) : 0;
  return sym > all_pairs ? sym : all_pairs;
}

size_t nbd_step_workspace_pref_bytes(int n) {
  if (n <= 0) return 0;
  const size_t least = nbd_step_workspace_bytes(n);
  const size_t pref = sym_step(n, kEps2Masked) ? sym_workspace_pref_bytes(n) : 0;
  return pref > least ? pref : least;
}

size_t nbd_accel_sym_workspace_bytes(int n) { return n <= 0 ? 0 : sym_workspace_bytes(n); }

// the symmetric force on its own: launch_sym(variant) and the finishing pass
static int accel_sym_uniform(const float* posm, int n, float softening_sq, float g_const, float mass_value,
                             float* acc_out, void* workspace, size_t workspace_bytes, int variant, nbd_stream_t stream) {
  if (n < 0 || (n > 0 && (!posm || !acc_out)) || misaligned16(posm)) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (plan_sym(n).m < 2 || softening_sq < kEps2Masked) return NBD_E_UNSUPPORTED;
  if (!workspace || workspace_bytes < sym_workspace_bytes(n)) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* slots = static_cast<float*>(workspace);
  const SymPlan sp = plan_sym(n, sym_slots_avail(n, workspace_bytes));
  int rc = launch_sym(posm, n, softening_sq, slots, sp, st, variant);
  if (rc) return rc;
  const int n3 = 3 * n;
  finish_kernel<<<ceil_div(n3, 64), 256, 0, st>>>(slots, sp.total_slots, (size_t)n3, g_const * mass_value,
                                                   acc_out, nullptr, 0.f, n3);
  return launch_status();
}

int nbd_accel_sym_uniform_f32(const float* posm, int n, float softening_sq, float g_const, float mass_value,
                              float* acc_out, void* workspace, size_t workspace_bytes, int variant, nbd_stream_t stream) {
  if (variant < 0 || variant > 2) return NBD_E_BADARG;
  return accel_sym_uniform(posm, n, softening_sq, g_const, mass_value, acc_out, workspace, workspace_bytes, variant,
                           stream);
}

int nbd_accel_sym_tail_uniform_f32(const float* posm, int n, float softening_sq, float g_const, float mass_value,
                                   float* acc_out, void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  return accel_sym_uniform(posm, n, softening_sq, g_const, mass_value, acc_out, workspace, workspace_bytes,
                           kSymTailVariant, stream);
}

int nbd_accel_f32(const float* posm_src, int n_src, const float* posm_tgt, int n_tgt,
                  int tgt_global_offset, float softening_sq, float g_const, float* acc_out,
                  void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  if (n_src < 0 || n_tgt < 0) return NBD_E_BADARG;
  if (n_tgt == 0) return 0;
  if (!acc_out || !posm_tgt || misaligned16(posm_tgt)) return NBD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (n_src == 0) {
    zero_f32_kernel<<<ceil_div(n_tgt * 3, 256), 256, 0, st>>>(acc_out, (size_t)n_tgt * 3);
    return launch_status();
  }
  if (!posm_src || misaligned16(posm_src)) return NBD_E_BADARG;
  const AccelPlan p = plan_accel(n_src, n_tgt);
  if (p.slabs == 1)
    return launch_accel(posm_src, full_view(n_src, p), posm_tgt, n_tgt, tgt_global_offset, softening_sq,
                        g_const, acc_out, p, st);
  const size_t need = (size_t)p.slabs * n_tgt * 3 * sizeof(float);
  if (!workspace || workspace_bytes < need) return NBD_E_WORKSPACE;
  float* slabs = static_cast<float*>(workspace);
  int rc = launch_accel(posm_src, full_view(n_src, p), posm_tgt, n_tgt, tgt_global_offset, softening_sq,
                        1.0f, slabs, p, st);
  if (rc) return rc;
  const int n3 = n_tgt * 3;
  finish_kernel<<<ceil_div(n3, 64), 256, 0, st>>>(slabs, p.slabs, (size_t)n3, g_const, acc_out,
                                                   nullptr, 0.f, n3);
  return launch_status();
}

// ---- tuning hook: the force with an explicit launch geometry (tools/sweep_accel_plan.py, tests)
size_t nbd_accel_tuned_workspace_bytes(int n_tgt, int slabs) {
  if (n_tgt <= 0 || slabs <= 0) return 0;
  return (size_t)slabs * n_tgt * 3 * sizeof(float);
}

int nbd_accel_tuned_f32(const float* posm_src, int n_src, int exclude_lo, int exclude_hi, const float* posm_tgt,
                        int n_tgt, int tgt_global_offset, float softening_sq, float g_const, float* acc_out,
                        void* workspace, size_t workspace_bytes, int slabs, int variant, nbd_stream_t stream) {
  if (n_src <= 0 || n_tgt <= 0 || slabs < 1 || slabs > kMaxSlabs || variant < 0 || variant > 1) return NBD_E_BADARG;
  if (exclude_lo < 0 || exclude_hi < exclude_lo || exclude_hi > n_src) return NBD_E_BADARG;
  if (!acc_out || !posm_tgt || !posm_src || misaligned16(posm_tgt) || misaligned16(posm_src)) return NBD_E_BADARG;
  if (!workspace || workspace_bytes < nbd_accel_tuned_workspace_bytes(n_tgt, slabs)) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  SrcView sv;
  const AccelPlan p =
      make_plan(ceil_div(n_tgt, kTgtPerWG), slabs, excluded_view(n_src, exclude_lo, exclude_hi, &sv), variant);
  float* sl = static_cast<float*>(workspace);
  const int n3 = n_tgt * 3;
  if (p.n_chunks == 0) {
    zero_f32_kernel<<<ceil_div(n3, 256), 256, 0, st>>>(acc_out, (size_t)n3);
    return launch_status();
  }
  int rc = launch_accel(posm_src, sv, posm_tgt, n_tgt, tgt_global_offset, softening_sq, 1.0f, sl, p, st);
  if (rc) return rc;
  finish_kernel<<<ceil_div(n3, 64), 256, 0, st>>>(sl, p.slabs, (size_t)n3, g_const, acc_out, nullptr, 0.f, n3);
  return launch_status();
}

// ---- range-sharded step (one rank of a torch.distributed group). The rank's targets are its
// own bodies [lo, lo + n_local). The force is issued in two launches so that the all-gather of the other
// ranks' bodies can be in flight during the first:
//   local  : sources = the rank's own packed bodies (posm_local, just written by nbd_kick_drift_f32)
//   remote : sources = the gathered array without [lo, lo + n_local), then the fixed-order slab sum,
//            acc = G * sum, and the second kick fused (finish_kernel), as in nbd_leapfrog_step_f32.
struct ShardPlan { AccelPlan local, remote; };

ShardPlan plan_shard_uncached(int n_total, int lo, int n_local) {
  ShardPlan sp;
  sp.local = plan_chunks(ceil_div(n_local, kChunk), n_local);
  const int rc = excluded_view(n_total, lo, lo + n_local, nullptr);
  sp.remote = plan_chunks(rc > 0 ? rc : 1, n_local);
  if (rc == 0) { sp.remote.slabs = 0; sp.remote.n_chunks = 0; }
  return sp;
}

// A sharded step asks for its plan four times (two launches, each sizing its workspace first) and every plan is two
// searches of up to 64 cost evaluations -- host time on the critical path of a ~140 us rank step. The plan is a pure
// function of (n_total, lo, n_local): memoised per calling thread (a rank steps ONE partition; no locks, no shared state).
ShardPlan plan_shard(int n_total, int lo, int n_local) {
  struct Memo { int n_total, lo, n_local; ShardPlan sp; };
  thread_local Memo memo[4] = {{-1, 0, 0, {}}, {-1, 0, 0, {}}, {-1, 0, 0, {}}, {-1, 0, 0, {}}};
  thread_local int next = 0;
  for (const Memo& m : memo)
    if (m.n_total == n_total && m.lo == lo && m.n_local == n_local) return m.sp;
  Memo& m = memo[next];
  next = (next + 1) & 3;
  m.n_total = n_total; m.lo = lo; m.n_local = n_local;
  m.sp = plan_shard_uncached(n_total, lo, n_local);
  return m.sp;
}

int nbd_shard_plan(int n_total, int lo, int n_local, int* slabs_local, int* cpw_local, int* slabs_remote,
                   int* cpw_remote) {
  if (!shard_args_ok(n_total, lo, n_local) || n_local == 0) return NBD_E_BADARG;
  const ShardPlan sp = plan_shard(n_total, lo, n_local);
  if (slabs_local) *slabs_local = sp.local.slabs;
  if (cpw_local) *cpw_local = sp.local.cpw;
  if (slabs_remote) *slabs_remote = sp.remote.slabs;
  if (cpw_remote) *cpw_remote = sp.remote.cpw;
  return 0;
}

size_t nbd_shard_workspace_bytes(int n_total, int lo, int n_local) {
  if (!shard_args_ok(n_total, lo, n_local) || n_local == 0) return 0;
  const ShardPlan sp = plan_shard(n_total, lo, n_local);
  return (size_t)(sp.local.slabs + sp.remote.slabs) * n_local * 3 * sizeof(float);
}

// the rank's own block: targets and sources are the same array, the diagonal is at j == i (offset 0)
static int shard_force_local(const float* posm_local, int n_local, float softening_sq, void* workspace,
                             size_t workspace_bytes, int n_total, int lo, nbd_stream_t stream, bool uniform) {
  if (!shard_args_ok(n_total, lo, n_local)) return NBD_E_BADARG;
  if (n_local == 0) return 0;
  if (!posm_local || misaligned16(posm_local)) return NBD_E_BADARG;
  if (!workspace || workspace_bytes < nbd_shard_workspace_bytes(n_total, lo, n_local)) return NBD_E_WORKSPACE;
  const ShardPlan sp = plan_shard(n_total, lo, n_local);
  return launch_accel(posm_local, full_view(n_local, sp.local), posm_local, n_local, 0, softening_sq, 1.0f,
                      static_cast<float*>(workspace), sp.local, (hipStream_t)stream, uniform);
}

// every other rank's bodies, then acc = g_scale * (all slabs, local ones first) and the fused kick
static int shard_force_remote(const float* posm_all, int n_total, const float* posm_local, int n_local, int lo,
                              float softening_sq, float g_scale, float* acc_out, float* vel, float c_kick,
                              void* workspace, size_t workspace_bytes, nbd_stream_t stream, bool uniform) {
  if (!shard_args_ok(n_total, lo, n_local)) return NBD_E_BADARG;
  if (n_local == 0) return 0;
  if (!posm_all || !posm_local || !acc_out || misaligned16(posm_all) || misaligned16(posm_local)) return NBD_E_BADARG;
  if (!workspace || workspace_bytes < nbd_shard_workspace_bytes(n_total, lo, n_local)) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const ShardPlan sp = plan_shard(n_total, lo, n_local);
  float* slabs = static_cast<float*>(workspace);
  const int n3 = 3 * n_local;
  if (sp.remote.slabs > 0) {
    SrcView sv;
    excluded_view(n_total, lo, lo + n_local, &sv);
    // the diagonal never occurs here (every j in [lo, lo + n_local) is excluded); lo keeps the index meaning
    int rc = launch_accel(posm_all, sv, posm_local, n_local, lo, softening_sq, 1.0f,
                          slabs + (size_t)sp.local.slabs * n3, sp.remote, st, uniform);
    if (rc) return rc;
  }
  finish_kernel<<<ceil_div(n3, 64), 256, 0, st>>>(slabs, sp.local.slabs + sp.remote.slabs, (size_t)n3, g_scale,
                                                   acc_out, vel, c_kick, n3);
  return launch_status();
}

int nbd_shard_force_local_f32(const float* posm_local, int n_local, float softening_sq, void* workspace,
                              size_t workspace_bytes, int n_total, int lo, nbd_stream_t stream) {
  return shard_force_local(posm_local, n_local, softening_sq, workspace, workspace_bytes, n_total, lo, stream, false);
}

int nbd_shard_force_remote_f32(const float* posm_all, int n_total, const float* posm_local, int n_local, int lo,
                               float softening_sq, float g_const, float* acc_out, float* vel, float c_kick,
                               void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  return shard_force_remote(posm_all, n_total, posm_local, n_local, lo, softening_sq, g_const, acc_out, vel, c_kick,
                            workspace, workspace_bytes, stream, false);
}

// The two force launches of the range-sharded step for a system of EQUAL masses (see nbd_leapfrog_step_uniform_f32): the
// kernels without their per-pair mass multiply, g_const * mass_value applied once by the finishing kernel.
int nbd_shard_force_local_uniform_f32(const float* posm_local, int n_local, float softening_sq, void* workspace,
                                      size_t workspace_bytes, int n_total, int lo, nbd_stream_t stream) {
  return shard_force_local(posm_local, n_local, softening_sq, workspace, workspace_bytes, n_total, lo, stream, true);
}

int nbd_shard_force_remote_uniform_f32(const float* posm_all, int n_total, const float* posm_local, int n_local, int lo,
                                       float softening_sq, float g_const, float mass_value, float* acc_out, float* vel,
                                       float c_kick, void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  return shard_force_remote(posm_all, n_total, posm_local, n_local, lo, softening_sq, g_const * mass_value, acc_out, vel,
                            c_kick, workspace, workspace_bytes, stream, true);
}

int nbd_kick_drift_f32(float* pos, float* vel, const float* acc, const float* mass, int n,
                       float c_kick, float c_drift, float* posm, nbd_stream_t stream) {
  if (n < 0 || (n > 0 && (!pos || !vel)) || (posm && (!mass || misaligned16(posm)))) return NBD_E_BADARG;
  if (n == 0) return 0;
  const int n_pad = posm ? nbd_posm_padded_len(n) : n;
  kick_drift_kernel<<<ceil_div(n_pad, 256), 256, 0, (hipStream_t)stream>>>(
      pos, vel, acc, mass, n, n_pad, c_kick, c_drift, reinterpret_cast<f4*>(posm));
  return launch_status();
}

int nbd_kick_f32(float* vel, const float* acc, int n, float c, nbd_stream_t stream) {
  if (n < 0 || (n > 0 && (!vel || !acc))) return NBD_E_BADARG;
  if (n == 0) return 0;
  axpy_kernel<<<ceil_div(3 * n, 256), 256, 0, (hipStream_t)stream>>>(vel, acc, c, 3 * n);
  return launch_status();
}

int nbd_drift_f32(float* pos, const float* vel, int n, float c, nbd_stream_t stream) {
  if (n < 0 || (n > 0 && (!pos || !vel))) return NBD_E_BADARG;
  if (n == 0) return 0;
  axpy_kernel<<<ceil_div(3 * n, 256), 256, 0, (hipStream_t)stream>>>(pos, vel, c, 3 * n);
  return launch_status();
}

int nbd_snapshot_f32(const float* pos, const float* vel, const float* acc, int n, float* out, nbd_stream_t stream) {
  if (n < 0 || (n > 0 && (!pos || !vel || !acc || !out))) return NBD_E_BADARG;
  if (n == 0) return 0;
  snapshot_kernel<float><<<ceil_div(3 * n, 256), 256, 0, (hipStream_t)stream>>>(pos, vel, acc, 3 * n, out);
  return launch_status();
}

int nbd_snapshot_f64(const double* pos, const double* vel, const double* acc, int n, double* out, nbd_stream_t stream) {
  if (n < 0 || (n > 0 && (!pos || !vel || !acc || !out))) return NBD_E_BADARG;
  if (n > 0 && ((reinterpret_cast<uintptr_t>(out) & 7) != 0)) return NBD_E_BADARG;
  if (n == 0) return 0;
  snapshot_kernel<double><<<ceil_div(3 * n, 256), 256, 0, (hipStream_t)stream>>>(pos, vel, acc, 3 * n, out);
  return launch_status();
}

// What the whole-system steps share: check, update the bodies and pack them (the kick-drift of a leapfrog step with
// acc_in; euler: a plain pack), the force of all n bodies into slabs, then acc = g_scale * (slab sum) and the fused kick
// v += c_kick acc. uniform: the kernels without the per-pair mass multiply (g_scale carries the mass), and from
// kSymStepMinN bodies on every pair once (accel_sym2_tail_kernel where the workspace holds a slot per round: three
// launches a step; else the diagonal launch and accel_sym2_kernel).
static int step_force(float* pos, float* vel, const float* acc_in, float* acc_out, const float* mass, int n, bool euler,
                      float c_kick, float c_drift, float softening_sq, float g_scale, bool uniform, float* posm,
                      void* workspace, size_t workspace_bytes, nbd_stream_t stream, void* ev_force_begin,
                      void* ev_force_end) {
  if (n < 0) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (!pos || !vel || (!euler && !acc_in) || !acc_out || !mass || !posm || misaligned16(posm)) return NBD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const bool sym = uniform && sym_step(n, softening_sq);
  const AccelPlan p = plan_accel(n, n);
  // one slab also goes to scratch
  const size_t need = sym ? sym_workspace_bytes(n) : (size_t)p.slabs * n * 3 * sizeof(float);
  if (!workspace || workspace_bytes < need) return NBD_E_WORKSPACE;
  int rc = euler ? nbd_pack_posm_f32(pos, mass, n, posm, stream)
                 : nbd_kick_drift_f32(pos, vel, acc_in, mass, n, c_kick, c_drift, posm, stream);
  if (rc) return rc;
  float* slabs = static_cast<float*>(workspace);
  if (ev_force_begin && (rc = check(hipEventRecord((hipEvent_t)ev_force_begin, st)))) return rc;
  const SymPlan sp = plan_sym(n, sym ? sym_slots_avail(n, workspace_bytes) : 0);
  if (sym) rc = launch_sym(posm, n, softening_sq, slabs, sp, st, kSymTailVariant);
  else rc = launch_accel(posm, full_view(n, p), posm, n, 0, softening_sq, 1.0f, slabs, p, st, uniform);
  if (rc) return rc;
  if (ev_force_end && (rc = check(hipEventRecord((hipEvent_t)ev_force_end, st)))) return rc;
  const int n3 = 3 * n;
  const int n_slabs = sym ? sp.total_slots : p.slabs;
  finish_kernel<<<ceil_div(n3, 64), 256, 0, st>>>(slabs, n_slabs, (size_t)n3, g_scale, acc_out, vel, c_kick, n3);
  return launch_status();
}

int nbd_leapfrog_step_ev_f32(float* pos, float* vel, const float* acc_in, float* acc_out,
                          const float* mass, int n, float dt_half, float dt, float softening_sq,
                          float g_const, float* posm, void* workspace, size_t workspace_bytes,
                          nbd_stream_t stream, void* ev_force_begin, void* ev_force_end) {
  return step_force(pos, vel, acc_in, acc_out, mass, n, false, dt_half, dt, softening_sq, g_const, false, posm,
                    workspace, workspace_bytes, stream, ev_force_begin, ev_force_end);
}

// LeapFrogSimulator.step (simulation.py:153-170) for a system whose bodies all have the SAME mass (the published
// configurations: Plummer, m = 1 / N): the mass factors out of the force sum, a = (G m) sum_j d_ij s_ij^3, so the kernel
// drops its per-pair multiply by m_j (accel_kernel<.., UNI = true>: 11 packed fp32 ops + 2 v_rsq_f32 per source and pair
// of targets instead of 12 + 2) and the finishing kernel applies g_const * mass_value once. Same differences, same slab
// sums; one multiplication rounds differently (per finished sum instead of per term). The CALLER vouches that every
// entry of `mass` equals mass_value (the Python simulator checks once, at construction); `mass` is still read to write
// the packed bodies {x, y, z, m} that the energy kernel and the surrogates consume.
int nbd_leapfrog_step_uniform_f32(float* pos, float* vel, const float* acc_in, float* acc_out, const float* mass,
                                  float mass_value, int n, float dt_half, float dt, float softening_sq, float g_const,
                                  float* posm, void* workspace, size_t workspace_bytes, nbd_stream_t stream,
                                  void* ev_force_begin, void* ev_force_end) {
  return step_force(pos, vel, acc_in, acc_out, mass, n, false, dt_half, dt, softening_sq, g_const * mass_value, true,
                    posm, workspace, workspace_bytes, stream, ev_force_begin, ev_force_end);
}

int nbd_leapfrog_step_f32(float* pos, float* vel, const float* acc_in, float* acc_out,
                          const float* mass, int n, float dt_half, float dt, float softening_sq,
                          float g_const, float* posm, void* workspace, size_t workspace_bytes,
                          nbd_stream_t stream) {
  return nbd_leapfrog_step_ev_f32(pos, vel, acc_in, acc_out, mass, n, dt_half, dt, softening_sq, g_const,
                                  posm, workspace, workspace_bytes, stream, nullptr, nullptr);
}

int nbd_euler_step_f32(float* pos, float* vel, float* acc_out, const float* mass, int n, float dt,
                       float softening_sq, float g_const, float* posm, void* workspace,
                       size_t workspace_bytes, nbd_stream_t stream) {
  const int rc = step_force(pos, vel, nullptr, acc_out, mass, n, true, dt, 0.f, softening_sq, g_const, false, posm,
                            workspace, workspace_bytes, stream, nullptr, nullptr);
  if (rc) return rc;
  return nbd_drift_f32(pos, vel, n, dt, stream);
}

size_t nbd_energy_workspace_bytes(int n) {
  if (n <= 0) return 0;
  const int groups = ceil_div(n, kTgtPerWG);
  return ((size_t)groups * energy_slabs(groups) + (size_t)ceil_div(n, 256)) * sizeof(double);
}

int nbd_energy_f32(const float* posm, const float* vel, int n, float softening, float g_const,
                   double* out_uk, void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  if (n < 0 || !out_uk) return NBD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    zero_f32_kernel<<<1, 256, 0, st>>>(reinterpret_cast<float*>(out_uk), 4);   // two doubles
    return launch_status();
  }
  if (!posm || !vel || misaligned16(posm)) return NBD_E_BADARG;
  if (!workspace || workspace_bytes < nbd_energy_workspace_bytes(n)) return NBD_E_WORKSPACE;
  const int groups = ceil_div(n, kTgtPerWG), slabs = energy_slabs(groups), nk = ceil_div(n, 256);
  double* pu = static_cast<double*>(workspace);
  double* pk = pu + (size_t)groups * slabs;
  const f4* pm = reinterpret_cast<const f4*>(posm);
  energy_kernel<<<dim3(groups, slabs), 64 * kWaves, 0, st>>>(pm, n, ceil_div(n, kChunk), softening,
                                                           softening > 0.f ? 0 : 1, pu);
  int rc = launch_status();
  if (rc) return rc;
  kinetic_kernel<<<nk, 256, 0, st>>>(pm, vel, n, pk);
  rc = launch_status();
  if (rc) return rc;
  energy_final_kernel<<<1, 256, 0, st>>>(pu, groups * slabs, pk, nk, g_const, out_uk);
  return launch_status();
}

}  // extern "C"
