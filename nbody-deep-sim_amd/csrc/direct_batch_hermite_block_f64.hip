// direct_batch_hermite_block_f64.hip -- direct_hermite_block_f64.hip's block-timestep Hermite integration (4th and 6th
// order, float64), applied to every scene of an ensemble of independent systems by ONE schedule and one set of launches
// per block step (gfx950). C-ABI: the nbd_batch_hblock_*_f64 / nbd_batch_hblock6_*_f64 entries of include/nbd.h; Python:
// galaxify.simulation.BatchedSimulator(integrator="block_hermite" / "block_hermite6").
//
// All scenes share one tick grid: an output interval is 2^K ticks for every scene (K = max_level), scene s's tick being
// dt_s 2^-K long. Body i of any scene carries its level k_i, step d_i = 2^(K - k_i) ticks and last correction tick t_i, a
// multiple of d_i. The scheduler runs over all bodies as one pool: t_next = the first multiple after the current tick T
// of any d present, body i active iff d_i divides t_next. A scene with no body due at t_next has no active body; a scene
// with one gets exactly the active set it would list alone, because no multiple of any of its d lies between its own
// last tick and T. So the ensemble's ticks are the sorted union of the scenes' own, every scene sees exactly its own
// block steps, and the host reads ONE record {t_next, n_act_total} per ensemble block step.
//
// Device records (int32, NBD_HBLOCK_SCHED_INTS each, the one-system layout of hermite_block_kernels.h): record 0 is the
// ensemble's {t_next, n_act_total, -, T, -, finished workgroups, histogram of all levels}; record 1 + s is scene s's
// {t_next, n_act_s, clamped_s, T_s, list cursor, -, histogram of the scene's levels}. The one-system re-levelling
// (hblock_relevel, hblock6_relevel) is handed the scene's record, so the clamp count is per scene; the corrector moves the
// body in the ensemble's histogram too. counters: int64 {block steps, pair interactions} per scene, added to by the
// scheduler (a scene counts a block step when it has an active body; pairs = n_act_s n_s). Nothing per scene reaches
// the host in a block step.
//
// The plan has direct_batch_plan.h's layout (items, scene records, row_scene) with a STATIC work list: scene s gets
// max over g in [1, ceil(n_s / 64)] of g slabs_f64(g, chunks_s) items (s, k), enough for any active count, and
// the one-system block workspace's partial-sum area for n_s bodies at ws_off. Workspace: the active lists, int[n_total rounded up to 8] (scene
// s's segment at its body offset, holding scene-local indices), then the partial sums. A block step:
//   schedule : t_next, n_act_total; every scene's active bodies into its own segment (integer atomics on the scene's
//              cursor; the order is free), n_act_s from the scene's histogram, the counters
//   predict  : one thread per packed row over (t_next - t_i) dt_s 2^-K (hblock_ticks_len), the constants formed in fp64
//              from that step; zero rows behind each scene's last body
//   evaluate : one workgroup per item (s, k). From n_act_s: groups = ceil(n_act_s / 64), slabs = slabs_f64(groups,
//              chunks_s) -- the one-system block step's plan -- and k >= groups slabs (or n_act_s = 0) leaves at once;
//              else group k / slabs, slab k % slabs: Group64, the scene's chunk split, Order::make, walk_f64 -- the lines
//              of active_force_f64_kernel -- into the scene's double[slabs][kOut][n_act_s]. Masked (eps_s^2 < 1e-24) per scene.
//   correct  : one thread per packed row p of a scene, p < n_act_s: the slabs in slab order x G_s, the corrector with the
//              body's own h_i = dt_s 2^-k_i, the new level with eta_s, t_i, posd = {x1, m}
// Every rounded operation is the single copy in hermite_kernels.h, hermite_f64_kernels.h, hermite6_f64_kernels.h and
// hermite_block_kernels.h: a scene's state, levels and counters are bit-identical to the one-system block entries on that
// scene alone, whatever its companions. No float atomics, no memsets in a step, no host sync but the one read;
// deterministic with a workspace that may hold anything.
// Per-scene scalars come from a device table par[NBD_BATCH_HBLOCK_PARAM_ROWS][S]: G, eps^2, eps, dt, eta.
// Resources (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage; VGPRs, LDS bytes per workgroup, waves
// per SIMD). batch_active_force_f64_kernel<Order4>: 90, 32768, 5 -- active_force_f64_kernel<Order4>'s figures (kMinWG = 5);
// <Order6>: 164, 49152, 3 -- that kernel's too. batch_hblock_schedule_kernel: 22, 4, 8. batch_hblock_predict_kernel: 46, 0,
// 8; batch_hblock6_predict_kernel: 52, 0, 8. batch_hblock_correct_kernel: 82, 0, 5; batch_hblock6_correct_kernel: 108, 0, 4.
// batch_hblock_init_kernel: 26, 88, 8; batch_hblock_pool_kernel: 11, 0, 8. No AGPRs, no SGPR or VGPR spills and no scratch
// anywhere. Every store is a vector store from plain HIP C++.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_batch_plan.h"
#include "direct_kernels.h"
#include "hermite6_f64_kernels.h"
#include "hermite_block_kernels.h"
#include "hermite_f64_kernels.h"
#include "hermite_kernels.h"
#include "hermite_orders_f64.h"

namespace {

enum ParamRow { kG = 0, kEps2, kEps, kDt, kEta, kParams };
static_assert(kParams == NBD_BATCH_HBLOCK_PARAM_ROWS, "the table include/nbd.h describes");

constexpr int kRec = NBD_HBLOCK_SCHED_INTS;

__device__ __forceinline__ int* scene_rec(int* __restrict__ bsched, int s) { return bsched + (size_t)(1 + s) * kRec; }

size_t act_bytes(int n_total) { return (size_t)ceil_div(n_total, 8) * 8 * sizeof(int); }

// ---- the plan: the static work list. A scene's items are numbered k in [0, items(n)); `groups` carries that count and
// `slabs` is 1, so batch_plan_fill writes (s, k, 0) and the totals count the items.
inline int block_items(int n) {
  const int chunks = ceil_div(n, kChunk), g_all = ceil_div(n, kTgtF64);
  int most = 0;
  for (int g = 1; g <= g_all; ++g) most = std::max(most, g * slabs_f64(g, chunks));
  return most;
}

// A scene's partial sums are the one-system block workspace's (nbd_hblock_f64_workspace_bytes /
// nbd_hblock6_f64_workspace_bytes: that entry's list of n ints rounded up to 8, then the largest slabs x kOut x n_act
// doubles any active set of n sources can need), asked of that entry so that there is one copy of the sizing.
template <int kOut>
int64_t scene_sum_doubles(int n) {
  const size_t all = kOut == 6 ? nbd_hblock_f64_workspace_bytes(n) : nbd_hblock6_f64_workspace_bytes(n);
  return (int64_t)((all - act_bytes(n)) / sizeof(double));
}

template <int kOut>
SceneGeom scene_geom_block(int n) {
  return SceneGeom{1, block_items(n), scene_sum_doubles<kOut>(n), 0};
}

template <int kOut>
int block_totals(const int* offsets, int n_scenes, BatchTotals* t) {
  return batch_totals(offsets, n_scenes, t, scene_geom_block<kOut>);
}

template <int kOut>
int block_prologue(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, BatchTotals* t) {
  return batch_prologue(offsets, n_scenes, plan, plan_bytes, t, scene_geom_block<kOut>);
}

size_t block_ws_bytes(const BatchTotals& t) { return act_bytes(t.n_total) + (size_t)t.ws_floats * sizeof(double); }

bool bad_block_ws(const void* ws, size_t have, size_t need) { return !ws || misaligned32(ws) || have < need; }

int* ws_act(void* ws) { return static_cast<int*>(ws); }
double* ws_sums(void* ws, const BatchTotals& t) {
  return reinterpret_cast<double*>(static_cast<char*>(ws) + act_bytes(t.n_total));
}

// ---- initial levels. One workgroup per scene (mask: only the scenes with mask[s] != 0; nullptr: all): ticks = 0, levels
// from hblock_initial_level with the scene's dt and eta, clamped ones counted into the scene's record, the scene's
// histogram rewritten, T_s and the cursor to 0. Then batch_hblock_pool_kernel adds the scenes' histograms.
__global__ __launch_bounds__(256) void batch_hblock_init_kernel(const SceneRec* __restrict__ scenes,
                                                                const double* __restrict__ acc,
                                                                const double* __restrict__ jerk,
                                                                const double* __restrict__ par, int n_scenes, int K,
                                                                const int* __restrict__ mask, int* __restrict__ ticks,
                                                                int* __restrict__ levels, int* __restrict__ bsched) {
  __shared__ int hist[kMaxLevel + 1];
  __shared__ int clamped;
  const int s = blockIdx.x;
  if (mask && !mask[s]) return;
  const SceneRec sc = load_scene(scenes, s);
  const double dt = par[kDt * n_scenes + s], eta = par[kEta * n_scenes + s];
  if (threadIdx.x <= kMaxLevel) hist[threadIdx.x] = 0;
  if (threadIdx.x == 0) clamped = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < sc.n; i += 256) {
    const size_t b = (size_t)sc.off + i;
    int k = hblock_initial_level(acc, jerk, b, K, dt, eta);
    if (k > K) {
      k = K;
      atomicAdd(&clamped, 1);
    }
    ticks[b] = 0;
    levels[b] = k;
    atomicAdd(&hist[k], 1);
  }
  __syncthreads();
  int* ss = scene_rec(bsched, s);
  if (threadIdx.x <= kMaxLevel) ss[kHist + threadIdx.x] = hist[threadIdx.x];
  if (threadIdx.x == 0) {
    ss[kClamped] += clamped;
    ss[kTCur] = 0;
    ss[kCursor] = 0;
  }
}

__global__ __launch_bounds__(64) void batch_hblock_pool_kernel(int n_scenes, int* __restrict__ bsched) {
  if (threadIdx.x <= kMaxLevel) {
    int sum = 0;
    for (int s = 0; s < n_scenes; ++s) sum += scene_rec(bsched, s)[kHist + threadIdx.x];
    bsched[kHist + threadIdx.x] = sum;
  }
  if (threadIdx.x == 0) {
    bsched[kTCur] = 0;
    bsched[kCursor] = 0;
    bsched[kDone] = 0;
  }
}

// ---- the schedule. One thread per packed row. t_next from the ensemble's histogram and T, as hblock_schedule_kernel
// forms it (integers only); a wave's 64 rows lie in one scene, and it appends its active bodies (scene-local indices) to
// that scene's segment at one integer atomic on the scene's cursor. The thread of a scene's first row publishes the
// scene's {t_next, n_act_s} (n_act_s from the scene's histogram) and adds to its counters; block 0 publishes the
// ensemble's record. The last workgroup to finish sets every cursor and the finished count back to 0.
__global__ __launch_bounds__(256) void batch_hblock_schedule_kernel(const int* __restrict__ row_scene,
                                                                    const SceneRec* __restrict__ scenes, int n_rows,
                                                                    int n_scenes, const int* __restrict__ levels, int K,
                                                                    int* __restrict__ bsched,
                                                                    long long* __restrict__ counters,
                                                                    int* __restrict__ act) {
  __shared__ int last;
  const int T = bsched[kTCur];
  int t_next = INT_MAX;
  for (int k = 0; k <= K; ++k)
    if (bsched[kHist + k] > 0) {
      const int d = 1 << (K - k);
      t_next = min(t_next, (T / d + 1) * d);
    }
  const int thr = max(0, K - __builtin_ctz(t_next));          // active: d_i divides t_next
  PlanRow w;
  const bool in = load_row(row_scene, scenes, n_rows, w);
  if (in) {
    int* ss = scene_rec(bsched, w.s);
    const int i = w.i();
    const bool on = i < w.sc.n && levels[(size_t)w.sc.off + i] >= thr;
    const unsigned long long mask = __ballot(on);
    if (mask) {
      const int lane = threadIdx.x & 63, leader = __ffsll((long long)mask) - 1;
      int base = 0;
      if (lane == leader) base = atomicAdd(&ss[kCursor], __popcll(mask));
      base = __shfl(base, leader);
      if (on) act[(size_t)w.sc.off + base + __popcll(mask & __lanemask_lt())] = i;
    }
    if (i == 0) {
      int n_act = 0;
      for (int k = thr; k <= K; ++k) n_act += ss[kHist + k];
      ss[kTNext] = t_next;
      ss[kNAct] = n_act;
      if (n_act > 0) {
        counters[2 * (size_t)w.s] += 1;
        counters[2 * (size_t)w.s + 1] += (long long)n_act * w.sc.n;
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int n_act = 0;
    for (int k = thr; k <= K; ++k) n_act += bsched[kHist + k];
    bsched[kTNext] = t_next;
    bsched[kNAct] = n_act;
  }
  __syncthreads();                                             // every wave of this workgroup has taken its places
  if (threadIdx.x == 0) {
    __threadfence();
    last = atomicAdd(&bsched[kDone], 1) == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (last) {                                                  // the last workgroup: no cursor update can follow
    for (int s = threadIdx.x; s < n_scenes; s += 256) scene_rec(bsched, s)[kCursor] = 0;
    if (threadIdx.x == 0) bsched[kDone] = 0;
  }
}

// ---- predict: hblock_predict_kernel<double> / hblock6_predict_kernel per packed row, with the scene's dt
__global__ __launch_bounds__(256) void batch_hblock_predict_kernel(
    const int* __restrict__ row_scene, const SceneRec* __restrict__ scenes, int n_rows, const double* __restrict__ pos,
    const double* __restrict__ vel, const double* __restrict__ acc, const double* __restrict__ jerk,
    const double* __restrict__ mass, const int* __restrict__ ticks, const double* __restrict__ par, int n_scenes,
    double tick, const int* __restrict__ bsched, d4* __restrict__ posd, d4* __restrict__ veld) {
  PlanRow w;
  if (!load_row(row_scene, scenes, n_rows, w)) return;
  d4 pm = HermiteFmt<double>::zero(), vp = HermiteFmt<double>::zero();
  if (w.i() < w.sc.n) {
    const size_t b = (size_t)w.sc.off + w.i();
    const HermiteStep<double> h =
        hermite_step_constants<double>(hblock_ticks_len(par[kDt * n_scenes + w.s], bsched[kTNext] - ticks[b], tick));
    const PosVel3<double> p = hermite_predict_row(pos, vel, acc, jerk, b, h.dt, h.dt2_half, h.dt3_sixth, true);
    pm = hermite_row(p.x, mass[b]);
    vp = hermite_row(p.v, 0.0);
  }
  posd[w.r] = pm;
  veld[w.r] = vp;
}

__global__ __launch_bounds__(256) void batch_hblock6_predict_kernel(
    const int* __restrict__ row_scene, const SceneRec* __restrict__ scenes, int n_rows, const double* __restrict__ pos,
    const double* __restrict__ vel, const double* __restrict__ acc, const double* __restrict__ jerk,
    const double* __restrict__ snap, const double* __restrict__ crackle, const double* __restrict__ mass,
    const int* __restrict__ ticks, const double* __restrict__ par, int n_scenes, double tick,
    const int* __restrict__ bsched, d4* __restrict__ posd, d4* __restrict__ veld, d4* __restrict__ accd) {
  PlanRow w;
  if (!load_row(row_scene, scenes, n_rows, w)) return;
  d4 pm = {0.0, 0.0, 0.0, 0.0}, vp = pm, ap = pm;
  if (w.i() < w.sc.n) {
    const size_t b = (size_t)w.sc.off + w.i();
    const Hermite6Step h =
        hermite6_step_constants(hblock_ticks_len(par[kDt * n_scenes + w.s], bsched[kTNext] - ticks[b], tick));
    hermite6_predict_row(pos, vel, acc, jerk, snap, crackle, mass, b, h, pm, vp, ap);
  }
  posd[w.r] = pm;
  veld[w.r] = vp;
  accd[w.r] = ap;
}

// ---- evaluate: active_force_f64_kernel's prologue per item, its geometry formed from the scene's n_act
template <class Order>
__global__ __launch_bounds__(64 * kWaves, Order::kMinWG) void batch_active_force_f64_kernel(
    const d4* __restrict__ posd, const d4* __restrict__ veld, const d4* __restrict__ accd,
    const int4* __restrict__ items, const SceneRec* __restrict__ scenes, const double* __restrict__ par, int n_scenes,
    const int* __restrict__ bsched, const int* __restrict__ act, double* __restrict__ ws) {
  using Pair = typename Order::Pair;
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads_n<Order::kArr>()];
  const Item w = load_item(items, scenes);
  const int n_act = __builtin_amdgcn_readfirstlane(bsched[(size_t)(1 + w.s) * kRec + kNAct]);
  if (n_act <= 0) return;
  const int slabs = slabs_f64(ceil_div(n_act, kTgtF64), w.n_chunks);
  if (w.grp >= ceil_div(n_act, kTgtF64) * slabs) return;       // this block step needs fewer items than the worst case
  const double eps2 = par[kEps2 * n_scenes + w.s];
  const d4* pd = posd + w.poff;
  const d4* vd = veld + w.poff;
  const d4* ad = Order::kArr == 3 ? accd + w.poff : nullptr;
  const Group64<int> g(w.grp / slabs, w.grp % slabs, n_act);
  const ChunkRange c = wave_chunks_of(g.jw(), w.n_chunks, slabs);
  const int i = act[(size_t)w.sc.off + g.row()];
  Pair pr = Order::make(pd, vd, ad, i, i, eps2, w.n);
  walk_f64(pr, pd, vd, c.begin, c.end, eps2 < kEps2MaskedF64, -1, lds, g.dst<Pair>(ws + (size_t)w.ws_off), (size_t)n_act,
           g.n_valid(), nullptr, ad);
}

// What the thread of packed row w corrects in this block step: list entry p = w.i() of its scene, if the scene has
// that many active bodies.
struct Entry {
  int* ss;
  int n_act, slabs, K;
  size_t b;        // the body in the state arrays
  int i, lev, d;
  double h;
};

__device__ __forceinline__ bool load_entry(const PlanRow& w, int* __restrict__ bsched, const int* __restrict__ act,
                                           const int* __restrict__ levels, const double* __restrict__ par,
                                           int n_scenes, int K, double tick, Entry& e) {
  e.ss = scene_rec(bsched, w.s);
  e.n_act = e.ss[kNAct];
  if (w.i() >= e.n_act) return false;
  e.slabs = slabs_f64(ceil_div(e.n_act, kTgtF64), w.sc.n_chunks);
  e.i = act[(size_t)w.sc.off + w.i()];
  e.b = (size_t)w.sc.off + e.i;
  e.lev = levels[e.b];
  e.d = 1 << (K - e.lev);
  e.h = hblock_ticks_len(par[kDt * n_scenes + w.s], e.d, tick);
  return true;
}

// the corrected body's move in the ensemble's histogram (the scene's own is hblock_move_level's), integers only
__device__ __forceinline__ void pool_move(int* __restrict__ bsched, int lev, int nl) {
  if (nl != lev) {
    atomicSub(&bsched[kHist + lev], 1);
    atomicAdd(&bsched[kHist + nl], 1);
  }
}

// the ensemble's T after this block step, by one thread of the launch
__device__ __forceinline__ void publish_tick(int* __restrict__ bsched, int K) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int t_next = bsched[kTNext];
    bsched[kTCur] = t_next == (1 << K) ? 0 : t_next;
  }
}

// ---- correct: hblock_correct_kernel<double>'s / hblock6_correct_kernel's lines per list entry of every scene
__global__ __launch_bounds__(256) void batch_hblock_correct_kernel(
    const int* __restrict__ row_scene, const SceneRec* __restrict__ scenes, int n_rows, const double* __restrict__ ws,
    const int* __restrict__ act, const double* __restrict__ par, int n_scenes, int K, double tick, double* pos,
    double* vel, double* acc, double* jerk, const double* __restrict__ mass, int* __restrict__ ticks,
    int* __restrict__ levels, int* __restrict__ bsched, d4* __restrict__ posd) {
  publish_tick(bsched, K);
  PlanRow w;
  Entry e;
  if (!load_row(row_scene, scenes, n_rows, w) || !load_entry(w, bsched, act, levels, par, n_scenes, K, tick, e)) return;
  double a1[3], j1[3];
  hermite_slab_sum(ws + (size_t)w.sc.ws_off, e.slabs, e.n_act, (size_t)w.i(), true, par[kG * n_scenes + w.s], a1, j1);
  const HermiteStep<double> hc = hermite_step_constants<double>(e.h);
  const Corrected<double> c = hermite_correct_row(pos, vel, acc, jerk, e.b, a1, j1, hc.dt_half, hc.dt2_twelfth);
  hermite_store_force(acc, jerk, e.b, a1, j1);
  posd[w.sc.poff + e.i] = hermite_row(c.x1, mass[e.b]);
  hblock_relevel(c.a0, c.j0, a1, j1, e.h, par[kDt * n_scenes + w.s], par[kEta * n_scenes + w.s], K, e.lev, e.d, (int)e.b,
                 w.i() == 0, ticks, levels, e.ss);
  pool_move(bsched, e.lev, levels[e.b]);
}

__global__ __launch_bounds__(256) void batch_hblock6_correct_kernel(
    const int* __restrict__ row_scene, const SceneRec* __restrict__ scenes, int n_rows, const double* __restrict__ ws,
    const int* __restrict__ act, const double* __restrict__ par, int n_scenes, int K, double tick, double* pos,
    double* vel, double* acc, double* jerk, double* snap, double* crackle, const double* __restrict__ mass,
    int* __restrict__ ticks, int* __restrict__ levels, int* __restrict__ bsched, d4* __restrict__ posd) {
  publish_tick(bsched, K);
  PlanRow w;
  Entry e;
  if (!load_row(row_scene, scenes, n_rows, w) || !load_entry(w, bsched, act, levels, par, n_scenes, K, tick, e)) return;
  const Hermite6Ends f = hermite6_finish_row(ws + (size_t)w.sc.ws_off, e.slabs, (size_t)e.n_act, (size_t)w.i(), e.b,
                                             par[kG * n_scenes + w.s], hermite6_step_constants(e.h), pos, vel, acc, jerk,
                                             snap, acc, jerk, snap, crackle, mass, posd, (size_t)w.sc.poff + e.i);
  hblock6_relevel(f.a0, f.j0, f.s0, f.a1, f.j1, f.s1, f.c1, e.h, par[kDt * n_scenes + w.s], par[kEta * n_scenes + w.s],
                  K, e.lev, e.d, (int)e.b, w.i() == 0, ticks, levels, e.ss);
  pool_move(bsched, e.lev, levels[e.b]);
}

// ---- host bodies

struct BlockState {
  double *pos, *vel, *acc, *jerk, *snap, *crackle;
  const double* mass;
  int *ticks, *levels, *bsched;
  const double* par;
  double *posd, *veld, *accd;
};

enum Stage { kPredict = 1, kForce = 2, kCorrect = 4, kStep = 7 };

// what the stages asked for read or write of the state (a stage entry leaves the rest nullptr)
template <class Order>
bool bad_state(const BlockState& s, int stages) {
  const bool six = Order::kArr == 3;
  if (!s.bsched || !s.par || misaligned8(s.par) || !s.posd || misaligned32(s.posd)) return true;
  if ((stages & (kPredict | kCorrect)) &&
      (!s.pos || !s.vel || !s.acc || !s.jerk || (six && (!s.snap || !s.crackle)) || !s.mass || !s.ticks))
    return true;
  if ((stages & kCorrect) && !s.levels) return true;
  return (stages & (kPredict | kForce)) &&
         (!s.veld || misaligned32(s.veld) || (six && (!s.accd || misaligned32(s.accd))));
}

template <class Order>
int launch_predict(const DevPlan& d, const BatchTotals& t, const BlockState& s, int K, hipStream_t st) {
  const double tick = ldexp(1.0, -K);
  const int grid = ceil_div(t.n_rows, 256);
  if (Order::kArr == 3)
    batch_hblock6_predict_kernel<<<grid, 256, 0, st>>>(d.row_scene, d.scenes, t.n_rows, s.pos, s.vel, s.acc, s.jerk,
                                                       s.snap, s.crackle, s.mass, s.ticks, s.par, t.n_scenes, tick,
                                                       s.bsched, reinterpret_cast<d4*>(s.posd),
                                                       reinterpret_cast<d4*>(s.veld), reinterpret_cast<d4*>(s.accd));
  else
    batch_hblock_predict_kernel<<<grid, 256, 0, st>>>(d.row_scene, d.scenes, t.n_rows, s.pos, s.vel, s.acc, s.jerk,
                                                      s.mass, s.ticks, s.par, t.n_scenes, tick, s.bsched,
                                                      reinterpret_cast<d4*>(s.posd), reinterpret_cast<d4*>(s.veld));
  return launch_status();
}

template <class Order>
int launch_force(const DevPlan& d, const BatchTotals& t, const BlockState& s, void* workspace, hipStream_t st) {
  batch_active_force_f64_kernel<Order><<<t.n_items, 64 * kWaves, 0, st>>>(
      reinterpret_cast<const d4*>(s.posd), reinterpret_cast<const d4*>(s.veld), reinterpret_cast<const d4*>(s.accd),
      d.items, d.scenes, s.par, t.n_scenes, s.bsched, ws_act(workspace), ws_sums(workspace, t));
  return launch_status();
}

template <class Order>
int launch_correct(const DevPlan& d, const BatchTotals& t, const BlockState& s, int K, void* workspace,
                   hipStream_t st) {
  const double tick = ldexp(1.0, -K);
  const int grid = ceil_div(t.n_rows, 256);
  if (Order::kArr == 3)
    batch_hblock6_correct_kernel<<<grid, 256, 0, st>>>(d.row_scene, d.scenes, t.n_rows, ws_sums(workspace, t),
                                                       ws_act(workspace), s.par, t.n_scenes, K, tick, s.pos, s.vel,
                                                       s.acc, s.jerk, s.snap, s.crackle, s.mass, s.ticks, s.levels,
                                                       s.bsched, reinterpret_cast<d4*>(s.posd));
  else
    batch_hblock_correct_kernel<<<grid, 256, 0, st>>>(d.row_scene, d.scenes, t.n_rows, ws_sums(workspace, t),
                                                      ws_act(workspace), s.par, t.n_scenes, K, tick, s.pos, s.vel, s.acc,
                                                      s.jerk, s.mass, s.ticks, s.levels, s.bsched,
                                                      reinterpret_cast<d4*>(s.posd));
  return launch_status();
}

// Everything the stages refuse, before the first launch; then the stages asked for, in order.
template <class Order>
int block_stages(int stages, const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const BlockState& s,
                 int max_level, void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  BatchTotals t;
  int rc = block_prologue<Order::Pair::kOut>(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc) return rc;
  if (bad_level(max_level)) return NBD_E_BADARG;
  if (t.n_total == 0) return 0;
  if (bad_state<Order>(s, stages)) return NBD_E_BADARG;
  if ((stages & (kForce | kCorrect)) && bad_block_ws(workspace, workspace_bytes, block_ws_bytes(t)))
    return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const DevPlan d = dev_plan(plan, t);
  if ((stages & kPredict) && (rc = launch_predict<Order>(d, t, s, max_level, st))) return rc;
  if ((stages & kForce) && (rc = launch_force<Order>(d, t, s, workspace, st))) return rc;
  if ((stages & kCorrect) && (rc = launch_correct<Order>(d, t, s, max_level, workspace, st))) return rc;
  return 0;
}

template <int kOut>
int block_plan_fill(const int* offsets, int n_scenes, void* plan, size_t plan_bytes) {
  BatchTotals t;
  const int rc = block_totals<kOut>(offsets, n_scenes, &t);
  if (rc) return rc;
  if (!plan || plan_bytes != plan_bytes_of(t)) return NBD_E_BADARG;
  batch_plan_fill(offsets, n_scenes, t, plan, scene_geom_block<kOut>);
  return 0;
}

template <int kOut>
int block_workspace_bytes(const int* offsets, int n_scenes, size_t* bytes) {
  BatchTotals t;
  const int rc = block_totals<kOut>(offsets, n_scenes, &t);
  if (rc) return rc;
  if (!bytes) return NBD_E_BADARG;
  *bytes = block_ws_bytes(t);
  return 0;
}

// a stage entry's read-only argument as a member of BlockState (the stage does not write through it)
template <class T>
T* mut(const T* p) { return const_cast<T*>(p); }

}  // namespace

extern "C" {

int nbd_batch_hblock_f64_plan(const int* offsets, int n_scenes, int* n_items, int* rows, size_t* plan_bytes) {
  BatchTotals t;
  const int rc = block_totals<6>(offsets, n_scenes, &t);
  if (rc) return rc;
  if (n_items) *n_items = t.n_items;
  if (rows) *rows = t.n_rows;
  if (plan_bytes) *plan_bytes = plan_bytes_of(t);
  return 0;
}

int nbd_batch_hblock_f64_plan_fill(const int* offsets, int n_scenes, void* plan, size_t plan_bytes) {
  return block_plan_fill<6>(offsets, n_scenes, plan, plan_bytes);
}

int nbd_batch_hblock6_f64_plan_fill(const int* offsets, int n_scenes, void* plan, size_t plan_bytes) {
  return block_plan_fill<9>(offsets, n_scenes, plan, plan_bytes);
}

int nbd_batch_hblock_f64_workspace_bytes(const int* offsets, int n_scenes, size_t* bytes) {
  return block_workspace_bytes<6>(offsets, n_scenes, bytes);
}

int nbd_batch_hblock6_f64_workspace_bytes(const int* offsets, int n_scenes, size_t* bytes) {
  return block_workspace_bytes<9>(offsets, n_scenes, bytes);
}

int nbd_batch_hblock_init_levels_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes,
                                     const double* acc, const double* jerk, const double* params, int max_level,
                                     const int* mask, int* ticks, int* levels, int* bsched, nbd_stream_t stream) {
  BatchTotals t;
  const int rc = block_prologue<6>(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc) return rc;
  if (bad_level(max_level) || !bsched || !params || misaligned8(params)) return NBD_E_BADARG;
  if (t.n_total > 0 && (!acc || !jerk || !ticks || !levels)) return NBD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  batch_hblock_init_kernel<<<n_scenes, 256, 0, st>>>(dev_plan(plan, t).scenes, acc, jerk, params, n_scenes, max_level,
                                                     mask, ticks, levels, bsched);
  int rc2 = launch_status();
  if (rc2) return rc2;
  batch_hblock_pool_kernel<<<1, 64, 0, st>>>(n_scenes, bsched);
  return launch_status();
}

int nbd_batch_hblock_schedule(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const int* levels,
                              int max_level, int* bsched, long long* counters, void* workspace, size_t workspace_bytes,
                              int* host_sched, nbd_stream_t stream) {
  BatchTotals t;
  int rc = block_prologue<6>(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc) return rc;
  if (t.n_total <= 0 || bad_level(max_level) || !levels || !bsched || !counters || misaligned8(counters))
    return NBD_E_BADARG;
  if (bad_block_ws(workspace, workspace_bytes, act_bytes(t.n_total))) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const DevPlan d = dev_plan(plan, t);
  batch_hblock_schedule_kernel<<<ceil_div(t.n_rows, 256), 256, 0, st>>>(d.row_scene, d.scenes, t.n_rows, n_scenes, levels,
                                                                        max_level, bsched, counters, ws_act(workspace));
  rc = launch_status();
  if (rc || !host_sched) return rc;
  hipError_t e = hipMemcpyAsync(host_sched, bsched, 4 * sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e == hipSuccess ? 0 : (int)e;
}

int nbd_batch_hblock_predict_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes,
                                 const double* pos, const double* vel, const double* acc, const double* jerk,
                                 const double* mass, const int* ticks, const double* params, int max_level,
                                 const int* bsched, double* posd, double* veld, nbd_stream_t stream) {
  const BlockState s{mut(pos), mut(vel), mut(acc), mut(jerk), nullptr, nullptr, mass, mut(ticks), nullptr, mut(bsched),
                     params, posd, veld, nullptr};
  return block_stages<Order4>(kPredict, offsets, n_scenes, plan, plan_bytes, s, max_level, nullptr, 0, stream);
}

int nbd_batch_hblock6_predict_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes,
                                  const double* pos, const double* vel, const double* acc, const double* jerk,
                                  const double* snap, const double* crackle, const double* mass, const int* ticks,
                                  const double* params, int max_level, const int* bsched, double* posd, double* veld,
                                  double* accd, nbd_stream_t stream) {
  const BlockState s{mut(pos), mut(vel), mut(acc), mut(jerk), mut(snap), mut(crackle), mass, mut(ticks), nullptr,
                     mut(bsched), params, posd, veld, accd};
  return block_stages<Order6>(kPredict, offsets, n_scenes, plan, plan_bytes, s, max_level, nullptr, 0, stream);
}

int nbd_batch_hblock_force_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes,
                               const double* posd, const double* veld, const double* params, const int* bsched,
                               void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  const BlockState s{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, mut(bsched),
                     params, mut(posd), mut(veld), nullptr};
  return block_stages<Order4>(kForce, offsets, n_scenes, plan, plan_bytes, s, 0, workspace, workspace_bytes, stream);
}

int nbd_batch_hblock6_force_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes,
                                const double* posd, const double* veld, const double* accd, const double* params,
                                const int* bsched, void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  const BlockState s{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, mut(bsched),
                     params, mut(posd), mut(veld), mut(accd)};
  return block_stages<Order6>(kForce, offsets, n_scenes, plan, plan_bytes, s, 0, workspace, workspace_bytes, stream);
}

int nbd_batch_hblock_correct_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, double* pos,
                                 double* vel, double* acc, double* jerk, const double* mass, int* ticks, int* levels,
                                 const double* params, int max_level, int* bsched, double* posd, void* workspace,
                                 size_t workspace_bytes, nbd_stream_t stream) {
  const BlockState s{pos, vel, acc, jerk, nullptr, nullptr, mass, ticks, levels, bsched, params, posd, nullptr, nullptr};
  return block_stages<Order4>(kCorrect, offsets, n_scenes, plan, plan_bytes, s, max_level, workspace, workspace_bytes,
                              stream);
}

int nbd_batch_hblock6_correct_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, double* pos,
                                  double* vel, double* acc, double* jerk, double* snap, double* crackle,
                                  const double* mass, int* ticks, int* levels, const double* params, int max_level,
                                  int* bsched, double* posd, void* workspace, size_t workspace_bytes,
                                  nbd_stream_t stream) {
  const BlockState s{pos, vel, acc, jerk, snap, crackle, mass, ticks, levels, bsched, params, posd, nullptr, nullptr};
  return block_stages<Order6>(kCorrect, offsets, n_scenes, plan, plan_bytes, s, max_level, workspace, workspace_bytes,
                              stream);
}

int nbd_batch_hblock_step_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, double* pos,
                              double* vel, double* acc, double* jerk, const double* mass, int* ticks, int* levels,
                              const double* params, int max_level, int* bsched, double* posd, double* veld,
                              void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  const BlockState s{pos, vel, acc, jerk, nullptr, nullptr, mass, ticks, levels, bsched, params, posd, veld, nullptr};
  return block_stages<Order4>(kStep, offsets, n_scenes, plan, plan_bytes, s, max_level, workspace, workspace_bytes,
                              stream);
}

int nbd_batch_hblock6_step_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, double* pos,
                               double* vel, double* acc, double* jerk, double* snap, double* crackle,
                               const double* mass, int* ticks, int* levels, const double* params, int max_level,
                               int* bsched, double* posd, double* veld, double* accd, void* workspace,
                               size_t workspace_bytes, nbd_stream_t stream) {
  const BlockState s{pos, vel, acc, jerk, snap, crackle, mass, ticks, levels, bsched, params, posd, veld, accd};
  return block_stages<Order6>(kStep, offsets, n_scenes, plan, plan_bytes, s, max_level, workspace, workspace_bytes,
                              stream);
}

}  // extern "C"
