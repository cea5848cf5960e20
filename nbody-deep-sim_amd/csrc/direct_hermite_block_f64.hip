// direct_hermite_block_f64.hip -- block-timestep Hermite integration in float64 for gfx950 (MI355X): the 4th order (the
// double-precision form of direct_hermite_block.hip, in the number format of direct_hermite_f64.hip) and the 6th order
// (the scheme of direct_hermite_f64.hip's 6th order, Nitadori & Makino 2008, on the same individual power-of-two steps). An
// extension. C-ABI: the nbd_hblock_*_f64 / nbd_accel_jerk_active_f64 and the nbd_hblock6_*_f64 /
// nbd_accel_jerk_snap_active_f64 entries of include/nbd.h; Python: galaxify.simulation.BlockHermiteSimulator(
// dtype=torch.float64) and BlockHermite6Simulator.
//
// One output interval dt is 2^K ticks, K = max_level. Body i carries its state at its last correction tick t_i and a
// level k_i; its step is h_i = dt 2^-k_i. Levels, ticks and the schedule record are the int32 of direct_hermite_block.hip;
// the scheduler is that unit's nbd_hblock_schedule and the initial levels are nbd_hblock_init_levels_f64's
// (dt_i = (eta / 2) |a| / |j|) at either order: neither reads anything else. What is fp64: the state, the packed rows, G,
// eps^2, dt, every body's own step constants (of its Delta, never rounded to fp32), the pair arithmetic and every sum.
// A block step to t_next = sched[kTNext] is three launches:
//   predict  : every body over its own Delta_i = (t_next - t_i) dt 2^-K into the packed rows, zero rows behind n
//   evaluate : active_force_f64_kernel<Order> -- the sums of the active targets under all n predicted sources into
//              double[slabs][kOut][n_act] partial sums in list order: the shared step's pair kernel with its targets
//              gathered through the list, the same walk_f64 and pair functor
//   correct  : the slabs in slab order, the corrector with the body's own h_i, the criterion for the new level,
//              t_i = t_next (0 at the end of the interval), posd = {x1, m}
// What the orders differ in (Order4, Order6 of hermite_orders_f64.h; the O(N) kernels and the pointer lists of the entries):
//         state         packed rows (d4)        sums: kOut   predict, correct
//   4th : x v a j       {x_p, m}, {v_p, 0}      a, j: 6      hblock_predict_kernel<double>, hblock_correct_kernel<double>:
//                                                            hermite_block_kernels.h's templates, the fp32 unit's source
//                                                            (hblock_relevel; kSumRows list entries per workgroup)
//   6th : x v a j s c   ... and {a_p, 0}        a, j, s: 9   hblock6_predict_kernel, hblock6_correct_kernel (below):
//                                                            hermite6_predict_row; hermite6_finish_row (corrector and c1),
//                                                            hblock6_relevel (p = 6); one thread per list entry
// The step constants are hermite_step_constants<double> resp. hermite6_step_constants of the body's own step, so a body
// whose step is the whole interval gets the shared step's; with every body listed the plan and the sums are the shared
// step's too: max_level = 0 is nbd_hermite_step_f64 resp. nbd_hermite6_step_f64 bit for bit.
// Exclusions. Below eps^2 = 1e-24 every chunk is walked index-masked, as in the shared step. Otherwise NO chunk is: a
// gathered group has no chunk of its own. The shared kernel walks its own chunk masked, which sets s = 0 for j == i and
// for the padding, so w = c = 0 and each fma adds a zero; un-masked, j == i has dr = dv = 0 (6th: and da = 0) with a
// finite w, c (s <= 1e12), and a padding row has m = 0 with a finite s, so each fma adds a zero again, to all 9 resp. 18
// sums. A partial sum starts at +0 and can never become -0 (x + -x is +0 in round-to-nearest), so adding a zero of
// either sign leaves its bits alone: with every body listed the sums are the shared step's, bit for bit, in whatever
// order the list holds them.
// Resources (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage). active_force_f64_kernel<Order4>: 90
// VGPRs, 32 KiB of LDS: 5 workgroups per CU, what the LDS allows and what force_f64_kernel<Order4> reaches at 89 VGPRs (left
// alone the compiler takes 116 here, one wave per SIMD fewer: kMinWG = 5). <Order6>: 164 VGPRs, 0 AGPRs, 48 KiB of LDS, 3
// waves per SIMD: three workgroups per CU by the LDS and by the registers alike, force_f64_kernel<Order6>'s figures,
// which the compiler reaches unasked (kMinWG = 1). hblock6_predict_kernel: 50 VGPRs; hblock6_correct_kernel: 98. No SGPR
// or VGPR spills and no scratch anywhere.
// No float atomics (the clamp counter and the histogram are integer atomics), no memsets in a step; the host reads
// {t_next, n_act} once per block step (nbd_hblock_schedule), so the path is eager-only. Deterministic run to run with a
// workspace that may hold anything.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_kernels.h"
#include "hermite6_f64_kernels.h"
#include "hermite_block_kernels.h"
#include "hermite_f64_kernels.h"
#include "hermite_kernels.h"
#include "hermite_orders_f64.h"

namespace {

// The sums (Pair::kOut per target) of the n_act targets act[0..n_act) under all n sources. Grid = (ceil(n_act / 64),
// slabs), block = 4 waves on the same 64 list entries, one per lane. The lanes behind n_act repeat the last target and
// store nothing. out: double[slab][kOut][n_act], in list order. A target's sums depend only on n and the slab count, not
// on where it sits in the list.
template <class Order>
__global__ __launch_bounds__(64 * kWaves, Order::kMinWG) void active_force_f64_kernel(
    const d4* __restrict__ posd, const d4* __restrict__ veld, const d4* __restrict__ accd, int n,
    const int* __restrict__ act, int n_act, int cpw_q, int cpw_r, double eps2, int all_masked,
    double* __restrict__ out) {
  using Pair = typename Order::Pair;
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads_n<Order::kArr>()];
  const Group64<unsigned> g(blockIdx.x, blockIdx.y, n_act);      // a group of list entries: the lane's body is act[its entry]
  const ChunkRange c = wave_chunks(g.jw(), cpw_q, cpw_r);
  const int i = act[g.row()];
  Pair pr = Order::make(posd, veld, accd, i, i, eps2, n);
  walk_f64(pr, posd, veld, c.begin, c.end, all_masked != 0, -1, lds, g.dst<Pair>(out), (size_t)n_act, g.n_valid(),
           nullptr, Order::kArr == 3 ? accd : nullptr);
}

// posd = {x_p, m}, veld = {v_p, 0}, accd = {a_p, 0} for rows [0, n_pad) (zero rows behind n): every body predicted from
// its last correction to t_next = sched[kTNext] by hermite6_predict_row over Delta_i = (t_next - t_i) dt / 2^K.
__global__ __launch_bounds__(256) void hblock6_predict_kernel(
    const double* __restrict__ pos, const double* __restrict__ vel, const double* __restrict__ acc,
    const double* __restrict__ jerk, const double* __restrict__ snap, const double* __restrict__ crackle,
    const double* __restrict__ mass, const int* __restrict__ ticks, int n, int n_pad, double dt, double tick,
    const int* __restrict__ sched, d4* __restrict__ posd, d4* __restrict__ veld, d4* __restrict__ accd) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n_pad) return;
  d4 pm = {0.0, 0.0, 0.0, 0.0}, vp = pm, ap = pm;
  if (i < (size_t)n) {
    const Hermite6Step h = hermite6_step_constants(hblock_ticks_len(dt, sched[kTNext] - ticks[i], tick));
    hermite6_predict_row(pos, vel, acc, jerk, snap, crackle, mass, i, h, pm, vp, ap);
  }
  posd[i] = pm;
  veld[i] = vp;
  accd[i] = ap;
}

// The active bodies' corrector, one thread per list entry p: a1, j1, s1 = G (slab 0 + slab 1 + ...) of row p of
// double[n_slabs][9][n_act]. pos == nullptr: written to row p of acc, jerk, snap (the force on its own, list order). Else,
// for body i = act[p] with its own step h = dt 2^-k_i: hermite6_finish_row with hermite6_step_constants(h), in place, then
// hblock6_relevel on the ends it returns.
__global__ __launch_bounds__(256) void hblock6_correct_kernel(const double* __restrict__ slabs, int n_slabs,
                                                              const int* __restrict__ act, int n_act, double g, int K,
                                                              double dt, double tick, double eta, double* pos,
                                                              double* vel, double* acc, double* jerk, double* snap,
                                                              double* crackle, const double* __restrict__ mass,
                                                              int* __restrict__ ticks, int* __restrict__ levels,
                                                              int* __restrict__ sched, d4* __restrict__ posd) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)n_act) return;
  if (!pos) {
    hermite6_finish_row(slabs, n_slabs, (size_t)n_act, p, p, g, hermite6_step_constants(0.0), nullptr, nullptr, nullptr,
                        nullptr, nullptr, acc, jerk, snap, nullptr, nullptr, nullptr, p);
    return;
  }
  const int i = act[p];
  const int lev = levels[i];
  const int d = 1 << (K - lev);
  const double h = hblock_ticks_len(dt, d, tick);
  const Hermite6Ends e = hermite6_finish_row(slabs, n_slabs, (size_t)n_act, p, (size_t)i, g, hermite6_step_constants(h),
                                             pos, vel, acc, jerk, snap, acc, jerk, snap, crackle, mass, posd, (size_t)i);
  hblock6_relevel(e.a0, e.j0, e.s0, e.a1, e.j1, e.s1, e.c1, h, dt, eta, K, lev, d, i, p == 0, ticks, levels, sched);
}

constexpr int kSumRows = HermiteFmt<double>::kSumRows;      // list entries per workgroup of the 4th-order corrector launch

// ---- the workspace: the active list (nbd_hblock_schedule writes it at the start, as in fp32), then, 32-byte aligned,
// the partial sums double[slabs][Pair::kOut][n_act]. With fewer than n targets plan_f64(n, n_act) has fewer groups and so
// more slabs towards kTargetWGs workgroups, never more than n_chunks / 4 (every wave keeps a chunk) or kMaxSlabs.
size_t act_bytes(int n) { return (size_t)ceil_div(n, 8) * 8 * sizeof(int); }

template <class Order>
size_t slab_bytes(size_t slab_rows) { return slab_rows * Order::Pair::kOut * sizeof(double); }

// what one block step with n_act targets uses of the workspace (O(1): one plan)
template <class Order>
size_t step_bytes(int n, int n_act) {
  return act_bytes(n) + (n_act > 0 ? slab_bytes<Order>((size_t)plan_f64(n, n_act).slabs * n_act) : 0);
}

// the largest slabs x n_act any active set of n sources can need: the slab count depends on the group count alone, so
// the fullest list of every group count
size_t slab_rows(int n) {
  size_t most = 0;
  const int g_all = ceil_div(n, kTgtF64);
  for (int g = 1; g <= g_all; ++g) {
    const int n_act = g == g_all ? n : g * kTgtF64;
    const size_t rows = (size_t)plan_f64(n, n_act).slabs * n_act;
    if (rows > most) most = rows;
  }
  return most;
}

int* ws_act(void* ws) { return static_cast<int*>(ws); }
double* ws_slabs(void* ws, int n) { return reinterpret_cast<double*>(static_cast<char*>(ws) + act_bytes(n)); }

inline bool bad_workspace(const void* ws, size_t have, size_t need) { return !ws || misaligned32(ws) || have < need; }

template <class Order>
int launch_active(const double* posd, const double* veld, const double* accd, int n, const int* act, int n_act,
                  double eps2, double* slabs, int groups, int n_slabs, hipStream_t st) {
  const ChunkSplit c = chunk_split(ceil_div(n, kChunk), n_slabs);
  active_force_f64_kernel<Order><<<dim3(groups, n_slabs), 64 * kWaves, 0, st>>>(
      reinterpret_cast<const d4*>(posd), reinterpret_cast<const d4*>(veld), reinterpret_cast<const d4*>(accd), n, act,
      n_act, c.q, c.r, eps2, eps2 < kEps2MaskedF64 ? 1 : 0, slabs);
  return launch_status();
}

// ---- the host bodies of the entries. state_ok: what the entry found of its own pointer list.

template <class Order>
size_t block_workspace_bytes(int n) { return n <= 0 ? 0 : act_bytes(n) + slab_bytes<Order>(slab_rows(n)); }

template <class Order>
int block_force(const double* posd, const double* veld, const double* accd, int n, int n_act, double softening_sq,
                void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  if (n <= 0 || n_act < 0 || n_act > n || bad_rows<Order>(posd, veld, accd)) return NBD_E_BADARG;
  if (bad_workspace(workspace, workspace_bytes, step_bytes<Order>(n, n_act))) return NBD_E_WORKSPACE;
  if (n_act == 0) return 0;
  const F64Plan p = plan_f64(n, n_act);
  return launch_active<Order>(posd, veld, accd, n, ws_act(workspace), n_act, softening_sq, ws_slabs(workspace, n),
                              p.groups, p.slabs, (hipStream_t)stream);
}

// A whole block step: everything the three stages refuse, before the first launch; then predict() and correct(), the
// entry's own stage entries, around the force of the listed bodies.
template <class Order, class Predict, class Correct>
int block_step(int n, int n_act, int max_level, double dt, double eta, bool state_ok, const double* posd,
               const double* veld, const double* accd, double softening_sq, void* workspace, size_t workspace_bytes,
               nbd_stream_t stream, Predict predict, Correct correct) {
  if (n <= 0 || n_act < 1 || n_act > n || bad_level(max_level) || !(dt > 0.0) || !(eta > 0.0)) return NBD_E_BADARG;
  if (!state_ok || bad_rows<Order>(posd, veld, accd)) return NBD_E_BADARG;
  if (bad_workspace(workspace, workspace_bytes, step_bytes<Order>(n, n_act))) return NBD_E_WORKSPACE;
  int rc = predict();
  if (rc) return rc;
  rc = block_force<Order>(posd, veld, accd, n, n_act, softening_sq, workspace, workspace_bytes, stream);
  return rc ? rc : correct();
}

// The force of a caller's list on its own, at the plan's slab count or a given one: the partial sums, then
// finish(slabs, n_slabs, stream), the entry's corrector launch without a state.
template <class Order, class Finish>
int active_force(const double* posd, const double* veld, const double* accd, int n, const int* act, int n_act,
                 double softening_sq, bool out_ok, void* workspace, size_t workspace_bytes, int slabs,
                 nbd_stream_t stream, Finish finish) {
  if (n < 0 || n_act < 0 || n_act > n || slabs < 0 || slabs > kMaxSlabs) return NBD_E_BADARG;
  if (n_act == 0) return 0;
  if (!act || !out_ok || bad_rows<Order>(posd, veld, accd)) return NBD_E_BADARG;
  const F64Plan p = plan_f64(n, n_act);
  if (slabs == 0) slabs = p.slabs;
  if (bad_workspace(workspace, workspace_bytes, act_bytes(n) + slab_bytes<Order>((size_t)slabs * n_act)))
    return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  double* part = ws_slabs(workspace, n);
  const int rc = launch_active<Order>(posd, veld, accd, n, act, n_act, softening_sq, part, p.groups, slabs, st);
  if (rc) return rc;
  finish(part, slabs, st);
  return launch_status();
}

}  // namespace

extern "C" {

size_t nbd_hblock_f64_workspace_bytes(int n) { return block_workspace_bytes<Order4>(n); }

size_t nbd_hblock6_f64_workspace_bytes(int n) { return block_workspace_bytes<Order6>(n); }

int nbd_hblock_init_levels_f64(const double* acc, const double* jerk, int n, double dt, double eta, int max_level,
                               int* ticks, int* levels, int* sched, nbd_stream_t stream) {
  return hblock_init_levels(acc, jerk, n, dt, eta, max_level, ticks, levels, sched, (hipStream_t)stream);
}

int nbd_hblock_predict_f64(const double* pos, const double* vel, const double* acc, const double* jerk,
                           const double* mass, const int* ticks, int n, int max_level, double dt, int* sched,
                           double* posd, double* veld, nbd_stream_t stream) {
  if (n <= 0 || bad_level(max_level) || !(dt > 0.0)) return NBD_E_BADARG;
  if (!pos || !vel || !acc || !jerk || !mass || !ticks || !sched || bad_rows<Order4>(posd, veld, nullptr))
    return NBD_E_BADARG;
  const int n_pad = nbd_posm_padded_len(n);
  hblock_predict_kernel<double><<<ceil_div(n_pad, 256), 256, 0, (hipStream_t)stream>>>(
      pos, vel, acc, jerk, mass, ticks, n, n_pad, dt, ldexp(1.0, -max_level), sched, reinterpret_cast<d4*>(posd),
      reinterpret_cast<d4*>(veld));
  return launch_status();
}

int nbd_hblock6_predict_f64(const double* pos, const double* vel, const double* acc, const double* jerk,
                            const double* snap, const double* crackle, const double* mass, const int* ticks, int n,
                            int max_level, double dt, int* sched, double* posd, double* veld, double* accd,
                            nbd_stream_t stream) {
  if (n <= 0 || bad_level(max_level) || !(dt > 0.0)) return NBD_E_BADARG;
  if (!pos || !vel || !acc || !jerk || !snap || !crackle || !mass || !ticks || !sched ||
      bad_rows<Order6>(posd, veld, accd))
    return NBD_E_BADARG;
  const int n_pad = nbd_posm_padded_len(n);
  hblock6_predict_kernel<<<ceil_div(n_pad, 256), 256, 0, (hipStream_t)stream>>>(
      pos, vel, acc, jerk, snap, crackle, mass, ticks, n, n_pad, dt, ldexp(1.0, -max_level), sched,
      reinterpret_cast<d4*>(posd), reinterpret_cast<d4*>(veld), reinterpret_cast<d4*>(accd));
  return launch_status();
}

int nbd_hblock_force_f64(const double* posd, const double* veld, int n, int n_act, double softening_sq, void* workspace,
                         size_t workspace_bytes, nbd_stream_t stream) {
  return block_force<Order4>(posd, veld, nullptr, n, n_act, softening_sq, workspace, workspace_bytes, stream);
}

int nbd_hblock6_force_f64(const double* posd, const double* veld, const double* accd, int n, int n_act,
                          double softening_sq, void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  return block_force<Order6>(posd, veld, accd, n, n_act, softening_sq, workspace, workspace_bytes, stream);
}

int nbd_hblock_correct_f64(double* pos, double* vel, double* acc, double* jerk, const double* mass, int* ticks,
                           int* levels, int n, int n_act, int max_level, double dt, double eta, double g_const,
                           int* sched, double* posd, void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  if (n <= 0 || n_act < 0 || n_act > n || bad_level(max_level) || !(dt > 0.0) || !(eta > 0.0)) return NBD_E_BADARG;
  if (!pos || !vel || !acc || !jerk || !mass || !ticks || !levels || !sched || !posd || misaligned32(posd))
    return NBD_E_BADARG;
  if (bad_workspace(workspace, workspace_bytes, step_bytes<Order4>(n, n_act))) return NBD_E_WORKSPACE;
  if (n_act == 0) return 0;
  hblock_correct_kernel<double><<<ceil_div(n_act, kSumRows), 256, 0, (hipStream_t)stream>>>(
      ws_slabs(workspace, n), plan_f64(n, n_act).slabs, ws_act(workspace), n_act, g_const, max_level, dt,
      ldexp(1.0, -max_level), eta, pos, vel, acc, jerk, mass, ticks, levels, sched, reinterpret_cast<d4*>(posd));
  return launch_status();
}

int nbd_hblock6_correct_f64(double* pos, double* vel, double* acc, double* jerk, double* snap, double* crackle,
                            const double* mass, int* ticks, int* levels, int n, int n_act, int max_level, double dt,
                            double eta, double g_const, int* sched, double* posd, void* workspace,
                            size_t workspace_bytes, nbd_stream_t stream) {
  if (n <= 0 || n_act < 0 || n_act > n || bad_level(max_level) || !(dt > 0.0) || !(eta > 0.0)) return NBD_E_BADARG;
  if (!pos || !vel || !acc || !jerk || !snap || !crackle || !mass || !ticks || !levels || !sched || !posd ||
      misaligned32(posd))
    return NBD_E_BADARG;
  if (bad_workspace(workspace, workspace_bytes, step_bytes<Order6>(n, n_act))) return NBD_E_WORKSPACE;
  if (n_act == 0) return 0;
  hblock6_correct_kernel<<<ceil_div(n_act, 256), 256, 0, (hipStream_t)stream>>>(
      ws_slabs(workspace, n), plan_f64(n, n_act).slabs, ws_act(workspace), n_act, g_const, max_level, dt,
      ldexp(1.0, -max_level), eta, pos, vel, acc, jerk, snap, crackle, mass, ticks, levels, sched,
      reinterpret_cast<d4*>(posd));
  return launch_status();
}

int nbd_hblock_step_f64(double* pos, double* vel, double* acc, double* jerk, const double* mass, int* ticks, int* levels,
                        int n, int n_act, int max_level, double dt, double eta, double softening_sq, double g_const,
                        int* sched, double* posd, double* veld, void* workspace, size_t workspace_bytes,
                        nbd_stream_t stream) {
  const bool state_ok = pos && vel && acc && jerk && mass && ticks && levels && sched;
  return block_step<Order4>(
      n, n_act, max_level, dt, eta, state_ok, posd, veld, nullptr, softening_sq, workspace, workspace_bytes, stream,
      [=] { return nbd_hblock_predict_f64(pos, vel, acc, jerk, mass, ticks, n, max_level, dt, sched, posd, veld, stream); },
      [=] {
        return nbd_hblock_correct_f64(pos, vel, acc, jerk, mass, ticks, levels, n, n_act, max_level, dt, eta, g_const,
                                      sched, posd, workspace, workspace_bytes, stream);
      });
}

int nbd_hblock6_step_f64(double* pos, double* vel, double* acc, double* jerk, double* snap, double* crackle,
                         const double* mass, int* ticks, int* levels, int n, int n_act, int max_level, double dt,
                         double eta, double softening_sq, double g_const, int* sched, double* posd, double* veld,
                         double* accd, void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  const bool state_ok = pos && vel && acc && jerk && snap && crackle && mass && ticks && levels && sched;
  return block_step<Order6>(
      n, n_act, max_level, dt, eta, state_ok, posd, veld, accd, softening_sq, workspace, workspace_bytes, stream,
      [=] {
        return nbd_hblock6_predict_f64(pos, vel, acc, jerk, snap, crackle, mass, ticks, n, max_level, dt, sched, posd,
                                       veld, accd, stream);
      },
      [=] {
        return nbd_hblock6_correct_f64(pos, vel, acc, jerk, snap, crackle, mass, ticks, levels, n, n_act, max_level, dt,
                                       eta, g_const, sched, posd, workspace, workspace_bytes, stream);
      });
}

int nbd_accel_jerk_active_f64(const double* posd, const double* veld, int n, const int* act, int n_act,
                              double softening_sq, double g_const, double* acc_out, double* jerk_out, void* workspace,
                              size_t workspace_bytes, int slabs, nbd_stream_t stream) {
  return active_force<Order4>(
      posd, veld, nullptr, n, act, n_act, softening_sq, acc_out && jerk_out, workspace, workspace_bytes, slabs, stream,
      [=](const double* part, int n_slabs, hipStream_t st) {
        hblock_correct_kernel<double><<<ceil_div(n_act, kSumRows), 256, 0, st>>>(
            part, n_slabs, act, n_act, g_const, 0, 1.0, 1.0, 1.0, nullptr, nullptr, acc_out, jerk_out, nullptr, nullptr,
            nullptr, nullptr, nullptr);
      });
}

int nbd_accel_jerk_snap_active_f64(const double* posd, const double* veld, const double* accd, int n, const int* act,
                                   int n_act, double softening_sq, double g_const, double* acc_out, double* jerk_out,
                                   double* snap_out, void* workspace, size_t workspace_bytes, int slabs,
                                   nbd_stream_t stream) {
  return active_force<Order6>(
      posd, veld, accd, n, act, n_act, softening_sq, acc_out && jerk_out && snap_out, workspace, workspace_bytes, slabs,
      stream, [=](const double* part, int n_slabs, hipStream_t st) {
        hblock6_correct_kernel<<<ceil_div(n_act, 256), 256, 0, st>>>(part, n_slabs, act, n_act, g_const, 0, 1.0, 1.0, 1.0,
                                                                     nullptr, nullptr, acc_out, jerk_out, snap_out, nullptr,
                                                                     nullptr, nullptr, nullptr, nullptr, nullptr);
      });
}

}  // extern "C"
