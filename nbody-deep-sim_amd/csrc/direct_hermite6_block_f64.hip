// direct_hermite6_block_f64.hip -- the 6th-order Hermite scheme of direct_hermite6_f64.hip (Nitadori & Makino 2008) with
// the individual block timesteps of direct_hermite_block_f64.hip, in float64, for gfx950 (MI355X). An extension. C-ABI:
// the nbd_hblock6_*_f64 / nbd_accel_jerk_snap_active_f64 entries of include/nbd.h under "block-timestep 6th-order
// Hermite"; Python: galaxify.simulation.BlockHermite6Simulator.
//
// One output interval dt is 2^K ticks, K = max_level. Body i carries x, v, a, j, s and the crackle c at its last
// correction tick t_i and a level k_i; its step is h_i = dt 2^-k_i. Levels, ticks and the schedule record are the int32
// of the 4th-order block units, the scheduler is nbd_hblock_schedule and the initial levels nbd_hblock_init_levels_f64
// (dt_i = (eta / 2) |a| / |j|): neither reads anything else. A block step to t_next:
//   predict  : hblock6_predict_kernel -- every body over its own Delta_i = (t_next - t_i) dt 2^-K by
//              hermite6_predict_row with hermite6_step_constants(Delta_i) -> posd = {x_p, m}, veld = {v_p, 0},
//              accd = {a_p, 0}, zero rows behind n
//   evaluate : accel_jerk_snap_active_f64_kernel -- a1, j1, s1 of the active targets under all n predicted sources into
//              double[slabs][9][n_act] partial sums in list order: accel_jerk_snap_f64_kernel with its targets gathered
//              through the list, the same walk_f64 and AccelJerkSnapPair (hermite6_f64_kernels.h)
//   correct  : hblock6_correct_kernel -- the slabs in slab order, hermite6_finish_row with hermite6_step_constants(h_i):
//              x, v in place, a, j, s, c stored, posd[i] = {x1, m}; then hblock6_relevel (hermite_block_kernels.h): the
//              generalised Aarseth criterion for p = 6 on both ends of the step, hblock_relevel's level rules
// A body whose step is the whole interval gets the shared step's constants, and with every body listed the sums are the
// shared step's, so max_level = 0 is nbd_hermite6_step_f64 bit for bit.
// Exclusions are direct_hermite_block_f64.hip's: below eps^2 = 1e-24 every chunk is walked index-masked, otherwise none
// is (a gathered group has no chunk of its own): i == j (r = v = a = 0, s finite) and a padding row (m = 0) add exact
// zeros to all eighteen sums, which start at +0 and cannot become -0.
// Resources (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage): accel_jerk_snap_active_f64_kernel
// takes 164 VGPRs, 0 AGPRs, no SGPR or VGPR spills, no scratch, 48 KiB of LDS, 3 waves per SIMD: three workgroups per CU
// by the LDS and by the registers alike, the figures of accel_jerk_snap_f64_kernel (164 VGPRs, 48 KiB, 3 waves per SIMD),
// with no second __launch_bounds__ argument. hblock6_predict_kernel: 50 VGPRs; hblock6_correct_kernel: 98; no spills.
// No float atomics (the clamp counter and the histogram are integer atomics), no memsets in a step; the host reads
// {t_next, n_act} once per block step, so the path is eager-only. Deterministic run to run with a workspace that may
// hold anything.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_kernels.h"
#include "hermite6_f64_kernels.h"
#include "hermite_block_kernels.h"
#include "hermite_f64_kernels.h"
#include "hermite_kernels.h"

namespace {

// Acceleration + jerk + snap of the n_act targets act[0..n_act) under all n sources. Grid = (ceil(n_act / 64), slabs),
// block = 4 waves on the same 64 list entries, one per lane. The lanes behind n_act repeat the last target and store
// nothing. out: double[slab][9][n_act], in list order. A target's sums depend only on n and the slab count, not on where
// it sits in the list.
__global__ __launch_bounds__(64 * kWaves) void accel_jerk_snap_active_f64_kernel(
    const d4* __restrict__ posd, const d4* __restrict__ veld, const d4* __restrict__ accd, int n,
    const int* __restrict__ act, int n_act, int cpw_q, int cpw_r, double eps2, int all_masked,
    double* __restrict__ out) {
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads_n<3>()];
  const Group64<unsigned> g(blockIdx.x, blockIdx.y, n_act);      // a group of list entries: the lane's body is act[its entry]
  const ChunkRange c = wave_chunks(g.jw(), cpw_q, cpw_r);
  const int i = act[g.row()];
  AccelJerkSnapPair pr(posd[i], veld[i], accd[i], eps2, i, n);
  walk_f64(pr, posd, veld, c.begin, c.end, all_masked != 0, -1, lds, g.dst<AccelJerkSnapPair>(out), (size_t)n_act,
           g.n_valid(), nullptr, accd);
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
    const Hermite6Step h = hermite6_step_constants(dt * (double)(sched[kTNext] - ticks[i]) * tick);
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
  const double h = dt * (double)d * tick;
  const Hermite6Ends e = hermite6_finish_row(slabs, n_slabs, (size_t)n_act, p, (size_t)i, g, hermite6_step_constants(h),
                                             pos, vel, acc, jerk, snap, acc, jerk, snap, crackle, mass, posd, (size_t)i);
  hblock6_relevel(e.a0, e.j0, e.s0, e.a1, e.j1, e.s1, e.c1, h, dt, eta, K, lev, d, i, p == 0, ticks, levels, sched);
}

// The workspace: the active list (nbd_hblock_schedule writes it at the start, as in the 4th-order units), then, 32-byte
// aligned, the partial sums double[slabs][9][n_act]. The plan of n_act targets is plan_f64(n, n_act), as in
// direct_hermite_block_f64.hip: with every body active that is the shared 6th-order step's.
size_t act_bytes6(int n) { return (size_t)ceil_div(n, 8) * 8 * sizeof(int); }

size_t slab_bytes6(int slabs, int n_act) { return (size_t)slabs * 9 * n_act * sizeof(double); }

// what one block step with n_act targets uses of the workspace (O(1): one plan)
size_t step_bytes6(int n, int n_act) {
  return act_bytes6(n) + (n_act > 0 ? slab_bytes6(plan_f64(n, n_act).slabs, n_act) : 0);
}

// the largest slabs x n_act any active set of n sources can need: the slab count depends on the group count alone, so
// the fullest list of every group count
size_t slab_rows6(int n) {
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
double* ws_slabs(void* ws, int n) { return reinterpret_cast<double*>(static_cast<char*>(ws) + act_bytes6(n)); }

int launch_active6(const double* posd, const double* veld, const double* accd, int n, const int* act, int n_act,
                   double eps2, double* slabs, int groups, int n_slabs, hipStream_t st) {
  const ChunkSplit c = chunk_split(ceil_div(n, kChunk), n_slabs);
  accel_jerk_snap_active_f64_kernel<<<dim3(groups, n_slabs), 64 * kWaves, 0, st>>>(
      reinterpret_cast<const d4*>(posd), reinterpret_cast<const d4*>(veld), reinterpret_cast<const d4*>(accd), n, act,
      n_act, c.q, c.r, eps2, eps2 < kEps2MaskedF64 ? 1 : 0, slabs);
  return launch_status();
}

}  // namespace

extern "C" {

size_t nbd_hblock6_f64_workspace_bytes(int n) {
  if (n <= 0) return 0;
  return act_bytes6(n) + slab_rows6(n) * 9 * sizeof(double);
}

int nbd_hblock6_predict_f64(const double* pos, const double* vel, const double* acc, const double* jerk,
                            const double* snap, const double* crackle, const double* mass, const int* ticks, int n,
                            int max_level, double dt, int* sched, double* posd, double* veld, double* accd,
                            nbd_stream_t stream) {
  if (n <= 0 || bad_level(max_level) || !(dt > 0.0)) return NBD_E_BADARG;
  if (!pos || !vel || !acc || !jerk || !snap || !crackle || !mass || !ticks || !sched || !posd || !veld || !accd)
    return NBD_E_BADARG;
  if (misaligned32(posd) || misaligned32(veld) || misaligned32(accd)) return NBD_E_BADARG;
  const int n_pad = nbd_posm_padded_len(n);
  hblock6_predict_kernel<<<ceil_div(n_pad, 256), 256, 0, (hipStream_t)stream>>>(
      pos, vel, acc, jerk, snap, crackle, mass, ticks, n, n_pad, dt, ldexp(1.0, -max_level), sched,
      reinterpret_cast<d4*>(posd), reinterpret_cast<d4*>(veld), reinterpret_cast<d4*>(accd));
  return launch_status();
}

int nbd_hblock6_force_f64(const double* posd, const double* veld, const double* accd, int n, int n_act,
                          double softening_sq, void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  if (n <= 0 || n_act < 0 || n_act > n || !posd || !veld || !accd || misaligned32(posd) || misaligned32(veld) ||
      misaligned32(accd))
    return NBD_E_BADARG;
  if (!workspace || misaligned32(workspace) || workspace_bytes < step_bytes6(n, n_act)) return NBD_E_WORKSPACE;
  if (n_act == 0) return 0;
  const F64Plan p = plan_f64(n, n_act);
  return launch_active6(posd, veld, accd, n, ws_act(workspace), n_act, softening_sq, ws_slabs(workspace, n), p.groups,
                        p.slabs, (hipStream_t)stream);
}

int nbd_hblock6_correct_f64(double* pos, double* vel, double* acc, double* jerk, double* snap, double* crackle,
                            const double* mass, int* ticks, int* levels, int n, int n_act, int max_level, double dt,
                            double eta, double g_const, int* sched, double* posd, void* workspace,
                            size_t workspace_bytes, nbd_stream_t stream) {
  if (n <= 0 || n_act < 0 || n_act > n || bad_level(max_level) || !(dt > 0.0) || !(eta > 0.0)) return NBD_E_BADARG;
  if (!pos || !vel || !acc || !jerk || !snap || !crackle || !mass || !ticks || !levels || !sched || !posd ||
      misaligned32(posd))
    return NBD_E_BADARG;
  if (!workspace || misaligned32(workspace) || workspace_bytes < step_bytes6(n, n_act)) return NBD_E_WORKSPACE;
  if (n_act == 0) return 0;
  hblock6_correct_kernel<<<ceil_div(n_act, 256), 256, 0, (hipStream_t)stream>>>(
      ws_slabs(workspace, n), plan_f64(n, n_act).slabs, ws_act(workspace), n_act, g_const, max_level, dt,
      ldexp(1.0, -max_level), eta, pos, vel, acc, jerk, snap, crackle, mass, ticks, levels, sched,
      reinterpret_cast<d4*>(posd));
  return launch_status();
}

int nbd_hblock6_step_f64(double* pos, double* vel, double* acc, double* jerk, double* snap, double* crackle,
                         const double* mass, int* ticks, int* levels, int n, int n_act, int max_level, double dt,
                         double eta, double softening_sq, double g_const, int* sched, double* posd, double* veld,
                         double* accd, void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  if (n <= 0 || n_act < 1 || n_act > n || bad_level(max_level) || !(dt > 0.0) || !(eta > 0.0)) return NBD_E_BADARG;
  // everything the later stages refuse, before the first launch
  if (!pos || !vel || !acc || !jerk || !snap || !crackle || !mass || !ticks || !levels || !sched || !posd || !veld ||
      !accd || misaligned32(posd) || misaligned32(veld) || misaligned32(accd))
    return NBD_E_BADARG;
  if (!workspace || misaligned32(workspace) || workspace_bytes < step_bytes6(n, n_act)) return NBD_E_WORKSPACE;
  int rc = nbd_hblock6_predict_f64(pos, vel, acc, jerk, snap, crackle, mass, ticks, n, max_level, dt, sched, posd, veld,
                                   accd, stream);
  if (rc) return rc;
  rc = nbd_hblock6_force_f64(posd, veld, accd, n, n_act, softening_sq, workspace, workspace_bytes, stream);
  if (rc) return rc;
  return nbd_hblock6_correct_f64(pos, vel, acc, jerk, snap, crackle, mass, ticks, levels, n, n_act, max_level, dt, eta,
                                 g_const, sched, posd, workspace, workspace_bytes, stream);
}

int nbd_accel_jerk_snap_active_f64(const double* posd, const double* veld, const double* accd, int n, const int* act,
                                   int n_act, double softening_sq, double g_const, double* acc_out, double* jerk_out,
                                   double* snap_out, void* workspace, size_t workspace_bytes, int slabs,
                                   nbd_stream_t stream) {
  if (n < 0 || n_act < 0 || n_act > n || slabs < 0 || slabs > kMaxSlabs) return NBD_E_BADARG;
  if (n_act == 0) return 0;
  if (!posd || !veld || !accd || !act || !acc_out || !jerk_out || !snap_out || misaligned32(posd) ||
      misaligned32(veld) || misaligned32(accd))
    return NBD_E_BADARG;
  const F64Plan p = plan_f64(n, n_act);
  if (slabs == 0) slabs = p.slabs;
  if (!workspace || misaligned32(workspace) || workspace_bytes < act_bytes6(n) + slab_bytes6(slabs, n_act))
    return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  double* part = ws_slabs(workspace, n);
  const int rc = launch_active6(posd, veld, accd, n, act, n_act, softening_sq, part, p.groups, slabs, st);
  if (rc) return rc;
  hblock6_correct_kernel<<<ceil_div(n_act, 256), 256, 0, st>>>(part, slabs, act, n_act, g_const, 0, 1.0, 1.0, 1.0,
                                                               nullptr, nullptr, acc_out, jerk_out, snap_out, nullptr,
                                                               nullptr, nullptr, nullptr, nullptr, nullptr);
  return launch_status();
}

}  // extern "C"
