// direct_hermite_block_f64.hip -- the double-precision form of direct_hermite_block.hip's block-timestep 4th-order Hermite
// integration, for gfx950 (MI355X): individual power-of-two steps with the number format of direct_hermite_f64.hip. An
// extension reached only when the caller asks for float64. C-ABI: the nbd_hblock_*_f64 / nbd_accel_jerk_active_f64 entries
// of include/nbd.h under "double-precision block-timestep Hermite"; Python:
// galaxify.simulation.BlockHermiteSimulator(dtype=torch.float64).
//
// The scheme is direct_hermite_block.hip's, stage for stage; levels, ticks and the schedule record are the int32 they are
// there, and the scheduler is that unit's nbd_hblock_schedule, which reads nothing else. What is fp64 here: the state
// (x, v, a, j, m), the packed rows posd = {x, y, z, m} / veld = {vx, vy, vz, 0} of direct_hermite_f64.hip, G, eps^2, dt,
// every body's own step constants (hermite_step_constants<double> of its Delta, never rounded to fp32), the pair
// arithmetic and every sum.
//   predict  : every body to t_next over its own Delta_i = (t_next - t_i) dt 2^-K -> posd = {x_p, m}, veld = {v_p, 0}
//   evaluate : accel_jerk_active_f64_kernel -- a1, j1 of the active targets under all n predicted sources, into
//              double[slabs][6][n_act] partial sums: accel_jerk_f64_kernel with its targets gathered through the list,
//              the same walk_f64 and AccelJerkPair (hermite_f64_kernels.h)
//   correct  : the slabs in slab order, hermite_correct<double> with the body's own h, the Aarseth criterion on the fp64
//              a0, j0, a1, j1 for the new level, t_i = t_next (0 at the end of the interval), posd = {x1, m}
// The three O(N) kernels are hermite_block_kernels.h's templates at T = double (hblock_init_kernel, hblock_predict_kernel,
// hblock_correct_kernel with its hblock_relevel): the same source as the fp32 unit's, not a copy of it.
// Exclusions. Below eps^2 = 1e-24 every chunk is walked index-masked, as in the shared step. Otherwise NO chunk is: a
// gathered group has no chunk of its own. The shared kernel walks its own chunk masked, which sets s = 0 for j == i and
// for the padding, so w = c = 0 and each of the nine fma's adds a zero; un-masked, j == i has dr = dv = 0 with a finite
// w, c (s <= 1e12), and a padding row has m = 0 with a finite s, so each fma adds a zero again. A partial sum starts at
// +0 and can never become -0 (x + -x is +0 in round-to-nearest), so adding a zero of either sign leaves its bits alone:
// with every body listed the sums are the shared step's, bit for bit, in whatever order the list holds them.
// No float atomics (the clamp counter and the histogram are integer atomics), no memsets in a step; the host reads
// {t_next, n_act} once per block step (nbd_hblock_schedule), so the path is eager-only. Deterministic run to run with a
// workspace that may hold anything.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_kernels.h"
#include "hermite_block_kernels.h"
#include "hermite_f64_kernels.h"
#include "hermite_kernels.h"

namespace {

// Acceleration + jerk of the n_act targets act[0..n_act) under all n sources. Grid = (ceil(n_act / 64), slabs), block =
// 4 waves on the same 64 list entries, one per lane. The lanes behind n_act repeat the last target and store nothing.
// out: double[slab][6][n_act], in list order. A target's sums depend only on n and the slab count, not on where it sits
// in the list. (5 workgroups per CU is what 32 KiB of LDS each allows and what accel_jerk_f64_kernel reaches at 89 VGPRs;
// left alone the compiler takes 116 here, one wave per SIMD fewer. With the bound it takes 90 and spills nothing.)
__global__ __launch_bounds__(64 * kWaves, 5) void accel_jerk_active_f64_kernel(const d4* __restrict__ posd,
                                                                            const d4* __restrict__ veld, int n,
                                                                            const int* __restrict__ act, int n_act,
                                                                            int cpw_q, int cpw_r, double eps2,
                                                                            int all_masked, double* __restrict__ out) {
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads<true>()];
  const Group64<unsigned> g(blockIdx.x, blockIdx.y, n_act);      // a group of list entries: the lane's body is act[its entry]
  const ChunkRange c = wave_chunks(g.jw(), cpw_q, cpw_r);
  const int i = act[g.row()];
  AccelJerkPair pr(posd[i], veld[i], eps2, i, n);
  walk_f64(pr, posd, veld, c.begin, c.end, all_masked != 0, -1, lds, g.dst<AccelJerkPair>(out), (size_t)n_act,
           g.n_valid());
}

constexpr int kSumRows = HermiteFmt<double>::kSumRows;      // list entries per workgroup of the corrector launch

// The workspace: the active list (nbd_hblock_schedule writes it at the start, as in fp32), then, 32-byte aligned, the
// partial sums double[slabs][6][n_act]. The plan of n_act targets is plan_f64(n, n_act): with every body active that is
// the shared fp64 step's, so the sums are its bits; with fewer, fewer groups and so more slabs towards kTargetWGs
// workgroups, never more than n_chunks / 4 (every wave keeps a chunk) or kMaxSlabs.
size_t act_bytes_f64(int n) { return (size_t)ceil_div(n, 8) * 8 * sizeof(int); }

size_t slab_bytes_f64(int slabs, int n_act) { return (size_t)slabs * 6 * n_act * sizeof(double); }

// what one block step with n_act targets uses of the workspace (O(1): one plan)
size_t step_bytes_f64(int n, int n_act) {
  return act_bytes_f64(n) + (n_act > 0 ? slab_bytes_f64(plan_f64(n, n_act).slabs, n_act) : 0);
}

// the largest slabs x n_act any active set of n sources can need: the slab count depends on the group count alone, so
// the fullest list of every group count
size_t slab_rows_f64(int n) {
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
double* ws_slabs(void* ws, int n) { return reinterpret_cast<double*>(static_cast<char*>(ws) + act_bytes_f64(n)); }

int launch_active_f64(const double* posd, const double* veld, int n, const int* act, int n_act, double eps2,
                      double* slabs, int groups, int n_slabs, hipStream_t st) {
  const ChunkSplit c = chunk_split(ceil_div(n, kChunk), n_slabs);
  accel_jerk_active_f64_kernel<<<dim3(groups, n_slabs), 64 * kWaves, 0, st>>>(
      reinterpret_cast<const d4*>(posd), reinterpret_cast<const d4*>(veld), n, act, n_act, c.q, c.r, eps2,
      eps2 < kEps2MaskedF64 ? 1 : 0, slabs);
  return launch_status();
}

}  // namespace

extern "C" {

size_t nbd_hblock_f64_workspace_bytes(int n) {
  if (n <= 0) return 0;
  return act_bytes_f64(n) + slab_rows_f64(n) * 6 * sizeof(double);
}

int nbd_hblock_init_levels_f64(const double* acc, const double* jerk, int n, double dt, double eta, int max_level,
                               int* ticks, int* levels, int* sched, nbd_stream_t stream) {
  if (n < 0 || bad_level(max_level) || !(dt > 0.0) || !(eta > 0.0)) return NBD_E_BADARG;
  if (!sched) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (!acc || !jerk || !ticks || !levels) return NBD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  // T, the cursor and the histogram start from zero; t_next, n_act and the clamp count are left as they are
  hipError_t e = hipMemsetAsync(sched + kTCur, 0, (NBD_HBLOCK_SCHED_INTS - kTCur) * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  hblock_init_kernel<double><<<ceil_div(n, 256), 256, 0, st>>>(acc, jerk, n, max_level, dt, eta, ticks, levels, sched);
  return launch_status();
}

int nbd_hblock_predict_f64(const double* pos, const double* vel, const double* acc, const double* jerk,
                           const double* mass, const int* ticks, int n, int max_level, double dt, int* sched,
                           double* posd, double* veld, nbd_stream_t stream) {
  if (n <= 0 || bad_level(max_level) || !(dt > 0.0)) return NBD_E_BADARG;
  if (!pos || !vel || !acc || !jerk || !mass || !ticks || !sched || !posd || !veld) return NBD_E_BADARG;
  if (misaligned32(posd) || misaligned32(veld)) return NBD_E_BADARG;
  const int n_pad = nbd_posm_padded_len(n);
  hblock_predict_kernel<double><<<ceil_div(n_pad, 256), 256, 0, (hipStream_t)stream>>>(
      pos, vel, acc, jerk, mass, ticks, n, n_pad, dt, ldexp(1.0, -max_level), sched, reinterpret_cast<d4*>(posd),
      reinterpret_cast<d4*>(veld));
  return launch_status();
}

int nbd_hblock_force_f64(const double* posd, const double* veld, int n, int n_act, double softening_sq, void* workspace,
                         size_t workspace_bytes, nbd_stream_t stream) {
  if (n <= 0 || n_act < 0 || n_act > n || !posd || !veld || misaligned32(posd) || misaligned32(veld))
    return NBD_E_BADARG;
  if (!workspace || misaligned32(workspace) || workspace_bytes < step_bytes_f64(n, n_act)) return NBD_E_WORKSPACE;
  if (n_act == 0) return 0;
  const F64Plan p = plan_f64(n, n_act);
  return launch_active_f64(posd, veld, n, ws_act(workspace), n_act, softening_sq, ws_slabs(workspace, n), p.groups,
                           p.slabs, (hipStream_t)stream);
}

int nbd_hblock_correct_f64(double* pos, double* vel, double* acc, double* jerk, const double* mass, int* ticks,
                           int* levels, int n, int n_act, int max_level, double dt, double eta, double g_const,
                           int* sched, double* posd, void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  if (n <= 0 || n_act < 0 || n_act > n || bad_level(max_level) || !(dt > 0.0) || !(eta > 0.0)) return NBD_E_BADARG;
  if (!pos || !vel || !acc || !jerk || !mass || !ticks || !levels || !sched || !posd || misaligned32(posd))
    return NBD_E_BADARG;
  if (!workspace || misaligned32(workspace) || workspace_bytes < step_bytes_f64(n, n_act)) return NBD_E_WORKSPACE;
  if (n_act == 0) return 0;
  hblock_correct_kernel<double><<<ceil_div(n_act, kSumRows), 256, 0, (hipStream_t)stream>>>(
      ws_slabs(workspace, n), plan_f64(n, n_act).slabs, ws_act(workspace), n_act, g_const, max_level, dt,
      ldexp(1.0, -max_level), eta, pos, vel, acc, jerk, mass, ticks, levels, sched, reinterpret_cast<d4*>(posd));
  return launch_status();
}

int nbd_hblock_step_f64(double* pos, double* vel, double* acc, double* jerk, const double* mass, int* ticks, int* levels,
                        int n, int n_act, int max_level, double dt, double eta, double softening_sq, double g_const,
                        int* sched, double* posd, double* veld, void* workspace, size_t workspace_bytes,
                        nbd_stream_t stream) {
  if (n <= 0 || n_act < 1 || n_act > n || bad_level(max_level) || !(dt > 0.0) || !(eta > 0.0)) return NBD_E_BADARG;
  if (!veld || misaligned32(veld)) return NBD_E_BADARG;
  int rc = nbd_hblock_predict_f64(pos, vel, acc, jerk, mass, ticks, n, max_level, dt, sched, posd, veld, stream);
  if (rc) return rc;
  rc = nbd_hblock_force_f64(posd, veld, n, n_act, softening_sq, workspace, workspace_bytes, stream);
  if (rc) return rc;
  return nbd_hblock_correct_f64(pos, vel, acc, jerk, mass, ticks, levels, n, n_act, max_level, dt, eta, g_const, sched,
                                posd, workspace, workspace_bytes, stream);
}

int nbd_accel_jerk_active_f64(const double* posd, const double* veld, int n, const int* act, int n_act,
                              double softening_sq, double g_const, double* acc_out, double* jerk_out, void* workspace,
                              size_t workspace_bytes, int slabs, nbd_stream_t stream) {
  if (n < 0 || n_act < 0 || n_act > n || slabs < 0 || slabs > kMaxSlabs) return NBD_E_BADARG;
  if (n_act == 0) return 0;
  if (!posd || !veld || !act || !acc_out || !jerk_out || misaligned32(posd) || misaligned32(veld)) return NBD_E_BADARG;
  const F64Plan p = plan_f64(n, n_act);
  if (slabs == 0) slabs = p.slabs;
  if (!workspace || misaligned32(workspace) || workspace_bytes < act_bytes_f64(n) + slab_bytes_f64(slabs, n_act))
    return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  double* part = ws_slabs(workspace, n);
  const int rc = launch_active_f64(posd, veld, n, act, n_act, softening_sq, part, p.groups, slabs, st);
  if (rc) return rc;
  hblock_correct_kernel<double><<<ceil_div(n_act, kSumRows), 256, 0, st>>>(
      part, slabs, act, n_act, g_const, 0, 1.0, 1.0, 1.0, nullptr, nullptr, acc_out, jerk_out, nullptr, nullptr, nullptr,
      nullptr, nullptr);
  return launch_status();
}

}  // extern "C"
