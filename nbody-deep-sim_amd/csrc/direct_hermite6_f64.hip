// direct_hermite6_f64.hip -- the shared-timestep 6th-order Hermite step (Nitadori & Makino 2008) in the number format of
// direct_hermite_f64.hip, for gfx950 (MI355X). An extension, float64 only: the fp32 Hermite run already sits on the fp32
// floor at a few dozen steps, so a higher order buys nothing there. C-ABI: the nbd_*hermite6* entries of include/nbd.h
// under "6th-order Hermite"; Python: galaxify.simulation.Hermite6Simulator.
//
// Pair terms for target i and source j, with r = x_j - x_i, v = v_j - v_i, a = a_j - a_i, s = (|r|^2 + eps^2)^(-1/2):
//   w = m_j s^3,  alpha = (r.v) s^2,  gamma = (v.v + r.a) s^2
//   A_ij = w r,  J_ij = w v - 3 alpha w r,  S_ij = w a - 6 alpha w v + (15 alpha^2 - 3 gamma) w r
// The sources are three arrays of 32-byte rows: posd = {x, y, z, m}, veld = {vx, vy, vz, 0} and accd = {ax, ay, az, 0},
// zero rows behind n up to a multiple of 64. The evaluation is walk_f64 (hermite_f64_kernels.h) with three streamed
// arrays and the pair functor AccelJerkSnapPair (hermite6_f64_kernels.h), in accel_jerk_f64_kernel's geometry (plan_f64,
// chunk_split, four waves on 64 targets, LDS-DMA double buffering, the counted vmcnt(6)); 48 KiB of LDS per workgroup:
// three per CU.
//
// One step is three launches (PEC form; a0, j0, s0 and the crackle c0 = d^3 a / dt^3 carried):
//   predict : hermite6_predict_kernel -> posd = {x_p, m}, veld = {v_p, 0}, accd = {a_p, 0}, Taylor series to c0
//   evaluate: accel_jerk_snap_f64_kernel -> double[slabs][9][n] partial sums (unscaled)
//   correct : hermite6_finish_kernel: the slabs in slab order (slab_order_sum<9>, one thread per body), a1, j1, s1 = G sum,
//             the corrector, c1 = the third derivative at t1 of the quintic through (a, j, s) at both ends, posd = {x1, m}
// The step constants are doubles formed from the double dt and are never rounded to fp32; every product and sum of the
// two O(N) kernels rounds on its own (the build has -ffp-contract=off). No atomics, no memsets, no host syncs:
// deterministic run to run with a workspace that may hold anything. The functor, the step constants and the per-row
// bodies of the two O(N) kernels are in hermite6_f64_kernels.h, shared with direct_batch_hermite6_f64.hip (many systems).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_kernels.h"
#include "hermite6_f64_kernels.h"
#include "hermite_f64_kernels.h"
#include "hermite_kernels.h"

namespace {

// Acceleration + jerk + snap of all n bodies under all n bodies, accel_jerk_f64_kernel's geometry: grid = (groups of 64
// targets, slabs), the source chunks spread over all slabs x 4 waves to within one. out: double[slab][9][n].
__global__ __launch_bounds__(64 * kWaves) void accel_jerk_snap_f64_kernel(const d4* __restrict__ posd,
                                                                          const d4* __restrict__ veld,
                                                                          const d4* __restrict__ accd, int n, int cpw_q,
                                                                          int cpw_r, double eps2, int all_masked,
                                                                          double* __restrict__ out) {
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads_n<3>()];
  const Group64<unsigned> g(blockIdx.x, blockIdx.y, n);
  const ChunkRange c = wave_chunks(g.jw(), cpw_q, cpw_r);
  AccelJerkSnapPair pr(posd[g.row()], veld[g.row()], accd[g.row()], eps2, g.i, n);
  walk_f64(pr, posd, veld, c.begin, c.end, all_masked != 0, blockIdx.x, lds, g.dst<AccelJerkSnapPair>(out), (size_t)n,
           g.n_valid(), nullptr, accd);
}

// posd = {x_p, m}, veld = {v_p, 0}, accd = {a_p, 0} for rows [0, n_pad), zero rows behind n:
//   x_p = x + v dt + a dt^2/2 + j dt^3/6 + s dt^4/24 + c dt^5/120,  v_p = v + a dt + j dt^2/2 + s dt^3/6 + c dt^4/24,
//   a_p = a + j dt + s dt^2/2 + c dt^3/6.
// jerk == nullptr (then snap and crackle are too): a plain pack of (pos, vel, acc); acc == nullptr as well: accd = 0.
__global__ __launch_bounds__(256) void hermite6_predict_kernel(const double* __restrict__ pos,
                                                               const double* __restrict__ vel,
                                                               const double* __restrict__ acc,
                                                               const double* __restrict__ jerk,
                                                               const double* __restrict__ snap,
                                                               const double* __restrict__ crackle,
                                                               const double* __restrict__ mass, int n, int n_pad,
                                                               Hermite6Step h, d4* __restrict__ posd,
                                                               d4* __restrict__ veld, d4* __restrict__ accd) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n_pad) return;
  d4 pm = {0.0, 0.0, 0.0, 0.0}, vp = pm, ap = pm;
  if (i < (size_t)n) hermite6_predict_row(pos, vel, acc, jerk, snap, crackle, mass, i, h, pm, vp, ap);
  posd[i] = pm;
  veld[i] = vp;
  accd[i] = ap;
}

// One thread per body: a1, j1, s1 = G (slab 0 + slab 1 + ...) of double[n_slabs][9][n] in slab order. pos == nullptr:
// write them only (the force on its own). Else the corrector
//   v1 = v + (a0 + a1) dt/2 - (j1 - j0) dt^2/10 + (s0 + s1) dt^3/120
//   x1 = x + (v + v1) dt/2 - (a1 - a0) dt^2/10 + (j0 + j1) dt^3/120
//   c1 = [60 (a1 - a0) - dt (36 j1 + 24 j0) + dt^2 (9 s1 - 3 s0)] / dt^3
// with pos and vel in place and posd = {x1, m}. The outputs may alias acc_in, jerk_in, snap_in: each element is read
// before it is written, by the same thread.
__global__ __launch_bounds__(256) void hermite6_finish_kernel(const double* __restrict__ slabs, int n_slabs, int n,
                                                              double g, Hermite6Step h, double* pos, double* vel,
                                                              const double* acc_in, const double* jerk_in,
                                                              const double* snap_in, double* acc_out, double* jerk_out,
                                                              double* snap_out, double* crackle_out,
                                                              const double* __restrict__ mass, d4* __restrict__ posd) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n) return;
  hermite6_finish_row(slabs, n_slabs, (size_t)n, i, i, g, h, pos, vel, acc_in, jerk_in, snap_in, acc_out, jerk_out,
                      snap_out, crackle_out, mass, posd, i);
}

// the unscaled acceleration + jerk + snap partial sums of every body into double[slabs][9][n]
int launch_snap_f64(const double* posd, const double* veld, const double* accd, int n, double eps2, double* out,
                    const F64Plan& p, int slabs, hipStream_t st) {
  const ChunkSplit c = chunk_split(p.n_chunks, slabs);
  accel_jerk_snap_f64_kernel<<<dim3(p.groups, slabs), 64 * kWaves, 0, st>>>(
      reinterpret_cast<const d4*>(posd), reinterpret_cast<const d4*>(veld), reinterpret_cast<const d4*>(accd), n, c.q,
      c.r, eps2, eps2 < kEps2MaskedF64 ? 1 : 0, out);
  return launch_status();
}

}  // namespace

extern "C" {

size_t nbd_hermite6_f64_workspace_bytes(int n) {
  if (n <= 0) return 0;
  return (size_t)plan_f64(n).slabs * 9 * n * sizeof(double);
}

int nbd_hermite6_f64_pack(const double* pos, const double* vel, const double* acc, const double* jerk,
                          const double* snap, const double* crackle, const double* mass, int n, double dt, double* posd,
                          double* veld, double* accd, nbd_stream_t stream) {
  if (n < 0 || (n > 0 && (!pos || !vel || !mass || !posd || !veld || !accd))) return NBD_E_BADARG;
  if ((!jerk != !snap) || (!jerk != !crackle) || (jerk && !acc)) return NBD_E_BADARG;
  if (misaligned32(posd) || misaligned32(veld) || misaligned32(accd)) return NBD_E_BADARG;
  if (n == 0) return 0;
  const int n_pad = nbd_posm_padded_len(n);
  hermite6_predict_kernel<<<ceil_div(n_pad, 256), 256, 0, (hipStream_t)stream>>>(
      pos, vel, acc, jerk, snap, crackle, mass, n, n_pad, hermite6_step_constants(dt), reinterpret_cast<d4*>(posd),
      reinterpret_cast<d4*>(veld), reinterpret_cast<d4*>(accd));
  return launch_status();
}

int nbd_accel_jerk_snap_f64(const double* posd, const double* veld, const double* accd, int n, double softening_sq,
                            double g_const, double* acc_out, double* jerk_out, double* snap_out, void* workspace,
                            size_t workspace_bytes, int slabs, nbd_stream_t stream) {
  if (n < 0 || slabs < 0 || slabs > kMaxSlabs) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (!posd || !veld || !accd || !acc_out || !jerk_out || !snap_out || misaligned32(posd) || misaligned32(veld) ||
      misaligned32(accd))
    return NBD_E_BADARG;
  const F64Plan p = plan_f64(n);
  if (slabs == 0) slabs = p.slabs;
  if (!workspace || misaligned8(workspace) || workspace_bytes < (size_t)slabs * 9 * n * sizeof(double))
    return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  double* part = static_cast<double*>(workspace);
  const int rc = launch_snap_f64(posd, veld, accd, n, softening_sq, part, p, slabs, st);
  if (rc) return rc;
  hermite6_finish_kernel<<<ceil_div(n, 256), 256, 0, st>>>(part, slabs, n, g_const, hermite6_step_constants(0.0),
                                                          nullptr, nullptr, nullptr, nullptr, nullptr, acc_out,
                                                          jerk_out, snap_out, nullptr, nullptr, nullptr);
  return launch_status();
}

int nbd_hermite6_step_f64(double* pos, double* vel, const double* acc_in, const double* jerk_in, const double* snap_in,
                          const double* crackle_in, double* acc_out, double* jerk_out, double* snap_out,
                          double* crackle_out, const double* mass, int n, double dt, double softening_sq, double g_const,
                          double* posd, double* veld, double* accd, void* workspace, size_t workspace_bytes,
                          nbd_stream_t stream) {
  if (n < 0) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (!pos || !vel || !acc_in || !jerk_in || !snap_in || !crackle_in || !acc_out || !jerk_out || !snap_out ||
      !crackle_out || !mass || !posd || !veld || !accd || misaligned32(posd) || misaligned32(veld) || misaligned32(accd))
    return NBD_E_BADARG;
  if (!workspace || misaligned8(workspace) || workspace_bytes < nbd_hermite6_f64_workspace_bytes(n))
    return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const Hermite6Step h = hermite6_step_constants(dt);
  const F64Plan p = plan_f64(n);
  double* part = static_cast<double*>(workspace);
  const int n_pad = nbd_posm_padded_len(n);
  hermite6_predict_kernel<<<ceil_div(n_pad, 256), 256, 0, st>>>(
      pos, vel, acc_in, jerk_in, snap_in, crackle_in, mass, n, n_pad, h, reinterpret_cast<d4*>(posd),
      reinterpret_cast<d4*>(veld), reinterpret_cast<d4*>(accd));
  int rc = launch_status();
  if (rc) return rc;
  if ((rc = launch_snap_f64(posd, veld, accd, n, softening_sq, part, p, p.slabs, st))) return rc;
  hermite6_finish_kernel<<<ceil_div(n, 256), 256, 0, st>>>(part, p.slabs, n, g_const, h, pos, vel, acc_in, jerk_in,
                                                          snap_in, acc_out, jerk_out, snap_out, crackle_out, mass,
                                                          reinterpret_cast<d4*>(posd));
  return launch_status();
}

}  // extern "C"
