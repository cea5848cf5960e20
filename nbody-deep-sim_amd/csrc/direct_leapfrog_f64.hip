// direct_leapfrog_f64.hip -- the double-precision form of the leapfrog (kick-drift-kick) and Euler steps of
// direct_force.hip and of the all-pairs acceleration on its own, for gfx950 (MI355X), in the number format of
// direct_hermite_f64.hip: state, scalars, pair arithmetic and every sum are fp64, the sources are posd = {x, y, z, m} rows
// of 32 bytes with zero rows behind n up to a multiple of 64. An extension: the reference is fp32 only; nothing here is
// reached unless the caller asks for float64. C-ABI: the entries of include/nbd.h under "double-precision leapfrog";
// Python: galaxify.simulation.LeapFrogSimulator / EulerSimulator(dtype=torch.float64).
//
// The force is walk_f64 (hermite_f64_kernels.h) with the pair functor AccelPair: AccelJerkPair's operations for the
// acceleration, one for one and in the same order, with ONE streamed array and half the LDS. Same plan (plan_f64), same
// split of the chunks (chunk_split / wave_chunk_range), same wave-order and slab-order sums, a = G * sum: nbd_accel_f64
// returns the bits of nbd_accel_jerk_f64's acceleration at every n and slab count.
//
// A leapfrog step is three launches (a0 carried):
//   kick-drift-pack: v += (dt/2) a0, x += dt v, posd = {x, m}                  leapfrog_pack_f64_kernel
//   force          : double[slabs][3][n] partial sums (unscaled)                accel_f64_kernel
//   finish-kick    : the slabs in slab order, a1 = G sum, v += (dt/2) a1        leapfrog_finish_f64_kernel<false>
// An Euler step is three launches as well, in the reference's order a(t), v += dt a, x += dt v:
//   pack           : posd = {x, m}                                              leapfrog_pack_f64_kernel (no acceleration)
//   force          : as above
//   finish         : a = G sum, v += dt a, x += dt v                            leapfrog_finish_f64_kernel<true>
// (posd keeps the positions from BEFORE the drift, as the fp32 Euler step leaves posm.)
// Every product and sum of the O(N) kernels rounds on its own (-ffp-contract=off). No atomics, no memsets, no host syncs:
// deterministic run to run with a workspace that may hold anything, and capturable.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_kernels.h"
#include "hermite_f64_kernels.h"
#include "hermite_kernels.h"

namespace {

// The acceleration of all n bodies under all n bodies: force_f64_kernel's geometry (direct_hermite_f64.hip) -- grid =
// (groups of 64 targets, slabs), the n_chunks source chunks spread over all slabs x 4 waves to within one. out: double[slab][3][n].
__global__ __launch_bounds__(64 * kWaves) void accel_f64_kernel(const d4* __restrict__ posd, int n, int cpw_q, int cpw_r,
                                                                double eps2, int all_masked, double* __restrict__ out) {
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads<false>()];
  const Group64<unsigned> g(blockIdx.x, blockIdx.y, n);
  const ChunkRange c = wave_chunks(g.jw(), cpw_q, cpw_r);
  AccelPair pr(posd[g.row()], eps2, g.i, n);
  walk_f64(pr, posd, posd, c.begin, c.end, all_masked != 0, blockIdx.x, lds, g.dst<AccelPair>(out), (size_t)n,
           g.n_valid());
}

// v += c_half a ; x += dt v ; posd = {x, m} for rows [0, n_pad), zero rows behind n. acc == nullptr: a plain pack of the
// positions as they are (no kick, no drift).
__global__ __launch_bounds__(256) void leapfrog_pack_f64_kernel(double* __restrict__ pos, double* __restrict__ vel,
                                                                const double* __restrict__ acc,
                                                                const double* __restrict__ mass, int n, int n_pad,
                                                                double c_half, double dt, d4* __restrict__ posd) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n_pad) return;
  d4 pm = {0.0, 0.0, 0.0, 0.0};
  if (i < (size_t)n) {
    double x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      x[k] = pos[3 * i + k];
      if (acc) {
        const double v = vel[3 * i + k] + c_half * acc[3 * i + k];
        vel[3 * i + k] = v;
        x[k] = x[k] + dt * v;
        pos[3 * i + k] = x[k];
      }
    }
    pm = d4{x[0], x[1], x[2], mass[i]};
  }
  posd[i] = pm;
}

// a = g * (slab 0 + slab 1 + ...) in slab order -- hermite_correct_kernel<double>'s expression for a1 --, v += c a, and
// with DRIFT (the Euler step) x += c v. One thread per body.
template <bool DRIFT>
__global__ __launch_bounds__(256) void leapfrog_finish_f64_kernel(const double* __restrict__ slabs, int n_slabs, int n,
                                                                  double g, double c, double* __restrict__ acc,
                                                                  double* __restrict__ vel, double* __restrict__ pos) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n) return;
  double sum[3];
  slab_order_sum<3>(slabs, n_slabs, (size_t)n, i, sum);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a = g * sum[k];
    acc[3 * i + k] = a;
    if (vel) {
      const double v = vel[3 * i + k] + c * a;
      vel[3 * i + k] = v;
      if (DRIFT) pos[3 * i + k] = pos[3 * i + k] + c * v;
    }
  }
}

size_t accel_bytes(int n, int slabs) { return (size_t)slabs * AccelPair::kOut * n * sizeof(double); }

// the unscaled acceleration partial sums of every body into double[slabs][3][n]
int launch_accel_f64(const double* posd, int n, double eps2, double* out, const F64Plan& p, int slabs, hipStream_t st) {
  const ChunkSplit c = chunk_split(p.n_chunks, slabs);
  accel_f64_kernel<<<dim3(p.groups, slabs), 64 * kWaves, 0, st>>>(reinterpret_cast<const d4*>(posd), n, c.q, c.r, eps2,
                                                                   eps2 < kEps2MaskedF64 ? 1 : 0, out);
  return launch_status();
}

// What the two steps share: the checks, the first launch (kick-drift-pack, or the plain pack when acc_in is null), the
// force, and the finishing launch (with the drift when acc_in is null: the Euler step).
int step_f64(double* pos, double* vel, const double* acc_in, double* acc_out, const double* mass, int n, double c_kick,
             double dt, double eps2, double g, double* posd, void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (n < 0) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (!pos || !vel || !acc_out || !mass || !posd || misaligned32(posd)) return NBD_E_BADARG;
  const F64Plan p = plan_f64(n);
  if (!workspace || misaligned8(workspace) || workspace_bytes < accel_bytes(n, p.slabs)) return NBD_E_WORKSPACE;
  double* part = static_cast<double*>(workspace);
  const int n_pad = nbd_posm_padded_len(n);
  leapfrog_pack_f64_kernel<<<ceil_div(n_pad, 256), 256, 0, st>>>(pos, vel, acc_in, mass, n, n_pad, c_kick, dt,
                                                                 reinterpret_cast<d4*>(posd));
  int rc = launch_status();
  if (rc) return rc;
  if ((rc = launch_accel_f64(posd, n, eps2, part, p, p.slabs, st))) return rc;
  if (acc_in)
    leapfrog_finish_f64_kernel<false><<<ceil_div(n, 256), 256, 0, st>>>(part, p.slabs, n, g, c_kick, acc_out, vel, pos);
  else
    leapfrog_finish_f64_kernel<true><<<ceil_div(n, 256), 256, 0, st>>>(part, p.slabs, n, g, dt, acc_out, vel, pos);
  return launch_status();
}

}  // namespace

extern "C" {

size_t nbd_accel_f64_workspace_bytes(int n, int slabs) {
  if (n <= 0 || slabs < 0 || slabs > kMaxSlabs) return 0;
  return accel_bytes(n, slabs ? slabs : plan_f64(n).slabs);
}

int nbd_accel_f64(const double* posd, int n, double softening_sq, double g_const, double* acc_out, void* workspace,
                  size_t workspace_bytes, int slabs, nbd_stream_t stream) {
  if (n < 0 || slabs < 0 || slabs > kMaxSlabs) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (!posd || !acc_out || misaligned32(posd)) return NBD_E_BADARG;
  const F64Plan p = plan_f64(n);
  if (slabs == 0) slabs = p.slabs;
  if (!workspace || misaligned8(workspace) || workspace_bytes < accel_bytes(n, slabs)) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  double* part = static_cast<double*>(workspace);
  const int rc = launch_accel_f64(posd, n, softening_sq, part, p, slabs, st);
  if (rc) return rc;
  leapfrog_finish_f64_kernel<false><<<ceil_div(n, 256), 256, 0, st>>>(part, slabs, n, g_const, 0.0, acc_out, nullptr,
                                                                      nullptr);
  return launch_status();
}

int nbd_leapfrog_step_f64(double* pos, double* vel, const double* acc_in, double* acc_out, const double* mass, int n,
                          double dt_half, double dt, double softening_sq, double g_const, double* posd, void* workspace,
                          size_t workspace_bytes, nbd_stream_t stream) {
  if (n > 0 && !acc_in) return NBD_E_BADARG;
  return step_f64(pos, vel, acc_in, acc_out, mass, n, dt_half, dt, softening_sq, g_const, posd, workspace,
                  workspace_bytes, (hipStream_t)stream);
}

int nbd_euler_step_f64(double* pos, double* vel, double* acc_out, const double* mass, int n, double dt,
                       double softening_sq, double g_const, double* posd, void* workspace, size_t workspace_bytes,
                       nbd_stream_t stream) {
  return step_f64(pos, vel, nullptr, acc_out, mass, n, 0.0, dt, softening_sq, g_const, posd, workspace, workspace_bytes,
                  (hipStream_t)stream);
}

}  // extern "C"
