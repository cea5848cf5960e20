// direct_hermite_f64.hip -- the shared-timestep Hermite steps in double precision for gfx950 (MI355X), 4th order (the
// double-precision form of direct_hermite.hip's step) and 6th order (Nitadori & Makino 2008), and the diagnostics that go
// with them. An extension: the reference is fp32 only; nothing here is reached unless the caller asks for float64 (the 6th
// order is float64 only: the fp32 Hermite run already sits on the fp32 floor at a few dozen steps, so a higher order buys
// nothing there). C-ABI: the nbd_*_f64 entries of include/nbd.h under "double-precision Hermite" and the nbd_*hermite6*
// entries under "6th-order Hermite"; Python: galaxify.simulation.HermiteSimulator(dtype=torch.float64) and
// Hermite6Simulator.
//
// State, scalars, pair arithmetic and every sum are fp64; there is no fp32 intermediate anywhere. The sources are arrays of
// 32-byte rows, posd = {x, y, z, m}, veld = {vx, vy, vz, 0} and, at the 6th order, accd = {ax, ay, az, 0}, zero rows behind
// n up to a multiple of 64.
//
// One wave body (walk_f64) for all the O(N^2) sums, parametrised by the pair functor -- acceleration + jerk
// (AccelJerkPair), acceleration + jerk + snap (AccelJerkSnapPair, hermite6_f64_kernels.h), the Plummer potential of the
// force's softening (PotentialPair), the reference's pair energy -m_i m_j / (|r| + eps) (EnergyPair). The structure is the
// fp32 units' (accel_jerk_body, hermite_kernels.h): a workgroup is 4 waves on the same 64 targets, ONE per lane (there is
// no packed fp64 arithmetic to fill with a second one); every wave streams its own chunks of 64 sources through LDS by
// LDS-DMA, double-buffered behind a counted vmcnt; the chunks are split over slabs x 4 waves by the balanced split
// (chunk_split / wave_chunk_range); the four waves' partials are added through LDS in wave order, the slabs by a
// finishing launch in slab order. No atomics, no memsets, no host syncs: deterministic run to run with a workspace that
// may hold anything, and capturable.
//
// The reciprocal square root: v_rsq_f64 as the seed -- its input range is all of fp64, so no separation or softening has
// to fit the fp32 exponent range as it would for a v_rsq_f32 seed -- refined by one third-order and one second-order
// Newton step on the fma residual 1 - x y^2 (rsqrt_f64). The second step squares whatever the first leaves, so the result
// is good to the rounding of its last two operations (about 1 ulp) for any seed better than 2^-10.
//
// One step is three launches, as in fp32 (PEC form), with one force kernel and one pair of host bodies (shared_force,
// shared_step) for both orders; what the orders differ in (Order4, Order6 of hermite_orders_f64.h; the O(N) kernels and the
// pointer lists of the entries):
//   4th : a0, j0 carried; packed rows {x_p, m}, {v_p, 0}
//     predict : hermite_predict_kernel<double>
//     evaluate: force_f64_kernel<Order4> -> double[slabs][6][n] partial sums (unscaled)
//     finish  : hermite_correct_kernel<double>: the slabs in slab order (slab_order_sum, one thread per body), a1 = G sum,
//               j1 = G sum, the corrector, posd = {x1, m}
//   6th : a0, j0, s0 and the crackle c0 = d^3 a / dt^3 carried; packed rows ... and {a_p, 0}
//     predict : hermite6_predict_kernel<1>: Taylor series to c0
//     evaluate: force_f64_kernel<Order6> -> double[slabs][9][n]
//     finish  : hermite6_finish_kernel<>: slab_order_sum<9>, a1, j1, s1 = G sum, the corrector, c1 = the third derivative at
//               t1 of the quintic through (a, j, s) at both ends, posd = {x1, m}
// The 4th order's two O(N) kernels, the predictor, the corrector and the step constants are hermite_kernels.h's templates
// at T = double; the 6th order's two O(N) kernels, row bodies and step constants are hermite6_f64_kernels.h's (this unit
// launches all four at the row stride 1 and with the packed store; direct_hermite_shard_f64.hip launches the same four
// on a rank's send buffer). The step constants are doubles formed from the double dt, never rounded to fp32; every
// product and sum of the O(N) kernels rounds on its own (the build has -ffp-contract=off). The finishing kernels of the
// diagnostics add their slabs with the same slab_order_sum.
// rsqrt_f64, the pair functors, the bodies of the finishing kernels, walk_f64, the kernels' prologue (Group64,
// wave_chunks_upper) and plan_f64 live in hermite_f64_kernels.h, shared with every other float64 unit (the block-timestep,
// the sharded, the batched, the leapfrog and the backward ones).
// Resources (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage). force_f64_kernel<Order4>: 89 VGPRs,
// 32 KiB of LDS, 5 waves per SIMD: five workgroups per CU, what the LDS allows. <Order6>: 164 VGPRs, 0 AGPRs, 48 KiB of
// LDS, 3 waves per SIMD: three workgroups per CU by the LDS and by the registers alike. hermite_predict_kernel<double>: 24
// VGPRs; hermite_correct_kernel<double>: 42; hermite6_predict_kernel<1>: 40; hermite6_finish_kernel<>: 52; potential_f64_kernel:
// 56 and energy_f64_kernel: 30, 16 KiB of LDS each. No SGPR or VGPR spills and no scratch anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_kernels.h"
#include "hermite6_f64_kernels.h"
#include "hermite_f64_kernels.h"
#include "hermite_kernels.h"
#include "hermite_orders_f64.h"

namespace {

// The sums of an order (acceleration + jerk, at the 6th order + snap: Pair::kOut per body) of all n bodies under all n
// bodies: grid = (groups of 64 targets, slabs), the n_chunks source chunks spread over all slabs x 4 waves to within one
// (cpw_q each, the first cpw_r waves one more). accd: the 6th order's third array, not read at the 4th.
// out: double[slab][kOut][n].
template <class Order>
__global__ __launch_bounds__(64 * kWaves) void force_f64_kernel(const d4* __restrict__ posd, const d4* __restrict__ veld,
                                                                const d4* __restrict__ accd, int n, int cpw_q, int cpw_r,
                                                                double eps2, int all_masked, double* __restrict__ out) {
  using Pair = typename Order::Pair;
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads_n<Order::kArr>()];
  const Group64<unsigned> g(blockIdx.x, blockIdx.y, n);
  const ChunkRange c = wave_chunks(g.jw(), cpw_q, cpw_r);
  Pair pr = Order::make(posd, veld, accd, g.row(), g.i, eps2, n);
  walk_f64(pr, posd, veld, c.begin, c.end, all_masked != 0, blockIdx.x, lds, g.dst<Pair>(out), (size_t)n, g.n_valid(),
           nullptr, Order::kArr == 3 ? accd : nullptr);
}

// The same geometry for the potential. out: double[slab][n].
__global__ __launch_bounds__(64 * kWaves) void potential_f64_kernel(const d4* __restrict__ posd, int n, int cpw_q,
                                                                    int cpw_r, double eps2, int all_masked,
                                                                    double* __restrict__ out) {
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads<false>()];
  const Group64<unsigned> g(blockIdx.x, blockIdx.y, n);
  const ChunkRange c = wave_chunks(g.jw(), cpw_q, cpw_r);
  PotentialPair pr(posd[g.row()], eps2, g.i, n);
  walk_f64(pr, posd, posd, c.begin, c.end, all_masked != 0, blockIdx.x, lds, g.dst<PotentialPair>(out), (size_t)n,
           g.n_valid());
}

// The pair energies of the upper triangle: group g needs the chunks [g, n_chunks) only (chunk g is the group's own rows),
// split over the slabs x 4 waves of the group by the same balanced split. out: double[slab][n].
__global__ __launch_bounds__(64 * kWaves) void energy_f64_kernel(const d4* __restrict__ posd, int n, int n_chunks,
                                                                 double soft, double* __restrict__ out) {
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads<false>()];
  const Group64<unsigned> g(blockIdx.x, blockIdx.y, n);
  const ChunkRange c = wave_chunks_upper<unsigned>(g.jw(), n_chunks, blockIdx.x, gridDim.y);
  EnergyPair pr(posd[g.row()], soft, g.i, n);
  walk_f64(pr, posd, posd, c.begin + blockIdx.x, c.end + blockIdx.x, true, blockIdx.x, lds, g.dst<EnergyPair>(out),
           (size_t)n, g.n_valid());
}

// phi[i] = potential_finish_f64 of body i
__global__ __launch_bounds__(256) void potential_finish_f64_kernel(const double* __restrict__ slabs, int n_slabs, int n,
                                                                   double g, double* __restrict__ phi) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  phi[i] = potential_finish_f64(slabs, n_slabs, n, i, g);
}

// {U, K} of the one system: one workgroup
__global__ __launch_bounds__(kSumThreads) void energy_finish_f64_kernel(const double* __restrict__ slabs, int n_slabs,
                                                                        int n, const d4* __restrict__ posd,
                                                                        const double* __restrict__ vel, double g,
                                                                        double* __restrict__ out_uk) {
  __shared__ double red[2][kSumWaves];
  energy_finish_f64(slabs, n_slabs, n, posd, vel, g, out_uk, red);
}

__global__ __launch_bounds__(kInvThreads) void invariants_state_f64_kernel(const double* __restrict__ pos,
                                                                           const double* __restrict__ vel,
                                                                           const double* __restrict__ mass,
                                                                           const double* __restrict__ phi, int n,
                                                                           double* __restrict__ row) {
  __shared__ double red[kInvSums][kInvWaves];
  invariants_body(F64State{pos, vel, mass}, phi, n, row, red);
}

constexpr int kSumRows = HermiteFmt<double>::kSumRows;      // bodies per workgroup of the 4th-order corrector launch

// ---- the host bodies of the entries. The geometry is the same for both orders: plan_f64(n).

// the partial sums double[slabs][kOut][n] of an order
template <class Order>
size_t slab_bytes(int slabs, int n) { return (size_t)slabs * Order::Pair::kOut * n * sizeof(double); }

template <class Order>
size_t step_workspace_bytes(int n) { return n <= 0 ? 0 : slab_bytes<Order>(plan_f64(n).slabs, n); }

inline bool bad_workspace(const void* ws, size_t have, size_t need) { return !ws || misaligned8(ws) || have < need; }

// the unscaled partial sums of every body into double[slabs][kOut][n]
template <class Order>
int launch_force(const double* posd, const double* veld, const double* accd, int n, double eps2, double* out,
                 const F64Plan& p, int slabs, hipStream_t st) {
  const ChunkSplit c = chunk_split(p.n_chunks, slabs);
  force_f64_kernel<Order><<<dim3(p.groups, slabs), 64 * kWaves, 0, st>>>(
      reinterpret_cast<const d4*>(posd), reinterpret_cast<const d4*>(veld), reinterpret_cast<const d4*>(accd), n, c.q,
      c.r, eps2, eps2 < kEps2MaskedF64 ? 1 : 0, out);
  return launch_status();
}

// The force on its own, at the plan's slab count or a given one: the partial sums, then finish(part, n_slabs, stream),
// the entry's finishing launch. out_ok: what the entry found of its own pointer list.
template <class Order, class Finish>
int shared_force(const double* posd, const double* veld, const double* accd, int n, double softening_sq, bool out_ok,
                 void* workspace, size_t workspace_bytes, int slabs, nbd_stream_t stream, Finish finish) {
  if (n < 0 || slabs < 0 || slabs > kMaxSlabs) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (!out_ok || bad_rows<Order>(posd, veld, accd)) return NBD_E_BADARG;
  const F64Plan p = plan_f64(n);
  if (slabs == 0) slabs = p.slabs;
  if (bad_workspace(workspace, workspace_bytes, slab_bytes<Order>(slabs, n))) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  double* part = static_cast<double*>(workspace);
  const int rc = launch_force<Order>(posd, veld, accd, n, softening_sq, part, p, slabs, st);
  if (rc) return rc;
  finish(part, slabs, st);
  return launch_status();
}

// A whole step: everything the three stages refuse, before the first launch; then predict(stream), the entry's
// predictor launch, and the force at the plan's slab count with the entry's corrector as its finish.
template <class Order, class Predict, class Finish>
int shared_step(int n, bool state_ok, const double* posd, const double* veld, const double* accd, double softening_sq,
                void* workspace, size_t workspace_bytes, nbd_stream_t stream, Predict predict, Finish finish) {
  if (n < 0) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (!state_ok || bad_rows<Order>(posd, veld, accd)) return NBD_E_BADARG;
  if (bad_workspace(workspace, workspace_bytes, step_workspace_bytes<Order>(n))) return NBD_E_WORKSPACE;
  predict((hipStream_t)stream);
  const int rc = launch_status();
  if (rc) return rc;
  return shared_force<Order>(posd, veld, accd, n, softening_sq, true, workspace, workspace_bytes, 0, stream, finish);
}

}  // namespace

extern "C" {

size_t nbd_hermite_f64_workspace_bytes(int n) { return step_workspace_bytes<Order4>(n); }

size_t nbd_hermite6_f64_workspace_bytes(int n) { return step_workspace_bytes<Order6>(n); }

int nbd_hermite_f64_plan(int n, int* groups, int* slabs, int* chunks_per_wave) {
  if (n <= 0) return NBD_E_BADARG;
  const F64Plan p = plan_f64(n);
  if (groups) *groups = p.groups;
  if (slabs) *slabs = p.slabs;
  if (chunks_per_wave) *chunks_per_wave = ceil_div(p.n_chunks, p.slabs * kWaves);
  return 0;
}

int nbd_hermite_f64_pack(const double* pos, const double* vel, const double* acc, const double* jerk, const double* mass,
                         int n, double dt, double* posd, double* veld, nbd_stream_t stream) {
  if (n < 0 || (n > 0 && (!pos || !vel || !mass || !posd || !veld)) || (!acc != !jerk)) return NBD_E_BADARG;
  if (misaligned32(posd) || misaligned32(veld)) return NBD_E_BADARG;
  if (n == 0) return 0;
  const int n_pad = nbd_posm_padded_len(n);
  hermite_predict_kernel<double><<<ceil_div(n_pad, 256), 256, 0, (hipStream_t)stream>>>(
      pos, vel, acc, jerk, mass, n, n_pad, hermite_step_constants<double>(dt), reinterpret_cast<d4*>(posd),
      reinterpret_cast<d4*>(veld));
  return launch_status();
}

int nbd_hermite6_f64_pack(const double* pos, const double* vel, const double* acc, const double* jerk,
                          const double* snap, const double* crackle, const double* mass, int n, double dt, double* posd,
                          double* veld, double* accd, nbd_stream_t stream) {
  if (n < 0 || (n > 0 && (!pos || !vel || !mass || !posd || !veld || !accd))) return NBD_E_BADARG;
  if ((!jerk != !snap) || (!jerk != !crackle) || (jerk && !acc)) return NBD_E_BADARG;
  if (misaligned32(posd) || misaligned32(veld) || misaligned32(accd)) return NBD_E_BADARG;
  if (n == 0) return 0;
  const int n_pad = nbd_posm_padded_len(n);
  hermite6_predict_kernel<><<<ceil_div(n_pad, 256), 256, 0, (hipStream_t)stream>>>(
      pos, vel, acc, jerk, snap, crackle, mass, n, n_pad, hermite6_step_constants(dt), reinterpret_cast<d4*>(posd),
      reinterpret_cast<d4*>(veld), reinterpret_cast<d4*>(accd));
  return launch_status();
}

int nbd_accel_jerk_f64(const double* posd, const double* veld, int n, double softening_sq, double g_const,
                       double* acc_out, double* jerk_out, void* workspace, size_t workspace_bytes, int slabs,
                       nbd_stream_t stream) {
  return shared_force<Order4>(
      posd, veld, nullptr, n, softening_sq, acc_out && jerk_out, workspace, workspace_bytes, slabs, stream,
      [=](const double* part, int n_slabs, hipStream_t st) {
        hermite_correct_kernel<double><<<ceil_div(n, kSumRows), 256, 0, st>>>(
            part, n_slabs, n, g_const, hermite_step_constants<double>(0.0), nullptr, nullptr, nullptr, nullptr, acc_out,
            jerk_out, nullptr, nullptr);
      });
}

int nbd_accel_jerk_snap_f64(const double* posd, const double* veld, const double* accd, int n, double softening_sq,
                            double g_const, double* acc_out, double* jerk_out, double* snap_out, void* workspace,
                            size_t workspace_bytes, int slabs, nbd_stream_t stream) {
  return shared_force<Order6>(
      posd, veld, accd, n, softening_sq, acc_out && jerk_out && snap_out, workspace, workspace_bytes, slabs, stream,
      [=](const double* part, int n_slabs, hipStream_t st) {
        hermite6_finish_kernel<><<<ceil_div(n, 256), 256, 0, st>>>(
            part, n_slabs, n, g_const, hermite6_step_constants(0.0), nullptr, nullptr, nullptr, nullptr, nullptr,
            acc_out, jerk_out, snap_out, nullptr, nullptr, nullptr);
      });
}

int nbd_hermite_step_f64(double* pos, double* vel, const double* acc_in, const double* jerk_in, double* acc_out,
                         double* jerk_out, const double* mass, int n, double dt, double softening_sq, double g_const,
                         double* posd, double* veld, void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  const bool state_ok = pos && vel && acc_in && jerk_in && acc_out && jerk_out && mass;
  const HermiteStep<double> h = hermite_step_constants<double>(dt);
  const int n_pad = nbd_posm_padded_len(n);
  d4 *pd = reinterpret_cast<d4*>(posd), *vd = reinterpret_cast<d4*>(veld);
  return shared_step<Order4>(
      n, state_ok, posd, veld, nullptr, softening_sq, workspace, workspace_bytes, stream,
      [=](hipStream_t st) {
        hermite_predict_kernel<double><<<ceil_div(n_pad, 256), 256, 0, st>>>(pos, vel, acc_in, jerk_in, mass, n, n_pad, h,
                                                                             pd, vd);
      },
      [=](const double* part, int n_slabs, hipStream_t st) {
        hermite_correct_kernel<double><<<ceil_div(n, kSumRows), 256, 0, st>>>(
            part, n_slabs, n, g_const, h, pos, vel, acc_in, jerk_in, acc_out, jerk_out, mass, pd);
      });
}

int nbd_hermite6_step_f64(double* pos, double* vel, const double* acc_in, const double* jerk_in, const double* snap_in,
                          const double* crackle_in, double* acc_out, double* jerk_out, double* snap_out,
                          double* crackle_out, const double* mass, int n, double dt, double softening_sq, double g_const,
                          double* posd, double* veld, double* accd, void* workspace, size_t workspace_bytes,
                          nbd_stream_t stream) {
  const bool state_ok = pos && vel && acc_in && jerk_in && snap_in && crackle_in && acc_out && jerk_out && snap_out &&
                        crackle_out && mass;
  const Hermite6Step h = hermite6_step_constants(dt);
  const int n_pad = nbd_posm_padded_len(n);
  d4 *pd = reinterpret_cast<d4*>(posd), *vd = reinterpret_cast<d4*>(veld), *ad = reinterpret_cast<d4*>(accd);
  return shared_step<Order6>(
      n, state_ok, posd, veld, accd, softening_sq, workspace, workspace_bytes, stream,
      [=](hipStream_t st) {
        hermite6_predict_kernel<><<<ceil_div(n_pad, 256), 256, 0, st>>>(pos, vel, acc_in, jerk_in, snap_in, crackle_in,
                                                                      mass, n, n_pad, h, pd, vd, ad);
      },
      [=](const double* part, int n_slabs, hipStream_t st) {
        hermite6_finish_kernel<><<<ceil_div(n, 256), 256, 0, st>>>(part, n_slabs, n, g_const, h, pos, vel, acc_in, jerk_in,
                                                                 snap_in, acc_out, jerk_out, snap_out, crackle_out, mass,
                                                                 pd);
      });
}

int nbd_energy_f64(const double* posd, const double* vel, int n, double softening, double g_const, double* out_uk,
                   void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  if (n < 0 || !out_uk || misaligned8(out_uk)) return NBD_E_BADARG;
  if (n > 0 && (!posd || !vel || misaligned32(posd))) return NBD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const d4* pd = reinterpret_cast<const d4*>(posd);
  double* part = static_cast<double*>(workspace);
  int slabs = 0;
  if (n > 0) {
    const F64Plan p = plan_f64(n);
    slabs = p.slabs;
    if (!workspace || misaligned8(workspace) || workspace_bytes < (size_t)slabs * n * sizeof(double))
      return NBD_E_WORKSPACE;
    energy_f64_kernel<<<dim3(p.groups, slabs), 64 * kWaves, 0, st>>>(pd, n, p.n_chunks, softening, part);
    const int rc = launch_status();
    if (rc) return rc;
  }
  energy_finish_f64_kernel<<<1, kSumThreads, 0, st>>>(part, slabs, n, pd, vel, g_const, out_uk);
  return launch_status();
}

int nbd_potential_f64(const double* posd, int n, double softening_sq, double g_const, double* phi_out, void* workspace,
                      size_t workspace_bytes, nbd_stream_t stream) {
  if (n < 0) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (!posd || misaligned32(posd) || !phi_out || misaligned8(phi_out)) return NBD_E_BADARG;
  const F64Plan p = plan_f64(n);
  if (!workspace || misaligned8(workspace) || workspace_bytes < (size_t)p.slabs * n * sizeof(double))
    return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  double* part = static_cast<double*>(workspace);
  const ChunkSplit c = chunk_split(p.n_chunks, p.slabs);
  potential_f64_kernel<<<dim3(p.groups, p.slabs), 64 * kWaves, 0, st>>>(
      reinterpret_cast<const d4*>(posd), n, c.q, c.r, softening_sq, softening_sq < kEps2MaskedF64 ? 1 : 0, part);
  const int rc = launch_status();
  if (rc) return rc;
  potential_finish_f64_kernel<<<ceil_div(n, 256), 256, 0, st>>>(part, p.slabs, n, g_const, phi_out);
  return launch_status();
}

int nbd_invariants_state_f64(const double* pos, const double* vel, const double* mass, const double* phi, int n,
                             double* out_row, nbd_stream_t stream) {
  if (n < 0 || !out_row || misaligned8(out_row)) return NBD_E_BADARG;
  if (n > 0 && (!pos || !vel || !mass || !phi || misaligned8(phi))) return NBD_E_BADARG;
  invariants_state_f64_kernel<<<1, kInvThreads, 0, (hipStream_t)stream>>>(pos, vel, mass, phi, n, out_row);
  return launch_status();
}

}  // extern "C"
