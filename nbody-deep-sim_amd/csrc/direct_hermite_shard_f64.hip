// direct_hermite_shard_f64.hip -- the double-precision form of direct_hermite_shard.hip's range-sharded 4th-order Hermite
// step, in the number format of direct_hermite_f64.hip: one rank of a torch.distributed group owns the bodies
// [lo, lo + n_local) of n_total and needs every other rank's PREDICTED position, mass and velocity per step. C-ABI: the
// nbd_hermite_shard_*_f64 entries of include/nbd.h; Python: galaxify.simulation.HermiteSimulator(dtype=torch.float64,
// process_group=...).
//
// The exchanged row is 8 doubles, {x_p, y_p, z_p, m, vx_p, vy_p, vz_p, 0}, 64 bytes: ONE all-gather per step carries both
// halves, and walk_f64 (hermite_f64_kernels.h, RQ = 4) fetches a chunk's position quads and velocity quads by LDS-DMA at
// a four-quad row stride into the LDS image the un-sharded kernels use, so the gathered array is read as it lands (no
// de-interleave launch) and the pair loops are the un-sharded ones. A rank's step is four launches, as in fp32:
//   predict : hermite_predict_row<double> of the own bodies -> the send buffer, zero rows behind n_local
//   local   : a, j partial sums of the own bodies under the own bodies (reads the send buffer only: runs while the
//             gather is in flight); accel_jerk_f64_kernel's geometry on n_local sources
//   remote  : the same targets under all bodies of the gathered array except [lo, lo + n_local): whole source chunks
//             inside the range are hopped over, the <= 2 chunks that straddle an end take the masked loop with the range
//             mask (excluded_view, direct_kernels.h)
//   finish  : slab_order_sum over the local slabs, then the remote ones, times G, and hermite_correct_row<double> of the
//             own rows (or a1, j1 only: the force on its own)
// Every rounded operation is hermite_f64_kernels.h's or hermite_kernels.h's: a rank that owns every body computes
// nbd_accel_jerk_f64's bits. No atomics, no memsets, no host syncs: deterministic with a workspace that may hold anything.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_kernels.h"
#include "hermite_f64_kernels.h"
#include "hermite_kernels.h"

namespace {

constexpr int kShardRowQuads = 2 * kRowQuads;      // 16-byte quads per exchanged row: {x_p, m}, {v_p, 0}

// Acceleration + jerk partial sums of the targets tgt[0 .. n_tgt) (64-byte rows; global index tgt_off + row) under the
// sources of the view sv on src (64-byte rows): accel_jerk_f64_kernel's geometry -- grid = (target groups of 64, slabs),
// the view's logical chunks spread over all slabs x 4 waves to within one. RANGE: sv leaves [ex_lo, ex_hi) out (the
// remote block: no target has a source index of its own there); else sv is the full view of src (the local block,
// src == tgt: group g's own indices are chunk g). out: double[slab][6][n_tgt].
template <bool RANGE>
__global__ __launch_bounds__(64 * kWaves) void shard_accel_jerk_f64_kernel(const d4* __restrict__ src, const SrcView sv,
                                                                           const d4* __restrict__ tgt, int n_tgt,
                                                                           int tgt_off, double eps2, int all_masked,
                                                                           double* __restrict__ out) {
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads<true>()];
  const Group64<unsigned> g(blockIdx.x, blockIdx.y, n_tgt);
  const ChunkRange c = wave_chunks(g.jw(), sv.cpw_q, sv.cpw_r);
  const size_t row = (size_t)g.row() * 2;
  AccelJerkPair pr(tgt[row], tgt[row + 1], eps2, tgt_off + g.i, sv.n_src);
  walk_f64<AccelJerkPair, kShardRowQuads, RANGE>(pr, src, src + 1, c.begin, c.end, all_masked != 0,
                                                 RANGE ? -1 : (int)blockIdx.x, lds, g.dst<AccelJerkPair>(out),
                                                 (size_t)n_tgt, g.n_valid(), &sv);
}

// rows [0, rows) of the send buffer: {x_p, m}, {v_p, 0} of the rank's bodies, zeros behind n. acc == nullptr: plain pack.
__global__ __launch_bounds__(256) void shard_predict_f64_kernel(const double* __restrict__ pos,
                                                                const double* __restrict__ vel,
                                                                const double* __restrict__ acc,
                                                                const double* __restrict__ jerk,
                                                                const double* __restrict__ mass, int n, int rows,
                                                                HermiteStep<double> h, d4* __restrict__ send) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)rows) return;
  d4 pm = HermiteFmt<double>::zero(), vp = HermiteFmt<double>::zero();
  if (i < (size_t)n) {
    const PosVel3<double> p = hermite_predict_row(pos, vel, acc, jerk, i, h.dt, h.dt2_half, h.dt3_sixth, acc != nullptr);
    pm = hermite_row(p.x, mass[i]);
    vp = hermite_row(p.v, 0.0);
  }
  send[2 * i] = pm;
  send[2 * i + 1] = vp;
}

// One thread per own body: a1, j1 = G * (the body's row of every slab in slab order, local ones first). pos == nullptr:
// write a1, j1 only. Else hermite_correct_row (acc_in / jerk_in may alias acc_out / jerk_out: each element is read before
// it is written, by the same thread).
__global__ __launch_bounds__(256) void shard_finish_f64_kernel(const double* __restrict__ slabs, int n_slabs, int n,
                                                               double g, HermiteStep<double> h, double* pos, double* vel,
                                                               const double* acc_in, const double* jerk_in,
                                                               double* acc_out, double* jerk_out) {
  const size_t i = hermite_sum_row<double>();
  double a1[3], j1[3];
  if (!hermite_slab_sum(slabs, n_slabs, n, i, i < (size_t)n, g, a1, j1)) return;
  if (pos) hermite_correct_row(pos, vel, acc_in, jerk_in, i, a1, j1, h.dt_half, h.dt2_twelfth);
  hermite_store_force(acc_out, jerk_out, i, a1, j1);
}

// The geometry of a rank's two force launches: HShardPlanF64, plan_hshard_f64 and slab_arg_ok of hermite_f64_kernels.h
// (shared with direct_hermite6_shard_f64.hip).
size_t slab_doubles(int n_local) { return (size_t)AccelJerkPair::kOut * n_local; }

}  // namespace

extern "C" {

int nbd_hermite_shard_f64_plan(int n_total, int lo, int n_local, int* slabs_local, int* chunks_per_wave_local,
                               int* slabs_remote, int* chunks_per_wave_remote) {
  if (!shard_args_ok(n_total, lo, n_local) || n_local == 0) return NBD_E_BADARG;
  const HShardPlanF64 p = plan_hshard_f64(n_total, lo, n_local, 0, 0);
  if (slabs_local) *slabs_local = p.slabs_local;
  if (chunks_per_wave_local) *chunks_per_wave_local = ceil_div(p.chunks_local, p.slabs_local * kWaves);
  if (slabs_remote) *slabs_remote = p.slabs_remote;
  if (chunks_per_wave_remote)
    *chunks_per_wave_remote = p.slabs_remote ? ceil_div(p.chunks_remote, p.slabs_remote * kWaves) : 0;
  return 0;
}

size_t nbd_hermite_shard_f64_workspace_bytes(int n_total, int lo, int n_local, int slabs_local, int slabs_remote) {
  if (!shard_args_ok(n_total, lo, n_local) || n_local == 0 || !slab_arg_ok(slabs_local) || !slab_arg_ok(slabs_remote))
    return 0;
  const HShardPlanF64 p = plan_hshard_f64(n_total, lo, n_local, slabs_local, slabs_remote);
  return (size_t)(p.slabs_local + p.slabs_remote) * slab_doubles(n_local) * sizeof(double);
}

int nbd_hermite_shard_predict_f64(const double* pos, const double* vel, const double* acc, const double* jerk,
                                  const double* mass, int n_local, double dt, double* send, int send_rows,
                                  nbd_stream_t stream) {
  if (n_local < 0 || send_rows < nbd_posm_padded_len(n_local) || (!acc != !jerk)) return NBD_E_BADARG;
  if (send_rows == 0) return 0;
  if (!send || misaligned32(send) || (n_local > 0 && (!pos || !vel || !mass))) return NBD_E_BADARG;
  shard_predict_f64_kernel<<<ceil_div(send_rows, 256), 256, 0, (hipStream_t)stream>>>(
      pos, vel, acc, jerk, mass, n_local, send_rows, hermite_step_constants<double>(dt), reinterpret_cast<d4*>(send));
  return launch_status();
}

int nbd_hermite_shard_force_local_f64(const double* send, int n_local, double softening_sq, void* workspace,
                                      size_t workspace_bytes, int n_total, int lo, int slabs, nbd_stream_t stream) {
  if (!shard_args_ok(n_total, lo, n_local) || !slab_arg_ok(slabs)) return NBD_E_BADARG;
  if (n_local == 0) return 0;
  if (!send || misaligned32(send)) return NBD_E_BADARG;
  const HShardPlanF64 p = plan_hshard_f64(n_total, lo, n_local, slabs, 0);
  // what this launch writes: the local slabs (the remote call checks the whole buffer)
  if (!workspace || misaligned8(workspace) ||
      workspace_bytes < (size_t)p.slabs_local * slab_doubles(n_local) * sizeof(double))
    return NBD_E_WORKSPACE;
  const SrcView sv = full_view(n_local, p.chunks_local, p.slabs_local);
  const d4* s = reinterpret_cast<const d4*>(send);
  // the rank's own block: targets and sources are the same rows, the diagonal is at j == i (offset 0)
  shard_accel_jerk_f64_kernel<false><<<dim3(p.groups, p.slabs_local), 64 * kWaves, 0, (hipStream_t)stream>>>(
      s, sv, s, n_local, 0, softening_sq, softening_sq < kEps2MaskedF64 ? 1 : 0, static_cast<double*>(workspace));
  return launch_status();
}

int nbd_hermite_shard_force_remote_f64(const double* all, int n_total, const double* send, int n_local, int lo,
                                       double softening_sq, double g_const, double* pos, double* vel,
                                       const double* acc_in, const double* jerk_in, double* acc_out, double* jerk_out,
                                       double dt, void* workspace, size_t workspace_bytes, int slabs_local,
                                       int slabs_remote, nbd_stream_t stream) {
  if (!shard_args_ok(n_total, lo, n_local) || !slab_arg_ok(slabs_local) || !slab_arg_ok(slabs_remote))
    return NBD_E_BADARG;
  if (n_local == 0) return 0;
  if (!all || !send || !acc_out || !jerk_out || misaligned32(all) || misaligned32(send)) return NBD_E_BADARG;
  if (pos && (!vel || !acc_in || !jerk_in)) return NBD_E_BADARG;
  if (!workspace || misaligned8(workspace) ||
      workspace_bytes < nbd_hermite_shard_f64_workspace_bytes(n_total, lo, n_local, slabs_local, slabs_remote))
    return NBD_E_WORKSPACE;
  const HShardPlanF64 p = plan_hshard_f64(n_total, lo, n_local, slabs_local, slabs_remote);
  double* slabs = static_cast<double*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  if (p.slabs_remote > 0) {
    // the diagonal never occurs here (every j in [lo, lo + n_local) is left out); lo keeps the index meaning
    shard_accel_jerk_f64_kernel<true><<<dim3(p.groups, p.slabs_remote), 64 * kWaves, 0, st>>>(
        reinterpret_cast<const d4*>(all), p.remote, reinterpret_cast<const d4*>(send), n_local, lo, softening_sq,
        softening_sq < kEps2MaskedF64 ? 1 : 0, slabs + (size_t)p.slabs_local * slab_doubles(n_local));
    const int rc = launch_status();
    if (rc) return rc;
  }
  shard_finish_f64_kernel<<<ceil_div(n_local, HermiteFmt<double>::kSumRows), 256, 0, st>>>(
      slabs, p.slabs_local + p.slabs_remote, n_local, g_const, hermite_step_constants<double>(dt), pos, vel, acc_in,
      jerk_in, acc_out, jerk_out);
  return launch_status();
}

}  // extern "C"
