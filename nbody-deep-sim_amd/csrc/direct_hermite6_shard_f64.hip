// direct_hermite6_shard_f64.hip -- the range-sharded form of direct_hermite6_f64.hip's 6th-order Hermite step, modelled on
// direct_hermite_shard_f64.hip: one rank of a torch.distributed group owns the bodies [lo, lo + n_local) of n_total and
// needs every other rank's PREDICTED position, mass, velocity and acceleration per step. C-ABI: the nbd_hermite6_shard_*
// entries of include/nbd.h; Python: galaxify.simulation.Hermite6Simulator(process_group=...).
//
// The exchanged row is 12 doubles, {x_p, y_p, z_p, m | vx_p, vy_p, vz_p, 0 | ax_p, ay_p, az_p, 0}, 96 bytes: ONE
// all-gather per step carries all three source arrays, and walk_f64 (hermite_f64_kernels.h, RQ = 6) fetches a chunk's
// position, velocity and acceleration quads by LDS-DMA at a six-quad row stride into the [pos | vel | third][128] LDS
// image the un-sharded kernel uses, so the gathered array is read as it lands and the pair loops are the un-sharded ones.
// A rank's step is four launches:
//   predict : hermite6_predict_row of the own bodies -> the send buffer, zero rows behind n_local
//   local   : a, j, s partial sums of the own bodies under the own bodies (reads the send buffer only: runs while the
//             gather is in flight); accel_jerk_snap_f64_kernel's geometry on n_local sources
//   remote  : the same targets under all bodies of the gathered array except [lo, lo + n_local): whole source chunks
//             inside the range are hopped over, the <= 2 chunks that straddle an end take the masked loop with the range
//             mask (excluded_view, direct_kernels.h)
//   finish  : slab_order_sum<9> over the local slabs, then the remote ones, times G, and hermite6_finish_row of the own
//             rows: the corrector and c1 (or a1, j1, s1 only: the force on its own)
// Every rounded operation is hermite6_f64_kernels.h's or hermite_f64_kernels.h's: a rank that owns every body computes
// nbd_accel_jerk_snap_f64's bits, and a and j of any rank are nbd_hermite_shard_force_*_f64's at the same slab counts. No
// atomics, no memsets, no host syncs: deterministic with a workspace that may hold anything.
// The LDS-DMA fetch reads whole 64-row chunks: the send buffer and the gathered array are allocated to
// nbd_posm_padded_len(rows) rows with zero rows behind the data, and the view's chunk counts come from n_total.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_kernels.h"
#include "hermite6_f64_kernels.h"
#include "hermite_f64_kernels.h"
#include "hermite_kernels.h"

namespace {

constexpr int kShard6RowQuads = 3 * kRowQuads;     // 16-byte quads per exchanged row: {x_p, m}, {v_p, 0}, {a_p, 0}
constexpr int kShard6RowD4 = 3;                    // ... and d4 elements

// Acceleration + jerk + snap partial sums of the targets tgt[0 .. n_tgt) (96-byte rows; global index tgt_off + row) under
// the sources of the view sv on src (96-byte rows): accel_jerk_snap_f64_kernel's geometry -- grid = (target groups of 64,
// slabs), the view's logical chunks spread over all slabs x 4 waves to within one. RANGE: sv leaves [ex_lo, ex_hi) out
// (the remote block: no target has a source index of its own there); else sv is the full view of src (the local block,
// src == tgt: group g's own indices are chunk g). out: double[slab][9][n_tgt].
template <bool RANGE>
__global__ __launch_bounds__(64 * kWaves) void shard_accel_jerk_snap_f64_kernel(const d4* __restrict__ src,
                                                                                const SrcView sv,
                                                                                const d4* __restrict__ tgt, int n_tgt,
                                                                                int tgt_off, double eps2, int all_masked,
                                                                                double* __restrict__ out) {
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads_n<3>()];
  const Group64<unsigned> g(blockIdx.x, blockIdx.y, n_tgt);
  const ChunkRange c = wave_chunks(g.jw(), sv.cpw_q, sv.cpw_r);
  const size_t row = (size_t)g.row() * kShard6RowD4;
  AccelJerkSnapPair pr(tgt[row], tgt[row + 1], tgt[row + 2], eps2, tgt_off + g.i, sv.n_src);
  walk_f64<AccelJerkSnapPair, kShard6RowQuads, RANGE>(pr, src, src + 1, c.begin, c.end, all_masked != 0,
                                                      RANGE ? -1 : (int)blockIdx.x, lds,
                                                      g.dst<AccelJerkSnapPair>(out), (size_t)n_tgt, g.n_valid(), &sv,
                                                      src + 2);
}

// rows [0, rows) of the send buffer: {x_p, m}, {v_p, 0}, {a_p, 0} of the rank's bodies, zeros behind n. jerk == nullptr
// (then snap and crackle are too): plain pack of (pos, vel, acc); acc == nullptr as well: a zero third quad pair.
__global__ __launch_bounds__(256) void shard6_predict_f64_kernel(const double* __restrict__ pos,
                                                                 const double* __restrict__ vel,
                                                                 const double* __restrict__ acc,
                                                                 const double* __restrict__ jerk,
                                                                 const double* __restrict__ snap,
                                                                 const double* __restrict__ crackle,
                                                                 const double* __restrict__ mass, int n, int rows,
                                                                 Hermite6Step h, d4* __restrict__ send) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)rows) return;
  d4 pm = {0.0, 0.0, 0.0, 0.0}, vp = pm, ap = pm;
  if (i < (size_t)n) hermite6_predict_row(pos, vel, acc, jerk, snap, crackle, mass, i, h, pm, vp, ap);
  send[kShard6RowD4 * i] = pm;
  send[kShard6RowD4 * i + 1] = vp;
  send[kShard6RowD4 * i + 2] = ap;
}

// One thread per own body: a1, j1, s1 = G * (the body's row of every slab in slab order, local ones first). pos ==
// nullptr: write them only. Else hermite6_finish_row's corrector and c1 (the inputs may alias the outputs: each element is
// read before it is written, by the same thread).
__global__ __launch_bounds__(256) void shard6_finish_f64_kernel(const double* __restrict__ slabs, int n_slabs, int n,
                                                                double g, Hermite6Step h, double* pos, double* vel,
                                                                const double* acc_in, const double* jerk_in,
                                                                const double* snap_in, double* acc_out,
                                                                double* jerk_out, double* snap_out,
                                                                double* crackle_out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n) return;
  hermite6_finish_row<false>(slabs, n_slabs, (size_t)n, i, i, g, h, pos, vel, acc_in, jerk_in, snap_in, acc_out,
                             jerk_out, snap_out, crackle_out, nullptr, nullptr, i);
}

size_t slab6_doubles(int n_local) { return (size_t)AccelJerkSnapPair::kOut * n_local; }

}  // namespace

extern "C" {

int nbd_hermite6_shard_f64_plan(int n_total, int lo, int n_local, int* slabs_local, int* chunks_per_wave_local,
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

size_t nbd_hermite6_shard_f64_workspace_bytes(int n_total, int lo, int n_local, int slabs_local, int slabs_remote) {
  if (!shard_args_ok(n_total, lo, n_local) || n_local == 0 || !slab_arg_ok(slabs_local) || !slab_arg_ok(slabs_remote))
    return 0;
  const HShardPlanF64 p = plan_hshard_f64(n_total, lo, n_local, slabs_local, slabs_remote);
  return (size_t)(p.slabs_local + p.slabs_remote) * slab6_doubles(n_local) * sizeof(double);
}

int nbd_hermite6_shard_predict_f64(const double* pos, const double* vel, const double* acc, const double* jerk,
                                   const double* snap, const double* crackle, const double* mass, int n_local, double dt,
                                   double* send, int send_rows, nbd_stream_t stream) {
  if (n_local < 0 || send_rows < nbd_posm_padded_len(n_local)) return NBD_E_BADARG;
  if ((!jerk != !snap) || (!jerk != !crackle) || (jerk && !acc)) return NBD_E_BADARG;
  if (send_rows == 0) return 0;
  if (!send || misaligned32(send) || (n_local > 0 && (!pos || !vel || !mass))) return NBD_E_BADARG;
  shard6_predict_f64_kernel<<<ceil_div(send_rows, 256), 256, 0, (hipStream_t)stream>>>(
      pos, vel, acc, jerk, snap, crackle, mass, n_local, send_rows, hermite6_step_constants(dt),
      reinterpret_cast<d4*>(send));
  return launch_status();
}

int nbd_hermite6_shard_force_local_f64(const double* send, int n_local, double softening_sq, void* workspace,
                                       size_t workspace_bytes, int n_total, int lo, int slabs, nbd_stream_t stream) {
  if (!shard_args_ok(n_total, lo, n_local) || !slab_arg_ok(slabs)) return NBD_E_BADARG;
  if (n_local == 0) return 0;
  if (!send || misaligned32(send)) return NBD_E_BADARG;
  const HShardPlanF64 p = plan_hshard_f64(n_total, lo, n_local, slabs, 0);
  // what this launch writes: the local slabs (the remote call checks the whole buffer)
  if (!workspace || misaligned8(workspace) ||
      workspace_bytes < (size_t)p.slabs_local * slab6_doubles(n_local) * sizeof(double))
    return NBD_E_WORKSPACE;
  // the full view of the send buffer: chunks_local = ceil(n_local / 64) chunks, all within its padded rows
  const SrcView sv = full_view(n_local, p.chunks_local, p.slabs_local);
  const d4* s = reinterpret_cast<const d4*>(send);
  // the rank's own block: targets and sources are the same rows, the diagonal is at j == i (offset 0)
  shard_accel_jerk_snap_f64_kernel<false><<<dim3(p.groups, p.slabs_local), 64 * kWaves, 0, (hipStream_t)stream>>>(
      s, sv, s, n_local, 0, softening_sq, softening_sq < kEps2MaskedF64 ? 1 : 0, static_cast<double*>(workspace));
  return launch_status();
}

int nbd_hermite6_shard_force_remote_f64(const double* all, int n_total, const double* send, int n_local, int lo,
                                        double softening_sq, double g_const, double* pos, double* vel,
                                        const double* acc_in, const double* jerk_in, const double* snap_in,
                                        double* acc_out, double* jerk_out, double* snap_out, double* crackle_out,
                                        double dt, void* workspace, size_t workspace_bytes, int slabs_local,
                                        int slabs_remote, nbd_stream_t stream) {
  if (!shard_args_ok(n_total, lo, n_local) || !slab_arg_ok(slabs_local) || !slab_arg_ok(slabs_remote))
    return NBD_E_BADARG;
  if (n_local == 0) return 0;
  if (!all || !send || !acc_out || !jerk_out || !snap_out || misaligned32(all) || misaligned32(send))
    return NBD_E_BADARG;
  if (pos && (!vel || !acc_in || !jerk_in || !snap_in || !crackle_out)) return NBD_E_BADARG;
  if (!workspace || misaligned8(workspace) ||
      workspace_bytes < nbd_hermite6_shard_f64_workspace_bytes(n_total, lo, n_local, slabs_local, slabs_remote))
    return NBD_E_WORKSPACE;
  const HShardPlanF64 p = plan_hshard_f64(n_total, lo, n_local, slabs_local, slabs_remote);
  double* slabs = static_cast<double*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  if (p.slabs_remote > 0) {
    // the diagonal never occurs here (every j in [lo, lo + n_local) is left out); lo keeps the index meaning. The view
    // is excluded_view(n_total, ...): its logical chunks map to physical chunks below ceil(n_total / 64)
    shard_accel_jerk_snap_f64_kernel<true><<<dim3(p.groups, p.slabs_remote), 64 * kWaves, 0, st>>>(
        reinterpret_cast<const d4*>(all), p.remote, reinterpret_cast<const d4*>(send), n_local, lo, softening_sq,
        softening_sq < kEps2MaskedF64 ? 1 : 0, slabs + (size_t)p.slabs_local * slab6_doubles(n_local));
    const int rc = launch_status();
    if (rc) return rc;
  }
  shard6_finish_f64_kernel<<<ceil_div(n_local, 256), 256, 0, st>>>(
      slabs, p.slabs_local + p.slabs_remote, n_local, g_const, hermite6_step_constants(dt), pos, vel, acc_in, jerk_in,
      snap_in, acc_out, jerk_out, snap_out, crackle_out);
  return launch_status();
}

}  // extern "C"
