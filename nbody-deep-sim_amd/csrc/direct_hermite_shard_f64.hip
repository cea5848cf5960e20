// direct_hermite_shard_f64.hip -- the double-precision range-sharded Hermite steps, 4th order (the form of
// direct_hermite_shard.hip's step in the number format of direct_hermite_f64.hip) and 6th order (the sharded form of
// direct_hermite_f64.hip's 6th-order step): one rank of a torch.distributed group owns the bodies [lo, lo + n_local) of n_total and
// needs every other rank's PREDICTED rows per step. C-ABI: the nbd_hermite_shard_*_f64 and nbd_hermite6_shard_* entries of
// include/nbd.h; Python: galaxify.simulation.HermiteSimulator(dtype=torch.float64, process_group=...) and
// Hermite6Simulator(process_group=...).
//
// The exchanged row is kArr 32-byte pieces (d4), the streamed arrays side by side: ONE all-gather per step carries them
// all, and walk_f64 (hermite_f64_kernels.h, RQ = 2 kArr) fetches a chunk's pieces by LDS-DMA at the row's stride into the
// [array][128] LDS image the un-sharded kernels use, so the gathered array is read as it lands (no de-interleave launch)
// and the pair loops are the un-sharded ones. A rank's step is four launches, as in fp32; the two O(N) ones are the
// un-sharded steps' kernels (hermite_kernels.h, hermite6_f64_kernels.h), so the only kernel defined here is the pair kernel:
//   predict : the un-sharded predictor kernel at the row's stride (the packed arrays are send, send + 1 and, at the 6th
//             order, send + 2) on the own bodies -> the send buffer, zero rows behind n_local
//   local   : partial sums of the own bodies under the own bodies (reads the send buffer only: runs while the gather is
//             in flight); the un-sharded pair kernel's geometry on n_local sources
//   remote  : the same targets under all bodies of the gathered array except [lo, lo + n_local): whole source chunks
//             inside the range are hopped over, the <= 2 chunks that straddle an end take the masked loop with the range
//             mask (excluded_view, direct_kernels.h)
//   finish  : the un-sharded finishing kernel without its packed store (the next predictor rebuilds the send buffer):
//             slab_order_sum over the local slabs, then the remote ones, times G, and the corrector of the own rows (or
//             the force on its own)
// What the orders differ in (Order4, Order6 of hermite_orders_f64.h; the O(N) kernels and the pointer lists of the entries):
//             row, 8-byte doubles           sums per body  predictor                          finish
//   4th : {x_p, m | v_p, 0}, 8              a, j: 6        hermite_predict_kernel<double, 2>  hermite_correct_kernel<double, false>
//   6th : {x_p, m | v_p, 0 | a_p, 0}, 12    a, j, s: 9     hermite6_predict_kernel<3>         hermite6_finish_kernel<false>: the
//                                                                                             corrector and c1
// Every rounded operation is hermite_f64_kernels.h's, hermite6_f64_kernels.h's or hermite_kernels.h's: a rank that owns
// every body computes nbd_accel_jerk_f64's resp. nbd_accel_jerk_snap_f64's bits, and a and j of any 6th-order rank are the
// 4th order's at the same slab counts. No atomics, no memsets, no host syncs: deterministic with a workspace that may hold
// anything. The LDS-DMA fetch reads whole 64-row chunks: the send buffer and the gathered array are allocated to
// nbd_posm_padded_len(rows) rows with zero rows behind the data, and the view's chunk counts come from n_total.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_kernels.h"
#include "hermite6_f64_kernels.h"
#include "hermite_f64_kernels.h"
#include "hermite_kernels.h"
#include "hermite_orders_f64.h"

namespace {

// The partial sums (Pair::kOut per target) of the targets tgt[0 .. n_tgt) (exchanged rows; global index tgt_off + row)
// under the sources of the view sv on src (exchanged rows): the un-sharded pair kernel's geometry -- grid = (target groups
// of 64, slabs), the view's logical chunks spread over all slabs x 4 waves to within one. RANGE: sv leaves [ex_lo, ex_hi)
// out (the remote block: no target has a source index of its own there); else sv is the full view of src (the local block,
// src == tgt: group g's own indices are chunk g). out: double[slab][kOut][n_tgt].
template <class Order, bool RANGE>
__global__ __launch_bounds__(64 * kWaves) void shard_pair_f64_kernel(const d4* __restrict__ src, const SrcView sv,
                                                                     const d4* __restrict__ tgt, int n_tgt, int tgt_off,
                                                                     double eps2, int all_masked,
                                                                     double* __restrict__ out) {
  using Pair = typename Order::Pair;
  constexpr int kArr = Order::kArr;
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads_n<kArr>()];
  const Group64<unsigned> g(blockIdx.x, blockIdx.y, n_tgt);
  const ChunkRange c = wave_chunks(g.jw(), sv.cpw_q, sv.cpw_r);
  Pair pr = Order::make(tgt, tgt + 1, tgt + 2, (size_t)g.row() * kArr, tgt_off + g.i, eps2, sv.n_src);
  walk_f64<Pair, kArr * kRowQuads, RANGE>(pr, src, src + 1, c.begin, c.end, all_masked != 0,
                                          RANGE ? -1 : (int)blockIdx.x, lds, g.dst<Pair>(out), (size_t)n_tgt,
                                          g.n_valid(), &sv, kArr == 3 ? src + 2 : nullptr);
}

// ---- the host bodies of the entries. The geometry of a rank's two force launches is the same for both orders:
// HShardPlan (hermite_kernels.h), plan_hshard_f64 and slab_arg_ok of hermite_f64_kernels.h.

template <class Order>
size_t slab_doubles(int n_local) { return (size_t)Order::Pair::kOut * n_local; }

int shard_plan(int n_total, int lo, int n_local, int* slabs_local, int* chunks_per_wave_local, int* slabs_remote,
               int* chunks_per_wave_remote) {
  if (!shard_args_ok(n_total, lo, n_local) || n_local == 0) return NBD_E_BADARG;
  hshard_plan_out(plan_hshard_f64(n_total, lo, n_local, 0, 0), slabs_local, chunks_per_wave_local, slabs_remote,
                  chunks_per_wave_remote);
  return 0;
}

template <class Order>
size_t shard_workspace_bytes(int n_total, int lo, int n_local, int slabs_local, int slabs_remote) {
  if (!shard_args_ok(n_total, lo, n_local) || n_local == 0 || !slab_arg_ok(slabs_local) || !slab_arg_ok(slabs_remote))
    return 0;
  const HShardPlan p = plan_hshard_f64(n_total, lo, n_local, slabs_local, slabs_remote);
  return (size_t)(p.slabs_local + p.slabs_remote) * slab_doubles<Order>(n_local) * sizeof(double);
}

template <class Order>
int shard_force_local(const double* send, int n_local, double softening_sq, void* workspace, size_t workspace_bytes,
                      int n_total, int lo, int slabs, nbd_stream_t stream) {
  if (!shard_args_ok(n_total, lo, n_local) || !slab_arg_ok(slabs)) return NBD_E_BADARG;
  if (n_local == 0) return 0;
  if (!send || misaligned32(send)) return NBD_E_BADARG;
  const HShardPlan p = plan_hshard_f64(n_total, lo, n_local, slabs, 0);
  // what this launch writes: the local slabs (the remote call checks the whole buffer)
  if (!workspace || misaligned8(workspace) ||
      workspace_bytes < (size_t)p.slabs_local * slab_doubles<Order>(n_local) * sizeof(double))
    return NBD_E_WORKSPACE;
  // the full view of the send buffer: chunks_local = ceil(n_local / 64) chunks, all within its padded rows
  const SrcView sv = full_view(n_local, p.chunks_local, p.slabs_local);
  const d4* s = reinterpret_cast<const d4*>(send);
  // the rank's own block: targets and sources are the same rows, the diagonal is at j == i (offset 0)
  shard_pair_f64_kernel<Order, false><<<dim3(p.groups, p.slabs_local), 64 * kWaves, 0, (hipStream_t)stream>>>(
      s, sv, s, n_local, 0, softening_sq, softening_sq < kEps2MaskedF64 ? 1 : 0, static_cast<double*>(workspace));
  return launch_status();
}

// The force part of a remote entry: the checks (state_ok: what the entry found of its own pointer list), the remote
// block where the rank does not own every body, then finish(slabs, n_slabs, stream), the entry's finish launch.
template <class Order, class Finish>
int shard_force_remote(const double* all, int n_total, const double* send, int n_local, int lo, double softening_sq,
                       bool state_ok, void* workspace, size_t workspace_bytes, int slabs_local, int slabs_remote,
                       nbd_stream_t stream, Finish finish) {
  if (!shard_args_ok(n_total, lo, n_local) || !slab_arg_ok(slabs_local) || !slab_arg_ok(slabs_remote))
    return NBD_E_BADARG;
  if (n_local == 0) return 0;
  if (!all || !send || misaligned32(all) || misaligned32(send) || !state_ok) return NBD_E_BADARG;
  if (!workspace || misaligned8(workspace) ||
      workspace_bytes < shard_workspace_bytes<Order>(n_total, lo, n_local, slabs_local, slabs_remote))
    return NBD_E_WORKSPACE;
  const HShardPlan p = plan_hshard_f64(n_total, lo, n_local, slabs_local, slabs_remote);
  double* slabs = static_cast<double*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  if (p.slabs_remote > 0) {
    // the diagonal never occurs here (every j in [lo, lo + n_local) is left out); lo keeps the index meaning. The view
    // is excluded_view(n_total, ...): its logical chunks map to physical chunks below ceil(n_total / 64)
    shard_pair_f64_kernel<Order, true><<<dim3(p.groups, p.slabs_remote), 64 * kWaves, 0, st>>>(
        reinterpret_cast<const d4*>(all), p.remote, reinterpret_cast<const d4*>(send), n_local, lo, softening_sq,
        softening_sq < kEps2MaskedF64 ? 1 : 0, slabs + (size_t)p.slabs_local * slab_doubles<Order>(n_local));
    const int rc = launch_status();
    if (rc) return rc;
  }
  finish(slabs, p.slabs_local + p.slabs_remote, st);
  return launch_status();
}

}  // namespace

extern "C" {

int nbd_hermite_shard_f64_plan(int n_total, int lo, int n_local, int* slabs_local, int* chunks_per_wave_local,
                               int* slabs_remote, int* chunks_per_wave_remote) {
  return shard_plan(n_total, lo, n_local, slabs_local, chunks_per_wave_local, slabs_remote, chunks_per_wave_remote);
}

int nbd_hermite6_shard_f64_plan(int n_total, int lo, int n_local, int* slabs_local, int* chunks_per_wave_local,
                                int* slabs_remote, int* chunks_per_wave_remote) {
  return shard_plan(n_total, lo, n_local, slabs_local, chunks_per_wave_local, slabs_remote, chunks_per_wave_remote);
}

size_t nbd_hermite_shard_f64_workspace_bytes(int n_total, int lo, int n_local, int slabs_local, int slabs_remote) {
  return shard_workspace_bytes<Order4>(n_total, lo, n_local, slabs_local, slabs_remote);
}

size_t nbd_hermite6_shard_f64_workspace_bytes(int n_total, int lo, int n_local, int slabs_local, int slabs_remote) {
  return shard_workspace_bytes<Order6>(n_total, lo, n_local, slabs_local, slabs_remote);
}

int nbd_hermite_shard_predict_f64(const double* pos, const double* vel, const double* acc, const double* jerk,
                                  const double* mass, int n_local, double dt, double* send, int send_rows,
                                  nbd_stream_t stream) {
  if (n_local < 0 || send_rows < nbd_posm_padded_len(n_local) || (!acc != !jerk)) return NBD_E_BADARG;
  if (send_rows == 0) return 0;
  if (!send || misaligned32(send) || (n_local > 0 && (!pos || !vel || !mass))) return NBD_E_BADARG;
  d4* s = reinterpret_cast<d4*>(send);
  hermite_predict_kernel<double, Order4::kArr><<<ceil_div(send_rows, 256), 256, 0, (hipStream_t)stream>>>(
      pos, vel, acc, jerk, mass, n_local, send_rows, hermite_step_constants<double>(dt), s, s + 1);
  return launch_status();
}

int nbd_hermite6_shard_predict_f64(const double* pos, const double* vel, const double* acc, const double* jerk,
                                   const double* snap, const double* crackle, const double* mass, int n_local, double dt,
                                   double* send, int send_rows, nbd_stream_t stream) {
  if (n_local < 0 || send_rows < nbd_posm_padded_len(n_local)) return NBD_E_BADARG;
  if ((!jerk != !snap) || (!jerk != !crackle) || (jerk && !acc)) return NBD_E_BADARG;
  if (send_rows == 0) return 0;
  if (!send || misaligned32(send) || (n_local > 0 && (!pos || !vel || !mass))) return NBD_E_BADARG;
  d4* s = reinterpret_cast<d4*>(send);
  hermite6_predict_kernel<Order6::kArr><<<ceil_div(send_rows, 256), 256, 0, (hipStream_t)stream>>>(
      pos, vel, acc, jerk, snap, crackle, mass, n_local, send_rows, hermite6_step_constants(dt), s, s + 1, s + 2);
  return launch_status();
}

int nbd_hermite_shard_force_local_f64(const double* send, int n_local, double softening_sq, void* workspace,
                                      size_t workspace_bytes, int n_total, int lo, int slabs, nbd_stream_t stream) {
  return shard_force_local<Order4>(send, n_local, softening_sq, workspace, workspace_bytes, n_total, lo, slabs, stream);
}

int nbd_hermite6_shard_force_local_f64(const double* send, int n_local, double softening_sq, void* workspace,
                                       size_t workspace_bytes, int n_total, int lo, int slabs, nbd_stream_t stream) {
  return shard_force_local<Order6>(send, n_local, softening_sq, workspace, workspace_bytes, n_total, lo, slabs, stream);
}

int nbd_hermite_shard_force_remote_f64(const double* all, int n_total, const double* send, int n_local, int lo,
                                       double softening_sq, double g_const, double* pos, double* vel,
                                       const double* acc_in, const double* jerk_in, double* acc_out, double* jerk_out,
                                       double dt, void* workspace, size_t workspace_bytes, int slabs_local,
                                       int slabs_remote, nbd_stream_t stream) {
  const bool state_ok = acc_out && jerk_out && !(pos && (!vel || !acc_in || !jerk_in));
  return shard_force_remote<Order4>(
      all, n_total, send, n_local, lo, softening_sq, state_ok, workspace, workspace_bytes, slabs_local, slabs_remote,
      stream, [=](const double* slabs, int n_slabs, hipStream_t st) {
        hermite_correct_kernel<double, false><<<ceil_div(n_local, HermiteFmt<double>::kSumRows), 256, 0, st>>>(
            slabs, n_slabs, n_local, g_const, hermite_step_constants<double>(dt), pos, vel, acc_in, jerk_in, acc_out,
            jerk_out, nullptr, nullptr);
      });
}

int nbd_hermite6_shard_force_remote_f64(const double* all, int n_total, const double* send, int n_local, int lo,
                                        double softening_sq, double g_const, double* pos, double* vel,
                                        const double* acc_in, const double* jerk_in, const double* snap_in,
                                        double* acc_out, double* jerk_out, double* snap_out, double* crackle_out,
                                        double dt, void* workspace, size_t workspace_bytes, int slabs_local,
                                        int slabs_remote, nbd_stream_t stream) {
  const bool state_ok =
      acc_out && jerk_out && snap_out && !(pos && (!vel || !acc_in || !jerk_in || !snap_in || !crackle_out));
  return shard_force_remote<Order6>(
      all, n_total, send, n_local, lo, softening_sq, state_ok, workspace, workspace_bytes, slabs_local, slabs_remote,
      stream, [=](const double* slabs, int n_slabs, hipStream_t st) {
        hermite6_finish_kernel<false><<<ceil_div(n_local, 256), 256, 0, st>>>(
            slabs, n_slabs, n_local, g_const, hermite6_step_constants(dt), pos, vel, acc_in, jerk_in, snap_in, acc_out,
            jerk_out, snap_out, crackle_out, nullptr, nullptr);
      });
}

}  // extern "C"
