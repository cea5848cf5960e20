// direct_hermite_shard.hip -- the range-sharded form of direct_hermite.hip's 4th-order Hermite step: one rank of a
// torch.distributed group owns the bodies [lo, lo + n_local) of n_total and needs every other rank's PREDICTED position,
// mass and velocity per step. C-ABI: the nbd_hermite_shard_* entries of include/nbd.h; Python:
// galaxify.simulation.HermiteSimulator(process_group=...).
//
// The exchanged row is 8 floats, {x_p, y_p, z_p, m, vx_p, vy_p, vz_p, 0}: ONE all-gather per step carries both quads, and
// accel_jerk_body (hermite_kernels.h, SS = 2) fetches a row's position quad and velocity quad by LDS-DMA at a two-quad
// stride, so the gathered array is read as it lands (no de-interleave launch). A rank's step is four launches; the two
// O(N) ones are the un-sharded step's kernels (hermite_kernels.h), so the only kernel defined here is the pair kernel:
//   predict : hermite_predict_kernel<float, 2> on the own bodies -> the send buffer (posm = send, velp = send + 1 at the
//             row's two-quad stride), zero rows behind n_local
//   local   : a, j partial sums of the own bodies under the own bodies (reads the send buffer only: runs while the
//             gather is in flight); the un-sharded kernel's geometry on n_local sources
//   remote  : the same under all bodies of the gathered array except [lo, lo + n_local): whole source chunks inside the
//             range are hopped over, the <= 2 chunks that straddle an end take the masked loop with the range mask
//             (excluded_view, direct_kernels.h -- the leapfrog shard's view)
//   finish  : hermite_correct_kernel<float, false>: hermite_slab_sum over the local slabs, then the remote ones (a fixed
//             order), times G, and hermite_correct_row of the own rows -- a launch of its own, as in the un-sharded step
//             (or a1, j1 only: the force on its own); no packed row is stored, the next predictor rebuilds the send buffer
// Every rounded operation is one of hermite_kernels.h's. No atomics, no memsets, no host syncs: deterministic, capturable.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_kernels.h"
#include "hermite_kernels.h"

namespace {

constexpr int kRowQuads = 2;      // float4 per exchanged row: {x_p, m}, {v_p, 0}

// Acceleration + jerk partial sums of the targets tgt[0 .. n_tgt) (8-float rows; global index tgt_off + row) under the
// sources of the view sv on src (8-float rows): accel_jerk_kernel<MASKED, 2>'s geometry -- grid = (target groups of 128,
// slabs), the view's logical chunks spread over all slabs x 4 waves to within one. RANGE: sv leaves [ex_lo, ex_hi) out
// (the remote block); else sv is the full view of src (the local block, src == tgt). out: float[slab][6][n_tgt].
// 6 waves per SIMD as accel_jerk_kernel<., 2>; RANGE holds both pair loops and the view, which do not fit 80 VGPRs
// without scratch: 5 waves per SIMD.
template <bool MASKED, bool RANGE>
__global__ __launch_bounds__(64 * kWaves, RANGE ? 5 : 6) void shard_accel_jerk_kernel(
    const f4* __restrict__ src, const SrcView sv, const f4* __restrict__ tgt, int n_tgt, int tgt_off, float eps2,
    float* __restrict__ out) {
  __shared__ f4 lds[kWaves * 4 * kChunk];
  const Group128<unsigned> g(blockIdx.x, blockIdx.y, n_tgt);
  const ChunkRange c = wave_chunks(g.jw(), sv.cpw_q, sv.cpw_r);
  accel_jerk_body<MASKED, 2, kRowQuads, RANGE>(src, src + 1, sv.n_src, tgt, tgt + 1, g.r0(), g.r1(), tgt_off + g.i0,
                                               tgt_off + g.i1, c.begin, c.end, eps2, lds, g.dst(out), n_tgt, g.n_valid(),
                                               &sv);
}

// The geometry of a rank's two force launches (HShardPlan, hermite_kernels.h): the leapfrog shard's slab counts
// (nbd_shard_plan: same targets, same chunks, the same balance problem), raised where a wave's sequential fp32 chain would
// pass 64 chunks (4096 sources).
int chain_slabs(int slabs, int n_chunks) {
  const int min_slabs = ceil_div(n_chunks, kWaves * 64);
  slabs = slabs < min_slabs ? min_slabs : slabs;
  return slabs > kMaxSlabs ? kMaxSlabs : slabs;
}

// n_local > 0
HShardPlan plan_hshard(int n_total, int lo, int n_local) {
  HShardPlan p;
  int cpw_l = 0, cpw_r = 0;
  nbd_shard_plan(n_total, lo, n_local, &p.slabs_local, &cpw_l, &p.slabs_remote, &cpw_r);
  p.groups = ceil_div(n_local, kTgtPerWG);
  p.chunks_local = ceil_div(n_local, kChunk);
  p.chunks_remote = excluded_view(n_total, lo, lo + n_local, &p.remote);
  p.slabs_local = chain_slabs(p.slabs_local, p.chunks_local);
  p.slabs_remote = p.chunks_remote > 0 ? chain_slabs(p.slabs_remote, p.chunks_remote) : 0;
  split_chunks(p.remote, p.chunks_remote, p.slabs_remote > 0 ? p.slabs_remote : 1);
  return p;
}

size_t slab_floats(int n_local) { return (size_t)6 * n_local; }

}  // namespace

extern "C" {

int nbd_hermite_shard_plan(int n_total, int lo, int n_local, int* slabs_local, int* chunks_per_wave_local,
                           int* slabs_remote, int* chunks_per_wave_remote) {
  if (!shard_args_ok(n_total, lo, n_local) || n_local == 0) return NBD_E_BADARG;
  hshard_plan_out(plan_hshard(n_total, lo, n_local), slabs_local, chunks_per_wave_local, slabs_remote,
                  chunks_per_wave_remote);
  return 0;
}

size_t nbd_hermite_shard_workspace_bytes(int n_total, int lo, int n_local) {
  if (!shard_args_ok(n_total, lo, n_local) || n_local == 0) return 0;
  const HShardPlan p = plan_hshard(n_total, lo, n_local);
  return (size_t)(p.slabs_local + p.slabs_remote) * slab_floats(n_local) * sizeof(float);
}

int nbd_hermite_shard_predict_f32(const float* pos, const float* vel, const float* acc, const float* jerk,
                                  const float* mass, int n_local, double dt, float* send, int send_rows,
                                  nbd_stream_t stream) {
  if (n_local < 0 || send_rows < nbd_posm_padded_len(n_local) || (!acc != !jerk)) return NBD_E_BADARG;
  if (send_rows == 0) return 0;
  if (!send || misaligned16(send) || (n_local > 0 && (!pos || !vel || !mass))) return NBD_E_BADARG;
  f4* s = reinterpret_cast<f4*>(send);
  hermite_predict_kernel<float, kRowQuads><<<ceil_div(send_rows, 256), 256, 0, (hipStream_t)stream>>>(
      pos, vel, acc, jerk, mass, n_local, send_rows, hermite_dt(dt), s, s + 1);
  return launch_status();
}

int nbd_hermite_shard_force_local_f32(const float* send, int n_local, float softening_sq, void* workspace,
                                      size_t workspace_bytes, int n_total, int lo, nbd_stream_t stream) {
  if (!shard_args_ok(n_total, lo, n_local)) return NBD_E_BADARG;
  if (n_local == 0) return 0;
  if (!send || misaligned16(send)) return NBD_E_BADARG;
  if (!workspace || workspace_bytes < nbd_hermite_shard_workspace_bytes(n_total, lo, n_local)) return NBD_E_WORKSPACE;
  const HShardPlan p = plan_hshard(n_total, lo, n_local);
  const SrcView sv = full_view(n_local, p.chunks_local, p.slabs_local);
  const dim3 grid(p.groups, p.slabs_local), block(64 * kWaves);
  const f4* s = reinterpret_cast<const f4*>(send);
  float* slabs = static_cast<float*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  // the rank's own block: targets and sources are the same rows, the diagonal is at j == i (offset 0)
  if (softening_sq < kEps2Masked)
    shard_accel_jerk_kernel<true, false><<<grid, block, 0, st>>>(s, sv, s, n_local, 0, softening_sq, slabs);
  else
    shard_accel_jerk_kernel<false, false><<<grid, block, 0, st>>>(s, sv, s, n_local, 0, softening_sq, slabs);
  return launch_status();
}

int nbd_hermite_shard_force_remote_f32(const float* all, int n_total, const float* send, int n_local, int lo,
                                       float softening_sq, float g_const, float* pos, float* vel, const float* acc_in,
                                       const float* jerk_in, float* acc_out, float* jerk_out, double dt, void* workspace,
                                       size_t workspace_bytes, nbd_stream_t stream) {
  if (!shard_args_ok(n_total, lo, n_local)) return NBD_E_BADARG;
  if (n_local == 0) return 0;
  if (!all || !send || !acc_out || !jerk_out || misaligned16(all) || misaligned16(send)) return NBD_E_BADARG;
  if (pos && (!vel || !acc_in || !jerk_in)) return NBD_E_BADARG;
  if (!workspace || workspace_bytes < nbd_hermite_shard_workspace_bytes(n_total, lo, n_local)) return NBD_E_WORKSPACE;
  const HShardPlan p = plan_hshard(n_total, lo, n_local);
  float* slabs = static_cast<float*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  if (p.slabs_remote > 0) {
    const dim3 grid(p.groups, p.slabs_remote), block(64 * kWaves);
    const f4* a = reinterpret_cast<const f4*>(all);
    const f4* s = reinterpret_cast<const f4*>(send);
    float* out = slabs + (size_t)p.slabs_local * slab_floats(n_local);
    // the diagonal never occurs here (every j in [lo, lo + n_local) is left out); lo keeps the index meaning
    if (softening_sq < kEps2Masked)
      shard_accel_jerk_kernel<true, true><<<grid, block, 0, st>>>(a, p.remote, s, n_local, lo, softening_sq, out);
    else
      shard_accel_jerk_kernel<false, true><<<grid, block, 0, st>>>(a, p.remote, s, n_local, lo, softening_sq, out);
    const int rc = launch_status();
    if (rc) return rc;
  }
  // all slabs, local ones first; the send buffer is not written (the next predictor rebuilds it)
  hermite_correct_kernel<float, false><<<ceil_div(n_local, HermiteFmt<float>::kSumRows), 256, 0, st>>>(
      slabs, p.slabs_local + p.slabs_remote, n_local, g_const, hermite_dt(dt), pos, vel, acc_in, jerk_in, acc_out,
      jerk_out, nullptr, nullptr);
  return launch_status();
}

}  // extern "C"
