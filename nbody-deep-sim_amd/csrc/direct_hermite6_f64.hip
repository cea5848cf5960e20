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
// arrays and the pair functor AccelJerkSnapPair below, in accel_jerk_f64_kernel's geometry (plan_f64, chunk_split, four
// waves on 64 targets, LDS-DMA double buffering, the counted vmcnt(6)); 48 KiB of LDS per workgroup: three per CU.
//
// One step is three launches (PEC form; a0, j0, s0 and the crackle c0 = d^3 a / dt^3 carried):
//   predict : hermite6_predict_kernel -> posd = {x_p, m}, veld = {v_p, 0}, accd = {a_p, 0}, Taylor series to c0
//   evaluate: accel_jerk_snap_f64_kernel -> double[slabs][9][n] partial sums (unscaled)
//   correct : hermite6_finish_kernel: the slabs in slab order (slab_order_sum<9>, one thread per body), a1, j1, s1 = G sum,
//             the corrector, c1 = the third derivative at t1 of the quintic through (a, j, s) at both ends, posd = {x1, m}
// The step constants are doubles formed from the double dt and are never rounded to fp32; every product and sum of the
// two O(N) kernels rounds on its own (the build has -ffp-contract=off). No atomics, no memsets, no host syncs:
// deterministic run to run with a workspace that may hold anything.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_kernels.h"
#include "hermite_f64_kernels.h"
#include "hermite_kernels.h"

namespace {

// The pair functor (what a functor is: hermite_f64_kernels.h). p = {x, y, z, m}, q = {vx, vy, vz, 0}, r = {ax, ay, az, 0}
// of source j. acc[0..8] are AccelJerkPair's sums, formed by AccelJerkPair::pair's operations one for one and in the same
// order, so out(0..5) are that functor's bits. The snap has sums of its own: sn[0..2] = sum w a, sn[3..5] = sum alpha w v,
// sn[6..8] = sum (15 alpha^2 - 3 gamma) w r; out(6..8) = (sn[0..2] - 6 sn[3..5]) + sn[6..8]. MASKED drops j == i and the
// padding behind n by the select on s (after the refinement: w, alpha and gamma of a dropped pair are exact zeros whatever
// its r^2 gave, NaN included). Un-masked, i == j (r = v = a = 0, s finite) and a padding row (m = 0) add exact zeros.
struct AccelJerkSnapPair {
  static constexpr int kStreams = 3;
  static constexpr int kOut = 9;
  double xi, yi, zi, ui, vi, wi, axi, ayi, azi, e2;
  double acc[9], sn[9];
  int i, n;

  __device__ __forceinline__ AccelJerkSnapPair(const d4 tp, const d4 tv, const d4 ta, double eps2, int i_, int n_)
      : xi(tp.x), yi(tp.y), zi(tp.z), ui(tv.x), vi(tv.y), wi(tv.z), axi(ta.x), ayi(ta.y), azi(ta.z), e2(eps2), i(i_),
        n(n_) {
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = sn[k] = 0.0;
  }

  template <bool MASKED>
  __device__ __forceinline__ void pair(const d4 p, const d4 q, const d4 r, int j) {
    const double dx = p.x - xi, dy = p.y - yi, dz = p.z - zi;      // r_j - r_i
    const double du = q.x - ui, dv = q.y - vi, dw = q.z - wi;
    const double dax = r.x - axi, day = r.y - ayi, daz = r.z - azi;
    double r2 = __builtin_fma(dx, dx, e2);
    r2 = __builtin_fma(dy, dy, r2);
    r2 = __builtin_fma(dz, dz, r2);
    double rv = dx * du;
    rv = __builtin_fma(dy, dv, rv);
    rv = __builtin_fma(dz, dw, rv);
    double va = du * du;                                           // v.v + r.a
    va = __builtin_fma(dv, dv, va);
    va = __builtin_fma(dw, dw, va);
    va = __builtin_fma(dx, dax, va);
    va = __builtin_fma(dy, day, va);
    va = __builtin_fma(dz, daz, va);
    double s = rsqrt_f64(r2);
    if (MASKED) s = (j < n && j != i) ? s : 0.0;
    const double s2 = s * s;
    const double w = (s2 * s) * p.w;
    const double al = rv * s2;
    const double c = al * w;
    const double gm = va * s2;
    const double b = __builtin_fma(15.0 * al, al, -3.0 * gm) * w;
    acc[0] = __builtin_fma(w, dx, acc[0]);
    acc[1] = __builtin_fma(w, dy, acc[1]);
    acc[2] = __builtin_fma(w, dz, acc[2]);
    acc[3] = __builtin_fma(w, du, acc[3]);
    acc[4] = __builtin_fma(w, dv, acc[4]);
    acc[5] = __builtin_fma(w, dw, acc[5]);
    acc[6] = __builtin_fma(c, dx, acc[6]);
    acc[7] = __builtin_fma(c, dy, acc[7]);
    acc[8] = __builtin_fma(c, dz, acc[8]);
    sn[0] = __builtin_fma(w, dax, sn[0]);
    sn[1] = __builtin_fma(w, day, sn[1]);
    sn[2] = __builtin_fma(w, daz, sn[2]);
    sn[3] = __builtin_fma(c, du, sn[3]);
    sn[4] = __builtin_fma(c, dv, sn[4]);
    sn[5] = __builtin_fma(c, dw, sn[5]);
    sn[6] = __builtin_fma(b, dx, sn[6]);
    sn[7] = __builtin_fma(b, dy, sn[7]);
    sn[8] = __builtin_fma(b, dz, sn[8]);
  }

  __device__ __forceinline__ double out(int k) const {
    if (k < 3) return acc[k];
    if (k < 6) return acc[k] - 3.0 * acc[k + 3];
    return (sn[k - 6] - 6.0 * sn[k - 3]) + sn[k];
  }
};

// Acceleration + jerk + snap of all n bodies under all n bodies, accel_jerk_f64_kernel's geometry: grid = (groups of 64
// targets, slabs), the source chunks spread over all slabs x 4 waves to within one. out: double[slab][9][n].
__global__ __launch_bounds__(64 * kWaves) void accel_jerk_snap_f64_kernel(const d4* __restrict__ posd,
                                                                          const d4* __restrict__ veld,
                                                                          const d4* __restrict__ accd, int n, int cpw_q,
                                                                          int cpw_r, double eps2, int all_masked,
                                                                          double* __restrict__ out) {
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads_n<3>()];
  const int t_base = blockIdx.x * kTgtF64;
  const int i = t_base + (threadIdx.x & 63), row = min(i, n - 1);
  const int jw = blockIdx.y * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int c_begin, c_end;
  wave_chunk_range(jw, cpw_q, cpw_r, c_begin, c_end);
  AccelJerkSnapPair pr(posd[row], veld[row], accd[row], eps2, i, n);
  walk_f64(pr, posd, veld, c_begin, c_end, all_masked != 0, blockIdx.x, lds,
           out + (size_t)blockIdx.y * AccelJerkSnapPair::kOut * n + t_base, (size_t)n, min(kTgtF64, n - t_base), nullptr,
           accd);
}

// The step constants: doubles formed from the double dt.
struct Hermite6Step { double dt, dt_half, dt2_half, dt3_6, dt4_24, dt5_120, dt2_10, dt3_120, dt2, dt3; };

inline Hermite6Step hermite6_step_constants(double dt) {
  const double dt2 = dt * dt, dt3 = dt2 * dt;
  return Hermite6Step{dt, 0.5 * dt, 0.5 * dt2, dt3 / 6.0, dt2 * dt2 / 24.0, dt2 * dt3 / 120.0, dt2 / 10.0, dt3 / 120.0,
                      dt2, dt3};
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
  if (i < (size_t)n) {
    double x[3], v[3], a[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      x[k] = pos[3 * i + k];
      v[k] = vel[3 * i + k];
      a[k] = acc ? acc[3 * i + k] : 0.0;
      if (jerk) {
        const double j = jerk[3 * i + k], s = snap[3 * i + k], c = crackle[3 * i + k];
        x[k] = ((((x[k] + v[k] * h.dt) + a[k] * h.dt2_half) + j * h.dt3_6) + s * h.dt4_24) + c * h.dt5_120;
        v[k] = (((v[k] + a[k] * h.dt) + j * h.dt2_half) + s * h.dt3_6) + c * h.dt4_24;
        a[k] = ((a[k] + j * h.dt) + s * h.dt2_half) + c * h.dt3_6;
      }
    }
    pm = d4{x[0], x[1], x[2], mass[i]};
    vp = d4{v[0], v[1], v[2], 0.0};
    ap = d4{a[0], a[1], a[2], 0.0};
  }
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
  double sum[9];
  slab_order_sum<9>(slabs, n_slabs, (size_t)n, i, sum);
  double x1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a1 = g * sum[k], j1 = g * sum[k + 3], s1 = g * sum[k + 6];
    if (pos) {
      const double a0 = acc_in[3 * i + k], j0 = jerk_in[3 * i + k], s0 = snap_in[3 * i + k];
      const double x = pos[3 * i + k], v = vel[3 * i + k];
      const double v1 = ((v + (a0 + a1) * h.dt_half) - (j1 - j0) * h.dt2_10) + (s0 + s1) * h.dt3_120;
      x1[k] = ((x + (v + v1) * h.dt_half) - (a1 - a0) * h.dt2_10) + (j0 + j1) * h.dt3_120;
      vel[3 * i + k] = v1;
      pos[3 * i + k] = x1[k];
      crackle_out[3 * i + k] =
          ((60.0 * (a1 - a0) - h.dt * (36.0 * j1 + 24.0 * j0)) + h.dt2 * (9.0 * s1 - 3.0 * s0)) / h.dt3;
    }
    acc_out[3 * i + k] = a1;
    jerk_out[3 * i + k] = j1;
    snap_out[3 * i + k] = s1;
  }
  if (pos) posd[i] = d4{x1[0], x1[1], x1[2], mass[i]};
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
