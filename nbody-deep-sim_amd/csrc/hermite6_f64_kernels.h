// hermite6_f64_kernels.h -- what the 6th-order Hermite translation units share (direct_hermite_f64.hip: one system;
// direct_batch_hermite_f64.hip: many independent systems, shared timestep per system; direct_hermite_shard_f64.hip: one
// rank's bodies of a range partition, beside the 4th order; direct_hermite_block_f64.hip: an active list of targets,
// block timesteps, each body with its own step constants): the pair functor of the
// acceleration + jerk + snap evaluation (AccelJerkSnapPair), the step constants (Hermite6Step, hermite6_step_constants),
// the per-row bodies of the predictor and of the finishing kernel (hermite6_predict_row, hermite6_finish_row) and the
// shared step's two O(N) kernels over them: hermite6_predict_kernel<SS> (SS: the row stride of the packed rows) and
// hermite6_finish_kernel<POSD> (POSD: whether it stores the packed row), launched as <1> and <true> by
// direct_hermite_f64.hip and as <3> (send, send + 1, send + 2) and <false> by direct_hermite_shard_f64.hip. As in
// hermite_f64_kernels.h there is one copy of every rounded operation: a scene of a batch has the one-system step's bits
// because the kernels of both units are a prologue and a call of the same inlined code.
// The definitions sit in an anonymous namespace: every translation unit that includes this file gets its own inlined copies.
#pragma once
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

// The step constants: doubles formed from the double dt. On the device too: a block-timestep body
// (direct_hermite_block_f64.hip) forms them from its own step, so one whose step is the whole interval gets the shared
// step's bits.
struct Hermite6Step { double dt, dt_half, dt2_half, dt3_6, dt4_24, dt5_120, dt2_10, dt3_120, dt2, dt3; };

__host__ __device__ inline Hermite6Step hermite6_step_constants(double dt) {
  const double dt2 = dt * dt, dt3 = dt2 * dt;
  return Hermite6Step{dt, 0.5 * dt, 0.5 * dt2, dt3 / 6.0, dt2 * dt2 / 24.0, dt2 * dt3 / 120.0, dt2 / 10.0, dt3 / 120.0,
                      dt2, dt3};
}

// The predictor of body b (its index in pos, vel, acc, jerk, snap, crackle, mass): pm = {x_p, m}, vp = {v_p, 0},
// ap = {a_p, 0},
//   x_p = x + v dt + a dt^2/2 + j dt^3/6 + s dt^4/24 + c dt^5/120,  v_p = v + a dt + j dt^2/2 + s dt^3/6 + c dt^4/24,
//   a_p = a + j dt + s dt^2/2 + c dt^3/6.
// jerk == nullptr (then snap and crackle are too, and h is not read): the plain rows of (pos, vel, acc); acc == nullptr as
// well: ap = 0.
__device__ __forceinline__ void hermite6_predict_row(const double* __restrict__ pos, const double* __restrict__ vel,
                                                     const double* __restrict__ acc, const double* __restrict__ jerk,
                                                     const double* __restrict__ snap,
                                                     const double* __restrict__ crackle,
                                                     const double* __restrict__ mass, size_t b, const Hermite6Step& h,
                                                     d4& pm, d4& vp, d4& ap) {
  double x[3], v[3], a[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    x[k] = pos[3 * b + k];
    v[k] = vel[3 * b + k];
    a[k] = acc ? acc[3 * b + k] : 0.0;
    if (jerk) {
      const double j = jerk[3 * b + k], s = snap[3 * b + k], c = crackle[3 * b + k];
      x[k] = ((((x[k] + v[k] * h.dt) + a[k] * h.dt2_half) + j * h.dt3_6) + s * h.dt4_24) + c * h.dt5_120;
      v[k] = (((v[k] + a[k] * h.dt) + j * h.dt2_half) + s * h.dt3_6) + c * h.dt4_24;
      a[k] = ((a[k] + j * h.dt) + s * h.dt2_half) + c * h.dt3_6;
    }
  }
  pm = d4{x[0], x[1], x[2], mass[b]};
  vp = d4{v[0], v[1], v[2], 0.0};
  ap = d4{a[0], a[1], a[2], 0.0};
}

// The finishing work of one body: a1, j1, s1 = g (slab 0 + slab 1 + ...) of row i of double[n_slabs][9][n] in slab order,
// written to element b of acc_out, jerk_out, snap_out. pos == nullptr: that only (the force on its own). Else the corrector
//   v1 = v + (a0 + a1) dt/2 - (j1 - j0) dt^2/10 + (s0 + s1) dt^3/120
//   x1 = x + (v + v1) dt/2 - (a1 - a0) dt^2/10 + (j0 + j1) dt^3/120
//   c1 = [60 (a1 - a0) - dt (36 j1 + 24 j0) + dt^2 (9 s1 - 3 s0)] / dt^3
// with pos and vel in place and posd[r] = {x1, m}. The outputs may alias acc_in, jerk_in, snap_in: each element is read
// before it is written, by the same thread. POSD = false (a range-sharded rank, direct_hermite_shard_f64.hip: its packed
// rows are rebuilt by the next predictor): posd and mass are not used.
// Returns both ends of the step as the corrector used them (a0, j0, s0 as read; a1, j1, s1, c1 as stored; zeros for a0,
// j0, s0, c1 where pos == nullptr): what a block-timestep body's new level is formed from (hblock6_relevel,
// hermite_block_kernels.h). A caller that drops them pays nothing.
struct Hermite6Ends { double a0[3], j0[3], s0[3], a1[3], j1[3], s1[3], c1[3]; };

template <bool POSD = true>
__device__ __forceinline__ Hermite6Ends hermite6_finish_row(const double* __restrict__ slabs, int n_slabs, size_t n, size_t i,
                                                    size_t b, double g, const Hermite6Step& h, double* pos, double* vel,
                                                    const double* acc_in, const double* jerk_in, const double* snap_in,
                                                    double* acc_out, double* jerk_out, double* snap_out,
                                                    double* crackle_out, const double* __restrict__ mass,
                                                    d4* __restrict__ posd, size_t r) {
  double sum[9];
  slab_order_sum<9>(slabs, n_slabs, n, i, sum);
  double x1[3];
  Hermite6Ends e;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a1 = g * sum[k], j1 = g * sum[k + 3], s1 = g * sum[k + 6];
    e.a0[k] = e.j0[k] = e.s0[k] = e.c1[k] = 0.0;
    if (pos) {
      const double a0 = acc_in[3 * b + k], j0 = jerk_in[3 * b + k], s0 = snap_in[3 * b + k];
      const double x = pos[3 * b + k], v = vel[3 * b + k];
      const double v1 = ((v + (a0 + a1) * h.dt_half) - (j1 - j0) * h.dt2_10) + (s0 + s1) * h.dt3_120;
      x1[k] = ((x + (v + v1) * h.dt_half) - (a1 - a0) * h.dt2_10) + (j0 + j1) * h.dt3_120;
      vel[3 * b + k] = v1;
      pos[3 * b + k] = x1[k];
      crackle_out[3 * b + k] = e.c1[k] =
          ((60.0 * (a1 - a0) - h.dt * (36.0 * j1 + 24.0 * j0)) + h.dt2 * (9.0 * s1 - 3.0 * s0)) / h.dt3;
      e.a0[k] = a0;
      e.j0[k] = j0;
      e.s0[k] = s0;
    }
    acc_out[3 * b + k] = e.a1[k] = a1;
    jerk_out[3 * b + k] = e.j1[k] = j1;
    snap_out[3 * b + k] = e.s1[k] = s1;
  }
  if constexpr (POSD) {
    if (pos) posd[r] = d4{x1[0], x1[1], x1[2], mass[b]};
  }
  return e;
}

// The shared step's two O(N) kernels (direct_hermite_f64.hip; direct_hermite_shard_f64.hip launches the same two on a
// rank's own bodies).
// posd = {x_p, m}, veld = {v_p, 0}, accd = {a_p, 0} for rows [0, n_pad), zero rows behind n: hermite6_predict_row of every
// body. SS: the d4 between consecutive bodies of each of the three, hermite_predict_kernel's SS. 1: three arrays; 3: the send
// buffer of a range-sharded rank, one array of rows {x_p, m | v_p, 0 | a_p, 0} (send, send + 1, send + 2).
template <int SS = 1>
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
  posd[SS * i] = pm;
  veld[SS * i] = vp;
  accd[SS * i] = ap;
}

// One thread per body: hermite6_finish_row<POSD> of the body's row of double[n_slabs][9][n] (pos == nullptr: a1, j1, s1
// only, the force on its own).
template <bool POSD = true>
__global__ __launch_bounds__(256) void hermite6_finish_kernel(const double* __restrict__ slabs, int n_slabs, int n,
                                                              double g, Hermite6Step h, double* pos, double* vel,
                                                              const double* acc_in, const double* jerk_in,
                                                              const double* snap_in, double* acc_out, double* jerk_out,
                                                              double* snap_out, double* crackle_out,
                                                              const double* __restrict__ mass, d4* __restrict__ posd) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n) return;
  hermite6_finish_row<POSD>(slabs, n_slabs, (size_t)n, i, i, g, h, pos, vel, acc_in, jerk_in, snap_in, acc_out, jerk_out,
                            snap_out, crackle_out, mass, posd, i);
}

}  // namespace
