// direct_batch_hermite6_f64.hip -- direct_hermite6_f64.hip's 6th-order Hermite step, applied to every scene of an ensemble of
// independent systems by one set of launches (gfx950): direct_batch_hermite_f64.hip in the scheme of direct_hermite6_f64.hip.
// C-ABI: the nbd_batch_hermite6_* / nbd_batch_accel_jerk_snap_f64 entries of include/nbd.h; Python:
// galaxify.simulation.BatchedSimulator(integrator="hermite6").
//
// The scenes lie back to back; the packed rows are posd = {x, y, z, m}, veld = {vx, vy, vz, 0} and accd = {ax, ay, az, 0},
// d4 each, every scene padded to whole chunks of 64 rows with zero rows. The work list is the float64 plan
// (direct_batch_plan.h, direct_batch_hermite_f64.hip: one item per (scene, group of 64 targets, slab), plan_f64(n_s)'s
// geometry) with ws_off the first double of the scene's double[slabs][9][n_s] partial sums: the same items, rows and
// bytes, so the float64 diagnostic entries run on it unchanged (they read ws_off and use the front of a scene's region).
//
// Every per-scene scalar comes from ONE device table of doubles, par[kParams][S]: rows 0..2 are the float64 table's G,
// eps^2, eps, then the ten members of Hermite6Step in its order, formed on the host by hermite6_step_constants'
// expressions. No kernel takes a per-scene scalar by value, so a step can be captured into a graph and a changed dt,
// softening or G is a rewrite of the table. One step is three launches:
//   predict  : one thread per packed row: hermite6_predict_row with the scene's constants
//   evaluate : one workgroup per item: AccelJerkSnapPair + walk_f64 on the scene's rows, the chunks of wave 4 k + w under
//              the scene's own balanced split; unscaled partial sums into the scene's double[slabs][9][n_s]
//   correct  : one thread per packed row: hermite6_finish_row (slab order, x G_s, corrector, crackle), posd = {x1, m}
// Every kernel here is a prologue that reads its geometry and calls the single copies of the arithmetic
// (hermite6_f64_kernels.h, hermite_f64_kernels.h): a scene's results are bit-identical to the one-system entries on that
// scene alone. No atomics, no memsets, no host syncs: deterministic with a workspace that may hold anything.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_batch_plan.h"
#include "direct_kernels.h"
#include "hermite6_f64_kernels.h"
#include "hermite_f64_kernels.h"
#include "hermite_kernels.h"

namespace {

// rows of the per-scene parameter table par[kParams][S]: the float64 table's first three, then Hermite6Step's members
enum ParamRow { kG = 0, kEps2, kEps, kStep, kParams = kStep + (int)(sizeof(Hermite6Step) / sizeof(double)) };
static_assert(kParams == NBD_BATCH_H6_PARAM_ROWS, "the table include/nbd.h describes");

// the scene's step constants, member k of Hermite6Step from row kStep + k
__device__ __forceinline__ Hermite6Step load_step(const double* __restrict__ par, int n_scenes, int s) {
  const double* p = par + (size_t)kStep * n_scenes + s;
  const size_t S = (size_t)n_scenes;
  return Hermite6Step{p[0], p[S], p[2 * S], p[3 * S], p[4 * S], p[5 * S], p[6 * S], p[7 * S], p[8 * S], p[9 * S]};
}

// the plan counted in doubles (direct_batch_plan.h) with the scene's slabs double[slabs][9][n]
constexpr int kOut = AccelJerkSnapPair::kOut;

// posd[r] = {x_p, m}, veld[r] = {v_p, 0}, accd[r] = {a_p, 0} for every packed row r (zero rows behind each scene's last
// body). jerk == nullptr (then snap, crackle and par are too): a plain pack of (x, v, a); acc == nullptr as well: accd = 0.
__global__ __launch_bounds__(256) void batch_hermite6_predict_kernel(
    const int* __restrict__ row_scene, const SceneRec* __restrict__ scenes, int n_rows, const double* __restrict__ pos,
    const double* __restrict__ vel, const double* __restrict__ acc, const double* __restrict__ jerk,
    const double* __restrict__ snap, const double* __restrict__ crackle, const double* __restrict__ mass,
    const double* __restrict__ par, int n_scenes, d4* __restrict__ posd, d4* __restrict__ veld, d4* __restrict__ accd) {
  PlanRow w;
  if (!load_row(row_scene, scenes, n_rows, w)) return;
  d4 pm = {0.0, 0.0, 0.0, 0.0}, vp = pm, ap = pm;
  if (w.i() < w.sc.n) {
    Hermite6Step h = {};
    if (jerk) h = load_step(par, n_scenes, w.s);
    hermite6_predict_row(pos, vel, acc, jerk, snap, crackle, mass, (size_t)w.sc.off + w.i(), h, pm, vp, ap);
  }
  posd[w.r] = pm;
  veld[w.r] = vp;
  accd[w.r] = ap;
}

// One workgroup per item (s, g, k): accel_jerk_snap_f64_kernel's prologue read from the scene record -- targets
// [64 g, 64 g + 64) of scene s, the chunks of wave 4 k + w under chunk_split(n_chunks, slabs) of the scene -- then the
// same walk_f64. out: the scene's double[slabs][9][n] at ws + ws_off.
__global__ __launch_bounds__(64 * kWaves) void batch_accel_jerk_snap_f64_kernel(
    const d4* __restrict__ posd, const d4* __restrict__ veld, const d4* __restrict__ accd,
    const int4* __restrict__ items, const SceneRec* __restrict__ scenes, const double* __restrict__ par, int n_scenes,
    double* __restrict__ ws) {
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads_n<3>()];
  const Item w = load_item(items, scenes);
  const double eps2 = par[kEps2 * n_scenes + w.s];
  const d4* pd = posd + w.poff;
  const d4* vd = veld + w.poff;
  const d4* ad = accd + w.poff;
  const Group64<int> g(w.grp, w.slab, w.n);
  const ChunkRange c = wave_chunks_of(g.jw(), w.n_chunks, w.slabs);
  AccelJerkSnapPair pr(pd[g.row()], vd[g.row()], ad[g.row()], eps2, g.i, w.n);
  walk_f64(pr, pd, vd, c.begin, c.end, eps2 < kEps2MaskedF64, w.grp, lds,
           g.dst<AccelJerkSnapPair>(ws + (size_t)w.ws_off), (size_t)w.n, g.n_valid(), nullptr, ad);
}

// One thread per packed row (a row belongs to one scene; the padding rows leave at once): hermite6_finish_row of the body's
// row in its scene's slabs with G_s and the scene's step constants. pos == nullptr: a1, j1, s1 only.
__global__ __launch_bounds__(256) void batch_hermite6_finish_kernel(
    const int* __restrict__ row_scene, const SceneRec* __restrict__ scenes, int n_rows, const double* __restrict__ ws,
    const double* __restrict__ par, int n_scenes, double* pos, double* vel, const double* acc_in, const double* jerk_in,
    const double* snap_in, double* acc_out, double* jerk_out, double* snap_out, double* crackle_out,
    const double* __restrict__ mass, d4* __restrict__ posd) {
  PlanRow w;
  if (!load_row(row_scene, scenes, n_rows, w) || w.i() >= w.sc.n) return;
  const Hermite6Step h = load_step(par, n_scenes, w.s);
  hermite6_finish_row(ws + (size_t)w.sc.ws_off, w.sc.slabs, (size_t)w.sc.n, (size_t)w.i(), (size_t)w.sc.off + w.i(),
                      par[kG * n_scenes + w.s], h, pos, vel, acc_in, jerk_in, snap_in, acc_out, jerk_out, snap_out,
                      crackle_out, mass, posd, (size_t)w.r);
}

int launch_predict(const DevPlan& d, const BatchTotals& t, const double* pos, const double* vel, const double* acc,
                   const double* jerk, const double* snap, const double* crackle, const double* mass, const double* par,
                   double* posd, double* veld, double* accd, hipStream_t st) {
  batch_hermite6_predict_kernel<<<ceil_div(t.n_rows, 256), 256, 0, st>>>(
      d.row_scene, d.scenes, t.n_rows, pos, vel, acc, jerk, snap, crackle, mass, par, t.n_scenes,
      reinterpret_cast<d4*>(posd), reinterpret_cast<d4*>(veld), reinterpret_cast<d4*>(accd));
  return launch_status();
}

// the evaluation of every scene at posd / veld / accd, then the slab sum (+ the corrector when pos is given)
int launch_force_finish(const DevPlan& d, const BatchTotals& t, double* posd, const double* veld, const double* accd,
                        const double* par, double* pos, double* vel, const double* acc_in, const double* jerk_in,
                        const double* snap_in, double* acc_out, double* jerk_out, double* snap_out, double* crackle_out,
                        const double* mass, void* workspace, hipStream_t st) {
  double* ws = static_cast<double*>(workspace);
  batch_accel_jerk_snap_f64_kernel<<<t.n_items, 64 * kWaves, 0, st>>>(
      reinterpret_cast<const d4*>(posd), reinterpret_cast<const d4*>(veld), reinterpret_cast<const d4*>(accd), d.items,
      d.scenes, par, t.n_scenes, ws);
  const int rc = launch_status();
  if (rc) return rc;
  batch_hermite6_finish_kernel<<<ceil_div(t.n_rows, 256), 256, 0, st>>>(
      d.row_scene, d.scenes, t.n_rows, ws, par, t.n_scenes, pos, vel, acc_in, jerk_in, snap_in, acc_out, jerk_out,
      snap_out, crackle_out, mass, reinterpret_cast<d4*>(posd));
  return launch_status();
}

bool bad_rows(const double* posd, const double* veld, const double* accd) {
  return !posd || !veld || !accd || misaligned32(posd) || misaligned32(veld) || misaligned32(accd);
}

}  // namespace

extern "C" {

int nbd_batch_hermite6_f64_plan_fill(const int* offsets, int n_scenes, void* plan, size_t plan_bytes) {
  return plan_fill_f64<kOut>(offsets, n_scenes, plan, plan_bytes);
}

int nbd_batch_hermite6_f64_workspace_bytes(const int* offsets, int n_scenes, size_t* bytes) {
  return workspace_bytes_f64<kOut>(offsets, n_scenes, bytes);
}

int nbd_batch_hermite6_pack_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const double* pos,
                                const double* vel, const double* acc, const double* mass, double* posd, double* veld,
                                double* accd, nbd_stream_t stream) {
  BatchTotals t;
  const int rc = prologue_f64<kOut>(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc) return rc;
  if (t.n_total == 0) return 0;
  if (!pos || !vel || !mass || bad_rows(posd, veld, accd)) return NBD_E_BADARG;
  return launch_predict(dev_plan(plan, t), t, pos, vel, acc, nullptr, nullptr, nullptr, mass, nullptr, posd, veld, accd,
                        (hipStream_t)stream);
}

int nbd_batch_accel_jerk_snap_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes,
                                  const double* posd, const double* veld, const double* accd, const double* params,
                                  double* acc_out, double* jerk_out, double* snap_out, void* workspace,
                                  size_t workspace_bytes, nbd_stream_t stream) {
  BatchTotals t;
  const int rc = prologue_f64<kOut>(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc) return rc;
  if (t.n_total == 0) return 0;
  if (bad_rows(posd, veld, accd) || !params || misaligned8(params) || !acc_out || misaligned8(acc_out) || !jerk_out ||
      misaligned8(jerk_out) || !snap_out || misaligned8(snap_out))
    return NBD_E_BADARG;
  if (bad_workspace(workspace, workspace_bytes, t)) return NBD_E_WORKSPACE;
  return launch_force_finish(dev_plan(plan, t), t, const_cast<double*>(posd), veld, accd, params, nullptr, nullptr,
                             nullptr, nullptr, nullptr, acc_out, jerk_out, snap_out, nullptr, nullptr, workspace,
                             (hipStream_t)stream);
}

int nbd_batch_hermite6_step_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, double* pos,
                                double* vel, const double* acc_in, const double* jerk_in, const double* snap_in,
                                const double* crackle_in, double* acc_out, double* jerk_out, double* snap_out,
                                double* crackle_out, const double* mass, const double* params, double* posd,
                                double* veld, double* accd, void* workspace, size_t workspace_bytes,
                                nbd_stream_t stream) {
  BatchTotals t;
  int rc = prologue_f64<kOut>(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc) return rc;
  if (t.n_total == 0) return 0;
  if (!pos || !vel || !acc_in || !jerk_in || !snap_in || !crackle_in || !mass || !params || misaligned8(params) ||
      !acc_out || misaligned8(acc_out) || !jerk_out || misaligned8(jerk_out) || !snap_out || misaligned8(snap_out) ||
      !crackle_out || misaligned8(crackle_out) || bad_rows(posd, veld, accd))
    return NBD_E_BADARG;
  if (bad_workspace(workspace, workspace_bytes, t)) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const DevPlan d = dev_plan(plan, t);
  if ((rc = launch_predict(d, t, pos, vel, acc_in, jerk_in, snap_in, crackle_in, mass, params, posd, veld, accd, st)))
    return rc;
  return launch_force_finish(d, t, posd, veld, accd, params, pos, vel, acc_in, jerk_in, snap_in, acc_out, jerk_out,
                             snap_out, crackle_out, mass, workspace, st);
}

}  // extern "C"
