// direct_batch_hermite_f64.hip -- direct_hermite_f64.hip's double-precision Hermite steps (4th and 6th order) and
// diagnostics, applied to every scene of an ensemble of independent systems by one set of launches (gfx950):
// direct_batch_hermite.hip in the number format of direct_hermite_f64.hip. C-ABI: the nbd_batch_*_f64 entries of
// include/nbd.h; Python: galaxify.simulation.BatchedSimulator(integrator="hermite", dtype=torch.float64) and
// BatchedSimulator(integrator="hermite6").
//
// The scenes lie back to back as in direct_batch.hip; the packed rows are posd = {x, y, z, m}, veld = {vx, vy, vz, 0} and,
// at the 6th order, accd = {ax, ay, az, 0}, d4 each, every scene padded to whole chunks of 64 rows with zero rows. The work
// list has the layout of the fp32 plan (direct_batch_plan.h: items, scene records, row_scene) but its own contents: one
// item per (scene, group of 64 targets, slab), the geometry of a scene being plan_f64(n_s) -- the one-system launch of
// direct_hermite_f64.hip for its size, a function of n_s alone -- and ws_off the first DOUBLE of the scene's
// double[slabs][kOut][n_s] partial sums, kOut = 6 resp. 9. The items, rows and bytes of the two orders' plans are the
// same, so the diagnostic entries run on either (they read ws_off and use the front of a scene's region).
//
// Every per-scene scalar comes from ONE device table of doubles, par[rows][S] (rows: ParamRow below: G, eps^2, eps, then
// the order's step constants), which the caller forms on the host by the expressions of the one-system path; no kernel
// takes a per-scene scalar by value, so a step can be captured into a graph and a changed dt, softening or G is a rewrite
// of the table. One step is three launches:
//   predict  : one thread per packed row. 4th: batch_hermite_predict_kernel<double> (hermite_batch_kernels.h, shared with
//              the fp32 unit) on rows kStep.. of par; 6th: hermite6_predict_row with the scene's constants
//   evaluate : one workgroup per item: batch_force_f64_kernel<Order>: Order::make's functor + walk_f64 on the scene's rows,
//              the chunks of wave 4 k + w under the scene's own balanced split; unscaled partial sums into the scene's
//              double[slabs][kOut][n_s]
//   finish   : one thread per packed row. 4th: batch_hermite_correct_kernel<double> (the same header) on rows kG and
//              kStep.. of par: hermite_slab_sum (slab order) x G_s, hermite_correct_row, posd = {x1, m};
//              6th: hermite6_finish_row (slab order, x G_s, corrector, crackle), posd = {x1, m}
// and the diagnostics walk the same items with EnergyPair / PotentialPair and finish per scene. Every kernel here is a
// prologue that reads its geometry and calls the single copies of the arithmetic (hermite_kernels.h,
// hermite_f64_kernels.h, hermite6_f64_kernels.h): a scene's results are bit-identical to the one-system entries on that
// scene alone. No atomics, no memsets, no host syncs: deterministic with a workspace that may hold anything.
// Resources (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage): batch_force_f64_kernel<Order4>: 89
// VGPRs, 32 KiB of LDS, 5 waves per SIMD; <Order6>: 164 VGPRs, 48 KiB, 3 waves per SIMD -- force_f64_kernel<Order>'s
// figures. batch_hermite_predict_kernel<double>: 32 VGPRs; batch_hermite_correct_kernel<double>: 46;
// batch_hermite6_predict_kernel: 52; batch_hermite6_finish_kernel: 68. No spills and no scratch anywhere.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_batch_plan.h"
#include "direct_kernels.h"
#include "hermite6_f64_kernels.h"
#include "hermite_batch_kernels.h"
#include "hermite_f64_kernels.h"
#include "hermite_kernels.h"
#include "hermite_orders_f64.h"

namespace {

// rows of the per-scene parameter tables par[rows][S]: G, eps^2, eps at either order (so the diagnostics read both), then
// the order's own step constants from row kStep on
enum ParamRow {
  kG = 0, kEps2, kEps, kStep,
  kParams4 = kStep + HermiteStepRow::kRows,                              // 4th: HermiteStep<double>'s, HermiteStepRow
  kParams6 = kStep + (int)(sizeof(Hermite6Step) / sizeof(double))        // 6th: Hermite6Step's members in its order
};
static_assert(kParams4 == NBD_BATCH_F64_PARAM_ROWS, "the table include/nbd.h describes");
static_assert(kParams6 == NBD_BATCH_H6_PARAM_ROWS, "the table include/nbd.h describes");

// the scene's step constants, member k of Hermite6Step from row kStep + k
__device__ __forceinline__ Hermite6Step load_step(const double* __restrict__ par, int n_scenes, int s) {
  const double* p = par + (size_t)kStep * n_scenes + s;
  const size_t S = (size_t)n_scenes;
  return Hermite6Step{p[0], p[S], p[2 * S], p[3 * S], p[4 * S], p[5 * S], p[6 * S], p[7 * S], p[8 * S], p[9 * S]};
}

// the plan counted in doubles (direct_batch_plan.h) with the scene's slabs double[slabs][kOut][n]: the 4th order's, and what
// the diagnostics check a plan of either order against (its items, rows and bytes do not depend on kOut)
constexpr int kOut = Order4::Pair::kOut;

// One workgroup per item (s, g, k): force_f64_kernel<Order>'s prologue (direct_hermite_f64.hip) read from the scene record
// -- targets [64 g, 64 g + 64) of scene s, the chunks of wave 4 k + w under chunk_split(n_chunks, slabs) of the scene --
// then the same walk_f64. accd: the 6th order's third array, not read at the 4th. out: the scene's double[slabs][kOut][n]
// at ws + ws_off.
template <class Order>
__global__ __launch_bounds__(64 * kWaves) void batch_force_f64_kernel(
    const d4* __restrict__ posd, const d4* __restrict__ veld, const d4* __restrict__ accd,
    const int4* __restrict__ items, const SceneRec* __restrict__ scenes, const double* __restrict__ par, int n_scenes,
    double* __restrict__ ws) {
  using Pair = typename Order::Pair;
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads_n<Order::kArr>()];
  const Item w = load_item(items, scenes);
  const double eps2 = par[kEps2 * n_scenes + w.s];
  const d4* pd = posd + w.poff;
  const d4* vd = veld + w.poff;
  const d4* ad = Order::kArr == 3 ? accd + w.poff : nullptr;
  const Group64<int> g(w.grp, w.slab, w.n);
  const ChunkRange c = wave_chunks_of(g.jw(), w.n_chunks, w.slabs);
  Pair pr = Order::make(pd, vd, ad, g.row(), g.i, eps2, w.n);
  walk_f64(pr, pd, vd, c.begin, c.end, eps2 < kEps2MaskedF64, w.grp, lds, g.dst<Pair>(ws + (size_t)w.ws_off), (size_t)w.n,
           g.n_valid(), nullptr, ad);
}

// ---- the 6th order's O(N) kernels

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

// ---- diagnostics. Their partial sums are double[slabs][n] per scene, at the scene's ws_off (the front of its
// double[slabs][6][n]).

// energy_f64_kernel's prologue per item: group g walks the chunks [g, n_chunks) of its scene, split over slabs x 4 waves.
__global__ __launch_bounds__(64 * kWaves) void batch_energy_f64_kernel(const d4* __restrict__ posd,
                                                                       const int4* __restrict__ items,
                                                                       const SceneRec* __restrict__ scenes,
                                                                       const double* __restrict__ par, int n_scenes,
                                                                       double* __restrict__ ws) {
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads<false>()];
  const Item w = load_item(items, scenes);
  const double soft = par[kEps * n_scenes + w.s];
  const d4* pd = posd + w.poff;
  const Group64<int> g(w.grp, w.slab, w.n);
  const ChunkRange c = wave_chunks_upper(g.jw(), w.n_chunks, w.grp, w.slabs);
  EnergyPair pr(pd[g.row()], soft, g.i, w.n);
  walk_f64(pr, pd, pd, c.begin + w.grp, c.end + w.grp, true, w.grp, lds, g.dst<EnergyPair>(ws + (size_t)w.ws_off),
           (size_t)w.n, g.n_valid());
}

// one workgroup per scene: out_uk[s] = {U_s, K_s} (energy_finish_f64; an empty scene gives {0, 0})
__global__ __launch_bounds__(kSumThreads) void batch_energy_finish_f64_kernel(const SceneRec* __restrict__ scenes,
                                                                              const double* __restrict__ ws,
                                                                              const d4* __restrict__ posd,
                                                                              const double* __restrict__ vel,
                                                                              const double* __restrict__ par,
                                                                              int n_scenes, double* __restrict__ out_uk) {
  __shared__ double red[2][kSumWaves];
  const int s = blockIdx.x;
  const SceneRec sc = load_scene(scenes, s);
  energy_finish_f64(ws + (size_t)sc.ws_off, sc.slabs, sc.n, posd + sc.poff, vel + (size_t)sc.off * 3,
                    par[kG * n_scenes + s], out_uk + 2 * (size_t)s, red);
}

// potential_f64_kernel's prologue per item
__global__ __launch_bounds__(64 * kWaves) void batch_potential_f64_kernel(const d4* __restrict__ posd,
                                                                          const int4* __restrict__ items,
                                                                          const SceneRec* __restrict__ scenes,
                                                                          const double* __restrict__ par, int n_scenes,
                                                                          double* __restrict__ ws) {
  __shared__ __attribute__((aligned(32))) f4 lds[kWaves * stage_quads<false>()];
  const Item w = load_item(items, scenes);
  const double eps2 = par[kEps2 * n_scenes + w.s];
  const d4* pd = posd + w.poff;
  const Group64<int> g(w.grp, w.slab, w.n);
  const ChunkRange c = wave_chunks_of(g.jw(), w.n_chunks, w.slabs);
  PotentialPair pr(pd[g.row()], eps2, g.i, w.n);
  walk_f64(pr, pd, pd, c.begin, c.end, eps2 < kEps2MaskedF64, w.grp, lds, g.dst<PotentialPair>(ws + (size_t)w.ws_off),
           (size_t)w.n, g.n_valid());
}

// phi[off_s + i] = potential_finish_f64 of body i of its scene: one thread per packed row
__global__ __launch_bounds__(256) void batch_potential_finish_f64_kernel(const int* __restrict__ row_scene,
                                                                         const SceneRec* __restrict__ scenes,
                                                                         int n_rows, const double* __restrict__ ws,
                                                                         const double* __restrict__ par, int n_scenes,
                                                                         double* __restrict__ phi) {
  PlanRow w;
  if (!load_row(row_scene, scenes, n_rows, w) || w.i() >= w.sc.n) return;
  phi[(size_t)w.sc.off + w.i()] =
      potential_finish_f64(ws + (size_t)w.sc.ws_off, w.sc.slabs, w.sc.n, w.i(), par[kG * n_scenes + w.s]);
}

// one workgroup per scene: invariants_state_f64_kernel's body on the scene's part of the state
__global__ __launch_bounds__(kInvThreads) void batch_invariants_state_f64_kernel(const SceneRec* __restrict__ scenes,
                                                                                 const double* __restrict__ pos,
                                                                                 const double* __restrict__ vel,
                                                                                 const double* __restrict__ mass,
                                                                                 const double* __restrict__ phi,
                                                                                 double* __restrict__ rows) {
  __shared__ double red[kInvSums][kInvWaves];
  const SceneRec sc = load_scene(scenes, blockIdx.x);
  const size_t off = (size_t)sc.off;
  invariants_body(F64State{pos + 3 * off, vel + 3 * off, mass + off}, phi + off, sc.n,
                  rows + (size_t)blockIdx.x * 16, red);
}

// ---- the host bodies of the force and step entries. args_ok: what the entry found of its own pointer list.

// What a force or step entry refuses, before the first launch; t->n_total == 0 with 0: nothing to do.
template <class Order>
int batch_refusals(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, bool args_ok,
                   const double* posd, const double* veld, const double* accd, const double* params,
                   const void* workspace, size_t workspace_bytes, BatchTotals* t) {
  const int rc = prologue_f64<Order::Pair::kOut>(offsets, n_scenes, plan, plan_bytes, t);
  if (rc || t->n_total == 0) return rc;
  if (!args_ok || bad_rows<Order>(posd, veld, accd) || !params || misaligned8(params)) return NBD_E_BADARG;
  return bad_workspace(workspace, workspace_bytes, *t) ? NBD_E_WORKSPACE : 0;
}

// the force of every scene at the packed rows, then finish(plan, totals, ws, stream), the entry's finishing launch: the
// slab sum (+ the corrector when the entry has a state)
template <class Order, class Finish>
int launch_force_finish(const DevPlan& d, const BatchTotals& t, const double* posd, const double* veld,
                        const double* accd, const double* par, void* workspace, hipStream_t st, Finish finish) {
  double* ws = static_cast<double*>(workspace);
  batch_force_f64_kernel<Order><<<t.n_items, 64 * kWaves, 0, st>>>(
      reinterpret_cast<const d4*>(posd), reinterpret_cast<const d4*>(veld), reinterpret_cast<const d4*>(accd), d.items,
      d.scenes, par, t.n_scenes, ws);
  const int rc = launch_status();
  if (rc) return rc;
  finish(d, t, ws, st);
  return launch_status();
}

// The force of packed rows on its own.
template <class Order, class Finish>
int batch_force(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, bool args_ok, const double* posd,
                const double* veld, const double* accd, const double* params, void* workspace, size_t workspace_bytes,
                nbd_stream_t stream, Finish finish) {
  BatchTotals t;
  const int rc = batch_refusals<Order>(offsets, n_scenes, plan, plan_bytes, args_ok, posd, veld, accd, params, workspace,
                                       workspace_bytes, &t);
  if (rc || t.n_total == 0) return rc;
  return launch_force_finish<Order>(dev_plan(plan, t), t, posd, veld, accd, params, workspace, (hipStream_t)stream,
                                    finish);
}

// predict(plan, totals, stream), the entry's predictor (or plain pack) launch, then the force of the rows it wrote.
template <class Order, class Predict, class Finish>
int batch_step(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, bool args_ok, const double* posd,
               const double* veld, const double* accd, const double* params, void* workspace, size_t workspace_bytes,
               nbd_stream_t stream, Predict predict, Finish finish) {
  BatchTotals t;
  int rc = batch_refusals<Order>(offsets, n_scenes, plan, plan_bytes, args_ok, posd, veld, accd, params, workspace,
                                 workspace_bytes, &t);
  if (rc || t.n_total == 0) return rc;
  hipStream_t st = (hipStream_t)stream;
  const DevPlan d = dev_plan(plan, t);
  predict(d, t, st);
  if ((rc = launch_status())) return rc;
  return launch_force_finish<Order>(d, t, posd, veld, accd, params, workspace, st, finish);
}

// the predictor launches (acc resp. jerk == nullptr: a plain pack, par not read) and the finishing launches
// (pos == nullptr: the force on its own) of the two orders, as the entries' lambdas call them
void predict4(const DevPlan& d, const BatchTotals& t, const double* pos, const double* vel, const double* acc,
              const double* jerk, const double* mass, const double* par, double* posd, double* veld, hipStream_t st) {
  batch_hermite_predict_kernel<double><<<ceil_div(t.n_rows, 256), 256, 0, st>>>(
      d.row_scene, d.scenes, t.n_rows, pos, vel, acc, jerk, mass, par ? par + (size_t)kStep * t.n_scenes : nullptr,
      t.n_scenes, reinterpret_cast<d4*>(posd), reinterpret_cast<d4*>(veld));
}

void predict6(const DevPlan& d, const BatchTotals& t, const double* pos, const double* vel, const double* acc,
              const double* jerk, const double* snap, const double* crackle, const double* mass, const double* par,
              double* posd, double* veld, double* accd, hipStream_t st) {
  batch_hermite6_predict_kernel<<<ceil_div(t.n_rows, 256), 256, 0, st>>>(
      d.row_scene, d.scenes, t.n_rows, pos, vel, acc, jerk, snap, crackle, mass, par, t.n_scenes,
      reinterpret_cast<d4*>(posd), reinterpret_cast<d4*>(veld), reinterpret_cast<d4*>(accd));
}

void finish4(const DevPlan& d, const BatchTotals& t, const double* ws, const double* par, double* pos, double* vel,
             const double* acc_in, const double* jerk_in, double* acc_out, double* jerk_out, const double* mass,
             double* posd, hipStream_t st) {
  batch_hermite_correct_kernel<double><<<ceil_div(t.n_rows, HermiteFmt<double>::kSumRows), 256, 0, st>>>(
      d.row_scene, d.scenes, t.n_rows, ws, par + (size_t)kG * t.n_scenes, par + (size_t)kStep * t.n_scenes, t.n_scenes,
      pos, vel, acc_in, jerk_in, acc_out, jerk_out, mass, reinterpret_cast<d4*>(posd));
}

void finish6(const DevPlan& d, const BatchTotals& t, const double* ws, const double* par, double* pos, double* vel,
             const double* acc_in, const double* jerk_in, const double* snap_in, double* acc_out, double* jerk_out,
             double* snap_out, double* crackle_out, const double* mass, double* posd, hipStream_t st) {
  batch_hermite6_finish_kernel<<<ceil_div(t.n_rows, 256), 256, 0, st>>>(
      d.row_scene, d.scenes, t.n_rows, ws, par, t.n_scenes, pos, vel, acc_in, jerk_in, snap_in, acc_out, jerk_out,
      snap_out, crackle_out, mass, reinterpret_cast<d4*>(posd));
}

// an output array of a force or step entry is there and on its 8 bytes
inline bool ok8(const double* p) { return p && !misaligned8(p); }

}  // namespace

extern "C" {

int nbd_batch_f64_plan(const int* offsets, int n_scenes, int* n_items, int* rows, size_t* plan_bytes) {
  BatchTotals t;
  const int rc = batch_totals_f64<kOut>(offsets, n_scenes, &t);
  if (rc) return rc;
  if (n_items) *n_items = t.n_items;
  if (rows) *rows = t.n_rows;
  if (plan_bytes) *plan_bytes = plan_bytes_of(t);
  return 0;
}

int nbd_batch_f64_workspace_bytes(const int* offsets, int n_scenes, size_t* bytes) {
  return workspace_bytes_f64<kOut>(offsets, n_scenes, bytes);
}

int nbd_batch_f64_plan_fill(const int* offsets, int n_scenes, void* plan, size_t plan_bytes) {
  return plan_fill_f64<kOut>(offsets, n_scenes, plan, plan_bytes);
}

int nbd_batch_hermite6_f64_plan_fill(const int* offsets, int n_scenes, void* plan, size_t plan_bytes) {
  return plan_fill_f64<Order6::Pair::kOut>(offsets, n_scenes, plan, plan_bytes);
}

int nbd_batch_hermite6_f64_workspace_bytes(const int* offsets, int n_scenes, size_t* bytes) {
  return workspace_bytes_f64<Order6::Pair::kOut>(offsets, n_scenes, bytes);
}

int nbd_batch_pack_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const double* pos,
                       const double* vel, const double* mass, double* posd, double* veld, nbd_stream_t stream) {
  BatchTotals t;
  const int rc = prologue_f64<kOut>(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc || t.n_total == 0) return rc;
  if (!pos || !vel || !mass || bad_rows<Order4>(posd, veld, nullptr)) return NBD_E_BADARG;
  predict4(dev_plan(plan, t), t, pos, vel, nullptr, nullptr, mass, nullptr, posd, veld, (hipStream_t)stream);
  return launch_status();
}

int nbd_batch_hermite6_pack_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const double* pos,
                                const double* vel, const double* acc, const double* mass, double* posd, double* veld,
                                double* accd, nbd_stream_t stream) {
  BatchTotals t;
  const int rc = prologue_f64<Order6::Pair::kOut>(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc || t.n_total == 0) return rc;
  if (!pos || !vel || !mass || bad_rows<Order6>(posd, veld, accd)) return NBD_E_BADARG;
  predict6(dev_plan(plan, t), t, pos, vel, acc, nullptr, nullptr, nullptr, mass, nullptr, posd, veld, accd,
           (hipStream_t)stream);
  return launch_status();
}

int nbd_batch_accel_jerk_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const double* pos,
                             const double* vel, const double* mass, const double* params, double* acc_out,
                             double* jerk_out, double* posd, double* veld, void* workspace, size_t workspace_bytes,
                             nbd_stream_t stream) {
  return batch_step<Order4>(
      offsets, n_scenes, plan, plan_bytes, pos && vel && mass && ok8(acc_out) && ok8(jerk_out), posd, veld, nullptr,
      params, workspace, workspace_bytes, stream,
      [=](const DevPlan& d, const BatchTotals& t, hipStream_t st) {
        predict4(d, t, pos, vel, nullptr, nullptr, mass, nullptr, posd, veld, st);
      },
      [=](const DevPlan& d, const BatchTotals& t, const double* ws, hipStream_t st) {
        finish4(d, t, ws, params, nullptr, nullptr, nullptr, nullptr, acc_out, jerk_out, nullptr, posd, st);
      });
}

int nbd_batch_accel_jerk_snap_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes,
                                  const double* posd, const double* veld, const double* accd, const double* params,
                                  double* acc_out, double* jerk_out, double* snap_out, void* workspace,
                                  size_t workspace_bytes, nbd_stream_t stream) {
  return batch_force<Order6>(
      offsets, n_scenes, plan, plan_bytes, ok8(acc_out) && ok8(jerk_out) && ok8(snap_out), posd, veld, accd, params,
      workspace, workspace_bytes, stream, [=](const DevPlan& d, const BatchTotals& t, const double* ws, hipStream_t st) {
        finish6(d, t, ws, params, nullptr, nullptr, nullptr, nullptr, nullptr, acc_out, jerk_out, snap_out, nullptr,
                nullptr, const_cast<double*>(posd), st);
      });
}

int nbd_batch_hermite_step_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, double* pos,
                               double* vel, const double* acc_in, const double* jerk_in, double* acc_out,
                               double* jerk_out, const double* mass, const double* params, double* posd, double* veld,
                               void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  return batch_step<Order4>(
      offsets, n_scenes, plan, plan_bytes, pos && vel && acc_in && jerk_in && mass && ok8(acc_out) && ok8(jerk_out),
      posd, veld, nullptr, params, workspace, workspace_bytes, stream,
      [=](const DevPlan& d, const BatchTotals& t, hipStream_t st) {
        predict4(d, t, pos, vel, acc_in, jerk_in, mass, params, posd, veld, st);
      },
      [=](const DevPlan& d, const BatchTotals& t, const double* ws, hipStream_t st) {
        finish4(d, t, ws, params, pos, vel, acc_in, jerk_in, acc_out, jerk_out, mass, posd, st);
      });
}

int nbd_batch_hermite6_step_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, double* pos,
                                double* vel, const double* acc_in, const double* jerk_in, const double* snap_in,
                                const double* crackle_in, double* acc_out, double* jerk_out, double* snap_out,
                                double* crackle_out, const double* mass, const double* params, double* posd,
                                double* veld, double* accd, void* workspace, size_t workspace_bytes,
                                nbd_stream_t stream) {
  return batch_step<Order6>(
      offsets, n_scenes, plan, plan_bytes,
      pos && vel && acc_in && jerk_in && snap_in && crackle_in && mass && ok8(acc_out) && ok8(jerk_out) &&
          ok8(snap_out) && ok8(crackle_out),
      posd, veld, accd, params, workspace, workspace_bytes, stream,
      [=](const DevPlan& d, const BatchTotals& t, hipStream_t st) {
        predict6(d, t, pos, vel, acc_in, jerk_in, snap_in, crackle_in, mass, params, posd, veld, accd, st);
      },
      [=](const DevPlan& d, const BatchTotals& t, const double* ws, hipStream_t st) {
        finish6(d, t, ws, params, pos, vel, acc_in, jerk_in, snap_in, acc_out, jerk_out, snap_out, crackle_out, mass,
                posd, st);
      });
}

int nbd_batch_energies_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const double* posd,
                           const double* vel, const double* params, double* out_uk, void* workspace,
                           size_t workspace_bytes, nbd_stream_t stream) {
  BatchTotals t;
  int rc = prologue_f64<kOut>(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc) return rc;
  if (!out_uk || misaligned8(out_uk) || !params || misaligned8(params)) return NBD_E_BADARG;
  if (t.n_total > 0 && (!posd || !vel || misaligned32(posd))) return NBD_E_BADARG;
  if (t.n_total > 0 && bad_workspace(workspace, workspace_bytes, t)) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const DevPlan d = dev_plan(plan, t);
  const d4* pd = reinterpret_cast<const d4*>(posd);
  double* ws = static_cast<double*>(workspace);
  if (t.n_items > 0) {
    batch_energy_f64_kernel<<<t.n_items, 64 * kWaves, 0, st>>>(pd, d.items, d.scenes, params, n_scenes, ws);
    if ((rc = launch_status())) return rc;
  }
  batch_energy_finish_f64_kernel<<<n_scenes, kSumThreads, 0, st>>>(d.scenes, ws, pd, vel, params, n_scenes, out_uk);
  return launch_status();
}

int nbd_batch_potential_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, const double* posd,
                            const double* params, double* phi_out, void* workspace, size_t workspace_bytes,
                            nbd_stream_t stream) {
  BatchTotals t;
  int rc = prologue_f64<kOut>(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc) return rc;
  if (t.n_total == 0) return 0;
  if (!posd || misaligned32(posd) || !params || misaligned8(params) || !phi_out || misaligned8(phi_out))
    return NBD_E_BADARG;
  if (bad_workspace(workspace, workspace_bytes, t)) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const DevPlan d = dev_plan(plan, t);
  double* ws = static_cast<double*>(workspace);
  batch_potential_f64_kernel<<<t.n_items, 64 * kWaves, 0, st>>>(reinterpret_cast<const d4*>(posd), d.items, d.scenes,
                                                                params, n_scenes, ws);
  if ((rc = launch_status())) return rc;
  batch_potential_finish_f64_kernel<<<ceil_div(t.n_rows, 256), 256, 0, st>>>(d.row_scene, d.scenes, t.n_rows, ws, params,
                                                                             n_scenes, phi_out);
  return launch_status();
}

int nbd_batch_invariants_state_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes,
                                   const double* pos, const double* vel, const double* mass, const double* phi,
                                   double* out_rows, nbd_stream_t stream) {
  BatchTotals t;
  const int rc = prologue_f64<kOut>(offsets, n_scenes, plan, plan_bytes, &t);
  if (rc) return rc;
  if (!out_rows || misaligned8(out_rows)) return NBD_E_BADARG;
  if (t.n_total > 0 && (!pos || !vel || !mass || !phi || misaligned8(phi))) return NBD_E_BADARG;
  batch_invariants_state_f64_kernel<<<n_scenes, kInvThreads, 0, (hipStream_t)stream>>>(
      dev_plan(plan, t).scenes, pos, vel, mass, phi, out_rows);
  return launch_status();
}

}  // extern "C"
