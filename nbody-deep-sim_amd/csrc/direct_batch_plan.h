// direct_batch_plan.h -- the device work list of the batched direct integrator (nbd_batch_plan / nbd_batch_plan_fill),
// what a kernel reads from it (load_item: one workgroup per item; load_row: one thread per packed row) and the host
// checks every batched entry point makes before it launches. Shared by direct_batch.hip (leapfrog, Euler, energies),
// direct_diag.hip (the batched diagnostics), direct_batch_hermite.hip (Hermite), direct_batch_hermite_f64.hip (Hermite in
// double precision, 4th and 6th order) and direct_batch_hermite_block_f64.hip (block
// timesteps per scene: the same layout with a static work list, a geometry of its own). The shared-timestep float64 unit fills the same layout
// with another geometry per scene (SceneGeom below); the host shell of such a plan counted in doubles -- totals, plan
// fill, workspace size and checks, for kOut doubles per body and slab -- is here once, at the end. The definitions sit in
// an anonymous namespace: every translation unit that includes this file gets its own copies.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/nbd.h"
#include "direct_kernels.h"
#include "hermite_f64_kernels.h"

namespace {

// scene record of the device plan (8 ints, two int4 loads)
struct SceneRec {
  int off;      // first body of the scene in pos / vel / acc / mass
  int n;        // bodies
  int poff;     // first packed row (multiple of 64)
  int ws_off;   // first float of the scene's slabs in the workspace: float[slabs][n][3] (fp64 plan: first double of
                // its double[slabs][6][n], or [9] in the 6th-order plan)
  int u_off;    // first fp64 energy partial of the scene: double[groups * slabs]
  int slabs;
  int n_chunks; // pad64(n) / 64
  int groups;   // ceil(n / 128) (fp64 plan: ceil(n / 64))
};

// The slab count of a scene: the single-system launch plan for its size (depends on n alone).
int scene_slabs(int n) {
  struct Memo { int n, slabs; };
  thread_local Memo memo[16] = {};
  thread_local int next = 0;
  for (const Memo& m : memo)
    if (m.n == n && m.slabs > 0) return m.slabs;
  int g = 0, s = 1, c = 0;
  if (nbd_accel_plan(n, n, &g, &s, &c) != 0 || s < 1) s = 1;
  memo[next] = {n, s};
  next = (next + 1) & 15;
  return s;
}

// What a plan gives a scene of n > 0 bodies, and all that the fp32 plan and the fp64 plans (scene_geom_f64 below: groups
// of 64 targets, plan_f64's slabs) differ in: a function int -> SceneGeom.
struct SceneGeom {
  int slabs, groups;
  int64_t ws;   // elements of the scene's slabs in the workspace, in the plan's own unit (ws_off counts them)
  int64_t u;    // fp64 energy partials of the scene (u_off counts them)
};

// The fp32 plan: groups of 128 targets, float[slabs][n][3], one energy partial per item.
inline SceneGeom scene_geom_f32(int n) {
  const int slabs = scene_slabs(n), groups = ceil_div(n, kTgtPerWG);
  return SceneGeom{slabs, groups, (int64_t)slabs * n * 3, (int64_t)groups * slabs};
}

struct BatchTotals {
  int n_scenes, n_items, n_total, n_rows;   // rows = packed rows (sum of pad64(n_s))
  int64_t ws_floats, u_doubles;             // sums of SceneGeom::ws (floats in the fp32 plan) and ::u
};

// Validates host offsets (offsets[0] == 0, non-decreasing) and sums the plan's sizes. Returns 0 or NBD_E_*.
template <class Geom>
int batch_totals(const int* offsets, int n_scenes, BatchTotals* t, Geom geom) {
  if (!offsets || n_scenes <= 0 || offsets[0] != 0) return NBD_E_BADARG;
  int64_t items = 0, rows = 0, ws = 0, ud = 0;
  for (int s = 0; s < n_scenes; ++s) {
    const int n = offsets[s + 1] - offsets[s];
    if (offsets[s + 1] < offsets[s] || offsets[s + 1] < 0) return NBD_E_BADARG;
    if (n == 0) continue;
    const SceneGeom g = geom(n);
    items += (int64_t)g.groups * g.slabs;
    rows += (int64_t)ceil_div(n, kChunk) * kChunk;
    ws += g.ws;
    ud += g.u;
  }
  if (items > INT_MAX || rows > INT_MAX / 4 || ws > INT_MAX || ud > INT_MAX) return NBD_E_UNSUPPORTED;
  t->n_scenes = n_scenes; t->n_items = (int)items; t->n_total = offsets[n_scenes]; t->n_rows = (int)rows;
  t->ws_floats = ws; t->u_doubles = ud;
  return 0;
}

inline int batch_totals(const int* offsets, int n_scenes, BatchTotals* t) {
  return batch_totals(offsets, n_scenes, t, scene_geom_f32);
}

// plan layout (int32): items int4[n_items] | scenes SceneRec[n_scenes] | row_scene int[n_rows]
size_t plan_bytes_of(const BatchTotals& t) {
  return (size_t)t.n_items * 16 + (size_t)t.n_scenes * sizeof(SceneRec) + (size_t)t.n_rows * 4;
}

struct DevPlan {
  const int4* items;
  const SceneRec* scenes;
  const int* row_scene;
};
DevPlan dev_plan(const void* plan, const BatchTotals& t) {
  const char* p = static_cast<const char*>(plan);
  DevPlan d;
  d.items = reinterpret_cast<const int4*>(p);
  d.scenes = reinterpret_cast<const SceneRec*>(p + (size_t)t.n_items * 16);
  d.row_scene = reinterpret_cast<const int*>(p + (size_t)t.n_items * 16 + (size_t)t.n_scenes * sizeof(SceneRec));
  return d;
}

__device__ __forceinline__ SceneRec load_scene(const SceneRec* scenes, int s) {
  const int4* q = reinterpret_cast<const int4*>(scenes + s);
  const int4 a = q[0], b = q[1];
  return SceneRec{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
}

// What a thread that works on packed row r reads from the plan: the row's scene s and record sc, and the body
// i = r - poff of that scene (i >= sc.n: a padding row).
struct PlanRow {
  int r, s;
  SceneRec sc;
  __device__ __forceinline__ int i() const { return r - sc.poff; }
};

__device__ __forceinline__ PlanRow row_of(const int* __restrict__ row_scene, const SceneRec* __restrict__ scenes,
                                          int r) {
  PlanRow w;
  w.r = r;
  w.s = row_scene[r];
  w.sc = load_scene(scenes, w.s);
  return w;
}

// ... of a per-row kernel (256 threads per workgroup, one per packed row) into w. False behind the last row: w is not
// set and the thread leaves.
__device__ __forceinline__ bool load_row(const int* __restrict__ row_scene, const SceneRec* __restrict__ scenes,
                                         int n_rows, PlanRow& w) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return false;
  w = row_of(row_scene, scenes, r);
  return true;
}

// What a workgroup of an item reads from the work list (one workgroup per item, in every plan), uniform across the
// workgroup (SGPRs); sc is the scene's record as it was loaded, for what a kernel only adds to a pointer (u_off, and the
// fp32 units' ws_off)
struct Item {
  int s, grp, slab, n, n_chunks, slabs, poff, ws_off;
  SceneRec sc;
};

__device__ __forceinline__ Item load_item(const int4* __restrict__ items, const SceneRec* __restrict__ scenes) {
  const int4 it = items[blockIdx.x];
  Item w;
  w.s = __builtin_amdgcn_readfirstlane(it.x);
  w.grp = __builtin_amdgcn_readfirstlane(it.y);
  w.slab = __builtin_amdgcn_readfirstlane(it.z);
  w.sc = load_scene(scenes, w.s);
  w.n = __builtin_amdgcn_readfirstlane(w.sc.n);
  w.n_chunks = __builtin_amdgcn_readfirstlane(w.sc.n_chunks);
  w.slabs = __builtin_amdgcn_readfirstlane(w.sc.slabs);
  w.poff = __builtin_amdgcn_readfirstlane(w.sc.poff);
  w.ws_off = __builtin_amdgcn_readfirstlane(w.sc.ws_off);
  return w;
}

// Writes the plan of the totals t (batch_totals with the same geom) into the host buffer `plan`, plan_bytes_of(t) bytes.
template <class Geom>
void batch_plan_fill(const int* offsets, int n_scenes, const BatchTotals& t, void* plan, Geom geom) {
  std::vector<int> items;             // (scene, group, slab, chunks per wave) before ordering
  items.reserve((size_t)t.n_items * 4);
  std::vector<SceneRec> scenes(n_scenes);
  std::vector<int> rows((size_t)t.n_rows);
  int poff = 0, ws_off = 0, u_off = 0;
  for (int s = 0; s < n_scenes; ++s) {
    SceneRec& r = scenes[s];
    r.off = offsets[s]; r.n = offsets[s + 1] - offsets[s]; r.poff = poff; r.ws_off = ws_off; r.u_off = u_off;
    const SceneGeom g = r.n > 0 ? geom(r.n) : SceneGeom{0, 0, 0, 0};
    r.slabs = g.slabs;
    r.n_chunks = ceil_div(r.n, kChunk);
    r.groups = g.groups;
    const int cpw = r.n > 0 ? ceil_div(r.n_chunks, r.slabs * kWaves) : 0;
    for (int grp = 0; grp < r.groups; ++grp)
      for (int k = 0; k < r.slabs; ++k) items.insert(items.end(), {s, grp, k, cpw});
    for (int i = 0; i < r.n_chunks * kChunk; ++i) rows[(size_t)poff + i] = s;
    poff += r.n_chunks * kChunk; ws_off += (int)g.ws; u_off += (int)g.u;
  }
  // dispatch order: longest items first (a stable order of the WORK; no sum depends on it)
  std::vector<int> order(t.n_items);
  for (int i = 0; i < t.n_items; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return items[4 * a + 3] > items[4 * b + 3]; });
  int* out = static_cast<int*>(plan);
  for (int i = 0; i < t.n_items; ++i) {
    const int* src = &items[4 * order[i]];
    out[4 * i] = src[0]; out[4 * i + 1] = src[1]; out[4 * i + 2] = src[2]; out[4 * i + 3] = 0;
  }
  memcpy(out + 4 * (size_t)t.n_items, scenes.data(), scenes.size() * sizeof(SceneRec));
  memcpy(reinterpret_cast<char*>(out + 4 * (size_t)t.n_items) + scenes.size() * sizeof(SceneRec), rows.data(),
         rows.size() * sizeof(int));
}

// common argument checks of the launching entry points; fills t
template <class Geom>
int batch_prologue(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, BatchTotals* t, Geom geom) {
  int rc = batch_totals(offsets, n_scenes, t, geom);
  if (rc) return rc;
  if (!plan || misaligned16(plan) || plan_bytes != plan_bytes_of(*t)) return NBD_E_BADARG;
  return 0;
}

inline int batch_prologue(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, BatchTotals* t) {
  return batch_prologue(offsets, n_scenes, plan, plan_bytes, t, scene_geom_f32);
}

// ---- the plans counted in doubles (direct_batch_hermite_f64.hip: kOut = 6 at the 4th order, 9 at the 6th): the
// layout and the checks above with plan_f64's geometry -- one item per (scene, group of 64 targets, slab), the one-system
// float64 launch for the scene's size. The scene's slabs are double[slabs][kOut][n], counted in DOUBLES
// (BatchTotals::ws_floats, SceneRec::ws_off); no energy partials. The items, rows and bytes of the plan do not depend on
// kOut, only ws_off does.
template <int kOut>
SceneGeom scene_geom_f64(int n) {
  const F64Plan p = plan_f64(n);
  return SceneGeom{p.slabs, p.groups, (int64_t)p.slabs * kOut * n, 0};
}

template <int kOut>
int batch_totals_f64(const int* offsets, int n_scenes, BatchTotals* t) {
  return batch_totals(offsets, n_scenes, t, scene_geom_f64<kOut>);
}
inline size_t ws_bytes_f64(const BatchTotals& t) { return (size_t)t.ws_floats * sizeof(double); }
template <int kOut>
int prologue_f64(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, BatchTotals* t) {
  return batch_prologue(offsets, n_scenes, plan, plan_bytes, t, scene_geom_f64<kOut>);
}
inline bool bad_workspace(const void* workspace, size_t workspace_bytes, const BatchTotals& t) {
  return !workspace || misaligned8(workspace) || workspace_bytes < ws_bytes_f64(t);
}

// the bodies of the nbd_batch_*f64_plan_fill and nbd_batch_*f64_workspace_bytes entries
template <int kOut>
int plan_fill_f64(const int* offsets, int n_scenes, void* plan, size_t plan_bytes) {
  BatchTotals t;
  const int rc = batch_totals_f64<kOut>(offsets, n_scenes, &t);
  if (rc) return rc;
  if (!plan || plan_bytes != plan_bytes_of(t)) return NBD_E_BADARG;
  batch_plan_fill(offsets, n_scenes, t, plan, scene_geom_f64<kOut>);
  return 0;
}
template <int kOut>
int workspace_bytes_f64(const int* offsets, int n_scenes, size_t* bytes) {
  BatchTotals t;
  const int rc = batch_totals_f64<kOut>(offsets, n_scenes, &t);
  if (rc) return rc;
  if (!bytes) return NBD_E_BADARG;
  *bytes = ws_bytes_f64(t);
  return 0;
}

}  // namespace
