// direct_batch_plan.h -- the device work list of the batched direct integrator (nbd_batch_plan / nbd_batch_plan_fill)
// and the host checks every batched entry point makes before it launches, shared by direct_batch.hip (leapfrog, Euler,
// energies) and direct_batch_hermite.hip (Hermite). The definitions sit in an anonymous namespace: every translation
// unit that includes this file gets its own copies.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_kernels.h"

namespace {

// scene record of the device plan (8 ints, two int4 loads)
struct SceneRec {
  int off;      // first body of the scene in pos / vel / acc / mass
  int n;        // bodies
  int poff;     // first packed row (multiple of 64)
  int ws_off;   // first float of the scene's slabs in the workspace: float[slabs][n][3]
  int u_off;    // first fp64 energy partial of the scene: double[groups * slabs]
  int slabs;
  int n_chunks; // pad64(n) / 64
  int groups;   // ceil(n / 128)
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

struct BatchTotals {
  int n_scenes, n_items, n_total, n_rows;   // rows = packed rows (sum of pad64(n_s))
  int64_t ws_floats, u_doubles;
};

// Validates host offsets (offsets[0] == 0, non-decreasing) and sums the plan's sizes. Returns 0 or NBD_E_*.
int batch_totals(const int* offsets, int n_scenes, BatchTotals* t) {
  if (!offsets || n_scenes <= 0 || offsets[0] != 0) return NBD_E_BADARG;
  int64_t items = 0, rows = 0, ws = 0, ud = 0;
  for (int s = 0; s < n_scenes; ++s) {
    const int n = offsets[s + 1] - offsets[s];
    if (offsets[s + 1] < offsets[s] || offsets[s + 1] < 0) return NBD_E_BADARG;
    if (n == 0) continue;
    const int slabs = scene_slabs(n), groups = ceil_div(n, kTgtPerWG);
    items += (int64_t)groups * slabs;
    rows += (int64_t)ceil_div(n, kChunk) * kChunk;
    ws += (int64_t)slabs * n * 3;
    ud += (int64_t)groups * slabs;
  }
  if (items > INT_MAX || rows > INT_MAX / 4 || ws > INT_MAX || ud > INT_MAX) return NBD_E_UNSUPPORTED;
  t->n_scenes = n_scenes; t->n_items = (int)items; t->n_total = offsets[n_scenes]; t->n_rows = (int)rows;
  t->ws_floats = ws; t->u_doubles = ud;
  return 0;
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

// common argument checks of the launching entry points; fills t
int batch_prologue(const int* offsets, int n_scenes, const void* plan, size_t plan_bytes, BatchTotals* t) {
  int rc = batch_totals(offsets, n_scenes, t);
  if (rc) return rc;
  if (!plan || misaligned16(plan) || plan_bytes != plan_bytes_of(*t)) return NBD_E_BADARG;
  return 0;
}

}  // namespace
