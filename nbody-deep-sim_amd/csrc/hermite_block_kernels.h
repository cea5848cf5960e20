// hermite_block_kernels.h -- what the two block-timestep translation units share (direct_hermite_block.hip: fp32 state;
// direct_hermite_block_f64.hip: fp64 state): the layout of the schedule record, and the level arithmetic (criterion,
// wanted_level, norm3). Levels, ticks and the schedule are integers and the criterion is evaluated in fp64 in both modes,
// so there is one copy of each; the scheduler itself (hblock_schedule_kernel, direct_hermite_block.hip) looks at nothing
// else and serves both.
// The definitions sit in an anonymous namespace: every translation unit that includes this file gets its own inlined copies.
#pragma once
#include <math.h>

#include "direct_kernels.h"

namespace {

constexpr int kMaxLevel = 20;        // 2^20 ticks per interval: the tick count fits an int32 with room for t_i + d_i

// sched[NBD_HBLOCK_SCHED_INTS]: t_next and n_act of the block step being taken, the cumulative clamp count, the tick T
// every body has reached (the last t_next, 0 at the start of an interval), the compaction's write cursor and its count
// of finished workgroups (both 0 between launches), and the level histogram (bin k: bodies at level k)
enum { kTNext = 0, kNAct = 1, kClamped = 2, kTCur = 3, kCursor = 4, kDone = 5, kHist = 8 };
static_assert(kHist + kMaxLevel + 1 <= NBD_HBLOCK_SCHED_INTS, "sched holds the level histogram");

inline bool bad_level(int K) { return K < 0 || K > kMaxLevel; }

// The Aarseth criterion sqrt(eta num / den). den = 0 (no jerk and no higher derivative: a lone body, or one in a
// uniform field) allows any step: +inf, not the NaN of 0/0. A NaN that comes from NaN forces stays NaN (clamped).
__device__ __forceinline__ double criterion(double eta, double num, double den) {
  return den == 0.0 ? INFINITY : sqrt(eta * num / den);
}

// The level a criterion value asks for: the smallest k >= 0 with dt 2^-k <= crit, compared against the exact powers of
// two. K + 1 means "deeper than K" (also for NaN, which no comparison accepts); +inf gives 0.
__device__ __forceinline__ int wanted_level(double crit, double dt, int K) {
  int k = 0;
  double step = dt;
  while (k <= K && !(step <= crit)) {
    ++k;
    step *= 0.5;
  }
  return k;
}

__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

}  // namespace
