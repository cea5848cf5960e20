// hermite_orders_f64.h -- the two orders of the float64 Hermite family as types, for every translation unit that evaluates
// either one: the shared step (direct_hermite_f64.hip: one system; direct_batch_hermite_f64.hip: many), the sharded step
// (direct_hermite_shard_f64.hip) and the block-timestep units (direct_hermite_block_f64.hip,
// direct_batch_hermite_block_f64.hip). Order4, Order6: the pair functor, the arrays it streams, the residency the gathered
// block kernel is bound to, the functor of a target. Every unit's force kernel is a prologue and one walk_f64 with
// Order::make's functor, so a scene of a batch, a rank that owns every body and a block step that lists every body have the
// one-system shared step's bits. The definitions sit in an anonymous namespace: every translation unit that includes this
// file gets its own inlined copies.
#pragma once
#include "direct_kernels.h"
#include "hermite6_f64_kernels.h"
#include "hermite_f64_kernels.h"

namespace {

// An order: its pair functor, the d4 arrays the functor streams (= the pieces of a sharded rank's exchanged row), the
// workgroups per CU the gathered block kernel is bound to (the all-bodies kernels take no such bound), and the functor of
// the target with index i, loaded from row `row` of those arrays (accd: the 6th order's third; the 4th is handed anything
// and never reads it). The all-bodies kernels pass Group64's row and i, which differ for the lanes behind n; the gathered
// kernels pass the listed body for both; the sharded kernel, whose arrays are the pieces of one interleaved row, passes
// tgt, tgt + 1, tgt + 2 and the row scaled by kArr.
struct Order4 {
  using Pair = AccelJerkPair;
  static constexpr int kArr = 2;                   // {x_p, m}, {v_p, 0}
  static constexpr int kMinWG = 5;
  static __device__ __forceinline__ Pair make(const d4* __restrict__ posd, const d4* __restrict__ veld,
                                              const d4* __restrict__, size_t row, int i, double eps2, int n) {
    return Pair(posd[row], veld[row], eps2, i, n);
  }
};

struct Order6 {
  using Pair = AccelJerkSnapPair;
  static constexpr int kArr = 3;                   // {x_p, m}, {v_p, 0}, {a_p, 0}
  static constexpr int kMinWG = 1;
  static __device__ __forceinline__ Pair make(const d4* __restrict__ posd, const d4* __restrict__ veld,
                                              const d4* __restrict__ accd, size_t row, int i, double eps2, int n) {
    return Pair(posd[row], veld[row], accd[row], eps2, i, n);
  }
};

// the packed source arrays of an order are missing or off their 32 bytes (accd is looked at by the 6th only)
template <class Order>
bool bad_rows(const double* posd, const double* veld, const double* accd) {
  return !posd || !veld || misaligned32(posd) || misaligned32(veld) ||
         (Order::kArr == 3 && (!accd || misaligned32(accd)));
}

}  // namespace
