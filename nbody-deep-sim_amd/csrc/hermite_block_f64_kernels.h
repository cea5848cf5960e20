// hermite_block_f64_kernels.h -- what the two float64 block-timestep translation units share beyond
// hermite_block_kernels.h (direct_hermite_block_f64.hip: one system; direct_batch_hermite_block_f64.hip: many independent
// systems on one tick grid): the two orders of the scheme as types (Order4, Order6: the pair functor, the arrays it
// streams, the residency the force kernel is bound to, the functor of a gathered target). Both units' force kernels are a
// prologue and one walk_f64 with Order::make's functor, so a scene of a batch has the one-system block step's bits.
// The definitions sit in an anonymous namespace: every translation unit that includes this file gets its own inlined copies.
#pragma once
#include "direct_kernels.h"
#include "hermite6_f64_kernels.h"
#include "hermite_block_kernels.h"
#include "hermite_f64_kernels.h"

namespace {

// An order: its pair functor, the d4 arrays the functor streams, the workgroups per CU the force kernel is bound to, and
// the functor of target i from those arrays (accd: the 6th order's third; the 4th is handed nullptr and never reads it).
struct Order4 {
  using Pair = AccelJerkPair;
  static constexpr int kArr = 2;                   // {x_p, m}, {v_p, 0}
  static constexpr int kMinWG = 5;
  static __device__ __forceinline__ Pair make(const d4* __restrict__ posd, const d4* __restrict__ veld,
                                              const d4* __restrict__, int i, double eps2, int n) {
    return Pair(posd[i], veld[i], eps2, i, n);
  }
};

struct Order6 {
  using Pair = AccelJerkSnapPair;
  static constexpr int kArr = 3;                   // {x_p, m}, {v_p, 0}, {a_p, 0}
  static constexpr int kMinWG = 1;
  static __device__ __forceinline__ Pair make(const d4* __restrict__ posd, const d4* __restrict__ veld,
                                              const d4* __restrict__ accd, int i, double eps2, int n) {
    return Pair(posd[i], veld[i], accd[i], eps2, i, n);
  }
};

}  // namespace
