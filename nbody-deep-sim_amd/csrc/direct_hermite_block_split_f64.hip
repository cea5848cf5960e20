// direct_hermite_block_split_f64.hip -- a block step of direct_hermite_block_f64.hip divided over the ranks of a process
// group, float64, 4th and 6th order, for gfx950 (MI355X). An extension. C-ABI: nbd_hblock_order_list and the
// nbd_hblock_split_* / nbd_hblock6_split_* entries of include/nbd.h; Python: BlockHermiteSimulator(dtype=torch.float64,
// process_group=) and BlockHermite6Simulator(process_group=) of galaxify.simulation. DESIGN.md K-HBS.
//
// Every rank holds the whole state, bit for bit the same, and runs the scheduler and the predictor as they are. A block
// step with many active bodies is divided: the list is put in ascending body index (the scheduler's own order varies from
// run to run), rank r takes the entries [first, first + count) of it, evaluates and corrects them WITHOUT touching the
// state, and writes one result row per entry behind a header row. The pieces of all ranks are exchanged (one all-gather,
// outside this unit) and every rank applies all n_act rows alike. Launches of one divided step on a rank:
//   order : hsplit_count_kernel, hsplit_order_kernel -- the active bodies of each 256-body workgroup counted, then each
//           workgroup adds the counts before it and writes its bodies in index order. Integer work, no readback. The
//           record's t_next / n_act / cursor fields are not written.
//   rows  : hsplit_head_kernel -- the header {t_next, n_act, first, count} and the slice of the list copied to the head of
//           an ordinary block workspace; then nbd_hblock_force_f64 / nbd_hblock6_force_f64 on that workspace as it is:
//           active_force_f64_kernel<Order> and walk_f64 at plan_f64(n, count), the slice's own slab count; then
//           hsplit_rows_kernel / hsplit6_rows_kernel, one thread per entry: the slab sum, the corrector with the body's own
//           step and the criterion through the functions of the un-divided correctors (hermite_slab_sum,
//           hermite_correct_row, hblock_wanted; hermite6_finish_row, hblock6_wanted; hblock_next_level) on the thread's own
//           copy of x and v, so a row holds the bits the un-divided corrector would have stored. count = 0: the header only.
//   apply : hsplit_apply_kernel<W, A>, one thread per list entry: the row scattered into the A state arrays, posd =
//           {x1, m}, and hblock_book_level's bookkeeping (level, tick, histogram, clamp count, sched[kTCur]). Every
//           piece's header is compared with the rank's own record and with the slice the piece should hold; a mismatch
//           raises sched[kDiverged] (the state is written all the same; the simulator reads the flag at the end of the
//           interval).
// A row is W doubles, W = NBD_HBLOCK_SPLIT_ROW = 16 (x1 v1 a1 j1, three spare) resp. NBD_HBLOCK6_SPLIT_ROW = 20 (x1 v1 a1
// j1 s1 c1, one spare); its last double-sized slot holds two int32, {new level, clamped}. Spare doubles and the rest of
// the header row are written as zeros: a row buffer may hold anything beforehand.
// The workspace: the ordered list (int[n], padded to 32 bytes), the per-workgroup counts of the ordering, then an ordinary
// block workspace of the order (the slice's list and its slabs). Its head is laid out as the ordinary workspace's, so the
// scheduler and an un-divided block step run on the same buffer.
// Resources (hipcc --offload-arch=gfx950 -O3): see DESIGN.md K-HBS; no scratch, no spills, no LDS beyond the ordering's
// 1 KiB. No float atomics (the histogram and the clamp count are integer atomics), no memsets.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nbd.h"
#include "direct_kernels.h"
#include "hermite6_f64_kernels.h"
#include "hermite_block_kernels.h"
#include "hermite_f64_kernels.h"
#include "hermite_kernels.h"

namespace {

constexpr int kRow4 = NBD_HBLOCK_SPLIT_ROW, kRow6 = NBD_HBLOCK6_SPLIT_ROW;
static_assert(kDiverged > kDone && kDiverged < kHist, "the flag sits in a free int of the record");
static_assert(kRow4 % 4 == 0 && kRow6 % 4 == 0, "rows keep 32-byte alignment");

// the level from which a body is active in the block step to t_next = sched[kTNext]: d_i divides t_next
__device__ __forceinline__ int split_threshold(const int* __restrict__ sched, int K) {
  return max(0, K - __builtin_ctz(sched[kTNext]));
}

// The active bodies of this workgroup's 256: the thread's place among them (`place`) and their count (returned), by one
// ballot per wave and the four wave counts through LDS.
__device__ __forceinline__ int split_places(bool on, int& place) {
  __shared__ int wave_count[4];
  const unsigned long long mask = __ballot(on);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) wave_count[w] = __popcll(mask);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < w) before += wave_count[k];
    all += wave_count[k];
  }
  place = before + __popcll(mask & __lanemask_lt());
  return all;
}

__global__ __launch_bounds__(256) void hsplit_count_kernel(const int* __restrict__ levels, int n, int K,
                                                           const int* __restrict__ sched, int* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  int place;
  const int all = split_places(i < n && levels[i] >= split_threshold(sched, K), place);
  if (threadIdx.x == 0) counts[blockIdx.x] = all;
}

__global__ __launch_bounds__(256) void hsplit_order_kernel(const int* __restrict__ levels, int n, int K,
                                                           const int* __restrict__ sched,
                                                           const int* __restrict__ counts, int* __restrict__ act) {
  __shared__ int part[256];
  int sum = 0;
  for (int b = threadIdx.x; b < (int)blockIdx.x; b += 256) sum += counts[b];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
    __syncthreads();
  }
  const int base = part[0];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool on = i < n && levels[i] >= split_threshold(sched, K);
  int place;
  split_places(on, place);
  if (on) act[base + place] = i;
}

// The header row of a piece and the slice [first, first + count) of the ordered list copied to `slice`, the head of the
// block workspace the force runs on. Grid: max(1, ceil(count / 256)).
__global__ __launch_bounds__(256) void hsplit_head_kernel(const int* __restrict__ act, int first, int count, int n_act,
                                                          const int* __restrict__ sched, int* __restrict__ slice,
                                                          double* __restrict__ rows, int row_len) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < count) slice[p] = act[first + p];
  if (blockIdx.x != 0) return;
  if (threadIdx.x == 0) {
    int* head = reinterpret_cast<int*>(rows);
    head[0] = sched[kTNext];
    head[1] = n_act;
    head[2] = first;
    head[3] = count;
  } else if ((int)threadIdx.x >= 2 && (int)threadIdx.x < row_len) {
    rows[threadIdx.x] = 0.0;
  }
}

// the last slot of a row: {new level, clamped}
__device__ __forceinline__ void store_slot(double* row, int row_len, int level, bool clamped) {
  int* slot = reinterpret_cast<int*>(row + row_len - 1);
  slot[0] = level;
  slot[1] = clamped ? 1 : 0;
}

// Row p of the slice (body i = act[p], its own step h = dt 2^-k_i): hblock_correct_kernel<double>'s arithmetic on the
// thread's own copy of x and v; nothing of the state is written. rows: the piece's first result row.
__global__ __launch_bounds__(256) void hsplit_rows_kernel(const double* __restrict__ slabs, int n_slabs,
                                                          const int* __restrict__ act, int count, double g, int K,
                                                          double dt, double tick, double eta,
                                                          const double* __restrict__ pos, const double* __restrict__ vel,
                                                          const double* __restrict__ acc, const double* __restrict__ jerk,
                                                          const int* __restrict__ levels, const int* __restrict__ sched,
                                                          double* __restrict__ rows) {
  const size_t p = hermite_sum_row<double>();
  double a1[3], j1[3];
  if (!hermite_slab_sum(slabs, n_slabs, count, p, p < (size_t)count, g, a1, j1)) return;
  const size_t i = (size_t)act[p];
  const int lev = levels[i];
  const int d = 1 << (K - lev);
  const double h = hblock_ticks_len(dt, d, tick);
  const HermiteStep<double> hc = hermite_step_constants<double>(h);
  double x[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
  double v[3] = {vel[3 * i], vel[3 * i + 1], vel[3 * i + 2]};
  const Corrected<double> c = hermite_correct_row(x, v, acc + 3 * i, jerk + 3 * i, (size_t)0, a1, j1, hc.dt_half,
                                                  hc.dt2_twelfth);
  bool clamped;
  const int nl = hblock_next_level(hblock_wanted(c.a0, c.j0, a1, j1, h, dt, eta, K), K, lev, d, sched[kTNext], clamped);
  double* row = rows + p * kRow4;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    row[k] = c.x1[k];
    row[3 + k] = v[k];
    row[6 + k] = a1[k];
    row[9 + k] = j1[k];
    row[12 + k] = 0.0;
  }
  store_slot(row, kRow4, nl, clamped);
}

// ... and of the 6th order: hblock6_correct_kernel's arithmetic (hermite6_finish_row, hblock6_wanted).
__global__ __launch_bounds__(256) void hsplit6_rows_kernel(const double* __restrict__ slabs, int n_slabs,
                                                           const int* __restrict__ act, int count, double g, int K,
                                                           double dt, double tick, double eta,
                                                           const double* __restrict__ pos, const double* __restrict__ vel,
                                                           const double* __restrict__ acc, const double* __restrict__ jerk,
                                                           const double* __restrict__ snap,
                                                           const int* __restrict__ levels, const int* __restrict__ sched,
                                                           double* __restrict__ rows) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)count) return;
  const size_t i = (size_t)act[p];
  const int lev = levels[i];
  const int d = 1 << (K - lev);
  const double h = hblock_ticks_len(dt, d, tick);
  double x[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
  double v[3] = {vel[3 * i], vel[3 * i + 1], vel[3 * i + 2]};
  double a1[3], j1[3], s1[3], c1[3];
  const Hermite6Ends e = hermite6_finish_row<false>(slabs, n_slabs, (size_t)count, p, (size_t)0, g,
                                                    hermite6_step_constants(h), x, v, acc + 3 * i, jerk + 3 * i,
                                                    snap + 3 * i, a1, j1, s1, c1, nullptr, nullptr, (size_t)0);
  bool clamped;
  const int nl = hblock_next_level(hblock6_wanted(e.a0, e.j0, e.s0, e.a1, e.j1, e.s1, e.c1, h, dt, eta, K), K, lev, d,
                                   sched[kTNext], clamped);
  double* row = rows + p * kRow6;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    row[k] = x[k];
    row[3 + k] = v[k];
    row[6 + k] = a1[k];
    row[9 + k] = j1[k];
    row[12 + k] = s1[k];
    row[15 + k] = c1[k];
  }
  row[18] = 0.0;
  store_slot(row, kRow6, nl, clamped);
}

// the A (n, 3) state arrays of an order, in row order: x v a j (s c)
template <int A>
struct SplitState { double* arr[A]; };

// The slice piece r of `world` holds of a list of n_act entries cut into pieces of q.
__device__ __forceinline__ int piece_first(int r, int q, int n_act) {
  const long long f = (long long)r * q;
  return f < n_act ? (int)f : n_act;
}

// One thread per list entry p: its row (piece p / q of rows_all, pieces of 1 + q rows of W doubles) into the state, then
// hblock_book_level. Workgroup 0 compares the headers first.
template <int W, int A>
__global__ __launch_bounds__(256) void hsplit_apply_kernel(const double* __restrict__ rows_all, int world, int q,
                                                           const int* __restrict__ act, int n_act, int K,
                                                           SplitState<A> st, const double* __restrict__ mass,
                                                           int* __restrict__ ticks, int* __restrict__ levels,
                                                           int* __restrict__ sched, d4* __restrict__ posd) {
  const int t_next = sched[kTNext];
  if (blockIdx.x == 0) {
    for (int r = threadIdx.x; r < world; r += 256) {
      const int* head = reinterpret_cast<const int*>(rows_all + (size_t)r * (q + 1) * W);
      const int first = piece_first(r, q, n_act);
      if (head[0] != t_next || head[1] != n_act || head[1] != sched[kNAct] || head[2] != first ||
          head[3] != piece_first(r + 1, q, n_act) - first)
        sched[kDiverged] = 1;
    }
  }
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n_act) return;
  const int r = p / q;
  const double* row = rows_all + ((size_t)r * (q + 1) + 1 + (p - r * q)) * W;
  const int i = act[p];
#pragma unroll
  for (int a = 0; a < A; ++a)
#pragma unroll
    for (int k = 0; k < 3; ++k) st.arr[a][3 * (size_t)i + k] = row[3 * a + k];
  posd[i] = d4{row[0], row[1], row[2], mass[i]};
  const int* slot = reinterpret_cast<const int*>(row + W - 1);
  const int lev = levels[i];
  int nl = slot[0];
  if (nl < 0 || nl > K) {                      // no row of a sound piece: keep the histogram's bounds, report
    sched[kDiverged] = 1;
    nl = lev;
  }
  hblock_book_level(nl, slot[1] != 0, K, lev, t_next, i, p == 0, ticks, levels, sched);
}

// ---- the workspace: the ordered list, the ordering's counts, then the block workspace of the slice
size_t list_bytes(int n) { return (size_t)ceil_div(n, 8) * 8 * sizeof(int); }
size_t count_bytes(int n) { return (size_t)ceil_div(ceil_div(n, 256), 8) * 8 * sizeof(int); }
size_t head_bytes(int n) { return list_bytes(n) + count_bytes(n); }

int* ws_list(void* ws) { return static_cast<int*>(ws); }
int* ws_counts(void* ws, int n) { return reinterpret_cast<int*>(static_cast<char*>(ws) + list_bytes(n)); }
char* ws_block(void* ws, int n) { return static_cast<char*>(ws) + head_bytes(n); }

// what the rows of a slice of `count` use: the head, the slice's list and its slabs (K_OUT sums per target and slab)
size_t rows_bytes(int n, int count, int k_out) {
  return head_bytes(n) +
         (count > 0 ? list_bytes(n) + (size_t)plan_f64(n, count).slabs * count * k_out * sizeof(double) : 0);
}

inline bool bad_ws(const void* ws, size_t have, size_t need) { return !ws || misaligned32(ws) || have < need; }

inline bool bad_scalars(int n, int n_act, int max_level) {
  return n <= 0 || n_act < 1 || n_act > n || bad_level(max_level);
}

// What the two rows entries share: the checks, the header and the slice's list, the force through `force` (the order's
// nbd_hblock*_force_f64 on the block workspace), then `rows_launch(slabs, n_slabs, slice)`.
template <class Force, class Rows>
int split_rows(int n, int n_act, int first, int count, int max_level, double dt, double eta, bool ptrs_ok,
               const int* sched, double* rows_out, int row_len, int k_out, void* workspace, size_t workspace_bytes,
               hipStream_t st, Force force, Rows rows_launch) {
  if (bad_scalars(n, n_act, max_level) || first < 0 || count < 0 || first > n_act || count > n_act - first ||
      !(dt > 0.0) || !(eta > 0.0))
    return NBD_E_BADARG;
  if (!ptrs_ok || !sched || !rows_out || misaligned32(rows_out)) return NBD_E_BADARG;
  if (bad_ws(workspace, workspace_bytes, rows_bytes(n, count, k_out))) return NBD_E_WORKSPACE;
  char* block = ws_block(workspace, n);
  hsplit_head_kernel<<<count > 0 ? ceil_div(count, 256) : 1, 256, 0, st>>>(
      ws_list(workspace), first, count, n_act, sched, reinterpret_cast<int*>(block), rows_out, row_len);
  int rc = launch_status();
  if (rc || count == 0) return rc;
  rc = force(block, workspace_bytes - head_bytes(n));
  if (rc) return rc;
  rows_launch(reinterpret_cast<const double*>(block + list_bytes(n)), plan_f64(n, count).slabs,
              reinterpret_cast<const int*>(block));
  return launch_status();
}

template <int W, int A>
int split_apply(const double* rows_all, int world, int q, int n_act, SplitState<A> s, const double* mass, int* ticks,
                int* levels, int n, int max_level, int* sched, double* posd, void* workspace, size_t workspace_bytes,
                hipStream_t st) {
  if (bad_scalars(n, n_act, max_level) || world < 1 || q < 1 || (long long)world * q < n_act) return NBD_E_BADARG;
  for (int a = 0; a < A; ++a)
    if (!s.arr[a]) return NBD_E_BADARG;
  if (!rows_all || misaligned32(rows_all) || !mass || !ticks || !levels || !sched || !posd || misaligned32(posd))
    return NBD_E_BADARG;
  if (bad_ws(workspace, workspace_bytes, head_bytes(n))) return NBD_E_WORKSPACE;
  hsplit_apply_kernel<W, A><<<ceil_div(n_act, 256), 256, 0, st>>>(rows_all, world, q, ws_list(workspace), n_act,
                                                                   max_level, s, mass, ticks, levels, sched,
                                                                   reinterpret_cast<d4*>(posd));
  return launch_status();
}

}  // namespace

extern "C" {

size_t nbd_hblock_split_f64_workspace_bytes(int n) {
  return n <= 0 ? 0 : head_bytes(n) + nbd_hblock_f64_workspace_bytes(n);
}

size_t nbd_hblock6_split_f64_workspace_bytes(int n) {
  return n <= 0 ? 0 : head_bytes(n) + nbd_hblock6_f64_workspace_bytes(n);
}

int nbd_hblock_order_list(const int* levels, int n, int max_level, int* sched, void* workspace, size_t workspace_bytes,
                          nbd_stream_t stream) {
  if (n <= 0 || bad_level(max_level) || !levels || !sched) return NBD_E_BADARG;
  if (bad_ws(workspace, workspace_bytes, head_bytes(n))) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int groups = ceil_div(n, 256);
  hsplit_count_kernel<<<groups, 256, 0, st>>>(levels, n, max_level, sched, ws_counts(workspace, n));
  const int rc = launch_status();
  if (rc) return rc;
  hsplit_order_kernel<<<groups, 256, 0, st>>>(levels, n, max_level, sched, ws_counts(workspace, n),
                                              ws_list(workspace));
  return launch_status();
}

int nbd_hblock_split_rows_f64(const double* pos, const double* vel, const double* acc, const double* jerk,
                              const int* levels, int n, int n_act, int first, int count, int max_level, double dt,
                              double eta, double softening_sq, double g_const, const int* sched, const double* posd,
                              const double* veld, double* rows_out, void* workspace, size_t workspace_bytes,
                              nbd_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  const bool ok = pos && vel && acc && jerk && levels && posd && veld && !misaligned32(posd) && !misaligned32(veld);
  return split_rows(
      n, n_act, first, count, max_level, dt, eta, ok, sched, rows_out, kRow4, 6, workspace, workspace_bytes, st,
      [=](void* block, size_t bytes) { return nbd_hblock_force_f64(posd, veld, n, count, softening_sq, block, bytes, stream); },
      [=](const double* slabs, int n_slabs, const int* slice) {
        hsplit_rows_kernel<<<ceil_div(count, 256), 256, 0, st>>>(slabs, n_slabs, slice, count, g_const, max_level, dt,
                                                                  ldexp(1.0, -max_level), eta, pos, vel, acc, jerk,
                                                                  levels, sched, rows_out + kRow4);
      });
}

int nbd_hblock6_split_rows_f64(const double* pos, const double* vel, const double* acc, const double* jerk,
                               const double* snap, const int* levels, int n, int n_act, int first, int count,
                               int max_level, double dt, double eta, double softening_sq, double g_const,
                               const int* sched, const double* posd, const double* veld, const double* accd,
                               double* rows_out, void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  const bool ok = pos && vel && acc && jerk && snap && levels && posd && veld && accd && !misaligned32(posd) &&
                  !misaligned32(veld) && !misaligned32(accd);
  return split_rows(
      n, n_act, first, count, max_level, dt, eta, ok, sched, rows_out, kRow6, 9, workspace, workspace_bytes, st,
      [=](void* block, size_t bytes) {
        return nbd_hblock6_force_f64(posd, veld, accd, n, count, softening_sq, block, bytes, stream);
      },
      [=](const double* slabs, int n_slabs, const int* slice) {
        hsplit6_rows_kernel<<<ceil_div(count, 256), 256, 0, st>>>(slabs, n_slabs, slice, count, g_const, max_level, dt,
                                                                   ldexp(1.0, -max_level), eta, pos, vel, acc, jerk,
                                                                   snap, levels, sched, rows_out + kRow6);
      });
}

int nbd_hblock_split_apply_f64(const double* rows_all, int world, int q, int n_act, double* pos, double* vel,
                               double* acc, double* jerk, const double* mass, int* ticks, int* levels, int n,
                               int max_level, int* sched, double* posd, void* workspace, size_t workspace_bytes,
                               nbd_stream_t stream) {
  return split_apply<kRow4, 4>(rows_all, world, q, n_act, SplitState<4>{{pos, vel, acc, jerk}}, mass, ticks, levels, n,
                               max_level, sched, posd, workspace, workspace_bytes, (hipStream_t)stream);
}

int nbd_hblock6_split_apply_f64(const double* rows_all, int world, int q, int n_act, double* pos, double* vel,
                                double* acc, double* jerk, double* snap, double* crackle, const double* mass,
                                int* ticks, int* levels, int n, int max_level, int* sched, double* posd,
                                void* workspace, size_t workspace_bytes, nbd_stream_t stream) {
  return split_apply<kRow6, 6>(rows_all, world, q, n_act, SplitState<6>{{pos, vel, acc, jerk, snap, crackle}}, mass,
                               ticks, levels, n, max_level, sched, posd, workspace, workspace_bytes,
                               (hipStream_t)stream);
}

}  // extern "C"
