// tree_force.hip -- Barnes-Hut force in fp32: the O(N log N) companion of nbd_accel_f32.
//
//   order   Morton keys (21 bits per axis on the bounding cube of all bodies) sorted with a stable radix sort
//           (hipCUB, its scratch inside the caller's workspace): equal keys stay in index order.
//   tree    implicit over the sorted order: a level-L node holds the sorted bodies [i 8^(L+1), min(n, (i+1) 8^(L+1))),
//           level 0 = ceil(n/8) nodes of up to 8 bodies, every level above groups 8 consecutive nodes until one node is
//           left. No pointers, no atomics. Per node: mass M, centre of mass c, traceless quadrupole Q about c and the
//           size s = longest AABB edge + max-norm of (c - AABB centre); M, c, Q are summed in fp64 and stored fp32. Kept
//           per node: the mass and the first moments about the centre of the bounding box of all bodies (a parent's are
//           the sums of its children's) and the second moments about the node's OWN centre of mass (a parent's from its
//           children's by the parallel-axis theorem). Second moments about the box centre would cancel down to the
//           node's own size squared: one body far away stretches the box, and a small node far from its centre lost
//           (distance / size)^2 2^-53 of its Q that way -- a percent with a body at 10^6 beside a cluster of size 1.
//   walk    one wave per target group of 64 consecutive sorted bodies, one lane per body. The wave tests 32 nodes at a
//           time against the group's AABB T: accepted when theta > 0 and s^2 < theta^2 d^2 (d = distance from c to T).
//           Accepted cells and rejected level-0 nodes go to two LDS lists by ballot and prefix; a list is evaluated
//           when it holds 64 entries or more and once at the end, every lane reading the same LDS entry. The walk
//           state is a depth-first stack in LDS: a pop takes up to 32 entries from the top, a push adds the children
//           (one level down) of the rejected ones. The stack stays sorted by level (the lowest on top), a level
//           receives entries only when everything below it has just been popped, and then at most 8 x 32 of them: it
//           never holds more than 256 x levels entries, whatever theta and the input are. (Popping 64 at a time needs
//           twice the stack: 5 instead of 7 waves per CU, and a walk 11 % slower at N = 524 288.)
//           A workgroup is ONE wave: waves run different numbers of iterations, and nothing in the loop waits for
//           another wave (the __syncthreads() below order this wave's own LDS traffic; hipcc emits no s_barrier for a
//           64-thread workgroup).
//   split   A group whose AABB straddles a coarse Morton boundary opens most of the tree (at N = 524 288 a few dozen
//           groups sum ~N bodies each and one wave per group left the launch waiting for them: 38.8 ms). So 8 waves
//           share a group: all of them walk from the top and decide alike, and below the highest level with >= 64
//           nodes wave w descends only into the subtrees of that level's nodes i with i % 8 == w (an accepted cell
//           above that level is summed by the wave its index selects). Each wave leaves a partial sum in a slab and a
//           last kernel adds the 8 slabs in order and scatters to the caller's order. Fewer than 64 nodes on every
//           level: one wave, no slabs. The set of accepted cells and of rejected level-0 nodes does not change.
//   sums    fixed order: the bodies of a level-0 node, then the nodes, and the cells of a list pass, then the passes (both
//           outer sums compensated) -- bit-identical from run to run.
//           The pair term is the direct kernel's: exact differences, explicit FMAs, v_rsq_f32; j == i is excluded by
//           index, so softening 0 and coincident bodies behave as nbd_accel_f32 does.
//   phi     the same walk sums the potential whose gradient the force above is, over the same cells and bodies: a body adds
//           m s (one FMA, s the masked rsq of the force), a cell M u + 1/2 (r.Qr) u^5 (two, u and r.Qr in registers). fp32
//           sums stop at 8 terms -- the bodies of a level-0 node, 8 consecutive cells of a list pass -- and everything
//           above them is fp64 in a fixed order: the lane's running sum, the 8 partial sums of a split group (a slab of
//           doubles [split][n] behind every other region of the workspace), the factor -G. The self term (m_i / eps, not 0
//           as in the force) is excluded by the same index mask, the padding rows too. ACC / PHI choose what a walk
//           accumulates at compile time; the acc-only instantiations are the force kernel unchanged.
//   ranks   ("Several ranks") every rank builds the same tree from the gathered packed rows {x, y, z, m}
//           (the row stride of the box / key / gather kernels is a compile-time switch: the same values, the same bits)
//           and walks a contiguous range of the target groups: kRange offsets the group index of the same walk and
//           leaves the finished rows in TREE order, row 0 = the first body of the range's first group, the padding rows
//           of the last group as 0. Slabs and per-group counters stay indexed by the global body and group. A group's
//           walk reads nothing of another group's, so a row is bit for bit the full walk's, whatever the range; the
//           exchanged rows are placed into a range of the caller's order by scatter_kernel through `order`.
//   active  ("Block timesteps") a block step wants the force on a subset of the bodies, scattered along
//           the curve. select_active compacts the sorted positions k with flags[order[k]] != 0 into an ascending list
//           (hipCUB DeviceSelect over the flags in tree order: stable, no atomics, its scratch in a workspace of its
//           own); kList walks the whole tree for target groups of 64 consecutive LIST entries, one lane each, T the
//           AABB of those bodies alone. Slabs and per-group counters are indexed by the active row and group; the
//           finishing launch writes the rows order[list[t]] of the caller's array and no other. With every body listed
//           the groups, the boxes and every sum are the full walk's: the same bits.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <stdint.h>

#include "../../include/nbd.h"

typedef float f4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kMaxBodies = 1 << 24;
constexpr int kMaxLevels = 8;          // 8^8 = 2^24 bodies under the top node
constexpr int kLeaf = 8;               // bodies per level-0 node, children per node
constexpr int kGroup = 64;             // targets per wave
constexpr int kBoxBlocks = 256;        // partial bounding boxes
constexpr int kMom = 13;               // doubles per node while building: M, sum m x (3), sum m d d^T about c (6), sum x (3)
constexpr int kListCap = 128;          // a list is flushed at >= 64 entries and grows by <= kPop per iteration
constexpr int kPop = 32;               // stack entries tested per iteration
constexpr int kStackPerLevel = kLeaf * kPop;
constexpr int kSplit = 8;              // waves that share a target group's walk (where the tree is deep enough)
constexpr int kSplitMinNodes = 64;     // ... by the nodes of the highest level that has at least this many

struct Levels {
  int levels, total;
  int split, start_level;      // the walk of a group is shared by `split` waves: wave w owns the subtrees of the
                               // start level's nodes i with i % split == w (split = 1: start_level = -1)
  int count[kMaxLevels], off[kMaxLevels];
};

inline Levels plan_levels(int n) {
  Levels L = {};
  int c = (n + kLeaf - 1) / kLeaf, off = 0, l = 0;
  for (;;) {
    L.count[l] = c; L.off[l] = off; off += c; ++l;
    if (c <= 1) break;
    c = (c + kLeaf - 1) / kLeaf;
  }
  L.levels = l; L.total = off;
  L.split = 1; L.start_level = -1;
  for (int k = l - 1; k >= 0; --k)
    if (L.count[k] >= kSplitMinNodes) { L.split = kSplit; L.start_level = k; break; }
  return L;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int pad64(int n) { return (n + 63) & ~63; }

size_t sort_temp_bytes(int n) {
  size_t b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const int*)nullptr,
                                           (int*)nullptr, n, 0, 63);      // a size query: nothing runs
  return align256(b);
}

struct Layout {
  size_t box, keys_in, keys_out, vals_in, order, posm, nodes, mom, aabb, gcnt, slabs, cub, cub_bytes, phi_slabs, total;
};

inline Layout layout(int n, const Levels& L) {
  Layout w = {};
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o = align256(o + bytes); return at; };
  w.box = take((size_t)(kBoxBlocks + 1) * 8 * sizeof(float));
  w.keys_in = take((size_t)n * 8); w.keys_out = take((size_t)n * 8);
  w.vals_in = take((size_t)n * 4); w.order = take((size_t)n * 4);
  w.posm = take((size_t)pad64(n) * 16);
  w.nodes = take((size_t)L.total * 48);
  w.mom = take((size_t)L.total * kMom * 8);
  w.aabb = take((size_t)L.total * 8 * 4);
  w.gcnt = take((size_t)(pad64(n) / kGroup) * L.split * 2 * 4);
  w.slabs = take(L.split > 1 ? (size_t)L.split * n * 3 * 4 : 0);
  w.cub_bytes = sort_temp_bytes(n);
  w.cub = take(w.cub_bytes);
  w.phi_slabs = take(L.split > 1 ? (size_t)L.split * n * 8 : 0);      // last: every offset above is the force's own
  w.total = o;
  return w;
}

// the workspace of select_active: the list first, then its count, the flags in tree order and the compaction's scratch
struct ActiveLayout { size_t list, n_act, flags, cub, cub_bytes, total; };

inline ActiveLayout active_layout(int n) {
  ActiveLayout w = {};
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o = align256(o + bytes); return at; };
  w.list = take((size_t)n * 4);
  w.n_act = take(sizeof(int));
  w.flags = take((size_t)n);
  size_t b = 0;
  (void)hipcub::DeviceSelect::Flagged(nullptr, b, hipcub::CountingInputIterator<int>(0), (const unsigned char*)nullptr,
                                      (int*)nullptr, (int*)nullptr, n);   // a size query: nothing runs
  w.cub_bytes = align256(b);
  w.cub = take(w.cub_bytes);
  w.total = o;
  return w;
}

inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// ---------------------------------------------------------------- bounding box, keys, gather

// Rows of the caller's bodies: pos (n,3) beside mass (n,) (STRIDE 3) or packed {x, y, z, m} (STRIDE 4, what the
// all-gather of a range-sharded step delivers); the layout is a compile-time switch of the three kernels that read them.
// part[b] = {lo (3), pad, hi (3), pad} of the bodies block b strides over (+-inf where it sees none)
template <int STRIDE>
__global__ __launch_bounds__(256) void box_partial_kernel(const float* __restrict__ pos, int n, float* __restrict__ part) {
  __shared__ float red[6][256];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
    for (int a = 0; a < 3; ++a) {
      const float v = pos[(size_t)STRIDE * i + a];
      lo[a] = fminf(lo[a], v); hi[a] = fmaxf(hi[a], v);
    }
  for (int a = 0; a < 3; ++a) { red[a][threadIdx.x] = lo[a]; red[3 + a][threadIdx.x] = hi[a]; }
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int a = 0; a < 3; ++a) {
        red[a][threadIdx.x] = fminf(red[a][threadIdx.x], red[a][threadIdx.x + w]);
        red[3 + a][threadIdx.x] = fmaxf(red[3 + a][threadIdx.x], red[3 + a][threadIdx.x + w]);
      }
    __syncthreads();
  }
  if (threadIdx.x < 3) {
    part[blockIdx.x * 8 + threadIdx.x] = red[threadIdx.x][0];
    part[blockIdx.x * 8 + 4 + threadIdx.x] = red[3 + threadIdx.x][0];
  }
}

// box = part[kBoxBlocks] = {lo (3), cells per unit length, centre (3), 0}: the bounding cube has the longest edge of the box
__global__ __launch_bounds__(256) void box_final_kernel(float* __restrict__ part) {
  __shared__ float red[6][256];
  const int t = threadIdx.x;
  for (int a = 0; a < 3; ++a) { red[a][t] = part[t * 8 + a]; red[3 + a][t] = part[t * 8 + 4 + a]; }
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w)
      for (int a = 0; a < 3; ++a) {
        red[a][t] = fminf(red[a][t], red[a][t + w]);
        red[3 + a][t] = fmaxf(red[3 + a][t], red[3 + a][t + w]);
      }
    __syncthreads();
  }
  if (t == 0) {
    float* box = part + kBoxBlocks * 8;
    float side = 0.f;
    for (int a = 0; a < 3; ++a) side = fmaxf(side, red[3 + a][0] - red[a][0]);
    for (int a = 0; a < 3; ++a) { box[a] = red[a][0]; box[4 + a] = 0.5f * red[a][0] + 0.5f * red[3 + a][0]; }
    box[3] = side > 0.f ? 2097152.0f / side : 0.f;
    box[7] = 0.f;
  }
}

__device__ inline uint64_t spread21(uint32_t v) {      // bit k of the low 21 -> bit 3k
  uint64_t x = v & 0x1fffffu;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}

template <int STRIDE>
__global__ __launch_bounds__(256) void key_kernel(const float* __restrict__ pos, int n, const float* __restrict__ box,
                                                  uint64_t* __restrict__ keys, int* __restrict__ vals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float scale = box[3];
  uint32_t q[3];
  for (int a = 0; a < 3; ++a) {
    const float f = (pos[(size_t)STRIDE * i + a] - box[a]) * scale;
    q[a] = (uint32_t)fminf(fmaxf(f, 0.f), 2097151.f);       // a NaN coordinate lands in cell 0
  }
  keys[i] = spread21(q[0]) << 2 | spread21(q[1]) << 1 | spread21(q[2]);
  vals[i] = i;
}

// posm[k] = {x, y, z, m} of body order[k] for k < n, zeros in the padding up to a multiple of 64; order_out = order
// (STRIDE 4: `pos` holds the packed rows, 16-byte aligned, and `mass` is not read)
template <int STRIDE>
__global__ __launch_bounds__(256) void gather_kernel(const float* __restrict__ pos, const float* __restrict__ mass, int n,
                                                     int n_pad, const int* __restrict__ order, f4* __restrict__ posm,
                                                     int* __restrict__ order_out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_pad) return;
  f4 p = {0.f, 0.f, 0.f, 0.f};
  if (k < n) {
    const int j = order[k];
    if (STRIDE == 4) p = reinterpret_cast<const f4*>(pos)[j];
    else p = f4{pos[(size_t)3 * j], pos[(size_t)3 * j + 1], pos[(size_t)3 * j + 2], mass[j]};
    order_out[k] = j;
  }
  posm[k] = p;
}

// ---------------------------------------------------------------- nodes

// c - centre of a node from its mass, first moments and sum of positions about `centre` (mom: kMom doubles) and its body
// count: the centre of mass, for a node without mass the mean of its bodies.
__device__ inline void node_centre(const double* m, long long cnt, double* c) {
  const double M = m[0];
  for (int a = 0; a < 3; ++a) c[a] = M != 0.0 ? m[1 + a] / M : m[10 + a] / (double)cnt;
}

// m[4..9] += w d d^T (xx, xy, xz, yy, yz, zz)
__device__ inline void add_second_moments(double* m, double w, const double* d) {
  m[4] += w * d[0] * d[0]; m[5] += w * d[0] * d[1]; m[6] += w * d[0] * d[2];
  m[7] += w * d[1] * d[1]; m[8] += w * d[1] * d[2]; m[9] += w * d[2] * d[2];
}

// The walk's record of a node from its moments (mom: kMom doubles, the second ones C_ab = sum m (x - c)_a (x - c)_b about
// the node's own centre), its body count and its AABB: nodes[3 id] = {c, s}, {M, Qxx, Qxy, Qxz}, {Qyy, Qyz, Qzz, 0}.
__device__ inline void finish_node(const double* m, long long cnt, const float* lo, const float* hi, const float* centre,
                                   f4* __restrict__ rec) {
  const double M = m[0];
  double c[3];
  node_centre(m, cnt, c);
  const double* C = m + 4;
  const double tr = C[0] + C[3] + C[5];
  double edge = 0.0, shift = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double l = lo[a], h = hi[a];
    edge = fmax(edge, h - l);
    shift = fmax(shift, fabs((double)centre[a] + c[a] - 0.5 * (l + h)));
  }
  rec[0] = f4{(float)((double)centre[0] + c[0]), (float)((double)centre[1] + c[1]), (float)((double)centre[2] + c[2]),
              (float)(edge + shift)};
  rec[1] = f4{(float)M, (float)(3.0 * C[0] - tr), (float)(3.0 * C[1]), (float)(3.0 * C[2])};
  rec[2] = f4{(float)(3.0 * C[3] - tr), (float)(3.0 * C[4]), (float)(3.0 * C[5] - tr), 0.f};
}

__global__ __launch_bounds__(128) void leaf_kernel(const f4* __restrict__ posm, int n, int count, const float* __restrict__ box,
                                                   double* __restrict__ mom, float* __restrict__ aabb, f4* __restrict__ nodes) {
  const int id = blockIdx.x * 128 + threadIdx.x;
  if (id >= count) return;
  const float centre[3] = {box[4], box[5], box[6]};
  const int b0 = id * kLeaf, b1 = min(n, b0 + kLeaf);
  double m[kMom] = {};
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int b = b0; b < b1; ++b) {
    const f4 p = posm[b];
    const float xf[3] = {p.x, p.y, p.z};
    const double w = p.w;
    double x[3];
    for (int a = 0; a < 3; ++a) {
      x[a] = (double)xf[a] - (double)centre[a];
      lo[a] = fminf(lo[a], xf[a]); hi[a] = fmaxf(hi[a], xf[a]);
      m[1 + a] += w * x[a]; m[10 + a] += x[a];
    }
    m[0] += w;
  }
  double c[3];
  node_centre(m, b1 - b0, c);
  for (int b = b0; b < b1; ++b) {                    // the second moments about the node's own centre
    const f4 p = posm[b];
    const double d[3] = {((double)p.x - (double)centre[0]) - c[0], ((double)p.y - (double)centre[1]) - c[1],
                         ((double)p.z - (double)centre[2]) - c[2]};
    add_second_moments(m, (double)p.w, d);
  }
  for (int k = 0; k < kMom; ++k) mom[(size_t)id * kMom + k] = m[k];
  for (int a = 0; a < 3; ++a) { aabb[(size_t)id * 8 + a] = lo[a]; aabb[(size_t)id * 8 + 4 + a] = hi[a]; }
  finish_node(m, b1 - b0, lo, hi, centre, nodes + (size_t)3 * id);
}

// level `lvl` >= 1 from the level below: node id sums its children [8 id, min(count_below, 8 id + 8))
__global__ __launch_bounds__(128) void upper_kernel(int n, int lvl, int count, int off, int count_below, int off_below,
                                                    const float* __restrict__ box, double* __restrict__ mom,
                                                    float* __restrict__ aabb, f4* __restrict__ nodes) {
  const int id = blockIdx.x * 128 + threadIdx.x;
  if (id >= count) return;
  const float centre[3] = {box[4], box[5], box[6]};
  const int c0 = id * kLeaf, c1 = min(count_below, c0 + kLeaf);
  double m[kMom] = {};
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int c = c0; c < c1; ++c) {
    const size_t g = (size_t)off_below + c;
    for (int k = 0; k < 4; ++k) m[k] += mom[g * kMom + k];
    for (int k = 10; k < kMom; ++k) m[k] += mom[g * kMom + k];
    for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], aabb[g * 8 + a]); hi[a] = fmaxf(hi[a], aabb[g * 8 + 4 + a]); }
  }
  const long long span = 1ll << (3 * (lvl + 1));
  const long long first = (long long)id * span, last = first + span < (long long)n ? first + span : (long long)n;
  double cn[3];
  node_centre(m, last - first, cn);
  for (int c = c0; c < c1; ++c) {                    // parallel axes: a child's own second moments, and its mass at its centre
    const double* child = mom + ((size_t)off_below + c) * kMom;
    for (int k = 4; k < 10; ++k) m[k] += child[k];
    const double Mk = child[0];
    if (Mk != 0.0) {
      const double d[3] = {child[1] / Mk - cn[0], child[2] / Mk - cn[1], child[3] / Mk - cn[2]};
      add_second_moments(m, Mk, d);
    }
  }
  const size_t g = (size_t)off + id;
  for (int k = 0; k < kMom; ++k) mom[g * kMom + k] = m[k];
  for (int a = 0; a < 3; ++a) { aabb[g * 8 + a] = lo[a]; aabb[g * 8 + 4 + a] = hi[a]; }
  finish_node(m, last - first, lo, hi, centre, nodes + 3 * g);
}

// ---------------------------------------------------------------- the walk

// which targets a launch walks: every group of the tree, the groups [group_lo, group_lo + gridDim.x) alone, or groups
// of 64 consecutive entries of a list of sorted positions. A compile-time switch of the walk and of its finishing kernel.
enum class Targets { kAll, kRange, kList };

// One record for every instantiation; an instantiation reads the fields of its own switches and no others.
struct WalkArgs {
  const f4* posm;          // sorted bodies, padded to a multiple of 64 with zeros
  const f4* nodes;         // 3 per node, level 0 first
  const int* order;        // sorted position -> caller's index
  float* acc_out;          // (n, 3) in the caller's order (written here when split == 1)
  float* slabs;            // [split][n][3] partial sums in tree order (split > 1)
  unsigned* gcnt;          // {accepted cells, rejected level-0 nodes} per wave: [split][groups][2]
  int n, levels, stack_cap, split, start_level;
  int count[kMaxLevels], off[kMaxLevels];
  float theta2, eps2, g;
  // PHI
  double* phi_out;         // (n,) in the caller's order (written here when split == 1)
  double* phi_slabs;       // [split][n] partial sums in tree order (split > 1)
  // kRange: acc_out / phi_out are in TREE order, row 0 = sorted body 64 group_lo, the last group's padding rows included
  int group_lo, groups;    // first group of the launch; groups of the whole tree (the stride of gcnt)
  // kList: lane t of the launch is sorted body list[t], t < n_act (an entry outside [0, n) is skipped as the lanes behind
  // n_act are); slabs are [split][n][3] by the active row t, gcnt by the active group
  const int* list;
  int n_act;
};

__device__ __forceinline__ int lanes_below(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

__device__ __forceinline__ float wave_min(float v) {
  for (int d = 32; d > 0; d >>= 1) v = fminf(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
  return v;
}

// tot += s, compensated (the library is built without fast-math and with -ffp-contract=off)
__device__ __forceinline__ void add_comp(float& tot, float& comp, float s) {
  const float y = s - comp, t = tot + y;
  comp = (t - tot) - y;
  tot = t;
}

constexpr int kWalkFixedLds = (3 * kListCap + 64 * kLeaf) * 16 + kListCap * 4 + 2 * kMaxLevels * 4;

template <bool QUAD, bool ACC, bool PHI, Targets TG>
__global__ __launch_bounds__(64) void tree_walk_kernel(const WalkArgs a) {
  constexpr bool RANGED = TG == Targets::kRange, ACTIVE = TG == Targets::kList;
  extern __shared__ f4 lds[];
  f4* cells = lds;                                   // [kListCap][3]
  f4* stage = cells + 3 * kListCap;                  // [64][kLeaf] bodies of one pass of the level-0 list
  int* leaf = reinterpret_cast<int*>(stage + 64 * kLeaf);   // [kListCap] level-0 node indices
  int* ltab = leaf + kListCap;                       // [kMaxLevels] count, [kMaxLevels] off
  unsigned* stack = reinterpret_cast<unsigned*>(ltab + 2 * kMaxLevels);

  const int lane = threadIdx.x;
  const int part = blockIdx.y;                       // which of the group's `split` waves this is
  int group_lo = 0;                                  // the launch's first target group (its row 0 of a ranged output)
  if constexpr (RANGED) group_lo = a.group_lo;
  const int row0 = group_lo * kGroup;
  int target = (group_lo + blockIdx.x) * kGroup + lane;
  bool listed = target < a.n;
  const int row = target;                            // the lane's row of the slabs
  f4 mine;
  if constexpr (ACTIVE) {                            // the lane's body comes from the list
    const int e = row < a.n_act ? a.list[row] : -1;
    listed = (unsigned)e < (unsigned)a.n;
    target = listed ? e : -1;                        // (no sorted index: nothing is masked for it, nothing stored)
    mine = listed ? a.posm[e] : f4{0.f, 0.f, 0.f, 0.f};
  } else {
    mine = a.posm[target];
  }
  const int i = target;
  const bool valid = listed;
  const f4 me = mine;
  const float x = me.x, y = me.y, z = me.z;
  // T: the AABB of the group's real bodies
  const float tlx = wave_min(valid ? x : INFINITY), tly = wave_min(valid ? y : INFINITY), tlz = wave_min(valid ? z : INFINITY);
  const float thx = wave_max(valid ? x : -INFINITY), thy = wave_max(valid ? y : -INFINITY),
              thz = wave_max(valid ? z : -INFINITY);

  if (lane < kMaxLevels) { ltab[lane] = a.count[lane]; ltab[kMaxLevels + lane] = a.off[lane]; }
  if (lane == 0) stack[0] = (unsigned)(a.levels - 1) << 24 | (unsigned)a.off[a.levels - 1];
  __syncthreads();

  float ax = 0.f, ay = 0.f, az = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;      // sums and their compensation
  double phi = 0.0;                                                      // sum of m s and of M u + 1/2 (r.Qr) u^5
  const float eps2 = a.eps2;
  int sp = 1, nc = 0, nl = 0;
  unsigned cells_total = 0, leaves_total = 0;

  auto flush_cells = [&](int count) {
    float sx = 0.f, sy = 0.f, sz = 0.f, sphi = 0.f;
#pragma unroll 4
    for (int e = 0; e < count; ++e) {
      const f4 v0 = cells[3 * e], v1 = cells[3 * e + 1];
      const float rx = v0.x - x, ry = v0.y - y, rz = v0.z - z;
      float r2 = __builtin_fmaf(rx, rx, eps2);
      r2 = __builtin_fmaf(ry, ry, r2);
      r2 = __builtin_fmaf(rz, rz, r2);
      const float u = __builtin_amdgcn_rsqf(r2);
      const float u2 = u * u, u3 = u2 * u;
      float w = v1.x * u3;
      if (QUAD) {
        const f4 v2 = cells[3 * e + 2];
        const float qx = __builtin_fmaf(v1.w, rz, __builtin_fmaf(v1.z, ry, v1.y * rx));
        const float qy = __builtin_fmaf(v2.y, rz, __builtin_fmaf(v2.x, ry, v1.z * rx));
        const float qz = __builtin_fmaf(v2.z, rz, __builtin_fmaf(v2.y, ry, v1.w * rx));
        const float rqr = __builtin_fmaf(rz, qz, __builtin_fmaf(ry, qy, rx * qx));
        const float u5 = u3 * u2, u7 = u5 * u2;
        w = __builtin_fmaf(2.5f * rqr, u7, w);
        if (ACC) { sx = __builtin_fmaf(-u5, qx, sx); sy = __builtin_fmaf(-u5, qy, sy); sz = __builtin_fmaf(-u5, qz, sz); }
        if (PHI) sphi = __builtin_fmaf(0.5f * rqr, u5, sphi);
      }
      if (ACC) { sx = __builtin_fmaf(w, rx, sx); sy = __builtin_fmaf(w, ry, sy); sz = __builtin_fmaf(w, rz, sz); }
      if (PHI) {
        sphi = __builtin_fmaf(v1.x, u, sphi);
        if ((e & 7) == 7) { phi += (double)sphi; sphi = 0.f; }   // the fp32 sum ends after 8 cells
      }
    }
    if (ACC) { add_comp(ax, cx, sx); add_comp(ay, cy, sy); add_comp(az, cz, sz); }
    if (PHI) phi += (double)sphi;
  };

  auto flush_leaves = [&](int count) {
    for (int base = 0; base < count; base += 64) {
      const int cnt = min(64, count - base);
      // 8 bodies of 8 nodes per load instruction: each octet of lanes reads one node's 128 contiguous bytes
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        const int e = p * 8 + (lane >> 3);
        if (e < cnt) stage[e * kLeaf + (lane & 7)] = a.posm[(size_t)leaf[base + e] * kLeaf + (lane & 7)];
      }
      __syncthreads();
      for (int e = 0; e < cnt; ++e) {
        const int j0 = __builtin_amdgcn_readfirstlane(leaf[base + e]) * kLeaf;
        float nx = 0.f, ny = 0.f, nz = 0.f, nphi = 0.f;
#pragma unroll
        for (int k = 0; k < kLeaf; ++k) {
          const f4 p = stage[e * kLeaf + k];
          const float dx = p.x - x, dy = p.y - y, dz = p.z - z;
          float r2 = __builtin_fmaf(dx, dx, eps2);
          r2 = __builtin_fmaf(dy, dy, r2);
          r2 = __builtin_fmaf(dz, dz, r2);
          float s = __builtin_amdgcn_rsqf(r2);
          s = (j0 + k != i && j0 + k < a.n) ? s : 0.f;        // j == i by index; the padding behind the last body
          if (ACC) {
            const float w = p.w * ((s * s) * s);
            nx = __builtin_fmaf(w, dx, nx); ny = __builtin_fmaf(w, dy, ny); nz = __builtin_fmaf(w, dz, nz);
          }
          if (PHI) nphi = __builtin_fmaf(p.w, s, nphi);
        }
        if (ACC) { add_comp(ax, cx, nx); add_comp(ay, cy, ny); add_comp(az, cz, nz); }
        if (PHI) phi += (double)nphi;
      }
      __syncthreads();
    }
  };

  while (sp > 0) {
    const int take = min(sp, kPop);
    sp -= take;
    const bool have = lane < take;
    const unsigned entry = have ? stack[sp + lane] : 0u;
    const int lvl = entry >> 24, node = entry & 0xffffffu;
    const f4 v0 = a.nodes[(size_t)3 * node];                      // node 0 for the idle lanes: in bounds, unused
    const float dx = fmaxf(fmaxf(tlx - v0.x, v0.x - thx), 0.f), dy = fmaxf(fmaxf(tly - v0.y, v0.y - thy), 0.f),
                dz = fmaxf(fmaxf(tlz - v0.z, v0.z - thz), 0.f);
    const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
    const bool accepted = have && a.theta2 > 0.f && v0.w * v0.w < a.theta2 * d2;
    const bool to_leaf = have && !accepted && lvl == 0;
    const bool open = have && !accepted && lvl > 0;
    // every wave of the group decides alike above the start level; there a cell is summed by one of them
    const int idx = node - ltab[kMaxLevels + lvl];
    const bool accept = accepted && (lvl <= a.start_level || idx % a.split == part);

    const unsigned long long m_acc = __ballot(accept), m_leaf = __ballot(to_leaf);
    if (accept) {
      const int at = nc + lanes_below(m_acc);
      cells[3 * at] = v0;
      cells[3 * at + 1] = a.nodes[(size_t)3 * node + 1];
      if (QUAD) cells[3 * at + 2] = a.nodes[(size_t)3 * node + 2];
    }
    if (to_leaf) leaf[nl + lanes_below(m_leaf)] = node;            // off[0] = 0: a level-0 node's index is its number
    nc += __popcll(m_acc); nl += __popcll(m_leaf);
    cells_total += __popcll(m_acc); leaves_total += __popcll(m_leaf);

    // children of the opened nodes, in lane order: the stack stays sorted by level
    // (at the start level: only the children this wave owns)
    int first = 0, born = 0, kids = 0, below_off = 0;
    bool own_only = false;
    if (open) {
      first = idx * kLeaf;
      born = min(kLeaf, ltab[lvl - 1] - first);
      below_off = ltab[kMaxLevels + lvl - 1];
      own_only = lvl - 1 == a.start_level;
      for (int k = 0; k < born; ++k) kids += !own_only || (first + k) % a.split == part;
    }
    int scan = kids;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(scan, d);
      if (lane >= d) scan += t;
    }
    const int pushed = __builtin_amdgcn_readfirstlane(__shfl(scan, 63));
    int at = sp + scan - kids;
    for (int k = 0; k < born; ++k)
      if ((!own_only || (first + k) % a.split == part) && at < a.stack_cap)
        stack[at++] = (unsigned)(lvl - 1) << 24 | (unsigned)(below_off + first + k);
    sp += pushed;
    __syncthreads();

    if (nc >= 64) { flush_cells(nc); nc = 0; }
    if (nl >= 64) { flush_leaves(nl); nl = 0; }
  }
  flush_cells(nc);
  flush_leaves(nl);

  if (ACC && valid) {
    if (a.split == 1) {
      const size_t o = (size_t)(RANGED ? i - row0 : a.order[i]) * 3;
      a.acc_out[o] = a.g * ax; a.acc_out[o + 1] = a.g * ay; a.acc_out[o + 2] = a.g * az;
    } else {
      const size_t o = ((size_t)part * a.n + row) * 3;
      a.slabs[o] = ax; a.slabs[o + 1] = ay; a.slabs[o + 2] = az;
    }
  }
  if constexpr (PHI) if (valid) {
    if (a.split == 1) a.phi_out[RANGED ? i - row0 : a.order[i]] = 0.0 - (double)a.g * phi;
    else a.phi_slabs[(size_t)part * a.n + row] = phi;
  }
  if (RANGED && !valid && a.split == 1) {           // the rows behind body n - 1 of the last group
    const size_t t = (size_t)(i - row0);
    if (ACC) { a.acc_out[3 * t] = 0.f; a.acc_out[3 * t + 1] = 0.f; a.acc_out[3 * t + 2] = 0.f; }
    if constexpr (PHI) a.phi_out[t] = 0.0;
  }
  if (lane == 0) {
    size_t o = ((size_t)part * gridDim.x + blockIdx.x) * 2;
    if constexpr (RANGED) o = ((size_t)part * a.groups + group_lo + blockIdx.x) * 2;   // by the global group
    a.gcnt[o] = cells_total; a.gcnt[o + 1] = leaves_total;
  }
}

// what a finished row is, from the sum of its partial sums: the acceleration g s (float), the potential -g s (double)
__device__ __forceinline__ float finish_row(float g, float s) { return g * s; }
__device__ __forceinline__ double finish_row(double g, double s) { return 0.0 - g * s; }

// The finishing launch of a split walk, for a (T = float, 3 columns) and for phi (T = double, 1 column): row t < rows adds
// the `split` partial sums of its slab row -- the waves of a group in their fixed order, each column on its own --
// scales by G and is placed by the walk's targets:
//   kAll    slab row t          -> out[order[t]]
//   kRange  slab row first + t  -> out[t], the TREE order; a row at or behind body n is written as 0
//   kList   slab row t          -> out[order[list[t]]]; an entry outside [0, n) is skipped, no other row is written
template <typename T, Targets TG>
__global__ __launch_bounds__(256) void slab_sum_kernel(const T* __restrict__ slabs, int split, int n, int first, int rows,
                                                       const int* __restrict__ order, const int* __restrict__ list, T g,
                                                       T* __restrict__ out) {
  constexpr int kCols = sizeof(T) == sizeof(float) ? 3 : 1;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= rows) return;
  const int i = TG == Targets::kRange ? first + t : t;           // the slab row
  const int body = TG == Targets::kList ? list[t] : i;           // the sorted position it belongs to
  const bool real = (unsigned)body < (unsigned)n;
  if (TG != Targets::kRange && !real) return;
  T s[kCols] = {};
  if (real)
    for (int w = 0; w < split; ++w)
      for (int c = 0; c < kCols; ++c) s[c] += slabs[((size_t)w * n + i) * kCols + c];
  const size_t o = (size_t)(TG == Targets::kRange ? t : order[body]) * kCols;
  for (int c = 0; c < kCols; ++c) out[o + c] = real ? finish_row(g, s[c]) : T(0);
}

// flags in tree order, one byte each: what the compaction of select_active reads
__global__ __launch_bounds__(256) void tree_flags_kernel(const int* __restrict__ flags, const int* __restrict__ order, int n,
                                                         unsigned char* __restrict__ sorted_flags) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < n) sorted_flags[k] = flags[order[k]] != 0;
}

// out[order[k] - lo] = sorted[k] for every sorted position k whose body the range [lo, hi) of the caller's order holds
// (order is a permutation: every output row is written once)
__global__ __launch_bounds__(256) void scatter_kernel(const int* __restrict__ order, int n, int lo, int hi,
                                                      const float* __restrict__ acc_sorted,
                                                      const double* __restrict__ phi_sorted, float* __restrict__ acc_out,
                                                      double* __restrict__ phi_out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int j = order[k];
  if (j < lo || j >= hi) return;
  const size_t o = (size_t)(j - lo);
  if (acc_sorted)
    for (int c = 0; c < 3; ++c) acc_out[o * 3 + c] = acc_sorted[(size_t)k * 3 + c];
  if (phi_sorted) phi_out[o] = phi_sorted[k];
}

// counters[0..1] = the per-group pairs of the groups [lo, hi) of all `split` waves (gcnt: [split][groups][2]); integers
__global__ __launch_bounds__(256) void counter_kernel(const unsigned* __restrict__ gcnt, int groups, int split, int lo,
                                                      int hi, unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long red[2][256];
  unsigned long long c = 0, l = 0;
  for (int w = 0; w < split; ++w)
    for (int g = lo + threadIdx.x; g < hi; g += 256) {
      const size_t o = ((size_t)w * groups + g) * 2;
      c += gcnt[o]; l += gcnt[o + 1];
    }
  red[0][threadIdx.x] = c; red[1][threadIdx.x] = l;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      red[0][threadIdx.x] += red[0][threadIdx.x + w];
      red[1][threadIdx.x] += red[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { counters[0] = red[0][0]; counters[1] = red[1][0]; }
}

// The targets of one walk: the groups [group_lo, group_hi) of the tree (kRange; kAll walks every group and reads
// neither), or the n_act sorted positions of `list` (kList).
struct TargetSet {
  int group_lo, group_hi;
  const int* list;
  int n_act;
};

// One walk over a built workspace: the acceleration (acc_out), the potential (phi_out) or both. kRange: of the target
// groups [group_lo, group_hi) alone, the outputs in tree order with (group_hi - group_lo) 64 rows; slabs and per-group
// counters stay where the full walk keeps them, indexed by the global body and group. kList: of the n_act sorted bodies
// of `list`, acc_out in the caller's order and only its listed rows; slabs and counters by the active row and group.
template <bool ACC, bool PHI, Targets TG>
int tree_walk(const void* workspace, int n, TargetSet t, float theta, float softening_sq, float g_const, int quadrupole,
              float* acc_out, double* phi_out, unsigned long long* counters_out, nbd_stream_t stream) {
  static_assert(TG != Targets::kList || (ACC && !PHI), "the listed walk sums the acceleration alone");
  hipStream_t st = (hipStream_t)stream;
  if (n < 0 || !(theta >= 0.f)) return NBD_E_BADARG;
  if (TG == Targets::kRange) {                       // the range first: an empty one asks for nothing
    if (n > kMaxBodies) return NBD_E_UNSUPPORTED;
    if (t.group_lo < 0 || t.group_lo > t.group_hi || t.group_hi > pad64(n) / kGroup) return NBD_E_BADARG;
    if (t.group_lo == t.group_hi) return 0;
  }
  if (TG == Targets::kList) {                        // the list first: an empty one is not walked, nothing is written
    if (t.n_act < 0 || t.n_act > n) return NBD_E_BADARG;
    if (n > kMaxBodies) return NBD_E_UNSUPPORTED;
    if (t.n_act == 0) {
      if (counters_out && hipMemsetAsync(counters_out, 0, 2 * sizeof(unsigned long long), st) != hipSuccess)
        return (int)hipGetLastError();
      return 0;
    }
    if (!t.list) return NBD_E_BADARG;
  }
  if (n > 0 && (!workspace || (ACC && !acc_out) || (PHI && !phi_out))) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (n > kMaxBodies) return NBD_E_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return NBD_E_BADARG;
  const int groups = pad64(TG == Targets::kList ? t.n_act : n) / kGroup;
  if (TG != Targets::kRange) { t.group_lo = 0; t.group_hi = groups; }
  const Levels L = plan_levels(n);
  const Layout w = layout(n, L);
  char* base = static_cast<char*>(const_cast<void*>(workspace));
  WalkArgs a = {};
  a.posm = reinterpret_cast<const f4*>(base + w.posm);
  a.nodes = reinterpret_cast<const f4*>(base + w.nodes);
  a.order = reinterpret_cast<const int*>(base + w.order);
  a.acc_out = acc_out;
  a.gcnt = reinterpret_cast<unsigned*>(base + w.gcnt);
  a.slabs = reinterpret_cast<float*>(base + w.slabs);
  a.phi_out = phi_out; a.phi_slabs = reinterpret_cast<double*>(base + w.phi_slabs);
  a.group_lo = t.group_lo; a.groups = groups;
  a.list = t.list; a.n_act = t.n_act;
  a.n = n; a.levels = L.levels; a.stack_cap = kStackPerLevel * L.levels;
  a.split = L.split; a.start_level = L.start_level;
  for (int l = 0; l < kMaxLevels; ++l) { a.count[l] = L.count[l]; a.off[l] = L.off[l]; }
  a.theta2 = theta * theta; a.eps2 = softening_sq; a.g = g_const;
  const size_t lds_bytes = kWalkFixedLds + (size_t)a.stack_cap * 4;
  const dim3 grid(t.group_hi - t.group_lo, L.split);
  if (quadrupole) tree_walk_kernel<true, ACC, PHI, TG><<<grid, 64, lds_bytes, st>>>(a);
  else tree_walk_kernel<false, ACC, PHI, TG><<<grid, 64, lds_bytes, st>>>(a);
  if (L.split > 1) {
    const int first = t.group_lo * kGroup;
    const int rows = TG == Targets::kAll ? n : TG == Targets::kList ? t.n_act : (t.group_hi - t.group_lo) * kGroup;
    const int blocks = (rows + 255) / 256;
    if constexpr (ACC)
      slab_sum_kernel<float, TG><<<blocks, 256, 0, st>>>(a.slabs, L.split, n, first, rows, a.order, t.list, g_const, acc_out);
    if constexpr (PHI)
      slab_sum_kernel<double, TG><<<blocks, 256, 0, st>>>(a.phi_slabs, L.split, n, first, rows, a.order, t.list,
                                                          (double)g_const, phi_out);
  }
  if (counters_out) counter_kernel<<<1, 256, 0, st>>>(a.gcnt, groups, L.split, t.group_lo, t.group_hi, counters_out);
  return launch_status();
}

// Keys, sort, sorted bodies and every node from the caller's rows: pos (n,3) beside mass (n,), or STRIDE 4 packed rows
template <int STRIDE>
int tree_build(const float* pos, const float* mass, int n, int* order_out, void* workspace, size_t workspace_bytes,
               nbd_stream_t stream) {
  if (n < 0 || (n > 0 && (!pos || (STRIDE == 3 && !mass) || !order_out))) return NBD_E_BADARG;
  if (n == 0) return 0;
  if (n > kMaxBodies) return NBD_E_UNSUPPORTED;
  if (!workspace) return NBD_E_BADARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return NBD_E_BADARG;
  if (STRIDE == 4 && (reinterpret_cast<uintptr_t>(pos) & 15)) return NBD_E_BADARG;
  const Levels L = plan_levels(n);
  const Layout w = layout(n, L);
  if (workspace_bytes < w.total) return NBD_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* base = static_cast<char*>(workspace);
  float* part = reinterpret_cast<float*>(base + w.box);
  float* box = part + kBoxBlocks * 8;
  uint64_t* keys_in = reinterpret_cast<uint64_t*>(base + w.keys_in);
  uint64_t* keys_out = reinterpret_cast<uint64_t*>(base + w.keys_out);
  int* vals_in = reinterpret_cast<int*>(base + w.vals_in);
  int* order = reinterpret_cast<int*>(base + w.order);
  f4* posm = reinterpret_cast<f4*>(base + w.posm);
  f4* nodes = reinterpret_cast<f4*>(base + w.nodes);
  double* mom = reinterpret_cast<double*>(base + w.mom);
  float* aabb = reinterpret_cast<float*>(base + w.aabb);

  box_partial_kernel<STRIDE><<<kBoxBlocks, 256, 0, st>>>(pos, n, part);
  box_final_kernel<<<1, 256, 0, st>>>(part);
  const int blocks = (n + 255) / 256;
  key_kernel<STRIDE><<<blocks, 256, 0, st>>>(pos, n, box, keys_in, vals_in);
  int rc = launch_status();
  if (rc) return rc;
  size_t cub_bytes = w.cub_bytes;
  const hipError_t e = hipcub::DeviceRadixSort::SortPairs(base + w.cub, cub_bytes, keys_in, keys_out, vals_in, order, n, 0,
                                                          63, st);
  if (e != hipSuccess) return (int)e;
  const int n_pad = pad64(n);
  gather_kernel<STRIDE><<<n_pad / 256 + 1, 256, 0, st>>>(pos, mass, n, n_pad, order, posm, order_out);
  leaf_kernel<<<(L.count[0] + 127) / 128, 128, 0, st>>>(posm, n, L.count[0], box, mom, aabb, nodes);
  for (int l = 1; l < L.levels; ++l)
    upper_kernel<<<(L.count[l] + 127) / 128, 128, 0, st>>>(n, l, L.count[l], L.off[l], L.count[l - 1], L.off[l - 1], box, mom,
                                                          aabb, nodes);
  return launch_status();
}

}  // namespace

extern "C" {

int nbd_tree_plan(int n, int* levels, int* nodes_total) {
  if (n < 0) return NBD_E_BADARG;
  if (n > kMaxBodies) return NBD_E_UNSUPPORTED;
  Levels L = {};
  if (n > 0) L = plan_levels(n);
  if (levels) *levels = L.levels;
  if (nodes_total) *nodes_total = L.total;
  return 0;
}

size_t nbd_tree_workspace_bytes(int n) {
  if (n <= 0 || n > kMaxBodies) return 0;
  return layout(n, plan_levels(n)).total;
}

int nbd_tree_regions(int n, size_t* order_off, size_t* posm_off, size_t* nodes_off) {
  if (n < 0 || !order_off || !posm_off || !nodes_off) return NBD_E_BADARG;
  if (n > kMaxBodies) return NBD_E_UNSUPPORTED;
  Layout w = {};                                     // n = 0: no workspace, every offset 0
  if (n > 0) w = layout(n, plan_levels(n));
  *order_off = w.order; *posm_off = w.posm; *nodes_off = w.nodes;
  return 0;
}

size_t nbd_tree_active_workspace_bytes(int n) {
  if (n <= 0 || n > kMaxBodies) return 0;
  return active_layout(n).total;
}

int nbd_tree_select_active(const void* workspace, int n, const int* flags, int* list_out, int* n_act_out,
                           void* active_workspace, size_t active_workspace_bytes, nbd_stream_t stream) {
  if (n < 0 || (n > 0 && (!workspace || !flags || !active_workspace))) return NBD_E_BADARG;
  if (n > kMaxBodies) return NBD_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    if (n_act_out && hipMemsetAsync(n_act_out, 0, sizeof(int), st) != hipSuccess) return (int)hipGetLastError();
    return 0;
  }
  if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(active_workspace)) & 255) return NBD_E_BADARG;
  const ActiveLayout w = active_layout(n);
  if (active_workspace_bytes < w.total) return NBD_E_WORKSPACE;
  char* base = static_cast<char*>(active_workspace);
  const int* order = reinterpret_cast<const int*>(static_cast<const char*>(workspace) + layout(n, plan_levels(n)).order);
  unsigned char* sorted_flags = reinterpret_cast<unsigned char*>(base + w.flags);
  if (!list_out) list_out = reinterpret_cast<int*>(base + w.list);
  if (!n_act_out) n_act_out = reinterpret_cast<int*>(base + w.n_act);
  tree_flags_kernel<<<(n + 255) / 256, 256, 0, st>>>(flags, order, n, sorted_flags);
  const int rc = launch_status();
  if (rc) return rc;
  size_t cub_bytes = w.cub_bytes;
  const hipError_t e = hipcub::DeviceSelect::Flagged(base + w.cub, cub_bytes, hipcub::CountingInputIterator<int>(0),
                                                     sorted_flags, list_out, n_act_out, n, st);
  return e == hipSuccess ? launch_status() : (int)e;
}

int nbd_tree_accel_active_f32(const void* workspace, size_t workspace_bytes, int n, const int* list, int n_act, float theta,
                              float softening_sq, float g_const, int quadrupole, float* acc_out,
                              unsigned long long* counters_out, nbd_stream_t stream) {
  // the one check tree_walk() cannot make, asked where it would launch: the size of the caller's workspace
  if (n_act >= 1 && n_act <= n && n <= kMaxBodies && workspace_bytes < layout(n, plan_levels(n)).total) return NBD_E_BADARG;
  return tree_walk<true, false, Targets::kList>(workspace, n, {0, 0, list, n_act}, theta, softening_sq, g_const, quadrupole,
                                                acc_out, nullptr, counters_out, stream);
}

int nbd_tree_build_f32(const float* pos, const float* mass, int n, int* order_out, void* workspace, size_t workspace_bytes,
                       nbd_stream_t stream) {
  return tree_build<3>(pos, mass, n, order_out, workspace, workspace_bytes, stream);
}

int nbd_tree_build_posm_f32(const float* posm, int n, int* order_out, void* workspace, size_t workspace_bytes,
                            nbd_stream_t stream) {
  return tree_build<4>(posm, nullptr, n, order_out, workspace, workspace_bytes, stream);
}

int nbd_tree_accel_f32(const void* workspace, int n, float theta, float softening_sq, float g_const, int quadrupole,
                       float* acc_out, unsigned long long* counters_out, nbd_stream_t stream) {
  return tree_walk<true, false, Targets::kAll>(workspace, n, {}, theta, softening_sq, g_const, quadrupole, acc_out, nullptr,
                                               counters_out, stream);
}

int nbd_tree_potential_f32(const void* workspace, int n, float theta, float softening_sq, float g_const, int quadrupole,
                           double* phi_out, unsigned long long* counters_out, nbd_stream_t stream) {
  return tree_walk<false, true, Targets::kAll>(workspace, n, {}, theta, softening_sq, g_const, quadrupole, nullptr, phi_out,
                                               counters_out, stream);
}

int nbd_tree_accel_potential_f32(const void* workspace, int n, float theta, float softening_sq, float g_const,
                                 int quadrupole, float* acc_out, double* phi_out, unsigned long long* counters_out,
                                 nbd_stream_t stream) {
  return tree_walk<true, true, Targets::kAll>(workspace, n, {}, theta, softening_sq, g_const, quadrupole, acc_out, phi_out,
                                              counters_out, stream);
}

int nbd_tree_accel_groups_f32(const void* workspace, int n, int group_lo, int group_hi, float theta, float softening_sq,
                              float g_const, int quadrupole, float* acc_sorted_out, unsigned long long* counters_out,
                              nbd_stream_t stream) {
  return tree_walk<true, false, Targets::kRange>(workspace, n, {group_lo, group_hi}, theta, softening_sq, g_const,
                                                 quadrupole, acc_sorted_out, nullptr, counters_out, stream);
}

int nbd_tree_potential_groups_f32(const void* workspace, int n, int group_lo, int group_hi, float theta,
                                  float softening_sq, float g_const, int quadrupole, double* phi_sorted_out,
                                  unsigned long long* counters_out, nbd_stream_t stream) {
  return tree_walk<false, true, Targets::kRange>(workspace, n, {group_lo, group_hi}, theta, softening_sq, g_const,
                                                 quadrupole, nullptr, phi_sorted_out, counters_out, stream);
}

int nbd_tree_accel_potential_groups_f32(const void* workspace, int n, int group_lo, int group_hi, float theta,
                                        float softening_sq, float g_const, int quadrupole, float* acc_sorted_out,
                                        double* phi_sorted_out, unsigned long long* counters_out, nbd_stream_t stream) {
  return tree_walk<true, true, Targets::kRange>(workspace, n, {group_lo, group_hi}, theta, softening_sq, g_const,
                                                quadrupole, acc_sorted_out, phi_sorted_out, counters_out, stream);
}

int nbd_tree_scatter_f32(const void* workspace, int n, int lo, int hi, const float* acc_sorted, const double* phi_sorted,
                         float* acc_out, double* phi_out, nbd_stream_t stream) {
  if (n < 0 || lo < 0 || lo > hi || hi > n) return NBD_E_BADARG;
  if (n > kMaxBodies) return NBD_E_UNSUPPORTED;
  if (lo == hi) return 0;                            // an empty range asks for nothing
  if (!acc_sorted && !phi_sorted) return NBD_E_BADARG;
  if (!workspace || (acc_sorted && !acc_out) || (phi_sorted && !phi_out)) return NBD_E_BADARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return NBD_E_BADARG;
  const Layout w = layout(n, plan_levels(n));
  const int* order = reinterpret_cast<const int*>(static_cast<const char*>(workspace) + w.order);
  scatter_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(order, n, lo, hi, acc_sorted, phi_sorted, acc_out, phi_out);
  return launch_status();
}

}  // extern "C"
