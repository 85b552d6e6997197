// forest.hip -- the SSM rescoring model, forest form: P histogram forests over ONE binned matrix (asl_forest_bin,
// asl_forest_fit, asl_forest_predict). gfx950 only.
//
// Method (DESIGN.md 3 "Rescoring model: forest"; restated in numpy by tests/forest_ref.py, bit for bit):
//   * a row is 64 bytes, one bin index per column (d <= 63); a tree is a complete heap of depth <= 12;
//   * every draw is fo_hash(seed, stream, counter, k): tree t's bootstrap is stream 2 t, counter = the draw;
//     its column draws are stream 2 t + 1, counter = the node id in heap order -- never a running counter, so a
//     tree cut at level d is the tree grown to depth d;
//   * trees grow level by level for a batch of (problem, tree) pairs sized from a workspace budget. Per level:
//       histogram  a workgroup stages 512 binned rows in LDS once and serves every pair of its group from them:
//                  a row adds its multiplicity into (node, slot, bin, class) uint32 counts. At levels 0 and 1 the
//                  counts are privatised in LDS and flushed with one integer atomic per non-empty bin; deeper,
//                  where the nodes are many and the contention is low, they go straight to global memory. The
//                  same pass first moves every row from its node of the previous level to the child its split
//                  sends it to (the partition step);
//       split      one wave per (node, slot) scans the 256 bins: integer prefix sums, the proxy in fp64 in ONE
//                  written order (the unit is built without contraction), the wave's best by (proxy, lowest bin);
//                  one thread then walks the slots in draw order.
//   Integer atomics only: the counts do not depend on arrival order, so equal inputs give equal bits.
#include <algorithm>
#include <cmath>

#include "fit_args.hpp"

namespace asl {

constexpr int FO_NT = 256;
constexpr int FO_ROWS = 512;                            // rows a workgroup of the histogram pass stages
constexpr int FO_LS = ASL_FOREST_ROW / 4 + 1;           // LDS row stride in dwords: odd, rows spread over the banks
constexpr int FO_MTRY = 7;                              // floor(sqrt(63))
constexpr int FO_SLOTS = 8;                             // column ids kept per node: one 8-byte load
constexpr int FO_HBINS = ASL_FOREST_MAX_BINS * 2;       // counts per (node, slot): (bin, class)
constexpr int FO_LDS_LEVELS = 2;                        // levels 0 and 1: histograms privatised in LDS
constexpr int FO_LDS_HIST = (1 << (FO_LDS_LEVELS - 1)) * FO_MTRY * FO_HBINS;
constexpr int FO_SPLIT_NT = 64 * 8;
constexpr unsigned FO_STOP = 0xFFFFu;                   // a row that is in no node of the level
static_assert((FO_ROWS * FO_LS + FO_LDS_HIST) * 4 <= 64 * 1024, "LDS of the histogram pass");
static_assert(FO_MTRY * FO_MTRY <= ASL_SVM_MAX_DIM && (FO_MTRY + 1) * (FO_MTRY + 1) > ASL_SVM_MAX_DIM, "mtry");
static_assert(ASL_FOREST_NODES == (1 << (ASL_FOREST_MAX_DEPTH + 1)) - 1 && ASL_FOREST_NODES < (int)FO_STOP, "heap");

// The one hash behind every draw (a 32-bit finaliser applied after each key word), and the map of a hash to
// 0 .. m - 1 by multiply-and-shift. tests/forest_ref.py states the same in numpy.
__host__ __device__ inline uint32_t fo_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
__host__ __device__ inline uint32_t fo_hash(uint32_t seed, uint32_t a, uint32_t b, uint32_t c) {
  uint32_t h = fo_mix(seed + 0x9e3779b9u);
  h = fo_mix(h + a);
  h = fo_mix(h + b);
  return fo_mix(h + c);
}
__host__ __device__ inline uint32_t fo_draw(uint32_t h, uint32_t m) { return (uint32_t)(((uint64_t)h * m) >> 32); }

// w1 / (w0 + w1) of a node; 0.5 where it has no weight
__device__ __forceinline__ double fo_value(double cw0, double cw1, uint32_t n0, uint32_t n1) {
  const double w0 = cw0 * (double)n0, w1 = cw1 * (double)n1;
  const double w = w0 + w1;
  return w > 0.0 ? w1 / w : 0.5;
}
// (a1^2 + a0^2) / (a0 + a1): one side of the proxy, and the parent's bound
__device__ __forceinline__ double fo_side(double a0, double a1) { return (a1 * a1 + a0 * a0) / (a0 + a1); }

__global__ __launch_bounds__(FO_NT) void forest_bin_kernel(const double *__restrict__ X, int64_t n, int d,
                                                           const double *__restrict__ edges,
                                                           const int32_t *__restrict__ n_edges,
                                                           uint8_t *__restrict__ out) {
  const int64_t i = block_linear() * FO_NT + threadIdx.x;
  if (i >= n * ASL_FOREST_ROW) return;
  const int64_t row = i / ASL_FOREST_ROW;
  const int j = (int)(i - row * ASL_FOREST_ROW);
  int lo = 0;
  if (j < d) {
    const double x = X[row * d + j];
    const double *e = edges + (size_t)j * (ASL_FOREST_MAX_BINS - 1);
    int hi = n_edges[j];
    while (lo < hi) {   // the first edge that is not < x
      const int mid = (lo + hi) >> 1;
      if (e[mid] < x) lo = mid + 1; else hi = mid;
    }
  }
  out[i] = (uint8_t)lo;
}

// mult[t, r] += 1 for each of tree t's n draws
__global__ __launch_bounds__(FO_NT) void forest_bootstrap_kernel(uint32_t *__restrict__ mult, int64_t n,
                                                                 uint32_t seed) {
  const int64_t j = (int64_t)blockIdx.x * FO_NT + threadIdx.x;
  const uint32_t t = blockIdx.y;
  if (j >= n) return;
  const uint32_t r = fo_draw(fo_hash(seed, 2u * t, (uint32_t)j, 0u), (uint32_t)n);
  atomicAdd(mult + (size_t)t * n + r, 1u);
}

// cols[t, node, 0 .. mtry): mtry distinct columns, in draw order. Draw k picks the r-th column not yet drawn,
// r uniform in 0 .. d - k - 1.
__global__ __launch_bounds__(FO_NT) void forest_columns_kernel(uint8_t *__restrict__ cols, int T, int d, int mtry,
                                                               uint32_t seed) {
  const int i = blockIdx.x * FO_NT + threadIdx.x;
  if (i >= T * ASL_FOREST_NODES) return;
  const uint32_t t = i / ASL_FOREST_NODES, node = i - t * ASL_FOREST_NODES;
  int taken[FO_MTRY];   // ascending
  uint64_t packed = 0;
  for (int k = 0; k < mtry; ++k) {
    int c = (int)fo_draw(fo_hash(seed, 2u * t + 1u, node, (uint32_t)k), (uint32_t)(d - k));
    for (int j = 0; j < k; ++j)
      if (c >= taken[j]) ++c;
    packed |= (uint64_t)c << (8 * k);
    int pos = k;
    while (pos > 0 && taken[pos - 1] > c) taken[pos] = taken[pos - 1], --pos;
    taken[pos] = c;
  }
  reinterpret_cast<uint64_t *>(cols)[i] = packed;
}

struct FoModel {
  int16_t *col;
  uint8_t *bin;
  uint32_t *n0, *n1;
  double *value;
};

__global__ __launch_bounds__(FO_NT) void forest_init_kernel(FoModel M, int64_t total) {
  const int64_t i = block_linear() * FO_NT + threadIdx.x;
  if (i >= total) return;
  M.col[i] = -1, M.bin[i] = 0, M.n0[i] = 0, M.n1[i] = 0;
  M.value[i] = i % ASL_FOREST_NODES == 0 ? 0.5 : 0.0;
}

struct FoArgs {
  const uint8_t *bins;    // [n, 64]
  int64_t n;
  int32_t d, mtry, T;
  const int8_t *label;    // [P, n]
  const double *cw;       // [P, 2]
  const uint32_t *mult;   // [T, n]
  const uint8_t *cols;    // [T, NODES, 8]
  int32_t q0, nq;         // the batch: pairs q0 .. q0 + nq - 1, pair = p * T + t
  int32_t level, group;   // pairs a workgroup of the histogram pass serves
  uint16_t *state;        // [nq, n]: the row's node, or FO_STOP
  uint32_t *hist;         // [nq, 2^level, mtry, 256, 2]
  FoModel M;
};

__device__ __forceinline__ unsigned fo_byte(const uint32_t *rows, int r, int c) {
  return (rows[r * FO_LS + (c >> 2)] >> ((c & 3) * 8)) & 0xffu;
}

template <bool LDS_HIST>
__global__ __launch_bounds__(FO_NT) void forest_hist_kernel(FoArgs A) {
  __shared__ uint32_t rows[FO_ROWS * FO_LS];
  __shared__ uint32_t hl[LDS_HIST ? FO_LDS_HIST : 1];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * FO_ROWS;
  const int nrows = (int)(A.n - row0 < FO_ROWS ? A.n - row0 : FO_ROWS);
  {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(A.bins) + row0 * (ASL_FOREST_ROW / 4);
    for (int i = tid; i < nrows * (ASL_FOREST_ROW / 4); i += FO_NT) rows[(i >> 4) * FO_LS + (i & 15)] = src[i];
  }
  __syncthreads();
  const int nodes_l = 1 << A.level, first = nodes_l - 1;
  const int per_pair = nodes_l * A.mtry * FO_HBINS;
  const int qa = blockIdx.y * A.group, qb = qa + A.group < A.nq ? qa + A.group : A.nq;
  for (int ql = qa; ql < qb; ++ql) {
    const int q = A.q0 + ql, p = q / A.T, t = q - p * A.T;
    const size_t mbase = (size_t)q * ASL_FOREST_NODES;
    uint32_t *hg = A.hist + (size_t)ql * per_pair;
    if (LDS_HIST) {
      for (int i = tid; i < per_pair; i += FO_NT) hl[i] = 0;
      __syncthreads();
    }
    for (int rr = tid; rr < nrows; rr += FO_NT) {
      const int64_t row = row0 + rr;
      uint16_t *st = A.state + (size_t)ql * A.n + row;
      unsigned node;
      if (A.level == 0) {   // in the problem and in the bag: at the root
        node = (A.label[(size_t)p * A.n + row] != 0 && A.mult[(size_t)t * A.n + row] != 0) ? 0u : FO_STOP;
        *st = (uint16_t)node;
      } else {              // partition: from the node of the level above to the child its split names
        node = *st;
        if (node == FO_STOP) continue;
        const int c = A.M.col[mbase + node];
        node = c < 0 ? FO_STOP : 2 * node + 1 + (fo_byte(rows, rr, c) > A.M.bin[mbase + node] ? 1u : 0u);
        *st = (uint16_t)node;
      }
      if (node == FO_STOP) continue;
      const uint32_t m = A.mult[(size_t)t * A.n + row];
      const int cls = A.label[(size_t)p * A.n + row] > 0 ? 1 : 0;
      const uint64_t cs = reinterpret_cast<const uint64_t *>(A.cols)[(size_t)t * ASL_FOREST_NODES + node];
      const int nl = (int)node - first;
      for (int k = 0; k < A.mtry; ++k) {
        const int c = (int)((cs >> (8 * k)) & 0xff);
        const int idx = ((nl * A.mtry + k) * ASL_FOREST_MAX_BINS + (int)fo_byte(rows, rr, c)) * 2 + cls;
        if (LDS_HIST) atomicAdd(hl + idx, m); else atomicAdd(hg + idx, m);
      }
    }
    if (LDS_HIST) {
      __syncthreads();
      for (int i = tid; i < per_pair; i += FO_NT) {
        const uint32_t v = hl[i];
        if (v) atomicAdd(hg + i, v);
      }
      __syncthreads();
    }
  }
}

// One workgroup per (node of the level, pair); wave k scans the histogram of the node's k-th drawn column.
__global__ __launch_bounds__(FO_SPLIT_NT) void forest_split_kernel(FoArgs A) {
  __shared__ double w_proxy[FO_SLOTS];
  __shared__ int w_bin[FO_SLOTS];
  __shared__ uint32_t w_l0[FO_SLOTS], w_l1[FO_SLOTS], w_tot[2];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nodes_l = 1 << A.level, nl = blockIdx.x, ql = blockIdx.y;
  const int q = A.q0 + ql, p = q / A.T, t = q - p * A.T;
  const unsigned node = (unsigned)(nodes_l - 1 + nl);
  const double cw0 = A.cw[2 * p], cw1 = A.cw[2 * p + 1];
  if (wave < A.mtry) {
    const uint32_t *h = A.hist + (((size_t)ql * nodes_l + nl) * A.mtry + wave) * FO_HBINS;
    const uint4 a = reinterpret_cast<const uint4 *>(h)[2 * lane], b = reinterpret_cast<const uint4 *>(h)[2 * lane + 1];
    const uint32_t c0[4] = {a.x, a.z, b.x, b.z}, c1[4] = {a.y, a.w, b.y, b.w};
    const uint32_t s0 = c0[0] + c0[1] + c0[2] + c0[3], s1 = c1[0] + c1[1] + c1[2] + c1[3];
    const uint32_t i0 = wave_incl_scan(s0), i1 = wave_incl_scan(s1);
    const uint32_t N0 = (uint32_t)__shfl((int)i0, 63, 64), N1 = (uint32_t)__shfl((int)i1, 63, 64);
    double best = -INFINITY;
    int best_bin = ASL_FOREST_MAX_BINS;
    uint32_t best_l0 = 0, best_l1 = 0;
    if (N0 != 0 && N1 != 0) {   // (a node of one class is a leaf; an absent node has no rows)
      uint32_t l0 = i0 - s0, l1 = i1 - s1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        l0 += c0[j], l1 += c1[j];
        const uint32_t r0 = N0 - l0, r1 = N1 - l1;
        const double wl0 = cw0 * (double)l0, wl1 = cw1 * (double)l1, wr0 = cw0 * (double)r0, wr1 = cw1 * (double)r1;
        if (l0 + l1 >= 1 && r0 + r1 >= 1 && wl0 + wl1 > 0.0 && wr0 + wr1 > 0.0) {
          const double proxy = fo_side(wl0, wl1) + fo_side(wr0, wr1);
          if (proxy > best) best = proxy, best_bin = 4 * lane + j, best_l0 = l0, best_l1 = l1;
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {   // the highest proxy, the lowest bin among equals
      const double op = __shfl_xor(best, o, 64);
      const int ob = __shfl_xor(best_bin, o, 64);
      const uint32_t ol0 = (uint32_t)__shfl_xor((int)best_l0, o, 64), ol1 = (uint32_t)__shfl_xor((int)best_l1, o, 64);
      if (op > best || (op == best && ob < best_bin)) best = op, best_bin = ob, best_l0 = ol0, best_l1 = ol1;
    }
    if (lane == 0) {
      w_proxy[wave] = best, w_bin[wave] = best_bin, w_l0[wave] = best_l0, w_l1[wave] = best_l1;
      if (wave == 0) w_tot[0] = N0, w_tot[1] = N1;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const uint32_t N0 = w_tot[0], N1 = w_tot[1];
  if (N0 + N1 == 0) return;
  const size_t mbase = (size_t)q * ASL_FOREST_NODES;
  if (A.level == 0) A.M.n0[mbase] = N0, A.M.n1[mbase] = N1, A.M.value[mbase] = fo_value(cw0, cw1, N0, N1);
  if (N0 == 0 || N1 == 0) return;
  double best = fo_side(cw0 * (double)N0, cw1 * (double)N1);   // what a split has to exceed
  int slot = -1;
  for (int k = 0; k < A.mtry; ++k)
    if (w_proxy[k] > best) best = w_proxy[k], slot = k;
  if (slot < 0) return;
  const uint64_t cs = reinterpret_cast<const uint64_t *>(A.cols)[(size_t)t * ASL_FOREST_NODES + node];
  A.M.col[mbase + node] = (int16_t)((cs >> (8 * slot)) & 0xff);
  A.M.bin[mbase + node] = (uint8_t)w_bin[slot];
  const uint32_t l0 = w_l0[slot], l1 = w_l1[slot];
  const size_t lc = mbase + 2 * node + 1, rc = lc + 1;
  A.M.n0[lc] = l0, A.M.n1[lc] = l1, A.M.value[lc] = fo_value(cw0, cw1, l0, l1);
  A.M.n0[rc] = N0 - l0, A.M.n1[rc] = N1 - l1, A.M.value[rc] = fo_value(cw0, cw1, N0 - l0, N1 - l1);
}

// proba[p, row]: one thread per row walks the T heaps of forest p
__global__ __launch_bounds__(FO_NT) void forest_predict_kernel(const uint8_t *__restrict__ bins, int64_t n, int T,
                                                               int max_depth, FoModel M, double *__restrict__ proba) {
  __shared__ uint32_t rows[FO_NT * FO_LS];
  const int tid = threadIdx.x, p = blockIdx.y;
  const int64_t row0 = (int64_t)blockIdx.x * FO_NT;
  const int nrows = (int)(n - row0 < FO_NT ? n - row0 : FO_NT);
  const uint32_t *src = reinterpret_cast<const uint32_t *>(bins) + row0 * (ASL_FOREST_ROW / 4);
  for (int i = tid; i < nrows * (ASL_FOREST_ROW / 4); i += FO_NT) rows[(i >> 4) * FO_LS + (i & 15)] = src[i];
  __syncthreads();
  if (tid >= nrows) return;
  double sum = 0.0;
  for (int t = 0; t < T; ++t) {
    const size_t mbase = ((size_t)p * T + t) * ASL_FOREST_NODES;
    unsigned node = 0;
    for (int l = 0; l < max_depth; ++l) {
      const int c = M.col[mbase + node];
      if (c < 0) break;
      node = 2 * node + 1 + (fo_byte(rows, tid, c) > M.bin[mbase + node] ? 1u : 0u);
    }
    sum += M.value[mbase + node];
  }
  proba[(size_t)p * n + row0 + tid] = sum / (double)T;
}

namespace {

int64_t forest_workspace = 1ll << 31;

struct ForestWork {
  DevBuf<uint32_t> mult, hist;
  DevBuf<uint8_t> cols;
  DevBuf<uint16_t> state;
  DevBuf<double> cw, edges;
  DevBuf<int32_t> n_edges;
};
ForestWork &fwork() {
  static ForestWork w;
  return w;
}

int fo_mtry(int d) {
  int m = 1;
  while ((m + 1) * (m + 1) <= d) ++m;
  return m;
}

// the five arrays of a model, wherever they live
struct ModelOut {
  Out<int16_t> col;
  Out<uint8_t> bin;
  Out<uint32_t> n0, n1;
  Out<double> value;
  int init(const asl_forest_model_t *m, size_t cnt) {
    ASL_TRY(col.init(m->col, cnt));
    ASL_TRY(bin.init(m->bin, cnt));
    ASL_TRY(n0.init(m->n0, cnt));
    ASL_TRY(n1.init(m->n1, cnt));
    return value.init(m->value, cnt);
  }
  FoModel dev() { return FoModel{col.d, bin.d, n0.d, n1.d, value.d}; }
  int finish() {
    ASL_TRY(col.finish());
    ASL_TRY(bin.finish());
    ASL_TRY(n0.finish());
    ASL_TRY(n1.finish());
    return value.finish();
  }
};

}  // namespace
}  // namespace asl

using namespace asl;

extern "C" int64_t asl_set_forest_workspace(int64_t bytes) {
  clear_error();
  if (bytes <= 0) return fail(ASL_ERR_INVALID, "set_forest_workspace: the budget must be positive");
  const int64_t prev = forest_workspace;
  forest_workspace = bytes;
  return prev;
}

extern "C" int asl_forest_bin(const double *X, int64_t n, int32_t d, const double *edges, const int32_t *n_edges,
                              uint8_t *out) {
  clear_error();
  ASL_TRY(check_shape("forest_bin", n, d, 1, true));
  if (!edges || !n_edges) return fail(ASL_ERR_INVALID, "forest_bin: null edges / n_edges");
  if (n > 0 && (!X || !out)) return fail(ASL_ERR_INVALID, "forest_bin: null X / out");
  ASL_TRY(ensure_device());
  std::vector<int32_t> h_ne;
  ASL_TRY(host_copy(h_ne, n_edges, (size_t)d));
  for (int j = 0; j < d; ++j)
    if (h_ne[j] < 0 || h_ne[j] > ASL_FOREST_MAX_BINS - 1)
      return fail(ASL_ERR_INVALID, "forest_bin: n_edges[%d] = %d, not in 0 .. %d", j, h_ne[j],
                  ASL_FOREST_MAX_BINS - 1);
  if (n == 0) return ASL_OK;
  ForestWork &W = fwork();
  In<double> iX;
  Out<uint8_t> o;
  ASL_TRY(iX.init(X, (size_t)n * d));
  ASL_TRY(o.init(out, (size_t)n * ASL_FOREST_ROW));
  ASL_TRY(W.edges.upload(edges, (size_t)d * (ASL_FOREST_MAX_BINS - 1)));
  ASL_TRY(W.n_edges.upload(h_ne.data(), (size_t)d));
  {
    ProfScope ps("forest_bin");
    hipLaunchKernelGGL(forest_bin_kernel, grid_2d(cdiv(n * ASL_FOREST_ROW, FO_NT)), dim3(FO_NT), 0, stream(), iX.d, n,
                       d, W.edges.p, W.n_edges.p, o.d);
    ASL_CHECK_LAUNCH();
  }
  ASL_TRY(o.finish());
  ASL_TRY(sync_stream());
  return ASL_OK;
}

extern "C" int asl_forest_fit(const uint8_t *bins, int64_t n, int32_t d, const int8_t *label, const double *cw,
                              int32_t P, const int32_t *n_bins, const asl_forest_params_t *params,
                              asl_forest_model_t *model) {
  clear_error();
  if (!cw || !params || !model || !model->col || !model->bin || !model->n0 || !model->n1 || !model->value)
    return fail(ASL_ERR_INVALID, "forest_fit: null argument");
  ASL_TRY(check_shape("forest_fit", n, d, P, true));
  const int T = params->trees, D = params->max_depth;
  if (T > ASL_FOREST_MAX_TREES) return fail(ASL_ERR_CAPACITY, "forest_fit: trees = %d, at most %d", T, ASL_FOREST_MAX_TREES);
  if (D > ASL_FOREST_MAX_DEPTH)
    return fail(ASL_ERR_CAPACITY, "forest_fit: max_depth = %d, at most %d", D, ASL_FOREST_MAX_DEPTH);
  if (T < 1 || D < 1) return fail(ASL_ERR_INVALID, "forest_fit: needs trees >= 1 and max_depth >= 1");
  if (n > 0 && (!bins || !label)) return fail(ASL_ERR_INVALID, "forest_fit: null bins / label");
  ASL_TRY(ensure_device());
  std::vector<double> h_cw;
  ASL_TRY(host_copy(h_cw, cw, (size_t)P * 2));
  ASL_TRY(check_class_weights("forest_fit", h_cw));
  std::vector<int32_t> h_nb(d, ASL_FOREST_MAX_BINS);
  if (n_bins) ASL_TRY(host_copy(h_nb, n_bins, (size_t)d));
  for (int j = 0; j < d; ++j)
    if (h_nb[j] < 1 || h_nb[j] > ASL_FOREST_MAX_BINS)
      return fail(ASL_ERR_INVALID, "forest_fit: n_bins[%d] = %d, not in 1 .. %d", j, h_nb[j], ASL_FOREST_MAX_BINS);
  ASL_TRY(check_labels("forest_fit", label, P, n));   // ... and the bins: on the host, before anything is launched
  if (n_bins) {
    std::vector<uint8_t> h_bins;
    const uint8_t *bp = bins;
    if (n && is_device_ptr(bins)) {
      ASL_TRY(host_copy(h_bins, bins, (size_t)n * ASL_FOREST_ROW));
      bp = h_bins.data();
    }
    for (int64_t i = 0; i < n; ++i)
      for (int j = 0; j < d; ++j)
        if (bp[i * ASL_FOREST_ROW + j] >= h_nb[j])
          return fail(ASL_ERR_INVALID, "forest_fit: bins[%lld, %d] = %d, the column has %d bins", (long long)i, j,
                      (int)bp[i * ASL_FOREST_ROW + j], h_nb[j]);
  }
  ForestWork &W = fwork();
  int cus = 0;
  ASL_TRY(cu_count(&cus));
  const int mtry = fo_mtry(d);
  const int64_t pairs = (int64_t)P * T;
  const size_t total = (size_t)pairs * ASL_FOREST_NODES;
  In<uint8_t> iB;
  In<int8_t> iL;
  ModelOut mo;
  ASL_TRY(iB.init(bins, (size_t)n * ASL_FOREST_ROW));
  ASL_TRY(iL.init(label, (size_t)P * (size_t)n));
  ASL_TRY(mo.init(model, total));
  FoArgs A{};
  A.M = mo.dev();
  hipLaunchKernelGGL(forest_init_kernel, grid_2d(cdiv((int64_t)total, FO_NT)), dim3(FO_NT), 0, stream(), A.M,
                     (int64_t)total);
  ASL_CHECK_LAUNCH();
  if (n > 0) {
    // what one pair holds while its deepest level is grown: the rows' nodes and that level's histograms
    const size_t hist_pair = ((size_t)1 << (D - 1)) * mtry * FO_HBINS;
    const size_t per_pair = (size_t)n * sizeof(uint16_t) + hist_pair * sizeof(uint32_t);
    const int64_t B = std::max<int64_t>(1, std::min<int64_t>(pairs, forest_workspace / (int64_t)per_pair));
    ASL_TRY(W.cw.upload(h_cw.data(), h_cw.size()));
    ASL_TRY(W.mult.reserve((size_t)T * n));
    ASL_TRY(W.cols.reserve((size_t)T * ASL_FOREST_NODES * FO_SLOTS));
    ASL_TRY(W.state.reserve((size_t)B * n));
    ASL_TRY(W.hist.reserve((size_t)B * hist_pair));
    HIP_TRY(hipMemsetAsync(W.mult.p, 0, (size_t)T * n * sizeof(uint32_t), stream()));
    {
      ProfScope ps("forest_draws");
      hipLaunchKernelGGL(forest_bootstrap_kernel, dim3((unsigned)cdiv(n, FO_NT), (unsigned)T), dim3(FO_NT), 0, stream(),
                         W.mult.p, n, params->seed);
      ASL_CHECK_LAUNCH();
      hipLaunchKernelGGL(forest_columns_kernel, dim3((unsigned)cdiv((int64_t)T * ASL_FOREST_NODES, FO_NT)), dim3(FO_NT),
                         0, stream(), W.cols.p, T, d, mtry, params->seed);
      ASL_CHECK_LAUNCH();
    }
    A.bins = iB.d, A.n = n, A.d = d, A.mtry = mtry, A.T = T, A.label = iL.d, A.cw = W.cw.p, A.mult = W.mult.p;
    A.cols = W.cols.p, A.state = W.state.p, A.hist = W.hist.p;
    const int64_t row_blocks = cdiv(n, FO_ROWS);
    for (int64_t q0 = 0; q0 < pairs; q0 += B) {
      A.q0 = (int32_t)q0, A.nq = (int32_t)std::min<int64_t>(B, pairs - q0);
      // pairs per workgroup: every staged row serves them all; enough workgroups to fill the chip
      const int64_t want_y = std::min<int64_t>(A.nq, std::max<int64_t>(1, cdiv(2 * cus, row_blocks)));
      A.group = (int32_t)cdiv(A.nq, want_y);
      const unsigned gy = (unsigned)cdiv(A.nq, A.group);
      for (int level = 0; level < D; ++level) {
        A.level = level;
        const size_t cnt = (size_t)A.nq * ((size_t)1 << level) * mtry * FO_HBINS;
        HIP_TRY(hipMemsetAsync(W.hist.p, 0, cnt * sizeof(uint32_t), stream()));
        {
          ProfScope ps("forest_hist");
          if (level < FO_LDS_LEVELS)
            hipLaunchKernelGGL(forest_hist_kernel<true>, dim3((unsigned)row_blocks, gy), dim3(FO_NT), 0, stream(), A);
          else
            hipLaunchKernelGGL(forest_hist_kernel<false>, dim3((unsigned)row_blocks, gy), dim3(FO_NT), 0, stream(), A);
          ASL_CHECK_LAUNCH();
        }
        {
          ProfScope ps("forest_split");
          hipLaunchKernelGGL(forest_split_kernel, dim3(1u << level, (unsigned)A.nq), dim3(FO_SPLIT_NT), 0, stream(), A);
          ASL_CHECK_LAUNCH();
        }
      }
    }
  }
  model->trees = T, model->max_depth = D;
  ASL_TRY(mo.finish());
  ASL_TRY(sync_stream());
  return ASL_OK;
}

extern "C" int asl_forest_predict(const uint8_t *bins, int64_t n, int32_t d, const asl_forest_model_t *model,
                                  int32_t P, int32_t max_depth, double *proba) {
  clear_error();
  if (!model || !model->col || !model->bin || !model->n0 || !model->n1 || !model->value)
    return fail(ASL_ERR_INVALID, "forest_predict: null model");
  ASL_TRY(check_shape("forest_predict", n, d, P, true));
  const int T = model->trees;
  if (T > ASL_FOREST_MAX_TREES)
    return fail(ASL_ERR_CAPACITY, "forest_predict: trees = %d, at most %d", T, ASL_FOREST_MAX_TREES);
  if (max_depth > ASL_FOREST_MAX_DEPTH)
    return fail(ASL_ERR_CAPACITY, "forest_predict: max_depth = %d, at most %d", max_depth, ASL_FOREST_MAX_DEPTH);
  if (T < 1 || max_depth < 0) return fail(ASL_ERR_INVALID, "forest_predict: needs trees >= 1 and max_depth >= 0");
  if (n == 0) return ASL_OK;
  if (!bins || !proba) return fail(ASL_ERR_INVALID, "forest_predict: null bins / proba");
  ASL_TRY(ensure_device());
  const size_t total = (size_t)P * T * ASL_FOREST_NODES;
  In<uint8_t> iB, mbin;
  In<int16_t> mcol;
  In<double> mval;
  Out<double> o;
  ASL_TRY(iB.init(bins, (size_t)n * ASL_FOREST_ROW));
  ASL_TRY(mcol.init(model->col, total));
  ASL_TRY(mbin.init(model->bin, total));
  ASL_TRY(mval.init(model->value, total));
  ASL_TRY(o.init(proba, (size_t)P * (size_t)n));
  FoModel M{const_cast<int16_t *>(mcol.d), const_cast<uint8_t *>(mbin.d), nullptr, nullptr,
            const_cast<double *>(mval.d)};
  {
    ProfScope ps("forest_predict");
    hipLaunchKernelGGL(forest_predict_kernel, dim3((unsigned)cdiv(n, FO_NT), (unsigned)P), dim3(FO_NT), 0, stream(),
                       iB.d, n, T, max_depth, M, o.d);
    ASL_CHECK_LAUNCH();
  }
  ASL_TRY(o.finish());
  ASL_TRY(sync_stream());
  return ASL_OK;
}
