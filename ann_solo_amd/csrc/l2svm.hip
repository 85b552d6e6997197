// l2svm.hip -- the SSM rescoring model: P L2-regularised squared-hinge linear SVMs over ONE feature matrix
// (asl_l2svm_fit) and the decision function of P models (asl_linear_scores). gfx950 only, all fp64.
//
// Method (DESIGN.md 3 "Rescoring model"): generalised Newton with Armijo backtracking. Per iteration
//   * the Newton pass streams X once: per running problem the weighted Gram matrix sum c x~x~^T, the gradient
//     part sum c r x~ and sum c r^2 over its active rows (x~ = (x, 1), r = y m, c = class weight, m > 0);
//   * the host forms g and H = I + 2 C sum..., solves H s = -g by Cholesky (D <= 64);
//   * the line pass streams X once: f(w~ + t s) for t = 0, 1, 1/2 .. 2^-7 for every problem.
// Both passes: a workgroup owns a fixed contiguous run of rows, walks it in tiles of 64 rows held in LDS
// (a row of X is fetched once and serves every problem), and writes its partial sums to a workspace; a second
// kernel adds the partials in block order. No floating-point atomics: equal inputs give equal bits.
//
// Newton pass, the Gram as 4 x 4 register blocks: the (D x D) upper triangle is cut into 4 x 4 blocks (bi <= bj),
// the gradient into 1 x 4 blocks that read the row (r, 0, 0, 0) from LDS in place of x~[4 bi ..]; a lane owns up
// to three blocks (<= 152 of them at D = 64) for all rows of an item. An item is (problem, row part): with fewer
// running problems than waves the 64 rows of a tile are split among the waves (P = 1: 8 parts), and a wave with
// one item keeps its sums in registers for the whole run of rows; otherwise they are added into the block's
// workspace slot after every tile (L2 traffic of 16 bytes per 64 FMAs).
#include <algorithm>
#include <cmath>

#include "fit_args.hpp"

namespace asl {

constexpr int SV_NW = 8;                       // waves per workgroup
constexpr int SV_NT = SV_NW * 64;
constexpr int SV_ROWS = 64;                    // rows per tile: one per lane in the margin step
constexpr int SV_PRE = 8;                      // prefetch registers per thread: 64 x 63 <= 8 x 512
constexpr int SV_MAXD1 = ASL_SVM_MAX_DIM + 1;  // columns of x~
constexpr int SV_MAXLS = SV_MAXD1 + 2;         // LDS row stride (doubles): even, so rows stay 16-byte aligned
constexpr int SV_NSTEP = 9;                    // t = 0, 1, 1/2 .. 2^-7
constexpr int SV_LINE_W = 16;                  // doubles per (block, problem) of the line pass
static_assert(SV_ROWS * ASL_SVM_MAX_DIM <= SV_PRE * SV_NT, "tile prefetch");

struct SvArgs {
  const double *X;
  int64_t n;
  int32_t d, ls;                 // features; LDS row stride
  const int8_t *label;           // [P, n]
  const double *cw;              // [P, 2]
  const double *wb, *sdir;       // [P, d + 1]: the point, the direction (line pass)
  const int32_t *plist;          // [n_act]: the running problems
  int32_t n_act, n_parts, items; // items = n_act * n_parts; item = part * n_act + pi
  int64_t rows_per_block;
  const uint8_t *blk;            // [n_tri, 2]: (bi, bj) of the Gram blocks
  int32_t n_tri, n_blk, os;      // Gram blocks, Gram + gradient blocks, doubles per item
  double *part;                  // [blocks, items, os]
};

__device__ __forceinline__ void tile_fetch(const double *__restrict__ X, int64_t row0, int rows, int d, int tid,
                                           double (&v)[SV_PRE]) {
  const int cnt = rows * d;
  const double *src = X + row0 * d;
#pragma unroll
  for (int k = 0; k < SV_PRE; ++k) {
    const int e = tid + k * SV_NT;
    v[k] = e < cnt ? src[e] : 0.0;
  }
}
__device__ __forceinline__ void tile_store(double *Z, int rows, int d, int ls, int tid, const double (&v)[SV_PRE]) {
  const int cnt = rows * d;
#pragma unroll
  for (int k = 0; k < SV_PRE; ++k) {
    const int e = tid + k * SV_NT;
    if (e < cnt) {
      const int r = e / d;
      Z[r * ls + (e - r * d)] = v[k];
    }
  }
}
// the tile: zeros, a column of ones at d (rows past the end keep finite values; their weights are zero)
__device__ __forceinline__ void tile_init(double *Z, int d, int ls, int tid) {
  for (int i = tid; i < SV_ROWS * ls; i += SV_NT) Z[i] = (i % ls) == d ? 1.0 : 0.0;
}
// sum over the wave in a fixed order, in every lane
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// w . x_r + b over the tile row of this lane (w wave-uniform)
__device__ __forceinline__ double row_dot(const double *__restrict__ w, const double *zrow, int d) {
  double acc = w[d];
  for (int j = 0; j < d; ++j) acc = fma(w[j], zrow[j], acc);
  return acc;
}

template <int NBL>
__global__ __launch_bounds__(SV_NT) void svm_newton_kernel(SvArgs A) {
  constexpr int Z_SIZE = SV_ROWS * SV_MAXLS;
  constexpr int C_OFF = Z_SIZE, G_OFF = C_OFF + SV_NW * SV_ROWS;
  __shared__ __attribute__((aligned(16))) double S[G_OFF + SV_NW * SV_ROWS * 4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int d = A.d, ls = A.ls, D = d + 1;
  const int64_t row0 = (int64_t)blockIdx.x * A.rows_per_block;
  const int64_t row1 = row0 + A.rows_per_block < A.n ? row0 + A.rows_per_block : A.n;
  tile_init(S, d, ls, tid);
  double *cw_l = S + C_OFF + wave * SV_ROWS;
  const int g_base = G_OFF + wave * SV_ROWS * 4;
  S[g_base + lane * 4 + 1] = 0.0, S[g_base + lane * 4 + 2] = 0.0, S[g_base + lane * 4 + 3] = 0.0;
  // this lane's blocks: where its a-row and b-row start, and the a-row's stride
  int aoff[NBL], astr[NBL], boff[NBL], blk_id[NBL];
#pragma unroll
  for (int s = 0; s < NBL; ++s) {
    const int b = lane + 64 * s;
    blk_id[s] = b < A.n_blk ? b : -1;
    if (b < A.n_tri) {
      aoff[s] = 4 * A.blk[2 * b], astr[s] = ls, boff[s] = 4 * A.blk[2 * b + 1];
    } else if (b < A.n_blk) {
      aoff[s] = g_base, astr[s] = 4, boff[s] = 4 * (b - A.n_tri);
    } else {
      aoff[s] = 0, astr[s] = ls, boff[s] = 0;
    }
  }
  const bool persist = A.items <= SV_NW;   // a wave has one item at the most: sums stay in registers
  double acc[NBL][16];
#pragma unroll
  for (int s = 0; s < NBL; ++s)
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[s][k] = 0.0;
  double qsum = 0.0;
  double pre[SV_PRE];
  {
    const int rows = (int)(row1 - row0 < SV_ROWS ? row1 - row0 : SV_ROWS);
    tile_fetch(A.X, row0, rows, d, tid, pre);
  }
  __syncthreads();
  bool first = true;
  for (int64_t t0 = row0; t0 < row1; t0 += SV_ROWS) {
    const int rows = (int)(row1 - t0 < SV_ROWS ? row1 - t0 : SV_ROWS);
    tile_store(S, rows, d, ls, tid, pre);
    __syncthreads();
    if (t0 + SV_ROWS < row1) {   // the next tile's loads fly under this tile's arithmetic
      const int64_t left = row1 - (t0 + SV_ROWS);
      tile_fetch(A.X, t0 + SV_ROWS, (int)(left < SV_ROWS ? left : SV_ROWS), d, tid, pre);
    }
    for (int item = wave; item < A.items; item += SV_NW) {
      const int pi = item % A.n_act, part = item / A.n_act;
      const int p = __builtin_amdgcn_readfirstlane(A.plist[pi]);
      const int ra = part * SV_ROWS / A.n_parts, rb = (part + 1) * SV_ROWS / A.n_parts;
      // margin step: lane = row
      {
        const int y = lane < rows ? (int)A.label[(int64_t)p * A.n + t0 + lane] : 0;
        const double f = row_dot(A.wb + (int64_t)p * D, S + lane * ls, d);
        const double m = 1.0 - (double)y * f;
        const bool act = y != 0 && m > 0.0 && lane >= ra && lane < rb;
        const double c = act ? A.cw[2 * p + (y > 0 ? 1 : 0)] : 0.0;
        const double r = act ? (double)y * m : 0.0;
        cw_l[lane] = c;
        S[g_base + lane * 4] = r;
        qsum += wave_sum(c * r * r);
      }
      wave_sync();
      for (int r = ra; r < rb; ++r) {
        const double c = cw_l[r];
        if (c == 0.0) continue;
#pragma unroll
        for (int s = 0; s < NBL; ++s) {
          const double2 *ap = reinterpret_cast<const double2 *>(S + aoff[s] + r * astr[s]);
          const double2 *bp = reinterpret_cast<const double2 *>(S + r * ls + boff[s]);
          const double2 a01 = ap[0], a23 = ap[1], b01 = bp[0], b23 = bp[1];
          const double ca[4] = {c * a01.x, c * a01.y, c * a23.x, c * a23.y};
          const double bb[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
          for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int l = 0; l < 4; ++l) acc[s][4 * k + l] = fma(ca[k], bb[l], acc[s][4 * k + l]);
        }
      }
      wave_sync();
      if (!persist) {   // add into the block's slot of this item (this wave alone touches it) and start over
        double *out = A.part + ((int64_t)blockIdx.x * A.items + item) * A.os;
#pragma unroll
        for (int s = 0; s < NBL; ++s) {
          if (blk_id[s] >= 0) {
            double *o = out + blk_id[s] * 16;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
              o[k] = first ? acc[s][k] : o[k] + acc[s][k];
              acc[s][k] = 0.0;
            }
          }
        }
        if (lane == 0) out[A.n_blk * 16] = first ? qsum : out[A.n_blk * 16] + qsum;
        qsum = 0.0;
      }
    }
    first = false;
    __syncthreads();
  }
  if (persist && wave < A.items) {
    double *out = A.part + ((int64_t)blockIdx.x * A.items + wave) * A.os;
#pragma unroll
    for (int s = 0; s < NBL; ++s)
      if (blk_id[s] >= 0)
#pragma unroll
        for (int k = 0; k < 16; ++k) out[blk_id[s] * 16 + k] = acc[s][k];
    if (lane == 0) out[A.n_blk * 16] = qsum;
  }
}

// sums[pi, e] = the partials of problem pi added in block order, then part order
__global__ void svm_reduce_kernel(const double *__restrict__ part, int blocks, int n_act, int n_parts, int width,
                                  double *__restrict__ sums) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_act * width) return;
  const int pi = i / width, e = i - pi * width;
  const int items = n_act * n_parts;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b)
    for (int q = 0; q < n_parts; ++q) s += part[((int64_t)b * items + q * n_act + pi) * width + e];
  sums[i] = s;
}

// line pass: part[block, pi, k] = sum over the block's rows of cw max(0, 1 - y ((w + t_k s) . x~))^2
__global__ __launch_bounds__(SV_NT) void svm_line_kernel(SvArgs A) {
  __shared__ __attribute__((aligned(16))) double Z[SV_ROWS * SV_MAXLS];
  __shared__ double Acc[ASL_SVM_MAX_PROBLEMS][SV_LINE_W];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int d = A.d, ls = A.ls, D = d + 1;
  const int64_t row0 = (int64_t)blockIdx.x * A.rows_per_block;
  const int64_t row1 = row0 + A.rows_per_block < A.n ? row0 + A.rows_per_block : A.n;
  tile_init(Z, d, ls, tid);
  for (int i = tid; i < ASL_SVM_MAX_PROBLEMS * SV_LINE_W; i += SV_NT) (&Acc[0][0])[i] = 0.0;
  double pre[SV_PRE];
  {
    const int rows = (int)(row1 - row0 < SV_ROWS ? row1 - row0 : SV_ROWS);
    tile_fetch(A.X, row0, rows, d, tid, pre);
  }
  __syncthreads();
  for (int64_t t0 = row0; t0 < row1; t0 += SV_ROWS) {
    const int rows = (int)(row1 - t0 < SV_ROWS ? row1 - t0 : SV_ROWS);
    tile_store(Z, rows, d, ls, tid, pre);
    __syncthreads();
    if (t0 + SV_ROWS < row1) {
      const int64_t left = row1 - (t0 + SV_ROWS);
      tile_fetch(A.X, t0 + SV_ROWS, (int)(left < SV_ROWS ? left : SV_ROWS), d, tid, pre);
    }
    for (int pi = wave; pi < A.n_act; pi += SV_NW) {
      const int p = __builtin_amdgcn_readfirstlane(A.plist[pi]);
      const int y = lane < rows ? (int)A.label[(int64_t)p * A.n + t0 + lane] : 0;
      const double fw = row_dot(A.wb + (int64_t)p * D, Z + lane * ls, d);
      const double fs = row_dot(A.sdir + (int64_t)p * D, Z + lane * ls, d);
      const double c = y != 0 ? A.cw[2 * p + (y > 0 ? 1 : 0)] : 0.0;
      double mine = 0.0;
#pragma unroll
      for (int k = 0; k < SV_NSTEP; ++k) {
        const double t = k == 0 ? 0.0 : 1.0 / (double)(1 << (k - 1));
        const double m = 1.0 - (double)y * fma(t, fs, fw);
        const double v = wave_sum(m > 0.0 ? c * m * m : 0.0);
        if (lane == k) mine = v;
      }
      if (lane < SV_NSTEP) Acc[pi][lane] += mine;   // (this wave alone owns row pi)
    }
    __syncthreads();
  }
  for (int i = tid; i < A.n_act * SV_LINE_W; i += SV_NT)
    A.part[(int64_t)blockIdx.x * A.n_act * SV_LINE_W + i] = (&Acc[0][0])[i];
}

// out[p, i] = w_p . x_i + b_p
__global__ __launch_bounds__(SV_NT) void svm_scores_kernel(SvArgs A, double *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) double Z[SV_ROWS * SV_MAXLS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int d = A.d, ls = A.ls, D = d + 1;
  const int64_t row0 = (int64_t)blockIdx.x * A.rows_per_block;
  const int64_t row1 = row0 + A.rows_per_block < A.n ? row0 + A.rows_per_block : A.n;
  tile_init(Z, d, ls, tid);
  double pre[SV_PRE];
  __syncthreads();
  for (int64_t t0 = row0; t0 < row1; t0 += SV_ROWS) {
    const int rows = (int)(row1 - t0 < SV_ROWS ? row1 - t0 : SV_ROWS);
    tile_fetch(A.X, t0, rows, d, tid, pre);
    tile_store(Z, rows, d, ls, tid, pre);
    __syncthreads();
    for (int p = wave; p < A.n_act; p += SV_NW)
      if (lane < rows) out[(int64_t)p * A.n + t0 + lane] = row_dot(A.wb + (int64_t)p * D, Z + lane * ls, d);
    __syncthreads();
  }
}

namespace {

// grow-only device workspace of the two entry points (never freed between calls; no hipMalloc per Newton step)
struct SvmWork {
  DevBuf<double> part, sums, cw, wb, sdir;
  DevBuf<int32_t> plist;
  DevBuf<uint8_t> blk;
};
SvmWork &work() {
  static SvmWork w;
  return w;
}

struct Grid {
  int blocks = 0;
  int64_t rows_per_block = 0;
};
int make_grid(int64_t n, Grid *g) {   // from the CU count, not from n: a fixed run of whole tiles per block
  int cus = 0;
  ASL_TRY(cu_count(&cus));
  const int64_t tiles = cdiv(n, SV_ROWS), per = cdiv(tiles, cus);
  g->blocks = (int)cdiv(tiles, per);
  g->rows_per_block = per * SV_ROWS;
  return ASL_OK;
}

// H s = -g by Cholesky, H symmetric (upper triangle read) and >= I
void newton_direction(std::vector<double> &H, const std::vector<double> &g, int D, std::vector<double> &s) {
  for (int j = 0; j < D; ++j) {   // H = U^T U, U over the upper triangle in place
    for (int k = 0; k < j; ++k)
      for (int c = j; c < D; ++c) H[j * D + c] -= H[k * D + j] * H[k * D + c];
    const double piv = std::sqrt(H[j * D + j]);
    for (int c = j; c < D; ++c) H[j * D + c] /= piv;
  }
  s.assign(D, 0.0);
  for (int j = 0; j < D; ++j) {   // U^T z = -g
    double v = -g[j];
    for (int k = 0; k < j; ++k) v -= H[k * D + j] * s[k];
    s[j] = v / H[j * D + j];
  }
  for (int j = D - 1; j >= 0; --j) {   // U s = z
    double v = s[j];
    for (int k = j + 1; k < D; ++k) v -= H[j * D + k] * s[k];
    s[j] = v / H[j * D + j];
  }
}

}  // namespace
}  // namespace asl

using namespace asl;

extern "C" int asl_l2svm_fit(const double *X, int64_t n, int32_t d, const int8_t *label, const double *cw, int32_t P,
                             const asl_l2svm_params_t *params, double *wb, double *objective, int32_t *n_newton,
                             int32_t *status) {
  clear_error();
  if (!cw || !params || !wb || !objective || !n_newton || !status)
    return fail(ASL_ERR_INVALID, "l2svm_fit: null argument");
  ASL_TRY(check_shape("l2svm_fit", n, d, P, false));
  if (n > 0 && (!X || !label)) return fail(ASL_ERR_INVALID, "l2svm_fit: null X / label");
  const double C = params->C;
  if (!(C >= 0.0) || !std::isfinite(C)) return fail(ASL_ERR_INVALID, "l2svm_fit: C must be finite and >= 0");
  if (!(params->gtol_abs >= 0.0) || !(params->gtol_rel >= 0.0) || params->max_newton < 0)
    return fail(ASL_ERR_INVALID, "l2svm_fit: gtol_abs, gtol_rel and max_newton must be >= 0");
  ASL_TRY(ensure_device());
  const int D = d + 1;
  std::vector<double> h_cw, h_wb;
  ASL_TRY(host_copy(h_cw, cw, (size_t)P * 2));
  ASL_TRY(host_copy(h_wb, wb, (size_t)P * D));
  ASL_TRY(check_class_weights("l2svm_fit", h_cw));
  for (double v : h_wb)
    if (!std::isfinite(v)) return fail(ASL_ERR_INVALID, "l2svm_fit: non-finite starting point");
  ASL_TRY(check_labels("l2svm_fit", label, P, n));
  SvmWork &W = work();
  In<double> iX;
  In<int8_t> iL;
  ASL_TRY(iX.init(X, (size_t)n * d));
  ASL_TRY(iL.init(label, (size_t)P * (size_t)n));
  // the Gram's blocks
  const int nbx = (D + 3) / 4, n_tri = nbx * (nbx + 1) / 2, n_blk = n_tri + nbx, os = n_blk * 16 + 2;
  std::vector<uint8_t> h_blk;
  for (int bi = 0; bi < nbx; ++bi)
    for (int bj = bi; bj < nbx; ++bj) h_blk.push_back((uint8_t)bi), h_blk.push_back((uint8_t)bj);
  Grid G;
  if (n > 0) {
    ASL_TRY(make_grid(n, &G));
    ASL_TRY(W.blk.upload(h_blk.data(), h_blk.size()));
    ASL_TRY(W.cw.upload(h_cw.data(), h_cw.size()));
    ASL_TRY(W.wb.reserve((size_t)P * D));
    ASL_TRY(W.sdir.reserve((size_t)P * D));
    ASL_TRY(W.plist.reserve((size_t)P));
    ASL_TRY(W.sums.reserve((size_t)P * os));
    // (the items of a pass are the running problems, or up to SV_NW row parts of fewer: sized once, for any pass)
    ASL_TRY(W.part.reserve((size_t)G.blocks * std::max<int>(P, SV_NW) * os));
    ASL_TRY(sync_stream());
  }
  SvArgs A{};
  A.X = iX.d, A.n = n, A.d = d, A.ls = 4 * nbx + 2, A.label = iL.d, A.cw = W.cw.p, A.wb = W.wb.p, A.sdir = W.sdir.p;
  A.plist = W.plist.p, A.rows_per_block = G.rows_per_block, A.blk = W.blk.p, A.n_tri = n_tri, A.n_blk = n_blk;
  std::vector<int32_t> h_status(P, -1), h_newton(P, 0);
  std::vector<double> h_obj(P, 0.0), g0(P, -1.0), h_sums, h_s((size_t)P * D), gs(P, 0.0), f0(P, 0.0);
  std::vector<double> H((size_t)D * D), g(D), s;
  std::vector<int32_t> act;
  for (;;) {
    act.clear();
    for (int p = 0; p < P; ++p)
      if (h_status[p] < 0) act.push_back(p);
    if (act.empty()) break;
    const int n_act = (int)act.size();
    h_sums.assign((size_t)n_act * os, 0.0);
    if (n > 0) {   // Newton pass
      A.n_act = n_act, A.n_parts = std::max(1, SV_NW / n_act), A.items = n_act * A.n_parts, A.os = os;
      A.part = W.part.p;
      HIP_TRY(hipMemcpyAsync(W.plist.p, act.data(), n_act * sizeof(int32_t), hipMemcpyHostToDevice, stream()));
      HIP_TRY(hipMemcpyAsync(W.wb.p, h_wb.data(), h_wb.size() * sizeof(double), hipMemcpyHostToDevice, stream()));
      const int nbl = (int)cdiv(n_blk, 64);
      {
        ProfScope ps("l2svm_newton");   // (the pass and the sum of its partials)
        if (nbl == 1)
          hipLaunchKernelGGL(svm_newton_kernel<1>, dim3(G.blocks), dim3(SV_NT), 0, stream(), A);
        else if (nbl == 2)
          hipLaunchKernelGGL(svm_newton_kernel<2>, dim3(G.blocks), dim3(SV_NT), 0, stream(), A);
        else
          hipLaunchKernelGGL(svm_newton_kernel<3>, dim3(G.blocks), dim3(SV_NT), 0, stream(), A);
        ASL_CHECK_LAUNCH();
        hipLaunchKernelGGL(svm_reduce_kernel, dim3((unsigned)cdiv((int64_t)n_act * os, 256)), dim3(256), 0, stream(),
                           W.part.p, G.blocks, n_act, A.n_parts, os, W.sums.p);
        ASL_CHECK_LAUNCH();
      }
      HIP_TRY(hipMemcpyAsync(h_sums.data(), W.sums.p, h_sums.size() * sizeof(double), hipMemcpyDeviceToHost,
                             stream()));
      ASL_TRY(sync_stream());
    }
    std::vector<int32_t> line;
    for (int pi = 0; pi < n_act; ++pi) {
      const int p = act[pi];
      const double *sm = h_sums.data() + (size_t)pi * os;
      double *w = h_wb.data() + (size_t)p * D;
      std::fill(H.begin(), H.end(), 0.0);
      for (int t = 0; t < n_tri; ++t) {
        const int bi = h_blk[2 * t], bj = h_blk[2 * t + 1];
        for (int k = 0; k < 4; ++k)
          for (int l = 0; l < 4; ++l) {
            const int j = 4 * bi + k, c = 4 * bj + l;
            if (j <= c && c < D) H[(size_t)j * D + c] = 2.0 * C * sm[t * 16 + 4 * k + l];
          }
      }
      double ww = 0.0, gg = 0.0;
      for (int j = 0; j < D; ++j) {
        H[(size_t)j * D + j] += 1.0;
        g[j] = w[j] - 2.0 * C * sm[(n_tri + j / 4) * 16 + (j & 3)];
        ww += w[j] * w[j];
        gg += g[j] * g[j];
      }
      const double gnorm = std::sqrt(gg);
      h_obj[p] = 0.5 * ww + C * sm[n_blk * 16];
      if (g0[p] < 0.0) g0[p] = gnorm;
      if (gnorm <= std::max(params->gtol_abs, params->gtol_rel * g0[p])) {
        h_status[p] = 0;
        continue;
      }
      if (h_newton[p] >= params->max_newton) {
        h_status[p] = 1;
        continue;
      }
      newton_direction(H, g, D, s);
      double dot = 0.0;
      for (int j = 0; j < D; ++j) h_s[(size_t)p * D + j] = s[j], dot += g[j] * s[j];
      gs[p] = dot;
      line.push_back(p);
    }
    if (line.empty()) continue;
    const int n_line = (int)line.size();
    std::vector<double> h_line((size_t)n_line * SV_LINE_W, 0.0);
    if (n > 0) {   // line pass
      A.n_act = n_line, A.n_parts = 1, A.items = n_line, A.os = SV_LINE_W;
      A.part = W.part.p;
      HIP_TRY(hipMemcpyAsync(W.plist.p, line.data(), n_line * sizeof(int32_t), hipMemcpyHostToDevice, stream()));
      HIP_TRY(hipMemcpyAsync(W.sdir.p, h_s.data(), h_s.size() * sizeof(double), hipMemcpyHostToDevice, stream()));
      {
        ProfScope ps("l2svm_line");
        hipLaunchKernelGGL(svm_line_kernel, dim3(G.blocks), dim3(SV_NT), 0, stream(), A);
        ASL_CHECK_LAUNCH();
        hipLaunchKernelGGL(svm_reduce_kernel, dim3((unsigned)cdiv((int64_t)n_line * SV_LINE_W, 256)), dim3(256), 0,
                           stream(), W.part.p, G.blocks, n_line, 1, SV_LINE_W, W.sums.p);
        ASL_CHECK_LAUNCH();
      }
      HIP_TRY(hipMemcpyAsync(h_line.data(), W.sums.p, h_line.size() * sizeof(double), hipMemcpyDeviceToHost,
                             stream()));
      ASL_TRY(sync_stream());
    }
    for (int pi = 0; pi < n_line; ++pi) {
      const int p = line[pi];
      double *w = h_wb.data() + (size_t)p * D;
      const double *sd = h_s.data() + (size_t)p * D, *fl = h_line.data() + (size_t)pi * SV_LINE_W;
      auto f_at = [&](int k) {
        const double t = k == 0 ? 0.0 : 1.0 / (double)(1 << (k - 1));
        double ww = 0.0;
        for (int j = 0; j < D; ++j) {
          const double v = w[j] + t * sd[j];
          ww += v * v;
        }
        return 0.5 * ww + C * fl[k];
      };
      const double fzero = f_at(0);
      int take = -1;
      for (int k = 1; k < SV_NSTEP && take < 0; ++k) {
        const double t = 1.0 / (double)(1 << (k - 1));
        if (f_at(k) <= fzero + 1e-4 * t * gs[p]) take = k;
      }
      if (take < 0) {
        h_status[p] = 2;
        continue;
      }
      const double t = 1.0 / (double)(1 << (take - 1));
      for (int j = 0; j < D; ++j) w[j] += t * sd[j];
      h_newton[p] += 1;
    }
  }
  ASL_TRY(host_copy_back(wb, h_wb));
  ASL_TRY(host_copy_back(objective, h_obj));
  ASL_TRY(host_copy_back(n_newton, h_newton));
  ASL_TRY(host_copy_back(status, h_status));
  return ASL_OK;
}

extern "C" int asl_linear_scores(const double *X, int64_t n, int32_t d, const double *wb, int32_t P, double *out) {
  clear_error();
  if (!wb) return fail(ASL_ERR_INVALID, "linear_scores: null argument");
  ASL_TRY(check_shape("linear_scores", n, d, P, false));
  if (n == 0) return ASL_OK;
  if (!X || !out) return fail(ASL_ERR_INVALID, "linear_scores: null X / out");
  ASL_TRY(ensure_device());
  SvmWork &W = work();
  In<double> iX;
  Out<double> o;
  ASL_TRY(iX.init(X, (size_t)n * d));
  ASL_TRY(o.init(out, (size_t)P * (size_t)n));
  ASL_TRY(W.wb.upload(wb, (size_t)P * (d + 1)));
  Grid G;
  ASL_TRY(make_grid(n, &G));
  SvArgs A{};
  A.X = iX.d, A.n = n, A.d = d, A.ls = 4 * ((d + 4) / 4) + 2, A.wb = W.wb.p, A.n_act = P;
  A.rows_per_block = G.rows_per_block;
  {
    ProfScope ps("linear_scores");
    hipLaunchKernelGGL(svm_scores_kernel, dim3(G.blocks), dim3(SV_NT), 0, stream(), A, o.d);
    ASL_CHECK_LAUNCH();
  }
  ASL_TRY(o.finish());
  ASL_TRY(sync_stream());
  return ASL_OK;
}
