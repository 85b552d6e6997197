// tdc.hip -- target-decoy q-values of the FDR step (asl_tdc_qvalues): fdr.tdc_qvalues per group on the device.
// gfx950 only. DESIGN.md 3 "Target-decoy q-values".
//
//   build    every used row -> (group key u32, score key u64, payload = row index | target << 31), compacted;
//            the digit histograms of all 12 key bytes and the NaN flag in the same pass (workspace only)
//   sort     LSD radix sort, 8 bits a pass: per-tile digit counts -> exclusive scan of the (digit-major,
//            tile-minor) counts -> stable scatter (rank in the wave by ballot match masks + mbcnt, across the
//            waves and rounds of a tile through LDS, across tiles by the scanned offsets). A pass whose byte is
//            the same in every key is skipped.
//   counts   forward scan of (targets so far, position of the group's head) over the sorted order
//   q        reverse min-scan of (group key, FDR at a run's end | +inf): group keys only fall along the reversed
//            order, so the lexicographic minimum IS the minimum inside the current group; its store scatters
//            q[index] and label[index]
//   fill     NaN / 0 into the rows that take no part
//
// Every scan is device_scan.hpp's: reduce -> scan of the block partials (recursively) -> apply, as separate launches
// on the library's stream, so no kernel waits on another workgroup. No floating-point sum or atomic anywhere: the
// counts are integers, a run's end does ONE fp64 division, min is exact. Rows of one (group, score) run get one q,
// so the order a sort leaves inside a run cannot reach the output.
#include <algorithm>
#include <cmath>

#include "device_scan.hpp"

namespace asl {

constexpr int TD_NT = 256;                     // threads of every kernel here (4 waves)
constexpr int TD_TILE = ASL_TDC_TILE;          // keys per sort tile
constexpr int TD_ROUNDS = TD_TILE / TD_NT;     // a thread's keys: element e = round * TD_NT + tid
constexpr int TD_SLOTS = TD_ROUNDS * (TD_NT / 64);
constexpr int TD_PASSES = 12;                  // 8 score bytes, then 4 group bytes
constexpr uint32_t TD_TARGET = 0x80000000u;
static_assert(TD_TILE % TD_NT == 0, "whole rounds");
static_assert(TD_NT == SCAN_NT, "one block size for the sort and the scans");

// ---------------------------------------------------------------------------------------------- scans
struct CountHead {   // s: targets so far; m: the largest head position so far
  uint32_t s, m;
};
struct CountHeadOp {
  using T = CountHead;
  __device__ static T identity() { return {0u, 0u}; }
  __device__ static T op(T a, T b) { return {a.s + b.s, a.m > b.m ? a.m : b.m}; }
};
struct GroupMin {    // lexicographic (group key, bits of a double >= 0)
  uint64_t v;
  uint32_t g, pad;
};
struct GroupMinOp {
  using T = GroupMin;
  __device__ static T identity() { return {~0ull, ~0u, 0u}; }
  __device__ static T op(T a, T b) { return (b.g < a.g || (b.g == a.g && b.v < a.v)) ? b : a; }
};

// the views (device_scan.hpp: an operator, load(i), store(i, inclusive, own))
struct ExclusiveU32View {   // counts -> offsets, in place
  using Op = SumU32;
  uint32_t *a;
  __device__ uint32_t load(int64_t i) const { return a[i]; }
  __device__ void store(int64_t i, uint32_t incl, uint32_t own) const { a[i] = incl - own; }
};
struct UsePosView {   // pos[i] = used rows before row i; *m = their number
  using Op = SumU32;
  const uint8_t *use;
  uint32_t *pos, *m;
  int64_t n;
  __device__ uint32_t load(int64_t i) const { return use[i] != 0 ? 1u : 0u; }
  __device__ void store(int64_t i, uint32_t incl, uint32_t own) const {
    pos[i] = incl - own;
    if (i == n - 1) *m = incl;
  }
};
struct SortedRows {   // the sorted order: gkey may be nullptr (one group)
  const uint64_t *skey;
  const uint32_t *gkey;
  const uint32_t *pay;
  int64_t m;
};
struct CountView {    // forward: ct[i] = targets among sorted rows 0 .. i, hd[i] = where row i's group starts
  using Op = CountHeadOp;
  SortedRows r;
  uint32_t *ct, *hd;
  __device__ CountHead load(int64_t i) const {
    const bool head = i > 0 && r.gkey != nullptr && r.gkey[i] != r.gkey[i - 1];
    return {r.pay[i] >> 31, head ? (uint32_t)i : 0u};
  }
  __device__ void store(int64_t i, CountHead incl, CountHead) const { ct[i] = incl.s, hd[i] = incl.m; }
};
struct QView {        // reversed: element j is sorted row m - 1 - j
  using Op = GroupMinOp;
  SortedRows r;
  const uint32_t *ct, *hd;
  double *q;
  int8_t *label;      // or nullptr
  double fdr;
  __device__ GroupMin load(int64_t j) const {
    const int64_t i = r.m - 1 - j;
    const uint32_t g = r.gkey != nullptr ? r.gkey[i] : 0u;
    bool end = i == r.m - 1 || r.skey[i + 1] != r.skey[i];
    if (!end && r.gkey != nullptr) end = r.gkey[i + 1] != g;
    double v = INFINITY;
    if (end) {        // FDR at the end of a run: (decoys + 1) / targets of the group so far, at most 1
      const uint32_t h = hd[i];
      const uint32_t t = ct[i] - (ct[h] - (r.pay[h] >> 31));
      const uint32_t d = (uint32_t)(i - h + 1) - t;
      v = t != 0u ? fmin((double)(d + 1u) / (double)t, 1.0) : 1.0;
    }
    return {(uint64_t)__double_as_longlong(v), g, 0u};
  }
  __device__ void store(int64_t j, GroupMin incl, GroupMin) const {
    const uint32_t p = r.pay[r.m - 1 - j];
    const uint32_t row = p & ~TD_TARGET;
    const double qv = __longlong_as_double((long long)incl.v);
    q[row] = qv;
    if (label != nullptr) label[row] = (p & TD_TARGET) ? (qv <= fdr ? 1 : 0) : -1;
  }
};

// ---------------------------------------------------------------------------------------------- keys
// ghist: [TD_PASSES, 256] digit counts over the used rows, then [0] of the tail = 1 where a used score is NaN
__global__ __launch_bounds__(TD_NT) void tdc_build_kernel(const double *__restrict__ score,
                                                          const uint8_t *__restrict__ is_target,
                                                          const int32_t *__restrict__ group,
                                                          const uint8_t *__restrict__ use,
                                                          const uint32_t *__restrict__ pos, int64_t n, int desc,
                                                          uint64_t *__restrict__ skey, uint32_t *__restrict__ gkey,
                                                          uint32_t *__restrict__ pay, uint32_t *__restrict__ ghist) {
  __shared__ uint32_t hist[TD_PASSES * 256];
  const int n_pass = group != nullptr ? TD_PASSES : 8;
  for (int k = threadIdx.x; k < n_pass * 256; k += TD_NT) hist[k] = 0u;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * TD_NT + threadIdx.x;
  if (i < n && (use == nullptr || use[i] != 0)) {
    const double s = score[i];
    if (s != s) atomicOr(&ghist[TD_PASSES * 256], 1u);
    uint64_t u = s == 0.0 ? 0ull : (uint64_t)__double_as_longlong(s);   // -0.0 and +0.0 are one run
    u = (u >> 63) ? ~u : (u | 0x8000000000000000ull);   // ascending in the score
    if (desc) u = ~u;
    const uint32_t g = group != nullptr ? (uint32_t)group[i] ^ 0x80000000u : 0u;
    const int64_t o = use != nullptr ? (int64_t)pos[i] : i;
    skey[o] = u;
    if (group != nullptr) gkey[o] = g;
    pay[o] = (uint32_t)i | (is_target[i] != 0 ? TD_TARGET : 0u);
#pragma unroll
    for (int p = 0; p < 8; ++p) atomicAdd(&hist[p * 256 + (int)((u >> (8 * p)) & 255u)], 1u);
    if (group != nullptr) {
#pragma unroll
      for (int p = 0; p < 4; ++p) atomicAdd(&hist[(8 + p) * 256 + (int)((g >> (8 * p)) & 255u)], 1u);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < n_pass * 256; k += TD_NT)
    if (hist[k] != 0u) atomicAdd(&ghist[k], hist[k]);   // (integer counts: the order of the adds is not seen)
}

__device__ __forceinline__ uint32_t key_digit(const uint64_t *__restrict__ skey, const uint32_t *__restrict__ gkey,
                                              int64_t i, int pass) {
  if (pass < 8) return (uint32_t)(skey[i] >> (8 * pass)) & 255u;
  return (gkey[i] >> (8 * (pass - 8))) & 255u;
}

// counts[digit * tiles + tile] = keys of the tile with that digit
__global__ __launch_bounds__(TD_NT) void tdc_hist_kernel(const uint64_t *__restrict__ skey,
                                                         const uint32_t *__restrict__ gkey, int64_t m, int pass,
                                                         int64_t tiles, uint32_t *__restrict__ counts) {
  __shared__ uint32_t hist[256];
  hist[threadIdx.x] = 0u;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * TD_TILE;
#pragma unroll
  for (int r = 0; r < TD_ROUNDS; ++r) {
    const int64_t i = base + r * TD_NT + threadIdx.x;
    if (i < m) atomicAdd(&hist[key_digit(skey, gkey, i, pass)], 1u);
  }
  __syncthreads();
  counts[(int64_t)threadIdx.x * tiles + blockIdx.x] = hist[threadIdx.x];
}

// offs: the exclusive scan of counts. Stable: keys of one digit keep their order (tile, round, thread).
__global__ __launch_bounds__(TD_NT) void tdc_scatter_kernel(const uint64_t *__restrict__ skey,
                                                            const uint32_t *__restrict__ gkey,
                                                            const uint32_t *__restrict__ pay, int64_t m, int pass,
                                                            int64_t tiles, const uint32_t *__restrict__ offs,
                                                            uint64_t *__restrict__ skey_out,
                                                            uint32_t *__restrict__ gkey_out,
                                                            uint32_t *__restrict__ pay_out) {
  __shared__ uint32_t before[TD_SLOTS][256];   // keys of this digit in earlier (round, wave) slots of the tile
  __shared__ uint32_t first[256];              // where the tile's keys of this digit start
  const int tid = threadIdx.x, wave = tid >> 6;
  for (int k = tid; k < TD_SLOTS * 256; k += TD_NT) (&before[0][0])[k] = 0u;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * TD_TILE;
  uint64_t sk[TD_ROUNDS];
  uint32_t gk[TD_ROUNDS], py[TD_ROUNDS], dg[TD_ROUNDS], rank[TD_ROUNDS];
#pragma unroll
  for (int r = 0; r < TD_ROUNDS; ++r) {
    const int64_t i = base + r * TD_NT + tid;
    const bool valid = i < m;
    sk[r] = valid ? skey[i] : 0ull;
    gk[r] = valid && gkey != nullptr ? gkey[i] : 0u;
    py[r] = valid ? pay[i] : 0u;
    dg[r] = pass < 8 ? (uint32_t)(sk[r] >> (8 * pass)) & 255u : (gk[r] >> (8 * (pass - 8))) & 255u;
    uint64_t peers = __ballot(valid);          // the lanes of this wave that hold the same digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (dg[r] >> b) & 1u;
      const uint64_t has = __ballot(bit);
      peers &= bit ? has : ~has;
    }
    rank[r] = __builtin_amdgcn_mbcnt_hi((uint32_t)(peers >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)peers, 0u));
    if (valid && rank[r] == 0u) before[r * (TD_NT / 64) + wave][dg[r]] = (uint32_t)__popcll(peers);
  }
  __syncthreads();
  {
    uint32_t run = 0u;
#pragma unroll
    for (int s = 0; s < TD_SLOTS; ++s) {
      const uint32_t c = before[s][tid];
      before[s][tid] = run;
      run += c;
    }
    first[tid] = offs[(int64_t)tid * tiles + blockIdx.x];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < TD_ROUNDS; ++r) {
    if (base + r * TD_NT + tid < m) {
      const int64_t o = (int64_t)first[dg[r]] + before[r * (TD_NT / 64) + wave][dg[r]] + rank[r];
      skey_out[o] = sk[r];
      if (gkey != nullptr) gkey_out[o] = gk[r];
      pay_out[o] = py[r];
    }
  }
}

// rows that take no part: q = NaN, label = 0
__global__ void tdc_fill_kernel(const uint8_t *__restrict__ use, int64_t n, double *__restrict__ q,
                                int8_t *__restrict__ label) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && use[i] == 0) {
    q[i] = __longlong_as_double(0x7ff8000000000000ll);
    if (label != nullptr) label[i] = 0;
  }
}

namespace {

// grow-only device workspace of the entry point, sized by n (about 40 bytes a row)
struct TdcWork {
  DevBuf<uint64_t> skey[2];
  DevBuf<uint32_t> gkey[2], pay[2];
  DevBuf<uint32_t> ct, hd;        // (ct doubles as the compaction's positions before the sort)
  DevBuf<uint32_t> counts, ghist;
  DevBuf<GroupMin> partial;       // the block partials of every scan level (the widest element)
};
TdcWork &work() {
  static TdcWork w;
  return w;
}

}  // namespace
}  // namespace asl

using namespace asl;

extern "C" int asl_tdc_qvalues(const double *score, const uint8_t *is_target, const int32_t *group,
                               const uint8_t *use, int64_t n, int32_t desc, double fdr, double *q, int8_t *label) {
  clear_error();
  if (n >= ((int64_t)1 << 31)) return fail(ASL_ERR_CAPACITY, "tdc_qvalues: n = %lld, below 2^31", (long long)n);
  if (n < 0) return fail(ASL_ERR_INVALID, "tdc_qvalues: n < 0");
  if (desc != 0 && desc != 1) return fail(ASL_ERR_INVALID, "tdc_qvalues: desc = %d, 0 or 1", (int)desc);
  if (label != nullptr && !(fdr >= 0.0)) return fail(ASL_ERR_INVALID, "tdc_qvalues: fdr must be >= 0");
  if (n == 0) return ASL_OK;
  if (!score || !is_target || !q) return fail(ASL_ERR_INVALID, "tdc_qvalues: null score / is_target / q");
  ASL_TRY(ensure_device());
  TdcWork &W = work();
  In<double> iS;
  In<uint8_t> iT, iU;
  In<int32_t> iG;
  ASL_TRY(iS.init(score, (size_t)n));
  ASL_TRY(iT.init(is_target, (size_t)n));
  ASL_TRY(iG.init(group, (size_t)n));
  ASL_TRY(iU.init(use, (size_t)n));
  const int64_t tiles_max = cdiv(n, TD_TILE);
  for (int b = 0; b < 2; ++b) {
    ASL_TRY(W.skey[b].reserve((size_t)n));
    ASL_TRY(W.pay[b].reserve((size_t)n));
    if (group != nullptr) ASL_TRY(W.gkey[b].reserve((size_t)n));
  }
  ASL_TRY(W.ct.reserve((size_t)n));
  ASL_TRY(W.hd.reserve((size_t)n));
  ASL_TRY(W.counts.reserve((size_t)(256 * tiles_max)));
  ASL_TRY(W.ghist.reserve((size_t)TD_PASSES * 256 + 2));
  ASL_TRY(W.partial.reserve((size_t)(partial_slots(std::max<int64_t>(n, 256 * tiles_max)) + 1)));
  const size_t n_ghist = (size_t)TD_PASSES * 256 + 2;
  uint32_t *m_dev = W.ghist.p + TD_PASSES * 256 + 1;
  ProfScope ps("tdc_qvalues");
  HIP_TRY(hipMemsetAsync(W.ghist.p, 0, n_ghist * sizeof(uint32_t), stream()));
  if (use != nullptr) ASL_TRY(scan_view(UsePosView{iU.d, W.ct.p, m_dev, n}, n, W.partial.p));
  hipLaunchKernelGGL(tdc_build_kernel, dim3((unsigned)cdiv(n, TD_NT)), dim3(TD_NT), 0, stream(), iS.d, iT.d, iG.d,
                     iU.d, W.ct.p, n, (int)desc, W.skey[0].p, group != nullptr ? W.gkey[0].p : nullptr, W.pay[0].p,
                     W.ghist.p);
  ASL_CHECK_LAUNCH();
  std::vector<uint32_t> h_hist(n_ghist);
  HIP_TRY(hipMemcpyAsync(h_hist.data(), W.ghist.p, n_ghist * sizeof(uint32_t), hipMemcpyDeviceToHost, stream()));
  ASL_TRY(sync_stream());
  if (h_hist[TD_PASSES * 256] != 0u) return fail(ASL_ERR_INVALID, "tdc_qvalues: a NaN score in a used row");
  const int64_t m = use != nullptr ? (int64_t)h_hist[TD_PASSES * 256 + 1] : n;
  Out<double> oQ;
  Out<int8_t> oL;
  ASL_TRY(oQ.init(q, (size_t)n));
  ASL_TRY(oL.init(label, (size_t)n));
  if (m > 0) {
    const int64_t tiles = cdiv(m, TD_TILE);
    int cur = 0;
    for (int pass = 0; pass < (group != nullptr ? TD_PASSES : 8); ++pass) {
      bool uniform = false;   // one digit holds every key: the pass would move nothing
      for (int dgt = 0; dgt < 256 && !uniform; ++dgt) uniform = (int64_t)h_hist[pass * 256 + dgt] == m;
      if (uniform) continue;
      const uint32_t *gk = group != nullptr ? W.gkey[cur].p : nullptr;
      hipLaunchKernelGGL(tdc_hist_kernel, dim3((unsigned)tiles), dim3(TD_NT), 0, stream(), W.skey[cur].p, gk, m, pass,
                         tiles, W.counts.p);
      ASL_CHECK_LAUNCH();
      ASL_TRY(scan_view(ExclusiveU32View{W.counts.p}, 256 * tiles, W.partial.p));
      hipLaunchKernelGGL(tdc_scatter_kernel, dim3((unsigned)tiles), dim3(TD_NT), 0, stream(), W.skey[cur].p, gk,
                         W.pay[cur].p, m, pass, tiles, W.counts.p, W.skey[cur ^ 1].p,
                         group != nullptr ? W.gkey[cur ^ 1].p : nullptr, W.pay[cur ^ 1].p);
      ASL_CHECK_LAUNCH();
      cur ^= 1;
    }
    const SortedRows R{W.skey[cur].p, group != nullptr ? W.gkey[cur].p : nullptr, W.pay[cur].p, m};
    ASL_TRY(scan_view(CountView{R, W.ct.p, W.hd.p}, m, W.partial.p));
    ASL_TRY(scan_view(QView{R, W.ct.p, W.hd.p, oQ.d, oL.d, fdr}, m, W.partial.p));
  }
  if (m < n) {
    hipLaunchKernelGGL(tdc_fill_kernel, dim3((unsigned)cdiv(n, TD_NT)), dim3(TD_NT), 0, stream(), iU.d, n, oQ.d,
                       oL.d);
    ASL_CHECK_LAUNCH();
  }
  ASL_TRY(oQ.finish());
  ASL_TRY(oL.finish());
  ASL_TRY(sync_stream());
  return ASL_OK;
}
