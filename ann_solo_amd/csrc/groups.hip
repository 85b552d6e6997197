// groups.hip -- mass-difference groups of the open level (asl_ssm_groups): fdr.ssm_groups on the device.
// gfx950 only. DESIGN.md 3 "Mass-difference groups"; the semantics are written out in include/annsolo_mi.h.
//
//   range    min / max of rint(md) and a non-finite flag: per-block partials, folded by a second launch
//   hist     int32 [span][100] counts, one thread per SSM; the lanes of a wave that hit one counter are combined
//            (match loop over the wave's distinct counters) before the global atomic
//   peaks    one wavefront per interval: the 100 counts in LDS, the peaks (scipy's _local_maxima_1d), their bases
//            (peak_prominences, wlen = None); per interval the peak count and (peak, left base, right base) bytes
//   scan     exclusive scan of the peak counts over the span, one workgroup
//   assign   one thread per SSM walks its interval's peaks: the nearest left bin edge among the enclosing bases;
//            the id's size by the same per-wave combining; the peaks' masses by one thread per peak
//   fold     ids of fewer than min_group_size SSMs -> -1; the labels that remain are counted
//
// Integer atomics only (the counts: the order of the adds is not seen); no kernel waits on another workgroup; no
// floating-point sum. The fp64 work is comparisons against edges formed by one rounded product and one rounded sum
// (__dmul_rn / __dadd_rn: never an FMA) and one rounded difference per (SSM, peak): the bytes are the host code's.
#include <algorithm>
#include <cmath>

#include "device_scan.hpp"

namespace asl {

constexpr int GR_NT = 256;                    // threads of the per-SSM kernels (4 waves)
constexpr int GR_BINS = 100;                  // bins of an interval
constexpr int GR_MAX_PEAKS = 49;              // strict local maxima among bins 1 .. 98
constexpr int GR_RANGE_BLOCKS = 1024;         // most partials of the range pass
static_assert(GR_NT == SCAN_NT, "groups_scan_kernel's rounds are block_scan's blocks");

// edge i of the interval of nominal value g, as numpy.linspace(g - 0.5, g + 0.5, 101) forms it
__device__ __forceinline__ double gr_edge(double g, int i) {
  if (i >= GR_BINS) return __dadd_rn(g, 0.5);
  return __dadd_rn(__dmul_rn((double)i, 0.01), __dadd_rn(g, -0.5));
}

// the bin of md in the interval of g: edge[i] <= md < edge[i + 1], bin 99 closed on the right
__device__ __forceinline__ int gr_bin(double g, double md) {
  const double t = __dmul_rn(__dadd_rn(md, -__dadd_rn(g, -0.5)), 100.0);
  int i = t >= 99.0 ? 99 : (t > 0.0 ? (int)t : 0);
  while (i > 0 && md < gr_edge(g, i)) --i;
  while (i < GR_BINS - 1 && md >= gr_edge(g, i + 1)) ++i;
  return i;
}

// tab[key] += the number of lanes that hold key, one atomic per distinct key of the wave. Every lane of the wave
// must arrive (want = false for a lane without a key).
__device__ __forceinline__ void wave_combined_add(uint32_t *__restrict__ tab, uint32_t key, bool want) {
  const int lane = threadIdx.x & 63;
  for (;;) {
    const uint64_t open = __ballot(want);
    if (open == 0ull) break;                               // (uniform over the wave)
    const int leader = __ffsll((unsigned long long)open) - 1;
    const uint32_t k = (uint32_t)__shfl((int)key, leader, 64);
    const bool mine = want && key == k;
    const uint64_t same = __ballot(mine);
    if (mine) {
      if (lane == leader) atomicAdd(&tab[k], (uint32_t)__popcll(same));
      want = false;
    }
  }
}

// ---------------------------------------------------------------------------------------------- range
// partial[b] = (min nominal, max nominal) over the finite md of block b's rows; flag[b] = 1 where one is not finite
__global__ __launch_bounds__(GR_NT) void groups_range_kernel(const double *__restrict__ md, int64_t n,
                                                             double *__restrict__ partial,
                                                             uint32_t *__restrict__ flag) {
  __shared__ double lo_s[GR_NT / 64], hi_s[GR_NT / 64];
  __shared__ uint32_t bad_s[GR_NT / 64];
  double lo = INFINITY, hi = -INFINITY;
  uint32_t bad = 0u;
  for (int64_t i = (int64_t)blockIdx.x * GR_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * GR_NT) {
    const double v = md[i];
    if (!isfinite(v)) {
      bad = 1u;
    } else {
      const double g = rint(v);
      lo = fmin(lo, g);
      hi = fmax(hi, g);
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    lo = fmin(lo, __shfl_down(lo, d, 64));
    hi = fmax(hi, __shfl_down(hi, d, 64));
    bad |= (uint32_t)__shfl_down((int)bad, d, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lo_s[wave] = lo, hi_s[wave] = hi, bad_s[wave] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < GR_NT / 64; ++w) lo = fmin(lo, lo_s[w]), hi = fmax(hi, hi_s[w]), bad |= bad_s[w];
    partial[2 * blockIdx.x] = lo;
    partial[2 * blockIdx.x + 1] = hi;
    flag[blockIdx.x] = bad;
  }
}

// one block: range[0 .. 1] = (min, max) over the partials, range_flag[0] = any flag
__global__ __launch_bounds__(GR_NT) void groups_range_fold_kernel(const double *__restrict__ partial,
                                                                  const uint32_t *__restrict__ flag, int blocks,
                                                                  double *__restrict__ range,
                                                                  uint32_t *__restrict__ range_flag) {
  __shared__ double lo_s[GR_NT], hi_s[GR_NT];
  __shared__ uint32_t bad_s[GR_NT];
  double lo = INFINITY, hi = -INFINITY;
  uint32_t bad = 0u;
  for (int b = threadIdx.x; b < blocks; b += GR_NT) {
    lo = fmin(lo, partial[2 * b]);
    hi = fmax(hi, partial[2 * b + 1]);
    bad |= flag[b];
  }
  lo_s[threadIdx.x] = lo, hi_s[threadIdx.x] = hi, bad_s[threadIdx.x] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int t = 1; t < GR_NT; ++t) lo = fmin(lo, lo_s[t]), hi = fmax(hi, hi_s[t]), bad |= bad_s[t];
    range[0] = lo;
    range[1] = hi;
    range_flag[0] = bad;
  }
}

// ---------------------------------------------------------------------------------------------- histogram
// the row of an SSM's interval, or -1 outside 0 .. span - 1 (cannot happen while md is what the range pass read)
__device__ __forceinline__ int gr_row(double g, double g_min, int span) {
  const double r = __dadd_rn(g, -g_min);        // both integers, |r| < 2^16: exact
  return (r >= 0.0 && r < (double)span) ? (int)r : -1;
}

__global__ __launch_bounds__(GR_NT) void groups_hist_kernel(const double *__restrict__ md, int64_t n, double g_min,
                                                            int span, uint32_t *__restrict__ hist) {
  const int64_t i = (int64_t)blockIdx.x * GR_NT + threadIdx.x;
  bool want = i < n;
  uint32_t key = 0u;
  if (want) {
    const double v = md[i], g = rint(v);
    const int row = gr_row(g, g_min, span);
    want = row >= 0;
    if (want) key = (uint32_t)row * GR_BINS + (uint32_t)gr_bin(g, v);
  }
  wave_combined_add(hist, key, want);
}

// ---------------------------------------------------------------------------------------------- peaks
// One wavefront (one block of 64) per interval. count[row] = its peaks; trip[row][p] = (peak, left base, right base).
__global__ __launch_bounds__(64) void groups_peaks_kernel(const uint32_t *__restrict__ hist, int span,
                                                          uint32_t *__restrict__ count, uint8_t *__restrict__ trip) {
  __shared__ uint32_t x[GR_BINS];
  __shared__ uint8_t pk[64];
  const int row = blockIdx.x, lane = threadIdx.x;
  const uint32_t *h = hist + (int64_t)row * GR_BINS;
  const uint32_t c0 = h[lane], c1 = lane + 64 < GR_BINS ? h[lane + 64] : 0u;
  if (__ballot((c0 | c1) != 0u) == 0ull) {      // an empty interval (uniform over the block)
    if (lane == 0) count[row] = 0u;
    return;
  }
  x[lane] = c0;
  if (lane + 64 < GR_BINS) x[lane + 64] = c1;
  __syncthreads();
  if (row == span - 1) {     // the reference never closes a last interval of one SSM (and so never a single SSM)
    uint64_t sum = 0;
    for (int b = 0; b < GR_BINS; ++b) sum += x[b];
    if (sum == 1) {
      if (lane == 0) count[row] = 0u;
      return;
    }
  }
  // a peak: a plateau that starts above its left neighbour and ends above its right one, before bin 99
  int n_pk = 0;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int i = lane + 64 * r;
    bool peak = false;
    int mid = 0;
    if (i >= 1 && i < GR_BINS - 1 && x[i - 1] < x[i]) {
      int ahead = i + 1;
      while (ahead < GR_BINS - 1 && x[ahead] == x[i]) ++ahead;
      peak = x[ahead] < x[i];
      mid = (i + ahead - 1) / 2;
    }
    const uint64_t m = __ballot(peak);
    const int rank = n_pk + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                           __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (peak && rank < GR_MAX_PEAKS) pk[rank] = (uint8_t)mid;
    n_pk += (int)__popcll(m);
  }
  n_pk = min(n_pk, GR_MAX_PEAKS);               // (49 is the most 98 bins can hold)
  __syncthreads();
  if (lane < n_pk) {
    const int p = pk[lane];
    const uint32_t top = x[p];
    int lb = p, rb = p;
    uint32_t low = top;
    for (int i = p; i >= 0 && x[i] <= top; --i)
      if (x[i] < low) low = x[i], lb = i;
    low = top;
    for (int i = p; i < GR_BINS && x[i] <= top; ++i)
      if (x[i] < low) low = x[i], rb = i;
    uint8_t *t = trip + ((int64_t)row * GR_MAX_PEAKS + lane) * 3;
    t[0] = (uint8_t)p, t[1] = (uint8_t)lb, t[2] = (uint8_t)rb;
  }
  if (lane == 0) count[row] = (uint32_t)n_pk;
}

// one block: offs[row] = peaks of the rows before it; counters[0] = all peaks
__global__ __launch_bounds__(GR_NT) void groups_scan_kernel(const uint32_t *__restrict__ count, int span,
                                                            uint32_t *__restrict__ offs,
                                                            unsigned long long *__restrict__ counters) {
  uint32_t carry = 0u;
  for (int base = 0; base < span; base += GR_NT) {
    const int i = base + threadIdx.x;
    const uint32_t own = i < span ? count[i] : 0u;
    uint32_t all;
    const uint32_t incl = block_scan<SumU32>(own, &all);
    if (i < span) offs[i] = carry + incl - own;
    carry += (uint32_t)__builtin_amdgcn_readfirstlane((int)all);   // (the same in every thread: a scalar register)
    __syncthreads();   // (the next round writes block_scan's wave totals)
  }
  if (threadIdx.x == 0) counters[0] = carry;
}

// ---------------------------------------------------------------------------------------------- assignment
// group[i] = the id before folding, or -1; size[id] = SSMs of the id. cap: entries of size (ids stay below it).
__global__ __launch_bounds__(GR_NT) void groups_assign_kernel(const double *__restrict__ md, int64_t n, double g_min,
                                                              int span, const uint32_t *__restrict__ count,
                                                              const uint32_t *__restrict__ offs,
                                                              const uint8_t *__restrict__ trip, int64_t cap,
                                                              int32_t *__restrict__ group,
                                                              uint32_t *__restrict__ size) {
  const int64_t i = (int64_t)blockIdx.x * GR_NT + threadIdx.x;
  int64_t id = -1;
  if (i < n) {
    const double v = md[i], g = rint(v);
    const int row = gr_row(g, g_min, span);
    if (row >= 0) {
      const int n_pk = (int)min(count[row], (uint32_t)GR_MAX_PEAKS);
      const uint8_t *t = trip + (int64_t)row * GR_MAX_PEAKS * 3;
      double best = INFINITY;
      int arg = -1;
      for (int p = 0; p < n_pk; ++p, t += 3) {
        if (gr_edge(g, t[1]) < v && v < gr_edge(g, t[2])) {
          const double dist = fabs(__dadd_rn(gr_edge(g, t[0]), -v));
          if (dist < best) best = dist, arg = p;      // the first of equal distances stays
        }
      }
      if (arg >= 0) id = (int64_t)offs[row] + arg;
      if (id >= cap) id = -1;                         // (never: an id's peak bin holds an SSM of its own)
    }
    group[i] = (int32_t)id;
  }
  wave_combined_add(size, (uint32_t)id, id >= 0);
}

// one thread per (interval, slot): peak_mass[id] = the peak's left bin edge
__global__ __launch_bounds__(64) void groups_mass_kernel(double g_min, const uint32_t *__restrict__ count,
                                                         const uint32_t *__restrict__ offs,
                                                         const uint8_t *__restrict__ trip, int64_t cap,
                                                         double *__restrict__ peak_mass) {
  const int row = blockIdx.x, p = threadIdx.x;
  if (p >= (int)min(count[row], (uint32_t)GR_MAX_PEAKS)) return;
  const int64_t id = (int64_t)offs[row] + p;
  if (id < cap) peak_mass[id] = gr_edge(__dadd_rn(g_min, (double)row), trip[((int64_t)row * GR_MAX_PEAKS + p) * 3]);
}

// ---------------------------------------------------------------------------------------------- fold
__global__ __launch_bounds__(GR_NT) void groups_fold_kernel(int64_t n, int64_t min_size,
                                                            const uint32_t *__restrict__ size,
                                                            int32_t *__restrict__ group) {
  const int64_t i = (int64_t)blockIdx.x * GR_NT + threadIdx.x;
  if (i >= n) return;
  const int32_t id = group[i];
  if (id >= 0 && (int64_t)size[id] < min_size) group[i] = -1;
}

// one thread per id: counters[1] += ids that stay, counters[2] += their SSMs; peak_size[id] where it is asked for
__global__ __launch_bounds__(GR_NT) void groups_labels_kernel(int64_t cap, int64_t min_size,
                                                              const uint32_t *__restrict__ size,
                                                              unsigned long long *__restrict__ counters,
                                                              int64_t *__restrict__ peak_size) {
  const int64_t id = (int64_t)blockIdx.x * GR_NT + threadIdx.x;
  if (id >= cap || id >= (int64_t)counters[0]) return;
  const uint32_t s = size[id];
  if (peak_size != nullptr) peak_size[id] = (int64_t)s;
  if (s != 0u && (int64_t)s >= min_size) {
    atomicAdd(&counters[1], 1ull);
    atomicAdd(&counters[2], (unsigned long long)s);
  }
}

namespace {

// grow-only device workspace of the entry point: 400 bytes per interval of the span, 4 per id
struct GroupsWork {
  DevBuf<double> partial, range;
  DevBuf<uint32_t> flag, hist, count, offs, size;
  DevBuf<uint8_t> trip;
  DevBuf<unsigned long long> counters;
};
GroupsWork &work() {
  static GroupsWork w;
  return w;
}

}  // namespace
}  // namespace asl

using namespace asl;

extern "C" int asl_ssm_groups(const double *mass_diff, int64_t n, int64_t min_group_size, int32_t *group,
                              int64_t *n_peaks, int64_t *n_labels, double *peak_mass, int64_t *peak_size) {
  clear_error();
  if (n >= ((int64_t)1 << 31)) return fail(ASL_ERR_CAPACITY, "ssm_groups: n = %lld, below 2^31", (long long)n);
  if (n < 0) return fail(ASL_ERR_INVALID, "ssm_groups: n < 0");
  if (min_group_size < 0) return fail(ASL_ERR_INVALID, "ssm_groups: min_group_size < 0");
  if (n == 0) {
    if (n_peaks) *n_peaks = 0;
    if (n_labels) *n_labels = 0;
    return ASL_OK;
  }
  if (!mass_diff || !group) return fail(ASL_ERR_INVALID, "ssm_groups: null mass_diff / group");
  ASL_TRY(ensure_device());
  GroupsWork &W = work();
  In<double> iM;
  ASL_TRY(iM.init(mass_diff, (size_t)n));
  const int blocks = (int)std::min<int64_t>(cdiv(n, GR_NT), GR_RANGE_BLOCKS);
  const unsigned n_blocks = (unsigned)cdiv(n, GR_NT);
  ASL_TRY(W.partial.reserve((size_t)2 * GR_RANGE_BLOCKS));
  ASL_TRY(W.flag.reserve((size_t)GR_RANGE_BLOCKS + 1));
  ASL_TRY(W.range.reserve(2));
  ASL_TRY(W.counters.reserve(3));
  ProfScope ps("ssm_groups");
  hipLaunchKernelGGL(groups_range_kernel, dim3((unsigned)blocks), dim3(GR_NT), 0, stream(), iM.d, n, W.partial.p,
                     W.flag.p);
  ASL_CHECK_LAUNCH();
  hipLaunchKernelGGL(groups_range_fold_kernel, dim3(1), dim3(GR_NT), 0, stream(), W.partial.p, W.flag.p, blocks,
                     W.range.p, W.flag.p + GR_RANGE_BLOCKS);
  ASL_CHECK_LAUNCH();
  double h_range[2];
  uint32_t h_flag = 0u;
  HIP_TRY(hipMemcpyAsync(h_range, W.range.p, sizeof(h_range), hipMemcpyDeviceToHost, stream()));
  HIP_TRY(hipMemcpyAsync(&h_flag, W.flag.p + GR_RANGE_BLOCKS, sizeof(h_flag), hipMemcpyDeviceToHost, stream()));
  ASL_TRY(sync_stream());
  if (h_flag != 0u) return fail(ASL_ERR_INVALID, "ssm_groups: a non-finite mass difference");
  const double g_min = h_range[0], span_d = h_range[1] - h_range[0] + 1.0;
  if (!(span_d >= 1.0 && span_d <= (double)ASL_GROUPS_MAX_SPAN))
    return fail(ASL_ERR_CAPACITY, "ssm_groups: nominal mass differences %.17g .. %.17g span more than %d intervals",
                h_range[0], h_range[1], (int)ASL_GROUPS_MAX_SPAN);
  const int span = (int)span_d;
  const int64_t cap = std::min<int64_t>(n, (int64_t)span * GR_MAX_PEAKS);     // ids: a peak's bin holds an SSM
  ASL_TRY(W.hist.reserve((size_t)span * GR_BINS));
  ASL_TRY(W.count.reserve((size_t)span));
  ASL_TRY(W.offs.reserve((size_t)span));
  ASL_TRY(W.trip.reserve((size_t)span * GR_MAX_PEAKS * 3));
  ASL_TRY(W.size.reserve((size_t)cap));
  Out<int32_t> oG;
  Out<double> oM;      // (nullptr where the masses / sizes are not asked for)
  Out<int64_t> oS;
  ASL_TRY(oG.init(group, (size_t)n));
  ASL_TRY(oM.init(peak_mass, (size_t)cap));
  ASL_TRY(oS.init(peak_size, (size_t)cap));
  HIP_TRY(hipMemsetAsync(W.hist.p, 0, (size_t)span * GR_BINS * sizeof(uint32_t), stream()));
  HIP_TRY(hipMemsetAsync(W.size.p, 0, (size_t)cap * sizeof(uint32_t), stream()));
  HIP_TRY(hipMemsetAsync(W.counters.p, 0, 3 * sizeof(unsigned long long), stream()));
  hipLaunchKernelGGL(groups_hist_kernel, dim3(n_blocks), dim3(GR_NT), 0, stream(), iM.d, n, g_min, span, W.hist.p);
  ASL_CHECK_LAUNCH();
  hipLaunchKernelGGL(groups_peaks_kernel, dim3((unsigned)span), dim3(64), 0, stream(), W.hist.p, span, W.count.p,
                     W.trip.p);
  ASL_CHECK_LAUNCH();
  hipLaunchKernelGGL(groups_scan_kernel, dim3(1), dim3(GR_NT), 0, stream(), W.count.p, span, W.offs.p,
                     W.counters.p);
  ASL_CHECK_LAUNCH();
  hipLaunchKernelGGL(groups_assign_kernel, dim3(n_blocks), dim3(GR_NT), 0, stream(), iM.d, n, g_min, span, W.count.p,
                     W.offs.p, W.trip.p, cap, oG.d, W.size.p);
  ASL_CHECK_LAUNCH();
  if (oM.d != nullptr) {
    hipLaunchKernelGGL(groups_mass_kernel, dim3((unsigned)span), dim3(64), 0, stream(), g_min, W.count.p, W.offs.p,
                       W.trip.p, cap, oM.d);
    ASL_CHECK_LAUNCH();
  }
  if (min_group_size > 1) {       // (a size an id has is at least 1)
    hipLaunchKernelGGL(groups_fold_kernel, dim3(n_blocks), dim3(GR_NT), 0, stream(), n, min_group_size, W.size.p,
                       oG.d);
    ASL_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(groups_labels_kernel, dim3((unsigned)cdiv(cap, GR_NT)), dim3(GR_NT), 0, stream(), cap,
                     min_group_size, W.size.p, W.counters.p, oS.d);
  ASL_CHECK_LAUNCH();
  unsigned long long h_counters[3] = {0ull, 0ull, 0ull};
  HIP_TRY(hipMemcpyAsync(h_counters, W.counters.p, sizeof(h_counters), hipMemcpyDeviceToHost, stream()));
  ASL_TRY(oG.finish());
  ASL_TRY(sync_stream());
  const size_t ids = (size_t)std::min<int64_t>((int64_t)h_counters[0], cap);
  ASL_TRY(oM.finish(ids));      // (the ids that exist: known only now)
  ASL_TRY(oS.finish(ids));
  if (ids > 0 && (oM.to_host() || oS.to_host())) ASL_TRY(sync_stream());
  if (n_peaks) *n_peaks = (int64_t)ids;
  if (n_labels) *n_labels = (int64_t)h_counters[1] + ((int64_t)h_counters[2] < n ? 1 : 0);
  return ASL_OK;
}
