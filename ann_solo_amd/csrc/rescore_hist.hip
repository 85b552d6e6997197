// rescore_hist.hip -- the score histogram of a query's candidates (asl_*_topn_hist; rescore_device's
// optional pass after the three scoring launches): how the exact scores of ALL scored slots are
// distributed, of which the selection keeps only the n best. Scoring is in rescore.hip, the selection
// in rescore_rank.hip; neither changes.
#include <algorithm>

#include "common.hpp"
#include "rescore_cand.hpp"

namespace asl {

// Bin of an exact score (annsolo_mi.h: ASL_SCORE_HIST_BINS bins of width 1/128 over [0, 1], lower
// edges inclusive, everything at or above 1 in the top bin). s * 128.0 is exact (a power of two), so
// the bin is floor(128 s).
__device__ __forceinline__ int score_bin(double s) {
  return !(s < 1.0) ? ASL_SCORE_HIST_BINS - 1 : (int)(s * (double)ASL_SCORE_HIST_BINS);
}

// hist[q, bin] += the number of query q's slots whose score falls into the bin. A slot counts exactly
// when the selection kernels count it into n_cand: its pair_score is not negative (the markers of
// filtered, invalid and out-of-range slots are; the request never prunes, so RS_PRUNED does not occur).
//
// One wave per (query, y): the wave takes every gridDim.y-th run of 64 slots of the query's list, a
// coalesced 512-byte read each. The wave's histogram lives in registers: lane b & 63 owns bins b
// and b + 64. Scores cluster in a few low bins, so the 64 bins of a run are resolved per DISTINCT
// value -- the bin of the first unresolved lane is broadcast, the lanes that hold it are balloted
// and the owning lane adds their number -- instead of 64 lanes serialising on one LDS word. At the
// end every lane adds its non-zero counts to the query's row: integer adds, so neither the order of
// the waves that share a row nor that of a tiled window search's passes shows in the result.
__global__ __launch_bounds__(64) void rescore_hist_kernel(CandView cv, int nq, const double *__restrict__ pair_score,
                                                          int32_t *__restrict__ hist) {
  const int q = blockIdx.x;
  const int lane = threadIdx.x;
  long long c0, c1;
  cv.range(q, c0, c1);
  int h_lo = 0, h_hi = 0;
  const long long step = 64ll * gridDim.y;
  for (long long base = c0 + 64ll * blockIdx.y; base < c1; base += step) {     // wave-uniform
    const long long c = base + lane;
    const double s = c < c1 ? pair_score[c] : -1.0;
    const bool live = !(s < 0.0);
    const int bin = score_bin(s);
    unsigned long long todo = __ballot(live);
    while (todo) {                                                             // once per distinct bin
      const int b = __builtin_amdgcn_readlane(bin, __builtin_ctzll(todo));
      const unsigned long long same = __ballot(live && bin == b);
      const int cnt = __popcll(same);
      if (lane == (b & 63)) {
        if (b < 64) h_lo += cnt; else h_hi += cnt;
      }
      todo &= ~same;
    }
  }
  int32_t *row = hist + (size_t)q * ASL_SCORE_HIST_BINS;
  if (h_lo) atomicAdd(row + lane, h_lo);
  if (h_hi) atomicAdd(row + 64 + lane, h_hi);
}

// Waves per query: one for the ANN rows (a few hundred slots), several for long lists -- few queries
// whose lists rescore_device splits, or a window tile's hundreds of thousands of slots per query --
// as long as the grid stays within a few waves per SIMD of the device.
int rescore_hist(const CandView &cv, int nq, int64_t total_slots, const double *pair_score, int32_t *hist) {
  if (nq <= 0) return ASL_OK;
  const int64_t avg = total_slots / nq;
  const int64_t want = cdiv(avg, (int64_t)1024), room = cdiv((int64_t)16384, (int64_t)nq);
  const unsigned ny = (unsigned)std::max<int64_t>(1, std::min<int64_t>(std::min(want, room), 1024));
  hipLaunchKernelGGL(rescore_hist_kernel, dim3(nq, ny), dim3(64), 0, stream(), cv, nq, pair_score, hist);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

}  // namespace asl
