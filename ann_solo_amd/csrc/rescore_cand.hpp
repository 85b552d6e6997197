// rescore_cand.hpp -- what the two rescoring units share (rescore.hip: scoring, single winner, peak
// matches; rescore_rank.hip: ranked selection, window fold). Internal: the search units see rescore.hpp only.
#pragma once
#include "rescore.hpp"

namespace asl {

enum { RS_STATUS_OK = 0, RS_STATUS_PEAKS = 1, RS_STATUS_MATCHES = 2, RS_STATUS_WINDOW = 4 };

// Candidate addressing: CSR (cand_offsets != null) or fixed stride; the CSR form either lists
// row ids (rows64 / rows32) or, for the window-only modes, is a run of the precursor-sorted view
// per query (win_begin: rescore.hpp, WindowRows).
struct CandView {
  const int64_t *rows64;
  const int32_t *rows32;
  const int32_t *offsets;
  int32_t stride;
  PrecFilter flt;
  // fixed-stride rows whose length the producer wrote (the scans' post-filter, common.hpp:
  // ScanPostFilter): counts[q] >= 0: the row holds that many hits, ALREADY filtered by the
  // precursor window; -1: the row holds `stride` unfiltered hits (filter here, as without counts)
  const int32_t *counts = nullptr;
  const int32_t *win_begin = nullptr;   // WindowRows::begin / sorted_row / valid
  const int32_t *win_rows = nullptr;
  const uint8_t *win_valid = nullptr;
  __device__ __forceinline__ bool prefiltered(int q) const { return counts != nullptr && counts[q] >= 0; }
  // row of query q's slot c if it is a candidate of the query (in range, passes the filter), else -1
  __device__ __forceinline__ long long cand(int q, long long c, double q_pmz, int n_lib) const {
    const long long r = row(q, c);
    return (r >= 0 && r < n_lib && filter_pass(flt, q, q_pmz, r)) ? r : -1;
  }
  __device__ __forceinline__ void range(int q, long long &c0, long long &c1) const {
    if (offsets) {
      c0 = offsets[q];
      c1 = offsets[q + 1];
    } else {
      c0 = (long long)q * stride;
      int len = stride;
      if (counts) {
        const int c = counts[q];
        if (c >= 0) len = c < stride ? c : stride;
      }
      c1 = c0 + len;
    }
  }
  // library row of query q's slot c (-1: none; an invalid row of a window, as window_fill_kernel
  // marks it)
  __device__ __forceinline__ long long row(int q, long long c) const {
    if (win_begin) {
      const int32_t r = win_rows[(long long)win_begin[q] + (c - offsets[q])];
      return (!win_valid || win_valid[r]) ? (long long)r : -1;
    }
    return rows64 ? rows64[c] : (long long)rows32[c];
  }
};

// The kernels' view of a candidate list (the fold of a tiled window search reads rows, not the filter)
inline CandView make_cand_view(const CandList &c, const PrecFilter &filter) {
  CandView cv{c.rows64, c.rows32, c.offsets, c.stride, filter};
  cv.counts = c.offsets ? nullptr : c.row_counts;
  if (c.window) {
    cv.win_begin = c.window->begin;
    cv.win_rows = c.window->sorted_row;
    cv.win_valid = c.window->valid;
  }
  return cv;
}

// The selection of ranked matches (rescore_rank.hip): rescore_device's pass 2 when n_best > 0. Launches
// rescore_topn_kernel<group != nullptr> on the stream; best_cand / best_slot / best_score are [nq, n].
int rescore_select_ranked(const CandView &cv, int nq, int n, const double *pair_score, int tie_by_row,
                          const int32_t *group, int n_lib, int32_t *best_cand, long long *best_slot,
                          double *best_score, int32_t *n_valid);

// The score histogram (rescore_hist.hip): rescore_device's pass after the scoring launches when the request
// carries BatchOut::score_hist. Launches rescore_hist_kernel on the stream; ADDS into hist [nq, ASL_SCORE_HIST_BINS].
int rescore_hist(const CandView &cv, int nq, int64_t total_slots, const double *pair_score, int32_t *hist);

}  // namespace asl
