// library.hpp -- the library handle (struct asl_library, library.hip) and the descriptor of one batch searched
// against it (SearchBatch): what library.hip, window_search.hip and search.hip share. Private to the library.
#pragma once
#include <algorithm>

#include "rescore.hpp"

struct asl_library {
  int64_t n = 0;
  uint64_t serial = 0;    // unique in the process, never reused: what an index's window key came from
  asl::DevBuf<int32_t> offsets, pcharge;
  asl::DevBuf<float> mz, intensity, pmz32;
  asl::DevBuf<uint8_t> charge, valid;
  asl::DevBuf<double> pmz;
  // One fixed-size SLOT per row: [RowMeta 32 B][mz x n][charge x n][intensity x n]. The rescoring
  // kernels gather the row record and find the row's first ~24 m/z values in the SAME 128-byte line;
  // the address of a row's peaks is row * slot + 32, not a second, dependent look-up (round 5; until
  // then a 32-byte record array and a separately packed record per row: 4.1 lines and two hops per
  // candidate instead of 3 lines and one).
  asl::DevBuf<uint8_t> records;   // n * slot bytes (DevPeaks::records)
  uint32_t slot = 0;         // bytes per row (a multiple of 128)
  asl::DevBuf<float> wcol;     // window column alone, NaN for invalid spectra
  bool has_valid = false;
  // selection (asl_library_set_selection): keep[row] != 0 = selected, and the columns every search reads
  // while it is installed -- wcol_eff: NaN where unselected or invalid, valid_eff: 0 there. sel_gen counts
  // the changes (install, replace, drop): with `serial` it names what an index derived from these columns.
  asl::DevBuf<uint8_t> keep, valid_eff;
  asl::DevBuf<float> wcol_eff;
  bool has_sel = false;
  uint64_t sel_gen = 0;
  const float *window_col() const { return has_sel ? wcol_eff.p : wcol.p; }
  const uint8_t *valid_col() const { return has_sel ? valid_eff.p : has_valid ? valid.p : nullptr; }
  // group id per row (asl_library_set_groups; the *_topn_distinct calls rank one row per group)
  asl::DevBuf<int32_t> group;
  bool has_group = false;
  asl::DevPeaks dev;
  // precursor-sorted view (window search)
  asl::DevBuf<float> sorted_pmz;
  asl::DevBuf<int32_t> sorted_row;
  // scratch
  asl::DevBuf<float> qvec;
  asl::DevBuf<uint2> q_ent;             // the synchronous batch's entry lists, written by the encoder with qvec
  asl::DevBuf<int32_t> q_cnt;
  asl::DevBuf<int32_t> knn, cand, lo, cnt, woff;
  // buffers that cross the two streams of the pipeline, by batch parity
  asl::DevBuf<float> p_qvec[2], p_cD[2];
  asl::DevBuf<int32_t> p_cI[2], p_knn[2], p_cnt[2];
  asl::DevBuf<int32_t> p_rows[2], rows_len;   // lengths of the neighbour rows when the scan applied the precursor filter
  asl::DevBuf<double> p_win[2];         // ASL_TOL_INTERVAL: the batch's intervals when the caller's array is on the host
  asl::DevBuf<uint2> p_ent[2];          // the batch's entry lists: listed by the coarse stage, read by the scan
  bool p_have_ent[2] = {false, false};
  asl::DevBuf<double> pair_score;
  asl::DevBuf<long long> best_slot;
  // tiled window search: per-tile CSR offsets + begins into sorted_row, running best of the batch
  asl::DevBuf<int32_t> wtile, run_row, run_n, tile_n;
  asl::DevBuf<double> run_score, tile_score;
  asl::DevBuf<int> status;
  asl::RescoreScratch rs_scratch;       // per-query flags between the rescoring launches of THIS handle's stream
};

namespace asl {

// the precursor filter / row records of a library handle
inline void library_filter(const asl_library *L, PrecFilter &flt) {
  flt.meta = reinterpret_cast<const RowMeta *>(L->records.p);
  flt.meta_stride = L->slot;
  flt.wcol = L->window_col();
}
inline void batch_filter(const asl_library *L, const asl_search_params_t *P, const double *win, PrecFilter &flt) {
  flt.lib_pmz = L->pmz32.p;
  flt.valid = L->valid_col();
  library_filter(L, flt);
  flt.tol = P->precursor_tol;
  flt.mode = P->precursor_mode;
  flt.charge = P->charge;
  if (P->precursor_mode == ASL_TOL_INTERVAL) flt.interval = win;     // (shares the tolerance's slot)
}

// One batch of asl_search_batch* / asl_rescore_knn*: what is searched, how, and where the results go.
// The params' arguments were checked where the call entered (search.hip: check_batch).
struct SearchBatch {
  asl_library *L = nullptr;
  DevPeaks Q;                           // the staged queries
  const asl_search_params_t *P = nullptr;
  const double *win = nullptr;          // ASL_TOL_INTERVAL: precursor_window on the device, [nq, 2]
  // n_best > 0 (asl_*_topn): outputs [nq, n_best] except n_cand. 0: the single winner -- the same launches
  // at n = 1 with the argmax as the selection. distinct (asl_*_topn_distinct): one row per group
  int n_best = 0;
  bool distinct = false;
  BatchOut out;                         // device pointers
  size_t winners() const { return (size_t)Q.n * (size_t)std::max(n_best, 1); }
  const int32_t *group() const { return distinct ? L->group.p : nullptr; }
  // What the window test reads per query: the queries' precursor m/z or, with ASL_TOL_INTERVAL, the intervals
  const double *window_operand() const { return P->precursor_mode == ASL_TOL_INTERVAL ? win : Q.precursor_mz; }
  // A rescoring request with everything that is the same for every pass over this batch: spectra, scoring
  // (params->allow_shift is the checked score flag word), selection, and the handle's work memory -- read
  // here, so reserve first -- and the batch's outputs. The caller sets the candidate list, the filter and
  // clear_status, and other outputs where a pass writes elsewhere.
  RescoreRequest rescore_request() const {
    return {.Q = Q, .L = L->dev, .tol = P->fragment_mz_tolerance,
            .tol_ppm = (P->allow_shift & ASL_SCORE_FRAGMENT_PPM) ? 1 : 0,
            .allow_shift = (P->allow_shift & ASL_SCORE_SHIFT) ? 1 : 0, .tie_by_row = 1,
            .n_best = n_best, .group = group(),
            .pair_score = L->pair_score.p, .best_slot = L->best_slot.p,
            .scratch = &L->rs_scratch, .status = L->status.p, .out = out};
  }
};

// window_search.hip: the window-only search of a batch (use_ann = 0)
int window_search_device(const SearchBatch &b);

}  // namespace asl
