// rescore.hpp -- interface of the rescoring driver (rescore.hip): the request, the kernel-argument
// structs and the output staging that window_search.hip and search.hip (through library.hpp) share with it.
#pragma once
#include "common.hpp"

namespace asl {

// Precursor-window post-filter of the candidate lists, evaluated inside the rescoring
// kernel's compaction stage (spectral_library.py:417-429 AND :441-446): a candidate row
// passes if it is valid and within the window of the query's precursor m/z.
// lib_pmz == nullptr switches the filter off.
// Everything the rescoring kernel needs to know about a library row, in one 32-byte sector
// (asl_library: the head of the row's slot, see PrecFilter::meta_stride):
// the candidate filter and the per-candidate metadata cost one random gather each instead of
// one per field (offsets x2, charge, precursor m/z, window column, validity).
struct __attribute__((aligned(32))) RowMeta {
  int32_t off;      // first peak of the spectrum
  int32_t cn;       // number of peaks
  int32_t charge;   // precursor charge
  float pmz32;      // spec_info's float32 precursor m/z column; NaN for invalid spectra
  double pmz64;     // precursor m/z
  uint32_t rec4;    // the spectrum's packed peak record (DevPeaks::records), in 4-byte units
  uint32_t pad;
};

struct PrecFilter {
  const float *lib_pmz = nullptr;   // spec_info's float32 precursor m/z column
  const uint8_t *valid = nullptr;   // is_valid flags (nullptr: all valid)
  // Da / ppm: the tolerance. ASL_TOL_INTERVAL, which reads no tolerance: the queries' intervals on the
  // window column, [nq, 2] (lo, hi) -- the window test reads these, never the query's precursor m/z
  // (which the shifted dot product still uses). One slot, so the kernels' arguments keep their size.
  union {
    double tol = 0.0;
    const double *interval;
  };
  int mode = ASL_TOL_DA;
  int charge = 0;
  const RowMeta *meta = nullptr;    // packed rows (asl_library): replaces lib_pmz / valid
  // bytes from one row's record to the next: sizeof(RowMeta) for a plain array; the library keeps
  // every row record at the head of its row's fixed-size SLOT, right in front of the packed peaks
  // (one gather brings the record AND the first peaks; the peaks' address needs no second hop)
  uint32_t meta_stride = sizeof(RowMeta);
  // the window column alone, NaN for invalid spectra (4 bytes per row: the flat kernel filters
  // 16.7 M slots per batch on it and touches the 32-byte records of the survivors only)
  const float *wcol = nullptr;
  // window-only modes: the candidate rows ARE the window's hits; `meta` is passed for the packed
  // rows (one gather per candidate, one peak record) and nothing is filtered
  bool pass_all = false;
};

__device__ __forceinline__ const RowMeta *meta_row(const PrecFilter &f, long long row) {
  return reinterpret_cast<const RowMeta *>(reinterpret_cast<const char *>(f.meta) + (size_t)row * f.meta_stride);
}

// precursor_ok (spectral_library.py:421-427): common.hpp -- the scans' finish applies it too

// the window test of query q on a row's window value
__device__ __forceinline__ bool window_pass(const PrecFilter &f, int q, double q_pmz, float key) {
  if (f.mode == ASL_TOL_INTERVAL) return precursor_ok(query_window(f.interval, q, f.mode), key, f.charge, 0.0, f.mode);
  return precursor_ok(q_pmz, key, f.charge, f.tol, f.mode);
}

__device__ __forceinline__ bool filter_pass(const PrecFilter &f, int q, double q_pmz, long long row) {
  if (f.pass_all) return true;
  if (f.wcol) return window_pass(f, q, q_pmz, f.wcol[row]);
  if (f.meta) return window_pass(f, q, q_pmz, meta_row(f, row)->pmz32);
  if (!f.lib_pmz) return true;
  if (f.valid && !f.valid[row]) return false;
  return window_pass(f, q, q_pmz, f.lib_pmz[row]);
}

// Per-query flags that pass from one rescoring launch to the next (which queries the flat kernel
// left to the binary-search kernel, which winners the small matches kernel left to the full-size
// one). Owned by whoever owns the stream the launches go to -- a library handle (its batches are
// issued in order on its own stream) or a one-shot call -- so that two handles pipelined on
// different streams never share, or re-allocate under each other, a buffer in flight.
//
// q_defer also carries the work list of the second launch (the pair kernel), so that one memset
// clears both: [nq] per-query flags, [1] the number of items on the list, then (from the next even
// index) the items, two ints each -- (query, y | ny << 8): block y of the ny blocks that share the
// query's deferred slots.
constexpr int RS_DEF_Y = 8;             // blocks per query the second launch may use
struct RescoreScratch {
  DevBuf<int> q_defer, m_defer;
  static size_t defer_ints(size_t nq, int ymax = RS_DEF_Y) { return nq + 2 + 2 * nq * (size_t)ymax; }
};

// Window-only candidate lists (asl_search_batch with use_ann = 0): no list of row ids, a query's
// window is a run of the library's precursor-sorted view. With the CSR offsets of the call (32-bit,
// tile-local), slot c of query q is the row sorted_row[begin[q] + (c - offsets[q])]; a row with
// valid[row] == 0 is not a candidate (valid == nullptr: every row is).
struct WindowRows {
  const int32_t *begin = nullptr;
  const int32_t *sorted_row = nullptr;
  const uint8_t *valid = nullptr;
};

// One list of candidate slots per query. CSR (offsets non-null) or fixed stride; the slots name
// library rows (rows64 or rows32) or, for a window-only list, are runs of the precursor-sorted view.
struct CandList {
  const int64_t *rows64 = nullptr;      // row ids, 64- or 32-bit: one of the two, neither with `window`
  const int32_t *rows32 = nullptr;
  const int32_t *offsets = nullptr;     // CSR [nq + 1]; nullptr: query q's slots are [q * stride, (q + 1) * stride)
  int32_t stride = 0;
  int64_t total_slots = 0;              // slots of all queries (offsets[nq] or nq * stride)
  // fixed-stride rows: their lengths as the scans' post-filter wrote them (-1: unfiltered row)
  const int32_t *row_counts = nullptr;
  // window-only lists (rows64 = rows32 = nullptr, offsets tile-local; the filter's packed row
  // records and annotated library peaks required)
  const WindowRows *window = nullptr;
};

// Where the results go, one entry per winner (any may be null). The caller's pointers, host or device, at
// an entry point; device pointers from BatchOutStage on and in a RescoreRequest.
struct BatchOut {
  int32_t *best_row = nullptr;          // the winner's library row (-1: none)
  int32_t *best_cand = nullptr;         // its position in its query's list (-1: none)
  double *best_score = nullptr;
  int32_t *n_cand = nullptr;            // [nq] candidates of the query that were scored
  int32_t *pm_count = nullptr;          // the winner's peak matches in greedy order: their number,
  uint32_t *pm_pairs = nullptr;         // (query peak, library peak) pairs [pm_stride, 2]
  int32_t pm_stride = 0;
  // [nq, ASL_SCORE_HIST_BINS] histogram of the scores of the slots n_cand counts (asl_*_topn_hist). A rescoring
  // pass ADDS into the rows (a tiled window search: one pass per tile); the entry point zeroes them once per batch
  int32_t *score_hist = nullptr;
};

// Stages a caller's BatchOut for nq queries and nw winners: kernels write to `dev`, finish() enqueues the
// copies back to whatever lives on the host (the caller synchronises once at the end).
struct BatchOutStage {
  Out<int32_t> row, cand, n_cand, count;
  Out<double> score;
  Out<uint32_t> pairs;
  Out<int32_t> hist;
  BatchOut dev;
  int init(const BatchOut &o, size_t nq, size_t nw) {
    ASL_TRY(row.init(o.best_row, nw));
    ASL_TRY(cand.init(o.best_cand, nw));
    ASL_TRY(score.init(o.best_score, nw));
    ASL_TRY(n_cand.init(o.n_cand, nq));
    ASL_TRY(count.init(o.pm_count, nw));
    ASL_TRY(pairs.init(o.pm_pairs, nw * (o.pm_pairs ? o.pm_stride : 0) * 2));
    ASL_TRY(hist.init(o.score_hist, nq * (size_t)ASL_SCORE_HIST_BINS));
    dev = {row.d, cand.d, score.d, n_cand.d, count.d, pairs.d, o.pm_stride, hist.d};
    // the rows are summed into: zeroed here, once per batch, so that queries without candidates read zero
    if (hist.d) HIP_TRY(hipMemsetAsync(hist.d, 0, nq * (size_t)ASL_SCORE_HIST_BINS * sizeof(int32_t), stream()));
    return ASL_OK;
  }
  int finish() {
    ASL_TRY(row.finish());
    ASL_TRY(cand.finish());
    ASL_TRY(score.finish());
    ASL_TRY(n_cand.finish());
    ASL_TRY(count.finish());
    ASL_TRY(hist.finish());
    return pairs.finish();
  }
};

// One call of the rescoring driver (rescore_device). All pointers are device pointers.
struct RescoreRequest {
  // -- spectra
  DevPeaks Q, L;                        // queries, library
  // -- candidate list
  CandList cand;
  // -- scoring
  double tol = 0.0;                     // fragment m/z tolerance: Da, or
  int tol_ppm = 0;                      // 1: ppm of the QUERY peak's m/z (rescore.hip: rs_frag_tol)
  int allow_shift = 0;
  int tie_by_row = 0;                   // equal scores: 0 the first slot wins, 1 the lowest library row
  PrecFilter filter;                    // precursor window applied to the slots (default: none)
  // -- selection
  // 0: the single winner (rescore_argmax_kernel). 1..ASL_MAX_BEST (asl_*_topn): the n best slots per
  // query (rescore_topn_kernel, the matches kernel over nq * n winners); best_slot and out's best_cand /
  // best_row / best_score / pm_count are then [nq, n_best], pm_pairs [nq, n_best, pm_stride, 2],
  // n_cand stays [nq]
  int n_best = 0;
  // n_best > 0, non-null (asl_*_topn_distinct): group id of every library row, [L.n]; the ranks then
  // hold distinct groups. nullptr: plain ranks
  const int32_t *group = nullptr;
  // -- work memory
  double *pair_score = nullptr;         // one double per candidate slot
  long long *best_slot = nullptr;       // one per winner
  RescoreScratch *scratch = nullptr;    // required
  int *status = nullptr;                // RS_STATUS_* flags, or-ed in (rescore_check_status)
  bool clear_status = true;             // zero the flags first
  // -- outputs
  BatchOut out;
  bool emit_matches = true;             // false: stop after the selection (no best_row, pm_count, pm_pairs written)
};

// The ABI's score flag word (annsolo_mi.h: ASL_SCORE_*, the `allow_shift` argument / member), decoded
// where a call enters: bits other than the two flags are ASL_ERR_INVALID.
struct ScoreFlags {
  int allow_shift = 0, tol_ppm = 0;
};
int decode_score_flags(int word, const char *who, ScoreFlags &out);

// Host driver shared by asl_rescore_batch, asl_search_batch and asl_rescore_knn.
int rescore_device(const RescoreRequest &rq);
// Tiled window search: folds one tile's n best (rescore_device's best_slot / best_score [nq, n], sorted,
// and n_valid over the tile's nq queries; `cand` is the tile's window list, whose slots best_slot
// names) into the running n best of those queries, run_score / run_row [nq, n], sorted by (score
// descending, row ascending), run_row -1 beyond the filled ranks: a higher score goes first, equal
// scores go to the lower library row, counts add up. n = 1 is the single winner. group (non-null:
// the distinct fold): the library rows' group ids, both lists then hold one row per group and so
// does the result.
int rescore_window_merge(const CandList &cand, int nq, int n, const long long *best_slot,
                         const double *best_score, const int32_t *n_valid, double *run_score,
                         int32_t *run_row, int32_t *run_n, const int32_t *group = nullptr);
// After the last tile and the n-candidate pass over the running lists (`rescored`: its best_score
// [nq, n], the same order): best_score = the merged scores (0 for an empty rank), n_cand = the summed
// counts; a filled rank whose rescored score differs from the merged one flags the status (an
// internal error).
int rescore_window_finish(int nq, int n, const double *run_score, const int32_t *run_row,
                          const int32_t *run_n, const double *rescored, double *best_score,
                          int32_t *n_cand, int *status);
int rescore_check_status(const int *status_dev);   // reads the flags back: synchronises
int rescore_status_error(int status_bits);         // ASL_OK or the error the flags stand for

}  // namespace asl
