// search.hip -- one batch of the open-modification hot path, device resident:
// SpectralLibrary._search_batch / _get_library_candidates
// (/root/reference/src/ann_solo/spectral_library.py:328-455).
//
//   encode (spectrum.py:166-214)  ->  index.search(k) (:443-444)
//   -> precursor-window post-filter (:417-429 AND :441-446)  ->  best match (:356-365)
//
// The reference builds two dense nq x N boolean masks; here the ANN ids are post-filtered inside the
// scan's finish or the rescoring kernel's candidate compaction (rescore.hpp: PrecFilter) and the
// window-only modes (window_search.hip) binary-search a precursor-sorted copy of the library, so nothing is
// O(nq*N). This unit: the batch drivers -- synchronous and pipelined -- and their entry points.
#include "index.hpp"
#include "library.hpp"

namespace asl {
int encode_device(const float *mz, const float *inten, const int32_t *offsets, int32_t n,
                  double min_bound, double bin_size, int32_t hash_len, uint32_t seed,
                  int norm, float *out);
int encode_both_device(const float *mz, const float *inten, const int32_t *offsets, int32_t n,
                       double min_bound, double bin_size, int32_t hash_len, uint32_t seed, int norm,
                       float *out, uint2 *ent, int32_t *cnt, int *n_over);
}  // namespace asl

using namespace asl;

// The precursor window applied inside the scan's finish (ScanPostFilter, common.hpp) whenever the
// neighbour rows are consumed as a set; ASL_SCAN_POSTFILTER=0 keeps it in the rescoring (A/B runs).
static int &scan_postfilter_flag() {
  static int on = -1;
  if (on < 0) {
    const char *e = getenv("ASL_SCAN_POSTFILTER");
    on = (e && e[0] == '0') ? 0 : 1;
  }
  return on;
}

// The one argument check of the six entry points (`who`; `kind`: what the entry adds to asl_search_batch).
// *run: the batch has queries; an empty one is ASL_OK and writes nothing. In this order: the rank count, before
// anything touches the device (no device: ASL_ERR_NO_DEVICE whatever else a *_topn call was passed; never
// pipelined, these calls wait here for the batches in flight); nulls; the group column; the empty batch; the rest.
enum { ENTRY_TOPN = 1, ENTRY_DISTINCT = 2, ENTRY_KNN = 4 };
static int check_batch(const char *who, int kind, const asl_library *L, const asl_index *idx,
                       const asl_peaks_t *queries, const asl_search_params_t *P, const int64_t *knn_I, int n_best,
                       const BatchOut &out, bool *run) {
  *run = false;
  if (kind & ENTRY_TOPN) {
    if (n_best < 1 || n_best > ASL_MAX_BEST)
      return fail(ASL_ERR_INVALID, "%s: n_best must be in [1, %d]", who, ASL_MAX_BEST);
    ASL_TRY(ensure_device());
  }
  if (!L || !queries || !P || ((kind & ENTRY_KNN) && !knn_I)) return fail(ASL_ERR_INVALID, "%s: null argument", who);
  if ((kind & ENTRY_DISTINCT) && !L->has_group)
    return fail(ASL_ERR_STATE, "%s: the library has no group column (asl_library_set_groups)", who);
  if (queries->n == 0) return ASL_OK;
  if (out.pm_pairs && out.pm_stride <= 0) return fail(ASL_ERR_INVALID, "%s: pm_stride", who);
  const bool ann = !(kind & ENTRY_KNN) && P->use_ann;
  if (ann && !idx) return fail(ASL_ERR_INVALID, "%s: use_ann needs an index", who);
  if ((ann || (kind & ENTRY_KNN)) && P->k <= 0) return fail(ASL_ERR_INVALID, "%s: k must be positive", who);
  if (P->precursor_mode == ASL_TOL_INTERVAL && !P->precursor_window)
    return fail(ASL_ERR_INVALID, "%s: precursor_mode ASL_TOL_INTERVAL needs precursor_window ([nq, 2] doubles)", who);
  ScoreFlags sf;      // params->allow_shift is the score flag word
  ASL_TRY(decode_score_flags(P->allow_shift, who, sf));
  *run = true;
  return ASL_OK;
}

// The scan request of an ANN batch and what its offers point to (filled in place: the request keeps pointers).
struct BatchScan {
  IndexSearch rq;
  IndexWindow w;
  IndexPostFilter pf;
};
// xq: the hashed queries; I32: the neighbour rows the rescoring reads; I64: the caller's ordered neighbour
// list -- without one the candidates are consumed as a set (filter + best match: no final sort) and the scan
// may apply the precursor window itself, row_len then receives the rows' lengths; pre_*: the coarse stage's
// results where it has run already (the entry lists when it made them: the scan does not list the rows again);
// pre_ent / pre_cnt / pre_over without pre_I: the encoder's entry lists for the coarse stage of the scan's own call.
static void batch_scan(BatchScan &s, const SearchBatch &b, const asl_index *idx, int nprobe, const float *xq,
                       int64_t *I64, int32_t *I32, int32_t *row_len, const float *pre_D = nullptr,
                       const int32_t *pre_I = nullptr, const uint2 *pre_ent = nullptr,
                       const int32_t *pre_cnt = nullptr, int *pre_over = nullptr) {
  const asl_library *L = b.L;
  const asl_search_params_t *P = b.P;
  const bool as_set = I64 == nullptr;
  s.rq = {.nq = b.Q.n, .xq = xq, .k = P->k, .nprobe = nprobe, .I64 = I64, .I32 = I32, .pre_D = pre_D, .pre_I = pre_I,
          .pre_ent = pre_ent, .pre_cnt = pre_cnt, .pre_over = pre_over, .rows = as_set ? ROWS_SET : ROWS_ORDERED};
  // what every ANN batch tells the index of its library: whose columns it may have derived a layout from
  // (serial, generation) and, with a selection installed, the selector
  s.rq.serial = L->serial;
  s.rq.gen = L->sel_gen;
  if (L->has_sel) {
    s.rq.sel_keep = L->keep.p;
    s.rq.sel_n = L->n;
  }
  // The precursor window of the scan: the window scan (asl_index_set_window_scan) when the index is in that
  // mode, else -- no ordered neighbour list asked for -- the scan-side post-filter of THIS library's window column
  if (window_mode(idx)) {
    s.w = {.q_pmz = b.window_operand(), .row_len = as_set ? row_len : nullptr, .tol = P->precursor_tol,
           .mode = P->precursor_mode, .charge = P->charge};
    s.rq.win = &s.w;
  } else if (as_set && scan_postfilter_flag() == 1) {
    s.pf = {.payload = L->window_col(), .n = L->n, .q_pmz = b.window_operand(), .count = row_len,
            .tol = P->precursor_tol, .mode = P->precursor_mode, .charge = P->charge};
    s.rq.post = &s.pf;
  }
}

// The rescoring of a batch over fixed-stride rows of k library row ids each (`cand`: the rows; stride and slots
// are set here), into the batch's outputs; the precursor filter runs inside the kernel's compaction stage.
static RescoreRequest rows_request(const SearchBatch &b, CandList cand) {
  cand.stride = b.P->k;
  cand.total_slots = (int64_t)b.Q.n * b.P->k;
  RescoreRequest rq = b.rescore_request();
  rq.cand = cand;
  batch_filter(b.L, b.P, b.win, rq.filter);
  return rq;
}

// the caller's outputs of the six entry points (library rows, no list positions)
static BatchOut row_outputs(int32_t *row, double *score, int32_t *n_cand, int32_t *count, uint32_t *pairs, int32_t stride,
                            int32_t *hist = nullptr) {
  return {.best_row = row, .best_score = score, .n_cand = n_cand, .pm_count = count, .pm_pairs = pairs, .pm_stride = stride,
          .score_hist = hist};
}

// The synchronous batch: every checked call but asl_search_batch in pipeline mode. The candidates are the
// caller's neighbour lists (knn_in: asl_rescore_knn*), the index's (use_ann; knn_out, if given, receives the
// ordered list) or the precursor windows alone.
static int search_batch_sync(asl_library *L, asl_index *idx, const asl_peaks_t *queries,
                             const asl_search_params_t *P, int n_best, bool distinct, const BatchOut &out,
                             const int64_t *knn_in, int64_t *knn_out) {
  const int nq = queries->n, k = P->k;
  ASL_TRY(ensure_device());
  PeaksStage Q;
  ASL_TRY(Q.init(queries));
  In<double> dwin;
  if (P->precursor_mode == ASL_TOL_INTERVAL) ASL_TRY(dwin.init(P->precursor_window, (size_t)nq * 2));
  SearchBatch b{.L = L, .Q = Q.dev, .P = P, .win = dwin.d, .n_best = n_best, .distinct = distinct};
  BatchOutStage o;
  ASL_TRY(o.init(out, (size_t)nq, b.winners()));
  b.out = o.dev;
  In<int64_t> knn;
  Out<int64_t> o_knn;
  ASL_TRY(L->best_slot.reserve(b.winners()));
  ASL_TRY(L->status.reserve(1));
  if (knn_in) {
    ASL_TRY(knn.init(knn_in, (size_t)nq * k));
    ASL_TRY(L->pair_score.reserve((size_t)nq * k));
    ASL_TRY(rescore_device(rows_request(b, {.rows64 = knn.d})));
  } else if (P->use_ann) {
    const int d = idx->d;
    ASL_TRY(o_knn.init(knn_out, (size_t)nq * k));
    ASL_TRY(L->qvec.reserve((size_t)nq * d));
    ASL_TRY(L->knn.reserve((size_t)nq * k));
    ASL_TRY(L->pair_score.reserve((size_t)nq * k));
    ASL_TRY(L->rows_len.reserve((size_t)nq));
    if (window_mode(idx))
      ASL_TRY(index_window_prepare(idx, L->serial, L->sel_gen, L->window_col(), L->n, nq, P->nprobe));
    // the rows and, where the coarse stage will score from them, their entry lists in the same kernel
    int *over = nullptr;
    ASL_TRY(coarse_lists_begin(idx, nq, &over));
    if (over) {
      ASL_TRY(L->q_ent.reserve((size_t)nq * 64));
      ASL_TRY(L->q_cnt.reserve((size_t)nq));
      ASL_TRY(encode_both_device(Q.dev.mz, Q.dev.intensity, Q.dev.offsets, nq, P->min_bound, P->bin_size,
                                 d, P->hash_seed, 1, L->qvec.p, L->q_ent.p, L->q_cnt.p, over));
    } else {
      ASL_TRY(encode_device(Q.dev.mz, Q.dev.intensity, Q.dev.offsets, nq, P->min_bound, P->bin_size,
                            d, P->hash_seed, 1, L->qvec.p));
    }
    BatchScan s;
    batch_scan(s, b, idx, P->nprobe, L->qvec.p, o_knn.d, L->knn.p, L->rows_len.p, nullptr, nullptr,
               over ? L->q_ent.p : nullptr, over ? L->q_cnt.p : nullptr, over);
    ASL_TRY(index_search_device(idx, s.rq));
    ASL_TRY(rescore_device(rows_request(b, {.rows32 = L->knn.p,
                                            .row_counts = s.rq.rows_filtered ? L->rows_len.p : nullptr})));
  } else {
    ASL_TRY(window_search_device(b));
  }
  ASL_TRY(o.finish());
  ASL_TRY(o_knn.finish());
  return rescore_check_status(L->status.p);  // synchronises the stream
}

// asl_search_batch in pipeline mode (asl_set_pipeline): nothing here waits for the device.
//   stream A: encode -> coarse GEMM -> coarse select          (MFMA-bound, ~1.1 ms of a 16 384 batch)
//   stream B: list scan                                       (fabric / VALU bound, ~6.3 ms)
//   stream C (three-stream mode; else B): filter + rescoring -> peak matches (VALU bound, ~2.2 ms)
// so the front of the next batch (and in three-stream mode the rescoring of the previous one)
// runs under the scan of this one.
// Buffers written by one stream and read by the next (hashed queries + probe lists: A -> B;
// neighbour ids: B -> C) exist twice; the producer re-uses a pair only after the consumer of
// the batch that read it has finished (ev_scan / ev_resc). Everything else is touched by one
// stream only. Errors the kernels flag are sticky and reported by the next call that drains
// (asl_synchronize or any other entry point).
static int search_batch_pipelined(asl_library *L, asl_index *idx, const asl_peaks_t *queries,
                                  const asl_search_params_t *P, const BatchOut &out, int64_t *knn_I) {
  Pipeline &pp = pipeline();
  struct InCall {
    Pipeline &p;
    explicit InCall(Pipeline &q) : p(q) { p.in_call = true; }
    ~InCall() { p.in_call = false; }
  } guard(pp);
  const int nq = queries->n, k = P->k, d = idx->d;
  const bool winflat = idx->kind == ASL_INDEX_WINFLAT;      // no coarse stage: stream A encodes, stream B scans
  const int nprobe = winflat ? 1 : index_nprobe(idx, P->nprobe);
  PeaksStage Q;
  ASL_TRY(Q.init(queries));   // device pointers + known peak count: no copy, no wait
  const int par = pp.parity;
  // allocations first (growing a buffer synchronises the device: only ever on the first batches)
  ASL_TRY(index_prepare(idx));
  if (window_mode(idx))      // (the window-ordered layout of THIS library, up front)
    ASL_TRY(index_window_prepare(idx, L->serial, L->sel_gen, L->window_col(), L->n, nq, nprobe));
  ASL_TRY(L->p_qvec[par].reserve((size_t)nq * d));
  ASL_TRY(L->p_cD[par].reserve((size_t)nq * nprobe));
  ASL_TRY(L->p_cI[par].reserve((size_t)nq * nprobe));
  ASL_TRY(L->p_knn[par].reserve((size_t)nq * k));
  ASL_TRY(L->p_ent[par].reserve((size_t)nq * 64));
  ASL_TRY(L->p_cnt[par].reserve((size_t)nq));
  ASL_TRY(L->p_rows[par].reserve((size_t)nq));
  ASL_TRY(L->pair_score.reserve((size_t)nq * k));
  ASL_TRY(L->best_slot.reserve((size_t)nq));
  // ASL_TOL_INTERVAL: the intervals where they are, or -- a host array -- copied into this parity's buffer
  // before the call returns. Its last readers were the scan and the rescoring of batch i-2.
  const double *dwin = nullptr;
  if (P->precursor_mode == ASL_TOL_INTERVAL) {
    dwin = P->precursor_window;
    if (!is_device_ptr(dwin)) {
      ASL_TRY(L->p_win[par].reserve((size_t)nq * 2));
      if (pp.resc_recorded[par]) HIP_TRY(hipStreamWaitEvent(stream(), pp.ev_resc[par], 0));
      HIP_TRY(hipMemcpyAsync(L->p_win[par].p, dwin, (size_t)nq * 16, hipMemcpyHostToDevice, stream()));
      HIP_TRY(hipStreamSynchronize(stream()));     // the array is the caller's again on return
      dwin = L->p_win[par].p;
    }
  }
  pp.parity ^= 1;
  // the caller's stream produced the inputs (and owns the output memory) up to here
  HIP_TRY(hipEventRecord(pp.ev_in, stream()));
  HIP_TRY(hipStreamWaitEvent(pp.A, pp.ev_in, 0));
  HIP_TRY(hipStreamWaitEvent(pp.B, pp.ev_in, 0));
  HIP_TRY(hipStreamWaitEvent(pp.C, pp.ev_in, 0));
  pp.inflight = true;
  const SearchBatch b{.L = L, .Q = Q.dev, .P = P, .win = dwin, .out = out};
  BatchScan s;
  {
    StreamScope on_a(pp.A);
    // The buffers of this parity were last read by the scan of batch i-2: the front of batch i
    // starts when that scan ends, i.e. it runs under the RESCORING of batch i-2. Measured
    // (profiles/r02_pipeline_ab.txt): holding it back until the batch has finished, so that it
    // runs under the next scan instead, is worse -- the scan loses 1.3 ms to a 0.9 ms GEMM
    // beside it (9.88 ms per step), the rescoring only 0.6 ms (9.35 ms).
    if (pp.scan_recorded[par]) HIP_TRY(hipStreamWaitEvent(pp.A, pp.ev_scan[par], 0));
    // (entry lists from the encoder into this parity's buffers: the coarse stage scores from them and, as
    // when it listed them itself, the scan reads them there)
    int *over = nullptr;
    if (!winflat) ASL_TRY(coarse_lists_begin(idx, nq, &over));
    if (over)
      ASL_TRY(encode_both_device(Q.dev.mz, Q.dev.intensity, Q.dev.offsets, nq, P->min_bound, P->bin_size,
                                 d, P->hash_seed, 1, L->p_qvec[par].p, L->p_ent[par].p, L->p_cnt[par].p, over));
    else
      ASL_TRY(encode_device(Q.dev.mz, Q.dev.intensity, Q.dev.offsets, nq, P->min_bound, P->bin_size,
                            d, P->hash_seed, 1, L->p_qvec[par].p));
    if (winflat)
      L->p_have_ent[par] = false;
    else
      ASL_TRY(coarse_search(idx, L->p_qvec[par].p, nq, nprobe, L->p_cD[par].p, L->p_cI[par].p,
                            L->p_ent[par].p, L->p_cnt[par].p, &L->p_have_ent[par],
                            over ? L->p_ent[par].p : nullptr, over ? L->p_cnt[par].p : nullptr, over));
    HIP_TRY(hipEventRecord(pp.ev_front[par], pp.A));
  }
  {
    StreamScope on_b(pp.B);
    HIP_TRY(hipStreamWaitEvent(pp.B, pp.ev_front[par], 0));
    if (pp.resc_recorded[par]) HIP_TRY(hipStreamWaitEvent(pp.B, pp.ev_resc[par], 0));
    const bool ent = L->p_have_ent[par];
    batch_scan(s, b, idx, nprobe, L->p_qvec[par].p, knn_I, L->p_knn[par].p, L->p_rows[par].p,
               winflat ? nullptr : L->p_cD[par].p, winflat ? nullptr : L->p_cI[par].p,
               ent ? L->p_ent[par].p : nullptr, ent ? L->p_cnt[par].p : nullptr);
    ASL_TRY(index_search_device(idx, s.rq));
    HIP_TRY(hipEventRecord(pp.ev_scan[par], pp.B));
    pp.scan_recorded[par] = true;
  }
  {
    // measured (profiles/r02_pipeline_ab.txt): scan and rescoring are both VALU-limited, so a
    // third stream only makes them share the CUs -- the default keeps rescoring behind its scan
    hipStream_t sc = pp.streams == 3 ? pp.C : pp.B;
    StreamScope on_c(sc);
    HIP_TRY(hipStreamWaitEvent(sc, pp.ev_scan[par], 0));
    // (window scan, scan-side filter: set-mode rows hold in-window hits only, and their lengths)
    RescoreRequest rq = rows_request(b, {.rows32 = L->p_knn[par].p,
                                         .row_counts = s.rq.rows_filtered ? L->p_rows[par].p : nullptr});
    rq.status = pp.status;      // the sticky flags of the batches in flight: never cleared here
    rq.clear_status = false;
    ASL_TRY(rescore_device(rq));
    HIP_TRY(hipEventRecord(pp.ev_resc[par], sc));
    pp.resc_recorded[par] = true;
  }
  return ASL_OK;
}

extern "C" {

int asl_set_scan_postfilter(int on) {
  clear_error();
  int &f = scan_postfilter_flag();
  const int prev = f;
  f = on ? 1 : 0;
  return prev;
}

int asl_search_batch(asl_library_t *L, asl_index_t *idx, const asl_peaks_t *queries,
                     const asl_search_params_t *P, int32_t *best_row, double *best_score,
                     int32_t *n_cand, int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride,
                     int64_t *knn_I) {
  clear_error();
  const BatchOut out = row_outputs(best_row, best_score, n_cand, pm_count, pm_pairs, pm_stride);
  bool run;
  ASL_TRY(check_batch("search_batch", 0, L, idx, queries, P, nullptr, 0, out, &run));
  if (!run) return ASL_OK;
  {
    // pipeline mode applies to ANN batches whose arguments all live on the device (nothing to
    // stage, nothing to copy back) and whose peak count the caller supplied; anything else takes
    // the synchronous path below, after the batches in flight have drained
    Pipeline &pp = pipeline();
    auto dev_or_null = [](const void *p) { return !p || is_device_ptr(p); };
    // (an exhaustive ASL_INDEX_FLAT index has no coarse stage to overlap: synchronous path)
    if (pp.on && P->use_ann && (index_nprobe(idx, P->nprobe) > 0 || idx->kind == ASL_INDEX_WINFLAT) &&
        queries->n_peaks > 0 &&
        peaks_on_device(queries) &&
        is_device_ptr(best_row) && is_device_ptr(best_score) && dev_or_null(n_cand) &&
        dev_or_null(pm_count) && dev_or_null(pm_pairs) && dev_or_null(knn_I)) {
      pp.in_call = true;                    // do not drain: this call joins the pipeline
      const int rc = ensure_device();
      pp.in_call = false;
      ASL_TRY(rc);
      return search_batch_pipelined(L, idx, queries, P, out, knn_I);
    }
  }
  return search_batch_sync(L, idx, queries, P, 0, false, out, nullptr, knn_I);
}

// The five other entries: the check of their kind, then the synchronous batch.
static int checked_batch_sync(const char *who, int kind, asl_library_t *L, asl_index_t *idx, const asl_peaks_t *queries,
                              const asl_search_params_t *P, int n_best, const BatchOut &out, const int64_t *knn_in,
                              int64_t *knn_out) {
  clear_error();
  bool run;
  ASL_TRY(check_batch(who, kind, L, idx, queries, P, knn_in, n_best, out, &run));
  if (!run) return ASL_OK;
  return search_batch_sync(L, idx, queries, P, n_best, (kind & ENTRY_DISTINCT) != 0, out, knn_in, knn_out);
}

int asl_search_batch_topn(asl_library_t *L, asl_index_t *idx, const asl_peaks_t *queries,
                          const asl_search_params_t *P, int32_t n_best, int32_t *best_row, double *best_score,
                          int32_t *n_cand, int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride,
                          int64_t *knn_I) {
  return checked_batch_sync("search_batch_topn", ENTRY_TOPN, L, idx, queries, P, n_best,
                            row_outputs(best_row, best_score, n_cand, pm_count, pm_pairs, pm_stride), nullptr, knn_I);
}

int asl_search_batch_topn_distinct(asl_library_t *L, asl_index_t *idx, const asl_peaks_t *queries,
                                   const asl_search_params_t *P, int32_t n_best, int32_t *best_row,
                                   double *best_score, int32_t *n_cand, int32_t *pm_count, uint32_t *pm_pairs,
                                   int32_t pm_stride, int64_t *knn_I) {
  return checked_batch_sync("search_batch_topn_distinct", ENTRY_TOPN | ENTRY_DISTINCT, L, idx, queries, P, n_best,
                            row_outputs(best_row, best_score, n_cand, pm_count, pm_pairs, pm_stride), nullptr, knn_I);
}

int asl_rescore_knn(asl_library_t *L, const asl_peaks_t *queries, const asl_search_params_t *P,
                    const int64_t *knn_I, int32_t *best_row, double *best_score,
                    int32_t *n_cand, int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride) {
  return checked_batch_sync("rescore_knn", ENTRY_KNN, L, nullptr, queries, P, 0,
                            row_outputs(best_row, best_score, n_cand, pm_count, pm_pairs, pm_stride), knn_I, nullptr);
}

int asl_rescore_knn_topn(asl_library_t *L, const asl_peaks_t *queries, const asl_search_params_t *P,
                         const int64_t *knn_I, int32_t n_best, int32_t *best_row, double *best_score,
                         int32_t *n_cand, int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride) {
  return checked_batch_sync("rescore_knn_topn", ENTRY_KNN | ENTRY_TOPN, L, nullptr, queries, P, n_best,
                            row_outputs(best_row, best_score, n_cand, pm_count, pm_pairs, pm_stride), knn_I, nullptr);
}

int asl_rescore_knn_topn_distinct(asl_library_t *L, const asl_peaks_t *queries, const asl_search_params_t *P,
                                  const int64_t *knn_I, int32_t n_best, int32_t *best_row, double *best_score,
                                  int32_t *n_cand, int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride) {
  return checked_batch_sync("rescore_knn_topn_distinct", ENTRY_KNN | ENTRY_TOPN | ENTRY_DISTINCT, L, nullptr, queries, P,
                            n_best, row_outputs(best_row, best_score, n_cand, pm_count, pm_pairs, pm_stride), knn_I,
                            nullptr);
}

// The ranked calls with the score histogram of every query's candidates (NULL: the plain calls, launch for launch).
int asl_search_batch_topn_hist(asl_library_t *L, asl_index_t *idx, const asl_peaks_t *queries,
                               const asl_search_params_t *P, int32_t n_best, int32_t distinct, int32_t *best_row,
                               double *best_score, int32_t *n_cand, int32_t *pm_count, uint32_t *pm_pairs,
                               int32_t pm_stride, int64_t *knn_I, int32_t *score_hist) {
  return checked_batch_sync("search_batch_topn_hist", ENTRY_TOPN | (distinct ? ENTRY_DISTINCT : 0), L, idx, queries, P,
                            n_best, row_outputs(best_row, best_score, n_cand, pm_count, pm_pairs, pm_stride, score_hist),
                            nullptr, knn_I);
}

int asl_rescore_knn_topn_hist(asl_library_t *L, const asl_peaks_t *queries, const asl_search_params_t *P,
                              const int64_t *knn_I, int32_t n_best, int32_t distinct, int32_t *best_row,
                              double *best_score, int32_t *n_cand, int32_t *pm_count, uint32_t *pm_pairs,
                              int32_t pm_stride, int32_t *score_hist) {
  return checked_batch_sync("rescore_knn_topn_hist", ENTRY_KNN | ENTRY_TOPN | (distinct ? ENTRY_DISTINCT : 0), L, nullptr,
                            queries, P, n_best,
                            row_outputs(best_row, best_score, n_cand, pm_count, pm_pairs, pm_stride, score_hist), knn_I,
                            nullptr);
}

}  // extern "C"
