// index_search.hip -- the host driver of every index search: the coarse quantiser, one function per scan
// path, index_search_device (what search.hip and sharded.hip call), the search entries of the C ABI.
#include <algorithm>

#include "index.hpp"

namespace asl {

// transposed centroid copy for the sparse coarse quantiser (rebuilt after train / set_trained)
static int coarse_transposed(asl_index *ix) {
  if (ix->cent_t_ready) return ASL_OK;
  ASL_TRY(ix->centroids_t.reserve((size_t)ix->nlist * ix->d));
  ASL_TRY(transpose_f32(ix->centroids.p, ix->nlist, ix->d, ix->centroids_t.p));
  ix->cent_t_ready = true;
  return ASL_OK;
}

// q . centroid of EVERY list for rows [0, m) of xq -> scores [m, nlist]: what coarse_search selects its probes
// from (and asl_index_rank's exhaustive IVF-PQ scope takes its coarse terms from). Hashed spectra are sparse
// (<= ~50 of 800 components): the scores come from the sparse kernel, bit-identical to the GEMM. Both are
// enqueued; a device-side count of dense rows (more than 64 non-zeros) decides which of the two does the
// work (the other returns at once). ent / cnt (may be null: the index's own buffers): the rows' entry lists.
// ready_over: ent / cnt hold the lists already and this is their count of dense rows (nothing is listed).
int coarse_scores_all(asl_index *ix, const float *xq, int m, float *scores, uint2 *ent, int32_t *cnt, int *ready_over) {
  const int nlist = ix->nlist, d = ix->d;
  const bool sparse = ix->scan_variant == 0 && coarse_sparse_supported(d, nlist);
  const int over_max = m / 64;
  if (sparse) {
    ASL_TRY(coarse_transposed(ix));
    ASL_TRY(ix->cs_ent.reserve((size_t)m * coarse_sparse_cap()));
    ASL_TRY(ix->cs_cnt.reserve((size_t)m));
    ASL_TRY(ix->cs_over.reserve(1));
    ASL_TRY(coarse_sparse(xq, m, d, ix->centroids_t.p, nlist, ent ? ent : ix->cs_ent.p, cnt ? cnt : ix->cs_cnt.p,
                          ready_over ? ready_over : ix->cs_over.p, over_max, scores, nlist, 0, ready_over != nullptr));
  }
  return gemm_nt_f32(xq, ix->centroids.p, scores, m, nlist, d, d, d, nlist,
                     sparse ? (ready_over ? ready_over : ix->cs_over.p) : nullptr, over_max);
}

// coarse quantiser: top-nprobe centroids by inner product -> ix->coarse_D / coarse_I
// ent_out / cnt_out (caller buffers [nq * 64] / [nq], may be null): the queries' entry lists, which
// the sparse coarse kernel lists anyway, for the scan that follows (*have_ent says whether they were
// produced: only the sparse formulation makes them)
int coarse_search(asl_index *ix, const float *xq, int nq, int nprobe, float *out_D, int32_t *out_I, uint2 *ent_out,
                  int32_t *cnt_out, bool *have_ent, const uint2 *pre_ent, const int32_t *pre_cnt, int *pre_over) {
  const int nlist = ix->nlist, d = ix->d;
  if (have_ent) *have_ent = false;
  if (!out_D) {
    ASL_TRY(ix->coarse_D.reserve((size_t)nq * nprobe));
    ASL_TRY(ix->coarse_I.reserve((size_t)nq * nprobe));
    out_D = ix->coarse_D.p;
    out_I = ix->coarse_I.p;
  }
  int rows = (int)std::min<int64_t>(nq, std::max<int64_t>(1, (int64_t)(SCORE_CHUNK_BYTES / ((size_t)nlist * 4))));
  ASL_TRY(ix->ws_scores.reserve((size_t)rows * nlist));
  const bool sparse = ix->scan_variant == 0 && coarse_sparse_supported(d, nlist);
  // the encoder's lists serve a batch scored as one chunk (their count of dense rows is the batch's); the scan
  // then reads them where they lie
  const bool ready = sparse && pre_ent && pre_cnt && pre_over && nq <= rows && coarse_sparse_cap() == 64;
  for (int r0 = 0; r0 < nq; r0 += rows) {
    const int m = std::min(rows, nq - r0);
    {
      ProfScope ps("coarse_gemm");
      if (ready)
        ASL_TRY(coarse_scores_all(ix, xq, m, ix->ws_scores.p, const_cast<uint2 *>(pre_ent),
                                  const_cast<int32_t *>(pre_cnt), pre_over));
      else
        ASL_TRY(coarse_scores_all(ix, xq + (size_t)r0 * d, m, ix->ws_scores.p, ent_out ? ent_out + (size_t)r0 * 64 : nullptr,
                                  cnt_out ? cnt_out + (size_t)r0 : nullptr));
    }
    {
      ProfScope ps("coarse_select");
      ASL_TRY(row_topk(ix->ws_scores.p, nlist, m, nlist, nprobe, nullptr, 0, nullptr, nullptr, 0,
                       out_D + (size_t)r0 * nprobe, nullptr, out_I + (size_t)r0 * nprobe, nprobe));
    }
  }
  // (own buffers: valid for the whole batch only when it was one chunk)
  if (have_ent) *have_ent = sparse && coarse_sparse_cap() == 64 && ((ent_out && cnt_out) || nq <= rows);
  return ASL_OK;
}

// ASL_COARSE_LISTS=0 keeps the lists rebuilt from the dense rows (A/B runs of one build). Read at every batch,
// not once: one process can then run both routes over the same queries (tests/test_gpu_coarse_select.py).
static bool coarse_lists_enabled() {
  const char *e = getenv("ASL_COARSE_LISTS");
  return !(e && e[0] == '0');
}

int coarse_lists_begin(asl_index *ix, int nq, int **over) {
  *over = nullptr;
  if (!coarse_lists_enabled() || nq <= 0 || ix->nlist <= 0) return ASL_OK;
  if (ix->kind != ASL_INDEX_IVFFLAT && ix->kind != ASL_INDEX_IVFPQ) return ASL_OK;
  if (!(ix->scan_variant == 0 && coarse_sparse_supported(ix->d, ix->nlist)) || coarse_sparse_cap() != 64) return ASL_OK;
  if ((size_t)nq > SCORE_CHUNK_BYTES / ((size_t)ix->nlist * 4)) return ASL_OK;      // more than one chunk
  ASL_TRY(ix->cs_over.reserve(1));
  HIP_TRY(hipMemsetAsync(ix->cs_over.p, 0, sizeof(int), stream()));
  *over = ix->cs_over.p;
  return ASL_OK;
}

// ---- what a scan path needs of the index at (k, nprobe); asl_index_supports_keys answers from the same
static bool postings_ok(const asl_index *ix, int k, int nprobe) {      // dimension-major postings (IVF-Flat)
  return ix->has_inv && ix->scan_variant == 0 && flat_inv_supported(ix->d, k, nprobe);
}
static bool tiled_shape_ok(const asl_index *ix, int k, int nprobe) {   // tiled IVF-PQ scan, once the lists are tiled
  return ix->scan_variant == 0 && tiled_index(ix) && pq_scan_tiled_supported(ix->pq_m, ix->ksub, k, nprobe);
}
static bool keys_fit(int k) { return k + FLAT_KEYS_SLACK <= TK_MAX_K; }  // packed-key and post-filtered rows

// nprobe clamped to the lists there are; more than the LDS top-k selects is an error
static int clamp_nprobe(const asl_index *ix, int *nprobe, const char *who) {
  *nprobe = std::max(1, std::min(*nprobe, ix->nlist));
  if (*nprobe > TK_MAX_K) return fail(ASL_ERR_CAPACITY, "%s: nprobe=%d > %d", who, *nprobe, TK_MAX_K);
  return ASL_OK;
}

// algorithmic work: vectors in probed lists, summed on the device (nothing waits inside a step)
static int count_scanned(const asl_index *ix, const int32_t *cI, int nq, int nprobe) {
  if (!prof_counts()) return ASL_OK;
  if (unsigned long long *acc = prof_scanned_dev())
    ASL_TRY(scanned_count(cI, (int64_t)nq * nprobe, ix->list_offsets.p, acc));
  return ASL_OK;
}

// What validate() settles of a request against the index, for the path functions.
struct SearchPlan {
  int unordered = 0;      // row mode in force: the handle's (asl_index_set_unordered) or the request's RAW / KEYS
  int nprobe = 0;         // clamped
  bool refine = false;    // exact re-rank of a k_scan short-list
  int k_scan = 0;         // the scan's k (k' under refine)
  bool use_inv = false, tiled = false;   // the layout-specific scan: postings (IVF-Flat) / tiles (IVF-PQ)
};

// The window-exact index (ASL_INDEX_WINFLAT): one list, no probes. What it does not serve is an error that names
// the reason, never a filter behind the top-k. A selector that comes WITH a window is the fused path's (the
// library's selection): the key column it installed is the effective one, NaN where unselected, so the runs
// leave the unselected out and the selector itself is unread.
static int validate_winflat(asl_index *ix, const IndexSearch &rq, const SearchPlan &pl) {
  if (rq.gate || rq.pre_I || rq.pre_D)
    return fail(ASL_ERR_STATE, "a window-exact index has no probe lists: no preassigned or gated search");
  if (rq.pre_ent && !rq.xq) return fail(ASL_ERR_STATE, "a window-exact index takes no entry-list-only queries");
  if (pl.unordered == 2) return fail(ASL_ERR_STATE, "packed-key rows are not served by a window-exact index");
  if (rq.sel_keep && !rq.win)
    return fail(ASL_ERR_STATE, "a window-exact index takes a selection through its key column (NaN: unselected), "
                               "not a selector");
  if (rq.win && !rq.win->q_pmz) return fail(ASL_ERR_INVALID, "window scan: null precursor m/z");
  if (rq.nq <= 0) return ASL_OK;
  if (!rq.xq) return fail(ASL_ERR_INVALID, "search: null queries");
  if (rq.k <= 0) return fail(ASL_ERR_CAPACITY, "search: k=%d outside 1..%d", rq.k, TK_MAX_K - FLAT_KEYS_SLACK);
  if (!keys_fit(rq.k))
    return fail(ASL_ERR_STATE, "a window-exact index holds k <= %d (k=%d)", TK_MAX_K - FLAT_KEYS_SLACK, rq.k);
  if (!flat_inv_supported(ix->d, rq.k, 1))
    return fail(ASL_ERR_STATE, "a window-exact index is searched by the postings scan, which holds d <= 4096 (d=%d)", ix->d);
  ASL_TRY(build_lists(ix));      // (after add or reset: the layout in id order, no key)
  if (ix->n_store > 0 && !ix->has_inv && ix->d <= 65535 && ix->nnz_max == 0)
    return fail(ASL_ERR_STATE, "a window-exact index of all-zero vectors has no postings to scan");
  if (ix->n_store > 0 && !ix->has_inv)
    return fail(ASL_ERR_STATE, "a window-exact index needs sparse vectors: its postings are built when the most "
                               "non-zeros of a vector (%d), times 8, stay below d=%d", ix->nnz_max, ix->d);
  if (rq.win && !ix->win_ready)
    return fail(ASL_ERR_STATE, "window scan: no window key (asl_index_set_window_key), or vectors were added "
                               "since it was set");
  return ASL_OK;
}

// Every request-versus-index check, in the order callers met them (a stale layout is rebuilt where one asks what the lists hold).
static int validate(asl_index *ix, const IndexSearch &rq, SearchPlan &pl) {
  const int k = rq.k;
  pl.unordered = rq.rows == ROWS_KEYS ? 2 : rq.rows == ROWS_SET_RAW ? 1 : ix->unordered;
  if (ix->kind == ASL_INDEX_WINFLAT) return validate_winflat(ix, rq, pl);
  pl.refine = ix->kind == ASL_INDEX_IVFPQ && ix->refine_k > k && ix->refine_rows && pl.unordered == 0;
  // a window (rq.win): only the in-window run of every probed list is scanned, in the window-ordered
  // layout; whatever cannot do that is an error, never the whole lists
  if (rq.win) {
    if (const char *why = window_unsupported(ix)) return fail(ASL_ERR_STATE, "%s", why);
    if (ix->scan_variant != 0)
      return fail(ASL_ERR_STATE, "the window scan needs the layout-specific scan (scan_variant 0), not the generic kernels");
    if (!keys_fit(k)) return fail(ASL_ERR_STATE, "the window scan holds k <= %d (k=%d)", TK_MAX_K - FLAT_KEYS_SLACK, k);
    if (rq.gate || pl.unordered == 2 || pl.refine)
      return fail(ASL_ERR_STATE, "the window scan takes no gate, packed keys or exact re-rank");
    if (!rq.win->q_pmz) return fail(ASL_ERR_INVALID, "window scan: null precursor m/z");
  }
  // a selector (rq.sel_keep): the scans choose their k among the selected vectors; whatever cannot do that
  // is an error, never a filter behind the top-k
  if (rq.sel_keep) {
    if (ix->kind == ASL_INDEX_FLAT) return fail(ASL_ERR_STATE, "a selector needs an IVF index (not a Flat index)");
    if (ix->shard_world > 1 || ix->has_vids) return fail(ASL_ERR_STATE, "a selector does not run on a sharded index");
    if (ix->scan_variant != 0)
      return fail(ASL_ERR_STATE, "a selector needs the layout-specific scan (scan_variant 0), not the generic kernels");
    if (!keys_fit(k)) return fail(ASL_ERR_STATE, "a selected search holds k <= %d (k=%d)", TK_MAX_K - FLAT_KEYS_SLACK, k);
    if (rq.gate || pl.unordered == 2 || (rq.pre_ent && !rq.xq))
      return fail(ASL_ERR_STATE, "a selected search takes no gate, packed keys or entry-list-only queries");
    if (pl.refine) return fail(ASL_ERR_STATE, "a selected search does not run with the exact re-rank");
    if (rq.sel_n != ix->ntotal)
      return fail(ASL_ERR_INVALID, "selector: %lld flags for %lld vectors", (long long)rq.sel_n, (long long)ix->ntotal);
  }
  if (rq.nq <= 0) return ASL_OK;
  // pre_ent / pre_cnt: the queries as ENTRY LISTS (list_nonzeros / encode_entries_device); xq may
  // then be null -- only the layout-specific scans read their queries in that form, and a row
  // whose count is negative (more than 64 non-zeros) is searched as an all-zero query: the
  // caller watches the producer's n_over
  // Without probe lists (no pre_I): lists ready, probes still to find -- with the dense rows and pre_over.
  if (rq.pre_ent && (!rq.pre_cnt || ix->kind == ASL_INDEX_FLAT ||
                     (rq.pre_I ? (!rq.xq && !rq.pre_D) : (!rq.xq || !rq.pre_over || rq.pre_D != nullptr))))
    return fail(ASL_ERR_STATE, "entry-list search: needs the counts, an IVF index, and the caller's probe lists (with "
                               "their scores when no dense rows are given) or the dense rows and the lists' count "
                               "of dense rows");
  // (with dense rows given as well, entry lists are a hint: a scan that does not read them ignores them)
  if (!rq.xq && !rq.pre_ent) return fail(ASL_ERR_INVALID, "search: null queries");
  // gate: a device-side count -- only the first *gate rows are searched (layout-specific scans only)
  if (rq.gate && (!rq.pre_I || ix->kind == ASL_INDEX_FLAT))
    return fail(ASL_ERR_STATE, "gated search: needs the caller's probe lists and an IVF index");
  if (!ix->trained) return fail(ASL_ERR_STATE, "search: index is not trained");
  if (k <= 0 || k > TK_MAX_K_PASSES) return fail(ASL_ERR_CAPACITY, "search: k=%d outside 1..%d", k, TK_MAX_K_PASSES);
  const bool ents_only = rq.pre_ent && !rq.xq;
  pl.nprobe = rq.nprobe;
  pl.k_scan = k;
  // beyond the LDS top-k (the reference's CPU path has no bound on --num_candidates, config.py:188-192;
  // its notebooks evaluate 5 000+ neighbours): ordered dense searches only, in bounded passes of the
  // generic kernels (rows asked for as an unordered set are served ordered: a valid answer)
  if (k > TK_MAX_K && (rq.gate || ents_only || pl.unordered == 2))
    return fail(ASL_ERR_STATE, "search: k=%d > %d is served from dense queries only (no packed keys, "
                               "entry-list-only queries or gates)", k, TK_MAX_K);
  if (ix->kind == ASL_INDEX_FLAT) {
    if (pl.unordered == 2) return fail(ASL_ERR_STATE, "packed-key rows need an IVF index");
    return ASL_OK;
  }
  ASL_TRY(clamp_nprobe(ix, &pl.nprobe, "search"));
  ASL_TRY(build_lists(ix));
  if (k > TK_MAX_K) return ASL_OK;      // neither layout-specific scan nor re-rank (k' <= TK_MAX_K)
  if (ix->kind == ASL_INDEX_IVFFLAT) {
    // variant 0: dimension-major postings; 1 (or an unsupported shape): dense GEMM + masked top-k
    pl.use_inv = postings_ok(ix, k, pl.nprobe);
    if (pl.unordered == 2 && !(pl.use_inv && rq.I64 && keys_fit(k)))
      return fail(ASL_ERR_STATE, "packed-key rows need the postings scan of IVF-Flat (sparse vectors, k <= 1280) and an int64 output");
    if (rq.gate && !pl.use_inv) return fail(ASL_ERR_STATE, "gated search: needs the postings scan of IVF-Flat");
    if (ents_only && !pl.use_inv) return fail(ASL_ERR_STATE, "entry-list search: needs the postings scan of IVF-Flat");
    if (rq.sel_keep && !pl.use_inv)
      return fail(ASL_ERR_STATE, "a selector needs the postings scan of IVF-Flat (sparse vectors, nprobe <= 1024), "
                                 "not dense rows");
    return ASL_OK;
  }
  // IVF-PQ. Exact re-rank: the ADC scan returns k' > k candidates as a set, refine.hip keeps the k best
  if (rq.gate && pl.refine) return fail(ASL_ERR_STATE, "gated search: not with the exact re-rank");
  if (ents_only && pl.refine) return fail(ASL_ERR_STATE, "entry-list search: not with the exact re-rank (it reads the dense queries)");
  if (pl.refine) {
    if (ix->refine_bad)
      return fail(ASL_ERR_CAPACITY, "search: refine is unavailable, a stored vector has more than %d non-zeros",
                  refine_stride());
    if (ix->r_n != ix->ntotal)
      return fail(ASL_ERR_STATE, "search: refine rows cover %lld of %lld vectors (enable refine before add)",
                  (long long)ix->r_n, (long long)ix->ntotal);
    pl.k_scan = std::min(ix->refine_k, (int)TK_MAX_K);
  }
  pl.tiled = ix->has_tiles && tiled_shape_ok(ix, pl.k_scan, pl.nprobe);
  if (pl.unordered == 2 && !(pl.tiled && rq.I64))
    return fail(ASL_ERR_STATE, "packed-key rows need the tiled IVF-PQ scan (m = 32, 8 bits) and an int64 output");
  if (rq.gate && !pl.tiled) return fail(ASL_ERR_STATE, "gated search: needs the tiled IVF-PQ scan");
  if (ents_only && !pl.tiled) return fail(ASL_ERR_STATE, "entry-list search: needs the tiled IVF-PQ scan (m = 32, 8 bits)");
  if (rq.sel_keep && !pl.tiled)
    return fail(ASL_ERR_STATE, "a selector needs the tiled IVF-PQ scan (m = 32, 8 bits, nprobe <= 1024)");
  if (rq.win && !pl.tiled) return fail(ASL_ERR_STATE, "the window scan needs the tiled IVF-PQ scan (m = 32, 8 bits)");
  if (rq.win && !ix->win_ready)
    return fail(ASL_ERR_STATE, "window scan: no window key (asl_index_set_window_key), or the lists changed "
                               "since it was set");
  return ASL_OK;
}

// The queries' non-zero components as ready lists for the layout-specific scans: the caller's, else the ones the
// coarse stage of this very call listed (same stream), else listed here. The tiled scan's table build then starts from
// 512 bytes instead of listing a 3.2 KB row (17 us per 16 384 queries here, ~4 us saved per (query, shard) workgroup).
static int query_entries(asl_index *ix, const IndexSearch &rq, bool own_ent, const uint2 **q_ent,
                         const int32_t **q_cnt) {
  *q_ent = rq.pre_ent;
  *q_cnt = rq.pre_cnt;
  if (!rq.pre_ent && own_ent) {
    *q_ent = ix->cs_ent.p;
    *q_cnt = ix->cs_cnt.p;
  } else if (!rq.pre_ent) {
    ASL_TRY(ix->scan_ent.reserve((size_t)rq.nq * 64));
    ASL_TRY(ix->scan_cnt.reserve((size_t)rq.nq));
    ASL_TRY(ix->scan_over.reserve(1));
    ASL_TRY(list_nonzeros(rq.xq, rq.nq, ix->d, ix->d, ix->scan_ent.p, ix->scan_cnt.p, ix->scan_over.p));
    *q_ent = ix->scan_ent.p;
    *q_cnt = ix->scan_cnt.p;
  }
  return ASL_OK;
}

// The scan's post-filter for this request, or an empty one (set-mode int32 rows of an unsharded index). Sets rq.rows_filtered.
static int take_post_filter(asl_index *ix, IndexSearch &rq, int mode, const int32_t *slot_ids, int64_t nslots,
                            ScanPostFilter &pf) {
  pf = ScanPostFilter();
  if (!rq.post) return ASL_OK;
  const IndexPostFilter &p = *rq.post;
  if (!(mode == 1 && rq.I32 && !rq.I64 && !rq.D && !rq.gate && keys_fit(rq.k)) || !p.payload || !p.q_pmz || !p.count ||
      p.n != ix->ntotal || ix->has_vids) return ASL_OK;
  ASL_TRY(post_filter_pairs(ix, p, rq.serial, rq.gen, slot_ids, nslots));
  pf = {.idpay = ix->idpay.p, .q_pmz = p.q_pmz, .count = p.count, .tol = p.tol, .mode = p.mode, .charge = p.charge};
  rq.rows_filtered = true;
  return ASL_OK;
}

// k > TK_MAX_K: ceil(k / TK_MAX_K) bounded passes of the generic kernels. Every hit has a unique
// 64-bit key (score, ~id); a pass keeps the TK_MAX_K best keys strictly below the row's bound = the
// smallest key the pass before it wrote (0 once a row is exhausted), and writes them behind the
// earlier ones: the rows are the exact (score desc, id asc) top-k, -1 padded, as for small k.
// IndexFlatIP / IVF-Flat: the scores of a row chunk are computed once (GEMM) and selected from
// ceil(k / 2048) times; IVF-PQ: the ADC scan of the generic kernel is repeated per pass.
static int pass_bounds(asl_index *ix, const IndexSearch &rq, uint64_t **upper) {   // (null: one pass, nothing to bound)
  *upper = nullptr;
  if (rq.k <= TK_MAX_K) return ASL_OK;
  ASL_TRY(ix->ws_upper.reserve((size_t)rq.nq));
  *upper = ix->ws_upper.p;
  return ASL_OK;
}

// IndexFlatIP, and IVF-Flat without postings (cI: its probe lists, as a bitmap over the lists):
// dense GEMM + (masked) top-k by row chunks. The generic kernels take no post-filter.
static int search_gemm_topk(asl_index *ix, const IndexSearch &rq, const int32_t *cI, int nprobe) {
  const int nq = rq.nq, k = rq.k, d = ix->d;
  const int64_t n = ix->n_store;
  const bool ivf = cI != nullptr;
  uint64_t *upper;
  ASL_TRY(pass_bounds(ix, rq, &upper));
  int words = 0;
  if (ivf) {
    words = (ix->nlist + 31) / 32;
    ASL_TRY(ix->bitmap.reserve((size_t)nq * words));
    ASL_TRY(probe_bitmap(cI, nq, nprobe, ix->bitmap.p, words));
    if (n > 0) ASL_TRY(count_scanned(ix, cI, nq, nprobe));
  }
  const int64_t ncol = std::max<int64_t>(n, 1);
  int rows = (int)std::min<int64_t>(nq, std::max<int64_t>(1, (int64_t)(SCORE_CHUNK_BYTES / ((size_t)ncol * 4))));
  ASL_TRY(ix->ws_scores.reserve((size_t)rows * ncol));
  auto out_at = [&](auto *base, int64_t r0, int c0) { return base ? base + (size_t)r0 * k + c0 : nullptr; };
  for (int r0 = 0; r0 < nq; r0 += rows) {
    const int m = std::min(rows, nq - r0);
    ProfScope ps("scan");
    if (n > 0)
      ASL_TRY(gemm_nt_f32(rq.xq + (size_t)r0 * d, ix->vecs.p, ix->ws_scores.p, m, (int)n, d, d, d, (int)n));
    for (int c0 = 0; c0 < k; c0 += TK_MAX_K) {
      const int kp = std::min<int>(TK_MAX_K, k - c0);
      ASL_TRY(row_topk(ix->ws_scores.p, n, m, (int)n, kp, ix->has_vids ? ix->vids.p : nullptr, 0,
                       ivf ? ix->vlist.p : nullptr, ivf ? ix->bitmap.p + (size_t)r0 * words : nullptr, words,
                       out_at(rq.D, r0, c0), out_at(rq.I64, r0, c0), out_at(rq.I32, r0, c0), k,
                       c0 ? upper + r0 : nullptr, upper ? upper + r0 : nullptr));
    }
  }
  return upper ? sync_stream() : ASL_OK;
}

// IVF-Flat: the postings scan (flat_scan.hip; flat_postings.hpp) when the lists have postings, else the GEMM
static int search_ivfflat(asl_index *ix, IndexSearch &rq, const SearchPlan &pl) {
  const int nq = rq.nq, nprobe = pl.nprobe;
  bool own_ent = false;
  if (!rq.pre_I)
    ASL_TRY(coarse_search(ix, rq.xq, nq, nprobe, nullptr, nullptr, nullptr, nullptr, &own_ent, rq.pre_ent, rq.pre_cnt,
                          rq.pre_over));
  // search_preassigned: the caller's probe lists are read where they lie (device memory that
  // stays valid until the scan has run: the pipeline's per-parity buffers, a caller's tensor on
  // this stream); the coarse scores are unused
  const int32_t *cI = rq.pre_I ? rq.pre_I : ix->coarse_I.p;
  if (!pl.use_inv) return search_gemm_topk(ix, rq, cI, nprobe);
  const uint2 *q_ent;
  const int32_t *q_cnt;
  ASL_TRY(query_entries(ix, rq, own_ent, &q_ent, &q_cnt));
  const int mode_ = pl.unordered ? pl.unordered : (rq.rows != ROWS_ORDERED ? 1 : 0);
  ScanPostFilter pf;
  ASL_TRY(take_post_filter(ix, rq, mode_, ix->ids.p, ix->n_store, pf));
  const unsigned long long *sel = nullptr;
  if (rq.sel_keep) ASL_TRY(selector_words(ix, rq, false, &sel));
  {
    ProfScope ps("scan");     // the scan kernel itself
    FlatScan fs;
    fs.xq = rq.xq, fs.ent = q_ent, fs.ent_cnt = q_cnt, fs.nq = nq, fs.k = rq.k;
    fs.coarse_I = cI, fs.nprobe = nprobe, fs.gate = rq.gate, fs.post = pf, fs.sel = sel;
    fs.D = rq.D, fs.I64 = rq.I64, fs.I32 = rq.I32, fs.set_mode = mode_;
    ASL_TRY(flat_inv_scan(postings_view(ix), fs));
  }
  return rq.gate ? ASL_OK : count_scanned(ix, cI, nq, nprobe);
}

// The window-exact index: every query's run of positions in the one precursor-ordered list (no window: all of
// it), then the ranged form of the postings scan over the blocks of the run. Set-mode rows of a windowed request
// hold in-window hits only; their lengths go to rq.win->row_len.
static int search_winflat(asl_index *ix, IndexSearch &rq, const SearchPlan &pl) {
  const int nq = rq.nq;
  const uint2 *q_ent;
  const int32_t *q_cnt;
  ASL_TRY(query_entries(ix, rq, false, &q_ent, &q_cnt));
  const int mode_ = (pl.unordered || rq.rows != ROWS_ORDERED) ? 1 : 0;
  ASL_TRY(ix->win_ranges.reserve((size_t)nq));
  {
    ProfScope ps("window_ranges");
    const IndexWindow *w = rq.win;
    ASL_TRY(winflat_runs(w ? w->q_pmz : nullptr, nq, ix->wf_key.p, ix->n_store, w ? w->charge : 0, w ? w->tol : 0.0,
                         w ? w->mode : ASL_TOL_DA, ix->win_ranges.p,
                         prof_counts() ? prof_scanned_dev() : nullptr));      // work: sum of hi - lo
  }
  FlatScan fs;      // no probes: the runs stand for them
  fs.xq = rq.xq, fs.ent = q_ent, fs.ent_cnt = q_cnt, fs.nq = nq, fs.k = rq.k;
  fs.D = rq.D, fs.I64 = rq.I64, fs.I32 = rq.I32, fs.set_mode = mode_;
  fs.ranges.range = ix->win_ranges.p;
  fs.ranges.row_len = (rq.win && mode_ == 1) ? rq.win->row_len : nullptr;
  rq.rows_filtered = fs.ranges.row_len != nullptr;
  ProfScope ps("scan");
  return flat_inv_scan(postings_view(ix), fs);      // (an empty index: every run is empty, no layout is read)
}

// [m][dsub][ksub] copy of the codebooks for the tiled scan's LUT build (rebuilt after train / set_trained)
int index_codebooks_transposed(asl_index *ix) {
  if (ix->cbt_ready) return ASL_OK;
  const size_t ncb = (size_t)ix->pq_m * ix->ksub * ix->dsub;
  std::vector<float> h((size_t)ncb), ht((size_t)ncb);
  ASL_TRY(ix->codebooks.download(h.data(), ncb));
  ASL_TRY(sync_stream());
  for (int m = 0; m < ix->pq_m; m++)
    for (int c = 0; c < ix->ksub; c++)
      for (int t = 0; t < ix->dsub; t++)
        ht[((size_t)m * ix->dsub + t) * ix->ksub + c] = h[((size_t)m * ix->ksub + c) * ix->dsub + t];
  ASL_TRY(ix->codebooks_t.upload(ht.data(), ncb));
  ASL_TRY(sync_stream());
  ix->cbt_ready = true;
  return ASL_OK;
}

// by_residual off: the coarse term of every score is FAISS' dis0 = 0, so the scans are handed zeros where they
// would read coarse scores. One buffer on the index, cleared on the stream when it grows; nothing writes it.
int index_zero_coarse(asl_index *ix, size_t n, const float **zeros) {
  if (n > ix->zero_D.cap) {
    ASL_TRY(ix->zero_D.reserve(n));
    HIP_TRY(hipMemsetAsync(ix->zero_D.p, 0, n * sizeof(float), stream()));
  }
  *zeros = ix->zero_D.p;
  return ASL_OK;
}

// The sub-quantiser-major copy of the default layout's codes (pq_scan_v3.hip, MM), built from codes_tiled when a
// plain scan finds none: after the lists changed, build_lists dropped it. The plane size is a whole number of
// 128-byte lines, and an odd one, so that the 32 planes of a tile do not start a power of two apart.
int index_codes_mmajor(asl_index *ix) {
  if (ix->mm_ready) return ASL_OK;
  const int64_t ntiles = ix->n_tile_slots / 64;
  const uint64_t plane = ((((uint64_t)ntiles * 64 + 127) / 128) | 1u) * 128;
  if (plane * (uint64_t)ix->pq_m >= (1ull << 32)) return ASL_OK;     // lane offsets are 32 bits: such an index stays tile-major
  ASL_TRY(ix->codes_mm.reserve((size_t)plane * (size_t)ix->pq_m));
  ASL_TRY(mmajor_codes(ix->codes_tiled.p, ntiles, (uint32_t)plane, ix->codes_mm.p));
  ASL_TRY(sync_stream());      // (as build_lists after tile_codes: later scans may run on the pipeline's other stream)
  ix->mm_plane = (uint32_t)plane;
  ix->mm_ready = true;
  return ASL_OK;
}

// IVF-PQ, tiled scan (pq_scan_v3.hip), over the default layout or -- rq.win -- over the in-window
// run of every probed list in the window-ordered one
static int scan_pq_tiled(asl_index *ix, IndexSearch &rq, const SearchPlan &pl, const float *cD, const int32_t *cI,
                         bool own_ent) {
  const int nq = rq.nq, nprobe = pl.nprobe;
  ASL_TRY(index_codebooks_transposed(ix));
  const uint2 *q_ent;
  const int32_t *q_cnt;
  ASL_TRY(query_entries(ix, rq, own_ent, &q_ent, &q_cnt));
  const int mode_ = pl.unordered ? pl.unordered : (rq.rows != ROWS_ORDERED ? 1 : 0);
  ScanPostFilter pf;
  ScanRanges rg;
  if (rq.win) {                // the rows are in-window already: no post-filter
    const IndexWindow &wq = *rq.win;
    ASL_TRY(ix->win_ranges.reserve((size_t)nq * nprobe));
    ProfScope ps("window_ranges");
    ASL_TRY(window_ranges(wq.q_pmz, nq, cI, nprobe, ix->list_offsets.p, ix->tile_offsets.p, ix->wkey_tiled.p,
                          wq.charge, wq.tol, wq.mode, ix->win_ranges.p,
                          prof_counts() ? prof_scanned_dev() : nullptr));   // work: sum of hi - lo
    rg.range = ix->win_ranges.p;
    rg.row_len = mode_ == 1 ? wq.row_len : nullptr;
    rq.rows_filtered = rg.row_len != nullptr;
  } else {
    ASL_TRY(take_post_filter(ix, rq, mode_, ix->ids_tiled.p, ix->n_tile_slots, pf));
  }
  const unsigned long long *sel = nullptr;
  if (rq.sel_keep) ASL_TRY(selector_words(ix, rq, rq.win != nullptr, &sel));
  // a plain request (no window, selector or gate, the whole index here) is scanned from the sub-quantiser-major
  // copy: same tiles, same slots, same results; the bytes of a query's all-zero sub-vectors are not fetched
  const bool mm = ix->scan_mmajor && !rq.win && !rq.sel_keep && !rq.gate && ix->shard_world == 1 && !ix->has_vids;
  if (mm) ASL_TRY(index_codes_mmajor(ix));
  const bool use_mm = mm && ix->mm_ready;
  ProfScope ps("scan");     // the scan kernel itself
  return pq_scan_v3(rq.xq, nq, ix->d, ix->codebooks_t.p, ix->dsub, cD, cI,
                    nprobe, ix->list_offsets.p, ix->tile_offsets.p,
                    rq.win ? ix->wcodes_tiled.p : ix->codes_tiled.p, rq.win ? ix->wids_tiled.p : ix->ids_tiled.p,
                    rq.k, rq.D, rq.I64, rq.I32, mode_, q_ent, q_cnt, rq.gate, &pf, &rg, sel,
                    use_mm ? ix->codes_mm.p : nullptr, use_mm ? ix->mm_plane : 0u);
}

// IVF-PQ: coarse stage, then the tiled scan or the generic kernel (which takes no post-filter)
static int search_ivfpq(asl_index *ix, IndexSearch &rq, const SearchPlan &pl) {
  const int nq = rq.nq, nprobe = pl.nprobe;
  bool own_ent = false;
  if (!rq.pre_D)
    ASL_TRY(coarse_search(ix, rq.xq, nq, nprobe, nullptr, nullptr, nullptr, nullptr, &own_ent, rq.pre_ent, rq.pre_cnt,
                          rq.pre_over));
  // search_preassigned: the caller's probe lists, read where they lie (see search_ivfflat)
  const float *cD = rq.pre_D ? rq.pre_D : ix->coarse_D.p;
  const int32_t *cI = rq.pre_D ? rq.pre_I : ix->coarse_I.p;
  // by_residual off: the probes select the lists as ever, their scores add nothing (whoever computed them)
  if (!ix->by_residual) ASL_TRY(index_zero_coarse(ix, (size_t)nq * nprobe, &cD));
  uint64_t *upper = nullptr;
  if (pl.tiled) {
    ASL_TRY(scan_pq_tiled(ix, rq, pl, cD, cI, own_ent));
  } else {
    const int k = rq.k;
    ASL_TRY(pass_bounds(ix, rq, &upper));
    auto out_at = [&](auto *base, int c0) { return base ? base + c0 : nullptr; };
    ProfScope ps("scan");
    for (int c0 = 0; c0 < k; c0 += TK_MAX_K) {
      const int kp = std::min<int>(TK_MAX_K, k - c0);
      ASL_TRY(pq_scan(rq.xq, nq, ix->d, ix->codebooks.p, ix->pq_m, ix->ksub, ix->dsub, cD, cI, nprobe,
                      ix->list_offsets.p, ix->ids.p, ix->codes.p, kp, out_at(rq.D, c0), out_at(rq.I64, c0),
                      out_at(rq.I32, c0), k, c0 ? upper : nullptr, upper));
    }
  }
  // (the window scan's ranges counted its own work)
  if (!rq.gate && !rq.win) ASL_TRY(count_scanned(ix, cI, nq, nprobe));
  return upper ? sync_stream() : ASL_OK;
}

// IVF-PQ with the exact re-rank: the scan's k' best as an unfiltered set, refine.hip keeps the k best
static int search_ivfpq_refined(asl_index *ix, IndexSearch &rq, const SearchPlan &pl) {
  IndexSearch scan = rq;
  scan.k = pl.k_scan;
  ASL_TRY(ix->ws_short.reserve((size_t)rq.nq * scan.k));
  scan.D = nullptr;
  scan.I64 = nullptr;
  scan.I32 = ix->ws_short.p;
  scan.rows = ROWS_SET;
  scan.post = nullptr;
  ASL_TRY(search_ivfpq(ix, scan, pl));
  ProfScope ps("refine");
  return refine_topk(rq.xq, rq.nq, ix->d, ix->ws_short.p, nullptr, scan.k, ix->r_dim.p, ix->r_val.p, ix->r_cnt.p,
                     ix->r_n, rq.k, rq.D, rq.I64, rq.I32);
}

// Search with all-device arguments (index.hpp: IndexSearch).
int index_search_device(asl_index *ix, IndexSearch &rq) {
  rq.rows_filtered = false;
  SearchPlan pl;
  ASL_TRY(validate(ix, rq, pl));
  if (rq.nq <= 0) return ASL_OK;
  if (ix->kind == ASL_INDEX_FLAT) return search_gemm_topk(ix, rq, nullptr, 0);
  if (ix->kind == ASL_INDEX_WINFLAT) return search_winflat(ix, rq, pl);
  if (ix->kind == ASL_INDEX_IVFFLAT) return search_ivfflat(ix, rq, pl);
  return pl.refine ? search_ivfpq_refined(ix, rq, pl) : search_ivfpq(ix, rq, pl);
}

// window scan of asl_search_batch: the index's mode, the key of library `serial` (installed when the
// layout holds another key or the lists changed; synchronises -- call before the batch forks into
// streams), the window of the next search
int index_window_prepare(asl_index *ix, uint64_t serial, uint64_t gen, const float *key, int64_t n, int nq,
                         int nprobe) {
  if (!ix->trained) return fail(ASL_ERR_STATE, "search: index is not trained");
  // (the window-exact index: a stale layout is rebuilt in key order at once, not in id order first)
  if (ix->kind != ASL_INDEX_WINFLAT) ASL_TRY(build_lists(ix));
  if (ix->lists_dirty || !ix->win_ready || ix->win_serial != serial || ix->win_gen != gen) {
    ASL_TRY(pipeline_drain());     // batches in flight may still scan the layout about to be rewritten
    ASL_TRY(window_install(ix, n, key, serial, gen));
  }
  return ix->win_ranges.reserve((size_t)std::max(nq, 1) * std::max(1, std::min(nprobe, ix->nlist)));
}

// The two halves of an IVF search for the two-stream pipeline (search.hip): the coarse
// quantiser into caller-owned buffers, then index_search_device with those as pre_D / pre_I.
int index_nprobe(const asl_index *ix, int nprobe) {
  return !ivf_kind(ix->kind) ? 0 : std::max(1, std::min(nprobe, ix->nlist));
}
int index_prepare(asl_index *ix) {   // everything that may allocate or synchronise, up front
  if (!ix->trained) return fail(ASL_ERR_STATE, "search: index is not trained");
  if (!ivf_kind(ix->kind)) return ASL_OK;      // (the window-exact layout: index_window_prepare)
  if (coarse_sparse_supported(ix->d, ix->nlist)) ASL_TRY(coarse_transposed(ix));
  return build_lists(ix);
}
// sharded.hip: k' when the exact re-rank is usable, else 0
int index_refine_k(const asl_index *ix) {
  return (ix->refine_rows && !ix->refine_bad && ix->r_n == ix->ntotal) ? ix->refine_k : 0;
}

// The tail the staging entries of the C ABI share: rows D / I [n] that may live on the host are staged, `call` fills
// the device rows, they are copied back; the stream is waited for when anything was staged (staged_in: an input was).
template <class F>
static int with_staged_rows(float *D, int64_t *I, size_t n, bool staged_in, F call) {
  Out<float> dD;
  Out<int64_t> dI;
  ASL_TRY(dD.init(D, n));
  ASL_TRY(dI.init(I, n));
  ASL_TRY(call(dD.d, dI.d));
  ASL_TRY(dD.finish());
  ASL_TRY(dI.finish());
  if (dD.to_host() || dI.to_host() || staged_in) ASL_TRY(sync_stream());
  return ASL_OK;
}

}  // namespace asl

using namespace asl;

extern "C" {

// 1 when asl_index_search_preassigned can emit packed 64-bit keys (unordered mode 2) for this
// index at (k, nprobe): the predicate index_search_device applies, for callers that must
// choose the exchange format up front (ann_solo_amd/distributed.py).
// IVF-Flat: the answer depends on the vectors THIS handle stores (has_inv: an empty or dense shard
// has no postings), so a stale layout is rebuilt first -- the value is then what a search meets --
// and sharded drivers agree on it across ranks before they pick the exchange format.
int asl_index_supports_keys(asl_index_t *ix, int32_t k, int32_t nprobe) {
  if (!ix) return 0;
  nprobe = std::max(1, std::min(nprobe, ix->nlist));
  if (ix->kind == ASL_INDEX_IVFFLAT) {    // the postings scan's set finish (flat_scan.hip)
    if (ix->lists_dirty && ix->trained && (ensure_device() != ASL_OK || build_lists(ix) != ASL_OK)) return 0;
    return postings_ok(ix, k, nprobe) && keys_fit(k);
  }
  if (ix->kind != ASL_INDEX_IVFPQ) return 0;
  return tiled_shape_ok(ix, k, nprobe) && keys_fit(k);
}

int asl_index_coarse(asl_index_t *ix, int32_t nq, const float *xq, int32_t nprobe,
                     float *coarse_D, int32_t *coarse_I) {
  clear_error();
  if (!ix || !ivf_kind(ix->kind) || !ix->trained)
    return fail(ASL_ERR_STATE, "coarse: trained IVF index required");
  if (nq <= 0) return ASL_OK;
  ASL_TRY(clamp_nprobe(ix, &nprobe, "coarse"));
  In<float> dq;
  ASL_TRY(dq.init(xq, (size_t)nq * ix->d));
  ASL_TRY(coarse_search(ix, dq.d, nq, nprobe, nullptr, nullptr, nullptr, nullptr, nullptr));
  if (coarse_D)
    HIP_TRY(hipMemcpyAsync(coarse_D, ix->coarse_D.p, (size_t)nq * nprobe * 4, hipMemcpyDefault, stream()));
  if (coarse_I)
    HIP_TRY(hipMemcpyAsync(coarse_I, ix->coarse_I.p, (size_t)nq * nprobe * 4, hipMemcpyDefault, stream()));
  return sync_stream();
}

int asl_index_postings_work(asl_index_t *ix, int32_t nq, const float *xq, int32_t nprobe,
                            int64_t *bytes, int64_t *lines) {
  clear_error();
  if (!ix || ix->kind != ASL_INDEX_IVFFLAT || !ix->trained)
    return fail(ASL_ERR_STATE, "postings_work: trained IVF-Flat index required");
  if (bytes) *bytes = 0;
  if (lines) *lines = 0;
  if (nq <= 0) return ASL_OK;
  ASL_TRY(ensure_device());
  ASL_TRY(clamp_nprobe(ix, &nprobe, "postings_work"));
  ASL_TRY(build_lists(ix));
  if (!ix->has_inv) return fail(ASL_ERR_STATE, "postings_work: the index holds no postings (dense vectors)");
  In<float> dq;
  ASL_TRY(dq.init(xq, (size_t)nq * ix->d));
  ASL_TRY(coarse_search(ix, dq.d, nq, nprobe, nullptr, nullptr, nullptr, nullptr, nullptr));
  DevBuf<unsigned long long> acc;
  ASL_TRY(acc.reserve(2));
  HIP_TRY(hipMemsetAsync(acc.p, 0, 16, stream()));
  ASL_TRY(flat_postings_work(postings_view(ix), dq.d, nq, ix->coarse_I.p, nprobe, acc.p));
  unsigned long long h[2] = {0, 0};
  ASL_TRY(acc.download(h, 2));
  ASL_TRY(sync_stream());
  if (bytes) *bytes = (int64_t)h[0];
  if (lines) *lines = (int64_t)h[1];
  return ASL_OK;
}

int asl_index_pq_lut(asl_index_t *ix, int32_t nq, const float *xq, float *lut) {
  clear_error();
  if (!ix || ix->kind != ASL_INDEX_IVFPQ || !ix->trained)
    return fail(ASL_ERR_STATE, "pq_lut: trained IVF-PQ index required");
  if (nq <= 0) return ASL_OK;
  In<float> dq;
  Out<float> dl;
  ASL_TRY(dq.init(xq, (size_t)nq * ix->d));
  ASL_TRY(dl.init(lut, (size_t)nq * ix->pq_m * ix->ksub));
  ASL_TRY(pq_lut(dq.d, nq, ix->d, ix->codebooks.p, ix->pq_m, ix->ksub, ix->dsub, dl.d));
  ASL_TRY(dl.finish());
  return sync_stream();
}

int asl_index_search(asl_index_t *ix, int32_t nq, const float *xq, int32_t k, int32_t nprobe,
                     float *D, int64_t *I) {
  clear_error();
  if (!ix) return fail(ASL_ERR_INVALID, "search: null index");
  if (nq <= 0) return ASL_OK;
  if (!xq || !I) return fail(ASL_ERR_INVALID, "search: null xq / I");
  ASL_TRY(ensure_device());
  In<float> dq;
  ASL_TRY(dq.init(xq, (size_t)nq * ix->d));
  return with_staged_rows(D, I, (size_t)nq * k, dq.own.p, [&](float *dD, int64_t *dI) {
    IndexSearch rq{.nq = nq, .xq = dq.d, .k = k, .nprobe = nprobe, .D = dD, .I64 = dI};
    return index_search_device(ix, rq);
  });
}

int asl_index_search_window(asl_index_t *ix, int32_t nq, const float *xq, const double *q_pmz, int32_t charge,
                            double tol, int32_t mode, int32_t k, int32_t nprobe, float *D, int64_t *I) {
  clear_error();
  ASL_TRY(ensure_device());
  if (!ix) return fail(ASL_ERR_INVALID, "search_window: null index");
  if (nq <= 0) return ASL_OK;
  if (!xq || !q_pmz || !I) return fail(ASL_ERR_INVALID, "search_window: null xq / q_pmz / I");
  if (mode != ASL_TOL_DA && mode != ASL_TOL_PPM && mode != ASL_TOL_INTERVAL)
    return fail(ASL_ERR_INVALID, "search_window: mode must be Da, ppm or interval");
  if (ix->kind != ASL_INDEX_WINFLAT)
    if (const char *why = window_unsupported(ix)) return fail(ASL_ERR_STATE, "%s", why);
  if (!ix->trained) return fail(ASL_ERR_STATE, "search: index is not trained");
  // (the window-exact index: add and reset dropped the key with the layout -- nothing is rebuilt to find that out)
  if (ix->kind != ASL_INDEX_WINFLAT || !ix->lists_dirty) ASL_TRY(build_lists(ix));
  if (!ix->win_ready || (ix->kind == ASL_INDEX_WINFLAT && ix->lists_dirty))
    return fail(ASL_ERR_STATE, "search_window: no window key (asl_index_set_window_key), or the lists changed since");
  In<float> dq;
  In<double> dp;
  ASL_TRY(dq.init(xq, (size_t)nq * ix->d));
  ASL_TRY(dp.init(q_pmz, (size_t)nq * (mode == ASL_TOL_INTERVAL ? 2 : 1)));
  return with_staged_rows(D, I, (size_t)nq * k, dq.own.p || dp.own.p, [&](float *dD, int64_t *dI) {
    IndexWindow w{.q_pmz = dp.d, .tol = tol, .mode = mode, .charge = charge};
    IndexSearch rq{.nq = nq, .xq = dq.d, .k = k, .nprobe = nprobe, .D = dD, .I64 = dI, .win = &w};
    return index_search_device(ix, rq);
  });
}

int asl_index_set_selector(asl_index_t *ix, int64_t n, const uint8_t *keep) {
  clear_error();
  ASL_TRY(ensure_device());       // (waits for batches in flight: they may still read the words)
  if (!ix) return fail(ASL_ERR_INVALID, "set_selector: null index");
  if (n == 0 || !keep) {
    ix->has_selector = false;
    return ASL_OK;
  }
  if (n != ix->ntotal)
    return fail(ASL_ERR_INVALID, "set_selector: %lld flags for %lld vectors", (long long)n, (long long)ix->ntotal);
  if (ivf_kind(ix->kind) && ix->trained) ASL_TRY(build_lists(ix));   // (a rebuild later drops the selector)
  ix->has_selector = false;
  ASL_TRY(ix->selector.reserve((size_t)n));
  HIP_TRY(hipMemcpyAsync(ix->selector.p, keep, (size_t)n, hipMemcpyDefault, stream()));
  ASL_TRY(sync_stream());         // a host array is the caller's again on return
  ix->has_selector = true;
  ++ix->selector_gen;
  return ASL_OK;
}

int asl_index_search_selected(asl_index_t *ix, int32_t nq, const float *xq, const double *q_pmz, int32_t charge,
                              double tol, int32_t mode, int32_t k, int32_t nprobe, float *D, int64_t *I) {
  clear_error();
  ASL_TRY(ensure_device());
  if (!ix) return fail(ASL_ERR_INVALID, "search_selected: null index");
  if (nq <= 0) return ASL_OK;
  if (!xq || !I) return fail(ASL_ERR_INVALID, "search_selected: null xq / I");
  if (q_pmz && mode != ASL_TOL_DA && mode != ASL_TOL_PPM && mode != ASL_TOL_INTERVAL)
    return fail(ASL_ERR_INVALID, "search_selected: mode must be Da, ppm or interval");
  if (ix->kind == ASL_INDEX_FLAT) return fail(ASL_ERR_STATE, "a selector needs an IVF index (not a Flat index)");
  if (ix->kind == ASL_INDEX_WINFLAT)
    return fail(ASL_ERR_STATE, "search_selected: a window-exact index takes a selection through its key column "
                               "(NaN: unselected), not a selector");
  if (!ix->trained) return fail(ASL_ERR_STATE, "search: index is not trained");
  ASL_TRY(build_lists(ix));
  if (!ix->has_selector)
    return fail(ASL_ERR_STATE, "search_selected: no selector (asl_index_set_selector), or the lists changed since "
                               "it was set");
  if (q_pmz) {
    if (const char *why = window_unsupported(ix)) return fail(ASL_ERR_STATE, "%s", why);
    if (!ix->win_ready)
      return fail(ASL_ERR_STATE, "search_selected: no window key (asl_index_set_window_key), or the lists changed since");
  }
  In<float> dq;
  In<double> dp;
  ASL_TRY(dq.init(xq, (size_t)nq * ix->d));
  if (q_pmz) ASL_TRY(dp.init(q_pmz, (size_t)nq * (mode == ASL_TOL_INTERVAL ? 2 : 1)));
  return with_staged_rows(D, I, (size_t)nq * k, dq.own.p || dp.own.p, [&](float *dD, int64_t *dI) {
    IndexWindow w{.q_pmz = dp.d, .tol = tol, .mode = mode, .charge = charge};
    IndexSearch rq{.nq = nq, .xq = dq.d, .k = k, .nprobe = nprobe, .D = dD, .I64 = dI, .serial = 0,
                   .gen = ix->selector_gen, .win = q_pmz ? &w : nullptr, .sel_keep = ix->selector.p, .sel_n = ix->ntotal};
    return index_search_device(ix, rq);
  });
}

int asl_index_search_preassigned(asl_index_t *ix, int32_t nq, const float *xq, int32_t k,
                                 int32_t nprobe, const float *coarse_D,
                                 const int32_t *coarse_I, float *D, int64_t *I) {
  clear_error();
  if (ix && ix->kind == ASL_INDEX_WINFLAT)
    return fail(ASL_ERR_STATE, "search_preassigned: a window-exact index has no probe lists");
  if (!ix || ix->kind == ASL_INDEX_FLAT)
    return fail(ASL_ERR_INVALID, "search_preassigned: IVF index required");
  if (nq <= 0) return ASL_OK;
  if (!xq || !I || !coarse_D || !coarse_I) return fail(ASL_ERR_INVALID, "search_preassigned: null argument");
  if (nprobe < 1 || nprobe > ix->nlist) return fail(ASL_ERR_INVALID, "search_preassigned: nprobe outside 1..nlist");
  ASL_TRY(ensure_device());
  In<float> dq, dcD;
  In<int32_t> dcI;
  ASL_TRY(dq.init(xq, (size_t)nq * ix->d));
  ASL_TRY(dcD.init(coarse_D, (size_t)nq * nprobe));
  ASL_TRY(dcI.init(coarse_I, (size_t)nq * nprobe));
  return with_staged_rows(D, I, (size_t)nq * k, dq.own.p || dcD.own.p || dcI.own.p, [&](float *dD, int64_t *dI) {
    IndexSearch rq{.nq = nq, .xq = dq.d, .k = k, .nprobe = nprobe, .D = dD, .I64 = dI, .pre_D = dcD.d, .pre_I = dcI.d};
    return index_search_device(ix, rq);
  });
}

// search_preassigned over a list whose length only the device knows: a launch for `cap` rows
// of which the first *count (device memory) are searched; the other rows of D / I are left
// untouched. Device pointers only; never waits.
int asl_index_search_gated(asl_index_t *ix, int32_t cap, const float *xq, int32_t k, int32_t nprobe,
                           const float *coarse_D, const int32_t *coarse_I, float *D, int64_t *I,
                           const int32_t *count) {
  clear_error();
  if (ix && ix->kind == ASL_INDEX_WINFLAT)
    return fail(ASL_ERR_STATE, "search_gated: a window-exact index has no probe lists");
  if (!ix || ix->kind == ASL_INDEX_FLAT) return fail(ASL_ERR_INVALID, "search_gated: IVF index required");
  if (cap <= 0) return ASL_OK;
  if (!xq || !I || !coarse_D || !coarse_I || !count) return fail(ASL_ERR_INVALID, "search_gated: null argument");
  if (nprobe < 1 || nprobe > ix->nlist) return fail(ASL_ERR_INVALID, "search_gated: nprobe outside 1..nlist");
  ASL_TRY(ensure_device());
  if (!is_device_ptr(xq) || !is_device_ptr(I) || !is_device_ptr(coarse_D) || !is_device_ptr(coarse_I) ||
      !is_device_ptr(count) || (D && !is_device_ptr(D)))
    return fail(ASL_ERR_INVALID, "search_gated: device pointers only");
  IndexSearch rq{.nq = cap, .xq = xq, .k = k, .nprobe = nprobe, .D = D, .I64 = I, .pre_D = coarse_D, .pre_I = coarse_I,
                 .gate = reinterpret_cast<const int *>(count)};
  return index_search_device(ix, rq);
}

// search_preassigned with the queries as ENTRY LISTS (asl_encode_entries_batch: entries [nq][64]
// word pairs, counts [nq]) instead of dense rows: what the layout-specific scans read anyway -- 512
// bytes per query instead of 3.2 KB, and no listing pass. Results are those of
// asl_index_search_preassigned on the dense rows, bit for bit. A row whose count is negative (more
// than 64 non-zeros) is searched as an all-zero query: check the n_over the encoder reported. `count`
// (may be null): a device int -- only the first *count rows are searched, the launch covers nq
// (asl_index_search_gated). Device pointers only; never waits.
int asl_index_search_entries(asl_index_t *ix, int32_t nq, const uint32_t *entries, const int32_t *counts,
                             int32_t k, int32_t nprobe, const float *coarse_D, const int32_t *coarse_I,
                             float *D, int64_t *I, const int32_t *count) {
  clear_error();
  if (ix && ix->kind == ASL_INDEX_WINFLAT)
    return fail(ASL_ERR_STATE, "search_entries: a window-exact index has no probe lists");
  if (!ix || ix->kind == ASL_INDEX_FLAT) return fail(ASL_ERR_INVALID, "search_entries: IVF index required");
  if (nq <= 0) return ASL_OK;
  if (!entries || !counts || !I || !coarse_D || !coarse_I) return fail(ASL_ERR_INVALID, "search_entries: null argument");
  if (nprobe < 1 || nprobe > ix->nlist) return fail(ASL_ERR_INVALID, "search_entries: nprobe outside 1..nlist");
  ASL_TRY(ensure_device());
  if (!is_device_ptr(entries) || !is_device_ptr(counts) || !is_device_ptr(I) || !is_device_ptr(coarse_D) ||
      !is_device_ptr(coarse_I) || (count && !is_device_ptr(count)) || (D && !is_device_ptr(D)))
    return fail(ASL_ERR_INVALID, "search_entries: device pointers only");
  IndexSearch rq{.nq = nq, .k = k, .nprobe = nprobe, .D = D, .I64 = I, .pre_D = coarse_D, .pre_I = coarse_I,
                 .pre_ent = reinterpret_cast<const uint2 *>(entries), .pre_cnt = counts,
                 .gate = reinterpret_cast<const int *>(count)};
  return index_search_device(ix, rq);
}

int asl_index_refine(asl_index_t *ix, int32_t nq, const float *xq, int32_t kp, const int64_t *I_in,
                     int32_t k, float *D, int64_t *I) {
  clear_error();
  if (!ix || !xq || !I_in || !I) return fail(ASL_ERR_INVALID, "refine: null argument");
  if (!ix->refine_rows || ix->r_n != ix->ntotal)
    return fail(ASL_ERR_STATE, "refine: the index stores no exact rows (asl_index_set_refine before add)");
  if (ix->refine_bad) return fail(ASL_ERR_CAPACITY, "refine: a stored vector has more than %d non-zeros", refine_stride());
  if (nq <= 0) return ASL_OK;
  if (k <= 0 || k > kp || kp > TK_MAX_K) return fail(ASL_ERR_INVALID, "refine: need 0 < k <= k' <= %d", TK_MAX_K);
  ASL_TRY(ensure_device());
  In<float> dq;
  In<int64_t> dI;
  ASL_TRY(dq.init(xq, (size_t)nq * ix->d));
  ASL_TRY(dI.init(I_in, (size_t)nq * kp));
  return with_staged_rows(D, I, (size_t)nq * k, dq.own.p || dI.own.p, [&](float *oD, int64_t *oI) {
    return refine_topk(dq.d, nq, ix->d, nullptr, dI.d, kp, ix->r_dim.p, ix->r_val.p, ix->r_cnt.p, ix->r_n, k, oD, oI,
                       nullptr);
  });
}

int asl_topk_merge(int32_t S, int32_t nq, int32_t k, const float *Ds, const int64_t *Is,
                   float *D, int64_t *I) {
  clear_error();
  if (S <= 0 || nq < 0 || k <= 0 || !Ds || !Is || !D || !I) return fail(ASL_ERR_INVALID, "topk_merge: bad arguments");
  if (nq == 0) return ASL_OK;
  ASL_TRY(ensure_device());
  In<float> dDs;
  In<int64_t> dIs;
  ASL_TRY(dDs.init(Ds, (size_t)S * nq * k));
  ASL_TRY(dIs.init(Is, (size_t)S * nq * k));
  return with_staged_rows(D, I, (size_t)nq * k, dDs.own.p || dIs.own.p, [&](float *dD, int64_t *dI) {
    return topk_merge(dDs.d, dIs.d, S, nq, k, dD, dI);
  });
}

int asl_topk_merge_keys(int32_t S, int32_t nq, int32_t k, const int64_t *Ks, float *D, int64_t *I,
                        int32_t unordered) {
  clear_error();
  if (S <= 0 || nq < 0 || k <= 0 || !Ks || !I) return fail(ASL_ERR_INVALID, "topk_merge_keys: bad arguments");
  if (nq == 0) return ASL_OK;
  ASL_TRY(ensure_device());
  In<int64_t> dKs;
  ASL_TRY(dKs.init(Ks, (size_t)S * nq * k));
  return with_staged_rows(D, I, (size_t)nq * k, dKs.own.p, [&](float *dD, int64_t *dI) {
    return topk_merge_keys(dKs.d, S, nq, k, dD, dI, unordered ? 1 : 0);
  });
}

}  // extern "C"
