// window_search.hip -- the window-only (brute-force) search: cascade level 'std', --mode bf
// (SpectralLibrary._get_library_candidates, spectral_library.py:417-455, without the index). The reference
// builds a dense nq x N boolean mask; here every query's window is one run of the precursor-sorted view of
// the library, found by binary search, so nothing is O(nq*N).
#include "library.hpp"

namespace asl {

// Window [lo,hi) of each query inside the precursor-sorted library (q_pmz: [nq, 2] with ASL_TOL_INTERVAL,
// where the walk is lower_bound(lo), upper_bound(hi)).
__global__ void window_range_kernel(const double *__restrict__ q_pmz, int nq,
                                    const float *__restrict__ sorted_pmz, int n, int charge,
                                    double tol, int mode, int32_t *__restrict__ lo_out,
                                    int32_t *__restrict__ cnt_out) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const QueryWindow w = query_window(q_pmz, q, mode);
  const double qm = w.q;
  int a = 0, b = n;  // p0 = first element with (double)l >= qm
  while (a < b) {
    const int mid = (a + b) >> 1;
    if ((double)sorted_pmz[mid] < qm) a = mid + 1; else b = mid;
  }
  const int p0 = a;
  // (interval: p0 is lower_bound(lo) and nothing left of it passes; a NaN bound or lo > hi: no run)
  a = mode == ASL_TOL_INTERVAL ? p0 : 0; b = p0;     // left side: first index whose value passes
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (precursor_ok(qm, sorted_pmz[mid], charge, tol, mode)) b = mid; else a = mid + 1;
  }
  const int lo = a;
  a = p0; b = (mode == ASL_TOL_INTERVAL && !(w.q <= w.hi)) ? p0 : n;     // right side: first index whose value fails
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (precursor_ok(w, sorted_pmz[mid], charge, tol, mode)) a = mid + 1; else b = mid;
  }
  lo_out[q] = lo;
  cnt_out[q] = a - lo;
}

__global__ void window_fill_kernel(const int32_t *__restrict__ lo, const int32_t *__restrict__ offsets,
                                   const int32_t *__restrict__ sorted_row,
                                   const uint8_t *__restrict__ valid, int32_t *__restrict__ cand) {
  const int q = blockIdx.x;
  const int b = offsets[q], n = offsets[q + 1] - b, l = lo[q];
  for (int t = threadIdx.x; t < n; t += blockDim.x) {
    const int32_t row = sorted_row[l + t];
    cand[b + t] = (!valid || valid[row]) ? row : -1;
  }
}

}  // namespace asl

using namespace asl;

// Pairs one rescoring pass of a window-only search may hold (asl_set_window_pair_budget): 2^28
// pair scores are 2 GiB of scratch. Capped at 2^31-1 where used: the tile-local offsets are 32-bit.
static int64_t window_pair_budget = 1ll << 28;

// The queries' windows into L->lo / L->cnt (reserved here, before the launch) and, the stream synchronised,
// their sizes on the host; h_lo, where given, receives their starts too.
static int window_ranges(asl_library *L, int nq, const double *q_pmz_dev, int charge, double tol, int mode,
                         std::vector<int32_t> *h_lo, std::vector<int32_t> &h_cnt) {
  ASL_TRY(L->lo.reserve((size_t)nq));
  ASL_TRY(L->cnt.reserve((size_t)nq));
  hipLaunchKernelGGL(window_range_kernel, dim3((unsigned)cdiv(nq, 256)), dim3(256), 0, stream(),
                     q_pmz_dev, nq, L->sorted_pmz.p, (int)L->n, charge, tol, mode, L->lo.p, L->cnt.p);
  ASL_CHECK_LAUNCH();
  if (h_lo) {
    h_lo->resize((size_t)nq);
    ASL_TRY(L->lo.download(h_lo->data(), (size_t)nq));
  }
  h_cnt.resize((size_t)nq);
  ASL_TRY(L->cnt.download(h_cnt.data(), (size_t)nq));
  return sync_stream();
}

// CSR window candidates on the device: fills L->woff ([nq+1], = h_off) and L->cand.
static int window_candidates_device(asl_library *L, int nq, const double *q_pmz_dev, int charge,
                                    double tol, int mode, std::vector<int32_t> &h_off) {
  ASL_TRY(L->woff.reserve((size_t)nq + 1));
  std::vector<int32_t> h_cnt;
  h_off.assign((size_t)nq + 1, 0);
  ASL_TRY(window_ranges(L, nq, q_pmz_dev, charge, tol, mode, nullptr, h_cnt));
  int64_t acc = 0;
  for (int q = 0; q < nq; q++) {
    h_off[(size_t)q] = (int32_t)acc;
    acc += h_cnt[(size_t)q];
    if (acc > 0x7fffffffLL)
      return fail(ASL_ERR_CAPACITY, "window: more than 2^31-1 candidate pairs in one batch; "
                                    "use a smaller batch_size for brute-force open search");
  }
  h_off[(size_t)nq] = (int32_t)acc;
  ASL_TRY(L->woff.upload(h_off.data(), (size_t)nq + 1));
  ASL_TRY(L->cand.reserve((size_t)std::max<int64_t>(acc, 1)));
  hipLaunchKernelGGL(window_fill_kernel, dim3(nq), dim3(256), 0, stream(), L->lo.p, L->woff.p,
                     L->sorted_row.p, L->valid_col(), L->cand.p);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// Window-only search of one batch (use_ann = 0: cascade level 'std', --mode bf). A query's
// candidates are the run sorted_row[lo[q], lo[q] + cnt[q]) of the precursor-sorted view, read in
// place by the rescoring kernels (rescore.hpp: WindowRows) -- no candidate list. The batch's pairs,
// counted in 64 bits, are cut into tiles of at most window_pair_budget pairs; a tile is a run of
// queries whose first and last may bring only part of their window. One tile (every batch whose
// pairs fit): the rescoring as for any list. Several: each tile's n best (n = 1: its argmax) are
// folded into the running n best (rescore_window_merge), then one pass over an n-candidate list per
// query -- its winners -- emits the peak matches. Scratch: pair scores of one tile, 12 bytes per winner.
int asl::window_search_device(const SearchBatch &b) {
  asl_library *L = b.L;
  const asl_search_params_t *P = b.P;
  const BatchOut &out = b.out;
  const int nq = b.Q.n;
  const int n = std::max(b.n_best, 1);
  const size_t nw = b.winners();
  std::vector<int32_t> h_lo, h_cnt;
  {
    ProfScope ps("filter");
    ASL_TRY(window_ranges(L, nq, b.window_operand(), P->charge, P->precursor_tol, P->precursor_mode, &h_lo, h_cnt));
  }
  std::vector<int64_t> pre((size_t)nq + 1, 0);     // exclusive prefix of the window sizes
  for (int q = 0; q < nq; q++) pre[(size_t)q + 1] = pre[(size_t)q] + h_cnt[(size_t)q];
  const int64_t total = pre[(size_t)nq];
  if (total == 0) {   // what the rescoring writes for empty lists
    HIP_TRY(hipMemsetAsync(L->status.p, 0, sizeof(int), stream()));
    if (out.best_row) HIP_TRY(hipMemsetAsync(out.best_row, 0xff, nw * 4, stream()));
    if (out.best_score) HIP_TRY(hipMemsetAsync(out.best_score, 0, nw * 8, stream()));
    if (out.n_cand) HIP_TRY(hipMemsetAsync(out.n_cand, 0, (size_t)nq * 4, stream()));
    if (out.pm_count) HIP_TRY(hipMemsetAsync(out.pm_count, 0, nw * 4, stream()));
    if (out.pm_pairs) HIP_TRY(hipMemsetAsync(out.pm_pairs, 0, nw * out.pm_stride * 8, stream()));
    return ASL_OK;
  }
  const int64_t B = std::min<int64_t>(window_pair_budget, 0x7fffffffLL);
  // every buffer before the first launch (growing one synchronises the device)
  // (the winners' pass after several tiles scores one slot per winner)
  ASL_TRY(L->pair_score.reserve((size_t)(total <= B ? total : std::max<int64_t>(B, (int64_t)nw))));
  ASL_TRY(L->rs_scratch.q_defer.reserve(RescoreScratch::defer_ints((size_t)nq)));
  ASL_TRY(L->rs_scratch.m_defer.reserve(nw));
  WindowRows win{.sorted_row = L->sorted_row.p, .valid = L->valid_col()};
  RescoreRequest rq = b.rescore_request();
  library_filter(L, rq.filter);       // packed row records for the kernels, no second filtering
  rq.filter.wcol = nullptr;
  rq.filter.pass_all = true;
  if (total <= B) {   // one tile: the whole batch
    std::vector<int32_t> h((size_t)2 * nq + 1);
    for (int q = 0; q <= nq; q++) h[(size_t)q] = (int32_t)pre[(size_t)q];
    for (int q = 0; q < nq; q++) h[(size_t)nq + 1 + q] = h_lo[(size_t)q];
    ASL_TRY(L->wtile.upload(h.data(), h.size()));
    win.begin = L->wtile.p + nq + 1;
    rq.cand = {.offsets = L->wtile.p, .total_slots = total, .window = &win};
    return rescore_device(rq);
  }
  // tiles [t0, t1) of the global pair range; queries qa..qb (the query of pair t0 .. that of t1-1)
  struct Tile {
    int qa, nq;
    int64_t pairs;
    size_t idx;       // its offsets [nq + 1] and begins [nq] in wtile
  };
  std::vector<Tile> tiles;
  std::vector<int32_t> h;
  for (int64_t t0 = 0; t0 < total; t0 += B) {
    const int64_t t1 = std::min(total, t0 + B);
    const int qa = (int)(std::upper_bound(pre.begin(), pre.end(), t0) - pre.begin()) - 1;
    const int qb = (int)(std::upper_bound(pre.begin(), pre.end(), t1 - 1) - pre.begin()) - 1;
    Tile T{qa, qb - qa + 1, t1 - t0, h.size()};
    h.resize(h.size() + 2 * (size_t)T.nq + 1);
    int32_t *off = h.data() + T.idx, *beg = off + T.nq + 1;
    for (int i = 0; i < T.nq; i++) {
      const int q = qa + i;
      const int64_t s = std::max(pre[(size_t)q], t0);
      off[i] = (int32_t)(s - t0);
      beg[i] = (int32_t)(h_lo[(size_t)q] + (s - pre[(size_t)q]));
    }
    off[T.nq] = (int32_t)(t1 - t0);
    tiles.push_back(T);
  }
  ASL_TRY(L->wtile.upload(h.data(), h.size()));
  ASL_TRY(L->run_score.reserve(nw));
  ASL_TRY(L->run_row.reserve(nw));
  ASL_TRY(L->run_n.reserve((size_t)nq));
  ASL_TRY(L->tile_score.reserve(nw));
  ASL_TRY(L->tile_n.reserve((size_t)nq));
  HIP_TRY(hipMemsetAsync(L->run_score.p, 0, nw * 8, stream()));
  HIP_TRY(hipMemsetAsync(L->run_row.p, 0xff, nw * 4, stream()));
  HIP_TRY(hipMemsetAsync(L->run_n.p, 0, (size_t)nq * 4, stream()));
  HIP_TRY(hipMemsetAsync(L->status.p, 0, sizeof(int), stream()));
  rq.clear_status = false;
  for (const Tile &T : tiles) {
    RescoreRequest rt = rq;     // the tile's queries: a view of the batch from query qa on; selection only
    rt.Q.n = T.nq;
    rt.Q.offsets += T.qa;
    rt.Q.precursor_mz += T.qa;
    if (rt.Q.precursor_charge) rt.Q.precursor_charge += T.qa;
    const int32_t *off = L->wtile.p + T.idx;
    win.begin = off + T.nq + 1;
    rt.cand = {.offsets = off, .total_slots = T.pairs, .window = &win};
    // (the histogram: every tile's pass adds its part of the window into the rows of its queries)
    rt.out = {.best_score = L->tile_score.p, .n_cand = L->tile_n.p,
              .score_hist = out.score_hist ? out.score_hist + (size_t)T.qa * ASL_SCORE_HIST_BINS : nullptr};
    rt.emit_matches = false;
    ASL_TRY(rescore_device(rt));
    ASL_TRY(rescore_window_merge(rt.cand, T.nq, n, L->best_slot.p, L->tile_score.p, L->tile_n.p,
                                 L->run_score.p + (size_t)T.qa * n, L->run_row.p + (size_t)T.qa * n,
                                 L->run_n.p + T.qa, b.group()));
  }
  // the running lists once more, as an n-candidate list per query (-1: an empty rank): the same
  // order comes out again, with rows and peak matches (n_best = 0: the one winner, by the argmax)
  // (distinct: every tile's ranks and the fold hold one row per group; these lists, already distinct, are
  // ranked as they are; the winners were counted with their tiles: no histogram here)
  rq.cand = {.rows32 = L->run_row.p, .stride = n, .total_slots = (int64_t)nw};
  rq.group = nullptr;
  rq.out = {.best_row = out.best_row, .best_score = L->tile_score.p, .pm_count = out.pm_count,
            .pm_pairs = out.pm_pairs, .pm_stride = out.pm_stride};
  ASL_TRY(rescore_device(rq));
  return rescore_window_finish(nq, n, L->run_score.p, L->run_row.p, L->run_n.p, L->tile_score.p, out.best_score,
                               out.n_cand, L->status.p);
}

extern "C" {

int64_t asl_set_window_pair_budget(int64_t pairs) {
  clear_error();
  if (pairs <= 0) return fail(ASL_ERR_INVALID, "set_window_pair_budget: the budget must be positive");
  const int64_t prev = window_pair_budget;
  window_pair_budget = pairs;
  return prev;
}

int asl_window_candidates(asl_library_t *L, int32_t nq, const double *query_pmz, int32_t charge,
                          double tol, int32_t mode, int32_t *cand_offsets, int64_t *cand_rows) {
  clear_error();
  if (!L || nq < 0 || !cand_offsets) return fail(ASL_ERR_INVALID, "window_candidates: bad arguments");
  if (nq == 0) {
    cand_offsets[0] = 0;
    return ASL_OK;
  }
  In<double> dq;
  ASL_TRY(dq.init(query_pmz, (size_t)nq * (mode == ASL_TOL_INTERVAL ? 2 : 1)));
  std::vector<int32_t> h_off;
  ASL_TRY(window_candidates_device(L, nq, dq.d, charge, tol, mode, h_off));
  const size_t total = (size_t)h_off[(size_t)nq];
  std::vector<int32_t> h_cand(total);
  if (total) ASL_TRY(L->cand.download(h_cand.data(), total));
  ASL_TRY(sync_stream());
  // compact invalid rows, ascending row order inside each list (spectral_library.py:451)
  std::vector<int32_t> out_off((size_t)nq + 1, 0);
  std::vector<int64_t> rows;
  rows.reserve(total);
  for (int q = 0; q < nq; q++) {
    const size_t b = rows.size();
    for (int32_t t = h_off[(size_t)q]; t < h_off[(size_t)q + 1]; t++)
      if (h_cand[(size_t)t] >= 0) rows.push_back(h_cand[(size_t)t]);
    std::sort(rows.begin() + (long)b, rows.end());
    out_off[(size_t)q + 1] = (int32_t)rows.size();
  }
  HIP_TRY(hipMemcpy(cand_offsets, out_off.data(), ((size_t)nq + 1) * 4, hipMemcpyDefault));
  if (cand_rows && !rows.empty())
    HIP_TRY(hipMemcpy(cand_rows, rows.data(), rows.size() * 8, hipMemcpyDefault));
  return ASL_OK;
}

}  // extern "C"
