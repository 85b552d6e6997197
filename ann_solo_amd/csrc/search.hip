// search.hip -- one batch of the open-modification hot path, device resident:
// SpectralLibrary._search_batch / _get_library_candidates
// (/root/reference/src/ann_solo/spectral_library.py:328-455).
//
//   encode (spectrum.py:166-214)  ->  index.search(k) (:443-444)
//   -> precursor-window post-filter (:417-429 AND :441-446)  ->  best match (:356-365)
//
// The reference builds two dense nq x N boolean masks; here the ANN ids are
// post-filtered inside the rescoring kernel's candidate compaction (rescore.hpp:
// PrecFilter) and the window-only modes
// (cascade level 'std', --mode bf) binary-search a precursor-sorted copy of the
// library, so nothing is O(nq*N).
#include <algorithm>
#include <atomic>

#include "index.hpp"
#include "rescore.hpp"

namespace asl {
int encode_device(const float *mz, const float *inten, const int32_t *offsets, int32_t n,
                  double min_bound, double bin_size, int32_t hash_len, uint32_t seed,
                  int norm, float *out);
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

// The effective columns of a library with a selection (asl_library_set_selection): the window column with
// NaN where the row is unselected (or was NaN: invalid), the validity flags with 0 there.
__global__ void selection_columns_kernel(const uint8_t *__restrict__ keep, const float *__restrict__ wcol,
                                         const uint8_t *__restrict__ valid, int64_t n,
                                         float *__restrict__ wcol_eff, uint8_t *__restrict__ valid_eff) {
  const int64_t i = block_linear() * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool on = keep[i] != 0;
  wcol_eff[i] = on ? wcol[i] : __builtin_nanf("");
  valid_eff[i] = (on && (!valid || valid[i])) ? 1 : 0;
}

}  // namespace asl

using namespace asl;

struct asl_library {
  int64_t n = 0;
  uint64_t serial = 0;    // unique in the process, never reused: what an index's window key came from
  DevBuf<int32_t> offsets, pcharge;
  DevBuf<float> mz, intensity, pmz32;
  DevBuf<uint8_t> charge, valid;
  DevBuf<double> pmz;
  // One fixed-size SLOT per row: [RowMeta 32 B][mz x n][charge x n][intensity x n]. The rescoring
  // kernels gather the row record and find the row's first ~24 m/z values in the SAME 128-byte line;
  // the address of a row's peaks is row * slot + 32, not a second, dependent look-up (round 5; until
  // then a 32-byte record array and a separately packed record per row: 4.1 lines and two hops per
  // candidate instead of 3 lines and one).
  DevBuf<uint8_t> records;   // n * slot bytes (DevPeaks::records)
  uint32_t slot = 0;         // bytes per row (a multiple of 128)
  DevBuf<float> wcol;     // window column alone, NaN for invalid spectra
  bool has_valid = false;
  // selection (asl_library_set_selection): keep[row] != 0 = selected, and the columns every search reads
  // while it is installed -- wcol_eff: NaN where unselected or invalid, valid_eff: 0 there. sel_gen counts
  // the changes (install, replace, drop): with `serial` it names what an index derived from these columns.
  DevBuf<uint8_t> keep, valid_eff;
  DevBuf<float> wcol_eff;
  bool has_sel = false;
  uint64_t sel_gen = 0;
  const float *window_col() const { return has_sel ? wcol_eff.p : wcol.p; }
  const uint8_t *valid_col() const { return has_sel ? valid_eff.p : has_valid ? valid.p : nullptr; }
  // group id per row (asl_library_set_groups; the *_topn_distinct calls rank one row per group)
  DevBuf<int32_t> group;
  bool has_group = false;
  DevPeaks dev;
  // precursor-sorted view (window search)
  DevBuf<float> sorted_pmz;
  DevBuf<int32_t> sorted_row;
  // scratch
  DevBuf<float> qvec;
  DevBuf<int32_t> knn, cand, lo, cnt, woff;
  // buffers that cross the two streams of the pipeline, by batch parity
  DevBuf<float> p_qvec[2], p_cD[2];
  DevBuf<int32_t> p_cI[2], p_knn[2], p_cnt[2];
  DevBuf<int32_t> p_rows[2], rows_len;   // lengths of the neighbour rows when the scan applied the precursor filter
  DevBuf<double> p_win[2];         // ASL_TOL_INTERVAL: the batch's intervals when the caller's array is on the host
  DevBuf<uint2> p_ent[2];          // the batch's entry lists: listed by the coarse stage, read by the scan
  bool p_have_ent[2] = {false, false};
  DevBuf<double> pair_score;
  DevBuf<long long> best_slot;
  // tiled window search: per-tile CSR offsets + begins into sorted_row, running best of the batch
  DevBuf<int32_t> wtile, run_row, run_n, tile_n;
  DevBuf<double> run_score, tile_score;
  DevBuf<int> status;
  RescoreScratch rs_scratch;       // per-query flags between the rescoring launches of THIS handle's stream
};

// one wave per spectrum: its row record and its peaks from the three arrays into its slot
__global__ void pack_records_kernel(const int32_t *__restrict__ offsets, const float *__restrict__ mz,
                                    const float *__restrict__ inten, const uint8_t *__restrict__ chg,
                                    const RowMeta *__restrict__ meta, int64_t n, uint32_t slot,
                                    uint8_t *__restrict__ rec) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= n) return;
  const int co = offsets[r], cn = offsets[r + 1] - co;
  uint8_t *s0 = rec + (size_t)r * slot;
  if (lane < 8) reinterpret_cast<uint32_t *>(s0)[lane] = reinterpret_cast<const uint32_t *>(meta + r)[lane];
  uint8_t *b = rec + (size_t)meta[r].rec4 * 4;      // = s0 + 32
  float *f = reinterpret_cast<float *>(b);
  for (int j = lane; j < cn; j += 64) {
    f[j] = mz[co + j];
    b[4 * (size_t)cn + j] = chg[co + j];
    f[rec_int0(cn) + j] = inten[co + j];
  }
}

static int pack_peak_records(const int32_t *offsets, const float *mz, const float *inten,
                             const uint8_t *chg, const RowMeta *meta, int64_t n, uint32_t slot, uint8_t *rec) {
  if (n <= 0) return ASL_OK;
  hipLaunchKernelGGL(pack_records_kernel, dim3((unsigned)cdiv(n, 4)), dim3(256), 0, stream(), offsets,
                     mz, inten, chg, meta, n, slot, rec);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

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
static bool scan_postfilter_on() { return scan_postfilter_flag() == 1; }

// Pairs one rescoring pass of a window-only search may hold (asl_set_window_pair_budget): 2^28
// pair scores are 2 GiB of scratch. Capped at 2^31-1 where used: the tile-local offsets are 32-bit.
static int64_t &window_pair_budget() {
  static int64_t b = 1ll << 28;
  return b;
}
// What the window test of a batch reads per query: the queries' precursor m/z or, with ASL_TOL_INTERVAL, the
// intervals of asl_search_params_t::precursor_window on the device (`win`: [nq, 2])
static const double *window_operand(const DevPeaks &Q, const asl_search_params_t *P, const double *win) {
  return P->precursor_mode == ASL_TOL_INTERVAL ? win : Q.precursor_mz;
}
static int check_window_arg(const asl_search_params_t *P, const char *who) {
  if (P->precursor_mode == ASL_TOL_INTERVAL && !P->precursor_window)
    return fail(ASL_ERR_INVALID, "%s: precursor_mode ASL_TOL_INTERVAL needs precursor_window ([nq, 2] doubles)", who);
  ScoreFlags sf;      // params->allow_shift is the score flag word: checked here, where every call enters
  return decode_score_flags(P->allow_shift, who, sf);
}
// (the checked word's two flags, for the rescoring requests)
static inline int score_shift(const asl_search_params_t *P) { return (P->allow_shift & ASL_SCORE_SHIFT) ? 1 : 0; }
static inline int score_ppm(const asl_search_params_t *P) { return (P->allow_shift & ASL_SCORE_FRAGMENT_PPM) ? 1 : 0; }
// The precursor window of a batch's scan, into its request: the window scan (asl_index_set_window_scan)
// when the index is in that mode, else -- no ordered neighbour list asked for -- the scan-side
// post-filter of THIS library's window column. row_len: the lengths of the set-mode rows.
static void offer_window(IndexSearch &rq, IndexWindow &w, const DevPeaks &Q, const asl_search_params_t *P,
                         const double *win, int32_t *row_len) {
  w = {.q_pmz = window_operand(Q, P, win), .row_len = row_len, .tol = P->precursor_tol, .mode = P->precursor_mode,
       .charge = P->charge};
  rq.win = &w;
}
static void offer_post_filter(IndexSearch &rq, IndexPostFilter &pf, const asl_library *L, const DevPeaks &Q,
                              const asl_search_params_t *P, const double *win, int32_t *row_len) {
  pf = {.payload = L->window_col(), .n = L->n, .q_pmz = window_operand(Q, P, win), .count = row_len, .tol = P->precursor_tol,
        .mode = P->precursor_mode, .charge = P->charge};
  rq.post = &pf;
}
// what every ANN batch tells the index of its library: whose columns it may have derived a layout from
// (serial, generation) and, with a selection installed, the selector
static void offer_library(IndexSearch &rq, const asl_library *L) {
  rq.serial = L->serial;
  rq.gen = L->sel_gen;
  if (L->has_sel) {
    rq.sel_keep = L->keep.p;
    rq.sel_n = L->n;
  }
}

// the precursor filter / row records of a library handle
static void library_filter(const asl_library *L, PrecFilter &flt) {
  flt.meta = reinterpret_cast<const RowMeta *>(L->records.p);
  flt.meta_stride = L->slot;
  flt.wcol = L->window_col();
}
static void batch_filter(const asl_library *L, const asl_search_params_t *P, const double *win, PrecFilter &flt) {
  flt.lib_pmz = L->pmz32.p;
  flt.valid = L->valid_col();
  library_filter(L, flt);
  flt.tol = P->precursor_tol;
  flt.mode = P->precursor_mode;
  flt.charge = P->charge;
  if (P->precursor_mode == ASL_TOL_INTERVAL) flt.interval = win;     // (shares the tolerance's slot)
}

extern "C" {

int asl_set_scan_postfilter(int on) {
  clear_error();
  int &f = scan_postfilter_flag();
  const int prev = f;
  f = on ? 1 : 0;
  return prev;
}

int64_t asl_set_window_pair_budget(int64_t pairs) {
  clear_error();
  if (pairs <= 0) return fail(ASL_ERR_INVALID, "set_window_pair_budget: the budget must be positive");
  int64_t &b = window_pair_budget();
  const int64_t prev = b;
  b = pairs;
  return prev;
}

asl_library_t *asl_library_create(const asl_peaks_t *p, const float *lib_pmz_f32,
                                  const uint8_t *valid) {
  clear_error();
  if (!p || p->n < 0) {
    fail(ASL_ERR_INVALID, "library_create: null peaks");
    return nullptr;
  }
  if (ensure_device() != ASL_OK) return nullptr;
  PeaksStage st;
  if (st.init(p) != ASL_OK) return nullptr;
  asl_library *L = new asl_library();
  static std::atomic<uint64_t> next_serial{1};
  L->serial = next_serial.fetch_add(1);
  L->n = p->n;
  const size_t n = (size_t)p->n, np = (size_t)st.dev.n_peaks;
  bool ok = true;
  auto up = [&](auto &buf, const auto *src, size_t cnt) {
    if (ok && cnt && buf.upload(src, cnt) != ASL_OK) ok = false;
  };
  up(L->offsets, st.dev.offsets, n + 1);
  up(L->mz, st.dev.mz, np);
  up(L->intensity, st.dev.intensity, np);
  if (st.dev.charge) {
    up(L->charge, st.dev.charge, np);
  } else if (np) {
    ok = ok && L->charge.reserve(np) == ASL_OK &&
         hipMemsetAsync(L->charge.p, 0, np, stream()) == hipSuccess;
  }
  up(L->pmz, st.dev.precursor_mz, n);
  up(L->pcharge, st.dev.precursor_charge, n);
  // float32 precursor column + precursor-sorted view (host side: one-time, O(n log n))
  std::vector<double> h_pmz(n);
  std::vector<float> h_pmz32(n);
  if (ok && n) {
    ok = hipMemcpyAsync(h_pmz.data(), L->pmz.p, n * 8, hipMemcpyDeviceToHost, stream()) == hipSuccess &&
         sync_stream() == ASL_OK;
    if (lib_pmz_f32) {
      ok = ok && hipMemcpy(h_pmz32.data(), lib_pmz_f32, n * 4, hipMemcpyDefault) == hipSuccess;
    } else {
      for (size_t i = 0; i < n; i++) h_pmz32[i] = (float)h_pmz[i];
    }
  }
  up(L->pmz32, h_pmz32.data(), n);
  if (valid) {
    up(L->valid, valid, n);
    L->has_valid = true;
  }
  if (ok && n) {   // packed rows: invalid spectra get a NaN window column (never a candidate)
    std::vector<int32_t> h_off(n + 1), h_chg(n);
    std::vector<uint8_t> h_valid(n, 1);
    ok = hipMemcpyAsync(h_off.data(), L->offsets.p, (n + 1) * 4, hipMemcpyDeviceToHost, stream()) == hipSuccess &&
         hipMemcpyAsync(h_chg.data(), L->pcharge.p, n * 4, hipMemcpyDeviceToHost, stream()) == hipSuccess &&
         sync_stream() == ASL_OK;
    if (ok && valid) ok = hipMemcpy(h_valid.data(), valid, n, hipMemcpyDefault) == hipSuccess;
    std::vector<RowMeta> hm(n);
    std::vector<float> h_wcol(n);
    int max_cn = 0;
    for (size_t i = 0; i < n; i++) max_cn = std::max(max_cn, h_off[i + 1] - h_off[i]);
    // slot = row record + the largest packed peak record, rounded up to whole 128-byte lines
    const uint64_t slot = (sizeof(RowMeta) + asl::rec_bytes((uint64_t)max_cn) + 127) & ~127ull;
    for (size_t i = 0; ok && i < n; i++) {
      hm[i].off = h_off[i];
      hm[i].cn = h_off[i + 1] - h_off[i];
      hm[i].charge = h_chg[i];
      hm[i].pmz32 = h_valid[i] ? h_pmz32[i] : __builtin_nanf("");
      hm[i].pmz64 = h_pmz[i];
      hm[i].rec4 = (uint32_t)(((uint64_t)i * slot + sizeof(RowMeta)) >> 2);
      hm[i].pad = 0u;
      h_wcol[i] = hm[i].pmz32;
    }
    if ((uint64_t)n * slot >= (1ull << 34)) {     // rec4 is 32 bits of 4-byte units
      ok = false;
      fail(ASL_ERR_CAPACITY, "library_create: more than 16 GiB of row slots (%llu rows x %llu bytes) in one partition",
           (unsigned long long)n, (unsigned long long)slot);
    }
    L->slot = (uint32_t)slot;
    up(L->wcol, h_wcol.data(), n);
    if (ok) {
      DevBuf<RowMeta> meta_tmp;
      ok = meta_tmp.upload(hm.data(), n) == ASL_OK && L->records.reserve((size_t)n * slot + 16) == ASL_OK &&
           hipMemsetAsync(L->records.p, 0, (size_t)n * slot + 16, stream()) == hipSuccess &&
           pack_peak_records(L->offsets.p, L->mz.p, L->intensity.p, L->charge.p, meta_tmp.p, (int64_t)n,
                             L->slot, L->records.p) == ASL_OK &&
           sync_stream() == ASL_OK;
    }
  }
  if (ok && n) {
    std::vector<int32_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = (int32_t)i;
    std::stable_sort(order.begin(), order.end(),
                     [&](int32_t a, int32_t b) { return h_pmz32[(size_t)a] < h_pmz32[(size_t)b]; });
    std::vector<float> sp(n);
    for (size_t i = 0; i < n; i++) sp[i] = h_pmz32[(size_t)order[i]];
    up(L->sorted_pmz, sp.data(), n);
    up(L->sorted_row, order.data(), n);
  }
  if (ok) ok = sync_stream() == ASL_OK;
  if (!ok) {
    delete L;
    if (!*asl_last_error()) fail(ASL_ERR_HIP, "library_create: device upload failed");
    return nullptr;
  }
  L->dev.n = (int32_t)p->n;
  L->dev.n_peaks = (int64_t)np;
  L->dev.offsets = L->offsets.p;
  L->dev.mz = L->mz.p;
  L->dev.intensity = L->intensity.p;
  L->dev.charge = L->charge.p;
  L->dev.precursor_mz = L->pmz.p;
  L->dev.precursor_charge = L->pcharge.p;
  L->dev.records = L->records.p;
  return L;
}

void asl_library_free(asl_library_t *L) { delete L; }
int64_t asl_library_size(const asl_library_t *L) { return L ? L->n : 0; }

int asl_library_set_groups(asl_library_t *L, int64_t n, const int32_t *group) {
  clear_error();
  if (!L) return fail(ASL_ERR_INVALID, "library_set_groups: null library");
  if (!group) {
    ASL_TRY(ensure_device());     // (batches in flight may still read the column)
    L->group.release();
    L->has_group = false;
    return ASL_OK;
  }
  if (n != L->n)
    return fail(ASL_ERR_INVALID, "library_set_groups: %lld group ids for a library of %lld rows", (long long)n,
                (long long)L->n);
  ASL_TRY(ensure_device());
  ASL_TRY(L->group.reserve((size_t)std::max<int64_t>(n, 1)));   // (an empty library keeps a column too)
  ASL_TRY(L->group.upload(group, (size_t)n));
  ASL_TRY(sync_stream());         // a host array is the caller's again on return
  L->has_group = true;
  return ASL_OK;
}

int asl_library_set_selection(asl_library_t *L, int64_t n, const uint8_t *keep) {
  clear_error();
  if (!L) return fail(ASL_ERR_INVALID, "library_set_selection: null library");
  if (n != 0 && keep && n != L->n)
    return fail(ASL_ERR_INVALID, "library_set_selection: %lld flags for a library of %lld rows", (long long)n,
                (long long)L->n);
  ASL_TRY(ensure_device());       // (waits for the batches in flight: they read the columns about to change)
  L->has_sel = false;
  ++L->sel_gen;                   // whatever an index derived from the columns so far is out of date
  if (n == 0 || !keep) return ASL_OK;
  ASL_TRY(L->keep.reserve((size_t)n));
  ASL_TRY(L->wcol_eff.reserve((size_t)n));
  ASL_TRY(L->valid_eff.reserve((size_t)n));
  HIP_TRY(hipMemcpyAsync(L->keep.p, keep, (size_t)n, hipMemcpyDefault, stream()));
  hipLaunchKernelGGL(selection_columns_kernel, grid_2d(cdiv(n, 256)), dim3(256), 0, stream(), L->keep.p, L->wcol.p,
                     L->has_valid ? L->valid.p : nullptr, n, L->wcol_eff.p, L->valid_eff.p);
  ASL_CHECK_LAUNCH();
  ASL_TRY(sync_stream());         // a host array is the caller's again on return
  L->has_sel = true;
  return ASL_OK;
}

// CSR window candidates on the device: fills L->woff ([nq+1]) and L->cand; total -> *total.
static int window_candidates_device(asl_library *L, int nq, const double *q_pmz_dev, int charge,
                                    double tol, int mode, int64_t *total) {
  ASL_TRY(L->lo.reserve((size_t)nq));
  ASL_TRY(L->cnt.reserve((size_t)nq));
  ASL_TRY(L->woff.reserve((size_t)nq + 1));
  hipLaunchKernelGGL(window_range_kernel, dim3((unsigned)cdiv(nq, 256)), dim3(256), 0, stream(),
                     q_pmz_dev, nq, L->sorted_pmz.p, (int)L->n, charge, tol, mode, L->lo.p, L->cnt.p);
  ASL_CHECK_LAUNCH();
  std::vector<int32_t> h_cnt((size_t)nq), h_off((size_t)nq + 1, 0);
  ASL_TRY(L->cnt.download(h_cnt.data(), (size_t)nq));
  ASL_TRY(sync_stream());
  int64_t acc = 0;
  for (int q = 0; q < nq; q++) {
    h_off[(size_t)q] = (int32_t)acc;
    acc += h_cnt[(size_t)q];
    if (acc > 0x7fffffffLL)
      return fail(ASL_ERR_CAPACITY, "window: more than 2^31-1 candidate pairs in one batch; "
                                    "use a smaller batch_size for brute-force open search");
  }
  h_off[(size_t)nq] = (int32_t)acc;
  *total = acc;
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
// counted in 64 bits, are cut into tiles of at most window_pair_budget() pairs; a tile is a run of
// queries whose first and last may bring only part of their window. One tile (every batch whose
// pairs fit): the rescoring as for any list. Several: each tile's n best (n = 1: its argmax) are
// folded into the running n best (rescore_window_merge), then one pass over an n-candidate list per
// query -- its winners -- emits the peak matches. Scratch: pair scores of one tile, 12 bytes per winner.
// n_best > 0 (asl_search_batch_topn): outputs [nq, n_best]. n_best = 0 is the single-winner search: the
// same launches at n = 1 with the argmax as the selection.
static int window_search_device(asl_library *L, const DevPeaks &Q, const asl_search_params_t *P,
                                const double *intervals, int32_t *best_row, double *best_score, int32_t *n_cand,
                                int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride, int n_best = 0,
                                bool distinct = false) {
  const int nq = Q.n;
  // distinct (asl_search_batch_topn_distinct): every tile's ranks and the fold hold one row per group;
  // the final pass over the n-candidate lists, already distinct, is the plain one
  const int32_t *group = distinct ? L->group.p : nullptr;
  const int n = std::max(n_best, 1);
  const size_t nw = (size_t)nq * (size_t)n;     // winners of the batch
  std::vector<int32_t> h_lo((size_t)nq), h_cnt((size_t)nq);
  {
    ProfScope ps("filter");
    ASL_TRY(L->lo.reserve((size_t)nq));
    ASL_TRY(L->cnt.reserve((size_t)nq));
    hipLaunchKernelGGL(window_range_kernel, dim3((unsigned)cdiv(nq, 256)), dim3(256), 0, stream(),
                       window_operand(Q, P, intervals), nq, L->sorted_pmz.p, (int)L->n, P->charge, P->precursor_tol,
                       P->precursor_mode, L->lo.p, L->cnt.p);
    ASL_CHECK_LAUNCH();
    ASL_TRY(L->lo.download(h_lo.data(), (size_t)nq));
    ASL_TRY(L->cnt.download(h_cnt.data(), (size_t)nq));
    ASL_TRY(sync_stream());
  }
  std::vector<int64_t> pre((size_t)nq + 1, 0);     // exclusive prefix of the window sizes
  for (int q = 0; q < nq; q++) pre[(size_t)q + 1] = pre[(size_t)q] + h_cnt[(size_t)q];
  const int64_t total = pre[(size_t)nq];
  if (total == 0) {   // what the rescoring writes for empty lists
    HIP_TRY(hipMemsetAsync(L->status.p, 0, sizeof(int), stream()));
    if (best_row) HIP_TRY(hipMemsetAsync(best_row, 0xff, nw * 4, stream()));
    if (best_score) HIP_TRY(hipMemsetAsync(best_score, 0, nw * 8, stream()));
    if (n_cand) HIP_TRY(hipMemsetAsync(n_cand, 0, (size_t)nq * 4, stream()));
    if (pm_count) HIP_TRY(hipMemsetAsync(pm_count, 0, nw * 4, stream()));
    if (pm_pairs) HIP_TRY(hipMemsetAsync(pm_pairs, 0, nw * pm_stride * 8, stream()));
    return ASL_OK;
  }
  const int64_t B = std::min<int64_t>(window_pair_budget(), 0x7fffffffLL);
  PrecFilter rows_only;       // packed row records for the kernels, no second filtering
  library_filter(L, rows_only);
  rows_only.wcol = nullptr;
  rows_only.pass_all = true;
  WindowRows win;
  win.sorted_row = L->sorted_row.p;
  win.valid = L->valid_col();
  // every buffer before the first launch (growing one synchronises the device)
  // (the winners' pass after several tiles scores one slot per winner)
  ASL_TRY(L->pair_score.reserve((size_t)(total <= B ? total : std::max<int64_t>(B, (int64_t)nw))));
  ASL_TRY(L->rs_scratch.q_defer.reserve(RescoreScratch::defer_ints((size_t)nq)));
  ASL_TRY(L->rs_scratch.m_defer.reserve(nw));
  if (total <= B) {   // one tile: the whole batch
    std::vector<int32_t> h((size_t)2 * nq + 1);
    for (int q = 0; q <= nq; q++) h[(size_t)q] = (int32_t)pre[(size_t)q];
    for (int q = 0; q < nq; q++) h[(size_t)nq + 1 + q] = h_lo[(size_t)q];
    ASL_TRY(L->wtile.upload(h.data(), h.size()));
    win.begin = L->wtile.p + nq + 1;
    return rescore_device({.Q = Q, .L = L->dev,
                           .cand = {.offsets = L->wtile.p, .total_slots = total, .window = &win},
                           .tol = P->fragment_mz_tolerance, .tol_ppm = score_ppm(P), .allow_shift = score_shift(P),
                            .tie_by_row = 1,
                           .filter = rows_only, .n_best = n_best, .group = group,
                           .pair_score = L->pair_score.p, .best_slot = L->best_slot.p,
                           .scratch = &L->rs_scratch, .status = L->status.p,
                           .best_row = best_row, .best_score = best_score, .n_valid = n_cand,
                           .pm_count = pm_count, .pm_pairs = pm_pairs, .pm_stride = pm_stride});
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
  for (const Tile &T : tiles) {
    DevPeaks Qt = Q;            // the tile's queries: a view of the batch from query qa on
    Qt.n = T.nq;
    Qt.offsets += T.qa;
    Qt.precursor_mz += T.qa;
    if (Qt.precursor_charge) Qt.precursor_charge += T.qa;
    const int32_t *off = L->wtile.p + T.idx;
    win.begin = off + T.nq + 1;
    const CandList tile{.offsets = off, .total_slots = T.pairs, .window = &win};
    ASL_TRY(rescore_device({.Q = Qt, .L = L->dev, .cand = tile,
                            .tol = P->fragment_mz_tolerance, .tol_ppm = score_ppm(P), .allow_shift = score_shift(P),
                            .tie_by_row = 1,
                            .filter = rows_only, .n_best = n_best, .group = group,
                            .pair_score = L->pair_score.p, .best_slot = L->best_slot.p,
                            .scratch = &L->rs_scratch, .status = L->status.p, .clear_status = false,
                            .best_score = L->tile_score.p, .n_valid = L->tile_n.p, .emit_matches = false}));
    ASL_TRY(rescore_window_merge(tile, T.nq, n, L->best_slot.p, L->tile_score.p, L->tile_n.p,
                                 L->run_score.p + (size_t)T.qa * n, L->run_row.p + (size_t)T.qa * n,
                                 L->run_n.p + T.qa, group));
  }
  // the running lists once more, as an n-candidate list per query (-1: an empty rank): the same
  // order comes out again, with rows and peak matches (n_best = 0: the one winner, by the argmax)
  ASL_TRY(rescore_device({.Q = Q, .L = L->dev,
                          .cand = {.rows32 = L->run_row.p, .stride = n, .total_slots = (int64_t)nw},
                          .tol = P->fragment_mz_tolerance, .tol_ppm = score_ppm(P), .allow_shift = score_shift(P),
                            .tie_by_row = 1,
                          .filter = rows_only, .n_best = n_best,
                          .pair_score = L->pair_score.p, .best_slot = L->best_slot.p,
                          .scratch = &L->rs_scratch, .status = L->status.p, .clear_status = false,
                          .best_row = best_row, .best_score = L->tile_score.p,
                          .pm_count = pm_count, .pm_pairs = pm_pairs, .pm_stride = pm_stride}));
  return rescore_window_finish(nq, n, L->run_score.p, L->run_row.p, L->run_n.p, L->tile_score.p, best_score,
                               n_cand, L->status.p);
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
  int64_t total = 0;
  ASL_TRY(window_candidates_device(L, nq, dq.d, charge, tol, mode, &total));
  std::vector<int32_t> h_off((size_t)nq + 1), h_cand((size_t)total);
  ASL_TRY(L->woff.download(h_off.data(), (size_t)nq + 1));
  if (total) ASL_TRY(L->cand.download(h_cand.data(), (size_t)total));
  ASL_TRY(sync_stream());
  // compact invalid rows, ascending row order inside each list (spectral_library.py:451)
  std::vector<int32_t> out_off((size_t)nq + 1, 0);
  std::vector<int64_t> rows;
  rows.reserve((size_t)total);
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

// asl_rescore_knn (n_best = 0) and asl_rescore_knn_topn (outputs [nq, n_best] except n_cand)
static int rescore_knn_sync(asl_library_t *L, const asl_peaks_t *queries, const asl_search_params_t *P,
                            const int64_t *knn_I, int n_best, int32_t *best_row, double *best_score,
                            int32_t *n_cand, int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride,
                            bool distinct = false) {
  if (!L || !queries || !P || !knn_I) return fail(ASL_ERR_INVALID, "rescore_knn: null argument");
  if (distinct && !L->has_group)
    return fail(ASL_ERR_STATE, "rescore_knn_topn_distinct: the library has no group column (asl_library_set_groups)");
  const int nq = queries->n, k = P->k;
  const size_t nw = (size_t)nq * (size_t)std::max(n_best, 1);
  if (nq == 0) return ASL_OK;
  if (k <= 0) return fail(ASL_ERR_INVALID, "rescore_knn: k must be positive");
  if (pm_pairs && pm_stride <= 0) return fail(ASL_ERR_INVALID, "rescore_knn: pm_stride");
  ASL_TRY(check_window_arg(P, "rescore_knn"));
  ASL_TRY(ensure_device());
  PeaksStage Q;
  ASL_TRY(Q.init(queries));
  In<double> dwin;
  if (P->precursor_mode == ASL_TOL_INTERVAL) ASL_TRY(dwin.init(P->precursor_window, (size_t)nq * 2));
  In<int64_t> knn;
  ASL_TRY(knn.init(knn_I, (size_t)nq * k));
  Out<int32_t> o_row, o_ncand, o_cnt;
  Out<double> o_score;
  Out<uint32_t> o_pairs;
  ASL_TRY(o_row.init(best_row, nw));
  ASL_TRY(o_score.init(best_score, nw));
  ASL_TRY(o_ncand.init(n_cand, nq));
  ASL_TRY(o_cnt.init(pm_count, nw));
  ASL_TRY(o_pairs.init(pm_pairs, nw * (pm_pairs ? pm_stride : 0) * 2));
  ASL_TRY(L->best_slot.reserve(nw));
  ASL_TRY(L->status.reserve(1));
  ASL_TRY(L->pair_score.reserve((size_t)nq * k));
  // the precursor filter runs inside the rescoring kernel's compaction stage
  PrecFilter flt;
  batch_filter(L, P, dwin.d, flt);
  ASL_TRY(rescore_device({.Q = Q.dev, .L = L->dev,
                          .cand = {.rows64 = knn.d, .stride = k, .total_slots = (int64_t)nq * k},
                          .tol = P->fragment_mz_tolerance, .tol_ppm = score_ppm(P), .allow_shift = score_shift(P),
                            .tie_by_row = 1,
                          .filter = flt, .n_best = n_best, .group = distinct ? L->group.p : nullptr,
                          .pair_score = L->pair_score.p, .best_slot = L->best_slot.p,
                          .scratch = &L->rs_scratch, .status = L->status.p,
                          .best_row = o_row.d, .best_score = o_score.d, .n_valid = o_ncand.d,
                          .pm_count = o_cnt.d, .pm_pairs = o_pairs.d, .pm_stride = pm_stride}));
  ASL_TRY(o_row.finish());
  ASL_TRY(o_score.finish());
  ASL_TRY(o_ncand.finish());
  ASL_TRY(o_cnt.finish());
  ASL_TRY(o_pairs.finish());
  return rescore_check_status(L->status.p);
}

int asl_rescore_knn(asl_library_t *L, const asl_peaks_t *queries, const asl_search_params_t *P,
                    const int64_t *knn_I, int32_t *best_row, double *best_score,
                    int32_t *n_cand, int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride) {
  clear_error();
  return rescore_knn_sync(L, queries, P, knn_I, 0, best_row, best_score, n_cand, pm_count, pm_pairs, pm_stride);
}

int asl_rescore_knn_topn(asl_library_t *L, const asl_peaks_t *queries, const asl_search_params_t *P,
                         const int64_t *knn_I, int32_t n_best, int32_t *best_row, double *best_score,
                         int32_t *n_cand, int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride) {
  clear_error();
  if (n_best < 1 || n_best > ASL_MAX_BEST)
    return fail(ASL_ERR_INVALID, "rescore_knn_topn: n_best must be in [1, %d]", ASL_MAX_BEST);
  ASL_TRY(ensure_device());     // (no device: ASL_ERR_NO_DEVICE whatever else was passed)
  return rescore_knn_sync(L, queries, P, knn_I, n_best, best_row, best_score, n_cand, pm_count, pm_pairs,
                          pm_stride);
}

// The synchronous batch: asl_search_batch outside pipeline mode (n_best = 0, the single winner) and
// asl_search_batch_topn (outputs [nq, n_best] except n_cand and knn_I). The arguments are checked.
static int search_batch_sync(asl_library_t *L, asl_index_t *idx, const asl_peaks_t *queries,
                             const asl_search_params_t *P, int n_best, int32_t *best_row, double *best_score,
                             int32_t *n_cand, int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride,
                             int64_t *knn_I, bool distinct = false) {
  const int nq = queries->n;
  const size_t nw = (size_t)nq * (size_t)std::max(n_best, 1);
  ASL_TRY(check_window_arg(P, "search_batch"));
  ASL_TRY(ensure_device());
  PeaksStage Q;
  ASL_TRY(Q.init(queries));
  In<double> dwin;
  if (P->precursor_mode == ASL_TOL_INTERVAL) ASL_TRY(dwin.init(P->precursor_window, (size_t)nq * 2));
  Out<int32_t> o_row, o_ncand, o_cnt;
  Out<double> o_score;
  Out<uint32_t> o_pairs;
  Out<int64_t> o_knn;
  ASL_TRY(o_row.init(best_row, nw));
  ASL_TRY(o_score.init(best_score, nw));
  ASL_TRY(o_ncand.init(n_cand, nq));
  ASL_TRY(o_cnt.init(pm_count, nw));
  ASL_TRY(o_pairs.init(pm_pairs, nw * (pm_pairs ? pm_stride : 0) * 2));
  ASL_TRY(L->best_slot.reserve(nw));
  ASL_TRY(L->status.reserve(1));
  if (P->use_ann) {
    const int d = idx->d, k = P->k;
    if (k <= 0) return fail(ASL_ERR_INVALID, "search_batch: k must be positive");
    ASL_TRY(o_knn.init(knn_I, (size_t)nq * k));
    ASL_TRY(L->qvec.reserve((size_t)nq * d));
    ASL_TRY(L->knn.reserve((size_t)nq * k));
    ASL_TRY(L->pair_score.reserve((size_t)nq * k));
    const bool win = idx->window_scan != 0;
    if (win) ASL_TRY(index_window_prepare(idx, L->serial, L->sel_gen, L->window_col(), L->n, nq, P->nprobe));
    ASL_TRY(encode_device(Q.dev.mz, Q.dev.intensity, Q.dev.offsets, nq, P->min_bound, P->bin_size,
                          d, P->hash_seed, 1, L->qvec.p));
    // the candidates are consumed as a set (filter + best match): no final sort unless the
    // caller asked for the ordered neighbour list
    ASL_TRY(L->rows_len.reserve((size_t)nq));
    IndexSearch rq{.nq = nq, .xq = L->qvec.p, .k = k, .nprobe = P->nprobe, .I64 = o_knn.d, .I32 = L->knn.p,
                   .rows = knn_I == nullptr ? ROWS_SET : ROWS_ORDERED};
    IndexWindow w;
    IndexPostFilter pf;
    offer_library(rq, L);
    if (win) offer_window(rq, w, Q.dev, P, dwin.d, knn_I == nullptr ? L->rows_len.p : nullptr);
    else if (knn_I == nullptr && scan_postfilter_on()) offer_post_filter(rq, pf, L, Q.dev, P, dwin.d, L->rows_len.p);
    ASL_TRY(index_search_device(idx, rq));
    const bool rows_filtered = rq.rows_filtered;
    PrecFilter flt;
    batch_filter(L, P, dwin.d, flt);
    ASL_TRY(rescore_device({.Q = Q.dev, .L = L->dev,
                            .cand = {.rows32 = L->knn.p, .stride = k, .total_slots = (int64_t)nq * k,
                                     .row_counts = rows_filtered ? L->rows_len.p : nullptr},
                            .tol = P->fragment_mz_tolerance, .tol_ppm = score_ppm(P), .allow_shift = score_shift(P),
                            .tie_by_row = 1,
                            .filter = flt, .n_best = n_best, .group = distinct ? L->group.p : nullptr,
                            .pair_score = L->pair_score.p, .best_slot = L->best_slot.p,
                            .scratch = &L->rs_scratch, .status = L->status.p,
                            .best_row = o_row.d, .best_score = o_score.d, .n_valid = o_ncand.d,
                            .pm_count = o_cnt.d, .pm_pairs = o_pairs.d, .pm_stride = pm_stride}));
  } else {
    ASL_TRY(window_search_device(L, Q.dev, P, dwin.d, o_row.d, o_score.d, o_ncand.d, o_cnt.d, o_pairs.d,
                                 pm_stride, n_best, distinct));
  }
  ASL_TRY(o_row.finish());
  ASL_TRY(o_score.finish());
  ASL_TRY(o_ncand.finish());
  ASL_TRY(o_cnt.finish());
  ASL_TRY(o_pairs.finish());
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
                                  const asl_search_params_t *P, int32_t *best_row,
                                  double *best_score, int32_t *n_cand, int32_t *pm_count,
                                  uint32_t *pm_pairs, int32_t pm_stride, int64_t *knn_I) {
  Pipeline &pp = pipeline();
  struct InCall {
    Pipeline &p;
    explicit InCall(Pipeline &q) : p(q) { p.in_call = true; }
    ~InCall() { p.in_call = false; }
  } guard(pp);
  const int nq = queries->n, k = P->k, d = idx->d;
  const int nprobe = index_nprobe(idx, P->nprobe);
  PeaksStage Q;
  ASL_TRY(Q.init(queries));   // device pointers + known peak count: no copy, no wait
  const int par = pp.parity;
  // allocations first (growing a buffer synchronises the device: only ever on the first batches)
  ASL_TRY(index_prepare(idx));
  const bool win = idx->window_scan != 0;      // (the window-ordered layout of THIS library, up front)
  if (win) ASL_TRY(index_window_prepare(idx, L->serial, L->sel_gen, L->window_col(), L->n, nq, nprobe));
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
  bool rows_filtered = false;
  {
    StreamScope on_a(pp.A);
    // The buffers of this parity were last read by the scan of batch i-2: the front of batch i
    // starts when that scan ends, i.e. it runs under the RESCORING of batch i-2. Measured
    // (profiles/r02_pipeline_ab.txt): holding it back until the batch has finished, so that it
    // runs under the next scan instead, is worse -- the scan loses 1.3 ms to a 0.9 ms GEMM
    // beside it (9.88 ms per step), the rescoring only 0.6 ms (9.35 ms).
    if (pp.scan_recorded[par]) HIP_TRY(hipStreamWaitEvent(pp.A, pp.ev_scan[par], 0));
    ASL_TRY(encode_device(Q.dev.mz, Q.dev.intensity, Q.dev.offsets, nq, P->min_bound, P->bin_size,
                          d, P->hash_seed, 1, L->p_qvec[par].p));
    ASL_TRY(coarse_search(idx, L->p_qvec[par].p, nq, nprobe, L->p_cD[par].p, L->p_cI[par].p,
                                L->p_ent[par].p, L->p_cnt[par].p, &L->p_have_ent[par]));
    HIP_TRY(hipEventRecord(pp.ev_front[par], pp.A));
  }
  {
    StreamScope on_b(pp.B);
    HIP_TRY(hipStreamWaitEvent(pp.B, pp.ev_front[par], 0));
    if (pp.resc_recorded[par]) HIP_TRY(hipStreamWaitEvent(pp.B, pp.ev_resc[par], 0));
    // (the entry lists of the coarse stage, when it made them: the scan does not list the rows again)
    IndexSearch rq{.nq = nq, .xq = L->p_qvec[par].p, .k = k, .nprobe = nprobe, .I64 = knn_I, .I32 = L->p_knn[par].p,
                   .pre_D = L->p_cD[par].p, .pre_I = L->p_cI[par].p,
                   .pre_ent = L->p_have_ent[par] ? L->p_ent[par].p : nullptr,
                   .pre_cnt = L->p_have_ent[par] ? L->p_cnt[par].p : nullptr,
                   .rows = knn_I == nullptr ? ROWS_SET : ROWS_ORDERED};
    IndexWindow w;
    IndexPostFilter pf;
    offer_library(rq, L);
    if (win) offer_window(rq, w, Q.dev, P, dwin, knn_I == nullptr ? L->p_rows[par].p : nullptr);
    else if (knn_I == nullptr && scan_postfilter_on()) offer_post_filter(rq, pf, L, Q.dev, P, dwin, L->p_rows[par].p);
    ASL_TRY(index_search_device(idx, rq));
    // (window scan: set-mode rows hold in-window hits only, and their lengths)
    rows_filtered = rq.rows_filtered;
    HIP_TRY(hipEventRecord(pp.ev_scan[par], pp.B));
    pp.scan_recorded[par] = true;
  }
  {
    // measured (profiles/r02_pipeline_ab.txt): scan and rescoring are both VALU-limited, so a
    // third stream only makes them share the CUs -- the default keeps rescoring behind its scan
    hipStream_t sc = pp.streams == 3 ? pp.C : pp.B;
    StreamScope on_c(sc);
    HIP_TRY(hipStreamWaitEvent(sc, pp.ev_scan[par], 0));
    PrecFilter flt;
    batch_filter(L, P, dwin, flt);
    ASL_TRY(rescore_device({.Q = Q.dev, .L = L->dev,
                            .cand = {.rows32 = L->p_knn[par].p, .stride = k, .total_slots = (int64_t)nq * k,
                                     .row_counts = rows_filtered ? L->p_rows[par].p : nullptr},
                            .tol = P->fragment_mz_tolerance, .tol_ppm = score_ppm(P), .allow_shift = score_shift(P),
                            .tie_by_row = 1,
                            .filter = flt,
                            .pair_score = L->pair_score.p, .best_slot = L->best_slot.p,
                            .scratch = &L->rs_scratch, .status = pp.status, .clear_status = false,
                            .best_row = best_row, .best_score = best_score, .n_valid = n_cand,
                            .pm_count = pm_count, .pm_pairs = pm_pairs, .pm_stride = pm_stride}));
    HIP_TRY(hipEventRecord(pp.ev_resc[par], sc));
    pp.resc_recorded[par] = true;
  }
  return ASL_OK;
}

int asl_search_batch(asl_library_t *L, asl_index_t *idx, const asl_peaks_t *queries,
                     const asl_search_params_t *P, int32_t *best_row, double *best_score,
                     int32_t *n_cand, int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride,
                     int64_t *knn_I) {
  clear_error();
  if (!L || !queries || !P) return fail(ASL_ERR_INVALID, "search_batch: null argument");
  const int nq = queries->n;
  if (nq == 0) return ASL_OK;
  if (pm_pairs && pm_stride <= 0) return fail(ASL_ERR_INVALID, "search_batch: pm_stride");
  if (P->use_ann && !idx) return fail(ASL_ERR_INVALID, "search_batch: use_ann needs an index");
  if (P->use_ann && P->k <= 0) return fail(ASL_ERR_INVALID, "search_batch: k must be positive");
  ASL_TRY(check_window_arg(P, "search_batch"));
  {
    // pipeline mode applies to ANN batches whose arguments all live on the device (nothing to
    // stage, nothing to copy back) and whose peak count the caller supplied; anything else takes
    // the synchronous path below, after the batches in flight have drained
    Pipeline &pp = pipeline();
    auto dev_or_null = [](const void *p) { return !p || is_device_ptr(p); };
    // (an exhaustive ASL_INDEX_FLAT index has no coarse stage to overlap: synchronous path)
    if (pp.on && P->use_ann && index_nprobe(idx, P->nprobe) > 0 && queries->n_peaks > 0 &&
        peaks_on_device(queries) &&
        is_device_ptr(best_row) && is_device_ptr(best_score) && dev_or_null(n_cand) &&
        dev_or_null(pm_count) && dev_or_null(pm_pairs) && dev_or_null(knn_I)) {
      pp.in_call = true;                    // do not drain: this call joins the pipeline
      const int rc = ensure_device();
      pp.in_call = false;
      ASL_TRY(rc);
      return search_batch_pipelined(L, idx, queries, P, best_row, best_score, n_cand, pm_count,
                                    pm_pairs, pm_stride, knn_I);
    }
  }
  return search_batch_sync(L, idx, queries, P, 0, best_row, best_score, n_cand, pm_count, pm_pairs, pm_stride,
                           knn_I);
}

int asl_search_batch_topn(asl_library_t *L, asl_index_t *idx, const asl_peaks_t *queries,
                          const asl_search_params_t *P, int32_t n_best, int32_t *best_row, double *best_score,
                          int32_t *n_cand, int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride,
                          int64_t *knn_I) {
  clear_error();
  if (n_best < 1 || n_best > ASL_MAX_BEST)
    return fail(ASL_ERR_INVALID, "search_batch_topn: n_best must be in [1, %d]", ASL_MAX_BEST);
  // (no device: ASL_ERR_NO_DEVICE whatever else was passed.) Never pipelined: this waits for the
  // batches of asl_set_pipeline in flight
  ASL_TRY(ensure_device());
  if (!L || !queries || !P) return fail(ASL_ERR_INVALID, "search_batch_topn: null argument");
  if (queries->n == 0) return ASL_OK;
  if (pm_pairs && pm_stride <= 0) return fail(ASL_ERR_INVALID, "search_batch_topn: pm_stride");
  if (P->use_ann && !idx) return fail(ASL_ERR_INVALID, "search_batch_topn: use_ann needs an index");
  if (P->use_ann && P->k <= 0) return fail(ASL_ERR_INVALID, "search_batch_topn: k must be positive");
  return search_batch_sync(L, idx, queries, P, n_best, best_row, best_score, n_cand, pm_count, pm_pairs,
                           pm_stride, knn_I);
}

int asl_search_batch_topn_distinct(asl_library_t *L, asl_index_t *idx, const asl_peaks_t *queries,
                                   const asl_search_params_t *P, int32_t n_best, int32_t *best_row,
                                   double *best_score, int32_t *n_cand, int32_t *pm_count, uint32_t *pm_pairs,
                                   int32_t pm_stride, int64_t *knn_I) {
  clear_error();
  if (n_best < 1 || n_best > ASL_MAX_BEST)
    return fail(ASL_ERR_INVALID, "search_batch_topn_distinct: n_best must be in [1, %d]", ASL_MAX_BEST);
  ASL_TRY(ensure_device());     // as asl_search_batch_topn: never pipelined
  if (!L || !queries || !P) return fail(ASL_ERR_INVALID, "search_batch_topn_distinct: null argument");
  if (!L->has_group)
    return fail(ASL_ERR_STATE,
                "search_batch_topn_distinct: the library has no group column (asl_library_set_groups)");
  if (queries->n == 0) return ASL_OK;
  if (pm_pairs && pm_stride <= 0) return fail(ASL_ERR_INVALID, "search_batch_topn_distinct: pm_stride");
  if (P->use_ann && !idx) return fail(ASL_ERR_INVALID, "search_batch_topn_distinct: use_ann needs an index");
  if (P->use_ann && P->k <= 0) return fail(ASL_ERR_INVALID, "search_batch_topn_distinct: k must be positive");
  return search_batch_sync(L, idx, queries, P, n_best, best_row, best_score, n_cand, pm_count, pm_pairs,
                           pm_stride, knn_I, true);
}

int asl_rescore_knn_topn_distinct(asl_library_t *L, const asl_peaks_t *queries, const asl_search_params_t *P,
                                  const int64_t *knn_I, int32_t n_best, int32_t *best_row, double *best_score,
                                  int32_t *n_cand, int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride) {
  clear_error();
  if (n_best < 1 || n_best > ASL_MAX_BEST)
    return fail(ASL_ERR_INVALID, "rescore_knn_topn_distinct: n_best must be in [1, %d]", ASL_MAX_BEST);
  ASL_TRY(ensure_device());     // (no device: ASL_ERR_NO_DEVICE whatever else was passed)
  return rescore_knn_sync(L, queries, P, knn_I, n_best, best_row, best_score, n_cand, pm_count, pm_pairs,
                          pm_stride, true);
}

}  // extern "C"
