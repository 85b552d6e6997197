// index_rank.hip -- asl_index_rank: the host driver of the rank scans (rank_scan.hip). Per call: the
// id -> storage slot map and, with a window, the key column by slot (both temporary: nothing is kept on
// the handle), the probes of the coarse quantiser (nprobe > 0) or the coarse term of every list (IVF-PQ,
// exhaustive), then per chunk of queries the target launch, the count and the outputs.
#include <algorithm>

#include "index.hpp"

namespace asl {

// what the index must be for a rank query; nullptr when it is, else why not
static const char *rank_unsupported(const asl_index *ix) {
  if (ix->kind == ASL_INDEX_WINFLAT) return "rank: not served by a window-exact index (IVF-Flat postings or tiled IVF-PQ)";
  if (ix->kind == ASL_INDEX_FLAT) return "rank: needs an IVF index (IVF-Flat postings or tiled IVF-PQ), not Flat";
  if (ix->shard_world > 1 || ix->has_vids) return "rank: does not run on a sharded index";
  if (ix->scan_variant != 0) return "rank: needs the layout-specific scan (scan_variant 0), not the generic kernels";
  if (ix->kind == ASL_INDEX_IVFPQ && !tiled_index(ix))
    return "rank: needs the tiled IVF-PQ scan (m = 32, 8 bits, d <= 1020), not a generic PQ shape";
  return nullptr;
}

static int index_rank_device(asl_index *ix, int nq, const float *xq, const int64_t *target, int nprobe,
                             const float *key, const double *q_pmz, int charge, double tol, int mode, int64_t *rank,
                             float *score, int64_t *scope) {
  const bool pq = ix->kind == ASL_INDEX_IVFPQ;
  const int nlist = ix->nlist, d = ix->d;
  const int32_t *slot_ids = pq ? ix->ids_tiled.p : ix->ids.p;
  const int64_t nslots = pq ? ix->n_tile_slots : ix->n_store;
  DevBuf<int32_t> inv;
  DevBuf<float> key_slot, tscore, coarse_all;
  DevBuf<unsigned long long> tkey, counts;
  ASL_TRY(inv.reserve((size_t)std::max<int64_t>(ix->ntotal, 1)));
  ASL_TRY(rank_invert(slot_ids, nslots, ix->ntotal, inv.p));
  RankWindow win;
  if (key) {
    ASL_TRY(key_slot.reserve((size_t)std::max<int64_t>(nslots, 1)));
    ASL_TRY(rank_slot_keys(slot_ids, nslots, key, ix->ntotal, key_slot.p));
    win.key_slot = key_slot.p;
    win.tol = tol, win.mode = mode, win.charge = charge;
  }
  if (pq) ASL_TRY(index_codebooks_transposed(ix));
  if (nprobe > 0) ASL_TRY(coarse_search(ix, xq, nq, nprobe, nullptr, nullptr, nullptr, nullptr, nullptr));
  // the coarse terms of an exhaustive IVF-PQ scope are [rows, nlist]: the queries go in chunks of rows
  int rows = nq;
  if (pq && nprobe == 0) {
    rows = (int)std::min<int64_t>(nq, std::max<int64_t>(1, (int64_t)(SCORE_CHUNK_BYTES / ((size_t)nlist * 4))));
    if (ix->by_residual) ASL_TRY(coarse_all.reserve((size_t)rows * nlist));
  }
  // by_residual off: zeros for the probes' scores and for the coarse term of every list (index_zero_coarse)
  const float *zeros = nullptr;
  if (pq && !ix->by_residual)
    ASL_TRY(index_zero_coarse(ix, nprobe ? (size_t)nq * nprobe : (size_t)rows * nlist, &zeros));
  ASL_TRY(tkey.reserve((size_t)nq));
  ASL_TRY(tscore.reserve((size_t)nq));
  ASL_TRY(counts.reserve((size_t)nq * 2));
  HIP_TRY(hipMemsetAsync(counts.p, 0, (size_t)nq * 16, stream()));
  for (int r0 = 0; r0 < nq; r0 += rows) {
    const int m = std::min(rows, nq - r0);
    const float *x = xq + (size_t)r0 * d;
    const float *cD = !nprobe ? nullptr : zeros ? zeros : ix->coarse_D.p + (size_t)r0 * nprobe;
    const int32_t *cI = nprobe ? ix->coarse_I.p + (size_t)r0 * nprobe : nullptr;
    win.q_pmz = key ? q_pmz + (size_t)r0 * (mode == ASL_TOL_INTERVAL ? 2 : 1) : nullptr;
    if (pq) {
      if (nprobe == 0 && !zeros) ASL_TRY(coarse_scores_all(ix, x, m, coarse_all.p));
      ASL_TRY(rank_pq(x, m, d, ix->codebooks_t.p, ix->dsub, nlist, ix->ntotal, cD, cI, nprobe,
                      zeros ? zeros : coarse_all.p,
                      ix->list_offsets.p, ix->tile_offsets.p, ix->codes_tiled.p, ix->ids_tiled.p, target + r0, inv.p,
                      win, tkey.p + r0, tscore.p + r0, counts.p + (size_t)r0 * 2, scope != nullptr));
    } else {
      ASL_TRY(rank_flat(postings_view(ix), x, m, ix->ntotal, cI, nprobe, target + r0, inv.p, win, tkey.p + r0,
                        tscore.p + r0, counts.p + (size_t)r0 * 2, scope != nullptr));
    }
  }
  ASL_TRY(rank_finish(tkey.p, tscore.p, counts.p, nq, rank, score, scope));
  return sync_stream();      // the temporaries above are freed on return
}

}  // namespace asl

using namespace asl;

extern "C" {

int asl_index_rank(asl_index_t *ix, int32_t nq, const float *xq, const int64_t *target, int32_t nprobe,
                   const float *key, const double *q_pmz, int32_t charge, double tol, int32_t mode, int64_t *rank,
                   float *score, int64_t *scope) {
  clear_error();
  ASL_TRY(ensure_device());
  if (!ix) return fail(ASL_ERR_INVALID, "rank: null index");
  if (nq <= 0) return ASL_OK;
  if (!xq || !target || !rank) return fail(ASL_ERR_INVALID, "rank: null xq / target / rank");
  if (nprobe < 0) return fail(ASL_ERR_INVALID, "rank: nprobe must be 0 (every list) or positive");
  if (key && !q_pmz) return fail(ASL_ERR_INVALID, "rank: a window key needs the queries' precursor m/z");
  if (key && mode != ASL_TOL_DA && mode != ASL_TOL_PPM && mode != ASL_TOL_INTERVAL)
    return fail(ASL_ERR_INVALID, "rank: mode must be Da, ppm or interval");
  if (const char *why = rank_unsupported(ix)) return fail(ASL_ERR_STATE, "%s", why);
  if (!ix->trained) return fail(ASL_ERR_STATE, "rank: index is not trained");
  ASL_TRY(build_lists(ix));
  if (ix->kind == ASL_INDEX_IVFFLAT) {
    // rank_flat_block (rank_scan.hip) reads float postings only. A fixed-point index (layout 2; its view carries
    // tab8, no tab32) is refused here and never reaches it. Ranking one is open: the walk would need the FX
    // decoding of flat_inv_scan_kernel (line counts summed into starts, 2^-22 folded into the query values).
    if (ix->n_store > 0 && ix->has_inv && ix->inv_layout == 2)
      return fail(ASL_ERR_STATE, "rank: fixed-point postings (ASL_FLAT_FX22) are not supported, only float postings");
    if (ix->n_store > 0 && !(ix->has_inv && ix->inv_layout == 1))
      return fail(ASL_ERR_STATE, "rank: the IVF-Flat index holds dense rows, no postings");
  } else if (!ix->has_tiles) {
    return fail(ASL_ERR_STATE, "rank: the IVF-PQ index has no tiled layout");
  }
  if (nprobe > 0) {
    nprobe = std::min(nprobe, ix->nlist);
    if (nprobe > TK_MAX_K) return fail(ASL_ERR_CAPACITY, "rank: nprobe=%d > %d (0 ranks over every list)", nprobe, TK_MAX_K);
  }
  In<float> dq, dkey;
  In<int64_t> dt;
  In<double> dp;
  Out<int64_t> drank, dscope;
  Out<float> dscore;
  ASL_TRY(dq.init(xq, (size_t)nq * ix->d));
  ASL_TRY(dt.init(target, (size_t)nq));
  if (key) {
    ASL_TRY(dkey.init(key, (size_t)ix->ntotal));
    ASL_TRY(dp.init(q_pmz, (size_t)nq * (mode == ASL_TOL_INTERVAL ? 2 : 1)));
  }
  ASL_TRY(drank.init(rank, (size_t)nq));
  ASL_TRY(dscore.init(score, (size_t)nq));
  ASL_TRY(dscope.init(scope, (size_t)nq));
  if (ix->n_store == 0) {        // an empty index: nothing is in scope
    HIP_TRY(hipMemsetAsync(drank.d, 0xff, (size_t)nq * 8, stream()));
    if (dscore.d) HIP_TRY(hipMemsetAsync(dscore.d, 0xff, (size_t)nq * 4, stream()));
    if (dscope.d) HIP_TRY(hipMemsetAsync(dscope.d, 0, (size_t)nq * 8, stream()));
  } else {
    ASL_TRY(index_rank_device(ix, nq, dq.d, dt.d, nprobe, key && ix->ntotal ? dkey.d : nullptr, dp.d, charge, tol, mode,
                              drank.d, dscore.d, dscope.d));
  }
  ASL_TRY(drank.finish());
  ASL_TRY(dscore.finish());
  ASL_TRY(dscope.finish());
  return sync_stream();
}

}  // extern "C"
