// index.hip -- the ANN index object behind the FAISS-shaped C ABI
// (replaces IndexFlatIP / IndexIVFFlat + train/add/search/write_index/read_index used at
// /root/reference/src/ann_solo/spectral_library.py:73-87,167-181,191,443-445,487-497;
// IVF-PQ is the north star's addition). Host orchestration only -- every flop runs
// in the kernels of gemm.hip / ivf_kernels.hip. This unit: create / free / info, the setters,
// add and reset; training, the scan layouts, search, sharding and persistence are index_*.hip.
#include <algorithm>

#include "index.hpp"

namespace asl {

template <class T>
static int dev_append(DevBuf<T> &buf, size_t old_n, const T *src_dev, size_t n) {
  if (old_n + n > buf.cap) {
    DevBuf<T> nb;
    size_t want = std::max(old_n + n, buf.cap + buf.cap / 2);
    ASL_TRY(nb.reserve(want));
    if (old_n)
      HIP_TRY(hipMemcpyAsync(nb.p, buf.p, old_n * sizeof(T), hipMemcpyDeviceToDevice, stream()));
    ASL_TRY(sync_stream());
    buf = std::move(nb);
  }
  if (n)
    HIP_TRY(hipMemcpyAsync(buf.p + old_n, src_dev, n * sizeof(T), hipMemcpyDeviceToDevice, stream()));
  return ASL_OK;
}

int index_shape_check(const char *who, int d, int nlist, int kind, int pq_m, int pq_bits) {
  if (d <= 0 || kind < ASL_INDEX_FLAT || kind > ASL_INDEX_WINFLAT) return fail(ASL_ERR_INVALID, "%s: bad d/kind", who);
  if (ivf_kind(kind) && nlist <= 0) return fail(ASL_ERR_INVALID, "%s: nlist must be positive", who);
  if (kind != ASL_INDEX_IVFPQ) return ASL_OK;
  if (pq_bits < 1 || pq_bits > 8) return fail(ASL_ERR_INVALID, "%s: pq_bits=%d outside 1..8", who, pq_bits);
  if (!(pq_m == 4 || pq_m == 8 || pq_m == 16 || pq_m == 32 || pq_m == 64))
    return fail(ASL_ERR_INVALID, "%s: pq_m=%d is not one of 4, 8, 16, 32, 64", who, pq_m);
  if (d % pq_m != 0) return fail(ASL_ERR_INVALID, "%s: pq_m=%d does not divide d=%d", who, pq_m, d);
  // the generic scan keeps a query, its ADC table and a top-k buffer in LDS: an index beyond that could be
  // trained and filled but never searched (and a code of d / pq_m < 10 240 floats always fits the 64 KB
  // rounds of the training / encoding kernels). The tiled scan has a tighter limit of its own, which
  // tiled_index() applies: past it, m = 32 at 8 bits is scanned by the generic kernel as well.
  const size_t lds = pq_scan_lds_bytes(pq_m, 1 << pq_bits, d, 1);
  if (lds > (size_t)PQ_MAX_LDS_BYTES)
    return fail(ASL_ERR_CAPACITY, "%s: d=%d, pq_m=%d, pq_bits=%d: a query, its look-up table and the smallest "
                                  "top-k buffer take %lld bytes of LDS, a workgroup has %d KB",
                who, d, pq_m, pq_bits, (long long)lds, PQ_MAX_LDS_BYTES / 1024);
  return ASL_OK;
}

}  // namespace asl

using namespace asl;

extern "C" {

asl_index_t *asl_index_create(int32_t d, int32_t nlist, int32_t kind, int32_t pq_m,
                              int32_t pq_bits) {
  clear_error();
  if (kind == ASL_INDEX_IVFPQ && pq_bits <= 0) pq_bits = 8;
  if (index_shape_check("index_create", d, nlist, kind, pq_m, pq_bits) != ASL_OK) return nullptr;
  if (ensure_device() != ASL_OK) return nullptr;
  asl_index *ix = new asl_index();
  ix->d = d;
  ix->nlist = ivf_kind(kind) ? nlist : 0;
  ix->kind = kind;
  if (kind == ASL_INDEX_IVFPQ) {
    ix->pq_m = pq_m;
    ix->pq_bits = pq_bits;
    ix->ksub = 1 << pq_bits;
    ix->dsub = d / pq_m;
  }
  ix->trained = !ivf_kind(kind);      // Flat and the window-exact index store the vectors as given
  return ix;
}

void asl_index_free(asl_index_t *ix) { delete ix; }

int asl_index_set_unordered(asl_index_t *ix, int32_t unordered) {
  clear_error();
  if (!ix) return fail(ASL_ERR_INVALID, "set_unordered: null index");
  if (unordered < 0 || unordered > 2) return fail(ASL_ERR_INVALID, "set_unordered: mode must be 0, 1 or 2");
  ix->unordered = unordered;
  return ASL_OK;
}

int asl_index_set_flat_storage(asl_index_t *ix, int32_t mode) {
  clear_error();
  if (!ix || (ix->kind != ASL_INDEX_IVFFLAT && ix->kind != ASL_INDEX_WINFLAT))
    return fail(ASL_ERR_INVALID, "set_flat_storage: an IVF-Flat or window-exact index is required");
  if (mode != ASL_FLAT_FX22 && mode != ASL_FLAT_F32) return fail(ASL_ERR_INVALID, "set_flat_storage: ASL_FLAT_FX22 or ASL_FLAT_F32");
  if (ix->ntotal > 0 && mode != ix->flat_storage)
    return fail(ASL_ERR_STATE, "set_flat_storage: set before add() (stored components are rounded as they arrive)");
  ix->flat_storage = mode;
  ix->agreed_val = -1;      // what asl_index_supports_keys answers may change: the ranks agree again
  return ASL_OK;
}

int asl_index_get_flat_storage(const asl_index_t *ix) { return ix ? ix->flat_storage : ASL_FLAT_F32; }

int asl_index_set_scan_variant(asl_index_t *ix, int32_t variant) {
  clear_error();
  if (!ix || variant < 0 || variant > 2)
    return fail(ASL_ERR_INVALID, "set_scan_variant: 0 (layout-specific scan), 1 (generic kernels) or 2 (as 0, the tiled "
                                 "IVF-PQ scan reading its tile-major codes only)");
  // 2: every layout-specific kernel as under 0, but no scan of the sub-quantiser-major copy (both in one process)
  ix->scan_variant = variant == 1 ? 1 : 0;
  ix->scan_mmajor = variant == 0;
  ix->agreed_val = -1;      // asl_index_supports_keys depends on the variant: the ranks agree again
  return ASL_OK;
}

int asl_index_codes_mmajor(const asl_index_t *ix) { return ix && ix->mm_ready && !ix->lists_dirty ? 1 : 0; }

int asl_index_set_window_scan(asl_index_t *ix, int32_t on) {
  clear_error();
  if (!ix) return fail(ASL_ERR_INVALID, "set_window_scan: null index");
  if (on != 0 && on != 1) return fail(ASL_ERR_INVALID, "set_window_scan: 0 (post-filter) or 1 (window scan)");
  if (ix->kind == ASL_INDEX_WINFLAT) return ASL_OK;      // the window is always the scan's: there is no other mode
  if (on)
    if (const char *why = window_unsupported(ix)) return fail(ASL_ERR_STATE, "%s", why);
  ix->window_scan = on;
  return ASL_OK;
}

int asl_index_set_niter(asl_index_t *ix, int32_t niter) {
  if (!ix || niter < 0) return fail(ASL_ERR_INVALID, "set_niter");
  ix->niter = niter;
  return ASL_OK;
}

int asl_index_set_by_residual(asl_index_t *ix, int32_t on) {
  clear_error();
  if (!ix) return fail(ASL_ERR_INVALID, "set_by_residual: null index");
  if (on != 0 && on != 1) return fail(ASL_ERR_INVALID, "set_by_residual: 0 (raw vectors) or 1 (residuals)");
  if (ix->kind != ASL_INDEX_IVFPQ) return fail(ASL_ERR_STATE, "set_by_residual: an IVF-PQ index is required");
  if (ix->trained)
    return fail(ASL_ERR_STATE, "set_by_residual: set before train() / set_trained() (the codebooks belong to the "
                               "mode they were trained or installed in)");
  ix->by_residual = on != 0;
  return ASL_OK;
}

int asl_index_get_by_residual(const asl_index_t *ix) { return ix && ix->kind == ASL_INDEX_IVFPQ ? ix->by_residual : 1; }

int asl_index_set_trained(asl_index_t *ix, const float *centroids, const float *codebooks) {
  clear_error();
  if (!ix) return fail(ASL_ERR_INVALID, "set_trained: null index");
  if (ix->kind == ASL_INDEX_WINFLAT)
    return fail(ASL_ERR_STATE, "set_trained: a window-exact index has no quantiser to install");
  ASL_TRY(ensure_device());
  if (ix->kind != ASL_INDEX_FLAT) {
    if (!centroids) return fail(ASL_ERR_INVALID, "set_trained: centroids required");
    ASL_TRY(ix->centroids.upload(centroids, (size_t)ix->nlist * ix->d));
  }
  if (ix->kind == ASL_INDEX_IVFPQ) {
    if (!codebooks) return fail(ASL_ERR_INVALID, "set_trained: codebooks required");
    ASL_TRY(ix->codebooks.upload(codebooks, (size_t)ix->pq_m * ix->ksub * ix->dsub));
  }
  ASL_TRY(sync_stream());
  ix->trained = true;
  ix->cbt_ready = false;
  ix->cent_t_ready = false;
  return ASL_OK;
}

static int index_add_impl(asl_index_t *ix, int64_t n, const float *x, const int32_t *lists);

int asl_index_add(asl_index_t *ix, int64_t n, const float *x) { return index_add_impl(ix, n, x, nullptr); }

// add() with the inverted list of every vector supplied by the caller instead of computed by the
// coarse quantiser: what re-creating an index from its stored inverted lists needs (an imported
// FAISS file keeps FAISS' own assignments, bit for bit whatever its BLAS rounded).
int asl_index_add_preassigned(asl_index_t *ix, int64_t n, const float *x, const int32_t *lists) {
  if (!lists) return fail(ASL_ERR_INVALID, "add_preassigned: null list assignment");
  if (ix && ix->kind == ASL_INDEX_WINFLAT)
    return fail(ASL_ERR_STATE, "add_preassigned: a window-exact index has one list, nothing to assign (use add)");
  if (!ix || ix->kind == ASL_INDEX_FLAT) return fail(ASL_ERR_INVALID, "add_preassigned: an IVF index is required");
  return index_add_impl(ix, n, x, lists);
}

static int index_add_impl(asl_index_t *ix, int64_t n, const float *x, const int32_t *lists) {
  clear_error();
  if (!ix) return fail(ASL_ERR_INVALID, "add: null index");
  if (!ix->trained) return fail(ASL_ERR_STATE, "add: index is not trained");
  if (ix->shard_world > 1) return fail(ASL_ERR_STATE, "add: index is already sharded");
  if (n <= 0) return ASL_OK;
  if (!x) return fail(ASL_ERR_INVALID, "add: null data");
  if (ix->ntotal + n > 0x7fffffffLL) return fail(ASL_ERR_CAPACITY, "add: more than 2^31-1 vectors");
  ASL_TRY(ensure_device());
  In<float> dx;
  ASL_TRY(dx.init(x, (size_t)n * ix->d));
  if (ivf_kind(ix->kind)) {
    ASL_TRY(ix->ws_assign.reserve((size_t)n));
    if (lists) {
      std::vector<int32_t> h((size_t)n);
      HIP_TRY(hipMemcpy(h.data(), lists, (size_t)n * 4, hipMemcpyDefault));
      for (int64_t i = 0; i < n; i++)
        if (h[(size_t)i] < 0 || h[(size_t)i] >= ix->nlist)
          return fail(ASL_ERR_INVALID, "add_preassigned: list %d of vector %lld outside 0..%d", h[(size_t)i],
                      (long long)i, ix->nlist - 1);
      ASL_TRY(ix->ws_assign.upload(h.data(), (size_t)n));
      ASL_TRY(sync_stream());
    } else {
      ASL_TRY(assign_ip(ix, dx.d, ix->d, n, ix->centroids.p, ix->nlist, ix->d, ix->ws_assign.p));
    }
    ASL_TRY(dev_append(ix->vlist, (size_t)ix->n_store, ix->ws_assign.p, (size_t)n));
  }
  if (ix->kind == ASL_INDEX_IVFPQ) {
    DevBuf<uint8_t> codes;
    ASL_TRY(codes.reserve((size_t)n * ix->pq_m));
    ASL_TRY(pq_encode(dx.d, ix->ws_assign.p, ix->centroids.p, ix->codebooks.p, n, ix->d, ix->pq_m,
                      ix->ksub, ix->dsub, codes.p, ix->by_residual));
    ASL_TRY(dev_append(ix->codes_add, (size_t)ix->n_store * ix->pq_m, codes.p, (size_t)n * ix->pq_m));
    ASL_TRY(sync_stream());
    if (ix->refine_rows) {
      const size_t S = (size_t)refine_stride(), have = (size_t)ix->r_n, want = have + (size_t)n;
      auto grow = [&](auto &buf, size_t per) -> int {
        using T = typename std::remove_reference<decltype(*buf.p)>::type;
        if (want * per <= buf.cap) return ASL_OK;
        DevBuf<T> nb;
        ASL_TRY(nb.reserve(std::max(want * per, buf.cap + buf.cap / 2)));
        if (have) HIP_TRY(hipMemcpyAsync(nb.p, buf.p, have * per * sizeof(T), hipMemcpyDeviceToDevice, stream()));
        ASL_TRY(sync_stream());
        buf = std::move(nb);
        return ASL_OK;
      };
      ASL_TRY(grow(ix->r_dim, S));
      ASL_TRY(grow(ix->r_val, S));
      ASL_TRY(grow(ix->r_cnt, 1));
      DevBuf<int> st;
      ASL_TRY(st.reserve(1));
      HIP_TRY(hipMemsetAsync(st.p, 0, sizeof(int), stream()));
      ASL_TRY(refine_append_rows(dx.d, n, ix->d, ix->r_n, ix->r_dim.p, ix->r_val.p, ix->r_cnt.p, st.p));
      int h = 0;
      HIP_TRY(hipMemcpyAsync(&h, st.p, sizeof(int), hipMemcpyDeviceToHost, stream()));
      ASL_TRY(sync_stream());
      if (h) ix->refine_bad = true;
      ix->r_n += n;
    }
  } else {
    ASL_TRY(dev_append(ix->vecs, (size_t)ix->n_store * ix->d, dx.d, (size_t)n * ix->d));
    if ((ix->kind == ASL_INDEX_IVFFLAT || ix->kind == ASL_INDEX_WINFLAT) &&
        ix->flat_storage == ASL_FLAT_FX22)                                       // stored components: 22-bit fixed point
      ASL_TRY(quantize_fx22(ix->vecs.p + (size_t)ix->n_store * ix->d, n * ix->d));
  }
  ASL_TRY(sync_stream());
  ix->n_store += n;
  ix->ntotal += n;
  ix->lists_dirty = true;
  ix->agreed_val = -1;
  return ASL_OK;
}

int asl_index_set_refine(asl_index_t *ix, int32_t kprime) {
  clear_error();
  if (!ix) return fail(ASL_ERR_INVALID, "set_refine: null index");
  if (ix->kind == ASL_INDEX_WINFLAT)
    return fail(ASL_ERR_STATE, "set_refine: a window-exact index scores exactly already, there is nothing to re-rank");
  if (ix->kind != ASL_INDEX_IVFPQ) return fail(ASL_ERR_INVALID, "set_refine: an IVF-PQ index is required");
  if (kprime < 0 || kprime > TK_MAX_K) return fail(ASL_ERR_INVALID, "set_refine: k' must be in 0..%d", TK_MAX_K);
  if (kprime > 0 && !ix->refine_rows) {
    if (ix->ntotal > 0)
      return fail(ASL_ERR_STATE, "set_refine: enable before add() (the exact rows are stored as vectors arrive)");
    ix->refine_rows = true;
  }
  ix->refine_k = kprime;
  ix->agreed_val = -1;
  return ASL_OK;
}

int asl_index_get_refine(const asl_index_t *ix) { return ix ? ix->refine_k : 0; }

int asl_index_reset(asl_index_t *ix) {
  if (!ix) return fail(ASL_ERR_INVALID, "reset: null index");
  ix->vecs.release();
  ix->vlist.release();
  ix->vids.release();
  ix->codes_add.release();
  ix->codes.release();
  ix->ids.release();
  ix->ws_scores.release();
  ix->ntotal = 0;
  ix->n_store = 0;
  ix->r_n = 0;
  ix->refine_bad = false;
  ix->has_vids = false;
  ix->shard_rank = 0;
  ix->shard_world = 1;
  ix->lists_dirty = true;
  return ASL_OK;
}

int64_t asl_index_ntotal(const asl_index_t *ix) { return ix ? ix->ntotal : 0; }
int asl_index_is_trained(const asl_index_t *ix) { return ix && ix->trained; }

int asl_index_info(const asl_index_t *ix, asl_index_info_t *info) {
  if (!ix || !info) return fail(ASL_ERR_INVALID, "info: null");
  info->d = ix->d;
  info->nlist = ix->nlist;
  info->kind = ix->kind;
  info->pq_m = ix->pq_m;
  info->pq_ksub = ix->ksub;
  info->pq_dsub = ix->dsub;
  info->ntotal = ix->ntotal;
  info->nlocal = ix->n_store;
  info->trained = ix->trained;
  info->shard_rank = ix->shard_rank;
  info->shard_world = ix->shard_world;
  return ASL_OK;
}

int asl_index_get_centroids(const asl_index_t *ix, float *out) {
  clear_error();
  if (!ix || !out || !ivf_kind(ix->kind) || !ix->trained)
    return fail(ASL_ERR_STATE, "get_centroids: not available");
  HIP_TRY(hipMemcpyAsync(out, ix->centroids.p, (size_t)ix->nlist * ix->d * 4, hipMemcpyDefault, stream()));
  return sync_stream();
}

int asl_index_get_codebooks(const asl_index_t *ix, float *out) {
  clear_error();
  if (!ix || !out || ix->kind != ASL_INDEX_IVFPQ || !ix->trained)
    return fail(ASL_ERR_STATE, "get_codebooks: not available");
  HIP_TRY(hipMemcpyAsync(out, ix->codebooks.p, (size_t)ix->pq_m * ix->ksub * ix->dsub * 4, hipMemcpyDefault, stream()));
  return sync_stream();
}

}  // extern "C"
