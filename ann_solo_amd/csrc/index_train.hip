// index_train.hip -- training of the coarse quantiser and the product quantiser.
//
// Training restates FAISS' Clustering (Lloyd iterations, assignment by the
// quantiser's metric, mean update, empty-cluster split with eps = 1/1024, at most
// 256 points per centroid; SPHERICAL -- centroids L2-renormalised every iteration -- for
// the inner-product coarse quantiser, as FAISS' IndexIVF sets cp.spherical for
// METRIC_INNER_PRODUCT) with a library-local RNG; it is deterministic and
// bit-identical to oracle/asl_oracle.c:orc_kmeans for the same seed.
#include <algorithm>
#include <cmath>

#include "index.hpp"

namespace asl {

// ------------------------------------------------------------------ RNG (same as the oracle's)
static inline uint64_t sm64(uint64_t *s) {
  uint64_t z = (*s += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
static void rand_perm(int64_t n, uint64_t seed, std::vector<int64_t> &perm) {
  uint64_t s = seed;
  perm.resize((size_t)n);
  for (int64_t i = 0; i < n; i++) perm[(size_t)i] = i;
  for (int64_t i = 0; i + 1 < n; i++) {
    int64_t j = i + (int64_t)(sm64(&s) % (uint64_t)(n - i));
    std::swap(perm[(size_t)i], perm[(size_t)j]);
  }
}

// Assign rows of x (device, [n, ld]) to the centroid with the largest inner product
// (ties: lowest index) -> assign_dev[n].
int assign_ip(asl_index *ix, const float *x, int64_t ld, int64_t n, const float *cent,
                     int k, int d, int32_t *assign_dev) {
  if (n <= 0) return ASL_OK;
  int64_t rows = (int64_t)std::max<size_t>(1, SCORE_CHUNK_BYTES / ((size_t)k * 4));
  rows = std::min<int64_t>(rows, n);
  ASL_TRY(ix->ws_scores.reserve((size_t)rows * k));
  // hashed spectra are sparse: the scores come from the sparse kernel (same bits as the GEMM,
  // 1/16 of its multiply-adds); a chunk with many dense rows is left to the GEMM by the
  // device-side gate (coarse_sparse.hip). The centroids change every iteration: transposed here.
  const bool sparse = ix->scan_variant == 0 && coarse_sparse_supported(d, k);
  if (sparse) {
    ASL_TRY(ix->kmeans_ct.reserve((size_t)k * d));
    ASL_TRY(transpose_f32(cent, k, d, ix->kmeans_ct.p));
    ASL_TRY(ix->cs_ent.reserve((size_t)rows * coarse_sparse_cap()));
    ASL_TRY(ix->cs_cnt.reserve((size_t)rows));
    ASL_TRY(ix->cs_over.reserve(1));
  }
  for (int64_t r0 = 0; r0 < n; r0 += rows) {
    const int m = (int)std::min<int64_t>(rows, n - r0);
    const int over_max = m / 64;
    if (sparse)
      ASL_TRY(coarse_sparse(x + (size_t)r0 * ld, m, d, ix->kmeans_ct.p, k, ix->cs_ent.p, ix->cs_cnt.p,
                            ix->cs_over.p, over_max, ix->ws_scores.p, k, ld));
    ASL_TRY(gemm_nt_f32(x + (size_t)r0 * ld, cent, ix->ws_scores.p, m, k, d, (int)ld, d, k,
                        sparse ? ix->cs_over.p : nullptr, over_max));
    ASL_TRY(row_argmax(ix->ws_scores.p, k, m, k, assign_dev + r0));
  }
  return ASL_OK;
}

// Lloyd k-means on the device; see file header. x: device [n, ld].
static int kmeans_device(asl_index *ix, const float *x, int64_t n, int64_t ld, int d, int k,
                         int niter, uint64_t seed, bool l2, int max_ppc, float *cent_dev) {
  if (n < 1) return fail(ASL_ERR_INVALID, "train: no training vectors");
  int64_t nt = n;
  const float *xt = x;
  int64_t ldt = ld;
  DevBuf<float> sub;
  DevBuf<int64_t> rows_dev;
  std::vector<int64_t> perm;
  if (max_ppc > 0 && n > (int64_t)k * max_ppc) {
    nt = (int64_t)k * max_ppc;
    rand_perm(n, seed, perm);
    ASL_TRY(rows_dev.upload(perm.data(), (size_t)nt));
    ASL_TRY(sub.reserve((size_t)nt * d));
    ASL_TRY(gather_rows_f32(x, ld, rows_dev.p, nt, d, sub.p, d));
    xt = sub.p;
    ldt = d;
  }
  {  // init: k distinct random training points
    rand_perm(nt, seed + 1, perm);
    std::vector<int64_t> pick((size_t)k);
    for (int c = 0; c < k; c++) pick[(size_t)c] = perm[(size_t)(c % nt)];
    ASL_TRY(rows_dev.upload(pick.data(), (size_t)k));
    ASL_TRY(gather_rows_f32(xt, ldt, rows_dev.p, k, d, cent_dev, d));
  }
  // FAISS IndexIVF: cp.spherical = true for METRIC_INNER_PRODUCT -> post_process_centroids
  // renormalises after the initialisation and after every iteration (oracle: orc_kmeans)
  const bool spherical = !l2;
  if (spherical) ASL_TRY(renorm_rows(cent_dev, k, d));
  DevBuf<int32_t> assign, order, offsets;
  ASL_TRY(assign.reserve((size_t)nt));
  ASL_TRY(order.reserve((size_t)nt));
  ASL_TRY(offsets.reserve((size_t)k + 1));
  std::vector<int32_t> h_assign((size_t)nt), h_order((size_t)nt), h_off((size_t)k + 1);
  std::vector<float> hassign((size_t)k), h_cent;
  uint64_t rng = seed + 2;
  for (int it = 0; it < niter; it++) {
    if (l2)
      ASL_TRY(l2_assign(xt, ldt, nt, d, cent_dev, k, assign.p));
    else
      ASL_TRY(assign_ip(ix, xt, ldt, nt, cent_dev, k, d, assign.p));
    ASL_TRY(assign.download(h_assign.data(), (size_t)nt));
    ASL_TRY(sync_stream());
    // counting sort by cluster (stable: ascending point order inside a cluster)
    std::fill(h_off.begin(), h_off.end(), 0);
    for (int64_t i = 0; i < nt; i++) h_off[(size_t)h_assign[(size_t)i] + 1]++;
    for (int c = 0; c < k; c++) {
      hassign[(size_t)c] = (float)h_off[(size_t)c + 1];
      h_off[(size_t)c + 1] += h_off[(size_t)c];
    }
    {
      std::vector<int32_t> cur(h_off.begin(), h_off.end() - 1);
      for (int64_t i = 0; i < nt; i++) h_order[(size_t)cur[(size_t)h_assign[(size_t)i]]++] = (int32_t)i;
    }
    ASL_TRY(order.upload(h_order.data(), (size_t)nt));
    ASL_TRY(offsets.upload(h_off.data(), (size_t)k + 1));
    ASL_TRY(centroid_update(xt, ldt, d, k, order.p, offsets.p, cent_dev));
    bool any_empty = false;
    for (int c = 0; c < k; c++) any_empty |= hassign[(size_t)c] == 0.0f;
    if (any_empty) {  // FAISS split_clusters, on the host (rare)
      h_cent.resize((size_t)k * d);
      HIP_TRY(hipMemcpyAsync(h_cent.data(), cent_dev, h_cent.size() * 4, hipMemcpyDeviceToHost, stream()));
      ASL_TRY(sync_stream());
      const float eps = 1.0f / 1024.0f;
      for (int ci = 0; ci < k; ci++) {
        if (hassign[(size_t)ci] != 0.0f) continue;
        int cj = 0;
        for (int guard = 0; guard < 64 * k + 64; guard++, cj = (cj + 1) % k) {
          float p = (hassign[(size_t)cj] - 1.0f) / (float)(nt - k);
          float r = (float)(sm64(&rng) >> 40) * (1.0f / 16777216.0f);
          if (r < p) break;
        }
        float *a = h_cent.data() + (size_t)ci * d, *b = h_cent.data() + (size_t)cj * d;
        memcpy(a, b, sizeof(float) * (size_t)d);
        for (int j = 0; j < d; j++) {
          if (j % 2 == 0) {
            a[j] *= 1 + eps;
            b[j] *= 1 - eps;
          } else {
            a[j] *= 1 - eps;
            b[j] *= 1 + eps;
          }
        }
        hassign[(size_t)ci] = floorf(hassign[(size_t)cj] / 2);
        hassign[(size_t)cj] -= hassign[(size_t)ci];
      }
      HIP_TRY(hipMemcpyAsync(cent_dev, h_cent.data(), h_cent.size() * 4, hipMemcpyHostToDevice, stream()));
      ASL_TRY(sync_stream());
    }
    if (spherical) ASL_TRY(renorm_rows(cent_dev, k, d));
  }
  ASL_TRY(sync_stream());
  return ASL_OK;
}

static int pq_train_device(asl_index *ix, const float *x, int64_t n, uint64_t seed) {
  const int d = ix->d, m = ix->pq_m, ksub = ix->ksub, dsub = ix->dsub;
  int64_t nt = n;
  const int64_t cap = (int64_t)ksub * 256;
  DevBuf<float> xt;
  DevBuf<int64_t> rows_dev;
  if (nt > cap) {
    nt = cap;
    std::vector<int64_t> perm;
    rand_perm(n, seed, perm);
    ASL_TRY(rows_dev.upload(perm.data(), (size_t)nt));
  }
  ASL_TRY(xt.reserve((size_t)nt * d));
  ASL_TRY(gather_rows_f32(x, d, nt < n ? rows_dev.p : nullptr, nt, d, xt.p, d));
  if (ix->by_residual) {      // (off: the sub-space k-means runs on the gathered rows as they are)
    DevBuf<int32_t> assign;
    ASL_TRY(assign.reserve((size_t)nt));
    ASL_TRY(assign_ip(ix, xt.p, d, nt, ix->centroids.p, ix->nlist, d, assign.p));
    ASL_TRY(residual(xt.p, assign.p, ix->centroids.p, nt, d, xt.p));
  }
  ASL_TRY(ix->codebooks.reserve((size_t)m * ksub * dsub));
  for (int mi = 0; mi < m; mi++)
    ASL_TRY(kmeans_device(ix, xt.p + (size_t)mi * dsub, nt, d, dsub, ksub, ix->niter,
                          seed + 16 + (uint64_t)mi, true, 0,
                          ix->codebooks.p + (size_t)mi * ksub * dsub));
  return ASL_OK;
}

}  // namespace asl

using namespace asl;

extern "C" {

int asl_index_train(asl_index_t *ix, int64_t n, const float *x, uint64_t seed) {
  clear_error();
  if (!ix) return fail(ASL_ERR_INVALID, "train: null index");
  ASL_TRY(ensure_device());
  if (!ivf_kind(ix->kind)) return ASL_OK;      // Flat, window-exact: nothing to train
  if (n <= 0 || !x) return fail(ASL_ERR_INVALID, "train: no data");
  if (n < ix->nlist) return fail(ASL_ERR_INVALID, "train: %lld vectors < nlist %d", (long long)n, ix->nlist);
  In<float> dx;
  ASL_TRY(dx.init(x, (size_t)n * ix->d));
  ASL_TRY(ix->centroids.reserve((size_t)ix->nlist * ix->d));
  ASL_TRY(kmeans_device(ix, dx.d, n, ix->d, ix->d, ix->nlist, ix->niter, seed, false, 256, ix->centroids.p));
  if (ix->kind == ASL_INDEX_IVFPQ) {
    if (n < ix->ksub) return fail(ASL_ERR_INVALID, "train: %lld vectors < 2^pq_bits", (long long)n);
    ASL_TRY(pq_train_device(ix, dx.d, n, seed + 7));
  }
  ASL_TRY(sync_stream());
  ix->trained = true;
  ix->cbt_ready = false;
  ix->cent_t_ready = false;
  return ASL_OK;
}

}  // extern "C"
