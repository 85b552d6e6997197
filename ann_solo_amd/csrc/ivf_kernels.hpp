// ivf_kernels.hpp -- host-callable wrappers of the IVF device kernels (all pointers
// are device pointers; everything is enqueued on asl::stream()). One block per translation unit.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace asl {

struct ScanPostFilter;            // common.hpp
struct ScanRanges;
struct FlatPostings;              // flat_postings.hpp

constexpr int TK_NT = 256;        // threads per top-k workgroup
constexpr int TK_MAX_K = 2048;    // largest k / nprobe the LDS top-k supports
constexpr int TK_MAX_K_PASSES = 16384;   // largest k of a search: beyond TK_MAX_K in bounded passes of the generic kernels
constexpr int PQ_MAX_DSUB = 32;   // register fast path of the PQ L2 kernels
constexpr int PQ_MAX_LDS_BYTES = 160 * 1024;   // a workgroup's LDS: what pq_scan_lds_bytes may come to

// ---- gemm.hip
// gate != nullptr: the kernel returns at once when *gate <= gate_max (device-side choice
// between this GEMM and the sparse coarse quantiser)
int gemm_nt_f32(const float *A, const float *B, float *C, int M, int N, int K, int lda,
                int ldb, int ldc, const int *gate = nullptr, int gate_max = 0);

// ---- coarse_sparse.hip: coarse quantiser for sparse queries
bool coarse_sparse_supported(int d, int nlist);
int coarse_sparse_cap();
// ent[q][64] = (dimension * 128, value bits) of the non-zero components of row q, ascending;
// cnt[q] = their number or -1 - count beyond 64; *n_over += rows beyond 64
int list_nonzeros(const float *xq, int nq, int d, int64_t ldq, uint2 *ent, int32_t *cnt, int *n_over);
int transpose_f32(const float *in, int rows, int cols, float *out);
int coarse_sparse(const float *xq, int nq, int d, const float *Ct, int nlist, uint2 *ent,
                  int32_t *cnt, int *n_over, int over_max, float *scores, int ld, int64_t ldq = 0,
                  bool lists_ready = false);

// ---- ivf_kernels.hip: top-k and merges, gathers, the ADC table and the generic IVF-PQ scan
int row_topk(const float *scores, int64_t ld, int rows, int n, int k, const int32_t *ids,
             int32_t id_base, const int32_t *vlist, const uint32_t *bitmap, int bitmap_words,
             float *D, int64_t *I64, int32_t *I32, int64_t out_ld,
             // bounded pass (k beyond TK_MAX_K in passes of <= TK_MAX_K): only keys below upper_in[row]
             // take part; upper_out[row] = the smallest key written by a full row, else 0
             const uint64_t *upper_in = nullptr, uint64_t *upper_out = nullptr);
int topk_merge(const float *Ds, const int64_t *Is, int S, int nq, int k, float *D, int64_t *I);
int topk_merge_keys(const int64_t *Ks, int S, int nq, int k, float *D, int64_t *I, int unordered);
int probe_bitmap(const int32_t *coarse_I, int nq, int nprobe, uint32_t *bitmap, int words);
int gather_rows_f32(const float *src, int64_t ld_src, const int64_t *rows, int64_t n, int d,
                    float *dst, int64_t ld_dst);
int gather_rows_u8(const uint8_t *src, const int32_t *rows, int64_t n, int m, uint8_t *dst);
int pq_lut(const float *xq, int nq, int d, const float *codebooks, int m, int ksub, int dsub,
           float *lut_out);
int pq_scan(const float *xq, int nq, int d, const float *codebooks, int m, int ksub, int dsub,
            const float *coarse_D, const int32_t *coarse_I, int nprobe,
            const int32_t *list_offsets, const int32_t *ids, const uint8_t *codes, int k,
            float *D, int64_t *I64, int32_t *I32, int64_t out_ld = 0,
            const uint64_t *upper_in = nullptr, uint64_t *upper_out = nullptr);
// LDS of a pq_scan workgroup: the top-k buffer of k, the ADC table and the query
size_t pq_scan_lds_bytes(int m, int ksub, int d, int k);
int scanned_count(const int32_t *coarse_I, int64_t n, const int32_t *list_offsets,
                  unsigned long long *out_dev);

// ---- quantizer.hip: what builds an index (k-means, list assignment, the PQ codec)
int row_argmax(const float *scores, int64_t ld, int rows, int n, int32_t *out);
int centroid_update(const float *x, int64_t ld, int d, int k, const int32_t *order,
                    const int32_t *offsets, float *centroids);
int renorm_rows(float *c, int k, int d);
int l2_assign(const float *x, int64_t ld, int64_t n, int dsub, const float *cb, int ksub,
              int32_t *assign);
int residual(const float *x, const int32_t *assign, const float *centroids, int64_t n, int d,
             float *dst);
int pq_encode(const float *x, const int32_t *assign, const float *centroids,
              const float *codebooks, int64_t n, int d, int m, int ksub, int dsub,
              uint8_t *codes, bool by_residual = true);   // false: x itself is encoded (assign / centroids unread)

// ---- pq_scan_v3.hip: tiled IVF-PQ scan, m = 32 sub-quantisers of 8 bits
bool pq_scan_tiled_supported(int m, int ksub, int k, int nprobe);
int pq_scan_v3(const float *xq, int nq, int d, const float *codebooks, int dsub,
               const float *coarse_D, const int32_t *coarse_I, int nprobe,
               const int32_t *list_offsets, const int32_t *tile_offsets,
               const uint8_t *codes_tiled, const int32_t *ids_tiled, int k, float *D,
               int64_t *I64, int32_t *I32, int set_mode, const uint2 *ent = nullptr,
               const int32_t *ent_cnt = nullptr,    // ent / ent_cnt: list_nonzeros (64 entries per query)
               const int *gate = nullptr,           // device-side row count: workgroups past it return at once
               const ScanPostFilter *post = nullptr,   // (common.hpp) set-mode int32 rows, k <= 1280 only
               const ScanRanges *ranges = nullptr,   // (common.hpp) window scan of the window-ordered layout, k <= 1280
               const unsigned long long *sel = nullptr,    // selector: a word per tile of the layout scanned, k <= 1280
               const uint8_t *codes_mm = nullptr,          // the sub-quantiser-major copy of codes_tiled and its plane
               uint32_t mm_plane = 0);                     // size (mmajor_codes): plain requests are scanned from it
// sub-quantiser-major copy of tile-major codes: plane m (plane bytes, a multiple of 128 and >= ntiles * 64) holds
// sub-quantiser m's 64 bytes of every tile in tile order; codes_mm: 32 * plane bytes
int mmajor_codes(const uint8_t *codes_tiled, int64_t ntiles, uint32_t plane, uint8_t *codes_mm);
// selector words of a tiled layout: bit v of words[tile] = keep[slot_ids[tile * 64 + v]] (id -1: unselected)
int tile_selector(const int32_t *slot_ids, int64_t ntiles, const uint8_t *keep, int64_t n,
                  unsigned long long *words);
// [lo, hi) of the in-window run of every (query, probe) in the window-ordered layout
int window_ranges(const double *q_pmz, int nq, const int32_t *coarse_I, int nprobe,
                  const int32_t *list_offsets, const int32_t *tile_offsets, const float *wkey, int charge,
                  double tol, int mode, int2 *ranges, unsigned long long *acc);
int tile_codes(const uint8_t *codes, const int32_t *ids, const int32_t *dst_slot, int64_t n,
               int64_t ntiles, uint8_t *codes_tiled, int32_t *ids_tiled);

// ---- flat_scan.hip, flat_build.hip, flat_tools.hip (the IVF-Flat postings): flat_postings.hpp

// ---- refine.hip: exact re-rank of a short-list against sparse stored rows
int refine_stride();
int refine_append_rows(const float *x, int64_t n, int d, int64_t row0, uint16_t *r_dim, float *r_val,
                       uint8_t *r_cnt, int *status);
int refine_topk(const float *xq, int nq, int d, const int32_t *I_in, const int64_t *I_in64, int kp,
                const uint16_t *r_dim, const float *r_val, const uint8_t *r_cnt, int64_t n_rows, int k, float *D,
                int64_t *I64, int32_t *I32);

// ---- exchange.hip: the exact top-k exchange of a sharded search
int keys_split(const unsigned long long *K, int64_t nrows, int k, int kp, unsigned long long *head,
               int32_t *floor_out, unsigned long long *rowmin_out = nullptr);
int keys_merge(const unsigned long long *heads, int S, int nq, int kp, int k, const unsigned long long *xbuf,
               long long xcap, const unsigned long long *prev_keys, int32_t *need,
               unsigned long long *out_keys, unsigned long long *bounds, int64_t *I, float *D, int sorted);
int keys_extras(const unsigned long long *K, const int32_t *floor_in, int64_t nrows, int k,
                const unsigned long long *bounds, int nq, long long xcap, unsigned long long *xbuf,
                unsigned int *cursor, int32_t *overflow, const int32_t *rmap = nullptr,
                const unsigned long long *K3 = nullptr, int k3 = 0);
int rescan_list(const unsigned long long *bounds, const unsigned long long *rowmin, int64_t nrows, int R,
                int64_t *rowlist, int32_t *rmap, int *count, int32_t *overflow);

// ---- rank_scan.hip: rank of a target vector in the scans' (score desc, id asc) order (asl_index_rank)
struct RankWindow {                 // the scope's precursor window; key_slot == nullptr: none
  const float *key_slot = nullptr;  // the key column by storage slot (rank_slot_keys)
  const double *q_pmz = nullptr;    // per query
  double tol = 0.0;
  int mode = 0, charge = 0;
};
int rank_invert(const int32_t *slot_ids, int64_t nslots, int64_t ntotal, int32_t *inv);
int rank_slot_keys(const int32_t *slot_ids, int64_t nslots, const float *key, int64_t ntotal, float *key_slot);
// tkey [nq] (0: the target is not in scope) / tscore [nq] are written, counts [nq][2] (rank, scope) added to
int rank_flat(const FlatPostings &P, const float *xq, int nq, int64_t ntotal, const int32_t *coarse_I, int nprobe,
              const int64_t *target, const int32_t *inv, const RankWindow &win, unsigned long long *tkey,
              float *tscore, unsigned long long *counts, int want_scope);      // (float postings only)
int rank_pq(const float *xq, int nq, int d, const float *cbT, int dsub, int nlist, int64_t ntotal,
            const float *coarse_D, const int32_t *coarse_I, int nprobe, const float *coarse_all,
            const int32_t *list_offsets, const int32_t *tile_offsets, const uint8_t *codes_tiled,
            const int32_t *ids_tiled, const int64_t *target, const int32_t *inv, const RankWindow &win,
            unsigned long long *tkey, float *tscore, unsigned long long *counts, int want_scope);
int rank_finish(const unsigned long long *tkey, const float *tscore, const unsigned long long *counts, int nq,
                int64_t *rank, float *score, int64_t *scope);

}  // namespace asl
