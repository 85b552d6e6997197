/*
 * annsolo_mi.h -- C ABI of libannsolo_mi.so, the MI355X (gfx950) implementation of
 * ANN-SoLo's open-modification search hot path.
 *
 * Every entry point names the reference interface it replaces (paths relative to
 * /root/reference). INTEGRATION.md shows the ctypes stubs a maintainer of the
 * reference would add at those seams.
 *
 * Conventions
 *   - plain C types only; no exceptions cross the boundary.
 *   - return value: 0 on success, a negative ASL_ERR_* code on failure;
 *     asl_last_error() returns a thread-local message for the last failure.
 *   - every array argument may be a HOST pointer or a DEVICE (HIP) pointer; the
 *     library detects which (hipPointerGetAttributes) and stages host buffers.
 *     Buffers stay owned by the caller. Handles are owned by the library.
 *   - all work is issued on the stream set by asl_set_stream() (default: the
 *     null stream). Calls that return results into host memory synchronise that
 *     stream before returning; calls whose outputs are device pointers do not.
 *   - one host thread per handle at a time (the reference calls FAISS from one
 *     thread and serialises index loads, spectral_library.py:44,483).
 *   - there is NO CPU fallback: without a HIP device every compute entry point
 *     returns ASL_ERR_NO_DEVICE.
 */
#ifndef ANNSOLO_MI_H
#define ANNSOLO_MI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASL_OK 0
#define ASL_ERR_INVALID (-1)    /* bad argument */
#define ASL_ERR_NO_DEVICE (-2)  /* no HIP device / runtime error */
#define ASL_ERR_STATE (-3)      /* e.g. search on an untrained index */
#define ASL_ERR_CAPACITY (-4)   /* a compiled-in capacity was exceeded (message says which) */
#define ASL_ERR_IO (-5)
#define ASL_ERR_HIP (-6)

#define ASL_INDEX_FLAT 0      /* IndexFlatIP: exact inner product            */
#define ASL_INDEX_IVFFLAT 1   /* IndexIVFFlat(IndexFlatIP, d, nlist, IP)     */
#define ASL_INDEX_IVFPQ 2     /* IVF + product quantiser, by-residual IP ADC */
#define ASL_INDEX_WINFLAT 3   /* window-exact: every vector in the query's precursor window, exact IP (see
                               * "Window scan" below); float32 vectors as given, no training, nlist / pq_* unread */

/* The precursor window of a query: which library rows are its candidates, by the float32 window column
 * `key` (lib_pmz_f32; NaN, or unselected under a selection: never a candidate).
 * ASL_TOL_DA / ASL_TOL_PPM: one tolerance for the batch, symmetric around the query's own precursor m/z q
 * (spectral_library.py:417-429, in double): |q - key| * charge <= tol, or |q - key| / key * 1e6 <= tol.
 * ASL_TOL_INTERVAL: a closed interval per query. Wherever a call takes the queries' precursor m/z for the
 * window test (q_pmz, query_pmz; asl_search_params_t::precursor_window for the fused calls) it then takes
 * [nq, 2] doubles, (lo_i, hi_i) interleaved, and row r passes iff lo_i <= (double)key[r] && (double)key[r]
 * <= hi_i. A NaN key or a NaN bound never passes, lo > hi is an empty window and no error, +-inf are legal
 * bounds; charge and tol are unread. Only the candidates change: the shifted dot product still takes its
 * precursor mass difference from the query's and the row's own precursor m/z, and the window is applied
 * before or after the top-k as configured. (FAISS: IDSelectorRange per query.) asl_index_search_window,
 * asl_index_search_selected and asl_index_rank answer any other value of their mode argument with
 * ASL_ERR_INVALID; asl_window_candidates and precursor_mode of the fused calls are not checked (as before the
 * third mode existed, a value other than these three is read as ASL_TOL_PPM). */
#define ASL_TOL_DA 0
#define ASL_TOL_PPM 1
#define ASL_TOL_INTERVAL 2

const char *asl_last_error(void);
const char *asl_version(void);
/* number of usable HIP devices (faiss.get_num_gpus(), spectral_library.py:73) */
int asl_get_num_gpus(void);
int asl_set_device(int device);
/* hipStream_t to issue work on (NULL = default stream). */
int asl_set_stream(void *hip_stream);
/* Waits for all work issued by the library, including batches of the pipeline below, and
 * reports any error those batches deferred. */
int asl_synchronize(void);
/* Software pipeline for asl_search_batch over internal streams (mode 0 = off, the default).
 * When on, a call with use_ann = 1 whose arrays ALL live on the device and whose
 * queries->n_peaks is set returns without waiting. Mode 1 (= 2): the encoder and the coarse
 * quantiser of a batch run on one stream, list scan + rescoring on a second, so the MFMA-bound
 * front of batch i+1 executes under the scan of batch i. Mode 3 moves filter + rescoring to a
 * third stream (measured no faster on MI355X: both compete for the vector ALUs). Contract in this mode: inputs must stay untouched and outputs are valid only after
 * asl_synchronize() (or a device-wide synchronisation); capacity errors the kernels flag are
 * reported by that call instead. Any other entry point first waits for the batches in flight.
 * Results are bit-identical to the synchronous path. */
int asl_set_pipeline(int on);
/* Where asl_search_batch applies the precursor-window post-filter of the neighbour lists
 * (/root/reference/src/ann_solo/spectral_library.py:417-429 AND :441-446 -- after the top-k in both
 * places): 1 (default) = inside the list scan's finish whenever the lists are consumed as a set (no
 * knn_I requested, layout-specific scan, k <= 1280): ids and window values arrive in one gather, only
 * the passing hits are written, the rescoring walks short rows; 0 = inside the rescoring kernel's
 * compaction (the only place until round 6; still used wherever the scan cannot take the filter).
 * Results are bit-identical. Returns the previous setting; environment ASL_SCAN_POSTFILTER=0 sets
 * the initial value. */
int asl_set_scan_postfilter(int on);
/* Pair budget of the window-only searches (asl_search_batch with use_ann = 0: cascade level 'std',
 * brute-force open search): a batch whose (query, library row) pairs of the precursor windows
 * number more than `pairs` is rescored in tiles of at most that many pairs (values above
 * 2^31 - 1 act as 2^31 - 1), so the scratch of a batch -- 8 bytes per pair of a tile -- is bounded
 * whatever its size and window width. Results do not depend on it. Default 2^28 (2 GiB).
 * Returns the previous budget; pairs <= 0 is ASL_ERR_INVALID (returned, message in
 * asl_last_error). Does not touch the device. */
int64_t asl_set_window_pair_budget(int64_t pairs);

/* ------------------------------------------------------------------ encoder
 * Replaces spectrum_to_vector / get_dim / hash_idx, src/ann_solo/spectrum.py:122-214
 * (callers spectral_library.py:158-161,438-440). Batch form: spectrum i owns
 * peaks [offsets[i], offsets[i+1]). out is row-major [n, hash_len], fully
 * overwritten. min_bound is get_dim()'s start_dim (10.96 for 11/2010/0.04). */
int asl_get_dim(double min_mz, double max_mz, double bin_size, int64_t *n_bins,
                double *start_dim, double *end_dim);
int32_t asl_hash_idx(int64_t bin_idx, int32_t hash_len, uint32_t seed);
int asl_encode_batch(const float *mz, const float *intensity, const int32_t *offsets,
                     int32_t n, double min_bound, double bin_size, int32_t hash_len,
                     uint32_t seed, int norm, float *out);
/* The same vectors as ENTRY LISTS -- the non-zero components only, the form the IVF scans read
 * their queries in (asl_index_search_entries; a hashed spectrum has <= ~50 non-zeros of 800):
 * entries [n][64] pairs of 32-bit words (dimension * 128, the bits of the fp32 value), ascending
 * dimension, unused pairs zero; counts [n] = the number of non-zero components, or -1 - count
 * when a vector has more than 64 (that query needs the dense form); n_over (may be null): a
 * device int the call ADDS the number of such rows to. The values are those asl_encode_batch
 * stores, bit for bit. entries / counts / n_over: device memory; n_peaks = offsets[n] when the
 * caller knows it (>= 0: nothing is read back, the call never waits), else -1. */
int asl_encode_entries_batch(const float *mz, const float *intensity, const int32_t *offsets,
                             int32_t n, int32_t n_peaks, double min_bound, double bin_size,
                             int32_t hash_len, uint32_t seed, int norm, uint32_t *entries,
                             int32_t *counts, int32_t *n_over);

/* ------------------------------------------------------------------ ANN index
 * Replaces the FAISS objects used at spectral_library.py:73-87,167-181,191,
 * 443-445,487-497: IndexFlatIP, IndexIVFFlat(quantizer, d, nlist, IP), train, add,
 * search, nprobe, reset, write_index/read_index. Row ids are implicit 0..ntotal-1
 * in add order. search(): rows sorted by (score desc, id asc); missing results
 * are I = -1, D = -FLT_MAX.
 * IVF-PQ shapes: pq_m in {4, 8, 16, 32, 64} dividing d, pq_bits 1..8 (0: 8), and
 * pq_m * 2^pq_bits + d <= 38 908 floats (a query, its look-up table and the smallest top-k
 * buffer share the 160 KB of LDS of a workgroup); asl_index_create refuses anything else
 * (NULL, asl_last_error says why), and asl_index_load makes the same check of a file. Every
 * accepted shape trains, encodes and searches; how large a k its scan holds shrinks with d
 * (asl_index_search says so where k does not fit). The tiled scan, and with it the window scan,
 * packed-key rows and gated / entry-list searches, serves pq_m = 32 at 8 bits up to d = 1020;
 * a wider index of that shape is searched by the generic kernel, like every other shape. */
typedef struct asl_index asl_index_t;

asl_index_t *asl_index_create(int32_t d, int32_t nlist, int32_t kind, int32_t pq_m,
                              int32_t pq_bits);
void asl_index_free(asl_index_t *idx);
int asl_index_train(asl_index_t *idx, int64_t n, const float *x, uint64_t seed);
int asl_index_add(asl_index_t *idx, int64_t n, const float *x);
/* add() with every vector's inverted list given by the caller (lists[n], host or device) instead
 * of computed by the coarse quantiser: re-creates an index from stored inverted lists, e.g. from
 * a FAISS .idxann file (faiss_compat.read_index_faiss), keeping the file's own assignments. */
int asl_index_add_preassigned(asl_index_t *idx, int64_t n, const float *x, const int32_t *lists);
int asl_index_search(asl_index_t *idx, int32_t nq, const float *xq, int32_t k,
                     int32_t nprobe, float *D, int64_t *I);
int asl_index_reset(asl_index_t *idx);
int64_t asl_index_ntotal(const asl_index_t *idx);
int asl_index_is_trained(const asl_index_t *idx);
int asl_index_save(const asl_index_t *idx, const char *path);
asl_index_t *asl_index_load(const char *path);
/* k-means iterations (FAISS ClusteringParameters.niter, default 25) */
int asl_index_set_niter(asl_index_t *idx, int32_t niter);

/* FAISS' IndexIVFPQ::by_residual. on = 1 (default): the product quantiser is trained on, and encodes,
 * the residuals x - centroid[list]; on = 0: the vectors as they are (the centroids still define the
 * inverted lists and the probes). The inner-product score of a stored vector is FAISS'
 *   dis0 + sum_m LUT[m][code_m],   LUT = q . codebook,
 * with dis0 = q . centroid[list] when by_residual is on and dis0 = 0 when it is off: the scans are the
 * same kernels in both modes, handed the coarse scores or zeros. IVF-PQ only (ASL_ERR_STATE on Flat /
 * IVF-Flat) and only while the index is untrained (ASL_ERR_STATE afterwards: the codebooks belong to
 * the mode they were trained or installed in). With 0, asl_index_set_trained installs quantisers for
 * raw codes. The mode is the handle's own: it survives asl_index_reset, asl_index_shard and
 * asl_index_save / asl_index_load (a raw index is written as file version 3, which earlier builds refuse). */
int asl_index_set_by_residual(asl_index_t *idx, int32_t on);
/* 1 or 0 as set or loaded; 1 for Flat / IVF-Flat (and a null handle). */
int asl_index_get_by_residual(const asl_index_t *idx);

/* Exact re-rank of the IVF-PQ short-list (FAISS IndexRefineFlat's role). kprime > 0, set BEFORE
 * add(): the index also keeps every added vector as a sparse fp32 row (<= 64 non-zeros, 384 B),
 * and asl_index_search / asl_search_batch with k < kprime let the ADC scan return kprime
 * candidates, rescore them with the exact inner product and return the k best, (score desc, id
 * asc) -- for the vectors it reaches, IVF-Flat's scores. kprime = 0 switches the re-rank off (the
 * rows stay). asl_index_refine re-ranks a short-list obtained elsewhere (e.g. merged shard rows).
 * In the unordered modes (asl_index_set_unordered: per-shard rows of a sharded search) the scan
 * returns its ADC candidates UN-refined: a sharded driver asks every shard for kprime hits, merges
 * them by ADC score into the kprime best of the whole index -- the unsharded short-list -- and
 * re-ranks that with asl_index_refine (every rank keeps the exact rows of ALL vectors), so 1 and
 * N GPUs return the same rows. asl_index_search_sharded does exactly this. */
int asl_index_set_refine(asl_index_t *idx, int32_t kprime);
/* kprime of the index (0: re-rank off) -- what a sharded driver needs to size the per-shard rows. */
int asl_index_get_refine(const asl_index_t *idx);
int asl_index_refine(asl_index_t *idx, int32_t nq, const float *xq, int32_t kprime,
                     const int64_t *I_in /* [nq,kprime], -1 = empty */, int32_t k, float *D, int64_t *I);

/* Window scan (FAISS: search(..., params=SearchParametersIVF(sel=IDSelectorRange(..., assume_sorted=true)))).
 * The index keeps a second, derived copy of its tiled IVF-PQ layout in which every inverted list is
 * ordered by a float32 key per vector (the library's precursor m/z), ascending, NaN last; a query's
 * precursor window is then one contiguous run of every list, and only that run is scanned. Never
 * saved; add, add_preassigned, reset and shard drop it. Unsupported (ASL_ERR_STATE, never a silent
 * post-filter): IVF-Flat and Flat, the generic PQ kernel (scan_variant 1, m != 32, bits != 8),
 * k > 1280, a sharded index.
 * ASL_INDEX_WINFLAT (the window-exact index) is the same idea without a coarse quantiser: ALL stored vectors form
 * one list ordered by the key (ascending, NaN last, id ascending), cut into blocks of 832 positions that hold the
 * per-dimension postings of the IVF-Flat scan (asl_index_set_flat_storage: float postings, or fixed-point words
 * in ASL_FLAT_FX22 when every non-zero is on the grid). asl_index_search_window then returns the top-k among
 * all stored vectors whose key passes -- a query's window is one contiguous run of blocks, nprobe is unread --
 * and asl_index_search the top-k of all vectors, NaN keys included (no key needed: before one is set the order
 * is by id). A score is the ascending-dimension fp32 fmaf chain over the stored non-zeros: the bits of the
 * IVF-Flat scan and the Flat index. The layout is derived and never saved (a file holds the kind and the
 * vectors); add, reset and a new key drop it. asl_search_batch and its _topn / _topn_distinct / _topn_hist
 * siblings always scan the window on this kind, with the library handle's window column as the key (a selection
 * arrives as NaN keys); asl_index_set_window_scan is a no-op returning 0. ASL_ERR_STATE, with the reason:
 * asl_index_search_window before a key is set (or after add), k > 1280, vectors too dense for postings (the
 * most non-zeros of a vector, times 8, reach d), asl_index_search_selected, asl_index_rank,
 * asl_index_set_refine, asl_index_set_trained, asl_index_add_preassigned, asl_index_shard and the sharded
 * searches, asl_index_search_preassigned / _gated / _entries, packed-key rows. asl_profile_scanned_vectors
 * counts the runs' lengths.
 * asl_index_set_window_key: sort key per vector id (float32 precursor m/z, NaN = never a candidate),
 * n == ntotal (else ASL_ERR_INVALID): copied, and the window-ordered layout built (IVF-PQ, trained, unsharded, no
 * caller ids; or ASL_INDEX_WINFLAT). */
int asl_index_set_window_key(asl_index_t *idx, int64_t n, const float *key);
/* top-k (score desc, id asc) among the probed lists' vectors whose key passes
 * precursor_ok(q_pmz[i], key, charge, tol, mode) -- the window test of asl_search_batch, same double
 * arithmetic; -1 / -FLT_MAX padded. Same coarse quantiser and nprobe as asl_index_search.
 * mode == ASL_TOL_INTERVAL: q_pmz is [nq, 2]. */
int asl_index_search_window(asl_index_t *idx, int32_t nq, const float *xq, const double *q_pmz,
                            int32_t charge, double tol, int32_t mode, int32_t k, int32_t nprobe,
                            float *D, int64_t *I);
/* 0 (default): asl_search_batch post-filters as the reference (the k best of the probed lists,
 * then the window); 1: it scans each query's window only (the k best in-window vectors of the
 * probed lists), with the window column of the library handle it is given as the key (installed
 * whenever the layout holds another library's key or the lists changed). Per handle. */
int asl_index_set_window_scan(asl_index_t *idx, int32_t on);

/* Subset search (FAISS: search(..., params=SearchParametersIVF(sel=IDSelectorBitmap(...)))). A selector is one
 * byte per vector id, keep[id] != 0 = selected. A selected search returns what asl_index_search (or, with a
 * window, asl_index_search_window) would return if the index held, in the same lists with the same centroids,
 * codebooks and codes, only the selected vectors: the scans choose their k among the selected vectors of the
 * probed lists -- select first, then top-k. Ids and score bits are those of the plain search; nothing is
 * renumbered. The scans read the selector as bits in storage order (a 64-bit word per 64-vector tile of the
 * IVF-PQ layouts, 13 words per block of IVF-Flat postings), derived like the window-ordered layout: never
 * saved, rebuilt when the selector or the lists change. Unselected codes and postings are still read.
 * asl_index_set_selector: n == ntotal (else ASL_ERR_INVALID): copied (keep: host or device memory); n == 0 or
 * keep == NULL drops it. add, add_preassigned, reset and shard drop it too. Waits for pipelined batches in
 * flight. asl_index_search, asl_index_search_window and every other search ignore it. */
int asl_index_set_selector(asl_index_t *idx, int64_t n, const uint8_t *keep);
/* The ordered top-k (score desc, id asc; -1 / -FLT_MAX padded) among the selected vectors of the probed
 * lists; same coarse quantiser and nprobe as asl_index_search. q_pmz == NULL: no window (charge, tol, mode
 * unread). With q_pmz, of the selected vectors only those whose window key passes precursor_ok(q_pmz[i], key,
 * charge, tol, mode; ASL_TOL_INTERVAL: q_pmz is [nq, 2]): the window-ordered layout, which needs
 * asl_index_set_window_key (and, like it, IVF-PQ).
 * Served by the tiled IVF-PQ scan (m = 32, 8 bits, by_residual on or off) and the IVF-Flat postings scan
 * (float and fixed-point postings), k <= 1280, nprobe <= 1024. Everything else is ASL_ERR_STATE with a message
 * that names the reason, never a filter behind the top-k: no selector (or the lists changed since it was set),
 * scan_variant 1, other PQ shapes, dense-row IVF-Flat, a Flat index, k > 1280, an index with the exact
 * re-rank on (asl_index_set_refine, k < kprime), packed-key rows (asl_index_set_unordered 2), a sharded index;
 * and, for requests that reach the index from inside the library, a gate or entry-list-only queries. */
int asl_index_search_selected(asl_index_t *idx, int32_t nq, const float *xq, const double *q_pmz /* NULL: no window */,
                              int32_t charge, double tol, int32_t mode, int32_t k, int32_t nprobe, float *D,
                              int64_t *I);

/* Rank of a given vector in the index's neighbour order (replaces the measurement of the reference's
 * notebooks/iprg2012_num_candidates.ipynb, the cell that searches IndexFlatIP with num_neighbors =
 * 1000000 and looks up where the brute-force match stands): rank[i] = the number of vectors v of the
 * scope with key(score(q_i, v), v) > key(score(q_i, t), t), t = target[i], key = (score desc, id asc),
 * scores being the bits the index's own scan produces. The scope is the vectors of the probed lists
 * -- nprobe = 0: of every list (exhaustive), else of the coarse quantiser's top-nprobe, the lists
 * asl_index_search scans -- and, with key != NULL (float32 per vector id, [ntotal]), of those only the
 * ones that pass precursor_ok(q_pmz[i], key[v], charge, tol, mode), as asl_index_search_window keeps
 * them (ASL_TOL_INTERVAL: q_pmz is [nq, 2]). rank[i] = -1 when the target is not in the scope (target < 0 or >= ntotal, its list not
 * probed, its key NaN or outside the window). So with the same probes and window the target is in the
 * rows of a search for every k > rank and for no k <= rank. score (optional): the target's score, NaN
 * where rank is -1; scope (optional): the number of vectors in the scope. Nothing is kept on the
 * handle. IVF-Flat with float postings and the tiled IVF-PQ (m = 32, 8 bits) only; ASL_ERR_STATE for
 * fixed-point postings, dense-row IVF-Flat, the generic kernels (scan_variant 1, other PQ shapes), a
 * Flat index and a sharded one. A selector (asl_index_set_selector, asl_library_set_selection) is ignored: the scope is
 * every vector of the probed lists. */
int asl_index_rank(asl_index_t *idx, int32_t nq, const float *xq, const int64_t *target /* [nq] */,
                   int32_t nprobe /* 0: all lists */, const float *key /* [ntotal] or NULL: no window */,
                   const double *q_pmz, int32_t charge, double tol, int32_t mode, int64_t *rank /* [nq] */,
                   float *score /* [nq], optional */, int64_t *scope /* [nq], optional */);

/* IVF-Flat component storage. ASL_FLAT_F32 (the default since round 5) keeps every component as
 * given: the float32 vectors FAISS' CPU IndexIVFFlat stores (spectral_library.py:174-181) -- ids
 * and scores are those of an index over the unquantised vectors. ASL_FLAT_FX22 (opt-in; no FAISS
 * counterpart on the CPU, the reference's GPU clone stores float16, spectral_library.py:490-497):
 * add() rounds every
 * component in [0, 1) to the nearest multiple of 2^-22 (ties to even, at most 1 - 2^-22;
 * |dx| <= 1.2e-7) and stores anything else as given. When ALL stored non-zeros are such values --
 * unit-norm hashed spectra always are -- the inverted lists are kept as 4-byte postings
 * (22-bit numerator | 10-bit local index) in whole 128-byte lines behind a one-byte-per-dimension
 * table (csrc/flat_postings.hpp: the layouts; csrc/flat_scan.hip: the scan) instead of 6-byte postings
 * behind 4-byte table words. Scores are
 * the canonical ascending-dimension fp32 fmaf chain over the STORED components either way, so
 * both layouts (and the generic kernels of asl_index_set_scan_variant) return identical ids and
 * score bits for the same stored vectors. Set
 * before the first add(); saved with the index (file version 2; a version-1 file that says
 * fixed point but holds off-grid components -- written before the modes existed -- loads as float32). asl_index_flat_layout: 0 = dense rows only (no
 * postings: vectors too dense), 1 = float postings, 2 = fixed-point postings. */
#define ASL_FLAT_FX22 0
#define ASL_FLAT_F32 1
int asl_index_set_flat_storage(asl_index_t *idx, int32_t mode);
int asl_index_get_flat_storage(const asl_index_t *idx);
int asl_index_flat_layout(asl_index_t *idx);

/* Scan kernel selection (identical results either way; the switch exists for A/B measurements
 * and for the parity tests): 0 = the layout-specific kernels (IVF-PQ: the tiled
 * sub-quantiser-per-lane scan with the histogram top-k when m = 32, 8 bits, nprobe <= 256;
 * IVF-Flat: the per-dimension postings scan), 1 = the generic kernels (IVF-PQ: lane-per-vector
 * scan; IVF-Flat: dense GEMM + masked top-k), 2 = as 0, except that the tiled IVF-PQ scan reads its
 * tile-major codes only. Under 0 a plain IVF-PQ search (no window, selector or gate, unsharded) is scanned
 * from a second, sub-quantiser-major copy of the codes, of which a query fetches only the lines of the
 * sub-vectors in which it has a non-zero component; the copy is derived on the device by the first such
 * search after the lists changed, is never saved, and takes as much memory as the codes themselves.
 * asl_index_codes_mmajor: 1 while that copy exists and matches the lists, else 0.
 * Any other value is ASL_ERR_INVALID. */
int asl_index_set_scan_variant(asl_index_t *idx, int32_t variant);
int asl_index_codes_mmajor(const asl_index_t *idx);

/* Introspection, used by the parity tests and by multi-GPU sharding. Sizes via
 * asl_index_info; every pointer may be NULL to skip. Lists are stored in list
 * order: ids/codes/vecs of list l are [list_offsets[l], list_offsets[l+1]). */
typedef struct {
  int32_t d, nlist, kind, pq_m, pq_ksub, pq_dsub;
  int64_t ntotal;      /* vectors added through this handle (global count)      */
  int64_t nlocal;      /* vectors stored on this shard (== ntotal if unsharded) */
  int32_t trained, shard_rank, shard_world;
} asl_index_info_t;
int asl_index_info(const asl_index_t *idx, asl_index_info_t *info);
int asl_index_get_centroids(const asl_index_t *idx, float *centroids /* [nlist,d] */);
int asl_index_get_codebooks(const asl_index_t *idx, float *cb /* [m,ksub,dsub] */);
/* Install externally trained quantisers (FAISS: quantizer.add(centroids) / pq copy). */
int asl_index_set_trained(asl_index_t *idx, const float *centroids, const float *codebooks);
int asl_index_get_lists(const asl_index_t *idx, int32_t *list_offsets /* [nlist+1] */,
                        int32_t *ids /* [nlocal] */, uint8_t *codes /* [nlocal,m] PQ */,
                        float *vecs /* [nlocal,d] FLAT */);
/* Keep only the inverted lists owned by `rank` of `world` (greedy heaviest-first balancing
 * of the expected scan load, weight = list size squared; identical on every rank, see
 * asl_lpt_owner). Must be called after add(). search() then
 * returns this shard's partial top-k; combine with asl_topk_merge. */
/* Unordered result rows: with mode 1 subsequent IVF-PQ searches return the exact top-k of
 * every query as a SET -- same ids and scores, unspecified order inside the row, padding last
 * -- and skip the final sort. For consumers that re-order anyway (asl_topk_merge of shard
 * results). Mode 2 additionally packs every hit into one 64-bit key in the int64 output
 * (order-preserving score bits << 32 | ~id, 0 = empty; D is not written): 8 instead of 12
 * bytes per hit on the wire of a sharded search; merge with asl_topk_merge_keys. 0 = sorted. */
int asl_index_set_unordered(asl_index_t *idx, int32_t mode);
/* Merge of S packed-key lists Ks[S, nq, k] (mode 2 above) -> D[nq,k] (may be NULL), I[nq,k];
 * k <= 1280. unordered != 0: the rows hold the exact top-k as a set (no final sort), for
 * consumers such as asl_rescore_knn that do not depend on the order. */
int asl_topk_merge_keys(int32_t S, int32_t nq, int32_t k, const int64_t *Ks, float *D, int64_t *I,
                        int32_t unordered);
int asl_index_shard(asl_index_t *idx, int32_t rank, int32_t world);
/* The sharded search itself, for hosts that bind the C ABI directly: every rank
 * of `rccl_comm` (an ncclComm_t the caller created; one rank per GPU) calls this with ITS nq
 * queries -- the same nq everywhere, device pointers only -- after asl_index_shard(idx, rank,
 * world) on an index that was filled identically on every rank. All-gather of the queries (as
 * entry lists, 516 bytes per query, whenever the packed-key scans run; a batch holding a query with
 * more than 64 non-zero components is repeated with dense rows) and of
 * the probe lists, scan of the local inverted lists for all world x nq queries, grouped
 * send/recv of the per-shard top-k (all-to-all), merge: D / I [nq, k] equal the unsharded
 * index's rows for these queries. Enqueued on the library's stream; RCCL is resolved from the
 * process at first use (never linked). */
int asl_index_search_sharded(asl_index_t *idx, void *rccl_comm, int32_t nq, const float *xq,
                             int32_t k, int32_t nprobe, float *D, int64_t *I);
/* The same with the exchange's three sizes given: keys a head carries (<= 0: ceil(2k / world)), the
 * shards' own k (<= 0: asl_shard_k(k, world)), answer slots per query and destination (< 0:
 * max(8, k / 16)). The result does not depend on them (a buffer that runs full sends the batch
 * down the full-row exchange); tests set them to run every step of the exchange on a communicator
 * of any size -- at world 1 the default head is the whole row. */
int asl_index_search_sharded_ex(asl_index_t *idx, void *rccl_comm, int32_t nq, const float *xq,
                                int32_t k, int32_t nprobe, float *D, int64_t *I, int32_t head_keys,
                                int32_t shard_keys, int64_t extras_per_query);
/* 1 if asl_index_search_preassigned can emit packed keys (unordered mode 2) for this index at
 * (k, nprobe) -- IVF-PQ: the tiled scan (m = 32, 8-bit codes, automatic scan variant, nprobe
 * within the tiled kernel's limit, k + 768 <= 2048); IVF-Flat: the postings scan (sparse stored
 * vectors, k <= 1280) --, else 0 (exchange (D, I) rows then). Builds the scan layout if it is
 * out of date, so the answer is the one a search would meet. For IVF-Flat it depends on the
 * vectors THIS shard holds (an empty or dense shard scans dense rows): a sharded driver must
 * agree on it across ranks (MIN) before choosing the exchange format, as distributed.py and
 * asl_index_search_sharded do. */
int asl_index_supports_keys(asl_index_t *idx, int32_t k, int32_t nprobe);
/* The exact top-k exchange of a sharded search (csrc/exchange.hip; device pointers only; what
 * ann_solo_amd/distributed.py and asl_index_search_sharded run between their collectives; no
 * reference counterpart: spectral_library.py:494 uses device 0 only). Rows of packed keys as
 * asl_index_set_unordered mode 2 emits them (0 = empty, any order).
 *   asl_keys_split: K [nrows, k_s] -> head [nrows, kp] (slots 0 .. kp-2: the row's best keys, all
 *     those at or above a score-bucket floor that admits at most kp - 1; slot kp-1: T, the best
 *     key held back, 0 if none), floor [nrows] (that bucket floor: the keys held back are the
 *     keys of K below it, which stay where they are) and -- rowmin != NULL, for shards that scan
 *     with k_s < k -- rowmin [nrows]: the row's smallest key if the row is FULL (the scan may have
 *     dropped keys, all below it), else 0.
 *   asl_keys_merge_heads: heads [S, nq, kp] of the S shards -> out_keys [nq, k] (the best k keys
 *     seen, a set), bounds [S, nq] (B = the k-th best key seen if shard s must send what it holds
 *     above B -- its T beats B --, else ~0: send nothing), need [nq] (some shard was asked).
 *   asl_keys_rescan_list: on the shard (k_s < k), after the bounds arrived: the rows whose bound
 *     lies below rowmin -- a dropped key may be above the bound -- -> rowlist [R] (int64, ZEROED BY
 *     THE CALLER; the first *count slots), rmap [nrows] (slot or -1), *count += their number
 *     (device memory: the gate of asl_index_search_gated, which scans exactly those rows again
 *     with the full k); more than R rows: *overflow = 1.
 *   asl_keys_extras: on the shard, rows destination-major (row = dst * nq + q): K [W * nq, k_s]
 *     and floor [W * nq] as asl_keys_split saw / wrote them, bounds [W * nq] -> xbuf
 *     [W, nq + xcap]: per destination nq header words (count << 32 | start) then the payload =
 *     the row's keys outside the head above the bound; rmap != NULL: a row with rmap[row] >= 0
 *     answers from K3 [rmap[row], k3], its second scan. cursor [W] int32, ZEROED BY THE CALLER
 *     (the payload cursors; the call returns without waiting); *overflow = 1 when a
 *     destination's xcap slots do not suffice (the caller must then repeat the batch with the
 *     full exchange of k-deep rows). *overflow is never cleared here.
 *   asl_keys_merge_final: heads + the xbuf [S, nq + xcap] received (NULL: none) + out_keys/need of
 *     asl_keys_merge_heads -> I [nq, k] ids (a set, -1 padded) and D (may be NULL): the exact
 *     top-k of the union of the shards' FULL rows. k <= 1280. */
int asl_keys_split(int64_t nrows, int32_t k, int32_t kp, const int64_t *K, int64_t *head, int32_t *floor,
                   int64_t *rowmin);
int asl_keys_merge_heads(int32_t S, int32_t nq, int32_t kp, int32_t k, const int64_t *heads,
                         int64_t *out_keys, int64_t *bounds, int32_t *need);
int asl_keys_rescan_list(int64_t nrows, const int64_t *bounds, const int64_t *rowmin, int32_t R, int64_t *rowlist,
                         int32_t *rmap, int32_t *count, int32_t *overflow);
int asl_keys_extras(int32_t W, int32_t nq, int32_t k, const int64_t *K, const int32_t *floor,
                    const int64_t *bounds, int64_t xcap, int64_t *xbuf, int32_t *cursor, int32_t *overflow,
                    const int32_t *rmap, const int64_t *K3, int32_t k3);
int asl_keys_merge_final(int32_t S, int32_t nq, int32_t kp, int32_t k, const int64_t *heads,
                         const int64_t *xbuf, int64_t xcap, const int64_t *prev_keys, const int32_t *need,
                         float *D, int64_t *I);
/* The shards' own k for a final k at `world` ranks: k / 2 from 8 ranks on, 5 k / 8 from 4
 * (rounded up to 64); k itself below 4 ranks or when that is not more than the head's
 * ceil(2 k / world) key slots (pure host integer code). */
int32_t asl_shard_k(int32_t k, int32_t world);
/* asl_index_search_preassigned for a list whose length only the device knows (device pointers
 * only, never waits): a launch for `cap` rows of which the first *count are searched; the other
 * rows of D / I stay untouched. Layout-specific scans only (what asl_index_supports_keys says). */
int asl_index_search_gated(asl_index_t *idx, int32_t cap, const float *xq, int32_t k, int32_t nprobe,
                           const float *coarse_D, const int32_t *coarse_I, float *D, int64_t *I,
                           const int32_t *count);
/* asl_index_search_preassigned with the queries as entry lists (asl_encode_entries_batch) instead
 * of dense rows: 512 bytes per query instead of 3.2 KB and no listing pass -- a sharded search
 * encodes the other ranks' queries straight into this form. Results equal the dense call's, bit
 * for bit. A row with a negative count is searched as an all-zero query (watch the encoder's
 * n_over). count (may be null): as in asl_index_search_gated. Device pointers only, never waits;
 * layout-specific scans only (what asl_index_supports_keys says), not with the exact re-rank. */
int asl_index_search_entries(asl_index_t *idx, int32_t nq, const uint32_t *entries, const int32_t *counts,
                             int32_t k, int32_t nprobe, const float *coarse_D, const int32_t *coarse_I,
                             float *D, int64_t *I, const int32_t *count);
/* list -> owner rank map of the balancing above, for inspection. */
int asl_index_shard_map(const asl_index_t *idx, int32_t world, int32_t *owner /* [nlist] */);

/* The list -> rank balancing rule by itself (pure host integer code, no device):
 * lists sorted by size descending (ties: lower list id first), each given to the
 * currently least-loaded rank (ties: lower rank). */
int asl_lpt_owner(int32_t nlist, const int64_t *sizes, int32_t world, int32_t *owner);

/* IndexIVF::search_preassigned: like asl_index_search but with the coarse quantiser's
 * answer supplied by the caller (coarse_D / coarse_I [nq, nprobe], as asl_index_coarse
 * emits; -1 entries are skipped). Used by the sharded search: every rank quantises only
 * its own slice of the batch, the probe lists are all-gathered, and each rank scans its
 * own inverted lists for the whole batch. IVF-PQ and IVF-Flat (which ignores coarse_D: its
 * scores do not contain the coarse term). An IVF-PQ index with by_residual off
 * (asl_index_set_by_residual) reads coarse_I alone, here and in asl_index_search_gated /
 * asl_index_search_entries: the caller's coarse_D selects nothing and adds nothing (dis0 = 0).
 * asl_index_coarse returns the real q . centroid in either mode. */
int asl_index_search_preassigned(asl_index_t *idx, int32_t nq, const float *xq, int32_t k,
                                 int32_t nprobe, const float *coarse_D,
                                 const int32_t *coarse_I, float *D, int64_t *I);

/* Merge S partial results [S, nq, k] into [nq, k] under (score desc, id asc). */
int asl_topk_merge(int32_t S, int32_t nq, int32_t k, const float *Ds, const int64_t *Is,
                   float *D, int64_t *I);

/* Algorithmic work of the IVF-Flat postings scan for these queries at this nprobe (measurement;
 * no reference counterpart): *bytes = sum over (query, probed block, non-zero query dimension)
 * of the 4-byte table word + 6 bytes per posting (fixed-point layout: 1-byte table entry + 4
 * bytes per posting); *lines = the 128-byte lines the scan touches for them (segments are placed
 * by line; fixed-point layout: the block's whole table row + the lines of the wanted segments).
 * What bench.py prices the scan kernel's roofline with. */
int asl_index_postings_work(asl_index_t *idx, int32_t nq, const float *xq, int32_t nprobe,
                            int64_t *bytes, int64_t *lines);

/* Exposed stages of the IVF search (parity tests; each mirrors one oracle function). */
int asl_index_coarse(asl_index_t *idx, int32_t nq, const float *xq, int32_t nprobe,
                     float *coarse_D /* [nq,nprobe] */, int32_t *coarse_I /* [nq,nprobe] */);
int asl_index_pq_lut(asl_index_t *idx, int32_t nq, const float *xq,
                     float *lut /* [nq,m,ksub] */);

/* ------------------------------------------------------------------ rescoring
 * Replaces get_best_match (src/ann_solo/spectrum_match.pyx:28-108) and
 * SpectrumMatcher::dot (src/ann_solo/SpectrumMatch.cpp:8-133), batched over
 * queries. Spectra are packed SoA; peaks ascending in m/z; `charge` is the
 * per-peak fragment-charge annotation (0 = none, pyx:74-79; ignored for queries). */
typedef struct {
  int32_t n;
  const int32_t *offsets;          /* [n+1] */
  const float *mz;                 /* [offsets[n]] */
  const float *intensity;          /* [offsets[n]] */
  const uint8_t *charge;           /* [offsets[n]] or NULL (all 0) */
  const double *precursor_mz;      /* [n] */
  const int32_t *precursor_charge; /* [n] */
  int64_t n_peaks;                 /* offsets[n] when the caller knows it, else 0: device-resident
                                      offsets are then read back (one stream synchronisation) */
} asl_peaks_t;

/* Candidates of query q are library rows cand_rows[cand_offsets[q] .. cand_offsets[q+1]).
 * Entries < 0 are skipped. Outputs (each may be NULL):
 *   best_cand[q]  position inside the query's candidate list (first strict maximum
 *                 wins, SpectrumMatch.cpp:118), -1 if the list has no valid entry
 *   best_score[q] SpectrumMatcher::dot score (double)
 *   pm_count[q]   number of matched peak pairs of the winner
 *   pm_pairs      [nq, pm_stride, 2] (query_peak, candidate_peak) in greedy order, zero beyond
 *                 pm_count[q] (asl_search_batch / asl_rescore_knn write every slot)
 *
 * `allow_shift` -- here, in the _topn entries below and as asl_search_params_t.allow_shift -- is a FLAG
 * WORD. 0 and 1 mean what they always meant; any bit other than the two below is ASL_ERR_INVALID.
 *   ASL_SCORE_SHIFT         the shifted dot product (config.allow_peak_shifts)
 *   ASL_SCORE_FRAGMENT_PPM  fragment_mz_tolerance t is in ppm of the QUERY peak's m/z, not in Da:
 *       rel   = t * 1e-6                      (fp64, once)
 *       tol_i = rel * (double)q_mz[i]         (fp64, one multiply) is the window of query peak i,
 *     read wherever SpectrumMatcher::dot reads its tolerance for that peak: the cursor test
 *     (double)q_mz[i] - tol_i > x and the window test fabs((double)q_mz[i] - x) <= tol_i, with
 *     x = (double)c_mz[j] + mass_diff[s] as before; and the shift gate (SpectrumMatch.cpp:20) becomes
 *     num_shifts = (shift && fabs(pmd) >= rel * q_precursor_mz) ? charge + 1 : 1. Products, their
 *     order, the greedy assignment, the fp64 sum and the tie rules between candidates do not change;
 *     with the flag clear every output is what it was, bit for bit. (The reference's
 *     --fragment_tol_mode never reaches its dot product, which reads the number as Da whatever the
 *     flag says: this mode has no counterpart there.) */
#define ASL_SCORE_SHIFT 1
#define ASL_SCORE_FRAGMENT_PPM 2
int asl_rescore_batch(const asl_peaks_t *queries, const asl_peaks_t *library,
                      const int64_t *cand_rows, const int32_t *cand_offsets,
                      double fragment_mz_tolerance, int allow_shift, int32_t *best_cand,
                      double *best_score, int32_t *pm_count, uint32_t *pm_pairs,
                      int32_t pm_stride);

/* The n best candidates of every query instead of the single best (top-n rescoring), 1 <= n_best <=
 * ASL_MAX_BEST (anything else: ASL_ERR_INVALID). Every candidate slot is scored once, as in
 * asl_rescore_batch; one more pass over the scores selects the n best in the order
 *   score descending, then position in the query's list ascending
 * (rank 0 is asl_rescore_batch's winner, bit for bit), and the peak matches of each are emitted.
 * Every slot of a list is a candidate of its own: a row listed twice can take two ranks, the
 * earlier position first. Outputs (each may be NULL, host or device memory, every element written):
 *   best_cand  [nq, n_best]  position inside the query's list; -1 for the ranks beyond the list's
 *                            valid entries (then score 0.0, count 0, zero pairs)
 *   best_score [nq, n_best], pm_count [nq, n_best], pm_pairs [nq, n_best, pm_stride, 2] */
#define ASL_MAX_BEST 16
int asl_rescore_batch_topn(const asl_peaks_t *queries, const asl_peaks_t *library,
                           const int64_t *cand_rows, const int32_t *cand_offsets,
                           double fragment_mz_tolerance, int allow_shift, int32_t n_best,
                           int32_t *best_cand, double *best_score, int32_t *pm_count,
                           uint32_t *pm_pairs, int32_t pm_stride);

/* DISTINCT ranked matches: asl_rescore_batch_topn with one rule added. Every library row carries a
 * 32-bit group id (lib_group [library->n], host or device memory; e.g. its peptide). The slots of a
 * list are walked in asl_rescore_batch_topn's order -- score descending, then position ascending --
 * and a slot is skipped when an earlier rank already holds a row of the same group, so the ranks
 * name n different groups, each by its best slot. A negative id means "ungrouped": such a row
 * collides with nothing, not even with itself listed twice. Rank 0 is asl_rescore_batch's winner,
 * bit for bit; ranks beyond the last distinct group hold -1 / 0.0 / 0 / zero pairs; with every id
 * negative the outputs equal asl_rescore_batch_topn's byte for byte. Exact: the selection keeps,
 * per lane and per tile, the best slot of every group it may still need.
 * lib_group == NULL is ASL_ERR_INVALID; n_best as in asl_rescore_batch_topn. */
int asl_rescore_batch_topn_distinct(const asl_peaks_t *queries, const asl_peaks_t *library,
                                    const int64_t *cand_rows, const int32_t *cand_offsets,
                                    const int32_t *lib_group /* [library->n] */,
                                    double fragment_mz_tolerance, int allow_shift, int32_t n_best,
                                    int32_t *best_cand, double *best_score, int32_t *pm_count,
                                    uint32_t *pm_pairs, int32_t pm_stride);

/* SCORE HISTOGRAM: the ranked calls keep the n best scores of a query and drop the rest; the *_hist
 * calls also say how ALL of the query's scored candidates are distributed, which is what tells a
 * winner among 160 candidates from one among 350 000 (ann_solo_amd/score_stats.py fits an expectation
 * value to it). score_hist is [nq, ASL_SCORE_HIST_BINS] int32, host or device memory, every element
 * written: ASL_SCORE_HIST_BINS bins of width 1/128 over [0, 1], lower edges inclusive; a candidate
 * with exact score s (the double the ranks report, s >= 0) is counted in bin
 *   !(s < 1.0) ? ASL_SCORE_HIST_BINS - 1 : (int)(s * 128.0)
 * (the product is exact, so this is floor(128 s); everything at or above 1 is in the top bin).
 * Counted are exactly the slots n_cand counts -- valid entries that pass the filter and the
 * selection; a row listed twice counts twice, an entry below 0 never -- so sum(score_hist[q]) ==
 * n_cand[q] for every query, on every path, at any pair budget; a query without candidates reads all
 * zero. The histogram does not depend on n_best or distinct. Counts are integers summed with integer
 * adds: the result does not depend on any order.
 * asl_rescore_batch_topn_hist is asl_rescore_batch_topn (distinct == 0; lib_group is not read) or
 * asl_rescore_batch_topn_distinct (distinct != 0; lib_group == NULL is then ASL_ERR_STATE) with the
 * histogram added. score_hist == NULL: exactly those calls, launch for launch and bit for bit; with the
 * pointer set every other output is unchanged. n_best as in asl_rescore_batch_topn (n_best = 1: the
 * single winner); synchronous. */
#define ASL_SCORE_HIST_BINS 128
int asl_rescore_batch_topn_hist(const asl_peaks_t *queries, const asl_peaks_t *library,
                                const int64_t *cand_rows, const int32_t *cand_offsets,
                                const int32_t *lib_group /* [library->n], read when distinct */,
                                double fragment_mz_tolerance, int allow_shift, int32_t n_best,
                                int32_t distinct, int32_t *best_cand, double *best_score,
                                int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride,
                                int32_t *score_hist /* [nq, ASL_SCORE_HIST_BINS] or NULL */);

/* ------------------------------------------------------------------ peak preprocessing
 * Replaces process_spectrum (src/ann_solo/spectrum.py:57-119: spectrum_utils set_mz_range,
 * round(resolution,'sum'), remove_precursor_peak(tol,'Da',2), filter_intensity,
 * scale_intensity, L2 norm, and the validity checks of :13-36), batched. Raw peaks ascending
 * in m/z, <= 4096 per spectrum. Outputs are padded to max_peaks per spectrum: out_mz /
 * out_intensity / out_src [n, max_peaks] (out_src = index of the kept peak inside its raw
 * spectrum -- after rounding: of the most intense of the merged peaks, whose annotation
 * survives --, may be NULL), out_count[n], out_valid[n] (is_valid). Only the first out_count[s]
 * slots of a spectrum's row are defined (none for an invalid spectrum); what the rest hold is
 * unspecified. One raw spectrum above 4096 peaks fails the WHOLE call with ASL_ERR_CAPACITY (the
 * outputs of the others are not to be used), so callers must split or pre-filter such spectra.
 * A NaN intensity of either sign among the peaks that reach the intensity filter (in range, after
 * the merge's sums, not removed with the precursor) makes its spectrum invalid: it is the base
 * peak, and nothing is above a NaN threshold.
 * scaling: 0 none, 1 rank, 2 root. */
typedef struct {
  double min_mz, max_mz;              /* config.min_mz / max_mz (inclusive) */
  int32_t remove_precursor;           /* config.remove_precursor */
  double remove_precursor_tolerance;  /* config.remove_precursor_tolerance (Da) */
  double min_intensity;               /* config.min_intensity (relative to the base peak) */
  int32_t max_peaks;                  /* config.max_peaks_used(_library), <= 256 */
  int32_t scaling;
  int32_t min_peaks;                  /* config.min_peaks */
  double min_mz_range;                /* config.min_mz_range */
  int32_t round_mz;                   /* config.resolution is not None (spectrum.py:84) */
  int32_t resolution;                 /* config.resolution: decimals of MsmsSpectrum.round */
} asl_process_params_t;
int asl_process_batch(const asl_peaks_t *raw, const asl_process_params_t *params,
                      float *out_mz, float *out_intensity, int32_t *out_src,
                      int32_t *out_count, uint8_t *out_valid);

/* ------------------------------------------------------------------ decoy spectra
 * Replaces the per-spectrum shuffle_and_reposition of src/ann_solo/decoy_generator.py:93-185 (annotate
 * the library spectrum with its peptide's a / b / p / y fragments, move every annotated peak to the same
 * fragment of the shuffled peptide, re-sort), batched. The shuffle itself is the caller's: spectrum s
 * brings its peptide as L = seq_offsets[s+1] - seq_offsets[s] residue masses m[0..L) (residue_mass,
 * modifications folded into their residue), the permutation perm[0..L) (decoy residue i is target residue
 * perm[i]; indices inside the spectrum's own slice), the terminal additions nterm[s] / cterm[s], which stay
 * on the termini, and the largest fragment charge max_fragment_charge[s]. Raw peaks ascending in m/z.
 * The arithmetic, all in IEEE double without fused multiply-add, is the contract:
 *  1. ladders, sequential: P[0] = nterm, P[k] = P[k-1] + m[k-1]; S[0] = cterm, S[k] = S[k-1] + m[L-k];
 *     the same two over m[perm[.]] for the decoy.
 *  2. fragments, ion types in the order a, b, p, y (codes 1..4): base b = P[k], a = P[k] - 27.994915,
 *     y = S[k] + 18.010565 for k = 1..L-1; p = (P[L] + cterm) + 18.010565 with k = L only. Fragment charge
 *     z = 1..max_fragment_charge. Neutral losses in this order (loss index 0..13): 0, -1.007825, -17.026549,
 *     -18.010565, -27.994915, -43.989829, -45.021464, -46.005479, -63.998301, -79.956818, -79.966331,
 *     -91.009195, -91.993211, -97.976896. theo = (base + loss) / z + 1.007276466: add, divide, add.
 *  3. peak i, x = (double)mz[i], matches a fragment iff fabs(x - theo) <= tolerance (ASL_TOL_DA) or
 *     fabs(x - theo) <= (tolerance * 1e-6) * theo (ASL_TOL_PPM: of the theoretical m/z). It is annotated
 *     with the match of LOWEST theo; exact ties by ion type, then k, then z, then loss index. No match: no
 *     annotation.
 *  4. an annotated peak moves to theo_decoy + (x - theo), theo_decoy being the same (type, k, z, loss) on
 *     the decoy's ladders; any other peak keeps x. Intensities travel with their peaks.
 *  5. stable ascending order by the double m/z (ties: raw peak index), then one rounding to float.
 * Outputs, each nullable, in raw's own CSR layout (element offsets[s] + j): out_mz / out_intensity, out_src
 * (the raw peak, inside its spectrum, decoy peak j came from), out_charge (its fragment charge, 0 = not
 * annotated), and in RAW peak order the annotation found: ann_type (0 none, 1 a, 2 b, 3 p, 4 y), ann_n (k),
 * ann_z, ann_loss (loss index). Spectra without peaks are legal.
 * Limits, all checked on the host before anything is launched or written: more than 4096 peaks, L > 128 or
 * max_fragment_charge > 8: ASL_ERR_CAPACITY; L < 2, max_fragment_charge < 1, a perm that is no permutation
 * of 0..L-1, a non-finite mass, a negative or NaN tolerance, a unit other than the two: ASL_ERR_INVALID. */
int asl_decoy_batch(const asl_peaks_t *raw, const int32_t *seq_offsets /* [n + 1] */,
                    const double *residue_mass, const int32_t *perm, const double *nterm /* [n] */,
                    const double *cterm /* [n] */, const int32_t *max_fragment_charge /* [n] */,
                    double tolerance, int32_t tolerance_unit, float *out_mz, float *out_intensity,
                    int32_t *out_src, uint8_t *out_charge, uint8_t *ann_type, uint8_t *ann_n,
                    uint8_t *ann_z, uint8_t *ann_loss);

/* ------------------------------------------------------------------ modification site localisation
 * An open-modification match says "this query spectrum is library peptide P carrying an unknown mass
 * delta"; this call says which residue of P the query's own peaks put that mass on, batched over SSMs.
 * SSM s brings: its query spectrum (spectrum s of `queries`, peaks ascending in m/z, intensities used as
 * given; precursor_mz / precursor_charge / charge are not read), the library peptide as L = seq_offsets[s+1]
 * - seq_offsets[s] residue masses m[0..L) (the peptide's own modifications folded in) with nterm[s], cterm[s]
 * and max_fragment_charge[s], the mass to place delta[s] (Da, neutral; 0 is legal) and one tolerance for the
 * batch (ASL_TOL_DA, or ASL_TOL_PPM: of the THEORETICAL m/z, as for the decoys).
 * The arithmetic, all in IEEE double without fused multiply-add, is the contract:
 *  1. ladders, sequential, exactly asl_decoy_batch's step 1: P[0] = nterm, P[k] = P[k-1] + m[k-1];
 *     S[0] = cterm, S[k] = S[k-1] + m[L-k].
 *  2. fragments: k = 1..L-1, ion types b then y, variant v = 0 (plain) or 1 (carries the modification):
 *     b base P[k], and P[k] + delta for v = 1; y base S[k] + 18.010565, and (S[k] + 18.010565) + delta for
 *     v = 1. Charge z = 1..max_fragment_charge, theo = base / z + 1.007276466. No a ions, no precursor
 *     ion, no neutral losses.
 *  3. evidence: peak i, x = (double)mz[i], matches iff -R <= x - theo && x - theo <= R with R = tolerance
 *     (Da) or (tolerance * 1e-6) * theo (ppm). A fragment at charge z contributes (double)intensity[i] of
 *     its most intense matching peak (ties: the lowest i) and 1 to a hit count; nothing matching: 0.0 and
 *     0. E[type][k][v] is the sum of the contributions over z = 1, 2, .. in that order from 0.0,
 *     C[type][k][v] the hit count.
 *  4. sites j = 0..L-1 (residue index, N-terminal residue first): b_k carries the modification iff
 *     k >= j + 1, y_k iff k >= L - j. score[j] is the sequential double sum, from 0.0, over k = 1..L-1 of
 *     E[b][k][v_b] then E[y][k][v_y]; count[j] the same sum over C. none_score / none_count: the same with
 *     every v = 0.
 *  5. summary: best_score is the largest score[j]; best_lo / best_hi the first and last site whose score
 *     equals it by exact double equality (two sites that no present fragment tells apart add the same
 *     addends in the same order, so they tie bit for bit), n_best their number, best_count =
 *     count[best_lo]; runner_score the largest score strictly below best_score, or best_score itself when
 *     every site ties.
 * Outputs, each nullable, host or device memory: per site, in the peptides' own CSR layout (element
 * seq_offsets[s] + j), site_score and site_count; per SSM best_lo, best_hi, n_best, best_count, best_score,
 * runner_score, none_score. A spectrum without peaks is legal: every score 0, best_lo = 0, best_hi = L - 1.
 * Limits, those of the decoys, all checked on host copies of the small arrays before anything is launched or
 * written: more than 4096 peaks, L > 128 or max_fragment_charge > 8: ASL_ERR_CAPACITY; L < 2,
 * max_fragment_charge < 1, a non-finite mass / terminus / delta, a negative or NaN tolerance, a unit other
 * than the two: ASL_ERR_INVALID. Ascending m/z is a precondition for the result, not for safety: no step
 * reads outside a spectrum's slice whatever the order of its peaks. Synchronous. */
int asl_localize_batch(const asl_peaks_t *queries, const int32_t *seq_offsets /* [n + 1] */,
                       const double *residue_mass, const double *nterm /* [n] */,
                       const double *cterm /* [n] */, const int32_t *max_fragment_charge /* [n] */,
                       const double *delta /* [n] */, double tolerance, int32_t tolerance_unit,
                       double *site_score, int32_t *site_count, int32_t *best_lo, int32_t *best_hi,
                       int32_t *n_best, int32_t *best_count, double *best_score, double *runner_score,
                       double *none_score);

/* ------------------------------------------------------------------ chimeric spectra: depletion
 * A co-fragmented scan holds the peaks of two peptides. This call takes an identification, removes from the
 * query every peak its winner explains and hands back the rest as a processed spectrum to search again.
 * SSM s is query spectrum s of `queries` against row lib_rows[s] of `library` (peaks ascending in m/z in both;
 * queries->charge and queries->precursor_charge are not read; library->charge == NULL: every charge 0).
 * "Explained" is the dot product's own window test -- the peak could have entered SpectrumMatcher::dot's match
 * list -- and the arithmetic, all in IEEE double without fused multiply-add, is the contract:
 *  1. shifts: z the library row's precursor charge, t = fragment_mz_tolerance,
 *       pmd = (q_pmz - l_pmz) * (double)z.
 *     `allow_shift` is asl_rescore_batch's FLAG WORD (any other bit: ASL_ERR_INVALID). ASL_SCORE_FRAGMENT_PPM
 *     clear: tol_i = t for every query peak i and the gate is fabs(pmd) >= t. Set: rel = t * 1e-6, tol_i =
 *     rel * (double)q_mz[i], the gate is fabs(pmd) >= rel * q_pmz.
 *       num_shifts = (ASL_SCORE_SHIFT && gate) ? z + 1 : 1; mass_diff[0] = 0, mass_diff[c] = pmd / c, c >= 1.
 *     The rescoring names no largest charge (it reads whatever the row holds; z + 1 <= 0: no shift at all,
 *     not even c = 0), and neither does this call.
 *  2. explained: query peak i iff there is a library peak j and a c < num_shifts with
 *       fabs((double)q_mz[i] - ((double)l_mz[j] + mass_diff[c])) <= tol_i  and
 *       (c == 0 || l_charge[j] == c || l_charge[j] == 0)     (the dot product's match_multiplier > 0).
 *     There is no cursor: any (j, c) will do.
 *  3. residue: the unexplained peaks in their order, out_mz / out_src (the peak's index in its query) as they
 *     are; intensities re-normalised exactly as asl_process_batch normalises: acc = 0.0f, acc = fmaf(v, v, acc)
 *     over the kept intensities v in ascending order (float32), nrm = sqrtf(acc), out_intensity = v / nrm (IEEE
 *     divide). kept_energy[s] = acc: for a unit-norm query the share of squared intensity the winner leaves.
 *  4. out_count[s] = n, the kept peaks; out_valid[s] = n >= min_peaks && n > 0 && (double)(mz_last - mz_first)
 *     >= min_mz_range with the float32 difference of the last and first kept m/z (asl_process_batch's is_valid).
 * Rows with lib_rows[s] < 0: count 0, valid 0, energy 0. out_mz / out_intensity / out_src are [n, out_stride]
 * and every slot is written: zero beyond out_count[s]. out_src and kept_energy may be NULL; every array may
 * live in host or device memory.
 * Limits, all checked on host copies of the small arrays before anything is launched or written: more than
 * 4096 peaks in a query or in a named library row, or out_stride below the largest query: ASL_ERR_CAPACITY; a
 * negative or NaN tolerance, a flag bit other than the two, a row >= library->n: ASL_ERR_INVALID. Ascending
 * m/z is a precondition for the result, not for safety: no step reads outside a spectrum's slice whatever the
 * order of its peaks. No atomics: equal inputs give equal bits. Synchronous. */
int asl_deplete_batch(const asl_peaks_t *queries, const asl_peaks_t *library,
                      const int64_t *lib_rows /* [n]; < 0: skip */,
                      double fragment_mz_tolerance, int allow_shift /* the flag word */,
                      int32_t min_peaks, double min_mz_range, int32_t out_stride,
                      float *out_mz, float *out_intensity, int32_t *out_src /* nullable */,
                      int32_t *out_count, uint8_t *out_valid, float *kept_energy /* nullable */);

/* ------------------------------------------------------------------ SSM features
 * Replaces the per-SSM SpectrumSimilarityCalculator calls of _compute_ssm_features
 *   /root/reference/src/ann_solo/utils.py:344-456
 *   /root/reference/src/ann_solo/spectrum_similarity.py:13-730
 * For every query i: the similarity features of (query i, library row lib_rows[i]) over
 * the peak matches pm_pairs[i, :pm_count[i]] that asl_search_batch / asl_rescore_* emit.
 * features[i, ASL_SSM_NFEAT], in the order of the reference's feature dictionary
 * (utils.py:309-342; `*_top` = restricted to the `top` = 5 most intense library peaks):
 *   0 cosine, 1 cosine_top, 2 n_matched_peaks, 3 frac_n_peaks_query, 4 frac_n_peaks_lib,
 *   5 frac_n_peaks_lib_top, 6 frac_int_query, 7 frac_int_lib, 8 frac_int_lib_top,
 *   9 mse_mz, 10 mse_mz_top, 11 mse_int, 12 mse_int_top, 13 contrast_angle,
 *   14 contrast_angle_top, 15 hypergeometric_score(min_mz, max_mz, bin_size), 16 kendalltau,
 *   17 ms_for_id_v1, 18 ms_for_id_v2, 19 entropy_unweighted, 20 entropy_weighted,
 *   21 scribe_fragment_acc, 22 scribe_fragment_acc_top, 23 manhattan, 24 euclidean,
 *   25 chebyshev, 26 pearsonr, 27 pearsonr_top, 28 spearmanr, 29 spearmanr_top,
 *   30 braycurtis, 31 canberra, 32 ruzicka.
 * Rows with lib_rows[i] < 0 are NaN (the reference skips SSMs without a match).
 * pm_count[i], for rows with a library row (the others are not read):
 *   - above pm_stride it is clipped to pm_stride (the row holds no more pairs);
 *   - negative: ASL_ERR_INVALID, as for a pair index beyond its spectrum;
 *   - the capacity is 256 peaks per spectrum and 256 pairs per SSM: more is ASL_ERR_CAPACITY.
 *     A matching uses every peak at most once, so it never has more pairs than min(nq, nl)
 *     peaks. A pair list that repeats peaks is evaluated as given (every pair counts, a peak
 *     is unmatched if no pair names it) while pairs + unmatched library peaks <= 256, beyond
 *     that it is ASL_ERR_CAPACITY too.
 * On an error the feature rows of the batch are unspecified. */
#define ASL_SSM_NFEAT 33
int asl_ssm_features_batch(const asl_peaks_t *queries, const asl_peaks_t *library,
                           const int32_t *lib_rows /* [nq] */,
                           const uint32_t *pm_pairs /* [nq, pm_stride, 2] */,
                           const int32_t *pm_count /* [nq] */, int32_t pm_stride,
                           double min_mz, double max_mz, double bin_size, int32_t top,
                           double *features /* [nq, ASL_SSM_NFEAT] */);

/* features[:, 0] alone -- the cosine over the peak matches (spectrum_similarity.py:81-106), the
 * cascade's default search-engine score (utils.py:407) -- with the same bits as column 0 of
 * asl_ssm_features_batch; rows with lib_rows[i] < 0 are NaN. pm_count[i] follows the same rule:
 * clipped to pm_stride, negative = ASL_ERR_INVALID; this entry stages nothing, so it has no
 * capacity (neither peaks nor pairs). */
int asl_ssm_cosine_batch(const asl_peaks_t *queries, const asl_peaks_t *library,
                         const int32_t *lib_rows /* [nq] */,
                         const uint32_t *pm_pairs /* [nq, pm_stride, 2] */,
                         const int32_t *pm_count /* [nq] */, int32_t pm_stride,
                         double *cosine /* [nq] */);

/* ------------------------------------------------------------------ SSM rescoring model
 * The model behind utils.score_ssms(model = 'svm') (/root/reference/src/ann_solo/utils.py:152-155: mokapot's
 * PercolatorModel, a LinearSVC(dual = False)): P L2-regularised squared-hinge linear SVMs over one feature
 * matrix, by a generalised Newton method with Armijo backtracking, all in fp64 (csrc/l2svm.hip). Per
 * iteration X is streamed twice (Newton pass, line pass), each row fetched once for all P problems; partial
 * sums are added in a fixed order, so two calls with the same inputs give the same bits. */
#define ASL_SVM_MAX_DIM      63   /* d; the bias makes D = d + 1 <= 64 */
#define ASL_SVM_MAX_PROBLEMS 32
typedef struct {
  double C;                   /* LinearSVC's C */
  double gtol_abs, gtol_rel;  /* stop when ||g||_2 <= max(gtol_abs, gtol_rel * ||g at the start||_2) */
  int32_t max_newton;         /* iteration cap per problem */
} asl_l2svm_params_t;
/* P problems over ONE matrix. label[p, i] in {+1, -1, 0}; 0 = row i is not part of problem p.
 * cw[p, 0] / cw[p, 1]: weight of the -1 / +1 class (sklearn's class_weight).
 * Minimises, per problem, over w in R^d and b:
 *   f = 0.5 * (w.w + b*b) + C * sum_i cw[p, cls(i)] * max(0, 1 - label[p,i] * (w.x_i + b))^2
 * This is LinearSVC(penalty='l2', loss='squared_hinge', dual=False, fit_intercept=True,
 * intercept_scaling=1): the bias is regularised. wb[p, 0..d) = w, wb[p, d] = b; read as the starting
 * point, written with the result. objective[p] = f at the result; n_newton[p] = steps taken.
 * Per step: g and H = I + 2 C sum cw x~x~^T over the rows with a positive margin deficit, H s = -g by
 * Cholesky on the host, then the first t in 1, 1/2 .. 2^-7 with f(w~ + t s) <= f(w~) + 1e-4 t g.s.
 * status[p]: 0 converged, 1 iteration cap, 2 line search stalled.
 * X, label: host or device memory, as the other entry points detect it; so are the small arrays.
 * Checked on the host before anything is launched or written: d > 63 or P > 32: ASL_ERR_CAPACITY;
 * d < 1, P < 1, n < 0, a label outside {-1, 0, +1}, a negative or non-finite class weight or C, a
 * negative or NaN tolerance or cap, a non-finite starting point: ASL_ERR_INVALID. A non-finite X is the
 * caller's precondition: it is not checked and gives non-finite results, never a fault. n = 0, a problem
 * whose labels are all 0 or of one class only are legal (no rows: w~ = 0, objective 0, status 0). */
int asl_l2svm_fit(const double *X /* [n, d] row-major */, int64_t n, int32_t d,
                  const int8_t *label /* [P, n] */, const double *cw /* [P, 2] */, int32_t P,
                  const asl_l2svm_params_t *params, double *wb /* [P, d + 1] */,
                  double *objective /* [P] */, int32_t *n_newton /* [P] */, int32_t *status /* [P] */);
/* out[p, i] = wb[p, 0..d) . x_i + wb[p, d]: the decision function of P models over X (X, wb, out: host
 * or device memory; the same limits on d, P and n) */
int asl_linear_scores(const double *X, int64_t n, int32_t d, const double *wb, int32_t P,
                      double *out /* [P, n] */);

/* ------------------------------------------------------------------ SSM rescoring model: forest
 * The model behind utils.score_ssms(model = 'rf'), restated as a HISTOGRAM forest (DESIGN.md 3 "Rescoring
 * model: forest"; csrc/forest.hip): every column of the matrix is a uint8 bin index, a split is (column, s)
 * with bins <= s going left, the criterion is Gini on class-weighted INTEGER counts, evaluated in fp64 in one
 * written order, and every random draw is a counter-based integer hash. Equal inputs give equal bits, and the
 * numpy restatement tests/forest_ref.py reproduces every node and every probability bit for bit. */
#define ASL_FOREST_MAX_BINS  256
#define ASL_FOREST_MAX_DEPTH 12
#define ASL_FOREST_MAX_TREES 1024
#define ASL_FOREST_NODES     8191 /* 2^(ASL_FOREST_MAX_DEPTH + 1) - 1: a complete heap, children 2i+1 / 2i+2 */
#define ASL_FOREST_ROW       64   /* bytes of a binned row (d <= ASL_SVM_MAX_DIM = 63: one row, one line) */
typedef struct {
  int32_t trees;      /* 1 .. ASL_FOREST_MAX_TREES */
  int32_t max_depth;  /* 1 .. ASL_FOREST_MAX_DEPTH: levels of splits; the leaves of a full tree are at this level */
  uint32_t seed;
} asl_forest_params_t;
/* P forests of `trees` heaps each; every array is [P, trees, ASL_FOREST_NODES], host or device memory.
 * col: the split column, -1 = a leaf or an absent node; bin: the split bin s (bins <= s go left);
 * n0 / n1: the node's in-bag count of the -1 / +1 class, with multiplicity; value = w1 / (w0 + w1) with
 * w_c = cw[p, c] * n_c (0.5 where w0 + w1 = 0), kept for internal nodes too: a forest grown to depth D and
 * read at depth d <= D IS the forest grown to depth d. */
typedef struct {
  int32_t trees, max_depth;   /* written by asl_forest_fit, read by asl_forest_predict */
  int16_t *col;
  uint8_t *bin;
  uint32_t *n0, *n1;
  double *value;
} asl_forest_model_t;
/* out[i, j] = the number of edges[j, 0 .. n_edges[j]) that are < X[i, j] (edges ascending), as a byte;
 * out is [n, ASL_FOREST_ROW], bytes d .. 63 of a row are 0. edges: [d, ASL_FOREST_MAX_BINS - 1] doubles.
 * d > 63: ASL_ERR_CAPACITY; d < 1, n < 0, an n_edges outside 0 .. 255: ASL_ERR_INVALID. */
int asl_forest_bin(const double *X /* [n, d] */, int64_t n, int32_t d, const double *edges,
                   const int32_t *n_edges /* [d] */, uint8_t *out /* [n, 64] */);
/* Grows P forests over ONE binned matrix. label[p, i] in {+1, -1, 0}; 0 = row i is not part of problem p.
 * cw[p, 0] / cw[p, 1]: weight of the -1 / +1 class. n_bins[j] (or NULL: 256 each): bins of column j.
 * Tree t draws n rows with replacement from all n rows (shared by the P problems) and, per node,
 * mtry = max(1, floor(sqrt(d))) distinct columns keyed by (seed, t, node); the best (column, bin) among them
 * maximises (wL1^2 + wL0^2) / wL + (wR1^2 + wR0^2) / wR, must exceed the node's (w1^2 + w0^2) / w strictly and
 * leave at least one in-bag row and a positive weight on either side; ties: the first drawn column, then the
 * lowest bin. A node of one class, or without such a split, is a leaf.
 * Checked on the host before anything is launched or written: d > 63, P > 32, max_depth > 12 or trees above
 * the cap: ASL_ERR_CAPACITY; d < 1, P < 1, n < 0 or n >= 2^31, trees < 1, max_depth < 1, a label outside
 * {-1, 0, +1}, a negative or non-finite class weight, an n_bins outside 1 .. 256 or a bin >= its column's
 * n_bins: ASL_ERR_INVALID. n = 0, a problem whose labels are all 0 or of one class only are legal: the root is
 * then a leaf, with value 0.5 for a problem without rows and 0 or 1 for a single class. */
int asl_forest_fit(const uint8_t *bins /* [n, 64] */, int64_t n, int32_t d, const int8_t *label /* [P, n] */,
                   const double *cw /* [P, 2] */, int32_t P, const int32_t *n_bins /* [d] or NULL */,
                   const asl_forest_params_t *params, asl_forest_model_t *model_out);
/* proba[p, i] = the mean over the trees of forest p, summed in tree order in fp64, of the value of the node
 * where row i stops when it walks at most max_depth levels (0 .. 12; may be lower than the grown depth). */
int asl_forest_predict(const uint8_t *bins /* [n, 64] */, int64_t n, int32_t d, const asl_forest_model_t *model,
                       int32_t P, int32_t max_depth, double *proba /* [P, n] */);
/* Bytes of device workspace one batch of (problem, tree) pairs may take while a level is grown (per pair: the
 * rows' node indices and the level's histograms); at least one pair always runs. Returns the previous value,
 * or a negative error for bytes <= 0. Default 2^31. The result does not depend on it. */
int64_t asl_set_forest_workspace(int64_t bytes);

/* ------------------------------------------------------------------ target-decoy q-values
 * The primitive of every FDR scorer (fdr.tdc_qvalues, fdr._grouped_q) on the device (csrc/tdc.hip; DESIGN.md 3
 * "Target-decoy q-values"). Within a group, walking the used rows from best to worst: FDR = (decoys so far + 1)
 * / targets so far, 1 while there is no target yet; rows of equal score (compared as doubles: -0.0 == +0.0) form
 * one run, which takes the FDR at its end, capped at 1; q = the smallest FDR of this run or any worse run.
 * Targets and decoys both get a q. The rows are ordered by an LSD radix sort of 8 bits a pass over the key
 * (group id with its sign bit flipped, order-preserving map of the score's bits) in tiles of ASL_TDC_TILE keys;
 * the counts are integer prefix sums, a run's end does one fp64 division, the rest is a min: equal inputs give
 * equal bytes, and the bytes are those of the numpy code. */
#define ASL_TDC_TILE 1024 /* keys per workgroup of a sort pass */
/* q[i] for every used row, by target-decoy competition inside the row's group
 * (fdr.tdc_qvalues per group = fdr._grouped_q).
 * Every array is host or device memory, as the other entry points detect it; q and label are written where
 * they live. Checked before q or label is written: n >= 2^31: ASL_ERR_CAPACITY (before any pointer is touched);
 * n < 0, desc outside {0, 1}, a NaN or negative fdr when label is given, a NaN score in a used row:
 * ASL_ERR_INVALID. Legal: n == 0 (launches nothing), +-inf scores, a NaN score in an unused row. */
int asl_tdc_qvalues(const double *score      /* [n] */,
                    const uint8_t *is_target /* [n], 0 / non-0 */,
                    const int32_t *group     /* [n] or NULL: one group; any int32 value is a group id */,
                    const uint8_t *use       /* [n] or NULL: all rows; rows with 0 take no part */,
                    int64_t n, int32_t desc  /* 1: a higher score is better; 0: lower */,
                    double fdr               /* read only when label is given */,
                    double *q                /* [n]; NaN for unused rows */,
                    int8_t *label            /* [n] or NULL: +1 used target with q <= fdr, 0 other used
                                                target and every unused row, -1 used decoy */);

/* ------------------------------------------------------------------ mass-difference groups
 * The group labels of the open level (fdr.ssm_groups = the reference's utils._get_ssm_groups, utils.py:204-274) on
 * the device (csrc/groups.hip; DESIGN.md 3 "Mass-difference groups"), byte for byte the host code's. The rule:
 *   - nominal = rint(md), half to even. The SSMs of one nominal value g form one interval.
 *   - Its 101 edges, as numpy.linspace(g - 0.5, g + 0.5, 101) forms them: edge[i] = fl(fl(i * 0.01) + (g - 0.5))
 *     for i < 100 -- a rounded product, then a rounded sum, never an FMA -- and edge[100] = g + 0.5.
 *   - An SSM is counted into the bin i with edge[i] <= md < edge[i + 1]; bin 99 also takes md == edge[100].
 *   - Peaks of the 100 counts (scipy.signal.find_peaks): a strict local maximum; a plateau counts once, at
 *     (first + last) / 2 rounded down; bins 0 and 99 are never peaks; a plateau that reaches bin 99 is no peak.
 *   - Bases of a peak (peak_prominences, wlen = None): walk outward from the peak while the count is <= the
 *     peak's count; the base is the position of the minimum met on the way, of equal minima the one nearest the
 *     peak, the peak itself if nothing lower is met.
 *   - An SSM belongs to the peak with the smallest |edge[peak] - md| (one rounded fp64 difference) among the peaks
 *     with edge[left base] < md < edge[right base], both strict; equal distances go to the lower peak index;
 *     with no such peak the SSM gets -1.
 *   - Group id = (number of peaks in all intervals of lower nominal value) + the peak's index in its interval.
 *   - The reference's quirks: the interval of the largest md is skipped (no peaks, no ids) when it holds exactly
 *     one SSM and n > 1; with n == 1 nothing is assigned.
 *   - Last, every id with fewer than min_group_size SSMs becomes -1. Ids are not renumbered.
 * Arrays are host or device memory, as the other entry points detect it; the outputs are written where they live.
 * peak_mass and peak_size are written for ids 0 .. *n_peaks - 1 only (an id's peak bin holds an SSM, so *n_peaks
 * <= n). Checked before any output is written: n < 0, min_group_size < 0, a non-finite md: ASL_ERR_INVALID;
 * n >= 2^31, or max nominal - min nominal + 1 > ASL_GROUPS_MAX_SPAN: ASL_ERR_CAPACITY (a +-500 Da window needs
 * 1 001 intervals). n == 0 is legal, launches nothing and sets both counts to 0. */
#define ASL_GROUPS_MAX_SPAN 65536 /* intervals between the smallest and the largest nominal mass difference */
int asl_ssm_groups(const double *mass_diff /* [n] */, int64_t n, int64_t min_group_size,
                   int32_t *group      /* [n] out */,
                   int64_t *n_peaks    /* out (host): number of group ids handed out, before folding */,
                   int64_t *n_labels   /* out (host): distinct values in group[], -1 included when present */,
                   double  *peak_mass  /* [n] or NULL: peak_mass[g] = left bin edge of group g's peak */,
                   int64_t *peak_size  /* [n] or NULL: peak_size[g] = SSMs assigned to g before folding */);

/* ------------------------------------------------------------------ MGF query files
 * A chunk of an MGF file, resident in device memory, parsed by kernels (csrc/mgf.hip; DESIGN.md 3 "Query files")
 * into the raw pack asl_process_batch takes. The dialect (what the reference's read_mgf reads through pyteomics'
 * mgf.MGF, restated; tests/mgf_ref.py is the same statement in Python):
 *   - Lines end at '\n'; a line is looked at without the blanks around it (space, \t, \n, \v, \f, \r). The last
 *     line need not end in '\n'.
 *   - Outside a block a line that is exactly BEGIN IONS opens one; every other line there is ignored.
 *   - Inside a block: an empty line or one whose first byte is one of # ; ! / is skipped; END IONS closes the
 *     block; a line with '=' is a parameter (key: the bytes before the first '=', ASCII lower-cased; value: the
 *     rest, stripped; the last duplicate wins); any other line is a peak line, split at blanks: m/z, intensity,
 *     further tokens unread.
 *   - Parameters read: title, else scan (the identifier); pepmass (its first token); charge (the first element of
 *     the list split at ',' or 'and': digits with the sign before or behind them); rtinseconds.
 *   - Structural errors: BEGIN IONS inside a block, a peak line of one token.
 * Numerals are converted on the device only where one correctly rounded fp64 operation is exact (asl_mgf_number
 * states the rule); every other token is DEFERRED: reported by byte range and destination, for the caller to
 * convert and store before asl_mgf_sort. Peaks are float32((double) numeral), in file order.
 * The calls go in this order: asl_mgf_measure(text) -- counts, errors, `consumed` --, asl_mgf_fill(the same text)
 * into arrays sized by those counts, then, the deferred values stored, asl_mgf_sort on the pack. The library keeps
 * what measure found until the next measure; a fill for another (text, n) is ASL_ERR_STATE. */
#define ASL_MGF_TILE 256       /* lines (and 16-byte spans of text) per workgroup of every scan level */
#define ASL_MGF_MAX_PEAKS 4096 /* peak lines of one spectrum: the limit of asl_process_batch */
#define ASL_MGF_MAX_LINE 65536 /* bytes of one line, its '\n' included: one thread walks a line */
/* counts[] of asl_mgf_measure */
#define ASL_MGF_N_LINES 0
#define ASL_MGF_N_SPECTRA 1       /* closed blocks */
#define ASL_MGF_N_PEAKS 2         /* two-token peak lines inside them */
#define ASL_MGF_N_DEFERRED 3      /* deferred tokens inside them */
#define ASL_MGF_CONSUMED 4        /* the byte behind the last closed block's END IONS line; 0 without one */
#define ASL_MGF_CONSUMED_LINES 5  /* the lines before that byte */
#define ASL_MGF_ERR_KIND 6        /* the first structural error: ASL_MGF_ERR_*, 0 = none */
#define ASL_MGF_ERR_LINE 7        /* its line, 0-based in the chunk; -1 = none */
#define ASL_MGF_OPEN 8            /* 1: the chunk ends inside a block (dropped by the caller at the file's end) */
#define ASL_MGF_COUNTS 9
#define ASL_MGF_ERR_NESTED 1      /* BEGIN IONS inside a block */
#define ASL_MGF_ERR_ONE_TOKEN 2   /* a peak line with one token */
/* destination kinds of a deferred token */
#define ASL_MGF_DEST_MZ 0         /* index: peak slot */
#define ASL_MGF_DEST_INTENSITY 1  /* index: peak slot */
#define ASL_MGF_DEST_PEPMASS 2    /* index: spectrum */
#define ASL_MGF_DEST_RT 3         /* index: spectrum */
#define ASL_MGF_DEST_NONE 4       /* a pepmass / rtinseconds line that a later duplicate overrides: unread */
/* text: [n] bytes in device memory; last != 0: the chunk ends the file. Then the lines of an unclosed last block
 * are checked too: its structural errors are reported and its deferred tokens listed (counted in
 * ASL_MGF_N_DEFERRED, with peak slots >= ASL_MGF_N_PEAKS: to be converted and refused or forgotten, never stored).
 * With last == 0 only lines before `consumed` are reported, the rest comes again with the next chunk, and a final
 * line that does not end in '\n' is not looked at, since it may be cut anywhere: it neither opens nor closes a block.
 * n >= 2^31: ASL_ERR_CAPACITY, before any pointer is touched; a line of more than ASL_MGF_MAX_LINE bytes anywhere
 * in the chunk (a file that is no text), or a closed block of more than ASL_MGF_MAX_PEAKS peak lines:
 * ASL_ERR_CAPACITY, whatever structural error the chunk also holds; n < 0, last outside {0, 1}, host memory:
 * ASL_ERR_INVALID. n == 0 is legal and launches nothing. counts: [ASL_MGF_COUNTS], host. */
int asl_mgf_measure(const uint8_t *text, int64_t n, int32_t last, int64_t *counts);
/* The measured chunk into caller-allocated arrays, host or device memory: the raw pack (the asl_peaks_t fields;
 * charge may be NULL, else it is zeroed), and per spectrum the precursor m/z (NaN: no pepmass line, or deferred),
 * the charge (0: no charge line; -1: outside 1 .. 255 or not a charge), the retention time (NaN: no rtinseconds
 * line, or deferred), the identifier's (offset, length) in the chunk (length -1: neither title nor scan) and the
 * block's BEGIN IONS line (0-based in the chunk). deferred: [n_deferred, 5] = (offset, length, destination kind,
 * destination index, line). An array of no elements may be NULL (with no closed block: all but offsets and,
 * where an unclosed last block has deferred tokens, deferred). */
int asl_mgf_fill(const uint8_t *text, int64_t n,
                 int32_t *offsets            /* [n_spectra + 1] */,
                 float *mz                   /* [n_peaks] */,
                 float *intensity            /* [n_peaks] */,
                 uint8_t *charge             /* [n_peaks] or NULL */,
                 double *precursor_mz        /* [n_spectra] */,
                 int32_t *precursor_charge   /* [n_spectra] */,
                 double *retention_time      /* [n_spectra] */,
                 int32_t *identifier         /* [n_spectra, 2] */,
                 int32_t *first_line         /* [n_spectra] */,
                 int32_t *deferred           /* [n_deferred, 5] */);
/* Every spectrum of the device-resident pack whose float32 m/z descend anywhere is sorted by m/z, stably (equal
 * m/z, -0.0 and +0.0 among them, keep file order): numpy.argsort(kind = 'stable') of library_store._sorted_peaks.
 * Spectra that ascend are not touched and launch nothing. *n_sorted (host, may be NULL): the spectra sorted.
 * A descending spectrum above ASL_MGF_MAX_PEAKS: ASL_ERR_CAPACITY; host memory: ASL_ERR_INVALID. */
int asl_mgf_sort(const int32_t *offsets, float *mz, float *intensity, int32_t n_spectra, int64_t n_peaks,
                 int64_t *n_sorted);
/* Host only: the numeral s[0 .. n) as the device converts it (csrc/mgf_number.hpp). Returns 0 and writes *out
 * where one correctly rounded fp64 operation gives float(s): [+-]? (digits [. digits*] | . digits) ([eE] [+-]?
 * digits)?, whose significand without leading zeros has at most 19 digits and is below 2^53, and whose decimal
 * exponent, counted from the last digit, lies in -22 .. 22 (a zero significand converts at any exponent). Returns
 * 1 (deferred, *out untouched) for every other byte string. */
int asl_mgf_number(const char *s, int32_t n, double *out);
/* asl_mgf_sort with the per-peak fragment charges as a third payload: charge [n_peaks], device memory, travels with
 * its peak. charge == NULL is asl_mgf_sort. */
int asl_mgf_sort_charged(const int32_t *offsets, float *mz, float *intensity, uint8_t *charge, int32_t n_spectra,
                         int64_t n_peaks, int64_t *n_sorted);

/* ------------------------------------------------------------------ Library files (.sptxt)
 * A chunk of a SpectraST .sptxt library, resident in device memory, parsed by kernels (csrc/sptxt.hip; DESIGN.md 3
 * "Library files") into the raw pack asl_process_batch takes, with the per-peak fragment charges. The dialect (the
 * well-formed subset of what the reference's sptxt reader accepts, restated; tests/sptxt_ref.py is the same
 * statement in Python):
 *   - Lines end at '\n'; a line is looked at without the blanks around it (space, \t, \n, \v, \f, \r), peak lines
 *     excepted. The last line need not end in '\n'. Keys are matched in any letter case.
 *   - A line whose head is `Name:` starts a record, which runs to the next such line or the end of the file; the
 *     lines before the first record are ignored. A `Name:` that is not preceded by a letter anywhere else in any
 *     line is refused (ERR_SECOND_NAME).
 *   - The identifier of a record is its ordinal in the file, from 1, as a decimal string.
 *   - Name line: the peptide is the text behind the last space before the first '/' (upper-case letters only), the
 *     precursor charge the text between that '/' and the next one or the line's end, stripped: digits only, 1 .. 255.
 *   - Metadata: the lines from the Name line to the `Num Peaks:` / `NumPeaks:` line (key, at most one blank, digits,
 *     nothing else: ERR_NUMPEAKS; the number is not read). Precursor m/z: the first line whose head is
 *     `PrecursorMZ:` (at most one blank, the numeral, nothing else: ERR_PRECURSOR), else the first `Parent=` of the
 *     first line that holds one (at most one blank, then the run of digits and points). The numeral is
 *     digits [. digits]. A `PrecursorMZ:` or `Num Peaks:` key that stands inside a metadata line, not at its
 *     head, is refused (ERR_STRAY_KEY): the reference's expressions would read it. is_decoy: `decoy` occurs in the Name line or in a metadata line that is no PrecursorMZ
 *     line. Modifications: the first `Mods=` of the first such line that holds one, up to the first blank.
 *   - Peaks: the lines behind the Num Peaks line (a second one in a record: ERR_SECOND_NUMPEAKS). A peak line is
 *     cut at the first '#', else loses its '\r' '\n' end; one that is then blank is skipped; the others are split at
 *     tabs: m/z and intensity (numerals, stripped), annotation (as it stands), further fields unread; fewer than three
 *     fields: ERR_FEW_FIELDS. Peaks are float32((double) numeral), in file order, deferred as in the MGF reader.
 *   - Fragment charge of a peak: asl_sptxt_fragment_charge of its annotation field.
 * Everything else a record must satisfy (a peptide, a charge, a precursor, one peak or more, well-formed Mods=) is
 * checked by the caller from the columns asl_sptxt_fill returns.
 * The calls go as for the MGF reader: asl_sptxt_measure(text), asl_sptxt_fill(the same text), the deferred values
 * stored, asl_mgf_sort_charged on the pack. A record is closed by the next Name line, or by the end of the chunk when
 * last != 0; with last == 0 the lines from the last Name line on are neither reported nor checked: they come again. */
/* counts[] of asl_sptxt_measure */
#define ASL_SPTXT_N_LINES 0
#define ASL_SPTXT_N_RECORDS 1       /* closed records */
#define ASL_SPTXT_N_PEAKS 2         /* peak lines inside them */
#define ASL_SPTXT_N_DEFERRED 3      /* deferred tokens inside them */
#define ASL_SPTXT_CONSUMED 4        /* the byte at which the first record that is not closed starts; n with last != 0;
                                       0 without a Name line */
#define ASL_SPTXT_CONSUMED_LINES 5  /* the lines checked: those before that byte; all of them without a Name line */
#define ASL_SPTXT_ERR_KIND 6        /* the first structural error: ASL_SPTXT_ERR_*, 0 = none */
#define ASL_SPTXT_ERR_LINE 7        /* its line, 0-based in the chunk; -1 = none */
#define ASL_SPTXT_OPEN 8            /* 1: the chunk ends inside a record */
#define ASL_SPTXT_COUNTS 9
#define ASL_SPTXT_ERR_SECOND_NAME 1
#define ASL_SPTXT_ERR_SECOND_NUMPEAKS 2
#define ASL_SPTXT_ERR_NUMPEAKS 3
#define ASL_SPTXT_ERR_FEW_FIELDS 4
#define ASL_SPTXT_ERR_PRECURSOR 5
#define ASL_SPTXT_ERR_STRAY_KEY 6
/* destination kinds of a deferred token */
#define ASL_SPTXT_DEST_MZ 0         /* index: peak slot */
#define ASL_SPTXT_DEST_INTENSITY 1  /* index: peak slot */
#define ASL_SPTXT_DEST_PRECURSOR 2  /* index: record */
#define ASL_SPTXT_DEST_NONE 3       /* a precursor numeral on a line that does not decide the precursor: unread */
/* info[] of a record */
#define ASL_SPTXT_INFO 8            /* precursor charge (-1: not 1 .. 255, or no '/'), precursor status, is_decoy,
                                       peptide offset and length (-1: no '/'), Mods= offset and length (-1: none; the
                                       range starts at the key), Name line (0-based in the chunk) */
#define ASL_SPTXT_PRECURSOR_OK 0      /* converted, or deferred (then precursor_mz is NaN and the token is listed) */
#define ASL_SPTXT_PRECURSOR_MISSING 1 /* neither a PrecursorMZ line nor a Parent= */
#define ASL_SPTXT_PRECURSOR_BAD 2     /* the Parent= numeral is not digits [. digits] */
/* As asl_mgf_measure: n >= 2^31, a line above ASL_MGF_MAX_LINE bytes or a closed record above ASL_MGF_MAX_PEAKS peak
 * lines: ASL_ERR_CAPACITY; n == 0 is legal and launches nothing. counts: [ASL_SPTXT_COUNTS], host. */
int asl_sptxt_measure(const uint8_t *text, int64_t n, int32_t last, int64_t *counts);
/* The measured chunk into caller-allocated arrays, host or device memory. precursor_mz: NaN where missing, bad or
 * deferred. deferred: [n_deferred, 5] = (offset, length, destination kind, destination index, line). */
int asl_sptxt_fill(const uint8_t *text, int64_t n,
                   int32_t *offsets            /* [n_records + 1] */,
                   float *mz                   /* [n_peaks] */,
                   float *intensity            /* [n_peaks] */,
                   uint8_t *charge             /* [n_peaks] */,
                   double *precursor_mz        /* [n_records] */,
                   int32_t *info               /* [n_records, ASL_SPTXT_INFO] */,
                   int32_t *deferred           /* [n_deferred, 5] */);
/* Host only: the fragment charge of the annotation s[0 .. n) as the device reads it (csrc/sptxt_annot.hpp). 0 for an
 * empty field or a first byte other than a b y p; else the leading digits behind the first '^' that stands before
 * the first '/', at most 255, and 1 without a '^' or without digits behind it. */
int asl_sptxt_fragment_charge(const char *s, int32_t n);

/* ------------------------------------------------------------------ mzML query files
 * A chunk of an mzML file, resident in device memory, parsed and decoded by kernels (csrc/mzml.hip, csrc/inflate.hpp;
 * DESIGN.md 3 "Query files") into the raw pack asl_process_batch takes. The dialect (what the reference's read_mzml
 * reads through pyteomics' mzml.MzML, restated; tests/mzml_ref.py is the same statement in Python):
 *   - The text is a sequence of tags, each starting at a '<' and ending at the first '>' outside quotes (" or ');
 *     newlines mean nothing. A tag of more than ASL_MZML_MAX_TAG bytes: ASL_ERR_CAPACITY. The content of <binary>
 *     runs from its '>' to the next '<'.
 *   - Every <spectrum> element has the 0-based ordinal `index`, whatever its MS level. Only spectra with a cvParam
 *     MS:1000511 of value "2" directly below <spectrum> are read; the others cost the tag pass alone. A
 *     <spectrum> inside a <spectrum>: ASL_MZML_ERR_NESTED.
 *   - Retention time: MS:1000016 in the first <scan>, value as written. Precursor m/z: MS:1000744 in the first
 *     <selectedIon> of the first <precursor>; charge: MS:1000041 there (digits, 1 .. 255), else exactly one
 *     MS:1000633, else unknown (0). Of a duplicated parameter the first wins. Numerals are converted as the MGF
 *     reader's (asl_mgf_number), or deferred: their byte ranges are handed back.
 *   - Arrays: the first <binaryDataArray> with MS:1000514 is m/z, the first with MS:1000515 intensity; precision
 *     MS:1000523 (64-bit float) or MS:1000521 (32-bit float); compression MS:1000576 (none) or MS:1000574 (zlib).
 *     Each holds exactly defaultArrayLength values; they become float32 by round-to-nearest, in file order.
 *     Base64: the standard alphabet, '=' padding, blanks skipped. zlib: RFC 1950 (CM = 8, window <= 32 KiB,
 *     FCHECK, no FDICT) around RFC 1951 (stored, fixed and dynamic blocks), Adler-32 verified; the stream of an
 *     array of b bytes is at most b + b / 8 + 64 bytes long.
 *   - Refused, per spectrum (ASL_MZML_E_*) or per array (ASL_MZML_INF_*): any other precision or compression
 *     accession (integers, Numpress), a missing one, an arrayLength attribute, a <referenceableParamGroupRef>, a
 *     missing array, scan start time or selected ion m/z, several MS:1000633 without a MS:1000041, a charge or a
 *     defaultArrayLength that is not plain digits, and everything the decoders refuse. A comment or a CDATA section
 *     after the first <spectrum is the structural error ASL_MZML_ERR_COMMENT.
 * The calls go as for the MGF reader: asl_mzml_measure(text), asl_mzml_fill(the same text), the deferred numerals
 * stored, asl_mgf_sort on the pack. A record is <spectrum ...> ... </spectrum>. */
#define ASL_MZML_MAX_TAG 4096       /* bytes of one tag, '<' to '>': one thread walks a tag */
#define ASL_MZML_SMALL_PEAKS 512    /* arrays up to this many values are decoded by the small-window kernel */
/* counts[] of asl_mzml_measure: ASL_MGF_N_LINES (tags) .. ASL_MGF_OPEN as for the MGF reader (N_SPECTRA: the closed
 * MS2 spectra; N_DEFERRED: 0), and */
#define ASL_MZML_N_ELEMENTS 9       /* closed <spectrum> elements of every MS level */
#define ASL_MZML_ERR_ELEMENT 10     /* <spectrum> elements of the chunk opened up to the structural error's tag */
#define ASL_MZML_COUNTS 11
#define ASL_MZML_ERR_NESTED 1       /* <spectrum> inside a <spectrum> */
#define ASL_MZML_ERR_COMMENT 2      /* a comment or CDATA section after the first <spectrum */
#define ASL_MZML_ERR_TAG 3          /* a tag inside a spectrum that the next '<' or the file's end cuts */
/* errors[] of asl_mzml_fill, per spectrum. What fails while the reference iterates over the file ... */
#define ASL_MZML_E_LENGTH 0x1       /* defaultArrayLength missing or not digits */
#define ASL_MZML_E_NO_MZ 0x2        /* no m/z array, or one without <binary> */
#define ASL_MZML_E_NO_INTENSITY 0x4
#define ASL_MZML_E_PRECISION 0x8    /* missing or unsupported, on either array */
#define ASL_MZML_E_COMPRESSION 0x10
#define ASL_MZML_E_ARRAY_LENGTH 0x20 /* an arrayLength attribute on a <binaryDataArray> */
#define ASL_MZML_E_PARAM_GROUP 0x40 /* <referenceableParamGroupRef> */
#define ASL_MZML_E_FILE 0x7f
/* ... and what fails after the identifier is read (a spectrum the identifier rule drops never gets here) */
#define ASL_MZML_E_NO_RT 0x100
#define ASL_MZML_E_NO_PRECURSOR 0x200
#define ASL_MZML_E_CHARGES 0x400    /* several MS:1000633 without a MS:1000041 */
#define ASL_MZML_E_CHARGE 0x800     /* a charge that is not digits in 1 .. 255 */
/* flags[] of asl_mzml_fill, per spectrum */
#define ASL_MZML_F_MZ_ZLIB 0x1
#define ASL_MZML_F_MZ_F64 0x2
#define ASL_MZML_F_INTENSITY_ZLIB 0x4
#define ASL_MZML_F_INTENSITY_F64 0x8
/* text: device memory, n bytes. last: bit 0: the chunk ends the file; bit 1: a <spectrum was seen before this chunk
 * (a comment anywhere in it is refused). Errors as asl_mgf_measure, with ASL_MZML_MAX_TAG for ASL_MGF_MAX_LINE and
 * defaultArrayLength for the peak lines. counts: [ASL_MZML_COUNTS], host. */
int asl_mzml_measure(const uint8_t *text, int64_t n, int32_t last, int64_t *counts);
/* The measured chunk into caller-allocated arrays, host or device memory; per MS2 spectrum s. identifier: the byte
 * range (offset, length) of the id attribute's value, length -1 without one. element: the ordinal of the spectrum
 * among the chunk's <spectrum> elements. numerals: (offset, length) of the scan start time's and of the selected
 * ion m/z's value where the device deferred it (then the column holds NaN), length -1 elsewhere. array_errors:
 * ASL_MZML_INF_* (csrc/inflate.hpp) of the m/z and of the intensity array, 0: decoded. A spectrum with errors[s] != 0
 * or an array error has undefined peaks: the caller refuses it. The arrays are decoded by one thread each over global scratch
 * (34 bytes a peak and 1.4 KiB an array, kept by the library); ASL_MZML_DECODE=wave in the environment decodes with
 * one wavefront per array over LDS instead: the same core, the same bytes and error codes, measured slower
 * (profiles/mzml_cost.json). */
int asl_mzml_fill(const uint8_t *text, int64_t n,
                  int32_t *offsets            /* [n_spectra + 1] */,
                  float *mz                   /* [n_peaks] */,
                  float *intensity            /* [n_peaks] */,
                  uint8_t *charge             /* [n_peaks], zeros */,
                  double *precursor_mz        /* [n_spectra] */,
                  int32_t *precursor_charge   /* [n_spectra], 0: unknown */,
                  double *retention_time      /* [n_spectra] */,
                  int32_t *identifier         /* [n_spectra, 2] */,
                  int32_t *first_tag          /* [n_spectra] */,
                  int32_t *element            /* [n_spectra] */,
                  int32_t *numerals           /* [n_spectra, 4] */,
                  int32_t *errors             /* [n_spectra] */,
                  int32_t *flags              /* [n_spectra] */,
                  int32_t *array_errors       /* [n_spectra, 2] */);
/* Host only: the decoder core of csrc/inflate.hpp as the device runs it, over one array's characters b64[0 .. n):
 * base64, then zlib where zlib_flag != 0. out: [cap]; *n_out: the bytes written. Returns 0 or ASL_MZML_INF_*
 * (1 bad byte, 2 length, 3 padding, 4 input too long, 5 zlib header, 6 block type, 7 stored lengths, 8 code
 * lengths, 9 invalid symbol, 10 distance too far back, 11 truncated, 12 more than cap bytes, 13 Adler-32,
 * 14 fewer bytes than expected), -1 for a null argument. */
int asl_mzml_inflate(const uint8_t *b64, int64_t n, int32_t zlib_flag, uint8_t *out, int64_t cap, int64_t *n_out);

/* ------------------------------------------------------------------ mzXML query files
 * A chunk of an mzXML file, resident in device memory, parsed and decoded by kernels (csrc/mzxml.hip, on the tag
 * helpers of csrc/xml_tag.hpp and the decoder of csrc/inflate.hpp; DESIGN.md 3 "Query files") into the raw pack
 * asl_process_batch takes. The dialect (what the reference's read_mzxml reads through pyteomics' mzxml.MzXML,
 * restated; tests/mzxml_ref.py is the same statement in Python):
 *   - Tags as for mzML: each from a '<' to the first '>' outside quotes, newlines mean nothing, a tag of more than
 *     ASL_MZML_MAX_TAG bytes: ASL_ERR_CAPACITY. A comment or CDATA section after the first <scan is the structural
 *     error ASL_MZXML_ERR_COMMENT; the schema's <comment> element is an ordinary ignored tag. The reader is NOT an
 *     XML validator: well-formedness beyond what is listed here is not checked.
 *   - Every <scan opening tag has the 0-based ordinal `index` among all <scan opening tags in document order,
 *     whatever its MS level or nesting depth. A scan's HEAD is the run of tags from its opening tag to the next
 *     <scan or </scan> tag (the schema puts precursorMz and peaks before child scans, so every tag a scan owns lies
 *     in its head); a self-closing <scan .../> is a head with nothing in it. A <precursorMz or <peaks tag outside
 *     any head: ASL_MZXML_ERR_OUTSIDE. The record of the chunk protocol is the head: it is closed once a complete
 *     <scan or </scan> tag follows it, so a chunk may end inside a scan whose children are still to come.
 *   - Only scans whose msLevel attribute is the digits "2" are read; a missing msLevel is skipped; other levels cost
 *     the tag pass alone, their <peaks> are never decoded (a corrupt MS1 array goes unnoticed). An msLevel that is
 *     not plain digits: ASL_MZXML_ERR_LEVEL.
 *   - Identifier: the value of num, handed to the host as a byte range (Python's int() is applied there).
 *   - Retention time: retentionTime, in minutes. "PT<seconds>S" with <seconds> = digits [. digits*] is converted as
 *     seconds / 60.0, one fp64 division behind asl_mgf_number; a value that does not begin with 'P' is the numeral
 *     as written; everything else (hours, minutes, a date part, a numeral the converter defers) is handed back as a
 *     byte range. asl_mzxml_duration is the same function on the host.
 *   - Precursor m/z: the text of the first <precursorMz> of the head, from its '>' to the next '<', blanks stripped,
 *     converted by asl_mgf_number or deferred; charge: its precursorCharge attribute (digits, 1 .. 255), absent:
 *     unknown (0).
 *   - Peaks: peaksCount on the scan (digits; above ASL_MGF_MAX_PEAKS: ASL_ERR_CAPACITY); the first <peaks> of the
 *     head, a second one is refused; precision "32" or "64"; byteOrder, where present, "network"; contentType or
 *     pairOrder, where present, "m/z-int"; compressionType absent, "none" or "zlib"; compressedLen is ignored. The
 *     content runs from '>' to the next '<'; base64 and zlib exactly as for mzML (above); the decoded stream is
 *     exactly peaksCount * 2 * precision / 8 bytes, and a compressed stream for b such bytes at most b + b / 8 + 64
 *     bytes long. peaksCount = 0 with no characters is an empty spectrum, whatever the compression. Values are
 *     big-endian, m/z every even element and intensity every odd one; 64-bit values become float32 by
 *     round-to-nearest (asl_mzxml_pairs is the same function on the host).
 * The calls go as for the mzML reader: asl_mzxml_measure(text), asl_mzxml_fill(the same text), the deferred values
 * stored, asl_mgf_sort on the pack. */
/* counts[] of asl_mzxml_measure: ASL_MGF_N_LINES (tags) .. ASL_MGF_OPEN as for the MGF reader (N_SPECTRA: the MS2
 * scans whose head is closed; N_DEFERRED: 0), and */
#define ASL_MZXML_N_ELEMENTS 9      /* <scan opening tags of every MS level whose head is closed */
#define ASL_MZXML_ERR_ELEMENT 10    /* <scan opening tags of the chunk up to the structural error's tag */
#define ASL_MZXML_DEPTH_ALL 11      /* <scan> elements open behind the chunk's last tag ... */
#define ASL_MZXML_DEPTH_CONSUMED 12 /* ... and behind tag ASL_MGF_CONSUMED_LINES - 1 */
#define ASL_MZXML_COUNTS 13
#define ASL_MZXML_ERR_OUTSIDE 1     /* <precursorMz or <peaks outside any scan's head */
#define ASL_MZXML_ERR_COMMENT 2     /* a comment or CDATA section after the first <scan */
#define ASL_MZXML_ERR_TAG 3         /* a tag after the first <scan that the next '<' or the file's end cuts */
#define ASL_MZXML_ERR_LEVEL 4       /* an msLevel that is not plain digits, on a scan of any level */
/* errors[] of asl_mzxml_fill, per MS2 scan. What fails while the reference iterates over the file (with a scan
 * without num, and with array_errors) ... */
#define ASL_MZXML_E_COUNT 0x1       /* peaksCount missing or not digits */
#define ASL_MZXML_E_NO_PEAKS 0x2    /* no <peaks> in the head */
#define ASL_MZXML_E_PEAKS_TWICE 0x4 /* more than one <peaks> in the head */
#define ASL_MZXML_E_PRECISION 0x8   /* missing, or neither 32 nor 64 */
#define ASL_MZXML_E_BYTE_ORDER 0x10 /* byteOrder other than network */
#define ASL_MZXML_E_CONTENT_TYPE 0x20 /* contentType or pairOrder other than m/z-int */
#define ASL_MZXML_E_COMPRESSION 0x40 /* compressionType other than none or zlib */
#define ASL_MZXML_E_FILE 0x7f
/* ... and what fails after the identifier is read (a scan the identifier rule drops never gets here) */
#define ASL_MZXML_E_NO_RT 0x100     /* no retentionTime attribute */
#define ASL_MZXML_E_NO_PRECURSOR 0x200 /* no <precursorMz> in the head */
#define ASL_MZXML_E_CHARGE 0x400    /* a precursorCharge that is not digits in 1 .. 255 */
/* flags[] of asl_mzxml_fill, per MS2 scan */
#define ASL_MZXML_F_ZLIB 0x1
#define ASL_MZXML_F_F64 0x2
#define ASL_MZXML_F_NESTED 0x4      /* the head opened inside another scan's element */
/* text: device memory, n bytes. last: bit 0: the chunk ends the file; bit 1: a <scan was seen before this chunk;
 * bits 8 .. 15: the <scan> elements open in front of the chunk (at most 255; only ASL_MZXML_F_NESTED and the two
 * depth counts depend on it). Errors as asl_mzml_measure, with peaksCount for defaultArrayLength.
 * counts: [ASL_MZXML_COUNTS], host. */
int asl_mzxml_measure(const uint8_t *text, int64_t n, int32_t last, int64_t *counts);
/* The measured chunk into caller-allocated arrays, host or device memory; per MS2 scan s. identifier: the byte
 * range (offset, length) of num's value, length -1 without one. element: the ordinal of the scan among the chunk's
 * <scan opening tags. numerals: (offset, length) of retentionTime's value and of the precursor m/z's text where
 * the device deferred it (then the column holds NaN), length -1 elsewhere. array_errors: ASL_MZML_INF_* of the
 * scan's one stream, 0: decoded. A scan with errors[s] != 0 or an array error has undefined peaks: the caller
 * refuses it. One thread decodes one stream over windows in global scratch that the library keeps (34 bytes a peak
 * and 1.4 KiB a scan): the raw window of a scan is up to ASL_MGF_MAX_PEAKS * 16 bytes = 64 KiB, twice DEFLATE's
 * largest distance, and serves the inflater as its history. */
int asl_mzxml_fill(const uint8_t *text, int64_t n,
                   int32_t *offsets            /* [n_spectra + 1] */,
                   float *mz                   /* [n_peaks] */,
                   float *intensity            /* [n_peaks] */,
                   uint8_t *charge             /* [n_peaks], zeros */,
                   double *precursor_mz        /* [n_spectra] */,
                   int32_t *precursor_charge   /* [n_spectra], 0: unknown */,
                   double *retention_time      /* [n_spectra], minutes */,
                   int32_t *identifier         /* [n_spectra, 2] */,
                   int32_t *first_tag          /* [n_spectra] */,
                   int32_t *element            /* [n_spectra] */,
                   int32_t *numerals           /* [n_spectra, 4] */,
                   int32_t *errors             /* [n_spectra] */,
                   int32_t *flags              /* [n_spectra] */,
                   int32_t *array_errors       /* [n_spectra] */);
/* Host only: the value s[0 .. n) of a retentionTime attribute as the device converts it (csrc/mzxml_value.hpp).
 * 0: *minutes written; 1: deferred to the caller's full rule, *minutes untouched. */
int asl_mzxml_duration(const char *s, int32_t n, double *minutes);
/* Host only: a decoded <peaks> stream raw[0 .. n_peaks * 2 * precision / 8) as the device converts it: big-endian
 * (m/z, intensity) pairs into mz[n_peaks] and intensity[n_peaks]. precision: 32 or 64. Returns 0, or -1 for a null
 * argument, a negative n_peaks or another precision. */
int asl_mzxml_pairs(const uint8_t *raw, int32_t n_peaks, int32_t precision, float *mz, float *intensity);

/* ------------------------------------------------------------------ hot path
 * One batch of same-charge queries through
 *   SpectralLibrary._search_batch / _get_library_candidates
 *   (src/ann_solo/spectral_library.py:328-455)
 * entirely on the device: encode -> index.search(k) -> precursor-window
 * post-filter (:417-429,:441-446) -> best match per query (:356-365).
 * A library handle keeps the packed peak store resident in HBM. */
typedef struct asl_library asl_library_t;
/* lib_pmz_f32: spec_info's float32 precursor m/z column (reader.py:184-191), may be
 * NULL (then (float)precursor_mz). valid: per-spectrum is_valid flag or NULL. */
asl_library_t *asl_library_create(const asl_peaks_t *library, const float *lib_pmz_f32,
                                  const uint8_t *valid);
void asl_library_free(asl_library_t *lib);
int64_t asl_library_size(const asl_library_t *lib);
/* The group column of a library handle (asl_*_topn_distinct): group[n], one 32-bit id per row, host
 * or device memory, n == asl_library_size(lib) (anything else: ASL_ERR_INVALID). The ids are copied
 * to the device; the array is the caller's again on return. group == NULL drops the column (n is
 * ignored). Setting it again replaces it. No other entry point reads it. */
int asl_library_set_groups(asl_library_t *lib, int64_t n, const int32_t *group);
/* Search a subset of the library: keep[n], keep[row] != 0 = selected, host or device memory, n ==
 * asl_library_size(lib) (anything else: ASL_ERR_INVALID); copied, the array is the caller's again on return.
 * n == 0 or keep == NULL drops the selection. Waits for pipelined batches in flight. While a selection is
 * installed every result of asl_search_batch / _topn / _topn_distinct, synchronous or pipelined, is what the
 * same call would return if the unselected rows were invalid library rows (never a candidate) AND the ANN index
 * held, in the same lists with the same centroids, codebooks and codes, only the selected vectors: the scans
 * choose their k among the selected vectors of the probed lists (as asl_index_search_selected), then the
 * precursor window applies as configured (asl_set_scan_postfilter, asl_index_set_window_scan); use_ann = 0
 * walks the selected rows of the window at any pair budget; asl_rescore_knn* drop an unselected row among the
 * caller's ids. Row numbers and score bits do not change. The selection has a generation number beside the
 * library's serial: an index notices a replaced or dropped selection as it notices another library, and
 * rebuilds what it derived (selector words, post-filter pairs, window-ordered layout). Where the index cannot
 * select inside its scan (the cases asl_index_search_selected lists) the fused calls return its
 * ASL_ERR_STATE. Without a selection every call runs the kernels and launches it ran before; dropping one
 * restores those results bit for bit. The selector of asl_index_set_selector plays no part in the fused calls. */
int asl_library_set_selection(asl_library_t *lib, int64_t n, const uint8_t *keep);

typedef struct {
  double min_bound, bin_size; /* encoder grid (get_dim) */
  uint32_t hash_seed;         /* 42 */
  int32_t k;                  /* config.num_candidates */
  int32_t nprobe;             /* config.num_probe */
  int32_t charge;             /* precursor charge of this batch */
  double precursor_tol;       /* config.precursor_tolerance_mass(_open) */
  int32_t precursor_mode;     /* ASL_TOL_DA / ASL_TOL_PPM / ASL_TOL_INTERVAL */
  double fragment_mz_tolerance; /* Da, or ppm of the query peak with ASL_SCORE_FRAGMENT_PPM */
  int32_t allow_shift;        /* flag word: ASL_SCORE_SHIFT (config.allow_peak_shifts) | ASL_SCORE_FRAGMENT_PPM */
  int32_t use_ann;            /* 1: ANN top-k AND window (open+ann); 0: window only (std / bf) */
  /* The queries' intervals, [nq, 2] (lo, hi), host or device memory: read only when precursor_mode ==
   * ASL_TOL_INTERVAL (NULL is then ASL_ERR_INVALID; precursor_tol is unread). A host array is copied before
   * the call returns, by a pipelined asl_search_batch too -- which for that copy waits on the host until the
   * batch before the previous one has been rescored (the copy goes into that batch's buffer), so part of
   * the pipeline's overlap is lost: pass device arrays to pipelined calls. A device array must stay as it
   * is for as long as the queries' arrays. The member was added behind the older ones: a caller compiled against the struct
   * without it never sets ASL_TOL_INTERVAL, so it is never read for that caller. Honoured by
   * asl_search_batch / _topn / _topn_distinct and asl_rescore_knn*, in every mode they have. */
  const double *precursor_window;
} asl_search_params_t;

/* Outputs, each [nq] (NULL to skip): best_row = library row of the best match
 * (-1: no candidate), best_score, n_cand = candidates that reached rescoring,
 * pm_count / pm_pairs as in asl_rescore_batch; knn_I [nq,k] = raw ANN ids. */
int asl_search_batch(asl_library_t *lib, asl_index_t *idx, const asl_peaks_t *queries,
                     const asl_search_params_t *params, int32_t *best_row,
                     double *best_score, int32_t *n_cand, int32_t *pm_count,
                     uint32_t *pm_pairs, int32_t pm_stride, int64_t *knn_I);

/* Same pipeline from the post-filter on, for candidates retrieved elsewhere (the
 * multi-GPU path: per-shard top-k lists are exchanged and merged first). knn_I is
 * [nq, k] int64 library rows, -1 padded, as asl_index_search / asl_topk_merge emit. */
int asl_rescore_knn(asl_library_t *lib, const asl_peaks_t *queries,
                    const asl_search_params_t *params, const int64_t *knn_I,
                    int32_t *best_row, double *best_score, int32_t *n_cand,
                    int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride);

/* asl_search_batch for the n best library matches of every query, 1 <= n_best <= ASL_MAX_BEST
 * (anything else: ASL_ERR_INVALID): best_row / best_score / pm_count are [nq, n_best], pm_pairs is
 * [nq, n_best, pm_stride, 2], n_cand [nq] and knn_I [nq, k] as in asl_search_batch. Ranks are ordered
 * by score descending, equal scores by the lower library row; ranks beyond the query's candidates
 * hold row -1, score 0.0, count 0 and zero pairs. Column 0 of every output, n_cand and knn_I equal
 * asl_search_batch's outputs bit for bit. Every mode of asl_search_batch is covered: use_ann = 1 on any
 * index kind, with the scan-side post-filter on or off and in window-scan mode, and use_ann = 0 at
 * any pair budget (each tile's n best are folded into a running n best per query on the device).
 * NOT pipelined: like every entry point other than asl_search_batch the call first waits for the
 * batches of asl_set_pipeline in flight, then runs on the library's stream and returns when its
 * outputs are written. */
int asl_search_batch_topn(asl_library_t *lib, asl_index_t *idx, const asl_peaks_t *queries,
                          const asl_search_params_t *params, int32_t n_best, int32_t *best_row,
                          double *best_score, int32_t *n_cand, int32_t *pm_count,
                          uint32_t *pm_pairs, int32_t pm_stride, int64_t *knn_I);

/* asl_rescore_knn for the n best matches: outputs as in asl_search_batch_topn (equal to it when
 * knn_I holds the ids it searched). An id that knn_I names twice is two candidates. */
int asl_rescore_knn_topn(asl_library_t *lib, const asl_peaks_t *queries,
                         const asl_search_params_t *params, const int64_t *knn_I, int32_t n_best,
                         int32_t *best_row, double *best_score, int32_t *n_cand,
                         int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride);

/* asl_search_batch_topn / asl_rescore_knn_topn with DISTINCT ranks (asl_rescore_batch_topn_distinct's
 * rule, ties to the lower library row): same arguments, same output shapes, the groups are the
 * library handle's column (asl_library_set_groups). Without a column: ASL_ERR_STATE, never a silent
 * fall-back to the plain ranks. Column 0 of every output, n_cand and knn_I equal asl_search_batch's
 * bit for bit; the ranks below name the best row of the next groups, -1 / 0.0 / 0 / zero pairs beyond
 * the last one. Every mode asl_search_batch_topn covers, use_ann = 0 at any pair budget included
 * (each tile's distinct ranks are folded into the running ones, skipping groups already held).
 * Synchronous and not pipelined, like the plain calls. */
int asl_search_batch_topn_distinct(asl_library_t *lib, asl_index_t *idx, const asl_peaks_t *queries,
                                   const asl_search_params_t *params, int32_t n_best,
                                   int32_t *best_row, double *best_score, int32_t *n_cand,
                                   int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride,
                                   int64_t *knn_I);
int asl_rescore_knn_topn_distinct(asl_library_t *lib, const asl_peaks_t *queries,
                                  const asl_search_params_t *params, const int64_t *knn_I,
                                  int32_t n_best, int32_t *best_row, double *best_score,
                                  int32_t *n_cand, int32_t *pm_count, uint32_t *pm_pairs,
                                  int32_t pm_stride);

/* asl_search_batch_topn / asl_rescore_knn_topn (distinct == 0) or their _distinct forms (distinct != 0;
 * without a group column: ASL_ERR_STATE) with the score histogram of asl_rescore_batch_topn_hist:
 * score_hist [nq, ASL_SCORE_HIST_BINS], host or device, sum(score_hist[q]) == n_cand[q]. NULL: exactly
 * the plain calls, launch for launch; with the pointer set every other output is unchanged. Every mode
 * of asl_search_batch_topn is covered: any index kind, the scan-side post-filter on or off, the window
 * scan, use_ann = 0 at any pair budget (every tile's pass adds its part of a query's window into the
 * query's row; the final pass over the running winners counts nothing), a library selection,
 * ASL_TOL_INTERVAL and ASL_SCORE_FRAGMENT_PPM. n_best = 1 is the single winner (column 0 equals
 * asl_search_batch's outputs). Synchronous and not pipelined, same argument contract as the plain calls. */
int asl_search_batch_topn_hist(asl_library_t *lib, asl_index_t *idx, const asl_peaks_t *queries,
                               const asl_search_params_t *params, int32_t n_best, int32_t distinct,
                               int32_t *best_row, double *best_score, int32_t *n_cand,
                               int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride,
                               int64_t *knn_I, int32_t *score_hist);
int asl_rescore_knn_topn_hist(asl_library_t *lib, const asl_peaks_t *queries,
                              const asl_search_params_t *params, const int64_t *knn_I,
                              int32_t n_best, int32_t distinct, int32_t *best_row, double *best_score,
                              int32_t *n_cand, int32_t *pm_count, uint32_t *pm_pairs,
                              int32_t pm_stride, int32_t *score_hist);

/* Precursor-window candidate generation alone (spectral_library.py:417-429):
 * CSR lists of library rows (ascending) whose precursor passes the window. Two-call
 * protocol: first with cand_rows == NULL to get cand_offsets[nq+1], then with a
 * buffer of cand_offsets[nq] entries. mode == ASL_TOL_INTERVAL: query_pmz is [nq, 2]. */
int asl_window_candidates(asl_library_t *lib, int32_t nq, const double *query_pmz,
                          int32_t charge, double tol, int32_t mode, int32_t *cand_offsets,
                          int64_t *cand_rows);

/* ------------------------------------------------------------------ profiling
 * HIP-event timing of the individual stages of the last asl_search_batch /
 * asl_index_search calls on the library's stream. Names: "encode","coarse_gemm",
 * "coarse_select","scan","filter","rescore","rescore_matches".
 * on = 1: every stage (two events around each: ~16 per batch, which keep the stages of a
 * pipelined batch from being dispatched back to back -- measured 0.3 ms of a 7.9 ms step);
 * on = 2: the list scan kernel only (the dominant kernel, two events per batch; the
 * scanned-vector counter, which costs a small kernel per scan, is not fed either); 0: off. */
int asl_profile_enable(int on);
int asl_profile_reset(void);
/* Accumulated milliseconds and launch count for a stage since the last reset. */
int asl_profile_get(const char *stage, double *total_ms, int64_t *launches);
/* Algorithmic work of the scan kernels since the last reset: sum over queries of
 * probed-list lengths (vectors scored). */
int64_t asl_profile_scanned_vectors(void);
/* The rescoring's second launch since the last reset, counted at level 1 only (all three stay 0
 * otherwise; any pointer may be null): candidates the first kernel could not score itself
 * (a doubly matched peak, ...), those of them it dropped because their upper bound lies below the
 * query's best exact score (winner-only calls; ASL_RESCORE_PRUNE=0 in the environment keeps them
 * all), and the items of the second launch's work list. */
int asl_profile_rescore_counts(int64_t *deferred, int64_t *pruned, int64_t *work_items);

#ifdef __cplusplus
}
#endif
#endif /* ANNSOLO_MI_H */
