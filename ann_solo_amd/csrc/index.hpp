// index.hpp -- the index object (struct asl_index) and the index's internal interface: what
// the index_*.hip units share and what search.hip / sharded.hip call. Private to the library.
#pragma once
#include "common.hpp"
#include "flat_postings.hpp"
#include "ivf_kernels.hpp"

namespace asl {

constexpr size_t SCORE_CHUNK_BYTES = (size_t)1 << 30;
constexpr int FLAT_KEYS_SLACK = 768;      // packed-key rows of the postings scan: k + 768 <= its 2048-key buffer

// scratch of asl_index_search_sharded (sharded.hip), grow-only: steady-state calls allocate nothing
struct ShardScratch {
  DevBuf<float> x_all, cD, cD_all, Dp, Dr, Dtmp, Dfin, x3, cD3;
  DevBuf<int32_t> cI, cI_all, cI3, mine, everyone;       // (mine / everyone: a few ints every rank must see the same way)
  DevBuf<int64_t> Ip, Ir, Im;
  // the queries as entry lists (coarse_sparse.hip: list_nonzeros): own, everybody's, second scans
  DevBuf<uint2> e_loc, e_all, e3;
  DevBuf<int32_t> c_loc, c_all, c3, over;
  // the exact key exchange (exchange.hip)
  DevBuf<int64_t> Kp, Hs, Hr, Ko, Bs, Br, Xs, Xr, Mn, rowlist, K3;
  DevBuf<int32_t> need, flag, Fl, rmap;
  DevBuf<unsigned int> cursor;
};

// what the rows of a search hold: ORDERED (score desc, id asc), -1 padded; SET: the same hits in any order;
// SET_RAW / KEYS: as under asl_index_set_unordered(1) / (2) -- a set never re-ranked / packed 64-bit keys in I64
enum IndexRows { ROWS_ORDERED = 0, ROWS_SET, ROWS_SET_RAW, ROWS_KEYS };

// One search of index_search_device. Value-initialised: a dense ordered search with the index's own
// coarse stage. All pointers are device memory that stays valid until the scan has run.
struct IndexSearch {
  int nq = 0;
  const float *xq = nullptr;        // [nq, d] dense queries; may be null when pre_ent is given
  int k = 0, nprobe = 0;
  float *D = nullptr;               // outputs [nq, k]; any may be null
  int64_t *I64 = nullptr;
  int32_t *I32 = nullptr;
  const float *pre_D = nullptr;     // the caller's probe lists [nq, nprobe] (null: the coarse stage runs here);
  const int32_t *pre_I = nullptr;   // IVF-Flat reads pre_I alone
  const uint2 *pre_ent = nullptr;   // the queries as entry lists [nq, 64] + counts [nq] (list_nonzeros /
  const int32_t *pre_cnt = nullptr; // encode_entries_device); a hint when xq is given as well
  // pre_ent / pre_cnt WITHOUT pre_I: lists ready, probes still to find -- the coarse stage of this call scores
  // from them instead of listing the rows of xq again. pre_over travels with them: the device count of rows
  // with more than 64 non-zeros that their producer (encode_both_device) added to, zeroed in front of it
  // (coarse_lists_begin); the coarse kernels' gate reads it.
  int *pre_over = nullptr;
  const int *gate = nullptr;        // device-side count: only the first *gate rows are searched
  int rows = ROWS_ORDERED;          // IndexRows; a mode set with asl_index_set_unordered goes before ORDERED / SET
  const IndexPostFilter *post = nullptr;   // precursor window applied in the scan's finish where the scan can
  // what state of which library this request speaks for: the asl_library serial and the generation of its
  // selection (0, generation of asl_index_set_selector: the handle's own selector). It names post->payload and
  // sel_keep alike; the index rebuilds what it derived from either exactly when the pair or the lists change.
  uint64_t serial = 0, gen = 0;
  const IndexWindow *win = nullptr; // scan the in-window run of every probed list only (window-ordered layout)
  // selector (asl_index_search_selected): keep[id] != 0 = selected, [sel_n] with sel_n == ntotal; the scans
  // choose their k among the selected vectors of the probed lists. (serial, gen) above name its content.
  const uint8_t *sel_keep = nullptr;
  int64_t sel_n = 0;
  bool rows_filtered = false;       // OUT: the rows hold in-window hits only, their lengths in count / row_len
};

}  // namespace asl

struct asl_index {
  int d = 0, nlist = 0, kind = 0, pq_m = 0, pq_bits = 8, ksub = 0, dsub = 0;
  int niter = 25;
  bool trained = false;
  // IVF-PQ, FAISS' IndexIVFPQ::by_residual (asl_index_set_by_residual): false = the quantiser is trained on and
  // encodes the vectors themselves, and a score's coarse term dis0 is 0 -- the scans get zero_D for coarse_D
  bool by_residual = true;
  int64_t ntotal = 0;   // global vectors added
  int64_t n_store = 0;  // vectors stored here
  int shard_rank = 0, shard_world = 1;
  asl::DevBuf<float> centroids, codebooks;
  asl::DevBuf<float> codebooks_t;  // [m][dsub][ksub] copy for the tiled scan's LUT build
  bool cbt_ready = false;
  // sparse coarse quantiser (coarse_sparse.hip): transposed centroids [d][nlist] + per-batch scratch
  asl::DevBuf<float> centroids_t;
  bool cent_t_ready = false;
  asl::DevBuf<float> kmeans_ct;       // transposed centroids of the running k-means iteration
  asl::DevBuf<uint2> scan_ent;        // the scan's own entry lists (the coarse stage of the NEXT batch
  asl::DevBuf<int32_t> scan_cnt;      // overwrites cs_ent on the other stream of the pipeline)
  asl::DevBuf<int> scan_over;
  asl::DevBuf<uint2> cs_ent;
  asl::DevBuf<int32_t> cs_cnt;
  asl::DevBuf<int> cs_over;
  // add-order storage
  asl::DevBuf<float> vecs;        // FLAT, IVFFLAT
  asl::DevBuf<int32_t> vlist;     // IVF kinds: inverted list of each stored vector
  asl::DevBuf<int32_t> vids;      // global id of each stored vector (only when sharded)
  bool has_vids = false;
  asl::DevBuf<uint8_t> codes_add; // IVFPQ
  // list-order storage (IVFPQ scan layout)
  asl::DevBuf<uint8_t> codes;
  asl::DevBuf<int32_t> ids, list_offsets;
  std::vector<int32_t> h_list_offsets;
  // 64-vector tiles for the tiled scan, pq_scan_v3.hip (m = 32)
  asl::DevBuf<uint8_t> codes_tiled;
  asl::DevBuf<int32_t> ids_tiled, tile_offsets;
  // post-filter in the scan's finish (common.hpp: ScanPostFilter): (id, window value) per storage slot
  // -- per tile slot (IVF-PQ) or per list position (IVF-Flat) --, built on demand
  asl::DevBuf<int2> idpay;
  int64_t n_tile_slots = 0;
  uint64_t pay_serial = 0;       // serial of the library whose window column the pairs hold
  uint64_t pay_gen = 0;          // ... and the generation of its selection (the column is the effective one)
  int64_t pay_n = 0;
  bool idpay_ready = false;
  bool has_tiles = false;
  // window-ordered copy of the tiled layout (window_install): each list's vectors by a float32 key per
  // vector, ascending, NaN last -- same list and tile offsets as the default layout, which stays as it
  // is. Derived, never saved; build_lists drops it (add, add_preassigned, reset and shard all rebuild).
  asl::DevBuf<uint8_t> wcodes_tiled;
  asl::DevBuf<int32_t> wids_tiled;
  asl::DevBuf<float> wkey_tiled;      // the key per tile slot (NaN in a list's last tile behind its end)
  bool win_ready = false;
  uint64_t win_serial = 0;       // serial of the library whose window column is the key; 0: a caller's key
  uint64_t win_gen = 0;          // ... and the generation of its selection
  int window_scan = 0;           // asl_index_set_window_scan: asl_search_batch scans each query's window only
  asl::DevBuf<int2> win_ranges;       // [nq, nprobe] in-window run of each probed list (WINFLAT: [nq], one run per query)
  // ASL_INDEX_WINFLAT (the window-exact index): ONE list of all vectors cut into postings blocks -- ids (the
  // id per position), blk_base, inv_tab / inv_tab8, inv_data, has_inv, inv_layout below, as IVF-Flat with one
  // list -- in id order, or, once a key is installed (win_ready; win_serial / win_gen as above), ordered by
  // (key ascending, NaN last, id ascending) with the key per position here. Derived, never saved; dropped by
  // add, reset and a new key.
  asl::DevBuf<float> wf_key;          // [n_store] the key by position
  // sub-quantiser-major copy of codes_tiled (index_codes_mmajor; pq_scan_v3.hip, MM): 32 planes of mm_plane bytes,
  // plane m = sub-quantiser m's 64 bytes of every tile of the default layout, in tile order. The plain tiled scan
  // reads it instead of codes_tiled and skips the planes of a query's all-zero sub-vectors. Derived on the device,
  // never saved, dropped by build_lists, rebuilt by the next plain scan; one more copy of the codes in memory.
  asl::DevBuf<uint8_t> codes_mm;
  uint32_t mm_plane = 0;
  bool mm_ready = false;
  bool scan_mmajor = true;       // asl_index_set_scan_variant(2) clears it: variant 0 with the tile-major codes only
  // selector words of the scans (tile_selector, ivf_kernels.hpp / flat_selector, flat_postings.hpp), derived like idpay: never
  // saved, dropped by build_lists, rebuilt when (serial, generation) of the selector or the lists change.
  // sel_words: per tile of the default layout (IVF-PQ) or per 64 positions of a block (IVF-Flat);
  // wsel_words: per tile of the window-ordered copy (dropped with it)
  asl::DevBuf<unsigned long long> sel_words, wsel_words;
  bool sel_ready = false, wsel_ready = false;
  uint64_t sel_serial = 0, sel_gen = 0, wsel_serial = 0, wsel_gen = 0;
  // the handle's own selector (asl_index_set_selector): one byte per vector id; dropped when the lists change
  asl::DevBuf<uint8_t> selector;
  bool has_selector = false;
  uint64_t selector_gen = 0;
  int64_t n_blocks = 0;               // blocks of the postings layout
  // dimension-major postings for flat_inv_scan (IVF-Flat): blocks of FI_BLK vectors. flat_postings.hpp owns the
  // two layouts and their encodings; the scans, the selector, the rank and the work counter read them through
  // postings_view() below, the one place that picks inv_tab or inv_tab8
  asl::DevBuf<int32_t> blk_offsets;   // [nlist + 1] first block of each list
  asl::DevBuf<uint32_t> blk_base;     // [nblocks] start of the block's postings, 64-byte units
  asl::DevBuf<uint32_t> inv_tab;      // [nblocks * d] table words (inv_word)
  asl::DevBuf<char> inv_data;         // segments: c values (f32) then c local vector indices (u16), placed by 128-byte line
  bool has_inv = false;
  // the fixed-point layout (inv_layout 2): blk_base in 128-byte lines, one byte per (block,
  // dimension) = lines of the segment, posting words (fx_word) in inv_data
  int flat_storage = ASL_FLAT_F32;   // ASL_FLAT_F32 (default): components as given; ASL_FLAT_FX22: add() rounds
                                     // components in [0, 1) to 22 fractional bits
  int inv_layout = 0;            // what build_lists found the data fit for: 0 none, 1 float postings, 2 fixed-point words
  int nnz_max = 0;               // the most non-zeros of a stored vector, as build_postings counted them
  int tab_stride = 0;            // bytes per block of inv_tab8 (d rounded up to a 128-byte line)
  asl::DevBuf<uint8_t> inv_tab8;
  asl::DevBuf<uint16_t> inv_cnt16;    // postings per (block, dimension): work accounting only (asl_index_postings_work)
  int scan_variant = 0;  // 0 = the layout-specific scan when the shape allows; 1 = the generic kernels
  int unordered = 0;  // 1: search rows = exact top-k as a set, unspecified order (no final sort); 2: rows of packed keys
  bool lists_dirty = true;
  // asl_index_search_sharded: did every rank's shard answer asl_index_supports_keys with 1 for this
  // (k, nprobe, world)? -1 = not agreed yet (reset whenever the lists are rebuilt)
  int agreed_k = -1, agreed_np = -1, agreed_world = -1, agreed_val = -1;
  // exact re-rank of the IVF-PQ short-list (refine.hip): sparse copies of the added vectors,
  // add order = global id; kept whole on every shard
  int refine_k = 0;            // 0 = off; else the short-list size k' (> k) that is re-ranked
  bool refine_rows = false;    // rows are being stored on add()
  bool refine_bad = false;     // a vector had more non-zeros than a row holds
  int64_t r_n = 0;
  asl::DevBuf<uint16_t> r_dim;
  asl::DevBuf<float> r_val;
  asl::DevBuf<uint8_t> r_cnt;
  asl::DevBuf<int32_t> ws_short;
  // scratch
  asl::DevBuf<float> ws_scores, coarse_D, ws_x;
  asl::DevBuf<int32_t> coarse_I, ws_assign;
  asl::DevBuf<float> zero_D;          // by_residual off: zeros for any coarse_D (index_zero_coarse); never written
  asl::DevBuf<uint32_t> bitmap;
  asl::DevBuf<uint64_t> ws_upper;     // k > TK_MAX_K: the bound of every row between the passes
  asl::ShardScratch shard;       // asl_index_search_sharded
};

namespace asl {

// index.hip: the one check of an index's shape, for asl_index_create and asl_index_load (`who`): ASL_OK
// when (d, nlist, kind, pq_m, pq_bits) can be trained, filled and searched, else fail() names what cannot.
int index_shape_check(const char *who, int d, int nlist, int kind, int pq_m, int pq_bits);
// The tiled scan (pq_scan_v3.hip) is built for m = 32 and 8 bits, and keeps a query's components as
// 2-byte entries behind an 8-byte head in the 2 KB of its tile table: d * 2 + 8 <= 2048. A wider index
// of that m and bits gets no tiles and is scanned by the generic kernel, like every other shape.
constexpr int PQ_TILED_MAX_D = 1020;
// the kinds with inverted lists, a coarse quantiser and training (not Flat, not the one-list window-exact index)
inline bool ivf_kind(int kind) { return kind == ASL_INDEX_IVFFLAT || kind == ASL_INDEX_IVFPQ; }
// asl_search_batch scans each query's window only: the index's mode, or the kind that has no other
inline bool window_mode(const asl_index *ix) { return ix->window_scan || ix->kind == ASL_INDEX_WINFLAT; }
inline bool tiled_index(const asl_index *ix) {
  return ix->kind == ASL_INDEX_IVFPQ && ix->pq_m == 32 && ix->ksub == 256 && ix->d <= PQ_TILED_MAX_D;
}
// The postings an index holds, as its readers take them (layout 0: none -- an empty window-exact index, whose
// every run is empty, is scanned in the float form and reads nothing).
inline FlatPostings postings_view(const asl_index *ix) {
  FlatPostings P;
  P.layout = ix->has_inv ? ix->inv_layout : 0, P.d = ix->d, P.nlist = ix->nlist, P.n_blocks = ix->n_blocks;
  P.list_offsets = ix->list_offsets.p, P.blk_offsets = ix->blk_offsets.p, P.blk_base = ix->blk_base.p;
  if (P.layout == 2) P.tab8 = ix->inv_tab8.p, P.cnt16 = ix->inv_cnt16.p;
  else P.tab32 = ix->inv_tab.p;
  P.tab_stride = ix->tab_stride, P.seg_bytes = ix->inv_data.p, P.ids = ix->ids.p;
  return P;
}
// index_train.hip
int assign_ip(asl_index *ix, const float *x, int64_t ld, int64_t n, const float *cent, int k, int d,
              int32_t *assign_dev);
// index_lists.hip
int build_lists(asl_index *ix);
// the per-dimension postings of ix->vecs for a position order (order[i]: the add-order row at position i; blk_off:
// [nlists + 1] first block of each list; pos_blk / pos_loc: block and local index per position): float postings,
// or the fixed-point words when ix->flat_storage is fx22 and every non-zero is on the grid. Sets has_inv /
// inv_layout; leaves them clear when the vectors are too dense or the layout does not fit its offsets.
int build_postings(asl_index *ix, const int32_t *order_dev, int64_t n, const std::vector<int32_t> &blk_off,
                   const std::vector<int32_t> &pos_blk, const std::vector<uint16_t> &pos_loc);
// the one-list layout of a window-exact index: in id order, or (keyed) by (key, NaN last, id)
int winflat_layout(asl_index *ix, bool keyed, const float *key, uint64_t serial, uint64_t gen);
const char *window_unsupported(const asl_index *ix);
int window_install(asl_index *ix, int64_t n, const float *key, uint64_t serial, uint64_t gen = 0);
int post_filter_pairs(asl_index *ix, const IndexPostFilter &p, uint64_t serial, uint64_t gen,
                      const int32_t *slot_ids, int64_t nslots);
// the selector words of rq's selector for the layout its scan reads (window: the window-ordered copy) -> *words
int selector_words(asl_index *ix, const IndexSearch &rq, bool window, const unsigned long long **words);
// index_search.hip
int index_search_device(asl_index *ix, IndexSearch &rq);
int index_nprobe(const asl_index *ix, int nprobe);
int index_prepare(asl_index *ix);
// pre_ent / pre_cnt / pre_over: the rows' entry lists where their producer made them already (IndexSearch)
int coarse_search(asl_index *ix, const float *xq, int nq, int nprobe, float *out_D, int32_t *out_I, uint2 *ent_out,
                  int32_t *cnt_out, bool *have_ent, const uint2 *pre_ent = nullptr, const int32_t *pre_cnt = nullptr,
                  int *pre_over = nullptr);
// Will the coarse stage of an nq-row search of this index take entry lists from the encoder? Then *over is the
// zeroed device counter the encoder adds to (on this stream). ASL_COARSE_LISTS=0: never (lists rebuilt from the rows).
int coarse_lists_begin(asl_index *ix, int nq, int **over);
int index_window_prepare(asl_index *ix, uint64_t serial, uint64_t gen, const float *key, int64_t n, int nq,
                         int nprobe);
int index_refine_k(const asl_index *ix);
int coarse_scores_all(asl_index *ix, const float *xq, int m, float *scores, uint2 *ent = nullptr, int32_t *cnt = nullptr,
                      int *ready_over = nullptr);
int index_codebooks_transposed(asl_index *ix);
int index_codes_mmajor(asl_index *ix);   // index_search.hip: the sub-quantiser-major copy, built when missing (mm_ready)
// n zeros (grow-only, cleared when it grows): the coarse_D of an IVF-PQ index with by_residual off
int index_zero_coarse(asl_index *ix, size_t n, const float **zeros);

}  // namespace asl
