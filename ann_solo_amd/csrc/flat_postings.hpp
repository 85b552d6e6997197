// flat_postings.hpp -- the dimension-major IVF-Flat postings: the two layouts and their encodings (every shift
// and mask of a posting format lives here), the view of one index's postings, the scan request, and what
// flat_scan.hip, flat_build.hip and flat_tools.hip export. Private to the library.
#pragma once
#include <cmath>

#include "common.hpp"

namespace asl {

// blocks of FI_BLK vectors with per-dimension postings
// FI_BLK measured (scan ms at nprobe 128): 512 7.69 | 640 7.14 | 768 6.81 | 832 6.71 | 864 6.70 (the LDS limit of three workgroups per CU) | 1024: two workgroups per CU
constexpr int FI_BLK = 832;
constexpr int FI_ROWS = (FI_BLK + 63) / 64;      // rows of 64 accumulators (and selector words) in a block

// ---- layout 1, float postings: a segment per (block, dimension) = its c values (f32), then its c local vector
// indices (u16); the table word = the segment's start from the block's base in 64-byte units << 16 | c
constexpr uint32_t INV_START_MAX = 0xffffu, INV_COUNT_MAX = 0xffffu;
__host__ __device__ inline uint32_t inv_word(uint32_t start, uint32_t count) { return (start << 16) | count; }
__host__ __device__ inline uint32_t inv_word_start(uint32_t w) { return w >> 16; }        // 64-byte units
__host__ __device__ inline uint32_t inv_word_count(uint32_t w) { return w & 0xffffu; }

// ---- layout 2, fixed-point words (flat_scan.hip, FX): a posting = value numerator (22 bits) << 10 | local vector
// index (10 bits); a segment is whole 128-byte lines of 32 words and its table BYTE is their number. A wave reads
// a table row with one 16-byte load per lane: at most 64 * 16 dimensions.
constexpr int FX_LOC_BITS = 10, FX_NUM_BITS = 22, FX_MAX_D = 64 * 16;
constexpr float FX_GRID = 4194304.0f;            // 2^22
static_assert(FX_LOC_BITS + FX_NUM_BITS == 32 && FX_GRID == (float)(1 << FX_NUM_BITS), "a posting is one 32-bit word");
static_assert(FI_BLK <= (1 << FX_LOC_BITS), "a block's local index fits the posting word");
static_assert((FI_BLK + 31) / 32 <= 255, "a segment's lines fit the table byte");
__host__ __device__ inline uint32_t fx_word(float x, uint32_t loc) {      // x on the grid: the product is exact
  return ((uint32_t)(x * FX_GRID) << FX_LOC_BITS) | loc;
}
__host__ __device__ inline uint32_t fx_word_num(uint32_t w) { return w >> FX_LOC_BITS; }
__host__ __device__ inline uint32_t fx_word_loc(uint32_t w) { return w & ((1u << FX_LOC_BITS) - 1u); }
__host__ __device__ inline uint32_t fx_seg_lines(uint32_t count) { return (count + 31u) / 32u; }

// fixed-point storage (22 fractional bits) of IVF-Flat components in [0, 1)
__host__ __device__ inline float fx22_round(float x) {
  if (!(x >= 0.0f && x < 1.0f)) return x;
  const float m = rintf(x * FX_GRID);             // a power of two: exact; ties to even
  return (m < FX_GRID - 1.0f ? m : FX_GRID - 1.0f) * (1.0f / FX_GRID);
}
__host__ __device__ inline bool fx22_on_grid(float x) {
  return x > 0.0f && x < 1.0f && x * FX_GRID == rintf(x * FX_GRID);
}

// Read-only view of one index's postings (index.hpp: postings_view). All pointers are device memory.
struct FlatPostings {
  int layout = 0, d = 0, nlist = 0;        // layout 0: none, 1: float postings, 2: fixed-point words
  int64_t n_blocks = 0;
  const int32_t *list_offsets = nullptr, *blk_offsets = nullptr;      // [nlist + 1] first position / block of each list
  const uint32_t *blk_base = nullptr;      // [n_blocks] start of the block's segments (layout 1: 64-byte units, 2: lines)
  const uint32_t *tab32 = nullptr;         // layout 1: table words [n_blocks, d]
  const uint8_t *tab8 = nullptr;           // layout 2: table bytes [n_blocks, tab_stride]; cnt16: postings per
  const uint16_t *cnt16 = nullptr;         // (block, dimension), for the work counter only
  int tab_stride = 0;
  const char *seg_bytes = nullptr;         // the segments
  const int32_t *ids = nullptr;            // the id per list-order position
};

// One postings scan. Value-initialised: dense queries, ordered rows, no gate, filter, selector or runs.
struct FlatScan {
  int nq = 0, nprobe = 0, k = 0;
  const float *xq = nullptr;               // [nq, d] dense queries; may be null when ent is given
  const uint2 *ent = nullptr;              // the queries as entry lists [nq, 64] + counts [nq] (list_nonzeros)
  const int32_t *ent_cnt = nullptr;
  const int32_t *coarse_I = nullptr;       // [nq, nprobe] probed lists (unread with ranges)
  float *D = nullptr;                      // output rows [nq, k]; any may be null
  int64_t *I64 = nullptr;
  int32_t *I32 = nullptr;
  int set_mode = 0;                        // 0: ordered rows, 1: the same hits as a set, 2: rows of packed keys
  const int *gate = nullptr;               // device-side row count: workgroups past it return at once
  ScanPostFilter post;                     // set-mode int32 rows, k <= 1280 only
  const unsigned long long *sel = nullptr; // selector: flat_selector's words, k <= 1280
  ScanRanges ranges;                       // the window-exact index: range [nq], a run of positions in ONE list
};

// A wave lists the non-zero components of a dense row, ascending: nzd[t] their dimensions, nzv[t] their
// values times `scale`; returns their number (the same in every lane).
__device__ __forceinline__ int list_row_nonzeros(const float *row, int d, int lane, float scale, uint16_t *nzd,
                                                 float *nzv) {
  int base = 0;
  for (int j0 = 0; j0 < d; j0 += 64) {
    const int j = j0 + lane;
    const float x = j < d ? row[j] : 0.0f;
    const unsigned long long m = __ballot(x != 0.0f);
    if (x != 0.0f) {
      const int t = base + __popcll(m & ((1ull << lane) - 1ull));
      nzd[t] = (uint16_t)j;
      nzv[t] = x * scale;
    }
    base += __popcll(m);
  }
  return base;
}

// ---- flat_scan.hip: the scan
bool flat_inv_supported(int d, int k, int nprobe);
int flat_inv_scan(const FlatPostings &P, const FlatScan &rq);

// ---- flat_build.hip: what builds postings from dense rows
int count_nnz(const float *vecs, int d, int64_t n, int32_t *nnz, int32_t *nnz_max_dev);
int quantize_fx22(float *x, int64_t n);
int inv_count(const float *vecs, int d, const int32_t *order, const int32_t *pos_blk, int64_t n, uint32_t *cnt);
// per layout: the host placement of one block's segments from its counts, then the fill (ordered inside a segment)
uint32_t inv_place_block(const uint32_t *cnt, int d, uint32_t *tab, bool *ok);
uint32_t fx_place_block(const uint32_t *cnt, int d, uint32_t line0, uint8_t *tab8, uint16_t *cnt16, uint32_t *seg_line);
int inv_fill(const float *vecs, int d, const int32_t *order, const int32_t *pos_blk, const uint16_t *pos_loc,
             int64_t n, int64_t nblocks, const uint32_t *blk_base, const uint32_t *seg_tab, uint32_t *cursor,
             char *seg_bytes);
int fx_fill(const float *vecs, int d, const int32_t *order, const int32_t *pos_blk, const uint16_t *pos_loc,
            int64_t n, int64_t ncell, const uint32_t *seg_line, uint32_t *cursor, uint32_t *words);

// ---- flat_tools.hip: what prepares or measures a scan
// the runs of the window-exact index: [lo, hi) per query over the key column by position (ascending, NaN last)
int winflat_runs(const double *q_pmz, int nq, const float *key, int64_t n, int charge, double tol, int mode,
                 int2 *runs, unsigned long long *acc);
// selector words of the postings layout: flat_selector_words_per_block() per block, bit v of word r of a
// block = keep[id of the block's position r * 64 + v] (behind the list's end: unselected)
int flat_selector(const FlatPostings &P, const uint8_t *keep, int64_t n, unsigned long long *words);
int flat_selector_words_per_block();
// algorithmic bytes and 128-byte lines of the scan of (xq, coarse_I): out_dev[0] += bytes, out_dev[1] += lines
int flat_postings_work(const FlatPostings &P, const float *xq, int nq, const int32_t *coarse_I, int nprobe,
                       unsigned long long *out_dev);

}  // namespace asl
