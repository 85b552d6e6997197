// flat_scan.hip -- exact IVF-Flat list scan over per-dimension POSTINGS inside every inverted
// list (replaces the scan inside FAISS IndexIVFFlat.search,
// /root/reference/src/ann_solo/spectral_library.py:443-444).
//
// A hashed spectrum vector has at most ~50 non-zeros out of 800 (one per peak). The score of a
// stored vector is acc = fmaf(q[dim], val, acc) over its non-zeros in ascending dimension --
// the ascending-index fp32 chain restricted to the stored non-zeros, which is bit-identical to
// the dense chain (a zero factor leaves the accumulator unchanged), to the fp32-MFMA GEMM and
// to the oracle. Top-k: hist_topk.hpp (no sorting while streaming).
#include <cstdlib>

#include "common.hpp"
#include "flat_postings.hpp"
#include "hist_topk.hpp"
#include "pq_tile.hpp"

namespace asl {

// Dimension-major ("postings") IVF-Flat. Streaming EVERY stored non-zero of the probed lists
// (~27 per vector; the sparse-tile scan of round 1) reads 16x more than needed: a query has
// <= ~50 non-zero components of 800 and only stored entries in those dimensions can
// contribute. So every inverted list is cut into blocks
// of FI_BLK vectors and each block keeps, per dimension, the postings (local vector index
// u16, value f32) of the vectors that are non-zero there -- an inverted file inside the
// inverted file. Storage: one segment per (block, dimension), its c values followed by its c
// local indices (6c bytes), and one table word per (block, dimension): the segment's start in
// 64-byte units from the block's base (high 16 bits) and c (low 16 bits). Every (query, block)
// pair touches its own lines (L2 hit rate < 10 %), so segments are PLACED BY LINE: one that
// fits a 128-byte line never straddles two, a longer one starts on a line boundary -- a
// dimension of a 512-vector list (17 postings, 102 bytes) costs one line instead of 1.8, for
// ~25 % padding. A wave takes one (query, block): it zeroes the block's accumulators in LDS
// and walks the query's non-zero dimensions in ASCENDING order, acc[loc] = fmaf(q_d, val,
// acc[loc]) over that dimension's postings (a vector occurs at most once per dimension, so
// the lanes of one step never collide -- lanes past a row's count repeat its last posting and
// store the same bits, see the row loop -- and steps of one wave reach LDS in program order).
// Per vector this is the ascending-dimension fp32 chain restricted to the dimensions where
// both factors are non-zero -- bit-identical to the dense chain, the MFMA GEMM and the oracle
// (a zero factor leaves the accumulator unchanged) -- at 1/16 of the tile kernel's traffic
// (50 of 800 dimensions) and 1/4 of its lane-steps. Then the wave offers its accumulators to
// the workgroup's histogram top-k, vectors with score 0 included (they are candidates of the
// dense scan too). The eight waves of a workgroup run their blocks independently (blocks are
// handed out by an LDS counter, a block's candidates are appended with one atomic, or one per
// row when they are many) and meet only when the key buffer is full: see "Offers" below.
// FI_CHUNK: blocks of a query listed at a time (a query of the bench probes ~150: one chunk, so the
// waves of a workgroup wait for each other once per query)
constexpr int FI_NW = 8, FI_NT = 64 * FI_NW, FI_CHUNK = 256, FI_U = 8;   // FI_U: rows in flight per wave
static_assert(64 % FI_U == 0, "a batch of dimensions must not straddle the 64 lanes of a chunk");

// (wave_incl_scan -- the seven-DPP-add prefix sum of hist_topk.hpp -- runs twice per block in the
// per-block bookkeeping: the kernel is VALU-bound, profiles/r04_ivfflat_np112_pmc_summary.txt:
// SQ_ACTIVE_INST_VALU 89 % of the SIMD cycles)

struct FiUnit {
  uint32_t blk;   // block index into the per-dimension table
  int32_t pos0;   // list-order position of the block's first vector
};                // (+ the block's vector count in a 16-bit array: 10 bytes per block of a chunk)

// FI_CAP: key buffer of the top-k (2048: k <= 1280, three workgroups per CU; 4096: k <= 3328, two)
//
// FX = true: the FIXED-POINT layout (round 4). Every stored component lies in (0, 1) on the grid
// of 2^-22 (asl_index_set_flat_storage: add() rounds them there), so a posting is ONE 32-bit word
// -- value numerator M (22 bits) << 10 | local vector index (10 bits) -- instead of a float and
// a 16-bit index. Segments are whole 128-byte lines of 32 postings, the tail of the last line
// repeating the last posting (a lane that applies a repeat reads the same accumulator, computes
// the same sum and stores the same bits -- the rule the row loop already relies on), so a
// segment needs no count, and the table shrinks from a 4-byte word to ONE BYTE per (block,
// dimension): the segment's number of lines. Its start is the running sum of the bytes before
// it, which the wave forms itself: lane L loads the 16 bytes of dimensions 16 L .. 16 L + 15
// (one 16-byte load covers the whole row of a block, 7 lines for d = 800 instead of the ~18 of
// 25 a query's dimensions hit in the 4-byte table), byte sums with v_sad_u8, a wave prefix
// scan, and the lane that owns a query dimension pulls its 16-dimension group's prefix and words
// (ds_bpermute) and adds the bytes in front of its own. The chain is unchanged --
// acc = fmaf(q_d, x_d, acc) over ascending d with x_d = M 2^-22 (the 2^-22 is folded into the
// query value: a power of two, exact) -- so ids and score bits equal the oracle's over the same
// stored vectors. Measured on the bench library (scripts/flat_layout_model.py): 13 135 -> 8 980
// lines per query at nprobe 112, and the row loop loses one of its two loads.
//
// SEL (asl_index_search_selected, a library's selection; the 2048-key instantiations only): sel holds
// FI_ROWS 64-bit words per block, bit v of word r = the vector at position r * 64 + v of the block is
// selected. The wave loads a block's words once (lanes 0 .. FI_ROWS - 1, one word each) and every lane
// keeps the FI_ROWS bits of its own positions; an unselected vector is accumulated like any other and
// never counted or offered: wherever a position is tested with v < nb, its bit is tested too.
//
// RANGED (the window-exact index, ASL_INDEX_WINFLAT; the 2048-key instantiations only): the index is ONE list
// in precursor order and rg.range[q] = [lo, hi) is the query's run of positions (winflat_runs_kernel, flat_tools.hip);
// coarse_I, nprobe, list_offsets and blk_offsets are unread. The unit table lists the blocks lo / FI_BLK ..
// (hi - 1) / FI_BLK -- a whole block outside the run is never listed and none of its lines are fetched -- and
// a unit's first and one-past-last in-run position follow from its pos0 and the run. An out-of-run vector of a
// boundary block is accumulated like any other and never counted or offered (the rule SEL follows): wherever
// a position is tested with v < nb, it is tested with first <= v && v < last. Set-mode rows hold in-run hits
// only and rg.row_len[q] their number, as in the ranged PQ scan.
template <int FI_CAP, bool FX, bool WIDE, bool SEL = false, bool RANGED = false>
__global__ __launch_bounds__(FI_NT, FI_CAP <= 2048 ? 6 : 4) void flat_inv_scan_kernel(
    const float *__restrict__ xq, int d, const int32_t *__restrict__ coarse_I, int nprobe,
    const int32_t *__restrict__ list_offsets, const int32_t *__restrict__ blk_offsets,
    const uint32_t *__restrict__ blk_base, const uint32_t *__restrict__ seg_tab,
    const char *__restrict__ seg_bytes, const int32_t *__restrict__ ids, int k,
    float *__restrict__ D, int64_t *__restrict__ I64, int32_t *__restrict__ I32, int set_mode,
    const uint2 *__restrict__ ent, const int32_t *__restrict__ ent_cnt, int tab_stride,
    const int *__restrict__ gate, const ScanPostFilter pf, const unsigned long long *__restrict__ sel,
    const ScanRanges rg) {
  static_assert(!SEL || FI_CAP <= 2048, "the selector is built into the 2048-key instantiations only");
  static_assert(!RANGED || (FI_CAP <= 2048 && !WIDE && !SEL), "the ranged form: 2048 keys, no probes, no selector");
  if (gate && (int)blockIdx.x >= *gate) return;      // device-side row count (see pq_scan_v3_kernel)
  constexpr float FX_SCALE = FX ? 1.0f / FX_GRID : 1.0f;      // 2^-22, folded into the query values
  using TopK = HistTopK<FI_CAP, FI_NT, FI_NT>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *s_acc = reinterpret_cast<float *>(smem + TopK::lds_bytes());      // [FI_NW][FI_BLK]
  float *s_nzv = s_acc + FI_NW * FI_BLK;                                   // [d]
  FiUnit *table = reinterpret_cast<FiUnit *>(s_nzv + ((d + 3) & ~3));      // [FI_CHUNK]
  int *s_misc = reinterpret_cast<int *>(table + FI_CHUNK);                 // [16]
  uint16_t *s_nzd = reinterpret_cast<uint16_t *>(s_misc + 16);             // [d rounded up to 8]
  uint16_t *s_nbv = s_nzd + ((d + 7) & ~7);                                // [FI_CHUNK] vectors per block
  volatile int *s_flag = s_misc + 9;      // a wave asks for a sync of the top-k
  int *s_done = s_misc + 10;              // waves that finished their blocks, summed over the chunks
  int *s_next = s_misc + 11;              // next block of the chunk to hand out
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.x;

  // the query's non-zero components, ascending: from the ready entry list (list_nonzeros: 512
  // bytes) or listed here from the dense row (staged through the accumulator area)
  float *s_q = s_acc;
  int ecnt = ent ? ent_cnt[q] : -1;                // block-uniform; < 0: more than 64 non-zeros
  if (!xq && ecnt < 0) ecnt = 0;                   // (entry lists only: such a row is searched as all-zero)
  const bool fast = ecnt >= 0;
  if (!fast)
    for (int i = tid; i < d; i += FI_NT) s_q[i] = xq[(size_t)q * d + i];
  // a thread per probe (WIDE: probes tid and tid + FI_NT -- nprobe up to 1024, the reference's clamp,
  // spectral_library.py:77-81)
  constexpr int PP = WIDE ? 2 : 1;
  int my_len[PP], my_pos[PP], my_b0[PP], my_nb[PP], my_pre[PP];
  int run_lo = 0, run_hi = 0, run_b0 = 0;      // RANGED: the query's run of positions and its first block
#pragma unroll
  for (int pp = 0; pp < PP; ++pp) {
    my_len[pp] = 0, my_pos[pp] = 0, my_b0[pp] = 0, my_nb[pp] = 0;
    const int p = tid + pp * FI_NT;
    if (!RANGED && p < nprobe) {
      const int l = coarse_I[(size_t)q * nprobe + p];
      if (l >= 0) {
        my_pos[pp] = list_offsets[l];
        my_len[pp] = list_offsets[l + 1] - my_pos[pp];
        my_b0[pp] = blk_offsets[l];
        my_nb[pp] = blk_offsets[l + 1] - my_b0[pp];
      }
    }
  }
  int total = 0;
  if constexpr (RANGED) {
    const int2 run = rg.range[q];              // block-uniform
    run_lo = run.x, run_hi = run.y;
    run_b0 = run_lo / FI_BLK;
    if (run_hi > run_lo) total = (run_hi - 1) / FI_BLK - run_b0 + 1;
    __syncthreads();                           // s_q complete
  }
#pragma unroll
  for (int pp = 0; pp < (RANGED ? 0 : PP); ++pp) {
    int part_total;
    if (pp) __syncthreads();      // the partial sums of the first scan have been read
    my_pre[pp] = total + block_excl_scan<FI_NW>(my_nb[pp], s_misc, tid, part_total);   // barrier inside: s_q complete
    total += part_total;
  }
  if (wave == 0 && fast) {
    if (lane < ecnt) {
      const uint2 e = ent[(size_t)q * 64 + lane];
      s_nzd[lane] = (uint16_t)(e.x >> 7);
      s_nzv[lane] = __uint_as_float(e.y) * FX_SCALE;
    }
    if (lane == 0) {
      s_misc[8] = ecnt;
      s_misc[9] = 0;      // sync flag
      s_misc[10] = 0;     // finished waves
    }
  } else if (wave == 0) {
    const int base = list_row_nonzeros(s_q, d, lane, FX_SCALE, s_nzd, s_nzv);
    if (lane == 0) {
      s_misc[8] = base;
      s_misc[9] = 0;      // sync flag
      s_misc[10] = 0;     // finished waves
    }
  }
  __syncthreads();
  const int K = s_misc[8];
  TopK top;
  top.init(smem, k, ids, tid);
  top.out_keys = set_mode == 2 && I64 != nullptr;     // rows of packed keys (sharded exchange)
  float *acc = s_acc + wave * FI_BLK;
  const uint32_t lane4 = (uint32_t)lane * 4u;
  int chunks_done = 0;
  auto sync = [&]() {             // raise the flag, meet the other waves, compact
    if (lane == 0) *s_flag = 1;
    __syncthreads();
    if (tid == 0) *s_flag = 0;
    top.free_sync();
  };
  auto sync_wanted = [&]() -> bool { return __builtin_amdgcn_readfirstlane(*s_flag) != 0; };
  for (int c0 = 0; c0 < total; c0 += FI_CHUNK) {
    if constexpr (RANGED) {
      for (int t = c0 + tid; t < min(total, c0 + FI_CHUNK); t += FI_NT) {
        FiUnit u;
        u.blk = (uint32_t)(run_b0 + t);
        u.pos0 = (run_b0 + t) * FI_BLK;
        table[t - c0] = u;
        s_nbv[t - c0] = (uint16_t)min(FI_BLK, run_hi - u.pos0);      // one past the block's last in-run position
      }
    }
#pragma unroll
    for (int pp = 0; pp < (RANGED ? 0 : PP); ++pp) {
      const int lo = max(my_pre[pp], c0), hi = min(my_pre[pp] + my_nb[pp], c0 + FI_CHUNK);
      for (int t = lo; t < hi; ++t) {
        const int j = t - my_pre[pp];
        FiUnit u;
        u.blk = (uint32_t)(my_b0[pp] + j);
        u.pos0 = my_pos[pp] + j * FI_BLK;
        table[t - c0] = u;
        s_nbv[t - c0] = (uint16_t)min(FI_BLK, my_len[pp] - j * FI_BLK);
      }
    }
    __syncthreads();
    const int nent = min(FI_CHUNK, total - c0);
    // The waves take blocks on their own: the first FI_NW in wave order (the cold start below
    // needs every wave), then whichever is next (probe order: the lists closest to the query
    // first, they raise the threshold soonest).
    if (tid == 0) *s_next = FI_NW;
    __syncthreads();
    bool first = true;
    for (int i = wave;; first = false) {
      int nb = 0, pos0 = 0;
      uint32_t selbits = 0;    // SEL: bit r = my position of row r (r * 64 + lane) is selected
      auto sel_ok = [&](int r) -> bool { return !SEL || ((selbits >> r) & 1u) != 0; };
      int first_in = 0;        // RANGED: the block's first in-run position (nb: one past its last)
      auto in_run = [&](int v) -> bool { return !RANGED || v >= first_in; };
      if (i < nent) {          // wave-uniform
        const FiUnit u = table[i];
        nb = __builtin_amdgcn_readfirstlane((int)s_nbv[i]);
        pos0 = __builtin_amdgcn_readfirstlane(u.pos0);
        if constexpr (RANGED) first_in = max(run_lo - pos0, 0);
        const uint32_t blk = (uint32_t)__builtin_amdgcn_readfirstlane((int)u.blk);
        const char *bptr = seg_bytes + (size_t)blk_base[blk] * (FX ? 128 : 64);     // (a scalar load: blk is wave-uniform)
        // (RANGED: the run's last block is zeroed up to its last in-run position; the postings of the vectors
        // behind it land on what the wave's previous block left there, and those positions are never read)
        for (int o = lane; o < nb; o += 64) acc[o] = 0.0f;
        // SEL: the block's words are requested here and used behind the row loop, which hides their latency
        // (requested there, the scan at nprobe 112 ran 2 % slower: DESIGN.md 5 "Subset search")
        unsigned long long w = 0ull;
        if constexpr (SEL)
          if (lane < FI_ROWS) w = sel[(size_t)blk * FI_ROWS + lane];
        const uint32_t *erow = seg_tab + (size_t)blk * d;
        // FX: the block's byte table (lines per dimension), 16 dimensions per lane, and the
        // lines in front of each group of 16
        uint4 tb = make_uint4(0u, 0u, 0u, 0u);
        uint32_t tpre = 0;
        if constexpr (FX) {
          const uint8_t *trow = reinterpret_cast<const uint8_t *>(seg_tab) + (size_t)blk * tab_stride;
          if (lane * 16 < tab_stride) tb = *reinterpret_cast<const uint4 *>(trow + lane * 16);
          const uint32_t mine = __builtin_amdgcn_sad_u8(tb.x, 0u, 0u) + __builtin_amdgcn_sad_u8(tb.y, 0u, 0u) +
                                __builtin_amdgcn_sad_u8(tb.z, 0u, 0u) + __builtin_amdgcn_sad_u8(tb.w, 0u, 0u);
          tpre = wave_incl_scan(mine) - mine;
        }
        for (int kk0 = 0; kk0 < K; kk0 += 64) {
          const int kk = kk0 + lane;
          uint2 e = make_uint2(0u, 0u);     // first byte (from the block's base), postings (FX: padded to whole lines)
          float qv = 0.0f;
          if constexpr (FX) {
            const int dim = kk < K ? (int)s_nzd[kk] : 0;
            const int src = (dim >> 4) << 2, b = dim & 15, wi = b >> 2, sh = (b & 3) * 8;
            const uint32_t gp = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)tpre);
            const uint32_t w0 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)tb.x);
            const uint32_t w1 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)tb.y);
            const uint32_t w2 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)tb.z);
            const uint32_t w3 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)tb.w);
            const uint32_t ws = wi == 0 ? w0 : wi == 1 ? w1 : wi == 2 ? w2 : w3;
            uint32_t before = __builtin_amdgcn_sad_u8(ws & ((1u << sh) - 1u), 0u, 0u);
            before += wi > 0 ? __builtin_amdgcn_sad_u8(w0, 0u, 0u) : 0u;
            before += wi > 1 ? __builtin_amdgcn_sad_u8(w1, 0u, 0u) : 0u;
            before += wi > 2 ? __builtin_amdgcn_sad_u8(w2, 0u, 0u) : 0u;
            if (kk < K) {
              e = make_uint2((gp + before) * 128u, ((ws >> sh) & 0xffu) * 32u);
              qv = s_nzv[kk];
            }
          } else if (kk < K) {
            const uint32_t w = erow[s_nzd[kk]];
            e = make_uint2(inv_word_start(w) * 64u, inv_word_count(w));
            qv = s_nzv[kk];
          }
          // The unit of work is a ROW: up to 64 postings of one dimension. A dimension of a
          // 512-vector list has ~17 postings (one row), but a fragment bin that half the library
          // shares has hundreds -- a third of the work of a query that holds it -- so rows, not
          // dimensions, go through the pipeline. Lane j owns dimension j of the chunk (start e.x,
          // postings e.y, query value qv); rows are numbered in dimension order, and lane r
          // looks its row up: the dimension whose rows include r (binary search over the
          // prefix sums, ds_bpermute pulls), then start, count and query value of that
          // dimension. More than 64 rows in a chunk (dense data): further passes.
          const uint32_t rows_j = (e.y + 63u) >> 6;
          const uint32_t incl = wave_incl_scan(rows_j);
          const uint32_t pre = incl - rows_j;      // first row of my dimension
          const uint32_t R = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
          for (uint32_t r0 = 0; r0 < R; r0 += 64) {
            // my row; a lane past the last row takes the last row again with a zero query value
            // (fmaf(0, val, acc) == acc: the accumulators are never -0), so every row the
            // pipeline sees is a real one
            const bool live = r0 + lane < R;
            const uint32_t x = min(r0 + (uint32_t)lane, R - 1u);
            int lo = 0, hi = 63;                   // the last dimension with pre <= x
#pragma unroll
            for (int it = 0; it < 6; ++it) {
              const int mid = (lo + hi + 1) >> 1;
              const uint32_t pm = (uint32_t)__builtin_amdgcn_ds_bpermute(mid << 2, (int)pre);
              if (pm <= x) lo = mid; else hi = mid - 1;
            }
            const uint32_t pj = (uint32_t)__builtin_amdgcn_ds_bpermute(lo << 2, (int)pre);
            const uint32_t stj = (uint32_t)__builtin_amdgcn_ds_bpermute(lo << 2, (int)e.x);
            const uint32_t cnj = (uint32_t)__builtin_amdgcn_ds_bpermute(lo << 2, (int)e.y);
            const float rq0 = __builtin_bit_cast(
                float, __builtin_amdgcn_ds_bpermute(lo << 2, __builtin_bit_cast(int, qv)));
            const float rq = live ? rq0 : 0.0f;
            const uint32_t t = x - pj;             // row inside the dimension
            const uint32_t rc1 = min(64u, cnj - 64u * t) - 1u;    // last lane of my row with a posting of its own
            const uint32_t rvo = stj + 256u * t;                  // its values (FX: its posting words) ...
            const uint32_t rlo = stj + 4u * cnj + 128u * t;       // ... and local indices
            const uint32_t rfx = rvo | (rc1 >> 5);                // FX: offset | (two lines wide)
            // Software pipeline over the rows, FI_U deep: row r + FI_U is requested as soon as
            // row r has been applied, so FI_U - 1 rows are always in flight (loads return in
            // order: the wait before applying r is "all but the 2 (FI_U - 1) youngest"). Loads
            // AND updates are unconditional: a lane without a posting of its own repeats the
            // row's last one -- same line, no traffic; it computes the same sum from the same
            // accumulator and stores the same bits -- so the row loop has neither an execution
            // mask nor a branch (4 of its ~20 instructions), nothing hides a load from the wait
            // counters, and the loop runs to a multiple of FI_U without a tail case. Rows of
            // one dimension touch different vectors; rows of different dimensions are applied in
            // dimension order: the canonical chain.
            // (FX: a row is one or two whole lines of posting words; rc1 is 31 or 63 -- a power of
            // two minus one, so the clamp is a mask -- and the lanes past a single line repeat it)
            uint32_t loc[FI_U];
            float qj[FI_U], val[FI_U];
#define FI_FETCH(u, r)                                                                            \
  {                                                                                               \
    qj[u] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rq), (r))); \
    if constexpr (FX) {                                                                           \
      /* one descriptor word: the row's byte offset (a multiple of 128) | 1 when it is two lines \
         wide; the offset goes into the scalar base, the width into the mask of my word index */  \
      const uint32_t s_ = (uint32_t)__builtin_amdgcn_readlane((int)rfx, (r));                     \
      const char *row_ = bptr + (s_ & ~1u);                                                       \
      loc[u] = *reinterpret_cast<const uint32_t *>(row_ + (lane4 & ((s_ & 1u) ? 255u : 127u)));   \
    } else {                                                                                      \
      const uint32_t vo_ = (uint32_t)__builtin_amdgcn_readlane((int)rvo, (r));                    \
      const uint32_t c1_ = (uint32_t)__builtin_amdgcn_readlane((int)rc1, (r));                    \
      const uint32_t lo_ = (uint32_t)__builtin_amdgcn_readlane((int)rlo, (r));                    \
      const uint32_t l_ = min((uint32_t)lane, c1_);                                               \
      val[u] = *reinterpret_cast<const float *>(bptr + (vo_ + 4u * l_));                          \
      loc[u] = *reinterpret_cast<const uint16_t *>(bptr + (lo_ + 2u * l_));                       \
    }                                                                                             \
    __builtin_amdgcn_sched_barrier(0);   /* the request stays here: FI_U - 1 rows in flight */     \
  }
#define FI_APPLY(u)                                                     \
  {                                                                     \
    if constexpr (FX) {                                                 \
      const uint32_t l_ = fx_word_loc(loc[u]);                          \
      acc[l_] = __builtin_fmaf(qj[u], (float)fx_word_num(loc[u]), acc[l_]); \
    } else {                                                            \
      acc[loc[u]] = __builtin_fmaf(qj[u], val[u], acc[loc[u]]);         \
    }                                                                   \
    __builtin_amdgcn_sched_barrier(0);                                  \
  }
            const int n = (int)min(64u, R - r0);
            const int n_up = (n + FI_U - 1) & ~(FI_U - 1);
#pragma unroll
            for (int u = 0; u < FI_U; ++u) FI_FETCH(u, u)
            for (int j0 = FI_U; j0 < n_up; j0 += FI_U) {
#pragma unroll
              for (int u = 0; u < FI_U; ++u) {
                FI_APPLY(u)
                FI_FETCH(u, j0 + u)
              }
            }
#pragma unroll
            for (int u = 0; u < FI_U; ++u) FI_APPLY(u)
#undef FI_FETCH
#undef FI_APPLY
          }
        }
        if constexpr (SEL) {      // (the transposition behind the row loop: its registers are free again)
#pragma unroll
          for (int r = 0; r < FI_ROWS; ++r) {
            const unsigned long long wr =
                ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(w >> 32), r) << 32) |
                (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)w, r);
            selbits |= (uint32_t)((wr >> lane) & 1ull) << r;
          }
        }
      }
      // the first blocks of a query: every accumulator of eight blocks would pass (4 k candidates
      // against a buffer of 2 k) -- the threshold is fixed from a histogram of all of them first
      const bool cold = c0 == 0 && first;     // the same for every wave
      if (cold) {
        for (int r = 0; r * 64 < nb; ++r) {
          const int v = r * 64 + lane;
          top.cold_count(v < nb && in_run(v) && sel_ok(r), v < nb ? acc[v] : 0.0f);
        }
        top.cold_threshold();
      }
      // Offers: a row of accumulators at a time, straight into the key buffer (free_append: one
      // atomic per row that holds a candidate, no barrier). When the buffer is full the wave
      // raises the sync flag and waits; every wave looks at the flag between blocks (and in
      // the wait at the end of the chunk) and joins; then the row is tried again against the
      // new threshold.
      // A block past the first few of a query holds a handful of candidates: the wave reads
      // all its accumulators at once (13 rows, one LDS latency instead of 13), counts what
      // passes and, if that fits one row of slots, reserves it with ONE atomic instead of one
      // per row.
      bool offered = false;
      if (!cold && !top.sort_mode) {
        float sc[FI_ROWS];
#pragma unroll
        for (int r = 0; r < FI_ROWS; ++r) {
          const int v = r * 64 + lane;
          sc[r] = v < nb ? acc[v] : 0.0f;
        }
        int c = 0;
#pragma unroll
        for (int r = 0; r < FI_ROWS; ++r)
          c += __popcll(__ballot(r * 64 + lane < nb && in_run(r * 64 + lane) && sel_ok(r) && top.passes(sc[r])));
        if (c == 0) {
          offered = true;
        } else if (c <= 64) {
          int base = top.free_reserve(c);
          if (base >= 0) {
#pragma unroll
            for (int r = 0; r < FI_ROWS; ++r) {
              const int v = r * 64 + lane;
              const bool p = v < nb && in_run(v) && sel_ok(r) && top.passes(sc[r]);
              const unsigned long long m = __ballot(p);
              if (m) {                                                     // wave-uniform
                top.free_write(p, m, sc[r], (uint32_t)(pos0 + v), base);
                base += __popcll(m);
              }
            }
            offered = true;
          }
        }
      }
      for (int r = 0; !offered && r * 64 < nb; ++r) {
        const int v = r * 64 + lane;
        const float score = v < nb ? acc[v] : 0.0f;
        for (;;) {
          const bool p = v < nb && in_run(v) && sel_ok(r) && top.passes(score);
          if (!__ballot(p)) break;                                        // wave-uniform
          if (top.free_append(p, score, (uint32_t)(pos0 + v), cold)) break;
          sync();
        }
      }
      if (sync_wanted()) sync();
      if (i >= nent) break;
      if (lane == 0) i = atomicAdd(s_next, 1);
      i = __builtin_amdgcn_readfirstlane(i);
      if (i >= nent) break;
    }
    // end of the chunk: wait for the other waves, joining the syncs they ask for
    if (lane == 0) atomicAdd(s_done, 1);
    ++chunks_done;
    for (;;) {
      if (sync_wanted()) {
        sync();
        continue;
      }
      if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(s_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) >=
          FI_NW * chunks_done)
        break;
      __builtin_amdgcn_s_sleep(4);
    }
    __syncthreads();
  }
  top.free_done();
  if constexpr (RANGED) {
    // set mode: the row holds in-run hits only, so its length goes to the rescoring as it is (-1 after exact
    // flushes: the row is -1 padded and the rescoring's own filter, which every hit passes, finds its end)
    static_assert((size_t)FI_CAP * 8 <= (size_t)FI_NW * FI_BLK * 4, "the set finish's scratch is the accumulators");
    if (set_mode) {
      const int n = top.finish_set(D ? D + (size_t)q * k : nullptr, I64 ? I64 + (size_t)q * k : nullptr,
                                   I32 ? I32 + (size_t)q * k : nullptr, reinterpret_cast<u64 *>(s_acc));
      if (rg.row_len && tid == 0) rg.row_len[q] = n;
    } else {
      top.finish(D ? D + (size_t)q * k : nullptr, I64 ? I64 + (size_t)q * k : nullptr,
                 I32 ? I32 + (size_t)q * k : nullptr);
    }
  } else if (set_mode && (size_t)FI_CAP * 9 <= (size_t)FI_NW * FI_BLK * 4)   // unordered exact top-k; the accumulators are dead: scratch
    top.finish_set(D ? D + (size_t)q * k : nullptr, I64 ? I64 + (size_t)q * k : nullptr,
                   I32 ? I32 + (size_t)q * k : nullptr, reinterpret_cast<u64 *>(s_acc), &pf, q);
  else if (set_mode && (size_t)FI_CAP * 8 <= (size_t)FI_NW * FI_BLK * 4)
    top.finish_set(D ? D + (size_t)q * k : nullptr, I64 ? I64 + (size_t)q * k : nullptr,
                   I32 ? I32 + (size_t)q * k : nullptr, reinterpret_cast<u64 *>(s_acc));
  else
    top.finish(D ? D + (size_t)q * k : nullptr, I64 ? I64 + (size_t)q * k : nullptr,
               I32 ? I32 + (size_t)q * k : nullptr);
}

bool flat_inv_supported(int d, int k, int nprobe) {
  return d <= 4096 && nprobe <= 2 * FI_NT && k >= 1 && k + FI_NT + 256 <= 4096;
}

// The one launch: the view and the request unpacked into the kernel's parameter list.
template <int FI_CAP, bool FX, bool WIDE, bool SEL, bool RANGED>
static int launch_flat_inv(const FlatPostings &P, const FlatScan &rq) {
  using TopK = HistTopK<FI_CAP, FI_NT, FI_NT>;
  const int d = P.d;
  const size_t lds = TopK::lds_bytes() + (size_t)FI_NW * FI_BLK * 4 + (size_t)((d + 3) & ~3) * 4 +
                     (size_t)FI_CHUNK * (sizeof(FiUnit) + 2) + 64 + (size_t)((d + 7) & ~7) * 2;
  if (lds > 160 * 1024) return fail(ASL_ERR_CAPACITY, "flat scan: d=%d does not fit LDS", d);
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute((const void *)flat_inv_scan_kernel<FI_CAP, FX, WIDE, SEL, RANGED>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // (the kernel reads the byte table of the fixed-point layout through its table pointer)
  const uint32_t *seg_tab = FX ? reinterpret_cast<const uint32_t *>(P.tab8) : P.tab32;
  const ScanPostFilter pf = rq.post.idpay ? rq.post : ScanPostFilter();
  hipLaunchKernelGGL((flat_inv_scan_kernel<FI_CAP, FX, WIDE, SEL, RANGED>), dim3(rq.nq), dim3(FI_NT), lds, stream(),
                     rq.xq, d, rq.coarse_I, rq.nprobe, P.list_offsets, P.blk_offsets, P.blk_base, seg_tab,
                     P.seg_bytes, P.ids, rq.k, rq.D, rq.I64, rq.I32, rq.set_mode, rq.ent, rq.ent_cnt, P.tab_stride,
                     rq.gate, pf, rq.sel, rq.ranges);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// FX and WIDE of a (FI_CAP, SEL, RANGED) the dispatcher chose; the ranged form has no probes, so it is never WIDE
template <int FI_CAP, bool SEL, bool RANGED>
static int launch_flat_form(bool fx, bool wide, const FlatPostings &P, const FlatScan &rq) {
  if constexpr (!RANGED) {
    if (wide)      // (the one-probe form keeps its registers)
      return fx ? launch_flat_inv<FI_CAP, true, true, SEL, false>(P, rq) : launch_flat_inv<FI_CAP, false, true, SEL, false>(P, rq);
  }
  return fx ? launch_flat_inv<FI_CAP, true, false, SEL, RANGED>(P, rq) : launch_flat_inv<FI_CAP, false, false, SEL, RANGED>(P, rq);
}

// What each form accepts, then the one choice of (FI_CAP, FX, WIDE, SEL, RANGED): 14 instantiations -- plain
// requests at both key capacities, the selector and the ranged form at 2048 keys only (the kernel's static_asserts).
int flat_inv_scan(const FlatPostings &P, const FlatScan &rq) {
  if (rq.nq <= 0) return ASL_OK;
  const bool small = rq.k + FI_NT + 256 <= 2048;      // k <= 1280: the 2048-key buffer, three workgroups per CU
  const bool ranged = rq.ranges.range != nullptr;     // one precursor-ordered list, a run of positions per query
  const bool filtered = rq.post.idpay != nullptr;     // the set-mode finish of the 2048-key instantiations only
  if (ranged && (!small || rq.set_mode == 2 || rq.sel || rq.gate || filtered))
    return fail(ASL_ERR_STATE, "postings scan: the ranged form needs k <= 1280 and rows of ids, and takes no "
                               "selector, gate or post-filter");
  if (!ranged && filtered && !(rq.set_mode == 1 && rq.I32 && small))
    return fail(ASL_ERR_STATE, "postings scan: a post-filter needs set-mode int32 rows and k <= 1280");
  if (!ranged && rq.sel && (!small || rq.set_mode == 2))      // one word per 64 positions of every block (flat_selector)
    return fail(ASL_ERR_STATE, "postings scan: a selector needs k <= 1280 and rows of ids");
  const bool fx = P.layout == 2, wide = rq.nprobe > FI_NT;      // wide: two probes per thread
  if (ranged) return launch_flat_form<2048, false, true>(fx, false, P, rq);
  if (rq.sel) return launch_flat_form<2048, true, false>(fx, wide, P, rq);
  return small ? launch_flat_form<2048, false, false>(fx, wide, P, rq)
               : launch_flat_form<4096, false, false>(fx, wide, P, rq);
}

}  // namespace asl

