// pq_scan_v3.hip -- IVF-PQ asymmetric-distance scan, m = 32 sub-quantisers of 8 bits, laid out
// for gfx950's LDS: the dominant kernel of the hot path (replaces the list scan inside FAISS'
// IndexIVF*.search, call site /root/reference/src/ann_solo/spectral_library.py:443-444).
//
// Layout (helpers in pq_tile.hpp). "One lane per vector" makes 32 random LUT reads per vector
// hit random LDS banks (~3.5-way conflicts on ds_read_b32); here lanes are SUB-QUANTISERS:
//   * LUT image in LDS: lut[c*32 + m] (row stride 128 B) -> bank == m. A 16-lane row reads 16
//     different m for one code position, the neighbouring row the other 16: every ds_read_b32
//     is bank-conflict-free BY CONSTRUCTION, whatever the codes are.
//   * codes are stored in 64-vector tiles (2 KiB): chunk[rho][m][16 B], the 16 bytes being
//     sub-quantiser m's codes of the row's 16 vectors, permuted b -> b ^ (m & 15). Lane
//     (rho, j) loads the chunks of m = j and m = j + 16 (two coalesced 16-B loads).
//   * register r of lane j then holds p_j(vector r ^ j); four DPP butterflies (row_mirror,
//     row_half_mirror, quad [3,2,1,0], quad [1,0,3,2]) reduce the 16x16 block with 15
//     v_add_dpp and NO selects, leaving vector j's sum in lane j -- the canonical mirror tree
//     of DESIGN.md, bit-identical to the oracle.
//   * ids are fetched only for the survivors of the top-k.
//
// Top-k without sorting while streaming (hist_topk.hpp). Only the k-th best SCORE is needed
// while scanning, so the kernel keeps
//   * hist[512]: counts of the appended candidates per score bucket (monotone linear
//     bucketing of the fp32 score over [-0.25, 1), i.e. 0.0024 per bucket),
//   * bstar: the highest bucket with at least k appended candidates at or above it.
// A candidate whose bucket is below bstar can never be among the k best (k candidates
// with strictly larger scores exist), so it is dropped without being stored; when the key
// buffer runs full it is COMPACTED by the same test (one prefix scan, no sort). The k
// best are sorted exactly once, at the end, after the storage slots of the survivors
// have been turned into ids -- (score desc, id asc), identical to the oracle.
// If compaction cannot free the buffer (thousands of bit-identical scores) the kernel
// switches, for that query, to exact sort-and-truncate flushes.
// The waves append on their own (one reservation per tile that holds a candidate) and meet only
// when the key buffer is full and at the end of a table chunk; the histogram is brought up to
// date where it is read, in that sync (see "free-running appends" in the kernel).
//
// What a wave scans. The tile-major, window and selected instantiations fill a table of tiles (256
// per chunk, 168 with a window) and a wave walks the entries wave, wave + 8, ... of it. The
// sub-quantiser-major instantiations (MM) keep one entry per PROBE instead (128 per chunk: nprobe <=
// 128 is one chunk per query, no scan of tile counts, no refill) and hand the lists out whole by a
// ticket counter; a tile's entry is scalar arithmetic on the list's (see "whole lists per wave").
// A plain request with nprobe < 32 takes the tile-major instantiation (pq_scan_v3()).
//
// LDS: LUT 32 KB + key buffer (2048 or 4096 keys) + histogram + tile / probe table (2 KB) => three
// (two) workgroups of 8 waves per CU.
#include "common.hpp"
#include "hist_topk.hpp"
#include "ivf_kernels.hpp"
#include "pq_tile.hpp"

namespace asl {

constexpr int V3_CHUNK = 256;   // tile-table entries per chunk
// Tuning constants of the code stream (scripts/build_variant.sh rewrites them for same-box A/Bs;
// profiles/r06_pq_beyond_llc_*: measured both where the codes sit in the Infinity Cache and where
// they come from DRAM).
constexpr int V3_DEPTH = 1;     // rounds of tiles in flight ahead of the one being scored
constexpr int V3_NT = 0;        // 1: non-temporal loads of the codes (streamed once per query; MM: the buffer loads' nt bit)
constexpr int V3_AHEAD = 8;     // tile_adc: LUT reads in flight ahead of the first-level adds (8: all 32; pq_tile.hpp)
// MM: buffer offset of a lane whose sub-quantiser is dead. A raw buffer (no stride, no index) returns 0 for every
// dword whose byte offset is not below the resource's num_records - 3 and sends no request for it; the resource of a
// tile is smaller than 2^32 - 4096 bytes (32 * mm_plane < 2^32, a multiple of 4096), so the four dwords of a 16-byte
// load at this offset -- 16-byte aligned, ...f0 to ...fc, no 32-bit wrap -- are all out of range, and with
// num_records = 0 (a fetch past the end of a wave's share) so is every offset.
constexpr uint32_t V3_MM_DEAD = 0xfffffff0u;
// Measurement builds only (scripts/build_variant.sh V3_PAD_SALU=16 ...; profiles/pq_tile_step_sensitivity.txt): N
// independent scalar / full-rate vector instructions more per tile step, on registers of their own, behind the
// ADC. What a step's time gains per added instruction is what removing one of that kind is worth. 0: nothing.
constexpr int V3_PAD_SALU = 0;
constexpr int V3_PAD_VALU = 0;
#define V3_PAD4(op) op " %0, 0\n\t" op " %1, 1\n\t" op " %2, 2\n\t" op " %3, 3\n\t"
#define V3_PAD16(op) V3_PAD4(op) V3_PAD4(op) V3_PAD4(op) V3_PAD4(op)
template <int NS_, int NV_>
__device__ __forceinline__ void v3_pad() {
  // (16 instructions per statement: the compiler puts an s_nop behind every asm statement)
  static_assert(NS_ % 16 == 0 && NV_ % 16 == 0, "the padding comes in blocks of 16 instructions");
#pragma unroll
  for (int n = 0; n < NS_ / 16; ++n) {
    uint32_t a, b, c, d;
    asm volatile(V3_PAD16("s_mov_b32") : "=s"(a), "=s"(b), "=s"(c), "=s"(d));
  }
#pragma unroll
  for (int n = 0; n < NV_ / 16; ++n) {
    uint32_t a, b, c, d;
    asm volatile(V3_PAD16("v_mov_b32") : "=v"(a), "=v"(b), "=v"(c), "=v"(d));
  }
}
#undef V3_PAD16
#undef V3_PAD4
// V3_PAD_LDSRT = N (profiles/pq_passer_path_price.txt): N LDS round trips more per hot-loop step, one after the
// other, behind the ADC -- a control word of the workgroup read, waited for and consumed by a v_readfirstlane, the
// next read's address held back until then. What a step's time gains per round trip is what the append's wait for
// its reservation costs, and what answering it a tile later could save. 0: nothing.
constexpr int V3_PAD_LDSRT = 0;
template <int N_>
__device__ __forceinline__ void v3_pad_ldsrt(const int *word) {
  if constexpr (N_ > 0) {
    typedef __attribute__((address_space(3))) int lds_int;
    uint32_t a = (uint32_t)(uintptr_t)(const lds_int *)word;
#pragma unroll
    for (int n = 0; n < N_; ++n) {
      const int r = __builtin_amdgcn_readfirstlane(
          __hip_atomic_load((const lds_int *)(uintptr_t)a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
      asm volatile("" : "+v"(a) : "s"(r));
    }
  }
}
constexpr int V3_WAVES_PER_SIMD = 6;   // occupancy the 2048-key instantiation is compiled for (3 workgroups per CU)

template <int NT_>
__device__ __forceinline__ uint4 load_codes16(const uint8_t *p) {
  if (NT_) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(p);
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(w));
    return make_uint4(v.x, v.y, v.z, v.w);
  }
  return *reinterpret_cast<const uint4 *>(p);
}

// LDS tile-table entry, 8 bytes: tile index (26 bits: ids are int32, so an index holds fewer
// than 2^25 + nlist tiles) | nvalid - 1 (6 bits), coarse term. Half the size of TileEnt: 256
// entries per chunk in the same 2 KB, i.e. half as many pipeline restarts (7.05 -> 6.84 ms).
struct TileEnt8 {
  uint32_t tile_nv;
  float coarse;
};

// The RANGED instantiations (asl_index_search_window / window scan of asl_search_batch)
// scan, of each probed list of the window-ordered layout, only the run [lo, hi) of the vectors that
// pass the query's precursor window: its tiles, the first of them from lane lo & 63 on, the last up to
// lane (hi - 1) & 63. TileEnt8 has no bit left for a first lane, so the entry is 12 bytes, and a chunk
// holds 168 of them (21 rounds of 8 tiles) in the 2 KB the 256 entries of TileEnt8 take: the workgroup
// keeps the LDS of the 2048-key instantiation to the byte (53 504 B, three per CU within 160 KiB
// whatever the allocation granule); only the table is refilled 1.5 times as often.
struct TileEnt12 {
  uint32_t tile_nv;   // tile (26 bits) | end lane - 1 (6 bits), as TileEnt8
  float coarse;
  uint32_t first;     // first lane of the run in this tile (0 except in the run's first tile)
};
constexpr int V3_CHUNK_RANGED = 168;
static_assert(V3_CHUNK_RANGED * sizeof(TileEnt12) <= V3_CHUNK * sizeof(TileEnt8), "the ranged table fits the 2 KB");

// The MM instantiations keep no tile table: a tile's index (tile0 + local), its coarse term (the list's) and its
// count (64 except in the list's last tile) follow from 12 bytes per PROBE, all of it wave-uniform. The table
// holds one entry per probe, 128 of them in the same 2 KB: nprobe <= 128 is one chunk per query, and a wave
// takes whole lists from it by a ticket counter (see "whole lists per wave" in the kernel).
struct ProbeEnt {
  uint32_t tile0;     // the list's first tile
  int32_t len;        // its vectors; 0: not probed (l < 0) or empty, skipped by the walk
  float coarse;
  uint32_t pad;
};
constexpr int V3_CHUNK_PROBES = 128;
static_assert(V3_CHUNK_PROBES * sizeof(ProbeEnt) <= V3_CHUNK * sizeof(TileEnt8), "the probe table fits the 2 KB");

// NW = waves per workgroup. LDS (LUT 32 KB + keys 16 KB + ...) allows three workgroups per CU
// whatever their size, so 8 waves per workgroup (one tile per wave and round) double the
// waves that share one LUT and one key buffer: 24 waves per CU at 80 VGPRs instead of 12 at
// 157 -- measured 8.28 -> 7.46 ms at the bench config (with ONE round of prefetch: at this
// occupancy the second prefetch stage only costs registers).
// RANGED: the tile table comes from rg.range instead of the whole lists (see TileEnt12)
// SEL (asl_index_search_selected, a library's selection; the 2048-key instantiations only): sel holds one
// 64-bit word per tile of the layout scanned, bit v = vector v of the tile is selected (padding slots are
// not). The word comes in with the tile's table entry -- the tile index is wave-uniform, so it is a scalar
// load into two scalar registers -- and is one more term of append()'s `in`: an unselected vector is scored
// like any other and never offered, so the k best are chosen among the selected vectors alone. Reservation,
// refused-tile retry, exact flushes and both finishes are those of the plain instantiations.
// MM (the plain instantiations only; index_codes_mmajor): codes_tiled is the SUB-QUANTISER-MAJOR copy --
// plane m, mm_plane bytes each, holds sub-quantiser m's 64 bytes of every tile, tile after tile, in the tile's
// own row order and byte permutation -- so a 128-byte line holds one sub-quantiser only, and a lane whose
// sub-quantiser has no non-zero query component (its LUT column is +0.0 whatever the code) fetches nothing: its
// buffer load is out of range and returns zeros, and the sums are those of the tile-major scan bit for bit.
template <int CAP, int T, int NW, int DEPTH, bool WIDE, bool RANGED = false, bool SEL = false, bool MM = false>
__global__ __launch_bounds__(64 * NW, (NW == 8 ? (CAP <= 2048 ? V3_WAVES_PER_SIMD : 4) : (CAP <= 2048 ? 3 : 1))) void pq_scan_v3_kernel(
    const float *__restrict__ xq, int d, const float *__restrict__ codebooks, int dsub,
    const float *__restrict__ coarse_D, const int32_t *__restrict__ coarse_I, int nprobe,
    const int32_t *__restrict__ list_offsets, const int32_t *__restrict__ tile_offsets,
    const uint8_t *__restrict__ codes_tiled, const int32_t *__restrict__ ids_tiled, int k,
    float *__restrict__ D, int64_t *__restrict__ I64, int32_t *__restrict__ I32, int set_mode,
    const uint2 *__restrict__ ent, const int32_t *__restrict__ ent_cnt, const int *__restrict__ gate,
    const ScanPostFilter pf, const ScanRanges rg, const unsigned long long *__restrict__ sel, const uint32_t mm_plane) {
  static_assert(!SEL || CAP <= 2048, "the selector is built into the 2048-key instantiations only");
  static_assert(!MM || (!RANGED && !SEL), "the sub-quantiser-major copy exists of the default layout only");
  // gate: a device-side row count -- workgroups past it leave at once (a launch of fixed size over
  // a list whose length only the device knows: the shard-side rescans of exchange.hip)
  if (gate && (int)blockIdx.x >= *gate) return;
  static_assert(DEPTH >= 1 && DEPTH <= 3, "rounds of prefetch");
  static_assert(T == 1, "one tile per wave at a time (two lost on registers: profiles/HISTORY.md)");
  constexpr int NT = 64 * NW, ROUND_VECS = NW * 64;
  using TopK = HistTopK<CAP, ROUND_VECS, NT>;
  using Ent = typename std::conditional<RANGED, TileEnt12, typename std::conditional<MM, ProbeEnt, TileEnt8>::type>::type;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *s_lut = reinterpret_cast<float *>(smem + TopK::lds_bytes());
  Ent *table = reinterpret_cast<Ent *>(s_lut + PQT_KSUB * PQT_M);
  float *s_q = reinterpret_cast<float *>(smem);  // aliases the key buffer during the LUT build

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.x;
  // ---- my probe (thread p < nprobe; WIDE: probes p and p + NT -- nprobe up to 2 x NT = 1024, the
  // reference's clamp, spectral_library.py:77-81): its dependent gathers are issued before the
  // table build and complete under it
  constexpr int PP = WIDE ? 2 : 1;
  int my_len[PP], my_tile0[PP], my_nt[PP], my_pre[PP];
  float my_coarse[PP];
#pragma unroll
  for (int pp = 0; pp < PP; ++pp) {
    my_len[pp] = 0, my_tile0[pp] = 0, my_nt[pp] = 0, my_coarse[pp] = 0.0f;
    const int p = tid + pp * NT;
    if (p < nprobe) {
      const int l = coarse_I[(size_t)q * nprobe + p];
      if (l >= 0) {
        if constexpr (RANGED) {
          // the run [lo, hi) of the list, counted from lane 0 of the tile that holds lo: the tile
          // count and the end lane of every tile follow from my_len as for a whole list
          const int2 r = rg.range[(size_t)q * nprobe + p];
          // (the first lane of the run's first tile rides in the six bits a tile index leaves free: a register less)
          my_len[pp] = r.y > r.x ? r.y - (r.x & ~63) : 0;
          my_tile0[pp] = (int)((uint32_t)(tile_offsets[l] + (r.x >> 6)) | ((uint32_t)(r.x & 63) << 26));
        } else {
          my_len[pp] = list_offsets[l + 1] - list_offsets[l];
          my_tile0[pp] = tile_offsets[l];
        }
        if constexpr (!MM) my_nt[pp] = (my_len[pp] + 63) >> 6;
        my_coarse[pp] = coarse_D[(size_t)q * nprobe + p];
      }
    }
  }
  build_lut_cbt<NT>(xq + (size_t)q * d, d, codebooks, dsub, s_q, s_lut, reinterpret_cast<uint8_t *>(table),
                    tid, ent ? ent + (size_t)q * 64 : nullptr,
                    ent ? (xq ? ent_cnt[q] : max(ent_cnt[q], 0)) : -1);  // codebooks = cbT[m][t][c]; the tile table is
                                                                        // not live yet; entry lists only: a row with
                                                                        // more than 64 non-zeros is searched as all-zero

  // MM: the sub-quantisers that have a non-zero query component, from the list the table build walked
  // (K entries, nz_m at +8 of its scratch, which is the tile table's memory and dies with the scan below)
  uint32_t live_u = 0;
  if constexpr (MM) {
    const uint8_t *s_nz = reinterpret_cast<const uint8_t *>(table);
    const int K = reinterpret_cast<const int *>(s_nz)[0];
    uint32_t mine = 0;
    for (int i = tid & 63; i < K; i += 64) mine |= 1u << (s_nz[8 + i] & 31);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine |= (uint32_t)__shfl_xor((int)mine, o);
    live_u = (uint32_t)__builtin_amdgcn_readfirstlane((int)mine);
    __syncthreads();
  }

  // ---- exclusive scan of the probes' tile counts (probe order: p, then p + NT)
  // (MM: the table is per probe -- nothing to scan, `total` counts probes)
  int total = MM ? nprobe : 0;
  if constexpr (!MM) {
    int *scan_part = reinterpret_cast<int *>(table);   // table is not live yet
#pragma unroll
    for (int pp = 0; pp < PP; ++pp) {
      int part_total;
      my_pre[pp] = total + block_excl_scan<NW>(my_nt[pp], scan_part, tid, part_total);
      total += part_total;
      __syncthreads();
    }
    total = __builtin_amdgcn_readfirstlane(total);   // the same in every thread: the loops below are scalar
  }

  TopK top;   // init zeroes the keys (which aliased s_q)
  top.init(smem, k, ids_tiled, tid);
  top.out_keys = set_mode == 2 && I64 != nullptr;

  const char *lut_bytes = reinterpret_cast<const char *>(s_lut);
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int rho = lane >> 4, j = lane & 15;
  const int ma = (rho & 1) ? j + 16 : j, mb = ma ^ 16;
  const uint32_t offA = (uint32_t)ma * 4u, offB = (uint32_t)mb * 4u;
  // lane part of a tile's two code loads: tile-major rho * 512 + m * 16; MM: plane m, row rho
  // MM: every lane issues both loads of a tile -- a load under `if (live)` leaves the number of loads in flight
  // unknown to the compiler, which then waits for all of them right behind their issue, see the tile loop -- as
  // buffer loads whose resource ends with the copy: a dead lane's offset lies beyond it, so the hardware returns
  // zeros and fetches nothing. Its LUT column is +0.0 whatever the bytes. (32 * mm_plane < 2^32, index_codes_mmajor,
  // a multiple of 4096: every live offset and the remaining size fit 32 bits, and V3_MM_DEAD is beyond any size.)
  const bool liveA = (live_u >> ma) & 1u, liveB = (live_u >> mb) & 1u;      // (MM only)
  const uint32_t chunkA = MM ? (liveA ? (uint32_t)ma * mm_plane + (uint32_t)(rho * 16) : V3_MM_DEAD) : (uint32_t)(rho * 512 + ma * 16);
  const uint32_t chunkB = liveB ? (uint32_t)mb * mm_plane + (uint32_t)(rho * 16) : V3_MM_DEAD;   // (MM only)

  // ---- free-running appends (HistTopK's free_* protocol, as in flat_scan.hip: flat_inv_scan_kernel) -----
  // A wave walks its own share of a table chunk (entries wave, wave + NW, ...) with its own register
  // prefetch pipeline and appends what passes the threshold with one reservation per tile; the waves
  // meet only when the key buffer is full (a sync) and at the end of a chunk. The histogram is not
  // touched per tile: the sync counts what was appended since the last one (lazy counts).
  //
  // The tile loop rotates the register sets of the prefetch pipeline by unrolling, in TWO places. The hot
  // loop holds the steps and the usual append: per tile the flag and table entry, the fetch, the ADC, one
  // compare, one ballot and one scalar test "anything to do?" (a passer, the flag, exact flushes in use), which
  // falls through; a tile with passers and nothing else reserves and writes its keys right there (with the
  // threshold moving only in a sync, about one vector of a 64-vector tile still passes at the end of a scan:
  // such a tile is the rule, profiles/HISTORY.md). A wave leaves the hot loop when the flag is up, exact flushes
  // are in use or its reservation was refused, deals with that tile off the loop, and walks the rest of
  // the rotation there, a step at a time with the append behind each, so that the hot loop always starts at
  // set 0. The sync has ONE place, behind both (free_sync inlines a compaction and a sort: a copy per register
  // set cost the instantiations their registers). A wave that has to meet the others -- its reservation was
  // refused, or the flag is up -- moves the tile in flight to set 0, joins the sync, offers a refused tile
  // again (its scores wait in a register) against the new threshold, and starts the rotation over.
  //
  // No deadlock, whatever the data: the workgroup's barriers are (a) the fixed sequence of one
  // sync and (b) the one barrier that ends a chunk. A wave enters (a) only with the flag raised --
  // by itself, right before its first barrier, or seen raised by another wave, which is then on its
  // way to that barrier and waits there -- and the flag is lowered behind the first barrier of the
  // sequence, before the barriers of free_sync, so no wave sees it raised once the sync is over
  // (a value read ahead of the sync is dropped in it). Every wave looks at the flag with every tile --
  // every step reads it, in the hot loop and off it, and the value read is part of the hot loop's one test,
  // ahead of the append there, and of the test behind every append off it -- and in the wait at the end of its share, so every wave joins
  // every sync. A wave enters (b) only after s_done says that all NW waves have finished their share of
  // this chunk; a wave counts itself finished once, when the hot loop ends with no entry left and no
  // reservation pending; a finished wave raises the flag only to join, and each request of an unfinished
  // wave was answered by a complete sync before that wave could finish, so at that point no sync is open or
  // can open. The retry of a refused tile ends: a sync leaves at least ROUND_VECS = NW * 64 free slots.
  // MM, whole lists by ticket: the ticket counter adds no wait -- taking a ticket is one atomic add, which
  // always returns, and the walk over empty entries ends because every round takes a higher ticket. "No entry
  // left" is then: a ticket at or past the chunk's probe count was drawn (every later one is too: the counter
  // only grows until thread 0 clears it between the chunk's two barriers, where no wave draws), both list
  // sets are empty and no tile is in flight; a wave in that state draws no further ticket, fetches nothing
  // and scores nothing, so it counts itself finished once and stays finished, and (a), (b) stand as above.
  // The table is read only through tickets below the probe count, i.e. entries written before the barrier
  // behind the fill; the last read of a chunk's table precedes its reader's count in s_done.
  int *s_flag = top.ctl + TopK::C_USER;            // a wave asks for a sync (C_USER is free until finish_set)
  int *s_done = top.ctl + TopK::C_USER + 1;        // waves that finished their share, summed over the chunks
  int *s_ticket = top.ctl + TopK::C_USER + 2;      // MM: the chunk's next list to hand out (cleared per chunk)
  if (tid == 0) {
    *s_flag = 0;
    *s_done = 0;
  }
  // (relaxed workgroup-scope accesses: plain LDS reads and writes that the compiler neither caches nor merges)
  auto flag_up = [&]() -> int { return __hip_atomic_load(s_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
  auto flag_set = [&](int v) { __hip_atomic_store(s_flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
  // the threshold snapshot, wave-uniform: it only changes inside a sync
  float thr_u = -INFINITY;
  uint32_t thr_hi_u = 0;          // != 0 exactly while exact flushes are in use (a flush then leaves k keys)
  int flag_u = 0;

  constexpr int CHUNK = RANGED ? V3_CHUNK_RANGED : MM ? V3_CHUNK_PROBES : V3_CHUNK;
  for (int c0 = 0; c0 < total; c0 += CHUNK) {
    if constexpr (MM) {
      // the probes [c0, c0 + CHUNK) of the query: thread p writes its own probe's entry, one 16-byte store
      // (a probe past nprobe, with l < 0 or of an empty list has len 0); the tickets start over
#pragma unroll
      for (int pp = 0; pp < PP; ++pp) {
        const uint32_t local = (uint32_t)(tid + pp * NT - c0);
        if (local < (uint32_t)CHUNK)
          *reinterpret_cast<uint4 *>(&table[local]) =
              make_uint4((uint32_t)my_tile0[pp], (uint32_t)my_len[pp], __float_as_uint(my_coarse[pp]), 0u);
      }
      if (tid == 0) __hip_atomic_store(s_ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if constexpr (!MM) {
#pragma unroll
      for (int pp = 0; pp < PP; ++pp) {
        // (my probe as values of their own: what the fill derives from them is made here, once per chunk,
        // not kept in registers across the tile loop)
        // (the probe's tile count is made again from its length here: a register less across the tile loop)
        asm volatile("" : "+v"(my_pre[pp]), "+v"(my_tile0[pp]), "+v"(my_len[pp]));
        const int lo = max(my_pre[pp], c0), hi = min(my_pre[pp] + ((my_len[pp] + 63) >> 6), c0 + CHUNK);
        for (int t = lo; t < hi; ++t) {
          const int local = t - my_pre[pp];
          Ent e;
          const uint32_t tile0 = RANGED ? (uint32_t)my_tile0[pp] & 0x3ffffffu : (uint32_t)my_tile0[pp];
          e.tile_nv = (tile0 + (uint32_t)local) | ((uint32_t)(min(64, my_len[pp] - local * 64) - 1) << 26);
          e.coarse = my_coarse[pp];
          if constexpr (RANGED) e.first = local == 0 ? (uint32_t)my_tile0[pp] >> 26 : 0u;
          table[t - c0] = e;
        }
      }
    }
    __syncthreads();
    const int nent = min(CHUNK, total - c0);
    // Register pipeline over my wave's entries, DEPTH tiles deep (the codes of the next DEPTH tiles
    // are in flight while one is scored). DEPTH + 1 register sets; `set` says which holds the tile to
    // score, and the step is instantiated per set, so every register index is a compile-time constant.
    constexpr int NS = DEPTH + 1;
    uint4 A[NS], B[NS];
    if constexpr (MM) {   // (defined bytes in the sets of a wave that has no entry in this chunk)
#pragma unroll
      for (int s = 0; s < NS; ++s) A[s] = B[s] = make_uint4(0u, 0u, 0u, 0u);
    }
    struct Tile {         // the entry is the same for the whole wave: scalar registers
      uint32_t tile_nv;   // tile | last lane << 26
      float coarse;
      uint32_t first;     // RANGED: first lane
      unsigned long long sel;   // SEL: the tile's selector word
    } e[NS];
    // The two code loads of tile en.tile_nv. num_records: the resource's size, 0 for a fetch past the wave's last
    // tile (MM only -- the loads are issued all the same, of an empty resource: every lane out of range, nothing
    // fetched).
    auto load_tile = [&](uint4 &a, uint4 &b, const Tile &en, uint32_t num_records) {
      // the tile's address is a scalar and the lane's part a 32-bit offset of its own: the loads take
      // them as they are (scalar base + lane offset), no 64-bit lane addresses to keep or add up per tile
      // (the second chunk's offset is made here from the first: a lane constant less to keep)
      if constexpr (MM) {
        const uint32_t toff = (en.tile_nv & 0x3ffffffu) * 64u;
        const uint8_t *base = codes_tiled + (size_t)toff;
        // (the resource: from the tile's first plane-0 byte on, raw, no stride. Its size is the whole copy's,
        // 32 * mm_plane, for every tile -- not the bytes left behind this tile, a subtraction per tile: a live
        // lane's offset is below 31 * mm_plane + 64, so what it reads lies inside the copy, tile + 64 <= mm_plane,
        // and V3_MM_DEAD is beyond 32 * mm_plane all the same)
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(base), 0, (int)num_records, 0x00020000);
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 va = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)chunkA, 0, V3_NT ? 2 : 0);   // (aux bit 1: nt)
        const u32x4 vb = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)chunkB, 0, V3_NT ? 2 : 0);
        a = make_uint4(va.x, va.y, va.z, va.w);
        b = make_uint4(vb.x, vb.y, vb.z, vb.w);
      } else {
        const uint8_t *base = codes_tiled + (size_t)(en.tile_nv & 0x3ffffffu) * 2048;
        uint32_t offa = chunkA;
        asm volatile("" : "+v"(offa));
        const uint32_t offb = offa ^ 256u;       // mb = ma ^ 16
        a = load_codes16<V3_NT>(base + offa);
        b = load_codes16<V3_NT>(base + offb);
      }
    };
    // Tile table (not MM): the entry to fetch is read at a running LDS address (a lane register that a step
    // advances by its wave's stride), not at an index turned into an address per tile.
    auto fetch = [&](uint32_t taddr, uint4 &a, uint4 &b, Tile &en) {
      // (tile_nv, coarse: one 8-byte read -- the table is 16-byte aligned, an entry 8 or 12 bytes long)
      typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
      const u32x2 t = *(const __attribute__((address_space(3))) u32x2 *)(uintptr_t)taddr;
      en.tile_nv = __builtin_amdgcn_readfirstlane(t.x);
      en.coarse = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane((int)t.y));
      if constexpr (RANGED)
        en.first = __builtin_amdgcn_readfirstlane(*(const __attribute__((address_space(3))) uint32_t *)(uintptr_t)(taddr + 8u));
      if constexpr (SEL) en.sel = sel[en.tile_nv & 0x3ffffffu];   // (a scalar load: the tile is wave-uniform)
      load_tile(a, b, en, 0u);
    };
    constexpr uint32_t ENT_STRIDE = NW * sizeof(Ent);   // from one entry of a wave to its next
    const uint32_t mm_size = (uint32_t)PQT_M * mm_plane;
    // ---- whole lists per wave (MM) ------------------------------------------------------------------------
    // The lists of a chunk are handed out whole, in probe order (best coarse score first), by the ticket
    // counter: a wave that needs a list takes the next ticket -- one lane's add, as HistTopK::reserve_add --
    // and reads that probe's entry; a ticket at or past the chunk's probe count means no list is left, an
    // entry of len 0 is skipped by taking the next ticket. A wave holds two lists as scalars -- (next tile,
    // tiles left, coarse, last tile's count - 1) of the one it fetches from and of the one it takes up next --
    // and draws the ticket for the second when it starts fetching the first, so neither LDS round trip is
    // waited for with no code load in flight. A tile's entry is scalar arithmetic on the first set; left == 0
    // there says that the wave has nothing left to fetch in this chunk.
    uint32_t cur_tile = 0, cur_last = 0, nx_tile = 0, nx_last = 0;
    int cur_left = 0, nx_left = 0;
    float cur_coarse = 0.0f, nx_coarse = 0.0f;
    int inflight = 0;             // tiles fetched and not yet scored
    auto take_list = [&]() {      // the look-ahead list: the next non-empty one, or none (nx_left == 0)
      typedef __attribute__((address_space(3))) int lds_int;
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      nx_left = 0;
      nx_tile = 0;                // (a valid tile for the fetches past the end, which read nothing)
      for (;;) {                  // wave-uniform
        // (the address as a lane value: the atomic optimizer leaves such an add alone, see reserve_add)
        uint32_t ta = (uint32_t)(uintptr_t)(lds_int *)s_ticket;
        asm volatile("" : "+v"(ta));
        int t = (int)ta;
        if (lane == 0)
          t = __hip_atomic_fetch_add((lds_int *)(uintptr_t)ta, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        t = __builtin_amdgcn_readfirstlane(t);
        if (t >= nent) break;
        const u32x4 v = *(const __attribute__((address_space(3))) u32x4 *)(uintptr_t)(
            (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char *)reinterpret_cast<const char *>(table) +
            (uint32_t)t * (uint32_t)sizeof(ProbeEnt));
        const int len = __builtin_amdgcn_readfirstlane((int)v.y);
        if (len > 0) {
          nx_tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)v.x);
          nx_coarse = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane((int)v.z));
          nx_left = (len + 63) >> 6;
          nx_last = (uint32_t)(len - 1) & 63u;
          break;
        }
      }
    };
    auto next_list = [&]() {      // the look-ahead list becomes the current one; the ticket for the one behind it
      cur_tile = nx_tile, cur_left = nx_left, cur_coarse = nx_coarse, cur_last = nx_last;
      if (cur_left != 0) take_list();
    };
    // Fetch my next tile (its entry made here), or -- nothing left -- any valid tile with an empty resource:
    // the loads issued per step stay a compile-time count. The list advance is a wave-uniform branch, taken
    // about every eighth tile. Counts the tile in `inflight`.
    auto fetch_mm = [&](uint4 &a, uint4 &b, Tile &en) {
      const bool real = cur_left != 0;
      en.tile_nv = cur_tile | ((cur_left == 1 ? cur_last : 63u) << 26);
      en.coarse = cur_coarse;
      load_tile(a, b, en, real ? mm_size : 0u);
      if (real) {
        ++inflight;
        ++cur_tile;
        if (--cur_left == 0) next_list();
      }
    };
    // the tile whose candidates are offered: its scores and (scalar) its entry
    float p_score = 0.0f;
    uint32_t p_tile_nv = 0, p_first = 0;
    unsigned long long p_sel = 0;
    bool pending = false;
    // The lanes that hold a vector to offer, as a scalar mask: lane <= end (RANGED: and lane >= first; SEL: and
    // selected). (A 64-bit shift takes the low six bits of its count: ~end is 63 - end there.)
    auto in_mask = [&]() -> unsigned long long {
      unsigned long long in = ~0ull >> (~(p_tile_nv >> 26) & 63u);
      if constexpr (RANGED) in &= ~0ull << (p_first & 63u);
      if constexpr (SEL) in &= p_sel;
      return in;
    };
    // A tile costs the ADC, one compare against the snapshot and the scalar AND with in_mask; everything
    // else is on the path a tile without a passer never enters.
    auto passers = [&]() -> unsigned long long { return __ballot(p_score >= thr_u) & in_mask(); };
    // The rare path: m = passers(). While exact flushes are in use (thr_hi_u != 0, wave-uniform) the
    // test is the ordered key's and m is made again; the ordered key of the lanes that pass is made in
    // free_write. The reservation's verdict is settled before the lanes part to write their keys:
    // `pending` stays a scalar, and with it every branch of the wave's loop.
    // The reservation (hist_topk.hpp: one lane's add on C_FILL, refused when it ends beyond CAP) is spelled out
    // here: the verdict is an add, a compare and the branch, with no -1 to encode and decode in between.
    // hot: the hot loop's call -- thresholded, and m != 0 is known from its one test.
    auto append = [&](unsigned long long m, bool hot = false) {
      if (!hot && thr_hi_u != 0) {
        float sc = p_score;
        asm volatile("; exact flushes" : "+v"(sc));
        m = __ballot(f2ord(sc) >= thr_hi_u) & in_mask();
      }
      pending = false;
      if (hot || m) {
        const int c = __builtin_amdgcn_readfirstlane(__popcll(m));   // wave-uniform
        const int base = top.reserve_add(c);
        pending = base + c > CAP;                                    // the buffer cannot take them: nothing is written
        if (!pending) top.free_write(__builtin_amdgcn_inverse_ballot_w64(m), m, p_score, (p_tile_nv << 6) + (uint32_t)lane, base, false);
      }
    };
    const uint32_t table_lds = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char *)reinterpret_cast<const char *>(table);
    int i = wave_u;               // my next entry; between syncs its codes are in set 0, the next tiles' behind
    if constexpr (MM) {           // my first two lists, and the first tiles in flight
      take_list();
      next_list();
#pragma unroll
      for (int s = 0; s < DEPTH; ++s)
        if (cur_left != 0) fetch_mm(A[s], B[s], e[s]);
    } else if (i < nent) {
      uint32_t t0 = table_lds + (uint32_t)i * (uint32_t)sizeof(Ent);
      asm volatile("" : "+v"(t0));
#pragma unroll
      for (int s = 0; s < DEPTH; ++s)
        if (i + s * NW < nent) fetch(t0 + s * ENT_STRIDE, A[s], B[s], e[s]);
    }
    // a tile to score in the set the rotation is at? (MM: a tile in flight; else: an entry of my share left)
    auto more = [&]() -> bool { return MM ? inflight != 0 : i < nent; };
    // One step: the flag is read (and, with a tile table, the next entry: one LDS wait for both), the next tile's
    // codes fetched, the tile in set s scored. taddr: the LDS address of the entry fetched last.
    // MM: the fetch is unconditional -- with no tile left, of any valid tile with an empty
    // resource, never scored -- so the loads issued per step are a compile-time count and the wait in front of
    // the ADC leaves this step's two in flight under it (vmcnt(3) / vmcnt(2); the older pair is waited for
    // before the issue). The other instantiations keep the conditional fetch and with it the full wait behind
    // their loads: the counted form measured slower there (profiles/HISTORY.md, "PQ scan: counted prefetch").
    uint32_t taddr = 0;
    auto step = [&](int s) {
      const int f = (s + DEPTH) % NS;
      const int fl = flag_up();
      if constexpr (MM) {
        fetch_mm(A[f], B[f], e[f]);
        --inflight;               // (the tile scored below)
        asm volatile("" : "+s"(inflight));   // (a count in a scalar register, not a lane mask made of `real`)
      } else if (i + DEPTH * NW < nent) {
        taddr += ENT_STRIDE;
        fetch(taddr, A[f], B[f], e[f]);
      }
      flag_u = __builtin_amdgcn_readfirstlane(fl);
      p_score = e[s].coarse + tile_adc<V3_AHEAD>(lut_bytes, A[s], B[s], offA, offB);
      p_tile_nv = e[s].tile_nv;
      if constexpr (RANGED) p_first = e[s].first;
      if constexpr (SEL) p_sel = e[s].sel;
      i += NW;
    };
    // The hot loop: the rotation of the register sets from set 0 on. Per step ONE scalar test -- a passer, the
    // flag, exact flushes in use: anything to do? -- which falls through for a tile without a passer, and the
    // test for the end of the share, which is the back edge. A tile with passers and nothing else is appended
    // here, by the thresholded test alone. Returns -1 at the end of the share; s if the tile of set s (it is
    // scored: p_score) is still to be offered -- the flag is up or exact flushes are in use --; s + NS if it
    // was offered here and refused (`pending`).
    auto hot = [&]() -> int {
      for (;;) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          if (!more()) return -1;
          step(s);
          v3_pad<V3_PAD_SALU, V3_PAD_VALU>();
          v3_pad_ldsrt<V3_PAD_LDSRT>(s_done);
          const unsigned long long m = passers();
          if (__builtin_expect(((uint32_t)m | (uint32_t)(m >> 32) | (uint32_t)flag_u | thr_hi_u) != 0u, 0)) {
            if (((uint32_t)flag_u | thr_hi_u) != 0u) return s;
            append(m, true);              // the usual case: a passer, nothing else
            if (pending) return s + NS;   // refused: offered already, to the sync
          }
        }
      }
    };
    bool finished = false;
    for (;;) {                    // every condition below is wave-uniform
      // (the entry fetched last is DEPTH - 1 strides ahead of i; where that is past the share, no entry is
      // fetched any more and the address only has to be one of the table)
      if constexpr (!MM) {
        taddr = table_lds + (uint32_t)(DEPTH == 1 ? min(i, CHUNK - 1) : min(i + (DEPTH - 1) * NW, nent - 1)) * (uint32_t)sizeof(Ent);
        asm volatile("" : "+v"(taddr));
      }
      int ev = hot();
      asm volatile("" : "+s"(ev));          // (one way out of the hot loop, whatever is made of ev below)
      bool meet = false;
      // Off the hot loop: the tile of set ev % NS is appended (unless it was, and was refused), then the rest of
      // the rotation is walked here, a step at a time, so that the hot loop always starts at set 0. A wave that has to meet the others --
      // its reservation was refused, or the flag is up -- moves the tiles in flight to the front sets
      // (register moves, once per sync) and goes to the sync.
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (ev < 0 || s < ev % NS || meet) continue;
        if (s > ev % NS) {
          if (!more()) continue;
          step(s);
        }
        if (!(ev >= NS && s == ev % NS)) append(passers());   // (ev >= NS: offered in the hot loop and refused)
        if (pending || flag_u) {
          meet = true;
          if (s + 1 < NS) {
#pragma unroll
            for (int u = 0; u < DEPTH; ++u) {
              A[u] = A[(s + 1 + u) % NS];
              B[u] = B[(s + 1 + u) % NS];
              e[u] = e[(s + 1 + u) % NS];
            }
          }
        }
      }
      if (ev >= 0 && !meet) continue;
      if (!meet) {
        // my share is done: wait for the other waves, joining the syncs they ask for
        if (!finished) {
          if (lane == 0) atomicAdd(s_done, 1);
          finished = true;
        }
        for (;;) {
          flag_u = __builtin_amdgcn_readfirstlane(flag_up());
          if (flag_u ||
              __builtin_amdgcn_readfirstlane(__hip_atomic_load(s_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) >=
                  NW * (c0 / CHUNK + 1))
            break;
          __builtin_amdgcn_s_sleep(4);
        }
        if (!flag_u) break;       // the chunk is done
      }
      do {                        // raise the flag, meet the other waves, count, compact; a refused tile again
        if (lane == 0) flag_set(1);
        __syncthreads();
        if (tid == 0) flag_set(0);
        // (the thread index as a value of its own: what the compaction and the sort derive from it --
        // addresses, wave predicates -- is then made here, not kept in registers across the tile loop)
        asm volatile("" : "+v"(top.tid));
        top.free_sync(true);
        thr_u = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, top.thr_f)));
        thr_hi_u = (uint32_t)__builtin_amdgcn_readfirstlane((int)top.thr_hi);
        flag_u = 0;               // read before this sync
        if (pending) append(passers());
      } while (pending);
    }
    __syncthreads();
  }
  top.free_done(true);
  if constexpr (RANGED) {
    // set mode: the row holds in-window hits only, so its length goes to the rescoring as it is
    // (rescore.hip: prefiltered rows; -1 after exact flushes: the row is -1 padded and the
    // rescoring's own filter, which every hit passes, finds its end)
    if (set_mode) {
      const int n = top.finish_set(D ? D + (size_t)q * k : nullptr, I64 ? I64 + (size_t)q * k : nullptr,
                                   I32 ? I32 + (size_t)q * k : nullptr, reinterpret_cast<u64 *>(s_lut));
      if (rg.row_len && tid == 0) rg.row_len[q] = n;
    } else {
      top.finish(D ? D + (size_t)q * k : nullptr, I64 ? I64 + (size_t)q * k : nullptr,
                 I32 ? I32 + (size_t)q * k : nullptr);
    }
  } else if (set_mode && CAP * 9 <= PQT_KSUB * PQT_M * 4)   // unordered exact top-k; the LUT is dead: scratch
    top.finish_set(D ? D + (size_t)q * k : nullptr, I64 ? I64 + (size_t)q * k : nullptr,
                   I32 ? I32 + (size_t)q * k : nullptr, reinterpret_cast<u64 *>(s_lut), &pf, q);
  else if (set_mode && CAP * 8 <= PQT_KSUB * PQT_M * 4)
    top.finish_set(D ? D + (size_t)q * k : nullptr, I64 ? I64 + (size_t)q * k : nullptr,
                   I32 ? I32 + (size_t)q * k : nullptr, reinterpret_cast<u64 *>(s_lut));
  else
    top.finish(D ? D + (size_t)q * k : nullptr, I64 ? I64 + (size_t)q * k : nullptr,
               I32 ? I32 + (size_t)q * k : nullptr);
}

template <int CAP, int T, int NW, int DEPTH, bool WIDE, bool RANGED = false, bool SEL = false, bool MM = false>
static int launch_v3(const float *xq, int nq, int d, const float *codebooks, int dsub,
                     const float *coarse_D, const int32_t *coarse_I, int nprobe,
                     const int32_t *list_offsets, const int32_t *tile_offsets,
                     const uint8_t *codes_tiled, const int32_t *ids_tiled, int k, float *D,
                     int64_t *I64, int32_t *I32, int set_mode, const uint2 *ent,
                     const int32_t *ent_cnt, const int *gate, const ScanPostFilter &pf,
                     const ScanRanges &rg, const unsigned long long *sel = nullptr, uint32_t mm_plane = 0) {
  // (the ranged table -- V3_CHUNK_RANGED entries of TileEnt12 -- fits the same bytes)
  constexpr size_t TABLE = RANGED ? V3_CHUNK_RANGED * sizeof(TileEnt12) : V3_CHUNK * sizeof(TileEnt8);
  if ((size_t)d * 4 > (size_t)CAP * 8 || dsub > 64 || (size_t)d * 2 + 8 > TABLE || d != PQT_M * dsub)
    return fail(ASL_ERR_CAPACITY, "pq scan: d=%d too large for the LDS staging", d);
  const size_t lds = HistTopK<CAP, NW * T * 64, 64 * NW>::lds_bytes() + (size_t)PQT_KSUB * PQT_M * 4 +
                     (size_t)V3_CHUNK * sizeof(TileEnt8);
  if (lds > 160 * 1024) return fail(ASL_ERR_CAPACITY, "pq scan: k=%d does not fit LDS", k);
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute((const void *)pq_scan_v3_kernel<CAP, T, NW, DEPTH, WIDE, RANGED, SEL, MM>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((pq_scan_v3_kernel<CAP, T, NW, DEPTH, WIDE, RANGED, SEL, MM>), dim3(nq), dim3(64 * NW), lds, stream(),
                     xq, d, codebooks, dsub, coarse_D, coarse_I, nprobe, list_offsets, tile_offsets,
                     codes_tiled, ids_tiled, k, D, I64, I32, set_mode, ent, ent_cnt, gate, pf, rg, sel, mm_plane);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

bool pq_scan_tiled_supported(int m, int ksub, int k, int nprobe) {
  return m == PQT_M && ksub == PQT_KSUB && nprobe <= 1024 && k >= 1 && k <= TK_MAX_K;
}

// k <= 1280: 2048-key buffer, three workgroups per CU; larger k: 4096 keys, two per CU
int pq_scan_v3(const float *xq, int nq, int d, const float *codebooks, int dsub,
               const float *coarse_D, const int32_t *coarse_I, int nprobe,
               const int32_t *list_offsets, const int32_t *tile_offsets,
               const uint8_t *codes_tiled, const int32_t *ids_tiled, int k, float *D,
               int64_t *I64, int32_t *I32, int set_mode, const uint2 *ent, const int32_t *ent_cnt,
               const int *gate, const ScanPostFilter *post, const ScanRanges *ranges,
               const unsigned long long *sel, const uint8_t *codes_mm, uint32_t mm_plane) {
  if (nq <= 0) return ASL_OK;
  // the post-filter needs the set-mode finish of the 2048-key instantiation (its scratch behind the keys)
  ScanPostFilter pf;
  if (post && post->idpay) {
    if (!(set_mode == 1 && I32 && k + 256 + 512 <= 2048))
      return fail(ASL_ERR_STATE, "pq scan: a post-filter needs set-mode int32 rows and k <= 1280");
    pf = *post;
  }
  const ScanRanges none;
#define V3_ARGS xq, nq, d, codebooks, dsub, coarse_D, coarse_I, nprobe, list_offsets, tile_offsets, \
                codes_tiled, ids_tiled, k, D, I64, I32, set_mode, ent, ent_cnt, gate, pf
  if (sel && (set_mode == 2 || k + 256 + 512 > 2048))
    return fail(ASL_ERR_STATE, "pq scan: a selector needs k <= 1280 and rows of ids");
  if (ranges && ranges->range) {   // the window-ordered layout, one run per probed list
    if (pf.idpay || set_mode == 2 || k + 256 + 512 > 2048)
      return fail(ASL_ERR_STATE, "pq scan: the window scan needs k <= 1280, rows of ids and no post-filter");
    if (sel) {                     // (sel: one word per tile of THAT layout)
      if (nprobe > 512) return launch_v3<2048, 1, 8, V3_DEPTH, true, true, true>(V3_ARGS, *ranges, sel);
      return launch_v3<2048, 1, 8, V3_DEPTH, false, true, true>(V3_ARGS, *ranges, sel);
    }
    if (nprobe > 512) return launch_v3<2048, 1, 8, V3_DEPTH, true, true>(V3_ARGS, *ranges);
    return launch_v3<2048, 1, 8, V3_DEPTH, false, true>(V3_ARGS, *ranges);
  }
  if (sel) {
    if (nprobe > 512) return launch_v3<2048, 1, 8, V3_DEPTH, true, false, true>(V3_ARGS, none, sel);
    return launch_v3<2048, 1, 8, V3_DEPTH, false, false, true>(V3_ARGS, none, sel);
  }
  // the sub-quantiser-major copy: plain requests (the caller gives it to no other). Its instantiations hand
  // out whole lists: with fewer than four lists per wave (nprobe < 32) that leaves waves idle, the strided
  // tile table does not, and such scans are short -- they take the tile-major instantiation below.
  if (codes_mm && !gate && nprobe >= 32) {
#define V3_MM_ARGS xq, nq, d, codebooks, dsub, coarse_D, coarse_I, nprobe, list_offsets, tile_offsets, \
                   codes_mm, ids_tiled, k, D, I64, I32, set_mode, ent, ent_cnt, gate, pf, none, nullptr, mm_plane
    if (nprobe > 512) {
      if (k + 256 + 512 <= 2048) return launch_v3<2048, 1, 8, V3_DEPTH, true, false, false, true>(V3_MM_ARGS);
      return launch_v3<4096, 1, 8, V3_DEPTH, true, false, false, true>(V3_MM_ARGS);
    }
    if (k + 256 + 512 <= 2048) return launch_v3<2048, 1, 8, V3_DEPTH, false, false, false, true>(V3_MM_ARGS);
    return launch_v3<4096, 1, 8, V3_DEPTH, false, false, false, true>(V3_MM_ARGS);
#undef V3_MM_ARGS
  }
  if (nprobe > 512) {         // two probes per thread (the one-probe form keeps its registers)
    if (k + 256 + 512 <= 2048) return launch_v3<2048, 1, 8, V3_DEPTH, true>(V3_ARGS, none);
    return launch_v3<4096, 1, 8, V3_DEPTH, true>(V3_ARGS, none);
  }
  if (k + 256 + 512 <= 2048) return launch_v3<2048, 1, 8, V3_DEPTH, false>(V3_ARGS, none);
  return launch_v3<4096, 1, 8, V3_DEPTH, false>(V3_ARGS, none);
#undef V3_ARGS
}

// [lo, hi) per (query, probe): the positions of the probed list, in the window-ordered layout (keys
// ascending, NaN last), whose key passes the query's window -- two binary searches with precursor_ok
// itself as the predicate, so the run holds exactly the vectors the reference's filter keeps (a
// precomputed interval q +- tol / z would round differently at its edges). The run is contiguous:
// left of the query's m/z, fabs(q - l) is a correctly rounded difference, non-increasing as l grows,
// and so are its product with the charge and its quotient by the growing l (ppm); right of it the
// same terms are non-decreasing (l - q is exact up to l = 2q, Sterbenz; beyond that a float32 step
// of l is still far above the double rounding of l - q). Correctly rounded operations are monotone,
// so on either side the predicate changes value once. NaN keys (sorted last) never pass.
// ASL_TOL_INTERVAL (q_pmz: [nq, 2]): the same walk is lower_bound(lo) and upper_bound(hi) -- the first
// search ends at the first key >= lo, the right-hand one at the first key from there that is not <= hi.
// acc (optional): += sum of hi - lo (asl_profile_scanned_vectors).
__global__ void window_ranges_kernel(const double *__restrict__ q_pmz, int nq,
                                     const int32_t *__restrict__ coarse_I, int nprobe,
                                     const int32_t *__restrict__ list_offsets,
                                     const int32_t *__restrict__ tile_offsets,
                                     const float *__restrict__ wkey, int charge, double tol, int mode,
                                     int2 *__restrict__ ranges, unsigned long long *__restrict__ acc) {
  const int64_t i = block_linear() * blockDim.x + threadIdx.x;
  unsigned long long cnt = 0;
  if (i < (int64_t)nq * nprobe) {
    const int l = coarse_I[i];
    int2 r = make_int2(0, 0);
    if (l >= 0) {
      const float *key = wkey + (size_t)tile_offsets[l] * 64;
      const int n = list_offsets[l + 1] - list_offsets[l];
      r = window_run(key, n, query_window(q_pmz, i / nprobe, mode), charge, tol, mode);
      cnt = (unsigned long long)(r.y - r.x);
    }
    ranges[i] = r;
  }
  if (acc) {
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(acc, cnt);
  }
}

int window_ranges(const double *q_pmz, int nq, const int32_t *coarse_I, int nprobe,
                  const int32_t *list_offsets, const int32_t *tile_offsets, const float *wkey, int charge,
                  double tol, int mode, int2 *ranges, unsigned long long *acc) {
  const int64_t n = (int64_t)nq * nprobe;
  if (n <= 0) return ASL_OK;
  hipLaunchKernelGGL(window_ranges_kernel, grid_2d(cdiv(n, 256)), dim3(256), 0, stream(), q_pmz, nq, coarse_I,
                     nprobe, list_offsets, tile_offsets, wkey, charge, tol, mode, ranges, acc);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// list-ordered codes [n,32] -> 64-vector tiles (see file header); dst_slot[i] = tile*64 + v
__global__ void tile_codes_kernel(const uint8_t *__restrict__ codes, const int32_t *__restrict__ ids,
                                  const int32_t *__restrict__ dst_slot, int64_t n,
                                  uint8_t *__restrict__ codes_tiled,
                                  int32_t *__restrict__ ids_tiled) {
  const int64_t t = block_linear() * blockDim.x + threadIdx.x;
  if (t >= n * PQT_M) return;
  const int64_t i = t >> 5;
  const int m = (int)(t & 31);
  const int32_t slot = dst_slot[i];
  const int64_t tile = slot >> 6;
  const int v = slot & 63, rho = v >> 4, b = (v & 15) ^ (m & 15);
  codes_tiled[tile * 2048 + rho * 512 + m * 16 + b] = codes[t];
  if (m == 0) ids_tiled[tile * 64 + v] = ids[i];
}

int tile_codes(const uint8_t *codes, const int32_t *ids, const int32_t *dst_slot, int64_t n,
               int64_t ntiles, uint8_t *codes_tiled, int32_t *ids_tiled) {
  HIP_TRY(hipMemsetAsync(codes_tiled, 0, (size_t)ntiles * 2048, stream()));
  HIP_TRY(hipMemsetAsync(ids_tiled, 0xff, (size_t)ntiles * 64 * 4, stream()));
  if (n <= 0) return ASL_OK;
  hipLaunchKernelGGL(tile_codes_kernel, grid_2d(cdiv(n * PQT_M, 256)), dim3(256), 0,
                     stream(), codes, ids, dst_slot, n, codes_tiled, ids_tiled);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// tile-major codes -> the sub-quantiser-major copy (MM above): one thread per 16-byte chunk (tile, rho, m)
__global__ void mmajor_codes_kernel(const uint4 *__restrict__ codes_tiled, int64_t ntiles, uint32_t plane,
                                    uint8_t *__restrict__ codes_mm) {
  const int64_t t = block_linear() * blockDim.x + threadIdx.x;
  if (t >= ntiles * 128) return;
  const int64_t tile = t >> 7;
  const int rho = (int)(t >> 5) & 3, m = (int)(t & 31);
  *reinterpret_cast<uint4 *>(codes_mm + (size_t)m * plane + (size_t)tile * 64 + rho * 16) = codes_tiled[t];
}

int mmajor_codes(const uint8_t *codes_tiled, int64_t ntiles, uint32_t plane, uint8_t *codes_mm) {
  HIP_TRY(hipMemsetAsync(codes_mm, 0, (size_t)plane * PQT_M, stream()));
  if (ntiles <= 0) return ASL_OK;
  hipLaunchKernelGGL(mmajor_codes_kernel, grid_2d(cdiv(ntiles * 128, 256)), dim3(256), 0, stream(),
                     reinterpret_cast<const uint4 *>(codes_tiled), ntiles, plane, codes_mm);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// ---- selector words of a tiled layout (SEL above): one wave per tile gathers keep[id] through the layout's
// slot ids and ballots; a padding slot (id -1) or an id outside [0, n) is unselected
__global__ __launch_bounds__(256) void tile_selector_kernel(const int32_t *__restrict__ slot_ids, int64_t ntiles,
                                                            const uint8_t *__restrict__ keep, int64_t n,
                                                            unsigned long long *__restrict__ words) {
  const int64_t tile = block_linear() * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (tile >= ntiles) return;          // (wave-uniform)
  const int32_t id = slot_ids[tile * 64 + lane];
  const unsigned long long m = __ballot(id >= 0 && id < n && keep[id] != 0);
  if (lane == 0) words[tile] = m;
}

int tile_selector(const int32_t *slot_ids, int64_t ntiles, const uint8_t *keep, int64_t n,
                  unsigned long long *words) {
  if (ntiles <= 0) return ASL_OK;
  hipLaunchKernelGGL(tile_selector_kernel, grid_2d(cdiv(ntiles, 4)), dim3(256), 0, stream(), slot_ids, ntiles,
                     keep, n, words);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

}  // namespace asl
