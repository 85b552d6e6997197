// rank_scan.hip -- asl_index_rank: where a given library vector stands in the index's neighbour order
// (replaces the measurement of the reference's notebooks/iprg2012_num_candidates.ipynb: IndexFlatIP
// searched with num_neighbors = 1000000, then the position of the brute-force match in that row).
//
// rank = #{ v in scope : key(score(q, v), v) > key(score(q, t), t) }, key = make_key (score desc, id
// asc). The scans run as in a search -- IVF-Flat: the postings walk of flat_inv_scan_kernel, the query's
// non-zeros ascending, acc = fmaf(q_d, val, acc) per posting; IVF-PQ: build_lut_cbt + tile_adc of
// pq_tile.hpp plus the coarse term -- so every score has the bits of the search's; in place of the top-k
// stands one compare with the target's key and the population count of its ballot. Counts are integers:
// any order of summation gives the same answer (per wave in registers, per workgroup in LDS, one
// atomicAdd per workgroup and counter).
//
// Two launches per call. TARGET = true, one workgroup per query: finds the target's slot (inv: id ->
// storage slot), decides whether it is in scope (list probed, key in the window) and scores ITS block
// (tile) with the very routine the count uses -- the target's score comes out of the same device code as
// everybody else's. TARGET = false, grid (query, chunk of lists): every workgroup walks the blocks
// (tiles) of `lists_per_wg` consecutive lists -- of the probe list, or with nprobe = 0 of the index
// itself: the exhaustive scope builds no probe list -- and counts.
#include <algorithm>

#include "common.hpp"
#include "flat_postings.hpp"
#include "ivf_kernels.hpp"
#include "pq_tile.hpp"
#include "topk.hpp"

namespace asl {

constexpr int RK_FLAT_NW = 4;      // waves of a counting workgroup (IVF-Flat): one block per wave at a time
constexpr int RK_FLAT_LISTS = 8;   // lists per workgroup
constexpr int RK_PQ_NW = 8;        // IVF-PQ: 512 threads build the table, one tile per wave at a time
constexpr int RK_PQ_LISTS = 4;     // fewest lists per workgroup (a table per workgroup: see rank_pq)
constexpr int RK_U = 4;            // dimensions whose first row of postings is in flight per wave

// inv[id] = storage slot (list position / tile slot) of vector id; slots without a vector hold id -1
__global__ void rank_invert_kernel(const int32_t *__restrict__ slot_ids, int64_t nslots, int64_t ntotal,
                                   int32_t *__restrict__ inv) {
  const int64_t i = block_linear() * blockDim.x + threadIdx.x;
  if (i >= nslots) return;
  const int32_t id = slot_ids[i];
  if (id >= 0 && id < ntotal) inv[id] = (int32_t)i;
}

// key_slot[slot] = key[id of the slot] (NaN where the slot is empty): the count reads the window column coalesced
__global__ void rank_slot_keys_kernel(const int32_t *__restrict__ slot_ids, int64_t nslots,
                                      const float *__restrict__ key, int64_t ntotal, float *__restrict__ key_slot) {
  const int64_t i = block_linear() * blockDim.x + threadIdx.x;
  if (i >= nslots) return;
  const int32_t id = slot_ids[i];
  key_slot[i] = (id >= 0 && id < ntotal) ? key[id] : __builtin_nanf("");
}

// the l with off[l] <= x < off[l + 1] (0 <= x < off[n]; empty lists are stepped over)
__device__ __forceinline__ int rank_find_list(const int32_t *__restrict__ off, int n, int x) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// is list l among the query's probes? p (wave-uniform): its place in the probe list, or -1
__device__ __forceinline__ int rank_find_probe(const int32_t *__restrict__ probes, int nprobe, int l, int lane) {
  for (int p0 = 0; p0 < nprobe; p0 += 64) {
    const int p = p0 + lane;
    const unsigned long long m = __ballot(p < nprobe && probes[p] == l);
    if (m) return p0 + __builtin_ctzll(m);
  }
  return -1;
}

// key(v) > key(t), over the lanes of a wave: the score's ordered bits decide; ids are fetched only where they tie
__device__ __forceinline__ bool rank_beats(bool in, float score, uint32_t t_ord, uint32_t t_id,
                                           const int32_t *__restrict__ slot_ids, int64_t slot) {
  const uint32_t o = f2ord(score);
  bool gt = in && o > t_ord;
  const bool eq = in && o == t_ord;
  if (__ballot(eq)) {                    // wave-uniform
    if (eq) gt = (uint32_t)slot_ids[slot] < t_id;
  }
  return gt;
}

// the workgroup's two counters -> counts[q][0 .. 1]
__device__ __forceinline__ void rank_add_counts(uint32_t n_rank, uint32_t n_scope, unsigned int *s_cnt, int tid,
                                                unsigned long long *__restrict__ counts, int q) {
  if ((tid & 63) == 0) {
    atomicAdd(&s_cnt[0], n_rank);
    atomicAdd(&s_cnt[1], n_scope);
  }
  __syncthreads();
  if (tid == 0) {
    if (s_cnt[0]) atomicAdd(&counts[(size_t)q * 2], (unsigned long long)s_cnt[0]);
    if (s_cnt[1]) atomicAdd(&counts[(size_t)q * 2 + 1], (unsigned long long)s_cnt[1]);
  }
}

// ---- IVF-Flat, float postings. acc[0 .. nb) of one block for the query's non-zero components (nzd /
// nzv [K], ascending): per vector the ascending-dimension chain acc = fmaf(q_d, val, acc) over the
// dimensions where both factors are non-zero, as flat_inv_scan_kernel forms it (a vector occurs at most
// once per dimension, so the lanes of one step never collide; the steps of a wave reach LDS in program
// order). Lane j of a chunk of 64 dimensions holds dimension j's table word; the first row of postings of
// RK_U dimensions is requested before any is applied, further rows of a long segment follow in place.
__device__ __forceinline__ void rank_flat_block(float *acc, int nb, const uint32_t *__restrict__ erow,
                                                const char *__restrict__ bptr, const uint16_t *nzd,
                                                const float *nzv, int K, int lane) {
  for (int o = lane; o < nb; o += 64) acc[o] = 0.0f;
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int kk = k0 + lane;
    const uint32_t w = kk < K ? erow[nzd[kk]] : 0u;      // the table word (flat_postings.hpp: inv_word); 0 past the end
    const float qv = kk < K ? nzv[kk] : 0.0f;
    const int n = min(64, K - k0);
    for (int j0 = 0; j0 < n; j0 += RK_U) {               // 64 % RK_U == 0: j0 + u stays a lane
      float val[RK_U];
      uint32_t loc[RK_U];
#pragma unroll
      for (int u = 0; u < RK_U; ++u) {
        const uint32_t wj = (uint32_t)__builtin_amdgcn_readlane((int)w, j0 + u);
        const uint32_t st = inv_word_start(wj) * 64u, c = inv_word_count(wj);
        val[u] = 0.0f, loc[u] = 0u;
        if ((uint32_t)lane < c) {
          val[u] = *reinterpret_cast<const float *>(bptr + st + 4u * (uint32_t)lane);
          loc[u] = *reinterpret_cast<const uint16_t *>(bptr + st + 4u * c + 2u * (uint32_t)lane);
        }
      }
#pragma unroll
      for (int u = 0; u < RK_U; ++u) {
        const uint32_t wj = (uint32_t)__builtin_amdgcn_readlane((int)w, j0 + u);
        const uint32_t st = inv_word_start(wj) * 64u, c = inv_word_count(wj);
        const float qj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, qv), j0 + u));
        if ((uint32_t)lane < c) acc[loc[u]] = __builtin_fmaf(qj, val[u], acc[loc[u]]);
        for (uint32_t p = 64u + (uint32_t)lane; p < c; p += 64u) {
          const float v = *reinterpret_cast<const float *>(bptr + st + 4u * p);
          const uint32_t lc = *reinterpret_cast<const uint16_t *>(bptr + st + 4u * c + 2u * p);
          acc[lc] = __builtin_fmaf(qj, v, acc[lc]);
        }
      }
    }
  }
}

template <int NW, bool TARGET>
__global__ __launch_bounds__(64 * NW) void rank_flat_kernel(
    const float *__restrict__ xq, int d, int nlist, int64_t ntotal, const int32_t *__restrict__ coarse_I, int nprobe,
    int lists_per_wg, const int32_t *__restrict__ list_offsets, const int32_t *__restrict__ blk_offsets,
    const uint32_t *__restrict__ blk_base, const uint32_t *__restrict__ seg_tab, const char *__restrict__ seg_bytes,
    const int32_t *__restrict__ ids, const int64_t *__restrict__ target, const int32_t *__restrict__ inv,
    const RankWindow win, unsigned long long *__restrict__ tkey, float *__restrict__ tscore,
    unsigned long long *__restrict__ counts, int want_scope) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *s_acc = reinterpret_cast<float *>(smem);                          // [NW][FI_BLK]
  float *s_nzv = s_acc + NW * FI_BLK;                                      // [d rounded up to 4]
  unsigned int *s_cnt = reinterpret_cast<unsigned int *>(s_nzv + ((d + 3) & ~3));   // rank, scope, K, -
  uint16_t *s_nzd = reinterpret_cast<uint16_t *>(s_cnt + 4);               // [d]
  const int tid = threadIdx.x, lane = tid & 63, q = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned long long tk = TARGET ? 0ull : tkey[q];
  if (!TARGET && tk == 0ull && !want_scope) return;       // not in scope and nobody asks for the scope's size
  // the query's non-zero components, ascending, listed from the dense row (any number of them)
  if (wave == 0) {
    const int base = list_row_nonzeros(xq + (size_t)q * d, d, lane, 1.0f, s_nzd, s_nzv);
    if (lane == 0) {
      s_cnt[0] = 0u, s_cnt[1] = 0u;
      s_cnt[2] = (unsigned int)base;
    }
  }
  __syncthreads();
  const int K = (int)s_cnt[2];
  float *acc = s_acc + wave * FI_BLK;
  const QueryWindow qm = win.key_slot ? query_window(win.q_pmz, q, win.mode) : QueryWindow{0.0, 0.0};
  if constexpr (TARGET) {
    // the target: its position in list order, its list, whether that list is probed and its key in the window
    const int64_t t = target[q];
    unsigned long long key = 0ull;
    float score = __builtin_nanf("");
    const int pos = (t >= 0 && t < ntotal) ? inv[t] : -1;
    if (pos >= 0) {
      const int l = rank_find_list(list_offsets, nlist, pos);
      bool ok = nprobe == 0 || rank_find_probe(coarse_I + (size_t)q * nprobe, nprobe, l, lane) >= 0;
      if (ok && win.key_slot) ok = precursor_ok(qm, win.key_slot[pos], win.charge, win.tol, win.mode);
      if (ok) {                         // wave-uniform
        const int r = pos - list_offsets[l], len = list_offsets[l + 1] - list_offsets[l];
        const int j = r / FI_BLK, blk = blk_offsets[l] + j;
        rank_flat_block(acc, min(FI_BLK, len - j * FI_BLK), seg_tab + (size_t)blk * d,
                        seg_bytes + (size_t)blk_base[blk] * 64, s_nzd, s_nzv, K, lane);
        score = acc[r - j * FI_BLK];
        key = make_key(score, (uint32_t)t);
      }
    }
    if (lane == 0) {
      tkey[q] = key;
      tscore[q] = key ? score : __builtin_nanf("");
    }
  } else {
    const uint32_t t_ord = (uint32_t)(tk >> 32), t_id = key_id(tk);
    const int L = nprobe ? nprobe : nlist;
    const int s0 = (int)blockIdx.y * lists_per_wg, s1 = min(s0 + lists_per_wg, L);
    uint32_t n_rank = 0, n_scope = 0;
    int u0 = 0;                         // blocks of the lists before this one, mod NW: the waves take blocks in turn
    for (int s = s0; s < s1; ++s) {
      const int l = nprobe ? coarse_I[(size_t)q * nprobe + s] : s;
      if (l < 0) continue;
      const int pos_l = list_offsets[l], len = list_offsets[l + 1] - pos_l;
      const int b0 = blk_offsets[l], nblk = blk_offsets[l + 1] - b0;
      for (int j = (wave - u0 + NW) % NW; j < nblk; j += NW) {
        const int blk = b0 + j, nb = min(FI_BLK, len - j * FI_BLK);
        rank_flat_block(acc, nb, seg_tab + (size_t)blk * d, seg_bytes + (size_t)blk_base[blk] * 64, s_nzd, s_nzv, K,
                        lane);
        for (int v0 = 0; v0 < nb; v0 += 64) {      // zero scores count: they are candidates of the dense scan too
          const int v = v0 + lane;
          const int64_t slot = (int64_t)pos_l + (int64_t)j * FI_BLK + v;
          bool in = v < nb;
          if (in && win.key_slot) in = precursor_ok(qm, win.key_slot[slot], win.charge, win.tol, win.mode);
          const float score = v < nb ? acc[v] : 0.0f;
          n_scope += (uint32_t)__popcll(__ballot(in));
          n_rank += (uint32_t)__popcll(__ballot(rank_beats(in, score, t_ord, t_id, ids, slot)));
        }
      }
      u0 = (u0 + nblk) % NW;
    }
    rank_add_counts(tk ? n_rank : 0u, n_scope, s_cnt, tid, counts, q);
  }
}

static size_t rank_flat_lds(int nw, int d) {
  return (size_t)nw * FI_BLK * 4 + (size_t)((d + 3) & ~3) * 4 + 16 + (size_t)((d + 7) & ~7) * 2;
}

int rank_flat(const FlatPostings &P, const float *xq, int nq, int64_t ntotal, const int32_t *coarse_I, int nprobe,
              const int64_t *target, const int32_t *inv, const RankWindow &win, unsigned long long *tkey,
              float *tscore, unsigned long long *counts, int want_scope) {
  if (nq <= 0) return ASL_OK;
  const int d = P.d, nlist = P.nlist;
  if (rank_flat_lds(RK_FLAT_NW, d) > 64 * 1024) return fail(ASL_ERR_CAPACITY, "rank: d=%d does not fit LDS", d);
  const int L = nprobe ? nprobe : nlist;
  const int per = std::max<int>(RK_FLAT_LISTS, (int)cdiv(L, 65535));
#define RK_ARGS xq, d, nlist, ntotal, coarse_I, nprobe, per, P.list_offsets, P.blk_offsets, P.blk_base, P.tab32, \
                P.seg_bytes, P.ids, target, inv, win, tkey, tscore, counts, want_scope
  hipLaunchKernelGGL((rank_flat_kernel<1, true>), dim3(nq), dim3(64), rank_flat_lds(1, d), stream(), RK_ARGS);
  ASL_CHECK_LAUNCH();
  hipLaunchKernelGGL((rank_flat_kernel<RK_FLAT_NW, false>), dim3(nq, (unsigned)cdiv(L, per)), dim3(64 * RK_FLAT_NW),
                     rank_flat_lds(RK_FLAT_NW, d), stream(), RK_ARGS);
#undef RK_ARGS
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// ---- IVF-PQ, tiled layout (m = 32, 8 bits): the table by build_lut_cbt, 64 sums per tile by tile_adc,
// + the coarse term of the tile's list -- the summation tree, and so the bits, of pq_scan_v3_kernel.
// coarse_D [nq, nprobe] beside coarse_I; nprobe = 0: coarse_all [nq, nlist], q . centroid of every list.
template <bool TARGET>
__global__ __launch_bounds__(64 * RK_PQ_NW) void rank_pq_kernel(
    const float *__restrict__ xq, int d, const float *__restrict__ cbT, int dsub, int nlist, int64_t ntotal,
    const float *__restrict__ coarse_D, const int32_t *__restrict__ coarse_I, int nprobe,
    const float *__restrict__ coarse_all, int lists_per_wg, const int32_t *__restrict__ list_offsets,
    const int32_t *__restrict__ tile_offsets, const uint8_t *__restrict__ codes_tiled,
    const int32_t *__restrict__ ids_tiled, const int64_t *__restrict__ target, const int32_t *__restrict__ inv,
    const RankWindow win, unsigned long long *__restrict__ tkey, float *__restrict__ tscore,
    unsigned long long *__restrict__ counts, int want_scope) {
  constexpr int NW = RK_PQ_NW, NT = 64 * NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *s_lut = reinterpret_cast<float *>(smem);                          // [256][32]
  float *s_q = s_lut + PQT_KSUB * PQT_M;                                   // [d rounded up to 4]
  unsigned int *s_cnt = reinterpret_cast<unsigned int *>(s_q + ((d + 3) & ~3));
  uint8_t *s_nz = reinterpret_cast<uint8_t *>(s_cnt + 4);                  // 8 + 2 d bytes
  const int tid = threadIdx.x, lane = tid & 63, q = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned long long tk = TARGET ? 0ull : tkey[q];
  if (!TARGET && tk == 0ull && !want_scope) return;       // (block-uniform: before the table's barriers)
  if (tid == 0) s_cnt[0] = 0u, s_cnt[1] = 0u;
  build_lut_cbt<NT>(xq + (size_t)q * d, d, cbT, dsub, s_q, s_lut, s_nz, tid);      // ends with a barrier
  const char *lut_bytes = reinterpret_cast<const char *>(s_lut);
  const int rho = lane >> 4, j = lane & 15;
  const int ma = (rho & 1) ? j + 16 : j, mb = ma ^ 16;
  const uint32_t offA = (uint32_t)ma * 4u, offB = (uint32_t)mb * 4u;
  const uint32_t chunkA = (uint32_t)(rho * 512 + ma * 16), chunkB = chunkA ^ 256u;
  const QueryWindow qm = win.key_slot ? query_window(win.q_pmz, q, win.mode) : QueryWindow{0.0, 0.0};
  auto tile_scores = [&](int tile, float coarse) -> float {        // lane l: the score of the tile's vector l
    const uint8_t *base = codes_tiled + (size_t)tile * 2048;
    const uint4 A = *reinterpret_cast<const uint4 *>(base + chunkA);
    const uint4 B = *reinterpret_cast<const uint4 *>(base + chunkB);
    return coarse + tile_adc(lut_bytes, A, B, offA, offB);
  };
  if constexpr (TARGET) {
    if (wave != 0) return;
    const int64_t t = target[q];
    unsigned long long key = 0ull;
    float score = __builtin_nanf("");
    const int slot = (t >= 0 && t < ntotal) ? inv[t] : -1;
    if (slot >= 0) {                    // wave-uniform, as everything below
      const int tile = slot >> 6;
      const int l = rank_find_list(tile_offsets, nlist, tile);
      const int p = nprobe ? rank_find_probe(coarse_I + (size_t)q * nprobe, nprobe, l, lane) : 0;
      bool ok = p >= 0;
      if (ok && win.key_slot) ok = precursor_ok(qm, win.key_slot[slot], win.charge, win.tol, win.mode);
      if (ok) {
        const float coarse = nprobe ? coarse_D[(size_t)q * nprobe + p] : coarse_all[(size_t)q * nlist + l];
        score = __shfl(tile_scores(tile, coarse), slot & 63);
        key = make_key(score, (uint32_t)t);
      }
    }
    if (lane == 0) {
      tkey[q] = key;
      tscore[q] = key ? score : __builtin_nanf("");
    }
  } else {
    const uint32_t t_ord = (uint32_t)(tk >> 32), t_id = key_id(tk);
    const int L = nprobe ? nprobe : nlist;
    const int s0 = (int)blockIdx.y * lists_per_wg, s1 = min(s0 + lists_per_wg, L);
    uint32_t n_rank = 0, n_scope = 0;
    int u0 = 0;                         // tiles of the lists before this one, mod NW: the waves take tiles in turn
    for (int s = s0; s < s1; ++s) {
      const int l = nprobe ? coarse_I[(size_t)q * nprobe + s] : s;
      if (l < 0) continue;
      const float coarse = nprobe ? coarse_D[(size_t)q * nprobe + s] : coarse_all[(size_t)q * nlist + l];
      const int len = list_offsets[l + 1] - list_offsets[l], tile0 = tile_offsets[l], nt = (len + 63) >> 6;
      for (int t = (wave - u0 + NW) % NW; t < nt; t += NW) {
        const float score = tile_scores(tile0 + t, coarse);
        const int64_t slot = (int64_t)(tile0 + t) * 64 + lane;
        bool in = lane < len - t * 64;               // the valid lanes of a list's last tile
        if (in && win.key_slot) in = precursor_ok(qm, win.key_slot[slot], win.charge, win.tol, win.mode);
        n_scope += (uint32_t)__popcll(__ballot(in));
        n_rank += (uint32_t)__popcll(__ballot(rank_beats(in, score, t_ord, t_id, ids_tiled, slot)));
      }
      u0 = (u0 + nt) % NW;
    }
    rank_add_counts(tk ? n_rank : 0u, n_scope, s_cnt, tid, counts, q);
  }
}

int rank_pq(const float *xq, int nq, int d, const float *cbT, int dsub, int nlist, int64_t ntotal,
            const float *coarse_D, const int32_t *coarse_I, int nprobe, const float *coarse_all,
            const int32_t *list_offsets, const int32_t *tile_offsets, const uint8_t *codes_tiled,
            const int32_t *ids_tiled, const int64_t *target, const int32_t *inv, const RankWindow &win,
            unsigned long long *tkey, float *tscore, unsigned long long *counts, int want_scope) {
  if (nq <= 0) return ASL_OK;
  if (d != PQT_M * dsub || dsub > 64 || d > 1020)
    return fail(ASL_ERR_CAPACITY, "rank: d=%d does not fit the tiled IVF-PQ scan", d);
  const size_t lds = (size_t)PQT_KSUB * PQT_M * 4 + (size_t)((d + 3) & ~3) * 4 + 16 + (size_t)((8 + 2 * d + 15) & ~15);
  const int L = nprobe ? nprobe : nlist;
  // a table per workgroup (~10 us): as few chunks as still fill the device -- ~2 048 workgroups over all
  // queries --, no fewer than RK_PQ_LISTS lists each
  const int64_t want = std::max<int64_t>(1, cdiv(2048, nq));
  const int chunks = (int)std::min<int64_t>(std::min<int64_t>(want, 65535), std::max<int64_t>(1, L / RK_PQ_LISTS));
  const int per = (int)cdiv(L, chunks);
#define RK_ARGS xq, d, cbT, dsub, nlist, ntotal, coarse_D, coarse_I, nprobe, coarse_all, per, list_offsets, \
                tile_offsets, codes_tiled, ids_tiled, target, inv, win, tkey, tscore, counts, want_scope
  hipLaunchKernelGGL((rank_pq_kernel<true>), dim3(nq), dim3(64 * RK_PQ_NW), lds, stream(), RK_ARGS);
  ASL_CHECK_LAUNCH();
  hipLaunchKernelGGL((rank_pq_kernel<false>), dim3(nq, (unsigned)cdiv(L, per)), dim3(64 * RK_PQ_NW), lds, stream(),
                     RK_ARGS);
#undef RK_ARGS
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// ---- the call's outputs from the target keys and the counters
__global__ void rank_finish_kernel(const unsigned long long *__restrict__ tkey, const float *__restrict__ tscore,
                                   const unsigned long long *__restrict__ counts, int nq, int64_t *__restrict__ rank,
                                   float *__restrict__ score, int64_t *__restrict__ scope) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  rank[q] = tkey[q] ? (int64_t)counts[(size_t)q * 2] : -1;
  if (score) score[q] = tscore[q];
  if (scope) scope[q] = (int64_t)counts[(size_t)q * 2 + 1];
}

int rank_finish(const unsigned long long *tkey, const float *tscore, const unsigned long long *counts, int nq,
                int64_t *rank, float *score, int64_t *scope) {
  if (nq <= 0) return ASL_OK;
  hipLaunchKernelGGL(rank_finish_kernel, dim3((unsigned)cdiv(nq, 256)), dim3(256), 0, stream(), tkey, tscore, counts,
                     nq, rank, score, scope);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

int rank_invert(const int32_t *slot_ids, int64_t nslots, int64_t ntotal, int32_t *inv) {
  if (ntotal > 0) HIP_TRY(hipMemsetAsync(inv, 0xff, (size_t)ntotal * 4, stream()));
  if (nslots <= 0) return ASL_OK;
  hipLaunchKernelGGL(rank_invert_kernel, grid_2d(cdiv(nslots, 256)), dim3(256), 0, stream(), slot_ids, nslots, ntotal,
                     inv);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

int rank_slot_keys(const int32_t *slot_ids, int64_t nslots, const float *key, int64_t ntotal, float *key_slot) {
  if (nslots <= 0) return ASL_OK;
  hipLaunchKernelGGL(rank_slot_keys_kernel, grid_2d(cdiv(nslots, 256)), dim3(256), 0, stream(), slot_ids, nslots, key,
                     ntotal, key_slot);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

}  // namespace asl
