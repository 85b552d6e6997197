// ivf_kernels.hip -- the generic device kernels of SEARCHING the hand-written IVF index (what builds one is in
// quantizer.hip; the tiled IVF-PQ scan, the postings scan, the re-rank, the exchange and the rank scan have units
// of their own).
//
//   wave_select_kernel exact top-k of a SHORT score row held in one wave's registers (the coarse
//                     top-nprobe of nlist): one histogram pass, one small sort, no workgroup barrier
//   row_topk_kernel   exact streaming top-k of one score row per workgroup (IndexFlatIP,
//                     long rows, and IVF-Flat through a probed-list bitmap mask)
//   topk_merge_hist_kernel / topk_merge_kernel  merge of per-shard partial top-k lists
//                     ((score, id) pairs or packed 64-bit keys), histogram-threshold selection
//   probe_bitmap_kernel  the probed lists of a query as a bitmap (row_topk_kernel's mask)
//   gather_rows_f32_kernel / gather_rows_u8_kernel  row gathers
//   pq_lut_kernel     the ADC look-up table of a query (build_lut_lds), written out
//   pq_scan_kernel    the IVF-PQ scan of every PQ shape: per-query ADC look-up table built in LDS,
//                     the packed PQ codes of the probed lists streamed from HBM (adc_score), fused exact top-k
//   scanned_count_kernel  sum of the probed lists' lengths (the work counter of a scan)
#include <algorithm>
#include <type_traits>

#include "common.hpp"
#include "ivf_kernels.hpp"
#include "hist_topk.hpp"
#include "topk.hpp"

namespace asl {

// ------------------------------------------------------------------ row top-k
// scores: [rows, ld]; hit id of column c is ids ? ids[c] : id_base + c.
// Mask (IVF-Flat): column c is visible to row r iff bit vlist[c] of bitmap[r] is set.
__global__ __launch_bounds__(TK_NT) void row_topk_kernel(
    const float *__restrict__ scores, int64_t ld, int n, int k, int cap,
    const int32_t *__restrict__ ids, int32_t id_base, const int32_t *__restrict__ vlist,
    const uint32_t *__restrict__ bitmap, int bitmap_words, float *__restrict__ D,
    int64_t *__restrict__ I64, int32_t *__restrict__ I32, int64_t out_ld,
    const u64 *__restrict__ upper_in, u64 *__restrict__ upper_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u64 *buf = reinterpret_cast<u64 *>(smem);
  u64 *thr = buf + cap;
  int *ctl = reinterpret_cast<int *>(thr + 1);
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  StreamTopK<TK_NT> tk;
  tk.init(buf, ctl, thr, cap, k, tid);
  const float *row = scores + (size_t)r * ld;
  const uint32_t *bm = bitmap ? bitmap + (size_t)r * bitmap_words : nullptr;
  // bounded pass (k beyond the LDS top-k, index.hip: search_large_k): only keys strictly below
  // the row's bound take part -- the keys at or above it were emitted by the earlier passes
  const u64 ub = upper_in ? upper_in[r] : ~0ull;
  for (int base = 0; base < n; base += TK_NT) {
    const int c = base + tid;
    u64 key = 0ull;
    if (c < n) {
      bool vis = true;
      if (bm) {
        const int l = vlist[c];
        vis = (bm[l >> 5] >> (l & 31)) & 1u;
      }
      if (vis) key = make_key(row[c], (uint32_t)(ids ? ids[c] : id_base + c));
      if (key >= ub) key = 0ull;
    }
    tk.push(key, tid);
  }
  tk.finish(D ? D + (size_t)r * out_ld : nullptr, I64 ? I64 + (size_t)r * out_ld : nullptr,
            I32 ? I32 + (size_t)r * out_ld : nullptr, tid);
  // the next pass's bound: the smallest key of a FULL row (0 = the row is exhausted: nothing passes)
  if (upper_out && tid == 0) upper_out[r] = ctl[0] >= k ? buf[k - 1] : 0ull;
}

// Short rows (n <= 4096, k <= 256; the coarse quantiser's top-nprobe of nlist): ONE WAVE per row, four
// rows per workgroup and no workgroup barrier anywhere, so a wave on the rare path never holds up its
// neighbours. The row sits in the wave's registers (CH * 4 values a lane; 16-byte loads where the row's
// address allows). One histogram pass over [row min, row max] in wave-private LDS finds the bucket of the
// k-th score; the <= SEL_CAP keys at or above it are compacted (v_mbcnt) and sorted inside the wave.
// A row whose threshold bucket is overfull (mass ties: an all-zero query scores every centroid 0; a range
// that overflows fp32) is refined inside the wave: further histogram passes over the 64-bit KEYS of the
// bucket's own range, 9 bits a pass. Keys are unique, so the passes end (at the latest with one key per
// bucket), and among equal scores the lower id is the larger key: ties resolve in column order.
constexpr int SEL_VPT = 16, SEL_CAP = 512, SEL_NB = 512;
constexpr int SEL_WAVES = TK_NT / 64;   // rows per workgroup

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// min and max over the wave (every source lane of these DPP patterns is inside its row), wave-uniform
__device__ __forceinline__ void wave_minmax(float &lo, float &hi) {
  lo = fminf(lo, dpp_f32<0xB1>(lo));    // quad_perm [1,0,3,2]
  hi = fmaxf(hi, dpp_f32<0xB1>(hi));
  lo = fminf(lo, dpp_f32<0x4E>(lo));    // quad_perm [2,3,0,1]
  hi = fmaxf(hi, dpp_f32<0x4E>(hi));
  lo = fminf(lo, dpp_f32<0x141>(lo));   // row_half_mirror
  hi = fmaxf(hi, dpp_f32<0x141>(hi));
  lo = fminf(lo, dpp_f32<0x140>(lo));   // row_mirror
  hi = fmaxf(hi, dpp_f32<0x140>(hi));
  float l4[4], h4[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    l4[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lo), 16 * i));
    h4[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hi), 16 * i));
  }
  lo = fminf(fminf(l4[0], l4[1]), fminf(l4[2], l4[3]));
  hi = fmaxf(fmaxf(h4[0], h4[1]), fmaxf(h4[2], h4[3]));
}

struct SelThr {
  int b, ge, gt;   // the threshold bucket, the values at or above it, the values above it
};

// The highest bucket of the wave's histogram with >= need values at or above it (lane t owns the eight
// buckets SEL_NB-8-8t .. SEL_NB-1-8t; suffix sums inside the wave). Fewer than `need` values in all:
// bucket 0, everything at or above it.
__device__ __forceinline__ SelThr wave_threshold(const int *hist, int lane, int need) {
  const int first = SEL_NB - 8 - 8 * lane;
  const int4 a = *reinterpret_cast<const int4 *>(hist + first);
  const int4 c = *reinterpret_cast<const int4 *>(hist + first + 4);
  const int h[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
  const int s = ((h[0] + h[1]) + (h[2] + h[3])) + ((h[4] + h[5]) + (h[6] + h[7]));
  int incl = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  int acc = incl - s, b = 0, ge = 0, gt = 0;
  const bool mine = acc < need && incl >= need;
  bool done = false;
#pragma unroll
  for (int i = 7; i >= 0; --i) {
    const int nxt = acc + h[i];
    if (!done && nxt >= need) {
      b = first + i;
      ge = nxt;
      gt = acc;
      done = true;
    }
    acc = nxt;
  }
  const u64 m = __ballot(mine);
  SelThr t;
  if (m == 0ull) {
    t.b = 0;
    t.ge = __builtin_amdgcn_readlane(incl, 63);
    t.gt = 0;
  } else {
    const int src = __ffsll((long long)m) - 1;
    t.b = __builtin_amdgcn_readlane(b, src);
    t.ge = __builtin_amdgcn_readlane(ge, src);
    t.gt = __builtin_amdgcn_readlane(gt, src);
  }
  return t;
}

__device__ __forceinline__ void wave_hist_clear(int *hist, int lane) {
  wave_lds_sync();   // other lanes' reads of the last pass stay in front of the stores
  reinterpret_cast<int4 *>(hist)[2 * lane] = make_int4(0, 0, 0, 0);
  reinterpret_cast<int4 *>(hist)[2 * lane + 1] = make_int4(0, 0, 0, 0);
  wave_lds_sync();
}

// CH: 16-byte chunks a lane holds (value j of a lane is column ((j / 4) * 64 + lane) * 4 + j % 4).
// FULL: n == CH * 256 and every row 16-byte aligned: no column is out of range, no load is narrow.
template <int CH, bool FULL>
__global__ __launch_bounds__(TK_NT, 4) void wave_select_kernel(
    const float *__restrict__ scores, int64_t ld, int rows, int n, int k, float *__restrict__ D,
    int64_t *__restrict__ I64, int32_t *__restrict__ I32, int64_t out_ld) {
  constexpr int NV = CH * 4;
  __shared__ __attribute__((aligned(16))) int s_hist[SEL_WAVES][SEL_NB];
  __shared__ __attribute__((aligned(16))) u64 s_buf[SEL_WAVES][SEL_CAP];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = blockIdx.x * SEL_WAVES + wave;
  if (r >= rows) return;      // wave-uniform; nothing below waits for another wave
  int *hist = s_hist[wave];
  u64 *buf = s_buf[wave];
  const float *row = scores + (size_t)r * ld;
  const int c0 = lane * 4;    // column of the lane's value e of chunk u: c0 + u * 256 + e
  // n or ld not a multiple of 4: every second row starts off a 16-byte boundary and loads by the value
  const bool wide = FULL || (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  auto chunk = [&](int u, float *x) {
    const int c = c0 + u * 256;
    if (FULL || (wide && c + 3 < n)) {
      const float4 t = *reinterpret_cast<const float4 *>(row + c);
      x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = c + e < n ? row[c + e] : 0.0f;
    }
  };
  auto col = [&](int j) { return c0 + (j >> 2) * 256 + (j & 3); };
  auto valid = [&](int c) { return FULL || c < n; };

  float v[NV];
#pragma unroll
  for (int u = 0; u < CH; ++u) chunk(u, v + 4 * u);
  float lo = 3.402823466e+38f, hi = -3.402823466e+38f;
#pragma unroll
  for (int j = 0; j < NV; ++j)
    if (valid(col(j))) {
      lo = fminf(lo, v[j]);
      hi = fmaxf(hi, v[j]);
    }
  wave_minmax(lo, hi);
  const float scale = hi > lo ? (float)(SEL_NB - 1) / (hi - lo) : 0.0f;   // monotone in the score
  // The bucket of a value is recomputed where it is needed (three instructions) and not kept: the second
  // pass reads lo and scale through an empty asm, or the compiler would hold 64 buckets a lane.
  float plo = lo, pscale = scale;
  auto bucket = [&](float x) {
    const float t = fminf(fmaxf((x - plo) * pscale, 0.0f), (float)(SEL_NB - 1));
    return (int)t;
  };
  wave_hist_clear(hist, lane);
#pragma unroll
  for (int j = 0; j < NV; ++j)
    if (valid(col(j))) atomicAdd(&hist[bucket(v[j])], 1);
  wave_lds_sync();
  const SelThr th = wave_threshold(hist, lane, k);

  // compaction of the selected values' keys, any order: position = keys so far + v_mbcnt of the ballot
  int total = 0;
  auto append = [&](float x, int c, bool sel) {
    const u64 m = __ballot(sel);
    const int pos = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, total));
    if (sel && pos < SEL_CAP) buf[pos] = make_key(x, (uint32_t)c);
    total += __popcll(m);
  };
  asm volatile("" : "+v"(plo), "+v"(pscale));
  if (th.ge <= SEL_CAP) {     // wave-uniform; the usual case
#pragma unroll
    for (int j = 0; j < NV; ++j) append(v[j], col(j), valid(col(j)) && bucket(v[j]) >= th.b);
  } else {
    // The threshold bucket is overfull: the th.gt values above it are in; the rest come from the bucket, by
    // histogram passes over its keys' own range [klo, khi]. Rare, so these passes read the row again (it is
    // in the cache) in rolled loops and keep the registers of the usual path out of scratch.
    int in = th.gt;
    u64 klo = ~0ull, khi = 0ull;
#pragma nounroll
    for (int u = 0; u < CH; ++u) {
      float x[4];
      chunk(u, x);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c0 + u * 256 + e;
        const u64 key = make_key(x[e], (uint32_t)c);
        if (valid(c) && bucket(x[e]) == th.b) {
          klo = key < klo ? key : klo;
          khi = key > khi ? key : khi;
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const u64 a = __shfl_xor(klo, o, 64), c = __shfl_xor(khi, o, 64);
      klo = a < klo ? a : klo;
      khi = c > khi ? c : khi;
    }
    u64 kthr;
#pragma nounroll
    for (;;) {
      const u64 range = khi - klo;
      const int sh = (range >> 9) ? 64 - 9 - __clzll((long long)range) : 0;   // (range >> sh) < SEL_NB
      wave_hist_clear(hist, lane);
#pragma nounroll
      for (int u = 0; u < CH; ++u) {
        float x[4];
        chunk(u, x);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = c0 + u * 256 + e;
          const u64 key = make_key(x[e], (uint32_t)c);
          if (valid(c) && key >= klo && key <= khi) atomicAdd(&hist[(int)((key - klo) >> sh)], 1);
        }
      }
      wave_lds_sync();
      const SelThr t2 = wave_threshold(hist, lane, k - in);
      kthr = klo + ((u64)t2.b << sh);
      if (in + t2.ge <= SEL_CAP) break;
      // still overfull: sh > 0 here (a bucket of single keys holds one), and the next range is 2^sh wide
      in += t2.gt;
      klo = kthr;
      const u64 top = kthr + ((1ull << sh) - 1ull);
      khi = top < khi ? top : khi;
      wave_lds_sync();
    }
#pragma nounroll
    for (int u = 0; u < CH; ++u) {
      float x[4];
      chunk(u, x);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c0 + u * 256 + e;
        append(x[e], c, valid(c) && make_key(x[e], (uint32_t)c) >= kthr);
      }
    }
    total = total < SEL_CAP ? total : SEL_CAP;
  }
  const int cap = total <= 64 ? 64 : total <= 128 ? 128 : total <= 256 ? 256 : SEL_CAP;
  for (int i = total + lane; i < cap; i += 64) buf[i] = 0ull;
  wave_lds_sync();
  if (cap == 64)             // wave-uniform: the smallest sort that holds the keys
    block_sort_desc<64, 1, true>(buf, lane, k);
  else if (cap == 128)
    block_sort_desc<64, 2, true>(buf, lane, k);
  else if (cap == 256)
    block_sort_desc<64, 4, true>(buf, lane, k);
  else
    block_sort_desc<64, 8, true>(buf, lane, k);
  const int f = total < k ? total : k;
  for (int i = lane; i < k; i += 64) {
    const u64 key = buf[i];
    const bool ok = i < f;
    if (D) D[(size_t)r * out_ld + i] = ok ? key_score(key) : -3.402823466e+38f;
    if (I64) I64[(size_t)r * out_ld + i] = ok ? (int64_t)key_id(key) : -1;
    if (I32) I32[(size_t)r * out_ld + i] = ok ? (int32_t)key_id(key) : -1;
  }
}

int row_topk(const float *scores, int64_t ld, int rows, int n, int k, const int32_t *ids,
             int32_t id_base, const int32_t *vlist, const uint32_t *bitmap, int bitmap_words,
             float *D, int64_t *I64, int32_t *I32, int64_t out_ld, const uint64_t *upper_in,
             uint64_t *upper_out) {
  if (rows <= 0) return ASL_OK;
  if (k <= 0 || k > TK_MAX_K) return fail(ASL_ERR_CAPACITY, "top-k: k=%d outside 1..%d", k, TK_MAX_K);
  const int cap = topk_cap_for(k);
  // Short plain rows: wave_select_kernel covers this whole domain (ties and degenerate ranges included,
  // inside the wave), so there is no second selection kernel and no second launch.
  if (n <= SEL_VPT * TK_NT && k <= 256 && !ids && id_base == 0 && !bitmap && !upper_in && !upper_out) {
    const dim3 grid((rows + SEL_WAVES - 1) / SEL_WAVES), block(TK_NT);
    const bool full = n == SEL_VPT * TK_NT && ld % 4 == 0 && (reinterpret_cast<uintptr_t>(scores) & 15) == 0;
    if (full)
      hipLaunchKernelGGL((wave_select_kernel<SEL_VPT, true>), grid, block, 0, stream(), scores, ld, rows,
                         n, k, D, I64, I32, out_ld);
    else if (n <= SEL_VPT / 4 * TK_NT)
      hipLaunchKernelGGL((wave_select_kernel<SEL_VPT / 4, false>), grid, block, 0, stream(), scores, ld,
                         rows, n, k, D, I64, I32, out_ld);
    else
      hipLaunchKernelGGL((wave_select_kernel<SEL_VPT, false>), grid, block, 0, stream(), scores, ld, rows,
                         n, k, D, I64, I32, out_ld);
    ASL_CHECK_LAUNCH();
    return ASL_OK;
  }
  const size_t lds = (size_t)cap * 8 + 16;
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute((const void *)row_topk_kernel,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(row_topk_kernel, dim3(rows), dim3(TK_NT), lds, stream(), scores, ld, n,
                     k, cap, ids, id_base, vlist, bitmap, bitmap_words, D, I64, I32, out_ld,
                     reinterpret_cast<const u64 *>(upper_in), reinterpret_cast<u64 *>(upper_out));
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// ------------------------------------------------------------------ merge
// Ds/Is: [S, nq, k] partial lists -> [nq, k].
__global__ __launch_bounds__(TK_NT) void topk_merge_kernel(
    const float *__restrict__ Ds, const int64_t *__restrict__ Is, int S, int nq, int k,
    int cap, float *__restrict__ D, int64_t *__restrict__ I) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u64 *buf = reinterpret_cast<u64 *>(smem);
  u64 *thr = buf + cap;
  int *ctl = reinterpret_cast<int *>(thr + 1);
  const int tid = threadIdx.x, q = blockIdx.x;
  StreamTopK<TK_NT> tk;
  tk.init(buf, ctl, thr, cap, k, tid);
  const int total = S * k;
  for (int base = 0; base < total; base += TK_NT) {
    const int t = base + tid;
    u64 key = 0ull;
    if (t < total) {
      const int s = t / k, i = t - s * k;
      const size_t o = ((size_t)s * nq + q) * k + i;
      const int64_t id = Is[o];
      if (id >= 0) key = make_key(Ds[o], (uint32_t)id);
    }
    tk.push(key, tid);
  }
  tk.finish(D + (size_t)q * k, I + (size_t)q * k, nullptr, tid);
}

// Histogram-threshold variant (hist_topk.hpp): no sort while streaming, the survivors are
// sorted once. The S lists are visited in interleaved 64-entry chunks, so that (for the
// usual sorted partial lists) the best entries of every list come first and the
// threshold bucket rises after the first rounds; reads stay coalesced (256 B per wave).
// KEYS: Is holds packed (ord(score) << 32 | ~id) keys (0 = empty), Ds is unused.
template <int CAP, int PT, bool KEYS = false>
__global__ __launch_bounds__(HT_NT) void topk_merge_hist_kernel(
    const float *__restrict__ Ds, const int64_t *__restrict__ Is, int S, int nq, int k,
    float *__restrict__ D, int64_t *__restrict__ I, int unordered) {
  using TopK = HistTopK<CAP, HT_NT * PT>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, q = blockIdx.x;
  TopK top;
  top.init(smem, k, nullptr, tid);
  const int kc = (k + 63) >> 6;          // 64-entry chunks per list
  const int total = kc * S * 64;
  for (int base = 0; base < total; base += HT_NT * PT) {
    top.begin_round();
    int appended = 0;
#pragma unroll
    for (int u = 0; u < PT; ++u) {
      const int v = base + u * HT_NT + tid;
      const int c = v >> 6, s = c % S, j = (c / S) * 64 + (v & 63);
      bool valid = v < total && j < k;
      float score = 0.0f;
      int64_t id = -1;
      uint32_t slot = 0;
      if (valid) {
        const size_t o = ((size_t)s * nq + q) * k + j;
        if (KEYS) {
          const u64 key = (u64)Is[o];
          valid = key != 0ull;
          score = key_score(key);
          slot = (uint32_t)key;
        } else {
          score = Ds[o];
          id = Is[o];
          valid = id >= 0;
          slot = 0xFFFFFFFFu - (uint32_t)id;
        }
      }
      const bool take = top.offer(valid, score, slot);
      appended += __popcll(__ballot(take));
    }
    top.end_round(appended);
  }
  if (unordered)   // exact top-k as a set: no sort (scratch = CAP keys behind the structure's LDS)
    top.finish_set(D ? D + (size_t)q * k : nullptr, I + (size_t)q * k, nullptr,
                   reinterpret_cast<u64 *>(smem + TopK::lds_bytes()));
  else
    top.finish(D ? D + (size_t)q * k : nullptr, I + (size_t)q * k, nullptr);
}

// merge of packed-key lists [S, nq, k] (asl_index_set_unordered mode 2)
int topk_merge_keys(const int64_t *Ks, int S, int nq, int k, float *D, int64_t *I, int unordered) {
  if (nq <= 0) return ASL_OK;
  if (k <= 0 || k + 256 + 512 > 2048)
    return fail(ASL_ERR_CAPACITY, "merge_keys: k=%d outside 1..1280", k);
  const size_t lds = HistTopK<2048, HT_NT * 2>::lds_bytes() + (unordered ? (size_t)2048 * 8 : 0);
  hipLaunchKernelGGL((topk_merge_hist_kernel<2048, 2, true>), dim3(nq), dim3(HT_NT), lds, stream(),
                     (const float *)nullptr, Ks, S, nq, k, D, I, unordered);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

int topk_merge(const float *Ds, const int64_t *Is, int S, int nq, int k, float *D, int64_t *I) {
  if (nq <= 0) return ASL_OK;
  if (k <= 0 || k > TK_MAX_K) return fail(ASL_ERR_CAPACITY, "merge: k=%d outside 1..%d", k, TK_MAX_K);
  if ((int64_t)S * k >= 2048 && k + 256 + 1024 <= 4096) {
    // CAP 2048 keeps the final sort at 8 keys per thread (~100 VGPRs, 4+ workgroups per CU);
    // CAP 4096 needs 16 (240 VGPRs, one workgroup per CU)
    if (k + 256 + 512 <= 2048)
      hipLaunchKernelGGL((topk_merge_hist_kernel<2048, 2>), dim3(nq), dim3(HT_NT),
                         (HistTopK<2048, HT_NT * 2>::lds_bytes()), stream(), Ds, Is, S, nq, k, D, I, 0);
    else
      hipLaunchKernelGGL((topk_merge_hist_kernel<4096, 4>), dim3(nq), dim3(HT_NT),
                         (HistTopK<4096, HT_NT * 4>::lds_bytes()), stream(), Ds, Is, S, nq, k, D, I, 0);
    ASL_CHECK_LAUNCH();
    return ASL_OK;
  }
  const int cap = topk_cap_for(k);
  const size_t lds = (size_t)cap * 8 + 16;
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute((const void *)topk_merge_kernel,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(topk_merge_kernel, dim3(nq), dim3(TK_NT), lds, stream(), Ds, Is, S, nq, k,
                     cap, D, I);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// ------------------------------------------------------------------ bitmap of probed lists
__global__ void probe_bitmap_kernel(const int32_t *__restrict__ coarse_I, int nq, int nprobe,
                                    uint32_t *__restrict__ bitmap, int words) {
  const int q = blockIdx.x;
  for (int p = threadIdx.x; p < nprobe; p += blockDim.x) {
    const int l = coarse_I[(size_t)q * nprobe + p];
    if (l >= 0) atomicOr(&bitmap[(size_t)q * words + (l >> 5)], 1u << (l & 31));
  }
}

int probe_bitmap(const int32_t *coarse_I, int nq, int nprobe, uint32_t *bitmap, int words) {
  HIP_TRY(hipMemsetAsync(bitmap, 0, (size_t)nq * words * sizeof(uint32_t), stream()));
  hipLaunchKernelGGL(probe_bitmap_kernel, dim3(nq), dim3(128), 0, stream(), coarse_I, nq,
                     nprobe, bitmap, words);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// ------------------------------------------------------------------ gathers
__global__ void gather_rows_f32_kernel(const float *__restrict__ src, int64_t ld_src,
                                       const int64_t *__restrict__ rows, int64_t n, int d,
                                       float *__restrict__ dst, int64_t ld_dst) {
  const int64_t i = block_linear();
  if (i >= n) return;
  const int64_t r = rows ? rows[i] : i;
  for (int j = threadIdx.x; j < d; j += blockDim.x)
    dst[i * ld_dst + j] = src[r * ld_src + j];
}
int gather_rows_f32(const float *src, int64_t ld_src, const int64_t *rows, int64_t n, int d,
                    float *dst, int64_t ld_dst) {
  if (n <= 0) return ASL_OK;
  hipLaunchKernelGGL(gather_rows_f32_kernel, grid_2d(n), dim3(256), 0, stream(), src,
                     ld_src, rows, n, d, dst, ld_dst);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

__global__ void gather_rows_u8_kernel(const uint8_t *__restrict__ src,
                                      const int32_t *__restrict__ rows, int64_t n, int m,
                                      uint8_t *__restrict__ dst) {
  const int64_t t = block_linear() * blockDim.x + threadIdx.x;
  if (t >= n * m) return;
  const int64_t i = t / m;
  const int j = (int)(t - i * m);
  dst[t] = src[(int64_t)rows[i] * m + j];
}
int gather_rows_u8(const uint8_t *src, const int32_t *rows, int64_t n, int m, uint8_t *dst) {
  if (n <= 0) return ASL_OK;
  hipLaunchKernelGGL(gather_rows_u8_kernel, grid_2d(cdiv(n * m, 256)), dim3(256), 0,
                     stream(), src, rows, n, m, dst);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// ------------------------------------------------------------------ PQ LUT + scan
// LUT[m][c] = ascending-t fmaf chain of q[m*dsub+t] * cb[m][c][t]; thread c owns code c.
__device__ __forceinline__ void build_lut_lds(const float *__restrict__ xq_row, int d,
                                              const float *__restrict__ codebooks, int m,
                                              int ksub, int dsub, float *s_q, float *s_lut,
                                              int tid) {
  for (int i = tid; i < d; i += TK_NT) s_q[i] = xq_row[i];
  __syncthreads();
  for (int c = tid; c < ksub; c += TK_NT) {
    for (int mi = 0; mi < m; ++mi) {
      const float *cb = codebooks + ((size_t)mi * ksub + c) * dsub;
      const float *qs = s_q + mi * dsub;
      float acc = 0.0f;
      for (int t = 0; t < dsub; ++t) acc = __builtin_fmaf(qs[t], cb[t], acc);
      s_lut[mi * ksub + c] = acc;
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(TK_NT) void pq_lut_kernel(const float *__restrict__ xq, int d,
                                                       const float *__restrict__ codebooks,
                                                       int m, int ksub, int dsub,
                                                       float *__restrict__ lut_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *s_lut = reinterpret_cast<float *>(smem);
  float *s_q = s_lut + m * ksub;
  const int q = blockIdx.x;
  build_lut_lds(xq + (size_t)q * d, d, codebooks, m, ksub, dsub, s_q, s_lut, threadIdx.x);
  for (int i = threadIdx.x; i < m * ksub; i += TK_NT) lut_out[(size_t)q * m * ksub + i] = s_lut[i];
}
int pq_lut(const float *xq, int nq, int d, const float *codebooks, int m, int ksub, int dsub,
           float *lut_out) {
  if (nq <= 0) return ASL_OK;
  const size_t lds = ((size_t)m * ksub + d) * 4;
  if (lds > (size_t)PQ_MAX_LDS_BYTES) return fail(ASL_ERR_CAPACITY, "pq lut: d=%d / m=%d do not fit LDS", d, m);
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute((const void *)pq_lut_kernel,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(pq_lut_kernel, dim3(nq), dim3(TK_NT), lds, stream(), xq, d, codebooks, m,
                     ksub, dsub, lut_out);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// Canonical ADC sum: p_j = sum_t v[j+16t]; 16->1 mirror tree
// (j,15-j)(j,7-j)(j,3-j)(0,1); + coarse.
template <int M>
__device__ __forceinline__ float adc_score(const float *__restrict__ s_lut, int ksub,
                                           const uint32_t *__restrict__ cw, float coarse) {
  float v[M];
#pragma unroll
  for (int w = 0; w < M / 4; ++w) {
    const uint32_t word = cw[w];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int mi = w * 4 + b;
      v[mi] = s_lut[mi * ksub + ((word >> (8 * b)) & 0xffu)];
    }
  }
  float p[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (j < M) {
      float a = v[j];
#pragma unroll
      for (int t = j + 16; t < M; t += 16) a = a + v[t];
      p[j] = a;
    } else {
      p[j] = 0.0f;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) p[j] = p[j] + p[15 - j];
#pragma unroll
  for (int j = 0; j < 4; ++j) p[j] = p[j] + p[7 - j];
#pragma unroll
  for (int j = 0; j < 2; ++j) p[j] = p[j] + p[3 - j];
  return coarse + (p[0] + p[1]);
}

// One workgroup per query: LUT in LDS, stream the probed lists, fused top-k.
template <int M>
__global__ __launch_bounds__(TK_NT) void pq_scan_kernel(
    const float *__restrict__ xq, int d, const float *__restrict__ codebooks, int ksub,
    int dsub, const float *__restrict__ coarse_D, const int32_t *__restrict__ coarse_I,
    int nprobe, const int32_t *__restrict__ list_offsets, const int32_t *__restrict__ ids,
    const uint8_t *__restrict__ codes, int k, int cap, float *__restrict__ D,
    int64_t *__restrict__ I64, int32_t *__restrict__ I32, int64_t out_ld,
    const u64 *__restrict__ upper_in, u64 *__restrict__ upper_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u64 *buf = reinterpret_cast<u64 *>(smem);
  u64 *thr = buf + cap;
  int *ctl = reinterpret_cast<int *>(thr + 1);       // 2 ints
  float *s_lut = reinterpret_cast<float *>(thr + 2);
  float *s_q = s_lut + M * ksub;
  const int tid = threadIdx.x, q = blockIdx.x;
  build_lut_lds(xq + (size_t)q * d, d, codebooks, M, ksub, dsub, s_q, s_lut, tid);
  StreamTopK<TK_NT> tk;
  tk.init(buf, ctl, thr, cap, k, tid);
  const u64 ub = upper_in ? upper_in[q] : ~0ull;      // bounded pass, see row_topk_kernel
  for (int p = 0; p < nprobe; ++p) {
    const int l = coarse_I[(size_t)q * nprobe + p];
    if (l < 0) continue;  // uniform
    const float coarse = coarse_D[(size_t)q * nprobe + p];
    const int start = list_offsets[l], len = list_offsets[l + 1] - start;
    for (int base = 0; base < len; base += TK_NT) {
      const int i = base + tid;
      u64 key = 0ull;
      if (i < len) {
        const uint32_t *cw = reinterpret_cast<const uint32_t *>(codes + (size_t)(start + i) * M);
        key = make_key(adc_score<M>(s_lut, ksub, cw, coarse), (uint32_t)ids[start + i]);
        if (key >= ub) key = 0ull;
      }
      tk.push(key, tid);
    }
  }
  tk.finish(D ? D + (size_t)q * out_ld : nullptr, I64 ? I64 + (size_t)q * out_ld : nullptr,
            I32 ? I32 + (size_t)q * out_ld : nullptr, tid);
  if (upper_out && tid == 0) upper_out[q] = ctl[0] >= k ? buf[k - 1] : 0ull;
}

size_t pq_scan_lds_bytes(int m, int ksub, int d, int k) {
  return (size_t)topk_cap_for(k) * 8 + 16 + ((size_t)m * ksub + d) * 4;
}

int pq_scan(const float *xq, int nq, int d, const float *codebooks, int m, int ksub, int dsub,
            const float *coarse_D, const int32_t *coarse_I, int nprobe,
            const int32_t *list_offsets, const int32_t *ids, const uint8_t *codes, int k,
            float *D, int64_t *I64, int32_t *I32, int64_t out_ld, const uint64_t *upper_in,
            uint64_t *upper_out) {
  if (nq <= 0) return ASL_OK;
  if (k <= 0 || k > TK_MAX_K) return fail(ASL_ERR_CAPACITY, "pq scan: k=%d outside 1..%d", k, TK_MAX_K);
  const auto launch = [&](auto m_const) -> int {      // the kernel's M arrives as a std::integral_constant
    constexpr int M = decltype(m_const)::value;
    const int cap = topk_cap_for(k);
    const size_t lds = pq_scan_lds_bytes(M, ksub, d, k);
    if (lds > (size_t)PQ_MAX_LDS_BYTES) return fail(ASL_ERR_CAPACITY, "pq scan: k=%d / m=%d do not fit LDS", k, M);
    if (lds > 64 * 1024)
      HIP_TRY(hipFuncSetAttribute((const void *)pq_scan_kernel<M>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(pq_scan_kernel<M>, dim3(nq), dim3(TK_NT), lds, stream(), xq, d, codebooks,
                       ksub, dsub, coarse_D, coarse_I, nprobe, list_offsets, ids, codes, k, cap,
                       D, I64, I32, out_ld > 0 ? out_ld : (int64_t)k, reinterpret_cast<const u64 *>(upper_in),
                       reinterpret_cast<u64 *>(upper_out));
    ASL_CHECK_LAUNCH();
    return ASL_OK;
  };
  switch (m) {
    case 4: return launch(std::integral_constant<int, 4>{});
    case 8: return launch(std::integral_constant<int, 8>{});
    case 16: return launch(std::integral_constant<int, 16>{});
    case 32: return launch(std::integral_constant<int, 32>{});
    case 64: return launch(std::integral_constant<int, 64>{});
    default: return fail(ASL_ERR_INVALID, "pq scan: pq_m must be one of 4,8,16,32,64 (got %d)", m);
  }
}


// sum over queries of probed list lengths (algorithmic work of a scan launch)
__global__ void scanned_count_kernel(const int32_t *__restrict__ coarse_I, int64_t n,
                                     const int32_t *__restrict__ list_offsets,
                                     unsigned long long *__restrict__ out) {
  unsigned long long acc = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int l = coarse_I[i];
    if (l >= 0) acc += (unsigned long long)(list_offsets[l + 1] - list_offsets[l]);
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out, acc);
}
int scanned_count(const int32_t *coarse_I, int64_t n, const int32_t *list_offsets,
                  unsigned long long *out_dev) {
  // accumulates into out_dev (the caller owns its zeroing)
  hipLaunchKernelGGL(scanned_count_kernel, dim3(256), dim3(256), 0, stream(), coarse_I, n,
                     list_offsets, out_dev);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

}  // namespace asl
