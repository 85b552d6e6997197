// flat_tools.hip -- what prepares or measures a postings scan (flat_scan.hip): the runs of the window-exact
// index, the selector words, and the scan's algorithmic work for the benchmark's roofline.
#include "flat_postings.hpp"

namespace asl {

// ---- the run [lo, hi) of every query in the one precursor-ordered list of the window-exact index (RANGED in
// flat_scan.hip): window_run (common.hpp), the two binary searches window_ranges_kernel makes per (query, probe),
// once per query over the whole key column (ascending, NaN last). q_pmz == nullptr: the window that passes
// everything, NaN keys included: [0, n). acc (optional): += sum of hi - lo.
__global__ void winflat_runs_kernel(const double *__restrict__ q_pmz, int nq, const float *__restrict__ key, int n,
                                    int charge, double tol, int mode, int2 *__restrict__ runs,
                                    unsigned long long *__restrict__ acc) {
  const int64_t i = block_linear() * blockDim.x + threadIdx.x;
  unsigned long long cnt = 0;
  if (i < nq) {
    int2 r = make_int2(0, n);
    if (q_pmz) r = window_run(key, n, query_window(q_pmz, i, mode), charge, tol, mode);
    runs[i] = r;
    cnt = (unsigned long long)(r.y - r.x);
  }
  if (acc) {
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(acc, cnt);
  }
}

int winflat_runs(const double *q_pmz, int nq, const float *key, int64_t n, int charge, double tol, int mode,
                 int2 *runs, unsigned long long *acc) {
  if (nq <= 0) return ASL_OK;
  hipLaunchKernelGGL(winflat_runs_kernel, grid_2d(cdiv(nq, 256)), dim3(256), 0, stream(), q_pmz, nq, key, (int)n,
                     charge, tol, mode, runs, acc);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// ---- selector words of the postings layout (SEL in flat_scan.hip): FI_ROWS words per block, one wave per word.
// The block's list comes from a binary search of blk_offsets; a position behind the list's end is unselected.
__global__ __launch_bounds__(256) void flat_selector_kernel(
    const int32_t *__restrict__ list_offsets, const int32_t *__restrict__ blk_offsets, int nlist,
    const int32_t *__restrict__ ids, const uint8_t *__restrict__ keep, int64_t n, int64_t nwords,
    unsigned long long *__restrict__ words) {
  const int64_t w = block_linear() * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= nwords) return;             // (wave-uniform)
  const int blk = (int)(w / FI_ROWS), r = (int)(w % FI_ROWS);
  int a = 0, b = nlist;                // the last list with blk_offsets[l] <= blk
  while (b - a > 1) {
    const int mid = (a + b) >> 1;
    if (blk_offsets[mid] <= blk) a = mid; else b = mid;
  }
  const int64_t pos = (int64_t)list_offsets[a] + (int64_t)(blk - blk_offsets[a]) * FI_BLK + r * 64 + lane;
  bool on = false;
  if (blk < blk_offsets[a + 1] && pos < list_offsets[a + 1]) {
    const int32_t id = ids[pos];
    on = id >= 0 && id < n && keep[id] != 0;
  }
  const unsigned long long m = __ballot(on);
  if (lane == 0) words[w] = m;
}

int flat_selector(const FlatPostings &P, const uint8_t *keep, int64_t n, unsigned long long *words) {
  const int64_t nwords = P.n_blocks * FI_ROWS;
  if (nwords <= 0 || P.nlist <= 0) return ASL_OK;
  hipLaunchKernelGGL(flat_selector_kernel, grid_2d(cdiv(nwords, 4)), dim3(256), 0, stream(), P.list_offsets,
                     P.blk_offsets, P.nlist, P.ids, keep, n, nwords, words);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}
int flat_selector_words_per_block() { return FI_ROWS; }

// ---- algorithmic work of a postings scan (bench.py: the roofline of this kernel), per (query, probed block,
// non-zero query dimension). One workgroup per query, outside any timed region. Float postings: the 4-byte table
// word and the dimension's postings (6 bytes each), out[0] += 4 + 6 c; out[1] counts what that costs in 128-byte
// lines: the lines every non-empty segment spans plus the distinct lines of the block's table row that hold a
// wanted word. FX: the table byte + 4 bytes per posting (cnt16: the real number of postings of every cell, kept
// for this accounting only); lines: the block's table row (read whole) + the lines of the wanted segments.
template <bool FX>
__global__ __launch_bounds__(256) void flat_postings_work_kernel(const FlatPostings P, const float *__restrict__ xq,
                                                                 const int32_t *__restrict__ coarse_I, int nprobe,
                                                                 unsigned long long *__restrict__ out) {
  extern __shared__ int s_work[];          // [d] non-zero dimensions, then 1 counter
  const int d = P.d;
  int *s_dim = s_work, *s_n = s_work + d;
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (tid == 0) *s_n = 0;
  __syncthreads();
  for (int j = tid; j < d; j += 256)
    if (xq[(size_t)q * d + j] != 0.0f) s_dim[atomicAdd(s_n, 1)] = j;
  __syncthreads();
  const int K = *s_n;
  unsigned long long bytes = 0, lines = 0;
  for (int p = 0; p < nprobe; ++p) {
    const int l = coarse_I[(size_t)q * nprobe + p];
    if (l < 0) continue;
    for (int b = P.blk_offsets[l]; b < P.blk_offsets[l + 1]; ++b) {
      if constexpr (FX) {
        for (int t = tid; t < K; t += 256) {
          bytes += 1ull + 4ull * P.cnt16[(size_t)b * d + s_dim[t]];
          lines += P.tab8[(size_t)b * P.tab_stride + s_dim[t]];
        }
        if (tid == 0) lines += (unsigned long long)((d + 127) / 128);
      } else {
        const uint32_t *row = P.tab32 + (size_t)b * d;
        for (int t = tid; t < K; t += 256) {
          const uint32_t w = row[s_dim[t]];
          const uint32_t c = inv_word_count(w), st = inv_word_start(w) * 64u;
          bytes += 4ull + 6ull * c;
          if (c) lines += ((st + 6u * c - 1u) >> 7) - (st >> 7) + 1u;
        }
        // distinct table lines: one wave walks the query's dimensions in line order
        if (tid < 64) {
          for (int ln0 = 0; ln0 * 32 < d; ln0 += 64) {      // 32 words per 128-byte line
            const int ln = ln0 + lane;
            bool hit = false;
            for (int t = 0; t < K; ++t) hit |= (s_dim[t] >> 5) == ln;
            lines += __popcll(__ballot(hit)) * (lane == 0);
          }
        }
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    bytes += __shfl_xor(bytes, off);
    lines += __shfl_xor(lines, off);
  }
  if (lane == 0) {
    atomicAdd(&out[0], bytes);
    atomicAdd(&out[1], lines);
  }
}

int flat_postings_work(const FlatPostings &P, const float *xq, int nq, const int32_t *coarse_I, int nprobe,
                       unsigned long long *out_dev) {
  if (nq <= 0) return ASL_OK;
  const auto kernel = P.layout == 2 ? flat_postings_work_kernel<true> : flat_postings_work_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(nq), dim3(256), (size_t)(P.d + 1) * 4, stream(), P, xq, coarse_I, nprobe, out_dev);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

}  // namespace asl
