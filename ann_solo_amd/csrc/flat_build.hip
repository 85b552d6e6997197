// flat_build.hip -- what builds the IVF-Flat postings (flat_postings.hpp) from dense rows: the non-zero
// counter that decides whether the postings pay, the fixed-point quantiser of add(), and per layout the
// host placement of a block's segments, the fill and the canonical order inside every segment.
#include "flat_postings.hpp"

namespace asl {

// non-zeros per vector (one wave per vector) and their maximum: decides at build time whether the postings layout
// pays. nnz_max[1] is raised when a non-zero component is NOT a fixed-point value (0 < x < 1 on the grid of
// 2^-22): such an index keeps float postings
__global__ void count_nnz_kernel(const float *__restrict__ vecs, int d, int64_t n, int32_t *__restrict__ nnz,
                                 int32_t *__restrict__ nnz_max) {
  const int64_t v = block_linear() * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (v >= n) return;
  int c = 0;
  bool off_grid = false;
  for (int j = lane; j < d; j += 64) {
    const float x = vecs[v * d + j];
    c += x != 0.0f;
    off_grid |= x != 0.0f && !fx22_on_grid(x);
  }
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if (__ballot(off_grid) && lane == 0) atomicMax(nnz_max + 1, 1);
  if (lane == 0) {
    nnz[v] = c;
    atomicMax(nnz_max, c);
  }
}

int count_nnz(const float *vecs, int d, int64_t n, int32_t *nnz, int32_t *nnz_max_dev) {
  HIP_TRY(hipMemsetAsync(nnz_max_dev, 0, 2 * sizeof(int32_t), stream()));
  if (n <= 0) return ASL_OK;
  hipLaunchKernelGGL(count_nnz_kernel, grid_2d(cdiv(n, 4)), dim3(256), 0, stream(), vecs, d, n, nnz, nnz_max_dev);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// add() of an IVF-Flat index in fixed-point storage mode: components in [0, 1) go to the nearest
// multiple of 2^-22 (ties to even; the largest is 1 - 2^-22); anything else is stored as given
// (and keeps the whole index on float postings). The oracle's orc_quantize_fx22 is the same rule.
__global__ void quantize_fx22_kernel(float *__restrict__ x, int64_t n) {
  const int64_t i = block_linear() * blockDim.x + threadIdx.x;
  if (i < n) x[i] = fx22_round(x[i]);
}

int quantize_fx22(float *x, int64_t n) {
  if (n <= 0) return ASL_OK;
  hipLaunchKernelGGL(quantize_fx22_kernel, grid_2d(cdiv(n, 256)), dim3(256), 0, stream(), x, n);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// ---- the float layout. Placement of a block's segments (counts cnt[0..d) -> table words tab[0..d)), by line as
// flat_scan.hip says; returns the block's size in 64-byte units, or 0 with *ok = false when a start or a count
// does not fit its 16 bits.
uint32_t inv_place_block(const uint32_t *cnt, int d, uint32_t *tab, bool *ok) {
  uint32_t pos = 0;     // 64-byte units; even = on a 128-byte line
  for (int j = 0; j < d; j++) {
    const uint32_t c = cnt[j];
    if (c == 0) {
      tab[j] = 0u;
      continue;
    }
    const uint32_t units = (6u * c + 63u) / 64u;
    if (units >= 2u && (pos & 1u)) ++pos;     // a full line or more: start on a line
    if (pos > INV_START_MAX || c > INV_COUNT_MAX) {
      *ok = false;
      return 0;
    }
    tab[j] = inv_word(pos, c);
    pos += units;
  }
  return pos;
}

// pos_blk / pos_loc: block and local index of the list-ordered position i (add-order row order[i]).
__global__ void inv_count_kernel(const float *__restrict__ vecs, int d, const int32_t *__restrict__ order,
                                 const int32_t *__restrict__ pos_blk, int64_t n, uint32_t *__restrict__ cnt) {
  const int64_t i = block_linear() * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= n) return;
  const float *row = vecs + (size_t)order[i] * d;
  uint32_t *c = cnt + (size_t)pos_blk[i] * d;
  for (int j = lane; j < d; j += 64)
    if (row[j] != 0.0f) atomicAdd(&c[j], 1u);
}

__global__ void inv_fill_kernel(const float *__restrict__ vecs, int d, const int32_t *__restrict__ order,
                                const int32_t *__restrict__ pos_blk, const uint16_t *__restrict__ pos_loc, int64_t n,
                                const uint32_t *__restrict__ blk_base, const uint32_t *__restrict__ seg_tab,
                                uint32_t *__restrict__ cursor, char *__restrict__ seg_bytes) {
  const int64_t i = block_linear() * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= n) return;
  const float *row = vecs + (size_t)order[i] * d;
  const size_t b = (size_t)pos_blk[i] * d;
  char *bptr = seg_bytes + (size_t)blk_base[pos_blk[i]] * 64;
  const uint16_t loc = pos_loc[i];
  for (int j = lane; j < d; j += 64) {
    const float x = row[j];
    if (x != 0.0f) {
      const uint32_t w = seg_tab[b + j];
      const size_t st = (size_t)inv_word_start(w) * 64;
      const uint32_t c = inv_word_count(w);
      const uint32_t p = atomicAdd(&cursor[b + j], 1u);     // any order inside a segment
      *reinterpret_cast<float *>(bptr + st + 4 * (size_t)p) = x;
      *reinterpret_cast<uint16_t *>(bptr + st + 4 * (size_t)c + 2 * (size_t)p) = loc;
    }
  }
}

// ---- canonical order inside every segment. inv_fill_kernel leaves the postings of a segment in the order its
// atomics happened to run; a vector occurs at most once per dimension, so ANY order gives the same accumulators.
// This pass (one wave per segment) makes the layout deterministic -- postings sorted by local index -- and, for
// segments longer than a row, deals each row of 64 to its first and second half (the LDS services lanes {0-31}
// and {32-63} of a ds instruction separately) so that the banks (local index mod 32) inside a half are distinct
// where the row allows it. Measured (profiles/r03_flat_scan_notes.txt): bank conflicts are NOT what the scan
// waits for -- a layout without any conflict runs at the same speed -- the sorted order is worth 1 %; it is kept
// for the reproducible file image.
constexpr int IO_WAVES = 4;
__global__ __launch_bounds__(64 * IO_WAVES) void inv_order_kernel(
    int64_t nseg, int d, const uint32_t *__restrict__ blk_base, const uint32_t *__restrict__ seg_tab,
    char *__restrict__ seg_bytes) {
  __shared__ float s_val[IO_WAVES][2][FI_BLK];
  __shared__ uint16_t s_loc[IO_WAVES][2][FI_BLK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t seg = (int64_t)blockIdx.x * IO_WAVES + wave;
  if (seg >= nseg) return;
  const uint32_t w = seg_tab[seg];
  const int c = (int)inv_word_count(w);
  if (c <= 1 || c > FI_BLK) return;
  char *ptr = seg_bytes + (size_t)blk_base[seg / d] * 64 + (size_t)inv_word_start(w) * 64;
  float *gv = reinterpret_cast<float *>(ptr);
  uint16_t *gl = reinterpret_cast<uint16_t *>(ptr + 4 * (size_t)c);
  float *v0 = s_val[wave][0], *v1 = s_val[wave][1];
  uint16_t *l0 = s_loc[wave][0], *l1 = s_loc[wave][1];
  for (int i = lane; i < c; i += 64) {
    v0[i] = gv[i];
    l0[i] = gl[i];
  }
  __builtin_amdgcn_wave_barrier();
  // rank sort by local index (unique inside a segment)
  for (int i = lane; i < c; i += 64) {
    const uint16_t me = l0[i];
    int r = 0;
    for (int t = 0; t < c; ++t) r += l0[t] < me;
    v1[r] = v0[i];
    l1[r] = me;
  }
  __builtin_amdgcn_wave_barrier();
  // greedy deal, serial per row (c is ~30; a shared fragment bin has a few hundred)
  if (lane == 0) {
    for (int r0 = 0; r0 < c; r0 += 64) {
      const int n = min(64, c - r0);
      const int cap0 = min(n, 32), cap1 = n - cap0;      // lanes 0-31 | lanes 32-63 of the row
      uint32_t used0 = 0, used1 = 0;
      int n0 = 0, n1 = 0;
      for (int t = 0; t < n; ++t) {
        const uint32_t bit = 1u << (l1[r0 + t] & 31);
        int g;
        if (!(used0 & bit) && n0 < cap0) g = 0;
        else if (!(used1 & bit) && n1 < cap1) g = 1;
        else g = (n0 < cap0 && (n1 >= cap1 || n0 - cap0 <= n1 - cap1)) ? 0 : 1;
        int dst;
        if (g == 0) {
          used0 |= bit;
          dst = r0 + n0++;
        } else {
          used1 |= bit;
          dst = r0 + cap0 + n1++;
        }
        v0[dst] = v1[r0 + t];
        l0[dst] = l1[r0 + t];
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  for (int i = lane; i < c; i += 64) {
    gv[i] = v0[i];
    gl[i] = l0[i];
  }
}

int inv_count(const float *vecs, int d, const int32_t *order, const int32_t *pos_blk, int64_t n, uint32_t *cnt) {
  if (n <= 0) return ASL_OK;
  hipLaunchKernelGGL(inv_count_kernel, grid_2d(cdiv(n, 4)), dim3(256), 0, stream(), vecs, d, order, pos_blk, n, cnt);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// the postings of n vectors into the placed segments of nblocks blocks (cursor: zeroed, [nblocks * d]), then ordered
int inv_fill(const float *vecs, int d, const int32_t *order, const int32_t *pos_blk, const uint16_t *pos_loc,
             int64_t n, int64_t nblocks, const uint32_t *blk_base, const uint32_t *seg_tab, uint32_t *cursor,
             char *seg_bytes) {
  const int64_t nseg = nblocks * d;
  if (n <= 0 || nseg <= 0) return ASL_OK;
  hipLaunchKernelGGL(inv_fill_kernel, grid_2d(cdiv(n, 4)), dim3(256), 0, stream(), vecs, d, order, pos_blk, pos_loc, n,
                     blk_base, seg_tab, cursor, seg_bytes);
  ASL_CHECK_LAUNCH();
  hipLaunchKernelGGL(inv_order_kernel, dim3((unsigned)cdiv(nseg, IO_WAVES)), dim3(64 * IO_WAVES), 0, stream(), nseg, d,
                     blk_base, seg_tab, seg_bytes);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// ---- the fixed-point layout (flat_inv_scan_kernel<.., true>). Placement of a block's segments, whole lines of 32
// posting words: counts cnt[0..d) -> table bytes tab8 (a count is <= FI_BLK: at most 26 lines), the counts in 16
// bits (the work counter's) and every segment's first line from the start of the data (the block's: line0).
// Returns the block's lines.
uint32_t fx_place_block(const uint32_t *cnt, int d, uint32_t line0, uint8_t *tab8, uint16_t *cnt16,
                        uint32_t *seg_line) {
  uint32_t pos = 0;
  for (int j = 0; j < d; j++) {
    seg_line[j] = line0 + pos;
    cnt16[j] = (uint16_t)cnt[j];
    tab8[j] = (uint8_t)fx_seg_lines(cnt[j]);
    pos += fx_seg_lines(cnt[j]);
  }
  return pos;
}

// posting words into their segments, in the order the atomics run (fx_order_kernel sorts them).
// seg_line[cell]: first line of the cell's segment, counted from the start of the data.
__global__ void fx_fill_kernel(const float *__restrict__ vecs, int d, const int32_t *__restrict__ order,
                               const int32_t *__restrict__ pos_blk, const uint16_t *__restrict__ pos_loc, int64_t n,
                               const uint32_t *__restrict__ seg_line, uint32_t *__restrict__ cursor,
                               uint32_t *__restrict__ words) {
  const int64_t i = block_linear() * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= n) return;
  const float *row = vecs + (size_t)order[i] * d;
  const size_t b = (size_t)pos_blk[i] * d;
  const uint32_t loc = pos_loc[i];
  for (int j = lane; j < d; j += 64) {
    const float x = row[j];
    if (x != 0.0f) {
      const uint32_t p = atomicAdd(&cursor[b + j], 1u);
      words[(size_t)seg_line[b + j] * 32 + p] = fx_word(x, loc);
    }
  }
}

// canonical image of every segment: postings ascending in the local index (unique inside a
// segment), the rest of the last line filled with repeats of the last posting. One wave per cell.
__global__ __launch_bounds__(64 * IO_WAVES) void fx_order_kernel(
    int64_t ncell, const uint32_t *__restrict__ seg_line, const uint32_t *__restrict__ count,
    uint32_t *__restrict__ words) {
  __shared__ uint32_t s_w[IO_WAVES][2][FI_BLK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t cell = (int64_t)blockIdx.x * IO_WAVES + wave;
  if (cell >= ncell) return;
  const int c = (int)count[cell];
  if (c <= 0 || c > FI_BLK) return;
  uint32_t *g = words + (size_t)seg_line[cell] * 32;
  uint32_t *a = s_w[wave][0], *b = s_w[wave][1];
  for (int i = lane; i < c; i += 64) a[i] = g[i];
  __builtin_amdgcn_wave_barrier();
  for (int i = lane; i < c; i += 64) {
    const uint32_t me = fx_word_loc(a[i]);
    int r = 0;
    for (int t = 0; t < c; ++t) r += fx_word_loc(a[t]) < me;
    b[r] = a[i];
  }
  __builtin_amdgcn_wave_barrier();
  const int padded = (int)fx_seg_lines((uint32_t)c) * 32;
  for (int i = lane; i < padded; i += 64) g[i] = b[min(i, c - 1)];
}

// the posting words of n vectors into the placed segments of ncell cells (cursor: zeroed, [ncell]), then ordered
int fx_fill(const float *vecs, int d, const int32_t *order, const int32_t *pos_blk, const uint16_t *pos_loc,
            int64_t n, int64_t ncell, const uint32_t *seg_line, uint32_t *cursor, uint32_t *words) {
  if (n <= 0 || ncell <= 0) return ASL_OK;
  hipLaunchKernelGGL(fx_fill_kernel, grid_2d(cdiv(n, 4)), dim3(256), 0, stream(), vecs, d, order, pos_blk, pos_loc, n,
                     seg_line, cursor, words);
  ASL_CHECK_LAUNCH();
  hipLaunchKernelGGL(fx_order_kernel, dim3((unsigned)cdiv(ncell, IO_WAVES)), dim3(64 * IO_WAVES), 0, stream(), ncell,
                     seg_line, cursor, words);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

}  // namespace asl
