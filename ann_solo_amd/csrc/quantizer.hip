// quantizer.hip -- device kernels of what BUILDS an index: k-means of the coarse and product quantisers and the
// encoding of added vectors (index_train.hip, asl_index_add). What searches one is in ivf_kernels.hip and the scans.
//
//   row_argmax_kernel       list assignment: arg-max of a row of centroid inner products
//   centroid_update_kernel  k-means update, the oracle's summation order
//   renorm_rows_kernel      spherical k-means: rows rescaled to unit length
//   l2_assign_kernel        PQ training: nearest code of a sub-vector
//   residual_kernel         x - centroid[assign]
//   pq_encode_kernel        PQ codes of the residuals, or of the vectors themselves
#include "common.hpp"
#include "ivf_kernels.hpp"

namespace asl {

// ------------------------------------------------------------------ row arg-max (ties: lowest col)
__global__ __launch_bounds__(256) void row_argmax_kernel(const float *__restrict__ scores,
                                                         int64_t ld, int n,
                                                         int32_t *__restrict__ out) {
  __shared__ float s_v[4];
  __shared__ int s_i[4];
  const int r = blockIdx.x, tid = threadIdx.x;
  const float *row = scores + (size_t)r * ld;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = tid; c < n; c += 256) {
    const float v = row[c];
    if (v > bv || (v == bv && c < bi)) {
      bv = v;
      bi = c;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off);
    const int oi = __shfl_xor(bi, off);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if ((tid & 63) == 0) {
    s_v[tid >> 6] = bv;
    s_i[tid >> 6] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w)
      if (s_v[w] > bv || (s_v[w] == bv && s_i[w] < bi)) {
        bv = s_v[w];
        bi = s_i[w];
      }
    out[r] = bi == 0x7fffffff ? 0 : bi;
  }
}

int row_argmax(const float *scores, int64_t ld, int rows, int n, int32_t *out) {
  if (rows <= 0) return ASL_OK;
  hipLaunchKernelGGL(row_argmax_kernel, dim3(rows), dim3(256), 0, stream(), scores, ld, n, out);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// ------------------------------------------------------------------ k-means update
// One workgroup per cluster: members (ascending point order) are summed in fp32 in
// that order, then divided by the count -- the oracle's loop, bit for bit.
__global__ __launch_bounds__(256) void centroid_update_kernel(
    const float *__restrict__ x, int64_t ld, int d, const int32_t *__restrict__ order,
    const int32_t *__restrict__ offsets, float *__restrict__ centroids) {
  const int c = blockIdx.x;
  const int b = offsets[c], e = offsets[c + 1];
  if (e == b) return;  // empty: left for the host-side split
  const float cnt = (float)(e - b);
  for (int j = threadIdx.x; j < d; j += 256) {
    float s = 0.0f;
    for (int t = b; t < e; ++t) s += x[(size_t)order[t] * ld + j];
    centroids[(size_t)c * d + j] = s / cnt;
  }
}
int centroid_update(const float *x, int64_t ld, int d, int k, const int32_t *order,
                    const int32_t *offsets, float *centroids) {
  hipLaunchKernelGGL(centroid_update_kernel, dim3(k), dim3(256), 0, stream(), x, ld, d, order,
                     offsets, centroids);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// Spherical k-means (FAISS cp.spherical for inner-product indexes): rows with a non-zero
// norm are rescaled to unit L2 length. Canonical chain: ascending fmaf from +0, sqrtf, IEEE
// divide (the encoder's norm) -- one lane walks the chain, the block divides.
__global__ __launch_bounds__(256) void renorm_rows_kernel(float *__restrict__ c, int d) {
  __shared__ float s_nrm;
  float *row = c + (size_t)blockIdx.x * d;
  if (threadIdx.x == 0) {
    float acc = 0.0f;
    for (int j = 0; j < d; ++j) acc = __builtin_fmaf(row[j], row[j], acc);
    s_nrm = acc > 0.0f ? __builtin_sqrtf(acc) : 0.0f;
  }
  __syncthreads();
  const float nrm = s_nrm;
  if (nrm > 0.0f)
    for (int j = threadIdx.x; j < d; j += 256) row[j] = row[j] / nrm;
}
int renorm_rows(float *c, int k, int d) {
  if (k <= 0) return ASL_OK;
  hipLaunchKernelGGL(renorm_rows_kernel, dim3(k), dim3(256), 0, stream(), c, d);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// ------------------------------------------------------------------ L2 arg-min (PQ training and encoding)
// The one rule of the product quantiser, which the oracle tests pin bit for bit
// (profiles/pq_codec_resource_usage.txt): the nearest of the ksub codes cb[c][0..dsub) to one operand per lane,
//   * the distance is the chain acc = fmaf(v[t] - code[t], v[t] - code[t], acc) from +0 over ascending t;
//   * the codes are taken in ascending c with a strict <, from best = 0: the lowest code wins a tie;
//   * RES: v[t] = xi[t] - ci[t] (fp32 subtract), else v[t] = xi[t] and ci is unread (may be null);
//   * the codes are staged in LDS -- the whole codebook, or (ROUNDS: a codebook beyond the 64 KB every kernel
//     may ask for, wide sub-vectors only: d = 800 with m = 4 is 204 800 B) pq_cb_chunk codes at a time, the
//     running (bs, best) carried from one round to the next;
//   * a whole codebook of dsub <= PQ_MAX_DSUB keeps the operand in registers, every other form re-reads it
//     through L1: the same arithmetic;
//   * a lane that is not `live` stages and meets every barrier, reads neither xi nor ci and returns 0.
// Launcher and kernel get the round size from pq_cb_chunk alike.
__host__ __device__ static inline int pq_cb_chunk(int ksub, int dsub) {
  const int fit = 64 * 1024 / 4 / dsub;      // (0: not even one code; asl_index_create accepts no such index)
  return ksub < fit ? ksub : fit;
}
template <bool RES, bool ROUNDS>
__device__ __forceinline__ int l2_argmin(const float *xi, const float *ci, bool live, int dsub,
                                         const float *__restrict__ cb, int ksub, float *s_cb) {
  const int chunk = ROUNDS ? pq_cb_chunk(ksub, dsub) : ksub;
  float bs = INFINITY;
  int best = 0;
  for (int c0 = 0; c0 < ksub; c0 += chunk) {
    const int nc = min(chunk, ksub - c0);
    if (c0) __syncthreads();      // every lane is done with the codes before
    for (int j = threadIdx.x; j < nc * dsub; j += 256) s_cb[j] = cb[(size_t)c0 * dsub + j];
    __syncthreads();
    if (!live) continue;
    if (!ROUNDS && dsub <= PQ_MAX_DSUB) {
      float v[PQ_MAX_DSUB];
#pragma unroll
      for (int t = 0; t < PQ_MAX_DSUB; ++t) v[t] = t < dsub ? (RES ? xi[t] - ci[t] : xi[t]) : 0.0f;
      for (int c = 0; c < nc; ++c) {
        float acc = 0.0f;
#pragma unroll
        for (int t = 0; t < PQ_MAX_DSUB; ++t)
          if (t < dsub) {
            const float df = v[t] - s_cb[c * dsub + t];
            acc = __builtin_fmaf(df, df, acc);
          }
        if (acc < bs) {
          bs = acc;
          best = c0 + c;
        }
      }
    } else {
      for (int c = 0; c < nc; ++c) {
        float acc = 0.0f;
        for (int t = 0; t < dsub; ++t) {
          const float df = (RES ? xi[t] - ci[t] : xi[t]) - s_cb[c * dsub + t];
          acc = __builtin_fmaf(df, df, acc);
        }
        if (acc < bs) {
          bs = acc;
          best = c0 + c;
        }
      }
    }
  }
  return best;
}

// PQ training: x: [n, ld] (sub-vector view), cb: [ksub, dsub]; assign[i] = the nearest code of row i.
template <bool ROUNDS>
__global__ __launch_bounds__(256) void l2_assign_kernel(const float *__restrict__ x, int64_t ld, int64_t n,
                                                        int dsub, const float *__restrict__ cb, int ksub,
                                                        int32_t *__restrict__ assign) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int64_t i = block_linear() * 256 + threadIdx.x;
  const bool live = i < n;
  const int best = l2_argmin<false, ROUNDS>(x + (live ? i : 0) * ld, nullptr, live, dsub, cb, ksub,
                                            reinterpret_cast<float *>(smem));
  if (live) assign[i] = best;
}
int l2_assign(const float *x, int64_t ld, int64_t n, int dsub, const float *cb, int ksub,
              int32_t *assign) {
  if (n <= 0) return ASL_OK;
  const int chunk = pq_cb_chunk(ksub, dsub);
  if (chunk < 1) return fail(ASL_ERR_CAPACITY, "l2_assign: a sub-vector of %d floats does not fit LDS", dsub);
  hipLaunchKernelGGL(chunk == ksub ? l2_assign_kernel<false> : l2_assign_kernel<true>, grid_2d(cdiv(n, 256)),
                     dim3(256), (size_t)chunk * dsub * 4, stream(), x, ld, n, dsub, cb, ksub, assign);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// residual r = x - centroid[assign] (fp32 subtract), in place or to dst
__global__ void residual_kernel(const float *__restrict__ x, const int32_t *__restrict__ assign,
                                const float *__restrict__ centroids, int64_t n, int d,
                                float *__restrict__ dst) {
  const int64_t i = block_linear();
  if (i >= n) return;
  const float *c = centroids + (size_t)assign[i] * d;
  for (int j = threadIdx.x; j < d; j += blockDim.x)
    dst[i * d + j] = x[i * d + j] - c[j];
}
int residual(const float *x, const int32_t *assign, const float *centroids, int64_t n, int d,
             float *dst) {
  if (n <= 0) return ASL_OK;
  hipLaunchKernelGGL(residual_kernel, grid_2d(n), dim3(256), 0, stream(), x, assign,
                     centroids, n, d, dst);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// PQ encode: grid (vector tiles, m). RES: code = argmin_c L2(x_sub - centroid[assign]_sub, cb[m][c]); else (FAISS'
// IndexIVFPQ::by_residual = false) of x_sub itself -- no list assignment, no centroid row.
template <bool RES, bool ROUNDS>
__global__ __launch_bounds__(256) void pq_encode_kernel(
    const float *__restrict__ x, const int32_t *__restrict__ assign,
    const float *__restrict__ centroids, const float *__restrict__ codebooks, int64_t n, int d,
    int m, int ksub, int dsub, uint8_t *__restrict__ codes) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int mi = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n;
  const float *xi = x + (size_t)(live ? i : 0) * d + (size_t)mi * dsub;
  const float *ci = RES ? centroids + (size_t)(live ? assign[i] : 0) * d + (size_t)mi * dsub : nullptr;
  const int best = l2_argmin<RES, ROUNDS>(xi, ci, live, dsub, codebooks + (size_t)mi * ksub * dsub, ksub,
                                          reinterpret_cast<float *>(smem));
  if (live) codes[(size_t)i * m + mi] = (uint8_t)best;
}
int pq_encode(const float *x, const int32_t *assign, const float *centroids,
              const float *codebooks, int64_t n, int d, int m, int ksub, int dsub,
              uint8_t *codes, bool by_residual) {
  if (n <= 0) return ASL_OK;
  const int chunk = pq_cb_chunk(ksub, dsub);
  if (chunk < 1) return fail(ASL_ERR_CAPACITY, "pq_encode: a sub-vector of %d floats does not fit LDS", dsub);
  const bool rounds = chunk != ksub;
  const auto kernel = by_residual ? (rounds ? pq_encode_kernel<true, true> : pq_encode_kernel<true, false>)
                                  : (rounds ? pq_encode_kernel<false, true> : pq_encode_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)cdiv(n, 256), m), dim3(256), (size_t)chunk * dsub * 4, stream(), x,
                     assign, centroids, codebooks, n, d, m, ksub, dsub, codes);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

}  // namespace asl
