// device_scan.hpp -- the device-wide scan of the units off the search hot path (text_scan.hpp for mgf.hip and
// sptxt.hip, tdc.hip, groups.hip): the block scan, its reduce / apply kernels and the host's driver. gfx950 only.
//
// Every scan is reduce -> scan of the block partials (recursively) -> apply, as separate launches on the library's
// stream: no kernel waits on another workgroup. Everything here has internal linkage: each translation unit is its
// own code object and holds its own kernels (with external linkage, one instantiation would exist under one name in
// several objects).
#pragma once
#include "common.hpp"

namespace asl {
namespace {

constexpr int SCAN_NT = 256;   // threads per block = elements per block of a scan level
static_assert(SCAN_NT == 4 * 64, "four waves: block_scan's wave totals");

struct SumU32 {
  using T = uint32_t;
  __device__ static T identity() { return 0u; }
  __device__ static T op(T a, T b) { return a + b; }
};

template <class T>
__device__ __forceinline__ T shfl_up_words(T v, int delta) {
  static_assert(sizeof(T) % 4 == 0, "whole words");
  uint32_t w[sizeof(T) / 4];
  __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
  for (size_t k = 0; k < sizeof(T) / 4; ++k) w[k] = (uint32_t)__shfl_up((int)w[k], delta, 64);
  __builtin_memcpy(&v, w, sizeof(T));
  return v;
}

// inclusive scan over the block's SCAN_NT values in thread order; *total: the block's sum, in every thread. A
// second call in one kernel needs a __syncthreads() in between (the wave totals are read until every wave is here).
template <class Op>
__device__ __forceinline__ typename Op::T block_scan(typename Op::T x, typename Op::T *total) {
  using T = typename Op::T;
  __shared__ T wave_tot[SCAN_NT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = shfl_up_words(x, d);
    if (lane >= d) x = Op::op(o, x);
  }
  if (lane == 63) wave_tot[wave] = x;
  __syncthreads();
  T pre = Op::identity(), all = Op::identity();
#pragma unroll
  for (int w = 0; w < SCAN_NT / 64; ++w) {
    if (w < wave) pre = Op::op(pre, wave_tot[w]);
    all = Op::op(all, wave_tot[w]);
  }
  *total = all;
  return Op::op(pre, x);
}

// A view names a scan's operator (Op), reads element i (load) and takes its inclusive result (store).
template <class V>
__global__ __launch_bounds__(SCAN_NT) void scan_reduce_kernel(V view, int64_t n, typename V::Op::T *partial) {
  using Op = typename V::Op;
  const int64_t i = (int64_t)blockIdx.x * SCAN_NT + threadIdx.x;
  typename Op::T total;
  block_scan<Op>(i < n ? view.load(i) : Op::identity(), &total);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}
// partial: the INCLUSIVE scan of the blocks' sums (block b starts from partial[b - 1]), or nullptr for one block
template <class V>
__global__ __launch_bounds__(SCAN_NT) void scan_apply_kernel(V view, int64_t n, const typename V::Op::T *partial) {
  using Op = typename V::Op;
  const int64_t i = (int64_t)blockIdx.x * SCAN_NT + threadIdx.x;
  const typename Op::T own = i < n ? view.load(i) : Op::identity();
  typename Op::T total;
  typename Op::T incl = block_scan<Op>(own, &total);
  if (partial != nullptr && blockIdx.x > 0) incl = Op::op(partial[blockIdx.x - 1], incl);
  if (i < n) view.store(i, incl, own);
}

template <class O>
struct PlainView {   // an array scanned in place (the upper levels)
  using Op = O;
  typename O::T *a;
  __device__ typename O::T load(int64_t i) const { return a[i]; }
  __device__ void store(int64_t i, typename O::T incl, typename O::T) const { a[i] = incl; }
};

inline int64_t partial_slots(int64_t n) {   // block partials of all levels of a scan over n elements
  int64_t total = 0;
  while (n > SCAN_NT) {
    n = cdiv(n, SCAN_NT);
    total += n;
  }
  return total;
}

// scratch: room for partial_slots(n) elements of the operator's type (a unit sizes one buffer for its widest)
template <class V>
int scan_view(const V &v, int64_t n, void *scratch_bytes) {
  using T = typename V::Op::T;
  T *scratch = static_cast<T *>(scratch_bytes);
  const int64_t nb = cdiv(n, SCAN_NT);
  if (nb > 1) {
    hipLaunchKernelGGL(scan_reduce_kernel<V>, dim3((unsigned)nb), dim3(SCAN_NT), 0, stream(), v, n, scratch);
    ASL_CHECK_LAUNCH();
    ASL_TRY(scan_view(PlainView<typename V::Op>{scratch}, nb, scratch + nb));
  }
  hipLaunchKernelGGL(scan_apply_kernel<V>, dim3((unsigned)nb), dim3(SCAN_NT), 0, stream(), v, n,
                     nb > 1 ? scratch : nullptr);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

}  // namespace
}  // namespace asl
