// peak_sort.hip -- the stable sort by m/z of the spectra of a raw pack whose peaks descend anywhere (asl_mgf_sort /
// asl_mgf_sort_charged): what both text readers (mgf.py, sptxt.py) run on the packs they fill. gfx950 only.
//
//   one adjacent compare per peak flags the spectra that descend anywhere; those alone are sorted, one workgroup
//   each, by a bitonic network over at most 4096 unique keys (m/z bits, ordinal) in LDS; asl_mgf_sort_charged moves
//   the fragment charges of a library's peaks with them, a third payload
//
// Integer atomics only, and none whose arrival order reaches the output (the order of the list of flagged spectra
// decides only which workgroup sorts which spectrum).
#include "common.hpp"

namespace asl {

constexpr int MG_NT = ASL_MGF_TILE;            // threads of every kernel here, as in the readers (SCAN_NT there)
constexpr int MG_MAX_PEAKS = ASL_MGF_MAX_PEAKS;
static_assert((MG_MAX_PEAKS & (MG_MAX_PEAKS - 1)) == 0, "the bitonic network pads to a power of two");

__global__ __launch_bounds__(MG_NT) void mgf_descending_kernel(const int32_t *__restrict__ offsets,
                                                               const float *__restrict__ mz, int32_t n_spec,
                                                               int64_t n_peaks, uint32_t *__restrict__ flag,
                                                               uint32_t *__restrict__ list,
                                                               uint32_t *__restrict__ n_list) {
  const int64_t i = (int64_t)blockIdx.x * MG_NT + threadIdx.x;
  if (i + 1 >= n_peaks || !(mz[i + 1] < mz[i])) return;
  int lo = 0, hi = n_spec;            // the last spectrum with offsets[s] <= i
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)offsets[mid] <= i) lo = mid; else hi = mid;
  }
  if (i + 1 >= (int64_t)offsets[lo + 1]) return;   // the pair straddles two spectra
  if (atomicExch(&flag[lo], 1u) == 0u) list[atomicAdd(n_list, 1u)] = (uint32_t)lo;   // (once per spectrum)
}

// Ascending in (float32 m/z, file order): -0.0 and +0.0 are one key, as in numpy's stable argsort.
__device__ __forceinline__ uint64_t mg_sort_key(float mz, uint32_t ordinal) {
  uint32_t u = mz == 0.0f ? 0u : __float_as_uint(mz);
  u = (u >> 31) ? ~u : (u | 0x80000000u);
  return ((uint64_t)u << 32) | ordinal;
}

__global__ __launch_bounds__(MG_NT) void mgf_sort_kernel(const uint32_t *__restrict__ list,
                                                         const int32_t *__restrict__ offsets,
                                                         const float *__restrict__ mz,
                                                         const float *__restrict__ intensity,
                                                         const uint8_t *__restrict__ charge,
                                                         float *__restrict__ mz_tmp, float *__restrict__ it_tmp,
                                                         uint8_t *__restrict__ chg_tmp,
                                                         uint32_t *__restrict__ too_long) {
  __shared__ uint64_t key[MG_MAX_PEAKS];
  const uint32_t s = list[blockIdx.x];
  const int a = offsets[s], cnt = offsets[s + 1] - a;
  if (cnt > MG_MAX_PEAKS) {            // (the same for the whole workgroup)
    if (threadIdx.x == 0) atomicOr(too_long, 1u);
    return;
  }
  int P = 2;
  while (P < cnt) P <<= 1;
  for (int i = threadIdx.x; i < P; i += MG_NT) key[i] = i < cnt ? mg_sort_key(mz[a + i], (uint32_t)i) : ~0ull;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < P; i += MG_NT) {
        const int o = i ^ j;
        if (o > i) {
          const uint64_t x = key[i], y = key[o];
          if ((x > y) == ((i & k) == 0)) key[i] = y, key[o] = x;
        }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < cnt; i += MG_NT) {
    const int src = (int)(uint32_t)key[i];
    mz_tmp[a + i] = mz[a + src], it_tmp[a + i] = intensity[a + src];
    if (charge != nullptr) chg_tmp[a + i] = charge[a + src];
  }
}

__global__ __launch_bounds__(MG_NT) void mgf_sort_copy_kernel(const uint32_t *__restrict__ list,
                                                              const int32_t *__restrict__ offsets,
                                                              const float *__restrict__ mz_tmp,
                                                              const float *__restrict__ it_tmp,
                                                              const uint8_t *__restrict__ chg_tmp,
                                                              float *__restrict__ mz, float *__restrict__ intensity,
                                                              uint8_t *__restrict__ charge) {
  const uint32_t s = list[blockIdx.x];
  const int a = offsets[s], cnt = offsets[s + 1] - a;
  if (cnt > MG_MAX_PEAKS) return;
  for (int i = threadIdx.x; i < cnt; i += MG_NT) {
    mz[a + i] = mz_tmp[a + i], intensity[a + i] = it_tmp[a + i];
    if (charge != nullptr) charge[a + i] = chg_tmp[a + i];
  }
}

namespace {

struct SortWork {   // grow-only device workspace
  DevBuf<uint32_t> flag, list, small;
  DevBuf<float> mz_tmp, it_tmp;
  DevBuf<uint8_t> chg_tmp;
};
SortWork &work() {
  static SortWork w;
  return w;
}

}  // namespace
}  // namespace asl

using namespace asl;

extern "C" int asl_mgf_sort(const int32_t *offsets, float *mz, float *intensity, int32_t n_spectra, int64_t n_peaks,
                            int64_t *n_sorted) {
  return asl_mgf_sort_charged(offsets, mz, intensity, nullptr, n_spectra, n_peaks, n_sorted);
}

extern "C" int asl_mgf_sort_charged(const int32_t *offsets, float *mz, float *intensity, uint8_t *charge,
                                    int32_t n_spectra, int64_t n_peaks, int64_t *n_sorted) {
  clear_error();
  if (n_spectra < 0 || n_peaks < 0) return fail(ASL_ERR_INVALID, "mgf_sort: a negative count");
  if (n_peaks >= ((int64_t)1 << 31)) return fail(ASL_ERR_CAPACITY, "mgf_sort: n_peaks = %lld, below 2^31",
                                                 (long long)n_peaks);
  if (n_sorted != nullptr) *n_sorted = 0;
  if (n_spectra == 0 || n_peaks < 2) return ASL_OK;
  if (!offsets || !mz || !intensity) return fail(ASL_ERR_INVALID, "mgf_sort: null offsets / mz / intensity");
  ASL_TRY(ensure_device());
  if (!is_device_ptr(offsets) || !is_device_ptr(mz) || !is_device_ptr(intensity))
    return fail(ASL_ERR_INVALID, "mgf_sort: the pack must be device memory");
  if (charge != nullptr && !is_device_ptr(charge))
    return fail(ASL_ERR_INVALID, "mgf_sort: the charges must be device memory");
  SortWork &W = work();
  ProfScope ps("mgf_sort");
  ASL_TRY(W.flag.reserve((size_t)n_spectra));
  ASL_TRY(W.list.reserve((size_t)n_spectra));
  ASL_TRY(W.small.reserve(2));     // [0]: flagged spectra, [1]: one of them is above the capacity
  HIP_TRY(hipMemsetAsync(W.flag.p, 0, (size_t)n_spectra * sizeof(uint32_t), stream()));
  HIP_TRY(hipMemsetAsync(W.small.p, 0, 2 * sizeof(uint32_t), stream()));
  hipLaunchKernelGGL(mgf_descending_kernel, dim3((unsigned)cdiv(n_peaks, MG_NT)), dim3(MG_NT), 0, stream(), offsets, mz,
                     n_spectra, n_peaks, W.flag.p, W.list.p, W.small.p);
  ASL_CHECK_LAUNCH();
  uint32_t h[2] = {0u, 0u};
  HIP_TRY(hipMemcpyAsync(h, W.small.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream()));
  ASL_TRY(sync_stream());
  if (n_sorted != nullptr) *n_sorted = h[0];
  if (h[0] == 0u) return ASL_OK;   // ascending everywhere: no sort is launched
  ASL_TRY(W.mz_tmp.reserve((size_t)n_peaks));
  ASL_TRY(W.it_tmp.reserve((size_t)n_peaks));
  if (charge != nullptr) ASL_TRY(W.chg_tmp.reserve((size_t)n_peaks));
  hipLaunchKernelGGL(mgf_sort_kernel, dim3(h[0]), dim3(MG_NT), 0, stream(), W.list.p, offsets, mz, intensity,
                     charge, W.mz_tmp.p, W.it_tmp.p, W.chg_tmp.p, W.small.p + 1);
  ASL_CHECK_LAUNCH();
  hipLaunchKernelGGL(mgf_sort_copy_kernel, dim3(h[0]), dim3(MG_NT), 0, stream(), W.list.p, offsets, W.mz_tmp.p,
                     W.it_tmp.p, W.chg_tmp.p, mz, intensity, charge);
  ASL_CHECK_LAUNCH();
  HIP_TRY(hipMemcpyAsync(h, W.small.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream()));
  ASL_TRY(sync_stream());
  if (h[1] != 0u)
    return fail(ASL_ERR_CAPACITY, "mgf_sort: a descending spectrum has more than %d peaks", MG_MAX_PEAKS);
  return ASL_OK;
}
