// text_scan.hpp -- what the text readers share (mgf.hip, sptxt.hip, mzml.hip) below their records: the unit-start
// pass over a chunk of text -- the lines behind a '\n', or the tags at a '<' -- and the blanks of bytes.strip, on the
// scan of device_scan.hpp. gfx950 only. What the readers share about records -- counts, stores, the host's measure
// and fill -- is text_records.hpp, which includes this header.
//
// Every kernel of the readers has SCAN_NT threads. Everything here has internal linkage, as in device_scan.hpp:
// each translation unit that includes the header holds its own kernels.
#pragma once
#include <algorithm>

#include "device_scan.hpp"

namespace asl {
namespace {

constexpr int MG_SPAN = 16;                    // bytes per thread of the line-start passes
static_assert(ASL_MGF_TILE == SCAN_NT, "mgf.SCAN_TILE is the scan's block");

// ---------------------------------------------------------------------------------------------- unit starts
// B: the byte that delimits the units. B == '\n': a line starts behind it, and at byte 0; the table's entry is the
// byte after the '\n'. Any other B (the '<' of a tag): the unit starts at the byte itself, bytes before the first
// one belong to no unit, and a chunk may hold none.
// Bit k of the result: byte 16 e + k is a B ('\n': one that is followed by another byte, i.e. byte 16 e + k + 1
// starts a line). vec: t is 16-byte aligned.
template <uint8_t B>
__device__ __forceinline__ uint32_t mg_newlines(const uint8_t *__restrict__ t, int64_t n, int64_t e, bool vec) {
  const int64_t j0 = e * MG_SPAN;
  uint32_t m = 0u;
  if (vec && j0 + MG_SPAN <= n) {
    const uint4 v = *reinterpret_cast<const uint4 *>(t + j0);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (((w[q] >> (8 * b)) & 255u) == (uint32_t)B) m |= 1u << (4 * q + b);
  } else {
    for (int k = 0; k < MG_SPAN; ++k)
      if (j0 + k < n && t[j0 + k] == B) m |= 1u << k;
  }
  const int64_t last = n - 1 - j0;   // (the chunk's last byte starts nothing behind it)
  if (B == (uint8_t)'\n' && last >= 0 && last < MG_SPAN) m &= ~(1u << last);
  return m;
}
template <uint8_t B>
__device__ __forceinline__ uint32_t mg_starts(const uint8_t *__restrict__ t, int64_t n, int64_t e, bool vec) {
  return (uint32_t)__popc(mg_newlines<B>(t, n, e, vec)) + (B == (uint8_t)'\n' && e == 0 && n > 0 ? 1u : 0u);
}

template <uint8_t B>
__global__ __launch_bounds__(SCAN_NT) void mgf_count_lines_kernel(const uint8_t *__restrict__ t, int64_t n, int64_t ne,
                                                                int vec, unsigned long long *__restrict__ total) {
  const int64_t e = (int64_t)blockIdx.x * SCAN_NT + threadIdx.x;
  uint32_t tot;
  block_scan<SumU32>(e < ne ? mg_starts<B>(t, n, e, vec != 0) : 0u, &tot);
  if (threadIdx.x == 0 && tot != 0u) atomicAdd(total, (unsigned long long)tot);   // (an integer count)
}

template <uint8_t B>
struct LineStartView {   // element e: the unit starts its MG_SPAN bytes produce, in file order
  using Op = SumU32;
  const uint8_t *t;
  int64_t n;
  int vec;
  uint32_t *line_start;   // [n_lines + 1]
  uint32_t n_lines;
  __device__ uint32_t load(int64_t e) const { return mg_starts<B>(t, n, e, vec != 0); }
  __device__ void store(int64_t e, uint32_t incl, uint32_t own) const {
    uint32_t o = incl - own;
    constexpr uint32_t behind = B == (uint8_t)'\n' ? 1u : 0u;
    if (behind != 0u && e == 0 && n > 0 && o < n_lines) line_start[o++] = 0u;
    uint32_t m = mg_newlines<B>(t, n, e, vec != 0);
    while (m != 0u) {
      const int k = __ffs((int)m) - 1;
      m &= m - 1u;
      if (o < n_lines) line_start[o++] = (uint32_t)(e * MG_SPAN + k) + behind;
    }
  }
};

// ---------------------------------------------------------------------------------------------- bytes
__device__ __forceinline__ bool mg_ws(uint8_t c) { return c == 32 || (c >= 9 && c <= 13); }   // bytes.strip / split

// [p, q): line L without the blanks around it (a == b gives p == q)
__device__ __forceinline__ void mg_strip(const uint8_t *__restrict__ t, uint32_t a, uint32_t b, uint32_t *p,
                                         uint32_t *q) {
  while (b > a && mg_ws(t[b - 1])) --b;
  while (a < b && mg_ws(t[a])) ++a;
  *p = a, *q = b;
}

// ---------------------------------------------------------------------------------------------- host
inline unsigned blocks_of(int64_t n) { return (unsigned)std::max<int64_t>(cdiv(n, SCAN_NT), 1); }

// The unit starts of the chunk text[0 .. n), n > 0: *n_lines (lines: >= 1; tags: >= 0) and line_start[0 .. *n_lines],
// the last entry being n. count: one word; partial: grown to what a scan over max(spans, units) elements needs.
template <uint8_t B = (uint8_t)'\n', class P>
int line_starts(const uint8_t *text, int64_t n, DevBuf<unsigned long long> &count, DevBuf<P> &partial,
                DevBuf<uint32_t> &line_start, int64_t *n_lines) {
  const int vec = (reinterpret_cast<uintptr_t>(text) & 15u) == 0 ? 1 : 0;
  const int64_t ne = cdiv(n, MG_SPAN);
  ASL_TRY(count.reserve(1));
  HIP_TRY(hipMemsetAsync(count.p, 0, sizeof(unsigned long long), stream()));
  hipLaunchKernelGGL(mgf_count_lines_kernel<B>, dim3(blocks_of(ne)), dim3(SCAN_NT), 0, stream(), text, n, ne, vec,
                     count.p);
  ASL_CHECK_LAUNCH();
  unsigned long long h_lines = 0;
  HIP_TRY(hipMemcpyAsync(&h_lines, count.p, sizeof(h_lines), hipMemcpyDeviceToHost, stream()));
  ASL_TRY(sync_stream());
  const int64_t nl = (int64_t)h_lines;
  ASL_TRY(partial.reserve((size_t)(partial_slots(std::max(ne, nl)) + 1)));
  ASL_TRY(line_start.reserve((size_t)nl + 1));
  ASL_TRY(scan_view(LineStartView<B>{text, n, vec, line_start.p, (uint32_t)nl}, ne, partial.p));
  HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(line_start.p + nl), (int)(uint32_t)n, 1, stream()));
  *n_lines = nl;
  return ASL_OK;
}

}  // namespace
}  // namespace asl
