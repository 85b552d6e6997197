// text_records.hpp -- what the readers of record-structured text share beyond the scans of text_scan.hpp (mgf.hip,
// sptxt.hip, mzml.hip; a "line" here is the format's unit: mzml.hip's is a tag): the counts scan's operator, the result block of a measure, the guard of a line walk, the peak and
// deferred-token stores, the capacity check, and on the host the workspace of a measured chunk with the grammar-free
// parts of asl_*_measure / asl_*_fill. gfx950 only. Everything here has internal linkage, as in text_scan.hpp; the
// grammars -- what a line is, what opens and closes a record -- stay in their units.
#pragma once
#include "text_scan.hpp"

namespace asl {
namespace {

static_assert(ASL_MGF_N_LINES == ASL_SPTXT_N_LINES && ASL_MGF_N_SPECTRA == ASL_SPTXT_N_RECORDS &&
                  ASL_MGF_N_PEAKS == ASL_SPTXT_N_PEAKS && ASL_MGF_N_DEFERRED == ASL_SPTXT_N_DEFERRED &&
                  ASL_MGF_ERR_KIND == ASL_SPTXT_ERR_KIND && ASL_MGF_ERR_LINE == ASL_SPTXT_ERR_LINE &&
                  ASL_MGF_COUNTS == ASL_SPTXT_COUNTS,
              "one layout of counts[]: the host parts below index it by the MGF names");

struct TextFinal {   // written by the line, resolve and capacity kernels
  unsigned long long err;   // (line << 8 | kind) of the first structural error, ~0: none
  uint32_t n_peaks, n_def;  // before the first record that is not closed
  uint32_t cap_rec;         // first record above ASL_MGF_MAX_PEAKS, ~0: none
  uint32_t long_line;       // first line (unit) above its cap in bytes, ~0: none
};

// The counts scan over a format's totals: the fields named in Sum are summed, of cons_byte and cons_line (byte and
// line up to which the chunk's records are closed) the maximum is taken. Totals holds nothing else.
template <class Totals, uint32_t Totals::*...Sum>
struct TextCount {
  using T = Totals;
  static_assert(sizeof(T) == 4 * (sizeof...(Sum) + 2), "a field of the totals is neither summed nor a maximum");
  __device__ static T identity() { return T{}; }
  __device__ static T op(T a, T b) {
    T r = {};
    ((r.*Sum = a.*Sum + b.*Sum), ...);
    r.cons_byte = a.cons_byte > b.cons_byte ? a.cons_byte : b.cons_byte;
    r.cons_line = a.cons_line > b.cons_line ? a.cons_line : b.cons_line;
    return r;
  }
};

// Is line L = [a, b) walked? A thread walks its line byte by byte: a line beyond the cap is not walked at all (the
// call fails). The final line of a chunk that is not the file's last may be cut anywhere: it is not looked at either.
__device__ __forceinline__ bool text_walks_line(const uint8_t *__restrict__ t, uint32_t a, uint32_t b, int64_t L,
                                                int64_t n_lines, int last, TextFinal *__restrict__ fin) {
  const bool too_long = b - a > (uint32_t)ASL_MGF_MAX_LINE;
  if (too_long) atomicMin(&fin->long_line, (uint32_t)L);
  return !(too_long || (last == 0 && L == n_lines - 1 && t[b - 1] != (uint8_t)'\n'));
}

__device__ __forceinline__ uint64_t pack_peak(double mz, double it) {
  return (uint64_t)__float_as_uint((float)mz) | ((uint64_t)__float_as_uint((float)it) << 32);
}
__device__ __forceinline__ void put_peak(float *__restrict__ mz, float *__restrict__ intensity, uint32_t o,
                                         uint64_t v) {
  mz[o] = __uint_as_float((uint32_t)v), intensity[o] = __uint_as_float((uint32_t)(v >> 32));
}
// rec: [n_def, 5] (offset, length, destination kind, destination index, line); r < n_def is the caller's to check
__device__ __forceinline__ void put_deferred(int32_t *__restrict__ rec, uint32_t r, uint32_t begin, uint32_t end,
                                             int dest, uint32_t index, int64_t line) {
  int32_t *o = rec + (size_t)r * 5;
  o[0] = (int32_t)begin, o[1] = (int32_t)(end - begin), o[2] = dest, o[3] = (int32_t)index, o[4] = (int32_t)line;
}

// close_last: the file's end closes the last record, at peak slot end_peaks (else every record has its end already).
// (unused by mzml.hip, whose peak counts are an attribute of the record.)
__attribute__((unused)) __global__ __launch_bounds__(SCAN_NT) void text_capacity_kernel(const uint32_t *__restrict__ peak_begin,
                                                              uint32_t *__restrict__ peak_end, uint32_t n_rec,
                                                              int close_last, uint32_t end_peaks,
                                                              TextFinal *__restrict__ fin) {
  const uint32_t s = blockIdx.x * SCAN_NT + threadIdx.x;
  if (s >= n_rec) return;
  if (close_last != 0 && s + 1u == n_rec) peak_end[s] = end_peaks;
  if (peak_end[s] - peak_begin[s] > (uint32_t)ASL_MGF_MAX_PEAKS) atomicMin(&fin->cap_rec, s);
}

// ---------------------------------------------------------------------------------------------- host
// Grow-only device workspace of one reader; its fill reads what the measure before it left here. A format adds the
// buffers of its own grammar.
template <class Totals>
struct ChunkWork {
  DevBuf<uint32_t> line_start, rec, slot, dslot, first_line, peak_begin, peak_end;
  DevBuf<uint8_t> kind, dflag, after;
  DevBuf<uint64_t> val;
  DevBuf<unsigned long long> count;
  DevBuf<Totals> partial, totals;
  DevBuf<TextFinal> fin;
  // the measured chunk
  const void *text = nullptr;
  int64_t n = -1, n_lines = 0;
  uint32_t n_rec = 0, n_peaks = 0, n_def = 0;
  uint32_t n_blocks = 0;   // records whose deferred tokens are listed
};

// The head of asl_<who>_measure: the arguments, counts[] cleared, nothing left to fill until the call succeeds; the
// empty chunk is measured here (n == 0: the caller returns).
template <class W>
int measure_begin(const char *who, W &w, const uint8_t *text, int64_t n, int32_t last, int64_t *counts) {
  if (n >= ((int64_t)1 << 31)) return fail(ASL_ERR_CAPACITY, "%s_measure: n = %lld, below 2^31", who, (long long)n);
  if (n < 0) return fail(ASL_ERR_INVALID, "%s_measure: n < 0", who);
  if (counts == nullptr) return fail(ASL_ERR_INVALID, "%s_measure: null counts", who);
  if (last != 0 && last != 1) return fail(ASL_ERR_INVALID, "%s_measure: last = %d, 0 or 1", who, (int)last);
  w.text = nullptr, w.n = -1;
  for (int k = 0; k < ASL_MGF_COUNTS; ++k) counts[k] = 0;
  counts[ASL_MGF_ERR_LINE] = -1;
  if (n == 0) {
    w.text = text, w.n = 0, w.n_lines = 0, w.n_rec = w.n_peaks = w.n_def = w.n_blocks = 0;
    return ASL_OK;
  }
  if (text == nullptr) return fail(ASL_ERR_INVALID, "%s_measure: null text", who);
  ASL_TRY(ensure_device());
  if (!is_device_ptr(text)) return fail(ASL_ERR_INVALID, "%s_measure: text must be device memory", who);
  return ASL_OK;
}

// The columns every format keeps per line, for the nl lines line_starts found, and the kernels' result block
template <class W>
int measure_lines(W &w, int64_t nl) {
  ASL_TRY(w.kind.reserve((size_t)nl));
  ASL_TRY(w.dflag.reserve((size_t)nl));
  ASL_TRY(w.after.reserve((size_t)nl));
  ASL_TRY(w.val.reserve((size_t)nl));
  ASL_TRY(w.rec.reserve((size_t)nl));
  ASL_TRY(w.slot.reserve((size_t)nl));
  ASL_TRY(w.dslot.reserve((size_t)nl));
  ASL_TRY(w.totals.reserve(1));
  ASL_TRY(w.fin.reserve(1));
  const TextFinal F{~0ull, 0u, 0u, ~0u, ~0u};
  HIP_TRY(hipMemcpyAsync(w.fin.p, &F, sizeof(F), hipMemcpyHostToDevice, stream()));
  return ASL_OK;
}

// The result block read back (the call's last synchronisation); a unit (a line, a tag) above its cap fails the call
// here, before the format fills counts[].
template <class W>
int measure_final(const char *who, W &w, TextFinal *F, const char *unit = "line", int cap = ASL_MGF_MAX_LINE) {
  HIP_TRY(hipMemcpyAsync(F, w.fin.p, sizeof(*F), hipMemcpyDeviceToHost, stream()));
  ASL_TRY(sync_stream());
  if (F->long_line != ~0u)
    return fail(ASL_ERR_CAPACITY, "%s_measure: %s %u of the chunk is longer than %d bytes", who, unit,
                (unsigned)F->long_line + 1u, cap);
  return ASL_OK;
}

// The tail of asl_<who>_measure, behind the format's counts[]: the first structural error, the capacity (noun: what
// the format calls a record), and the measured chunk remembered for the fill.
template <class W>
int measure_end(const char *who, const char *noun, W &w, const TextFinal &F, const uint8_t *text, int64_t n,
                int64_t *counts, const char *peaks = "peak lines") {
  if (F.err != ~0ull) {
    counts[ASL_MGF_ERR_KIND] = (int64_t)(F.err & 255u);
    counts[ASL_MGF_ERR_LINE] = (int64_t)(F.err >> 8);
  }
  if (F.cap_rec != ~0u)
    return fail(ASL_ERR_CAPACITY, "%s_measure: %s %u of the chunk has more than %d %s", who, noun,
                (unsigned)F.cap_rec + 1u, ASL_MGF_MAX_PEAKS, peaks);
  w.text = text, w.n = n, w.n_lines = counts[ASL_MGF_N_LINES], w.n_rec = (uint32_t)counts[ASL_MGF_N_SPECTRA];
  w.n_peaks = (uint32_t)counts[ASL_MGF_N_PEAKS], w.n_def = (uint32_t)counts[ASL_MGF_N_DEFERRED];
  return ASL_OK;
}

// The head of asl_<who>_fill
template <class W>
int fill_begin(const char *who, const W &w, const void *text, int64_t n, const int32_t *offsets) {
  if (w.n < 0 || text != w.text || n != w.n)
    return fail(ASL_ERR_STATE, "%s_fill: not the chunk the last successful asl_%s_measure measured", who, who);
  if (offsets == nullptr) return fail(ASL_ERR_INVALID, "%s_fill: null offsets", who);
  return ASL_OK;
}
// ... and all of it when the chunk closed nothing: offsets[0] = 0, on the host or the device
inline int fill_empty(int32_t *offsets) {
  if (is_device_ptr(offsets)) {
    HIP_TRY(hipMemsetAsync(offsets, 0, sizeof(int32_t), stream()));
    ASL_TRY(sync_stream());
  } else {
    offsets[0] = 0;
  }
  return ASL_OK;
}
// The copies back of a fill's host outputs, in the order given, and the call's one synchronisation
template <class... O>
int finish_outputs(O &...outs) {
  int rc = ASL_OK;
  (void)(... && ((rc = outs.finish()) == ASL_OK));
  return rc != ASL_OK ? rc : sync_stream();
}

}  // namespace
}  // namespace asl
