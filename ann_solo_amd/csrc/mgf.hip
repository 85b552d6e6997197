// mgf.hip -- MGF query files parsed on the device (asl_mgf_measure / asl_mgf_fill) and the numeral converter on the
// host (asl_mgf_number). gfx950 only. DESIGN.md 3 "Query files"; the dialect is stated in include/annsolo_mi.h and
// restated in tests/mgf_ref.py. Shared with sptxt.hip: the scans and the line starts (text_scan.hpp); the counts
// operator, the walk guard, the peak and deferred-token stores, the capacity check and the grammar-free host parts
// of measure and fill (text_records.hpp). The sort of descending spectra, asl_mgf_sort, is peak_sort.hip.
//
//   starts   count the line starts (MG_SPAN bytes a thread), scan the counts, write line_start[] (text_scan.hpp)
//   lines    one thread per line: strip, classify (BEGIN, END, the five parameters, other parameter, peak, skip)
//            and convert its numerals (mgf_number.hpp); what the converter defers is flagged, never guessed
//   state    a scan that composes the lines' maps of the two states {outside, inside a block}: BEGIN -> inside,
//            END -> outside, anything else keeps the state. (A +1 / -1 depth sum would go negative on a stray
//            END outside a block, which the dialect ignores; the composed maps saturate by construction.)
//   counts   a scan of (blocks opened, blocks closed, in-block peaks, in-block deferred tokens, byte and line
//            behind the last closed block): spectrum ordinal, peak slot and deferred slot of every line
//   resolve  per line: nested BEGIN / one-token peak line -> the first structural error (integer atomicMin of
//            line << 8 | kind); "the last duplicate wins" -> integer atomicMax of the line number per (spectrum,
//            key); BEGIN and END lines record their block's extent
//   fill     peaks scattered to their slots, the deferred tokens' byte ranges and destinations, the per-spectrum
//            columns
//
// Every scan is reduce -> scan of the block partials (recursively) -> apply, as separate launches on the library's
// stream: no kernel waits on another workgroup. Integer atomics only, and none whose arrival order reaches the
// output. Every byte index is bounded by the chunk length and every line by line_start[n_lines] == n.
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "mgf_number.hpp"
#include "text_records.hpp"

namespace asl {

enum : uint8_t {   // what a line is, whatever surrounds it
  MK_SKIP = 0, MK_BEGIN, MK_END, MK_TITLE, MK_SCAN, MK_PEPMASS, MK_CHARGE, MK_RT, MK_OTHER, MK_PEAK, MK_PEAK1
};
constexpr int MG_KEYS = 5;                     // MK_TITLE .. MK_RT

struct MgTotals {   // the counts scan's result over all lines
  uint32_t opens, closes, peaks, defers, cons_byte, cons_line;
};
using MgCount = TextCount<MgTotals, &MgTotals::opens, &MgTotals::closes, &MgTotals::peaks, &MgTotals::defers>;

// ---------------------------------------------------------------------------------------------- scans
// A line as a map of the block state: bit x of the value is the state after the line when the state before is x.
struct MgState {
  using T = uint32_t;
  __device__ static T identity() { return 2u; }
  __device__ static T op(T a, T b) { return ((b >> (a & 1u)) & 1u) | (((b >> ((a >> 1) & 1u)) & 1u) << 1); }
};

// ---------------------------------------------------------------------------------------------- one line
__device__ __forceinline__ bool mg_is(const uint8_t *__restrict__ t, uint32_t p, uint32_t len, const char *lit,
                                      uint32_t lit_len, bool fold) {
  if (len != lit_len) return false;
  for (uint32_t k = 0; k < lit_len; ++k) {
    uint8_t c = t[p + k];
    if (fold && c >= 'A' && c <= 'Z') c += 32;
    if (c != (uint8_t)lit[k]) return false;
  }
  return true;
}
__device__ __forceinline__ uint32_t mg_find(const uint8_t *__restrict__ t, uint32_t p, uint32_t q, uint8_t c) {
  while (p < q && t[p] != c) ++p;
  return p;
}
__device__ __forceinline__ uint32_t mg_token_end(const uint8_t *__restrict__ t, uint32_t p, uint32_t q) {
  while (p < q && !mg_ws(t[p])) ++p;
  return p;
}
__device__ __forceinline__ uint32_t mg_skip_ws(const uint8_t *__restrict__ t, uint32_t p, uint32_t q) {
  while (p < q && mg_ws(t[p])) ++p;
  return p;
}
// The two tokens a peak line reads; t1a == q: there is no second one.
struct MgPeakTokens {
  uint32_t t0a, t0b, t1a, t1b;
};
__device__ __forceinline__ MgPeakTokens mg_peak_tokens(const uint8_t *__restrict__ t, uint32_t p, uint32_t q) {
  MgPeakTokens k;
  k.t0a = p;
  k.t0b = mg_token_end(t, p, q);
  k.t1a = mg_skip_ws(t, k.t0b, q);
  k.t1b = mg_token_end(t, k.t1a, q);
  return k;
}
// The numeral a PEPMASS (first token of the value) or RTINSECONDS (the whole value) line reads; [p, q) stripped.
__device__ __forceinline__ void mg_param_token(const uint8_t *__restrict__ t, uint32_t p, uint32_t q, uint8_t kind,
                                               uint32_t *ta, uint32_t *tb) {
  const uint32_t v = mg_skip_ws(t, mg_find(t, p, q, (uint8_t)'=') + 1u, q);   // ('=' exists: v <= q)
  *ta = v < q ? v : q;
  *tb = kind == MK_PEPMASS ? mg_token_end(t, *ta, q) : q;
}
// The first element of a charge list: digits with the sign before or behind them; what follows is the end, a
// comma or "and". 1 .. 255, else -1.
__device__ __forceinline__ int mg_charge(const uint8_t *__restrict__ t, uint32_t i, uint32_t q) {
  int sign = 0;
  if (i < q && (t[i] == '+' || t[i] == '-')) sign = t[i++] == '-' ? -1 : 1;
  int v = 0, nd = 0;
  for (; i < q && t[i] >= '0' && t[i] <= '9'; ++i, ++nd)
    if (v < 100000) v = v * 10 + (t[i] - '0');
  if (nd == 0) return -1;
  if (sign == 0 && i < q && (t[i] == '+' || t[i] == '-')) sign = t[i++] == '-' ? -1 : 1;
  i = mg_skip_ws(t, i, q);
  const bool ends = i == q || t[i] == ',' || (q - i >= 3u && t[i] == 'a' && t[i + 1] == 'n' && t[i + 2] == 'd');
  if (!ends || sign < 0 || v < 1 || v > 255) return -1;
  return v;
}

// kind, dflag (bit k: numeral k of the line was deferred) and val (a peak's two float32, a parameter's double or
// charge) of every line
__global__ __launch_bounds__(SCAN_NT) void mgf_lines_kernel(const uint8_t *__restrict__ t,
                                                          const uint32_t *__restrict__ line_start, int64_t n_lines,
                                                          int last, uint8_t *__restrict__ kind,
                                                          uint8_t *__restrict__ dflag, uint64_t *__restrict__ val,
                                                          TextFinal *__restrict__ fin) {
  const int64_t L = (int64_t)blockIdx.x * SCAN_NT + threadIdx.x;
  if (L >= n_lines) return;
  const uint32_t a = line_start[L], b = line_start[L + 1];
  if (!text_walks_line(t, a, b, L, n_lines, last, fin)) {
    kind[L] = MK_SKIP, dflag[L] = 0, val[L] = 0;
    return;
  }
  uint32_t p, q;
  mg_strip(t, a, b, &p, &q);
  uint8_t k = MK_SKIP, df = 0;
  uint64_t v = 0;
  const uint8_t c = p < q ? t[p] : (uint8_t)'#';
  if (c == '#' || c == ';' || c == '!' || c == '/') {
    k = MK_SKIP;
  } else if (mg_is(t, p, q - p, "BEGIN IONS", 10, false)) {
    k = MK_BEGIN;
  } else if (mg_is(t, p, q - p, "END IONS", 8, false)) {
    k = MK_END;
  } else {
    const uint32_t eq = mg_find(t, p, q, (uint8_t)'=');
    if (eq < q) {
      const uint32_t kl = eq - p;
      k = mg_is(t, p, kl, "title", 5, true) ? MK_TITLE
          : mg_is(t, p, kl, "scan", 4, true) ? MK_SCAN
          : mg_is(t, p, kl, "pepmass", 7, true) ? MK_PEPMASS
          : mg_is(t, p, kl, "charge", 6, true) ? MK_CHARGE
          : mg_is(t, p, kl, "rtinseconds", 11, true) ? MK_RT : MK_OTHER;
      if (k == MK_PEPMASS || k == MK_RT) {
        uint32_t ta, tb;
        mg_param_token(t, p, q, k, &ta, &tb);
        double d = 0.0;
        df = (uint8_t)mgf_number(reinterpret_cast<const char *>(t) + ta, (int)(tb - ta), &d);
        v = (uint64_t)__double_as_longlong(d);
      } else if (k == MK_CHARGE) {
        v = (uint64_t)(int64_t)mg_charge(t, mg_skip_ws(t, eq + 1u, q), q);
      }
    } else {
      const MgPeakTokens tk = mg_peak_tokens(t, p, q);
      if (tk.t1a == q) {
        k = MK_PEAK1;
      } else {
        k = MK_PEAK;
        double d0 = 0.0, d1 = 0.0;
        df = (uint8_t)(mgf_number(reinterpret_cast<const char *>(t) + tk.t0a, (int)(tk.t0b - tk.t0a), &d0) |
                       (mgf_number(reinterpret_cast<const char *>(t) + tk.t1a, (int)(tk.t1b - tk.t1a), &d1) << 1));
        v = pack_peak(d0, d1);
      }
    }
  }
  kind[L] = k, dflag[L] = df, val[L] = v;
}

struct StateView {   // after[L]: is line L + 1 inside a block?
  using Op = MgState;
  const uint8_t *kind;
  uint8_t *after;
  __device__ uint32_t load(int64_t L) const {
    const uint8_t k = kind[L];
    return k == MK_BEGIN ? 3u : k == MK_END ? 0u : 2u;
  }
  __device__ void store(int64_t L, uint32_t incl, uint32_t) const { after[L] = (uint8_t)(incl & 1u); }   // from outside
};

struct CountView {   // spec[L]: blocks opened up to and including L; slot / dslot: peaks / deferred tokens before L
  using Op = MgCount;
  const uint8_t *kind, *dflag, *after;
  const uint32_t *line_start;
  uint32_t *spec, *slot, *dslot;
  MgTotals *totals;
  int64_t n_lines;
  __device__ MgTotals load(int64_t L) const {
    const bool in = L > 0 && after[L - 1] != 0;
    const uint8_t k = kind[L];
    MgTotals v = {0u, 0u, 0u, 0u, 0u, 0u};
    if (!in) {
      v.opens = k == MK_BEGIN ? 1u : 0u;
      return v;
    }
    if (k == MK_END) v.closes = 1u, v.cons_byte = line_start[L + 1], v.cons_line = (uint32_t)(L + 1);
    if (k == MK_PEAK) v.peaks = 1u;
    if (k == MK_PEAK || k == MK_PEPMASS || k == MK_RT) v.defers = (uint32_t)__popc((uint32_t)dflag[L]);
    return v;
  }
  __device__ void store(int64_t L, MgTotals incl, MgTotals own) const {
    spec[L] = incl.opens, slot[L] = incl.peaks - own.peaks, dslot[L] = incl.defers - own.defers;
    if (L == n_lines - 1) *totals = incl;
  }
};

// gate: lines behind it belong to a block this chunk does not close (they come again with the next chunk)
__global__ __launch_bounds__(SCAN_NT) void mgf_resolve_kernel(const uint8_t *__restrict__ kind,
                                                            const uint8_t *__restrict__ after,
                                                            const uint32_t *__restrict__ spec,
                                                            const uint32_t *__restrict__ slot,
                                                            const uint32_t *__restrict__ dslot, int64_t n_lines,
                                                            int64_t gate, uint32_t n_open, uint32_t n_closed,
                                                            uint32_t *__restrict__ first_line,
                                                            uint32_t *__restrict__ peak_begin,
                                                            uint32_t *__restrict__ peak_end,
                                                            uint32_t *__restrict__ key_line,
                                                            TextFinal *__restrict__ fin) {
  const int64_t L = (int64_t)blockIdx.x * SCAN_NT + threadIdx.x;
  if (L >= n_lines) return;
  const bool in = L > 0 && after[L - 1] != 0;
  const uint8_t k = kind[L];
  const uint32_t s = spec[L] - 1u;   // (in a block, or opening one: spec[L] >= 1)
  if (!in) {
    if (k == MK_BEGIN && s < n_open) first_line[s] = (uint32_t)L, peak_begin[s] = slot[L];
    return;
  }
  if (s >= n_open) return;           // (cannot happen: kept as the bound of every per-spectrum store)
  if ((k == MK_BEGIN || k == MK_PEAK1) && L < gate)
    atomicMin(&fin->err, ((unsigned long long)L << 8) | (k == MK_BEGIN ? ASL_MGF_ERR_NESTED : ASL_MGF_ERR_ONE_TOKEN));
  if (k == MK_END) {
    peak_end[s] = slot[L];
    if (s + 1u == n_closed) fin->n_peaks = slot[L], fin->n_def = dslot[L];
  }
  if (k >= MK_TITLE && k <= MK_RT) atomicMax(&key_line[(size_t)s * MG_KEYS + (k - MK_TITLE)], (uint32_t)(L + 1));
}

// ---------------------------------------------------------------------------------------------- fill
// rec: [n_def, 5], the records of put_deferred
__global__ __launch_bounds__(SCAN_NT) void mgf_fill_lines_kernel(
    const uint8_t *__restrict__ t, const uint32_t *__restrict__ line_start, const uint8_t *__restrict__ kind,
    const uint8_t *__restrict__ dflag, const uint64_t *__restrict__ val, const uint8_t *__restrict__ after,
    const uint32_t *__restrict__ spec, const uint32_t *__restrict__ slot, const uint32_t *__restrict__ dslot,
    int64_t n_lines, uint32_t n_blocks, uint32_t n_peaks, uint32_t n_def, float *__restrict__ mz,
    float *__restrict__ intensity, uint8_t *__restrict__ charge, int32_t *__restrict__ rec) {
  const int64_t L = (int64_t)blockIdx.x * SCAN_NT + threadIdx.x;
  if (L >= n_lines) return;
  if (!(L > 0 && after[L - 1] != 0) || spec[L] - 1u >= n_blocks) return;   // (an open block's slots lie behind n_peaks)
  const uint8_t k = kind[L], df = dflag[L];
  if (k == MK_PEAK) {
    const uint32_t o = slot[L];
    if (o < n_peaks) {
      put_peak(mz, intensity, o, val[L]);
      if (charge != nullptr) charge[o] = 0;
    }
  }
  if (df == 0 || !(k == MK_PEAK || k == MK_PEPMASS || k == MK_RT)) return;
  uint32_t p, q, r = dslot[L];
  mg_strip(t, line_start[L], line_start[L + 1], &p, &q);
  if (k == MK_PEAK) {
    const MgPeakTokens tk = mg_peak_tokens(t, p, q);
    if ((df & 1) && r < n_def) put_deferred(rec, r++, tk.t0a, tk.t0b, ASL_MGF_DEST_MZ, slot[L], L);
    if ((df & 2) && r < n_def) put_deferred(rec, r, tk.t1a, tk.t1b, ASL_MGF_DEST_INTENSITY, slot[L], L);
  } else if (r < n_def) {   // (the spectrum kernel names the destination of the line that wins)
    uint32_t ta, tb;
    mg_param_token(t, p, q, k, &ta, &tb);
    put_deferred(rec, r, ta, tb, ASL_MGF_DEST_NONE, spec[L] - 1u, L);
  }
}

__global__ __launch_bounds__(SCAN_NT) void mgf_fill_spectra_kernel(
    const uint8_t *__restrict__ t, const uint32_t *__restrict__ line_start, const uint8_t *__restrict__ dflag,
    const uint64_t *__restrict__ val, const uint32_t *__restrict__ dslot, const uint32_t *__restrict__ first_line,
    const uint32_t *__restrict__ peak_begin, const uint32_t *__restrict__ key_line, uint32_t n_closed,
    uint32_t n_peaks, uint32_t n_def, int32_t *__restrict__ offsets, double *__restrict__ pmz,
    int32_t *__restrict__ pcharge, double *__restrict__ rt, int32_t *__restrict__ ident,
    int32_t *__restrict__ first, int32_t *__restrict__ rec) {
  const uint32_t s = blockIdx.x * SCAN_NT + threadIdx.x;
  if (s >= n_closed) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  offsets[s] = (int32_t)peak_begin[s];
  if (s + 1u == n_closed) offsets[n_closed] = (int32_t)n_peaks;
  first[s] = (int32_t)first_line[s];
  const uint32_t *kl = key_line + (size_t)s * MG_KEYS;
  double *const dst[2] = {pmz, rt};
  const int which[2] = {MK_PEPMASS - MK_TITLE, MK_RT - MK_TITLE};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const uint32_t l = kl[which[j]];
    double v = nan;
    if (l != 0u) {
      if (dflag[l - 1u] == 0) {
        v = __longlong_as_double((long long)val[l - 1u]);
      } else if (dslot[l - 1u] < n_def) {
        rec[(size_t)dslot[l - 1u] * 5 + 2] = j == 0 ? ASL_MGF_DEST_PEPMASS : ASL_MGF_DEST_RT;
      }
    }
    dst[j][s] = v;
  }
  const uint32_t lc = kl[MK_CHARGE - MK_TITLE];
  pcharge[s] = lc != 0u ? (int32_t)(int64_t)val[lc - 1u] : 0;
  const uint32_t li = kl[0] != 0u ? kl[0] : kl[MK_SCAN - MK_TITLE];
  int32_t io = 0, il = -1;
  if (li != 0u) {
    uint32_t p, q;
    mg_strip(t, line_start[li - 1u], line_start[li], &p, &q);
    const uint32_t v = mg_skip_ws(t, mg_find(t, p, q, (uint8_t)'=') + 1u, q);
    io = (int32_t)(v < q ? v : q), il = (int32_t)(q - (uint32_t)io);
  }
  ident[2 * (size_t)s] = io, ident[2 * (size_t)s + 1] = il;
}

namespace {

// n_rec: the closed blocks; n_blocks: they, and at the file's end the open one too
struct MgfWork : ChunkWork<MgTotals> {
  DevBuf<uint32_t> key_line;
};
MgfWork &work() {
  static MgfWork w;
  return w;
}

}  // namespace
}  // namespace asl

using namespace asl;

extern "C" int asl_mgf_number(const char *s, int32_t n, double *out) {
  if (s == nullptr || n < 0 || out == nullptr) return 1;
  return mgf_number(s, (int)n, out);
}

extern "C" int asl_mgf_measure(const uint8_t *text, int64_t n, int32_t last, int64_t *counts) {
  clear_error();
  MgfWork &W = work();
  ASL_TRY(measure_begin("mgf", W, text, n, last, counts));
  if (n == 0) return ASL_OK;
  ProfScope ps("mgf_measure");
  int64_t nl = 0;   // >= 1
  ASL_TRY(line_starts(text, n, W.count, W.partial, W.line_start, &nl));
  // lines, block state, counts
  ASL_TRY(measure_lines(W, nl));
  hipLaunchKernelGGL(mgf_lines_kernel, dim3(blocks_of(nl)), dim3(SCAN_NT), 0, stream(), text, W.line_start.p, nl,
                     (int)last, W.kind.p, W.dflag.p, W.val.p, W.fin.p);
  ASL_CHECK_LAUNCH();
  ASL_TRY(scan_view(StateView{W.kind.p, W.after.p}, nl, W.partial.p));
  ASL_TRY(scan_view(CountView{W.kind.p, W.dflag.p, W.after.p, W.line_start.p, W.rec.p, W.slot.p, W.dslot.p,
                              W.totals.p, nl},
                    nl, W.partial.p));
  MgTotals T;
  HIP_TRY(hipMemcpyAsync(&T, W.totals.p, sizeof(T), hipMemcpyDeviceToHost, stream()));
  ASL_TRY(sync_stream());
  // per block: extent, winning parameter lines, the first structural error, the capacity
  const uint32_t n_open = T.opens, n_closed = T.closes;
  const size_t ns = std::max<size_t>(n_open, 1);
  ASL_TRY(W.first_line.reserve(ns));
  ASL_TRY(W.peak_begin.reserve(ns));
  ASL_TRY(W.peak_end.reserve(ns));
  ASL_TRY(W.key_line.reserve(ns * MG_KEYS));
  HIP_TRY(hipMemsetAsync(W.key_line.p, 0, ns * MG_KEYS * sizeof(uint32_t), stream()));
  const int64_t gate = last != 0 ? nl : (int64_t)T.cons_line;
  hipLaunchKernelGGL(mgf_resolve_kernel, dim3(blocks_of(nl)), dim3(SCAN_NT), 0, stream(), W.kind.p, W.after.p,
                     W.rec.p, W.slot.p, W.dslot.p, nl, gate, n_open, n_closed, W.first_line.p, W.peak_begin.p,
                     W.peak_end.p, W.key_line.p, W.fin.p);
  ASL_CHECK_LAUNCH();
  if (n_closed > 0) {
    hipLaunchKernelGGL(text_capacity_kernel, dim3(blocks_of(n_closed)), dim3(SCAN_NT), 0, stream(), W.peak_begin.p,
                       W.peak_end.p, n_closed, 0, 0u, W.fin.p);
    ASL_CHECK_LAUNCH();
  }
  TextFinal F;
  ASL_TRY(measure_final("mgf", W, &F));
  counts[ASL_MGF_N_LINES] = nl;
  counts[ASL_MGF_N_SPECTRA] = n_closed;
  counts[ASL_MGF_N_PEAKS] = F.n_peaks;
  // at the file's end the numerals of an unclosed last block are reported too, so that the caller can refuse them
  counts[ASL_MGF_N_DEFERRED] = last != 0 ? T.defers : F.n_def;
  counts[ASL_MGF_CONSUMED] = T.cons_byte;
  counts[ASL_MGF_CONSUMED_LINES] = T.cons_line;
  counts[ASL_MGF_OPEN] = n_open > n_closed ? 1 : 0;
  W.n_blocks = last != 0 ? n_open : n_closed;
  return measure_end("mgf", "spectrum", W, F, text, n, counts);
}

extern "C" int asl_mgf_fill(const uint8_t *text, int64_t n, int32_t *offsets, float *mz, float *intensity,
                            uint8_t *charge, double *precursor_mz, int32_t *precursor_charge,
                            double *retention_time, int32_t *identifier, int32_t *first_line, int32_t *deferred) {
  clear_error();
  MgfWork &W = work();
  ASL_TRY(fill_begin("mgf", W, text, n, offsets));
  const uint32_t ns = W.n_rec, np = W.n_peaks, nd = W.n_def;
  if (ns == 0 && nd == 0) return fill_empty(offsets);
  if ((np > 0 && (!mz || !intensity)) ||
      (ns > 0 && (!precursor_mz || !precursor_charge || !retention_time || !identifier || !first_line)) ||
      (nd > 0 && !deferred))
    return fail(ASL_ERR_INVALID, "mgf_fill: a null output");
  ASL_TRY(ensure_device());
  ProfScope ps("mgf_fill");
  Out<int32_t> oOff, oZ, oId, oFirst, oRec;
  Out<float> oMz, oIt;
  Out<uint8_t> oChg;
  Out<double> oPmz, oRt;
  ASL_TRY(oOff.init(offsets, (size_t)ns + 1));
  ASL_TRY(oMz.init(mz, np));
  ASL_TRY(oIt.init(intensity, np));
  ASL_TRY(oChg.init(charge, np));
  ASL_TRY(oPmz.init(precursor_mz, ns));
  ASL_TRY(oZ.init(precursor_charge, ns));
  ASL_TRY(oRt.init(retention_time, ns));
  ASL_TRY(oId.init(identifier, (size_t)ns * 2));
  ASL_TRY(oFirst.init(first_line, ns));
  ASL_TRY(oRec.init(deferred, (size_t)nd * 5));
  hipLaunchKernelGGL(mgf_fill_lines_kernel, dim3(blocks_of(W.n_lines)), dim3(SCAN_NT), 0, stream(), text,
                     W.line_start.p, W.kind.p, W.dflag.p, W.val.p, W.after.p, W.rec.p, W.slot.p, W.dslot.p,
                     W.n_lines, W.n_blocks, np, nd, oMz.d, oIt.d, oChg.d, oRec.d);
  ASL_CHECK_LAUNCH();
  if (ns > 0) {   // (none: the deferred tokens of an unclosed last block alone)
    hipLaunchKernelGGL(mgf_fill_spectra_kernel, dim3(blocks_of(ns)), dim3(SCAN_NT), 0, stream(), text, W.line_start.p,
                       W.dflag.p, W.val.p, W.dslot.p, W.first_line.p, W.peak_begin.p, W.key_line.p, ns, np, nd, oOff.d,
                       oPmz.d, oZ.d, oRt.d, oId.d, oFirst.d, oRec.d);
    ASL_CHECK_LAUNCH();
  } else if (oOff.d != nullptr) {
    HIP_TRY(hipMemsetAsync(oOff.d, 0, sizeof(int32_t), stream()));
  }
  return finish_outputs(oOff, oMz, oIt, oChg, oPmz, oZ, oRt, oId, oFirst, oRec);
}
