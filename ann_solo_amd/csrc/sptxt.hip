// sptxt.hip -- SpectraST .sptxt libraries parsed on the device (asl_sptxt_measure / asl_sptxt_fill) and the
// annotation rule on the host (asl_sptxt_fragment_charge). gfx950 only. DESIGN.md 3 "Library files"; the dialect is
// stated in include/annsolo_mi.h and restated in tests/sptxt_ref.py. Shared with mgf.hip: the scans and the line
// starts (text_scan.hpp); the counts operator, the walk guard, the peak and deferred-token stores, the capacity check
// and the grammar-free host parts of measure and fill (text_records.hpp).
//
//   starts    the line starts of the chunk (text_scan.hpp)
//   classify  one thread per line looks at the head of the stripped line: Name:, Num Peaks:, PrecursorMZ:, other
//   state     a scan that composes the lines' maps of the three states {outside a record, in its metadata, in its
//             peaks}: Name: -> metadata, Num Peaks: in the metadata -> peaks, anything else keeps the state
//   parse     one thread per line, now knowing its state, walks it: a second Name:, and in the metadata `decoy`, the
//             first Parent= and Mods=, the precursor numeral and a PrecursorMZ: or Num Peaks: key inside the line; in the peaks the '#' cut, the three tab-separated
//             fields, the two numerals (mgf_number.hpp; what it defers is flagged, never guessed) and the
//             annotation's fragment charge (sptxt_annot.hpp)
//   counts    a scan of (records opened, peak lines, deferred tokens, byte and line of the last Name: line): record
//             ordinal, peak slot and deferred slot of every line
//   resolve   per line: the first structural error (integer atomicMin of line << 8 | kind); per record the first
//             PrecursorMZ:, Parent= and Mods= line (integer atomicMin of the line number) and the OR of the decoy flags
//   fill      peaks scattered to their slots with their charge bytes, the deferred tokens' byte ranges and
//             destinations, the per-record columns (one thread per record reads its Name: line and the lines that won)
//
// A record is closed by the next Name: line, or by the end of the file when `last` is set. The sort of descending
// spectra is asl_mgf_sort_charged (peak_sort.hip). Integer atomics only, and none whose arrival order reaches the
// output. Every byte index is bounded by the chunk length and every line by line_start[n_lines] == n.
#include <algorithm>

#include "common.hpp"
#include "mgf_number.hpp"
#include "sptxt_annot.hpp"
#include "text_records.hpp"

namespace asl {
namespace {

enum : uint8_t { SK_SKIP = 0, SK_NAME, SK_NUMPEAKS, SK_PMZ, SK_OTHER };   // the head of a line, whatever surrounds it
enum : uint8_t {                                                          // what the parse found in a line
  SF_NAME2 = 1, SF_DECOY = 2, SF_PARENT = 4, SF_MODS = 8, SF_BADNUM = 16, SF_PEAK = 32, SF_FEW = 64, SF_BADNP = 128
};   // SF_BADNP: a Num Peaks line of another shape; on a metadata line, a Num Peaks: or PrecursorMZ: key inside it
enum : uint32_t { SS_OUT = 0, SS_META = 1, SS_PEAKS = 2 };

struct SpTotals {   // the counts scan's result over all lines
  uint32_t opens, peaks, defers, cons_byte, cons_line;
};
using SpCount = TextCount<SpTotals, &SpTotals::opens, &SpTotals::peaks, &SpTotals::defers>;

// A line as a map of the record state: bits 2 x, 2 x + 1 of the value hold the state after the line when the state
// before it is x.
struct SpState {
  using T = uint32_t;
  __device__ static T identity() { return 0u | (1u << 2) | (2u << 4); }
  __device__ static T op(T a, T b) {
    T r = 0u;
#pragma unroll
    for (int s = 0; s < 3; ++s) r |= ((b >> (2u * ((a >> (2 * s)) & 3u))) & 3u) << (2 * s);
    return r;
  }
};

// ---------------------------------------------------------------------------------------------- bytes
__device__ __forceinline__ uint8_t sp_lower(uint8_t c) { return c >= 'A' && c <= 'Z' ? (uint8_t)(c + 32) : c; }
__device__ __forceinline__ bool sp_letter(uint8_t c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }
__device__ __forceinline__ bool sp_digit(uint8_t c) { return c >= '0' && c <= '9'; }
// does the lower-case literal stand at t[i .. ), inside [i, q), in any letter case?
__device__ __forceinline__ bool sp_at(const uint8_t *__restrict__ t, uint32_t i, uint32_t q, const char *lit,
                                      uint32_t len) {
  if (q - i < len) return false;
  for (uint32_t k = 0; k < len; ++k)
    if (sp_lower(t[i + k]) != (uint8_t)lit[k]) return false;
  return true;
}
// the first occurrence of the literal in [p, q), else q
__device__ __forceinline__ uint32_t sp_find(const uint8_t *__restrict__ t, uint32_t p, uint32_t q, const char *lit,
                                            uint32_t len) {
  for (uint32_t i = p; i + len <= q; ++i)
    if (sp_at(t, i, q, lit, len)) return i;
  return q;
}
// length of the Num Peaks: key at the head of [p, q), 0: none
__device__ __forceinline__ uint32_t sp_numpeaks_key(const uint8_t *__restrict__ t, uint32_t p, uint32_t q) {
  if (sp_at(t, p, q, "numpeaks:", 9)) return 9u;
  if (sp_at(t, p, q, "num", 3) && q - p >= 10u && mg_ws(t[p + 3]) && sp_at(t, p + 4, q, "peaks:", 6)) return 10u;
  return 0u;
}
// The precursor numeral behind a key that ends at v: at most one blank, then the run of digits and points [*ta, *tb).
// Returns whether the run is digits [. digits]; strict: nothing but the numeral may stand before q.
__device__ __forceinline__ bool sp_precursor_token(const uint8_t *__restrict__ t, uint32_t v, uint32_t q, bool strict,
                                                   uint32_t *ta, uint32_t *tb) {
  if (v < q && mg_ws(t[v])) ++v;
  uint32_t e = v;
  while (e < q && (sp_digit(t[e]) || t[e] == '.')) ++e;
  *ta = v, *tb = e;
  uint32_t i = v;
  while (i < e && sp_digit(t[i])) ++i;
  bool ok = i > v;
  if (i < e) {   // a point: digits behind it, up to the run's end
    uint32_t j = i + 1;
    while (j < e && sp_digit(t[j])) ++j;
    ok = ok && j > i + 1 && j == e;
  }
  return ok && (!strict || e == q);
}
// [*e): the peak line [a, b) cut at the first '#', else without its line end; returns whether anything but blanks
// is left
__device__ __forceinline__ bool sp_peak_extent(const uint8_t *__restrict__ t, uint32_t a, uint32_t b, uint32_t *e) {
  uint32_t h = a;
  while (h < b && t[h] != '#') ++h;
  if (h == b)
    while (h > a && (t[h - 1] == '\n' || t[h - 1] == '\r')) --h;
  *e = h;
  for (uint32_t i = a; i < h; ++i)
    if (!mg_ws(t[i])) return true;
  return false;
}
struct SpFields {   // the first three tab-separated fields of [a, e); n: how many there are (at most 3 counted)
  uint32_t f0a, f0b, f1a, f1b, f2a, f2b;
  int n;
};
__device__ __forceinline__ SpFields sp_fields(const uint8_t *__restrict__ t, uint32_t a, uint32_t e) {
  SpFields f = {a, e, e, e, e, e, 1};
  uint32_t i = a;
  while (i < e && t[i] != '\t') ++i;
  f.f0b = i;
  if (i == e) return f;
  f.n = 2, f.f1a = ++i;
  while (i < e && t[i] != '\t') ++i;
  f.f1b = i;
  if (i == e) return f;
  f.n = 3, f.f2a = ++i;
  while (i < e && t[i] != '\t') ++i;
  f.f2b = i;
  return f;
}

// ---------------------------------------------------------------------------------------------- lines
__global__ __launch_bounds__(SCAN_NT) void sptxt_classify_kernel(const uint8_t *__restrict__ t,
                                                               const uint32_t *__restrict__ line_start,
                                                               int64_t n_lines, int last, uint8_t *__restrict__ kind,
                                                               TextFinal *__restrict__ fin) {
  const int64_t L = (int64_t)blockIdx.x * SCAN_NT + threadIdx.x;
  if (L >= n_lines) return;
  const uint32_t a = line_start[L], b = line_start[L + 1];
  if (!text_walks_line(t, a, b, L, n_lines, last, fin)) {
    kind[L] = SK_SKIP;
    return;
  }
  uint32_t p, q;
  mg_strip(t, a, b, &p, &q);
  kind[L] = sp_at(t, p, q, "name:", 5) ? SK_NAME
            : sp_numpeaks_key(t, p, q) != 0u ? SK_NUMPEAKS
            : sp_at(t, p, q, "precursormz:", 12) ? SK_PMZ : SK_OTHER;
}

struct SpStateView {   // after[L]: the state line L + 1 finds
  using Op = SpState;
  const uint8_t *kind;
  uint8_t *after;
  __device__ uint32_t load(int64_t L) const {
    const uint8_t k = kind[L];
    return k == SK_NAME ? (1u | (1u << 2) | (1u << 4)) : k == SK_NUMPEAKS ? (0u | (2u << 2) | (2u << 4))
                                                                          : SpState::identity();
  }
  __device__ void store(int64_t L, uint32_t incl, uint32_t) const { after[L] = (uint8_t)(incl & 3u); }   // from outside
};

// flags, dflag (bit k: numeral k of the line was deferred), val (a peak's two float32, or the precursor's double)
// and chg (a peak's fragment charge) of every line
__global__ __launch_bounds__(SCAN_NT) void sptxt_parse_kernel(const uint8_t *__restrict__ t,
                                                            const uint32_t *__restrict__ line_start, int64_t n_lines,
                                                            const uint8_t *__restrict__ kind,
                                                            const uint8_t *__restrict__ after,
                                                            uint8_t *__restrict__ flags, uint8_t *__restrict__ dflag,
                                                            uint8_t *__restrict__ chg, uint64_t *__restrict__ val) {
  const int64_t L = (int64_t)blockIdx.x * SCAN_NT + threadIdx.x;
  if (L >= n_lines) return;
  const uint8_t k = kind[L];
  uint8_t fl = 0, df = 0, cz = 0;
  uint64_t v = 0;
  if (k != SK_SKIP) {
    const uint32_t sb = L > 0 ? after[L - 1] : SS_OUT;
    const uint32_t a = line_start[L], b = line_start[L + 1];
    uint32_t p, q;
    mg_strip(t, a, b, &p, &q);
    const bool meta = k == SK_NAME || (sb == SS_META && k == SK_OTHER);
    for (uint32_t i = p; i < q; ++i) {
      const uint8_t c = sp_lower(t[i]);
      if (c == 'n') {
        if (i > p && !sp_letter(t[i - 1]) && sp_at(t, i, q, "name:", 5)) fl |= SF_NAME2;
        if (meta && i > p && sp_numpeaks_key(t, i, q) != 0u) fl |= SF_BADNP;   // (a key the reference would find)
      } else if (!meta) {
        continue;
      } else if (c == 'd') {
        if (sp_at(t, i, q, "decoy", 5)) fl |= SF_DECOY;
      } else if (c == 'm') {
        if (sp_at(t, i, q, "mods=", 5)) fl |= SF_MODS;
      } else if (c == 'p' && i > p && sp_at(t, i, q, "precursormz:", 12)) {
        fl |= SF_BADNP;
      } else if (c == 'p' && !(fl & SF_PARENT) && sp_at(t, i, q, "parent=", 7)) {
        fl |= SF_PARENT;
        uint32_t ta, tb;
        if (!sp_precursor_token(t, i + 7u, q, false, &ta, &tb)) {
          fl |= SF_BADNUM;
        } else {
          double d = 0.0;
          df = (uint8_t)mgf_number(reinterpret_cast<const char *>(t) + ta, (int)(tb - ta), &d);
          v = (uint64_t)__double_as_longlong(d);
        }
      }
    }
    if (k == SK_PMZ && sb == SS_META) {
      uint32_t ta, tb;
      if (!sp_precursor_token(t, p + 12u, q, true, &ta, &tb)) {
        fl |= SF_BADNUM;
      } else {
        double d = 0.0;
        df = (uint8_t)mgf_number(reinterpret_cast<const char *>(t) + ta, (int)(tb - ta), &d);
        v = (uint64_t)__double_as_longlong(d);
      }
    } else if (k == SK_NUMPEAKS && sb != SS_OUT) {
      uint32_t i = p + sp_numpeaks_key(t, p, q);
      if (i < q && mg_ws(t[i])) ++i;
      const uint32_t d0 = i;
      while (i < q && sp_digit(t[i])) ++i;
      if (i == d0 || i != q) fl |= SF_BADNP;
    } else if (sb == SS_PEAKS && (k == SK_OTHER || k == SK_PMZ)) {
      uint32_t e;
      if (sp_peak_extent(t, a, b, &e)) {
        const SpFields f = sp_fields(t, a, e);
        if (f.n < 3) {
          fl |= SF_FEW;
        } else {
          fl |= SF_PEAK;
          uint32_t m0, m1, i0, i1;
          mg_strip(t, f.f0a, f.f0b, &m0, &m1);
          mg_strip(t, f.f1a, f.f1b, &i0, &i1);
          double d0 = 0.0, d1 = 0.0;
          df = (uint8_t)(mgf_number(reinterpret_cast<const char *>(t) + m0, (int)(m1 - m0), &d0) |
                         (mgf_number(reinterpret_cast<const char *>(t) + i0, (int)(i1 - i0), &d1) << 1));
          v = pack_peak(d0, d1);
          cz = (uint8_t)sptxt_fragment_charge(reinterpret_cast<const char *>(t) + f.f2a, (int)(f.f2b - f.f2a));
        }
      }
    }
  }
  flags[L] = fl, dflag[L] = df, chg[L] = cz, val[L] = v;
}

struct SpCountView {   // rec[L]: Name: lines up to and including L; slot / dslot: peaks / deferred tokens before L
  using Op = SpCount;
  const uint8_t *kind, *flags, *dflag;
  const uint32_t *line_start;
  uint32_t *rec, *slot, *dslot;
  SpTotals *totals;
  int64_t n_lines;
  __device__ SpTotals load(int64_t L) const {
    SpTotals v = {0u, 0u, 0u, 0u, 0u};
    if (kind[L] == SK_NAME) v.opens = 1u, v.cons_byte = line_start[L], v.cons_line = (uint32_t)L;
    if (flags[L] & SF_PEAK) v.peaks = 1u;
    v.defers = (uint32_t)__popc((uint32_t)dflag[L]);
    return v;
  }
  __device__ void store(int64_t L, SpTotals incl, SpTotals own) const {
    rec[L] = incl.opens, slot[L] = incl.peaks - own.peaks, dslot[L] = incl.defers - own.defers;
    if (L == n_lines - 1) *totals = incl;
  }
};

// gate: lines from it on belong to a record this chunk does not close (they come again with the next chunk)
__global__ __launch_bounds__(SCAN_NT) void sptxt_resolve_kernel(
    const uint8_t *__restrict__ kind, const uint8_t *__restrict__ flags, const uint8_t *__restrict__ after,
    const uint32_t *__restrict__ rec, const uint32_t *__restrict__ slot, const uint32_t *__restrict__ dslot,
    int64_t n_lines, int64_t gate, uint32_t n_open, uint32_t n_rec, uint32_t *__restrict__ first_line,
    uint32_t *__restrict__ peak_begin, uint32_t *__restrict__ peak_end, uint32_t *__restrict__ pmz_line,
    uint32_t *__restrict__ parent_line, uint32_t *__restrict__ mods_line, uint32_t *__restrict__ decoy,
    TextFinal *__restrict__ fin) {
  const int64_t L = (int64_t)blockIdx.x * SCAN_NT + threadIdx.x;
  if (L >= n_lines) return;
  const uint8_t k = kind[L], fl = flags[L];
  const uint32_t sb = L > 0 ? after[L - 1] : SS_OUT;
  if (L < gate) {
    const uint32_t e = (fl & SF_NAME2)                       ? ASL_SPTXT_ERR_SECOND_NAME
                       : (k == SK_NUMPEAKS && sb == SS_PEAKS) ? ASL_SPTXT_ERR_SECOND_NUMPEAKS
                       : (fl & SF_BADNP) ? (k == SK_NUMPEAKS ? ASL_SPTXT_ERR_NUMPEAKS : ASL_SPTXT_ERR_STRAY_KEY)
                       : (fl & SF_FEW)                        ? ASL_SPTXT_ERR_FEW_FIELDS
                       : (k == SK_PMZ && (fl & SF_BADNUM))    ? ASL_SPTXT_ERR_PRECURSOR
                                                              : 0u;
    if (e != 0u) atomicMin(&fin->err, ((unsigned long long)L << 8) | e);
  }
  if (rec[L] == 0u) return;          // before the first record
  const uint32_t s = rec[L] - 1u;
  if (s >= n_open) return;           // (cannot happen: kept as the bound of every per-record store)
  if (k == SK_NAME) {
    first_line[s] = (uint32_t)L, peak_begin[s] = slot[L];
    if (s > 0u) peak_end[s - 1u] = slot[L];
    if (s == n_rec) fin->n_peaks = slot[L], fin->n_def = dslot[L];
  }
  if (s >= n_rec) return;
  if (fl & SF_DECOY) atomicOr(&decoy[s], 1u);
  if (k == SK_PMZ && sb == SS_META) atomicMin(&pmz_line[s], (uint32_t)L);
  if (fl & SF_PARENT) atomicMin(&parent_line[s], (uint32_t)L);
  if (fl & SF_MODS) atomicMin(&mods_line[s], (uint32_t)L);
}

// ---------------------------------------------------------------------------------------------- fill
// out: [n_def, 5], the records of put_deferred
__global__ __launch_bounds__(SCAN_NT) void sptxt_fill_lines_kernel(
    const uint8_t *__restrict__ t, const uint32_t *__restrict__ line_start, const uint8_t *__restrict__ kind,
    const uint8_t *__restrict__ flags, const uint8_t *__restrict__ dflag, const uint8_t *__restrict__ chg,
    const uint64_t *__restrict__ val, const uint32_t *__restrict__ rec, const uint32_t *__restrict__ slot,
    const uint32_t *__restrict__ dslot, int64_t n_lines, uint32_t n_blocks, uint32_t n_peaks, uint32_t n_def,
    float *__restrict__ mz, float *__restrict__ intensity, uint8_t *__restrict__ charge, int32_t *__restrict__ out) {
  const int64_t L = (int64_t)blockIdx.x * SCAN_NT + threadIdx.x;
  if (L >= n_lines) return;
  if (rec[L] == 0u || rec[L] - 1u >= n_blocks) return;   // (an open record's slots lie behind n_peaks)
  const uint8_t fl = flags[L], df = dflag[L];
  if (fl & SF_PEAK) {
    const uint32_t o = slot[L];
    if (o < n_peaks) {
      put_peak(mz, intensity, o, val[L]);
      charge[o] = chg[L];
    }
  }
  if (df == 0) return;
  uint32_t r = dslot[L];
  const uint32_t a = line_start[L], b = line_start[L + 1];
  if (fl & SF_PEAK) {
    uint32_t e;
    sp_peak_extent(t, a, b, &e);
    const SpFields f = sp_fields(t, a, e);
    uint32_t x0, x1;
    if ((df & 1) && r < n_def) {
      mg_strip(t, f.f0a, f.f0b, &x0, &x1);
      put_deferred(out, r++, x0, x1, ASL_SPTXT_DEST_MZ, slot[L], L);
    }
    if ((df & 2) && r < n_def) {
      mg_strip(t, f.f1a, f.f1b, &x0, &x1);
      put_deferred(out, r, x0, x1, ASL_SPTXT_DEST_INTENSITY, slot[L], L);
    }
  } else if (r < n_def) {   // a precursor numeral: the record kernel names the destination of the line that wins
    uint32_t p, q, ta, tb;
    mg_strip(t, a, b, &p, &q);
    if (kind[L] == SK_PMZ) sp_precursor_token(t, p + 12u, q, true, &ta, &tb);
    else sp_precursor_token(t, sp_find(t, p, q, "parent=", 7) + 7u, q, false, &ta, &tb);
    put_deferred(out, r, ta, tb, ASL_SPTXT_DEST_NONE, rec[L] - 1u, L);
  }
}

// info: [n_rec, ASL_SPTXT_INFO]
__global__ __launch_bounds__(SCAN_NT) void sptxt_fill_records_kernel(
    const uint8_t *__restrict__ t, const uint32_t *__restrict__ line_start, const uint8_t *__restrict__ flags,
    const uint8_t *__restrict__ dflag, const uint64_t *__restrict__ val, const uint32_t *__restrict__ dslot,
    const uint32_t *__restrict__ first_line, const uint32_t *__restrict__ peak_begin,
    const uint32_t *__restrict__ pmz_line, const uint32_t *__restrict__ parent_line,
    const uint32_t *__restrict__ mods_line, const uint32_t *__restrict__ decoy, uint32_t n_rec, uint32_t n_peaks,
    uint32_t n_def, int32_t *__restrict__ offsets, double *__restrict__ pmz, int32_t *__restrict__ info,
    int32_t *__restrict__ out) {
  const uint32_t s = blockIdx.x * SCAN_NT + threadIdx.x;
  if (s >= n_rec) return;
  offsets[s] = (int32_t)peak_begin[s];
  if (s + 1u == n_rec) offsets[n_rec] = (int32_t)n_peaks;
  int32_t *o = info + (size_t)s * ASL_SPTXT_INFO;
  // the precursor: the first PrecursorMZ: line, else the first line with Parent=
  const uint32_t l = pmz_line[s] != ~0u ? pmz_line[s] : parent_line[s];
  double v = __longlong_as_double(0x7ff8000000000000ll);
  int32_t status = ASL_SPTXT_PRECURSOR_OK;
  if (l == ~0u) {
    status = ASL_SPTXT_PRECURSOR_MISSING;
  } else if (flags[l] & SF_BADNUM) {
    status = ASL_SPTXT_PRECURSOR_BAD;
  } else if (dflag[l] == 0) {
    v = __longlong_as_double((long long)val[l]);
  } else if (dslot[l] < n_def) {
    out[(size_t)dslot[l] * 5 + 2] = ASL_SPTXT_DEST_PRECURSOR;
  }
  pmz[s] = v;
  // the Name: line: the peptide behind the last space before the first '/', the charge behind that '/'
  uint32_t p, q;
  mg_strip(t, line_start[first_line[s]], line_start[first_line[s] + 1u], &p, &q);
  uint32_t sl = p;
  while (sl < q && t[sl] != '/') ++sl;
  int32_t z = -1, na = 0, nl = -1;
  if (sl < q) {
    uint32_t pa = sl, pb = sl;
    while (pa > p && t[pa - 1] != ' ') --pa;
    mg_strip(t, pa, pb, &pa, &pb);
    na = (int32_t)pa, nl = (int32_t)(pb - pa);
    uint32_t ca = sl + 1u, cb = ca;
    while (cb < q && t[cb] != '/') ++cb;
    mg_strip(t, ca, cb, &ca, &cb);
    int zv = 0;
    bool ok = cb > ca;
    for (uint32_t i = ca; i < cb; ++i) {
      ok = ok && sp_digit(t[i]);
      if (zv < 100000) zv = zv * 10 + (int)(t[i] - '0');
    }
    if (ok && zv >= 1 && zv <= 255) z = zv;
  }
  // the first Mods=: up to the first blank
  int32_t ma = 0, ml = -1;
  if (mods_line[s] != ~0u) {
    mg_strip(t, line_start[mods_line[s]], line_start[mods_line[s] + 1u], &p, &q);
    const uint32_t m = sp_find(t, p, q, "mods=", 5);
    uint32_t e = m;
    while (e < q && !mg_ws(t[e])) ++e;
    ma = (int32_t)m, ml = (int32_t)(e - m);
  }
  o[0] = z, o[1] = status, o[2] = decoy[s] != 0u ? 1 : 0, o[3] = na, o[4] = nl, o[5] = ma, o[6] = ml;
  o[7] = (int32_t)first_line[s];
}

// n_rec == n_blocks: the closed records
struct SptxtWork : ChunkWork<SpTotals> {
  DevBuf<uint32_t> pmz_line, parent_line, mods_line, decoy;
  DevBuf<uint8_t> flags, chg;
};
SptxtWork &work() {
  static SptxtWork w;
  return w;
}

}  // namespace
}  // namespace asl

using namespace asl;

extern "C" int asl_sptxt_fragment_charge(const char *s, int32_t n) {
  if (s == nullptr || n < 0) return 0;
  return sptxt_fragment_charge(s, (int)n);
}

extern "C" int asl_sptxt_measure(const uint8_t *text, int64_t n, int32_t last, int64_t *counts) {
  clear_error();
  SptxtWork &W = work();
  ASL_TRY(measure_begin("sptxt", W, text, n, last, counts));
  if (n == 0) return ASL_OK;
  ProfScope ps("sptxt_measure");
  int64_t nl = 0;   // >= 1
  {
    ProfScope p1("sptxt_starts");   // (the inner scopes split the stage for scripts/sptxt_cost.py)
    ASL_TRY(line_starts(text, n, W.count, W.partial, W.line_start, &nl));
  }
  // heads, record state, the lines themselves, counts
  ASL_TRY(W.flags.reserve((size_t)nl));
  ASL_TRY(W.chg.reserve((size_t)nl));
  ASL_TRY(measure_lines(W, nl));
  {
    ProfScope p2("sptxt_classify");
    hipLaunchKernelGGL(sptxt_classify_kernel, dim3(blocks_of(nl)), dim3(SCAN_NT), 0, stream(), text, W.line_start.p,
                       nl, (int)last, W.kind.p, W.fin.p);
    ASL_CHECK_LAUNCH();
  }
  {
    ProfScope p3("sptxt_state");
    ASL_TRY(scan_view(SpStateView{W.kind.p, W.after.p}, nl, W.partial.p));
  }
  {
    ProfScope p4("sptxt_parse");
    hipLaunchKernelGGL(sptxt_parse_kernel, dim3(blocks_of(nl)), dim3(SCAN_NT), 0, stream(), text, W.line_start.p, nl,
                       W.kind.p, W.after.p, W.flags.p, W.dflag.p, W.chg.p, W.val.p);
    ASL_CHECK_LAUNCH();
  }
  {
    ProfScope p5("sptxt_counts");
    ASL_TRY(scan_view(SpCountView{W.kind.p, W.flags.p, W.dflag.p, W.line_start.p, W.rec.p, W.slot.p, W.dslot.p,
                                  W.totals.p, nl},
                      nl, W.partial.p));
  }
  SpTotals T;
  HIP_TRY(hipMemcpyAsync(&T, W.totals.p, sizeof(T), hipMemcpyDeviceToHost, stream()));
  ASL_TRY(sync_stream());
  // per record: extent, winning lines, the first structural error, the capacity
  const uint32_t n_open = T.opens;
  const uint32_t n_rec = n_open == 0u ? 0u : (last != 0 ? n_open : n_open - 1u);
  const size_t ns = std::max<size_t>(n_open, 1);
  ASL_TRY(W.first_line.reserve(ns));
  ASL_TRY(W.peak_begin.reserve(ns));
  ASL_TRY(W.peak_end.reserve(ns));
  ASL_TRY(W.pmz_line.reserve(ns));
  ASL_TRY(W.parent_line.reserve(ns));
  ASL_TRY(W.mods_line.reserve(ns));
  ASL_TRY(W.decoy.reserve(ns));
  HIP_TRY(hipMemsetAsync(W.pmz_line.p, 0xff, ns * sizeof(uint32_t), stream()));
  HIP_TRY(hipMemsetAsync(W.parent_line.p, 0xff, ns * sizeof(uint32_t), stream()));
  HIP_TRY(hipMemsetAsync(W.mods_line.p, 0xff, ns * sizeof(uint32_t), stream()));
  HIP_TRY(hipMemsetAsync(W.decoy.p, 0, ns * sizeof(uint32_t), stream()));
  // (without a Name: line the chunk is preamble: all its lines are checked; a cut final line was not looked at)
  const int64_t gate = last != 0 || n_open == 0u ? nl : (int64_t)T.cons_line;
  ProfScope p6("sptxt_resolve");
  hipLaunchKernelGGL(sptxt_resolve_kernel, dim3(blocks_of(nl)), dim3(SCAN_NT), 0, stream(), W.kind.p, W.flags.p,
                     W.after.p, W.rec.p, W.slot.p, W.dslot.p, nl, gate, n_open, n_rec, W.first_line.p, W.peak_begin.p,
                     W.peak_end.p, W.pmz_line.p, W.parent_line.p, W.mods_line.p, W.decoy.p, W.fin.p);
  ASL_CHECK_LAUNCH();
  if (n_rec > 0) {
    hipLaunchKernelGGL(text_capacity_kernel, dim3(blocks_of(n_rec)), dim3(SCAN_NT), 0, stream(), W.peak_begin.p,
                       W.peak_end.p, n_rec, (int)last, T.peaks, W.fin.p);
    ASL_CHECK_LAUNCH();
  }
  TextFinal F;
  ASL_TRY(measure_final("sptxt", W, &F));
  const bool open = last == 0 && n_open > 0u;
  const uint32_t n_peaks = open ? F.n_peaks : T.peaks, n_def = open ? F.n_def : T.defers;
  counts[ASL_SPTXT_N_LINES] = nl;
  counts[ASL_SPTXT_N_RECORDS] = n_rec;
  counts[ASL_SPTXT_N_PEAKS] = n_rec > 0u ? n_peaks : 0;
  counts[ASL_SPTXT_N_DEFERRED] = n_rec > 0u ? n_def : 0;
  counts[ASL_SPTXT_CONSUMED] = last != 0 ? n : (n_open > 0u ? (int64_t)T.cons_byte : 0);
  counts[ASL_SPTXT_CONSUMED_LINES] = gate;
  counts[ASL_SPTXT_OPEN] = open ? 1 : 0;
  W.n_blocks = n_rec;
  return measure_end("sptxt", "record", W, F, text, n, counts);
}

extern "C" int asl_sptxt_fill(const uint8_t *text, int64_t n, int32_t *offsets, float *mz, float *intensity,
                              uint8_t *charge, double *precursor_mz, int32_t *info, int32_t *deferred) {
  clear_error();
  SptxtWork &W = work();
  ASL_TRY(fill_begin("sptxt", W, text, n, offsets));
  const uint32_t ns = W.n_rec, np = W.n_peaks, nd = W.n_def;
  if (ns == 0) return fill_empty(offsets);
  if ((np > 0 && (!mz || !intensity || !charge)) || !precursor_mz || !info || (nd > 0 && !deferred))
    return fail(ASL_ERR_INVALID, "sptxt_fill: a null output");
  ASL_TRY(ensure_device());
  ProfScope ps("sptxt_fill");
  Out<int32_t> oOff, oInfo, oRec;
  Out<float> oMz, oIt;
  Out<uint8_t> oChg;
  Out<double> oPmz;
  ASL_TRY(oOff.init(offsets, (size_t)ns + 1));
  ASL_TRY(oMz.init(mz, np));
  ASL_TRY(oIt.init(intensity, np));
  ASL_TRY(oChg.init(charge, np));
  ASL_TRY(oPmz.init(precursor_mz, ns));
  ASL_TRY(oInfo.init(info, (size_t)ns * ASL_SPTXT_INFO));
  ASL_TRY(oRec.init(deferred, (size_t)nd * 5));
  {
    ProfScope p1("sptxt_fill_lines");
    hipLaunchKernelGGL(sptxt_fill_lines_kernel, dim3(blocks_of(W.n_lines)), dim3(SCAN_NT), 0, stream(), text,
                       W.line_start.p, W.kind.p, W.flags.p, W.dflag.p, W.chg.p, W.val.p, W.rec.p, W.slot.p, W.dslot.p,
                       W.n_lines, W.n_blocks, np, nd, oMz.d, oIt.d, oChg.d, oRec.d);
    ASL_CHECK_LAUNCH();
  }
  ProfScope p2("sptxt_fill_records");
  hipLaunchKernelGGL(sptxt_fill_records_kernel, dim3(blocks_of(ns)), dim3(SCAN_NT), 0, stream(), text, W.line_start.p,
                     W.flags.p, W.dflag.p, W.val.p, W.dslot.p, W.first_line.p, W.peak_begin.p, W.pmz_line.p,
                     W.parent_line.p, W.mods_line.p, W.decoy.p, ns, np, nd, oOff.d, oPmz.d, oInfo.d, oRec.d);
  ASL_CHECK_LAUNCH();
  return finish_outputs(oOff, oMz, oIt, oChg, oPmz, oInfo, oRec);
}
