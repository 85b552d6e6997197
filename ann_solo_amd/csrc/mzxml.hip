// mzxml.hip -- mzXML query files parsed and decoded on the device (asl_mzxml_measure / asl_mzxml_fill) and the two
// value rules on the host (asl_mzxml_duration, asl_mzxml_pairs). gfx950 only. DESIGN.md 3 "Query files"; the dialect
// is stated in include/annsolo_mi.h and restated in tests/mzxml_ref.py. Shared with the other readers: the scans and
// the tag starts (text_scan.hpp, with '<' as the byte), the grammar-free host parts of measure and fill
// (text_records.hpp), the tag helpers (xml_tag.hpp, with mzml.hip), the numeral converter (mgf_number.hpp) and the
// base64 step and the inflater (inflate.hpp). The grammar is mzXML's own: scans nest, and the record is a scan's
// HEAD, the tags from its <scan to the next <scan or </scan>.
//
//   starts   count the tag starts, scan the counts, write line_start[] (text_scan.hpp; an entry is the byte of a '<')
//   tags     one thread per tag: find its '>' outside quotes, classify it (scan open / close / self-closed,
//            precursorMz, peaks, comment / CDATA, cut, other), read the attributes it needs (scan: msLevel,
//            peaksCount, retentionTime; precursorMz: precursorCharge and the extent of its text; peaks: precision,
//            byteOrder, contentType / pairOrder, compressionType and the extent of its content) and convert its
//            numeral (mzxml_value.hpp, mgf_number.hpp); what the converter defers is flagged, never guessed. The
//            thread of <peaks> never walks the content: an MS1 profile array costs the start pass alone.
//   context  a scan that composes the tags' maps of the head state -- one assignment {keep, clear, set}: set by a
//            <scan, cleared by </scan> and by a self-closed <scan/> -- with the sums of the <scan tags (the ordinal
//            of the owning scan) and of the elements opened less closed (the nesting depth).
//   resolve  per tag: "the first wins" for <precursorMz> and <peaks> -> integer atomicMin of the tag ordinal per
//            scan, and a count of the <peaks> (a second one is refused); the first structural error -> atomicMin of
//            (tag << 8 | kind); the byte behind the last closed head -> atomicMax. Then per scan: MS level, errors,
//            peak count.
//   slots    a scan over the scans hands out the MS2 ordinals and the peak slots from peaksCount
//   fill     the per-scan columns, then one stream per MS2 scan by one thread over windows in global scratch (the
//            shape profiles/mzml_cost.json measured as the faster one for mzML): base64 into the in window, the
//            inflater of inflate.hpp into the out window, which is its history too -- up to ASL_MGF_MAX_PEAKS * 16 =
//            64 KiB, twice DEFLATE's largest distance; nothing in the inflater assumes less -- then the big-endian
//            pairs into the two float32 columns.
//
// Every scan is reduce -> scan of the block partials -> apply, as separate launches on the library's stream: no
// kernel waits on another workgroup. Integer atomics only, and none whose arrival order reaches the output. Every
// byte index is bounded by the chunk length, every tag by line_start[n_tags] == n.
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "inflate.hpp"
#include "mzxml_value.hpp"
#include "text_records.hpp"
#include "xml_tag.hpp"

namespace asl {

enum : uint8_t { XK_OTHER = 0, XK_SCAN, XK_SCAN_END, XK_PMZ, XK_PEAKS, XK_COMMENT, XK_CUT };   // what a tag is
enum : uint8_t { XD_DEFERRED = 1, XD_SELF = 2, XD_NO_RT = 4, XD_BAD_LEVEL = 8 };                // dflag

struct XCtx {   // the context scan's element; also the scratch type of the unit's other scans (the widest)
  uint32_t nscan;    // sum: <scan opening tags
  uint32_t assign;   // the head state's assignment (0 keep, 2 clear, 3 set): the later one wins
  int32_t depth;     // sum: <scan> elements opened less </scan>
};
struct XCtxOp {
  using T = XCtx;
  __device__ static T identity() { return T{0u, 0u, 0}; }
  __device__ static T op(T a, T b) { return T{a.nscan + b.nscan, b.assign != 0u ? b.assign : a.assign, a.depth + b.depth}; }
};
struct XPair {
  uint32_t a, b;
};
struct XPairOp {
  using T = XPair;
  __device__ static T identity() { return T{0u, 0u}; }
  __device__ static T op(T x, T y) { return T{x.a + y.a, x.b + y.b}; }
};

// ---------------------------------------------------------------------------------------------- one tag
__device__ __forceinline__ bool xm_value_is(const uint8_t *__restrict__ t, uint32_t va, uint32_t vb, const char *lit,
                                            uint32_t n) {
  return zm_is(t, va, vb - va, lit, n);
}
// The end of the tag at line_start[L], bounded as in the tag pass, and the byte behind its name.
__device__ __forceinline__ void xm_tag(const uint8_t *__restrict__ t, const uint32_t *__restrict__ line_start,
                                       uint32_t L, uint32_t *q, uint32_t *e) {
  const uint32_t a = line_start[L];
  *e = zm_tag_end(t, a, min(line_start[L + 1], a + (uint32_t)ASL_MZML_MAX_TAG));
  uint32_t p = a + 1u;
  while (p < *e && !mg_ws(t[p]) && t[p] != '/') ++p;
  *q = p;
}

// kind, dflag, val, val2 and aux of every tag:
//   scan         val: msLevel (NONE: none, or XD_BAD_LEVEL) | peaksCount << 32 (NONE: none, or not plain digits);
//                val2: the retention time in minutes as a double's bits (XD_DEFERRED: not converted; XD_NO_RT)
//   precursorMz  val: its text as a double's bits (XD_DEFERRED: not converted); aux: precursorCharge (0: none; NONE:
//                not digits in 1 .. 255)
//   peaks        val: the content's (begin | end << 32); aux: ASL_MZXML_F_ZLIB | ASL_MZXML_F_F64 | ASL_MZXML_E_* << 8
__global__ __launch_bounds__(SCAN_NT) void mzxml_tags_kernel(const uint8_t *__restrict__ t,
                                                           const uint32_t *__restrict__ line_start, int64_t n_tags,
                                                           int last, uint8_t *__restrict__ kind,
                                                           uint8_t *__restrict__ dflag, uint64_t *__restrict__ val,
                                                           uint64_t *__restrict__ val2, uint32_t *__restrict__ aux,
                                                           TextFinal *__restrict__ fin) {
  const int64_t L = (int64_t)blockIdx.x * SCAN_NT + threadIdx.x;
  if (L >= n_tags) return;
  const uint32_t a = line_start[L], b = line_start[L + 1];
  uint8_t k = XK_OTHER, df = 0;
  uint64_t v = 0, v2 = 0;
  uint32_t x = 0u;
  // the last tag of a chunk that is not the file's last may be cut anywhere: it is not looked at
  const bool skip = last == 0 && L == n_tags - 1;
  uint32_t p = a + 1u;
  const bool closer = !skip && p < b && t[p] == '/';
  if (closer) ++p;
  uint32_t q = p;
  while (!skip && q < b && q - a <= 32u && !mg_ws(t[q]) && t[q] != '>' && t[q] != '/') ++q;
  if (skip) {
  } else if (b - p >= 3u && zm_is(t, p, 3u, "!--", 3u)) {
    k = XK_COMMENT;
  } else if (b - p >= 8u && zm_is(t, p, 8u, "![CDATA[", 8u)) {
    k = XK_COMMENT;
  } else {
    const uint32_t lim = min(b, a + (uint32_t)ASL_MZML_MAX_TAG);
    const uint32_t e = zm_tag_end(t, a, lim);
    const uint32_t nl = q - p;
    if (e == lim) {
      if (b - a > (uint32_t)ASL_MZML_MAX_TAG) atomicMin(&fin->long_line, (uint32_t)L);
      k = XK_CUT;
    } else {
      if (t[e - 1u] == '/' && e - 1u > a) df |= XD_SELF;
      if (zm_is(t, p, nl, "scan", 4u)) k = closer ? XK_SCAN_END : XK_SCAN;
      else if (!closer && zm_is(t, p, nl, "precursorMz", 11u)) k = XK_PMZ;
      else if (!closer && zm_is(t, p, nl, "peaks", 5u)) k = XK_PEAKS;
      uint32_t va, vb;
      if (k == XK_SCAN) {
        uint32_t level = NONE, count = NONE;
        if (zm_attr(t, q, e, "msLevel", 7u, &va, &vb)) {
          level = zm_uint(t, va, vb);
          if (level == NONE) df |= XD_BAD_LEVEL;
        }
        if (zm_attr(t, q, e, "peaksCount", 10u, &va, &vb)) count = zm_uint(t, va, vb);
        v = (uint64_t)level | ((uint64_t)count << 32);
        double d = 0.0;
        if (!zm_attr(t, q, e, "retentionTime", 13u, &va, &vb)) df |= XD_NO_RT;
        else if (mzx_duration(reinterpret_cast<const char *>(t) + va, (int)(vb - va), &d) != 0) df |= XD_DEFERRED;
        v2 = (uint64_t)__double_as_longlong(d);
      } else if (k == XK_PMZ) {
        uint32_t ca = e + 1u, cb = (df & XD_SELF) ? ca : b;   // (ca <= b)
        mg_strip(t, ca, cb, &ca, &cb);
        double d = 0.0;
        if (mgf_number(reinterpret_cast<const char *>(t) + ca, (int)(cb - ca), &d) != 0) df |= XD_DEFERRED;
        v = (uint64_t)__double_as_longlong(d);
        if (zm_attr(t, q, e, "precursorCharge", 15u, &va, &vb)) {
          x = zm_uint(t, va, vb);
          if (x < 1u || x > 255u) x = NONE;
        }
      } else if (k == XK_PEAKS) {
        const uint32_t cb = e + 1u;   // (<= b)
        v = (uint64_t)cb | ((uint64_t)((df & XD_SELF) ? cb : b) << 32);
        uint32_t err = 0u;
        if (!zm_attr(t, q, e, "precision", 9u, &va, &vb)) err |= ASL_MZXML_E_PRECISION;
        else if (xm_value_is(t, va, vb, "64", 2u)) x |= ASL_MZXML_F_F64;
        else if (!xm_value_is(t, va, vb, "32", 2u)) err |= ASL_MZXML_E_PRECISION;
        if (zm_attr(t, q, e, "byteOrder", 9u, &va, &vb) && !xm_value_is(t, va, vb, "network", 7u))
          err |= ASL_MZXML_E_BYTE_ORDER;
        if (zm_attr(t, q, e, "contentType", 11u, &va, &vb) && !xm_value_is(t, va, vb, "m/z-int", 7u))
          err |= ASL_MZXML_E_CONTENT_TYPE;
        if (zm_attr(t, q, e, "pairOrder", 9u, &va, &vb) && !xm_value_is(t, va, vb, "m/z-int", 7u))
          err |= ASL_MZXML_E_CONTENT_TYPE;
        if (zm_attr(t, q, e, "compressionType", 15u, &va, &vb)) {
          if (xm_value_is(t, va, vb, "zlib", 4u)) x |= ASL_MZXML_F_ZLIB;
          else if (!xm_value_is(t, va, vb, "none", 4u)) err |= ASL_MZXML_E_COMPRESSION;
        }
        x |= err << 8;
      }
    }
  }
  kind[L] = k, dflag[L] = df, val[L] = v, val2[L] = v2, aux[L] = x;
}

struct XCtxView {   // rec[L]: <scan tags up to and including tag L; dslot[L]: inside a head behind L; slot[L]: depth
  using Op = XCtxOp;
  const uint8_t *kind, *dflag;
  uint32_t *rec, *slot, *dslot;
  XCtx *totals;
  int64_t n_tags;
  __device__ XCtx load(int64_t L) const {
    const uint8_t k = kind[L];
    const bool self = (dflag[L] & XD_SELF) != 0;
    if (k == XK_SCAN) return XCtx{1u, self ? 2u : 3u, self ? 0 : 1};
    if (k == XK_SCAN_END) return XCtx{0u, 2u, -1};
    return XCtx{0u, 0u, 0};
  }
  __device__ void store(int64_t L, XCtx incl, XCtx) const {
    rec[L] = incl.nscan, slot[L] = (uint32_t)incl.depth, dslot[L] = incl.assign == 3u ? 1u : 0u;
    if (L == n_tags - 1) *totals = incl;
  }
};

// The tables of a measured chunk, in one buffer of words, per <scan tag s (stride ns): the tags that won, then,
// zeroed, the count of <peaks> and the errors.
enum : uint32_t { S_FIRST = 0, S_CLOSE, S_PMZ, S_PEAKS, S_DEPTH, S_FIELDS };
enum : uint32_t { Z_NPEAKS = 0, Z_ERR, Z_FIELDS };
struct XTables {
  uint32_t *S, *Z;
  uint32_t ns;
  __device__ uint32_t &s(uint32_t f, uint32_t i) const { return S[(size_t)f * ns + i]; }
  __device__ uint32_t &z(uint32_t f, uint32_t i) const { return Z[(size_t)f * ns + i]; }
};

// after_first: a <scan was seen before this chunk. cons: (tags << 32 | bytes) up to the last closed head.
__global__ __launch_bounds__(SCAN_NT) void mzxml_resolve_kernel(
    const uint8_t *__restrict__ kind, const uint8_t *__restrict__ dflag, const uint32_t *__restrict__ line_start,
    const uint32_t *__restrict__ rec, const uint32_t *__restrict__ slot, const uint32_t *__restrict__ dslot,
    int64_t n_tags, int after_first, XTables T, unsigned long long *__restrict__ cons, TextFinal *__restrict__ fin) {
  const int64_t L = (int64_t)blockIdx.x * SCAN_NT + threadIdx.x;
  if (L >= n_tags) return;
  const uint8_t k = kind[L];
  if (k == XK_OTHER) return;
  const bool in = L > 0 && dslot[L - 1] != 0u;   // inside a head in front of the tag (a chunk starts outside one)
  const uint32_t opened = rec[L];
  const bool seen = opened > 0u || after_first != 0;
  const auto error = [&](int e) { atomicMin(&fin->err, ((unsigned long long)L << 8) | (unsigned long long)e); };
  const auto closed = [&](int64_t tags) {
    atomicMax(cons, ((unsigned long long)tags << 32) | (unsigned long long)line_start[tags]);
  };
  if (k == XK_COMMENT && seen) error(ASL_MZXML_ERR_COMMENT);
  if (k == XK_CUT && seen) error(ASL_MZXML_ERR_TAG);
  if (k == XK_SCAN) {
    const uint32_t s = opened - 1u;
    if (s >= T.ns) return;   // (cannot happen: kept as the bound of every per-scan store)
    T.s(S_FIRST, s) = (uint32_t)L;
    T.s(S_DEPTH, s) = L > 0 ? slot[L - 1] : 0u;
    if (dflag[L] & XD_BAD_LEVEL) error(ASL_MZXML_ERR_LEVEL);
    if (in && s > 0u) T.s(S_CLOSE, s - 1u) = (uint32_t)L, closed(L);   // the head in front ends here
    if (dflag[L] & XD_SELF) T.s(S_CLOSE, s) = (uint32_t)L + 1u, closed(L + 1);
    return;
  }
  if (k == XK_SCAN_END) {
    if (in && opened - 1u < T.ns) T.s(S_CLOSE, opened - 1u) = (uint32_t)L + 1u, closed(L + 1);
    return;
  }
  if (k == XK_PMZ || k == XK_PEAKS) {
    if (!in) {
      error(ASL_MZXML_ERR_OUTSIDE);
      return;
    }
    const uint32_t s = opened - 1u;   // (inside a head: opened >= 1)
    if (s >= T.ns) return;
    if (k == XK_PMZ) atomicMin(&T.s(S_PMZ, s), (uint32_t)L);
    else atomicMin(&T.s(S_PEAKS, s), (uint32_t)L), atomicAdd(&T.z(Z_NPEAKS, s), 1u);   // (an integer count)
  }
}

// per <scan tag: read or not (sel), its peak count (npk), its charge (zc), its errors
__global__ __launch_bounds__(SCAN_NT) void mzxml_scans_kernel(const uint8_t *__restrict__ dflag,
                                                            const uint64_t *__restrict__ val,
                                                            const uint32_t *__restrict__ aux, XTables T,
                                                            uint32_t *__restrict__ sel, uint32_t *__restrict__ npk,
                                                            uint32_t *__restrict__ zc, TextFinal *__restrict__ fin) {
  const uint32_t s = blockIdx.x * SCAN_NT + threadIdx.x;
  if (s >= T.ns) return;
  const uint32_t ft = T.s(S_FIRST, s);
  const bool ms2 = T.s(S_CLOSE, s) != NONE && ft != NONE && (uint32_t)val[ft] == 2u;
  if (!ms2) {
    sel[s] = 0u, npk[s] = 0u, zc[s] = 0u;
    return;
  }
  uint32_t err = 0u, n = (uint32_t)(val[ft] >> 32), z = 0u;
  if (n == NONE) err |= ASL_MZXML_E_COUNT, n = 0u;
  const uint32_t pk = T.s(S_PEAKS, s), pm = T.s(S_PMZ, s);
  if (pk == NONE) err |= ASL_MZXML_E_NO_PEAKS;
  else err |= (aux[pk] >> 8) & (uint32_t)ASL_MZXML_E_FILE;
  if (T.z(Z_NPEAKS, s) > 1u) err |= ASL_MZXML_E_PEAKS_TWICE;
  if (dflag[ft] & XD_NO_RT) err |= ASL_MZXML_E_NO_RT;
  if (pm == NONE) {
    err |= ASL_MZXML_E_NO_PRECURSOR;
  } else {
    z = aux[pm];
    if (z == NONE) err |= ASL_MZXML_E_CHARGE, z = 0u;
  }
  if (n > (uint32_t)ASL_MGF_MAX_PEAKS) atomicMin(&fin->cap_rec, s), n = 0u;
  T.z(Z_ERR, s) = err;
  sel[s] = 1u, npk[s] = n, zc[s] = z;
}

struct XSlotView {   // ord[s]: MS2 scans before s; pbeg[s]: their peaks
  using Op = XPairOp;
  const uint32_t *sel, *npk;
  uint32_t *ord, *pbeg;
  XPair *totals;
  int64_t ns;
  __device__ XPair load(int64_t s) const { return XPair{sel[s], npk[s]}; }
  __device__ void store(int64_t s, XPair incl, XPair own) const {
    ord[s] = incl.a - own.a, pbeg[s] = incl.b - own.b;
    if (s == ns - 1) *totals = incl;
  }
};

// ---------------------------------------------------------------------------------------------- fill
struct XStream {   // the one stream of an MS2 scan
  uint32_t begin, end;   // its characters
  uint32_t slot, n;      // its first peak slot and its peaks
  uint32_t mode;         // ASL_MZXML_F_ZLIB, ASL_MZXML_F_F64; 4: not to be decoded (the scan has an error)
};

__global__ __launch_bounds__(SCAN_NT) void mzxml_fill_scans_kernel(
    const uint8_t *__restrict__ t, const uint32_t *__restrict__ line_start, const uint8_t *__restrict__ dflag,
    const uint64_t *__restrict__ val, const uint64_t *__restrict__ val2, const uint32_t *__restrict__ aux, XTables T,
    const uint32_t *__restrict__ sel, const uint32_t *__restrict__ npk, const uint32_t *__restrict__ zc,
    const uint32_t *__restrict__ ord, const uint32_t *__restrict__ pbeg, uint32_t n_out, uint32_t n_text, int depth0,
    int32_t *__restrict__ offsets, double *__restrict__ pmz, int32_t *__restrict__ pcharge, double *__restrict__ rt,
    int32_t *__restrict__ ident, int32_t *__restrict__ first, int32_t *__restrict__ element,
    int32_t *__restrict__ numerals, int32_t *__restrict__ errors, int32_t *__restrict__ flags,
    XStream *__restrict__ streams) {
  const uint32_t s = blockIdx.x * SCAN_NT + threadIdx.x;
  if (s >= T.ns || sel[s] == 0u) return;
  const uint32_t o = ord[s];
  if (o >= n_out) return;   // (cannot happen: n_out is the scan's total)
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const uint32_t ft = T.s(S_FIRST, s), err = T.z(Z_ERR, s), pm = T.s(S_PMZ, s), pk = T.s(S_PEAKS, s);
  offsets[o] = (int32_t)pbeg[s];
  first[o] = (int32_t)ft, element[o] = (int32_t)s, errors[o] = (int32_t)err, pcharge[o] = (int32_t)zc[s];
  // the scan's tag is walked again for the byte ranges the host wants, as mgf.hip walks a deferred line again
  uint32_t q, e, va, vb;
  xm_tag(t, line_start, ft, &q, &e);
  const bool has_num = zm_attr(t, q, e, "num", 3u, &va, &vb);
  ident[2 * (size_t)o] = has_num ? (int32_t)va : 0, ident[2 * (size_t)o + 1] = has_num ? (int32_t)(vb - va) : -1;
  int32_t *const num = numerals + 4 * (size_t)o;
  num[0] = num[2] = 0, num[1] = num[3] = -1;
  double v = nan;
  if ((dflag[ft] & XD_NO_RT) == 0) {
    if ((dflag[ft] & XD_DEFERRED) == 0) {
      v = __longlong_as_double((long long)val2[ft]);
    } else if (zm_attr(t, q, e, "retentionTime", 13u, &va, &vb)) {
      num[0] = (int32_t)va, num[1] = (int32_t)(vb - va);
    }
  }
  rt[o] = v;
  v = nan;
  if (pm != NONE) {
    if ((dflag[pm] & XD_DEFERRED) == 0) {
      v = __longlong_as_double((long long)val[pm]);
    } else {
      xm_tag(t, line_start, pm, &q, &e);
      uint32_t ca = min(e + 1u, line_start[pm + 1]), cb = (dflag[pm] & XD_SELF) ? ca : line_start[pm + 1];
      mg_strip(t, ca, cb, &ca, &cb);
      num[2] = (int32_t)ca, num[3] = (int32_t)(cb - ca);
    }
  }
  pmz[o] = v;
  XStream A = {0u, 0u, pbeg[s], npk[s], 4u};
  uint32_t fl = (depth0 + (int)T.s(S_DEPTH, s)) > 0 ? (uint32_t)ASL_MZXML_F_NESTED : 0u;
  if (pk != NONE) fl |= aux[pk] & (uint32_t)(ASL_MZXML_F_ZLIB | ASL_MZXML_F_F64);
  if (err == 0u) {   // (err == 0: the <peaks> exists, with its precision and compression)
    const uint64_t c = val[pk];
    A.begin = min((uint32_t)c, n_text), A.end = min((uint32_t)(c >> 32), n_text);
    A.mode = aux[pk] & (uint32_t)(ASL_MZXML_F_ZLIB | ASL_MZXML_F_F64);
  }
  streams[o] = A;
  flags[o] = (int32_t)fl;
}

// One thread per stream over windows in global scratch. The stream of a scan with n peaks from peak slot p has its
// out window at 16 p (n pairs of at most 16 bytes), its in window at 18 p + 80 a (the base64-decoded bytes: at most
// 16 n + 2 n + 64 of a compressed stream, and a quad's three bytes of room) and its tables at index a.
__global__ __launch_bounds__(64) void mzxml_decode_kernel(const uint8_t *__restrict__ t,
                                                        const XStream *__restrict__ streams, uint32_t n_streams,
                                                        uint32_t n_peaks, uint8_t *__restrict__ out_all,
                                                        uint8_t *__restrict__ in_all, InfWork *__restrict__ work_all,
                                                        float *__restrict__ mz, float *__restrict__ intensity,
                                                        int32_t *__restrict__ aerr) {
  const uint32_t a = blockIdx.x * 64u + threadIdx.x;
  if (a >= n_streams) return;
  const XStream A = streams[a];
  if ((uint64_t)A.slot + A.n > (uint64_t)n_peaks) {   // (cannot happen: the slots are a scan over the counts)
    aerr[a] = 0;
    return;
  }
  int err = INF_OK;
  const uint8_t *src = nullptr;
  const uint32_t width = (A.mode & ASL_MZXML_F_F64) ? 8u : 4u;
  if ((A.mode & 4u) == 0u) {
    uint8_t *const out = out_all + 16ull * A.slot, *const in = in_all + 18ull * A.slot + 80ull * a;
    const uint32_t expect = A.n * 2u * width, limit = expect + expect / 8u + 64u;
    uint32_t m = 0u, got = 0u;
    err = b64_decode(t + A.begin, A.end > A.begin ? A.end - A.begin : 0u, in, 18u * A.n + 80u, &m);   // (limit + 3 <= 18 n + 80)
    src = in;
    if (err == INF_OK && (A.mode & ASL_MZXML_F_ZLIB) != 0u && !(expect == 0u && m == 0u)) {
      err = m > limit ? INF_INPUT : inf_inflate(in, m, out, expect, &got, work_all + a);
      if (err == INF_OK && got < expect) err = INF_LENGTH;
      src = out;
    } else if (err == INF_OK) {
      err = m > expect ? INF_SINK : m < expect ? INF_LENGTH : INF_OK;
    }
  }
  // a scan that is refused or not decoded keeps its slots (the host drops or refuses it): zeros, not what the
  // buffer held, so that nothing behind this kernel depends on it
  const bool decoded = src != nullptr && err == INF_OK;
  for (uint32_t i = 0; i < A.n; ++i) {   // (A.slot + i < n_peaks: checked above)
    float x = 0.0f, y = 0.0f;
    if (decoded) mzx_pair(src, i, width, &x, &y);
    mz[A.slot + i] = x, intensity[A.slot + i] = y;
  }
  aerr[a] = err;
}

namespace {

struct MzxmlWork : ChunkWork<XCtx> {
  DevBuf<uint8_t> scratch_out, scratch_in;
  DevBuf<InfWork> scratch_work;
  DevBuf<uint64_t> val2;
  DevBuf<uint32_t> aux, tab, sel, npk, zc, ord, pbeg;
  DevBuf<XPair> pair;
  DevBuf<XStream> streams;
  uint32_t n_open = 0;
  int depth0 = 0;
  XTables tables() { return XTables{tab.p, tab.p + (size_t)S_FIELDS * n_open, n_open}; }
};
MzxmlWork &work() {
  static MzxmlWork w;
  return w;
}

}  // namespace
}  // namespace asl

using namespace asl;

extern "C" int asl_mzxml_duration(const char *s, int32_t n, double *minutes) {
  if (minutes == nullptr || n < 0 || (s == nullptr && n > 0)) return 1;
  return mzx_duration(s != nullptr ? s : "", (int)n, minutes);
}

extern "C" int asl_mzxml_pairs(const uint8_t *raw, int32_t n_peaks, int32_t precision, float *mz, float *intensity) {
  if (n_peaks < 0 || (precision != 32 && precision != 64)) return -1;
  if (n_peaks > 0 && (raw == nullptr || mz == nullptr || intensity == nullptr)) return -1;
  for (int32_t i = 0; i < n_peaks; ++i) mzx_pair(raw, (uint32_t)i, (uint32_t)precision / 8u, mz + i, intensity + i);
  return 0;
}

extern "C" int asl_mzxml_measure(const uint8_t *text, int64_t n, int32_t last, int64_t *counts) {
  clear_error();
  MzxmlWork &W = work();
  if (last < 0 || (last & ~0xff03) != 0)
    return fail(ASL_ERR_INVALID, "mzxml_measure: last = %d, bits 0, 1 and 8 .. 15", (int)last);
  const int after_first = (last >> 1) & 1, depth0 = (last >> 8) & 255;
  last &= 1;
  ASL_TRY(measure_begin("mzxml", W, text, n, last, counts));
  counts[ASL_MZXML_N_ELEMENTS] = counts[ASL_MZXML_ERR_ELEMENT] = 0;
  counts[ASL_MZXML_DEPTH_ALL] = counts[ASL_MZXML_DEPTH_CONSUMED] = depth0;
  W.n_open = 0, W.depth0 = depth0;
  if (n == 0) return ASL_OK;
  ProfScope ps("mzxml_measure");
  int64_t nl = 0;   // >= 0
  ASL_TRY(line_starts<(uint8_t)'<'>(text, n, W.count, W.partial, W.line_start, &nl));
  ASL_TRY(measure_lines(W, std::max<int64_t>(nl, 1)));
  TextFinal F{~0ull, 0u, 0u, ~0u, ~0u};
  if (nl == 0) {   // no tag at all: nothing to consume but the bytes
    counts[ASL_MGF_CONSUMED] = 0;
    return measure_end("mzxml", "scan", W, F, text, n, counts, "peaks");
  }
  // tags, context
  ASL_TRY(W.aux.reserve((size_t)nl));
  ASL_TRY(W.val2.reserve((size_t)nl));
  hipLaunchKernelGGL(mzxml_tags_kernel, dim3(blocks_of(nl)), dim3(SCAN_NT), 0, stream(), text, W.line_start.p, nl,
                     (int)last, W.kind.p, W.dflag.p, W.val.p, W.val2.p, W.aux.p, W.fin.p);
  ASL_CHECK_LAUNCH();
  ASL_TRY(scan_view(XCtxView{W.kind.p, W.dflag.p, W.rec.p, W.slot.p, W.dslot.p, W.totals.p, nl}, nl, W.partial.p));
  XCtx C;
  HIP_TRY(hipMemcpyAsync(&C, W.totals.p, sizeof(C), hipMemcpyDeviceToHost, stream()));
  ASL_TRY(sync_stream());
  // per scan: the winning tags, the errors, the peak counts; then the slots
  const uint32_t ns = C.nscan;
  const bool open = C.assign == 3u;
  W.n_open = ns;
  const size_t ones = (size_t)S_FIELDS * ns, zeros = (size_t)Z_FIELDS * ns;
  ASL_TRY(W.tab.reserve(std::max<size_t>(ones + zeros, 1)));
  ASL_TRY(W.sel.reserve(std::max<size_t>(ns, 1)));
  ASL_TRY(W.npk.reserve(std::max<size_t>(ns, 1)));
  ASL_TRY(W.zc.reserve(std::max<size_t>(ns, 1)));
  ASL_TRY(W.ord.reserve(std::max<size_t>(ns, 1)));
  ASL_TRY(W.pbeg.reserve(std::max<size_t>(ns, 1)));
  ASL_TRY(W.pair.reserve(1));
  if (ones > 0) HIP_TRY(hipMemsetAsync(W.tab.p, 0xff, ones * sizeof(uint32_t), stream()));
  if (zeros > 0) HIP_TRY(hipMemsetAsync(W.tab.p + ones, 0, zeros * sizeof(uint32_t), stream()));
  HIP_TRY(hipMemsetAsync(W.count.p, 0, sizeof(unsigned long long), stream()));
  HIP_TRY(hipMemsetAsync(W.pair.p, 0, sizeof(XPair), stream()));
  const XTables T = W.tables();
  hipLaunchKernelGGL(mzxml_resolve_kernel, dim3(blocks_of(nl)), dim3(SCAN_NT), 0, stream(), W.kind.p, W.dflag.p,
                     W.line_start.p, W.rec.p, W.slot.p, W.dslot.p, nl, after_first, T, W.count.p, W.fin.p);
  ASL_CHECK_LAUNCH();
  if (ns > 0) {
    hipLaunchKernelGGL(mzxml_scans_kernel, dim3(blocks_of(ns)), dim3(SCAN_NT), 0, stream(), W.dflag.p, W.val.p,
                       W.aux.p, T, W.sel.p, W.npk.p, W.zc.p, W.fin.p);
    ASL_CHECK_LAUNCH();
    ASL_TRY(scan_view(XSlotView{W.sel.p, W.npk.p, W.ord.p, W.pbeg.p, W.pair.p, (int64_t)ns}, ns, W.partial.p));
  }
  XPair P;
  unsigned long long cons = 0;
  HIP_TRY(hipMemcpyAsync(&P, W.pair.p, sizeof(P), hipMemcpyDeviceToHost, stream()));
  HIP_TRY(hipMemcpyAsync(&cons, W.count.p, sizeof(cons), hipMemcpyDeviceToHost, stream()));
  ASL_TRY(measure_final("mzxml", W, &F, "tag", ASL_MZML_MAX_TAG));
  counts[ASL_MGF_N_LINES] = nl;
  counts[ASL_MGF_N_SPECTRA] = P.a;
  counts[ASL_MGF_N_PEAKS] = P.b;
  counts[ASL_MGF_N_DEFERRED] = 0;
  counts[ASL_MGF_CONSUMED] = (int64_t)(cons & 0xffffffffull);
  counts[ASL_MGF_CONSUMED_LINES] = (int64_t)(cons >> 32);
  counts[ASL_MGF_OPEN] = open ? 1 : 0;
  counts[ASL_MZXML_N_ELEMENTS] = (int64_t)ns - (open ? 1 : 0);
  counts[ASL_MZXML_DEPTH_ALL] = std::max(0, depth0 + (int)C.depth);
  const int64_t cl = (int64_t)(cons >> 32);   // <= nl
  uint32_t opened = 0, depth = 0;
  if (cl > 0) HIP_TRY(hipMemcpyAsync(&depth, W.slot.p + (cl - 1), sizeof(depth), hipMemcpyDeviceToHost, stream()));
  if (F.err != ~0ull)
    HIP_TRY(hipMemcpyAsync(&opened, W.rec.p + (F.err >> 8), sizeof(opened), hipMemcpyDeviceToHost, stream()));
  if (cl > 0 || F.err != ~0ull) ASL_TRY(sync_stream());
  counts[ASL_MZXML_DEPTH_CONSUMED] = std::max(0, depth0 + (int)depth);
  counts[ASL_MZXML_ERR_ELEMENT] = opened;
  return measure_end("mzxml", "scan", W, F, text, n, counts, "peaks");
}

extern "C" int asl_mzxml_fill(const uint8_t *text, int64_t n, int32_t *offsets, float *mz, float *intensity,
                              uint8_t *charge, double *precursor_mz, int32_t *precursor_charge,
                              double *retention_time, int32_t *identifier, int32_t *first_tag, int32_t *element,
                              int32_t *numerals, int32_t *errors, int32_t *flags, int32_t *array_errors) {
  clear_error();
  MzxmlWork &W = work();
  ASL_TRY(fill_begin("mzxml", W, text, n, offsets));
  const uint32_t ns = W.n_rec, np = W.n_peaks;
  if (ns == 0) return fill_empty(offsets);
  if ((np > 0 && (!mz || !intensity)) || !precursor_mz || !precursor_charge || !retention_time || !identifier ||
      !first_tag || !element || !numerals || !errors || !flags || !array_errors)
    return fail(ASL_ERR_INVALID, "mzxml_fill: a null output");
  ASL_TRY(ensure_device());
  ProfScope ps("mzxml_fill");
  Out<int32_t> oOff, oZ, oId, oFirst, oEl, oNum, oErr, oFl, oAe;
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
  ASL_TRY(oFirst.init(first_tag, ns));
  ASL_TRY(oEl.init(element, ns));
  ASL_TRY(oNum.init(numerals, (size_t)ns * 4));
  ASL_TRY(oErr.init(errors, ns));
  ASL_TRY(oFl.init(flags, ns));
  ASL_TRY(oAe.init(array_errors, ns));
  ASL_TRY(W.streams.reserve((size_t)ns));
  if (oChg.d != nullptr) HIP_TRY(hipMemsetAsync(oChg.d, 0, np, stream()));
  HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(oOff.d + ns), (int)np, 1, stream()));
  hipLaunchKernelGGL(mzxml_fill_scans_kernel, dim3(blocks_of(W.n_open)), dim3(SCAN_NT), 0, stream(), text,
                     W.line_start.p, W.dflag.p, W.val.p, W.val2.p, W.aux.p, W.tables(), W.sel.p, W.npk.p, W.zc.p,
                     W.ord.p, W.pbeg.p, ns, (uint32_t)n, W.depth0, oOff.d, oPmz.d, oZ.d, oRt.d, oId.d, oFirst.d, oEl.d,
                     oNum.d, oErr.d, oFl.d, W.streams.p);
  ASL_CHECK_LAUNCH();
  ASL_TRY(W.scratch_out.reserve(std::max<size_t>((size_t)np * 16, 1)));
  ASL_TRY(W.scratch_in.reserve((size_t)np * 18 + (size_t)ns * 80));
  ASL_TRY(W.scratch_work.reserve((size_t)ns));
  {
    ProfScope pd("mzxml_decode");
    hipLaunchKernelGGL(mzxml_decode_kernel, dim3((unsigned)cdiv((int64_t)ns, 64)), dim3(64), 0, stream(), text,
                       W.streams.p, ns, np, W.scratch_out.p, W.scratch_in.p, W.scratch_work.p, oMz.d, oIt.d, oAe.d);
    ASL_CHECK_LAUNCH();
  }
  return finish_outputs(oOff, oMz, oIt, oChg, oPmz, oZ, oRt, oId, oFirst, oEl, oNum, oErr, oFl, oAe);
}
