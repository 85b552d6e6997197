// mzml.hip -- mzML query files parsed and decoded on the device (asl_mzml_measure / asl_mzml_fill) and the decoder
// core on the host (asl_mzml_inflate). gfx950 only. DESIGN.md 3 "Query files"; the dialect is stated in
// include/annsolo_mi.h and restated in tests/mzml_ref.py. Shared with mgf.hip and sptxt.hip: the scans and the unit
// starts (text_scan.hpp, with '<' as the byte: a unit is a tag) and the grammar-free host parts of measure and fill
// (text_records.hpp). The base64 step and the inflater are inflate.hpp, which the host compiles too.
//
//   starts   count the tag starts, scan the counts, write line_start[] (text_scan.hpp; an entry is the byte of a '<')
//   tags     one thread per tag: find its '>' outside quotes, classify it by name, read the attributes it needs
//            (spectrum: id, defaultArrayLength; cvParam: accession, value; binary: the extent of its content) and
//            convert its numeral (mgf_number.hpp); what the converter defers is flagged, never guessed. The thread
//            of <binary> never walks the content: an MS1 profile array costs the start pass alone.
//   context  a scan that composes the tags' maps of the element state: per container (spectrum, scanList, scan,
//            precursorList, precursor, selectedIon, binaryDataArray) a two-bit assignment {keep, clear, set}, and
//            the counts of scans and precursors since the last <spectrum> and of selected ions since the last
//            <precursor> as segmented sums. Every tag learns: inside a spectrum, which one, inside the first scan,
//            the first selected ion of the first precursor, which binary array.
//   resolve  per tag: "the first wins" -> integer atomicMin of the tag ordinal per (spectrum or array, parameter);
//            the first structural error -> atomicMin of (tag << 8 | kind); the byte behind the last closed spectrum
//            -> atomicMax. Then per array (which spectrum's m/z or intensity it is) and per spectrum (MS level,
//            errors, peak count).
//   slots    a scan over the spectra hands out the MS2 ordinals and the peak slots from defaultArrayLength
//   fill     the per-spectrum columns, then the arrays. Two shapes of the decode were built and measured
//            (profiles/mzml_cost.json), both on the core of inflate.hpp. The default is the faster one, one thread
//            per (MS2 spectrum, array) over windows in global scratch: 28.7 ms for 2 * 10^5 arrays of about 100
//            values. The other (ASL_MZML_DECODE=wave in the environment; 52.5 ms) is one wavefront per array:
//            base64 into LDS by the whole wave, the inflater by one lane from LDS into a window in LDS (the raw
//            array is at most ASL_MGF_MAX_PEAKS * 8 = 32 KiB, DEFLATE's largest distance), conversion and stores
//            by the whole wave, in two launches by size: arrays up to ASL_MZML_SMALL_PEAKS values take 10 KiB of
//            LDS a wave, the others 70 KiB. With one lane in the symbol loop, LDS limits it to 15 waves a CU.
//
// Every scan is reduce -> scan of the block partials -> apply, as separate launches on the library's stream: no
// kernel waits on another workgroup. Integer atomics only, and none whose arrival order reaches the output. Every
// byte index is bounded by the chunk length, every tag by line_start[n_tags] == n, every LDS index by its buffer.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "inflate.hpp"
#include "mgf_number.hpp"
#include "text_records.hpp"
#include "xml_tag.hpp"

namespace asl {

enum : uint8_t {   // what a tag is, whatever surrounds it
  ZK_OTHER = 0, ZK_SPEC, ZK_SPEC_END, ZK_CV, ZK_SCANLIST, ZK_SCANLIST_END, ZK_SCAN, ZK_SCAN_END, ZK_PRECLIST,
  ZK_PRECLIST_END, ZK_PREC, ZK_PREC_END, ZK_SION, ZK_SION_END, ZK_BDA, ZK_BDA_END, ZK_BIN, ZK_BIN_END, ZK_REF,
  ZK_COMMENT, ZK_CUT
};
enum : uint8_t { ZD_DEFERRED = 1, ZD_SELF = 2, ZD_ARRAY_LENGTH = 4 };   // dflag
enum : uint32_t {   // a cvParam's accession (aux)
  CV_NONE = 0, CV_LEVEL, CV_RT, CV_PMZ, CV_Z, CV_PZ, CV_MZ, CV_IT, CV_F64, CV_F32, CV_PLAIN, CV_ZLIB, CV_BAD_PREC,
  CV_BAD_COMP
};
// the containers of the context: field f holds bits 2f, 2f + 1 of an assignment (0 keep, 2 clear, 3 set)
enum : uint32_t { ZF_SPEC = 0, ZF_SCANLIST, ZF_SCAN, ZF_PRECLIST, ZF_PREC, ZF_SION, ZF_BDA, ZF_N };
constexpr uint32_t ZF_CLEAR_ALL = 0x2AAAu;
static_assert(ZF_N == 7, "ZF_CLEAR_ALL clears seven fields");

struct MzCtx {   // the context scan's element; also the scratch type of the unit's other scans (the widest)
  uint32_t spec, bda;              // sums: <spectrum> and <binaryDataArray> opened
  uint32_t assign;                 // the containers' assignments: the later one wins
  uint32_t reset;                  // bit 0: n_scan and n_prec start again; bit 1: n_sion does
  uint32_t n_scan, n_prec, n_sion; // segmented sums
};
struct MzCtxOp {
  using T = MzCtx;
  __device__ static T identity() { return T{0u, 0u, 0u, 0u, 0u, 0u, 0u}; }
  __device__ static T op(T a, T b) {
    const uint32_t hb = b.assign & 0xAAAAu, m = hb | (hb >> 1);
    T r;
    r.spec = a.spec + b.spec, r.bda = a.bda + b.bda;
    r.assign = (a.assign & ~m) | (b.assign & m);
    r.reset = a.reset | b.reset;
    r.n_scan = (b.reset & 1u) ? b.n_scan : a.n_scan + b.n_scan;
    r.n_prec = (b.reset & 1u) ? b.n_prec : a.n_prec + b.n_prec;
    r.n_sion = (b.reset & 2u) ? b.n_sion : a.n_sion + b.n_sion;
    return r;
  }
};
struct MzPair {
  uint32_t a, b;
};
struct MzPairOp {
  using T = MzPair;
  __device__ static T identity() { return T{0u, 0u}; }
  __device__ static T op(T x, T y) { return T{x.a + y.a, x.b + y.b}; }
};

// a tag's context as one word: bit f: inside container f; the three counts, saturated at 3, from bit 8 on
__device__ __forceinline__ uint32_t zm_pack(const MzCtx &c) {
  uint32_t w = 0u;
#pragma unroll
  for (uint32_t f = 0; f < ZF_N; ++f)
    if (((c.assign >> (2u * f)) & 3u) == 3u) w |= 1u << f;
  return w | (min(c.n_scan, 3u) << 8) | (min(c.n_prec, 3u) << 10) | (min(c.n_sion, 3u) << 12);
}
__device__ __forceinline__ bool zm_in(uint32_t w, uint32_t f) { return ((w >> f) & 1u) != 0u; }

// ---------------------------------------------------------------------------------------------- one tag
// (where a tag ends, its name, its attributes, plain digits: xml_tag.hpp, shared with mzxml.hip)
__device__ __forceinline__ uint32_t zm_accession(const uint8_t *__restrict__ t, uint32_t a, uint32_t b) {
  if (b - a != 10u || !zm_is(t, a, 3u, "MS:", 3u)) return CV_NONE;
  const uint32_t v = zm_uint(t, a + 3u, b);
  switch (v) {
    case 1000511u: return CV_LEVEL;
    case 1000016u: return CV_RT;
    case 1000744u: return CV_PMZ;
    case 1000041u: return CV_Z;
    case 1000633u: return CV_PZ;
    case 1000514u: return CV_MZ;
    case 1000515u: return CV_IT;
    case 1000523u: return CV_F64;
    case 1000521u: return CV_F32;
    case 1000576u: return CV_PLAIN;
    case 1000574u: return CV_ZLIB;
    case 1000519u: case 1000522u: case 1000520u: case 1001479u: return CV_BAD_PREC;   // integers, half, strings
    case 1002312u: case 1002313u: case 1002314u: case 1002746u: case 1002747u: case 1002748u: case 1003089u:
    case 1003090u: return CV_BAD_COMP;                                                // Numpress and its kin
    default: return CV_NONE;
  }
}

// kind, dflag, val and aux of every tag:
//   spectrum   val: the id's (offset | length << 32), length NONE without one; aux: defaultArrayLength or NONE
//   cvParam    aux: CV_*; val: the value as a double's bits (CV_RT, CV_PMZ; ZD_DEFERRED: not converted) or as an
//              integer (CV_LEVEL, CV_Z, CV_PZ; NONE: not plain digits)
//   binary     val: the content's (begin | end << 32)
__global__ __launch_bounds__(SCAN_NT) void mzml_tags_kernel(const uint8_t *__restrict__ t,
                                                          const uint32_t *__restrict__ line_start, int64_t n_tags,
                                                          int last, uint8_t *__restrict__ kind,
                                                          uint8_t *__restrict__ dflag, uint64_t *__restrict__ val,
                                                          uint32_t *__restrict__ aux, TextFinal *__restrict__ fin) {
  const int64_t L = (int64_t)blockIdx.x * SCAN_NT + threadIdx.x;
  if (L >= n_tags) return;
  const uint32_t a = line_start[L], b = line_start[L + 1];
  uint8_t k = ZK_OTHER, df = 0;
  uint64_t v = 0;
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
    k = ZK_COMMENT;
  } else if (b - p >= 8u && zm_is(t, p, 8u, "![CDATA[", 8u)) {
    k = ZK_COMMENT;
  } else {
    const uint32_t lim = min(b, a + (uint32_t)ASL_MZML_MAX_TAG);
    const uint32_t e = zm_tag_end(t, a, lim);
    const uint32_t nl = q - p;
    if (e == lim) {
      if (b - a > (uint32_t)ASL_MZML_MAX_TAG) atomicMin(&fin->long_line, (uint32_t)L);
      k = ZK_CUT;
    } else {
      if (t[e - 1u] == '/' && e - 1u > a) df |= ZD_SELF;
      if (zm_is(t, p, nl, "spectrum", 8u)) k = closer ? ZK_SPEC_END : ZK_SPEC;
      else if (zm_is(t, p, nl, "cvParam", 7u)) k = closer ? ZK_OTHER : ZK_CV;
      else if (zm_is(t, p, nl, "scanList", 8u)) k = closer ? ZK_SCANLIST_END : ZK_SCANLIST;
      else if (zm_is(t, p, nl, "scan", 4u)) k = closer ? ZK_SCAN_END : ZK_SCAN;
      else if (zm_is(t, p, nl, "precursorList", 13u)) k = closer ? ZK_PRECLIST_END : ZK_PRECLIST;
      else if (zm_is(t, p, nl, "precursor", 9u)) k = closer ? ZK_PREC_END : ZK_PREC;
      else if (zm_is(t, p, nl, "selectedIon", 11u)) k = closer ? ZK_SION_END : ZK_SION;
      else if (zm_is(t, p, nl, "binaryDataArray", 15u)) k = closer ? ZK_BDA_END : ZK_BDA;
      else if (zm_is(t, p, nl, "binary", 6u)) k = closer ? ZK_BIN_END : ZK_BIN;
      else if (zm_is(t, p, nl, "referenceableParamGroupRef", 26u)) k = closer ? ZK_OTHER : ZK_REF;
      uint32_t va, vb;
      if (k == ZK_SPEC) {
        v = zm_attr(t, q, e, "id", 2u, &va, &vb) ? ((uint64_t)va | ((uint64_t)(vb - va) << 32))
                                                  : ((uint64_t)NONE << 32);
        x = zm_attr(t, q, e, "defaultArrayLength", 18u, &va, &vb) ? zm_uint(t, va, vb) : NONE;
      } else if (k == ZK_BDA) {
        if (zm_attr(t, q, e, "arrayLength", 11u, &va, &vb)) df |= ZD_ARRAY_LENGTH;
      } else if (k == ZK_BIN) {
        const uint32_t cb = e + 1u;   // (<= b)
        v = (uint64_t)cb | ((uint64_t)((df & ZD_SELF) ? cb : b) << 32);
      } else if (k == ZK_CV) {
        x = zm_attr(t, q, e, "accession", 9u, &va, &vb) ? zm_accession(t, va, vb) : CV_NONE;
        if (x == CV_RT || x == CV_PMZ) {
          double d = 0.0;
          if (!zm_attr(t, q, e, "value", 5u, &va, &vb)) va = vb = e;
          if (mgf_number(reinterpret_cast<const char *>(t) + va, (int)(vb - va), &d) != 0) df |= ZD_DEFERRED;
          v = (uint64_t)__double_as_longlong(d);
        } else if (x == CV_LEVEL || x == CV_Z || x == CV_PZ) {
          v = zm_attr(t, q, e, "value", 5u, &va, &vb) ? (uint64_t)zm_uint(t, va, vb) : (uint64_t)NONE;
        }
      }
    }
  }
  kind[L] = k, dflag[L] = df, val[L] = v, aux[L] = x;
}

struct CtxView {   // rec[L]: spectra opened up to and including tag L; slot[L]: arrays; dslot[L]: zm_pack behind L
  using Op = MzCtxOp;
  const uint8_t *kind, *dflag;
  uint32_t *rec, *slot, *dslot;
  MzCtx *totals;
  int64_t n_tags;
  __device__ MzCtx load(int64_t L) const {
    const uint8_t k = kind[L];
    const bool self = (dflag[L] & ZD_SELF) != 0;
    MzCtx c = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    const auto open = [&](uint32_t f) { return self ? 0u : 3u << (2u * f); };
    const auto shut = [](uint32_t f) { return 2u << (2u * f); };
    switch (k) {
      case ZK_SPEC: c.spec = 1u, c.reset = 3u, c.assign = self ? ZF_CLEAR_ALL : (ZF_CLEAR_ALL | 3u); break;
      case ZK_SPEC_END: c.assign = ZF_CLEAR_ALL; break;
      case ZK_SCANLIST: c.assign = open(ZF_SCANLIST); break;
      case ZK_SCANLIST_END: c.assign = shut(ZF_SCANLIST) | shut(ZF_SCAN); break;
      case ZK_SCAN: c.n_scan = 1u, c.assign = open(ZF_SCAN); break;
      case ZK_SCAN_END: c.assign = shut(ZF_SCAN); break;
      case ZK_PRECLIST: c.assign = open(ZF_PRECLIST); break;
      case ZK_PRECLIST_END: c.assign = shut(ZF_PRECLIST) | shut(ZF_PREC) | shut(ZF_SION); break;
      case ZK_PREC: c.n_prec = 1u, c.reset = 2u, c.assign = open(ZF_PREC) | shut(ZF_SION); break;
      case ZK_PREC_END: c.assign = shut(ZF_PREC) | shut(ZF_SION); break;
      case ZK_SION: c.n_sion = 1u, c.assign = open(ZF_SION); break;
      case ZK_SION_END: c.assign = shut(ZF_SION); break;
      case ZK_BDA: c.bda = 1u, c.assign = open(ZF_BDA); break;
      case ZK_BDA_END: c.assign = shut(ZF_BDA); break;
      default: break;
    }
    return c;
  }
  __device__ void store(int64_t L, MzCtx incl, MzCtx) const {
    rec[L] = incl.spec, slot[L] = incl.bda, dslot[L] = zm_pack(incl);
    if (L == n_tags - 1) *totals = incl;
  }
};

// The tables of a measured chunk, in one buffer of words. Per spectrum element s (stride ns): the tags that won;
// per array b (stride nb); per spectrum again, zeroed: counts and flags.
enum : uint32_t { S_FIRST = 0, S_CLOSE, S_LEVEL, S_RT, S_PMZ, S_Z, S_PZ, S_MZB, S_ITB, S_FIELDS };
enum : uint32_t { B_SPEC = 0, B_TYPE, B_PREC, B_COMP, B_BIN, B_FIELDS };
enum : uint32_t { Z_NPZ = 0, Z_ERR, Z_FIELDS };
struct MzTables {
  uint32_t *S, *B, *Z;
  uint32_t ns, nb;
  __device__ uint32_t &s(uint32_t f, uint32_t i) const { return S[(size_t)f * ns + i]; }
  __device__ uint32_t &b(uint32_t f, uint32_t i) const { return B[(size_t)f * nb + i]; }
  __device__ uint32_t &z(uint32_t f, uint32_t i) const { return Z[(size_t)f * ns + i]; }
};

// after_first: a <spectrum was seen before this chunk. cons: (tags << 32 | bytes) up to the last closed spectrum.
__global__ __launch_bounds__(SCAN_NT) void mzml_resolve_kernel(
    const uint8_t *__restrict__ kind, const uint8_t *__restrict__ dflag, const uint64_t *__restrict__ val,
    const uint32_t *__restrict__ aux, const uint32_t *__restrict__ line_start, const uint32_t *__restrict__ rec,
    const uint32_t *__restrict__ slot, const uint32_t *__restrict__ dslot, int64_t n_tags, int after_first,
    MzTables T, unsigned long long *__restrict__ cons, TextFinal *__restrict__ fin) {
  const int64_t L = (int64_t)blockIdx.x * SCAN_NT + threadIdx.x;
  if (L >= n_tags) return;
  const uint8_t k = kind[L];
  const uint32_t w = L > 0 ? dslot[L - 1] : 0u;       // the context in front of the tag
  const bool in = zm_in(w, ZF_SPEC);
  const uint32_t opened = rec[L];
  const auto error = [&](int e) { atomicMin(&fin->err, ((unsigned long long)L << 8) | (unsigned long long)e); };
  if (k == ZK_COMMENT && (opened > 0u || after_first != 0)) error(ASL_MZML_ERR_COMMENT);
  if (k == ZK_SPEC) {
    if (in) {
      error(ASL_MZML_ERR_NESTED);
    } else if (opened - 1u < T.ns) {
      T.s(S_FIRST, opened - 1u) = (uint32_t)L;
      if (dflag[L] & ZD_SELF) T.s(S_CLOSE, opened - 1u) = (uint32_t)L + 1u;
    }
    if (!in && (dflag[L] & ZD_SELF))
      atomicMax(cons, ((unsigned long long)(L + 1) << 32) | (unsigned long long)line_start[L + 1]);
    return;
  }
  if (!in) return;
  const uint32_t s = opened - 1u;   // (inside a spectrum: opened >= 1)
  if (s >= T.ns) return;            // (cannot happen: kept as the bound of every per-spectrum store)
  if (k == ZK_CUT) error(ASL_MZML_ERR_TAG);
  if (k == ZK_SPEC_END) {
    T.s(S_CLOSE, s) = (uint32_t)L + 1u;
    atomicMax(cons, ((unsigned long long)(L + 1) << 32) | (unsigned long long)line_start[L + 1]);
  }
  if (k == ZK_REF) atomicOr(&T.z(Z_ERR, s), (uint32_t)ASL_MZML_E_PARAM_GROUP);
  if (k == ZK_BDA) {
    const uint32_t b = slot[L] - 1u;
    if (b < T.nb) T.b(B_SPEC, b) = s;
    if (dflag[L] & ZD_ARRAY_LENGTH) atomicOr(&T.z(Z_ERR, s), (uint32_t)ASL_MZML_E_ARRAY_LENGTH);
  }
  const bool in_bda = zm_in(w, ZF_BDA);
  const uint32_t b = (L > 0 ? slot[L - 1] : 0u) - 1u;
  if (k == ZK_BIN && in_bda && b < T.nb) atomicMin(&T.b(B_BIN, b), (uint32_t)L);
  if (k != ZK_CV) return;
  const uint32_t cv = aux[L];
  const uint32_t n_scan = (w >> 8) & 3u, n_prec = (w >> 10) & 3u, n_sion = (w >> 12) & 3u;
  const bool first_scan = zm_in(w, ZF_SCANLIST) && zm_in(w, ZF_SCAN) && n_scan == 1u;
  const bool first_ion = zm_in(w, ZF_PRECLIST) && zm_in(w, ZF_PREC) && n_prec == 1u && zm_in(w, ZF_SION) && n_sion == 1u;
  const bool direct = !zm_in(w, ZF_SCANLIST) && !zm_in(w, ZF_PRECLIST) && !in_bda;
  if (cv == CV_LEVEL && direct) atomicMin(&T.s(S_LEVEL, s), (uint32_t)L);
  if (cv == CV_RT && first_scan) atomicMin(&T.s(S_RT, s), (uint32_t)L);
  if (first_ion) {
    if (cv == CV_PMZ) atomicMin(&T.s(S_PMZ, s), (uint32_t)L);
    if (cv == CV_Z) atomicMin(&T.s(S_Z, s), (uint32_t)L);
    if (cv == CV_PZ) atomicMin(&T.s(S_PZ, s), (uint32_t)L), atomicAdd(&T.z(Z_NPZ, s), 1u);   // (an integer count)
  }
  if (in_bda && b < T.nb) {
    if (cv == CV_MZ || cv == CV_IT) atomicMin(&T.b(B_TYPE, b), (uint32_t)L);
    if (cv == CV_F64 || cv == CV_F32 || cv == CV_BAD_PREC) atomicMin(&T.b(B_PREC, b), (uint32_t)L);
    if (cv == CV_PLAIN || cv == CV_ZLIB || cv == CV_BAD_COMP) atomicMin(&T.b(B_COMP, b), (uint32_t)L);
  }
  (void)val;
}

// which spectrum's m/z or intensity array is array b: the first of its kind wins
__global__ __launch_bounds__(SCAN_NT) void mzml_arrays_kernel(const uint32_t *__restrict__ aux, MzTables T) {
  const uint32_t b = blockIdx.x * SCAN_NT + threadIdx.x;
  if (b >= T.nb) return;
  const uint32_t s = T.b(B_SPEC, b), ty = T.b(B_TYPE, b);
  if (s >= T.ns || ty == NONE) return;
  atomicMin(&T.s(aux[ty] == CV_MZ ? S_MZB : S_ITB, s), b);
}

// per spectrum element: read or not (sel), its peak count (npk), its charge (zc), its errors
__global__ __launch_bounds__(SCAN_NT) void mzml_spectra_kernel(const uint64_t *__restrict__ val,
                                                             const uint32_t *__restrict__ aux, MzTables T,
                                                             uint32_t *__restrict__ sel, uint32_t *__restrict__ npk,
                                                             uint32_t *__restrict__ zc,
                                                             TextFinal *__restrict__ fin) {
  const uint32_t s = blockIdx.x * SCAN_NT + threadIdx.x;
  if (s >= T.ns) return;
  const uint32_t lt = T.s(S_LEVEL, s);
  const bool ms2 = T.s(S_CLOSE, s) != NONE && T.s(S_FIRST, s) != NONE && lt != NONE && (uint32_t)val[lt] == 2u;
  if (!ms2) {
    sel[s] = 0u, npk[s] = 0u, zc[s] = 0u;
    return;
  }
  uint32_t err = T.z(Z_ERR, s);
  uint32_t n = aux[T.s(S_FIRST, s)];
  if (n == NONE) err |= ASL_MZML_E_LENGTH, n = 0u;
  for (int j = 0; j < 2; ++j) {
    const uint32_t b = T.s(j == 0 ? S_MZB : S_ITB, s);
    if (b >= T.nb || T.b(B_BIN, b) == NONE) {
      err |= j == 0 ? ASL_MZML_E_NO_MZ : ASL_MZML_E_NO_INTENSITY;
      continue;
    }
    const uint32_t pt = T.b(B_PREC, b), ct = T.b(B_COMP, b);
    if (pt == NONE || aux[pt] == CV_BAD_PREC) err |= ASL_MZML_E_PRECISION;
    if (ct == NONE || aux[ct] == CV_BAD_COMP) err |= ASL_MZML_E_COMPRESSION;
  }
  if (T.s(S_RT, s) == NONE) err |= ASL_MZML_E_NO_RT;
  if (T.s(S_PMZ, s) == NONE) err |= ASL_MZML_E_NO_PRECURSOR;
  uint32_t z = 0u;
  const uint32_t zt = T.s(S_Z, s), np = T.z(Z_NPZ, s);
  if (zt != NONE || np == 1u) {
    z = (uint32_t)val[zt != NONE ? zt : T.s(S_PZ, s)];
    if (z < 1u || z > 255u) err |= ASL_MZML_E_CHARGE, z = 0u;
  } else if (np > 1u) {
    err |= ASL_MZML_E_CHARGES;
  }
  if (n > (uint32_t)ASL_MGF_MAX_PEAKS) atomicMin(&fin->cap_rec, s), n = 0u;
  T.z(Z_ERR, s) = err;
  sel[s] = 1u, npk[s] = n, zc[s] = z;
}

struct SlotView {   // ord[s]: MS2 spectra before s; pbeg[s]: their peaks
  using Op = MzPairOp;
  const uint32_t *sel, *npk;
  uint32_t *ord, *pbeg;
  MzPair *totals;
  int64_t ns;
  __device__ MzPair load(int64_t s) const { return MzPair{sel[s], npk[s]}; }
  __device__ void store(int64_t s, MzPair incl, MzPair own) const {
    ord[s] = incl.a - own.a, pbeg[s] = incl.b - own.b;
    if (s == ns - 1) *totals = incl;
  }
};

// ---------------------------------------------------------------------------------------------- fill
struct MzArray {   // one array of an MS2 spectrum
  uint32_t begin, end;   // its characters
  uint32_t slot, n;      // its values' first peak slot and their number
  uint32_t mode;         // 1 zlib, 2 64-bit, 4 not to be decoded (the spectrum has an error)
};

__global__ __launch_bounds__(SCAN_NT) void mzml_fill_spectra_kernel(
    const uint8_t *__restrict__ t, const uint32_t *__restrict__ line_start, const uint8_t *__restrict__ dflag,
    const uint64_t *__restrict__ val, const uint32_t *__restrict__ aux, MzTables T, const uint32_t *__restrict__ sel,
    const uint32_t *__restrict__ npk, const uint32_t *__restrict__ zc, const uint32_t *__restrict__ ord,
    const uint32_t *__restrict__ pbeg, uint32_t n_out, uint32_t n_text, int32_t *__restrict__ offsets,
    double *__restrict__ pmz, int32_t *__restrict__ pcharge, double *__restrict__ rt, int32_t *__restrict__ ident,
    int32_t *__restrict__ first, int32_t *__restrict__ element, int32_t *__restrict__ numerals,
    int32_t *__restrict__ errors, int32_t *__restrict__ flags, MzArray *__restrict__ arrays) {
  const uint32_t s = blockIdx.x * SCAN_NT + threadIdx.x;
  if (s >= T.ns || sel[s] == 0u) return;
  const uint32_t o = ord[s];
  if (o >= n_out) return;   // (cannot happen: n_out is the scan's total)
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const uint32_t ft = T.s(S_FIRST, s), err = T.z(Z_ERR, s);
  offsets[o] = (int32_t)pbeg[s];
  first[o] = (int32_t)ft, element[o] = (int32_t)s, errors[o] = (int32_t)err, pcharge[o] = (int32_t)zc[s];
  const uint64_t id = val[ft];
  ident[2 * (size_t)o] = (int32_t)(uint32_t)id, ident[2 * (size_t)o + 1] = (int32_t)(uint32_t)(id >> 32);
  double *const dst[2] = {rt, pmz};
  const uint32_t tag[2] = {T.s(S_RT, s), T.s(S_PMZ, s)};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    double v = nan;
    int32_t off = 0, len = -1;
    if (tag[j] != NONE) {
      if ((dflag[tag[j]] & ZD_DEFERRED) == 0) {
        v = __longlong_as_double((long long)val[tag[j]]);
      } else {   // the value's byte range: walked again, as mgf.hip walks a deferred line again
        const uint32_t a = line_start[tag[j]];
        const uint32_t e = zm_tag_end(t, a, min(line_start[tag[j] + 1], a + (uint32_t)ASL_MZML_MAX_TAG));
        uint32_t q = a + 1u, va, vb;
        while (q < e && !mg_ws(t[q]) && t[q] != '/') ++q;
        if (!zm_attr(t, q, e, "value", 5u, &va, &vb)) va = vb = e;
        off = (int32_t)va, len = (int32_t)(vb - va);
      }
    }
    dst[j][o] = v;
    numerals[4 * (size_t)o + 2 * j] = off, numerals[4 * (size_t)o + 2 * j + 1] = len;
  }
  uint32_t fl = 0u;
  for (int j = 0; j < 2; ++j) {
    MzArray A = {0u, 0u, pbeg[s], npk[s], 4u};
    const uint32_t b = T.s(j == 0 ? S_MZB : S_ITB, s);
    if (err == 0u && b < T.nb) {   // (err == 0: the array, its <binary>, its precision and compression exist)
      const uint64_t c = val[T.b(B_BIN, b)];
      A.begin = min((uint32_t)c, n_text), A.end = min((uint32_t)(c >> 32), n_text);
      A.mode = (aux[T.b(B_COMP, b)] == CV_ZLIB ? 1u : 0u) | (aux[T.b(B_PREC, b)] == CV_F64 ? 2u : 0u);
      fl |= (A.mode & 3u) << (2 * j);
    }
    arrays[2 * (size_t)o + j] = A;
  }
  flags[o] = (int32_t)fl;
}

// The other shape (ASL_MZML_DECODE=wave): one wavefront per array. PEAKS: the values the windows hold. LDS: out [PEAKS * 8] | in [IN] | tables | stage.
template <int PEAKS>
struct DecodeLds {
  static constexpr uint32_t OUT = PEAKS * 8u, IN = OUT + OUT / 8u + 64u, STAGE = 272u;
  static constexpr uint32_t BYTES = OUT + IN + (uint32_t)sizeof(InfWork) + STAGE + 16u;
  static_assert(IN % 16u == 0u && sizeof(InfWork) % 16u == 0u, "aligned parts");
};
template <int PEAKS>
__global__ __launch_bounds__(64) void mzml_decode_kernel(const uint8_t *__restrict__ t,
                                                       const MzArray *__restrict__ arrays, uint32_t n_arrays,
                                                       uint32_t n_peaks, float *__restrict__ mz,
                                                       float *__restrict__ intensity, int32_t *__restrict__ aerr) {
  using Lds = DecodeLds<PEAKS>;
  extern __shared__ __attribute__((aligned(16))) uint8_t mzml_lds[];
  uint8_t *const out = mzml_lds, *const in = out + Lds::OUT;
  InfWork *const work = reinterpret_cast<InfWork *>(in + Lds::IN);
  uint8_t *const stage = reinterpret_cast<uint8_t *>(work + 1);
  uint32_t *const result = reinterpret_cast<uint32_t *>(stage + Lds::STAGE);   // [0] error, [1] bytes
  const uint32_t a = blockIdx.x, lane = threadIdx.x;
  if (a >= n_arrays) return;
  const MzArray A = arrays[a];
  const bool small = A.n <= (uint32_t)ASL_MZML_SMALL_PEAKS;
  if (small != (PEAKS == ASL_MZML_SMALL_PEAKS)) return;          // the other launch's array
  if ((A.mode & 4u) != 0u || A.n > (uint32_t)PEAKS) {            // (A.n > PEAKS cannot happen: capacity is checked)
    if (lane == 0u) aerr[a] = 0;
    return;
  }
  const uint32_t width = (A.mode & 2u) ? 8u : 4u, expect = A.n * width;
  // base64 by the whole wave: 256 characters a round, the blanks squeezed out through a scan of the lanes' counts
  uint32_t carry = 0u, outpos = 0u, chars = 0u, first_pad = NONE, pads = 0u;
  int err = INF_OK;
  for (uint32_t base = A.begin; base < A.end; base += 256u) {
    uint8_t v[4];
    uint32_t cnt = 0u;
    bool bad = false;
    for (uint32_t k = 0; k < 4u; ++k) {
      const uint32_t i = base + 4u * lane + k;
      if (i < A.end) {
        const uint32_t x = b64_value(t[i]);
        if (x == B64_BAD) bad = true;
        else if (x != B64_BLANK) v[cnt++] = (uint8_t)x;
      }
    }
    uint32_t incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
      if ((int)lane >= d) incl += o;
    }
    const uint32_t tot = (uint32_t)__shfl((int)incl, 63, 64), excl = incl - cnt;
    for (uint32_t j = 0; j < cnt; ++j) {
      if (v[j] == B64_PAD) {
        first_pad = min(first_pad, chars + excl + j);
        ++pads;
      }
      stage[carry + excl + j] = v[j];   // (carry <= 3, tot <= 256: below STAGE)
    }
    if (__any(bad ? 1 : 0)) {
      err = INF_B64_BYTE;
      break;
    }
    __syncthreads();
    const uint32_t total = carry + tot, nq = total / 4u;
    if (outpos + 3u * nq > Lds::IN) {
      err = INF_INPUT;
      break;
    }
    for (uint32_t q = lane; q < nq; q += 64u) b64_quad(stage + 4u * q, in + outpos + 3u * q);
    __syncthreads();
    const uint32_t rem = total - 4u * nq;
    const uint8_t keep = lane < rem ? stage[4u * nq + lane] : (uint8_t)0;
    __syncthreads();
    if (lane < rem) stage[lane] = keep;
    __syncthreads();
    carry = rem, outpos += 3u * nq, chars += tot;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    first_pad = min(first_pad, (uint32_t)__shfl_xor((int)first_pad, d, 64));
    pads += (uint32_t)__shfl_xor((int)pads, d, 64);
  }
  uint32_t m = 0u;
  if (err == INF_OK) err = b64_finish(chars, pads != 0u ? first_pad : chars, pads, &m);   // (chars counts the carry)
  const uint8_t *src = in;
  if (err == INF_OK && (A.mode & 1u) != 0u) {
    // the symbol loop by one lane, from LDS to LDS
    if (m > expect + expect / 8u + 64u) {
      err = INF_INPUT;
    } else {
      __syncthreads();
      if (lane == 0u) {
        uint32_t got = 0u;
        result[0] = (uint32_t)inf_inflate(in, m, out, expect, &got, work);
        result[1] = got;
      }
      __syncthreads();
      err = (int)result[0];
      if (err == INF_OK && result[1] < expect) err = INF_LENGTH;
      src = out;
    }
  } else if (err == INF_OK) {
    err = m > expect ? INF_SINK : m < expect ? INF_LENGTH : INF_OK;
    __syncthreads();
  }
  if (err == INF_OK) {
    float *const dst = (a & 1u) ? intensity : mz;
    for (uint32_t i = lane; i < A.n; i += 64u) {
      const float f = width == 8u ? (float)*reinterpret_cast<const double *>(src + 8u * i)
                                  : *reinterpret_cast<const float *>(src + 4u * i);
      if (A.slot + i < n_peaks) dst[A.slot + i] = f;
    }
  }
  if (lane == 0u) aerr[a] = err;
}

// The default shape: one thread per array over windows in global scratch. Array a of a spectrum with n values from peak slot p has
// its out window at 8 (2 p + j n), its in window at 9 (2 p + j n) + 80 a (j = a & 1: the m/z or the intensity array)
// and its tables at index a: scratch for 2 n_peaks values and n_arrays arrays.
__global__ __launch_bounds__(64) void mzml_decode_thread_kernel(const uint8_t *__restrict__ t,
                                                              const MzArray *__restrict__ arrays, uint32_t n_arrays,
                                                              uint32_t n_peaks, uint8_t *__restrict__ out_all,
                                                              uint8_t *__restrict__ in_all,
                                                              InfWork *__restrict__ work_all, float *__restrict__ mz,
                                                              float *__restrict__ intensity,
                                                              int32_t *__restrict__ aerr) {
  const uint32_t a = blockIdx.x * 64u + threadIdx.x;
  if (a >= n_arrays) return;
  const MzArray A = arrays[a];
  const uint64_t first = 2ull * A.slot + (uint64_t)(a & 1u) * A.n;   // values in front of the array's, both columns
  if ((A.mode & 4u) != 0u || first + A.n > 2ull * n_peaks) {         // (beyond: cannot happen, the slots are a scan)
    aerr[a] = 0;
    return;
  }
  uint8_t *const out = out_all + 8ull * first, *const in = in_all + 9ull * first + 80ull * a;
  const uint32_t width = (A.mode & 2u) ? 8u : 4u, expect = A.n * width, limit = expect + expect / 8u + 64u;
  uint32_t m = 0u, got = 0u;
  int err = b64_decode(t + A.begin, A.end > A.begin ? A.end - A.begin : 0u, in, 9u * A.n + 80u, &m);   // (limit + 3 <= 9 n + 80)
  const uint8_t *src = in;
  if (err == INF_OK && (A.mode & 1u) != 0u) {
    err = m > limit ? INF_INPUT : inf_inflate(in, m, out, expect, &got, work_all + a);
    if (err == INF_OK && got < expect) err = INF_LENGTH;
    src = out;
  } else if (err == INF_OK) {
    err = m > expect ? INF_SINK : m < expect ? INF_LENGTH : INF_OK;
  }
  if (err == INF_OK) {
    float *const dst = (a & 1u) ? intensity : mz;
    for (uint32_t i = 0; i < A.n; ++i) {
      double d;
      float f;
      if (width == 8u) __builtin_memcpy(&d, src + 8u * i, 8), f = (float)d;   // (the in window is not 8-aligned)
      else __builtin_memcpy(&f, src + 4u * i, 4);
      if (A.slot + i < n_peaks) dst[A.slot + i] = f;
    }
  }
  aerr[a] = err;
}

namespace {

struct MzmlWork : ChunkWork<MzCtx> {
  DevBuf<uint8_t> scratch_out, scratch_in;
  DevBuf<InfWork> scratch_work;
  DevBuf<uint32_t> aux, tab, sel, npk, zc, ord, pbeg;
  DevBuf<MzPair> pair;
  DevBuf<MzArray> arrays;
  uint32_t n_open = 0, n_bda = 0;
  MzTables tables() {
    uint32_t *S = tab.p, *B = S + (size_t)S_FIELDS * n_open, *Z = B + (size_t)B_FIELDS * n_bda;
    return MzTables{S, B, Z, n_open, n_bda};
  }
};
MzmlWork &work() {
  static MzmlWork w;
  return w;
}

template <int PEAKS>
int launch_decode(const uint8_t *text, const MzArray *arrays, uint32_t n_arrays, uint32_t n_peaks, float *mz,
                  float *intensity, int32_t *aerr) {
  constexpr size_t lds = DecodeLds<PEAKS>::BYTES;
  HIP_TRY(hipFuncSetAttribute((const void *)mzml_decode_kernel<PEAKS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds));
  hipLaunchKernelGGL(mzml_decode_kernel<PEAKS>, dim3(n_arrays), dim3(64), lds, stream(), text, arrays, n_arrays,
                     n_peaks, mz, intensity, aerr);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

}  // namespace
}  // namespace asl

using namespace asl;

extern "C" int asl_mzml_inflate(const uint8_t *b64, int64_t n, int32_t zlib_flag, uint8_t *out, int64_t cap,
                                int64_t *n_out) {
  if ((b64 == nullptr && n > 0) || n < 0 || n >= ((int64_t)1 << 31) || cap < 0 || cap >= ((int64_t)1 << 31) ||
      (out == nullptr && cap > 0) || n_out == nullptr)
    return -1;
  std::vector<uint8_t> tmp((size_t)n / 4 * 3 + 3);
  InfWork w;
  uint32_t got = 0;
  uint8_t none = 0;
  const int rc = inf_array(b64 != nullptr ? b64 : &none, (uint32_t)n, zlib_flag, tmp.data(), (uint32_t)tmp.size(),
                           out != nullptr ? out : &none, (uint32_t)cap, &got, &w);
  *n_out = rc == INF_OK ? (int64_t)got : 0;
  return rc;
}

extern "C" int asl_mzml_measure(const uint8_t *text, int64_t n, int32_t last, int64_t *counts) {
  clear_error();
  MzmlWork &W = work();
  if (last < 0 || last > 3) return fail(ASL_ERR_INVALID, "mzml_measure: last = %d, bits 0 and 1", (int)last);
  const int after_first = (last >> 1) & 1;
  last &= 1;
  ASL_TRY(measure_begin("mzml", W, text, n, last, counts));
  counts[ASL_MZML_N_ELEMENTS] = counts[ASL_MZML_ERR_ELEMENT] = 0;
  W.n_open = W.n_bda = 0;
  if (n == 0) return ASL_OK;
  ProfScope ps("mzml_measure");
  int64_t nl = 0;   // >= 0
  ASL_TRY(line_starts<(uint8_t)'<'>(text, n, W.count, W.partial, W.line_start, &nl));
  ASL_TRY(measure_lines(W, std::max<int64_t>(nl, 1)));
  TextFinal F{~0ull, 0u, 0u, ~0u, ~0u};
  if (nl == 0) {   // no tag at all: nothing to consume but the bytes
    counts[ASL_MGF_CONSUMED] = 0;
    return measure_end("mzml", "spectrum", W, F, text, n, counts, "peaks");
  }
  // tags, context
  ASL_TRY(W.aux.reserve((size_t)nl));
  hipLaunchKernelGGL(mzml_tags_kernel, dim3(blocks_of(nl)), dim3(SCAN_NT), 0, stream(), text, W.line_start.p, nl,
                     (int)last, W.kind.p, W.dflag.p, W.val.p, W.aux.p, W.fin.p);
  ASL_CHECK_LAUNCH();
  ASL_TRY(scan_view(CtxView{W.kind.p, W.dflag.p, W.rec.p, W.slot.p, W.dslot.p, W.totals.p, nl}, nl, W.partial.p));
  MzCtx C;
  HIP_TRY(hipMemcpyAsync(&C, W.totals.p, sizeof(C), hipMemcpyDeviceToHost, stream()));
  ASL_TRY(sync_stream());
  // per spectrum and per array: the winning tags, the errors, the peak counts; then the slots
  const uint32_t ns = C.spec, nb = C.bda;
  const bool open = (C.assign & 3u) == 3u;
  W.n_open = ns, W.n_bda = nb;
  const size_t ones = (size_t)S_FIELDS * ns + (size_t)B_FIELDS * nb, zeros = (size_t)Z_FIELDS * ns;
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
  HIP_TRY(hipMemsetAsync(W.pair.p, 0, sizeof(MzPair), stream()));
  const MzTables T = W.tables();
  hipLaunchKernelGGL(mzml_resolve_kernel, dim3(blocks_of(nl)), dim3(SCAN_NT), 0, stream(), W.kind.p, W.dflag.p, W.val.p,
                     W.aux.p, W.line_start.p, W.rec.p, W.slot.p, W.dslot.p, nl, after_first, T, W.count.p, W.fin.p);
  ASL_CHECK_LAUNCH();
  if (nb > 0) {
    hipLaunchKernelGGL(mzml_arrays_kernel, dim3(blocks_of(nb)), dim3(SCAN_NT), 0, stream(), W.aux.p, T);
    ASL_CHECK_LAUNCH();
  }
  if (ns > 0) {
    hipLaunchKernelGGL(mzml_spectra_kernel, dim3(blocks_of(ns)), dim3(SCAN_NT), 0, stream(), W.val.p, W.aux.p, T,
                       W.sel.p, W.npk.p, W.zc.p, W.fin.p);
    ASL_CHECK_LAUNCH();
    ASL_TRY(scan_view(SlotView{W.sel.p, W.npk.p, W.ord.p, W.pbeg.p, W.pair.p, (int64_t)ns}, ns, W.partial.p));
  }
  MzPair P;
  unsigned long long cons = 0;
  HIP_TRY(hipMemcpyAsync(&P, W.pair.p, sizeof(P), hipMemcpyDeviceToHost, stream()));
  HIP_TRY(hipMemcpyAsync(&cons, W.count.p, sizeof(cons), hipMemcpyDeviceToHost, stream()));
  ASL_TRY(measure_final("mzml", W, &F, "tag", ASL_MZML_MAX_TAG));
  counts[ASL_MGF_N_LINES] = nl;
  counts[ASL_MGF_N_SPECTRA] = P.a;
  counts[ASL_MGF_N_PEAKS] = P.b;
  counts[ASL_MGF_N_DEFERRED] = 0;
  counts[ASL_MGF_CONSUMED] = (int64_t)(cons & 0xffffffffull);
  counts[ASL_MGF_CONSUMED_LINES] = (int64_t)(cons >> 32);
  counts[ASL_MGF_OPEN] = open ? 1 : 0;
  counts[ASL_MZML_N_ELEMENTS] = (int64_t)ns - (open ? 1 : 0);
  if (F.err != ~0ull) {
    uint32_t opened = 0;
    HIP_TRY(hipMemcpyAsync(&opened, W.rec.p + (F.err >> 8), sizeof(opened), hipMemcpyDeviceToHost, stream()));
    ASL_TRY(sync_stream());
    counts[ASL_MZML_ERR_ELEMENT] = opened;
  }
  return measure_end("mzml", "spectrum", W, F, text, n, counts, "peaks");
}

extern "C" int asl_mzml_fill(const uint8_t *text, int64_t n, int32_t *offsets, float *mz, float *intensity,
                             uint8_t *charge, double *precursor_mz, int32_t *precursor_charge,
                             double *retention_time, int32_t *identifier, int32_t *first_tag, int32_t *element,
                             int32_t *numerals, int32_t *errors, int32_t *flags, int32_t *array_errors) {
  clear_error();
  MzmlWork &W = work();
  ASL_TRY(fill_begin("mzml", W, text, n, offsets));
  const uint32_t ns = W.n_rec, np = W.n_peaks;
  if (ns == 0) return fill_empty(offsets);
  if ((np > 0 && (!mz || !intensity)) || !precursor_mz || !precursor_charge || !retention_time || !identifier ||
      !first_tag || !element || !numerals || !errors || !flags || !array_errors)
    return fail(ASL_ERR_INVALID, "mzml_fill: a null output");
  ASL_TRY(ensure_device());
  ProfScope ps("mzml_fill");
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
  ASL_TRY(oAe.init(array_errors, (size_t)ns * 2));
  ASL_TRY(W.arrays.reserve((size_t)ns * 2));
  if (oChg.d != nullptr) HIP_TRY(hipMemsetAsync(oChg.d, 0, np, stream()));
  HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(oOff.d + ns), (int)np, 1, stream()));
  hipLaunchKernelGGL(mzml_fill_spectra_kernel, dim3(blocks_of(W.n_open)), dim3(SCAN_NT), 0, stream(), text,
                     W.line_start.p, W.dflag.p, W.val.p, W.aux.p, W.tables(), W.sel.p, W.npk.p, W.zc.p, W.ord.p,
                     W.pbeg.p, ns, (uint32_t)n, oOff.d, oPmz.d, oZ.d, oRt.d, oId.d, oFirst.d, oEl.d, oNum.d, oErr.d,
                     oFl.d, W.arrays.p);
  ASL_CHECK_LAUNCH();
  // the arrays, in two launches by size: the small windows leave room for many waves a CU
  const char *shape = std::getenv("ASL_MZML_DECODE");
  if (shape == nullptr || std::strcmp(shape, "wave") != 0) {   // one thread per array: the faster of the two shapes
    ASL_TRY(W.scratch_out.reserve(std::max<size_t>((size_t)np * 16, 1)));
    ASL_TRY(W.scratch_in.reserve((size_t)np * 18 + (size_t)ns * 160));
    ASL_TRY(W.scratch_work.reserve((size_t)ns * 2));
    ProfScope pd("mzml_decode");
    hipLaunchKernelGGL(mzml_decode_thread_kernel, dim3((unsigned)cdiv(2 * (int64_t)ns, 64)), dim3(64), 0, stream(),
                       text, W.arrays.p, 2u * ns, np, W.scratch_out.p, W.scratch_in.p, W.scratch_work.p, oMz.d, oIt.d,
                       oAe.d);
    ASL_CHECK_LAUNCH();
  } else {
    ProfScope pd("mzml_decode");
    ASL_TRY(launch_decode<ASL_MZML_SMALL_PEAKS>(text, W.arrays.p, 2u * ns, np, oMz.d, oIt.d, oAe.d));
    ASL_TRY(launch_decode<ASL_MGF_MAX_PEAKS>(text, W.arrays.p, 2u * ns, np, oMz.d, oIt.d, oAe.d));
  }
  return finish_outputs(oOff, oMz, oIt, oChg, oPmz, oZ, oRt, oId, oFirst, oEl, oNum, oErr, oFl, oAe);
}
