// rescore.hip -- batched (shifted) dot-product rescoring.
// Replaces get_best_match (/root/reference/src/ann_solo/spectrum_match.pyx:28-108)
// and SpectrumMatcher::dot (/root/reference/src/ann_solo/SpectrumMatch.cpp:8-133).
//
// Pass 1a (rescore_flat_kernel): one workgroup per query. The query's peaks are hashed once
// into LDS (m/z bins of width 2*tol + a bitmap of occupied bins); the candidate list is
// filtered (precursor window, rescore.hpp) and compacted in LDS; a wave sets 32 candidates up
// one lane each and walks their peaks (m/z and fragment charge) as ONE stream, a peak per lane,
// testing the bitmap for every shift; the (peak, shift) items whose bin is marked are queued
// and probed -- hash walk, exact window / cursor predicate -- a full row of lanes at a time;
// a match is accumulated where it is found (LDS atomics: masks of matched peaks, exponent
// range, exact fp64 sum). Candidates with a doubly matched peak are marked -- unless, in a winner-only
// request, the sum of all their matches already shows that they cannot reach the query's best score
// (RS_PRUNED) -- and the queries that still have some are put on a work list for
// Pass 1b (rescore_score_v2_kernel, the pair kernel): two candidates per wave, one per
// half-wave, matches into per-half LDS lists keyed (product desc, generation order asc),
// resolved by a conflict-free fast path or a bitonic sort + scalar greedy loop. What neither
// takes (> 64 peaks or matches, > 100 query peaks, tol <= 0) goes to
// Pass 1c (rescore_score_kernel): one wave per (query, candidate) pair, lanes = query
// peaks, cursor by binary search (same cursor value as the reference's running cursor
// because both peak lists ascend).
// Pass 2 (rescore_argmax_kernel): per query first-strict-maximum (cpp:118-129).
// Pass 3 (rescore_matches_kernel): the winning pair is re-run once per winner to
// emit its peak_matches in greedy order.
// Ranked matches (asl_*_topn, asl_*_topn_distinct; n_best > 0 in the request): Pass 2 is
// rescore_topn_kernel (rescore_rank.hip), the n best slots per query in one pass over the scores, of n
// different groups where the library rows carry group ids; Pass 3 then runs over nq * n winners.
//
// Arithmetic mirrors the reference: window tests in double on float->double
// promoted m/z (cpp:42,53); product = (float)(mult * (double)q_int * (double)c_int)
// (cpp:81); score = double sum of those floats in sorted order (cpp:104).
#include <atomic>
#include <cstdlib>

#include "common.hpp"
#include "rescore_cand.hpp"

namespace asl {

constexpr int RS_WAVES = 4;
#ifndef RS_OCC
#define RS_OCC 7   // waves per SIMD the hash kernel is built for (A/B: -DRS_OCC=6)
#endif
constexpr int RS_MAXP = 256;   // peaks per spectrum the kernels accept
constexpr int RS_MCAP = 512;   // generated peak matches per pair the kernels accept

template <int MAXP_, int MCAP_>
struct WaveLdsT {
  static constexpr int MAXP = MAXP_, MCAP = MCAP_;
  float c_mz[MAXP_];
  float c_int[MAXP_];
  unsigned long long keys[MCAP_];
  uint32_t pay[MCAP_];
  uint8_t c_chg[MAXP_];
  uint8_t own_q[RS_MAXP];   // resolve fast path: last lane that claimed a query / candidate peak
  uint8_t own_c[RS_MAXP];
  int counter;
  int pad[3];
};
typedef WaveLdsT<RS_MAXP, RS_MCAP> WaveLds;

template <int MAXP_>
struct QueryLdsT {
  static constexpr int MAXP = MAXP_;
  float mz[MAXP_];
  float inten[MAXP_];
};
typedef QueryLdsT<RS_MAXP> QueryLds;

template <int CTRL>
__device__ __forceinline__ uint32_t rs_dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, false);
}

// max over the wave, in every lane (row butterflies on DPP, rows joined on the scalar unit)
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  v = max(v, rs_dpp<0xB1>(v));    // quad_perm [1,0,3,2]
  v = max(v, rs_dpp<0x4E>(v));    // quad_perm [2,3,0,1]
  v = max(v, rs_dpp<0x141>(v));   // row_half_mirror
  v = max(v, rs_dpp<0x140>(v));   // row_mirror
  const uint32_t a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
  const uint32_t c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
  return max(max(a, b), max(c, d));
}

template <int CTRL>
__device__ __forceinline__ double rs_dpp_d(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const uint32_t lo = rs_dpp<CTRL>((uint32_t)u), hi = rs_dpp<CTRL>((uint32_t)(u >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Sum over the wave in a fixed tree order; callers use it only where the sum is exact.
__device__ __forceinline__ double wave_sum_f64(double v) {
  v += rs_dpp_d<0xB1>(v);
  v += rs_dpp_d<0x4E>(v);
  v += rs_dpp_d<0x141>(v);
  v += rs_dpp_d<0x140>(v);
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)u, hi = (uint32_t)(u >> 32);
  double r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t l = __builtin_amdgcn_readlane(lo, 16 * i), h = __builtin_amdgcn_readlane(hi, 16 * i);
    r[i] = __longlong_as_double((long long)(((unsigned long long)h << 32) | l));
  }
  return (r[0] + r[1]) + (r[2] + r[3]);
}

// Sort the wave's match list (product desc, generation order asc) and assign greedily
// (SpectrumMatch.cpp:92-111). Lists of <= 64 matches are sorted in registers with
// cross-lane shuffles; longer ones in LDS. Returns the score in every lane.
template <bool EMIT, class WL>
__device__ double resolve_matches(int lane, WL &W, uint32_t *out_pairs, int out_cap,
                                  int *out_count, int *status, int kbase = 0, int m_in = -1,
                                  int mcap = RS_MCAP) {
  int M = m_in >= 0 ? m_in : W.counter;
  M = __builtin_amdgcn_readfirstlane(M);
  if (M > mcap) {
    if (lane == 0) atomicOr(status, RS_STATUS_MATCHES);
    M = mcap;
  }
  if (M == 0) return 0.0;
  unsigned long long *wkeys = W.keys + kbase;
  uint32_t *wpay = W.pay + kbase;
  unsigned long long rkey = 0ull;
  uint32_t rpay = 0;
  const bool small = M <= 64;
  if (small) {
    if (lane < M) {
      rkey = wkeys[lane];
      rpay = wpay[lane];
    }
    if (!EMIT && M > 1) {
      // Fast path: if no query peak and no candidate peak occurs twice, the greedy pass
      // accepts every match and the score is the plain sum of the products. The products
      // are fp32; when their exponents span <= 23 binades every partial sum of <= 64 of
      // them is exactly representable in fp64, so the sum does not depend on the order
      // and equals the reference's sorted accumulation bit for bit.
      const bool inl = lane < M;
      const uint32_t qi = (rpay >> 16) & (RS_MAXP - 1), ci = rpay & (RS_MAXP - 1);
      if (inl) {
        W.own_q[qi] = (uint8_t)lane;
        W.own_c[ci] = (uint8_t)lane;
      }
      wave_sync();
      const bool mine = !inl || (W.own_q[qi] == (uint8_t)lane && W.own_c[ci] == (uint8_t)lane);
      const uint32_t e = inl ? max((uint32_t)(rkey >> 55) & 0xffu, 1u) : 0u;
      const uint32_t emax = wave_max_u32(e);
      const bool exact = !inl || e + 23u >= emax;
      if (!__ballot(!(mine && exact)))
        return wave_sum_f64(inl ? (double)__uint_as_float((uint32_t)(rkey >> 32)) : 0.0);
    }
    if (M > 1) {
#pragma unroll
      for (int k = 2; k <= 64; k <<= 1) {
        if ((k >> 1) >= M) break;   // sorted runs of nextpow2(M) lanes suffice (wave-uniform)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
          const unsigned long long ok = __shfl_xor(rkey, j, 64);
          const uint32_t op = __shfl_xor(rpay, j, 64);
          const bool keep_max = (((lane & j) == 0) == ((lane & k) == 0));
          const bool take = ((ok > rkey) == keep_max) && (ok != rkey);
          rkey = take ? ok : rkey;
          rpay = take ? op : rpay;
        }
      }
    }
  } else {
    int P = 2;
    while (P < M) P <<= 1;
    for (int i = M + lane; i < P; i += 64) wkeys[i] = 0ull;
    wave_sync();
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = lane; t < (P >> 1); t += 64) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const int l = i | j;
          const unsigned long long a = wkeys[i], b = wkeys[l];
          const bool desc = (i & k) == 0;
          if (desc ? (a < b) : (a > b)) {
            wkeys[i] = b;
            wkeys[l] = a;
            const uint32_t pa = wpay[i];
            wpay[i] = wpay[l];
            wpay[l] = pa;
          }
        }
        wave_sync();
      }
    }
  }

  // greedy one-to-one assignment on the scalar unit
  unsigned long long qu0 = 0, qu1 = 0, qu2 = 0, qu3 = 0, cu0 = 0, cu1 = 0, cu2 = 0, cu3 = 0;
  double score = 0.0;
  int nm = 0;
  for (int t = 0; t < M; ++t) {
    uint32_t pl, pb;
    if (small) {
      pl = __builtin_amdgcn_readlane(rpay, t);
      pb = __builtin_amdgcn_readlane((uint32_t)(rkey >> 32), t);
    } else {
      pl = __builtin_amdgcn_readfirstlane(wpay[t]);
      pb = __builtin_amdgcn_readfirstlane((uint32_t)(wkeys[t] >> 32));
    }
    const uint32_t qi = pl >> 16, ci = pl & 0xffffu;
    const unsigned long long qbit = 1ull << (qi & 63), cbit = 1ull << (ci & 63);
    const uint32_t qw = qi >> 6, cw = ci >> 6;
    const unsigned long long qword = qw == 0 ? qu0 : qw == 1 ? qu1 : qw == 2 ? qu2 : qu3;
    const unsigned long long cword = cw == 0 ? cu0 : cw == 1 ? cu1 : cw == 2 ? cu2 : cu3;
    if (!(qword & qbit) && !(cword & cbit)) {
      score += (double)__uint_as_float(pb);
      if (qw == 0) qu0 |= qbit; else if (qw == 1) qu1 |= qbit; else if (qw == 2) qu2 |= qbit; else qu3 |= qbit;
      if (cw == 0) cu0 |= cbit; else if (cw == 1) cu1 |= cbit; else if (cw == 2) cu2 |= cbit; else cu3 |= cbit;
      if (EMIT) {
        if (lane == 0 && nm < out_cap) {
          out_pairs[2 * nm] = qi;
          out_pairs[2 * nm + 1] = ci;
        }
      }
      ++nm;
    }
  }
  if (EMIT && out_count && lane == 0) *out_count = nm;
  return score;
}

// Wave-cooperative SpectrumMatcher::dot for one pair. All 64 lanes call it with
// identical arguments; returns the score in every lane. EMIT: lane 0 writes the
// greedy (query_peak, candidate_peak) pairs.
// DEFER (the small-LDS instantiation of the matches kernel): a pair that does not fit the
// structures -- more candidate peaks or generated matches than they hold -- is not an error, the
// call returns -1 and the pair is left to the full-size instantiation.
// The fragment window of query peak qm. Da: `tol` itself. ppm (`ppm` != 0, wave-uniform): `tol` holds
// rel = fragment_mz_tolerance * 1e-6 and the window is relative to the QUERY peak, tol_i = rel * qm --
// one fp64 multiply (the build has -ffp-contract=off). qm - tol_i = qm (1 - rel) ascends with qm, so the
// reference's cursors still only advance. The shift gate (cpp:20) reads rs_frag_tol(tol, ppm, q_pmz).
__device__ __forceinline__ double rs_frag_tol(double tol, int ppm, double qm) { return ppm ? tol * qm : tol; }

template <bool EMIT, bool DEFER = false, class QL = QueryLds, class WL = WaveLds>
__device__ double dot_pair_wave(int lane, const QL &Q, int qn, double q_pmz,
                                const DevPeaks &L, int row, double tol, int ppm, int allow_shift,
                                WL &W, uint32_t *out_pairs, int out_cap, int *out_count,
                                int *status) {
  const int co = L.offsets[row];
  int cn = L.offsets[row + 1] - co;
  if (EMIT && out_count && lane == 0) *out_count = 0;
  if (cn > WL::MAXP) {
    if (DEFER) return -1.0;
    if (lane == 0) atomicOr(status, RS_STATUS_PEAKS);
    cn = WL::MAXP;
  }
  if (cn <= 0 || qn <= 0) return 0.0;
  for (int i = lane; i < cn; i += 64) {
    W.c_mz[i] = L.mz[co + i];
    W.c_int[i] = L.intensity[co + i];
    W.c_chg[i] = L.charge ? L.charge[co + i] : (uint8_t)0;
  }
  if (lane == 0) W.counter = 0;
  const int c_charge = L.precursor_charge[row];
  const double pmd = (q_pmz - L.precursor_mz[row]) * (double)(unsigned)c_charge;  // cpp:18
  const int S = (allow_shift && fabs(pmd) >= rs_frag_tol(tol, ppm, q_pmz)) ? c_charge + 1 : 1;   // cpp:20
  wave_sync();

  for (int qb = 0; qb < qn; qb += 64) {
    const int qi = qb + lane;
    if (qi < qn) {
      const double qm = (double)Q.mz[qi];
      const float q_int = Q.inten[qi];
      const double tl = rs_frag_tol(tol, ppm, qm);
      for (int s = 0; s < S; ++s) {
        const double md = s ? pmd / (double)s : 0.0;  // cpp:26-31
        // cursor = first j where NOT (qm - tol > c_mz[j] + md), capped at cn-1 (cpp:39-46)
        int lo = 0, hi = cn;
        const double lim = qm - tl;
        while (lo < hi) {
          int mid = (lo + hi) >> 1;
          if (lim > (double)W.c_mz[mid] + md)
            lo = mid + 1;
          else
            hi = mid;
        }
        int j = min(lo, cn - 1);
        // cpp:49-55
        while (j < cn && fabs(qm - ((double)W.c_mz[j] + md)) <= tl) {
          const int chg = W.c_chg[j];
          double mult = 0.0;
          if (s == 0 || chg == s)
            mult = 1.0;
          else if (chg == 0)
            mult = 2.0 / 3.0;
          if (mult > 0.0) {
            const float prod = (float)(mult * (double)q_int * (double)W.c_int[j]);  // cpp:81
            const int slot = atomicAdd(&W.counter, 1);
            if (slot < WL::MCAP) {
              const uint32_t gen = (uint32_t)((qi * S + s) * cn + j);
              W.keys[slot] = ((unsigned long long)__float_as_uint(prod) << 32) |
                             (unsigned long long)(0xFFFFFFFFu - gen);
              W.pay[slot] = ((uint32_t)qi << 16) | (uint32_t)j;
            }
          }
          ++j;
        }
      }
    }
  }
  wave_sync();
  if (DEFER && W.counter > WL::MCAP) return -1.0;     // (wave-uniform: the counter is final)
  return resolve_matches<EMIT>(lane, W, out_pairs, out_cap, out_count, status, 0, -1, WL::MCAP);
}

template <class QL>
__device__ __forceinline__ void load_query(int tid, int nthreads, const DevPeaks &Qs, int q,
                                           QL &Q, int &qn, int *status) {
  const int qo = Qs.offsets[q];
  qn = Qs.offsets[q + 1] - qo;
  if (qn > QL::MAXP) {
    if (tid == 0) atomicOr(status, RS_STATUS_PEAKS);
    qn = QL::MAXP;
  }
  for (int i = tid; i < qn; i += nthreads) {
    Q.mz[i] = Qs.mz[qo + i];
    Q.inten[i] = Qs.intensity[qo + i];
  }
}

constexpr int RS_BS_GROUP = 16;      // queries per workgroup of the binary-search kernel
__global__ __launch_bounds__(64 * RS_WAVES) void rescore_score_kernel(
    DevPeaks Qs, DevPeaks L, CandView cv, double tol, int ppm, int allow_shift,
    double *__restrict__ pair_score, const int *__restrict__ q_defer, int *status, int group) {
  __shared__ QueryLds Q;
  __shared__ WaveLds W[RS_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // A workgroup takes `group` (RS_BS_GROUP; 1 for small batches) consecutive queries: as the third launch of the rescoring the
  // kernel normally finds nothing marked -- one coalesced read of the group's flags says so (a
  // workgroup per query, 46 KB of LDS each, placed only to return, cost 0.02 ms of a step); when
  // every query is marked (tol <= 0, long queries) nq / 16 workgroups still fill the chip.
  // deferred mode: only the pairs the fast kernels marked RS_DEFER_BS (-3)
  __shared__ unsigned long long s_todo;
  const int q0 = blockIdx.x * group;
  if (wave == 0) {
    const int qt = q0 + lane;
    const unsigned long long m = __ballot(lane < group && qt < Qs.n && (!q_defer || (q_defer[qt] & 2)));
    if (lane == 0) s_todo = m;
  }
  __syncthreads();
  {
   unsigned long long todo = s_todo;          // workgroup-uniform
   while (todo) {
    const int q = q0 + __builtin_ctzll(todo);
    todo &= todo - 1ull;
    long long c0, c1;
    cv.range(q, c0, c1);
    if (c0 >= c1) continue;
    int qn;
    __syncthreads();              // the previous query's peaks are no longer read
    load_query(threadIdx.x, blockDim.x, Qs, q, Q, qn, status);
    __syncthreads();
    const double q_pmz = Qs.precursor_mz[q];
    const long long step = (long long)RS_WAVES * gridDim.y;
    for (long long c = c0 + (long long)blockIdx.y * RS_WAVES + wave; c < c1; c += step) {
      if (q_defer && pair_score[c] != -3.0) continue;
      const long long row = cv.cand(q, c, q_pmz, L.n);
      double s = -1.0;
      if (row >= 0)
        s = dot_pair_wave<false>(lane, Q, qn, q_pmz, L, (int)row, tol, ppm, allow_shift, W[wave],
                                 nullptr, 0, nullptr, status);
      if (lane == 0) pair_score[c] = s;
    }
   }
  }
}

// ---------------------------------------------------------------------------------
// Pass 1, fast path. The binary-search formulation above spends its time in dependent
// LDS round trips (6 per shift per query peak). Here the QUERY is hashed once per
// workgroup instead: every query peak is entered into an LDS hash table under the
// m/z bins of width 2*tol that its window [mz-tol, mz+tol] touches; a candidate peak at
// shifted position x can only match peaks filed under floor(x / (2*tol)). Lanes are the
// candidate's peaks, each does one independent probe per shift (a one-word Bloom-style
// bitmap rejects most probes), and the reference's exact window/cursor predicate is
// applied to the few hits:
//   match(i,j,s) <=> |q_i - x_j| <= tol and (not(q_i - tol > x_j) or j = n_c-1)
// and every peak between the cursor and j passes the window test (SpectrumMatch.cpp:39-55).
//
// Work distribution: the valid slots of the candidate list are compacted in LDS and dealt
// out evenly to the waves; a wave gathers 64 candidates' metadata at once, stages the
// peaks of RS_PF candidates per burst in LDS and scores them two at a time (one candidate
// per half-wave: an average library spectrum has ~27 peaks).
//
// The kernel only handles what fits its small LDS budget (4 workgroups per CU):
// candidates with <= 64 peaks and <= RS_HC generated matches, queries with <= RS_HQ_MAX
// peaks, tol > 0. Everything else is marked RS_DEFER and scored by the binary-search
// kernel in a second launch that skips queries with nothing deferred.
constexpr int RS_HT = 512;            // hash slots
constexpr int RS_HQ_MAX = 100;        // query peaks the hash path accepts (<= 3 bins each)
constexpr int RS_EMPTY = (int)0x80000000;
constexpr int RS_BM_BITS = 1 << 14;   // bin filter: <= 300 bits set of 16 384
constexpr int RS_SUPER = 1024;        // candidate slots compacted at a time
constexpr int RS_PF = 2;              // candidates staged per burst
constexpr int RS_HC = 64;             // matches per candidate resolved in this kernel
constexpr double RS_DEFER = -2.0;     // pair_score marker: left to the pair kernel (second launch)
constexpr double RS_DEFER_BS = -3.0;  // pair_score marker: left to the binary-search kernel (third launch)
// pair_score marker: a valid candidate whose score was not computed because it cannot reach the
// query's best score (winner-only requests: rescore_flat_kernel's epilogue). Counts as scored.
constexpr double RS_PRUNED = -4.0;
enum { RS_QD_PAIR = 1, RS_QD_BS = 2 };   // q_defer bits: the query has slots marked RS_DEFER / RS_DEFER_BS;
                                         // bits 2.. count the RS_DEFER slots (work split of the second launch)

// blocks of the second launch a query with n_defer slots marked RS_DEFER gets: one pair step per wave
__device__ __forceinline__ int rs_pair_blocks(int n_defer, int ymax) {
  const int want = (n_defer + 2 * RS_WAVES - 1) / (2 * RS_WAVES);
  return want < ymax ? want : ymax;
}
// appends a query's items to the second launch's work list (RescoreScratch: q_defer + nq is the count)
__device__ __forceinline__ int rs_append_items(int *__restrict__ q_defer, int nq, int q, int n_defer, int ymax) {
  const int ny = rs_pair_blocks(n_defer, ymax);
  if (ny <= 0) return 0;
  const int at = atomicAdd(&q_defer[nq], ny);
  int2 *items = reinterpret_cast<int2 *>(q_defer + ((nq + 2) & ~1));
  for (int y = 0; y < ny; ++y) items[at + y] = make_int2(q, y | (ny << 8));
  return ny;
}

// The bin filter's numeric envelope. The fast kernels compute the bin of a shifted candidate peak
// in fp32, b = floorf(fl(fl(cm + fl(md)) * fl(inv_w))) with inv_w = 1 / (2 tol), where the exact
// window test is done on x = cm + md in fp64. With u = 2^-24 (round to nearest, fp32) the three
// roundings are
//   fl(md)          = md + e1,                  |e1| <= u |md|        ((float)md)
//   fl(cm + fl(md)) = (x + e1) (1 + d2),        |d2| <= u             (the fp32 sum)
//   the product     = ... * inv_w (1 + d3) (1 + d4), |d3|, |d4| <= u  ((float)inv_w, the fp32 product)
// so, in bins, |b_fp32 - x inv_w| <= inv_w (u |md| + 3 u |x|) (1 + 3 u). A peak that matches query
// peak qm has |x| <= |qm| + tol, and |md| = |pmd / s| <= |pmd|: filing every query peak under the
// bins of [qm - tol, qm + tol] widened by
//   margin = 1e-3 + (0.5 / tol) * 6.0e-8 * (RS_MD_ENV + 3 (max|qm| + tol))          (6.0e-8 > u (1 + 3 u))
// on both sides covers every candidate with |pmd| <= RS_MD_ENV (the 1e-3 takes the fp64 rounding of
// the filing itself and fp32 underflow near zero). The accepted envelope is therefore
//   * per candidate: |pmd| <= RS_MD_ENV (4096: an open-search window of +-500 Da at any charge
//     the kernels take fits eight times), beyond it the candidate is marked RS_DEFER_BS;
//   * per query: margin <= RS_MARGIN_MAX with max|qm| its own largest peak (peaks ascend: the first
//     or the last), so that a peak still files under <= 3 bins (1 + 2 * 0.45 < 2 bin widths); beyond
//     it the whole query goes to the binary-search kernel, which has no filter. At m/z 2000 that is
//     tol >= 6.8e-4, at 20 000 tol >= 4.3e-3, at 100 000 tol >= 2.04e-2.
// Nothing is scored through a filter whose margin does not cover it; inside the envelope the
// bins, and so the exact test's inputs, are the same whatever the margin.
// ppm windows (rs_frag_tol: tol_i = rel * qm_i per query peak) keep LINEAR bins, of width 2 tol_max with
// tol_max = rel * (the query's largest m/z), the widest window of the query (rs_tol_max). A peak is
// filed under the bins of its own window [qm - tol_i, qm + tol_i] widened by the margin at tol_max.
// The argument above holds with tol := tol_max: a candidate peak that matches query peak i has
// |x| <= |qm_i| + tol_i <= max|qm| + tol_max, inv_w is 1 / (2 tol_max), so its fp32 bin lies within
// `margin` bins of x inv_w, which lies inside the filed interval; and since tol_i <= tol_max that
// interval spans (2 tol_i) / (2 tol_max) + 2 margin <= 1 + 0.9 < 2 bin widths: still <= 3 bins per peak
// (RS_HT holds them). Low-mass peaks, whose windows are narrower than a bin, share bins with
// non-matching positions more often: extra hits, which the exact test rejects. !(tol_max > 0) or a
// margin above RS_MARGIN_MAX defers the query as in Da mode (at m/z 2000 that is below 0.34 ppm).
// (The kernels take the margin from the query's peaks once they are in LDS: two loads from memory
// in front of the peak load, to decide first, were a dependent round trip per workgroup and cost the
// rescoring stage 0.08 ms of 2.1 at 32 768 queries -- profiles/rescore_envelope_ab.txt.)
constexpr double RS_MD_ENV = 4096.0;
constexpr double RS_MARGIN_MAX = 0.45;
// the widest fragment window of a query whose peaks ascend (Da: the tolerance itself)
__device__ __forceinline__ double rs_tol_max(float q_first, float q_last, double tol, int ppm) {
  return ppm ? tol * (double)fmaxf(q_first, q_last) : tol;
}
__device__ __forceinline__ double rs_bin_margin(float q_first, float q_last, double tol) {
  if (!(tol > 0.0)) return 1.0;
  const double q_abs = (double)fmaxf(fabsf(q_first), fabsf(q_last));
  return 1e-3 + (0.5 / tol) * 6.0e-8 * (RS_MD_ENV + 3.0 * (q_abs + tol));
}

struct QueryLds2 {   // hash path: at most RS_HQ_MAX query peaks
  float mz[128];
  float inten[128];
};

struct HashLds {
  int bin[RS_HT];
  uint32_t bm[RS_BM_BITS / 32];
  uint8_t peak[RS_HT];
};

struct PairLds {   // per wave
  float c_mz[RS_PF * 64];
  float c_int[RS_PF * 64];
  unsigned long long keys[2 * RS_HC];   // half A, half B
  uint32_t pay[2 * RS_HC];
  uint8_t c_chg[RS_PF * 64];
  uint8_t own_q[RS_MAXP];
  uint8_t own_c[RS_MAXP];
  double mdt[64];   // mass_diff[s] of half A (0..31) and half B (32..63)
  int counter;
  int pad[3];
};

// bit of a bin in the query's bin filter: the bin's low bits (bins 16 384 apart = 650 Da at the
// default tolerance share a bit; as dense as a multiplicative hash, without the quarter-rate multiply)
__device__ __forceinline__ uint32_t hbit(int b) { return (uint32_t)b & (uint32_t)(RS_BM_BITS - 1); }
__device__ __forceinline__ bool bm_test(const HashLds &H, int b) {
  const uint32_t bit = hbit(b);
  return (H.bm[bit >> 5] >> (bit & 31)) & 1u;
}

__device__ __forceinline__ uint32_t hbin(int b) {
  return ((uint32_t)b * 2654435761u) >> 23;  // 9 bits
}

__device__ __forceinline__ int rl_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ long long rl_ll(long long v, int l) {
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)(unsigned long long)v, l);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)((unsigned long long)v >> 32), l);
  return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double rl_d(double v, int l) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)u, l);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(u >> 32), l);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// Conflict-free resolve of BOTH half-wave match lists in one pass (each <= 32 matches):
// lanes 0-31 hold A's matches, lanes 32-63 B's; same test and same exact-sum argument as the
// fast path of resolve_matches, evaluated per half (row reductions on DPP, the two rows of a
// half joined on the scalar unit). ok bit 0 / 1: A / B resolved here (else the caller runs
// the general path for that half).
__device__ __forceinline__ int resolve_two_fast(int lane, PairLds &W, int MA, int MB,
                                                double &sA, double &sB) {
  const int half = lane >> 5, hl = lane & 31;
  const int M = half ? MB : MA;
  const bool inl = hl < M;
  unsigned long long key = 0ull;
  uint32_t pay = 0;
  if (inl) {
    key = W.keys[half * RS_HC + hl];
    pay = W.pay[half * RS_HC + hl];
  }
  // query peaks < 128 (RS_HQ_MAX) and candidate peaks < 64 on this path: one table per half
  const uint32_t qi = half * 128 + ((pay >> 16) & 127), ci = half * 128 + (pay & 127);
  if (inl) {
    W.own_q[qi] = (uint8_t)lane;
    W.own_c[ci] = (uint8_t)lane;
  }
  wave_sync();
  const bool mine = !inl || (W.own_q[qi] == (uint8_t)lane && W.own_c[ci] == (uint8_t)lane);
  uint32_t e = inl ? max((uint32_t)(key >> 55) & 0xffu, 1u) : 0u;
  uint32_t v = e;
  v = max(v, rs_dpp<0xB1>(v));
  v = max(v, rs_dpp<0x4E>(v));
  v = max(v, rs_dpp<0x141>(v));
  v = max(v, rs_dpp<0x140>(v));
  const uint32_t eA = max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16));
  const uint32_t eB = max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48));
  const bool exact = !inl || e + 23u >= (half ? eB : eA);
  const unsigned long long bad = __ballot(!(mine && exact));
  double x = inl ? (double)__uint_as_float((uint32_t)(key >> 32)) : 0.0;
  x += rs_dpp_d<0xB1>(x);
  x += rs_dpp_d<0x4E>(x);
  x += rs_dpp_d<0x141>(x);
  x += rs_dpp_d<0x140>(x);
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  const uint32_t lo = (uint32_t)u, hi = (uint32_t)(u >> 32);
  double r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t l = __builtin_amdgcn_readlane(lo, 16 * i), h = __builtin_amdgcn_readlane(hi, 16 * i);
    r[i] = __longlong_as_double((long long)(((unsigned long long)h << 32) | l));
  }
  sA = r[0] + r[1];
  sB = r[2] + r[3];
  return ((bad & 0xffffffffull) ? 0 : 1) | ((bad >> 32) ? 0 : 2);
}

// General resolve of one half's match list, out of line: it is the rare path, and inlined its
// loop-invariant lane predicates (bitonic directions) get hoisted into scalar registers that
// the hot loops of the kernel then spill around.
__device__ __attribute__((noinline)) double resolve_half_slow(int lane, PairLds &W, int *status,
                                                              int kbase, int M) {
  return resolve_matches<false>(lane, W, nullptr, 0, nullptr, status, kbase, M, RS_HC);
}

// Two candidates per wave: lanes 0-31 score candidate A, lanes 32-63 candidate B (peaks in
// passes of 32; cn = 0 leaves a half idle). The probing instruction stream -- the bulk of
// this instruction-bound kernel -- is shared by both. Per-half match lists live in the two
// halves of the wave's key buffer. A score of RS_DEFER means the half overflowed RS_HC.
__device__ __forceinline__ void score_two(int lane, const QueryLds2 &Q, const HashLds &H,
                                          PairLds &Wv, int slotA, int slotB, int cnA, int cnB,
                                          int chgA, int chgB, double pmzA, double pmzB,
                                          double q_pmz, double tol, int ppm, double inv_w, int allow_shift,
                                          int *status, double &scoreA, double &scoreB) {
  const int half = lane >> 5, hl = lane & 31;
  if (lane == 0) {
    Wv.pad[0] = 0;
    Wv.pad[1] = 0;
  }
  const double pmdA = (q_pmz - pmzA) * (double)(unsigned)chgA;          // cpp:18
  const double pmdB = (q_pmz - pmzB) * (double)(unsigned)chgB;
  const double gate = rs_frag_tol(tol, ppm, q_pmz);
  const int SA = (allow_shift && fabs(pmdA) >= gate) ? chgA + 1 : 1;     // cpp:20
  const int SB = (allow_shift && fabs(pmdB) >= gate) ? chgB + 1 : 1;
  const int slot = half ? slotB : slotA, cn = half ? cnB : cnA, S = half ? SB : SA;
  const double pmd = half ? pmdB : pmdA;
  const float *s_mz = Wv.c_mz + slot * 64;
  const float *s_in = Wv.c_int + slot * 64;
  const uint8_t *s_ch = Wv.c_chg + slot * 64;
  // mass_diff[s] = pmd / s (cpp:26-31): lane (32*half + s) performs its half's (expensive,
  // exact) fp64 division once and parks the quotient in LDS for the other lanes
  const int Smax = SA > SB ? SA : SB;
  {
    // x / 1 and x / 2 are exact scalings: precursor charges <= 2 (S <= 3) never need the fp64
    // division sequence (~40 VALU instructions every lane would execute per pair); the branch is
    // wave-uniform. Identical bits either way.
    double mdv = 0.0;
    if (Smax <= 3) {
      if (hl > 0 && hl < S) mdv = hl == 1 ? pmd : pmd * 0.5;
    } else if (hl > 0 && hl < S) {
      mdv = hl == 1 ? pmd : hl == 2 ? pmd * 0.5 : hl == 4 ? pmd * 0.25 : pmd / (double)hl;
    }
    Wv.mdt[lane] = mdv;
  }
  const float inv_w_f = (float)inv_w;
  const int cmax = cnA > cnB ? cnA : cnB;
  unsigned long long *keys = Wv.keys + half * RS_HC;
  uint32_t *pay = Wv.pay + half * RS_HC;
  wave_sync();
  for (int jb = 0; jb < cmax; jb += 32) {   // wave-uniform
    const int j = jb + hl;
    const bool act = j < cn;
    const float cm = act ? s_mz[j] : 0.0f, ci = act ? s_in[j] : 0.0f;
    const int cc = act ? s_ch[j] : 0;
    // shifts this peak takes part in (cpp:58-75): every s < S for an unannotated peak, else
    // s = 0 and s = its fragment charge
    const uint32_t smask = !act ? 0u : cc == 0 ? (1u << S) - 1u : (1u | (cc < S ? 1u << cc : 0u));
    for (int s = 0; s < Smax; ++s) {        // wave-uniform
      const double md = Wv.mdt[half * 32 + s];
      // bin of the shifted peak in fp32 (the query was filed with a margin that covers the
      // fp32 rounding: rs_bin_margin); bitmap reject first, the exact fp64 window test on the rare hits
      const bool can = (smask >> s) & 1u;
      const int b = (int)floorf((cm + (float)md) * inv_w_f);
      const bool maybe = can && bm_test(H, b);
      if (!__ballot(maybe)) continue;         // wave-uniform
      if (maybe) {
        const double mult = (s == 0 || cc == s) ? 1.0 : 2.0 / 3.0;
        uint32_t h = hbin(b);
        for (;;) {
          const int eb = H.bin[h];
          if (eb == RS_EMPTY) break;
          if (eb == b) {
            const int i = H.peak[h];
            const double x = (double)cm + md;
            const double qm = (double)Q.mz[i];
            const double tl = rs_frag_tol(tol, ppm, qm);
            const double lim = qm - tl;
            if (fabs(qm - x) <= tl && (!(lim > x) || j == cn - 1)) {
              // the reference walks from its cursor: every peak between the cursor and j
              // must pass the window test too (differs only on fp boundaries)
              bool run = true;
              for (int jj = j; jj > 0; --jj) {
                const double xp = (double)s_mz[jj - 1] + md;
                if (lim > xp) break;
                if (!(fabs(qm - xp) <= tl)) {
                  run = false;
                  break;
                }
              }
              if (run) {
                const float prod = (float)(mult * (double)Q.inten[i] * (double)ci);   // cpp:81
                const int mslot = atomicAdd(&Wv.pad[half], 1);
                if (mslot < RS_HC) {
                  const uint32_t gen = (uint32_t)((i * S + s) * cn + j);
                  keys[mslot] = ((unsigned long long)__float_as_uint(prod) << 32) |
                                (unsigned long long)(0xFFFFFFFFu - gen);
                  pay[mslot] = ((uint32_t)i << 16) | (uint32_t)j;
                }
              }
            }
          }
          h = (h + 1) & (RS_HT - 1);
        }
      }
    }
  }
  wave_sync();
  const int MA = __builtin_amdgcn_readfirstlane(Wv.pad[0]);
  const int MB = __builtin_amdgcn_readfirstlane(Wv.pad[1]);
  if (MA == 0 && MB == 0) {   // wave-uniform: nothing matched
    scoreA = scoreB = 0.0;
    return;
  }
  int ok = 0;
  if (MA <= 32 && MB <= 32) ok = resolve_two_fast(lane, Wv, MA, MB, scoreA, scoreB);
  if (!(ok & 1))
    scoreA = MA > RS_HC ? RS_DEFER
             : MA     ? resolve_half_slow(lane, Wv, status, 0, MA)
                      : 0.0;
  if (!(ok & 2))
    scoreB = MB > RS_HC ? RS_DEFER
             : MB     ? resolve_half_slow(lane, Wv, status, RS_HC, MB)
                      : 0.0;
}

// FORM: the shapes the search path calls with -- fixed-stride neighbour lists (1: int32
// rows, 2: int64 rows), packed row records for the precursor filter, annotated library peaks;
// 3: the window-only modes' CSR runs of the precursor-sorted view (CandView::win_begin) --
// are compiled with those facts folded in (each open "is this pointer null" question is a
// wave-uniform predicate held in scalar registers across the hot loops); 0 = any shape but 3.
// The kernel is the SECOND LAUNCH behind rescore_flat_kernel: it scores only the slots that kernel
// marked RS_DEFER; what it cannot resolve either goes on to the binary-search kernel (RS_DEFER_BS /
// RS_QD_BS). Its work is the list the first launch left in q_defer (RescoreScratch): an item is
// (query, y, ny) -- a query's deferred slots are few (a handful: one item) or nearly all of its
// candidates (two query peaks closer than the tolerance make every candidate with a peak there a
// conflict: up to RS_DEF_Y items, block y takes the slots of every ny-th group of 32). The grid is
// as many blocks as the device holds at once; block b walks items b, b + gridDim.x, ...
//
// One item. The block's LDS structures are rebuilt per item (the caller puts a barrier in between).
template <int FORM>
__device__ __forceinline__ void pair_item(const int q, const int y, const int ny, const DevPeaks &Qs,
                                          const DevPeaks &L, const CandView &cv, const double tol, const int ppm,
                                          const int allow_shift, double *__restrict__ pair_score,
                                          int *__restrict__ q_defer, int *status, QueryLds2 &Q, HashLds &H,
                                          PairLds (&W)[RS_WAVES], uint16_t (&s_list)[RS_SUPER], int &s_nv,
                                          int &s_defer) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  long long c0, c1;
  cv.range(q, c0, c1);
  if (c0 >= c1) return;
  const int qo = Qs.offsets[q];
  const int qn = Qs.offsets[q + 1] - qo;
  const double q_pmz = Qs.precursor_mz[q];
  // fp32 evaluation of a probe bin: its error bound in bin units (rs_bin_margin); the query
  // peaks are filed with that margin on both sides (still <= 3 bins per peak)
  // (the first launch applies the same tests and sends such a query to the binary-search kernel
  // whole, so none is on the work list; should one be, its deferred slots follow)
  auto defer_query = [&]() {      // uniform
    for (long long c = c0 + (long long)y * blockDim.x + tid; c < c1; c += (long long)blockDim.x * ny) {
      if (pair_score[c] == RS_DEFER) pair_score[c] = RS_DEFER_BS;
    }
    if (tid == 0) atomicOr(&q_defer[q], RS_QD_BS);
  };
  if (!(tol > 0.0) || qn > RS_HQ_MAX) {
    defer_query();
    return;
  }
  for (int i = tid; i < qn; i += blockDim.x) {   // qn <= RS_HQ_MAX here
    Q.mz[i] = Qs.mz[qo + i];
    Q.inten[i] = Qs.intensity[qo + i];
  }
  for (int i = tid; i < RS_HT; i += blockDim.x) H.bin[i] = RS_EMPTY;
  for (int i = tid; i < RS_BM_BITS / 32; i += blockDim.x) H.bm[i] = 0u;
  if (tid == 0) s_defer = 0;
  __syncthreads();
  // the margin of this query's own m/z range, from the peaks just loaded (no extra trip to memory
  // in front of the load); beyond RS_MARGIN_MAX the query leaves the hash path (uniform)
  // (ppm: linear bins of the query's widest window, tol_max -- see rs_bin_margin)
  const double tol_max = qn > 0 ? rs_tol_max(Q.mz[0], Q.mz[qn - 1], tol, ppm) : tol;
  const double margin = qn > 0 ? rs_bin_margin(Q.mz[0], Q.mz[qn - 1], tol_max) : 0.0;
  if (!(margin <= RS_MARGIN_MAX)) {
    defer_query();
    return;
  }
  const double inv_w = 1.0 / (2.0 * tol_max);
  if (tid < qn) {
    const double qm = (double)Q.mz[tid];
    const double tl = rs_frag_tol(tol, ppm, qm);
    // (tol_i <= tol_max for ascending peaks; the clamp keeps a spectrum that breaks that rule at <= 3
    // bins per peak, which is what the table is sized for)
    const double tf = fmin(tl, tol_max);
    const int blo = (int)floor((qm - tf) * inv_w - margin);
    const int bhi = (int)floor((qm + tf) * inv_w + margin);
    for (int b = blo; b <= bhi; ++b) {
      const uint32_t bit = hbit(b);
      atomicOr(&H.bm[bit >> 5], 1u << (bit & 31));
      uint32_t h = hbin(b);
      for (;;) {
        const int old = atomicCAS(&H.bin[h], RS_EMPTY, b);
        if (old == RS_EMPTY) {
          H.peak[h] = (uint8_t)tid;
          break;
        }
        h = (h + 1) & (RS_HT - 1);
      }
    }
  }
  __syncthreads();
  PairLds &Wv = W[wave];
  const int parts = RS_WAVES, part = wave;

  for (long long sb = c0; sb < c1; sb += RS_SUPER) {
    // ---- compact the valid slots of this super-chunk (order is irrelevant: scores are
    // written back to their slots)
    const int sn = (int)((c1 - sb) < RS_SUPER ? (c1 - sb) : RS_SUPER);
    if (tid == 0) s_nv = 0;
    __syncthreads();
    for (int i0 = 0; i0 < sn; i0 += blockDim.x) {
      const int i = i0 + tid;
      bool ok = false;
      if (i < sn) {
        ok = pair_score[sb + i] == RS_DEFER;     // a valid candidate: the first launch checked
        // several blocks per query: each takes the slots of every ny-th group of 32 (the order
        // inside s_list depends on the waves' timing, so blocks must not split it by position)
        ok = ok && (ny == 1 || ((i >> 5) % ny) == y);
      }
      const unsigned long long bal = __ballot(ok);
      int wbase = 0;
      if (lane == 0 && bal) wbase = atomicAdd(&s_nv, __popcll(bal));
      wbase = rl_i(wbase, 0);
      if (ok) s_list[wbase + __popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)i;
    }
    __syncthreads();
    const int nv = s_nv;
    const int per = (nv + parts - 1) / parts;
    const int wb = part * per;
    const int we = wb + per < nv ? wb + per : nv;

    for (int base = wb; base < we; base += 64) {
      const bool okr = base + lane < we;
      const int slot = okr ? (int)s_list[base + lane] : 0;   // candidate slot = sb + slot
      int m_co = 0, m_cn = 0, m_chg = 0;
      double m_pmz = 0.0;
      if (okr) {
        const long long row = cv.row(q, sb + slot);
        if (cv.flt.meta) {     // one 32-byte sector per candidate
          const RowMeta *mr = meta_row(cv.flt, row);
          const uint4 a = *reinterpret_cast<const uint4 *>(mr);
          m_co = (int)a.x;
          m_cn = (int)a.y;
          m_chg = (int)a.z;
          m_pmz = mr->pmz64;
        } else {
          m_co = L.offsets[row];
          m_cn = L.offsets[row + 1] - m_co;
          m_chg = L.precursor_charge[row];
          m_pmz = L.precursor_mz[row];
        }
      }
      // a shifted candidate beyond the bin filter's envelope (RS_MD_ENV) is not scored here
      const int m_far = (allow_shift && !(fabs((q_pmz - m_pmz) * (double)(unsigned)m_chg) <= RS_MD_ENV)) ? 1 : 0;
      double my_score = 0.0;
      const int cnt = we - base < 64 ? we - base : 64;
      // Bursts of RS_PF candidates: all their peak loads are issued back to back (straight
      // line, so hipcc keeps them in flight together), parked in this wave's LDS staging
      // area, and the candidates are then scored from LDS with no global load in the way.
      for (int g0 = 0; g0 < cnt; g0 += RS_PF) {
        float fm[RS_PF], fi[RS_PF];
        int fc[RS_PF];
#pragma unroll
        for (int u = 0; u < RS_PF; ++u) {
          const int l = g0 + u < cnt ? g0 + u : cnt - 1;
          const int co = rl_i(m_co, l), cn = rl_i(m_cn, l);
          const bool ld = lane < cn && g0 + u < cnt;
          fm[u] = ld ? L.mz[co + lane] : 0.0f;
          fi[u] = ld ? L.intensity[co + lane] : 0.0f;
          fc[u] = (ld && L.charge) ? L.charge[co + lane] : 0;
        }
#pragma unroll
        for (int u = 0; u < RS_PF; ++u) {
          Wv.c_mz[u * 64 + lane] = fm[u];
          Wv.c_int[u * 64 + lane] = fi[u];
          Wv.c_chg[u * 64 + lane] = (uint8_t)fc[u];
        }
        wave_sync();
#pragma unroll
        for (int u = 0; u < RS_PF; u += 2) {
          const int lA = g0 + u, lB = g0 + u + 1;
          const bool vA = lA < cnt, vB = lB < cnt;   // wave-uniform
          const int cnA = vA ? rl_i(m_cn, lA) : 0, cnB = vB ? rl_i(m_cn, lB) : 0;
          const int chA = vA ? rl_i(m_chg, lA) : 0, chB = vB ? rl_i(m_chg, lB) : 0;
          const bool defA = cnA > 64 || chA >= 31 || (vA && rl_i(m_far, lA));
          const bool defB = cnB > 64 || chB >= 31 || (vB && rl_i(m_far, lB));
          const bool runA = vA && !defA && cnA > 0 && qn > 0;
          const bool runB = vB && !defB && cnB > 0 && qn > 0;
          double sA = 0.0, sB = 0.0;
          if (runA || runB) {
            score_two(lane, Q, H, Wv, u, u + 1, runA ? cnA : 0, runB ? cnB : 0, chA, chB,
                      rl_d(m_pmz, vA ? lA : 0), rl_d(m_pmz, vB ? lB : 0), q_pmz, tol, ppm, inv_w,
                      allow_shift, status, sA, sB);
          }
          if (defA || sA == RS_DEFER) sA = RS_DEFER_BS;
          if (defB || sB == RS_DEFER) sB = RS_DEFER_BS;
          if (vA && lane == lA) my_score = sA;
          if (vB && lane == lB) my_score = sB;
        }
        wave_sync();
      }
      if (okr) pair_score[sb + slot] = my_score;
      if (__ballot(okr && my_score == RS_DEFER_BS) && lane == 0) s_defer = 1;
    }
    __syncthreads();   // s_list is rebuilt for the next super-chunk
  }
  if (tid == 0 && s_defer) atomicOr(&q_defer[q], RS_QD_BS);
}

template <int FORM>
__global__ __launch_bounds__(64 * RS_WAVES, RS_OCC) void rescore_score_v2_kernel(
    DevPeaks Qs, DevPeaks L, CandView cv, double tol, int ppm, int allow_shift,
    double *__restrict__ pair_score, int *__restrict__ q_defer, int *status) {
  cv.flt.wcol = nullptr;      // this kernel wants filter column and metadata from ONE gather
  if (FORM != 3) cv.win_begin = nullptr;
  if (FORM == 3) {            // window-only lists: a run of the precursor-sorted view per query
    cv.rows64 = nullptr;
    cv.rows32 = nullptr;
    cv.counts = nullptr;
    cv.flt.lib_pmz = nullptr;
    cv.flt.valid = nullptr;
    cv.flt.pass_all = true;
    __builtin_assume(cv.offsets != nullptr);
    __builtin_assume(cv.win_begin != nullptr);
    __builtin_assume(cv.flt.meta != nullptr);
    __builtin_assume(L.charge != nullptr);
  } else if (FORM != 0) {
    cv.offsets = nullptr;
    cv.flt.lib_pmz = nullptr;
    cv.flt.valid = nullptr;
    __builtin_assume(cv.flt.meta != nullptr);
    __builtin_assume(L.charge != nullptr);
    if (FORM == 1) {
      cv.rows64 = nullptr;
    } else {
      __builtin_assume(cv.rows64 != nullptr);
    }
  }
  __shared__ QueryLds2 Q;
  __shared__ HashLds H;
  __shared__ PairLds W[RS_WAVES];
  __shared__ uint16_t s_list[RS_SUPER];
  __shared__ int s_nv, s_defer;
  const int nq = Qs.n;
  // (block-uniform values, said so: the query and all that follows from it stay in scalar registers)
  const int n_items = __builtin_amdgcn_readfirstlane(q_defer[nq]);
  const int2 *items = reinterpret_cast<const int2 *>(q_defer + ((nq + 2) & ~1));
  for (int it = (int)blockIdx.x; it < n_items; it += (int)gridDim.x) {
    if (it != (int)blockIdx.x) __syncthreads();      // the previous item's tables are no longer read
    const int2 w = items[it];
    const int wq = __builtin_amdgcn_readfirstlane(w.x), wy = __builtin_amdgcn_readfirstlane(w.y);
    pair_item<FORM>(wq, wy & 0xff, wy >> 8, Qs, L, cv, tol, ppm, allow_shift, pair_score, q_defer, status, Q, H, W,
                    s_list, s_nv, s_defer);
  }
}

// ---------------------------------------------------------------------------------
// Pass 1, FLAT formulation (the first launch of the search path). The pair kernel above spends
// two thirds of its instructions outside the probing loop: per pair of candidates it stages
// peaks through LDS, sets up shifts and tables with every lane, and resolves two match lists
// with DPP trees. Here a wave takes RF_NC candidates at a time and
//   * SETS THEM UP ONE LANE PER CANDIDATE (row record, shift count, mass-difference table,
//     zeroed accumulators, a prefix sum of the peak counts),
//   * walks their peaks as ONE STREAM, one candidate peak per lane whatever candidate it
//     belongs to (an owner table maps stream positions to candidates; peaks are loaded straight
//     from HBM a step ahead, no LDS staging), probing the query's bin bitmap / hash per shift
//     exactly like the pair kernel,
//   * and ACCUMULATES a match where it is found: atomicOr into the candidate's masks of matched
//     query / candidate peaks (a bit that was already set = a doubly matched peak), atomic
//     min / max of the product's exponent, and an fp64 atomic add of the product.
// If no peak was matched twice the reference's greedy pass accepts every match, and if the
// products span <= 23 binades the fp64 sum of <= 64 fp32 products is exact in ANY order
// (24 + 23 + 6 = 53 bits): the accumulated sum IS the reference's sorted sum, bit for bit.
// Anything else -- a doubly matched peak, a wider span, more shifts than the table holds -- is
// marked RS_DEFER for the pair kernel (second launch, ~2 % of the candidates); what that
// kernel does not take either (> 64 peaks, > 64 matches, query > 100 peaks, tol <= 0) goes to
// the binary-search kernel as RS_DEFER_BS.
constexpr int RF_NC = 32;        // candidates per wave chunk (set-up lanes)
constexpr int RF_PMAX = 1024;    // candidate peaks per wave chunk (owner table)
constexpr int RF_SMAX = 5;       // shifts the mass-difference table holds (precursor charge <= 4)
constexpr int RF_MQ = 128;       // (peak, shift) items queued per wave before a drain

struct FlatLds {   // per wave
  double sum[RF_NC];
  double pmd[RF_NC];
  float mdf[RF_NC][RF_SMAX - 1];   // (float)(pmd / s), s = 1..4: the probe bins
  uint32_t qmask[RF_NC][4];        // matched query peaks (<= 128 on this path)
  uint32_t cmask[RF_NC][2];        // matched candidate peaks (<= 64)
  uint32_t emax[RF_NC];            // largest exponent byte of a product | bit 31: doubly matched peak
  uint32_t emin[RF_NC];
  // where a candidate's peaks are: the address of its peak record, or (no records) its first peak
  // in the library arrays
  unsigned long long cptr[RF_NC];
  // bits 0-23: rf_key(candidate, shifts) - first stream position, so that adding a stream position
  // gives the peak's key (modulo 2^16); bits 24-31: peaks
  uint32_t ckey[RF_NC];
  uint8_t owner[RF_PMAX];
  uint16_t mq[RF_MQ];              // queued (peak of its candidate | candidate << 6 | shift << 11) items whose bin is marked
};

// (a peak record's address comes out of LDS as a number: these say that it is global memory)
using gfloat_p = const __attribute__((address_space(1))) float *;
using gbyte_p = const __attribute__((address_space(1))) uint8_t *;
// What a stream step and a queued item need to know of a peak's candidate, in 16 bits: the peak's
// index in the candidate (< 64) | the candidate's lane << 6 | the shifts it probes, as the bits
// below S (S <= RF_SMAX), << 11.
__device__ __forceinline__ uint32_t rf_key(int t, int S) { return ((uint32_t)t << 6) | (((1u << S) - 1u) << 11); }

// Winner-only requests (`prune`, one block per query): a candidate deferred for a doubly matched
// peak or a wide exponent span still has, in sum[], the sum of ALL its generated matches -- an upper
// bound of its score, which is the sum of a subset of the same non-negative products (DESIGN.md
// section 3). Such candidates are listed in LDS with their bounds instead of being marked at once; the
// block keeps the maximum of the exact scores it writes, and after the last chunk a listed candidate
// whose bound lies below that maximum (by more than the rounding of the two sums: RS_PRUNE_REL /
// _ABS) becomes RS_PRUNED, the others RS_DEFER. A candidate the list has no room for, one with a
// negative or NaN product (emax bit 30: the subset argument needs products >= 0), and one deferred
// before anything was accumulated (def_pair, def_bs) are never pruned.
// The epilogue also puts the query's surviving deferred slots on the second launch's work list.
constexpr int RF_DLIST = 256;    // deferred candidates per query that can be pruned
constexpr double RS_PRUNE_REL = 1e-9, RS_PRUNE_ABS = 1e-12;
constexpr int RF_OCC = 6;      // waves per SIMD: 80 VGPRs (7 / 8: 72 / 64 VGPRs and more spills: +2 % / +12 %, profiles/r03_rescore_ab.txt)
template <int FORM>
__global__ __launch_bounds__(64 * RS_WAVES, RF_OCC) void rescore_flat_kernel(
    DevPeaks Qs, DevPeaks L, CandView cv, double tol, int ppm, int allow_shift,
    double *__restrict__ pair_score, int *__restrict__ q_defer, int *status, int prune, int ymax,
    unsigned long long *__restrict__ counts) {
  if (FORM != 3) cv.win_begin = nullptr;
  if (FORM == 3) {            // window-only lists: a run of the precursor-sorted view per query
    cv.rows64 = nullptr;
    cv.rows32 = nullptr;
    cv.counts = nullptr;
    cv.flt.lib_pmz = nullptr;
    cv.flt.valid = nullptr;
    cv.flt.wcol = nullptr;
    cv.flt.pass_all = true;
    __builtin_assume(cv.offsets != nullptr);
    __builtin_assume(cv.win_begin != nullptr);
    __builtin_assume(cv.flt.meta != nullptr);
    __builtin_assume(L.charge != nullptr);
    __builtin_assume(L.records != nullptr);
  } else if (FORM != 0) {
    cv.offsets = nullptr;
    cv.flt.lib_pmz = nullptr;
    cv.flt.valid = nullptr;
    __builtin_assume(cv.flt.meta != nullptr);
    __builtin_assume(cv.flt.wcol != nullptr);
    __builtin_assume(L.charge != nullptr);
    __builtin_assume(L.records != nullptr);
    if (FORM == 1) {
      cv.rows64 = nullptr;
    } else {
      __builtin_assume(cv.rows64 != nullptr);
    }
  }
  __shared__ QueryLds2 Q;
  __shared__ HashLds H;
  __shared__ FlatLds W[RS_WAVES];
  __shared__ uint16_t s_list[RS_SUPER];
  __shared__ int s_nv, s_defer, s_ndef, s_nlist, s_npruned;
  __shared__ unsigned long long s_best;      // largest exact score written (>= 0: orders as u64)
  __shared__ double s_dbound[RF_DLIST];
  __shared__ uint32_t s_dslot[RF_DLIST];     // the listed candidate's slot - c0
  // the window of every query peak (rs_frag_tol; Da: the one tolerance), worked out once at the filing:
  // the drain reads it beside the peak, and neither the tolerance nor the mode stays in registers
  // across the stream loop
  __shared__ double s_qtol[RS_HQ_MAX];
  const int q = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  long long c0, c1;
  cv.range(q, c0, c1);
  if (c0 >= c1) return;
  const int qo = Qs.offsets[q];
  const int qn = Qs.offsets[q + 1] - qo;
  const double q_pmz = Qs.precursor_mz[q];
  const double gate = rs_frag_tol(tol, ppm, q_pmz);      // the shift gate's threshold (cpp:20)
  // the row was filtered where it was made (block-uniform): every slot in range is a candidate
  const bool pre = cv.prefiltered(q);
  auto is_cand = [&](long long c) -> bool {
    if (pre) {
      const long long r = cv.row(q, c);
      return r >= 0 && r < L.n;
    }
    return cv.cand(q, c, q_pmz, L.n) >= 0;
  };
  // (same bin filter as the pair kernel: see there)
  auto defer_query = [&]() {      // uniform: the whole query goes to the binary-search kernel
    for (long long c = c0 + (long long)blockIdx.y * blockDim.x + tid; c < c1;
         c += (long long)blockDim.x * gridDim.y) {
      pair_score[c] = is_cand(c) ? RS_DEFER_BS : -1.0;
    }
    if (tid == 0) atomicOr(&q_defer[q], RS_QD_BS);
  };
  if (!(tol > 0.0) || qn > RS_HQ_MAX) {
    defer_query();
    return;
  }
  for (int i = tid; i < qn; i += blockDim.x) {
    Q.mz[i] = Qs.mz[qo + i];
    Q.inten[i] = Qs.intensity[qo + i];
  }
  for (int i = tid; i < RS_HT; i += blockDim.x) H.bin[i] = RS_EMPTY;
  for (int i = tid; i < RS_BM_BITS / 32; i += blockDim.x) H.bm[i] = 0u;
  if (tid == 0) {
    s_defer = s_ndef = s_nlist = s_npruned = 0;
    s_best = 0ull;
  }
  __syncthreads();
  // the margin of this query's own m/z range, from the peaks just loaded (no extra trip to memory
  // in front of the load); beyond RS_MARGIN_MAX the query leaves the hash path (uniform)
  // (ppm: linear bins of the query's widest window, tol_max -- see rs_bin_margin)
  const double tol_max = qn > 0 ? rs_tol_max(Q.mz[0], Q.mz[qn - 1], tol, ppm) : tol;
  const double margin = qn > 0 ? rs_bin_margin(Q.mz[0], Q.mz[qn - 1], tol_max) : 0.0;
  if (!(margin <= RS_MARGIN_MAX)) {
    defer_query();
    return;
  }
  const double inv_w = 1.0 / (2.0 * tol_max);
  if (tid < qn) {
    const double qm = (double)Q.mz[tid];
    const double tl = rs_frag_tol(tol, ppm, qm);
    s_qtol[tid] = tl;
    // (tol_i <= tol_max for ascending peaks; the clamp keeps a spectrum that breaks that rule at <= 3
    // bins per peak, which is what the table is sized for)
    const double tf = fmin(tl, tol_max);
    const int blo = (int)floor((qm - tf) * inv_w - margin);
    const int bhi = (int)floor((qm + tf) * inv_w + margin);
    for (int b = blo; b <= bhi; ++b) {
      const uint32_t bit = hbit(b);
      atomicOr(&H.bm[bit >> 5], 1u << (bit & 31));
      uint32_t h = hbin(b);
      for (;;) {
        const int old = atomicCAS(&H.bin[h], RS_EMPTY, b);
        if (old == RS_EMPTY) {
          H.peak[h] = (uint8_t)tid;
          break;
        }
        h = (h + 1) & (RS_HT - 1);
      }
    }
  }
  __syncthreads();
  FlatLds &Wv = W[wave];
  const float inv_w_f = (float)inv_w;
  const int parts = RS_WAVES, part = wave, ny = (int)gridDim.y;
  const int t = lane & 31, hi = lane >> 5;

  for (long long sb = c0; sb < c1; sb += RS_SUPER) {
    // ---- compact the valid slots of this super-chunk
    const int sn = (int)((c1 - sb) < RS_SUPER ? (c1 - sb) : RS_SUPER);
    if (tid == 0) s_nv = 0;
    __syncthreads();
    for (int i0 = 0; i0 < sn; i0 += blockDim.x) {
      const int i = i0 + tid;
      bool ok = false;
      if (i < sn) {
        ok = is_cand(sb + i);
        if (!ok && blockIdx.y == 0) pair_score[sb + i] = -1.0;
        ok = ok && (ny == 1 || ((i >> 5) % ny) == (int)blockIdx.y);   // (see the pair kernel)
      }
      const unsigned long long bal = __ballot(ok);
      int wbase = 0;
      if (lane == 0 && bal) wbase = atomicAdd(&s_nv, __popcll(bal));
      wbase = rl_i(wbase, 0);
      if (ok) s_list[wbase + __popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)i;
    }
    __syncthreads();
    const int nv = s_nv;
    const int per = (nv + parts - 1) / parts;
    const int wb = part * per;
    const int we = wb + per < nv ? wb + per : nv;

    for (int base = wb; base < we;) {
      // ---- set-up: lanes t and t + 32 both hold candidate t (they share the owner fill)
      const bool okr = base + t < we;
      const int slot = okr ? (int)s_list[base + t] : 0;
      int m_co = 0, m_cn = 0, m_chg = 0;
      double m_pmz = 0.0;
      if (okr) {
        const long long row = cv.row(q, sb + slot);
        if (cv.flt.meta) {     // one 32-byte sector per candidate
          const RowMeta *mr = meta_row(cv.flt, row);
          const uint4 a = *reinterpret_cast<const uint4 *>(mr);
          m_co = (int)a.x;
          m_cn = (int)a.y;
          m_chg = (int)a.z;
          m_pmz = mr->pmz64;
          if (L.records) m_co = (int)mr->rec4;     // base of the peak record, 4-byte units
        } else {
          m_co = L.offsets[row];
          m_cn = L.offsets[row + 1] - m_co;
          m_chg = L.precursor_charge[row];
          m_pmz = L.precursor_mz[row];
        }
      }
      const double pmd = (q_pmz - m_pmz) * (double)(unsigned)m_chg;            // cpp:18
      const int S = (allow_shift && fabs(pmd) >= gate) ? m_chg + 1 : 1;         // cpp:20
      // (a shift beyond the bin filter's envelope: RS_MD_ENV)
      const bool def_bs = okr && (m_cn > 64 || m_chg >= 31 || (S > 1 && !(fabs(pmd) <= RS_MD_ENV)));
      const bool def_pair = okr && !def_bs && S > RF_SMAX;
      const int cn_eff = (okr && !def_bs && !def_pair && qn > 0) ? m_cn : 0;
      // prefix sums over the 32 candidates: both halves of the wave hold the same values, so the
      // 64-lane DPP scan (common.hpp) is the 32-lane one plus, in the upper half, the total
      int incl = (int)wave_incl_scan((uint32_t)cn_eff);
      incl -= hi ? rl_i(incl, 31) : 0;
      // the chunk ends where the owner table is full (the prefix sums ascend)
      const uint32_t fit = (uint32_t)__ballot(okr && incl <= RF_PMAX);
      const int ntake = __popc(fit);          // >= 1: a candidate has <= 64 peaks here
      const bool take = t < ntake;
      const int excl = incl - cn_eff;
      const int P = rl_i(incl, ntake - 1);
      int cmaxw = take ? cn_eff : 0, Smaxw = (take && cn_eff > 0) ? S : 0;
      cmaxw = rl_i(wave_max_to_lane63(cmaxw), 63);     // (both >= 0)
      Smaxw = rl_i(wave_max_to_lane63(Smaxw), 63);
      if (take && hi == 0) {
        Wv.cptr[t] = (L.records && cv.flt.meta)
                         ? (unsigned long long)(reinterpret_cast<const float *>(L.records) + (uint32_t)m_co)
                         : (unsigned long long)(uint32_t)m_co;
        // (a candidate with more shifts has no peak in the stream: cn_eff = 0)
        Wv.ckey[t] = ((uint32_t)cn_eff << 24) | ((rf_key(t, min(S, RF_SMAX)) - (uint32_t)excl) & 0xffffffu);
        Wv.pmd[t] = pmd;
        Wv.sum[t] = 0.0;
        Wv.qmask[t][0] = Wv.qmask[t][1] = Wv.qmask[t][2] = Wv.qmask[t][3] = 0u;
        Wv.cmask[t][0] = Wv.cmask[t][1] = 0u;
        Wv.emax[t] = 0u;
        Wv.emin[t] = 255u;
        // mass_diff[s] = pmd / s (cpp:26-31); x / 1, x / 2, x / 4 are exact scalings
        Wv.mdf[t][0] = (float)pmd;
        Wv.mdf[t][1] = (float)(pmd * 0.5);
        Wv.mdf[t][3] = (float)(pmd * 0.25);
      }
      if (Smaxw > 3) {          // wave-uniform: the fp64 division only where a charge-3 candidate is
        if (take && hi == 0) Wv.mdf[t][2] = (float)(pmd / 3.0);
      }
      // (a lane past its candidate's last peak writes that peak's byte again: one predicate for the
      // whole loop instead of one per store)
      if (take && cn_eff > 0) {
        for (int j0 = 0; j0 < cmaxw; j0 += 2) Wv.owner[excl + min(j0 + hi, cn_eff - 1)] = (uint8_t)t;
      }
      wave_sync();

      // ---- the chunk's peaks as one stream, loads one step ahead. The stream needs a peak's m/z
      // and fragment charge only; intensities are read by the drain, for the peaks that hit
      float n_cm = 0.0f;
      int n_cc = 0;
      uint32_t n_key = 0u;      // rf_key + the peak's index; 0 where the lane holds no peak: no shift is probed
      auto fetch = [&](int p0) {
        // A lane beyond the stream reads the stream's last peak again and gets the key 0: neither the
        // table reads nor the loads need a predicate (P > 0 here).
        const bool act = p0 + lane < P;
        const int p = min(p0 + lane, P - 1);
        const uint32_t n_tt = (uint32_t)Wv.owner[p];
        const unsigned long long cp = Wv.cptr[n_tt];
        const uint32_t ck = Wv.ckey[n_tt];
        const uint32_t k = (ck + (uint32_t)p) & 0xffffu;
        const int n_j = (int)(k & 63u);
        n_key = act ? k : 0u;
        if (L.records && cv.flt.meta) {      // [mz x cn][charge x cn][intensity x cn], one record
          const gfloat_p rf = (gfloat_p)cp;
          const int cnr = (int)(ck >> 24);
          n_cm = rf[n_j];
          n_cc = (int)((gbyte_p)rf)[4 * cnr + n_j];
        } else {
          const int n_co = (int)(uint32_t)cp;
          n_cm = L.mz[n_co + n_j];
          n_cc = L.charge ? (int)L.charge[n_co + n_j] : 0;
        }
      };
      // ---- queued (peak, shift) items, a row at a time: an item names its candidate and its peak
      // there (the peak's values come from the lines the stream has just read)
      int mq_n = 0;
      auto drain = [&]() {
        wave_sync();
        for (int e0 = 0; e0 < mq_n; e0 += 64) {
          const bool on = e0 + lane < mq_n;
          // Read by every lane: e0 is a multiple of 64 below mq_n <= RF_MQ, so e0 + lane < RF_MQ, and a
          // stale or never written item beyond mq_n is masked into the tables (tt < RF_NC); whatever is
          // dereferenced from it sits under `on`.
          static_assert(RF_MQ % 64 == 0 && RF_MQ >= 128, "the drain reads the queue in rows of 64; a probe appends up to 64");
          const uint32_t ent = (uint32_t)Wv.mq[e0 + lane];
          const int s = on ? (int)(ent >> 11) : 0, tt = (int)((ent >> 6) & (uint32_t)(RF_NC - 1)), j = (int)(ent & 63u);
          const unsigned long long cp = Wv.cptr[tt];
          const int co = (int)(uint32_t)cp, cn = (int)(Wv.ckey[tt] >> 24);
          float cm = 0.0f, ci = 0.0f;
          int cc = 0;
          if (on) {
            if (L.records && cv.flt.meta) {
              const gfloat_p rf = (gfloat_p)cp;
              cm = rf[j];
              ci = rf[rec_int0(cn) + j];
              cc = (int)((gbyte_p)rf)[4 * cn + j];
            } else {
              cm = L.mz[co + j];
              ci = L.intensity[co + j];
              cc = L.charge ? (int)L.charge[co + j] : 0;
            }
          }
          if (on) {
            const float mdv = s ? Wv.mdf[tt][s - 1] : 0.0f;
            const int b = (int)floorf((cm + mdv) * inv_w_f);
            const double pm = Wv.pmd[tt];
            // mass_diff[s] = pmd / s: exact scalings but for s = 3, and a shift beyond 2 is queued only in
            // a chunk that holds a candidate of charge >= 3 (wave-uniform, as at the set-up)
            double md = s == 0 ? 0.0 : s == 2 ? pm * 0.5 : pm;
            if (Smaxw > 3) md = s == 3 ? pm / 3.0 : s == 4 ? pm * 0.25 : md;
            const double mult = (s == 0 || cc == s) ? 1.0 : 2.0 / 3.0;
            uint32_t h = hbin(b);
            for (;;) {
              const int eb = H.bin[h];
              if (eb == RS_EMPTY) break;
              if (eb == b) {
                const int i = H.peak[h];
                const double x = (double)cm + md;
                const double qm = (double)Q.mz[i];
                const double tl = s_qtol[i];
                const double lim = qm - tl;
                if (fabs(qm - x) <= tl && (!(lim > x) || j == cn - 1)) {
                  // the reference walks from its cursor: every peak between the cursor and j
                  // must pass the window test too (differs only on fp boundaries)
                  bool run = true;
                  for (int jj = j; jj > 0; --jj) {
                    const double xp = (double)((L.records && cv.flt.meta) ? ((gfloat_p)cp)[jj - 1] : L.mz[co + jj - 1]) + md;
                    if (lim > xp) break;
                    if (!(fabs(qm - xp) <= tl)) {
                      run = false;
                      break;
                    }
                  }
                  if (run) {
                    const float prod = (float)(mult * (double)Q.inten[i] * (double)ci);   // cpp:81
                    const uint32_t e = max((__float_as_uint(prod) >> 23) & 0xffu, 1u);
                    const uint32_t qb = 1u << (i & 31), cb = 1u << (j & 31);
                    const uint32_t oq = atomicOr(&Wv.qmask[tt][i >> 5], qb);
                    const uint32_t oc = atomicOr(&Wv.cmask[tt][j >> 5], cb);
                    // bit 31: a doubly matched peak; bits 31 + 30: a negative or NaN product (no
                    // exact order-free sum AND no upper bound; both bits, so that the max keeps them)
                    atomicMax(&Wv.emax[tt], !(prod >= 0.0f)               ? (0xC0000000u | e)
                                            : ((oq & qb) || (oc & cb)) ? (0x80000000u | e)
                                                                       : e);
                    atomicMin(&Wv.emin[tt], e);
                    atomicAdd(&Wv.sum[tt], (double)prod);
                  }
                }
              }
              h = (h + 1) & (RS_HT - 1);
            }
          }
        }
        mq_n = 0;
        wave_sync();
      };
      if (P > 0) fetch(0);
      for (int p0 = 0; p0 < P; p0 += 64) {
        const float cm = n_cm;
        const int cc = n_cc;
        const uint32_t key = n_key;
        if (p0 + 64 < P) fetch(p0 + 64);
        // shifts this peak takes part in (cpp:58-75): every s < S for an unannotated peak, else
        // s = 0 and s = its fragment charge where that is < S (none where the lane holds no peak: the
        // key is 0). As bits below S, so that no lane branches: a charge byte beyond 31 is a bit
        // beyond every S
        const uint32_t sall = key >> 11;
        const uint32_t smask = (cc == 0 ? sall : (1u | (1u << min(cc, 31)))) & sall;
        // The bins of all the chunk's shifts are tested first, by every lane and without a branch (a
        // bin index is masked into the bitmap): the bitmap reads are in flight together, behind one
        // read of the candidate's shift table.
        auto bin_of = [&](float mdv) -> int { return (int)floorf((cm + mdv) * inv_w_f); };
        auto bm_word = [&](int b) -> uint32_t { return H.bm[(b >> 5) & (RS_BM_BITS / 32 - 1)]; };
        auto bm_bit = [&](uint32_t w, int b) -> uint32_t { return __builtin_amdgcn_ubfe(w, (uint32_t)b, 1u); };   // (bit b & 31)
        const int b0 = (int)floorf(cm * inv_w_f);      // (the bin of cm + 0.0f, also for -0.0f)
        uint32_t hits;
        if (Smaxw > 1) {          // wave-uniform
          const float *mr = Wv.mdf[(key >> 6) & (uint32_t)(RF_NC - 1)];
          const float2 m12 = *reinterpret_cast<const float2 *>(mr);
          const int b1 = bin_of(m12.x), b2 = bin_of(m12.y);
          const uint32_t w0 = bm_word(b0), w1 = bm_word(b1), w2 = bm_word(b2);
          hits = bm_bit(w0, b0) | (bm_bit(w1, b1) << 1) | (bm_bit(w2, b2) << 2);
          if (Smaxw > 3) {
            const float2 m34 = *reinterpret_cast<const float2 *>(mr + 2);
            const int b3 = bin_of(m34.x), b4 = bin_of(m34.y);
            const uint32_t w3 = bm_word(b3), w4 = bm_word(b4);
            hits |= (bm_bit(w3, b3) << 3) | (bm_bit(w4, b4) << 4);
          }
        } else {
          hits = bm_bit(bm_word(b0), b0);
        }
        hits &= smask;
        // A (peak, shift) whose bin is marked goes to the wave's queue, shift by shift; the probing
        // proper runs over full rows of queued items (drain) instead of inside this loop with the one
        // or two lanes that hit.
        const uint32_t item = key & 0x7ffu;
        for (int s = 0; s < Smaxw; ++s) {        // wave-uniform bound
          uint32_t hs = hits & (1u << s);
          // (keeps `hs` one value, so that the ballot and the store share one v_and + v_cmp: 2 vector
          // instructions a shift instead of the 5 the compiler makes of two separate bit tests
          // (profiles/rescore_flat_diet_isa.txt). Results do not depend on it: removing the line is safe.)
          asm volatile("" : "+v"(hs));
          const unsigned long long mm = __ballot(hs != 0u);
          if (!mm) continue;                      // wave-uniform
          const int c = __popcll(mm);
          if (mq_n + c > RF_MQ) drain();
          if (hs) {
            const uint32_t at = __builtin_amdgcn_mbcnt_hi((uint32_t)(mm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mm, (uint32_t)mq_n));
            Wv.mq[at] = (uint16_t)(item | ((uint32_t)s << 11));
          }
          mq_n += c;
        }
      }
      drain();
      wave_sync();
      // ---- scores of the chunk
      if (take && hi == 0) {
        const uint32_t em = Wv.emax[t], en = Wv.emin[t];
        double sc = Wv.sum[t];
        bool listed = false;
        if ((em >> 31) || ((em & 0xffu) > en + 23u)) {     // sort + greedy pass needed
          if (prune && !(em & 0x40000000u) && !def_pair && !def_bs) {   // sum[t] bounds the score: the epilogue decides
            const int k = atomicAdd(&s_nlist, 1);
            if (k < RF_DLIST) {
              s_dbound[k] = sc;
              s_dslot[k] = (uint32_t)(sb - c0) + (uint32_t)slot;
              listed = true;
            }
          }
          sc = RS_DEFER;
        }
        if (def_pair) sc = RS_DEFER;
        if (def_bs) sc = RS_DEFER_BS;
        if (!listed) pair_score[sb + slot] = sc;
        // (read first: after a query's first chunks hardly any score passes the maximum, and 32 lanes'
        // atomics on one address are served one by one; a stale read only costs a needless atomic)
        if (prune && sc >= 0.0) {
          const unsigned long long bits = (unsigned long long)__double_as_longlong(sc);
          if (bits > s_best) atomicMax(&s_best, bits);
        }
        if (sc == RS_DEFER) {
          atomicOr(&s_defer, RS_QD_PAIR);
          atomicAdd(&s_ndef, 1);
        }
        if (sc == RS_DEFER_BS) atomicOr(&s_defer, RS_QD_BS);
      }
      base += ntake;
      wave_sync();     // the chunk's tables are rebuilt
    }
    __syncthreads();   // s_list is rebuilt for the next super-chunk
  }
  // ---- the verdicts of the listed candidates, against the final best exact score (the loop's last
  // barrier has made every wave's list entries and maximum visible)
  const int nlist = s_nlist < RF_DLIST ? s_nlist : RF_DLIST;      // block-uniform; 0 unless `prune`
  if (nlist) {
    const double best = __longlong_as_double((long long)s_best);
    for (int k0 = 0; k0 < nlist; k0 += blockDim.x) {
      const int k = k0 + tid;
      bool out = false;
      if (k < nlist) {
        out = s_dbound[k] * (1.0 + RS_PRUNE_REL) + RS_PRUNE_ABS < best;
        pair_score[c0 + s_dslot[k]] = out ? RS_PRUNED : RS_DEFER;
      }
      const unsigned long long bal = __ballot(out);
      if (lane == 0 && bal) atomicAdd(&s_npruned, __popcll(bal));
    }
    __syncthreads();
  }
  if (tid == 0 && s_defer) {      // (several blocks per query when gridDim.y > 1: or + add)
    const int left = s_ndef - s_npruned;
    atomicOr(&q_defer[q], left ? s_defer : (s_defer & ~RS_QD_PAIR));
    if (left) atomicAdd(&q_defer[q], left << 2);
    // one block per query: its count is final, the query's items go on the work list here
    // (gridDim.y > 1: rescore_worklist_kernel, once every block's count is in)
    const int items = gridDim.y == 1 ? rs_append_items(q_defer, Qs.n, q, left, ymax) : 0;
    if (counts) {
      atomicAdd(&counts[0], (unsigned long long)s_ndef);
      atomicAdd(&counts[1], (unsigned long long)s_npruned);
      atomicAdd(&counts[2], (unsigned long long)items);
    }
  }
}

// The work list of the second launch where several blocks shared a query in the first (few queries
// with long lists): one thread per query, after the first launch.
__global__ void rescore_worklist_kernel(int *__restrict__ q_defer, int nq, int ymax,
                                        unsigned long long *__restrict__ counts) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const int qd = q_defer[q];
  if (!(qd & RS_QD_PAIR)) return;
  const int items = rs_append_items(q_defer, nq, q, qd >> 2, ymax);
  if (counts) atomicAdd(&counts[2], (unsigned long long)items);
}

// tie_by_row = 0: first position wins ties (get_best_match on a caller-ordered list);
// tie_by_row = 1: lowest library row wins ties (the reference's lists ascend in row,
// spectral_library.py:451, so this is the same rule for an unordered ANN list).
__global__ __launch_bounds__(64) void rescore_argmax_kernel(
    CandView cv, int nq, const double *__restrict__ pair_score, int tie_by_row,
    int32_t *__restrict__ best_cand, long long *__restrict__ best_slot,
    double *__restrict__ best_score, int32_t *__restrict__ n_valid) {
  const int q = blockIdx.x;
  const int lane = threadIdx.x;
  long long c0, c1;
  cv.range(q, c0, c1);
  double bs = -1.0;
  long long bkey = 0x7fffffffffffffffll, bpos = -1;
  int cnt = 0;
  for (long long c = c0 + lane; c < c1; c += 64) {
    const double s = pair_score[c];
    if (s < 0.0) {
      if (s == RS_PRUNED) ++cnt;      // a valid candidate below the best score: counted, never compared
      continue;
    }
    ++cnt;
    const long long key = tie_by_row ? cv.row(q, c) : c;
    if (s > bs || (s == bs && key < bkey)) {
      bs = s;
      bkey = key;
      bpos = c;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double os = __shfl_xor(bs, off);
    const long long ok = __shfl_xor(bkey, off);
    const long long op = __shfl_xor(bpos, off);
    cnt += __shfl_xor(cnt, off);
    if (os > bs || (os == bs && ok < bkey)) {
      bs = os;
      bkey = ok;
      bpos = op;
    }
  }
  if (lane == 0) {
    if (best_cand) best_cand[q] = bpos >= 0 ? (int32_t)(bpos - c0) : -1;
    if (best_slot) best_slot[q] = bpos;
    if (best_score) best_score[q] = bpos >= 0 ? bs : 0.0;
    if (n_valid) n_valid[q] = cnt;
  }
}

// One wave per winner, and a wave is a chain of dependent memory round trips (winner's slot -> its
// row -> its peaks) around little arithmetic: the kernel lives on the number of waves in flight,
// i.e. on the LDS a wave needs. SMALL: structures for spectra of <= 128 peaks and <= 128
// generated matches (4 KB per wave instead of 11: 32 waves per CU instead of 12); a winner beyond
// them is marked in m_defer and done by the full-size instantiation, which runs second and only
// looks at marked winners.
// `w` is the winner's index in best_slot, in m_defer and in every output, [nq, n]: q * n + rank
// (n = 1, the single winner: the query itself).
constexpr int RS_SMALL_P = 128, RS_SMALL_M = 128;
template <bool SMALL, class QL, class WL>
__device__ __forceinline__ void matches_one(int q, int w, int lane, QL &Qw, WL &Ww, int *s_cnt_w, const DevPeaks &Qs,
                                            const DevPeaks &L, const CandView &cv,
                                            const long long *__restrict__ best_slot, double tol, int ppm,
                                            int allow_shift, int32_t *__restrict__ pm_count, uint32_t *__restrict__ pm_pairs,
                                            int pm_stride, int32_t *__restrict__ best_row, int *status,
                                            int *__restrict__ m_defer) {
  const long long slot = best_slot[w];
  const long long row = slot >= 0 ? cv.row(q, slot) : -1;
  if (best_row && lane == 0) best_row[w] = (int32_t)row;
  if (row < 0) {
    if (pm_count && lane == 0) pm_count[w] = 0;
    if (pm_pairs)   // rows are fully defined: zero beyond the matches (callers may pass raw memory)
      for (int t = lane; t < 2 * pm_stride; t += 64) pm_pairs[(size_t)w * pm_stride * 2 + t] = 0u;
    return;
  }
  if (!pm_count && !pm_pairs) return;
  if (SMALL && Qs.offsets[q + 1] - Qs.offsets[q] > RS_SMALL_P) {
    if (lane == 0) m_defer[w] = 1;
    return;
  }
  int qn;
  load_query(lane, 64, Qs, q, Qw, qn, status);
  wave_sync();
  int cnt_tmp = 0;
  const double sc = dot_pair_wave<true, SMALL>(lane, Qw, qn, Qs.precursor_mz[q], L, (int)row, tol, ppm, allow_shift,
                                               Ww, pm_pairs ? pm_pairs + (size_t)w * pm_stride * 2 : nullptr,
                                               pm_pairs ? pm_stride : 0, s_cnt_w, status);
  if (SMALL && sc < 0.0) {        // (wave-uniform) does not fit: the second launch does this query
    if (lane == 0) m_defer[w] = 1;
    return;
  }
  wave_sync();
  cnt_tmp = *s_cnt_w;
  if (pm_count && lane == 0) pm_count[w] = cnt_tmp;
  if (pm_pairs)
    for (int t = 2 * (cnt_tmp < pm_stride ? cnt_tmp : pm_stride) + lane; t < 2 * pm_stride; t += 64)
      pm_pairs[(size_t)w * pm_stride * 2 + t] = 0u;
}

// SMALL: a wave per winner. Full size: a wave per RS_MF_GROUP winners, which reads their flags at once
// and does the marked ones (normally none: a 44 KB workgroup per four queries -- one per 64 now --, placed only to
// return, took 0.04 ms of a step).
constexpr int RS_MF_GROUP = 16;
template <bool SMALL>
__global__ __launch_bounds__(64 * RS_WAVES) void rescore_matches_kernel(
    DevPeaks Qs, DevPeaks L, CandView cv, int nq, int n, const long long *__restrict__ best_slot,
    double tol, int ppm, int allow_shift, int32_t *__restrict__ pm_count,
    uint32_t *__restrict__ pm_pairs, int pm_stride, int32_t *__restrict__ best_row,
    int *status, int *__restrict__ m_defer) {
  typedef QueryLdsT<SMALL ? RS_SMALL_P : RS_MAXP> QL;
  typedef WaveLdsT<SMALL ? RS_SMALL_P : RS_MAXP, SMALL ? RS_SMALL_M : RS_MCAP> WL;
  __shared__ QL Q[RS_WAVES];
  __shared__ WL W[RS_WAVES];
  __shared__ int s_cnt[RS_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long nw = (long long)nq * n;
  if (SMALL) {
    const long long w = (long long)blockIdx.x * RS_WAVES + wave;
    if (w >= nw) return;
    if (lane == 0) m_defer[w] = 0;
    matches_one<true>((int)(w / n), (int)w, lane, Q[wave], W[wave], &s_cnt[wave], Qs, L, cv, best_slot, tol,
                      ppm, allow_shift, pm_count, pm_pairs, pm_stride, best_row, status, m_defer);
    return;
  }
  // a wave takes RS_MF_GROUP consecutive winners: one read of their flags; if every one is marked
  // (spectra of more than 128 peaks) the grid still holds nw / 16 workgroups
  const long long base = ((long long)blockIdx.x * RS_WAVES + wave) * RS_MF_GROUP;
  unsigned long long todo = __ballot(lane < RS_MF_GROUP && base + lane < nw && m_defer[base + lane] != 0);
  while (todo) {          // wave-uniform
    const int l = __builtin_ctzll(todo);
    todo &= todo - 1ull;
    const long long w = base + l;
    matches_one<false>((int)(w / n), (int)w, lane, Q[wave], W[wave], &s_cnt[wave], Qs, L, cv, best_slot, tol,
                       ppm, allow_shift, pm_count, pm_pairs, pm_stride, best_row, status, m_defer);
    wave_sync();
  }
}

// ASL_RESCORE_PRUNE=0 keeps every deferred candidate for the pair kernel (A/B runs of one build);
// read once.
static bool rescore_prune_enabled() {
  static const bool on = [] {
    const char *e = getenv("ASL_RESCORE_PRUNE");
    return !(e && e[0] == '0');
  }();
  return on;
}

// Grid of the second launch: the blocks of the pair kernel the device holds at once (they walk the
// work list; more would only queue up to find it empty).
static int pair_resident_blocks(int form, const void *kern, int *blocks) {
  constexpr int MAX_DEV = 64;
  static std::atomic<int> cached[MAX_DEV][4];      // per device and form; 0: not asked yet
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  const bool slot = dev >= 0 && dev < MAX_DEV;
  int n = slot ? cached[dev][form].load(std::memory_order_relaxed) : 0;
  if (!n) {
    int cus = 0, per_cu = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 64 * RS_WAVES, 0));
    n = std::max(cus * per_cu, 1);
    if (slot) cached[dev][form].store(n, std::memory_order_relaxed);   // (every thread computes the same value)
  }
  *blocks = n;
  return ASL_OK;
}

// Host driver shared by asl_rescore_batch and asl_search_batch (rescore.hpp: RescoreRequest).
int rescore_device(const RescoreRequest &rq) {
  const DevPeaks &Q = rq.Q, &L = rq.L;
  const CandList &cand = rq.cand;
  const PrecFilter &filter = rq.filter;
  const BatchOut &out = rq.out;
  const int nq = Q.n, n_best = rq.n_best;
  if (nq == 0) return ASL_OK;
  if (!rq.scratch) return fail(ASL_ERR_INVALID, "rescore: no scratch (internal)");
  if (n_best < 0 || n_best > ASL_MAX_BEST) return fail(ASL_ERR_INVALID, "rescore: n_best (internal)");
  if (rq.group && n_best == 0) return fail(ASL_ERR_INVALID, "rescore: groups without n_best (internal)");
  if (cand.window && (!cand.offsets || cand.rows64 || cand.rows32 || !cand.window->begin ||
                      !cand.window->sorted_row || !filter.meta || !L.charge || !L.records))
    return fail(ASL_ERR_INVALID, "rescore: window lists need CSR offsets and packed rows (internal)");
  DevBuf<int> &q_defer = rq.scratch->q_defer, &m_defer = rq.scratch->m_defer;
  const CandView cv = make_cand_view(cand, filter);
  // what the kernels read as `tol`: the tolerance in Da, or (tol_ppm) the relative tolerance, one fp64
  // multiply done here once
  const int ppm = rq.tol_ppm ? 1 : 0;
  const double tol = ppm ? rq.tol * 1e-6 : rq.tol;
  if (rq.clear_status) HIP_TRY(hipMemsetAsync(rq.status, 0, sizeof(int), stream()));
  {
    ProfScope ps("rescore");
    // split long candidate lists over blockIdx.y when there are few queries
    int64_t avg = cand.total_slots / (nq > 0 ? nq : 1);
    int ysplit = 1;
    if (nq < 2048 && avg > 4096) ysplit = (int)std::min<int64_t>(64, cdiv(avg, 4096));
    {
      // hash kernel, then the binary-search kernel on whatever it deferred (its blocks
      // return at once for queries with nothing deferred)
      // the second launch may use more blocks per query where the first one splits the lists
      const int ymax = std::max(ysplit, RS_DEF_Y);
      ASL_TRY(q_defer.reserve(RescoreScratch::defer_ints((size_t)nq, ymax)));
      HIP_TRY(hipMemsetAsync(q_defer.p, 0, sizeof(int) * ((size_t)nq + 1), stream()));   // flags + item count
      const bool shaped = !cand.offsets && filter.meta && filter.wcol && L.charge && L.records &&
                          (cand.rows64 || cand.rows32);
      const int form = cand.window ? 3 : !shaped ? 0 : cand.rows64 ? 2 : 1;
      // Pruning (rescore_flat_kernel) is for the single winner, decided by the one block that sees all
      // of a query's candidates: ranked requests and split lists never meet RS_PRUNED. Nor does a request
      // with a score histogram, whatever its selection: a pruned slot holds no score to count
      const int prune = (n_best == 0 && ysplit == 1 && !out.score_hist && rescore_prune_enabled()) ? 1 : 0;
      unsigned long long *counts = prof_counts() ? prof_rescore_dev() : nullptr;
      // 1. flat kernel; 2. pair kernel over the work list of what it marked RS_DEFER; 3. binary-search
      // kernel on RS_DEFER_BS (its blocks return at once for queries without such slots)
      auto flat = form == 3 ? rescore_flat_kernel<3>
                  : form == 0 ? rescore_flat_kernel<0>
                  : form == 2 ? rescore_flat_kernel<2> : rescore_flat_kernel<1>;
      hipLaunchKernelGGL(flat, dim3(nq, ysplit), dim3(64 * RS_WAVES), 0, stream(), Q, L, cv, tol,
                         ppm, rq.allow_shift, rq.pair_score, q_defer.p, rq.status, prune, ymax, counts);
      ASL_CHECK_LAUNCH();
      if (ysplit > 1) {
        hipLaunchKernelGGL(rescore_worklist_kernel, dim3((unsigned)cdiv(nq, 256)), dim3(256), 0, stream(),
                           q_defer.p, nq, ymax, counts);
        ASL_CHECK_LAUNCH();
      }
      auto kern = form == 3 ? rescore_score_v2_kernel<3>
                  : form == 0 ? rescore_score_v2_kernel<0>
                  : form == 2 ? rescore_score_v2_kernel<2> : rescore_score_v2_kernel<1>;
      int pair_grid = 0;
      ASL_TRY(pair_resident_blocks(form, (const void *)kern, &pair_grid));
      hipLaunchKernelGGL(kern, dim3((unsigned)std::min<int64_t>(pair_grid, (int64_t)nq * ymax)),
                         dim3(64 * RS_WAVES), 0, stream(), Q, L, cv, tol, ppm, rq.allow_shift, rq.pair_score,
                         q_defer.p, rq.status);
      ASL_CHECK_LAUNCH();
      // (small batches keep a workgroup per query: when every query is marked -- tol <= 0, queries
      // of more than 100 peaks -- they need all the parallelism there is)
      const int bs_group = nq >= 4096 ? RS_BS_GROUP : 1;
      hipLaunchKernelGGL(rescore_score_kernel, dim3((unsigned)cdiv(nq, bs_group), ysplit), dim3(64 * RS_WAVES), 0,
                         stream(), Q, L, cv, tol, ppm, rq.allow_shift, rq.pair_score,
                         (const int *)q_defer.p, rq.status, bs_group);
    }
    ASL_CHECK_LAUNCH();
    if (out.score_hist) ASL_TRY(rescore_hist(cv, nq, cand.total_slots, rq.pair_score, out.score_hist));
    if (n_best > 0) {
      ASL_TRY(rescore_select_ranked(cv, nq, n_best, rq.pair_score, rq.tie_by_row, rq.group, (int)L.n, out.best_cand,
                                    rq.best_slot, out.best_score, out.n_cand));
    } else {
      hipLaunchKernelGGL(rescore_argmax_kernel, dim3(nq), dim3(64), 0, stream(), cv, nq,
                         rq.pair_score, rq.tie_by_row, out.best_cand, rq.best_slot, out.best_score, out.n_cand);
      ASL_CHECK_LAUNCH();
    }
  }
  if (rq.emit_matches) {
    ProfScope ps("rescore_matches");
    const int n = std::max(n_best, 1);
    const long long nw = (long long)nq * n;
    ASL_TRY(m_defer.reserve((size_t)nw));
    hipLaunchKernelGGL(rescore_matches_kernel<true>, dim3((unsigned)cdiv(nw, RS_WAVES)),
                       dim3(64 * RS_WAVES), 0, stream(), Q, L, cv, nq, n, rq.best_slot, tol,
                       ppm, rq.allow_shift, out.pm_count, out.pm_pairs, out.pm_stride, out.best_row, rq.status, m_defer.p);
    ASL_CHECK_LAUNCH();
    hipLaunchKernelGGL(rescore_matches_kernel<false>, dim3((unsigned)cdiv(nw, RS_MF_GROUP * RS_WAVES)),
                       dim3(64 * RS_WAVES), 0, stream(), Q, L, cv, nq, n, rq.best_slot, tol,
                       ppm, rq.allow_shift, out.pm_count, out.pm_pairs, out.pm_stride, out.best_row, rq.status, m_defer.p);
    ASL_CHECK_LAUNCH();
  }
  return ASL_OK;
}

int decode_score_flags(int word, const char *who, ScoreFlags &out) {
  if (word & ~(ASL_SCORE_SHIFT | ASL_SCORE_FRAGMENT_PPM))
    return fail(ASL_ERR_INVALID, "%s: allow_shift holds bits other than ASL_SCORE_SHIFT | ASL_SCORE_FRAGMENT_PPM", who);
  out.allow_shift = (word & ASL_SCORE_SHIFT) ? 1 : 0;
  out.tol_ppm = (word & ASL_SCORE_FRAGMENT_PPM) ? 1 : 0;
  return ASL_OK;
}

int rescore_status_error(int st) {
  if (st & RS_STATUS_PEAKS)
    return fail(ASL_ERR_CAPACITY, "rescore: a spectrum has more than %d peaks", RS_MAXP);
  if (st & RS_STATUS_MATCHES)
    return fail(ASL_ERR_CAPACITY, "rescore: a pair generated more than %d peak matches", RS_MCAP);
  if (st & RS_STATUS_WINDOW)
    return fail(ASL_ERR_STATE, "rescore: a tiled window search's winner rescored to another score (internal)");
  return ASL_OK;
}

int rescore_check_status(const int *status_dev) {
  int st = 0;
  HIP_TRY(hipMemcpyAsync(&st, status_dev, sizeof(int), hipMemcpyDeviceToHost, stream()));
  ASL_TRY(sync_stream());
  return rescore_status_error(st);
}

}  // namespace asl

using namespace asl;

// asl_rescore_batch (n_best = 0), asl_rescore_batch_topn (outputs [nq, n_best]) and
// asl_rescore_batch_topn_distinct (lib_group: [library->n] group ids, host or device; null: plain)
static int rescore_batch_sync(const asl_peaks_t *queries, const asl_peaks_t *library,
                              const int64_t *cand_rows, const int32_t *cand_offsets, double tol,
                              int score_flags, int n_best, int32_t *best_cand, double *best_score,
                              int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride,
                              const int32_t *lib_group = nullptr, int32_t *score_hist = nullptr) {
  if (!queries || !library) return fail(ASL_ERR_INVALID, "rescore_batch: null spectra");
  ScoreFlags sf;
  ASL_TRY(decode_score_flags(score_flags, "rescore_batch", sf));
  const int nq = queries->n;
  const size_t nw = (size_t)nq * (size_t)std::max(n_best, 1);
  if (nq == 0) return ASL_OK;
  if (!cand_offsets) return fail(ASL_ERR_INVALID, "rescore_batch: null cand_offsets");
  if (pm_pairs && pm_stride <= 0) return fail(ASL_ERR_INVALID, "rescore_batch: pm_stride");
  ASL_TRY(ensure_device());
  PeaksStage Q, L;
  ASL_TRY(Q.init(queries));
  ASL_TRY(L.init(library));
  In<int32_t> off;
  ASL_TRY(off.init(cand_offsets, (size_t)nq + 1));
  int32_t total = 0;
  if (is_device_ptr(cand_offsets)) {
    HIP_TRY(hipMemcpyAsync(&total, cand_offsets + nq, sizeof(int32_t), hipMemcpyDeviceToHost,
                           stream()));
    ASL_TRY(sync_stream());
  } else {
    total = cand_offsets[nq];
  }
  if (total < 0) return fail(ASL_ERR_INVALID, "rescore_batch: negative cand_offsets");
  if (total > 0 && !cand_rows) return fail(ASL_ERR_INVALID, "rescore_batch: null cand_rows");
  In<int64_t> rows;
  ASL_TRY(rows.init(cand_rows, (size_t)total));
  In<int32_t> grp;
  if (lib_group) ASL_TRY(grp.init(lib_group, (size_t)library->n));
  BatchOutStage o;
  ASL_TRY(o.init({.best_cand = best_cand, .best_score = best_score, .pm_count = pm_count, .pm_pairs = pm_pairs,
                  .pm_stride = pm_stride, .score_hist = score_hist}, (size_t)nq, nw));
  DevBuf<double> pair_score;
  DevBuf<long long> best_slot;
  DevBuf<int> status;
  ASL_TRY(pair_score.reserve((size_t)std::max(total, 1)));
  ASL_TRY(best_slot.reserve(nw));
  ASL_TRY(status.reserve(1));
  RescoreScratch scratch;      // lives until rescore_check_status below has synchronised
  ASL_TRY(rescore_device({.Q = Q.dev, .L = L.dev,
                          .cand = {.rows64 = rows.d, .offsets = off.d, .total_slots = total},
                          .tol = tol, .tol_ppm = sf.tol_ppm, .allow_shift = sf.allow_shift, .n_best = n_best,
                          .group = lib_group ? grp.d : nullptr,
                          .pair_score = pair_score.p, .best_slot = best_slot.p, .scratch = &scratch,
                          .status = status.p, .out = o.dev}));
  ASL_TRY(o.finish());
  return rescore_check_status(status.p);  // synchronises
}

extern "C" int asl_rescore_batch(const asl_peaks_t *queries, const asl_peaks_t *library,
                                 const int64_t *cand_rows, const int32_t *cand_offsets,
                                 double tol, int allow_shift, int32_t *best_cand,
                                 double *best_score, int32_t *pm_count, uint32_t *pm_pairs,
                                 int32_t pm_stride) {
  clear_error();
  return rescore_batch_sync(queries, library, cand_rows, cand_offsets, tol, allow_shift, 0, best_cand,
                            best_score, pm_count, pm_pairs, pm_stride);
}

extern "C" int asl_rescore_batch_topn(const asl_peaks_t *queries, const asl_peaks_t *library,
                                      const int64_t *cand_rows, const int32_t *cand_offsets,
                                      double tol, int allow_shift, int32_t n_best, int32_t *best_cand,
                                      double *best_score, int32_t *pm_count, uint32_t *pm_pairs,
                                      int32_t pm_stride) {
  clear_error();
  if (n_best < 1 || n_best > ASL_MAX_BEST)
    return fail(ASL_ERR_INVALID, "rescore_batch_topn: n_best must be in [1, %d]", ASL_MAX_BEST);
  ASL_TRY(ensure_device());     // (no device: ASL_ERR_NO_DEVICE whatever else was passed)
  return rescore_batch_sync(queries, library, cand_rows, cand_offsets, tol, allow_shift, n_best, best_cand,
                            best_score, pm_count, pm_pairs, pm_stride);
}

extern "C" int asl_rescore_batch_topn_distinct(const asl_peaks_t *queries, const asl_peaks_t *library,
                                               const int64_t *cand_rows, const int32_t *cand_offsets,
                                               const int32_t *lib_group, double tol, int allow_shift,
                                               int32_t n_best, int32_t *best_cand, double *best_score,
                                               int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride) {
  clear_error();
  if (n_best < 1 || n_best > ASL_MAX_BEST)
    return fail(ASL_ERR_INVALID, "rescore_batch_topn_distinct: n_best must be in [1, %d]", ASL_MAX_BEST);
  ASL_TRY(ensure_device());     // (no device: ASL_ERR_NO_DEVICE whatever else was passed)
  if (!lib_group) return fail(ASL_ERR_INVALID, "rescore_batch_topn_distinct: null lib_group");
  return rescore_batch_sync(queries, library, cand_rows, cand_offsets, tol, allow_shift, n_best, best_cand,
                            best_score, pm_count, pm_pairs, pm_stride, lib_group);
}

extern "C" int asl_rescore_batch_topn_hist(const asl_peaks_t *queries, const asl_peaks_t *library,
                                           const int64_t *cand_rows, const int32_t *cand_offsets,
                                           const int32_t *lib_group, double tol, int allow_shift, int32_t n_best,
                                           int32_t distinct, int32_t *best_cand, double *best_score,
                                           int32_t *pm_count, uint32_t *pm_pairs, int32_t pm_stride,
                                           int32_t *score_hist) {
  clear_error();
  if (n_best < 1 || n_best > ASL_MAX_BEST)
    return fail(ASL_ERR_INVALID, "rescore_batch_topn_hist: n_best must be in [1, %d]", ASL_MAX_BEST);
  ASL_TRY(ensure_device());     // (no device: ASL_ERR_NO_DEVICE whatever else was passed)
  if (distinct && !lib_group) return fail(ASL_ERR_STATE, "rescore_batch_topn_hist: distinct ranks without lib_group");
  return rescore_batch_sync(queries, library, cand_rows, cand_offsets, tol, allow_shift, n_best, best_cand,
                            best_score, pm_count, pm_pairs, pm_stride, distinct ? lib_group : nullptr, score_hist);
}
