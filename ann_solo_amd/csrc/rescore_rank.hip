// rescore_rank.hip -- the ranked side of the rescoring: selection of the n best slots per query
// (asl_*_topn, asl_*_topn_distinct; rescore_device's pass 2 when n_best > 0) and the fold of a tiled
// window search's per-tile winners into the running ones (window_search.hip: window_search_device).
// Scoring, the single-winner argmax and the peak matches are in rescore.hip.
#include "common.hpp"
#include "rescore_cand.hpp"

namespace asl {

// The order of the ranks: score descending, then the tie key ascending, then the position.
// Does (s, k, p) go before (ps, pk, pp)?
__device__ __forceinline__ bool ranks_before(double s, int32_t k, int32_t p, double ps, int32_t pk, int32_t pp) {
  return s > ps || (s == ps && (k < pk || (k == pk && p < pp)));
}

// The first of the lanes' (s, k, p) in that order, in every lane.
__device__ __forceinline__ void wave_first(double &s, int32_t &k, int32_t &p) {
  for (int off = 32; off > 0; off >>= 1) {
    const double os = __shfl_xor(s, off);
    const int32_t ok = __shfl_xor(k, off), op = __shfl_xor(p, off);
    if (ranks_before(os, ok, op, s, k, p)) {
      s = os;
      k = ok;
      p = op;
    }
  }
}

// Top-n selection (asl_*_topn): the n best slots of a query instead of the single best, in the
// argmax's order -- score descending, then the tie key ascending (tie_by_row as for the argmax), then
// the slot position (only a row that a caller's list names twice under tie_by_row = 1 gets that far).
// One wave per query, ONE pass over the list whatever n is: every lane keeps the best n of the
// slots it reads, sorted, in an LDS array laid out [n][64] (lane-strided: a lane's entries sit in
// its own banks); a slot is inserted only when it beats the lane's n-th, which after the first few
// hundred slots is rare, so the pass costs the argmax's coalesced read of pair_score. Then the 64
// sorted lane lists are merged: n rounds of a wave arg-max over the lanes' heads. Positions and
// rows are kept as 32-bit values (positions relative to the list's first slot; lists and library
// rows are 32-bit everywhere in the callers). Dynamic LDS: n * 64 * 16 bytes.
// Outputs [nq, n]; ranks beyond the valid slots: slot -1, score 0.
//
// DISTINCT (asl_*_topn_distinct): the same ranking with one rule added -- walking the slots in that
// order, a slot is skipped when an earlier rank holds a row of the same group (group[row], 32 bits
// per library row; a negative id is "ungrouped" and collides with nothing, not even with itself
// listed twice). The same single pass: every lane keeps the best n of its slots WITH DISTINCT GROUPS
// (a fourth LDS plane [n][64] of group ids). A slot whose group the lane holds replaces that entry
// if it beats it and is dropped otherwise; a slot with a new group is inserted as above. The
// `s < ts` cut stands: a lane that holds n groups, all ahead of the slot, has no use for it whatever
// its group -- so group[row] is gathered only for the slots that pass the cut.
// Merge: the winner's group (wave-uniform, at most n of them) goes to a 16-entry LDS line, and every
// lane moves its head past entries whose group is on that line.
// Exact: an element of the answer is the best of its group among all slots, hence in its lane, and
// the groups ahead of it in its lane are ahead of it in the answer too, fewer than n: the lane kept
// it. In the merge the best slot of a group not yet emitted is its lane's first entry off the line
// (everything ahead of it in the lane beats it and would otherwise be that best slot), so it is
// the arg-max of the heads. Rank 0 is the plain winner; with every group negative nothing ever
// collides and the outputs are the plain instantiation's byte for byte.
// Dynamic LDS: n * 64 * 20 + 64 bytes (20 KB at n = 16).
template <bool DISTINCT>
__global__ __launch_bounds__(64) void rescore_topn_kernel(
    CandView cv, int nq, int n, const double *__restrict__ pair_score, int tie_by_row,
    const int32_t *__restrict__ group, int n_lib, int32_t *__restrict__ best_cand, long long *__restrict__ best_slot,
    double *__restrict__ best_score, int32_t *__restrict__ n_valid) {
  extern __shared__ __attribute__((aligned(16))) double topn_lds[];      // (no static LDS in front of it)
  double *S = topn_lds;                                      // [n][64] scores
  int32_t *K = reinterpret_cast<int32_t *>(S + n * 64);      // [n][64] tie keys
  int32_t *P = K + n * 64;                                   // [n][64] positions
  int32_t *G = P + n * 64;                                   // DISTINCT: [n][64] group ids
  int32_t *E = G + n * 64;                                   // DISTINCT: [16] groups emitted so far (merge)
  const int q = blockIdx.x;
  const int lane = threadIdx.x;
  long long c0, c1;
  cv.range(q, c0, c1);
  int have = 0, cnt = 0;
  double ts = -1.0;          // the lane's n-th entry once it holds n
  int32_t tk = 0, tp = 0;
  for (long long c = c0 + lane; c < c1; c += 64) {
    const double s = pair_score[c];
    if (s < 0.0) continue;
    ++cnt;
    if (have == n && s < ts) continue;
    const int32_t pos = (int32_t)(c - c0);
    const int32_t row = (DISTINCT || tie_by_row) ? (int32_t)cv.row(q, c) : 0;   // (a scored slot: a row of the library)
    const int32_t key = tie_by_row ? row : pos;
    if (have == n && !ranks_before(s, key, pos, ts, tk, tp)) continue;
    int i = have < n ? have : n - 1;                 // a new entry: from the end, the n-th falls out
    int32_t g = -1;
    bool held = false;
    if (DISTINCT) {
      g = (uint32_t)row < (uint32_t)n_lib ? group[row] : -1;
      if (g >= 0) {
        for (int j = 0; j < have; ++j) {
          if (G[j * 64 + lane] == g) {
            i = j;                                   // the group's entry: replaced in place or kept
            held = true;
            break;
          }
        }
      }
      if (held && !ranks_before(s, key, pos, S[i * 64 + lane], K[i * 64 + lane], P[i * 64 + lane])) continue;
    }
    while (i > 0) {
      const double ps = S[(i - 1) * 64 + lane];
      const int32_t pk = K[(i - 1) * 64 + lane], pp = P[(i - 1) * 64 + lane];
      if (!ranks_before(s, key, pos, ps, pk, pp)) break;
      S[i * 64 + lane] = ps;
      K[i * 64 + lane] = pk;
      P[i * 64 + lane] = pp;
      if (DISTINCT) G[i * 64 + lane] = G[(i - 1) * 64 + lane];
      --i;
    }
    S[i * 64 + lane] = s;
    K[i * 64 + lane] = key;
    P[i * 64 + lane] = pos;
    if (DISTINCT) G[i * 64 + lane] = g;
    if (!held && have < n) ++have;
    if (have == n) {
      ts = S[(n - 1) * 64 + lane];
      tk = K[(n - 1) * 64 + lane];
      tp = P[(n - 1) * 64 + lane];
    }
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  int head = 0, ne = 0;      // ne: groups on the line (wave-uniform)
  for (int r = 0; r < n; ++r) {
    const bool live = head < have;
    const double ms = live ? S[head * 64 + lane] : -1.0;
    const int32_t mk = live ? K[head * 64 + lane] : 0x7fffffff;
    const int32_t mp = live ? P[head * 64 + lane] : 0x7fffffff;
    double bs = ms;
    int32_t bk = mk, bp = mp;
    wave_first(bs, bk, bp);
    const bool any = bs >= 0.0;               // wave-uniform: positions are unique, the order is total
    if (lane == 0) {
      const size_t o = (size_t)q * n + r;
      if (best_cand) best_cand[o] = any ? bp : -1;
      if (best_slot) best_slot[o] = any ? c0 + bp : -1;
      if (best_score) best_score[o] = any ? bs : 0.0;
    }
    if (!any) continue;                       // (every later round is empty too)
    const bool mine = live && mp == bp;       // the lane that held the winner moves on
    if (!DISTINCT) {
      if (mine) ++head;
      continue;
    }
    const unsigned long long who = __ballot(mine);
    const int32_t wg = __shfl(live ? G[head * 64 + lane] : -1, __builtin_ctzll(who));
    if (mine) ++head;
    if (wg >= 0) {
      if (lane == 0) E[ne] = wg;
      ++ne;
      wave_sync();
    }
    while (head < have) {                     // past the entries whose group has a rank already
      const int32_t hg = G[head * 64 + lane];
      bool out = false;
      if (hg >= 0)
        for (int e = 0; e < ne; ++e) out = out || E[e] == hg;
      if (!out) break;
      ++head;
    }
  }
  if (lane == 0 && n_valid) n_valid[q] = cnt;
}

int rescore_select_ranked(const CandView &cv, int nq, int n, const double *pair_score, int tie_by_row,
                          const int32_t *group, int n_lib, int32_t *best_cand, long long *best_slot,
                          double *best_score, int32_t *n_valid) {
  if (group)
    hipLaunchKernelGGL(rescore_topn_kernel<true>, dim3(nq), dim3(64), (size_t)n * 64 * 20 + 64, stream(), cv, nq, n,
                       pair_score, tie_by_row, group, n_lib, best_cand, best_slot, best_score, n_valid);
  else
    hipLaunchKernelGGL(rescore_topn_kernel<false>, dim3(nq), dim3(64), (size_t)n * 64 * 16, stream(), cv, nq, n,
                       pair_score, tie_by_row, group, n_lib, best_cand, best_slot, best_score, n_valid);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

// Tiled window search (window_search.hip): the fold of one tile, one thread per query of the tile. Each
// query's tiles are folded in stream order, so the running list needs no atomics. The tile's n best
// (slots, scores: the selection above or the argmax, sorted) and the running n best of the query
// (rows, scores, sorted, row -1 beyond the filled ranks) are two sorted lists of at most n over
// disjoint rows, so merging them by (score descending, row ascending) and keeping n is exact
// whatever the tile cuts were. With groups both lists hold one row per group (the running list by
// induction) and an entry whose group the output already holds is skipped: an element of the
// distinct top-n of the union is the best of its group in its own list with fewer than n groups
// ahead of it there, so it is in that list's distinct top-n, and the walk meets the two lists'
// entries in the order of the union. Skipping moves entries up by any number of ranks: the result is
// built in a local array and written back.
__global__ __launch_bounds__(256) void window_merge_kernel(
    CandView cv, int nq, int n, const long long *__restrict__ best_slot, const double *__restrict__ best_score,
    const int32_t *__restrict__ n_valid, const int32_t *__restrict__ group, double *__restrict__ run_score,
    int32_t *__restrict__ run_row, int32_t *__restrict__ run_n) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  run_n[q] += n_valid[q];
  const long long *ts = best_slot + (size_t)q * n;
  const double *tsc = best_score + (size_t)q * n;
  double *rs = run_score + (size_t)q * n;
  int32_t *rr = run_row + (size_t)q * n;
  int la = 0, lb = 0;
  while (la < n && rr[la] >= 0) ++la;
  while (lb < n && ts[lb] >= 0) ++lb;
  if (lb == 0) return;
  double os[ASL_MAX_BEST];
  int32_t orow[ASL_MAX_BEST], og[ASL_MAX_BEST];
  int no = 0, ia = 0, ib = 0;
  while (no < n && (ia < la || ib < lb)) {
    double s;
    int32_t r;
    bool a = ib >= lb;
    if (!a) {
      s = tsc[ib];
      r = (int32_t)cv.row(q, ts[ib]);
      a = ia < la && ranks_before(rs[ia], rr[ia], 0, s, r, 0);     // (the rows are disjoint: no third key)
    }
    if (a) {
      s = rs[ia];
      r = rr[ia];
      ++ia;
    } else {
      ++ib;
    }
    const int32_t g = group ? group[r] : -1;
    bool dup = false;
    if (g >= 0)
      for (int k = 0; k < no; ++k) dup = dup || og[k] == g;
    if (dup) continue;
    os[no] = s;
    orow[no] = r;
    og[no] = g;
    ++no;
  }
  for (int k = 0; k < no; ++k) {      // (no >= la: nothing of the running list is left behind)
    rs[k] = os[k];
    rr[k] = orow[k];
  }
}

// After the last tile and the n-candidate pass over the running lists (`rescored`: its best_score
// [nq, n], the same order): every filled rank's rescored score must be the merged one.
__global__ __launch_bounds__(256) void window_finish_kernel(
    int nq, int n, const double *__restrict__ run_score, const int32_t *__restrict__ run_row,
    const int32_t *__restrict__ run_n, const double *__restrict__ rescored, double *__restrict__ best_score,
    int32_t *__restrict__ n_cand, int *status) {
  const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= (long long)nq * n) return;
  const bool won = run_row[w] >= 0;
  if (won && rescored[w] != run_score[w]) atomicOr(status, RS_STATUS_WINDOW);
  if (best_score) best_score[w] = won ? run_score[w] : 0.0;
  if (n_cand && w % n == 0) n_cand[w / n] = run_n[w / n];
}

int rescore_window_merge(const CandList &cand, int nq, int n, const long long *best_slot,
                         const double *best_score, const int32_t *n_valid, double *run_score,
                         int32_t *run_row, int32_t *run_n, const int32_t *group) {
  if (nq <= 0) return ASL_OK;
  if (n < 1 || n > ASL_MAX_BEST || !cand.window) return fail(ASL_ERR_INVALID, "window merge: n or list (internal)");
  hipLaunchKernelGGL(window_merge_kernel, dim3((unsigned)cdiv(nq, 256)), dim3(256), 0, stream(),
                     make_cand_view(cand, PrecFilter()), nq, n, best_slot, best_score, n_valid, group, run_score,
                     run_row, run_n);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

int rescore_window_finish(int nq, int n, const double *run_score, const int32_t *run_row,
                          const int32_t *run_n, const double *rescored, double *best_score,
                          int32_t *n_cand, int *status) {
  if (nq <= 0) return ASL_OK;
  hipLaunchKernelGGL(window_finish_kernel, dim3((unsigned)cdiv((long long)nq * n, 256)), dim3(256), 0,
                     stream(), nq, n, run_score, run_row, run_n, rescored, best_score, n_cand, status);
  ASL_CHECK_LAUNCH();
  return ASL_OK;
}

}  // namespace asl
