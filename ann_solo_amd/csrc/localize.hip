// localize.hip -- where on the peptide does the unknown mass of an open-search match sit? Batched over the
// SSMs of a search (asl_localize_batch; the arithmetic contract is its comment in include/annsolo_mi.h and
// tests/localize_ref.py, bit for bit; DESIGN.md 3 "Localisation").
//
// One wavefront per SSM, four per 256-thread workgroup; the waves of a workgroup share nothing, so there
// is no workgroup barrier and a wave past the end of the batch leaves alone. Per wave, in its own LDS:
//   0. the residue masses and (spectra of at most 256 peaks, all that process_spectrum emits) the peaks
//      are staged; longer spectra are read from global memory;
//   1. lanes 0 / 1 build the prefix / suffix ladder (fp64, sequential: fragments.hpp);
//   2. a lane owns one (ion type, k, variant) entry at a time and walks the fragment charges in order: per
//      charge it bisects the ascending m/z for the first peak with x - theo >= -R (theo and R are fixed, the
//      subtraction is monotone in x: false .. true along the spectrum, exact) and walks forward while the
//      peak matches, keeping the most intense one; E / C of the entry are plain stores, no atomics;
//   3. a lane owns a site (slot L: no modification) and adds its 2 (L - 1) addends sequentially;
//   4. the summary is reduced over the wave on the order key of the double (d2ord) and the site index.
// Every peak index stays inside [0, n) whatever the order of the peaks: the bisection never leaves its
// bracket and the walk ends at n.
#include "fragments.hpp"

namespace asl {

constexpr int LZ_NT = 256, LZ_WAVES = LZ_NT / 64, LZ_STAGE = 256;

struct LocalizeArgs {
  const int32_t *seq_off;
  const double *mass, *nterm, *cterm;
  const int32_t *zmax;
  const double *delta;
  double tol, ppm_k;   // ppm_k = tol * 1e-6 (ppm mode)
  int ppm;
  double *site_score;
  int32_t *site_count;
  int32_t *best_lo, *best_hi, *n_best, *best_count;
  double *best_score, *runner_score, *none_score;
};

struct alignas(16) LocalizeLds {
  double lad[2][DC_LAD];      // P, S; from the site sums on: lad[0][t] the score of slot t, lad[1] its count (int32)
  double E[4][DC_MAXL];       // [(type << 1) | variant][k]; until the ladders stand: the residue masses
  uint8_t C[4][DC_MAXL];      // hits of the entry: at most one per charge
  float mz[LZ_STAGE], inten[LZ_STAGE];
};

__device__ __forceinline__ uint64_t lz_shfl_xor(uint64_t v, int m) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(v >> 32), m);
  return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(LZ_NT) void localize_kernel(DevPeaks Q, LocalizeArgs A) {
  __shared__ LocalizeLds lds[LZ_WAVES];
  const int lane = threadIdx.x & 63;
  LocalizeLds &W = lds[threadIdx.x >> 6];
  const int64_t sl = block_linear() * LZ_WAVES + (threadIdx.x >> 6);
  if (sl >= Q.n) return;
  const int s = (int)sl;
  const int o = Q.offsets[s], n = Q.offsets[s + 1] - o;
  if (n < 0 || n > DC_MAXN) return;         // (the host checked the counts)
  const int q0 = A.seq_off[s], L = A.seq_off[s + 1] - q0;
  if (L < 2 || L > DC_MAXL) return;         // (host-checked too: never beyond the LDS arrays)
  const int zmax = min(max(A.zmax[s], 1), DC_MAXZ);
  const double delta = A.delta[s];
  const float *g_mz = Q.mz + o, *g_int = Q.intensity + o;
  const bool staged = n <= LZ_STAGE;
  // 0. stage
  double *m = &W.E[0][0];
  for (int i = lane; i < L; i += 64) m[i] = A.mass[q0 + i];
  if (staged)
    for (int i = lane; i < n; i += 64) {
      W.mz[i] = g_mz[i];
      W.inten[i] = g_int[i];
    }
  wave_sync();
  // 1. ladders: P[0] = nterm, P[k] = P[k-1] + m[k-1]; S[0] = cterm, S[k] = S[k-1] + m[L-k]
  if (lane < 2) build_ladder(W.lad[lane], lane ? A.cterm[s] : A.nterm[s], L, lane, [&](int pos) { return m[pos]; });
  wave_sync();
  // 2./3. fragments and their evidence
  const int nk = L - 1;
  for (int e = lane; e < 4 * nk; e += 64) {
    const int tv = e / nk, k = 1 + (e - tv * nk);
    double base = (tv & 2) ? W.lad[1][k] + DC_H2O : W.lad[0][k];
    if (tv & 1) base = base + delta;
    double Es = 0.0;
    int Cs = 0;
    for (int z = 1; z <= zmax; ++z) {
      const double theo = frag_theo(base, 0.0, z);      // (base + 0.0 is base: no neutral losses here)
      const double R = A.ppm ? A.ppm_k * theo : A.tol;
      int a = 0, b = n;       // first peak with x - theo >= -R
      while (a < b) {
        const int mid = (a + b) >> 1;
        const double x = (double)(staged ? W.mz[mid] : g_mz[mid]);
        if (x - theo >= -R) b = mid; else a = mid + 1;
      }
      bool hit = false;
      float top = 0.0f;
      for (int i = a; i < n; ++i) {
        const double d = (double)(staged ? W.mz[i] : g_mz[i]) - theo;
        if (!(-R <= d && d <= R)) break;
        const float it = staged ? W.inten[i] : g_int[i];
        if (!hit || it > top) top = it;   // ties: the lowest index stays
        hit = true;
      }
      Es = Es + (hit ? (double)top : 0.0);
      Cs += hit;
    }
    W.E[tv][k] = Es;
    W.C[tv][k] = (uint8_t)Cs;
  }
  wave_sync();
  // 4. sites: b_k carries the mass iff k >= j + 1, y_k iff k >= L - j; slot L: nothing carries it
  double *score = W.lad[0];
  int32_t *count = reinterpret_cast<int32_t *>(W.lad[1]);
  for (int t = lane; t <= L; t += 64) {
    double sc = 0.0;
    int c = 0;
    for (int k = 1; k <= nk; ++k) {
      const int vb = (t < L && k >= t + 1) ? 1 : 0, vy = (t < L && k >= L - t) ? 3 : 2;
      sc = sc + W.E[vb][k];
      sc = sc + W.E[vy][k];
      c += W.C[vb][k] + W.C[vy][k];
    }
    score[t] = sc;
    count[t] = c;
    if (t < L) {
      if (A.site_score) A.site_score[q0 + t] = sc;
      if (A.site_count) A.site_count[q0 + t] = c;
    }
  }
  wave_sync();
  // 5. summary (every valid key is above 0: a lane without a site offers 0)
  uint64_t best = 0;
  for (int t = lane; t < L; t += 64) best = max(best, d2ord(score[t]));
  for (int sh = 32; sh; sh >>= 1) best = max(best, lz_shfl_xor(best, sh));
  int lo = DC_MAXL, hi = -1, nb = 0;
  uint64_t runner = 0;
  for (int t = lane; t < L; t += 64) {
    const uint64_t key = d2ord(score[t]);
    if (key == best) {
      lo = min(lo, t);
      hi = max(hi, t);
      ++nb;
    } else {
      runner = max(runner, key);
    }
  }
  for (int sh = 32; sh; sh >>= 1) {
    lo = min(lo, __shfl_xor(lo, sh));
    hi = max(hi, __shfl_xor(hi, sh));
    nb += __shfl_xor(nb, sh);
    runner = max(runner, lz_shfl_xor(runner, sh));
  }
  if (lane == 0) {
    if (A.best_lo) A.best_lo[s] = lo;
    if (A.best_hi) A.best_hi[s] = hi;
    if (A.n_best) A.n_best[s] = nb;
    if (A.best_count) A.best_count[s] = count[lo];
    if (A.best_score) A.best_score[s] = score[lo];
    if (A.runner_score) A.runner_score[s] = runner ? ord2d(runner) : score[lo];
    if (A.none_score) A.none_score[s] = score[L];
  }
}

}  // namespace asl

using namespace asl;

extern "C" int asl_localize_batch(const asl_peaks_t *queries, const int32_t *seq_offsets,
                                  const double *residue_mass, const double *nterm, const double *cterm,
                                  const int32_t *max_fragment_charge, const double *delta, double tolerance,
                                  int32_t tolerance_unit, double *site_score, int32_t *site_count,
                                  int32_t *best_lo, int32_t *best_hi, int32_t *n_best, int32_t *best_count,
                                  double *best_score, double *runner_score, double *none_score) {
  clear_error();
  if (!queries || !seq_offsets || !residue_mass || !nterm || !cterm || !max_fragment_charge || !delta)
    return fail(ASL_ERR_INVALID, "localize_batch: null argument");
  if (tolerance_unit != ASL_TOL_DA && tolerance_unit != ASL_TOL_PPM)
    return fail(ASL_ERR_INVALID, "localize_batch: tolerance_unit must be ASL_TOL_DA or ASL_TOL_PPM");
  if (!(tolerance >= 0.0)) return fail(ASL_ERR_INVALID, "localize_batch: negative (or NaN) tolerance");
  const int n = queries->n;
  if (n < 0) return fail(ASL_ERR_INVALID, "localize_batch: negative n");
  if (n == 0) return ASL_OK;
  if (!queries->offsets) return fail(ASL_ERR_INVALID, "localize_batch: peaks without offsets");
  ASL_TRY(ensure_device());
  // every limit is checked here, on host copies of the small arrays, before anything is launched or written
  std::vector<int32_t> h_off, h_seq, h_z;
  std::vector<double> h_nt, h_ct, h_delta, h_mass;
  ASL_TRY(to_host(h_off, queries->offsets, (size_t)n + 1));
  ASL_TRY(to_host(h_seq, seq_offsets, (size_t)n + 1));
  ASL_TRY(to_host(h_z, max_fragment_charge, (size_t)n));
  ASL_TRY(to_host(h_nt, nterm, (size_t)n));
  ASL_TRY(to_host(h_ct, cterm, (size_t)n));
  ASL_TRY(to_host(h_delta, delta, (size_t)n));
  ASL_TRY(sync_stream());
  int max_n = 0;
  ASL_TRY(check_fragment_batch("localize_batch", n, queries->n_peaks, h_off, h_seq, h_z, h_nt, h_ct, &max_n));
  for (int s = 0; s < n; ++s)
    if (!std::isfinite(h_delta[s])) return fail(ASL_ERR_INVALID, "localize_batch: spectrum %d: non-finite delta", s);
  const size_t R = (size_t)h_seq[n], total = (size_t)h_off[n];
  ASL_TRY(to_host(h_mass, residue_mass, R));
  ASL_TRY(sync_stream());
  for (int s = 0; s < n; ++s)
    for (int i = h_seq[s]; i < h_seq[s + 1]; ++i)
      if (!std::isfinite(h_mass[i]))
        return fail(ASL_ERR_INVALID, "localize_batch: spectrum %d: non-finite residue mass", s);
  if (total && (!queries->mz || !queries->intensity))
    return fail(ASL_ERR_INVALID, "localize_batch: peaks without mz / intensity");
  In<int32_t> i_off, i_seq, i_z;
  In<float> i_mz, i_int;
  In<double> i_mass, i_nt, i_ct, i_delta;
  ASL_TRY(i_off.init(queries->offsets, (size_t)n + 1));
  ASL_TRY(i_mz.init(queries->mz, total));
  ASL_TRY(i_int.init(queries->intensity, total));
  ASL_TRY(i_seq.init(seq_offsets, (size_t)n + 1));
  ASL_TRY(i_z.init(max_fragment_charge, (size_t)n));
  ASL_TRY(i_mass.init(residue_mass, R));
  ASL_TRY(i_nt.init(nterm, (size_t)n));
  ASL_TRY(i_ct.init(cterm, (size_t)n));
  ASL_TRY(i_delta.init(delta, (size_t)n));
  Out<double> o_ss, o_bs, o_rs, o_ns;
  Out<int32_t> o_sc, o_lo, o_hi, o_nb, o_bc;
  ASL_TRY(o_ss.init(site_score, R));
  ASL_TRY(o_sc.init(site_count, R));
  ASL_TRY(o_lo.init(best_lo, (size_t)n));
  ASL_TRY(o_hi.init(best_hi, (size_t)n));
  ASL_TRY(o_nb.init(n_best, (size_t)n));
  ASL_TRY(o_bc.init(best_count, (size_t)n));
  ASL_TRY(o_bs.init(best_score, (size_t)n));
  ASL_TRY(o_rs.init(runner_score, (size_t)n));
  ASL_TRY(o_ns.init(none_score, (size_t)n));
  DevPeaks Q;
  Q.n = n;
  Q.n_peaks = (int64_t)total;
  Q.offsets = i_off.d;
  Q.mz = i_mz.d;
  Q.intensity = i_int.d;
  LocalizeArgs A{i_seq.d, i_mass.d, i_nt.d, i_ct.d, i_z.d, i_delta.d, tolerance, tolerance * 1e-6,
                 tolerance_unit == ASL_TOL_PPM, o_ss.d, o_sc.d, o_lo.d, o_hi.d, o_nb.d, o_bc.d, o_bs.d, o_rs.d,
                 o_ns.d};
  {
    ProfScope ps("localize");
    hipLaunchKernelGGL(localize_kernel, grid_2d(cdiv(n, LZ_WAVES)), dim3(LZ_NT), 0, stream(), Q, A);
    ASL_CHECK_LAUNCH();
  }
  ASL_TRY(o_ss.finish());
  ASL_TRY(o_sc.finish());
  ASL_TRY(o_lo.finish());
  ASL_TRY(o_hi.finish());
  ASL_TRY(o_nb.finish());
  ASL_TRY(o_bc.finish());
  ASL_TRY(o_bs.finish());
  ASL_TRY(o_rs.finish());
  ASL_TRY(o_ns.finish());
  ASL_TRY(sync_stream());
  return ASL_OK;
}
