// decoy.hip -- batched shuffle-and-reposition decoys (replaces the per-spectrum Python loop of
// /root/reference/src/ann_solo/decoy_generator.py:93-185: annotate_proforma + get_theoretical_fragments +
// the reposition loop + argsort). The shuffle itself stays on the host (ann_solo_amd/decoy_generator.py);
// this file gets the permutation. PARITY: pinned by the reference's own known answer
// (tests/golden/decoy_kat.json) where that data can pin it, see DESIGN.md 3 "Decoys"; the arithmetic
// contract is the comment of asl_decoy_batch in include/annsolo_mi.h and tests/decoy_ref.py, bit for bit.
//
// One workgroup per library spectrum (<= 4096 peaks, peptide of 2 .. 128 residues). Four threads build
// the prefix / suffix mass ladders of target and decoy in LDS (fp64, sequential); every thread then
// annotates its peaks: per (ion type, fragment charge, neutral loss) the ladder index of the first
// fragment that can still match is found by bisection, the winner over all series is the match of lowest
// theoretical m/z. The repositioned peaks are ordered by a bitonic sort of (fp64 m/z, raw index) in LDS,
// sized to the largest spectrum of the batch (256 / 1024 / 4096).
#include "fragments.hpp"

namespace asl {

constexpr int DC_NT = 256, DC_NLOSS = 14;

__constant__ double dc_loss[DC_NLOSS] = {0.0,        -1.007825,  -17.026549, -18.010565, -27.994915,
                                         -43.989829, -45.021464, -46.005479, -63.998301, -79.956818,
                                         -79.966331, -91.009195, -91.993211, -97.976896};

struct DecoyArgs {
  const int32_t *seq_off;
  const double *mass;
  const int32_t *perm;
  const double *nterm, *cterm;
  const int32_t *zmax;
  double tol, ppm_k;   // ppm_k = tol * 1e-6 (ppm mode)
  int ppm;
  float *o_mz, *o_int;
  int32_t *o_src;
  uint8_t *o_chg, *a_type, *a_n, *a_z, *a_loss;
};

// ion types: 1 a, 2 b, 3 p, 4 y (0: no annotation). P / S: prefix / suffix ladder of one peptide.
__device__ __forceinline__ double frag_base(const double *P, const double *S, int type, int n, int L,
                                            double cterm) {
  if (type == 1) return P[n] - DC_CO;
  if (type == 2) return P[n];
  if (type == 3) return (P[L] + cterm) + DC_H2O;
  return S[n] + DC_H2O;
}

struct Ann {
  double theo;
  int type, n, z, loss;
};
__device__ __forceinline__ void offer(Ann &b, double theo, int type, int n, int z, int loss) {
  bool better = b.type == 0 || theo < b.theo;
  if (!better && theo == b.theo) {      // exact tie: ion type, then n, then z, then loss order
    if (type != b.type) better = type < b.type;
    else if (n != b.n) better = n < b.n;
    else if (z != b.z) better = z < b.z;
    else better = loss < b.loss;
  }
  if (better) b = Ann{theo, type, n, z, loss};
}

__global__ __launch_bounds__(DC_NT) void decoy_kernel(DevPeaks raw, DecoyArgs A, int nsort_max) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double *lad = reinterpret_cast<double *>(smem);                       // P, S, Pd, Sd: [4][DC_LAD]
  uint64_t *key = reinterpret_cast<uint64_t *>(lad + 4 * DC_LAD);       // [nsort_max]
  int32_t *ord = reinterpret_cast<int32_t *>(key + nsort_max);          // [nsort_max]
  uint8_t *zr = reinterpret_cast<uint8_t *>(ord + nsort_max);           // [nsort_max] z | 0x80: m/z is -0
  int *ctl = reinterpret_cast<int *>(zr + nsort_max);                   // 4 ints
  const int64_t sl = block_linear();
  if (sl >= raw.n) return;
  const int s = (int)sl, tid = threadIdx.x;
  const int o = raw.offsets[s], n = raw.offsets[s + 1] - o;
  if (n <= 0 || n > nsort_max) return;      // (the host checked the counts: never beyond the LDS arrays)
  const int q0 = A.seq_off[s], L = A.seq_off[s + 1] - q0;
  if (L < 2 || L > DC_MAXL) return;         // (host-checked too)
  const double nterm = A.nterm[s], cterm = A.cterm[s];
  const int zmax = min(max(A.zmax[s], 1), DC_MAXZ);
  const float *mz = raw.mz + o, *inten = raw.intensity + o;
  // 1. ladders: P[0] = nterm, P[k] = P[k-1] + m[k-1]; S[0] = cterm, S[k] = S[k-1] + m[L-k]
  if (tid < 4) {
    const bool dec = tid >= 2;
    // the bisection below needs ladders that rise by clear steps inside a moderate range (see there)
    ctl[tid] = build_ladder(lad + tid * DC_LAD, (tid & 1) ? cterm : nterm, L, tid & 1,
                            [&](int pos) { return A.mass[q0 + (dec ? A.perm[q0 + pos] : pos)]; });
  }
  __syncthreads();
  const double *P = lad, *S = lad + DC_LAD, *Pd = lad + 2 * DC_LAD, *Sd = lad + 3 * DC_LAD;
  // Bisection is exact where, per series, the fragments that match a peak are the leading ones of those
  // with x - theo <= R (R = tol, or ppm_k * theo): theo rises with n (every operation of frag_theo is
  // monotone), so that test is false .. true along the ladder and no fragment before the first `true`
  // matches. In Da mode none after a first `true` that fails |x - theo| <= R matches either (theo - x only
  // grows). In ppm mode that needs theo - x to outgrow ppm_k * theo, rounding included: steps of at least
  // 1e-3 / 8 against rounding errors below 1e-9 (|ladder| <= 1e6) and ppm_k <= 0.5 make it so. Any other
  // input (a residue lighter than 1e-3, say) takes the exhaustive scan.
  const bool fast = ctl[0] && ctl[1] && ctl[2] && ctl[3] && (!A.ppm || A.ppm_k <= 0.5);
  const int nsort = n <= 256 ? 256 : (n <= 1024 ? 1024 : 4096);
  for (int i = tid; i < nsort; i += DC_NT) {
    if (i >= n) {
      key[i] = ~0ull;
      ord[i] = i;
      continue;
    }
    // 2./3. annotation: the matching fragment of lowest theoretical m/z
    const double x = (double)mz[i];
    Ann best{0.0, 0, 0, 0, 0};
    for (int type = 1; type <= 4; ++type) {
      for (int z = 1; z <= zmax; ++z)
        for (int l = 0; l < DC_NLOSS; ++l) {
          const double loss = dc_loss[l];
          auto theo_at = [&](int k) { return frag_theo(frag_base(P, S, type, k, L, cterm), loss, z); };
          auto reach = [&](double t) { return A.ppm ? A.ppm_k * t : A.tol; };
          if (type == 3) {
            const double t = theo_at(L);
            if (fabs(x - t) <= reach(t)) offer(best, t, type, L, z, l);
          } else if (fast) {
            int a = 1, b = L;       // first k in [1, L) with x - theo(k) <= R(k)
            while (a < b) {
              const int mid = (a + b) >> 1;
              const double t = theo_at(mid);
              if (x - t <= reach(t)) b = mid; else a = mid + 1;
            }
            if (a < L) {
              const double t = theo_at(a);
              if (fabs(x - t) <= reach(t)) offer(best, t, type, a, z, l);
            }
          } else {
            for (int k = 1; k < L; ++k) {
              const double t = theo_at(k);
              if (fabs(x - t) <= reach(t)) offer(best, t, type, k, z, l);
            }
          }
        }
    }
    // 4. reposition: the same fragment on the decoy's ladders, the peak's own mass error kept
    double nm = x;
    if (best.type != 0) {
      const double td = frag_theo(frag_base(Pd, Sd, best.type, best.n, L, cterm), dc_loss[best.loss], best.z);
      nm = td + (x - best.theo);
    }
    key[i] = d2ord(nm);
    ord[i] = i;
    zr[i] = (uint8_t)(best.z | ((nm == 0.0 && signbit(nm)) ? 0x80 : 0));
    if (A.a_type) A.a_type[o + i] = (uint8_t)best.type;
    if (A.a_n) A.a_n[o + i] = (uint8_t)best.n;
    if (A.a_z) A.a_z[o + i] = (uint8_t)best.z;
    if (A.a_loss) A.a_loss[o + i] = (uint8_t)best.loss;
  }
  __syncthreads();
  // 5. ascending by (fp64 m/z, raw index): bitonic network over nsort entries
  for (int k = 2; k <= nsort; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (nsort >> 1); t += DC_NT) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const uint64_t ka = key[lo], kb = key[hi];
        const int32_t ia = ord[lo], ib = ord[hi];
        const bool gt = ka > kb || (ka == kb && ia > ib);
        if (gt == ((lo & k) == 0)) {
          key[lo] = kb;
          key[hi] = ka;
          ord[lo] = ib;
          ord[hi] = ia;
        }
      }
      __syncthreads();
    }
  // 6. one rounding to float32; intensity and fragment charge travel with the peak
  for (int j = tid; j < n; j += DC_NT) {
    const int src = ord[j];
    const int zf = zr[src];
    float v = mz[src];                     // an unannotated peak keeps its m/z
    if (zf & 0x0f) {
      const double nm = ord2d(key[j]);
      v = (float)((zf & 0x80) ? -nm : nm);
    }
    if (A.o_mz) A.o_mz[o + j] = v;
    if (A.o_int) A.o_int[o + j] = inten[src];
    if (A.o_src) A.o_src[o + j] = src;
    if (A.o_chg) A.o_chg[o + j] = (uint8_t)(zf & 0x0f);
  }
}

}  // namespace asl

using namespace asl;

extern "C" int asl_decoy_batch(const asl_peaks_t *raw, const int32_t *seq_offsets,
                               const double *residue_mass, const int32_t *perm, const double *nterm,
                               const double *cterm, const int32_t *max_fragment_charge,
                               double tolerance, int32_t tolerance_unit, float *out_mz,
                               float *out_intensity, int32_t *out_src, uint8_t *out_charge,
                               uint8_t *ann_type, uint8_t *ann_n, uint8_t *ann_z, uint8_t *ann_loss) {
  clear_error();
  if (!raw || !seq_offsets || !residue_mass || !perm || !nterm || !cterm || !max_fragment_charge)
    return fail(ASL_ERR_INVALID, "decoy_batch: null argument");
  if (tolerance_unit != ASL_TOL_DA && tolerance_unit != ASL_TOL_PPM)
    return fail(ASL_ERR_INVALID, "decoy_batch: tolerance_unit must be ASL_TOL_DA or ASL_TOL_PPM");
  if (!(tolerance >= 0.0)) return fail(ASL_ERR_INVALID, "decoy_batch: negative (or NaN) tolerance");
  const int n = raw->n;
  if (n < 0) return fail(ASL_ERR_INVALID, "decoy_batch: negative n");
  if (n == 0) return ASL_OK;
  if (!raw->offsets) return fail(ASL_ERR_INVALID, "decoy_batch: peaks without offsets");
  ASL_TRY(ensure_device());
  // every limit is checked here, on host copies of the small arrays, before anything is launched or written
  std::vector<int32_t> h_off, h_seq, h_z, h_perm;
  std::vector<double> h_nt, h_ct, h_mass;
  ASL_TRY(to_host(h_off, raw->offsets, (size_t)n + 1));
  ASL_TRY(to_host(h_seq, seq_offsets, (size_t)n + 1));
  ASL_TRY(to_host(h_z, max_fragment_charge, (size_t)n));
  ASL_TRY(to_host(h_nt, nterm, (size_t)n));
  ASL_TRY(to_host(h_ct, cterm, (size_t)n));
  ASL_TRY(sync_stream());
  int max_n = 0;
  ASL_TRY(check_fragment_batch("decoy_batch", n, raw->n_peaks, h_off, h_seq, h_z, h_nt, h_ct, &max_n));
  const size_t R = (size_t)h_seq[n];
  ASL_TRY(to_host(h_mass, residue_mass, R));
  ASL_TRY(to_host(h_perm, perm, R));
  ASL_TRY(sync_stream());
  for (int s = 0; s < n; ++s) {
    const int q0 = h_seq[s], L = h_seq[s + 1] - q0;
    bool seen[DC_MAXL] = {false};
    for (int i = 0; i < L; ++i) {
      if (!std::isfinite(h_mass[q0 + i]))
        return fail(ASL_ERR_INVALID, "decoy_batch: spectrum %d: non-finite residue mass", s);
      const int p = h_perm[q0 + i];
      if (p < 0 || p >= L || seen[p])
        return fail(ASL_ERR_INVALID, "decoy_batch: spectrum %d: perm is not a permutation", s);
      seen[p] = true;
    }
  }
  const size_t total = (size_t)h_off[n];
  if (total == 0) return ASL_OK;
  if (!raw->mz || !raw->intensity) return fail(ASL_ERR_INVALID, "decoy_batch: peaks without mz / intensity");
  asl_peaks_t rp = *raw;
  rp.n_peaks = (int64_t)total;
  PeaksStage Rg;
  ASL_TRY(Rg.init(&rp));
  In<int32_t> i_seq, i_perm, i_z;
  In<double> i_mass, i_nt, i_ct;
  ASL_TRY(i_seq.init(seq_offsets, (size_t)n + 1));
  ASL_TRY(i_perm.init(perm, R));
  ASL_TRY(i_z.init(max_fragment_charge, (size_t)n));
  ASL_TRY(i_mass.init(residue_mass, R));
  ASL_TRY(i_nt.init(nterm, (size_t)n));
  ASL_TRY(i_ct.init(cterm, (size_t)n));
  Out<float> o_mz, o_int;
  Out<int32_t> o_src;
  Out<uint8_t> o_chg, a_type, a_n, a_z, a_loss;
  ASL_TRY(o_mz.init(out_mz, total));
  ASL_TRY(o_int.init(out_intensity, total));
  ASL_TRY(o_src.init(out_src, total));
  ASL_TRY(o_chg.init(out_charge, total));
  ASL_TRY(a_type.init(ann_type, total));
  ASL_TRY(a_n.init(ann_n, total));
  ASL_TRY(a_z.init(ann_z, total));
  ASL_TRY(a_loss.init(ann_loss, total));
  DecoyArgs A{i_seq.d, i_mass.d, i_perm.d, i_nt.d, i_ct.d, i_z.d, tolerance, tolerance * 1e-6,
              tolerance_unit == ASL_TOL_PPM, o_mz.d, o_int.d, o_src.d, o_chg.d, a_type.d, a_n.d, a_z.d,
              a_loss.d};
  const int nsort = max_n <= 256 ? 256 : (max_n <= 1024 ? 1024 : DC_MAXN);
  const size_t lds = (size_t)4 * DC_LAD * sizeof(double) + (size_t)nsort * (8 + 4 + 1) + 16;
  HIP_TRY(hipFuncSetAttribute((const void *)decoy_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds));
  {
    ProfScope ps("decoy");
    hipLaunchKernelGGL(decoy_kernel, grid_2d(n), dim3(DC_NT), lds, stream(), Rg.dev, A, nsort);
    ASL_CHECK_LAUNCH();
  }
  ASL_TRY(o_mz.finish());
  ASL_TRY(o_int.finish());
  ASL_TRY(o_src.finish());
  ASL_TRY(o_chg.finish());
  ASL_TRY(a_type.finish());
  ASL_TRY(a_n.finish());
  ASL_TRY(a_z.finish());
  ASL_TRY(a_loss.finish());
  ASL_TRY(sync_stream());
  return ASL_OK;
}
