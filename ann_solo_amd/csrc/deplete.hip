// deplete.hip -- chimeric spectra: what is left of a query once its winner has taken its peaks? Batched
// over the SSMs of a search (asl_deplete_batch; the contract is its comment in include/annsolo_mi.h and
// tests/deplete_ref.py, bit for bit; DESIGN.md 3 "Chimeric search").
//
// One wavefront per SSM, four per 256-thread workgroup; the waves of a workgroup share nothing, so there
// is no workgroup barrier and a wave past the end of the batch leaves alone. Per wave, in its own LDS:
//   0. the library row's peaks (m/z widened to double, charge) are staged when there are at most DP_STAGE
//      of them -- all that process_spectrum emits --; longer rows are read from global memory;
//   1. lanes take query peaks lane, lane + 64, ..: per shift c the lane bisects the row for the first
//      peak j with q - (l[j] + md) <= tol_i (the window test's own subtraction, which does not increase
//      with j: false .. true along the row, exact) and walks forward while the peak is inside the window,
//      until one passes the charge rule;
//   2. the unexplained peaks of a 64-peak chunk are compacted in order with a ballot and its mbcnt prefix:
//      m/z and source index go to the output row, the intensity to the wave's LDS;
//   3. lane 0 runs process.hip's L2 norm over the kept intensities (ascending fmaf chain, sqrtf), the
//      lanes divide, pad the row with zeros and lane 0 writes count, validity and energy.
// No atomics: equal inputs give equal bits. Every peak index stays inside its spectrum's slice whatever
// the order of the peaks: the bisection never leaves its bracket and the walk ends at the row's end.
#include "fragments.hpp"   // to_host
#include "rescore.hpp"     // decode_score_flags

namespace asl {

constexpr int DP_NT = 256, DP_WAVES = DP_NT / 64, DP_STAGE = 256, DP_MAXN = 4096;

struct DepleteArgs {
  const int64_t *lib_rows;
  double tol;          // Da: the tolerance; ppm: rel = tolerance * 1e-6
  int ppm, shift;
  int32_t min_peaks;
  double min_mz_range;
  int32_t stride;
  int32_t kept_cap;    // floats of LDS per wave for the kept intensities: >= the batch's largest query
  float *out_mz, *out_int;
  int32_t *out_src, *out_count;
  uint8_t *out_valid;
  float *energy;
};

// a wave's LDS: the staged row, then the kept intensities, [kept_cap] floats (a multiple of 64)
struct alignas(16) DepleteLds {
  double mz[DP_STAGE];
  uint8_t chg[DP_STAGE];
};
inline size_t dp_wave_bytes(int kept_cap) { return sizeof(DepleteLds) + (size_t)kept_cap * sizeof(float); }

__global__ __launch_bounds__(DP_NT) void deplete_kernel(DevPeaks Q, DevPeaks L, DepleteArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  char *mine = smem + (size_t)wave * (sizeof(DepleteLds) + (size_t)A.kept_cap * sizeof(float));
  DepleteLds &W = *reinterpret_cast<DepleteLds *>(mine);
  float *kept = reinterpret_cast<float *>(mine + sizeof(DepleteLds));
  const int64_t sl = block_linear() * DP_WAVES + wave;
  if (sl >= Q.n) return;
  const int s = (int)sl;
  const size_t row0 = (size_t)s * A.stride;
  const int64_t row = A.lib_rows[s];
  const int qo = Q.offsets[s];
  int qn = Q.offsets[s + 1] - qo;
  // (the host checked every limit: nothing here goes beyond the LDS arrays or the output row)
  if (row < 0 || row >= L.n || qn < 0 || qn > A.kept_cap || qn > A.stride) qn = -1;
  int total = 0, first = 0, last = 0;
  if (qn > 0) {
    const int lo = L.offsets[row];
    const int ln = max(L.offsets[row + 1] - lo, 0);
    const float *l_mz = L.mz + lo;
    const uint8_t *l_chg = L.charge ? L.charge + lo : nullptr;
    const float *q_mz = Q.mz + qo, *q_int = Q.intensity + qo;
    const bool staged = ln <= DP_STAGE;
    if (staged) {
      for (int j = lane; j < ln; j += 64) {
        W.mz[j] = (double)l_mz[j];
        W.chg[j] = l_chg ? l_chg[j] : (uint8_t)0;
      }
      wave_sync();
    }
    const double q_pmz = Q.precursor_mz[s];
    const int z = L.precursor_charge[row];
    const double pmd = (q_pmz - L.precursor_mz[row]) * (double)z;
    const bool gate = fabs(pmd) >= (A.ppm ? A.tol * q_pmz : A.tol);
    const int64_t S = (A.shift && gate) ? (int64_t)z + 1 : 1;
    for (int qb = 0; qb < qn; qb += 64) {
      const int i = qb + lane;
      bool explained = false;
      float x_mz = 0.0f;
      if (i < qn) {
        x_mz = q_mz[i];
        const double qm = (double)x_mz;
        const double tl = A.ppm ? A.tol * qm : A.tol;
        for (int64_t c = 0; c < S && !explained; ++c) {
          const double md = c ? pmd / (double)c : 0.0;
          int a = 0, b = ln;      // first j with qm - (l[j] + md) <= tl
          while (a < b) {
            const int mid = (a + b) >> 1;
            const double x = (staged ? W.mz[mid] : (double)l_mz[mid]) + md;
            if (qm - x <= tl) b = mid; else a = mid + 1;
          }
          for (int j = a; j < ln; ++j) {
            const double x = (staged ? W.mz[j] : (double)l_mz[j]) + md;
            if (!(fabs(qm - x) <= tl)) break;
            const int cj = staged ? (int)W.chg[j] : (l_chg ? (int)l_chg[j] : 0);
            if (c == 0 || cj == 0 || (int64_t)cj == c) {
              explained = true;
              break;
            }
          }
        }
      }
      const bool keep = i < qn && !explained;
      const uint64_t mask = __ballot(keep);
      if (keep) {
        const int pos = total + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                               __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        A.out_mz[row0 + pos] = x_mz;
        if (A.out_src) A.out_src[row0 + pos] = i;
        kept[pos] = q_int[i];
      }
      if (mask) {
        if (total == 0) first = qb + __builtin_ctzll(mask);
        last = qb + 63 - __builtin_clzll(mask);
        total += __popcll(mask);
      }
    }
    wave_sync();
    // process.hip's L2 norm: ascending fmaf chain, sqrtf, IEEE divide
    float acc = 0.0f;
    if (lane == 0)
      for (int t = 0; t < total; ++t) acc = __builtin_fmaf(kept[t], kept[t], acc);
    acc = __shfl(acc, 0);
    const float nrm = __builtin_sqrtf(acc);
    for (int t = lane; t < total; t += 64) A.out_int[row0 + t] = kept[t] / nrm;
    if (lane == 0) {
      // process.hip's wg_valid on the kept peaks
      const bool ok = total >= A.min_peaks && total > 0 && (double)(q_mz[last] - q_mz[first]) >= A.min_mz_range;
      A.out_count[s] = total;
      A.out_valid[s] = ok ? 1 : 0;
      if (A.energy) A.energy[s] = acc;
    }
  } else if (lane == 0) {
    A.out_count[s] = 0;
    A.out_valid[s] = 0;
    if (A.energy) A.energy[s] = 0.0f;
  }
  for (int t = total + lane; t < A.stride; t += 64) {
    A.out_mz[row0 + t] = 0.0f;
    A.out_int[row0 + t] = 0.0f;
    if (A.out_src) A.out_src[row0 + t] = 0;
  }
}

}  // namespace asl

using namespace asl;

extern "C" int asl_deplete_batch(const asl_peaks_t *queries, const asl_peaks_t *library, const int64_t *lib_rows,
                                 double fragment_mz_tolerance, int allow_shift, int32_t min_peaks,
                                 double min_mz_range, int32_t out_stride, float *out_mz, float *out_intensity,
                                 int32_t *out_src, int32_t *out_count, uint8_t *out_valid, float *kept_energy) {
  clear_error();
  if (!queries || !library || !lib_rows || !out_count || !out_valid)
    return fail(ASL_ERR_INVALID, "deplete_batch: null argument");
  ScoreFlags sf;
  ASL_TRY(decode_score_flags(allow_shift, "deplete_batch", sf));
  if (!(fragment_mz_tolerance >= 0.0)) return fail(ASL_ERR_INVALID, "deplete_batch: negative (or NaN) tolerance");
  const int n = queries->n;
  if (n < 0 || library->n < 0) return fail(ASL_ERR_INVALID, "deplete_batch: negative n");
  if (out_stride < 0) return fail(ASL_ERR_INVALID, "deplete_batch: negative out_stride");
  if (n == 0) return ASL_OK;
  if (!queries->offsets || !queries->precursor_mz)
    return fail(ASL_ERR_INVALID, "deplete_batch: queries without offsets / precursor m/z");
  ASL_TRY(ensure_device());
  // every limit is checked here, on host copies of the small arrays, before anything is launched or written
  std::vector<int32_t> h_qoff, h_loff;
  std::vector<int64_t> h_rows;
  ASL_TRY(to_host(h_qoff, queries->offsets, (size_t)n + 1));
  ASL_TRY(to_host(h_rows, lib_rows, (size_t)n));
  if (library->n) {
    if (!library->offsets || !library->precursor_mz || !library->precursor_charge)
      return fail(ASL_ERR_INVALID, "deplete_batch: library without offsets / precursor arrays");
    // (the whole column, 8 MB at 2.1 M rows, once per call of up to 32 768 SSMs: the named rows' peak counts
    // are read here and nowhere else on the host)
    ASL_TRY(to_host(h_loff, library->offsets, (size_t)library->n + 1));
  }
  ASL_TRY(sync_stream());
  if (h_qoff[0] < 0) return fail(ASL_ERR_INVALID, "deplete_batch: negative offsets");
  int max_q = 0;
  for (int s = 0; s < n; ++s) {
    const int c = h_qoff[s + 1] - h_qoff[s];
    if (c < 0) return fail(ASL_ERR_INVALID, "deplete_batch: peak offsets descend at spectrum %d", s);
    if (c > DP_MAXN)
      return fail(ASL_ERR_CAPACITY, "deplete_batch: spectrum %d has more than %d peaks", s, DP_MAXN);
    max_q = std::max(max_q, c);
  }
  if (queries->n_peaks > 0 && h_qoff[n] > queries->n_peaks)
    return fail(ASL_ERR_INVALID, "deplete_batch: offsets beyond n_peaks");
  if (library->n && h_loff[0] < 0) return fail(ASL_ERR_INVALID, "deplete_batch: negative library offsets");
  bool lib_peaks = false;
  for (int s = 0; s < n; ++s) {
    const int64_t r = h_rows[s];
    if (r < 0) continue;
    if (r >= library->n)
      return fail(ASL_ERR_INVALID, "deplete_batch: SSM %d: library row %lld of %d", s, (long long)r, library->n);
    const int c = h_loff[r + 1] - h_loff[r];
    if (c < 0) return fail(ASL_ERR_INVALID, "deplete_batch: library offsets descend at row %lld", (long long)r);
    if (c > DP_MAXN)
      return fail(ASL_ERR_CAPACITY, "deplete_batch: library row %lld has more than %d peaks", (long long)r, DP_MAXN);
    if (library->n_peaks > 0 && h_loff[r + 1] > library->n_peaks)
      return fail(ASL_ERR_INVALID, "deplete_batch: library offsets beyond n_peaks");
    lib_peaks = lib_peaks || c > 0;
  }
  if (out_stride < max_q)
    return fail(ASL_ERR_CAPACITY, "deplete_batch: out_stride %d below the largest query (%d peaks)", out_stride, max_q);
  const size_t total = (size_t)h_qoff[n], slots = (size_t)n * (size_t)out_stride;
  if (total && (!queries->mz || !queries->intensity))
    return fail(ASL_ERR_INVALID, "deplete_batch: peaks without mz / intensity");
  if (lib_peaks && !library->mz) return fail(ASL_ERR_INVALID, "deplete_batch: library peaks without mz");
  if (slots && (!out_mz || !out_intensity)) return fail(ASL_ERR_INVALID, "deplete_batch: null output rows");
  const size_t ltotal = library->n ? (size_t)h_loff[library->n] : 0;
  In<int32_t> q_off, l_off, l_pz;
  In<float> q_mz, q_int, l_mz;
  In<uint8_t> l_chg;
  In<double> q_pmz, l_pmz;
  In<int64_t> rows;
  ASL_TRY(q_off.init(queries->offsets, (size_t)n + 1));
  ASL_TRY(q_mz.init(queries->mz, total));
  ASL_TRY(q_int.init(queries->intensity, total));
  ASL_TRY(q_pmz.init(queries->precursor_mz, (size_t)n));
  ASL_TRY(rows.init(lib_rows, (size_t)n));
  if (library->n) {
    ASL_TRY(l_off.init(library->offsets, (size_t)library->n + 1));
    ASL_TRY(l_mz.init(library->mz, ltotal));
    ASL_TRY(l_chg.init(library->charge, ltotal));
    ASL_TRY(l_pmz.init(library->precursor_mz, (size_t)library->n));
    ASL_TRY(l_pz.init(library->precursor_charge, (size_t)library->n));
  }
  Out<float> o_mz, o_int, o_en;
  Out<int32_t> o_src, o_cnt;
  Out<uint8_t> o_val;
  ASL_TRY(o_mz.init(out_mz, slots));
  ASL_TRY(o_int.init(out_intensity, slots));
  ASL_TRY(o_src.init(out_src, slots));
  ASL_TRY(o_cnt.init(out_count, (size_t)n));
  ASL_TRY(o_val.init(out_valid, (size_t)n));
  ASL_TRY(o_en.init(kept_energy, (size_t)n));
  DevPeaks Q, L;
  Q.n = n;
  Q.n_peaks = (int64_t)total;
  Q.offsets = q_off.d;
  Q.mz = q_mz.d;
  Q.intensity = q_int.d;
  Q.precursor_mz = q_pmz.d;
  L.n = library->n;
  L.n_peaks = (int64_t)ltotal;
  L.offsets = l_off.d;
  L.mz = l_mz.d;
  L.charge = l_chg.d;
  L.precursor_mz = l_pmz.d;
  L.precursor_charge = l_pz.d;
  const int kept_cap = std::max((max_q + 63) & ~63, 64);
  DepleteArgs A{rows.d, sf.tol_ppm ? fragment_mz_tolerance * 1e-6 : fragment_mz_tolerance, sf.tol_ppm,
                sf.allow_shift, min_peaks, min_mz_range, out_stride, kept_cap, o_mz.d, o_int.d, o_src.d,
                o_cnt.d, o_val.d, o_en.d};
  const size_t dyn = DP_WAVES * dp_wave_bytes(kept_cap);   // 10 KiB at 64 peaks, 73 KiB at 4096
  HIP_TRY(hipFuncSetAttribute((const void *)deplete_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
  {
    ProfScope ps("deplete");
    hipLaunchKernelGGL(deplete_kernel, grid_2d(cdiv(n, DP_WAVES)), dim3(DP_NT), dyn, stream(), Q, L, A);
    ASL_CHECK_LAUNCH();
  }
  ASL_TRY(o_mz.finish());
  ASL_TRY(o_int.finish());
  ASL_TRY(o_src.finish());
  ASL_TRY(o_cnt.finish());
  ASL_TRY(o_val.finish());
  ASL_TRY(o_en.finish());
  ASL_TRY(sync_stream());
  return ASL_OK;
}
