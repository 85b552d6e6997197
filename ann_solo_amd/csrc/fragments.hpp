// fragments.hpp -- what the peptide-fragment kernels share (decoy.hip, localize.hip): the mass constants
// and capacity limits, the prefix / suffix mass ladders, the theoretical m/z of a fragment, the order key
// of a double, and the host-side check of a batch's small arrays. The arithmetic is the contract written
// down in include/annsolo_mi.h (asl_decoy_batch steps 1-2, asl_localize_batch steps 1-2): IEEE double,
// no fused multiply-add, every sum sequential.
#pragma once
#include <cmath>
#include <vector>

#include "common.hpp"

namespace asl {

constexpr int DC_MAXN = 4096, DC_MAXL = 128, DC_MAXZ = 8;
constexpr int DC_LAD = DC_MAXL + 1;
constexpr double DC_PROTON = 1.007276466, DC_CO = 27.994915, DC_H2O = 18.010565;

// One ladder, sequential: out[0] = start, out[k] = out[k-1] + m(pos) with pos = k - 1 (prefix) or L - k
// (suffix); mass_at(pos) is residue pos of the peptide. Returns whether the ladder is `steady`: |start|
// and |out[L]| at most 1e6 and every step at least 1e-3 (what the decoy kernel's bisection along the
// ladder needs).
template <class MassAt>
__device__ __forceinline__ bool build_ladder(double *out, double start, int L, bool suffix, MassAt mass_at) {
  double acc = start;
  bool steady = fabs(acc) <= 1e6;
  out[0] = acc;
  for (int k = 1; k <= L; ++k) {
    const double m = mass_at(suffix ? L - k : k - 1);
    acc = acc + m;
    out[k] = acc;
    steady = steady && m >= 1e-3;
  }
  return steady && fabs(acc) <= 1e6;
}

__device__ __forceinline__ double frag_theo(double base, double loss, int z) {
  return (base + loss) / (double)z + DC_PROTON;     // add, divide, add
}

// fp64 -> u64 whose unsigned order is the numeric order (-0 and +0 share a key, NaN last)
__device__ __forceinline__ uint64_t d2ord(double v) {
  if (v != v) return 0xFFFFFFFFFFFFFFFEull;
  if (v == 0.0) return 0x8000000000000000ull;
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double ord2d(uint64_t k) {
  if (k == 0xFFFFFFFFFFFFFFFEull) return __longlong_as_double(0x7FF8000000000000ll);
  const uint64_t b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  return __longlong_as_double((long long)b);
}

// host copy of a small array that may live on either side (the caller synchronises)
template <class T>
inline int to_host(std::vector<T> &h, const T *src, size_t n) {
  h.resize(n);
  if (n) HIP_TRY(hipMemcpyAsync(h.data(), src, n * sizeof(T), hipMemcpyDefault, stream()));
  return ASL_OK;
}

// The limits both calls share, on host copies, before anything is launched or written: peak counts
// (0 .. DC_MAXN, offsets ascending from >= 0 and inside n_peaks when the caller gave it), 2 .. DC_MAXL
// residues, fragment charge 1 .. DC_MAXZ, finite termini. max_n: the largest peak count of the batch.
inline int check_fragment_batch(const char *who, int n, int64_t n_peaks, const std::vector<int32_t> &off,
                                const std::vector<int32_t> &seq, const std::vector<int32_t> &z,
                                const std::vector<double> &nt, const std::vector<double> &ct, int *max_n) {
  if (off[0] < 0 || seq[0] < 0) return fail(ASL_ERR_INVALID, "%s: negative offsets", who);
  *max_n = 0;
  for (int s = 0; s < n; ++s) {
    const int c = off[s + 1] - off[s], L = seq[s + 1] - seq[s];
    if (c < 0) return fail(ASL_ERR_INVALID, "%s: peak offsets descend at spectrum %d", who, s);
    if (c > DC_MAXN) return fail(ASL_ERR_CAPACITY, "%s: spectrum %d has more than %d peaks", who, s, DC_MAXN);
    if (L < 2) return fail(ASL_ERR_INVALID, "%s: spectrum %d: a peptide needs 2 residues or more", who, s);
    if (L > DC_MAXL) return fail(ASL_ERR_CAPACITY, "%s: spectrum %d: more than %d residues", who, s, DC_MAXL);
    if (z[s] < 1) return fail(ASL_ERR_INVALID, "%s: spectrum %d: max_fragment_charge < 1", who, s);
    if (z[s] > DC_MAXZ)
      return fail(ASL_ERR_CAPACITY, "%s: spectrum %d: max_fragment_charge above %d", who, s, DC_MAXZ);
    if (!std::isfinite(nt[s]) || !std::isfinite(ct[s]))
      return fail(ASL_ERR_INVALID, "%s: spectrum %d: non-finite terminal mass", who, s);
    *max_n = c > *max_n ? c : *max_n;
  }
  if (n_peaks > 0 && (int64_t)off[n] > n_peaks) return fail(ASL_ERR_INVALID, "%s: offsets run past n_peaks", who);
  return ASL_OK;
}

}  // namespace asl
