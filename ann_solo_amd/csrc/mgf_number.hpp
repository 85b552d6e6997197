// mgf_number.hpp -- decimal numeral -> double, on the host and on the device, for the MGF reader (mgf.hip).
// DESIGN.md 3 "Query files".
//
// The function converts a numeral only where ONE correctly rounded fp64 operation on exact operands gives the
// correctly rounded value of the numeral, i.e. what Python's float() returns:
//
//   numeral   [+-]? (digits [. digits*] | . digits) ([eE] [+-]? digits)?        -- the whole byte range
//   w         the digits of the significand without the point and without leading zeros: at most 19 of them
//             (so w fits a uint64) and w < 2^53 (so (double)w is exact)
//   e         the decimal exponent of w's last digit: -22 .. 22 (10^|e| is exact in a double)
//   value     w * 10^e (e >= 0) or w / 10^-e (e < 0): exact operands, one IEEE operation, never an FMA
//             w == 0: a signed zero, whatever the exponent
//
// Everything else -- inf, nan, 1_0, 20 digits, w >= 2^53, e = 23, an empty range, a stray byte -- is DEFERRED
// (return 1, *out untouched): the caller hands the token to a full converter. The function never guesses.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MGF_HD __host__ __device__
#else
#define MGF_HD
#endif

namespace asl {

// 0: converted, *out written; 1: deferred
MGF_HD inline int mgf_number(const char *s, int n, double *out) {
  constexpr double p10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                              1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  int i = 0;
  bool neg = false;
  if (i < n && (s[i] == '+' || s[i] == '-')) neg = s[i++] == '-';
  uint64_t w = 0;
  int nd = 0;          // digits of w (leading zeros dropped)
  int seen = 0;        // digits of the significand, zeros included
  int frac = 0;        // digits behind the point
  for (; i < n && s[i] >= '0' && s[i] <= '9'; ++i) {
    ++seen;
    if (nd > 0 || s[i] != '0') {
      if (++nd > 19) return 1;
      w = w * 10u + (uint64_t)(s[i] - '0');
    }
  }
  if (i < n && s[i] == '.') {
    for (++i; i < n && s[i] >= '0' && s[i] <= '9'; ++i) {
      ++seen;
      ++frac;          // (at most n)
      if (nd > 0 || s[i] != '0') {
        if (++nd > 19) return 1;
        w = w * 10u + (uint64_t)(s[i] - '0');
      }
    }
  }
  if (seen == 0) return 1;
  int64_t ex = 0;
  if (i < n && (s[i] == 'e' || s[i] == 'E')) {
    ++i;
    bool eneg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) eneg = s[i++] == '-';
    int ed = 0;
    for (; i < n && s[i] >= '0' && s[i] <= '9'; ++i) {
      ++ed;
      // (exact below 2^40, which no fraction of a token of n < 2^31 bytes brings back into -22 .. 22)
      if (ex < ((int64_t)1 << 40)) ex = ex * 10 + (s[i] - '0');
    }
    if (ed == 0) return 1;
    if (eneg) ex = -ex;
  }
  if (i != n) return 1;
  if (w == 0) {
    *out = neg ? -0.0 : 0.0;
    return 0;
  }
  if (w >= (1ull << 53)) return 1;
  const int64_t e = ex - (int64_t)frac;
  if (e < -22 || e > 22) return 1;
  const double v = e >= 0 ? (double)w * p10[e] : (double)w / p10[-e];
  *out = neg ? -v : v;
  return 0;
}

}  // namespace asl
