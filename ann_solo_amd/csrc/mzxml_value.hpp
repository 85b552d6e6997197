// mzxml_value.hpp -- the two value rules of the mzXML reader (mzxml.hip) that the host runs too: a retentionTime
// attribute -> minutes, and one decoded <peaks> stream -> the two float32 columns. The header compiles as plain C++17
// (asl_mzxml_duration, asl_mzxml_pairs; tests/native/mzxml_check.cpp). DESIGN.md 3 "Query files".
#pragma once
#include <cstdint>

#include "mgf_number.hpp"

namespace asl {

// s[0 .. n): the value of a retentionTime attribute. 0: converted, *minutes written; 1: deferred to the host's rule
// (ann_solo_amd/mzxml.py duration_minutes), *minutes untouched.
//   PT<seconds>S, <seconds> = digits [. digits*]   the numeral by mgf_number, then ONE fp64 division by 60.0; a
//                                                  numeral mgf_number defers defers the whole value
//   anything else that begins with 'P'             deferred: hours, minutes, a date part, no duration at all
//   anything else                                  the numeral as written by mgf_number (minutes), or deferred
MGF_HD inline int mzx_duration(const char *s, int n, double *minutes) {
  if (n <= 0 || s[0] != 'P') return mgf_number(s, n, minutes);
  if (n < 4 || s[1] != 'T' || s[n - 1] != 'S') return 1;
  int i = 2, digits = 0;
  for (; i < n - 1 && s[i] >= '0' && s[i] <= '9'; ++i) ++digits;
  if (digits == 0) return 1;
  if (i < n - 1 && s[i] == '.')
    for (++i; i < n - 1 && s[i] >= '0' && s[i] <= '9'; ++i) {
    }
  if (i != n - 1) return 1;   // (a sign, an exponent, a blank: not the plain form)
  double seconds = 0.0;
  if (mgf_number(s + 2, n - 3, &seconds) != 0) return 1;
  *minutes = seconds / 60.0;
  return 0;
}

// Peak i of a decoded stream: big-endian (m/z, intensity) pairs of width 4 (float32: the bits as they are) or 8
// (float64 -> float32 by round-to-nearest). raw need not be aligned.
MGF_HD inline void mzx_pair(const uint8_t *raw, uint32_t i, uint32_t width, float *mz, float *intensity) {
  float *const dst[2] = {mz, intensity};
  for (uint32_t j = 0; j < 2u; ++j) {
    const uint8_t *p = raw + (size_t)(2u * i + j) * width;
    if (width == 8u) {
      uint64_t w = 0;
      for (int k = 0; k < 8; ++k) w = (w << 8) | p[k];
      double d;
      __builtin_memcpy(&d, &w, 8);
      *dst[j] = (float)d;
    } else {
      const uint32_t w = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
      __builtin_memcpy(dst[j], &w, 4);
    }
  }
}

}  // namespace asl
