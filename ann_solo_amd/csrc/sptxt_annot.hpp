// sptxt_annot.hpp -- the fragment charge of a .sptxt peak annotation, on the host and on the device, for the
// library reader (sptxt.hip). include/annsolo_mi.h "Library files" states the rule; tests/sptxt_ref.py restates it.
#pragma once
#include <cstdint>

#include "mgf_number.hpp"   // MGF_HD

namespace asl {

// s[0 .. n): the annotation field of a peak line. 0: unannotated (empty, or a first byte other than a b y p).
// Else the leading digits behind the first '^' before the first '/', at most 255; 1 without '^' or digits there.
MGF_HD inline int sptxt_fragment_charge(const char *s, int n) {
  if (n <= 0) return 0;
  const char c = s[0];
  if (c != 'a' && c != 'b' && c != 'y' && c != 'p') return 0;
  int i = 1;
  while (i < n && s[i] != '/' && s[i] != '^') ++i;
  if (i >= n || s[i] == '/') return 1;
  int v = 0, nd = 0;
  for (++i; i < n && s[i] >= '0' && s[i] <= '9'; ++i, ++nd)
    if (v < 1000) v = v * 10 + (s[i] - '0');
  if (nd == 0) return 1;
  return v > 255 ? 255 : v;
}

}  // namespace asl
