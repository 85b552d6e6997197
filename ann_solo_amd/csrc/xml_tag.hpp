// xml_tag.hpp -- one XML tag on the device, for the readers whose unit is a tag (mzml.hip, mzxml.hip): where it ends,
// what its name is, the value of one of its attributes, a value of plain digits. gfx950 only. The readers are no XML
// validators: a tag runs from its '<' to the first '>' outside quotes, and nothing else about it is checked.
#pragma once
#include "text_scan.hpp"

namespace asl {

constexpr uint32_t NONE = ~0u;

// The '>' that ends the tag at a, outside quotes; lim when there is none before lim.
__device__ __forceinline__ uint32_t zm_tag_end(const uint8_t *__restrict__ t, uint32_t a, uint32_t lim) {
  uint8_t quote = 0;
  for (uint32_t i = a + 1u; i < lim; ++i) {
    const uint8_t c = t[i];
    if (quote != 0) {
      if (c == quote) quote = 0;
    } else if (c == '"' || c == '\'') {
      quote = c;
    } else if (c == '>') {
      return i;
    }
  }
  return lim;
}
__device__ __forceinline__ bool zm_is(const uint8_t *__restrict__ t, uint32_t p, uint32_t len, const char *lit,
                                      uint32_t lit_len) {
  if (len != lit_len) return false;
  for (uint32_t k = 0; k < lit_len; ++k)
    if (t[p + k] != (uint8_t)lit[k]) return false;
  return true;
}
// The value [*va, *vb) of attribute `name` among the attributes in [p, e), e the tag's '>'.
__device__ __forceinline__ bool zm_attr(const uint8_t *__restrict__ t, uint32_t p, uint32_t e, const char *name,
                                        uint32_t name_len, uint32_t *va, uint32_t *vb) {
  while (p < e) {
    while (p < e && mg_ws(t[p])) ++p;
    const uint32_t na = p;
    while (p < e && t[p] != '=' && !mg_ws(t[p])) ++p;
    const uint32_t nb = p;
    while (p < e && mg_ws(t[p])) ++p;
    if (p >= e) return false;
    if (t[p] != '=') continue;   // (a name without a value, as the '/' of a self-closing tag: nb > na, so p moved)
    ++p;
    while (p < e && mg_ws(t[p])) ++p;
    if (p >= e) return false;
    const uint8_t quote = t[p];
    if (quote != '"' && quote != '\'') return false;
    const uint32_t a = ++p;
    while (p < e && t[p] != quote) ++p;
    if (p >= e) return false;
    if (zm_is(t, na, nb - na, name, name_len)) {
      *va = a, *vb = p;
      return true;
    }
    ++p;
  }
  return false;
}
// plain digits -> the number (at most 10^9), else NONE
__device__ __forceinline__ uint32_t zm_uint(const uint8_t *__restrict__ t, uint32_t a, uint32_t b) {
  if (a >= b) return NONE;
  uint32_t v = 0u;
  for (; a < b; ++a) {
    if (t[a] < '0' || t[a] > '9' || v > 100000000u) return NONE;
    v = v * 10u + (uint32_t)(t[a] - '0');
  }
  return v;
}

}  // namespace asl
