// inflate.hpp -- base64 and zlib (RFC 1950 around RFC 1951) decoding for the mzML reader (mzml.hip), on the host and
// on the device: the header compiles as plain C++17 too. DESIGN.md 3 "Query files".
//
// The decoder reads from a bounded byte source and writes to a bounded sink: every read is checked against the
// source's length, every write against the sink's capacity, every back-reference against the bytes written so far,
// and every set of code lengths for over-subscription and incompleteness, as zlib's inflate_table checks them (an
// incomplete set is legal only as one single code of one bit, and never for the code-length code). Whatever the
// input, the functions return an error code and touch nothing outside [src, src + n) and [out, out + cap).
//
// The verdict (error or not) is zlib.decompress's: a truncated stream is an error, bytes behind the Adler-32 are
// ignored, the header's window size is checked but distances are not held to it (zlib without INFLATE_STRICT).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define INF_HD __host__ __device__
#else
#define INF_HD
#endif

namespace asl {

enum : int {   // ASL_MZML_INF_* of include/annsolo_mi.h
  INF_OK = 0,
  INF_B64_BYTE = 1,     // a byte that is neither of the alphabet, '=' nor a blank
  INF_B64_LENGTH = 2,   // not a multiple of four characters
  INF_B64_PAD = 3,      // '=' anywhere but as the last one or two characters
  INF_INPUT = 4,        // the decoded stream is longer than the reader takes for the array's length
  INF_HEADER = 5,       // zlib header: CM != 8, window > 32 KiB, FCHECK, FDICT
  INF_BLOCK_TYPE = 6,   // block type 3
  INF_STORED = 7,       // LEN != ~NLEN
  INF_CODES = 8,        // code lengths: counts, repeats, over-subscribed, incomplete, no end-of-block
  INF_SYMBOL = 9,       // a bit pattern that is no code, or a length / distance symbol that does not exist
  INF_DISTANCE = 10,    // a back-reference before the first byte written
  INF_TRUNCATED = 11,   // the source ends inside the stream
  INF_SINK = 12,        // more bytes than the sink holds
  INF_ADLER = 13,       // Adler-32 mismatch
  INF_LENGTH = 14       // fewer bytes than defaultArrayLength promises
};

// ---------------------------------------------------------------------------------------------- base64
constexpr uint32_t B64_PAD = 64, B64_BLANK = 65, B64_BAD = 66;

// 0 .. 63: a character of the standard alphabet; B64_PAD '='; B64_BLANK what bytes.strip strips; B64_BAD the rest
INF_HD inline uint32_t b64_value(uint8_t c) {
  if (c >= 'A' && c <= 'Z') return (uint32_t)(c - 'A');
  if (c >= 'a' && c <= 'z') return (uint32_t)(c - 'a') + 26u;
  if (c >= '0' && c <= '9') return (uint32_t)(c - '0') + 52u;
  if (c == '+') return 62u;
  if (c == '/') return 63u;
  if (c == '=') return B64_PAD;
  if (c == 32 || (c >= 9 && c <= 13)) return B64_BLANK;
  return B64_BAD;
}
// The three bytes of four sextets (a pad counts as 0); o[0 .. 3) must be writable.
INF_HD inline void b64_quad(const uint8_t *v, uint8_t *o) {
  const uint32_t w = ((uint32_t)(v[0] & 63u) << 18) | ((uint32_t)(v[1] & 63u) << 12) | ((uint32_t)(v[2] & 63u) << 6) |
                     (uint32_t)(v[3] & 63u);
  o[0] = (uint8_t)(w >> 16), o[1] = (uint8_t)(w >> 8), o[2] = (uint8_t)w;
}
// After the blanks are dropped: n_chars characters, the first '=' at first_pad (n_chars: none), n_pads of them.
// The length of the decoded stream, or the error.
INF_HD inline int b64_finish(uint32_t n_chars, uint32_t first_pad, uint32_t n_pads, uint32_t *n_out) {
  if (n_chars % 4u != 0u) return INF_B64_LENGTH;
  if (n_pads != 0u && (n_pads > 2u || first_pad + n_pads != n_chars)) return INF_B64_PAD;
  *n_out = n_chars / 4u * 3u - n_pads;
  return INF_OK;
}

// One thread's decoder: s[0 .. n) -> out[0 .. cap), *n_out bytes. A quad needs room for its three bytes.
INF_HD inline int b64_decode(const uint8_t *s, uint32_t n, uint8_t *out, uint32_t cap, uint32_t *n_out) {
  uint8_t q[4];
  uint32_t k = 0, o = 0, chars = 0, first_pad = 0, pads = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t v = b64_value(s[i]);
    if (v == B64_BLANK) continue;
    if (v == B64_BAD) return INF_B64_BYTE;
    if (v == B64_PAD && pads++ == 0u) first_pad = chars;
    ++chars;
    q[k++] = (uint8_t)v;
    if (k == 4u) {
      if (o + 3u > cap) return INF_INPUT;
      b64_quad(q, out + o);
      o += 3u, k = 0;
    }
  }
  return b64_finish(chars, pads != 0u ? first_pad : chars, pads, n_out);
}

// ---------------------------------------------------------------------------------------------- inflate
struct InfWork {   // the decoder's tables: LDS on the device, the stack on the host
  uint16_t lcount[16], lsym[288], dcount[16], dsym[32], lens[320];
};

struct InfSrc {
  const uint8_t *p;
  uint32_t n, pos, buf;
  int cnt;   // bits in buf: below 8 between calls
};

// need <= 16
INF_HD inline int inf_bits(InfSrc &s, int need, uint32_t *out) {
  while (s.cnt < need) {
    if (s.pos >= s.n) return INF_TRUNCATED;
    s.buf |= (uint32_t)s.p[s.pos++] << s.cnt;
    s.cnt += 8;
  }
  *out = s.buf & ((1u << need) - 1u);
  s.buf >>= need;
  s.cnt -= need;
  return INF_OK;
}

// Canonical code of length[0 .. n) (each 0 .. 15): count[len] and the symbols in code order. Returns the code space
// left over: 0 complete, > 0 incomplete, < 0 over-subscribed. n <= 288.
INF_HD inline int inf_construct(uint16_t *count, uint16_t *symbol, const uint16_t *length, int n) {
  uint16_t offs[16];
  for (int l = 0; l < 16; ++l) count[l] = 0;
  for (int s = 0; s < n; ++s) ++count[length[s] & 15u];
  if (count[0] == n) return 0;   // no codes at all: nothing can be decoded, which the caller may allow
  int left = 1;
  for (int l = 1; l < 16; ++l) {
    left <<= 1;
    left -= (int)count[l];
    if (left < 0) return left;
  }
  offs[1] = 0;
  for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
  for (int s = 0; s < n; ++s)
    if ((length[s] & 15u) != 0u) symbol[offs[length[s] & 15u]++] = (uint16_t)s;
  return left;
}
// zlib's rule for a literal/length or distance set: complete, or one single code of one bit
INF_HD inline bool inf_set_ok(const uint16_t *count, int n, int left) {
  return left == 0 || (left > 0 && (int)count[0] + (int)count[1] == n && count[1] == 1);
}

INF_HD inline int inf_decode(InfSrc &s, const uint16_t *count, const uint16_t *symbol, uint32_t *sym) {
  int code = 0, first = 0, index = 0;
  for (int l = 1; l < 16; ++l) {
    uint32_t b;
    const int rc = inf_bits(s, 1, &b);
    if (rc != INF_OK) return rc;
    code |= (int)b;
    const int c = (int)count[l];
    if (code - c < first) {
      *sym = symbol[index + (code - first)];   // (index + code - first < the number of codes)
      return INF_OK;
    }
    index += c, first += c;
    first <<= 1, code <<= 1;
  }
  return INF_SYMBOL;
}

INF_HD inline uint32_t inf_adler32(const uint8_t *p, uint32_t n) {
  uint32_t a = 1u, b = 0u, i = 0u;
  while (i < n) {
    const uint32_t stop = n - i > 5552u ? i + 5552u : n;   // (the sums stay below 2^32 for 5552 bytes)
    for (; i < stop; ++i) a += p[i], b += a;
    a %= 65521u, b %= 65521u;
  }
  return (b << 16) | a;
}

// The blocks of one stream, literal by literal and match by match.
INF_HD inline int inf_blocks(InfSrc &s, uint8_t *out, uint32_t cap, uint32_t *n_out, InfWork *w) {
  constexpr uint16_t lbase[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                  31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
  constexpr uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  constexpr uint16_t dbase[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                  193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
  constexpr uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2,  3,  3,  4,  4,  5,  5,  6,
                                6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
  constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint32_t o = 0, last = 0, v = 0;
  int rc;
  while (last == 0u) {
    if ((rc = inf_bits(s, 1, &last)) != INF_OK) return rc;
    uint32_t type;
    if ((rc = inf_bits(s, 2, &type)) != INF_OK) return rc;
    if (type == 3u) return INF_BLOCK_TYPE;
    if (type == 0u) {
      s.buf = 0u, s.cnt = 0;   // (fewer than 8 bits: the rest of the current byte)
      if (s.n - s.pos < 4u) return INF_TRUNCATED;
      const uint32_t len = (uint32_t)s.p[s.pos] | ((uint32_t)s.p[s.pos + 1] << 8);
      const uint32_t nlen = (uint32_t)s.p[s.pos + 2] | ((uint32_t)s.p[s.pos + 3] << 8);
      s.pos += 4u;
      if (len != (~nlen & 0xffffu)) return INF_STORED;
      if (s.n - s.pos < len) return INF_TRUNCATED;
      if (cap - o < len) return INF_SINK;
      for (uint32_t k = 0; k < len; ++k) out[o + k] = s.p[s.pos + k];
      o += len, s.pos += len;
      continue;
    }
    if (type == 1u) {
      for (int k = 0; k < 288; ++k) w->lens[k] = (uint16_t)(k < 144 ? 8 : k < 256 ? 9 : k < 280 ? 7 : 8);
      inf_construct(w->lcount, w->lsym, w->lens, 288);
      for (int k = 0; k < 30; ++k) w->lens[k] = 5;
      inf_construct(w->dcount, w->dsym, w->lens, 30);   // (codes 30 and 31 do not exist: no symbol)
    } else {
      uint32_t nlen, ndist, ncode;
      if ((rc = inf_bits(s, 5, &nlen)) != INF_OK) return rc;
      if ((rc = inf_bits(s, 5, &ndist)) != INF_OK) return rc;
      if ((rc = inf_bits(s, 4, &ncode)) != INF_OK) return rc;
      nlen += 257u, ndist += 1u, ncode += 4u;
      if (nlen > 286u || ndist > 30u) return INF_CODES;
      for (uint32_t k = 0; k < 19u; ++k) w->lens[k] = 0;
      for (uint32_t k = 0; k < ncode; ++k) {
        if ((rc = inf_bits(s, 3, &v)) != INF_OK) return rc;
        w->lens[order[k]] = (uint16_t)v;
      }
      if (inf_construct(w->lcount, w->lsym, w->lens, 19) != 0) return INF_CODES;
      uint32_t idx = 0;
      while (idx < nlen + ndist) {
        uint32_t sym;
        if ((rc = inf_decode(s, w->lcount, w->lsym, &sym)) != INF_OK) return rc;
        if (sym < 16u) {
          w->lens[idx++] = (uint16_t)sym;
          continue;
        }
        uint32_t prev = 0, rep;
        if (sym == 16u) {
          if (idx == 0u) return INF_CODES;
          prev = w->lens[idx - 1u];
          if ((rc = inf_bits(s, 2, &rep)) != INF_OK) return rc;
          rep += 3u;
        } else if (sym == 17u) {
          if ((rc = inf_bits(s, 3, &rep)) != INF_OK) return rc;
          rep += 3u;
        } else {
          if ((rc = inf_bits(s, 7, &rep)) != INF_OK) return rc;
          rep += 11u;
        }
        if (idx + rep > nlen + ndist) return INF_CODES;
        while (rep-- != 0u) w->lens[idx++] = (uint16_t)prev;
      }
      if (w->lens[256] == 0u) return INF_CODES;
      int left = inf_construct(w->lcount, w->lsym, w->lens, (int)nlen);
      if (!inf_set_ok(w->lcount, (int)nlen, left)) return INF_CODES;
      left = inf_construct(w->dcount, w->dsym, w->lens + nlen, (int)ndist);
      if (!inf_set_ok(w->dcount, (int)ndist, left)) return INF_CODES;
    }
    for (;;) {
      uint32_t sym;
      if ((rc = inf_decode(s, w->lcount, w->lsym, &sym)) != INF_OK) return rc;
      if (sym < 256u) {
        if (o >= cap) return INF_SINK;
        out[o++] = (uint8_t)sym;
        continue;
      }
      if (sym == 256u) break;
      sym -= 257u;
      if (sym >= 29u) return INF_SYMBOL;
      if ((rc = inf_bits(s, lext[sym], &v)) != INF_OK) return rc;
      const uint32_t len = lbase[sym] + v;
      uint32_t ds;
      if ((rc = inf_decode(s, w->dcount, w->dsym, &ds)) != INF_OK) return rc;
      if (ds >= 30u) return INF_SYMBOL;
      if ((rc = inf_bits(s, dext[ds], &v)) != INF_OK) return rc;
      const uint32_t dist = dbase[ds] + v;
      if (dist > o) return INF_DISTANCE;
      if (cap - o < len) return INF_SINK;
      for (uint32_t k = 0; k < len; ++k) out[o + k] = out[o + k - dist];   // (overlapping: byte by byte)
      o += len;
    }
  }
  *n_out = o;
  return INF_OK;
}

// src[0 .. n): one zlib stream. out[0 .. cap) receives its bytes, *n_out of them.
INF_HD inline int inf_inflate(const uint8_t *src, uint32_t n, uint8_t *out, uint32_t cap, uint32_t *n_out,
                              InfWork *w) {
  if (n < 2u) return INF_TRUNCATED;
  const uint32_t cmf = src[0], flg = src[1];
  if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u) != 0u) return INF_HEADER;
  InfSrc s = {src, n, 2u, 0u, 0};
  uint32_t o = 0;
  const int rc = inf_blocks(s, out, cap, &o, w);
  if (rc != INF_OK) return rc;
  if (s.n - s.pos < 4u) return INF_TRUNCATED;   // (the bits left in buf belong to the last block's last byte)
  const uint32_t want = ((uint32_t)s.p[s.pos] << 24) | ((uint32_t)s.p[s.pos + 1] << 16) |
                        ((uint32_t)s.p[s.pos + 2] << 8) | (uint32_t)s.p[s.pos + 3];
  if (inf_adler32(out, o) != want) return INF_ADLER;
  *n_out = o;
  return INF_OK;
}

// One array by one thread: the characters b64[0 .. n) -> out[0 .. cap). tmp[0 .. tmp_cap) receives the decoded
// base64, which is the zlib stream (zlib != 0) or the array itself.
INF_HD inline int inf_array(const uint8_t *b64, uint32_t n, int zlib, uint8_t *tmp, uint32_t tmp_cap, uint8_t *out,
                            uint32_t cap, uint32_t *n_out, InfWork *w) {
  uint32_t m = 0;
  const int rc = b64_decode(b64, n, tmp, tmp_cap, &m);
  if (rc != INF_OK) return rc;
  if (zlib != 0) return inf_inflate(tmp, m, out, cap, n_out, w);
  if (m > cap) return INF_SINK;
  for (uint32_t k = 0; k < m; ++k) out[k] = tmp[k];
  *n_out = m;
  return INF_OK;
}

}  // namespace asl
