// The deflate code-table builder and its accept / reject rules (RFC 1951 section 3.2.2, with zlib's verdicts), shared
// by the host entry vge_inflate_check_lengths (vge_ingest.cpp) and the device inflate kernel (vge_inflate.hip) so that
// the rules exist once: what the CPU tests pin against zlib is the code the kernel runs.  Plain integer code over
// caller-provided arrays; it allocates nothing and reads nothing outside lens[0, n).
//
// zlib's verdict on a set of code lengths (inflate_table in inftrees.c):
//   over-subscribed (Kraft sum above 1)            reject, every kind
//   incomplete (Kraft sum below 1)                 reject -- except a length/literal or distance set whose longest
//                                                  code is 1 bit (one symbol, one 1-bit code): accepted, and its unused
//                                                  code is an error only when a stream meets it
//   no code at all                                 accepted for a distance set (any distance code met is an error);
//                                                  a length/literal set cannot be empty (symbol 256 needs a code, which
//                                                  the caller checks); an empty code-length code is rejected here: zlib
//                                                  builds it but then reads every length as 0 and rejects the block for
//                                                  its missing end-of-block code, so the stream's verdict is the same
#ifndef VGE_INFLATE_TABLES_H
#define VGE_INFLATE_TABLES_H

#include <stdint.h>

#if defined(__HIPCC__)
#define VGE_INF_HD __host__ __device__ inline
#else
#define VGE_INF_HD inline
#endif

namespace vge_inflate {

enum { KIND_CODES = 0, KIND_LENS = 1, KIND_DISTS = 2 };
enum { MAX_BITS = 15, MAX_LITLEN = 288, MAX_LENS = 320 /* 288 + 32 */ };

// Canonical code of one alphabet: the symbols sorted by (length, value); a code of length l is the l stream bits read
// most significant first; the codes of length l are first[l] .. first[l] + count[l] - 1 and belong to
// sym[offs[l]] .. in that order.
struct Table {
  uint16_t count[16];
  uint16_t first[16];
  uint16_t offs[16];
  uint16_t sym[MAX_LITLEN];
};
static_assert(sizeof(Table) % 4 == 0, "Table lives in LDS beside dword arrays");

// lens[n] (each 0..15, n <= 288) -> t; returns 0 when zlib accepts the set, non-zero when it rejects it (see above).
VGE_INF_HD int build_table(Table& t, const uint8_t* lens, int n, int kind) {
  for (int l = 0; l <= MAX_BITS; ++l) t.count[l] = 0;
  for (int s = 0; s < n; ++s) t.count[lens[s] & 15]++;
  int maxlen = MAX_BITS;
  while (maxlen >= 1 && t.count[maxlen] == 0) --maxlen;
  int left = 1;
  for (int l = 1; l <= MAX_BITS; ++l) {
    left = (left << 1) - (int)t.count[l];
    if (left < 0) return 1;  // over-subscribed
  }
  if (maxlen == 0) {
    if (kind == KIND_CODES) return 1;
  } else if (left > 0 && (kind == KIND_CODES || maxlen != 1)) {
    return 1;  // incomplete
  }
  int code = 0, k = 0;
  t.first[0] = 0;
  t.offs[0] = 0;
  for (int l = 1; l <= MAX_BITS; ++l) {
    code = (code + (int)t.count[l - 1] * (l > 1)) << 1;
    t.first[l] = (uint16_t)code;
    t.offs[l] = (uint16_t)k;
    k += t.count[l];
  }
  for (int s = 0; s < n; ++s) {  // offs[] serve as the cursors (no private array: the device has no scratch to index)
    const int l = lens[s] & 15;
    if (l) t.sym[t.offs[l]++] = (uint16_t)s;
  }
  for (int l = 1; l <= MAX_BITS; ++l) t.offs[l] = (uint16_t)(t.offs[l] - t.count[l]);
  return 0;
}

// Decode one symbol from `msb`, the next `nbits` (<= 15) stream bits with the first bit most significant.  Returns
// (symbol << 4) | length, or 0 when no code of up to nbits bits matches (a longer code, or the unused code of an
// incomplete set).
VGE_INF_HD uint32_t decode_msb(const Table& t, uint32_t msb, int nbits) {
  for (int l = 1; l <= nbits; ++l) {
    const uint32_t c = msb >> (nbits - l);
    const uint32_t k = c - t.first[l];
    if (c >= t.first[l] && k < t.count[l]) return ((uint32_t)t.sym[t.offs[l] + k] << 4) | (uint32_t)l;
  }
  return 0;
}

// The low `nbits` of v in reverse order: stream bits (least significant first) -> a code's reading order.
VGE_INF_HD uint32_t reverse_bits(uint32_t v, int nbits) {
  uint32_t r = 0;
  for (int i = 0; i < nbits; ++i) r |= ((v >> i) & 1u) << (nbits - 1 - i);
  return r;
}

// Length and distance symbols: base value and extra bits (RFC 1951 section 3.2.5), in closed form.  Length symbols
// 257..285 are indices 0..28; 286 and 287, and distance symbols 30 and 31, have no value and are rejected where met.
VGE_INF_HD int length_extra(int i) { return i < 8 || i == 28 ? 0 : (i - 4) >> 2; }
VGE_INF_HD int length_base(int i) { return i < 8 ? 3 + i : i == 28 ? 258 : 3 + ((4 + (i & 3)) << length_extra(i)); }
VGE_INF_HD int dist_extra(int i) { return i < 4 ? 0 : (i - 2) >> 1; }
VGE_INF_HD int dist_base(int i) { return i < 4 ? 1 + i : 1 + ((2 + (i & 1)) << dist_extra(i)); }

// The fixed code's lengths (section 3.2.6): 288 length/literal lengths then 32 distance lengths (30 and 31 take part
// in the code but are invalid where met).
VGE_INF_HD int fixed_length(int s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5; }

// Order in which a dynamic header sends the code-length code's lengths.
VGE_INF_HD int clen_order(int i) {
  constexpr uint8_t o[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return o[i];
}

}  // namespace vge_inflate
#endif  // VGE_INFLATE_TABLES_H
