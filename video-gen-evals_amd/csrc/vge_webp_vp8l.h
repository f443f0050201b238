// The rules of the lossless WebP (VP8L) decoders, compiled for both sides (as vge_gif_lzw.h holds GIF's): the bit
// reader, the code-length reader, the canonical-code build and symbol decode, the length / distance tables and the
// distance map, the entropy decode of an image and its sub-images, the per-pixel inverse-transform steps and the
// per-pixel composition step.  The host decoder (vge_webp.cpp) and the kernels (vge_webp.hip) call these and nothing
// else for the format's logic, so they cannot drift apart, and the logic can be stepped through on a CPU build.
//
// Nothing here allocates.  A frame decodes into caller-provided storage: two ARGB planes, an arena (Arena below) that
// holds the frame's header for the inverse transforms, the transform data, the entropy image and the prefix-code
// tables of the groups, and a scratch block (Scratch: the colour cache, the code lengths being read and the current
// group's code headers; LDS on the device).  The capacities are part of the format this project accepts
// (include/vge_webp.h): a frame that needs more groups or more table space than the arena has is refused with
// VGE_WEBP_ERR_GROUPS by whoever decodes it.
#pragma once
#include <stdint.h>

#include "../../include/vge_webp.h"

#if defined(__HIPCC__)
#define VGE_WEBP_HD __host__ __device__
#else
#define VGE_WEBP_HD
#endif

namespace vge_webp {

constexpr int MAX_GROUPS = VGE_WEBP_MAX_GROUPS;
constexpr int SYM_CAP = VGE_WEBP_TABLE_SYMBOLS;  // sorted symbols of all groups of a frame
constexpr int MAX_CACHE_BITS = 11;
constexpr int GREEN_BASE = 256 + 24;
constexpr int MAX_ALPHABET = GREEN_BASE + (1 << MAX_CACHE_BITS);
constexpr int MAX_LEN = 15;

enum { T_PREDICTOR = 0, T_CROSS_COLOR = 1, T_SUB_GREEN = 2, T_INDEXING = 3 };

// What a file exercised (host only; the coverage assertion of the tests).
enum : uint64_t {
  F_PRED0 = 1ull << 0,  // .. F_PRED0 << 13: predictor modes met on a pixel they decide (x > 0, y > 0)
  F_XFORM0 = 1ull << 14,  // .. << 17: the four transforms
  F_SIMPLE1 = 1ull << 18, F_SIMPLE2 = 1ull << 19, F_ZERO_BIT = 1ull << 20, F_NORMAL = 1ull << 21,
  F_MAX_SYMBOL = 1ull << 22, F_REP16 = 1ull << 23, F_REP16_FIRST = 1ull << 24, F_REP17 = 1ull << 25,
  F_REP18 = 1ull << 26, F_CACHE = 1ull << 27, F_CACHE_SUB = 1ull << 28, F_META = 1ull << 29, F_COPY = 1ull << 30,
  F_DIST_MAP = 1ull << 31, F_DIST_PLAIN = 1ull << 32, F_DIST_CLAMP = 1ull << 33, F_MANY_GROUPS = 1ull << 34,
  F_BUNDLE8 = 1ull << 35, F_BUNDLE4 = 1ull << 36, F_BUNDLE2 = 1ull << 37, F_INDEX_OOB = 1ull << 38,
  F_COPY_OVERLAP = 1ull << 39, F_COPY_FAR = 1ull << 40,  // distance < length; distance > 32768
  F_CACHE_HIT = 1ull << 41, F_TRAILING = 1ull << 42, F_ALL_XFORMS = 1ull << 43
};
struct Stats {
  uint64_t features;
  uint64_t dist_codes[2];  // distance-map codes 1..120 met, bit code - 1
  uint64_t max_groups;
};

struct BitReader {
  const uint8_t* p;
  uint32_t n;    // bytes (< 2^28)
  uint32_t pos;  // bits consumed
  int32_t eos;   // a read went past the end: the frame fails, whatever else happens
};

// The next 32 - 7 = 25 or more bits, zeros beyond the end.
VGE_WEBP_HD inline uint32_t peek(const BitReader& b) {
  const uint32_t at = b.pos >> 3;
  uint64_t v = 0;
  if (at + 5 <= b.n) {
    v = (uint64_t)b.p[at] | ((uint64_t)b.p[at + 1] << 8) | ((uint64_t)b.p[at + 2] << 16) |
        ((uint64_t)b.p[at + 3] << 24) | ((uint64_t)b.p[at + 4] << 32);
  } else {
    for (uint32_t k = 0; k < 5 && at + k < b.n; ++k) v |= (uint64_t)b.p[at + k] << (8 * k);
  }
  return (uint32_t)(v >> (b.pos & 7));
}
VGE_WEBP_HD inline void skip(BitReader& b, int n) {
  if (b.pos + (uint32_t)n > b.n * 8u) {
    b.eos = 1;
    b.pos = b.n * 8u;
  } else {
    b.pos += (uint32_t)n;
  }
}
VGE_WEBP_HD inline uint32_t read_bits(BitReader& b, int n) {  // n <= 24
  const uint32_t v = peek(b) & ((1u << n) - 1);
  skip(b, n);
  return b.eos ? 0 : v;
}

// One canonical prefix code: the number of codes of each length and the symbols in code order (by length, then by
// value), as deflate's.  A code with one symbol consumes no bits.
struct Code {
  uint16_t count[MAX_LEN + 1];
  uint16_t n_syms;
  uint16_t single;
  uint32_t sym_off;  // into the symbol store
};
struct Group {
  Code c[5];  // green + length + cache, red, blue, alpha, distance
};

VGE_WEBP_HD inline int alphabet_size(int k, int cache_bits) {
  return k == 0 ? GREEN_BASE + (cache_bits > 0 ? 1 << cache_bits : 0) : k == 4 ? 40 : 256;
}

// lens[n] -> code.  libwebp's rule: no symbol at all is an error, one symbol of any length is the zero-bit code, and
// any other set must be complete: neither over-subscribed nor incomplete.  Returns 0, VGE_WEBP_ERR_IO or
// VGE_WEBP_ERR_GROUPS (the symbol store is full).
VGE_WEBP_HD inline int build_code(const uint8_t* lens, int n, Code& c, uint16_t* syms, uint32_t& used, uint32_t cap) {
  for (int l = 0; l <= MAX_LEN; ++l) c.count[l] = 0;
  int nz = 0, last = 0;
  for (int s = 0; s < n; ++s)
    if (lens[s]) {
      c.count[lens[s]]++;
      nz++;
      last = s;
    }
  c.n_syms = (uint16_t)nz;
  c.single = (uint16_t)last;
  c.sym_off = used;
  if (nz == 0) return VGE_WEBP_ERR_IO;
  if (nz == 1) return 0;
  int left = 1;
  for (int l = 1; l <= MAX_LEN; ++l) {
    left = (left << 1) - c.count[l];
    if (left < 0) return VGE_WEBP_ERR_IO;  // over-subscribed
  }
  if (left != 0) return VGE_WEBP_ERR_IO;  // incomplete
  if ((uint32_t)nz > cap - used) return VGE_WEBP_ERR_GROUPS;
  uint16_t offs[MAX_LEN + 2];
  offs[1] = 0;
  for (int l = 1; l <= MAX_LEN; ++l) offs[l + 1] = (uint16_t)(offs[l] + c.count[l]);
  for (int s = 0; s < n; ++s)
    if (lens[s]) syms[used + offs[lens[s]]++] = (uint16_t)s;
  used += (uint32_t)nz;
  return 0;
}

// One symbol.  A complete code always ends within 15 bits; bits beyond the end of the data read as zeros and set eos.
VGE_WEBP_HD inline int read_symbol(BitReader& b, const Code& c, const uint16_t* syms) {
  if (c.n_syms <= 1) return c.single;
  uint32_t v = peek(b);
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= MAX_LEN; ++l) {
    code |= (int)(v & 1);
    v >>= 1;
    const int cnt = c.count[l];
    if (code - cnt < first) {
      skip(b, l);
      return syms[c.sym_off + (uint32_t)(index + (code - first))];
    }
    index += cnt;
    first = (first + cnt) << 1;
    code <<= 1;
  }
  skip(b, MAX_LEN);
  b.eos = 1;  // unreachable for a complete code
  return 0;
}

struct Scratch {
  uint32_t cache[1 << MAX_CACHE_BITS];
  Group cur;              // the group in use (a copy: the arena is global memory on the device)
  Code clc;               // the code-length code
  uint16_t clc_syms[20];
  uint8_t lens[MAX_ALPHABET];
};

VGE_WEBP_HD inline void note(Stats* st, uint64_t f) {
#if !defined(__HIP_DEVICE_COMPILE__)
  if (st) st->features |= f;
#endif
}

// One prefix code of alphabet n, in either form, into c.
VGE_WEBP_HD inline int read_code(BitReader& b, int n, Scratch& S, Code& c, uint16_t* syms, uint32_t& used,
                                 uint32_t cap, Stats* st) {
  uint8_t* lens = S.lens;
  for (int s = 0; s < n; ++s) lens[s] = 0;
  if (read_bits(b, 1)) {  // simple: one or two symbols of length 1
    const int two = (int)read_bits(b, 1);
    const int first_bits = read_bits(b, 1) ? 8 : 1;
    lens[read_bits(b, first_bits)] = 1;  // < 256 <= n
    if (two) lens[read_bits(b, 8)] = 1;
    note(st, two ? F_SIMPLE2 : F_SIMPLE1);
  } else {
    const uint8_t order[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
    uint8_t cl[19];
    for (int k = 0; k < 19; ++k) cl[k] = 0;
    const int num = 4 + (int)read_bits(b, 4);
    for (int k = 0; k < num; ++k) cl[order[k]] = (uint8_t)read_bits(b, 3);
    uint32_t clc_used = 0;
    if (build_code(cl, 19, S.clc, S.clc_syms, clc_used, 20) != 0) return VGE_WEBP_ERR_IO;
    int max_symbol = n;
    if (read_bits(b, 1)) {
      const int nbits = 2 + 2 * (int)read_bits(b, 3);
      max_symbol = 2 + (int)read_bits(b, nbits);
      if (max_symbol > n) return VGE_WEBP_ERR_IO;
      note(st, F_MAX_SYMBOL);
    }
    int s = 0, prev = 8;
    bool any_nonzero = false;
    while (s < n) {  // every round consumes a token of max_symbol or advances s
      if (max_symbol-- == 0) break;
      const int len = read_symbol(b, S.clc, S.clc_syms);
      if (b.eos) return VGE_WEBP_ERR_IO;
      if (len < 16) {
        lens[s++] = (uint8_t)len;
        if (len) {
          prev = len;
          any_nonzero = true;
        }
      } else {
        const int extra = len == 16 ? 2 : len == 17 ? 3 : 7;
        const int repeat = (int)read_bits(b, extra) + (len == 18 ? 11 : 3);
        if (s + repeat > n) return VGE_WEBP_ERR_IO;
        const int v = len == 16 ? prev : 0;
        for (int k = 0; k < repeat; ++k) lens[s++] = (uint8_t)v;
        note(st, len == 16 ? (any_nonzero ? F_REP16 : F_REP16 | F_REP16_FIRST) : len == 17 ? F_REP17 : F_REP18);
      }
    }
    note(st, F_NORMAL);
  }
  if (b.eos) return VGE_WEBP_ERR_IO;
  const int r = build_code(lens, n, c, syms, used, cap);
  if (r == 0 && c.n_syms == 1) note(st, F_ZERO_BIT);
  return r;
}

VGE_WEBP_HD inline int read_group(BitReader& b, int cache_bits, Scratch& S, Group& g, uint16_t* syms, uint32_t& used,
                                  uint32_t cap, Stats* st) {
  for (int k = 0; k < 5; ++k) {
    const int r = read_code(b, alphabet_size(k, cache_bits), S, g.c[k], syms, used, cap, st);
    if (r != 0) return r;
  }
  return 0;
}

// Length and distance prefix symbols: value = offset + extra bits.
VGE_WEBP_HD inline int read_lz_value(BitReader& b, int sym) {
  if (sym < 4) return sym + 1;
  const int extra = (sym - 2) >> 1;
  const int offset = (2 + (sym & 1)) << extra;
  return offset + (int)read_bits(b, extra) + 1;
}

// The 120 short distance codes: (dx, dy) neighbours, packed as libwebp packs them (yoffset << 4 | 8 - xoffset).
VGE_WEBP_HD inline int map_distance(int width, int code, Stats* st) {
  const uint8_t kMap[120] = {
      0x18, 0x07, 0x17, 0x19, 0x28, 0x06, 0x27, 0x29, 0x16, 0x1a, 0x26, 0x2a, 0x38, 0x05, 0x37, 0x39, 0x15, 0x1b, 0x36,
      0x3a, 0x25, 0x2b, 0x48, 0x04, 0x47, 0x49, 0x14, 0x1c, 0x35, 0x3b, 0x46, 0x4a, 0x24, 0x2c, 0x58, 0x45, 0x4b, 0x34,
      0x3c, 0x03, 0x57, 0x59, 0x13, 0x1d, 0x56, 0x5a, 0x23, 0x2d, 0x44, 0x4c, 0x55, 0x5b, 0x33, 0x3d, 0x68, 0x02, 0x67,
      0x69, 0x12, 0x1e, 0x66, 0x6a, 0x22, 0x2e, 0x54, 0x5c, 0x43, 0x4d, 0x65, 0x6b, 0x32, 0x3e, 0x78, 0x01, 0x77, 0x79,
      0x53, 0x5d, 0x11, 0x1f, 0x64, 0x6c, 0x42, 0x4e, 0x76, 0x7a, 0x21, 0x2f, 0x75, 0x7b, 0x31, 0x3f, 0x63, 0x6d, 0x52,
      0x5e, 0x00, 0x74, 0x7c, 0x41, 0x4f, 0x10, 0x20, 0x62, 0x6e, 0x30, 0x73, 0x7d, 0x51, 0x5f, 0x40, 0x72, 0x7e, 0x61,
      0x6f, 0x50, 0x71, 0x7f, 0x60, 0x70};
  if (code > 120) {
    note(st, F_DIST_PLAIN);
    return code - 120;
  }
  const int packed = kMap[code - 1];
  const int dist = (packed >> 4) * width + (8 - (packed & 0xf));
#if !defined(__HIP_DEVICE_COMPILE__)
  if (st) {
    st->features |= F_DIST_MAP | (dist < 1 ? F_DIST_CLAMP : 0);
    st->dist_codes[(code - 1) >> 6] |= 1ull << ((code - 1) & 63);
  }
#endif
  return dist >= 1 ? dist : 1;
}

VGE_WEBP_HD inline int sub_size(int v, int bits) { return (v + (1 << bits) - 1) >> bits; }

// What the entropy stage leaves for the inverse transforms.
struct Xform {
  int32_t type, bits;
  int32_t xsize;     // the width the transform applies to (for colour indexing: the width it produces)
  int32_t data_off;  // its data in Arena::sub
  int32_t aux;       // colour indexing: the palette's size
};
struct FrameHdr {
  int32_t n_xforms;
  int32_t in_b;    // the coded image is in plane B (a colour-indexing transform expands it into plane A)
  int32_t xsize;   // the coded image's width (bundled when colour indexing packs pixels)
  int32_t n_groups;
  Xform x[4];
};

// Per frame, in the workspace on the device.  sub holds the palette (256) and up to three sub-images.
struct Arena {
  FrameHdr* hdr;
  uint32_t* sub;
  uint32_t sub_cap;
  Group* groups;   // MAX_GROUPS
  uint16_t* syms;  // SYM_CAP
};
VGE_WEBP_HD inline int64_t arena_sub_cap(int w, int h) {
  return 256 + 3 * (int64_t)sub_size(w, 2) * sub_size(h, 2);
}
VGE_WEBP_HD inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }
// Byte layout of a frame's slot: plane A, plane B, header, sub, groups, symbols; each 16-aligned.
struct SlotLayout {
  int64_t plane_a, plane_b, hdr, sub, groups, syms, bytes;
};
VGE_WEBP_HD inline SlotLayout slot_layout(int w, int h) {
  SlotLayout L;
  const int64_t plane = align16((int64_t)w * h * 4);
  L.plane_a = 0;
  L.plane_b = plane;
  L.hdr = 2 * plane;
  L.sub = L.hdr + align16((int64_t)sizeof(FrameHdr));
  L.groups = L.sub + align16(arena_sub_cap(w, h) * 4);
  L.syms = L.groups + align16((int64_t)sizeof(Group) * MAX_GROUPS);
  L.bytes = L.syms + align16((int64_t)SYM_CAP * 2);
  return L;
}
VGE_WEBP_HD inline Arena slot_arena(uint8_t* slot, int w, int h) {
  const SlotLayout L = slot_layout(w, h);
  Arena A;
  A.hdr = reinterpret_cast<FrameHdr*>(slot + L.hdr);
  A.sub = reinterpret_cast<uint32_t*>(slot + L.sub);
  A.sub_cap = (uint32_t)arena_sub_cap(w, h);
  A.groups = reinterpret_cast<Group*>(slot + L.groups);
  A.syms = reinterpret_cast<uint16_t*>(slot + L.syms);
  return A;
}

// The ARGB pixels of an image of xs * ys from the stream: literals, cache reads and copies.  meta / meta_bits: the
// entropy image (group of a pixel = (meta[tile] >> 8) & 0xffff), or NULL for the one group already in S.cur.
VGE_WEBP_HD inline int decode_pixels(BitReader& b, int xs, int ys, uint32_t* out, int cache_bits, const uint32_t* meta,
                                     int meta_bits, int n_groups, const Arena& A, Scratch& S, Stats* st, bool sub) {
  const int64_t npix = (int64_t)xs * ys;
  const int cache_shift = 32 - cache_bits;
  if (cache_bits > 0) {
    for (int k = 0; k < (1 << cache_bits); ++k) S.cache[k] = 0;
    note(st, sub ? F_CACHE | F_CACHE_SUB : F_CACHE);
  }
  const int meta_xs = meta ? sub_size(xs, meta_bits) : 0;
  const int mask = meta ? (1 << meta_bits) - 1 : -1;
  int cur_group = -1;
  bool refresh = true;  // after a copy the position may be in another tile
  int64_t pos = 0;
  int col = 0, row = 0;
  while (pos < npix) {  // every round stores at least one pixel or fails
    if (meta && ((col & mask) == 0 || refresh)) {
      refresh = false;
      const int g = (int)((meta[(int64_t)(row >> meta_bits) * meta_xs + (col >> meta_bits)] >> 8) & 0xffff);
      if (g >= n_groups) return VGE_WEBP_ERR_IO;  // cannot happen: n_groups is the largest index + 1
      if (g != cur_group) {
        S.cur = A.groups[g];
        cur_group = g;
      }
    }
    const int code = read_symbol(b, S.cur.c[0], A.syms);
    if (code < 256) {
      const uint32_t red = (uint32_t)read_symbol(b, S.cur.c[1], A.syms);
      const uint32_t blue = (uint32_t)read_symbol(b, S.cur.c[2], A.syms);
      const uint32_t alpha = (uint32_t)read_symbol(b, S.cur.c[3], A.syms);
      if (b.eos) return VGE_WEBP_ERR_IO;
      const uint32_t argb = (alpha << 24) | (red << 16) | ((uint32_t)code << 8) | blue;
      out[pos++] = argb;
      if (cache_bits > 0) S.cache[(0x1e35a7bdu * argb) >> cache_shift] = argb;
      if (++col >= xs) {
        col = 0;
        ++row;
      }
    } else if (code < GREEN_BASE) {
      const int length = read_lz_value(b, code - 256);
      const int dsym = read_symbol(b, S.cur.c[4], A.syms);
      const int dcode = read_lz_value(b, dsym);
      if (b.eos) return VGE_WEBP_ERR_IO;
      const int64_t dist = map_distance(xs, dcode, st);
      if (dist > pos || (int64_t)length > npix - pos) return VGE_WEBP_ERR_IO;  // before pixel 0, or past the end
      note(st, F_COPY | (dist < length ? F_COPY_OVERLAP : 0) | (dist > 32768 ? F_COPY_FAR : 0));
      for (int k = 0; k < length; ++k) {  // source j mod d: each pixel is stored before it is needed again
        const uint32_t argb = out[pos - dist];
        out[pos++] = argb;
        if (cache_bits > 0) S.cache[(0x1e35a7bdu * argb) >> cache_shift] = argb;
      }
      col += length;
      while (col >= xs) {
        col -= xs;
        ++row;
      }
      refresh = true;
    } else {  // a colour-cache read; the alphabet has exactly 1 << cache_bits such symbols
      const uint32_t argb = S.cache[code - GREEN_BASE];
      note(st, F_CACHE_HIT);
      out[pos++] = argb;
      S.cache[(0x1e35a7bdu * argb) >> cache_shift] = argb;
      if (++col >= xs) {
        col = 0;
        ++row;
      }
    }
  }
  return b.eos ? VGE_WEBP_ERR_IO : 0;
}

// A sub-image (transform data, entropy image): no transforms, no meta codes, its own colour cache, one group.
VGE_WEBP_HD inline int decode_sub_image(BitReader& b, int xs, int ys, uint32_t* out, const Arena& A, Scratch& S,
                                        Stats* st) {
  int cache_bits = 0;
  if (read_bits(b, 1)) {
    cache_bits = (int)read_bits(b, 4);
    if (cache_bits < 1 || cache_bits > MAX_CACHE_BITS) return VGE_WEBP_ERR_IO;
  }
  uint32_t used = 0;  // a sub-image's tables are dead when it ends: the symbol store starts over
  const int r = read_group(b, cache_bits, S, S.cur, A.syms, used, SYM_CAP, st);
  if (r != 0) return r;
  return decode_pixels(b, xs, ys, out, cache_bits, nullptr, 0, 1, A, S, st, true);
}

// The 5-byte header.  Returns 0 or VGE_WEBP_ERR_IO.
VGE_WEBP_HD inline int read_header(BitReader& b, int* w, int* h, int* alpha) {
  if (read_bits(b, 8) != 0x2f) return VGE_WEBP_ERR_IO;
  *w = 1 + (int)read_bits(b, 14);
  *h = 1 + (int)read_bits(b, 14);
  *alpha = (int)read_bits(b, 1);
  if (read_bits(b, 3) != 0 || b.eos) return VGE_WEBP_ERR_IO;
  return 0;
}

// The entropy stage of one frame: header, transforms' data, groups, and the coded image into plane A or B.  The
// payload's size must be w x h (the caller has compared it with the container's rectangle).
VGE_WEBP_HD inline int decode_entropy(const uint8_t* p, uint32_t n, int w, int h, uint32_t* plane_a, uint32_t* plane_b,
                                      const Arena& A, Scratch& S, Stats* st) {
  BitReader b{p, n, 0, 0};
  int hw, hh, alpha;
  if (read_header(b, &hw, &hh, &alpha) != 0) return VGE_WEBP_ERR_IO;
  if (hw != w || hh != h) return VGE_WEBP_ERR_BOUNDS;
  FrameHdr H;
  H.n_xforms = 0;
  H.in_b = 0;
  H.n_groups = 1;
  int xs = w, seen = 0;
  uint32_t sub_used = 0;
  while (read_bits(b, 1)) {  // at most four rounds: a type may come once
    const int type = (int)read_bits(b, 2);
    if (seen & (1 << type)) return VGE_WEBP_ERR_IO;
    seen |= 1 << type;
    Xform& X = H.x[H.n_xforms++];
    X.type = type;
    X.bits = 0;
    X.xsize = xs;
    X.data_off = (int32_t)sub_used;
    X.aux = 0;
    note(st, F_XFORM0 << type);
    if (type == T_PREDICTOR || type == T_CROSS_COLOR) {
      X.bits = 2 + (int)read_bits(b, 3);
      const int sx = sub_size(xs, X.bits), sy = sub_size(h, X.bits);
      if ((uint32_t)(sx * sy) > A.sub_cap - sub_used) return VGE_WEBP_ERR_IO;  // cannot happen: bits >= 2
      const int r = decode_sub_image(b, sx, sy, A.sub + sub_used, A, S, st);
      if (r != 0) return r;
      sub_used += (uint32_t)(sx * sy);
    } else if (type == T_INDEXING) {
      const int colors = 1 + (int)read_bits(b, 8);
      X.bits = colors > 16 ? 0 : colors > 4 ? 1 : colors > 2 ? 2 : 3;
      X.aux = colors;
      if (256 > A.sub_cap - sub_used) return VGE_WEBP_ERR_IO;  // cannot happen
      uint32_t* map = A.sub + sub_used;
      const int r = decode_sub_image(b, colors, 1, map, A, S, st);
      if (r != 0) return r;
      for (int k = 1; k < colors; ++k) {  // the palette is delta-coded, byte by byte
        const uint32_t a = map[k], c = map[k - 1];
        map[k] = (((a & 0xff00ff00u) + (c & 0xff00ff00u)) & 0xff00ff00u) |
                 (((a & 0x00ff00ffu) + (c & 0x00ff00ffu)) & 0x00ff00ffu);
      }
      for (int k = colors; k < 256; ++k) map[k] = 0;  // an index beyond the palette reads as transparent black
      sub_used += 256;
      xs = sub_size(xs, X.bits);
      H.in_b = 1;
      note(st, X.bits == 3 ? F_BUNDLE8 : X.bits == 2 ? F_BUNDLE4 : X.bits == 1 ? F_BUNDLE2 : 0);
    }
  }
  if (seen == 15) note(st, F_ALL_XFORMS);
  int cache_bits = 0;
  if (read_bits(b, 1)) {
    cache_bits = (int)read_bits(b, 4);
    if (cache_bits < 1 || cache_bits > MAX_CACHE_BITS) return VGE_WEBP_ERR_IO;
  }
  const uint32_t* meta = nullptr;
  int meta_bits = 0, n_groups = 1;
  if (read_bits(b, 1)) {
    meta_bits = 2 + (int)read_bits(b, 3);
    const int sx = sub_size(xs, meta_bits), sy = sub_size(h, meta_bits);
    if ((uint32_t)(sx * sy) > A.sub_cap - sub_used) return VGE_WEBP_ERR_IO;  // cannot happen
    uint32_t* m = A.sub + sub_used;
    const int r = decode_sub_image(b, sx, sy, m, A, S, st);
    if (r != 0) return r;
    for (int k = 0; k < sx * sy; ++k) {
      const int g = (int)((m[k] >> 8) & 0xffff);
      if (g + 1 > n_groups) n_groups = g + 1;
    }
    meta = m;
    note(st, n_groups > 1 ? F_META | F_MANY_GROUPS : F_META);
  }
  if (b.eos) return VGE_WEBP_ERR_IO;
#if !defined(__HIP_DEVICE_COMPILE__)
  if (st && (uint64_t)n_groups > st->max_groups) st->max_groups = (uint64_t)n_groups;
#endif
  if (n_groups > MAX_GROUPS) return VGE_WEBP_ERR_GROUPS;
  uint32_t used = 0;
  for (int g = 0; g < n_groups; ++g) {
    const int r = read_group(b, cache_bits, S, S.cur, A.syms, used, SYM_CAP, st);
    if (r != 0) return r;
    A.groups[g] = S.cur;
  }
  H.xsize = xs;
  H.n_groups = n_groups;
  *A.hdr = H;
  const int r = decode_pixels(b, xs, h, H.in_b ? plane_b : plane_a, cache_bits, meta, meta_bits, n_groups, A, S, st,
                              false);
  if (r == 0 && (b.pos + 7) / 8 < n) note(st, F_TRAILING);
  return r;
}

// ---- The inverse transforms, pixel by pixel.

VGE_WEBP_HD inline uint32_t add_pixels(uint32_t a, uint32_t b) {
  return (((a & 0xff00ff00u) + (b & 0xff00ff00u)) & 0xff00ff00u) | (((a & 0x00ff00ffu) + (b & 0x00ff00ffu)) & 0x00ff00ffu);
}
VGE_WEBP_HD inline uint32_t avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xfefefefeu) >> 1) + (a & b); }
VGE_WEBP_HD inline int clip255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
VGE_WEBP_HD inline int iabs(int v) { return v < 0 ? -v : v; }
VGE_WEBP_HD inline int ch(uint32_t v, int s) { return (int)((v >> s) & 0xff); }

VGE_WEBP_HD inline uint32_t select_px(uint32_t T, uint32_t L, uint32_t TL) {
  int d = 0;  // sum |L - TL| - |T - TL|: the Manhattan distances of L + T - TL to T and to L
  for (int s = 0; s < 32; s += 8) d += iabs(ch(L, s) - ch(TL, s)) - iabs(ch(T, s) - ch(TL, s));
  return d <= 0 ? T : L;
}
VGE_WEBP_HD inline uint32_t clamp_add_sub_full(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r = 0;
  for (int s = 0; s < 32; s += 8) r |= (uint32_t)clip255(ch(a, s) + ch(b, s) - ch(c, s)) << s;
  return r;
}
VGE_WEBP_HD inline uint32_t clamp_add_sub_half(uint32_t a, uint32_t c) {
  uint32_t r = 0;
  for (int s = 0; s < 32; s += 8) r |= (uint32_t)clip255(ch(a, s) + (ch(a, s) - ch(c, s)) / 2) << s;
  return r;
}

// The prediction of pixel (x, y), x > 0 and y > 0, from its left, top, top-left and top-right neighbours.  Modes 14
// and 15 are black, as in libwebp.
VGE_WEBP_HD inline uint32_t predict(int mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
  switch (mode) {
    case 1: return L;
    case 2: return T;
    case 3: return TR;
    case 4: return TL;
    case 5: return avg2(avg2(L, TR), T);
    case 6: return avg2(L, TL);
    case 7: return avg2(L, T);
    case 8: return avg2(TL, T);
    case 9: return avg2(T, TR);
    case 10: return avg2(avg2(L, TL), avg2(T, TR));
    case 11: return select_px(T, L, TL);
    case 12: return clamp_add_sub_full(L, T, TL);
    case 13: return clamp_add_sub_half(avg2(L, T), TL);
    default: return 0xff000000u;
  }
}

VGE_WEBP_HD inline int color_delta(int8_t t, int8_t c) { return ((int)t * (int)c) >> 5; }
// m: the tile's multipliers (green_to_red, green_to_blue << 8, red_to_blue << 16).
VGE_WEBP_HD inline uint32_t cross_color_inverse(uint32_t m, uint32_t argb) {
  const int8_t green = (int8_t)(argb >> 8);
  int red = (int)((argb >> 16) & 0xff), blue = (int)(argb & 0xff);
  red = (red + color_delta((int8_t)(m & 0xff), green)) & 0xff;
  blue += color_delta((int8_t)((m >> 8) & 0xff), green);
  blue = (blue + color_delta((int8_t)((m >> 16) & 0xff), (int8_t)red)) & 0xff;
  return (argb & 0xff00ff00u) | ((uint32_t)red << 16) | (uint32_t)blue;
}
VGE_WEBP_HD inline uint32_t add_green(uint32_t argb) {
  const uint32_t g = (argb >> 8) & 0xff;
  return (argb & 0xff00ff00u) | (((argb & 0x00ff00ffu) + ((g << 16) | g)) & 0x00ff00ffu);
}
// Pixel x of a row whose words bundle 1 << bits indices each (in the green byte).
VGE_WEBP_HD inline uint32_t unbundle(const uint32_t* row, int x, int bits, const uint32_t* map) {
  const int bpp = 8 >> bits;
  const uint32_t word = (row[x >> bits] >> 8) & 0xff;
  return map[(word >> ((x & ((1 << bits) - 1)) * bpp)) & ((1u << bpp) - 1)];
}

// ---- Composition: what libwebp's animation decoder does to one canvas pixel.

VGE_WEBP_HD inline uint32_t argb_to_rgba(uint32_t v) {  // canvas pixel: R | G << 8 | B << 16 | A << 24
  return (v & 0xff00ff00u) | ((v >> 16) & 0xff) | ((v & 0xff) << 16);
}
VGE_WEBP_HD inline uint32_t blend_channel(uint32_t src, uint32_t sa, uint32_t dst, uint32_t da, uint32_t scale, int s) {
  const uint32_t v = ((src >> s) & 0xff) * sa + ((dst >> s) & 0xff) * da;
  return (uint32_t)(((uint64_t)v * scale) >> 24) & 0xff;
}
// Non-premultiplied source-over.  Opaque and fully transparent sources take the short ways libwebp takes.
VGE_WEBP_HD inline uint32_t blend_pixel(uint32_t src, uint32_t dst) {
  const uint32_t sa = src >> 24;
  if (sa == 255) return src;
  if (sa == 0) return dst;
  const uint32_t da = ((dst >> 24) * (256 - sa)) >> 8;
  const uint32_t a = sa + da;
  const uint32_t scale = (1u << 24) / a;
  return blend_channel(src, sa, dst, da, scale, 0) | (blend_channel(src, sa, dst, da, scale, 8) << 8) |
         (blend_channel(src, sa, dst, da, scale, 16) << 16) | (a << 24);
}

struct Pixel {
  uint32_t canvas;    // the frame as shown
  uint32_t disposed;  // the canvas after the frame's disposal: what the next frame draws on
};
// Frame d drawn over canvas pixel (px, py); prev: the previous frame of the file (d.index > 0).  plane: d's ARGB
// pixels, w * h.
VGE_WEBP_HD inline void compose_pixel(Pixel& P, const vge_webp_desc& d, const vge_webp_desc& prev, int px, int py,
                                      const uint32_t* plane) {
  uint32_t c = d.key ? 0u : P.disposed;
  const bool in = px >= d.x && py >= d.y && px < d.x + d.w && py < d.y + d.h;
  if (in) {
    const uint32_t src = argb_to_rgba(plane[(int64_t)(py - d.y) * d.w + (px - d.x)]);
    bool blend = d.index > 0 && d.blend && !d.key;
    if (blend && prev.dispose) {  // the previous rectangle was cleared: there the frame is copied, not blended
      if (px >= prev.x && py >= prev.y && px < prev.x + prev.w && py < prev.y + prev.h) blend = false;
    }
    c = blend ? blend_pixel(src, P.disposed) : src;
  }
  P.canvas = c;
  P.disposed = in && d.dispose ? 0u : c;
}

}  // namespace vge_webp
