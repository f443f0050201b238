// The rules of the GIF decoders, compiled for both sides (as vge_inflate_tables.h holds deflate's): the per-code LZW
// step -- width schedule, validity check, entry insertion -- and the per-pixel composition step.  The host decoder
// (vge_gif.cpp) and the kernels (vge_gif.hip) call these and nothing else for the format's logic, so they cannot drift
// apart, and the logic can be stepped through on a CPU build.
#pragma once
#include <stdint.h>

#include "../../include/vge_gif.h"

#if defined(__HIPCC__)
#define VGE_GIF_HD __host__ __device__
#else
#define VGE_GIF_HD
#endif

namespace vge_gif {

constexpr int TABLE = 4096;   // dictionary entries
constexpr int MAX_BITS = 12;

// One dictionary string: the string of `prefix` plus `suffix`.  A colour index below the clear code is its own string.
struct Entry {
  uint16_t prefix;
  uint16_t len;     // bytes of the string
  uint8_t suffix;   // its last byte
  uint8_t first;    // its first byte
  uint16_t pad;
};

// Everything the width of the next code and the next free entry depend on is how many codes were read since the last
// clear code: the first of them adds no entry, every later one adds one while there is room.
struct Lzw {
  int32_t mcs;     // minimum code size, 2..8
  int32_t since;   // codes read since the last clear code (or the start of the stream)
  int32_t prev;    // the previous code, -1 before the first
  int32_t prev_len, prev_first;  // its string's length and first byte: a step reads the dictionary once, for `code`
};

enum { STEP_DATA = 0, STEP_CLEAR = 1, STEP_END = 2, STEP_BAD = 3 };

VGE_GIF_HD inline int clear_code(int mcs) { return 1 << mcs; }

// The next free entry when `since` codes have been read since the last clear code.
VGE_GIF_HD inline int next_free(int mcs, int since) {
  const int s = since > 1 ? since : 1;
  return s >= TABLE ? TABLE : (clear_code(mcs) + 1 + s > TABLE ? TABLE : clear_code(mcs) + 1 + s);
}

// The width of the code read then: it grows when the next free entry reaches a power of two, and stays at 12.
VGE_GIF_HD inline int code_width(int mcs, int since) {
  const int next = next_free(mcs, since);
  int w = mcs + 1;
  while ((1 << w) <= next && w < MAX_BITS) ++w;
  return w;
}

// The literal strings and the two reserved codes, entries [0, clear + 2); they survive every clear code.
VGE_GIF_HD inline Entry initial_entry(int mcs, int k) {
  Entry e;
  e.prefix = 0;
  e.len = k < clear_code(mcs) ? 1 : 0;
  e.suffix = (uint8_t)k;
  e.first = (uint8_t)k;
  e.pad = 0;
  return e;
}

// One code.  STEP_DATA: the code's string is in the table (walk prefix links from `code`, *len bytes, last byte first).
VGE_GIF_HD inline int lzw_step(Lzw& L, Entry* table, int code, int* len) {
  const int clear = clear_code(L.mcs);
  *len = 0;
  if (code == clear) {
    L.since = 0;
    L.prev = -1;
    return STEP_CLEAR;
  }
  if (code == clear + 1) return STEP_END;
  if (L.since == 0) {  // the first code after a clear code: a plain colour index
    if (code > clear) return STEP_BAD;
    L.prev = code;
    L.prev_len = 1;
    L.prev_first = code;
    L.since = 1;
    *len = 1;
    return STEP_DATA;
  }
  const int next = next_free(L.mcs, L.since);
  if (code > next || code >= TABLE) return STEP_BAD;
  int code_len, code_first;
  if (code == next) {  // KwKwK (next < TABLE here): the previous string plus its own first byte
    code_len = L.prev_len + 1;
    code_first = L.prev_first;
  } else {
    const Entry c = table[code];
    code_len = c.len;
    code_first = c.first;
  }
  if (next < TABLE) {
    Entry e;
    e.prefix = (uint16_t)L.prev;
    e.len = (uint16_t)(L.prev_len + 1);
    e.suffix = (uint8_t)code_first;
    e.first = (uint8_t)L.prev_first;
    e.pad = 0;
    table[next] = e;
  }
  *len = code_len;
  L.prev = code;
  L.prev_len = code_len;
  L.prev_first = code_first;
  if (L.since < TABLE) L.since++;  // beyond the full dictionary nothing depends on the count any more
  return STEP_DATA;
}

// Row r of an interlaced frame of h rows is stored at this row: rows 0, 8, 16.., then 4, 12.., then 2, 6.., then 1, 3...
VGE_GIF_HD inline int stored_row(int r, int h, int interlace) {
  if (!interlace) return r;
  const int n0 = (h + 7) / 8, n1 = h > 4 ? (h - 4 + 7) / 8 : 0, n2 = h > 2 ? (h - 2 + 3) / 4 : 0;
  if ((r & 7) == 0) return r >> 3;
  if ((r & 7) == 4) return n0 + (r >> 3);
  if ((r & 3) == 2) return n0 + n1 + (r >> 2);
  return n0 + n1 + n2 + (r >> 1);
}

VGE_GIF_HD inline int32_t pack_rgb(const uint8_t* p) {
  return (int32_t)p[0] | ((int32_t)p[1] << 8) | ((int32_t)p[2] << 16);
}

// A colour index resolved for fills and the first canvas: inside the table its colour, beyond it entry 0 on later
// frames and black on frame 0.
VGE_GIF_HD inline int32_t fill_color(const uint8_t* table, int ct_size, int c, int frame_index) {
  if (c < ct_size) return pack_rgb(table + 3 * c);
  return frame_index >= 1 ? pack_rgb(table) : 0;
}

// One screen pixel's state between frames.
struct Pixel {
  int32_t canvas;    // R | G << 8 | B << 16
  int32_t pending;   // what the previous frame's disposal puts back before the next frame
  int32_t has_pending;
};

// Frame d drawn over pixel (px, py): the pending restore, what d leaves pending, then d's own pixel.  idx: d's index
// plane (w * h, stored row order); table: its colour table.  P.canvas is the output pixel afterwards.
VGE_GIF_HD inline void compose_pixel(Pixel& P, const vge_gif_desc& d, int px, int py, const uint8_t* idx,
                                     const uint8_t* table) {
  if (P.has_pending) {
    P.canvas = P.pending;
    P.has_pending = 0;
  }
  if (px < d.x || py < d.y || px >= d.x + d.w || py >= d.y + d.h) return;
  if (d.disposal == 2 || (d.disposal >= 3 && d.index == 0)) {
    if (d.fill_rgb >= 0) {
      P.pending = d.fill_rgb;
      P.has_pending = 1;
    }
  } else if (d.disposal >= 3) {
    P.pending = P.canvas;
    P.has_pending = 1;
  }
  const int row = stored_row(py - d.y, d.h, d.interlace);
  const int i = idx[(int64_t)row * d.w + (px - d.x)];
  if (d.index == 0 || i != d.transparent) P.canvas = i < d.ct_size ? pack_rgb(table + 3 * i) : 0;
}

}  // namespace vge_gif
