// The per-pixel step of the APNG front end (include/vge_apng.h), compiled for the host decoder (vge_apng.cpp) and for
// the device compose kernel (vge_apng.hip): which operations take effect, the frame's pixel for a canvas position and
// its alpha, the blend, and the disposal that the next frame meets.  The rule is Pillow's (PngImagePlugin._seek and
// load_end), frame by frame; DESIGN.md section 5b'''''' lists where that is not the APNG specification's.
#pragma once
#include <stdint.h>

#include "../../include/vge_apng.h"

#if defined(__HIPCC__)
#define VGE_APNG_HD __host__ __device__
#else
#define VGE_APNG_HD
#endif

namespace vge_apng {

VGE_APNG_HD inline int bytes_per_pixel(int ct) { return ct == 0 ? 1 : ct == 2 ? 3 : ct == 4 ? 2 : 4; }

// PREVIOUS on a file's first frame acts as BACKGROUND; an operation Pillow does not know disposes of nothing.
VGE_APNG_HD inline int effective_dispose(const vge_apng_desc& d) {
  if (d.dispose_op == VGE_APNG_DISPOSE_PREVIOUS && d.index == 0) return VGE_APNG_DISPOSE_BACKGROUND;
  return d.dispose_op == VGE_APNG_DISPOSE_BACKGROUND || d.dispose_op == VGE_APNG_DISPOSE_PREVIOUS
             ? d.dispose_op
             : VGE_APNG_DISPOSE_NONE;
}

// OVER is an alpha blend where the frame has an alpha: its own channel (types 4 and 6) or the tRNS colour key (type 2).
// On a file's first frame, for type 0 (with or without tRNS) and for type 2 without tRNS it acts as SOURCE.
VGE_APNG_HD inline bool blends_over(const vge_apng_desc& d) {
  if (d.blend_op != VGE_APNG_BLEND_OVER || d.index == 0) return false;
  return d.color_type == 4 || d.color_type == 6 || (d.color_type == 2 && d.trns >= 0);
}

// Pillow's paste through a mask: (src * a + dst * (255 - a)) / 255, rounded as ImagingPaste rounds it.
VGE_APNG_HD inline uint32_t over8(uint32_t src, uint32_t dst, uint32_t a) {
  const uint32_t t = src * a + dst * (255u - a) + 128u;
  return (t + (t >> 8)) >> 8;
}

struct Pixel {
  uint32_t canvas;   // R | G << 8 | B << 16
  uint32_t restore;  // what the previous frame's disposal puts back before the next frame is drawn
  int32_t pending;   // 1: restore is to be applied
};

// One canvas pixel through one frame.  rows: the frame's slot, h rows of a filter byte and w raw pixels.
VGE_APNG_HD inline void compose_pixel(Pixel& P, const vge_apng_desc& d, int px, int py, const uint8_t* rows) {
  if (P.pending) {
    P.canvas = P.restore;
    P.pending = 0;
  }
  if (px < d.x || py < d.y || px - d.x >= d.w || py - d.y >= d.h) return;
  const uint32_t before = P.canvas;
  const int bpp = bytes_per_pixel(d.color_type);
  const uint8_t* s = rows + (int64_t)(py - d.y) * (1 + (int64_t)d.w * bpp) + 1 + (int64_t)(px - d.x) * bpp;
  const bool grey = bpp < 3;
  const uint32_t r = s[0], g = s[grey ? 0 : 1], b = s[grey ? 0 : 2];
  const uint32_t src = r | g << 8 | b << 16;
  if (!blends_over(d)) {
    P.canvas = src;
  } else {
    const uint32_t a = d.color_type == 2 ? (src == (uint32_t)d.trns ? 0u : 255u) : s[bpp - 1];
    P.canvas = over8(r, before & 255u, a) | over8(g, (before >> 8) & 255u, a) << 8 |
               over8(b, (before >> 16) & 255u, a) << 16;
  }
  const int disp = effective_dispose(d);
  if (disp == VGE_APNG_DISPOSE_BACKGROUND) {
    P.restore = 0;
    P.pending = 1;
  } else if (disp == VGE_APNG_DISPOSE_PREVIOUS) {
    P.restore = before;
    P.pending = 1;
  }
}

}  // namespace vge_apng
