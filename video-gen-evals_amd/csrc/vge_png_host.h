// The host steps that the still PNG decoder (vge_png.cpp) and the animated one (vge_apng.cpp) share: a zlib stream cut
// into chunk payloads -> filtered rows, and filtered rows -> pixels.  Plain C++ and zlib.
#pragma once
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace vge_png_host {

struct Chunk {
  size_t off, len;  // payload inside the file
};

inline int bytes_per_pixel(int color_type) { return color_type == 0 ? 1 : color_type == 2 ? 3 : color_type == 4 ? 2 : 4; }

inline int paeth(int a, int b, int c) {
  const int pa = std::abs(b - c), pb = std::abs(a - c), pc = std::abs(a + b - 2 * c);
  return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

// Filtered rows -> RGB rows; false: a filter byte above 4.  raw is reconstructed in place, alpha included; rgb may be
// NULL for a caller that wants the raw pixels only.
inline bool unfilter(uint8_t* raw, int width, int height, int color_type, uint8_t* rgb) {
  const int bpp = bytes_per_pixel(color_type);
  const size_t rowb = (size_t)width * bpp, stride = 1 + rowb;
  for (int y = 0; y < height; ++y)
    if (raw[y * stride] > 4) return false;
  for (int y = 0; y < height; ++y) {
    uint8_t* cur = raw + y * stride + 1;
    const uint8_t* up = y ? cur - stride : nullptr;
    const int ft = cur[-1];
    for (size_t i = 0; i < rowb; ++i) {
      const int a = i >= (size_t)bpp ? cur[i - bpp] : 0, b = up ? up[i] : 0, c = up && i >= (size_t)bpp ? up[i - bpp] : 0;
      const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : paeth(a, b, c);
      cur[i] = (uint8_t)(cur[i] + pred);
    }
    if (!rgb) continue;
    uint8_t* out = rgb + (size_t)y * width * 3;
    for (int x = 0; x < width; ++x) {
      const uint8_t* px = cur + (size_t)x * bpp;
      const bool grey = bpp < 3;
      out[3 * x] = px[0];
      out[3 * x + 1] = px[grey ? 0 : 1];
      out[3 * x + 2] = px[grey ? 0 : 2];
    }
  }
  return true;
}

// The zlib stream in the payloads `chunks` of the file at p -> raw (resized to count + 1: one spare byte, so that zlib
// reads on through the end of the stream and its trailer).  false: zlib reports a data error, or the count is not
// reached (include/vge_png.h states the rule).
inline bool inflate_chunks(const uint8_t* p, const std::vector<Chunk>& chunks, size_t count, std::vector<uint8_t>& raw) {
  raw.resize(count + 1);
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (inflateInit(&zs) != Z_OK) return false;
  zs.next_out = raw.data();
  size_t out_left = raw.size();
  bool bad = false, done = false;
  for (const Chunk& c : chunks) {
    size_t in_left = c.len;
    const uint8_t* in = p + c.off;
    while (in_left > 0 && !bad && !done) {
      const uInt ai = (uInt)std::min<size_t>(in_left, 1u << 30), ao = (uInt)std::min<size_t>(out_left, 1u << 30);
      zs.next_in = const_cast<Bytef*>(in);
      zs.avail_in = ai;
      zs.avail_out = ao;
      const int r = inflate(&zs, Z_NO_FLUSH);
      in += ai - zs.avail_in;
      in_left -= ai - zs.avail_in;
      out_left -= ao - zs.avail_out;
      if (r == Z_STREAM_END || out_left == 0) done = true;
      else if (r != Z_OK && r != Z_BUF_ERROR) bad = true;  // Z_DATA_ERROR, Z_NEED_DICT (FDICT), Z_MEM_ERROR
      else if (r == Z_BUF_ERROR && zs.avail_in == ai) bad = true;  // no progress: cannot happen with room on both sides
    }
    if (bad || done) break;
  }
  inflateEnd(&zs);
  return !bad && raw.size() - out_left >= count;
}

}  // namespace vge_png_host
