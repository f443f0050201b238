// The JPEG header parser (SOI .. SOS) and the Huffman decode tables it builds, shared by the host entropy decoder
// (vge_jpeg.cpp) and the device one (vge_jpeg_dehuff.hip) so that the marker rules and the status decisions exist once:
// both sides give a stream the same status because they run the same code over the same bytes.  Plain integer code
// over a byte range [p, p + n); it reads no byte outside it and allocates nothing.
#ifndef VGE_JPEG_HEADER_H
#define VGE_JPEG_HEADER_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/vge_frames.h"
#include "vge_jpeg_huff_tables.h"
#include "vge_jpeg_math.h"  // VGE_JPEG_HD

namespace vge_jpeg {

// Zigzag position -> natural index, for both sides: device code cannot index the host's kZigzag at run time, so the
// function carries a compile-time copy of it.
struct ZigzagCopy {
  uint8_t v[64];
};
constexpr ZigzagCopy zigzag_copy() {
  ZigzagCopy z{};
  for (int i = 0; i < 64; ++i) z.v[i] = kZigzag[i];
  return z;
}
VGE_JPEG_HD int zigzag_at(int k) {
  constexpr ZigzagCopy z = zigzag_copy();
  return z.v[k];
}

struct Huff {
  uint8_t ok;
  uint8_t look_len[512];  // 9-bit lookahead: code length (0: longer than 9 bits)
  uint8_t look_sym[512];
  int32_t maxcode[18];    // largest code of each length, -1 if none
  int32_t valoff[17];     // index of the first value of a length minus its first code
  uint8_t vals[256];
};
static_assert(sizeof(Huff) % 4 == 0, "Huff is staged into LDS as dwords");

VGE_JPEG_HD bool build_huff(const uint8_t* bits /*[16]*/, const uint8_t* vals, int nvals, Huff& h) {
  for (int i = 0; i < 512; ++i) h.look_len[i] = 0;
  for (int i = 0; i < 256; ++i) h.vals[i] = i < nvals ? vals[i] : 0;  // nvals <= 256
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int cnt = bits[l - 1];
    h.valoff[l] = k - code;
    if (cnt) {
      if (code + cnt > (1 << l)) return false;  // over-subscribed
      if (l <= 9)
        for (int i = 0; i < cnt; ++i) {
          const int first = (code + i) << (9 - l);
          for (int j = 0; j < (1 << (9 - l)); ++j) {
            h.look_len[first + j] = (uint8_t)l;
            h.look_sym[first + j] = vals[k + i];
          }
        }
      k += cnt;
      code += cnt;
      h.maxcode[l] = code - 1;
    } else {
      h.maxcode[l] = -1;
    }
    code <<= 1;
  }
  h.maxcode[17] = 0x7fffffff;
  h.ok = 1;
  return true;
}

struct Header {
  int32_t width, height, n_comp;
  int32_t cid[3], h[3], v[3], tq[3];
  int32_t td[3], ta[3];
  uint16_t q[4][64];  // natural order
  uint8_t q_ok[4];
  Huff dc[4], ac[4];
  int32_t restart;
  uint32_t scan;  // offset of the entropy-coded data
};

// The state parse_header starts from (a Header in a workspace is not constructed).
VGE_JPEG_HD void header_init(Header& H) {
  H.width = H.height = H.n_comp = 0;
  for (int c = 0; c < 3; ++c) {
    H.cid[c] = H.tq[c] = H.td[c] = H.ta[c] = 0;
    H.h[c] = H.v[c] = 1;
  }
  for (int t = 0; t < 4; ++t) H.q_ok[t] = H.dc[t].ok = H.ac[t].ok = 0;
  H.restart = 0;
  H.scan = 0;
}

VGE_JPEG_HD int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Parses SOI .. SOS of the file p[0..n) into H (header_init'ed).  Returns a VGE_JPEG_* status.
VGE_JPEG_HD int parse_header(const uint8_t* p, size_t n, Header& H) {
  if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) return VGE_JPEG_ERR_IO;
  size_t q = 2;
  bool sof = false;
  while (true) {  // every pass consumes at least one byte of the n
    if (q + 4 > n) return VGE_JPEG_ERR_IO;
    if (p[q] != 0xFF) return VGE_JPEG_ERR_IO;
    while (q < n && p[q] == 0xFF) ++q;  // fill bytes
    if (q >= n) return VGE_JPEG_ERR_IO;
    const int m = p[q++];
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // no payload
    if (m == 0xD9) return VGE_JPEG_ERR_IO;                             // EOI before any scan
    if (q + 2 > n) return VGE_JPEG_ERR_IO;
    const int len = be16(p + q);
    if (len < 2 || q + (size_t)len > n) return VGE_JPEG_ERR_IO;
    const uint8_t* s = p + q + 2;
    const int sl = len - 2;
    if (m == 0xC0 || m == 0xC1 || m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) ||
        (m >= 0xCD && m <= 0xCF)) {
      if (sl < 6) return VGE_JPEG_ERR_IO;
      H.height = be16(s + 1);
      H.width = be16(s + 3);
      H.n_comp = s[5];
      if (m >= 0xC9) return VGE_JPEG_ERR_ARITHMETIC;
      if (m != 0xC0 && m != 0xC1) return VGE_JPEG_ERR_PROGRESSIVE;
      if (s[0] != 8) return VGE_JPEG_ERR_PRECISION;
      if (m == 0xC1) return VGE_JPEG_ERR_PROGRESSIVE;  // extended sequential: not the baseline process
      if (H.n_comp != 1 && H.n_comp != 3) return VGE_JPEG_ERR_COMPONENTS;
      if (sl < 6 + 3 * H.n_comp || H.width < 1 || H.height < 1 || sof) return VGE_JPEG_ERR_IO;
      for (int c = 0; c < H.n_comp; ++c) {
        H.cid[c] = s[6 + 3 * c];
        H.h[c] = s[7 + 3 * c] >> 4;
        H.v[c] = s[7 + 3 * c] & 15;
        H.tq[c] = s[8 + 3 * c];
        if (H.h[c] < 1 || H.h[c] > 4 || H.v[c] < 1 || H.v[c] > 4 || H.tq[c] > 3) return VGE_JPEG_ERR_IO;
      }
      if (H.n_comp == 1) {
        H.h[0] = H.v[0] = 1;  // a single-component scan is not interleaved: one block per MCU whatever the factors
      } else {
        const bool luma = (H.h[0] == 1 && H.v[0] == 1) || (H.h[0] == 2 && H.v[0] == 1) || (H.h[0] == 2 && H.v[0] == 2);
        if (!luma || H.h[1] != 1 || H.v[1] != 1 || H.h[2] != 1 || H.v[2] != 1) return VGE_JPEG_ERR_SAMPLING;
      }
      sof = true;
    } else if (m == 0xDB) {  // DQT
      int o = 0;
      while (o < sl) {
        const int pq = s[o] >> 4, t = s[o] & 15;
        if (pq != 0) return pq == 1 ? VGE_JPEG_ERR_PRECISION : VGE_JPEG_ERR_IO;
        if (t > 3 || o + 65 > sl) return VGE_JPEG_ERR_IO;
        for (int k = 0; k < 64; ++k) H.q[t][zigzag_at(k)] = s[o + 1 + k];
        H.q_ok[t] = 1;
        o += 65;
      }
    } else if (m == 0xC4) {  // DHT
      int o = 0;
      while (o < sl) {
        if (o + 17 > sl) return VGE_JPEG_ERR_IO;
        const int tc = s[o] >> 4, t = s[o] & 15;
        int cnt = 0;
        for (int k = 0; k < 16; ++k) cnt += s[o + 1 + k];
        if (tc > 1 || t > 3 || cnt > 256 || o + 17 + cnt > sl) return VGE_JPEG_ERR_IO;
        if (!build_huff(s + o + 1, s + o + 17, cnt, tc ? H.ac[t] : H.dc[t])) return VGE_JPEG_ERR_IO;
        o += 17 + cnt;
      }
    } else if (m == 0xDD) {  // DRI
      if (sl < 2) return VGE_JPEG_ERR_IO;
      H.restart = be16(s);
    } else if (m == 0xDA) {  // SOS
      if (!sof) return VGE_JPEG_ERR_IO;
      if (sl < 1 || s[0] != H.n_comp || sl < 1 + 2 * H.n_comp + 3) return VGE_JPEG_ERR_IO;  // one interleaved scan
      for (int c = 0; c < H.n_comp; ++c) {
        if (s[1 + 2 * c] != H.cid[c]) return VGE_JPEG_ERR_IO;
        H.td[c] = s[2 + 2 * c] >> 4;
        H.ta[c] = s[2 + 2 * c] & 15;
        if (H.td[c] > 3 || H.ta[c] > 3 || !H.dc[H.td[c]].ok || !H.ac[H.ta[c]].ok || !H.q_ok[H.tq[c]])
          return VGE_JPEG_ERR_IO;
      }
      H.scan = (uint32_t)(q + (size_t)len);
      return VGE_JPEG_OK;
    }
    // APPn, COM, DAC, DNL, ...: skipped
    q += (size_t)len;
  }
}

VGE_JPEG_HD bool same_shape(const Header& H, const vge_jpeg_layout& L) {
  return H.width == L.width && H.height == L.height && H.n_comp == L.n_comp && H.h[0] == L.h0 && H.v[0] == L.v0;
}

}  // namespace vge_jpeg
#endif  // VGE_JPEG_HEADER_H
