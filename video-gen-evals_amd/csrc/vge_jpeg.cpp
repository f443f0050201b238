// Host half of the JPEG frame front end (include/vge_frames.h): header probe, the baseline entropy decoder (marker
// parsing + Huffman decoding into int16 coefficients, a pool of host threads over frames; from paths or from files in
// memory) and the plain-C++ reconstruct that the no-GPU path and the CPU tests use.  The device reconstruct is
// vge_jpeg.hip; both take their arithmetic from vge_jpeg_math.h.  The header parser is vge_jpeg_header.h, shared with the
// device entropy decoder (vge_jpeg_dehuff.hip).  Below them the mirror images for encoding: libjpeg's quantisation tables, the
// plain-C++ forward transform (the device one is vge_jpeg_enc.hip) and the baseline Huffman encoder, into files or into
// memory (the device one is vge_jpeg_huff.hip; the Huffman tables both carry are vge_jpeg_huff_tables.h).
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/vge_frames.h"
#include "../../include/vge_ingest.h"
#include "vge_error.h"
#include "vge_host_files.h"
#include "vge_jpeg_header.h"
#include "vge_jpeg_huff_tables.h"
#include "vge_jpeg_math.h"

using vge::Mapped;
using vge::parallel_for;
using vge::set_last_error;

namespace {

using vge_jpeg::kZigzag;  // vge_jpeg_huff_tables.h

const char* status_name(int st) {
  switch (st) {
    case VGE_JPEG_OK: return "ok";
    case VGE_JPEG_ERR_ARG: return "bad argument";
    case VGE_JPEG_ERR_IO: return "unreadable, truncated or corrupt JPEG stream";
    case VGE_JPEG_ERR_SHAPE: return "frame size / sampling differs from the first frame's";
    case VGE_JPEG_ERR_PROGRESSIVE: return "unsupported JPEG: progressive / non-baseline process";
    case VGE_JPEG_ERR_ARITHMETIC: return "unsupported JPEG: arithmetic coding";
    case VGE_JPEG_ERR_PRECISION: return "unsupported JPEG: not 8-bit precision";
    case VGE_JPEG_ERR_COMPONENTS: return "unsupported JPEG: component count other than 1 or 3";
    case VGE_JPEG_ERR_SAMPLING: return "unsupported JPEG: sampling factors other than 4:4:4 / 4:2:2 / 4:2:0";
    default: return "error";
  }
}

// ------------------------------------------------------------------ headers: vge_jpeg_header.h, shared with the device
using vge_jpeg::Header;
using vge_jpeg::Huff;
using vge_jpeg::parse_header;
using vge_jpeg::same_shape;

// A heap Header (~12 KB of tables: off the worker's stack) in parse_header's start state.
struct HeaderBox {
  Header* h;
  HeaderBox() : h(new Header()) { vge_jpeg::header_init(*h); }
  ~HeaderBox() { delete h; }
  HeaderBox(const HeaderBox&) = delete;
  HeaderBox& operator=(const HeaderBox&) = delete;
};

// ------------------------------------------------------------------ entropy-coded segment
struct Bits {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t acc = 0;
  int cnt = 0;   // valid bits in acc (low end)
  int fake = 0;  // zero bits fed past the end of the segment (a marker or the end of the file)
  void fill() {
    while (cnt <= 56) {
      uint32_t b = 0;
      if (p < end && !(p[0] == 0xFF && (p + 1 >= end || p[1] != 0))) {
        b = *p;
        p += (b == 0xFF) ? 2 : 1;  // FF 00: a stuffed FF
      } else {
        fake += 8;
      }
      acc = (acc << 8) | b;
      cnt += 8;
    }
  }
  inline uint32_t peek(int n) { return (uint32_t)(acc >> (cnt - n)) & ((1u << n) - 1); }
  inline void skip(int n) { cnt -= n; }
  bool overrun() const { return cnt < fake; }  // consumed bits that were never in the stream
};

inline int decode_sym(Bits& b, const Huff& h) {
  if (b.cnt < 16) b.fill();
  const uint32_t look = b.peek(9);
  int l = h.look_len[look];
  if (l) {
    b.skip(l);
    return h.look_sym[look];
  }
  const uint32_t c16 = b.peek(16);
  for (l = 10; l <= 16; ++l) {
    const int32_t code = (int32_t)(c16 >> (16 - l));
    if (code <= h.maxcode[l]) {
      b.skip(l);
      const int idx = code + h.valoff[l];
      return (idx >= 0 && idx < 256) ? h.vals[idx] : -1;
    }
  }
  return -1;
}

inline int receive_extend(Bits& b, int s) {
  if (b.cnt < s) b.fill();
  const int v = (int)b.peek(s);
  b.skip(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One block into dst[64] (natural order, pre-zeroed).  False: corrupt.
bool decode_block(Bits& b, const Huff& dc, const Huff& ac, const uint16_t* q, int& pred, int16_t* dst) {
  int s = decode_sym(b, dc);
  if (s < 0 || s > 11) return false;
  if (s) pred += receive_extend(b, s);
  if (pred < -32768 || pred > 32767) return false;
  dst[0] = (int16_t)pred;
  int64_t l1 = (int64_t)std::abs(pred) * q[0];
  for (int k = 1; k < 64;) {
    const int rs = decode_sym(b, ac);
    if (rs < 0) return false;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) break;  // EOB
      k += 16;
      continue;
    }
    k += r;
    if (k > 63) return false;
    const int v = receive_extend(b, s);
    const int nat = kZigzag[k++];
    dst[nat] = (int16_t)v;
    l1 += (int64_t)std::abs(v) * q[nat];
  }
  return l1 <= VGE_JPEG_BLOCK_L1_MAX;  // the reconstructs' 32-bit IDCT bound (vge_jpeg_math.h)
}

// One file in memory, data[0 .. size).  An empty file is what an unreadable one is: VGE_JPEG_ERR_IO.
int decode_frame_mem(const uint8_t* data, size_t size, const vge_jpeg_layout& L, int16_t* coef, uint16_t* qtab) {
  if (size == 0) return VGE_JPEG_ERR_IO;
  struct {
    const uint8_t* p;
    size_t n;
  } f{data, size};
  HeaderBox box;
  Header& H = *box.h;
  const int st = parse_header(f.p, f.n, H);
  if (st != VGE_JPEG_OK) return st;
  if (!same_shape(H, L)) return VGE_JPEG_ERR_SHAPE;
  for (int c = 0; c < H.n_comp; ++c) memcpy(qtab + 64 * c, H.q[H.tq[c]], 64 * sizeof(uint16_t));
  Bits b{f.p + H.scan, f.p + f.n};
  int pred[3] = {0, 0, 0};
  const int n_mcu = L.mcus_x * L.mcus_y;
  int until_restart = H.restart > 0 ? H.restart : -1, rst = 0;
  for (int m = 0; m < n_mcu; ++m) {
    if (until_restart == 0) {
      // the segment ended at a marker: it must be the expected RSTn
      if (b.overrun()) return VGE_JPEG_ERR_IO;
      const uint8_t* p = b.p;
      if (p + 2 > b.end || p[0] != 0xFF || p[1] != 0xD0 + (rst & 7)) return VGE_JPEG_ERR_IO;
      b = Bits{p + 2, b.end};
      rst++;
      pred[0] = pred[1] = pred[2] = 0;
      until_restart = H.restart;
    }
    const int mx = m % L.mcus_x, my = m / L.mcus_x;
    for (int c = 0; c < H.n_comp; ++c) {
      const uint16_t* q = H.q[H.tq[c]];
      for (int v = 0; v < H.v[c]; ++v)
        for (int h = 0; h < H.h[c]; ++h) {
          const int bx = mx * H.h[c] + h, by = my * H.v[c] + v;
          int16_t* dst = coef + ((size_t)L.off[c] + (size_t)by * L.bw[c] + bx) * 64;
          if (!decode_block(b, H.dc[H.td[c]], H.ac[H.ta[c]], q, pred[c], dst)) return VGE_JPEG_ERR_IO;
        }
    }
    if (b.overrun()) return VGE_JPEG_ERR_IO;  // ran past the end of the data: truncated
    if (until_restart > 0) --until_restart;
  }
  return VGE_JPEG_OK;
}

int decode_frame(const char* path, const vge_jpeg_layout& L, int16_t* coef, uint16_t* qtab) {
  Mapped f(path);
  if (!f.ok) return VGE_JPEG_ERR_IO;
  return decode_frame_mem(f.p, f.n, L, coef, qtab);
}

// Headers only of one file in memory -> I; the probe's status.
int probe_mem(const uint8_t* data, size_t size, vge_jpeg_info& I) {
  if (size == 0) return VGE_JPEG_ERR_IO;
  HeaderBox box;
  const int s = parse_header(data, size, *box.h);
  I.width = box.h->width;
  I.height = box.h->height;
  I.n_comp = box.h->n_comp;
  I.h0 = box.h->h[0];
  I.v0 = box.h->v[0];
  return s;
}

// File i of a packed buffer lies inside it.
bool range_ok(int64_t off, int64_t size, int64_t data_bytes) {
  return off >= 0 && size >= 0 && off <= data_bytes && size <= data_bytes - off;
}

int first_failure_mem(const int32_t* st, int n, const char* what) {
  for (int i = 0; i < n; ++i)
    if (st[i] != VGE_JPEG_OK) {
      set_last_error(std::string(what) + ": file " + std::to_string(i) + ": " + status_name(st[i]));
      return st[i];
    }
  return VGE_JPEG_OK;
}

int first_failure(const int32_t* st, int n, const char* const* paths, const char* what) {
  for (int i = 0; i < n; ++i)
    if (st[i] != VGE_JPEG_OK) {
      set_last_error(std::string(what) + ": " + (paths[i] ? paths[i] : "(null)") + ": " + status_name(st[i]));
      return st[i];
    }
  return VGE_JPEG_OK;
}

bool layout_ok(const vge_jpeg_layout* L) {
  if (!L) return false;
  vge_jpeg_layout want;
  return vge_jpeg_make_layout(L->width, L->height, L->n_comp, L->h0, L->v0, &want) == VGE_JPEG_OK &&
         memcmp(&want, L, sizeof(want)) == 0;
}

void reconstruct_frame(const int16_t* coef, const uint16_t* qtab, const vge_jpeg_layout& L, uint8_t* rgb) {
  using namespace vge_jpeg;
  std::vector<uint8_t> plane[3];
  int pitch[3] = {0, 0, 0};
  for (int c = 0; c < L.n_comp; ++c) {
    pitch[c] = L.bw[c] * 8;
    plane[c].resize((size_t)pitch[c] * L.bh[c] * 8);
    const uint16_t* q = qtab + 64 * c;
    for (int by = 0; by < L.bh[c]; ++by)
      for (int bx = 0; bx < L.bw[c]; ++bx) {
        const int16_t* blk = coef + ((size_t)L.off[c] + (size_t)by * L.bw[c] + bx) * 64;
        int32_t ws[64], in[8], o[8];
        for (int u = 0; u < 8; ++u) {  // columns
          for (int v = 0; v < 8; ++v) in[v] = (int32_t)blk[v * 8 + u] * (int32_t)q[v * 8 + u];
          idct_pass(in, o);
          for (int v = 0; v < 8; ++v) ws[v * 8 + u] = descale1(o[v]);
        }
        for (int v = 0; v < 8; ++v) {  // rows
          idct_pass(ws + v * 8, o);
          uint8_t* dst = plane[c].data() + (size_t)(by * 8 + v) * pitch[c] + bx * 8;
          for (int u = 0; u < 8; ++u) dst[u] = (uint8_t)descale2(o[u]);
        }
      }
  }
  const int W = L.width, Hh = L.height;
  if (L.n_comp == 1) {
    for (int y = 0; y < Hh; ++y)
      for (int x = 0; x < W; ++x) {
        const uint8_t g = plane[0][(size_t)y * pitch[0] + x];
        uint8_t* o = rgb + ((size_t)y * W + x) * 3;
        o[0] = o[1] = o[2] = g;
      }
    return;
  }
  const int mode = L.h0 == 1 ? MODE_444 : (L.v0 == 1 ? MODE_H2V1 : MODE_H2V2);
  const int cw = (W + L.h0 - 1) / L.h0, ch = (Hh + L.v0 - 1) / L.v0;
  const uint8_t* pb = plane[1].data();
  const uint8_t* pr = plane[2].data();
  const int cp = pitch[1];
  auto at_b = [pb, cp](int cx, int cy) { return (int)pb[(size_t)cy * cp + cx]; };
  auto at_r = [pr, cp](int cx, int cy) { return (int)pr[(size_t)cy * cp + cx]; };
  for (int y = 0; y < Hh; ++y)
    for (int x = 0; x < W; ++x) {
      int r, g, b;
      ycc_to_rgb(plane[0][(size_t)y * pitch[0] + x], chroma_at(at_b, x, y, cw, ch, mode),
                 chroma_at(at_r, x, y, cw, ch, mode), &r, &g, &b);
      uint8_t* o = rgb + ((size_t)y * W + x) * 3;
      o[0] = (uint8_t)r;
      o[1] = (uint8_t)g;
      o[2] = (uint8_t)b;
    }
}

// ------------------------------------------------------------------ encoding: the mirror images of the above
// Annex K.1 / K.2 base tables, natural order.
const uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                               14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                               18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// Annex K.3 - K.6 Huffman tables: vge_jpeg_huff_tables.h, shared with the device coder (vge_jpeg_huff.hip).
using vge_jpeg::kAcChromaBits;
using vge_jpeg::kAcChromaVals;
using vge_jpeg::kAcLumaBits;
using vge_jpeg::kAcLumaVals;
using vge_jpeg::kDcChromaBits;
using vge_jpeg::kDcLumaBits;
using vge_jpeg::kDcVals;

struct EncHuff {
  uint16_t code[256];
  uint8_t len[256];  // 0: no code for the symbol
  EncHuff(const uint8_t* bits, const uint8_t* vals) {
    memset(len, 0, sizeof(len));
    memset(code, 0, sizeof(code));
    int c = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
      for (int i = 0; i < bits[l - 1]; ++i, ++k, ++c) {
        code[vals[k]] = (uint16_t)c;
        len[vals[k]] = (uint8_t)l;
      }
      c <<= 1;
    }
  }
};

struct EncTables {
  EncHuff dc[2] = {EncHuff(kDcLumaBits, kDcVals), EncHuff(kDcChromaBits, kDcVals)};
  EncHuff ac[2] = {EncHuff(kAcLumaBits, kAcLumaVals), EncHuff(kAcChromaBits, kAcChromaVals)};
};

struct BitWriter {
  std::vector<uint8_t>& out;
  uint64_t acc = 0;
  int cnt = 0;
  void byte(uint32_t b) {
    out.push_back((uint8_t)b);
    if (b == 0xFF) out.push_back(0);  // a stuffed FF
  }
  void put(uint32_t v, int n) {  // n <= 27
    acc = (acc << n) | (v & ((1u << n) - 1));
    cnt += n;
    while (cnt >= 8) {
      cnt -= 8;
      byte((uint32_t)(acc >> cnt) & 0xFF);
    }
  }
  void flush() {
    if (cnt) put(0x7F, 8 - cnt);  // pad the final byte with 1 bits
  }
};

inline int bit_length(int a) {
  int n = 0;
  while (a) {
    ++n;
    a >>= 1;
  }
  return n;
}

// False: a coefficient beyond what baseline Huffman coding can carry (DC difference > 11 bits, AC > 10 bits).
bool encode_block(BitWriter& w, const EncHuff& dc, const EncHuff& ac, int& pred, const int16_t* blk) {
  const int diff = (int)blk[0] - pred;
  pred = blk[0];
  int n = bit_length(std::abs(diff));
  if (n > 11) return false;
  w.put(dc.code[n], dc.len[n]);
  if (n) w.put((uint32_t)(diff < 0 ? diff - 1 : diff), n);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = blk[kZigzag[k]];
    if (v == 0) {
      ++run;
      continue;
    }
    for (; run > 15; run -= 16) w.put(ac.code[0xF0], ac.len[0xF0]);
    n = bit_length(std::abs(v));
    if (n > 10) return false;
    const int sym = (run << 4) | n;
    w.put(ac.code[sym], ac.len[sym]);
    w.put((uint32_t)(v < 0 ? v - 1 : v), n);
    run = 0;
  }
  if (run) w.put(ac.code[0], ac.len[0]);  // EOB
  return true;
}

void put_marker(std::vector<uint8_t>& o, int m, size_t payload) {
  o.push_back(0xFF);
  o.push_back((uint8_t)m);
  o.push_back((uint8_t)((payload + 2) >> 8));
  o.push_back((uint8_t)((payload + 2) & 255));
}

void put_dht(std::vector<uint8_t>& o, int id, const uint8_t* bits, const uint8_t* vals) {
  size_t n = 0;
  for (int l = 0; l < 16; ++l) n += bits[l];
  put_marker(o, 0xC4, 17 + n);
  o.push_back((uint8_t)id);
  o.insert(o.end(), bits, bits + 16);
  o.insert(o.end(), vals, vals + n);
}

// A complete baseline JFIF file, segment for segment what libjpeg writes with its defaults (jcmarker.c): SOI, APP0
// (JFIF 1.01, no density unit, 1 x 1), one DQT per table, SOF0, one DHT per table, SOS, one interleaved scan, EOI.
bool encode_file(const int16_t* coef, const uint16_t* qtab, const vge_jpeg_layout& L, const EncTables& T,
                 std::vector<uint8_t>& o) {
  o.clear();
  o.reserve((size_t)L.blocks_per_frame * 24 + 1024);
  o.push_back(0xFF);
  o.push_back(0xD8);
  put_marker(o, 0xE0, 14);
  const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  o.insert(o.end(), jfif, jfif + 14);
  for (int t = 0; t < 2; ++t) {  // component 0: table 0; components 1 and 2: table 1
    put_marker(o, 0xDB, 65);
    o.push_back((uint8_t)t);
    for (int k = 0; k < 64; ++k) o.push_back((uint8_t)qtab[64 * t + kZigzag[k]]);
  }
  put_marker(o, 0xC0, 15);
  const uint8_t sof[15] = {8,
                           (uint8_t)(L.height >> 8),
                           (uint8_t)(L.height & 255),
                           (uint8_t)(L.width >> 8),
                           (uint8_t)(L.width & 255),
                           3,
                           1,
                           (uint8_t)((L.h0 << 4) | L.v0),
                           0,
                           2,
                           0x11,
                           1,
                           3,
                           0x11,
                           1};
  o.insert(o.end(), sof, sof + 15);
  put_dht(o, 0x00, kDcLumaBits, kDcVals);
  put_dht(o, 0x10, kAcLumaBits, kAcLumaVals);
  put_dht(o, 0x01, kDcChromaBits, kDcVals);
  put_dht(o, 0x11, kAcChromaBits, kAcChromaVals);
  put_marker(o, 0xDA, 10);
  const uint8_t sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  o.insert(o.end(), sos, sos + 10);
  BitWriter w{o};
  int pred[3] = {0, 0, 0};
  for (int my = 0; my < L.mcus_y; ++my)
    for (int mx = 0; mx < L.mcus_x; ++mx)
      for (int c = 0; c < 3; ++c) {
        const int ch = c == 0 ? L.h0 : 1, cv = c == 0 ? L.v0 : 1, t = c == 0 ? 0 : 1;
        for (int v = 0; v < cv; ++v)
          for (int h = 0; h < ch; ++h) {
            const int bx = mx * ch + h, by = my * cv + v;
            const int16_t* blk = coef + ((size_t)L.off[c] + (size_t)by * L.bw[c] + bx) * 64;
            if (!encode_block(w, T.dc[t], T.ac[t], pred[c], blk)) return false;
          }
      }
  w.flush();
  o.push_back(0xFF);
  o.push_back(0xD9);
  return true;
}

bool write_file(const char* path, const uint8_t* data, size_t size) {
  const int fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
  if (fd < 0) return false;
  size_t done = 0;
  while (done < size) {
    const ssize_t k = ::write(fd, data + done, size - done);
    if (k <= 0) break;
    done += (size_t)k;
  }
  const bool ok = ::close(fd) == 0 && done == size;
  return ok;
}

// The lossy half of libjpeg's encoder for one frame: colour conversion, edge expansion, downsampling, FDCT,
// quantisation, dummy blocks (arithmetic and rules: vge_jpeg_math.h).
void forward_frame(const uint8_t* rgb, const uint16_t* qtab, const vge_jpeg_layout& L, int16_t* coef) {
  using namespace vge_jpeg;
  const int W = L.width, H = L.height;
  const int hs = L.h0 == 2 ? 1 : 0, vs = L.v0 == 2 ? 1 : 0;
  std::vector<uint8_t> plane;
  for (int c = 0; c < 3; ++c) {
    const int pw = L.bw[c] * 8, ph = L.bh[c] * 8;
    const int chs = c ? hs : 0, cvs = c ? vs : 0;
    plane.resize((size_t)pw * ph);
    auto comp = [&](int x, int y) {  // component c of input pixel (x, y); the right edge replicates the last column
      const uint8_t* p = rgb + ((size_t)y * W + std::min(x, W - 1)) * 3;
      int yy, cb, cr;
      rgb_to_ycc(p[0], p[1], p[2], &yy, &cb, &cr);
      return c == 0 ? yy : (c == 1 ? cb : cr);
    };
    for (int j = 0; j < ph; ++j) {
      int r0 = std::min(j, H - 1), r1 = r0;
      if (cvs) down_rows_v2(j, H, &r0, &r1);
      for (int i = 0; i < pw; ++i) {
        int s;
        if (!chs)
          s = comp(i, r0);
        else if (!cvs)
          s = down_h2v1(comp(2 * i, r0), comp(2 * i + 1, r0), i);
        else
          s = down_h2v2(comp(2 * i, r0), comp(2 * i + 1, r0), comp(2 * i, r1), comp(2 * i + 1, r1), i);
        plane[(size_t)j * pw + i] = (uint8_t)s;
      }
    }
    const int cw = (W + (1 << chs) - 1) >> chs, chh = (H + (1 << cvs) - 1) >> cvs;
    const int rbw = (cw + 7) / 8, rbh = (chh + 7) / 8;
    const uint16_t* q = qtab + 64 * c;
    for (int by = 0; by < L.bh[c]; ++by)
      for (int bx = 0; bx < L.bw[c]; ++bx) {
        int sx = bx, sy = by;
        const bool dummy = dummy_source(&sx, &sy, c == 0 ? L.h0 : 1, rbw, rbh);
        int32_t ws[64], d[8], o[8];
        for (int v = 0; v < 8; ++v) {  // rows
          const uint8_t* src = plane.data() + (size_t)(sy * 8 + v) * pw + sx * 8;
          for (int u = 0; u < 8; ++u) d[u] = (int32_t)src[u] - 128;
          fdct_pass(d, o);
          for (int u = 0; u < 8; ++u) ws[v * 8 + u] = fdct_row_out(o[u], u);
        }
        int16_t* dst = coef + ((size_t)L.off[c] + (size_t)by * L.bw[c] + bx) * 64;
        for (int u = 0; u < 8; ++u) {  // columns
          for (int v = 0; v < 8; ++v) d[v] = ws[v * 8 + u];
          fdct_pass(d, o);
          for (int v = 0; v < 8; ++v) {
            const int k = v * 8 + u;
            dst[k] = (dummy && k) ? (int16_t)0 : (int16_t)quantise(fdct_col_out(o[v], v), q[k]);
          }
        }
      }
  }
}

bool qtab_ok(const uint16_t* q) {
  for (int k = 0; k < 192; ++k)
    if (q[k] < 1 || q[k] > 255) return false;
  return true;
}

}  // namespace

extern "C" {

int vge_jpeg_quant_tables(int quality, uint16_t* qtab) {
  if (!qtab) {
    set_last_error("vge_jpeg_quant_tables: bad argument");
    return VGE_JPEG_ERR_ARG;
  }
  const int q = std::max(1, std::min(quality, 100));
  const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < 64; ++k) {
      const int v = ((c == 0 ? kBaseLuma[k] : kBaseChroma[k]) * scale + 50) / 100;
      qtab[64 * c + k] = (uint16_t)std::max(1, std::min(v, 255));
    }
  return VGE_JPEG_OK;
}

int vge_jpeg_forward_host(const uint8_t* rgb, const vge_jpeg_layout* layout, int n_frames, int n_threads,
                          const uint16_t* qtab, int16_t* coef) {
  if (n_frames < 0 || !layout_ok(layout) || !qtab || !qtab_ok(qtab) || (n_frames > 0 && (!rgb || !coef))) {
    set_last_error("vge_jpeg_forward_host: bad argument (layout not from vge_jpeg_make_layout, null buffer, or a "
                   "quantisation entry outside 1..255)");
    return VGE_JPEG_ERR_ARG;
  }
  if (layout->n_comp != 3) {
    set_last_error("vge_jpeg_forward_host: only 3-component (RGB) frames are encoded");
    return VGE_JPEG_ERR_COMPONENTS;
  }
  const vge_jpeg_layout L = *layout;
  const size_t per = (size_t)L.blocks_per_frame * 64, px = (size_t)L.width * L.height * 3;
  parallel_for(n_frames, n_threads,
               [&](int i) { forward_frame(rgb + px * (size_t)i, qtab, L, coef + per * (size_t)i); });
  return VGE_JPEG_OK;
}

int vge_jpeg_entropy_encode(const int16_t* coef, const uint16_t* qtab, const vge_jpeg_layout* layout, int n,
                            int n_threads, const char* const* paths, int64_t* sizes, int32_t* status) {
  if (n < 0 || !layout_ok(layout) || !qtab || !qtab_ok(qtab) || (n > 0 && (!coef || !paths))) {
    set_last_error("vge_jpeg_entropy_encode: bad argument");
    return VGE_JPEG_ERR_ARG;
  }
  if (layout->n_comp != 3) {
    set_last_error("vge_jpeg_entropy_encode: only 3-component (RGB) frames are encoded");
    return VGE_JPEG_ERR_COMPONENTS;
  }
  const vge_jpeg_layout L = *layout;
  const size_t per = (size_t)L.blocks_per_frame * 64;
  const EncTables T;
  std::vector<int32_t> st((size_t)n, VGE_JPEG_OK);
  std::vector<int64_t> sz((size_t)n, 0);
  parallel_for(n, n_threads, [&](int i) {
    int s = VGE_JPEG_ERR_ARG;
    try {
      std::vector<uint8_t> buf;
      if (!paths[i]) {
        s = VGE_JPEG_ERR_ARG;
      } else if (!encode_file(coef + per * (size_t)i, qtab, L, T, buf)) {
        s = VGE_JPEG_ERR_ARG;  // a coefficient no baseline stream can carry: not the forward transform's output
      } else if (!write_file(paths[i], buf.data(), buf.size())) {
        s = VGE_JPEG_ERR_IO;
      } else {
        s = VGE_JPEG_OK;
        sz[(size_t)i] = (int64_t)buf.size();
      }
    } catch (...) {
      s = VGE_JPEG_ERR_IO;  // out of memory
    }
    st[(size_t)i] = s;
  });
  if (sizes) memcpy(sizes, sz.data(), (size_t)n * sizeof(int64_t));
  if (status) memcpy(status, st.data(), (size_t)n * sizeof(int32_t));
  for (int i = 0; i < n; ++i)
    if (st[(size_t)i] != VGE_JPEG_OK) {
      set_last_error(std::string("vge_jpeg_entropy_encode: ") + (paths[i] ? paths[i] : "(null)") + ": " +
                     (st[(size_t)i] == VGE_JPEG_ERR_IO ? "cannot write the file" : "bad argument or coefficients"));
      return st[(size_t)i];
    }
  return VGE_JPEG_OK;
}

int vge_jpeg_entropy_encode_mem(const int16_t* coef, const uint16_t* qtab, const vge_jpeg_layout* layout, int n,
                                int n_threads, const int64_t* offsets, uint8_t* out, int64_t out_bytes, int64_t* sizes,
                                int32_t* status) {
  if (n < 0 || !layout_ok(layout) || !qtab || !qtab_ok(qtab) || (n > 0 && !coef) ||
      (out && (out_bytes < 0 || (n > 0 && !offsets)))) {
    set_last_error("vge_jpeg_entropy_encode_mem: bad argument");
    return VGE_JPEG_ERR_ARG;
  }
  if (layout->n_comp != 3) {
    set_last_error("vge_jpeg_entropy_encode_mem: only 3-component (RGB) frames are encoded");
    return VGE_JPEG_ERR_COMPONENTS;
  }
  const vge_jpeg_layout L = *layout;
  const size_t per = (size_t)L.blocks_per_frame * 64;
  const EncTables T;
  std::vector<int32_t> st((size_t)n, VGE_JPEG_OK);
  std::vector<int64_t> sz((size_t)n, 0);
  parallel_for(n, n_threads, [&](int i) {
    int s = VGE_JPEG_ERR_ARG;
    try {
      std::vector<uint8_t> buf;
      if (encode_file(coef + per * (size_t)i, qtab, L, T, buf)) {  // else: a coefficient no baseline stream can carry
        const int64_t len = (int64_t)buf.size();
        if (!out) {
          s = VGE_JPEG_OK;
        } else if (offsets[i] >= 0 && offsets[i] <= out_bytes && len <= out_bytes - offsets[i]) {
          memcpy(out + offsets[i], buf.data(), buf.size());
          s = VGE_JPEG_OK;
        }
        if (s == VGE_JPEG_OK) sz[(size_t)i] = len;
      }
    } catch (...) {
      s = VGE_JPEG_ERR_IO;  // out of memory
    }
    st[(size_t)i] = s;
  });
  if (sizes) memcpy(sizes, sz.data(), (size_t)n * sizeof(int64_t));
  if (status) memcpy(status, st.data(), (size_t)n * sizeof(int32_t));
  for (int i = 0; i < n; ++i)
    if (st[(size_t)i] != VGE_JPEG_OK) {
      set_last_error("vge_jpeg_entropy_encode_mem: frame " + std::to_string(i) +
                     (st[(size_t)i] == VGE_JPEG_ERR_IO ? ": out of memory"
                                                       : ": coefficients beyond baseline coding, or no room in out"));
      return st[(size_t)i];
    }
  return VGE_JPEG_OK;
}

int vge_jpeg_write_files(const uint8_t* data, const int64_t* offsets, const int64_t* sizes, int n, int n_threads,
                         const char* const* paths, int32_t* status) {
  if (n < 0 || (n > 0 && (!data || !offsets || !sizes || !paths))) {
    set_last_error("vge_jpeg_write_files: bad argument");
    return VGE_JPEG_ERR_ARG;
  }
  std::vector<int32_t> st((size_t)n, VGE_JPEG_OK);
  parallel_for(n, n_threads, [&](int i) {
    if (!paths[i] || offsets[i] < 0 || sizes[i] < 0)
      st[(size_t)i] = VGE_JPEG_ERR_ARG;
    else if (!write_file(paths[i], data + offsets[i], (size_t)sizes[i]))
      st[(size_t)i] = VGE_JPEG_ERR_IO;
  });
  if (status) memcpy(status, st.data(), (size_t)n * sizeof(int32_t));
  for (int i = 0; i < n; ++i)
    if (st[(size_t)i] != VGE_JPEG_OK) {
      set_last_error(std::string("vge_jpeg_write_files: ") + (paths[i] ? paths[i] : "(null)") + ": " +
                     (st[(size_t)i] == VGE_JPEG_ERR_IO ? "cannot write the file" : "bad argument"));
      return st[(size_t)i];
    }
  return VGE_JPEG_OK;
}

int vge_jpeg_probe(const char* const* paths, int n, int n_threads, vge_jpeg_info* info) {
  if (n < 0 || (n > 0 && (!paths || !info))) {
    set_last_error("vge_jpeg_probe: bad argument");
    return VGE_JPEG_ERR_ARG;
  }
  std::vector<int32_t> st((size_t)n, VGE_JPEG_OK);
  parallel_for(n, n_threads, [&](int i) {
    vge_jpeg_info& I = info[i];
    I.width = I.height = I.n_comp = I.h0 = I.v0 = 0;
    int s = VGE_JPEG_ERR_ARG;
    if (paths[i]) {
      Mapped f(paths[i]);
      s = f.ok ? probe_mem(f.p, f.n, I) : VGE_JPEG_ERR_IO;
    }
    I.status = st[(size_t)i] = s;
  });
  return first_failure(st.data(), n, paths, "vge_jpeg_probe");
}

int vge_jpeg_file_sizes(const char* const* paths, int n, int n_threads, int64_t* sizes) {
  if (n < 0 || (n > 0 && (!paths || !sizes))) {
    set_last_error("vge_jpeg_file_sizes: bad argument");
    return VGE_JPEG_ERR_ARG;
  }
  parallel_for(n, n_threads, [&](int i) {
    struct stat st;
    sizes[i] = (paths[i] && ::stat(paths[i], &st) == 0 && S_ISREG(st.st_mode)) ? (int64_t)st.st_size : 0;
  });
  return VGE_JPEG_OK;
}

int vge_jpeg_read_files(const char* const* paths, int n, int n_threads, const int64_t* offsets, const int64_t* sizes,
                        uint8_t* data, int64_t data_bytes, int32_t* status) {
  if (n < 0 || data_bytes < 0 || (n > 0 && (!paths || !offsets || !sizes || !data))) {
    set_last_error("vge_jpeg_read_files: bad argument");
    return VGE_JPEG_ERR_ARG;
  }
  std::vector<int32_t> st((size_t)n, VGE_JPEG_OK);
  parallel_for(n, n_threads, [&](int i) {
    if (!paths[i] || !range_ok(offsets[i], sizes[i], data_bytes)) {
      st[(size_t)i] = VGE_JPEG_ERR_ARG;
      return;
    }
    uint8_t* dst = data + offsets[i];
    const size_t want = (size_t)sizes[i];
    size_t done = 0;
    const int fd = want ? ::open(paths[i], O_RDONLY | O_CLOEXEC) : -1;
    if (fd >= 0) {
      while (done < want) {
        const ssize_t k = ::read(fd, dst + done, want - done);
        if (k <= 0) break;
        done += (size_t)k;
      }
      ::close(fd);
    }
    if (done != want) {  // shorter than it was, or unreadable: no JPEG is left in its place
      memset(dst, 0, want);
      st[(size_t)i] = VGE_JPEG_ERR_IO;
    }
  });
  if (status) memcpy(status, st.data(), (size_t)n * sizeof(int32_t));
  return first_failure(st.data(), n, paths, "vge_jpeg_read_files");
}

int vge_jpeg_probe_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                       int n_threads, vge_jpeg_info* info) {
  if (n < 0 || data_bytes < 0 || (n > 0 && (!data || !offsets || !sizes || !info))) {
    set_last_error("vge_jpeg_probe_mem: bad argument");
    return VGE_JPEG_ERR_ARG;
  }
  std::vector<int32_t> st((size_t)n, VGE_JPEG_OK);
  parallel_for(n, n_threads, [&](int i) {
    vge_jpeg_info& I = info[i];
    I.width = I.height = I.n_comp = I.h0 = I.v0 = 0;
    I.status = st[(size_t)i] = range_ok(offsets[i], sizes[i], data_bytes)
                                   ? probe_mem(data + offsets[i], (size_t)sizes[i], I)
                                   : VGE_JPEG_ERR_ARG;
  });
  return first_failure_mem(st.data(), n, "vge_jpeg_probe_mem");
}

int vge_jpeg_entropy_decode_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes,
                                int n, int n_threads, const vge_jpeg_layout* layout, int16_t* coef, uint16_t* qtab,
                                int32_t* status) {
  if (n < 0 || data_bytes < 0 || !layout_ok(layout) || (n > 0 && (!data || !offsets || !sizes || !coef || !qtab))) {
    set_last_error("vge_jpeg_entropy_decode_mem: bad argument");
    return VGE_JPEG_ERR_ARG;
  }
  const vge_jpeg_layout L = *layout;
  const size_t per = (size_t)L.blocks_per_frame * 64;
  std::vector<int32_t> st((size_t)n, VGE_JPEG_OK);
  parallel_for(n, n_threads, [&](int i) {
    int16_t* c = coef + per * (size_t)i;
    uint16_t* q = qtab + 192 * (size_t)i;
    memset(c, 0, per * sizeof(int16_t));
    for (int k = 0; k < 192; ++k) q[k] = 1;
    const int s = range_ok(offsets[i], sizes[i], data_bytes)
                      ? decode_frame_mem(data + offsets[i], (size_t)sizes[i], L, c, q)
                      : VGE_JPEG_ERR_ARG;  // a file outside the buffer: nothing of it is read
    if (s != VGE_JPEG_OK) {
      memset(c, 0, per * sizeof(int16_t));
      for (int k = 0; k < 192; ++k) q[k] = 1;
    }
    st[(size_t)i] = s;
  });
  if (status) memcpy(status, st.data(), (size_t)n * sizeof(int32_t));
  return first_failure_mem(st.data(), n, "vge_jpeg_entropy_decode_mem");
}

int vge_jpeg_make_layout(int width, int height, int n_comp, int h0, int v0, vge_jpeg_layout* L) {
  if (!L || width < 1 || height < 1 || width > 65535 || height > 65535) {
    set_last_error("vge_jpeg_make_layout: bad argument");
    return VGE_JPEG_ERR_ARG;
  }
  if (n_comp != 1 && n_comp != 3) {
    set_last_error("vge_jpeg_make_layout: component count other than 1 or 3");
    return VGE_JPEG_ERR_COMPONENTS;
  }
  if (n_comp == 1) h0 = v0 = 1;
  if (!((h0 == 1 && v0 == 1) || (h0 == 2 && v0 == 1) || (h0 == 2 && v0 == 2))) {
    set_last_error("vge_jpeg_make_layout: sampling factors other than 4:4:4 / 4:2:2 / 4:2:0");
    return VGE_JPEG_ERR_SAMPLING;
  }
  memset(L, 0, sizeof(*L));
  L->width = width;
  L->height = height;
  L->n_comp = n_comp;
  L->h0 = h0;
  L->v0 = v0;
  L->mcus_x = (width + 8 * h0 - 1) / (8 * h0);
  L->mcus_y = (height + 8 * v0 - 1) / (8 * v0);
  int off = 0;
  for (int c = 0; c < n_comp; ++c) {
    L->bw[c] = L->mcus_x * (c == 0 ? h0 : 1);
    L->bh[c] = L->mcus_y * (c == 0 ? v0 : 1);
    L->off[c] = off;
    off += L->bw[c] * L->bh[c];
  }
  L->blocks_per_frame = off;
  return VGE_JPEG_OK;
}

int vge_jpeg_entropy_decode(const char* const* paths, int n, int n_threads, const vge_jpeg_layout* layout,
                            int16_t* coef, uint16_t* qtab, int32_t* status) {
  if (n < 0 || !layout_ok(layout) || (n > 0 && (!paths || !coef || !qtab))) {
    set_last_error("vge_jpeg_entropy_decode: bad argument");
    return VGE_JPEG_ERR_ARG;
  }
  const vge_jpeg_layout L = *layout;
  const size_t per = (size_t)L.blocks_per_frame * 64;
  std::vector<int32_t> st((size_t)n, VGE_JPEG_OK);
  parallel_for(n, n_threads, [&](int i) {
    int16_t* c = coef + per * (size_t)i;
    uint16_t* q = qtab + 192 * (size_t)i;
    memset(c, 0, per * sizeof(int16_t));
    for (int k = 0; k < 192; ++k) q[k] = 1;
    int s = paths[i] ? decode_frame(paths[i], L, c, q) : VGE_JPEG_ERR_ARG;
    if (s != VGE_JPEG_OK) {
      memset(c, 0, per * sizeof(int16_t));
      for (int k = 0; k < 192; ++k) q[k] = 1;
    }
    st[(size_t)i] = s;
  });
  if (status) memcpy(status, st.data(), (size_t)n * sizeof(int32_t));
  return first_failure(st.data(), n, paths, "vge_jpeg_entropy_decode");
}

int vge_jpeg_reconstruct_host(const int16_t* coef, const uint16_t* qtab, const vge_jpeg_layout* layout, int n_frames,
                              int n_threads, uint8_t* rgb) {
  if (n_frames < 0 || !layout_ok(layout) || (n_frames > 0 && (!coef || !qtab || !rgb))) {
    set_last_error("vge_jpeg_reconstruct_host: bad argument");
    return VGE_JPEG_ERR_ARG;
  }
  const vge_jpeg_layout L = *layout;
  const size_t per = (size_t)L.blocks_per_frame * 64, px = (size_t)L.width * L.height * 3;
  parallel_for(n_frames, n_threads, [&](int i) {
    reconstruct_frame(coef + per * (size_t)i, qtab + 192 * (size_t)i, L, rgb + px * (size_t)i);
  });
  return VGE_JPEG_OK;
}

}  // extern "C"
