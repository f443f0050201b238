// Host half of the JPEG frame front end (include/vge_frames.h): header probe, the baseline entropy decoder (marker
// parsing + Huffman decoding into int16 coefficients, a pool of host threads over frames) and the plain-C++
// reconstruct that the no-GPU path and the CPU tests use.  The device reconstruct is vge_jpeg.hip; both take their
// arithmetic from vge_jpeg_math.h.
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
#include "vge_jpeg_math.h"

namespace vge {
void set_last_error(const std::string& msg);  // vge_api.cpp (vge_last_error)
}
using vge::set_last_error;

namespace {

struct Mapped {
  const uint8_t* p = nullptr;
  size_t n = 0;
  bool ok = false;
  explicit Mapped(const char* path) {
    const int fd = ::open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return;
    struct stat st;
    if (::fstat(fd, &st) == 0 && st.st_size > 0) {
      void* m = ::mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
      if (m != MAP_FAILED) {
        p = static_cast<const uint8_t*>(m);
        n = (size_t)st.st_size;
        ok = true;
      }
    }
    ::close(fd);
  }
  ~Mapped() {
    if (ok) ::munmap(const_cast<uint8_t*>(p), n);
  }
  Mapped(const Mapped&) = delete;
  Mapped& operator=(const Mapped&) = delete;
};

template <class Fn>
void parallel_for(int n, int n_threads, Fn fn) {
  int T = n_threads > 0 ? n_threads : vge_ingest_default_threads();
  T = std::max(1, std::min(T, n));
  if (T == 1) {
    for (int i = 0; i < n; ++i) fn(i);
    return;
  }
  std::atomic<int> next{0};
  std::vector<std::thread> pool;
  pool.reserve((size_t)T);
  for (int t = 0; t < T; ++t)
    pool.emplace_back([&]() {
      for (int i; (i = next.fetch_add(1)) < n;) fn(i);
    });
  for (std::thread& th : pool) th.join();
}

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

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

// ------------------------------------------------------------------ headers
struct Huff {
  bool ok = false;
  uint8_t look_len[512];  // 9-bit lookahead: code length (0: longer than 9 bits)
  uint8_t look_sym[512];
  int32_t maxcode[18];    // largest code of each length, -1 if none
  int32_t valoff[17];     // index of the first value of a length minus its first code
  uint8_t vals[256];
};

bool build_huff(const uint8_t* bits /*[16]*/, const uint8_t* vals, int nvals, Huff& h) {
  memset(h.look_len, 0, sizeof(h.look_len));
  memcpy(h.vals, vals, (size_t)nvals);
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
  h.ok = true;
  return true;
}

struct Header {
  int width = 0, height = 0, n_comp = 0;
  int cid[3] = {0, 0, 0}, h[3] = {1, 1, 1}, v[3] = {1, 1, 1}, tq[3] = {0, 0, 0};
  int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
  uint16_t q[4][64];  // natural order
  bool q_ok[4] = {false, false, false, false};
  Huff dc[4], ac[4];
  int restart = 0;
  size_t scan = 0;  // offset of the entropy-coded data
};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Parses SOI .. SOS.  Returns a status; `tables` false: sizes only (the probe), the tables are still validated.
int parse_header(const uint8_t* p, size_t n, Header& H) {
  if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) return VGE_JPEG_ERR_IO;
  size_t q = 2;
  bool sof = false;
  while (true) {
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
        for (int k = 0; k < 64; ++k) H.q[t][kZigzag[k]] = s[o + 1 + k];
        H.q_ok[t] = true;
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
      H.scan = q + (size_t)len;
      return VGE_JPEG_OK;
    }
    // APPn, COM, DAC, DNL, ...: skipped
    q += (size_t)len;
  }
}

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

bool same_shape(const Header& H, const vge_jpeg_layout& L) {
  return H.width == L.width && H.height == L.height && H.n_comp == L.n_comp && H.h[0] == L.h0 && H.v[0] == L.v0;
}

int decode_frame(const char* path, const vge_jpeg_layout& L, int16_t* coef, uint16_t* qtab) {
  Mapped f(path);
  if (!f.ok) return VGE_JPEG_ERR_IO;
  Header* Hp = new Header();  // ~6 KB of tables: off the worker's stack
  struct Del {
    Header* h;
    ~Del() { delete h; }
  } del{Hp};
  Header& H = *Hp;
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

}  // namespace

extern "C" {

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
      if (!f.ok) {
        s = VGE_JPEG_ERR_IO;
      } else {
        Header* H = new Header();
        s = parse_header(f.p, f.n, *H);
        I.width = H->width;
        I.height = H->height;
        I.n_comp = H->n_comp;
        I.h0 = H->h[0];
        I.v0 = H->v[0];
        delete H;
      }
    }
    I.status = st[(size_t)i] = s;
  });
  return first_failure(st.data(), n, paths, "vge_jpeg_probe");
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
