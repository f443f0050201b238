// The host half of the lossless WebP front end (include/vge_webp.h): the RIFF chunk walk, the probe, the host decoder
// (the shared bitstream reader and the per-pixel steps of vge_webp_vp8l.h, in plain loops) and the plan of the device
// route.  Plain C++: no HIP, so that the parser and decoder can also be built into a stand-alone program under a
// sanitizer.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/vge_webp.h"
#include "vge_error.h"
#include "vge_host_files.h"
#include "vge_webp_vp8l.h"

using vge::Mapped;
using vge::parallel_for;
using vge::set_last_error;

namespace {

using namespace vge_webp;

const char* status_name(int st) {
  switch (st) {
    case VGE_WEBP_OK: return "ok";
    case VGE_WEBP_ERR_ARG: return "bad argument";
    case VGE_WEBP_ERR_IO: return "unreadable, truncated or corrupt WebP";
    case VGE_WEBP_ERR_SHAPE: return "canvas differs from the call's";
    case VGE_WEBP_ERR_LOSSY: return "unsupported WebP: a lossy (VP8 / ALPH) frame";
    case VGE_WEBP_ERR_BOUNDS: return "unsupported WebP: a frame outside the canvas or of another size than its header";
    case VGE_WEBP_ERR_GROUPS: return "unsupported WebP: more prefix-code groups than the table arena holds";
    default: return "error";
  }
}

struct Frame {
  int x = 0, y = 0, w = 0, h = 0, blend = 1, dispose = 0, has_alpha = 0;
  size_t pay_off = 0, pay_bytes = 0;  // the VP8L payload inside the file
  int status = VGE_WEBP_OK;           // what the parser alone sees
};

struct Parsed {
  int width = 0, height = 0;
  int status = VGE_WEBP_OK;  // the file-level code: set when the file has no frame to carry it
  int64_t n_chunks = 0;
  std::vector<Frame> frames;
};

inline uint32_t le24(const uint8_t* p) { return p[0] | (p[1] << 8) | ((uint32_t)p[2] << 16); }
inline uint32_t le32(const uint8_t* p) { return le24(p) | ((uint32_t)p[3] << 24); }
inline bool is(const uint8_t* p, const char* cc) { return memcmp(p, cc, 4) == 0; }

// The VP8L header of a payload into f (w, h when they are not set yet, has_alpha); the code it earns.
int look_at_vp8l(const uint8_t* p, size_t n, Frame& f, bool size_known) {
  BitReader b{p, (uint32_t)n, 0, 0};
  int w, h, alpha;
  if (read_header(b, &w, &h, &alpha) != 0) return VGE_WEBP_ERR_IO;
  f.has_alpha = alpha;
  if (!size_known) {
    f.w = w;
    f.h = h;
  } else if (w != f.w || h != f.h) {
    return VGE_WEBP_ERR_BOUNDS;
  }
  return VGE_WEBP_OK;
}

// The chunk walk: everything a frame needs except its pixels.
void parse(const uint8_t* p, size_t n, Parsed& out) {
  out = Parsed{};
  if (n >= ((size_t)1 << 28)) {
    out.status = VGE_WEBP_ERR_ARG;
    return;
  }
  if (n < 12 || !is(p, "RIFF") || !is(p + 8, "WEBP")) {
    out.status = VGE_WEBP_ERR_IO;
    return;
  }
  const uint64_t riff_end = 8 + (uint64_t)le32(p + 4);
  if (riff_end > n || riff_end < 12) {  // truncated: libwebp's demuxer refuses the file whole
    out.status = VGE_WEBP_ERR_IO;
    return;
  }
  n = (size_t)riff_end;
  bool vp8x = false, still_seen = false;
  size_t at = 12;
  while (n - at >= 8) {
    const uint8_t* c = p + at;
    const size_t size = le32(c + 4);
    const size_t body = at + 8;
    const bool fits = size <= n - body;
    out.n_chunks++;
    if (is(c, "VP8X") && fits && size >= 10 && !vp8x && out.frames.empty()) {
      vp8x = true;
      out.width = 1 + (int)le24(p + body + 4);
      out.height = 1 + (int)le24(p + body + 7);
    } else if ((is(c, "VP8L") || is(c, "VP8 ") || is(c, "ALPH")) && !still_seen && out.frames.empty()) {
      still_seen = true;
      out.frames.emplace_back();
      Frame& f = out.frames.back();
      if (vp8x) {
        f.w = out.width;
        f.h = out.height;
      }
      if (!is(c, "VP8L")) {
        f.status = VGE_WEBP_ERR_LOSSY;
        if (!vp8x && is(c, "VP8 ") && fits && size >= 10) {  // the key frame's size, for the probe
          f.w = out.width = (p[body + 6] | (p[body + 7] << 8)) & 0x3fff;
          f.h = out.height = (p[body + 8] | (p[body + 9] << 8)) & 0x3fff;
        }
      } else if (!fits) {
        f.status = VGE_WEBP_ERR_IO;
      } else {
        f.pay_off = body;
        f.pay_bytes = size;
        f.status = look_at_vp8l(p + body, size, f, vp8x);
        if (!vp8x) {
          out.width = f.w;
          out.height = f.h;
        }
      }
    } else if (is(c, "ANMF") && !still_seen) {
      out.frames.emplace_back();
      Frame& f = out.frames.back();
      if (!vp8x || !fits || size < 16) {
        f.status = VGE_WEBP_ERR_IO;
        if (!fits) break;
      } else {
        const uint8_t* a = p + body;
        f.x = 2 * (int)le24(a);
        f.y = 2 * (int)le24(a + 3);
        f.w = 1 + (int)le24(a + 6);
        f.h = 1 + (int)le24(a + 9);
        f.dispose = a[15] & 1;
        f.blend = (a[15] & 2) ? 0 : 1;
        f.status = VGE_WEBP_ERR_IO;  // until an image chunk is found
        size_t sat = body + 16;
        const size_t send = body + size;
        while (send - sat >= 8) {
          const uint8_t* sc = p + sat;
          const size_t ssize = le32(sc + 4);
          out.n_chunks++;
          if (is(sc, "VP8 ") || is(sc, "ALPH")) {
            f.status = VGE_WEBP_ERR_LOSSY;
            break;
          }
          if (ssize > send - (sat + 8)) break;
          if (is(sc, "VP8L")) {
            f.pay_off = sat + 8;
            f.pay_bytes = ssize;
            f.status = look_at_vp8l(p + sat + 8, ssize, f, true);
            break;
          }
          break;  // libwebp's demuxer ends a frame at a chunk it does not know: the frame has no image
        }
        if (f.status == VGE_WEBP_OK && ((int64_t)f.x + f.w > out.width || (int64_t)f.y + f.h > out.height))
          f.status = VGE_WEBP_ERR_BOUNDS;
      }
    }
    if (!fits) break;
    at = body + size + (size & 1);
    if (at > n) break;
  }
  if (out.frames.empty()) out.status = VGE_WEBP_ERR_IO;  // no frame
  else if (out.width < 1 || out.height < 1) out.frames[0].status = std::max(out.frames[0].status, (int)VGE_WEBP_ERR_IO);
}

void fill_info(const Parsed& P, vge_webp_info& info) {
  info = vge_webp_info{};
  info.width = P.width;
  info.height = P.height;
  info.n_frames = (int32_t)P.frames.size();
  info.status = P.status;
  info.n_chunks = P.n_chunks;
  for (const Frame& f : P.frames) {
    info.vp8l_bytes += (int64_t)f.pay_bytes;
    if (info.status == VGE_WEBP_OK) info.status = f.status;
  }
}

bool full_frame(const Frame& f, int width, int height) { return f.w == width && f.h == height; }

// A parsed file's frames as descriptors (without workspace offsets): libwebp's key-frame rule and the code that the
// first refused frame hands to every later one.  Returns the file's first failing code.
int resolve(const Parsed& P, int width, int height, int file, int64_t first_frame, vge_webp_desc* descs) {
  if (P.status != VGE_WEBP_OK) return P.status;
  int carried = P.width == width && P.height == height ? VGE_WEBP_OK : VGE_WEBP_ERR_SHAPE;
  bool prev_key = false;
  for (size_t k = 0; k < P.frames.size(); ++k) {
    const Frame& f = P.frames[k];
    vge_webp_desc& d = descs[k];
    d = vge_webp_desc{};
    d.file = file;
    d.index = (int32_t)k;
    d.frame = (int32_t)(first_frame + (int64_t)k);
    d.x = f.x;
    d.y = f.y;
    d.w = f.w;
    d.h = f.h;
    d.blend = f.blend;
    d.dispose = f.dispose;
    d.pay_off = (int64_t)f.pay_off;
    d.pay_bytes = (int64_t)f.pay_bytes;
    bool key = k == 0;
    if (k > 0) {
      const Frame& prev = P.frames[k - 1];
      if ((!f.has_alpha || !f.blend) && full_frame(f, width, height)) key = true;
      else key = prev.dispose && (full_frame(prev, width, height) || prev_key);
    }
    d.key = key ? 1 : 0;
    prev_key = key;
    if (carried == VGE_WEBP_OK) carried = f.status;
    d.plan_status = carried;
  }
  return carried;
}

// The inverse transforms of one decoded frame, last to first, in the loops the kernels run in parallel.  The result is
// in plane A.
void inverse_transforms(uint8_t* slot, int w, int h, Stats* st) {
  const SlotLayout L = slot_layout(w, h);
  const Arena A = slot_arena(slot, w, h);
  uint32_t* plane_a = reinterpret_cast<uint32_t*>(slot + L.plane_a);
  uint32_t* plane_b = reinterpret_cast<uint32_t*>(slot + L.plane_b);
  const FrameHdr H = *A.hdr;
  uint32_t* cur = H.in_b ? plane_b : plane_a;
  for (int i = H.n_xforms - 1; i >= 0; --i) {
    const Xform& X = H.x[i];
    const uint32_t* data = A.sub + X.data_off;
    const int xs = X.xsize, tiles = sub_size(xs, X.bits);
    if (X.type == T_PREDICTOR) {
      for (int y = 0; y < h; ++y) {
        uint32_t* row = cur + (size_t)y * xs;
        const uint32_t* up = y > 0 ? row - xs : row;
        for (int x = 0; x < xs; ++x) {
          uint32_t pred;
          if (y == 0) pred = x == 0 ? 0xff000000u : row[x - 1];
          else if (x == 0) pred = up[0];
          else {
            const int mode = (int)((data[(size_t)(y >> X.bits) * tiles + (x >> X.bits)] >> 8) & 0xf);
            if (st && mode < 14) st->features |= F_PRED0 << mode;
            pred = predict(mode, row[x - 1], up[x], up[x - 1], up[x + 1]);  // up[xs] is row[0]
          }
          row[x] = add_pixels(row[x], pred);
        }
      }
    } else if (X.type == T_CROSS_COLOR) {
      for (int y = 0; y < h; ++y)
        for (int x = 0; x < xs; ++x) {
          uint32_t& v = cur[(size_t)y * xs + x];
          v = cross_color_inverse(data[(size_t)(y >> X.bits) * tiles + (x >> X.bits)], v);
        }
    } else if (X.type == T_SUB_GREEN) {
      for (size_t q = 0; q < (size_t)xs * h; ++q) cur[q] = add_green(cur[q]);
    } else {  // colour indexing: plane B's bundled rows into plane A
      const int in_xs = sub_size(xs, X.bits);
      for (int y = 0; y < h; ++y)
        for (int x = 0; x < xs; ++x) {
          plane_a[(size_t)y * xs + x] = unbundle(plane_b + (size_t)y * in_xs, x, X.bits, data);
          if (st) {
            const int bpp = 8 >> X.bits;
            const uint32_t word = (plane_b[(size_t)y * in_xs + (x >> X.bits)] >> 8) & 0xff;
            if ((int)((word >> ((x & ((1 << X.bits) - 1)) * bpp)) & ((1u << bpp) - 1)) >= X.aux)
              st->features |= F_INDEX_OOB;
          }
        }
      cur = plane_a;
    }
  }
}

// One frame's payload -> its w * h ARGB pixels.
int decode_frame(const uint8_t* pay, size_t n, int w, int h, std::vector<uint32_t>& out, Stats* st) {
  const SlotLayout L = slot_layout(w, h);
  std::vector<uint64_t> slot((size_t)(L.bytes + 7) / 8);
  uint8_t* s = reinterpret_cast<uint8_t*>(slot.data());
  std::unique_ptr<Scratch> S(new Scratch);
  const int r = decode_entropy(pay, (uint32_t)n, w, h, reinterpret_cast<uint32_t*>(s + L.plane_a),
                               reinterpret_cast<uint32_t*>(s + L.plane_b), slot_arena(s, w, h), *S, st);
  if (r != 0) return r;
  inverse_transforms(s, w, h, st);
  const uint32_t* a = reinterpret_cast<const uint32_t*>(s + L.plane_a);
  out.assign(a, a + (size_t)w * h);
  return VGE_WEBP_OK;
}

struct View {
  const uint8_t* p = nullptr;
  size_t n = 0;
  int status = VGE_WEBP_OK;  // why the file cannot be looked at
};

int first_code(const char* what, const std::vector<int32_t>& file_st) {
  for (size_t i = 0; i < file_st.size(); ++i)
    if (file_st[i] != VGE_WEBP_OK) {
      set_last_error(std::string(what) + ": file " + std::to_string(i) + ": " + status_name(file_st[i]));
      return file_st[i];
    }
  return VGE_WEBP_OK;
}

int decode_views(const char* what, const std::vector<View>& views, int n_threads, int width, int height,
                 int64_t frame_cap, uint8_t* rgb, int32_t* status, int32_t* file_status, int64_t* n_frames_out) {
  const int n = (int)views.size();
  std::vector<Parsed> parsed((size_t)n);
  parallel_for(n, n_threads, [&](int i) {
    if (views[i].status != VGE_WEBP_OK) parsed[i].status = views[i].status;
    else parse(views[i].p, views[i].n, parsed[i]);
  });
  std::vector<int64_t> first((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i) first[i + 1] = first[i] + (int64_t)parsed[i].frames.size();
  const int64_t total = first[n];
  if (n_frames_out) *n_frames_out = total;
  if (total > frame_cap || total >= ((int64_t)1 << 31)) {
    set_last_error(std::string(what) + ": the files hold more frames than frame_cap");
    return VGE_WEBP_ERR_ARG;
  }
  std::vector<vge_webp_desc> descs((size_t)total);
  std::vector<int32_t> file_st((size_t)n, 0), frame_st((size_t)total, 0);
  std::vector<int32_t> owner((size_t)total);
  for (int i = 0; i < n; ++i) {
    file_st[i] = resolve(parsed[i], width, height, i, first[i], descs.data() + first[i]);
    for (int64_t k = first[i]; k < first[i + 1]; ++k) owner[k] = i;
  }
  std::vector<std::vector<uint32_t>> planes((size_t)total);
  parallel_for((int)total, n_threads, [&](int k) {  // the VP8L streams of all frames of all files
    const vge_webp_desc& d = descs[k];
    if (d.plan_status != VGE_WEBP_OK) return;
    frame_st[k] = decode_frame(views[owner[k]].p + d.pay_off, (size_t)d.pay_bytes, d.w, d.h, planes[k], nullptr);
  });
  const size_t npix = (size_t)width * height;
  parallel_for(n, n_threads, [&](int i) {
    if (first[i + 1] == first[i] || descs[first[i]].plan_status != VGE_WEBP_OK) {
      for (int64_t k = first[i]; k < first[i + 1]; ++k)
        if (status) status[k] = descs[k].plan_status;
      return;
    }
    std::vector<Pixel> canvas(npix, Pixel{0, 0});
    int carried = VGE_WEBP_OK;
    for (int64_t k = first[i]; k < first[i + 1]; ++k) {
      const vge_webp_desc& d = descs[k];
      if (carried == VGE_WEBP_OK) carried = d.plan_status != VGE_WEBP_OK ? d.plan_status : frame_st[k];
      if (status) status[k] = carried;
      if (carried != VGE_WEBP_OK) continue;
      const vge_webp_desc& prev = descs[k > first[i] ? k - 1 : k];
      uint8_t* out = rgb + (size_t)k * npix * 3;
      size_t q = 0;
      for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x, ++q) {
          compose_pixel(canvas[q], d, prev, x, y, planes[k].data());
          const uint32_t c = canvas[q].canvas;
          out[3 * q] = (uint8_t)c;
          out[3 * q + 1] = (uint8_t)(c >> 8);
          out[3 * q + 2] = (uint8_t)(c >> 16);
        }
    }
    if (file_st[i] == VGE_WEBP_OK) file_st[i] = carried;
  });
  if (file_status)
    for (int i = 0; i < n; ++i) file_status[i] = file_st[i];
  return first_code(what, file_st);
}

bool inside(int64_t off, int64_t size, int64_t data_bytes) {
  return off >= 0 && size >= 0 && off <= data_bytes && size <= data_bytes - off;
}

bool mem_args_ok(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n) {
  return n >= 0 && data_bytes >= 0 && (n == 0 || (data && offsets && sizes));
}

bool canvas_ok(int width, int height) { return width > 0 && height > 0 && width <= 16384 && height <= 16384; }

std::vector<View> mem_views(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes,
                            int n) {
  std::vector<View> views((size_t)n);
  for (int i = 0; i < n; ++i) {
    if (!inside(offsets[i], sizes[i], data_bytes)) views[i].status = VGE_WEBP_ERR_ARG;
    else if (sizes[i] == 0) views[i].status = VGE_WEBP_ERR_IO;
    else views[i] = View{data + offsets[i], (size_t)sizes[i], VGE_WEBP_OK};
  }
  return views;
}

}  // namespace

extern "C" {

int vge_webp_probe(const char* const* paths, int n, int n_threads, vge_webp_info* info) {
  if (n < 0 || (n > 0 && (!paths || !info))) {
    set_last_error("vge_webp_probe: bad argument");
    return VGE_WEBP_ERR_ARG;
  }
  std::vector<int32_t> st((size_t)n, 0);
  parallel_for(n, n_threads, [&](int i) {
    Mapped m(paths[i] ? paths[i] : "");
    Parsed P;
    if (m.ok) parse(m.p, m.n, P);
    else P.status = VGE_WEBP_ERR_IO;
    fill_info(P, info[i]);
    st[i] = info[i].status;
  });
  return first_code("vge_webp_probe", st);
}

int vge_webp_probe_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                       int n_threads, vge_webp_info* info) {
  if (!mem_args_ok(data, data_bytes, offsets, sizes, n) || (n > 0 && !info)) {
    set_last_error("vge_webp_probe_mem: bad argument");
    return VGE_WEBP_ERR_ARG;
  }
  const std::vector<View> views = mem_views(data, data_bytes, offsets, sizes, n);
  std::vector<int32_t> st((size_t)n, 0);
  parallel_for(n, n_threads, [&](int i) {
    Parsed P;
    if (views[i].status == VGE_WEBP_OK) parse(views[i].p, views[i].n, P);
    else P.status = views[i].status;
    fill_info(P, info[i]);
    st[i] = info[i].status;
  });
  return first_code("vge_webp_probe_mem", st);
}

int vge_webp_decode(const char* const* paths, int n, int n_threads, int width, int height, int64_t frame_cap,
                    uint8_t* rgb, int32_t* status, int32_t* file_status, int64_t* n_frames_out) {
  if (n < 0 || !canvas_ok(width, height) || frame_cap < 0 || (n > 0 && !paths) || (frame_cap > 0 && !rgb)) {
    set_last_error("vge_webp_decode: bad argument");
    return VGE_WEBP_ERR_ARG;
  }
  std::vector<std::unique_ptr<Mapped>> maps((size_t)n);
  std::vector<View> views((size_t)n);
  for (int i = 0; i < n; ++i) {
    maps[i].reset(new Mapped(paths[i] ? paths[i] : ""));
    if (maps[i]->ok) views[i] = View{maps[i]->p, maps[i]->n, VGE_WEBP_OK};
    else views[i].status = VGE_WEBP_ERR_IO;
  }
  return decode_views("vge_webp_decode", views, n_threads, width, height, frame_cap, rgb, status, file_status,
                      n_frames_out);
}

int vge_webp_decode_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                        int n_threads, int width, int height, int64_t frame_cap, uint8_t* rgb, int32_t* status,
                        int32_t* file_status, int64_t* n_frames_out) {
  if (!mem_args_ok(data, data_bytes, offsets, sizes, n) || !canvas_ok(width, height) || frame_cap < 0 ||
      (frame_cap > 0 && !rgb)) {
    set_last_error("vge_webp_decode_mem: bad argument");
    return VGE_WEBP_ERR_ARG;
  }
  return decode_views("vge_webp_decode_mem", mem_views(data, data_bytes, offsets, sizes, n), n_threads, width, height,
                      frame_cap, rgb, status, file_status, n_frames_out);
}

int vge_webp_plan_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                      int n_threads, int width, int height, vge_webp_desc* descs, int64_t desc_cap, int64_t* n_descs,
                      int32_t* status, int32_t* file_status, int64_t* workspace_bytes) {
  if (!mem_args_ok(data, data_bytes, offsets, sizes, n) || !canvas_ok(width, height) || desc_cap < 0 ||
      (desc_cap > 0 && !descs) || !n_descs) {
    set_last_error("vge_webp_plan_mem: bad argument");
    return VGE_WEBP_ERR_ARG;
  }
  const std::vector<View> views = mem_views(data, data_bytes, offsets, sizes, n);
  std::vector<Parsed> parsed((size_t)n);
  parallel_for(n, n_threads, [&](int i) {
    if (views[i].status != VGE_WEBP_OK) parsed[i].status = views[i].status;
    else parse(views[i].p, views[i].n, parsed[i]);
  });
  int64_t nd = 0;
  for (int i = 0; i < n; ++i) nd += (int64_t)parsed[i].frames.size();
  *n_descs = nd;
  if (workspace_bytes) *workspace_bytes = 16;
  if ((descs && nd > desc_cap) || nd >= ((int64_t)1 << 31)) {
    set_last_error("vge_webp_plan_mem: desc_cap is smaller than the number of frames");
    return VGE_WEBP_ERR_ARG;
  }
  std::vector<int32_t> file_st((size_t)n, 0);
  if (!descs) {  // counting only: the parser's codes
    for (int i = 0; i < n; ++i) {
      vge_webp_info info;
      fill_info(parsed[i], info);
      file_st[i] = info.status != VGE_WEBP_OK ? info.status
                   : (info.width != width || info.height != height) ? VGE_WEBP_ERR_SHAPE : VGE_WEBP_OK;
      if (file_status) file_status[i] = file_st[i];
    }
    return first_code("vge_webp_plan_mem", file_st);
  }
  int64_t ws = 0, k0 = 0;
  for (int i = 0; i < n; ++i) {
    const Parsed& P = parsed[i];
    file_st[i] = resolve(P, width, height, i, k0, descs + k0);
    for (size_t k = 0; k < P.frames.size(); ++k) {
      vge_webp_desc& d = descs[k0 + (int64_t)k];
      if (status) status[k0 + (int64_t)k] = d.plan_status;
      if (d.plan_status != VGE_WEBP_OK) continue;
      d.file_off = offsets[i];
      d.file_bytes = sizes[i];
      d.slot_off = ws;
      ws += slot_layout(d.w, d.h).bytes;
    }
    k0 += (int64_t)P.frames.size();
  }
  if (workspace_bytes) *workspace_bytes = std::max<int64_t>(ws, 16);
  if (file_status)
    for (int i = 0; i < n; ++i) file_status[i] = file_st[i];
  return first_code("vge_webp_plan_mem", file_st);
}

size_t vge_webp_decode_device_workspace_bytes(const vge_webp_desc* descs, int n_descs) {
  int64_t ws = 16;
  if (descs)
    for (int k = 0; k < n_descs; ++k)
      if (descs[k].frame >= 0 && descs[k].plan_status == VGE_WEBP_OK && descs[k].w > 0 && descs[k].h > 0 &&
          descs[k].w <= 16384 && descs[k].h <= 16384)
        ws = std::max(ws, descs[k].slot_off + slot_layout(descs[k].w, descs[k].h).bytes);
  return (size_t)ws;
}

int64_t vge_webp_slot_bytes(int w, int h) {
  return w > 0 && h > 0 && w <= 16384 && h <= 16384 ? slot_layout(w, h).bytes : 0;
}

// For the tests' coverage assertion: what the frames of one file exercised in the host decoder.  out[0]: the F_* mask
// of vge_webp_vp8l.h; out[1], out[2]: the distance-map codes 1..120 met (bit code - 1); out[3]: the largest number of
// prefix-code groups a frame asked for.  Returns the file's first failing code.
int vge_debug_webp_features(const uint8_t* data, int64_t bytes, uint64_t* out) {
  if (!data || bytes < 0 || !out) return VGE_WEBP_ERR_ARG;
  Parsed P;
  parse(data, (size_t)bytes, P);
  Stats st{};
  int code = P.status;
  for (const Frame& f : P.frames) {
    if (code == VGE_WEBP_OK) code = f.status;
    if (code != VGE_WEBP_OK) break;
    std::vector<uint32_t> plane;
    code = decode_frame(data + f.pay_off, f.pay_bytes, f.w, f.h, plane, &st);
  }
  out[0] = st.features;
  out[1] = st.dist_codes[0];
  out[2] = st.dist_codes[1];
  out[3] = st.max_groups;
  return code;
}

}  // extern "C"
