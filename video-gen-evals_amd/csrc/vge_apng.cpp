// The host half of the APNG video front end (include/vge_apng.h): the chunk walk (acTL, fcTL, fdAT, sequence numbers,
// the default image), the probe, the host decoder (zlib's inflate and the C++ unfilter of the still path,
// vge_png_host.h, then the shared composition step of vge_apng_px.h in plain loops) and the plan of the device route.
// Plain C++ and zlib: no HIP, so that the parser and decoder can also be built into a stand-alone program under a
// sanitizer.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/vge_apng.h"
#include "vge_apng_px.h"
#include "vge_error.h"
#include "vge_host_files.h"
#include "vge_png_host.h"

using vge::Mapped;
using vge::parallel_for;
using vge::set_last_error;
using vge_png_host::Chunk;

namespace {

using namespace vge_apng;

const char* status_name(int st) {
  switch (st) {
    case VGE_APNG_OK: return "ok";
    case VGE_APNG_ERR_ARG: return "bad argument";
    case VGE_APNG_ERR_IO: return "unreadable, truncated or corrupt PNG";
    case VGE_APNG_ERR_SHAPE: return "canvas or colour type differ from the call's";
    case VGE_APNG_ERR_INTERLACED: return "unsupported PNG: interlaced";
    case VGE_APNG_ERR_BITDEPTH: return "unsupported PNG: bit depth other than 8";
    case VGE_APNG_ERR_PALETTE: return "unsupported PNG: palette";
    case VGE_APNG_ERR_BOUNDS: return "a frame rectangle that does not fit the canvas";
    default: return "error";
  }
}

inline uint32_t be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}
inline uint32_t be16(const uint8_t* p) { return ((uint32_t)p[0] << 8) | (uint32_t)p[1]; }

struct Frame {
  int x = 0, y = 0, w = 0, h = 0, dispose_op = 0, blend_op = 0;
  bool has_fctl = false;
  size_t data_bytes = 0, n_chunks = 0;  // the non-empty payloads
  std::vector<Chunk> chunks;            // those payloads (when the caller keeps them)
  bool any_chunk = false;               // a data chunk followed the fcTL, empty or not
  int status = VGE_APNG_OK;             // what the parser alone sees
};

struct Parsed {
  int width = 0, height = 0, color_type = 0, bit_depth = 0, interlace = 0;
  int trns = -1;
  bool default_image = false;
  int status = VGE_APNG_OK;  // the file-level code: set when the file has no frame to carry it
  std::vector<Frame> frames;
};

inline void refuse(Frame& f, int code) {
  if (f.status == VGE_APNG_OK) f.status = code;
}

// The chunk walk: everything a frame needs except its pixels.  include/vge_apng.h states the rule.  A file-level
// failure leaves out.status set; parse() below then drops the frames seen so far.
void walk(const uint8_t* p, size_t n, Parsed& out, bool keep_chunks) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  out = Parsed{};
  out.status = VGE_APNG_ERR_IO;
  if (n < 8 || memcmp(p, sig, 8) != 0) return;
  if (n < 8 + 8 + 13 + 4 || be32(p + 8) != 13 || memcmp(p + 12, "IHDR", 4) != 0) return;
  const uint8_t* h = p + 16;
  const uint32_t W = be32(h), H = be32(h + 4);
  const int depth = h[8], ct = h[9], comp = h[10], filt = h[11], lace = h[12];
  if (W == 0 || H == 0 || W > 0x7fffffffu || H > 0x7fffffffu) return;
  out.width = (int)W;
  out.height = (int)H;
  out.color_type = ct;
  out.bit_depth = depth;
  out.interlace = lace;
  const bool depth_ok = ct == 0   ? (depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16)
                        : ct == 3 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8)
                        : (ct == 2 || ct == 4 || ct == 6) ? (depth == 8 || depth == 16)
                                                          : false;
  if (!depth_ok || comp != 0 || filt != 0 || lace > 1) return;
  if (ct == 3) out.status = VGE_APNG_ERR_PALETTE;
  else if (depth != 8) out.status = VGE_APNG_ERR_BITDEPTH;
  else if (lace != 0) out.status = VGE_APNG_ERR_INTERLACED;
  if (out.status != VGE_APNG_ERR_IO) return;

  bool declared = false, animated = false, seen_idat = false;
  bool run_open = false, run_is_idat = false;  // the last frame still takes data chunks, and of which kind
  uint32_t count = 0;
  int64_t seq = -1, limit = 1;
  std::vector<Frame>& F = out.frames;

  auto open_frame = [&](const uint8_t* s, size_t len) {  // an fcTL chunk
    if (!F.empty() && !F.back().any_chunk) refuse(F.back(), VGE_APNG_ERR_IO);  // an fcTL followed by no data
    F.emplace_back();
    Frame& f = F.back();
    f.has_fctl = true;
    run_open = true;
    if (len < 26) return refuse(f, VGE_APNG_ERR_IO);
    if ((int64_t)be32(s) != seq + 1) refuse(f, VGE_APNG_ERR_IO);
    seq = (int64_t)be32(s);
    const uint64_t w = be32(s + 4), hh = be32(s + 8), x = be32(s + 12), y = be32(s + 16);
    f.dispose_op = s[24];
    f.blend_op = s[25];
    if (w == 0 || hh == 0 || x + w > W || y + hh > H) return refuse(f, VGE_APNG_ERR_BOUNDS);
    f.x = (int)x;
    f.y = (int)y;
    f.w = (int)w;
    f.h = (int)hh;
  };
  auto add_data = [&](size_t off, size_t len) {
    Frame& f = F.back();
    f.any_chunk = true;
    if (len == 0) return;
    f.n_chunks++;
    f.data_bytes += len;
    if (keep_chunks) f.chunks.push_back(Chunk{off, len});
  };

  size_t at = 8 + 8 + 13 + 4;
  while (true) {
    if (n - at < 8) {
      if (!seen_idat && at != n) return;  // the file ends inside a chunk header in front of the picture
      break;
    }
    const size_t len = be32(p + at);
    const uint8_t* type = p + at + 4;
    const uint8_t* s = p + at + 8;
    if (len > n - at - 8 || n - at - 8 - len < 4) {  // payload and CRC do not lie inside the file
      if (!seen_idat) return;
      if (run_open) refuse(F.back(), VGE_APNG_ERR_IO);  // the end of the file cuts the frame
      break;
    }
    const bool is_idat = memcmp(type, "IDAT", 4) == 0, is_fdat = memcmp(type, "fdAT", 4) == 0;
    const bool is_fctl = memcmp(type, "fcTL", 4) == 0;
    if (memcmp(type, "IEND", 4) == 0) break;
    if (!seen_idat) {
      if (memcmp(type, "acTL", 4) == 0) {
        if (len < 8) return;
        if (declared) {
          declared = false;  // a second acTL: Pillow falls back to the default picture
        } else if (be32(s) != 0 && be32(s) <= 0x80000000u) {
          declared = true;
          count = be32(s);
        }
      } else if (memcmp(type, "tRNS", 4) == 0) {
        if (ct == 2 && len >= 6) {
          const uint32_t r = be16(s), g = be16(s + 2), b = be16(s + 4);
          out.trns = r < 256 && g < 256 && b < 256 ? (int)(r | g << 8 | b << 16) : -1;
        }
      } else if (is_fctl) {
        if (F.empty()) {
          open_frame(s, len);
        } else {  // two fcTL in front of the picture: the second one's sequence number is out of order or has no data
          refuse(F.back(), VGE_APNG_ERR_IO);
        }
      } else if (is_idat) {
        seen_idat = true;
        animated = declared;
        if (!animated) F.clear();  // fcTL chunks of a file that is not animated are not looked at
        if (F.empty()) {           // no fcTL in front of the picture: a still, or a default image outside the animation
          F.emplace_back();
          F.back().w = (int)W;
          F.back().h = (int)H;
          out.default_image = animated;
        } else if (F.back().status == VGE_APNG_OK &&
                   (F.back().x != 0 || F.back().y != 0 || F.back().w != (int)W || F.back().h != (int)H)) {
          refuse(F.back(), VGE_APNG_ERR_BOUNDS);  // the first animation frame is the whole canvas
        }
        limit = animated ? (int64_t)count + (out.default_image ? 1 : 0) : 1;
        run_open = run_is_idat = true;
        add_data(at + 8, len);
      }
    } else if (!animated) {
      if (!is_idat) break;  // the one run of IDATs has ended
      add_data(at + 8, len);
    } else if (is_fctl) {
      if ((int64_t)F.size() >= limit) break;  // frames beyond the declared count are not looked at
      open_frame(s, len);
      run_is_idat = false;
    } else if (is_fdat) {
      if (len < 4) {
        refuse(F.back(), VGE_APNG_ERR_IO);
      } else {
        if ((int64_t)be32(s) != seq + 1) refuse(F.back(), VGE_APNG_ERR_IO);
        seq = (int64_t)be32(s);
        if (run_open && !run_is_idat && F.back().has_fctl) add_data(at + 12, len - 4);
      }
    } else if (is_idat) {
      if (run_open && run_is_idat) add_data(at + 8, len);
    } else if (F.back().any_chunk) {
      run_open = false;  // a frame's data chunks are consecutive
    }
    at += 8 + len + 4;
  }
  if (!seen_idat) return;  // no IDAT
  if (!F.back().any_chunk) refuse(F.back(), VGE_APNG_ERR_IO);
  out.status = VGE_APNG_OK;
}

void parse(const uint8_t* p, size_t n, Parsed& out, bool keep_chunks) {
  walk(p, n, out, keep_chunks);
  if (out.status != VGE_APNG_OK) out.frames.clear();
}

void fill_info(const Parsed& P, vge_apng_info& info) {
  info = vge_apng_info{};
  info.width = P.width;
  info.height = P.height;
  info.color_type = P.color_type;
  info.bit_depth = P.bit_depth;
  info.interlace = P.interlace;
  info.n_frames = (int32_t)P.frames.size();
  info.default_image = P.default_image ? 1 : 0;
  info.status = P.status;
  for (const Frame& f : P.frames) {
    info.data_bytes += (int64_t)f.data_bytes;
    info.n_chunks += (int64_t)f.n_chunks;
    if (info.status == VGE_APNG_OK) info.status = f.status;
  }
}

inline int64_t raw_bytes_of(const Frame& f, int color_type) {
  return (int64_t)f.h * (1 + (int64_t)f.w * bytes_per_pixel(color_type));
}

// A parsed file's frames as descriptors (without workspace offsets), with the code that the first refused frame hands
// to every later one.  Returns the file's first failing code.
int resolve(const Parsed& P, int width, int height, int color_type, int file, int64_t first_frame,
            vge_apng_desc* descs) {
  if (P.status != VGE_APNG_OK) return P.status;
  int carried = P.width == width && P.height == height && P.color_type == color_type ? VGE_APNG_OK : VGE_APNG_ERR_SHAPE;
  for (size_t k = 0; k < P.frames.size(); ++k) {
    const Frame& f = P.frames[k];
    vge_apng_desc& d = descs[k];
    d = vge_apng_desc{};
    d.file = file;
    d.index = (int32_t)k;
    d.frame = (int32_t)(first_frame + (int64_t)k);
    d.x = f.x;
    d.y = f.y;
    d.w = f.w;
    d.h = f.h;
    d.color_type = P.color_type;
    d.dispose_op = f.dispose_op;
    d.blend_op = f.blend_op;
    d.trns = P.trns;
    if (carried == VGE_APNG_OK) carried = f.status;
    if (carried == VGE_APNG_OK && ((int64_t)f.data_bytes >= (1ll << 28) || raw_bytes_of(f, P.color_type) >= (1ll << 31)))
      carried = VGE_APNG_ERR_ARG;  // the kernel's bit positions are 32-bit
    d.plan_status = carried;
    if (carried == VGE_APNG_OK) d.raw_bytes = raw_bytes_of(f, P.color_type);
  }
  return carried;
}

struct View {
  const uint8_t* p = nullptr;
  size_t n = 0;
  int status = VGE_APNG_OK;  // why the file cannot be looked at
};

int first_code(const char* what, const std::vector<int32_t>& file_st) {
  for (size_t i = 0; i < file_st.size(); ++i)
    if (file_st[i] != VGE_APNG_OK) {
      set_last_error(std::string(what) + ": file " + std::to_string(i) + ": " + status_name(file_st[i]));
      return file_st[i];
    }
  return VGE_APNG_OK;
}

void parse_views(const std::vector<View>& views, int n_threads, bool keep_chunks, std::vector<Parsed>& parsed) {
  parsed.assign(views.size(), Parsed{});
  parallel_for((int)views.size(), n_threads, [&](int i) {
    if (views[i].status != VGE_APNG_OK) parsed[i].status = views[i].status;
    else parse(views[i].p, views[i].n, parsed[i], keep_chunks);
  });
}

int decode_views(const char* what, const std::vector<View>& views, int n_threads, int width, int height,
                 int color_type, int64_t frame_cap, uint8_t* rgb, int32_t* status, int32_t* file_status,
                 int64_t* n_frames_out) {
  const int n = (int)views.size();
  std::vector<Parsed> parsed;
  parse_views(views, n_threads, true, parsed);
  std::vector<int64_t> first((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i) first[i + 1] = first[i] + (int64_t)parsed[i].frames.size();
  const int64_t total = first[n];
  if (n_frames_out) *n_frames_out = total;
  if (total > frame_cap || total >= ((int64_t)1 << 31)) {
    set_last_error(std::string(what) + ": the files hold more frames than frame_cap");
    return VGE_APNG_ERR_ARG;
  }
  std::vector<vge_apng_desc> descs((size_t)total);
  std::vector<int32_t> file_st((size_t)n, 0), px_st((size_t)total, 0);
  std::vector<int32_t> owner((size_t)total);
  for (int i = 0; i < n; ++i) {
    file_st[i] = resolve(parsed[i], width, height, color_type, i, first[i], descs.data() + first[i]);
    for (int64_t k = first[i]; k < first[i + 1]; ++k) owner[k] = i;
  }
  std::vector<std::vector<uint8_t>> rows((size_t)total);
  parallel_for((int)total, n_threads, [&](int k) {  // inflate and unfilter, all frames of all files
    const vge_apng_desc& d = descs[k];
    if (d.plan_status != VGE_APNG_OK) return;
    const uint8_t* p = views[owner[k]].p;
    const std::vector<Chunk>& chunks = parsed[owner[k]].frames[d.index].chunks;
    const bool ok = vge_png_host::inflate_chunks(p, chunks, (size_t)d.raw_bytes, rows[k]) &&
                    vge_png_host::unfilter(rows[k].data(), d.w, d.h, d.color_type, nullptr);
    if (!ok) px_st[k] = VGE_APNG_ERR_IO;
  });
  const size_t npix = (size_t)width * height;
  parallel_for(n, n_threads, [&](int i) {
    if (first[i + 1] == first[i] || descs[first[i]].plan_status != VGE_APNG_OK) {
      for (int64_t k = first[i]; k < first[i + 1]; ++k)
        if (status) status[k] = descs[k].plan_status;
      return;
    }
    std::vector<Pixel> canvas(npix, Pixel{0, 0, 0});
    int carried = VGE_APNG_OK;
    for (int64_t k = first[i]; k < first[i + 1]; ++k) {
      const vge_apng_desc& d = descs[k];
      if (carried == VGE_APNG_OK) carried = d.plan_status != VGE_APNG_OK ? d.plan_status : px_st[k];
      if (status) status[k] = carried;
      if (carried != VGE_APNG_OK) continue;
      uint8_t* out = rgb + (size_t)k * npix * 3;
      size_t q = 0;
      for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x, ++q) {
          compose_pixel(canvas[q], d, x, y, rows[k].data());
          const uint32_t c = canvas[q].canvas;
          out[3 * q] = (uint8_t)c;
          out[3 * q + 1] = (uint8_t)(c >> 8);
          out[3 * q + 2] = (uint8_t)(c >> 16);
        }
    }
    if (file_st[i] == VGE_APNG_OK) file_st[i] = carried;
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

bool layout_ok(int width, int height, int color_type) {
  return width > 0 && height > 0 && (color_type == 0 || color_type == 2 || color_type == 4 || color_type == 6);
}

constexpr int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

std::vector<View> mem_views(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes,
                            int n) {
  std::vector<View> views((size_t)n);
  for (int i = 0; i < n; ++i) {
    if (!inside(offsets[i], sizes[i], data_bytes)) views[i].status = VGE_APNG_ERR_ARG;
    else if (sizes[i] == 0) views[i].status = VGE_APNG_ERR_IO;
    else views[i] = View{data + offsets[i], (size_t)sizes[i], VGE_APNG_OK};
  }
  return views;
}

void path_views(const char* const* paths, int n, std::vector<std::unique_ptr<Mapped>>& maps, std::vector<View>& views) {
  maps.resize((size_t)n);
  views.assign((size_t)n, View{});
  for (int i = 0; i < n; ++i) {
    maps[i].reset(new Mapped(paths[i] ? paths[i] : ""));
    if (maps[i]->ok) views[i] = View{maps[i]->p, maps[i]->n, VGE_APNG_OK};
    else views[i].status = VGE_APNG_ERR_IO;
  }
}

int probe_views(const char* what, const std::vector<View>& views, int n_threads, vge_apng_info* info) {
  std::vector<int32_t> st(views.size(), 0);
  parallel_for((int)views.size(), n_threads, [&](int i) {
    Parsed P;
    if (views[i].status == VGE_APNG_OK) parse(views[i].p, views[i].n, P, false);
    else P.status = views[i].status;
    fill_info(P, info[i]);
    st[i] = info[i].status;
  });
  return first_code(what, st);
}

}  // namespace

extern "C" {

int vge_apng_probe(const char* const* paths, int n, int n_threads, vge_apng_info* info) {
  if (n < 0 || (n > 0 && (!paths || !info))) {
    set_last_error("vge_apng_probe: bad argument");
    return VGE_APNG_ERR_ARG;
  }
  std::vector<std::unique_ptr<Mapped>> maps;
  std::vector<View> views;
  path_views(paths, n, maps, views);
  return probe_views("vge_apng_probe", views, n_threads, info);
}

int vge_apng_probe_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                       int n_threads, vge_apng_info* info) {
  if (!mem_args_ok(data, data_bytes, offsets, sizes, n) || (n > 0 && !info)) {
    set_last_error("vge_apng_probe_mem: bad argument");
    return VGE_APNG_ERR_ARG;
  }
  return probe_views("vge_apng_probe_mem", mem_views(data, data_bytes, offsets, sizes, n), n_threads, info);
}

int vge_apng_decode(const char* const* paths, int n, int n_threads, int width, int height, int color_type,
                    int64_t frame_cap, uint8_t* rgb, int32_t* status, int32_t* file_status, int64_t* n_frames_out) {
  if (n < 0 || !layout_ok(width, height, color_type) || frame_cap < 0 || (n > 0 && !paths) || (frame_cap > 0 && !rgb)) {
    set_last_error("vge_apng_decode: bad argument");
    return VGE_APNG_ERR_ARG;
  }
  std::vector<std::unique_ptr<Mapped>> maps;
  std::vector<View> views;
  path_views(paths, n, maps, views);
  return decode_views("vge_apng_decode", views, n_threads, width, height, color_type, frame_cap, rgb, status,
                      file_status, n_frames_out);
}

int vge_apng_decode_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                        int n_threads, int width, int height, int color_type, int64_t frame_cap, uint8_t* rgb,
                        int32_t* status, int32_t* file_status, int64_t* n_frames_out) {
  if (!mem_args_ok(data, data_bytes, offsets, sizes, n) || !layout_ok(width, height, color_type) || frame_cap < 0 ||
      (frame_cap > 0 && !rgb)) {
    set_last_error("vge_apng_decode_mem: bad argument");
    return VGE_APNG_ERR_ARG;
  }
  return decode_views("vge_apng_decode_mem", mem_views(data, data_bytes, offsets, sizes, n), n_threads, width, height,
                      color_type, frame_cap, rgb, status, file_status, n_frames_out);
}

int vge_apng_plan_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                      int n_threads, int width, int height, int color_type, vge_apng_desc* descs, int64_t desc_cap,
                      int64_t* n_descs, vge_apng_segment* segs, int64_t seg_cap, int64_t* n_segs, int32_t* status,
                      int32_t* file_status, int64_t* workspace_bytes) {
  if (!mem_args_ok(data, data_bytes, offsets, sizes, n) || !layout_ok(width, height, color_type) || desc_cap < 0 ||
      (desc_cap > 0 && !descs) || seg_cap < 0 || (seg_cap > 0 && !segs) || !n_descs || !n_segs) {
    set_last_error("vge_apng_plan_mem: bad argument");
    return VGE_APNG_ERR_ARG;
  }
  const std::vector<View> views = mem_views(data, data_bytes, offsets, sizes, n);
  std::vector<Parsed> parsed;
  parse_views(views, n_threads, true, parsed);
  int64_t nd = 0, ns = 0;
  for (int i = 0; i < n; ++i) {
    nd += (int64_t)parsed[i].frames.size();
    for (const Frame& f : parsed[i].frames) ns += (int64_t)f.n_chunks;
  }
  *n_descs = nd;
  *n_segs = ns;  // an upper bound while counting: refused frames own no segment
  if (workspace_bytes) *workspace_bytes = 16;
  if ((descs && nd > desc_cap) || (segs && ns > seg_cap) || nd >= ((int64_t)1 << 31)) {
    set_last_error("vge_apng_plan_mem: desc_cap or seg_cap is smaller than the number of frames or data chunks");
    return VGE_APNG_ERR_ARG;
  }
  std::vector<int32_t> file_st((size_t)n, 0);
  if (!descs) {  // counting only: the parser's codes
    for (int i = 0; i < n; ++i) {
      vge_apng_info info;
      fill_info(parsed[i], info);
      file_st[i] = info.status != VGE_APNG_OK ? info.status
                   : (info.width != width || info.height != height || info.color_type != color_type)
                       ? VGE_APNG_ERR_SHAPE
                       : VGE_APNG_OK;
      if (file_status) file_status[i] = file_st[i];
    }
    return first_code("vge_apng_plan_mem", file_st);
  }
  int64_t ws = align16(nd * 8), k0 = 0;  // the inflate kernel's per-frame records come first
  ns = 0;
  for (int i = 0; i < n; ++i) {
    const Parsed& P = parsed[i];
    file_st[i] = resolve(P, width, height, color_type, i, k0, descs + k0);
    for (size_t k = 0; k < P.frames.size(); ++k) {
      vge_apng_desc& d = descs[k0 + (int64_t)k];
      if (status) status[k0 + (int64_t)k] = d.plan_status;
      if (d.plan_status != VGE_APNG_OK) continue;
      d.file_off = offsets[i];
      d.file_bytes = sizes[i];
      d.gat_off = ws;
      for (const Chunk& c : P.frames[k].chunks) {
        if (segs) segs[ns] = vge_apng_segment{offsets[i] + (int64_t)c.off, d.gat_off + d.gat_bytes, (int64_t)c.len,
                                              (int32_t)(k0 + (int64_t)k), 0};
        ++ns;
        d.gat_bytes += (int64_t)c.len;
      }
      ws = align16(ws + d.gat_bytes);
      d.slot_off = ws;
      ws = align16(ws + d.raw_bytes);
    }
    k0 += (int64_t)P.frames.size();
  }
  *n_segs = ns;
  if (workspace_bytes) *workspace_bytes = std::max<int64_t>(ws, 16);
  if (file_status)
    for (int i = 0; i < n; ++i) file_status[i] = file_st[i];
  return first_code("vge_apng_plan_mem", file_st);
}

size_t vge_apng_decode_device_workspace_bytes(const vge_apng_desc* descs, int n_descs) {
  int64_t ws = align16((int64_t)std::max(n_descs, 0) * 8);
  if (descs)
    for (int k = 0; k < n_descs; ++k)
      if (descs[k].frame >= 0 && descs[k].plan_status == VGE_APNG_OK) {
        ws = std::max(ws, align16(descs[k].gat_off + descs[k].gat_bytes));
        ws = std::max(ws, align16(descs[k].slot_off + descs[k].raw_bytes));
      }
  return (size_t)std::max<int64_t>(ws, 16);
}

}  // extern "C"
