// The host half of the GIF video front end (include/vge_gif.h): the block parser, the probe, the host decoder (the
// shared LZW and composition steps of vge_gif_lzw.h, in plain loops) and the plan of the device route.  Plain C++: no
// HIP, so that the parser and decoder can also be built into a stand-alone program under a sanitizer.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/vge_gif.h"
#include "vge_error.h"
#include "vge_gif_lzw.h"
#include "vge_host_files.h"

using vge::Mapped;
using vge::parallel_for;
using vge::set_last_error;

namespace {

using namespace vge_gif;

const char* status_name(int st) {
  switch (st) {
    case VGE_GIF_OK: return "ok";
    case VGE_GIF_ERR_ARG: return "bad argument";
    case VGE_GIF_ERR_IO: return "unreadable, truncated or corrupt GIF";
    case VGE_GIF_ERR_SHAPE: return "logical screen differs from the call's";
    case VGE_GIF_ERR_NO_PALETTE: return "unsupported GIF: a frame without any colour table";
    case VGE_GIF_ERR_BOUNDS: return "unsupported GIF: a frame reaches outside the logical screen";
    default: return "error";
  }
}

struct Block {
  size_t off, len;  // payload inside the file
};

struct Frame {
  int x = 0, y = 0, w = 0, h = 0, interlace = 0, mcs = 0;
  int transparent = -1, disposal_bits = 0;
  size_t ct_off = 0;
  int ct_size = 0;
  size_t lzw_bytes = 0, n_blocks = 0;
  std::vector<Block> blocks;  // the non-empty data sub-blocks (when the caller keeps them)
  int status = VGE_GIF_OK;    // what the parser alone sees
};

struct Parsed {
  int width = 0, height = 0, background = 0;
  int status = VGE_GIF_OK;  // the file-level code: set when the file has no frame to carry it
  std::vector<Frame> frames;
};

inline int le16(const uint8_t* p) { return p[0] | (p[1] << 8); }

// The block walk: everything a frame needs except its LZW codes.
void parse(const uint8_t* p, size_t n, Parsed& out, bool keep_blocks) {
  out = Parsed{};
  if (n >= ((size_t)1 << 28)) {
    out.status = VGE_GIF_ERR_ARG;
    return;
  }
  if (n < 13 || (memcmp(p, "GIF87a", 6) != 0 && memcmp(p, "GIF89a", 6) != 0)) {
    out.status = VGE_GIF_ERR_IO;
    return;
  }
  out.width = le16(p + 6);
  out.height = le16(p + 8);
  out.background = p[11];
  size_t at = 13, gct_off = 0;
  int gct_size = 0;
  if (p[10] & 0x80) {
    gct_size = 2 << (p[10] & 7);
    gct_off = at;
    if ((size_t)gct_size * 3 > n - at) {
      out.status = VGE_GIF_ERR_IO;
      return;
    }
    at += (size_t)gct_size * 3;
  }
  if (out.width == 0 || out.height == 0) {
    out.status = VGE_GIF_ERR_IO;
    return;
  }
  int transparent = -1, disposal_bits = 0;  // of the graphic control extension in front of the next image
  while (at < n) {
    const int b = p[at++];
    if (b == 0x3B) break;
    if (b == 0x21) {
      if (at >= n) break;
      const int label = p[at++];
      bool first = true;
      while (at < n) {  // the extension's sub-blocks
        const size_t len = p[at++];
        if (len == 0) break;
        const size_t have = std::min(len, n - at);
        if (first && label == 0xF9 && have >= 4) {
          const int flags = p[at];
          if (flags & 1) transparent = p[at + 3];
          disposal_bits = (flags >> 2) & 7;
        }
        first = false;
        at += have;
      }
      continue;
    }
    if (b != 0x2C) continue;  // Pillow skips bytes it does not know between blocks, and so do we
    out.frames.emplace_back();
    Frame& f = out.frames.back();
    f.transparent = transparent;
    f.disposal_bits = disposal_bits;
    transparent = -1;
    disposal_bits = 0;
    if (n - at < 9) {
      f.status = VGE_GIF_ERR_IO;
      break;
    }
    f.x = le16(p + at);
    f.y = le16(p + at + 2);
    f.w = le16(p + at + 4);
    f.h = le16(p + at + 6);
    const int flags = p[at + 8];
    at += 9;
    f.interlace = (flags >> 6) & 1;
    f.ct_off = gct_off;
    f.ct_size = gct_size;
    if (flags & 0x80) {
      f.ct_size = 2 << (flags & 7);
      f.ct_off = at;
      if ((size_t)f.ct_size * 3 > n - at) {
        f.status = VGE_GIF_ERR_IO;
        break;
      }
      at += (size_t)f.ct_size * 3;
    }
    if (at >= n) {
      f.status = VGE_GIF_ERR_IO;
      break;
    }
    f.mcs = p[at++];
    while (at < n) {  // the data sub-blocks; a file that ends inside them gives the decoder what is there
      const size_t len = p[at++];
      if (len == 0) break;
      const size_t have = std::min(len, n - at);
      if (have > 0) {
        if (keep_blocks) f.blocks.push_back(Block{at, have});
        f.lzw_bytes += have;
        f.n_blocks++;
      }
      at += have;
    }
    if (f.w == 0 || f.h == 0 || f.mcs < 2 || f.mcs > 8) f.status = VGE_GIF_ERR_IO;
    else if (f.ct_size == 0) f.status = VGE_GIF_ERR_NO_PALETTE;
    else if (f.x + f.w > out.width || f.y + f.h > out.height) f.status = VGE_GIF_ERR_BOUNDS;
  }
  if (out.frames.empty()) out.status = VGE_GIF_ERR_IO;  // no image
}

void fill_info(const Parsed& P, vge_gif_info& info) {
  info = vge_gif_info{};
  info.width = P.width;
  info.height = P.height;
  info.n_frames = (int32_t)P.frames.size();
  info.status = P.status;
  for (const Frame& f : P.frames) {
    info.lzw_bytes += (int64_t)f.lzw_bytes;
    info.n_blocks += (int64_t)f.n_blocks;
    if (info.status == VGE_GIF_OK) info.status = f.status;
  }
}

// A parsed file's frames as descriptors (without workspace offsets): the effective disposal method, the resolved fill
// colours, and the code that the first refused frame hands to every later one.  Returns the file's first failing code.
int resolve(const uint8_t* p, const Parsed& P, int width, int height, int file, int64_t first_frame,
            vge_gif_desc* descs) {
  if (P.status != VGE_GIF_OK) return P.status;
  int carried = P.width == width && P.height == height ? VGE_GIF_OK : VGE_GIF_ERR_SHAPE;
  int method = 0;
  for (size_t k = 0; k < P.frames.size(); ++k) {
    const Frame& f = P.frames[k];
    vge_gif_desc& d = descs[k];
    d = vge_gif_desc{};
    d.file = file;
    d.index = (int32_t)k;
    d.frame = (int32_t)(first_frame + (int64_t)k);
    d.x = f.x;
    d.y = f.y;
    d.w = f.w;
    d.h = f.h;
    d.interlace = f.interlace;
    d.min_code_size = f.mcs;
    d.transparent = f.transparent;
    d.ct_off = (int64_t)f.ct_off;
    d.ct_size = f.ct_size;
    d.fill_rgb = -1;
    if (f.disposal_bits) method = f.disposal_bits;  // an unspecified method inherits the previous frame's
    d.disposal = std::min(method, 3);
    if (carried == VGE_GIF_OK) carried = f.status;
    d.plan_status = carried;
    if (carried != VGE_GIF_OK) continue;
    const uint8_t* table = p + f.ct_off;
    const int t = f.transparent;
    if (k == 0) d.first_rgb = fill_color(table, f.ct_size, t >= 0 ? t : 0, 0);
    if (d.disposal == 2) d.fill_rgb = fill_color(table, f.ct_size, t >= 0 ? t : P.background, (int)k);
    else if (d.disposal == 3 && k == 0 && t >= 0) d.fill_rgb = fill_color(table, f.ct_size, t, 0);
  }
  return carried;
}

inline int read_code(const uint8_t* g, size_t n, uint64_t bit, int width) {
  const size_t b = (size_t)(bit >> 3);
  uint32_t v = g[b];
  if (b + 1 < n) v |= (uint32_t)g[b + 1] << 8;
  if (b + 2 < n) v |= (uint32_t)g[b + 2] << 16;
  return (int)((v >> (bit & 7)) & ((1u << width) - 1));
}

// One frame's sub-blocks -> its w * h indices.
int lzw_decode(const uint8_t* p, const Frame& f, uint8_t* out) {
  std::vector<uint8_t> g;
  g.reserve(f.lzw_bytes);
  for (const Block& b : f.blocks) g.insert(g.end(), p + b.off, p + b.off + b.len);
  const int64_t count = (int64_t)f.w * f.h;
  const uint64_t total = (uint64_t)g.size() * 8;
  std::vector<Entry> table(TABLE);
  for (int k = 0; k < clear_code(f.mcs) + 2; ++k) table[k] = initial_entry(f.mcs, k);
  Lzw L{f.mcs, 0, -1, 0, 0};
  uint64_t bit = 0;
  int64_t o = 0;
  while (o < count) {
    const int width = code_width(f.mcs, L.since);
    if (bit + (uint64_t)width > total) return VGE_GIF_ERR_IO;  // the data ends before the count
    const int code = read_code(g.data(), g.size(), bit, width);
    bit += (uint64_t)width;
    int len;
    const int r = lzw_step(L, table.data(), code, &len);
    if (r == STEP_BAD || r == STEP_END) return VGE_GIF_ERR_IO;
    if (r == STEP_CLEAR) continue;
    int c = code;
    for (int k = len - 1; k >= 0; --k) {
      const Entry e = table[c];
      if (o + k < count) out[o + k] = e.suffix;
      c = e.prefix;
    }
    o += len;
  }
  return VGE_GIF_OK;
}

struct View {
  const uint8_t* p = nullptr;
  size_t n = 0;
  int status = VGE_GIF_OK;  // why the file cannot be looked at
};

int first_code(const char* what, const std::vector<int32_t>& file_st) {
  for (size_t i = 0; i < file_st.size(); ++i)
    if (file_st[i] != VGE_GIF_OK) {
      set_last_error(std::string(what) + ": file " + std::to_string(i) + ": " + status_name(file_st[i]));
      return file_st[i];
    }
  return VGE_GIF_OK;
}

int decode_views(const char* what, const std::vector<View>& views, int n_threads, int width, int height,
                 int64_t frame_cap, uint8_t* rgb, int32_t* status, int32_t* file_status, int64_t* n_frames_out) {
  const int n = (int)views.size();
  std::vector<Parsed> parsed((size_t)n);
  parallel_for(n, n_threads, [&](int i) {
    if (views[i].status != VGE_GIF_OK) parsed[i].status = views[i].status;
    else parse(views[i].p, views[i].n, parsed[i], true);
  });
  std::vector<int64_t> first((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i) first[i + 1] = first[i] + (int64_t)parsed[i].frames.size();
  const int64_t total = first[n];
  if (n_frames_out) *n_frames_out = total;
  if (total > frame_cap || total >= ((int64_t)1 << 31)) {
    set_last_error(std::string(what) + ": the files hold more frames than frame_cap");
    return VGE_GIF_ERR_ARG;
  }
  std::vector<vge_gif_desc> descs((size_t)total);
  std::vector<int32_t> file_st((size_t)n, 0), lzw_st((size_t)total, 0);
  std::vector<int32_t> owner((size_t)total);
  for (int i = 0; i < n; ++i) {
    file_st[i] = resolve(views[i].p, parsed[i], width, height, i, first[i], descs.data() + first[i]);
    for (int64_t k = first[i]; k < first[i + 1]; ++k) owner[k] = i;
  }
  std::vector<std::vector<uint8_t>> planes((size_t)total);
  parallel_for((int)total, n_threads, [&](int k) {  // the LZW streams of all frames of all files
    const vge_gif_desc& d = descs[k];
    if (d.plan_status != VGE_GIF_OK) return;
    planes[k].resize((size_t)d.w * d.h);
    lzw_st[k] = lzw_decode(views[owner[k]].p, parsed[owner[k]].frames[d.index], planes[k].data());
  });
  const size_t npix = (size_t)width * height;
  parallel_for(n, n_threads, [&](int i) {
    if (first[i + 1] == first[i] || descs[first[i]].plan_status != VGE_GIF_OK) {
      for (int64_t k = first[i]; k < first[i + 1]; ++k)
        if (status) status[k] = descs[k].plan_status;
      return;
    }
    std::vector<Pixel> canvas(npix, Pixel{descs[first[i]].first_rgb, 0, 0});
    int carried = VGE_GIF_OK;
    for (int64_t k = first[i]; k < first[i + 1]; ++k) {
      const vge_gif_desc& d = descs[k];
      if (carried == VGE_GIF_OK) carried = d.plan_status != VGE_GIF_OK ? d.plan_status : lzw_st[k];
      if (status) status[k] = carried;
      if (carried != VGE_GIF_OK) continue;
      const uint8_t* table = views[i].p + d.ct_off;
      uint8_t* out = rgb + (size_t)k * npix * 3;
      size_t q = 0;
      for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x, ++q) {
          compose_pixel(canvas[q], d, x, y, planes[k].data(), table);
          const int32_t c = canvas[q].canvas;
          out[3 * q] = (uint8_t)c;
          out[3 * q + 1] = (uint8_t)(c >> 8);
          out[3 * q + 2] = (uint8_t)(c >> 16);
        }
    }
    if (file_st[i] == VGE_GIF_OK) file_st[i] = carried;
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

bool screen_ok(int width, int height) { return width > 0 && height > 0 && width <= 65535 && height <= 65535; }

constexpr int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

std::vector<View> mem_views(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes,
                            int n) {
  std::vector<View> views((size_t)n);
  for (int i = 0; i < n; ++i) {
    if (!inside(offsets[i], sizes[i], data_bytes)) views[i].status = VGE_GIF_ERR_ARG;
    else if (sizes[i] == 0) views[i].status = VGE_GIF_ERR_IO;
    else views[i] = View{data + offsets[i], (size_t)sizes[i], VGE_GIF_OK};
  }
  return views;
}

}  // namespace

extern "C" {

int vge_gif_probe(const char* const* paths, int n, int n_threads, vge_gif_info* info) {
  if (n < 0 || (n > 0 && (!paths || !info))) {
    set_last_error("vge_gif_probe: bad argument");
    return VGE_GIF_ERR_ARG;
  }
  std::vector<int32_t> st((size_t)n, 0);
  parallel_for(n, n_threads, [&](int i) {
    Mapped m(paths[i] ? paths[i] : "");
    Parsed P;
    if (m.ok) parse(m.p, m.n, P, false);
    else P.status = VGE_GIF_ERR_IO;
    fill_info(P, info[i]);
    st[i] = info[i].status;
  });
  return first_code("vge_gif_probe", st);
}

int vge_gif_probe_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                      int n_threads, vge_gif_info* info) {
  if (!mem_args_ok(data, data_bytes, offsets, sizes, n) || (n > 0 && !info)) {
    set_last_error("vge_gif_probe_mem: bad argument");
    return VGE_GIF_ERR_ARG;
  }
  const std::vector<View> views = mem_views(data, data_bytes, offsets, sizes, n);
  std::vector<int32_t> st((size_t)n, 0);
  parallel_for(n, n_threads, [&](int i) {
    Parsed P;
    if (views[i].status == VGE_GIF_OK) parse(views[i].p, views[i].n, P, false);
    else P.status = views[i].status;
    fill_info(P, info[i]);
    st[i] = info[i].status;
  });
  return first_code("vge_gif_probe_mem", st);
}

int vge_gif_decode(const char* const* paths, int n, int n_threads, int width, int height, int64_t frame_cap,
                   uint8_t* rgb, int32_t* status, int32_t* file_status, int64_t* n_frames_out) {
  if (n < 0 || !screen_ok(width, height) || frame_cap < 0 || (n > 0 && !paths) || (frame_cap > 0 && !rgb)) {
    set_last_error("vge_gif_decode: bad argument");
    return VGE_GIF_ERR_ARG;
  }
  std::vector<std::unique_ptr<Mapped>> maps((size_t)n);
  std::vector<View> views((size_t)n);
  for (int i = 0; i < n; ++i) {
    maps[i].reset(new Mapped(paths[i] ? paths[i] : ""));
    if (maps[i]->ok) views[i] = View{maps[i]->p, maps[i]->n, VGE_GIF_OK};
    else views[i].status = VGE_GIF_ERR_IO;
  }
  return decode_views("vge_gif_decode", views, n_threads, width, height, frame_cap, rgb, status, file_status,
                      n_frames_out);
}

int vge_gif_decode_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                       int n_threads, int width, int height, int64_t frame_cap, uint8_t* rgb, int32_t* status,
                       int32_t* file_status, int64_t* n_frames_out) {
  if (!mem_args_ok(data, data_bytes, offsets, sizes, n) || !screen_ok(width, height) || frame_cap < 0 ||
      (frame_cap > 0 && !rgb)) {
    set_last_error("vge_gif_decode_mem: bad argument");
    return VGE_GIF_ERR_ARG;
  }
  return decode_views("vge_gif_decode_mem", mem_views(data, data_bytes, offsets, sizes, n), n_threads, width, height,
                      frame_cap, rgb, status, file_status, n_frames_out);
}

int vge_gif_plan_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                     int n_threads, int width, int height, vge_gif_desc* descs, int64_t desc_cap, int64_t* n_descs,
                     vge_gif_segment* segs, int64_t seg_cap, int64_t* n_segs, int32_t* status, int32_t* file_status,
                     int64_t* workspace_bytes) {
  if (!mem_args_ok(data, data_bytes, offsets, sizes, n) || !screen_ok(width, height) || desc_cap < 0 ||
      (desc_cap > 0 && !descs) || seg_cap < 0 || (seg_cap > 0 && !segs) || !n_descs || !n_segs) {
    set_last_error("vge_gif_plan_mem: bad argument");
    return VGE_GIF_ERR_ARG;
  }
  const std::vector<View> views = mem_views(data, data_bytes, offsets, sizes, n);
  std::vector<Parsed> parsed((size_t)n);
  parallel_for(n, n_threads, [&](int i) {
    if (views[i].status != VGE_GIF_OK) parsed[i].status = views[i].status;
    else parse(views[i].p, views[i].n, parsed[i], true);
  });
  int64_t nd = 0, ns = 0;
  for (int i = 0; i < n; ++i) {
    nd += (int64_t)parsed[i].frames.size();
    for (const Frame& f : parsed[i].frames) ns += (int64_t)f.n_blocks;
  }
  *n_descs = nd;
  *n_segs = ns;  // an upper bound while counting: refused frames own no segment
  if (workspace_bytes) *workspace_bytes = 16;
  if ((descs && nd > desc_cap) || (segs && ns > seg_cap) || nd >= ((int64_t)1 << 31)) {
    set_last_error("vge_gif_plan_mem: desc_cap or seg_cap is smaller than the number of frames or data sub-blocks");
    return VGE_GIF_ERR_ARG;
  }
  std::vector<int32_t> file_st((size_t)n, 0);
  if (!descs) {  // counting only: the parser's codes
    for (int i = 0; i < n; ++i) {
      vge_gif_info info;
      fill_info(parsed[i], info);
      file_st[i] = info.status != VGE_GIF_OK ? info.status
                   : (info.width != width || info.height != height) ? VGE_GIF_ERR_SHAPE : VGE_GIF_OK;
      if (file_status) file_status[i] = file_st[i];
    }
    return first_code("vge_gif_plan_mem", file_st);
  }
  int64_t ws = 0, k0 = 0;
  ns = 0;
  for (int i = 0; i < n; ++i) {
    const Parsed& P = parsed[i];
    file_st[i] = resolve(views[i].p, P, width, height, i, k0, descs + k0);
    for (size_t k = 0; k < P.frames.size(); ++k) {
      vge_gif_desc& d = descs[k0 + (int64_t)k];
      if (status) status[k0 + (int64_t)k] = d.plan_status;
      if (d.plan_status != VGE_GIF_OK) continue;
      d.file_off = offsets[i];
      d.file_bytes = sizes[i];
      d.gat_off = ws;
      for (const Block& b : P.frames[k].blocks) {
        if (segs) segs[ns] = vge_gif_segment{offsets[i] + (int64_t)b.off, d.gat_off + d.gat_bytes, (int64_t)b.len,
                                             (int32_t)(k0 + (int64_t)k), 0};
        ++ns;
        d.gat_bytes += (int64_t)b.len;
      }
      ws = align16(ws + d.gat_bytes);
      d.slot_off = ws;
      ws = align16(ws + (int64_t)d.w * d.h);
    }
    k0 += (int64_t)P.frames.size();
  }
  *n_segs = ns;
  if (workspace_bytes) *workspace_bytes = std::max<int64_t>(ws, 16);
  if (file_status)
    for (int i = 0; i < n; ++i) file_status[i] = file_st[i];
  return first_code("vge_gif_plan_mem", file_st);
}

size_t vge_gif_decode_device_workspace_bytes(const vge_gif_desc* descs, int n_descs) {
  int64_t ws = 16;
  if (descs)
    for (int k = 0; k < n_descs; ++k)
      if (descs[k].frame >= 0 && descs[k].plan_status == VGE_GIF_OK) {
        ws = std::max(ws, align16(descs[k].gat_off + descs[k].gat_bytes));
        ws = std::max(ws, align16(descs[k].slot_off + (int64_t)descs[k].w * descs[k].h));
      }
  return (size_t)ws;
}

}  // extern "C"
