// The host half of the PNG frame front end (include/vge_png.h): the chunk parser, the probe, the host decoder (zlib's
// inflate and a plain C++ unfilter, vge_png_host.h, one frame per thread) and the plan of the device route.  Plain C++
// and zlib: no HIP.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vge_png.h"
#include "vge_error.h"
#include "vge_host_files.h"
#include "vge_png_host.h"

using vge::Mapped;
using vge::parallel_for;
using vge::set_last_error;
using vge_png_host::bytes_per_pixel;
using vge_png_host::Chunk;
using vge_png_host::inflate_chunks;
using vge_png_host::unfilter;

namespace {

const char* status_name(int st) {
  switch (st) {
    case VGE_PNG_OK: return "ok";
    case VGE_PNG_ERR_ARG: return "bad argument";
    case VGE_PNG_ERR_IO: return "unreadable, truncated or corrupt PNG";
    case VGE_PNG_ERR_SHAPE: return "width, height or colour type differ from the layout";
    case VGE_PNG_ERR_INTERLACED: return "unsupported PNG: interlaced";
    case VGE_PNG_ERR_BITDEPTH: return "unsupported PNG: bit depth other than 8";
    case VGE_PNG_ERR_PALETTE: return "unsupported PNG: palette";
    default: return "error";
  }
}

inline uint32_t be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

// The chunk walk: signature, IHDR, then every chunk up to the end of the one run of IDATs.  idat (may be NULL) receives
// the payload ranges, empty chunks included.  A chunk that runs past the file before the IDAT run has ended is a
// truncated file; whatever follows the run (IEND or its absence) is not looked at.
int parse(const uint8_t* p, size_t n, vge_png_info& info, std::vector<Chunk>* idat) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  info = vge_png_info{};
  if (n < 8 || memcmp(p, sig, 8) != 0) return VGE_PNG_ERR_IO;
  if (n < 8 + 8 + 13 + 4 || be32(p + 8) != 13 || memcmp(p + 12, "IHDR", 4) != 0) return VGE_PNG_ERR_IO;
  const uint8_t* h = p + 16;
  const uint32_t w = be32(h), hgt = be32(h + 4);
  const int depth = h[8], ct = h[9], comp = h[10], filt = h[11], lace = h[12];
  if (w == 0 || hgt == 0 || w > 0x7fffffffu || hgt > 0x7fffffffu) return VGE_PNG_ERR_IO;
  info.width = (int32_t)w;
  info.height = (int32_t)hgt;
  info.color_type = ct;
  info.bit_depth = depth;
  info.interlace = lace;
  const bool depth_ok = ct == 0   ? (depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16)
                        : ct == 3 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8)
                        : (ct == 2 || ct == 4 || ct == 6) ? (depth == 8 || depth == 16)
                                                          : false;
  if (!depth_ok || comp != 0 || filt != 0 || lace > 1) return VGE_PNG_ERR_IO;
  if (ct == 3) return VGE_PNG_ERR_PALETTE;
  if (depth != 8) return VGE_PNG_ERR_BITDEPTH;
  if (lace != 0) return VGE_PNG_ERR_INTERLACED;
  size_t at = 8 + 8 + 13 + 4;
  bool in_run = false;
  while (true) {
    if (n - at < 8) {
      if (in_run || at == n) break;  // the file ends between chunks
      return VGE_PNG_ERR_IO;
    }
    const size_t len = be32(p + at);
    const bool is_idat = memcmp(p + at + 4, "IDAT", 4) == 0;
    if (in_run && !is_idat) break;
    if (len > n - at - 8 || n - at - 8 - len < 4) return VGE_PNG_ERR_IO;  // payload and CRC lie inside the file
    if (is_idat) {
      in_run = true;
      info.n_idat++;
      info.idat_bytes += (int64_t)len;
      if (idat) idat->push_back(Chunk{at + 8, len});
    } else if (memcmp(p + at + 4, "IEND", 4) == 0) {
      break;
    }
    at += 8 + len + 4;
  }
  return info.n_idat > 0 ? VGE_PNG_OK : VGE_PNG_ERR_IO;
}

int check_layout(const vge_png_info& info, int width, int height, int color_type) {
  return info.width == width && info.height == height && info.color_type == color_type ? VGE_PNG_OK : VGE_PNG_ERR_SHAPE;
}

int decode_one(const uint8_t* p, size_t n, int width, int height, int color_type, uint8_t* rgb) {
  vge_png_info info;
  std::vector<Chunk> idat;
  int st = parse(p, n, info, &idat);
  if (st == VGE_PNG_OK) st = check_layout(info, width, height, color_type);
  if (st != VGE_PNG_OK) return st;
  const size_t count = (size_t)height * (1 + (size_t)width * bytes_per_pixel(color_type));
  std::vector<uint8_t> raw;
  if (!inflate_chunks(p, idat, count, raw)) return VGE_PNG_ERR_IO;
  return unfilter(raw.data(), width, height, color_type, rgb) ? VGE_PNG_OK : VGE_PNG_ERR_IO;
}

bool inside(int64_t off, int64_t size, int64_t data_bytes) {
  return off >= 0 && size >= 0 && off <= data_bytes && size <= data_bytes - off;
}

int finish(const char* what, const std::vector<int32_t>& st, int32_t* status) {
  int rc = VGE_PNG_OK;
  for (size_t i = 0; i < st.size(); ++i) {
    if (status) status[i] = st[i];
    if (rc == VGE_PNG_OK && st[i] != VGE_PNG_OK) {
      rc = st[i];
      set_last_error(std::string(what) + ": frame " + std::to_string(i) + ": " + status_name(rc));
    }
  }
  return rc;
}

bool mem_args_ok(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n) {
  return n >= 0 && data_bytes >= 0 && (n == 0 || (data && offsets && sizes));
}

bool layout_ok(int width, int height, int color_type) {
  return width > 0 && height > 0 && (color_type == 0 || color_type == 2 || color_type == 4 || color_type == 6);
}

constexpr int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

}  // namespace

extern "C" {

int vge_png_probe(const char* const* paths, int n, int n_threads, vge_png_info* info) {
  if (n < 0 || (n > 0 && (!paths || !info))) {
    set_last_error("vge_png_probe: bad argument");
    return VGE_PNG_ERR_ARG;
  }
  std::vector<int32_t> st((size_t)n, 0);
  parallel_for(n, n_threads, [&](int i) {
    Mapped m(paths[i] ? paths[i] : "");
    st[i] = m.ok ? parse(m.p, m.n, info[i], nullptr) : (info[i] = vge_png_info{}, VGE_PNG_ERR_IO);
    info[i].status = st[i];
  });
  return finish("vge_png_probe", st, nullptr);
}

int vge_png_probe_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                      int n_threads, vge_png_info* info) {
  if (!mem_args_ok(data, data_bytes, offsets, sizes, n) || (n > 0 && !info)) {
    set_last_error("vge_png_probe_mem: bad argument");
    return VGE_PNG_ERR_ARG;
  }
  std::vector<int32_t> st((size_t)n, 0);
  parallel_for(n, n_threads, [&](int i) {
    info[i] = vge_png_info{};
    st[i] = !inside(offsets[i], sizes[i], data_bytes) ? VGE_PNG_ERR_ARG
                                                      : parse(data + offsets[i], (size_t)sizes[i], info[i], nullptr);
    info[i].status = st[i];
  });
  return finish("vge_png_probe_mem", st, nullptr);
}

int vge_png_decode(const char* const* paths, int n, int n_threads, int width, int height, int color_type,
                   uint8_t* rgb, int32_t* status) {
  if (n < 0 || !layout_ok(width, height, color_type) || (n > 0 && (!paths || !rgb))) {
    set_last_error("vge_png_decode: bad argument");
    return VGE_PNG_ERR_ARG;
  }
  std::vector<int32_t> st((size_t)n, 0);
  const size_t frame = (size_t)width * height * 3;
  parallel_for(n, n_threads, [&](int i) {
    Mapped m(paths[i] ? paths[i] : "");
    st[i] = m.ok ? decode_one(m.p, m.n, width, height, color_type, rgb + i * frame) : VGE_PNG_ERR_IO;
  });
  return finish("vge_png_decode", st, status);
}

int vge_png_decode_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                       int n_threads, int width, int height, int color_type, uint8_t* rgb, int32_t* status) {
  if (!mem_args_ok(data, data_bytes, offsets, sizes, n) || !layout_ok(width, height, color_type) || (n > 0 && !rgb)) {
    set_last_error("vge_png_decode_mem: bad argument");
    return VGE_PNG_ERR_ARG;
  }
  std::vector<int32_t> st((size_t)n, 0);
  const size_t frame = (size_t)width * height * 3;
  parallel_for(n, n_threads, [&](int i) {
    st[i] = !inside(offsets[i], sizes[i], data_bytes)
                ? VGE_PNG_ERR_ARG
                : decode_one(data + offsets[i], (size_t)sizes[i], width, height, color_type, rgb + i * frame);
  });
  return finish("vge_png_decode_mem", st, status);
}

int vge_png_plan_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                     int n_threads, int width, int height, int color_type, vge_png_desc* descs, vge_png_segment* segs,
                     int64_t seg_cap, int64_t* n_segs, int32_t* status, int64_t* workspace_bytes) {
  if (!mem_args_ok(data, data_bytes, offsets, sizes, n) || !layout_ok(width, height, color_type) ||
      (n > 0 && !descs) || seg_cap < 0 || (seg_cap > 0 && !segs) || !n_segs) {
    set_last_error("vge_png_plan_mem: bad argument");
    return VGE_PNG_ERR_ARG;
  }
  std::vector<int32_t> st((size_t)n, 0);
  std::vector<std::vector<Chunk>> idat((size_t)n);
  const int64_t raw_bytes = (int64_t)height * (1 + (int64_t)width * bytes_per_pixel(color_type));
  parallel_for(n, n_threads, [&](int i) {
    vge_png_info info;
    if (!inside(offsets[i], sizes[i], data_bytes)) {
      st[i] = VGE_PNG_ERR_ARG;
      return;
    }
    st[i] = parse(data + offsets[i], (size_t)sizes[i], info, &idat[i]);
    if (st[i] == VGE_PNG_OK) st[i] = check_layout(info, width, height, color_type);
    if (st[i] == VGE_PNG_OK && (info.idat_bytes >= (1ll << 28) || raw_bytes >= (1ll << 31))) st[i] = VGE_PNG_ERR_ARG;
  });
  int64_t ws = align16((int64_t)n * 8);  // the inflate kernel's per-frame records come first
  int64_t ns = 0;
  for (int i = 0; i < n; ++i) {
    vge_png_desc& d = descs[i];
    d = vge_png_desc{};
    d.frame = -1;
    if (st[i] != VGE_PNG_OK) continue;
    d.file_off = offsets[i];
    d.file_bytes = sizes[i];
    d.color_type = color_type;
    d.frame = i;
    d.gat_off = ws;
    for (const Chunk& c : idat[i]) {
      if (c.len == 0) continue;
      if (ns < seg_cap) segs[ns] = vge_png_segment{offsets[i] + (int64_t)c.off, d.gat_off + d.gat_bytes, (int64_t)c.len, i, 0};
      ++ns;
      d.gat_bytes += (int64_t)c.len;
    }
    ws = align16(ws + d.gat_bytes);
    d.slot_off = ws;
    d.raw_bytes = raw_bytes;
    ws = align16(ws + raw_bytes);
  }
  *n_segs = ns;
  if (workspace_bytes) *workspace_bytes = std::max<int64_t>(ws, 16);
  if (segs && ns > seg_cap) {
    set_last_error("vge_png_plan_mem: seg_cap is smaller than the number of IDAT chunks");
    return VGE_PNG_ERR_ARG;
  }
  return finish("vge_png_plan_mem", st, status);
}

size_t vge_png_decode_device_workspace_bytes(const vge_png_desc* descs, int n_descs) {
  int64_t ws = align16((int64_t)std::max(n_descs, 0) * 8);
  if (descs)
    for (int k = 0; k < n_descs; ++k)
      if (descs[k].frame >= 0) {
        ws = std::max(ws, align16(descs[k].gat_off + descs[k].gat_bytes));
        ws = std::max(ws, align16(descs[k].slot_off + descs[k].raw_bytes));
      }
  return (size_t)std::max<int64_t>(ws, 16);
}

}  // extern "C"
