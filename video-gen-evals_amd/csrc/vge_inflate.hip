// Device inflate for the feature front end (include/vge_ingest.h): raw .npz / .npy bytes in device memory -> the rows
// of the device frame store, with no decoded floats staged on the host.
//
// One wave (one 64-thread workgroup) owns one stream -- one array of one video -- and nothing is shared between
// workgroups: no communication, no waiting, so a kernel that parses untrusted bytes has nothing to spin on.
//   history   a 32 KiB ring in LDS indexed by the uncompressed position, npy header included: matches that reach into
//             the header (numpy's space padding is coded as matches; a payload can repeat header bytes) read it there,
//             and only positions at or beyond `skip` are ever written to the destination.  Matched bytes other lanes
//             stored a moment ago are read back from LDS behind a workgroup barrier, never from global memory.
//   input     the compressed bytes are staged into LDS STAGE bytes at a time by all lanes; the bit reader works on LDS.
//   tables    vge_inflate_tables.h (shared with the host, which tests its rules against zlib): lane 0 sorts the
//             canonical code (a few hundred steps per block), then all lanes fill the lookup tables from it, one
//             entry per lane and step.
//   decode    sequential and wave-uniform: every lane decodes the same symbol, lane k keeps the k-th of a batch of 64
//             together with its output position (the running position is known to every lane, so no prefix sum is
//             needed to place the batch).
//   copy      literals are stored by their lanes; each match is copied by all lanes (an overlapping match of distance
//             d < length reads source byte j mod d); literal runs and matches alternate in stream order because a
//             later literal may overwrite ring bytes an earlier match of distance near 32 KiB still reads.
//   output    after every batch the ring's new bytes go to the destination as whole dwords with ordinary per-lane
//             stores (float32: the rows; float64: the workspace, converted by a second kernel).
// Bounds: every descriptor is checked against the buffer sizes and row counts the host passed; the reader never leaves
// [src, src + csize) (bytes beyond read as zero and the bit position is checked after every symbol); stores stay below
// `count` elements; every loop consumes at least one input bit or produces at least one byte.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vge_ingest.h"
#include "vge_error.h"
#include "vge_inflate_tables.h"

namespace {

using namespace vge_inflate;
using vge::set_last_error;

constexpr int WAVE = 64;             // one symbol per lane and batch
constexpr int RING = 32768;          // deflate's window
constexpr int RMASK = RING - 1;
constexpr int STAGE = 2048;          // compressed bytes staged in LDS per refill (+ 8 so that a peek never runs out)
constexpr int STAGE_DW = STAGE / 4 + 2;
constexpr int HEADER_MARGIN = 1024;  // a block header is at most 3 + 14 + 57 + 320 * 14 bits = 572 bytes
constexpr int BATCH_MARGIN = 512;    // a symbol is at most 15 + 5 + 15 + 13 bits: 64 of them are 384 bytes
constexpr int COPY_CHUNK = 16384;    // stored blocks pass through the ring in chunks the flush can follow
constexpr int LUT_L = 10, LUT_D = 8;
constexpr int ERR_HIP = 2;
static_assert(WAVE * 258 + 3 < RING && COPY_CHUNK + 3 < RING, "a batch and the unflushed tail fit the ring");
static_assert(HEADER_MARGIN + 3 <= STAGE && BATCH_MARGIN + 3 <= STAGE, "margins fit the stage");

struct Args {
  const uint8_t* data;
  int64_t data_bytes;
  const vge_inflate_desc* descs;
  int64_t n_rows, kp_rows;
  float* arr[5];
  uint8_t* ws;
  int64_t ws_bytes;
  int32_t* status;
  int32_t n_descs, n_videos, vit_dim;
};

struct Shared {
  uint32_t ring[RING / 4];
  uint32_t stage[STAGE_DW];
  uint16_t lut_l[1 << LUT_L];
  uint16_t lut_d[1 << LUT_D];
  Table tl, td;
  uint8_t lens[MAX_LENS];
  int32_t verdict;
};

__device__ inline uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

__device__ inline int array_width(int a, int vit_dim) { return a == 0 ? 207 : a == 1 ? 9 : a == 2 ? 10 : a == 3 ? vit_dim : 120; }

// 0: run it; -1: an unused slot; else the status code of a descriptor that does not fit what the host passed.
__device__ int check_desc(const Args& A, const vge_inflate_desc& d) {
  if (d.array < 0) return -1;
  if (d.array > 4 || d.video < 0 || d.video >= A.n_videos) return -1;  // nobody to report to
  if ((d.method != 0 && d.method != 8) || (d.itemsize != 4 && d.itemsize != 8) || d.skip < 0 || d.count < 0 ||
      d.csize < 0 || d.csize >= (1ll << 28) || d.src_off < 0 || d.src_off > A.data_bytes ||
      d.csize > A.data_bytes - d.src_off || d.dst_off < 0)
    return VGE_INGEST_ERR_ARG;
  const int64_t cap = (d.array == 4 ? A.kp_rows : A.n_rows) * (int64_t)array_width(d.array, A.vit_dim);
  if (d.dst_off > cap || d.count > cap - d.dst_off || A.arr[d.array] == nullptr) return VGE_INGEST_ERR_ARG;
  if (d.itemsize == 8 && (d.ws_off < 0 || (d.ws_off & 7) || d.ws_off > A.ws_bytes || d.count > (A.ws_bytes - d.ws_off) / 8))
    return VGE_INGEST_ERR_ARG;
  return 0;
}

__device__ inline void fail(const Args& A, int video, int code) {
  if (threadIdx.x == 0) atomicCAS(&A.status[video], 0, code);
}

// 4 bytes at src + off (inside the stream), by a dword load where the address allows
__device__ inline uint32_t load32(const uint8_t* src, int64_t off) {
  const uint8_t* p = src + off;
  if (((uintptr_t)p & 3) == 0) return *reinterpret_cast<const uint32_t*>(p);
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// The bit reader: wave-uniform state over the staged window [win, win + STAGE + 8) of the stream.  Either the window
// reaches the stream's end, or ensure() has put the bytes a caller is about to read below wend.
struct Reader {
  const uint8_t* src;
  int32_t csize;
  int32_t win;       // stream byte of stage[0]; may be -3..-1 so that the window starts on an aligned address
  int32_t wend;      // win + STAGE: positions below it can be peeked (the stage holds 8 bytes more)
  uint32_t bp;       // bit position in the stream
  uint32_t cbit;     // stream bit of cache bit 0
  uint64_t cache;    // 64 staged bits
  bool cached;
};

__device__ void refill(Reader& R, Shared& S, int32_t from_byte) {
  __syncthreads();
  R.win = from_byte - (int32_t)(((uintptr_t)R.src + (uintptr_t)from_byte) & 3);
  R.wend = R.win + STAGE;
  for (int k = threadIdx.x; k < STAGE_DW; k += WAVE) {
    const int32_t p = R.win + 4 * k;
    uint32_t v = 0;
    if (p >= 0 && p + 4 <= R.csize) {
      v = *reinterpret_cast<const uint32_t*>(R.src + p);  // aligned by the choice of win
    } else {
      for (int b = 0; b < 4; ++b)
        if (p + b >= 0 && p + b < R.csize) v |= (uint32_t)R.src[p + b] << (8 * b);
    }
    S.stage[k] = v;
  }
  __syncthreads();
  R.cached = false;
}

// Make the next `need` bytes from the current position peekable (or everything up to the stream's end).
__device__ inline void ensure(Reader& R, Shared& S, int need) {
  const int32_t b0 = (int32_t)(R.bp >> 3);
  if (b0 + need > R.wend && R.wend < R.csize) refill(R, S, b0);
}

// The next 32 stream bits (zero beyond the stream's end).
__device__ inline uint32_t peek(Reader& R, const Shared& S) {
  uint32_t off = R.bp - R.cbit;
  if (!R.cached || off > 32) {
    const uint32_t rel = R.bp - (uint32_t)(R.win * 8);  // win * 8 may be negative: the difference is not
    uint32_t idx = rel >> 5;
    if (idx > STAGE_DW - 2) idx = STAGE_DW - 2;          // only beyond the stream's end, where the caller stops
    const uint32_t lo = uni(S.stage[idx]), hi = uni(S.stage[idx + 1]);
    R.cache = (uint64_t)lo | ((uint64_t)hi << 32);
    R.cbit = R.bp - (rel & 31);
    R.cached = true;
    off = rel & 31;
  }
  return (uint32_t)(R.cache >> off);
}

__device__ inline uint32_t brev_n(uint32_t v, int n) { return __brev(v) >> (32 - n); }

// All lanes: the lookup tables from the sorted codes (index: the next stream bits; 0: a longer code or none).
__device__ void fill_luts(Shared& S) {
  for (int x = threadIdx.x; x < (1 << LUT_L); x += WAVE) S.lut_l[x] = (uint16_t)decode_msb(S.tl, brev_n(x, LUT_L), LUT_L);
  for (int x = threadIdx.x; x < (1 << LUT_D); x += WAVE) S.lut_d[x] = (uint16_t)decode_msb(S.td, brev_n(x, LUT_D), LUT_D);
  __syncthreads();
}

// lens[0, nl) and lens[nl, nl + nd) -> tl, td and the lookup tables; false: zlib rejects a set.
__device__ bool build_codes(Shared& S, int nl, int nd) {
  __syncthreads();
  if (threadIdx.x == 0) {
    int v = build_table(S.tl, S.lens, nl, KIND_LENS);
    if (v == 0) v = build_table(S.td, S.lens + nl, nd, KIND_DISTS);
    S.verdict = v;
  }
  __syncthreads();
  if (uni((uint32_t)S.verdict) != 0) return false;
  fill_luts(S);
  return true;
}

// Dynamic block header (after the 3 block bits) -> lens, tables.  false: rejected.
__device__ bool dynamic_header(Reader& R, Shared& S, uint32_t end_bits) {
  uint32_t w = peek(R, S);
  const int hlit = (int)(w & 31) + 257, hdist = (int)((w >> 5) & 31) + 1, hclen = (int)((w >> 10) & 15) + 4;
  R.bp += 14;
  if (hlit > 286 || hdist > 30) return false;
  __syncthreads();
  for (int i = threadIdx.x; i < 19; i += WAVE) S.lens[i] = 0;
  __syncthreads();
  for (int i = 0; i < hclen; ++i) {
    S.lens[clen_order(i)] = (uint8_t)(peek(R, S) & 7);
    R.bp += 3;
  }
  if (R.bp > end_bits) return false;
  __syncthreads();
  if (threadIdx.x == 0) S.verdict = build_table(S.td, S.lens, 19, KIND_CODES);  // td: free until the sets are read
  __syncthreads();
  if (uni((uint32_t)S.verdict) != 0) return false;
  const int total = hlit + hdist;
  int n = 0;
  while (n < total) {
    w = peek(R, S);
    const uint32_t e = uni(decode_msb(S.td, brev_n(w, 7), 7));
    if (e == 0) return false;
    const int l = (int)(e & 15), s = (int)(e >> 4);
    R.bp += l;
    w >>= l;
    if (s < 16) {
      S.lens[n++] = (uint8_t)s;
    } else {
      int v = 0, rep;
      if (s == 16) {
        if (n == 0) return false;
        v = (int)uni(S.lens[n - 1]);
        rep = 3 + (int)(w & 3);
        R.bp += 2;
      } else if (s == 17) {
        rep = 3 + (int)(w & 7);
        R.bp += 3;
      } else {
        rep = 11 + (int)(w & 127);
        R.bp += 7;
      }
      if (n + rep > total) return false;
      for (int k = 0; k < rep; ++k) S.lens[n + k] = (uint8_t)v;
      n += rep;
    }
    if (R.bp > end_bits) return false;
  }
  __syncthreads();
  if (uni(S.lens[256]) == 0) return false;  // no end-of-block code
  return build_codes(S, hlit, hdist);
}

__device__ inline uint8_t* ring_bytes(Shared& S) { return reinterpret_cast<uint8_t*>(S.ring); }

// Ring positions [flushed, hi) -> the destination, whole dwords only; returns the new `flushed`.
__device__ int64_t flush(Shared& S, uint32_t* dst, int64_t skip, int64_t flushed, int64_t hi) {
  __syncthreads();
  if (hi <= flushed) return flushed;
  const int64_t d0 = (flushed - skip) >> 2, d1 = (hi - skip) >> 2;
  const uint8_t* rb = ring_bytes(S);
  for (int64_t d = d0 + threadIdx.x; d < d1; d += WAVE) {
    const uint32_t p = (uint32_t)(skip + 4 * d);
    uint32_t v;
    if ((p & 3) == 0) {
      v = S.ring[(p & RMASK) >> 2];
    } else {
      v = (uint32_t)rb[p & RMASK] | ((uint32_t)rb[(p + 1) & RMASK] << 8) | ((uint32_t)rb[(p + 2) & RMASK] << 16) |
          ((uint32_t)rb[(p + 3) & RMASK] << 24);
    }
    dst[d] = v;
  }
  return skip + 4 * d1;
}

__global__ __launch_bounds__(WAVE) void inflate_kernel(Args A) {
  __shared__ Shared S;
  if (blockIdx.x >= (unsigned)A.n_descs) return;
  const vge_inflate_desc d = A.descs[blockIdx.x];
  const int chk = check_desc(A, d);
  if (chk < 0) return;
  if (chk > 0) return fail(A, d.video, chk);
  if (uni((uint32_t)A.status[d.video]) != 0) return;  // a sibling stream has failed already: the video is lost
  const int lane = threadIdx.x;
  const uint8_t* src = A.data + d.src_off;
  const int64_t skip = d.skip, total = skip + d.count * d.itemsize;
  uint32_t* dst = d.itemsize == 4 ? reinterpret_cast<uint32_t*>(A.arr[d.array] + d.dst_off)
                                  : reinterpret_cast<uint32_t*>(A.ws + d.ws_off);
  const int64_t n_dw = (total - skip) >> 2;

  if (d.method == 0) {  // stored member / plain .npy: the copy path
    if (total > d.csize) return fail(A, d.video, VGE_INGEST_ERR_IO);
    for (int64_t k = lane; k < n_dw; k += WAVE) dst[k] = load32(src, skip + 4 * k);
    return;
  }

  Reader R;
  R.src = src;
  R.csize = (int32_t)d.csize;
  R.bp = 0;
  R.cached = false;
  R.cbit = 0;
  R.cache = 0;
  refill(R, S, 0);
  const uint32_t end_bits = (uint32_t)d.csize * 8u;
  uint8_t* rb = ring_bytes(S);
  int64_t pos = 0, flushed = skip;
  bool final_block = false;

  while (pos < total && !final_block) {
    ensure(R, S, HEADER_MARGIN);
    uint32_t w = peek(R, S);
    final_block = (w & 1) != 0;
    const int type = (int)((w >> 1) & 3);
    R.bp += 3;
    if (R.bp > end_bits || type == 3) return fail(A, d.video, VGE_INGEST_ERR_IO);
    if (type == 0) {
      R.bp = (R.bp + 7) & ~7u;
      w = peek(R, S);
      R.bp += 32;
      if (R.bp > end_bits || (w & 0xffffu) != ((~w >> 16) & 0xffffu)) return fail(A, d.video, VGE_INGEST_ERR_IO);
      const int64_t len = w & 0xffffu, from = R.bp >> 3;
      const int64_t n = len < total - pos ? len : total - pos;
      if (from + n > d.csize) return fail(A, d.video, VGE_INGEST_ERR_IO);
      for (int64_t done = 0; done < n;) {
        const int c = (int)(n - done < COPY_CHUNK ? n - done : COPY_CHUNK);
        __syncthreads();
        for (int j = lane; j < c; j += WAVE) rb[(uint32_t)(pos + j) & RMASK] = src[from + done + j];
        pos += c;
        done += c;
        flushed = flush(S, dst, skip, flushed, pos > skip ? pos : skip);
      }
      R.bp = (uint32_t)(from + n) * 8u;
      continue;
    }
    if (type == 1) {
      __syncthreads();
      for (int s = lane; s < MAX_LENS; s += WAVE) S.lens[s] = (uint8_t)fixed_length(s);
      if (!build_codes(S, 288, 32)) return fail(A, d.video, VGE_INGEST_ERR_IO);
    } else if (!dynamic_header(R, S, end_bits)) {
      return fail(A, d.video, VGE_INGEST_ERR_IO);
    }

    bool eob = false;
    while (!eob && pos < total) {  // one batch: up to WAVE symbols, lane k keeps the k-th
      ensure(R, S, BATCH_MARGIN);
      const int64_t base = pos;
      int my_kind = 0, my_val = 0, my_dist = 0, my_rel = 0;  // kind 1: literal my_val; 2: match of my_val bytes
      bool bad = false;
      int k = 0;
      for (; k < WAVE && pos < total; ++k) {
        w = peek(R, S);
        uint32_t e = uni(S.lut_l[w & ((1 << LUT_L) - 1)]);
        if (e == 0) e = uni(decode_msb(S.tl, brev_n(w, MAX_BITS), MAX_BITS));
        if (e == 0) { bad = true; break; }
        int l = (int)(e & 15);
        const int sym = (int)(e >> 4);
        R.bp += l;
        if (sym < 256) {
          if (R.bp > end_bits) { bad = true; break; }
          if (lane == k) { my_kind = 1; my_val = sym; my_rel = (int)(pos - base); }
          pos += 1;
          continue;
        }
        if (sym == 256) {
          if (R.bp > end_bits) bad = true;
          eob = true;
          break;
        }
        if (sym >= 286) { bad = true; break; }
        const int li = sym - 257, lx = length_extra(li);
        const int mlen = length_base(li) + (int)((w >> l) & ((1u << lx) - 1));
        R.bp += lx;
        w = peek(R, S);
        e = uni(S.lut_d[w & ((1 << LUT_D) - 1)]);
        if (e == 0) e = uni(decode_msb(S.td, brev_n(w, MAX_BITS), MAX_BITS));
        if (e == 0) { bad = true; break; }
        l = (int)(e & 15);
        const int ds = (int)(e >> 4);
        if (ds >= 30) { bad = true; break; }
        const int dx = dist_extra(ds);
        const int dist = dist_base(ds) + (int)((w >> l) & ((1u << dx) - 1));
        R.bp += l + dx;
        if (R.bp > end_bits || dist > pos) { bad = true; break; }  // input exhausted / before the member's first byte
        const int n = (int)(mlen < total - pos ? mlen : total - pos);
        if (lane == k) { my_kind = 2; my_val = n; my_dist = dist; my_rel = (int)(pos - base); }
        pos += n;
      }
      if (bad) return fail(A, d.video, VGE_INGEST_ERR_IO);

      // copy stage, in stream order: the literals before each match, then the match by all lanes
      uint64_t matches = __ballot(my_kind == 2);
      int prev = 0;
      __syncthreads();
      while (matches) {
        const int m = __ffsll((unsigned long long)matches) - 1;
        matches &= matches - 1;
        if (my_kind == 1 && lane >= prev && lane < m) rb[(uint32_t)(base + my_rel) & RMASK] = (uint8_t)my_val;
        __syncthreads();
        const int mlen = __shfl(my_val, m), mdist = __shfl(my_dist, m);
        const uint32_t mp = (uint32_t)(base + __shfl(my_rel, m));
        for (int j = lane; j < mlen; j += WAVE) {
          const int sj = mdist >= mlen ? j : j % mdist;
          rb[(mp + j) & RMASK] = rb[(mp - mdist + sj) & RMASK];
        }
        __syncthreads();
        prev = m + 1;
      }
      if (my_kind == 1 && lane >= prev) rb[(uint32_t)(base + my_rel) & RMASK] = (uint8_t)my_val;
      flushed = flush(S, dst, skip, flushed, pos > skip ? pos : skip);
    }
  }
  if (pos < total) return fail(A, d.video, VGE_INGEST_ERR_IO);  // the stream ended before the count was reached
}

// float64 streams: workspace -> rows, with the host's (float) rounding.
__global__ __launch_bounds__(256) void convert_kernel(Args A) {
  if (blockIdx.x >= (unsigned)A.n_descs) return;
  const vge_inflate_desc d = A.descs[blockIdx.x];
  if (check_desc(A, d) != 0 || d.itemsize != 8 || A.status[d.video] != 0) return;
  const double* in = reinterpret_cast<const double*>(A.ws + d.ws_off);
  float* out = A.arr[d.array] + d.dst_off;
  for (int64_t i = threadIdx.x; i < d.count; i += 256) out[i] = (float)in[i];
}

}  // namespace

extern "C" int vge_ingest_decode_device_batch_symbols(void) { return WAVE; }
extern "C" int vge_ingest_decode_device_ring_bytes(void) { return RING; }
extern "C" int vge_ingest_decode_device_stage_bytes(void) { return STAGE; }

extern "C" size_t vge_ingest_decode_device_workspace_bytes(const vge_inflate_desc* descs, int n_descs) {
  int64_t ws = 0;
  if (descs)
    for (int k = 0; k < n_descs; ++k)
      if (descs[k].array >= 0 && descs[k].itemsize == 8 && descs[k].count > 0) ws += descs[k].count * 8;
  return (size_t)(ws > 8 ? ws : 8);
}

extern "C" int vge_ingest_decode_device(const uint8_t* data, int64_t data_bytes, const vge_inflate_desc* descs,
                                        int n_descs, int n_videos, int64_t n_rows, int64_t kp_rows, int vit_dim,
                                        float* pose, float* gori, float* betas, float* vit, float* kp, void* workspace,
                                        int64_t workspace_bytes, int32_t* status, void* stream) {
  if (n_descs < 0 || n_videos < 0 || data_bytes < 0 || n_rows < 0 || kp_rows < 0 || vit_dim < 1 ||
      workspace_bytes < 0) {
    set_last_error("vge_ingest_decode_device: bad argument (negative count or size)");
    return VGE_INGEST_ERR_ARG;
  }
  if (n_videos == 0 || n_descs == 0) return VGE_INGEST_OK;
  if (!data || !descs || !status || !workspace || !pose || !gori || !betas || !vit || ((uintptr_t)descs & 7) ||
      ((uintptr_t)workspace & 7) || ((uintptr_t)status & 3) || ((uintptr_t)pose & 3) || ((uintptr_t)gori & 3) ||
      ((uintptr_t)betas & 3) || ((uintptr_t)vit & 3) || ((uintptr_t)kp & 3)) {
    set_last_error("vge_ingest_decode_device: bad argument (null or misaligned buffer)");
    return VGE_INGEST_ERR_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(status, 0, (size_t)n_videos * 4, s) != hipSuccess) {
    set_last_error(std::string("vge_ingest_decode_device: ") + hipGetErrorString(hipGetLastError()));
    return ERR_HIP;
  }
  Args A;
  A.data = data;
  A.data_bytes = data_bytes;
  A.descs = descs;
  A.n_rows = n_rows;
  A.kp_rows = kp_rows;
  A.arr[0] = pose;
  A.arr[1] = gori;
  A.arr[2] = betas;
  A.arr[3] = vit;
  A.arr[4] = kp;
  A.ws = static_cast<uint8_t*>(workspace);
  A.ws_bytes = workspace_bytes;
  A.status = status;
  A.n_descs = n_descs;
  A.n_videos = n_videos;
  A.vit_dim = vit_dim;
  hipLaunchKernelGGL(inflate_kernel, dim3((unsigned)n_descs), dim3(WAVE), 0, s, A);
  hipLaunchKernelGGL(convert_kernel, dim3((unsigned)n_descs), dim3(256), 0, s, A);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_last_error(std::string("vge_ingest_decode_device: ") + hipGetErrorString(e));
    return ERR_HIP;
  }
  return VGE_INGEST_OK;
}
