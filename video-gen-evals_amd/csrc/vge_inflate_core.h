// The device inflate core: what one wave needs to decode one deflate stream, whatever the stream belongs to.  Included
// by vge_inflate.hip (npz members -> the frame store) and vge_png.hip (a PNG frame's zlib stream -> its filtered rows);
// each gives the core a sink, the place the ring's new bytes go to.
//
// One wave (one 64-thread workgroup) owns one stream and nothing is shared between workgroups: no communication, no
// waiting, so a kernel that parses untrusted bytes has nothing to spin on.
//   history   a 32 KiB ring in LDS indexed by the uncompressed position.  Matched bytes other lanes stored a moment ago
//             are read back from LDS behind a workgroup barrier, never from global memory.
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
//   output    after every batch the ring's new bytes go to the sink as whole dwords with ordinary per-lane stores.
// Bounds: the reader never leaves [src, src + csize) (bytes beyond read as zero and the bit position is checked after
// every symbol); the sink is never handed a position at or beyond `total`; every loop consumes at least one input bit
// or produces at least one byte.
#ifndef VGE_INFLATE_CORE_H
#define VGE_INFLATE_CORE_H

#include <hip/hip_runtime.h>

#include "vge_inflate_tables.h"

namespace vge_inflate {

constexpr int WAVE = 64;             // one symbol per lane and batch
constexpr int RING = 32768;          // deflate's window
constexpr int RMASK = RING - 1;
constexpr int STAGE = 2048;          // compressed bytes staged in LDS per refill (+ 8 so that a peek never runs out)
constexpr int STAGE_DW = STAGE / 4 + 2;
constexpr int HEADER_MARGIN = 1024;  // a block header is at most 3 + 14 + 57 + 320 * 14 bits = 572 bytes
constexpr int BATCH_MARGIN = 512;    // a symbol is at most 15 + 5 + 15 + 13 bits: 64 of them are 384 bytes
constexpr int COPY_CHUNK = 16384;    // stored blocks pass through the ring in chunks the flush can follow
constexpr int LUT_L = 10, LUT_D = 8;
static_assert(WAVE * 258 + 3 < RING && COPY_CHUNK + 3 < RING, "a batch and the unflushed tail fit the ring");
static_assert(HEADER_MARGIN + 3 <= STAGE && BATCH_MARGIN + 3 <= STAGE, "margins fit the stage");

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

__device__ inline void refill(Reader& R, Shared& S, int32_t from_byte) {
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
__device__ inline void fill_luts(Shared& S) {
  for (int x = threadIdx.x; x < (1 << LUT_L); x += WAVE) S.lut_l[x] = (uint16_t)decode_msb(S.tl, brev_n(x, LUT_L), LUT_L);
  for (int x = threadIdx.x; x < (1 << LUT_D); x += WAVE) S.lut_d[x] = (uint16_t)decode_msb(S.td, brev_n(x, LUT_D), LUT_D);
  __syncthreads();
}

// lens[0, nl) and lens[nl, nl + nd) -> tl, td and the lookup tables; false: zlib rejects a set.
__device__ inline bool build_codes(Shared& S, int nl, int nd) {
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
__device__ inline bool dynamic_header(Reader& R, Shared& S, uint32_t end_bits) {
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

// The dword of ring positions [p, p + 4).
__device__ inline uint32_t ring_dword(Shared& S, uint32_t p) {
  if ((p & 3) == 0) return S.ring[(p & RMASK) >> 2];
  const uint8_t* rb = ring_bytes(S);
  return (uint32_t)rb[p & RMASK] | ((uint32_t)rb[(p + 1) & RMASK] << 8) | ((uint32_t)rb[(p + 2) & RMASK] << 16) |
         ((uint32_t)rb[(p + 3) & RMASK] << 24);
}

// The sink every stream so far has: uncompressed positions from `skip` on go to dst, whole dwords only.
struct DwordSink {
  uint32_t* dst;
  int64_t skip;
  // Ring positions [flushed, hi) -> the destination; returns the new `flushed`.
  __device__ int64_t flush(Shared& S, int64_t flushed, int64_t hi) const {
    __syncthreads();
    if (hi <= flushed) return flushed;
    const int64_t d0 = (flushed - skip) >> 2, d1 = (hi - skip) >> 2;
    for (int64_t d = d0 + threadIdx.x; d < d1; d += WAVE) dst[d] = ring_dword(S, (uint32_t)(skip + 4 * d));
    return skip + 4 * d1;
  }
};

// What became of a stream.
enum { STREAM_FAIL = 0,   // zlib would reject it, or it ended (or its input ran out) before `total` bytes
       STREAM_OPEN = 1,   // `total` bytes produced; the stream goes on, its input ran out, or what follows is unreadable
       STREAM_ENDED = 2   // `total` bytes produced and the final block ended exactly there, at bit R.bp
};

// Inflate `total` bytes of the raw deflate stream R reads (R.bp: its first bit) through the ring into the sink.
// TAIL false: stop as soon as `total` bytes are out (STREAM_OPEN).  TAIL true: read on, through end-of-block codes and
// empty blocks, until the final block has ended (STREAM_ENDED) or the stream tries to produce one more byte, runs out
// of input or cannot be read (STREAM_OPEN) -- what zlib does when it is offered one spare byte of output.
// On return every whole dword of [sink.skip, total) has been flushed; *flushed_out: the first position that has not.
template <bool TAIL, class Sink>
__device__ inline int inflate_stream(Reader& R, Shared& S, const Sink& sink, int64_t total, int64_t* flushed_out) {
  const int lane = threadIdx.x;
  const uint8_t* src = R.src;
  const int64_t csize = R.csize, skip = sink.skip;
  const uint32_t end_bits = (uint32_t)R.csize * 8u;
  uint8_t* rb = ring_bytes(S);
  int64_t pos = 0, flushed = skip;
  bool final_block = false;
  *flushed_out = flushed;
  refill(R, S, (int32_t)(R.bp >> 3));

  while (!final_block && (TAIL || pos < total)) {
    const bool past = TAIL && pos >= total;  // nothing that goes wrong from here on is the frame's failure
    ensure(R, S, HEADER_MARGIN);
    uint32_t w = peek(R, S);
    final_block = (w & 1) != 0;
    const int type = (int)((w >> 1) & 3);
    R.bp += 3;
    if (R.bp > end_bits || type == 3) return past ? STREAM_OPEN : STREAM_FAIL;
    if (type == 0) {
      R.bp = (R.bp + 7) & ~7u;
      w = peek(R, S);
      R.bp += 32;
      if (R.bp > end_bits || (w & 0xffffu) != ((~w >> 16) & 0xffffu)) return past ? STREAM_OPEN : STREAM_FAIL;
      const int64_t len = w & 0xffffu, from = R.bp >> 3;
      const int64_t n = len < total - pos ? len : total - pos;
      if (from + n > csize) return STREAM_FAIL;
      for (int64_t done = 0; done < n;) {
        const int c = (int)(n - done < COPY_CHUNK ? n - done : COPY_CHUNK);
        __syncthreads();
        for (int j = lane; j < c; j += WAVE) rb[(uint32_t)(pos + j) & RMASK] = src[from + done + j];
        pos += c;
        done += c;
        flushed = sink.flush(S, flushed, pos > skip ? pos : skip);
        *flushed_out = flushed;
      }
      if (TAIL && len > n) return STREAM_OPEN;  // the block holds a byte beyond the count
      R.bp = (uint32_t)(from + n) * 8u;
      continue;
    }
    if (type == 1) {
      __syncthreads();
      for (int s = lane; s < MAX_LENS; s += WAVE) S.lens[s] = (uint8_t)fixed_length(s);
      if (!build_codes(S, 288, 32)) return past ? STREAM_OPEN : STREAM_FAIL;
    } else if (!dynamic_header(R, S, end_bits)) {
      return past ? STREAM_OPEN : STREAM_FAIL;
    }

    bool eob = false;
    while (!eob && (TAIL || pos < total)) {  // one batch: up to WAVE symbols, lane k keeps the k-th
      ensure(R, S, BATCH_MARGIN);
      const int64_t base = pos;
      int my_kind = 0, my_val = 0, my_dist = 0, my_rel = 0;  // kind 1: literal my_val; 2: match of my_val bytes
      bool bad = false, over = false;  // over: the count is out and the stream wants to go on (or cannot be read)
      int k = 0;
      for (; k < WAVE && (TAIL || pos < total); ++k) {
        const bool full = TAIL && pos >= total;
        w = peek(R, S);
        uint32_t e = uni(S.lut_l[w & ((1 << LUT_L) - 1)]);
        if (e == 0) e = uni(decode_msb(S.tl, brev_n(w, MAX_BITS), MAX_BITS));
        if (e == 0) { bad = true; break; }
        int l = (int)(e & 15);
        const int sym = (int)(e >> 4);
        R.bp += l;
        if (sym < 256) {
          if (R.bp > end_bits) { bad = true; break; }
          if (full) { over = true; break; }
          if (lane == k) { my_kind = 1; my_val = sym; my_rel = (int)(pos - base); }
          pos += 1;
          continue;
        }
        if (sym == 256) {
          if (R.bp > end_bits) bad = true;
          eob = true;
          break;
        }
        if (full) { over = true; break; }
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
        if (R.bp > end_bits || dist > pos) { bad = true; break; }  // input exhausted / before the stream's first byte
        const int n = (int)(mlen < total - pos ? mlen : total - pos);
        if (lane == k) { my_kind = 2; my_val = n; my_dist = dist; my_rel = (int)(pos - base); }
        pos += n;
        if (TAIL && n < mlen) { over = true; break; }
      }
      if (bad) {
        if (!(TAIL && pos >= total)) return STREAM_FAIL;
        over = true;  // the symbols before it brought the count out: they are still to be copied
        eob = false;
      }

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
      flushed = sink.flush(S, flushed, pos > skip ? pos : skip);
      *flushed_out = flushed;
      if (over) return STREAM_OPEN;
    }
  }
  if (pos < total) return STREAM_FAIL;  // the stream ended before the count was reached
  return TAIL ? STREAM_ENDED : STREAM_OPEN;
}

}  // namespace vge_inflate
#endif  // VGE_INFLATE_CORE_H
