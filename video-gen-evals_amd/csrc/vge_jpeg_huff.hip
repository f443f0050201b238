// Device entropy coder (include/vge_frames.h): the coefficients vge_jpeg_forward leaves -> complete baseline JPEG files,
// byte for byte what encode_file (vge_jpeg.cpp) writes.  Huffman ENcoding has no serial dependency that matters: a
// block's DC predictor is the stored DC of the previous block of its component in scan order, whose position the layout
// gives in closed form, and everything else is three prefix sums.  No workgroup ever waits for another: the phases are
// separate launches ordered by the stream.
//
//   plan  1 huff_count     a workgroup per SEGMENT (SEG = 128 consecutive blocks of one frame's scan), a wave per block,
//                          a lane per zigzag position: lane k's code is a function of its coefficient and of the
//                          ballot of non-zero lanes (its zero run is the distance to the previous set bit), so a block
//                          is one wave scan with no loop over coefficients.  Writes bits per block and per segment.
//         2 huff_seg_scan  a workgroup per frame: exclusive scan of the segments' bit counts (wave scans + LDS), the
//                          frame's scan length, its refusal flag; clears the scan words that two segments share.
//         3 huff_pack      the segment's blocks again, each lane ORs its <= 59 bits into the segment's zeroed bit
//                          string in LDS at (block start + lane prefix); the string goes out byte-swapped, whole words
//                          by plain stores, the first / last partial word by atomic OR into the words step 2 cleared.
//         4 huff_ff_count  a workgroup per CHUNK (4096 scan bytes): the chunk's FF bytes.
//         5 huff_ff_scan   a workgroup per frame: exclusive scan of the chunks' FF counts; sizes[] and status[].
//   emit  6 huff_emit      a workgroup per chunk: a block scan of FF counts places every byte, the stuffed chunk is
//                          built in LDS and copied out with consecutive lanes on consecutive bytes; chunk 0 also
//                          writes the header (a compile-time template + the tables and the frame size) and EOI.
// Every loop is bounded by the layout: a block is at most 20 + 63 * 26 = 1,658 bits, a segment SEG blocks, a frame
// ceil(blocks / SEG) segments and ceil(blocks * 1658 / 8 / CHUNK) chunks.  The code / length tables and the header's
// DHT segments are derived at compile time from the arrays the host coder uses (vge_jpeg_huff_tables.h).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/vge_frames.h"
#include "vge_error.h"
#include "vge_jpeg_huff_tables.h"

using vge::set_last_error;

namespace {

constexpr int SEG = 128;              // scan blocks per workgroup (vge_jpeg_entropy_segment_blocks)
constexpr int BLOCK_BITS_MAX = 1658;  // DC 9 + 11 (chroma: 11 + 11 with AC 63 * (16 + 10) is the same bound or less)
constexpr int OBUF_WORDS = (SEG * BLOCK_BITS_MAX + 31 + 7 + 31) / 32 + 1;  // a segment's bits from any bit phase + pad
constexpr int CHUNK = 4096;           // unstuffed scan bytes per workgroup: 256 lanes x 16 bytes
constexpr int HDR = 623;              // SOI .. SOS
constexpr uint32_t BAD = 0x80000000u;

// ---- compile-time tables
struct HuffLut {
  uint32_t ac[2][256];  // code | length << 16, by symbol; [0] luminance, [1] chrominance
  uint32_t dc[2][16];
};

constexpr void fill_lut(uint32_t* dst, const uint8_t* bits, const uint8_t* vals) {
  uint32_t c = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l - 1]; ++i, ++k, ++c) dst[vals[k]] = c | ((uint32_t)l << 16);
    c <<= 1;
  }
}

constexpr HuffLut make_lut() {
  HuffLut t{};
  fill_lut(t.ac[0], vge_jpeg::kAcLumaBits, vge_jpeg::kAcLumaVals);
  fill_lut(t.ac[1], vge_jpeg::kAcChromaBits, vge_jpeg::kAcChromaVals);
  fill_lut(t.dc[0], vge_jpeg::kDcLumaBits, vge_jpeg::kDcVals);
  fill_lut(t.dc[1], vge_jpeg::kDcChromaBits, vge_jpeg::kDcVals);
  return t;
}

// SOI, APP0 (JFIF 1.01, no density unit, 1 x 1), two DQT, SOF0, four DHT, SOS: libjpeg's defaults (jcmarker.c), as
// encode_file writes them.  The quantisation entries, the frame size and the luma sampling byte are filled in per call.
constexpr int DQT0 = 20, SOF = 158, DHT0 = 177, SOS = 609;
struct Header {
  uint8_t b[HDR];
  uint8_t zigzag[64];
};

constexpr int put_dht(uint8_t* b, int o, int id, const uint8_t* bits, const uint8_t* vals) {
  int n = 0;
  for (int l = 0; l < 16; ++l) n += bits[l];
  b[o++] = 0xFF;
  b[o++] = 0xC4;
  b[o++] = (uint8_t)((n + 19) >> 8);
  b[o++] = (uint8_t)((n + 19) & 255);
  b[o++] = (uint8_t)id;
  for (int l = 0; l < 16; ++l) b[o++] = bits[l];
  for (int i = 0; i < n; ++i) b[o++] = vals[i];
  return o;
}

constexpr Header make_header() {
  Header h{};
  const uint8_t head[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  for (int i = 0; i < 20; ++i) h.b[i] = head[i];
  for (int t = 0; t < 2; ++t) {
    const int o = DQT0 + 69 * t;
    h.b[o] = 0xFF;
    h.b[o + 1] = 0xDB;
    h.b[o + 2] = 0;
    h.b[o + 3] = 67;
    h.b[o + 4] = (uint8_t)t;
  }
  const uint8_t sof[19] = {0xFF, 0xC0, 0, 17, 8, 0, 0, 0, 0, 3, 1, 0, 0, 2, 0x11, 1, 3, 0x11, 1};
  for (int i = 0; i < 19; ++i) h.b[SOF + i] = sof[i];
  int o = DHT0;
  o = put_dht(h.b, o, 0x00, vge_jpeg::kDcLumaBits, vge_jpeg::kDcVals);
  o = put_dht(h.b, o, 0x10, vge_jpeg::kAcLumaBits, vge_jpeg::kAcLumaVals);
  o = put_dht(h.b, o, 0x01, vge_jpeg::kDcChromaBits, vge_jpeg::kDcVals);
  o = put_dht(h.b, o, 0x11, vge_jpeg::kAcChromaBits, vge_jpeg::kAcChromaVals);
  const uint8_t sos[14] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  for (int i = 0; i < 14; ++i) h.b[o + i] = sos[i];
  for (int i = 0; i < 64; ++i) h.zigzag[i] = vge_jpeg::kZigzag[i];
  return h;
}
static_assert(DHT0 + 33 + 183 + 33 + 183 == SOS && SOS + 14 == HDR, "header offsets");

__constant__ HuffLut d_lut = make_lut();
__constant__ Header d_header = make_header();

// ---- workspace: everything the kernels exchange, carved from the caller's buffer
struct FrameInfo {
  uint32_t scan_bytes;  // unstuffed scan, padded to a whole byte
  uint32_t ff_total;    // FF bytes in it
  uint32_t bad;         // a coefficient baseline coding cannot carry
  uint32_t pad;
};

struct Plan {
  vge_jpeg_layout L;
  int n_frames, S, nseg, nchunk;  // S: blocks per frame; segments and (worst case) chunks per frame
  uint32_t pitch_words;           // scan words per frame
  uint32_t* scan;                 // [n][pitch_words]  the unstuffed scan, stream byte order
  uint32_t* seg_bits;             // [n][nseg]  bits of a segment | BAD
  uint32_t* seg_off;              // [n][nseg]  first bit of a segment
  uint32_t* chunk_ff;             // [n][nchunk]
  uint32_t* chunk_off;            // [n][nchunk] FF bytes before a chunk
  FrameInfo* info;                // [n]
  uint16_t* blk_bits;             // [n][S]
  size_t bytes;
};

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// False: not a 3-component layout of vge_jpeg_make_layout, or too large for 32-bit bit positions.
bool make_plan(const vge_jpeg_layout* layout, int n_frames, void* workspace, Plan& P, int* err) {
  vge_jpeg_layout want;
  *err = VGE_JPEG_ERR_ARG;
  if (n_frames < 0 || !layout ||
      vge_jpeg_make_layout(layout->width, layout->height, layout->n_comp, layout->h0, layout->v0, &want) != VGE_JPEG_OK ||
      memcmp(&want, layout, sizeof(want)) != 0)
    return false;
  if (want.n_comp != 3) {
    *err = VGE_JPEG_ERR_COMPONENTS;
    return false;
  }
  const long long max_bits = (long long)want.blocks_per_frame * BLOCK_BITS_MAX + 7;
  if (max_bits >= 0x7fffffffLL) return false;
  P.L = want;
  P.n_frames = n_frames;
  P.S = want.blocks_per_frame;
  P.nseg = (P.S + SEG - 1) / SEG;
  const size_t max_bytes = (size_t)(max_bits / 8);
  P.nchunk = (int)((max_bytes + CHUNK - 1) / CHUNK);
  P.pitch_words = (uint32_t)(align16(max_bytes + 8) / 4);
  const size_t n = (size_t)n_frames;
  const uintptr_t base = reinterpret_cast<uintptr_t>(workspace);  // null when only the size is asked for
  size_t o = 0;
  auto carve = [&](size_t bytes) {
    void* q = reinterpret_cast<void*>(base + o);
    o += align16(bytes);
    return q;
  };
  P.scan = static_cast<uint32_t*>(carve(n * P.pitch_words * 4));
  P.seg_bits = static_cast<uint32_t*>(carve(n * P.nseg * 4));
  P.seg_off = static_cast<uint32_t*>(carve(n * P.nseg * 4));
  P.chunk_ff = static_cast<uint32_t*>(carve(n * P.nchunk * 4));
  P.chunk_off = static_cast<uint32_t*>(carve(n * P.nchunk * 4));
  P.info = static_cast<FrameInfo*>(carve(n * sizeof(FrameInfo)));
  P.blk_bits = static_cast<uint16_t*>(carve(n * P.S * 2));
  P.bytes = o;
  return true;
}

// ---- wave and workgroup scans (256 threads)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

// Exclusive prefix of v over the workgroup and the workgroup's total; tmp: 4 words of LDS.  Ends on a barrier that
// makes tmp reusable.
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* tmp, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t incl = wave_incl_scan(v, lane);
  if (lane == 63) tmp[wave] = incl;
  __syncthreads();
  const uint32_t t0 = tmp[0], t1 = tmp[1], t2 = tmp[2], t3 = tmp[3];
  __syncthreads();
  *total = t0 + t1 + t2 + t3;
  return incl - v + (wave > 0 ? t0 : 0u) + (wave > 1 ? t1 : 0u) + (wave > 2 ? t2 : 0u);
}

// ---- the scan order
// Luma block j of MCU m -> its index in the frame's coefficient buffer.
__device__ __forceinline__ int luma_block(const vge_jpeg_layout& L, int m, int j) {
  const int my = m / L.mcus_x, mx = m - my * L.mcus_x;
  const int v = j / L.h0, h = j - v * L.h0;
  return L.off[0] + (my * L.v0 + v) * L.bw[0] + mx * L.h0 + h;
}

// Scan position s of a frame -> its block, the block whose DC is its predictor (-1: none, predictor 0), its table.
__device__ __forceinline__ void scan_block(const vge_jpeg_layout& L, int s, int* blk, int* prev, int* tbl) {
  const int nl = L.h0 * L.v0, B = nl + 2;
  const int m = s / B, j = s - m * B;
  if (j < nl) {
    *blk = luma_block(L, m, j);
    *prev = j > 0 ? luma_block(L, m, j - 1) : (m > 0 ? luma_block(L, m - 1, nl - 1) : -1);
    *tbl = 0;
  } else {  // a chroma plane is mcus_x x mcus_y blocks, row-major: MCU m's block is block m
    *blk = (j == nl ? L.off[1] : L.off[2]) + m;
    *prev = m > 0 ? *blk - 1 : -1;
    *tbl = 1;
  }
}

// The segment's scan positions resolved once, a thread per position, instead of by every wave in its loop (the integer
// divisions above are ~250 scalar instructions).  sblk / sprev: SEG ints of LDS each; the caller's barrier publishes them.
__device__ __forceinline__ void resolve_segment(const vge_jpeg_layout& L, int s0, int nb, int* sblk, int* sprev) {
  if ((int)threadIdx.x < nb) {
    int blk, prev, tbl;
    scan_block(L, s0 + threadIdx.x, &blk, &prev, &tbl);
    sblk[threadIdx.x] = blk;
    sprev[threadIdx.x] = prev;
  }
}

// ---- one block: lane k codes zigzag position k.  lut: the LDS copy of d_lut.
struct LaneCode {
  uint64_t bits;  // right-aligned
  uint32_t len;   // <= 3 * 11 + 16 + 10 = 59
};

__device__ __forceinline__ const uint32_t* lut_ac(const uint32_t* lut, int tbl) { return lut + 256 * tbl; }
__device__ __forceinline__ const uint32_t* lut_dc(const uint32_t* lut, int tbl) { return lut + 512 + 16 * tbl; }

// coef: the frame's coefficients; zz: this lane's natural index.  *bad (wave-uniform): the block cannot be coded, its
// offending lanes emit nothing.
__device__ __forceinline__ LaneCode code_lane(const int16_t* coef, int blk, int prev, int tbl, int lane, int zz,
                                              const uint32_t* lut, bool* bad) {
  int val = coef[(size_t)blk * 64 + zz];
  if (lane == 0 && prev >= 0) val -= coef[(size_t)prev * 64];
  const unsigned long long nz = __ballot(lane > 0 && val != 0);
  const int mag = val < 0 ? -val : val;
  int n = 32 - __clz(mag);  // __clz(0) is 32
  const bool over = n > (lane == 0 ? 11 : 10);
  *bad = __any(over);
  if (over) n = 0;
  const uint32_t mant = (uint32_t)(val < 0 ? val - 1 : val) & ((1u << n) - 1u);
  LaneCode c{0, 0};
  if (over) return c;
  if (lane == 0) {
    const uint32_t e = lut_dc(lut, tbl)[n];
    c.bits = ((uint64_t)(e & 0xffffu) << n) | mant;
    c.len = (e >> 16) + n;
  } else if (val != 0) {
    const unsigned long long below = nz & ((1ull << lane) - 1ull);
    const int last = below ? 63 - __clzll((long long)below) : 0;  // the previous coded position (0: the DC)
    const int run = lane - last - 1, zrl = run >> 4;
    const uint32_t e = lut_ac(lut, tbl)[((run & 15) << 4) | n], z = lut_ac(lut, tbl)[0xF0];
    const uint32_t zl = z >> 16, el = (e >> 16) + n;
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)  // run <= 62: at most three ZRLs
      if (i < zrl) acc = (acc << zl) | (z & 0xffffu);
    c.bits = (acc << el) | ((uint64_t)(e & 0xffffu) << n) | mant;
    c.len = zrl * zl + el;
  } else if (lane == 63) {  // the block ends in zeros: EOB
    const uint32_t e = lut_ac(lut, tbl)[0];
    c.bits = e & 0xffffu;
    c.len = e >> 16;
  }
  return c;
}

__device__ __forceinline__ void load_lut(uint32_t* lut) {
  for (int i = threadIdx.x; i < 512 + 32; i += 256)
    lut[i] = i < 512 ? d_lut.ac[i >> 8][i & 255] : d_lut.dc[(i - 512) >> 4][i & 15];
}

// ---- 1: bits per block and per segment
__global__ __launch_bounds__(256) void huff_count_kernel(const Plan P, const int16_t* __restrict__ coef_all) {
  __shared__ uint32_t lut[512 + 32];
  __shared__ uint32_t wsum[4];
  __shared__ int sblk[SEG], sprev[SEG];
  const int f = blockIdx.x / P.nseg, seg = blockIdx.x - f * P.nseg;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s0 = seg * SEG, nb = min(SEG, P.S - s0);
  load_lut(lut);
  resolve_segment(P.L, s0, nb, sblk, sprev);
  __syncthreads();
  const int zz = d_header.zigzag[lane];
  const int16_t* coef = coef_all + (size_t)f * P.S * 64;
  uint32_t sum = 0;
  for (int i = wave; i < nb; i += 4) {
    const int blk = sblk[i], prev = sprev[i], tbl = blk >= P.L.off[1] ? 1 : 0;
    bool bad;
    const LaneCode c = code_lane(coef, blk, prev, tbl, lane, zz, lut, &bad);
    const uint32_t total = __shfl(wave_incl_scan(c.len, lane), 63);
    if (lane == 0) P.blk_bits[(size_t)f * P.S + s0 + i] = (uint16_t)total;
    sum = (sum + total) | (bad ? BAD : 0u);
  }
  if (lane == 0) wsum[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t a = wsum[0], b = wsum[1], c = wsum[2], d = wsum[3];
    P.seg_bits[blockIdx.x] = (((a & ~BAD) + (b & ~BAD) + (c & ~BAD) + (d & ~BAD))) | ((a | b | c | d) & BAD);
  }
}

// ---- 2: where each segment starts; the frame's length; clear the words two segments share
__global__ __launch_bounds__(256) void huff_seg_scan_kernel(const Plan P) {
  __shared__ uint32_t tmp[4];
  const int f = blockIdx.x, tid = threadIdx.x;
  uint32_t* scan = P.scan + (size_t)f * P.pitch_words;
  uint32_t carry = 0, bad = 0;
  for (int base = 0; base < P.nseg; base += 256) {
    const int idx = base + tid;
    const uint32_t raw = idx < P.nseg ? P.seg_bits[(size_t)f * P.nseg + idx] : 0u;
    uint32_t total;
    const uint32_t off = carry + block_excl_scan(raw & ~BAD, tmp, &total);
    bad |= raw & BAD;
    if (idx < P.nseg) {
      P.seg_off[(size_t)f * P.nseg + idx] = off;
      scan[off >> 5] = 0;  // the word a segment starts in: its predecessor's last bits are ORed into it too
    }
    carry += total;
  }
  const bool any_bad = __syncthreads_or(bad != 0);
  if (tid == 0) {
    scan[carry >> 5] = 0;  // the word the scan ends in (inside the pitch: it has 8 bytes of slack)
    FrameInfo I;
    I.scan_bytes = (carry + 7) >> 3;
    I.ff_total = 0;
    I.bad = any_bad ? 1u : 0u;
    I.pad = 0;
    P.info[f] = I;
  }
}

// ORs the low `len` bits of `bits` into the big-endian bit string obuf at bit q (MSB of word 0 is bit 0).
__device__ __forceinline__ void or_bits(uint32_t* obuf, uint32_t q, uint64_t bits, uint32_t len) {
  if (len == 0) return;
  const uint64_t top = bits << (64 - len);
  const uint32_t sh = q & 31, w = q >> 5;
  const uint64_t hi = top >> sh;
  const uint32_t w0 = (uint32_t)(hi >> 32), w1 = (uint32_t)hi;
  const uint32_t w2 = sh ? (uint32_t)((top << (64 - sh)) >> 32) : 0u;
  if (w0) atomicOr(&obuf[w], w0);
  if (w1) atomicOr(&obuf[w + 1], w1);
  if (w2) atomicOr(&obuf[w + 2], w2);
}

// ---- 3: the segment's bit string, built in LDS, into the frame's scan
__global__ __launch_bounds__(256) void huff_pack_kernel(const Plan P, const int16_t* __restrict__ coef_all) {
  __shared__ uint32_t lut[512 + 32];
  __shared__ uint32_t obuf[OBUF_WORDS + 2];  // + 2: or_bits names up to two words past a code's first
  __shared__ uint32_t bstart[SEG];
  __shared__ int sblk[SEG], sprev[SEG];
  __shared__ uint32_t tmp[4];
  const int f = blockIdx.x / P.nseg, seg = blockIdx.x - f * P.nseg;
  if (P.info[f].bad) return;  // uniform: a refused frame writes nothing
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int s0 = seg * SEG, nb = min(SEG, P.S - s0);
  const uint32_t start = P.seg_off[blockIdx.x], sbits = P.seg_bits[blockIdx.x] & ~BAD;
  const uint32_t pad = seg == P.nseg - 1 ? (0u - (start + sbits)) & 7u : 0u;  // the frame's last byte is filled with 1s
  const uint32_t end = start + sbits + pad;
  const uint32_t word0 = start >> 5;
  const uint32_t nwords = min(((end + 31) >> 5) - word0, (uint32_t)OBUF_WORDS);
  load_lut(lut);
  resolve_segment(P.L, s0, nb, sblk, sprev);
  for (uint32_t i = tid; i < nwords + 2; i += 256) obuf[i] = 0;
  uint32_t total;
  const uint32_t mine = tid < nb ? P.blk_bits[(size_t)f * P.S + s0 + tid] : 0u;
  const uint32_t excl = block_excl_scan(mine, tmp, &total);
  if (tid < SEG) bstart[tid] = excl;
  __syncthreads();
  if (total != sbits) return;  // cannot happen: steps 1 and 3 count with the same function (keeps every OR in obuf)
  const int zz = d_header.zigzag[lane];
  const int16_t* coef = coef_all + (size_t)f * P.S * 64;
  for (int i = wave; i < nb; i += 4) {
    const int blk = sblk[i], prev = sprev[i], tbl = blk >= P.L.off[1] ? 1 : 0;
    bool bad;
    const LaneCode c = code_lane(coef, blk, prev, tbl, lane, zz, lut, &bad);
    const uint32_t incl = wave_incl_scan(c.len, lane);
    const uint32_t blk_total = __shfl(incl, 63);
    // a block whose bits differ from the recorded count (cannot happen) is dropped rather than written elsewhere
    if (blk_total == (i + 1 < nb ? bstart[i + 1] : sbits) - bstart[i])
      or_bits(obuf, (start & 31) + bstart[i] + incl - c.len, c.bits, c.len);
  }
  if (tid == 0 && pad) or_bits(obuf, (start & 31) + sbits, (1u << pad) - 1u, pad);
  __syncthreads();
  uint32_t* scan = P.scan + (size_t)f * P.pitch_words;
  for (uint32_t i = tid; i < nwords; i += 256) {
    const uint32_t gw = word0 + i;
    if (gw >= P.pitch_words) break;
    const uint32_t v = __builtin_bswap32(obuf[i]);  // stream order: the first bit is the first byte's MSB
    const bool whole = gw * 32 >= start && gw * 32 + 32 <= end;
    if (whole)
      scan[gw] = v;
    else if (v)
      atomicOr(&scan[gw], v);  // shared with a neighbouring segment; cleared by step 2
  }
}

// The FF bytes among the 16 scan bytes at `byte0` (a multiple of 16) that lie below scan_bytes; *w: the bytes.
__device__ __forceinline__ uint32_t load_count_ff(const uint32_t* scan, uint32_t byte0, uint32_t scan_bytes, uint4* w) {
  *w = make_uint4(0, 0, 0, 0);
  if (byte0 >= scan_bytes) return 0;
  *w = *reinterpret_cast<const uint4*>(scan + (byte0 >> 2));
  const uint32_t ww[4] = {w->x, w->y, w->z, w->w};
  uint32_t n = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k)
    n += (byte0 + k < scan_bytes && ((ww[k >> 2] >> (8 * (k & 3))) & 255u) == 255u) ? 1u : 0u;
  return n;
}

// ---- 4: FF bytes per chunk
__global__ __launch_bounds__(256) void huff_ff_count_kernel(const Plan P) {
  __shared__ uint32_t tmp[4];
  const int f = blockIdx.x / P.nchunk, c = blockIdx.x - f * P.nchunk;
  const FrameInfo I = P.info[f];
  if (I.bad || (uint32_t)c * CHUNK >= I.scan_bytes) return;
  uint4 w;
  const uint32_t n = load_count_ff(P.scan + (size_t)f * P.pitch_words, (uint32_t)c * CHUNK + threadIdx.x * 16,
                                   I.scan_bytes, &w);
  uint32_t total;
  block_excl_scan(n, tmp, &total);
  if (threadIdx.x == 0) P.chunk_ff[blockIdx.x] = total;
}

// ---- 5: FF bytes before each chunk; the file sizes
__global__ __launch_bounds__(256) void huff_ff_scan_kernel(const Plan P, int64_t* __restrict__ sizes,
                                                          int32_t* __restrict__ status) {
  __shared__ uint32_t tmp[4];
  const int f = blockIdx.x, tid = threadIdx.x;
  const FrameInfo I = P.info[f];
  if (I.bad) {
    if (tid == 0) {
      sizes[f] = 0;
      status[f] = VGE_JPEG_ERR_ARG;
    }
    return;
  }
  const int nch = min((int)((I.scan_bytes + CHUNK - 1) / CHUNK), P.nchunk);
  uint32_t carry = 0;
  for (int base = 0; base < nch; base += 256) {
    const int idx = base + tid;
    const uint32_t v = idx < nch ? P.chunk_ff[(size_t)f * P.nchunk + idx] : 0u;
    uint32_t total;
    const uint32_t off = carry + block_excl_scan(v, tmp, &total);
    if (idx < nch) P.chunk_off[(size_t)f * P.nchunk + idx] = off;
    carry += total;
  }
  if (tid == 0) {
    P.info[f].ff_total = carry;
    sizes[f] = (int64_t)HDR + I.scan_bytes + carry + 2;
    status[f] = VGE_JPEG_OK;
  }
}

// ---- 6: the files
__global__ __launch_bounds__(256) void huff_emit_kernel(const Plan P, const uint16_t* __restrict__ qtab,
                                                       const int64_t* __restrict__ offsets, uint8_t* __restrict__ out,
                                                       int64_t out_bytes) {
  __shared__ uint32_t tmp[4];
  __shared__ uint8_t sbuf[2 * CHUNK];
  const int f = blockIdx.x / P.nchunk, c = blockIdx.x - f * P.nchunk, tid = threadIdx.x;
  const FrameInfo I = P.info[f];
  if (I.bad || (uint32_t)c * CHUNK >= I.scan_bytes) return;
  const int64_t size = (int64_t)HDR + I.scan_bytes + I.ff_total + 2, off = offsets[f];
  if (off < 0 || off > out_bytes || size > out_bytes - off) return;  // the file does not lie inside out: not written
  uint8_t* file = out + off;
  const uint32_t byte0 = (uint32_t)c * CHUNK + tid * 16;
  uint4 w;
  const uint32_t n = load_count_ff(P.scan + (size_t)f * P.pitch_words, byte0, I.scan_bytes, &w);
  uint32_t total_ff;
  uint32_t o = tid * 16 + block_excl_scan(n, tmp, &total_ff);
  const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint32_t b = (ww[k >> 2] >> (8 * (k & 3))) & 255u;
    if (byte0 + k < I.scan_bytes) {
      sbuf[o++] = (uint8_t)b;
      if (b == 255u) sbuf[o++] = 0;
    }
  }
  __syncthreads();
  const uint32_t valid = min((uint32_t)CHUNK, I.scan_bytes - (uint32_t)c * CHUNK);
  const uint32_t len = min(valid + total_ff, (uint32_t)(2 * CHUNK));
  uint8_t* dst = file + HDR + (size_t)c * CHUNK + P.chunk_off[blockIdx.x];
  for (uint32_t i = tid; i < len; i += 256) dst[i] = sbuf[i];
  if (c == 0) {
    for (int i = tid; i < HDR; i += 256) {
      uint8_t b = d_header.b[i];
      if (i >= DQT0 + 5 && i < DQT0 + 69)
        b = (uint8_t)qtab[d_header.zigzag[i - DQT0 - 5]];
      else if (i >= DQT0 + 69 + 5 && i < SOF)
        b = (uint8_t)qtab[64 + d_header.zigzag[i - DQT0 - 69 - 5]];
      else if (i == SOF + 5)
        b = (uint8_t)(P.L.height >> 8);
      else if (i == SOF + 6)
        b = (uint8_t)(P.L.height & 255);
      else if (i == SOF + 7)
        b = (uint8_t)(P.L.width >> 8);
      else if (i == SOF + 8)
        b = (uint8_t)(P.L.width & 255);
      else if (i == SOF + 11)
        b = (uint8_t)((P.L.h0 << 4) | P.L.v0);
      file[i] = b;
    }
    if (tid == 0) {
      file[size - 2] = 0xFF;
      file[size - 1] = 0xD9;
    }
  }
}

int launch_error(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return VGE_JPEG_OK;
  set_last_error(std::string(what) + ": " + hipGetErrorString(e));
  return VGE_JPEG_ERR_HIP;
}

bool grid_ok(const Plan& P) {
  return (long long)P.n_frames * P.nseg <= 0x7fffffffLL && (long long)P.n_frames * P.nchunk <= 0x7fffffffLL;
}

}  // namespace

extern "C" int vge_jpeg_entropy_segment_blocks(void) { return SEG; }

extern "C" size_t vge_jpeg_entropy_workspace_bytes(const vge_jpeg_layout* layout, int n_frames) {
  Plan P;
  int err;
  if (!make_plan(layout, n_frames, nullptr, P, &err)) return 0;
  return P.bytes;
}

extern "C" int vge_jpeg_entropy_plan(const int16_t* coef, const vge_jpeg_layout* layout, int n_frames, void* workspace,
                                     int64_t* sizes, int32_t* status, void* stream) {
  Plan P;
  int err;
  if (!make_plan(layout, n_frames, workspace, P, &err)) {
    set_last_error(err == VGE_JPEG_ERR_COMPONENTS
                       ? "vge_jpeg_entropy_plan: only 3-component (RGB) frames are encoded"
                       : "vge_jpeg_entropy_plan: bad argument (layout not from vge_jpeg_make_layout, or too large)");
    return err;
  }
  if (n_frames == 0) return VGE_JPEG_OK;
  if (!coef || !workspace || !sizes || !status || ((uintptr_t)workspace & 15) || ((uintptr_t)coef & 1) ||
      ((uintptr_t)sizes & 7) || ((uintptr_t)status & 3) || !grid_ok(P)) {
    set_last_error("vge_jpeg_entropy_plan: bad argument (null or misaligned buffer, or too many frames for one launch)");
    return VGE_JPEG_ERR_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned n = (unsigned)n_frames;
  hipLaunchKernelGGL(huff_count_kernel, dim3(n * P.nseg), dim3(256), 0, s, P, coef);
  hipLaunchKernelGGL(huff_seg_scan_kernel, dim3(n), dim3(256), 0, s, P);
  hipLaunchKernelGGL(huff_pack_kernel, dim3(n * P.nseg), dim3(256), 0, s, P, coef);
  hipLaunchKernelGGL(huff_ff_count_kernel, dim3(n * P.nchunk), dim3(256), 0, s, P);
  hipLaunchKernelGGL(huff_ff_scan_kernel, dim3(n), dim3(256), 0, s, P, sizes, status);
  return launch_error("vge_jpeg_entropy_plan");
}

extern "C" int vge_jpeg_entropy_emit(const void* workspace, const uint16_t* qtab, const vge_jpeg_layout* layout,
                                     int n_frames, const int64_t* offsets, uint8_t* out, int64_t out_bytes,
                                     void* stream) {
  Plan P;
  int err;
  if (!make_plan(layout, n_frames, const_cast<void*>(workspace), P, &err)) {
    set_last_error(err == VGE_JPEG_ERR_COMPONENTS
                       ? "vge_jpeg_entropy_emit: only 3-component (RGB) frames are encoded"
                       : "vge_jpeg_entropy_emit: bad argument (layout not from vge_jpeg_make_layout, or too large)");
    return err;
  }
  if (out_bytes < 0) {
    set_last_error("vge_jpeg_entropy_emit: bad argument (negative out_bytes)");
    return VGE_JPEG_ERR_ARG;
  }
  if (n_frames == 0) return VGE_JPEG_OK;
  if (!workspace || !qtab || !offsets || !out || ((uintptr_t)workspace & 15) || ((uintptr_t)qtab & 1) ||
      ((uintptr_t)offsets & 7) || !grid_ok(P)) {
    set_last_error("vge_jpeg_entropy_emit: bad argument (null or misaligned buffer, or too many frames for one launch)");
    return VGE_JPEG_ERR_ARG;
  }
  hipLaunchKernelGGL(huff_emit_kernel, dim3((unsigned)n_frames * P.nchunk), dim3(256), 0,
                     static_cast<hipStream_t>(stream), P, qtab, offsets, out, out_bytes);
  return launch_error("vge_jpeg_entropy_emit");
}
