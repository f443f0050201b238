// Device entropy decoder (include/vge_frames.h): raw baseline JPEG files in device memory -> the int16 coefficients and
// uint16 quantisation tables vge_jpeg_reconstruct consumes, bit for bit what the host decoder (vge_jpeg.cpp) gives.
// Huffman DEcoding is serial -- a symbol's position is known only once its predecessor is decoded -- and is made
// parallel by self-synchronisation (Weissenberger & Schmidt): a decoder started at a wrong bit falls into
// step with the true symbol sequence after a few symbols, so every lane decodes one SUBSEQUENCE (SUB scan bytes) from
// a guessed state, the guesses are repaired by carrying exit states forward, and a second pass writes from the states
// that have become true.  No workgroup ever waits for another: the phases are separate launches ordered by the stream.
//
//   1 dehuff_place     one workgroup: checks every (offset, size) against the data buffer and gives each frame its
//                      place in the workspace's scan copy (a 64-bit exclusive scan of the sizes).
//   2 dehuff_header    a wave per frame, lane 0 walks the markers with the host's parser (vge_jpeg_header.h): status,
//                      restart interval, scan start, table selectors, the decode tables; writes qtab.
//   3 dehuff_prepare   a workgroup per frame over the scan bytes, 16 per lane: classifies every byte (data, the stuffed 00
//                      after an FF, a terminator = FF followed by anything but 00 or ending the file, the byte after a
//                      terminator), block scans of the data and terminator counts place the data bytes in the frame's
//                      unstuffed scan copy and record where terminator t ends restart interval t and which marker it is.
//   4 dehuff_decode    a workgroup per (frame, restart-interval group) passes over an interval in TILES of TILE_LANES
//                      subsequences: speculative decode, synchronisation rounds (in LDS, barriers only), an exclusive
//                      scan of the blocks completed, the write pass, then the interval's DC prefix sums and checks.
//   5 dehuff_finalise  a workgroup per frame: a frame with any failed interval gets VGE_JPEG_ERR_IO; a failed frame's
//                      coefficients are zeroed and its tables set to 1; status[] and rounds[].
// Termination.  Every loop is bounded by sizes: the header walk by the file's bytes (each pass consumes one), a table
// build by a DHT's 256 values, prepare by the scan bytes, a lane's decode of one subsequence by its 8 * SUB bits (each
// symbol consumes at least one), the synchronisation rounds of a tile by the tile's subsequence count (lane 0 starts
// from the true state and after that many rounds has rewritten every record itself), the tiles by the interval's
// bytes.  A stream never fails to "converge": in the worst case lane 0 decodes the whole tile serially.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <string>

#include "../../include/vge_frames.h"
#include "vge_error.h"
#include "vge_jpeg_header.h"

using vge::set_last_error;
using vge_jpeg::Header;
using vge_jpeg::Huff;

namespace {

constexpr int SUB = 32;                 // scan bytes one lane starts on (vge_jpeg_entropy_decode_subsequence_bytes)
constexpr uint32_t SUB_BITS = SUB * 8;
constexpr int TILE_LANES = 256;         // subsequences per pass = lanes of the workgroup
constexpr int PREP_BYTES = 16;          // scan bytes per lane and pass in dehuff_prepare
constexpr int GROUPS_MAX = 16;          // workgroups that share a frame's restart intervals
constexpr int BLOCK_BITS_MAX = 1658;
constexpr int64_t FILE_BYTES_MAX = (1ll << 28) - 1;  // bit positions are 32-bit
constexpr uint32_t INVALID = 0xffffffffu;            // a state's bit position: the guess (or the stream) ended here
constexpr int HUFF_WORDS = (int)(sizeof(Huff) / 4);
constexpr int TILE_WORDS = TILE_LANES * SUB / 4 + 4;  // a tile's dwords in LDS: + 1 unaligned start, + 3 lookahead

struct FrameRec {
  int32_t status;
  uint32_t n_int;       // restart intervals of the scan
  uint32_t n_terms;     // terminators found in the scan bytes
  uint32_t total_data;  // unstuffed data bytes in the scan copy
  uint32_t rounds;      // the most rounds any tile needed
  uint32_t pad;
  uint64_t scan_off;    // the frame's place in the scan copy, a multiple of 16
};

struct DPlan {
  vge_jpeg_layout L;
  int n_frames, n_mcu, groups;
  int64_t data_bytes;
  uint64_t scan_cap;   // bytes of the scan copy
  Header* hdr;         // [n]
  FrameRec* rec;       // [n]
  uint32_t* seg_end;   // [n][n_mcu]  data bytes of the frame before terminator t
  uint32_t* mark;      // [n][n_mcu]  the byte after terminator t (0x100: none, the file ends)
  uint32_t* ivl_err;   // [n][n_mcu]
  uint8_t* scan;       // [scan_cap]
  size_t bytes;
};

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

bool make_plan(const vge_jpeg_layout* layout, int n_frames, int64_t data_bytes, void* workspace, DPlan& P) {
  vge_jpeg_layout want;
  if (n_frames < 0 || data_bytes < 0 || !layout ||
      vge_jpeg_make_layout(layout->width, layout->height, layout->n_comp, layout->h0, layout->v0, &want) != VGE_JPEG_OK ||
      memcmp(&want, layout, sizeof(want)) != 0)
    return false;
  if ((long long)want.blocks_per_frame * BLOCK_BITS_MAX + 7 >= 0x7fffffffLL) return false;
  P.L = want;
  P.n_frames = n_frames;
  P.n_mcu = want.mcus_x * want.mcus_y;
  P.groups = P.n_mcu < GROUPS_MAX ? P.n_mcu : GROUPS_MAX;
  P.data_bytes = data_bytes;
  const size_t n = (size_t)n_frames;
  P.scan_cap = align16((size_t)data_bytes) + 32 * n;
  const uintptr_t base = reinterpret_cast<uintptr_t>(workspace);  // null when only the size is asked for
  size_t o = 0;
  auto carve = [&](size_t bytes) {
    void* q = reinterpret_cast<void*>(base + o);
    o += align16(bytes);
    return q;
  };
  P.hdr = static_cast<Header*>(carve(n * sizeof(Header)));
  P.rec = static_cast<FrameRec*>(carve(n * sizeof(FrameRec)));
  P.seg_end = static_cast<uint32_t*>(carve(n * P.n_mcu * 4));
  P.mark = static_cast<uint32_t*>(carve(n * P.n_mcu * 4));
  P.ivl_err = static_cast<uint32_t*>(carve(n * P.n_mcu * 4));
  P.scan = static_cast<uint8_t*>(carve(P.scan_cap));
  P.bytes = o;
  return true;
}

// ---- wave and workgroup scans (256 threads)
template <class T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

// Exclusive prefix of v over the workgroup and the workgroup's total; tmp: 4 elements of LDS.  Ends on a barrier that
// makes tmp reusable.
template <class T>
__device__ __forceinline__ T block_excl_scan(T v, T* tmp, T* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T incl = wave_incl_scan(v, lane);
  if (lane == 63) tmp[wave] = incl;
  __syncthreads();
  const T t0 = tmp[0], t1 = tmp[1], t2 = tmp[2], t3 = tmp[3];
  __syncthreads();
  *total = t0 + t1 + t2 + t3;
  return incl - v + (wave > 0 ? t0 : (T)0) + (wave > 1 ? t1 : (T)0) + (wave > 2 ? t2 : (T)0);
}

// ---- 1: argument checks and the frames' places in the scan copy
__global__ __launch_bounds__(256) void dehuff_place_kernel(const DPlan P, const int64_t* __restrict__ offsets,
                                                          const int64_t* __restrict__ sizes) {
  __shared__ unsigned long long tmp[4];
  unsigned long long carry = 0;
  for (int base = 0; base < P.n_frames; base += 256) {
    const int i = base + (int)threadIdx.x;
    bool ok = false;
    unsigned long long want = 0;
    if (i < P.n_frames) {
      const int64_t off = offsets[i], size = sizes[i];
      ok = off >= 0 && size >= 0 && size <= FILE_BYTES_MAX && off <= P.data_bytes && size <= P.data_bytes - off;
      if (ok) want = (((unsigned long long)size + 15ull) & ~15ull) + 16ull;
    }
    unsigned long long total;
    const unsigned long long at = carry + block_excl_scan(want, tmp, &total);
    if (i < P.n_frames) {
      if (ok && at + want > P.scan_cap) ok = false;  // the sizes add up to more than the workspace was sized for
      FrameRec R;
      R.status = ok ? VGE_JPEG_OK : VGE_JPEG_ERR_ARG;
      R.n_int = R.n_terms = R.total_data = R.rounds = R.pad = 0;
      R.scan_off = ok ? at : 0ull;
      P.rec[i] = R;
    }
    carry += total;
  }
}

// ---- 2: headers
__global__ __launch_bounds__(64) void dehuff_header_kernel(const DPlan P, const uint8_t* __restrict__ data,
                                                          const int64_t* __restrict__ offsets,
                                                          const int64_t* __restrict__ sizes,
                                                          uint16_t* __restrict__ qtab_all) {
  const int f = blockIdx.x;
  if (threadIdx.x != 0) return;
  int st = P.rec[f].status;
  if (st != VGE_JPEG_OK) return;  // outside the buffer: nothing of it is read
  Header& H = P.hdr[f];
  vge_jpeg::header_init(H);
  st = vge_jpeg::parse_header(data + offsets[f], (size_t)sizes[f], H);
  if (st == VGE_JPEG_OK && !vge_jpeg::same_shape(H, P.L)) st = VGE_JPEG_ERR_SHAPE;
  P.rec[f].status = st;
  if (st != VGE_JPEG_OK) return;
  const uint32_t restart = (uint32_t)H.restart;
  P.rec[f].n_int = restart > 0 ? ((uint32_t)P.n_mcu + restart - 1) / restart : 1u;
  uint16_t* q = qtab_all + (size_t)f * 192;
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < 64; ++k) q[64 * c + k] = c < H.n_comp ? H.q[H.tq[c]][k] : (uint16_t)1;
}

// ---- 3: the unstuffed scan copy and the restart intervals
__global__ __launch_bounds__(256) void dehuff_prepare_kernel(const DPlan P, const uint8_t* __restrict__ data,
                                                           const int64_t* __restrict__ offsets,
                                                           const int64_t* __restrict__ sizes) {
  __shared__ uint32_t tmp[4];
  const int f = blockIdx.x, tid = threadIdx.x;
  const FrameRec R = P.rec[f];
  if (R.status != VGE_JPEG_OK) return;
  const uint8_t* p = data + offsets[f];
  const uint32_t size = (uint32_t)sizes[f], scan = P.hdr[f].scan;  // scan <= size: the parser's check
  uint8_t* out = P.scan + R.scan_off;
  uint32_t* seg_end = P.seg_end + (size_t)f * P.n_mcu;
  uint32_t* mark = P.mark + (size_t)f * P.n_mcu;
  uint32_t data_before = 0, terms_before = 0;
  for (uint32_t c0 = scan; c0 < size; c0 += 256 * PREP_BYTES) {  // size < 2^28: no wrap
    const uint32_t x0 = c0 + (uint32_t)tid * PREP_BYTES;
    // byte x is dropped when it follows an FF (a stuffed 00, or the byte that makes the FF a terminator), a terminator
    // when it is an FF not followed by 00, data otherwise.  The host's reader never skips an FF, so the rule is local;
    // it differs from a serial walk only behind a terminator that is not a restart marker, where the frame has
    // failed or the rest of the file is ignored.
    uint32_t prev = (x0 > scan && x0 <= size) ? p[x0 - 1] : 0u;
    uint32_t cur = x0 < size ? p[x0] : 0u;
    uint32_t is_data = 0, is_term = 0, nd = 0, nt = 0;
    uint32_t w[PREP_BYTES / 4] = {0, 0, 0, 0};
    uint32_t after[PREP_BYTES];
#pragma unroll
    for (int k = 0; k < PREP_BYTES; ++k) {
      const uint32_t x = x0 + k;
      const uint32_t nxt = x + 1 < size ? p[x + 1] : 0x100u;
      after[k] = nxt;
      if (x < size) {
        const bool drop = x > scan && prev == 0xFFu;
        const bool term = !drop && cur == 0xFFu && nxt != 0u;
        if (term) {
          is_term |= 1u << k;
          ++nt;
        } else if (!drop) {
          is_data |= 1u << k;
          ++nd;
        }
        w[k >> 2] |= cur << (8 * (k & 3));
      }
      prev = cur;
      cur = nxt & 0xFFu;
    }
    uint32_t total_d, total_t;
    uint32_t o = data_before + block_excl_scan(nd, tmp, &total_d);
    uint32_t t = terms_before + block_excl_scan(nt, tmp, &total_t);
#pragma unroll
    for (int k = 0; k < PREP_BYTES; ++k) {
      if (is_data & (1u << k)) out[o++] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
      if (is_term & (1u << k)) {
        if (t < (uint32_t)P.n_mcu) {
          seg_end[t] = o;
          mark[t] = after[k];
        }
        ++t;
      }
    }
    data_before += total_d;
    terms_before += total_t;
  }
  if (tid == 0) {
    P.rec[f].n_terms = terms_before;
    P.rec[f].total_data = data_before;
  }
}

// ---- 4: decode
struct State {
  uint32_t p;   // bit position in the frame's scan copy; INVALID: ended
  uint32_t ck;  // block phase inside the MCU << 8 | zigzag index
};

// The bit reader of the decode loops.  The tile's bytes are staged in LDS as big-endian dwords (first bit = MSB), so a
// symbol costs one two-dword LDS read: the 32 bits at p hold a whole code (<= 16 bits) and its extra bits (<= 15).
struct Reader {
  const uint32_t* w;  // LDS: the tile's dwords, byte-swapped
  uint32_t word0;     // the scan copy's dword that w[0] holds
  __device__ __forceinline__ uint32_t window(uint32_t p) const {
    const uint32_t i = (p >> 5) - word0;
    const uint64_t two = ((uint64_t)w[i] << 32) | w[i + 1];
    return (uint32_t)(two >> (32u - (p & 31u)));
  }
};

// decode_sym of the host on the 32 bits at the read position, the table in LDS.  *len: the code's length; -1: no such
// code.
__device__ __forceinline__ int decode_sym(uint32_t win, const Huff* h, int* len) {
  const uint32_t look = win >> 23;
  int l = h->look_len[look];
  const int quick = h->look_sym[look];
  *len = l;
  if (l) return quick;
  const uint32_t c16 = win >> 16;
  for (l = 10; l <= 16; ++l) {
    const int32_t code = (int32_t)(c16 >> (16 - l));
    if (code <= h->maxcode[l]) {
      *len = l;
      const int idx = code + h->valoff[l];
      return (idx >= 0 && idx < 256) ? h->vals[idx] : -1;
    }
  }
  return -1;
}

// receive_extend of the host: the s bits (1 <= s <= 15) behind a code of `len` bits.
__device__ __forceinline__ int receive_extend(uint32_t win, int len, int s) {
  const int v = (int)((win << len) >> (32 - s));
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// Luma block j of MCU m -> its index in the frame's coefficient buffer.
__device__ __forceinline__ int luma_block(const vge_jpeg_layout& L, int m, int j) {
  const int my = m / L.mcus_x, mx = m - my * L.mcus_x;
  const int v = j / L.h0, h = j - v * L.h0;
  return L.off[0] + (my * L.v0 + v) * L.bw[0] + mx * L.h0 + h;
}

struct Shape {
  int nl, B;  // luma blocks per MCU, blocks per MCU
};
__device__ __forceinline__ int comp_of(const Shape& S, int phase) { return phase < S.nl ? 0 : phase - S.nl + 1; }

// What the write pass needs beyond the state.
struct Writer {
  int16_t* coef;          // the frame's coefficients
  const uint8_t* zz;      // LDS
  int mcu0;               // the interval's first MCU
  uint32_t blk, need;     // scan blocks of the interval before the one in progress; the interval's block count
  uint32_t* err;          // LDS
  uint32_t* pfinal;       // LDS: the bit position at which block need - 1 ended
};

// Decodes symbols from s until the bit position reaches bnd; returns the blocks completed.  Speculative (WRITE false):
// an impossible symbol ends the guess (s.p = INVALID).  WRITE: stores the coefficients (DC differences in slot 0),
// raises *err on an impossible symbol and stops after block need - 1.
template <bool WRITE>
__device__ __forceinline__ uint32_t run(const Reader& r, const Huff* tabs, const vge_jpeg_layout& L, const Shape S, State& s,
                                        uint32_t bnd, Writer* wr) {
  uint32_t p = s.p, n = 0;
  int phase = (int)(s.ck >> 8), k = (int)(s.ck & 255u);
  int16_t* dst = nullptr;
  auto locate = [&]() {
    if (WRITE) {
      const int m = wr->mcu0 + (int)(wr->blk / (uint32_t)S.B);
      const int c = comp_of(S, phase);
      dst = wr->coef + (size_t)(c == 0 ? luma_block(L, m, phase) : L.off[c] + m) * 64;
    }
  };
  locate();
  bool bad = false;
  while (p < bnd) {  // every pass consumes at least one bit or ends the loop
    // one path for DC and AC symbols: lanes of a wave are in both states at once
    const bool dc = k == 0;
    const Huff* h = tabs + 2 * comp_of(S, phase) + (dc ? 0 : 1);
    const uint32_t win = r.window(p);
    int len;
    const int sym = decode_sym(win, h, &len);
    if (sym < 0 || (dc && sym > 11)) {
      bad = true;
      break;
    }
    const int sz = dc ? sym : (sym & 15), run_len = dc ? 0 : (sym >> 4);
    const int v = sz ? receive_extend(win, len, sz) : 0;
    p += (uint32_t)(len + sz);
    bool done = false;
    if (dc) {
      if (WRITE && v) dst[0] = (int16_t)v;
      k = 1;
    } else if (sz == 0) {
      k += 16;                            // ZRL; an EOB (run_len != 15) ends the block like an index past 63 does
      done = run_len != 15 || k >= 64;
    } else {
      k += run_len;
      if (k > 63) {
        bad = true;
        break;
      }
      if (WRITE) dst[wr->zz[k]] = (int16_t)v;
      done = ++k >= 64;
    }
    if (done) {
      k = 0;
      phase = phase + 1 == S.B ? 0 : phase + 1;
      ++n;
      if (WRITE) {
        if (++wr->blk == wr->need) {
          *wr->pfinal = p;
          break;
        }
        locate();
      }
    }
  }
  if (bad) {
    if (WRITE) atomicOr(wr->err, 1u);
    p = INVALID;
  }
  s.p = p;
  s.ck = ((uint32_t)phase << 8) | (uint32_t)k;
  return n;
}

__global__ __launch_bounds__(256) void dehuff_decode_kernel(const DPlan P, int16_t* __restrict__ coef_all,
                                                          const uint16_t* __restrict__ qtab_all) {
  __shared__ uint32_t tabs_w[6 * HUFF_WORDS];
  __shared__ uint32_t rec_p[TILE_LANES], rec_ck[TILE_LANES], rec_n[TILE_LANES];
  __shared__ uint32_t tile_w[TILE_WORDS];
  __shared__ uint32_t tmp[4];
  __shared__ uint32_t sh_err, sh_pfinal;
  __shared__ uint16_t sq[192];
  __shared__ uint8_t zz[64];
  // group-major: consecutive workgroups go to different XCDs, and a frame without restart markers has work for its
  // group 0 only -- frame-major order would put all of those on one XCD
  const int g = blockIdx.x / P.n_frames, f = blockIdx.x - g * P.n_frames, tid = threadIdx.x;
  const FrameRec R = P.rec[f];
  if (R.status != VGE_JPEG_OK || (uint32_t)g >= R.n_int) return;  // uniform
  const Header& H = P.hdr[f];
  const vge_jpeg_layout& L = P.L;
  Shape S;
  S.nl = L.n_comp == 1 ? 1 : L.h0 * L.v0;
  S.B = L.n_comp == 1 ? 1 : S.nl + 2;
  for (int c = 0; c < L.n_comp; ++c) {  // component c's DC table at 2c, its AC table at 2c + 1
    const uint32_t* sd = reinterpret_cast<const uint32_t*>(&H.dc[H.td[c]]);
    const uint32_t* sa = reinterpret_cast<const uint32_t*>(&H.ac[H.ta[c]]);
    for (int i = tid; i < HUFF_WORDS; i += 256) {
      tabs_w[(2 * c) * HUFF_WORDS + i] = sd[i];
      tabs_w[(2 * c + 1) * HUFF_WORDS + i] = sa[i];
    }
  }
  if (tid < 192) sq[tid] = qtab_all[(size_t)f * 192 + tid];
  if (tid < 64) zz[tid] = (uint8_t)vge_jpeg::zigzag_at(tid);
  __syncthreads();
  const Huff* tabs = reinterpret_cast<const Huff*>(tabs_w);
  const uint32_t* scan_w = reinterpret_cast<const uint32_t*>(P.scan + R.scan_off);  // aligned dwords
  Reader rd;
  rd.w = tile_w;
  int16_t* coef = coef_all + (size_t)f * L.blocks_per_frame * 64;
  const uint32_t* seg_end = P.seg_end + (size_t)f * P.n_mcu;
  const uint32_t* mark = P.mark + (size_t)f * P.n_mcu;
  const uint32_t restart = H.restart > 0 ? (uint32_t)H.restart : (uint32_t)P.n_mcu;
  uint32_t rounds_max = 0;
  for (uint32_t j = (uint32_t)g; j < R.n_int; j += (uint32_t)P.groups) {
    // the interval's bytes in the scan copy: it starts after terminator j - 1, which must be the RSTn that is due
    bool ok = true;
    uint32_t b0 = 0, b1 = 0;
    if (j > 0) {
      ok = j - 1 < R.n_terms && mark[j - 1] == 0xD0u + ((j - 1) & 7u);
      if (ok) b0 = seg_end[j - 1];
    }
    if (ok) b1 = j < R.n_terms ? seg_end[j] : R.total_data;
    const uint32_t mcu0 = j * restart, nm = min(restart, (uint32_t)P.n_mcu - mcu0);
    const uint32_t need = nm * (uint32_t)S.B;
    const uint32_t bit0 = b0 * 8u, end = b1 * 8u;
    const uint32_t ns = (b1 - b0 + SUB - 1) / SUB;
    if (tid == 0) {
      sh_err = ok ? 0u : 1u;
      sh_pfinal = INVALID;
    }
    __syncthreads();
    State entry{bit0, 0u};
    uint32_t base = 0;
    for (uint32_t t0 = 0; ok && t0 < ns; t0 += TILE_LANES) {
      const uint32_t na = min((uint32_t)TILE_LANES, ns - t0);
      const bool active = (uint32_t)tid < na;
      const uint32_t start = bit0 + (t0 + (uint32_t)tid) * SUB_BITS;
      State s = tid == 0 ? entry : State{start, 0u};
      // the tile's dwords into LDS: from the one its first bit lies in to three past its last subsequence (a symbol
      // overhangs a boundary by at most 31 bits and the reader looks one dword ahead); inside the frame's scan copy,
      // which is 16 bytes longer than the file
      rd.word0 = (bit0 + t0 * SUB_BITS) >> 5;
      for (uint32_t i = (uint32_t)tid; i < na * (SUB / 4) + 4; i += 256) tile_w[i] = __builtin_bswap32(scan_w[rd.word0 + i]);
      __syncthreads();
      // round 1: every lane decodes its own subsequence from its guess (lane 0: from the true state)
      if (active) {
        const uint32_t n = run<false>(rd, tabs, L, S, s, min(start + SUB_BITS, end), nullptr);
        rec_p[tid] = s.p;
        rec_ck[tid] = s.ck;
        rec_n[tid] = n;
      }
      __syncthreads();
      // rounds 2 ..: lane i carries its exit state through subsequence i + r and rewrites that record; it stops when
      // the record already held the state it arrived with.  Bounded by the tile's subsequence count.
      bool alive = active;
      uint32_t r = 1;
      for (; r < na; ++r) {
        const uint32_t tgt = (uint32_t)tid + r;
        if (alive && tgt < na && s.p != INVALID) {
          const uint32_t n = run<false>(rd, tabs, L, S, s, min(bit0 + (t0 + tgt + 1u) * SUB_BITS, end), nullptr);
          const bool same = rec_p[tgt] == s.p && rec_ck[tgt] == s.ck;
          rec_p[tgt] = s.p;
          rec_ck[tgt] = s.ck;
          rec_n[tgt] = n;  // the count belongs to this lane's entry state, the truer one
          alive = !same;
        } else {
          alive = false;
        }
        if (!__syncthreads_or(alive)) {
          ++r;
          break;
        }
      }
      rounds_max = max(rounds_max, r);
      // placement and the write pass, each lane from the state that has become true
      uint32_t total;
      const uint32_t excl = block_excl_scan(active ? rec_n[tid] : 0u, tmp, &total);
      if (active) {
        State e = tid == 0 ? entry : State{rec_p[tid - 1], rec_ck[tid - 1]};
        const uint32_t first = base + excl;
        if (e.p != INVALID && first < need) {
          Writer wr{coef, zz, (int)mcu0, first, need, &sh_err, &sh_pfinal};
          run<true>(rd, tabs, L, S, e, min(start + SUB_BITS, end), &wr);
        }
      }
      entry = State{rec_p[na - 1], rec_ck[na - 1]};
      base += total;
      __syncthreads();  // the records are read; the next tile may rewrite them, and the stores are visible below
      if (entry.p == INVALID || base >= need) break;
    }
    __syncthreads();
    const uint32_t pfinal = sh_pfinal;
    // the host's overrun(): the last MCU may not end past the interval's real bits; and where a marker is due the
    // interval must end inside its last byte (a whole surplus byte before the marker is refused)
    bool err = sh_err != 0u || pfinal == INVALID || pfinal > end || (j + 1 < R.n_int && end - pfinal >= 8u);
    // DC: per component an inclusive scan of the differences in scan order, the host's range check on every prefix,
    // then the per-block L1 bound with the final DC
    if (!err) {
      uint32_t bad = 0;
      for (int c = 0; c < L.n_comp; ++c) {
        const uint32_t per = c == 0 ? (uint32_t)S.nl : 1u, cnt = nm * per;
        uint32_t carry = 0;
        for (uint32_t e0 = 0; e0 < cnt; e0 += 256) {
          const uint32_t e = e0 + (uint32_t)tid;
          int16_t* blk = nullptr;
          uint32_t d = 0;
          if (e < cnt) {
            const int m = (int)(mcu0 + e / per);
            blk = coef + (size_t)(c == 0 ? luma_block(L, m, (int)(e % per)) : L.off[c] + m) * 64;
            d = (uint32_t)(int32_t)blk[0];
          }
          uint32_t total;
          const uint32_t excl = block_excl_scan(d, tmp, &total);
          if (e < cnt) {
            const int32_t pred = (int32_t)(carry + excl + d);
            if (pred < -32768 || pred > 32767) {
              bad = 1;
            } else {
              uint32_t l1 = (uint32_t)(pred < 0 ? -pred : pred) * sq[64 * c];
#pragma unroll 8
              for (int k = 1; k < 64; ++k) {
                const int val = blk[k];
                l1 += (uint32_t)(val < 0 ? -val : val) * sq[64 * c + k];
              }
              if (l1 > (uint32_t)VGE_JPEG_BLOCK_L1_MAX) bad = 1;
              blk[0] = (int16_t)pred;
            }
          }
          carry += total;
        }
      }
      err = __syncthreads_or(bad != 0u);
    }
    if (tid == 0) P.ivl_err[(size_t)f * P.n_mcu + j] = err ? 1u : 0u;
    __syncthreads();  // sh_err / sh_pfinal are reset by the next interval
  }
  if (tid == 0) atomicMax(&P.rec[f].rounds, rounds_max);
}

// ---- 5: per-frame status; a failed frame's buffers
__global__ __launch_bounds__(256) void dehuff_finalise_kernel(const DPlan P, int16_t* __restrict__ coef_all,
                                                            uint16_t* __restrict__ qtab_all,
                                                            int32_t* __restrict__ status,
                                                            int32_t* __restrict__ rounds) {
  const int f = blockIdx.x, tid = threadIdx.x;
  const FrameRec R = P.rec[f];
  int st = R.status;
  if (st == VGE_JPEG_OK) {
    uint32_t bad = 0;
    for (uint32_t j = (uint32_t)tid; j < R.n_int; j += 256) bad |= P.ivl_err[(size_t)f * P.n_mcu + j];
    if (__syncthreads_or(bad != 0u)) st = VGE_JPEG_ERR_IO;
  }
  if (st != VGE_JPEG_OK) {
    uint4* c = reinterpret_cast<uint4*>(coef_all + (size_t)f * P.L.blocks_per_frame * 64);
    for (int i = tid; i < P.L.blocks_per_frame * 8; i += 256) c[i] = make_uint4(0, 0, 0, 0);
    if (tid < 192) qtab_all[(size_t)f * 192 + tid] = 1;
  }
  if (tid == 0) {
    status[f] = st;
    if (rounds) rounds[f] = (int32_t)R.rounds;
  }
}

std::atomic<int> g_prepare_only{0};

}  // namespace

// For tools/bench_frames.py, which times the stages on device events: non-zero makes the decode call stop after scan
// preparation (steps 1 - 3; coef is cleared, status and rounds are not written).  Returns the previous value.
extern "C" int vge_debug_jpeg_dehuff_prepare_only(int on) { return g_prepare_only.exchange(on ? 1 : 0); }

extern "C" int vge_jpeg_entropy_decode_subsequence_bytes(void) { return SUB; }
extern "C" int vge_jpeg_entropy_decode_tile_bytes(void) { return SUB * TILE_LANES; }

extern "C" size_t vge_jpeg_entropy_decode_workspace_bytes(const vge_jpeg_layout* layout, int n_frames,
                                                          int64_t total_file_bytes) {
  DPlan P;
  if (!make_plan(layout, n_frames, total_file_bytes, nullptr, P)) return 0;
  return P.bytes;
}

extern "C" int vge_jpeg_entropy_decode_device(const uint8_t* data, int64_t data_bytes, const int64_t* offsets,
                                              const int64_t* sizes, int n_frames, const vge_jpeg_layout* layout,
                                              void* workspace, int16_t* coef, uint16_t* qtab, int32_t* status,
                                              int32_t* rounds, void* stream) {
  DPlan P;
  if (!make_plan(layout, n_frames, data_bytes, workspace, P)) {
    set_last_error("vge_jpeg_entropy_decode_device: bad argument (layout not from vge_jpeg_make_layout or too large, "
                   "negative count or size)");
    return VGE_JPEG_ERR_ARG;
  }
  if (n_frames == 0) return VGE_JPEG_OK;
  if (!data || !offsets || !sizes || !workspace || !coef || !qtab || !status || ((uintptr_t)workspace & 15) ||
      ((uintptr_t)coef & 15) || ((uintptr_t)qtab & 1) || ((uintptr_t)offsets & 7) || ((uintptr_t)sizes & 7) ||
      ((uintptr_t)status & 3) || ((uintptr_t)rounds & 3) || (long long)n_frames * P.groups > 0x7fffffffLL) {
    set_last_error("vge_jpeg_entropy_decode_device: bad argument (null or misaligned buffer, or too many frames for "
                   "one launch)");
    return VGE_JPEG_ERR_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned n = (unsigned)n_frames;
  if (hipMemsetAsync(coef, 0, (size_t)n * P.L.blocks_per_frame * 128, s) != hipSuccess) {
    set_last_error(std::string("vge_jpeg_entropy_decode_device: ") + hipGetErrorString(hipGetLastError()));
    return VGE_JPEG_ERR_HIP;
  }
  hipLaunchKernelGGL(dehuff_place_kernel, dim3(1), dim3(256), 0, s, P, offsets, sizes);
  hipLaunchKernelGGL(dehuff_header_kernel, dim3(n), dim3(64), 0, s, P, data, offsets, sizes, qtab);
  hipLaunchKernelGGL(dehuff_prepare_kernel, dim3(n), dim3(256), 0, s, P, data, offsets, sizes);
  if (g_prepare_only.load() == 0) {
    hipLaunchKernelGGL(dehuff_decode_kernel, dim3(n * (unsigned)P.groups), dim3(256), 0, s, P, coef, qtab);
    hipLaunchKernelGGL(dehuff_finalise_kernel, dim3(n), dim3(256), 0, s, P, coef, qtab, status, rounds);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_last_error(std::string("vge_jpeg_entropy_decode_device: ") + hipGetErrorString(e));
    return VGE_JPEG_ERR_HIP;
  }
  return VGE_JPEG_OK;
}
