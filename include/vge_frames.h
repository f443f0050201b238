/* vge_frames.h -- the frame front end: baseline-JPEG frame folders decoded to uint8 RGB on the device.
 *
 * The reference never hands its extractors frames straight from a video: extract_mesh.py:47-82,200-209 writes every
 * frame to frames/<action>/<video>/frame_%06d.jpg (cv2.imwrite, quality 95, 4:2:0) and reads the JPEGs back with
 * cv2.imread, so the pixels its models see have been through libjpeg's decoder (the "islow" integer IDCT, fancy
 * chroma upsampling, the 16-bit fixed-point YCbCr -> RGB).  This ABI reproduces those pixels exactly, split at the
 * host/device line:
 *   probe            headers only: size, component count, luma sampling factors
 *   entropy decode   marker parsing + Huffman decoding -> int16 coefficients (natural order) and the uint16
 *                    quantisation tables.  Host threads, one frame each, from paths or from files in memory, into
 *                    caller-provided (normally pinned) buffers; or the device, parallel inside a frame, from file
 *                    bytes in device memory into device buffers (vge_jpeg_entropy_decode_device, below)
 *   reconstruct      device (HIP, caller's stream) or host (plain C++): dequantise, IDCT, upsample, colour convert
 *                    -> uint8 [F, H, W, 3] RGB; grayscale is replicated to three channels (cv2.imread's default flag)
 * Both reconstructs share their arithmetic through one host/device header (csrc/vge_jpeg_math.h).
 *
 * Supported streams: 8-bit baseline (SOF0), Huffman coded, 1 or 3 components, luma sampling 1x1, 2x1 or 2x2 with
 * chroma 1x1 (4:4:4, 4:2:2, 4:2:0), restart intervals.  Everything else gets its own status below.  All frames of one
 * call share H x W and sampling (a video's frames do); a frame that differs from the layout gets the shape status.
 *
 * Every call returns VGE_JPEG_OK or the first failing frame's code; per-frame codes go to status[] / info[].status;
 * vge_last_error names the first failure.  No exceptions cross the ABI.  n_threads <= 0: vge_ingest_default_threads().
 */
#ifndef VGE_FRAMES_H
#define VGE_FRAMES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  VGE_JPEG_OK = 0,
  VGE_JPEG_ERR_ARG = 1,           /* bad argument */
  VGE_JPEG_ERR_HIP = 2,           /* a HIP call failed (device reconstruct) */
  VGE_JPEG_ERR_IO = 7,            /* unreadable, truncated or corrupt stream (also: a coefficient block beyond
                                     VGE_JPEG_BLOCK_L1_MAX, see below) */
  VGE_JPEG_ERR_SHAPE = 8,         /* size / components / sampling differ from the call's layout */
  VGE_JPEG_ERR_PROGRESSIVE = 20,  /* SOF2 (and the other non-baseline Huffman processes: SOF1, SOF3, SOF5-7) */
  VGE_JPEG_ERR_ARITHMETIC = 21,   /* arithmetic coding (SOF9-11, SOF13-15) */
  VGE_JPEG_ERR_PRECISION = 22,    /* sample precision other than 8 bits, or 16-bit quantisation tables */
  VGE_JPEG_ERR_COMPONENTS = 23,   /* component count other than 1 or 3 (CMYK / YCCK) */
  VGE_JPEG_ERR_SAMPLING = 24      /* sampling factors other than luma 1x1 / 2x1 / 2x2 with chroma 1x1 */
};

/* The reconstructs run the IDCT in 32-bit arithmetic.  With S = sum over a block of |coef * q|, no value the IDCT
 * descales leaves int32 while S <= VGE_JPEG_BLOCK_L1_MAX (derivation: csrc/vge_jpeg_math.h); a stream encoded from
 * 8-bit samples stays below 16,400.  The entropy decoder gives a frame with a block beyond the bound VGE_JPEG_ERR_IO,
 * so host and device agree on every frame they accept. */
#define VGE_JPEG_BLOCK_L1_MAX 32767

typedef struct {
  int32_t width, height;
  int32_t n_comp;  /* 1 or 3 for supported streams */
  int32_t h0, v0;  /* sampling factors of component 0 */
  int32_t status;  /* VGE_JPEG_OK or a code above */
} vge_jpeg_info;

/* Where each component's blocks live inside one frame's coefficient buffer.  A component's plane is bw x bh blocks
 * (whole MCUs), row-major, 64 int16 per block in natural order; component c starts at block off[c]; a frame is
 * blocks_per_frame blocks.  Unused components are zero.  Computable from the probe result alone. */
typedef struct {
  int32_t width, height, n_comp, h0, v0;
  int32_t mcus_x, mcus_y;
  int32_t bw[3], bh[3], off[3];
  int32_t blocks_per_frame;
} vge_jpeg_layout;

/* paths[n] -> info[n], reading the headers (up to the first SOS) only. */
int vge_jpeg_probe(const char* const* paths, int n, int n_threads, vge_jpeg_info* info);

/* Layout for frames of this size and sampling; VGE_JPEG_ERR_COMPONENTS / _SAMPLING / _ARG for unsupported ones. */
int vge_jpeg_make_layout(int width, int height, int n_comp, int h0, int v0, vge_jpeg_layout* layout);

/* Host, multithreaded over frames.  coef: int16 [n, blocks_per_frame, 64]; qtab: uint16 [n, 3, 64] (natural order,
 * one table per component).  A frame that fails has its coefficients zeroed and its tables set to 1 and does not
 * disturb the others.  status[n] may be NULL. */
int vge_jpeg_entropy_decode(const char* const* paths, int n, int n_threads, const vge_jpeg_layout* layout,
                            int16_t* coef, uint16_t* qtab, int32_t* status);

/* Device: coef / qtab / rgb are device pointers, stream is a hipStream_t (NULL: the default stream); the launch is
 * asynchronous.  rgb: uint8 [n_frames, height, width, 3]. */
int vge_jpeg_reconstruct(const int16_t* coef, const uint16_t* qtab, const vge_jpeg_layout* layout, int n_frames,
                         uint8_t* rgb, void* stream);

/* Host: the same inputs and output in host memory, plain C++, multithreaded over frames. */
int vge_jpeg_reconstruct_host(const int16_t* coef, const uint16_t* qtab, const vge_jpeg_layout* layout, int n_frames,
                              int n_threads, uint8_t* rgb);

/* ---- Encoding: the mirror images of the calls above, for frames that are already in memory.
 *
 * The reference's models only ever see pixels that went through cv2.imwrite (libjpeg's encoder: quality 95, 4:2:0) and
 * cv2.imread.  Huffman coding is lossless, so those pixels are reconstruct(forward(frame)): the forward call below is
 * the lossy half of libjpeg's encoder -- RGB -> YCbCr, edge expansion, box downsampling, the "islow" forward DCT,
 * quantisation, the dummy blocks that fill the last MCU column / row -- and yields exactly the coefficients
 * vge_jpeg_entropy_decode reads out of the file libjpeg would have written, in the same layout.  The entropy encoder
 * writes that file (baseline JFIF, the standard Huffman tables, no restart markers, one interleaved scan), byte for byte:
 * on host threads to paths or into memory, or on the device into memory (plan / emit below).
 * Only 3-component layouts are encoded (frames here are RGB): a 1-component layout gets VGE_JPEG_ERR_COMPONENTS. */

/* libjpeg's tables for `quality` (clamped to 1..100; Annex K.1 / K.2 scaled and forced to baseline) -> qtab
 * uint16 [3][64], natural order: component 0 the luminance table, components 1 and 2 the chrominance table. */
int vge_jpeg_quant_tables(int quality, uint16_t* qtab);

/* Device: rgb uint8 [n_frames, height, width, 3], qtab uint16 [3][64] (one set for the whole call, entries 1..255),
 * coef int16 [n_frames, blocks_per_frame, 64] are device pointers (qtab and coef 16-byte aligned; rgb 4-byte aligned
 * when the width is a multiple of 4, where it is read as dwords); stream
 * is a hipStream_t (NULL: the default stream); the launch is asynchronous.  Every block of the layout is written. */
int vge_jpeg_forward(const uint8_t* rgb, const vge_jpeg_layout* layout, int n_frames, const uint16_t* qtab,
                     int16_t* coef, void* stream);

/* Host: the same in host memory, plain C++, multithreaded over frames. */
int vge_jpeg_forward_host(const uint8_t* rgb, const vge_jpeg_layout* layout, int n_frames, int n_threads,
                          const uint16_t* qtab, int16_t* coef);

/* Host, multithreaded over frames: frame i's coefficients -> a complete JPEG file at paths[i]; sizes[i] its length in
 * bytes.  A frame whose file cannot be written gets VGE_JPEG_ERR_IO in status[i] (sizes[i] 0) and does not disturb the
 * others.  sizes and status may be NULL. */
int vge_jpeg_entropy_encode(const int16_t* coef, const uint16_t* qtab, const vge_jpeg_layout* layout, int n,
                            int n_threads, const char* const* paths, int64_t* sizes, int32_t* status);

/* Host: the same files into memory.  out == NULL: sizes only.  Otherwise file i goes to out + offsets[i] (offsets are
 * the caller's: files may be packed with gaps, no byte outside a file is touched); a file that does not fit into
 * out_bytes gets VGE_JPEG_ERR_ARG.  A frame with a DC difference beyond 11 bits or an AC value beyond 10 bits (not the
 * forward transform's output) gets VGE_JPEG_ERR_ARG and size 0 and does not disturb the others.  sizes and status may
 * be NULL. */
int vge_jpeg_entropy_encode_mem(const int16_t* coef, const uint16_t* qtab, const vge_jpeg_layout* layout, int n,
                                int n_threads, const int64_t* offsets, uint8_t* out, int64_t out_bytes, int64_t* sizes,
                                int32_t* status);

/* Host, multithreaded over files: sizes[i] bytes at data + offsets[i] -> paths[i].  A file that cannot be written gets
 * VGE_JPEG_ERR_IO in status[i] (may be NULL) and does not disturb the others. */
int vge_jpeg_write_files(const uint8_t* data, const int64_t* offsets, const int64_t* sizes, int n, int n_threads,
                         const char* const* paths, int32_t* status);

/* Device entropy coder (csrc/vge_jpeg_huff.hip): the coefficient buffer exactly as vge_jpeg_forward leaves it -> the
 * same files as above, on the device.  All pointers but the layout are device pointers (workspace 16-byte aligned,
 * coef 2-byte, sizes / offsets 8-byte); the calls are asynchronous on `stream` and allocate nothing.  The split is at
 * the only point where the host must learn something, the file sizes:
 *   plan   codes every block (one wave per block, one lane per zigzag position), builds each frame's unstuffed scan in
 *          the workspace and counts its FF bytes; sizes[i] is file i's length, status[i] VGE_JPEG_OK -- or size 0 and
 *          VGE_JPEG_ERR_ARG for a frame baseline coding cannot carry.  It clears what it accumulates into itself, so
 *          a workspace may be reused as it is.
 *   emit   writes file i (headers, the scan with 00 stuffed after every FF, EOI) to out + offsets[i] and touches no
 *          byte outside [offsets[i], offsets[i] + sizes[i]).  A refused frame writes nothing.  The offsets live on the
 *          device, so the host cannot compare them with out_bytes: a negative out_bytes is VGE_JPEG_ERR_ARG before
 *          any launch, and a file that would not lie inside [0, out_bytes) is left unwritten by the kernel.
 * Frames of more than 2^31 / 1658 blocks are refused with VGE_JPEG_ERR_ARG (bit positions are 32-bit).
 * vge_jpeg_entropy_segment_blocks: the scan blocks one workgroup codes -- a frame is ceil(blocks / that) independent
 * work segments (exported for the tests, which make sure a case spans several). */
size_t vge_jpeg_entropy_workspace_bytes(const vge_jpeg_layout* layout, int n_frames);
int vge_jpeg_entropy_plan(const int16_t* coef, const vge_jpeg_layout* layout, int n_frames, void* workspace,
                          int64_t* sizes, int32_t* status, void* stream);
int vge_jpeg_entropy_emit(const void* workspace, const uint16_t* qtab, const vge_jpeg_layout* layout, int n_frames,
                          const int64_t* offsets, uint8_t* out, int64_t out_bytes, void* stream);
int vge_jpeg_entropy_segment_blocks(void);

/* ---- Files held in memory: the probe's and the entropy decoder's twins for a packed buffer.
 *
 * File i is sizes[i] bytes at data + offsets[i] of a buffer of data_bytes bytes -- the (data, offsets) pair the
 * in-memory encoders above produce.  Files may be packed with gaps and in any order.  A file with a negative offset or
 * size, or one that does not lie inside [0, data_bytes), gets VGE_JPEG_ERR_ARG and none of its bytes is read; an empty
 * file is VGE_JPEG_ERR_IO, as an empty file on disk is.  Everything else -- outputs, per-frame statuses, the frame that
 * fails alone -- is vge_jpeg_probe's and vge_jpeg_entropy_decode's contract, to the bit; the path calls map the file
 * and run the same code.  status may be NULL on the host calls. */
/* Host threads over files, for callers that want the raw files in one (pinned) buffer: sizes[i] is the length of
 * paths[i] (0 for a path that is no readable regular file); read_files then reads sizes[i] bytes of paths[i] to
 * data + offsets[i].  A file that cannot be read or has become shorter gets VGE_JPEG_ERR_IO (_ARG when it does
 * not lie inside data_bytes) and zero bytes in its place, and does not disturb the others.  status may be NULL. */
int vge_jpeg_file_sizes(const char* const* paths, int n, int n_threads, int64_t* sizes);
int vge_jpeg_read_files(const char* const* paths, int n, int n_threads, const int64_t* offsets, const int64_t* sizes,
                        uint8_t* data, int64_t data_bytes, int32_t* status);

int vge_jpeg_probe_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                       int n_threads, vge_jpeg_info* info);
int vge_jpeg_entropy_decode_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes,
                                int n, int n_threads, const vge_jpeg_layout* layout, int16_t* coef, uint16_t* qtab,
                                int32_t* status);

/* Device entropy decoder (csrc/vge_jpeg_dehuff.hip): the same files in device memory -> coef / qtab / status in device
 * memory, equal to the host decoder's; Huffman decoding is parallel inside a frame by self-synchronisation.  Every
 * pointer but the layout is a device pointer (workspace and coef 16-byte aligned, offsets / sizes 8-byte, status /
 * rounds 4-byte).  The call is asynchronous on `stream`, allocates nothing and learns nothing from the device: its
 * return value covers the arguments the host can see and the launches (VGE_JPEG_ERR_ARG / _HIP); the per-frame codes
 * are in status[] only.  The kernels own every block of every frame: coef need not be cleared, a failed frame is zeroed
 * with tables of 1.  rounds (may be NULL): int32 [n], the most synchronisation rounds any tile of frame i needed (1: a
 * single subsequence; 2: every guess was right after one carry).
 *   workspace_bytes  for n_frames files inside a buffer of total_file_bytes; pass the same value as data_bytes.  The
 *                    workspace holds one unstuffed copy of every scan: sizes that add up to no more than
 *                    total_file_bytes always fit; where files overlap so far that the copies do not, the files from
 *                    the first that no longer fits get VGE_JPEG_ERR_ARG.
 * A file of 2^28 bytes or more gets VGE_JPEG_ERR_ARG (bit positions are 32-bit).
 * One class of corrupt stream is outside the equality with the host: a restart interval with a whole surplus byte or
 * more between its last MCU and its marker.  The host's verdict there depends on how far its 64-bit reader has read
 * ahead; the device always gives VGE_JPEG_ERR_IO.
 * subsequence_bytes: the scan bytes one lane starts on; tile_bytes: the scan bytes one workgroup covers per pass over a
 * restart interval (exported for the tests, which make sure a case spans several). */
size_t vge_jpeg_entropy_decode_workspace_bytes(const vge_jpeg_layout* layout, int n_frames, int64_t total_file_bytes);
int vge_jpeg_entropy_decode_device(const uint8_t* data, int64_t data_bytes, const int64_t* offsets,
                                   const int64_t* sizes, int n_frames, const vge_jpeg_layout* layout, void* workspace,
                                   int16_t* coef, uint16_t* qtab, int32_t* status, int32_t* rounds, void* stream);
int vge_jpeg_entropy_decode_subsequence_bytes(void);
int vge_jpeg_entropy_decode_tile_bytes(void);

#ifdef __cplusplus
}
#endif
#endif /* VGE_FRAMES_H */
