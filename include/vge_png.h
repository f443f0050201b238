/* vge_png.h -- PNG frame folders decoded to uint8 RGB, on host threads or on the device.
 *
 * Generators of the videos this project scores usually leave a folder of PNG frames (diffusers exports,
 * `ffmpeg -i x.mp4 %06d.png`): the lossless first generation, the array cap.read() would have handed to the reference.
 * A PNG frame is one zlib stream cut into IDAT chunks plus a per-row filter.  This ABI decodes it twice with the same
 * verdicts: on host threads (zlib's inflate and a plain C++ unfilter: the route without a GPU, and the parity partner),
 * and on the device, from the file bytes alone (csrc/vge_png.hip, with the inflate core of the npz path).
 *
 * Conventions are vge_frames.h's and vge_ingest.h's: files on disk or packed in memory (file j is sizes[j] bytes at
 * data + offsets[j]; gaps and any order are fine); per-frame status[]; every call returns VGE_PNG_OK or the first
 * failing frame's code; vge_last_error names the first failure; n_threads <= 0: vge_ingest_default_threads().
 *
 * Supported files: 8 bits per sample, not interlaced, colour type 0 (grey, replicated to RGB), 2 (RGB), 4 and 6 (alpha
 * dropped, not composited).  Ancillary chunks (tRNS and gAMA included) are ignored.  This is what Pillow's
 * Image.open(f).convert("RGB") and cv2.imread's default flag give for these types.  All frames of one call share
 * width, height and colour type; a frame that differs gets the shape status.
 *
 * Accept / reject, the same on host and device:
 *   - a frame is accepted when its stream produces the full count height * (1 + width * bytes_per_pixel), every filter
 *     byte is <= 4, and the Adler-32 matches -- if all four trailer bytes directly follow a final block that ends
 *     exactly at the count.  An absent or partial trailer is accepted, and so is a missing IEND;
 *   - a stream that has not ended at the count is accepted without its checksum (the device stops at the count);
 *   - the zlib header must have CM = 8, CINFO <= 7, (CMF * 256 + FLG) % 31 == 0 and FDICT clear; the declared window is
 *     not enforced beyond that (zlib does not enforce it either);
 *   - chunk CRCs are checked by neither side; the IDAT run ends at the first chunk of another type;
 *   - the host offers zlib the whole input with one spare output byte after the count, and accepts unless zlib reports
 *     a data error or the count was not reached, so its verdict does not depend on how far zlib had read when the
 *     buffer ran full.
 * One class stays outside the equality: a stream with corrupt bytes after the count (the host's zlib meets them, the
 * device accepts the frame without its checksum).  The npz path has the same exception.
 */
#ifndef VGE_PNG_H
#define VGE_PNG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  VGE_PNG_OK = 0,
  VGE_PNG_ERR_ARG = 1,         /* bad argument */
  VGE_PNG_ERR_HIP = 2,         /* a HIP call failed */
  VGE_PNG_ERR_IO = 7,          /* not a PNG, truncated file, bad IHDR, zero width or height, no IDAT, corrupt stream,
                                  too few bytes, filter byte > 4, wrong Adler-32 */
  VGE_PNG_ERR_SHAPE = 8,       /* width, height or colour type differ from the call's layout */
  VGE_PNG_ERR_INTERLACED = 30, /* Adam7 */
  VGE_PNG_ERR_BITDEPTH = 31,   /* bit depth other than 8 */
  VGE_PNG_ERR_PALETTE = 32     /* colour type 3 */
};

typedef struct {
  int32_t width, height;
  int32_t color_type; /* 0, 2, 4 or 6 for supported files */
  int32_t bit_depth;
  int32_t interlace;
  int32_t n_idat;     /* IDAT chunks of the file's one run of them */
  int64_t idat_bytes; /* their payload bytes */
  int32_t status;     /* VGE_PNG_OK or a code above */
  int32_t reserved;
} vge_png_info;

/* Headers only (the chunk headers are walked, nothing is inflated). */
int vge_png_probe(const char* const* paths, int n, int n_threads, vge_png_info* info);
int vge_png_probe_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                      int n_threads, vge_png_info* info);

/* The host decoder, multithreaded over frames: rgb is uint8 [n, height, width, 3] in host memory.  A frame that fails
 * leaves its rows unspecified and does not disturb the others.  A file with a negative offset or size, or one that does
 * not lie inside [0, data_bytes), gets VGE_PNG_ERR_ARG and none of its bytes is read; an empty file is VGE_PNG_ERR_IO.
 * status[n] may be NULL. */
int vge_png_decode(const char* const* paths, int n, int n_threads, int width, int height, int color_type,
                   uint8_t* rgb, int32_t* status);
int vge_png_decode_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                       int n_threads, int width, int height, int color_type, uint8_t* rgb, int32_t* status);

/* ---- Device route.  Plain data, copied to the device as bytes. */
typedef struct {
  int64_t file_off;   /* the frame's file inside the buffer: its segments must lie inside it */
  int64_t file_bytes;
  int64_t gat_off;    /* workspace byte offset of the frame's gathered IDAT payloads (the zlib stream) */
  int64_t gat_bytes;
  int64_t slot_off;   /* workspace byte offset of the frame's filtered rows (16-byte aligned; padded to a dword) */
  int64_t raw_bytes;  /* filtered byte count: height * (1 + width * bytes_per_pixel) */
  int32_t color_type;
  int32_t frame;      /* owner: index into status[] and the output's first axis; -1: an unused slot */
} vge_png_desc;

typedef struct {
  int64_t src_off; /* payload bytes inside the buffer */
  int64_t dst_off; /* where they go inside the workspace */
  int64_t bytes;
  int32_t desc;    /* index of the descriptor the segment belongs to */
  int32_t reserved;
} vge_png_segment;

/* Host; inflates nothing.  Walks the chunks of every file, checks IHDR against (width, height, color_type) and emits
 * descs[n] -- frame i in slot i -- and up to seg_cap segments, one per non-empty IDAT chunk, frame after frame and in
 * file order (segs may be NULL with seg_cap 0 to count only; the sum of the probe's n_idat always suffices).  A frame
 * that fails here gets its final status in status[i] and an unused slot.  A frame of 2^28 gathered bytes or more, or of
 * 2^31 filtered bytes or more, gets VGE_PNG_ERR_ARG (the kernel's bit positions are 32-bit).  *n_segs: segments emitted
 * (or needed); *workspace_bytes (may be NULL): what vge_png_decode_device needs for these descriptors.  Returns
 * VGE_PNG_ERR_ARG when seg_cap is too small, else VGE_PNG_OK or the first failing frame's code. */
int vge_png_plan_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                     int n_threads, int width, int height, int color_type, vge_png_desc* descs, vge_png_segment* segs,
                     int64_t seg_cap, int64_t* n_segs, int32_t* status, int64_t* workspace_bytes);

/* Device.  data, descs, segs, workspace, rgb (uint8 [n_frames, height, width, 3]) and status[n_frames] (int32) are
 * device pointers (descs and segs 8-byte aligned, workspace 16-byte, status 4-byte).  The call is asynchronous on
 * `stream` (a hipStream_t; NULL: the default stream), allocates nothing and learns nothing from the device: its return
 * value covers the arguments the host can see and the launches (VGE_PNG_ERR_ARG / _HIP, named by vge_last_error); the
 * per-frame codes are in status[] only, which the call clears first (pass the plan's codes separately).
 * Four kernels: gather (each frame's IDAT payloads into one run of the workspace), inflate (one wave per frame: zlib
 * header, deflate through a 32 KiB LDS ring into the frame's slot, where the final block ended), Adler-32 (a weighted
 * byte sum, parallel over lanes, compared with the trailer) and unfilter (one wave per frame, lane l on row r0 + l of a
 * 64-row band, one pixel behind lane l - 1; writes the RGB rows).  Every descriptor and segment is checked against
 * data_bytes, workspace_bytes and n_frames: a frame reads only its own file bytes, writes only its own workspace slot
 * and its own output rows, and every loop consumes input or produces output.  A frame that fails sets its own status
 * (the first failure wins), may leave any bytes in its own rows and touches nothing else.  The workspace may be reused
 * as it is. */
int vge_png_decode_device(const uint8_t* data, int64_t data_bytes, const vge_png_desc* descs, int n_descs,
                          const vge_png_segment* segs, int64_t n_segs, int n_frames, int width, int height,
                          int color_type, void* workspace, int64_t workspace_bytes, uint8_t* rgb, int32_t* status,
                          void* stream);
/* Workspace for host-side descs[n_descs]: the end of the last gathered run or slot (at least 16). */
size_t vge_png_decode_device_workspace_bytes(const vge_png_desc* descs, int n_descs);
/* Rows of one unfilter band (for the tests, which make sure a case spans several). */
int vge_png_decode_device_band_rows(void);

#ifdef __cplusplus
}
#endif
#endif /* VGE_PNG_H */
