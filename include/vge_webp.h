/* vge_webp.h -- lossless WebP (VP8L) videos and frames decoded to uint8 RGB frames, on host threads or on the device.
 *
 * Lossless WebP is what ComfyUI's SaveAnimatedWEBP node writes by default and what Pillow's
 * save(..., "WEBP", save_all=True, lossless=True) writes: a RIFF container with one VP8L bitstream (a still) or an
 * animation of ANMF frames, each a VP8L-coded sub-rectangle with a blend and a dispose bit, drawn onto an RGBA canvas
 * that is carried from frame to frame.  Unlike GIF it keeps all 24 colour bits.  This ABI decodes it twice with the
 * same verdicts: on host threads, and on the device from the file bytes alone (csrc/vge_webp.hip).  Both run the same
 * bitstream reader, per-pixel inverse-transform steps and per-pixel composition step (csrc/vge_webp_vp8l.h).
 *
 * Conventions are vge_gif.h's: files on disk or packed in memory (file j is sizes[j] bytes at data + offsets[j]; gaps
 * and any order are fine); one status per frame; every call returns VGE_WEBP_OK or the first failing code;
 * vge_last_error names the first failure; n_threads <= 0: vge_ingest_default_threads().  A call's output holds the
 * frames of its files back to back; all files of one call share the canvas (width, height); a file of another size
 * gets VGE_WEBP_ERR_SHAPE on all its frames.  A file that fails before its first frame has no frames: its code is in
 * file_status[] only.
 *
 * Container.  RIFF/WEBP with a bare VP8L chunk; VP8X + VP8L; VP8X + ANIM + ANMF frames (x / 2, y / 2, w - 1, h - 1,
 * duration, blend bit, dispose bit, then the frame's VP8L chunk; any other chunk in front of it leaves the frame
 * without an image, VGE_WEBP_ERR_IO, as libwebp's demuxer has it).  Odd chunk sizes are padded;
 * chunks that are not known (ICCP, EXIF, "XMP ", anything else) are skipped; durations, the loop count and ANIM's
 * background colour are ignored (the canvas starts transparent black, as Pillow's decoder has it).  A RIFF size that
 * reaches beyond the file is a truncated file and is refused whole with VGE_WEBP_ERR_IO, as libwebp's demuxer refuses
 * it; bytes after the RIFF size are ignored.  Without VP8X the canvas is the VP8L header's size.
 *
 * Accept / reject of a VP8L stream, the same on host and device (and libwebp's, pinned against Pillow):
 *   - signature 0x2f and version 0, else VGE_WEBP_ERR_IO; each transform at most once;
 *   - a set of code lengths is accepted when it holds exactly one symbol (of any length: the code then consumes no
 *     bits), or when it is complete; no symbol at all, an over-subscribed and an incomplete set are refused; the same
 *     holds for the code-length code; max_symbol beyond the alphabet and a repeat that runs beyond it are refused; a
 *     simple code's symbol beyond the alphabet (distance codes: 40) is dropped;
 *   - a colour cache of 0 or 12..15 bits is refused;
 *   - a copy whose distance reaches before pixel 0 or whose length runs beyond the last pixel is refused;
 *   - a stream is refused as soon as one read needs a bit beyond the payload (a stream that ends early); bits and bytes
 *     after the last pixel are ignored;
 *   - predictor modes 14 and 15 predict opaque black; a colour index beyond the palette reads as 0x00000000.
 * All of these give VGE_WEBP_ERR_IO.  A failing frame takes every later frame of its file with it, each with the same
 * code; the earlier frames stand.
 *
 * Prefix-code groups.  A frame's groups are decoded into a table arena of fixed capacity: VGE_WEBP_MAX_GROUPS groups,
 * whose codes are kept in canonical form (16 counts per code and the symbols that have a code, in code order), with
 * VGE_WEBP_TABLE_SYMBOLS symbols for all groups of the frame together.  A frame whose entropy image names a group
 * index of VGE_WEBP_MAX_GROUPS or more, or whose groups hold more coded symbols than that, is refused with
 * VGE_WEBP_ERR_GROUPS by the host and the device alike.  The largest count seen over the test cases, the golden files
 * and the benchmark's files is in profiles/webp_decode_device.json.
 *
 * Composition is what PIL.ImageSequence frames give after .convert("RGB"): libwebp's animation decoder on an RGBA
 * canvas, alpha dropped at the end; DESIGN.md section 5b''''' states the rule, key frames and partial alpha included.
 */
#ifndef VGE_WEBP_H
#define VGE_WEBP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VGE_WEBP_MAX_GROUPS 256
#define VGE_WEBP_TABLE_SYMBOLS 131072

enum {
  VGE_WEBP_OK = 0,
  VGE_WEBP_ERR_ARG = 1,     /* bad argument; a file of 2^28 bytes or more (bit positions are 32-bit) */
  VGE_WEBP_ERR_HIP = 2,     /* a HIP call failed */
  VGE_WEBP_ERR_IO = 7,      /* not a WebP, truncated, no frame, a corrupt stream */
  VGE_WEBP_ERR_SHAPE = 8,   /* the file's canvas differs from the call's */
  VGE_WEBP_ERR_LOSSY = 50,  /* a VP8 or ALPH chunk: lossy WebP is not decoded */
  VGE_WEBP_ERR_BOUNDS = 51, /* an ANMF rectangle outside the canvas, or a VP8L header whose size differs from its
                               rectangle (a still: from the VP8X canvas) */
  VGE_WEBP_ERR_GROUPS = 52  /* more prefix-code groups or coded symbols than the table arena holds */
};

typedef struct {
  int32_t width, height; /* the canvas */
  int32_t n_frames;
  int32_t status;        /* VGE_WEBP_OK or the first failing code the parser sees (only VP8L headers are looked at) */
  int64_t vp8l_bytes;    /* payload bytes of all VP8L chunks that are frames */
  int64_t n_chunks;      /* chunks walked, ANMF sub-chunks included */
} vge_webp_info;

/* Headers and chunk structure only; nothing is decoded. */
int vge_webp_probe(const char* const* paths, int n, int n_threads, vge_webp_info* info);
int vge_webp_probe_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                       int n_threads, vge_webp_info* info);

/* The host decoder: rgb is uint8 [frame_cap, height, width, 3] and status int32 [frame_cap] in host memory.  Files are
 * parsed on threads, then the VP8L streams of all frames of all files are decoded (entropy and inverse transforms)
 * across the threads, then the files are composed on threads.  *n_frames_out (may be NULL): the frames of all files;
 * when that exceeds frame_cap nothing is decoded and the call returns VGE_WEBP_ERR_ARG.  file_status[n] (may be NULL):
 * per file, its first failing code.  A failing frame and the later frames of its file have unspecified pixels.  A file
 * that does not lie inside [0, data_bytes) gets VGE_WEBP_ERR_ARG and none of its bytes is read. */
int vge_webp_decode(const char* const* paths, int n, int n_threads, int width, int height, int64_t frame_cap,
                    uint8_t* rgb, int32_t* status, int32_t* file_status, int64_t* n_frames_out);
int vge_webp_decode_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                        int n_threads, int width, int height, int64_t frame_cap, uint8_t* rgb, int32_t* status,
                        int32_t* file_status, int64_t* n_frames_out);

/* ---- Device route.  Plain data, copied to the device as bytes. */
typedef struct {
  int64_t file_off;   /* the frame's file inside the buffer: the payload must lie inside it */
  int64_t file_bytes;
  int64_t pay_off;    /* the frame's VP8L payload, relative to file_off */
  int64_t pay_bytes;
  int64_t slot_off;   /* workspace byte offset of the frame's slot (16-aligned): two ARGB planes of w * h and the table
                         arena, vge_webp_slot_bytes(w, h) bytes */
  int32_t file;       /* owner file */
  int32_t index;      /* frame index within it; a file's descriptors are consecutive and start at index 0 */
  int32_t frame;      /* index into status[] and the output's first axis; -1: an unused slot */
  int32_t x, y, w, h; /* rectangle on the canvas */
  int32_t blend;      /* 1: source-over (ANMF's blend bit clear), 0: overwrite */
  int32_t dispose;    /* 1: the rectangle is cleared to transparent after the frame */
  int32_t key;        /* 1: libwebp's key-frame rule holds: the frame is drawn on a cleared canvas and never blended */
  int32_t plan_status; /* non-zero: the plan refused the frame (or an earlier one of its file) with this code */
  int32_t reserved;
} vge_webp_desc;

/* Host; decodes nothing.  Walks every file and emits one descriptor per frame, file after file, into descs[desc_cap]
 * (frame = position in that order); descs may be NULL with capacity 0 to count only (the sum of the probe's n_frames
 * always suffices).  A VP8L payload is contiguous in its file, so a descriptor points into the file and there is
 * nothing to gather: the route has no segments.  status[desc_cap] (may be NULL) gets the plan's code per frame: a frame
 * the parser refuses, and every later frame of its file, carries it in plan_status and here, and owns no workspace.
 * file_status[n] (may be NULL) as in vge_webp_decode_mem.  Returns VGE_WEBP_ERR_ARG when the capacity is too small,
 * else VGE_WEBP_OK or the first failing code. */
int vge_webp_plan_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                      int n_threads, int width, int height, vge_webp_desc* descs, int64_t desc_cap, int64_t* n_descs,
                      int32_t* status, int32_t* file_status, int64_t* workspace_bytes);

/* Device.  data, descs, workspace, rgb (uint8 [n_frames, height, width, 3]) and status[n_frames] (int32) are device
 * pointers (descs 8-byte aligned, workspace 16-byte, status 4-byte).  The call is asynchronous on `stream` (a
 * hipStream_t; NULL: the default stream), allocates nothing and learns nothing from the device: its return value
 * covers the arguments the host can see and the launches; the per-frame codes are in status[] only, which the call
 * clears first.  Three kernels: entropy (one wave per frame reads the stream out of the file bytes and writes the
 * coded ARGB plane, the transform data and the groups' tables into the frame's slot), transforms (one wave per frame:
 * the predictor with a lane per row of a 64-row band, two pixels behind the lane above; the other three pointwise) and
 * compose (a row of workgroups per file; a lane per canvas pixel walks the file's frames in order with the RGBA canvas
 * pixel in registers, stores every frame's RGB, stops at the first frame whose status is set and gives the later
 * frames of the file that status).  Every descriptor is checked against data_bytes, workspace_bytes, n_frames and the
 * canvas: a frame reads only its own payload, writes only its own slot and output frame, and every loop consumes
 * input or produces output.  The workspace may be reused as it is.  n_files and the order of descs[] are as in
 * vge_gif_decode_device: owner files in increasing order, each file's descriptors consecutive with index 0, 1, 2...;
 * a descriptor that cannot be reached that way gets VGE_WEBP_ERR_ARG, and an unused slot (frame = -1) inside a file
 * gives the later frames of that file VGE_WEBP_ERR_ARG: no frame is left with status 0 and no pixels. */
int vge_webp_decode_device(const uint8_t* data, int64_t data_bytes, const vge_webp_desc* descs, int n_descs,
                           int n_frames, int n_files, int width, int height, void* workspace, int64_t workspace_bytes,
                           uint8_t* rgb, int32_t* status, void* stream);
/* Workspace for host-side descs[n_descs]: the end of the last slot (at least 16). */
size_t vge_webp_decode_device_workspace_bytes(const vge_webp_desc* descs, int n_descs);
/* Bytes of the slot of a w x h frame. */
int64_t vge_webp_slot_bytes(int w, int h);

#ifdef __cplusplus
}
#endif
#endif /* VGE_WEBP_H */
