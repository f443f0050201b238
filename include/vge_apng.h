/* vge_apng.h -- animated PNG videos decoded to uint8 RGB frames, on host threads or on the device.
 *
 * The animated PNG is the lossless, 24-bit, single-file video that Pillow writes (Image.save(..., save_all=True)), that
 * ComfyUI's SaveAnimatedPNG leaves and that ffmpeg's apng muxer produces.  An APNG frame is a delta: a sub-rectangle of
 * the canvas with a zlib stream of its own (cut into IDAT chunks for the first picture, into fdAT chunks, each behind a
 * sequence number, for the others), a dispose operation and a blend operation.  This ABI decodes it twice with the same
 * verdicts: on host threads (zlib and the C++ unfilter of the still path), and on the device from the file bytes alone
 * (csrc/vge_apng.hip, with the gather kernel and the inflate core of the still path).  Both run the same per-pixel
 * composition step (csrc/vge_apng_px.h).
 *
 * Conventions are vge_gif.h's: files on disk or packed in memory (file j is sizes[j] bytes at data + offsets[j]; gaps
 * and any order are fine); one status per frame; every call returns VGE_APNG_OK or the first failing code;
 * vge_last_error names the first failure; n_threads <= 0: vge_ingest_default_threads().
 *
 * A call's output holds the frames of its files back to back: file j's frames follow those of files 0 .. j - 1, and a
 * file has the probe's n_frames.  All files of one call share the canvas (IHDR width and height) and the colour type; a
 * file that differs gets VGE_APNG_ERR_SHAPE on all its frames.  A file that fails before its first frame (not a PNG, a
 * bad or unsupported IHDR, no IDAT) has no frames: its code is in file_status[] only.
 *
 * Supported pixels are the still path's (vge_png.h): 8 bits per sample, not interlaced, colour types 0, 2, 4 and 6.
 *
 * Frames, as PIL.ImageSequence yields them (Pillow 12; where it differs from the APNG specification, Pillow wins):
 *   - a file is animated when an acTL chunk with a count of 1 .. 2^31 stands in front of the first IDAT, and only one
 *     such chunk; otherwise (no acTL, acTL behind IDAT, two of them) it is a video of one frame, its IDAT picture, and
 *     fcTL and fdAT chunks are not looked at;
 *   - an fcTL chunk opens a frame, whose data are the IDAT chunks (first picture) or fdAT chunks that follow up to the
 *     next fcTL; an IDAT run with no fcTL in front of it is a default image that is not part of the animation, and
 *     Pillow yields it as a frame of its own, first: whole canvas, no disposal, blend SOURCE;
 *   - n_frames is min(acTL count + 1 for such a default image, frames present in the file): a file that declares more
 *     frames than it holds has those it holds, one that declares fewer has the declared ones;
 *   - tRNS counts when it stands in front of the first IDAT.
 *
 * Accept / reject, the same on host and device:
 *   - the zlib and filter rules are vge_png.h's (a partial trailer is accepted, filter bytes above 4 are refused, the
 *     stream stops at the count), per frame with the frame's own count h * (1 + w * bytes_per_pixel);
 *   - sequence numbers (fcTL and fdAT share one counter from 0) must come in order: the frame that holds the chunk out
 *     of order gets VGE_APNG_ERR_IO, and so does a frame whose fcTL is followed by no data chunk, an fcTL shorter than
 *     26 bytes, and a frame that the end of the file cuts;
 *   - a rectangle that reaches outside the canvas or has a zero side, and an fcTL in front of IDAT that is not the whole
 *     canvas, get VGE_APNG_ERR_BOUNDS;
 *   - a rejected frame takes every later frame of its file with it, each with the same code; the earlier frames stand.
 * Chunk CRCs, delays and loop counts are ignored.
 *
 * Composition is what PIL.ImageSequence frames give after .convert("RGB"); DESIGN.md section 5b'''''' states the rule.
 */
#ifndef VGE_APNG_H
#define VGE_APNG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  VGE_APNG_OK = 0,
  VGE_APNG_ERR_ARG = 1,         /* bad argument; a frame of 2^28 gathered or 2^31 filtered bytes or more */
  VGE_APNG_ERR_HIP = 2,         /* a HIP call failed */
  VGE_APNG_ERR_IO = 7,          /* not a PNG, truncated, bad IHDR, no IDAT, a sequence number out of order, an fcTL
                                   without data, a corrupt stream, too few bytes, filter byte > 4, wrong Adler-32 */
  VGE_APNG_ERR_SHAPE = 8,       /* the file's canvas or colour type differ from the call's */
  VGE_APNG_ERR_INTERLACED = 30, /* Adam7 */
  VGE_APNG_ERR_BITDEPTH = 31,   /* bit depth other than 8 */
  VGE_APNG_ERR_PALETTE = 32,    /* colour type 3 */
  VGE_APNG_ERR_BOUNDS = 60      /* a frame rectangle reaches outside the canvas or is zero-sized, or the first
                                   animation frame (an fcTL in front of IDAT) is not the whole canvas */
};

enum { VGE_APNG_DISPOSE_NONE = 0, VGE_APNG_DISPOSE_BACKGROUND = 1, VGE_APNG_DISPOSE_PREVIOUS = 2 };
enum { VGE_APNG_BLEND_SOURCE = 0, VGE_APNG_BLEND_OVER = 1 };

typedef struct {
  int32_t width, height; /* the canvas (IHDR) */
  int32_t color_type;    /* 0, 2, 4 or 6 for supported files */
  int32_t bit_depth;
  int32_t interlace;
  int32_t n_frames;      /* what the iterator yields: see above */
  int32_t default_image; /* 1: frame 0 is a default image that is not part of the animation */
  int32_t status;        /* VGE_APNG_OK or the first failing code the parser sees (no byte is inflated) */
  int64_t n_chunks;      /* non-empty IDAT / fdAT payloads of those frames */
  int64_t data_bytes;    /* their bytes, without the fdAT sequence numbers */
} vge_apng_info;

/* Chunk headers only; nothing is inflated. */
int vge_apng_probe(const char* const* paths, int n, int n_threads, vge_apng_info* info);
int vge_apng_probe_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                       int n_threads, vge_apng_info* info);

/* The host decoder: rgb is uint8 [frame_cap, height, width, 3] and status int32 [frame_cap] in host memory.  Files are
 * parsed on threads, then the frames of all files are inflated and unfiltered on the threads, then the files are
 * composed on threads.  *n_frames_out (may be NULL): the frames of all files; when that exceeds frame_cap nothing is
 * decoded and the call returns VGE_APNG_ERR_ARG.  file_status[n] (may be NULL): per file, its first failing code.  A
 * failing frame and the later frames of its file have unspecified pixels.  A file that does not lie inside
 * [0, data_bytes) gets VGE_APNG_ERR_ARG and none of its bytes is read. */
int vge_apng_decode(const char* const* paths, int n, int n_threads, int width, int height, int color_type,
                    int64_t frame_cap, uint8_t* rgb, int32_t* status, int32_t* file_status, int64_t* n_frames_out);
int vge_apng_decode_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                        int n_threads, int width, int height, int color_type, int64_t frame_cap, uint8_t* rgb,
                        int32_t* status, int32_t* file_status, int64_t* n_frames_out);

/* ---- Device route.  Plain data, copied to the device as bytes. */
typedef struct {
  int64_t file_off;   /* the frame's file inside the buffer: its segments must lie inside it */
  int64_t file_bytes;
  int64_t gat_off;    /* workspace byte offset of the frame's gathered IDAT / fdAT payloads (the zlib stream) */
  int64_t gat_bytes;
  int64_t slot_off;   /* workspace byte offset of the frame's rows, filtered and then as raw pixels of the file's colour
                         type behind their filter bytes (16-byte aligned; padded to a dword) */
  int64_t raw_bytes;  /* h * (1 + w * bytes_per_pixel) */
  int32_t file;       /* owner file */
  int32_t index;      /* frame index within it; a file's descriptors are consecutive and start at index 0 */
  int32_t frame;      /* index into status[] and the output's first axis; -1: an unused slot */
  int32_t x, y, w, h; /* rectangle on the canvas */
  int32_t color_type;
  int32_t dispose_op; /* as the file states them; csrc/vge_apng_px.h derives what takes effect */
  int32_t blend_op;
  int32_t trns;       /* colour type 2: the tRNS colour R | G << 8 | B << 16; -1: none (or one no 8-bit pixel equals) */
  int32_t plan_status; /* non-zero: the plan refused the frame (or an earlier one of its file) with this code */
} vge_apng_desc;

typedef struct { /* the shape of vge_png_segment */
  int64_t src_off; /* payload bytes inside the buffer, behind the 4 sequence bytes of an fdAT */
  int64_t dst_off; /* where they go inside the workspace */
  int64_t bytes;
  int32_t desc;    /* index of the descriptor the segment belongs to */
  int32_t reserved;
} vge_apng_segment;

/* Host; inflates nothing.  Walks every file and emits one descriptor per frame, file after file, into descs[desc_cap]
 * (frame = position in that order) and one segment per non-empty IDAT / fdAT payload into segs[seg_cap]; either may be
 * NULL with capacity 0 to count only (the sums of the probe's n_frames and n_chunks always suffice).  status[desc_cap]
 * (may be NULL) gets the plan's code per frame: a frame the parser refuses, and every later frame of its file, carries
 * it in plan_status and here, and owns no workspace.  file_status[n] (may be NULL) as in vge_apng_decode_mem.  Returns
 * VGE_APNG_ERR_ARG when a capacity is too small, else VGE_APNG_OK or the first failing code. */
int vge_apng_plan_mem(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const int64_t* sizes, int n,
                      int n_threads, int width, int height, int color_type, vge_apng_desc* descs, int64_t desc_cap,
                      int64_t* n_descs, vge_apng_segment* segs, int64_t seg_cap, int64_t* n_segs, int32_t* status,
                      int32_t* file_status, int64_t* workspace_bytes);

/* Device.  data, descs, segs, workspace, rgb (uint8 [n_frames, height, width, 3]) and status[n_frames] (int32) are
 * device pointers (descs and segs 8-byte aligned, workspace 16-byte, status 4-byte).  The call is asynchronous on
 * `stream` (a hipStream_t; NULL: the default stream), allocates nothing and learns nothing from the device: its return
 * value covers the arguments the host can see and the launches; the per-frame codes are in status[] only, which the
 * call clears first.  Five kernels: gather (each frame's payloads into one run of the workspace; csrc/vge_gather.h),
 * inflate (one wave per frame, the core of the still path, into the frame's slot with the frame's own count), Adler-32
 * (per frame), unfilter (one wave per frame, a lane per row of a 64-row band, with the rectangle's width, height and
 * stride; the slot keeps the raw pixels) and compose (a row of workgroups per file; a lane per canvas pixel walks the
 * file's frames in order with the canvas and the saved value of dispose PREVIOUS in registers, stores every frame's
 * RGB, stops at the first frame whose status is set and gives the later frames of the file that status).  Every
 * descriptor and segment is checked against data_bytes, workspace_bytes, n_frames, the canvas and the colour type: a
 * frame reads only its own file bytes and gathered run, writes only its own slot and output frame, and every loop
 * consumes input or produces output.  The workspace may be reused as it is.
 * n_files: the files of the plan; the compose kernel finds a file's first descriptor by a binary search on the owner
 * field.  The order of descs[] is therefore part of the contract, and it is the order the plan emits: owner files in
 * increasing order, each file's descriptors consecutive with index 0, 1, 2...  A descriptor that cannot be reached that
 * way (its run does not start at index 0, its owner is outside [0, n_files), another run of the same owner comes first,
 * the owners are out of order) gets VGE_APNG_ERR_ARG from the inflate kernel, and an unused slot (frame = -1) inside a
 * file gives the later frames of that file VGE_APNG_ERR_ARG: no frame is left with status 0 and no pixels. */
int vge_apng_decode_device(const uint8_t* data, int64_t data_bytes, const vge_apng_desc* descs, int n_descs,
                           const vge_apng_segment* segs, int64_t n_segs, int n_frames, int n_files, int width,
                           int height, int color_type, void* workspace, int64_t workspace_bytes, uint8_t* rgb,
                           int32_t* status, void* stream);
/* Workspace for host-side descs[n_descs]: the end of the last gathered run or slot (at least 16). */
size_t vge_apng_decode_device_workspace_bytes(const vge_apng_desc* descs, int n_descs);

#ifdef __cplusplus
}
#endif
#endif /* VGE_APNG_H */
