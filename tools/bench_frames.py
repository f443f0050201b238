"""Frames per second of vge.frames.load_frames on JPEG frame folders, split into its stages, beside Pillow.

    python tools/bench_frames.py [--frames 1024] [--size 256] [--quality 95] [--threads 16] [--folder DIR]
                                 [--entropy host|device] [--format jpg|png|gif|webp|apng] [--out profiles/jpeg_decode.json]

Writes its own JPEGs with Pillow (vge.synth.make_frames content, 4:2:0, quality 95: what cv2.imwrite writes) into a
temporary folder, or reads the *.jpg files of --folder (cycled up to --frames).  Needs a GPU: there is no fallback.

Stages, each warmed up and repeated, reported as median [min, max] over the repeats:
  entropy   vge_jpeg_entropy_decode on --threads host threads into pinned memory   (host clock)
  upload    the pinned coefficient + table buffers to the device                   (device events)
  kernel    vge_jpeg_reconstruct, --inner launches per repeat                      (device events / launches)
  e2e       load_frames(paths, device) ending in a device synchronise              (host clock)
  pillow    PIL decode of the same files on --threads host threads                 (host clock; when Pillow imports)
With --entropy device the rows of the device entropy decoder are measured as well (and written to
profiles/jpeg_decode_device.json unless --out says otherwise):
  read_upload     host threads read the raw files into one pinned buffer + its upload    (host clock, ends in a sync)
  prepare         headers + scan preparation: the same call stopped before its decode kernel   (device events)
  device_entropy  the whole vge_jpeg_entropy_decode_device call: prepare + decode (all rounds) + write + DC
                  (device events); decode_write_dc is the difference of the two medians
  rounds          mean and max of rounds[]
  e2e_device      load_frames(paths, device, entropy="device") ending in a device synchronise   (host clock)
The kernel's HBM floor is (coefficient + table + RGB bytes) / 6.3 TB/s (the achievable rate of a float4 copy).

With --format png (written to profiles/png_decode_device.json unless --out says otherwise) the same frames are written
as PNG files by Pillow at level 6, whose adaptive choice mixes the filter types, and both routes are measured:
  host_decode     vge_png_decode on --threads host threads into pinned memory            (host clock)
  plan            vge_png_plan_mem over the files in memory                              (host clock)
  device_call     vge_png_decode_device: gather + inflate + adler + unfilter             (device events)
  *_kernel        each of the four kernels alone                                         (device events)
  e2e_host / e2e_device      load_frames(paths, device, entropy=...) ending in a device synchronise   (host clock)
  e2e_jpeg_device            the same frames as JPEG files through load_frames(entropy="device")      (host clock)

With --format gif (written to profiles/gif_decode_device.json unless --out says otherwise) the same frames are written
as animated GIFs by Pillow, --gif-files files of --frames / --gif-files frames each (RGB frames, save_all=True: what
diffusers' export_to_gif does, a local colour table per frame), and both routes are measured:
  host_decode     vge_gif_decode on --threads host threads into pinned memory            (host clock)
  plan            vge_gif_plan_mem over the files in memory                              (host clock)
  device_call     vge_gif_decode_device: gather + LZW + compose                          (device events)
  *_kernel        each of the three kernels alone                                        (device events)
  e2e_host / e2e_device      load_videos(files, device, entropy=...) ending in a device synchronise   (host clock)

With --format webp (written to profiles/webp_decode_device.json unless --out says otherwise) the same frames are
written as lossless animated WebP by Pillow (save_all=True, lossless=True), --gif-files files, and both routes are
measured:
  host_decode     vge_webp_decode on --threads host threads into pinned memory           (host clock)
  plan            vge_webp_plan_mem over the files in memory                             (host clock)
  device_call     vge_webp_decode_device: entropy + transforms + compose                 (device events)
  entropy_kernel, entropy_transforms, compose_kernel   the first kernel, the first two, the last alone   (device events)
  e2e_host / e2e_device      load_videos(files, device, entropy=...) ending in a device synchronise   (host clock)
The report also holds the largest number of prefix-code groups a frame asked for, beside the arena's capacity.

With --format apng (written to profiles/apng_decode_device.json unless --out says otherwise) animated PNGs are written
by Pillow (save_all=True), --gif-files files, in two kinds of content -- "deltas": RGB frames that differ in a moving
square, which Pillow crops to the rectangle that changed; "rgba": whole RGBA frames blended OVER -- and both routes are
measured for each kind:
  host_decode     vge_apng_decode on --threads host threads into pinned memory           (host clock)
  plan            vge_apng_plan_mem over the files in memory                             (host clock)
  device_call     vge_apng_decode_device: gather + inflate + adler + unfilter + compose  (device events)
  gather_kernel, inflate_kernel, adler_kernel, inflate_unfilter_kernel, compose_kernel   (device events)
  e2e_host / e2e_device      load_videos(files, device, entropy=...) ending in a device synchronise   (host clock)
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "video-gen-evals_amd"))

HBM_ACHIEVABLE = 6.3e12  # bytes/s


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames.py needs a GPU")
    return torch.device("cuda:0")


def events(fn, inner=1):
    """Seconds per call of fn between two device events, over `inner` calls."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def clocked(lib, call, also=lambda: True):
    """Host seconds of one C call that has to return 0 (and leave `also` true)."""
    t = time.perf_counter()
    rc = call()
    dt = time.perf_counter() - t
    assert rc == 0 and also(), lib.vge_last_error()
    return dt


def staged(set_mask, mask, whole, device_call):
    """One kernel of the device call alone (a hook of the library for this tool), on the data the others left."""
    set_mask(mask)
    try:
        return events(device_call)
    finally:
        set_mask(whole)


def e2e(videos, n, dev, threads, entropy):
    """load_videos ending in a device synchronise -> (host seconds, every frame); all n frames have to decode."""
    import torch
    from vge import frames as FR
    t = time.perf_counter()
    out = FR.load_videos(videos, device=dev, threads=threads, entropy=entropy)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    assert sum(k.size for _, k in out) == n
    return dt, torch.cat([f for f, _ in out])


def measure_calls(args, host_decode, plan, device_call, warm_e2e):
    """Warm up everything, then the three stages every format has -> res."""
    for _ in range(args.warmup):
        host_decode(); events(device_call); warm_e2e()
    return {"host_decode_s": spread([host_decode() for _ in range(args.repeats)]),
            "plan_s": spread([plan() for _ in range(args.repeats)]),
            "device_call_s": spread([events(device_call) for _ in range(args.repeats)])}


def measure_e2e(args, res, videos, n, dev, more=()):
    """The host route, then the device route, then `more` (name, videos, entropy) of load_videos into res -> whether
    the two routes gave the same frames."""
    import torch
    runs = [("e2e_host", videos, "host"), ("e2e_device", videos, "device"), *more]
    took = [[e2e(v, n, dev, args.threads, entropy) for _ in range(args.repeats)] for _, v, entropy in runs]
    for (name, _, _), r in zip(runs, took):
        res[f"{name}_s"] = spread([t for t, _ in r])
    return bool(torch.equal(took[1][-1][1], took[0][-1][1]))


def rates(res, n):
    return {"stages": res, "ms_per_pass": {key[:-2]: 1e3 * v["median"] for key, v in res.items()},
            "frames_per_s": {key[:-2]: n / v["median"] for key, v in res.items()}}


def write_report(args, report) -> int:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))
    return 0


def write_frames(folder: Path, n: int, size: int, ext: str, **save):
    """vge.synth.make_frames content, one file per frame, as Pillow saves it."""
    from PIL import Image
    from vge import synth
    paths = []
    for v in range((n + 63) // 64):
        fr = synth.make_frames(1000 + v, min(64, n - 64 * v), h=size, w=size)
        for f in range(fr.shape[0]):
            p = folder / f"frame_{64 * v + f:06d}{ext}"
            Image.fromarray(fr[f]).save(p, **save)
            paths.append(str(p))
    return paths


def write_jpegs(folder: Path, n: int, size: int, quality: int):
    return write_frames(folder, n, size, ".jpg", format="JPEG", quality=quality, subsampling=2)


def write_pngs(folder: Path, n: int, size: int):
    """Pillow at level 6: its adaptive choice mixes the five filter types."""
    return write_frames(folder, n, size, ".png", format="PNG", compress_level=6)


def write_clips(folder: Path, n_files: int, per_file: int, size: int, ext: str, **save):
    """vge.synth.make_frames content, one animated file per clip, as Pillow saves RGB frames with save_all=True."""
    from PIL import Image
    from vge import synth
    paths = []
    for v in range(n_files):
        fr = synth.make_frames(1000 + v, per_file, h=size, w=size)
        ims = [Image.fromarray(fr[f]) for f in range(per_file)]
        p = folder / f"clip_{v:04d}{ext}"
        ims[0].save(p, save_all=True, append_images=ims[1:], duration=100, loop=0, **save)
        paths.append(str(p))
    return paths


def bench_png(args) -> int:
    """--format png: both routes of load_frames on a PNG folder, the device call's kernels one by one, and the JPEG
    device route on the same frames beside them."""
    import torch
    import zlib
    from vge import frames as FR
    from vge import lib as L
    dev = gpu()
    lib = L.load()
    tmp = tempfile.TemporaryDirectory()
    (Path(tmp.name) / "png").mkdir()
    (Path(tmp.name) / "jpg").mkdir()
    paths = write_pngs(Path(tmp.name) / "png", args.frames, args.size)
    jpegs = write_jpegs(Path(tmp.name) / "jpg", args.frames, args.size, args.quality)
    n = len(paths)
    rows = FR.png_probe(paths, args.threads)
    assert not rows[:, -1].any()
    key = tuple(int(x) for x in rows[0, :3])
    w, h, ct = key
    filters = {}
    for p in paths[:16]:   # which filter types the writer chose
        data = open(p, "rb").read()
        raw = zlib.decompress(b"".join(data[a:a + m] for a, m in _idat(data)))
        for t in raw[::1 + w * 3]:
            filters[int(t)] = filters.get(int(t), 0) + 1

    out_h = torch.empty((n, h, w, 3), dtype=torch.uint8, pin_memory=True)
    status = np.zeros(n, np.int32)
    arr = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
    raw, raw_off, raw_size = FR._read_files(paths, args.threads, pin=True)
    raw_d = raw.to(dev)
    descs = (L.PngDesc * n)()
    n_segs, ws_bytes = C.c_int64(0), C.c_int64(0)
    plan_st = np.zeros(n, np.int32)
    seg_cap = int(rows[:, 5].sum())
    segs = (L.PngSegment * seg_cap)()

    def host_decode():
        return clocked(lib, lambda: lib.vge_png_decode(arr, n, args.threads, w, h, ct, out_h.data_ptr(),
                                                       status.ctypes.data))

    def plan():
        return clocked(lib, lambda: lib.vge_png_plan_mem(
            raw.data_ptr(), int(raw.numel()), raw_off.ctypes.data, raw_size.ctypes.data, n, args.threads, w, h, ct,
            descs, segs, seg_cap, C.byref(n_segs), plan_st.ctypes.data, C.byref(ws_bytes)))

    plan()
    descs_d = torch.frombuffer(descs, dtype=torch.uint8).to(dev)
    segs_d = torch.frombuffer(segs, dtype=torch.uint8).to(dev)
    ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=dev)
    status_d = torch.empty(n, dtype=torch.int32, device=dev)
    out_d = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)

    def device_call():
        L.check(lib.vge_png_decode_device(raw_d.data_ptr(), int(raw_d.numel()), descs_d.data_ptr(), n,
                                          segs_d.data_ptr(), n_segs.value, n, w, h, ct, ws.data_ptr(), int(ws.numel()),
                                          out_d.data_ptr(), status_d.data_ptr(), stream.cuda_stream),
                "vge_png_decode_device")

    def stage(mask):
        return staged(lib.vge_debug_png_stage_mask, mask, 15, device_call)

    def warm_e2e():
        for videos, entropy in (([paths], "host"), ([paths], "device"), ([jpegs], "device")):
            e2e(videos, n, dev, args.threads, entropy)

    res = measure_calls(args, host_decode, plan, device_call, warm_e2e)
    assert int(status_d.abs().sum()) == 0
    calls_equal = bool(torch.equal(out_d.cpu(), out_h))
    for name, mask in (("gather", 1), ("inflate", 2), ("adler", 4)):   # each after a whole call, before the unfilter
        res[f"{name}_kernel_s"] = spread([stage(mask) for _ in range(args.repeats)])
    device_call()
    res["unfilter_kernel_s"] = spread([stage(8) for _ in range(args.repeats)])
    routes_equal = measure_e2e(args, res, [paths], n, dev, more=[("e2e_jpeg_device", [jpegs], "device")])
    report = {
        "what": "vge.frames.load_frames on a PNG folder, both routes, measured on the GPU by tools/bench_frames.py "
                "--format png",
        "device": torch.cuda.get_device_name(0), "frames": n, "width": w, "height": h, "color_type": ct,
        "threads": args.threads,
        "source": f"written here by Pillow: vge.synth.make_frames {args.size}x{args.size}, compress_level 6",
        "filter_types_of_16_files": filters,
        "png_bytes_per_frame": float(raw_size.mean()), "idat_chunks_per_frame": float(rows[:, 5].mean()),
        "jpeg_bytes_per_frame": sum(os.path.getsize(p) for p in jpegs) / n,
        **rates(res, n),
        "device_equals_host": calls_equal and routes_equal,
    }
    tmp.cleanup()
    return write_report(args, report)


def write_gifs(folder: Path, n_files: int, per_file: int, size: int):
    """Animated GIFs from RGB frames (each frame quantised to a local table of its own), the way diffusers'
    export_to_gif calls Pillow."""
    return write_clips(folder, n_files, per_file, size, ".gif", format="GIF", optimize=False)


def bench_gif(args) -> int:
    """--format gif: both routes of load_videos on animated GIFs and the device call's kernels one by one."""
    import torch
    from vge import frames as FR
    from vge import lib as L
    dev = gpu()
    lib = L.load()
    tmp = tempfile.TemporaryDirectory()
    n_files = args.gif_files
    per_file = max(1, args.frames // n_files)
    paths = write_gifs(Path(tmp.name), n_files, per_file, args.size)
    rows = FR.gif_probe(paths, args.threads)
    assert not rows[:, -1].any()
    n = int(rows[:, 2].sum())
    n_blocks = int(rows[:, 4].sum())
    w, h = int(rows[0, 0]), int(rows[0, 1])

    out_h = torch.empty((n, h, w, 3), dtype=torch.uint8, pin_memory=True)
    status = np.zeros(n, np.int32)
    arr = (C.c_char_p * n_files)(*[os.fsencode(p) for p in paths])
    raw, raw_off, raw_size = FR._read_files(paths, args.threads, pin=True)
    raw_d = raw.to(dev)
    descs = (L.GifDesc * n)()
    segs = (L.GifSegment * n_blocks)()
    n_descs, n_segs, ws_bytes = C.c_int64(0), C.c_int64(0), C.c_int64(0)

    def host_decode():
        return clocked(lib, lambda: lib.vge_gif_decode(arr, n_files, args.threads, w, h, n, out_h.data_ptr(),
                                                       status.ctypes.data, None, None))

    def plan():
        return clocked(lib, lambda: lib.vge_gif_plan_mem(
            raw.data_ptr(), int(raw.numel()), raw_off.ctypes.data, raw_size.ctypes.data, n_files, args.threads, w, h,
            descs, n, C.byref(n_descs), segs, n_blocks, C.byref(n_segs), None, None, C.byref(ws_bytes)),
            also=lambda: n_descs.value == n)

    plan()
    descs_d = torch.frombuffer(descs, dtype=torch.uint8).to(dev)
    segs_d = torch.frombuffer(segs, dtype=torch.uint8).to(dev)
    ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=dev)
    status_d = torch.empty(n, dtype=torch.int32, device=dev)
    out_d = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)

    def device_call():
        L.check(lib.vge_gif_decode_device(raw_d.data_ptr(), int(raw_d.numel()), descs_d.data_ptr(), n,
                                          segs_d.data_ptr(), n_segs.value, n, n_files, w, h, ws.data_ptr(), int(ws.numel()),
                                          out_d.data_ptr(), status_d.data_ptr(), stream.cuda_stream),
                "vge_gif_decode_device")

    def warm_e2e():
        e2e(paths, n, dev, args.threads, "host"); e2e(paths, n, dev, args.threads, "device")

    res = measure_calls(args, host_decode, plan, device_call, warm_e2e)
    assert int(status_d.abs().sum()) == 0
    calls_equal = bool(torch.equal(out_d.cpu(), out_h))
    for name, mask in (("gather", 1), ("lzw", 2), ("compose", 4)):   # each on what a whole call left in the workspace
        res[f"{name}_kernel_s"] = spread([staged(lib.vge_debug_gif_stage_mask, mask, 7, device_call)
                                          for _ in range(args.repeats)])
    routes_equal = measure_e2e(args, res, paths, n, dev)
    report = {
        "what": "vge.frames.load_videos on animated GIFs, both routes, measured on the GPU by tools/bench_frames.py "
                "--format gif",
        "device": torch.cuda.get_device_name(0), "files": n_files, "frames": n, "width": w, "height": h,
        "threads": args.threads,
        "source": f"written here by Pillow: vge.synth.make_frames {args.size}x{args.size}, RGB frames, save_all",
        "gif_bytes_per_frame": float(raw_size.sum()) / n, "sub_blocks_per_frame": n_blocks / n,
        "lzw_expansion": "chain walk: each lane walks its code's (prefix, suffix) links backwards from LDS",
        **rates(res, n),
        "yardstick_host_decode_ms": 1e3 * res["host_decode_s"]["median"],
        "device_call_ms": 1e3 * res["device_call_s"]["median"],
        "lzw_share_of_device_call": res["lzw_kernel_s"]["median"] / res["device_call_s"]["median"],
        "device_equals_host": calls_equal and routes_equal,
    }
    tmp.cleanup()
    return write_report(args, report)


def write_webps(folder: Path, n_files: int, per_file: int, size: int):
    """Lossless animated WebP (save_all=True, lossless=True: what ComfyUI's SaveAnimatedWEBP node calls with its
    defaults)."""
    return write_clips(folder, n_files, per_file, size, ".webp", format="WEBP", lossless=True)


def bench_webp(args) -> int:
    """--format webp: both routes of load_videos on lossless animated WebP and the device call's kernels one by one."""
    import torch
    from vge import frames as FR
    from vge import lib as L
    dev = gpu()
    lib = L.load()
    tmp = tempfile.TemporaryDirectory()
    n_files = args.gif_files
    per_file = max(1, args.frames // n_files)
    paths = write_webps(Path(tmp.name), n_files, per_file, args.size)
    rows = FR.webp_probe(paths, args.threads)
    assert not rows[:, -1].any()
    n = int(rows[:, 2].sum())
    w, h = int(rows[0, 0]), int(rows[0, 1])

    out_h = torch.empty((n, h, w, 3), dtype=torch.uint8, pin_memory=True)
    status = np.zeros(n, np.int32)
    arr = (C.c_char_p * n_files)(*[os.fsencode(p) for p in paths])
    raw, raw_off, raw_size = FR._read_files(paths, args.threads, pin=True)
    raw_d = raw.to(dev)
    descs = (L.WebpDesc * n)()
    n_descs, ws_bytes = C.c_int64(0), C.c_int64(0)

    def host_decode():
        return clocked(lib, lambda: lib.vge_webp_decode(arr, n_files, args.threads, w, h, n, out_h.data_ptr(),
                                                        status.ctypes.data, None, None))

    def plan():
        return clocked(lib, lambda: lib.vge_webp_plan_mem(
            raw.data_ptr(), int(raw.numel()), raw_off.ctypes.data, raw_size.ctypes.data, n_files, args.threads, w, h,
            descs, n, C.byref(n_descs), None, None, C.byref(ws_bytes)), also=lambda: n_descs.value == n)

    plan()
    # the largest number of prefix-code groups any frame asks for (the table arena holds VGE_WEBP_MAX_GROUPS)
    feats = lib.vge_debug_webp_features
    feats.argtypes, feats.restype = [C.c_void_p, C.c_int64, C.c_void_p], C.c_int
    most_groups, word = 0, np.zeros(4, np.uint64)
    for i in range(n_files):
        assert feats(raw.data_ptr() + int(raw_off[i]), int(raw_size[i]), word.ctypes.data) == 0
        most_groups = max(most_groups, int(word[3]))
    descs_d = torch.frombuffer(descs, dtype=torch.uint8).to(dev)
    ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=dev)
    status_d = torch.empty(n, dtype=torch.int32, device=dev)
    out_d = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)

    def device_call():
        L.check(lib.vge_webp_decode_device(raw_d.data_ptr(), int(raw_d.numel()), descs_d.data_ptr(), n, n, n_files, w, h,
                                           ws.data_ptr(), int(ws.numel()), out_d.data_ptr(), status_d.data_ptr(),
                                           stream.cuda_stream), "vge_webp_decode_device")

    def warm_e2e():
        e2e(paths, n, dev, args.threads, "host"); e2e(paths, n, dev, args.threads, "device")

    res = measure_calls(args, host_decode, plan, device_call, warm_e2e)
    assert int(status_d.abs().sum()) == 0
    calls_equal = bool(torch.equal(out_d.cpu(), out_h))
    # entropy alone rewrites the coded planes; the transforms then run on fresh input once more before compose is timed
    for name, mask in (("entropy_kernel", 1), ("entropy_transforms", 3), ("compose_kernel", 4)):
        res[f"{name}_s"] = spread([staged(lib.vge_debug_webp_stage_mask, mask, 7, device_call)
                                   for _ in range(args.repeats)])
    routes_equal = measure_e2e(args, res, paths, n, dev)
    report = {
        "what": "vge.frames.load_videos on lossless animated WebP, both routes, measured on the GPU by "
                "tools/bench_frames.py --format webp",
        "device": torch.cuda.get_device_name(0), "files": n_files, "frames": n, "width": w, "height": h,
        "threads": args.threads,
        "source": f"written here by Pillow: vge.synth.make_frames {args.size}x{args.size}, RGB frames, save_all, "
                  "lossless",
        "webp_bytes_per_frame": float(raw_size.sum()) / n,
        "workspace_bytes_per_frame": int(ws_bytes.value) / n,
        "group_capacity": L.WEBP_MAX_GROUPS, "most_groups_in_a_frame": most_groups,
        "entropy_kernel": "one wave per frame, the stream walked by one lane (the shared decoder of "
                          "csrc/vge_webp_vp8l.h); transforms and compose are parallel",
        **rates(res, n),
        "yardstick_host_decode_ms": 1e3 * res["host_decode_s"]["median"],
        "device_call_ms": 1e3 * res["device_call_s"]["median"],
        "entropy_share_of_device_call": res["entropy_kernel_s"]["median"] / res["device_call_s"]["median"],
        "device_equals_host": calls_equal and routes_equal,
    }
    tmp.cleanup()
    return write_report(args, report)


def write_apngs(folder: Path, n_files: int, per_file: int, size: int, kind: str):
    """Animated PNGs as Pillow writes them (save_all=True).  kind "deltas": RGB frames that repeat the clip's first
    vge.synth.make_frames frame with a square moving over it, so that Pillow crops every frame to the rectangle that
    changed; kind "rgba": vge.synth.make_frames frames with an alpha channel of their own, which change everywhere, so
    that every frame is a whole RGBA picture, blended OVER the one before."""
    from PIL import Image
    from vge import synth
    paths = []
    y, x = np.mgrid[0:size, 0:size]
    for v in range(n_files):
        fr = synth.make_frames(1000 + v, per_file, h=size, w=size)
        if kind == "deltas":
            ims = []
            for f in range(per_file):
                a = fr[0].copy()
                q = size // 4
                ox, oy = (7 * f + 3 * v) % (size - q), (5 * f + v) % (size - q)
                a[oy:oy + q, ox:ox + q] = fr[f][oy:oy + q, ox:ox + q][::-1]
                ims.append(Image.fromarray(a))
            kw = {}
        else:
            alpha = ((3 * x + 5 * y) % 256).astype(np.uint8)
            ims = [Image.fromarray(np.dstack([fr[f], np.roll(alpha, 11 * f, axis=1)]), "RGBA") for f in range(per_file)]
            kw = dict(blend=1)
        p = folder / f"{kind}_{v:04d}.png"
        ims[0].save(p, format="PNG", save_all=True, append_images=ims[1:], duration=100, loop=0, **kw)
        paths.append(str(p))
    return paths


def bench_apng(args) -> int:
    """--format apng: both routes of load_videos on animated PNGs of two kinds of content and the device call's kernels
    one by one."""
    import torch
    from vge import frames as FR
    from vge import lib as L
    dev = gpu()
    lib = L.load()
    n_files = args.gif_files
    per_file = max(1, args.frames // n_files)

    def one_kind(kind):
        tmp = tempfile.TemporaryDirectory()
        paths = write_apngs(Path(tmp.name), n_files, per_file, args.size, kind)
        rows = FR.apng_probe(paths, args.threads)
        assert not rows[:, -1].any()
        n, n_chunks = int(rows[:, 5].sum()), int(rows[:, 7].sum())
        w, h, ct = int(rows[0, 0]), int(rows[0, 1]), int(rows[0, 2])

        out_h = torch.empty((n, h, w, 3), dtype=torch.uint8, pin_memory=True)
        status = np.zeros(n, np.int32)
        arr = (C.c_char_p * n_files)(*[os.fsencode(p) for p in paths])
        raw, raw_off, raw_size = FR._read_files(paths, args.threads, pin=True)
        raw_d = raw.to(dev)
        descs = (L.ApngDesc * n)()
        segs = (L.ApngSegment * n_chunks)()
        n_descs, n_segs, ws_bytes = C.c_int64(0), C.c_int64(0), C.c_int64(0)

        def host_decode():
            return clocked(lib, lambda: lib.vge_apng_decode(arr, n_files, args.threads, w, h, ct, n, out_h.data_ptr(),
                                                            status.ctypes.data, None, None))

        def plan():
            return clocked(lib, lambda: lib.vge_apng_plan_mem(
                raw.data_ptr(), int(raw.numel()), raw_off.ctypes.data, raw_size.ctypes.data, n_files, args.threads, w,
                h, ct, descs, n, C.byref(n_descs), segs, n_chunks, C.byref(n_segs), None, None, C.byref(ws_bytes)),
                also=lambda: n_descs.value == n)

        plan()
        descs_d = torch.frombuffer(descs, dtype=torch.uint8).to(dev)
        segs_d = torch.frombuffer(segs, dtype=torch.uint8).to(dev)
        ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=dev)
        status_d = torch.empty(n, dtype=torch.int32, device=dev)
        out_d = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)

        def device_call():
            L.check(lib.vge_apng_decode_device(raw_d.data_ptr(), int(raw_d.numel()), descs_d.data_ptr(), n,
                                               segs_d.data_ptr(), n_segs.value, n, n_files, w, h, ct, ws.data_ptr(),
                                               int(ws.numel()), out_d.data_ptr(), status_d.data_ptr(),
                                               stream.cuda_stream), "vge_apng_decode_device")

        def warm_e2e():
            e2e(paths, n, dev, args.threads, "host"); e2e(paths, n, dev, args.threads, "device")

        res = measure_calls(args, host_decode, plan, device_call, warm_e2e)
        assert int(status_d.abs().sum()) == 0
        calls_equal = bool(torch.equal(out_d.cpu(), out_h))
        # gather, inflate and adler run on what the call before left; unfilter rewrites its slot in place, so it is
        # timed together with the inflate that fills it, and compose on the pixels a whole call left
        for name, mask in (("gather", 1), ("inflate", 2), ("adler", 4), ("inflate_unfilter", 2 | 8), ("compose", 16)):
            if name == "compose":
                events(device_call)
            res[f"{name}_kernel_s"] = spread([staged(lib.vge_debug_apng_stage_mask, mask, 31, device_call)
                                              for _ in range(args.repeats)])
        routes_equal = measure_e2e(args, res, paths, n, dev)
        rect = np.array([[descs[k].w, descs[k].h] for k in range(n)])
        tmp.cleanup()
        return {
            "files": n_files, "frames": n, "width": w, "height": h, "color_type": ct,
            "apng_bytes_per_frame": float(raw_size.sum()) / n, "chunks_per_frame": n_chunks / n,
            "mean_rectangle": [float(rect[:, 0].mean()), float(rect[:, 1].mean())],
            **rates(res, n),
            "yardstick_host_decode_ms": 1e3 * res["host_decode_s"]["median"],
            "device_call_ms": 1e3 * res["device_call_s"]["median"],
            "device_call_over_host_decode": res["device_call_s"]["median"] / res["host_decode_s"]["median"],
            "e2e_device_over_e2e_host": res["e2e_device_s"]["median"] / res["e2e_host_s"]["median"],
            "device_equals_host": calls_equal and routes_equal,
        }

    return write_report(args, {
        "what": "vge.frames.load_videos on animated PNGs, both routes, measured on the GPU by tools/bench_frames.py "
                "--format apng",
        "device": torch.cuda.get_device_name(0), "threads": args.threads,
        "source": f"written here by Pillow (save_all): vge.synth.make_frames {args.size}x{args.size}; deltas: RGB, a "
                  "moving square over a fixed frame, cropped by Pillow; rgba: whole RGBA frames blended OVER",
        "deltas": one_kind("deltas"),
        "rgba": one_kind("rgba"),
    })


def _idat(data: bytes):
    """(offset, length) of a PNG file's IDAT payloads."""
    at, out = 8, []
    while at + 8 <= len(data):
        m, typ = int.from_bytes(data[at:at + 4], "big"), data[at + 4:at + 8]
        if typ == b"IDAT":
            out.append((at + 8, m))
        at += 12 + m
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--format", choices=("jpg", "png", "gif", "webp", "apng"), default="jpg")
    ap.add_argument("--gif-files", type=int, default=32,
                    help="--format gif / webp / apng: files the frames are spread over")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--folder", default=None)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=50, help="kernel launches per timed repeat")
    ap.add_argument("--entropy", choices=("host", "device"), default="host")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.format == "png":
        if args.out is None:
            args.out = str(REPO / "profiles" / "png_decode_device.json")
        return bench_png(args)
    if args.format == "gif":
        if args.out is None:
            args.out = str(REPO / "profiles" / "gif_decode_device.json")
        return bench_gif(args)
    if args.format == "webp":
        if args.out is None:
            args.out = str(REPO / "profiles" / "webp_decode_device.json")
        return bench_webp(args)
    if args.format == "apng":
        if args.out is None:
            args.out = str(REPO / "profiles" / "apng_decode_device.json")
        return bench_apng(args)
    if args.out is None:
        args.out = str(REPO / "profiles" / ("jpeg_decode.json" if args.entropy == "host" else "jpeg_decode_device.json"))

    import torch
    from vge import frames as FR
    from vge import lib as L
    dev = gpu()
    try:
        import PIL
        from PIL import Image
    except ImportError:
        PIL = None
    tmp = None
    if args.folder:
        src = FR.list_frames(args.folder)
        if not src:
            raise SystemExit(f"no *.jpg in {args.folder}")
        paths = [src[i % len(src)] for i in range(args.frames)]
        source = f"{len(src)} files of {args.folder}, cycled"
    else:
        if PIL is None:
            raise SystemExit("Pillow is not available: pass --folder with JPEG frames")
        tmp = tempfile.TemporaryDirectory()
        paths = write_jpegs(Path(tmp.name), args.frames, args.size, args.quality)
        source = f"written here: vge.synth.make_frames {args.size}x{args.size}, 4:2:0, quality {args.quality}"
    n = len(paths)
    info = FR.probe(paths[:1], args.threads)[0]
    lay = FR.make_layout(*[int(x) for x in info[:5]])
    lib = L.load()
    arr = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
    coef = torch.empty((n, lay.blocks_per_frame, 64), dtype=torch.int16, pin_memory=True)
    qtab = torch.empty((n, 3, 64), dtype=torch.int16, pin_memory=True)
    status = np.zeros(n, np.int32)
    out = torch.empty((n, lay.height, lay.width, 3), dtype=torch.uint8, device=dev)
    coef_d, qtab_d = torch.empty_like(coef, device=dev), torch.empty_like(qtab, device=dev)
    stream = torch.cuda.current_stream(dev)

    def entropy():
        return clocked(lib, lambda: lib.vge_jpeg_entropy_decode(arr, n, args.threads, C.byref(lay), coef.data_ptr(),
                                                                qtab.data_ptr(), status.ctypes.data))

    def upload():
        coef_d.copy_(coef, non_blocking=True)
        qtab_d.copy_(qtab, non_blocking=True)

    def kernel():
        L.check(lib.vge_jpeg_reconstruct(coef_d.data_ptr(), qtab_d.data_ptr(), C.byref(lay), n, out.data_ptr(),
                                         stream.cuda_stream), "vge_jpeg_reconstruct")

    def pillow():
        t = time.perf_counter()
        with ThreadPoolExecutor(args.threads) as ex:
            arrs = list(ex.map(lambda p: np.asarray(Image.open(p).convert("RGB")), paths))
        return time.perf_counter() - t, arrs

    res = {}
    for _ in range(args.warmup):
        entropy(); events(upload); events(kernel); e2e([paths], n, dev, args.threads, "host")
    res["entropy_s"] = spread([entropy() for _ in range(args.repeats)])
    res["upload_s"] = spread([events(upload) for _ in range(args.repeats)])
    res["kernel_s"] = spread([events(kernel, args.inner) for _ in range(args.repeats)])
    e = [e2e([paths], n, dev, args.threads, "host") for _ in range(args.repeats)]
    res["e2e_s"] = spread([t for t, _ in e])
    frames = e[-1][1]
    exact = None
    if PIL is not None:
        for _ in range(args.warmup):
            pillow()
        p = [pillow() for _ in range(args.repeats)]
        res["pillow_decode_s"] = spread([t for t, _ in p])
        exact = bool(np.array_equal(frames.cpu().numpy(), np.stack(p[-1][1])))
    device_rows = None
    if args.entropy == "device":
        raw, raw_off, raw_size = FR._read_files(paths, args.threads, pin=True)
        raw_d = raw.to(dev)
        nbytes = int(raw.numel())
        table = torch.from_numpy(np.stack([raw_off, raw_size])).to(dev)
        ws = torch.empty(int(lib.vge_jpeg_entropy_decode_workspace_bytes(C.byref(lay), n, nbytes)), dtype=torch.uint8,
                         device=dev)
        status_d = torch.empty(n, dtype=torch.int32, device=dev)
        rounds_d = torch.empty(n, dtype=torch.int32, device=dev)

        def read_upload():
            t = time.perf_counter()
            r, _, _ = FR._read_files(paths, args.threads, pin=True)
            r.to(dev, non_blocking=True)
            torch.cuda.synchronize()
            return time.perf_counter() - t

        def device_entropy():
            L.check(lib.vge_jpeg_entropy_decode_device(raw_d.data_ptr(), nbytes, table[0].data_ptr(),
                                                       table[1].data_ptr(), n,
                                                       C.byref(lay), ws.data_ptr(), coef_d.data_ptr(),
                                                       qtab_d.data_ptr(), status_d.data_ptr(), rounds_d.data_ptr(),
                                                       stream.cuda_stream), "vge_jpeg_entropy_decode_device")

        def prepare():   # the same call stopped after headers + scan preparation
            return staged(lib.vge_debug_jpeg_dehuff_prepare_only, 1, 0, device_entropy)

        for _ in range(args.warmup):
            read_upload(); events(device_entropy); prepare(); e2e([paths], n, dev, args.threads, "device")
        res["read_upload_s"] = spread([read_upload() for _ in range(args.repeats)])
        res["prepare_s"] = spread([prepare() for _ in range(args.repeats)])
        res["device_entropy_s"] = spread([events(device_entropy) for _ in range(args.repeats)])
        ed = [e2e([paths], n, dev, args.threads, "device") for _ in range(args.repeats)]
        res["e2e_device_s"] = spread([t for t, _ in ed])
        device_entropy()
        torch.cuda.synchronize()
        assert int(status_d.abs().sum()) == 0
        r = rounds_d.cpu().numpy()
        device_rows = {
            "file_bytes": nbytes, "rounds_mean": float(r.mean()), "rounds_max": int(r.max()),
            "decode_write_dc_s": res["device_entropy_s"]["median"] - res["prepare_s"]["median"],
            "subsequence_bytes": int(lib.vge_jpeg_entropy_decode_subsequence_bytes()),
            "tile_bytes": int(lib.vge_jpeg_entropy_decode_tile_bytes()),
            "equals_host_path": bool(torch.equal(ed[-1][1], frames)),
            "coefficients_equal_host": bool(torch.equal(coef_d.cpu(), coef) and torch.equal(qtab_d.cpu(), qtab)),
        }
    coef_b, tab_b, rgb_b = coef.numel() * 2, qtab.numel() * 2, out.numel()
    floor = (coef_b + tab_b + rgb_b) / HBM_ACHIEVABLE
    k = res["kernel_s"]["median"]
    report = {
        "what": "vge.frames.load_frames stages, measured on the GPU by tools/bench_frames.py",
        "device": torch.cuda.get_device_name(0), "frames": n, "width": lay.width, "height": lay.height,
        "sampling": f"{lay.h0}x{lay.v0}", "threads": args.threads, "source": source,
        "jpeg_bytes_per_frame": sum(os.path.getsize(p) for p in set(paths)) / len(set(paths)),
        "stages": res,
        "frames_per_s": {key[:-2]: n / v["median"] for key, v in res.items()},
        "kernel_bytes": {"coefficients": coef_b, "tables": tab_b, "rgb": rgb_b,
                         "per_frame": (coef_b + tab_b + rgb_b) / n},
        "kernel_hbm_floor_s": floor, "kernel_time_over_floor": k / floor,
        "kernel_bytes_per_s": (coef_b + tab_b + rgb_b) / k,
        "equals_pillow": exact if exact is not None else "not measured (Pillow not importable)",
        "pillow": getattr(PIL, "__version__", None),
    }
    if device_rows is not None:
        report["device_entropy"] = device_rows
    if tmp is not None:
        tmp.cleanup()
    return write_report(args, report)


if __name__ == "__main__":
    raise SystemExit(main())
