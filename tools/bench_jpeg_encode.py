"""Frames per second of vge.frames.jpeg_roundtrip and save_frames on frames in device memory, beside Pillow.

    python tools/bench_jpeg_encode.py [--frames 1024] [--size 256] [--quality 95] [--threads 16]
                                      [--out profiles/jpeg_encode.json]

The frames are vge.synth.make_frames content (as tools/bench_frames.py uses), 4:2:0.  Needs a GPU: there is no fallback.

Stages, each warmed up and repeated, reported as median [min, max] over the repeats:
  forward    vge_jpeg_forward, --inner launches per repeat                           (device events / launches)
  roundtrip  jpeg_roundtrip(frames, out=...): forward + table expansion + reconstruct (device events / calls)
  download   the coefficients into pinned host memory                                (device events)
  huffman    vge_jpeg_entropy_encode on --threads host threads, into a temporary     (host clock)
             folder
  save       save_frames(frames, folder) end to end                                  (host clock)
  pillow     PIL encode + decode of the same frames in memory on --threads threads   (host clock; when Pillow imports)
The round trip's algorithmic traffic is 3 B/pixel read + the coefficients written, then the coefficients read + 3 B/pixel
written; its HBM floor is that over 6.3 TB/s (the achievable rate of a float4 copy).
"""
from __future__ import annotations

import argparse
import ctypes as C
import io
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


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=50, help="kernel launches per timed repeat")
    ap.add_argument("--out", default=str(REPO / "profiles" / "jpeg_encode.json"))
    args = ap.parse_args(argv)

    import torch
    from vge import frames as FR
    from vge import lib as L
    from vge import synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_encode.py needs a GPU")
    dev = torch.device("cuda:0")
    try:
        import PIL
        from PIL import Image
    except ImportError:
        PIL = None
    n, size = args.frames, args.size
    host = np.concatenate([synth.make_frames(1000 + v, min(64, n - 64 * v), h=size, w=size)
                           for v in range((n + 63) // 64)])
    frames = torch.from_numpy(host).to(dev)
    lib = L.load()
    lay = FR.make_layout(size, size, 3, 2, 2)
    qtab_h = FR.quant_tables(args.quality)
    qtab = torch.from_numpy(qtab_h.view(np.int16)).to(dev)
    coef = torch.empty((n, lay.blocks_per_frame, 64), dtype=torch.int16, device=dev)
    coef_h = torch.empty(coef.shape, dtype=torch.int16, pin_memory=True)
    out = torch.empty_like(frames)
    stream = torch.cuda.current_stream(dev)
    tmp = tempfile.TemporaryDirectory()
    paths = [os.path.join(tmp.name, f"frame_{i:06d}.jpg") for i in range(n)]
    arr = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
    sizes = np.zeros(n, np.int64)

    def events(fn, inner=1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3 / inner

    def forward():
        L.check(lib.vge_jpeg_forward(frames.data_ptr(), C.byref(lay), n, qtab.data_ptr(), coef.data_ptr(),
                                     stream.cuda_stream), "vge_jpeg_forward")

    def roundtrip():
        FR.jpeg_roundtrip(frames, quality=args.quality, out=out)

    def download():
        coef_h.copy_(coef, non_blocking=True)

    def huffman():
        t = time.perf_counter()
        rc = lib.vge_jpeg_entropy_encode(coef_h.data_ptr(), qtab_h.ctypes.data, C.byref(lay), n, args.threads, arr,
                                         sizes.ctypes.data, None)
        dt = time.perf_counter() - t
        assert rc == 0, lib.vge_last_error()
        return dt

    def save():
        t = time.perf_counter()
        FR.save_frames(frames, tmp.name, quality=args.quality, threads=args.threads)
        return time.perf_counter() - t

    def pillow_one(a):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="JPEG", quality=args.quality, subsampling=2)
        return np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))

    def pillow():
        t = time.perf_counter()
        with ThreadPoolExecutor(args.threads) as ex:
            arrs = list(ex.map(pillow_one, host))
        return time.perf_counter() - t, arrs

    res = {}
    for _ in range(args.warmup):
        events(forward); events(roundtrip); events(download); huffman(); save()
    res["forward_s"] = spread([events(forward, args.inner) for _ in range(args.repeats)])
    res["roundtrip_s"] = spread([events(roundtrip, args.inner) for _ in range(args.repeats)])
    res["download_s"] = spread([events(download) for _ in range(args.repeats)])
    res["huffman_s"] = spread([huffman() for _ in range(args.repeats)])
    res["save_s"] = spread([save() for _ in range(args.repeats)])
    exact = None
    if PIL is not None:
        for _ in range(args.warmup):
            pillow()
        p = [pillow() for _ in range(args.repeats)]
        res["pillow_encode_decode_s"] = spread([t for t, _ in p])
        exact = bool(np.array_equal(out.cpu().numpy(), np.stack(p[-1][1])))
    rgb_b, coef_b = frames.numel(), coef.numel() * 2
    traffic = 2 * (rgb_b + coef_b)
    floor = traffic / HBM_ACHIEVABLE
    k = res["roundtrip_s"]["median"]
    report = {
        "what": "vge.frames.jpeg_roundtrip / save_frames stages, measured on the GPU by tools/bench_jpeg_encode.py",
        "device": torch.cuda.get_device_name(0), "frames": n, "width": size, "height": size, "sampling": "2x2",
        "quality": args.quality, "threads": args.threads,
        "source": f"vge.synth.make_frames {size}x{size}",
        "jpeg_bytes_per_frame": float(sizes.mean()),
        "stages": res,
        "frames_per_s": {key[:-2]: n / v["median"] for key, v in res.items()},
        "roundtrip_bytes": {"rgb": rgb_b, "coefficients": coef_b, "algorithmic": traffic, "per_frame": traffic / n},
        "roundtrip_hbm_floor_s": floor, "roundtrip_time_over_floor": k / floor, "roundtrip_bytes_per_s": traffic / k,
        "forward_bytes_per_s": (rgb_b + coef_b) / res["forward_s"]["median"],
        "huffman_share_of_save": res["huffman_s"]["median"] / res["save_s"]["median"],
        "equals_pillow": exact if exact is not None else "not measured (Pillow not importable)",
        "pillow": getattr(PIL, "__version__", None),
    }
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))
    tmp.cleanup()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
