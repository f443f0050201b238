"""Frames per second of vge.frames.jpeg_roundtrip, save_frames and encode_frames on frames in device memory, beside
Pillow.

    python tools/bench_jpeg_encode.py [--frames 1024] [--size 256] [--quality 95] [--threads 16]
                                      [--out profiles/jpeg_encode.json]
                                      [--entropy-out profiles/jpeg_entropy_device.json] [--only-entropy]

The frames are vge.synth.make_frames content (as tools/bench_frames.py uses), 4:2:0.  Needs a GPU: there is no fallback.

Stages, each warmed up and repeated, reported as median [min, max] over the repeats:
  forward    vge_jpeg_forward, --inner launches per repeat                           (device events / launches)
  roundtrip  jpeg_roundtrip(frames, out=...): forward + table expansion + reconstruct (device events / calls)
  download   the coefficients into pinned host memory                                (device events)
  huffman    vge_jpeg_entropy_encode on --threads host threads, into a temporary     (host clock)
             folder
  save       save_frames(frames, folder) end to end                                  (host clock)
  pillow     PIL encode + decode of the same frames in memory on --threads threads   (host clock; when Pillow imports)
The device entropy coder (csrc/vge_jpeg_huff.hip) against the host coder of the same build, into --entropy-out:
  plan, emit     vge_jpeg_entropy_plan / vge_jpeg_entropy_emit, --inner launches per repeat  (device events / launches)
  files_copy     the finished files into pinned host memory                                  (device events)
  encode_frames  end to end, entropy "host" and "device" alternating                         (host clock)
  save_frames    end to end, "host" and "device" at --threads and at 2 threads, alternating  (host clock)
  one 1920x1080 frame alone: plan, emit, encode_frames host and device
Every timed output is compared byte for byte with the host coder's.  The algorithmic traffic of plan + emit is counted
from the shapes and the file sizes (the coefficients read twice, the bits per block written and read, the unstuffed scan
written once and read twice, the files written); its HBM floor is that over 6.3 TB/s.
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
    ap.add_argument("--entropy-out", default=str(REPO / "profiles" / "jpeg_entropy_device.json"))
    ap.add_argument("--only-entropy", action="store_true", help="skip the stages that go to --out")
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

    def read_all(folder):
        return [open(os.path.join(folder, f"frame_{i:06d}.jpg"), "rb").read() for i in range(n)]

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, r

    def entropy_stages(fr, layout, inner):
        """plan / emit by device events and encode_frames by the host clock for the frames `fr`; every output is
        compared with the host coder's bytes."""
        F = int(fr.shape[0])
        cf = torch.empty((F, layout.blocks_per_frame, 64), dtype=torch.int16, device=dev)
        L.check(lib.vge_jpeg_forward(fr.data_ptr(), C.byref(layout), F, qtab.data_ptr(), cf.data_ptr(),
                                     stream.cuda_stream), "vge_jpeg_forward")
        ws = torch.empty(int(lib.vge_jpeg_entropy_workspace_bytes(C.byref(layout), F)), dtype=torch.uint8, device=dev)
        sz_d = torch.empty(F, dtype=torch.int64, device=dev)
        st_d = torch.empty(F, dtype=torch.int32, device=dev)

        def plan():
            L.check(lib.vge_jpeg_entropy_plan(cf.data_ptr(), C.byref(layout), F, ws.data_ptr(), sz_d.data_ptr(),
                                              st_d.data_ptr(), stream.cuda_stream), "vge_jpeg_entropy_plan")
        plan()
        sz = sz_d.cpu().numpy()
        assert not st_d.cpu().numpy().any()
        offs = np.concatenate([[0], np.cumsum(sz)]).astype(np.int64)
        off_d = torch.from_numpy(offs[:F]).to(dev)
        files_d = torch.empty(int(offs[F]), dtype=torch.uint8, device=dev)
        files_h = torch.empty(int(offs[F]), dtype=torch.uint8, pin_memory=True)

        def emit():
            L.check(lib.vge_jpeg_entropy_emit(ws.data_ptr(), qtab.data_ptr(), C.byref(layout), F, off_d.data_ptr(),
                                              files_d.data_ptr(), int(offs[F]), stream.cuda_stream),
                    "vge_jpeg_entropy_emit")

        def copy():
            files_h.copy_(files_d, non_blocking=True)
        for _ in range(args.warmup):
            events(plan); events(emit); events(copy)
            FR.encode_frames(fr, args.quality, entropy="host", threads=args.threads)
            FR.encode_frames(fr, args.quality, entropy="device")
        r = {"plan_s": spread([events(plan, inner) for _ in range(args.repeats)]),
             "emit_s": spread([events(emit, inner) for _ in range(args.repeats)]),
             "files_copy_s": spread([events(copy) for _ in range(args.repeats)])}
        th, td, same = [], [], True
        want, want_off = FR.encode_frames(fr, args.quality, entropy="host", threads=args.threads)
        same &= bool(np.array_equal(want_off.numpy(), offs)) and torch.equal(files_h, want)
        for _ in range(args.repeats):       # the two alternate in the same run
            t, (d, o) = clock(lambda: FR.encode_frames(fr, args.quality, entropy="host", threads=args.threads))
            th.append(t)
            same &= torch.equal(d, want) and torch.equal(o, want_off)
            t, (d, o) = clock(lambda: FR.encode_frames(fr, args.quality, entropy="device"))
            td.append(t)
            same &= torch.equal(d, want) and torch.equal(o, want_off)
        r["encode_frames_host_s"], r["encode_frames_device_s"] = spread(th), spread(td)
        coef_b, blocks = cf.numel() * 2, F * layout.blocks_per_frame
        scan_b = int(offs[F]) - F * (623 + 2)          # an upper bound: it counts the stuffed 00 bytes too
        traffic = 2 * coef_b + 2 * 2 * blocks + 3 * scan_b + int(offs[F])
        k = r["plan_s"]["median"] + r["emit_s"]["median"]
        return {"frames": F, "width": layout.width, "height": layout.height, "blocks_per_frame": layout.blocks_per_frame,
                "segments_per_frame": -(-layout.blocks_per_frame // lib.vge_jpeg_entropy_segment_blocks()),
                "workspace_bytes": ws.numel(), "file_bytes": int(offs[F]), "coefficient_bytes": coef_b,
                "stages": r, "equal_to_host_coder": bool(same),
                "plan_emit_bytes": traffic, "plan_emit_hbm_floor_s": traffic / HBM_ACHIEVABLE,
                "plan_emit_bytes_per_s": traffic / k, "plan_emit_time_over_floor": k / (traffic / HBM_ACHIEVABLE),
                "encode_frames_host_over_device": r["encode_frames_host_s"]["median"]
                / r["encode_frames_device_s"]["median"]}

    def entropy_report():
        rep = {"what": "the device entropy coder (vge_jpeg_entropy_plan / _emit) against the host coder of the same "
                       "build, measured on the GPU by tools/bench_jpeg_encode.py",
               "device": torch.cuda.get_device_name(0), "quality": args.quality, "sampling": "2x2",
               "source": "vge.synth.make_frames", "batch": entropy_stages(frames, lay, args.inner)}
        tmp_h, tmp_d = tempfile.TemporaryDirectory(), tempfile.TemporaryDirectory()
        saves, same = {}, True
        combos = [(th, e) for th in (args.threads, 2) for e in ("host", "device")]
        for th, e in combos:
            for _ in range(args.warmup):
                FR.save_frames(frames, (tmp_h if e == "host" else tmp_d).name, quality=args.quality, threads=th, entropy=e)
        times = {c: [] for c in combos}
        for _ in range(args.repeats):       # all four alternate in the same run
            for th, e in combos:
                folder = (tmp_h if e == "host" else tmp_d).name
                t, _ = clock(lambda: FR.save_frames(frames, folder, quality=args.quality, threads=th, entropy=e))
                times[(th, e)].append(t)
            same &= read_all(tmp_h.name) == read_all(tmp_d.name)
        for th in (args.threads, 2):
            h, d = spread(times[(th, "host")]), spread(times[(th, "device")])
            saves[f"threads_{th}"] = {"host_s": h, "device_s": d, "host_over_device": h["median"] / d["median"]}
        rep["save_frames"] = saves
        rep["save_frames_files_equal"] = bool(same)
        tmp_h.cleanup(); tmp_d.cleanup()
        one = torch.from_numpy(synth.make_frames(77, 1, h=1080, w=1920)).to(dev)
        rep["one_1920x1080"] = entropy_stages(one, FR.make_layout(1920, 1080, 3, 2, 2), args.inner)
        Path(args.entropy_out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.entropy_out, "w") as f:
            json.dump(rep, f, indent=1)
        print(json.dumps(rep))

    if args.only_entropy:
        entropy_report()
        tmp.cleanup()
        return 0
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
    entropy_report()
    tmp.cleanup()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
