#!/usr/bin/env python3
"""Disk-to-HBM ingest, host route against device route, on one GPU.

Both routes go from files in the page cache to a frame store resident in HBM:

  host     vge.ingest.load_frame_store_native (zlib on host threads, pinned) + ops.DeviceFrameStore.from_host
  device   vge.ingest.load_device_frame_store (raw bytes uploaded, inflated by csrc/vge_inflate.hip)
  sidecar  vge.ingest.load_sidecar + from_host, for scale (no zlib at all; needs a first run over the same set)

on two synthetic sets (vge.synth: random floats, which deflate by only about 8 %; real extractor output compresses and
matches more): the config-4 shape (300 generated videos of 32-128 frames + 80 real ones) and N clips of 32 frames,
also cut down to smaller sizes to find where the routes cross.  After a warm-up the routes alternate; every figure is
the median over the repeats with the spread beside it.  The device route is also split into file read, plan, upload
and kernel (device events).  One JSON document goes to --out and its summary line to stdout.

    python tools/bench_ingest.py [--threads 16] [--reps 5] [--clips 4096] [--out profiles/ingest_device.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_ingest.py --device-only     (kernel time, a run of its own)
    python tools/bench_ingest.py --merge-rocprof DIR --out profiles/ingest_device.json
"""
import argparse
import csv
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "video-gen-evals_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vge import ingest, ops, synth  # noqa: E402
from vge.data import NpzVideoDataset, create_dataset_from_generated_meshes  # noqa: E402

N_GEN, T_GEN = 300, (32, 48, 64, 96, 128, 40, 72)       # bench_tag.py's config-4 set
N_REAL_PER_CLASS, T_REAL = 8, (64, 48, 96)
UNIQUE_CLIPS = 512                                      # the 32-frame set repeats this many distinct clips


def write_clips(work: Path, n: int, threads: int):
    """n clips of 32 frames in the generated layout; clip i's content is that of clip i % UNIQUE_CLIPS."""
    gen, kps = work / "clips" / "generated_meshes", work / "clips" / "generated_kps"
    gen.mkdir(parents=True, exist_ok=True)

    def one(i):
        name = synth.generated_name(i)
        c = synth.make_clip(synth.SEED_GEN, i, 32)
        synth.save_clip_npz(gen / f"{name}.npz", c)
        (kps / name).mkdir(parents=True, exist_ok=True)
        np.save(kps / name / "keypoints.npy", c.keypoints)

    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(one, range(min(n, UNIQUE_CLIPS))))
    for i in range(UNIQUE_CLIPS, n):
        src, name = synth.generated_name(i % UNIQUE_CLIPS), synth.generated_name(i) + f"_{i}"
        shutil.copyfile(gen / f"{src}.npz", gen / f"{name}.npz")
        (kps / name).mkdir(parents=True, exist_ok=True)
        shutil.copyfile(kps / src / "keypoints.npy", kps / name / "keypoints.npy")
    return create_dataset_from_generated_meshes(str(gen)).items, str(kps)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def measure(name, groups, dev, threads, reps, work):
    """groups: [(items, keypoint dir, require_kp)] loaded one after the other, as a flow does."""
    n = sum(len(g[0]) for g in groups)
    mb = sum(os.path.getsize(it.path) for g in groups for it in g[0]) / 1e6

    def host():
        return [ops.DeviceFrameStore.from_host(ingest.load_frame_store_native(it, kd, rq, threads=threads), dev)
                for it, kd, rq in groups]

    def device(tm=None):
        return [ingest.load_device_frame_store(it, kd, rq, dev, threads=threads,
                                               timings=None if tm is None else tm.setdefault(i, {}))
                for i, (it, kd, rq) in enumerate(groups)]

    sides = []
    for i, (it, kd, rq) in enumerate(groups):
        p = work / f"{name}_{i}.vgefs"
        ingest.save_sidecar(ingest.load_frame_store_native(it, kd, rq, threads=threads, pinned=False), str(p))
        sides.append(str(p))

    def sidecar():
        return [ops.DeviceFrameStore.from_host(ingest.load_sidecar(p), dev) for p in sides]

    a, b = host(), device()                                   # warm-up, and the two routes agree
    for x, y in zip(a, b):
        assert torch.equal(x.vit, y.vit) and torch.equal(x.pose, y.pose) and torch.equal(x.videos, y.videos)
    sidecar()
    del a, b
    t = {"host": [], "device": [], "sidecar": []}
    stages = {"read_s": [], "plan_s": [], "upload_ms": [], "kernel_ms": []}
    for _ in range(reps):
        t["host"].append(timed(host, dev)[0])
        t["device"].append(timed(device, dev)[0])
        t["sidecar"].append(timed(sidecar, dev)[0])
        tm = {}
        device(tm)
        for k in stages:
            stages[k].append(sum(v[k] for v in tm.values()))
    row = {"set": name, "videos": n, "compressed_MB": round(mb, 2)}
    for k, v in t.items():
        s = spread(v)
        row[k] = {"seconds": s, "clips_per_s": round(n / s["median"], 1), "compressed_MB_per_s": round(mb / s["median"], 1)}
    row["device_stages"] = {k: spread(v) for k, v in stages.items()}
    row["device_speedup_over_host"] = round(statistics.median(t["host"]) / statistics.median(t["device"]), 3)
    print(json.dumps({"set": name, "clips_per_s": {k: row[k]["clips_per_s"] for k in t}}), flush=True)
    return row


def merge_rocprof(d, out):
    rows = []
    for p in Path(d).rglob("*kernel_stats.csv"):
        with open(p) as f:
            rows += [r for r in csv.DictReader(f) if "inflate_kernel" in r.get("Name", "") or "convert_kernel" in r.get("Name", "")]
    doc = json.loads(Path(out).read_text()) if Path(out).exists() else {}
    doc["rocprofv3_kernel_stats"] = [{k: r[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs")
                                      if k in r} for r in rows]
    Path(out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc["rocprofv3_kernel_stats"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 512])
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ingest_device.json"))
    ap.add_argument("--device-only", action="store_true", help="three device-route loads of the config-4 set, no timing")
    ap.add_argument("--merge-rocprof", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.merge_rocprof:
        return merge_rocprof(a.merge_rocprof, a.out)
    dev = torch.device("cuda:0")
    work = Path(a.dir or tempfile.mkdtemp(prefix="vge_bench_ingest_"))
    paths = {k: str(work / "cfg4" / k) for k in ("real", "real_kp", "generated_meshes", "generated_kps")}
    if not (work / "cfg4" / "written").exists():
        synth.write_dataset(str(work / "cfg4"), n_real_per_class=N_REAL_PER_CLASS, n_gen=N_GEN, T_real=T_REAL,
                            T_gen=T_GEN, kp_short_every=7)
        (work / "cfg4" / "written").write_text("1")
    print("config-4 set written", flush=True)
    gen = sorted(create_dataset_from_generated_meshes(paths["generated_meshes"]).items, key=lambda it: it.path)
    real = NpzVideoDataset(paths["real"]).items
    cfg4 = [(real, paths["real_kp"], False), (gen, paths["generated_kps"], True)]
    if a.device_only:
        for _ in range(3):
            for it, kd, rq in cfg4:
                ingest.load_device_frame_store(it, kd, rq, dev, threads=a.threads)
        torch.cuda.synchronize(dev)
        return
    clips, clip_kps = write_clips(work, a.clips, a.threads)
    print("32-frame clips written", flush=True)
    rows = [measure("config4_300gen_80real", cfg4, dev, a.threads, a.reps, work)]
    for n in sorted(set(a.sizes + [a.clips])):
        rows.append(measure(f"clips32_{n}", [(clips[:n], clip_kps, True)], dev, a.threads, a.reps, work))
    doc = {"tool": "tools/bench_ingest.py", "gpu": torch.cuda.get_device_name(0), "threads": a.threads, "reps": a.reps,
           "data": "vge.synth (random floats: deflate saves about 8 %; real extractor output compresses and matches more); "
                   f"the 32-frame set repeats {UNIQUE_CLIPS} distinct clips",
           "routes": "files in the page cache -> frame store in HBM", "sets": rows}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({r["set"]: {k: r[k]["clips_per_s"] for k in ("host", "device", "sidecar")} for r in rows}))
    if a.dir is None:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
