#!/usr/bin/env python3
"""Time one checkpoint's validation batch (vge.validate's flow, train.py:286-333) piece by piece with hipEvents:
2,048 windows over the config-2 synthetic set (256 synthetic 32-frame clips, one window each, repeated to fill the
batch), after a warm-up.  Prints one JSON object and nothing else.

    python tools/bench_validate.py

ms are medians over the timed repetitions; "encodes" is the four encoder passes of the batch, "gathers" the three
time_gather calls (with their achieved bytes per second: one read and one write of the batch each), "losses" the TCL
and the three hard-negative kernels."""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "video-gen-evals_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vge import ops, synth, validate as V  # noqa: E402
from vge.data import pack_frame_store  # noqa: E402

WINDOWS, CLIPS, WARMUP, REPS = 2048, 256, 2, 7


def main():
    dev = torch.device("cuda", 0)
    clips, names = [], []
    for i in range(CLIPS):
        c = synth.make_clip(synth.SEED_GEN, 10_000 + i, 32)
        clips.append({"pose": c.pose, "global_orient": c.global_orient, "betas": c.betas, "vit": c.vit,
                      "keypoints": c.keypoints})
        names.append(synth.generated_name(10_000 + i))
    store = ops.DeviceFrameStore.from_host(pack_frame_store(clips, names, ["X"] * CLIPS), dev)
    rng = np.random.default_rng(0)
    mean = torch.from_numpy(rng.normal(0, 0.1, ops.FEAT_DIM).astype(np.float32)).to(dev)
    std = torch.from_numpy(rng.uniform(0.5, 2.0, ops.FEAT_DIM).astype(np.float32)).to(dev)
    win = torch.tensor([[i % CLIPS, 0] for i in range(WINDOWS)], dtype=torch.int32, device=dev)
    labels = torch.tensor([i % 10 for i in range(WINDOWS)], dtype=torch.int32, device=dev)
    enc = ops.Encoder(synth.make_state_dict(synth.DIMS_RAW, synth.DIMS_DIFF), device=dev, compute="f32x3")
    enc.reserve(WINDOWS)
    feats = ops.featurize(store, win, mean, std)
    var = torch.empty_like(feats)
    emb = torch.empty((WINDOWS, enc.d_model), device=dev)
    neg = torch.empty_like(emb)
    losses = torch.empty((4,), device=dev, dtype=torch.float64)
    tables = [V.partial_shuffle_indices(WINDOWS, 32, generator=torch.Generator().manual_seed(1337)).to(dev),
              V.reverse_indices(WINDOWS).to(dev), V.static_indices(WINDOWS).to(dev)]
    times = {"encodes": [], "gathers": [], "losses": [], "tcl": [], "batch": []}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    for rep in range(WARMUP + REPS):
        ev = {k: [] for k in times}
        t0 = torch.cuda.Event(enable_timing=True)
        t0.record()
        ev["encodes"].append(timed(lambda: enc.encode(feats, tc=False, seq_out=emb)))
        ev["tcl"].append(timed(lambda: ops.tcl_loss(emb, labels, out=losses[0:1])))
        for k, t in enumerate(tables):
            ev["gathers"].append(timed(lambda: ops.time_gather(feats, t, out=var)))
            ev["encodes"].append(timed(lambda: enc.encode(var, tc=False, seq_out=neg)))
            ev["losses"].append(timed(lambda: ops.hardneg_loss(emb, neg, out=losses[k + 1:k + 2])))
        t1 = torch.cuda.Event(enable_timing=True)
        t1.record()
        torch.cuda.synchronize(dev)
        if rep < WARMUP:
            continue
        ev["losses"] += ev["tcl"]
        for k in ("encodes", "gathers", "losses", "tcl"):
            times[k].append(sum(a.elapsed_time(b) for a, b in ev[k]))
        times["batch"].append(t0.elapsed_time(t1))
    enc.status()
    ms = {k: statistics.median(v) for k, v in times.items()}
    gather_bytes = 3 * 2 * feats.numel() * 4
    print(json.dumps({
        "windows": WINDOWS, "compute": "f32x3", "reps": REPS,
        "encodes_ms": round(ms["encodes"], 4), "gathers_ms": round(ms["gathers"], 4),
        "losses_ms": round(ms["losses"], 4), "tcl_ms": round(ms["tcl"], 4), "batch_ms": round(ms["batch"], 4),
        "gather_gb_per_s": round(gather_bytes / (ms["gathers"] * 1e-3) / 1e9, 1),
        "gathers_share_of_encodes": round(ms["gathers"] / ms["encodes"], 4),
        "losses_share_of_encodes": round(ms["losses"] / ms["encodes"], 4),
        "loss_values": [float(x) for x in losses.cpu()],
    }))


if __name__ == "__main__":
    main()
