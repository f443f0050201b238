#!/usr/bin/env python3
"""Time one training step (vge.train's, train.py:488-524) piece by piece with hipEvents: P x K = 240 windows over the
config-2 synthetic set (256 synthetic 32-frame clips, one window each), d_model 256, dropout 0.1, after a warm-up.
Prints one JSON object and nothing else.

    python tools/bench_train.py

ms are medians over the timed repetitions.  Per repetition the pieces of one step are timed in order -- featurise,
the three time gathers, the four module forwards, the loss forward + backward (to the gradients of the four
embeddings), the module's backward, the optimiser step -- once with the HIP loss and once with the torch loss, in
alternating order; "step" is vge.train.train_step as the loop calls it (its device-to-host copy of the four loss
values included).  "loss_2048" is the loss pair alone (TCL + three hard-negative terms, forward + backward) at
B = 2048 on unit embeddings of ten classes."""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "video-gen-evals_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vge import ops, synth, train as T, validate as V  # noqa: E402
from vge.data import pack_frame_store  # noqa: E402
from vge.losses import TCL, SupConWithHardNegatives  # noqa: E402
from vge.model import HumanActionScorer  # noqa: E402

P, K, CLIPS, WARMUP, REPS = 10, 24, 256, 3, 15
BACKENDS = ("hip", "torch")
PIECES = ("featurize", "gathers", "forwards", "loss_fwd_bwd", "module_backward", "optimizer", "pieces_total", "step")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    return (a, b), out


def loss_pair(tcl, hard, emb, negs, labels):
    total = tcl(emb, labels) + 10.0 * (hard(emb, emb, negs[0]) + hard(emb, emb, negs[1]) + hard(emb, emb, negs[2]))
    return total, torch.autograd.grad(total, [emb] + list(negs))


def main():
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
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
    B = P * K
    win = torch.tensor([[i % CLIPS, 0] for i in range(B)], dtype=torch.int32, device=dev)
    labels = torch.tensor([i % P for i in range(B)], dtype=torch.int32, device=dev)
    dims_raw = dict(zip(ops.MODALITIES, ops.DIMS_RAW))
    dims_diff = dict(zip(ops.MODALITIES, ops.DIMS_DIFF))
    model = HumanActionScorer(dims_raw, dims_diff, dropout=0.1).to(dev).train()
    opt, sched = T.make_optimizer(model, 3e-4, 100, 30)
    losses = {b: (TCL(backend=b), SupConWithHardNegatives(backend=b)) for b in BACKENDS}
    gen = torch.Generator().manual_seed(1337)
    tables = [V.partial_shuffle_indices(B, 32, generator=gen).to(dev), V.reverse_indices(B).to(dev),
              V.static_indices(B).to(dev)]
    times = {b: {k: [] for k in PIECES} for b in BACKENDS}
    values = {}
    for rep in range(WARMUP + REPS):
        for backend in (BACKENDS if rep % 2 == 0 else BACKENDS[::-1]):
            tcl, hard = losses[backend]
            ev = {}
            ev["featurize"], feats = timed(lambda: ops.featurize(store, win, mean, std))
            ev["gathers"], variants = timed(lambda: [ops.time_gather(feats, t) for t in tables])
            ev["forwards"], embs = timed(lambda: [model(x)[0] for x in [feats] + variants])
            ev["loss_fwd_bwd"], (total, grads) = timed(lambda: loss_pair(tcl, hard, embs[0], embs[1:], labels))
            opt.zero_grad()
            ev["module_backward"], _ = timed(lambda: torch.autograd.backward(embs, grads))
            ev["optimizer"], _ = timed(lambda: (opt.step(), sched.step()))
            ev["step"], (stepped, vals) = timed(lambda: T.train_step(model, opt, sched, tcl, hard, feats, variants,
                                                                     labels))
            torch.cuda.synchronize(dev)
            assert stepped
            values[backend] = float(total.detach())
            if rep < WARMUP:
                continue
            for k, (a, b) in ev.items():
                times[backend][k].append(a.elapsed_time(b))
            times[backend]["pieces_total"].append(ev["featurize"][0].elapsed_time(ev["optimizer"][1]))
    out = {"windows": B, "d_model": 256, "dropout": 0.1, "reps": REPS,
           "parameters": int(sum(p.numel() for p in model.parameters()))}
    for backend in BACKENDS:
        ms = {k: statistics.median(v) for k, v in times[backend].items()}
        out[backend] = {k + "_ms": round(v, 4) for k, v in ms.items()}
        out[backend]["loss_share_of_pieces"] = round(ms["loss_fwd_bwd"] / ms["pieces_total"], 5)
        out[backend]["last_loss"] = values[backend]
    out["loss_hip_over_torch_240"] = round(out["hip"]["loss_fwd_bwd_ms"] / out["torch"]["loss_fwd_bwd_ms"], 4)

    # the loss pair alone at B = 2048
    Bl = 2048
    g = torch.Generator().manual_seed(5)
    lab = torch.tensor([i % 10 for i in range(Bl)], dtype=torch.int32, device=dev)
    base = torch.randn(10, 256, generator=g)
    mk = lambda s: torch.nn.functional.normalize(base[lab.cpu().long()] + s * torch.randn(Bl, 256, generator=g),  # noqa: E731
                                                 dim=-1).to(dev).requires_grad_(True)
    emb, negs = mk(0.6), [mk(0.7), mk(0.8), mk(0.9)]
    t2048 = {b: [] for b in BACKENDS}
    for rep in range(WARMUP + REPS):
        for backend in (BACKENDS if rep % 2 == 0 else BACKENDS[::-1]):
            e, _ = timed(lambda: loss_pair(*losses[backend], emb, negs, lab))
            torch.cuda.synchronize(dev)
            if rep >= WARMUP:
                t2048[backend].append(e[0].elapsed_time(e[1]))
    out["loss_2048"] = {b + "_ms": round(statistics.median(v), 4) for b, v in t2048.items()}
    out["loss_hip_over_torch_2048"] = round(out["loss_2048"]["hip_ms"] / out["loss_2048"]["torch_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
