"""Checkpoint selection on libvge: the held-out loss the reference's training loop ranks checkpoints by.

  partial_shuffle_indices / reverse_indices / static_indices
                          utils.py:65-95 (partial_shuffle_within_window, reverse_sequence, get_static_window) as
                          int32 [B,T] source-index tables for ops.time_gather
  validate_checkpoint     train.py:286-333 (evaluate_test_set with Exp_TCL_Hard_V2Plus.compute_loss_components,
                          train.py:511-524: TCL + 10 x SupConWithHardNegatives against shuffled, reversed and static
                          windows) and train.py:335-399 (evaluate_test_set_centroid_distance)
  rank_checkpoints        BaseExperiment.__init__'s data path (train.py:117-128) once, then every checkpoint through
                          validate_checkpoint; train.py:450-455 keeps the checkpoint with the lowest loss
  python -m vge.validate  the command line

  build_data_path         that data path by itself: vge.train builds its loop on it

This module is the forward side: the optimiser loop that minimises this loss is vge.train, the gradients of the two
losses are vge.losses (vge_tcl_loss_grad / vge_hardneg_loss_grad), the batch sampler is data.PKBatchSampler.  The batches
run on one GPU; sharding them over ranks is out of scope (a batch's TCL couples all of its windows, so the unit of
work is a whole batch -- a few per checkpoint).
"""
from __future__ import annotations

import json
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .lib import UnsupportedModelError

COMPONENTS = ("tcl", "hard_shuf", "hard_rev", "hard_stat")
TCL_TEMPERATURE, TCL_K1, TCL_K2 = 0.1, 5000.0, 1.0   # TCL() defaults (losses.py:7)
HARD_TEMPERATURE = 0.07                               # SupConWithHardNegatives() default (losses.py:38)


# ----------------------------------------------------------------------------- index tables

def reverse_indices(B: int, T: int = 32) -> torch.Tensor:
    """reverse_sequence (utils.py:78-86): src[b,t] = T-1-t."""
    return torch.arange(T - 1, -1, -1, dtype=torch.int32).repeat(B, 1)


def static_indices(B: int, T: int = 32) -> torch.Tensor:
    """get_static_window (utils.py:88-95): every frame is the window's first."""
    return torch.zeros((B, T), dtype=torch.int32)


def partial_shuffle_indices(B: int, T: int = 32, shuffle_fraction: float = 0.7,
                            generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """partial_shuffle_within_window (utils.py:65-75) as a source-index table: per window, in the reference's order,
    idx = randperm(T)[:n], p = randperm(n), src[idx[j]] = idx[p[j]], identity elsewhere.  The draws come from the CPU
    generator exactly as the reference's (generator None: torch's global one, so torch.manual_seed(s) reproduces the
    reference's tables)."""
    src = torch.arange(T, dtype=torch.int32).repeat(B, 1)
    if T > 1:
        n = max(1, int(shuffle_fraction * T))
        for b in range(B):
            idx = torch.randperm(T, generator=generator)[:n]
            p = torch.randperm(n, generator=generator)
            src[b, idx] = idx[p].to(torch.int32)
    return src


# ----------------------------------------------------------------------------- one checkpoint

def _reduce_batches(batch_losses: Sequence[Sequence[float]]) -> dict:
    """evaluate_test_set's bookkeeping (train.py:294-333) over per-batch component values in COMPONENTS order: a
    batch whose sum is not finite adds to neither the total, the components nor n_batches."""
    total, comp, n, skipped = 0.0, dict.fromkeys(COMPONENTS, 0.0), 0, 0
    for vals in batch_losses:
        s = float(sum(vals))
        if not math.isfinite(s):
            skipped += 1
            continue
        total += s
        for k, v in zip(COMPONENTS, vals):
            comp[k] += float(v)
        n += 1
    if n == 0:
        return {"loss": float("inf"), "components": {}, "n_batches": 0, "skipped_batches": skipped}
    return {"loss": total / n, "components": {k: v / n for k, v in comp.items()}, "n_batches": n,
            "skipped_batches": skipped}


def validate_checkpoint(model: ops.Encoder, store: ops.DeviceFrameStore, windows: torch.Tensor, labels: torch.Tensor,
                        stats, centroids: Optional[torch.Tensor] = None, batch: int = 2048,
                        shuffle_tables: Optional[Sequence[torch.Tensor]] = None,
                        generator: Optional[torch.Generator] = None, hard_weight: float = 10.0,
                        label_dict: Optional[Dict[str, int]] = None) -> dict:
    """evaluate_test_set (train.py:286-333) of one checkpoint over `windows` (device int32 [N,2], the
    enumerate_test_windows order of make_test_loader) with `labels` (device int32 [N]), in batches of `batch`
    consecutive windows: featurise once, encode, gather + encode the shuffled / reversed / static variants (two
    feature buffers), then TCL and the three hard-negative terms.  A batch whose sum is not finite is skipped as the
    reference does.  shuffle_tables: one int32 [b,32] table per batch instead of drawing them (generator: the CPU
    generator of the draw, None = torch's global one).

    -> {"loss", "components", "n_batches", "skipped_batches"} and, with `centroids` [C,d],
    {"centroid_distance", "class_distances"} (train.py:383-396; class_distances keyed by label_dict's class names
    when given, else by label).  One GPU; the batches are not sharded over ranks."""
    n = int(windows.shape[0])
    dev = windows.device
    if model.layout != stats.layout:
        raise ValueError(f"model takes the {model.layout!r} feature layout but the stats are {stats.layout!r}")
    if labels.dtype != torch.int32 or labels.numel() != n:
        raise ValueError("validate_checkpoint: labels must be int32 [N]")
    n_batches = (n + batch - 1) // batch
    if shuffle_tables is not None and len(shuffle_tables) != n_batches:
        raise ValueError(f"validate_checkpoint: {len(shuffle_tables)} shuffle tables for {n_batches} batches")
    cap = min(batch, max(n, 1))
    model.reserve(cap)
    d = model.d_model
    feats = torch.empty((cap, 32, model.feat_dim), device=dev)
    var = torch.empty_like(feats)
    emb = torch.empty((cap, d), device=dev)
    neg = torch.empty((cap, d), device=dev)
    all_emb = torch.empty((n, d), device=dev) if centroids is not None else None
    losses = torch.empty((4,), device=dev, dtype=torch.float64)
    rev, stat = reverse_indices(cap).to(dev), static_indices(cap).to(dev)
    per_batch: List[List[float]] = []
    for k, b0 in enumerate(range(0, n, batch)):
        b1 = min(n, b0 + batch)
        b = b1 - b0
        if shuffle_tables is not None:
            shuf = torch.as_tensor(shuffle_tables[k], dtype=torch.int32)
            if tuple(shuf.shape) != (b, 32):
                raise ValueError(f"validate_checkpoint: shuffle table {k} must be [{b}, 32]")
        else:
            shuf = partial_shuffle_indices(b, 32, generator=generator)
        f = ops.featurize(store, windows[b0:b1], stats.mean, stats.std, out=feats[:b], layout=stats.layout)
        e, _, _ = model.encode(f, tc=False, seq_out=emb[:b])
        if all_emb is not None:
            all_emb[b0:b1] = e
        ops.tcl_loss(e, labels[b0:b1], TCL_TEMPERATURE, TCL_K1, TCL_K2, out=losses[0:1])
        for slot, table in ((1, shuf.to(dev)), (2, rev[:b]), (3, stat[:b])):
            v = ops.time_gather(f, table, out=var[:b])
            ne, _, _ = model.encode(v, tc=False, seq_out=neg[:b])
            ops.hardneg_loss(e, ne, HARD_TEMPERATURE, out=losses[slot:slot + 1])
        vals = losses.cpu().tolist()      # the batch's four scalars: one small device-to-host copy
        per_batch.append([vals[0]] + [hard_weight * x for x in vals[1:]])
    out = _reduce_batches(per_batch)
    if centroids is not None and n:
        dist = ops.centroid_distance(all_emb, labels, centroids).cpu().numpy()
        lab = labels.cpu().numpy()
        keep = ~np.isnan(dist)            # labels outside the centroid table (train.py:373-374)
        out["centroid_distance"] = float(np.mean(dist[keep].astype(np.float64))) if keep.any() else float("inf")
        names = {i: c for c, i in label_dict.items()} if label_dict is not None else {}
        out["class_distances"] = {str(names.get(int(c), int(c))): float(dist[lab == c].mean(dtype=np.float32))
                                  for c in np.unique(lab[keep])}
    torch.cuda.synchronize(dev)
    model.status()
    return out


# ----------------------------------------------------------------------------- the data path

@dataclass
class DataPath:
    """BaseExperiment.__init__'s data path (train.py:117-128), built once: what rank_checkpoints and vge.train share."""
    train_ds: object
    test_ds: object
    label_dict: Dict[str, int]
    train_store: ops.DeviceFrameStore
    stats: object
    dims_raw: Dict[str, int]
    dims_diff: Dict[str, int]
    test_store: ops.DeviceFrameStore
    windows: torch.Tensor           # the held-out split's windows, device int32 [N,2] (enumerate_test_windows order)
    labels: torch.Tensor            # their labels, device int32 [N]


def build_data_path(real_meshes_dir: str, real_kp_dir: Optional[str], clip_len: int = 32, stride: int = 8,
                    device="cuda", ingest: str = "host") -> DataPath:
    """NpzVideoDataset over the ten classes, train_test_split(0.8, 1337), stats from the train split, label_dict
    from the sorted classes of the full set; both frame stores on the device."""
    from . import eval as E
    from .data import ACTION_CLASSES, NpzVideoDataset, enumerate_test_windows, train_test_split
    real_ds = NpzVideoDataset(real_meshes_dir, filter_classes=ACTION_CLASSES)
    train_ds, test_ds = train_test_split(real_ds, train_ratio=0.8, seed=1337)
    label_dict = {cls: i for i, cls in enumerate(sorted({it.cls for it in real_ds.items}))}
    train_store = E.device_frame_store(train_ds.items, real_kp_dir, False, device, ingest)
    stats = E.compute_stats_from_npz(train_ds.items, real_kp_dir, device=device, store=train_store)
    dims_raw, dims_diff = E.infer_dims_from_stats(stats)
    test_store = E.device_frame_store(test_ds.items, real_kp_dir, real_kp_dir is not None, device, ingest)
    samples = enumerate_test_windows(test_ds, clip_len, stride)
    idx = {it.path: i for i, it in enumerate(test_ds.items)}
    windows = E._window_tensor(samples, idx, device)
    labels = torch.as_tensor([label_dict[it.cls] for it, _ in samples], dtype=torch.int32, device=device)
    return DataPath(train_ds, test_ds, label_dict, train_store, stats, dims_raw, dims_diff, test_store, windows,
                    labels)


# ----------------------------------------------------------------------------- many checkpoints

def rank_checkpoints(real_meshes_dir: str, real_kp_dir: Optional[str], checkpoints: Sequence, compute: str = "f32x3",
                     seed: int = 1337, batch: int = 2048, clip_len: int = 32, stride: int = 8,
                     device="cuda", ingest: str = "host") -> List[dict]:
    """Rank checkpoints by the held-out loss.  The data path is BaseExperiment.__init__'s (train.py:117-128):
    NpzVideoDataset over the ten classes, train_test_split(0.8, 1337), stats from the train split, label_dict from
    the sorted classes of the full set.  Stats, both frame stores and the window / label tensors are built once;
    each checkpoint is then loaded (load_model), its centroids built from the train split (build_real_centroids) and
    validated on the test split, with the CPU generator seeded afresh (`seed`) so that all checkpoints see the same
    shuffles.  A checkpoint whose shape the kernels refuse (UnsupportedModelError) is reported with its error and
    ranked last.  -> a list of {"checkpoint", "loss", ...validate_checkpoint's keys} sorted by loss.  One GPU; the
    batches are not sharded over ranks."""
    from . import eval as E
    dp = build_data_path(real_meshes_dir, real_kp_dir, clip_len, stride, device, ingest)
    train_ds, label_dict, train_store, stats = dp.train_ds, dp.label_dict, dp.train_store, dp.stats
    dims_raw, dims_diff = dp.dims_raw, dp.dims_diff
    test_store, windows, labels = dp.test_store, dp.windows, dp.labels
    results = []
    for ck in checkpoints:
        entry = {"checkpoint": str(ck) if not isinstance(ck, (dict, tuple)) else f"<state_dict {len(results)}>"}
        try:
            model = E.load_model(ck, dims_raw, dims_diff, device=device, compute=compute)
            centroids, _, _ = E.build_real_centroids(model, real_meshes_dir, real_kp_dir, stats, clip_len, stride,
                                                     device, train_items=train_ds.items, label_dict=label_dict,
                                                     store=train_store)
            gen = torch.Generator().manual_seed(seed)
            entry.update(validate_checkpoint(model, test_store, windows, labels, stats, centroids=centroids,
                                             batch=batch, generator=gen, label_dict=label_dict))
        except UnsupportedModelError as e:
            entry.update(loss=float("inf"), error=str(e))
        results.append(entry)
    # unsupported checkpoints last; among the rest the lowest loss first (ties keep the order given)
    results.sort(key=lambda r: ("error" in r, r["loss"] if not math.isnan(r["loss"]) else float("inf")))
    return results


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m vge.validate",
                                 description="rank checkpoints by the held-out loss (train.py:286-333) on an MI355X")
    ap.add_argument("--real-meshes", required=True)
    ap.add_argument("--real-kp", default=None,
                    help="real keypoint dir; omit for the keypoint-less 4-modality layout (keypoint_dir None)")
    ap.add_argument("--kp-layout", default=None, choices=["auto", "flat", "per_class"],
                    help="layout of --real-kp (as vge.eval's --real-kp-layout; default: VGE_KP_LAYOUT or auto)")
    ap.add_argument("--compute", default="f32x3", choices=["f32x3", "f32", "f16"])
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--seed", type=int, default=1337)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default="ranking.json")
    ap.add_argument("--ingest", default="host", choices=["host", "device"],
                    help="where the npz archives are inflated: host threads (default) or the GPU")
    ap.add_argument("checkpoints", nargs="+", metavar="CKPT")
    a = ap.parse_args(argv)
    if a.kp_layout is not None:
        if a.real_kp is None:
            ap.error("a keypoint layout was given without its keypoint directory")
        from .data import set_keypoint_layout
        set_keypoint_layout(a.kp_layout, a.real_kp)
    ranking = rank_checkpoints(a.real_meshes, a.real_kp, a.checkpoints, compute=a.compute, seed=a.seed,
                               batch=a.batch, device=a.device, ingest=a.ingest)
    for rank, r in enumerate(ranking, 1):
        if "error" in r:
            print(f"{rank:3d}  {r['checkpoint']}  unsupported: {r['error']}")
        else:
            comp = "  ".join(f"{k} {v:.4f}" for k, v in r["components"].items())
            cd = f"  centroid_distance {r['centroid_distance']:.4f}" if "centroid_distance" in r else ""
            print(f"{rank:3d}  {r['checkpoint']}  loss {r['loss']:.6f}  {comp}  batches {r['n_batches']} "
                  f"(+{r['skipped_batches']} skipped){cd}")
    with open(a.out, "w") as f:
        json.dump(ranking, f, indent=2)
    print(f"Saved the ranking of {len(ranking)} checkpoints to {a.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
