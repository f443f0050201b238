"""Training the scorer on one MI355X: the reference's optimiser loop (train.py:433-524) on the device data path.

  window_variants   the three hard-negative variants of a batch (utils.py:65-95) from one shuffle table
  loss_components   train.py:511-524: TCL + hard_weight x SupConWithHardNegatives against the shuffled, reversed and
                    static windows (four module forwards)
  train_step        train.py:491-507: one optimiser step; a non-finite loss skips it without touching the optimiser
                    or the scheduler
  train             BaseExperiment.__init__'s data path (validate.build_data_path) once, PKBatchSampler over the train
                    split's windows, AdamW + CosineAnnealingLR, and per epoch the held-out loss (validate_checkpoint,
                    with the module's weights loaded into the hand-written forward), the best-checkpoint rule
                    (train.py:450-455) and the centroid distance
  python -m vge.train   the command line; prints the per-epoch records as JSON lines

What runs where.  Featurise, the time gathers, the two losses with their gradients and the per-epoch validation are
this library's HIP kernels.  The module's forward and backward (vge.model.HumanActionScorer) and the optimiser run on
torch's kernels: the hand-written encoder keeps no activations and has no backward.  With conv_backend="hip" the
residual blocks of the movement encoders run on vge_convblock.hip's forward and backward kernels instead
(vge.convblock), and with time_backend="hip" the layers of the temporal stack run on vge_timelayer.hip's
(vge.timelayer); with linear_backend="hip" the stems and projections run on vge_linear.hip's (vge.linear) and with
fusion_backend="hip" the per-modality LayerNorm and the fusion on vge_fusion.hip's (vge.fusion).  All four default to
"torch" and are independent of each other.

Differences from the reference, all deliberate: the sampler is seeded (default_rng(seed); the reference's is not), the
shuffle tables come from a CPU generator seeded with `seed` rather than torch's global one, dropout masks come from
this process's RNG stream, evaluate_human_corr is not run inside the loop (run python -m vge.eval on the saved
checkpoint), checkpoints carry their hyper-parameters next to the state dict (eval.py:136-160 reads both forms), and
one GPU trains (no DataParallel).
"""
from __future__ import annotations

import json
import math
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .lib import UnsupportedModelError
from .losses import TCL, SupConWithHardNegatives
from .model import HumanActionScorer
from .validate import (build_data_path, partial_shuffle_indices, reverse_indices, static_indices,
                       validate_checkpoint)


def window_variants(feats: torch.Tensor, shuffle_table: torch.Tensor) -> List[torch.Tensor]:
    """-> [shuffled, reversed, static] windows of feats [B,32,D].  Device tensors go through ops.time_gather; CPU
    tensors (the host tests) through torch.gather with the same tables."""
    B, T, D = feats.shape
    tables = (shuffle_table.to(torch.int32), reverse_indices(B, T), static_indices(B, T))
    if feats.is_cuda:
        return [ops.time_gather(feats, t.to(feats.device)) for t in tables]
    return [torch.gather(feats, 1, t.long().unsqueeze(-1).expand(-1, -1, D)) for t in tables]


def loss_components(model, tcl, hard, feats, variants: Sequence[torch.Tensor], labels, hard_weight: float = 10.0):
    """-> the four loss terms in COMPONENTS order (weights applied), as scalar tensors with autograd history."""
    emb = model(feats)[0]
    negs = [model(v)[0] for v in variants]
    return [tcl(emb, labels)] + [hard_weight * hard(emb, emb, n) for n in negs]


def train_step(model, optimizer, scheduler, tcl, hard, feats, variants, labels, hard_weight: float = 10.0):
    """One step of train_one_epoch -> (stepped, [tcl, hard_shuf, hard_rev, hard_stat] as floats).  A non-finite sum
    leaves the parameters, the optimiser state and the scheduler untouched (train.py:499-500)."""
    comps = loss_components(model, tcl, hard, feats, variants, labels, hard_weight)
    total = comps[0] + comps[1] + comps[2] + comps[3]
    vals = torch.stack([c.detach().double() for c in comps]).cpu().tolist()     # the step's one device-to-host copy
    if not math.isfinite(sum(vals)):
        return False, vals
    optimizer.zero_grad()
    total.backward()
    optimizer.step()
    scheduler.step()
    return True, vals


def make_optimizer(model, lr: float, steps_per_epoch: int, epochs: int):
    """AdamW(lr) and CosineAnnealingLR(T_max = steps_per_epoch x epochs, eta_min 1e-6) (train.py:162-186)."""
    opt = torch.optim.AdamW(list(model.parameters()), lr=lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=max(1, steps_per_epoch) * epochs, eta_min=1e-6)
    return opt, sched


def checkpoint_dict(model: HumanActionScorer) -> dict:
    return {"model_state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()},
            **model.hyper_parameters}


# ----------------------------------------------------------------------------- per-epoch validation

class ModuleEncoder:
    """ops.Encoder's interface (what validate_checkpoint and build_real_centroids call) over the torch module, in eval
    mode and without autograd: the encoder of the per-epoch validation for a checkpoint shape the kernels refuse."""

    def __init__(self, model: HumanActionScorer, layout: str):
        self.model, self.layout = model, layout
        self.d_model = model.hyper_parameters["d_model"]
        self.feat_dim = sum(model.dims_raw.values()) + sum(model.dims_diff.values())

    def reserve(self, max_windows: int) -> None:
        pass

    def status(self) -> None:
        pass

    @torch.no_grad()
    def encode(self, feats, frame_embed: bool = False, tc: bool = True, seq_out=None, tc_out=None):
        was_training = self.model.training
        self.model.eval()
        try:
            seq, fe, _ = self.model(feats)
        finally:
            self.model.train(was_training)
        if seq_out is not None:
            seq = seq_out.copy_(seq)
        tcw = None
        if tc:          # vge_tc_windows: mean_t || f[t+1] - f[t] || over the frame rows (CLS dropped)
            tcw = (fe[:, 2:] - fe[:, 1:-1]).norm(dim=-1).mean(dim=1)
            if tc_out is not None:
                tcw = tc_out.copy_(tcw)
        return seq.contiguous(), (fe if frame_embed else None), tcw


def validate_module(model: HumanActionScorer, dp, real_meshes_dir, real_kp_dir, clip_len=32, stride=8, batch=2048,
                    seed=1337, compute="f32x3", hard_weight=10.0) -> dict:
    """The held-out loss and centroid distance of the module's current weights (train.py:439-458): the state dict is
    loaded into an ops.Encoder -- the hand-written forward -- with centroids from the train split.  -> the keys of
    validate_checkpoint plus "validated_by": "kernels", or "module" with "kernels_refused" when the kernels refuse
    the shape and the torch module encodes instead."""
    from . import eval as E
    dev = dp.windows.device
    extra = {"validated_by": "kernels"}
    try:
        enc = E.load_model((model.numpy_state_dict(), model.hyper_parameters), dp.dims_raw, dp.dims_diff, device=dev,
                           compute=compute)
    except UnsupportedModelError as e:
        enc = ModuleEncoder(model, dp.stats.layout)
        extra = {"validated_by": "module", "kernels_refused": str(e)}
    centroids, _, _ = E.build_real_centroids(enc, real_meshes_dir, real_kp_dir, dp.stats, clip_len, stride, dev,
                                             train_items=dp.train_ds.items, label_dict=dp.label_dict,
                                             store=dp.train_store)
    out = validate_checkpoint(enc, dp.test_store, dp.windows, dp.labels, dp.stats, centroids=centroids, batch=batch,
                              generator=torch.Generator().manual_seed(seed), hard_weight=hard_weight,
                              label_dict=dp.label_dict)
    out.update(extra)
    return out


# ----------------------------------------------------------------------------- the loop

def train(real_meshes_dir: str, real_kp_dir: Optional[str], save_dir: str, epochs: int = 30, lr: float = 3e-4,
          P: int = 10, K: int = 24, clip_len: int = 32, stride: int = 8, seed: int = 1337, dropout: float = 0.1,
          hard_weight: float = 10.0, eval_batch: int = 2048, ingest: str = "host", device="cuda",
          loss_backend: str = "hip", model_kwargs: Optional[dict] = None, compute: str = "f32x3",
          init_state_dict: Optional[dict] = None, log=None, conv_backend: str = "torch",
          time_backend: str = "torch", linear_backend: str = "torch", fusion_backend: str = "torch") -> List[dict]:
    """Exp_TCL_Hard_V2Plus.run (train.py:433-467) -> one record per epoch: {"epoch", "train_loss", "steps",
    "skipped_steps", "lr", "eval_loss", "components", "n_batches", "skipped_batches", "centroid_distance",
    "class_distances", "validated_by", "conv_backend", "time_backend", "linear_backend", "fusion_backend", "checkpoint" (the file written this epoch, or None)}.  save_dir receives
    label_mapping.json once and best_eval_epoch{e:03d}_loss{loss:.4f}.pt whenever the held-out loss improves.
    model_kwargs: d_model / time_layers / time_heads of another shape; init_state_dict: initial weights."""
    from . import eval as E
    from .data import PKBatchSampler, sample_all_windows_npz
    os.makedirs(save_dir, exist_ok=True)
    torch.manual_seed(seed)                      # the module's initial weights and its dropout masks
    dev = torch.device(device)
    dp = build_data_path(real_meshes_dir, real_kp_dir, clip_len, stride, dev, ingest)
    with open(os.path.join(save_dir, "label_mapping.json"), "w") as f:
        json.dump(dp.label_dict, f, indent=2)
    samples = sample_all_windows_npz(dp.train_ds, clip_len, stride)
    idx = {it.path: i for i, it in enumerate(dp.train_ds.items)}
    train_windows = E._window_tensor(samples, idx, dev)
    label_list = [dp.label_dict[it.cls] for it, _ in samples]
    train_labels = torch.as_tensor(label_list, dtype=torch.int32, device=dev)
    sampler = PKBatchSampler(label_list, P=P, K=K, drop_last=True, generator=np.random.default_rng(seed))

    model = HumanActionScorer(dp.dims_raw, dp.dims_diff, dropout=dropout, conv_backend=conv_backend,
                              time_backend=time_backend, linear_backend=linear_backend,
                              fusion_backend=fusion_backend, **(model_kwargs or {}))
    if init_state_dict is not None:
        model.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in init_state_dict.items()})
    model.to(dev).train()
    tcl, hard = TCL(backend=loss_backend), SupConWithHardNegatives(backend=loss_backend)
    optimizer, scheduler = make_optimizer(model, lr, len(sampler), epochs)
    shuffle_gen = torch.Generator().manual_seed(seed)
    best, records = float("inf"), []
    for epoch in range(epochs):
        total, steps, skipped = 0.0, 0, 0
        for batch in sampler:
            b = torch.as_tensor(batch, dtype=torch.long, device=dev)
            feats = ops.featurize(dp.train_store, train_windows[b], dp.stats.mean, dp.stats.std,
                                  layout=dp.stats.layout)
            variants = window_variants(feats, partial_shuffle_indices(len(batch), clip_len, generator=shuffle_gen))
            stepped, vals = train_step(model, optimizer, scheduler, tcl, hard, feats, variants, train_labels[b],
                                       hard_weight)
            if stepped:
                total += sum(vals)
                steps += 1
            else:
                skipped += 1
        rec = {"epoch": epoch + 1, "train_loss": total / max(1, len(sampler)), "steps": steps,
               "skipped_steps": skipped, "lr": float(scheduler.get_last_lr()[0]), "conv_backend": conv_backend,
               "time_backend": time_backend, "linear_backend": linear_backend, "fusion_backend": fusion_backend}
        val = validate_module(model, dp, real_meshes_dir, real_kp_dir, clip_len, stride, eval_batch, seed, compute,
                              hard_weight)
        rec["eval_loss"] = val.pop("loss")
        rec.update(val)
        rec["checkpoint"] = None
        if rec["eval_loss"] < best:
            best = rec["eval_loss"]
            path = os.path.join(save_dir, f"best_eval_epoch{epoch + 1:03d}_loss{best:.4f}.pt")
            torch.save(checkpoint_dict(model), path)
            rec["checkpoint"] = path
        records.append(rec)
        if log is not None:
            log(rec)
    return records


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m vge.train",
                                 description="train the scorer (train.py's Exp_TCL_Hard_V2Plus) on one MI355X")
    ap.add_argument("real_meshes")
    ap.add_argument("--real-kp", default=None,
                    help="real keypoint dir; omit for the keypoint-less 4-modality layout (keypoint_dir None)")
    ap.add_argument("--kp-layout", default=None, choices=["auto", "flat", "per_class"])
    ap.add_argument("--save-dir", required=True)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("-P", type=int, default=10, help="classes per batch")
    ap.add_argument("-K", type=int, default=24, help="windows per class")
    ap.add_argument("--clip-len", type=int, default=32)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1337)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--hard-weight", type=float, default=10.0)
    ap.add_argument("--eval-batch", type=int, default=2048)
    ap.add_argument("--ingest", default="host", choices=["host", "device"])
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--loss-backend", default="hip", choices=["hip", "torch"])
    ap.add_argument("--conv-backend", default="torch", choices=["torch", "hip"],
                    help="the movement encoders' residual blocks: torch ops, or the forward / backward HIP kernels")
    ap.add_argument("--time-backend", default="torch", choices=["torch", "hip"],
                    help="the temporal stack's layers: torch's nn.TransformerEncoder, or the forward / backward HIP kernels")
    ap.add_argument("--linear-backend", default="torch", choices=["torch", "hip"],
                    help="the movement encoders' stems and projections: torch matmuls, or the forward / backward HIP kernels")
    ap.add_argument("--fusion-backend", default="torch", choices=["torch", "hip"],
                    help="the per-modality LayerNorm and the fusion: torch ops, or the forward / backward HIP kernels")
    ap.add_argument("--d-model", type=int, default=256)
    ap.add_argument("--time-layers", type=int, default=4)
    ap.add_argument("--time-heads", type=int, default=8)
    a = ap.parse_args(argv)
    if a.kp_layout is not None:
        if a.real_kp is None:
            ap.error("a keypoint layout was given without its keypoint directory")
        from .data import set_keypoint_layout
        set_keypoint_layout(a.kp_layout, a.real_kp)
    train(a.real_meshes, a.real_kp, a.save_dir, epochs=a.epochs, lr=a.lr, P=a.P, K=a.K, clip_len=a.clip_len,
          stride=a.stride, seed=a.seed, dropout=a.dropout, hard_weight=a.hard_weight, eval_batch=a.eval_batch,
          ingest=a.ingest, device=a.device, loss_backend=a.loss_backend, conv_backend=a.conv_backend, time_backend=a.time_backend,
          linear_backend=a.linear_backend, fusion_backend=a.fusion_backend,
          model_kwargs={"d_model": a.d_model, "time_layers": a.time_layers, "time_heads": a.time_heads},
          log=lambda rec: print(json.dumps(rec), flush=True))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
