#!/usr/bin/env python3
"""Time one training step (vge.train's, train.py:488-524) piece by piece with hipEvents: P x K = 240 windows over the
config-2 synthetic set (256 synthetic 32-frame clips, one window each), d_model 256, dropout 0.1, after a warm-up.
Prints one JSON object and nothing else.

    python tools/bench_train.py [--conv-backend hip] [--time-backend hip] [--linear-backend hip] [--fusion-backend hip]

ms are medians over the timed repetitions.  Per repetition the pieces of one step are timed in order -- featurise,
the three time gathers, the four module forwards, the loss forward + backward (to the gradients of the four
embeddings), the module's backward, the optimiser step -- once with the HIP loss and once with the torch loss, in
alternating order; "step" is vge.train.train_step as the loop calls it (its device-to-host copy of the four loss
values included).  "loss_2048" is the loss pair alone (TCL + three hard-negative terms, forward + backward) at
B = 2048 on unit embeddings of ten classes.

--conv-backend hip adds a third column, "conv_hip": the same step with the movement encoders' residual blocks on the
forward / backward kernels of vge_convblock.hip (a second module with the same initial weights and its own optimiser,
HIP loss), alternated with the two existing columns in the same repetitions; and "convblock_240", one block alone
(B = 240, T = 32, C = 256; events around 20 calls) with its FLOPs over the time against the 155 TFLOP/s the f32-input
MFMA was measured at.  Without the flag the output is what it was.

--time-backend hip adds the column "time_hip" in the same way: the same step with the temporal stack's layers on the
forward / backward kernels of vge_timelayer.hip (conv blocks on torch, HIP loss), alternated with the other columns in
the same repetitions; and "timelayer_240", one layer alone (B = 240, S = 33, D = 256, 8 heads, dropout 0.1; events
around 10 calls) on the kernels and as torch's own layer under autograd, forward and backward.

--linear-backend hip and --fusion-backend hip add the columns "linear_hip" (stems and projections on vge_linear.hip)
and "fusion_hip" (the per-modality LayerNorm and the fusion on vge_fusion.hip); given together they add
"linear_fusion_hip" with both, and with all four backend flags on hip the column "all_hip".  --fusion-backend hip also
adds "fusion_240", the fusion node alone (R = 240 x 32, M = 5, D = 256, dropout 0.1; events around 10 calls) on the
kernels and as the module's _Fusion behind F.layer_norm under autograd, forward and backward."""
import argparse
import copy
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


MFMA_F32_TFLOPS = 155.0      # v_mfma_f32_16x16x4_f32 / 32x32x2, measured back-to-back issue rate on an MI355X


def convblock_alone(dev, B=240, Tn=32, Cn=256, calls=20):
    """One block's forward and backward alone -> ms per call, TFLOP/s, and the share of the f32-MFMA ceiling."""
    g = torch.Generator().manual_seed(11)
    x, dy = (torch.randn(B, Tn, Cn, generator=g).to(dev) for _ in range(2))
    w1, w2 = (torch.randn(Cn, Cn, 5, generator=g).div_((5 * Cn) ** 0.5).to(dev) for _ in range(2))
    gamma, beta = torch.ones(Cn, device=dev), torch.zeros(Cn, device=dev)
    mask = torch.nn.functional.dropout(torch.ones_like(x), 0.1, True)
    conv_flop = 2.0 * B * Tn * 5 * Cn * Cn           # one dilated k = 5 convolution, or one weight gradient
    out = {}
    for dil in (1, 8):
        _, saved = ops.convblock_forward(x, w1, w2, gamma, beta, dil, mask)
        fwd, bwd = [], []
        for rep in range(WARMUP + REPS):
            e, _ = timed(lambda: [ops.convblock_forward(x, w1, w2, gamma, beta, dil, mask) for _ in range(calls)])
            f, _ = timed(lambda: [ops.convblock_backward(dy, x, w1, w2, gamma, dil, saved, mask) for _ in range(calls)])
            torch.cuda.synchronize(dev)
            if rep >= WARMUP:
                fwd.append(e[0].elapsed_time(e[1]) / calls)
                bwd.append(f[0].elapsed_time(f[1]) / calls)
        for name, ms, flop in (("forward", statistics.median(fwd), 2 * conv_flop),
                               ("backward", statistics.median(bwd), 4 * conv_flop)):
            tf = flop / (ms * 1e-3) / 1e12
            out[f"{name}_dil{dil}"] = {"ms": round(ms, 4), "gflop": round(flop / 1e9, 3), "tflops": round(tf, 2),
                                       "share_of_f32_mfma_ceiling": round(tf / MFMA_F32_TFLOPS, 4)}
    return out


def timelayer_alone(dev, B=240, S=33, D=256, H=8, calls=10):
    """One temporal layer's forward and backward alone, on the kernels and as torch's layer -> ms per call, and the
    kernels' TFLOP/s over the 12 D^2 weights' GEMMs (forward 2, backward 4 FLOP per weight and row)."""
    from torch.nn.attention import SDPBackend, sdpa_kernel
    from vge import timelayer as TL
    torch.manual_seed(3)
    layer = torch.nn.TransformerEncoderLayer(D, H, 4 * D, 0.1, batch_first=True).to(dev).train()
    params = tuple(p.detach() for p in TL.layer_params(layer))
    x, dy = torch.randn(B, S, D, device=dev), torch.randn(B, S, D, device=dev)
    masks = TL.draw_masks(x, H, 4 * D, 0.1)
    _, saved = ops.timelayer_forward(x, params, H, masks)
    xr = x.clone().requires_grad_(True)
    t = {k: [] for k in ("hip_forward", "hip_backward", "torch_forward", "torch_backward")}
    for rep in range(WARMUP + REPS):
        ev = {}
        ev["hip_forward"], _ = timed(lambda: [ops.timelayer_forward(x, params, H, masks) for _ in range(calls)])
        ev["hip_backward"], _ = timed(lambda: [ops.timelayer_backward(dy, x, params, H, saved, masks)
                                               for _ in range(calls)])
        with sdpa_kernel(SDPBackend.MATH):
            ev["torch_forward"], ys = timed(lambda: [layer(xr) for _ in range(calls)])
            ev["torch_backward"], _ = timed(lambda: [torch.autograd.grad(y, [xr] + list(layer.parameters()), dy)
                                                     for y in ys])
        torch.cuda.synchronize(dev)
        if rep >= WARMUP:
            for k, (a, b) in ev.items():
                t[k].append(a.elapsed_time(b) / calls)
    out = {k + "_ms": round(statistics.median(v), 4) for k, v in t.items()}
    gemm_flop = 2.0 * B * S * 12 * D * D
    for k, flop in (("hip_forward", gemm_flop), ("hip_backward", 2 * gemm_flop)):
        tf = flop / (out[k + "_ms"] * 1e-3) / 1e12
        out[k + "_tflops"] = round(tf, 2)
        out[k + "_share_of_f32_mfma_ceiling"] = round(tf / MFMA_F32_TFLOPS, 4)
    out["hip_over_torch_forward"] = round(out["hip_forward_ms"] / out["torch_forward_ms"], 4)
    out["hip_over_torch_backward"] = round(out["hip_backward_ms"] / out["torch_backward_ms"], 4)
    return out


def fusion_alone(dev, R=240 * 32, M=5, D=256, calls=10):
    """The fusion node's forward and backward alone, on the kernels and as torch's graph -> ms per call."""
    import torch.nn.functional as F
    from vge import fusion as FU
    from vge.model import _Fusion
    torch.manual_seed(4)
    mod = _Fusion(D, M, 0.1).to(dev).train()
    params = tuple(p.detach().reshape(D) if i == 0 else p.detach() for i, p in enumerate(FU.fusion_params(mod)))
    s, dy = torch.randn(R, M, D, device=dev), torch.randn(R, D, device=dev)
    m_attn = F.dropout(torch.ones(R, M, device=dev), 0.1, True)
    _, saved = ops.fusion_forward(s, params, m_attn)
    sr = s.view(240, R // 240, M, D).clone().requires_grad_(True)          # _Fusion takes [B,T,M,D]
    dyr = dy.view(240, R // 240, D)
    t = {k: [] for k in ("hip_forward", "hip_backward", "torch_forward", "torch_backward")}
    for rep in range(WARMUP + REPS):
        ev = {}
        ev["hip_forward"], _ = timed(lambda: [ops.fusion_forward(s, params, m_attn) for _ in range(calls)])
        ev["hip_backward"], _ = timed(lambda: [ops.fusion_backward(dy, s, params, saved, m_attn) for _ in range(calls)])
        ev["torch_forward"], ys = timed(lambda: [mod(F.layer_norm(sr, (D,))) for _ in range(calls)])
        ev["torch_backward"], _ = timed(lambda: [torch.autograd.grad(y, [sr] + list(mod.parameters()), dyr) for y in ys])
        torch.cuda.synchronize(dev)
        if rep >= WARMUP:
            for k, (a, b) in ev.items():
                t[k].append(a.elapsed_time(b) / calls)
    out = {k + "_ms": round(statistics.median(v), 4) for k, v in t.items()}
    out["hip_over_torch_forward"] = round(out["hip_forward_ms"] / out["torch_forward_ms"], 4)
    out["hip_over_torch_backward"] = round(out["hip_backward_ms"] / out["torch_backward_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conv-backend", default="torch", choices=["torch", "hip"],
                    help="hip: add the conv_hip column (residual blocks on vge_convblock.hip) and convblock_240")
    ap.add_argument("--time-backend", default="torch", choices=["torch", "hip"],
                    help="hip: add the time_hip column (temporal layers on vge_timelayer.hip) and timelayer_240")
    ap.add_argument("--linear-backend", default="torch", choices=["torch", "hip"],
                    help="hip: add the linear_hip column (stems and projections on vge_linear.hip)")
    ap.add_argument("--fusion-backend", default="torch", choices=["torch", "hip"],
                    help="hip: add the fusion_hip column (LayerNorm + fusion on vge_fusion.hip) and fusion_240")
    args = ap.parse_args()
    conv_backend, time_backend = args.conv_backend, args.time_backend
    linear_backend, fusion_backend = args.linear_backend, args.fusion_backend
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
    # column -> (module, optimiser, scheduler, loss backend); the two existing columns share one module
    columns = {b: (model, opt, sched, b) for b in BACKENDS}
    if conv_backend == "hip":
        model_h = HumanActionScorer(dims_raw, dims_diff, dropout=0.1, conv_backend="hip").to(dev).train()
        model_h.load_state_dict(copy.deepcopy(model.state_dict()))
        columns["conv_hip"] = (model_h, *T.make_optimizer(model_h, 3e-4, 100, 30), "hip")
    if time_backend == "hip":
        model_t = HumanActionScorer(dims_raw, dims_diff, dropout=0.1, time_backend="hip").to(dev).train()
        model_t.load_state_dict(copy.deepcopy(model.state_dict()))
        columns["time_hip"] = (model_t, *T.make_optimizer(model_t, 3e-4, 100, 30), "hip")
    extra = {}
    if fusion_backend == "hip":
        extra["fusion_hip"] = {"fusion_backend": "hip"}
    if linear_backend == "hip":
        extra["linear_hip"] = {"linear_backend": "hip"}
    if linear_backend == fusion_backend == "hip":
        extra["linear_fusion_hip"] = {"linear_backend": "hip", "fusion_backend": "hip"}
        if conv_backend == time_backend == "hip":
            extra["all_hip"] = {"conv_backend": "hip", "time_backend": "hip", "linear_backend": "hip",
                                "fusion_backend": "hip"}
    for name, kw in extra.items():
        m = HumanActionScorer(dims_raw, dims_diff, dropout=0.1, **kw).to(dev).train()
        m.load_state_dict(copy.deepcopy(model.state_dict()))
        columns[name] = (m, *T.make_optimizer(m, 3e-4, 100, 30), "hip")
    order = tuple(columns)
    gen = torch.Generator().manual_seed(1337)
    tables = [V.partial_shuffle_indices(B, 32, generator=gen).to(dev), V.reverse_indices(B).to(dev),
              V.static_indices(B).to(dev)]
    times = {b: {k: [] for k in PIECES} for b in order}
    values = {}
    for rep in range(WARMUP + REPS):
        for backend in (order if rep % 2 == 0 else order[::-1]):
            model, opt, sched, loss_backend = columns[backend]
            tcl, hard = losses[loss_backend]
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
    for backend in order:
        ms = {k: statistics.median(v) for k, v in times[backend].items()}
        out[backend] = {k + "_ms": round(v, 4) for k, v in ms.items()}
        out[backend]["loss_share_of_pieces"] = round(ms["loss_fwd_bwd"] / ms["pieces_total"], 5)
        out[backend]["last_loss"] = values[backend]
    out["loss_hip_over_torch_240"] = round(out["hip"]["loss_fwd_bwd_ms"] / out["torch"]["loss_fwd_bwd_ms"], 4)
    if conv_backend == "hip":
        for k in ("forwards", "module_backward", "step"):
            out[f"conv_hip_over_torch_{k}"] = round(out["conv_hip"][k + "_ms"] / out["hip"][k + "_ms"], 4)
        out["convblock_240"] = convblock_alone(dev)
    if time_backend == "hip":
        for k in ("forwards", "module_backward", "step"):
            out[f"time_hip_over_torch_{k}"] = round(out["time_hip"][k + "_ms"] / out["hip"][k + "_ms"], 4)
        out["timelayer_240"] = timelayer_alone(dev)
    for name in extra:
        for k in ("forwards", "module_backward", "step"):
            out[f"{name}_over_torch_{k}"] = round(out[name][k + "_ms"] / out["hip"][k + "_ms"], 4)
    if fusion_backend == "hip":
        out["fusion_240"] = fusion_alone(dev)

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
