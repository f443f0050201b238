"""Float64 restatement of the reference's held-out validation loss (test helper, not a test).

  tcl            losses.py:6-34   (TCL.forward, the literal expression with its [B,B] / [B] broadcast)
  hardneg        losses.py:37-56  (SupConWithHardNegatives.forward(anchor, anchor, neg))
  centroid_distance
                 train.py:366-378 (F.normalize eps 1e-12, torch.norm)
  reduce_batches train.py:294-333 (evaluate_test_set's sums and its skip of non-finite batches)
  flow           train.py:286-333 + 511-524 over an encoder callable, in batches of consecutive windows

Every function takes a dtype: float64 is the reference the GPU tests compare against, float32 gives the reference's
own arithmetic on the CPU (the distance between the two is the tolerance unit `r` of tests/test_validate_gpu.py).
"""
from __future__ import annotations

import hashlib
import math

import numpy as np
import torch
import torch.nn.functional as F

COMPONENTS = ("tcl", "hard_shuf", "hard_rev", "hard_stat")


def tcl(emb, labels, temperature=0.1, k1=5000.0, k2=1.0, dtype=torch.float64):
    """losses.py:14-34, line by line.  `exp_dot / denom` divides a [B,B] matrix by a [B] vector: the vector runs
    along the last axis, so element (i,j) is divided by the denominator of row j."""
    z = torch.as_tensor(emb).to(dtype)
    t = torch.as_tensor(labels).long()
    k1 = torch.tensor(k1)
    k2 = torch.tensor(k2)
    dot = torch.mm(z, z.T)
    exp_dot = torch.exp(dot / temperature)
    exp_dot_n = torch.exp(-1 * dot)
    similar = t.unsqueeze(1).repeat(1, t.shape[0]) == t
    anchor_out = 1 - torch.eye(exp_dot.shape[0])
    positives = similar * anchor_out
    negatives = ~similar
    per_sample = torch.sum(positives, dim=1)
    den = torch.sum(exp_dot * positives, dim=1) + (k1 * torch.sum(exp_dot_n * positives, dim=1)) + \
        (k2 * torch.sum(exp_dot * negatives, dim=1))
    loss = torch.sum(-torch.log(exp_dot / den) * positives, dim=1) / per_sample
    return torch.mean(loss)


def hardneg(anchor, neg, temperature=0.07, dtype=torch.float64):
    """losses.py:42-56 with positive = anchor: cross entropy of (sim_ap, sim_ah) against class 0."""
    a = torch.as_tensor(anchor).to(dtype)
    n = torch.as_tensor(neg).to(dtype)
    sim_ap = torch.sum(a * a, dim=-1) / temperature
    sim_ah = torch.sum(a * n, dim=-1) / temperature
    logits = torch.stack([sim_ap, sim_ah], dim=1)
    return F.cross_entropy(logits, torch.zeros(a.shape[0], dtype=torch.long))


def centroid_distance(emb, labels, centroids, dtype=torch.float64):
    """train.py:366-378 per sample; NaN where the label has no centroid (the reference's `continue`)."""
    e = F.normalize(torch.as_tensor(emb).to(dtype), p=2, dim=-1)
    c = torch.as_tensor(centroids).to(dtype)
    t = torch.as_tensor(labels).long()
    out = torch.full((e.shape[0],), float("nan"), dtype=dtype)
    ok = (t >= 0) & (t < c.shape[0])
    out[ok] = torch.norm(e[ok] - c[t[ok]], p=2, dim=-1)
    return out


def reduce_batches(batch_losses):
    """train.py:294-333: batch_losses is a list of four-component lists (COMPONENTS order, weights applied).
    -> (loss, components, n_batches, skipped_batches)."""
    total, comp, n, skipped = 0.0, dict.fromkeys(COMPONENTS, 0.0), 0, 0
    for vals in batch_losses:
        s = sum(float(v) for v in vals)
        if not math.isfinite(s):
            skipped += 1
            continue
        total += s
        for k, v in zip(COMPONENTS, vals):
            comp[k] += float(v)
        n += 1
    if n == 0:
        return float("inf"), {}, 0, skipped
    return total / n, {k: v / n for k, v in comp.items()}, n, skipped


def flow(encode, feats, labels, batch, shuffle_tables, hard_weight=10.0, dtype=torch.float64):
    """evaluate_test_set over feats [N,T,D] with `encode(x) -> seq_embed [b,d]` (the oracle encoder), in batches of
    `batch` consecutive windows and the given per-batch shuffle tables [b,T].  -> reduce_batches' tuple."""
    feats = torch.as_tensor(feats).to(dtype)
    labels = torch.as_tensor(labels).long()
    N, T, _ = feats.shape
    per_batch = []
    for k, b0 in enumerate(range(0, N, batch)):
        x = feats[b0:b0 + batch]
        y = labels[b0:b0 + batch]
        src = torch.as_tensor(shuffle_tables[k]).long()
        e = encode(x).to(dtype)
        shuf = torch.gather(x, 1, src.unsqueeze(-1).expand(-1, -1, x.shape[-1]))
        rev = torch.flip(x, dims=[1])
        stat = x[:, :1].expand(-1, T, -1)
        vals = [tcl(e, y, dtype=dtype)]
        for v in (shuf, rev, stat):
            vals.append(hard_weight * hardneg(e, encode(v).to(dtype), dtype=dtype))
        per_batch.append([float(v) for v in vals])
    return reduce_batches(per_batch)


# ----------------------------------------------------------------------------- shared inputs of the fixture and tests

FLOW_SMALL_BATCH = 10   # the golden test split (34 windows) gives 3 counted and 1 skipped batch at this size
PERTURBED_KEY = "temporal.layers.0.linear1.weight"


def make_labels(B, kind, seed):
    """kind "ten": ten classes at random, every one at least twice when B allows; "singleton": the same with one
    label that appears once (TCL is NaN); "equal": one class (no negatives; finite for B >= 2)."""
    rng = np.random.default_rng(seed)
    if kind == "equal":
        return np.full(B, 3, np.int32)
    lab = rng.integers(0, 10, B).astype(np.int32)
    if B >= 20:
        lab[:20] = np.repeat(np.arange(10, dtype=np.int32), 2)   # no accidental singleton
    elif B >= 2:
        lab = (np.arange(B) % max(1, B // 2)).astype(np.int32)   # pairs (an odd B leaves a triple)
        if B % 2:
            lab[-1] = lab[0]
    rng.shuffle(lab)
    if kind == "singleton":
        lab[rng.integers(0, B)] = 11
    return lab


def make_embeddings(B, d, labels, seed):
    """L2-normalised float32 rows scattered around one direction per class (what a trained encoder emits)."""
    rng = np.random.default_rng(seed + 1000)
    centers = rng.standard_normal((12, d))
    x = centers[np.asarray(labels) % 12] + 0.6 * rng.standard_normal((B, d))
    x = x / np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x.astype(np.float32))


def fixture_cases():
    """Fixture (b): B in {1, 2, 7, 65, 300} x d in {32, 256}, with the non-finite cases (B = 1, a singleton class)
    and all labels equal.  -> [(name, B, d, kind, seed)]"""
    out = []
    for d in (32, 256):
        for B, kinds in ((1, ("ten",)), (2, ("equal", "singleton")), (7, ("ten", "singleton", "equal")),
                         (65, ("ten", "singleton")), (300, ("ten", "singleton", "equal"))):
            for kind in kinds:
                out.append((f"B{B}_d{d}_{kind}", B, d, kind, 100 * B + d))
    return out


def case_inputs(B, d, kind, seed):
    """-> (emb [B,d], neg [B,d], labels [B]) of one loss case; neg is emb moved by about half its length and
    normalised again (a hard negative: cosine about 0.9 to its anchor)."""
    lab = make_labels(B, kind, seed)
    emb = make_embeddings(B, d, lab, seed)
    rng = np.random.default_rng(seed + 7)
    neg = emb.astype(np.float64) + (0.5 / np.sqrt(d)) * rng.standard_normal((B, d))
    neg = neg / np.linalg.norm(neg, axis=1, keepdims=True)
    return emb, np.ascontiguousarray(neg.astype(np.float32)), lab


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest()[:8], np.uint8).copy()


def perturbed_state_dict(sd):
    """The golden checkpoint with one layer's weights perturbed (the second checkpoint of the ranking test)."""
    rng = np.random.default_rng(4242)
    out = dict(sd)
    w = np.asarray(sd[PERTURBED_KEY], np.float32)
    out[PERTURBED_KEY] = (w + 0.25 * np.abs(w).mean() * rng.standard_normal(w.shape)).astype(np.float32)
    return out
