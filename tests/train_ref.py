"""Shared references of the training tests (test helper, not a test): autograd of tests/validate_ref.py's float64
restatement of the two losses, each result computed once per input and left unchanged; the golden checkpoints as
torch modules; and the recorded training steps of tests/golden/train_golden.npz run through vge.train, with their bars."""
from __future__ import annotations


import numpy as np
import torch

from tests import validate_ref as R

_CACHE = {}


def _key(tag, dtype, *arrays):
    return (tag, str(dtype)) + tuple(bytes(R.digest(a)) + bytes(str(a.shape), "ascii") for a in arrays)


def tcl_autograd(emb, labels, dtype):
    """-> (loss, d loss / d emb [B,d]) of validate_ref.tcl in `dtype` on the CPU, as float / numpy of that dtype."""
    k = _key("tcl", dtype, emb, labels)
    if k not in _CACHE:
        z = torch.from_numpy(np.asarray(emb, np.float32)).to(dtype).requires_grad_(True)
        loss = R.tcl(z, labels, dtype=dtype)
        (g,) = torch.autograd.grad(loss, z)
        g = g.numpy()
        g.setflags(write=False)
        _CACHE[k] = (float(loss.detach()), g)
    return _CACHE[k]


def hardneg_autograd(anchor, neg, dtype):
    """-> (loss, d / d anchor, d / d neg) of validate_ref.hardneg (positive = anchor) in `dtype` on the CPU."""
    k = _key("hardneg", dtype, anchor, neg)
    if k not in _CACHE:
        a = torch.from_numpy(np.asarray(anchor, np.float32)).to(dtype).requires_grad_(True)
        n = torch.from_numpy(np.asarray(neg, np.float32)).to(dtype).requires_grad_(True)
        loss = R.hardneg(a, n, dtype=dtype)
        ga, gn = torch.autograd.grad(loss, (a, n))
        ga, gn = ga.numpy(), gn.numpy()
        ga.setflags(write=False)
        gn.setflags(write=False)
        _CACHE[k] = (float(loss.detach()), ga, gn)
    return _CACHE[k]


# ----------------------------------------------------------------------------- the module and the training step

def module(layout, dropout=0.0):
    from tests.golden.dataset_spec import SMALL_HP, golden_state_dict
    from vge import synth
    from vge.model import HumanActionScorer
    sd = golden_state_dict(layout)
    mods = list(synth.DIMS_RAW)[:4 if layout == "nokp" else 5]
    hp = dict(SMALL_HP) if layout == "small" else {}
    m = HumanActionScorer({k: synth.DIMS_RAW[k] for k in mods}, {k: synth.DIMS_DIFF[k] for k in mods},
                          dropout=dropout, **hp)
    return m, sd


def load(m, sd):
    m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32).copy()) for k, v in sd.items()})
    return m


def run_steps(tgold, ckpt, feats_of, labels, device, backend, n_steps=4, tables_key=None, batches=None):
    """n_steps of vge.train.train_step from the golden checkpoint on the recorded batches and shuffle tables ->
    (components [n,4], {name: step-0 gradient}, the module)."""
    from vge import train as T
    from vge.losses import TCL, SupConWithHardNegatives
    m, sd = module(ckpt)
    load(m, sd).to(device).train()
    batches = tgold[f"steps_{ckpt}_batches"] if batches is None else batches
    tables = tgold[tables_key or f"steps_{ckpt}_tables"]
    opt, sched = T.make_optimizer(m, 3e-4, len(labels) // 12, 30)
    tcl, hard = TCL(backend=backend), SupConWithHardNegatives(backend=backend)
    comps, grads = [], {}
    for k in range(n_steps):
        b = torch.from_numpy(batches[k % len(batches)].astype(np.int64))
        feats = feats_of(b)
        variants = T.window_variants(feats, torch.from_numpy(tables[k].astype(np.int32)))
        stepped, vals = T.train_step(m, opt, sched, tcl, hard, feats, variants, labels[b].to(device))
        assert stepped
        comps.append(vals)
        if k == 0:
            grads = {n: p.grad.detach().double().cpu().numpy().copy() for n, p in m.named_parameters()}
    assert sched.last_epoch == n_steps
    return np.array(comps), grads, m


def check_steps(tgold, ckpt, comps, grads, tag):
    """The bars of fixture (c) -> the largest ratios seen (components, norms, small tensors)."""
    p = f"steps_{ckpt}_"
    factor = int(tgold[p + "factor"][0])
    rk = np.abs(comps - tgold[p + "comp_f64"]) / tgold[p + "r_k"]
    names = [str(n) for n in tgold[p + "names"]]
    assert sorted(grads) == names
    norms = np.array([np.linalg.norm(grads[n].ravel()) for n in names])
    rn = np.abs(norms - tgold[p + "norm_f64"]) / tgold[p + "r_norm"]
    rs = {}
    for key in tgold:
        if key.startswith(p + "small_") and key.endswith("_f64"):
            n = key[len(p + "small_"):-len("_f64")]
            rs[n] = float(np.abs(grads[n] - tgold[key]).max() / tgold[p + f"r_small_{n}"][0])
    assert len(rs) == 8
    print(f"{tag} {ckpt}: factor {factor}; largest |x - f64| / r: components {rk.max():.3f} (per step "
          f"{np.round(rk.max(axis=1), 3).tolist()}), gradient norms {rn.max():.3f} ({names[int(rn.argmax())]}), "
          f"small tensors {max(rs.values()):.3f}")
    assert rk.max() <= factor, (tag, ckpt, rk)
    assert rn.max() <= factor, (tag, ckpt, names[int(rn.argmax())], rn.max())
    assert max(rs.values()) <= factor, (tag, ckpt, rs)
    return float(rk.max()), float(rn.max()), max(rs.values())
