"""Generate tests/golden/train_golden.npz by running the REFERENCE's training code (build container only; the
reference is imported read-only as make_validate_golden.py does and nothing of it is copied -- only arrays and
numbers it produced).

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_train_golden.py

  a. sampler_<case>_labels / _batches   the reference's PKBatchSampler (utils.py:922-1015) under default_rng(1337):
                           the batches of two consecutive epochs, [epoch, batch, P K]
                             "4x3"     4 classes x 3, P 4, K 3
                             "uneven"  5 classes of sizes 7 / 3 / 2 / 5 / 1, P 3, K 4: a short queue is topped up;
                                       18 // 12 = one batch an epoch, so the class order cannot wrap here
                             "uneven36"  the same with doubled class sizes (three batches an epoch): the class
                                       order wraps and is reshuffled, and queues are topped up -- asserted here
                             "golden"  the golden train split's window labels, P 4, K 3
  b. grad_<case>_*         the reference's TCL() / SupConWithHardNegatives() float32 CPU autograd gradients on the
                           inputs of validate_ref.fixture_cases (finite cases only) next to the float64 autograd of
                           validate_ref's restatement, for the three tensors (d tcl / d emb, d hard / d anchor,
                           d hard / d neg):  r [3] = max |float32 - float64| over the whole tensor, floored at one
                           float32 ulp of the largest float64 magnitude;  head32 / head64 [3, min(B,4), d] the first
                           rows of both (a full B = 300 gradient in both precisions would not fit a fixture; the
                           tests recompute the float64 side);  loss [tcl32, tcl64, hard32, hard64]
  c. steps_<ckpt>_*        four training steps of Exp_TCL_Hard_V2Plus.train_one_epoch (an instance made with
                           object.__new__; AdamW(3e-4), CosineAnnealingLR as train.py:183-186) on the golden real
                           set's train split, P 4, K 3, dropout 0, from golden_state_dict("kp") / ("small"):
                             batches [4,12] window indices, tables [4,12,32] the shuffle tables it drew
                             comp_f32 / comp_f32_t1 / comp_f64 [4,4]  the loss components per step: float32 with
                                       16 threads, float32 with 1 thread, model.double()
                             names     the parameter names, norm_* [n] the L2 norm of each step-0 gradient
                             small_<name>_*  the step-0 gradient of the small tensors (SMALL_TENSORS)
                             r_k [4,4], r_norm [n], r_small_<name>  |f32 - f64| floored at one float32 ulp of the
                                       value (a tensor's value: its largest magnitude)
                             factor    8, or the smallest power of two above it that admits the 1-thread float32
                                       run (|f32_t1 - f64| <= factor r everywhere)
  d. overfit_*             21 forward passes / 20 updates of the reference on the first batch of (c), "kp", dropout 0:
                           overfit_loss [step-0 loss, step-20 loss], overfit_lower [1 when step 20 is lower],
                           overfit_tables [21,12,32]
"""
from __future__ import annotations

import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(REPO / "video-gen-evals_amd"))
sys.path.insert(0, str(REPO))

from tests import validate_ref as R  # noqa: E402
from tests.golden.dataset_spec import SMALL_HP, build_golden_dataset, golden_state_dict  # noqa: E402
from tests.golden.make_golden import _write_npz_fixed  # noqa: E402
from tests.golden.make_validate_golden import tables_from_draws  # noqa: E402

REF = "/root/reference"
SEED = 1337
P, K, STEPS, OVERFIT_STEPS = 4, 3, 4, 20
GRAD_ROWS = 4       # rows of each gradient kept in (b): the file stays small, r covers the whole tensor
SMALL_TENSORS = ("fusion.latent", "fusion.logit_temp", "fusion.logit_bias", "cls", "state_enc.beta.stem.weight",
                 "motion_enc.beta.stem.weight", "state_enc.global.stem.weight", "motion_enc.global.stem.weight")


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def sampler_epochs(U, labels, p, k, epochs=2):
    s = U.PKBatchSampler(labels, P=p, K=k, drop_last=True, generator=np.random.default_rng(SEED))
    return s, np.array([[b for b in s] for _ in range(epochs)], np.int32)


class CountingRng:
    """A numpy Generator that notes which of its methods the sampler called, with the length of what was shuffled."""

    def __init__(self):
        self.rng, self.calls = np.random.default_rng(SEED), []

    def shuffle(self, x):
        self.calls.append(("shuffle", len(x)))
        return self.rng.shuffle(x)

    def choice(self, *a, **k):
        self.calls.append(("choice", 0))
        return self.rng.choice(*a, **k)


def sampler_events(U, labels, p, k, epochs=2):
    """-> (the class order wrapped and was reshuffled, a short queue was topped up) over the recorded epochs: after
    the n_classes + 1 shuffles of an epoch's reset, a shuffle that is not a batch's is the reshuffle of the wrap."""
    rng = CountingRng()
    s = U.PKBatchSampler(labels, P=p, K=k, drop_last=True, generator=rng)
    n_cls = len(set(int(y) for y in labels))
    wrapped = topped = False
    for _ in range(epochs):
        rng.calls.clear()
        n_batches = len([b for b in s])
        calls = rng.calls[n_cls + 1:]
        topped |= any(c == "choice" for c, _ in calls)
        wrapped |= sum(1 for c, _ in calls if c == "shuffle") > n_batches
    return wrapped, topped


class Setup:
    """BaseExperiment.__init__'s data path (train.py:117-169) for the golden real set."""

    def __init__(self, U, E, paths):
        real = U.NpzVideoDataset(paths["real"], filter_classes=E.ACTION_CLASSES)
        self.train_ds, _ = U.train_test_split(real, train_ratio=0.8, seed=SEED)
        self.stats = U.compute_stats_from_npz(self.train_ds.items, keypoint_dir=paths["real_kp"])
        self.label_dict = {c: i for i, c in enumerate(sorted({it.cls for it in real.items}))}
        self.dims = E.infer_dims_from_stats(self.stats)
        samples = U.sample_all_windows_npz(self.train_ds, clip_len=32, stride=8)
        self.windows = U.WindowDataset(samples, clip_len=32, stats=self.stats, keypoint_dir=paths["real_kp"], seed=SEED)
        self.labels = [self.label_dict[it.cls] for it, _ in samples]
        self.sampler = U.PKBatchSampler(self.labels, P=P, K=K, drop_last=True, generator=np.random.default_rng(SEED))
        self.batches = [b for b in self.sampler][:STEPS]
        assert len(self.batches) == STEPS, len(self.batches)
        self.collated = [U.safe_collate([self.windows[i] for i in b]) for b in self.batches]


def reference_steps(U, TR, MODEL, LS, setup, sd, hp, loader, dtype=torch.float32, threads=16):
    """train_one_epoch over `loader` (a list of collated batches) -> components [n,4], step-0 gradients, tables."""
    torch.set_num_threads(threads)
    model = MODEL.HumanActionScorer(dims_map_raw=setup.dims[0], dims_map_diff=setup.dims[1], latent_dim=128,
                                    dropout=0.0, **hp)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32).copy()) for k, v in sd.items()})
    model.train()
    if dtype == torch.float64:
        model.double()
        loader = [(f.double(), c, v) for f, c, v in loader]
    exp = object.__new__(TR.Exp_TCL_Hard_V2Plus)
    exp.model, exp.device, exp.label_dict = model, torch.device("cpu"), setup.label_dict
    exp.tcl, exp.hard = LS.TCL(), LS.SupConWithHardNegatives()
    exp.optimizer = torch.optim.AdamW(list(model.parameters()), lr=3e-4)
    exp.scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(exp.optimizer, T_max=max(1, len(setup.sampler)) * 30,
                                                               eta_min=1e-6)
    exp.train_loader = loader
    comps, grads, draws = [], {}, []
    orig_clc, orig_step, orig_randperm = exp.compute_loss_components, exp.optimizer.step, torch.randperm

    def clc(emb, labels, feats=None):
        d = orig_clc(emb, labels, feats)
        comps.append([float(d[k]) for k in R.COMPONENTS])
        return d

    def step(*a, **k):
        if not grads:
            grads.update({n: p.grad.detach().double().numpy().copy() for n, p in model.named_parameters()})
        return orig_step(*a, **k)

    def randperm(*a, **k):
        r = orig_randperm(*a, **k)
        draws.append(r.clone())
        return r

    exp.compute_loss_components, exp.optimizer.step = clc, step
    torch.manual_seed(SEED)
    torch.randperm = randperm
    try:
        exp.train_one_epoch(0)
    finally:
        torch.randperm = orig_randperm
        torch.set_num_threads(16)
    B = loader[0][0].shape[0]
    tables = tables_from_draws(draws).reshape(len(loader), B, 32)
    assert exp.scheduler.last_epoch == len(loader), "a step was skipped as non-finite"
    return np.array(comps, np.float64), grads, tables


def main():
    sys.path.insert(0, REF)
    import utils as U  # noqa
    import eval as E  # noqa
    import train as TR  # noqa
    import losses as LS  # noqa
    import model as MODEL  # noqa
    out = {}

    # ---------------- a. the sampler
    cases = {"4x3": (np.repeat(np.arange(4), 3), 4, 3),
             "uneven": (np.repeat(np.arange(5), (7, 3, 2, 5, 1)), 3, 4)}
    # one epoch of "uneven" is a single batch (18 // 12), so its class order cannot wrap: "uneven36" doubles the
    # class sizes (three batches an epoch) and is where the wrap and the reshuffle occur
    cases["uneven36"] = (np.repeat(np.arange(5), (14, 6, 4, 10, 2)), 3, 4)
    events = {n: sampler_events(U, *cases[n]) for n in ("uneven", "uneven36")}
    print("sampler events (wrapped + reshuffled, topped up):", events)
    assert events["uneven"][1] and events["uneven36"] == (True, True), events

    # ---------------- b. the loss gradients
    tcl, hard = LS.TCL(), LS.SupConWithHardNegatives()
    for name, B, d, kind, seed in R.fixture_cases():
        emb, neg, lab = R.case_inputs(B, d, kind, seed)
        if not np.isfinite(float(R.tcl(emb, lab))):
            continue
        y = torch.from_numpy(lab).long()
        e32 = torch.from_numpy(emb).requires_grad_(True)
        l32 = tcl(e32, y)
        (g32,) = torch.autograd.grad(l32, e32)
        e64 = torch.from_numpy(emb).double().requires_grad_(True)
        l64 = R.tcl(e64, lab)
        (g64,) = torch.autograd.grad(l64, e64)
        a32, n32 = torch.from_numpy(emb).requires_grad_(True), torch.from_numpy(neg).requires_grad_(True)
        h32 = hard(a32, a32, n32)
        ha32 = torch.autograd.grad(h32, (a32, n32))
        a64 = torch.from_numpy(emb).double().requires_grad_(True)
        n64 = torch.from_numpy(neg).double().requires_grad_(True)
        h64 = R.hardneg(a64, n64)
        ha64 = torch.autograd.grad(h64, (a64, n64))
        t32 = [g32.numpy()] + [g.numpy() for g in ha32]
        t64 = [g64.numpy()] + [g.numpy() for g in ha64]
        out[f"grad_{name}_r"] = np.array([max(float(np.abs(a - b).max()), float(ulp32(np.abs(b).max())))
                                          for a, b in zip(t32, t64)])
        out[f"grad_{name}_head32"] = np.stack([a[:GRAD_ROWS] for a in t32])
        out[f"grad_{name}_head64"] = np.stack([b[:GRAD_ROWS] for b in t64])
        out[f"grad_{name}_loss"] = np.array([l32.item(), l64.item(), h32.item(), h64.item()], np.float64)
        out[f"grad_{name}_digest"] = R.digest(emb, neg, lab)

    # ---------------- c. four training steps, d. the overfit check
    for ckpt, layout in (("kp", "kp"), ("small", "small")):
        with tempfile.TemporaryDirectory() as tmp:
            paths, _, _ = build_golden_dataset(tmp, layout=layout)
            setup = Setup(U, E, paths)
            hp = dict(SMALL_HP) if layout == "small" else {}
            sd = golden_state_dict(layout)
            if ckpt == "kp":
                cases["golden"] = (np.asarray(setup.labels), P, K)
            c32, g32, t32 = reference_steps(U, TR, MODEL, LS, setup, sd, hp, setup.collated)
            c1, g1, t1 = reference_steps(U, TR, MODEL, LS, setup, sd, hp, setup.collated, threads=1)
            c64, g64, t64 = reference_steps(U, TR, MODEL, LS, setup, sd, hp, setup.collated, dtype=torch.float64)
            assert (t32 == t1).all() and (t32 == t64).all(), "the three runs drew different shuffle tables"
            p = f"steps_{ckpt}_"
            names = sorted(g64)
            norm = lambda g: np.array([np.linalg.norm(g[n].ravel()) for n in names])  # noqa: E731
            n32, n1, n64 = norm(g32), norm(g1), norm(g64)
            out[p + "batches"] = np.array(setup.batches, np.int32)
            out[p + "tables"] = t32.astype(np.uint8)
            out[p + "comp_f32"], out[p + "comp_f32_t1"], out[p + "comp_f64"] = c32, c1, c64
            out[p + "names"] = np.array(names)
            out[p + "norm_f32"], out[p + "norm_f32_t1"], out[p + "norm_f64"] = n32, n1, n64
            out[p + "r_k"] = np.maximum(np.abs(c32 - c64), ulp32(c64))
            out[p + "r_norm"] = np.maximum(np.abs(n32 - n64), ulp32(n64))
            worst = max(float((np.abs(c1 - c64) / out[p + "r_k"]).max()),
                        float((np.abs(n1 - n64) / out[p + "r_norm"]).max()))
            for n in SMALL_TENSORS:
                out[p + f"small_{n}_f32"] = g32[n].astype(np.float32)
                out[p + f"small_{n}_f64"] = g64[n]
                r = max(float(np.abs(g32[n] - g64[n]).max()), float(ulp32(np.abs(g64[n]).max())))
                out[p + f"r_small_{n}"] = np.array([r])
                worst = max(worst, float(np.abs(g1[n] - g64[n]).max()) / r)
            factor = 8
            while worst > factor:
                factor *= 2
            out[p + "factor"] = np.array([factor], np.int64)
            print(ckpt, "components f32\n", c32, "\n f64\n", c64, "\n 1-thread worst ratio", worst, "factor", factor)
            if ckpt == "kp":
                loader = [setup.collated[0]] * (OVERFIT_STEPS + 1)
                co, _, to = reference_steps(U, TR, MODEL, LS, setup, sd, hp, loader)
                loss = co.sum(axis=1)
                assert loss[OVERFIT_STEPS] < loss[0], "the reference does not overfit one batch from this seed"
                out["overfit_loss"] = np.array([loss[0], loss[OVERFIT_STEPS]])
                out["overfit_lower"] = np.array([int(loss[OVERFIT_STEPS] < loss[0])], np.int64)
                out["overfit_tables"] = to.astype(np.uint8)
                print("overfit", loss[0], "->", loss[OVERFIT_STEPS])

    for name, (labels, p, k) in cases.items():
        s, batches = sampler_epochs(U, labels, p, k)
        assert batches.shape[1] == len(s) >= 1 and batches.shape[2] == p * k
        out[f"sampler_{name}_labels"] = np.asarray(labels, np.int32)
        out[f"sampler_{name}_pk"] = np.array([p, k], np.int64)
        out[f"sampler_{name}_batches"] = batches
    _write_npz_fixed(HERE / "train_golden.npz", out)
    print("written", HERE / "train_golden.npz", (HERE / "train_golden.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
