"""Training without a GPU: the PK sampler, the scorer as a torch module, the torch-backend losses and the training
step on the CPU, against what the reference itself produced (tests/golden/train_golden.npz, written by
tests/golden/make_train_golden.py).

Tolerances.  r is the distance of the reference's own float32 result from float64 on the same inputs, floored at
one float32 ulp of the value (a tensor's value: its largest magnitude).  Losses and loss gradients must lie within
8 r of float64; the training steps within `factor` r, the factor the fixture stores: 8, or the smallest power of two
that admits the reference's own single-threaded float32 run."""
import copy

import numpy as np
import pytest
import torch

from tests import train_ref as TR
from tests import validate_ref as R
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def tgold():
    return dict(np.load(GOLDEN / "train_golden.npz"))


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


# ----------------------------------------------------------------------------- the sampler

@pytest.mark.parametrize("case", ["4x3", "uneven", "uneven36", "golden"])
def test_sampler_yields_the_reference_batches(tgold, case):
    from vge.data import PKBatchSampler
    labels = tgold[f"sampler_{case}_labels"]
    p, k = (int(v) for v in tgold[f"sampler_{case}_pk"])
    want = tgold[f"sampler_{case}_batches"]
    s = PKBatchSampler(labels, P=p, K=k, drop_last=True, generator=np.random.default_rng(1337))
    assert len(s) == len(labels) // (p * k)
    for epoch in range(want.shape[0]):
        got = [b for b in s]
        assert all(len(b) == p * k for b in got)
        assert np.array_equal(np.array(got, np.int32), want[epoch]), (case, epoch)


def test_sampler_labels_of_the_golden_split(tgold, golden_dataset):
    from vge.data import ACTION_CLASSES, NpzVideoDataset, sample_all_windows_npz, train_test_split
    paths, _ = golden_dataset
    real = NpzVideoDataset(paths["real"], filter_classes=ACTION_CLASSES)
    train_ds, _ = train_test_split(real, train_ratio=0.8, seed=1337)
    label_dict = {c: i for i, c in enumerate(sorted({it.cls for it in real.items}))}
    labels = [label_dict[it.cls] for it, _ in sample_all_windows_npz(train_ds, 32, 8)]
    assert np.array_equal(np.array(labels, np.int32), tgold["sampler_golden_labels"])


def test_sampler_refuses_more_classes_than_there_are():
    from vge.data import PKBatchSampler
    with pytest.raises(ValueError, match="P = 3"):
        PKBatchSampler([0, 0, 1, 1], P=3, K=2)


# ----------------------------------------------------------------------------- the module

@pytest.mark.parametrize("layout", ["kp", "nokp", "small"])
def test_module_state_dict_is_the_checkpoints(layout):
    m, sd = TR.module(layout)
    msd = m.state_dict()
    assert sorted(msd) == sorted(sd)
    assert {k: tuple(v.shape) for k, v in msd.items()} == {k: tuple(np.shape(v)) for k, v in sd.items()}
    TR.load(m, sd)                                   # strict: every key, no extra one
    back = m.numpy_state_dict()
    assert all(np.array_equal(back[k], np.asarray(sd[k], np.float32)) for k in sd)


def test_module_refuses_bad_arguments():
    from vge.model import HumanActionScorer
    with pytest.raises(ValueError, match="same modalities"):
        HumanActionScorer({"vit": 4}, {"pose": 4})
    m = HumanActionScorer({"a": 4}, {"a": 0}, d_model=32, time_layers=1, time_heads=2)
    assert m.motion_enc is None
    with pytest.raises(ValueError, match=r"\[B,T,4\]"):
        m(torch.zeros(2, 32, 5))


@pytest.fixture(scope="module")
def cpu_features(golden_dataset):
    """The oracle's features of the generated set's windows and of the train split's windows (the reference's
    sample_all_windows_npz order), computed once."""
    from oracle import evalflow as EF
    from oracle.featurize import featurize_window
    from vge.data import ACTION_CLASSES, NpzVideoDataset, sample_all_windows_npz, train_test_split
    paths, _ = golden_dataset
    kdir = paths["real_kp"]
    real = NpzVideoDataset(paths["real"], filter_classes=ACTION_CLASSES)
    train_ds, _ = train_test_split(real, train_ratio=0.8, seed=1337)
    label_dict = {c: i for i, c in enumerate(sorted({it.cls for it in real.items}))}
    stats = EF.compute_stats([(it.cls, it.name, it.path, it.length) for it in train_ds.items], kdir)
    samples = sample_all_windows_npz(train_ds, 32, 8)
    cache = {}

    def arrays(path, kd, cls):
        if path not in cache:
            cache[path] = EF.load(path, kd, cls)
        return cache[path]
    train = np.stack([featurize_window(*arrays(it.path, kdir, it.cls), s, stats) for it, s in samples])
    gen_items = EF.scan_generated(paths["generated_meshes"])
    gen = np.stack([featurize_window(*arrays(p, paths["generated_kps"], c), s, stats)
                    for c, n, p, T in gen_items for s in EF.windows_for(T)])
    labels = np.array([label_dict[it.cls] for it, _ in samples], np.int64)
    return {"train": torch.from_numpy(train), "labels": torch.from_numpy(labels), "gen": torch.from_numpy(gen)}


@pytest.mark.parametrize("layout,flow", [("kp", "golden_flow.npz"), ("small", "golden_flow_small.npz")])
def test_module_eval_embeddings_match_the_golden_ones(cpu_features, layout, flow):
    want = np.load(GOLDEN / flow)["seq_embeds"]
    m, sd = TR.module(layout, dropout=0.1)
    TR.load(m, sd).eval()
    with torch.no_grad():
        got = torch.cat([m(cpu_features["gen"][i:i + 16])[0] for i in range(0, want.shape[0], 16)]).numpy()
    assert got.shape == want.shape
    err = float(np.abs(got - want).max())
    print(f"{layout}: module eval-mode seq_embed max|err| vs the reference {err:.3e}")
    assert err <= 2e-5


# ----------------------------------------------------------------------------- the torch-backend losses

@pytest.mark.parametrize("case", [c for c in R.fixture_cases()], ids=lambda c: c[0])
def test_torch_backend_losses_and_gradients(tgold, case):
    from vge import losses
    name, B, d, kind, seed = case
    emb, neg, lab = R.case_inputs(B, d, kind, seed)
    if f"grad_{name}_r" not in tgold:
        assert not np.isfinite(float(R.tcl(emb, lab)))           # the fixture holds the finite cases
        e = torch.from_numpy(emb)
        assert torch.isnan(losses.TCL(backend="torch")(e, torch.from_numpy(lab)))      # NaN where the reference's is
        return
    assert np.array_equal(R.digest(emb, neg, lab), tgold[f"grad_{name}_digest"]), "case generator drifted"
    l64, g64 = TR.tcl_autograd(emb, lab, torch.float64)
    h64, ga64, gn64 = TR.hardneg_autograd(emb, neg, torch.float64)
    head64 = tgold[f"grad_{name}_head64"]
    for k, g in enumerate((g64, ga64, gn64)):
        assert np.abs(g[:head64.shape[1]] - head64[k]).max() <= 1e-12        # the float64 side is the fixture's
    tcl32, tcl64, hard32, hard64 = (float(v) for v in tgold[f"grad_{name}_loss"])
    e = torch.from_numpy(emb).requires_grad_(True)
    lt = losses.TCL(backend="torch")(e, torch.from_numpy(lab))
    (gt,) = torch.autograd.grad(lt, e)
    a, n = torch.from_numpy(emb).requires_grad_(True), torch.from_numpy(neg).requires_grad_(True)
    lh = losses.SupConWithHardNegatives(backend="torch")(a, a, n)
    ga, gn = torch.autograd.grad(lh, (a, n))
    r = tgold[f"grad_{name}_r"]
    for what, got, want, rr in (("tcl", lt.item(), l64, max(abs(tcl32 - tcl64), _ulp32(tcl64))),
                                ("hardneg", lh.item(), h64, max(abs(hard32 - hard64), _ulp32(hard64)))):
        print(f"{name} {what} loss: |torch-f64| / r {abs(got - want) / rr:.3f}")
        assert abs(got - want) <= 8 * rr, (name, what, got, want, rr)
    for what, got, want, rr in (("tcl grad", gt, g64, r[0]), ("grad_anchor", ga, ga64, r[1]), ("grad_neg", gn, gn64, r[2])):
        err = float(np.abs(got.numpy().astype(np.float64) - want).max())
        print(f"{name} {what}: |torch-f64| / r {err / rr:.3f}")
        assert err <= 8 * float(rr), (name, what, err, rr)


def test_general_positive_goes_through_torch():
    from vge import losses
    g = torch.Generator().manual_seed(3)
    a, p, n = (torch.nn.functional.normalize(torch.randn(6, 16, generator=g, dtype=torch.float64), dim=-1)
               for _ in range(3))
    got = losses.SupConWithHardNegatives()(a, p, n)
    logits = torch.stack([(a * p).sum(-1), (a * n).sum(-1)], 1) / 0.07
    want = torch.nn.functional.cross_entropy(logits, torch.zeros(6, dtype=torch.long))
    assert abs(float(got) - float(want)) <= 1e-12


# ----------------------------------------------------------------------------- the training step

@pytest.mark.parametrize("ckpt", ["kp", "small"])
def test_four_steps_reproduce_the_reference(tgold, cpu_features, ckpt):
    comps, grads, _ = TR.run_steps(tgold, ckpt, lambda b: cpu_features["train"][b], cpu_features["labels"], "cpu",
                                "torch")
    TR.check_steps(tgold, ckpt, comps, grads, "cpu torch")


def test_overfits_one_batch(tgold, cpu_features):
    """Fixture (d): 20 updates on one fixed batch lower the loss, as they do for the reference."""
    assert int(tgold["overfit_lower"][0]) == 1 and tgold["overfit_loss"][1] < tgold["overfit_loss"][0]
    comps, _, _ = TR.run_steps(tgold, "kp", lambda b: cpu_features["train"][b], cpu_features["labels"], "cpu", "torch",
                            n_steps=21, tables_key="overfit_tables", batches=tgold["steps_kp_batches"][:1])
    loss = comps.sum(axis=1)
    print(f"overfit: step 0 {loss[0]:.4f} (reference {tgold['overfit_loss'][0]:.4f}), step 20 {loss[20]:.4f} "
          f"(reference {tgold['overfit_loss'][1]:.4f})")
    assert loss[20] < loss[0]


def test_non_finite_loss_skips_the_step():
    """A batch with a label that appears once makes TCL NaN: parameters, optimiser state and scheduler stay as they
    were (train.py:499-500)."""
    from vge import train as T
    from vge.losses import TCL, SupConWithHardNegatives
    m, sd = TR.module("small")
    TR.load(m, sd).train()
    opt, sched = T.make_optimizer(m, 3e-4, 5, 30)
    tcl, hard = TCL(backend="torch"), SupConWithHardNegatives(backend="torch")
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(4, 32, 2596, generator=g)
    variants = T.window_variants(feats, T.partial_shuffle_indices(4, 32, generator=g))
    stepped, vals = T.train_step(m, opt, sched, tcl, hard, feats, variants, torch.tensor([0, 0, 1, 1]))
    assert stepped and np.isfinite(vals).all() and sched.last_epoch == 1
    before = copy.deepcopy({"model": m.state_dict(), "opt": opt.state_dict(), "sched": sched.state_dict()})
    stepped, vals = T.train_step(m, opt, sched, tcl, hard, feats, variants, torch.tensor([0, 0, 1, 2]))
    assert not stepped and np.isnan(vals[0]) and np.isfinite(vals[1:]).all()
    assert all(torch.equal(v, before["model"][k]) for k, v in m.state_dict().items())
    after = opt.state_dict()
    assert after["param_groups"] == before["opt"]["param_groups"]
    for i, st in after["state"].items():
        assert all(torch.equal(torch.as_tensor(v), torch.as_tensor(before["opt"]["state"][i][k])) for k, v in st.items())
    assert sched.state_dict() == before["sched"] and sched.last_epoch == 1
