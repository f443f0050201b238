"""Checkpoint validation on the GPU (vge_validate.hip through vge.ops / vge.validate) against the float64 restatement
of tests/validate_ref.py and the reference's own recorded results (tests/golden/validate_golden.npz).

Tolerances.  A loss must lie within 8 r of the float64 restatement, r being the distance of the reference's own float32
CPU result from that restatement on the same inputs (from the fixture, or computed here with the restated float32
expression), floored at one float32 ulp of the value; the flow's components within 4 r_c, r_c from the fixture.
Largest ratios |gpu - f64| / r seen on an MI355X are recorded in DESIGN.md ("Checkpoint validation")."""
import math

import numpy as np
import pytest
import torch

from tests import validate_ref as R
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def vgold():
    return dict(np.load(GOLDEN / "validate_golden.npz"))


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


# ----------------------------------------------------------------------------- time_gather

@pytest.mark.parametrize("D", [2596, 2356])
@pytest.mark.parametrize("B", [1, 3])
def test_time_gather_is_a_bit_exact_copy(vgold, B, D):
    from vge import ops, validate as V
    from vge.lib import VgeError
    g = torch.Generator().manual_seed(B * 10000 + D)
    feats = torch.randn((B, 32, D), generator=g).to(DEV)
    tables = {"identity": torch.arange(32, dtype=torch.int32).repeat(B, 1), "reverse": V.reverse_indices(B),
              "static": V.static_indices(B), "shuffle": torch.from_numpy(vgold["shuffle_1337"][:B].copy()),
              "repeated": torch.randint(0, 5, (B, 32), generator=g, dtype=torch.int32) * 7}
    for name, t in tables.items():
        t = t.to(DEV)
        want = torch.gather(feats, 1, t.long().unsqueeze(-1).expand(-1, -1, D))
        got = ops.time_gather(feats, t)
        assert torch.equal(got, want), name
    bad = tables["identity"].clone()
    bad[B - 1, 5] = 32
    with pytest.raises(VgeError, match="src entries"):
        ops.time_gather(feats, bad.to(DEV))
    bad[B - 1, 5] = -1
    with pytest.raises(VgeError, match="src entries"):
        ops.time_gather(feats, bad.to(DEV))


# ----------------------------------------------------------------------------- the two losses

LARGE_CASES = [(f"B{B}_d{d}_ten", B, d, "ten", 7 * B + d) for B in (63, 64, 257, 2048) for d in (32, 96, 256)] + \
              [("B257_d96_equal", 257, 96, "equal", 31)]
RATIOS = {}


def _check_loss(name, what, gpu, f64, r):
    assert math.isnan(gpu) == math.isnan(f64), (name, what, gpu, f64)
    if math.isnan(f64):
        return
    assert math.isfinite(gpu)
    r = max(r, _ulp32(f64))
    ratio = abs(gpu - f64) / r
    RATIOS[(name, what)] = ratio
    print(f"{name} {what}: gpu {gpu!r} f64 {f64!r} r {r:.3e} |gpu-f64|/r {ratio:.4f}")
    assert abs(gpu - f64) <= 8 * r, (name, what, gpu, f64, r)


def _run_losses(emb, neg, lab):
    from vge import ops
    e, n, y = (torch.from_numpy(a).to(DEV) for a in (emb, neg, lab))
    t1, h1 = ops.tcl_loss(e, y), ops.hardneg_loss(e, n)
    t2, h2 = ops.tcl_loss(e, y), ops.hardneg_loss(e, n)
    # the same bits on every call (a fixed summation order; NaN compared as bits)
    assert torch.equal(t1.view(torch.int64), t2.view(torch.int64))
    assert torch.equal(h1.view(torch.int64), h2.view(torch.int64))
    return float(t1), float(h1)


@pytest.mark.parametrize("case", R.fixture_cases(), ids=lambda c: c[0])
def test_losses_on_the_fixture_cases(vgold, case):
    name, B, d, kind, seed = case
    emb, neg, lab = R.case_inputs(B, d, kind, seed)
    assert np.array_equal(R.digest(emb, neg, lab), vgold[f"digest_{name}"]), "case generator drifted from the fixture"
    tcl32, tcl64, hard32, hard64 = (float(v) for v in vgold[f"loss_{name}"])
    gt, gh = _run_losses(emb, neg, lab)
    assert math.isnan(float(R.tcl(emb, lab))) == math.isnan(tcl64)
    _check_loss(name, "tcl", gt, tcl64, abs(tcl32 - tcl64))
    _check_loss(name, "hardneg", gh, hard64, abs(hard32 - hard64))


@pytest.mark.parametrize("case", LARGE_CASES, ids=lambda c: c[0])
def test_losses_on_larger_batches(case):
    name, B, d, kind, seed = case
    emb, neg, lab = R.case_inputs(B, d, kind, seed)
    tcl64, hard64 = float(R.tcl(emb, lab)), float(R.hardneg(emb, neg))
    tcl32 = float(R.tcl(emb, lab, dtype=torch.float32))
    hard32 = float(R.hardneg(emb, neg, dtype=torch.float32))
    assert math.isfinite(tcl64) and math.isfinite(hard64)
    gt, gh = _run_losses(emb, neg, lab)
    _check_loss(name, "tcl", gt, tcl64, abs(tcl32 - tcl64))
    _check_loss(name, "hardneg", gh, hard64, abs(hard32 - hard64))


# ----------------------------------------------------------------------------- centroid distance

@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("n", [1, 37])
def test_centroid_distance(n, d):
    from vge import ops
    C_ = 10
    g = torch.Generator().manual_seed(n * 1000 + d)
    emb = torch.randn((n, d), generator=g) * 3.0          # not normalised: the kernel normalises
    cent = torch.nn.functional.normalize(torch.randn((C_, d), generator=g), dim=-1)
    lab = torch.randint(0, C_, (n,), generator=g, dtype=torch.int32)
    variants = [lab]
    if n == 1:
        variants += [torch.tensor([-1], dtype=torch.int32), torch.tensor([C_], dtype=torch.int32)]
    else:
        lab[3], lab[20] = -1, C_
    for y in variants:
        want = R.centroid_distance(emb, y, cent).numpy()
        got = ops.centroid_distance(emb.to(DEV), y.to(DEV), cent.to(DEV)).cpu().numpy().astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.isnan(want).sum() == int(((y < 0) | (y >= C_)).sum())
        ok = ~np.isnan(want)
        if ok.any():
            err = float(np.abs(got[ok] - want[ok]).max())
            print(f"centroid_distance n {n} d {d}: max |gpu - f64| {err:.3e}")
            assert err <= 1e-6


# ----------------------------------------------------------------------------- the flow

def _setup(paths, device=DEV):
    """BaseExperiment.__init__'s data path once: stats from the train split, the test split's store / windows /
    labels."""
    from vge import eval as E, ops
    from vge.data import ACTION_CLASSES, NpzVideoDataset, enumerate_test_windows, train_test_split
    real = NpzVideoDataset(paths["real"], filter_classes=ACTION_CLASSES)
    train_ds, test_ds = train_test_split(real, train_ratio=0.8, seed=1337)
    label_dict = {c: i for i, c in enumerate(sorted({it.cls for it in real.items}))}
    train_store = ops.DeviceFrameStore.from_host(E.load_frame_store(train_ds.items, paths["real_kp"], False), device)
    stats = E.compute_stats_from_npz(train_ds.items, paths["real_kp"], device=device, store=train_store)
    test_store = ops.DeviceFrameStore.from_host(E.load_frame_store(test_ds.items, paths["real_kp"], True), device)
    samples = enumerate_test_windows(test_ds, 32, 8)
    windows = E._window_tensor(samples, {it.path: i for i, it in enumerate(test_ds.items)}, device)
    labels = torch.as_tensor([label_dict[it.cls] for it, _ in samples], dtype=torch.int32, device=device)
    return dict(train_items=train_ds.items, label_dict=label_dict, train_store=train_store, stats=stats,
                test_store=test_store, windows=windows, labels=labels)


@pytest.fixture(scope="module")
def flow_setup(golden_dataset):
    paths, ckpt = golden_dataset
    return paths, ckpt, _setup(paths)


def _validate(paths, ckpt, s, compute, batch, tables):
    from vge import eval as E, validate as V
    dims_raw, dims_diff = E.infer_dims_from_stats(s["stats"])
    model = E.load_model(ckpt, dims_raw, dims_diff, device=DEV, compute=compute)
    cents, _, _ = E.build_real_centroids(model, paths["real"], paths["real_kp"], s["stats"], 32, 8, DEV,
                                         train_items=s["train_items"], label_dict=s["label_dict"],
                                         store=s["train_store"])
    n = int(s["windows"].shape[0])
    tabs = [torch.from_numpy(tables[b0:b0 + batch].astype(np.int32)) for b0 in range(0, n, batch)]
    return V.validate_checkpoint(model, s["test_store"], s["windows"], s["labels"], s["stats"], centroids=cents,
                                 batch=batch, shuffle_tables=tabs, label_dict=s["label_dict"])


def _check_flow(vgold, run, out, tag):
    counted, skipped = (int(v) for v in vgold[f"flow_{run}_counts"])
    assert (out["n_batches"], out["skipped_batches"]) == (counted, skipped)
    f64, r, up = vgold[f"flow_{run}_f64"], vgold[f"flow_{run}_r"], vgold[f"flow_{run}_up"]
    if counted == 0:
        assert out["loss"] == float("inf") == float(up[0]) and out["components"] == {}
    else:
        got = [out["loss"]] + [out["components"][k] for k in R.COMPONENTS]
        for k, g, w, rc in zip(("loss",) + R.COMPONENTS, got, f64, r):
            print(f"{tag} {run} {k}: gpu {g!r} f64 {float(w)!r} r_c {float(rc):.3e} |gpu-f64|/r_c "
                  f"{abs(g - float(w)) / float(rc):.4f}")
        for k, g, w, rc in zip(("loss",) + R.COMPONENTS, got, f64, r):
            assert abs(g - float(w)) <= 4 * float(rc), (tag, run, k, g, float(w), float(rc))
    # centroid distances: unit vectors whose embeddings the encoder tests hold to 2e-5 of the reference
    cd = vgold[f"flow_{run}_cd_f64"]
    print(f"{tag} {run} centroid_distance: gpu {out['centroid_distance']!r} f64 {float(cd[0])!r}")
    assert abs(out["centroid_distance"] - float(cd[0])) <= 2e-5
    assert len(out["class_distances"]) == int((~np.isnan(cd[1:])).sum())


@pytest.mark.parametrize("batch", [2048, R.FLOW_SMALL_BATCH])
@pytest.mark.parametrize("compute", ["f32x3", "f32"])
def test_flow_on_the_golden_dataset(vgold, flow_setup, compute, batch):
    """Measured on an MI355X (batch 10, |gpu - f64| / r_c per component): see DESIGN.md "Checkpoint validation"."""
    paths, ckpt, s = flow_setup
    run = f"b{batch}"
    if batch == R.FLOW_SMALL_BATCH:
        counted, skipped = vgold[f"flow_{run}_counts"]
        assert counted >= 3 and skipped >= 1          # the condition the fixture was generated under
    out = _validate(paths, ckpt, s, compute, batch, vgold[f"flow_{run}_tables"])
    _check_flow(vgold, run, out, compute)


def test_flow_small_checkpoint(vgold, golden_dataset_small):
    """The d_model 64 / 2-layer / 4-head checkpoint through the generic exact-f32 kernels."""
    paths, ckpt = golden_dataset_small
    run = f"small_b{R.FLOW_SMALL_BATCH}"
    out = _validate(paths, ckpt, _setup(paths), "f32", R.FLOW_SMALL_BATCH, vgold[f"flow_{run}_tables"])
    _check_flow(vgold, run, out, "small f32")


def test_rank_checkpoints_orders_like_the_float64_flow(vgold, golden_dataset, tmp_path, monkeypatch):
    from tests.golden.dataset_spec import golden_state_dict
    from vge import eval as E, synth, validate as V
    paths, ckpt = golden_dataset
    pert = str(tmp_path / "model_perturbed.pt")
    synth.save_checkpoint(pert, R.perturbed_state_dict(golden_state_dict("kp")))
    calls = []
    real_stats = E.compute_stats_from_npz

    def counting(*a, **k):
        calls.append(1)
        return real_stats(*a, **k)
    monkeypatch.setattr(E, "compute_stats_from_npz", counting)
    ranking = V.rank_checkpoints(paths["real"], paths["real_kp"], [ckpt, pert], compute="f32x3",
                                 batch=R.FLOW_SMALL_BATCH, device=DEV)
    assert len(calls) == 1                               # the stats are built once for all checkpoints
    assert sorted(r["checkpoint"] for r in ranking) == sorted([ckpt, pert])
    f64 = {ckpt: float(vgold["flow_b10_f64"][0]), pert: float(vgold["flow_b10_perturbed_f64"][0])}
    assert [r["checkpoint"] for r in ranking] == sorted(f64, key=f64.get)
    assert ranking[0]["loss"] <= ranking[1]["loss"]
    for r in ranking:
        print(f"rank {r['checkpoint'].rsplit('/', 1)[-1]}: gpu {r['loss']!r} f64 {f64[r['checkpoint']]!r}")
        assert r["n_batches"] == int(vgold["flow_b10_counts"][0])
