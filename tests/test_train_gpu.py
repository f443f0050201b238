"""Training on the GPU: the loss gradients of vge_validate.hip (vge_tcl_loss_grad, vge_hardneg_loss_grad) through
vge.ops and vge.losses, the training step and train() itself, against float64 autograd of tests/validate_ref.py on
the CPU and the reference's own recorded steps (tests/golden/train_golden.npz).

Tolerances.  A gradient tensor must lie within 8 r of the float64 autograd, max over its elements, r being the
distance of the float32 CPU autograd from the float64 one on the same inputs, floored at one float32 ulp of the
largest float64 gradient magnitude (DESIGN.md 5d's convention).  Ratios measured on an MI355X are in DESIGN.md 5e."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import train_ref as TR
from tests import validate_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64            # floats before and after a gradient buffer (a multiple of 4: the buffer stays 16-byte aligned)
SENTINEL = -12345.0


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def _guarded(B, d):
    buf = torch.full((B * d + 2 * GUARD,), SENTINEL, device=DEV)
    return buf, buf[GUARD:GUARD + B * d].view(B, d)


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _check_grad(name, what, gpu, f64, f32):
    r = max(float(np.abs(f32.astype(np.float64) - f64).max()), _ulp32(np.abs(f64).max()))
    err = float(np.abs(gpu.astype(np.float64) - f64).max())
    print(f"{name} {what}: max|gpu-f64| {err:.3e} r {r:.3e} ratio {err / r:.4f}")
    assert np.isfinite(gpu).all(), (name, what)
    assert err <= 8 * r, (name, what, err, r)


# ----------------------------------------------------------------------------- vge_tcl_loss_grad

def _shape_labels(B, kind):
    if kind == "one":
        return np.zeros(B, np.int32)
    if kind == "two":
        return (np.arange(B) % 2).astype(np.int32)
    if kind == "522":
        return np.array([0] * 5 + [1] * 2 + [2] * 2, np.int32)[np.random.default_rng(9).permutation(9)]
    if kind == "pk":
        return np.repeat(np.arange(10, dtype=np.int32), 24)[np.random.default_rng(240).permutation(240)]
    return R.make_labels(B, "ten", 7 * B)


TCL_SHAPES = [(2, 32, "one"), (4, 32, "two"), (9, 96, "522"), (6, 32, "one"), (240, 256, "pk"), (257, 32, "ten"),
              (2048, 256, "ten")]


def _run_tcl(name, emb, lab):
    from vge import ops
    e, y = torch.from_numpy(emb).to(DEV), torch.from_numpy(lab).to(DEV)
    B, d = emb.shape
    buf, grad = _guarded(B, d)
    loss, g = ops.tcl_loss_grad(e, y, grad=grad)
    assert g.data_ptr() == grad.data_ptr()
    first = g.clone()
    loss2, g2 = ops.tcl_loss_grad(e, y)
    fwd = ops.tcl_loss(e, y)
    assert _guards_intact(buf), name
    # the forward's bits (NaN compared as bits), and the same bits on every call
    assert torch.equal(loss.view(torch.int64), fwd.view(torch.int64)), name
    assert torch.equal(loss.view(torch.int64), loss2.view(torch.int64)), name
    assert torch.equal(first.view(torch.int32), g2.view(torch.int32)), name
    return float(loss), first.cpu().numpy()


@pytest.mark.parametrize("case", R.fixture_cases(), ids=lambda c: c[0])
def test_tcl_grad_on_the_fixture_cases(case):
    name, B, d, kind, seed = case
    emb, _, lab = R.case_inputs(B, d, kind, seed)
    l64, g64 = TR.tcl_autograd(emb, lab, torch.float64)
    loss, g = _run_tcl(name, emb, lab)
    assert math.isnan(loss) == math.isnan(l64), (name, loss, l64)
    if math.isnan(l64):
        assert kind == "singleton" or B == 1      # the NaN rule: a label that appears once, and B = 1
        return
    _, g32 = TR.tcl_autograd(emb, lab, torch.float32)
    _check_grad(name, "tcl grad", g, g64, g32)


@pytest.mark.parametrize("shape", TCL_SHAPES, ids=lambda s: f"B{s[0]}_d{s[1]}_{s[2]}")
def test_tcl_grad_shapes(shape):
    B, d, kind = shape
    name = f"B{B}_d{d}_{kind}"
    lab = _shape_labels(B, kind)
    emb = R.make_embeddings(B, d, lab, 31 * B + d)
    l64, g64 = TR.tcl_autograd(emb, lab, torch.float64)
    _, g32 = TR.tcl_autograd(emb, lab, torch.float32)
    assert math.isfinite(l64)
    loss, g = _run_tcl(name, emb, lab)
    assert abs(loss - l64) <= 1e-9 * abs(l64)
    _check_grad(name, "tcl grad", g, g64, g32)


def test_tcl_grad_refuses_what_the_kernels_do_not_take():
    from vge import ops
    from vge.lib import VgeError
    e = torch.zeros((4, 32), device=DEV)
    y = torch.zeros((4,), dtype=torch.int32, device=DEV)
    with pytest.raises(VgeError, match="emb"):
        ops.tcl_loss_grad(e.double(), y)
    with pytest.raises(VgeError, match="labels"):
        ops.tcl_loss_grad(e, y.long())
    with pytest.raises(VgeError, match="labels"):
        ops.tcl_loss_grad(e, y[:3])
    with pytest.raises(VgeError, match="grad"):
        ops.tcl_loss_grad(e, y, grad=torch.zeros((4, 64), device=DEV))
    with pytest.raises(VgeError, match="d must be"):
        ops.tcl_loss_grad(torch.zeros((4, 48), device=DEV), y)


# ----------------------------------------------------------------------------- vge_hardneg_loss_grad

def _hardneg_inputs(B, d):
    """Unit anchors and hard negatives (validate_ref's), with the rows the closed form bends at: neg = anchor
    (p = 0.5), neg = 3 anchor (margin / temperature = +28.6) and neg = -anchor (-28.6)."""
    rng = np.random.default_rng(B * 1000 + d)
    a = rng.standard_normal((B, d))
    a = (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    n = a.astype(np.float64) + (0.5 / np.sqrt(d)) * rng.standard_normal((B, d))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    n[0] = a[0]
    if B > 2:
        n[1], n[2] = 3.0 * a[1], -a[2]
    return np.ascontiguousarray(a), np.ascontiguousarray(n)


@pytest.mark.parametrize("shape", [(1, 4), (5, 36), (240, 256), (2048, 256)], ids=lambda s: f"B{s[0]}_d{s[1]}")
def test_hardneg_grad(shape):
    from vge import ops
    B, d = shape
    name = f"B{B}_d{d}"
    a, n = _hardneg_inputs(B, d)
    l64, ga64, gn64 = TR.hardneg_autograd(a, n, torch.float64)
    _, ga32, gn32 = TR.hardneg_autograd(a, n, torch.float32)
    ta, tn = torch.from_numpy(a).to(DEV), torch.from_numpy(n).to(DEV)
    bufa, ga = _guarded(B, d)
    bufn, gn = _guarded(B, d)
    loss, _, _ = ops.hardneg_loss_grad(ta, tn, grad_anchor=ga, grad_neg=gn)
    ga1, gn1 = ga.clone(), gn.clone()
    loss2, ga2, gn2 = ops.hardneg_loss_grad(ta, tn)
    fwd = ops.hardneg_loss(ta, tn)
    assert _guards_intact(bufa) and _guards_intact(bufn)
    assert torch.equal(loss.view(torch.int64), fwd.view(torch.int64))
    assert torch.equal(loss.view(torch.int64), loss2.view(torch.int64))
    assert torch.equal(ga1.view(torch.int32), ga2.view(torch.int32))
    assert torch.equal(gn1.view(torch.int32), gn2.view(torch.int32))
    assert abs(float(loss) - l64) <= 1e-9 * abs(l64)
    _check_grad(name, "hardneg grad_anchor", ga1.cpu().numpy(), ga64, ga32)
    _check_grad(name, "hardneg grad_neg", gn1.cpu().numpy(), gn64, gn32)


def test_hardneg_grad_refuses_what_the_kernel_does_not_take():
    from vge import ops
    from vge.lib import VgeError
    a = torch.zeros((4, 8), device=DEV)
    with pytest.raises(VgeError, match="anchor"):
        ops.hardneg_loss_grad(a.double(), a.clone())
    with pytest.raises(VgeError, match="neg"):
        ops.hardneg_loss_grad(a, torch.zeros((4, 12), device=DEV))
    with pytest.raises(VgeError, match="grad_neg"):
        ops.hardneg_loss_grad(a, a.clone(), grad_neg=torch.zeros((3, 8), device=DEV))
    with pytest.raises(VgeError, match="d a positive multiple of 4"):
        ops.hardneg_loss_grad(torch.zeros((4, 6), device=DEV), torch.zeros((4, 6), device=DEV))


# ----------------------------------------------------------------------------- the autograd functions

@functools.lru_cache(maxsize=None)
def _step_loss_inputs(B, d):
    lab = _shape_labels(B, "pk") if B == 240 else R.make_labels(B, "ten", 3 * B)
    emb = R.make_embeddings(B, d, lab, B + d)
    rng = np.random.default_rng(B)
    negs = []
    for k in range(3):
        n = emb.astype(np.float64) + ((0.3 + 0.2 * k) / np.sqrt(d)) * rng.standard_normal((B, d))
        negs.append(np.ascontiguousarray((n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)))
    return emb, negs, lab


def _total_backward(backend, dtype, device, emb, negs, lab, upstream):
    from vge import losses
    e = torch.from_numpy(emb).to(device=device, dtype=dtype).requires_grad_(True)
    ns = [torch.from_numpy(n).to(device=device, dtype=dtype).requires_grad_(True) for n in negs]
    y = torch.from_numpy(lab).to(device)
    tcl, hard = losses.TCL(backend=backend), losses.SupConWithHardNegatives(backend=backend)
    total = tcl(e, y) + 10.0 * (hard(e, e, ns[0]) + hard(e, e, ns[1]) + hard(e, e, ns[2]))
    (total * upstream).backward()
    return float(total.detach()), [t.grad.detach().cpu().numpy() for t in [e] + ns]


@pytest.mark.parametrize("shape", [(24, 64), (240, 256)], ids=lambda s: f"B{s[0]}_d{s[1]}")
def test_autograd_functions_match_the_torch_backend(shape):
    """(tcl + 10 (h1 + h2 + h3)).backward() under a non-unit upstream scalar: the HIP route's gradients equal the
    torch backend's on the device within the bar of the kernels, measured against float64 autograd on the CPU."""
    emb, negs, lab = _step_loss_inputs(*shape)
    up = 0.37
    l64, g64 = _total_backward("torch", torch.float64, "cpu", emb, negs, lab, up)
    _, g32 = _total_backward("torch", torch.float32, "cpu", emb, negs, lab, up)
    lhip, ghip = _total_backward("hip", torch.float32, DEV, emb, negs, lab, up)
    ltor, gtor = _total_backward("torch", torch.float32, DEV, emb, negs, lab, up)
    assert abs(lhip - l64) <= 1e-9 * abs(l64) and abs(ltor - l64) <= 1e-4 * abs(l64)
    for what, gh, gt, w64, w32 in zip(("emb", "neg1", "neg2", "neg3"), ghip, gtor, g64, g32):
        r = max(float(np.abs(w32.astype(np.float64) - w64).max()), _ulp32(np.abs(w64).max()))
        print(f"B{shape[0]} {what}: hip-f64 {np.abs(gh - w64).max() / r:.3f} r, torch(dev)-f64 "
              f"{np.abs(gt - w64).max() / r:.3f} r, hip-torch(dev) {np.abs(gh.astype(np.float64) - gt).max() / r:.3f} r")
        assert np.abs(gh.astype(np.float64) - w64).max() <= 8 * r
        assert np.abs(gh.astype(np.float64) - gt).max() <= 8 * r


def test_loss_modules_refuse_bad_arguments():
    from vge import losses
    from vge.lib import VgeError
    e = torch.zeros((4, 32), device=DEV, requires_grad=True)
    y = torch.zeros((4,), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="backend"):
        losses.TCL(backend="triton")
    with pytest.raises(ValueError, match="targets"):
        losses.TCL()(e, y[:3])
    with pytest.raises(ValueError, match="projections must be float32"):
        losses.TCL()(e.double(), y)
    with pytest.raises(VgeError, match="d must be"):
        losses.TCL()(torch.zeros((4, 48), device=DEV), y)
    with pytest.raises(ValueError, match="hard_negative"):
        losses.SupConWithHardNegatives()(e, e, torch.zeros((4, 16), device=DEV))
    with pytest.raises(ValueError, match="float32"):
        losses.SupConWithHardNegatives()(e, e, torch.zeros((4, 32), device=DEV, dtype=torch.float64))
    with pytest.raises(VgeError, match="d a positive multiple of 4"):
        a = torch.zeros((4, 6), device=DEV)
        losses.SupConWithHardNegatives()(a, a, a.clone())


# ----------------------------------------------------------------------------- the training step

@pytest.fixture(scope="module")
def tgold():
    from tests.conftest import GOLDEN
    return dict(np.load(GOLDEN / "train_golden.npz"))


@pytest.fixture(scope="module")
def train_setup(golden_dataset):
    """The data path of vge.train on the golden real set, built once: the train split's windows and labels."""
    from vge import eval as E, validate as V
    from vge.data import sample_all_windows_npz
    paths, _ = golden_dataset
    dp = V.build_data_path(paths["real"], paths["real_kp"], device=DEV)
    samples = sample_all_windows_npz(dp.train_ds, 32, 8)
    windows = E._window_tensor(samples, {it.path: i for i, it in enumerate(dp.train_ds.items)}, DEV)
    labels = torch.as_tensor([dp.label_dict[it.cls] for it, _ in samples], dtype=torch.int64)

    def feats_of(b):
        from vge import ops
        return ops.featurize(dp.train_store, windows[b.to(DEV)], dp.stats.mean, dp.stats.std, layout=dp.stats.layout)
    return dp, feats_of, labels


_STEPPED = {}


def _four_steps(tgold, train_setup, ckpt):
    """The four recorded steps with loss_backend "hip", run once per checkpoint and shared by the two tests below."""
    if ckpt not in _STEPPED:
        _, feats_of, labels = train_setup
        _STEPPED[ckpt] = TR.run_steps(tgold, ckpt, feats_of, labels, DEV, "hip")
    return _STEPPED[ckpt]


@pytest.mark.parametrize("ckpt", ["kp", "small"])
def test_four_steps_reproduce_the_reference(tgold, train_setup, ckpt):
    """Fixture (c) with loss_backend "hip" under the bars of the CPU test: components within factor r_k, gradient
    norms and the small tensors' gradients within factor r_g (factor 8 for "kp", 16 for "small").

    Measured on an MI355X, largest |gpu - f64| / r:
      kp     components 3.05, small tensors 1.03, gradient norms 2.15 (state_enc.pose.blocks.0.norm.bias); bar 8
      small  components 2.85, small tensors 1.56, gradient norms 15.7 (state_enc.global.blocks.3.norm.weight, a
             tensor whose r sits at its floor of one float32 ulp); bar 16
    The module's attention takes the "math" route of scaled_dot_product_attention (vge/model.py): with torch's fused
    attention kernels two gradient norms of "kp" were 8.67 r and 8.11 r away."""
    comps, grads, _ = _four_steps(tgold, train_setup, ckpt)
    TR.check_steps(tgold, ckpt, comps, grads, "gpu hip")


@pytest.mark.parametrize("ckpt,compute", [("kp", "f32x3"), ("small", "f32")])
def test_trained_state_dict_round_trips_into_the_kernels(tgold, train_setup, ckpt, compute):
    """After the four steps the module's state dict goes into the hand-written forward, whose embeddings of one
    featurised batch lie within 2e-5 of the module's eval-mode embeddings."""
    from tests.golden.dataset_spec import SMALL_HP
    from vge import eval as E
    dp, feats_of, _ = train_setup
    _, _, m = _four_steps(tgold, train_setup, ckpt)
    hp = dict(SMALL_HP) if ckpt == "small" else {"d_model": 256, "time_layers": 4, "time_heads": 8}
    enc = E.load_model((m.numpy_state_dict(), hp), dp.dims_raw, dp.dims_diff, device=DEV, compute=compute)
    assert enc.compute == compute
    feats = feats_of(torch.from_numpy(tgold[f"steps_{ckpt}_batches"][0].astype(np.int64)))
    m.eval()
    with torch.no_grad():
        want = m(feats)[0]
    m.train()
    got, _, _ = enc.encode(feats, tc=False)
    err = float((got - want).abs().max())
    print(f"{ckpt} {compute}: kernel vs module seq_embed after four steps, max|err| {err:.3e}")
    assert err <= 2e-5


def test_overfits_one_batch_with_the_hip_loss(tgold, train_setup):
    _, feats_of, labels = train_setup
    comps, _, _ = TR.run_steps(tgold, "kp", feats_of, labels, DEV, "hip", n_steps=21, tables_key="overfit_tables",
                               batches=tgold["steps_kp_batches"][:1])
    loss = comps.sum(axis=1)
    print(f"overfit (hip): step 0 {loss[0]:.4f} (reference {tgold['overfit_loss'][0]:.4f}), step 20 {loss[20]:.4f} "
          f"(reference {tgold['overfit_loss'][1]:.4f})")
    assert int(tgold["overfit_lower"][0]) == 1 and loss[20] < loss[0]


# ----------------------------------------------------------------------------- train()

def test_train_two_epochs_on_the_golden_set(golden_dataset, tmp_path):
    import json
    from vge import eval as E, train as T, validate as V
    paths, _ = golden_dataset
    save = tmp_path / "run"
    recs = T.train(paths["real"], paths["real_kp"], str(save), epochs=2, P=4, K=3, dropout=0.0,
                   eval_batch=R.FLOW_SMALL_BATCH, device=DEV)
    assert [r["epoch"] for r in recs] == [1, 2]
    with open(save / "label_mapping.json") as f:
        assert len(json.load(f)) == 10
    saved = sorted(save.glob("best_eval_epoch*_loss*.pt"))
    assert saved and recs[0]["checkpoint"] == str(saved[0])
    for r in recs:
        print({k: r[k] for k in ("epoch", "train_loss", "steps", "skipped_steps", "eval_loss", "n_batches",
                                 "skipped_batches", "centroid_distance", "validated_by", "checkpoint")})
        assert r["validated_by"] == "kernels" and r["n_batches"] >= 3 and r["steps"] + r["skipped_steps"] > 0
        assert math.isfinite(r["train_loss"]) and math.isfinite(r["eval_loss"]) and set(r["components"]) == set(R.COMPONENTS)
    dp = V.build_data_path(paths["real"], paths["real_kp"], device=DEV)
    for r in recs:
        if r["checkpoint"] is None:
            continue
        assert f"epoch{r['epoch']:03d}_loss{r['eval_loss']:.4f}" in r["checkpoint"]
        assert isinstance(E.load_model(r["checkpoint"], dp.dims_raw, dp.dims_diff, device=DEV), E.ops.Encoder)
        again = V.rank_checkpoints(paths["real"], paths["real_kp"], [r["checkpoint"]], batch=R.FLOW_SMALL_BATCH,
                                   device=DEV)[0]
        assert again["loss"] == r["eval_loss"] and again["n_batches"] == r["n_batches"]


def test_train_goes_on_when_the_kernels_refuse_the_shape(golden_dataset, tmp_path):
    """d_model 96 with one head (head dim 96 > 64) is a shape ops.Encoder refuses: the epoch is
    validated through the torch module, its record says so, and the checkpoint is still written."""
    from vge import train as T
    paths, _ = golden_dataset
    recs = T.train(paths["real"], paths["real_kp"], str(tmp_path / "run"), epochs=1, P=4, K=3, dropout=0.0,
                   eval_batch=R.FLOW_SMALL_BATCH, device=DEV,
                   model_kwargs={"d_model": 96, "time_layers": 1, "time_heads": 1})
    (r,) = recs
    print({k: r[k] for k in ("train_loss", "steps", "eval_loss", "n_batches", "centroid_distance", "validated_by")})
    assert r["validated_by"] == "module" and "VGE_ERR_UNSUPPORTED" in r["kernels_refused"]
    assert r["steps"] > 0 and math.isfinite(r["eval_loss"]) and r["n_batches"] >= 3
    assert r["checkpoint"] is not None and len(list((tmp_path / "run").glob("best_eval_epoch001_*.pt"))) == 1
