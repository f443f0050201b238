"""Checkpoint validation (vge.validate), the parts that need no GPU: the shuffle tables against the reference's own,
the float64 restatement against the reference's float32 losses, the skip rule, the CLI and the C ABI's argument
checks (fixtures: tests/golden/validate_golden.npz, written by tests/golden/make_validate_golden.py)."""
import ctypes as C
import json
import math
import types

import numpy as np
import pytest
import torch

from tests import validate_ref as R
from tests.conftest import GOLDEN

SYMBOLS = ("vge_time_gather", "vge_tcl_workspace_bytes", "vge_tcl_loss", "vge_hardneg_loss", "vge_centroid_distance")


@pytest.fixture(scope="module")
def vgold():
    return dict(np.load(GOLDEN / "validate_golden.npz"))


# ----------------------------------------------------------------------------- index tables

@pytest.mark.parametrize("seed", [1337, 7])
def test_partial_shuffle_indices_equal_the_reference(vgold, seed):
    from vge.validate import partial_shuffle_indices
    want = torch.from_numpy(vgold[f"shuffle_{seed}"])
    torch.manual_seed(seed)                       # generator None: torch's global generator, as the reference
    got = partial_shuffle_indices(5, 32)
    assert got.dtype == torch.int32 and torch.equal(got, want)
    got = partial_shuffle_indices(5, 32, generator=torch.Generator().manual_seed(seed))
    assert torch.equal(got, want)
    # 22 of 32 positions are permuted among themselves: every row is a permutation of 0..31
    assert torch.equal(got.sort(dim=1).values, torch.arange(32, dtype=torch.int32).repeat(5, 1))


def test_reverse_and_static_tables():
    from vge.validate import reverse_indices, static_indices
    x = torch.arange(3 * 32 * 2, dtype=torch.float32).view(3, 32, 2)

    def gather(t):
        return torch.gather(x, 1, t.long().unsqueeze(-1).expand(-1, -1, 2))
    assert torch.equal(gather(reverse_indices(3)), torch.flip(x, dims=[1]))
    assert torch.equal(gather(static_indices(3)), x[:, :1].expand(-1, 32, -1))


def test_recorded_tables_follow_the_seed(vgold):
    """What make_validate_golden.py found: the reference's make_test_loader hands the DataLoader its own generator,
    so creating the loader's iterator draws nothing from the global generator and torch.manual_seed(1337) before
    evaluate_test_set reproduces the tables it draws."""
    from vge.validate import partial_shuffle_indices
    assert int(vgold["tables_follow_manual_seed"][0]) == 1
    t = vgold["flow_b10_tables"]
    mine = partial_shuffle_indices(t.shape[0], 32, generator=torch.Generator().manual_seed(1337))
    assert np.array_equal(mine.numpy(), t.astype(np.int32))


# ----------------------------------------------------------------------------- the restatement against the reference

@pytest.mark.parametrize("case", R.fixture_cases(), ids=lambda c: c[0])
def test_float64_restatement_agrees_with_the_reference(vgold, case):
    name, B, d, kind, seed = case
    emb, neg, lab = R.case_inputs(B, d, kind, seed)
    assert np.array_equal(R.digest(emb, neg, lab), vgold[f"digest_{name}"]), "case generator drifted from the fixture"
    tcl32, tcl64, hard32, hard64 = vgold[f"loss_{name}"]
    for got, f32, f64 in ((float(R.tcl(emb, lab)), tcl32, tcl64), (float(R.hardneg(emb, neg)), hard32, hard64)):
        assert math.isnan(got) == math.isnan(f32) == math.isnan(f64), (got, f32, f64)
        if math.isnan(got):
            continue
        assert math.isfinite(got) and math.isfinite(f32)
        assert abs(got - f64) <= 1e-12 * abs(f64)
        # float32 rounding level: the reference sums B float32 terms of this size per row and B rows; 16 ulps of the
        # value covers the worst fixture case (B = 300) with room (measured: below 1 ulp)
        assert abs(got - f32) <= 16 * float(np.spacing(np.float32(abs(f32)))), (got, f32)
    expect_nan = kind == "singleton" or B == 1
    assert math.isnan(tcl32) == expect_nan
    assert math.isfinite(hard32)


def test_float32_restatement_is_the_reference_arithmetic(vgold):
    """The float32 mode of the restatement (the tolerance unit of the larger GPU cases) lands where the reference's
    own float32 run did."""
    for name, B, d, kind, seed in R.fixture_cases():
        emb, neg, lab = R.case_inputs(B, d, kind, seed)
        tcl32, _, hard32, _ = vgold[f"loss_{name}"]
        a, b = float(R.tcl(emb, lab, dtype=torch.float32)), float(R.hardneg(emb, neg, dtype=torch.float32))
        assert math.isnan(a) == math.isnan(tcl32)
        if not math.isnan(a):
            assert abs(a - tcl32) <= 4 * float(np.spacing(np.float32(abs(tcl32))))
        assert abs(b - hard32) <= 4 * float(np.spacing(np.float32(abs(hard32))))


def test_tcl_broadcast_divides_by_the_column_denominator():
    """The quirk stated literally: element (i,j) is divided by row j's denominator.  With unequal class sizes the
    row-i reading gives another number."""
    emb, _, _ = R.case_inputs(7, 32, "ten", 5)
    lab = np.array([0, 0, 0, 0, 1, 1, 1], np.int32)
    z = torch.from_numpy(emb).double()
    t = torch.from_numpy(lab).long()
    dot = z @ z.T
    e, en = torch.exp(dot / 0.1), torch.exp(-dot)
    same = (t[:, None] == t[None, :])
    pos = same & ~torch.eye(7, dtype=torch.bool)
    den = (e * pos).sum(1) + 5000.0 * (en * pos).sum(1) + (e * ~same).sum(1)
    by_col = (-torch.log(e / den[None, :]) * pos).sum(1) / pos.sum(1)
    by_row = (-torch.log(e / den[:, None]) * pos).sum(1) / pos.sum(1)
    got = R.tcl(emb, lab)
    assert abs(float(got) - float(by_col.mean())) < 1e-12
    # the per-row losses differ between the two readings ...
    assert float((by_col - by_row).abs().max()) > 1e-6
    # ... but their means agree up to rounding: j in P(i) implies |P(i)| = |P(j)| and e is symmetric, so the double
    # sum over positive pairs is the same either way.  The quirk reorders the sum; it does not change the loss.
    assert abs(float(by_col.mean()) - float(by_row.mean())) < 1e-12


# ----------------------------------------------------------------------------- the skip rule

def test_skip_rule_and_averaging():
    from vge.validate import _reduce_batches
    seq = [[1.0, 2.0, 3.0, 4.0], [float("nan"), 1.0, 1.0, 1.0], [3.0, 2.0, 1.0, 0.0], [1.0, float("inf"), 1.0, 1.0]]
    out = _reduce_batches(seq)
    assert out["n_batches"] == 2 and out["skipped_batches"] == 2
    assert out["loss"] == pytest.approx((10.0 + 6.0) / 2)
    assert out["components"] == {"tcl": 2.0, "hard_shuf": 2.0, "hard_rev": 2.0, "hard_stat": 2.0}
    ref = R.reduce_batches(seq)
    assert (out["loss"], out["components"], out["n_batches"], out["skipped_batches"]) == ref
    none = _reduce_batches([[float("nan"), 0.0, 0.0, 0.0]])
    assert none == {"loss": float("inf"), "components": {}, "n_batches": 0, "skipped_batches": 1}


class _StubModel:
    layout, d_model, feat_dim = "kp", 8, 16

    def __init__(self):
        self.encodes, self.status_checks = 0, 0

    def reserve(self, n):
        pass

    def encode(self, feats, frame_embed=False, tc=True, seq_out=None, tc_out=None):
        self.encodes += 1
        seq_out.zero_()
        return seq_out, None, None

    def status(self):
        self.status_checks += 1


def test_validate_checkpoint_skips_non_finite_batches(monkeypatch):
    """The flow on stubbed device calls: 3 batches of which the second has a NaN TCL; four encodes and three gathers
    per batch; the hard-negative weight applied; the status word checked once at the end."""
    from vge import ops, validate as V
    tcl_seq = iter([1.0, float("nan"), 3.0])
    calls = {"gather": 0, "tables": []}
    monkeypatch.setattr(ops, "featurize", lambda store, w, mean, std, out=None, layout="kp": out)

    def gather(f, table, out=None):
        calls["gather"] += 1
        calls["tables"].append(table.clone())
        return out
    monkeypatch.setattr(ops, "time_gather", gather)
    monkeypatch.setattr(ops, "tcl_loss", lambda e, y, t, k1, k2, out=None: out.fill_(next(tcl_seq)))
    monkeypatch.setattr(ops, "hardneg_loss", lambda a, n, t, out=None: out.fill_(0.5))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda dev=None: None)
    model = _StubModel()
    stats = types.SimpleNamespace(layout="kp", mean=None, std=None)
    windows = torch.zeros((10, 2), dtype=torch.int32)
    labels = torch.zeros(10, dtype=torch.int32)
    tables = [torch.arange(32, dtype=torch.int32).repeat(b, 1) for b in (4, 4, 2)]
    out = V.validate_checkpoint(model, None, windows, labels, stats, batch=4, shuffle_tables=tables, hard_weight=10.0)
    assert out["n_batches"] == 2 and out["skipped_batches"] == 1
    assert out["components"] == {"tcl": 2.0, "hard_shuf": 5.0, "hard_rev": 5.0, "hard_stat": 5.0}
    assert out["loss"] == pytest.approx(17.0)
    assert model.encodes == 12 and calls["gather"] == 9 and model.status_checks == 1
    assert torch.equal(calls["tables"][1], V.reverse_indices(4)) and torch.equal(calls["tables"][2], V.static_indices(4))
    with pytest.raises(ValueError, match="shuffle tables"):
        V.validate_checkpoint(model, None, windows, labels, stats, batch=4, shuffle_tables=tables[:2])


# ----------------------------------------------------------------------------- the command line

def test_cli_writes_a_sorted_ranking(monkeypatch, tmp_path, capsys):
    """python -m vge.validate with the device work stubbed: one line per checkpoint, a JSON list sorted by loss, a
    refused checkpoint reported with its error and ranked last; stats and stores are built once."""
    from vge import eval as E, ops, synth, validate as V
    from vge.lib import UnsupportedModelError
    paths = synth.write_dataset(str(tmp_path / "ds"), n_real_per_class=3, n_gen=1, T_real=(32, 40))
    built = {"stats": 0, "stores": 0, "seeds": []}

    def from_host(st, device):
        built["stores"] += 1
        return types.SimpleNamespace(n_videos=len(st.names))

    def stats_fn(items, kp_dir, device="cuda", store=None, reduce_fn=None):
        built["stats"] += 1
        return types.SimpleNamespace(layout="kp")
    monkeypatch.setattr(ops.DeviceFrameStore, "from_host", staticmethod(from_host))
    monkeypatch.setattr(E, "compute_stats_from_npz", stats_fn)

    def load_model(ck, dims_raw, dims_diff, device="cuda", compute="f32x3"):
        if "odd" in str(ck):
            raise UnsupportedModelError("vge_encoder_create failed: VGE_ERR_UNSUPPORTED: d_model 48")
        return types.SimpleNamespace(name=str(ck))
    monkeypatch.setattr(E, "load_model", load_model)
    monkeypatch.setattr(E, "build_real_centroids", lambda model, *a, **k: (torch.zeros(10, 4), None, None))
    losses = {"a.pt": 3.0, "b.pt": 1.0, "c.pt": 2.0}

    def validate(model, store, windows, labels, stats, centroids=None, batch=2048, shuffle_tables=None, generator=None,
                 hard_weight=10.0, label_dict=None):
        built["seeds"].append(generator.initial_seed())
        assert windows.dtype == torch.int32 and windows.shape[1] == 2 and labels.shape[0] == windows.shape[0]
        assert batch == 64 and sorted(label_dict.values()) == list(range(10))
        return {"loss": losses[model.name], "components": dict.fromkeys(V.COMPONENTS, losses[model.name] / 4),
                "n_batches": 1, "skipped_batches": 0, "centroid_distance": 0.5, "class_distances": {}}
    monkeypatch.setattr(V, "validate_checkpoint", validate)
    out = tmp_path / "ranking.json"
    rc = V.main(["--real-meshes", paths["real"], "--real-kp", paths["real_kp"], "--kp-layout", "per_class",
                 "--batch", "64", "--device", "cpu", "--out", str(out), "a.pt", "odd.pt", "b.pt", "c.pt"])
    assert rc == 0
    ranking = json.loads(out.read_text())
    assert [r["checkpoint"] for r in ranking] == ["b.pt", "c.pt", "a.pt", "odd.pt"]
    assert [r["loss"] for r in ranking[:3]] == [1.0, 2.0, 3.0]
    assert "VGE_ERR_UNSUPPORTED" in ranking[3]["error"] and "components" not in ranking[3]
    assert set(ranking[0]) >= {"checkpoint", "loss", "components", "n_batches", "skipped_batches", "centroid_distance",
                               "class_distances"}
    assert built["stats"] == 1 and built["stores"] == 2
    assert built["seeds"] == [1337, 1337, 1337]      # seeded afresh for every checkpoint
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ".pt" in ln]
    assert len(lines) == 4 and "b.pt" in lines[0] and "unsupported" in lines[3]


# ----------------------------------------------------------------------------- the C ABI

def test_symbols_are_exported():
    from vge import lib as L
    so = L.load()
    for name in SYMBOLS:
        assert name in L.EXPORTS and hasattr(so, name), name
    assert so.vge_tcl_workspace_bytes(2048) >= 2 * 2048 * 8
    assert so.vge_tcl_workspace_bytes(0) == 0


def test_argument_errors_need_no_device_work():
    """Null or out-of-range arguments: VGE_ERR_ARG with the function's name in vge_last_error, before any launch
    (the pointers below are never dereferenced)."""
    from vge import lib as L
    so = L.load()
    p = C.c_void_p(0x1000)   # an aligned non-null address

    def refused(name, status):
        assert status == 1, (name, status)
        assert name.encode() in so.vge_last_error()

    refused("vge_time_gather", so.vge_time_gather(None, p, 1, 32, 2596, p, None))
    refused("vge_time_gather", so.vge_time_gather(p, None, 1, 32, 2596, C.c_void_p(0x2000), None))
    refused("vge_time_gather", so.vge_time_gather(p, p, 1, 31, 2596, C.c_void_p(0x2000), None))      # T != 32
    refused("vge_time_gather", so.vge_time_gather(p, p, 1, 32, 2598, C.c_void_p(0x2000), None))      # D % 4
    refused("vge_time_gather", so.vge_time_gather(p, p, 1, 32, 2596, p, None))                       # out aliases feats
    refused("vge_time_gather", so.vge_time_gather(p, p, -1, 32, 2596, C.c_void_p(0x2000), None))
    refused("vge_time_gather", so.vge_time_gather(C.c_void_p(0x1004), p, 1, 32, 2596, C.c_void_p(0x2000), None))
    ws = so.vge_tcl_workspace_bytes(8192)
    refused("vge_tcl_loss", so.vge_tcl_loss(None, p, 4, 32, 0.1, 5000.0, 1.0, p, ws, p, None))
    refused("vge_tcl_loss", so.vge_tcl_loss(p, p, 4, 32, 0.1, 5000.0, 1.0, p, ws, None, None))
    for B, d in ((0, 32), (8193, 32), (4, 0), (4, 48), (4, 288), (4, 16)):
        refused("vge_tcl_loss", so.vge_tcl_loss(p, p, B, d, 0.1, 5000.0, 1.0, p, ws, p, None))
    refused("vge_tcl_loss", so.vge_tcl_loss(p, p, 4, 32, 0.1, 5000.0, 1.0, p, 8, p, None))           # workspace too small
    refused("vge_tcl_loss", so.vge_tcl_loss(p, p, 4, 32, 0.0, 5000.0, 1.0, p, ws, p, None))
    refused("vge_hardneg_loss", so.vge_hardneg_loss(None, p, 4, 32, 0.07, p, None))
    refused("vge_hardneg_loss", so.vge_hardneg_loss(p, p, 4, 32, 0.07, None, None))
    refused("vge_hardneg_loss", so.vge_hardneg_loss(p, p, 0, 32, 0.07, p, None))
    refused("vge_hardneg_loss", so.vge_hardneg_loss(p, p, 4, 0, 0.07, p, None))
    refused("vge_centroid_distance", so.vge_centroid_distance(None, p, p, 4, 10, 32, p, None))
    refused("vge_centroid_distance", so.vge_centroid_distance(p, p, p, 4, 10, 32, None, None))
    refused("vge_centroid_distance", so.vge_centroid_distance(p, p, p, -1, 10, 32, p, None))
    refused("vge_centroid_distance", so.vge_centroid_distance(p, p, p, 4, 0, 32, p, None))
    refused("vge_centroid_distance", so.vge_centroid_distance(p, p, p, 4, 10, 0, p, None))
