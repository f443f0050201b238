"""The crafted cases of tests/frcnn_op_cases.py under the oracle alone (no GPU): every case has the property it is
named for, so the GPU tests that run them (tests/test_frcnn_ops.py) cannot pass vacuously.  A case whose property
fails is a broken case."""
import numpy as np
import pytest
import torch

from oracle import frcnn as O
from tests import frcnn_op_cases as FC

F32 = np.float32


# ------------------------------------------------------------------------------------------------ RPN
@pytest.mark.parametrize("k", [1, 63, 64, 65, 1000, 1024])
def test_cut_ties_kth_and_next_logits_equal(k):
    c = FC.rpn_cases()[f"cut_ties_k{k}"]
    assert c.pre_topk == k
    for f in range(c.n):
        lo = c.logits(f)[0]
        assert lo.shape[0] > k, "level 0 has more anchors than pre_topk"
        v = torch.sort(lo, descending=True).values
        assert float(v[k - 1]) == float(v[k]), (k, f)
        # the tie decides: the anchors at the tied value differ in position, and not all of them fit
        tied = torch.nonzero(lo == v[k]).view(-1)
        assert int((lo > v[k]).sum()) < k < int((lo > v[k]).sum()) + tied.numel()
    sizes = [h * w * 3 for h, w in c.shapes()]
    if k >= 1000:
        assert min(sizes) == 3 and sum(s < k for s in sizes) >= 3     # levels shorter than pre_topk, one of 1 x 1
    assert bool((c.levels[0][1, ..., 3:15] != 0).any()) and not bool((c.levels[0][0, ..., 3:15] != 0).any())


def test_all_equal_case():
    c = FC.rpn_cases()["all_equal"]
    for l in range(5):
        assert len(set(c.logits(0)[l].tolist())) == 1
        z = c.logits(1)[l]
        assert bool((z == 0).all())
    z = c.levels[0][1, ..., :3].view(np.uint32)
    assert (z == 0x80000000).any() and (z == 0).any(), "zeros of both signs"
    assert z.reshape(-1)[0] == 0x80000000 or (z.reshape(-1)[:50] == 0x80000000).any()
    b, s = FC.rpn_oracle(c, 0)
    assert b.shape[0] > 1


def test_cross_level_ties_cut_inside_the_tie():
    c = FC.rpn_cases()["cross_level_ties"]
    b, s = FC.rpn_oracle(c, 0, post_topk=1024)           # the kept boxes before the cut
    lvl = torch.round(torch.log2(torch.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])) / 32)).long()
    tie = s == 1.0
    assert len(set(lvl[tie].tolist())) >= 2, "at least two levels share a score among the kept boxes"
    p = c.post_topk
    assert b.shape[0] > p and float(s[p - 1]) == float(s[p]) == 1.0, "post_topk cuts inside the tie"
    assert int(lvl[p - 1]) <= int(lvl[p])


def test_near_iou_07_pairs():
    c = FC.rpn_cases()["near_iou_0.7"]
    thr = F32(0.7)
    d = (FC.pair_ious(c).astype(np.float64) - float(thr)) / FC.ulp(0.7)
    assert (np.abs(d) <= 4).all(), d
    below, above, exact = int((d < 0).sum()), int((d > 0).sum()), int((d == 0).sum())
    print(f"pairs within 4 ulp of 0.7: {below} below, {above} above, {exact} exact")
    assert len(d) >= 32 and below >= 8 and above >= 8 and exact >= 4
    assert len({p[1] for p in c.pairs}) == 3, "levels 0, 1 and 2: offsets 0, max + 1, 2 (max + 1)"
    per, mx = FC.rpn_valid_boxes(c, 0)
    assert float(mx) == 1000.0
    # decisive: B of a pair just above the threshold is suppressed, and kept when the threshold moves past that IoU
    n0 = FC.rpn_oracle(c, 0)[0].shape[0]
    n_hi = FC.rpn_oracle(c, 0, nms=float(thr) + 8 * FC.ulp(0.7))[0].shape[0]
    n_lo = FC.rpn_oracle(c, 0, nms=float(thr) - 8 * FC.ulp(0.7))[0].shape[0]
    assert n_hi == n0 + above and n_lo == n0 - below - exact, (n0, n_hi, n_lo)


def test_nonfinite_case():
    c = FC.rpn_cases()["nonfinite"]
    lo = c.logits(0)[0]
    bits = lo.numpy().view(np.uint32)
    assert (bits == 0x7FC00001).any() and (bits == 0xFFC00001).any() and torch.isinf(lo).sum() == 2
    v, i, box, ok = FC.rpn_select_oracle(c, 0, 0)
    nan_first = int(torch.isnan(v).sum())
    assert nan_first == 3 and bool(torch.isnan(v[:3]).all()) and i[:3].tolist() == [5, 901, 1102]
    assert float(v[3]) == float("inf") and not bool(ok[:4].any()) and int(ok.sum()) == c.pre_topk - 4
    assert lo.shape[0] > c.pre_topk, "the non-finite entries displace finite ones from the top-k"
    v, i, box, ok = FC.rpn_select_oracle(c, 1, 0)
    pos = {int(a): j for j, a in enumerate(i.tolist())}
    assert all(a in pos for a in (40, 340, 640, 940, 1000))
    assert not ok[pos[40]] and not ok[pos[340]], "NaN / +inf in dx"
    assert ok[pos[640]] and ok[pos[1000]], "+inf in dw or dh is clamped: finite"
    assert not ok[pos[940]] and bool(torch.isfinite(box[pos[940]]).all()), "-inf in dw: finite, zero width"
    assert float(box[pos[940], 2] - box[pos[940], 0]) == 0.0


def test_no_valid_box_case():
    c = FC.rpn_cases()["no_valid_box"]
    for f in range(3):
        assert FC.rpn_oracle(c, f)[0].shape[0] == 0, f
        for l in range(5):
            assert not bool(FC.rpn_select_oracle(c, f, l)[3].any())
    v, i, box, ok = FC.rpn_select_oracle(c, 2, 0)
    assert bool(torch.isfinite(v).all()) and bool((box[:, 2] - box[:, 0] == 0).all()), "clipped to zero width"
    assert c.n == 3


def test_empty_level_case():
    c = FC.rpn_cases()["empty_level"]
    valid = [bool(FC.rpn_select_oracle(c, 0, l)[3].any()) for l in range(5)]
    assert valid == [True, True, False, True, True]
    assert FC.rpn_oracle(c, 0)[0].shape[0] > 0


def test_disjoint_1024_case():
    c = FC.rpn_cases()["disjoint_1024"]
    b, s = FC.rpn_oracle(c, 0, post_topk=1024)
    assert b.shape[0] == 1024, "all kept"
    assert float(O.pair_iou(b[:, None], b[None]).fill_diagonal_(0).max()) == 0.0
    assert FC.rpn_oracle(c, 0)[0].shape[0] == 1000


# ------------------------------------------------------------------------------------------------ ROIAlign
@pytest.mark.parametrize("b", [112, 224, 448])
def test_roi_level_boundary_has_both_sides(b):
    c = FC.roi_case()
    bx = c.boxes(f"level_{b}")
    lv = O.assign_levels(bx)
    want = {112: (0, 1), 224: (1, 2), 448: (2, 3)}[b]
    assert set(lv.tolist()) == set(want), lv
    s = (bx[:, 2] - bx[:, 0]).numpy()
    assert s[0] == np.nextafter(F32(b), F32(0)) and s[1] == b and s[2] == np.nextafter(F32(b), F32(1e9))
    assert int(lv[1]) == want[1] and int(lv[3]) == want[0] and int(lv[4]) == want[1]


def test_roi_clamped_levels():
    c = FC.roi_case()
    assert O.assign_levels(c.boxes("clamp_p2")).tolist() == [0, 0]
    assert O.assign_levels(c.boxes("clamp_p5")).tolist() == [3, 3]
    bx = c.boxes("clamp_p2")
    raw = torch.floor(4 + torch.log2(torch.sqrt((bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])) / 224 + 1e-8))
    assert bool((raw < 2).all())
    bx = c.boxes("clamp_p5")
    raw = torch.floor(4 + torch.log2(torch.sqrt((bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])) / 224 + 1e-8))
    assert bool((raw > 5).all())


@pytest.mark.parametrize("ax", ["x", "y"])
def test_roi_grid_sizes(ax):
    c = FC.roi_case()
    bx = c.boxes(f"grid_{ax}")
    assert O.assign_levels(bx).tolist() == [0] * 5
    g = [FC.roi_geometry(b, 0) for b in bx.numpy()]
    assert [q[ax][0] for q in g] == [1, 2, 13, 14, 25]          # 13: the last on the tables; 14: the sample loop
    other = "y" if ax == "x" else "x"
    assert all(q[other][0] == 1 for q in g)
    both = [FC.roi_geometry(b, int(l)) for b, l in zip(c.boxes("grid_xy").numpy(), O.assign_levels(c.boxes("grid_xy")))]
    assert both[0]["x"][0] == 14 and both[0]["y"][0] == 1 and min(both[1]["x"][0], both[1]["y"][0]) >= 2


def test_roi_edge_branches_taken():
    c = FC.roi_case()
    skipped, clamped, last = FC.roi_branch_counts(c, "edges")
    print(f"edge samples: {skipped} skipped, {clamped} clamped to 0, {last} on the last cell")
    assert skipped > 0 and clamped > 0 and last > 0
    lv = O.assign_levels(c.boxes("edges")).tolist()
    assert set(lv) == {0, 1, 2, 3}
    assert c.n_prop.tolist() == [c.props.shape[1], 0, 7] and c.props.shape[1] % 2 == 1


# ------------------------------------------------------------------------------------------------ box inference
def _far_or_exact(c):
    for f in range(len(c.n_prop)):
        p = FC.det_probs(c, f)[:, :c.K]
        p = p[torch.isfinite(p)]
        d = (p - c.score_thresh).abs()
        assert bool(((d >= 1e-3) | (p == c.score_thresh)).all()), (c.name, f, float(d[d > 0].min()))


@pytest.mark.parametrize("name", FC.DET_NAMES)
def test_det_probabilities_far_from_threshold_or_exact(name):
    _far_or_exact(FC.det_cases()[name])


def test_det_full_case():
    c = FC.det_cases()["full_4096"]
    assert c.K == 127 and c.score_thresh == 0.2 and int(c.n_prop[0]) == 1024
    p = FC.det_probs(c, 0)[:, :c.K]
    passing = p > c.score_thresh
    assert bool((passing.sum(1) == 4).all()) and int(passing.sum()) == 4096
    assert bool((p[passing] == 0.25).all())
    cls = passing.nonzero()[:, 1]
    assert int((cls >= 64).sum()) > 0 and int((cls == 126).sum()) > 0
    r = FC.det_candidates(c, 0)
    assert r["b"].shape[0] == 4096 > c.det_per_img, "every candidate survives"
    assert float(r["s"][c.det_per_img - 1]) == float(r["s"][c.det_per_img])


@pytest.mark.parametrize("K", [1, 80, 127])
def test_det_mixed_case(K):
    c = FC.det_cases()[f"mixed_K{K}"]
    assert [FC.det_oracle(c, f)["n_person"] for f in range(3)] == [0, 1, 2]
    for f in range(3):
        r, p = FC.det_oracle(c, f), FC.det_probs(c, f)
        n = int(c.n_prop[f])
        assert int(torch.isnan(p).any(dim=1).sum()) == 1, "one row with a NaN logit"
        de = torch.from_numpy(c.head[f, :n, K + 1:5 * K + 1].copy())
        bx = O.apply_deltas(de, torch.from_numpy(c.props[f, :n, :4].copy()), (10.0, 10.0, 5.0, 5.0))
        assert int((~torch.isfinite(bx).all(dim=1)).sum()) == 1, "+inf in dx: not finite; +inf / -inf in dw: finite"
        assert int(torch.isinf(de).any(dim=1).sum()) == 3
        if K >= 4:
            assert int(((p[:, :K] == 0.25).sum(1) == 4).sum()) == 1, "four classes at 0.25 exactly: none passes"
        w = r["b"][:, 2] - r["b"][:, 0]
        assert int((w == 0).sum()) == 1 and int(r["k"][w == 0]) == K - 1, "a zero-area candidate survives inference"
        thin = 1 if f == 1 else 0
        assert r["b"].shape[0] == r["fb"].shape[0] + 1 + thin
        assert r["fb"].shape[0] == f + (1 if K > 1 else 0) + 1 + (1 if f == 2 else 0)
        if K > 64:
            assert int((r["k"] >= 64).sum()) > 0
    r = FC.det_oracle(c, 2)
    assert int(((r["fk"] == 0) & (r["fs"] == 0.5)).sum()) == 1, "a person at the gate threshold exactly"
    bits = c.head[:, :, 0].view(np.uint32)
    assert (bits == 0x7FC00001).any() and (bits == 0xFFC00001).any()


def test_det_three_persons_case():
    c = FC.det_cases()["three_persons"]
    big = FC.det_candidates(c, 0)
    assert big["b"].shape[0] == 8 > c.det_per_img == 4 and int((big["fk"] == 0).sum()) == 3
    assert FC.det_oracle(c, 0)["n_person"] == 2
    r = FC.det_oracle(c, 1)
    assert r["n_person"] == 3 and r["b"].shape[0] == 4
    assert c.n_prop.tolist() == [8, 4, 0]


def test_det_near_iou_05_pairs():
    c = FC.det_cases()["near_iou_0.5"]
    d = (FC.det_pair_ious(c).astype(np.float64) - 0.5) / FC.ulp(0.5)
    assert (np.abs(d) <= 4).all(), d
    below, above, exact = int((d < 0).sum()), int((d > 0).sum()), int((d == 0).sum())
    print(f"pairs within 4 ulp of 0.5: {below} below, {above} above, {exact} exact")
    assert len(d) >= 32 and below >= 8 and above >= 8 and exact >= 4
    assert len({p[3] for p in c.pairs}) >= 8 and max(p[3] for p in c.pairs) == 126
    n0 = FC.det_oracle(c, 0)["b"].shape[0]
    n_hi = FC.det_oracle(c, 0, nms_thresh=0.5 + 8 * FC.ulp(0.5))["b"].shape[0]
    n_lo = FC.det_oracle(c, 0, nms_thresh=0.5 - 8 * FC.ulp(0.5))["b"].shape[0]
    assert n_hi == n0 + above and n_lo == n0 - below - exact, (n0, n_hi, n_lo)
