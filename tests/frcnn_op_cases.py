"""Crafted inputs for the gate detector's op entry points (include/vge_frcnn.h vge_op_*), built from seeds in memory.
Plain functions returning named cases; every case is a valid input of the detector's own launchers.

  rpn_cases()   RpnCase: five level tensors f32 [n, h, w, 16] (logits 3 | deltas 12 | one unread column of NaN), the
                top-k sizes, NMS threshold and image size; `pairs` lists the near-threshold pairs a case was built for
  roi_case()    RoiCase: four bf16 level maps and one list of boxes, `groups` naming the slice each property lives in
  det_cases()   DetCase: head rows (logits K + 1 | deltas 4 K), proposals and the sizes of vge_op_det_post

tests/test_frcnn_op_cases.py runs the oracle alone on every case and asserts the property the case is named for;
tests/test_frcnn_ops.py runs the same cases on the GPU.  The oracle helpers both use are here too (rpn_oracle,
rpn_select_oracle, det_oracle), so the two files look at one reference.

Boxes whose IoU must be identical on both sides are decoded with dw = dh = 0 (exp(0) = 1 exactly; the centre shift
dx * w + cx is a float32 multiply and an add, separately rounded on both sides), so a near-threshold decision tests
the IoU arithmetic and not expf.
"""
from dataclasses import dataclass, field
from functools import lru_cache
from types import SimpleNamespace
from typing import Dict, List, Tuple

import numpy as np
import torch

from oracle import frcnn as O

INF = float("inf")
NAN = float("nan")
F32 = np.float32
ANCHOR_SIZES = (32, 64, 128, 256, 512)
RATIOS = (0.5, 1.0, 2.0)
SMALL = ((20, 20), (10, 10), (5, 5), (3, 3), (1, 1))   # 1,200 / 300 / 75 / 27 / 3 anchors


def nan_bits(bits: int) -> np.float32:
    return np.array([bits], np.uint32).view(np.float32)[0]


NAN_POS, NAN_NEG = nan_bits(0x7FC00001), nan_bits(0xFFC00001)   # sign bit clear / set


def oracle(pre_topk=1000, post_topk=1000, rpn_nms=0.7, score_thresh=0.25, nms_thresh=0.5, det_per_img=100):
    cfg = SimpleNamespace(rpn_pre_topk=pre_topk, rpn_post_topk=post_topk, rpn_nms=rpn_nms, anchor_sizes=ANCHOR_SIZES,
                          aspect_ratios=RATIOS, score_thresh=score_thresh, nms_thresh=nms_thresh,
                          det_per_img=det_per_img, pool=7)
    return O.OracleFrcnn({}, cfg, bf16=True)


def ulp(thr: float) -> float:
    return float(np.spacing(F32(thr)))


# ------------------------------------------------------------------------------------------------ RPN
@dataclass
class RpnCase:
    name: str
    levels: List[np.ndarray]                 # five f32 [n, h, w, 16]
    pre_topk: int
    post_topk: int
    image_size: Tuple[int, int]
    nms: float = 0.7
    zero_deltas: bool = False                # every delta is 0: boxes are clipped anchors, compared exactly
    pairs: list = field(default_factory=list)  # (frame, level, flat anchor index A, B) of near-threshold pairs
    note: str = ""

    @property
    def n(self):
        return self.levels[0].shape[0]

    def logits(self, f):
        return [torch.from_numpy(t[f, ..., :3].reshape(-1).copy()) for t in self.levels]

    def deltas(self, f):
        return [torch.from_numpy(t[f, ..., 3:15].reshape(-1, 4).copy()) for t in self.levels]

    def shapes(self):
        return [tuple(t.shape[1:3]) for t in self.levels]


def blank(n, sizes, fill=-INF):
    out = []
    for h, w in sizes:
        t = np.zeros((n, h, w, 16), np.float32)
        t[..., :3] = fill
        t[..., 15] = NAN
        out.append(t)
    return out


def put(t, f, idx, logit=None, d=None):
    """anchor `idx` (flat (y, x, a)) of frame f of one level tensor"""
    loc, a = divmod(int(idx), 3)
    row = t[f].reshape(-1, 16)[loc]
    if logit is not None:
        row[a] = logit
    if d is not None:
        row[3 + 4 * a:7 + 4 * a] = d


def rpn_oracle(case: RpnCase, f: int, post_topk=None, nms=None):
    """oracle proposals() of frame f -> (boxes [P, 4], logits [P])"""
    o = oracle(case.pre_topk, case.post_topk if post_topk is None else post_topk, case.nms if nms is None else nms)
    return o.proposals(case.logits(f), case.deltas(f), case.image_size, case.shapes())


def rpn_select_oracle(case: RpnCase, f: int, l: int):
    """The level's top-k as find_top_rpn_proposals forms it -> (logits [k], anchor index [k], clipped boxes [k, 4],
    valid [k]): what rpn_select_kernel leaves in `sel`."""
    lo, de = case.logits(f)[l], case.deltas(f)[l]
    h, w = case.shapes()[l]
    k = min(case.pre_topk, lo.shape[0])
    v, i = O.topk_stable(lo, k)
    anc = O.grid_anchors(h, w, 4 * 2 ** l, ANCHOR_SIZES[l], RATIOS)[i]
    b = O.apply_deltas(de[i], anc, (1.0, 1.0, 1.0, 1.0))
    fin = torch.isfinite(b).all(dim=1) & torch.isfinite(v)
    c = O.clip_boxes(b, case.image_size[0], case.image_size[1])
    return v, i, c, fin & O.nonempty(c)


def rpn_valid_boxes(case: RpnCase, f: int):
    """-> per level (boxes, logits, anchor index) of the valid top-k entries, and the largest coordinate over all"""
    per = []
    for l in range(5):
        v, i, c, ok = rpn_select_oracle(case, f, l)
        per.append((c[ok], v[ok], i[ok]))
    allb = torch.cat([p[0] for p in per])
    return per, (allb.max() if allb.numel() else torch.tensor(0.0))


def pair_ious(case: RpnCase):
    """float32 IoU of every listed pair, on the level-offset boxes, as oracle.nms computes it"""
    out = []
    for f in sorted({p[0] for p in case.pairs}):
        per, mx = rpn_valid_boxes(case, f)
        for (_, l, ia, ib) in [p for p in case.pairs if p[0] == f]:
            b, _, idx = per[l]
            pos = {int(v): j for j, v in enumerate(idx.tolist())}
            off = torch.tensor(float(l)) * (mx + torch.tensor(1.0))
            out.append(float(O.pair_iou(b[pos[ia]] + off, b[pos[ib]] + off)))
    return np.array(out, np.float32)


def _tie_levels(rng, n, k, sizes=SMALL):
    """Level 0: max(k - 3, 0) logits above t, 7 equal to t at scattered anchors, the rest below: the k-th and the
    (k + 1)-th largest are both t.  The other levels: logits from a set of 9 values (ties everywhere)."""
    lv = blank(n, sizes, 0.0)
    for f in range(n):
        for l, t in enumerate(lv):
            N = t.shape[1] * t.shape[2] * 3
            if l == 0:
                tval = F32(0.25)
                perm = rng.permutation(N)
                g = max(k - 3, 0)
                lg = np.empty(N, np.float32)
                lg[perm[:g]] = tval + F32(0.01) + rng.random(g).astype(np.float32)
                lg[perm[g:g + 7]] = tval
                lg[perm[g + 7:]] = tval - F32(0.01) - rng.random(N - g - 7).astype(np.float32)
            else:
                lg = (rng.integers(-4, 5, N) * 0.5).astype(np.float32)
            t[f, ..., :3] = lg.reshape(t.shape[1], t.shape[2], 3)
            if f == 1:   # the second frame decodes real deltas
                d = rng.uniform(-0.3, 0.3, (t.shape[1], t.shape[2], 12)).astype(np.float32)
                t[f, ..., 3:15] = d
    return lv


def _search_b(anc_a, anc_b, off, thr, rng, size, tries=200000):
    """Deltas (dx, dy, 0, 0) for anchor B such that IoU(A, B) on the offset boxes lies within 4 ulp of thr ->
    {-1: [...], 0: [...], +1: [...]} lists of (dx, dy) by side."""
    t = float(F32(thr))
    a_box = O.apply_deltas(torch.zeros(1, 4), anc_a[None], (1.0,) * 4)[0]
    inter = 2.0 * size * size * t / (1.0 + t)
    b0 = rng.uniform(0.0, 0.08 * size, tries)
    a0 = size - inter / (size - b0)
    shift0 = float(anc_b[0] - anc_a[0])
    d = 3e-4
    dx = ((a0 - shift0) / size + rng.uniform(-d, d, tries)).astype(np.float32)
    dy = (b0 / size + rng.uniform(-d, d, tries)).astype(np.float32)
    de = torch.from_numpy(np.stack([dx, dy, np.zeros_like(dx), np.zeros_like(dx)], 1))
    bb = O.apply_deltas(de, anc_b[None].expand(tries, 4), (1.0,) * 4)
    o = torch.tensor(off, dtype=torch.float32)
    iou = O.pair_iou((a_box + o)[None], bb + o).numpy()
    u = ulp(thr)
    diff = (iou.astype(np.float64) - t) / u
    out = {}
    for side, m in ((-1, (diff < 0) & (diff >= -4)), (0, diff == 0), (1, (diff > 0) & (diff <= 4))):
        j = np.nonzero(m)[0]
        out[side] = [(dx[i], dy[i]) for i in j[:4]]
    return out


def _near_iou_case(seed=707):
    """Isolated pairs (A, B) of ratio-1 anchors on levels 0..2: A with zero deltas, B the next cell's anchor shifted
    by (dx, dy) found by a seeded random search so that the float32 IoU of the offset boxes lies within 4 ulp of 0.7,
    on a chosen side; pairs at the right image edge, clipped to widths 10 and 7 (20 and 14, ...): IoU = 0.7 exactly.
    A level-3 anchor clipped at the image edge pins the largest coordinate (the level offsets) to the image size."""
    rng = np.random.default_rng(seed)
    img = (1000, 1000)
    sizes = ((64, 250), (64, 64), (64, 64), (32, 32), (1, 1))
    lv = blank(1, sizes)
    put(lv[3], 0, (31 * 32 + 31) * 3 + 1, logit=-5.0)            # x2 = 1120 -> 1000: the largest coordinate
    mx = 1000.0
    pairs, score = [], 5.0
    want = [-1, 1]
    for l in range(3):
        h, w = sizes[l]
        stride, size = 4 << l, 32 << l
        anc = O.grid_anchors(h, w, stride, ANCHOR_SIZES[l], RATIOS)
        off = l * (mx + 1.0)
        k = 0
        for cy in range(6, h - 6, 12):
            for cx in range(6, min(w, 62) - 8, 12):
                ia, ib = (cy * w + cx) * 3 + 1, (cy * w + cx + 1) * 3 + 1
                found = _search_b(anc[ia], anc[ib], off, 0.7, rng, float(size))
                side = want[k % 2]
                if not found[side]:
                    continue
                dx, dy = found[side][0]
                put(lv[l], 0, ia, logit=score)
                put(lv[l], 0, ib, logit=score - 0.005, d=(dx, dy, 0.0, 0.0))
                pairs.append((0, l, ia, ib))
                score -= 0.01
                k += 1
    # exact pairs on level 0 at the right edge: A spans [1000 - 10 m, 1000], B [1000 - 7 m, 1000], the same rows
    anc = O.grid_anchors(*sizes[0], 4, 32, RATIOS)
    w0 = sizes[0][1]
    for j, m in enumerate((1.0, 2.0, 0.5, 1.5, 0.25, 2.5)):
        cy, cx = 6 + 9 * j, 247                                   # anchor x1 = 4 * 247 - 16 = 972
        ia, ib = (cy * w0 + cx) * 3 + 1, (cy * w0 + cx + 1) * 3 + 1   # B: x1 = 976
        put(lv[0], 0, ia, logit=score, d=((1000 - 10 * m - 972) / 32.0, 0.0, 0.0, 0.0))
        put(lv[0], 0, ib, logit=score - 0.005, d=((1000 - 7 * m - 976) / 32.0, 0.0, 0.0, 0.0))
        pairs.append((0, 0, ia, ib))
        score -= 0.01
    return RpnCase("near_iou_0.7", lv, 1000, 1000, img, pairs=pairs,
                   note="pairs within 4 ulp of 0.7 on levels 0..2 (level offsets), exact 0.7 at the image edge")


def _cross_level_case():
    """Spaced ratio-1 anchors (zero deltas, no overlap inside a level) with the score 1.0 on levels 0, 1 and 2, a few
    higher and lower scores around them; post_topk cuts inside the run of 1.0."""
    sizes = ((100, 100), (50, 50), (25, 25), (3, 3), (1, 1))
    lv = blank(2, sizes)
    per_level = []
    for l in range(3):
        h, w = sizes[l]
        cells = [(y, x) for y in range(5, h - 4, 10) for x in range(5, w - 4, 10)]
        per_level.append(len(cells))
        for j, (y, x) in enumerate(cells):
            s = 1.0 if j % 3 else (2.0 - 0.01 * j - 0.001 * l if j % 2 else 0.5 - 0.01 * j - 0.001 * l)
            for f in range(2):
                put(lv[l], f, (y * w + x) * 3 + 1, logit=s)
    return RpnCase("cross_level_ties", lv, 1000, 40, (400, 400), zero_deltas=True,
                   note="equal scores on three levels; post_topk 40 cuts inside the tie")


def _nonfinite_case(seed=99):
    """pre_topk 64 on a level of 1,200 anchors: the non-finite entries take top-k slots and are then dropped.  Frame 0:
    logits +inf, -inf, NaN with the sign bit clear and set.  Frame 1: finite top logits whose deltas hold NaN / +inf in
    dx, +inf in dw (clamped: the box stays finite) and -inf in dw (zero width: empty)."""
    rng = np.random.default_rng(seed)
    lv = blank(2, SMALL, 0.0)
    for f in range(2):
        for t in lv:
            N = t.shape[1] * t.shape[2] * 3
            t[f, ..., :3] = rng.permutation(N).astype(np.float32).reshape(t.shape[1], t.shape[2], 3) / F32(N) - F32(2.0)
            t[f, ..., 3:15] = rng.uniform(-0.2, 0.2, (t.shape[1], t.shape[2], 12)).astype(np.float32)
    L0 = lv[0]
    put(L0, 0, 100, logit=INF)
    put(L0, 0, 700, logit=-INF)
    put(L0, 0, 901, logit=NAN_POS)
    put(L0, 0, 5, logit=NAN_NEG)
    put(L0, 0, 1102, logit=NAN_NEG)
    put(lv[1], 0, 17, logit=NAN_NEG)     # a level with fewer anchors than pre_topk
    put(lv[4], 0, 1, logit=NAN_POS)      # the 1 x 1 level
    put(L0, 1, 40, logit=3.0, d=(NAN, 0.0, 0.0, 0.0))
    put(L0, 1, 340, logit=2.9, d=(INF, 0.0, 0.0, 0.0))
    put(L0, 1, 640, logit=2.8, d=(0.0, 0.0, INF, 0.0))
    put(L0, 1, 940, logit=2.7, d=(0.0, 0.0, -INF, 0.0))
    put(L0, 1, 1000, logit=2.6, d=(0.0, 0.1, 0.0, INF))
    return RpnCase("nonfinite", lv, 64, 1000, (80, 80), note="inf / NaN logits and deltas")


def _no_valid_case():
    """Frame 0: every logit -inf.  Frame 1: every dw -inf (zero width).  Frame 2: every box decoded to the right of the
    image and clipped to zero width."""
    rng = np.random.default_rng(5)
    lv = blank(3, SMALL, 0.0)
    for t in lv:
        t[..., :3] = rng.standard_normal(t[..., :3].shape).astype(np.float32)
        t[0, ..., :3] = -INF
        t[1, ..., 5:15:4] = -INF
        t[2, ..., 3:15:4] = 100.0
    return RpnCase("no_valid_box", lv, 1000, 1000, (80, 80), note="n_prop = 0")


def _empty_level_case():
    """Level 2 alone has no valid box (every logit -inf); the other levels hold random logits and deltas."""
    rng = np.random.default_rng(6)
    lv = blank(1, SMALL, 0.0)
    for t in lv:
        t[..., :3] = rng.standard_normal(t[..., :3].shape).astype(np.float32)
        t[..., 3:15] = rng.uniform(-0.2, 0.2, t[..., 3:15].shape).astype(np.float32)
    lv[2][0, ..., :3] = -INF
    return RpnCase("empty_level", lv, 1000, 1000, (80, 80), note="one level without a valid box")


def _disjoint_case(seed=31):
    """1,024 ratio-1 level-0 anchors 36 pixels apart (32-pixel boxes: disjoint), distinct logits above the rest."""
    rng = np.random.default_rng(seed)
    sizes = ((288, 288), (2, 2), (1, 1), (1, 1), (1, 1))
    lv = blank(1, sizes)
    t = lv[0]
    t[0, ..., :3] = -3.0 - rng.random((288, 288, 3)).astype(np.float32)
    sc = rng.permutation(1024).astype(np.float32) / F32(64.0)
    for j in range(1024):
        y, x = 9 * (j // 32) + 4, 9 * (j % 32) + 4
        put(t, 0, (y * 288 + x) * 3 + 1, logit=sc[j])
    return RpnCase("disjoint_1024", lv, 1024, 1000, (1200, 1200), zero_deltas=True,
                   note="1,024 disjoint boxes kept, post_topk 1000")


def _all_equal_case():
    """Frame 0: every logit 0.5.  Frame 1: every logit a zero of random sign (equal values: the index decides)."""
    rng = np.random.default_rng(8)
    lv = blank(2, SMALL, 0.5)
    for t in lv:
        z = np.zeros(t[1, ..., :3].shape, np.float32)
        z[rng.random(z.shape) < 0.5] = -0.0
        t[1, ..., :3] = z
    return RpnCase("all_equal", lv, 1000, 1000, (80, 80), zero_deltas=True, note="all logits equal; signed zeros")


RPN_NAMES = [f"cut_ties_k{k}" for k in (1, 63, 64, 65, 1000, 1024)] + [
    "all_equal", "cross_level_ties", "near_iou_0.7", "nonfinite", "no_valid_box", "empty_level", "disjoint_1024"]
DET_NAMES = ["full_4096", "mixed_K1", "mixed_K80", "mixed_K127", "three_persons", "near_iou_0.5"]


@lru_cache(maxsize=None)
def rpn_cases() -> Dict[str, RpnCase]:
    cases = []
    for k in (1, 63, 64, 65, 1000, 1024):
        rng = np.random.default_rng(1000 + k)
        cases.append(RpnCase(f"cut_ties_k{k}", _tie_levels(rng, 2, k), k, 1000, (80, 80),
                             note="the k-th and (k + 1)-th logits of level 0 are equal"))
    cases += [_all_equal_case(), _cross_level_case(), _near_iou_case(), _nonfinite_case(), _no_valid_case(), _empty_level_case(),
              _disjoint_case()]
    assert [c.name for c in cases] == RPN_NAMES
    return {c.name: c for c in cases}


# ------------------------------------------------------------------------------------------------ ROIAlign
@dataclass
class RoiCase:
    levels: List[torch.Tensor]               # four bf16 [n, h, w, 256]
    props: np.ndarray                        # f32 [n, P, 5]
    n_prop: np.ndarray                       # int32 [n]
    groups: Dict[str, slice]                 # name -> rows of frame 0's boxes

    def boxes(self, name=None):
        b = torch.from_numpy(self.props[0, :self.n_prop[0], :4].copy())
        return b if name is None else b[self.groups[name]]


ROI_MAPS = ((184, 184), (64, 64), (32, 32), (34, 34))     # P2..P5 cells (strides 4, 8, 16, 32)


def _sq(x, y, s):
    return [x, y, F32(x) + F32(s), F32(y) + F32(s)]


def roi_boxes() -> Tuple[np.ndarray, Dict[str, slice]]:
    g, rows = {}, []

    def add(name, bs):
        g[name] = slice(len(rows), len(rows) + len(bs))
        rows.extend(bs)

    for b in (112.0, 224.0, 448.0):          # x1 = y1 = 8: x2 = 8 + s stays in s's binade, so x2 - x1 = s exactly
        lo, hi = np.nextafter(F32(b), F32(0)), np.nextafter(F32(b), F32(1e9))
        add(f"level_{int(b)}", [_sq(8.0, 8.0, s) for s in (lo, F32(b), hi, F32(b - 1), F32(b + 1), F32(b * 0.75))])
    add("clamp_p2", [_sq(20.0, 30.0, 3.0), [5.0, 5.0, 5.5, 40.0]])
    add("clamp_p5", [_sq(10.0, 10.0, 1000.0), _sq(0.0, 0.0, 2000.0)])
    # samples per bin along one axis on P2 (20 pixels = 5 cells across: 1 sample): 1, 2, 13, 14, 25
    lens = (20.0, 40.0, 364.0, 365.0, 700.0)
    add("grid_x", [[16.0, 100.0, 16.0 + v, 100.0 + (12.0 if v > 600 else 20.0)] for v in lens])
    add("grid_y", [[100.0, 16.0, 100.0 + (12.0 if v > 600 else 20.0), 16.0 + v] for v in lens])
    add("grid_xy", [[8.0, 8.0, 8.0 + 365.0, 8.0 + 28.0], [300.0, 300.0, 300.0 + 60.0, 300.0 + 100.0]])
    # off every side of its map (P2 covers 736 pixels, P3 512, P4 512, P5 1088), and along the last cells
    add("edges", [[-40.0, 10.0, 30.0, 60.0], [10.0, -40.0, 60.0, 30.0], [700.0, 10.0, 790.0, 60.0],
                  [10.0, 700.0, 60.0, 790.0], [-30.0, -30.0, 20.0, 20.0], [720.0, 720.0, 780.0, 780.0],
                  [-100.0, 300.0, 100.0, 480.0], [400.0, 400.0, 640.0, 640.0], [-200.0, -200.0, 300.0, 300.0],
                  [300.0, 300.0, 800.0, 800.0], [0.0, 0.0, 2.0, 2.0], [0.0, 0.0, 736.0, 12.0],
                  [730.0, 0.0, 736.0, 736.0], [500.0, 100.0, 1200.0, 1100.0], [200.0, 650.0, 260.0, 736.0]])
    return np.asarray(rows, np.float32), g


@lru_cache(maxsize=None)
def roi_case(seed=4242) -> RoiCase:
    """Frame 0: every box, n_prop = P (an odd count).  Frame 1: n_prop = 0.  Frame 2: the first 7 boxes only.  Slots
    from n_prop on hold NaN boxes that must not be read."""
    g = torch.Generator().manual_seed(seed)
    boxes, groups = roi_boxes()
    P = boxes.shape[0]
    n = 3
    levels = [torch.randn((n, h, w, 256), generator=g).to(torch.bfloat16) for h, w in ROI_MAPS]
    props = np.full((n, P, 5), NAN, np.float32)
    props[0, :, :4] = boxes
    props[0, :, 4] = 0.0
    props[2, :7] = props[0, :7]
    return RoiCase(levels, props, np.array([P, 0, 7], np.int32), groups)


def roi_geometry(box, l):
    """ROIAlign's per-axis geometry of one box on level l (0..3), in float32 as the oracle computes it -> dict with
    grid (gh, gw) and, per axis, the sample coordinates [7, g]."""
    sc = F32(1.0 / (4 * 2 ** l))
    x1, y1, x2, y2 = (F32(v) for v in box)
    out = {}
    for ax, (a, b) in (("x", (x1, x2)), ("y", (y1, y2))):
        s, e = F32(a * sc) - F32(0.5), F32(b * sc) - F32(0.5)
        r = F32(e - s)
        bs = F32(r / F32(7))
        gcount = int(np.ceil(r / F32(7)))
        p = np.arange(7, dtype=np.float32)[:, None]
        i = np.arange(max(gcount, 0), dtype=np.float32)[None, :]
        out[ax] = (gcount, (F32(s) + p * bs) + ((i + F32(0.5)) * bs) / F32(max(gcount, 1)))
    return out


def roi_branch_counts(case: RoiCase, name: str):
    """-> samples (over both axes of the group's boxes) skipped (v < -1 or v > L), clamped to 0 (-1 <= v <= 0), and on
    the last cell (lo >= L - 1)"""
    bx = case.boxes(name)
    lv = O.assign_levels(bx)
    skipped = clamped = last = 0
    for b, l in zip(bx.numpy(), lv.tolist()):
        geo = roi_geometry(b, l)
        for ax, L in (("x", ROI_MAPS[l][1]), ("y", ROI_MAPS[l][0])):
            v = geo[ax][1]
            out = (v < -1.0) | (v > L)
            skipped += int(out.sum())
            clamped += int(((v <= 0) & ~out).sum())
            last += int(((np.floor(np.maximum(v, 0)) >= L - 1) & ~out).sum())
    return skipped, clamped, last


# ------------------------------------------------------------------------------------------------ box inference
@dataclass
class DetCase:
    name: str
    head: np.ndarray                         # f32 [n, P, ld]
    props: np.ndarray                        # f32 [n, P, 5]
    n_prop: np.ndarray                       # int32 [n]
    K: int
    det_per_img: int
    image_size: Tuple[int, int]
    frame_hw: Tuple[int, int]
    score_thresh: float = 0.25
    nms_thresh: float = 0.5
    gate_thresh: float = 0.5
    pairs: list = field(default_factory=list)   # (frame, row A, row B, class)
    note: str = ""


def det_blank(n, P, K, image_size, frame_hw, **kw):
    ld = -(-(5 * K + 1) // 8) * 8
    head = np.zeros((n, P, ld), np.float32)
    head[..., :K + 1] = -INF
    head[..., K] = 0.0                       # background
    head[..., 5 * K + 1:] = NAN              # the row's padding is not read
    props = np.full((n, P, 5), NAN, np.float32)
    return DetCase(kw.pop("name"), head, props, np.zeros(n, np.int32), K, kw.pop("det_per_img", 100), image_size,
                   frame_hw, **kw)


def det_row(c: DetCase, f, box, classes, logits=None, bg=0.0):
    """append a proposal to frame f: `classes` get `logits` (default 0: equal to the background's `bg` = 0), the rest
    -inf"""
    r = int(c.n_prop[f])
    c.props[f, r, :4] = box
    c.props[f, r, 4] = 0.0
    c.head[f, r, c.K] = bg
    for j, k in enumerate(classes):
        c.head[f, r, k] = 0.0 if logits is None else logits[j]
    c.n_prop[f] = r + 1
    return r


def det_probs(c: DetCase, f):
    cl = torch.from_numpy(c.head[f, :c.n_prop[f], :c.K + 1].copy())
    e = torch.exp(cl - cl.max(dim=1, keepdim=True).values)
    return e / e.sum(dim=1, keepdim=True)


def det_oracle(c: DetCase, f: int, nms_thresh=None):
    """oracle inference() + postprocess() + the gate count of frame f"""
    o = oracle(score_thresh=c.score_thresh, nms_thresh=c.nms_thresh if nms_thresh is None else nms_thresh,
               det_per_img=c.det_per_img)
    n = int(c.n_prop[f])
    cl = torch.from_numpy(c.head[f, :n, :c.K + 1].copy())
    de = torch.from_numpy(c.head[f, :n, c.K + 1:5 * c.K + 1].copy())
    pb = torch.from_numpy(c.props[f, :n, :4].copy())
    b, s, k = o.inference(cl, de, pb, c.image_size)
    fb, fs, fk = O.OracleFrcnn.postprocess(b, s, k, c.image_size, c.frame_hw[0], c.frame_hw[1])
    return dict(b=b, s=s, k=k, fb=fb, fs=fs, fk=fk,
                n_person=int(((fk == 0) & (fs > c.gate_thresh)).sum()))


def det_candidates(c: DetCase, f: int):
    """every candidate of frame f before NMS -> (boxes, scores, classes, the oracle's survivors with no cut)"""
    big = DetCase(**{**c.__dict__, "det_per_img": 1 << 20})
    r = det_oracle(big, f)
    return r


def _grid_boxes(nx, ny, size=20.0, step=30.0):
    return [[step * x + 2.0, step * y + 2.0, step * x + 2.0 + size, step * y + 2.0 + size]
            for y in range(ny) for x in range(nx)]


def _det_full_case():
    """1,024 disjoint proposals x 4 classes at 0.25 exactly (four equal logits, the rest -inf; score_thresh 0.2): 4,096
    candidates, all kept, all scores equal: det_per_img = 100 cuts by candidate order.  K = 127; every row has a class
    >= 64, every ninth class 126."""
    K = 127
    c = det_blank(1, 1024, K, (1000, 1000), (500, 750), name="full_4096", score_thresh=0.2)
    for j, b in enumerate(_grid_boxes(32, 32)):
        base = j % 60
        det_row(c, 0, b, [base, base + 21, 126 if j % 9 == 0 else base + 42, base + 64], bg=-INF)
    return c


def _det_mixed_case(K):
    """Three frames with 0 / 1 / 2 persons above the gate.  Every frame also holds: an ordinary row of another class
    (K > 1), a zero-area candidate of class K - 1 (dw = -inf), four classes at 0.25 exactly (K >= 4: none passes
    0.25), a row with a NaN logit and a row with +inf in class K - 1's dx (both dropped whole), and a class-0 row at
    0.27 with +inf in dw (clamped: it stays, below the gate).  Frame 2 adds a person at 0.5 exactly (not above the
    gate), frame 1 a box one float wide that is empty only after scaling to the frame."""
    img, frame = (107, 200), (60, 110)
    c = det_blank(3, 16, K, img, frame, name=f"mixed_K{K}")
    boxes = _grid_boxes(6, 4, 20.0, 25.0)
    last = K - 1
    for f in range(3):
        bi = iter(boxes)
        for p in range(f):
            det_row(c, f, next(bi), [0], logits=[2.0 + 0.25 * p])
        if K > 1:
            det_row(c, f, next(bi), [min(K - 2, 70)], logits=[1.5])
        r = det_row(c, f, next(bi), [last], logits=[1.0])
        c.head[f, r, K + 1 + 4 * last + 2] = -INF
        if K >= 4:
            det_row(c, f, next(bi), [0, 1, 2, 3], bg=-INF)
        det_row(c, f, next(bi), [0], logits=[NAN_POS if f != 1 else NAN_NEG])
        r = det_row(c, f, next(bi), [0], logits=[3.0])
        c.head[f, r, K + 1 + 4 * last] = INF
        r = det_row(c, f, next(bi), [0], logits=[-1.0])
        c.head[f, r, K + 1 + 2] = INF
    det_row(c, 2, [150.0, 60.0, 170.0, 80.0], [0])
    # a box one float wide at the right image edge: centre 200 exactly (dx = 0.5 of a 2-pixel proposal), half width
    # 1e-5 (dw = log(1e-5)), so x1 rounds to the float below 200 (spacing 1.5e-5) and x2 is clipped to 200, whatever
    # the last bit of exp.  Scaled by float32(out_w / 200), rounded up, x1 lands within half a float of out_w at some
    # frame widths and is clipped to it: the first such width.
    r = det_row(c, 1, [198.0, 90.0, 200.0, 100.0], [last], logits=[0.5])
    c.head[1, r, K + 1 + 4 * last] = 5.0
    c.head[1, r, K + 1 + 4 * last + 2] = F32(5.0 * np.log(1e-5))
    for out_w in range(101, 200):
        trial = DetCase(**{**c.__dict__, "frame_hw": (60, out_w)})
        q = det_oracle(trial, 1)
        w = q["b"][:, 2] - q["b"][:, 0]
        if int((w > 0).sum()) == q["fb"].shape[0] + 1:
            return trial
    raise AssertionError("no frame width at which the thin box empties")


def _det_three_persons():
    """Frame 0: eight survivors, det_per_img = 4 keeps two of its three persons.  Frame 1: three persons above the
    gate within the cut (the first two are reported).  Frame 2: n_prop = 0."""
    c = det_blank(3, 16, 80, (200, 300), (400, 600), name="three_persons", det_per_img=4)
    for j, b in enumerate(_grid_boxes(4, 2, 30.0, 40.0)):
        det_row(c, 0, b, [0 if j in (1, 2, 5) else 17 + j], logits=[2.0 - 0.125 * j])
        if j < 4:
            det_row(c, 1, b, [0 if j != 1 else 33], logits=[1.0 + 0.125 * j])
    return c


def _det_near_iou(seed=505):
    """Pairs of proposals of one class (zero deltas: the candidates are the proposals' own decode) whose float32 IoU on
    the class-offset boxes lies within 4 ulp of 0.5, found by a seeded random search, and pairs at 0.5 exactly
    (widths 10 and 5 on a 1/8 grid).  A proposal touching the image edge pins the largest coordinate."""
    rng = np.random.default_rng(seed)
    K, img = 127, (1000, 1000)
    c = det_blank(1, 256, K, img, (1000, 1000), name="near_iou_0.5", det_per_img=256)
    det_row(c, 0, [900.0, 900.0, 1000.0, 1000.0], [5], logits=[0.5])
    o = oracle()
    t, u = float(F32(0.5)), ulp(0.5)
    k = 0
    slots = [(40.0 + 70.0 * x, 40.0 + 70.0 * y) for y in range(11) for x in range(11)]
    classes = [0, 1, 2, 3, 7, 20, 63, 64, 65, 100, 126]
    for (x0, y0) in slots:
        cls = classes[k % len(classes)]
        off = torch.tensor(float(cls)) * torch.tensor(1001.0)
        w, h = float(rng.uniform(20, 40)), float(rng.uniform(20, 40))
        A = np.array([x0, y0, x0 + w, y0 + h], np.float32)
        tries = 200000
        b = rng.uniform(0, 0.05 * h, tries)
        inter = 2.0 * w * h * t / (1.0 + t)
        a = w - inter / (h - b)
        Bx = np.stack([x0 + a + rng.uniform(-0.02, 0.02, tries), y0 + b + rng.uniform(-0.02, 0.02, tries)], 1)
        Bb = np.concatenate([Bx, Bx + np.array([w, h])], 1).astype(np.float32)
        z = torch.zeros(1, 4)
        da = O.apply_deltas(z, torch.from_numpy(A)[None], (10.0, 10.0, 5.0, 5.0))
        db = O.apply_deltas(z.expand(tries, 4), torch.from_numpy(Bb), (10.0, 10.0, 5.0, 5.0))
        iou = O.pair_iou(da + off, db + off).numpy().astype(np.float64)
        diff = (iou - t) / u
        side = (-1, 1)[k % 2]
        m = ((diff < 0) & (diff >= -4)) if side < 0 else ((diff > 0) & (diff <= 4))
        j = np.nonzero(m)[0]
        if len(j) == 0:
            continue
        s = 2.0 - 0.01 * k
        ra = det_row(c, 0, A, [cls], logits=[s])
        rb = det_row(c, 0, Bb[j[0]], [cls], logits=[s - 0.005])
        c.pairs.append((0, ra, rb, cls))
        k += 1
        if k >= 44:
            break
    for j, m in enumerate((1.0, 2.0, 0.5, 4.0)):                # exact: A [x, x + 10 m], B [x + 5 m, x + 10 m]
        x0, y0 = 100.0 + 60.0 * j, 860.0
        cls = (0, 64, 126, 9)[j]
        ra = det_row(c, 0, [x0, y0, x0 + 10 * m, y0 + 16.0], [cls], logits=[1.0])
        rb = det_row(c, 0, [x0 + 5 * m, y0, x0 + 10 * m, y0 + 16.0], [cls], logits=[0.9])
        c.pairs.append((0, ra, rb, cls))
    return c


def det_pair_ious(c: DetCase):
    f = 0
    n = int(c.n_prop[f])
    pb = torch.from_numpy(c.props[f, :n, :4].copy())
    de = torch.from_numpy(c.head[f, :n, c.K + 1:5 * c.K + 1].copy())
    boxes = O.clip_boxes(O.apply_deltas(de, pb, (10.0, 10.0, 5.0, 5.0)).reshape(-1, 4), *c.image_size).view(n, c.K, 4)
    p = det_probs(c, f)[:, :c.K]
    mx = boxes[p > c.score_thresh].max()
    out = []
    for (_, ra, rb, cls) in c.pairs:
        off = torch.tensor(float(cls)) * (mx + torch.tensor(1.0))
        out.append(float(O.pair_iou(boxes[ra, cls] + off, boxes[rb, cls] + off)))
    return np.array(out, np.float32)


@lru_cache(maxsize=None)
def det_cases() -> Dict[str, DetCase]:
    cases = [_det_full_case(), _det_mixed_case(1), _det_mixed_case(80), _det_mixed_case(127), _det_three_persons(),
             _det_near_iou()]
    assert [c.name for c in cases] == DET_NAMES
    return {c.name: c for c in cases}
