"""The gate detector (vge.frcnn.FrcnnDetector, include/vge_frcnn.h) at the frame geometries tests/test_frcnn.py never
reaches.  There every frame is 256 x 256 -> 800 x 800: square, upscaled, and already a multiple of 32, so an H / W
swap, the zero-padded border, odd level sizes, PIL's widened downscaling support, the MAX_SIZE_TEST cap, the workspace
rebuild on a new frame size and the ROI features' own allocation are all invisible.  Here the same stage-wise checks
(tests/frcnn_checks.py, the same thresholds) run at

  cfg (min, max)  frame H x W   resized      padded       P2 .. P6                               what it adds
  200, 333         96 x 160     200 x 333    224 x 352    56x88 28x44 14x22 7x11 4x6             landscape, cap, pad on both axes, odd P5
  200, 333        160 x  96     333 x 200    352 x 224    transposed                             portrait: any H / W swap
  200, 333        300 x 260     231 x 200    256 x 224    64x56 32x28 16x14 8x7 4x4              downscale: 5-tap PIL support on both axes
  200, 333         90 x 160     187 x 333    192 x 352    48x88 24x44 12x22 6x11 3x6             odd nh, 5 pad rows, even x odd P5
   64, 107         48 x  80      64 x 107     64 x 128    16x32 8x16 4x8 2x4 1x2                 every level under one tile, k = 6 on P6
  800, 1333       144 x 256     750 x 1333   768 x 1344   192x336 96x168 48x84 24x42 12x21       the reference's config on 16:9

with full-width weights (synth.make_frcnn_state_dict(FRCNN_X101)).  Rows 1-5: five frames in chunks of two (three
chunks, a one-frame tail), every stage check, the from-frames oracle on the first two frames.  Row 6: one frame,
everything downstream of the FPN on the GPU's own taps plus the resize (rows 1-5 pin the backbone).  The tiny row was
read through the launch paths before its first run (conv / GEMM tiles guard their rows past M, the grouped conv and the
fused stem + pool guard ragged tiles, the RPN select takes k = min(pre_topk, h w 3)): it is supported, so it runs
against the oracle like the others.  What the code cannot support is a frame whose short edge rounds to 0 pixels under
the max_size cap (aspect ratio above ~2 max_size): that is refused, and the last accepted frame beside it (one resized
row) runs against the oracle.

Also: the ROIAlign and stem A/B paths at rows 1 and 3, one detector switching frame sizes (bit-stable, equal to a fresh
detector), and a CPU test of the proposal check itself (landscape RPN outputs read with the portrait geometry, or with
only the clip size swapped, must fail it).
"""
import dataclasses

import pytest
import torch

from tests import frcnn_checks as K

DEV = "cuda:0"
gpu = pytest.mark.gpu

# (min_size, max_size, H, W) -> (resized, padded, levels P2..P6), computed by hand from ResizeShortestEdge / pad-to-32
ROWS = [
    ((200, 333, 96, 160), ((200, 333), (224, 352), [(56, 88), (28, 44), (14, 22), (7, 11), (4, 6)])),
    ((200, 333, 160, 96), ((333, 200), (352, 224), [(88, 56), (44, 28), (22, 14), (11, 7), (6, 4)])),
    ((200, 333, 300, 260), ((231, 200), (256, 224), [(64, 56), (32, 28), (16, 14), (8, 7), (4, 4)])),
    ((200, 333, 90, 160), ((187, 333), (192, 352), [(48, 88), (24, 44), (12, 22), (6, 11), (3, 6)])),
    ((64, 107, 48, 80), ((64, 107), (64, 128), [(16, 32), (8, 16), (4, 8), (2, 4), (1, 2)])),
    ((800, 1333, 144, 256), ((750, 1333), (768, 1344), [(192, 336), (96, 168), (48, 84), (24, 42), (12, 21)])),
]
IDS = [f"{k[0]}-{k[1]}-{k[2]}x{k[3]}" for k, _ in ROWS]
SEEDS = [9400, 9401, 9402, 9403, 9404, 9405]  # a row whose inference check skips more than allowed takes another seed
NF, CHUNK = 5, 2
TAIL = (0, NF - 1)  # a first-chunk frame and the tail chunk's only frame


def _cfg(mn, mx):
    from vge.frcnn import FRCNN_X101
    return dataclasses.replace(FRCNN_X101, min_size=mn, max_size=mx)


def test_geometry_table_is_the_oracles():
    """The table above against oracle.frcnn.output_shape / pil_coeffs on the CPU: the sizes, the cap, the pad, the level
    pyramid and the PIL support (5 taps where the frame is downscaled, 3 where it is upscaled)."""
    from oracle.frcnn import output_shape, pil_coeffs
    for (mn, mx, H, W), (resized, padded, levels) in ROWS:
        nh, nw = output_shape(H, W, mn, mx)
        assert (nh, nw) == resized
        hp, wp = -(-nh // 32) * 32, -(-nw // 32) * 32
        assert (hp, wp) == padded
        lv = [(hp >> (l + 2), wp >> (l + 2)) for l in range(4)]
        lv.append((((hp >> 5) - 1) // 2 + 1, ((wp >> 5) - 1) // 2 + 1))
        assert lv == levels
        assert max(nh, nw) <= mx and (min(nh, nw) == mn or max(nh, nw) == mx)
        for a, b in ((H, nh), (W, nw)):
            assert pil_coeffs(a, b)[2].shape[1] == (5 if a > b else 3), (a, b)
    # what each row is there for
    assert ROWS[1][1][2] == [(w, h) for h, w in ROWS[0][1][2]]                  # portrait = landscape transposed
    assert all(r[1][1] != r[1][0] for r in ROWS[:4])                             # rows 1-4: a padded border exists
    assert ROWS[3][1][0][0] % 2 == 1 and ROWS[3][1][1][0] - ROWS[3][1][0][0] == 5
    assert ROWS[4][1][2][4] == (1, 2)                                            # 6 anchors on the tiny row's P6


def test_proposal_check_sees_an_h_w_swap():
    """A test of the check itself, on the CPU: RPN outputs the oracle's head computes on random landscape levels (row
    1's sizes), laid out as the detector's taps with the oracle's own proposals, pass check_proposals at row 1's
    geometry and fail it when read with row 2's (level sizes and the clip size transposed)."""
    from oracle.frcnn import OracleFrcnn
    from vge import synth
    from vge.frcnn import FrcnnConfig
    cfg = dataclasses.replace(FrcnnConfig(depth=50), min_size=200, max_size=333)
    o = OracleFrcnn(synth.make_frcnn_state_dict(cfg), cfg, bf16=True)
    (r1, _, lv1), (r2, _, lv2) = ROWS[0][1], ROWS[1][1]
    g = torch.Generator().manual_seed(7)
    rpn, lo, de = [], [], []
    for h, w in lv1:
        l_, d_ = o.rpn_head(torch.randn((1, cfg.fpn_ch, h, w), generator=g))
        lo.append(l_[0])
        de.append(d_[0])
        rpn.append(torch.cat([l_.view(1, h, w, 3), d_.view(1, h, w, 12), torch.zeros(1, h, w, 1)], -1))
    pb, ps = o.proposals(lo, de, r1, lv1)
    assert pb.shape[0] > 10
    props = torch.zeros((1, cfg.rpn_post_topk, 5))
    props[0, :pb.shape[0], :4], props[0, :pb.shape[0], 4] = pb, ps
    taps = dict(rpn=rpn, proposals=props, n_proposals=torch.tensor([pb.shape[0]], dtype=torch.int32))
    run = dict(oracle=o, taps=taps, shapes=dict(levels=lv1, resized=r1))
    K.check_proposals(run)
    with pytest.raises(AssertionError):
        K.check_proposals(run, shapes=dict(levels=lv2, resized=r2))
    with pytest.raises(AssertionError):                      # the clip size alone: nh / nw swapped in clip_boxes
        K.check_proposals(run, shapes=dict(levels=lv1, resized=r2))


@pytest.fixture(scope="module")
def sd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vge import synth
    from vge.frcnn import FRCNN_X101
    return synth.make_frcnn_state_dict(FRCNN_X101)


def _frames(i):
    from vge import synth
    mn, mx, H, W = ROWS[i][0]
    return synth.make_frame_pool(SEEDS[i], 1 if i == 5 else NF, h=H, w=W)


@pytest.fixture(scope="module")
def runs(sd):
    """row index -> the run dict of frcnn_checks (one taps-on detect on a detector built for that row), made on first
    use: the first test below asks for the rows in the table's order."""
    from vge.frcnn import FrcnnDetector
    cache = {}

    def get(i):
        if i not in cache:
            mn, mx, H, W = ROWS[i][0]
            cfg = _cfg(mn, mx)
            det = FrcnnDetector(sd, cfg, device=DEV, chunk=CHUNK, frame_hw=(H, W))
            try:
                cache[i] = K.collect_run(det, sd, cfg, _frames(i), DEV)
            finally:
                det.close()
        return cache[i]
    return get


@pytest.fixture(scope="module")
def fwds(runs):
    cache = {}

    def get(i):
        if i not in cache:
            cache[i] = K.oracle_forward(runs(i), (0, 1))
        return cache[i]
    return get


ALL = pytest.mark.parametrize("row", range(6), ids=IDS)
SMALL = pytest.mark.parametrize("row", range(5), ids=IDS[:5])


@gpu
@ALL
def test_shapes_and_resize(runs, row):
    """vge_frcnn_shapes equals the table, the taps have those sizes, and the resize is PIL's byte for byte (the padded
    border never reaches the tap; the backbone check below sees it)."""
    run = runs(row)
    resized, padded, levels = ROWS[row][1]
    sh = run["shapes"]
    assert tuple(sh["resized"]) == resized and tuple(sh["padded"]) == padded
    assert [tuple(s) for s in sh["levels"]] == levels
    assert tuple(run["taps"]["resized"].shape[1:3]) == resized
    K.check_resize(run)


@gpu
@SMALL
def test_backbone_fpn_vs_oracle(runs, fwds, row):
    K.check_backbone_fpn(runs(row), fwds(row)[1], (0, 1))


@gpu
@ALL
def test_rpn_head_vs_oracle(runs, row):
    K.check_rpn_head(runs(row), (0,) if row == 5 else tuple(range(NF)))


@gpu
@ALL
def test_proposals_vs_oracle_on_gpu_logits(runs, row):
    K.check_proposals(runs(row))


@gpu
@ALL
def test_box_features_vs_oracle_on_gpu_levels(runs, row):
    K.check_box_features(runs(row), (0,) if row == 5 else TAIL)


@gpu
@ALL
def test_box_head_vs_oracle_on_gpu_features(runs, row):
    K.check_box_head(runs(row), (0,) if row == 5 else TAIL)


@gpu
@ALL
def test_inference_and_postprocess_vs_oracle_on_gpu_head(runs, row):
    K.check_inference_postprocess(runs(row), min_checked=1 if row == 5 else 4)


@gpu
@SMALL
def test_predictor_end_to_end_vs_oracle(runs, fwds, row):
    K.check_end_to_end(runs(row), fwds(row)[0], (0, 1))


@gpu
@pytest.mark.parametrize("row", [0, 2], ids=[IDS[0], IDS[2]])
def test_roi_align_separable_matches_sample_order(sd, row):
    mn, mx = ROWS[row][0][:2]
    K.check_roi_modes(sd, _cfg(mn, mx), _frames(row), DEV, chunk=CHUNK)


@gpu
@pytest.mark.parametrize("row", [0, 2], ids=[IDS[0], IDS[2]])
def test_stem_pool_fused_matches_split(sd, row):
    mn, mx = ROWS[row][0][:2]
    K.check_stem_fused_vs_split(sd, _cfg(mn, mx), _frames(row), DEV, chunk=CHUNK)


def _detect_all(det, frames):
    F_, H, W = (int(v) for v in frames.shape[:3])
    taps = det.make_taps(F_, H, W)
    out = det.detect(torch.from_numpy(frames).to(DEV), taps=taps)
    torch.cuda.synchronize()
    flat = {f"out.{k}": v.cpu() for k, v in out.items()}
    for k, v in taps.items():
        for j, x in enumerate(v if isinstance(v, list) else [v]):
            flat[f"tap.{k}.{j}"] = x.cpu()
    return flat


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


@gpu
def test_one_detector_switches_frame_sizes(sd):
    """One detector built at the default 256 x 256 detects row 1's frames, row 3's, then row 1's again (the workspace,
    the PIL tables and the alias table are rebuilt each time): the third result is the first bit for bit, outputs and
    taps, and row 3's is that of a fresh detector built for 300 x 260.  With the library GEMMs off, as the chunk test
    runs for bit-stability (hipBLASLt's stream-K algorithms are not bit-stable across launches' M)."""
    import ctypes as C
    from vge import lib as L
    from vge.frcnn import FrcnnDetector
    lib = L.load()
    lib.vge_debug_set_gemm_lib.argtypes = [C.c_int]
    cfg = _cfg(200, 333)
    f1, f3 = _frames(0), _frames(2)
    lib.vge_debug_set_gemm_lib(0)
    try:
        det = FrcnnDetector(sd, cfg, device=DEV, chunk=CHUNK)
        try:
            assert det.frame_hw == (256, 256)
            a = _detect_all(det, f1)
            b = _detect_all(det, f3)
            assert det.frame_hw == (300, 260)
            c = _detect_all(det, f1)
        finally:
            det.close()
        fresh = FrcnnDetector(sd, cfg, device=DEV, chunk=CHUNK, frame_hw=(300, 260))
        try:
            d = _detect_all(fresh, f3)
        finally:
            fresh.close()
    finally:
        lib.vge_debug_set_gemm_lib(1)
    _same(c, a, "row 1 again vs row 1")
    _same(b, d, "row 3 after a switch vs a fresh detector")
    assert int(a["out.n_dets"].sum()) > 0 and int(b["out.n_dets"].sum()) > 0


@gpu
def test_frame_that_resizes_to_nothing_is_refused_and_the_next_runs(sd):
    """ResizeShortestEdge under the max_size cap rounds the short edge of a 1 x W frame to int(333 / W + 0.5) pixels:
    1 x 667 resizes to 0 x 333, which has no shape downstream (PIL refuses an empty resize).  vge_frcnn_shapes and
    vge_frcnn_reserve refuse it with VGE_ERR_ARG and a message before any launch, detect raises and leaves the detector
    usable; 1 x 666 -- one resized row, 32 padded ones, P5 1 x 11 -- is the last accepted frame and runs against the
    oracle: resize, RPN head, proposals, ROIAlign, box head, inference."""
    from oracle.frcnn import output_shape
    from vge import lib as L, synth
    from vge.frcnn import FrcnnDetector
    cfg = _cfg(200, 333)
    assert output_shape(1, 667, 200, 333) == (0, 333) and output_shape(1, 666, 200, 333) == (1, 333)
    ok = synth.make_frame_pool(9410, 3, h=1, w=666)
    det = FrcnnDetector(sd, cfg, device=DEV, chunk=CHUNK, frame_hw=(1, 666))
    try:
        assert det.lib.vge_frcnn_reserve(det.h, 1, 1, 667) == 1                  # VGE_ERR_ARG
        assert "0 x 333" in L.load().vge_last_error().decode()
        assert det.lib.vge_frcnn_reserve(det.h, 1, 667, 1) == 1
        with pytest.raises(L.VgeError, match="rounds to 0 pixels"):
            det.shapes(1, 667)
        with pytest.raises(L.VgeError, match="rounds to 0 pixels"):
            det.detect(torch.zeros((1, 1, 667, 3), dtype=torch.uint8, device=DEV))
        assert det.frame_hw == (1, 666)
        run = K.collect_run(det, sd, cfg, ok, DEV)
    finally:
        det.close()
    assert tuple(run["shapes"]["resized"]) == (1, 333) and tuple(run["shapes"]["padded"]) == (32, 352)
    assert [tuple(s) for s in run["shapes"]["levels"]] == [(8, 88), (4, 44), (2, 22), (1, 11), (1, 6)]
    K.check_resize(run)
    K.check_rpn_head(run, (0, 2))
    K.check_proposals(run)
    K.check_box_features(run, (0, 2))
    K.check_box_head(run, (0, 2))
    K.check_inference_postprocess(run, min_checked=2)
