"""GPU parity of TokenHMR's gate detector (detectron2 Faster R-CNN X101-32x8d-FPN, modifications/mesh_generator.py:69-73,
103-117) through the C ABI (include/vge_frcnn.h) against oracle/frcnn.py, at full width and the reference's 800-pixel
input on four 256 x 256 frames (two chunks of the workspace).

Every stage is checked on the GPU's own input to that stage, so a tolerance covers one stage's arithmetic (the check
bodies live in tests/frcnn_checks.py, shared with the non-square geometries of tests/test_frcnn_shapes.py):
  resize        the PIL bilinear resample, byte for byte
  backbone+FPN  P2..P6 vs the oracle run from the frames (bf16 storage points, 101 layers: relative L2 < 3e-2)
  RPN head      logits / deltas from the GPU's P levels (one bf16 conv + f32 1x1)
  proposals     top-k / decode / clip / batched NMS / merge from the GPU's logits: identical order and scores
  ROIAlign      from the GPU's P levels and proposals: torchvision's float order, identical but for rare 1-ulp bf16
  box head      fc1 / fc2 / predictor from the GPU's box features
  inference     softmax / per-class decode / NMS / top 100 / postprocess from the GPU's head: identical instances
  gate          the person count of mesh_generator.py:106-108, and the whole predictor end to end vs the oracle
Parity vs detectron2's trained model is UNPINNED (code and weights absent offline; random weights of the reference's
shapes, vge.synth.make_frcnn_state_dict).
"""
import pytest
import torch

from tests import frcnn_checks as K

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NF = 4


@pytest.fixture(scope="module")
def run():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vge import synth
    from vge.frcnn import FRCNN_X101, FrcnnDetector
    cfg = FRCNN_X101
    sd = synth.make_frcnn_state_dict(cfg)
    det = FrcnnDetector(sd, cfg, device=DEV, chunk=3)          # 4 frames = two chunks (tap / output offsets)
    r = K.collect_run(det, sd, cfg, synth.make_frame_pool(9100, NF), DEV)
    det.close()
    return r


@pytest.fixture(scope="module")
def oracle_fwd(run):
    """The oracle predictor from the frames themselves, on the first two frames."""
    return K.oracle_forward(run, (0, 1))


def test_resize_is_pil_bilinear(run):
    K.check_resize(run)


def test_backbone_fpn_vs_oracle(run, oracle_fwd):
    K.check_backbone_fpn(run, oracle_fwd[1], (0, 1))


def test_rpn_head_vs_oracle(run):
    K.check_rpn_head(run, (0, 1))


def test_proposals_vs_oracle_on_gpu_logits(run):
    K.check_proposals(run)


def test_box_features_vs_oracle_on_gpu_levels(run):
    K.check_box_features(run, (0, 1))


def test_roi_align_separable_matches_sample_order(run):
    """The default ROIAlign (separable per-bin cell weights, roi_align_sep_kernel) against torchvision's sample order
    (roi_align_kernel, vge_debug_set_roi_direct) on the same levels and proposals: the same sums reassociated, so
    bins identical but for rare 1-ulp bf16 differences.  The separable kernel's sample-loop branch (taken for bins
    wider than its LDS tables, forced here for every ROI) is roi_align_kernel's arithmetic: identical."""
    from vge import synth
    K.check_roi_modes(run["sd"], run["cfg"], synth.make_frame_pool(9100, NF), DEV, chunk=NF)


def test_stem_pool_fused_matches_split(run):
    """The fused stem conv + ReLU + max pool (frcnn_stem_pool_kernel, default) against the stem conv kernel followed by
    the max-pool kernel (vge_debug_set_stem_split): the same MFMA K order and bf16 rounding point, so P2..P6 agree to
    the conv kernel's own summation differences and the gate's person counts are the same."""
    from vge import synth
    K.check_stem_fused_vs_split(run["sd"], run["cfg"], synth.make_frame_pool(9100, NF), DEV, chunk=NF)


def test_box_head_vs_oracle_on_gpu_features(run):
    K.check_box_head(run, (0, 1))


def test_inference_and_postprocess_vs_oracle_on_gpu_head(run):
    K.check_inference_postprocess(run, min_checked=2)


def test_predictor_end_to_end_vs_oracle(run, oracle_fwd):
    """The whole predictor from the frames: the oracle's instances are found among the GPU's (same class, IoU > 0.9,
    score within 0.05) and the gate's person count agrees unless an oracle person score is within 0.05 of 0.5."""
    K.check_end_to_end(run, oracle_fwd[0], (0, 1))


@pytest.mark.parametrize("gw,stride,C,H,W", [(8, 1, 256, 20, 37), (16, 2, 512, 21, 18), (32, 1, 1024, 13, 11),
                                             (64, 1, 2048, 9, 10), (32, 2, 1024, 14, 13), (64, 2, 2048, 7, 6),
                                             (8, 2, 256, 15, 16), (16, 1, 512, 10, 33),
                                             (32, 1, 1024, 50, 50), (16, 1, 512, 100, 100), (8, 1, 256, 200, 200),
                                             (32, 2, 1024, 100, 100), (16, 2, 512, 200, 200), (32, 1, 1024, 51, 47)])
def test_grouped_conv_kernel_vs_torch(gw, stride, C, H, W):
    """The bottlenecks' grouped 3x3 conv (vge_gconv.hip: + folded bias, ReLU) alone vs torch conv2d(groups = C / gw)
    in f32 on the same bf16 operands: every group width of X101-32x8d (8 .. 64 channels per group), both strides,
    ragged tiles (group widths 8 / 16 run two taps per 16x16x32 MFMA, the ninth against zero weights; 32 / 64 one or
    two MFMAs per tap).  The kernel rounds its f32 sums to bf16 once.  The output tile is picked per shape
    (gc_pick_tile): the detector's 200 / 100 / 50-wide maps at both strides take tiles whose 16-pixel groups run across
    rows (5 x 25, 6 x 10), the small shapes whole-image tiles, 51 x 47 a partial last group."""
    _gconv_check(gw, stride, C, H, W, 2)


def _gconv_run(x, w, b, gw, stride):
    """vge_debug_gconv3 on x bf16 [n, H, W, C] (host) -> bf16 [n, Ho, Wo, C] (host), over a NaN pre-fill"""
    import ctypes as C_
    from vge import lib as L
    so = L.load()
    n, H, W, C = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xd = x.to(DEV)
    out = torch.full((n, Ho, Wo, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    rc = so.vge_debug_gconv3(C_.c_void_p(xd.data_ptr()), n, H, W, C, gw, stride, C_.c_void_p(w.data_ptr()),
                             C_.c_void_p(b.data_ptr()), C_.c_void_p(out.data_ptr()), C_.c_void_p(st))
    assert rc == 0, L.load().vge_last_error()
    return out.cpu()


def _gconv_check(gw, stride, C, H, W, n):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(gw * 7 + stride)
    x = torch.randn((n, H, W, C), generator=g).to(torch.bfloat16)
    w = (torch.randn((C, gw, 3, 3), generator=g) / (3.0 * gw ** 0.5)).float()
    b = (0.1 * torch.randn(C, generator=g)).float()
    out = _gconv_run(x, w, b, gw, stride)
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.to(torch.bfloat16).float(), b, stride=stride, padding=1,
                   groups=C // gw).relu().permute(0, 2, 3, 1)
    got = out.float()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    bound = 2.0 ** -7 * ref.abs() + 1e-4          # one bf16 rounding of the output (+ f32 summation order)
    print(f"gw {gw} stride {stride} n {n}: max |d| {err.max():.2e}, max |ref| {ref.abs().max():.2e}, "
          f"worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err - bound).max())
    return x, w, b, out


@pytest.mark.parametrize("n", [1, 8, 9, 17])
@pytest.mark.parametrize("gw,stride,C,H,W", [(8, 1, 256, 20, 37), (16, 2, 512, 21, 18), (32, 1, 1024, 13, 11),
                                             (64, 1, 2048, 9, 10), (32, 2, 1024, 14, 13), (64, 2, 2048, 7, 6),
                                             (8, 2, 256, 15, 16), (16, 1, 512, 10, 33)])
def test_grouped_conv_image_groups(gw, stride, C, H, W, n):
    """The same bound at 1, 8, 9 and 17 images per call, one small shape per kernel template (group widths 8 / 16, 32
    and 64, each at stride 1 and 2): a workgroup of gconv3_kernel loops over up to GC_NI = 8 images with the next
    image's loads in flight, so 8 is one full group, 9 and 17 end in a group of one, 1 is a group of one alone.  Image
    i of the 17-image call equals the same image run alone, bit for bit."""
    x, w, b, out = _gconv_check(gw, stride, C, H, W, n)
    if n == 17:
        for i in range(n):
            one = _gconv_run(x[i:i + 1].contiguous(), w, b, gw, stride)
            assert torch.equal(one[0].view(torch.int16), out[i].view(torch.int16)), f"image {i} differs when run alone"


def test_chunk_cap_and_128_frame_chunk_matches_64(run):
    """Activations are addressed through 64-bit offsets (the 1x1 convs' GEMM epilogue included), so a chunk is bounded
    only by int32 row / thread counts: 838 frames at 800 px (vge_frcnn_reserve refuses one more before allocating).
    A 128-frame chunk -- T1 of res3.0's conv1 then holds 2.6e9 elements, past the old 2 GiB cap of 104 frames -- gives
    the same detections, bit for bit, as the same frames in 64-frame chunks (every kernel is per frame or per output
    element with a fixed K order, and the tuner's conv variants are bit-identical).  Run with the library path off:
    hipBLASLt's stream-K algorithms split a GEMM's K loop by its tile count, so the library's 1x1 convs are not
    bit-stable across M (test_chunk_128_with_library_gemms_matches_64 bounds them instead)."""
    import ctypes as C
    from vge import synth
    from vge.frcnn import FrcnnDetector
    frames = torch.from_numpy(synth.make_frame_pool(9300, 128)).to(DEV)
    outs = {}
    lib = L_load()
    lib.vge_debug_set_gemm_lib.argtypes = [C.c_int]
    lib.vge_debug_set_gemm_lib(0)
    for chunk in (128, 64):
        det = FrcnnDetector(run["sd"], run["cfg"], device=DEV, chunk=chunk)
        try:
            if chunk == 128:
                cap = det.max_chunk(256, 256)
                assert cap == 838, cap
                assert det.lib.vge_frcnn_reserve(det.h, cap + 1, 256, 256) == 1      # VGE_ERR_ARG, nothing allocated
            assert det.chunk == chunk
            o = det.detect(frames)
            torch.cuda.synchronize()
            outs[chunk] = {k: v.cpu() for k, v in o.items()}
        finally:
            det.close()
            if chunk == 64:
                lib.vge_debug_set_gemm_lib(1)
        torch.cuda.empty_cache()
    for k in outs[64]:
        assert torch.equal(outs[128][k], outs[64][k]), k
    print(f"128-frame chunk == 2 x 64: {int(outs[64]['n_dets'].sum())} instances, "
          f"{int((outs[64]['n_person'] == 1).sum())} single-person frames")


def L_load():
    from vge import lib as L
    return L.load()


def test_chunk_128_with_library_gemms_matches_64(run):
    """The default path (1x1 convs on hipBLASLt): a 128-frame chunk's FPN maps agree with 64-frame chunks' to the
    library GEMMs' f32 summation-order differences carried through the network (bf16 storage), and the gate's person
    counts agree on every frame whose best person score is not within 0.05 of the gate threshold."""
    from vge import synth
    from vge.frcnn import FrcnnDetector
    frames = torch.from_numpy(synth.make_frame_pool(9300, 128)).to(DEV)
    outs = {}
    for chunk in (128, 64):
        det = FrcnnDetector(run["sd"], run["cfg"], device=DEV, chunk=chunk)
        try:
            taps = det.make_taps(128, 256, 256)
            o = det.detect(frames, taps=taps)
            torch.cuda.synchronize()
            outs[chunk] = ({k: v.cpu() for k, v in o.items()}, [t.float().cpu() for t in taps["fpn"]])
        finally:
            det.close()
        torch.cuda.empty_cache()
    for lv, (a, b) in enumerate(zip(outs[128][1], outs[64][1])):
        rel = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
        print(f"P{lv + 2}: max |d| / max |P| = {rel:.2e}")
        assert rel < 5e-2, (lv, rel)
    d128, d64 = outs[128][0], outs[64][0]
    same = (d128["n_person"] == d64["n_person"])
    assert float(same.float().mean()) >= 0.95, float(same.float().mean())
