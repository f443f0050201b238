"""The host layer the four native extractor models share (csrc/vge_model_host.h; vge.lib.NativeModel): loader
errors by name, per-call profiling that stops at its call budget, a workspace that grows to what a fresh reserve
gives, and the release of the workspace it supersedes.  All on the tiny configs of the per-model test files.
"""
import numpy as np
import pytest
import torch

from vge import lib as L
from vge import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _hmr_cfg():
    from vge.hmr import HmrConfig
    return HmrConfig(embed_dim=256, depth=2, heads=4, mlp_dim=1024, dec_dim=256, dec_depth=2, dec_heads=4,
                     dec_mlp=256, tok_num=4, tok_classes=256, tok_code_dim=256)


def _rtmpose_cfg():
    from vge.dwpose import RtmposeConfig
    return RtmposeConfig(in_h=128, in_w=96, stem_ch=16, stage_ch=(32, 64, 128, 256), stage_blocks=(1, 1, 1, 1))


def _yolox_cfg():
    from vge.dwpose import YoloxConfig
    return YoloxConfig(in_size=128, width=16, depth=1, head_ch=64)


def _frcnn_cfg():
    from vge.frcnn import FrcnnConfig
    return FrcnnConfig(depth=50, min_size=128, max_size=213, rpn_pre_topk=300, rpn_post_topk=200)


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------ loader errors by name
def _hmr_model(sd):
    from vge.hmr import HmrExtractor
    return HmrExtractor(sd, _hmr_cfg(), device=DEV, max_frames=1)


def _frcnn_model(sd):
    from vge.frcnn import FrcnnDetector
    return FrcnnDetector(sd, _frcnn_cfg(), device=DEV, chunk=1, frame_hw=(96, 80))


@pytest.mark.parametrize("make_sd,model,missing,reshaped", [
    (lambda: synth.make_hmr_state_dict(_hmr_cfg()), _hmr_model,
     "backbone.blocks.1.mlp.fc1.bias", "smpl_head.decpose.codebook"),
    (lambda: synth.make_frcnn_state_dict(_frcnn_cfg()), _frcnn_model,
     "backbone.bottom_up.res3.1.conv2.norm.running_var", "roi_heads.box_head.fc2.weight"),
], ids=["hmr", "frcnn"])
def test_loader_names_the_missing_and_the_misshapen_weight(make_sd, model, missing, reshaped):
    sd = make_sd()
    cut = {k: v for k, v in sd.items() if k != missing}
    with pytest.raises(L.VgeError, match="missing weight " + missing.replace(".", r"\.")):
        model(cut)
    bent = dict(sd)
    bent[reshaped] = np.ascontiguousarray(sd[reshaped].reshape(-1)[:-1])
    with pytest.raises(L.VgeError, match="wrong shape for " + reshaped.replace(".", r"\.")):
        model(bent)
    model(sd).close()  # the failed creates left nothing behind that stops the next one


# ------------------------------------------------------------------------------ profiling stops at its call budget
def test_hmr_profile_one_call_of_two():
    from vge.hmr import HmrExtractor
    cfg = _hmr_cfg()
    ex = HmrExtractor(synth.make_hmr_state_dict(cfg), cfg, device=DEV, max_frames=8)
    frames = torch.from_numpy(synth.make_frames(3, 5)).to(DEV)
    ex.profile_begin(1)
    first = {k: v.clone() for k, v in ex.extract(frames).items()}
    second = ex.extract(frames)
    torch.cuda.synchronize()
    ms, n, fl = ex.profile_read()
    assert n == 1 and ms["gemm"] > 0
    E, P, T = cfg.embed_dim, cfg.patch, 192  # gemm_flops of vge_hmr_create: per frame, the backbone's GEMMs
    want = 2.0 * T * (E * 3.0 * P * P + cfg.depth * (E * 3.0 * E + 1.0 * E * E + 2.0 * E * cfg.mlp_dim))
    assert abs(fl - want) <= 1e-9 * want
    for k in first:
        assert torch.equal(first[k], second[k]), k
    ex.close()


def test_yolox_profile_one_call_of_two():
    from vge.dwpose import YoloxDetector, yolox_flops
    cfg = _yolox_cfg()
    det = YoloxDetector(synth.make_yolox_state_dict(cfg), cfg, device=DEV, chunk=2)
    frames = torch.from_numpy(synth.make_frames(7, 3, 240, 320)).to(DEV)  # two chunks
    det.profile_begin(1)
    b1, n1 = det.detect(frames)
    b2, n2 = det.detect(frames)
    torch.cuda.synchronize()
    ms, n, fl = det.profile_read()
    assert n == 1 and ms["gemm"] > 0
    want = 3 * yolox_flops(cfg)
    assert abs(fl - want) <= 1e-9 * want
    assert torch.equal(b1, b2) and torch.equal(n1, n2)
    det.close()


def test_rtmpose_profile_one_call_of_two():
    from vge.dwpose import DwposeExtractor, rtmpose_flops
    cfg = _rtmpose_cfg()
    ex = DwposeExtractor(synth.make_rtmpose_state_dict(cfg), cfg, device=DEV, max_instances=8)
    frames = torch.from_numpy(synth.make_frames(3, 8)).to(DEV)
    ex.profile_begin(1)
    k1 = ex.keypoints(frames).clone()
    k2 = ex.keypoints(frames)
    torch.cuda.synchronize()
    ms, n, fl = ex.profile_read()
    assert n == 1 and ms["gemm"] > 0
    # as test_dwpose.test_extractor_profile_and_flops: the dense work minus the GAU token mixing (not a GEMM launch)
    want = 8 * (rtmpose_flops(cfg) - 2.0 * cfg.keypoints ** 2 * (cfg.gau_s + cfg.gau_e))
    assert abs(fl - want) <= 1e-9 * want
    assert torch.equal(k1, k2)
    ex.close()


# ------------------------------------------------------------------------------ growth = a fresh reserve
def test_hmr_grown_workspace_equals_fresh():
    from vge.hmr import HmrExtractor
    cfg = _hmr_cfg()
    sd = synth.make_hmr_state_dict(cfg)
    a, b = 2, 300  # head rows pad to 256 and 512, token rows to 512 and 57,600
    frames = torch.from_numpy(synth.make_frames(5, b)).to(DEV)
    grown = HmrExtractor(sd, cfg, device=DEV, max_frames=a)
    grown.extract(frames[:a])
    got = grown.extract(frames)  # grows on demand
    fresh = HmrExtractor(sd, cfg, device=DEV, max_frames=b)
    want = fresh.extract(frames)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    grown.close()
    fresh.close()


def test_rtmpose_grown_workspace_equals_fresh():
    from vge.dwpose import DwposeExtractor
    cfg = _rtmpose_cfg()
    sd = synth.make_rtmpose_state_dict(cfg)
    a, b = 1, 3  # every buffer is sized by the instance count itself
    frames = torch.from_numpy(synth.make_frames(9, b)).to(DEV)
    grown = DwposeExtractor(sd, cfg, device=DEV, max_instances=a)
    grown.keypoints(frames[:a])
    got = grown.keypoints(frames)  # grows on demand
    fresh = DwposeExtractor(sd, cfg, device=DEV, max_instances=b)
    assert torch.equal(got, fresh.keypoints(frames))
    grown.close()
    fresh.close()


def test_yolox_grown_workspace_equals_fresh():
    from vge.dwpose import YoloxDetector
    cfg = _yolox_cfg()
    sd = synth.make_yolox_state_dict(cfg)
    a, b = 1, 3  # frames per workspace pass
    frames = torch.from_numpy(synth.make_frames(7, b, 240, 320)).to(DEV)
    grown = YoloxDetector(sd, cfg, device=DEV, chunk=a)
    grown.detect(frames[:a])
    with torch.cuda.device(DEV):
        L.check(grown.lib.vge_yolox_reserve(grown.h, b), "vge_yolox_reserve")
    got = grown.detect(frames)
    fresh = YoloxDetector(sd, cfg, device=DEV, chunk=b)
    want = fresh.detect(frames)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    grown.close()
    fresh.close()


# ------------------------------------------------------------------------------ a superseded workspace is released
def test_superseded_workspace_is_released():
    """Device memory in use (hipMemGetInfo) with an RTMPose model reserved at a, at b, and at a then grown to b: the
    grown model holds what the fresh b model holds, not the a workspace on top of it.  At a = 160 instances the tiny
    config's workspace is ~2.3 MB x 160 (asserted >= 256 MiB), far above the allocator's granularity over its 23
    buffers, so half of it separates "released" from "kept" (before the shared Workspace: the whole of it was kept)."""
    from vge.dwpose import DwposeExtractor
    cfg = _rtmpose_cfg()
    sd = synth.make_rtmpose_state_dict(cfg)
    a, b = 160, 224

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info(DEV)
        return total - free

    DwposeExtractor(sd, cfg, device=DEV, max_instances=1).close()  # the runtime's one-off allocations
    base = used()

    def footprint(first, then=None):
        ex = DwposeExtractor(sd, cfg, device=DEV, max_instances=first)
        if then is not None:
            ex.reserve(then)
        n = used() - base
        ex.close()
        return n

    fa, fb, grown = footprint(a), footprint(b), footprint(a, b)
    print(f"footprint MiB: a={a}: {fa / 2**20:.1f}, b={b}: {fb / 2**20:.1f}, a then b: {grown / 2**20:.1f}")
    assert fa >= 256 * 2**20
    assert grown - fb < fa / 2
