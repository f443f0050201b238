"""extract_frame_tree on the GPU with the tiny extractors of tests/test_extract.py: the driver feeds the pixels
vge.frames decodes from the folder's JPEGs, in RGB order, to TokenHMR and DWPose."""
import json

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN

DEV = "cuda:0"


class FullFrameDetector:
    """The gate detector's interface with one person box over the whole frame (the detector has its own tests)."""
    def detect(self, fr):
        F, H, W = (int(v) for v in fr.shape[:3])
        person = torch.zeros(F, 1, 5, device=fr.device)
        person[:, 0, :4] = torch.tensor([0.0, 0.0, W, H], device=fr.device)
        return {"person": person, "n_person": torch.ones(F, dtype=torch.int32, device=fr.device)}


@pytest.mark.gpu
def test_tree_driver_feeds_decoded_rgb_pixels_to_the_extractors(tmp_path):
    from vge import dwpose as D, hmr as H, synth
    from vge.extract import extract_frame_tree
    from vge.frames import load_frames
    gold = np.load(GOLDEN / "jpeg_golden.npz")
    hcfg = H.HmrConfig(embed_dim=256, depth=1, heads=4, mlp_dim=256, dec_dim=256, dec_depth=1, dec_heads=4,
                       dec_mlp=256, tok_num=4, tok_classes=256, tok_code_dim=256)
    hmr = H.HmrExtractor(synth.make_hmr_state_dict(hcfg), hcfg, device=DEV, max_frames=8)
    ycfg = D.YoloxConfig(in_size=128, width=16, depth=1, head_ch=64)
    pcfg = D.RtmposeConfig(in_h=128, in_w=96, stem_ch=16, stage_ch=(32, 64, 128, 256), stage_blocks=(1, 1, 1, 1))
    wb = D.Wholebody(D.YoloxDetector(synth.make_yolox_state_dict(ycfg), ycfg, device=DEV, chunk=8),
                     D.DwposeExtractor(synth.make_rtmpose_state_dict(pcfg), pcfg, device=DEV, max_instances=16))
    folders = []
    for v in range(2):
        d = tmp_path / "frames" / "Soccer" / f"v_s_{v:02d}"
        d.mkdir(parents=True)
        for f in range(6):
            (d / f"frame_{f:06d}.jpg").write_bytes(gold[f"jpeg/tree_v{v}_f{f}"].tobytes())
        folders.append(d)
    s = extract_frame_tree(hmr, wb, FullFrameDetector(), tmp_path / "frames", tmp_path / "meshes", tmp_path / "kps",
                           tmp_path / "logs", device=DEV)
    assert s["Soccer"]["single"] == ["v_s_00", "v_s_01"] and not s["Soccer"]["errors"]
    for v, d in enumerate(folders):
        frames, kept = load_frames(d, device=DEV)
        assert tuple(frames.shape) == (6, 128, 128, 3) and kept.tolist() == list(range(6))
        crops = H.crop_persons(frames, np.tile(np.array([0, 0, 128, 128], np.float32), (6, 1)))
        ref = hmr.extract(crops)
        z = np.load(tmp_path / "meshes" / "Soccer" / f"v_s_{v:02d}.npz")
        np.testing.assert_array_equal(z["frame_idx"], np.arange(6))
        np.testing.assert_array_equal(z["vit"], ref["vit"].cpu().numpy())
        # channel order matters to the model: BGR input gives other rows
        assert not np.array_equal(z["vit"], hmr.extract(crops.flip(-1).contiguous())["vit"].cpu().numpy())
        kp = np.load(tmp_path / "kps" / "Soccer" / f"v_s_{v:02d}" / "keypoints.npy")
        np.testing.assert_array_equal(kp, wb(frames).cpu().numpy())
        assert json.loads(str(z["meta"]))["action"] == "Soccer"
