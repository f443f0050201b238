"""vge.extract.extract_frame_tree (the reference's extract_mesh.py:150-241 + process_video.py:59-94 over frame folders)
on the host JPEG path with stub models that return rows computed from the pixels they are given: bookkeeping, resume,
error isolation.  No GPU needed."""
import json

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN


class Calls:
    def __init__(self):
        self.n = {"detect": 0, "kp": 0, "hmr": 0}


class StubDetector:
    """One person box on every 64-wide frame, two on frames of any other width; raises on a poisoned frame."""
    def __init__(self, calls, poison=None):
        self.calls, self.poison = calls, poison

    def detect(self, fr):
        self.calls.n["detect"] += 1
        F, H, W = (int(v) for v in fr.shape[:3])
        if self.poison is not None and any(torch.equal(f, self.poison) for f in fr):
            raise RuntimeError("boom: poisoned frame")
        person = torch.zeros(F, 1, 5)
        person[:, 0, :4] = torch.tensor([0.0, 0.0, W, H])
        return {"person": person, "n_person": torch.full((F,), 1 if W == 64 else 2, dtype=torch.int32)}


class StubWholebody:
    def __init__(self, calls):
        self.calls = calls

    def __call__(self, fr):
        self.calls.n["kp"] += 1
        m = fr.float().mean(dim=(1, 2))                               # [F, 3]
        return m.repeat(1, 40)                                        # [F, 120]


class StubHmr:
    def __init__(self, calls):
        self.calls = calls

    def extract(self, crops):
        self.calls.n["hmr"] += 1
        n = crops.shape[0]
        m = crops.float().mean(dim=(1, 2))                            # per-channel means: RGB order shows
        return {"pose": m[:, :1].repeat(1, 207), "betas": m[:, 1:2].repeat(1, 10),
                "global_orient": m[:, 2:3].repeat(1, 9), "vit": torch.cat([m, crops[:, 0, 0, :].float()], 1)}


def stub_crop(fr, boxes, idx):
    return fr[torch.as_tensor(np.asarray(idx, np.int64))]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN / "jpeg_golden.npz"))


def write_video(root, action, video, blobs):
    d = root / action / video
    d.mkdir(parents=True, exist_ok=True)
    for i, b in enumerate(blobs):
        (d / f"frame_{i:06d}.jpg").write_bytes(b)


def make_tree(gold, root):
    b = [gold[f"jpeg/{n}"].tobytes() for n in gold["batch_names"]]
    small = [gold[f"jpeg/16x16_{e}_smooth"].tobytes() for e in ("420", "420rst", "420opt")]
    write_video(root, "Archery", "v_a_01", b[:4])
    write_video(root, "Archery", "v_a_02", [b[0], gold["bad/truncated"].tobytes()] + b[1:])
    (root / "Bowling" / "v_b_empty").mkdir(parents=True)
    write_video(root, "Bowling", "v_b_02", b[1:5])
    write_video(root, "Curling", "v_c_multi", small)
    write_video(root, "Curling", "v_c_02", b[2:5])
    return b


def run(tmp_path, calls, **kw):
    from vge.extract import extract_frame_tree
    return extract_frame_tree(StubHmr(calls), StubWholebody(calls), kw.pop("detector", None) or StubDetector(calls),
                              tmp_path / "frames", tmp_path / "meshes", tmp_path / "kps", tmp_path / "logs",
                              device="cpu", crop=stub_crop, **kw)


def outputs(tmp_path):
    return {str(p.relative_to(tmp_path)): p.read_bytes()
            for sub in ("meshes", "kps") for p in sorted((tmp_path / sub).rglob("*")) if p.is_file()}


def test_tree_bookkeeping_resume_and_retry(gold, tmp_path):
    b = make_tree(gold, tmp_path / "frames")
    rgb = [gold[f"rgb/{n}"] for n in gold["batch_names"]]
    calls = Calls()
    s1 = run(tmp_path, calls)
    assert s1 == {"Archery": {"single": ["v_a_01", "v_a_02"], "not_single": [], "errors": [], "skipped": []},
                  "Bowling": {"single": ["v_b_02"], "not_single": [], "errors": ["v_b_empty"], "skipped": []},
                  "Curling": {"single": ["v_c_02"], "not_single": ["v_c_multi"], "errors": [], "skipped": []}}
    logs = tmp_path / "logs"
    assert json.loads((logs / "single" / "Archery.json").read_text()) == ["v_a_01", "v_a_02"]
    assert json.loads((logs / "not_single" / "Curling.json").read_text()) == ["v_c_multi"]
    err = json.loads((logs / "errors" / "Bowling.json").read_text())
    assert list(err) == ["v_b_empty"] and "no frames" in err["v_b_empty"]
    assert not (logs / "errors" / "Archery.json").exists()
    # the truncated frame is dropped and frame_idx shows the gap; rows follow the decoded pixels, RGB order
    z = np.load(tmp_path / "meshes" / "Archery" / "v_a_02.npz")
    np.testing.assert_array_equal(z["frame_idx"], [0, 2, 3, 4, 5])
    want = np.stack([rgb[i].astype(np.float32).mean(axis=(0, 1)) for i in range(5)])
    np.testing.assert_allclose(z["vit"][:, :3], want, rtol=1e-6)
    np.testing.assert_array_equal(z["vit"][:, 3:], np.stack([rgb[i][0, 0] for i in range(5)]).astype(np.float32))
    assert z["pose"].shape == (5, 23, 3, 3) and z["global_orient"].shape == (5, 1, 3, 3) and z["betas"].shape == (5, 10)
    meta = json.loads(str(z["meta"]))
    assert meta == {"action": "Archery", "video": "v_a_02",
                    "source_path": str(tmp_path / "frames" / "Archery" / "v_a_02")}
    kp = np.load(tmp_path / "kps" / "Archery" / "v_a_02" / "keypoints.npy")
    assert kp.shape == (5, 120) and kp.dtype == np.float32
    # the rejected video has keypoints (process_video.py writes them for every video) and no npz
    assert (tmp_path / "kps" / "Curling" / "v_c_multi" / "keypoints.npy").exists()
    assert not (tmp_path / "meshes" / "Curling" / "v_c_multi.npz").exists()
    assert not (tmp_path / "meshes" / "Bowling" / "v_b_empty.npz").exists()
    # two same-size videos of an action share one pass
    assert calls.n["detect"] == 4 and calls.n["hmr"] == 3     # Archery 1, Bowling 1, Curling 2 (two sizes) / multi: no hmr

    # second run: nothing finished runs again; the error video is retried (and fails again before any model call)
    before, n1 = outputs(tmp_path), dict(calls.n)
    s2 = run(tmp_path, calls)
    assert calls.n == n1
    assert s2["Archery"] == {"single": [], "not_single": [], "errors": [], "skipped": ["v_a_01", "v_a_02"]}
    assert s2["Bowling"]["errors"] == ["v_b_empty"] and s2["Bowling"]["skipped"] == ["v_b_02"]
    assert s2["Curling"]["skipped"] == ["v_c_02", "v_c_multi"]
    assert outputs(tmp_path) == before

    # third run, after the empty folder got its frames: only that video runs, and it leaves the error list
    write_video(tmp_path / "frames", "Bowling", "v_b_empty", b[:3])
    s3 = run(tmp_path, calls, actions="Bowling")
    assert s3 == {"Bowling": {"single": ["v_b_empty"], "not_single": [], "errors": [], "skipped": ["v_b_02"]}}
    assert calls.n == {k: v + 1 for k, v in n1.items()}
    assert json.loads((logs / "errors" / "Bowling.json").read_text()) == {}
    assert json.loads((logs / "single" / "Bowling.json").read_text()) == ["v_b_02", "v_b_empty"]
    after = outputs(tmp_path)
    assert {k: v for k, v in after.items() if "v_b_empty" not in k} == before


def test_one_failing_video_does_not_lose_its_pass(gold, tmp_path):
    b = [gold[f"jpeg/{n}"].tobytes() for n in gold["batch_names"]]
    root = tmp_path / "frames"
    write_video(root, "Diving", "v_d_01", b[:3])
    write_video(root, "Diving", "v_d_02", [b[4]] * 3)           # poisoned
    write_video(root, "Diving", "v_d_03", b[1:4])
    (root / "Diving" / "v_d_04").mkdir()
    (root / "Diving" / "v_d_04" / "frame_000000.jpg").write_bytes(gold["bad/truncated"].tobytes())
    calls = Calls()
    det = StubDetector(calls, poison=torch.from_numpy(gold["rgb/batch_4"]))
    s = run(tmp_path, calls, detector=det)
    assert s["Diving"] == {"single": ["v_d_01", "v_d_03"], "not_single": [], "errors": ["v_d_04", "v_d_02"],
                           "skipped": []}
    err = json.loads((tmp_path / "logs" / "errors" / "Diving.json").read_text())
    assert "boom" in err["v_d_02"] and "could be decoded" in err["v_d_04"]
    assert (tmp_path / "meshes" / "Diving" / "v_d_03.npz").exists()


def test_existing_keypoints_are_not_recomputed(gold, tmp_path):
    b = [gold[f"jpeg/{n}"].tobytes() for n in gold["batch_names"]]
    write_video(tmp_path / "frames", "Archery", "v_a_01", b[:3])
    kp = tmp_path / "kps" / "Archery" / "v_a_01" / "keypoints.npy"
    kp.parent.mkdir(parents=True)
    np.save(kp, np.full((3, 120), 7, np.float32))
    calls = Calls()
    run(tmp_path, calls)
    assert calls.n == {"detect": 1, "kp": 0, "hmr": 1}
    assert (np.load(kp) == 7).all()


def test_unknown_action_is_an_error(gold, tmp_path):
    make_tree(gold, tmp_path / "frames")
    with pytest.raises(ValueError, match="not found"):
        run(tmp_path, Calls(), actions="Nope")


def test_extract_videos_packing_is_unchanged():
    """The factored packing rule: consecutive videos, at most max_frames per pass, a longer video alone."""
    from vge.extract import _pack_passes
    items = [("a", None, 5), ("b", None, 4), ("c", None, 12), ("d", None, 3), ("e", None, 7), ("f", None, 1)]
    assert [[k for k, _, _ in g] for g in _pack_passes(items, 10)] == [["a", "b"], ["c"], ["d", "e"], ["f"]]


def test_cli_asks_for_checkpoints(tmp_path, capsys):
    """python -m vge.extract: the reference's --action flag plus the roots and the checkpoint paths; without weights
    (and without --synthetic-weights) it stops at the argument parser, before touching a device."""
    from vge.extract import main
    with pytest.raises(SystemExit) as e:
        main(["--frames-root", str(tmp_path), "--mesh-root", str(tmp_path / "m"), "--kp-root", str(tmp_path / "k"),
              "--log-root", str(tmp_path / "l"), "--action", "Archery"])
    assert e.value.code == 2 and "--hmr-ckpt is required" in capsys.readouterr().err
