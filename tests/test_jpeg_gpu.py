"""The JPEG reconstruct kernel (csrc/vge_jpeg.hip) against the committed Pillow fixture and the host path: exact
equality.  Reads tests/golden/jpeg_golden.npz only (no Pillow needed)."""
import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN / "jpeg_golden.npz"))


@pytest.fixture(scope="module")
def files(gold, tmp_path_factory):
    root = tmp_path_factory.mktemp("jpeg_gpu")
    out = {}
    for k, v in gold.items():
        if k.startswith("jpeg/") or k.startswith("bad/"):
            p = root / (k.replace("/", "_") + ".jpg")
            p.write_bytes(v.tobytes())
            out[k.split("/", 1)[1]] = str(p)
    return out


def test_device_reconstruct_equals_pillow_on_every_fixture(gold, files):
    """Every size / sampling / restart / table variant: one-tile images, widths that take the dword-store path
    (4, 8, 16, 64) and the byte-store path (1, 2, 3, 5, 17, 19, 37)."""
    from vge.frames import load_frames
    for name in list(gold["names"]) + list(gold["batch_names"]):
        fr, kept = load_frames([files[name]], device=DEV)
        assert kept.tolist() == [0], name
        assert fr.device.type == "cuda" and fr.dtype == torch.uint8
        assert torch.equal(fr[0].cpu(), torch.from_numpy(gold[f"rgb/{name}"])), name


def test_batch_equals_host_path(gold, files):
    from vge.frames import load_frames
    paths = [files[n] for n in gold["batch_names"]]
    dev, kd = load_frames(paths, device=DEV)
    host, kh = load_frames(paths, device="cpu")
    assert kd.tolist() == kh.tolist() == [0, 1, 2, 3, 4]
    assert torch.equal(dev.cpu(), host)


def test_several_tiles_equal_host_path(gold, files):
    """The 128 x 128 frames span two 128 x 64 tiles: the chroma halo across the tile boundary, frame edges included."""
    from vge.frames import load_frames
    paths = [files[n] for n in gold["tree_names"]]
    dev, _ = load_frames(paths, device=DEV)
    host, _ = load_frames(paths, device="cpu")
    assert tuple(dev.shape) == (12, 128, 128, 3)
    assert torch.equal(dev.cpu(), host)


def test_many_tiles_with_ragged_edges_equal_host_path(gold, files):
    """260 x 140 (3 x 3 tiles, dword stores) and 150 x 131 (2 x 3 tiles, byte stores) in every sampling: the frame edge
    falls inside the last tiles, the chroma halo crosses tile boundaries in both directions."""
    from vge.frames import load_frames
    for name in gold["tile_names"]:
        dev, kept = load_frames([files[name]], device=DEV)
        host, _ = load_frames([files[name]], device="cpu")
        assert kept.tolist() == [0] and dev.shape[1] in (140, 131), name
        assert torch.equal(dev.cpu(), host), name


def test_frame_beside_a_failed_frame_is_intact(gold, files):
    from vge.frames import load_frames
    names = list(gold["batch_names"])
    paths = [files[names[0]], files["truncated"], files[names[1]], files["16x16_420_smooth"], files[names[2]]]
    fr, kept = load_frames(paths, device=DEV)
    assert kept.tolist() == [0, 2, 4]
    for j, n in enumerate(names[:3]):
        assert torch.equal(fr[j].cpu(), torch.from_numpy(gold[f"rgb/{n}"])), n


def test_non_default_stream_equals_default_stream(gold, files):
    from vge.frames import load_frames
    paths = [files[n] for n in gold["batch_names"]]
    ref, _ = load_frames(paths, device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        fr, _ = load_frames(paths, device=DEV)
    s.synchronize()
    assert torch.equal(fr, ref)


def test_progressive_raises_on_the_device_path(files):
    from vge.frames import UnsupportedJpegError, load_frames
    with pytest.raises(UnsupportedJpegError, match="progressive"):
        load_frames([files["progressive"]], device=DEV)
