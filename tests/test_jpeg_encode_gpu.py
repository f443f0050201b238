"""The JPEG forward kernel (csrc/vge_jpeg_enc.hip) and the on-device round trip against the committed Pillow fixture
(tests/golden/make_jpeg_enc_golden.py) and the host path: exact equality everywhere.  No Pillow needed."""
import numpy as np
import pytest
import torch

from tests import jpeg_enc_cases as JC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return JC.load_gold()


@pytest.fixture(scope="module")
def files(gold, tmp_path_factory):
    return JC.write_files(gold, tmp_path_factory.mktemp("jpeg_enc_gpu"))


def src_tensor(gold, case):
    return torch.from_numpy(gold[f"src/{JC.parts(case)[0]}"])[None]


def device_forward(frames, quality, sub):
    """int16 [F, blocks, 64] from the kernel, as a host array."""
    from vge.frames import _forward
    lay, coef, _ = _forward(frames.to(DEV).contiguous(), quality, sub)
    assert coef.device.type == "cuda" and tuple(coef.shape) == (frames.shape[0], lay.blocks_per_frame, 64)
    return coef.cpu().numpy()


def test_device_forward_equals_host_and_pillow_on_every_case(gold, files):
    """Every block, dummy blocks included, in the three samplings: one-tile sizes with the vertical edge rule (5x6, 16x12,
    32x44), dummy luma column (8x14) and row (16x6), odd and narrow planes, widths on the dword path (8, 16, 32, 64, 260)
    and on the byte path, and 3 x 3 / 2 x 3 tiles with both frame edges ragged inside a tile."""
    for case in JC.all_cases(gold):
        image, sub, q = JC.parts(case)
        img = gold[f"src/{image}"]
        lay = JC.layout_for(img, sub)
        got = device_forward(torch.from_numpy(img)[None], q, sub)[0]
        host = JC.host_forward(img[None], lay, q)[0]
        pillow, _ = JC.pillow_coefficients(files[case], lay)
        assert np.array_equal(got, host), (case, np.argwhere(got != host)[:4].tolist())
        assert np.array_equal(got, pillow), case


def test_batch_in_one_call(gold, files):
    names = list(gold["batch_names"])
    img = np.stack([gold[f"src/{JC.parts(n)[0]}"] for n in names])
    lay = JC.layout_for(img[0], "420")
    got = device_forward(torch.from_numpy(img), 95, "420")
    assert np.array_equal(got, JC.host_forward(img, lay, 95))
    for i, n in enumerate(names):
        assert np.array_equal(got[i], JC.pillow_coefficients(files[n], lay)[0]), n


def test_roundtrip_on_the_device_equals_pillows_decode(gold):
    from vge.frames import jpeg_roundtrip
    for case in list(gold["names"]) + list(gold["batch_names"]):
        _, sub, q = JC.parts(case)
        src = src_tensor(gold, case).to(DEV)
        rt = jpeg_roundtrip(src, quality=q, subsampling=sub)
        assert rt.device.type == "cuda" and rt.dtype == torch.uint8 and rt.shape == src.shape
        assert torch.equal(rt[0].cpu(), torch.from_numpy(gold[f"rgb/{case}"])), case


def test_roundtrip_of_several_tiles_equals_host_roundtrip(gold):
    from vge.frames import jpeg_roundtrip
    for case in gold["tile_names"]:
        _, sub, q = JC.parts(case)
        src = src_tensor(gold, case)
        out = torch.zeros_like(src, device=DEV)
        assert jpeg_roundtrip(src.to(DEV), quality=q, subsampling=sub, out=out) is out
        assert torch.equal(out.cpu(), jpeg_roundtrip(src, quality=q, subsampling=sub)), case


def test_save_frames_from_the_device_writes_pillows_bytes(gold, tmp_path):
    from vge.frames import jpeg_roundtrip, load_frames, save_frames
    for case in JC.all_cases(gold):
        _, sub, q = JC.parts(case)
        paths = save_frames(src_tensor(gold, case).to(DEV), tmp_path / case, quality=q, subsampling=sub)
        with open(paths[0], "rb") as f:
            assert f.read() == gold[f"jpeg/{case}"].tobytes(), case
    names = list(gold["batch_names"])
    fr = torch.cat([src_tensor(gold, n) for n in names]).to(DEV)
    paths = save_frames(fr, tmp_path / "video", threads=2)
    for p, n in zip(paths, names):
        with open(p, "rb") as f:
            assert f.read() == gold[f"jpeg/{n}"].tobytes(), n
    back, kept = load_frames(tmp_path / "video", device=DEV)
    assert kept.tolist() == [0, 1, 2, 3, 4] and torch.equal(back, jpeg_roundtrip(fr))


def test_non_default_stream_equals_default_stream(gold):
    from vge.frames import _forward, jpeg_roundtrip
    fr = torch.cat([src_tensor(gold, n) for n in gold["batch_names"]]).to(DEV)
    _, ref, _ = _forward(fr, 95, "420")
    ref_rt = jpeg_roundtrip(fr)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        _, coef, _ = _forward(fr, 95, "420")
        rt = jpeg_roundtrip(fr)
    s.synchronize()
    assert torch.equal(coef, ref) and torch.equal(rt, ref_rt)


def test_frame_in_a_batch_is_untouched_by_its_neighbours(gold):
    """Three different 260 x 140 frames (3 x 3 tiles each) in one launch: each equals its single-frame result."""
    from vge.frames import jpeg_roundtrip
    a = torch.from_numpy(gold["src/tile260x140"])
    g = torch.Generator().manual_seed(5)
    b = torch.randint(0, 256, a.shape, generator=g, dtype=torch.uint8)
    fr = torch.stack([a, b, a.flip(0, 1)])
    for sub in ("420", "422", "444"):
        got = device_forward(fr, 95, sub)
        rt = jpeg_roundtrip(fr.to(DEV), subsampling=sub).cpu()
        for i in range(3):
            assert np.array_equal(got[i], device_forward(fr[i:i + 1], 95, sub)[0]), (sub, i)
            assert torch.equal(rt[i], jpeg_roundtrip(fr[i:i + 1].to(DEV), subsampling=sub)[0].cpu()), (sub, i)
