"""The device entropy coder (csrc/vge_jpeg_huff.hip: vge_jpeg_entropy_plan / vge_jpeg_entropy_emit) and the Python layer
over it, against Pillow's bytes in the committed fixture, the host coder and the plain-Python restatement
(tests/jpeg_huff_ref.py): exact equality everywhere, tiny shapes."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import jpeg_enc_cases as JC
from tests import jpeg_entropy_cases as EC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xA5


@pytest.fixture(scope="module")
def gold():
    return JC.load_gold()


def src_tensor(gold, case):
    return torch.from_numpy(gold[f"src/{JC.parts(case)[0]}"])[None]


def file_bytes(data, offsets, i):
    return data[int(offsets[i]):int(offsets[i + 1])].cpu().numpy().tobytes()


def device_code(coef, lay, quality=95, ws=None, gap=0, stream=None):
    """Raw ABI: int16 [n, blocks, 64] uploaded, plan, offsets with `gap` canary bytes in front of, between and after the
    files, emit.  -> (sizes, status, [bytes per frame], the output buffer as a host array, offsets, the workspace)."""
    from vge import lib as L
    from vge.frames import quant_tables
    so = L.load()
    n = int(coef.shape[0])
    coef_d = torch.from_numpy(np.ascontiguousarray(coef, np.int16)).to(DEV)
    q_d = torch.from_numpy(quant_tables(quality).view(np.int16)).to(DEV)
    need = int(so.vge_jpeg_entropy_workspace_bytes(C.byref(lay), n))
    assert need > 0
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert ws.numel() >= need
    sizes_d = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    st_d = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream(DEV).cuda_stream if stream is None else stream.cuda_stream
    assert so.vge_jpeg_entropy_plan(coef_d.data_ptr(), C.byref(lay), n, ws.data_ptr(), sizes_d.data_ptr(),
                                    st_d.data_ptr(), s) == 0
    if stream is not None:
        stream.synchronize()
    sizes, st = sizes_d.cpu().numpy(), st_d.cpu().numpy()
    offsets = (gap + np.concatenate([[0], np.cumsum(sizes + gap)[:-1]])).astype(np.int64)
    total = int(offsets[-1] + sizes[-1] + gap)
    out_d = torch.full((total,), CANARY, dtype=torch.uint8, device=DEV)
    off_d = torch.from_numpy(offsets).to(DEV)
    torch.cuda.synchronize()
    assert so.vge_jpeg_entropy_emit(ws.data_ptr(), q_d.data_ptr(), C.byref(lay), n, off_d.data_ptr(), out_d.data_ptr(),
                                    total, s) == 0
    torch.cuda.synchronize()
    out = out_d.cpu().numpy()
    files = [out[int(o):int(o) + int(z)].tobytes() for o, z in zip(offsets, sizes)]
    return sizes, st, files, out, offsets, ws


def assert_only_files_written(out, offsets, sizes):
    covered = np.zeros(out.size, bool)
    for o, z in zip(offsets, sizes):
        covered[int(o):int(o) + int(z)] = True
    assert (out[~covered] == CANARY).all()
    return int((~covered).sum())


def test_encode_frames_equals_pillow_on_every_case(gold):
    from vge.frames import encode_frames
    for case in JC.all_cases(gold):
        _, sub, q = JC.parts(case)
        data, offsets = encode_frames(src_tensor(gold, case).to(DEV), q, sub)
        assert data.device.type == "cpu" and data.dtype == torch.uint8 and offsets.tolist() == [0, data.numel()]
        assert data.numpy().tobytes() == gold[f"jpeg/{case}"].tobytes(), case
    names = list(gold["batch_names"])
    fr = torch.cat([src_tensor(gold, n) for n in names]).to(DEV)
    for entropy in (None, "device", "host"):
        data, offsets = encode_frames(fr, entropy=entropy)
        assert offsets.shape == (6,) and int(offsets[5]) == data.numel()
        for i, n in enumerate(names):
            assert file_bytes(data, offsets, i) == gold[f"jpeg/{n}"].tobytes(), (entropy, n)


def test_frame_in_a_batch_is_untouched_by_its_neighbours(gold):
    """Three different 260 x 140 frames in one call: each equals its single-frame result, in the three samplings."""
    from vge.frames import encode_frames
    a = torch.from_numpy(gold["src/tile260x140"])
    g = torch.Generator().manual_seed(5)
    b = torch.randint(0, 256, a.shape, generator=g, dtype=torch.uint8)
    fr = torch.stack([a, b, a.flip(0, 1)]).to(DEV)
    for sub in ("420", "422", "444"):
        data, offsets = encode_frames(fr, subsampling=sub)
        host, hoff = encode_frames(fr, subsampling=sub, entropy="host")
        assert torch.equal(offsets, hoff) and torch.equal(data, host), sub
        for i in range(3):
            one, _ = encode_frames(fr[i:i + 1], subsampling=sub)
            assert file_bytes(data, offsets, i) == one.numpy().tobytes(), (sub, i)


def test_synthetic_set_through_the_raw_abi_equals_the_host_coder():
    """Every synthetic frame equals vge_jpeg_entropy_encode_mem's bytes (and with it the restatement's: the host test
    pins those two together); sizes and status agree; no byte outside the files is written."""
    from vge import lib as L
    seg = L.load().vge_jpeg_entropy_segment_blocks()
    truth = EC.synthetic_truth()
    for name, shape, coef in EC.synthetic_set():
        lay = EC.layout(*shape)
        rc, hs, hst, hf = EC.encode_mem(coef[None], lay)
        sizes, st, files, out, offsets, _ = device_code(coef[None], lay, gap=37)
        assert sizes.tolist() == hs.tolist() and st.tolist() == hst.tolist() == [0], name
        assert files[0] == hf[0] == truth[name], name
        assert assert_only_files_written(out, offsets, sizes) == 74
    # the large frame spans several of the kernel's per-frame work segments, the last one partial
    blocks = EC.layout(520, 280, "444").blocks_per_frame
    assert blocks >= 3 * seg and blocks % seg != 0


@pytest.mark.parametrize("kind", ["ac", "dc"])
def test_refused_middle_frame_leaves_its_neighbours_alone(kind):
    lay, coef = EC.refusal_batch(kind)
    rc, hs, hst, hf = EC.encode_mem(coef, lay)
    sizes, st, files, out, offsets, _ = device_code(coef, lay, gap=16)
    assert st.tolist() == hst.tolist() == [0, EC.ERR_ARG, 0] and sizes.tolist() == hs.tolist() and sizes[1] == 0
    assert files[0] == hf[0] and files[2] == hf[2]
    assert_only_files_written(out, offsets, sizes)


def test_workspace_reuse_gives_the_same_bytes():
    """The dense frame, then the all-zero frame of the same layout in the same workspace: plan clears what it ORs into."""
    cases = {name: (shape, coef) for name, shape, coef in EC.synthetic_set()}
    shape, dense = cases["dense"]
    lay = EC.layout(*shape)
    _, _, first, _, _, ws = device_code(dense[None], lay)
    assert first[0] == EC.synthetic_truth()["dense"]
    zero = np.zeros_like(dense)
    _, _, second, _, _, _ = device_code(zero[None], lay, ws=ws)
    assert second[0] == EC.encode_mem(zero[None], lay)[3][0]
    _, _, third, _, _, _ = device_code(dense[None], lay, ws=ws)
    assert third[0] == first[0]


def test_emit_never_writes_outside_out(gold):
    """Canaries between and after the files stay (device_code packs with gaps); a negative out_bytes is refused before
    any launch; the offsets live on the device, so a buffer too short for them cannot be refused by the host: the
    kernel leaves a file that does not lie inside out_bytes unwritten and touches nothing."""
    from vge import lib as L
    from vge.frames import quant_tables
    so = L.load()
    names = list(gold["batch_names"])[:3]
    img = np.stack([gold[f"src/{JC.parts(n)[0]}"] for n in names])
    lay = JC.layout_for(img[0], "420")
    coef = JC.host_forward(img, lay, 95)
    want = [gold[f"jpeg/{n}"].tobytes() for n in names]
    sizes, st, files, out, offsets, ws = device_code(coef, lay, gap=64)
    assert files == want and assert_only_files_written(out, offsets, sizes) == 4 * 64
    q_d = torch.from_numpy(quant_tables(95).view(np.int16)).to(DEV)
    off_d = torch.from_numpy(offsets).to(DEV)
    out_d = torch.full((out.size,), CANARY, dtype=torch.uint8, device=DEV)
    args = (ws.data_ptr(), q_d.data_ptr(), C.byref(lay), 3, off_d.data_ptr(), out_d.data_ptr())
    assert so.vge_jpeg_entropy_emit(*args, -1, None) == EC.ERR_ARG
    torch.cuda.synchronize()
    assert bool((out_d == CANARY).all())
    short = int(offsets[2]) + int(sizes[2]) - 1          # one byte short of the last file
    assert so.vge_jpeg_entropy_emit(*args, short, None) == 0
    torch.cuda.synchronize()
    got = out_d.cpu().numpy()
    assert [got[int(o):int(o) + int(z)].tobytes() for o, z in zip(offsets[:2], sizes[:2])] == want[:2]
    assert (got[int(offsets[1]) + int(sizes[1]):] == CANARY).all()


def test_non_default_stream_equals_default_stream(gold):
    from vge.frames import encode_frames
    fr = torch.cat([src_tensor(gold, n) for n in gold["batch_names"]]).to(DEV)
    ref, ref_off = encode_frames(fr)
    cases = {name: (shape, coef) for name, shape, coef in EC.synthetic_set()}
    shape, coef = cases["sparse_520x280"]
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        data, off = encode_frames(fr)
        _, _, files, _, _, _ = device_code(coef[None], EC.layout(*shape), stream=s)
    s.synchronize()
    assert torch.equal(data, ref) and torch.equal(off, ref_off)
    assert files[0] == EC.synthetic_truth()["sparse_520x280"]


def test_keep_on_device_returns_the_same_bytes_on_the_gpu(gold):
    from vge.frames import encode_frames
    fr = torch.cat([src_tensor(gold, n) for n in gold["batch_names"]]).to(DEV)
    host, off = encode_frames(fr)
    dev, doff = encode_frames(fr, keep_on_device=True)
    assert dev.device.type == "cuda" and dev.dtype == torch.uint8 and doff.device.type == "cpu"
    assert torch.equal(dev.cpu(), host) and torch.equal(doff, off)
    empty, eoff = encode_frames(fr[:0], keep_on_device=True)
    assert empty.device.type == "cuda" and empty.numel() == 0 and eoff.tolist() == [0]


def test_save_frames_device_path_writes_pillows_bytes(gold, tmp_path):
    from vge.frames import jpeg_roundtrip, load_frames, save_frames
    for case in JC.all_cases(gold):
        _, sub, q = JC.parts(case)
        paths = save_frames(src_tensor(gold, case).to(DEV), tmp_path / case, quality=q, subsampling=sub,
                            entropy="device")
        assert [p.rsplit("/", 1)[1] for p in paths] == ["frame_000000.jpg"]
        with open(paths[0], "rb") as f:
            assert f.read() == gold[f"jpeg/{case}"].tobytes(), case
    names = list(gold["batch_names"])
    fr = torch.cat([src_tensor(gold, n) for n in names]).to(DEV)
    paths = save_frames(fr, tmp_path / "video", threads=2, entropy="device")
    for p, n in zip(paths, names):
        with open(p, "rb") as f:
            assert f.read() == gold[f"jpeg/{n}"].tobytes(), n
    back, kept = load_frames(tmp_path / "video", device=DEV)
    assert kept.tolist() == [0, 1, 2, 3, 4] and torch.equal(back, jpeg_roundtrip(fr))


def test_extract_videos_codes_the_cache_of_gpu_frames_on_the_device(gold, tmp_path, monkeypatch):
    import vge.frames
    import vge.hmr
    from tests.test_jpeg_encode_host import Recorder
    from vge.extract import extract_videos
    frames = torch.cat([src_tensor(gold, n) for n in gold["batch_names"]]).to(DEV)
    seen = []
    real = vge.frames.save_frames
    monkeypatch.setattr(vge.frames, "save_frames", lambda *a, **k: (seen.append(k.get("entropy")), real(*a, **k))[1])

    class GpuRecorder(Recorder):
        def detect(self, fr):
            return {k: v.to(fr.device) for k, v in super().detect(fr).items()}

        def crop(self, fr, boxes, idx):
            return fr[torch.as_tensor(np.asarray(idx, np.int64), device=fr.device)]

    rec = GpuRecorder()
    monkeypatch.setattr(vge.hmr, "crop_persons", rec.crop)
    extract_videos(rec, rec, rec, [("v", frames)], tmp_path / "m", tmp_path / "k", frame_cache=tmp_path / "frames")
    assert seen == ["device"]
    for i, n in enumerate(gold["batch_names"]):
        with open(tmp_path / "frames" / "v" / f"frame_{i:06d}.jpg", "rb") as f:
            assert f.read() == gold[f"jpeg/{n}"].tobytes(), n
