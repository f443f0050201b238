"""JPEG encoding on the host (include/vge_frames.h, vge/frames.py): the quantisation tables, the plain-C++ forward
transform and the Huffman encoder reproduce Pillow / libjpeg-turbo (the encoder cv2.imwrite uses too) exactly on the
committed fixture (tests/golden/make_jpeg_enc_golden.py): every coefficient, every file byte, every round-tripped pixel.
Every comparison is equality; nothing here has a tolerance.  No GPU and no Pillow needed.

The device kernel quantises with an integer division, as the host does (vge_jpeg_math.h quantise), so there is no
reciprocal to check against `/`."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import jpeg_enc_cases as JC


@pytest.fixture(scope="module")
def gold():
    return JC.load_gold()


@pytest.fixture(scope="module")
def files(gold, tmp_path_factory):
    return JC.write_files(gold, tmp_path_factory.mktemp("jpeg_enc"))


def src_tensor(gold, case):
    return torch.from_numpy(gold[f"src/{JC.parts(case)[0]}"])[None]


def test_quant_tables_equal_pillow_for_every_quality(gold):
    from vge.frames import quant_tables
    for q in range(1, 101):
        t = quant_tables(q)
        assert np.array_equal(t[0], gold["qtables"][q - 1, 0]), q
        assert np.array_equal(t[1], gold["qtables"][q - 1, 1]) and np.array_equal(t[2], t[1]), q
    assert np.array_equal(quant_tables(0), quant_tables(1)) and np.array_equal(quant_tables(101), quant_tables(100))


def test_host_forward_equals_pillow_coefficients(gold, files):
    """Every block of every case, dummy blocks included, in all three samplings: the coefficients our own entropy
    decoder reads out of Pillow's file.  The sizes are the smallest at which each rule can go wrong: 5x6, 16x12, 32x44
    (an even height that is no multiple of 16: padded chroma rows repeat the last DOWNSAMPLED row), 8x14 (right-hand
    dummy luma blocks), 16x6 (a whole dummy luma row), odd and narrow sizes, several kernel tiles."""
    from vge.frames import quant_tables
    for case in JC.all_cases(gold):
        image, sub, q = JC.parts(case)
        img = gold[f"src/{image}"]
        lay = JC.layout_for(img, sub)
        want, wq = JC.pillow_coefficients(files[case], lay)
        got = JC.host_forward(img[None], lay, q)[0]
        assert np.array_equal(wq, quant_tables(q)), case
        assert np.array_equal(got, want), (case, np.argwhere(got != want)[:4].tolist())


def test_fixture_has_the_dummy_block_cases(gold, files):
    """8x14 in 4:2:0 has a dummy luma column, 16x6 a whole dummy luma row (2 x 2 luma blocks for 1 x 2 and 2 x 1 real
    ones), and Pillow's files carry them as libjpeg makes them: all-zero AC, the DC of the previous block of the MCU."""
    for image, dummies in (("8x14_noise", {1: 0, 3: 2}), ("16x6_noise", {2: 1, 3: 1})):
        lay = JC.layout_for(gold[f"src/{image}"], "420")
        assert (lay.bw[0], lay.bh[0], lay.blocks_per_frame) == (2, 2, 6)
        coef, _ = JC.pillow_coefficients(files[f"{image}_420_q95"], lay)
        for blk, source in dummies.items():
            assert not coef[blk, 1:].any() and coef[blk, 0] == coef[source, 0], (image, blk)
        assert all(coef[b, 1:].any() for b in range(4) if b not in dummies), image


def test_save_frames_from_cpu_writes_pillows_bytes(gold, tmp_path):
    """Whole files, SOI to EOI: no header segment is excluded from the comparison."""
    from vge.frames import save_frames
    for case in JC.all_cases(gold):
        _, sub, q = JC.parts(case)
        paths = save_frames(src_tensor(gold, case), tmp_path / case, quality=q, subsampling=sub)
        assert [p.rsplit("/", 1)[1] for p in paths] == ["frame_000000.jpg"]
        with open(paths[0], "rb") as f:
            assert f.read() == gold[f"jpeg/{case}"].tobytes(), case


def test_save_frames_batch_numbering_and_listing(gold, tmp_path):
    from vge.frames import list_frames, save_frames
    names = list(gold["batch_names"])
    fr = torch.cat([src_tensor(gold, n) for n in names])
    paths = save_frames(fr, tmp_path / "v", start=7, threads=3)
    assert [p.rsplit("/", 1)[1] for p in paths] == [f"frame_{7 + i:06d}.jpg" for i in range(5)]
    assert list_frames(tmp_path / "v") == paths
    for p, n in zip(paths, names):
        with open(p, "rb") as f:
            assert f.read() == gold[f"jpeg/{n}"].tobytes(), n


def test_roundtrip_on_the_cpu_equals_pillows_decode(gold):
    from vge.frames import jpeg_roundtrip
    for case in list(gold["names"]) + list(gold["batch_names"]):
        _, sub, q = JC.parts(case)
        src = src_tensor(gold, case)
        keep = src.clone()
        rt = jpeg_roundtrip(src, quality=q, subsampling=sub)
        assert rt.shape == src.shape and rt.dtype == torch.uint8 and torch.equal(src, keep)
        assert torch.equal(rt[0], torch.from_numpy(gold[f"rgb/{case}"])), case


def test_roundtrip_defaults_and_out(gold):
    """The defaults are the reference's: quality 95, 4:2:0.  `out` receives the result."""
    from vge.frames import jpeg_roundtrip
    names = list(gold["batch_names"])
    fr = torch.cat([src_tensor(gold, n) for n in names])
    want = torch.stack([torch.from_numpy(gold[f"rgb/{n}"]) for n in names])
    assert torch.equal(jpeg_roundtrip(fr), want)
    out = torch.zeros_like(fr)
    assert jpeg_roundtrip(fr, out=out) is out and torch.equal(out, want)
    assert jpeg_roundtrip(fr[:0]).shape == (0, 48, 64, 3)
    with pytest.raises(ValueError):
        jpeg_roundtrip(fr, subsampling="411")
    with pytest.raises(ValueError):
        jpeg_roundtrip(fr.float())


def test_written_files_decode_through_load_frames(gold, tmp_path):
    from vge.frames import jpeg_roundtrip, load_frames, save_frames
    for case in ("37x53_noise_420_q95", "16x12_smooth_422_q95", "32x44_noise_444_q30", "tile150x131_420_q95"):
        _, sub, q = JC.parts(case)
        src = src_tensor(gold, case)
        save_frames(src, tmp_path / case, quality=q, subsampling=sub)
        fr, kept = load_frames(tmp_path / case, device="cpu")
        assert kept.tolist() == [0]
        assert torch.equal(fr, jpeg_roundtrip(src, quality=q, subsampling=sub)), case


def test_argument_errors(gold):
    from vge import lib as L
    from vge.frames import make_layout, quant_tables
    so = L.load()
    img = np.ascontiguousarray(gold["src/16x16_noise"])
    q = quant_tables(95)
    lay = make_layout(16, 16, 3, 2, 2)
    coef = np.zeros((lay.blocks_per_frame + 1) * 64, np.int16)
    base = coef.ctypes.data + (-coef.ctypes.data) % 16          # a 16-byte aligned address inside coef
    qa = np.zeros(192 + 8, np.uint16)
    qbase = qa.ctypes.data + (-qa.ctypes.data) % 16
    C.memmove(qbase, q.ctypes.data, 384)
    paths = (C.c_char_p * 1)(b"/nonexistent-dir/x.jpg")
    # grayscale layouts are not encoded
    gray = make_layout(16, 16, 1, 1, 1)
    assert so.vge_jpeg_forward(img.ctypes.data, C.byref(gray), 1, qbase, base, None) == 23
    assert so.vge_jpeg_forward_host(img.ctypes.data, C.byref(gray), 1, 1, q.ctypes.data, base) == 23
    assert so.vge_jpeg_entropy_encode(base, q.ctypes.data, C.byref(gray), 1, 1, paths, None, None) == 23
    assert b"3-component" in so.vge_last_error()
    # a layout struct that vge_jpeg_make_layout did not make
    foreign = make_layout(16, 16, 3, 2, 2)
    foreign.bw[0] += 1
    assert so.vge_jpeg_forward(img.ctypes.data, C.byref(foreign), 1, qbase, base, None) == 1
    assert so.vge_jpeg_forward_host(img.ctypes.data, C.byref(foreign), 1, 1, q.ctypes.data, base) == 1
    assert so.vge_jpeg_entropy_encode(base, q.ctypes.data, C.byref(foreign), 1, 1, paths, None, None) == 1
    # misaligned buffers (refused before anything is launched): coefficients, tables, and rgb where it is read as dwords
    assert so.vge_jpeg_forward(img.ctypes.data, C.byref(lay), 1, qbase, base + 2, None) == 1
    assert so.vge_jpeg_forward(img.ctypes.data, C.byref(lay), 1, qbase + 2, base, None) == 1
    assert so.vge_jpeg_forward(img.ctypes.data + 1, C.byref(lay), 1, qbase, base, None) == 1
    assert b"misaligned" in so.vge_last_error()
    # null buffers, a table entry outside 1..255
    assert so.vge_jpeg_forward(None, C.byref(lay), 1, qbase, base, None) == 1
    assert so.vge_jpeg_forward_host(img.ctypes.data, C.byref(lay), 1, 1, None, base) == 1
    bad = q.copy()
    bad[1, 5] = 0
    assert so.vge_jpeg_forward_host(img.ctypes.data, C.byref(lay), 1, 1, bad.ctypes.data, base) == 1
    assert so.vge_jpeg_quant_tables(95, None) == 1
    # nothing to do is not an error
    assert so.vge_jpeg_forward(None, C.byref(lay), 0, qbase, None, None) == 0


def test_one_unwritable_path_leaves_the_others_intact(gold, tmp_path):
    from vge import lib as L
    from vge.frames import quant_tables, save_frames
    names = list(gold["batch_names"])[:3]
    img = np.stack([gold[f"src/{JC.parts(n)[0]}"] for n in names])
    lay = JC.layout_for(img[0], "420")
    coef = JC.host_forward(img, lay, 95)
    good = [str(tmp_path / f"f{i}.jpg") for i in range(3)]
    blocked = tmp_path / "missing-folder" / "f1.jpg"
    paths = [good[0], str(blocked), good[2]]
    arr = (C.c_char_p * 3)(*[p.encode() for p in paths])
    sizes = np.full(3, -1, np.int64)
    st = np.full(3, -1, np.int32)
    q = quant_tables(95)
    rc = L.load().vge_jpeg_entropy_encode(coef.ctypes.data, q.ctypes.data, C.byref(lay), 3, 2, arr, sizes.ctypes.data,
                                          st.ctypes.data)
    assert rc == 7 and st.tolist() == [0, 7, 0]
    assert str(blocked).encode() in L.load().vge_last_error()
    assert not blocked.exists() and sizes[1] == 0
    for i in (0, 2):
        data = gold[f"jpeg/{names[i]}"].tobytes()
        with open(paths[i], "rb") as f:
            assert f.read() == data
        assert sizes[i] == len(data)
    # through save_frames: the failure is reported by name
    (tmp_path / "v").mkdir()
    (tmp_path / "v" / "frame_000001.jpg").mkdir()            # a directory where frame 1's file should go
    with pytest.raises(L.VgeError, match="frame_000001.jpg"):
        save_frames(torch.from_numpy(img), tmp_path / "v")
    with open(tmp_path / "v" / "frame_000002.jpg", "rb") as f:
        assert f.read() == gold[f"jpeg/{names[2]}"].tobytes()


class Recorder:
    """Stub models in the manner of tests/test_extract_tree.py; they record the frame tensors they are given."""
    def __init__(self):
        self.detect_in, self.kp_in, self.crop_in = [], [], []

    def detect(self, fr):
        self.detect_in.append(fr)
        F, H, W = (int(v) for v in fr.shape[:3])
        person = torch.zeros(F, 1, 5)
        person[:, 0, :4] = torch.tensor([0.0, 0.0, W, H])
        return {"person": person, "n_person": torch.ones(F, dtype=torch.int32)}

    def __call__(self, fr):
        self.kp_in.append(fr)
        return fr.float().mean(dim=(1, 2)).repeat(1, 40)

    def crop(self, fr, boxes, idx):
        self.crop_in.append(fr)
        return fr[torch.as_tensor(np.asarray(idx, np.int64))]

    def extract(self, crops):
        m = crops.float().mean(dim=(1, 2))
        return {"pose": m[:, :1].repeat(1, 207), "betas": m[:, 1:2].repeat(1, 10),
                "global_orient": m[:, 2:3].repeat(1, 9), "vit": m}


def test_extract_videos_feeds_the_models_round_tripped_frames(gold, tmp_path, monkeypatch):
    import vge.hmr
    from vge.extract import extract_videos
    from vge.frames import jpeg_roundtrip
    frames = torch.cat([src_tensor(gold, n) for n in gold["batch_names"]])
    for quality in (None, 95, 30):
        rec = Recorder()
        monkeypatch.setattr(vge.hmr, "crop_persons", rec.crop)
        root = tmp_path / str(quality)
        out = extract_videos(rec, rec, rec, [("v0", frames)], root / "m", root / "k", jpeg_quality=quality)
        assert out["v0"] is not None
        seen = rec.detect_in + rec.kp_in + rec.crop_in
        assert len(seen) == 3
        if quality is None:
            assert all(s is frames for s in seen)               # the input tensor itself: today's behaviour
        else:
            want = jpeg_roundtrip(frames, quality=quality)
            assert not torch.equal(want, frames)
            assert all(torch.equal(s, want) for s in seen)
    # two videos in one pass: each is round-tripped, the pass sees them stacked
    rec = Recorder()
    monkeypatch.setattr(vge.hmr, "crop_persons", rec.crop)
    extract_videos(rec, rec, rec, [("a", frames[:2]), ("b", frames[2:])], tmp_path / "m2", tmp_path / "k2",
                   jpeg_quality=95)
    assert torch.equal(rec.detect_in[0], jpeg_roundtrip(frames)) and torch.equal(rec.kp_in[0], rec.detect_in[0])


def test_forward_kernel_has_no_scratch_and_no_flat_access():
    """The forward kernel as built: no scratch, no FLAT memory instructions (tools/isa_guard.py, as
    tests/test_jpeg_host.py reads the reconstruct kernel)."""
    import os
    import shutil
    import sys
    from tests.conftest import REPO
    lib = os.path.join(REPO, "video-gen-evals_amd", "vge", "libvge.so")
    if not shutil.which("objcopy") or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("objcopy / ROCm llvm-objdump not available")
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa_guard
    hits = {k: v for k, v in isa_guard.kernels(lib).items() if "jpeg_forward_kernel" in k}
    assert hits
    for name, r in hits.items():
        assert r["flat"] == 0, f"{name}: {r['flat']} FLAT memory instructions"
        assert r["scratch"] == 0 and r["scratch_ops"] == 0, f"{name}: {r['scratch']} B/lane scratch"
