"""The in-memory host entropy coder (vge_jpeg_entropy_encode_mem), the file writer (vge_jpeg_write_files) and the
Python layer over them (encode_frames, save_frames(entropy=...), extract_videos(frame_cache=...)), on the CPU.  Ground
truth: Pillow's bytes in the committed fixture (tests/golden/jpeg_enc_golden.npz) for real frames, and a plain-Python
restatement of baseline Huffman coding (tests/jpeg_huff_ref.py), itself pinned against Pillow here, for synthetic
coefficients.  Every comparison is equality."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import jpeg_enc_cases as JC
from tests import jpeg_entropy_cases as EC
from tests import jpeg_huff_ref as R
from tests.test_jpeg_encode_host import Recorder


@pytest.fixture(scope="module")
def gold():
    return JC.load_gold()


@pytest.fixture(scope="module")
def files(gold, tmp_path_factory):
    return JC.write_files(gold, tmp_path_factory.mktemp("jpeg_entropy"))


def src_tensor(gold, case):
    return torch.from_numpy(gold[f"src/{JC.parts(case)[0]}"])[None]


def test_encode_mem_equals_pillow_and_the_file_coder_on_every_case(gold, tmp_path):
    """Every fixture case: the bytes equal Pillow's, sizes-only mode gives the same sizes (EC.encode_mem asserts it), and
    vge_jpeg_entropy_encode writes the same bytes to disk."""
    from vge import lib as L
    from vge.frames import quant_tables
    for case in JC.all_cases(gold):
        image, sub, q = JC.parts(case)
        img = gold[f"src/{image}"]
        lay = JC.layout_for(img, sub)
        coef = JC.host_forward(img[None], lay, q)
        want = gold[f"jpeg/{case}"].tobytes()
        rc, sizes, st, got = EC.encode_mem(coef, lay, q)
        assert rc == 0 and st.tolist() == [0] and sizes.tolist() == [len(want)], case
        assert got[0] == want, case
        path = str(tmp_path / f"{case}.jpg")
        arr = (C.c_char_p * 1)(path.encode())
        assert L.load().vge_jpeg_entropy_encode(coef.ctypes.data, quant_tables(q).ctypes.data, C.byref(lay), 1, 1, arr,
                                                None, None) == 0
        with open(path, "rb") as f:
            assert f.read() == got[0], case


def test_batch_at_caller_offsets_leaves_the_gaps_untouched(gold):
    names = list(gold["batch_names"])
    img = np.stack([gold[f"src/{JC.parts(n)[0]}"] for n in names])
    lay = JC.layout_for(img[0], "420")
    coef = JC.host_forward(img, lay, 95)
    want = [gold[f"jpeg/{n}"].tobytes() for n in names]
    offsets, o = [], 13
    for w in want:                     # gaps of 13, 7, 11, ... bytes in front of, between and after the files
        offsets.append(o)
        o += len(w) + 7 + 4 * len(offsets)
    out = np.full(o, 0xA5, np.uint8)
    rc, sizes, st, got = EC.encode_mem(coef, lay, 95, offsets=np.array(offsets, np.int64), out=out, threads=3)
    assert rc == 0 and got == want and sizes.tolist() == [len(w) for w in want]
    covered = np.zeros(o, bool)
    for off, w in zip(offsets, want):
        covered[off:off + len(w)] = True
    assert (out[~covered] == 0xA5).all() and (~covered).sum() > 40
    # a buffer that ends inside the last file: that file alone is refused
    short = np.full(offsets[-1] + 100, 0xA5, np.uint8)
    rc, sizes, st, got = EC.encode_mem(coef, lay, 95, offsets=np.array(offsets, np.int64), out=short)
    assert rc == EC.ERR_ARG and st.tolist() == [0, 0, 0, 0, EC.ERR_ARG] and got[:4] == want[:4]
    assert (short[offsets[-1]:] == 0xA5).all()


def test_restatement_reproduces_pillows_bytes(gold, files):
    """Pins the restatement itself: from the coefficients our decoder reads out of Pillow's file, it rebuilds the file."""
    for case in list(gold["names"]) + list(gold["batch_names"]):
        image, sub, _ = JC.parts(case)
        lay = JC.layout_for(gold[f"src/{image}"], sub)
        coef, q = JC.pillow_coefficients(files[case], lay)
        assert R.encode(coef, q, lay, EC.template(gold)) == gold[f"jpeg/{case}"].tobytes(), case


def test_synthetic_set_equals_the_restatement(gold):
    """An all-zero frame; every block holding only natural index 63; zero runs of exactly 15 and 16; the 1,658-bit block
    with DC steps of +-2040; dense uniform coefficients; 6,825 sparse blocks; a frame whose padded last scan byte is FF."""
    truth = EC.synthetic_truth()
    for name, shape, coef in EC.synthetic_set():
        rc, sizes, st, got = EC.encode_mem(coef[None], EC.layout(*shape))
        assert rc == 0 and st.tolist() == [0], name
        assert got[0] == truth[name], name
    assert truth["ff_tail"].endswith(b"\xff\x00\xff\xd9")
    assert EC.layout(520, 280, "444").blocks_per_frame == 6825
    assert EC.find_ff_tail_seed(gold, EC.FF_TAIL_SEED + 1) == EC.FF_TAIL_SEED


def test_cases_cover_every_branch_of_the_coder(gold, files):
    """Counted from the coefficients: ZRL blocks, blocks without EOB, AC of size 10, DC differences of size 11 and
    negative ones all occur in the fixture and the synthetic set together (the synthetic frames hold each by
    construction)."""
    total = dict(zrl=0, no_eob=0, ac10=0, dc11=0, dc_neg=0)
    for name, shape, coef in EC.synthetic_set():
        for k, v in R.stats(coef, EC.layout(*shape)).items():
            total[k] += int(v)
    for case in gold["names"]:
        image, sub, _ = JC.parts(case)
        lay = JC.layout_for(gold[f"src/{image}"], sub)
        for k, v in R.stats(JC.pillow_coefficients(files[case], lay)[0], lay).items():
            total[k] += int(v)
    assert all(v > 0 for v in total.values()), total


@pytest.mark.parametrize("kind", ["ac", "dc"])
def test_a_frame_beyond_baseline_coding_is_refused_alone(kind):
    lay, coef = EC.refusal_batch(kind)
    rc, sizes, st, got = EC.encode_mem(coef, lay)
    assert rc == EC.ERR_ARG and st.tolist() == [0, EC.ERR_ARG, 0] and sizes[1] == 0 and sizes[0] > 0 and sizes[2] > 0
    for i in (0, 2):
        alone = EC.encode_mem(coef[i:i + 1], lay)
        assert alone[0] == 0 and got[i] == alone[3][0]


def test_grayscale_layout_is_refused():
    from vge import lib as L
    from vge.frames import make_layout, quant_tables
    gray = make_layout(16, 16, 1, 1, 1)
    coef = np.zeros((1, gray.blocks_per_frame, 64), np.int16)
    sizes = np.zeros(1, np.int64)
    so = L.load()
    assert so.vge_jpeg_entropy_encode_mem(coef.ctypes.data, quant_tables(95).ctypes.data, C.byref(gray), 1, 1, None,
                                          None, 0, sizes.ctypes.data, None) == EC.ERR_COMPONENTS
    assert so.vge_jpeg_entropy_workspace_bytes(C.byref(gray), 1) == 0
    assert so.vge_jpeg_entropy_plan(None, C.byref(gray), 1, None, None, None, None) == EC.ERR_COMPONENTS
    assert so.vge_jpeg_entropy_emit(None, None, C.byref(gray), 1, None, None, 0, None) == EC.ERR_COMPONENTS


def test_write_files_writes_what_it_is_given(tmp_path):
    from vge import lib as L
    data = np.arange(256, dtype=np.uint8)
    offsets, sizes = np.array([3, 100, 40], np.int64), np.array([10, 156, 0], np.int64)
    blocked = tmp_path / "missing-folder" / "b.bin"
    paths = [str(tmp_path / "a.bin"), str(blocked), str(tmp_path / "c.bin")]
    arr = (C.c_char_p * 3)(*[p.encode() for p in paths])
    st = np.full(3, -1, np.int32)
    rc = L.load().vge_jpeg_write_files(data.ctypes.data, offsets.ctypes.data, sizes.ctypes.data, 3, 2, arr,
                                       st.ctypes.data)
    assert rc == EC.ERR_IO and st.tolist() == [0, EC.ERR_IO, 0] and not blocked.exists()
    assert str(blocked).encode() in L.load().vge_last_error()
    assert open(paths[0], "rb").read() == data[3:13].tobytes() and open(paths[2], "rb").read() == b""
    blocked.parent.mkdir()
    assert L.load().vge_jpeg_write_files(data.ctypes.data, offsets.ctypes.data, sizes.ctypes.data, 3, 0, arr,
                                         None) == 0
    assert open(paths[1], "rb").read() == data[100:].tobytes()


def test_encode_frames_on_cpu_tensors_equals_the_fixture(gold, tmp_path):
    from vge.frames import encode_frames, save_frames
    for case in JC.all_cases(gold):
        _, sub, q = JC.parts(case)
        data, offsets = encode_frames(src_tensor(gold, case), quality=q, subsampling=sub)
        assert data.dtype == torch.uint8 and data.device.type == "cpu" and offsets.dtype == torch.int64
        assert offsets.tolist() == [0, data.numel()]
        assert data.numpy().tobytes() == gold[f"jpeg/{case}"].tobytes(), case
    names = list(gold["batch_names"])
    fr = torch.cat([src_tensor(gold, n) for n in names])
    data, offsets = encode_frames(fr, entropy="host", threads=3)
    assert offsets.shape == (6,) and offsets[0] == 0 and offsets[5] == data.numel()
    for i, n in enumerate(names):
        assert data[offsets[i]:offsets[i + 1]].numpy().tobytes() == gold[f"jpeg/{n}"].tobytes(), n
    data, offsets = encode_frames(fr[:0])
    assert data.numel() == 0 and offsets.tolist() == [0]
    with pytest.raises(ValueError):
        encode_frames(fr, entropy="device")          # a CPU tensor has no device coder
    with pytest.raises(ValueError):
        encode_frames(fr, entropy="gpu")
    with pytest.raises(ValueError):
        save_frames(fr, tmp_path / "v", entropy="device")
    assert not (tmp_path / "v").exists()


def test_extract_videos_writes_the_frame_cache(gold, tmp_path, monkeypatch):
    import vge.hmr
    from vge.extract import extract_videos
    from vge.frames import list_frames, load_frames, jpeg_roundtrip, save_frames
    frames = torch.cat([src_tensor(gold, n) for n in gold["batch_names"]])
    for quality in (None, 30):
        rec = Recorder()
        monkeypatch.setattr(vge.hmr, "crop_persons", rec.crop)
        root = tmp_path / str(quality)
        videos = ((s, f) for s, f in [("a", frames[:2]), ("b", frames[2:])])    # an iterator, consumed once
        out = extract_videos(rec, rec, rec, videos, root / "m", root / "k", jpeg_quality=quality,
                             frame_cache=root / "frames")
        assert set(out) == {"a", "b"}
        q = 95 if quality is None else quality
        for stem, fr in (("a", frames[:2]), ("b", frames[2:])):
            want = save_frames(fr, root / "want" / stem, quality=q)
            got = list_frames(root / "frames" / stem)
            assert [p.rsplit("/", 1)[1] for p in got] == [p.rsplit("/", 1)[1] for p in want]
            for g, w in zip(got, want):
                assert open(g, "rb").read() == open(w, "rb").read()
            back, kept = load_frames(root / "frames" / stem, device="cpu")
            assert kept.tolist() == list(range(len(want))) and torch.equal(back, jpeg_roundtrip(fr, quality=q))
    # the default leaves no cache behind
    rec = Recorder()
    monkeypatch.setattr(vge.hmr, "crop_persons", rec.crop)
    extract_videos(rec, rec, rec, [("a", frames)], tmp_path / "m", tmp_path / "k")
    assert sorted(p.name for p in tmp_path.iterdir() if p.is_dir()) == ["30", "None", "k", "m"]
