"""The host entropy decoder for files held in memory (vge_jpeg_probe_mem / vge_jpeg_entropy_decode_mem) against the
path decoder, and decode_frames on CPU tensors: exact equality.  Reads the three JPEG fixtures (no Pillow needed)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import jpeg_dehuff_cases as DC
from tests import jpeg_enc_cases as JC


@pytest.fixture(scope="module")
def files():
    return DC.all_files()


@pytest.fixture(scope="module")
def paths(files, tmp_path_factory):
    root = tmp_path_factory.mktemp("jpeg_dehuff_host")
    out = {}
    for name, blob in files.items():
        p = root / f"{name}.jpg"
        p.write_bytes(blob)
        out[name] = str(p)
    return out


def test_memory_probe_equals_the_path_probe(files, paths):
    from vge.frames import probe, probe_mem
    names = list(files)
    data, off, size = DC.pack([files[n] for n in names], gap=3, order=reversed(range(len(names))))
    assert np.array_equal(probe_mem(data, off, size, 2), probe([paths[n] for n in names], 2))


def test_files_are_read_into_one_buffer(files, paths, tmp_path):
    from vge import lib as L
    from vge.frames import _read_files
    names = ["batch_0", "truncated", "1x1_gray_noise"]
    empty = tmp_path / "empty.jpg"
    empty.write_bytes(b"")
    listed = [paths[names[0]], str(tmp_path / "missing.jpg"), paths[names[1]], str(empty), paths[names[2]]]
    buf, off, size = _read_files(listed, 2, pin=False)
    assert size.tolist() == [len(files[names[0]]), 0, len(files[names[1]]), 0, len(files[names[2]])]
    assert off.tolist() == np.concatenate([[0], np.cumsum(size)[:-1]]).tolist() and buf.numel() == size.sum()
    for i, n in zip((0, 2, 4), names):
        assert buf[off[i]:off[i] + size[i]].numpy().tobytes() == files[n]
    # a file that has become shorter than its recorded size: zero bytes and its own status, the neighbours intact
    so = L.load()
    arr = (C.c_char_p * 2)(listed[4].encode(), listed[0].encode())
    want = np.array([size[4] + 9, size[0]], np.int64)
    at = np.array([0, size[4] + 9], np.int64)
    out = np.full(int(want.sum()) + 3, DC.CANARY, np.uint8)
    st = np.full(2, -1, np.int32)
    assert so.vge_jpeg_read_files(arr, 2, 2, at.ctypes.data, want.ctypes.data, out.ctypes.data, out.size - 3,
                                  st.ctypes.data) == DC.ERR_IO
    assert st.tolist() == [DC.ERR_IO, 0] and not out[:at[1]].any() and (out[-3:] == DC.CANARY).all()
    assert out[at[1]:at[1] + want[1]].tobytes() == files[names[0]]
    want[1] += 1   # past the buffer: refused, nothing written
    assert so.vge_jpeg_read_files(arr, 2, 2, at.ctypes.data, want.ctypes.data, out.ctypes.data, out.size - 3,
                                  st.ctypes.data) == DC.ERR_IO and st.tolist() == [DC.ERR_IO, DC.ERR_ARG]


def test_memory_decoder_equals_the_path_decoder_on_every_fixture_file(files, paths):
    from vge.frames import make_layout
    seen = set()
    for name, blob in files.items():
        row = DC.probe_one(blob)
        # an unsupported file has no layout of its own: it is decoded against a small one and must keep its status
        lay = make_layout(*[int(x) for x in row[:5]]) if int(row[5]) == 0 else make_layout(16, 16, 3, 2, 2)
        a = DC.host_decode_files([blob], lay)
        b = DC.host_decode_paths([paths[name]], lay)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]), name
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), name
        seen.add(int(a[1][0]))
    assert seen == {0, DC.ERR_IO, DC.ERR_PROGRESSIVE}


def test_packing_with_gaps_in_any_order_and_a_frame_between_failed_frames(files):
    gold_names = ["batch_0", "truncated", "batch_1", "16x16_420_smooth", "batch_2"]
    blobs = [files[n] for n in gold_names]
    lay = DC.layout_of(blobs[0])
    data, off, size = DC.pack(blobs, gap=5, order=[4, 2, 0, 3, 1])
    assert (np.diff(off) < 0).any()
    before = data.copy()
    rc, st, coef, qtab = DC.host_decode_mem(data, off, size, lay)
    assert rc == DC.ERR_IO and st.tolist() == [0, DC.ERR_IO, 0, DC.ERR_SHAPE, 0]
    assert np.array_equal(data, before)
    from vge import lib as L
    assert b"file 1" in L.load().vge_last_error()   # the first failing frame is named
    for i, blob in enumerate(blobs):
        _, s1, c1, q1 = DC.host_decode_files([blob], lay)
        assert s1[0] == st[i] and np.array_equal(c1[0], coef[i]) and np.array_equal(q1[0], qtab[i]), i
    assert not coef[1].any() and (qtab[1] == 1).all() and not coef[3].any() and (qtab[3] == 1).all()


def test_argument_refusals(files):
    from vge import lib as L
    so = L.load()
    blob = files["batch_0"]
    lay = DC.layout_of(blob)
    data, off, size = DC.pack([blob, blob, blob])
    # a negative size and a size past the buffer: ERR_ARG for that file alone, nothing of it is read
    bad = size.copy()
    bad[0], bad[2] = -1, size[2] + 1
    rc, st, coef, qtab = DC.host_decode_mem(data, off, bad, lay)
    assert rc == DC.ERR_ARG and st.tolist() == [DC.ERR_ARG, 0, DC.ERR_ARG]
    assert not coef[0].any() and (qtab[0] == 1).all() and coef[1].any() and not coef[2].any()
    neg = off.copy()
    neg[1] = -4
    assert DC.host_decode_mem(data, neg, size, lay)[1].tolist() == [0, DC.ERR_ARG, 0]
    # the buffer's length is the caller's word: a file is outside a shorter one
    assert DC.host_decode_mem(data, off, size, lay, data_bytes=int(off[2]) + 10)[1].tolist() == [0, 0, DC.ERR_ARG]
    # an empty file is what an unreadable path is
    zero = size.copy()
    zero[1] = 0
    assert DC.host_decode_mem(data, off, zero, lay)[1].tolist() == [0, DC.ERR_IO, 0]
    # n = 0 is fine and touches nothing; a negative count, a negative length and null buffers are refused
    assert so.vge_jpeg_entropy_decode_mem(None, 0, None, None, 0, 1, C.byref(lay), None, None, None) == 0
    assert so.vge_jpeg_probe_mem(None, 0, None, None, 0, 1, None) == 0
    assert so.vge_jpeg_entropy_decode_mem(data.ctypes.data, data.size, off.ctypes.data, size.ctypes.data, -1, 1,
                                          C.byref(lay), None, None, None) == DC.ERR_ARG
    assert b"vge_jpeg_entropy_decode_mem" in so.vge_last_error()
    assert so.vge_jpeg_entropy_decode_mem(data.ctypes.data, -1, off.ctypes.data, size.ctypes.data, 1, 1,
                                          C.byref(lay), None, None, None) == DC.ERR_ARG
    assert so.vge_jpeg_probe_mem(None, 8, None, None, 1, 1, None) == DC.ERR_ARG
    info = (L.JpegInfo * 3)()
    assert so.vge_jpeg_probe_mem(data.ctypes.data, data.size, off.ctypes.data, bad.ctypes.data, 3, 1,
                                 info) == DC.ERR_ARG
    assert [i.status for i in info] == [DC.ERR_ARG, 0, DC.ERR_ARG]


def test_corrupt_streams_have_the_expected_host_verdicts(files):
    """What the device tests compare against: the cut files, the broken restart sequences and the seeded bit flips."""
    blob = files["37x53_420_noise"]
    lay = DC.layout_of(blob)
    cut = DC.cuts(blob)
    st = DC.host_decode_files(list(cut.values()), lay)[1]
    verdict = dict(zip(cut, st.tolist()))
    assert verdict["header"] == verdict["scan0"] == verdict["scan1"] == verdict["ff_00"] == DC.ERR_IO
    assert verdict["last_scan_byte"] == DC.ERR_IO
    assert verdict["before_eoi"] == 0 and verdict["half_eoi"] == 0   # the end of the file ends the segment too
    rst = files["rst1_80x48_420"]
    assert len(DC.restart_markers(rst)) == 14 and rst[DC.restart_markers(rst)[8] + 1] == 0xD0   # the index wraps
    lay = DC.layout_of(rst)
    assert DC.host_decode_files([rst, DC.wrong_marker_index(rst), DC.removed_marker(rst)], lay)[1].tolist() == \
        [0, DC.ERR_IO, DC.ERR_IO]
    st = DC.flip_set_verdicts()
    assert (st == 0).any() and (st == DC.ERR_IO).any() and set(st.tolist()) <= {0, DC.ERR_IO}


def test_decode_frames_on_cpu_tensors_equals_load_frames(files, paths):
    from vge.frames import decode_frames, load_frames
    names = ["batch_0", "truncated", "batch_1", "16x16_420_smooth", "batch_2", "batch_3"]
    data, off, size = DC.pack([files[n] for n in names])
    offsets = np.concatenate([off, [data.size]])
    fr, kept = decode_frames(torch.from_numpy(data), torch.from_numpy(offsets), device="cpu")
    ref, rkept = load_frames([paths[n] for n in names], device="cpu")
    assert kept.tolist() == rkept.tolist() == [0, 2, 4, 5]
    assert fr.device.type == "cpu" and torch.equal(fr, ref)
    empty, ek = decode_frames(torch.zeros(0, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), device="cpu")
    assert tuple(empty.shape) == (0, 0, 0, 3) and ek.size == 0
    bad = torch.from_numpy(np.frombuffer(files["truncated"], np.uint8).copy())
    none, nk = decode_frames(bad, np.array([0, bad.numel()]), device="cpu")
    assert tuple(none.shape) == (0,) + tuple(ref.shape[1:]) and nk.size == 0


def test_decode_frames_refuses_what_load_frames_refuses(files):
    from vge.frames import UnsupportedJpegError, decode_frames
    blob = np.frombuffer(files["batch_0"] + files["progressive"], np.uint8).copy()
    off = np.array([0, len(files["batch_0"]), blob.size])
    with pytest.raises(UnsupportedJpegError, match="progressive"):
        decode_frames(torch.from_numpy(blob), off, device="cpu")
    with pytest.raises(ValueError):
        decode_frames(torch.from_numpy(blob), np.array([0, blob.size + 1]), device="cpu")
    with pytest.raises(ValueError):
        decode_frames(torch.from_numpy(blob), off, device="cpu", entropy="device")


def test_decode_frames_inverts_encode_frames_on_the_host():
    from vge.frames import decode_frames, encode_frames, jpeg_roundtrip
    gold = JC.load_gold()
    fr = torch.cat([torch.from_numpy(gold[f"src/{JC.parts(n)[0]}"])[None] for n in gold["batch_names"]])
    data, offsets = encode_frames(fr, entropy="host")
    out, kept = decode_frames(data, offsets, device="cpu")
    assert kept.tolist() == [0, 1, 2, 3, 4] and torch.equal(out, jpeg_roundtrip(fr))
