"""The ingest calls over files held in memory (vge_ingest_probe_mem / _decode_mem / _plan_mem) and the shared deflate
code-length rules (vge_inflate_check_lengths) on the CPU: the `_mem` calls equal the path calls, the plan's descriptors
equal what np.load sees, the length rules equal zlib's verdicts, and files outside the buffer are refused unread."""
import ctypes as C
import io
import struct
import zlib

import numpy as np
import pytest

from tests import inflate_cases as IC

ERR_ARG, ERR_IO, ERR_SHAPE, ERR_KP = 1, 7, 8, 9


def _cstrs(strs):
    arr = (C.c_char_p * max(len(strs), 1))()
    arr[:len(strs)] = [None if s is None else s.encode() for s in strs]
    return arr


def path_calls(tmp_path, files, videos, vit_dim, F, Fk):
    """The same videos through vge_ingest_probe / vge_ingest_decode on files on disk."""
    from vge import lib as L
    lib = L.load()
    n = len(files)
    npz, kps = [], []
    for i, (z, k) in enumerate(files):
        (tmp_path / f"v{i}.npz").write_bytes(z)
        npz.append(str(tmp_path / f"v{i}.npz"))
        if k is not None:
            (tmp_path / f"k{i}.npy").write_bytes(k)
        kps.append(str(tmp_path / f"k{i}.npy"))   # a path that does not exist: no keypoints
    info = (L.ClipInfo * n)()
    rc_p = lib.vge_ingest_probe(_cstrs(npz), _cstrs(kps), n, 2, info)
    rows = [(info[i].n_frames, info[i].vit_dim, info[i].kp_frames, info[i].status) for i in range(n)]
    st = np.full(n, -77, np.int32)
    a = IC.empty_store(F, Fk, vit_dim)
    p = IC._ptr
    rc_d = lib.vge_ingest_decode(_cstrs(npz), _cstrs(kps), n, 2, p(videos), vit_dim, p(a["pose"]), p(a["gori"]),
                                 p(a["betas"]), p(a["vit"]), p(a["kp"]), p(st))
    return rc_p, rows, rc_d, st, a


def assert_mem_equals_paths(tmp_path, files, vit_dim, gap=0, order=None):
    data, off, size = IC.pack(files, gap=gap, order=order)
    rc_p, rows = IC.host_probe_mem(data, off, size)
    videos, F, Fk = IC.video_table(rows)
    rc_d, st, a = IC.host_decode_mem(data, off, size, videos, vit_dim, F, Fk)
    prc_p, prows, prc_d, pst, pa = path_calls(tmp_path, files, videos, vit_dim, F, Fk)
    assert (rc_p, rows, rc_d, st.tolist()) == (prc_p, prows, prc_d, pst.tolist())
    for k in a:
        assert IC.same_bits(a[k], pa[k]), k
    return rows, st, a, videos


def test_case_streams_have_their_properties():
    """inflate_cases asserts each stream's property while building it; this runs the builders in the CPU suite."""
    cases = IC.stream_cases()
    assert sum(not c.ok for c in cases.values()) >= 20 and sum(c.ok for c in cases.values()) >= 12
    assert len(IC.archive_cases()) == 9


def test_archive_cases_mem_equals_paths_and_numpy(tmp_path):
    for name, (z, k, vit_dim) in IC.archive_cases().items():
        ref = np.load(io.BytesIO(z))
        vit_dim = vit_dim or ref["vit"].shape[1]
        d = tmp_path / name
        d.mkdir()
        rows, st, a, videos = assert_mem_equals_paths(d, [(z, k)], vit_dim, gap=3)
        T = ref["pose"].shape[0]
        kT = -1 if k is None else np.load(io.BytesIO(k)).shape[0]
        assert rows == [(T, vit_dim, kT, 0)] and st.tolist() == [0], name
        assert np.array_equal(a["pose"], ref["pose"].reshape(T, 207).astype(np.float32)), name
        assert np.array_equal(a["vit"], ref["vit"].astype(np.float32)), name
        assert np.array_equal(a["gori"], ref["global_orient"].reshape(T, 9).astype(np.float32)), name
        assert np.array_equal(a["betas"], ref["betas"].astype(np.float32)), name
        if k is not None:
            assert np.array_equal(a["kp"], np.load(io.BytesIO(k)).astype(np.float32)), name


def test_several_videos_with_gaps_and_in_reverse_order(tmp_path):
    A = IC.archive_cases()
    files = [A[k][:2] for k in ("plain_f32", "all_f64", "mixed_f32_f64", "uncompressed", "kp_shorter", "kp_absent",
                                "one_frame")]
    rows, st, a, _ = assert_mem_equals_paths(tmp_path, files, 1024, gap=7, order=list(range(2 * len(files)))[::-1])
    assert st.tolist() == [0] * len(files) and [r[2] for r in rows] == [40, 33, 35, 36, 31, -1, 1]


def test_stream_cases_mem_equals_paths(tmp_path):
    """Every crafted member inside a whole video: the host reference gives zlib's verdict through both routes."""
    for name, c in IC.stream_cases().items():
        if c.device_only:
            continue
        z, vit_dim = IC.video_for_stream(c)
        d = tmp_path / name
        d.mkdir()
        rows, st, a, _ = assert_mem_equals_paths(d, [(z, None)], vit_dim)
        assert rows[0][3] == 0 and st.tolist() == [0 if c.ok else ERR_IO], name
        if c.ok:
            key = {"vit": "vit", "pose": "pose", "betas": "betas"}[c.member]
            assert a[key].tobytes() == c.payload, name


def _zip64_with_wrapping_cd(src: bytes) -> bytes:
    e = src.rindex(b"PK\x05\x06")
    rec = struct.pack("<IQHHIIQQQQ", 0x06064B50, 44, 45, 45, 0, 0, 1, 1, 32, (1 << 64) - 16)
    loc = struct.pack("<IIQI", 0x07064B50, 0, e, 1)
    eocd = bytearray(src[e:])
    eocd[10:12] = b"\xff\xff"
    eocd[12:16] = b"\xff\xff\xff\xff"
    eocd[16:20] = b"\xff\xff\xff\xff"
    return src[:e] + rec + loc + bytes(eocd)


def _patch_shape(raw: bytes, old: bytes, new: bytes) -> bytes:
    i = raw.index(old)
    end = raw.index(b"\n", i)
    line = raw[i:end].replace(old, new, 1).rstrip(b" ")
    assert len(line) <= end - i
    return raw[:i] + line + b" " * (end - i - len(line)) + raw[end:]


def test_crafted_sizes_mem_equals_paths(tmp_path):
    """Zip64 offsets that wrap, npy shapes whose element count overflows, garbage and empty files: refused alike."""
    good = IC.savez(IC.clip_arrays(30, 32, 64))
    kp = IC.kp_bytes(30, 32)
    stored = IC.savez({"pose": np.zeros((2, 23, 3, 3), np.float32), "global_orient": np.zeros((2, 1, 3, 3), np.float32),
                       "betas": np.zeros((2, 10), np.float32), "vit": np.zeros((2, 64), np.float32)}, compressed=False)
    files = [(_zip64_with_wrapping_cd(good), kp),
             (good, _patch_shape(kp, b"(32, 120)", f"({1 << 62}, 120)".encode())),
             (_patch_shape(stored, b"(2, 23, 3, 3)", f"({1 << 40}, 23, 3, 3)".encode()), None),
             (b"not a zip file at all, just some bytes", kp),
             (good, b""),
             (good, kp)]
    rows, st, _, _ = assert_mem_equals_paths(tmp_path, files, 64, gap=5)
    assert [r[3] for r in rows] == [ERR_IO, ERR_KP, ERR_SHAPE, ERR_IO, ERR_KP, 0]


def test_plan_descriptors_against_numpy():
    A = IC.archive_cases()
    names = ("plain_f32", "all_f64", "mixed_f32_f64", "uncompressed", "kp_shorter", "kp_absent", "one_frame")
    files = [A[k][:2] for k in names]
    data, off, size = IC.pack(files, gap=9)
    _, rows = IC.host_probe_mem(data, off, size)
    videos, F, Fk = IC.video_table(rows)
    rc, descs, prow, ws = IC.host_plan_mem(data, off, size, videos, 1024)
    assert rc == 0 and prow == rows
    width = {"pose": 207, "global_orient": 9, "betas": 10, "vit": 1024}
    want_ws = 0
    for i, (z, k) in enumerate(files):
        ref = np.load(io.BytesIO(z))
        with __import__("zipfile").ZipFile(io.BytesIO(z)) as zf:
            zi = {m.filename: m for m in zf.infolist()}
        for a, key in enumerate(("pose", "global_orient", "betas", "vit")):
            d, arr, m = descs[5 * i + a], ref[key], zi[key + ".npy"]
            raw = IC.npy_bytes(arr)
            assert (d.array, d.video, d.count, d.itemsize, d.skip) == (a, i, arr.size, arr.dtype.itemsize,
                                                                       len(raw) - arr.nbytes), (names[i], key)
            assert (d.method, d.csize, d.dst_off) == (m.compress_type, m.compress_size, int(videos[i, 0]) * width[key])
            comp = data[d.src_off:d.src_off + d.csize].tobytes()
            assert (zlib.decompressobj(-15).decompress(comp) if d.method == 8 else comp) == raw, (names[i], key)
            if d.itemsize == 8:
                assert d.ws_off == want_ws
                want_ws += 8 * d.count
            else:
                assert d.ws_off == -1
        d = descs[5 * i + 4]
        if k is None:
            assert d.array == -1
        else:
            karr = np.load(io.BytesIO(k))
            assert (d.array, d.video, d.count, d.itemsize, d.skip, d.method) == (4, i, karr.size, karr.dtype.itemsize,
                                                                                 len(k) - karr.nbytes, 0)
            assert (d.src_off, d.csize, d.dst_off) == (off[2 * i + 1], len(k), int(videos[i, 2]) * 120)
            if d.itemsize == 8:
                assert d.ws_off == want_ws
                want_ws += 8 * d.count
    assert ws == max(want_ws, 8)
    from vge import lib as L
    assert L.load().vge_ingest_decode_device_workspace_bytes(descs, 5 * len(files)) == ws


def test_plan_refuses_what_the_decoder_refuses():
    """Shape and count checks happen in the plan with the decoder's codes; a refused video gets no streams."""
    A = IC.archive_cases()
    good = A["plain_f32"]
    files = [good[:2], (good[0], IC.kp_bytes(1, 39)), (IC.savez(IC.clip_arrays(40, 40, 64)), None),
             (b"PK\x05\x06" + bytes(18), None), good[:2]]
    data, off, size = IC.pack(files, gap=2)
    videos = np.array([[0, 40, 0, 40], [40, 40, 40, 40], [80, 40, 80, 0], [120, 3, 80, 0], [123, 39, 80, 40]], np.int32)
    rc, descs, rows, _ = IC.host_plan_mem(data, off, size, videos, 1024)
    _, st, _ = IC.host_decode_mem(data, off, size, videos, 1024, 162, 120)
    assert [r[3] for r in rows] == st.tolist() == [0, ERR_KP, ERR_SHAPE, ERR_IO, ERR_SHAPE] and rc == ERR_KP
    for i, r in enumerate(rows):
        used = [descs[5 * i + a].array for a in range(5)]
        assert used == ([0, 1, 2, 3, 4] if r[3] == 0 else [-1] * 5), i


def test_files_outside_the_buffer_are_refused_unread():
    """A file that does not lie inside [0, data_bytes) gets ERR_ARG; its bytes are not read: the buffer handed over is
    shorter than the allocation behind it, and the out-of-range entries point far outside both."""
    A = IC.archive_cases()
    files = [A["plain_f32"][:2]] * 5
    data, off, size = IC.pack(files)
    off, size = off.copy(), size.copy()
    off[2] = -1                       # negative offset
    off[4] = data.size - 10           # runs past the end
    off[7] = 1 << 60                  # keypoint file far outside
    size[8] = -5                      # an npz of negative size
    rc, rows = IC.host_probe_mem(data, off, size)
    assert rc == ERR_ARG and [r[3] for r in rows] == [0, ERR_ARG, ERR_ARG, ERR_ARG, ERR_ARG]
    videos, F, Fk = IC.video_table(rows)
    rc, st, a = IC.host_decode_mem(data, off, size, videos, 1024, F, Fk)
    assert rc == ERR_ARG and st.tolist() == [0, ERR_ARG, ERR_ARG, ERR_ARG, ERR_ARG]
    rc, descs, prow, _ = IC.host_plan_mem(data, off, size, videos, 1024)
    assert rc == ERR_ARG and [r[3] for r in prow] == [0, ERR_ARG, ERR_ARG, ERR_ARG, ERR_ARG]
    assert all(descs[k].array == -1 for k in range(5, 25))
    from vge import lib as L
    lib = L.load()
    info = (L.ClipInfo * 5)()
    assert lib.vge_ingest_probe_mem(IC._ptr(data), -1, IC._ptr(off), IC._ptr(size), 5, 1, info) == ERR_ARG
    assert lib.vge_ingest_probe_mem(None, 10, IC._ptr(off), IC._ptr(size), 5, 1, info) == ERR_ARG


# ---- the code-length rules against zlib

SET_ERROR = {IC.CODES: "invalid code lengths set", IC.LENS: "invalid literal/lengths set",
             IC.DISTS: "invalid distances set"}


def zlib_accepts_set(stream: bytes, kind) -> bool:
    """zlib's verdict on the set of `kind` in a dynamic block header that is otherwise in order: it raises that set's
    error, or goes on (whatever it then makes of the padding bits behind the header is not the set's verdict)."""
    try:
        zlib.decompressobj(-15).decompress(stream)
    except zlib.error as e:
        return SET_ERROR[kind] not in str(e)
    return True


def check(lens, kind) -> bool:
    from vge import lib as L
    a = np.asarray(lens, np.uint8)
    r = L.load().vge_inflate_check_lengths(IC._ptr(a), len(a), kind)
    assert r in (0, 1)
    return r == 0


def random_set(g, n, must=None, longest=15):
    """Random lengths for n symbols around a complete code: exact, over-subscribed, incomplete, tiny or empty."""
    mode = g.integers(0, 8)
    used = int(g.integers(1, n + 1)) if mode else int(g.integers(0, 3))
    syms = g.permutation(n)[:used].tolist()
    if must is not None and must not in syms:
        syms = [must] + syms[:max(used - 1, 0)]
    lens = [0] * n
    if not syms:
        return lens
    # split the code space: start with one code of length 0 and split random leaves until every symbol has one
    leaves = [0]
    while len(leaves) < len(syms):
        k = int(g.integers(0, len(leaves)))
        if leaves[k] >= longest:
            if all(l >= longest for l in leaves):
                break
            continue
        leaves[k] += 1
        leaves.append(leaves[k])
    leaves = [max(l, 1) for l in leaves]
    for s, l in zip(syms, leaves):
        lens[s] = l
    for _ in range(int(g.integers(0, 3)) if mode > 3 else 0):   # perturb: usually breaks completeness one way or the other
        s = syms[int(g.integers(0, len(syms)))]
        lens[s] = int(np.clip(lens[s] + g.integers(-2, 3), 0 if s != must else 1, longest))
    return lens


def test_length_rules_equal_zlib():
    g = np.random.default_rng(1951)
    ok_ll = IC.pad_lens({**{k: 8 for k in range(255)}, 256: 8}, 257)
    seen = {}
    sets = []
    for _ in range(2200):
        sets.append((IC.LENS, random_set(g, int(g.integers(257, 287)), must=256)))
    for _ in range(2200):
        sets.append((IC.DISTS, random_set(g, int(g.integers(1, 31)))))
    for _ in range(1200):
        sets.append((IC.CODES, random_set(g, 19, longest=7)))   # the header sends these in 3 bits
    one = IC.pad_lens({256: 1}, 257)
    sets += [(IC.LENS, one), (IC.LENS, IC.pad_lens({0: 1, 256: 1}, 257)), (IC.LENS, IC.pad_lens({256: 2}, 257)),
             (IC.LENS, IC.pad_lens({0: 1, 1: 1, 256: 1}, 257)), (IC.LENS, IC.FIXED_LL[:286]),
             (IC.DISTS, [0]), (IC.DISTS, [0] * 30), (IC.DISTS, [1]), (IC.DISTS, [0, 0, 1]), (IC.DISTS, [2]),
             (IC.DISTS, [1, 1]), (IC.DISTS, [1, 1, 1]), (IC.DISTS, [15] * 30), (IC.DISTS, [5] * 30),
             (IC.CODES, [1] + [0] * 18), (IC.CODES, [1, 1] + [0] * 17), (IC.CODES, [7] * 19), (IC.CODES, [2] * 4 + [0] * 15),
             (IC.CODES, IC.CL_PLAIN)]
    for kind, lens in sets:
        if kind == IC.CODES and not any(lens):
            continue   # the empty code-length code: below
        w = IC.BitWriter()
        if kind == IC.LENS:
            IC.dynamic_header(w, lens, [0])
        elif kind == IC.DISTS:
            IC.dynamic_header(w, ok_ll, lens)
        else:
            IC.dynamic_header(w, ok_ll, [0], cl=lens, cl_syms=[])
        want = zlib_accepts_set(w.bytes(), kind)
        got = check(lens, kind)
        assert got == want == IC.set_verdict(lens, kind), (kind, lens)
        seen[(kind, want)] = seen.get((kind, want), 0) + 1
    assert sum(seen.values()) >= 5000 and all(seen.get((k, v), 0) >= 100 for k in range(3) for v in (True, False)), seen
    # an empty code-length code: zlib builds it, reads every length as 0 and rejects the block; the shared rule
    # rejects the set at once -- the stream's verdict is the same
    w = IC.BitWriter()
    IC.dynamic_header(w, ok_ll, [0], cl=[0] * 19, cl_syms=[])
    with pytest.raises(zlib.error, match="missing end-of-block"):
        zlib.decompressobj(-15).decompress(w.bytes() + bytes(64))
    assert not check([0] * 19, IC.CODES)
    from vge import lib as L
    bad = np.array([16, 1], np.uint8)
    assert L.load().vge_inflate_check_lengths(IC._ptr(bad), 2, 1) == -1
    assert L.load().vge_inflate_check_lengths(None, 2, 1) == -1 and L.load().vge_inflate_check_lengths(IC._ptr(bad), 1, 3) == -1


def test_ingest_argument_is_checked_and_on_the_command_lines(tmp_path, capsys):
    """ingest is "host" or "device" wherever a frame store is built; anything else is refused before any work."""
    from vge import dist as VD
    from vge import eval as VE
    from vge import validate as VV
    assert VE.INGEST_ROUTES == ("host", "device")
    with pytest.raises(ValueError, match="ingest"):
        VE.device_frame_store([], None, False, "cpu", ingest="gpu")
    with pytest.raises(ValueError, match="ingest"):
        VE.run_eval(str(tmp_path), str(tmp_path), None, None, None, out_json=None, ingest="gpu")
    with pytest.raises(ValueError, match="ingest"):
        VD.run_eval_distributed(str(tmp_path), str(tmp_path), None, None, None, out_json=None, ingest="gpu")
    for mod, argv in ((VE, ["--generated-meshes", "g", "--real-meshes", "r", "--model", "m", "--ingest", "gpu"]),
                      (VV, ["--real-meshes", "r", "--ingest", "gpu", "ckpt"])):
        with pytest.raises(SystemExit):
            mod.main(argv)
        assert "--ingest" in capsys.readouterr().err
