"""The device inflate (csrc/vge_inflate.hip: vge_ingest_decode_device) and the Python layer on it
(load_device_frame_store, ingest="device") against the host reference vge_ingest_decode_mem: exact equality of
statuses and of all five frame-store arrays, with canaries around every array, in the gaps of the file buffer and
around the workspace.  Streams come from tests/inflate_cases.py, which has asserted each one's property on the CPU."""
import json

import numpy as np
import pytest
import torch

from tests import inflate_cases as IC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64            # canary elements in front of and behind every output buffer
CANARY = 0x5A5A5A5A
ERR_IO, ERR_SHAPE, ERR_KP = 7, 8, 9
WIDTH = {"pose": 207, "gori": 9, "betas": 10, "kp": 120}


def lib():
    from vge import lib as L
    return L.load()


def device_decode(data, off, size, videos, vit_dim, F, Fk, ws=None):
    """Plan on the host, decode on the device -> (return code, combined status [n], the five arrays as int32 bit
    patterns, whether every canary and the input buffer survived, the workspace tensor)."""
    n = len(off) // 2
    _, descs, rows, ws_bytes = IC.host_plan_mem(data, off, size, videos, vit_dim)
    plan_st = np.array([r[3] for r in rows], np.int32)
    d = torch.from_numpy(data).to(DEV)
    dd = torch.from_numpy(np.frombuffer(bytes(descs), np.uint8).copy()).to(DEV)
    bufs = {}
    for k in ("pose", "gori", "betas", "vit", "kp"):
        rows_k = max(Fk, 1) if k == "kp" else F
        bufs[k] = torch.full((rows_k * WIDTH.get(k, vit_dim) + 2 * PAD,), CANARY, dtype=torch.int32, device=DEV)
    st = torch.full((n + 2 * PAD,), -77, dtype=torch.int32, device=DEV)
    if ws is None:
        ws = torch.full((ws_bytes + 512,), 0x5A, dtype=torch.uint8, device=DEV)
    assert ws.numel() == ws_bytes + 512
    p = {k: v[PAD:].data_ptr() for k, v in bufs.items()}
    rc = lib().vge_ingest_decode_device(d.data_ptr(), data.size, dd.data_ptr(), 5 * n, n, F, max(Fk, 1), vit_dim,
                                        p["pose"], p["gori"], p["betas"], p["vit"], p["kp"], ws[256:].data_ptr(),
                                        ws_bytes, st[PAD:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    intact = all(bool((t[:PAD] == v).all()) and bool((t[t.numel() - PAD:] == v).all())
                 for t, v in [(b, CANARY) for b in bufs.values()] + [(st, -77)])
    intact = intact and bool((ws[:256] == 0x5A).all()) and bool((ws[256 + ws_bytes:] == 0x5A).all())
    intact = intact and np.array_equal(d.cpu().numpy(), data) and bytes(dd.cpu().numpy()) == bytes(descs)
    dev_st = st[PAD:PAD + n].cpu().numpy()
    assert not (plan_st != 0)[dev_st != 0].any()       # a video the plan refused has no streams to fail
    out = {k: v[PAD:v.numel() - PAD].cpu().numpy().reshape(-1, WIDTH.get(k, vit_dim)) for k, v in bufs.items()}
    return rc, np.where(plan_st != 0, plan_st, dev_st), out, intact, ws


def rows_of(videos, i, k):
    o, T, ko, kT = (int(x) for x in videos[i])
    return slice(ko, ko + kT) if k == "kp" else slice(o, o + T)


def assert_equals_host(files, vit_dim, what, gap=16, order=None, ws=None):
    """Device statuses equal the host's and accepted videos are bit-equal in all five arrays (a refused video's own rows
    may hold anything); the canaries around every buffer and the input are intact."""
    data, off, size = IC.pack(files, gap=gap, order=order)
    _, rows = IC.host_probe_mem(data, off, size)
    videos, F, Fk = IC.video_table(rows)
    _, hst, ha = IC.host_decode_mem(data, off, size, videos, vit_dim, F, Fk)
    rc, st, da, intact, ws = device_decode(data, off, size, videos, vit_dim, F, Fk, ws=ws)
    assert rc == 0 and intact, what
    assert st.tolist() == hst.tolist(), (what, st.tolist(), hst.tolist())
    for i in range(len(files)):
        if st[i] == 0:
            for k in da:
                r = rows_of(videos, i, k)
                assert np.array_equal(da[k][r], ha[k][r].view(np.int32)), (what, i, k)
    if Fk == 0:
        assert (da["kp"] == CANARY).all(), what
    return st, da, videos, ws


def test_every_stream_case_equals_the_host():
    """One video per call around each crafted or zlib-made member: stored, fixed and dynamic blocks, codes beyond the
    lookup table and of 15 bits, long and overlapping matches, matches into the npy header and across its end, distance
    32,768, matches into earlier blocks, empty blocks, the one-code distance set, and every class zlib rejects."""
    L = lib()
    batch, ring, stage = (L.vge_ingest_decode_device_batch_symbols(), L.vge_ingest_decode_device_ring_bytes(),
                          L.vge_ingest_decode_device_stage_bytes())
    cases = IC.stream_cases()
    big = cases["dynamic_four_blocks"]
    info = IC.inflate(big.stream)
    assert info.n_symbols > 100 * batch and big.total > 4 * ring and len(big.stream) > 50 * stage  # batches, ring wraps
    assert cases["distance_32768"].total > ring and IC.inflate(cases["distance_32768"].stream).max_dist == ring
    seen = set()
    for name, c in cases.items():
        z, vit_dim = IC.video_for_stream(c)
        if c.device_only:
            continue
        st, da, videos, _ = assert_equals_host([(z, None)], vit_dim, name)
        assert st.tolist() == [0 if c.ok else ERR_IO], name
        seen.add(int(st[0]))
        if c.ok:
            key = {"vit": "vit", "pose": "pose", "betas": "betas"}[c.member]
            assert da[key].tobytes() == c.payload, name
    assert seen == {0, ERR_IO}


def test_overlong_member_stops_at_the_count():
    """The class outside the equality with the host: a stream that carries more than its header declares.  The device
    stops at the count and reports OK, as np.load would."""
    c = IC.stream_cases()["overlong_member"]
    z, vit_dim = IC.video_for_stream(c)
    data, off, size = IC.pack([(z, None)], gap=16)
    _, rows = IC.host_probe_mem(data, off, size)
    videos, F, Fk = IC.video_table(rows)
    rc, st, da, intact, _ = device_decode(data, off, size, videos, vit_dim, F, Fk)
    assert rc == 0 and intact and st.tolist() == [0]
    assert da["vit"].tobytes() == c.payload


def test_archive_cases_equal_the_host():
    """float64 and mixed archives (through the workspace), an uncompressed archive and keypoint files (the copy path),
    keypoints shorter than the mesh or absent, vit_dim 64, one frame, the reference-written archive."""
    import io
    A = IC.archive_cases()
    for name, (z, k, vit_dim) in A.items():
        vit_dim = vit_dim or np.load(io.BytesIO(z))["vit"].shape[1]
        st, _, _, _ = assert_equals_host([(z, k)], vit_dim, name)
        assert st.tolist() == [0], name
    names = ("plain_f32", "all_f64", "mixed_f32_f64", "uncompressed", "kp_shorter", "kp_absent", "one_frame")
    files = [A[k][:2] for k in names]
    st, _, videos, _ = assert_equals_host(files, 1024, "together, gaps, reverse order", gap=13,
                                          order=list(range(2 * len(files)))[::-1])
    assert st.tolist() == [0] * len(files) and videos[:, 3].tolist() == [40, 33, 35, 36, 31, 0, 1]


def mixed_files():
    """Good and refused videos of vit_dim 1024 for one call: a truncated vit stream, a corrupt pose stream (an invalid
    block type in the middle), a float64 member whose stream ends early, a keypoint file the plan refuses."""
    A = IC.archive_cases()
    arr = IC.clip_arrays(50, 34)
    vit = IC.deflate(IC.npy_bytes(arr["vit"]))
    w = IC.BitWriter()
    raw = IC.npy_bytes(arr["pose"])
    IC.stored_block(w, raw[:5000])
    w.put(0, 1)
    w.put(3, 2)
    pose_bad = w.bytes() + bytes(64)
    a64 = IC.clip_arrays(51, 20, dtype=np.float64)
    raw64 = IC.npy_bytes(a64["betas"])
    w = IC.BitWriter()
    IC.stored_block(w, raw64[:900])
    IC.fixed_block(w, list(raw64[900:1000]), final=True)
    return [A["plain_f32"][:2],
            (IC.make_npz(arr, streams={"vit": vit[:len(vit) - 500]}), IC.kp_bytes(50, 34)),
            A["all_f64"][:2],
            (IC.make_npz(arr, streams={"pose": pose_bad}), None),
            (IC.make_npz(a64, streams={"betas": w.bytes()}), IC.kp_bytes(51, 20, np.float64)),
            (A["kp_shorter"][0], IC.npy_bytes(np.zeros((31, 7), np.float32))),
            A["mixed_f32_f64"][:2]]


def test_good_and_refused_videos_in_one_call():
    st, da, videos, _ = assert_equals_host(mixed_files(), 1024, "mixed", gap=32)
    # video 5's probe fails (ERR_KP), so it owns no rows; plan and decoder then refuse it for its shape, before any launch
    assert st.tolist() == [0, ERR_IO, 0, ERR_IO, ERR_IO, ERR_SHAPE, 0] and videos[5].tolist()[1] == 0


def test_reused_workspace_gives_the_same_result():
    files = mixed_files()
    st1, da1, _, ws = assert_equals_host(files, 1024, "first call", gap=8)
    st2, da2, _, _ = assert_equals_host(files, 1024, "second call, same workspace", gap=8, ws=ws)
    assert st1.tolist() == st2.tolist() and np.flatnonzero(st1 == 0).tolist() == [0, 2, 6]


def test_bad_arguments_are_refused_before_any_launch():
    L = lib()
    t = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = t.data_ptr()
    args = lambda **kw: [kw.get("data", p), kw.get("data_bytes", 16), kw.get("descs", p), kw.get("n_descs", 5), 1, 1, 1,  # noqa: E731
                         kw.get("vit_dim", 4), p, p, p, p, p, kw.get("ws", p), 8, kw.get("status", p), None]
    assert L.vge_ingest_decode_device(*args(data_bytes=-1)) == 1
    assert L.vge_ingest_decode_device(*args(vit_dim=0)) == 1
    assert L.vge_ingest_decode_device(*args(data=None)) == 1
    assert L.vge_ingest_decode_device(*args(descs=p + 4)) == 1
    assert L.vge_ingest_decode_device(*args(status=p + 2)) == 1
    assert L.vge_ingest_decode_device(*args(n_descs=0)) == 0
    assert b"vge_ingest_decode_device" in L.vge_last_error()
    torch.cuda.synchronize()
    assert bool((t == 0).all())


def assert_same_store(a, b):
    assert a.names == b.names and a.classes == b.classes
    assert np.array_equal(a.host_videos, b.host_videos) and torch.equal(a.videos, b.videos)
    for k in ("pose", "gori", "betas", "vit"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.dtype == y.dtype and x.device == y.device, k
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k
    nk = int(a.host_videos[:, 3].sum())
    assert a.kp.shape == b.kp.shape and torch.equal(a.kp[:nk].view(torch.int32), b.kp[:nk].view(torch.int32))


def test_load_device_frame_store_equals_the_host_route(golden_dataset):
    from vge import ingest, ops
    from vge.data import NpzVideoDataset, create_dataset_from_generated_meshes
    paths, _ = golden_dataset
    gen = create_dataset_from_generated_meshes(paths["generated_meshes"]).items
    real = NpzVideoDataset(paths["real"]).items
    for items, kp_dir, req in ((gen, paths["generated_kps"], True), (real, paths["real_kp"], False), (gen, None, False)):
        host = ops.DeviceFrameStore.from_host(ingest.load_frame_store_native(items, kp_dir, req), DEV)
        assert_same_store(ingest.load_device_frame_store(items, kp_dir, req, DEV), host)


def test_load_device_frame_store_raises_what_the_host_route_raises(tmp_path):
    from pathlib import Path

    from tests.test_ingest import _write
    from vge import ingest
    from vge.data import VideoItem
    kp_dir = str(tmp_path / "generated_kps")
    good, nokp = _write(tmp_path, "g", 32), _write(tmp_path, "f", 33, kp=False, seed=5)
    bad = _write(tmp_path, "t", 32, seed=7)
    blob = Path(bad.path).read_bytes()
    Path(bad.path).write_bytes(blob[:len(blob) // 2])
    k = _write(tmp_path, "k", 32, seed=8)
    np.save(tmp_path / "generated_kps" / "k" / "keypoints.npy", np.zeros((32, 7), np.float32))
    cut = _write(tmp_path, "c", 40, seed=9)       # the central directory is whole, the vit stream ends early
    arr = IC.clip_arrays(9, 40, 64)
    vit = IC.deflate(IC.npy_bytes(arr["vit"]))
    Path(cut.path).write_bytes(IC.make_npz(arr, streams={"vit": vit[:len(vit) - 300]}))

    def both(items, kd, req):
        out = []
        for fn in (lambda: ingest.load_frame_store_native(items, kd, req),
                   lambda: ingest.load_device_frame_store(items, kd, req, DEV)):
            try:
                fn()
                out.append(None)
            except Exception as e:  # noqa: BLE001
                out.append((type(e), str(e)))
        assert out[0] == out[1], out
        return out[0]

    assert both([good, nokp], kp_dir, True)[0] is FileNotFoundError
    assert both([good, bad], kp_dir, False)[0] is RuntimeError
    assert both([good, k], kp_dir, True)[0] is RuntimeError
    assert both([good, k, nokp], kp_dir, False) is None
    junk = tmp_path / "junk.npz"
    junk.write_bytes(b"PK\x03\x04 not really a zip")
    assert both([VideoItem("Unknown", "junk.npz", str(junk), 1, 64)], None, False)[0] is RuntimeError
    e = both([good, cut], kp_dir, False)
    assert e[0] is RuntimeError and cut.path in e[1] and "decoding" in e[1]
    from vge import ops
    host = ops.DeviceFrameStore.from_host(ingest.load_frame_store_native([good, k, nokp], kp_dir, False), DEV)
    assert_same_store(ingest.load_device_frame_store([good, k, nokp], kp_dir, False, DEV), host)


def test_run_eval_with_device_ingest_writes_the_same_scores(golden_dataset, tmp_path):
    from vge import eval as VE
    paths, ckpt = golden_dataset
    args = (paths["generated_meshes"], paths["real"], ckpt, paths["generated_kps"], paths["real_kp"])
    out = {}
    for route in ("host", "device"):
        VE.run_eval(*args, out_json=str(tmp_path / f"{route}.json"), device=DEV, ingest=route)
        out[route] = (tmp_path / f"{route}.json").read_text()
    assert out["host"] == out["device"]
    assert sorted(json.loads(out["device"])) == sorted(json.loads(out["host"])) and len(json.loads(out["host"])) > 0
    with pytest.raises(ValueError):
        VE.run_eval(*args, out_json=None, device=DEV, ingest="gpu")
