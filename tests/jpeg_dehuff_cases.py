"""Shared by tests/test_jpeg_dehuff_host.py and tests/test_jpeg_dehuff_gpu.py: the three JPEG fixtures' files, packing,
the host calls both make (the memory decoder is the device decoder's reference), and the seeded corrupt streams."""
import ctypes as C
import functools

import numpy as np

from tests.conftest import GOLDEN

ERR_ARG, ERR_IO, ERR_SHAPE, ERR_PROGRESSIVE = 1, 7, 8, 20
CANARY = 0x5A
FLIP_SEED = 20250311      # checked by flip_set_verdicts(): the set holds streams the host accepts and ones it refuses
FLIP_COUNT = 24
FLIP_FILE = "17x33_444_noise"     # jpeg_golden.npz, no restart markers
ROUNDS_CASE = "only63"    # found by find_rounds_case(): the first synthetic_set entry whose rounds[] exceeds 2
DENSE_QUALITY = 100       # dense_frame() is coded with tables of 1, so that its blocks stay inside VGE_JPEG_BLOCK_L1_MAX
L1_REFUSED = ("max_block", "dense")   # synthetic_set entries beyond that bound at quality 95: ERR_IO on both sides


@functools.lru_cache(maxsize=None)
def all_files():
    """{name: bytes} of every jpeg/ and bad/ entry of the three fixtures, in fixture order."""
    out = {}
    for f in ("jpeg_golden.npz", "jpeg_enc_golden.npz", "jpeg_dehuff_golden.npz"):
        g = np.load(GOLDEN / f)
        for k in g.files:
            if k.startswith("jpeg/") or k.startswith("bad/"):
                name = k.split("/", 1)[1]
                assert name not in out, name
                out[name] = g[k].tobytes()
    return out


def pack(files, gap=0, order=None):
    """files (list of bytes) -> (data uint8, offsets int64 [n], sizes int64 [n]).  `gap` canary bytes in front of,
    between and behind the files; `order`: the files' order inside data (offsets stay indexed like `files`)."""
    n = len(files)
    order = list(range(n)) if order is None else list(order)
    sizes = np.array([len(f) for f in files], np.int64)
    offsets = np.zeros(n, np.int64)
    o = gap
    for i in order:
        offsets[i] = o
        o += len(files[i]) + gap
    data = np.full(max(o, 1), CANARY, np.uint8)
    for i in range(n):
        data[offsets[i]:offsets[i] + sizes[i]] = np.frombuffer(files[i], np.uint8)
    return data, offsets, sizes


def probe_one(blob):
    """The probe row (width, height, components, h0, v0, status) of one file in memory."""
    from vge.frames import probe_mem
    d = np.frombuffer(blob, np.uint8) if len(blob) else np.zeros(1, np.uint8)
    return probe_mem(d, np.zeros(1, np.int64), np.array([len(blob)], np.int64), 1)[0]


def layout_of(blob):
    from vge.frames import make_layout
    row = probe_one(blob)
    assert int(row[5]) == 0, row
    return make_layout(*[int(x) for x in row[:5]])


def host_decode_mem(data, offsets, sizes, lay, threads=2, data_bytes=None):
    """vge_jpeg_entropy_decode_mem -> (return code, status [n], coef int16 [n, blocks, 64], qtab uint16 [n, 3, 64]);
    the outputs start as canaries."""
    from vge import lib as L
    n = len(offsets)
    coef = np.full((n, lay.blocks_per_frame, 64), 0x5A5A, np.int16)
    qtab = np.full((n, 3, 64), 0x5A5A, np.uint16)
    st = np.full(n, -1, np.int32)
    rc = L.load().vge_jpeg_entropy_decode_mem(data.ctypes.data, data.size if data_bytes is None else data_bytes,
                                              offsets.ctypes.data, sizes.ctypes.data, n, threads, C.byref(lay),
                                              coef.ctypes.data, qtab.ctypes.data, st.ctypes.data)
    return rc, st, coef, qtab


def host_decode_files(files, lay):
    return host_decode_mem(*pack(files), lay)


def host_decode_paths(paths, lay, threads=2):
    from vge import lib as L
    n = len(paths)
    coef = np.full((n, lay.blocks_per_frame, 64), 0x5A5A, np.int16)
    qtab = np.full((n, 3, 64), 0x5A5A, np.uint16)
    st = np.full(n, -1, np.int32)
    arr = (C.c_char_p * n)(*[p.encode() for p in paths])
    rc = L.load().vge_jpeg_entropy_decode(arr, n, threads, C.byref(lay), coef.ctypes.data, qtab.ctypes.data,
                                          st.ctypes.data)
    return rc, st, coef, qtab


# ---- corrupt streams
def scan_start(blob):
    """Offset of the first entropy-coded byte: behind the SOS segment."""
    i = 2
    while True:
        assert blob[i] == 0xFF, i
        m, ln = blob[i + 1], (blob[i + 2] << 8) | blob[i + 3]
        i += 2 + ln
        if m == 0xDA:
            return i


def restart_markers(blob):
    """Offsets of the FF of every RSTn inside the scan."""
    s = scan_start(blob)
    return [i for i in range(s, len(blob) - 1) if blob[i] == 0xFF and 0xD0 <= blob[i + 1] <= 0xD7]


def cuts(blob):
    """{what: the file cut there}: inside the header, at the first scan byte, between an FF and its 00, one byte
    before EOI's last byte."""
    s = scan_start(blob)
    ff = next(i for i in range(s, len(blob) - 2) if blob[i] == 0xFF and blob[i + 1] == 0x00)
    return {"header": blob[:s // 2], "scan0": blob[:s], "scan1": blob[:s + 1], "ff_00": blob[:ff + 1],
            "last_scan_byte": blob[:-3], "before_eoi": blob[:-2], "half_eoi": blob[:-1]}


def wrong_marker_index(blob):
    m = restart_markers(blob)[3]
    b = bytearray(blob)
    b[m + 1] = 0xD0 + ((b[m + 1] - 0xD0 + 3) & 7)
    return bytes(b)


def removed_marker(blob):
    m = restart_markers(blob)[2]
    return blob[:m] + blob[m + 2:]


def surplus_before_marker(blob):
    """A whole extra byte between an interval's last MCU and its marker: the documented class where the host's verdict
    depends on its reader's lookahead and the device always answers ERR_IO."""
    m = restart_markers(blob)[1]
    return blob[:m] + b"\x55" + blob[m:]


def flip_set(blob=None, seed=FLIP_SEED, count=FLIP_COUNT):
    """`count` copies of the file, each with one seeded bit of its scan flipped (never making or breaking an FF)."""
    blob = all_files()[FLIP_FILE] if blob is None else blob
    g = np.random.default_rng(seed)
    s, e = scan_start(blob), len(blob) - 2
    out = []
    while len(out) < count:
        i, bit = int(g.integers(s, e)), int(g.integers(0, 8))
        b = bytearray(blob)
        b[i] ^= 1 << bit
        if blob[i] == 0xFF or b[i] == 0xFF or (blob[i - 1] == 0xFF and i > s):
            continue   # keeps the byte structure: the flip lands in the Huffman-coded bits only
        out.append(bytes(b))
    return out


def flip_set_verdicts():
    """The authoring-time check behind FLIP_SEED: host statuses of the flip set (tests/test_jpeg_dehuff_host.py asserts
    that both verdicts occur)."""
    files = flip_set()
    return host_decode_files(files, layout_of(all_files()[FLIP_FILE]))[1]


def dense_frame(tile_bytes, seed=5):
    """A 4:4:4 frame of dense random coefficients (every one non-zero, |c| <= 700: a block is about 1,500 bits, five
    subsequences, and its L1 norm at DENSE_QUALITY about 22,400 +- 1,600) whose scan is at least three tiles and not a
    whole number of them: (layout, int16 [blocks, 64])."""
    from tests import jpeg_entropy_cases as EC
    blocks_needed = int(3.3 * tile_bytes / 150)
    side = 8 * int(np.ceil(np.sqrt(blocks_needed / 3.0)))
    lay = EC.layout(side, side, "444")
    g = np.random.default_rng(seed)
    c = g.integers(1, 701, size=(lay.blocks_per_frame, 64)) * g.choice([-1, 1], size=(lay.blocks_per_frame, 64))
    c[:, 0] = g.integers(-300, 300, size=lay.blocks_per_frame)   # DC values, within the 11-bit difference
    return lay, c.astype(np.int16)


def find_rounds_case(decode_rounds):
    """The authoring-time search behind ROUNDS_CASE: decode_rounds(name, shape, coef) -> rounds[0] on the device; the
    first synthetic_set entry that needs more than two rounds."""
    from tests import jpeg_entropy_cases as EC
    for name, shape, coef in EC.synthetic_set():
        if decode_rounds(name, shape, coef) > 2:
            return name
    raise AssertionError("no case found")
