"""Shared by tests/test_jpeg_entropy_host.py and tests/test_jpeg_entropy_gpu.py: the seeded synthetic coefficient set,
its ground truth by the plain-Python restatement (tests/jpeg_huff_ref.py), and the ABI calls both files make."""
import ctypes as C
import functools

import numpy as np

from tests import jpeg_enc_cases as JC
from tests import jpeg_huff_ref as R

TEMPLATE_CASE = "37x53_noise_420_q95"   # the fixture file whose DHT segments and header the restatement uses
FF_TAIL_SEED = 42                       # found by find_ff_tail_seed() at authoring time
ERR_ARG, ERR_IO, ERR_COMPONENTS = 1, 7, 23


def layout(width, height, sub):
    from vge.frames import make_layout
    return make_layout(width, height, 3, *JC.SAMPLING[sub])


def template(gold):
    return gold[f"jpeg/{TEMPLATE_CASE}"].tobytes()


def ff_tail_frame(seed):
    """One 8 x 8 4:4:4 frame (three blocks) of sparse random coefficients."""
    g = np.random.default_rng(seed)
    coef = np.zeros((3, 64), np.int16)
    mask = g.random((3, 64)) < 0.3
    coef[mask] = g.integers(-40, 41, size=int(mask.sum()))
    return coef


def find_ff_tail_seed(gold, limit=100000):
    """The authoring-time search behind FF_TAIL_SEED: the first seed whose frame's padded last scan byte is FF."""
    from vge.frames import quant_tables
    lay, q = layout(8, 8, "444"), quant_tables(95)
    for seed in range(limit):
        if R.encode(ff_tail_frame(seed), q, lay, template(gold)).endswith(b"\xff\x00\xff\xd9"):
            return seed
    raise AssertionError("no seed found")


def synthetic_set():
    """[(name, (width, height, sampling), int16 [blocks, 64])], seeded.  Each entry is there for a path of the coder:
    see tests/test_jpeg_entropy_host.py::test_synthetic_set_equals_the_restatement."""
    g = np.random.default_rng(20240607)
    out = []
    lay = layout(16, 16, "420")
    out.append(("zero", (16, 16, "420"), np.zeros((lay.blocks_per_frame, 64), np.int16)))
    lay = layout(32, 16, "422")
    c = np.zeros((lay.blocks_per_frame, 64), np.int16)
    c[:, 63] = g.integers(1, 9, size=lay.blocks_per_frame) * g.choice([-1, 1], size=lay.blocks_per_frame)
    out.append(("only63", (32, 16, "422"), c))
    lay = layout(16, 16, "444")   # zero runs of exactly 15 and exactly 16, after the DC and between coefficients
    c = np.zeros((lay.blocks_per_frame, 64), np.int16)
    for b in range(lay.blocks_per_frame):
        first = 16 if b % 2 == 0 else 17            # zigzag 1 .. 15 zero: a run of 15; 1 .. 16: ZRL + run 0
        second = first + (17 if b % 3 == 0 else 16)  # 16 zeros between the two, or 15
        for k in (first, second, 63 if b % 4 == 1 else 50):
            c[b, R.ZZ[k]] = int(g.integers(1, 30)) * (-1 if (b + k) % 2 else 1)
        c[b, 0] = int(g.integers(-50, 50))
    out.append(("runs15_16", (16, 16, "444"), c))
    c = np.zeros((lay.blocks_per_frame, 64), np.int16)   # the 1,658-bit block, DC steps of +-2040
    order = R.scan_order(lay)
    seen = [0, 0, 0]
    for comp, b in order:
        c[b, 0] = 1016 if seen[comp] % 2 == 0 else -1024
        seen[comp] += 1
        c[b, 1:] = 1023 * g.choice([-1, 1], size=63)
    out.append(("max_block", (16, 16, "444"), c))
    lay = layout(48, 40, "444")
    out.append(("dense", (48, 40, "444"), g.integers(-1023, 1024, size=(lay.blocks_per_frame, 64)).astype(np.int16)))
    lay = layout(520, 280, "444")
    c = np.zeros((lay.blocks_per_frame, 64), np.int16)
    mask = g.random(c.shape) < 0.04
    c[mask] = (g.geometric(0.2, size=int(mask.sum())) * g.choice([-1, 1], size=int(mask.sum()))).clip(-1023, 1023)
    c[:, 0] = g.integers(-300, 300, size=lay.blocks_per_frame)
    out.append(("sparse_520x280", (520, 280, "444"), c))
    out.append(("ff_tail", (8, 8, "444"), ff_tail_frame(FF_TAIL_SEED)))
    return out


@functools.lru_cache(maxsize=None)
def synthetic_truth():
    """{name: bytes} by the restatement, computed once per process and shared."""
    from vge.frames import quant_tables
    gold = JC.load_gold()
    q = quant_tables(95)
    return {name: R.encode(coef, q, layout(*shape), template(gold)) for name, shape, coef in synthetic_set()}


def refusal_batch(kind):
    """Three 16 x 16 4:2:0 frames; the middle one holds an AC of 1024 ('ac') or a DC step of 2048 ('dc')."""
    g = np.random.default_rng(7)
    lay = layout(16, 16, "420")
    c = g.integers(-60, 61, size=(3, lay.blocks_per_frame, 64)).astype(np.int16)
    if kind == "ac":
        c[1, 2, 9] = 1024
    else:
        c[1, 0, 0], c[1, 1, 0] = -1024, 1024   # the MCU's first two luma blocks: consecutive in the scan
    return lay, c


def encode_mem(coef, lay, quality=95, offsets=None, out=None, threads=2):
    """vge_jpeg_entropy_encode_mem on int16 [n, blocks, 64] -> (return code, sizes, status, [bytes per frame] or None).
    Without `offsets` the files are packed back to back in a buffer made here."""
    from vge import lib as L
    from vge.frames import quant_tables
    coef = np.ascontiguousarray(coef, np.int16)
    n = coef.shape[0]
    q = quant_tables(quality)
    so = L.load()
    sizes, st = np.full(n, -1, np.int64), np.full(n, -1, np.int32)
    rc = so.vge_jpeg_entropy_encode_mem(coef.ctypes.data, q.ctypes.data, C.byref(lay), n, threads, None, None, 0,
                                        sizes.ctypes.data, st.ctypes.data)
    own = offsets is None
    if own:
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        out = np.zeros(int(sizes.sum()), np.uint8)
    sizes2, st2 = np.full(n, -1, np.int64), np.full(n, -1, np.int32)
    rc2 = so.vge_jpeg_entropy_encode_mem(coef.ctypes.data, q.ctypes.data, C.byref(lay), n, threads,
                                         offsets.ctypes.data, out.ctypes.data, out.size, sizes2.ctypes.data,
                                         st2.ctypes.data)
    if own or rc2 == 0:   # sizes-only mode agrees (a caller's buffer may be too short for a file: its size is then 0)
        assert rc == rc2 and np.array_equal(sizes, sizes2) and np.array_equal(st, st2)
    files = [out[int(o):int(o) + int(s)].tobytes() for o, s in zip(offsets, sizes2)]
    return rc2, sizes2, st2, files
