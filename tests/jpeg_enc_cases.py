"""Shared by tests/test_jpeg_encode_host.py and tests/test_jpeg_encode_gpu.py: the encoder fixture
(tests/golden/make_jpeg_enc_golden.py) and the ABI calls both files make."""
import ctypes as C

import numpy as np

from tests.conftest import GOLDEN

SAMPLING = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}


def load_gold():
    return dict(np.load(GOLDEN / "jpeg_enc_golden.npz"))


def all_cases(gold):
    return list(gold["names"]) + list(gold["batch_names"]) + list(gold["tile_names"])


def parts(case):
    """'<image>_<sampling>_q<quality>' -> (image, sampling, quality)."""
    image, sub, q = str(case).rsplit("_", 2)
    return image, sub, int(q[1:])


def write_files(gold, root):
    """Every fixture JPEG written to disk once: {case: path}."""
    out = {}
    for case in all_cases(gold):
        p = root / f"{case}.jpg"
        p.write_bytes(gold[f"jpeg/{case}"].tobytes())
        out[case] = str(p)
    return out


def layout_for(img, sub):
    from vge.frames import make_layout
    return make_layout(img.shape[1], img.shape[0], 3, *SAMPLING[sub])


def pillow_coefficients(path, lay):
    """(int16 [blocks, 64], uint16 [3, 64]) that vge_jpeg_entropy_decode reads out of Pillow's file."""
    from vge import lib as L
    coef = np.full((1, lay.blocks_per_frame, 64), 0x5a5a, np.int16)
    qtab = np.zeros((1, 3, 64), np.uint16)
    st = np.zeros(1, np.int32)
    paths = (C.c_char_p * 1)(path.encode())
    assert L.load().vge_jpeg_entropy_decode(paths, 1, 1, C.byref(lay), coef.ctypes.data, qtab.ctypes.data,
                                            st.ctypes.data) == 0 and st[0] == 0
    return coef[0], qtab[0]


def host_forward(frames, lay, quality):
    """vge_jpeg_forward_host on uint8 [F, H, W, 3] -> int16 [F, blocks, 64]."""
    from vge import lib as L
    from vge.frames import quant_tables
    frames = np.ascontiguousarray(frames)
    coef = np.full((frames.shape[0], lay.blocks_per_frame, 64), 0x5a5a, np.int16)
    q = quant_tables(quality)
    assert L.load().vge_jpeg_forward_host(frames.ctypes.data, C.byref(lay), frames.shape[0], 2, q.ctypes.data,
                                          coef.ctypes.data) == 0
    return coef
