"""Animated PNG files for the tests of the APNG front end (include/vge_apng.h), written chunk by chunk, with a numpy
model of the composition rule (Pillow's, as include/vge_apng.h and DESIGN.md state it) that gives the expected pixels of
every frame that stands, and the C calls.  tests/golden/apng_golden.npz holds what Pillow decodes from the same files
(tests/golden/make_apng_golden.py), so the tests need no Pillow.

The shapes are the smallest at which the kernels can still go wrong: a 37 x 29 canvas (odd, 1073 pixels: five compose
workgroups of 256 lanes with a ragged tail), a 40 x 80 canvas with a 9 x 70 rectangle (two unfilter bands of 64 rows), a
1 x 1 canvas, and the 256 x 256 blend table (every alpha against every value)."""
import struct
import zlib
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np

from tests import inflate_cases as IC
from tests import png_cases as PC

ERR_ARG, ERR_IO, ERR_SHAPE, ERR_INTERLACED, ERR_BITDEPTH, ERR_PALETTE, ERR_BOUNDS = 1, 7, 8, 30, 31, 32, 60
NONE, BACKGROUND, PREVIOUS = 0, 1, 2
SOURCE, OVER = 0, 1
CHANNELS = PC.CHANNELS


@dataclass(frozen=True, eq=False)
class Spec:
    """One frame: its rectangle (x, y, w, h), its pixels uint8 [h, w, C], its operations and how it is written."""
    rect: Tuple[int, int, int, int]
    px: np.ndarray
    dispose: int = NONE
    blend: int = SOURCE
    filters: tuple = PC.CYCLE
    split: object = None    # PC.split's `how`: how the zlib stream is cut into IDAT / fdAT chunks
    stream: Optional[bytes] = None   # the zlib stream, when it is not the one zlib gives for the pixels


def zstream(f: Spec) -> bytes:
    if f.stream is not None:
        return f.stream
    rows = PC.filter_rows(f.px, f.filters)
    return PC.zwrap(IC.deflate(rows, 6), rows)


def fctl(seq, rect, dispose, blend) -> bytes:
    x, y, w, h = rect
    return struct.pack(">IIIIIHHBB", seq, w, h, x, y, 1, 10, dispose, blend)


def chunks(canvas, ct, frames, default=None, trns=None, declared=None, depth=8, lace=0):
    """The file as a list of [type, payload]: IHDR, acTL, tRNS, then the default image's IDATs (when there is one),
    then every frame's fcTL and its IDAT (frame 0 without a default image) or fdAT chunks, then IEND."""
    out = [[b"IHDR", struct.pack(">IIBBBBB", canvas[0], canvas[1], depth, ct, 0, 0, lace)],
           [b"acTL", struct.pack(">II", len(frames) if declared is None else declared, 0)]]
    if trns is not None:
        out.append([b"tRNS", struct.pack(">HHH", *trns) if ct == 2 else struct.pack(">H", trns)])
    if default is not None:
        out += [[b"IDAT", part] for part in PC.split(zstream(default), default.split)]
    for k, f in enumerate(frames):
        out.append([b"fcTL", fctl(0, f.rect, f.dispose, f.blend)])
        kind = b"IDAT" if k == 0 and default is None else b"fdAT"
        out += [[kind, (b"\0\0\0\0" if kind == b"fdAT" else b"") + part] for part in PC.split(zstream(f), f.split)]
    out.append([b"IEND", b""])
    return renumber(out)


def renumber(chs):
    """Sequence numbers 0, 1, 2... over the fcTL and fdAT chunks, in file order."""
    seq = 0
    for c in chs:
        if c[0] in (b"fcTL", b"fdAT"):
            c[1] = struct.pack(">I", seq) + c[1][4:]
            seq += 1
    return chs


def assemble(chs) -> bytes:
    return PC.SIG + b"".join(PC.chunk(t, p) for t, p in chs)


def nth(chs, typ, k):
    """Index of the k-th chunk of a type."""
    return [i for i, c in enumerate(chs) if c[0] == typ][k]


# ---------------------------------------------------------------------------------------- the model of the rule

def _rgb_alpha(px, ct, trns):
    """Frame pixels [h, w, C] -> (RGB int32 [h, w, 3], the alpha OVER uses int32 [h, w], or None when OVER acts as
    SOURCE for this kind of file)."""
    px = px.astype(np.int32)
    if ct == 0:
        return np.repeat(px, 3, axis=2), None
    if ct == 4:
        return np.repeat(px[..., :1], 3, axis=2), px[..., 1]
    if ct == 6:
        return px[..., :3], px[..., 3]
    if trns is None:
        return px, None
    return px, np.where((px == np.array(trns)).all(axis=2), 0, 255).astype(np.int32)


def model(canvas, ct, frames, default=None, trns=None):
    """What PIL.ImageSequence yields after .convert("RGB"), frame by frame: uint8 [F, H, W, 3]."""
    W, H = canvas
    seq = ([Spec((0, 0, W, H), default.px)] if default is not None else []) + list(frames)
    canv = np.zeros((H, W, 3), np.int32)
    pending, out = None, []
    for k, f in enumerate(seq):
        if pending is not None:
            (px_, py_, pw, ph), value = pending
            canv[py_:py_ + ph, px_:px_ + pw] = value
        x, y, w, h = f.rect
        before = canv[y:y + h, x:x + w].copy()
        rgb, a = _rgb_alpha(f.px, ct, trns)
        if f.blend == OVER and k > 0 and a is not None:
            t = rgb * a[..., None] + before * (255 - a[..., None]) + 128
            rgb = (t + (t >> 8)) >> 8
        canv[y:y + h, x:x + w] = rgb
        out.append(canv.astype(np.uint8))
        dispose = BACKGROUND if f.dispose == PREVIOUS and k == 0 else f.dispose
        pending = (f.rect, 0) if dispose == BACKGROUND else (f.rect, before) if dispose == PREVIOUS else None
    return np.stack(out)


# ---------------------------------------------------------------------------------------- the cases

@dataclass(frozen=True, eq=False)
class Case:
    name: str
    data: bytes
    layout: Tuple[int, int, int]      # the call's (width, height, colour type)
    n_frames: int                     # what the probe counts
    want: Optional[np.ndarray]        # the model's pixels of the frames that stand, uint8 [n, H, W, 3]
    accept: bool = True
    expect: Optional[int] = None      # the refused frame's code (or the file's, when it has no frame)
    bad_frame: Optional[int] = None   # the first refused frame
    pillow: bool = True               # Pillow yields exactly the frames that stand here


# Refused cases where Pillow yields another number of frames than stand here, with the reason.
OUTSIDE_PILLOW = {
    "first_smaller": "Pillow decodes an fcTL in front of IDAT that is smaller than the canvas; the specification and "
                     "this decoder refuse it",
    "other_canvas": "a matter of the call, not of the file",
}


def px(seed, rect_or_hw, ct, smooth=True):
    h, w = (rect_or_hw[3], rect_or_hw[2]) if len(rect_or_hw) == 4 else rect_or_hw
    p = PC.pixels(seed, h, w, ct, smooth=smooth).copy()
    if ct in (4, 6):   # every kind of alpha in every frame: clear, opaque and in between
        a = np.random.default_rng(seed + 1000).integers(0, 256, (h, w))
        a[::3, ::2] = 0
        a[1::3, 1::2] = 255
        p[..., -1] = a
    return p


def full(seed, canvas, ct, **kw):
    return Spec((0, 0, canvas[0], canvas[1]), px(seed, (canvas[1], canvas[0]), ct), **kw)


def sub(seed, rect, ct, **kw):
    return Spec(rect, px(seed, rect, ct), **kw)


RECTS_37 = [(0, 0, 10, 8), (27, 21, 10, 8), (5, 5, 1, 1), (12, 3, 1, 20), (0, 0, 37, 29), (3, 2, 30, 25)]
BIG_37 = (2, 1, 33, 27)


def ops_frames(ct, canvas=(37, 29)):
    """A whole first frame, then each disposal followed by each blend: the frame that disposes takes the rectangles
    at the corner, flush with the far edges, 1 x 1, one column wide, the whole canvas; the frame that blends covers
    nearly everything.  Sub-rectangle frames take every filter type."""
    frames = [full(10 * ct, canvas, ct)]
    k = 0
    for dispose in (NONE, BACKGROUND, PREVIOUS):
        for blend in (SOURCE, OVER):
            frames.append(sub(100 + 10 * ct + k, RECTS_37[k % 6], ct, dispose=dispose, blend=(OVER, SOURCE)[k % 2],
                              filters=(k % 5,)))
            frames.append(sub(200 + 10 * ct + k, BIG_37, ct, blend=blend, filters=((k + 3) % 5, (k + 1) % 5)))
            k += 1
    return frames


def blend_table():
    r, c = np.mgrid[0:256, 0:256]
    first = np.stack([255 - c, (7 * c + 3 * r) % 256, ((r + c) % 2) * 255, np.full_like(c, 255)], -1).astype(np.uint8)
    second = np.stack([c, c, c, r], -1).astype(np.uint8)
    return [Spec((0, 0, 256, 256), first), Spec((0, 0, 256, 256), second, blend=OVER)]


def _accepted(name, canvas, ct, frames, default=None, trns=None, declared=None, n_frames=None):
    data = assemble(chunks(canvas, ct, frames, default, trns, declared))
    want = model(canvas, ct, frames, default, trns)
    n = len(want) if n_frames is None else n_frames
    return Case(name, data, (canvas[0], canvas[1], ct), n, want[:n])


def _refused(name, canvas, ct, frames, chs, expect, bad, n_frames=None, layout=None, pillow=True, trns=None):
    want = model(canvas, ct, frames, trns=trns)[:bad] if frames else None
    n = len(frames) if n_frames is None else n_frames
    return Case(name, assemble(chs), layout or (canvas[0], canvas[1], ct), n, want, False, expect, bad,
                pillow and name not in OUTSIDE_PILLOW)


@lru_cache(maxsize=1)
def cases():
    out = []
    C37 = (37, 29)
    for ct in (0, 2, 4, 6):
        out.append(_accepted(f"ops_ct{ct}", C37, ct, ops_frames(ct)))
    out.append(_accepted("prev_first", C37, 6, [full(1, C37, 6, dispose=PREVIOUS, blend=OVER),
                                                sub(2, (4, 3, 20, 15), 6, blend=OVER),
                                                sub(3, BIG_37, 6, blend=OVER)]))
    out.append(_accepted("prev_twice", C37, 6, [full(4, C37, 6), sub(5, (3, 3, 20, 12), 6, dispose=PREVIOUS),
                                                sub(6, (10, 8, 20, 12), 6, dispose=PREVIOUS, blend=OVER),
                                                sub(7, (0, 0, 5, 29), 6, blend=OVER)]))
    clear = np.zeros((12, 20, 4), np.uint8)
    clear[..., :3] = 200
    out.append(_accepted("bg_over_alpha0", C37, 6, [full(8, C37, 6), sub(9, (3, 3, 20, 12), 6, dispose=BACKGROUND),
                                                    Spec((3, 3, 20, 12), clear, blend=OVER)]))
    out.append(_accepted("unknown_ops", C37, 6, [full(11, C37, 6), sub(12, (3, 3, 20, 12), 6, dispose=3, blend=2),
                                                 sub(13, BIG_37, 6, blend=OVER)]))
    key = (17, 34, 51)
    keyed = px(14, BIG_37, 2)
    keyed[::2, 1::3] = key
    out.append(_accepted("rgb_trns_over", C37, 2, [full(15, C37, 2), Spec(BIG_37, keyed, blend=OVER, dispose=PREVIOUS),
                                                   Spec(BIG_37, keyed[::-1].copy(), blend=SOURCE)], trns=key))
    grey = px(16, BIG_37, 0)
    grey[::2, 1::3] = 99
    out.append(_accepted("grey_trns_over", C37, 0, [full(17, C37, 0), Spec(BIG_37, grey, blend=OVER)], trns=99))
    out.append(_accepted("default_image", C37, 6, [sub(18, (4, 3, 20, 15), 6, blend=OVER, dispose=PREVIOUS),
                                                   sub(19, BIG_37, 6, blend=OVER), sub(20, (0, 0, 37, 29), 6)],
                         default=full(21, C37, 6)))
    out.append(_accepted("split_chunks", C37, 6, [full(22, C37, 6, split=[0, 1, 2, 0, 700, 1]),
                                                  sub(23, BIG_37, 6, blend=OVER, split=[0, 3, 0, 0, 500]),
                                                  sub(24, (5, 5, 1, 1), 6, split=1),
                                                  sub(25, BIG_37, 6, split=[-4, 2])]))
    out.append(_accepted("declares_more", C37, 6, [full(26, C37, 6), sub(27, BIG_37, 6, blend=OVER),
                                                   sub(28, (1, 1, 9, 9), 6)], declared=5))
    out.append(_accepted("declares_fewer", C37, 6, [full(29, C37, 6), sub(30, BIG_37, 6, blend=OVER),
                                                    sub(31, (1, 1, 9, 9), 6), sub(32, (1, 1, 9, 9), 6)],
                         declared=2, n_frames=2))
    fr = [full(33, C37, 6), sub(34, BIG_37, 6, blend=OVER)]
    chs = chunks(C37, 6, fr)
    chs.insert(nth(chs, b"IDAT", 0) + 1, chs.pop(nth(chs, b"acTL", 0)))   # acTL behind IDAT: a still
    out.append(Case("actl_after_idat", assemble(chs), (37, 29, 6), 1, model(C37, 6, fr[:1])))
    still = full(35, C37, 2)
    out.append(Case("still", PC.simple(still.px, 2, idat=300), (37, 29, 2), 1, model(C37, 2, [still])))
    rows = PC.filter_rows(px(36, BIG_37, 6), PC.CYCLE)
    cut = Spec(BIG_37, px(36, BIG_37, 6), blend=OVER, stream=PC.zwrap(IC.deflate(rows, 6), rows, trailer=2))
    out.append(_accepted("partial_trailer", C37, 6, [full(37, C37, 6), cut]))
    # two unfilter bands: an 80-row first frame, a 9 x 70 rectangle, every filter type in it
    C80 = (40, 80)
    out.append(_accepted("bands", C80, 6, [full(38, C80, 6),
                                           sub(39, (31, 10, 9, 70), 6, blend=OVER, filters=(4, 3, 1, 2, 0)),
                                           sub(40, (0, 5, 9, 70), 6, dispose=PREVIOUS, filters=(3,)),
                                           sub(41, (20, 0, 1, 80), 6, blend=OVER, filters=(4,))]))
    out.append(_accepted("canvas_1x1", (1, 1), 6, [full(42, (1, 1), 6, dispose=BACKGROUND),
                                                   full(43, (1, 1), 6, blend=OVER, dispose=PREVIOUS),
                                                   full(44, (1, 1), 6, blend=OVER)]))
    out.append(_accepted("blend_table", (256, 256), 6, blend_table()))

    # ---- refused
    def four(seed):
        return [full(seed, C37, 6), sub(seed + 1, BIG_37, 6, blend=OVER), sub(seed + 2, (4, 3, 20, 15), 6, blend=OVER),
                sub(seed + 3, (1, 1, 9, 9), 6)]
    fr = four(50)
    chs = chunks(C37, 6, fr)
    i = nth(chs, b"fdAT", 1)   # frame 2's data
    chs[i][1] = struct.pack(">I", 9) + chs[i][1][4:]
    out.append(_refused("seq_fdat", C37, 6, fr, chs, ERR_IO, 2))
    chs = chunks(C37, 6, fr)
    i = nth(chs, b"fcTL", 1)
    chs[i][1] = struct.pack(">I", 7) + chs[i][1][4:]
    out.append(_refused("seq_fctl", C37, 6, fr, chs, ERR_IO, 1))
    chs = chunks(C37, 6, fr)
    del chs[nth(chs, b"fdAT", 1)]
    out.append(_refused("fctl_no_data", C37, 6, fr, renumber(chs), ERR_IO, 2))
    chs = chunks(C37, 6, fr)
    i = nth(chs, b"fcTL", 2)
    chs[i][1] = fctl(0, (18, 3, 20, 15), NONE, OVER)   # 18 + 20 > 37
    out.append(_refused("rect_outside", C37, 6, fr, renumber(chs), ERR_BOUNDS, 2))
    chs = chunks(C37, 6, fr)
    i = nth(chs, b"fcTL", 2)
    chs[i][1] = fctl(0, (4, 3, 0, 15), NONE, OVER)
    out.append(_refused("rect_zero", C37, 6, fr, renumber(chs), ERR_BOUNDS, 2))
    small = [sub(54, (0, 0, 30, 29), 6), sub(55, (1, 1, 9, 9), 6)]
    out.append(_refused("first_smaller", C37, 6, small, chunks(C37, 6, small), ERR_BOUNDS, 0))
    bad = list(fr)
    bad[2] = Spec(fr[2].rect, fr[2].px, blend=OVER, stream=PC.zwrap(b"\x07" + bytes(40), b""))   # block type 3
    out.append(_refused("corrupt_deflate", C37, 6, fr, chunks(C37, 6, bad), ERR_IO, 2))
    rows = PC.filter_rows(fr[1].px, PC.CYCLE)
    bad = list(fr)
    bad[1] = Spec(fr[1].rect, fr[1].px, blend=OVER,
                  stream=PC.zwrap(IC.deflate(rows, 6), rows, adler=zlib.adler32(rows) ^ 1))
    out.append(_refused("wrong_adler", C37, 6, fr, chunks(C37, 6, bad), ERR_IO, 1))
    bad = list(fr)
    bad[1] = Spec(fr[1].rect, fr[1].px, blend=OVER, filters=(1, 5))
    out.append(_refused("filter_5", C37, 6, fr, chunks(C37, 6, bad), ERR_IO, 1))
    whole = assemble(chunks(C37, 6, fr))
    chs = chunks(C37, 6, fr)
    at = len(assemble(chs[:nth(chs, b"fdAT", 1)])) + 8 + 40   # inside frame 2's data
    out.append(Case("truncated", whole[:at], (37, 29, 6), 3, model(C37, 6, fr)[:2], False, ERR_IO, 2))
    other = [full(60, (21, 16), 6), sub(61, (1, 1, 9, 9), 6, blend=OVER)]
    out.append(_refused("other_canvas", (21, 16), 6, None, chunks((21, 16), 6, other), ERR_SHAPE, 0, n_frames=2,
                        layout=(37, 29, 6)))
    for name, kw, ct, code in (("interlaced", dict(lace=1), 6, ERR_INTERLACED),
                               ("depth16", dict(depth=16), 6, ERR_BITDEPTH), ("palette", {}, 3, ERR_PALETTE)):
        out.append(_refused(name, C37, ct, None, chunks(C37, ct, fr, **kw), code, 0, n_frames=0, layout=(37, 29, 6)))
    out.append(Case("not_png", b"GIF89a" + bytes(40), (37, 29, 6), 0, None, False, ERR_IO, 0))
    out.append(Case("empty_file", b"", (37, 29, 6), 0, None, False, ERR_IO, 0))
    assert len({c.name for c in out}) == len(out)
    return out


def by_name():
    return {c.name: c for c in cases()}


def by_layout():
    """{layout: [cases]} in first-seen order: one decode call per layout takes good and refused files together."""
    groups = {}
    for c in cases():
        groups.setdefault(c.layout, []).append(c)
    return groups


pack = PC.pack


# ------------------------------------------------------------------------------------------ the C calls

def host_probe_mem(data, off, size, threads=2):
    """vge_apng_probe_mem -> (return code, int64 [n, 10] rows as vge.frames.apng_probe gives them)."""
    from vge import lib as L
    from vge.frames import _apng_rows
    n = len(off)
    info = (L.ApngInfo * max(n, 1))()
    rc = L.load().vge_apng_probe_mem(IC._ptr(data), data.size, IC._ptr(off), IC._ptr(size), n, threads, info)
    return rc, _apng_rows(info, n)


def host_decode_mem(data, off, size, layout, cap, threads=2, fill=0x5A):
    """vge_apng_decode_mem -> (return code, uint8 [cap, H, W, 3], status [cap], file status [n], frames of all files)."""
    import ctypes as C

    from vge import lib as L
    w, h, ct = layout
    n = len(off)
    rgb, st = np.full((max(cap, 1), h, w, 3), fill, np.uint8), np.zeros(max(cap, 1), np.int32)
    fst, total = np.full(max(n, 1), -1, np.int32), C.c_int64(-1)
    rc = L.load().vge_apng_decode_mem(IC._ptr(data), data.size, IC._ptr(off), IC._ptr(size), n, threads, w, h, ct, cap,
                                      IC._ptr(rgb), IC._ptr(st), IC._ptr(fst), C.byref(total))
    return rc, rgb[:cap], st[:cap], fst[:n], total.value


def host_plan_mem(data, off, size, layout, threads=2, desc_cap=None, seg_cap=None):
    """vge_apng_plan_mem -> (return code, descs, n_descs, segs, n_segs, status [n_descs], file status [n], workspace
    bytes); capacities None: counted by a first call without arrays."""
    import ctypes as C

    from vge import lib as L
    lib = L.load()
    w, h, ct = layout
    n = len(off)
    nd, ns, ws = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    head = (IC._ptr(data), data.size, IC._ptr(off), IC._ptr(size), n, threads, w, h, ct)
    lib.vge_apng_plan_mem(*head, None, 0, C.byref(nd), None, 0, C.byref(ns), None, None, None)
    desc_cap = nd.value if desc_cap is None else desc_cap
    seg_cap = ns.value if seg_cap is None else seg_cap
    descs = (L.ApngDesc * max(desc_cap, 1))()
    segs = (L.ApngSegment * max(seg_cap, 1))()
    st, fst = np.full(max(desc_cap, 1), -1, np.int32), np.full(max(n, 1), -1, np.int32)
    rc = lib.vge_apng_plan_mem(*head, descs, desc_cap, C.byref(nd), segs, seg_cap, C.byref(ns), IC._ptr(st),
                               IC._ptr(fst), C.byref(ws))
    return rc, descs, nd.value, segs, ns.value, st[:max(nd.value, 0)][:desc_cap], fst[:n], ws.value
