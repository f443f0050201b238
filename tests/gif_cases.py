"""GIF files for the GIF front end's tests (include/vge_gif.h), built from seeds in memory by a writer in plain Python:
an LZW encoder with the switches a writer has (clear when the dictionary is full, or never: the "deferred clear";
a clear code every N codes; a "trivial" mode that clears before the width ever grows), a packer that takes any code
list as given (for broken streams), a free sub-block size and free frame descriptors.

  cases()   every file the host and device decoders are tested on: Case(name, data, screen, accept, ...)
            screen    (width, height) the decode call is made with
            accept    what the case was built to be: True every frame accepted, False some frame refused
            bad_frame the first refused frame of a refused case (the frames before it stand); None: no frame stands
            expect    the status of the refused frames (VGE_GIF_ERR_IO unless the case names another)
            pillow    False: the case is outside the equality with Pillow (OUTSIDE_PILLOW lists them by name)
Every case is at most 96 x 80 and 8 frames."""
import io
import struct
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np

ERR_ARG, ERR_IO, ERR_SHAPE, ERR_NO_PALETTE, ERR_BOUNDS = 1, 7, 8, 40, 41
TABLE = 4096


# ------------------------------------------------------------------------------------------ LZW

def code_width(mcs: int, since: int) -> int:
    """The width of the code read when `since` codes were read since the last clear code: the first adds no entry,
    every later one adds one; the width grows when the next free entry reaches a power of two, up to 12."""
    nxt = min(TABLE, (1 << mcs) + 1 + max(since, 1))
    return min(12, max(mcs + 1, nxt.bit_length()))


def lzw_encode(indices, mcs: int, full="clear", clear_every=None, trivial=False, lead_clear=True, end=True):
    """Colour indices -> a code list.  full: "clear" emits a clear code once the dictionary is full, "defer" goes on
    with 12-bit codes and adds nothing.  clear_every: a clear code after every N data codes.  trivial: plain indices
    only, and a clear code before the width would grow."""
    clear, eoi = 1 << mcs, (1 << mcs) + 1
    idx = [int(v) for v in np.asarray(indices).ravel()]
    assert idx and max(idx) < clear
    codes = [clear] if lead_clear else []
    if trivial:
        room = max(1, clear - 2)   # data codes after a clear code before the next free entry reaches 2 * clear
        for k, v in enumerate(idx):
            if k and k % room == 0:
                codes.append(clear)
            codes.append(v)
        return codes + ([eoi] if end else [])
    table, since, cur = {}, 0, idx[0]
    for v in idx[1:]:
        if (cur, v) in table:
            cur = table[(cur, v)]
            continue
        codes.append(cur)
        entry = clear + 2 + since   # the entry the decoder adds when it meets the next code
        since += 1
        if entry < TABLE:
            table[(cur, v)] = entry
        if (entry >= TABLE - 1 and full == "clear") or (clear_every and since % clear_every == 0):
            codes.append(clear)
            table, since = {}, 0
        cur = v
    codes.append(cur)
    return codes + ([eoi] if end else [])


def pack_codes(codes, mcs: int, widths=None) -> bytes:
    """Any code list, packed as given, least significant bit first; the widths follow the decoder's schedule (a clear
    code restarts it) unless they are given."""
    clear = 1 << mcs
    acc, nbits, out, since = 0, 0, bytearray(), 0
    for k, c in enumerate(codes):
        w = widths[k] if widths is not None else code_width(mcs, since)
        acc |= (int(c) & ((1 << w) - 1)) << nbits
        nbits += w
        since = 0 if c == clear else since + 1
        while nbits >= 8:
            out.append(acc & 255)
            acc >>= 8
            nbits -= 8
    if nbits:
        out.append(acc & 255)
    return bytes(out)


def sub_blocks(data: bytes, size=255, terminator=True) -> bytes:
    out = bytearray()
    for i in range(0, len(data), size):
        part = data[i:i + size]
        out.append(len(part))
        out += part
    return bytes(out) + (b"\x00" if terminator else b"")


# ------------------------------------------------------------------------------------------ the container

def palette(seed: int, n: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)


def _table_bits(n: int) -> int:
    assert n in (2, 4, 8, 16, 32, 64, 128, 256)
    return n.bit_length() - 2


INTERLACE_PASSES = ((0, 8), (4, 8), (2, 4), (1, 2))


def interlace_order(h: int):
    return [r for start, step in INTERLACE_PASSES for r in range(start, h, step)]


def gce(disposal=0, transparent=None, delay=0) -> bytes:
    flags = (disposal << 2) | (1 if transparent is not None else 0)
    return b"\x21\xf9\x04" + struct.pack("<BHB", flags, delay, transparent if transparent is not None else 0) + b"\x00"


def frame(rect, indices=None, lct=None, interlace=False, mcs=None, disposal=None, transparent=None, block=255,
          stream=None, terminator=True, **enc) -> bytes:
    """One frame: an optional graphic control extension (when disposal or transparent is given), the image descriptor,
    an optional local table, and the LZW data -- of `indices` ([h, w]), or `stream` (packed bytes) as given."""
    x, y, w, h = rect
    out = bytearray()
    if disposal is not None or transparent is not None:
        out += gce(disposal or 0, transparent)
    flags = (0x80 | _table_bits(len(lct)) if lct is not None else 0) | (0x40 if interlace else 0)
    out += b"\x2c" + struct.pack("<HHHHB", x, y, w, h, flags)
    if lct is not None:
        out += np.asarray(lct, np.uint8).tobytes()
    if stream is None:
        idx = np.asarray(indices).reshape(h, w)
        if interlace:
            idx = idx[interlace_order(h)]
        if mcs is None:
            mcs = max(2, int(idx.max()).bit_length())
        stream = pack_codes(lzw_encode(idx, mcs, **enc), mcs)
    out.append(mcs)
    out += sub_blocks(stream, block, terminator)
    return bytes(out)


def gif(screen, frames, gct=None, bg=0, version=b"GIF89a", trailer=True, before=b"") -> bytes:
    w, h = screen
    flags = (0x80 | _table_bits(len(gct)) | 0x70) if gct is not None else 0x70
    out = version + struct.pack("<HHBBB", w, h, flags, bg, 0)
    if gct is not None:
        out += np.asarray(gct, np.uint8).tobytes()
    return out + before + b"".join(frames) + (b"\x3b" if trailer else b"")


COMMENT = b"\x21\xfe\x05hello\x00"
NETSCAPE = b"\x21\xff\x0bNETSCAPE2.0\x03\x01\x00\x00\x00"
PLAIN_TEXT = b"\x21\x01\x0c" + bytes(12) + b"\x02hi\x00"


@dataclass(frozen=True)
class Case:
    name: str
    data: bytes
    screen: Tuple[int, int]
    accept: bool
    bad_frame: Optional[int] = None
    expect: int = ERR_IO
    pillow: bool = True


# the cases outside the equality with Pillow: only our documented status is asserted for them
OUTSIDE_PILLOW = ("no_palette", "bounds", "code_size_0", "code_size_1", "code_size_9", "cut_in_global_table",
                  "cut_in_local_table", "cut_in_header")


def _rand(seed, h, w, n):
    return np.random.default_rng(seed).integers(0, n, (h, w), dtype=np.uint8)


def _de_bruijn_pairs():
    """Disposal methods 0..3 in an order in which every adjacent pair (a, b) occurs: 17 frames."""
    seq, seen = [0], set()

    def walk(a):
        for b in range(4):
            if (a, b) not in seen:
                seen.add((a, b))
                walk(b)
                seq.append(b)
    walk(0)
    seq = seq[::-1]
    assert len(seq) == 17 and len({(seq[i], seq[i + 1]) for i in range(16)}) == 16
    return seq


@lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, data, screen, accept=True, bad_frame=None, expect=ERR_IO):
        out.append(Case(name, data, screen, accept, bad_frame, expect, name not in OUTSIDE_PILLOW))

    # ---- LZW
    S = (96, 80)
    full = (0, 0, 96, 80)
    g256 = palette(1, 256)
    noise = _rand(2, 80, 96, 256)
    for mode in ("clear", "defer"):
        codes = lzw_encode(noise, 8, full=mode)
        assert len(codes) > 3850   # more codes than the dictionary has free entries: it fills
        assert (codes.count(256) > 1) == (mode == "clear")
        add(f"lzw_noise_{mode}", gif(S, [frame(full, noise, mcs=8, full=mode)], g256), S)
    flat = np.full((80, 96), 7, np.uint8)
    add("lzw_flat", gif(S, [frame(full, flat, mcs=8)], g256), S)   # KwKwK runs and the longest strings
    for mcs in (2, 3, 5, 6, 7, 8):   # 6, 7 and 8: the width grows on the last lane of a 64-code batch
        add(f"lzw_mcs{mcs}", gif((40, 30), [frame((0, 0, 40, 30), _rand(10 + mcs, 30, 40, 1 << mcs), mcs=mcs)],
                                 palette(3, 1 << mcs)), (40, 30))
    add("lzw_two_colours", gif((40, 30), [frame((0, 0, 40, 30), _rand(4, 30, 40, 2), mcs=2)], palette(5, 2)), (40, 30))
    for every in (63, 64, 65, 1):   # a clear code as the last and as the first code of a 64-code batch
        add(f"lzw_clear_every_{every}", gif((40, 30), [frame((0, 0, 40, 30), _rand(6, 30, 40, 200), mcs=8,
                                                             clear_every=every)], g256), (40, 30))
    add("lzw_trivial", gif((40, 30), [frame((0, 0, 40, 30), _rand(7, 30, 40, 16), mcs=4, trivial=True)],
                           palette(8, 16)), (40, 30))
    smooth = ((np.mgrid[0:30, 0:40][0] // 3 + np.mgrid[0:30, 0:40][1] // 5) % 32).astype(np.uint8)
    for block in (255, 1, 7):   # codes straddle sub-blocks
        add(f"lzw_block_{block}", gif((40, 30), [frame((0, 0, 40, 30), smooth, mcs=5, block=block)], palette(9, 32)),
            (40, 30))
    add("lzw_no_lead_clear", gif((40, 30), [frame((0, 0, 40, 30), smooth, mcs=5, lead_clear=False)], palette(9, 32)),
        (40, 30))
    base = lzw_encode(smooth, 5)
    add("lzw_extra_codes", gif((40, 30), [frame((0, 0, 40, 30), mcs=5, stream=pack_codes(
        base[:-1] + [3, 4, 5, 4095, 7], 5))], palette(9, 32)), (40, 30))
    add("lzw_no_end_code", gif((40, 30), [frame((0, 0, 40, 30), smooth, mcs=5, end=False)], palette(9, 32)), (40, 30))
    add("lzw_no_trailer", gif((40, 30), [frame((0, 0, 40, 30), smooth, mcs=5)], palette(9, 32), trailer=False),
        (40, 30))
    add("lzw_no_terminator", gif((40, 30), [frame((0, 0, 40, 30), smooth, mcs=5, terminator=False)], palette(9, 32),
                                 trailer=False), (40, 30))
    add("gif87a", gif((40, 30), [frame((0, 0, 40, 30), smooth, mcs=5)], palette(9, 32), version=b"GIF87a"), (40, 30))
    add("extensions", gif((40, 30), [COMMENT + frame((0, 0, 40, 30), smooth, mcs=5, disposal=1), PLAIN_TEXT +
                                     frame((3, 3, 5, 5), _rand(1, 5, 5, 32), mcs=5)], palette(9, 32),
                          before=NETSCAPE), (40, 30))

    # ---- composition
    C = (12, 10)
    g16 = palette(20, 16)
    l4 = palette(21, 4)
    rng = np.random.default_rng(22)

    def rnd_rect(W, H):
        w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        return int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h

    def rnd_frame(rect, n, **kw):
        return frame(rect, rng.integers(0, n, (rect[3], rect[2])), **kw)

    rects = [(0, 0, 12, 10), (5, 4, 1, 1), (0, 2, 4, 5), (8, 3, 4, 6), (2, 0, 7, 3), (3, 7, 6, 3)]
    add("rects", gif(C, [rnd_frame(r, 16, mcs=4, disposal=1, transparent=3) for r in rects], g16), C)
    for h in (1, 3, 4, 5, 9, 80):
        scr = (7, h)
        add(f"interlace_h{h}", gif(scr, [rnd_frame((0, 0, 7, h), 16, mcs=4, interlace=True),
                                         rnd_frame((1, 0, 5, h), 16, mcs=4, interlace=True, transparent=2)], g16), scr)
    for n in (2, 4, 16, 256):
        add(f"table_{n}", gif(C, [rnd_frame((0, 0, 12, 10), n), rnd_frame(rnd_rect(*C), n, lct=palette(30 + n, n))],
                              palette(31 + n, n)), C)
    add("local_after_global", gif(C, [rnd_frame((0, 0, 12, 10), 16, mcs=4), rnd_frame(rnd_rect(*C), 4, lct=l4),
                                      rnd_frame(rnd_rect(*C), 16, mcs=4)], g16), C)
    add("global_after_local", gif(C, [rnd_frame((0, 0, 12, 10), 4, lct=l4), rnd_frame(rnd_rect(*C), 16, mcs=4),
                                      rnd_frame(rnd_rect(*C), 4, lct=l4)], g16), C)
    add("local_only", gif(C, [rnd_frame((0, 0, 12, 10), 4, lct=l4), rnd_frame(rnd_rect(*C), 4, lct=palette(23, 4))]), C)
    seq = _de_bruijn_pairs()
    for fi, chunk in enumerate((seq[0:6], seq[5:11], seq[10:16], seq[13:17])):
        for variant, (tr, first_full) in enumerate(((None, True), (1, True), (1, False))):
            frames = []
            for k, d in enumerate(chunk):
                rect = (0, 0, 12, 10) if (k == 0 and first_full) else rnd_rect(*C)
                kw = dict(mcs=4, lct=l4 if k % 3 == 2 else None)
                if d == 0 and k % 2 == 1 and tr is None:
                    frames.append(rnd_frame(rect, 4, **kw))   # no control extension at all
                else:
                    frames.append(rnd_frame(rect, 4, disposal=d, transparent=tr if k % 4 != 3 else None, **kw))
            add(f"disposal_{fi}_{variant}", gif(C, frames, g16, bg=2), C)
    for tr in (None, 2):
        add(f"method3_first_tr{tr}", gif(C, [rnd_frame((2, 1, 6, 5), 16, mcs=4, disposal=3, transparent=tr),
                                             rnd_frame((4, 3, 7, 6), 16, mcs=4, disposal=1, transparent=1),
                                             rnd_frame((0, 0, 3, 3), 16, mcs=4)], g16), C)
        add(f"method2_first_tr{tr}", gif(C, [rnd_frame((2, 1, 6, 5), 16, mcs=4, disposal=2, transparent=tr),
                                             rnd_frame((4, 3, 7, 6), 16, mcs=4, disposal=2, transparent=1),
                                             rnd_frame((0, 0, 3, 3), 16, mcs=4)], g16, bg=5), C)
    add("transparent_first", gif(C, [rnd_frame((1, 1, 10, 8), 16, mcs=4, transparent=0),
                                     rnd_frame((0, 0, 12, 10), 16, mcs=4, transparent=0)], g16), C)
    add("no_control_extension", gif(C, [rnd_frame((0, 0, 12, 10), 16, mcs=4), rnd_frame((3, 3, 4, 4), 16, mcs=4)],
                                    g16), C)
    # the background index lies beyond a small local table, on frame 0 and on a later frame
    add("background_beyond_first", gif(C, [rnd_frame((2, 2, 5, 5), 4, lct=l4, disposal=2),
                                           rnd_frame((0, 0, 6, 6), 4, lct=l4, transparent=1)], g16, bg=9), C)
    add("background_beyond_later", gif(C, [rnd_frame((0, 0, 12, 10), 16, mcs=4, disposal=1),
                                           rnd_frame((2, 2, 5, 5), 4, lct=l4, disposal=2),
                                           rnd_frame((0, 0, 6, 6), 16, mcs=4, transparent=1)], g16, bg=9), C)
    add("transparent_beyond_table", gif(C, [rnd_frame((2, 2, 5, 5), 4, lct=l4, disposal=2, transparent=200),
                                            rnd_frame((1, 1, 5, 5), 4, lct=l4, disposal=2, transparent=200),
                                            rnd_frame((0, 0, 6, 6), 4, lct=l4)], g16), C)
    # pixel indices beyond the table: code size 4 over a four-entry table
    add("indices_beyond_table", gif(C, [rnd_frame((0, 0, 12, 10), 16, mcs=4, lct=l4),
                                        rnd_frame((1, 1, 9, 7), 16, mcs=4, lct=l4, transparent=9)], g16), C)
    for w in (1, 3, 5, 67):   # RGB stores that do not fill a dword
        scr = (w, 6)
        add(f"width_{w}", gif(scr, [rnd_frame((0, 0, w, 6), 16, mcs=4, disposal=2),
                                    rnd_frame((0, 1, w, 3), 16, mcs=4, transparent=5, disposal=3),
                                    rnd_frame((w - 1, 0, 1, 6), 16, mcs=4)], g16), scr)
    # a batch of three files of 1, 4 and 8 frames
    for n in (1, 4, 8):
        add(f"frames_{n}", gif(C, [rnd_frame((0, 0, 12, 10) if k == 0 else rnd_rect(*C), 16, mcs=4,
                                             disposal=k % 4, transparent=k % 5) for k in range(n)], g16), C)

    # ---- refused
    R = (20, 16)
    pix = [_rand(40 + k, 16, 20, 32) for k in range(4)]
    good = [frame((0, 0, 20, 16), pix[k], mcs=5, disposal=1) for k in range(4)]
    codes = lzw_encode(pix[0], 5)
    half = len(codes) // 2
    assert code_width(5, half) > 6
    beyond = list(codes)
    assert codes.count(32) == 1
    beyond[half] = (1 << _widths(codes, 5)[half]) - 1   # greater than the next free entry there
    assert beyond[half] > 33 + (half - 1) + 1
    broken = {
        "code_beyond": pack_codes(beyond, 5, widths=_widths(codes, 5)),
        "end_at_half": pack_codes(codes[:half] + [33], 5),
        "data_ends_at_half": pack_codes(codes[:half], 5),
        "first_code_not_plain": pack_codes([32, 34] + codes[2:], 5, widths=_widths(codes, 5)),
    }
    for name, stream in broken.items():
        bad = frame((0, 0, 20, 16), mcs=5, stream=stream, disposal=1)
        add(f"{name}_frame0", gif(R, [bad] + good[1:], palette(41, 32)), R, False, None)
        add(f"{name}_frame2", gif(R, good[:2] + [bad] + good[3:], palette(41, 32)), R, False, 2)
    whole = gif(R, good, palette(41, 32))
    add("cut_in_frame2", whole[:13 + 96 + 2 * len(good[0]) + len(good[2]) // 2], R, False, 2)
    add("cut_in_global_table", whole[:13 + 40], R, False, None)
    add("cut_in_header", whole[:9], R, False, None)
    lgood = frame((0, 0, 20, 16), pix[0], mcs=5, lct=palette(42, 32))
    add("cut_in_local_table", gif(R, [good[0]], palette(41, 32))[:-1] + lgood[:10 + 50], R, False, 1)
    add("cut_in_descriptor", gif(R, [good[0]], palette(41, 32))[:-1] + good[1][:8 + 5], R, False, 1)
    for mcs in (0, 1, 9):
        bad = bytearray(good[1])
        at = 8 + 10
        assert bad[at] == 5
        bad[at] = mcs
        add(f"code_size_{mcs}", gif(R, [good[0], bytes(bad), good[2]], palette(41, 32)), R, False, 1)
    add("zero_width_frame", gif(R, [good[0], frame((3, 3, 0, 4), mcs=5, stream=pack_codes([32, 33], 5))],
                                palette(41, 32)), R, False, 1)
    add("no_image", gif(R, [COMMENT], palette(41, 32)), R, False, None)
    add("not_gif", b"\x89PNG\r\n" + whole[6:], R, False, None)
    add("empty_file", b"", R, False, None)
    add("no_palette", gif(R, [frame((0, 0, 20, 16), pix[0], mcs=5, lct=palette(42, 32)),
                              frame((0, 0, 20, 16), pix[1], mcs=5)]), R, False, 1, ERR_NO_PALETTE)
    add("bounds", gif(R, [good[0], frame((5, 5, 16, 4), _rand(1, 4, 16, 32), mcs=5)], palette(41, 32)), R, False, 1,
        ERR_BOUNDS)
    add("other_size", gif((21, 16), [frame((0, 0, 21, 16), _rand(43, 16, 21, 32), mcs=5)], palette(41, 32)), R, False,
        None, ERR_SHAPE)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    assert all(c.screen[0] <= 96 and c.screen[1] <= 80 for c in out)
    return tuple(out)


def _widths(codes, mcs):
    """The widths the unbroken code list was packed with, for a list that is broken in place."""
    clear, since, out = 1 << mcs, 0, []
    for c in codes:
        out.append(code_width(mcs, since))
        since = 0 if c == clear else since + 1
    return out


def mutations(count=300, seed=1234):
    """Single-byte mutations of the case files, from a fixed seed: (case name, position, new byte)."""
    rng = np.random.default_rng(seed)
    pool = [c for c in cases() if len(c.data) > 0]
    out = []
    for _ in range(count):
        c = pool[int(rng.integers(0, len(pool)))]
        out.append((c.name, int(rng.integers(0, len(c.data))), int(rng.integers(0, 256))))
    return out


# ------------------------------------------------------------------------------------------ Pillow

def pillow_frames(data: bytes, n_frames: int):
    """(frames Pillow decodes before it raises, as uint8 [H, W, 3] each; the index of the frame it raised on or None)."""
    from PIL import Image
    frames = []
    try:
        im = Image.open(io.BytesIO(data))
    except Exception:
        return frames, 0
    for k in range(n_frames):
        try:
            im.seek(k)
            frames.append(np.array(im.convert("RGB")))
        except Exception:
            return frames, k
    return frames, None


# ------------------------------------------------------------------------------------------ the C calls

def _ptr(a):
    return a.ctypes.data


def pack(files, gap=0, order=None, fill=0xA5):
    """files -> (buffer uint8, offsets int64 [n], sizes int64 [n]); `gap` bytes of `fill` before, between and after
    the files; order: the order the files are laid in."""
    order = list(range(len(files))) if order is None else order
    off, size = np.zeros(len(files), np.int64), np.zeros(len(files), np.int64)
    pos = gap
    for j in order:
        off[j], size[j] = pos, len(files[j])
        pos += len(files[j]) + gap
    data = np.full(max(pos, 1), fill, np.uint8)
    for j, b in enumerate(files):
        data[off[j]:off[j] + len(b)] = np.frombuffer(b, np.uint8)
    return data, off, size


def host_probe_mem(data, off, size, threads=2):
    """vge_gif_probe_mem -> (return code, int64 [n, 6] rows as vge.frames.gif_probe gives them)."""
    from vge import lib as L
    from vge.frames import _gif_rows
    n = len(off)
    info = (L.GifInfo * max(n, 1))()
    rc = L.load().vge_gif_probe_mem(_ptr(data), data.size, _ptr(off), _ptr(size), n, threads, info)
    return rc, _gif_rows(info, n)


def host_decode_mem(data, off, size, screen, frame_cap, threads=2, fill=0x5A):
    """vge_gif_decode_mem -> (return code, uint8 [frame_cap, H, W, 3], status [frame_cap], file status [n], frames)."""
    import ctypes as C

    from vge import lib as L
    w, h = screen
    n = len(off)
    rgb, st = np.full((max(frame_cap, 1), h, w, 3), fill, np.uint8), np.full(max(frame_cap, 1), -1, np.int32)
    fst, total = np.full(max(n, 1), -1, np.int32), C.c_int64(-1)
    rc = L.load().vge_gif_decode_mem(_ptr(data), data.size, _ptr(off), _ptr(size), n, threads, w, h, frame_cap,
                                     _ptr(rgb), _ptr(st), _ptr(fst), C.byref(total))
    return rc, rgb[:frame_cap], st[:frame_cap], fst[:n], total.value


def host_plan_mem(data, off, size, screen, threads=2, desc_cap=None, seg_cap=None):
    """vge_gif_plan_mem -> (return code, descs, n_descs, segs, n_segs, status [n_descs], file status [n], workspace
    bytes); a capacity of None is counted by a first call without buffers."""
    import ctypes as C

    from vge import lib as L
    lib = L.load()
    w, h = screen
    n = len(off)
    nd, ns, ws = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    fst = np.full(max(n, 1), -1, np.int32)
    head = (_ptr(data), data.size, _ptr(off), _ptr(size), n, threads, w, h)
    if desc_cap is None or seg_cap is None:
        lib.vge_gif_plan_mem(*head, None, 0, C.byref(nd), None, 0, C.byref(ns), None, None, None)
        desc_cap = nd.value if desc_cap is None else desc_cap
        seg_cap = ns.value if seg_cap is None else seg_cap
    descs = (L.GifDesc * max(desc_cap, 1))()
    segs = (L.GifSegment * max(seg_cap, 1))()
    st = np.full(max(desc_cap, 1), -1, np.int32)
    rc = lib.vge_gif_plan_mem(*head, descs, desc_cap, C.byref(nd), segs, seg_cap, C.byref(ns), _ptr(st), _ptr(fst),
                              C.byref(ws))
    return rc, descs, nd.value, segs, ns.value, st[:max(nd.value, 0)], fst[:n], ws.value


def by_screen():
    """{screen: [cases]} in first-seen order: one decode call per screen takes good and refused files together."""
    groups = {}
    for c in cases():
        groups.setdefault(c.screen, []).append(c)
    return groups
