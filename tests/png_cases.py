"""PNG files for the PNG front end's tests (include/vge_png.h), built from seeds in memory: a writer in a few lines
(struct, zlib.crc32, a filter function for the five filter types, free IDAT splitting) on top of tests/inflate_cases.py,
whose bit writer builds the deflate streams zlib will not emit.

  cases()   every file the host and device decoders are tested on: Case(name, data, layout, accept, expect)
            layout   (width, height, colour type) the decode call is made with
            accept   what the case was built to be: True accepted, False refused
            expect   None: the status follows from the verdict (0 or VGE_PNG_ERR_IO), which the host test takes from
                     Pillow at test time; an int: the status the decoders must give (shape, unsupported kinds), where
                     Pillow's verdict says nothing
No case has corrupt bytes after the count inside its deflate stream: that class is outside the equality of host and
device (include/vge_png.h), so it is left out here by construction."""
import struct
import zlib
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np

from tests import inflate_cases as IC

SIG = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}
ERR_IO, ERR_SHAPE, ERR_INTERLACED, ERR_BITDEPTH, ERR_PALETTE = 7, 8, 30, 31, 32
CYCLE = (4, 3, 2, 1, 0)


def chunk(typ: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + typ + data + struct.pack(">I", zlib.crc32(typ + data))


def ihdr(w, h, ct, depth=8, lace=0) -> bytes:
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ct, 0, 0, lace))


def filter_rows(px: np.ndarray, filters) -> bytes:
    """px uint8 [H, W, C] -> the filtered rows; row y takes filter type filters[y % len(filters)]."""
    H, W, Cn = px.shape
    rows = px.reshape(H, W * Cn).astype(np.int32)
    out = bytearray()
    zero = np.zeros(W * Cn, np.int32)
    for y in range(H):
        f = filters[y % len(filters)]
        cur, b = rows[y], rows[y - 1] if y else zero
        a = np.concatenate([zero[:Cn], cur[:-Cn]]) if W * Cn > Cn else zero[:W * Cn]
        c = np.concatenate([zero[:Cn], b[:-Cn]]) if W * Cn > Cn else zero[:W * Cn]
        if f == 4:
            p = a + b - c
            pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        else:
            pred = (zero, a, b, (a + b) >> 1)[f] if f < 4 else zero   # an invalid type filters as None
        out.append(f)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def zwrap(raw: bytes, filtered: bytes, cmf=0x78, fdict=False, fcheck_off=0, adler=None, trailer=4) -> bytes:
    """A raw deflate stream -> a zlib stream: header (FLG chosen so that FCHECK holds, then moved by fcheck_off), the
    stream, and the first `trailer` bytes of Adler-32(filtered) (or of `adler`)."""
    flg = 0x20 if fdict else 0
    flg += (31 - (cmf * 256 + flg) % 31) % 31
    a = zlib.adler32(filtered) if adler is None else adler
    return bytes([cmf, (flg + fcheck_off) & 255]) + raw + struct.pack(">I", a)[:trailer]


def split(stream: bytes, how):
    """IDAT payloads: None one chunk; an int k: a cut every k bytes; a list: those sizes in turn, then the rest."""
    if how is None:
        return [stream]
    if isinstance(how, int):
        return [stream[i:i + how] for i in range(0, len(stream), how)]
    out, at = [], 0
    for n in how:
        n = len(stream) - at + n if n < 0 else n   # a negative size: up to that many bytes before the end
        out.append(stream[at:at + n])
        at += n
    return out + [stream[at:]]


def png(w, h, ct, zstream: bytes, idat=None, before=b"", iend=True, depth=8, lace=0) -> bytes:
    body = b"".join(chunk(b"IDAT", p) for p in split(zstream, idat))
    return SIG + ihdr(w, h, ct, depth, lace) + before + body + (chunk(b"IEND", b"") if iend else b"")


def pixels(seed: int, h: int, w: int, ct: int, smooth=False) -> np.ndarray:
    rng = np.random.default_rng(seed)
    Cn = CHANNELS[ct]
    if not smooth:
        return rng.integers(0, 256, (h, w, Cn), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(3 * x + y) % 256, (x + 2 * y) % 256, (x * y // 7) % 256, (255 - x) % 256], -1)[..., :Cn]
    return ((base + rng.integers(0, 6, (h, w, Cn))) % 256).astype(np.uint8)


def simple(px: np.ndarray, ct: int, filters=CYCLE, level=6, idat=None, **kw) -> bytes:
    """The file zlib and this writer give for the pixels."""
    h, w = px.shape[:2]
    f = filter_rows(px, filters)
    return png(w, h, ct, zwrap(IC.deflate(f, level), f), idat, **kw)


@dataclass(frozen=True)
class Case:
    name: str
    data: bytes
    layout: Tuple[int, int, int]
    accept: bool
    expect: Optional[int] = None


def _ring_stream():
    """300 x 40 RGB (36,040 filtered bytes): 32 KiB in stored blocks, then matches of length 258 at distance 32768 --
    the far end of the window, so that the ring wraps -- and literals for the rest.  Every byte is 0..4, so whatever
    byte a row starts on is a filter type."""
    w, h = 300, 40
    total = h * (1 + 3 * w)
    rng = np.random.default_rng(11)
    head = rng.integers(0, 5, 32768, dtype=np.uint8).tobytes()
    bw = IC.BitWriter()
    IC.stored_block(bw, head[:30000])
    IC.stored_block(bw, head[30000:])
    n_match = (total - 32768) // 258
    tail = total - 32768 - 258 * n_match
    IC.fixed_block(bw, [(258, 32768)] * n_match + [int(v) for v in head[258 * n_match:258 * n_match + tail]], final=True)
    raw = bw.bytes()
    info = IC.inflate(raw)
    assert len(info.out) == total and info.max_dist == 32768 and info.max_len == 258 and total > 32768 + 258
    assert zlib.decompressobj(-15).decompress(raw) == info.out
    return w, h, raw, info.out


def _switch_stream(px, ct):
    """Fixed, dynamic and stored blocks, and a fixed block again, inside the first row; zlib for the others."""
    h, w = px.shape[:2]
    f = filter_rows(px, CYCLE)
    row = 1 + w * CHANNELS[ct]
    q = row // 4
    assert q >= 2
    ll = [9] * 256 + [1]   # a complete code: 256 literals of 9 bits and the end-of-block code of 1 bit
    bw = IC.BitWriter()
    IC.fixed_block(bw, list(f[:q]))
    IC.dynamic_block(bw, list(f[q:2 * q]), ll, [1, 1])
    IC.stored_block(bw, f[2 * q:3 * q])
    IC.fixed_block(bw, list(f[3 * q:row - 1]))
    IC.stored_block(bw, b"")   # ends on a byte boundary, where zlib's own blocks can follow
    raw = bw.bytes() + IC.deflate(f[row - 1:], 6)
    info = IC.inflate(raw)
    assert info.out == f and [b[0] for b in info.blocks][:5] == [1, 2, 0, 1, 0] and info.blocks[4][1] < row
    return raw, f


def _bit_flip(stream: bytes, count: int) -> bytes:
    """One flipped bit in the middle third of the zlib stream, chosen so that zlib rejects the stream."""
    for at in range(len(stream) // 3, 2 * len(stream) // 3):
        bad = stream[:at] + bytes([stream[at] ^ 0x10]) + stream[at + 1:]
        try:
            zlib.decompressobj().decompress(bad, count + 1)
        except zlib.error:
            return bad
    raise AssertionError("no bit flip in the middle of the stream makes zlib reject it")


@lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, data, layout, accept, expect=None):
        out.append(Case(name, data, layout, accept, expect))

    # the grid: every colour type, sizes around the lane count, every filter type and their cycle, IDAT cut every 7 bytes
    for ct in (0, 2, 4, 6):
        for w, h in ((1, 1), (1, 5), (2, 3), (3, 2), (64, 3), (65, 6), (257, 5)):
            for fi, filters in enumerate([(0,), (1,), (2,), (3,), (4,), CYCLE]):
                px = pixels(100 * ct + fi, h, w, ct)
                add(f"grid_ct{ct}_{w}x{h}_f{fi}", simple(px, ct, filters, idat=7), (w, h, ct), True)
    # the unfilter band boundary: Average and Paeth rows that need the carried row (alpha included)
    for ct in (2, 6):
        for h in (63, 64, 65, 129):
            for fi, filters in (("avg", (3,)), ("paeth", (4,)), ("cycle", (2, 4, 0, 3, 1))):
                add(f"band_ct{ct}_h{h}_{fi}", simple(pixels(7 * h + ct, h, 5, ct), ct, filters), (5, h, ct), True)
    # filtered sizes 2, 3, 3 and 4 bytes: the last partial dword
    add("tail_grey_1x1", simple(pixels(1, 1, 1, 0), 0), (1, 1, 0), True)
    add("tail_greyalpha_1x1", simple(pixels(2, 1, 1, 4), 4), (1, 1, 4), True)
    add("tail_grey_2x1", simple(pixels(3, 1, 2, 0), 0), (2, 1, 0), True)
    add("tail_rgb_1x1", simple(pixels(4, 1, 1, 2), 2), (1, 1, 2), True)

    # one base frame, written in every way a writer may write it and broken in every way a file may break
    W, H, CT = 13, 7, 2
    L = (W, H, CT)
    px = pixels(5, H, W, CT, smooth=True)
    f = filter_rows(px, CYCLE)
    z = zwrap(IC.deflate(f, 6), f)
    add("idat_one", png(W, H, CT, z), L, True)
    add("idat_bytes", png(W, H, CT, z, idat=1), L, True)
    add("idat_empty_first", png(W, H, CT, z, idat=[0]), L, True)
    add("idat_cut_in_header", png(W, H, CT, z, idat=[1]), L, True)
    add("idat_cut_in_trailer", png(W, H, CT, z, idat=[-2]), L, True)
    big = pixels(6, 48, 64, CT, smooth=True)
    for level in (0, 1, 6, 9):
        add(f"level{level}", simple(big, CT, (0, 1, 2, 3, 4, 4, 1), level), (64, 48, CT), True)
    rw, rh, rraw, rf = _ring_stream()
    add("ring_wrap", png(rw, rh, 2, zwrap(rraw, rf), idat=8192), (rw, rh, 2), True)
    sraw, sf = _switch_stream(px, CT)
    add("block_switch", png(W, H, CT, zwrap(sraw, sf)), L, True)
    try:
        import io

        from PIL import Image
        nat = pixels(8, 256, 256, 2, smooth=True)
        buf = io.BytesIO()
        Image.fromarray(nat, "RGB").save(buf, "PNG")
        add("pillow_256", buf.getvalue(), (256, 256, 2), True)
    except ImportError:
        pass
    more = f + bytes(range(40))
    add("stream_goes_on", png(W, H, CT, zwrap(IC.deflate(more, 6), more)), L, True)
    add("junk_after_trailer", png(W, H, CT, z + b"\x00\xff" * 9), L, True)
    add("no_trailer", png(W, H, CT, z[:-4]), L, True)
    add("half_trailer", png(W, H, CT, z[:-2]), L, True)
    add("no_iend", png(W, H, CT, z, iend=False), L, True)
    add("ancillary", png(W, H, CT, z, before=chunk(b"gAMA", struct.pack(">I", 45455)) +
                         chunk(b"tRNS", struct.pack(">HHH", 1, 2, 3))), L, True)
    add("window_256", png(W, H, CT, zwrap(IC.deflate(f, 6), f, cmf=0x08)), L, True)

    add("bad_adler", png(W, H, CT, zwrap(IC.deflate(f, 6), f, adler=zlib.adler32(f) ^ 1)), L, False)
    add("fdict", png(W, H, CT, zwrap(IC.deflate(f, 6), f, fdict=True)), L, False)
    add("bad_fcheck", png(W, H, CT, zwrap(IC.deflate(f, 6), f, fcheck_off=1)), L, False)
    add("cm_not_8", png(W, H, CT, zwrap(IC.deflate(f, 6), f, cmf=0x77)), L, False)
    add("bit_flip", png(W, H, CT, _bit_flip(z, len(f))), L, False)
    for row in (0, H - 1):
        g = bytearray(f)
        g[row * (1 + 3 * W)] = 5
        g = bytes(g)
        add(f"filter5_row{row}", png(W, H, CT, zwrap(IC.deflate(g, 6), g)), L, False)
    short = f[:-10]
    add("ten_short", png(W, H, CT, zwrap(IC.deflate(short, 6), short)), L, False)
    whole = png(W, H, CT, z)
    add("cut_in_idat", whole[:len(SIG) + 25 + 8 + len(z) // 2], L, False)
    add("no_idat", SIG + ihdr(W, H, CT) + chunk(b"IEND", b""), L, False)
    add("width_0", SIG + ihdr(0, H, CT) + chunk(b"IDAT", z) + chunk(b"IEND", b""), L, False)
    add("not_png", b"\xff\xd8\xff\xe0" + whole[4:], L, False)
    add("empty_file", b"", L, False)
    add("interlaced", png(W, H, CT, z, lace=1), L, False, ERR_INTERLACED)
    add("sixteen_bit", png(W, H, CT, z, depth=16), L, False, ERR_BITDEPTH)
    add("palette", png(W, H, 3, z, before=chunk(b"PLTE", bytes(range(48)))), L, False, ERR_PALETTE)
    add("other_size", simple(pixels(9, H, W + 1, CT), CT), L, False, ERR_SHAPE)
    add("other_colour_type", simple(pixels(10, H, W, 6), 6), L, False, ERR_SHAPE)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


# ------------------------------------------------------------------------------------------ the C calls

def host_probe_mem(data, off, size, threads=2):
    """vge_png_probe_mem -> (return code, int64 [n, 8] rows as vge.frames.png_probe gives them)."""
    from vge import lib as L
    from vge.frames import _png_rows
    n = len(off)
    info = (L.PngInfo * max(n, 1))()
    rc = L.load().vge_png_probe_mem(IC._ptr(data), data.size, IC._ptr(off), IC._ptr(size), n, threads, info)
    return rc, _png_rows(info, n)


def host_decode_mem(data, off, size, layout, threads=2, fill=0x5A):
    """vge_png_decode_mem -> (return code, uint8 [n, H, W, 3] (rows of failed frames are unspecified), status [n])."""
    from vge import lib as L
    w, h, ct = layout
    n = len(off)
    rgb, st = np.full((n, h, w, 3), fill, np.uint8), np.full(n, -1, np.int32)
    rc = L.load().vge_png_decode_mem(IC._ptr(data), data.size, IC._ptr(off), IC._ptr(size), n, threads, w, h, ct,
                                     IC._ptr(rgb), IC._ptr(st))
    return rc, rgb, st


def host_plan_mem(data, off, size, layout, threads=2, seg_cap=None):
    """vge_png_plan_mem -> (return code, descs, segs, n_segs, status [n], workspace bytes); seg_cap None: counted by a
    first call without segments."""
    import ctypes as C

    from vge import lib as L
    lib = L.load()
    w, h, ct = layout
    n = len(off)
    descs = (L.PngDesc * max(n, 1))()
    st = np.full(n, -1, np.int32)
    n_segs, ws = C.c_int64(-1), C.c_int64(-1)
    head = (IC._ptr(data), data.size, IC._ptr(off), IC._ptr(size), n, threads, w, h, ct, descs)
    if seg_cap is None:
        lib.vge_png_plan_mem(*head, None, 0, C.byref(n_segs), IC._ptr(st), None)
        seg_cap = n_segs.value
    segs = (L.PngSegment * max(seg_cap, 1))()
    rc = lib.vge_png_plan_mem(*head, segs, seg_cap, C.byref(n_segs), IC._ptr(st), C.byref(ws))
    return rc, descs, segs, n_segs.value, st, ws.value


def by_layout():
    """{layout: [cases]} in first-seen order: one decode call per layout takes good and refused frames together."""
    groups = {}
    for c in cases():
        groups.setdefault(c.layout, []).append(c)
    return groups


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
