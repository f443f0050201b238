"""Lossless WebP test files for tests/test_webp_host.py and tests/test_webp_gpu.py: a VP8L bit writer of our own that can
force every feature of the format (each predictor mode, each transform, tile sizes, colour-cache sizes, one and many
prefix-code groups, both code-length forms with their corner cases, every distance-map code, long, overlapping and far
copies, every palette bundling), a RIFF container writer (still, VP8X still, animation), Pillow-written files, files
the decoders must refuse, and seeded byte mutations.  Nothing is larger than 256 x 256."""
import functools
import heapq
import io
import struct

import numpy as np

ERR_ARG, ERR_IO, ERR_SHAPE, ERR_LOSSY, ERR_BOUNDS, ERR_GROUPS = 1, 7, 8, 50, 51, 52
MAX_GROUPS = 256

# the host decoder's coverage bits (csrc/vge_webp_vp8l.h F_*)
F_PRED0, F_XFORM0 = 0, 14
(F_SIMPLE1, F_SIMPLE2, F_ZERO_BIT, F_NORMAL, F_MAX_SYMBOL, F_REP16, F_REP16_FIRST, F_REP17, F_REP18, F_CACHE,
 F_CACHE_SUB, F_META, F_COPY, F_DIST_MAP, F_DIST_PLAIN, F_DIST_CLAMP, F_MANY_GROUPS, F_BUNDLE8, F_BUNDLE4, F_BUNDLE2,
 F_INDEX_OOB, F_COPY_OVERLAP, F_COPY_FAR, F_CACHE_HIT, F_TRAILING, F_ALL_XFORMS) = range(18, 44)

PREDICTOR, CROSS, GREEN, INDEX = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------ bits and prefix codes

class Bits:
    """An LSB-first bit sink."""
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value: int, nbits: int):
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.acc |= value << self.n
        self.n += nbits

    def bytes(self) -> bytes:
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def huff_lengths(freq: dict, limit: int = 15) -> dict:
    """{symbol: count} -> {symbol: code length}; two or more symbols give a complete code of at most `limit` bits."""
    syms = sorted(freq)
    if len(syms) <= 1:
        return {s: 1 for s in syms}
    f = {s: max(int(freq[s]), 1) for s in syms}
    while True:
        heap = [(c, i, (s,)) for i, (s, c) in enumerate(sorted(f.items()))]
        heapq.heapify(heap)
        depth = {s: 0 for s in syms}
        tick = len(heap)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2]))
            tick += 1
        if max(depth.values()) <= limit:
            return depth
        f = {s: (c + 1) // 2 for s, c in f.items()}   # flatten and try again


def canonical(lengths: dict) -> dict:
    """{symbol: length} -> {symbol: (bit-reversed code, length)}: codes in (length, symbol) order, as deflate's."""
    out, code, prev = {}, 0, 0
    for s in sorted(lengths, key=lambda s: (lengths[s], s)):
        n = lengths[s]
        code <<= n - prev
        prev = n
        out[s] = (int(format(code, "0%db" % n)[::-1], 2), n)
        code += 1
    return out


CL_ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)


def length_tokens(arr, rle: bool):
    """Code lengths -> [(token, extra bits, extra value)] with or without the repeat codes 16 / 17 / 18."""
    if not rle:
        return [(v, 0, 0) for v in arr]
    out, i, prev = [], 0, 8
    while i < len(arr):
        v, j = arr[i], i
        while j < len(arr) and arr[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 3:
                n = min(run, 138)
                out.append((17, 3, n - 3) if n <= 10 else (18, 7, n - 11))
                run -= n
            out += [(0, 0, 0)] * run
        else:
            if v != prev:
                out.append((v, 0, 0))
                run -= 1
                prev = v
            while run >= 3:
                n = min(run, 6)
                out.append((16, 2, n - 3))
                run -= n
            out += [(v, 0, 0)] * run
        i = j
    return out


def write_normal_code(b: Bits, arr, rle=True, max_symbol=False):
    """The normal form: the code-length code, an optional max_symbol, then the lengths' tokens."""
    tokens = length_tokens(list(arr), rle)
    if max_symbol:
        while len(tokens) > 2 and tokens[-1][0] in (0, 17, 18):
            tokens.pop()
    freq = {}
    for t, _, _ in tokens:
        freq[t] = freq.get(t, 0) + 1
    cl = huff_lengths(freq, 7)
    codes = canonical(cl) if len(cl) > 1 else {}
    b.put(0, 1)
    num = max(4, 1 + max(CL_ORDER.index(t) for t in cl))
    b.put(num - 4, 4)
    for t in CL_ORDER[:num]:
        b.put(cl.get(t, 0), 3)
    if max_symbol:
        n = len(tokens)
        k = 0
        while (n - 2) >> (2 + 2 * k):
            k += 1
        b.put(1, 1)
        b.put(k, 3)
        b.put(n - 2, 2 + 2 * k)
    else:
        b.put(0, 1)
    for t, nb, ev in tokens:
        if codes:
            b.put(*codes[t])
        b.put(ev, nb)


def write_plain_lengths(b: Bits, arr):
    """The normal form with a fixed code-length code (lengths 0..15 at 4 bits each, no repeats): any set of lengths,
    valid or not, goes through as it is."""
    b.put(0, 1)
    b.put(19 - 4, 4)
    for t in CL_ORDER:
        b.put(4 if t < 16 else 0, 3)
    b.put(0, 1)
    codes = canonical({t: 4 for t in range(16)})
    for v in arr:
        b.put(*codes[v])


def write_code(b: Bits, lengths: dict, alphabet: int, opts: dict):
    """One prefix code in the smallest form the options allow.  Returns the symbols' codes ({} for a zero-bit code)."""
    if not lengths:
        lengths = {0: 1}
    syms = sorted(lengths)
    if len(syms) <= 2 and syms[-1] < 256 and not opts.get("no_simple"):
        b.put(1, 1)
        b.put(len(syms) - 1, 1)
        if syms[0] < 2:
            b.put(0, 1)
            b.put(syms[0], 1)
        else:
            b.put(1, 1)
            b.put(syms[0], 8)
        if len(syms) == 2:
            b.put(syms[1], 8)
    else:
        arr = [lengths.get(s, 0) for s in range(alphabet)]
        write_normal_code(b, arr, rle=opts.get("rle", True), max_symbol=opts.get("max_symbol", False))
    return canonical(lengths) if len(syms) > 1 else {}


def lz_prefix(v: int):
    """A length or distance value (>= 1) -> (prefix symbol, extra bits, extra value)."""
    if v <= 4:
        return v - 1, 0, 0
    d = v - 1
    hb = d.bit_length() - 1
    extra = hb - 1
    return 2 * hb + ((d >> (hb - 1)) & 1), extra, d & ((1 << extra) - 1)


# the 120 (dx, dy) neighbours of the short distance codes, from the format's table
DIST_MAP = [(0, 1), (1, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (1, 2), (-1, 2), (2, 1), (-2, 1), (2, 2), (-2, 2), (0, 3),
            (3, 0), (1, 3), (-1, 3), (3, 1), (-3, 1), (2, 3), (-2, 3), (3, 2), (-3, 2), (0, 4), (4, 0), (1, 4), (-1, 4),
            (4, 1), (-4, 1), (3, 3), (-3, 3), (2, 4), (-2, 4), (4, 2), (-4, 2), (0, 5), (3, 4), (-3, 4), (4, 3), (-4, 3),
            (5, 0), (1, 5), (-1, 5), (5, 1), (-5, 1), (2, 5), (-2, 5), (5, 2), (-5, 2), (4, 4), (-4, 4), (3, 5), (-3, 5),
            (5, 3), (-5, 3), (0, 6), (6, 0), (1, 6), (-1, 6), (6, 1), (-6, 1), (2, 6), (-2, 6), (6, 2), (-6, 2), (4, 5),
            (-4, 5), (5, 4), (-5, 4), (3, 6), (-3, 6), (6, 3), (-6, 3), (0, 7), (7, 0), (1, 7), (-1, 7), (5, 5), (-5, 5),
            (7, 1), (-7, 1), (4, 6), (-4, 6), (6, 4), (-6, 4), (2, 7), (-2, 7), (7, 2), (-7, 2), (3, 7), (-3, 7), (7, 3),
            (-7, 3), (5, 6), (-5, 6), (6, 5), (-6, 5), (8, 0), (4, 7), (-4, 7), (7, 4), (-7, 4), (8, 1), (8, 2), (6, 6),
            (-6, 6), (8, 3), (5, 7), (-5, 7), (7, 5), (-7, 5), (8, 4), (6, 7), (-6, 7), (7, 6), (-7, 6), (8, 5), (7, 7),
            (-7, 7), (8, 6), (8, 7)]


def map_code_distance(code: int, width: int) -> int:
    dx, dy = DIST_MAP[code - 1]
    return max(dx + dy * width, 1)


def cache_key(argb: int, bits: int) -> int:
    return ((0x1e35a7bd * argb) & 0xffffffff) >> (32 - bits)


# ------------------------------------------------------------------------------------------ the entropy-coded image

def tokens_from_pixels(px, width: int, cache_bits: int = 0, lz: bool = False):
    """Pixels -> tokens ("lit", argb) | ("copy", length, distance code) | ("cache", key): cache hits where the cache
    holds the pixel, and with lz greedy copies from the pixel before and the row above."""
    px = [int(v) for v in px]
    cache = {} if cache_bits else None
    out, i, n = [], 0, len(px)

    def insert(v):
        if cache is not None:
            cache[cache_key(v, cache_bits)] = v

    while i < n:
        best, best_d = 0, 0
        if lz:
            for d in (1, width):
                if d <= i:
                    m = 0
                    while i + m < n and m < 4096 and px[i + m] == px[i + m - d]:
                        m += 1
                    if m > best:
                        best, best_d = m, d
        if best >= 3:
            out.append(("copy", best, best_d + 120))
            for k in range(best):
                insert(px[i + k])
            i += best
            continue
        v = px[i]
        if cache is not None and cache.get(cache_key(v, cache_bits)) == v:
            out.append(("cache", cache_key(v, cache_bits)))
        else:
            out.append(("lit", v))
        insert(v)
        i += 1
    return out


def pixels_from_tokens(tokens, width: int, cache_bits: int = 0):
    """What a decoder makes of the tokens (used to build images from explicit token lists)."""
    px, cache = [], {}

    def push(v):
        px.append(v)
        if cache_bits:
            cache[cache_key(v, cache_bits)] = v

    for t in tokens:
        if t[0] == "lit":
            push(t[1])
        elif t[0] == "cache":
            push(cache.get(t[1], 0))
        else:
            d = map_code_distance(t[2], width) if t[2] <= 120 else t[2] - 120
            assert d <= len(px)
            for _ in range(t[1]):
                push(px[len(px) - d])
    return px


def token_span(t) -> int:
    return t[1] if t[0] == "copy" else 1


def write_image(b: Bits, tokens, width: int, cache_bits: int, groups=None, meta_bits: int = 0, n_groups: int = 1,
                opts=None):
    """The groups' codes, then the tokens.  groups: the entropy image [tiles_y, tiles_x] of group indices, or None."""
    opts = opts or {}
    alphabets = (280 + ((1 << cache_bits) if cache_bits else 0), 256, 256, 256, 40)
    freq = [[{} for _ in range(5)] for _ in range(n_groups)]
    coded, pos = [], 0
    for t in tokens:
        g = int(groups[(pos // width) >> meta_bits, (pos % width) >> meta_bits]) if groups is not None else 0
        if t[0] == "lit":
            v = t[1]
            syms = [(0, (v >> 8) & 255), (1, (v >> 16) & 255), (2, v & 255), (3, v >> 24)]
            extra = []
        elif t[0] == "cache":
            syms, extra = [(0, 280 + t[1])], []
        else:
            ls, lb, lv = lz_prefix(t[1])
            ds, db, dv = lz_prefix(t[2])
            syms, extra = [(0, 256 + ls), (4, ds)], [(lv, lb), (dv, db)]
        for a, s in syms:
            freq[g][a][s] = freq[g][a].get(s, 0) + 1
        coded.append((g, syms, extra))
        pos += token_span(t)
    codes = []
    for g in range(n_groups):
        row = []
        for a in range(5):
            o = dict(opts)
            if isinstance(opts.get("no_simple"), (set, tuple, list)):
                o["no_simple"] = a in opts["no_simple"]
            writer = opts.get("raw_code", {}).get((g, a))
            if writer is not None:
                writer(b)
                row.append(canonical(huff_lengths(freq[g][a])) if len(freq[g][a]) > 1 else {})
            else:
                row.append(write_code(b, huff_lengths(freq[g][a]), alphabets[a], o))
        codes.append(row)
    for g, syms, extra in coded:
        for k, (a, s) in enumerate(syms):
            if codes[g][a]:
                b.put(*codes[g][a][s])
            if extra:
                b.put(extra[k][0], extra[k][1])


def write_sub_image(b: Bits, px, width: int, cache_bits: int = 0, opts=None):
    """A sub-image: its colour-cache bits, one group's codes, the pixels; no transforms and no entropy image."""
    if cache_bits:
        b.put(1, 1)
        b.put(cache_bits, 4)
    else:
        b.put(0, 1)
    write_image(b, tokens_from_pixels(px, width, cache_bits), width, cache_bits, opts=opts)


# ------------------------------------------------------------------------------------------ forward transforms

def _ch(a, s):
    return ((a >> np.uint32(s)) & np.uint32(0xff)).astype(np.int32)


def _join(chs):
    out = np.zeros(chs[0].shape, np.uint32)
    for k, c in enumerate(chs):
        out |= (c.astype(np.uint32) & np.uint32(0xff)) << np.uint32(8 * k)
    return out


def _avg2(a, b):
    return (((a ^ b) & np.uint32(0xfefefefe)) >> np.uint32(1)) + (a & b)


def predictions(flat, w: int, modes):
    """The prediction of every pixel of an image (flat uint32 ARGB) from its true neighbours; modes: per pixel."""
    L, T, TL, TR = np.roll(flat, 1), np.roll(flat, w), np.roll(flat, w + 1), np.roll(flat, w - 1)
    cl = lambda v: np.clip(v, 0, 255)   # noqa: E731
    sel = sum(np.abs(_ch(L, s) - _ch(TL, s)) - np.abs(_ch(T, s) - _ch(TL, s)) for s in (0, 8, 16, 24))
    a7 = _avg2(L, T)
    table = [np.full(flat.shape, 0xff000000, np.uint32), L, T, TR, TL, _avg2(_avg2(L, TR), T), _avg2(L, TL), a7,
             _avg2(TL, T), _avg2(T, TR), _avg2(_avg2(L, TL), _avg2(T, TR)), np.where(sel <= 0, T, L),
             _join([cl(_ch(L, s) + _ch(T, s) - _ch(TL, s)) for s in (0, 8, 16, 24)]),
             _join([cl(_ch(a7, s) + np.trunc((_ch(a7, s) - _ch(TL, s)) / 2).astype(np.int32)) for s in (0, 8, 16, 24)])]
    table += [table[0], table[0]]
    pred = np.choose(modes, table)
    n = flat.size
    x, y = np.arange(n) % w, np.arange(n) // w
    pred = np.where(y == 0, L, np.where(x == 0, T, pred))
    pred[0] = 0xff000000
    return pred.astype(np.uint32)


def sub_pixels(a, b):
    return _join([_ch(a, s) - _ch(b, s) for s in (0, 8, 16, 24)])


def tile_expand(tiles, bits: int, w: int, h: int):
    return np.repeat(np.repeat(tiles, 1 << bits, 0), 1 << bits, 1)[:h, :w].ravel()


def _i8(v):
    return ((v.astype(np.int32) + 128) & 255) - 128


def sub_size(v: int, bits: int) -> int:
    return (v + (1 << bits) - 1) >> bits


# ------------------------------------------------------------------------------------------ the VP8L stream

def vp8l(argb, transforms=(), cache_bits=0, lz=False, meta_bits=0, groups=None, opts=None, tokens=None, alpha=None,
         version=0, signature=0x2f, trailing=b"", header_size=None):
    """An image (uint32 ARGB [h, w]) -> a VP8L payload.  transforms, in stream order:
    (PREDICTOR, bits, modes [tiles_y, tiles_x] or an int[, sub-image cache bits]), (CROSS, bits, multipliers uint32
    [tiles_y, tiles_x]), (GREEN,), (INDEX, palette [n] uint32, indices [h, w] or None to look the pixels up).
    tokens: an explicit token list for the coded image in place of the tokeniser (no transforms then).
    groups: the entropy image of group indices, [tiles_y, tiles_x] for meta_bits."""
    argb = np.asarray(argb, np.uint32)
    h, w = argb.shape
    b = Bits()
    hw, hh = header_size or (w, h)
    b.put(signature, 8)
    b.put(hw - 1, 14)
    b.put(hh - 1, 14)
    b.put(int(bool((argb >> 24 != 255).any())) if alpha is None else alpha, 1)
    b.put(version, 3)
    cur, cw = argb.copy(), w
    for t in transforms:
        b.put(1, 1)
        b.put(t[0], 2)
        if t[0] == PREDICTOR:
            bits = t[1]
            ty, tx = sub_size(h, bits), sub_size(cw, bits)
            modes = np.full((ty, tx), t[2], np.int64) if np.isscalar(t[2]) else np.asarray(t[2], np.int64)
            assert modes.shape == (ty, tx)
            b.put(bits - 2, 3)
            write_sub_image(b, (0xff000000 | (modes.ravel() << 8)).astype(np.uint32), tx,
                            t[3] if len(t) > 3 else 0, opts)
            flat = cur.ravel()
            cur = sub_pixels(flat, predictions(flat, cw, tile_expand(modes, bits, cw, h))).reshape(h, cw)
        elif t[0] == CROSS:
            bits = t[1]
            ty, tx = sub_size(h, bits), sub_size(cw, bits)
            m = np.asarray(t[2], np.uint32)
            assert m.shape == (ty, tx)
            b.put(bits - 2, 3)
            write_sub_image(b, (0xff000000 | m.ravel()).astype(np.uint32), tx, 0, opts)
            mm = tile_expand(m, bits, cw, h)
            flat = cur.ravel()
            g, r, bl = _i8(_ch(flat, 8)), _ch(flat, 16), _ch(flat, 0)
            nr = r - ((_i8(_ch(mm, 0)) * g) >> 5)
            nb = bl - ((_i8(_ch(mm, 8)) * g) >> 5) - ((_i8(_ch(mm, 16)) * _i8(r)) >> 5)
            cur = ((flat & np.uint32(0xff00ff00)) | ((nr & 255).astype(np.uint32) << np.uint32(16)) |
                   (nb & 255).astype(np.uint32)).reshape(h, cw)
        elif t[0] == GREEN:
            flat = cur.ravel()
            g = _ch(flat, 8)
            cur = ((flat & np.uint32(0xff00ff00)) | (((_ch(flat, 16) - g) & 255).astype(np.uint32) << np.uint32(16)) |
                   ((_ch(flat, 0) - g) & 255).astype(np.uint32)).reshape(h, cw)
        else:
            pal = np.asarray(t[1], np.uint32)
            n = len(pal)
            idx = t[2]
            if idx is None:
                look = {int(v): k for k, v in reversed(list(enumerate(pal)))}
                idx = np.array([look[int(v)] for v in cur.ravel()]).reshape(h, cw)
            idx = np.asarray(idx, np.uint32)
            bits = 0 if n > 16 else 1 if n > 4 else 2 if n > 2 else 3
            b.put(n - 1, 8)
            delta = pal.copy()
            delta[1:] = sub_pixels(pal[1:], pal[:-1])
            write_sub_image(b, delta, n, 0, opts)
            per, bpp = 1 << bits, 8 >> bits
            bw = sub_size(cw, bits)
            packed = np.zeros((h, bw), np.uint32)
            for x in range(cw):
                packed[:, x >> bits] |= idx[:, x] << np.uint32((x & (per - 1)) * bpp)
            cur, cw = (np.uint32(0xff000000) | (packed << np.uint32(8))), bw
    b.put(0, 1)
    if cache_bits:
        b.put(1, 1)
        b.put(cache_bits, 4)
    else:
        b.put(0, 1)
    n_groups = 1
    if meta_bits:
        groups = np.asarray(groups, np.int64)
        assert groups.shape == (sub_size(h, meta_bits), sub_size(cw, meta_bits))
        n_groups = int(groups.max()) + 1
        b.put(1, 1)
        b.put(meta_bits - 2, 3)
        write_sub_image(b, (((groups.ravel() >> 8) << 16) | ((groups.ravel() & 255) << 8)).astype(np.uint32),
                        groups.shape[1], 0, opts)
    else:
        b.put(0, 1)
    if tokens is None:
        tokens = tokens_from_pixels(cur.ravel(), cw, cache_bits, lz)
    write_image(b, tokens, cw, cache_bits, groups if meta_bits else None, meta_bits, n_groups, opts)
    return b.bytes() + trailing


# ------------------------------------------------------------------------------------------ the container

def chunk(fourcc: bytes, payload: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def le24(v: int) -> bytes:
    return struct.pack("<I", v)[:3]


def riff(body: bytes, size=None) -> bytes:
    return b"RIFF" + struct.pack("<I", 4 + len(body) if size is None else size) + b"WEBP" + body


def vp8x(w: int, h: int, anim=False, alpha=False) -> bytes:
    return chunk(b"VP8X", bytes([(2 if anim else 0) | (16 if alpha else 0), 0, 0, 0]) + le24(w - 1) + le24(h - 1))


def anmf(x: int, y: int, w: int, h: int, payload: bytes, blend=True, dispose=False, duration=40, inner=b"VP8L",
         before=b"") -> bytes:
    flags = (0 if blend else 2) | (1 if dispose else 0)
    return chunk(b"ANMF", le24(x // 2) + le24(y // 2) + le24(w - 1) + le24(h - 1) + le24(duration) + bytes([flags]) +
                 before + chunk(inner, payload))


def still(payload: bytes) -> bytes:
    return riff(chunk(b"VP8L", payload))


def animation(canvas, frames, alpha=True, before=b"", loop=0) -> bytes:
    return riff(vp8x(canvas[0], canvas[1], anim=True, alpha=alpha) +
                chunk(b"ANIM", struct.pack("<IH", 0xffffffff, loop)) + before + b"".join(frames))


UNKNOWN = chunk(b"ZZZZ", b"odd")   # an unknown chunk of odd size: padded


# ------------------------------------------------------------------------------------------ images

def rgb_to_argb(rgb, alpha=255):
    rgb = np.asarray(rgb, np.uint32)
    a = np.broadcast_to(np.asarray(alpha, np.uint32), rgb.shape[:2])
    return (a << np.uint32(24)) | (rgb[..., 0] << np.uint32(16)) | (rgb[..., 1] << np.uint32(8)) | rgb[..., 2]


def picture(w: int, h: int, seed: int, noise=True):
    """A smooth picture with flat stretches (copies), a noisy patch (literals) and repeated rows."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    rgb = np.stack([(3 * x + 2 * y + 7 * seed) % 256, (x * y // 3 + seed) % 256, (x + 5 * y) % 256], -1).astype(np.uint8)
    if noise and h >= 3 and w >= 3:
        rgb[h // 3:h // 3 + max(h // 4, 1), w // 4:w // 4 + max(w // 3, 1)] = rng.integers(
            0, 256, (max(h // 4, 1), max(w // 3, 1), 3))[:h - h // 3, :w - w // 4]
    if h >= 6:
        rgb[h // 2:h // 2 + 2] = rgb[h // 2 - 1]
    if w >= 12:
        rgb[:, w - 6:] = rgb[:, w - 7:w - 6]
    return rgb


def all_features(rgb, seed=0, alpha=255, cache_bits=4, meta_bits=2, n_groups=3, pbits=2, trailing=b""):
    """A picture through predictor (random modes per tile), cross-colour and subtract-green, with a colour cache,
    copies and several groups: everything at once, for the shapes."""
    rng = np.random.default_rng(seed)
    h, w = rgb.shape[:2]
    modes = rng.integers(0, 14, (sub_size(h, pbits), sub_size(w, pbits)))
    mult = rng.integers(0, 1 << 24, (sub_size(h, 3), sub_size(w, 3))).astype(np.uint32)
    groups = rng.integers(0, n_groups, (sub_size(h, meta_bits), sub_size(w, meta_bits)))
    groups.ravel()[0] = n_groups - 1
    return vp8l(rgb_to_argb(rgb, alpha), [(PREDICTOR, pbits, modes), (CROSS, 3, mult), (GREEN,)], cache_bits=cache_bits,
                lz=True, meta_bits=meta_bits, groups=groups, trailing=trailing)


# ------------------------------------------------------------------------------------------ cases

class Case:
    def __init__(self, name, data, canvas, n_frames, accept=True, expect=0, bad_frame=None):
        self.name, self.data, self.canvas, self.n_frames = name, data, canvas, n_frames
        self.accept, self.expect, self.bad_frame = accept, expect, bad_frame   # bad_frame None: the file has no frames

    def __repr__(self):
        return f"Case({self.name})"


# Cases outside the equality with Pillow, with the reason:
#   groups_257        libwebp has no group capacity; this project's arena has (VGE_WEBP_ERR_GROUPS)
#   bounds, mismatch,
#   lossy_frame_2,    libwebp's demuxer refuses the file when it is opened; this project refuses the frame (and, like
#   unknown_in_anmf,  Pillow, shows no frame of it for a refusal in frame 0) but keeps the earlier frames
#   still_mismatch
#   lossy_still,      Pillow decodes lossy WebP (these two are headers only, which it refuses for their content); this
#   lossy_alpha_still project refuses lossy frames by name (VGE_WEBP_ERR_LOSSY)
OUTSIDE_PILLOW = ("groups_257", "bounds", "mismatch", "lossy_frame_2", "still_mismatch", "unknown_in_anmf",
                  "lossy_still", "lossy_alpha_still")


def have_pillow() -> bool:
    try:
        import PIL  # noqa: F401
        return True
    except ImportError:
        return False


def _pillow_bytes(frames, **kw):
    from PIL import Image
    ims = [Image.fromarray(f) for f in frames]
    bio = io.BytesIO()
    if len(ims) > 1:
        ims[0].save(bio, "WEBP", save_all=True, append_images=ims[1:], lossless=True, duration=40, **kw)
    else:
        ims[0].save(bio, "WEBP", lossless=True, **kw)
    return bio.getvalue()


def _moving(w, h, n, seed, alpha=False):
    base = picture(w, h, seed)
    out = []
    for k in range(n):
        f = base.copy()
        f[2 + 3 * k:2 + 3 * k + h // 3, 3 + 4 * k:3 + 4 * k + w // 3] = picture(w // 3, h // 3, seed + k + 1)
        if alpha:
            a = np.full((h, w, 1), 255, np.uint8)
            a[h // 4:h // 2, 2 * k:2 * k + w // 2] = (0, 70, 160, 255)[k % 4]
            f = np.concatenate([f, a], -1)
        out.append(f)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, data, canvas, n=1, **kw):
        out.append(Case(name, data, canvas, n, **kw))

    rng = np.random.default_rng(5)
    # every predictor mode alone, on a noisy picture (17 x 9, tiles of 4)
    pic = picture(17, 9, 3)
    for m in range(14):
        add(f"pred_{m}", still(vp8l(rgb_to_argb(pic, rng.integers(0, 256, (9, 17))), [(PREDICTOR, 2, m)])), (17, 9))
    add("pred_modes_14_15", still(vp8l(rgb_to_argb(pic), [(PREDICTOR, 2, np.array([[14, 15, 1, 14, 15]] * 3))])), (17, 9))
    # each of the other transforms alone, and tile sizes 2^2 and 2^9
    add("cross", still(vp8l(rgb_to_argb(pic), [(CROSS, 2, rng.integers(0, 1 << 24, (3, 5)))])), (17, 9))
    add("green", still(vp8l(rgb_to_argb(pic), [(GREEN,)])), (17, 9))
    big = picture(64, 66, 4)
    add("tile_512", still(vp8l(rgb_to_argb(big), [(PREDICTOR, 9, 11), (CROSS, 9, [[0x123456]])], lz=True)), (64, 66))
    add("pred_sub_cache", still(vp8l(rgb_to_argb(big), [(PREDICTOR, 2, rng.integers(0, 14, (17, 16)), 3)], lz=True)),
        (64, 66))
    # palettes: 2, 4, 16, 17 and 256 colours at widths that leave bundling remainders, and indices beyond the palette
    for n, w in ((2, 9), (2, 17), (4, 7), (4, 9), (16, 7), (16, 8), (17, 8), (256, 17), (3, 17), (1, 8)):
        pal = rgb_to_argb(rng.integers(0, 256, (1, n, 3)), rng.integers(0, 256, (1, n)))[0]
        idx = rng.integers(0, n, (5, w))
        add(f"index_{n}_w{w}", still(vp8l(np.zeros((5, w), np.uint32), [(INDEX, pal, idx)], alpha=1)), (w, 5))
    pal = rgb_to_argb(rng.integers(0, 256, (1, 3, 3)))[0]
    add("index_oob_3", still(vp8l(np.zeros((5, 9), np.uint32), [(INDEX, pal, rng.integers(0, 4, (5, 9)))], alpha=1)),
        (9, 5))
    pal = rgb_to_argb(rng.integers(0, 256, (1, 17, 3)))[0]
    add("index_oob_17", still(vp8l(np.zeros((5, 9), np.uint32), [(INDEX, pal, rng.integers(0, 256, (5, 9)))], alpha=1)),
        (9, 5))
    # all four together: indices, then predictor, cross-colour and subtract-green on the bundled image
    pal = rgb_to_argb(rng.integers(0, 256, (1, 16, 3)))[0]
    idx = (np.add.outer(np.arange(66), np.arange(64)) // 3 + rng.integers(0, 2, (66, 64))) % 16
    add("all_four", still(vp8l(np.zeros((66, 64), np.uint32),
                               [(INDEX, pal, idx), (PREDICTOR, 2, rng.integers(0, 14, (17, 8))),
                                (CROSS, 3, rng.integers(0, 1 << 24, (9, 4))), (GREEN,)], lz=True, cache_bits=2)),
        (64, 66))
    add("three_rgb", still(vp8l(rgb_to_argb(big), [(GREEN,), (CROSS, 4, rng.integers(0, 1 << 24, (5, 4))),
                                                   (PREDICTOR, 3, rng.integers(0, 14, (9, 8)))], lz=True)), (64, 66))
    # colour cache of 1 and 11 bits, with copies (a copied pixel enters the cache too)
    flat = picture(64, 66, 9, noise=False) // 64 * 64
    add("cache_1", still(vp8l(rgb_to_argb(flat), cache_bits=1, lz=True)), (64, 66))
    add("cache_11", still(vp8l(rgb_to_argb(big), [(GREEN,)], cache_bits=11, lz=True)), (64, 66))
    t = [("lit", 0xff102030), ("lit", 0xff405060), ("copy", 2, 2 + 120), ("cache", cache_key(0xff102030, 3)),
         ("cache", cache_key(0xff405060, 3)), ("cache", 7 if cache_key(0xff102030, 3) != 7 else 6)]
    t += [("copy", 2, 1 + 120)]
    px = pixels_from_tokens(t, 3, 3)
    add("cache_after_copy", still(vp8l(np.array(px, np.uint32).reshape(3, 3), cache_bits=3, tokens=t)), (3, 3))
    # one group and many; a group change inside a row and right after a copy
    groups = (np.add.outer(np.arange(17), np.arange(16)) % 7)
    add("groups_7", still(vp8l(rgb_to_argb(big), [(GREEN,)], lz=True, cache_bits=5, meta_bits=2, groups=groups)),
        (64, 66))
    g = np.zeros((2, 3), np.int64)
    g[0, 1] = MAX_GROUPS - 1
    add("groups_256", still(vp8l(rgb_to_argb(pic), meta_bits=3, groups=g)), (17, 9))
    g[0, 2] = MAX_GROUPS
    add("groups_257", still(vp8l(rgb_to_argb(pic), meta_bits=3, groups=g)), (17, 9), accept=False, expect=ERR_GROUPS,
        bad_frame=0)
    # code forms
    add("one_colour", still(vp8l(np.full((3, 3), 0xff336699, np.uint32))), (3, 3))             # zero-bit codes
    two = np.where(rng.integers(0, 2, (9, 17)) > 0, 0xff00ff00, 0xff000000).astype(np.uint32)
    add("two_symbols", still(vp8l(two)), (17, 9))
    add("two_symbols_normal", still(vp8l(two, opts={"no_simple": True})), (17, 9))
    ramp = rgb_to_argb(np.stack([np.arange(256).reshape(16, 16)] * 3, -1))
    add("rep16_first", still(vp8l(ramp)), (16, 16))                                            # 256 lengths of 8
    add("plain_lengths", still(vp8l(rgb_to_argb(pic), opts={"rle": False})), (17, 9))
    add("max_symbol", still(vp8l(rgb_to_argb(pic) & np.uint32(0xff3f3f3f), opts={"max_symbol": True})), (17, 9))
    # every distance-map code on a width where some clamp to 1 (7) and on one where none does (17)
    for w in (7, 8, 17):
        t = [("lit", int(v)) for v in rgb_to_argb(rng.integers(0, 256, (9, w, 3))).ravel()]
        t += [("copy", 1 + c % 3, c) for c in range(1, 121)]
        px = pixels_from_tokens(t, w)
        t += [("lit", 0xff000000 | k) for k in range(-len(px) % w)]
        px = pixels_from_tokens(t, w)
        add(f"dist_map_w{w}", still(vp8l(np.array(px, np.uint32).reshape(-1, w), tokens=t)), (w, len(px) // w))
    # a copy of distance 1 and length 4096; a copy from 32,800 pixels back; lengths that end exactly at the last pixel
    t = [("lit", 0xffabcdef), ("copy", 4096, 1 + 120), ("lit", 0xff010203), ("copy", 70 * 70 - 4098, 2 + 120)]
    add("copy_4096", still(vp8l(np.array(pixels_from_tokens(t, 70), np.uint32).reshape(70, 70), tokens=t)), (70, 70))
    t = [("lit", int(v)) for v in rgb_to_argb(rng.integers(0, 256, (1, 200, 3))).ravel()]
    while sum(token_span(k) for k in t) < 33000:
        t.append(("copy", 200, 200 + 120))
    t += [("lit", 0xff112233)] * 7 + [("copy", 150, 32800 + 120)]
    t.append(("copy", 200 * 180 - sum(token_span(k) for k in t), 33007 + 120))
    add("copy_far", still(vp8l(np.array(pixels_from_tokens(t, 200), np.uint32).reshape(180, 200), tokens=t)), (200, 180))
    # the smallest shapes that can still go wrong, everything at once
    for w, h in ((1, 1), (1, 70), (70, 1), (3, 3), (7, 5), (8, 5), (9, 5), (17, 5), (20, 65), (20, 130), (64, 66),
                 (200, 180)):
        add(f"shape_{w}x{h}", still(all_features(picture(w, h, w + h), seed=w * h, trailing=b"\x00\x01" * (w & 1))),
            (w, h))
    # containers
    add("vp8x_still", riff(vp8x(17, 9) + chunk(b"ICCP", b"xyz") + chunk(b"VP8L", vp8l(rgb_to_argb(pic))) +
                           chunk(b"EXIF", b"e")), (17, 9))
    add("riff_longer_file", still(vp8l(rgb_to_argb(pic))) + b"trailing bytes", (17, 9))
    cv = (40, 30)

    def fr(x, y, w, h, seed, alpha=255, hint=None, **kw):
        return anmf(x, y, w, h, vp8l(rgb_to_argb(picture(w, h, seed), alpha), [(GREEN,)], lz=True, alpha=hint), **kw)

    soft = rng.integers(0, 256, (30, 40))
    holes = np.where(rng.integers(0, 3, (30, 40)) > 0, 0, 255)
    add("anim_hand", animation(cv, [
        fr(0, 0, 40, 30, 1),
        fr(4, 2, 21, 13, 2, alpha=holes[:13, :21]),                       # odd size on an even offset, blended
        fr(10, 6, 20, 10, 3, blend=False, dispose=True),                  # overwritten, then cleared
        fr(2, 2, 30, 20, 4, alpha=soft[:20, :30]),                        # partial alpha over the cleared rectangle
        fr(0, 0, 40, 30, 5, alpha=soft, dispose=True),                    # a full-canvas frame in the middle
        fr(6, 4, 9, 7, 6, alpha=soft[:7, :9]),                            # after a cleared full frame: a key frame
        fr(0, 0, 40, 30, 7, alpha=holes, hint=0),                         # full frame without the alpha hint
        fr(8, 8, 12, 12, 8, alpha=soft[:12, :12])], before=UNKNOWN + chunk(b"EXIF", b"ab")), cv, 8)
    add("anim_alpha_rules", animation(cv, [
        fr(0, 0, 20, 10, 1, alpha=soft[:10, :20], dispose=True),          # frame 0 smaller than the canvas, cleared
        fr(2, 2, 30, 20, 2, alpha=soft[:20, :30]),                        # previous cleared and was a key frame: key
        fr(0, 0, 40, 30, 3, alpha=soft),                                  # full, blended, with alpha: not a key frame
        fr(0, 0, 40, 30, 4, alpha=soft, blend=False),                     # full, not blended: key
        fr(4, 4, 30, 20, 5, alpha=soft[:20, :30], dispose=True),
        fr(0, 0, 40, 30, 6, alpha=holes)]), cv, 6)                        # blended outside the cleared rectangle only
    # Pillow's own files (tests/golden/webp_golden.npz keeps such files for machines without Pillow)
    if have_pillow():
        add("pil_default", _pillow_bytes([picture(96, 80, 1)]), (96, 80))
        add("pil_m6", _pillow_bytes([picture(96, 80, 2)], method=6, quality=100), (96, 80))
        add("pil_anim", _pillow_bytes(_moving(96, 80, 4, 3)), (96, 80), 4)
        add("pil_anim_min", _pillow_bytes(_moving(96, 80, 4, 4), minimize_size=True), (96, 80), 4)
        add("pil_anim_rgba", _pillow_bytes(_moving(96, 80, 4, 5, alpha=True)), (96, 80), 4)
        add("pil_16_colours", _pillow_bytes([f // 128 * 128 for f in _moving(96, 80, 3, 6)]), (96, 80), 3)

    # ---- refused
    # a lossy key frame's first bytes: frame tag, start code, 14-bit width and height (nothing of it is decoded)
    vp8 = bytes([0x10, 0x02, 0x00, 0x9d, 0x01, 0x2a, 17, 0, 9, 0]) + bytes(range(30))
    add("lossy_still", riff(chunk(b"VP8 ", vp8)), (17, 9), accept=False, expect=ERR_LOSSY, bad_frame=0)
    add("lossy_alpha_still", riff(vp8x(17, 9, alpha=True) + chunk(b"ALPH", bytes(9)) + chunk(b"VP8 ", vp8)), (17, 9),
        accept=False, expect=ERR_LOSSY, bad_frame=0)
    add("lossy_frame_2", animation((17, 9), [fr(0, 0, 17, 9, 1), fr(0, 0, 17, 9, 2),
                                             anmf(0, 0, 17, 9, vp8, inner=b"VP8 "), fr(0, 0, 17, 9, 4)]), (17, 9), 4,
        accept=False, expect=ERR_LOSSY, bad_frame=2)
    add("bounds", animation(cv, [fr(0, 0, 40, 30, 1), fr(22, 0, 20, 10, 2), fr(0, 0, 8, 8, 3)]), cv, 3, accept=False,
        expect=ERR_BOUNDS, bad_frame=1)
    add("mismatch", animation(cv, [fr(0, 0, 40, 30, 1), anmf(0, 0, 10, 10, vp8l(rgb_to_argb(picture(11, 10, 2))))]),
        cv, 2, accept=False, expect=ERR_BOUNDS, bad_frame=1)
    add("unknown_in_anmf", animation(cv, [fr(0, 0, 40, 30, 1), fr(8, 8, 12, 12, 8, before=UNKNOWN)]), cv, 2,
        accept=False, expect=ERR_IO, bad_frame=1)
    add("still_mismatch", riff(vp8x(18, 9) + chunk(b"VP8L", vp8l(rgb_to_argb(pic)))), (18, 9), accept=False,
        expect=ERR_BOUNDS, bad_frame=0)
    good = out[[c.name for c in out].index("anim_hand")].data
    at, cuts = 12, []
    while at < len(good):
        cuts.append(at)
        at += 8 + struct.unpack("<I", good[at + 4:at + 8])[0]
        at += at & 1
    for k, cut in enumerate(cuts[1:] + [cuts[3] + 21, len(good) - 9]):
        add(f"cut_{k}", good[:cut], cv, 0, accept=False, expect=ERR_IO)        # the RIFF size says more: no frame at all
    base = vp8l(rgb_to_argb(big), [(GREEN,)], lz=True)
    for k, keep in enumerate((4, 5, 9, len(base) // 2, len(base) - 1)):
        add(f"stream_ends_{k}", still(base[:keep]), (64, 66) if keep >= 5 else (0, 0), 1, accept=False, expect=ERR_IO,
            bad_frame=0)
    ok_frame = fr(0, 0, 17, 9, 1)
    add("stream_ends_frame_1", animation((17, 9), [ok_frame, anmf(0, 0, 17, 9, vp8l(rgb_to_argb(pic))[:40]), ok_frame]),
        (17, 9), 3, accept=False, expect=ERR_IO, bad_frame=1)

    def bad_code(lengths):
        return {"raw_code": {(0, 1): lambda b: write_plain_lengths(b, lengths + [0] * (256 - len(lengths)))}}

    for name, lengths in (("over_subscribed", [1, 1, 1]), ("incomplete", [1, 2]), ("incomplete_deep", [2, 2, 2, 15]),
                          ("no_symbol", [0])):
        add(name, still(vp8l(two, opts=bad_code(lengths))), (17, 9), accept=False, expect=ERR_IO, bad_frame=0)
    add("one_symbol_length_7", still(vp8l(two, opts=bad_code([0, 0, 7]))), (17, 9))   # any length: the zero-bit code
    add("copy_before_0", still(vp8l(np.zeros((3, 3), np.uint32), tokens=[("lit", 0xff000000), ("copy", 3, 2 + 120)] +
                                    [("lit", 0xff000000)] * 5)), (3, 3), accept=False, expect=ERR_IO, bad_frame=0)
    add("copy_past_end", still(vp8l(np.zeros((3, 3), np.uint32), tokens=[("lit", 0xff000000), ("copy", 9, 1 + 120)])),
        (3, 3), accept=False, expect=ERR_IO, bad_frame=0)
    add("version_1", still(vp8l(rgb_to_argb(pic), version=1)), (0, 0), accept=False, expect=ERR_IO, bad_frame=0)
    add("signature", still(vp8l(rgb_to_argb(pic), signature=0x2e)), (0, 0), accept=False, expect=ERR_IO, bad_frame=0)
    add("cache_bits_12", still(vp8l(rgb_to_argb(pic), cache_bits=12)), (17, 9), accept=False, expect=ERR_IO, bad_frame=0)
    b = Bits()
    for v, n in ((0x2f, 8), (16, 14), (8, 14), (0, 1), (0, 3), (1, 1), (GREEN, 2), (1, 1), (GREEN, 2)):
        b.put(v, n)
    add("transform_twice", still(b.bytes() + bytes(40)), (17, 9), accept=False, expect=ERR_IO, bad_frame=0)
    add("not_webp", b"RIFF\x10\0\0\0WAVEfmt " + bytes(12), (0, 0), 0, accept=False, expect=ERR_IO)
    add("no_frame", riff(vp8x(17, 9) + UNKNOWN), (17, 9), 0, accept=False, expect=ERR_IO)
    return tuple(out)


def mutations(count=300, seed=1234):
    """Seeded byte mutations of valid files: (name, data).  One to three bytes of a file are replaced."""
    rng = np.random.default_rng(seed)
    pool = [c for c in cases() if c.accept and len(c.data) < 6000]
    out = []
    for k in range(count):
        c = pool[int(rng.integers(0, len(pool)))]
        d = bytearray(c.data)
        for _ in range(int(rng.integers(1, 4))):
            # the head of the file (container and stream headers, the codes) more often than the pixel data
            at = int(rng.integers(0, min(len(d), 96))) if rng.integers(0, 2) else int(rng.integers(0, len(d)))
            d[at] = int(rng.integers(0, 256))
        out.append((f"mut_{k}_{c.name}", bytes(d)))
    return out


# ------------------------------------------------------------------------------------------ Pillow

def pillow_frames(data: bytes):
    """(frames Pillow decodes before it raises, as uint8 [H, W, 3] each; the index of the frame it raised on or None)."""
    from PIL import Image
    frames = []
    try:
        im = Image.open(io.BytesIO(data))
        n = getattr(im, "n_frames", 1)
    except Exception:
        return frames, 0
    for k in range(n):
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
    """vge_webp_probe_mem -> (return code, int64 [n, 6] rows as vge.frames.webp_probe gives them)."""
    from vge import lib as L
    from vge.frames import _webp_rows
    n = len(off)
    info = (L.WebpInfo * max(n, 1))()
    rc = L.load().vge_webp_probe_mem(_ptr(data), data.size, _ptr(off), _ptr(size), n, threads, info)
    return rc, _webp_rows(info, n)


def host_decode_mem(data, off, size, canvas, frame_cap, threads=2, fill=0x5A):
    """vge_webp_decode_mem -> (return code, uint8 [frame_cap, H, W, 3], status [frame_cap], file status [n], frames)."""
    import ctypes as C

    from vge import lib as L
    w, h = canvas
    n = len(off)
    rgb, st = np.full((max(frame_cap, 1), h, w, 3), fill, np.uint8), np.full(max(frame_cap, 1), -1, np.int32)
    fst, total = np.full(max(n, 1), -1, np.int32), C.c_int64(-1)
    rc = L.load().vge_webp_decode_mem(_ptr(data), data.size, _ptr(off), _ptr(size), n, threads, w, h, frame_cap,
                                      _ptr(rgb), _ptr(st), _ptr(fst), C.byref(total))
    return rc, rgb[:frame_cap], st[:frame_cap], fst[:n], total.value


def host_plan_mem(data, off, size, canvas, threads=2, desc_cap=None):
    """vge_webp_plan_mem -> (return code, descs, n_descs, status [n_descs], file status [n], workspace bytes); a
    capacity of None is counted by a first call without buffers."""
    import ctypes as C

    from vge import lib as L
    lib = L.load()
    w, h = canvas
    n = len(off)
    nd, ws = C.c_int64(-1), C.c_int64(-1)
    fst = np.full(max(n, 1), -1, np.int32)
    head = (_ptr(data), data.size, _ptr(off), _ptr(size), n, threads, w, h)
    if desc_cap is None:
        lib.vge_webp_plan_mem(*head, None, 0, C.byref(nd), None, None, None)
        desc_cap = nd.value
    descs = (L.WebpDesc * max(desc_cap, 1))()
    st = np.full(max(desc_cap, 1), -1, np.int32)
    rc = lib.vge_webp_plan_mem(*head, descs, desc_cap, C.byref(nd), _ptr(st), _ptr(fst), C.byref(ws))
    return rc, descs, nd.value, st[:max(nd.value, 0)], fst[:n], ws.value


def features(data: bytes):
    """(first failing code, feature mask, the set of distance-map codes met, the largest group count) of one file in
    the host decoder (vge_debug_webp_features)."""
    import ctypes as C

    from vge import lib as L
    f = L.load().vge_debug_webp_features
    f.argtypes, f.restype = [C.c_void_p, C.c_int64, C.c_void_p], C.c_int
    buf = np.frombuffer(data, np.uint8)
    out = np.zeros(4, np.uint64)
    rc = f(_ptr(buf), buf.size, _ptr(out))
    codes = {k + 1 for k in range(120) if (int(out[1 + k // 64]) >> (k % 64)) & 1}
    return rc, int(out[0]), codes, int(out[3])


def by_canvas():
    """{canvas: [cases]} in first-seen order: one decode call per canvas takes good and refused files together.  Files
    without a readable canvas go with the first group."""
    groups = {}
    for c in cases():
        groups.setdefault(c.canvas if c.canvas[0] > 0 else (17, 9), []).append(c)
    return groups
