"""Deflate streams and npz archives for the ingest `_mem` calls and the device inflate kernel, built from seeds in
memory (no committed binaries).

  deflate()          Python's zlib, raw deflate, for the ordinary streams
  inflate()          a pure-Python instrumented inflate: output plus, per stream, block types and ends, the longest
                     code met, the largest distance and length, overlapping matches, the smallest match source
  BitWriter & co.    a minimal stored / fixed / dynamic block writer for streams zlib will not emit
  stream_cases()     one member stream per mechanism the kernel can get wrong, each asserted HERE (through inflate()
                     and zlib) to have the property it is named for, so a case that stops covering its ground fails
                     in the CPU suite
  archive_cases()    whole videos: npz bytes plus optional keypoints.npy bytes

A member's uncompressed stream is its npy header (128 bytes for every shape here) followed by the payload.  Crafted
members are `vit` [1, D] float32 with D = payload bytes / 4, so any byte string of a multiple of 4 bytes is a payload;
they open with a stored block that carries the header and the first payload bytes, so that zlib's header-only read (the
planner's) stops inside that block and everything crafted is left to the data decode."""
import io
import struct
import zlib
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

HDR = 128
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
CODES, LENS, DISTS = 0, 1, 2


def deflate(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def zlib_verdict(stream: bytes, total: int):
    """What vge_ingest_decode_mem's reader concludes: (accepted, bytes) for `total` wanted bytes."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream, total)
    except zlib.error:
        return False, b""
    return len(out) == total, out


# ------------------------------------------------------------------------------------------ instrumented inflate

class InflateError(Exception):
    pass


@dataclass
class Info:
    out: bytes = b""
    blocks: list = field(default_factory=list)   # (type, output position at the block's end)
    max_code_len: int = 0                        # longest length/literal or distance code met
    max_dist: int = 0
    max_len: int = 0
    n_matches: int = 0
    n_overlap: int = 0                           # matches with distance < length
    min_src: int = 1 << 60                       # smallest output position a match read
    n_symbols: int = 0                           # literals + matches + end-of-block codes
    match_srcs: list = field(default_factory=list)   # (position, source position, length) of the first 64 matches
    bits: int = 0                                # input bits consumed
    final: bool = False


def set_fault(lens, kind):
    """zlib's inflate_table verdict on a set of code lengths: None when accepted, else what is wrong with it."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    mx = max((l for l in range(1, 16) if count[l]), default=0)
    left = 1
    for l in range(1, 16):
        left = left * 2 - count[l]
        if left < 0:
            return "over-subscribed"
    if mx == 0:   # zlib builds an empty code-length code but then rejects the block (no code for 256)
        return "empty" if kind == CODES else None
    return "incomplete" if left > 0 and (kind == CODES or mx != 1) else None


def set_verdict(lens, kind) -> bool:
    return set_fault(lens, kind) is None


def canon(lens):
    """{symbol: (code, length)}: the canonical code of RFC 1951 3.2.2."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def _rev(v, n):
    return int(format(v, f"0{n}b")[::-1], 2) if n else 0


def _lut(lens):
    mx = max(lens, default=0)
    if mx == 0:
        return [None], 0
    t = [None] * (1 << mx)
    for s, (code, l) in canon(lens).items():
        r = _rev(code, l)
        for k in range(r, 1 << mx, 1 << l):
            t[k] = (s, l)
    return t, mx


class _Bits:
    def __init__(self, data):
        self.d, self.p, self.end = data, 0, 8 * len(data)

    def peek(self):
        b = self.p >> 3
        return int.from_bytes(self.d[b:b + 5], "little") >> (self.p & 7)

    def take(self, n):
        v = self.peek() & ((1 << n) - 1)
        self.p += n
        if self.p > self.end:
            raise InflateError("input exhausted")
        return v

    def sym(self, lut, mx, info=None):
        e = lut[self.peek() & ((1 << mx) - 1)] if mx else None
        if e is None:
            raise InflateError("invalid code")
        self.p += e[1]
        if self.p > self.end:
            raise InflateError("input exhausted")
        if info is not None:
            info.max_code_len = max(info.max_code_len, e[1])
        return e[0]


def inflate(stream: bytes, limit=None) -> Info:
    """Decode a raw deflate stream (up to `limit` output bytes).  Raises InflateError where zlib rejects."""
    r, info, out = _Bits(stream), Info(), bytearray()
    lim = limit if limit is not None else 1 << 60
    while not info.final and len(out) < lim:
        info.final = bool(r.take(1))
        typ = r.take(2)
        if typ == 3:
            raise InflateError("block type 3")
        if typ == 0:
            r.p = (r.p + 7) & ~7
            ln, nl = r.take(16), r.take(16)
            if ln != (~nl & 0xFFFF):
                raise InflateError("stored LEN != ~NLEN")
            n = min(ln, lim - len(out))
            b = r.p >> 3
            if b + n > len(stream):
                raise InflateError("input exhausted")
            out += stream[b:b + n]
            r.p += 8 * n
            info.blocks.append((0, len(out)))
            continue
        if typ == 1:
            ll, dl = FIXED_LL, FIXED_D
        else:
            hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
            if hlit > 286 or hdist > 30:
                raise InflateError("too many length or distance codes")
            cl = [0] * 19
            for i in range(hclen):
                cl[CLEN_ORDER[i]] = r.take(3)
            if not set_verdict(cl, CODES):
                raise InflateError(set_fault(cl, CODES) + " code-length code")
            clut, cmx = _lut(cl)
            lens = []
            while len(lens) < hlit + hdist:
                s = r.sym(clut, cmx)
                if s < 16:
                    lens.append(s)
                    continue
                if s == 16:
                    if not lens:
                        raise InflateError("repeat with no previous length")
                    v, rep = lens[-1], 3 + r.take(2)
                elif s == 17:
                    v, rep = 0, 3 + r.take(3)
                else:
                    v, rep = 0, 11 + r.take(7)
                if len(lens) + rep > hlit + hdist:
                    raise InflateError("repeat past the end")
                lens += [v] * rep
            ll, dl = lens[:hlit], lens[hlit:]
            if ll[256] == 0:
                raise InflateError("no end-of-block code")
            if not set_verdict(ll, LENS):
                raise InflateError(set_fault(ll, LENS) + " length set")
            if not set_verdict(dl, DISTS):
                raise InflateError(set_fault(dl, DISTS) + " distance set")
        llut, lmx = _lut(ll)
        dlut, dmx = _lut(dl)
        while len(out) < lim:
            s = r.sym(llut, lmx, info)
            info.n_symbols += 1
            if s < 256:
                out.append(s)
                continue
            if s == 256:
                break
            if s >= 286:
                raise InflateError("invalid length symbol")
            ln = LEN_BASE[s - 257] + r.take(LEN_EXTRA[s - 257])
            ds = r.sym(dlut, dmx, info)
            if ds >= 30:
                raise InflateError("invalid distance symbol")
            dist = DIST_BASE[ds] + r.take(DIST_EXTRA[ds])
            if dist > len(out):
                raise InflateError("distance before the first byte")
            info.n_matches += 1
            info.max_dist, info.max_len = max(info.max_dist, dist), max(info.max_len, ln)
            info.n_overlap += dist < ln
            info.min_src = min(info.min_src, len(out) - dist)
            if len(info.match_srcs) < 64:
                info.match_srcs.append((len(out), len(out) - dist, ln))
            for _ in range(min(ln, lim - len(out))):
                out.append(out[-dist])
        info.blocks.append((typ, len(out)))
    if limit is not None and len(out) < limit:
        raise InflateError("stream ended before the count")
    info.out, info.bits = bytes(out), r.p
    return info


# ------------------------------------------------------------------------------------------ block writer

class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, n):          # n bits of v, least significant first (header fields, extra bits)
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n

    def code(self, c):            # a Huffman code (code, length): most significant bit first
        self.put(_rev(c[0], c[1]), c[1])

    def align(self):
        self.n = (self.n + 7) & ~7

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def stored_block(w, data, final=False, nlen=None):
    w.put(int(final), 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put((~len(data) & 0xFFFF) if nlen is None else nlen, 16)
    for b in data:
        w.put(b, 8)


def _len_sym(ln):
    i = max(k for k in range(29) if LEN_BASE[k] <= ln) if ln < 258 else 28
    return 257 + i, ln - LEN_BASE[i], LEN_EXTRA[i]


def _dist_sym(d):
    i = max(k for k in range(30) if DIST_BASE[k] <= d)
    return i, d - DIST_BASE[i], DIST_EXTRA[i]


def put_symbols(w, syms, ll, dl, eob=True):
    """syms: int literal | (length, distance) | ("L", symbol) / ("D", symbol): a raw code with no extra bits."""
    lc, dc = canon(ll), canon(dl)
    for s in syms:
        if isinstance(s, int):
            w.code(lc[s])
        elif s[0] == "L":
            w.code(lc[s[1]])
        elif s[0] == "D":
            w.code(dc[s[1]])
        else:
            ls, lx, ln = _len_sym(s[0])
            w.code(lc[ls])
            w.put(lx, ln)
            ds, dx, dn = _dist_sym(s[1])
            w.code(dc[ds])
            w.put(dx, dn)
    if eob:
        w.code(lc[256])


def fixed_block(w, syms, final=False, eob=True):
    w.put(int(final), 1)
    w.put(1, 2)
    put_symbols(w, syms, FIXED_LL, FIXED_D, eob)


CL_PLAIN = [4] * 13 + [5] * 6   # a complete code-length code with a code for each of the 19 symbols


def dynamic_header(w, ll, dl, final=False, cl=None, cl_syms=None, hlit_field=None, hdist_field=None, hclen=19):
    """cl_syms: the code-length symbols to send, (symbol, extra value) pairs; default: every length on its own."""
    cl = CL_PLAIN if cl is None else cl
    w.put(int(final), 1)
    w.put(2, 2)
    w.put(len(ll) - 257 if hlit_field is None else hlit_field, 5)
    w.put(len(dl) - 1 if hdist_field is None else hdist_field, 5)
    w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl[CLEN_ORDER[i]], 3)
    cc = canon(cl)
    for s, x in ([(l, 0) for l in list(ll) + list(dl)] if cl_syms is None else cl_syms):
        w.code(cc[s])
        w.put(x, {16: 2, 17: 3, 18: 7}.get(s, 0))


def dynamic_block(w, syms, ll, dl, final=False, eob=True, **kw):
    dynamic_header(w, ll, dl, final, **kw)
    put_symbols(w, syms, ll, dl, eob)


def pad_lens(d, n):
    out = [0] * n
    for s, l in d.items():
        out[s] = l
    return out


# ------------------------------------------------------------------------------------------ npy / zip

def npy_bytes(a: np.ndarray) -> bytes:
    f = io.BytesIO()
    np.lib.format.write_array(f, np.ascontiguousarray(a), version=(1, 0))
    return f.getvalue()


def npy_header(shape, descr="<f4") -> bytes:
    h = npy_bytes(np.zeros(shape, np.dtype(descr)))[:HDR]
    assert h.endswith(b"\n") and len(npy_bytes(np.zeros(shape, np.dtype(descr)))) == HDR + int(np.prod(shape)) * int(descr[-1])
    return h


def make_zip(members) -> bytes:
    """members: [(name, method, compressed bytes, uncompressed size)] -> a zip file (CRC fields zero: nobody checks)."""
    out, cd = bytearray(), bytearray()
    for name, method, comp, usize in members:
        nm = name.encode()
        off = len(out)
        out += struct.pack("<IHHHHHIIIHH", 0x04034B50, 20, 0, method, 0, 0x21, 0, len(comp), usize, len(nm), 0) + nm
        out += comp
        cd += struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 20, 20, 0, method, 0, 0x21, 0, len(comp), usize, len(nm),
                          0, 0, 0, 0, 0, off) + nm
    eocd = struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, len(members), len(members), len(cd), len(out), 0)
    return bytes(out + cd + eocd)


def clip_arrays(seed, T, vit_dim=1024, dtype=np.float32):
    g = np.random.default_rng(seed)
    return {"pose": g.standard_normal((T, 23, 3, 3)).astype(dtype),
            "global_orient": g.standard_normal((T, 1, 3, 3)).astype(dtype),
            "betas": g.standard_normal((T, 10)).astype(dtype),
            "vit": g.standard_normal((T, vit_dim)).astype(dtype)}


def make_npz(arrays, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, streams=None, method=8) -> bytes:
    """np.savez_compressed's layout with our own writer; streams: {name: ready-made member stream} overrides."""
    streams = streams or {}
    members = []
    for k, a in arrays.items():
        raw = npy_bytes(a)
        if k in streams:
            members.append((k + ".npy", 8, streams[k], len(raw)))
        elif method == 0:
            members.append((k + ".npy", 0, raw, len(raw)))
        else:
            members.append((k + ".npy", 8, deflate(raw, level, strategy), len(raw)))
    return make_zip(members)


def savez(arrays, compressed=True) -> bytes:
    f = io.BytesIO()
    (np.savez_compressed if compressed else np.savez)(f, **arrays)
    return f.getvalue()


# ------------------------------------------------------------------------------------------ member streams

@dataclass
class StreamCase:
    stream: bytes
    total: int                 # header + payload bytes the member declares
    ok: bool                   # zlib's verdict (and so the device's)
    payload: bytes = b""       # for accepted streams
    member: str = "vit"        # the member that carries it; the video has T frames
    T: int = 1
    device_only: bool = False  # the class outside the equality: asserted on the device side only
    why: str = ""              # rejected streams: what inflate() must say of it (the class the case stands for)

    @property
    def vit_dim(self):
        return (self.total - HDR) // 4 if self.member == "vit" and self.T == 1 else 1024


def _floats(seed, n):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32).tobytes()


def _open(w, payload_bytes, lead):
    """The stored opening block of a crafted vit [1, D] member: header + the payload's first `lead` bytes."""
    head = npy_header((1, len(payload_bytes) // 4))
    stored_block(w, head + payload_bytes[:lead])
    return head


def _case_from_writer(w, payload, ok=True, **kw):
    return StreamCase(w.bytes(), HDR + len(payload), ok, payload if ok else b"", **kw)


def _zlib_member(arr, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, member="vit"):
    raw = npy_bytes(arr)
    assert len(raw) - arr.nbytes == HDR
    return StreamCase(deflate(raw, level, strategy), len(raw), True, raw[HDR:], member=member, T=arr.shape[0]), raw


@lru_cache(maxsize=None)
def stream_cases():
    """name -> StreamCase.  Every property a case is named for is asserted here."""
    C = {}
    g = np.random.default_rng(20240)

    # ---- zlib's own streams
    c, raw = _zlib_member(g.standard_normal((18, 1024)).astype(np.float32), level=0)
    i = inflate(c.stream)
    assert len(raw) == 73856 and [b for b in i.blocks] == [(0, 65535), (0, 73856)]
    C["stored_two_blocks"] = c

    c, raw = _zlib_member(g.standard_normal((2, 10)).astype(np.float32), strategy=zlib.Z_FIXED, member="betas")
    assert [t for t, _ in inflate(c.stream).blocks] == [1]
    C["fixed_2x10"] = c

    c, raw = _zlib_member(g.standard_normal((8, 1024)).astype(np.float32))
    i = inflate(c.stream)
    assert [t for t, _ in i.blocks] == [2] and i.max_code_len > 10, (i.blocks, i.max_code_len)  # beyond the fast table
    C["dynamic_one_block"] = c

    c, raw = _zlib_member(g.standard_normal((32, 1024)).astype(np.float32))
    i = inflate(c.stream)
    assert len(i.blocks) >= 4 and all(t == 2 for t, _ in i.blocks) and i.blocks[-1][1] == 131200, i.blocks
    C["dynamic_four_blocks"] = c

    c, raw = _zlib_member(np.zeros((40, 1024), np.float32))
    i = inflate(c.stream)
    assert i.max_len == 258 and i.n_overlap >= 600 and any(p - s == 1 for p, s, _ in i.match_srcs), vars(i)
    C["zeros_rle"] = c

    frame = g.standard_normal((1, 23, 3, 3)).astype(np.float32)
    c, raw = _zlib_member(np.repeat(frame, 64, 0), member="pose")
    i = inflate(c.stream)
    assert i.max_len == 258 and i.max_dist >= 828, (i.max_len, i.max_dist)
    C["static_pose"] = c

    # ---- the header as LZ77 history
    head = npy_header((1, 320))
    c = StreamCase(deflate(head + head * 10), HDR + 1280, True, head * 10)
    i = inflate(c.stream)
    assert i.min_src < HDR and any(p - s == 128 and p >= HDR > s for p, s, _ in i.match_srcs), i.match_srcs
    C["payload_repeats_header"] = c

    pay = _floats(1, 16)
    w = BitWriter()
    head = _open(w, pay, 4)
    # position 132: a 20-byte match from position 120: 8 header bytes, then the 4 stored payload bytes, then its own output
    fixed_block(w, [(20, 12)] + list(pay[:40]), final=True)
    payload = pay[:4] + bytes((head + pay[:4])[120 + k % 12] for k in range(20)) + pay[:40]
    c = _case_from_writer(w, payload)
    i = inflate(c.stream)
    assert i.out[HDR:] == payload and i.match_srcs[0] == (132, 120, 20)
    C["match_straddles_header"] = c

    # ---- crafted with the block writer
    pay = _floats(2, 8192 + 64)                      # 33,024 bytes
    w = BitWriter()
    _open(w, pay, 33020)                              # output position 33,148 after the stored block
    fixed_block(w, [(4, 32768)], final=True)
    c = _case_from_writer(w, pay[:33020] + pay[33020 - 32768:33020 - 32768 + 4])
    i = inflate(c.stream)
    assert i.max_dist == 32768 and i.match_srcs[0][1] == HDR + 33020 - 32768
    C["distance_32768"] = c

    pay = _floats(3, 64)
    w = BitWriter()
    _open(w, pay[:108], 40)                                               # stored: positions 0..167; 108 bytes in all
    fixed_block(w, list(pay[40:60]) + [(8, 30)])                          # match source in the stored block
    fixed_block(w, [(10, 20)] + list(pay[:8]))                            # match source in the previous coded block
    stored_block(w, b"")                                                  # an empty stored block between coded ones
    fixed_block(w, list(pay[8:30]))
    fixed_block(w, [], final=True)                                        # an empty final block
    i = inflate(w.bytes())
    c = _case_from_writer(w, i.out[HDR:])
    assert [t for t, _ in i.blocks] == [0, 1, 1, 0, 1, 1] and i.blocks[3][1] == i.blocks[2][1] \
        and i.blocks[5][1] == i.blocks[4][1] and i.match_srcs[0][1] < 168 <= i.match_srcs[0][0] \
        and 168 <= i.match_srcs[1][1] < i.blocks[1][1] <= i.match_srcs[1][0] and len(i.out) % 4 == 0
    C["blocks_mixed"] = c

    # 15-bit codes: literals 0..13 with lengths 1..14, literal 14 and the end-of-block code with 15 bits
    ll = pad_lens({**{k: k + 1 for k in range(14)}, 14: 15, 256: 15}, 257)
    pay = bytes([14, 13, 0, 1] * 8 + [12, 14, 14, 3] * 4)
    w = BitWriter()
    _open(w, pay, 4)
    dynamic_block(w, list(pay[4:]), ll, [0], final=True)
    c = _case_from_writer(w, pay)
    assert inflate(c.stream).max_code_len == 15
    C["codes_15_bits"] = c

    # a distance set of one 1-bit code: used; then the same set with its unused code met
    ll = pad_lens({**{k: 8 for k in range(252)}, 256: 8, 257: 8, 258: 8, 259: 8}, 260)
    assert set_verdict(ll, LENS)
    for name, unused in (("one_distance_code", False), ("one_distance_code_unused_met", True)):
        pay = bytes(range(4, 44))
        w = BitWriter()
        _open(w, pay, 8)
        dynamic_header(w, ll, [0, 0, 1], final=True)
        put_symbols(w, list(pay[8:36]), ll, [0, 0, 1], eob=False)
        w.code(canon(ll)[258])                    # length 4
        w.put(1 if unused else 0, 1)              # the distance set's only code is '0' (symbol 2: distance 3)
        put_symbols(w, [], ll, [0, 0, 1])
        body = pay[:36] + bytes([pay[33], pay[34], pay[35], pay[33]])
        C[name] = _case_from_writer(w, body, ok=not unused)

    # ---- every rejection class (the stream breaks in the payload, after the stored opening block)
    pay = _floats(4, 32)

    def broken(fn, lead=8):
        w = BitWriter()
        _open(w, pay, lead)
        fn(w)
        return _case_from_writer(w, pay, ok=False)

    def raw_block(w, bits):          # a non-final block header of the given type, then raw (value, count) bit fields
        for v, n in bits:
            w.put(v, n)

    C["reject_block_type_3"] = broken(lambda w: raw_block(w, [(0, 1), (3, 2), (0, 64)]))
    C["reject_stored_nlen"] = broken(lambda w: stored_block(w, pay[8:], True, nlen=0x1234))
    C["reject_length_symbol_286"] = broken(lambda w: fixed_block(w, list(pay[8:20]) + [("L", 286)] + [0] * 8, True))
    C["reject_length_symbol_287"] = broken(lambda w: fixed_block(w, list(pay[8:20]) + [("L", 287)] + [0] * 8, True))
    for ds in (30, 31):
        def f(w, ds=ds):
            fixed_block(w, list(pay[8:20]) + [("L", 257), ("D", ds)] + [0] * 8, True)
        C[f"reject_distance_symbol_{ds}"] = broken(f)
    C["reject_distance_before_member"] = broken(lambda w: fixed_block(w, [(3, HDR + 8 + 1)] + [0] * 8, True))
    C["reject_stream_ends_before_count"] = broken(lambda w: fixed_block(w, list(pay[8:40]), True))   # 96 of 120 payload bytes
    ok_ll = pad_lens({**{k: 8 for k in range(255)}, 256: 8}, 257)
    assert set_verdict(ok_ll, LENS)
    C["reject_too_many_length_codes"] = broken(lambda w: dynamic_header(w, ok_ll, [0], hlit_field=30))
    C["reject_too_many_distance_codes"] = broken(lambda w: dynamic_header(w, ok_ll, [0], hdist_field=30))
    C["reject_repeat_without_previous"] = broken(lambda w: dynamic_header(w, ok_ll, [0], cl_syms=[(16, 0)]))
    C["reject_repeat_past_end"] = broken(
        lambda w: dynamic_header(w, ok_ll, [0], cl_syms=[(8, 0)] * 250 + [(18, 127)]))
    C["reject_no_end_of_block_code"] = broken(
        lambda w: dynamic_header(w, pad_lens({k: 8 for k in range(256)}, 257), [0]))
    C["reject_oversubscribed_lengths"] = broken(
        lambda w: dynamic_header(w, pad_lens({**{k: 8 for k in range(255)}, 255: 1, 256: 8}, 257), [0]))
    C["reject_oversubscribed_distances"] = broken(lambda w: dynamic_header(w, ok_ll, [1, 1, 1]))
    C["reject_incomplete_lengths"] = broken(
        lambda w: dynamic_header(w, pad_lens({**{k: 8 for k in range(200)}, 256: 8}, 257), [0]))
    C["reject_incomplete_distances"] = broken(lambda w: dynamic_header(w, ok_ll, [2, 2, 2]))
    C["reject_incomplete_code_length_code"] = broken(
        lambda w: dynamic_header(w, ok_ll, [0], cl=[4] * 12 + [0] * 7, cl_syms=[]))
    C["reject_oversubscribed_code_length_code"] = broken(
        lambda w: dynamic_header(w, ok_ll, [0], cl=[2] * 5 + [0] * 14, cl_syms=[]))
    # two truncations: in the middle of a symbol, in the middle of a stored block
    w = BitWriter()
    _open(w, pay, 8)
    fixed_block(w, list(pay[8:]), True)
    whole = w.bytes()
    assert inflate(whole, HDR + len(pay)).out[HDR:] == pay
    cut = len(whole) - 40
    C["reject_truncated_mid_symbol"] = StreamCase(whole[:cut], HDR + len(pay), False)
    w = BitWriter()
    _open(w, pay, 8)
    stored_block(w, pay[8:], True)
    C["reject_truncated_mid_stored"] = StreamCase(w.bytes()[:-30], HDR + len(pay), False)

    # ---- the class outside the equality: the stream carries more than the header declares
    w = BitWriter()
    _open(w, pay, 8)
    fixed_block(w, list(pay[8:]) + list(range(40)), True)
    C["overlong_member"] = StreamCase(w.bytes(), HDR + len(pay), True, pay, device_only=True)

    why = {"one_distance_code_unused_met": "invalid code", "reject_block_type_3": "block type 3",
           "reject_stored_nlen": "stored LEN != ~NLEN", "reject_length_symbol_286": "invalid length symbol",
           "reject_length_symbol_287": "invalid length symbol", "reject_distance_symbol_30": "invalid distance symbol",
           "reject_distance_symbol_31": "invalid distance symbol",
           "reject_distance_before_member": "distance before the first byte",
           "reject_stream_ends_before_count": "stream ended before the count",
           "reject_too_many_length_codes": "too many length or distance codes",
           "reject_too_many_distance_codes": "too many length or distance codes",
           "reject_repeat_without_previous": "repeat with no previous length",
           "reject_repeat_past_end": "repeat past the end", "reject_no_end_of_block_code": "no end-of-block code",
           "reject_oversubscribed_lengths": "over-subscribed length set",
           "reject_oversubscribed_distances": "over-subscribed distance set",
           "reject_incomplete_lengths": "incomplete length set",
           "reject_incomplete_distances": "incomplete distance set",
           "reject_incomplete_code_length_code": "incomplete code-length code",
           "reject_oversubscribed_code_length_code": "over-subscribed code-length code",
           "reject_truncated_mid_symbol": "input exhausted", "reject_truncated_mid_stored": "input exhausted"}
    assert sorted(why) == sorted(n for n, c in C.items() if not c.ok)
    for name, c in C.items():
        c.why = why.get(name, "")
        assert (c.total - HDR) % 4 == 0 and c.total - HDR >= 0, name
        if c.device_only:
            assert inflate(c.stream, c.total).out[HDR:] == c.payload, name
            continue
        ok, out = zlib_verdict(c.stream, c.total)
        assert ok == c.ok, (name, "zlib", ok)
        try:
            mine, said = inflate(c.stream, c.total).out, ""
        except InflateError as e:
            mine, said = None, str(e)
        assert (mine is not None) == c.ok and said == c.why, (name, "inflate()", said)
        if c.ok:
            assert out[HDR:] == c.payload == mine[HDR:], name
            assert out[:HDR] == (npy_header((1, c.vit_dim)) if c.member == "vit" and c.T == 1 else out[:HDR]), name
        else:
            # the header alone must inflate, or the planner would refuse the video before the kernel sees it
            d = zlib.decompressobj(-15)
            assert len(d.decompress(c.stream, 12)) == 12 and len(d.decompress(d.unconsumed_tail, HDR - 12)) == HDR - 12, name
    return C


def video_for_stream(c: StreamCase, seed=7):
    """A whole video around a member stream -> (npz bytes, vit_dim)."""
    arrays = clip_arrays(seed, c.T, c.vit_dim)
    return make_npz(arrays, streams={c.member: c.stream}), c.vit_dim


# ------------------------------------------------------------------------------------------ whole videos

def kp_bytes(seed, rows, dtype=np.float32):
    return npy_bytes(np.random.default_rng(seed).standard_normal((rows, 120)).astype(dtype))


@lru_cache(maxsize=None)
def archive_cases():
    """name -> (npz bytes, keypoints.npy bytes or None, vit_dim)."""
    from tests.conftest import GOLDEN
    A = {}
    A["plain_f32"] = (savez(clip_arrays(11, 40)), kp_bytes(11, 40), 1024)
    A["all_f64"] = (savez(clip_arrays(12, 33, dtype=np.float64)), kp_bytes(12, 33, np.float64), 1024)
    mixed = clip_arrays(13, 35)
    mixed["pose"] = mixed["pose"].astype(np.float64)
    mixed["vit"] = mixed["vit"].astype(np.float64)
    A["mixed_f32_f64"] = (savez(mixed), kp_bytes(13, 35), 1024)
    A["uncompressed"] = (savez(clip_arrays(14, 36), compressed=False), kp_bytes(14, 36), 1024)
    A["kp_shorter"] = (savez(clip_arrays(15, 40)), kp_bytes(15, 31), 1024)
    A["kp_absent"] = (savez(clip_arrays(16, 34)), None, 1024)
    A["one_frame"] = (savez(clip_arrays(17, 1)), kp_bytes(17, 1), 1024)
    A["vit_dim_64"] = (savez(clip_arrays(18, 37, vit_dim=64)), kp_bytes(18, 37), 64)
    A["reference_written"] = ((GOLDEN / "npz_format" / "Action" / "v_ref.npz").read_bytes(), None, None)
    return A


def pack(files, gap=0, order=None, fill=0xA5):
    """files: per video (npz bytes, kp bytes or None) -> (buffer, offsets [2n], sizes [2n]): entries 2i / 2i + 1, kp size
    -1 when absent; `gap` bytes of `fill` before, between and after the files; order: the order the files are laid in."""
    flat = [b for pair in files for b in pair]
    order = list(range(len(flat))) if order is None else order
    off, size = np.zeros(len(flat), np.int64), np.full(len(flat), -1, np.int64)
    pos = gap
    for j in order:
        if flat[j] is None:
            continue
        off[j], size[j] = pos, len(flat[j])
        pos += len(flat[j]) + gap
    data = np.full(max(pos, 1), fill, np.uint8)
    for j, b in enumerate(flat):
        if b is not None:
            data[off[j]:off[j] + len(b)] = np.frombuffer(b, np.uint8)
    return data, off, size


# ------------------------------------------------------------------------------------------ the C calls

def _ptr(a):
    import ctypes as C
    return a.ctypes.data_as(C.c_void_p)


def host_probe_mem(data, off, size, threads=2):
    """vge_ingest_probe_mem -> (return code, [(n_frames, vit_dim, kp_frames, status)])."""
    from vge import lib as L
    n = len(off) // 2
    info = (L.ClipInfo * max(n, 1))()
    rc = L.load().vge_ingest_probe_mem(_ptr(data), data.size, _ptr(off), _ptr(size), n, threads, info)
    return rc, [(info[i].n_frames, info[i].vit_dim, info[i].kp_frames, info[i].status) for i in range(n)]


def video_table(rows):
    """The frame-store layout a caller derives from the probe: failed videos get no rows."""
    videos = np.zeros((len(rows), 4), np.int32)
    o = ko = 0
    for i, (T, _, kT, st) in enumerate(rows):
        T, kT = (T, max(kT, 0)) if st == 0 else (0, 0)
        videos[i] = (o, T, ko, kT)
        o, ko = o + T, ko + kT
    return videos, o, ko


def empty_store(F, Fk, vit_dim, fill=np.nan):
    return {"pose": np.full((F, 207), fill, np.float32), "gori": np.full((F, 9), fill, np.float32),
            "betas": np.full((F, 10), fill, np.float32), "vit": np.full((F, vit_dim), fill, np.float32),
            "kp": np.full((max(Fk, 1), 120), fill, np.float32)}


def host_decode_mem(data, off, size, videos, vit_dim, F, Fk, threads=2):
    """vge_ingest_decode_mem -> (return code, status [n], the five arrays)."""
    from vge import lib as L
    n = len(off) // 2
    st = np.full(max(n, 1), -77, np.int32)
    a = empty_store(F, Fk, vit_dim)
    rc = L.load().vge_ingest_decode_mem(_ptr(data), data.size, _ptr(off), _ptr(size), n, threads, _ptr(videos), vit_dim,
                                        _ptr(a["pose"]), _ptr(a["gori"]), _ptr(a["betas"]), _ptr(a["vit"]),
                                        _ptr(a["kp"]), _ptr(st))
    return rc, st[:n], a


def host_plan_mem(data, off, size, videos, vit_dim, threads=2):
    """vge_ingest_plan_mem -> (return code, descriptor array [5n], info rows, workspace bytes)."""
    import ctypes as C
    from vge import lib as L
    n = len(off) // 2
    descs = (L.InflateDesc * max(5 * n, 1))()
    info = (L.ClipInfo * max(n, 1))()
    ws = C.c_int64(-1)
    rc = L.load().vge_ingest_plan_mem(_ptr(data), data.size, _ptr(off), _ptr(size), n, threads, _ptr(videos), vit_dim,
                                      descs, info, C.byref(ws))
    return rc, descs, [(info[i].n_frames, info[i].vit_dim, info[i].kp_frames, info[i].status) for i in range(n)], \
        int(ws.value)


def same_bits(a, b):
    """Equality of float arrays as bit patterns (crafted payloads are arbitrary bytes: NaNs must compare equal)."""
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
