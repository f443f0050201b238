"""Baseline Huffman coding of one frame's coefficient array, restated in plain Python: the independent ground truth for
synthetic coefficients (tests/test_jpeg_entropy_host.py, tests/test_jpeg_entropy_gpu.py).  Nothing is typed in and
nothing comes from the code under test: the four Huffman tables are parsed from the DHT segments of a fixture file
written by Pillow, and the header is that file's own, with the quantisation entries and the frame size replaced."""
import numpy as np


def zigzag():
    """Natural index of each zigzag position, walked along the anti-diagonals."""
    order = sorted(((r + c, r if (r + c) % 2 else c, r * 8 + c) for r in range(8) for c in range(8)))
    return [nat for _, _, nat in order]


ZZ = zigzag()


def parse(jpeg: bytes):
    """Marker walk of a baseline file -> {'dht': {(class, id): {symbol: (code, length)}}, 'dqt': [payload offsets],
    'sof': payload offset, 'scan': offset of the entropy-coded data}."""
    out, p = {"dht": {}, "dqt": []}, 2
    assert jpeg[:2] == b"\xff\xd8"
    while True:
        assert jpeg[p] == 0xFF
        m, n = jpeg[p + 1], (jpeg[p + 2] << 8) | jpeg[p + 3]
        s = p + 4
        if m == 0xC4:
            tc, th, bits = jpeg[s] >> 4, jpeg[s] & 15, jpeg[s + 1:s + 17]
            vals, table, code, k = jpeg[s + 17:s + 17 + sum(bits)], {}, 0, 0
            for length in range(1, 17):
                for _ in range(bits[length - 1]):
                    table[vals[k]] = (code, length)
                    code, k = code + 1, k + 1
                code <<= 1
            out["dht"][(tc, th)] = table
        elif m == 0xDB:
            out["dqt"].append(s + 1)
        elif m == 0xC0:
            out["sof"] = s
        elif m == 0xDA:
            out["scan"] = p + 2 + n
            return out
        p += 2 + n


def scan_order(lay):
    """[(component, block index in the frame's coefficient array)] in the order of the interleaved scan."""
    order = []
    for my in range(lay.mcus_y):
        for mx in range(lay.mcus_x):
            for c in range(3):
                ch, cv = (lay.h0, lay.v0) if c == 0 else (1, 1)
                order += [(c, lay.off[c] + (my * cv + v) * lay.bw[c] + mx * ch + h) for v in range(cv) for h in range(ch)]
    return order


def encode(coef, qtab, lay, template: bytes):
    """coef int [blocks, 64] natural order, qtab [3, 64] -> the file's bytes; None for a frame baseline coding cannot
    carry (a DC difference beyond 11 bits, an AC value beyond 10)."""
    info = parse(template)
    head = bytearray(template[:info["scan"]])
    for t, o in enumerate(info["dqt"]):
        head[o:o + 64] = bytes(int(qtab[t][ZZ[k]]) for k in range(64))
    s = info["sof"]
    head[s + 1:s + 5] = bytes([lay.height >> 8, lay.height & 255, lay.width >> 8, lay.width & 255])
    head[s + 7] = (lay.h0 << 4) | lay.v0
    bits, pred = [], [0, 0, 0]

    def put(value, length):
        if length:
            bits.append(format(value & ((1 << length) - 1), f"0{length}b"))

    for c, b in scan_order(lay):
        dc, ac = info["dht"][(0, min(c, 1))], info["dht"][(1, min(c, 1))]
        blk = [int(v) for v in coef[b]]
        diff, pred[c] = blk[0] - pred[c], blk[0]
        n = abs(diff).bit_length()
        if n > 11:
            return None
        put(*dc[n])
        put(diff if diff >= 0 else diff - 1, n)
        run = 0
        for k in range(1, 64):
            v = blk[ZZ[k]]
            if v == 0:
                run += 1
                continue
            while run > 15:
                put(*ac[0xF0])
                run -= 16
            n = abs(v).bit_length()
            if n > 10:
                return None
            put(*ac[(run << 4) | n])
            put(v if v >= 0 else v - 1, n)
            run = 0
        if run:
            put(*ac[0])
    stream = "".join(bits)
    stream += "1" * (-len(stream) % 8)
    scan = int(stream, 2).to_bytes(len(stream) // 8, "big").replace(b"\xff", b"\xff\x00")
    return bytes(head) + scan + b"\xff\xd9"


def stats(coef, lay):
    """Counted from the coefficients themselves: blocks with a ZRL, blocks without EOB, AC values of size 10, DC
    differences of size 11, negative DC differences."""
    out = dict(zrl=0, no_eob=0, ac10=0, dc11=0, dc_neg=0)
    pred = [0, 0, 0]
    for c, b in scan_order(lay):
        blk = [int(v) for v in coef[b]]
        diff, pred[c] = blk[0] - pred[c], blk[0]
        out["dc11"] += abs(diff).bit_length() == 11
        out["dc_neg"] += diff < 0
        z = [blk[ZZ[k]] for k in range(1, 64)]
        nz = [k for k, v in enumerate(z) if v]
        out["no_eob"] += bool(z[62])
        out["ac10"] += sum(abs(v).bit_length() == 10 for v in z)
        out["zrl"] += any(b - a > 16 for a, b in zip([-1] + nz, nz))
    return out
