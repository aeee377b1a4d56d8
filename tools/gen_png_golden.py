#!/usr/bin/env python
"""Writes tests/golden/png_streams.npz: the annotation PNG files the N26 tests decode (tests/test_png_host.py, tests/test_hip_png.py).

The files are built by hand - ``struct`` and ``zlib.crc32`` for the chunks, NumPy for the filters and the bit packing, and a small deflate
writer with PRESCRIBED code lengths - so that they hold filters, depths and deflate shapes Pillow's writer never produces.  Every stream
is checked against ``zlib.decompress`` here, every supported file against Pillow's decode.  Keys: ``ok__<name>`` supported files,
``bad__<status>__<name>`` broken ones (m6 = status -6) and ``uns__<reason>__<name>`` unsupported ones.

    python tools/gen_png_golden.py            # rewrites the fixture (deterministic)
"""
import io
import os
import struct
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "png_streams.npz")
SIGNATURE = b"\x89PNG\r\n\x1a\n"
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


# ---- chunks and rows ----------------------------------------------------------------------------------------------------------------
def chunk(kind: bytes, data: bytes, crc=None) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) if crc is None else crc)


def png(H, W, depth, color, zdata, split=None, interlace=0, extra=b"") -> bytes:
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, color, 0, 0, interlace))
    if color == 3:
        out += chunk(b"PLTE", bytes(range(256)) * 3)
    out += extra
    step = split or max(len(zdata), 1)
    for at in range(0, max(len(zdata), 1), step):
        out += chunk(b"IDAT", zdata[at:at + step])
    return out + chunk(b"IEND", b"")


def pack_rows(idx, depth):
    """uint8 [H, W] indices -> uint8 [H, ceil(W depth / 8)], MSB first."""
    H, W = idx.shape
    if depth == 8:
        return idx.copy()
    bits = np.zeros((H, -(-W * depth // 8) * 8), np.uint8)
    for k in range(depth):
        bits[:, k:W * depth:depth] = (idx >> (depth - 1 - k)) & 1
    return np.packbits(bits, axis=1)


def filter_rows(rows, types) -> bytes:
    """rows uint8 [H, rb], types[r] in 0 .. 4 -> the filtered bytes, each row behind its filter byte (bpp = 1)."""
    H, rb = rows.shape
    r16 = rows.astype(np.int32)
    out = bytearray()
    for r in range(H):
        x = r16[r]
        a = np.concatenate([[0], x[:-1]])
        b = r16[r - 1] if r else np.zeros(rb, np.int32)
        c = np.concatenate([[0], b[:-1]])
        t = types[r]
        if t == 0:
            pred = 0
        elif t == 1:
            pred = a
        elif t == 2:
            pred = b
        elif t == 3:
            pred = (a + b) >> 1
        else:
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        out += bytes([t]) + ((x - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def raw_of(idx, depth, types=None) -> bytes:
    return filter_rows(pack_rows(idx, depth), types if types is not None else [r % 5 for r in range(idx.shape[0])])


def blobs(H, W, n_values, seed):
    """A label map of a few elliptic blobs on background 0."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), np.uint8)
    for v in range(1, n_values):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        ry, rx = rng.uniform(H / 8 + 1, H / 3 + 1), rng.uniform(W / 8 + 1, W / 3 + 1)
        m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1] = v
    return m


# ---- a deflate writer with prescribed code lengths -----------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def bits(self, value, count):       # LSB first
        self.acc |= (value & ((1 << count) - 1)) << self.n
        self.n += count

    def code(self, code, length):       # a Huffman code: its first bit first
        for k in range(length - 1, -1, -1):
            self.bits((code >> k) & 1, 1)

    def align(self):
        self.n = -(-self.n // 8) * 8

    def bytes(self):
        return self.acc.to_bytes(-(-self.n // 8), "little")


def canonical(lens):
    """code lengths -> {symbol: (code, length)} (RFC 1951 3.2.2)"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def complete(symbols, n):
    """A complete code over ``symbols`` (in this order: the first ones get the shorter codes), as a list of n lengths."""
    m = len(symbols)
    lens = [0] * n
    if m == 1:
        lens[symbols[0]] = 1
        return lens
    k = (m - 1).bit_length()
    short = (1 << k) - m
    for i, s in enumerate(symbols):
        lens[s] = k - 1 if i < short else k
    return lens


def ladder(symbols, n):
    """Lengths 1, 2, ..., 14, 15, 15 over exactly 16 symbols in this order: a complete code with two 15-bit codes."""
    assert len(symbols) == 16
    lens = [0] * n
    for i, s in enumerate(symbols):
        lens[s] = min(i + 1, 15)
    return lens


def tokens_of(raw: bytes, dists=(1,), max_len=258, forced=None):
    """A greedy tokeniser: ('lit', b) / ('match', length, dist), trying only the distances given; forced {pos: (length, dist)}."""
    out, pos, n, forced = [], 0, len(raw), forced or {}
    while pos < n:
        best = (0, 0)
        if pos in forced:
            best = forced[pos]
            assert raw[pos:pos + best[0]] == bytes(raw[pos - best[1] + (i % best[1])] for i in range(best[0])), pos
        else:
            for d in dists:
                if d > pos:
                    continue
                l = 0
                while l < max_len and pos + l < n and raw[pos + l] == raw[pos + l - d] and not any(pos < f < pos + l + 1 for f in forced):
                    l += 1
                if l >= 3 and l > best[0]:
                    best = (l, d)
        if best[0]:
            out.append(("match",) + best)
            pos += best[0]
        else:
            out.append(("lit", raw[pos]))
            pos += 1
    return out


def len_symbol(length):
    s = max(i for i in range(29) if LEN_BASE[i] <= length)
    if length == 258:
        s = 28
    return 257 + s, length - LEN_BASE[s], LEN_EXTRA[s]


def dist_symbol(dist):
    s = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return s, dist - DIST_BASE[s], DIST_EXTRA[s]


def used_symbols(tokens):
    lit, dist = {256}, set()
    for t in tokens:
        if t[0] == "lit":
            lit.add(t[1])
        else:
            lit.add(len_symbol(t[1])[0])
            dist.add(dist_symbol(t[2])[0])
    return sorted(lit), sorted(dist)


def write_symbols(w, tokens, lit_lens, dist_lens):
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    for t in tokens:
        if t[0] == "lit":
            w.code(*lit[t[1]])
        else:
            s, extra, nbits = len_symbol(t[1])
            w.code(*lit[s])
            w.bits(extra, nbits)
            s, extra, nbits = dist_symbol(t[2])
            w.code(*dist[s])
            w.bits(extra, nbits)
    w.code(*lit[256])


def header_ops(lens):
    """The run-length form of the code lengths: [(symbol, extra value, extra bits, index, run)], greedy."""
    ops, i, n = [], 0, len(lens)
    while i < n:
        v, run = lens[i], 1
        while i + run < n and lens[i + run] == v:
            run += 1
        if v == 0 and run >= 11:
            r = min(run, 138)
            ops.append((18, r - 11, 7, i, r))
        elif v == 0 and run >= 3:
            r = min(run, 10)
            ops.append((17, r - 3, 3, i, r))
        elif v != 0 and run >= 4:
            r = min(run - 1, 6)
            ops.append((v, 0, 0, i, 1))
            ops.append((16, r - 3, 2, i + 1, r))
            r += 1
        else:
            r = 1
            ops.append((v, 0, 0, i, 1))
        i += r
    return ops


def dynamic_block(w, tokens, lit_lens, dist_lens, final, ops_out=None):
    nlit = max(257, max(i for i, l in enumerate(lit_lens) if l) + 1)
    ndist = max(1, max([i for i, l in enumerate(dist_lens) if l], default=0) + 1)
    lens = list(lit_lens[:nlit]) + list(dist_lens[:ndist])
    ops = header_ops(lens)
    if ops_out is not None:
        ops_out.extend((o, nlit) for o in ops)
    cl = canonical([4] * 13 + [5] * 6)        # a complete code-length code: 13 / 16 + 6 / 32 = 1
    w.bits(final, 1)
    w.bits(2, 2)
    w.bits(nlit - 257, 5)
    w.bits(ndist - 1, 5)
    w.bits(19 - 4, 4)
    for s in ORDER:
        w.bits(4 if s < 13 else 5, 3)
    for sym, extra, nbits, _, _ in ops:
        w.code(*cl[sym])
        w.bits(extra, nbits)
    write_symbols(w, tokens, lit_lens, dist_lens)


def fixed_block(w, tokens, final):
    w.bits(final, 1)
    w.bits(1, 2)
    write_symbols(w, tokens, FIXED_LIT, FIXED_DIST)


def stored_block(w, data, final, nlen=None):
    w.bits(final, 1)
    w.bits(0, 2)
    w.align()
    w.bits(len(data), 16)
    w.bits((len(data) ^ 0xffff) if nlen is None else nlen, 16)
    for b in data:
        w.bits(b, 8)


def zwrap(deflate: bytes, raw: bytes, adler=None) -> bytes:
    return b"\x78\x9c" + deflate + struct.pack(">I", zlib.adler32(raw) if adler is None else adler)


def accepted(z: bytes, raw: bytes) -> bytes:
    assert zlib.decompress(z) == raw
    return z


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def zlib_variant(raw: bytes, k: int, flush: bool) -> bytes:
    level, strategy = [(0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)][k % 5]
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    half = len(raw) // 2
    z = c.compress(raw[:half]) + (c.flush(zlib.Z_FULL_FLUSH) if flush else b"") + c.compress(raw[half:]) + c.flush()
    return accepted(z, raw)


def adam7(idx, depth) -> bytes:
    out = b""
    for y0, x0, dy, dx in [(0, 0, 8, 8), (0, 4, 8, 8), (4, 0, 8, 4), (0, 2, 4, 4), (2, 0, 4, 2), (0, 1, 2, 2), (1, 0, 2, 1)]:
        sub = idx[y0::dy, x0::dx]
        if sub.size:
            out += raw_of(np.ascontiguousarray(sub), depth, [0] * sub.shape[0])
    return out


def build():
    ok, bad, uns = {}, {}, {}
    rng = np.random.RandomState(26)
    k = 0
    for H, W in [(1, 1), (1, 9), (3, 7), (7, 1), (63, 33), (64, 33), (65, 33), (130, 33)]:
        for depth in (1, 2, 4, 8):
            nv = min(1 << depth, 6)
            idx = blobs(H, W, nv, 100 * H + W + depth) if H > 8 else rng.randint(0, 1 << min(depth, 7), (H, W)).astype(np.uint8)
            raw = raw_of(idx, depth)
            ok[f"z{k % 5}_{H}x{W}_d{depth}" + ("_flush7" if k % 3 == 0 else "")] = (
                png(H, W, depth, 3, zlib_variant(raw, k, k % 3 == 0), split=7 if k % 3 == 0 else None), idx)
            k += 1
    for H, W in [(3, 7), (65, 33)]:
        idx = rng.randint(0, 256, (H, W)).astype(np.uint8)
        ok[f"gray_{H}x{W}"] = (png(H, W, 8, 0, zlib_variant(raw_of(idx, 8), 2, False), extra=chunk(b"tEXt", b"Comment\0label map")), idx)

    from PIL import Image
    for (H, W), optimize in [((375, 500), False), ((480, 854), True)]:
        idx = blobs(H, W, 5, H)
        im = Image.fromarray(idx, "P")
        im.putpalette(list(range(256)) * 3)
        buf = io.BytesIO()
        im.save(buf, "PNG", optimize=optimize)
        ok[f"pillow_{H}x{W}" + ("_opt" if optimize else "")] = (buf.getvalue(), idx)

    def crafted(name, idx, deflate, raw, depth=8):
        ok[name] = (png(idx.shape[0], idx.shape[1], depth, 3, accepted(zwrap(deflate, raw), raw)), idx)

    # 15-bit codes in both alphabets: 16 literal/length symbols and 16 distance symbols on the ladder 1, 2, ..., 14, 15, 15
    idx = np.zeros((12, 40), np.uint8)
    idx[:, ::3] = 1
    idx[5:, 7:30] = 2
    idx[11, 39] = 3                                       # the rarest literal: it gets a 15-bit code
    raw = raw_of(idx, 8, [0] * 12)
    toks = tokens_of(raw, dists=(3, 41), max_len=10)
    lit_used, dist_used = used_symbols(toks)
    assert len(lit_used) <= 16 and len(dist_used) <= 16 and 3 in lit_used and dist_symbol(41)[0] in dist_used, (lit_used, dist_used)
    lit_order = [s for s in lit_used if s != 3] + [s for s in range(100, 140)][:16 - len(lit_used)] + [3]
    dist_order = [s for s in dist_used if s != dist_symbol(41)[0]] + [s for s in range(16, 30) if s not in dist_used][:16 - len(dist_used)] + [dist_symbol(41)[0]]
    w = BitWriter()
    dynamic_block(w, toks, ladder(lit_order, 286), ladder(dist_order, 30), 1)
    crafted("craft_15bit_codes", idx, w.bytes(), raw)

    # a distance set with a single code (all matches at distance 1), and with none (an all-literal block)
    idx = np.zeros((9, 30), np.uint8)
    idx[3:6] = 4
    raw = raw_of(idx, 8, [0] * 9)
    toks = tokens_of(raw, dists=(1,))
    w = BitWriter()
    dynamic_block(w, toks, complete(used_symbols(toks)[0], 286), complete([0], 30), 1)
    crafted("craft_one_distance_code", idx, w.bytes(), raw)
    idx = rng.randint(0, 4, (5, 11)).astype(np.uint8)
    raw = raw_of(idx, 2)
    toks = [("lit", b) for b in raw]
    w = BitWriter()
    dynamic_block(w, toks, complete(used_symbols(toks)[0], 286), [0] * 30, 1)
    crafted("craft_no_distance_code", idx, w.bytes(), raw, depth=2)

    # code-length repeats 16 / 17 / 18, one of them running from the literal/length lengths into the distance lengths
    idx = rng.randint(0, 150, (10, 20)).astype(np.uint8)
    idx[4:8] = idx[3]
    raw = raw_of(idx, 8, [0] * 10)
    toks = tokens_of(raw, dists=(21, 1), max_len=30)
    lit_syms = list(range(150)) + list(range(155, 200)) + list(range(256, 272))
    assert set(used_symbols(toks)[0]) <= set(lit_syms) and set(used_symbols(toks)[1]) <= set(range(9))
    ops = []
    w = BitWriter()
    dynamic_block(w, toks, complete(lit_syms, 286), [8, 8, 7, 6, 5, 4, 3, 2, 1] + [0] * 21, 1, ops)
    kinds = {o[0] for o, _ in ops}
    assert {16, 17, 18} <= kinds and any(o[0] == 16 and o[3] < nlit < o[3] + o[4] for o, nlit in ops), "no repeat crosses into the distances"
    crafted("craft_length_repeats", idx, w.bytes(), raw)

    # a match of length 258 at distance 1 (a flat map)
    idx = np.zeros((8, 300), np.uint8)
    raw = raw_of(idx, 8, [0] * 8)
    toks = tokens_of(raw, dists=(1,))
    assert ("match", 258, 1) in toks
    w = BitWriter()
    dynamic_block(w, toks, complete(used_symbols(toks)[0], 286), complete(used_symbols(toks)[1], 30), 1)
    crafted("craft_len258_dist1", idx, w.bytes(), raw)

    # matches of length 3 at distance 32768 and in the last distance code (13 extra bits), in a map of 33930 bytes
    idx = rng.randint(0, 8, (130, 260)).astype(np.uint8)
    flat = bytearray(raw_of(idx, 8, [0] * 130))
    flat[32773:32776] = flat[5:8]
    flat[32780:32783] = flat[2780:2783]
    raw = bytes(flat)
    idx = np.frombuffer(raw, np.uint8).reshape(130, 261)[:, 1:].copy()
    toks = tokens_of(raw, dists=(), forced={32773: (3, 32768), 32780: (3, 30000)})
    w = BitWriter()
    dynamic_block(w, toks, complete(used_symbols(toks)[0], 286), complete(used_symbols(toks)[1], 30), 1)
    crafted("craft_dist32768_len3", idx, w.bytes(), raw)

    # a stored block of 65535 bytes
    idx = blobs(260, 255, 4, 7)
    raw = raw_of(idx, 8, [0] * 260)
    w = BitWriter()
    stored_block(w, raw[:65535], 0)
    stored_block(w, raw[65535:], 1)
    crafted("craft_stored_65535", idx, w.bytes(), raw)

    # a final fixed block ending exactly on a byte boundary: 3 + 7 bits of frame, 8 bits per value below 144, 9 above: six of those
    idx = np.array([[1, 2, 200, 201, 202, 3, 203, 204, 205, 4]], np.uint8)
    raw = raw_of(idx, 8, [0])
    w = BitWriter()
    fixed_block(w, [("lit", b) for b in raw], 1)
    assert w.n % 8 == 0
    crafted("craft_final_on_byte_boundary", idx, w.bytes(), raw)

    # the three block kinds in one stream; the later blocks reach back into the earlier ones
    idx = blobs(20, 50, 4, 3)
    raw = raw_of(idx, 8)
    toks = tokens_of(raw, dists=(1, 51))
    a, b, cut1, cut2 = 0, 0, 0, 0
    for i, t in enumerate(toks):
        a += 1 if t[0] == "lit" else t[1]
        if a >= 300 and not cut1:
            cut1, b = i + 1, a
        if a >= 700 and not cut2:
            cut2 = i + 1
    w = BitWriter()
    stored_block(w, raw[:b], 0)
    fixed_block(w, toks[cut1:cut2], 0)
    rest = toks[cut2:]
    dynamic_block(w, rest, complete(used_symbols(rest)[0], 286), complete(used_symbols(rest)[1] or [0], 30), 1)
    crafted("craft_three_block_kinds", idx, w.bytes(), raw)

    # a Huffman block that ends with pending literals (7, then 100: neither a multiple of 64) in front of a non-empty stored block, by hand
    # and as zlib writes it when noise follows runs
    idx = np.arange(40, dtype=np.uint8).reshape(4, 10)
    raw = raw_of(idx, 8, [0] * 4)
    w = BitWriter()
    fixed_block(w, [("lit", b) for b in raw[:7]], 0)
    stored_block(w, raw[7:], 1)
    crafted("craft_stored_after_7_literals", idx, w.bytes(), raw)
    idx = rng.randint(0, 256, (12, 30)).astype(np.uint8)
    raw = raw_of(idx, 8, [0] * 12)
    toks = [("lit", b) for b in raw[:100]]
    w = BitWriter()
    dynamic_block(w, toks, complete(used_symbols(toks)[0], 286), [0] * 30, 0)
    stored_block(w, raw[100:200], 0)
    fixed_block(w, [("lit", b) for b in raw[200:]], 1)
    crafted("craft_stored_after_100_literals", idx, w.bytes(), raw)
    idx = np.zeros((120, 400), np.uint8)
    idx[:15, 50:120] = 7
    idx[20:] = rng.randint(0, 256, (100, 400))
    raw = raw_of(idx, 8, [0] * 120)
    ok["gray_runs_then_noise_120x400"] = (png(120, 400, 8, 0, accepted(zlib.compress(raw, 6), raw)), idx)

    # ---- broken files (a small map between the guards of the GPU test): status, then the file
    idx = blobs(12, 20, 4, 5)
    raw = raw_of(idx, 8)
    good = zlib.compress(raw, 9)

    def broken(name, status, z, H=12, W=20):
        bad[f"m{-status}__{name}"] = png(H, W, 8, 3, z)

    broken("wrong_adler", -6, good[:-4] + struct.pack(">I", zlib.adler32(raw) ^ 0x10))
    data = png(12, 20, 8, 3, good)
    at = data.index(b"IDAT") + 4 + len(good)
    bad["m6__wrong_idat_crc"] = data[:at] + bytes([data[at] ^ 1]) + data[at + 1:]
    r5 = bytearray(raw)
    r5[21 * 3] = 5
    broken("filter_byte_5", -7, zlib.compress(bytes(r5), 9))
    broken("truncated_idat", -2, good[:len(good) * 2 // 3])
    w = BitWriter()
    fixed_block(w, [("match", 4, 1)] + [("lit", b) for b in raw[4:]], 1)
    broken("distance_before_start", -4, zwrap(w.bytes(), raw))
    toks = [("lit", b) for b in raw]
    lens = complete(used_symbols(toks)[0], 286)
    over = list(lens)
    over[used_symbols(toks)[0][-2]] = 1
    over[used_symbols(toks)[0][0]] = 1
    over[256] = 1
    w = BitWriter()
    dynamic_block(w, toks, over, [0] * 30, 1)
    broken("oversubscribed_table", -3, zwrap(w.bytes(), raw))
    with_eob = complete(used_symbols(toks)[0] + [257], 286)
    no_eob = list(with_eob)
    no_eob[257], no_eob[256] = with_eob[256], 0           # the end-of-block code's length moves to symbol 257: complete, but no 256
    w = BitWriter()
    try:
        dynamic_block(w, toks, no_eob, [0] * 30, 1)
    except KeyError:
        pass                                              # (the writer cannot spell the end of the block: the header is what matters)
    broken("missing_end_of_block", -3, zwrap(w.bytes() + b"\0" * 8, raw))
    broken("one_row_too_long", -5, zlib.compress(raw + raw[-21:], 9))
    broken("one_row_too_short", -2, zlib.compress(raw[:-21], 9))
    w = BitWriter()                                       # 7 pending literals, then a stored block that runs one row past the map
    fixed_block(w, [("lit", b) for b in raw[:7]], 0)
    stored_block(w, raw[7:] + raw[-21:], 1)
    broken("stored_after_literals_too_long", -5, zwrap(w.bytes(), raw + raw[-21:]))
    w = BitWriter()
    stored_block(w, raw, 1, nlen=(len(raw) ^ 0xffff) ^ 0x0100)
    broken("nlen_mismatch", -1, zwrap(w.bytes(), raw))
    for name, data in bad.items():
        ok_for_zlib = name.split("__")[1] in ("wrong_idat_crc", "filter_byte_5", "one_row_too_long", "one_row_too_short", "stored_after_literals_too_long")
        z = b"".join(data[m + 4:m + 4 + struct.unpack(">I", data[m - 4:m])[0]] for m in [data.index(b"IDAT")])
        try:
            zlib.decompress(z)
            assert ok_for_zlib, name
        except zlib.error:
            assert not ok_for_zlib, name

    # ---- unsupported files: reason, then the file
    idx = blobs(16, 16, 3, 9)
    uns["1__interlaced"] = png(16, 16, 8, 3, zlib.compress(adam7(idx, 8)), interlace=1)
    rgb = np.repeat(idx, 3, axis=1)
    uns["2__rgb"] = png(16, 16, 8, 2, zlib.compress(raw_of(rgb, 8, [0] * 16)))
    uns["3__gray_depth4"] = png(16, 16, 4, 0, zlib.compress(raw_of(idx, 4)))
    uns["4__gray_16bit"] = png(16, 16, 16, 0, zlib.compress(raw_of(np.repeat(idx, 2, axis=1), 8, [0] * 16)))

    # every supported file decodes in Pillow to exactly the indices put in; the interlaced one too (the loaders fall back to it)
    for name, (data, idx) in ok.items():
        got = np.asarray(Image.open(io.BytesIO(data)))
        assert got.shape == idx.shape and (got == idx).all(), name
    assert (np.asarray(Image.open(io.BytesIO(uns["1__interlaced"]))) == blobs(16, 16, 3, 9)).all()
    return ok, bad, uns


def main():
    ok, bad, uns = build()
    arrays = {f"ok__{n}": np.frombuffer(d, np.uint8) for n, (d, _) in ok.items()}
    arrays.update({f"bad__{n}": np.frombuffer(d, np.uint8) for n, d in bad.items()})
    arrays.update({f"uns__{n}": np.frombuffer(d, np.uint8) for n, d in uns.items()})
    np.savez_compressed(OUT, **arrays)
    print(f"{len(ok)} supported, {len(bad)} broken, {len(uns)} unsupported files; {os.path.getsize(OUT)} bytes -> {os.path.normpath(OUT)}")


if __name__ == "__main__":
    sys.exit(main())
