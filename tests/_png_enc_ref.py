"""N29: a plain-Python restatement of the device PNG writer's byte format - the chunk rule, the run tokens, the fixed code of RFC 1951
3.2.6, the sync-flush framing, the Adler-32 and the file wrapper - written from the format's description and the RFC, not from the
C++; and the list of maps the encoder tests share (the smallest shapes at which each part can go wrong)."""
import struct
import zlib
from functools import lru_cache

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]


def rows_per_chunk(H, W):
    return max(1, min(H, 16384 // (W + 1)))


def filtered_image(x):
    """uint8 [H, W] -> uint8 [H, W + 1]: filter type 2, then the difference to the row above (zeros above row 0), modulo 256"""
    x = np.asarray(x, np.uint8)
    up = np.vstack([np.zeros((1, x.shape[1]), np.uint8), x[:-1]])
    return np.hstack([np.full((x.shape[0], 1), 2, np.uint8), x - up])


class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, count):
        """`count` bits of `value`, least significant first (header fields, extra bits)"""
        self.acc |= value << self.n
        self.n += count

    def put_code(self, code, count):
        """a Huffman code: most significant bit first"""
        for k in range(count - 1, -1, -1):
            self.put((code >> k) & 1, 1)

    def align(self):
        self.n = (self.n + 7) // 8 * 8

    def bytes(self):
        assert self.n % 8 == 0
        return self.acc.to_bytes(self.n // 8, "little")


def put_symbol(w, sym):
    """one symbol of the fixed literal/length code"""
    if sym < 144:
        w.put_code(0b00110000 + sym, 8)
    elif sym < 256:
        w.put_code(0b110010000 + sym - 144, 9)
    elif sym < 280:
        w.put_code(sym - 256, 7)
    else:
        w.put_code(0b11000000 + sym - 280, 8)


def put_match(w, length):
    idx = max(i for i in range(29) if LEN_BASE[i] <= length)
    if length == 258:
        idx = 28
    put_symbol(w, 257 + idx)
    w.put(length - LEN_BASE[idx], LEN_EXTRA[idx])
    w.put_code(0, 5)                                   # distance code 0 = distance 1, no extra bits


def runs(data):
    data = np.asarray(data, np.uint8)
    starts = np.flatnonzero(np.concatenate([[True], data[1:] != data[:-1]]))
    lengths = np.diff(np.concatenate([starts, [data.size]]))
    return [(int(data[s]), int(n)) for s, n in zip(starts, lengths)]


def chunk_stream(data, last):
    w = BitWriter()
    w.put(0, 1)                                        # BFINAL
    w.put(1, 2)                                        # BTYPE 01
    for b, L in runs(data):
        put_symbol(w, b)
        rem = L - 1
        while rem >= 3:
            m = min(rem, 258)
            put_match(w, m)
            rem -= m
        for _ in range(rem):
            put_symbol(w, b)
    put_symbol(w, 256)
    w.put(1 if last else 0, 1)
    w.put(0, 2)                                        # BTYPE 00
    w.align()
    return w.bytes() + b"\x00\x00\xff\xff"


def chunks_of(x):
    H, W = x.shape
    rpc = rows_per_chunk(H, W)
    f = filtered_image(x)
    return [f[r:r + rpc].reshape(-1) for r in range(0, H, rpc)]


def stream(x):
    """(the deflate stream of the map, the Adler-32 of its filtered bytes, its capacity by the rule (9 n + 7) / 8 + 7 per chunk)"""
    parts = chunks_of(np.asarray(x, np.uint8))
    out = b"".join(chunk_stream(p, k == len(parts) - 1) for k, p in enumerate(parts))
    return out, zlib.adler32(filtered_image(x).tobytes()), sum((9 * p.size + 7) // 8 + 7 for p in parts)


def png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def png_file(x, palette=None):
    x = np.asarray(x, np.uint8)
    s, adler, _ = stream(x)
    out = SIGNATURE + png_chunk(b"IHDR", struct.pack(">IIBBBBB", x.shape[1], x.shape[0], 8, 3 if palette is not None else 0, 0, 0, 0))
    if palette is not None:
        out += png_chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    return out + png_chunk(b"IDAT", b"\x78\x01" + s + struct.pack(">I", adler)) + png_chunk(b"IEND", b"")


def idat_payload(data):
    """the concatenated IDAT payloads of a file"""
    at, out = 8, b""
    while at < len(data):
        n, kind = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        if kind == b"IDAT":
            out += data[at + 8:at + 8 + n]
        at += 12 + n
    return out


# ---- the map list

RUNS = (1, 2, 3, 4, 258, 259, 260, 261, 262, 517, 520)


def run_row(values):
    """one row built of runs of the lengths RUNS, their values cycling through ``values`` (neighbours differ)"""
    return np.concatenate([np.full(n, values[k % len(values)], np.uint8) for k, n in enumerate(RUNS)])[None, :]


def blob_map(H, W, seed, objects=4):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), np.uint8)
    for o in range(1, objects + 1):
        for _ in range(2):
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            ry, rx = rng.uniform(0.05, 0.25) * H + 1, rng.uniform(0.05, 0.25) * W + 1
            m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = o
    return m


def straddle_map():
    """400 x 99: rows of 100 filtered bytes, 163 rows per chunk, three chunks.  Built from its FILTERED bytes (noise, integrated down the
    columns into pixels) so that runs of 300 equal filtered bytes lie where they can go wrong: across the first chunk boundary (the
    encoder must cut it there), across position 256 of the second chunk, across position 64 (and so 256) of the third, and across
    positions 8192 and 4096, where a 256-thread workgroup that owns 64 positions per thread passes from one wave to the next.  The runs
    are of the byte 2, which joins the rows' filter bytes: they cross row starts."""
    H, W = 400, 99
    n = rows_per_chunk(H, W) * (W + 1)
    rng = np.random.default_rng(29)
    f = rng.integers(0, 256, (H, W + 1)).astype(np.uint8)
    f[:, 0] = 2
    flat = f.reshape(-1)
    for at in (n - 150, n + 200, n + 8192 - 100, 2 * n + 10, 2 * n + 4096 - 290):
        flat[at:at + 300] = 2
    return np.cumsum(f[:, 1:].astype(np.int64), 0).astype(np.uint8)


@lru_cache(maxsize=None)
def map_list():
    """name -> uint8 [H, W], seeded"""
    rng = np.random.default_rng(2029)
    rpc = rows_per_chunk(10 ** 6, 100)
    maps = {
        "1x1": np.array([[7]], np.uint8), "1x2": np.array([[0, 200]], np.uint8), "2x1": np.array([[255], [3]], np.uint8),
        "runs": run_row((5, 9, 77)),
        "runs_code_boundary": run_row((2, 143, 144, 255)),         # the first run joins the row's filter byte
        "zeros_40x300": np.zeros((40, 300), np.uint8), "max_40x300": np.full((40, 300), 255, np.uint8),
        "alternating_rows": np.where(np.arange(50)[:, None] % 2 == 0, 200, 10).astype(np.uint8) * np.ones((1, 70), np.uint8),
        "straddle": straddle_map(),
        "1x32767": np.repeat(rng.integers(0, 256, 700).astype(np.uint8), 47)[None, :32767].copy(),
        "16384x1": (rng.integers(0, 3, (16384, 1)) * 90).astype(np.uint8),
        "noise_64x100": rng.integers(144, 256, (64, 100)).astype(np.uint8),
        "blob_480x854": blob_map(480, 854, 1), "blob_375x500": blob_map(375, 500, 2),
    }
    for H in (rpc - 1, rpc, rpc + 1):
        maps[f"rows_{H}x100"] = blob_map(H, 100, H, 3)
    # Up turns pixel noise in 144..255 into differences of which half are below 144 again (8-bit codes); the capacity bound is reached
    # by FILTERED bytes of 9-bit codes, so a second noise map is the first one integrated down its columns
    maps["noise9_64x100"] = np.cumsum(maps["noise_64x100"].astype(np.int64), 0).astype(np.uint8)
    maps["noise9_1x32767"] = rng.integers(144, 256, (1, 32767)).astype(np.uint8)     # the largest chunk at its capacity
    assert maps["1x32767"].shape == (1, 32767)
    return maps


def palette(n=256, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)
