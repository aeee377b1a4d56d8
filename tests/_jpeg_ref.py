"""NumPy restatement of a baseline JPEG decode as Pillow's bundled libjpeg-turbo performs it with its defaults (accurate integer
IDCT, triangle-filter chroma up-sampling, 16-bit fixed-point colour tables) - the yardstick of tt_jpeg_scan and tt_jpeg_decode_batch.
Written from the JPEG standard's stream layout and the arithmetic rules of DESIGN.md N21; nothing here is fast, and nothing has to be.

  parse(data)   -> Parsed: H, W, sampling code, per-component block grids, quantisation tables and coefficients (natural order)
  decode(data)  -> uint8 [H, W, 3], bit-equal to np.asarray(Image.open(...).convert("RGB")) for the supported files
Unsupported / malformed input raises ValueError: the fixtures are all supported files.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62,
                   63])   # zigzag position -> natural (row-major) position
SAMPLING = {(1, 1): 0, (2, 1): 1, (2, 2): 2}   # luma (h, v) -> the sampling code: 4:4:4, 4:2:2, 4:2:0


@dataclass
class Parsed:
    H: int
    W: int
    sampling: int
    hv: list            # (h, v) per component
    grids: list         # (block rows, block columns) per component
    qtables: np.ndarray  # uint16 [3, 64], natural order, the table OF each component
    coeffs: list        # int16 [rows, cols, 64] per component, natural order


def _huffman(bits, vals):
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


class _Bits:
    def __init__(self, data: bytes):
        self.acc = int.from_bytes(data, "big") if data else 0
        self.left = 8 * len(data)

    def get(self, n):
        if n == 0:
            return 0
        if n > self.left:
            raise ValueError("scan data ends early")
        self.left -= n
        return (self.acc >> self.left) & ((1 << n) - 1)

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.get(1)
            v = table.get((length, code))
            if v is not None:
                return v
        raise ValueError("bad Huffman code")


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _intervals(data: bytes, pos: int):
    """The entropy-coded bytes from `pos` on, un-stuffed and split at the RSTn markers; (segments, the markers' numbers)."""
    segs, marks, cur = [], [], bytearray()
    n = len(data)
    while pos < n:
        b = data[pos]
        if b != 0xFF:
            cur.append(b)
            pos += 1
            continue
        if pos + 1 >= n:
            break
        b2 = data[pos + 1]
        if b2 == 0x00:
            cur.append(0xFF)
            pos += 2
        elif b2 == 0xFF:
            pos += 1
        elif 0xD0 <= b2 <= 0xD7:
            segs.append(bytes(cur))
            marks.append(b2 - 0xD0)
            cur = bytearray()
            pos += 2
        else:
            break
    segs.append(bytes(cur))
    return segs, marks


def parse(data: bytes) -> Parsed:
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    pos, qt, huff, frame, restart = 2, {}, {}, None, 0
    while True:
        while data[pos] == 0xFF and data[pos + 1] == 0xFF:
            pos += 1
        if data[pos] != 0xFF:
            raise ValueError("marker expected")
        marker = data[pos + 1]
        length = int.from_bytes(data[pos + 2:pos + 4], "big")
        seg = data[pos + 4:pos + 2 + length]
        pos += 2 + length
        if marker == 0xDB:
            i = 0
            while i < len(seg):
                if seg[i] >> 4:
                    raise ValueError("16-bit quantisation table")
                t = np.zeros(64, np.uint16)
                t[ZIGZAG] = np.frombuffer(seg[i + 1:i + 65], np.uint8)
                qt[seg[i] & 15] = t
                i += 65
        elif marker == 0xC4:
            i = 0
            while i < len(seg):
                bits = list(seg[i + 1:i + 17])
                vals = list(seg[i + 17:i + 17 + sum(bits)])
                huff[seg[i]] = _huffman(bits, vals)
                i += 17 + sum(bits)
        elif marker in (0xC0, 0xC1):
            if seg[0] != 8 or seg[5] != 3:
                raise ValueError("not 8-bit three-component")
            H, W = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big")
            frame = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(3)]
        elif marker == 0xDD:
            restart = int.from_bytes(seg[:2], "big")
        elif marker == 0xDA:
            if seg[0] != 3:
                raise ValueError("not one interleaved scan")
            tabs = [(seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(3)]
            break
        elif 0xC0 <= marker <= 0xCF and marker not in (0xC4, 0xC8):
            raise ValueError("unsupported frame type")
    hv = [(h, v) for _, h, v, _ in frame]
    if hv[0] not in SAMPLING or hv[1] != (1, 1) or hv[2] != (1, 1):
        raise ValueError("unsupported sampling")
    hmax, vmax = hv[0]
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    grids = [(my * v, mx * h) for h, v in hv]
    coeffs = [np.zeros((r, c, 64), np.int16) for r, c in grids]
    segs, marks = _intervals(data, pos)
    per = restart if restart else mx * my
    if len(segs) < -(-mx * my // per) or any(m != i % 8 for i, m in enumerate(marks)):
        raise ValueError("restart markers")
    mcu = 0
    for seg in segs:
        if mcu >= mx * my:
            break
        bits, pred = _Bits(seg), [0, 0, 0]
        for _ in range(min(per, mx * my - mcu)):
            row, col = divmod(mcu, mx)
            for c, (h, v) in enumerate(hv):
                dc, ac = huff[tabs[c][0]], huff[0x10 | tabs[c][1]]
                for y in range(v):
                    for x in range(h):
                        blk = coeffs[c][row * v + y, col * h + x]
                        s = bits.symbol(dc)
                        pred[c] += _extend(bits.get(s), s)
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = bits.symbol(ac)
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            if k > 63:
                                raise ValueError("run past coefficient 63")
                            blk[ZIGZAG[k]] = _extend(bits.get(s), s)
                            k += 1
            mcu += 1
    q = np.stack([qt[f[3]] for f in frame])
    return Parsed(H, W, SAMPLING[hv[0]], hv, grids, q, coeffs)


def _pass(x, shift):
    """One 1-D pass over the LAST axis of an int64 array [..., 8]."""
    x0, x1, x2, x3, x4, x5, x6, x7 = (x[..., i] for i in range(8))
    z1 = (x2 + x6) * 4433
    t2 = z1 - x6 * 15137
    t3 = z1 + x2 * 6270
    t0 = (x0 + x4) << 13
    t1 = (x0 - x4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = x7, x5, x3, x1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3 = -z3 * 16069 + z5
    z4 = -z4 * 3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3], axis=-1)
    return (out + (1 << (shift - 1))) >> shift


def idct_plane(coeffs: np.ndarray, q: np.ndarray) -> np.ndarray:
    """int16 [rows, cols, 64] and uint16 [64] -> the uint8 plane [8 rows, 8 cols] of the whole block grid."""
    rows, cols = coeffs.shape[:2]
    x = (coeffs.astype(np.int64) * q.astype(np.int64)).reshape(rows, cols, 8, 8)
    x = _pass(x.swapaxes(-1, -2), 11).swapaxes(-1, -2)      # columns
    x = _pass(x, 18)                                       # rows
    x = np.clip(x + 128, 0, 255).astype(np.uint8)
    return x.transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8)


def _upsample_h2v1(p):
    p = p.astype(np.int64)
    left = np.concatenate([p[:, :1], p[:, :-1]], 1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    return out


def _upsample_h2v2(p):
    p = p.astype(np.int64)
    up = np.concatenate([p[:1], p[:-1]], 0)
    down = np.concatenate([p[1:], p[-1:]], 0)
    out = np.empty((2 * p.shape[0], 2 * p.shape[1]), np.int64)
    for parity, nbr in ((0, up), (1, down)):
        s = 3 * p + nbr
        left = np.concatenate([s[:, :1], s[:, :-1]], 1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
        out[parity::2, 0::2] = (3 * s + left + 8) >> 4
        out[parity::2, 1::2] = (3 * s + right + 7) >> 4
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def reconstruct(p: Parsed) -> np.ndarray:
    H, W = p.H, p.W
    hmax, vmax = p.hv[0]
    planes = [idct_plane(p.coeffs[c], p.qtables[c]) for c in range(3)]
    y = planes[0][:H, :W].astype(np.int64)
    dh, dw = -(-H // vmax), -(-W // hmax)
    chroma = []
    for c in (1, 2):
        pl = planes[c][:dh, :dw]
        if p.sampling == 1:
            pl = _upsample_h2v1(pl)
        elif p.sampling == 2:
            pl = _upsample_h2v2(pl)
        chroma.append(np.asarray(pl, np.int64)[:H, :W] - 128)
    cb, cr = chroma
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb - _fix(0.71414) * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data: bytes) -> np.ndarray:
    return reconstruct(parse(data))


def fixture(path):
    """tests/golden/jpeg_frames.npz (tools/gen_jpeg_golden.py) -> ({name: (bytes, uint8 [H, W, 3] or None)}, {name: (PNG bytes, uint8 [H, W])})."""
    g = np.load(path)
    pixels = []
    for k, (h, w) in enumerate(g["pshape"]):
        planar = g["pblob"][g["poffs"][k]:g["poffs"][k + 1]].reshape(3, h, w)
        pixels.append(np.ascontiguousarray(np.cumsum(planar, axis=-1, dtype=np.uint8).transpose(1, 2, 0)))   # undoes the row differences
    files = {}
    for i, name in enumerate(g["names"]):
        k = int(g["pix"][i])
        files[str(name)] = (g["blob"][g["offs"][i]:g["offs"][i + 1]].tobytes(), pixels[k] if k >= 0 else None)
    anns = {str(name): (g["ann_blob"][g["ann_offs"][i]:g["ann_offs"][i + 1]].tobytes(), g["ann_idx"][i]) for i, name in enumerate(g["ann_names"])}
    return files, anns
