"""What the N26 tests share: the fixture tests/golden/png_streams.npz (tools/gen_png_golden.py), Pillow's decode as the yardstick, and a
NumPy statement of the PNG row filters that owes nothing to the code under test."""
import io
import os
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_streams.npz")
# What Pillow 12.2 does with the fixture's broken files, found by running it: it raises OSError on seven of the eleven and ACCEPTS four -
# it never checks the CRC-32 of an IDAT chunk, and it ignores inflated bytes beyond, or missing from, the last row.  The device route is
# stricter there, as the issue lists these files as broken: on such a file png="device" raises where png="host" returns a map.  The tests
# pin both sides.
PILLOW_ACCEPTS = {"wrong_idat_crc", "one_row_too_long", "one_row_too_short", "stored_after_literals_too_long"}


def fixture():
    """-> (ok {name: bytes}, bad {name: (status, bytes)}, uns {name: (reason, bytes)})"""
    z = np.load(GOLDEN)
    ok, bad, uns = {}, {}, {}
    for key in z.files:
        kind, rest = key.split("__", 1)
        data = z[key].tobytes()
        if kind == "ok":
            ok[rest] = data
        elif kind == "bad":
            status, name = rest.split("__", 1)
            bad[name] = (-int(status[1:]), data)
        else:
            reason, name = rest.split("__", 1)
            uns[name] = (int(reason), data)
    return ok, bad, uns


def pillow(data: bytes) -> np.ndarray:
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)))


def pillow_raises(data: bytes) -> bool:
    from PIL import Image

    try:
        Image.open(io.BytesIO(data)).load()
    except (OSError, SyntaxError, ValueError):
        return True
    return False


def idat(data: bytes) -> bytes:
    """The concatenated IDAT payloads of a well-formed file: its zlib stream."""
    at, out = 8, b""
    while at < len(data):
        n, kind = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        if kind == b"IDAT":
            out += data[at + 8:at + 8 + n]
        at += 12 + n
    return out


def unfilter(raw: bytes, H: int, W: int, depth: int):
    """The inflated bytes of an H x W map at ``depth`` bits -> (the unfiltered bytes, each row behind its filter byte, as uint8
    [H, 1 + rb]; the pixels uint8 [H, W]).  None when the length is not H (1 + rb) or a filter byte is above 4."""
    rb = (W * depth + 7) // 8
    if len(raw) != H * (1 + rb):
        return None
    rows = np.frombuffer(raw, np.uint8).reshape(H, 1 + rb).astype(np.int64)
    if (rows[:, 0] > 4).any():
        return None
    prev = np.zeros(rb, np.int64)
    for r in range(H):
        t, x = int(rows[r, 0]), rows[r, 1:]
        if t == 2:
            x[:] = (x + prev) & 255
        elif t != 0:
            a = c = 0
            for i in range(rb):
                b = int(prev[i])
                if t == 1:
                    p = a
                elif t == 3:
                    p = (a + b) >> 1
                else:
                    q = a + b - c
                    pa, pb, pc = abs(q - a), abs(q - b), abs(q - c)
                    p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                a = x[i] = (int(x[i]) + p) & 255
                c = b
        prev = x
    rows = rows.astype(np.uint8)
    bits = np.unpackbits(rows[:, 1:], axis=1)
    pix = np.zeros((H, W), np.uint8)
    for k in range(depth):
        pix |= bits[:, k:W * depth:depth][:, :W] << (depth - 1 - k)
    return rows, pix


def zlib_accepts(stream: bytes):
    """zlib.decompress of a deflate stream as tt_png_prepare leaves it (behind the two-byte header it dropped), or None."""
    try:
        return zlib.decompress(b"\x78\x9c" + stream)
    except zlib.error:
        return None


def _writer():
    """tools/gen_png_golden.py as a module: the hand-built PNG writer."""
    import importlib.util

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "gen_png_golden.py")
    spec = importlib.util.spec_from_file_location("gen_png_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def label_png(idx: np.ndarray, depth: int, interlaced: bool = False) -> bytes:
    """A palette PNG of the indices at ``depth`` bits, filters cycling per row; ``interlaced``: Adam7 (the device decoder does not take it)."""
    G = _writer()
    H, W = idx.shape
    if interlaced:
        return G.png(H, W, depth, 3, zlib.compress(G.adam7(idx, depth)), interlace=1)
    return G.png(H, W, depth, 3, zlib.compress(G.raw_of(idx, depth), 9), split=97)


def write_video_tree(root, videos: int = 3, frames: int = 4, H: int = 24, W: int = 32):
    """<root>/JPEGImages/video<v>/0000<f>.jpg and <root>/Annotations/video<v>/0000<f>.png: palette maps of depth 1 / 2 / 4 / 8 by turns, the
    map of (video 1, frame 2) interlaced.  Returns {(v, f): the indices}."""
    from PIL import Image

    yy, xx = np.mgrid[0:H, 0:W]
    maps, k = {}, 0
    for v in range(videos):
        os.makedirs(os.path.join(root, "JPEGImages", f"video{v}"))
        os.makedirs(os.path.join(root, "Annotations", f"video{v}"))
        for f in range(frames):
            depth = (1, 2, 4, 8)[k % 4]
            k += 1
            idx = np.zeros((H, W), np.uint8)
            idx[3 + f:14 + f, 2 + 3 * v:15 + 3 * v] = 1
            if depth > 1:
                idx[10:20, 20 - f:30 - f] = min(3, (1 << depth) - 1)
            rgb = np.stack([(idx * 70 + xx * 3 + 9 * f) % 256, (yy * 7 + 50 * v) % 256, (xx + yy + 31 * idx) % 256], axis=-1).astype(np.uint8)
            Image.fromarray(rgb).save(os.path.join(root, "JPEGImages", f"video{v}", f"{f:05d}.jpg"), quality=90)
            with open(os.path.join(root, "Annotations", f"video{v}", f"{f:05d}.png"), "wb") as out:
                out.write(label_png(idx, depth, interlaced=(v, f) == (1, 2)))
            maps[(v, f)] = idx
    return maps
