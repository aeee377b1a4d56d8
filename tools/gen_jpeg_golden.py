#!/usr/bin/env python
"""Writes tests/golden/jpeg_frames.npz: JPEG files encoded by Pillow and Pillow's own decode of them, the yardstick of the N21 decoder
(tests/test_jpeg_host.py, tests/test_hip_jpeg.py).  Needs Pillow; the tests that read the fixture do not.

  names        the cases, in order
  blob, offs   the files' bytes, concatenated: case i is blob[offs[i]:offs[i + 1]]
  pix          per case the index of its decoded pixels, -1 where none are kept (grayscale / CMYK: classification only)
  pblob, pshape, poffs   the decoded uint8 [H, W, 3] arrays, each stored as filtered() leaves it, concatenated (the three encodings of one grid image - default tables,
                optimize=True, a restart interval of 3 MCUs - hold the same coefficients and share one array; the generator checks it)
  ann_names, ann_blob, ann_offs, ann_idx   palette PNG annotations of the clip frames and their index maps [10, 48, 64]
"""
import io
import os
import sys

import numpy as np
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (8, 8), (9, 15), (16, 16), (17, 33), (40, 24), (37, 53)]          # H x W
SAMPLINGS = {"444": 0, "422": 1, "420": 2}                                        # Pillow's subsampling argument
QUALITIES = [30, 75, 95, 100]
VARIANTS = {"std": {}, "opt": {"optimize": True}, "rst": {"restart_marker_blocks": 3}}


def picture(h, w, seed, noise=1.0, rects=None, flat=False):
    """Smooth ramps, a few flat rectangles with hard edges and mild noise: every coefficient band and both clamps get exercised."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.empty((h, w, 3))
    for c in range(3):
        fy, fx, ph = rng.uniform(0.5, 3.0, 3)
        img[..., c] = rng.integers(40, 216) if flat else 128 + 110 * np.sin(fy * yy / max(h, 8) * np.pi + ph) * np.cos(fx * xx / max(w, 8) * np.pi + c)
    for _ in range(max(2, h * w // 600) if rects is None else rects):
        y0, x0 = rng.integers(0, h), rng.integers(0, w)
        y1, x1 = y0 + rng.integers(1, max(2, h // 3 + 1)), x0 + rng.integers(1, max(2, w // 3 + 1))
        img[y0:y1, x0:x1] = rng.integers(0, 256, 3)
    if noise:
        img += rng.normal(0, noise, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def big_frame():
    """The workload's frame size once: flat ground and flat rectangles (their decode deflates well, the fixture has a size limit) around
    one textured corner."""
    img = picture(360, 480, 903, noise=0, rects=16, flat=True)
    img[200:264, 300:364] = picture(64, 64, 904, noise=2.0)
    return img


def encode(arr, **kw):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", **kw)
    return buf.getvalue()


def decoded(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def filtered(p):
    """uint8 [H, W, 3] -> planar [3, H, W] with every row replaced by its differences modulo 256 (PNG's "sub" filter: decoded photographs
    deflate to a third this way).  The readers undo it with a cumulative sum along the last axis."""
    q = np.ascontiguousarray(p.transpose(2, 0, 1))
    out = q.copy()
    out[..., 1:] = q[..., 1:] - q[..., :-1]
    return out


def main():
    names, files, pix, pixels = [], [], [], []

    def add(name, data, keep=True, share=None):
        names.append(name)
        files.append(data)
        if not keep:
            pix.append(-1)
            return
        d = decoded(data)
        if share is not None:
            assert np.array_equal(pixels[share], d), name
            pix.append(share)
        else:
            pix.append(len(pixels))
            pixels.append(d)

    seed = 0
    for h, w in SIZES:
        for sname, sub in SAMPLINGS.items():
            for q in QUALITIES:
                seed += 1
                arr, first = picture(h, w, seed), None
                for vname, kw in VARIANTS.items():
                    add(f"grid_{h}x{w}_{sname}_q{q}_{vname}", encode(arr, quality=q, subsampling=sub, **kw), share=first)
                    first = pix[-1]
    yy, xx = np.mgrid[0:16, 0:16]
    checker = np.stack([((yy + xx) % 2) * 255, ((yy // 2 + xx) % 2) * 255, ((yy + xx // 2) % 2) * 255], -1).astype(np.uint8)
    for sname, sub in SAMPLINGS.items():
        add(f"checker_16x16_{sname}_q100", encode(checker, quality=100, subsampling=sub))
    add("strip_64x8_420_q75", encode(picture(64, 8, 901), quality=75, subsampling=2))
    add("strip_8x64_420_q75", encode(picture(8, 64, 902), quality=75, subsampling=2))
    add("frame_360x480_420_q90", encode(big_frame(), quality=90, subsampling=2))
    ann_names, ann_files, ann_idx = [], [], []
    palette = [int(v) for v in np.random.default_rng(5).integers(0, 256, 768)]
    for v in range(2):
        for f in range(5):
            arr = np.roll(picture(48, 64, 1000 + v, noise=0, rects=6, flat=True), 3 * f, axis=1)
            add(f"clip_v{v}_f{f}", encode(arr, quality=90, subsampling=2 - v))
            lab = np.zeros((48, 64), np.uint8)
            lab[8 + v:30, 5 + 3 * f:25 + 3 * f] = 1 + v
            lab[20:44, 40 - 2 * f:60 - 2 * f] = 3
            im = Image.fromarray(lab, "P")
            im.putpalette(palette)
            buf = io.BytesIO()
            im.save(buf, "PNG")
            ann_names.append(f"clip_v{v}_f{f}")
            ann_files.append(buf.getvalue())
            ann_idx.append(lab)
    base = picture(48, 64, 1000, noise=0, rects=6, flat=True)
    add("prog_48x64_420_q90", encode(np.roll(base, 6, axis=1), quality=90, subsampling=2, progressive=True))
    add("gray_16x16_q75", encode(picture(16, 16, 950)[..., 0], quality=75), keep=False)
    buf = io.BytesIO()
    Image.fromarray(picture(16, 16, 951)).convert("CMYK").save(buf, "JPEG", quality=75)
    add("cmyk_16x16_q75", buf.getvalue(), keep=False)

    cat = lambda blobs: (np.frombuffer(b"".join(blobs), np.uint8), np.cumsum([0] + [len(b) for b in blobs]).astype(np.int64))
    blob, offs = cat(files)
    pblob, poffs = cat([filtered(p).tobytes() for p in pixels])
    ann_blob, ann_offs = cat(ann_files)
    out = os.path.join(REPO, "tests", "golden", "jpeg_frames.npz")
    np.savez_compressed(out, names=np.array(names), blob=blob, offs=offs, pix=np.array(pix, np.int32), pblob=pblob, poffs=poffs,
                        pshape=np.array([p.shape[:2] for p in pixels], np.int32), ann_names=np.array(ann_names), ann_blob=ann_blob,
                        ann_offs=ann_offs, ann_idx=np.stack(ann_idx))
    size = os.path.getsize(out)
    print(f"{out}: {len(names)} files, {len(pixels)} pixel arrays, {size} bytes")
    assert size < 300 * 1024, "the fixture must stay under 300 KB"
    return 0


if __name__ == "__main__":
    sys.exit(main())
