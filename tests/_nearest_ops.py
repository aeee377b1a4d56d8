"""NumPy restatements of the three nearest-neighbour operations of Pillow that the annotation pipeline needs, written from
Pillow's behaviour (Geometry.c ImagingScaleAffine / affine_fixed, Image.rotate) and pinned against Pillow itself by
tests/test_nearest_ops_pillow.py.  The GPU tests use them as their reference, so they need neither Pillow nor a GPU.  Deliberately
independent of timetuning_amd.video_transformations: the table and coefficient builders there are checked against these."""
import math

import numpy as np


def nearest_index(n_in: int, n_out: int) -> np.ndarray:
    """Image.resize(NEAREST) of a line: the source index of every output position (a running double sum, as the C loop)."""
    a0 = n_in / n_out
    xo = a0 * 0.5
    out = np.empty(n_out, np.int64)
    for x in range(n_out):
        out[x] = -1 if xo < 0.0 else int(xo)
        xo += a0
    assert out.min() >= 0 and out.max() < n_in
    return out


def resize_nearest(img: np.ndarray, out_h: int, out_w: int, box=None) -> np.ndarray:
    """``img.crop(box).resize((out_w, out_h), NEAREST)`` for an array [H, W] or [H, W, C]; box = (left, upper, right, lower)."""
    if box is not None:
        img = img[box[1]:box[3], box[0]:box[2]]
    return img[nearest_index(img.shape[0], out_h)][:, nearest_index(img.shape[1], out_w)]


def gather(clip: np.ndarray, ytab, xtab) -> np.ndarray:
    """out[f, y, x] = clip[f, ytab[y], xtab[x]] for a clip [F, H, W] or [F, H, W, C]."""
    return clip[:, np.asarray(ytab)][:, :, np.asarray(xtab)]


def rotate_fixed_coeffs(w: int, h: int, angle: float):
    """Image.rotate(angle)'s affine matrix (defaults: no expand, centre (w / 2, h / 2)) as Geometry.c's six 16.16 integers."""
    angle = angle % 360.0
    r = -math.radians(angle)
    a, b, d, e = round(math.cos(r), 15), round(math.sin(r), 15), round(-math.sin(r), 15), round(math.cos(r), 15)
    cx, cy = w / 2, h / 2
    c = (a * -cx + b * -cy + 0.0) + cx
    f = (d * -cx + e * -cy + 0.0) + cy

    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))

    return fix(a), fix(b), fix(c + a * 0.5 + b * 0.5), fix(d), fix(e), fix(f + d * 0.5 + e * 0.5)


def affine_nearest(img: np.ndarray, coeffs) -> np.ndarray:
    """Geometry.c affine_fixed with the NEAREST filter and zero fill on an array [H, W] or [H, W, C] (output of the same size)."""
    a0, a1, a2, a3, a4, a5 = (int(v) for v in coeffs)
    H, W = img.shape[:2]
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    xin = (a2 + a1 * y + a0 * x) >> 16
    yin = (a5 + a4 * y + a3 * x) >> 16
    ok = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    out = np.zeros_like(img)
    out[ok] = img[yin[ok], xin[ok]]
    return out


def rotate(img: np.ndarray, angle: float) -> np.ndarray:
    """``img.rotate(angle)`` with Pillow's defaults."""
    return affine_nearest(img, rotate_fixed_coeffs(img.shape[1], img.shape[0], angle))


def center_crop_origin(im_h, im_w, h, w):
    return int(round((im_h - h) / 2.)), int(round((im_w - w) / 2.))


def label_clip(fs: int, H: int, W: int, seed: int, objects: int = 4) -> np.ndarray:
    """Integer label maps uint8 [fs, H, W] with several moving objects (labels 1..objects, 255 as a void rim on one of them)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((fs, H, W), np.uint8)
    c = rng.uniform(0.15, 0.85, (objects, 2))
    r = rng.uniform(0.08, 0.22, (objects, 2))
    v = rng.uniform(-0.04, 0.04, (objects, 2))
    for t in range(fs):
        for o in range(objects):
            cy, cx = (c[o, 0] + t * v[o, 0]) * H, (c[o, 1] + t * v[o, 1]) * W
            d = ((yy - cy) / (r[o, 0] * H + 1)) ** 2 + ((xx - cx) / (r[o, 1] * W + 1)) ** 2
            if o == 0:
                out[t][d <= 1.3] = 255
            out[t][d <= 1] = o + 1
    return out


def frame_clip(fs: int, H: int, W: int, seed: int) -> np.ndarray:
    """Textured uint8 frames [fs, H, W, 3]."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    frames = []
    for t in range(fs):
        base = np.stack([127 + 100 * np.sin((xx + 5 * t) / 9.0 + c) * np.cos((yy - 3 * t) / 7.0 + 2 * c) for c in range(3)], -1)
        frames.append(np.clip(base + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8))
    return np.stack(frames)
