"""Pillow is the judge of the nearest-neighbour arithmetic: the NumPy restatements of tests/_nearest_ops.py (the reference of the
GPU tests) and the host builders of timetuning_amd.video_transformations (what the kernels are fed) against Pillow itself, bit for
bit, with no case excused.  No GPU needed."""
import os
import random
import sys

import numpy as np
import pytest

Image = pytest.importorskip("PIL.Image")

from timetuning_amd import video_transformations as VT  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nearest_ops as NO  # noqa: E402


def _image(rng, h, w, mode):
    return rng.integers(0, 256, (h, w) if mode == "L" else (h, w, 3), dtype=np.uint8)


def _resize_cases():
    """(h, w, out_h, out_w, box or None): 1-pixel sides, identity, up- and down-scaling, then seeded shapes, a third of them cropped."""
    cases = [(1, 1, 1, 1, None), (1, 1, 7, 5, None), (1, 9, 4, 1, None), (9, 1, 1, 4, None), (5, 7, 1, 1, None), (1, 40, 1, 13, None),
             (40, 1, 13, 1, None), (16, 16, 16, 16, None), (10, 12, 20, 24, None), (20, 24, 10, 12, None), (13, 29, 224, 224, None),
             (360, 480, 224, 224, None), (480, 854, 448, 448, None), (37, 223, 100, 500, None)]
    rng = np.random.default_rng(11)
    for n in range(330):
        h, w = (int(v) for v in rng.integers(1, 200, 2))
        oh, ow = (int(v) for v in rng.integers(1, 260, 2))
        box = None
        if n % 3 == 0:
            l, u = int(rng.integers(0, w)), int(rng.integers(0, h))
            box = (l, u, int(rng.integers(l + 1, w + 1)), int(rng.integers(u + 1, h + 1)))
        cases.append((h, w, oh, ow, box))
    return cases


def test_nearest_resize_matches_pillow():
    cases = _resize_cases()
    assert len(cases) >= 300
    rng = np.random.default_rng(5)
    for n, (h, w, oh, ow, box) in enumerate(cases):
        mode = "L" if n % 2 else "RGB"
        a = _image(rng, h, w, mode)
        img = Image.fromarray(a, mode)
        if box is not None:
            img = img.crop(box)
        want = np.array(img.resize((ow, oh), Image.NEAREST))
        assert np.array_equal(NO.resize_nearest(a, oh, ow, box), want), (h, w, oh, ow, box, mode)
        l, u, r, b = box if box is not None else (0, 0, w, h)
        ytab, xtab = VT.nearest_table(b - u, oh, u), VT.nearest_table(r - l, ow, l)
        assert ytab.dtype == np.int32 and xtab.dtype == np.int32
        assert np.array_equal(a[ytab][:, xtab], want), (h, w, oh, ow, box, mode)


def test_nearest_table_is_not_the_multiply_form():
    """The running sum and ``floor(a0 / 2 + x * a0)`` part ways (320 -> 224: 20 positions); the table must follow Pillow's sum."""
    n_in, n_out = 320, 224
    a = np.arange(n_in, dtype=np.int32).reshape(1, n_in)
    want = np.array(Image.fromarray(a, "I").resize((n_out, 1), Image.NEAREST))[0]
    mult = np.floor((n_in / n_out) * 0.5 + np.arange(n_out) * (n_in / n_out)).astype(np.int64)
    assert int((want != mult).sum()) == 20
    assert np.array_equal(VT.nearest_table(n_in, n_out), want)
    assert np.array_equal(NO.nearest_index(n_in, n_out), want)


def _rotate_cases():
    sizes = [(64, 64), (48, 80), (80, 48), (33, 33), (1, 1), (1, 17), (17, 1), (37, 91)]
    cases = [(h, w, float(a)) for (h, w) in sizes[:4] for a in (0, 90, -90, 180, 270, 360, -180, 450, 1e-14, 45, -45)]
    rng = np.random.default_rng(23)
    for n in range(220):
        h, w = sizes[n % len(sizes)]
        cases.append((h, w, float(rng.uniform(-400, 400))))
    return cases


def test_rotate_matches_pillow():
    cases = _rotate_cases()
    assert len(cases) >= 200
    rng = np.random.default_rng(7)
    for n, (h, w, angle) in enumerate(cases):
        mode = "L" if n % 2 else "RGB"
        a = _image(rng, h, w, mode)
        want = np.array(Image.fromarray(a, mode).rotate(angle))
        assert np.array_equal(NO.rotate(a, angle), want), (h, w, angle, mode)
        coeffs = VT.rotate_coeffs(w, h, angle)
        assert coeffs == NO.rotate_fixed_coeffs(w, h, angle)
        assert np.array_equal(NO.affine_nearest(a, coeffs), want), (h, w, angle, mode)


def test_flips_match_transpose():
    rng = np.random.default_rng(9)
    for (h, w) in ((1, 1), (1, 6), (6, 1), (17, 30), (64, 48)):
        for mode in ("L", "RGB"):
            a = _image(rng, h, w, mode)
            img = Image.fromarray(a, mode)
            ident_y, ident_x = VT.nearest_table(h, h), VT.nearest_table(w, w)
            assert np.array_equal(ident_y, np.arange(h)) and np.array_equal(ident_x, np.arange(w))
            lr = a[ident_y][:, VT.nearest_table(w, w, flip=True)]
            tb = a[VT.nearest_table(h, h, flip=True)][:, ident_x]
            assert np.array_equal(lr, np.array(img.transpose(Image.FLIP_LEFT_RIGHT)))
            assert np.array_equal(tb, np.array(img.transpose(Image.FLIP_TOP_BOTTOM)))
    # crop + resize + flip in one table
    a = _image(rng, 40, 50, "L")
    want = np.array(Image.fromarray(a, "L").crop((7, 3, 45, 33)).resize((21, 19), Image.NEAREST).transpose(Image.FLIP_LEFT_RIGHT))
    assert np.array_equal(a[VT.nearest_table(30, 19, 3)][:, VT.nearest_table(38, 21, 7, flip=True)], want)


def test_crop_origins_match_pillow_crop():
    rng = np.random.default_rng(13)
    for n in range(60):
        h, w = (int(v) for v in rng.integers(1, 90, 2))
        ch, cw = int(rng.integers(1, h + 1)), int(rng.integers(1, w + 1))
        a = _image(rng, h, w, "L" if n % 2 else "RGB")
        img = Image.fromarray(a)
        # CenterCrop (:596-601)
        y1, x1 = VT.center_crop_origin(h, w, ch, cw)
        assert (y1, x1) == NO.center_crop_origin(h, w, ch, cw) == (int(round((h - ch) / 2.)), int(round((w - cw) / 2.)))
        assert np.array_equal(a[y1:y1 + ch, x1:x1 + cw], np.array(img.crop((x1, y1, x1 + cw, y1 + ch))))
        # RandomCrop (:410-419): x1 is drawn first
        random.seed(n)
        y1, x1 = VT.random_crop_origin(h, w, ch, cw)
        random.seed(n)
        rx = random.randint(0, w - cw)
        ry = random.randint(0, h - ch)
        assert (y1, x1) == (ry, rx)
        assert np.array_equal(a[y1:y1 + ch, x1:x1 + cw], np.array(img.crop((x1, y1, x1 + cw, y1 + ch))))
    assert VT.center_crop_origin(10, 11, 5, 6) == (2, 2)      # 2.5 rounds half to even
    assert VT.center_crop_origin(12, 13, 5, 6) == (4, 4)      # 3.5 -> 4
    with pytest.raises(ValueError):
        VT.center_crop_origin(4, 9, 5, 3)
    with pytest.raises(ValueError):
        VT.random_crop_origin(9, 4, 3, 5)
