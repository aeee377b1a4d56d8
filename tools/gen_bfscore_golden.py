#!/usr/bin/env python3
"""Writes tests/golden/bfscore.npz from the reference's own boundary F-score (N8, ``bfscore.py``).

Runs on the CPU of the build container, next to a reference checkout (``oracle/gen_golden.py``'s stand-ins for the third-party
imports; ``cv2.__version__`` is set on the cv2 stand-in, which the module reads at import), with ``MKL_CBWR=COMPATIBLE`` like every
golden here:

    MKL_CBWR=COMPATIBLE python tools/gen_bfscore_golden.py

cv2 is not installed.  ``bfscore`` calls ``cv2.findContours`` (RETR_LIST, CHAIN_APPROX_NONE), ``cv2.contourArea`` and
``cv2.drawContours``; they are replaced by tests/_border_follow.py, a restatement of Suzuki-Abe border following written from the
published algorithm (the areas and the drawing feed nothing the fixture keeps).  The fixture pins the reference's own code around
them but NOT cv2 itself: "parity unpinned", as N1's and N7's stand-ins.

Inputs come from ``make_*`` below and are NOT stored whole: only samples the tests check they regenerate, except the hand-made cases.
Cases:
  - ``cbfe``: 8 CBFE-like images at 100 x 100 (ellipses, 255 borders and holes, noise; masks 0 / 1 from perturbed foreground, one
    single-valued mask, one mask with a value 2, one all-void annotation): ``evaluate_bf_score`` per image and overall, t = 16
  - ``multi``: 3 multi-class label maps 40 x 50 (classes 0..4, one class only in gt, one only in pr): ``bfscore`` at t = 2, 2.5, 5, 16
  - ``row`` / ``col``: 1 x 61 and 61 x 1 label maps, t = 2 and 5
  - hand-made, stored whole (``hand_<name>_gt`` / ``_pr``, t = 2): a single pixel, a 3-pixel line, a 1-pixel ring, an X, a
    checkerboard, all foreground, an empty gt with a non-empty pred (the ``[nan]`` path); and a single-valued pred through
    ``evaluate_bf_score`` (score 0)
"""
from __future__ import annotations

import contextlib
import io
import os
import sys

os.environ.setdefault("MKL_CBWR", "COMPATIBLE")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle"))   # timet_oracle, which oracle.gen_golden's stand-ins import by that name
sys.path.insert(0, os.path.join(REPO, "tests"))    # _border_follow
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

CBFE = (8, 100, 100, 21)        # N, H, W, seed
MULTI = (3, 40, 50, 22)         # maps, H, W, seed
MULTI_TH = (2, 2.5, 5, 16)
LINE_TH = (2, 5)
LINE_LEN, LINE_SEED = 61, 23


def _ellipses(rng, H, W, n, value, out):
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(n):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        ry, rx = rng.uniform(0.08, 0.35) * H + 0.5, rng.uniform(0.08, 0.35) * W + 0.5
        out[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = value
    return out


def make_cbfe(N=CBFE[0], H=CBFE[1], W=CBFE[2], seed=CBFE[3]):
    """-> (gt uint8 [N, H, W]: 0 background, object labels, 255 borders / holes; masks int64 [N, H, W] in {0, 1} (one image
    single-valued, one with a 2))."""
    rng = np.random.default_rng(seed)
    gt = np.zeros((N, H, W), np.uint8)
    masks = np.zeros((N, H, W), np.int64)
    for k in range(N):
        g = _ellipses(rng, H, W, int(rng.integers(1, 4)), 0, np.zeros((H, W), np.uint8))
        for o in range(int(rng.integers(1, 4))):
            g = _ellipses(rng, H, W, 1, int(rng.integers(1, 21)), g)
        fg = g != 0
        border = fg & ~(np.roll(fg, 1, 0) & np.roll(fg, -1, 0) & np.roll(fg, 1, 1) & np.roll(fg, -1, 1))
        g[border] = 255
        g[_ellipses(rng, H, W, 1, 1, np.zeros((H, W), np.uint8)) & fg & (rng.random((H, W)) < 0.5)] = 255   # holes of void
        gt[k] = g
        m = fg.copy()
        m ^= rng.random((H, W)) < 0.03                                          # noise
        m = np.roll(m, tuple(rng.integers(-3, 4, 2)), (0, 1))                 # shifted
        masks[k] = m
    masks[1] = 0                       # a single value: score 0
    masks[2][masks[2] == 1] = np.where(rng.random(int((masks[2] == 1).sum())) < 0.1, 2, 1)   # a value 2: the [nan] path
    gt[3] = 255                        # all void: no background at all
    return gt, masks


def make_multi(n=MULTI[0], H=MULTI[1], W=MULTI[2], seed=MULTI[3]):
    """-> (gt, pr) uint8 [n, H, W], classes 0..4; map 0 has class 4 only in gt, map 1 class 4 only in pr."""
    rng = np.random.default_rng(seed)
    gt = np.zeros((n, H, W), np.uint8)
    pr = np.zeros((n, H, W), np.uint8)
    for k in range(n):
        for c in (1, 2, 3):
            _ellipses(rng, H, W, 1, c, gt[k])
            _ellipses(rng, H, W, 1, c, pr[k])
        noise = rng.random((H, W)) < 0.02
        pr[k][noise] = rng.integers(0, 4, int(noise.sum()))
    gt[0][5:9, 5:9] = 4
    pr[1][30:33, 40:45] = 4
    return gt, pr


def make_lines(n=LINE_LEN, seed=LINE_SEED):
    """-> (gt, pr) uint8 [2, n] label rows (used as 1 x n and n x 1 maps)."""
    rng = np.random.default_rng(seed)
    gt = (rng.random((2, n)) < 0.5).astype(np.uint8) * rng.integers(1, 3, (2, n)).astype(np.uint8)
    pr = (rng.random((2, n)) < 0.5).astype(np.uint8) * rng.integers(1, 3, (2, n)).astype(np.uint8)
    gt[:, 0] = pr[:, 0] = 1
    gt[:, 1] = pr[:, 1] = 2
    return gt, pr


def make_hand():
    """Hand-made (gt, pr) pairs, stored whole."""
    z = lambda h, w: np.zeros((h, w), np.uint8)  # noqa: E731
    cases = {}
    g, p = z(5, 5), z(5, 5)
    g[2, 2] = 1
    p[2, 3] = 1
    cases["pixel"] = (g, p)
    g, p = z(5, 7), z(5, 7)
    g[2, 2:5] = 1
    p[3, 1:4] = 1
    cases["line"] = (g, p)
    g, p = z(7, 7), z(7, 7)
    g[2:5, 2:5] = 1
    g[3, 3] = 0
    p[1:6, 1:6] = 1
    p[2:5, 2:5] = 0
    cases["ring"] = (g, p)
    g = np.eye(7, dtype=np.uint8) | np.eye(7, dtype=np.uint8)[::-1]
    p = z(7, 7)
    p[3, :] = 1
    cases["x"] = (g, p)
    yy, xx = np.mgrid[0:6, 0:8]
    g = ((yy + xx) % 2 == 0).astype(np.uint8)
    cases["checker"] = (g, 1 - g)
    cases["allfg"] = (np.ones((4, 6), np.uint8), np.ones((4, 6), np.uint8))
    g, p = z(6, 6), z(6, 6)
    p[1:4, 2:5] = 1
    cases["empty_gt"] = (g, p)
    return cases


def _reference():
    from oracle.gen_golden import import_reference

    import_reference()   # installs the stub finder and the reference's path
    import cv2

    import _border_follow as bf

    cv2.__version__ = "4.5.5"
    cv2.RETR_LIST, cv2.CHAIN_APPROX_NONE = 1, 1
    cv2.findContours = bf.find_contours
    cv2.contourArea = bf.contour_area
    cv2.drawContours = bf.draw_contours
    import bfscore as ref   # the reference module
    return ref


def _overall(ref, masks, gt, th):
    """The reference's evaluate_bf_score prints its result; parse the line after "overall boundary score"."""
    import torch

    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ref.evaluate_bf_score(torch.from_numpy(masks), torch.from_numpy(gt), th)
    lines = buf.getvalue().splitlines()
    return float(lines[lines.index("overall boundary score") + 1])


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def main():
    ref = _reference()
    from oracle.gen_golden import OUT

    out = {}
    gt, masks = make_cbfe()
    out["cbfe_cfg"] = np.array(CBFE, np.int64)
    out["cbfe_gt_sample"], out["cbfe_masks_sample"] = gt[:, ::7, ::9], masks[:, ::7, ::9]
    out["cbfe_scores"] = np.array([_overall(ref, masks[k:k + 1], gt[k:k + 1], 16) for k in range(len(gt))], np.float64)
    out["cbfe_overall"] = np.array(_overall(ref, masks, gt, 16), np.float64)
    print("cbfe:", out["cbfe_scores"], out["cbfe_overall"])

    g, p = make_multi()
    out["multi_cfg"] = np.array(MULTI, np.int64)
    out["multi_th"] = np.array(MULTI_TH, np.float64)
    out["multi_gt_sample"], out["multi_pr_sample"] = g[:, ::5, ::3], p[:, ::5, ::3]
    for k in range(len(g)):
        for j, th in enumerate(MULTI_TH):
            try:
                s = _quiet(ref.bfscore, g[k], p[k], th)[0]
            except IndexError:   # pr has no class the gt has: the uncaught path
                s = np.array([-1.0])
            out[f"multi{k}_t{j}"] = np.asarray(s, np.float64)
        print(f"multi{k}:", out[f"multi{k}_t0"])

    g, p = make_lines()
    out["line_cfg"] = np.array([LINE_LEN, LINE_SEED], np.int64)
    out["line_th"] = np.array(LINE_TH, np.float64)
    out["line_gt"], out["line_pr"] = g, p   # 2 x 61 bytes: stored whole
    for k in range(len(g)):
        for j, th in enumerate(LINE_TH):
            out[f"row{k}_t{j}"] = np.asarray(_quiet(ref.bfscore, g[k][None, :].copy(), p[k][None, :].copy(), th)[0], np.float64)
            out[f"col{k}_t{j}"] = np.asarray(_quiet(ref.bfscore, g[k][:, None].copy(), p[k][:, None].copy(), th)[0], np.float64)

    for name, (g, p) in make_hand().items():
        out[f"hand_{name}_gt"], out[f"hand_{name}_pr"] = g, p
        out[f"hand_{name}_score"] = np.asarray(_quiet(ref.bfscore, g.copy(), p.copy(), 2)[0], np.float64)
        print(f"hand {name}:", out[f"hand_{name}_score"])
    g = np.zeros((1, 6, 6), np.uint8)
    g[0, 1:3, 1:3] = 7
    out["hand_single_gt"], out["hand_single_pr"] = g, np.ones((1, 6, 6), np.int64)
    out["hand_single_overall"] = np.array(_overall(ref, out["hand_single_pr"], g, 16), np.float64)

    path = os.path.join(OUT, "bfscore.npz")
    np.savez_compressed(path, **out)
    print(f"{path} written ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
