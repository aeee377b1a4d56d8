"""NumPy restatements of the metric counters, shared by the host tests (tests/test_davis_metrics_host.py, tests/test_bfscore_host.py pin them
to the reference's fixtures), the GPU tests (tests/test_hip_davis_metrics.py, tests/test_hip_bfscore.py) and the sweep's fifth tier
(tests/_sweep_checks_metric.py).  Nothing here touches a GPU."""
from __future__ import annotations

import numpy as np

import _border_follow as bfl

BF_TABLE = bfl.multiplicity_table()


# ---- tt_davis_jf_counts -------------------------------------------------------------------------------------------------------------------

def np_seg2bmap(seg):
    s = np.asarray(seg) != 0
    H, W = s.shape
    e = np.zeros_like(s)
    e[:, :-1] = s[:, 1:]
    d = np.zeros_like(s)
    d[:-1, :] = s[1:, :]
    de = np.zeros_like(s)
    de[:-1, :-1] = s[1:, 1:]
    b = (s ^ e) | (s ^ d) | (s ^ de)
    b[H - 1, :] = s[H - 1, :] ^ e[H - 1, :]
    b[:, W - 1] = s[:, W - 1] ^ d[:, W - 1]
    b[H - 1, W - 1] = False
    return b


def np_dilate(b, element):
    b = np.asarray(b, bool)
    H, W = b.shape
    el = np.asarray(element) != 0
    ay, ax = el.shape[0] // 2, el.shape[1] // 2
    pad = np.zeros((H + 2 * el.shape[0], W + 2 * el.shape[1]), bool)
    pad[el.shape[0]:el.shape[0] + H, el.shape[1]:el.shape[1] + W] = b
    out = np.zeros_like(b)
    for i, j in zip(*np.nonzero(el)):
        y0, x0 = el.shape[0] + i - ay, el.shape[1] + j - ax
        out |= pad[y0:y0 + H, x0:x0 + W]
    return out


def davis_np_counts(pred, gt, num_objects, element, void=None):
    """int64 [O, T, 6] = {J intersection, J union, n_fg, n_gt, fg_match, gt_match} of objects 1..O."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    T = pred.shape[0]
    keep = np.ones(pred.shape, bool) if void is None else np.asarray(void) == 0
    out = np.zeros((num_objects, T, 6), np.int64)
    for o in range(1, num_objects + 1):
        for t in range(T):
            p, g = (pred[t] == o) & keep[t], (gt[t] == o) & keep[t]
            fb, gb = np_seg2bmap(p), np_seg2bmap(g)
            out[o - 1, t] = [(p & g).sum(), (p | g).sum(), fb.sum(), gb.sum(), (fb & np_dilate(gb, element)).sum(),
                             (gb & np_dilate(fb, element)).sum()]
    return out


# ---- tt_bf_counts -------------------------------------------------------------------------------------------------------------------------

def np_mult(a):
    """Per-pixel multiplicity of a binary map from the follower-derived table."""
    a = np.asarray(a) != 0
    return np.where(a, BF_TABLE[bfl.neighbourhood_index(a)], 0).astype(np.int64)


def np_within(b, t):
    """bool [H, W]: a set pixel of ``b`` at integer squared distance d < t * t (the bound a Python float, as the reference)."""
    b = np.asarray(b, bool)
    H, W = b.shape
    tt = float(t) * float(t)
    out = np.zeros_like(b)
    ys, xs = np.nonzero(b)
    if not len(ys):
        return out
    reach = int(np.ceil(abs(float(t)))) + 1
    for dy in range(-reach, reach + 1):
        for dx in range(-reach, reach + 1):
            if dy * dy + dx * dx < tt:
                y, x = ys - dy, xs - dx
                ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
                out[y[ok], x[ok]] = True
    return out


def bf_np_counts(gt, pr, t):
    """int64 [P, 4] = {n_pr, hit_pr, n_gt, hit_gt} of binary maps [P, H, W]."""
    gt, pr = np.asarray(gt), np.asarray(pr)
    out = np.zeros((gt.shape[0], 4), np.int64)
    for k in range(gt.shape[0]):
        mp, mg = np_mult(pr[k]), np_mult(gt[k])
        out[k] = [mp.sum(), mp[np_within(mg > 0, t)].sum(), mg.sum(), mg[np_within(mp > 0, t)].sum()]
    return out


# ---- tt_confusion_counts_segments ------------------------------------------------------------------------------------------------------------

def confusion_segments_np(pred, gt, Cg, Cp, ignore=None):
    """int64 [S, Cg, Cp]: np.bincount of gt * Cp + pred per segment over the elements with 0 <= gt < Cg, 0 <= pred < Cp, gt != ignore
    (the ``expected`` of tests/test_hip_confusion_segments.py, on host arrays)."""
    pred, gt = np.asarray(pred).astype(np.int64), np.asarray(gt).astype(np.int64)
    out = np.zeros((pred.shape[0], Cg, Cp), np.int64)
    for s in range(pred.shape[0]):
        p, g = pred[s], gt[s]
        ok = (g >= 0) & (g < Cg) & (p >= 0) & (p < Cp)
        if ignore is not None:
            ok &= g != ignore
        out[s] = np.bincount(g[ok] * Cp + p[ok], minlength=Cg * Cp).reshape(Cg, Cp)
    return out
