"""The boundary F1 contour-matching score with the reference's surface (``bfscore.py``), N8.

The reference lists the contour points of ``gt == c`` and ``pr == c`` with ``cv2.findContours(RETR_LIST, CHAIN_APPROX_NONE)``, with
multiplicity, and for every point of one list takes a numpy distance to every point of the other (``calc_precision_recall``).  Every
number it forms is a function of four integer counts per (map, class) - {n_pr, hit_pr, n_gt, hit_gt}, include/timetuning_hip.h N8 -
which ``tt_bf_counts`` computes for all classes (``bfscore``) or all images (``evaluate_bf_score``) in ONE launch.  The host then
forms precision, recall and F1 with the reference's fp64 expressions and branches, the two IndexError paths included:
  - gt contour empty, pr contour not: the precision call fails inside the reference's ``try``, and ``bfscore`` returns ``[nan]`` for
    the whole call, whatever the other classes are;
  - pr contour empty, gt contour not: precision is 0 / 0 = nan, then the recall call raises an IndexError nobody catches;
  - p + r == 0: F1 is nan.
Differences: ``bfscore`` returns ``(scores, None)``, not the GT contour areas (they depend on cv2's contour order and no caller reads
them); ``evaluate_bf_score`` returns the mean it prints (the reference returns None); labels must be non-negative integers; the
threshold is at most 64 (``hip_ops.BF_MAX_RADIUS``); ``bfscore_old`` (file paths, ``cv2.imread``) is not built.  cv2 is not needed.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch

from . import hip_ops as ops


def calc_precision_recall(contours_a, contours_b, threshold):
    """The reference's point-list form: the share of the points of ``contours_b`` with a point of ``contours_a`` at squared distance
    below ``threshold * threshold`` -> (share, hits, len(contours_b)).  An empty ``contours_a`` with a non-empty ``contours_b``
    raises IndexError, an empty ``contours_b`` gives nan, as in the reference."""
    a = np.array(contours_a)
    hits = [np.any(np.square(a[:, 0] - b[0]) + np.square(a[:, 1] - b[1]) < threshold * threshold) for b in contours_b]
    top = np.sum(hits)
    try:
        share = top / len(contours_b)
    except ZeroDivisionError:
        share = 0
    return share, top, len(contours_b)


def _empty_points_index_error():
    """The IndexError the reference meets when it indexes the array of an empty point list."""
    try:
        np.array([])[:, 0]
    except IndexError as e:
        return e
    raise AssertionError("unreachable")


def _f1_from_counts(n_pr, hit_pr, n_gt, hit_gt, verbose=False):
    """One class of the reference's loop from its counts -> f1, or None for the caught IndexError (``[nan]`` for the whole call);
    raises the uncaught one."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if n_pr > 0 and n_gt == 0:   # precision: indexing the empty GT points
            return None
        precision = np.float64(hit_pr) / n_pr if n_pr else np.float64(0.0) / 0
        if verbose:
            print("\tprecision:", int(n_pr), int(hit_pr) if n_pr else 0.0)
        if n_gt > 0 and n_pr == 0:   # recall: indexing the empty predicted points, outside any try
            raise _empty_points_index_error()
        recall = np.float64(hit_gt) / n_gt if n_gt else np.float64(0.0) / 0
        if verbose:
            print("\trecall:", int(n_gt), int(hit_gt) if n_gt else 0.0)
        f1 = 2 * recall * precision / (recall + precision)
    if verbose:
        print("\tf1:", f1)
    return f1


def _scores_from_counts(targets, counts, m, verbose=False):
    """bfscore's class loop: classes ``targets`` (ascending, no 0) with their counts [len, 4], largest label m -> fp64 [m]."""
    scores = np.full(m + 1, np.nan)
    for c, (n_pr, hit_pr, n_gt, hit_gt) in zip(targets, counts):
        if verbose:
            print(">>> Calculate for class:", c)
        f1 = _f1_from_counts(n_pr, hit_pr, n_gt, hit_gt, verbose)
        if f1 is None:
            print(f"Caught exception {_empty_points_index_error()}. returning nan")
            return np.array([np.nan])
        scores[c] = f1
    return scores[1:]


def _image_score(lo, hi, counts, verbose=False):
    """evaluate_bf_score's score of one image from the smallest and largest value of its uint8 mask and the counts of
    (gt == 0, mask == 1)."""
    if lo == hi:
        if verbose:
            print(np.array([lo], np.uint8))
            print("empty fg mask. f1 of 0")
        return 0
    # the classes are 0, 1 (gt == 0) and the mask's values.  Class 1 comes first (it may raise); then every class >= 2 of the mask
    # finds no GT contour: the caught IndexError, [nan] for the image
    n_pr, hit_pr, n_gt, hit_gt = counts
    f1 = _f1_from_counts(n_pr, hit_pr, n_gt, hit_gt, verbose) if (n_pr or n_gt) else np.nan
    if f1 is None or hi >= 2:
        if verbose:
            print(f"Caught exception {_empty_points_index_error()}. returning nan")
        f1 = np.nan
    return f1


def _host_labels(x) -> np.ndarray:
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if not np.issubdtype(a.dtype, np.integer) and a.dtype != np.bool_:
        raise TypeError(f"bfscore: integer label maps are required, got {a.dtype}")
    if a.size and a.min() < 0:
        raise ValueError("bfscore: labels must be non-negative")
    return a.astype(np.int64)


def bfscore(gt, pr, threshold: float = 2, verbose=False):
    """The BF score of every class 1..max of two 2-D label maps (numpy or torch) -> (fp64 [max] scores, nan for a class in neither
    map, None).  All classes are counted in one launch."""
    g, p = _host_labels(gt), _host_labels(pr)
    if g.ndim != 2 or g.shape != p.shape:
        raise ValueError(f"bfscore: gt {g.shape} and pr {p.shape} must be the same 2-D shape")
    classes = np.union1d(np.unique(g), np.unique(p))
    if verbose:
        print("Classes :", classes)
    m = int(classes.max())
    targets = [int(c) for c in classes if c != 0]
    if targets:
        dev = torch.device("cuda", torch.cuda.current_device())
        gd, pd = torch.from_numpy(g).to(dev), torch.from_numpy(p).to(dev)
        cls = torch.tensor(targets, dtype=torch.int64, device=dev)[:, None, None]
        counts = ops.bf_counts((gd[None] == cls).to(torch.uint8).contiguous(), (pd[None] == cls).to(torch.uint8).contiguous(),
                               threshold).cpu().numpy()
        return _scores_from_counts(targets, counts, m, verbose), None
    return np.full(m, np.nan), None


def evaluate_bf_score(segmentation_masks, gt, match_threshold: float = 16, verbose=False):
    """Per image k: the BF score of class 1 between ``gt[k] == 0`` (the background: 255 void pixels count as "not background", as in
    the reference) and ``segmentation_masks[k]`` cast to uint8; 0 where the mask has a single value.  All N images in one launch.
    Prints "overall boundary score" and the nan-mean, and returns that mean."""
    masks = torch.as_tensor(segmentation_masks)
    gt = torch.as_tensor(gt)
    if verbose:
        print("pred fg mask shape")
        print(masks.shape)
        print("gt shape")
        print(gt.shape)
    N = gt.shape[0]
    H, W = (gt.shape[-2], gt.shape[-1]) if gt.dim() >= 3 else (0, 0)
    if masks.shape[0] != N or H * W == 0 or gt.numel() != N * H * W or masks.numel() != N * H * W:
        raise ValueError(f"evaluate_bf_score: masks {tuple(masks.shape)} and gt {tuple(gt.shape)} must both hold N maps of H x W")
    dev = torch.device("cuda", torch.cuda.current_device())
    pred = masks.to(dev).reshape(N, H, W)
    if pred.is_floating_point():
        pred = pred.trunc()   # numpy's astype(uint8) of values in [0, 256)
    pred = pred.to(torch.uint8).contiguous()
    gt_fg = (gt.to(dev).reshape(N, H, W) == 0).to(torch.uint8).contiguous()
    lo, hi = pred.amin(dim=(1, 2)).cpu().numpy(), pred.amax(dim=(1, 2)).cpu().numpy()
    counts = ops.bf_counts(gt_fg, (pred == 1).to(torch.uint8), match_threshold).cpu().numpy()
    scores = [_image_score(lo[k], hi[k], counts[k], verbose) for k in range(N)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # the mean of no number is nan, as the reference prints it
        overall = np.nanmean(np.array(scores, dtype=np.float64))
    print("overall boundary score")
    print(overall)
    return overall
