#!/usr/bin/env python3
"""Boundary F-score (N8) at Pascal-VOC-val size: 1 449 masks at 100 x 100 (CBFE's eval_resolution) and at 448 x 448, t = 16.

Prints one JSON line per measurement:
  - ``tt_bf_counts`` device time (events, after warm-up), the bytes it must read (gt + pr binary maps, uint8; the computed floor, not a
    measured transfer) and that floor's time at 6.3 TB/s (the measured HBM copy rate) over the kernel time;
  - ``evaluate_bf_score`` end to end (label maps on the GPU -> printed mean), wall clock;
  - the reference-style per-image loop (tests/_border_follow.py's contours + ``calc_precision_recall`` on the point lists) on a few
    images, EXTRAPOLATED to N (cv2 is not installed, so this is not the reference's own speed).
Inputs: ``gen_bfscore_golden.make_cbfe`` images, tiled to N and resized by nearest neighbour.

    python tools/bench_bfscore.py [--images 1449] [--iters 10]
"""
from __future__ import annotations

import argparse
import contextlib
import importlib.util
import io
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _border_follow as bfl  # noqa: E402
from timetuning_amd import bfscore as BF  # noqa: E402
from timetuning_amd import hip_ops as ops  # noqa: E402

HBM_BPS = 6.3e12


def _generator():
    spec = importlib.util.spec_from_file_location("gen_bfscore_golden", os.path.join(REPO, "tools", "gen_bfscore_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def time_events(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def reference_style(masks, gt, t):
    """Per image: the point lists of (gt == 0) and the mask, then calc_precision_recall both ways, as bfscore.py does."""
    scores = []
    for m, g in zip(masks, gt):
        m = m.astype(np.uint8)
        if len(np.unique(m)) == 1:
            scores.append(0)
            continue
        gp, pp = bfl.contour_points(g == 0), bfl.contour_points(m == 1)
        p = BF.calc_precision_recall(gp, pp, t)[0]
        r = BF.calc_precision_recall(pp, gp, t)[0]
        scores.append(2 * r * p / (r + p))
    return scores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1449)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--threshold", type=float, default=16)
    ap.add_argument("--host_images", type=int, default=4)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bfscore needs a GPU"
    dev = torch.device("cuda", 0)
    gt0, masks0 = _generator().make_cbfe(N=16)
    masks0[1], masks0[2] = masks0[0], masks0[4]   # the generator's single-valued, value-2 and all-void images would skip the
    gt0[3] = gt0[5]                               # counting (or raise) in the host baseline
    N = a.images
    for R in (100, 448):
        idx = (np.arange(R) * 100) // R
        gt_np = np.resize(gt0[:, idx][:, :, idx], (N, R, R))
        masks_np = np.resize(masks0[:, idx][:, :, idx], (N, R, R))
        gt = torch.from_numpy(gt_np).to(dev)
        masks = torch.from_numpy(masks_np).to(dev)
        gfg = (gt == 0).to(torch.uint8).contiguous()
        pr = (masks == 1).to(torch.uint8).contiguous()
        nbytes = 2 * gfg.numel()
        med, best = time_events(lambda: ops.bf_counts(gfg, pr, a.threshold), a.iters)
        floor_ms = nbytes / HBM_BPS * 1e3
        print(json.dumps({"bench": "tt_bf_counts", "N": N, "H": R, "W": R, "t": a.threshold, "ms_median": round(med, 4),
                          "ms_min": round(best, 4), "bytes_read_floor": nbytes, "floor_ms_at_6.3TBps": round(floor_ms, 4),
                          "fraction_of_floor": round(floor_ms / med, 4)}), flush=True)
        walls = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                overall = BF.evaluate_bf_score(masks, gt, a.threshold)
            walls.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"bench": "evaluate_bf_score_end_to_end", "N": N, "H": R, "ms_wall_median_of_3": round(float(np.median(walls)), 2),
                          "overall": float(overall)}), flush=True)
        n = min(a.host_images, N)
        t0 = time.perf_counter()
        host = reference_style(masks_np[:n], gt_np[:n], a.threshold)
        host_s = time.perf_counter() - t0
        with contextlib.redirect_stdout(io.StringIO()):
            dev_scores = [BF.evaluate_bf_score(masks[k:k + 1], gt[k:k + 1], a.threshold) for k in range(n)]
        same = all(np.float64(h).tobytes() == np.float64(d).tobytes() for h, d in zip(host, dev_scores))
        print(json.dumps({"bench": "reference_style_point_lists", "H": R, "images_timed": n, "s_timed": round(host_s, 3),
                          "s_extrapolated_to_N": round(host_s * N / n, 1), "extrapolated": True, "scores_match_kernel": same}),
              flush=True)


if __name__ == "__main__":
    main()
