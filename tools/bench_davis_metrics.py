#!/usr/bin/env python3
"""DAVIS J&F (N7) at DAVIS-2017-val size: T = 2 000 frames of 480 x 854, O = 3 objects, disk radius 8 (bound_th 0.008).

Prints one JSON line per measurement:
  - ``tt_davis_jf_counts`` device time (events, after warm-up) for uint8 and int64 labels, the bytes it must read (pred + gt; the
    computed floor, not a measured transfer) and that floor's time at 6.3 TB/s (the measured HBM copy rate) over the kernel time;
  - ``davis_jf`` end to end (launch, copy of the [O, T, 6] counts, J and F on the host), wall clock;
  - a host baseline on a subset, EXTRAPOLATED to T: numpy boundaries + ``scipy.ndimage.binary_dilation`` with the same disk, per
    (object, frame) as the reference loops (cv2 is not installed, so this is not the reference's own speed).
Inputs: ``synthetic_davis_labels`` frames, tiled to T.

    python tools/bench_davis_metrics.py [--frames 2000] [--iters 10]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from timetuning_amd import hip_ops as ops  # noqa: E402
from timetuning_amd import mask_propagation as MP  # noqa: E402

HBM_BPS = 6.3e12


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


def host_counts(pred, gt, O, element):
    """numpy + scipy per (object, frame): the reference's loop structure."""
    from scipy.ndimage import binary_dilation

    out = np.zeros((O, pred.shape[0], 6), np.int64)
    for o in range(1, O + 1):
        for t in range(pred.shape[0]):
            p, g = pred[t] == o, gt[t] == o
            bm = []
            for s in (p, g):
                e = np.zeros_like(s); e[:, :-1] = s[:, 1:]
                d = np.zeros_like(s); d[:-1] = s[1:]
                de = np.zeros_like(s); de[:-1, :-1] = s[1:, 1:]
                b = (s ^ e) | (s ^ d) | (s ^ de)
                b[-1] = s[-1] ^ e[-1]; b[:, -1] = s[:, -1] ^ d[:, -1]; b[-1, -1] = False
                bm.append(b)
            fb, gb = bm
            out[o - 1, t] = [(p & g).sum(), (p | g).sum(), fb.sum(), gb.sum(), (fb & binary_dilation(gb, element)).sum(),
                             (gb & binary_dilation(fb, element)).sum()]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=854)
    ap.add_argument("--objects", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--host_frames", type=int, default=8)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_davis_metrics needs a GPU"
    dev = torch.device("cuda", 0)
    T, H, W, O = a.frames, a.height, a.width, a.objects
    base = 16
    gt_np, pred_np, _ = MP.synthetic_davis_labels(base, H, W, O, seed=11)
    reps = (T + base - 1) // base
    gt8 = torch.from_numpy(gt_np).to(dev).repeat(reps, 1, 1)[:T].contiguous()
    pred8 = torch.from_numpy(pred_np).to(dev).repeat(reps, 1, 1)[:T].contiguous()
    radius = float(MP._bound_pix(0.008, (H, W)))
    element = MP.disk(radius)
    ref = None
    for dtype in (torch.uint8, torch.int64):
        pred, gt = pred8.to(dtype), gt8.to(dtype)
        nbytes = 2 * pred.numel() * pred.element_size()
        med, best = time_events(lambda: ops.davis_jf_counts(pred, gt, O, element), a.iters)
        counts = ops.davis_jf_counts(pred, gt, O, element)
        if ref is None:
            ref = counts
        floor_ms = nbytes / HBM_BPS * 1e3
        print(json.dumps({"bench": "tt_davis_jf_counts", "labels": str(dtype).replace("torch.", ""), "T": T, "H": H, "W": W, "O": O,
                          "radius": radius, "ms_median": round(med, 4), "ms_min": round(best, 4), "bytes_read_floor": nbytes,
                          "floor_ms_at_6.3TBps": round(floor_ms, 4), "fraction_of_floor": round(floor_ms / med, 4),
                          "same_counts_as_uint8": bool(torch.equal(counts, ref))}), flush=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    J, F = MP.davis_jf(pred8, gt8, O)
    wall = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"bench": "davis_jf_end_to_end", "labels": "uint8", "T": T, "ms_wall": round(wall, 2), "J_mean": float(J.mean()),
                      "F_mean": float(F.mean())}), flush=True)
    n = min(a.host_frames, T)
    t0 = time.perf_counter()
    hc = host_counts(pred_np[:n], gt_np[:n], O, element.astype(bool))
    host_s = time.perf_counter() - t0
    print(json.dumps({"bench": "host_numpy_scipy_baseline", "frames_timed": n, "s_timed": round(host_s, 3),
                      "s_extrapolated_to_T": round(host_s * T / n, 1), "extrapolated": True,
                      "counts_match_kernel": bool(np.array_equal(hc, ref[:, :n].cpu().numpy()))}), flush=True)


if __name__ == "__main__":
    main()
