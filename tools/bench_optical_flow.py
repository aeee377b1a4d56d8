#!/usr/bin/env python3
"""N10: the optical-flow baseline (dense Farneback flow + nearest label remap, farneback.hip) on a DAVIS-size clip (50 frames of
480 x 854, 49 pairs) and a 25-frame 224 x 224 clip, the reference's parameters (0.5, 3, 15, 3, 5, 1.2, 0).  One JSON line per clip:
  - ``ms_per_clip`` / ``ms_per_pair``: ``propagate_clip_optical_flow`` end to end (gray conversion, all pairs' flow, the label chain;
    workspace allocation included), device events, median of ``--iters`` after a warm-up; ``flow_ms_per_pair``: ``farneback_flow``
    alone on the gray frames;
  - ``floor_compulsory_ms``: frames read once and flows written once at 6.3 TB/s (the measured HBM copy rate), from the shapes;
    ``floor_staged_ms``: the same for the bytes the staged kernels move (every intermediate written once and read once per reader,
    R read twice per pair), also from the shapes - neither is measured;
  - ``numpy_restatement_ms_per_pair``: tests/_farneback.py (fp64, one pair, single thread of NumPy) - the in-repo stand-in for cv2,
    NOT cv2's speed;
  - ``--stats <results.db | kernel_stats.csv>`` instead prints (without a GPU) the per-stage kernel times of a separate
    ``rocprofv3 --kernel-trace --stats`` run of this script (``--iters 1 --no-numpy``: 3 calls per clip, both clips).

    python tools/bench_optical_flow.py [--iters 5] [--no-numpy]
    python tools/bench_optical_flow.py --stats <rocprofv3 output>
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from timetuning_amd import hip_ops as ops  # noqa: E402
from timetuning_amd import mask_propagation as MP  # noqa: E402

HBM_BPS = 6.3e12
CLIPS = [("davis_480x854", 50, 480, 854), ("square_224", 25, 224, 224)]


def time_events(fn, iters, warmup=1):
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
    return float(np.median(times))


def floors(fs, H, W, levels=3, winsize=15, iterations=3):
    L, sizes = ops.farneback_plan(H, W, 0.5, levels)
    F, P = fs, fs - 1
    compulsory = F * H * W + P * H * W * 8
    staged = 0
    for k in range(L + 1):
        hw = sizes[k][0] * sizes[k][1]
        staged += F * H * W * (1 + 4 + 4)                  # vblur: u8 in, fp32 out; hblur_resize reads it
        staged += F * hw * (4 + 4 + 12 + 12 + 20)          # level image out + in, V out + in, R out
        staged += P * hw * (40 + 8 + 20)                   # init: R of both frames, flow, M
        staged += P * hw * iterations * (20 + 20 + 20 + 8) + P * hw * (iterations - 1) * (40 + 20)   # box_v, box_h_solve (+ update)
    return compulsory / HBM_BPS * 1e3, staged / HBM_BPS * 1e3


def stage_table(path):
    if path.endswith(".db"):                      # rocprofv3's rocpd database
        import sqlite3

        cur = sqlite3.connect(path).cursor()
        rows = list(cur.execute("select name, count(*), sum(end - start) from kernels group by name"))
    else:
        rows = [(r["Name"], int(r["Calls"]), int(r["TotalDurationNs"])) for r in csv.DictReader(open(path))]
    out = {}
    for n, c, t in rows:
        for stage in ("fb_gray_u8", "fb_vblur", "fb_hblur_resize", "fb_poly_v", "fb_poly_h", "fb_init_level", "fb_box_v", "fb_box_h_solve",
                      "fb_remap_nearest"):
            if stage in n:
                s = out.setdefault(stage, [0, 0])
                s[0] += c
                s[1] += t
    return {k: {"calls": c, "total_ms": round(t / 1e6, 3)} for k, (c, t) in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    if a.stats:                                   # no GPU: the table of an earlier profiled run
        print(json.dumps({"stages": stage_table(a.stats)}))
        return
    torch.cuda.set_device(0)
    for name, fs, H, W in CLIPS:
        Wc = -(-W // 8) * 8                                   # the synthetic texture is 8 x 8 cells: 856 wide, cropped to 854
        clip, masks = MP.synthetic_tracking_clip(fs, H, seed=1, width=Wc)
        clip, first = clip[..., :W].contiguous().cuda(), masks[0, :, :W].contiguous().cuda()
        gray = ops.flow_gray_u8(clip)
        pairs = MP._clip_pairs(1, fs)
        clip_ms = time_events(lambda: MP.propagate_clip_optical_flow(clip, first), a.iters)
        flow_ms = time_events(lambda: ops.farneback_flow(gray, pairs), a.iters)
        fc, fsd = floors(fs, H, W)
        rec = {"clip": name, "frames": fs, "pairs": fs - 1, "H": H, "W": W, "ms_per_clip": round(clip_ms, 3),
               "ms_per_pair": round(clip_ms / (fs - 1), 4), "flow_ms_per_pair": round(flow_ms / (fs - 1), 4),
               "floor_compulsory_ms": round(fc, 4), "floor_staged_ms": round(fsd, 3)}
        if not a.no_numpy:
            import _farneback as FB

            g = gray[:2].cpu().numpy()
            t0 = time.perf_counter()
            FB.farneback(g[1], g[0])
            rec["numpy_restatement_ms_per_pair"] = round((time.perf_counter() - t0) * 1e3, 1)
            rec["numpy_note"] = "fp64 NumPy restatement, not cv2"
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
