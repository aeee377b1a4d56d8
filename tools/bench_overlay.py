#!/usr/bin/env python3
"""N17: the render launch and the histogram launch on one GPU, device events, median of ``--iters`` after a warm-up.  One JSON line each:
  - ``overlay_photo`` / ``overlay_labels``: ``hip_ops.overlay_grid`` on 64 frames at 224 x 224 - float32 frames with int16 cluster
    maps (what ``cluster_features`` returns) for the photo mode, two int64 maps with a per-frame LUT for the labels mode;
  - ``argmax_hist``: ``hip_ops.upsample_argmax_hist`` at (M, g, K, R) = (64, 14, 200, 224) beside ``upsample_argmax_f32`` followed by
    ``torch.bincount`` on the same scores (``labels_bincount_ms``; ``labels_ms`` is the arg-max launch alone);
  - ``floor_ms`` / ``floor_fraction``: the bytes a launch cannot avoid at 6.3 TB/s (the measured HBM copy rate) - every input byte
    once plus every output byte once - computed from the shapes, not measured; fraction = floor / measured.

    python tools/bench_overlay.py [--iters 20]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from timetuning_amd import hip_ops as ops  # noqa: E402
from timetuning_amd.visualization import voc_palette  # noqa: E402

HBM_BPS = 6.3e12
F, H, W, PAD = 64, 224, 224, 2
M, G, K, R = 64, 14, 200, 224


def time_events(fn, iters, warmup=3):
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


def line(what, ms, floor_bytes, **more):
    floor = floor_bytes / HBM_BPS * 1e3
    print(json.dumps({"what": what, "ms": round(ms, 4), "floor_ms": round(floor, 5), "floor_fraction": round(floor / ms, 3), **more}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda").manual_seed(1)
    pal = torch.from_numpy(voc_palette()).cuda()
    # piecewise constant maps, as up-sampled token maps are: 14 x 14 cells of 16 x 16 pixels
    cells = torch.randint(0, 200, (F, 14, 14), generator=gen, device="cuda")
    maps = cells.repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous()
    frames = torch.rand((F, 3, H, W), generator=gen, device="cuda")
    maps16, gt = maps.to(torch.int16), (maps % 21).contiguous()
    lut = torch.randint(0, 21, (F, 200), generator=gen, device="cuda", dtype=torch.int32)
    out_photo, out_labels = F * 3 * (H + 2 * PAD) * (2 * W + 3 * PAD), F * 3 * (H + 2 * PAD) * (3 * W + 4 * PAD)
    ms = time_events(lambda: ops.overlay_grid(ops.OVERLAY_PHOTO, maps16, pal, frames=frames), args.iters)
    line("overlay_photo", ms, frames.numel() * 4 + maps16.numel() * 2 + out_photo, frames=F, H=H, W=W, out_bytes=out_photo)
    ms = time_events(lambda: ops.overlay_grid(ops.OVERLAY_LABELS, maps, pal, labels_b=gt, lut=lut), args.iters)
    line("overlay_labels", ms, 2 * maps.numel() * 8 + lut.numel() * 4 + out_labels, frames=F, H=H, W=W, out_bytes=out_labels)

    scores = torch.randn((M, G * G, K), generator=gen, device="cuda")
    counts = torch.zeros(K, dtype=torch.int64, device="cuda")
    hist_ms = time_events(lambda: ops.upsample_argmax_hist(scores, R, counts), args.iters)
    labels_ms = time_events(lambda: ops.upsample_argmax_f32(scores, R), args.iters)
    both_ms = time_events(lambda: torch.bincount(ops.upsample_argmax_f32(scores, R).flatten(), minlength=K), args.iters)
    assert torch.equal(ops.upsample_argmax_hist(scores, R), torch.bincount(ops.upsample_argmax_f32(scores, R).flatten(), minlength=K))
    line("argmax_hist", hist_ms, scores.numel() * 4 + K * 8, M=M, g=G, K=K, R=R, labels_ms=round(labels_ms, 4), labels_bincount_ms=round(both_ms, 4),
         labels_bytes=M * R * R * 8)


if __name__ == "__main__":
    main()
