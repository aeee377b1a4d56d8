#!/usr/bin/env python
"""N23: what the label-map kernels buy the evaluator (profiles/n23_video_eval.txt).

  python tools/bench_video_eval.py [--tree DIR] [--calls 5] [--tag new]      cluster_features(annotations=...) at the default evaluation
        shape - 16 clips x 4 frames, 14 x 14 tokens of 384 columns, R = 224, frame-wise and sample-wise - wall clock around
        torch.cuda.synchronize(), one warm-up call; and the cluster counts alone (one torch.unique per segment against
        hip_ops.label_value_counts where the tree has it).  --tree: a built checkout to import instead of this one (the parent commit).
  python tools/bench_video_eval.py --kernels [--reps 20]                     only launches tt_label_presence_segments (uint8 and int64)
        and tt_map_instances on 16 segments of 4 x 224 x 224 labels: run it under `rocprofv3 --kernel-trace --stats` for the kernels'
        own times.
Synthetic label maps constant on 16 x 16 blocks (4 or 5 values per frame).  Needs a GPU."""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS, FS, G, DIM, R = 16, 4, 14, 384, 224


def label_maps(torch):
    yy, xx = np.mgrid[0:R, 0:R] // 16
    maps = np.stack([[((yy * (1 + (b + f) % 3) + xx) % (4 + (b + f) % 2)) for f in range(FS)] for b in range(BS)])
    return torch.from_numpy(maps.astype(np.int64)).cuda()


def timed(torch, fn, calls):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(round((time.perf_counter() - t0) * 1e3, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", type=str, default=REPO)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tag", type=str, default="new")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))

    import torch

    from timetuning_amd import clustering, hip_ops as ops, synth

    ann = label_maps(torch)
    if a.kernels:
        small = ann.to(torch.uint8).view(BS, -1)
        cat = torch.full((BS, 256), -1, dtype=torch.int32, device="cuda")
        cat[:, 1:8] = torch.arange(2, 9, dtype=torch.int32, device="cuda")
        for _ in range(a.reps):
            ops.label_presence(small)
            ops.label_presence(ann.view(BS, -1))
            ops.map_instances(small, cat, True)
        torch.cuda.synchronize()
        print(f"{a.reps} rounds of label_presence (uint8, int64) and map_instances on {BS} segments of {FS} x {R} x {R} labels")
        return
    feats = torch.from_numpy(synth.normal("n23.bench", (BS, FS, G * G, DIM)).astype(np.float32)).cuda()
    rows = []
    for protocol, segments in (("frame-wise", BS * FS), ("sample-wise", BS)):
        ms = timed(torch, lambda: clustering.cluster_features(feats, 10, G, R, protocol, annotations=ann), a.calls)
        rows.append(("cluster_features(annotations)", protocol, ms))
        seg = ann.view(segments, -1)
        ms = timed(torch, lambda: [torch.unique(seg[s]).shape[0] for s in range(segments)], a.calls)
        rows.append(("counts: torch.unique loop", protocol, ms))
        if hasattr(ops, "label_value_counts"):
            assert ops.label_value_counts(seg) == [torch.unique(seg[s]).shape[0] for s in range(segments)]
            ms = timed(torch, lambda: ops.label_value_counts(seg), a.calls)
            rows.append(("counts: label_value_counts", protocol, ms))
    for what, protocol, ms in rows:
        print(f"{what:32s} {protocol:12s} {a.tag:7s} {sum(ms) / len(ms):9.3f} {min(ms):9.3f}   {ms}")


if __name__ == "__main__":
    main()
