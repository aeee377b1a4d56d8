#!/usr/bin/env python3
"""Times ``clustering.cluster_features`` for the frame-wise and sample-wise protocols (N13: one k-means per frame / per clip) on one GPU.

Shapes: the evaluation command line's default batch - 16 clips of 4 frames, 14 x 14 tokens of 384 columns, resolution 224, k = 10 -
and a single frame (1 clip of 1 frame).  Synthetic features: a few prototypes plus noise, so the fits are ordinary ones.

Wall clock around ``torch.cuda.synchronize()``, one warm-up call, then ``--reps`` calls (5).  Wall clock on purpose: the per-problem
loop this replaces is bound by launches and host round trips, which device events would not see.

The tool calls nothing but ``cluster_features``, so it runs unchanged on a commit from before N13: ``--tree PATH`` imports the package
from another (built) checkout.  For a before / after, run the two trees in turn on one box, more than once:

    python tools/bench_kmeans_fit.py                      # this tree
    python tools/bench_kmeans_fit.py --tree ../parent     # a checkout of the parent commit, built

``--masked SHARE`` multiplies that share of every frame's tokens (its first rows) by 0 before clustering - what the evaluator's
``use_mask=True`` does to the background tokens.  They become one and the same point, seeds land on it twice and every fit meets
empty clusters (N18): a tree from before N18 reruns each such problem on the host-driven loop, this one splits in the kernel.

Prints one JSON line per (shape, protocol): every call's milliseconds, their mean and minimum, the masked share and the tree's path.
``--only default|frame`` restricts the shapes (for a profiler run of one of them).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def features(bs, fs, n_tok, dim, synth, torch, masked=0.0):
    import numpy as np

    protos = synth.normal("bench.kf.p", (12, dim)) * 3
    which = np.arange(bs * fs * n_tok) * 7 % 12
    noise = synth.normal("bench.kf.n", (bs * fs * n_tok, dim))
    feats = (protos[which] + 0.5 * noise).astype(np.float32).reshape(bs, fs, n_tok, dim)
    feats[:, :, : int(round(masked * n_tok))] = 0.0
    return torch.from_numpy(feats).cuda()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE, help="the checkout whose timetuning_amd is timed (default: the one this file is in)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["default", "frame"], default=None)
    ap.add_argument("--masked", type=float, default=0.0, metavar="SHARE", help="share of every frame's tokens multiplied by 0 (use_mask's input)")
    args = ap.parse_args(argv)
    if not 0.0 <= args.masked < 1.0:
        ap.error("--masked takes a share in [0, 1)")
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)

    import torch

    from timetuning_amd import synth
    from timetuning_amd.clustering import cluster_features

    if not torch.cuda.is_available():
        raise SystemExit("bench_kmeans_fit.py needs a GPU: there is nothing to time without one")
    g, dim, R, k = 14, 384, 224, 10
    shapes = [("default", 16, 4), ("frame", 1, 1)]
    for name, bs, fs in shapes:
        if args.only and args.only != name:
            continue
        feats = features(bs, fs, g * g, dim, synth, torch, args.masked)
        for protocol in ("frame-wise", "sample-wise"):
            cluster_features(feats, k, g, R, protocol)   # warm-up
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                cluster_features(feats, k, g, R, protocol)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            print(json.dumps({"what": "cluster_features", "shape": name, "bs": bs, "fs": fs, "protocol": protocol, "k": k,
                              "ms": [round(m, 2) for m in ms], "mean_ms": round(sum(ms) / len(ms), 2), "min_ms": round(min(ms), 2),
                              "masked": args.masked, "tree": tree}), flush=True)


if __name__ == "__main__":
    main()
