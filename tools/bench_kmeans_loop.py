#!/usr/bin/env python3
"""Times ``clustering.Kmeans.train`` with ``loop="host"`` and ``loop="device"`` (N28) on one GPU, on the same tree, alternating.

Shapes (n, d, k), each the training set AFTER faiss' subsample of 256 points per centroid - what the large fits of the evaluation path
hand the Lloyd loop:

    over-clustering   (128 000, 50, 500)   cluster_features(..., "dataset-wise") at num_clusters = 500
    dataset-wise 21   (5 376, 50, 21)      the same protocol at Pascal VOC's 21 clusters
    cbfe              (76 800, 384, 300)   create_overclustering_maps at the default k_fg_extraction on 384 raw feature columns
    cbfe pca          (76 800, 50, 300)    the same on eval_feature_dim = 50 PCA columns, what get_foreground_masks clusters here

Synthetic points: 64 prototypes plus unit noise, so the fits are ordinary ones (no empty clusters after the first iterations).  The
reference's parameters: niter 50, nredo 5, seed 1.

Wall clock around ``torch.cuda.synchronize()``: the host loop is bound by launches and host round trips, which device events would not
see.  One warm-up ``train`` per loop and shape, then ``--reps`` (at least 5) pairs host / device in turn.  The two results are compared
on the way: the centroids must be equal bit for bit.

Prints one JSON line per shape: every call's milliseconds per loop, the medians, the minima, whether the device loop's median lies
below the host loop's minimum (the rule by which a caller's default is ``"device"``), and the redos per launch the workspace budget gave.
``--only NAME`` restricts the shapes.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"over-clustering": (128000, 50, 500), "dataset-wise 21": (5376, 50, 21), "cbfe": (76800, 384, 300), "cbfe pca": (76800, 50, 300)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--niter", type=int, default=50)
    ap.add_argument("--only", choices=sorted(SHAPES), default=None)
    args = ap.parse_args(argv)
    if args.reps < 5:
        ap.error("--reps: at least 5 runs per loop")
    sys.path.insert(0, HERE)

    import numpy as np
    import torch

    from timetuning_amd import cluster_based_foreground_extraction as cbfe
    from timetuning_amd import synth
    from timetuning_amd.clustering import Kmeans

    def train(x, k, loop, budget):
        km = Kmeans(x.shape[1], k, niter=args.niter, nredo=5, seed=1, loop=loop, loop_workspace_bytes=budget)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        km.train(x)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, km

    for name, (n, d, k) in SHAPES.items():
        if args.only not in (None, name):
            continue
        protos = synth.normal(f"bench.kl.p.{name}", (64, d)) * 3
        x = torch.from_numpy((protos[np.arange(n) * 7 % 64] + synth.normal(f"bench.kl.n.{name}", (n, d))).astype(np.float32)).cuda()
        budget = cbfe.LOOP_WORKSPACE_BYTES if name.startswith("cbfe") else None   # what the caller of this shape passes
        ms = {"host": [], "device": []}
        kms = {loop: train(x, k, loop, budget)[1] for loop in ms}         # warm-up, and the comparison
        equal = bool(np.array_equal(kms["host"].centroids.view(np.int32), kms["device"].centroids.view(np.int32)))
        for _ in range(args.reps):
            for loop in ms:
                ms[loop].append(round(train(x, k, loop, budget)[0], 2))
        med = {loop: statistics.median(v) for loop, v in ms.items()}
        print(json.dumps({"what": "Kmeans.train", "shape": name, "n": n, "d": d, "k": k, "niter": args.niter, "nredo": 5,
                          "host_ms": ms["host"], "device_ms": ms["device"], "host_median": med["host"], "device_median": med["device"],
                          "host_min": min(ms["host"]), "device_min": min(ms["device"]),
                          "device_median_below_host_min": med["device"] < min(ms["host"]), "speedup_of_medians": round(med["host"] / med["device"], 2),
                          "centroids_equal": equal, "device_fallback": kms["device"].fallback, "redos_per_launch": kms["device"].redo_group,
                          "host_objectives": kms["host"].obj, "device_objectives": kms["device"].obj}), flush=True)


if __name__ == "__main__":
    main()
