#!/usr/bin/env python3
"""Times the tiled k-means kernels (N12) against the LDS-resident ones (both in kmeans.hip) on one GPU, with HIP events
after warm-up, the two kernels of a comparison alternating inside one timed series.

1. A shape both take - the CBFE over-clustering, P = 1 100 000 points, d = 50, k = 300: tt_kmeans_assign against
   tt_kmeans_assign_tiled (default tile; k fits one tile) and against a forced two-tile walk (tile_k = 150); the outputs are compared
   bit for bit as well.
2. The reference's over-clustering beyond the resident limit, d = 50, k = 500: tt_kmeans_assign_tiled at P = 1 100 000 and
   tt_kmeans_accumulate_tiled at P = 128 000 (the k * 256 points faiss subsamples for training), with the resident accumulation at
   k = 300 on the same points beside it.

    python tools/bench_kmeans_tiled.py [--points 1100000] [--train-points 128000] [--reps 10]

Prints one JSON line per measurement: milliseconds per call, and the (point, centroid, column) terms per second the assignment
sustains (P * k * d over the time: one subtraction and one fused multiply-add each).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from timetuning_amd import hip_ops as ops, synth  # noqa: E402


def alternating_ms(fns, reps, warmup=3):
    """Mean device milliseconds of each callable, the callables taking turns inside the timed series."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    marks = [[torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)] for _ in range(reps)]
    for row in marks:
        row[0].record()
        for fn, e in zip(fns, row[1:]):
            fn()
            e.record()
    torch.cuda.synchronize()
    return [sum(row[i].elapsed_time(row[i + 1]) for row in marks) / reps for i in range(len(fns))]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_100_000)
    ap.add_argument("--train-points", type=int, default=128_000)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_kmeans_tiled.py needs a GPU: there is nothing to time without one")
    d = 50
    x = torch.from_numpy(synth.normal("bench.kt.x", (args.points, d))).cuda()
    c500 = (x[:500] * 0.5).contiguous()
    c300 = c500[:300].contiguous()
    xt = x[: args.train_points].contiguous()

    def report(what, ms, P, k):
        print(json.dumps({"what": what, "P": P, "d": d, "k": k, "ms": round(ms, 4), "gterms_per_s": round(P * k * d / ms / 1e6, 1)}))

    # 1. where both run
    same = all(torch.equal(a, b) for t in (0, 150) for a, b in zip(ops.kmeans_assign(x, c300, return_dist=True),
                                                                    ops.kmeans_assign_tiled(x, c300, return_dist=True, tile_k=t)))
    print(json.dumps({"what": "tiled assignment equals the resident one bit for bit (k = 300, tiles 0 and 150)", "equal": bool(same)}))
    res, tiled, tiled2 = alternating_ms([lambda: ops.kmeans_assign(x, c300), lambda: ops.kmeans_assign_tiled(x, c300),
                                         lambda: ops.kmeans_assign_tiled(x, c300, tile_k=150)], args.reps)
    report("kmeans_assign (resident)", res, args.points, 300)
    report("kmeans_assign_tiled (one tile)", tiled, args.points, 300)
    report("kmeans_assign_tiled (tile_k = 150: two tiles)", tiled2, args.points, 300)
    # 2. beyond the resident limit
    (big,) = alternating_ms([lambda: ops.kmeans_assign_tiled(x, c500)], args.reps)
    report("kmeans_assign_tiled (two tiles of 327 and 173)", big, args.points, 500)
    l500, l300 = ops.kmeans_assign_tiled(xt, c500), ops.kmeans_assign(xt, c300)
    acc_t, acc_r = alternating_ms([lambda: ops.kmeans_accumulate_tiled(xt, l500, 500), lambda: ops.kmeans_accumulate(xt, l300, 300)], args.reps)
    print(json.dumps({"what": "kmeans_accumulate_tiled", "P": args.train_points, "d": d, "k": 500, "ms": round(acc_t, 4)}))
    print(json.dumps({"what": "kmeans_accumulate (resident)", "P": args.train_points, "d": d, "k": 300, "ms": round(acc_r, 4)}))


if __name__ == "__main__":
    main()
