#!/usr/bin/env python3
"""Times the scoring step of the three evaluation protocols, ``evaluation.evaluate_localizations`` alone (N15), on one GPU, and - with
``--kernel`` - the segmented confusion kernel by itself.

Scoring cases (synthetic maps that are constant on 16 x 16 blocks, as up-sampled token maps are; predictions int16 like
``cluster_features``' output, a noisy function of the ground truth):
  frame-wise / sample-wise   16 clips x 4 frames at 224 x 224, k = 10 against 4 ground-truth values
  dataset-wise 21            1449 clips x 1 frame at 112 x 112, k = 21 against 21 classes, a 255 border on every frame
  dataset-wise 500           the same frames, k = 500, many-to-one (the over-clustering protocol)
Wall clock around ``torch.cuda.synchronize()``, one warm-up call, then ``--reps`` calls (5): the loop this replaces is bound by launches
and host round trips, which device events would not see.  Beside the frame-wise and sample-wise figures the tool prints the time of
``clustering.cluster_features`` on a batch of that shape (14 x 14 tokens of 384 columns), the step that runs straight before the scoring.

The scoring part calls nothing but ``evaluate_localizations`` and ``cluster_features``, so it runs unchanged on a commit from before
N15: ``--tree PATH`` imports the package from another (built) checkout.  For a before / after, run the two trees in turn on one box,
more than once:

    python tools/bench_eval_scoring.py                      # this tree
    python tools/bench_eval_scoring.py --tree ../parent     # a checkout of the parent commit, built

``--kernel`` (this tree only): HIP events around ``hip_ops.confusion_counts_segments`` and, alternating with it call by call,
``hip_ops.confusion_counts`` on the same elements, 10 calls each, at 64 x 50176 elements with 5 x 10 classes (frame-wise) and
1449 x 12544 = 18.2 M elements with 21 x 21 and 21 x 500 (dataset-wise; the square entry counts max(Cg, Cp)^2 cells); int16 and int64
predictions.  Each line carries the byte floor of its shape - 2 or 8 bytes of pred and 8 of gt per element at 6.3 TB/s, computed, not
measured - and the fraction of it the segmented kernel reached.  The one-atomic-per-element form of the kernel is a variant build:

    tools/build_variant.sh confseg_nomerge confusion.hip -DTT_CONFSEG_NO_MERGE
    TT_LIB_PATH=tools/bin/libconfseg_nomerge.so python tools/bench_eval_scoring.py --kernel

``--match`` (this tree only, N20): HIP events around ``hip_ops.match_segments`` alone, ``--kernel-reps`` calls after one warm-up, on the
counts of such maps: 64 segments of 5 x 10 and of 21 x 21, Hungarian, and one segment of 21 x 500, many-to-one.  Each line carries the
statuses the kernel reported and the largest class sets it met.

Prints one JSON line per case.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 6.3e12


def block_maps(torch, frames, R, classes, k, seed, border):
    """-> (gts int64, preds int16) [frames, R, R] on the GPU, constant on 16 x 16 blocks; 70 % of the blocks' predictions follow gt."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    g = R // 16
    gt = torch.randint(0, classes, (frames, g, g), generator=gen, device="cuda")
    free = torch.randint(0, k, (frames, g, g), generator=gen, device="cuda")
    follow = torch.rand((frames, g, g), generator=gen, device="cuda") < 0.7
    sub = max(k // classes, 1)
    pred = torch.where(follow, (gt * sub + free % sub) % k, free)
    up = lambda t: t.repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous()   # noqa: E731
    gts, preds = up(gt), up(pred).to(torch.int16)
    if border:
        gts[:, 0, :] = gts[:, -1, :] = 255
        gts[:, :, 0] = gts[:, :, -1] = 255
    return gts, preds


def features(bs, fs, n_tok, dim, synth, torch):
    import numpy as np

    protos = synth.normal("bench.es.p", (12, dim)) * 3
    which = np.arange(bs * fs * n_tok) * 7 % 12
    noise = synth.normal("bench.es.n", (bs * fs * n_tok, dim))
    return torch.from_numpy((protos[which] + 0.5 * noise).astype(np.float32).reshape(bs, fs, n_tok, dim)).cuda()


def wall_ms(torch, fn, reps):
    fn()   # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def report(**kw):
    ms = kw["ms"]
    kw.update(ms=[round(m, 3) for m in ms], mean_ms=round(sum(ms) / len(ms), 3), min_ms=round(min(ms), 3))
    print(json.dumps(kw), flush=True)


def scoring(args, tree, torch):
    from timetuning_amd import synth
    from timetuning_amd.clustering import cluster_features
    from timetuning_amd.evaluation import evaluate_localizations
    from timetuning_amd.metrics import PredsmIoU

    bs, fs, R, k = 16, 4, 224, 10
    gts, preds = block_maps(torch, bs * fs, R, 4, k, 1, border=False)
    gts, preds = gts.view(bs, fs, R, R), preds.view(bs, fs, R, R)
    feats = features(bs, fs, 14 * 14, 384, synth, torch)
    for protocol in ("frame-wise", "sample-wise"):
        ev = PredsmIoU(k, k)
        score = evaluate_localizations(ev, gts, preds, protocol)
        report(what="evaluate_localizations", case=protocol, bs=bs, fs=fs, R=R, k=k, score=score,
               ms=wall_ms(torch, lambda: evaluate_localizations(ev, gts, preds, protocol), args.reps), tree=tree)
        report(what="cluster_features", case=protocol, bs=bs, fs=fs, R=R, k=k,
               ms=wall_ms(torch, lambda: cluster_features(feats, k, 14, R, protocol), args.reps), tree=tree)
    frames, R = 1449, 112
    for k, many in ((21, False), (500, True)):
        gts, preds = block_maps(torch, frames, R, 21, k, 2, border=True)
        gts, preds = gts.view(frames, 1, R, R), preds.view(frames, 1, R, R)
        ev = PredsmIoU(k, 21)
        score = evaluate_localizations(ev, gts, preds, "dataset-wise", None, many)
        report(what="evaluate_localizations", case=f"dataset-wise {k}", bs=frames, fs=1, R=R, k=k, many_to_one=many, score=score,
               ms=wall_ms(torch, lambda: evaluate_localizations(ev, gts, preds, "dataset-wise", None, many), args.reps), tree=tree)


def kernel(args, tree, torch):
    from timetuning_amd import _lib
    from timetuning_amd import hip_ops as ops

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for name, S, n, classes, k in (("frame-wise", 64, 50176, 5, 10), ("dataset-wise 21", 1, 1449 * 12544, 21, 21),
                                   ("dataset-wise 500", 1, 1449 * 12544, 21, 500)):
        R = 224 if S > 1 else 112
        gts, preds = block_maps(torch, S * n // (R * R), R, classes, k, 3, border=S == 1)
        gt = gts.view(S, n)
        C = max(classes, k)
        for pred in (preds.view(S, n), preds.view(S, n).long()):
            flat = pred.reshape(-1).long()
            ops.confusion_counts_segments(pred, gt, classes, k, 255)   # warm-up of both
            ops.confusion_counts(flat, gt.view(-1), C)
            seg, old = [], []
            for _ in range(args.kernel_reps):
                seg.append(event_ms(lambda: ops.confusion_counts_segments(pred, gt, classes, k, 255)))
                old.append(event_ms(lambda: ops.confusion_counts(flat, gt.view(-1), C)))
            floor_ms = S * n * (pred.element_size() + 8) / HBM_BYTES_PER_S * 1e3
            report(what="confusion_counts_segments", case=name, S=S, n=n, Cg=classes, Cp=k, pred=str(pred.dtype), ms=seg,
                   floor_ms=round(floor_ms, 4), fraction_of_floor=round(floor_ms / (sum(seg) / len(seg)), 3), lib=_lib.LIB_PATH)
            report(what="confusion_counts", case=name, n=S * n, C=C, pred="torch.int64", ms=old, lib=_lib.LIB_PATH)


def match(args, tree, torch):
    """HIP events around ``hip_ops.match_segments`` alone, on the counts of block maps like the scoring cases'."""
    from timetuning_amd import _lib
    from timetuning_amd import hip_ops as ops

    for name, S, R, classes, k, mode in (("frame-wise", 64, 224, 5, 10, "hungarian"), ("frame-wise 21", 64, 224, 21, 21, "hungarian"),
                                         ("dataset-wise 500", 1, 112, 21, 500, "many_to_one")):
        frames = S if S > 1 else 1449
        gts, preds = block_maps(torch, frames, R, classes, k, 3, border=S == 1)
        counts = ops.confusion_counts_segments(preds.view(S, -1), gts.view(S, -1), classes, k, 255)
        ops.match_segments(counts, mode)   # warm-up
        ms = []
        for _ in range(args.kernel_reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = ops.match_segments(counts, mode)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        info = out.info.cpu()
        report(what="match_segments", case=name, S=S, Cg=classes, Cp=k, mode=mode, statuses=sorted(set(info[:, 0].tolist())),
               n_gt=int(info[:, 1].max()), n_pred=int(info[:, 2].max()), ms=ms, lib=_lib.LIB_PATH)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE, help="the checkout whose timetuning_amd is timed (default: the one this file is in)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel", action="store_true", help="time the segmented kernel alone instead of the scoring step")
    ap.add_argument("--match", action="store_true", help="time match_segments alone instead of the scoring step")
    ap.add_argument("--kernel-reps", type=int, default=10)
    args = ap.parse_args(argv)
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_scoring.py needs a GPU: there is nothing to time without one")
    (kernel if args.kernel else match if args.match else scoring)(args, tree, torch)


if __name__ == "__main__":
    main()
