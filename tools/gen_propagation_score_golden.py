#!/usr/bin/env python3
"""Writes tests/golden/propagation_score.npz from the reference's own ``metrics.PredsmIoU.compute_propagation_score``
(``metrics.py:271-346``) and ``evaluation.evaluate_propagation`` (``evaluation.py:228-246``), N15.

Runs on the CPU of the build container, next to a reference checkout (``oracle/gen_golden.py``'s stand-ins for the third-party
imports), with ``MKL_CBWR=COMPATIBLE`` like every golden here:

    MKL_CBWR=COMPATIBLE python tools/gen_propagation_score_golden.py

The fixture holds data only: three clips of 5 frames at 24 x 20 (stored whole, int16) and the reference's results on them.
  - ``gts`` / ``preds`` [3, 5, 24, 20]: objects 1 ... 3 as moving rectangles, the predictions shifted and noisy copies.  Object 2 is
    missing from frames 1 and 3 of every clip's ground truth (the divisor is the number of frames that hold an object); object 3 is
    missing from clip 1 altogether; label 5 occurs in the predictions of clip 2 only (an object of the prediction alone: it is scored
    when the predictions are stored as ``gt``, which is what ``evaluate_propagation`` does).
  - ``clip<i>_scores``: ``compute_propagation_score`` after ``update(gts[i, j], preds[i, j])`` for every frame j.
  - ``clip<i>_scores_swapped``: the same after ``update(preds[i, j], gts[i, j])``, the order ``evaluate_propagation`` uses.
  - ``evaluate_propagation``: the reference function on the whole batch.
"""
from __future__ import annotations

import contextlib
import io
import os
import sys

os.environ.setdefault("MKL_CBWR", "COMPATIBLE")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle"))   # timet_oracle, which oracle.gen_golden's stand-ins import by that name
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

CLIPS, FRAMES, H, W, SEED = 3, 5, 24, 20, 31


def make_clips(clips=CLIPS, frames=FRAMES, H=H, W=W, seed=SEED):
    """-> (gts, preds) int16 [clips, frames, H, W]."""
    rng = np.random.default_rng(seed)
    gts = np.zeros((clips, frames, H, W), np.int16)
    preds = np.zeros((clips, frames, H, W), np.int16)
    for i in range(clips):
        for obj in (1, 2, 3):
            if obj == 3 and i == 1:
                continue
            y, x = int(rng.integers(0, H - 8)), int(rng.integers(0, W - 8))
            h, w = int(rng.integers(4, 9)), int(rng.integers(4, 9))
            for j in range(frames):
                dy, dx = int(rng.integers(-1, 2)), int(rng.integers(-1, 2))
                y, x = min(max(y + dy, 0), H - h), min(max(x + dx, 0), W - w)
                if not (obj == 2 and j in (1, 3)):
                    gts[i, j, y:y + h, x:x + w] = obj
                sy, sx = int(rng.integers(-2, 3)), int(rng.integers(-2, 3))
                py, px = min(max(y + sy, 0), H - h), min(max(x + sx, 0), W - w)
                preds[i, j, py:py + h, px:px + w] = obj
        noise = rng.random((frames, H, W)) < 0.04
        preds[i][noise] = rng.integers(0, 4, int(noise.sum()))
    preds[2, 1:4, 0:3, 0:4] = 5
    return gts, preds


def main():
    import torch

    from oracle.gen_golden import OUT, import_reference

    import_reference()
    import evaluation as ref_evaluation   # the reference modules
    import metrics as ref_metrics

    gts, preds = make_clips()
    out = {"gts": gts, "preds": preds}
    tg, tp = torch.from_numpy(gts.astype(np.int64)), torch.from_numpy(preds.astype(np.int64))
    with contextlib.redirect_stdout(io.StringIO()):
        for i in range(CLIPS):
            for tag, (a, b) in dict(scores=(tg, tp), scores_swapped=(tp, tg)).items():
                m = ref_metrics.PredsmIoU(4, 4)
                for j in range(FRAMES):
                    m.update(a[i, j].flatten(), b[i, j].flatten())
                out[f"clip{i}_{tag}"] = np.array(m.compute_propagation_score(True), np.float64)
        out["evaluate_propagation"] = np.float64(ref_evaluation.evaluate_propagation(ref_metrics.PredsmIoU(4, 4), tg, tp))
    for k, v in out.items():
        if k.startswith("clip") or k == "evaluate_propagation":
            print(k, v)
    path = os.path.join(OUT, "propagation_score.npz")
    np.savez_compressed(path, **out)
    print(f"{path} written ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
