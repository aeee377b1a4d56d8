#!/usr/bin/env python3
"""Writes tests/golden/davis_metrics.npz from the reference's own DAVIS metric functions (N7, ``mask_propagation.py:501-715``).

Runs on the CPU of the build container, next to a reference checkout (``oracle/gen_golden.py``'s stand-ins for the third-party
imports), with ``MKL_CBWR=COMPATIBLE`` like every golden here:

    MKL_CBWR=COMPATIBLE python tools/gen_davis_metrics_golden.py

cv2 and skimage are not installed.  ``f_measure`` calls ``cv2.dilate`` and imports ``skimage.morphology.disk``; both are replaced
by stand-ins written from their published definitions (below), so the fixture pins the reference's own code around them but NOT
those two libraries: "parity unpinned" for cv2 / skimage, as N1's blur and labelling stand-ins.
    disk(r)          X^2 + Y^2 <= r^2 over the grid arange(-r, r + 1) in both directions (uint8)
    dilate(src, k)   dst(y, x) = max over the set (i, j) of k of src(y + i - k.rows // 2, x + j - k.cols // 2); outside the image
                     contributes nothing (cv2's default anchor and constant border for dilation)

Inputs are ``mask_propagation.synthetic_davis_labels`` maps, NOT stored: only samples the tests check they regenerate.  Cases:
  - label maps at 64 x 96 (bound_th 0.008, 0.02, 2, 2.5) and 240 x 427, 1 x 53 and 53 x 1 (0.008), each with and without void:
    per object o, ``db_eval_iou`` and ``db_eval_boundary`` of (gt == o, pred == o)
  - empty prediction, empty GT, both empty (2-D ``db_eval_iou`` / ``f_measure``)
  - ``_seg2bmap`` of three maps (stored whole, small)
  - ``db_statistics`` at lengths 1, 2, 3, 5, 17, 300 (values with NaNs, stored)
  - ``evaluate_semisupervised`` with 2 predicted objects for 3 GT objects
"""
from __future__ import annotations

import os
import sys

os.environ.setdefault("MKL_CBWR", "COMPATIBLE")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle"))   # timet_oracle, which oracle.gen_golden's stand-ins import by that name
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

from oracle.gen_golden import OUT, import_reference  # noqa: E402

# name -> (T, H, W, O, seed, bound_ths)
LABEL_CASES = {
    "small": (4, 64, 96, 3, 1, (0.008, 0.02, 2, 2.5)),
    "mid": (2, 240, 427, 3, 2, (0.008,)),
    "row": (3, 1, 53, 2, 3, (0.008,)),
    "col": (3, 53, 1, 2, 4, (0.008,)),
}
STAT_LENGTHS = (1, 2, 3, 5, 17, 300)
SEMI = (3, 40, 56, 5)   # T, H, W, seed of evaluate_semisupervised (3 GT objects, 2 predicted)


def disk_standin(radius, dtype=np.uint8):
    L = np.arange(-radius, radius + 1)
    X, Y = np.meshgrid(L, L)
    return np.array((X ** 2 + Y ** 2) <= radius ** 2, dtype=dtype)


def dilate_standin(src, kernel):
    src = np.asarray(src)
    H, W = src.shape
    ay, ax = kernel.shape[0] // 2, kernel.shape[1] // 2
    out = np.zeros_like(src)
    for i, j in zip(*np.nonzero(kernel)):
        dy, dx = i - ay, j - ax   # dst(y, x) |= src(y + dy, x + dx)
        ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
        xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
        out[yd, xd] = np.maximum(out[yd, xd], src[ys, xs])
    return out


def sample(a):
    return a[:, ::7, ::11]


def main():
    ref = import_reference()
    mp = ref["mp"]
    mp.cv2.dilate = dilate_standin
    sys.modules["skimage.morphology"].disk = disk_standin

    from timetuning_amd.mask_propagation import synthetic_davis_labels

    out = {}
    for name, (T, H, W, O, seed, ths) in LABEL_CASES.items():
        gt, pred, void = synthetic_davis_labels(T, H, W, O, seed)
        out[f"{name}_cfg"] = np.array([T, H, W, O, seed], np.int64)
        out[f"{name}_bound_th"] = np.array(ths, np.float64)
        out[f"{name}_gt_sample"], out[f"{name}_pred_sample"], out[f"{name}_void_sample"] = sample(gt), sample(pred), sample(void)
        for vname, v in (("novoid", None), ("void", void)):
            J = np.stack([mp.db_eval_iou(gt == o, pred == o, v) for o in range(1, O + 1)])
            out[f"{name}_{vname}_J"] = J
            for k, th in enumerate(ths):
                F = np.stack([mp.db_eval_boundary(gt == o, pred == o, v, bound_th=th) for o in range(1, O + 1)])
                out[f"{name}_{vname}_F{k}"] = F
            print(f"{name} {vname}: J {J.mean():.4f}, F {out[f'{name}_{vname}_F0'].mean():.4f}")
    # empty masks (2-D): pred empty, GT empty, both
    g2, p2, _ = synthetic_davis_labels(1, 16, 16, 1, 6)
    g2, p2 = (g2[0] == 1).astype(np.uint8), (p2[0] == 1).astype(np.uint8)
    z = np.zeros_like(g2)
    out["empty_gt"], out["empty_pred"] = g2, p2
    out["empty_J"] = np.array([mp.db_eval_iou(g2, z), mp.db_eval_iou(z, p2), mp.db_eval_iou(z, z)], np.float64)
    out["empty_F"] = np.array([mp.f_measure(z, g2), mp.f_measure(p2, z), mp.f_measure(z, z)], np.float64)
    # _seg2bmap
    rng = np.random.default_rng(7)
    for k, shape in enumerate(((23, 31), (1, 29), (29, 1))):
        seg = (rng.random(shape) < 0.5).astype(np.uint8)
        out[f"bmap{k}_seg"], out[f"bmap{k}"] = seg, mp._seg2bmap(seg).astype(np.uint8)
    # db_statistics
    for n in STAT_LENGTHS:
        v = rng.random(n)
        v[rng.random(n) < 0.1] = np.nan
        out[f"stats{n}_values"] = v
        out[f"stats{n}"] = np.array(mp.db_statistics(v), np.float64)
    # evaluate_semisupervised: 3 GT objects, 2 predicted
    T, H, W, seed = SEMI
    gt, pred, void = synthetic_davis_labels(T, H, W, 3, seed)
    gm = np.stack([gt == o for o in (1, 2, 3)]).astype(np.uint8)
    rm = np.stack([pred == o for o in (1, 2)]).astype(np.uint8)
    J, F = mp.evaluate_semisupervised(gm, rm, void, ("J", "F"))
    out["semi_cfg"] = np.array(SEMI, np.int64)
    out["semi_J"], out["semi_F"] = J, F
    path = os.path.join(OUT, "davis_metrics.npz")
    np.savez_compressed(path, **out)
    print(f"{path} written ({os.path.getsize(path)} bytes); empty J {out['empty_J']}, F {out['empty_F']}")


if __name__ == "__main__":
    main()
