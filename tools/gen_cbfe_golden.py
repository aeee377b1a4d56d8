#!/usr/bin/env python3
"""Writes tests/golden/cbfe.npz from the reference's own ``cluster_based_foreground_extraction`` functions (N6).

Runs on the CPU of the build container, next to a reference checkout (``oracle/gen_golden.py``'s stand-ins for the third-party
imports; ``cv2.__version__`` is set on the cv2 stand-in, which the reference's imports read), with ``MKL_CBWR=COMPATIBLE`` like every
golden here:

    MKL_CBWR=COMPATIBLE python tools/gen_cbfe_golden.py

Two cases, k = 60 and k = 300 (M = 40 images of 100 x 100): cluster maps, attention masks and VOC labels (255 borders) from
``cluster_based_foreground_extraction.synthetic_cluster_maps`` - the inputs are NOT stored, only samples that the tests check they
regenerate.  The maps have precision ties at exactly 1.0 (straddling the cut positions) and 0.0.  Per case: ``get_cluster_precs``,
the ``np.argsort`` order the reference used, ``find_good_threshold``'s (precision, start, Jaccard) list, ``get_tuned_threshold``,
then on a second ("val") set of maps ``create_soft_masks`` (``create_overclustering_maps`` replaced by one returning those maps:
faiss is absent), its precisions and foreground ids, and ``eval_jac`` of the mask with both ``with_boundary`` values.  A small
hand-made case (stored whole) has an image with an empty GT foreground and an empty prediction: NaN Jaccards.  Also
``process_data_group`` on all 256 label values and ``interpolate`` on index-valued features.
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

M, R = 40, 100
CASES = {60: 11, 300: 12}   # k -> seed of the train maps (the val maps use seed + 100)
VAL_SEED_OFFSET = 100


def sample(t):
    """What the fixture keeps of a regenerated [M, R, R] map."""
    return t[:, ::17, ::13]


def nan_case():
    """3 images of 8 x 8, k = 4: image 0 is all cluster 0 with GT 0 and attention 0 (empty union at the cut)."""
    import torch

    cl = torch.zeros((3, 8, 8), dtype=torch.int64)
    at = torch.zeros_like(cl)
    gt = torch.zeros_like(cl)
    cl[1, :, :4], cl[1, :, 4:] = 1, 2
    at[1, :2, :4] = 1            # cluster 1: precision 0.25
    at[1, :, 4:] = 1             # cluster 2: 1.0
    gt[1, :, 4:] = 1
    gt[1, :, 6] = 255
    cl[2, :4], cl[2, 4:] = 3, 2
    at[2, :3] = 1                # cluster 3: 0.75
    at[2, 4:] = 1
    gt[2, 2:6] = 2
    return cl, at, gt


def main():
    import torch

    ref = import_reference()
    import cv2

    cv2.__version__ = "4.5.5"
    import cluster_based_foreground_extraction as cb   # the reference module

    from timetuning_amd.cluster_based_foreground_extraction import synthetic_cluster_maps

    def ref_cbfe(k):
        obj = cb.ClusterBasedForegroundExtraction.__new__(cb.ClusterBasedForegroundExtraction)
        torch.nn.Module.__init__(obj)
        obj.k_fg_extraction, obj.eval_resolution, obj.device, obj.eval_feature_dim = k, R, "cpu", 50
        return obj

    out = {"cfg": np.array([M, R, VAL_SEED_OFFSET], np.int64), "ks": np.array(sorted(CASES), np.int64)}
    for k, seed in sorted(CASES.items()):
        cl, at, gt = synthetic_cluster_maps(M, R, k, seed)
        vcl, vat, vgt = synthetic_cluster_maps(M, R, k, seed + VAL_SEED_OFFSET)
        p = f"k{k}_"
        out[p + "seed"] = np.int64(seed)
        out[p + "clusters_sample"] = sample(cl).numpy().astype(np.int16)
        out[p + "attn_sample"] = sample(at).numpy().astype(np.uint8)
        out[p + "gt_sample"] = sample(gt).numpy().astype(np.uint8)
        out[p + "val_clusters_sample"] = sample(vcl).numpy().astype(np.int16)
        precs = cb.get_cluster_precs(cl, at, k)
        out[p + "precs"] = np.array(precs, np.float64)
        out[p + "order"] = np.argsort(precs).astype(np.int32)
        res = cb.find_good_threshold(cl, gt, precs, k)
        out[p + "cut_prec"] = np.array([r[0] for r in res], np.float64)
        out[p + "cut_start"] = np.array([r[1] for r in res], np.int64)
        out[p + "cut_jac"] = np.array([r[2] for r in res], np.float64)
        obj = ref_cbfe(k)
        th = obj.get_tuned_threshold(at[:, None], gt[:, None], cl[:, None])
        out[p + "threshold"] = np.float64(th)
        obj.create_overclustering_maps = lambda features, _m=vcl: _m[:, None]
        mask = obj.create_soft_masks(vat[:, None], vgt[:, None], None, th)
        out[p + "soft_mask_bits"] = np.packbits(mask.numpy().astype(np.uint8).ravel())
        vprecs = cb.get_cluster_precs(vcl, vat, k)
        out[p + "val_precs"] = np.array(vprecs, np.float64)
        out[p + "val_order"] = np.argsort(vprecs).astype(np.int32)
        out[p + "val_fg_ids"] = np.argsort(vprecs)[np.where((np.sort(vprecs) >= th) == True)[0][0]:].astype(np.int32)  # noqa: E712
        out[p + "eval_jac_boundary"] = np.float64(cb.eval_jac(vgt, mask, with_boundary=True))
        out[p + "eval_jac_no_boundary"] = np.float64(cb.eval_jac(vgt, mask, with_boundary=False))
        ties1 = int((np.array(precs) == 1.0).sum())
        print(f"k {k}: threshold {th}, best cut {res[-1][1]} jac {res[-1][2]:.6f}, precision-1.0 ties {ties1}, "
              f"0.0 ties {int((np.array(precs) == 0.0).sum())}, val jac {out[p + 'eval_jac_boundary']:.6f}")
    # NaN: an image with an empty GT foreground and an empty prediction
    cl, at, gt = nan_case()
    precs = cb.get_cluster_precs(cl, at, 4)
    res = cb.find_good_threshold(cl, gt, precs, 4)
    out["nan_clusters"], out["nan_attn"], out["nan_gt"] = cl.numpy().astype(np.int16), at.numpy().astype(np.uint8), gt.numpy().astype(np.uint8)
    out["nan_precs"] = np.array(precs, np.float64)
    out["nan_order"] = np.argsort(precs).astype(np.int32)
    out["nan_cut_start"] = np.array([r[1] for r in res], np.int64)
    out["nan_cut_jac"] = np.array([r[2] for r in res], np.float64)
    fg = ref_cbfe(4).make_post_matching_maps(cl, 0.5, precs)
    out["nan_eval_jac"] = np.float64(cb.eval_jac(gt, fg, with_boundary=True))
    # process_data_group's x 255 then truncating .long() on every label value stored as v / 255
    ann = torch.arange(256, dtype=torch.float32).div(255).view(1, 1, 16, 16)
    _, lab = cb.process_data_group((torch.zeros(1, 3, 2, 2), ann), cb.ScaleType.ZERO_TO_255)
    out["labels256"] = lab.numpy().astype(np.int16)
    # interpolate: index-valued features, so the output names the source token of every pixel
    for g, r, dim in ((28, 100, 1), (14, 37, 3)):
        obj = ref_cbfe(1)
        obj.spatial_resolution = g
        feats = torch.arange(2 * g * g * dim, dtype=torch.float32).view(2, 1, g * g, dim)
        up = obj.interpolate(feats, r)
        out[f"interp_{g}_{r}"] = up.numpy().astype(np.int32)
    path = os.path.join(OUT, "cbfe.npz")
    np.savez_compressed(path, **out)
    print(f"{path} written ({os.path.getsize(path)} bytes); NaN case jacs {out['nan_cut_jac']}, eval_jac {out['nan_eval_jac']}")


if __name__ == "__main__":
    main()
