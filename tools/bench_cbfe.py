#!/usr/bin/env python3
"""Times the cluster-based foreground extraction statistics (N6) on one GPU.

1. The kernels at Pascal trainaug scale (M = 10 582 images, R = 100, k = 300): tt_cbfe_cluster_stats + tt_cbfe_cluster_precs +
   tt_cbfe_cut_jaccard (60 candidate cuts), device time; and the host functions get_cluster_precs + find_good_threshold end to end.
2. The reference's loops (get_cluster_precs, :85-108; find_good_threshold with eval_jac, :111-153) restated in GPU torch, timed on a
   subset of the images and EXTRAPOLATED linearly to M (marked as such in the output).
3. k-means assignment of the nearest-upsampled points: once per token + tt_nearest_upsample_labels, against tt_kmeans_assign on
   the materialised points (M_assign images, g = 28 -> R = 100, d = 50, k = 300).

    python tools/bench_cbfe.py [--M 10582] [--subset 64] [--assign-images 1000]

Prints one JSON line per measurement.  The maps are synthetic_cluster_maps of 256 images, tiled to M.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from timetuning_amd import cluster_based_foreground_extraction as CB, hip_ops as ops  # noqa: E402
from timetuning_amd.clustering import Kmeans, nearest_index_table  # noqa: E402


def device_ms(fn, reps=5, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def wall_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def ref_cluster_precs(cluster, mask):
    """get_cluster_precs' loop restated in GPU torch (the reference's own operations, per image and cluster)."""
    occ, cum = {}, {}
    for img in range(cluster.size(0)):
        a, c = mask[img].flatten(), cluster[img].flatten()
        for cid in torch.unique(c):
            ta, tc = a == 1, c == cid
            tp = torch.sum(ta & tc).item()
            fp = torch.sum(~ta & tc).item()
            prec = float(tp) / max(float(tp + fp), 1e-8)
            occ[cid.item()] = occ.get(cid.item(), 0) + 1
            cum[cid.item()] = cum.get(cid.item(), 0.0) + prec
    return occ, cum


def ref_one_cut(clusters, gt, fg_ids):
    """One candidate of find_good_threshold: the mask by one masked assignment per foreground cluster, then eval_jac's loop."""
    mask = torch.zeros_like(clusters)
    for i in fg_ids:
        mask[clusters == int(i)] = 1
    jacs = 0
    for k, m in enumerate(gt):
        fg = (m != 0).float()
        inter = torch.sum(torch.sum(fg * mask[k], dim=-1), dim=-1)
        union = torch.sum(torch.sum((fg + mask[k]) > 0, dim=-1), dim=-1)
        jacs += inter / union
    return (jacs / gt.size(0)).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=10582)
    ap.add_argument("--R", type=int, default=100)
    ap.add_argument("--k", type=int, default=300)
    ap.add_argument("--subset", type=int, default=64, help="images the restated reference loops run on")
    ap.add_argument("--cuts", type=int, default=2, help="candidate cuts the restated reference runs")
    ap.add_argument("--assign-images", type=int, default=1000)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    M, R, k = a.M, a.R, a.k
    base = 256
    cl0, at0, gt0 = CB.synthetic_cluster_maps(base, R, k, seed=7)
    reps = (M + base - 1) // base
    cl = cl0.repeat(reps, 1, 1)[:M].to(dev).view(M, R * R).contiguous()
    at = at0.repeat(reps, 1, 1)[:M].to(dev).view(M, R * R).contiguous()
    gt = gt0.repeat(reps, 1, 1)[:M].to(dev).view(M, R * R).contiguous()
    gpu = torch.cuda.get_device_name(0)

    starts = torch.tensor(CB.cut_positions(k), dtype=torch.int32, device=dev)
    stats, gt_fg = ops.cbfe_cluster_stats(cl, at, gt, k)
    precs, _ = ops.cbfe_cluster_precs(stats)
    order = torch.from_numpy(np.argsort(precs.cpu().numpy()).astype(np.int32)).to(dev)
    t_stats = device_ms(lambda: ops.cbfe_cluster_stats(cl, at, gt, k, check=False, range_flag=torch.zeros(1, dtype=torch.int32, device=dev)))
    t_precs = device_ms(lambda: ops.cbfe_cluster_precs(stats))
    t_cut = device_ms(lambda: ops.cbfe_cut_jaccard(stats, gt_fg, order, starts))
    print(json.dumps({"what": "kernels: stats + precs + 60 cuts", "M": M, "R": R, "k": k, "stats_ms": round(t_stats, 3),
                      "precs_ms": round(t_precs, 3), "cut_jaccard_ms": round(t_cut, 3), "total_ms": round(t_stats + t_precs + t_cut, 3),
                      "gpu": gpu}), flush=True)
    clm, atm, gtm = cl.view(M, R, R), at.view(M, R, R), gt.view(M, R, R)
    CB.find_good_threshold(clm, gtm, CB.get_cluster_precs(clm, atm, k), k)   # warm
    t_host = wall_s(lambda: CB.find_good_threshold(clm, gtm, CB.get_cluster_precs(clm, atm, k), k))
    print(json.dumps({"what": "get_cluster_precs + find_good_threshold (host functions, wall)", "M": M, "s": round(t_host, 4)}), flush=True)

    # the reference's loops in GPU torch, on a subset, extrapolated
    S = min(a.subset, M)
    ref_cluster_precs(clm[:2], atm[:2])   # warm
    t_p = wall_s(lambda: ref_cluster_precs(clm[:S], atm[:S]))
    sorted_args = np.argsort(precs.cpu().numpy())
    cut_list = CB.cut_positions(k)[: a.cuts]
    ref_one_cut(clm[:2], gtm[:2], sorted_args[cut_list[0]:])   # warm
    t_c = wall_s(lambda: [ref_one_cut(clm[:S], gtm[:S], sorted_args[s:]) for s in cut_list])
    n_cuts = len(CB.cut_positions(k))
    est_p = t_p * M / S
    est_c = t_c / len(cut_list) * n_cuts * M / S
    print(json.dumps({"what": "reference loops restated in GPU torch, EXTRAPOLATED", "measured_images": S, "measured_cuts": len(cut_list),
                      "M": M, "get_cluster_precs_s_est": round(est_p, 2), "find_good_threshold_s_est": round(est_c, 2),
                      "total_s_est": round(est_p + est_c, 2), "speedup_vs_kernels_est": round((est_p + est_c) * 1e3 / (t_stats + t_precs + t_cut), 1)}),
          flush=True)

    # assignment: per token + label upsampling, against the materialised points
    Ma, g, d = a.assign_images, 28, 50
    gen = torch.Generator(device="cpu").manual_seed(3)
    tokens = torch.randn((Ma, g * g, d), generator=gen).to(dev)
    km = Kmeans(d, k)
    km._centroids_dev = torch.randn((k, d), generator=gen).to(dev)
    iy, ix = nearest_index_table(g, R)
    idx = torch.from_numpy((iy.astype(np.int64)[:, None] * g + ix.astype(np.int64)[None, :]).reshape(-1)).to(dev)
    t_tok = device_ms(lambda: km.assign_upsampled(tokens, R), reps=3, warmup=1)
    pts = tokens[:, idx, :].reshape(Ma * R * R, d).contiguous()
    t_mat = device_ms(lambda: ops.kmeans_assign(pts, km._centroids_dev), reps=3, warmup=1)
    same = bool(torch.equal(km.assign_upsampled(tokens, R).view(-1), ops.kmeans_assign(pts, km._centroids_dev).long()))
    t_build = device_ms(lambda: tokens[:, idx, :].reshape(Ma * R * R, d).contiguous(), reps=3, warmup=1)
    print(json.dumps({"what": "k-means assignment: per token vs materialised", "images": Ma, "g": g, "R": R, "d": d, "k": k,
                      "token_ms": round(t_tok, 3), "materialised_ms": round(t_mat, 3), "materialise_build_ms": round(t_build, 3),
                      "materialised_bytes": pts.numel() * 4, "labels_equal": same}), flush=True)


if __name__ == "__main__":
    main()
