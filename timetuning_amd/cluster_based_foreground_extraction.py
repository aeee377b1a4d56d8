"""Cluster-based foreground extraction (CBFE) with the reference's surface (``cluster_based_foreground_extraction.py``), N6.

The Pascal-VOC "overclustering with foreground masks" evaluation: the features of every image are over-clustered (k = 300 k-means
on their PCA-50 nearest upsampling to R x R), every cluster is scored by the share of its pixels inside the ViT-attention foreground
(``get_cluster_precs``), the precision cut that maximises the Jaccard index against the ground truth is searched on the train set
(``find_good_threshold``, ``get_tuned_threshold``), and the val clusters above it become foreground masks
(``make_post_matching_maps``), which ``evaluation.Evaluator(fg_masks=...).evaluate(use_mask=True)`` consumes.

The reference runs these statistics as Python loops over images and clusters (four ``.item()`` round trips per pair) and builds a
full-dataset mask per candidate cut.  Here they are per-(image, cluster) integer counts on the GPU (include/timetuning_hip.h, N6):
``tt_cbfe_cluster_stats`` -> ``tt_cbfe_cluster_precs`` (get_cluster_precs bit for bit) and ``tt_cbfe_cut_jaccard`` (all candidate
cuts from suffix sums, eval_jac's fp32 sums bit for bit).  Sorting, tie order and the choice of the threshold stay on the host,
with the same numpy / Python calls the reference makes.

Memory.  The reference materialises the nearest upsampling of the PCA features of both sets ([N, 50, R, R] fp32: about 24 GB for
Pascal trainaug + val at R = 100) only to feed k-means.  Nearest upsampling repeats token vectors, so the k-means here runs on the
tokens (``clustering.Kmeans.train_upsampled`` / ``assign_upsampled``, bit-identical to the materialised run).  Only the returned
set's upsampled features are built, on the host as in the reference (its features live on the CPU), because
``get_foreground_masks`` returns them; the train set's never exist.

The token grid is read off the features (g = sqrt(tokens)); the reference takes it from ``spatial_resolution``, which is 14 for
``dino-s16`` whatever the input size.  The boundary F-score the reference prints on every run (``evaluate_bf_score``,
``bfscore.py``) runs when ``bf_score=True`` (CLI ``--bf_score``) from ``timetuning_amd.bfscore`` (one launch of ``tt_bf_counts`` for
all images; its cv2 border following pinned through a stand-in, N8); by default it is skipped and the output is unchanged.  Dataset readers
are out of scope as for the other entry points: ``main`` runs on synthetic data (``--dataset synthetic``).
"""
from __future__ import annotations

import argparse
from typing import NamedTuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import clustering
from . import hip_ops as ops
from .data_loader import add_decode_arguments
from .bfscore import evaluate_bf_score
from .clustering import Kmeans, nearest_index_table, normalize_and_transform
from .models import FeatureExtractor, process_attentions

ATTENTION_THRESHOLD = 0.65   # :242,252
# What the over-clustering's device loop (clustering.Kmeans(loop="device")) may take for its redos in flight: one redo's partials at the
# default k = 300 on 50 columns (73 MB) and no second - the host loop's footprint, which get_foreground_masks' memory bound was set with.
LOOP_WORKSPACE_BYTES = 96 << 20


class ScaleType:
    ZERO_TO_ONE = 0
    ZERO_TO_255 = 1


def process_data_group(data_group, scale=ScaleType.ZERO_TO_ONE):
    """:59-73.  (data, annotations, label) video batches lose their clip axis; (data, annotations) image batches gain a frame axis on
    ``data`` (in place).  With ZERO_TO_255 the annotations are multiplied by 255 in place and truncated with ``.long()``, as the
    reference does (for labels stored as v / 255 in fp32 the product rounds back to v: tests/golden/cbfe.npz holds all 256)."""
    if len(data_group) == 3:
        data, annotations = data_group[0].squeeze(1), data_group[1].squeeze(1)
    else:
        data, annotations = data_group
        data = data.unsqueeze_(1)
    if scale == ScaleType.ZERO_TO_255:
        annotations.mul_(255)
        annotations = annotations.long()
    return data, annotations


def normalize_features(features, reduction_dim=None):
    """:76-81: StandardScaler + PCA (``clustering.normalize_and_transform``) over all tokens of features [bs, fs, n, dim]."""
    bs, fs, n, dim = features.shape
    flat = features.reshape(bs * fs * n, dim)
    if not flat.is_cuda:
        flat = flat.cuda()
    out = normalize_and_transform(flat, dim if reduction_dim is None else int(reduction_dim))
    return out.view(bs, fs, n, out.shape[1])


def _dev_long(t) -> torch.Tensor:
    t = torch.as_tensor(t)
    if not t.is_cuda:
        t = t.cuda()
    return t.long().contiguous()


def get_cluster_precs(cluster, mask, k):
    """:85-107: per cluster id, the mean over the images that contain it of the share of its pixels with ``mask == 1``; a list of k
    Python floats.  Raises AssertionError, as the reference, when an id in [0, k) never occurs (or one outside it does)."""
    assert cluster.size(0) == mask.size(0)
    M = cluster.size(0)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    stats, _ = ops.cbfe_cluster_stats(_dev_long(cluster).view(M, -1), _dev_long(mask).view(M, -1), None, int(k), check=False,
                                      range_flag=flag)
    precs, occ = ops.cbfe_cluster_precs(stats)
    assert int(flag.item()) == 0 and bool((occ > 0).all())
    return precs.cpu().tolist()


def eval_jac(gt, pred_mask, with_boundary):
    """:111-129: the fp32 mean over the images of |GT fg & pred| / |GT fg | pred|, pred_mask a 0/1 mask; the GT foreground is
    ``gt != 0``, or ``gt != 0 and gt != 255`` without ``with_boundary``.  An image with an empty union makes the result NaN."""
    M = gt.size(0)
    stats, gt_fg = ops.cbfe_cluster_stats(_dev_long(pred_mask).view(M, -1), None, _dev_long(gt).view(M, -1), 2,
                                          ignore=-1 if with_boundary else 255)
    dev = stats.device
    jac = ops.cbfe_cut_jaccard(stats, gt_fg, torch.tensor([0, 1], dtype=torch.int32, device=dev),
                               torch.tensor([1], dtype=torch.int32, device=dev))
    return float(jac[0].item())


def cut_positions(k: int):
    """The candidate cuts of find_good_threshold (:144): 55% to 75% of the clusters to background."""
    return list(range(int(0.55 * k), int(0.75 * k)))


def find_good_threshold(train_clusters, train_gt, precs, k):
    """:140-153: for every cut ``start`` the clusters ``np.argsort(precs)[start:]`` are foreground; returns the list of
    ``(np.sort(precs)[start], start, jaccard)`` sorted (stably) by the Jaccard index of ``eval_jac(with_boundary=True)``."""
    sorted_precs = np.sort(precs)
    sorted_args = np.argsort(precs)
    starts = cut_positions(k)
    M = train_clusters.size(0)
    stats, gt_fg = ops.cbfe_cluster_stats(_dev_long(train_clusters).view(M, -1), None, _dev_long(train_gt).view(M, -1), int(k))
    dev = stats.device
    jac = ops.cbfe_cut_jaccard(stats, gt_fg, torch.from_numpy(sorted_args.astype(np.int32)).to(dev),
                               torch.tensor(starts, dtype=torch.int32, device=dev)).cpu()
    jacs = [(sorted_precs[s], s, float(jac[i])) for i, s in enumerate(starts)]
    return sorted(jacs, key=lambda x: x[2])


def threshold_from_cuts(res):
    """:216: the precision of the best cut rounded to the nearest multiple of 0.05 below 1."""
    return min(np.arange(0, 1, 0.05), key=lambda x: abs(x - res[-1][0]))


def foreground_ids(cluster_precs, threshold):
    """:222-223: the clusters from the first sorted precision >= threshold on, in ``np.argsort`` order."""
    start_idx = np.where((np.sort(cluster_precs) >= threshold) == True)[0][0]   # noqa: E712  (the reference's expression)
    return np.argsort(cluster_precs)[start_idx:]


class UpsampledFeatures(NamedTuple):
    """The nearest upsampling of tokens [bs, fs, g*g, dim] to resolution x resolution, not materialised:
    ``create_overclustering_maps`` clusters it through ``Kmeans.train_upsampled``."""
    tokens: torch.Tensor
    resolution: int


class ClusterBasedForegroundExtraction(nn.Module):
    """:156-279.  ``model`` is a FeatureExtractor (or holds one as ``feature_extractor``) built with ``return_attention=True``."""

    with_bf_score = False   # bf_score=True: evaluate_bf_score before the Jaccard score (:193), its result in bf_score
    bf_score = None

    def __init__(self, model, k_fg_extraction, eval_resolution=100, eval_feature_dim=50, train_loader=None, val_loader=None, device="cuda",
                 *, bf_score=False):
        super().__init__()
        self.with_bf_score = bf_score
        self.model = model
        self.k_fg_extraction = k_fg_extraction
        self.eval_resolution = eval_resolution
        fe = model if isinstance(model, FeatureExtractor) or not hasattr(model, "feature_extractor") else model.feature_extractor
        self.feature_extractor = fe
        self.spatial_resolution = fe.spatial_resolution
        self.train_loader = train_loader
        self.val_loader = val_loader
        self.device = device
        self.eval_feature_dim = eval_feature_dim

    def get_foreground_masks(self, set="val"):
        """:172-196 -> (foreground masks int64 [N, R, R] on the device, annotations [N, 1, R, R], the set's upsampled features
        [bs, fs, dim, R, R] on the host).  Device memory beyond the extracted features: the normalised tokens of one set, the three
        int64 [N, R*R] maps of the threshold search and the k-means training subsample (k * 256 points); the train set's upsampled
        features ([N, dim, R, R]) are never built, and the PCA tokens wait on the host while k-means trains."""
        train_features, train_attentions, train_annotations = self.extract_dataset_features_attentions(self.train_loader)
        val_features, val_attentions, val_annotations = self.extract_dataset_features_attentions(self.val_loader)
        R = self.eval_resolution
        # the PCA tokens are kept on the host, as the reference keeps its features; k-means moves what it needs
        train_tokens = normalize_features(train_features, self.eval_feature_dim).cpu()
        del train_features
        train_cluster_maps = self.create_overclustering_maps(UpsampledFeatures(train_tokens, R))
        if set == "val":
            del train_tokens
        threshold = self.get_tuned_threshold(train_attentions, train_annotations, train_cluster_maps)
        del train_cluster_maps
        set_tokens = normalize_features(val_features, self.eval_feature_dim).cpu() if set == "val" else train_tokens
        del val_features
        set_annotations = val_annotations if set == "val" else train_annotations
        set_attentions = val_attentions if set == "val" else train_attentions
        set_annotations = F.interpolate(set_annotations.float(), size=(R, R), mode="nearest").long()
        set_attentions = F.interpolate(set_attentions.float(), size=(R, R), mode="nearest").long()
        attn_mask_soft = self.create_soft_masks(set_attentions, set_annotations, UpsampledFeatures(set_tokens, R), threshold)
        resized_set_features = self.interpolate(set_tokens, R)
        if self.with_bf_score:
            self.bf_score = evaluate_bf_score(attn_mask_soft, set_annotations.flatten(0, 1))
        score = eval_jac(set_annotations.flatten(0, 1), attn_mask_soft, with_boundary=True)
        print(f"Jaccard score is {score}")
        return attn_mask_soft, set_annotations, resized_set_features

    def create_soft_masks(self, val_attentions, val_annotations, resized_val_features, threshold):
        """:198-206: over-cluster the set, score its clusters against its attention, keep those at or above ``threshold``."""
        val_cluster_maps = self.create_overclustering_maps(resized_val_features)
        val_attentions = val_attentions.flatten(0, 1)
        val_cluster_maps = val_cluster_maps.flatten(0, 1).to(self.device)
        val_cluster_precs = get_cluster_precs(val_cluster_maps, val_attentions, self.k_fg_extraction)
        return self.make_post_matching_maps(val_cluster_maps, threshold, val_cluster_precs)

    def get_tuned_threshold(self, attentions, annotations, cluster_maps):
        """:208-218: the precision cut with the best train Jaccard, rounded to a multiple of 0.05."""
        R = self.eval_resolution
        annotations = F.interpolate(annotations.float(), size=(R, R), mode="nearest").long().flatten(0, 1)
        attentions = F.interpolate(attentions.float(), size=(R, R), mode="nearest").long().flatten(0, 1)
        cluster_maps = cluster_maps.flatten(0, 1).to(self.device)
        cluster_precs = get_cluster_precs(cluster_maps, attentions, self.k_fg_extraction)
        res = find_good_threshold(cluster_maps, annotations, cluster_precs, self.k_fg_extraction)
        threshold = threshold_from_cuts(res)
        print(f"Found threshold {threshold}")
        return threshold

    def make_post_matching_maps(self, cluster_maps, threshold, cluster_precs):
        """:221-227: 1 where the pixel's cluster is foreground (``foreground_ids``), int64 like ``cluster_maps``."""
        table = np.zeros(len(cluster_precs), np.uint8)
        table[foreground_ids(cluster_precs, threshold)] = 1
        maps = _dev_long(cluster_maps)
        return ops.cbfe_apply_fg(maps, torch.from_numpy(table).to(maps.device))

    def interpolate(self, features, target_resolution=100, mode="nearest"):
        """:229-235: features [bs, fs, g*g, dim] -> [bs, fs, dim, R, R], the nearest upsampling (a gather through torch's own index
        tables: the same values as F.interpolate), on the features' device."""
        if mode != "nearest":
            raise NotImplementedError("only the nearest upsampling of the reference's calls is built")
        bs, fs, n, dim = features.shape
        g = int(round(n ** 0.5))
        R = int(target_resolution)
        iy, ix = nearest_index_table(g, R)
        idx = torch.from_numpy((iy.astype(np.int64)[:, None] * g + ix.astype(np.int64)[None, :]).reshape(-1)).to(features.device)
        out = features.reshape(bs * fs, n, dim)[:, idx, :].permute(0, 2, 1).contiguous()
        return out.view(bs, fs, dim, R, R)

    @torch.no_grad()
    def extract_dataset_features_attentions(self, data_loader):
        """:237-265 -> (features [bs, fs, g*g, dim] on the host, attention foreground [N, 1, g, g] fp32 and annotations [bs, 1, H, W]
        int64 on the device)."""
        feature_group, attention_group, annotation_group = [], [], []
        for batch in data_loader:
            data, annotations = process_data_group(batch, ScaleType.ZERO_TO_255)
            bs, fs, c, h, w = data.shape
            features, attentions = self.feature_extractor(data.flatten(0, 1).to(self.device), use_head=False)
            if attentions is None:
                raise ValueError("ClusterBasedForegroundExtraction needs the attention probabilities: build the FeatureExtractor with "
                                 "return_attention=True")
            _, num_patches, dim = features.shape
            g = int(round(num_patches ** 0.5))
            feature_group.append(features.view(bs, fs, num_patches, dim).cpu())
            attention_group.append(process_attentions(attentions, g, threshold=ATTENTION_THRESHOLD))
            annotation_group.append(annotations.to(self.device))
        return torch.cat(feature_group, dim=0), torch.cat(attention_group, dim=0), torch.cat(annotation_group, dim=0)

    def create_overclustering_maps(self, features):
        """:268-279: k-means (niter 50, nredo 5, seed 1, ``clustering.Kmeans``) over every pixel of the upsampled features ->
        cluster maps int64 [bs, fs, R, R] on the device.  ``features``: materialised [bs, fs, dim, R, R], or ``UpsampledFeatures``
        (same labels, without the points)."""
        k = self.k_fg_extraction
        if isinstance(features, UpsampledFeatures):
            tokens, R = features.tokens, int(features.resolution)
            bs, fs, n, dim = tokens.shape
            tokens = tokens.reshape(bs * fs, n, dim)
            km = Kmeans(dim, k, niter=50, nredo=5, seed=1, loop="device" if clustering.DEVICE_LOOP else "host",
                        loop_workspace_bytes=LOOP_WORKSPACE_BYTES)
            km.train_upsampled(tokens, R)
            return km.assign_upsampled(tokens, R).view(bs, fs, R, R)
        bs, fs, dim, R, _ = features.shape
        points = features.permute(0, 1, 3, 4, 2).reshape(-1, dim)
        km = Kmeans(dim, k, niter=50, nredo=5, seed=1, loop="device" if clustering.DEVICE_LOOP else "host",
                        loop_workspace_bytes=LOOP_WORKSPACE_BYTES)
        km.train(points)
        return km.assign(points)[1].view(bs, fs, R, R)


# ---- synthetic inputs (fixtures, benchmark, the driver) ---------------------------------------------------------------------------

def synthetic_cluster_maps(M: int, R: int, k: int, seed: int, cell: int = 10):
    """Cluster maps, attention masks and VOC-style labels, int64 [M, R, R] each, with every id in [0, k) present.  Labels come from
    ``linear_finetune.synthetic_segmentation`` (discs, 255 borders).  Pixels are clustered in cell x cell blocks: blocks whose centre
    is foreground draw ids from the first 40% of [0, k), the others from the rest.  Ids below 0.3 k have attention 1 everywhere
    (precision exactly 1.0), ids from 0.8 k on attention 0 everywhere (exactly 0.0); the rest follow the GT foreground with 15% noise."""
    from . import synth
    from .linear_finetune import synthetic_segmentation

    _, y01 = synthetic_segmentation(M, R, 21, seed=seed)
    gt = (y01[:, 0] * 255).round().long()
    n_fg = max(int(0.4 * k), 1)
    perm_fg = np.argsort(synth.normal("cbfe.perm.fg", (n_fg,), 1.0, 0.0, seed), kind="stable")
    perm_bg = n_fg + np.argsort(synth.normal("cbfe.perm.bg", (k - n_fg,), 1.0, 0.0, seed), kind="stable")
    clusters = np.zeros((M, R, R), np.int64)
    nc = (R + cell - 1) // cell
    i_fg = i_bg = 0
    for m in range(M):
        for by in range(nc):
            for bx in range(nc):
                cy, cx = min(by * cell + cell // 2, R - 1), min(bx * cell + cell // 2, R - 1)
                if int(gt[m, cy, cx]) != 0:
                    cid, i_fg = perm_fg[i_fg % n_fg], i_fg + 1
                else:
                    cid, i_bg = perm_bg[i_bg % (k - n_fg)], i_bg + 1
                clusters[m, by * cell:(by + 1) * cell, bx * cell:(bx + 1) * cell] = cid
    noise = synth.normal("cbfe.attn.noise", (M, R, R), 1.0, 0.0, seed) < -1.0364   # ~15%
    gfg = (gt != 0).numpy()
    attn = np.where(noise, ~gfg, gfg).astype(np.int64)
    attn[clusters < int(0.3 * k)] = 1
    attn[clusters >= int(0.8 * k)] = 0
    return torch.from_numpy(clusters), torch.from_numpy(attn), gt


# ---- the driver (:281-373) --------------------------------------------------------------------------------------------------------

def build_parser() -> argparse.ArgumentParser:
    """The reference's flags with its defaults (:352-371).  ``--dataset synthetic`` and ``--num_*_images`` are additions, and
    so is ``--dataset voc``: ``leoloader.pascal_loader`` on ``--dataset_path`` (the VOCSegmentation root), as :340-341 call it."""
    p = argparse.ArgumentParser()
    p.add_argument("--architecture", type=str, default="dino-s16", help="which back-bone architecture do you want to use?")
    p.add_argument("--model_path", type=str, default="/home/ssalehi/video/dino/outputs/checkpoint0080.pth")
    p.add_argument("--dataset", type=str, default="davis")
    p.add_argument("--dataset_path", type=str, default="../data")
    add_decode_arguments(p, jpeg=False)
    p.add_argument("--destination_path", type=str, default="ytvos")
    p.add_argument("--evaluation_protocol", type=str, default="dataset-wise")
    p.add_argument("--logging_directory", type=str, default="visualizations")
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--num_workers", type=int, default=3)
    p.add_argument("--k_fg_extraction", type=int, default=300)
    p.add_argument("--num_clusters", type=int, default=21)
    p.add_argument("--input_resolution", type=int, default=448)
    p.add_argument("--many_to_one", type=bool, default=False)
    p.add_argument("--num_frames", type=int, default=4)
    p.add_argument("--precision_based", type=bool, default=False)
    p.add_argument("--uvos", type=int, default=False)
    p.add_argument("--use_teacher", type=bool, default=False)
    p.add_argument("--EMA_decay", type=float, default=0.999)
    p.add_argument("--num_train_images", type=int, default=64, help="synthetic data only")
    p.add_argument("--num_val_images", type=int, default=32, help="synthetic data only")
    p.add_argument("--bf_score", action="store_true", help="also print the boundary F-score of the val masks (evaluate_bf_score)")
    return p


def _batches(x, y, batch_size):
    return [(x[i:i + batch_size], y[i:i + batch_size]) for i in range(0, x.shape[0], batch_size)]


def main(args=None) -> float:
    """:281-348 on synthetic data: CBFE foreground masks of the val set, then the masked dataset-wise Evaluator (21 clusters).
    ``args``: an argparse namespace or an argument list.  The reference also loads a fixed TimeT checkpoint; here the backbone
    comes from ``--model_path`` ('' = synthetic weights).  Returns the Evaluator's score."""
    from .evaluation import Evaluator
    from .linear_finetune import synthetic_segmentation
    from .time_tuning import TimeT

    if args is None or isinstance(args, (list, tuple)):
        args = build_parser().parse_args(args)
    if args.dataset not in ("synthetic", "voc"):
        raise NotImplementedError("this build reads Pascal VOC through --dataset voc (leoloader.pascal_loader on --dataset_path, the "
                                  "VOCSegmentation root) and generated data through --dataset synthetic")
    eval_resolution = 100 if args.evaluation_protocol == "dataset-wise" else args.input_resolution
    if args.dataset == "voc":                                                            # :340-341
        from .leoloader import pascal_loader

        train_loader = pascal_loader(args.batch_size, args.dataset_path, "trainaug", eval_resolution, train_size=args.input_resolution, png=args.png_decode)
        val_loader = pascal_loader(args.batch_size, args.dataset_path, "val", eval_resolution, train_size=args.input_resolution, png=args.png_decode)
        eval_batches = val_loader
    else:
        x_tr, y_tr = synthetic_segmentation(args.num_train_images, args.input_resolution, 21, seed=1)
        x_va, y_va = synthetic_segmentation(args.num_val_images, args.input_resolution, 21, seed=2)
        train_loader = _batches(x_tr, y_tr, args.batch_size)
        val_loader = _batches(x_va, y_va.clone(), args.batch_size)
        eval_batches = _batches(x_va, y_va, args.batch_size)
    torch.cuda.set_device(0)
    feature_extractor = FeatureExtractor(args.architecture, args.model_path, [1024, 1024, 512, 256], return_attention=True)
    model = TimeT(feature_extractor, 200).cuda()
    cbfe = ClusterBasedForegroundExtraction(model, args.k_fg_extraction, eval_resolution, 50, train_loader, val_loader,
                                            bf_score=args.bf_score)
    set_soft_masks, set_annotations, _ = cbfe.get_foreground_masks("val")
    # the Evaluator reads integer labels: the val annotations as process_data_group made them
    eval_loader = [(x[:, None], (y * 255).long()) for x, y in eval_batches]
    evaluator = Evaluator(model, eval_loader, num_prototypes=21, fg_masks=set_soft_masks)
    score = evaluator.evaluate(many_to_one=args.many_to_one, evaluation_protocol=args.evaluation_protocol, eval_resolution=eval_resolution,
                               num_clusters=21, use_annotations=False, use_mask=True, precision_based=args.precision_based)
    print(f"Dataset score is {score}")
    return score


if __name__ == "__main__":
    main()
