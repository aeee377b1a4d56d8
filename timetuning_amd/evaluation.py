"""Evaluator with the reference's surface (``evaluation.py:250-310,312-486``): features without head -> clustering ->
matched mIoU, for the three protocols (frame-wise / sample-wise / dataset-wise), with the GIF logs of the matched maps
(``evaluation.py:255-300``) on ``visualization``'s render launch.  The wandb plumbing is out of scope; the loader is any iterable of
``(data, annotations[, label])`` batches - ``main`` builds it from a video tree (``data_loader.make_loader``, with the YouTube-VOS category
mapping where the tree has a ``meta.json``), from Pascal VOC or from synthetic clips.
``evaluate_localizations`` scores a whole batch from one segmented confusion-count launch (``PredsmIoU.compute_segments``);
``evaluate_propagation`` is the reference's (``evaluation.py:228-246``).

``use_mask=True`` evaluates masked features as the reference does (``evaluation.py:411-424,461-462``): with ``fg_masks`` given to the
constructor (the foreground masks of cluster_based_foreground_extraction, [N, R', R']) the dataset-wise features are multiplied by
the masks' nearest downsampling to the token grid; otherwise by the attention foreground (``models.apply_attention_mask``).

``build_parser`` / ``main`` are the command line of ``evaluation.py:490-566`` (``python -m timetuning_amd.evaluation``): the reference's
flags and defaults on a synthetic loader.  Any ``--num_clusters`` runs: ``clustering.Kmeans`` takes the tiled k-means kernels beyond what
the LDS-resident ones hold, so the over-clustering protocol (``--num_clusters 500 --many_to_one True``) is one invocation."""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import hip_ops as ops
from .data_loader import add_decode_arguments
from .clustering import cluster_features, nearest_index_table, proto_clustering
from .metrics import PredsmIoU
from .models import FeatureExtractor, apply_attention_mask


def evaluate_propagation(PredsEval, gts, preds):
    """gts / preds [bs, fs, h, w] -> the mean, over every object of every clip, of ``PredsmIoU.compute_propagation_score``
    (``evaluation.py:228-246``).  As in the reference the clip's frames are stored with ``update(preds, gts)`` - the arguments of
    ``update(gt, pred)`` swapped - so the objects the score iterates over are the non-zero values of the PREDICTIONS and a frame "holds"
    an object when its prediction does.  That quirk is kept: the scores are the reference's."""
    bs, fs = preds.shape[:2]
    scores = []
    for i in range(bs):
        PredsEval.reset()
        for j in range(fs):
            PredsEval.update(preds[i, j].flatten(), gts[i, j].flatten())
        scores += PredsEval.compute_propagation_score(is_global_zero=True)
    return np.array(scores).mean()


def evaluate_localizations(PredsEval, gts, preds, evaluation_protocol, logging_directory=None, many_to_one=False, precision_based=False,
                           first_clip=0):
    """gts / preds [bs, fs, R, R] -> mean score (``evaluation.py:250-310``).  Every ``PredsmIoU.compute`` of the reference's loops - one
    per frame (frame-wise), per clip (sample-wise) or for everything but Pascal VOC's ignore label 255 (dataset-wise, :304-305) - is one
    segment of a single ``PredsmIoU.compute_segments`` call: one counting launch and one read-back per protocol call.

    ``logging_directory`` (``evaluation.py:255-300``): frame-wise and sample-wise write two GIFs per clip into
    ``{logging_directory}/{protocol}/`` under the reference's names - "Reordered" shows the predictions through the matching (per frame
    for frame-wise, per clip for sample-wise), "Inorder" as they are - at 80 ms per frame; dataset-wise writes nothing, as in the
    reference.  A frame is ``visualization.label_panels``' ``[ground truth | prediction | both]`` (the reference's matplotlib figure
    is not restated); all frames of the call are rendered by one launch per GIF kind.  The score is the one returned without a
    directory.  ``first_clip`` numbers the clips from there and keeps the GIFs already in the directory (0 clears them, as
    ``my_utils.make_working_directory`` does)."""
    bs, fs = preds.shape[:2]
    if evaluation_protocol == "frame-wise":
        segments, ignore_gt = bs * fs, None
    elif evaluation_protocol == "sample-wise":
        segments, ignore_gt = bs, None
    elif evaluation_protocol == "dataset-wise":
        segments, ignore_gt = 1, 255
    else:
        raise ValueError(f"unknown evaluation protocol {evaluation_protocol!r}")
    log = logging_directory is not None and evaluation_protocol != "dataset-wise"
    results = PredsEval.compute_segments(gts.reshape(segments, -1), preds.reshape(segments, -1), many_to_one, precision_based, ignore_gt,
                                         with_mapping=log)
    PredsEval.reset()
    scores = [r[0] for r in results]
    if log:
        _log_matched_maps(gts, preds, results, evaluation_protocol, logging_directory, first_clip)
    return sum(scores) / len(scores)


def _log_matched_maps(gts, preds, results, evaluation_protocol, logging_directory, first_clip):
    """The GIFs of ``evaluation.py:255-300`` for one scored batch; ``results`` are ``compute_segments(..., with_mapping=True)``'s."""
    from . import visualization as V

    bs, fs, h, w = preds.shape
    sub_directory = logging_directory + "/" + evaluation_protocol
    if first_clip == 0:
        V.make_working_directory(sub_directory)
    else:
        os.makedirs(sub_directory, exist_ok=True)
    per_clip = len(results) // bs                                  # fs segments per clip (frame-wise) or one (sample-wise)
    length = max(int(r[4].numel()) for r in results)
    lut = torch.zeros((len(results), length), dtype=torch.int64)  # rows padded with 0, the value of an unmapped prediction
    for s, r in enumerate(results):
        lut[s, : r[4].numel()] = r[4]
    lut = lut.repeat_interleave(fs // per_clip, dim=0)              # one row per frame
    g, p = gts.reshape(bs * fs, h, w), preds.reshape(bs * fs, h, w)
    reordered = V.grids_to_frames(V.label_panels(g, p, lut))
    inorder = V.grids_to_frames(V.label_panels(g, p))
    sep = ":" if evaluation_protocol == "frame-wise" else "-"      # evaluation.py:277-278 against :299-300
    for i in range(bs):
        clip_score = [r[0] for r in results[i * per_clip:(i + 1) * per_clip]]
        stem = f"Score{sep}{sum(clip_score) / len(clip_score)}_Evaluation_{evaluation_protocol}_"
        V.convert_list_to_video(reordered[i * fs:(i + 1) * fs], f"{stem}Reordered_{first_clip + i}", speed=80, directory=sub_directory + "/")
        V.convert_list_to_video(inorder[i * fs:(i + 1) * fs], f"{stem}Inorder_{first_clip + i}", speed=80, directory=sub_directory + "/")


class Evaluator:
    """``Evaluator(model, data_loader, num_prototypes, device, logger, clustering_algorithm)`` (``evaluation.py:312-371``) reduced
    to what ``evaluate`` needs.  ``fg_masks`` ([N, R', R'] or [N, 1, R', R'], one per frame of the loader in order): the reference's
    foreground masks for ``evaluate(use_mask=True)`` (``evaluation.py:325,340``).  ``logging_directory`` (None = no GIFs) is handed to
    ``evaluate_localizations`` for the frame-wise and sample-wise protocols; the clips are numbered over the WHOLE loader.  The reference
    restarts ``i`` at every batch (``evaluation.py:261,280``) and clears the directory per call (:259), so there only the last batch's
    GIFs survive; here the directory is cleared at the loader's first batch."""

    def __init__(self, model, data_loader, num_prototypes=21, device="cuda", logger=None, clustering_algorithm="k-means", uvos_flag=False,
                 involve_bg=False, fg_masks=None, logging_directory=None):
        self.model, self.data_loader, self.device = model, data_loader, device
        self.logging_directory = logging_directory
        self.clustering_algorithm = clustering_algorithm
        self.uvos_flag = uvos_flag
        self.PredsEval = PredsmIoU(num_prototypes, num_prototypes, involve_bg=involve_bg)
        self.fg_masks = fg_masks

    def _features(self, data, with_attention=False):
        fe = self.model if isinstance(self.model, FeatureExtractor) else self.model.feature_extractor
        bs, fs, c, h, w = data.shape
        feats, attn = fe(data.view(bs * fs, c, h, w).to(self.device), use_head=False)
        feats = feats.view(bs, fs, feats.shape[1], feats.shape[2])
        if with_attention:
            return feats, fe.spatial_resolution, attn
        return feats, fe.spatial_resolution

    def _attention_masked(self, data):
        """features * the attention foreground (evaluation.py:411-413,461-462)."""
        feats, g, attn = self._features(data, with_attention=True)
        if attn is None:
            raise ValueError("evaluate(use_mask=True) without fg_masks needs the attention probabilities: build the FeatureExtractor "
                             "with return_attention=True")
        return apply_attention_mask(feats, attn, g)[0], g

    def _apply_fg_masks(self, features, spatial_resolution):
        """features [bs, fs, g*g, dim] times the nearest downsampling of fg_masks to g x g (evaluation.py:415-424)."""
        bs, fs, n, dim = features.shape
        m = torch.as_tensor(self.fg_masks)
        Rm = m.shape[-1]
        if m.numel() != bs * fs * Rm * Rm:
            raise ValueError(f"fg_masks hold {m.numel() // (Rm * Rm)} masks, the loader {bs * fs} frames")
        iy, ix = nearest_index_table(Rm, spatial_resolution)
        iy, ix = torch.from_numpy(iy.astype("int64")), torch.from_numpy(ix.astype("int64"))
        m = m.reshape(bs * fs, Rm, Rm).to(self.device)
        small = m[:, iy.to(m.device)][:, :, ix.to(m.device)].reshape(bs * fs * n).float().contiguous()
        out = ops.scale_rows_(features.detach().contiguous().float().clone().view(bs * fs * n, dim), small)
        return out.view(bs, fs, n, dim)

    def _cluster(self, features, spatial_resolution, eval_resolution, protocol, num_clusters, annotations):
        if self.clustering_algorithm == "k-means":
            return cluster_features(features, num_clusters, spatial_resolution, eval_resolution, protocol, annotations)
        if self.clustering_algorithm == "prototypes":
            bs, fs, n, dim = features.shape
            maps = proto_clustering(features.view(bs * fs, n, dim), self.model.prototypes, spatial_resolution, output_size=eval_resolution,
                                    num_classes=num_clusters)
            return maps.view(bs, fs, eval_resolution, eval_resolution)
        raise ValueError(f"unknown clustering algorithm {self.clustering_algorithm!r}")

    @torch.no_grad()
    def evaluate(self, many_to_one=False, evaluation_protocol="frame-wise", eval_resolution=None, num_clusters=10, use_mask=False,
                 use_annotations=False, precision_based=False):
        """``evaluation.py:373-480``.  Batches are ``(data [bs,(1,)fs,3,H,W], annotations [bs,(1,)fs,H,W] integer labels[, label])``."""
        self.model.eval()
        if evaluation_protocol == "dataset-wise":
            feats, anns = [], []
            for batch in self.data_loader:
                data, annotations = batch[0], batch[1]
                if data.dim() == 6:
                    data, annotations = data.squeeze(1), annotations.squeeze(1)
                f, g = self._attention_masked(data) if (use_mask and self.fg_masks is None) else self._features(data)
                feats.append(f)
                anns.append(annotations.long())
            features, annotations = torch.cat(feats, dim=0), torch.cat(anns, dim=0)
            if use_mask and self.fg_masks is not None:
                features = self._apply_fg_masks(features, g)
            annotations = F.interpolate(annotations.double(), size=(eval_resolution, eval_resolution), mode="nearest").long().to(self.device)
            maps = self._cluster(features, g, eval_resolution, evaluation_protocol, num_clusters, annotations if use_annotations else None)
            return evaluate_localizations(self.PredsEval, annotations, maps, evaluation_protocol, None, many_to_one, precision_based)
        scores, first_clip = [], 0
        for batch in self.data_loader:
            data, annotations = batch[0].squeeze(1), batch[1].squeeze(1).long()
            features, g = self._attention_masked(data) if use_mask else self._features(data)
            if self.uvos_flag:
                annotations = (annotations > 0).long()
            annotations = F.interpolate(annotations.double(), size=(eval_resolution, eval_resolution), mode="nearest").long().to(self.device)
            maps = self._cluster(features, g, eval_resolution, evaluation_protocol, num_clusters, annotations if use_annotations else None)
            scores.append(evaluate_localizations(self.PredsEval, annotations, maps, evaluation_protocol, self.logging_directory, many_to_one,
                                                 precision_based, first_clip=first_clip))
            first_clip += data.shape[0]
        return sum(scores) / len(scores)


# ------------------------------------------------------------------------------------------------
# command line (evaluation.py:490-566)
# ------------------------------------------------------------------------------------------------

def build_parser() -> argparse.ArgumentParser:
    """Flag names, types and defaults of ``evaluation.py:544-566``.  The ``type=bool`` flags treat ANY non-empty string as True, as in
    the reference (and in ``time_tuning.build_parser``): ``--many_to_one False`` turns many-to-one matching ON.  ``--destination_path``
    is parsed and unused; ``--num_workers`` is the thread count of the loader's host decode.  Any ``--dataset`` but ``synthetic`` / ``voc``
    names a video dataset (``davis_val``, ``ytvos_val``, ...) read from ``--dataset_path`` - the tree ``<dataset_path>/JPEGImages/<video>/*.jpg``
    + ``<dataset_path>/Annotations/<video>/*.png`` - through ``data_loader.make_loader`` with the reference's transforms (``:533``) and
    ``SamplingMode.UNIFORM``; when the name contains ``ytvos`` and ``<dataset_path>/meta.json`` exists, instance ids become category ids
    (``YVOSDataset``), by the reference's chained loop unless ``--plain_category_map`` is given.  Added: ``--dataset synthetic`` and
    ``--eval_clips``; ``--dataset voc`` (``leoloader.pascal_loader`` on ``--dataset_path``, the VOCSegmentation root: the "for Pascal VOC"
    line of ``:537``); an EMPTY ``--model_path`` selects synthetic weights; ``--log_videos`` (off by default: an evaluation
    writes no file unless asked) makes ``--logging_directory`` live - the frame-wise and sample-wise protocols then write the GIFs of the
    matched maps there (``evaluate_localizations``)."""
    p = argparse.ArgumentParser()
    p.add_argument("--architecture", type=str, default="dino-s16", help="which back-bone architecture do you want to use?")
    p.add_argument("--model_path", type=str, default="/home/ssalehi/video/vos_pretrained/cyclic_swav/src/leopart_vits16.ckpt")
    p.add_argument("--dataset", type=str, default="davis_val")
    p.add_argument("--dataset_path", type=str, default="../data")
    p.add_argument("--destination_path", type=str, default="ytvos")
    p.add_argument("--evaluation_protocol", type=str, default="frame-wise")
    p.add_argument("--logging_directory", type=str, default="visualizations")
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--num_workers", type=int, default=3)
    add_decode_arguments(p)
    p.add_argument("--num_clusters", type=int, default=10)
    p.add_argument("--input_resolution", type=int, default=224)
    p.add_argument("--many_to_one", type=bool, default=False)
    p.add_argument("--num_frames", type=int, default=4)
    p.add_argument("--precision_based", type=bool, default=False)
    p.add_argument("--uvos", type=int, default=False)
    p.add_argument("--use_teacher", type=bool, default=False)
    p.add_argument("--EMA_decay", type=float, default=0.999)
    p.add_argument("--eval_clips", type=int, default=8, help="synthetic evaluation set size")
    p.add_argument("--log_videos", action="store_true", help="write the matched-map GIFs into --logging_directory (frame-wise / sample-wise)")
    p.add_argument("--plain_category_map", action="store_true",
                   help="YouTube-VOS meta.json: map every object id straight to its category, not by the reference's chained in-place loop")
    return p


def main(argv=None, vit_cfg=None) -> float:
    """``evaluation.py:490-540``: a FeatureExtractor with the [1024, 1024, 512, 256] head inside ``TimeT(fe, 200)``, optionally with its
    EMA teacher, evaluated by k-means over the headless features; returns (and prints, as the reference) the dataset score.
    ``vit_cfg`` (not a flag) replaces the architecture's transformer sizes - a testing aid, as in ``FeatureExtractor``."""
    from .time_tuning import SyntheticEvalClips, TimeT

    args = build_parser().parse_args(argv)
    video_dataset = args.dataset not in ("synthetic", "voc")
    if video_dataset and not os.path.isdir(os.path.join(args.dataset_path, "JPEGImages")):
        raise NotImplementedError("the video dataset readers are out of scope for this build; run with --dataset voc (Pascal VOC through "
                                  "leoloader.pascal_loader on --dataset_path, the VOCSegmentation root) or --dataset synthetic")
    eval_resolution = 112 if args.evaluation_protocol == "dataset-wise" else args.input_resolution   # :536
    voc_loader = None
    if args.dataset == "voc":                                                          # :537, the "for Pascal VOC" line
        from .leoloader import EvaluatorLoader, pascal_loader

        voc_loader = EvaluatorLoader(pascal_loader(args.batch_size, args.dataset_path, "val", eval_resolution, train_size=args.input_resolution,
                                                       jpeg_entropy=args.jpeg_entropy, png=args.png_decode))
    num_epochs, num_itr = 50, 1000                                                     # :491,513
    device = torch.device("cuda", 0)
    fe = FeatureExtractor(args.architecture, args.model_path, [1024, 1024, 512, 256], vit_cfg=vit_cfg, return_attention=False)  # :520
    model = TimeT(fe, 200)
    if args.use_teacher:
        model.init_momentum_teacher()
        model.set_momentum_teacher_schedular_params(args.EMA_decay, 1.0, num_epochs, num_itr)
    model = model.to(device)
    if video_dataset:                                                                  # :533-535
        from . import data_loader as DL
        from . import video_transformations as VT

        meta = os.path.join(args.dataset_path, "meta.json")
        loader = DL.make_loader(args.dataset_path, args.num_frames, args.batch_size, sampling_mode=DL.SamplingMode.UNIFORM, frame_transform=None,
                                target_transform=None, video_transform=VT.evaluation_transforms(args.input_resolution), shuffle=False,
                                num_workers=args.num_workers, device=device, jpeg_entropy=args.jpeg_entropy, png=args.png_decode,
                                meta_file_directory=meta if "ytvos" in args.dataset and os.path.isfile(meta) else None,
                                sequential_category_map=not args.plain_category_map)
        if not loader.dataset.use_annotations:
            raise FileNotFoundError(f"{args.dataset_path}/Annotations: the evaluation needs annotation maps")
    else:
        loader = voc_loader or SyntheticEvalClips(args.eval_clips, args.num_frames, args.input_resolution, args.batch_size, device)
    logging_directory = None
    if args.log_videos:
        logging_directory = args.logging_directory
        os.makedirs(logging_directory, exist_ok=True)
    evaluator = Evaluator(model, loader, 10, device, clustering_algorithm="k-means", uvos_flag=bool(args.uvos), involve_bg=True,
                          logging_directory=logging_directory)                                                        # :364,539
    score = float(evaluator.evaluate(many_to_one=args.many_to_one, evaluation_protocol=args.evaluation_protocol,
                                     eval_resolution=eval_resolution, num_clusters=args.num_clusters, use_annotations=False,
                                     use_mask=False, precision_based=args.precision_based))
    if video_dataset:
        print(f"Frames decoded on the host (fallback): {loader.fallback_frames}")
    print(f"Dataset score is {score}")
    return score


if __name__ == "__main__":
    main()
