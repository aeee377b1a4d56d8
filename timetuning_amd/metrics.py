"""``PredsmIoU`` with the reference's surface (``metrics.py:209-505``): matched mean IoU between predicted cluster maps and
ground-truth label maps, Hungarian or many-to-one matching.

The reference concatenates every prediction / ground-truth pixel on the host and re-scans the two arrays once per
(ground-truth class, predicted class) pair (``compute_score_matrix``, joblib-parallel).  Every quantity it derives - the
score matrix, the matching, tp / fp / fn after remapping - is a function of the confusion matrix alone, so here one GPU
pass (``tt_confusion_counts``) builds that matrix and the rest is exact integer bookkeeping on a few hundred numbers.

``compute_segments`` scores MANY independent (gt, pred) pairs - the frames or clips of one ``evaluate_localizations`` call - from one
launch (``tt_confusion_counts_segments``), matches and scores them in a second one (``tt_match_segments``) and reads the results back
once; ``compute_propagation_score`` (``metrics.py:271-346``) reads the per-frame true / false positives and false negatives of every
object off the same per-frame matrices.
"""
from __future__ import annotations

from collections import defaultdict
from typing import Dict, List

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from . import hip_ops as ops

# ``compute_segments`` matches and scores on the device (``hip_ops.match_segments``, N20) where the counts are in GPU memory and the shape
# is inside ``match_segments_shape_ok``; everywhere else, and with the switch off, the host loop over ``compute_miou_from_confusion`` runs.
# The two routes return equal objects, so the switch does not show in any score.  On: every protocol of
# tools/bench_eval_scoring.py was faster than the host loop in both rounds, one-segment calls included (profiles/n20_match_segments.txt).
DEVICE_MATCH = True


class PredsmIoU(torch.nn.Module):
    def __init__(self, num_pred_classes: int, num_gt_classes: int, involve_bg: bool = False):
        super().__init__()
        self.num_pred_classes = num_pred_classes
        self.num_gt_classes = num_gt_classes
        self.gt: List[torch.Tensor] = []
        self.pred: List[torch.Tensor] = []
        self.involve_bg = involve_bg

    def update(self, gt: torch.Tensor, pred: torch.Tensor) -> None:
        self.gt.append(gt.reshape(-1))
        self.pred.append(pred.reshape(-1))

    def reset(self) -> None:
        self.gt, self.pred = [], []

    # -- confusion matrix over the VALUES that occur (the reference re-derives the class sets from the data, :262-263)
    def _confusion(self):
        pred = torch.cat(self.pred).long().cuda().contiguous()
        gt = torch.cat(self.gt).long().cuda().contiguous()
        C = int(max(pred.max().item(), gt.max().item())) + 1
        counts = ops.confusion_counts(pred, gt, C).cpu().numpy().astype(np.int64)   # [gt value, pred value]
        gt_unique = np.nonzero(counts.sum(1))[0]
        pred_unique = np.nonzero(counts.sum(0))[0]
        return pred, counts[np.ix_(gt_unique, pred_unique)], gt_unique, pred_unique

    def compute(self, is_global_zero: bool, many_to_one: bool = False, precision_based: bool = False, linear_probe: bool = False):
        if not is_global_zero:
            return None
        pred, conf, gt_unique, pred_unique = self._confusion()
        self.num_pred_classes, self.num_gt_classes = len(pred_unique), len(gt_unique)
        return self.compute_miou_from_confusion(conf, gt_unique, pred_unique, pred, many_to_one, precision_based, linear_probe)

    def compute_segments(self, gt: torch.Tensor, pred: torch.Tensor, many_to_one: bool = False, precision_based: bool = False,
                         ignore_gt=None, *, with_mapping: bool = False) -> list:
        """``compute`` of S independent segments at once: gt, pred [S, n] -> a list of S ``compute`` tuples (score, tp, fp, fn, None,
        matched background share), WITHOUT the reordered map; ``with_mapping=True`` puts the host int64 table ``pred value -> matched gt
        value`` (unmapped values 0, as long as the segment's largest predicted value + 1) in slot 4 instead of None: ``table[pred]`` IS the
        reordered map, and a renderer takes the table (``visualization.label_panels``).  ``ignore_gt``: elements whose ground truth has
        this value are left out (Pascal VOC's 255).  One read-back of the two maxima sizes the matrices (any upper bound gives the same scores: the class sets are
        the non-empty rows and columns, as in ``_confusion``), one ``confusion_counts_segments`` call counts, one ``match_segments`` call
        matches and scores every matrix on the device and one ``.cpu()`` brings its outputs to the host (``DEVICE_MATCH``; with counts in
        host memory, a shape beyond ``match_segments_shape_ok`` or the switch off, one ``.cpu()`` brings every matrix to the host and
        ``compute_miou_from_confusion`` runs per segment - the same objects either way); what was stored with ``update`` is neither used
        nor changed."""
        gt = gt.long().cuda().contiguous()
        pred = (pred if pred.dtype in (torch.int16, torch.int64) else pred.long()).cuda().contiguous()
        if gt.dim() != 2 or gt.shape != pred.shape:
            raise ValueError(f"compute_segments: expected gt and pred of one shape [S, n], got {tuple(gt.shape)} and {tuple(pred.shape)}")
        counted_gt = gt if ignore_gt is None else torch.where(gt == ignore_gt, -1, gt)
        gt_max, pred_max = torch.stack([counted_gt.max(), pred.max().long()]).tolist()
        counts = ops.confusion_counts_segments(pred, gt, max(gt_max, 0) + 1, max(pred_max, 0) + 1, ignore_gt)
        _, Cg, Cp = counts.shape
        if DEVICE_MATCH and counts.is_cuda and ops.match_segments_shape_ok(Cg, Cp):
            return self._segments_on_device(counts, many_to_one, precision_based, with_mapping)
        return [self._segment_on_host(s, full, many_to_one, precision_based, with_mapping) for s, full in enumerate(counts.cpu().numpy())]

    def _segment_on_host(self, s, full, many_to_one, precision_based, with_mapping):
        """One segment of ``compute_segments`` from its matrix ``full[gt value, pred value]`` on the host."""
        gt_unique = np.nonzero(full.sum(1))[0]
        pred_unique = np.nonzero(full.sum(0))[0]
        if len(gt_unique) == 0:
            raise ValueError(f"compute_segments: segment {s} has no element to score")
        self.num_pred_classes, self.num_gt_classes = len(pred_unique), len(gt_unique)
        return self.compute_miou_from_confusion(full[np.ix_(gt_unique, pred_unique)], gt_unique, pred_unique, None, many_to_one, precision_based,
                                                with_mapping=with_mapping)

    def _segments_on_device(self, counts, many_to_one, precision_based, with_mapping):
        """``compute_segments`` behind the counts: one ``match_segments`` launch and one read-back of its packed outputs; the host only
        builds the dicts.  A segment the kernel flags (status 2 or 3) is scored by the host path - the counts are read back for that alone."""
        m = ops.match_segments(counts, "many_to_one" if many_to_one else "hungarian", precision_based, self.involve_bg).cpu()
        score, bg, info = m.score.tolist(), m.matched_bg.tolist(), m.info.tolist()
        tp_all, fp_all, fn_all = m.tp.tolist(), m.fp.tolist(), m.fn.tolist()
        host_counts = None
        results = []
        for s, (status, n_gt, n_pred, pred_max) in enumerate(info):
            if status == 1:
                raise ValueError(f"compute_segments: segment {s} has no element to score")
            if status != 0:
                if host_counts is None:
                    host_counts = counts.cpu().numpy()
                results.append(self._segment_on_host(s, host_counts[s], many_to_one, precision_based, with_mapping))
                continue
            self.num_pred_classes, self.num_gt_classes = n_pred, n_gt
            tp_s, fp_s, fn_s = tp_all[s], fp_all[s], fn_all[s]
            present = [g for g in range(len(tp_s)) if tp_s[g] + fn_s[g] > 0]                # a present gt value has a non-empty row
            table = m.lut[s, :pred_max + 1].clone() if with_mapping else None
            results.append((score[s], {g: tp_s[g] for g in present}, {g: fp_s[g] for g in present}, {g: fn_s[g] for g in present}, table, bg[s]))
        return results

    def compute_propagation_score(self, is_global_zero: bool):
        """``metrics.py:271-296``: the per-object scores of ONE clip whose frames were stored with ``update``, one per call and all of
        one size (the reference stacks them)."""
        if not is_global_zero:
            return None
        return self.compute_propagation_iou(torch.stack(self.gt), torch.stack(self.pred))

    def compute_propagation_iou(self, gt, pred) -> List[float]:
        """``metrics.py:297-346`` on gt, pred [frames, ...]: no matching - for every non-zero value v of gt, in ascending order, tp, fp
        and fn of (gt == v) against (pred == v) ACCUMULATE over the frames, every frame adds the Jaccard index of the sums so far, and the
        total is divided by the number of frames whose gt holds v.  Per frame, tp is the diagonal cell of that frame's confusion matrix,
        tp + fn its row sum and tp + fp its column sum: one segmented call, one read-back.  Labels must be non-negative (the kernel skips
        negative ones, which the reference would count among the false positives and negatives)."""
        gt, pred = torch.as_tensor(gt), torch.as_tensor(pred)
        if gt.shape != pred.shape or gt.dim() < 1:
            raise ValueError(f"compute_propagation_iou: gt {tuple(gt.shape)} and pred {tuple(pred.shape)} need one shape [frames, ...]")
        frames = gt.shape[0]
        gt = gt.reshape(frames, -1).long().cuda().contiguous()
        pred = pred.reshape(frames, -1)
        pred = (pred if pred.dtype in (torch.int16, torch.int64) else pred.long()).cuda().contiguous()
        gt_max, pred_max, gt_min, pred_min = torch.stack([gt.max(), pred.max().long(), gt.min(), pred.min().long()]).tolist()
        if min(gt_min, pred_min) < 0:
            raise ValueError(f"compute_propagation_iou: negative labels (gt from {gt_min}, pred from {pred_min})")
        C = max(gt_max, pred_max) + 1
        counts = ops.confusion_counts_segments(pred, gt, C, C).cpu().numpy()             # [frame, gt value, pred value]
        in_gt, in_pred = counts.sum(2), counts.sum(1)                                   # [frame, value]
        self.num_pred_classes, self.num_gt_classes = int((in_pred.sum(0) > 0).sum()), int((in_gt.sum(0) > 0).sum())
        jac = []
        for v in np.nonzero(in_gt.sum(0))[0]:
            if v == 0:
                continue
            tp = fp = fn = 0
            score = 0
            for f in range(frames):
                tp += int(counts[f, v, v])
                fp += int(in_pred[f, v] - counts[f, v, v])
                fn += int(in_gt[f, v] - counts[f, v, v])
                score += float(tp) / max(float(tp + fp + fn), 1e-8)
            jac.append(score / int((in_gt[:, v] > 0).sum()))
        return jac

    @staticmethod
    def score_matrix(conf: np.ndarray, precision_based: bool = False) -> np.ndarray:
        """[num_gt, num_pred]: IoU (or precision) if ground-truth class i were matched to predicted class j (:435-474)."""
        tp = conf.astype(np.float64)
        fp = conf.sum(0, keepdims=True) - tp
        if precision_based:
            return tp / np.maximum(tp + fp, 1e-8)
        fn = conf.sum(1, keepdims=True) - tp
        return tp / np.maximum(tp + fp + fn, 1e-8)

    def compute_miou_from_confusion(self, conf, gt_unique, pred_unique, pred=None, many_to_one=False, precision_based=False,
                                    linear_probe=False, with_mapping=False):
        """``compute_miou`` (:357-432) on the confusion matrix ``conf[gt index, pred index]``.  ``with_mapping`` (without ``pred``): slot 4
        is the table the reordered map is read through, int64 ``lut[pred value] = matched gt value`` (unmapped values 0)."""
        num_gt, num_pred = conf.shape
        mapping: Dict[int, int] = {}          # predicted VALUE -> ground-truth VALUE; unmapped predictions count as 0
        if linear_probe:
            mapping = {int(p): int(p) for p in pred_unique}
            matched_bg_clusters = {}
        elif many_to_one:
            match = self._original_match(conf, precision_based)
            for target_i, matched_preds in match.items():
                for pred_i in matched_preds:
                    mapping[int(pred_unique[pred_i])] = int(gt_unique[target_i])
            matched_bg_clusters = len(match[0]) / num_pred
        else:
            rows, cols = linear_sum_assignment(1 - self.score_matrix(conf))
            for target_i, pred_i in zip(rows, cols):
                mapping[int(pred_unique[pred_i])] = int(gt_unique[target_i])
            matched_bg_clusters = 1 / num_gt
        # confusion after remapping: remapped[gt index][target VALUE]
        tp, fp, fn, jac = {}, {}, {}, {}
        col_target = np.array([mapping.get(int(p), 0) for p in pred_unique])
        for gi, g in enumerate(gt_unique):
            sel = col_target == g
            tp_g = int(conf[gi, sel].sum())
            fp_g = int(conf[:, sel].sum()) - tp_g
            fn_g = int(conf[gi].sum()) - tp_g
            tp[int(g)], fp[int(g)], fn[int(g)] = tp_g, fp_g, fn_g
            jac[int(g)] = float(tp_g) / max(float(tp_g + fp_g + fn_g), 1e-8)
        if not self.involve_bg:
            jac.pop(0, None)
            if len(jac) == 0:  # the found cluster is solely background (:426-427)
                jac[0] = 0
        reordered = None
        if pred is not None or with_mapping:
            lut = torch.zeros(int(pred_unique.max()) + 1, dtype=torch.int64)
            for p, g in mapping.items():
                lut[p] = g
            reordered = lut if pred is None else lut.to(pred.device)[pred]
        return float(np.mean(np.array(list(jac.values())))), tp, fp, fn, reordered, matched_bg_clusters

    def _original_match(self, conf, precision_based=False) -> Dict[int, list]:
        """Greedy many-to-one: every predicted class goes to the ground-truth class with the best score (:489-505)."""
        score_mat = self.score_matrix(conf, precision_based)
        gt_to_matches = defaultdict(list)
        for pred_c in range(conf.shape[1]):
            gt_to_matches[int(np.argmax(score_mat[:, pred_c]))].append(pred_c)   # first maximum, as the `>` scan
        return gt_to_matches
