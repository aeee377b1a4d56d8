"""Label propagation with the reference's surface (``mask_propagation.py``) on the HIP kernels.

``propagate_labels`` / ``to_one_hot`` keep the reference signatures (``mask_propagation.py:349-361,448-496``);
``propagate_clip`` is the per-clip body of the evaluation loop (``:821-831``: extractor without head ->
``propagate_labels`` -> bilinear upsampling -> arg-max) and ``jaccard`` scores the propagated masks.  The evaluation
driver reproduces the reference's flag set (``:849-871``, DAVIS protocol defaults ``--n_last_frames 4
--size_mask_neighborhood 12 --topk 5``); ``--dataset synthetic`` / ``synthetic_frames`` run on generated clips, any other name on
the frames under ``--dataset_path`` (data_loader.py).

Labels propagate on the frames' own token grid (H / P, W / P), so rectangular clips run at native size (``--frame_size H W``), and
``--size_mask_neighborhood 0`` is the unrestricted variant (``:422``).  Shapes the square entry accepts (``square_entry_accepts``) go to
``tt_label_propagate_maps`` / ``tt_upsample_argmax`` as before; the rest to ``tt_label_propagate_grid_maps`` / ``tt_upsample_argmax_hw``.

The DAVIS metrics (``:501-715``) keep the reference's names, signatures and return types: ``db_eval_iou`` (J),
``db_eval_boundary`` / ``f_measure`` / ``_seg2bmap`` (F), ``db_statistics`` and ``evaluate_semisupervised``; ``davis_jf``
scores every object of label maps in one launch.  The counts come from ``tt_davis_jf_counts`` on the GPU; J and F are formed
from them on the host with the reference's fp64 expressions and branches, so they are the reference's to the bit.

The optical-flow baseline (``--use_optical_flow``, ``:803-815``) keeps the reference's ``dense_optical_flow`` / ``interpolate_frames`` /
``propagate`` (``:265-346``): OpenCV's dense Farneback flow and nearest-neighbour remap on the HIP kernels of farneback.hip, with
``calc_optical_flow_farneback`` in place of the cv2 call.  Parity with cv2 itself is unpinned (cv2 is not a dependency); the kernels are
held to an fp64 restatement of OpenCV's algorithm in the tests.
"""
from __future__ import annotations

import argparse
import os
import sys
import warnings
from typing import List, Optional, Tuple

import numpy as np

import torch
import torch.nn.functional as F

from . import hip_ops as ops
from .data_loader import add_decode_arguments


def to_one_hot(y_tensor: torch.Tensor, n_dims: Optional[int] = None) -> torch.Tensor:
    """Integer map [1,h,w] -> one-hot [n_dims,h,w] float (``mask_propagation.py:349-361``)."""
    if n_dims is None:
        n_dims = int(y_tensor.max() + 1)
    _, h, w = y_tensor.size()
    idx = y_tensor.long().reshape(-1, 1)
    one_hot = torch.zeros(idx.shape[0], n_dims, device=y_tensor.device).scatter_(1, idx, 1)
    return one_hot.view(h, w, n_dims).permute(2, 0, 1)


# the existing square entry's limits (label_prop.hip lp_run): context frames 1 + min(fs - 2, n_last_frames), window side min(2r + 1, g),
# at most 256 * LP_CAND_MAX candidates per query
_SQUARE_CAND_MAX = 4096


def square_entry_accepts(grid, fs: int, n_last_frames: int, radius: int) -> bool:
    """The routing rule: True where ``tt_label_propagate_maps`` (the square entry) takes the shape - a square grid, radius >= 1 and at most
    4 096 candidates per query - so every result it gave before stays bit for bit the same; elsewhere ``tt_label_propagate_grid_maps``."""
    gh, gw = (int(v) for v in grid)
    if gh != gw or radius < 1 or n_last_frames < 0:
        return False
    win = min(2 * radius + 1, gh)
    return win * win * max(1, 1 + min(fs - 2, n_last_frames)) <= _SQUARE_CAND_MAX


def _pair(v) -> Tuple[int, int]:
    return (int(v), int(v)) if isinstance(v, (int, np.integer)) else tuple(int(x) for x in v)


def _maps(n_last_frames, size_mask_neighborhood, topk, model, frame_list, first_seg, features_exist, grid=None):
    fe = model.feature_extractor if hasattr(model, "feature_extractor") else model
    if not features_exist:
        P = fe.backbone.patch_embed.patch_size
        grid = (frame_list.shape[-2] // P, frame_list.shape[-1] // P)   # the token grid of the frames themselves
        frame_list, _ = fe(frame_list, use_head=False)
    elif grid is None:
        grid = (fe.spatial_resolution, fe.spatial_resolution)
    gh, gw = _pair(grid)
    fs, n, D = frame_list.shape
    if gh * gw != n:
        raise ValueError(f"propagate_labels: grid {gh}x{gw} does not hold the {n} tokens of a frame")
    # the seed is resized to the token grid with nearest-neighbour sampling, in fp64 as the reference (:456)
    first_seg = F.interpolate(first_seg.double(), size=(gh, gw), mode="nearest")
    C = first_seg.shape[1]
    xn = ops.l2norm_fwd(frame_list.reshape(fs * n, D).contiguous().float()).view(fs, 1, n, D)
    seed = first_seg.reshape(C, n).t().contiguous().float().view(1, n, C).to(xn.device)
    if square_entry_accepts((gh, gw), fs, n_last_frames, size_mask_neighborhood):
        maps = ops.label_propagate_maps(xn, seed, n_last_frames, size_mask_neighborhood, topk, 0.1)
    else:
        maps = ops.label_propagate_grid_maps(xn, seed, (gh, gw), n_last_frames, size_mask_neighborhood, topk, 0.1)
    return maps, C, (gh, gw)  # [fs-1, 1, n, C]


@torch.no_grad()
def propagate_labels(n_last_frames, size_mask_neighborhood, topk, model, frame_list, first_seg, features_exist=False, *,
                     grid=None) -> List[torch.Tensor]:
    """frame_list [fs, n, D] backbone tokens (``features_exist=True``) or [fs, 3, H, W] frames; first_seg [1, C, h, w].
    Returns the fs-1 propagated maps ``[C, gh, gw]`` fp64, as the reference (``mask_propagation.py:448-496``).  The token grid is the
    frames' own (H / P, W / P); with ``features_exist=True`` it is ``grid=(gh, gw)``, by default the square ``spatial_resolution``."""
    maps, C, (gh, gw) = _maps(n_last_frames, size_mask_neighborhood, topk, model, frame_list, first_seg, features_exist, grid)
    return [m[0].t().reshape(C, gh, gw) for m in maps]


@torch.no_grad()
def propagate_clip(model, clip: torch.Tensor, first_annotation: torch.Tensor, n_last_frames: int = 4, size_mask_neighborhood: int = 12,
                   topk: int = 5, input_resolution=224, num_classes: Optional[int] = None) -> torch.Tensor:
    """One clip of the evaluation loop (``mask_propagation.py:824-830``): clip [fs,3,H,W], first_annotation [H,W] integer
    labels of frame 0 -> predictions [fs-1, R, R] int64 for frames 1..fs-1, or [fs-1, H', W'] for ``input_resolution=(H', W')``.
    The labels propagate on the clip's own token grid (H / P, W / P)."""
    fe = model.feature_extractor if hasattr(model, "feature_extractor") else model
    P = fe.backbone.patch_embed.patch_size
    grid = (clip.shape[-2] // P, clip.shape[-1] // P)
    feats, _ = fe(clip, use_head=False)
    seed = to_one_hot(first_annotation.unsqueeze(0), num_classes).unsqueeze(0)
    maps, C, (gh, gw) = _maps(n_last_frames, size_mask_neighborhood, topk, model, feats, seed, True, grid)
    H, W = _pair(input_resolution)
    if gh == gw and H == W:
        return ops.upsample_argmax(maps.view(maps.shape[0], gh * gw, C), H)
    return ops.upsample_argmax_hw(maps.view(maps.shape[0], gh * gw, C), (gh, gw), (H, W))


@torch.no_grad()
def jaccard(pred: torch.Tensor, gt: torch.Tensor, num_classes: int, involve_bg: bool = False) -> Tuple[float, torch.Tensor]:
    """Mean Jaccard index (J) of integer label maps with IDENTITY label matching (propagated labels keep their ids) and the
    per-class values.  Classes absent from both prediction and ground truth are skipped; the background (class 0) is
    excluded unless ``involve_bg`` (the reference builds ``PredsmIoU(num_clusters, 10, involve_bg=False)``, :746).  The
    reference's Hungarian / many-to-one matching of ``evaluate_localizations`` belongs to the clustering evaluator and
    is not part of this build."""
    counts = ops.confusion_counts(pred.contiguous().view(-1), gt.contiguous().view(-1).long(), num_classes).double()
    inter = counts.diagonal()
    union = counts.sum(0) + counts.sum(1) - inter
    valid = union > 0
    if not involve_bg:
        valid[0] = False
    iou = torch.where(valid, inter / union.clamp(min=1), torch.full_like(inter, float("nan")))
    return (float(iou[valid].mean()) if valid.any() else float("nan")), iou


# ---- the optical-flow baseline (mask_propagation.py:265-346, :803-815) -------------------------------------------------------------

def _gpu(x) -> torch.Tensor:
    return _device_tensor(x).contiguous()


def calc_optical_flow_farneback(prev, next, pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2, flags=0):
    """``cv2.calcOpticalFlowFarneback(prev, next, None, ...)`` batched over the leading dimensions: prev, next uint8 [..., H, W] (numpy
    or torch) -> flow [..., H, W, 2] fp32 (dx, dy) with prev(x) ~ next(x + flow(x)); numpy in gives numpy out, a tensor gives a tensor
    on the GPU.  flags 0 only (OPTFLOW_USE_INITIAL_FLOW / OPTFLOW_FARNEBACK_GAUSSIAN raise NotImplementedError); see
    ``hip_ops.check_farneback_params`` for the other rules (ValueError)."""
    ops.check_farneback_params(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
    as_numpy = not isinstance(prev, torch.Tensor)
    a, b = _gpu(prev), _gpu(next)
    if a.dtype != torch.uint8 or b.dtype != torch.uint8:
        raise TypeError(f"calc_optical_flow_farneback: frames must be uint8, got {a.dtype} and {b.dtype}")
    if a.dim() < 2 or a.shape != b.shape:
        raise ValueError(f"calc_optical_flow_farneback: prev {tuple(a.shape)} and next {tuple(b.shape)} must be the same [..., H, W]")
    lead, (H, W) = tuple(a.shape[:-2]), tuple(a.shape[-2:])
    n = int(np.prod(lead)) if lead else 1
    frames = torch.cat([a.reshape(n, H, W), b.reshape(n, H, W)], 0).contiguous()
    flow = ops.farneback_flow(frames, [(i, n + i) for i in range(n)], pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
    flow = flow.view(*lead, H, W, 2)
    return flow.cpu().numpy() if as_numpy else flow


def _clip_pairs(bs: int, fs: int):
    """(new, old) = (j + 1, j) of every clip of [bs, fs] frames, frame-major: the argument order of the reference's call (:299)."""
    return [(i * fs + j + 1, i * fs + j) for i in range(bs) for j in range(fs - 1)]


def dense_optical_flow(data_list, params=[], to_gray=False):
    """The reference's ``dense_optical_flow`` (``:265-319``): uint8 gray clips [bs, fs, H, W] -> the flow of every consecutive pair,
    ``calcOpticalFlowFarneback(new, old, None, 0.5, 3, 15, 3, 5, 1.2, 0)``, all pairs of all clips in one batch.  numpy in gives nested
    lists [bs][fs - 1] of [H, W, 2] float32 arrays, as the reference; a GPU tensor gives a GPU tensor [bs, fs - 1, H, W, 2].  ``params``
    and ``to_gray`` are unused, as in the reference; so is its HSV visualisation, which is not built."""
    as_numpy = not isinstance(data_list, torch.Tensor)
    d = _gpu(data_list)
    if d.dim() != 4 or d.dtype != torch.uint8:
        raise ValueError(f"dense_optical_flow: expected uint8 [bs, fs, H, W], got {d.dtype} {tuple(d.shape)}")
    bs, fs, H, W = d.shape
    assert fs >= 2
    flow = ops.farneback_flow(d.reshape(bs * fs, H, W), _clip_pairs(bs, fs)).view(bs, fs - 1, H, W, 2)
    if not as_numpy:
        return flow
    host = flow.cpu().numpy()
    return [[host[i, j] for j in range(fs - 1)] for i in range(bs)]


def _label_tensor(x) -> Tuple[torch.Tensor, object]:
    """Labels -> (uint8 or int64 GPU tensor, the dtype to give back)."""
    t = _device_tensor(x)
    back = t.dtype
    if t.dtype not in (torch.uint8, torch.int64):
        t = t.long()
    return t.contiguous(), back


def interpolate_frames(frame, flow, n_frames):
    """The reference's ``interpolate_frames`` (``:322-333``): [cv2.remap(frame, coords + ((f + 1) / n_frames) * flow, None,
    INTER_NEAREST) for f in range(n_frames)], constant-0 border.  frame [h, w] integer labels, flow [h, w, 2]; numpy in gives numpy
    arrays of the frame's dtype, tensors give GPU tensors."""
    as_numpy = not isinstance(frame, torch.Tensor)
    lab, back = _label_tensor(frame)
    fl = _device_tensor(flow).float().contiguous()
    h, w = lab.shape
    out = []
    for f in range(n_frames):
        r = ops.remap_nearest_labels(lab.view(1, h, w), fl.view(1, 1, h, w, 2), float(np.float32((f + 1) / n_frames)))[0, 0]
        r = r.to(back)
        out.append(r.cpu().numpy() if as_numpy else r)
    return out


def propagate(dataset_flow_list, annotations):
    """The reference's ``propagate`` (``:336-346``): label_{j+1}(x) = label_j(x + flow_j(x)) from annotations[:, 0], each step from the
    previous result, for every clip.  dataset_flow_list: ``dense_optical_flow``'s nested lists or its GPU tensor; annotations [bs, fs, h,
    w] -> uint8 [bs, fs - 1, h, w] (on the CPU for nested lists, as the reference; on the GPU for a GPU flow tensor)."""
    bs, fs, h, w = annotations.shape
    if isinstance(dataset_flow_list, torch.Tensor):
        flows, on_gpu = dataset_flow_list.float().contiguous(), True
    else:
        flows = torch.from_numpy(np.ascontiguousarray(np.asarray(dataset_flow_list, np.float32)))
        flows, on_gpu = _device_tensor(flows).contiguous(), False
    if tuple(flows.shape) != (bs, fs - 1, h, w, 2):
        raise ValueError(f"propagate: flows {tuple(flows.shape)} do not match annotations {tuple(annotations.shape)}")
    first, _ = _label_tensor(annotations[:, 0])
    out = ops.remap_nearest_labels(first, flows).to(torch.uint8)
    return out if on_gpu else out.cpu()


@torch.no_grad()
def propagate_clip_optical_flow(clip: torch.Tensor, first_annotation: torch.Tensor) -> torch.Tensor:
    """The optical-flow branch of the evaluation loop for one clip (``:803-815``): clip [fs, 3, H, W] fp32 on the GPU -> 8-bit gray ->
    Farneback flow of every (new, old) consecutive pair -> the annotation of frame 0 carried forward by nearest remapping.  Returns
    [fs - 1, H, W] int64 predictions for frames 1..fs-1, the contract of ``propagate_clip``; no host round trip."""
    fs, _, H, W = clip.shape
    gray = ops.flow_gray_u8(clip.float().contiguous())
    flows = ops.farneback_flow(gray, _clip_pairs(1, fs))
    first = _device_tensor(first_annotation).long().contiguous().view(1, H, W)
    return ops.remap_nearest_labels(first, flows.view(1, fs - 1, H, W, 2))[0]


# ---- DAVIS J&F (mask_propagation.py:501-715) -------------------------------------------------------------------------------

def disk(radius) -> np.ndarray:
    """The disk structuring element ``f_measure`` takes from ``skimage.morphology.disk``: over the grid ``arange(-radius, radius + 1)``
    in both directions, the points with X^2 + Y^2 <= radius^2, uint8.  A non-integer radius (``bound_th >= 1`` is used as is) gives
    an even size, e.g. 2.5 -> 6 x 6, whose dilation anchor (rows // 2, cols // 2) is off centre."""
    L = np.arange(-radius, radius + 1)
    X, Y = np.meshgrid(L, L)
    return (X ** 2 + Y ** 2 <= radius ** 2).astype(np.uint8)


def _bound_pix(bound_th, shape):
    """Dilation radius of ``f_measure``: ``bound_th`` itself when >= 1, else ceil(bound_th * ||(H, W)||)."""
    return bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm(shape))


def _device_tensor(x) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        t = x
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    return t.to(torch.device("cuda", torch.cuda.current_device()) if not t.is_cuda else t.device)


def _binary(x) -> torch.Tensor:
    """Any mask -> uint8 0 / 1 on the GPU (non-zero is set: the reference's ``astype(bool)``)."""
    return (_device_tensor(x) != 0).to(torch.uint8).contiguous()


def _labels(x) -> torch.Tensor:
    t = _device_tensor(x)
    if t.dtype in (torch.uint8, torch.int64):
        return t.contiguous()
    if t.dtype == torch.bool or not (t.dtype.is_floating_point or t.dtype.is_complex):
        return t.long().contiguous()
    raise TypeError(f"davis_jf: label maps must be integer, got {t.dtype}")


def _binary_counts(gt_mask, fg_mask, void_pixels, bound_th) -> np.ndarray:
    """Binary masks [..., H, W] -> int64 counts [N, 6] over the N = prod(...) frames, one launch."""
    gt_b, fg_b = _binary(gt_mask), _binary(fg_mask)
    if gt_b.dim() < 2:
        raise ValueError(f"masks need at least 2 dimensions, got {gt_b.dim()}")
    H, W = gt_b.shape[-2:]
    gt_b, fg_b = gt_b.reshape(-1, H, W), fg_b.reshape(-1, H, W)
    void = None if void_pixels is None else _binary(void_pixels).reshape(-1, H, W)
    element = disk(_bound_pix(bound_th, (H, W)))
    return ops.davis_jf_counts(fg_b, gt_b, 1, element, void)[0].cpu().numpy()


def _f_from_counts(n_fg, n_gt, fg_match, gt_match):
    """F of ``f_measure`` from its four counts, with its branches and fp64 expressions."""
    if n_fg == 0 and n_gt > 0:
        precision, recall = 1, 0
    elif n_fg > 0 and n_gt == 0:
        precision, recall = 0, 1
    elif n_fg == 0 and n_gt == 0:
        precision, recall = 1, 1
    else:
        precision = fg_match / float(n_fg)
        recall = gt_match / float(n_gt)
    if precision + recall == 0:
        return 0
    return 2 * precision * recall / (precision + recall)


def _f_table(counts: np.ndarray) -> np.ndarray:
    """counts [..., 6] -> F [...] fp64."""
    flat = counts.reshape(-1, 6)
    f = np.zeros(flat.shape[0])
    for i, c in enumerate(flat):
        f[i] = _f_from_counts(c[2], c[3], c[4], c[5])
    return f.reshape(counts.shape[:-1])


def _j_table(counts: np.ndarray) -> np.ndarray:
    """counts [..., 6] -> J [...] fp64: intersection / union, 1 where the union is empty."""
    inter, union = counts[..., 0], counts[..., 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        j = inter / union
    j[union == 0] = 1
    return j


def db_eval_iou(annotation, segmentation, void_pixels=None):
    """Region similarity J (``mask_propagation.py:670-700``) of binary masks [..., H, W] (non-zero is set), numpy or torch:
    |A & S & !void| / |(A | S) & !void| per frame, 1 where that union is empty.  A scalar for 2-D masks (the int 1 for an
    empty union, as the reference), an array of shape [...] otherwise."""
    assert tuple(annotation.shape) == tuple(segmentation.shape), \
        f"Annotation({tuple(annotation.shape)}) and segmentation:{tuple(segmentation.shape)} dimensions do not match."
    if void_pixels is not None:
        assert tuple(annotation.shape) == tuple(void_pixels.shape), \
            f"Annotation({tuple(annotation.shape)}) and void pixels:{tuple(void_pixels.shape)} dimensions do not match."
    counts = _binary_counts(annotation, segmentation, void_pixels, 0.008)
    if len(annotation.shape) == 2:
        inter, union = counts[0, 0], counts[0, 1]
        return 1 if union == 0 else inter / union
    return _j_table(counts).reshape(tuple(annotation.shape[:-2]))


def f_measure(foreground_mask, gt_mask, void_pixels=None, bound_th=0.008):
    """Boundary F-measure (``mask_propagation.py:519-579``) of one binary frame [H, W]: the boundaries of both masks times
    "not void", each dilated by ``disk(bound_pix)`` and matched against the other.  Counts on the GPU, F on the host."""
    assert len(foreground_mask.shape) == 2, "f_measure takes one [H, W] frame"
    assert tuple(foreground_mask.shape) == tuple(gt_mask.shape)
    c = _binary_counts(gt_mask, foreground_mask, void_pixels, bound_th)[0]
    return _f_from_counts(c[2], c[3], c[4], c[5])


def db_eval_boundary(annotation, segmentation, void_pixels=None, bound_th=0.008):
    """Boundary F (``mask_propagation.py:501-515``): [T, H, W] masks -> fp64 [T] (one launch for all frames), [H, W] ->
    ``f_measure(segmentation, annotation)``."""
    assert tuple(annotation.shape) == tuple(segmentation.shape)
    if void_pixels is not None:
        assert tuple(annotation.shape) == tuple(void_pixels.shape)
    if len(annotation.shape) == 3:
        return _f_table(_binary_counts(annotation, segmentation, void_pixels, bound_th))
    if len(annotation.shape) == 2:
        return f_measure(segmentation, annotation, void_pixels, bound_th=bound_th)
    raise ValueError(f"db_eval_boundary does not support tensors with {len(annotation.shape)} dimensions")


def _seg2bmap(seg, width=None, height=None):
    """Binary boundary map of a 2-D segmentation (``mask_propagation.py:582-638``): pixel (y, x) is set where seg differs from its
    right, lower or lower-right neighbour; the last row compares only to the right, the last column only downwards, and the
    bottom-right pixel is 0.  Returns a bool array [H, W].  The reference's rescale to another ``width`` / ``height`` is used by
    no caller and raises NotImplementedError here."""
    assert len(seg.shape) == 2, "_seg2bmap takes one [H, W] map"
    h, w = seg.shape
    if (width is not None and width != w) or (height is not None and height != h):
        raise NotImplementedError("_seg2bmap: rescaling the boundary map to another width / height is not part of this build")
    return ops.davis_seg2bmap(_binary(seg).view(1, h, w))[0].cpu().numpy().astype(bool)


def db_statistics(per_frame_values):
    """Mean, recall (fraction > 0.5) and decay (first quarter minus last quarter) of per-frame values (``mask_propagation.py:
    641-666``), NaN-aware.  The quarter boundaries go through uint8 as in the reference, so past 255 frames they wrap round."""
    v = per_frame_values
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        M = np.nanmean(v)
        O = np.nanmean(v > 0.5)
    edges = (np.round(np.linspace(1, len(v), 4 + 1) + 1e-10) - 1).astype(np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        first = v[edges[0]:edges[1] + 1]
        last = v[edges[3]:edges[4] + 1]
        D = np.nanmean(first) - np.nanmean(last)
    return M, O, D


def evaluate_semisupervised(all_gt_masks, all_res_masks, all_void_masks, metric):
    """Per-object, per-frame J and F tables [O, T] (``mask_propagation.py:702-715``) of binary masks [O, T, H, W] and void
    [T, H, W] (or None).  Missing predicted objects are zero masks; more predicted than GT objects ends the program, as the
    reference.  Every (object, frame) is counted in one launch."""
    n_gt, n_res = all_gt_masks.shape[0], all_res_masks.shape[0]
    if n_res > n_gt:
        sys.stdout.write("\nIn your PNG files there is an index higher than the number of objects in the sequence!")
        sys.exit()
    res = _binary(all_res_masks)
    if n_res < n_gt:
        res = torch.cat([res, torch.zeros((n_gt - n_res, *res.shape[1:]), dtype=res.dtype, device=res.device)], 0)
    gt = _binary(all_gt_masks)
    O, T, H, W = gt.shape
    void = None if all_void_masks is None else _binary(all_void_masks).reshape(1, T, H, W).expand(O, T, H, W)
    j_res, f_res = np.zeros((O, T)), np.zeros((O, T))
    if "J" in metric or "F" in metric:
        counts = _binary_counts(gt, res, void, 0.008).reshape(O, T, 6)
        if "J" in metric:
            j_res[:] = _j_table(counts)
        if "F" in metric:
            f_res[:] = _f_table(counts)
    return j_res, f_res


def davis_jf(pred, gt, num_objects: int, void=None, bound_th: float = 0.008):
    """J and F of objects 1..num_objects of label maps pred, gt [T, H, W] (uint8 or int64 labels; void [T, H, W] or None),
    numpy or torch, from ONE launch of ``tt_davis_jf_counts``: (J, F) fp64 [O, T], each the reference's ``db_eval_iou`` /
    ``db_eval_boundary`` of the masks ``label == o`` to the bit."""
    p, g = _labels(pred), _labels(gt)
    if p.dim() == 2:
        p, g = p.unsqueeze(0), g.unsqueeze(0)
    if p.shape != g.shape:
        raise ValueError(f"davis_jf: pred {tuple(p.shape)} and gt {tuple(g.shape)} differ")
    vd = None if void is None else _binary(void).reshape(p.shape)
    counts = ops.davis_jf_counts(p, g, int(num_objects), disk(_bound_pix(bound_th, tuple(p.shape[-2:]))), vd).cpu().numpy()
    return _j_table(counts), _f_table(counts)


def synthetic_davis_labels(T: int, H: int, W: int, num_objects: int, seed: int):
    """Seeded label maps for the DAVIS metrics: (gt, pred, void) uint8 [T, H, W].  gt has blobby objects 1..num_objects (unions
    of ellipses) with holes, object 1 also covers a band along every image edge, and 1-pixel objects sit in the last row and the
    last column; pred is gt moved by a few pixels with some labels flipped; void marks a few rectangles (DAVIS' 255 regions)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    gt = np.zeros((T, H, W), np.uint8)
    pred = np.zeros((T, H, W), np.uint8)
    void = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        g = gt[t]
        bw = max(1, min(H, W) // 16)
        band = (yy < bw) | (yy >= H - bw) | (xx < bw) | (xx >= W - bw)
        g[band & (rng.random((H, W)) < 0.7)] = 1
        for o in range(1, num_objects + 1):
            for _ in range(int(rng.integers(1, 4))):
                cy, cx = rng.uniform(-0.1, 1.1) * H, rng.uniform(-0.1, 1.1) * W
                ry, rx = rng.uniform(0.05, 0.3) * H + 0.5, rng.uniform(0.05, 0.3) * W + 0.5
                g[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = o
            hy, hx = rng.uniform(0, H), rng.uniform(0, W)
            g[((yy - hy) / (0.04 * H + 0.5)) ** 2 + ((xx - hx) / (0.04 * W + 0.5)) ** 2 <= 1] = 0   # a hole
        g[H - 1, int(rng.integers(0, W))] = int(rng.integers(1, num_objects + 1))
        g[int(rng.integers(0, H)), W - 1] = int(rng.integers(1, num_objects + 1))
        dy, dx = (int(v) for v in rng.integers(-3, 4, 2))
        p = np.roll(g, (dy, dx), (0, 1))
        flip = rng.random((H, W)) < 0.01
        p[flip] = rng.integers(0, num_objects + 2, int(flip.sum()))   # num_objects + 1 is no object
        pred[t] = p
        for _ in range(2):
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            void[t, y0:y0 + max(1, H // 8), x0:x0 + max(1, W // 8)] = 1
    return gt, pred, void


def build_parser() -> argparse.ArgumentParser:
    """Flag names and defaults of ``mask_propagation.py:849-871`` (``type=bool`` flags keep the any-non-empty-string-is-True
    quirk).  ``--dataset synthetic`` / ``synthetic_frames``, ``--raw_size``, ``--num_clips`` and ``--davis_metrics`` are additions; so is
    ``--save_masks DIR``, which writes every clip's seed and predictions as palette PNGs (``my_utils.write_indexed_clip``)."""
    p = argparse.ArgumentParser()
    p.add_argument("--architecture", type=str, default="dino-s16")
    p.add_argument("--model_path", type=str, default="../models/leopart_vits16.ckpt")
    p.add_argument("--dataset", type=str, default="davis_val")
    p.add_argument("--dataset_path", type=str, default="../data")
    p.add_argument("--destination_path", type=str, default="ytvos")
    p.add_argument("--evaluation_protocol", type=str, default="frame-wise")
    p.add_argument("--logging_directory", type=str, default="visualizations")
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--num_workers", type=int, default=10)
    add_decode_arguments(p)
    p.add_argument("--num_clusters", type=int, default=10)
    p.add_argument("--input_resolution", type=int, default=224)
    p.add_argument("--many_to_one", type=bool, default=False)
    p.add_argument("--num_frames", type=int, default=25)
    p.add_argument("--n_last_frames", type=int, default=4)
    p.add_argument("--uvos", type=int, default=True)
    p.add_argument("--topk", type=int, default=5)
    p.add_argument("--size_mask_neighborhood", default=12, type=int)
    p.add_argument("--epsilon", default=0.05, type=float)
    p.add_argument("--sinkhorn_iterations", default=3, type=float)
    p.add_argument("--use_projection_head", type=bool, default=True)
    p.add_argument("--use_optical_flow", type=bool, default=False,
                   help="the dense Farneback optical-flow baseline instead of the ViT features (no backbone is built)")
    p.add_argument("--num_clips", type=int, default=4, help="synthetic data only")
    p.add_argument("--davis_metrics", action="store_true",
                   help="also print DAVIS J / F mean, recall and decay and J&F-Mean per clip and overall (addition)")
    p.add_argument("--raw_size", type=int, nargs=2, default=(360, 480), metavar=("H", "W"),
                   help="--dataset synthetic_frames: size of the raw uint8 frames and label maps that go through the reference's "
                        "Resize -> RandomCrop -> ClipToTensor pair transform; multiples of 8 (addition)")
    p.add_argument("--save_masks", type=str, default=None, metavar="DIR",
                   help="write what is scored as palette PNGs, deflated on the device: DIR/<clip>/00000.png ... per clip - frame 0 the seed "
                        "annotation as propagated from, frames 1.. the predictions, at the size they were predicted at; <clip> is the "
                        "video directory's name, or clip_0000 ... for the synthetic datasets (addition)")
    p.add_argument("--frame_size", type=int, nargs=2, default=None, metavar=("H", "W"),
                   help="synthetic H x W clips propagated on their native token grid (H / P, W / P) and scored at H x W; multiples of "
                        "the patch size P (addition)")
    return p


def synthetic_tracking_clip(fs: int, resolution: int, seed: int, objects: int = 2, width: Optional[int] = None):
    """A clip with ``objects`` textured discs drifting over a textured background, and its per-frame integer masks:
    frames [fs,3,R,W] fp32 (roughly unit-normal, like normalised images), masks [fs,R,W] int64 (0 = background); ``width``
    defaults to R (a square clip)."""
    import numpy as np

    from . import synth

    R = resolution
    W = R if width is None else int(width)
    yy, xx = np.mgrid[0:R, 0:W].astype(np.float32)
    tex = synth.normal("trk.tex", (objects + 1, 3, 8, 8), 1.0, 0.0, seed)
    tex = np.kron(tex, np.ones((1, 1, R // 8, W // 8), np.float32))[:, :, :R, :W]
    pos = synth.normal("trk.pos", (objects, 4), 1.0, 0.0, seed)
    frames, masks = [], []
    for t in range(fs):
        img = tex[0].copy()
        m = np.zeros((R, W), np.int64)
        for o in range(objects):
            cy = R * (0.3 + 0.4 * o / max(objects - 1, 1)) + 3.0 * t * np.tanh(pos[o, 0])
            cx = W * (0.3 + 0.2 * o) + 4.0 * t * np.tanh(pos[o, 1])
            rad = min(R, W) * (0.12 + 0.03 * abs(np.tanh(pos[o, 2])))
            inside = (yy - cy) ** 2 + (xx - cx) ** 2 < rad ** 2
            img = np.where(inside[None], tex[o + 1] + 1.5 * (o + 1), img)
            m[inside] = o + 1
        frames.append(img + 0.05 * synth.normal(f"trk.noise.{t}", (3, R, W), 1.0, 0.0, seed))
        masks.append(m)
    return torch.from_numpy(np.stack(frames).astype(np.float32)), torch.from_numpy(np.stack(masks))


def synthetic_frame_clip(fs: int, height: int, width: int, seed: int, objects: int = 2):
    """``synthetic_tracking_clip`` as a decoder would hand it over: raw frames uint8 [fs, H, W, 3] (the unit-normal textures mapped to
    127 + 50 x, clipped) and label maps uint8 [fs, H, W] (0 = background, objects 1..).  H and W are multiples of the 8 x 8 texture cell."""
    if height <= 0 or width <= 0 or height % 8 or width % 8:
        raise ValueError(f"raw size {height} x {width}: both sides must be positive multiples of 8")
    clip, masks = synthetic_tracking_clip(fs, height, seed, objects, width=width)
    frames = (127.0 + 50.0 * clip).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return frames, masks.to(torch.uint8)


def synthetic_frames_clip(args, index: int, device):
    """Clip ``index`` of ``--dataset synthetic_frames``: raw frames and label maps through ``propagation_transforms`` (the pair
    transform of ``mask_propagation.py:779``, seeded per clip) and ``read_batch``'s uint8 conversion, as the reference's loader
    delivers them: (clip float32 [fs, 3, R, R], masks int64 [fs, R, R]) on ``device``."""
    import random

    from . import video_transformations as VT

    H, W = (int(v) for v in args.raw_size)
    frames, labels = synthetic_frame_clip(args.num_frames, H, W, seed=index + 1)
    random.seed(index + 1)
    data, ann = VT.propagation_transforms(args.input_resolution)(frames.to(device), labels.to(device))
    return data, VT.annotations_to_uint8(ann[None])[0].long()


def clip_size(args, patch_size: int) -> Tuple[int, int]:
    """(H, W) of the evaluation clips: ``--frame_size H W`` (each a multiple of the patch size, else ValueError) or the square
    ``--input_resolution``."""
    if getattr(args, "frame_size", None) is None:
        return args.input_resolution, args.input_resolution
    H, W = (int(v) for v in args.frame_size)
    if H <= 0 or W <= 0 or H % patch_size or W % patch_size:
        raise ValueError(f"--frame_size {H} {W}: both sides must be positive multiples of the patch size {patch_size}")
    return H, W


# the synthetic clips' textures are 8 x 8 cells, so the optical-flow branch (which builds no backbone) takes --frame_size in multiples of 8
_FLOW_FRAME_MULTIPLE = 8


def mask_propagation(args, vit_cfg: Optional[dict] = None) -> float:
    """The evaluation loop of ``mask_propagation.py:757-846``; returns the mean J over clips.  ``--dataset synthetic`` renders normalised
    clips at the model's size; ``--dataset synthetic_frames`` renders raw uint8 frames with label maps at ``--raw_size`` and takes them
    through the reference's pair transform first (``synthetic_frames_clip``); any other name reads ``--dataset_path``
    (``data_loader.make_loader``: JPEGImages/ and Annotations/, ``propagation_transforms``, ``SamplingMode.DENSE``, ``--num_frames``, batch 1,
    one clip per video; the first frame's annotation is the seed).  With
    ``--davis_metrics`` it also prints the DAVIS statistics (``db_statistics`` over each object's frames) per clip and over all
    objects of all clips; the return value is the same.  ``--use_optical_flow`` runs the optical-flow baseline
    (``propagate_clip_optical_flow``) on the same clips, with the same scoring, and builds no backbone.  ``--save_masks DIR`` writes,
    in both branches, one directory per clip with the seed annotation as frame 0 and the predictions behind it as palette PNGs deflated on
    the device (``my_utils.write_indexed_clip``: the only writer this build has; one encode call per clip); printed scores and the return
    value are unchanged.  ``vit_cfg`` replaces the architecture's dimensions (tests).  Both branches score predicted
    frame j against annotated frame j; the reference compares ``predictions[:, 1:]`` with ``annotations[:, 1:]``, one frame off."""
    use_flow = bool(args.use_optical_flow)
    save_masks = getattr(args, "save_masks", None)
    native = getattr(args, "frame_size", None) is not None
    from_disk = args.dataset not in ("synthetic", "synthetic_frames")
    raw_frames = args.dataset == "synthetic_frames"
    if (raw_frames or from_disk) and native:
        raise ValueError("--dataset synthetic_frames and the datasets on disk crop to --input_resolution as the reference's loader does; "
                         "--frame_size does not apply")
    device = torch.device("cuda", 0)
    disk_clips, disk_loader = None, None
    if from_disk:   # <dataset_path>/JPEGImages + Annotations, decoded on the device (data_loader.py, N21); batch 1 (:775-790)
        from . import data_loader as DL
        from . import video_transformations as VT

        disk_loader = DL.make_loader(args.dataset_path, args.num_frames, 1, 1, DL.SamplingMode.DENSE, frame_transform=None, target_transform=None,
                                     video_transform=VT.propagation_transforms(args.input_resolution), shuffle=False,
                                     num_workers=args.num_workers, device=device, jpeg_entropy=args.jpeg_entropy, png=args.png_decode)
        if not disk_loader.dataset.use_annotations:
            raise FileNotFoundError(f"{args.dataset_path}/Annotations: the propagation evaluation needs the first frame's annotation")
        disk_clips = iter(disk_loader)
    if use_flow:
        H, W = clip_size(args, _FLOW_FRAME_MULTIPLE)
        model = None
    else:
        from .models import FeatureExtractor
        from .time_tuning import TimeT

        fe = FeatureExtractor(args.architecture, args.model_path, [1024, 1024, 512, 256], return_attention=False, vit_cfg=vit_cfg)  # "" = synthetic weights
        H, W = clip_size(args, fe.backbone.patch_embed.patch_size)
        model = TimeT(fe, 200).to(device).eval()
    scores = []
    davis = []   # per object: (J_M, J_R, J_D, F_M, F_R, F_D)
    for i in range(len(disk_loader) if from_disk else args.num_clips):
        if from_disk:
            data, annotations, label = next(disk_clips)
            clip, masks = data[0, 0], annotations[0, 0].long()   # the first frame's annotation is the seed
        elif raw_frames:
            clip, masks = synthetic_frames_clip(args, i, device)
        elif native:
            clip, masks = synthetic_tracking_clip(args.num_frames, H, seed=i + 1, width=W)
        else:
            clip, masks = synthetic_tracking_clip(args.num_frames, args.input_resolution, seed=i + 1)
        if args.uvos:  # all objects become one foreground class (:797-799)
            masks = (masks > 0).long()
        C = int(masks.max()) + 1
        if use_flow:
            pred = propagate_clip_optical_flow(clip.to(device), masks[0].to(device))
        else:
            pred = propagate_clip(model, clip.to(device), masks[0].to(device), args.n_last_frames, args.size_mask_neighborhood, args.topk,
                                  (H, W) if native else args.input_resolution, C)
        if save_masks:   # what is scored, as files: the seed as propagated from, then the predictions (one encode call per clip)
            from .my_utils import write_indexed_clip

            name = os.path.basename(os.path.normpath(str(disk_loader.dataset.keys[int(label)]))) if from_disk else f"clip_{i:04d}"
            seed = masks[0].to(device)
            if seed.shape != pred.shape[1:]:
                raise ValueError(f"--save_masks: the seed is {tuple(seed.shape)}, the predictions are {tuple(pred.shape[1:])}")
            write_indexed_clip(os.path.join(save_masks, name), torch.cat([seed[None].to(pred.dtype), pred], 0))
        j, _ = jaccard(pred, masks[1:].to(device), C)
        scores.append(j)
        print(f"clip {i}: J = {j:.4f}")
        if getattr(args, "davis_metrics", False) and C > 1:
            J, Fb = davis_jf(pred, masks[1:].to(device), C - 1)
            rows = [db_statistics(J[o]) + db_statistics(Fb[o]) for o in range(C - 1)]
            davis.extend(rows)
            print(f"clip {i}: " + _davis_line(np.array(rows, np.float64)))
    mean = sum(scores) / len(scores)
    print(f"mean J over {len(scores)} clips: {mean:.4f}")
    if from_disk:
        print(f"frames decoded with Pillow on the host (files the device decoder does not take): {disk_loader.fallback_frames}")
    if davis:
        print(f"DAVIS over {len(davis)} objects of {len(scores)} clips: " + _davis_line(np.array(davis, np.float64)))
    return mean


def _davis_line(rows: np.ndarray) -> str:
    """rows [objects, 6] of (J_M, J_R, J_D, F_M, F_R, F_D) -> their means over the objects, and J&F-Mean."""
    m = rows.mean(0)
    return (f"J&F-Mean {(m[0] + m[3]) / 2:.4f}  J_M {m[0]:.4f} J_R {m[1]:.4f} J_D {m[2]:.4f}  "
            f"F_M {m[3]:.4f} F_R {m[4]:.4f} F_D {m[5]:.4f}")


if __name__ == "__main__":
    mask_propagation(build_parser().parse_args())
