"""Dense nearest-neighbour retrieval evaluation (N31): the "in-context scene understanding" protocol of Balazevic et al., 2023
("Hummingbird").  Nothing is trained: the patch features of a labelled training set form a memory bank with their per-patch class
distributions; every patch of a validation image retrieves its k nearest bank patches by cosine similarity and takes the
softmax-weighted mean of their distributions; the result is upsampled, arg-maxed and scored as mIoU with identity matching, exactly as
``linear_finetune.validate`` scores the linear probe.

    features -> l2norm_fwd -> nn_search (linear_fwd blocks + tt_topk_merge) -> nn_label_aggregate -> upsample_argmax_f32

The reference has no such evaluation; DESIGN.md N31 states what is built and what is not.
"""
from __future__ import annotations

import argparse
from typing import Optional

import torch
import torch.nn.functional as F

from . import hip_ops as ops
from .data_loader import add_decode_arguments
from .linear_finetune import IGNORE_INDEX, MAX_C, MAX_G, MAX_R, _batches, _extractor, synthetic_segmentation
from .metrics import PredsmIoU

DEFAULT_SELECT = "hip"   # the command line's --select: DESIGN.md N31, "measured"


class MemoryBank:
    """``MemoryBank(num_classes, patches_per_image=None, seed=1)``: ``add(features [B, n, D], masks uint8 [B, R, R])`` L2-normalises the
    features, turns the masks into per-patch class distributions (counts / valid pixels over the sqrt(n) x sqrt(n) grid, 255 ignored),
    drops the patches without a valid pixel and - with ``patches_per_image`` - keeps a random subset of that many patches per image,
    drawn by a CPU ``torch.Generator`` seeded once, so a run is reproducible.  ``finalize()`` -> ``(features [N, D], labels [N, C])``."""

    def __init__(self, num_classes: int, patches_per_image: Optional[int] = None, seed: int = 1):
        if not 1 <= int(num_classes) <= MAX_C:
            raise ValueError(f"MemoryBank: {num_classes} classes are not supported (need 1..{MAX_C})")
        if patches_per_image is not None and int(patches_per_image) < 1:
            raise ValueError(f"MemoryBank: patches_per_image = {patches_per_image} must be at least 1 (or None for all)")
        self.num_classes = int(num_classes)
        self.patches_per_image = None if patches_per_image is None else int(patches_per_image)
        self.generator = torch.Generator(device="cpu")
        self.generator.manual_seed(int(seed))
        self._features, self._labels = [], []
        self.features = self.labels = None

    def sample(self, valid_row: torch.Tensor) -> torch.Tensor:
        """Host only: the sorted indices of the patches of one image that enter the bank.  valid_row: the image's valid-pixel counts on the CPU."""
        keep = torch.nonzero(valid_row > 0).flatten()
        if self.patches_per_image is not None and keep.numel() > self.patches_per_image:
            pick = torch.randperm(keep.numel(), generator=self.generator)[: self.patches_per_image]
            keep = keep[torch.sort(pick).values]
        return keep

    def add(self, features: torch.Tensor, masks: torch.Tensor) -> None:
        if self.features is not None:
            raise RuntimeError("MemoryBank.add: the bank is finalized")
        B, n, D = features.shape
        g = int(round(n ** 0.5))
        if g * g != n:
            raise ValueError(f"MemoryBank.add: {n} tokens are not a square grid")
        feats = ops.l2norm_fwd(features.detach().float().contiguous().view(B * n, D))
        counts, valid = ops.patch_label_counts(masks.contiguous(), g, self.num_classes, ignore=IGNORE_INDEX)
        valid_host = valid.cpu()
        keep = torch.cat([b * n + self.sample(valid_host[b]) for b in range(B)]).to(features.device)
        dist = counts.view(B * n, -1)[keep].float() / valid.view(B * n, 1)[keep].float()
        self._features.append(feats[keep])
        self._labels.append(dist)

    def finalize(self):
        if self.features is None:
            if not self._features:
                raise RuntimeError("MemoryBank.finalize: the bank is empty")
            self.features = torch.cat(self._features).contiguous()
            self.labels = torch.cat(self._labels).contiguous()
            self._features, self._labels = [], []
        if self.features.shape[0] < 1:
            raise RuntimeError("MemoryBank.finalize: no patch of the training set has a valid pixel")
        return self.features, self.labels

    def __len__(self) -> int:
        return int(self.features.shape[0]) if self.features is not None else sum(int(f.shape[0]) for f in self._features)


def prepare_masks(y: torch.Tensor, mask_size: int) -> torch.Tensor:
    """Labels as the loaders deliver them ([B, 1, S, S] fp32, label / 255) -> uint8 [B, R, R]: ``y * 255``, nearest to the mask size
    (``linear_finetune.prepare_labels``), as bytes."""
    y = F.interpolate((y * 255).float(), size=(mask_size, mask_size), mode="nearest")
    return y.squeeze(1).round().to(torch.uint8).contiguous()


class DenseNNEvaluator:
    """``DenseNNEvaluator(model, num_classes, k=30, beta=0.02, mask_size=100, use_head=False)``.  ``model``: a ``FeatureExtractor`` or a
    module holding one as ``feature_extractor`` (``TimeT``); ``model(x, use_head=...)`` must return ``(features [B, n, D], _)``.
    ``fit(train_loader)`` builds the bank, ``predict(x)`` -> [B, R, R] int64, ``evaluate(val_loader)`` -> mIoU."""

    def __init__(self, model, num_classes: int, k: int = 30, beta: float = 0.02, mask_size: int = 100, use_head: bool = False,
                 patches_per_image: Optional[int] = None, seed: int = 1, search_workspace_bytes: int = ops.NN_SEARCH_WORKSPACE_BYTES,
                 select: str = "hip"):
        if not 1 <= int(k) <= ops.NN_MAX_K:
            raise ValueError(f"DenseNNEvaluator: k = {k} is outside 1 .. {ops.NN_MAX_K}")
        if not float(beta) > 0:
            raise ValueError(f"DenseNNEvaluator: beta = {beta} must be positive")
        if not 1 <= int(mask_size) <= MAX_R:
            raise ValueError(f"DenseNNEvaluator: mask size {mask_size} is not supported (need 1..{MAX_R})")
        if select not in ("hip", "torch"):
            raise ValueError(f"DenseNNEvaluator: select = {select!r} is neither 'hip' nor 'torch'")
        self.model = model
        self.num_classes, self.k, self.beta, self.mask_size, self.use_head = int(num_classes), int(k), float(beta), int(mask_size), bool(use_head)
        self.select, self.search_workspace_bytes = select, int(search_workspace_bytes)
        self.bank = MemoryBank(num_classes, patches_per_image, seed)
        self._workspace = None

    @torch.no_grad()
    def features(self, x: torch.Tensor) -> torch.Tensor:
        """[B, g*g, D] fp32 patch features of the images x, not normalised."""
        feats, _ = self.model(x, use_head=self.use_head)
        feats = feats.detach().float().contiguous()
        g = int(round(feats.shape[1] ** 0.5))
        if g * g != feats.shape[1] or not 1 <= g <= MAX_G:
            raise ValueError(f"DenseNNEvaluator: {feats.shape[1]} tokens are not a square grid of at most {MAX_G}^2")
        return feats

    def bank_mask_size(self, g: int) -> int:
        """The bank's masks are resized to the multiple of the token grid nearest above the mask size: every cell is whole pixels."""
        return g * max(-(-self.mask_size // g), 1)

    @torch.no_grad()
    def fit(self, train_loader, max_images: Optional[int] = None) -> MemoryBank:
        _extractor(self.model).eval()
        seen = 0
        for x, y in train_loader:
            if max_images is not None and seen >= max_images:
                break
            if max_images is not None:
                x, y = x[: max_images - seen], y[: max_images - seen]
            x, y = x.cuda(), y.cuda()
            feats = self.features(x)
            g = int(round(feats.shape[1] ** 0.5))
            self.bank.add(feats, prepare_masks(y, self.bank_mask_size(g)))
            seen += int(x.shape[0])
        self.bank.finalize()
        return self.bank

    def search(self, queries: torch.Tensor):
        """``hip_ops.nn_search`` of L2-normalised queries [Q, D] against the bank, on the evaluator's workspace."""
        bank, _ = self.bank.finalize()
        if self._workspace is None or self._workspace.device != queries.device:
            self._workspace = torch.empty(max(self.search_workspace_bytes, 16), dtype=torch.uint8, device=queries.device)
        return ops.nn_search(queries, bank, self.k, self.search_workspace_bytes, select=self.select, workspace=self._workspace)

    @torch.no_grad()
    def scores_from_features(self, feats: torch.Tensor) -> torch.Tensor:
        """feats [B, n, D] -> the retrieved class distributions [B, n, C]."""
        _, labels = self.bank.finalize()
        B, n, D = feats.shape
        queries = ops.l2norm_fwd(feats.view(B * n, D))
        vals, idx = self.search(queries)
        return ops.nn_label_aggregate(vals, idx, labels, self.beta).view(B, n, -1)

    @torch.no_grad()
    def predict(self, x: torch.Tensor) -> torch.Tensor:
        return ops.upsample_argmax_f32(self.scores_from_features(self.features(x)), self.mask_size)

    @torch.no_grad()
    def evaluate(self, val_loader) -> float:
        """``linear_finetune.validate``'s scoring (reference ``linear_finetune.py:34-51``) of ``predict``."""
        _extractor(self.model).eval()
        miou = PredsmIoU(self.num_classes, self.num_classes, involve_bg=True)
        R = self.mask_size
        for x, y in val_loader:
            x, y = x.cuda(), y.cuda()
            gt = F.interpolate((y * 255).float(), size=(R, R), mode="nearest").squeeze(1)
            valid = gt != IGNORE_INDEX
            out = self.predict(x)
            miou.update(gt[valid].flatten(), out[valid].flatten())
        value = miou.compute(True, linear_probe=True)[0]
        print("dense NN retrieval: k {}, beta {}, bank {} patches, mIoU: {}".format(self.k, self.beta, len(self.bank), value))
        return value


# ---- the command line -------------------------------------------------------------------------------------------------------------------

def build_parser() -> argparse.ArgumentParser:
    """``linear_finetune.build_parser``'s model and data flags, and the protocol's own.  ``--select``: DESIGN.md N31 has the measurement
    behind the default."""
    p = argparse.ArgumentParser()
    p.add_argument("--architecture", type=str, default="dino-s16")
    p.add_argument("--model_path", type=str, default="dino-s16.pth")
    p.add_argument("--head_layers", type=int, nargs="+", default=[1024, 1024, 512, 256])
    p.add_argument("--num_prototypes", type=int, default=200)
    p.add_argument("--num_classes", type=int, default=21)
    p.add_argument("--mask_size", type=int, default=100)
    p.add_argument("--batch_size", type=int, default=60)
    p.add_argument("--input_resolution", type=int, default=448)
    p.add_argument("--dataset", type=str, default="voc", choices=["synthetic", "voc"])
    p.add_argument("--dataset_path", type=str, default="../../dataset/leopascal/VOCSegmentation")
    add_decode_arguments(p, jpeg=False)
    p.add_argument("--num_train_images", type=int, default=120, help="synthetic data only")
    p.add_argument("--num_val_images", type=int, default=60, help="synthetic data only")
    p.add_argument("--k", type=int, default=30, help="neighbours per patch")
    p.add_argument("--beta", type=float, default=0.02, help="softmax temperature of the neighbours' weights")
    p.add_argument("--patches_per_image", type=int, default=0, help="bank patches kept per training image, a seeded random subset (0 = all)")
    p.add_argument("--bank_images", type=int, default=0, help="training images that enter the bank (0 = all)")
    p.add_argument("--bank_seed", type=int, default=1)
    p.add_argument("--search_workspace_mb", type=int, default=ops.NN_SEARCH_WORKSPACE_BYTES >> 20,
                   help="MiB of similarities held at once by the search")
    p.add_argument("--select", type=str, default=DEFAULT_SELECT, choices=["hip", "torch"],
                   help="the search's select step: tt_topk_merge, or torch.topk on the same blocks")
    return p


def main(argv: Optional[list] = None) -> float:
    """Builds the bank from the training split, scores the validation split; returns the mIoU."""
    from .models import FeatureExtractor
    from .time_tuning import TimeT

    args = build_parser().parse_args(argv)
    torch.cuda.set_device(0)
    feature_extractor = FeatureExtractor(args.architecture, args.model_path, list(args.head_layers), return_attention=False)
    return run(TimeT(feature_extractor, args.num_prototypes).cuda(), args)


def run(model, args) -> float:
    """``main`` behind the model's construction (tests hand in a small architecture)."""
    if args.dataset == "voc":
        from .leoloader import pascal_loader

        train_loader = pascal_loader(args.batch_size, args.dataset_path, "trainaug", args.mask_size, train_size=args.input_resolution,
                                     png=args.png_decode)
        val_loader = pascal_loader(args.batch_size, args.dataset_path, "val", args.mask_size, train_size=args.input_resolution, png=args.png_decode)
    else:
        x_tr, y_tr = synthetic_segmentation(args.num_train_images, args.input_resolution, args.num_classes, seed=1)
        x_va, y_va = synthetic_segmentation(args.num_val_images, args.input_resolution, args.num_classes, seed=2)
        train_loader = _batches(x_tr, y_tr, args.batch_size)
        val_loader = _batches(x_va, y_va, args.batch_size)
    evaluator = DenseNNEvaluator(model, args.num_classes, k=args.k, beta=args.beta, mask_size=args.mask_size,
                                 patches_per_image=args.patches_per_image or None, seed=args.bank_seed,
                                 search_workspace_bytes=args.search_workspace_mb << 20, select=args.select)
    evaluator.fit(train_loader, max_images=args.bank_images or None)
    print("bank", len(evaluator.bank), "patches")
    return evaluator.evaluate(val_loader)


if __name__ == "__main__":
    main()
