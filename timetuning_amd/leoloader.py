"""The reference's Pascal VOC reader (``leoloader.py:129-264``) with the pixel work on the device (N22).

``pascal_loader(batch_size, root, split, val_size, train_size)`` is what every reference program that reports a VOC number reads its data
from (``time_tuning.py:596``, ``linear_finetune.py:69-71``, ``cluster_based_foreground_extraction.py:340-341``, ``evaluation.py:537``).
Both of its branches yield ``(x float32 [b, 3, S, S], y float32 [b, 1, R, R])``: ``Resize((S, S))`` + ``ToTensor`` + ``Normalize`` of
``Image.open(..).convert('RGB')`` and ``Resize((R, R), NEAREST)`` + ``ToTensor`` of the palette PNG (index / 255), in file order (the
reference overrides ``shuffle`` to ``False``, ``:263``), the last batch partial.

Here a batch is two host steps and three device steps.  Host (may run one batch ahead in a background thread, as ``data_loader.ClipLoader``
does): the files are read, the JPEGs entropy-decoded into one pinned buffer (``data_loader.scan_frames``) and the PNGs decoded with Pillow
(``data_loader.decode_annotations``, in the thread pool) into ONE packed pinned buffer - or, with ``png="device"`` (N26), prepared for ONE
``hip_ops.png_decode`` launch whose buffer and offsets the mask gather then reads (a PNG it does not take: Pillow, counted in
``fallback_annotations``).  Device: ``data_loader.finish_frames`` reconstructs the frames, then
ONE ``tt_img_resize_ragged`` launch covers every image of the mixed-size batch and ONE ``tt_img_gather_nearest_ragged`` launch every mask.
A JPEG the device decoder does not take (progressive, gray, ...) is decoded with Pillow and COUNTED (``fallback_frames``), by N21's rule; a
supported file that fails to decode raises.  All of it is bit-equal to the reference's Pillow chain.

The pair transforms the reference defines beside the loader (``Compose``, ``RandomResizedCrop``, ``RandomHorizontalFlip``, ``ToTensor``,
``Normalize``; it builds ``train_transforms`` from them and then does not use it, ``:242-257``) are batch-level objects here: they fill
the box and flip fields of the batch's descriptor table, and the same two launches carry them out.  ``pascal_loader`` does not use them
either.  ``VOCDataModule`` needs Lightning and is not built; its class list is ``CLASS_IDX_TO_NAME``.
"""
from __future__ import annotations

import math
import os
import random
from typing import List, Optional

import numpy as np
import torch

from . import hip_ops as ops
from . import data_loader as DL     # (scan_frames and decode_annotations through the module: looked up when called, as ClipLoader does)
from .data_loader import _read, _route, finish_annotations, finish_frames, prefetched, scan_annotations

CLASS_IDX_TO_NAME = ['background', 'aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair',
                     'cow', 'diningtable', 'dog', 'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa',
                     'train', 'tvmonitor']
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


# ---- the pair transforms (:129-183) as batch-level plans ---------------------------------------------------------------------------

class BatchPlan:
    """What a chain of pair transforms decided for one batch: per item a crop box ``(x0, y0, w, h)`` (None = the whole image) and a flip,
    the output size of a ``RandomResizedCrop`` (None = the loader's sizes), and whether ``ToTensor`` / ``Normalize`` end the chain."""

    def __init__(self, dims):
        self.dims = [(int(h), int(w)) for h, w in dims]
        self.boxes: List[Optional[tuple]] = [None] * len(self.dims)
        self.flips = [False] * len(self.dims)
        self.size = None
        self.to_tensor = False
        self.mean_std = None


class RandomHorizontalFlip:
    """``:129-137``: one ``random()`` per pair, image and target flipped together."""

    def __init__(self, p=0.5):
        self.p = p

    def __call__(self, plan: BatchPlan, rng) -> BatchPlan:
        for i in range(len(plan.dims)):
            if rng.random() < self.p:
                plan.flips[i] = not plan.flips[i]
        return plan


class RandomResizedCrop:
    """``:140-148``: one box per pair by torchvision's ``RandomResizedCrop.get_params`` rule, drawn from a ``random.Random``; the image is
    resized to ``size`` bilinearly and the target with NEAREST."""

    def __init__(self, size, scale, ratio=(3. / 4., 4. / 3.)):
        self.size = (size, size) if isinstance(size, int) else tuple(size)
        self.scale, self.ratio = tuple(scale), tuple(ratio)

    @staticmethod
    def get_params(height: int, width: int, scale, ratio, rng):
        """-> (y1, x1, h, w): ten tries of (area fraction uniform in ``scale``, aspect ratio log-uniform in ``ratio``), then the central
        crop at the nearest allowed ratio."""
        area = height * width
        log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
        for _ in range(10):
            target_area = area * rng.uniform(scale[0], scale[1])
            aspect_ratio = math.exp(rng.uniform(log_ratio[0], log_ratio[1]))
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            if 0 < w <= width and 0 < h <= height:
                i = rng.randint(0, height - h)
                j = rng.randint(0, width - w)
                return i, j, h, w
        in_ratio = float(width) / float(height)
        if in_ratio < min(ratio):
            w = width
            h = int(round(w / min(ratio)))
        elif in_ratio > max(ratio):
            h = height
            w = int(round(h * max(ratio)))
        else:
            w, h = width, height
        return (height - h) // 2, (width - w) // 2, h, w

    def __call__(self, plan: BatchPlan, rng) -> BatchPlan:
        if any(b is not None for b in plan.boxes) or any(plan.flips):
            raise ValueError("RandomResizedCrop must come first in a chain: it draws its box on the stored image")
        for i, (H, W) in enumerate(plan.dims):
            y1, x1, h, w = self.get_params(H, W, self.scale, self.ratio, rng)
            plan.boxes[i] = (x1, y1, w, h)
        plan.size = self.size
        return plan


class ToTensor:
    def __call__(self, plan: BatchPlan, rng) -> BatchPlan:
        plan.to_tensor = True
        return plan


class Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = tuple(mean), tuple(std)

    def __call__(self, plan: BatchPlan, rng) -> BatchPlan:
        if not plan.to_tensor:
            raise ValueError("Normalize works on tensors: ToTensor must come before it")
        plan.mean_std = (self.mean, self.std)
        return plan


class Compose:
    """``:168-183``.  ``compose(dims, rng)`` -> the ``BatchPlan`` of a batch whose images are ``dims[i] = (H, W)``."""

    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, dims, rng=None) -> BatchPlan:
        plan = dims if isinstance(dims, BatchPlan) else BatchPlan(dims)
        rng = random if rng is None else rng
        for t in self.transforms:
            plan = t(plan, rng)
        return plan

    def __repr__(self):
        format_string = self.__class__.__name__ + "("
        for t in self.transforms:
            format_string += "\n"
            format_string += "    {0}".format(t)
        format_string += "\n)"
        return format_string


def train_transforms(train_size: int) -> Compose:
    """The chain ``pascal_loader`` builds and leaves unused (``:242-247``)."""
    return Compose([RandomResizedCrop(size=train_size, scale=(0.8, 1.)), RandomHorizontalFlip(p=0.5), ToTensor(), Normalize(mean=MEAN, std=STD)])


# ---- the dataset (:185-238) --------------------------------------------------------------------------------------------------------

class VOCDataset:
    """The reference's file layout and errors: ``root/images/<name>.jpg``, ``root/SegmentationClassAug/<name>.png`` for ``train`` /
    ``trainaug`` and ``root/SegmentationClass/<name>.png`` for ``val``, names from ``root/sets/<image_set>.txt`` in the file's order.
    ``device``, ``threads``, ``jpeg_entropy`` ("host" / "device": where the Huffman coding is undone) and ``png`` ("host" / "device": where
    the mask PNGs are inflated) belong to the decode."""

    def __init__(self, root: str, image_set: str = "trainaug", transform=None, target_transform=None, transforms=None, return_masks: bool = False,
                 device=None, threads: int = 8, jpeg_entropy: str = "host", png: str = "host"):
        self.jpeg_entropy, self.png = _route("jpeg_entropy", jpeg_entropy), _route("png", png)
        self.root, self.image_set = root, image_set
        if image_set == "trainaug" or image_set == "train":
            seg_folder = "SegmentationClassAug"
        elif image_set == "val":
            seg_folder = "SegmentationClass"
        else:
            raise ValueError(f"No support for image set {self.image_set}")
        seg_dir = os.path.join(root, seg_folder)
        image_dir = os.path.join(root, 'images')
        if not os.path.isdir(seg_dir) or not os.path.isdir(image_dir) or not os.path.isdir(root):
            raise RuntimeError('Dataset not found or corrupted.')
        split_f = os.path.join(root, 'sets', image_set.rstrip('\n') + '.txt')
        with open(split_f, "r") as f:
            file_names = [x.strip() for x in f.readlines()]
        self.seg_folder = seg_folder
        self.images = [os.path.join(image_dir, x + ".jpg") for x in file_names]
        self.masks = [os.path.join(seg_dir, x + ".png") for x in file_names]
        self.transform, self.target_transform, self.transforms, self.return_masks = transform, target_transform, transforms, return_masks
        for path in self.masks + self.images:     # (the reference asserts: masks first, then images)
            if not os.path.isfile(path):
                raise FileNotFoundError(f"VOCDataset: {path} is listed in {split_f} but is not a file")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None and torch.cuda.is_available() else device
        self.threads = int(threads)
        self.fallback_frames = 0
        self.fallback_annotations = 0

    def __len__(self) -> int:
        return len(self.images)


class _VOCHostBatch:
    def __init__(self, frames, mask_buf, mask_offs, mask_dims, masks=None):
        self.frames, self.mask_buf, self.mask_offs, self.mask_dims = frames, mask_buf, mask_offs, mask_dims
        self.masks = masks      # png="device": the ``HostFiles`` of the batch, and the three mask_* fields are None


class VOCLoader:
    """What ``pascal_loader`` returns: an iterable of ``(x float32 [b, 3, S, S], y float32 [b, 1, R, R])`` on the device with
    ``__len__`` = ceil(n / batch_size).  ``transforms``: a ``Compose`` of the pair transforms above (``pascal_loader`` passes none); its
    ``RandomResizedCrop`` size then replaces both S and R, as in the reference, and ``rng`` (a ``random.Random``) draws for it."""

    def __init__(self, dataset: VOCDataset, batch_size: int, val_size: int, train_size: int = 448, transforms: Optional[Compose] = None,
                 rng=None, prefetch: bool = True):
        if batch_size < 1:
            raise ValueError(f"batch_size {batch_size}")
        self.dataset, self.batch_size, self.val_size, self.train_size = dataset, int(batch_size), int(val_size), int(train_size)
        self.transforms, self.rng, self.prefetch = transforms, (random.Random(0) if rng is None else rng), prefetch

    @property
    def fallback_frames(self) -> int:
        return self.dataset.fallback_frames

    @property
    def fallback_annotations(self) -> int:
        return self.dataset.fallback_annotations

    def __len__(self) -> int:
        return -(-len(self.dataset) // self.batch_size)

    # ---- host half: file reads, entropy decode, PNG decode (no launch: a background thread may run it)
    def _host(self, indices) -> _VOCHostBatch:
        ds = self.dataset
        frames = DL.scan_frames([_read(ds.images[i]) for i in indices], ds.threads, ds.jpeg_entropy)
        if ds.png == "device":
            return _VOCHostBatch(frames, None, None, None, scan_annotations([_read(ds.masks[i]) for i in indices], ds.threads))
        masks = DL.decode_annotations([_read(ds.masks[i]) for i in indices], ds.threads)
        offs = np.zeros(len(masks) + 1, np.int64)
        np.cumsum([m.size for m in masks], out=offs[1:])
        mask_buf = torch.empty(int(offs[-1]), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        view = mask_buf.numpy()
        for m, o in zip(masks, offs):
            view[o:o + m.size] = m.reshape(-1)
        return _VOCHostBatch(frames, mask_buf, [int(o) for o in offs[:-1]], [m.shape for m in masks])

    # ---- device half: reconstruction and the two ragged launches
    def _finish(self, host: _VOCHostBatch):
        ds = self.dataset
        if ds.device is None:
            raise ops._lib.HipLibraryError("pascal_loader: needs a GPU (the HIP path has no CPU fallback)")
        frames, fallbacks = finish_frames(host.frames, ds.device)
        ds.fallback_frames += fallbacks
        if host.masks is not None:      # the maps, their buffer and their offsets come straight from the decode
            maps, fallbacks = finish_annotations(host.masks, ds.device)
            ds.fallback_annotations += fallbacks
            host.mask_dims = host.masks.dims
        else:
            buf = host.mask_buf.to(ds.device, non_blocking=True)
            maps = [buf[o:o + h * w].view(h, w) for o, (h, w) in zip(host.mask_offs, host.mask_dims)]
        S, R, boxes, flips, mean_std, target_float = self.train_size, self.val_size, None, None, (MEAN, STD), True
        if self.transforms is not None:
            if any(tuple(d) != tuple(m) for d, m in zip(host.frames.dims, host.mask_dims)):
                raise ValueError("pair transforms need every mask at its image's size")
            plan = self.transforms(host.frames.dims, self.rng)
            boxes, flips = plan.boxes, plan.flips
            if plan.size is not None:
                S = R = plan.size
            mean_std = None if not plan.to_tensor else (plan.mean_std or ((0., 0., 0.), (1., 1., 1.)))
            target_float = plan.to_tensor
        x = ops.img_resize_ragged(frames, S, boxes, flips, to_tensor=mean_std)
        y = ops.img_gather_nearest_ragged(maps, R, boxes, flips, to_tensor=target_float)
        return x, y

    def __iter__(self):
        order = list(range(len(self.dataset)))
        batches = [order[i:i + self.batch_size] for i in range(0, len(order), self.batch_size)]
        for host in prefetched(batches, self._host, self.dataset.device, self.prefetch):
            yield self._finish(host)


def pascal_loader(batch_size, root, split, val_size, train_size=448, device=None, threads=8, jpeg_entropy="host", png="host") -> VOCLoader:
    """``leoloader.pascal_loader`` (``:241-264``): both of its branches apply the same image and target transforms, so both splits read
    through one path; ``train_transforms`` is built and unused there, and is not used here."""
    dataset = VOCDataset(root=root, image_set=split, return_masks=(split == 'trainaug'), device=device, threads=threads, jpeg_entropy=jpeg_entropy,
                         png=png)
    return VOCLoader(dataset, batch_size, val_size, train_size)


def evaluator_batches(loader):
    """A ``pascal_loader`` as the ``Evaluator`` reads batches: ``(data [b, 1, 1, 3, S, S], integer labels [b, 1, 1, R, R])`` - one clip of one
    frame per image.  ``(y * 255).long()`` rounds back to the PNG's index for all 256 values (pinned by tests/golden/cbfe.npz)."""
    for x, y in loader:
        yield x[:, None, None], (y * 255).long()[:, None]


class EvaluatorLoader:
    """``evaluator_batches`` as a re-iterable with the loader's length."""

    def __init__(self, loader):
        self.loader = loader

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        return evaluator_batches(self.loader)
