"""The reference's ``VideoDataset`` over directories of frames (``data_loader.py:543-767``) with the decode on the device (N21).

A dataset is a frames root ``<root>/<video>/*.jpg`` and an optional annotations root ``<root>/<video>/*.png``.  The two video lists are
sorted and paired by position (``:575-577, 746-752``); inside a video the files are the sorted ``*.jpg``, else the sorted ``*.png``
(``read_clips``, ``:595-599``); ``generate_indices`` makes the reference's ``random`` calls in the reference's order (``:617-642``), so a
run seeded like the reference picks the reference's frames.  ``__getitem__`` returns ``(data, annotations, label)``, and ``read_batch``
ends with the ``(255 * a).uint8`` conversion (``video_transformations.annotations_to_uint8``).

What differs, on purpose:
* JPEG frames are entropy-decoded on the host (``hip_ops.jpeg_scan_batch``: a thread pool over ``tt_jpeg_scan``) and reconstructed on the
  device (``tt_jpeg_decode_batch``), bit-equal to ``Image.open``; the clip a transform receives is ``uint8 [fs, H, W, 3]`` in GPU memory.
  A file ``hip_ops.jpeg_probe`` reports as unsupported (progressive, grayscale, CMYK, ...) - or a frame that is not a JPEG at all - is
  decoded with Pillow on the host and uploaded, and COUNTED (``fallback_frames``).  A supported file that fails to decode raises: the
  fallback never hides a decoder failure.
* Annotation PNGs (mode ``P`` / ``L`` -> indices) become ``uint8 [fs, H, W]`` on the device.  ``png="host"`` (the default): Pillow in the
  loader's thread pool (its decoder releases the GIL), one upload per clip.  ``png="device"`` (N26): the compressed IDAT streams of the whole
  batch cross PCIe once and ``hip_ops.png_decode`` inflates and unfilters them in one launch; a file ``hip_ops.png_probe`` reports as
  unsupported (interlaced, RGB, 16-bit, ...) is decoded with Pillow and COUNTED (``fallback_annotations``), a broken one raises.
* A video's length is the number of its frame files (the reference counts every directory entry, ``:590-592``); its label is its position
  in the sorted list (the reference: its position in ``os.listdir``'s arbitrary order).
* ``frame_transformation`` errors raise (the reference prints "Error in frame transformation" and goes on with the untransformed clip).
* The ``meta.json`` category mapping of ``YVOSDataset`` (``:774-796``, N23) runs on the device, ONCE per batch on the stacked annotations
  (``hip_ops.map_instances``: two launches), not once per sample on the host.  ``compose_instance_lut`` states its rule; by default it is
  the reference's chained in-place loop (``map_instances``, ``:497-506``), ``sequential_category_map=False`` selects the plain
  ``id -> category``.  ``make_categories_dict`` raises ``ValueError`` for a name other than ``"ytvos"`` (the reference: an unbound local),
  and ``num_clips != 1`` with a meta file raises (the reference's loop re-maps the already mapped clip there).
Not reproduced (out of scope): the extraction of video files with cv2 and the ``mkdir`` / ``remove`` it performs (``:509-540``), the
hard-coded per-host dataset roots, ``Kinetics`` and the SBD reader ``pascalVOCLoader`` (Pascal VOC is read by ``leoloader.py``).

``ClipLoader`` stands in for ``make_loader``'s ``DataLoader`` + ``DistributedSampler`` (``:1047-1110``).
"""
from __future__ import annotations

import glob
import io
import json
import os
import random
from concurrent.futures import ThreadPoolExecutor
from contextlib import nullcontext
from enum import Enum
from typing import List, Optional

import numpy as np
import torch

from . import hip_ops as ops
from . import video_transformations as VT


class SamplingMode(Enum):
    UNIFORM = 0
    DENSE = 1
    Full = 2
    Regular = 3


def generate_indices(size: int, sampling_num: int, sampling_mode: SamplingMode, num_clips: int = 1, regular_step: int = 1, rng=random) -> list:
    """``VideoDataset.generate_indices`` (``data_loader.py:617-642``): the same calls on ``rng`` (the ``random`` module or a
    ``random.Random``) in the same order, the same lists / ranges back."""
    indices = []
    for _ in range(num_clips):
        if sampling_mode == SamplingMode.UNIFORM:
            if size < sampling_num:
                idx = rng.choices(range(0, size), k=sampling_num)   # sample repeatedly
            else:
                idx = rng.sample(range(0, size), sampling_num)
            idx.sort()
            indices.append(idx)
        elif sampling_mode == SamplingMode.DENSE:
            base = rng.randint(0, size - sampling_num)
            indices.append(range(base, base + sampling_num))
        elif sampling_mode == SamplingMode.Full:
            indices.append(range(0, size))
        elif sampling_mode == SamplingMode.Regular:
            step = size // sampling_num if size < sampling_num * regular_step else regular_step
            base = rng.randint(0, size - (sampling_num * step))
            indices.append(range(base, base + (sampling_num * step), step))
    return indices


def list_videos(root: str) -> List[str]:
    """The video directories of a root, sorted."""
    return sorted(os.path.join(root, d) for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))


def list_frames(path: str) -> List[str]:
    """``read_clips``' file order: the sorted ``*.jpg``, else the sorted ``*.png``."""
    files = sorted(glob.glob(os.path.join(path, "*.jpg")))
    if len(files) == 0:
        files = sorted(glob.glob(os.path.join(path, "*.png")))
    return files


def decode_annotation(data: bytes) -> np.ndarray:
    """A mode ``P`` / ``L`` image -> its indices, uint8 [H, W]."""
    from PIL import Image

    im = Image.open(io.BytesIO(data))
    if im.mode not in ("P", "L"):
        raise ValueError(f"annotation image of mode {im.mode}: expected a palette (P) or gray (L) label map")
    return np.asarray(im, np.uint8)


def decode_annotations(files, threads: int = 1) -> List[np.ndarray]:
    """``decode_annotation`` of every file, in the pool the file batches use (at most 16 threads; Pillow's decoder releases the GIL): the
    list a serial loop gives."""
    files = list(files)
    return ops._each_file(lambda i: decode_annotation(files[i]), len(files), threads)


def decode_frame_on_host(data: bytes) -> np.ndarray:
    """The counted fallback: Pillow's decode, uint8 [H, W, 3]."""
    from PIL import Image

    return np.array(Image.open(io.BytesIO(data)).convert("RGB"), np.uint8)   # (a writable copy)


maps_as_clip = ops.frames_as_clip     # label maps of one size -> [k, H, W]: one rule for every rank


class HostFiles:
    """The host half of a list of files, frames or annotation maps: ``batch`` - the ``hip_ops.JpegBatch`` / ``PngBatch`` of the files the
    device decoder takes, None without any -, ``device_slots`` their places in the list, ``host_items`` {slot: uint8 [H, W, 3] or [H, W]}
    the Pillow decode of every other file, ``dims`` the (H, W) of every slot and ``n`` their number."""

    def __init__(self, batch, device_slots, host_items, dims):
        self.batch, self.device_slots, self.host_items, self.dims, self.n = batch, device_slots, host_items, dims, len(dims)


def _scan_files(files, probe, fallback, build, threads: int, pin: Optional[bool]) -> HostFiles:
    """Classifies every file (``probe``: its info, None = not this codec's; a broken file raises there), builds the batch of the supported
    ones (``build``) and decodes the others with Pillow (``fallback``).  ``pin`` None: where there is a GPU."""
    device_slots, host_items, dims = [], {}, [None] * len(files)
    for k, data in enumerate(files):
        info = probe(data)
        if info is not None and info.supported:
            device_slots.append(k)
            dims[k] = (info.H, info.W)
        else:
            host_items[k] = fallback(data)
            dims[k] = host_items[k].shape[:2]
    pin = torch.cuda.is_available() if pin is None else pin
    return HostFiles(build([files[k] for k in device_slots], threads, pin) if device_slots else None, device_slots, host_items, dims)


def _finish_files(host: HostFiles, decode, device):
    """(every file as a tensor on ``device`` in file order - ``decode(batch, device)`` of the batch, an upload of the others -, the number
    of files Pillow decoded: the fall-backs a loader counts)"""
    items = [None] * host.n
    if host.batch is not None:
        for k, t in zip(host.device_slots, decode(host.batch, device)):
            items[k] = t
    for k, arr in host.host_items.items():
        items[k] = torch.from_numpy(arr if arr.flags.writeable else arr.copy()).to(device)     # (Pillow's label maps are read-only)
    return items, len(host.host_items)


def scan_frames(files, threads: int, entropy: str = "host", pin: Optional[bool] = None) -> HostFiles:
    """Classifies every file and builds the batch of the supported ones on the ``entropy`` route ("host": ``hip_ops.jpeg_scan_batch``,
    "device": ``jpeg_prepare_batch``); an unsupported file or one that is not a JPEG is decoded with Pillow.  A broken JPEG raises
    ``ValueError``.  No GPU call: a background thread may run it."""
    return _scan_files(files, lambda data: ops.jpeg_probe(data) if data[:2] == b"\xff\xd8" else None, decode_frame_on_host,
                       ops.jpeg_prepare_batch if entropy == "device" else ops.jpeg_scan_batch, threads, pin)


def finish_frames(host: HostFiles, device):
    """The device half of ``scan_frames``: (the frames as uint8 [H, W, 3] tensors on ``device`` in file order, the number of them that
    Pillow decoded)."""
    return _finish_files(host, ops.jpeg_decode, device)


def scan_annotations(files, threads: int, pin: Optional[bool] = None) -> HostFiles:
    """Classifies every annotation file and prepares the supported ones (``hip_ops.png_prepare_batch``); an unsupported file is decoded
    with Pillow.  A broken PNG raises ``ValueError``.  No GPU call: a background thread may run it."""
    return _scan_files(files, ops.png_probe, decode_annotation, ops.png_prepare_batch, threads, pin)


def finish_annotations(host: HostFiles, device):
    """The device half of ``scan_annotations``: (the maps as uint8 [H, W] tensors on ``device`` in file order - the device-decoded ones
    views of ONE flat buffer, consecutive files one after the other -, the number of maps Pillow decoded).  A non-zero status raises,
    naming the file."""
    return _finish_files(host, lambda batch, dev: ops.png_decode(batch, dev)[0], device)


def _route(name: str, value, optional: bool = False):
    """``value`` where it names a decode route ("host" / "device"; None too where ``optional``), else ValueError naming the argument."""
    if value not in ("host", "device") and not (optional and value is None):
        raise ValueError(f"{name} must be 'host' or 'device', not {value!r}")
    return value


def prefetched(batches, host, device=None, prefetch: bool = True):
    """``host(indices)`` of every index batch, in order.  With ``prefetch`` a background thread works on batch k + 1 while the caller has
    batch k.  ``host`` runs under ``torch.cuda.device(device)`` where that is a GPU: a new thread starts on device 0, and the pinned
    buffers belong to the loader's device."""
    on_gpu = device is not None and torch.device(device).type == "cuda"

    def run(indices):
        with torch.cuda.device(device) if on_gpu else nullcontext():
            return host(indices)

    if not (prefetch and batches):
        yield from map(run, batches)
        return
    pool = ThreadPoolExecutor(1, thread_name_prefix="tt_prefetch")
    try:
        pending = pool.submit(run, batches[0])
        for k in range(len(batches)):
            item = pending.result()
            if k + 1 < len(batches):
                pending = pool.submit(run, batches[k + 1])
            yield item
    finally:
        pool.shutdown(wait=True)


def add_decode_arguments(parser, jpeg: bool = True, png: bool = True) -> None:
    """The drivers' ``--jpeg_entropy`` and ``--png_decode``."""
    if jpeg:
        parser.add_argument("--jpeg_entropy", choices=["host", "device"], default="host",
                            help="where the frames' Huffman coding is undone: in the host thread pool, or on the device from the compressed scans (N24)")
    if png:
        parser.add_argument("--png_decode", choices=["host", "device"], default="host",
                            help="where the annotation PNGs are inflated: Pillow in the host thread pool, or on the device from the IDAT streams (N26)")


def make_categories_dict(meta_dict, name):
    """``make_categories_dict`` (``data_loader.py:453-464``): the categories of every object of every video, sorted, numbered from 1 -
    0 stays the background.  Only ``name == "ytvos"`` is defined (the reference falls into an unbound local for any other)."""
    if name != "ytvos":
        raise ValueError(f"make_categories_dict: only the \"ytvos\" meta layout is defined, got {name!r}")
    categories = {obj["category"] for video in meta_dict["videos"].values() for obj in video["objects"].values()}
    return {k: v + 1 for v, k in enumerate(sorted(categories))}


def video_category_table(meta_dict, category_dict, video: str) -> np.ndarray:
    """int32 [256]: the category id of each object id of ``meta["videos"][video]["objects"]``, -1 where the meta file has none (a video
    the file does not list has none at all)."""
    table = np.full(256, -1, np.int32)
    entry = meta_dict["videos"].get(video)
    for key, obj in ({} if entry is None else entry["objects"]).items():
        if not 0 <= int(key) <= 255:
            raise ValueError(f"video {video}: object id {key} does not fit a uint8 annotation map")
        table[int(key)] = category_dict[obj["category"]]
    if table.max() > 255:
        raise ValueError(f"{len(category_dict)} categories do not fit a uint8 annotation map")
    return table


def compose_instance_lut(present, cat, sequential: bool = True) -> np.ndarray:
    """The 256-entry table ``tt_map_instances`` applies to one segment (uint8 [256]); the host statement of the kernel's rule.
    ``present``: the values that occur in the ORIGINAL segment (any iterable of ints, or a bool [256] array); ``cat``: int [256], the
    category of each object id, -1 = none.

    ``sequential``: the reference's ``map_instances`` - ``frame[frame == obj] = category`` in place, for obj over the ascending
    ``torch.unique`` of the clip taken BEFORE the loop.  From the identity, for obj = 1 .. 255 in order, if obj is present every entry
    whose CURRENT value equals obj becomes ``cat[obj]``; a pixel mapped onto a later, present object id is mapped again.  Otherwise the
    plain ``v -> cat[v]`` for present v >= 1.  0 is never remapped.  Raises ``KeyError(obj)`` for the smallest present object without a
    category in 0 .. 255 (the kernel: ``status`` = obj and the identity)."""
    cat = np.asarray(cat).astype(np.int64)
    flags = np.asarray(present)
    if flags.dtype != np.bool_ or flags.shape != (256,):
        flags = np.zeros(256, np.bool_)
        flags[np.asarray(list(present), np.int64)] = True
    objs = [v for v in range(1, 256) if flags[v]]
    for obj in objs:
        if not 0 <= cat[obj] <= 255:
            raise KeyError(obj)
    lut = np.arange(256, dtype=np.int64)
    for obj in objs:
        if sequential:
            lut[lut == obj] = cat[obj]
        else:
            lut[obj] = cat[obj]
    return lut.astype(np.uint8)


def _read(path: str) -> bytes:
    with open(path, "rb") as f:
        return f.read()


class _HostSample:
    """One video's clips as the host leaves them: the frame files' bytes and the decoded annotation maps, per clip."""

    def __init__(self, frames, annotations, label, index=None, annotation_files=None):
        self.frames, self.annotations, self.label, self.index = frames, annotations, label, index
        self.annotation_files = annotation_files      # png="device": the files' bytes per clip, and ``annotations`` is None


class _HostBatch:
    def __init__(self, samples, frames: HostFiles, annotations: Optional[HostFiles] = None):
        self.samples, self.frames, self.annotations = samples, frames, annotations


class VideoDataset:
    """``VideoDataset(classes_directory, annotations_directory, sampling_mode, num_clips, num_frames, ...)`` (``:552``).  ``rng`` draws the
    frame indices (default: the ``random`` module, as in the reference); ``device`` and ``threads`` belong to the decode, and so does
    ``jpeg_entropy``: "host" undoes the Huffman coding in the thread pool (``hip_ops.jpeg_scan_batch``), "device" copies the compressed
    scans and undoes it in one launch (``hip_ops.jpeg_prepare_batch``) - the same pixels either way.  ``png``: "host" decodes the
    annotation PNGs with Pillow in the thread pool, "device" inflates and unfilters them in one launch per batch
    (``hip_ops.png_decode``) - the same maps either way.
    ``meta_file_directory`` (``:563-573``): the path of a YouTube-VOS ``meta.json``; when the file exists the annotations' per-video
    instance ids become dataset-wide category ids (``map_categories``), ``sequential_category_map`` choosing the rule of
    ``compose_instance_lut``.  A path that does not exist prints "There is no meta file." and maps nothing, as in the reference."""

    def __init__(self, classes_directory, annotations_directory, sampling_mode, num_clips, num_frames, num_labels=1, frame_transform=None,
                 target_transform=None, video_transform=None, meta_file_directory=None, regular_step=1, device=None, threads=8, rng=None,
                 sequential_category_map=True, jpeg_entropy="host", png="host"):
        self.jpeg_entropy, self.png = _route("jpeg_entropy", jpeg_entropy), _route("png", png)
        if num_labels != 1:
            raise NotImplementedError("nested class directories (num_labels > 1) are not reproduced")
        self.meta_dict, self.category_dict, self.category_tables = None, None, None
        self.sequential_category_map = bool(sequential_category_map)
        if meta_file_directory is not None:
            if os.path.exists(meta_file_directory):
                if num_clips != 1:
                    raise NotImplementedError("the meta.json category mapping with num_clips != 1: the reference's loop maps the already "
                                              "mapped clip again there, and make_loader never asks for it")
                with open(meta_file_directory) as f:
                    self.meta_dict = json.load(f)
                self.category_dict = make_categories_dict(self.meta_dict, "ytvos")
            else:
                print("There is no meta file.")
        self.keys = list_videos(classes_directory)
        if len(self.keys) == 0:
            raise FileNotFoundError(f"no video directories under {classes_directory}")
        self.train_dict = {k: np.array([i]) for i, k in enumerate(self.keys)}
        if self.meta_dict is not None:   # one int32 [256] table per video, by the directory's name
            self.category_tables = np.stack([video_category_table(self.meta_dict, self.category_dict, os.path.basename(k)) for k in self.keys])
        self.files = {k: list_frames(k) for k in self.keys}
        self.train_dict_lenghts = {k: len(v) for k, v in self.files.items()}
        if annotations_directory and os.path.exists(annotations_directory):
            self.annotation_keys = list_videos(annotations_directory)
            if len(self.annotation_keys) != len(self.keys):
                raise ValueError(f"{len(self.keys)} videos but {len(self.annotation_keys)} annotation directories: they are paired by position")
            self.annotation_files = {k: list_frames(k) for k in self.annotation_keys}
            self.use_annotations = True
        else:
            self.use_annotations = False
        self.sampling_mode, self.num_clips, self.num_frames, self.regular_step = sampling_mode, num_clips, num_frames, regular_step
        self.frame_transform, self.target_transform, self.video_transform = frame_transform, target_transform, video_transform
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None and torch.cuda.is_available() else device
        self.threads = int(threads)
        self.rng = random if rng is None else rng
        self.fallback_frames = 0
        self.fallback_annotations = 0

    def __len__(self):
        return len(self.keys)

    def generate_indices(self, size, sampling_num, rng=None):
        return generate_indices(size, sampling_num, self.sampling_mode, self.num_clips, self.regular_step, self.rng if rng is None else rng)

    # ---- host half: index draws, file reads, annotation decode (no GPU call: a background thread may run it)
    def read_host(self, idx: int, rng=None, png: Optional[str] = None, decode: bool = True) -> _HostSample:
        """The index draws and file reads of one video.  Its annotation files are decoded here on the "host" route (in the thread pool)
        unless ``decode`` is False: a loader leaves them as bytes for ``scan_host``, which pools over the whole BATCH."""
        path = self.keys[idx]
        clip_indices = self.generate_indices(self.train_dict_lenghts[path], self.num_frames, rng)
        files = self.files[path]
        frames = [[_read(files[j]) for j in clip] for clip in clip_indices]
        annotations, raw = None, None
        if self.use_annotations:
            afiles = self.annotation_files[self.annotation_keys[idx]]
            raw = [[_read(afiles[j]) for j in clip] for clip in clip_indices]
            if (png or self.png) == "host" and decode:
                decoded = iter(decode_annotations([f for clip in raw for f in clip], self.threads))
                annotations, raw = [np.stack([next(decoded) for _ in clip]) for clip in raw], None
        return _HostSample(frames, annotations, np.tile(self.train_dict[path], (self.num_clips,)), idx, raw)

    def scan_host(self, samples: List[_HostSample], jpeg_entropy: Optional[str] = None, png: Optional[str] = None) -> _HostBatch:
        """Classifies every frame of the samples, entropy-decodes the supported ones into one pinned buffer and decodes the others with
        Pillow.  The annotation files the samples still carry as bytes are, on the "host" route, decoded in the thread pool - all files
        of the batch in one go - and on the "device" route prepared for ONE device decode."""
        flat = [f for s in samples for clip in s.frames for f in clip]
        pending = [s for s in samples if s.annotation_files is not None]
        if pending and (png or self.png) == "host":
            decoded = iter(decode_annotations([f for s in pending for clip in s.annotation_files for f in clip], self.threads))
            for s in pending:
                s.annotations, s.annotation_files = [np.stack([next(decoded) for _ in clip]) for clip in s.annotation_files], None
        ann = [f for s in samples if s.annotation_files is not None for clip in s.annotation_files for f in clip]
        return _HostBatch(samples, scan_frames(flat, self.threads, jpeg_entropy or self.jpeg_entropy),    # a loader may choose for itself
                          scan_annotations(ann, self.threads) if ann else None)

    # ---- device half: reconstruction, transforms
    def finish(self, batch: _HostBatch):
        """-> per sample (data, annotations, label) as ``__getitem__`` returns them."""
        flat, fallbacks = finish_frames(batch.frames, self.device)
        self.fallback_frames += fallbacks
        maps = []
        if batch.annotations is not None:
            maps, fallbacks = finish_annotations(batch.annotations, self.device)
            self.fallback_annotations += fallbacks
        flat, maps, out = iter(flat), iter(maps), []
        for s in batch.samples:     # the files of the batch in the order scan_host listed them: sample by sample, clip by clip
            clips = [ops.frames_as_clip([next(flat) for _ in clip]) for clip in s.frames]
            ann = None if s.annotations is None else [torch.from_numpy(a).to(self.device) for a in s.annotations]
            if s.annotation_files is not None:
                ann = [maps_as_clip([next(maps) for _ in clip]) for clip in s.annotation_files]
            out.append(self._transform(clips, ann) + (torch.Tensor(s.label),))
        return out

    def _transform(self, clips, annotations):
        """``read_batch`` behind the file reads (``:653-680``)."""
        anns = [] if annotations is None else list(annotations)
        if anns and self.target_transform is not None:
            anns = [self.target_transform(a) for a in anns]
        if self.frame_transform is not None:
            clips = [self.frame_transform(c) for c in clips]
        if self.video_transform is not None:
            for i in range(len(clips)):
                if anns:
                    clips[i], anns[i] = self.video_transform(clips[i], anns[i])
                else:
                    clips[i] = self.video_transform(clips[i])
        data = torch.stack(clips)
        if anns:
            stacked = torch.stack(anns)
            sampled = VT.annotations_to_uint8(stacked) if stacked.is_floating_point() else stacked
        else:
            sampled = torch.empty(0)
        return data, sampled

    def map_categories(self, annotations: torch.Tensor, indices) -> torch.Tensor:
        """annotations uint8 [n, ...] of the videos ``indices`` (one clip each) -> the same with instance ids replaced by category ids:
        ONE ``hip_ops.map_instances`` call for all n clips, each with its video's table.  Without a meta file, or without annotations,
        the tensor comes back as it is.  A present object id the meta file does not list raises ``KeyError`` naming the video and the
        id (the reference raises ``KeyError`` there too)."""
        if self.category_tables is None or annotations.numel() == 0:
            return annotations
        if annotations.dtype != torch.uint8:
            raise TypeError(f"the category mapping reads uint8 annotation maps, got {annotations.dtype}")
        n = len(indices)
        cat = torch.from_numpy(self.category_tables[np.asarray(indices, np.int64)]).to(annotations.device)
        mapped, _, status = ops.map_instances(annotations.contiguous().view(n, -1), cat, self.sequential_category_map)
        status = status.cpu()
        for k in range(n):
            if int(status[k]) != 0:
                raise KeyError(f"video {os.path.basename(self.keys[indices[k]])}: object id {int(status[k])} is not in the meta file")
        return mapped.view(annotations.shape)

    def __getitem__(self, idx):
        """(data [num_clips, fs, 3, R, R], annotations uint8 [num_clips, fs, R, R] or an empty tensor, label [num_clips])."""
        data, annotations, label = self.finish(self.scan_host([self.read_host(idx)]))[0]
        return data, self.map_categories(annotations, [idx]), label


class YVOSDataset(VideoDataset):
    """``YVOSDataset`` (``:774-796``): a ``VideoDataset`` whose ``meta_file_directory`` must hold a readable YouTube-VOS ``meta.json``
    (the reference fails on ``None["videos"]`` without one)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if self.meta_dict is None:
            raise FileNotFoundError("YVOSDataset needs meta_file_directory, the path of an existing meta.json")


class ClipLoader:
    """``make_loader``'s ``DataLoader`` (+ ``DistributedSampler`` when ``world_size`` > 1): yields ``(data [bs, num_clips, fs, 3, R, R] float32,
    annotations, label)`` on the device.  Per batch: the files' bytes are read and all ``bs * num_clips * fs`` frames entropy-decoded in the
    thread pool, ONE ``tt_jpeg_decode_batch`` call reconstructs them, and the GPU transforms run per clip.  A background thread prepares
    the host half of batch i + 1 while the caller works on batch i; it draws the frame indices from the loader's own ``random.Random``
    (``seed``), so the transforms' draws from the ``random`` module on the caller's thread are not disturbed.  The last batch may be short
    (``drop_last=False``, the DataLoader default)."""

    def __init__(self, dataset: VideoDataset, batch_size: int, shuffle: bool = False, world_size: int = 1, rank: int = 0, seed: int = 0,
                 prefetch: bool = True, jpeg_entropy: Optional[str] = None, png: Optional[str] = None):
        self.jpeg_entropy = _route("jpeg_entropy", jpeg_entropy, optional=True) or dataset.jpeg_entropy   # the loader's own: the dataset is not touched
        self.png = _route("png", png, optional=True) or dataset.png
        self.dataset, self.batch_size, self.shuffle, self.world_size, self.rank, self.seed = dataset, int(batch_size), shuffle, world_size, rank, seed
        self.prefetch, self.epoch = prefetch, 0
        self.rng = random.Random(seed * 1000003 + rank)

    @property
    def fallback_frames(self) -> int:
        return self.dataset.fallback_frames

    @property
    def fallback_annotations(self) -> int:
        return self.dataset.fallback_annotations

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def _order(self) -> List[int]:
        n = len(self.dataset)
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            order = torch.randperm(n, generator=g).tolist()
        else:
            order = list(range(n))
        if self.world_size > 1:   # DistributedSampler: pad to a multiple of world_size with the head of the list, then every world_size-th
            total = -(-n // self.world_size) * self.world_size
            order = (order * (total // n + 1))[:total]
            order = order[self.rank:total:self.world_size]
        return order

    def __len__(self):
        n = len(self.dataset)
        local = -(-n // self.world_size) if self.world_size > 1 else n
        return -(-local // self.batch_size)

    def _host(self, indices) -> _HostBatch:
        return self.dataset.scan_host([self.dataset.read_host(i, self.rng, self.png, decode=False) for i in indices], self.jpeg_entropy, self.png)

    def __iter__(self):
        order = self._order()
        batches = [order[i:i + self.batch_size] for i in range(0, len(order), self.batch_size)]
        for host in prefetched(batches, self._host, self.dataset.device, self.prefetch):
            items = self.dataset.finish(host)
            data = torch.stack([d for d, _, _ in items])
            annotations = self.dataset.map_categories(torch.stack([a for _, a, _ in items]), [s.index for s in host.samples])
            label = torch.stack([l for _, _, l in items])
            yield data, annotations, label


def make_loader(dataset_path: str, num_clip_frames: int, batch_size: int, regular_step: int = 1, sampling_mode: SamplingMode = SamplingMode.UNIFORM,
                frame_transform=None, target_transform=None, video_transform=None, shuffle: bool = False, num_workers: int = 6, world_size: int = 1,
                rank: int = 0, device=None, seed: int = 0, meta_file_directory=None, sequential_category_map: bool = True,
                jpeg_entropy: str = "host", png: str = "host") -> ClipLoader:
    """``make_loader`` (``:1047``) for the layout every ``VideoDataset`` branch of it reads: frames under ``<dataset_path>/JPEGImages/``,
    annotations under ``<dataset_path>/Annotations/`` when present.  ``num_workers`` is the thread count of the host decode (at most 16
    are used); ``jpeg_entropy`` "host" / "device": where the frames' Huffman coding is undone, ``png`` "host" /
    "device": where the annotation PNGs are inflated (``VideoDataset``).  ``meta_file_directory``: the path of a YouTube-VOS ``meta.json`` - a ``YVOSDataset`` then maps instance ids to category
    ids (the ``ytvos`` branches, ``:1073-1090``).  It is never looked for: without the argument a tree that holds one is read as before."""
    frames = os.path.join(dataset_path, "JPEGImages")
    if not os.path.isdir(frames):
        # (the reference maps a dataset NAME to a hard-coded root and a layout of its own per name, :1055-1104: not reproduced)
        raise NotImplementedError(f"dataset readers: only the layout <dataset_path>/JPEGImages/<video>/*.jpg (+ <dataset_path>/Annotations/"
                                  f"<video>/*.png) is read, and {frames} is not a directory; point --dataset_path at such a tree, or run "
                                  "with --dataset synthetic / synthetic_frames")
    cls = VideoDataset if meta_file_directory is None else YVOSDataset
    dataset = cls(frames, os.path.join(dataset_path, "Annotations"), sampling_mode, 1, num_clip_frames, 1, frame_transform,
                  target_transform, video_transform, meta_file_directory=meta_file_directory, regular_step=regular_step, device=device,
                  threads=num_workers, sequential_category_map=sequential_category_map, jpeg_entropy=jpeg_entropy, png=png)
    return ClipLoader(dataset, batch_size, shuffle=shuffle, world_size=world_size, rank=rank, seed=seed)
