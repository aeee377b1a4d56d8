"""The clip transforms of the reference (``video_transformations.py``) on GPU-resident frames.

Same class names, constructor arguments, defaults and - deliberately - the same random-number calls in the same order
(``random.random`` / ``random.uniform`` / ``random.randint`` / ``random.shuffle`` / ``torch.rand``), so that a run seeded like
the reference takes the same decisions and, because every kernel reproduces Pillow's arithmetic, produces the same tensors.
A data clip is a ``torch.uint8`` tensor ``[fs, H, W, 3]`` on the device (what a video decoder hands over) instead of a list of
PIL images; an annotation clip is ``torch.uint8 [fs, H, W]`` (what a mode ``L`` / ``P`` PNG decodes to).  ``ClipToTensor`` ends
the chain with ``float32 [fs, 3, H, W]`` (and ``[fs, 1, H, W] = v / 255`` for the annotations) exactly as the reference does.

Annotation clips only ever meet nearest-neighbour gathering (crop, Pillow's NEAREST resize, the two flips), so a ``Compose``
called with a pair keeps ONE pair of index tables per clip, folds every such step into them on the host and launches one
gather where the chain ends (``ClipToTensor`` writes the float plane in that launch).  The data clip of a pair keeps the two
bilinear resampling launches; crops and flips behind them fold into tables the same way, and an untouched or merely mirrored
resize hands ``ClipToTensor`` to the vertical pass as the training chain does.  Fused and step-by-step calls give equal bits.

Reference quirks that are reproduced (and worth knowing):
* ``ColorJitter`` builds four adjustment closures, shuffles them, and then applies EACH to the ORIGINAL image, keeping only
  the last result (``video_transformations.py:774-777``): one randomly chosen adjustment takes effect, not a chain of four.
* ``RandomHorizontalFlip`` without annotations calls its helper with the default ``chance=0.5``, and ``0.5 < p`` is False
  for the default ``p=0.5`` (``:168-170,190-193``): training clips are never flipped and no random number is drawn.  WITH
  annotations it draws ``random.random()`` once and flips both clips when ``chance < p`` (``:189-191``).
* ``RandomVerticalFlip`` without annotations calls its helper without ``chance`` and raises ``TypeError`` (``:234``).
* ``RandomResize`` hands ``(new_w, new_h)`` to ``resize_clip``, which swaps a tuple again (``:85,344-348``): the result has
  ``int(im_w * s)`` ROWS and ``int(im_h * s)`` COLUMNS.
* ``RandomGaussianBlur`` draws a fresh radius per frame inside the list comprehension (``:640``).
* ``RandomGrayscale`` draws from torch's generator, everything else from Python's ``random``.
* ``CenterCrop`` rounds its origin with Python's round-half-even (``:596-597``).
Not built: the numpy-array (cv2 / skimage) code paths, ``Normalize`` (its PIL branch returns nothing usable), bilinear resizing
of annotation clips.  The files are read and decoded by ``data_loader.py``.
"""
from __future__ import annotations

import math
import numbers
import random
from functools import lru_cache

import numpy as np
import torch

from . import hip_ops as ops

PRECISION_BITS = 32 - 8 - 2


@lru_cache(maxsize=4096)
def resample_coeffs(in_size: int, out_size: int):
    """Pillow's bilinear taps for resizing a line of ``in_size`` pixels to ``out_size`` (Resample.c precompute_coeffs +
    normalize_coeffs_8bpc): (int32 [out_size, ksize], int32 [out_size, 2] = first input index and tap count) as CPU tensors.
    Vectorised over the output positions; every float64 operation and the left-to-right tap sum are the C loop's."""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    cnt = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    a = np.abs((x + xmin[:, None] - center[:, None] + 0.5) * ss)
    w = np.where((a < 1.0) & (x < cnt[:, None]), 1.0 - a, 0.0)
    ww = np.zeros(out_size, np.float64)
    for t in range(ksize):  # sequential sum, as the C loop
        ww = ww + w[:, t]
    v = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    kk = np.trunc(0.5 + v * (1 << PRECISION_BITS)).astype(np.int32)
    kk = np.where(x < cnt[:, None], kk, 0).astype(np.int32)
    bounds = np.stack([xmin, cnt], axis=1).astype(np.int32)
    return torch.from_numpy(np.ascontiguousarray(kk)), torch.from_numpy(np.ascontiguousarray(bounds))


_DEVICE_COEFFS: dict = {}


def _coeffs_on(device, in_size, out_size):
    key = (str(device), in_size, out_size)
    hit = _DEVICE_COEFFS.get(key)
    if hit is None:
        if len(_DEVICE_COEFFS) > 4096:
            _DEVICE_COEFFS.clear()
        kk, bounds = resample_coeffs(in_size, out_size)
        hit = _DEVICE_COEFFS[key] = (kk.to(device), bounds.to(device))
    return hit


def resized_crop(clip: torch.Tensor, i: int, j: int, h: int, w: int, size, to_tensor=None, flip: bool = False) -> torch.Tensor:
    """``img.crop((j, i, j + w, i + h)).resize((size[1], size[0]), BILINEAR)`` for every frame; with ``to_tensor=(mean, std)`` the
    result leaves as the normalised float tensor (optionally flipped) in the same launch."""
    OH, OW = size
    dev = clip.device
    x = clip
    y0 = i
    if OW != w:
        kk, bounds = _coeffs_on(dev, w, OW)
        x = ops.img_resample_h(x, kk, bounds, i, j, h)          # rows i..i+h only, columns j..j+w
        y0 = 0
    elif j != 0 or w != clip.shape[2]:
        x = x[:, :, j:j + w].contiguous()
    if OH != h or to_tensor is not None or y0 != 0 or x.shape[1] != h:
        kk, bounds = _coeffs_on(dev, h, OH)                      # (identity taps when OH == h)
        return ops.img_resample_v(x, kk, bounds, y0, to_tensor, flip)
    return x


@lru_cache(maxsize=4096)
def _pillow_nearest(n_in: int, n_out: int) -> np.ndarray:
    a0 = n_in / n_out
    xo = a0 * 0.5
    tab = np.empty(n_out, np.int32)
    for x in range(n_out):  # a running double sum, as the C loop: a product per position rounds differently
        tab[x] = int(xo)
        xo += a0
    if tab[-1] >= n_in:
        raise ValueError(f"resizing {n_in} -> {n_out}: the running sum leaves the line (Pillow would leave such pixels unset)")
    tab.setflags(write=False)
    return tab


def nearest_table(n_in: int, n_out: int, offset: int = 0, flip: bool = False) -> np.ndarray:
    """Source index of every output position of ``Image.resize(NEAREST)`` for a line of ``n_in`` pixels that starts at
    ``offset`` of a longer line (``crop`` first) and is resized to ``n_out`` (Geometry.c ImagingScaleAffine: ``xo = a0 / 2``, then
    ``tab[x] = floor(xo); xo += a0`` in double); ``flip`` reverses the table (``transpose(FLIP_*)`` afterwards).  int32 [n_out]."""
    if n_in <= 0 or n_out <= 0 or offset < 0:
        raise ValueError(f"nearest_table: n_in {n_in}, n_out {n_out}, offset {offset}")
    tab = _pillow_nearest(int(n_in), int(n_out)) + np.int32(offset)
    return np.ascontiguousarray(tab[::-1]) if flip else tab


def rotate_coeffs(w: int, h: int, angle: float):
    """The six 16.16 fixed-point integers (a0 .. a5) of ``Image.rotate(angle)`` with its defaults (NEAREST, no expand, centre
    ``(w / 2, h / 2)``, fill 0) on a ``w`` x ``h`` image: Image.py's matrix, then Geometry.c's ``FIX(v) = floor(v * 65536 + 0.5)``
    with the half-pixel shift folded into a2 / a5."""
    angle = angle % 360.0
    r = -math.radians(angle)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    cx, cy = w / 2, h / 2
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy

    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))

    return (fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


def _crop_check(im_h, im_w, h, w, word):
    if w > im_w or h > im_h:
        raise ValueError(f"Initial image size should be larger {word} cropped size but got cropped sizes : ({w}, {h}) while "
                         f"initial image is ({im_w}, {im_h})")


def center_crop_origin(im_h: int, im_w: int, h: int, w: int):
    """(y1, x1) of ``CenterCrop`` (``:596-597``; Python's ``round`` is half-to-even)."""
    _crop_check(im_h, im_w, h, w, "than")
    return int(round((im_h - h) / 2.)), int(round((im_w - w) / 2.))


def random_crop_origin(im_h: int, im_w: int, h: int, w: int):
    """(y1, x1) of ``RandomCrop`` (``:410-411``): ``randint`` for x1 first, then for y1."""
    _crop_check(im_h, im_w, h, w, "then")
    x1 = random.randint(0, im_w - w)
    y1 = random.randint(0, im_h - h)
    return y1, x1


def gather_clip(clip: torch.Tensor, ytab, xtab, to_tensor=None) -> torch.Tensor:
    """``clip[:, ytab][:, :, xtab]`` in one launch for a data clip [fs, H, W, 3] or an annotation clip [fs, H, W]; with
    ``to_tensor`` (``(mean, std)`` for data, ``True`` for annotations) the result leaves as ``ClipToTensor``'s float tensor."""
    return ops.img_gather_nearest(clip, ytab, xtab, to_tensor)


def rotate_clip(clip: torch.Tensor, angle: float) -> torch.Tensor:
    """``img.rotate(angle)`` for every frame of either kind of clip."""
    return ops.img_affine_nearest(clip, rotate_coeffs(clip.shape[2], clip.shape[1], angle))


class _Lazy:
    """A clip on its way through a chain: ``src``, then (optionally) a pending bilinear ``crop + resize`` of it, then
    (optionally) index tables over that.  ``shape`` is what a materialised tensor would have."""

    def __init__(self, src: torch.Tensor):
        self.src, self.resize, self.yt, self.xt = src, None, None, None

    @property
    def is_annotation(self):
        return self.src.dim() == 3

    @property
    def shape(self):
        F_, H, W = self.src.shape[:3]
        if self.resize is not None:
            H, W = self.resize[4]
        if self.yt is not None:
            H, W = len(self.yt), len(self.xt)
        return (F_, H, W) if self.is_annotation else (F_, H, W, 3)

    def gather(self, ytab, xtab):
        """Index the (virtual) clip with two tables over its current rows and columns."""
        _, H, W = self.shape[:3]
        if self.yt is None:
            if len(ytab) == H and len(xtab) == W and np.array_equal(ytab, np.arange(H)) and np.array_equal(xtab, np.arange(W)):
                return self
            self.yt, self.xt = np.asarray(ytab, np.int32), np.asarray(xtab, np.int32)
        else:
            self.yt, self.xt = self.yt[np.asarray(ytab)], self.xt[np.asarray(xtab)]
        return self

    def resized_crop(self, i, j, h, w, size):
        """``crop((j, i, j + w, i + h)).resize(size)``: bilinear for a data clip, nearest for an annotation clip."""
        if self.is_annotation:
            return self.gather(nearest_table(h, size[0], i), nearest_table(w, size[1], j))
        self.src, self.yt, self.xt = self.materialize(), None, None
        self.resize = (i, j, h, w, (int(size[0]), int(size[1])))
        return self

    def materialize(self, to_tensor=None):
        src = self.src
        if self.resize is not None:
            i, j, h, w, size = self.resize
            mirrored = self.yt is not None and np.array_equal(self.yt, np.arange(size[0])) and \
                np.array_equal(self.xt, np.arange(size[1])[::-1])
            if self.yt is None or (mirrored and to_tensor is not None):
                return resized_crop(src, i, j, h, w, size, to_tensor=to_tensor, flip=self.yt is not None)
            src = resized_crop(src, i, j, h, w, size)
        if self.yt is not None:
            return ops.img_gather_nearest(src, self.yt, self.xt, to_tensor)
        if to_tensor is None:
            return src
        _, H, W = src.shape[:3]
        if self.is_annotation:
            return ops.img_gather_nearest(src, np.arange(H, dtype=np.int32), np.arange(W, dtype=np.int32), True)
        return resized_crop(src, 0, 0, H, W, (H, W), to_tensor=to_tensor)


def _lazy(clip):
    return clip if isinstance(clip, _Lazy) else _Lazy(clip)


def _pair(transform, data_clip, annotation_clip):
    """Run a transform's table form on a pair; tensors in -> tensors out, lazy clips (inside a Compose) stay lazy."""
    inside = isinstance(data_clip, _Lazy)
    d, a = transform._apply(_lazy(data_clip), _lazy(annotation_clip))
    return (d, a) if inside else (d.materialize(), a.materialize())


def get_resize_sizes(im_h, im_w, size):
    if im_w < im_h:
        return int(size * im_h / im_w), size
    return size, int(size * im_w / im_h)


def _resize_target(im_h, im_w, size):
    """(new_h, new_w) of ``resize_clip`` (:76-85), or None for its early return."""
    if isinstance(size, numbers.Number):
        if (im_w <= im_h and im_w == size) or (im_h <= im_w and im_h == size):
            return None
        return get_resize_sizes(im_h, im_w, size)
    return size[0], size[1]


def resize_clip(clip: torch.Tensor, size, interpolation="bilinear") -> torch.Tensor:
    """``video_transformations.resize_clip`` (:56-94) for PIL clips: a number resizes the SHORTER side, keeping the aspect.
    ``'nearest'`` (Pillow's NEAREST) works for data and annotation clips, ``'bilinear'`` for data clips."""
    if interpolation not in ("bilinear", "nearest"):
        raise NotImplementedError("only bilinear and nearest resizing are built")
    if interpolation == "bilinear" and clip.dim() == 3:
        raise NotImplementedError("bilinear resizing of annotation clips is not built: label maps are gathered, never blended")
    im_h, im_w = clip.shape[1], clip.shape[2]
    target = _resize_target(im_h, im_w, size)
    if target is None:
        return clip
    new_h, new_w = target
    if interpolation == "nearest":
        return gather_clip(clip, nearest_table(im_h, new_h), nearest_table(im_w, new_w))
    return resized_crop(clip, 0, 0, im_h, im_w, (new_h, new_w))


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, data_clip, annotation_clip=None):
        if annotation_clip is not None:
            return self._call_pair(data_clip, annotation_clip)
        ts = self.transforms
        k = 0
        while k < len(ts):
            # RandomResizedCrop [-> RandomHorizontalFlip] -> ClipToTensor: the crop's vertical resampling pass writes the
            # normalised float tensor directly (same arithmetic, same random draws, one launch and one uint8 round trip less)
            if isinstance(ts[k], RandomResizedCrop):
                nxt = k + 1
                flipper = ts[nxt] if nxt < len(ts) and isinstance(ts[nxt], RandomHorizontalFlip) else None
                nxt += flipper is not None
                if nxt < len(ts) and isinstance(ts[nxt], ClipToTensor):
                    data_clip = ts[k](data_clip, _finish=(flipper, ts[nxt]))
                    k = nxt + 1
                    continue
            data_clip = ts[k](data_clip)
            k += 1
        return data_clip

    def _call_pair(self, data_clip, annotation_clip):
        """``for t in transforms: data, ann = t(data, ann)`` (:155-157) with the clips kept lazy between the steps that can fold:
        every draw happens where the reference makes it, the launches happen where a step needs pixels or the chain ends."""
        d, a = _Lazy(data_clip), _Lazy(annotation_clip)
        for t in self.transforms:
            if isinstance(d, _Lazy) and not hasattr(t, "_apply"):
                d, a = d.materialize(), a.materialize()
            d, a = t(d, a)
        if isinstance(d, _Lazy):
            d, a = d.materialize(), a.materialize()
        return d, a


class RandomApply:
    def __init__(self, transforms, p=0.5):
        self.transforms, self.p = transforms, p

    def __call__(self, clip):
        if random.random() < self.p:
            for t in self.transforms:
                clip = t(clip)
        return clip


class ColorJitter:
    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0, per_frame=False):
        if per_frame:
            raise NotImplementedError("per_frame colour jitter is not used by the training pipeline")
        self.brightness, self.contrast, self.saturation, self.hue = brightness, contrast, saturation, hue

    def get_params(self, brightness, contrast, saturation, hue):
        b = random.uniform(max(0, 1 - brightness), 1 + brightness) if brightness > 0 else None
        c = random.uniform(max(0, 1 - contrast), 1 + contrast) if contrast > 0 else None
        s = random.uniform(max(0, 1 - saturation), 1 + saturation) if saturation > 0 else None
        h = random.uniform(-hue, hue) if hue > 0 else None
        return b, c, s, h

    def __call__(self, clip):
        b, c, s, h = self.get_params(self.brightness, self.contrast, self.saturation, self.hue)
        todo = []  # the reference's order of appends: brightness, saturation, hue, contrast (:762-769)
        if b is not None:
            todo.append((ops.IMG_BRIGHTNESS, b))
        if s is not None:
            todo.append((ops.IMG_SATURATION, s))
        if h is not None:
            todo.append((ops.IMG_HUE, h))
        if c is not None:
            todo.append((ops.IMG_CONTRAST, c))
        random.shuffle(todo)
        if not todo:
            raise UnboundLocalError("jittered_img")  # what the reference does with all four strengths at 0
        mode, value = todo[-1]  # each closure is applied to the ORIGINAL frame; only the last result is kept
        out = clip.clone()
        if mode == ops.IMG_HUE:
            return ops.img_color_(out, mode, 1.0, int(value * 255) % 256)
        return ops.img_color_(out, mode, value)


class RandomGrayscale:
    def __init__(self, p=0.2, per_frame=False):
        if per_frame:
            raise NotImplementedError("per_frame grayscale is not used by the training pipeline")
        self.p = p

    def __call__(self, clip):
        if torch.rand(1) < self.p:
            return ops.img_color_(clip.clone(), ops.IMG_GRAYSCALE)
        return clip


def gaussian_box_params(radius: float, passes: int = 3):
    """BoxBlur.c: the extended-box radius that approximates a Gaussian of std ``radius`` in ``passes`` passes, and its
    fixed-point weights (integer radius, ww, fw); float32 arithmetic as in the C source."""
    f32 = np.float32
    radius = f32(radius)
    sigma2 = f32(radius * radius / f32(passes))
    L = f32(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = f32((2 * l + 1) * (l * (l + 1) - 3 * sigma2))
    a = f32(a / f32(6 * (sigma2 - (l + 1) * (l + 1))))
    fr = f32(l + a)
    r = int(fr)
    ww = int(np.uint32(f32(1 << 24) / f32(fr * f32(2) + f32(1))))
    fw = ((1 << 24) - (r * 2 + 1) * ww) // 2
    return r, ww, fw


def gaussian_blur(frames: torch.Tensor, radius: float) -> torch.Tensor:
    """``img.filter(ImageFilter.GaussianBlur(radius))`` on every frame of ``frames`` (all with the same radius)."""
    r, ww, fw = gaussian_box_params(radius)
    out = frames
    for direction in (0, 1):
        for _ in range(3):
            out = ops.img_box_blur(out, direction, r, ww, fw)
    return out


class RandomGaussianBlur:
    def __init__(self, p=0.5, radius_min=0.1, radius_max=2., per_frame=False):
        if per_frame:
            raise NotImplementedError("per_frame blur is not used by the training pipeline")
        self.p, self.radius_min, self.radius_max = p, radius_min, radius_max

    def __call__(self, clip):
        if random.random() < self.p:
            radii = [random.uniform(self.radius_min, self.radius_max) for _ in range(clip.shape[0])]  # one draw per frame (:640)
            return torch.cat([gaussian_blur(clip[t:t + 1].contiguous(), radii[t]) for t in range(clip.shape[0])], dim=0)
        return clip


class Resize:
    def __init__(self, size, interpolation="bilinear"):
        self.size, self.interpolation = size, interpolation

    def __call__(self, data_clip, annotaion_clip=None):
        if annotaion_clip is not None:
            return _pair(self, data_clip, annotaion_clip)
        return resize_clip(data_clip, self.size, self.interpolation)

    def _apply(self, d, a):
        if self.interpolation not in ("bilinear", "nearest"):
            raise NotImplementedError("only bilinear and nearest resizing are built")
        for clip, nearest in ((d, self.interpolation == "nearest"), (a, True)):   # data as asked, annotations always nearest (:368)
            _, im_h, im_w = clip.shape[:3]
            target = _resize_target(im_h, im_w, self.size)
            if target is None:
                continue
            if nearest:
                clip.gather(nearest_table(im_h, target[0]), nearest_table(im_w, target[1]))
            else:
                clip.resized_crop(0, 0, im_h, im_w, target)
        return d, a


class RandomResize:
    """One ``random.uniform`` scaling factor per clip (:322-349); a clip only, ``'nearest'`` by default.  The reference hands
    ``(new_w, new_h)`` to ``resize_clip``, which swaps a tuple once more: ``int(im_w * s)`` rows by ``int(im_h * s)`` columns."""

    def __init__(self, ratio=(3. / 4., 4. / 3.), interpolation="nearest"):
        self.ratio, self.interpolation = ratio, interpolation

    def __call__(self, clip):
        scaling_factor = random.uniform(self.ratio[0], self.ratio[1])
        im_h, im_w = clip.shape[1], clip.shape[2]
        new_w = int(im_w * scaling_factor)
        new_h = int(im_h * scaling_factor)
        return resize_clip(clip, (new_w, new_h), interpolation=self.interpolation)


class RandomCrop:
    """The same random window for every frame of both clips (:373-419)."""

    def __init__(self, size):
        self.size = (size, size) if isinstance(size, numbers.Number) else size

    def __call__(self, data_clip, annotation_clip=None):
        if annotation_clip is not None:
            return _pair(self, data_clip, annotation_clip)
        return self._apply(_Lazy(data_clip), None)[0].materialize()

    def _apply(self, d, a):
        h, w = self.size
        _, im_h, im_w = d.shape[:3]
        y1, x1 = random_crop_origin(im_h, im_w, h, w)
        for clip in (d, a):
            if clip is not None:
                clip.gather(np.arange(y1, y1 + h, dtype=np.int32), np.arange(x1, x1 + w, dtype=np.int32))
        return d, a


class CenterCrop:
    """The centred window (:559-601)."""

    def __init__(self, size):
        self.size = (size, size) if isinstance(size, numbers.Number) else size

    def __call__(self, data_clip, annotaion_clip=None):
        if annotaion_clip is not None:
            return _pair(self, data_clip, annotaion_clip)
        return self._apply(_Lazy(data_clip), None)[0].materialize()

    def _apply(self, d, a):
        h, w = self.size
        _, im_h, im_w = d.shape[:3]
        y1, x1 = center_crop_origin(im_h, im_w, h, w)
        for clip in (d, a):
            if clip is not None:
                clip.gather(np.arange(y1, y1 + h, dtype=np.int32), np.arange(x1, x1 + w, dtype=np.int32))
        return d, a


class RandomRotation:
    """One ``random.uniform`` angle per clip, then ``img.rotate(angle)`` on every frame (:517-556); a clip only."""

    def __init__(self, degrees):
        if isinstance(degrees, numbers.Number):
            if degrees < 0:
                raise ValueError("If degrees is a single number,must be positive")
            degrees = (-degrees, degrees)
        elif len(degrees) != 2:
            raise ValueError("If degrees is a sequence,it must be of len 2.")
        self.degrees = degrees

    def __call__(self, clip):
        angle = random.uniform(self.degrees[0], self.degrees[1])
        return rotate_clip(clip, angle)


class RandomResizedCrop:
    def __init__(self, size, scale=(0.4, 1.0), ratio=(3. / 4., 4. / 3.), interpolation="bilinear"):
        self.size = size if isinstance(size, (tuple, list)) else (size, size)
        self.interpolation, self.scale, self.ratio = interpolation, scale, ratio

    @staticmethod
    def get_params(clip, scale, ratio):
        """(i, j, h, w) with the reference's draws (``video_transformations.py:447-489``)."""
        height, width = clip.shape[1], clip.shape[2]
        area = height * width
        for _ in range(10):
            target_area = random.uniform(*scale) * area
            log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
            aspect_ratio = math.exp(random.uniform(*log_ratio))
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            if 0 < w <= width and 0 < h <= height:
                i = random.randint(0, height - h)
                j = random.randint(0, width - w)
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

    def _apply(self, d, a):
        if self.interpolation != "bilinear":
            raise NotImplementedError("RandomResizedCrop resizes data clips bilinearly")
        i, j, h, w = self.get_params(d, self.scale, self.ratio)   # one set of parameters for both clips (:498)
        return d.resized_crop(i, j, h, w, self.size), a.resized_crop(i, j, h, w, self.size)

    def __call__(self, data_clip, annotaion_clip=None, _finish=None):
        if annotaion_clip is not None:
            return _pair(self, data_clip, annotaion_clip)
        i, j, h, w = self.get_params(data_clip, self.scale, self.ratio)
        if _finish is None:
            return resized_crop(data_clip, i, j, h, w, self.size)
        flipper, to_tensor = _finish
        flip = flipper is not None and flipper.will_flip()
        return resized_crop(data_clip, i, j, h, w, self.size, to_tensor=to_tensor.mean_std(), flip=flip)


class RandomHorizontalFlip:
    def __init__(self, p=0.5):
        self.p = p

    def __call__(self, data_clip, annotation_clip=None):
        if annotation_clip is not None:
            return _pair(self, data_clip, annotation_clip)
        return torch.flip(data_clip, dims=[2]) if self.will_flip() else data_clip

    def will_flip(self) -> bool:
        chance = 0.5  # the helper's default argument: no random number is drawn on this path
        return chance < self.p

    def _apply(self, d, a):
        chance = random.random()   # with annotations the reference draws (:190)
        if chance < self.p:
            for clip in (d, a):
                _, H, W = clip.shape[:3]
                clip.gather(np.arange(H, dtype=np.int32), np.arange(W, dtype=np.int32)[::-1])
        return d, a


class RandomVerticalFlip:
    """``transpose(FLIP_TOP_BOTTOM)`` of both clips when ``random.random() < p`` (:199-237).  Without an annotation clip the
    reference calls its helper without ``chance`` and raises ``TypeError``; so does this."""

    def __init__(self, p=0.5):
        self.p = p

    def __call__(self, data_clip, annotation_clip=None):
        if annotation_clip is not None:
            return _pair(self, data_clip, annotation_clip)
        raise TypeError("random_vertical_flip() missing 1 required positional argument: 'chance'")

    def _apply(self, d, a):
        chance = random.random()
        if chance < self.p:
            for clip in (d, a):
                _, H, W = clip.shape[:3]
                clip.gather(np.arange(H, dtype=np.int32)[::-1], np.arange(W, dtype=np.int32))
        return d, a


class ClipToTensor:
    """uint8 [fs, H, W, 3] -> float32 [fs, 3, H, W] in [0, 1], normalised when mean and std are given; an annotation clip
    uint8 [fs, H, W] -> float32 [fs, 1, H, W] = v / 255."""

    _apply = None   # ends a lazy chain itself: Compose hands it the lazy clips

    def __init__(self, mean=None, std=None):
        self.mean, self.std = mean, std

    def __call__(self, data_clip, annotation_clip=None):
        if annotation_clip is not None:   # only the data is normalised; the annotations leave as v / 255 (:269-278)
            return _lazy(data_clip).materialize(to_tensor=self.mean_std()), _lazy(annotation_clip).materialize(to_tensor=True)
        _, H, W, _ = data_clip.shape
        return resized_crop(data_clip, 0, 0, H, W, (H, W), to_tensor=self.mean_std())

    def mean_std(self):
        if self.mean is not None and self.std is not None:
            return self.mean, self.std
        return (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def training_transforms(input_resolution: int = 224):
    """The two ``Compose`` objects ``time_tuning.time_tuning`` builds (``time_tuning.py:588-593``): (frame_transform, video_transform)."""
    rand_color_jitter = RandomApply([ColorJitter(brightness=0.8, contrast=0.8, saturation=0.8, hue=0.2)], p=0.8)
    data_transform = Compose([rand_color_jitter, RandomGrayscale(), RandomGaussianBlur()])
    video_transform = Compose([Resize(input_resolution), RandomResizedCrop((input_resolution, input_resolution)), RandomHorizontalFlip(),
                               ClipToTensor(mean=[0.485, 0.456, 0.406], std=[0.228, 0.224, 0.225])])
    return data_transform, video_transform


def evaluation_transforms(input_resolution: int):
    """The pair transform of the evaluation loaders (``evaluation.py:533``, ``cluster_based_foreground_extraction.py:335``)."""
    R = input_resolution
    return Compose([Resize((R, R), "bilinear"), CenterCrop(R), ClipToTensor(mean=[0.485, 0.456, 0.406], std=[0.228, 0.224, 0.225])])


def propagation_transforms(input_resolution: int = 224):
    """The pair transform of the propagation evaluation (``mask_propagation.py:779``)."""
    R = input_resolution
    return Compose([Resize(R, "bilinear"), RandomCrop(R), ClipToTensor(mean=[0.485, 0.456, 0.406], std=[0.228, 0.224, 0.225])])


def annotations_to_uint8(stacked: torch.Tensor) -> torch.Tensor:
    """``read_batch``'s ``(255 * annotations).type(torch.uint8)`` on the stacked clips ``[clips, fs, 1, H, W]`` and its squeeze of
    a size-1 axis 2 (``data_loader.py:673-675``) -> uint8 ``[clips, fs, H, W]``.  Lossless: ``ClipToTensor``'s ``v / 255`` is an exact
    division, and ``255 * (v / 255)`` truncates back to ``v`` for all 256 values."""
    out = (255 * stacked).type(torch.uint8)
    if out.dim() > 2 and out.shape[2] == 1:
        out = out.squeeze(2)
    return out
