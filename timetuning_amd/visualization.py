"""Overlay rendering and GIF logs: the qualitative side of the reference (``time_tuning.py:305-352``, ``my_utils.py:41-141``,
``evaluation.py:255-300``) on one render launch per batch (``hip_ops.overlay_grid``).

The reference renders frame by frame on the host: ``torchvision.utils.draw_segmentation_masks`` on a full one-hot mask after a
``.cpu()``, ``make_grid``, a matplotlib figure saved to PNG and decoded again.  Here a batch of frames and cluster maps leaves the
device as finished ``uint8`` grids in ``make_grid``'s layout (n tiles in one row, padding 2, pad value 0).  What is kept: the layout,
the blend arithmetic of ``draw_segmentation_masks``, the colours of ``my_utils.generate_colors`` (so a run seeded like the reference
draws its colours), the GIF call of ``my_utils.convert_list_to_video`` and the file names.  What is not restated: the pixel output
of the matplotlib figures (axes, colour bar, the ten named colours of ``my_utils.localize_objects``) - the panels are "unpinned" -
and the wandb leg."""
from __future__ import annotations

import os
import random

import numpy as np
import torch
import torch.nn.functional as F

from . import hip_ops as ops

MEAN, STD = [0.485, 0.456, 0.406], [0.228, 0.224, 0.225]   # time_tuning.py:456-457 (the reference's own std, 0.228 included)


def voc_palette(n: int = 256) -> np.ndarray:
    """The Pascal VOC colour map, uint8 [n, 3]: bit j of the label feeds bit 7 - j / 3 of the channel j % 3 (index 1 = (128, 0, 0),
    2 = (0, 128, 0), 15 = (192, 128, 128), 255 = (224, 224, 192)); its first 256 entries are distinct."""
    pal = np.zeros((n, 3), np.uint8)
    for i in range(n):
        c, r, g, b = i, 0, 0, 0
        for j in range(8):
            r |= ((c >> 0) & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        pal[i] = (r, g, b)
    return pal


def generate_colors(num_colors: int) -> list:
    """``my_utils.generate_colors`` (my_utils.py:82-89): three ``random.randint(0, 255)`` per colour, in order."""
    colors = []
    for _ in range(num_colors):
        colors.append(tuple([random.randint(0, 255), random.randint(0, 255), random.randint(0, 255)]))
    return colors


def denormalize(data: torch.Tensor, mean, std) -> torch.Tensor:
    """``my_utils.denormalize`` (my_utils.py:68-70) for [..., 3, H, W]."""
    shape = (1,) * (data.dim() - 3) + (3, 1, 1)
    return data * torch.tensor(std, device=data.device).view(shape) + torch.tensor(mean, device=data.device).view(shape)


def _palette(colors) -> torch.Tensor:
    pal = voc_palette() if colors is None else np.asarray(colors)
    if pal.ndim != 2 or pal.shape[1] != 3 or pal.shape[0] < 1 or pal.min() < 0 or pal.max() > 255:
        raise ValueError("colors: a list of (r, g, b) with 0 <= r, g, b <= 255 is needed")
    return torch.from_numpy(np.ascontiguousarray(pal.astype(np.uint8)))


def nearest_tables(Hl: int, Wl: int, H: int, W: int):
    """int32 numpy tables (ytab [H], xtab [W]) of ``F.interpolate(mode="nearest")`` from Hl x Wl to H x W, read off torch itself."""
    def one(src, dst):
        ramp = torch.arange(src, dtype=torch.float64).view(1, 1, src)
        return F.interpolate(ramp, size=dst, mode="nearest")[0, 0].long().numpy().astype(np.int32)

    return one(Hl, H), one(Wl, W)


def _labels(maps: torch.Tensor, name: str) -> torch.Tensor:
    maps = torch.as_tensor(maps)
    if maps.dtype not in (torch.uint8, torch.int16, torch.int64):
        if maps.is_floating_point() or maps.dtype == torch.bool:
            raise TypeError(f"{name}: integer label maps are needed, got {maps.dtype}")
        maps = maps.long()
    return maps.cuda().contiguous()


def _tables(Hl, Wl, H, W):
    return (None, None) if (Hl, Wl) == (H, W) else nearest_tables(Hl, Wl, H, W)


def overlay_clips(data, maps, colors=None, alpha: float = 0.5, mean=None, std=None, pad: int = 2) -> torch.Tensor:
    """data [bs, fs, 3, H, W] float32 (``mean`` / ``std``: its normalisation, None = frames in [0, 1]), maps [bs, fs, h, w] integer
    cluster maps -> uint8 [bs, fs, 3, H + 2 pad, 2 W + 3 pad] on the device, ``[frame | frame under its coloured map]`` per frame,
    from ONE launch.  Maps of another size are read by nearest up-sampling."""
    bs, fs, c, H, W = data.shape
    maps = _labels(maps, "maps")
    if tuple(maps.shape[:2]) != (bs, fs) or maps.dim() != 4:
        raise ValueError(f"maps: expected [{bs}, {fs}, h, w], got {tuple(maps.shape)}")
    h, w = maps.shape[2:]
    ytab, xtab = _tables(h, w, H, W)
    frames = data.reshape(bs * fs, c, H, W).float().cuda().contiguous()
    out = ops.overlay_grid(ops.OVERLAY_PHOTO, maps.view(bs * fs, h, w), _palette(colors), frames=frames, ytab=ytab, xtab=xtab, alpha=alpha,
                           pad=pad, mean=mean, std=std)
    return out.view(bs, fs, *out.shape[1:])


def make_overlayed_grid(input_img, cluster_map, colors=None, alpha: float = 0.5) -> torch.Tensor:
    """``time_tuning.make_overlayed_grid`` (time_tuning.py:332-341): input_img [3, H, W] in [0, 1], cluster_map [h, w] ->
    uint8 [3, H + 4, 2 W + 6].  ``colors`` stands for the reference's global ``label_color_map`` (None = the VOC palette)."""
    return overlay_clips(input_img[None, None], torch.as_tensor(cluster_map)[None, None], colors, alpha)[0, 0]


def label_panels(gt, pred, lut=None, colors=None, alpha: float = 0.5, size=None, pad: int = 2) -> torch.Tensor:
    """gt, pred [F, h, w] integer maps -> uint8 [F, 3, H + 2 pad, 3 W + 4 pad]: ``[colour(gt) | colour(lut[pred]) | both blended]``
    per frame from one launch - what ``my_utils.localize_objects(gt, map)`` shows (my_utils.py:41-65), without the matplotlib figure.
    ``lut`` [L] or [F, L] maps a predicted value to the value whose colour it takes (the ground truth's colours are never mapped)."""
    gt, pred = _labels(gt, "gt"), _labels(pred, "pred")
    if gt.dtype != pred.dtype:
        gt, pred = gt.long(), pred.long()
    if gt.dim() != 3 or gt.shape != pred.shape:
        raise ValueError(f"label_panels: gt {tuple(gt.shape)} and pred {tuple(pred.shape)} need one shape [F, h, w]")
    Fr, h, w = gt.shape
    H, W = (h, w) if size is None else size
    ytab, xtab = _tables(h, w, H, W)
    pal = _palette(colors)
    return ops.overlay_grid(ops.OVERLAY_LABELS, pred, pal, labels_b=gt, size=(H, W), ytab=ytab, xtab=xtab, lut=lut, alpha=alpha, pad=pad)


def convert_list_to_video(frames_list, name: str, speed, directory: str = "") -> str:
    """``my_utils.convert_list_to_video`` (my_utils.py:139-141) without the wandb leg: frames (uint8 [H, W, 3] arrays) ->
    ``{directory}{name}.gif`` through Pillow, ``duration=speed`` milliseconds per frame, looping forever.  Returns the path."""
    from PIL import Image

    frames = [Image.fromarray(np.asarray(frame)) for frame in frames_list]
    path = f"{directory}{name}.gif"
    frames[0].save(path, save_all=True, append_images=frames[1:], duration=speed, loop=0)
    return path


def grids_to_frames(grids: torch.Tensor) -> list:
    """uint8 [F, 3, h, w] on the device -> F host arrays [h, w, 3] (one copy)."""
    return list(grids.permute(0, 2, 3, 1).contiguous().cpu().numpy())


def make_working_directory(name: str) -> None:
    """``my_utils.make_working_directory`` (my_utils.py:160-167): the directory exists afterwards and holds no GIF."""
    if os.path.isdir(name):
        for f in os.listdir(name):
            if f.endswith(".gif"):
                os.remove(os.path.join(name, f))
    else:
        os.makedirs(name)


def localize_clip(data, cluster_map, logging_directory: str, name: str, colors=None, mean=None, std=None) -> list:
    """``time_tuning.localize_clip`` (time_tuning.py:322-329): data [bs, fs, 3, H, W], cluster_map [bs, fs, h, w] -> one GIF per clip,
    ``{logging_directory}/{name}_{i}.gif`` at ``speed = 1000 / fs``; all frames are rendered by one launch.  Returns the paths."""
    grids = overlay_clips(data, cluster_map, colors, mean=mean, std=std)
    bs, fs = grids.shape[:2]
    return [convert_list_to_video(grids_to_frames(grids[i]), name + "_" + str(i), speed=1000 / fs, directory=logging_directory + "/")
            for i in range(bs)]
