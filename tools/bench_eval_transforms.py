#!/usr/bin/env python3
"""N11: the evaluation pair transform (``evaluation_transforms(R)``: Resize((R, R), bilinear) -> CenterCrop(R) -> ClipToTensor on
the frames, one nearest gather that writes the float plane on the label maps) on one DAVIS-size clip - 50 frames of 480 x 854,
uint8 frames [50, 480, 854, 3] and uint8 label maps [50, 480, 854] in device memory - to 224 x 224 and 448 x 448.  One JSON line per
resolution:
  - ``chain_ms_per_clip``: ``evaluation_transforms(R)(frames, labels)`` + ``annotations_to_uint8``, device events, median of
    ``--iters`` after a warm-up; ``data_ms`` / ``labels_ms`` the two halves on their own (two resampling launches; one gather);
  - ``gather_f32_ms`` / ``gather_u8_ms``: ``tt_img_gather_nearest`` alone on the label maps with the chain's tables, and
    ``affine_labels_ms`` / ``affine_frames_ms``: ``tt_img_affine_nearest`` (a 30 degree ``rotate``) on the label maps and the frames at
    full size;
  - ``*_floor_ms`` and ``*_floor_fraction``: the bytes a launch cannot avoid at 6.3 TB/s (the measured HBM copy rate) - the source
    bytes actually gathered (distinct rows x distinct columns; for the rotation the pixels that land inside the frame) plus the
    bytes written - from the shapes, not measured; fraction = floor / measured;
  - ``pillow_ms_per_clip``: where Pillow is importable, the same chain on PIL images on the host, single thread (the reference's
    engine: ``Image.resize`` BILINEAR / NEAREST, ``crop``, the ToTensor arithmetic in torch).

    python tools/bench_eval_transforms.py [--iters 20] [--no-pillow]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from timetuning_amd import hip_ops as ops  # noqa: E402
from timetuning_amd import video_transformations as VT  # noqa: E402

HBM_BPS = 6.3e12
FS, H, W = 50, 480, 854
MEAN, STD = [0.485, 0.456, 0.406], [0.228, 0.224, 0.225]


def time_events(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def gather_floor_ms(ytab, xtab, channels, out_bytes_per_value):
    src = FS * len(np.unique(ytab)) * len(np.unique(xtab)) * channels
    dst = FS * len(ytab) * len(xtab) * channels * out_bytes_per_value
    return (src + dst) / HBM_BPS * 1e3


def affine_floor_ms(coeffs, channels):
    a0, a1, a2, a3, a4, a5 = coeffs
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    xin, yin = (a2 + a1 * y + a0 * x) >> 16, (a5 + a4 * y + a3 * x) >> 16
    inside = int(((xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)).sum())
    return FS * (inside + H * W) * channels / HBM_BPS * 1e3


def pillow_chain_ms(frames, labels, R):
    from PIL import Image

    imgs, anns = [Image.fromarray(f) for f in frames], [Image.fromarray(m, "L") for m in labels]
    mean, std = torch.tensor(MEAN)[None, :, None, None], torch.tensor(STD)[None, :, None, None]
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    y1, x1 = VT.center_crop_origin(R, R, R, R)
    d = [im.resize((R, R), Image.BILINEAR).crop((x1, y1, x1 + R, y1 + R)) for im in imgs]
    a = [im.resize((R, R), Image.NEAREST).crop((x1, y1, x1 + R, y1 + R)) for im in anns]
    d = torch.stack([torch.from_numpy(np.array(im)).permute(2, 0, 1).contiguous().float().div(255) for im in d])
    a = torch.stack([torch.from_numpy(np.array(im))[None].float().div(255) for im in a])
    d = (d - mean) / std
    a = (255 * a).type(torch.uint8).squeeze(1)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-pillow", action="store_true")
    args = ap.parse_args()
    import _nearest_ops as NO

    torch.cuda.set_device(0)
    one = NO.frame_clip(1, H, W, 1)
    frames_np = np.concatenate([np.roll(one, 3 * t, axis=2) for t in range(FS)])
    labels_np = NO.label_clip(FS, H, W, 1)
    frames, labels = torch.from_numpy(frames_np).cuda(), torch.from_numpy(labels_np).cuda()
    rot = VT.rotate_coeffs(W, H, 30.0)
    affine_labels = time_events(lambda: ops.img_affine_nearest(labels, rot), args.iters)
    affine_frames = time_events(lambda: ops.img_affine_nearest(frames, rot), args.iters)
    for R in (224, 448):
        chain = VT.evaluation_transforms(R)
        ytab, xtab = VT.nearest_table(H, R), VT.nearest_table(W, R)

        def run():
            d, a = chain(frames, labels)
            return d, VT.annotations_to_uint8(a[None])

        rec = {"R": R, "frames": FS, "H": H, "W": W, "chain_ms_per_clip": round(time_events(run, args.iters), 4),
               "data_ms": round(time_events(lambda: VT.resized_crop(frames, 0, 0, H, W, (R, R), to_tensor=(MEAN, STD)), args.iters), 4),
               "labels_ms": round(time_events(lambda: ops.img_gather_nearest(labels, ytab, xtab, True), args.iters), 4)}
        for key, fn, floor in (("gather_f32", lambda: ops.img_gather_nearest(labels, ytab, xtab, True), gather_floor_ms(ytab, xtab, 1, 4)),
                               ("gather_u8", lambda: ops.img_gather_nearest(labels, ytab, xtab), gather_floor_ms(ytab, xtab, 1, 1)),
                               ("gather_frames_f32", lambda: ops.img_gather_nearest(frames, ytab, xtab, (MEAN, STD)), gather_floor_ms(ytab, xtab, 3, 4))):
            ms = time_events(fn, args.iters)
            rec.update({key + "_ms": round(ms, 4), key + "_floor_ms": round(floor, 5), key + "_floor_fraction": round(floor / ms, 3)})
        for key, ms, ch in (("affine_labels", affine_labels, 1), ("affine_frames", affine_frames, 3)):
            floor = affine_floor_ms(rot, ch)
            rec.update({key + "_ms": round(ms, 4), key + "_floor_ms": round(floor, 5), key + "_floor_fraction": round(floor / ms, 3)})
        if not args.no_pillow:
            try:
                rec["pillow_ms_per_clip"] = round(pillow_chain_ms(frames_np, labels_np, R), 1)
            except ImportError:
                rec["pillow_ms_per_clip"] = None
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
