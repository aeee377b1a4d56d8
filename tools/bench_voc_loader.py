#!/usr/bin/env python
"""The device half of a Pascal VOC batch behind the decoder: the ragged route against the per-image route.

  python tools/bench_voc_loader.py [--batch 60] [--train_size 448] [--val_size 100] [--reps 30] [--out FILE]

A batch of --batch generated JPEGs and palette PNGs at VOC's common sizes (500 x 375, 375 x 500, 500 x 333, ...) is decoded once
(``decode_jpeg_batch``; the masks are uploaded as one packed buffer) and then resized to S = --train_size / R = --val_size two ways:
  ragged     one ``img_resize_ragged`` call for the images and one ``img_gather_nearest_ragged`` call for the masks
  per image  a loop of ``video_transformations.resized_crop`` / ``gather_clip`` per image, into rows of the same outputs
Reported per route: the median host time of the whole route around a synchronise (table building, uploads and launches included), the
median device time between two events, and the number of kernel launches and of host-to-device table uploads one batch costs.  The two
routes' outputs are compared once.  Needs a GPU and Pillow."""
import argparse
import io
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
VOC_SIZES = [(375, 500), (500, 375), (333, 500), (500, 333), (500, 500), (374, 500), (332, 500), (281, 500), (500, 400), (366, 500)]   # (H, W)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def make_batch(n):
    from PIL import Image

    from timetuning_amd import synth

    files, masks = [], []
    for i in range(n):
        H, W = VOC_SIZES[i % len(VOC_SIZES)]
        z = synth.normal(f"voc.{i}", (-(-H // 8), -(-W // 8), 3), 60.0, 127.0)
        raw = np.clip(np.kron(z, np.ones((8, 8, 1), np.float32)), 0, 255).astype(np.uint8)[:H, :W]
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(raw)).save(buf, "JPEG", quality=90, subsampling=2)
        files.append(buf.getvalue())
        m = (np.add.outer(np.arange(H) // 40, np.arange(W) // 40) % 21).astype(np.uint8)
        m[::37] = 255
        png = io.BytesIO()
        im = Image.fromarray(m, "P")
        im.putpalette([v % 256 for v in range(768)])
        im.save(png, "PNG")
        masks.append(np.asarray(Image.open(io.BytesIO(png.getvalue())), np.uint8))
    return files, masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=60)
    ap.add_argument("--train_size", type=int, default=448)
    ap.add_argument("--val_size", type=int, default=100)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    files, masks = make_batch(a.batch)

    import torch

    from timetuning_amd import hip_ops as ops, video_transformations as VT

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    frames = ops.decode_jpeg_batch(files, dev)
    packed = torch.from_numpy(np.concatenate([m.reshape(-1) for m in masks])).to(dev)
    offs = np.cumsum([0] + [m.size for m in masks])
    maps = [packed[offs[i]:offs[i] + m.size].view(*m.shape) for i, m in enumerate(masks)]
    S, R, n = a.train_size, a.val_size, a.batch

    counts = {"launches": 0, "uploads": 0}

    def counted(name, launches, uploads=0):
        fn = getattr(ops, name)

        def wrapper(*args, **kw):
            counts["launches"] += launches
            counts["uploads"] += uploads
            return fn(*args, **kw)

        setattr(ops, name, wrapper)

    # the per-clip entry points launch once each; a ragged call launches once and uploads its table and its pool
    for name in ("img_resample_h", "img_resample_v", "img_gather_nearest"):
        counted(name, 1)
    counted("img_resize_ragged", 1, 2)
    counted("img_gather_nearest_ragged", 1, 2)
    real_index_table = ops._index_table_on
    real_coeffs = VT._coeffs_on

    def ragged():
        x = ops.img_resize_ragged(frames, S, to_tensor=(MEAN, STD))
        y = ops.img_gather_nearest_ragged(maps, R, to_tensor=True)
        return x, y

    def per_image(cold_tables=False):
        if cold_tables:      # what a first batch pays: every (in, out) table uploaded on its own
            VT._DEVICE_COEFFS.clear()
            ops._DEVICE_TABLES.clear()
        x = torch.empty((n, 3, S, S), dtype=torch.float32, device=dev)
        y = torch.empty((n, 1, R, R), dtype=torch.float32, device=dev)
        for i in range(n):
            H, W = frames[i].shape[:2]
            x[i] = VT.resized_crop(frames[i][None], 0, 0, H, W, (S, S), to_tensor=(MEAN, STD))[0]
            y[i] = VT.gather_clip(maps[i][None], VT.nearest_table(H, R), VT.nearest_table(W, R), True)[0]
        return x, y

    xr, yr = ragged()
    xp, yp = per_image()
    torch.cuda.synchronize()
    lines = [f"N22 VOC batch behind the decoder: {n} images at VOC's sizes -> {S} x {S} float, masks -> {R} x {R} float; {a.reps} repetitions "
             f"after 3 warm-up rounds", f"outputs of both routes equal bit for bit: {bool(torch.equal(xr, xp) and torch.equal(yr, yp))}"]

    def uploads_of_per_image():
        ups = {"n": 0}

        def index_table(tab, limit, device, what):
            key = (str(device), np.ascontiguousarray(np.asarray(tab), dtype=np.int32).tobytes())
            ups["n"] += key not in ops._DEVICE_TABLES
            return real_index_table(tab, limit, device, what)

        def coeffs(device, in_size, out_size):
            ups["n"] += 2 * ((str(device), in_size, out_size) not in VT._DEVICE_COEFFS)
            return real_coeffs(device, in_size, out_size)

        ops._index_table_on, VT._coeffs_on = index_table, coeffs
        try:
            per_image(cold_tables=True)
        finally:
            ops._index_table_on, VT._coeffs_on = real_index_table, real_coeffs
        return ups["n"]

    results = {}
    for label, fn in (("ragged", ragged), ("per image", per_image)):
        host, device = [], []
        for rep in range(a.reps + 3):
            counts["launches"] = counts["uploads"] = 0
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            w0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            w1 = time.perf_counter()
            if rep >= 3:
                host.append(w1 - w0)
                device.append(e0.elapsed_time(e1) * 1e-3)
        results[label] = (float(np.median(host)), float(np.median(device)), min(host), max(host), counts["launches"], counts["uploads"])
    cold_uploads = uploads_of_per_image()
    for label, (h, d, lo, hi, launches, uploads) in results.items():
        extra = f"{uploads} table uploads" if label == "ragged" else f"0 table uploads with warm table caches, {cold_uploads} on a first batch"
        copies = "" if label == "ragged" else f" + {2 * n} row copies into the batch tensors"
        lines.append(f"{label:10s}: {h * 1e3:8.3f} ms host (median; min {lo * 1e3:.3f} / max {hi * 1e3:.3f}), {d * 1e3:8.3f} ms between device events; "
                     f"{launches} kernel launches{copies}, {extra}")
    ratio = results["per image"][0] / results["ragged"][0]
    lines.append(f"per image / ragged, host time: {ratio:.2f} x" + ("" if ratio > 1 else "  (the ragged route is NOT faster)"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
