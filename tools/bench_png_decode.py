#!/usr/bin/env python
"""N26: annotation PNG decode, three routes alternating inside each repetition, medians after warm-up.

  (a) parent   serial ``decode_annotation`` (Pillow) on one thread, then the uploads the loaders made: one per clip of 8 maps (video
               batch) or one packed buffer (VOC batch)
  (b) pooled   the same through ``data_loader.decode_annotations`` at 16 threads
  (c) device   ``hip_ops.png_prepare_batch`` (16 threads) + one copy + ONE launch (``tt_png_decode_batch``), timed apart

    python tools/bench_png_decode.py [--reps 15] [--warmup 3]
"""
import argparse
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from timetuning_amd import _lib, data_loader as DL, hip_ops as ops  # noqa: E402

THREADS = 16


def blob_png(H, W, seed):
    from PIL import Image

    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), np.uint8)
    for v in range(1, 5):
        cy, cx, ry, rx = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(H / 8, H / 3), rng.uniform(W / 8, W / 3)
        m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1] = v
    im = Image.fromarray(m, "P")
    im.putpalette(list(range(256)) * 3)
    buf = io.BytesIO()
    im.save(buf, "PNG")
    return buf.getvalue()


def upload(maps, clip, dev):
    if clip:
        return [torch.from_numpy(np.stack(maps[i:i + clip])).to(dev) for i in range(0, len(maps), clip)]
    buf = torch.empty(sum(m.size for m in maps), dtype=torch.uint8, pin_memory=True)
    view, at = buf.numpy(), 0
    for m in maps:
        view[at:at + m.size] = m.reshape(-1)
        at += m.size
    return [buf.to(dev, non_blocking=True)]


def bench(name, files, clip, reps, warmup, dev):
    lib = _lib.load()
    t = {k: [] for k in ("a", "b", "c", "c_prepare", "c_copy", "c_launch")}
    for rep in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        upload([DL.decode_annotation(f) for f in files], clip, dev)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        upload(DL.decode_annotations(files, THREADS), clip, dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        batch = ops.png_prepare_batch(files, THREADS)
        t3 = time.perf_counter()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        n, table = len(files), batch.table
        out = torch.empty(batch.out_bytes, dtype=torch.uint8, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        ws = ops._ws(batch.ws_bytes, dev)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        e[0].record()
        meta = batch.meta.to(dev, non_blocking=True)
        e[1].record()
        _lib.check(lib.tt_png_decode_batch(meta.data_ptr() + batch.layout["streams"][0], batch.layout["streams"][1], table.ctypes.data, meta.data_ptr(), n,
                                           out.data_ptr(), out.numel(), ws.data_ptr(), ws.numel(), status.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), "tt_png_decode_batch")
        e[2].record()
        bad = int(status.cpu().abs().sum())
        t5 = time.perf_counter()
        assert bad == 0
        if rep >= warmup:
            t["a"].append(t1 - t0)
            t["b"].append(t2 - t1)
            t["c_prepare"].append(t3 - t2)
            t["c_copy"].append(e[0].elapsed_time(e[1]) / 1e3)
            t["c_launch"].append(e[1].elapsed_time(e[2]) / 1e3)
            t["c"].append((t3 - t2) + (t5 - t4))
    med = {k: 1e3 * statistics.median(v) for k, v in t.items()}
    pixels, compressed = batch.out_bytes, batch.meta.numel()
    print(f"{name}: {len(files)} maps, {pixels} pixels, {sum(len(f) for f in files)} file bytes")
    print(f"  (a) parent, serial + uploads        {med['a']:8.3f} ms   PCIe {pixels} bytes")
    print(f"  (b) pooled host, {THREADS} threads         {med['b']:8.3f} ms   PCIe {pixels} bytes        (b)/(a) = {med['b'] / med['a']:.3f}")
    print(f"  (c) device route                    {med['c']:8.3f} ms   PCIe {compressed} bytes + {4 * len(files)} back   (c)/(b) = {med['c'] / med['b']:.3f}")
    print(f"      prepare {med['c_prepare']:.3f} ms, copy {med['c_copy']:.3f} ms, launch {med['c_launch']:.3f} ms = {1e3 * med['c_launch'] / len(files):.1f} us per file")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=15)
    p.add_argument("--warmup", type=int, default=3)
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    print(torch.cuda.get_device_name(0))
    bench("video batch 480 x 854", [blob_png(480, 854, k) for k in range(128)], 8, args.reps, args.warmup, dev)
    sizes = [(375, 500), (500, 375), (333, 500), (500, 333), (281, 500), (366, 500)]
    bench("VOC batch", [blob_png(*sizes[k % 6], 1000 + k) for k in range(60)], 0, args.reps, args.warmup, dev)


if __name__ == "__main__":
    main()
