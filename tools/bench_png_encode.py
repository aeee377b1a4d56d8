#!/usr/bin/env python
"""N29: label maps written as palette PNGs, three routes alternating inside each repetition, medians after warm-up.  The maps are on
the GPU (predictions); every route ends with the finished files as ``bytes`` on the host.

  (a) parent   one device-to-host copy of the raw maps, then Pillow's ``Image.fromarray`` + ``putpalette`` + ``save`` file after file:
               what a user of the parent commit would write
  (b) pooled   the same ``save`` in 16 pool threads
  (c) device   ``hip_ops.encode_png_batch``: tables, three launches (``tt_png_encode_batch``), two read-backs, ``tt_png_write_file`` in the
               pool - timed apart

    python tools/bench_png_encode.py [--reps 15] [--warmup 3]
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
from timetuning_amd import _lib, hip_ops as ops, visualization  # noqa: E402

THREADS = 16


def blob_map(H, W, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), np.uint8)
    for v in range(1, 5):
        cy, cx, ry, rx = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(H / 8, H / 3), rng.uniform(W / 8, W / 3)
        m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1] = v
    return m


def pillow_save(m, flat_palette):
    from PIL import Image

    im = Image.fromarray(m)
    im.putpalette(flat_palette)
    buf = io.BytesIO()
    im.save(buf, format="PNG")
    return buf.getvalue()


def bench(name, host_maps, reps, warmup, dev):
    from PIL import Image

    lib = _lib.load()
    pal = visualization.voc_palette()
    flat = pal.reshape(-1).tolist()
    maps = [torch.from_numpy(m).to(dev) for m in host_maps]
    n = len(maps)
    t = {k: [] for k in ("a", "b", "c", "c_plan", "c_copy", "c_launch", "c_back", "c_wrap")}
    sizes = {}
    for rep in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        raw = [m.cpu().numpy() for m in maps]
        files_a = [pillow_save(m, flat) for m in raw]
        t1 = time.perf_counter()
        raw = [m.cpu().numpy() for m in maps]
        files_b = ops._each_file(lambda i: pillow_save(raw[i], flat), n, THREADS)
        t2 = time.perf_counter()
        files_c = ops.encode_png_batch(maps, palette=pal, threads=THREADS)
        t3 = time.perf_counter()
        # (c) again, split into its parts
        plan = ops.png_encode_plan(maps)
        t4 = time.perf_counter()
        out = torch.empty(plan.out_bytes, dtype=torch.uint8, device=dev)
        results = torch.empty(n * 32, dtype=torch.uint8, device=dev)
        ws = ops._ws(plan.ws_bytes, dev)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        e[0].record()
        meta = plan.meta.to(dev, non_blocking=True)
        e[1].record()
        _lib.check(lib.tt_png_encode_batch(plan.table.ctypes.data, meta.data_ptr() + plan.layout["maps"][0], n, plan.chunks.ctypes.data,
                                           meta.data_ptr() + plan.layout["chunks"][0], plan.n_chunks, out.data_ptr(), out.numel(), results.data_ptr(),
                                           ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "tt_png_encode_batch")
        e[2].record()
        torch.cuda.synchronize()
        t5 = time.perf_counter()
        table = results.cpu().numpy().view(ops._PNG_RESULT)
        total = int(table["offset"][-1] + table["length"][-1])
        host = out[:total].cpu().numpy()
        t6 = time.perf_counter()
        streams, adlers = ops._png_streams(host, table)
        again = ops.png_wrap_files(streams, adlers, [tuple(m.shape) for m in maps], pal, THREADS)
        t7 = time.perf_counter()
        if rep == 0:
            assert again == files_c
            for fa, fb, fc, m in zip(files_a, files_b, files_c, host_maps):
                assert fa == fb and np.array_equal(np.asarray(Image.open(io.BytesIO(fc))), m) and np.array_equal(np.asarray(Image.open(io.BytesIO(fa))), m)
            sizes = dict(a=sum(map(len, files_a)), c=sum(map(len, files_c)), tables=plan.meta.numel(), back=total + 32 * n, chunks=plan.n_chunks)
        if rep >= warmup:
            t["a"].append(t1 - t0)
            t["b"].append(t2 - t1)
            t["c"].append(t3 - t2)
            t["c_plan"].append(t4 - t3)
            t["c_copy"].append(e[0].elapsed_time(e[1]) / 1e3)
            t["c_launch"].append(e[1].elapsed_time(e[2]) / 1e3)
            t["c_back"].append(t6 - t5)
            t["c_wrap"].append(t7 - t6)
    med = {k: 1e3 * statistics.median(v) for k, v in t.items()}
    pixels = sum(m.size for m in host_maps)
    print(f"{name}: {n} maps, {pixels} pixels, {sizes['chunks']} chunks")
    print(f"  (a) copy + Pillow save, serial      {med['a']:8.3f} ms   PCIe {pixels} bytes back   files {sizes['a']} bytes")
    print(f"  (b) copy + Pillow save, {THREADS} threads  {med['b']:8.3f} ms   PCIe {pixels} bytes back   files {sizes['a']} bytes   (b)/(a) = {med['b'] / med['a']:.3f}")
    print(f"  (c) encode_png_batch                {med['c']:8.3f} ms   PCIe {sizes['tables']} bytes of tables + {sizes['back']} back   files {sizes['c']} bytes"
          f"   (c)/(b) = {med['c'] / med['b']:.3f}   (c)/(a) = {med['c'] / med['a']:.3f}")
    print(f"      tables {med['c_plan']:.3f} ms, copy {med['c_copy']:.3f} ms, three launches {med['c_launch']:.3f} ms = {1e3 * med['c_launch'] / n:.1f} us per map, "
          f"two read-backs {med['c_back']:.3f} ms, wrapping {med['c_wrap']:.3f} ms")
    print(f"      file bytes (c) / Pillow = {sizes['c'] / sizes['a']:.2f}; (c) / raw pixels = {100.0 * sizes['c'] / pixels:.2f} %")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=15)
    p.add_argument("--warmup", type=int, default=3)
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    print(torch.cuda.get_device_name(0))
    bench("video batch 480 x 854", [blob_map(480, 854, k) for k in range(128)], args.reps, args.warmup, dev)
    sizes = [(375, 500), (500, 375), (333, 500), (500, 333), (281, 500), (366, 500)]
    bench("VOC batch", [blob_map(*sizes[k % 6], 1000 + k) for k in range(60)], args.reps, args.warmup, dev)


if __name__ == "__main__":
    main()
