#!/usr/bin/env python
"""Decode rate of the N21 JPEG route against Pillow in worker processes (output: profiles/n21_jpeg_decode.txt).

  python tools/bench_jpeg_decode.py [--frames 128] [--threads 16] [--procs 16] [--reps 20] [--out FILE]

The frames are ``SyntheticFrameClips``' raw 360 x 480 frames, encoded once with Pillow (quality 90, 4:2:0).  Device route, per batch of
--frames files: host scan (jpeg_scan_batch in --threads threads, host clock), the two host-to-device copies and the two launches (device
events each), and the whole call end to end (host clock around a synchronise).  Yardstick: the same bytes through ``Image.open`` in --procs
worker processes, as the reference's DataLoader workers decode them (the workers return a checksum, not the pixels: their transport is
not charged).  The pixels of both routes are compared once.  Needs a GPU and Pillow."""
import argparse
import io
import multiprocessing as mp
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12      # bytes / s: a float4 copy as measured on an MI355X, and the data-sheet figure


def pillow_decode(data):
    from PIL import Image

    return int(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).sum())


def make_files(n, H=360, W=480):
    from PIL import Image

    from timetuning_amd import synth

    files = []
    for i in range(n):
        z = synth.normal(f"raw.0.{i // 4}.{i % 4}", (1, H // 8, W // 8, 3), 60.0, 127.0)
        raw = np.clip(np.kron(z, np.ones((1, 8, 8, 1), np.float32)), 0, 255).astype(np.uint8)[0]
        buf = io.BytesIO()
        Image.fromarray(raw).save(buf, "JPEG", quality=90, subsampling=2)
        files.append(buf.getvalue())
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    files = make_files(a.frames)
    lines = [f"N21 JPEG decode: {a.frames} frames of 360 x 480, 4:2:0, quality 90, {sum(map(len, files)) / a.frames / 1024:.1f} KiB per file; "
             f"{a.reps} repetitions after 3 warm-up rounds"]

    # ---- the yardstick first, before this process touches the GPU: Pillow in worker processes (spawned: they never open the GPU)
    with mp.get_context("spawn").Pool(a.procs) as pool:
        for _ in range(3):
            sums = pool.map(pillow_decode, files, chunksize=max(1, a.frames // (4 * a.procs)))
        t0 = time.perf_counter()
        for _ in range(a.reps):
            pool.map(pillow_decode, files, chunksize=max(1, a.frames // (4 * a.procs)))
        t_pillow = (time.perf_counter() - t0) / a.reps
    t0 = time.perf_counter()
    for f in files:
        pillow_decode(f)
    t_pillow_one = time.perf_counter() - t0
    lines.append(f"Pillow, {a.procs} worker processes : {t_pillow * 1e3:8.2f} ms per batch = {a.frames / t_pillow:9.0f} frames/s   "
                 f"(one process: {a.frames / t_pillow_one:.0f} frames/s)")

    import torch

    import timetuning_amd  # noqa: F401
    from timetuning_amd import _lib, hip_ops

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    frames = hip_ops.decode_jpeg_batch(files, dev, a.threads)
    torch.cuda.synchronize()
    got = [int(f.sum().item()) for f in frames]
    lines.append(f"pixels equal Pillow's on all {a.frames} frames (sum check): {got == sums}")
    from PIL import Image
    same = all(np.array_equal(frames[i].cpu().numpy(), np.asarray(Image.open(io.BytesIO(files[i])).convert("RGB"))) for i in range(0, a.frames, 16))
    lines.append(f"pixels equal Pillow's bit for bit on every 16th frame: {same}")

    n, row = a.frames, 16 * 8
    ev = lambda: torch.cuda.Event(enable_timing=True)
    t_scan, t_h2d, t_kern, t_all = [], [], [], []
    for rep in range(a.reps + 3):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        batch = hip_ops.jpeg_scan_batch(files, a.threads)
        w1 = time.perf_counter()
        table = batch.meta.numpy()[:n * row]
        ws_bytes = int(lib.tt_jpeg_decode_batch_workspace_bytes(table.ctypes.data, n))
        out = torch.empty(batch.out_bytes, dtype=torch.uint8, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        coeffs = batch.coeffs.to(dev, non_blocking=True)
        meta = batch.meta.to(dev, non_blocking=True)
        e1.record()
        rc = lib.tt_jpeg_decode_batch(coeffs.data_ptr(), batch.n_coeffs, meta.data_ptr() + n * row, 3 * n, table.ctypes.data, meta.data_ptr(), n,
                                      out.data_ptr(), out.numel(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        e2.record()
        torch.cuda.synchronize()
        w2 = time.perf_counter()
        if rep >= 3:
            t_scan.append(w1 - w0)
            t_h2d.append(e0.elapsed_time(e1) * 1e-3)
            t_kern.append(e1.elapsed_time(e2) * 1e-3)
            t_all.append(w2 - w0)
    med = lambda v: float(np.median(v))
    spread = lambda v: f"min {min(v) * 1e3:.2f} / max {max(v) * 1e3:.2f}"
    lines.append(f"device route, {a.threads} host threads  : {med(t_all) * 1e3:8.2f} ms per batch = {a.frames / med(t_all):9.0f} frames/s   (end to end, "
                 f"median; {spread(t_all)} ms)")
    lines.append(f"  host scan (markers + Huffman)  : {med(t_scan) * 1e3:8.2f} ms   ({spread(t_scan)})  = {a.frames / med(t_scan):.0f} frames/s")
    coeff_bytes = 2 * batch.n_coeffs
    lines.append(f"  host-to-device copies          : {med(t_h2d) * 1e3:8.2f} ms   ({spread(t_h2d)})  {coeff_bytes / 1e6:.1f} MB of coefficients = "
                 f"{coeff_bytes / med(t_h2d) / 1e9:.1f} GB/s; the decoded RGB would be {batch.out_bytes / 1e6:.1f} MB")
    moved = coeff_bytes + batch.n_coeffs + batch.n_coeffs + batch.out_bytes      # IDCT: coefficients in, planes out; colour: planes in, RGB out
    rate = moved / med(t_kern)
    lines.append(f"  the two launches               : {med(t_kern) * 1e3:8.2f} ms   ({spread(t_kern)})  {moved / 1e6:.1f} MB moved = {rate / 1e9:.0f} GB/s = "
                 f"{100 * rate / HBM_MEASURED:.1f} % of the measured HBM copy rate ({HBM_MEASURED / 1e12:.2f} TB/s), {100 * rate / HBM_SPEC:.1f} % of the "
                 f"{HBM_SPEC / 1e12:.0f} TB/s data-sheet figure (event time of both launches, launch gaps included)")
    ratio = t_pillow / med(t_all)
    lines.append(f"device route / Pillow at {a.threads} host CPUs each: {ratio:.2f} x" + ("" if ratio > 1 else "  (NOT faster)"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
