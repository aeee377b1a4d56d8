#!/usr/bin/env python
"""Decode rate of the JPEG routes against Pillow in worker processes (output: profiles/n21_jpeg_decode.txt,
profiles/n24_jpeg_entropy.txt).

  python tools/bench_jpeg_decode.py [--frames 128] [--size 360x480] [--threads 16] [--procs 16] [--reps 20] [--entropy host|device|both]
                                    [--subseq_bits 1024[,256,...]] [--skip_pillow] [--out FILE]

The frames are ``SyntheticFrameClips``' raw frames (360 x 480, or --size), encoded once with Pillow (quality 90, 4:2:0).  Host-entropy route
(N21), per batch of --frames files: host scan (jpeg_scan_batch in --threads threads, host clock), the two host-to-device copies and the
two launches (device events each), and the whole call end to end (host clock around a synchronise).  Device-entropy route (N24): host
prepare (jpeg_prepare_batch, host clock), the ONE copy of the compressed streams and tables, the entropy launch with its memset, the
same two launches (device events each), and end to end - per --subseq_bits value, with the rounds the kernel reports.  With "both" the
routes alternate inside every repetition.  Yardstick: the same bytes through ``Image.open`` in --procs worker processes, as the
reference's DataLoader workers decode them (the workers return a checksum, not the pixels: their transport is not charged).  The pixels
of every route are compared once.  Needs a GPU and Pillow."""
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
    ap.add_argument("--size", type=str, default="360x480", help="H x W of the frames (multiples of 8)")
    ap.add_argument("--entropy", choices=["host", "device", "both"], default="host")
    ap.add_argument("--subseq_bits", type=str, default="", help="comma-separated values for the device route (default: hip_ops.JPEG_SUBSEQ_BITS)")
    ap.add_argument("--skip_pillow", action="store_true", help="no Pillow worker yardstick (the routes' split only)")
    a = ap.parse_args()
    H, W = (int(v) for v in a.size.split("x"))
    files = make_files(a.frames, H, W)
    lines = [f"JPEG decode: {a.frames} frames of {H} x {W}, 4:2:0, quality 90, {sum(map(len, files)) / a.frames / 1024:.1f} KiB per file; "
             f"{a.reps} repetitions after 3 warm-up rounds"]

    t_pillow, sums = None, None
    if not a.skip_pillow:
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
    from PIL import Image

    routes = ["host", "device"] if a.entropy == "both" else [a.entropy]
    sweep = [int(v) for v in a.subseq_bits.split(",") if v] or [hip_ops.JPEG_SUBSEQ_BITS]
    want = {i: np.asarray(Image.open(io.BytesIO(files[i])).convert("RGB")) for i in range(0, a.frames, 16)}
    for route in routes:
        for bits in (sweep if route == "device" else [None]):
            frames = hip_ops.decode_jpeg_batch(files, dev, a.threads, entropy=route, subseq_bits=bits)
            torch.cuda.synchronize()
            what = f"entropy on the {route}" + (f", {bits} bits per lane" if bits else "")
            if sums is not None:
                lines.append(f"{what}: pixels equal Pillow's on all {a.frames} frames (sum check): {[int(f.sum().item()) for f in frames] == sums}")
            lines.append(f"{what}: pixels equal Pillow's bit for bit on every 16th frame: {all(np.array_equal(frames[i].cpu().numpy(), w) for i, w in want.items())}")

    n = a.frames
    ev = lambda: torch.cuda.Event(enable_timing=True)
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def rep_host():
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        batch = hip_ops.jpeg_scan_batch(files, a.threads)
        w1 = time.perf_counter()
        table = batch.part("frames")
        ws_bytes = int(lib.tt_jpeg_decode_batch_workspace_bytes(table.ctypes.data, n))
        out = torch.empty(batch.out_bytes, dtype=torch.uint8, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        coeffs = batch.coeffs.to(dev, non_blocking=True)
        meta = batch.meta.to(dev, non_blocking=True)
        e1.record()
        at = lambda name: meta.data_ptr() + batch.layout[name][0]
        rc = lib.tt_jpeg_decode_batch(coeffs.data_ptr(), batch.n_coeffs, at("qtables"), 3 * n, table.ctypes.data, at("frames"), n, out.data_ptr(),
                                      out.numel(), ws.data_ptr(), ws.numel(), stream())
        assert rc == 0
        e2.record()
        torch.cuda.synchronize()
        w2 = time.perf_counter()
        return {"host": w1 - w0, "h2d": e0.elapsed_time(e1) * 1e-3, "kern": e1.elapsed_time(e2) * 1e-3, "all": w2 - w0,
                "sizes": (batch.n_coeffs, batch.out_bytes, 2 * batch.n_coeffs)}       # (the batch itself is dropped: its pinned buffers go back to the pool)

    def rep_device(bits):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        batch = hip_ops.jpeg_prepare_batch(files, a.threads)
        w1 = time.perf_counter()
        table, streams, segs = batch.part("frames"), batch.part("streams"), batch.part("segs")
        ws_bytes = int(lib.tt_jpeg_decode_batch_workspace_bytes(table.ctypes.data, n))
        out = torch.empty(batch.out_bytes, dtype=torch.uint8, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        coeffs = torch.empty(batch.n_coeffs, dtype=torch.int16, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        stats = torch.empty(int(lib.tt_jpeg_entropy_batch_workspace_bytes(streams.ctypes.data, n, bits)), dtype=torch.uint8, device=dev)
        e0, e1, e2, e3 = ev(), ev(), ev(), ev()
        e0.record()
        meta = batch.meta.to(dev, non_blocking=True)
        e1.record()
        at = lambda name: meta.data_ptr() + batch.layout[name][0]
        rc = lib.tt_jpeg_entropy_batch(at("scan"), batch.layout["scan"][1], segs.ctypes.data, at("segs"), batch.n_segs, streams.ctypes.data,
                                       at("streams"), n, bits, coeffs.data_ptr(), batch.n_coeffs, status.data_ptr(), stats.data_ptr(), stats.numel(),
                                       stream())
        assert rc == 0
        e2.record()
        rc = lib.tt_jpeg_decode_batch(coeffs.data_ptr(), batch.n_coeffs, at("qtables"), 3 * n, table.ctypes.data, at("frames"), n, out.data_ptr(),
                                      out.numel(), ws.data_ptr(), ws.numel(), stream())
        assert rc == 0
        e3.record()
        bad = int((status.cpu() != 0).sum())          # the route's one read-back: inside the end-to-end time
        w2 = time.perf_counter()
        assert bad == 0
        return {"host": w1 - w0, "h2d": e0.elapsed_time(e1) * 1e-3, "entropy": e1.elapsed_time(e2) * 1e-3, "kern": e2.elapsed_time(e3) * 1e-3,
                "all": w2 - w0, "sizes": (batch.n_coeffs, batch.out_bytes, batch.meta.numel()), "stats": stats[:16 * n].view(torch.int32).view(n, 4).cpu().numpy()}

    runs = [("host", None)] * ("host" in routes) + [("device", b) for b in sweep] * ("device" in routes)
    times = {r: [] for r in runs}
    for rep in range(a.reps + 3):          # the routes alternate inside a repetition
        for r in runs:
            t = rep_host() if r[0] == "host" else rep_device(r[1])
            if rep >= 3:
                times[r].append(t)
    med = lambda v: float(np.median(v))
    spread = lambda v: f"min {min(v) * 1e3:.2f} / max {max(v) * 1e3:.2f}"
    col = lambda r, k: [t[k] for t in times[r]]
    for r in runs:
        (n_coeffs, out_bytes, copied), t_all = times[r][-1]["sizes"], col(r, "all")
        name = "host entropy (N21)" if r[0] == "host" else f"device entropy (N24), {r[1]} bits per lane"
        lines.append(f"{name}, {a.threads} host threads: {med(t_all) * 1e3:8.2f} ms per batch = {a.frames / med(t_all):9.0f} frames/s   (end to end, "
                     f"median; {spread(t_all)} ms)")
        t_host, t_h2d, t_kern = col(r, "host"), col(r, "h2d"), col(r, "kern")
        if r[0] == "host":
            lines.append(f"  host scan (markers + Huffman)  : {med(t_host) * 1e3:8.2f} ms   ({spread(t_host)})  = {a.frames / med(t_host):.0f} frames/s")
            lines.append(f"  host-to-device copies          : {med(t_h2d) * 1e3:8.2f} ms   ({spread(t_h2d)})  {copied / 1e6:.1f} MB of coefficients = "
                         f"{copied / med(t_h2d) / 1e9:.1f} GB/s; the decoded RGB would be {out_bytes / 1e6:.1f} MB")
        else:
            lines.append(f"  host prepare (markers + copy)  : {med(t_host) * 1e3:8.2f} ms   ({spread(t_host)})  = {a.frames / med(t_host):.0f} frames/s")
            lines.append(f"  host-to-device copy            : {med(t_h2d) * 1e3:8.2f} ms   ({spread(t_h2d)})  {copied / 1e6:.2f} MB of streams and tables = "
                         f"{copied / med(t_h2d) / 1e9:.1f} GB/s; the coefficients would be {2 * n_coeffs / 1e6:.1f} MB")
            t_ent, st = col(r, "entropy"), times[r][-1]["stats"]
            lines.append(f"  entropy launch (+ memset)      : {med(t_ent) * 1e3:8.2f} ms   ({spread(t_ent)})  per frame: {st[:, 2].mean():.0f} subsequences in "
                         f"{st[:, 1].max()} tile(s), rounds median {int(np.median(st[:, 0]))} / max {st[:, 0].max()}")
        moved = 2 * n_coeffs + n_coeffs + n_coeffs + out_bytes      # IDCT: coefficients in, planes out; colour: planes in, RGB out
        rate = moved / med(t_kern)
        lines.append(f"  the two launches               : {med(t_kern) * 1e3:8.2f} ms   ({spread(t_kern)})  {moved / 1e6:.1f} MB moved = {rate / 1e9:.0f} GB/s = "
                     f"{100 * rate / HBM_MEASURED:.1f} % of the measured HBM copy rate ({HBM_MEASURED / 1e12:.2f} TB/s), {100 * rate / HBM_SPEC:.1f} % of the "
                     f"{HBM_SPEC / 1e12:.0f} TB/s data-sheet figure (event time of both launches, launch gaps included)")
        if t_pillow is not None:
            ratio = t_pillow / med(t_all)
            lines.append(f"  this route / Pillow at {a.threads} host CPUs each: {ratio:.2f} x" + ("" if ratio > 1 else "  (NOT faster)"))
    if len(runs) > 1 and runs[0][0] == "host":
        for r in runs[1:]:
            lines.append(f"device entropy at {r[1]} bits / host entropy, end to end: {med(col(runs[0], 'all')) / med(col(r, 'all')):.2f} x")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
