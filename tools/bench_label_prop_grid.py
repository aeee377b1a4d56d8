#!/usr/bin/env python3
"""N9: label propagation on rectangular token grids at native frame size (480 x 848), one clip of 50 frames, K = 5 classes.

Cases: ViT-S/16 (30 x 53 tokens) and ViT-S/8 (60 x 106) with radius 12 and n_last_frames 4 and 7; radius 0 (no mask) at 30 x 53; and
for comparison the square entry at 28 x 28 (radius 12, n_last 4).  Prints one JSON line per case:
  - ``prop_ms_per_frame``: ``label_propagate_grid_maps`` (the square entry for the 28 x 28 row) over the 49 target frames, device
    events around the call (workspace allocation included), median of ``--iters`` after a warm-up, divided by 49;
  - ``upsample_ms_per_frame``: ``upsample_argmax_hw`` of the 49 maps to 480 x 848, the same way;
  - ``backbone_ms_per_frame``: the extractor forward (no head) of the 50 frames in batches of 10, per frame (none for 28 x 28);
  - ``workspace_bytes``: what ``tt_label_propagate_grid_workspace_bytes`` asks for;
  - computed floors per target frame (from shapes, not measured): the similarity GEMMs' FLOPs at the 155 TFLOP/s fp32 MFMA rate, and
    the similarity buffer written once and read once at 6.3 TB/s (the measured HBM copy rate).

    python tools/bench_label_prop_grid.py [--iters 3] [--frames 50]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from timetuning_amd import _lib, synth  # noqa: E402
from timetuning_amd import hip_ops as ops  # noqa: E402

FP32_FLOPS = 155e12
HBM_BPS = 6.3e12
H, W, K = 480, 848, 5


def time_events(fn, iters, warmup=1):
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


def floors(fs, n, D, n_last):
    """Per target frame, averaged over the clip: GEMM FLOPs of the context slots in use and the similarity bytes (written + read once)."""
    slots = sum(1 + min(t - 1, n_last) for t in range(1, fs))
    flops = 2.0 * n * n * D * slots / (fs - 1)
    nbytes = 2.0 * 4 * n * n * slots / (fs - 1)
    return flops / FP32_FLOPS * 1e3, nbytes / HBM_BPS * 1e3


def backbone_ms(arch, clip, iters):
    from timetuning_amd.models import FeatureExtractor

    fe = FeatureExtractor(arch, "", [], return_attention=False).cuda().eval()
    out = {}

    def run():
        out["f"] = torch.cat([fe(clip[i:i + 10], use_head=False)[0] for i in range(0, clip.shape[0], 10)])

    ms = time_events(run, iters)
    return ms / clip.shape[0], out["f"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--frames", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_prop_grid: needs a GPU (nothing here is measured on the host)")
    lib = _lib.load()
    fs = a.frames
    clip = torch.from_numpy(synth.normal("lpg.bench.clip", (fs, 3, H, W))).cuda()
    rng = np.random.default_rng(0)
    cases = [("dino-s16", 12, 4), ("dino-s16", 12, 7), ("dino-s16", 0, 4), ("dino-s8", 12, 4), ("dino-s8", 12, 7)]
    feats = {}
    for arch, radius, n_last in cases:
        P = synth.ARCHS[arch]["patch_size"]
        gh, gw = H // P, W // P
        n = gh * gw
        row = dict(case=f"{arch} {H}x{W} -> {gh}x{gw} tokens, r={radius}, n_last={n_last}", frames=fs, K=K)
        if arch not in feats:
            row["backbone_ms_per_frame"], f = backbone_ms(arch, clip, a.iters)
            feats[arch] = ops.l2norm_fwd(f.reshape(-1, f.shape[-1]).contiguous().float()).view(fs, 1, n, -1)
            del f
        xn = feats[arch]
        D = xn.shape[-1]
        seed = torch.from_numpy(rng.dirichlet(np.ones(K), n).astype(np.float32)).view(1, n, K).cuda()
        row["workspace_bytes"] = int(lib.tt_label_propagate_grid_workspace_bytes(1, fs, gh, gw, D, K, n_last, radius))
        out = {}

        def prop():
            out["m"] = ops.label_propagate_grid_maps(xn, seed, (gh, gw), n_last, radius, 5, 0.1)

        row["prop_ms_per_frame"] = time_events(prop, a.iters) / (fs - 1)
        maps = out["m"].view(fs - 1, n, K)
        row["upsample_ms_per_frame"] = time_events(lambda: ops.upsample_argmax_hw(maps, (gh, gw), (H, W)), a.iters) / (fs - 1)
        row["gemm_floor_ms_per_frame"], row["sims_bytes_floor_ms_per_frame"] = floors(fs, n, D, n_last)
        print(json.dumps(row), flush=True)
        del out, maps
        torch.cuda.empty_cache()
    # the square entry at 28 x 28 (what a 448 x 448 ViT-S/16 or 224 x 224 ViT-S/8 clip gives), for comparison
    g, n_last, D = 28, 4, 384
    n = g * g
    x = torch.from_numpy(synth.normal("lpg.bench.sq", (fs * n, D))).cuda()
    xn = ops.l2norm_fwd(x).view(fs, 1, n, D)
    seed = torch.from_numpy(rng.dirichlet(np.ones(K), n).astype(np.float32)).view(1, n, K).cuda()
    row = dict(case=f"square entry 28x28 tokens, r=12, n_last={n_last}", frames=fs, K=K,
               workspace_bytes=int(lib.tt_label_propagate_workspace_bytes(1, fs, g, D, K, n_last)))
    out = {}

    def prop_sq():
        out["m"] = ops.label_propagate_maps(xn, seed, n_last, 12, 5, 0.1)

    row["prop_ms_per_frame"] = time_events(prop_sq, a.iters) / (fs - 1)
    row["grid_entry_same_shape_ms_per_frame"] = time_events(
        lambda: ops.label_propagate_grid_maps(xn, seed, (g, g), n_last, 12, 5, 0.1), a.iters) / (fs - 1)
    maps = out["m"].view(fs - 1, n, K)
    row["upsample_ms_per_frame"] = time_events(lambda: ops.upsample_argmax(maps, 448), a.iters) / (fs - 1)
    row["gemm_floor_ms_per_frame"], row["sims_bytes_floor_ms_per_frame"] = floors(fs, n, D, n_last)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
