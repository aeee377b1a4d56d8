#!/usr/bin/env python3
"""Times the stem gradients (N19) on one GPU.

1. ``tt_patch_embed_bwd``'s weight gradient (the patches gathered from the frames inside the kernel) against the materialised route:
   ``torch.nn.functional.unfold`` + the gather of dtok's patch rows (torch) followed by ``ops.linear_bwd_weight``.  The materialised
   route is timed whole (it is what a caller without the fused kernel would run) and its GEMM alone.  Shapes: ViT-S/16 at 6 272 rows
   (the 32 target frames of BASELINE C2), ViT-S/16 at 25 088 rows (all 128 frames), ViT-B/16 at 6 272 rows and ViT-S/8 at 12 544 rows
   (K = 192).  Also the whole call with its four outputs (dw, dbias, dcls, dtable).
   Device events around each launch sequence, ``--warmup`` (3) calls, then the median and minimum of ``--reps`` (20) timed calls; the
   two routes alternate call by call.  Random data; the results are compared before anything is timed.
2. One C2 training step (32 clips x 4 frames of ViT-S/16, K = 200, the driver's "f16x3" arithmetic, ``TimeT.train_update`` included) with
   the default ``unfreeze_layers`` (blocks.11, blocks.10) and with everything trainable (blocks, patch_embed, pos_embed, cls_token): wall
   clock around ``torch.cuda.synchronize()``, ``--step_warmup`` (5) steps, then ``--steps`` (20), the two models in turn, twice.

Prints one JSON line per measurement.  ``--only kernels|step`` restricts the run.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

SHAPES = [("ViT-S/16 6272 rows", 32, 3, 224, 224, 16, 384), ("ViT-S/16 25088 rows", 128, 3, 224, 224, 16, 384),
          ("ViT-B/16 6272 rows", 32, 3, 224, 224, 16, 768), ("ViT-S/8 12544 rows", 16, 3, 224, 224, 8, 384)]


def timed(fns, warmup, reps, torch):
    """Median / minimum device milliseconds of each callable, alternating between them call by call."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    return [(statistics.median(m), min(m)) for m in ms]


def kernels(args, torch, ops, lib):
    import torch.nn.functional as F

    for name, Fr, C, H, W, P, D in SHAPES:
        n, K = (H // P) * (W // P), C * P * P
        gen = torch.Generator(device="cuda").manual_seed(1)
        img = torch.randn((Fr, C, H, W), device="cuda", generator=gen)
        dtok = torch.randn((Fr, n + 1, D), device="cuda", generator=gen)
        ws = torch.empty(lib.tt_patch_embed_bwd_workspace_bytes(Fr, C, H, W, P, D), dtype=torch.uint8, device="cuda")
        dw = torch.empty((D, K), device="cuda")
        outs = dict(dw_out=dw, dbias_out=torch.empty(D, device="cuda"), dcls_out=torch.empty(D, device="cuda"),
                    dtable_out=torch.empty((n + 1, D), device="cuda"))

        def fused():
            ops.patch_embed_bwd(dtok, img, P, need=("dw",), dw_out=dw, workspace=ws)

        def fused_all():
            ops.patch_embed_bwd(dtok, img, P, workspace=ws, **outs)

        def rows_of():
            return (F.unfold(img, P, stride=P).transpose(1, 2).reshape(Fr * n, K).contiguous(), dtok[:, 1:].reshape(Fr * n, D).contiguous())

        def materialised():
            x, dy = rows_of()
            return ops.linear_bwd_weight(dy, x, need_bias=False)[0]

        x_kept, dy_kept = rows_of()

        def gemm_alone():
            return ops.linear_bwd_weight(dy_kept, x_kept, need_bias=False)[0]

        fused()
        ref = materialised()
        err = float((dw - ref).abs().max() / ref.abs().max())
        (f_med, f_min), (a_med, a_min), (m_med, m_min), (g_med, g_min) = timed([fused, fused_all, materialised, gemm_alone], args.warmup, args.reps, torch)
        flop = 2.0 * Fr * n * D * K
        print(json.dumps({"what": "patch weight gradient", "shape": name, "F": Fr, "rows": Fr * n, "D": D, "K": K,
                          "fused_ms": [round(f_med, 4), round(f_min, 4)], "fused_four_outputs_ms": [round(a_med, 4), round(a_min, 4)],
                          "materialised_ms": [round(m_med, 4), round(m_min, 4)], "materialised_gemm_alone_ms": [round(g_med, 4), round(g_min, 4)],
                          "fused_tflops": round(flop / (f_med * 1e-3) / 1e12, 2), "materialised_over_fused": round(m_med / f_med, 3),
                          "gemm_alone_over_fused": round(g_med / f_med, 3), "max_normalised_difference": err,
                          "workspace_MB": round(ws.numel() / 2 ** 20, 2), "stat": "median, min of %d" % args.reps}), flush=True)


def step(args, torch, ops):
    from timetuning_amd import synth
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.my_utils import cosine_scheduler
    from timetuning_amd.time_tuning import SwavOptimizer, TimeT

    bs, fs, K = 32, 4, 200
    ops.set_gemm_precision("f16x3")
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=1)).cuda()
    total = 4 * (args.steps + args.step_warmup) + 8
    models = {}
    for name, layers in (("default", ["blocks.11", "blocks.10"]), ("everything", ["blocks", "patch_embed", "pos_embed", "cls_token"])):
        fe = FeatureExtractor("dino-s16", "", [1024, 1024, 512, 256], unfreeze_layers=layers, init="dino", return_attention=False, train_stem=True)
        m = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, fe.feature_dim))).cuda()
        o = SwavOptimizer(m, "AdamW", True, 1e-5, 1e-4, "CosineAnnealingLR", cosine_scheduler(0.04, 0.4, 1, total), total, 1)
        models[name] = (m, o, sum(p.numel() for p in m.parameters() if p.requires_grad))

    def one(m, o):
        loss = m(x, None, True, False)
        m.train_update(o, loss, 0)
        return loss

    for rnd in range(2):
        for name, (m, o, count) in models.items():
            for _ in range(args.step_warmup):
                one(m, o)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = one(m, o)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            print(json.dumps({"what": "C2 step", "unfreeze": name, "round": rnd + 1, "ms_per_step": round(ms, 3), "trainable_parameters": count,
                              "loss": round(float(loss.item()), 5), "steps": args.steps, "precision": "f16x3"}), flush=True)
    ops.set_gemm_precision("f32")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step_warmup", type=int, default=5)
    ap.add_argument("--only", choices=["kernels", "step"], default=None)
    args = ap.parse_args(argv)

    import torch

    import timetuning_amd  # noqa: F401
    from timetuning_amd import _lib
    from timetuning_amd import hip_ops as ops

    if not torch.cuda.is_available():
        raise SystemExit("bench_stem_grad.py needs a GPU: there is nothing to time without one")
    if args.only != "step":
        kernels(args, torch, ops, _lib.load())
    if args.only != "kernels":
        step(args, torch, ops)


if __name__ == "__main__":
    main()
