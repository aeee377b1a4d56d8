#!/usr/bin/env python3
"""Times one linear-probe training step (N5) at the reference's shape: B 60, dino-s16 at 448^2 (28 x 28 tokens, D 384), 21 classes,
mask 100.  Reports, each with its peak memory above what was allocated before it:
  backbone    the frozen-backbone forward (LinearFinetune._features), which every step pays
  fused       the head step on given features: tt_probe_logits -> tt_probe_upsample_ce -> tt_probe_wgrad -> FusedSGD
  reference   the same head step in the reference's order with torch ops on the GPU: interpolate the D channels to the mask size,
              1x1 conv, CrossEntropyLoss(ignore_index=255), backward, torch.optim.SGD (linear_finetune.py:23-31,81-85)
and the fused and reference losses / head gradients of the first step, which must agree.  Synthetic weights and data.

    python tools/bench_linear_probe.py [--batch 60] [--iters 20] [--out result.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import timetuning_amd  # noqa: E402,F401
from timetuning_amd import linear_finetune as L  # noqa: E402


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=60)
    ap.add_argument("--resolution", type=int, default=448)
    ap.add_argument("--mask_size", type=int, default=100)
    ap.add_argument("--classes", type=int, default=21)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, R, C = a.batch, a.mask_size, a.classes
    fe = FeatureExtractor("dino-s16", "", [1024, 1024, 512, 256], return_attention=False)
    model = L.LinearFinetune(TimeT(fe, 200), C, R).to(dev)
    x, y01 = L.synthetic_segmentation(B, a.resolution, C, seed=1)
    x = x.to(dev)
    labels = L.prepare_labels(y01.to(dev), R)
    feats = model._features(x, False)
    _, n, D = feats.shape
    g = int(round(n ** 0.5))
    res = dict(batch=B, tokens=f"{g}x{g}", D=D, classes=C, mask=R, resolution=a.resolution, iters=a.iters)

    res["backbone_ms"], res["backbone_peak_mib"] = _time(lambda: model._features(x, False), a.iters, a.warmup)

    head = model.finetune_head
    opt = L.FusedSGD(head.parameters(), lr=0.01, momentum=0.9, weight_decay=0.0001)

    def fused():
        loss = model.head_loss(feats, labels)
        opt.zero_grad()
        loss.backward()
        opt.step()

    # the reference order on a copy of the head, with stock torch ops
    ref_head = torch.nn.Conv2d(D, C, 1).to(dev)
    ref_head.load_state_dict(head.state_dict())
    ref_opt = torch.optim.SGD(ref_head.parameters(), lr=0.01, momentum=0.9, weight_decay=0.0001)
    crit = torch.nn.CrossEntropyLoss(ignore_index=255)
    f4 = feats.permute(0, 2, 1).reshape(B, D, g, g)

    def reference():
        with torch.no_grad():
            up = F.interpolate(f4, size=(R, R), mode="bilinear")
        loss = crit(ref_head(up), labels)
        ref_opt.zero_grad()
        loss.backward()
        ref_opt.step()
        return loss

    # agreement of one step from the same head (before any update)
    lf = model.head_loss(feats, labels)
    lf.backward()
    lr_ = crit(ref_head(F.interpolate(f4, size=(R, R), mode="bilinear")), labels)
    lr_.backward()
    res["loss_fused"], res["loss_reference"] = lf.item(), lr_.item()
    res["dw_rel_err"] = float((head.weight.grad - ref_head.weight.grad).abs().max() / ref_head.weight.grad.abs().max())
    head.zero_grad(set_to_none=True)
    ref_head.zero_grad(set_to_none=True)

    res["fused_head_step_ms"], res["fused_head_step_peak_mib"] = _time(fused, a.iters, a.warmup)
    res["reference_head_step_ms"], res["reference_head_step_peak_mib"] = _time(reference, a.iters, a.warmup)
    res["bytes_floor_fused_mb"] = (B * n * D * 4 * 2 + B * R * R * 8) / 1e6       # feats read twice (logits, wgrad) + labels
    res["bytes_reference_upsampled_mb"] = B * D * R * R * 4 / 1e6
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
