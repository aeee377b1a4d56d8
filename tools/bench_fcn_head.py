"""Times the FCN head (N32) on one GPU: the fused head step of ``FCNFinetune`` and each token-grid convolution launch, next to the same
head as ``nn.Conv2d`` modules under torch autograd in fp32, channels-last - what a user of the parent commit would write.

    python tools/bench_fcn_head.py [--out profiles/n32_fcn_head.txt] [--no-torch]

HIP events, 2 warm-up + 5 timed repetitions, medians; the two routes alternate inside a repetition.  Shape: B = 60, g = 28, D = 384,
channels = 512, C = 21, R = 100.  TFLOP/s are 2 rows 9 Cin Cout per convolution product against the 157 TFLOP/s f32-matrix peak."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from timetuning_amd import fcn_finetune as FF, hip_ops as ops, synth  # noqa: E402

PEAK = 157.0


class _Stub(nn.Module):
    def __init__(self, D):
        super().__init__()
        self.backbone = nn.Module()
        self.backbone.embed_dim = D
        self.feature_dim = D
        self.keep = nn.Parameter(torch.zeros(1))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


class TorchHead(nn.Module):
    def __init__(self, D, ch, C, p):
        super().__init__()
        self.c0, self.c1, self.cat = nn.Conv2d(D, ch, 3, padding=1), nn.Conv2d(ch, ch, 3, padding=1), nn.Conv2d(D + ch, ch, 3, padding=1)
        self.drop, self.seg = nn.Dropout2d(p), nn.Conv2d(ch, C, 1)

    def forward(self, x, R):
        h = F.relu(self.c1(F.relu(self.c0(x))))
        h = self.drop(F.relu(self.cat(torch.cat([x, h], 1))))
        return F.interpolate(self.seg(h), size=(R, R), mode="bilinear", align_corners=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, g, D, ch, C, R = 60, 28, 384, 512, 21, 100
    rows, grid = B * g * g, (g, g)
    feats = torch.from_numpy(synth.normal("bench.fcn.x", (B, g * g, D))).to(dev)
    labels = torch.from_numpy(np.random.default_rng(0).integers(0, C, (B, R, R))).to(dev)
    model = FF.FCNFinetune(_Stub(D), C, R, channels=ch).to(dev).train()
    h = model.decode_head
    convs = {"convs.0": (h.convs[0].conv, D, 0), "convs.1": (h.convs[1].conv, ch, 0), "conv_cat": (h.conv_cat.conv, D, ch)}
    xs = {k: (torch.from_numpy(synth.normal(f"bench.fcn.{k}.a", (B, g * g, ca))).to(dev),
              torch.from_numpy(synth.normal(f"bench.fcn.{k}.b", (B, g * g, cb))).to(dev) if cb else None) for k, (_, ca, cb) in convs.items()}
    dpre = torch.from_numpy(synth.normal("bench.fcn.dpre", (B, g * g, ch))).to(dev)
    use_torch = not args.no_torch
    if use_torch:
        ref = TorchHead(D, ch, C, h.dropout_ratio).to(dev).to(memory_format=torch.channels_last).train()
        x_cl = feats.view(B, g, g, D).permute(0, 3, 1, 2)                      # NCHW view of NHWC memory: channels-last
        tx = {k: torch.cat([t.view(B, g, g, -1) for t in v if t is not None], 3).permute(0, 3, 1, 2) for k, v in xs.items()}
        tw = {"convs.0": ref.c0.weight, "convs.1": ref.c1.weight, "conv_cat": ref.cat.weight}
        tg = dpre.view(B, g, g, ch).permute(0, 3, 1, 2)
        cb = torch.ops.aten.convolution_backward

    def hip_step():
        model.zero_grad(set_to_none=True)
        model.head_loss(feats, labels).backward()

    def torch_step():
        ref.zero_grad(set_to_none=True)
        F.cross_entropy(ref(x_cl, R), labels, ignore_index=255).backward()

    jobs = {"step": (hip_step, torch_step if use_torch else None)}
    for k, (m, ca, cb_) in convs.items():
        xa, xb = xs[k]
        w, b = m.weight.detach(), m.bias.detach()
        jobs[f"{k}.fwd"] = (lambda xa=xa, xb=xb, w=w, b=b: ops.conv3x3_tokens(xa, w, b, xb=xb, grid=grid, act=1),
                            (lambda k=k: F.relu(F.conv2d(tx[k], tw[k], None, padding=1))) if use_torch else None)
        jobs[f"{k}.bwd_data"] = (lambda w=w: ops.conv3x3_tokens_bwd_data(dpre, w, grid),
                                 (lambda k=k: cb(tg, tx[k], tw[k], None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [True, False, False]))
                                 if use_torch else None)
        jobs[f"{k}.bwd_weight"] = (lambda xa=xa, xb=xb: ops.conv3x3_tokens_bwd_weight(dpre, xa, xb, grid),
                                   (lambda k=k: cb(tg, tx[k], tw[k], [ch], [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, True]))
                                   if use_torch else None)
    times = {k: ([], []) for k in jobs}
    for rep in range(args.warmup + args.reps):
        for k, (hip, tor) in jobs.items():
            th = timed(hip)
            tt = timed(tor) if tor else float("nan")
            if rep >= args.warmup:
                times[k][0].append(th)
                times[k][1].append(tt)
    lines = [f"# FCN head, B {B} g {g} D {D} channels {ch} C {C} R {R}: medians of {args.reps} after {args.warmup} warm-up, HIP events, routes alternating",
             f"# device: {torch.cuda.get_device_name(0)}; torch route: {'nn.Conv2d, fp32, channels-last' if use_torch else 'not run'}",
             f"{'what':<22}{'hip ms':>10}{'hip TF/s':>10}{'% peak':>8}{'torch ms':>10}{'torch TF/s':>11}"]
    for k, (th, tt) in times.items():
        mh, mt = statistics.median(th), statistics.median(tt)
        if k == "step":
            lines.append(f"{k:<22}{mh:>10.3f}{'':>10}{'':>8}{mt:>10.3f}")
            continue
        _, ca, cb_ = convs[k.split(".fwd")[0].split(".bwd")[0]]
        fl = 2.0 * rows * 9 * (ca + cb_) * ch / 1e9
        lines.append(f"{k:<22}{mh:>10.3f}{fl / mh:>10.1f}{100 * fl / mh / PEAK:>8.1f}{mt:>10.3f}{fl / mt:>11.1f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
