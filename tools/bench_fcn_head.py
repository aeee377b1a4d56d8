"""Times the FCN head (N32) on one GPU: the fused head step of ``FCNFinetune`` and each token-grid convolution launch, next to the same
head as ``nn.Conv2d`` modules under torch autograd in fp32, channels-last - what a user of the parent commit would write.

    python tools/bench_fcn_head.py [--out profiles/n32_fcn_head.txt] [--no-torch] [--norm bn]

``--norm bn`` (N33) times the head with norm layers instead: its fused step beside the step without them (the same tree, alternating) and
beside ``nn.Conv2d(bias=False) + nn.BatchNorm2d + ReLU``, and each batch-normalisation entry on [B g g, channels] - 20 enqueued calls
between two events, bytes / time beside the floor of 3 (forward) and 5 (backward) tensors over the 6.29 TB/s measured copy rate.

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
COPY_TBS = 6.29   # measured copy rate, MI355X_MICROARCH.md


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
    def __init__(self, D, ch, C, p, norm=False):
        super().__init__()

        def module(cin):
            conv = nn.Conv2d(cin, ch, 3, padding=1, bias=not norm)
            return nn.Sequential(conv, nn.BatchNorm2d(ch)) if norm else conv

        self.c0, self.c1, self.cat = module(D), module(ch), module(D + ch)
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
    ap.add_argument("--norm", choices=("none", "bn"), default="none")
    args = ap.parse_args()
    if args.norm == "bn":
        return main_bn(args)
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


def main_bn(args):
    from timetuning_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    B, g, D, ch, C, R = 60, 28, 384, 512, 21, 100
    rows, n = B * g * g, g * g
    feats = torch.from_numpy(synth.normal("bench.fcn.x", (B, n, D))).to(dev)
    labels = torch.from_numpy(np.random.default_rng(0).integers(0, C, (B, R, R))).to(dev)
    plain = FF.FCNFinetune(_Stub(D), C, R, channels=ch).to(dev).train()
    model = FF.FCNFinetune(_Stub(D), C, R, channels=ch, norm_cfg=dict(type="BN", requires_grad=True)).to(dev).train()
    use_torch = not args.no_torch
    if use_torch:
        ref = TorchHead(D, ch, C, model.decode_head.dropout_ratio, norm=True).to(dev).to(memory_format=torch.channels_last).train()
        x_cl = feats.view(B, g, g, D).permute(0, 3, 1, 2)

    def step_of(m):
        def run():
            m.zero_grad(set_to_none=True)
            m.head_loss(feats, labels).backward()
        return run

    def torch_step():
        ref.zero_grad(set_to_none=True)
        F.cross_entropy(ref(x_cl, R), labels, ignore_index=255).backward()

    # the batch-normalisation entries on preallocated buffers, 20 enqueued calls per timing
    z = torch.from_numpy(synth.normal("bench.bn.z", (B, n, ch))).to(dev)
    gr = torch.from_numpy(synth.normal("bench.bn.g", (B, n, ch))).to(dev)
    y, dz = torch.empty_like(z), torch.empty_like(z)
    gamma, beta, rm, rv = torch.ones(ch, device=dev), torch.zeros(ch, device=dev), torch.zeros(ch, device=dev), torch.ones(ch, device=dev)
    sm, sr, dgam, dbet = (torch.empty(ch, device=dev) for _ in range(4))
    scale = model.dropout_scale(B, dev)
    nb = lib.tt_bn_tokens_fwd_workspace_bytes(rows, ch)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    p = lambda t: None if t is None else t.data_ptr()
    CALLS = 20

    def many(call):
        def run():
            s = torch.cuda.current_stream().cuda_stream
            for _ in range(CALLS):
                assert call(s) == 0
        return run

    def fwd(training, sc):
        return lambda s: lib.tt_bn_tokens_fwd(p(z), p(gamma), p(beta), p(sc), p(rm), p(rv), p(y), p(sm), p(sr), rows, n, ch, training, 1, 0.1, 1e-5,
                                              p(ws), nb, s)

    bwd = lambda s: lib.tt_bn_tokens_bwd(p(gr), p(z), p(sm), p(sr), p(gamma), p(dz), p(dgam), p(dbet), rows, ch, p(ws), nb, s)
    if use_torch:
        bn_t = nn.BatchNorm2d(ch).to(dev).train()
        z_cl = z.view(B, g, g, ch).permute(0, 3, 1, 2).requires_grad_(True)
        g_cl = gr.view(B, g, g, ch).permute(0, 3, 1, 2)
        out_t = []

        def t_fwd():
            for _ in range(CALLS):
                out_t[:] = [bn_t(z_cl)]

        def t_bwd():
            for _ in range(CALLS):
                torch.autograd.grad(out_t[0], [z_cl, bn_t.weight, bn_t.bias], g_cl, retain_graph=True)

    tensor_mb = rows * ch * 4 / 1e6
    # name: (hip, torch, tensors moved, launches)
    jobs = {"step bn": (step_of(model), torch_step if use_torch else None, 0, 0), "step none": (step_of(plain), None, 0, 0),
            "bn fwd train": (many(fwd(1, None)), t_fwd if use_torch else None, 3, 2),
            "bn fwd train+scale": (many(fwd(1, scale)), None, 3, 2),
            "bn fwd eval": (many(fwd(0, None)), None, 2, 1),
            "bn bwd": (many(bwd), t_bwd if use_torch else None, 5, 2)}
    times = {k: ([], []) for k in jobs}
    for rep_ in range(args.warmup + args.reps):
        for k, (hip, tor, _, _) in jobs.items():
            th = timed(hip)
            tt = timed(tor) if tor else float("nan")
            if rep_ >= args.warmup:
                times[k][0].append(th)
                times[k][1].append(tt)
    lines = [f"# FCN head with norm layers (--norm bn), B {B} g {g} D {D} channels {ch} C {C} R {R}: medians of {args.reps} after {args.warmup} "
             f"warm-up, HIP events, routes alternating",
             f"# device: {torch.cuda.get_device_name(0)}; torch route: "
             f"{'nn.Conv2d(bias=False) + nn.BatchNorm2d + ReLU, fp32, channels-last' if use_torch else 'not run'}",
             f"# bn entries: [{rows}, {ch}] fp32 = {tensor_mb:.1f} MB per tensor, {CALLS} enqueued calls per timing, time per call; floor = "
             f"tensors x {tensor_mb:.1f} MB / {COPY_TBS} TB/s; torch: nn.BatchNorm2d forward (training) / autograd.grad of it, without the ReLU",
             f"{'what':<22}{'launches':>9}{'hip ms':>10}{'TB/s':>8}{'floor ms':>10}{'% floor':>9}{'torch ms':>10}"]
    for k, (th, tt) in times.items():
        mh, mt = statistics.median(th), statistics.median(tt)
        _, _, tensors, launches = jobs[k]
        if not tensors:
            lines.append(f"{k:<22}{'':>9}{mh:>10.3f}{'':>8}{'':>10}{'':>9}{mt:>10.3f}")
            continue
        mh, mt = mh / CALLS, mt / CALLS
        floor = tensors * tensor_mb / 1e6 / COPY_TBS * 1e3
        lines.append(f"{k:<22}{launches:>9}{mh:>10.4f}{tensors * tensor_mb / 1e6 / mh * 1e3:>8.2f}{floor:>10.4f}{100 * floor / mh:>9.1f}{mt:>10.4f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
