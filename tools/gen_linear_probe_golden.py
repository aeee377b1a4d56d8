#!/usr/bin/env python3
"""Writes tests/golden/linear_probe.npz from the reference's own ``linear_finetune.LinearFinetune`` (N5).

Runs on the CPU of the build container, next to a reference checkout (``oracle/gen_golden.py``'s stand-ins for the third-party
imports), with ``MKL_CBWR=COMPATIBLE`` like every golden here:

    MKL_CBWR=COMPATIBLE python tools/gen_linear_probe_golden.py

The model is ``LinearFinetune(TimeT(FeatureExtractor("dino-s8", ...)), 21, R)`` with synthetic weights (embed 384, depth 2,
6 heads, patch 8: 28 x 28 tokens at 224^2, the grid the reference hard-codes) and a head drawn from ``synth.normal``.  Stored: the
labels (some 255), the mask-resolution logits, the CrossEntropyLoss(ignore_index=255), the head gradients, the head parameters and
momentum buffers after 3 SGD steps (lr 0.01, momentum 0.9, wd 1e-4) with StepLR(1, 0.5), and the validation predictions of the
stepped head with their top-2 margins and PredsmIoU(linear_probe=True).  The inputs are NOT stored: the images and labels come from
``linear_finetune.synthetic_segmentation``, the head from ``synth.normal`` (``make_inputs`` below, restated by
tests/test_linear_probe_host.py) and the features from the oracle's backbone on the same synthetic weights; small samples of the
images and features are kept so that the tests can check they regenerate what the reference saw.
"""
from __future__ import annotations

import os
import sys

os.environ.setdefault("MKL_CBWR", "COMPATIBLE")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle"))   # timet_oracle, which oracle.gen_golden's stand-ins import by that name
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

from oracle.gen_golden import OUT, build_reference_model, import_reference, t2n  # noqa: E402

CFG = dict(embed_dim=384, depth=2, num_heads=6, patch_size=8)
B, RES, C, R = 2, 224, 21, 40
HEAD_LIST, K, MODE, SEED = [128, 64], 10, "dino", 3
STEPS = 3


def make_inputs():
    from timetuning_amd import synth
    from timetuning_amd.linear_finetune import synthetic_segmentation

    x, y01 = synthetic_segmentation(B, RES, C, seed=SEED)
    w = synth.normal("lp.golden.w", (C, CFG["embed_dim"], 1, 1), 0.05, 0.0, SEED)
    b = synth.normal("lp.golden.b", (C,), 0.1, 0.0, SEED)
    return x, y01, w, b


def main():
    import torch
    import torch.nn.functional as F

    ref = import_reference()
    import linear_finetune as lf   # the reference module (its leoloader import resolves under the stand-ins)
    import metrics as ref_metrics

    tt_model = build_reference_model(ref, "dino-s8", CFG, K, HEAD_LIST, MODE, SEED)
    model = lf.LinearFinetune(tt_model, C, R)
    x, y01, w, b = make_inputs()
    with torch.no_grad():
        model.finetune_head.weight.copy_(torch.from_numpy(w))
        model.finetune_head.bias.copy_(torch.from_numpy(b))
    # the reference's label preparation (linear_finetune.py:78-80)
    y = y01 * 255
    y = F.interpolate(y.float(), size=(R, R), mode="nearest")
    labels = y.long().squeeze(1)
    with torch.no_grad():
        feats, _ = tt_model(x, use_head=False)
    out = {"cfg": np.array([B, RES, C, R, CFG["embed_dim"], CFG["depth"], CFG["num_heads"], CFG["patch_size"], K, SEED], np.int64),
           "head_list": np.array(HEAD_LIST, np.int64), "mode": np.array(MODE), "labels": t2n(labels).astype(np.uint8),
           "x_sample": t2n(x[:, :, ::16, ::16]), "feats_sample": t2n(feats[:, ::49])}
    criterion = torch.nn.CrossEntropyLoss(ignore_index=255)
    logits = model(x, use_head=False)
    loss = criterion(logits, labels)
    loss.backward()
    out["logits"] = t2n(logits)
    out["loss"] = np.float64(loss.item())
    out["dw"] = t2n(model.finetune_head.weight.grad)
    out["db"] = t2n(model.finetune_head.bias.grad)
    model.zero_grad()
    opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=0.0001)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    for step in range(STEPS):
        loss = criterion(model(x, use_head=False), labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        out[f"loss_step{step}"] = np.float64(loss.item())
    out["w3"] = t2n(model.finetune_head.weight)
    out["b3"] = t2n(model.finetune_head.bias)
    out["mw3"] = t2n(opt.state[model.finetune_head.weight]["momentum_buffer"])
    out["mb3"] = t2n(opt.state[model.finetune_head.bias]["momentum_buffer"])
    # validate (linear_finetune.py:34-51) on the stepped head, restated on the CPU (the reference moves the batch to cuda)
    miou = ref_metrics.PredsmIoU(10, 10, involve_bg=True)
    miou.n_jobs = 1
    with torch.no_grad():
        gt = F.interpolate((y01 * 255).float(), size=(R, R), mode="nearest").squeeze(1)
        valid = gt != 255
        o = model(x)
        pred = torch.argmax(o, dim=1)
        top2 = o.topk(2, dim=1).values
        miou.update(gt[valid].flatten(), pred[valid].flatten())
    out["pred"] = t2n(pred).astype(np.uint8)
    out["margin"] = t2n(top2[:, 0] - top2[:, 1])
    out["miou"] = np.float64(miou.compute(True, linear_probe=True)[0])
    path = os.path.join(OUT, "linear_probe.npz")
    np.savez_compressed(path, **out)
    print(f"{path} written: loss {out['loss']:.6f}, steps {[float(out[f'loss_step{s}']) for s in range(STEPS)]}, mIoU {out['miou']:.4f}, "
          f"ignored {(t2n(labels) == 255).mean():.3f}")


if __name__ == "__main__":
    main()
