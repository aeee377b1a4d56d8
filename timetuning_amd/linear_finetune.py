"""Linear-probe fine-tuning with the reference's surface (``linear_finetune.py``) on the HIP kernels.

``LinearFinetune`` keeps the reference module (``linear_finetune.py:13-31``): a frozen backbone and a ``finetune_head =
nn.Conv2d(D, C, 1)``, so its ``state_dict`` keys are the reference's.  The reference upsamples the D feature channels to the mask size
and then applies the conv (``:23-31``); both are linear and the bilinear weights sum to 1, so here the conv runs at token
resolution and only the C logits are upsampled.  ``forward`` returns the mask-resolution logits with autograd to the
head, so the reference loop (``CrossEntropyLoss`` -> ``backward`` -> SGD, ``:81-85``) works unchanged; ``loss(x, y)`` is the fused
form of the same step, which never materialises the mask-resolution logits.  ``validate`` is ``:34-51``, ``FusedSGD`` is
``torch.optim.SGD`` on one kernel launch, and ``main`` is the training driver of ``:55-89`` on synthetic data (dataset readers are
out of scope, as in ``mask_propagation.py``).
"""
from __future__ import annotations

import argparse
import math
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import hip_ops as ops
from .data_loader import add_decode_arguments
from .metrics import PredsmIoU

MAX_D, MAX_C, MAX_G, MAX_R = 1024, 256, 64, 1024   # what the N5 kernels support (include/timetuning_hip.h)
IGNORE_INDEX = 255


def _extractor(model):
    return model.feature_extractor if hasattr(model, "feature_extractor") else model


class _ProbeHead(torch.autograd.Function):
    """Module-surface head: logits at token resolution (tt_probe_logits), upsampled to R x R (tt_upsample_bilinear_tokens).
    Backward: the adjoint of the upsampling (tt_bilinear_adjoint_tokens), then the weight / bias gradients (tt_probe_wgrad)."""

    @staticmethod
    def forward(ctx, feats, weight, bias, R):
        B, n, D = feats.shape
        low = ops.probe_logits(feats.view(B * n, D), weight.detach().reshape(weight.shape[0], D), bias.detach())
        ctx.save_for_backward(feats)
        ctx.g, ctx.wshape = int(round(n ** 0.5)), weight.shape
        return ops.upsample_bilinear_tokens(low.view(B, n, -1), R)

    @staticmethod
    def backward(ctx, d_hi):
        (feats,) = ctx.saved_tensors
        B, n, D = feats.shape
        d_low = ops.bilinear_adjoint_tokens(d_hi.contiguous(), ctx.g)
        dw, db = ops.probe_wgrad(d_low.view(B * n, -1), feats.view(B * n, D))
        return None, dw.view(ctx.wshape), db, None


class _FusedProbeLoss(torch.autograd.Function):
    """``loss(x, y)``: forward runs logits -> fused upsample + CE + adjoint -> weight gradient and keeps the gradients; backward scales
    them by the incoming gradient (1 for ``loss.backward()``), as ``time_tuning._FusedLoss``."""

    @staticmethod
    def forward(ctx, feats, labels, weight, bias, out: dict):
        B, n, D = feats.shape
        C = weight.shape[0]
        low = ops.probe_logits(feats.view(B * n, D), weight.detach().reshape(C, D), bias.detach())
        loss, dlow, out["counts"] = ops.probe_upsample_ce(low.view(B, n, C), labels)
        dw, db = ops.probe_wgrad(dlow.view(B * n, C), feats.view(B * n, D))
        ctx.grads = [dw.view(weight.shape), db]
        return loss.view(())

    @staticmethod
    def backward(ctx, gout):
        out, ctx.grads = ctx.grads, None
        if out is None:
            raise RuntimeError("the fused linear-probe loss was already back-propagated")
        ops.scale_tensors_(out, gout.reshape(1).to(torch.float32).contiguous())
        return None, None, out[0], out[1], None


class LinearFinetune(nn.Module):
    """``LinearFinetune(model, num_classes, train_mask_size)`` (``linear_finetune.py:13-21``).  D is the backbone width of ``model``
    (the reference hard-codes 384) and the token grid g comes from the features (the reference hard-codes 28: dino-s16 at 448^2 or
    dino-s8 at 224^2)."""

    def __init__(self, model, num_classes, train_mask_size):
        super().__init__()
        self.model = model
        self.train_mask_size = int(train_mask_size)
        for param in self.model.parameters():   # freeze the model (:17-19)
            param.requires_grad = False
        D = _extractor(model).backbone.embed_dim
        if D % 4 or not 0 < D <= MAX_D:
            raise ValueError(f"LinearFinetune: feature width {D} is not supported (need D % 4 == 0, D <= {MAX_D})")
        if not 1 <= num_classes <= MAX_C:
            raise ValueError(f"LinearFinetune: {num_classes} classes are not supported (need 1..{MAX_C})")
        if not 1 <= self.train_mask_size <= MAX_R:
            raise ValueError(f"LinearFinetune: mask size {self.train_mask_size} is not supported (need 1..{MAX_R})")
        self.num_classes = int(num_classes)
        self.finetune_head = nn.Conv2d(D, num_classes, kernel_size=1)

    def _features(self, x, use_head: bool) -> torch.Tensor:
        fe = _extractor(self.model)
        D = self.finetune_head.in_channels
        width = fe.feature_dim if use_head else fe.backbone.embed_dim
        if width != D:
            raise ValueError(f"LinearFinetune: the features are {width} wide (use_head={use_head}), the head expects {D}")
        with torch.no_grad():
            feats, _ = self.model(x, use_head=use_head)
        feats = feats.detach().float().contiguous()
        g = int(round(feats.shape[1] ** 0.5))
        if g * g != feats.shape[1] or not 1 <= g <= MAX_G:
            raise ValueError(f"LinearFinetune: {feats.shape[1]} tokens are not a square grid of at most {MAX_G}^2")
        return feats

    def _head(self):
        w, b = self.finetune_head.weight, self.finetune_head.bias
        if not (w.is_cuda and b.is_cuda):
            raise ops._lib.HipLibraryError("LinearFinetune: the head must be in GPU memory (the HIP path has no CPU fallback)")
        return w, b

    def head_forward(self, feats: torch.Tensor) -> torch.Tensor:
        """feats [B, g*g, D] -> logits [B, C, R, R] with autograd to the head (the commuted order of :26-30)."""
        w, b = self._head()
        B = feats.shape[0]
        R = self.train_mask_size
        hi = _ProbeHead.apply(feats, w, b, R)
        return hi.view(B, R, R, -1).permute(0, 3, 1, 2)

    def forward(self, x, use_head=False):
        """``linear_finetune.py:23-31``: [B, C, R, R] logits at the mask size (a channels-last view)."""
        return self.head_forward(self._features(x, use_head))

    def head_loss(self, feats: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """The fused head step on given features: mean CrossEntropyLoss(ignore_index=255) of the mask-resolution logits against
        y [B, R, R] (or [B, 1, R, R]) integer labels, with the head gradients already computed.  Raises ValueError for labels
        outside [0, C) other than 255 (this reads the kernel's count: one device-to-host copy)."""
        w, b = self._head()
        R = self.train_mask_size
        B = feats.shape[0]
        labels = y.reshape(B, -1).long().contiguous()
        if labels.shape[1] != R * R:
            raise ValueError(f"LinearFinetune.loss: labels of {labels.shape[1]} pixels per image, the mask size is {R} x {R}")
        out: dict = {}
        loss = _FusedProbeLoss.apply(feats, labels.view(B, R, R), w, b, out)
        invalid = int(out["counts"][1])
        if invalid:
            raise ValueError(f"LinearFinetune.loss: {invalid} labels outside [0, {self.num_classes}) that are not the ignore index "
                             f"{IGNORE_INDEX}")
        return loss

    def loss(self, x, y, use_head=False) -> torch.Tensor:
        """``criterion(model(x), y)`` of :81-82 as one fused step."""
        return self.head_loss(self._features(x, use_head), y)

    @torch.no_grad()
    def predict(self, x, use_head=False) -> torch.Tensor:
        """argmax over classes of ``forward(x)``: [B, R, R] int64, from the token-resolution logits (tt_upsample_argmax_f32)."""
        feats = self._features(x, use_head)
        w, b = self._head()
        B, n, D = feats.shape
        low = ops.probe_logits(feats.view(B * n, D), w.reshape(w.shape[0], D), b)
        return ops.upsample_argmax_f32(low.view(B, n, -1), self.train_mask_size)


def prepare_labels(y: torch.Tensor, mask_size: int) -> torch.Tensor:
    """The reference's label preparation (:78-80): ``y*255``, nearest interpolation to the mask size, ``.long()``; -> [B, R, R]."""
    y = y * 255
    y = F.interpolate(y.float(), size=(mask_size, mask_size), mode="nearest")
    return y.long().squeeze(1)


@torch.no_grad()
def validate(model: LinearFinetune, val_loader, epoch) -> float:
    """``linear_finetune.py:34-51``: mIoU of the arg-max predictions over the pixels whose label is not 255, with identity
    matching (``PredsmIoU.compute(True, linear_probe=True)``)."""
    model.eval()
    miou = PredsmIoU(10, 10, involve_bg=True)
    R = model.train_mask_size
    for x, y in val_loader:
        x = x.cuda()
        y = y.cuda()
        gt = y * 255
        gt = F.interpolate(gt.float(), size=(R, R), mode="nearest").squeeze(1)
        valid = gt != IGNORE_INDEX
        out = model.predict(x)
        miou.update(gt[valid].flatten(), out[valid].flatten())
    value = miou.compute(True, linear_probe=True)[0]
    print("Epoch: {}, mIoU: {}".format(epoch, value))
    model.train()
    return value


class FusedSGD(torch.optim.Optimizer):
    """``torch.optim.SGD`` (constructor, defaults and ``momentum_buffer`` state, so state dicts interchange) with the update of every
    parameter in one launch (tt_sgd_step).  Dampening, Nesterov and ``maximize`` are not built."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, foreach=None,
                 differentiable=False, fused=None):
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError(f"FusedSGD: invalid lr {lr}, momentum {momentum} or weight_decay {weight_decay}")
        if dampening != 0 or nesterov or maximize or differentiable:
            raise NotImplementedError("FusedSGD: dampening, nesterov, maximize and differentiable are not built")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize,
                        foreach=foreach, differentiable=differentiable, fused=fused)
        super().__init__(params, defaults)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            mom, lr, wd = float(group["momentum"]), float(group["lr"]), float(group["weight_decay"])
            first, later = [], []
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise NotImplementedError("FusedSGD: sparse gradients are not built")
                state = self.state[p]
                buf = state.get("momentum_buffer")
                if mom != 0 and buf is None:
                    buf = state["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                    first.append((p, p.grad.contiguous(), buf, lr, wd))
                else:
                    later.append((p, p.grad.contiguous(), buf if mom != 0 else None, lr, wd))
            if first:
                ops.sgd_step_(first, mom, first_step=True)
            if later:
                ops.sgd_step_(later, mom, first_step=False)
        return loss


# ---- the training driver (linear_finetune.py:55-89) ---------------------------------------------------------------------------------

def build_parser() -> argparse.ArgumentParser:
    """The constants of ``linear_finetune.py:55-89`` as flags.  ``--dataset synthetic`` and the ``--num_*_images`` flags are additions,
    and so is ``--dataset voc``: ``leoloader.pascal_loader`` on ``--dataset_path`` (the VOCSegmentation root), as ``:69-71`` calls it."""
    p = argparse.ArgumentParser()
    p.add_argument("--architecture", type=str, default="dino-s16")
    p.add_argument("--model_path", type=str, default="dino-s16.pth")
    p.add_argument("--head_layers", type=int, nargs="+", default=[1024, 1024, 512, 256])
    p.add_argument("--num_prototypes", type=int, default=200)
    p.add_argument("--num_classes", type=int, default=21)
    p.add_argument("--mask_size", type=int, default=100)
    p.add_argument("--batch_size", type=int, default=60)
    p.add_argument("--epochs", type=int, default=50)
    p.add_argument("--lr", type=float, default=0.01)
    p.add_argument("--momentum", type=float, default=0.9)
    p.add_argument("--weight_decay", type=float, default=0.0001)
    p.add_argument("--step_size", type=int, default=20)
    p.add_argument("--gamma", type=float, default=0.1)
    p.add_argument("--input_resolution", type=int, default=448)
    p.add_argument("--dataset", type=str, default="pascal")
    p.add_argument("--dataset_path", type=str, default="../../dataset/leopascal/VOCSegmentation")
    add_decode_arguments(p, jpeg=False)
    p.add_argument("--save_path", type=str, default="linear_finetune.pth", help="state_dict written after every epoch ('' = none)")
    p.add_argument("--num_train_images", type=int, default=120, help="synthetic data only")
    p.add_argument("--num_val_images", type=int, default=60, help="synthetic data only")
    return p


def synthetic_segmentation(n: int, resolution: int, num_classes: int, seed: int, band: int = 2):
    """Images [n, 3, S, S] fp32 of textured class discs on a textured background, and their labels [n, 1, S, S] as the VOC reader
    delivers them (fp32 label / 255, ToTensor of the PNG), with a 255 band of ``band`` pixels at every object border as VOC has."""
    from . import synth

    S = resolution
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    tex = synth.normal("lp.tex", (num_classes, 3, 8, 8), 1.0, 0.0, seed)
    cell = max(S // 8, 1)
    tex = np.kron(tex, np.ones((1, 1, cell, cell), np.float32))
    tex = np.pad(tex, ((0, 0), (0, 0), (0, max(S - tex.shape[2], 0)), (0, max(S - tex.shape[3], 0))), mode="edge")[:, :, :S, :S]
    params = synth.normal("lp.discs", (n, 3, 4), 1.0, 0.0, seed)
    imgs, labels = [], []
    for k in range(n):
        img = tex[0].copy()
        lab = np.zeros((S, S), np.int64)
        border = np.zeros((S, S), bool)
        for o in range(3):
            a = params[k, o]
            cls = 1 + int(abs(a[0]) * 997) % max(num_classes - 1, 1) if num_classes > 1 else 0
            cy, cx = S * (0.5 + 0.3 * np.tanh(a[1])), S * (0.5 + 0.3 * np.tanh(a[2]))
            rad = S * (0.12 + 0.06 * abs(np.tanh(a[3])))
            d = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
            inside = d < rad
            img = np.where(inside[None], tex[cls] + 0.5 * cls, img)
            lab[inside] = cls
            border |= np.abs(d - rad) < band
        lab[border] = IGNORE_INDEX
        imgs.append(img + 0.05 * synth.normal(f"lp.noise.{k}", (3, S, S), 1.0, 0.0, seed))
        labels.append(lab)
    x = torch.from_numpy(np.stack(imgs).astype(np.float32))
    y = torch.from_numpy(np.stack(labels)[:, None].astype(np.uint8)).float() / 255
    return x, y


def _batches(x, y, batch_size):
    return [(x[i:i + batch_size], y[i:i + batch_size]) for i in range(0, x.shape[0], batch_size)]


def main(argv: Optional[list] = None) -> float:
    """``linear_finetune.py:55-89`` on synthetic data or (``--dataset voc``) on a Pascal VOC tree: validate, train one epoch with CrossEntropyLoss(ignore_index=255) and SGD +
    StepLR, validate; returns the last mIoU."""
    from .models import FeatureExtractor
    from .time_tuning import TimeT

    args = build_parser().parse_args(argv)
    if args.dataset not in ("synthetic", "voc"):
        raise NotImplementedError("this build reads Pascal VOC through --dataset voc (leoloader.pascal_loader on --dataset_path, the "
                                  "VOCSegmentation root) and generated data through --dataset synthetic")
    train_loader = val_loader = None
    if args.dataset == "voc":                                                            # linear_finetune.py:69-71
        from .leoloader import pascal_loader

        train_loader = pascal_loader(args.batch_size, args.dataset_path, "trainaug", args.mask_size, train_size=args.input_resolution, png=args.png_decode)
        val_loader = pascal_loader(args.batch_size, args.dataset_path, "val", args.mask_size, train_size=args.input_resolution, png=args.png_decode)
    torch.cuda.set_device(0)
    feature_extractor = FeatureExtractor(args.architecture, args.model_path, list(args.head_layers), return_attention=False)
    model = TimeT(feature_extractor, args.num_prototypes)
    model = LinearFinetune(model, args.num_classes, args.mask_size)
    model.cuda()
    model.train()
    optimizer = FusedSGD(model.parameters(), lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay)
    scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=args.step_size, gamma=args.gamma)
    if train_loader is None:
        x_tr, y_tr = synthetic_segmentation(args.num_train_images, args.input_resolution, args.num_classes, seed=1)
        x_va, y_va = synthetic_segmentation(args.num_val_images, args.input_resolution, args.num_classes, seed=2)
        train_loader = _batches(x_tr, y_tr, args.batch_size)
        val_loader = _batches(x_va, y_va, args.batch_size)
    print("train_loader", len(train_loader))
    print("val_loader", len(val_loader))
    miou = math.nan
    for epoch in range(args.epochs):
        validate(model, val_loader, epoch)
        for i, (x, y) in enumerate(train_loader):
            x = x.cuda()
            y = y.cuda()
            loss = model.loss(x, prepare_labels(y, args.mask_size))
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            print("Epoch: {}, Iter: {}, Loss: {}".format(epoch, i, loss.item()))
        scheduler.step()
        if args.save_path:
            torch.save(model.state_dict(), args.save_path)
        miou = validate(model, val_loader, epoch)
    return miou


if __name__ == "__main__":
    main()
