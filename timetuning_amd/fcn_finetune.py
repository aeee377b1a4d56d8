"""FCN-head fine-tuning: the second supervised Pascal VOC read-out of frozen dense features, next to ``linear_finetune.py``.

``FCNFinetune`` has ``LinearFinetune``'s surface (``forward``, ``loss`` / ``head_loss``, ``predict``, ``train_mask_size``), so
``linear_finetune.validate``, ``prepare_labels`` and ``FusedSGD`` work on it unchanged; the head is ``leopart.FCNHead``
(``leopart.py:83-147``) under the attribute ``decode_head``.  The head runs at token resolution and only the C logits are upsampled to
the mask size, as in the linear probe.  ``forward`` returns the mask-resolution logits with autograd to every head
parameter; ``loss(x, y)`` is the fused step: convs -> tt_probe_logits -> tt_probe_upsample_ce -> tt_probe_wgrad -> the backward chain of
``leopart.head_backward``, with the gradients held and scaled by the incoming gradient, as ``linear_finetune._FusedProbeLoss`` does.
Dropout2d is a per-(image, channel) multiplier drawn by torch from a module-owned ``torch.Generator`` (``rand(B, channels) >= p``,
divided by ``1 - p``) and applied in the last convolution's epilogue; in ``eval()`` there is none.  ``norm_cfg`` (``--norm bn``) gives every
ConvModule its BatchNorm2d (tt_bn_tokens_fwd / _bwd): batch statistics in ``train()``, running ones in ``eval()`` and in
``predict``.
"""
from __future__ import annotations

import argparse
import math
from typing import Optional

import torch
import torch.nn as nn

from . import hip_ops as ops
from . import leopart
from .linear_finetune import (IGNORE_INDEX, MAX_C, MAX_D, MAX_G, MAX_R, FusedSGD, _batches, _extractor, build_parser as _linear_parser,
                              prepare_labels, synthetic_segmentation, validate)


class _FusedHeadLoss(torch.autograd.Function):
    """``loss(x, y)``: forward runs the head, the fused upsample + CE + adjoint and the whole backward chain and keeps the gradients;
    backward scales them by the incoming gradient (1 for ``loss.backward()``)."""

    @staticmethod
    def forward(ctx, feats, labels, out_scale, grid, num_convs, concat_input, norm, out: dict, *params):
        leopart.check_norm_backward(norm, bool(num_convs or concat_input))
        acts, f, low, saved = leopart.head_forward(feats, grid, params, num_convs, concat_input, out_scale, norm)
        loss, dlow, out["counts"] = ops.probe_upsample_ce(low, labels)
        ctx.grads = [g.contiguous() for g in leopart.head_backward(feats, grid, params, num_convs, concat_input, out_scale, acts, f, dlow,
                                                                   saved)]
        return loss.view(())

    @staticmethod
    def backward(ctx, gout):
        out, ctx.grads = ctx.grads, None
        if out is None:
            raise RuntimeError("the fused FCN-head loss was already back-propagated")
        ops.scale_tensors_(out, gout.reshape(1).to(torch.float32).contiguous())
        return (None,) * 8 + tuple(out)


class FCNFinetune(nn.Module):
    """``FCNFinetune(model, num_classes, train_mask_size, channels=512, **head_args)``: a frozen backbone and an ``FCNHead`` on its
    features.  ``head_args``: ``num_convs``, ``kernel_size``, ``concat_input``, ``dropout_ratio``, ``norm_cfg`` of ``leopart.FCNHead``;
    ``seed`` seeds the dropout generator.  With a norm layer, ``train()`` normalises with batch statistics and updates the running ones;
    ``eval()`` (``predict``, ``validate``) normalises with the running ones."""

    def __init__(self, model, num_classes, train_mask_size, channels=512, seed: int = 0, **head_args):
        super().__init__()
        self.model = model
        self.train_mask_size = int(train_mask_size)
        for param in self.model.parameters():
            param.requires_grad = False
        D = _extractor(model).backbone.embed_dim
        if D % 4 or not 0 < D <= MAX_D:
            raise ValueError(f"FCNFinetune: feature width {D} is not supported (need D % 4 == 0, D <= {MAX_D})")
        if not 1 <= num_classes <= MAX_C:
            raise ValueError(f"FCNFinetune: {num_classes} classes are not supported (need 1..{MAX_C})")
        if not 1 <= self.train_mask_size <= MAX_R:
            raise ValueError(f"FCNFinetune: mask size {self.train_mask_size} is not supported (need 1..{MAX_R})")
        self.num_classes = int(num_classes)
        self.decode_head = leopart.FCNHead(D, channels, num_classes=self.num_classes, **head_args)
        self._seed, self._generator = int(seed), None

    def _features(self, x, use_head: bool) -> torch.Tensor:
        fe = _extractor(self.model)
        D = self.decode_head.in_channels
        width = fe.feature_dim if use_head else fe.backbone.embed_dim
        if width != D:
            raise ValueError(f"FCNFinetune: the features are {width} wide (use_head={use_head}), the head expects {D}")
        with torch.no_grad():
            feats, _ = self.model(x, use_head=use_head)
        return feats.detach().float().contiguous()

    def _grid(self, feats: torch.Tensor):
        g = int(round(feats.shape[1] ** 0.5))
        if g * g != feats.shape[1] or not 1 <= g <= MAX_G:
            raise ValueError(f"FCNFinetune: {feats.shape[1]} tokens are not a square grid of at most {MAX_G}^2")
        return (g, g)

    def _params(self) -> list:
        params = self.decode_head.parameter_list()
        if not all(p.is_cuda for p in params):
            raise ops._lib.HipLibraryError("FCNFinetune: the head must be in GPU memory (the HIP path has no CPU fallback)")
        return params

    def dropout_scale(self, B: int, device) -> Optional[torch.Tensor]:
        """The Dropout2d multipliers of one step, [B, channels]: 0 or 1 / (1 - p); None in ``eval()`` or with p = 0."""
        p = self.decode_head.dropout_ratio
        if not self.training or p <= 0.0:
            return None
        if self._generator is None or self._generator.device != torch.device(device):
            self._generator = torch.Generator(device=device)
            self._generator.manual_seed(self._seed)
        keep = torch.rand(B, self.decode_head.channels, generator=self._generator, device=device) >= p
        return keep.to(torch.float32) / (1.0 - p)

    def head_forward(self, feats: torch.Tensor, out_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
        """feats [B, g*g, D] -> logits [B, C, R, R] with autograd to the head.  ``out_scale``: given dropout multipliers (default:
        drawn in training mode, none in ``eval()``)."""
        params = self._params()
        B, R = feats.shape[0], self.train_mask_size
        if out_scale is None:
            out_scale = self.dropout_scale(B, feats.device)
        h = self.decode_head
        hi = leopart.HeadFunction.apply(feats, out_scale, self._grid(feats), R, h.num_convs, h.concat_input, h.head_norm(), *params)
        return hi.view(B, R, R, -1).permute(0, 3, 1, 2)

    def forward(self, x, use_head=False):
        """[B, C, R, R] logits at the mask size (a channels-last view)."""
        return self.head_forward(self._features(x, use_head))

    def head_loss(self, feats: torch.Tensor, y: torch.Tensor, out_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The fused head step on given features: mean CrossEntropyLoss(ignore_index=255) of the mask-resolution logits against
        y [B, R, R] (or [B, 1, R, R]) integer labels, with every head gradient already computed.  Raises ValueError for labels
        outside [0, C) other than 255 (this reads the kernel's count: one device-to-host copy)."""
        params = self._params()
        R = self.train_mask_size
        B = feats.shape[0]
        labels = y.reshape(B, -1).long().contiguous()
        if labels.shape[1] != R * R:
            raise ValueError(f"FCNFinetune.loss: labels of {labels.shape[1]} pixels per image, the mask size is {R} x {R}")
        if out_scale is None:
            out_scale = self.dropout_scale(B, feats.device)
        h = self.decode_head
        out: dict = {}
        loss = _FusedHeadLoss.apply(feats, labels.view(B, R, R), out_scale, self._grid(feats), h.num_convs, h.concat_input, h.head_norm(), out,
                                    *params)
        invalid = int(out["counts"][1])
        if invalid:
            raise ValueError(f"FCNFinetune.loss: {invalid} labels outside [0, {self.num_classes}) that are not the ignore index "
                             f"{IGNORE_INDEX}")
        return loss

    def loss(self, x, y, use_head=False) -> torch.Tensor:
        """``criterion(model(x), y)`` as one fused step."""
        return self.head_loss(self._features(x, use_head), y)

    @torch.no_grad()
    def predict(self, x, use_head=False) -> torch.Tensor:
        """argmax over classes of ``forward(x)`` without dropout: [B, R, R] int64, from the token-resolution logits."""
        return self.head_predict(self._features(x, use_head))

    @torch.no_grad()
    def head_predict(self, feats: torch.Tensor) -> torch.Tensor:
        h = self.decode_head
        norm = h.head_norm()
        if norm is not None:
            norm.training = False   # a prediction normalises with the running statistics, whatever the module's mode
        _, _, low, _ = leopart.head_forward(feats, self._grid(feats), self._params(), h.num_convs, h.concat_input, None, norm)
        return ops.upsample_argmax_f32(low, self.train_mask_size)


# ---- the training driver: linear_finetune.main with the FCN head --------------------------------------------------------------------

def build_parser() -> argparse.ArgumentParser:
    """``linear_finetune.build_parser()`` plus the head's arguments."""
    p = _linear_parser()
    p.add_argument("--channels", type=int, default=512)
    p.add_argument("--num_convs", type=int, default=2)
    p.add_argument("--concat_input", action=argparse.BooleanOptionalAction, default=True)
    p.add_argument("--dropout_ratio", type=float, default=0.1)
    p.add_argument("--norm", choices=("none", "bn"), default="none", help="bn: conv (no bias) -> BatchNorm2d -> ReLU in every ConvModule")
    p.set_defaults(save_path="fcn_finetune.pth")
    return p


def main(argv: Optional[list] = None) -> float:
    """``linear_finetune.main`` with ``FCNFinetune``: validate, train with the fused step and FusedSGD + StepLR, validate; returns the
    last mIoU.  ``--dataset voc`` reads a Pascal VOC tree, ``--dataset synthetic`` generated data."""
    from .models import FeatureExtractor
    from .time_tuning import TimeT

    args = build_parser().parse_args(argv)
    if args.dataset not in ("synthetic", "voc"):
        raise NotImplementedError("this build reads Pascal VOC through --dataset voc (leoloader.pascal_loader on --dataset_path, the "
                                  "VOCSegmentation root) and generated data through --dataset synthetic")
    train_loader = val_loader = None
    if args.dataset == "voc":
        from .leoloader import pascal_loader

        train_loader = pascal_loader(args.batch_size, args.dataset_path, "trainaug", args.mask_size, train_size=args.input_resolution, png=args.png_decode)
        val_loader = pascal_loader(args.batch_size, args.dataset_path, "val", args.mask_size, train_size=args.input_resolution, png=args.png_decode)
    torch.cuda.set_device(0)
    feature_extractor = FeatureExtractor(args.architecture, args.model_path, list(args.head_layers), return_attention=False)
    model = TimeT(feature_extractor, args.num_prototypes)
    model = FCNFinetune(model, args.num_classes, args.mask_size, channels=args.channels, num_convs=args.num_convs,
                        concat_input=args.concat_input, dropout_ratio=args.dropout_ratio,
                        norm_cfg=dict(type="BN", requires_grad=True) if args.norm == "bn" else None)
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
