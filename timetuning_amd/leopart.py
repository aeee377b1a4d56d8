"""The FCN decode head of the reference (``leopart.py:83-147``, on ``BaseDecodeHead`` ``:13-80``) on the HIP kernels of N32 and N33.

``FCNHead`` holds the parameters under the names the reference's module has with mmcv's ``ConvModule`` (``convs.{i}.conv.weight/bias``,
``conv_cat.conv.weight/bias``, ``conv_seg.weight/bias``), so state dicts interchange.  The arithmetic is ``head_forward`` /
``head_backward`` below, on token-major features ``[B, gh*gw, C]``: 3x3 conv + ReLU layers (tt_conv3x3_tokens_fwd), the optional
``conv_cat`` over ``cat([x, convs(x)])`` read from its two sources without storing the concatenation, ``Dropout2d`` as a per-(image,
channel) multiplier in the last convolution's epilogue, and the 1x1 ``conv_seg`` (tt_probe_logits).  The reference's ``cls_seg`` ends
in a bare ``return`` (``:75-80``); the head returns the ``conv_seg`` output, which is what it evidently means.  ``norm_cfg``
(``:21,48,56,114,124,137``) of type ``BN`` / ``SyncBN`` makes every ConvModule ``conv (no bias) -> BatchNorm2d -> ReLU`` with the keys
``convs.{i}.bn.*`` / ``conv_cat.bn.*`` (tt_bn_tokens_fwd / _bwd, N33; statistics of this process only); other norm types and kernel
sizes other than 3 are not built.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import hip_ops as ops

MAX_CHANNELS = 1024   # per source of a convolution (include/timetuning_hip.h, N32)


def _parse_norm_cfg(norm_cfg) -> Optional[dict]:
    """None, or {eps, momentum, requires_grad} of a ``dict(type='BN' | 'SyncBN', requires_grad=True, eps=1e-5, momentum=0.1)``."""
    if norm_cfg is None:
        return None
    if not isinstance(norm_cfg, dict) or "type" not in norm_cfg:
        raise ValueError(f"FCNHead: norm_cfg must be None or a dict with a 'type' (got {norm_cfg!r})")
    cfg = dict(norm_cfg)
    kind = cfg.pop("type")
    if kind not in ("BN", "SyncBN"):
        raise ValueError(f"FCNHead: norm_cfg type {kind!r} is not built (batch normalisation only: 'BN' or 'SyncBN')")
    out = dict(requires_grad=bool(cfg.pop("requires_grad", True)), eps=cfg.pop("eps", 1e-5), momentum=cfg.pop("momentum", 0.1))
    if cfg:
        raise ValueError(f"FCNHead: norm_cfg arguments {sorted(cfg)} are not built")
    if out["momentum"] is None:
        raise ValueError("FCNHead: norm_cfg momentum=None (a cumulative average) is not built")
    out["eps"], out["momentum"] = float(out["eps"]), float(out["momentum"])
    if not out["eps"] > 0.0 or not 0.0 <= out["momentum"] <= 1.0:
        raise ValueError(f"FCNHead: norm_cfg needs eps > 0 and 0 <= momentum <= 1 (got {out['eps']}, {out['momentum']})")
    if kind == "SyncBN" and torch.distributed.is_available() and torch.distributed.is_initialized() \
            and torch.distributed.get_world_size() > 1:
        raise ValueError("FCNHead: 'SyncBN' over more than one rank is not built (the statistics are those of this process)")
    return out


class _ConvModule(nn.Module):
    """mmcv's ``ConvModule``.  Without a norm layer: a 3x3 ``conv`` with bias, followed by ReLU.  With one (``norm`` from
    ``_parse_norm_cfg``): ``conv`` without bias (``bias='auto'``), a child ``bn`` (an ``nn.BatchNorm2d`` that holds the parameters and
    buffers; the arithmetic is tt_bn_tokens_fwd / _bwd), ReLU.  Init is ConvModule's default (Kaiming normal, fan-out, ReLU gain; zero
    bias; bn.weight 1, bn.bias 0)."""

    def __init__(self, in_channels: int, out_channels: int, norm: Optional[dict] = None):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size=3, padding=1, bias=norm is None)
        nn.init.kaiming_normal_(self.conv.weight, a=0, mode="fan_out", nonlinearity="relu")
        if norm is None:
            nn.init.zeros_(self.conv.bias)
        else:
            self.bn = nn.BatchNorm2d(out_channels, eps=norm["eps"], momentum=norm["momentum"])
            nn.init.ones_(self.bn.weight)
            nn.init.zeros_(self.bn.bias)
            for p in self.bn.parameters():
                p.requires_grad = norm["requires_grad"]


def _check_channels(name: str, value: int) -> int:
    value = int(value)
    if value <= 0 or value % 4 or value > MAX_CHANNELS:
        raise ValueError(f"FCNHead: {name} = {value} is not supported (need a multiple of 4 in 4..{MAX_CHANNELS})")
    return value


class HeadNorm:
    """What ``head_forward`` / ``head_backward`` need beside the parameters when the ConvModules have a norm layer: their ``bn`` children
    (for eps, momentum and the running buffers, which a training forward updates in place), in ``parameter_list`` order, and whether
    batch statistics are used."""

    def __init__(self, bns, training: bool):
        self.bns, self.training = list(bns), bool(training)


class FCNHead(nn.Module):
    """``FCNHead(in_channels, channels, *, num_classes, num_convs=2, kernel_size=3, concat_input=True, dropout_ratio=0.1,
    norm_cfg=None)`` (``leopart.py:93-138`` with the arguments of ``:41-49``)."""

    def __init__(self, in_channels, channels, *, num_classes, num_convs=2, kernel_size=3, concat_input=True, dropout_ratio=0.1,
                 norm_cfg=None):
        super().__init__()
        assert num_convs >= 0
        if kernel_size != 3:
            raise ValueError(f"FCNHead: kernel_size {kernel_size} is not built (the token-grid convolution kernels are 3x3)")
        if not 0.0 <= float(dropout_ratio) < 1.0:
            raise ValueError(f"FCNHead: dropout_ratio {dropout_ratio} is not in [0, 1)")
        norm = _parse_norm_cfg(norm_cfg)
        self.norm_cfg = None if norm_cfg is None else dict(norm_cfg)
        self.in_channels = _check_channels("in_channels", in_channels)
        self.channels = _check_channels("channels", channels)
        self.num_classes = int(num_classes)
        self.num_convs = int(num_convs)
        self.kernel_size = 3
        self.concat_input = bool(concat_input)
        self.dropout_ratio = float(dropout_ratio)
        if self.num_convs == 0:
            assert self.in_channels == self.channels   # :103-104
            self.convs = nn.Identity()
        else:
            self.convs = nn.Sequential(*[_ConvModule(self.in_channels if i == 0 else self.channels, self.channels, norm)
                                         for i in range(self.num_convs)])
        if self.concat_input:
            self.conv_cat = _ConvModule(self.in_channels + self.channels, self.channels, norm)
        self.conv_seg = nn.Conv2d(self.channels, self.num_classes, kernel_size=1)
        nn.init.normal_(self.conv_seg.weight, mean=0.0, std=0.01)
        nn.init.zeros_(self.conv_seg.bias)

    def _conv_modules(self) -> list:
        mods = list(self.convs) if self.num_convs else []
        if self.concat_input:
            mods.append(self.conv_cat)
        return mods

    def parameter_list(self) -> list:
        """[w, b] (with a norm layer: [w, bn.weight, bn.bias]) of every ConvModule of ``convs``, then of ``conv_cat`` (if built), then
        [w, b] of ``conv_seg``: the order ``head_backward`` returns the gradients in."""
        out = []
        for m in self._conv_modules():
            out += [m.conv.weight, m.conv.bias] if self.norm_cfg is None else [m.conv.weight, m.bn.weight, m.bn.bias]
        return out + [self.conv_seg.weight, self.conv_seg.bias]

    def head_norm(self) -> Optional[HeadNorm]:
        """The ``norm`` argument of ``head_forward``: None without a norm layer; the module's ``training`` flag decides the statistics."""
        if self.norm_cfg is None:
            return None
        return HeadNorm([m.bn for m in self._conv_modules()], self.training)

    def forward(self, feats: torch.Tensor, grid, out_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
        """feats [B, gh*gw, in_channels] -> the ``conv_seg`` output at token resolution [B, gh*gw, num_classes], with autograd to
        every parameter (none to the features: the backbone is frozen).  ``out_scale`` [B, channels]: the Dropout2d multipliers."""
        params = self.parameter_list()
        if not all(p.is_cuda for p in params):
            raise ops._lib.HipLibraryError("FCNHead: the head must be in GPU memory (the HIP path has no CPU fallback)")
        return HeadFunction.apply(feats, out_scale, tuple(int(v) for v in grid), None, self.num_convs, self.concat_input, self.head_norm(),
                                  *params)


def _split(params, num_convs: int, concat_input: bool, per: int = 2):
    params = [p.detach() for p in params]
    convs = [tuple(params[per * i:per * i + per]) for i in range(num_convs)]
    cat = tuple(params[per * num_convs:per * num_convs + per]) if concat_input else None
    return convs, cat, (params[-2], params[-1])


def _scale_channels(feats: torch.Tensor, out_scale: torch.Tensor) -> torch.Tensor:
    """feats[b, :, c] * out_scale[b, c]: Dropout2d on the features themselves (num_convs = 0 without conv_cat, where no convolution's
    epilogue can carry it).  One launch per image."""
    out = feats.clone()
    zero = torch.zeros_like(out_scale[0])
    for b in range(out.shape[0]):
        ops.affine_cols_(out[b], out_scale[b].contiguous(), zero)
    return out


def _conv_module(xa, xb, p, grid, out_scale, bn, training: bool, saved: list):
    """One ConvModule: conv + bias + ReLU (+ dropout multipliers) in the convolution's epilogue, or with a norm layer the bare
    convolution and tt_bn_tokens_fwd with ReLU (+ multipliers); a training forward appends (z, save_mean, save_rstd) to ``saved``."""
    if bn is None:
        return ops.conv3x3_tokens(xa, p[0], p[1], xb=xb, grid=grid, act=1, out_scale=out_scale)
    z = ops.conv3x3_tokens(xa, p[0], None, xb=xb, grid=grid, act=0)
    y, mean, rstd = ops.bn_tokens(z, p[1], p[2], bn.running_mean, bn.running_var, training=training, momentum=bn.momentum, eps=bn.eps,
                                  act=1, out_scale=out_scale)
    if training:
        bn.num_batches_tracked.add_(1)
        saved.append((z, mean, rstd))
    return y


def head_forward(feats, grid, params, num_convs: int, concat_input: bool, out_scale=None, norm: Optional[HeadNorm] = None):
    """-> (acts, f, low, saved): the outputs of ``convs``, the input of ``conv_seg`` (after dropout), the token-resolution logits and,
    from a training forward with a norm layer, (z, save_mean, save_rstd) of every ConvModule in order (else an empty list)."""
    convs, cat, (ws, bs) = _split(params, num_convs, concat_input, 2 if norm is None else 3)
    B, n, _ = feats.shape
    bns = [None] * (num_convs + 1) if norm is None else norm.bns
    training = norm is not None and norm.training
    acts, saved, x = [], [], feats
    for i, p in enumerate(convs):
        last = cat is None and i == num_convs - 1
        x = _conv_module(x, None, p, grid, out_scale if last else None, bns[i], training, saved)
        acts.append(x)
    if cat is not None:
        f = _conv_module(feats, x, cat, grid, out_scale, bns[num_convs], training, saved)
    elif convs or out_scale is None:
        f = x
    else:
        f = _scale_channels(feats, out_scale)
    C, ch = ws.shape[0], ws.shape[1]
    low = ops.probe_logits(f.view(B * n, ch), ws.reshape(C, ch), bs).view(B, n, C)
    return acts, f, low, saved


def head_backward(feats, grid, params, num_convs: int, concat_input: bool, out_scale, acts, f, dlow, saved=()) -> list:
    """The gradients of every parameter, in ``parameter_list`` order, from dlow [B, gh*gw, C], the gradient of the token-resolution
    logits.  The gradient entering the last ConvModule is ``dlow W_seg * out_scale * [f > 0]`` (tt_fcn_head_grad); each data gradient
    is gated by the producing layer's saved output in its own epilogue; the features get none.  With a norm layer (``saved`` from a
    training ``head_forward``) that gradient is the one of the BN output: tt_bn_tokens_bwd turns it into bn.weight's, bn.bias' and the
    convolution output's, which the weight- and data-gradient launches take."""
    per = 3 if saved else 2
    convs, cat, (ws, bs) = _split(params, num_convs, concat_input, per)
    B, n, D = feats.shape
    C, ch = ws.shape[0], ws.shape[1]
    dws, dbs = ops.probe_wgrad(dlow.view(B * n, C), f.view(B * n, ch))
    grads = [None] * (per * (num_convs + (1 if concat_input else 0))) + [dws.view(ws.shape), dbs]
    if cat is None and not convs:
        return grads

    def module_grads(k, dpre, p, xa, xb):
        """-> dpre of ConvModule k's convolution; fills its slots of ``grads``."""
        if not saved:
            grads[per * k:per * k + per] = ops.conv3x3_tokens_bwd_weight(dpre, xa, xb, grid)
            return dpre
        z, mean, rstd = saved[k]
        dz, dgamma, dbeta = ops.bn_tokens_bwd(dpre, z, mean, rstd, p[1])
        grads[per * k:per * k + per] = [ops.conv3x3_tokens_bwd_weight(dz, xa, xb, grid, need_bias=False)[0], dgamma, dbeta]
        return dz

    dpre = ops.fcn_head_grad(dlow, ws.reshape(C, ch), grid, out_scale, f)
    if cat is not None:
        dpre = module_grads(num_convs, dpre, cat, feats, acts[-1] if acts else feats)
        if convs:
            dpre = ops.conv3x3_tokens_bwd_data(dpre, cat[0], grid, c_begin=D, c_count=ch, gate=acts[-1])
    for i in reversed(range(num_convs)):
        dpre = module_grads(i, dpre, convs[i], acts[i - 1] if i else feats, None)
        if i:
            dpre = ops.conv3x3_tokens_bwd_data(dpre, convs[i][0], grid, gate=acts[i - 1])
    return grads


def check_norm_backward(norm: Optional[HeadNorm], has_modules: bool) -> None:
    """The backward of a norm layer is the one of batch statistics; on running statistics (``eval()``) it is not built."""
    if norm is not None and not norm.training and has_modules:
        raise NotImplementedError("FCNHead: the backward of a head with a norm layer in eval() mode is not built")


class HeadFunction(torch.autograd.Function):
    """The head with autograd to its parameters: the token-resolution logits (``R`` None) or their bilinear upsampling to R x R
    (tt_upsample_bilinear_tokens; backward: tt_bilinear_adjoint_tokens, then ``head_backward``)."""

    @staticmethod
    def forward(ctx, feats, out_scale, grid, R, num_convs, concat_input, norm, *params):
        acts, f, low, saved = head_forward(feats, grid, params, num_convs, concat_input, out_scale, norm)
        ctx.save_for_backward(feats, out_scale, f, *acts, *[t for s in saved for t in s], *[p.detach() for p in params])
        ctx.cfg = (grid, R, num_convs, concat_input, len(acts), len(saved), norm)
        return low if R is None else ops.upsample_bilinear_tokens(low, R)

    @staticmethod
    def backward(ctx, d):
        grid, R, num_convs, concat_input, n_acts, n_saved, norm = ctx.cfg
        check_norm_backward(norm, bool(num_convs or concat_input))
        feats, out_scale, f, *rest = ctx.saved_tensors
        acts, flat, params = rest[:n_acts], rest[n_acts:n_acts + 3 * n_saved], rest[n_acts + 3 * n_saved:]
        saved = [tuple(flat[3 * k:3 * k + 3]) for k in range(n_saved)]
        dlow = d.contiguous() if R is None else ops.bilinear_adjoint_tokens(d.contiguous(), grid[0])
        grads = head_backward(feats, grid, params, num_convs, concat_input, out_scale, acts, f, dlow, saved)
        return (None,) * 7 + tuple(grads)
