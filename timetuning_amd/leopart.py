"""The FCN decode head of the reference (``leopart.py:83-147``, on ``BaseDecodeHead`` ``:13-80``) on the HIP kernels of N32.

``FCNHead`` holds the parameters under the names the reference's module has with mmcv's ``ConvModule`` (``convs.{i}.conv.weight/bias``,
``conv_cat.conv.weight/bias``, ``conv_seg.weight/bias``), so state dicts interchange.  The arithmetic is ``head_forward`` /
``head_backward`` below, on token-major features ``[B, gh*gw, C]``: 3x3 conv + ReLU layers (tt_conv3x3_tokens_fwd), the optional
``conv_cat`` over ``cat([x, convs(x)])`` read from its two sources without storing the concatenation, ``Dropout2d`` as a per-(image,
channel) multiplier in the last convolution's epilogue, and the 1x1 ``conv_seg`` (tt_probe_logits).  The reference's ``cls_seg`` ends
in a bare ``return`` (``:75-80``); the head returns the ``conv_seg`` output, which is what it evidently means.  ``norm_cfg`` is not
built (every conv has a bias) and neither are kernel sizes other than 3.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import hip_ops as ops

MAX_CHANNELS = 1024   # per source of a convolution (include/timetuning_hip.h, N32)


class _ConvModule(nn.Module):
    """mmcv's ``ConvModule`` without a norm layer: a 3x3 ``conv`` with bias, followed by ReLU.  Init is ConvModule's default
    (Kaiming normal, fan-out, ReLU gain; zero bias)."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size=3, padding=1)
        nn.init.kaiming_normal_(self.conv.weight, a=0, mode="fan_out", nonlinearity="relu")
        nn.init.zeros_(self.conv.bias)


def _check_channels(name: str, value: int) -> int:
    value = int(value)
    if value <= 0 or value % 4 or value > MAX_CHANNELS:
        raise ValueError(f"FCNHead: {name} = {value} is not supported (need a multiple of 4 in 4..{MAX_CHANNELS})")
    return value


class FCNHead(nn.Module):
    """``FCNHead(in_channels, channels, *, num_classes, num_convs=2, kernel_size=3, concat_input=True, dropout_ratio=0.1)``
    (``leopart.py:93-138`` with the arguments of ``:41-49``)."""

    def __init__(self, in_channels, channels, *, num_classes, num_convs=2, kernel_size=3, concat_input=True, dropout_ratio=0.1):
        super().__init__()
        assert num_convs >= 0
        if kernel_size != 3:
            raise ValueError(f"FCNHead: kernel_size {kernel_size} is not built (the token-grid convolution kernels are 3x3)")
        if not 0.0 <= float(dropout_ratio) < 1.0:
            raise ValueError(f"FCNHead: dropout_ratio {dropout_ratio} is not in [0, 1)")
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
            self.convs = nn.Sequential(*[_ConvModule(self.in_channels if i == 0 else self.channels, self.channels)
                                         for i in range(self.num_convs)])
        if self.concat_input:
            self.conv_cat = _ConvModule(self.in_channels + self.channels, self.channels)
        self.conv_seg = nn.Conv2d(self.channels, self.num_classes, kernel_size=1)
        nn.init.normal_(self.conv_seg.weight, mean=0.0, std=0.01)
        nn.init.zeros_(self.conv_seg.bias)

    def parameter_list(self) -> list:
        """[w, b] of every conv of ``convs``, then of ``conv_cat`` (if built), then of ``conv_seg``: the order ``head_backward``
        returns the gradients in."""
        mods = list(self.convs) if self.num_convs else []
        if self.concat_input:
            mods.append(self.conv_cat)
        out = []
        for m in mods:
            out += [m.conv.weight, m.conv.bias]
        return out + [self.conv_seg.weight, self.conv_seg.bias]

    def forward(self, feats: torch.Tensor, grid, out_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
        """feats [B, gh*gw, in_channels] -> the ``conv_seg`` output at token resolution [B, gh*gw, num_classes], with autograd to
        every parameter (none to the features: the backbone is frozen).  ``out_scale`` [B, channels]: the Dropout2d multipliers."""
        params = self.parameter_list()
        if not all(p.is_cuda for p in params):
            raise ops._lib.HipLibraryError("FCNHead: the head must be in GPU memory (the HIP path has no CPU fallback)")
        return HeadFunction.apply(feats, out_scale, tuple(int(v) for v in grid), None, self.num_convs, self.concat_input, *params)


def _split(params, num_convs: int, concat_input: bool):
    params = [p.detach() for p in params]
    convs = [(params[2 * i], params[2 * i + 1]) for i in range(num_convs)]
    cat = (params[2 * num_convs], params[2 * num_convs + 1]) if concat_input else None
    return convs, cat, (params[-2], params[-1])


def _scale_channels(feats: torch.Tensor, out_scale: torch.Tensor) -> torch.Tensor:
    """feats[b, :, c] * out_scale[b, c]: Dropout2d on the features themselves (num_convs = 0 without conv_cat, where no convolution's
    epilogue can carry it).  One launch per image."""
    out = feats.clone()
    zero = torch.zeros_like(out_scale[0])
    for b in range(out.shape[0]):
        ops.affine_cols_(out[b], out_scale[b].contiguous(), zero)
    return out


def head_forward(feats, grid, params, num_convs: int, concat_input: bool, out_scale=None):
    """-> (acts, f, low): the outputs of ``convs``, the input of ``conv_seg`` (after dropout) and the token-resolution logits."""
    convs, cat, (ws, bs) = _split(params, num_convs, concat_input)
    B, n, _ = feats.shape
    acts, x = [], feats
    for i, (w, b) in enumerate(convs):
        last = cat is None and i == num_convs - 1
        x = ops.conv3x3_tokens(x, w, b, grid=grid, act=1, out_scale=out_scale if last else None)
        acts.append(x)
    if cat is not None:
        f = ops.conv3x3_tokens(feats, cat[0], cat[1], xb=x, grid=grid, act=1, out_scale=out_scale)
    elif convs or out_scale is None:
        f = x
    else:
        f = _scale_channels(feats, out_scale)
    C, ch = ws.shape[0], ws.shape[1]
    low = ops.probe_logits(f.view(B * n, ch), ws.reshape(C, ch), bs).view(B, n, C)
    return acts, f, low


def head_backward(feats, grid, params, num_convs: int, concat_input: bool, out_scale, acts, f, dlow) -> list:
    """The gradients of every parameter, in ``parameter_list`` order, from dlow [B, gh*gw, C], the gradient of the token-resolution
    logits.  The gradient entering the last convolution is ``dlow W_seg * out_scale * [f > 0]`` (tt_fcn_head_grad); each data gradient
    is gated by the producing layer's saved output in its own epilogue; the features get none."""
    convs, cat, (ws, bs) = _split(params, num_convs, concat_input)
    B, n, D = feats.shape
    C, ch = ws.shape[0], ws.shape[1]
    dws, dbs = ops.probe_wgrad(dlow.view(B * n, C), f.view(B * n, ch))
    grads = [None] * (2 * num_convs + (2 if concat_input else 0)) + [dws.view(ws.shape), dbs]
    if cat is None and not convs:
        return grads
    dpre = ops.fcn_head_grad(dlow, ws.reshape(C, ch), grid, out_scale, f)
    if cat is not None:
        xb = acts[-1] if acts else feats
        grads[2 * num_convs:2 * num_convs + 2] = ops.conv3x3_tokens_bwd_weight(dpre, feats, xb, grid)
        if convs:
            dpre = ops.conv3x3_tokens_bwd_data(dpre, cat[0], grid, c_begin=D, c_count=ch, gate=acts[-1])
    for i in reversed(range(num_convs)):
        grads[2 * i:2 * i + 2] = ops.conv3x3_tokens_bwd_weight(dpre, acts[i - 1] if i else feats, None, grid)
        if i:
            dpre = ops.conv3x3_tokens_bwd_data(dpre, convs[i][0], grid, gate=acts[i - 1])
    return grads


class HeadFunction(torch.autograd.Function):
    """The head with autograd to its parameters: the token-resolution logits (``R`` None) or their bilinear upsampling to R x R
    (tt_upsample_bilinear_tokens; backward: tt_bilinear_adjoint_tokens, then ``head_backward``)."""

    @staticmethod
    def forward(ctx, feats, out_scale, grid, R, num_convs, concat_input, *params):
        acts, f, low = head_forward(feats, grid, params, num_convs, concat_input, out_scale)
        ctx.save_for_backward(feats, out_scale, f, *acts, *[p.detach() for p in params])
        ctx.cfg = (grid, R, num_convs, concat_input, len(acts))
        return low if R is None else ops.upsample_bilinear_tokens(low, R)

    @staticmethod
    def backward(ctx, d):
        grid, R, num_convs, concat_input, n_acts = ctx.cfg
        feats, out_scale, f, *rest = ctx.saved_tensors
        acts, params = rest[:n_acts], rest[n_acts:]
        dlow = d.contiguous() if R is None else ops.bilinear_adjoint_tokens(d.contiguous(), grid[0])
        grads = head_backward(feats, grid, params, num_convs, concat_input, out_scale, acts, f, dlow)
        return (None,) * 6 + tuple(grads)
