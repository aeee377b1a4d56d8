"""fp64 CPU restatement of the FCN head with a norm layer (N33): every ConvModule is ``conv (no bias) -> batch_norm -> ReLU``, on
``F.conv2d`` / ``F.batch_norm`` / ``F.relu`` / ``F.interpolate`` / ``F.cross_entropy`` under torch autograd, next to the N32 restatement
tests/_fcn_ref.py; a twin module of ``nn.Conv2d`` / ``nn.BatchNorm2d`` under ``FCNHead``'s state-dict names; and the element-wise
bounds the batch-normalisation kernels are held to."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import _fcn_ref as R
from timetuning_amd import synth

U = R.U
BN = dict(type="BN", requires_grad=True)
EPS, MOMENTUM = 1e-5, 0.1


def module_names(num_convs, concat_input):
    return [f"convs.{i}" for i in range(num_convs)] + (["conv_cat"] if concat_input else [])


def head_keys(num_convs, concat_input):
    """``FCNHead(norm_cfg=BN).state_dict()`` in order."""
    keys = []
    for m in module_names(num_convs, concat_input):
        keys += [f"{m}.conv.weight"] + [f"{m}.bn.{k}" for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    return keys + ["conv_seg.weight", "conv_seg.bias"]


def param_keys(num_convs, concat_input):
    """``FCNHead(norm_cfg=BN).parameter_list()`` in order."""
    keys = []
    for m in module_names(num_convs, concat_input):
        keys += [f"{m}.conv.weight", f"{m}.bn.weight", f"{m}.bn.bias"]
    return keys + ["conv_seg.weight", "conv_seg.bias"]


def head_shapes(D, channels, C, num_convs, concat_input):
    shapes = {}
    for i, m in enumerate(module_names(num_convs, concat_input)):
        cin = D + channels if m == "conv_cat" else (D if i == 0 else channels)
        shapes[f"{m}.conv.weight"] = (channels, cin, 3, 3)
        for k in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{m}.bn.{k}"] = (channels,)
        shapes[f"{m}.bn.num_batches_tracked"] = ()
    shapes["conv_seg.weight"] = (C, channels, 1, 1)
    shapes["conv_seg.bias"] = (C,)
    return shapes


def head_state(tag, D, channels, C, num_convs, concat_input):
    """A deterministic fp32 state dict: conv weights of std 1 / sqrt(fan-in), bn.weight around 1 with negative entries, bn.bias of std
    0.3, running_mean of std 0.5, running_var in [0.5, 1.5], num_batches_tracked 3."""
    out = {}
    for k, s in head_shapes(D, channels, C, num_convs, concat_input).items():
        name = f"{tag}.{k}"
        if k.endswith("num_batches_tracked"):
            out[k] = torch.tensor(3, dtype=torch.int64)
        elif k.endswith("bn.weight"):
            w = 1.0 + torch.from_numpy(synth.normal(name, s, 0.3))
            w[1::3] *= -1.0
            out[k] = w
        elif k.endswith("bn.bias"):
            out[k] = torch.from_numpy(synth.normal(name, s, 0.3))
        elif k.endswith("running_mean"):
            out[k] = torch.from_numpy(synth.normal(name, s, 0.5))
        elif k.endswith("running_var"):
            out[k] = 1.0 + 0.5 * torch.tanh(torch.from_numpy(synth.normal(name, s)))
        elif len(s) == 1:
            out[k] = torch.from_numpy(synth.normal(name, s, 0.1))
        else:
            out[k] = torch.from_numpy(synth.normal(name, s, 1.0 / np.sqrt(s[1] * s[2] * s[3])))
    return out


def head_logits(feats, state, num_convs, concat_input, out_scale, g, R_, training=True, momentum=MOMENTUM, eps=EPS):
    """The head with norm layers in fp64 on [B, g*g, D] features -> logits [B, C, R, R].  ``state`` maps the state-dict keys to fp64
    tensors (leaves for autograd); in training the running buffers in it are updated in place, as ``F.batch_norm`` does."""
    x = R.to_nchw(feats, g, g)

    def module(name, inp):
        z = F.conv2d(inp, state[f"{name}.conv.weight"], None, padding=1)
        y = F.batch_norm(z, state[f"{name}.bn.running_mean"], state[f"{name}.bn.running_var"], state[f"{name}.bn.weight"],
                         state[f"{name}.bn.bias"], training=training, momentum=momentum, eps=eps)
        return F.relu(y)

    out = x
    for i in range(num_convs):
        out = module(f"convs.{i}", out)
    if concat_input:
        out = module("conv_cat", torch.cat([x, out], 1))
    if out_scale is not None:
        out = out * out_scale.double()[:, :, None, None]
    low = F.conv2d(out, state["conv_seg.weight"], state["conv_seg.bias"])
    return F.interpolate(low, size=(R_, R_), mode="bilinear", align_corners=False)


def as_leaves(state32):
    """fp64 copies: the parameters as autograd leaves, the buffers plain."""
    out = {}
    for k, v in state32.items():
        if "running" in k or "num_batches" in k:
            out[k] = v.double().clone() if "running" in k else v.clone()
        else:
            out[k] = v.double().clone().requires_grad_(True)
    return out


def head_loss_and_grads(feats, state32, labels, num_convs, concat_input, out_scale, g, R_):
    """-> (loss, {parameter key: gradient}, logits, {buffer key: value after the forward}) of one training forward, in fp64."""
    state = as_leaves(state32)
    logits = head_logits(feats, state, num_convs, concat_input, out_scale, g, R_, training=True)
    loss = F.cross_entropy(logits, labels, ignore_index=255)
    loss.backward()
    grads = {k: v.grad for k, v in state.items() if v.requires_grad}
    return loss.detach(), grads, logits.detach(), {k: v for k, v in state.items() if "running" in k}


class TwinConvModule(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 3, padding=1, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=EPS, momentum=MOMENTUM)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


class TwinHead(nn.Module):
    """The head as plain torch modules under ``FCNHead(norm_cfg=BN)``'s names; NCHW in, token-resolution logits out.  Dropout is the
    given multipliers."""

    def __init__(self, D, channels, C, num_convs, concat_input):
        super().__init__()
        self.num_convs, self.concat_input = num_convs, concat_input
        self.convs = nn.Sequential(*[TwinConvModule(D if i == 0 else channels, channels) for i in range(num_convs)]) if num_convs else nn.Identity()
        if concat_input:
            self.conv_cat = TwinConvModule(D + channels, channels)
        self.conv_seg = nn.Conv2d(channels, C, 1)

    def forward(self, x, out_scale=None, R_=None):
        out = self.convs(x)
        if self.concat_input:
            out = self.conv_cat(torch.cat([x, out], 1))
        if out_scale is not None:
            out = out * out_scale.to(out.dtype)[:, :, None, None]
        low = self.conv_seg(out)
        return low if R_ is None else F.interpolate(low, size=(R_, R_), mode="bilinear", align_corners=False)


# ---- the batch-normalisation kernels: fp64 values and the bounds of the issue -------------------------------------------------------

def bn_case(B, gh, gw, C, tag="acc"):
    """z [B, n, C] with column 0 at a mean 100 times its standard deviation, gamma with negative entries, beta, out_scale [B, C] (a whole
    row of zeros when B > 1), g [B, n, C], running statistics."""
    n = gh * gw
    t = lambda name, shape, std=1.0: torch.from_numpy(synth.normal(f"bn.{tag}.{name}.{B}.{n}.{C}", shape, std))
    z = t("z", (B, n, C)) * (0.5 + t("zs", (C,)).abs()) + t("zm", (C,))
    z[:, :, 0] = 100.0 * 0.25 + 0.25 * t("z0", (B, n))
    gamma = 1.0 + t("gamma", (C,), 0.3)
    gamma[1::3] *= -1.0
    beta = t("beta", (C,), 0.3)
    scale = t("s", (B, C)).abs() + 0.25
    scale[-1, ::3] = 0.0
    if B > 1:
        scale[0] = 0.0
    g = t("g", (B, n, C))
    rm, rv = t("rm", (C,), 0.5), 0.5 + t("rv", (C,)).abs()
    return z, gamma, beta, scale, g, rm, rv


def bn_forward64(z, gamma, beta, scale, act, eps, mean=None, var=None):
    """-> (y, mean, var (biased), rstd, q) in fp64; given ``mean`` / ``var`` (eval mode) they replace the batch values."""
    z2 = z.double().reshape(-1, z.shape[-1])
    if mean is None:
        mean, var = z2.mean(0), z2.var(0, unbiased=False)
    mean, var = mean.double(), var.double()
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (z2 - mean) * rstd * gamma.double() + beta.double()
    if act:
        y = F.relu(y)
    y = y.reshape(z.shape)
    if scale is not None:
        y = y * scale.double()[:, None, :]
    q = ((z2.abs() + mean.abs()) * rstd).reshape(z.shape)
    return y, mean, var, rstd, q


def bn_backward64(g, z, gamma, mean, rstd):
    """-> (dz, dgamma, dbeta) in fp64 from the gradient of the BN output."""
    g2, z2 = g.double().reshape(-1, g.shape[-1]), z.double().reshape(-1, z.shape[-1])
    rows = g2.shape[0]
    xhat = (z2 - mean) * rstd
    dbeta, dgamma = g2.sum(0), (g2 * xhat).sum(0)
    dz = gamma.double() * rstd * (g2 - dbeta / rows - xhat * dgamma / rows)
    return dz.reshape(z.shape), dgamma, dbeta


# ---- the fixture tests/golden/fcn_head_bn.npz (tools/gen_fcn_bn_golden.py writes it, test_fcn_bn_host.py recomputes it): the N32
# fixture's features, labels and dropout multipliers on a head with norm layers
FIXTURE = R.FIXTURE


def fixture_inputs():
    c = FIXTURE
    feats, _, labels, out_scale = R.fixture_inputs()
    return feats, head_state("fcn.bn.fix", c["D"], c["channels"], c["C"], c["num_convs"], c["concat_input"]), labels, out_scale


def fixture_arrays():
    c = FIXTURE
    feats, state, labels, out_scale = fixture_inputs()
    loss, grads, logits, buffers = head_loss_and_grads(feats, state, labels, c["num_convs"], c["concat_input"], out_scale, c["g"], c["R"])
    out = {"feats": feats.numpy(), "labels": labels.numpy().astype(np.uint8), "out_scale": out_scale.numpy(),
           "loss": np.float32(loss.item()), "logits": logits.numpy().astype(np.float32)}
    for k, v in state.items():
        out["state." + k] = v.numpy()
    for k, v in grads.items():
        out["grad." + k] = v.numpy().astype(np.float32)
    for k, v in buffers.items():
        out["after." + k] = v.numpy().astype(np.float32)
    return out
