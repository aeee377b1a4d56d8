"""fp64 CPU restatement of the FCN head (N32) on ``torch.nn.functional.conv2d``: what the token-grid convolution kernels and
``FCNFinetune`` are held to.  Token-major tensors [B, gh*gw, C] go in and out; inside, everything is NCHW fp64 under torch autograd."""
import numpy as np
import torch
import torch.nn.functional as F

from timetuning_amd import synth

U = 2.0 ** -24   # fp32 unit roundoff


def to_nchw(x, gh, gw):
    B, n, C = x.shape
    return x.double().permute(0, 2, 1).reshape(B, C, gh, gw)


def to_tokens(x):
    B, C, gh, gw = x.shape
    return x.reshape(B, C, gh * gw).permute(0, 2, 1).contiguous()


def conv(xa, xb, w, bias, act, out_scale, gh, gw):
    """y [B, gh*gw, Cout] fp64 = act(bias + conv3x3(cat([xa, xb]), w)) * out_scale[b, co], zero padding."""
    x = to_nchw(xa, gh, gw) if xb is None else torch.cat([to_nchw(xa, gh, gw), to_nchw(xb, gh, gw)], 1)
    y = F.conv2d(x, w.double(), None if bias is None else bias.double(), padding=1)
    if act:
        y = F.relu(y)
    if out_scale is not None:
        y = y * out_scale.double()[:, :, None, None]
    return to_tokens(y)


def conv_abs(xa, xb, w, bias, out_scale, gh, gw):
    """sum |w| |x| + |bias|, times |out_scale|: what the forward error bound multiplies."""
    return conv(xa.abs(), None if xb is None else xb.abs(), w.abs(), None if bias is None else bias.abs(), 0,
                None if out_scale is None else out_scale.abs(), gh, gw)


def conv_grads(dpre, xa, xb, w, gh, gw):
    """(dx [B, gh*gw, Cin], dw, db) of sum(dpre * conv(x, w)) in fp64: the transposed convolution and the two parameter gradients."""
    x = to_nchw(xa, gh, gw) if xb is None else torch.cat([to_nchw(xa, gh, gw), to_nchw(xb, gh, gw)], 1)
    x = x.clone().requires_grad_(True)
    w64 = w.double().clone().requires_grad_(True)
    b64 = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    (F.conv2d(x, w64, b64, padding=1) * to_nchw(dpre, gh, gw)).sum().backward()
    return to_tokens(x.grad), w64.grad, b64.grad


def head_keys(num_convs, concat_input):
    keys = []
    for i in range(num_convs):
        keys += [f"convs.{i}.conv.weight", f"convs.{i}.conv.bias"]
    if concat_input:
        keys += ["conv_cat.conv.weight", "conv_cat.conv.bias"]
    return keys + ["conv_seg.weight", "conv_seg.bias"]


def head_shapes(D, channels, C, num_convs, concat_input):
    shapes = {}
    for i in range(num_convs):
        shapes[f"convs.{i}.conv.weight"] = (channels, D if i == 0 else channels, 3, 3)
        shapes[f"convs.{i}.conv.bias"] = (channels,)
    if concat_input:
        shapes["conv_cat.conv.weight"] = (channels, D + channels, 3, 3)
        shapes["conv_cat.conv.bias"] = (channels,)
    shapes["conv_seg.weight"] = (C, channels, 1, 1)
    shapes["conv_seg.bias"] = (C,)
    return shapes


def head_params(tag, D, channels, C, num_convs, concat_input):
    """Deterministic fp32 parameters under the state-dict keys: weights of std 1 / sqrt(fan-in), biases of std 0.1."""
    out = {}
    for k, s in head_shapes(D, channels, C, num_convs, concat_input).items():
        std = 0.1 if len(s) == 1 else 1.0 / np.sqrt(s[1] * s[2] * s[3])
        out[k] = torch.from_numpy(synth.normal(f"{tag}.{k}", s, std))
    return out


def head_logits(feats, params, num_convs, concat_input, out_scale, g, R):
    """The reference head (leopart.py:140-147) in fp64 on [B, g*g, D] features: convs -> conv_cat(cat([x, convs(x)])) -> dropout as
    the given multipliers -> conv_seg, then the bilinear upsampling (align_corners=False) of the logits to R x R.  ``params`` maps the
    state-dict keys to tensors (fp64 leaves for autograd)."""
    x = to_nchw(feats, g, g)
    out = x
    for i in range(num_convs):
        out = F.relu(F.conv2d(out, params[f"convs.{i}.conv.weight"], params[f"convs.{i}.conv.bias"], padding=1))
    if concat_input:
        out = F.relu(F.conv2d(torch.cat([x, out], 1), params["conv_cat.conv.weight"], params["conv_cat.conv.bias"], padding=1))
    if out_scale is not None:
        out = out * out_scale.double()[:, :, None, None]
    low = F.conv2d(out, params["conv_seg.weight"], params["conv_seg.bias"])
    return F.interpolate(low, size=(R, R), mode="bilinear", align_corners=False)


def head_loss_and_grads(feats, params32, labels, num_convs, concat_input, out_scale, g, R):
    """-> (loss, {key: gradient}, logits) in fp64: mean cross-entropy with ignore_index 255 of the mask-resolution logits."""
    params = {k: v.double().clone().requires_grad_(True) for k, v in params32.items()}
    logits = head_logits(feats, params, num_convs, concat_input, out_scale, g, R)
    loss = F.cross_entropy(logits, labels, ignore_index=255)
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in params.items()}, logits.detach()


# ---- the fixture tests/golden/fcn_head.npz (tools/gen_fcn_golden.py writes it, test_fcn_head_host.py recomputes it)
FIXTURE = dict(B=2, g=4, D=16, channels=8, C=5, R=9, num_convs=2, concat_input=True, p=0.25)


def fixture_inputs():
    c = FIXTURE
    feats = torch.from_numpy(synth.normal("fcn.fix.feats", (c["B"], c["g"] * c["g"], c["D"])))
    params = head_params("fcn.fix", c["D"], c["channels"], c["C"], c["num_convs"], c["concat_input"])
    rng = np.random.default_rng(32)
    labels = rng.integers(0, c["C"], (c["B"], c["R"], c["R"]))
    labels[rng.random(labels.shape) < 0.15] = 255
    keep = rng.random((c["B"], c["channels"])) >= c["p"]
    out_scale = torch.from_numpy((keep / (1.0 - c["p"])).astype(np.float32))
    return feats, params, torch.from_numpy(labels.astype(np.int64)), out_scale


def fixture_arrays():
    """Everything the fixture file holds, as fp32 / int64 arrays."""
    c = FIXTURE
    feats, params, labels, out_scale = fixture_inputs()
    loss, grads, logits = head_loss_and_grads(feats, params, labels, c["num_convs"], c["concat_input"], out_scale, c["g"], c["R"])
    out = {"feats": feats.numpy(), "labels": labels.numpy().astype(np.uint8), "out_scale": out_scale.numpy(),
           "loss": np.float32(loss.item()), "logits": logits.numpy().astype(np.float32)}
    for k, v in params.items():
        out["param." + k] = v.numpy()
        out["grad." + k] = grads[k].numpy().astype(np.float32)
    return out
