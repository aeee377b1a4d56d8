"""FCN-head fine-tuning on the GPU (N32): the token-grid 3x3 convolution kernels against the fp64 restatement tests/_fcn_ref.py with
derived element-wise bounds, exact impulse responses (the row / image wrap-around of a token-major gather), repeatability, refusals, the
launch path, and ``FCNFinetune`` against the fixture tests/golden/fcn_head.npz.

The f32 MFMA is a k-ordered fmaf chain, so a reduction of K products followed by two more roundings (bias, scale) is within
(K + 2) 2^-24 sum |a| |b| of the exact value, element by element."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _fcn_ref as R
from conftest import rel_err
from timetuning_amd import _lib, fcn_finetune as FF, hip_ops as ops, leopart, linear_finetune as L, synth

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
U = R.U

GRIDS = [(1, 1, 1), (1, 7, 9), (1, 5, 13), (2, 5, 13), (3, 14, 14)]          # rows 1, 63, 65, 130, 588
COUTS = [4, 60, 68, 132]
SOURCES = [(4, 0), (36, 0), (12, 20), (384, 0)]


def _t(name, shape, std=1.0):
    return torch.from_numpy(synth.normal(name, shape, std))


def _g(t):
    return None if t is None else t.to(dev)


def _ratio(got, want, bound):
    """max over the elements of |got - want| / bound (0 / 0 = 0); a non-zero error over a zero bound is infinite."""
    err = (got.detach().cpu().double() - want).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def _case(B, gh, gw, Ca, Cb, Cout, tag="acc"):
    n = gh * gw
    xa = _t(f"fcn.{tag}.xa.{B}.{n}.{Ca}", (B, n, Ca))
    xb = _t(f"fcn.{tag}.xb.{B}.{n}.{Cb}", (B, n, Cb)) if Cb else None
    w = _t(f"fcn.{tag}.w.{Cout}.{Ca + Cb}", (Cout, Ca + Cb, 3, 3), 1.0 / np.sqrt(9 * (Ca + Cb)))
    bias = _t(f"fcn.{tag}.b.{Cout}", (Cout,), 0.5)
    scale = (_t(f"fcn.{tag}.s.{B}.{Cout}", (B, Cout)).abs() + 0.25)
    scale[0] = 0.0                                                              # a whole scale row of zeros
    scale[-1, ::3] = 0.0
    dpre = _t(f"fcn.{tag}.dpre.{B}.{n}.{Cout}", (B, n, Cout))
    return xa, xb, w, bias, scale, dpre


# ---- impulse responses, exact -------------------------------------------------------------------------------------------------------

def _positions(gh, gw):
    """(image, row, column): every corner, the last token of a row, the last token of image 0, the first token of image 1."""
    pos = {(0, 0, 0), (0, 0, gw - 1), (0, gh - 1, 0), (0, gh - 1, gw - 1), (0, gh // 2, gw - 1), (1, 0, 0), (1, gh - 1, gw - 1)}
    return sorted(pos)


def _scatter(B, gh, gw, b, i, j, taps, sign):
    """taps [n, 3, 3] written around (b, i, j): tap (di, dj) lands on (i - sign di, j - sign dj) if that is on the grid."""
    out = torch.zeros(B, gh * gw, taps.shape[0])
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            ii, jj = i - sign * di, j - sign * dj
            if 0 <= ii < gh and 0 <= jj < gw:
                out[b, ii * gw + jj] = taps[:, 1 + di, 1 + dj]
    return out


@pytest.mark.parametrize("gh,gw", [(1, 1), (1, 5), (5, 1), (2, 2), (3, 5)])
def test_impulse_response_is_the_taps_exactly(gh, gw):
    B, Cin, Cout = 2, 8, 12
    w = _t("fcn.imp.w", (Cout, Cin, 3, 3))
    wd = w.to(dev)
    for k, (b, i, j) in enumerate(_positions(gh, gw)):
        ci, co = (3 * k + 1) % Cin, (5 * k + 2) % Cout
        x = torch.zeros(B, gh * gw, Cin)
        x[b, i * gw + j, ci] = 1.0
        y = ops.conv3x3_tokens(x.to(dev), wd, grid=(gh, gw))
        assert torch.equal(y.cpu(), _scatter(B, gh, gw, b, i, j, w[:, ci], +1)), (b, i, j)
        # two sources: the same impulse in the second one
        y2 = ops.conv3x3_tokens(x[:, :, :4].contiguous().to(dev), wd, xb=x[:, :, 4:].contiguous().to(dev), grid=(gh, gw))
        assert torch.equal(y2, y), (b, i, j)
        d = torch.zeros(B, gh * gw, Cout)
        d[b, i * gw + j, co] = 1.0
        dx = ops.conv3x3_tokens_bwd_data(d.to(dev), wd, (gh, gw))
        assert torch.equal(dx.cpu(), _scatter(B, gh, gw, b, i, j, w[co], -1)), (b, i, j)
        dxs = ops.conv3x3_tokens_bwd_data(d.to(dev), wd, (gh, gw), c_begin=4, c_count=4)
        assert torch.equal(dxs, dx[:, :, 4:8]), (b, i, j)


# ---- accuracy against fp64, element by element --------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,gh,gw", GRIDS)
def test_forward_accuracy(B, gh, gw):
    worst = 0.0
    for Cout in COUTS:
        for Ca, Cb in SOURCES:
            xa, xb, w, bias, scale, _ = _case(B, gh, gw, Ca, Cb, Cout)
            K = 9 * (Ca + Cb)
            for use_bias, act, use_scale in [(False, 0, False), (True, 1, True), (True, 0, False), (False, 1, False), (False, 0, True)]:
                b_, s_ = bias if use_bias else None, scale if use_scale else None
                y = ops.conv3x3_tokens(_g(xa), _g(w), _g(b_), xb=_g(xb), grid=(gh, gw), act=act, out_scale=_g(s_))
                want = R.conv(xa, xb, w, b_, act, s_, gh, gw)
                bound = (K + 2) * U * R.conv_abs(xa, xb, w, b_, s_, gh, gw)
                r = _ratio(y, want, bound)
                worst = max(worst, r)
                assert r <= 1.0, (Cout, Ca, Cb, use_bias, act, use_scale, r)
                if use_scale:
                    assert not y[0].abs().max().item()
    print(f"conv3x3_tokens_fwd rows {B * gh * gw}: largest error / bound = {worst:.4f}")


@pytest.mark.parametrize("B,gh,gw", GRIDS)
def test_backward_data_accuracy(B, gh, gw):
    worst = 0.0
    for Cout in COUTS:
        for Ca, Cb in SOURCES:
            Cin = Ca + Cb
            xa, xb, w, _, _, dpre = _case(B, gh, gw, Ca, Cb, Cout)
            want, _, _ = R.conv_grads(dpre, xa, xb, w, gh, gw)
            bound = (9 * Cout + 2) * U * R.conv_grads(dpre.abs(), xa, xb, w.abs(), gh, gw)[0]
            for c0, cn in [(0, Cin)] + ([(12, 20)] if Cin >= 32 else []):
                dx = ops.conv3x3_tokens_bwd_data(_g(dpre), _g(w), (gh, gw), c_begin=c0, c_count=cn)
                r = _ratio(dx, want[:, :, c0:c0 + cn], bound[:, :, c0:c0 + cn])
                worst = max(worst, r)
                assert r <= 1.0, (Cout, Ca, Cb, c0, cn, r)
    print(f"conv3x3_tokens_bwd_data rows {B * gh * gw}: largest error / bound = {worst:.4f}")


@pytest.mark.parametrize("B,gh,gw", GRIDS)
def test_backward_weight_accuracy(B, gh, gw):
    worst = 0.0
    rows = B * gh * gw
    for Cout in COUTS:
        for Ca, Cb in SOURCES:
            xa, xb, w, _, _, dpre = _case(B, gh, gw, Ca, Cb, Cout)
            _, dw64, db64 = R.conv_grads(dpre, xa, xb, w, gh, gw)
            _, dwb, dbb = R.conv_grads(dpre.abs(), xa.abs(), None if xb is None else xb.abs(), w, gh, gw)
            dw, db = ops.conv3x3_tokens_bwd_weight(_g(dpre), _g(xa), _g(xb), (gh, gw))
            r = max(_ratio(dw, dw64, (rows + 2) * U * dwb), _ratio(db, db64, (rows + 2) * U * dbb))
            worst = max(worst, r)
            assert r <= 1.0, (Cout, Ca, Cb, r)
    print(f"conv3x3_tokens_bwd_weight rows {rows}: largest error / bound = {worst:.4f}")


def test_gate_and_device_scale():
    B, gh, gw, Ca, Cb, Cout = 2, 5, 13, 12, 20, 68
    xa, xb, w, _, _, dpre = _case(B, gh, gw, Ca, Cb, Cout)
    gate = _t("fcn.gate", (B, gh * gw, 20))
    gate[0, :7] = 0.0                                                           # zeros and negatives both close the gate
    dx = ops.conv3x3_tokens_bwd_data(_g(dpre), _g(w), (gh, gw), c_begin=12, c_count=20, gate=_g(gate))
    want = R.conv_grads(dpre, xa, xb, w, gh, gw)[0][:, :, 12:32] * (gate > 0)
    bound = (9 * Cout + 2) * U * R.conv_grads(dpre.abs(), xa, xb, w.abs(), gh, gw)[0][:, :, 12:32]
    assert _ratio(dx, want, bound) <= 1.0
    assert not dx.cpu()[gate <= 0].abs().max().item() and dx.cpu()[gate > 0].abs().min().item() > 0
    half = torch.tensor([0.5], device=dev)
    dw, db = ops.conv3x3_tokens_bwd_weight(_g(dpre), _g(xa), _g(xb), (gh, gw))
    dwh, dbh = ops.conv3x3_tokens_bwd_weight(_g(dpre), _g(xa), _g(xb), (gh, gw), scale=half)
    assert torch.equal(dwh, 0.5 * dw) and torch.equal(dbh, 0.5 * db)            # a power of two: exact
    dwn, dbn = ops.conv3x3_tokens_bwd_weight(_g(dpre), _g(xa), _g(xb), (gh, gw), need_bias=False)
    assert dbn is None and torch.equal(dwn, dw)


@pytest.mark.parametrize("B,gh,gw", [(1, 1, 1), (2, 5, 13), (3, 14, 14)])
def test_head_gradient_accuracy(B, gh, gw):
    Cc, ch = 21, 68
    n = gh * gw
    dl = _t(f"fcn.hg.dl.{n}", (B, n, Cc))
    ws = _t("fcn.hg.ws", (Cc, ch), 0.1)
    y = _t(f"fcn.hg.y.{n}", (B, n, ch))
    y[y < 0] = 0.0
    scale = _t(f"fcn.hg.s.{B}", (B, ch)).abs()
    scale[:, ::4] = 0.0
    for s_, y_ in [(scale, y), (None, y), (scale, None), (None, None)]:
        got = ops.fcn_head_grad(_g(dl), _g(ws), (gh, gw), out_scale=_g(s_), y=_g(y_))
        want = dl.double() @ ws.double()
        bound = (Cc + 2) * U * (dl.double().abs() @ ws.double().abs())
        if s_ is not None:
            want, bound = want * s_.double()[:, None, :], bound * s_.double()[:, None, :]
        if y_ is not None:
            want, bound = want * (y_ > 0), bound * (y_ > 0)
        assert _ratio(got, want, bound) <= 1.0


def test_every_entry_is_repeatable():
    B, gh, gw, Ca, Cb, Cout = 3, 14, 14, 12, 20, 132
    xa, xb, w, bias, scale, dpre = (_g(t) for t in _case(B, gh, gw, Ca, Cb, Cout, tag="rep"))
    wseg = _g(_t("fcn.rep.wseg", (20, Cout), 0.1))
    runs = []
    for _ in range(2):
        y = ops.conv3x3_tokens(xa, w, bias, xb=xb, grid=(gh, gw), act=1, out_scale=scale)
        dx = ops.conv3x3_tokens_bwd_data(dpre, w, (gh, gw), c_begin=12, c_count=20, gate=xb)
        dw, db = ops.conv3x3_tokens_bwd_weight(dpre, xa, xb, (gh, gw))
        hg = ops.fcn_head_grad(xb, wseg, (gh, gw), out_scale=scale, y=y)
        runs.append((y, dx, dw, db, hg))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- refusals and the launch path ---------------------------------------------------------------------------------------------------

SENTINEL = 7.0


def test_refusals_write_nothing():
    lib = _lib.load()
    B, gh, gw, Ca, Cb, Cout = 2, 3, 5, 8, 4, 12
    n = gh * gw
    s = torch.cuda.current_stream().cuda_stream
    xa, xb = torch.ones(B, n, Ca, device=dev), torch.ones(B, n, Cb, device=dev)
    w = torch.ones(Cout, Ca + Cb, 3, 3, device=dev)
    dpre = torch.ones(B, n, Cout, device=dev)
    dl = torch.ones(B, n, 5, device=dev)
    ws = torch.full((1 << 16,), SENTINEL, device=dev)
    outs = [torch.full((B * n * 2048,), SENTINEL, device=dev) for _ in range(2)]
    o, o2 = (t.data_ptr() for t in outs)
    p = lambda t: t.data_ptr()
    nb = ws.numel() * 4

    def fwd(xa_=p(xa), xb_=p(xb), B_=B, gh_=gh, gw_=gw, Ca_=Ca, Cb_=Cb, Cout_=Cout, act=0, ws_=p(ws), nb_=nb):
        return lib.tt_conv3x3_tokens_fwd(xa_, xb_, p(w), None, None, o, B_, gh_, gw_, Ca_, Cb_, Cout_, act, ws_, nb_, s)

    def bdata(Cin=Ca + Cb, Cout_=Cout, c0=0, cn=Ca + Cb, gh_=gh, nb_=nb):
        return lib.tt_conv3x3_tokens_bwd_data(p(dpre), p(w), None, o, B, gh_, gw, Cin, Cout_, c0, cn, p(ws), nb_, s)

    def bweight(Ca_=Ca, Cb_=Cb, Cout_=Cout, xb_=p(xb), gw_=gw, nb_=nb):
        return lib.tt_conv3x3_tokens_bwd_weight(p(dpre), p(xa), xb_, None, o, o2, B, gh, gw_, Ca_, Cb_, Cout_, p(ws), nb_, s)

    def hgrad(Cc=5, ch=Cout, B_=B):
        return lib.tt_fcn_head_grad(p(dl), p(w), None, None, o, B_, gh, gw, Cc, ch, s)

    bad = [lambda: fwd(Ca_=6), lambda: fwd(Cb_=6), lambda: fwd(Cout_=10), lambda: fwd(Ca_=1028), lambda: fwd(Cout_=0), lambda: fwd(gh_=65),
           lambda: fwd(gw_=0), lambda: fwd(B_=0), lambda: fwd(B_=1 << 20, gh_=64, gw_=64), lambda: fwd(act=2), lambda: fwd(xb_=None),
           lambda: fwd(xa_=None), lambda: fwd(xa_=p(xa) + 4), lambda: fwd(ws_=None), lambda: fwd(nb_=9 * (Ca + Cb) * Cout * 4 - 1),
           lambda: bdata(c0=4), lambda: bdata(cn=6), lambda: bdata(c0=-4, cn=4), lambda: bdata(Cout_=1028), lambda: bdata(gh_=65),
           lambda: bdata(nb_=16), lambda: bdata(Cin=4100),
           lambda: bweight(Ca_=6), lambda: bweight(Cout_=1028), lambda: bweight(xb_=None), lambda: bweight(gw_=65), lambda: bweight(nb_=16),
           lambda: hgrad(Cc=257), lambda: hgrad(Cc=0), lambda: hgrad(ch=10), lambda: hgrad(B_=0)]
    for k, call in enumerate(bad):
        assert call() != 0, k
        assert lib.tt_last_error(), k
    torch.cuda.synchronize()
    for t in outs + [ws]:
        assert bool((t == SENTINEL).all())
    assert fwd() == 0 and bdata() == 0 and bweight() == 0 and hgrad() == 0      # the same calls with good arguments run
    torch.cuda.synchronize()
    assert not bool((outs[0] == SENTINEL).all())
    with pytest.raises(ValueError):
        ops.conv3x3_tokens(xa, w, grid=(gh, gw))                                # weight expects Ca + Cb channels
    with pytest.raises(ValueError):
        ops.conv3x3_tokens(xa, w, xb=xb, grid=(gh, gw + 1))
    with pytest.raises(_lib.HipLibraryError):
        ops.conv3x3_tokens(xa.cpu(), w, xb=xb, grid=(gh, gw))


def test_launch_neither_allocates_nor_breaks_capture():
    lib = _lib.load()
    B, gh, gw, Ca, Cb, Cout, Cc = 2, 5, 13, 12, 20, 68, 5
    n, Cin = gh * gw, 32
    xa, xb, w, bias, scale, dpre = _case(B, gh, gw, Ca, Cb, Cout, tag="cap")
    dl = _t("fcn.cap.dl", (B, n, Cc))
    wseg = _t("fcn.cap.wseg", (Cc, Cout), 0.1)
    want_y = R.conv(xa, xb, w, bias, 1, scale, gh, gw)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        xa, xb, w, bias, scale, dpre, dl, wseg = (_g(t) for t in (xa, xb, w, bias, scale, dpre, dl, wseg))
        y = torch.empty(B, n, Cout, device=dev)
        hg = torch.empty(B, n, Cout, device=dev)
        dx = torch.empty(B, n, 20, device=dev)
        dw = torch.empty(Cout, Cin, 3, 3, device=dev)
        db = torch.empty(Cout, device=dev)
        nbs = [lib.tt_conv3x3_tokens_fwd_workspace_bytes(Ca, Cb, Cout), lib.tt_conv3x3_tokens_bwd_data_workspace_bytes(Cout, 20),
               lib.tt_conv3x3_tokens_bwd_weight_workspace_bytes(B * n, Cin, Cout)]
        wss = [torch.empty(nb, dtype=torch.uint8, device=dev) for nb in nbs]
        outputs = (y, hg, dx, dw, db)
        p = lambda t: t.data_ptr()

        def launch():
            s = torch.cuda.current_stream().cuda_stream
            assert lib.tt_conv3x3_tokens_fwd(p(xa), p(xb), p(w), p(bias), p(scale), p(y), B, gh, gw, Ca, Cb, Cout, 1, p(wss[0]), nbs[0], s) == 0
            assert lib.tt_fcn_head_grad(p(dl), p(wseg), p(scale), p(y), p(hg), B, gh, gw, Cc, Cout, s) == 0
            assert lib.tt_conv3x3_tokens_bwd_data(p(hg), p(w), p(xb), p(dx), B, gh, gw, Cin, Cout, 12, 20, p(wss[1]), nbs[1], s) == 0
            assert lib.tt_conv3x3_tokens_bwd_weight(p(hg), p(xa), p(xb), None, p(dw), p(db), B, gh, gw, Ca, Cb, Cout, p(wss[2]), nbs[2], s) == 0

        launch()
        torch.cuda.synchronize()
        first = [t.clone() for t in outputs]
        assert rel_err(y, want_y) <= 1e-5
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(3):
            for t in outputs:
                t.fill_(SENTINEL)
            launch()
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0, "a launch changed the device's free memory"
        assert all(torch.equal(a, b) for a, b in zip(outputs, first))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch()
        for _ in range(2):
            for t in outputs:
                t.fill_(SENTINEL)
            g.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(outputs, first))


# ---- the module ---------------------------------------------------------------------------------------------------------------------

class _FeatureStub(nn.Module):
    """A frozen 'model' whose backbone width is D (FCNFinetune only reads embed_dim from it on these paths)."""

    def __init__(self, D):
        super().__init__()
        self.backbone = nn.Module()
        self.backbone.embed_dim = D
        self.feature_dim = D
        self.keep = nn.Parameter(torch.zeros(1))


def _model(D, channels, Cc, Rr, params=None, **head_args):
    model = FF.FCNFinetune(_FeatureStub(D), Cc, Rr, channels=channels, **head_args).to(dev)
    if params is not None:
        model.decode_head.load_state_dict({k: v for k, v in params.items()})
    return model


def _grads(model):
    return {k: p.grad.clone() for k, p in model.decode_head.named_parameters()}


def test_fused_step_and_module_surface_on_the_fixture(golden):
    g = golden("fcn_head")
    c = R.FIXTURE
    params = {k[len("param."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param.")}
    model = _model(c["D"], c["channels"], c["C"], c["R"], params, num_convs=c["num_convs"], concat_input=c["concat_input"])
    feats = torch.from_numpy(g["feats"]).to(dev)
    labels = torch.from_numpy(g["labels"].astype(np.int64)).to(dev)
    scale = torch.from_numpy(g["out_scale"]).to(dev)
    loss = model.head_loss(feats, labels, out_scale=scale)
    loss.backward()
    fused = _grads(model)
    e_loss = abs(loss.item() - float(g["loss"])) / float(g["loss"])
    print(f"fixture: loss rel. error {e_loss:.3e}")
    assert e_loss <= 1e-3
    for k, v in fused.items():
        e = rel_err(v, g["grad." + k])
        print(f"fixture: grad {k} rel_err {e:.3e}")
        assert e <= 1e-3, k
    # the module surface: forward + F.cross_entropy + backward
    model.zero_grad()
    logits = model.head_forward(feats, out_scale=scale)
    assert logits.shape == (c["B"], c["C"], c["R"], c["R"])
    e = rel_err(logits, g["logits"])
    print(f"fixture: logits rel_err {e:.3e}")
    assert e <= 1e-3
    ref = F.cross_entropy(logits, labels, ignore_index=255)
    ref.backward()
    assert abs(ref.item() - float(g["loss"])) <= 1e-3 * float(g["loss"])
    for k, v in _grads(model).items():
        assert rel_err(v, g["grad." + k]) <= 1e-3, k
        assert rel_err(v, fused[k]) <= 1e-3, k
    # the incoming gradient scales the fused step's gradients
    model.zero_grad()
    (2.0 * model.head_loss(feats, labels, out_scale=scale)).backward()
    for k, v in _grads(model).items():
        assert torch.equal(v, 2 * fused[k]), k
    with pytest.raises(ValueError):
        model.head_loss(feats, torch.full_like(labels, c["C"]), out_scale=scale)


@pytest.mark.parametrize("concat_input", [True, False])
@pytest.mark.parametrize("num_convs", [0, 1, 2])
def test_head_variants(num_convs, concat_input):
    B, g, channels, Cc, Rr = 2, 5, 8, 5, 11
    D = 12 if num_convs else 8                                                  # num_convs = 0 asserts in_channels == channels
    tag = f"fcn.var.{num_convs}.{int(concat_input)}"
    params = R.head_params(tag, D, channels, Cc, num_convs, concat_input)
    model = _model(D, channels, Cc, Rr, params, num_convs=num_convs, concat_input=concat_input)
    feats = _t(tag + ".feats", (B, g * g, D))
    labels = torch.from_numpy(np.random.default_rng(num_convs).integers(0, Cc, (B, Rr, Rr)))
    labels[0, :2] = 255
    scale = torch.tensor([[0.0, 2.0] * (channels // 2), [2.0, 2.0, 0.0, 2.0] * (channels // 4)])
    loss64, grads64, logits64 = R.head_loss_and_grads(feats, params, labels, num_convs, concat_input, scale, g, Rr)
    loss = model.head_loss(feats.to(dev), labels.to(dev), out_scale=scale.to(dev))
    loss.backward()
    assert abs(loss.item() - loss64.item()) <= 1e-3 * loss64.item()
    assert set(dict(model.decode_head.named_parameters())) == set(grads64)
    for k, v in _grads(model).items():
        assert rel_err(v, grads64[k]) <= 1e-3, k
    assert rel_err(model.head_forward(feats.to(dev), out_scale=scale.to(dev)), logits64) <= 1e-3


def test_eval_has_no_dropout_and_predict_is_the_argmax_of_forward():
    B, g, D, channels, Cc, Rr = 3, 6, 16, 16, 7, 20
    params = R.head_params("fcn.eval", D, channels, Cc, 2, True)
    model = _model(D, channels, Cc, Rr, params, num_convs=2, concat_input=True, dropout_ratio=0.5)
    feats = _t("fcn.eval.feats", (B, g * g, D)).to(dev)
    model.train()
    s1, s2 = model.dropout_scale(B, dev), model.dropout_scale(B, dev)
    assert s1.shape == (B, channels) and set(s1.unique().tolist()) <= {0.0, 2.0} and not torch.equal(s1, s2)
    with torch.no_grad():
        assert not torch.equal(model.head_forward(feats), model.head_forward(feats))
    model.eval()
    assert model.dropout_scale(B, dev) is None
    with torch.no_grad():
        a, b = model.head_forward(feats), model.head_forward(feats)
    assert torch.equal(a, b)
    assert rel_err(a, R.head_logits(feats.cpu(), {k: v.double() for k, v in params.items()}, 2, True, None, g, Rr)) <= 1e-3
    pred = model.head_predict(feats)
    top = a.topk(2, dim=1)
    differ = pred != top.indices[:, 0]
    assert bool(((top.values[:, 0] - top.values[:, 1])[differ] < 1e-4).all())   # only near-ties may differ
    model.train()
    assert torch.equal(model.head_predict(feats), pred)                         # predict never drops


def test_learning_sanity():
    """Planted linear features on 8 x 8 tokens, labels = the arg-max of their upsampled planted logits; 20 FusedSGD steps on every
    head parameter, no dropout.  The fp32 CPU restatement of this run (torch.optim.SGD on tests/_fcn_ref.py's head) ends at 0.51 of its
    first loss (lr 0.2, momentum 0.9, from a zero conv_seg), never above it; the bound leaves that run a quarter of margin."""
    from test_linear_probe_host import restate_logits

    B, g, D, channels, Cc, Rr = 4, 8, 16, 16, 5, 24
    feats = _t("fcn.plant.x", (B, g * g, D))
    wt = _t("fcn.plant.w", (Cc, D, 1, 1))
    labels = restate_logits(feats, wt, torch.zeros(Cc), Rr).argmax(1)
    params = R.head_params("fcn.plant", D, channels, Cc, 1, True)
    params["conv_seg.weight"].zero_()
    params["conv_seg.bias"].zero_()
    model = _model(D, channels, Cc, Rr, params, num_convs=1, concat_input=True, dropout_ratio=0.0)
    opt = L.FusedSGD(model.parameters(), lr=0.2, momentum=0.9, weight_decay=0.0001)
    feats, labels = feats.to(dev), labels.to(dev)
    losses = []
    for _ in range(20):
        loss = model.head_loss(feats, labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[0] == pytest.approx(np.log(Cc), rel=1e-5)
    assert losses[-1] < 0.65 * losses[0], losses


def test_main_runs_on_synthetic_data(tmp_path):
    miou = FF.main(["--dataset", "synthetic", "--model_path", "", "--input_resolution", "64", "--mask_size", "32", "--batch_size", "2",
                    "--epochs", "1", "--num_train_images", "4", "--num_val_images", "4", "--num_prototypes", "10", "--head_layers", "64", "32",
                    "--channels", "32", "--save_path", str(tmp_path / "fcn.pth")])
    assert np.isfinite(miou) and 0.0 <= miou <= 1.0
    sd = torch.load(tmp_path / "fcn.pth")
    assert sd["decode_head.convs.1.conv.weight"].shape == (32, 32, 3, 3)
    assert sd["decode_head.conv_cat.conv.weight"].shape == (32, 384 + 32, 3, 3)
    assert sd["decode_head.conv_seg.weight"].shape == (21, 32, 1, 1)
