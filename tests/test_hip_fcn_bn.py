"""The FCN head's norm layers on the GPU (N33): tt_bn_tokens_fwd / tt_bn_tokens_bwd against fp64 with element-wise bounds, the running
statistics, eval mode, repeatability, refusals and the launch path; ``FCNHead(norm_cfg=BN)`` / ``FCNFinetune`` against the fixture
tests/golden/fcn_head_bn.npz and against an fp64 twin of ``nn.Conv2d`` / ``nn.BatchNorm2d`` (tests/_fcn_bn_ref.py).

The bounds, with u = 2^-24, q = (|z| + |mean|) rstd and s = out_scale[r / n, c]: save_mean 2u |mean|, save_rstd 4u rstd, y 8u (q |gamma| +
|beta|) |s|, dbeta 2u sum |g|, dgamma 8u sum(|g| q), dz 8u |gamma| rstd (|g| + mean|g| + q mean(|g| q)).  Each constant counts the roundings
of an fp32 evaluation on fp64 column sums (the mean rounded to fp32, the subtraction, three to six multiplies and adds)."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _fcn_bn_ref as RB
import _fcn_ref as R
from conftest import rel_err
from timetuning_amd import _lib, fcn_finetune as FF, hip_ops as ops, leopart, linear_finetune as L, synth

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
U = R.U
EPS = RB.EPS

GRIDS = [(2, 1, 1), (1, 7, 9), (1, 5, 13), (2, 5, 13), (3, 14, 14)]             # rows 2, 63, 65, 130, 588
CHANNELS = [4, 60, 68, 132]
SENTINEL = 7.0


def _t(name, shape, std=1.0):
    return torch.from_numpy(synth.normal(name, shape, std))


def _g(t):
    return None if t is None else t.to(dev)


def _ratio(got, want, bound):
    """max over the elements of |got - want| / bound (0 / 0 = 0); a non-zero error over a zero bound is infinite."""
    err = (got.detach().cpu().double() - want).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def _y_bound(q, gamma, beta, scale):
    b = 8 * U * (q * gamma.double().abs() + beta.double().abs())
    return b if scale is None else b * scale.double().abs()[:, None, :]


# ---- the kernels against fp64, element by element -----------------------------------------------------------------------------------

@pytest.mark.parametrize("B,gh,gw", GRIDS)
def test_forward_accuracy(B, gh, gw):
    worst = {"mean": 0.0, "rstd": 0.0, "y": 0.0}
    for C in CHANNELS:
        z, gamma, beta, scale, _, rm, rv = RB.bn_case(B, gh, gw, C)
        if B * gh * gw > 2:
            col = z[:, :, 0].double()
            assert abs(float(col.mean() / col.std()) - 100) < 30                # the column with a small variance beside a large mean
        assert bool((gamma < 0).any())
        for use_scale, act in [(False, 0), (True, 1), (False, 1), (True, 0)]:
            s_ = scale if use_scale else None
            y, mean, rstd = ops.bn_tokens(_g(z), _g(gamma), _g(beta), _g(rm), _g(rv), training=True, eps=EPS, act=act, out_scale=_g(s_))
            y64, mean64, _, rstd64, q = RB.bn_forward64(z, gamma, beta, s_, act, EPS)
            r = {"mean": _ratio(mean, mean64, 2 * U * mean64.abs()), "rstd": _ratio(rstd, rstd64, 4 * U * rstd64),
                 "y": _ratio(y, y64, _y_bound(q, gamma, beta, s_))}
            for k, v in r.items():
                worst[k] = max(worst[k], v)
                assert v <= 1.0, (C, use_scale, act, k, v)
            if use_scale and B > 1:
                assert not y[0].abs().max().item()                              # the image whose multipliers are all zero
            if act:
                assert y.min().item() >= 0
    print(f"bn_tokens_fwd rows {B * gh * gw}: largest error / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))


@pytest.mark.parametrize("B,gh,gw", GRIDS)
def test_backward_accuracy(B, gh, gw):
    worst = {"dbeta": 0.0, "dgamma": 0.0, "dz": 0.0}
    rows = B * gh * gw
    for C in CHANNELS:
        z, gamma, beta, _, g, rm, rv = RB.bn_case(B, gh, gw, C)
        g[:, ::2, 1] = 0.0                                                      # as a ReLU gate leaves it
        _, mean, rstd = ops.bn_tokens(_g(z), _g(gamma), _g(beta), None, None, training=True, eps=EPS)
        dz, dgamma, dbeta = ops.bn_tokens_bwd(_g(g), _g(z), mean, rstd, _g(gamma))
        _, mean64, _, rstd64, q = RB.bn_forward64(z, gamma, beta, None, 0, EPS)
        dz64, dgamma64, dbeta64 = RB.bn_backward64(g, z, gamma, mean64, rstd64)
        ga = g.double().abs().reshape(rows, C)
        q2 = q.reshape(rows, C)
        bound_dz = 8 * U * gamma.double().abs() * rstd64 * (ga + ga.mean(0) + q2 * (ga * q2).mean(0))
        r = {"dbeta": _ratio(dbeta, dbeta64, 2 * U * ga.sum(0)), "dgamma": _ratio(dgamma, dgamma64, 8 * U * (ga * q2).sum(0)),
             "dz": _ratio(dz, dz64, bound_dz.reshape(z.shape))}
        for k, v in r.items():
            worst[k] = max(worst[k], v)
            assert v <= 1.0, (C, k, v)
    print(f"bn_tokens_bwd rows {rows}: largest error / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))


@pytest.mark.parametrize("momentum", [0.1, 0.5])
def test_running_statistics_follow_the_recurrence(momentum):
    """running <- (1 - m) running + m stat, the variance unbiased, after one and after three calls.  The kernel evaluates a step in fp64
    and rounds once, so a step's error is at most (1 - m) times the previous one plus u |value|: with A <- (1 - m) A + m |stat| from
    A = |running| that is under 3 u A after three calls; the bound is 4 u A."""
    B, gh, gw, C = 2, 5, 13, 68
    rows = B * gh * gw
    z0, gamma, beta, _, _, rm, rv = RB.bn_case(B, gh, gw, C, tag="run")
    zs = [z0, 0.5 * z0 + 1.0, z0.flip(2).contiguous()]
    rm_d, rv_d = _g(rm), _g(rv)
    rm64, rv64, a_m, a_v = rm.double(), rv.double(), rm.double().abs(), rv.double().abs()
    for k, z in enumerate(zs):
        ops.bn_tokens(_g(z), _g(gamma), _g(beta), rm_d, rv_d, training=True, momentum=momentum, eps=EPS)
        z2 = z.double().reshape(rows, C)
        mean, var = z2.mean(0), z2.var(0, unbiased=True)
        rm64, rv64 = (1 - momentum) * rm64 + momentum * mean, (1 - momentum) * rv64 + momentum * var
        a_m, a_v = (1 - momentum) * a_m + momentum * mean.abs(), (1 - momentum) * a_v + momentum * var
        if k in (0, 2):
            assert _ratio(rm_d, rm64, 4 * U * a_m) <= 1.0, k
            assert _ratio(rv_d, rv64, 4 * U * a_v) <= 1.0, k
    assert not torch.equal(rm_d.cpu(), rm)


@pytest.mark.parametrize("B,gh,gw", [(1, 1, 1), (2, 5, 13), (3, 14, 14)])
def test_eval_mode_normalises_with_the_running_statistics(B, gh, gw):
    lib = _lib.load()
    for C in (4, 68, 132):
        z, gamma, beta, scale, _, rm, rv = RB.bn_case(B, gh, gw, C, tag="eval")
        rm_d, rv_d = _g(rm), _g(rv)
        for use_scale, act in [(False, 1), (True, 1), (False, 0)]:
            s_ = scale if use_scale else None
            y, mean, rstd = ops.bn_tokens(_g(z), _g(gamma), _g(beta), rm_d, rv_d, training=False, eps=EPS, act=act, out_scale=_g(s_))
            assert mean is None and rstd is None
            y64, _, _, _, q = RB.bn_forward64(z, gamma, beta, s_, act, EPS, mean=rm, var=rv)
            want = F.batch_norm(z.double().reshape(-1, C), rm.double(), rv.double(), gamma.double(), beta.double(), training=False, eps=EPS)
            want = (F.relu(want) if act else want).reshape(z.shape) * (1.0 if s_ is None else s_.double()[:, None, :])
            assert float((want - y64).abs().max()) <= 1e-12
            assert _ratio(y, want, _y_bound(q, gamma, beta, s_)) <= 1.0, (C, use_scale, act)
        assert torch.equal(rm_d.cpu(), rm) and torch.equal(rv_d.cpu(), rv)
        # through the C entry: save_mean / save_rstd given in eval mode stay untouched, and no workspace is needed
        zd, gd, bd = _g(z), _g(gamma), _g(beta)
        y = torch.empty_like(zd)
        sm, sr = torch.full((C,), SENTINEL, device=dev), torch.full((C,), SENTINEL, device=dev)
        p = lambda t: t.data_ptr()
        rc = lib.tt_bn_tokens_fwd(p(zd), p(gd), p(bd), None, p(rm_d), p(rv_d), p(y), p(sm), p(sr), B * gh * gw, gh * gw, C, 0, 1, 0.1, EPS,
                                  None, 0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.tt_last_error()
        torch.cuda.synchronize()
        assert bool((sm == SENTINEL).all()) and bool((sr == SENTINEL).all())
        assert torch.equal(rm_d.cpu(), rm) and torch.equal(rv_d.cpu(), rv)
    with pytest.raises(ValueError):
        ops.bn_tokens(_g(z), _g(gamma), _g(beta), None, None, training=False)


def test_every_entry_is_repeatable():
    B, gh, gw, C = 3, 14, 14, 132
    z, gamma, beta, scale, g, rm, rv = RB.bn_case(B, gh, gw, C, tag="rep")
    zd, gd, bd, sd, gg = _g(z), _g(gamma), _g(beta), _g(scale), _g(g)
    runs = []
    for _ in range(2):
        rm_d, rv_d = _g(rm), _g(rv)
        y, mean, rstd = ops.bn_tokens(zd, gd, bd, rm_d, rv_d, training=True, act=1, out_scale=sd)
        ye, _, _ = ops.bn_tokens(zd, gd, bd, rm_d, rv_d, training=False, act=1)
        dz, dgamma, dbeta = ops.bn_tokens_bwd(gg, zd, mean, rstd, gd)
        runs.append((y, mean, rstd, rm_d, rv_d, ye, dz, dgamma, dbeta))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- refusals and the launch path ---------------------------------------------------------------------------------------------------

def test_refusals_write_nothing():
    lib = _lib.load()
    B, n, C = 2, 15, 12
    rows = B * n
    s = torch.cuda.current_stream().cuda_stream
    z, g = torch.ones(rows * 2048, device=dev), torch.ones(rows * 2048, device=dev)
    gamma, beta = torch.ones(2048, device=dev), torch.ones(2048, device=dev)
    scale = torch.ones(B * 2048, device=dev)
    ws = torch.full((1 << 16,), SENTINEL, device=dev)
    outs = [torch.full((rows * 2048,), SENTINEL, device=dev)] + [torch.full((2048,), SENTINEL, device=dev) for _ in range(4)]
    o, sm, sr, rm, rv = (t.data_ptr() for t in outs)
    p = lambda t: t.data_ptr()
    nb = lib.tt_bn_tokens_fwd_workspace_bytes(rows, C)
    assert 0 < nb <= ws.numel() * 4 and nb == lib.tt_bn_tokens_bwd_workspace_bytes(rows, C)

    def fwd(z_=p(z), rows_=rows, n_=n, C_=C, training=1, act=1, mom=0.1, eps=1e-5, ws_=p(ws), nb_=nb, scale_=p(scale), sm_=sm):
        return lib.tt_bn_tokens_fwd(z_, p(gamma), p(beta), scale_, rm, rv, o, sm_, sr, rows_, n_, C_, training, act, mom, eps, ws_, nb_, s)

    def bwd(g_=p(g), rows_=rows, C_=C, ws_=p(ws), nb_=nb, dz_=o):
        return lib.tt_bn_tokens_bwd(g_, p(z), p(gamma), p(beta), p(gamma), dz_, sm, sr, rows_, C_, ws_, nb_, s)

    bad = [lambda: fwd(C_=6), lambda: fwd(C_=1028), lambda: fwd(C_=0), lambda: fwd(rows_=1, n_=1), lambda: fwd(rows_=0), lambda: fwd(eps=0.0),
           lambda: fwd(mom=1.5), lambda: fwd(act=2), lambda: fwd(z_=None), lambda: fwd(z_=p(z) + 4), lambda: fwd(ws_=None), lambda: fwd(nb_=nb - 1),
           lambda: fwd(rows_=1 << 31), lambda: fwd(eps=-1.0), lambda: fwd(mom=-0.1), lambda: fwd(eps=float("nan")), lambda: fwd(training=2),
           lambda: fwd(n_=7), lambda: fwd(n_=0), lambda: fwd(sm_=None), lambda: fwd(scale_=p(scale) + 4),
           lambda: fwd(training=0, C_=6), lambda: fwd(training=0, rows_=0), lambda: fwd(training=0, act=2), lambda: fwd(training=0, eps=0.0),
           lambda: bwd(C_=6), lambda: bwd(C_=1028), lambda: bwd(C_=0), lambda: bwd(rows_=1), lambda: bwd(rows_=0), lambda: bwd(g_=None),
           lambda: bwd(g_=p(g) + 4), lambda: bwd(dz_=o + 4), lambda: bwd(ws_=None), lambda: bwd(nb_=nb - 1)]
    for k, call in enumerate(bad):
        assert call() == -1, k                                                  # TT_EINVAL
        assert lib.tt_last_error(), k
    torch.cuda.synchronize()
    for t in outs + [ws]:
        assert bool((t == SENTINEL).all())
    assert fwd() == 0 and fwd(training=0) == 0 and fwd(rows_=1, n_=1, training=0, scale_=None) == 0   # the same calls with good arguments run
    torch.cuda.synchronize()
    assert not bool((outs[0][:rows * C] == SENTINEL).any()) and bool((outs[0][rows * C:] == SENTINEL).all())
    assert not bool((outs[1][:C] == SENTINEL).any()) and bool((outs[1][C:] == SENTINEL).all())
    assert bwd() == 0
    torch.cuda.synchronize()
    z3, v = torch.ones(2, 15, 12, device=dev), torch.ones(12, device=dev)
    with pytest.raises(ValueError):
        ops.bn_tokens(z3, v, torch.ones(8, device=dev), v.clone(), v.clone(), training=True)
    with pytest.raises(ValueError):
        ops.bn_tokens(torch.ones(1, 1, 12, device=dev), v, v, v.clone(), v.clone(), training=True)   # one row: torch raises there too
    with pytest.raises(ValueError):
        ops.bn_tokens(torch.ones(2, 15, 6, device=dev), v[:6].clone(), v[:6].clone(), v[:6].clone(), v[:6].clone(), training=True)
    with pytest.raises(ValueError):
        ops.bn_tokens(z3, v, v, v.clone(), v.clone(), training=True, out_scale=torch.ones(3, 12, device=dev))
    with pytest.raises(ValueError):
        ops.bn_tokens(z3, v, v, v.clone(), v.clone(), training=True, eps=0.0)
    with pytest.raises(ValueError):
        ops.bn_tokens_bwd(torch.ones(2, 15, 8, device=dev), z3, v, v, v)
    with pytest.raises(_lib.HipLibraryError):
        ops.bn_tokens(z3.cpu(), v, v, v.clone(), v.clone(), training=True)


def test_launch_neither_allocates_nor_breaks_capture():
    lib = _lib.load()
    B, gh, gw, C = 2, 5, 13, 68
    n, rows = gh * gw, 2 * 5 * 13
    z, gamma, beta, scale, g, rm, rv = RB.bn_case(B, gh, gw, C, tag="cap")
    y64, mean64, _, rstd64, _ = RB.bn_forward64(z, gamma, beta, scale, 1, EPS)
    dz64, _, _ = RB.bn_backward64(g, z, gamma, mean64, rstd64)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        z, gamma, beta, scale, g = (_g(t) for t in (z, gamma, beta, scale, g))
        rm_d, rv_d = _g(rm), _g(rv)
        y, dz = torch.empty(B, n, C, device=dev), torch.empty(B, n, C, device=dev)
        sm, sr, dgamma, dbeta = (torch.empty(C, device=dev) for _ in range(4))
        nbs = [lib.tt_bn_tokens_fwd_workspace_bytes(rows, C), lib.tt_bn_tokens_bwd_workspace_bytes(rows, C)]
        wss = [torch.empty(nb, dtype=torch.uint8, device=dev) for nb in nbs]
        outputs = (y, sm, sr, dz, dgamma, dbeta)
        p = lambda t: t.data_ptr()

        def launch():
            s = torch.cuda.current_stream().cuda_stream
            assert lib.tt_bn_tokens_fwd(p(z), p(gamma), p(beta), p(scale), p(rm_d), p(rv_d), p(y), p(sm), p(sr), rows, n, C, 1, 1, 0.1, EPS,
                                        p(wss[0]), nbs[0], s) == 0
            assert lib.tt_bn_tokens_bwd(p(g), p(z), p(sm), p(sr), p(gamma), p(dz), p(dgamma), p(dbeta), rows, C, p(wss[1]), nbs[1], s) == 0

        launch()
        torch.cuda.synchronize()
        first = [t.clone() for t in outputs]
        assert rel_err(y, y64) <= 1e-5 and rel_err(dz, dz64) <= 1e-5
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(3):
            for t in outputs:
                t.fill_(SENTINEL)
            launch()
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0, "a launch changed the device's free memory"
        assert all(torch.equal(a, b) for a, b in zip(outputs, first))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            launch()
        for _ in range(2):
            for t in outputs:
                t.fill_(SENTINEL)
            graph.replay()
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


def _model(D, channels, Cc, Rr, state=None, norm_cfg=RB.BN, **head_args):
    model = FF.FCNFinetune(_FeatureStub(D), Cc, Rr, channels=channels, norm_cfg=norm_cfg, **head_args).to(dev)
    if state is not None:
        model.decode_head.load_state_dict(state, strict=True)
    return model


def _grads(model):
    return {k: p.grad.clone() for k, p in model.decode_head.named_parameters()}


def _buffers(model):
    return {k: v.clone() for k, v in model.decode_head.named_buffers()}


def _fixture(golden):
    g = golden("fcn_head_bn")
    state = {k[len("state."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("state.")}
    return g, state, torch.from_numpy(g["feats"]).to(dev), torch.from_numpy(g["labels"].astype(np.int64)).to(dev), torch.from_numpy(g["out_scale"]).to(dev)


def test_fused_step_and_autograd_route_on_the_fixture(golden):
    g, state, feats, labels, scale = _fixture(golden)
    c = RB.FIXTURE
    model = _model(c["D"], c["channels"], c["C"], c["R"], state, num_convs=c["num_convs"], concat_input=c["concat_input"])
    loss = model.head_loss(feats, labels, out_scale=scale)
    loss.backward()
    fused = _grads(model)
    e_loss = abs(loss.item() - float(g["loss"])) / float(g["loss"])
    print(f"bn fixture: loss rel. error {e_loss:.3e}")
    assert e_loss <= 1e-5
    assert sorted(fused) == sorted(RB.param_keys(c["num_convs"], c["concat_input"]))
    for k, v in fused.items():
        e = rel_err(v, g["grad." + k])
        print(f"bn fixture: grad {k} rel_err {e:.3e}")
        assert e <= 1e-5, k
    after = _buffers(model)
    for k, v in after.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 4, k                                               # 3 in the fixture's state, one training forward
        else:
            assert rel_err(v, g["after." + k]) <= 1e-5, k
    # the autograd route: forward + F.cross_entropy + backward, from the same state
    model.decode_head.load_state_dict(state, strict=True)
    model.zero_grad()
    logits = model.head_forward(feats, out_scale=scale)
    assert logits.shape == (c["B"], c["C"], c["R"], c["R"])
    e = rel_err(logits, g["logits"])
    print(f"bn fixture: logits rel_err {e:.3e}")
    assert e <= 1e-5
    ref = F.cross_entropy(logits, labels, ignore_index=255)
    ref.backward()
    assert abs(ref.item() - float(g["loss"])) <= 1e-5 * float(g["loss"])
    for k, v in _grads(model).items():
        assert rel_err(v, g["grad." + k]) <= 1e-5, k
        assert rel_err(v, fused[k]) <= 1e-5, k
    for k, v in _buffers(model).items():
        assert torch.equal(v, after[k]), k                                      # the same forward: the same buffers, bit for bit
    # the incoming gradient scales the fused step's gradients
    model.decode_head.load_state_dict(state, strict=True)
    model.zero_grad()
    (2.0 * model.head_loss(feats, labels, out_scale=scale)).backward()
    for k, v in _grads(model).items():
        assert torch.equal(v, 2 * fused[k]), k


def test_three_sgd_steps_follow_the_fp64_twin(golden):
    g, state, feats, labels, _ = _fixture(golden)
    c = RB.FIXTURE
    model = _model(c["D"], c["channels"], c["C"], c["R"], state, num_convs=c["num_convs"], concat_input=c["concat_input"])
    twin = RB.TwinHead(c["D"], c["channels"], c["C"], c["num_convs"], c["concat_input"]).double()
    twin.load_state_dict(state, strict=True)
    model.train()
    twin.train()
    hyper = dict(lr=0.1, momentum=0.9, weight_decay=1e-4)
    opt, opt64 = L.FusedSGD(model.parameters(), **hyper), torch.optim.SGD(twin.parameters(), **hyper)
    x64 = R.to_nchw(feats.cpu(), c["g"], c["g"])
    rng = np.random.default_rng(33)
    for step in range(3):
        scale = torch.from_numpy(((rng.random((c["B"], c["channels"])) >= 0.25) / 0.75).astype(np.float32))
        loss64 = F.cross_entropy(twin(x64, scale, c["R"]), labels.cpu(), ignore_index=255)
        opt64.zero_grad()
        loss64.backward()
        opt64.step()
        loss = model.head_loss(feats, labels, out_scale=scale.to(dev))
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert abs(loss.item() - loss64.item()) <= 1e-5 * loss64.item(), step
    want = twin.state_dict()
    got = model.decode_head.state_dict()
    assert list(got) == list(want)
    for k, v in got.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(want[k]) == 6, k
        else:
            e = rel_err(v, want[k])
            print(f"bn three steps: {k} rel_err {e:.3e}")
            assert e <= 1e-5, k
            assert not torch.equal(v.cpu(), state[k]), k                        # everything moved


@pytest.mark.parametrize("concat_input", [True, False])
@pytest.mark.parametrize("num_convs", [0, 1, 2])
def test_head_variants(num_convs, concat_input):
    B, g, channels, Cc, Rr = 2, 5, 8, 5, 11
    D = 12 if num_convs else 8                                                  # num_convs = 0 asserts in_channels == channels
    tag = f"fcn.bn.var.{num_convs}.{int(concat_input)}"
    state = RB.head_state(tag, D, channels, Cc, num_convs, concat_input)
    model = _model(D, channels, Cc, Rr, state, num_convs=num_convs, concat_input=concat_input)
    feats = _t(tag + ".feats", (B, g * g, D))
    labels = torch.from_numpy(np.random.default_rng(num_convs).integers(0, Cc, (B, Rr, Rr)))
    labels[0, :2] = 255
    scale = torch.tensor([[0.0, 2.0] * (channels // 2), [2.0, 2.0, 0.0, 2.0] * (channels // 4)])
    loss64, grads64, logits64, buffers64 = RB.head_loss_and_grads(feats, state, labels, num_convs, concat_input, scale, g, Rr)
    loss = model.head_loss(feats.to(dev), labels.to(dev), out_scale=scale.to(dev))
    loss.backward()
    assert abs(loss.item() - loss64.item()) <= 1e-5 * loss64.item()
    assert set(dict(model.decode_head.named_parameters())) == set(grads64)
    for k, v in _grads(model).items():
        assert rel_err(v, grads64[k]) <= 1e-5, k
    for k, v in buffers64.items():
        assert rel_err(model.decode_head.state_dict()[k], v) <= 1e-5, k
    assert rel_err(model.head_forward(feats.to(dev), out_scale=scale.to(dev)), logits64) <= 1e-5
    n_modules = num_convs + int(concat_input)
    assert sum(int(v) for k, v in model.decode_head.state_dict().items() if k.endswith("num_batches_tracked")) == (3 + 2) * n_modules


def test_eval_uses_the_running_statistics_and_moves_no_buffer(golden):
    g, state, feats, labels, _ = _fixture(golden)
    c = RB.FIXTURE
    model = _model(c["D"], c["channels"], c["C"], c["R"], state, num_convs=c["num_convs"], concat_input=c["concat_input"], dropout_ratio=0.5)
    twin = RB.TwinHead(c["D"], c["channels"], c["C"], c["num_convs"], c["concat_input"]).double()
    twin.load_state_dict(state, strict=True)
    twin.eval()
    model.eval()
    before = _buffers(model)
    with torch.no_grad():
        a, b = model.head_forward(feats), model.head_forward(feats)
        want = twin(R.to_nchw(feats.cpu(), c["g"], c["g"]), None, c["R"])
    assert torch.equal(a, b)
    e = rel_err(a, want)
    print(f"bn eval: logits rel_err {e:.3e}")
    assert e <= 1e-5
    pred = model.head_predict(feats)
    top = a.topk(2, dim=1)
    differ = pred != top.indices[:, 0]
    assert bool(((top.values[:, 0] - top.values[:, 1])[differ] < 1e-4).all())   # only near-ties may differ
    # the token-resolution head in eval mode, and a backward on running statistics, which is not built
    low = model.decode_head(feats, (c["g"], c["g"]))
    assert low.shape == (c["B"], c["g"] ** 2, c["C"])
    with pytest.raises(NotImplementedError):
        model.head_loss(feats, labels)
    for k, v in _buffers(model).items():
        assert torch.equal(v, before[k]), k
    model.train()
    assert torch.equal(model.head_predict(feats), pred)                         # predict never drops and never uses batch statistics
    for k, v in _buffers(model).items():
        assert torch.equal(v, before[k]), k
    with torch.no_grad():
        train_logits = model.head_forward(feats, out_scale=torch.ones(c["B"], c["channels"], device=dev))
    assert not torch.equal(train_logits, a)                                     # batch statistics differ from the running ones
    assert int(model.decode_head.convs[0].bn.num_batches_tracked) == 3 + 1      # the one forward in train()


def test_frozen_norm_parameters_get_no_gradient_and_do_not_move(golden):
    g, state, feats, labels, scale = _fixture(golden)
    c = RB.FIXTURE
    model = _model(c["D"], c["channels"], c["C"], c["R"], state, norm_cfg=dict(type="BN", requires_grad=False), num_convs=c["num_convs"],
                   concat_input=c["concat_input"])
    opt = L.FusedSGD([p for p in model.parameters()], lr=0.1, momentum=0.9)
    for route in ("fused", "autograd"):
        opt.zero_grad()
        if route == "fused":
            model.head_loss(feats, labels, out_scale=scale).backward()
        else:
            F.cross_entropy(model.head_forward(feats, out_scale=scale), labels, ignore_index=255).backward()
        for k, p in model.decode_head.named_parameters():
            if ".bn." in k:
                assert p.grad is None, (route, k)
            else:
                assert rel_err(p.grad, g["grad." + k]) <= 1e-5, (route, k)      # the frozen values are the fixture's
        model.decode_head.load_state_dict(state, strict=True)
    model.head_loss(feats, labels, out_scale=scale).backward()
    opt.step()
    for k, v in model.decode_head.state_dict().items():
        if k.endswith(("bn.weight", "bn.bias")):
            assert torch.equal(v.cpu(), state[k]), k
        elif k.endswith("weight"):
            assert not torch.equal(v.cpu(), state[k]), k


def test_norm_cfg_none_is_the_head_without_the_argument():
    c = R.FIXTURE
    feats, params, labels, scale = R.fixture_inputs()
    feats, labels, scale = feats.to(dev), labels.to(dev), scale.to(dev)
    out = []
    for kwargs in (dict(), dict(norm_cfg=None)):
        model = FF.FCNFinetune(_FeatureStub(c["D"]), c["C"], c["R"], channels=c["channels"], num_convs=c["num_convs"],
                               concat_input=c["concat_input"], **kwargs).to(dev)
        model.decode_head.load_state_dict(params, strict=True)
        model.head_loss(feats, labels, out_scale=scale).backward()
        out.append((model.head_forward(feats, out_scale=scale).detach(), _grads(model)))
    assert torch.equal(out[0][0], out[1][0])
    for k, v in out[0][1].items():
        assert torch.equal(v, out[1][1][k]), k
    g64 = R.head_loss_and_grads(feats.cpu(), params, labels.cpu(), c["num_convs"], c["concat_input"], scale.cpu(), c["g"], c["R"])[1]
    for k, v in out[1][1].items():
        assert rel_err(v, g64[k]) <= 1e-3, k                                    # N32's contract, unchanged


LEARNING = dict(B=4, g=8, D=16, channels=16, C=5, R=24, steps=20, lr=0.2, momentum=0.9, weight_decay=0.0001)
LEARNING_BOUND = 0.55


def learning_inputs():
    from test_linear_probe_host import restate_logits

    c = LEARNING
    feats = _t("fcn.plant.x", (c["B"], c["g"] ** 2, c["D"]))
    wt = _t("fcn.plant.w", (c["C"], c["D"], 1, 1))
    labels = restate_logits(feats, wt, torch.zeros(c["C"]), c["R"]).argmax(1)
    twin = RB.TwinHead(c["D"], c["channels"], c["C"], 1, True)
    state = {k: v.clone() for k, v in twin.state_dict().items()}
    for k, v in R.head_params("fcn.bn.plant", c["D"], c["channels"], c["C"], 1, True).items():
        if k in state:
            state[k] = v
    state["conv_seg.weight"] = torch.zeros_like(state["conv_seg.weight"])
    state["conv_seg.bias"] = torch.zeros_like(state["conv_seg.bias"])
    return feats, labels, state


def test_learning_sanity():
    """N32's planted run with norm layers: linear features on 8 x 8 tokens, labels = the arg-max of their upsampled planted logits, 20
    FusedSGD steps on every head parameter from fresh norm layers and a zero conv_seg, no dropout.  The fp32 CPU run of the twin
    (``learning_inputs`` + torch.optim.SGD) ends at 0.43 of its first loss, never above it; the bound leaves that run a quarter of margin, as
    N32's does."""
    c = LEARNING
    feats, labels, state = learning_inputs()
    model = _model(c["D"], c["channels"], c["C"], c["R"], state, num_convs=1, concat_input=True, dropout_ratio=0.0)
    opt = L.FusedSGD(model.parameters(), lr=c["lr"], momentum=c["momentum"], weight_decay=c["weight_decay"])
    feats, labels = feats.to(dev), labels.to(dev)
    losses = []
    for _ in range(c["steps"]):
        loss = model.head_loss(feats, labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("bn learning sanity:", " ".join(f"{v:.4f}" for v in losses))
    assert losses[0] == pytest.approx(np.log(c["C"]), rel=1e-5)
    assert losses[-1] < LEARNING_BOUND * losses[0], losses


def test_main_runs_with_norm_layers_and_the_checkpoint_loads_back(tmp_path):
    miou = FF.main(["--dataset", "synthetic", "--model_path", "", "--input_resolution", "64", "--mask_size", "32", "--batch_size", "2",
                    "--epochs", "1", "--num_train_images", "4", "--num_val_images", "4", "--num_prototypes", "10", "--head_layers", "64", "32",
                    "--channels", "32", "--norm", "bn", "--save_path", str(tmp_path / "fcn_bn.pth")])
    assert np.isfinite(miou) and 0.0 <= miou <= 1.0
    sd = torch.load(tmp_path / "fcn_bn.pth")
    head_sd = {k[len("decode_head."):]: v for k, v in sd.items() if k.startswith("decode_head.")}
    assert list(head_sd) == RB.head_keys(2, True) and not any(k.endswith("conv.bias") for k in head_sd)
    assert head_sd["conv_cat.conv.weight"].shape == (32, 384 + 32, 3, 3) and head_sd["convs.1.bn.running_var"].shape == (32,)
    assert int(head_sd["convs.0.bn.num_batches_tracked"]) == 2                  # two training batches; validation moves nothing
    assert float(head_sd["conv_cat.bn.running_mean"].abs().max()) > 0
    head = leopart.FCNHead(384, 32, num_classes=21, norm_cfg=dict(type="BN", requires_grad=True))
    head.load_state_dict(head_sd, strict=True)
    twin = RB.TwinHead(384, 32, 21, 2, True)
    twin.load_state_dict(head_sd, strict=True)
