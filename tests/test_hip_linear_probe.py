"""Linear-probe fine-tuning on the GPU (N5): every kernel against an fp64 torch-CPU restatement, the module surface and the fused
step against the reference's outputs (tests/golden/linear_probe.npz), FusedSGD against torch.optim.SGD, the memory bound of the fused
head step, a learning run and the training driver."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import rel_err
from test_linear_probe_host import golden_inputs, restate_logits
from timetuning_amd import hip_ops as ops, linear_finetune as L, synth

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)


def _up64(low, g, R):
    """[B, g*g, C] -> [B, C, R, R] fp64 bilinear upsampling (align_corners=False)."""
    B, n, C = low.shape
    return F.interpolate(low.permute(0, 2, 1).reshape(B, C, g, g), size=(R, R), mode="bilinear", align_corners=False)


@pytest.mark.parametrize("rows,D,C", [(47040, 384, 21), (1001, 768, 256), (7, 384, 1)])
def test_probe_logits(rows, D, C):
    x = torch.from_numpy(synth.normal(f"pl.x.{rows}", (rows, D)))
    w = torch.from_numpy(synth.normal(f"pl.w.{rows}", (C, D), 0.05))
    b = torch.from_numpy(synth.normal(f"pl.b.{rows}", (C,), 0.1))
    out = ops.probe_logits(x.to(dev), w.to(dev), b.to(dev))
    ref = x.double() @ w.double().t() + b.double()
    assert rel_err(out, ref) <= 1e-6


def _labels(B, R, C, ignored, seed):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, C, (B, R, R))
    if ignored >= 1.0:
        y[:] = 255
    elif ignored > 0:
        y[rng.random((B, R, R)) < ignored] = 255
    return torch.from_numpy(y.astype(np.int64))


@pytest.mark.parametrize("ignored", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("g,R", [(28, 100), (14, 224), (28, 28), (7, 100), (28, 37)])
def test_probe_upsample_ce(g, R, ignored):
    B, C = 3, 21
    low = torch.from_numpy(synth.normal(f"ce.low.{g}.{R}", (B, g * g, C), 2.0))
    y = _labels(B, R, C, ignored, seed=g * 1000 + R)
    loss, dlow, counts = ops.probe_upsample_ce(low.to(dev), y.to(dev))
    loss2, dlow2, _ = ops.probe_upsample_ce(low.to(dev), y.to(dev))
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(dlow, dlow2)   # deterministic, bit for bit (NaN too)
    l64 = low.double().requires_grad_(True)
    ref = F.cross_entropy(_up64(l64, g, R), y, ignore_index=255)
    ref.backward()
    assert int(counts[0]) == int((y != 255).sum()) and int(counts[1]) == 0
    if ignored >= 1.0:
        assert torch.isnan(ref) and torch.isnan(loss).all()
        assert not dlow.abs().max().item() and not l64.grad.abs().max().item()
        return
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    assert rel_err(dlow, l64.grad) <= 1e-5


def test_invalid_labels_are_counted_and_raise():
    B, g, C, R = 2, 28, 21, 100
    low = torch.from_numpy(synth.normal("ce.bad", (B, g * g, C))).to(dev)
    y = _labels(B, R, C, 0.2, seed=3)
    y[0, 5, 7], y[1, 99, 99], y[1, 0, 0] = C, -1, 1 << 40        # out of range in both directions; never read as an index
    loss, dlow, counts = ops.probe_upsample_ce(low, y.to(dev))
    torch.cuda.synchronize()
    assert int(counts[1]) == 3
    model = L.LinearFinetune(_FeatureStub(16), C, R).to(dev)
    feats = torch.from_numpy(synth.normal("ce.bad.f", (B, g * g, 16))).to(dev)
    bad = torch.zeros(B, R, R, dtype=torch.int64)
    bad[1, 50, 50] = C
    with pytest.raises(ValueError):
        model.head_loss(feats, bad.to(dev))
    torch.cuda.synchronize()


@pytest.mark.parametrize("g,R,C", [(28, 100, 21), (14, 224, 5), (7, 100, 256), (28, 37, 21)])
def test_bilinear_adjoint_and_wgrad(g, R, C):
    B, D = 2, 384
    d_hi = torch.from_numpy(synth.normal(f"adj.{g}.{R}.{C}", (B, R * R, C)))
    d_low = ops.bilinear_adjoint_tokens(d_hi.to(dev), g)
    l64 = torch.zeros(B, g * g, C, dtype=torch.float64, requires_grad=True)
    up = _up64(l64, g, R)
    (up * d_hi.double().view(B, R, R, C).permute(0, 3, 1, 2)).sum().backward()
    assert rel_err(d_low, l64.grad) <= 1e-6
    feats = torch.from_numpy(synth.normal(f"wg.{g}.{C}", (B * g * g, D)))
    scale = torch.tensor([0.5], device=dev)
    dw, db = ops.probe_wgrad(d_low.view(B * g * g, C), feats.to(dev), scale)
    dl = d_low.view(B * g * g, C).cpu().double()
    assert rel_err(dw, 0.5 * dl.t() @ feats.double()) <= 1e-6
    assert rel_err(db, 0.5 * dl.sum(0)) <= 1e-6


def test_fused_sgd_matches_torch_sgd():
    shapes = [(21, 384, 1, 1), (21,), (7, 5)]
    ps = [torch.from_numpy(synth.normal(f"sgd.p{i}", s)) for i, s in enumerate(shapes)]
    mine = [nn.Parameter(p.clone().to(dev)) for p in ps]
    ref = [nn.Parameter(p.clone()) for p in ps]
    kw = dict(lr=0.01, momentum=0.9, weight_decay=0.0001)
    o1, o2 = L.FusedSGD(mine, **kw), torch.optim.SGD(ref, **kw)
    s1, s2 = torch.optim.lr_scheduler.StepLR(o1, 2, 0.1), torch.optim.lr_scheduler.StepLR(o2, 2, 0.1)
    for step in range(5):
        for i, s in enumerate(shapes):
            gr = torch.from_numpy(synth.normal(f"sgd.g{i}.{step}", s))
            mine[i].grad, ref[i].grad = gr.to(dev), gr.clone()
        o1.step(); o2.step(); s1.step(); s2.step()
        for a, b in zip(mine, ref):
            assert rel_err(a, b) <= 1e-6
    for a, b in zip(mine, ref):
        assert rel_err(o1.state[a]["momentum_buffer"], o2.state[b]["momentum_buffer"]) <= 1e-6
    # state dicts interchange both ways
    o3 = torch.optim.SGD([nn.Parameter(p.clone()) for p in ps], **kw)
    o3.load_state_dict(o1.state_dict())
    o4 = L.FusedSGD([nn.Parameter(p.clone().to(dev)) for p in ps], **kw)
    o4.load_state_dict(o2.state_dict())
    assert o3.param_groups[0]["lr"] == o1.param_groups[0]["lr"]
    assert torch.equal(o4.state[o4.param_groups[0]["params"][0]]["momentum_buffer"].cpu(), o2.state[ref[0]]["momentum_buffer"])


class _FeatureStub(nn.Module):
    """A frozen 'model' whose backbone width is D (LinearFinetune only reads embed_dim from it on these paths)."""

    def __init__(self, D):
        super().__init__()
        self.backbone = nn.Module()
        self.backbone.embed_dim = D
        self.feature_dim = D
        self.keep = nn.Parameter(torch.zeros(1))


def _golden_model(g):
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    Bn, res, C, R, D, depth, heads, patch, K, seed = [int(v) for v in g["cfg"]]
    fe = FeatureExtractor("dino-s8", "", [int(v) for v in g["head_list"]], vit_cfg=dict(embed_dim=D, depth=depth, num_heads=heads, patch_size=patch),
                          init=str(g["mode"]), seed=seed, return_attention=False)
    model = L.LinearFinetune(TimeT(fe, K), C, R).to(dev)
    x, y01, feats, w0, b0 = golden_inputs(g)
    with torch.no_grad():
        model.finetune_head.weight.copy_(w0)
        model.finetune_head.bias.copy_(b0)
    return model, R, x, y01, feats


def test_module_surface_against_the_reference(golden):
    g = golden("linear_probe")
    model, R, x_cpu, y01, feats_cpu = _golden_model(g)
    x = x_cpu.to(dev)
    labels = torch.from_numpy(g["labels"].astype(np.int64)).to(dev)
    feats = feats_cpu.to(dev)
    assert rel_err(model._features(x, False), feats_cpu) <= 1e-4              # the HIP backbone (its own contract is tested elsewhere)
    # the head on the reference's features: logits, loss and gradients through the module surface
    logits = model.head_forward(feats)
    loss = F.cross_entropy(logits, labels, ignore_index=255)
    loss.backward()
    assert rel_err(logits, g["logits"]) <= 1e-5
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * float(g["loss"])
    assert rel_err(model.finetune_head.weight.grad, g["dw"]) <= 1e-5
    assert rel_err(model.finetune_head.bias.grad, g["db"]) <= 1e-5
    # end to end from the images
    assert rel_err(model(x), g["logits"]) <= 1e-4
    # three steps of the reference loop with FusedSGD + StepLR(1, 0.5)
    model.zero_grad()
    opt = L.FusedSGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=0.0001)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    for step in range(3):
        loss = F.cross_entropy(model.head_forward(feats), labels, ignore_index=255)
        assert abs(loss.item() - float(g[f"loss_step{step}"])) <= 1e-5 * float(g[f"loss_step{step}"])
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
    assert rel_err(model.finetune_head.weight, g["w3"]) <= 1e-5
    assert rel_err(model.finetune_head.bias, g["b3"]) <= 1e-5
    assert rel_err(opt.state[model.finetune_head.weight]["momentum_buffer"], g["mw3"]) <= 1e-5
    assert rel_err(opt.state[model.finetune_head.bias]["momentum_buffer"], g["mb3"]) <= 1e-5
    # validation: predictions from the token-resolution logits; only near-ties may differ
    pred = model.predict(x).cpu().numpy()
    differ = pred != g["pred"]
    assert (g["margin"][differ] < 1e-4).all(), (differ.sum(), g["margin"][differ].max() if differ.any() else 0)
    miou = L.validate(model, [(x_cpu, y01)], 0)
    # equal when the predictions are; a flipped near-tie pixel moves it by at most a few of its share
    assert miou == pytest.approx(float(g["miou"]), abs=1e-12 if not differ.any() else 1e-3)


def test_fused_step_against_the_reference_and_the_module_surface(golden):
    g = golden("linear_probe")
    model, R, _, _, feats = _golden_model(g)
    feats = feats.to(dev)
    labels = torch.from_numpy(g["labels"].astype(np.int64)).to(dev)
    loss = model.head_loss(feats, labels)
    loss.backward()
    dw, db = model.finetune_head.weight.grad.clone(), model.finetune_head.bias.grad.clone()
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * float(g["loss"])
    assert rel_err(dw, g["dw"]) <= 1e-5 and rel_err(db, g["db"]) <= 1e-5
    model.zero_grad()
    ref = F.cross_entropy(model.head_forward(feats), labels, ignore_index=255)
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-6 * abs(ref.item())
    assert rel_err(dw, model.finetune_head.weight.grad) <= 1e-6
    assert rel_err(db, model.finetune_head.bias.grad) <= 1e-6
    # the incoming gradient scales the fused step's gradients
    model.zero_grad()
    (2.0 * model.head_loss(feats, labels)).backward()
    assert rel_err(model.finetune_head.weight.grad, 2 * dw) <= 1e-6


def test_fused_head_step_memory():
    B, g, R, D, C = 16, 28, 100, 384, 21
    model = L.LinearFinetune(_FeatureStub(D), C, R).to(dev)
    opt = L.FusedSGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=0.0001)
    feats = torch.from_numpy(synth.normal("mem.f", (B, g * g, D))).to(dev)
    labels = _labels(B, R, C, 0.1, seed=9).to(dev)
    model.finetune_head.weight.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = model.head_loss(feats, labels)
    opt.zero_grad()
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    raised = torch.cuda.max_memory_allocated() - base
    assert raised < B * D * R * R * 4 / 4, raised


def test_learning_sanity():
    """Planted linear features, labels = the arg-max of their upsampled planted logits; 30 FusedSGD steps from a zero head.  The
    fp32 CPU restatement of this run ends at 0.19 of its first loss."""
    B, g, D, C, R = 8, 14, 64, 5, 56
    feats = torch.from_numpy(synth.normal("lp.plant.x", (B, g * g, D)))
    wt = torch.from_numpy(synth.normal("lp.plant.w", (C, D, 1, 1)))
    labels = restate_logits(feats, wt, torch.zeros(C), R).argmax(1)
    model = L.LinearFinetune(_FeatureStub(D), C, R).to(dev)
    nn.init.zeros_(model.finetune_head.weight)
    nn.init.zeros_(model.finetune_head.bias)
    opt = L.FusedSGD(model.parameters(), lr=0.3, momentum=0.9, weight_decay=0.0001)
    feats, labels = feats.to(dev), labels.to(dev)
    losses = []
    for _ in range(30):
        loss = model.head_loss(feats, labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[0] == pytest.approx(np.log(C), rel=1e-5)
    assert losses[-1] < 0.3 * losses[0], losses


def test_main_runs_on_synthetic_data(tmp_path):
    miou = L.main(["--dataset", "synthetic", "--model_path", "", "--input_resolution", "64", "--mask_size", "32", "--batch_size", "2",
                   "--epochs", "1", "--num_train_images", "4", "--num_val_images", "2", "--num_prototypes", "10", "--head_layers", "64", "32",
                   "--save_path", str(tmp_path / "lf.pth")])
    assert np.isfinite(miou) and 0.0 <= miou <= 1.0
    sd = torch.load(tmp_path / "lf.pth")
    assert sd["finetune_head.weight"].shape == (21, 384, 1, 1)
