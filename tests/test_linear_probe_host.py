"""CPU checks of the linear-probe fine-tuning surface (N5, ``timetuning_amd.linear_finetune``).

The torch restatement below is what the GPU tests (test_hip_linear_probe.py) hold the kernels to: the head applied at token
resolution and its C logits upsampled, the commuted order of the reference's ``linear_finetune.py:23-31``.  Here it is held to the
reference's own outputs (tests/golden/linear_probe.npz, tools/gen_linear_probe_golden.py), which shows that the commutation is exact
up to rounding and that the restatement is the reference.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from timetuning_amd import _lib, linear_finetune as L


def restate_logits(feats, w, b, R):
    """feats [B, g*g, D], conv weight [C, D, 1, 1], bias [C] -> [B, C, R, R] logits, head first, then bilinear upsampling."""
    B, n, D = feats.shape
    g = int(round(n ** 0.5))
    low = feats @ w.reshape(w.shape[0], D).t() + b                       # [B, n, C]
    low = low.permute(0, 2, 1).reshape(B, -1, g, g)
    return F.interpolate(low, size=(R, R), mode="bilinear", align_corners=False)


def restate_step(feats, w, b, labels, R):
    """(logits, loss, dW, db) of CrossEntropyLoss(ignore_index=255) through the restatement, by autograd."""
    w = w.detach().clone().requires_grad_(True)
    b = b.detach().clone().requires_grad_(True)
    logits = restate_logits(feats, w, b, R)
    loss = F.cross_entropy(logits, labels, ignore_index=255)
    loss.backward()
    return logits.detach(), loss.detach(), w.grad, b.grad


def golden_inputs(g):
    """The inputs of linear_probe.npz, regenerated as tools/gen_linear_probe_golden.py made them (the fixture stores only samples
    of them): images and labels from ``synthetic_segmentation``, the head from ``synth.normal``, and the backbone features from the
    oracle's restatement of the backbone on the same synthetic weights.  Returns (x, y01, feats, w0, b0)."""
    from oracle import timet_oracle as O
    from timetuning_amd import synth

    Bn, res, C, R, D, depth, heads, patch, K, seed = [int(v) for v in g["cfg"]]
    x, y01 = L.synthetic_segmentation(Bn, res, C, seed=seed)
    w0 = torch.from_numpy(synth.normal("lp.golden.w", (C, D, 1, 1), 0.05, 0.0, seed))
    b0 = torch.from_numpy(synth.normal("lp.golden.b", (C,), 0.1, 0.0, seed))
    om = O.build_oracle("dino-s8", K, [int(v) for v in g["head_list"]], mode=str(g["mode"]), seed=seed,
                        vit_cfg=dict(embed_dim=D, depth=depth, num_heads=heads, patch_size=patch))
    with torch.no_grad():
        feats, _ = om.feature_extractor(x, use_head=False, faithful=False)
    return x, y01, feats.detach().contiguous(), w0, b0


def _golden_tensors(g):
    x, y01, feats, w0, b0 = golden_inputs(g)
    labels = torch.from_numpy(g["labels"].astype(np.int64))
    return feats, w0, b0, labels, int(g["cfg"][3])


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def test_regenerated_inputs_are_the_references(golden):
    g = golden("linear_probe")
    x, y01, feats, w0, b0 = golden_inputs(g)
    assert np.array_equal(x[:, :, ::16, ::16].numpy(), g["x_sample"])
    assert _rel(feats[:, ::49], g["feats_sample"]) < 1e-6
    R = int(g["cfg"][3])
    assert torch.equal(L.prepare_labels(y01, R), torch.from_numpy(g["labels"].astype(np.int64)))


def test_restatement_reproduces_the_reference(golden):
    g = golden("linear_probe")
    feats, w, b, labels, R = _golden_tensors(g)
    assert 0.0 < float((labels == 255).float().mean()) < 0.5       # the fixture has ignored pixels, and not only those
    logits, loss, dw, db = restate_step(feats, w, b, labels, R)
    assert _rel(logits, g["logits"]) < 1e-5
    assert abs(float(loss) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    assert _rel(dw, g["dw"]) < 1e-5 and _rel(db, g["db"]) < 1e-5
    # three SGD steps with StepLR(1, 0.5), as the fixture
    wp, bp = nn.Parameter(w.clone()), nn.Parameter(b.clone())
    opt = torch.optim.SGD([wp, bp], lr=0.01, momentum=0.9, weight_decay=0.0001)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    for step in range(3):
        loss = F.cross_entropy(restate_logits(feats, wp, bp, R), labels, ignore_index=255)
        assert abs(loss.item() - float(g[f"loss_step{step}"])) <= 1e-5 * float(g[f"loss_step{step}"])
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
    assert _rel(wp.detach(), g["w3"]) < 1e-5 and _rel(bp.detach(), g["b3"]) < 1e-5
    assert _rel(opt.state[wp]["momentum_buffer"], g["mw3"]) < 1e-5


def test_label_preparation_matches_the_fixture(golden):
    g = golden("linear_probe")
    R = int(g["cfg"][3])
    labels = L.prepare_labels(golden_inputs(g)[1], R)
    assert labels.dtype == torch.int64 and labels.shape == (int(g["cfg"][0]), R, R)
    assert torch.equal(labels, torch.from_numpy(g["labels"].astype(np.int64)))
    # uint8 label / 255 * 255 -> .long() is exact for every byte value
    v = torch.arange(256, dtype=torch.uint8).float() / 255
    assert torch.equal((v * 255).long(), torch.arange(256))


def test_parser_defaults_are_the_reference_constants():
    a = L.build_parser().parse_args([])
    assert (a.architecture, a.model_path, a.head_layers, a.num_prototypes) == ("dino-s16", "dino-s16.pth", [1024, 1024, 512, 256], 200)
    assert (a.num_classes, a.mask_size, a.batch_size, a.epochs) == (21, 100, 60, 50)
    assert (a.lr, a.momentum, a.weight_decay, a.step_size, a.gamma) == (0.01, 0.9, 0.0001, 20, 0.1)
    assert a.input_resolution == 448


def test_other_datasets_are_not_built():
    with pytest.raises(NotImplementedError):
        L.main(["--dataset", "pascal"])


class _Backbone(nn.Module):
    def __init__(self, D):
        super().__init__()
        self.embed_dim = D
        self.w = nn.Parameter(torch.zeros(2))


class _Extractor(nn.Module):
    def __init__(self, D, head_dim=None):
        super().__init__()
        self.backbone = _Backbone(D)
        self.feature_dim = head_dim or D

    def forward(self, x, use_head=True):   # would be a launch: the checks must come first
        raise AssertionError("the model ran before the shapes were checked")


@pytest.mark.parametrize("D,C", [(6, 21), (1028, 21), (384, 0), (384, 257)])
def test_unsupported_shapes_raise_at_construction(D, C):
    with pytest.raises(ValueError):
        L.LinearFinetune(_Extractor(D), C, 100)


def test_mismatched_feature_width_raises_before_the_model_runs():
    m = L.LinearFinetune(_Extractor(384, head_dim=256), 21, 100)
    assert [p.requires_grad for p in m.model.parameters()] == [False]
    assert m.finetune_head.weight.shape == (21, 384, 1, 1)
    assert set(m.state_dict()) >= {"finetune_head.weight", "finetune_head.bias"}
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 64, 64), use_head=True)
    with pytest.raises(ValueError):
        m.loss(torch.zeros(1, 3, 64, 64), torch.zeros(1, 100, 100, dtype=torch.int64), use_head=True)


def test_wrappers_have_no_cpu_fallback():
    from timetuning_amd import hip_ops

    with pytest.raises(_lib.HipLibraryError):
        hip_ops.probe_logits(torch.zeros(8, 4), torch.zeros(2, 4), torch.zeros(2))
    with pytest.raises(_lib.HipLibraryError):
        hip_ops.probe_upsample_ce(torch.zeros(1, 4, 2), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(_lib.HipLibraryError):
        hip_ops.bilinear_adjoint_tokens(torch.zeros(1, 16, 2), 2)
    with pytest.raises(_lib.HipLibraryError):
        hip_ops.probe_wgrad(torch.zeros(8, 2), torch.zeros(8, 4))
    p = torch.zeros(4)
    with pytest.raises(_lib.HipLibraryError):
        hip_ops.sgd_step_([(p, p, None, 0.1, 0.0)])


def test_fused_sgd_keeps_the_sgd_surface():
    p = nn.Parameter(torch.zeros(3))
    opt = L.FusedSGD([p], lr=0.01, momentum=0.9, weight_decay=0.0001)
    ref = torch.optim.SGD([nn.Parameter(torch.zeros(3))], lr=0.01, momentum=0.9, weight_decay=0.0001)
    assert opt.state_dict()["param_groups"][0].keys() == ref.state_dict()["param_groups"][0].keys()
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    sched.step()
    assert opt.param_groups[0]["lr"] == pytest.approx(0.005)
    with pytest.raises(NotImplementedError):
        L.FusedSGD([p], lr=0.1, momentum=0.9, nesterov=True)
