"""The FCN head's norm layers without a GPU (N33): the fixture against the fp64 restatement that wrote it, the state-dict layout of
``FCNHead(norm_cfg=...)`` and its interchange with a twin of ``nn.Conv2d`` / ``nn.BatchNorm2d``, the refusals of ``norm_cfg``, the
driver's ``--norm`` and the five C entries' declarations."""
import os
import re

import numpy as np
import pytest
import torch

import _fcn_bn_ref as RB
import _fcn_ref as R
from timetuning_amd import _lib, fcn_finetune, leopart

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tt_bn_tokens_fwd", "tt_bn_tokens_fwd_workspace_bytes", "tt_bn_tokens_bwd", "tt_bn_tokens_bwd_workspace_bytes", "tt_bn_tokens_shape_ok")


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_fixture_is_what_the_restatement_computes(golden):
    g = golden("fcn_head_bn")
    want = RB.fixture_arrays()
    assert sorted(g.files) == sorted(want)
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "fcn_head_bn.npz")) < 100_000
    for k, v in want.items():
        assert g[k].dtype == v.dtype and g[k].shape == np.shape(v), k
        if k.startswith(("grad.", "logits", "loss", "after.")):
            # fp64 results rounded to fp32: equal up to that rounding whatever the CPU's summation order
            scale = np.abs(np.asarray(v, np.float64)).max()
            assert np.abs(g[k].astype(np.float64) - np.asarray(v, np.float64)).max() <= 2.0 ** -22 * scale, k
        else:
            assert np.array_equal(g[k], v), k
    c = RB.FIXTURE
    assert np.isfinite(g["loss"]) and float(g["loss"]) > 0
    assert np.array_equal(g["feats"], R.fixture_inputs()[0].numpy())            # the N32 fixture's inputs
    keys = RB.param_keys(c["num_convs"], c["concat_input"])
    assert sorted("grad." + k for k in keys) == sorted(k for k in g.files if k.startswith("grad."))
    for k in keys:
        assert np.abs(g["grad." + k]).max() > 0, k
    assert (g["state.convs.0.bn.weight"] < 0).any()
    for k in g.files:
        if k.startswith("after."):
            assert not np.array_equal(g[k], g["state." + k[len("after."):]]), k   # a training forward moved every running buffer


@pytest.mark.parametrize("norm", [None, "BN"])
@pytest.mark.parametrize("concat_input", [True, False])
@pytest.mark.parametrize("num_convs", [0, 1, 2, 3])
def test_state_dict_keys_and_shapes(num_convs, concat_input, norm):
    D = 8 if num_convs == 0 else 16
    head = leopart.FCNHead(D, 8, num_classes=5, num_convs=num_convs, concat_input=concat_input,
                           norm_cfg=None if norm is None else dict(type=norm, requires_grad=True))
    sd = head.state_dict()
    if norm is None:
        assert list(sd) == R.head_keys(num_convs, concat_input)
        assert {k: tuple(v.shape) for k, v in sd.items()} == R.head_shapes(D, 8, 5, num_convs, concat_input)
        assert head.head_norm() is None
        return
    want = RB.head_shapes(D, 8, 5, num_convs, concat_input)
    assert list(sd) == RB.head_keys(num_convs, concat_input)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert not any(k.endswith("conv.bias") for k in sd)                         # bias='auto': none with a norm layer
    names = [k for k, _ in head.named_parameters()]
    assert [tuple(p.shape) for p in head.parameter_list()] == [want[k] for k in RB.param_keys(num_convs, concat_input)]
    assert sorted(names) == sorted(RB.param_keys(num_convs, concat_input))
    for m in RB.module_names(num_convs, concat_input):
        assert bool((sd[f"{m}.bn.weight"] == 1).all()) and not float(sd[f"{m}.bn.bias"].abs().max())
        assert not float(sd[f"{m}.bn.running_mean"].abs().max()) and bool((sd[f"{m}.bn.running_var"] == 1).all())
        assert int(sd[f"{m}.bn.num_batches_tracked"]) == 0 and float(sd[f"{m}.conv.weight"].abs().max()) > 0
    assert len(head.head_norm().bns) == len(RB.module_names(num_convs, concat_input)) and head.head_norm().training
    assert not head.eval().head_norm().training


@pytest.mark.parametrize("num_convs,concat_input", [(2, True), (1, False), (0, True)])
def test_state_dicts_interchange_with_the_twin(num_convs, concat_input):
    D = 8 if num_convs == 0 else 16
    state = RB.head_state("fcn.bn.sd", D, 8, 5, num_convs, concat_input)
    head = leopart.FCNHead(D, 8, num_classes=5, num_convs=num_convs, concat_input=concat_input, norm_cfg=dict(type="SyncBN", requires_grad=True))
    twin = RB.TwinHead(D, 8, 5, num_convs, concat_input)
    assert list(head.state_dict()) == list(twin.state_dict())
    twin.load_state_dict(state, strict=True)
    head.load_state_dict(twin.state_dict(), strict=True)
    for k, v in head.state_dict().items():
        assert torch.equal(v, state[k]), k
    fresh = RB.TwinHead(D, 8, 5, num_convs, concat_input)
    fresh.load_state_dict(head.state_dict(), strict=True)
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, state[k]), k
    with pytest.raises(RuntimeError):                                            # a head without norm layers has other keys
        leopart.FCNHead(D, 8, num_classes=5, num_convs=num_convs, concat_input=concat_input).load_state_dict(state, strict=True)


def test_norm_cfg_arguments():
    head = leopart.FCNHead(16, 8, num_classes=5, norm_cfg=dict(type="BN", requires_grad=False, eps=1e-3, momentum=0.25))
    for m in list(head.convs) + [head.conv_cat]:
        assert m.bn.eps == 1e-3 and m.bn.momentum == 0.25
        assert not m.bn.weight.requires_grad and not m.bn.bias.requires_grad and m.conv.weight.requires_grad
    head = leopart.FCNHead(16, 8, num_classes=5, norm_cfg=dict(type="BN"))
    assert head.convs[0].bn.eps == 1e-5 and head.convs[0].bn.momentum == 0.1 and head.convs[0].bn.weight.requires_grad
    # no ConvModule: norm_cfg changes nothing
    plain = leopart.FCNHead(8, 8, num_classes=5, num_convs=0, concat_input=False, norm_cfg=dict(type="BN"))
    assert list(plain.state_dict()) == ["conv_seg.weight", "conv_seg.bias"] and len(plain.parameter_list()) == 2


def test_norm_cfg_refusals():
    for cfg in (dict(type="GN", num_groups=4), dict(type="LN"), dict(type="BN", momentum=None), dict(requires_grad=True), "BN",
                dict(type="BN", eps=0.0), dict(type="BN", momentum=1.5), dict(type="BN", affine=False)):
        with pytest.raises(ValueError):
            leopart.FCNHead(16, 8, num_classes=5, norm_cfg=cfg)


def test_syncbn_over_several_ranks_is_refused(monkeypatch):
    import torch.distributed as dist

    leopart.FCNHead(16, 8, num_classes=5, norm_cfg=dict(type="SyncBN"))          # one process: the statistics are complete
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(ValueError):
        leopart.FCNHead(16, 8, num_classes=5, norm_cfg=dict(type="SyncBN"))
    leopart.FCNHead(16, 8, num_classes=5, norm_cfg=dict(type="BN"))
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 1)
    leopart.FCNHead(16, 8, num_classes=5, norm_cfg=dict(type="SyncBN"))


def test_parser_has_norm():
    p = fcn_finetune.build_parser()
    assert p.parse_args([]).norm == "none" and p.parse_args(["--norm", "bn"]).norm == "bn"
    with pytest.raises(SystemExit):
        p.parse_args(["--norm", "gn"])


def test_new_symbols_are_declared_bound_and_exported(lib):
    text = open(os.path.join(REPO, "include", "timetuning_hip.h")).read()
    declared = set(re.findall(r"\b(tt_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.tt_abi_version() == 8                                             # additive
    assert f"{len(declared)} entry points" in open(os.path.join(REPO, "README.md")).read()
    assert "bn_tokens.hip" in open(os.path.join(REPO, "timetuning_amd", "csrc", "Makefile")).read()
    # the shape rule and the workspace queries are host code
    assert lib.tt_bn_tokens_shape_ok(588, 132, 1) == 1 and lib.tt_bn_tokens_shape_ok(1, 4, 0) == 1
    for rows, C, training in [(1, 4, 1), (0, 4, 0), (8, 6, 1), (8, 1028, 1), (8, 0, 1), (1 << 31, 4, 1)]:
        assert lib.tt_bn_tokens_shape_ok(rows, C, training) == 0, (rows, C, training)
    for rows, C in [(2, 4), (63, 60), (588, 132), (47040, 512), ((1 << 31) - 1, 1024)]:
        nb = lib.tt_bn_tokens_fwd_workspace_bytes(rows, C)
        assert nb == lib.tt_bn_tokens_bwd_workspace_bytes(rows, C) and nb % (16 * C) == 0 and 0 < nb <= 192 * 16 * C, (rows, C, nb)
    assert lib.tt_bn_tokens_fwd_workspace_bytes(0, 4) == 0 and lib.tt_bn_tokens_fwd_workspace_bytes(8, 0) == 0
    # refusals that need no device: nothing is launched
    assert lib.tt_bn_tokens_fwd(None, None, None, None, None, None, None, None, None, 8, 8, 4, 1, 1, 0.1, 1e-5, None, 0, None) != 0
    assert b"bn_tokens_fwd" in lib.tt_last_error()
    assert lib.tt_bn_tokens_bwd(None, None, None, None, None, None, None, None, 8, 4, None, 0, None) != 0
    assert b"bn_tokens_bwd" in lib.tt_last_error()
