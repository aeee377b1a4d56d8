"""FCN-head fine-tuning without a GPU (N32): the fixture against the fp64 restatement that wrote it, the state-dict layout of
``FCNHead``, its refusals and the driver's parser."""
import os

import numpy as np
import pytest
import torch

import _fcn_ref as R
from timetuning_amd import fcn_finetune, leopart, linear_finetune


def test_fixture_is_what_the_restatement_computes(golden):
    g = golden("fcn_head")
    want = R.fixture_arrays()
    assert sorted(g.files) == sorted(want)
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "fcn_head.npz")) < 100_000
    for k, v in want.items():
        assert g[k].dtype == v.dtype and g[k].shape == np.shape(v), k
        if k.startswith(("grad.", "logits", "loss")):
            # fp64 results rounded to fp32: equal up to that rounding whatever the CPU's summation order
            scale = np.abs(np.asarray(v, np.float64)).max()
            assert np.abs(g[k].astype(np.float64) - np.asarray(v, np.float64)).max() <= 2.0 ** -22 * scale, k
        else:
            assert np.array_equal(g[k], v), k
    assert np.isfinite(g["loss"]) and float(g["loss"]) > 0
    c = R.FIXTURE
    assert g["feats"].shape == (c["B"], c["g"] ** 2, c["D"]) and g["labels"].shape == (c["B"], c["R"], c["R"])
    assert (g["labels"] == 255).any() and (g["out_scale"] == 0).any() and (g["out_scale"] > 1).any()
    for k in R.head_keys(c["num_convs"], c["concat_input"]):
        assert np.abs(g["grad." + k]).max() > 0, k


@pytest.mark.parametrize("concat_input", [True, False])
@pytest.mark.parametrize("num_convs", [0, 1, 2, 3])
def test_state_dict_keys_and_shapes(num_convs, concat_input):
    D = 8 if num_convs == 0 else 16
    head = leopart.FCNHead(D, 8, num_classes=5, num_convs=num_convs, concat_input=concat_input)
    sd = head.state_dict()
    want = R.head_shapes(D, 8, 5, num_convs, concat_input)
    assert list(sd) == R.head_keys(num_convs, concat_input)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert [tuple(p.shape) for p in head.parameter_list()] == [want[k] for k in R.head_keys(num_convs, concat_input)]
    assert all(float(v.abs().max()) == 0 for k, v in sd.items() if k.endswith("bias"))
    assert float(sd["conv_seg.weight"].abs().max()) < 0.1   # normal(0, 0.01)


def test_refusals():
    with pytest.raises(ValueError):
        leopart.FCNHead(16, 8, num_classes=5, kernel_size=5)
    with pytest.raises(AssertionError):
        leopart.FCNHead(16, 8, num_classes=5, num_convs=0)
    with pytest.raises(ValueError):
        leopart.FCNHead(16, 10, num_classes=5)
    with pytest.raises(ValueError):
        leopart.FCNHead(18, 8, num_classes=5)
    with pytest.raises(ValueError):
        leopart.FCNHead(16, 2048, num_classes=5)


def test_parser_defaults():
    a = fcn_finetune.build_parser().parse_args([])
    assert (a.channels, a.num_convs, a.concat_input, a.dropout_ratio) == (512, 2, True, 0.1)
    assert fcn_finetune.build_parser().parse_args(["--no-concat_input"]).concat_input is False
    base = vars(linear_finetune.build_parser().parse_args([]))
    mine = vars(a)
    assert {k: mine[k] for k in base if k != "save_path"} == {k: v for k, v in base.items() if k != "save_path"}
    assert mine["save_path"] == "fcn_finetune.pth" and base["save_path"] == "linear_finetune.pth"
    assert fcn_finetune.validate is linear_finetune.validate and fcn_finetune.FusedSGD is linear_finetune.FusedSGD
