"""CPU checks of the DAVIS J&F surface (N7, ``timetuning_amd.mask_propagation``).

The fixture tests/golden/davis_metrics.npz comes from the reference's own functions (tools/gen_davis_metrics_golden.py).  Here: the
stand-ins the generator used give the published answers, the inputs regenerate, a numpy restatement of the six counts turned into J
and F by the product's host code reproduces every fixture value to the bit, ``db_statistics`` matches, and the driver flag exists.
The kernel is checked against the same restatement on the GPU (test_hip_davis_metrics.py)."""
import importlib.util
import os

import numpy as np
import pytest

from _metric_refs import davis_np_counts as np_counts, np_dilate, np_seg2bmap
from timetuning_amd import hip_ops
from timetuning_amd import mask_propagation as MP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location("gen_davis_metrics_golden", os.path.join(REPO, "tools", "gen_davis_metrics_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- numpy restatement of tt_davis_jf_counts: tests/_metric_refs.py (shared with the sweep's fifth tier) -------------------

def golden_labels(g, name):
    T, H, W, O, seed = [int(v) for v in g[f"{name}_cfg"]]
    gt, pred, void = MP.synthetic_davis_labels(T, H, W, O, seed)
    return gt, pred, void, O


def bits_equal(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- stand-ins and element ---------------------------------------------------------------------------------------------

def test_disk_stand_in_and_product_disk_known_answers():
    gen = _generator()
    d1 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8)
    d2 = np.array([[0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [1, 1, 1, 1, 1], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0]], np.uint8)
    d25 = np.zeros((6, 6), np.uint8)
    d25[1:5, 1:5] = 1      # grid -2.5..2.5: the corners (+-0.5, +-2.5) lie outside r = 2.5, the outer ring is empty
    for disk in (gen.disk_standin, MP.disk):
        assert np.array_equal(disk(1), d1) and np.array_equal(disk(2), d2) and np.array_equal(disk(2.5), d25)
        assert np.array_equal(disk(0), np.ones((1, 1), np.uint8))
        assert disk(8.0).shape == (17, 17) and disk(8.0).sum() == 197
    spans, shape, anchor = hip_ops.davis_element_spans(MP.disk(2.5))
    assert shape == (6, 6) and anchor == (3, 3)     # cv2's default anchor: off centre for an even size
    assert spans == [(1, 0), (1, 4), (1, 4), (1, 4), (1, 4), (1, 0)]
    assert hip_ops.davis_element_spans(MP.disk(1))[0] == [(1, 1), (0, 2), (1, 1)]
    with pytest.raises(ValueError):
        hip_ops.davis_element_spans(np.array([[1, 0, 1]]))


def test_dilate_stand_in_single_pixel_by_the_asymmetric_element():
    gen = _generator()
    el = MP.disk(2.5)                       # set rows / columns 1..4, anchor (3, 3): offsets -2..1
    src = np.zeros((9, 11), np.uint8)
    src[4, 5] = 1
    want = np.zeros_like(src)
    want[3:7, 4:8] = 1                      # dst(y, x) = src(y + i - 3, x + j - 3): y - 4 in -1..2 -> rows 3..6, columns 4..7
    assert np.array_equal(gen.dilate_standin(src, el), want)
    assert np.array_equal(np_dilate(src, el), want.astype(bool))
    edge = np.zeros((4, 4), np.uint8)
    edge[0, 0] = 1                          # outside the image contributes nothing
    w2 = np.zeros_like(edge)
    w2[0:3, 0:3] = 1
    assert np.array_equal(gen.dilate_standin(edge, el), w2) and np.array_equal(np_dilate(edge, el), w2.astype(bool))


def test_seg2bmap_restatement_equals_the_reference(golden):
    g = golden("davis_metrics")
    for k in range(3):
        assert np.array_equal(np_seg2bmap(g[f"bmap{k}_seg"]).astype(np.uint8), g[f"bmap{k}"])


def test_seg2bmap_rescale_is_not_built():
    with pytest.raises(NotImplementedError):
        MP._seg2bmap(np.zeros((4, 6), np.uint8), width=3, height=2)


# ---- the fixture --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["small", "mid", "row", "col"])
def test_regenerated_inputs_are_the_references(golden, name):
    g = golden("davis_metrics")
    gt, pred, void, _ = golden_labels(g, name)
    assert np.array_equal(gt[:, ::7, ::11], g[f"{name}_gt_sample"])
    assert np.array_equal(pred[:, ::7, ::11], g[f"{name}_pred_sample"])
    assert np.array_equal(void[:, ::7, ::11], g[f"{name}_void_sample"])


@pytest.mark.parametrize("name", ["small", "row", "col"])
def test_host_j_and_f_from_restated_counts_bit_equal_the_reference(golden, name):
    """The product's host formation of J and F (_j_table / _f_table, with the void handling folded into the counts) on counts
    from the numpy restatement: every fixture value, bit for bit."""
    g = golden("davis_metrics")
    gt, pred, void, O = golden_labels(g, name)
    H, W = gt.shape[1:]
    for vname, v in (("novoid", None), ("void", void)):
        for k, th in enumerate(g[f"{name}_bound_th"]):
            counts = np_counts(pred, gt, O, MP.disk(MP._bound_pix(float(th), (H, W))), v)
            if k == 0:
                assert bits_equal(MP._j_table(counts), g[f"{name}_{vname}_J"])
            assert bits_equal(MP._f_table(counts), g[f"{name}_{vname}_F{k}"]), (vname, th)


def test_empty_masks_branches(golden):
    g = golden("davis_metrics")
    gm, pm = g["empty_gt"], g["empty_pred"]
    z = np.zeros_like(gm)
    el = MP.disk(MP._bound_pix(0.008, gm.shape))
    js, fs = [], []
    for gt, pred in ((gm, z), (z, pm), (z, z)):   # (annotation, segmentation)
        c = np_counts(pred[None], gt[None], 1, el)[0, 0]
        js.append(1 if c[1] == 0 else c[0] / c[1])
        fs.append(MP._f_from_counts(c[2], c[3], c[4], c[5]))
    assert bits_equal(js, g["empty_J"]) and bits_equal(fs, g["empty_F"])
    assert fs == [0, 0, 1] and js[2] == 1


@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 300])
def test_db_statistics_bit_equal_the_reference(golden, n):
    g = golden("davis_metrics")
    got = MP.db_statistics(g[f"stats{n}_values"])
    assert bits_equal(got, g[f"stats{n}"])
    if n == 300:
        assert np.isnan(got[2])     # the uint8 quarter boundaries wrap round past 255 frames: the last quarter is empty


def test_more_predicted_objects_than_gt_exits():
    gt = np.zeros((1, 2, 4, 4), np.uint8)
    res = np.zeros((2, 2, 4, 4), np.uint8)
    with pytest.raises(SystemExit):
        MP.evaluate_semisupervised(gt, res, None, ("J", "F"))


def test_semisupervised_padding_restated(golden):
    """The missing predicted object is scored as an empty mask: J 0 where its GT is non-empty, F from the empty-prediction branch."""
    g = golden("davis_metrics")
    T, H, W, seed = [int(v) for v in g["semi_cfg"]]
    gt, pred, void = MP.synthetic_davis_labels(T, H, W, 3, seed)
    pred = np.where(pred == 3, 0, pred)       # only objects 1 and 2 predicted
    counts = np_counts(pred, gt, 3, MP.disk(MP._bound_pix(0.008, (H, W))), void)
    assert bits_equal(MP._j_table(counts), g["semi_J"]) and bits_equal(MP._f_table(counts), g["semi_F"])


def test_parser_flag_present_and_off_by_default():
    p = MP.build_parser()
    assert p.parse_args([]).davis_metrics is False
    assert p.parse_args(["--davis_metrics"]).davis_metrics is True
