"""DAVIS J&F on the GPU (N7): tt_davis_seg2bmap and the six counts of tt_davis_jf_counts equal to the numpy restatement
(test_davis_metrics_host.py) over shapes, radii, object counts, label dtypes and void; every J and F of the reference's own functions
(tests/golden/davis_metrics.npz) bit for bit; determinism; the element cap; the driver's --davis_metrics."""
import re

import numpy as np
import pytest
import torch

from _metric_refs import davis_np_counts as np_counts, np_seg2bmap
from test_davis_metrics_host import bits_equal, golden_labels
from timetuning_amd import _lib, hip_ops as ops
from timetuning_amd import mask_propagation as MP

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)


def _labels(rng, T, H, W, O, dtype):
    """Blobs of 1..O plus values outside 1..O (0, O + 1, and for int64 negatives and large ids)."""
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.zeros((T, H, W), np.int64)
    for t in range(T):
        for o in range(1, O + 3):
            cy, cx = rng.uniform(-0.2, 1.2) * H, rng.uniform(-0.2, 1.2) * W
            ry, rx = rng.uniform(0.1, 0.5) * H + 0.5, rng.uniform(0.1, 0.5) * W + 0.5
            lab[t][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = o
        noise = rng.random((H, W)) < 0.02
        lab[t][noise] = rng.integers(0, O + 2, int(noise.sum()))
    if dtype == np.int64:
        odd = rng.random(lab.shape) < 0.01
        lab[odd] = rng.choice([-1, -(O + 1), 1 << 40, 257], int(odd.sum()))
    return lab.astype(dtype)


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 77), (2, 77, 1), (3, 13, 29), (2, 65, 129), (1, 480, 854), (2, 3, 200)])
def test_seg2bmap_equals_restatement(shape):
    rng = np.random.default_rng(sum(shape))
    seg = (rng.random(shape) < 0.4).astype(np.uint8) * rng.integers(1, 4, shape).astype(np.uint8)   # any non-zero is set
    got = ops.davis_seg2bmap(torch.from_numpy(seg).to(dev)).cpu().numpy()
    want = np.stack([np_seg2bmap(s) for s in seg]).astype(np.uint8)
    assert np.array_equal(got, want)


CASES = [
    # T, H, W, O, radius, pred dtype, gt dtype, void
    (1, 1, 1, 1, 0, np.uint8, np.uint8, False),
    (2, 1, 1, 2, 3, np.int64, np.uint8, True),
    (2, 1, 150, 2, 2, np.uint8, np.int64, False),
    (2, 150, 1, 2, 2, np.int64, np.int64, True),
    (3, 17, 23, 3, 1, np.uint8, np.uint8, True),
    (2, 37, 61, 5, 4, np.int64, np.int64, False),
    (2, 64, 64, 8, 8, np.int64, np.uint8, True),
    (2, 33, 130, 4, 20, np.uint8, np.uint8, False),
    (2, 5, 7, 2, 10, np.int64, np.int64, True),          # the element is larger than the image
    (1, 99, 203, 3, 2.5, np.uint8, np.int64, True),      # even 6 x 6 element, off-centre anchor
    (1, 71, 300, 2, 63, np.uint8, np.uint8, False),      # the largest element, 127 x 127
    (1, 480, 854, 3, 8, np.uint8, np.uint8, True),
    (1, 480, 854, 3, 8, np.int64, np.int64, False),
]


@pytest.mark.parametrize("T,H,W,O,radius,pt,gtt,use_void", CASES)
def test_counts_equal_restatement(T, H, W, O, radius, pt, gtt, use_void):
    rng = np.random.default_rng(T * 1000003 + H * 1009 + W * 7 + O + int(radius * 10))
    gt = _labels(rng, T, H, W, O, gtt)
    pred = _labels(rng, T, H, W, O, pt)
    void = (rng.random((T, H, W)) < 0.05).astype(np.uint8) if use_void else None
    el = MP.disk(radius)
    got = ops.davis_jf_counts(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), O, el,
                              None if void is None else torch.from_numpy(void).to(dev)).cpu().numpy()
    want = np_counts(pred, gt, O, el, void)
    assert got.shape == (O, T, 6) and got.dtype == np.int64
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("name", ["small", "mid", "row", "col"])
def test_davis_jf_bit_equal_the_reference(golden, name):
    g = golden("davis_metrics")
    gt, pred, void, O = golden_labels(g, name)
    for vname, v in (("novoid", None), ("void", void)):
        for k, th in enumerate(g[f"{name}_bound_th"]):
            for conv in (lambda a: a, lambda a: torch.from_numpy(a.astype(np.int64)).to(dev)):   # numpy uint8, torch int64
                J, F = MP.davis_jf(conv(pred), conv(gt), O, void=v, bound_th=float(th))
                assert bits_equal(J, g[f"{name}_{vname}_J"]) and bits_equal(F, g[f"{name}_{vname}_F{k}"]), (vname, th)


def test_mirror_functions_bit_equal_the_reference(golden):
    g = golden("davis_metrics")
    gt, pred, void, O = golden_labels(g, "small")
    th = g["small_bound_th"]
    for o in range(1, O + 1):
        assert bits_equal(MP.db_eval_iou(gt == o, pred == o, void), g["small_void_J"][o - 1])
        assert bits_equal(MP.db_eval_iou(torch.from_numpy(gt == o), torch.from_numpy(pred == o)), g["small_novoid_J"][o - 1])
        for k in (0, 3):
            want = g[f"small_void_F{k}"][o - 1]
            assert bits_equal(MP.db_eval_boundary(gt == o, pred == o, void, bound_th=float(th[k])), want)
            assert bits_equal([MP.db_eval_boundary(gt[1] == o, pred[1] == o, void[1], bound_th=float(th[k]))], [want[1]])
            assert bits_equal([MP.f_measure(pred[2] == o, gt[2] == o, void[2], bound_th=float(th[k]))], [want[2]])
    gm, pm = g["empty_gt"], g["empty_pred"]
    z = np.zeros_like(gm)
    assert bits_equal([MP.db_eval_iou(gm, z), MP.db_eval_iou(z, pm), MP.db_eval_iou(z, z)], g["empty_J"])
    assert MP.db_eval_iou(z, z) == 1
    assert bits_equal([MP.f_measure(z, gm), MP.f_measure(pm, z), MP.f_measure(z, z)], g["empty_F"])
    for k in range(3):
        assert np.array_equal(MP._seg2bmap(g[f"bmap{k}_seg"]).astype(np.uint8), g[f"bmap{k}"])
        assert MP._seg2bmap(g[f"bmap{k}_seg"]).dtype == bool


def test_evaluate_semisupervised_pads_missing_objects(golden):
    g = golden("davis_metrics")
    T, H, W, seed = [int(v) for v in g["semi_cfg"]]
    gt, pred, void = MP.synthetic_davis_labels(T, H, W, 3, seed)
    gm = np.stack([gt == o for o in (1, 2, 3)]).astype(np.uint8)
    rm = np.stack([pred == o for o in (1, 2)]).astype(np.uint8)
    J, F = MP.evaluate_semisupervised(gm, rm, void, ("J", "F"))
    assert bits_equal(J, g["semi_J"]) and bits_equal(F, g["semi_F"])
    J2, F2 = MP.evaluate_semisupervised(torch.from_numpy(gm).to(dev), torch.from_numpy(rm).to(dev), torch.from_numpy(void).to(dev), ("J",))
    assert bits_equal(J2, g["semi_J"]) and not F2.any()


def test_two_runs_give_identical_bits():
    rng = np.random.default_rng(5)
    gt = torch.from_numpy(_labels(rng, 6, 480, 854, 3, np.uint8)).to(dev)
    pred = torch.from_numpy(_labels(rng, 6, 480, 854, 3, np.uint8)).to(dev)
    void = torch.from_numpy((rng.random((6, 480, 854)) < 0.02).astype(np.uint8)).to(dev)
    a = ops.davis_jf_counts(pred, gt, 3, MP.disk(8), void)
    b = ops.davis_jf_counts(pred, gt, 3, MP.disk(8), void)
    assert torch.equal(a, b)
    J1, F1 = MP.davis_jf(pred, gt, 3, void)
    J2, F2 = MP.davis_jf(pred, gt, 3, void)
    assert bits_equal(J1, J2) and bits_equal(F1, F2)


def test_element_cap_raises():
    m = torch.zeros((1, 32, 32), dtype=torch.uint8, device=dev)
    ops.davis_jf_counts(m, m, 1, MP.disk(63))                     # 127 x 127: the cap
    with pytest.raises(_lib.HipLibraryError, match="structuring element"):
        ops.davis_jf_counts(m, m, 1, MP.disk(64))                 # 129 x 129
    with pytest.raises(_lib.HipLibraryError):
        MP.davis_jf(m, m, 1, bound_th=64)
    with pytest.raises(TypeError):
        ops.davis_jf_counts(m.int(), m, 1, MP.disk(1))


def _driver_args(*extra):
    return MP.build_parser().parse_args(["--dataset", "synthetic", "--model_path", "", "--num_frames", "5", "--num_clips", "2", *extra])


@pytest.mark.parametrize("uvos", ["1", "0"])
def test_driver_davis_metrics_are_one_when_the_prediction_is_the_gt(monkeypatch, capsys, uvos):
    monkeypatch.setattr(MP, "propagate_clip", lambda model, clip, first, *a, **k: torch.from_numpy(
        _current_masks["m"][1:].numpy()).to(clip.device))
    real = MP.synthetic_tracking_clip

    def clip_and_remember(fs, R, seed, objects=2):
        c, m = real(fs, R, seed, objects)
        _current_masks["m"] = (m > 0).long() if uvos == "1" else m
        return c, m

    monkeypatch.setattr(MP, "synthetic_tracking_clip", clip_and_remember)
    MP.mask_propagation(_driver_args("--davis_metrics", "--uvos", uvos))
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if "J&F-Mean" in ln]
    assert len(lines) == 3, out   # two clips and the overall line
    for ln in lines:
        vals = dict(re.findall(r"(J&F-Mean|J_M|J_R|F_M|F_R|J_D|F_D) (-?[0-9.]+)", ln))
        assert float(vals["J&F-Mean"]) == 1.0 and float(vals["J_M"]) == 1.0 and float(vals["F_M"]) == 1.0
        assert float(vals["J_R"]) == 1.0 and float(vals["F_R"]) == 1.0 and float(vals["J_D"]) == 0.0 and float(vals["F_D"]) == 0.0


_current_masks = {}


def test_driver_davis_metrics_finite_and_default_output_unchanged(capsys):
    j_default = MP.mask_propagation(_driver_args())
    default_out = capsys.readouterr().out
    assert "J&F" not in default_out
    j_davis = MP.mask_propagation(_driver_args("--davis_metrics", "--uvos", "0"))
    out = capsys.readouterr().out
    overall = [ln for ln in out.splitlines() if ln.startswith("DAVIS over")]
    assert len(overall) == 1
    assert all(np.isfinite(float(v)) for v in re.findall(r"(?:J&F-Mean|J_M|J_R|J_D|F_M|F_R|F_D) (-?[0-9.]+|nan)", overall[0]))
    assert np.isfinite(j_default) and np.isfinite(j_davis)
