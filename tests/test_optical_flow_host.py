"""CPU checks of N10, the optical-flow baseline (mask_propagation.py:265-346, :803-815): the fp64 restatement of OpenCV's Farneback flow
(tests/_farneback.py, standing in for cv2) on known translations, the pyramid plan and the workspace query of the library (host-only
functions), the parameter rules, the uint8 cast, the remap's rounding and border, and the --use_optical_flow route with the GPU
stubbed."""
import os
import sys

import numpy as np
import pytest
import torch

from timetuning_amd import _lib
from timetuning_amd import hip_ops as ops
from timetuning_amd import mask_propagation as MP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _farneback as FB  # noqa: E402


def smooth_texture(H, W, shift=(0.0, 0.0), seed=0):
    """A sum of 12 random plane waves (periods >= ~21 px), 8-bit, unclipped, moved by shift = (dx, dy) pixels."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    yy, xx = yy - shift[1], xx - shift[0]
    v = np.zeros((H, W))
    for _ in range(12):
        fy, fx = rng.uniform(-0.3, 0.3, 2)
        v += np.sin(fy * yy + fx * xx + rng.uniform(0, 2 * np.pi))
    return np.clip(128 + 25 * v / np.sqrt(6), 0, 255).astype(np.uint8)


def _lib_loaded():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.mark.parametrize("H,W,shift", [(96, 128, (1.3, -0.7)), (120, 100, (-0.4, 2.2))])
def test_restatement_recovers_translation(H, W, shift):
    # prev(x) = next(x + shift): the flow is the shift.  The interior (32 px from every edge) holds the mean within 0.1 px per
    # component and 90 % of the pixels within 0.25 px (measured: mean errors <= 0.05, 90th percentile <= 0.12).
    a, b = smooth_texture(H, W), smooth_texture(H, W, shift)
    f = FB.farneback(a, b)[32:-32, 32:-32]
    err = np.abs(f - np.array(shift))
    assert np.all(np.abs(f.reshape(-1, 2).mean(0) - shift) < 0.1)
    assert np.quantile(err.max(-1), 0.9) < 0.25


def test_restatement_identical_frames():
    # constant frames: exactly zero.  Textured identical frames: OpenCV treats the last row and column as outside the frame, which seeds
    # a small flow at the bottom / right edges that the pyramid and the box spread; 32 px in, it is below 1e-6.
    c = np.full((64, 80), 77, np.uint8)
    assert np.array_equal(FB.farneback(c, c), np.zeros((64, 80, 2)))
    a = smooth_texture(128, 128)
    assert np.abs(FB.farneback(a, a)[32:-32, 32:-32]).max() < 1e-6


@pytest.mark.parametrize("H,W", [(224, 224), (480, 854), (97, 131), (33, 1000), (63, 64), (31, 200), (20, 50), (1, 1), (1000, 7)])
@pytest.mark.parametrize("pyr_scale,levels", [(0.5, 3), (0.5, 5), (0.8, 3), (0.3, 10), (0.5, 1)])
def test_plan_matches_restatement(H, W, pyr_scale, levels):
    _lib_loaded()
    assert ops.farneback_plan(H, W, pyr_scale, levels) == FB.plan(H, W, pyr_scale, levels)


def test_plan_known_sizes():
    assert FB.plan(224, 224) == (2, [(224, 224), (112, 112), (56, 56)])
    assert FB.plan(480, 854) == (3, [(480, 854), (240, 427), (120, 214), (60, 107)])   # 213.5 -> 214, 106.75 -> 107
    assert FB.plan(40, 40) == (0, [(40, 40)])


def test_workspace_query():
    lib = _lib_loaded()
    al = lambda b: (b + 255) // 256 * 256   # noqa: E731
    F, P, H, W = 50, 49, 480, 854
    HW = H * W
    expect = al(4 * HW * F) * 2 + al(12 * HW * F) + al(20 * HW * F) + 2 * al(20 * HW * P) + 2 * al(8 * 240 * 427 * P)
    assert lib.tt_farneback_workspace_bytes(F, P, H, W, 0.5, 3) == expect
    assert lib.tt_farneback_workspace_bytes(2, 1, 20, 50, 0.5, 3) == al(4 * 1000 * 2) * 2 + al(12 * 2000) + al(20 * 2000) + 2 * al(20 * 1000)
    for bad in ((0, 1, 64, 64, 0.5, 3), (2, -1, 64, 64, 0.5, 3), (2, 1, 0, 64, 0.5, 3), (2, 1, 64, 64, 1.0, 3), (2, 1, 64, 64, 0.0, 3),
                (2, 1, 64, 64, 0.5, 0)):
        assert lib.tt_farneback_workspace_bytes(*bad) == 0


@pytest.mark.parametrize("kw,exc", [({"flags": 256}, NotImplementedError), ({"flags": 4}, NotImplementedError), ({"flags": 1}, ValueError),
                                    ({"poly_n": 6}, ValueError), ({"poly_n": 3}, ValueError), ({"pyr_scale": 1.0}, ValueError),
                                    ({"pyr_scale": 0.0}, ValueError), ({"winsize": 0}, ValueError), ({"winsize": 128}, ValueError),
                                    ({"winsize": 15.0}, ValueError), ({"iterations": 0}, ValueError), ({"levels": 0}, ValueError),
                                    ({"levels": True}, ValueError), ({"poly_sigma": 0.0}, ValueError), ({"poly_sigma": float("nan")}, ValueError)])
def test_parameter_rules(kw, exc):
    a = np.zeros((40, 40), np.uint8)
    with pytest.raises(exc):
        MP.calc_optical_flow_farneback(a, a, **kw)       # raises before any GPU work
    args = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2, flags=0)
    args.update(kw)
    with pytest.raises(exc):
        FB.check_params(**args)


def test_parameter_rules_accept_the_reference_call():
    ops.check_farneback_params(0.5, 3, 15, 3, 5, 1.2, 0)
    ops.check_farneback_params(0.25, 1, 1, 1, 7, 1.5, 0)
    ops.check_farneback_params(0.5, 3, 127, 3, 5, 1, 0)


def test_u8_cast_matches_torch():
    v = np.concatenate([np.linspace(-3, 3, 20011, dtype=np.float32), np.array([-1.7, 2.5, -0.5, 1.0, 0.999, -300.2, 1e4], np.float32)])
    x = torch.from_numpy(v) * 255
    assert np.array_equal(FB.u8_cast(x.numpy()), x.type(torch.uint8).numpy())
    assert FB.u8_cast(np.float32([-1.7 * 255]))[0] == 79 and FB.u8_cast(np.float32([2.5]) * np.float32(255))[0] == 125


def test_gray_formula():
    clip = np.random.default_rng(3).normal(size=(2, 3, 5, 7)).astype(np.float32)
    v = (torch.from_numpy(clip) * 255).type(torch.uint8).numpy().astype(np.int64)
    expect = (v[:, 0] * 4899 + v[:, 1] * 9617 + v[:, 2] * 1868 + 8192) >> 14
    assert np.array_equal(FB.gray_u8(clip), expect.astype(np.uint8))


def test_remap_ties_and_border():
    lab = np.arange(1, 31, dtype=np.int64).reshape(5, 6)
    fl = np.zeros((5, 6, 2), np.float32)
    fl[..., 0] = 0.5     # x + 0.5 rounds to the even neighbour
    out = FB.remap_nearest(lab, fl)
    xs = np.rint(np.arange(6) + 0.5).astype(int)
    for x in range(6):
        assert np.array_equal(out[:, x], lab[:, xs[x]] if xs[x] < 6 else np.zeros(5, np.int64))
    fl[..., 0] = -0.5    # x - 0.5: 0 -> -0 (inside), 1 -> 0, 3 -> 2
    out = FB.remap_nearest(lab, fl)
    assert np.array_equal(out[:, 0], lab[:, 0]) and np.array_equal(out[:, 1], lab[:, 0]) and np.array_equal(out[:, 3], lab[:, 2])
    fl[...] = 0
    fl[..., 1] = -1.6    # two rows up: out of the frame for rows 0 and 1
    out = FB.remap_nearest(lab, fl)
    assert np.all(out[:2] == 0) and np.array_equal(out[2:], lab[:3])
    assert np.all(FB.remap_nearest(lab, np.full((5, 6, 2), np.nan, np.float32)) == 0)
    # interpolate_frames' scale: (f + 1) / n_frames rounded to float32, then one multiply and one add in float32
    fl = np.zeros((5, 6, 2), np.float32)
    fl[..., 0] = 1.0
    assert np.array_equal(FB.remap_nearest(lab, fl, 0.5), FB.remap_nearest(lab, fl * 0.5))


def test_propagate_chain_restatement():
    lab = np.zeros((6, 8), np.uint8)
    lab[2:4, 2:4] = 1
    step = np.zeros((6, 8, 2), np.float32)
    step[..., 0] = -1.0    # label_{j+1}(x) = label_j(x - 1): the object moves right by one pixel per step
    out = FB.propagate_chain(lab, [step] * 3)
    for j in range(3):
        assert np.array_equal(out[j], np.roll(lab, j + 1, 1))


def test_use_optical_flow_routes_to_the_flow_body(monkeypatch, capsys):
    calls = []

    def body(clip, first):
        calls.append((tuple(clip.shape), tuple(first.shape)))
        return torch.zeros((clip.shape[0] - 1, *clip.shape[2:]), dtype=torch.int64)

    monkeypatch.setattr(MP, "propagate_clip_optical_flow", body)
    monkeypatch.setattr(MP, "propagate_clip", lambda *a, **k: pytest.fail("the feature branch ran"))
    monkeypatch.setattr(MP, "jaccard", lambda pred, gt, C: (0.25, None))
    monkeypatch.setattr(MP, "_device_tensor", lambda x: x)
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)
    args = MP.build_parser().parse_args(["--dataset", "synthetic", "--use_optical_flow", "True", "--num_clips", "2", "--num_frames", "4",
                                         "--input_resolution", "64", "--model_path", "/nonexistent"])
    assert args.use_optical_flow is True
    assert MP.mask_propagation(args) == 0.25
    assert calls == [((4, 3, 64, 64), (64, 64))] * 2
    args = MP.build_parser().parse_args(["--dataset", "synthetic", "--use_optical_flow", "True", "--num_clips", "1", "--num_frames", "3",
                                         "--frame_size", "48", "80"])
    calls.clear()
    MP.mask_propagation(args)
    assert calls == [((3, 3, 48, 80), (48, 80))]
    with pytest.raises(ValueError):
        MP.mask_propagation(MP.build_parser().parse_args(["--dataset", "synthetic", "--use_optical_flow", "True", "--frame_size", "48", "81"]))


def test_use_optical_flow_default_is_the_feature_branch():
    assert MP.build_parser().parse_args([]).use_optical_flow is False
