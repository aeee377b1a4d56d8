"""Boundary F-score on the GPU (N8): the four counts of tt_bf_counts equal the numpy restatement (test_bfscore_host.py) over shapes,
thresholds and densities, all 256 neighbourhoods included; every score of the reference's own bfscore.py (tests/golden/bfscore.npz)
bit for bit through bfscore / evaluate_bf_score; determinism; the element cap; the CBFE driver's --bf_score."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import _border_follow as bfl
from _metric_refs import bf_np_counts as np_counts
from test_bfscore_host import _generator, bits_equal, np_bfscore, np_image_scores
from timetuning_amd import _lib, hip_ops as ops
from timetuning_amd import bfscore as BF
from timetuning_amd import cluster_based_foreground_extraction as CB

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)


def _maps(rng, P, H, W, density):
    if density == "checker":
        yy, xx = np.mgrid[0:H, 0:W]
        a = np.broadcast_to(((yy + xx) % 2).astype(np.uint8), (P, H, W)).copy()
        return a, 1 - a
    if density == "blobs":
        out = []
        for _ in range(2):
            yy, xx = np.mgrid[0:H, 0:W]
            m = np.zeros((P, H, W), np.uint8)
            for k in range(P):
                for _ in range(3):
                    cy, cx = rng.uniform(0, H), rng.uniform(0, W)
                    ry, rx = rng.uniform(0.1, 0.4) * H + 0.5, rng.uniform(0.1, 0.4) * W + 0.5
                    m[k][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = 1
                m[k] ^= (rng.random((H, W)) < 0.01).astype(np.uint8)
            out.append(m)
        return out[0], out[1] * rng.integers(1, 256, (P, H, W)).astype(np.uint8) * out[1]   # any non-zero value is set
    return tuple((rng.random((P, H, W)) < density).astype(np.uint8) for _ in range(2))


def _run(gt, pr, t):
    return ops.bf_counts(torch.from_numpy(gt).to(dev), torch.from_numpy(pr).to(dev), t).cpu().numpy()


SHAPES = [(3, 1, 1), (2, 1, 77), (2, 77, 1), (3, 13, 29), (2, 65, 129), (2, 100, 100), (1, 480, 854), (1, 9, 2113)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("t", [2, 16])
def test_counts_equal_restatement_shapes(shape, t):
    rng = np.random.default_rng(sum(shape) + t)
    gt, pr = _maps(rng, *shape, "blobs")
    got = _run(gt, pr, t)
    assert got.shape == (shape[0], 4) and got.dtype == np.int64
    assert np.array_equal(got, np_counts(gt, pr, t))


@pytest.mark.parametrize("t", [0, 0.5, 1, 2, 2.5, 5, 16, 63.9, 64])
def test_counts_equal_restatement_thresholds(t):
    rng = np.random.default_rng(int(t * 10))
    for shape in ((2, 37, 61), (1, 150, 200)):
        gt, pr = _maps(rng, *shape, 0.02)
        assert np.array_equal(_run(gt, pr, t), np_counts(gt, pr, t)), (shape, t)


@pytest.mark.parametrize("density", [0.0, 0.05, 0.5, 0.95, 1.0, "checker"])
def test_counts_equal_restatement_densities(density):
    rng = np.random.default_rng(3)
    for shape, t in (((2, 31, 70), 2.5), ((1, 64, 200), 5)):
        gt, pr = _maps(rng, *shape, density)
        assert np.array_equal(_run(gt, pr, t), np_counts(gt, pr, t)), (shape, density)


def test_all_256_neighbourhoods():
    """Every 3 x 3 configuration, tiled with gaps, so each centre's multiplicity reaches n exactly as the table says."""
    P, cell = 2, 4
    gt = np.zeros((P, 16 * cell, 16 * cell), np.uint8)
    for idx in range(256):
        y, x = (idx // 16) * cell + 1, (idx % 16) * cell + 1
        gt[0, y, x] = 1
        for k, (di, dj) in enumerate(bfl.DIRS):
            gt[0, y + di, x + dj] = idx >> k & 1
    gt[1] = gt[0][::-1, ::-1]
    pr = np.roll(gt, 1, axis=2)
    for t in (0, 1.5, 3):
        assert np.array_equal(_run(gt, pr, t), np_counts(gt, pr, t))


def test_repeated_launches_bit_equal():
    rng = np.random.default_rng(4)
    gt, pr = _maps(rng, 4, 200, 300, "blobs")
    g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pr).to(dev)
    first = ops.bf_counts(g, p, 16)
    for _ in range(5):
        assert torch.equal(ops.bf_counts(g, p, 16), first)


def test_element_cap():
    g = torch.zeros((1, 8, 8), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        ops.bf_counts(g, g, 64.5)
    lib = _lib.load()
    counts = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    spans = (C.c_int * 258)(*([0, 128] * 129))
    assert lib.tt_bf_counts(g.data_ptr(), g.data_ptr(), counts.data_ptr(), 1, 8, 8, spans, 129, ops._stream()) == -1
    assert lib.tt_bf_counts(g.data_ptr(), g.data_ptr(), counts.data_ptr(), 1, 8, 8, spans, 2, ops._stream()) == -1   # even


def test_golden_bit_equal(golden, capsys):
    g, gen = golden("bfscore"), _generator()
    gt, masks = gen.make_cbfe()
    overall = BF.evaluate_bf_score(torch.from_numpy(masks), torch.from_numpy(gt), 16)
    assert bits_equal(overall, g["cbfe_overall"])
    out = capsys.readouterr().out.splitlines()
    assert out[out.index("overall boundary score") + 1] == str(np.float64(g["cbfe_overall"]))
    for k in range(len(gt)):
        s = BF.evaluate_bf_score(torch.from_numpy(masks[k:k + 1]).to(dev), torch.from_numpy(gt[k:k + 1]).to(dev))
        assert bits_equal(s, g["cbfe_scores"][k]), k
    gm, pm = gen.make_multi()
    for k in range(len(gm)):
        for j, t in enumerate(g["multi_th"]):
            want = g[f"multi{k}_t{j}"]
            if want.tolist() == [-1.0]:
                with pytest.raises(IndexError):
                    BF.bfscore(gm[k], pm[k], t)
            else:
                s, areas = BF.bfscore(torch.from_numpy(gm[k]), pm[k], t)
                assert areas is None and bits_equal(s, want), (k, t)
    for k in range(2):
        for j, t in enumerate(g["line_th"]):
            assert bits_equal(BF.bfscore(g["line_gt"][k][None], g["line_pr"][k][None], t)[0], g[f"row{k}_t{j}"])
            assert bits_equal(BF.bfscore(g["line_gt"][k][:, None], g["line_pr"][k][:, None], t)[0], g[f"col{k}_t{j}"])
    for name in gen.make_hand():
        assert bits_equal(BF.bfscore(g[f"hand_{name}_gt"], g[f"hand_{name}_pr"], 2)[0], g[f"hand_{name}_score"]), name
    assert BF.evaluate_bf_score(g["hand_single_pr"], torch.from_numpy(g["hand_single_gt"])) == 0.0


def test_multiclass_against_restatement():
    rng = np.random.default_rng(9)
    for H, W in ((60, 90), (1, 40), (40, 1)):
        gt = rng.integers(0, 4, (H, W)).astype(np.uint8)
        pr = rng.integers(0, 4, (H, W)).astype(np.uint8)
        for t in (2, 5.5):
            assert bits_equal(BF.bfscore(gt, pr, t)[0], np_bfscore(gt, pr, t))


def _driver_args(*extra):
    return ["--dataset", "synthetic", "--model_path", "", "--num_train_images", "8", "--num_val_images", "6", "--batch_size", "4",
            "--k_fg_extraction", "20", "--input_resolution", "224", *extra]


def test_cbfe_driver_bf_score(monkeypatch, capsys):
    CB.main(_driver_args())
    default_out = capsys.readouterr().out
    assert "overall boundary score" not in default_out
    seen = {}
    real = CB.evaluate_bf_score

    def record(masks, gt, *a, **k):
        seen["masks"], seen["gt"] = masks.cpu().numpy(), gt.cpu().numpy()
        seen["score"] = real(masks, gt, *a, **k)
        return seen["score"]

    monkeypatch.setattr(CB, "evaluate_bf_score", record)
    CB.main(_driver_args("--bf_score"))
    out = capsys.readouterr().out
    lines = out.splitlines()
    assert "overall boundary score" in lines
    assert lines.index("overall boundary score") < next(i for i, ln in enumerate(lines) if ln.startswith("Jaccard score is"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want = np.nanmean(np_image_scores(seen["masks"], seen["gt"]))
    assert bits_equal(seen["score"], want) and lines[lines.index("overall boundary score") + 1] == str(seen["score"])
