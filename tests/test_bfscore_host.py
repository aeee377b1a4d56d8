"""CPU checks of the boundary F-score (N8, ``timetuning_amd.bfscore``).

The fixture tests/golden/bfscore.npz comes from the reference's own ``bfscore.py`` with the border-following stand-in of
tests/_border_follow.py (tools/gen_bfscore_golden.py).  Here: the stand-in gives the published answers on hand cases; the 256-entry
multiplicity table of the kernel equals the follower's visit counts in every context; the inputs regenerate; a numpy restatement of
the four counts (table + brute-force distances) turned into scores by the product's host code reproduces every fixture value to the
bit; the host branches on crafted counts; the CLI flag exists.  The kernel is checked against the same restatement on the GPU
(test_hip_bfscore.py)."""
import importlib.util
import os
import re

import numpy as np
import pytest

import _border_follow as bfl
from _metric_refs import BF_TABLE as TABLE, bf_np_counts as np_counts, np_mult
from timetuning_amd import bfscore as BF
from timetuning_amd import hip_ops
from timetuning_amd import cluster_based_foreground_extraction as CB

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location("gen_bfscore_golden", os.path.join(REPO, "tools", "gen_bfscore_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- numpy restatement of tt_bf_counts: tests/_metric_refs.py (shared with the sweep's fifth tier) -----------------------

def np_bfscore(gt, pr, t):
    """bfscore through the restated counts and the product's host code."""
    g, p = np.asarray(gt).astype(np.int64), np.asarray(pr).astype(np.int64)
    classes = np.union1d(np.unique(g), np.unique(p))
    targets = [int(c) for c in classes if c != 0]
    if not targets:
        return np.full(int(classes.max()), np.nan)
    counts = np_counts(np.stack([g == c for c in targets]), np.stack([p == c for c in targets]), t)
    return BF._scores_from_counts(targets, counts, int(classes.max()))


def np_image_scores(masks, gt, t=16):
    """evaluate_bf_score's per-image scores through the restated counts and the product's host code."""
    scores = []
    for m, g in zip(masks, gt):
        m = np.asarray(m).astype(np.uint8)
        c = np_counts((np.asarray(g) == 0)[None], (m == 1)[None], t)[0]
        scores.append(BF._image_score(m.min(), m.max(), c))
    return np.array(scores, np.float64)


def bits_equal(a, b):
    """Same shape, NaN at the same places (the reference's NaNs reach the fixture through "nan" text, so their sign bit means nothing)
    and every other value bit for bit."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64))


# ---- the border follower ------------------------------------------------------------------------------------------------

def test_follower_hand_cases():
    assert bfl.contour_points(np.array([[1, 1, 1]])) == [(0, 0), (1, 0), (2, 0), (1, 0)]   # a, b, c, b
    ring = np.ones((3, 3), np.uint8)
    ring[1, 1] = 0
    contours, _ = bfl.find_contours(ring)
    assert [len(c) for c in contours] == [8, 4]
    assert bfl.contour_points(np.pad([[5]], 2)) == [(2, 2)]   # an isolated pixel: one point
    x = np.array([[1, 0, 1], [0, 1, 0], [1, 0, 1]])
    assert bfl.visit_counts(x)[1, 1] == 4
    assert bfl.visit_counts(np.ones((4, 5)))[1:-1, 1:-1].sum() == 0   # interior pixels are not passed
    assert bfl.visit_counts(np.ones((4, 5))).sum() == 14              # edge pixels are border pixels (zero padding)


def test_table_is_the_cyclic_run_rule():
    def runs(idx):
        if idx == 0:
            return 1
        z = [not (idx >> k & 1) for k in range(8)]
        n = 0
        for k in range(8):
            if z[k] and not z[k - 1]:
                j, four = k, False
                while z[j % 8] and j < k + 8:
                    four |= j % 2 == 0
                    j += 1
                n += four
        return n

    assert [runs(i) for i in range(256)] == TABLE.tolist()
    assert TABLE.max() == 4 and TABLE[255] == 0 and TABLE[0] == 1


def test_kernel_table_is_the_follower_table():
    src = open(os.path.join(REPO, "timetuning_amd", "csrc", "bfscore.hip")).read()
    body = re.search(r"BF_MULT\[256\] = \{([^}]*)\}", src).group(1)
    assert [int(v) for v in body.replace("\n", " ").split(",")] == TABLE.tolist()


def test_table_equals_visit_counts_in_every_context():
    rng = np.random.default_rng(0)
    for idx in range(256):
        for H, W, y, x in ((3, 3, 1, 1), (7, 9, 3, 4), (5, 6, 1, 4), (6, 5, 4, 1)):
            a = (rng.random((H, W)) < 0.5).astype(np.uint8)
            a[y, x] = 1
            for k, (di, dj) in enumerate(bfl.DIRS):
                a[y + di, x + dj] = idx >> k & 1
            assert bfl.visit_counts(a)[y, x] == TABLE[idx], (idx, H, W)
    for _ in range(400):
        H, W = rng.integers(1, 12, 2)
        a = (rng.random((H, W)) < rng.random()).astype(np.uint8)
        assert np.array_equal(bfl.visit_counts(a), np_mult(a))


def test_counts_equal_point_lists():
    """The restated counts against calc_precision_recall on the follower's point lists."""
    rng = np.random.default_rng(1)
    for _ in range(40):
        H, W = rng.integers(2, 14, 2)
        g = (rng.random((H, W)) < 0.4).astype(np.uint8)
        p = (rng.random((H, W)) < 0.4).astype(np.uint8)
        if not g.any() or not p.any():
            continue
        t = float(rng.choice([0, 0.5, 1, 2, 2.5, 5]))
        gp, pp = bfl.contour_points(g), bfl.contour_points(p)
        _, hit_pr, n_pr = BF.calc_precision_recall(gp, pp, t)
        _, hit_gt, n_gt = BF.calc_precision_recall(pp, gp, t)
        assert np_counts(g[None], p[None], t)[0].tolist() == [n_pr, hit_pr, n_gt, hit_gt]


def test_element_spans():
    for t in (0, 0.5, 1, 2, 2.5, 5, 16, 63.9, 64, -3):
        spans, r = hip_ops.bf_element_spans(t)
        want = {(dy, dx) for dy in range(-66, 67) for dx in range(-66, 67) if dy * dy + dx * dx < float(t) * float(t)}
        got = {(i - r, j - r) for i, (lo, hi) in enumerate(spans) for j in range(lo, hi + 1)}
        assert got == want and len(spans) == 2 * r + 1 and r <= hip_ops.BF_MAX_RADIUS
    with pytest.raises(ValueError):
        hip_ops.bf_element_spans(64.5)


# ---- the fixture --------------------------------------------------------------------------------------------------------

def test_inputs_regenerate(golden):
    g, gen = golden("bfscore"), _generator()
    gt, masks = gen.make_cbfe()
    assert list(g["cbfe_cfg"]) == list(gen.CBFE)
    assert np.array_equal(g["cbfe_gt_sample"], gt[:, ::7, ::9]) and np.array_equal(g["cbfe_masks_sample"], masks[:, ::7, ::9])
    gm, pm = gen.make_multi()
    assert np.array_equal(g["multi_gt_sample"], gm[:, ::5, ::3]) and np.array_equal(g["multi_pr_sample"], pm[:, ::5, ::3])
    gl, pl = gen.make_lines()
    assert np.array_equal(g["line_gt"], gl) and np.array_equal(g["line_pr"], pl)
    for name, (hg, hp) in gen.make_hand().items():
        assert np.array_equal(g[f"hand_{name}_gt"], hg) and np.array_equal(g[f"hand_{name}_pr"], hp)


def test_restatement_reproduces_the_reference(golden):
    g, gen = golden("bfscore"), _generator()
    gt, masks = gen.make_cbfe()
    scores = np_image_scores(masks, gt)
    assert bits_equal(scores, g["cbfe_scores"])
    assert bits_equal(np.nanmean(scores), g["cbfe_overall"])
    gm, pm = gen.make_multi()
    for k in range(len(gm)):
        for j, t in enumerate(g["multi_th"]):
            want = g[f"multi{k}_t{j}"]
            if want.tolist() == [-1.0]:   # the reference raised
                with pytest.raises(IndexError):
                    np_bfscore(gm[k], pm[k], t)
            else:
                assert bits_equal(np_bfscore(gm[k], pm[k], t), want), (k, t)
    for k in range(2):
        for j, t in enumerate(g["line_th"]):
            assert bits_equal(np_bfscore(g["line_gt"][k][None], g["line_pr"][k][None], t), g[f"row{k}_t{j}"])
            assert bits_equal(np_bfscore(g["line_gt"][k][:, None], g["line_pr"][k][:, None], t), g[f"col{k}_t{j}"])
    for name in gen.make_hand():
        assert bits_equal(np_bfscore(g[f"hand_{name}_gt"], g[f"hand_{name}_pr"], 2), g[f"hand_{name}_score"]), name
    assert bits_equal(np_image_scores(g["hand_single_pr"], g["hand_single_gt"]), [0.0])
    assert float(g["hand_single_overall"]) == 0.0


# ---- the host branches --------------------------------------------------------------------------------------------------

def test_host_branches_on_crafted_counts(capsys):
    # gt contour empty, pr not: the caught IndexError -> [nan] for the whole call, whatever comes before or after
    out = BF._scores_from_counts([1, 2, 3], np.array([[4, 4, 4, 4], [3, 0, 0, 0], [5, 5, 5, 5]]), 3)
    assert np.isnan(out).all() and out.shape == (1,)
    assert "Caught exception" in capsys.readouterr().out
    # pr contour empty, gt not: precision nan, then the uncaught IndexError
    with pytest.raises(IndexError):
        BF._scores_from_counts([1], np.array([[0, 0, 3, 0]]), 1)
    # both empty: nan, no exception; p + r == 0: nan
    assert np.isnan(BF._f1_from_counts(0, 0, 0, 0))
    assert np.isnan(BF._f1_from_counts(4, 0, 6, 0))
    s = BF._scores_from_counts([2], np.array([[4, 1, 8, 6]]), 3)
    p, r = np.float64(1) / 4, np.float64(6) / 8
    assert np.isnan(s[0]) and np.isnan(s[2]) and s[1] == 2 * r * p / (r + p)
    # evaluate_bf_score's image rule: one value -> 0; a value >= 2 -> nan; gt background absent -> nan
    assert BF._image_score(1, 1, [0, 0, 0, 0]) == 0
    assert np.isnan(BF._image_score(0, 2, [4, 4, 4, 4]))
    assert np.isnan(BF._image_score(0, 1, [4, 4, 0, 0]))
    with pytest.raises(IndexError):
        BF._image_score(0, 2, [0, 0, 4, 0])   # class 1 is scored before the classes >= 2
    assert BF._image_score(0, 1, [4, 2, 4, 4]) == 2 * np.float64(1.0) * np.float64(0.5) / (np.float64(1.0) + np.float64(0.5))


def test_calc_precision_recall_point_lists():
    a, b = [[0, 0], [3, 0]], [[0, 1], [10, 10], [0, 1]]
    share, hits, n = BF.calc_precision_recall(a, b, 2)
    assert (hits, n) == (2, 3) and share == 2 / 3
    assert BF.calc_precision_recall(a, [[2, 0]], 1)[1] == 0          # d == t^2 misses
    with pytest.raises(IndexError):
        BF.calc_precision_recall([], b, 2)
    with np.errstate(invalid="ignore"):
        assert np.isnan(BF.calc_precision_recall(a, [], 2)[0])


def test_cli_flag():
    assert CB.build_parser().parse_args(["--bf_score"]).bf_score is True
    assert CB.build_parser().parse_args([]).bf_score is False
