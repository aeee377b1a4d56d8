"""CPU-only checks of N20, matching and scoring on the device: the two C entries and their host-side rules (shape rule, refusals), the
plain-Python restatement of the kernel's statement (``_match_ref``) against the installed scipy and numpy and against
``PredsmIoU.compute_miou_from_confusion``, and the routing of ``PredsmIoU.compute_segments`` around CPU counts."""
import os
import re

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import _match_ref as REF
from timetuning_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TT_EINVAL = -1   # include/timetuning_hip.h
NEW = ("tt_match_segments_shape_ok", "tt_match_segments")
MODES = dict(hungarian=(REF.HUNGARIAN, False, {}), many=(REF.MANY_TO_ONE, False, dict(many_to_one=True)),
             many_prec=(REF.MANY_TO_ONE, True, dict(many_to_one=True, precision_based=True)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_new_symbols_are_declared_bound_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "timetuning_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tt_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.tt_abi_version() == 8          # additive
    assert "match.hip" in open(os.path.join(REPO, "timetuning_amd", "csrc", "Makefile")).read()
    assert "TT_MATCH_HUNGARIAN 0" in text and "TT_MATCH_MANY_TO_ONE 1" in text


def test_shape_rule(lib):
    from timetuning_amd import hip_ops

    for (Cg, Cp), want in {(1, 1): 1, (21, 500): 1, (128, 1024): 1, (129, 1): 0, (1, 1025): 0, (0, 5): 0}.items():
        assert lib.tt_match_segments_shape_ok(Cg, Cp) == want, (Cg, Cp)
        assert hip_ops.match_segments_shape_ok(Cg, Cp) is bool(want) and REF.shape_ok(Cg, Cp) is bool(want)
    assert lib.tt_match_segments_shape_ok(5, 0) == 0 and lib.tt_match_segments_shape_ok(-1, 3) == 0


ARGS = ("counts", "S", "Cg", "Cp", "mode", "precision_based", "involve_bg", "score", "matched_bg", "tp", "fp", "fn", "lut", "info")


def _call(lib, **kw):
    # (every refusal comes before any pointer is read or any kernel launched: dummy non-null device pointers, no GPU)
    a = dict(counts=16, S=3, Cg=5, Cp=7, mode=0, precision_based=0, involve_bg=0, score=16, matched_bg=16, tp=16, fp=16, fn=16, lut=16, info=16)
    a.update(kw)
    rc = lib.tt_match_segments(*[a[k] for k in ARGS], None)
    return rc, lib.tt_last_error().decode()


def test_refusals_name_their_numbers(lib):
    for null in ("counts", "score", "matched_bg", "tp", "fp", "fn", "lut", "info"):
        rc, msg = _call(lib, **{null: None})
        assert rc == TT_EINVAL and "null pointer" in msg, (null, msg)
    for S in (0, -2):
        rc, msg = _call(lib, S=S)
        assert rc == TT_EINVAL and f"S = {S}" in msg, msg
    for Cg, Cp in ((0, 5), (129, 1), (5, 0), (1, 1025), (-1, 3)):
        rc, msg = _call(lib, Cg=Cg, Cp=Cp)
        assert rc == TT_EINVAL and f"Cg = {Cg}, Cp = {Cp}" in msg and "128" in msg and "1024" in msg, msg
    for mode in (2, -1):
        rc, msg = _call(lib, mode=mode)
        assert rc == TT_EINVAL and f"mode code {mode}" in msg, msg
    for name in ("counts", "score", "matched_bg", "tp", "fp", "fn", "lut"):
        rc, msg = _call(lib, **{name: 20})
        assert rc == TT_EINVAL and "aligned to 8" in msg and hex(20) in msg, (name, msg)
    rc, msg = _call(lib, info=18)
    assert rc == TT_EINVAL and "aligned to 4" in msg and hex(18) in msg, msg


# ---- the statement, restated in Python, against scipy, numpy and the host path ---------------------------------------------------------

def drawn_matrices():
    """At least 2000 count matrices, every kind of ``_match_ref.draw_counts`` at shapes from 1 x 1 to 23 x 29: more gts than preds (the
    transposed orientation), and 9 present gt classes or more (the eight-accumulator mean)."""
    rng = np.random.default_rng(20)
    shapes = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (4, 10), (5, 12), (12, 5), (9, 4), (10, 10), (13, 9), (16, 17), (23, 29), (21, 8)]
    out = []
    for rep in range(18):
        for Cg, Cp in shapes:
            for kind in REF.KINDS:
                out.append((kind, REF.draw_counts(rng, Cg, Cp, kind)))
    return out


@pytest.fixture(scope="module")
def drawn():
    return drawn_matrices()


def test_the_draws_cover_the_named_cases(drawn):
    assert len(drawn) >= 2000
    n_gt = np.array([(c.sum(1) > 0).sum() for _, c in drawn])
    n_pred = np.array([(c.sum(0) > 0).sum() for _, c in drawn])
    assert (n_gt > n_pred).sum() > 100 and (n_gt < n_pred).sum() > 100 and (n_gt >= 9).sum() > 100 and (n_gt == 8).any()
    assert sum(c.max() <= 2 for _, c in drawn) > 100 and sum((c > 0).sum() == 1 for _, c in drawn) > 100
    assert sum(c.min() == c.max() for _, c in drawn) > 100
    assert sum(c[0].sum() == 0 for _, c in drawn) > 100                                 # gt value 0 absent
    assert sum(c[0].sum() > 0 and c[1:].sum() == 0 for _, c in drawn) > 100             # gt value 0 alone
    assert sum(0 < (c.sum(0) > 0).sum() < c.shape[1] and (c.sum(0) > 0)[-1] for _, c in drawn) > 50   # absent columns inside the range


def test_lsap_restatement_equals_scipy_pair_for_pair(drawn):
    from timetuning_amd.metrics import PredsmIoU

    rng = np.random.default_rng(5)
    costs = []
    for _, c in drawn:
        conf = c[np.ix_(c.sum(1) > 0, c.sum(0) > 0)]
        costs.append(1 - PredsmIoU.score_matrix(conf))
    for shape in ((21, 50), (40, 21), (6, 6)):
        costs += [np.ones(shape), rng.integers(0, 3, shape) / 2.0, rng.random(shape)]
    for cost in costs:
        rows, cols = linear_sum_assignment(cost)
        got_rows, got_cols = REF.lsap(cost.tolist())
        assert got_rows == rows.tolist() and got_cols == cols.tolist(), cost.shape


def test_mean_restatement_equals_numpy_at_every_length():
    rng = np.random.default_rng(6)
    for n in range(1, 129):
        for a in (rng.random(n), np.round(rng.random(n), 1), np.ones(n) / 3):
            assert REF.numpy_mean(a.tolist()) == float(np.mean(np.array(a.tolist()))), n


@pytest.mark.parametrize("involve_bg", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
def test_restatement_equals_compute_miou_from_confusion(drawn, mode, involve_bg):
    from timetuning_amd.metrics import PredsmIoU

    code, precision, kw = MODES[mode]
    ev = PredsmIoU(3, 3, involve_bg=involve_bg)
    for kind, c in drawn:
        gt_unique, pred_unique = np.nonzero(c.sum(1))[0], np.nonzero(c.sum(0))[0]
        want = ev.compute_miou_from_confusion(c[np.ix_(gt_unique, pred_unique)], gt_unique, pred_unique, None, with_mapping=True, **kw)
        out = REF.match_segment(c.tolist(), code, precision, involve_bg)
        got = REF.as_compute_tuple(c.tolist(), out, True)
        assert out["status"] == REF.OK and (out["n_gt"], out["n_pred"]) == (len(gt_unique), len(pred_unique))
        assert got[0] == want[0] and got[1:4] == want[1:4] and got[5] == want[5], (kind, c.shape)
        assert list(got[1]) == list(want[1])                                            # the dicts' key order too
        assert torch.equal(got[4], want[4]), (kind, c.shape)


def test_restatement_flags_empty_and_inexact_segments():
    assert REF.match_segment([[0, 0], [0, 0]], REF.HUNGARIAN, False, False)["status"] == REF.EMPTY
    assert REF.match_segment([[2 ** 52, 0], [0, 2 ** 52]], REF.HUNGARIAN, False, False)["status"] == REF.INEXACT
    assert REF.match_segment([[2 ** 52, 0], [0, 2 ** 52 - 1]], REF.HUNGARIAN, False, False)["status"] == REF.OK


# ---- routing -------------------------------------------------------------------------------------------------------------------------------

def test_compute_segments_on_cpu_counts_never_calls_the_device_match(monkeypatch):
    from timetuning_amd import hip_ops, metrics

    def bincount_stand_in(pred, gt, num_gt, num_pred, ignore_gt=None):                  # host memory in, host memory out
        out = np.zeros((pred.shape[0], num_gt, num_pred), np.int64)
        for s, (p, g) in enumerate(zip(pred.numpy().astype(np.int64), gt.numpy())):
            out[s] = np.bincount(g * num_pred + p, minlength=num_gt * num_pred).reshape(num_gt, num_pred)
        return torch.from_numpy(out)

    assert metrics.DEVICE_MATCH in (True, False)
    monkeypatch.setattr(metrics, "DEVICE_MATCH", True)
    monkeypatch.setattr(hip_ops, "confusion_counts_segments", bincount_stand_in)
    monkeypatch.setattr(hip_ops, "match_segments", lambda *a, **k: pytest.fail("the device route was taken with counts in host memory"))
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **kw: self)
    gt = torch.tensor([[0, 1, 2, 2, 1, 1], [3, 0, 0, 3, 3, 1]])
    pred = torch.tensor([[4, 4, 0, 1, 2, 0], [1, 1, 2, 2, 0, 0]], dtype=torch.int16)
    for kw in (v[2] for v in MODES.values()):
        res = metrics.PredsmIoU(5, 4, involve_bg=True).compute_segments(gt, pred, with_mapping=True, **kw)
        assert len(res) == 2 and set(res[0][1]) == {0, 1, 2} and set(res[1][1]) == {0, 1, 3} and res[0][4].shape == (5,)
