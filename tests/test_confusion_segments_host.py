"""CPU-only checks of N15, the segmented confusion counts: the two C entries and their host-side rules (route, refusals), and
``PredsmIoU.compute_segments`` / ``compute_propagation_score`` / ``evaluation.evaluate_propagation`` / ``evaluate_localizations`` around a
``np.bincount`` stand-in for the kernel."""
import os
import re

import numpy as np
import pytest
import torch

from timetuning_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TT_EINVAL = -1   # include/timetuning_hip.h
NEW = ("tt_confusion_segments_route", "tt_confusion_counts_segments")
MODES = dict(hungarian={}, many=dict(many_to_one=True), many_prec=dict(many_to_one=True, precision_based=True))


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
    assert "confusion.hip" in open(os.path.join(REPO, "timetuning_amd", "csrc", "Makefile")).read()


def test_route_is_lds_up_to_16384_cells_and_global_up_to_4096_classes(lib):
    for Cg, Cp in ((21, 500), (128, 128), (1, 1)):
        assert lib.tt_confusion_segments_route(Cg, Cp) == 1, (Cg, Cp)
    for Cg, Cp in ((128, 129), (4096, 4096)):
        assert lib.tt_confusion_segments_route(Cg, Cp) == 2, (Cg, Cp)
    for Cg, Cp in ((0, 5), (4097, 1), (5, 0), (1, 4097), (-1, 3)):
        assert lib.tt_confusion_segments_route(Cg, Cp) == 0, (Cg, Cp)
    assert lib.tt_confusion_segments_route(4, 4096) == 1 and lib.tt_confusion_segments_route(5, 4096) == 2


def _call(lib, pred=16, dtype=0, gt=16, S=3, n=100, Cg=5, Cp=7, ignore=255, has_ignore=1, counts=16):
    # (every refusal comes before any pointer is read or any kernel launched: dummy non-null device pointers, no GPU)
    rc = lib.tt_confusion_counts_segments(pred, dtype, gt, S, n, Cg, Cp, ignore, has_ignore, counts, None)
    return rc, lib.tt_last_error().decode()


def test_refusals_name_their_numbers(lib):
    for null in ("pred", "gt", "counts"):
        rc, msg = _call(lib, **{null: None})
        assert rc == TT_EINVAL and "null pointer" in msg, (null, msg)
    rc, msg = _call(lib, S=0)
    assert rc == TT_EINVAL and "S = 0" in msg, msg
    rc, msg = _call(lib, n=0)
    assert rc == TT_EINVAL and "n = 0" in msg, msg
    for Cg, Cp in ((0, 5), (4097, 1), (5, 0), (5, 4097)):
        rc, msg = _call(lib, Cg=Cg, Cp=Cp)
        assert rc == TT_EINVAL and f"Cg = {Cg}, Cp = {Cp}" in msg and "4096" in msg, msg
    rc, msg = _call(lib, dtype=2)
    assert rc == TT_EINVAL and "dtype code 2" in msg, msg
    rc, msg = _call(lib, S=257, Cg=4096, Cp=4096)                       # more cells than the entry addresses
    assert rc == TT_EINVAL and "S = 257" in msg and str(257 * 4096 * 4096) in msg and str(2 ** 32) in msg, msg
    rc, msg = _call(lib, S=3, n=2 ** 58)
    assert rc == TT_EINVAL and f"n = {2 ** 58}" in msg and "2^59" in msg, msg
    rc, msg = _call(lib, pred=17, dtype=0)                              # int16 labels at an odd address
    assert rc == TT_EINVAL and "aligned" in msg, msg
    rc, msg = _call(lib, pred=18, dtype=1)
    assert rc == TT_EINVAL and "aligned" in msg, msg
    rc, msg = _call(lib, gt=20)
    assert rc == TT_EINVAL and "aligned" in msg, msg


# ---- the Python layers, with np.bincount standing in for the kernel --------------------------------------------------------------------------

def bincount_segments(calls):
    def stand_in(pred, gt, num_gt, num_pred, ignore_gt=None):
        assert pred.dim() == 2 and pred.shape == gt.shape and gt.dtype == torch.int64 and pred.dtype in (torch.int16, torch.int64)
        calls.append((tuple(pred.shape), num_gt, num_pred, ignore_gt))
        out = np.zeros((pred.shape[0], num_gt, num_pred), np.int64)
        for s, (p, g) in enumerate(zip(pred.numpy().astype(np.int64), gt.numpy())):
            ok = (g >= 0) & (g < num_gt) & (p >= 0) & (p < num_pred)
            if ignore_gt is not None:
                ok &= g != ignore_gt
            out[s] = np.bincount(g[ok] * num_pred + p[ok], minlength=num_gt * num_pred).reshape(num_gt, num_pred)
        return torch.from_numpy(out)
    return stand_in


@pytest.fixture
def calls(monkeypatch):
    from timetuning_amd import hip_ops

    seen = []
    monkeypatch.setattr(hip_ops, "confusion_counts_segments", bincount_segments(seen))
    monkeypatch.setattr(hip_ops, "confusion_counts", lambda *a, **k: pytest.fail("confusion_counts is not part of the segmented route"))
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **kw: self)
    return seen


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_compute_segments_at_one_segment_reproduces_the_golden_scores(golden, calls, tag):
    from timetuning_amd.metrics import PredsmIoU

    d = golden("evaluator")
    gt, pred = torch.from_numpy(d[f"{tag}_gt"].astype(np.int64))[None], torch.from_numpy(d[f"{tag}_pred"])[None]   # pred stays int16
    for involve_bg in (0, 1):
        for mode, kw in MODES.items():
            key = f"{tag}_{mode}_{involve_bg}"
            (score, tp, fp, fn, reordered, bg), = PredsmIoU(3, 3, involve_bg=bool(involve_bg)).compute_segments(gt, pred, **kw)
            assert abs(score - float(d[key + "_score"])) < 1e-12, key
            ks = [int(k) for k in d[key + "_classes"]]
            assert [tp[k] for k in ks] == list(d[key + "_tp"]) and [fp[k] for k in ks] == list(d[key + "_fp"]) and [fn[k] for k in ks] == list(d[key + "_fn"])
            assert reordered is None and abs(bg - float(d[key + "_bg"])) < 1e-12
    assert len(calls) == 6 and all(c[0] == (1, gt.shape[1]) and c[3] is None for c in calls)


def test_compute_segments_sizes_the_matrices_without_the_ignored_value_and_refuses_an_empty_segment(calls):
    from timetuning_amd.metrics import PredsmIoU

    gt = torch.tensor([[0, 1, 2, 255, 255, 1], [255, 0, 0, 3, 3, 255]])
    pred = torch.tensor([[4, 4, 0, 1, 2, 0], [1, 1, 2, 2, 0, 0]], dtype=torch.int16)
    res = PredsmIoU(5, 4, involve_bg=True).compute_segments(gt, pred, ignore_gt=255)
    assert calls == [((2, 6), 4, 5, 255)] and len(res) == 2                # 21 x 500 stays 21 x 500 beside a 255 border
    assert set(res[0][1]) == {0, 1, 2} and set(res[1][1]) == {0, 3}
    with pytest.raises(ValueError, match="segment 1 has no element"):
        PredsmIoU(5, 4).compute_segments(torch.tensor([[1, 2], [255, 255]]), torch.tensor([[0, 1], [0, 1]]), ignore_gt=255)
    with pytest.raises(ValueError, match=r"\[S, n\]"):
        PredsmIoU(5, 4).compute_segments(torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))


def test_propagation_score_equals_the_reference(golden, calls):
    from timetuning_amd.evaluation import evaluate_propagation
    from timetuning_amd.metrics import PredsmIoU

    d = golden("propagation_score")
    gts, preds = torch.from_numpy(d["gts"]), torch.from_numpy(d["preds"])
    assert gts.shape[1] <= 6 and max(gts.shape[2:]) <= 32
    for i in range(gts.shape[0]):
        for tag, (a, b) in dict(scores=(gts, preds), scores_swapped=(preds, gts)).items():
            m = PredsmIoU(4, 4)
            for j in range(gts.shape[1]):
                m.update(a[i, j], b[i, j])
            got = m.compute_propagation_score(True)
            assert all(type(v) is float for v in got) and got == list(d[f"clip{i}_{tag}"]), (i, tag, got)
            assert m.compute_propagation_score(False) is None
    assert len(calls) == 2 * gts.shape[0]                                    # one segmented call per clip
    # the fixture's edge cases are in it: an object missing from some frames, and one the predictions alone hold
    assert (d["gts"][0, 1] == 2).sum() == 0 and (d["gts"][0, 0] == 2).sum() > 0 and (d["preds"] == 5).any() and not (d["gts"] == 5).any()
    assert len(d["clip2_scores_swapped"]) == len(d["clip2_scores"]) + 1
    got = evaluate_propagation(PredsmIoU(4, 4), gts, preds)
    assert got == float(d["evaluate_propagation"])
    with pytest.raises(ValueError, match="negative labels"):
        PredsmIoU(4, 4).compute_propagation_iou(torch.tensor([[0, -1, 1]]), torch.tensor([[0, 1, 1]]))


@pytest.mark.parametrize("protocol,segments,ignore", [("frame-wise", 6, None), ("sample-wise", 2, None), ("dataset-wise", 1, 255)])
def test_evaluate_localizations_makes_one_segmented_call_and_scores_like_the_loop(calls, protocol, segments, ignore):
    from timetuning_amd.evaluation import evaluate_localizations
    from timetuning_amd.metrics import PredsmIoU

    rng = np.random.default_rng(3)
    bs, fs, R, k = 2, 3, 12, 5
    gts = np.kron(rng.integers(0, 4, (bs, fs, 3, 3)), np.ones((4, 4), np.int64))
    gts[:, :, 0, :] = 255
    preds = np.where(rng.random(gts.shape) < 0.7, gts % k, rng.integers(0, k, gts.shape)).astype(np.int16)
    gts_t, preds_t = torch.from_numpy(gts), torch.from_numpy(preds)
    for kw in MODES.values():
        for involve_bg in (False, True):
            del calls[:]
            ev = PredsmIoU(k, k, involve_bg=involve_bg)
            got = evaluate_localizations(ev, gts_t, preds_t, protocol, None, **kw)
            assert len(calls) == 1 and calls[0][0] == (segments, bs * fs * R * R // segments) and calls[0][3] == ignore
            assert ev.gt == [] and ev.pred == []
            # the loop this replaces, on compute_miou_from_confusion directly (PredsmIoU.compute needs the GPU entry)
            scores = []
            for g, p in zip(gts.reshape(segments, -1), preds.reshape(segments, -1).astype(np.int64)):
                if ignore is not None:
                    g, p = g[g != ignore], p[g != ignore]
                gu, pu = np.unique(g), np.unique(p)
                conf = np.array([[np.sum((g == a) & (p == b)) for b in pu] for a in gu])
                scores.append(PredsmIoU(k, k, involve_bg=involve_bg).compute_miou_from_confusion(conf, gu, pu, None, **kw)[0])
            assert got == sum(scores) / len(scores)
    with pytest.raises(ValueError, match="unknown evaluation protocol"):
        evaluate_localizations(PredsmIoU(k, k), gts_t, preds_t, "clip-wise")
