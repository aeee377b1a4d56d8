"""N20 on the GPU: ``tt_match_segments`` behind ``PredsmIoU.compute_segments`` against the host loop over
``compute_miou_from_confusion`` (the installed scipy and numpy: the yardstick), with ``==``.  The count matrices are built directly as
int64 tensors and handed in where ``confusion_counts_segments`` would put them, so every shape, every kind of counts and every status
is reached without label maps; the whole call (``evaluate_localizations``) runs on real maps."""
import numpy as np
import pytest
import torch

import _match_ref as REF

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (7, 1), (3, 3), (5, 12), (12, 5), (10, 10), (21, 21), (21, 500), (128, 128), (16, 1024)]
SEGMENTS = (1, 3, 70)
MODES = dict(hungarian={}, many=dict(many_to_one=True), many_prec=dict(many_to_one=True, precision_based=True))


def drawn_segments(Cg, Cp):
    """70 matrices of one shape: the kinds of ``_match_ref.draw_counts`` in turn, segment 1 with counts near 2^40 (in at most about
    1000 cells, so that its total, below 2^51, stays exact in fp64)."""
    rng = np.random.default_rng(1000 * Cg + Cp)
    out = np.stack([REF.draw_counts(rng, Cg, Cp, REF.KINDS[s % len(REF.KINDS)]) for s in range(max(SEGMENTS))])
    large = rng.integers(500, 1000, (Cg, Cp)) * (rng.random((Cg, Cp)) < 1000 / (Cg * Cp)) * 2 ** 30
    out[1] = large + REF.draw_counts(rng, Cg, Cp, "small")
    assert 2 ** 38 < out[1].max() < 2 ** 40 and out[1].sum() < 2 ** 51
    return out


def compute_segments_on(counts, device_match, monkeypatch, involve_bg=False, with_mapping=True, **kw):
    """``compute_segments`` with ``counts`` (a GPU tensor) standing where the counting launch would put them."""
    from timetuning_amd import hip_ops, metrics

    S = counts.shape[0]
    with monkeypatch.context() as mp:
        mp.setattr(metrics, "DEVICE_MATCH", device_match)
        mp.setattr(hip_ops, "confusion_counts_segments", lambda *a, **k: counts)
        launches, real = [], hip_ops.match_segments
        if not device_match:
            mp.setattr(hip_ops, "match_segments", lambda *a, **k: pytest.fail("the yardstick is the host loop"))
        else:
            mp.setattr(hip_ops, "match_segments", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
        ev = metrics.PredsmIoU(3, 3, involve_bg=involve_bg)
        zeros = torch.zeros((S, 1), dtype=torch.int64)
        try:
            res = ev.compute_segments(zeros, zeros, with_mapping=with_mapping, **kw)
        finally:
            assert len(launches) == int(device_match)                               # one launch, or the host loop alone
    return res, (ev.num_pred_classes, ev.num_gt_classes)


def assert_equal_results(got, want, note):
    assert len(got) == len(want), note
    for s, (g, w) in enumerate(zip(got, want)):
        assert type(g[0]) is float and g[0] == w[0], (note, s, g[0], w[0])
        assert type(g[5]) is float and g[5] == w[5], (note, s, g[5], w[5])
        for k in (1, 2, 3):
            assert g[k] == w[k] and list(g[k]) == list(w[k]) and all(type(v) is int for v in g[k].values()), (note, s, k, g[k], w[k])
        if w[4] is None:
            assert g[4] is None, (note, s)
        else:
            assert g[4].dtype == torch.int64 and not g[4].is_cuda and torch.equal(g[4], w[4]), (note, s, g[4], w[4])


@pytest.mark.parametrize("Cg,Cp", SHAPES)
def test_device_route_equals_the_host_loop(monkeypatch, Cg, Cp):
    """The shapes reach: the transposed orientation (12 x 5, 7 x 1), partly filled last chunks of 64 lanes (7, 12, 21, 500), lists longer
    than one pass of the wave (128 x 128, 21 x 500, 16 x 1024), absent rows and columns inside the range (the sparse kinds), 8 gt classes
    and more in the mean (10 x 10 upwards) and, at S = 70 one-wave workgroups of up to 54 KB LDS, more segments than one CU holds."""
    from timetuning_amd import hip_ops, metrics

    host = drawn_segments(Cg, Cp)
    counts = torch.from_numpy(host).cuda()
    for mode, kw in MODES.items():
        for involve_bg in (False, True):
            want, want_classes = compute_segments_on(counts, False, monkeypatch, involve_bg, **kw)
            for S in SEGMENTS:
                part = counts[:S].contiguous()
                got, classes = compute_segments_on(part, True, monkeypatch, involve_bg, **kw)
                assert_equal_results(got, want[:S], (Cg, Cp, mode, involve_bg, S))
                if S == max(SEGMENTS):
                    assert classes == want_classes
    # every segment was scored by the kernel, none by the fallback
    m = hip_ops.match_segments(counts, "hungarian").cpu()
    assert m.info[:, 0].tolist() == [0] * max(SEGMENTS)
    assert metrics.DEVICE_MATCH in (True, False)


def test_without_mapping_slot_four_is_none(monkeypatch):
    counts = torch.from_numpy(drawn_segments(5, 12)[:3]).cuda()
    want, _ = compute_segments_on(counts, False, monkeypatch, with_mapping=False)
    got, _ = compute_segments_on(counts, True, monkeypatch, with_mapping=False)
    assert all(r[4] is None for r in got)
    assert_equal_results(got, want, "no mapping")


def test_an_empty_segment_raises_the_host_message(monkeypatch):
    host = drawn_segments(5, 12)[:3]
    host[1] = 0
    counts = torch.from_numpy(host).cuda()
    for device_match in (False, True):
        with pytest.raises(ValueError, match="compute_segments: segment 1 has no element to score"):
            compute_segments_on(counts, device_match, monkeypatch)


def test_a_total_of_2_to_the_53_is_flagged_and_scored_by_the_host(monkeypatch):
    from timetuning_amd import hip_ops

    host = drawn_segments(3, 3)[:3]
    host[1] = 0
    host[1, 0, 1] = host[1, 2, 2] = 2 ** 52
    counts = torch.from_numpy(host).cuda()
    m = hip_ops.match_segments(counts, "hungarian").cpu()
    assert m.info[:, 0].tolist() == [0, 3, 0] and m.info[1].tolist() == [3, 2, 2, 2]
    assert m.score[1].item() == 0.0 and not m.tp[1].any() and not m.lut[1].any()
    for kw in MODES.values():
        want, _ = compute_segments_on(counts, False, monkeypatch, True, **kw)
        got, _ = compute_segments_on(counts, True, monkeypatch, True, **kw)
        assert_equal_results(got, want, "inexact")


def test_two_calls_give_equal_bits():
    from timetuning_amd import hip_ops

    counts = torch.from_numpy(drawn_segments(21, 21)).cuda()
    for mode in ("hungarian", "many_to_one"):
        a, b = hip_ops.match_segments(counts, mode, False, True), hip_ops.match_segments(counts, mode, False, True)
        assert torch.equal(a.packed, b.packed)
        assert a.packed.numel() == hip_ops.MatchedSegments.words(70, 21, 21)


def test_wrapper_refuses_what_it_cannot_take():
    from timetuning_amd import _lib, hip_ops

    counts = torch.zeros((2, 3, 4), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="mode"):
        hip_ops.match_segments(counts, "greedy")
    with pytest.raises(ValueError, match=r"\[S, Cg, Cp\]"):
        hip_ops.match_segments(counts[0])
    with pytest.raises(TypeError):
        hip_ops.match_segments(counts.int())
    with pytest.raises(_lib.HipLibraryError, match="Cg = 129"):
        hip_ops.match_segments(torch.zeros((1, 129, 4), dtype=torch.int64, device="cuda"))


@pytest.fixture(scope="module")
def maps():
    rng = np.random.default_rng(3)
    bs, fs, R, k = 2, 3, 32, 5
    gts = np.kron(rng.integers(0, 4, (bs, fs, 4, 4)), np.ones((8, 8), np.int64))
    gts[:, :, 0, :] = 255
    gts[:, :, :, -1] = 255
    preds = np.where(rng.random(gts.shape) < 0.7, gts % k, rng.integers(0, k, gts.shape)).astype(np.int16)
    return torch.from_numpy(gts).cuda(), torch.from_numpy(preds).cuda(), k


@pytest.mark.parametrize("protocol", ["frame-wise", "sample-wise", "dataset-wise"])
def test_evaluate_localizations_is_unchanged_by_the_switch(monkeypatch, maps, protocol):
    from timetuning_amd import hip_ops, metrics
    from timetuning_amd.evaluation import evaluate_localizations

    gts, preds, k = maps
    if protocol != "dataset-wise":
        gts = torch.where(gts == 255, 0, gts)                                       # the 255 border belongs to the dataset-wise case
    launches = []
    real = hip_ops.match_segments
    monkeypatch.setattr(hip_ops, "match_segments", lambda *a, **kw: (launches.append(a[0].shape), real(*a, **kw))[1])
    for kw in MODES.values():
        for involve_bg in (False, True):
            scores = {}
            for switch in (False, True):
                monkeypatch.setattr(metrics, "DEVICE_MATCH", switch)
                del launches[:]
                scores[switch] = evaluate_localizations(metrics.PredsmIoU(k, k, involve_bg=involve_bg), gts, preds, protocol, None, **kw)
                assert len(launches) == int(switch)
            assert type(scores[True]) is float and scores[True] == scores[False], (protocol, kw, involve_bg, scores)


@pytest.mark.parametrize("protocol", ["frame-wise", "sample-wise"])
def test_mapping_tables_are_unchanged_by_the_switch(monkeypatch, maps, protocol):
    from timetuning_amd import metrics

    gts, preds, k = maps
    gts = torch.where(gts == 255, 0, gts)
    segments = 6 if protocol == "frame-wise" else 2
    for kw in MODES.values():
        res = {}
        for switch in (False, True):
            monkeypatch.setattr(metrics, "DEVICE_MATCH", switch)
            res[switch] = metrics.PredsmIoU(k, k).compute_segments(gts.reshape(segments, -1), preds.reshape(segments, -1), with_mapping=True, **kw)
        assert_equal_results(res[True], res[False], (protocol, kw))
