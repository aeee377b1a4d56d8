"""GPU checks of N15: ``tt_confusion_counts_segments`` against ``torch.bincount`` at every route, dtype, alignment and ignore value, and
the evaluation protocols built on it against the per-frame loop over the public ``PredsmIoU.update / compute / reset`` they replace."""
import numpy as np
import pytest
import torch

from timetuning_amd import _lib
from timetuning_amd import hip_ops as ops

pytestmark = pytest.mark.gpu

SEGMENTS = (1, 3, 64)
LENGTHS = (1, 63, 64, 255, 257, 777, 4095, 4097)     # odd n at S > 1 with int16: segments that start 2-byte aligned only
SHAPES = ((1, 1), (3, 5), (21, 500), (128, 128), (127, 129), (128, 129), (5, 4096))   # LDS up to 16384 cells, global atomics beyond
IGNORES = (None, 255, 0)
MODES = dict(hungarian={}, many=dict(many_to_one=True), many_prec=dict(many_to_one=True, precision_based=True))


def expected(pred, gt, Cg, Cp, ignore):
    """torch.bincount of gt * Cp + pred per segment (the segment's offset folded into the key), after the kernel's filtering."""
    S = pred.shape[0]
    p, g = pred.long(), gt
    ok = (g >= 0) & (g < Cg) & (p >= 0) & (p < Cp)
    if ignore is not None:
        ok &= g != ignore
    key = (torch.arange(S, device=pred.device)[:, None] * Cg + g) * Cp + p
    return torch.bincount(key[ok], minlength=S * Cg * Cp).view(S, Cg, Cp)


def draw(gen, count, C, dtype):
    """Labels in [-1, C + 1]: -1 and values >= C are among them (and 0, the third ignore value)."""
    return torch.randint(-1, C + 2, (count,), generator=gen, device="cuda").to(dtype)


@pytest.mark.parametrize("dtype", [torch.int16, torch.int64], ids=["int16", "int64"])
@pytest.mark.parametrize("Cg,Cp", SHAPES)
def test_counts_equal_bincount_on_the_grid_of_small_shapes(Cg, Cp, dtype):
    assert _lib.load().tt_confusion_segments_route(Cg, Cp) == (1 if Cg * Cp <= 16384 else 2)
    gen = torch.Generator(device="cuda").manual_seed(Cg * 8192 + Cp)
    pred_all, gt_all = draw(gen, 64 * 4097, Cp, dtype), draw(gen, 64 * 4097, Cg, torch.int64)
    gt_all[::37] = 255                                      # the Pascal value, inside or outside [0, Cg)
    for S in SEGMENTS:
        for n in LENGTHS:
            pred, gt = pred_all[: S * n].view(S, n), gt_all[: S * n].view(S, n)
            for ignore in IGNORES:
                got = ops.confusion_counts_segments(pred, gt, Cg, Cp, ignore)
                assert got.shape == (S, Cg, Cp) and got.dtype == torch.int64
                assert torch.equal(got, expected(pred, gt, Cg, Cp, ignore)), (S, n, ignore)


@pytest.mark.parametrize("dtype", [torch.int16, torch.int64], ids=["int16", "int64"])
def test_tensors_that_start_off_a_16_byte_boundary(dtype):
    """Views one element into their storage: pred 2 (8) bytes and gt 8 bytes past a 16-byte boundary, so the strips start after a head
    of up to 7 elements and gt is read in 8-byte loads; and gt alone shifted, pred aligned."""
    gen = torch.Generator(device="cuda").manual_seed(5)
    Cg, Cp, S = 6, 9, 3
    for n in (1, 5, 8, 9, 777, 4097):
        pred_all, gt_all = draw(gen, S * n + 3, Cp, dtype), draw(gen, S * n + 3, Cg, torch.int64)
        for po, go in ((1, 1), (0, 1), (3, 0), (1, 2)):
            pred, gt = pred_all[po: po + S * n].view(S, n), gt_all[go: go + S * n].view(S, n)
            assert torch.equal(ops.confusion_counts_segments(pred, gt, Cg, Cp, 0), expected(pred, gt, Cg, Cp, 0)), (n, po, go)


@pytest.mark.parametrize("Cg,Cp", [(5, 10), (21, 500), (130, 130)])
def test_run_shaped_labels_and_one_cell_that_takes_every_count(Cg, Cp):
    """Labels constant in blocks of 16, as up-sampled token maps are (the strips of 8 merge them into one atomic per run), and one segment
    with every element equal: a single cell receives n counts."""
    gen = torch.Generator(device="cuda").manual_seed(9)
    S, n = 4, 50176
    pred = draw(gen, S * n // 16, Cp, torch.int16).repeat_interleave(16).view(S, n).clone()
    gt = draw(gen, S * n // 16, Cg, torch.int64).repeat_interleave(16).view(S, n).clone()
    pred[2], gt[2] = Cp - 1, Cg - 1
    got = ops.confusion_counts_segments(pred, gt, Cg, Cp)
    assert torch.equal(got, expected(pred, gt, Cg, Cp, None))
    assert int(got[2, Cg - 1, Cp - 1]) == n and int(got[2].sum()) == n
    assert torch.equal(ops.confusion_counts_segments(pred.long(), gt, Cg, Cp, 1), expected(pred, gt, Cg, Cp, 1))


def test_a_255_border_beside_256_ground_truth_rows():
    """ignore_gt = 255 where 255 is inside [0, Cg): the row stays empty."""
    gen = torch.Generator(device="cuda").manual_seed(11)
    pred, gt = draw(gen, 3 * 3000, 10, torch.int16).view(3, 3000), draw(gen, 3 * 3000, 256, torch.int64).view(3, 3000)
    gt[:, ::5] = 255
    got = ops.confusion_counts_segments(pred, gt, 256, 10, 255)
    assert torch.equal(got, expected(pred, gt, 256, 10, 255)) and int(got[:, 255].sum()) == 0
    assert int(ops.confusion_counts_segments(pred, gt, 256, 10)[:, 255].sum()) > 0


def test_more_segments_than_one_launch_carries():
    gen = torch.Generator(device="cuda").manual_seed(13)
    S, n, Cg, Cp = 65536 + 3, 5, 3, 5
    pred, gt = draw(gen, S * n, Cp, torch.int16).view(S, n), draw(gen, S * n, Cg, torch.int64).view(S, n)
    got = ops.confusion_counts_segments(pred, gt, Cg, Cp, 0)
    assert torch.equal(got, expected(pred, gt, Cg, Cp, 0))
    assert int(got[65535:].sum()) > 0                       # the second launch's segments were counted


@pytest.mark.parametrize("C", [7, 96, 130])
def test_one_square_segment_equals_confusion_counts(C):
    gen = torch.Generator(device="cuda").manual_seed(C)
    n = 30001
    pred, gt = draw(gen, n, C, torch.int64), draw(gen, n, C, torch.int64)
    want = ops.confusion_counts(pred, gt, C)
    assert torch.equal(ops.confusion_counts_segments(pred[None], gt[None], C, C)[0], want)
    assert torch.equal(ops.confusion_counts_segments(pred.to(torch.int16)[None], gt[None], C, C)[0], want)


def test_front_end_checks():
    z = torch.zeros((2, 8), dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.HipLibraryError):
        ops.confusion_counts_segments(z.cpu(), z.cpu(), 3, 3)
    with pytest.raises(TypeError):
        ops.confusion_counts_segments(z.int(), z, 3, 3)
    with pytest.raises(TypeError):
        ops.confusion_counts_segments(z, z.int(), 3, 3)
    with pytest.raises(ValueError):
        ops.confusion_counts_segments(z, z[:1], 3, 3)
    with pytest.raises(ValueError):
        ops.confusion_counts_segments(z.t(), z.t(), 3, 3)
    with pytest.raises(_lib.HipLibraryError, match=r"Cg = 4097, Cp = 3"):
        ops.confusion_counts_segments(z, z, 4097, 3)


# ---- the scores ---------------------------------------------------------------------------------------------------------------------------------

def loop_over_compute(ev, gts, preds, protocol, many_to_one, precision_based):
    """evaluate_localizations as a loop over the public PredsmIoU.update / compute / reset: one compute per frame, per clip or per
    dataset, Pascal's 255 filtered with a mask per frame - what the segmented route replaces."""
    scores = []
    if protocol == "frame-wise":
        for i, datum in enumerate(preds):
            for j, frame in enumerate(datum):
                ev.update(gts[i, j].flatten(), frame.flatten())
                scores.append(ev.compute(True, many_to_one, precision_based=precision_based)[0])
                ev.reset()
    elif protocol == "sample-wise":
        for i, datum in enumerate(preds):
            for j, frame in enumerate(datum):
                ev.update(gts[i, j].flatten(), frame.flatten())
            scores.append(ev.compute(True, many_to_one, precision_based=precision_based)[0])
            ev.reset()
    else:
        for i, datum in enumerate(preds):
            for j, frame in enumerate(datum):
                valid = gts[i, j] != 255
                ev.update(gts[i, j][valid].flatten(), frame[valid].flatten())
        scores.append(ev.compute(True, many_to_one, precision_based=precision_based)[0])
        ev.reset()
    return sum(scores) / len(scores)


def block_maps(bs, fs, R, classes, k, seed, border):
    """Ground truth constant on 7 x 7 blocks (values 0 ... classes - 1, optionally a 255 border), predictions a noisy function of it."""
    rng = np.random.default_rng(seed)
    gts = np.kron(rng.integers(0, classes, (bs, fs, R // 7, R // 7)), np.ones((7, 7), np.int64))
    fine = np.kron(rng.integers(0, k, (bs, fs, R // 7, R // 7)), np.ones((7, 7), np.int64))
    preds = np.where(rng.random(gts.shape) < 0.6, (gts * (k // classes) + fine % (k // classes)) % k, rng.integers(0, k, gts.shape))
    if border:
        gts[:, :, 0, :] = gts[:, :, -1, :] = gts[:, :, :, 0] = gts[:, :, :, -1] = 255
    return torch.from_numpy(gts).cuda(), torch.from_numpy(preds.astype(np.int16)).cuda()


@pytest.fixture
def old_entry_calls(monkeypatch):
    seen, real = [], ops.confusion_counts

    def spy(*a, **k):
        seen.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "confusion_counts", spy)
    return seen


@pytest.mark.parametrize("protocol", ["frame-wise", "sample-wise", "dataset-wise"])
def test_evaluate_localizations_equals_the_loop_over_compute(protocol, old_entry_calls):
    from timetuning_amd.evaluation import evaluate_localizations
    from timetuning_amd.metrics import PredsmIoU

    gts, preds = block_maps(2, 3, 28, 4, 5, seed=17, border=protocol == "dataset-wise")
    for involve_bg in (False, True):
        for kw in MODES.values():
            many, prec = kw.get("many_to_one", False), kw.get("precision_based", False)
            for p in (preds, preds.long()):           # what cluster_features and what proto_clustering return
                del old_entry_calls[:]
                got = evaluate_localizations(PredsmIoU(5, 5, involve_bg=involve_bg), gts, p, protocol, None, many, prec)
                assert old_entry_calls == []            # tt_confusion_counts is not on the segmented route
                want = loop_over_compute(PredsmIoU(5, 5, involve_bg=involve_bg), gts, p, protocol, many, prec)
                assert len(old_entry_calls) == {"frame-wise": 6, "sample-wise": 2, "dataset-wise": 1}[protocol]
                assert got == want, (protocol, involve_bg, kw)


def test_over_clustering_scores_equal_the_loop(old_entry_calls):
    """k = 300 against 4 classes at R = 56, many-to-one, with a 255 border: the dataset-wise shape whose matrix the parent counted with
    global atomics."""
    from timetuning_amd.evaluation import evaluate_localizations
    from timetuning_amd.metrics import PredsmIoU

    gts, preds = block_maps(3, 1, 56, 4, 300, seed=19, border=True)
    for involve_bg in (False, True):
        for prec in (False, True):
            got = evaluate_localizations(PredsmIoU(300, 4, involve_bg=involve_bg), gts, preds, "dataset-wise", None, True, prec)
            assert old_entry_calls == []
            assert got == loop_over_compute(PredsmIoU(300, 4, involve_bg=involve_bg), gts, preds, "dataset-wise", True, prec)
            del old_entry_calls[:]


def test_propagation_score_equals_the_reference(golden):
    from timetuning_amd.evaluation import evaluate_propagation
    from timetuning_amd.metrics import PredsmIoU

    d = golden("propagation_score")
    gts, preds = torch.from_numpy(d["gts"]).cuda(), torch.from_numpy(d["preds"]).cuda()
    for i in range(gts.shape[0]):
        for tag, (a, b) in dict(scores=(gts, preds), scores_swapped=(preds, gts)).items():
            m = PredsmIoU(4, 4)
            for j in range(gts.shape[1]):
                m.update(a[i, j], b[i, j])
            assert m.compute_propagation_score(True) == list(d[f"clip{i}_{tag}"]), (i, tag)
    assert evaluate_propagation(PredsmIoU(4, 4), gts, preds) == float(d["evaluate_propagation"])
    assert evaluate_propagation(PredsmIoU(4, 4), gts.long(), preds.long()) == float(d["evaluate_propagation"])
