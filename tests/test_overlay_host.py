"""CPU-only checks of N17 (overlay rendering, matched-map GIF logs, the prototype histogram): the palette and the colours, the
entropy, the two C entries' declarations and refusals, the GIF writer read back with Pillow, and the Python layers
(``PredsmIoU.compute_segments(with_mapping=True)``, ``evaluate_localizations(logging_directory=...)``, ``Evaluator``'s clip numbering)
around torch-CPU stand-ins for the two kernels (tests/_overlay_ref.py, ``np.bincount``)."""
import math
import os
import random
import re

import numpy as np
import pytest
import torch

import _overlay_ref as REF
from timetuning_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TT_EINVAL = -1   # include/timetuning_hip.h
NEW = ("tt_overlay_grid", "tt_upsample_argmax_hist_f32")


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


# ---- colours ----------------------------------------------------------------------------------------------------------------------------

def test_voc_palette_spot_values_and_distinct_entries():
    from timetuning_amd.visualization import voc_palette

    pal = voc_palette(256)
    assert pal.shape == (256, 3) and pal.dtype == np.uint8
    for i, rgb in {0: (0, 0, 0), 1: (128, 0, 0), 2: (0, 128, 0), 3: (128, 128, 0), 4: (0, 0, 128), 15: (192, 128, 128),
                   255: (224, 224, 192)}.items():
        assert tuple(pal[i]) == rgb, i
    assert len({tuple(c) for c in pal}) == 256
    assert np.array_equal(voc_palette(21), pal[:21])


def test_generate_colors_draws_the_references_random_sequence():
    from timetuning_amd.visualization import generate_colors

    random.seed(1)
    want = [tuple(random.randint(0, 255) for _ in range(3)) for _ in range(7)]
    after = random.random()
    random.seed(1)
    assert generate_colors(7) == want
    assert random.random() == after            # 21 draws, no more
    assert generate_colors(0) == []


def test_denormalize_is_x_times_std_plus_mean_per_channel():
    from timetuning_amd.visualization import MEAN, STD, denormalize

    x = torch.arange(2 * 3 * 2 * 2, dtype=torch.float32).view(2, 3, 2, 2) / 7
    want = x * torch.tensor(STD).view(1, 3, 1, 1) + torch.tensor(MEAN).view(1, 3, 1, 1)
    assert torch.equal(denormalize(x, MEAN, STD), want)
    assert torch.equal(denormalize(x[None], MEAN, STD), want[None])       # [bs, fs, 3, H, W]
    assert STD[0] == 0.228                                                # the reference's own value (time_tuning.py:456)


def test_assignment_entropy_is_a_mean_in_fp64():
    from timetuning_amd.time_tuning import assignment_entropy

    # p = (1/2, 1/4, 1/4, 0): -(1/2 ln(1/2 + e) + 2 * 1/4 ln(1/4 + e) + 0 * ln(e)) / 4 with e = 1e-8
    want = -(0.5 * math.log(0.5 + 1e-8) + 0.5 * math.log(0.25 + 1e-8)) / 4
    got = assignment_entropy(torch.tensor([4, 2, 2, 0]))
    assert type(got) is float and abs(got - want) < 1e-15
    assert abs(want - 1.5 * math.log(2) / 4) < 1e-7                        # 1.5 bits of entropy, divided by K = 4: the mean, not the sum
    assert abs(assignment_entropy(torch.ones(200)) + math.log(1 / 200 + 1e-8) / 200) < 1e-15     # uniform: log K / K up to the 1e-8
    assert abs(assignment_entropy(torch.ones(200)) - math.log(200) / 200) < 2e-8
    assert abs(assignment_entropy(torch.tensor([[0, 7, 0]]))) < 1e-7       # [1, K] as the reference's histogram; one prototype takes all
    big = torch.tensor([2 ** 40 + 1, 2 ** 40 - 1])                         # counts beyond fp32's integers
    assert abs(assignment_entropy(big) + math.log(0.5 + 1e-8) / 2) < 1e-12


# ---- the boundary -----------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_declared_bound_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "timetuning_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tt_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.tt_abi_version() == 8          # additive
    assert "overlay.hip" in open(os.path.join(REPO, "timetuning_amd", "csrc", "Makefile")).read()
    for macro, value in (("TT_OVERLAY_PHOTO", 0), ("TT_OVERLAY_LABELS", 1), ("TT_LABELS_U8", 2)):
        assert re.search(rf"#define {macro} {value}\b", text), macro


def _overlay(lib, out=16, mode=0, frames=16, a=16, b=None, dtype=2, Hl=7, Wl=14, ytab=None, xtab=None, lut=None, lut_len=0, lut_stride=0,
             palette=16, P=3, alpha=0.5, F=3, H=7, W=14, pad=2):
    # (every refusal comes before any pointer is read or any kernel launched: dummy non-null device pointers, no GPU)
    rc = lib.tt_overlay_grid(out, mode, frames, None, None, a, b, dtype, Hl, Wl, ytab, xtab, lut, lut_len, lut_stride, palette, P, alpha, F, H, W,
                             pad, None)
    return rc, lib.tt_last_error().decode()


def test_overlay_refusals(lib):
    for null in ("out", "a", "palette", "frames"):
        rc, msg = _overlay(lib, **{null: None})
        assert rc == TT_EINVAL and "overlay_grid" in msg, (null, msg)
    rc, msg = _overlay(lib, mode=1, b=None)                                # LABELS without B
    assert rc == TT_EINVAL and "labels_b" in msg, msg
    for dim in ("F", "H", "W"):
        for bad in (0, -1):
            rc, msg = _overlay(lib, **{dim: bad})
            assert rc == TT_EINVAL and "overlay_grid" in msg, (dim, bad, msg)
    for P in (0, -3):
        rc, msg = _overlay(lib, P=P)
        assert rc == TT_EINVAL and f"P = {P}" in msg, msg
    for dtype in (3, -1):
        rc, msg = _overlay(lib, dtype=dtype)
        assert rc == TT_EINVAL and f"dtype code {dtype}" in msg, msg
    for mode in (2, -1):
        rc, msg = _overlay(lib, mode=mode)
        assert rc == TT_EINVAL and f"mode {mode}" in msg, msg
    rc, msg = _overlay(lib, pad=-1)
    assert rc == TT_EINVAL and "pad = -1" in msg, msg
    # an output row of more than 2^31 - 1 bytes: 2 W + 3 pad (photo), 3 W + 4 pad (labels)
    rc, msg = _overlay(lib, W=2 ** 30, Wl=2 ** 30, pad=0)
    assert rc == TT_EINVAL and str(2 ** 31) in msg, msg
    rc, msg = _overlay(lib, W=2 ** 30 - 2, Wl=2 ** 30 - 2, pad=2)          # 2^31 - 4 + 6
    assert rc == TT_EINVAL and str(2 ** 31 + 2) in msg, msg
    rc, msg = _overlay(lib, mode=1, b=16, W=715827883, Wl=715827883, pad=0)
    assert rc == TT_EINVAL and str(3 * 715827883) in msg, msg
    # maps of another size need both tables
    rc, msg = _overlay(lib, Hl=5, Wl=3)
    assert rc == TT_EINVAL and "index tables" in msg, msg
    rc, msg = _overlay(lib, Hl=5, Wl=3, ytab=16)
    assert rc == TT_EINVAL and "index tables" in msg, msg
    rc, msg = _overlay(lib, lut=16, lut_len=0)
    assert rc == TT_EINVAL and "lut_len = 0" in msg, msg
    rc, msg = _overlay(lib, alpha=1.5)
    assert rc == TT_EINVAL and "alpha" in msg, msg
    rc, msg = _overlay(lib, a=17, dtype=0)                                  # int16 labels at an odd address
    assert rc == TT_EINVAL and "aligned" in msg, msg


def _hist(lib, maps=16, counts=16, M=3, g=3, K=5, R=7):
    rc = lib.tt_upsample_argmax_hist_f32(maps, counts, M, g, K, R, None)
    return rc, lib.tt_last_error().decode()


def test_histogram_refusals(lib):
    for null in ("maps", "counts"):
        rc, msg = _hist(lib, **{null: None})
        assert rc == TT_EINVAL and "null pointer" in msg, (null, msg)
    for dim in ("M", "g", "K", "R"):
        rc, msg = _hist(lib, **{dim: 0})
        assert rc == TT_EINVAL and "upsample_argmax_hist_f32" in msg, (dim, msg)
    rc, msg = _hist(lib, K=16385)                                           # one bin more than the LDS histogram holds
    assert rc == TT_EINVAL and "K = 16385" in msg and "16384" in msg, msg
    rc, msg = _hist(lib, counts=20)
    assert rc == TT_EINVAL and "aligned" in msg, msg


# ---- the GIF writer ---------------------------------------------------------------------------------------------------------------------

def _palette_frames(count, h=12, w=20, colours=200, seed=0):
    """Frames over at most 256 colours, consecutive frames distinct: Pillow writes such frames losslessly and keeps every one of them
    (it quantises frames of more colours - an error of up to 60 was seen - and merges identical consecutive frames)."""
    from timetuning_amd.visualization import voc_palette

    rng = np.random.default_rng(seed)
    pal = voc_palette(256)[:colours]
    frames = [pal[rng.integers(0, colours, (h, w))] for _ in range(count)]
    assert all(not np.array_equal(a, b) for a, b in zip(frames, frames[1:]))
    return frames


@pytest.mark.parametrize("speed", [80, 1000 / 4])
def test_convert_list_to_video_reads_back_with_pillow(tmp_path, speed):
    from PIL import Image

    from timetuning_amd.visualization import convert_list_to_video

    frames = _palette_frames(4)
    path = convert_list_to_video(frames, "Score:0.5_clip_0", speed, directory=str(tmp_path) + "/")
    assert path == f"{tmp_path}/Score:0.5_clip_0.gif" and os.path.isfile(path)        # {directory}{name}.gif, my_utils.py:141
    with Image.open(path) as im:
        assert im.format == "GIF" and im.n_frames == 4 and im.size == (20, 12)
        assert im.info["loop"] == 0
        for k in range(4):
            im.seek(k)
            assert im.info["duration"] == int(speed)
            assert np.array_equal(np.asarray(im.convert("RGB")), frames[k]), k


# ---- the Python layers around stand-ins for the kernels ---------------------------------------------------------------------------------

def bincount_segments(pred, gt, num_gt, num_pred, ignore_gt=None):
    out = np.zeros((pred.shape[0], num_gt, num_pred), np.int64)
    for s, (p, g) in enumerate(zip(pred.numpy().astype(np.int64), gt.numpy())):
        ok = (g >= 0) & (g < num_gt) & (p >= 0) & (p < num_pred)
        if ignore_gt is not None:
            ok &= g != ignore_gt
        out[s] = np.bincount(g[ok] * num_pred + p[ok], minlength=num_gt * num_pred).reshape(num_gt, num_pred)
    return torch.from_numpy(out)


@pytest.fixture
def renders(monkeypatch):
    from timetuning_amd import hip_ops

    seen = []

    def overlay(mode, labels_a, palette, **kw):
        out = REF.overlay_grid(mode, labels_a, palette, **kw)
        seen.append(dict(mode=mode, labels_a=labels_a.clone(), lut=None if kw.get("lut") is None else torch.as_tensor(kw["lut"]).clone(), out=out, **{
            k: v for k, v in kw.items() if k in ("labels_b", "frames", "mean", "std", "alpha")}))
        return out

    monkeypatch.setattr(hip_ops, "overlay_grid", overlay)
    monkeypatch.setattr(hip_ops, "confusion_counts_segments", bincount_segments)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **kw: self)
    return seen


def _clips(bs=2, fs=3, R=16, k=5, seed=3):
    """Piecewise constant maps, every frame different from the one before (Pillow would merge equal ones)."""
    rng = np.random.default_rng(seed)
    gts = np.kron(rng.integers(0, 4, (bs, fs, 4, 4)), np.ones((R // 4, R // 4), np.int64))
    preds = np.where(rng.random(gts.shape) < 0.7, (gts + 1) % k, rng.integers(0, k, gts.shape)).astype(np.int16)
    for i in range(bs):
        for j in range(1, fs):
            assert not np.array_equal(gts[i, j], gts[i, j - 1]) and not np.array_equal(preds[i, j], preds[i, j - 1])
    return torch.from_numpy(gts), torch.from_numpy(preds)


def test_compute_segments_with_mapping_returns_the_table_of_the_reordered_map(renders):
    from timetuning_amd.metrics import PredsmIoU

    gts, preds = _clips()
    g, p = gts.reshape(6, -1), preds.reshape(6, -1)
    for kw in ({}, dict(many_to_one=True), dict(many_to_one=True, precision_based=True)):
        plain = PredsmIoU(5, 5).compute_segments(g, p, **kw)
        mapped = PredsmIoU(5, 5).compute_segments(g, p, **kw, with_mapping=True)
        with pytest.raises(TypeError):
            PredsmIoU(5, 5).compute_segments(g, p, False, False, None, True)          # keyword-only
        for s, (a, b) in enumerate(zip(plain, mapped)):
            assert a[4] is None and a[:4] == b[:4] and a[5] == b[5]
            lut = b[4]
            assert lut.dtype == torch.int64 and lut.numel() == int(p[s].max()) + 1
            # the table's image of the map scores what the segment scored: tp of every class is the agreement of lut[pred] with gt
            reordered = lut[p[s].long()]
            for cls, tp in b[1].items():
                assert int(((reordered == cls) & (g[s] == cls)).sum()) == tp, (s, cls)


@pytest.mark.parametrize("protocol", ["frame-wise", "sample-wise"])
def test_evaluate_localizations_writes_two_gifs_per_clip_and_returns_the_same_score(renders, tmp_path, protocol):
    from PIL import Image

    from timetuning_amd.evaluation import evaluate_localizations
    from timetuning_amd.metrics import PredsmIoU
    from timetuning_amd.visualization import voc_palette

    gts, preds = _clips()
    bs, fs, R = 2, 3, 16
    plain = evaluate_localizations(PredsmIoU(5, 5), gts, preds, protocol)
    assert renders == []
    logged = evaluate_localizations(PredsmIoU(5, 5), gts, preds, protocol, str(tmp_path))
    assert logged == plain
    assert len(renders) == 2 and all(r["mode"] == REF.LABELS for r in renders)         # one launch per GIF kind for the whole batch
    sub = tmp_path / protocol
    names = sorted(os.listdir(sub))
    assert len(names) == 4
    segs = PredsmIoU(5, 5).compute_segments(gts.reshape(-1, R * R) if protocol == "frame-wise" else gts.reshape(bs, -1),
                                            preds.reshape(-1, R * R) if protocol == "frame-wise" else preds.reshape(bs, -1), with_mapping=True)
    per = len(segs) // bs
    pal = torch.from_numpy(voc_palette())
    for i in range(bs):
        sc = [s[0] for s in segs[i * per:(i + 1) * per]]
        sep = ":" if protocol == "frame-wise" else "-"
        for kind in ("Reordered", "Inorder"):
            name = f"Score{sep}{sum(sc) / len(sc)}_Evaluation_{protocol}_{kind}_{i}.gif"
            assert name in names, (name, names)
            with Image.open(sub / name) as im:
                assert im.n_frames == fs and im.size == (3 * R + 8, R + 4) and im.info["loop"] == 0 and im.info["duration"] == 80
                for j in range(fs):
                    im.seek(j)
                    frame = torch.from_numpy(np.asarray(im.convert("RGB")).copy())
                    pred_tile = frame[2:2 + R, R + 4:2 * R + 4]                        # tile 1 of [gt | pred | both]
                    gt_tile = frame[2:2 + R, 2:2 + R]
                    p = preds[i, j].long()
                    if kind == "Reordered":
                        p = segs[(i * fs + j) if protocol == "frame-wise" else i][4][p]
                    assert torch.equal(pred_tile, pal[p]), (name, j)
                    assert torch.equal(gt_tile, pal[gts[i, j]]), (name, j)             # the ground truth is never mapped
    # dataset-wise writes nothing; an existing directory's GIFs go when a call starts at clip 0 and stay when it continues
    assert evaluate_localizations(PredsmIoU(5, 5), gts, preds, "dataset-wise", str(tmp_path)) == \
        evaluate_localizations(PredsmIoU(5, 5), gts, preds, "dataset-wise")
    assert not (tmp_path / "dataset-wise").exists()
    evaluate_localizations(PredsmIoU(5, 5), gts[:1], preds[:1], protocol, str(tmp_path), first_clip=2)
    assert len(os.listdir(sub)) == 6 and any(n.endswith("_Reordered_2.gif") for n in os.listdir(sub))
    evaluate_localizations(PredsmIoU(5, 5), gts[:1], preds[:1], protocol, str(tmp_path))
    assert len(os.listdir(sub)) == 2


def test_label_panels_and_overlay_clips_hand_the_kernel_what_it_needs(renders):
    from timetuning_amd import visualization as V

    gts, preds = _clips()
    out = V.label_panels(gts[0], preds[0])                     # int64 beside int16: one dtype reaches the kernel
    assert out.shape == (3, 3, 20, 56) and renders[-1]["labels_a"].dtype == renders[-1]["labels_b"].dtype == torch.int64
    data = torch.rand(2, 3, 3, 32, 32)
    grids = V.overlay_clips(data, preds, alpha=0.3)            # 16 x 16 maps under 32 x 32 frames: nearest tables
    assert grids.shape == (2, 3, 3, 36, 70) and renders[-1]["mode"] == REF.PHOTO and renders[-1]["alpha"] == 0.3
    up = torch.nn.functional.interpolate(preds.reshape(6, 1, 16, 16).float(), size=(32, 32), mode="nearest")[:, 0].long()
    want = REF.overlay_grid(REF.PHOTO, up, V.voc_palette(), frames=data.view(6, 3, 32, 32), alpha=0.3)
    assert torch.equal(grids.view(6, 3, 36, 70), want)
    one = V.make_overlayed_grid(data[0, 0], preds[0, 0])
    assert one.shape == (3, 36, 70) and torch.equal(one, REF.overlay_grid(REF.PHOTO, up[:1], V.voc_palette(), frames=data[0, :1])[0])
    random.seed(1)
    colors = V.generate_colors(5)
    V.overlay_clips(data, preds, colors)
    with pytest.raises(ValueError, match="colors"):
        V.overlay_clips(data, preds, [(0, 0, 256)])
    with pytest.raises(TypeError, match="integer label maps"):
        V.overlay_clips(data, preds.float())


def test_localize_clip_writes_one_gif_per_clip_at_1000_over_fs(renders, tmp_path):
    from PIL import Image

    from timetuning_amd import visualization as V

    _, preds = _clips()
    data = torch.from_numpy(V.voc_palette()[np.random.default_rng(1).integers(0, 64, (2, 3, 16, 16))]).permute(0, 1, 4, 2, 3).float() / 255
    paths = V.localize_clip(data, preds, str(tmp_path), "7")
    assert paths == [f"{tmp_path}/7_0.gif", f"{tmp_path}/7_1.gif"] and len(renders) == 1
    for path in paths:
        with Image.open(path) as im:
            assert im.n_frames == 3 and im.size == (2 * 16 + 6, 16 + 4) and im.info["loop"] == 0
            assert im.info["duration"] == 330      # 1000 / 3 ms in the hundredths of a second a GIF frame delay is stored in


def test_evaluator_numbers_the_clips_over_the_whole_loader(renders, tmp_path, monkeypatch):
    from timetuning_amd import evaluation as E

    gts, preds = _clips(bs=3)
    loader = [(torch.zeros(2, 1, 3, 3, 16, 16), gts[:2].unsqueeze(1)), (torch.zeros(1, 1, 3, 3, 16, 16), gts[2:].unsqueeze(1))]
    batches = iter([preds[:2], preds[2:]])
    ev = E.Evaluator(torch.nn.Identity(), loader, 5, "cpu", logging_directory=str(tmp_path))
    monkeypatch.setattr(ev, "_features", lambda data: (None, 1))
    monkeypatch.setattr(ev, "_cluster", lambda *a: next(batches))
    ev.evaluate(evaluation_protocol="sample-wise", eval_resolution=16, num_clusters=5)
    names = os.listdir(tmp_path / "sample-wise")
    assert sorted(int(n[:-4].rsplit("_", 1)[1]) for n in names) == [0, 0, 1, 1, 2, 2]
    assert E.Evaluator(torch.nn.Identity(), loader, 5, "cpu").logging_directory is None


def test_the_two_command_lines_have_the_new_flags():
    from timetuning_amd import evaluation as E
    from timetuning_amd import time_tuning as T

    args = E.build_parser().parse_args([])
    assert args.log_videos is False and args.logging_directory == "visualizations"
    assert E.build_parser().parse_args(["--log_videos"]).log_videos is True
    assert T.build_parser().parse_args([]).log_localization_every == 0
    assert T.build_parser().parse_args(["--log_localization_every", "4"]).log_localization_every == 4
    for name in ("localize_clip", "make_overlayed_grid", "log_clip_localization", "get_similarity_histogram", "log_assignment_histogram"):
        assert callable(getattr(T, name)), name


def test_log_assignment_histogram_prints_entropy_and_unassigned(monkeypatch, capsys):
    from timetuning_amd import time_tuning as T

    monkeypatch.setattr(T, "get_similarity_histogram", lambda model, loader, mask_features=False: torch.tensor([4, 2, 2, 0]))
    logged = []

    class Writer:
        def add_scalar(self, name, value, global_step=None):
            logged.append((name, value, global_step))

    hist, entropy = T.log_assignment_histogram(None, 4, None, False, 8, writer=Writer())
    assert entropy == T.assignment_entropy(hist) and ("Scores/entropy", entropy, 8) in logged
    out = capsys.readouterr().out
    assert "unassigned prototypes 1/4" in out and "Scores/entropy" in out
    T.log_assignment_histogram(None, 4, None, False, 8)                     # no writer: prints only
