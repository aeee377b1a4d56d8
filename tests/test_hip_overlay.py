"""GPU checks of N17: ``tt_overlay_grid`` against the torch-CPU restatement of tests/_overlay_ref.py with ``torch.equal`` - both modes,
row widths that are no multiple of 16 bytes, every label dtype, the tables, the LUT forms, the modulo, the clamp -,
``tt_upsample_argmax_hist_f32`` against ``torch.bincount`` of ``upsample_argmax_f32``'s labels, and the layers built on them end to end."""
import os

import numpy as np
import pytest
import torch

import _overlay_ref as REF
from timetuning_amd import hip_ops as ops

pytestmark = pytest.mark.gpu

DTYPES = [torch.uint8, torch.int16, torch.int64]
# (F, H, W, pad): a 34-byte row (both row ends and unaligned row starts), a 32-byte row, no padding, one full-size frame
PHOTO_SHAPES = [(3, 7, 14, 2), (3, 7, 13, 2), (3, 7, 14, 0), (2, 5, 3, 1), (1, 224, 224, 2)]


def _palette(P, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (P, 3), dtype=np.uint8))


def _labels(gen, shape, dtype, hi):
    """Labels in [0, hi) with the values 255 and (where the dtype has them) negative ones planted."""
    v = torch.randint(0, hi, shape, generator=gen).to(dtype)
    flat = v.view(-1)
    flat[0] = 255
    if dtype != torch.uint8:
        flat[1], flat[-1] = -1, -7
    return v


def _frames(gen, F, H, W):
    x = torch.rand((F, 3, H, W), generator=gen) * 1.3 - 0.15            # beyond [0, 1] on both sides
    flat = x.view(-1)
    flat[0], flat[1], flat[2], flat[3], flat[4] = 1.2, -0.1, float("nan"), 1.0, 0.0
    flat[5], flat[6] = float("inf"), -float("inf")
    return x


def _check(mode, a, palette, **kw):
    want = REF.overlay_grid(mode, a, palette, **kw)
    dev = {k: (v.cuda() if isinstance(v, torch.Tensor) and k in ("frames", "labels_b") else v) for k, v in kw.items()}
    got = ops.overlay_grid(mode, a.cuda(), palette, **dev)
    assert got.dtype == torch.uint8 and got.shape == want.shape
    assert torch.equal(got.cpu(), want), (mode, tuple(want.shape), (got.cpu() != want).sum().item())
    return want


@pytest.mark.parametrize("F,H,W,pad", PHOTO_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["uint8", "int16", "int64"])
def test_photo_equals_the_restatement(F, H, W, pad, dtype):
    gen = torch.Generator().manual_seed(H * 1000 + W * 10 + pad)
    P = 21
    a = _labels(gen, (F, H, W), dtype, 40)                                # labels >= P: the modulo
    frames = _frames(gen, F, H, W)
    for alpha in (0.5, 0.3):
        want = _check(REF.PHOTO, a, _palette(P), frames=frames, alpha=alpha, pad=pad)
    assert want.shape == (F, 3, H + 2 * pad, 2 * W + 3 * pad)
    # the padding is zero everywhere
    mask = torch.ones_like(want, dtype=torch.bool)
    for k in range(2):
        mask[:, :, pad:pad + H, k * (W + pad) + pad:k * (W + pad) + pad + W] = False
    assert not want[mask].any()
    # normalised frames: denormalize's mean and std
    mean, std = [0.485, 0.456, 0.406], [0.228, 0.224, 0.225]
    _check(REF.PHOTO, a, _palette(256, 1), frames=(frames - 0.4) / 0.25, alpha=0.5, pad=pad, mean=mean, std=std)


@pytest.mark.parametrize("F,H,W,pad", PHOTO_SHAPES[:4])
@pytest.mark.parametrize("dtype", DTYPES, ids=["uint8", "int16", "int64"])
def test_labels_equals_the_restatement(F, H, W, pad, dtype):
    gen = torch.Generator().manual_seed(H * 1000 + W * 10 + pad + 1)
    a, b = _labels(gen, (F, H, W), dtype, 300 if dtype != torch.uint8 else 256), _labels(gen, (F, H, W), dtype, 25)
    for alpha in (0.5, 0.3):
        want = _check(REF.LABELS, a, _palette(21), labels_b=b, alpha=alpha, pad=pad)
    assert want.shape == (F, 3, H + 2 * pad, 3 * W + 4 * pad)
    mask = torch.ones_like(want, dtype=torch.bool)
    for k in range(3):
        mask[:, :, pad:pad + H, k * (W + pad) + pad:k * (W + pad) + pad + W] = False
    assert not want[mask].any()
    got = ops.overlay_grid(ops.OVERLAY_LABELS, a.cuda(), _palette(21), labels_b=b.cuda(), pad=pad).cpu()
    assert not got[mask].any()
    # P = 1: everything is the one colour; P = 256 with the value 255
    _check(REF.LABELS, a, _palette(1, 2), labels_b=b, pad=pad)
    _check(REF.LABELS, a, _palette(256, 3), labels_b=b, pad=pad)


@pytest.mark.parametrize("dtype", DTYPES, ids=["uint8", "int16", "int64"])
def test_maps_of_another_size_are_gathered_through_the_tables(dtype):
    from timetuning_amd.visualization import nearest_tables

    gen = torch.Generator().manual_seed(11)
    F, H, W = 3, 7, 14
    a, b = _labels(gen, (F, 5, 3), dtype, 30), _labels(gen, (F, 5, 3), dtype, 30)
    ytab, xtab = nearest_tables(5, 3, H, W)
    assert ytab.tolist() == [0, 0, 1, 2, 2, 3, 4] and xtab.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2]
    frames = _frames(gen, F, H, W)
    _check(REF.PHOTO, a, _palette(21), frames=frames, ytab=ytab, xtab=xtab)
    _check(REF.LABELS, a, _palette(21), labels_b=b, size=(H, W), ytab=ytab, xtab=xtab)
    rev = (ytab[::-1].copy(), xtab[::-1].copy())                           # any table, not only a monotone one
    _check(REF.LABELS, a, _palette(21), labels_b=b, size=(H, W), ytab=rev[0], xtab=rev[1], pad=0)
    with pytest.raises(ValueError, match="need ytab and xtab"):
        ops.overlay_grid(ops.OVERLAY_PHOTO, a.cuda(), _palette(21), frames=frames.cuda())
    with pytest.raises(ValueError, match=r"entries must lie in \[0, 5\)"):
        ops.overlay_grid(ops.OVERLAY_PHOTO, a.cuda(), _palette(21), frames=frames.cuda(), ytab=ytab + 1, xtab=xtab)


@pytest.mark.parametrize("dtype", DTYPES, ids=["uint8", "int16", "int64"])
def test_shared_and_per_frame_lut_with_values_outside_it(dtype):
    gen = torch.Generator().manual_seed(12)
    F, H, W, L = 3, 7, 14, 9
    a, b = _labels(gen, (F, H, W), dtype, 12), _labels(gen, (F, H, W), dtype, 12)    # 9, 10, 11, 255 (and -1, -7) lie outside [0, L)
    frames = _frames(gen, F, H, W)
    shared = torch.randint(-3, 300, (L,), generator=gen)                           # LUT entries >= P and negative ones: the modulo again
    per_frame = torch.randint(0, 21, (F, L), generator=gen)
    assert not torch.equal(per_frame[0], per_frame[1])
    for lut in (shared, per_frame, per_frame.to(torch.int32), None):
        _check(REF.PHOTO, a, _palette(21), frames=frames, lut=lut)
        want = _check(REF.LABELS, a, _palette(21), labels_b=b, lut=lut)
        # the ground-truth tile never goes through the LUT
        assert torch.equal(want[:, :, 2:2 + H, 2:2 + W], REF.colour(b.long(), _palette(21)))
    with pytest.raises(ValueError, match="lut"):
        ops.overlay_grid(ops.OVERLAY_LABELS, a.cuda(), _palette(21), labels_b=b.cuda(), lut=per_frame[:2])


def test_output_rows_at_every_alignment():
    """F * 3 * OH rows of 34 bytes start at every even offset inside a 16-byte piece; an odd row width covers the odd ones."""
    gen = torch.Generator().manual_seed(13)
    for W in (1, 2, 5, 8, 15, 16, 17, 31):
        for pad in (0, 1, 3):
            a, b = _labels(gen, (2, 3, W), torch.int16, 30), _labels(gen, (2, 3, W), torch.int16, 30)
            _check(REF.LABELS, a, _palette(7), labels_b=b, pad=pad)
            _check(REF.PHOTO, a, _palette(7), frames=_frames(gen, 2, 3, W), pad=pad)


# ---- the histogram ---------------------------------------------------------------------------------------------------------------------

def _hist_ref(maps, R, K):
    return torch.bincount(ops.upsample_argmax_f32(maps, R).flatten(), minlength=K)


# small and full-size shapes (K = 1 among them), one token, down-sampling, the LDS limit, and 336 x 224 x 224 = 16.9 M pixels: more than
# 65536 workgroups of 256, so workgroups make a second round
@pytest.mark.parametrize("M,g,K,R", [(3, 3, 5, 7), (2, 14, 200, 224), (2, 4, 1, 9), (1, 1, 3, 5), (2, 14, 21, 8), (1, 2, 16384, 3), (336, 2, 3, 224)])
def test_histogram_equals_bincount_of_the_labels(M, g, K, R):
    gen = torch.Generator(device="cuda").manual_seed(M * 100 + K)
    maps = torch.randn((M, g * g, K), generator=gen, device="cuda")
    got = ops.upsample_argmax_hist(maps, R)
    assert got.dtype == torch.int64 and got.shape == (K,)
    assert torch.equal(got, _hist_ref(maps, R, K)) and int(got.sum()) == M * R * R


def test_histogram_of_ties_and_constant_maps():
    """Constant maps: every pixel ties on every k, the first maximum is 0, one run per wave.  Scores that take few values: ties between
    prototypes wherever two corners agree, which only the same statement resolves the same way."""
    maps = torch.full((2, 14 * 14, 50), 0.25, device="cuda")
    got = ops.upsample_argmax_hist(maps, 224)
    assert int(got[0]) == 2 * 224 * 224 and not got[1:].any()
    gen = torch.Generator(device="cuda").manual_seed(3)
    coarse = torch.randint(0, 3, (3, 14 * 14, 40), generator=gen, device="cuda").float() / 2
    for R in (224, 37):
        assert torch.equal(ops.upsample_argmax_hist(coarse, R), _hist_ref(coarse, R, 40))


def test_two_accumulating_calls_equal_one_call_on_the_concatenation():
    gen = torch.Generator(device="cuda").manual_seed(4)
    a, b = torch.randn((2, 49, 30), generator=gen, device="cuda"), torch.randn((3, 49, 30), generator=gen, device="cuda")
    counts = ops.upsample_argmax_hist(a, 56)
    first = counts.clone()
    assert ops.upsample_argmax_hist(b, 56, counts) is counts
    assert torch.equal(counts, ops.upsample_argmax_hist(torch.cat([a, b]), 56)) and torch.equal(counts - first, _hist_ref(b, 56, 30))
    with pytest.raises(ValueError, match="counts"):
        ops.upsample_argmax_hist(a, 56, torch.zeros(31, dtype=torch.int64, device="cuda"))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------

def _clips(bs=2, fs=3, R=16, k=5, seed=3):
    rng = np.random.default_rng(seed)
    gts = np.kron(rng.integers(0, 4, (bs, fs, 4, 4)), np.ones((R // 4, R // 4), np.int64))
    preds = np.where(rng.random(gts.shape) < 0.7, (gts + 1) % k, rng.integers(0, k, gts.shape)).astype(np.int16)
    for i in range(bs):
        for j in range(1, fs):   # distinct consecutive frames: Pillow merges equal ones
            assert not np.array_equal(gts[i, j], gts[i, j - 1]) and not np.array_equal(preds[i, j], preds[i, j - 1])
    return torch.from_numpy(gts).cuda(), torch.from_numpy(preds).cuda()


@pytest.mark.parametrize("protocol", ["frame-wise", "sample-wise"])
def test_evaluate_localizations_logs_gifs_and_returns_the_same_score(tmp_path, protocol):
    from PIL import Image

    from timetuning_amd.evaluation import evaluate_localizations
    from timetuning_amd.metrics import PredsmIoU
    from timetuning_amd.visualization import voc_palette

    gts, preds = _clips()
    bs, fs, R = 2, 3, 16
    plain = evaluate_localizations(PredsmIoU(5, 5), gts, preds, protocol)
    assert evaluate_localizations(PredsmIoU(5, 5), gts, preds, protocol, str(tmp_path)) == plain
    sub = tmp_path / protocol
    names = sorted(os.listdir(sub))
    assert len(names) == 4 and sum("Reordered" in n for n in names) == 2 and sum("Inorder" in n for n in names) == 2
    S = bs * fs if protocol == "frame-wise" else bs
    segs = PredsmIoU(5, 5).compute_segments(gts.reshape(S, -1), preds.reshape(S, -1), with_mapping=True)
    pal = torch.from_numpy(voc_palette())
    for name in names:
        i = int(name[:-4].rsplit("_", 1)[1])
        assert name.startswith("Score:" if protocol == "frame-wise" else "Score-") and f"_Evaluation_{protocol}_" in name
        with Image.open(sub / name) as im:
            assert im.n_frames == fs and im.size == (3 * R + 8, R + 4)
            for j in range(fs):
                im.seek(j)
                frame = torch.from_numpy(np.asarray(im.convert("RGB")).copy())
                p = preds[i, j].long().cpu()
                if "Reordered" in name:
                    p = segs[(i * fs + j) if protocol == "frame-wise" else i][4][p]
                assert torch.equal(frame[2:2 + R, R + 4:2 * R + 4], pal[p]), (name, j)      # the prediction panel = palette[lut[pred]]
                assert torch.equal(frame[2:2 + R, 2:2 + R], pal[gts[i, j].cpu()]), (name, j)
    assert evaluate_localizations(PredsmIoU(5, 5), gts, preds, "dataset-wise", str(tmp_path)) == \
        evaluate_localizations(PredsmIoU(5, 5), gts, preds, "dataset-wise")
    assert not (tmp_path / "dataset-wise").exists()


@pytest.fixture(scope="module")
def tiny_model():
    from timetuning_amd import synth
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    K = 20
    fe = FeatureExtractor("dino-s16", "", [128, 128, 64, 32], unfreeze_layers=["blocks.11", "blocks.10"], vit_cfg=synth.ARCHS["tiny-s16"],
                          init="stress", return_attention=False)
    model = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, fe.feature_dim))).cuda()
    clips = torch.from_numpy(synth.make_clips(2, 2, 224, seed=1))
    return model, clips


def test_similarity_histogram_equals_the_bincount_of_proto_clustering(tiny_model):
    from timetuning_amd.clustering import proto_clustering
    from timetuning_amd.time_tuning import assignment_entropy, get_similarity_histogram

    model, clips = tiny_model
    model.train()
    loader = [(clips[:1].unsqueeze(1), None, None), (clips[1:].unsqueeze(1), None, None)]      # two batches: the counts add up
    hist = get_similarity_histogram(model, loader)
    assert model.training                                                                   # left as it was
    assert hist.dtype == torch.int64 and hist.shape == (20,) and int(hist.sum()) == 4 * 224 * 224
    model.eval()
    feats, _ = model(clips.cuda().view(4, 3, 224, 224))
    maps = proto_clustering(feats, model.prototypes)
    assert maps.shape == (4, 224, 224)
    assert torch.equal(hist, torch.bincount(maps.flatten(), minlength=20))
    small = get_similarity_histogram(model, loader, output_size=56)
    assert torch.equal(small, torch.bincount(proto_clustering(feats, model.prototypes, output_size=56).flatten(), minlength=20))
    assert 0.0 <= assignment_entropy(hist) <= np.log(20) / 20 + 1e-9


def test_log_clip_localization_writes_one_overlay_gif_per_clip(tiny_model, tmp_path):
    from PIL import Image

    from timetuning_amd.time_tuning import log_clip_localization

    model, clips = tiny_model
    model.eval()
    paths = log_clip_localization(model, clips, False, "frame-wise", str(tmp_path / "vis"), 4, 32)
    assert paths == [f"{tmp_path}/vis/4_0.gif", f"{tmp_path}/vis/4_1.gif"]
    for path in paths:
        with Image.open(path) as im:
            assert im.size == (2 * 224 + 6, 224 + 4) and im.n_frames >= 1 and im.info["loop"] == 0


def test_evaluation_command_line_logs_videos_only_when_asked(tmp_path):
    from PIL import Image

    from timetuning_amd import evaluation as E
    from timetuning_amd import synth

    argv = ["--dataset", "synthetic", "--model_path", "", "--eval_clips", "3", "--batch_size", "2", "--num_frames", "3", "--input_resolution", "64",
            "--num_clusters", "4", "--evaluation_protocol", "sample-wise", "--logging_directory", str(tmp_path / "vis")]
    plain = E.main(argv, vit_cfg=synth.ARCHS["tiny-s16"])
    assert not (tmp_path / "vis").exists()
    assert E.main(argv + ["--log_videos"], vit_cfg=synth.ARCHS["tiny-s16"]) == plain
    names = sorted(os.listdir(tmp_path / "vis" / "sample-wise"))
    # three clips in two batches, numbered over the whole loader
    assert sorted(n[:-4].rsplit("_", 2)[1:] for n in names) == sorted([k, str(i)] for i in range(3) for k in ("Inorder", "Reordered")), names
    with Image.open(tmp_path / "vis" / "sample-wise" / names[0]) as im:
        assert im.size == (3 * 64 + 8, 64 + 4) and im.info["duration"] == 80


def test_training_driver_logs_the_histogram_and_the_overlay_gifs(tmp_path, capsys):
    from timetuning_amd.time_tuning import build_parser, time_tuning

    args = build_parser().parse_args(["--dataset", "synthetic", "--model_path", "", "--batch_size", "2", "--num_frames", "2", "--num_clusters", "20",
                                      "--num_epochs", "1", "--steps_per_epoch", "1", "--eval_clips", "2", "--logging_directory", str(tmp_path / "logs"),
                                      "--visualization_directory", str(tmp_path / "vis"), "--log_localization_every", "1",
                                      "--evaluation_protocol", "frame-wise"])
    before = ops.get_gemm_precision()
    try:
        time_tuning(0, args)
    finally:
        ops.set_gemm_precision(before)            # the driver switches the process to its own default, "f16x3"
    out = capsys.readouterr().out
    assert "Scores/entropy" in out and "unassigned prototypes" in out
    assert sorted(os.listdir(tmp_path / "vis")) == ["0_0.gif", "0_1.gif"]                # one per clip of the first evaluation batch
