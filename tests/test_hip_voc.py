"""GPU checks of the Pascal VOC reader (N22): the two ragged kernels and ``pascal_loader`` against Pillow, bit for bit (``torch.equal``):
the arithmetic is integer up to one correctly rounded division and subtraction, so no tolerance is needed.

Figures of the mutation sweep are in DESIGN.md (N22)."""
import functools
import os

import numpy as np
import pytest
import torch

import _voc_ref as R
from timetuning_amd import hip_ops as ops, leoloader as L

pytestmark = pytest.mark.gpu

GUARD = 256


@functools.lru_cache(maxsize=None)
def _images():
    return [R.image(h, w, k) for k, (h, w) in enumerate(R.SOURCES)]


@functools.lru_cache(maxsize=None)
def _masks():
    return [R.mask(h, w, k) for k, (h, w) in enumerate(R.SOURCES)]


@functools.lru_cache(maxsize=None)
def _pillow(S):
    return [R.pillow_resize(img, S) for img in _images()]


def _views(arrays):
    """The arrays packed back to back in ONE device buffer, as views of it: odd row lengths put the later items at odd byte offsets."""
    buf, offs = R.pack(arrays)
    dev = torch.from_numpy(buf).cuda()
    return [dev[o:o + a.size].view(*a.shape) for a, o in zip(arrays, offs)], offs


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    flat = torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")
    return flat, flat[:n].view(*shape)


def _resize_checked(frames, size, want_u8, boxes=None, flips=None):
    """One call per output form into sentinel-filled buffers with a guard behind them: every element written, nothing beyond."""
    n = len(frames)
    OH, OW = (size, size) if isinstance(size, int) else size
    want = torch.from_numpy(np.stack(want_u8)).cuda()
    for fill in (0x5A, 0xA5):        # an element left unwritten differs from Pillow under at least one of the two fills
        flat, out = _guarded((n, OH, OW, 3), torch.uint8, fill)
        got = ops.img_resize_ragged(frames, size, boxes, flips, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(got, want)
        assert bool((flat[-GUARD:] == fill).all())
    flat, out = _guarded((n, 3, OH, OW), torch.float32, float("nan"))
    got = ops.img_resize_ragged(frames, size, boxes, flips, to_tensor=(R.MEAN, R.STD), out=out)
    want_f = torch.from_numpy(np.stack([R.to_tensor_normalize(w) for w in want_u8])).cuda()
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got, want_f)
    assert bool(torch.isnan(flat[-GUARD:]).all())


@pytest.mark.parametrize("S", R.TARGETS)
def test_bilinear_grid_mixed_batch_and_alone(S):
    """Ten sizes in ONE call.  The grid holds a skipped horizontal pass (5 x 7 -> 7), a skipped vertical one (7 x 5 -> 7), both (23 -> 23),
    ksize 3 up-scaling, ksize >= 7 down-scaling (200 -> 33 and smaller), output heights that are no multiple of the band of 16 (1, 4, 7,
    23, 33), bands whose rows touch the first and the last image row, and odd byte offsets."""
    frames, offs = _views(_images())
    assert any(o % 2 for o in offs)
    _resize_checked(frames, S, _pillow(S))
    for i, f in enumerate(frames):
        got = ops.img_resize_ragged([f], S)
        assert torch.equal(got[0].cpu(), torch.from_numpy(_pillow(S)[i])), (R.SOURCES[i], S)
        got = ops.img_resize_ragged([f], S, to_tensor=(R.MEAN, R.STD))
        assert torch.equal(got[0].cpu(), torch.from_numpy(R.to_tensor_normalize(_pillow(S)[i]))), (R.SOURCES[i], S)


def test_rectangular_output():
    frames, _ = _views(_images())
    size = (19, 40)
    _resize_checked(frames, size, [R.pillow_resize(img, size) for img in _images()])


def test_crop_and_flip():
    (h, w), box, S = R.BOX_CASE
    img = R.image(h, w, 77)
    frames, _ = _views([img])
    for flip in (False, True):
        _resize_checked(frames, S, [R.pillow_resize(img, S, box, flip)], [box], [flip])
    # flips on a subset of the items of one call, a box on one of them
    frames, _ = _views(_images())
    flips = [i % 3 == 1 for i in range(len(frames))]
    boxes = [None] * len(frames)
    boxes[4] = box
    want = [R.pillow_resize(img, 16, b, f) for img, b, f in zip(_images(), boxes, flips)]
    _resize_checked(frames, 16, want, boxes, flips)


def test_workload_geometry():
    dims = [(375, 500), (500, 375), (333, 500)]
    imgs = [R.image(h, w, 30 + k) for k, (h, w) in enumerate(dims)]
    frames, _ = _views(imgs)
    got = ops.img_resize_ragged(frames, 448, to_tensor=(R.MEAN, R.STD))
    want = np.stack([R.to_tensor_normalize(R.pillow_resize(img, 448)) for img in imgs])
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    masks = [R.mask(h, w, 40 + k) for k, (h, w) in enumerate(dims)]
    maps, _ = _views(masks)
    got = ops.img_gather_nearest_ragged(maps, 100, to_tensor=True)
    want = np.stack([(R.pillow_mask_resize(m, 100).astype(np.float32) / np.float32(255))[None] for m in masks])
    assert torch.equal(got.cpu(), torch.from_numpy(want))


def test_fallback_route_inside_a_mixed_batch():
    """1366 x 1 -> 16 x 16 is the smallest item the rule refuses at S = 16 (one band reaches all 1366 rows x 48 bytes = 65568 > 65536);
    1365 x 1 is the largest it takes, at 65520 bytes of LDS.  Both sit in one batch with ordinary items; the refused one goes through
    ``resized_crop`` into its row of the same output."""
    assert not ops.img_resize_ragged_shape_ok(1366, 1, 16, 16) and ops.img_resize_ragged_shape_ok(1365, 1, 16, 16)
    dims = [(5, 7), (1366, 1), (37, 53), (1365, 1)]
    imgs = [R.image(h, w, 90 + k) for k, (h, w) in enumerate(dims)]
    frames, _ = _views(imgs)
    flips = [False, True, True, False]
    _resize_checked(frames, 16, [R.pillow_resize(img, 16, None, f) for img, f in zip(imgs, flips)], None, flips)
    # the same items from storages of their own: packed with one torch.cat, same result
    own = [torch.from_numpy(img).cuda() for img in imgs]
    _resize_checked(own, 16, [R.pillow_resize(img, 16) for img in imgs])


@pytest.mark.parametrize("Rm", R.MASK_TARGETS)
def test_mask_grid_mixed_batch(Rm):
    maps, offs = _views(_masks())
    assert any(o % 2 for o in offs)
    want = np.stack([R.pillow_mask_resize(m, Rm) for m in _masks()])
    for fill in (0x5A, 0xA5):
        flat, out = _guarded((len(maps), Rm, Rm), torch.uint8, fill)
        got = ops.img_gather_nearest_ragged(maps, Rm, out=out)
        assert torch.equal(got.cpu(), torch.from_numpy(want))
        assert bool((flat[-GUARD:] == fill).all())
    flat, out = _guarded((len(maps), 1, Rm, Rm), torch.float32, float("nan"))
    got = ops.img_gather_nearest_ragged(maps, Rm, to_tensor=True, out=out)
    assert torch.equal(got.cpu(), torch.from_numpy(want.astype(np.float32) / np.float32(255))[:, None])
    assert bool(torch.isnan(flat[-GUARD:]).all())
    # crop and flip fold into the tables
    (h, w), box, S = R.BOX_CASE
    m = R.mask(h, w, 5)
    maps, _ = _views([m, m])
    got = ops.img_gather_nearest_ragged(maps, S, [box, box], [False, True])
    assert np.array_equal(got[0].cpu().numpy(), R.pillow_mask_resize(m, S, box, False))
    assert np.array_equal(got[1].cpu().numpy(), R.pillow_mask_resize(m, S, box, True))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def voc_tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("voc") / "VOCSegmentation")
    return root, R.make_voc_tree(root)


def test_pascal_loader_equals_the_pillow_chain(voc_tree):
    root, names = voc_tree
    per_split = {}
    for split, folder in (("val", "SegmentationClass"), ("trainaug", "SegmentationClassAug")):
        loader = L.pascal_loader(2, root, split, 9, train_size=16)
        batches = list(loader)
        assert len(loader) == 3 and [b[0].shape[0] for b in batches] == [2, 2, 1]
        assert loader.fallback_frames == 1                      # the progressive file
        k = 0
        for x, y in batches:
            assert x.is_cuda and y.is_cuda and x.dtype == torch.float32 and y.dtype == torch.float32
            assert x.shape[1:] == (3, 16, 16) and y.shape[1:] == (1, 9, 9)
            labels = (y * 255).long()
            for i in range(x.shape[0]):
                wx, wy, idx = R.voc_reference(root, names[k], folder, 16, 9)
                assert torch.equal(x[i].cpu(), torch.from_numpy(wx)), names[k]
                assert torch.equal(y[i].cpu(), torch.from_numpy(wy)), names[k]
                assert torch.equal(labels[i, 0].cpu(), torch.from_numpy(idx.astype(np.int64))), names[k]
                k += 1
        assert k == len(names)
        per_split[split] = (torch.cat([b[0] for b in batches]), torch.cat([b[1] for b in batches]))
    assert torch.equal(per_split["val"][0], per_split["trainaug"][0]) and torch.equal(per_split["val"][1], per_split["trainaug"][1])
    # a second pass over the same loader, without the background thread: the same batches
    loader = L.VOCLoader(L.VOCDataset(root, "val"), 2, 9, 16, prefetch=False)
    assert torch.equal(torch.cat([x for x, _ in loader]), per_split["val"][0])
    assert 255 in (per_split["val"][1] * 255).long().unique().tolist()


def test_pair_transforms_through_the_loader(voc_tree):
    import random
    from PIL import Image

    root, names = voc_tree
    chain = L.Compose([L.RandomResizedCrop(size=12, scale=(0.5, 1.)), L.RandomHorizontalFlip(p=0.5), L.ToTensor(), L.Normalize(L.MEAN, L.STD)])
    loader = L.VOCLoader(L.VOCDataset(root, "val"), 5, 9, 16, transforms=chain, rng=random.Random(3))
    (x, y), = list(loader)
    dims = [Image.open(os.path.join(root, "images", n + ".jpg")).size[::-1] for n in names]
    plan = chain(dims, random.Random(3))
    assert True in plan.flips and False in plan.flips
    for i, n in enumerate(names):
        img = np.asarray(Image.open(os.path.join(root, "images", n + ".jpg")).convert("RGB"))
        m = np.asarray(Image.open(os.path.join(root, "SegmentationClass", n + ".png")))
        assert torch.equal(x[i].cpu(), torch.from_numpy(R.to_tensor_normalize(R.pillow_resize(img, 12, plan.boxes[i], plan.flips[i]))))
        wy = R.pillow_mask_resize(m, 12, plan.boxes[i], plan.flips[i]).astype(np.float32) / np.float32(255)
        assert torch.equal(y[i, 0].cpu(), torch.from_numpy(wy))


def test_command_lines_read_the_tree(voc_tree, tmp_path):
    from timetuning_amd import evaluation as E, linear_finetune as LF, synth

    root, _ = voc_tree
    miou = LF.main(["--dataset", "voc", "--dataset_path", root, "--model_path", "", "--input_resolution", "64", "--mask_size", "32",
                    "--batch_size", "2", "--epochs", "1", "--num_prototypes", "10", "--head_layers", "64", "32", "--save_path", ""])
    assert np.isfinite(miou) and 0.0 <= miou <= 1.0
    score = E.main(["--dataset", "voc", "--dataset_path", root, "--model_path", "", "--batch_size", "2", "--input_resolution", "64",
                    "--num_clusters", "4", "--evaluation_protocol", "dataset-wise"], vit_cfg=synth.ARCHS["tiny-s16"])
    assert np.isfinite(score) and 0.0 <= score <= 1.0


def test_foreground_extraction_reads_the_tree(voc_tree):
    from timetuning_amd import cluster_based_foreground_extraction as CB

    root, _ = voc_tree
    score = CB.main(["--dataset", "voc", "--dataset_path", root, "--model_path", "", "--input_resolution", "224", "--k_fg_extraction", "20",
                     "--batch_size", "4"])
    assert np.isfinite(score) and 0.0 <= score <= 1.0


def test_training_driver_evaluates_on_the_tree(voc_tree, tmp_path, capsys):
    from timetuning_amd.time_tuning import build_parser, time_tuning

    root, _ = voc_tree
    args = build_parser().parse_args(["--dataset", "synthetic", "--model_path", "", "--batch_size", "2", "--num_frames", "2", "--num_clusters", "20",
                                      "--num_epochs", "1", "--steps_per_epoch", "1", "--logging_directory", str(tmp_path / "logs"),
                                      "--evaluation_protocol", "dataset-wise", "--eval_dataset_path", root])
    before = ops.get_gemm_precision()
    try:
        time_tuning(0, args)
    finally:
        ops.set_gemm_precision(before)            # the driver switches the process to its own default, "f16x3"
    assert "Scores/localization" in capsys.readouterr().out
