"""Host-side checks of the Pascal VOC reader (N22): the descriptor table and pool of the ragged kernels against Pillow through a NumPy
restatement, the launchers' validation through the C ABI (it returns before any launch, so no GPU is needed), the shape rule, the dataset's
layout and errors, the crop box against torchvision's rule, and the command lines."""
import ctypes as C
import math
import os
import random

import numpy as np
import pytest

import _voc_ref as R
from timetuning_amd import _lib, hip_ops as ops, leoloader as L
from timetuning_amd.video_transformations import resample_coeffs

TT_EINVAL = -1
FAKE_DEV = 4096    # a non-null "device pointer": every call below is refused before anything could read it


# ---- the NumPy restatement over the front end's table and pool equals Pillow ----------------------------------------------------------

@pytest.mark.parametrize("S", R.TARGETS)
def test_resize_table_and_pool_equal_pillow(S):
    imgs = [R.image(h, w, k) for k, (h, w) in enumerate(R.SOURCES)]
    buf, offs = R.pack(imgs)
    assert any(o % 2 == 1 for o in offs)                     # odd W * 3: later items start at odd byte offsets
    table, pool = ops.img_resize_ragged_plan(R.SOURCES, offs, S)
    got = R.numpy_resize_ragged(buf, table, pool, S, S)
    for i, img in enumerate(imgs):
        want = R.pillow_resize(img, S)
        assert np.array_equal(got[i], want), (R.SOURCES[i], S)
    # one copy of the taps per (in, out) length: 5 x 7 and 7 x 5 share theirs
    lengths = {n for hw in R.SOURCES for n in hw if n != S}
    assert pool.size == sum(resample_coeffs(n, S)[0].numel() + 2 * S for n in lengths)


@pytest.mark.parametrize("flip", [False, True])
def test_crop_and_flip_equal_pillow(flip):
    (h, w), box, S = R.BOX_CASE
    img = R.image(h, w, 77)
    table, pool = ops.img_resize_ragged_plan([(h, w)], [0], S, [box], [flip])
    got = R.numpy_resize_ragged(img.reshape(-1), table, pool, S, S)[0]
    assert np.array_equal(got, R.pillow_resize(img, S, box, flip))


@pytest.mark.parametrize("Rm", R.MASK_TARGETS)
def test_mask_table_and_pool_equal_pillow(Rm):
    masks = [R.mask(h, w, k) for k, (h, w) in enumerate(R.SOURCES)]
    assert {int(v) for m in masks[4:] for v in np.unique(m)} >= set(range(22)) | {255}
    buf, offs = R.pack(masks)
    table, pool = ops.img_gather_nearest_ragged_plan(R.SOURCES, offs, Rm)
    got = R.numpy_gather_ragged(buf, table, pool, Rm, Rm)
    for i, m in enumerate(masks):
        assert np.array_equal(got[i], R.pillow_mask_resize(m, Rm)), (R.SOURCES[i], Rm)
    (h, w), box, S = R.BOX_CASE
    m = R.mask(h, w, 5)
    for flip in (False, True):
        table, pool = ops.img_gather_nearest_ragged_plan([(h, w)], [0], S, [box], [flip])
        assert np.array_equal(R.numpy_gather_ragged(m.reshape(-1), table, pool, S, S)[0], R.pillow_mask_resize(m, S, box, flip))


def test_to_tensor_normalize_is_the_fp32_chain():
    u8 = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    x = R.to_tensor_normalize(u8)
    assert x.dtype == np.float32 and x.shape == (3, 16, 16)
    for c in range(3):
        want = (np.arange(256, dtype=np.float32) / np.float32(255) - np.float32(R.MEAN[c])) / np.float32(R.STD[c])
        assert np.array_equal(x[c].reshape(-1), want)


# ---- validation through the C ABI ---------------------------------------------------------------------------------------------------

def _resize_call(table, pool, in_bytes, OH, OW, n=None):
    lib = _lib.load()
    table = np.ascontiguousarray(table, np.int64)
    pool = np.ascontiguousarray(pool, np.int32)
    return lib.tt_img_resize_ragged(FAKE_DEV, in_bytes, table.ctypes.data, FAKE_DEV, len(table) if n is None else n, pool.ctypes.data, FAKE_DEV,
                                    pool.size, FAKE_DEV, None, OH, OW, None, None, None)


def _gather_call(table, pool, in_bytes, OH, OW):
    lib = _lib.load()
    table = np.ascontiguousarray(table, np.int64)
    pool = np.ascontiguousarray(pool, np.int32)
    return lib.tt_img_gather_nearest_ragged(FAKE_DEV, in_bytes, table.ctypes.data, FAKE_DEV, len(table), pool.ctypes.data, FAKE_DEV, pool.size,
                                            FAKE_DEV, None, OH, OW, None)


def _good_resize():
    dims = [(37, 53), (5, 7)]
    offs = [0, 37 * 53 * 3]
    table, pool = ops.img_resize_ragged_plan(dims, offs, 16, [(3, 2, 20, 11), None])
    return table, pool, 37 * 53 * 3 + 5 * 7 * 3


def _resize_mutations():
    def offset_past(t, p, nb):
        t[1, R.SRC] += 1

    def zero_size(t, p, nb):
        t[0, R.BW] = 0

    def zero_image(t, p, nb):
        t[1, R.H] = 0

    def box_outside(t, p, nb):
        t[0, R.X0] = 53 - 19

    def box_negative(t, p, nb):
        t[0, R.Y0] = -1

    def bound_outside(t, p, nb):
        p[t[0, R.HB] + 2 * 15] += 1              # the last column's first tap + cnt now ends one past the box

    def bound_negative(t, p, nb):
        p[t[0, R.VB]] = -1

    def count_past_ksize(t, p, nb):
        t[0, R.VKS] = 1

    def pool_past(t, p, nb):
        t[1, R.VK] = p.size - 3

    def pool_negative(t, p, nb):
        t[1, R.HB] = -2

    def bad_flip(t, p, nb):
        t[0, R.FLIP] = 2

    return [offset_past, zero_size, zero_image, box_outside, box_negative, bound_outside, bound_negative, count_past_ksize, pool_past,
            pool_negative, bad_flip]


@pytest.mark.parametrize("mutate", _resize_mutations(), ids=lambda f: f.__name__)
def test_resize_validation_refuses(mutate):
    table, pool, nbytes = _good_resize()
    table, pool = table.copy(), pool.copy()
    mutate(table, pool, nbytes)
    assert _resize_call(table, pool, nbytes, 16, 16) == TT_EINVAL
    assert b"img_resize_ragged" in _lib.load().tt_last_error()


def test_resize_validation_sizes_and_shape_rule():
    table, pool, nbytes = _good_resize()
    assert _resize_call(table, pool, nbytes, 0, 16) == TT_EINVAL
    assert _resize_call(table, pool, nbytes, 16, 40000) == TT_EINVAL
    assert _resize_call(table, pool, nbytes, 16, 16, n=0) == TT_EINVAL
    assert _resize_call(table, pool, nbytes - 1, 16, 16) == TT_EINVAL       # the last image ends one byte past the buffer
    # an item beyond shape_ok: 1400 x 3 -> 16 x 16 needs all 1400 rows x 48 bytes for its one band
    assert not ops.img_resize_ragged_shape_ok(1400, 3, 16, 16)
    table, pool = ops.img_resize_ragged_plan([(1400, 3)], [0], 16)
    assert _resize_call(table, pool, 1400 * 3 * 3, 16, 16) == TT_EINVAL
    assert b"LDS" in _lib.load().tt_last_error()


def _good_gather():
    dims = [(37, 53), (5, 7)]
    offs = [0, 37 * 53]
    table, pool = ops.img_gather_nearest_ragged_plan(dims, offs, 9, [(3, 2, 20, 11), None], [True, False])
    return table, pool, 37 * 53 + 5 * 7


def _gather_mutations():
    def offset_past(t, p, nb):
        t[1, R.SRC] += 1

    def zero_size(t, p, nb):
        t[1, R.BH] = 0

    def box_outside(t, p, nb):
        t[0, R.Y0] = 37 - 10

    def ytab_outside(t, p, nb):
        p[t[1, R.YT] + 8] = 5

    def xtab_negative(t, p, nb):
        p[t[0, R.XT]] = -1

    def pool_past(t, p, nb):
        t[0, R.XT] = p.size - 8

    return [offset_past, zero_size, box_outside, ytab_outside, xtab_negative, pool_past]


@pytest.mark.parametrize("mutate", _gather_mutations(), ids=lambda f: f.__name__)
def test_gather_validation_refuses(mutate):
    table, pool, nbytes = _good_gather()
    table, pool = table.copy(), pool.copy()
    mutate(table, pool, nbytes)
    assert _gather_call(table, pool, nbytes, 9, 9) == TT_EINVAL
    assert b"img_gather_nearest_ragged" in _lib.load().tt_last_error()
    assert _gather_call(*_good_gather()[:2], nbytes, 0, 9) == TT_EINVAL
    assert _gather_call(*_good_gather()[:2], nbytes, 9, 32768) == TT_EINVAL


# ---- the shape rule -----------------------------------------------------------------------------------------------------------------

def _lds_rule(h, w, OH, OW):
    """The rule in Python: the source rows a band of 16 output rows reaches (from the first row's first tap to the last row's last), at
    OW x 3 bytes each; an equal-length vertical pass reads the band's own rows."""
    rows = 0
    bounds = None if h == OH else resample_coeffs(h, OH)[1].numpy()
    for y0 in range(0, OH, ops.IMG_RAGGED_BAND):
        y1 = min(y0 + ops.IMG_RAGGED_BAND, OH)
        rows = max(rows, y1 - y0 if bounds is None else int(bounds[y1 - 1, 0] + bounds[y1 - 1, 1] - bounds[y0, 0]))
    return rows * OW * 3


def test_shape_ok_agrees_with_the_rule():
    lib = _lib.load()
    sides = [1, 2, 3, 15, 16, 17, 100, 333, 375, 448, 500, 1365, 1366, 1400, 4000, 32767]
    outs = [1, 4, 16, 17, 33, 112, 224, 448, 1024]
    seen = set()
    for h in sides:
        for OH in outs:
            for w, OW in ((3, 4), (500, 448), (4000, 1024), (h, OH)):
                need = _lds_rule(h, w, OH, OW)
                assert lib.tt_img_resize_ragged_lds_bytes(h, w, OH, OW) == need, (h, w, OH, OW)
                ok = need <= ops.IMG_RAGGED_LDS_BUDGET
                assert ops.img_resize_ragged_shape_ok(h, w, OH, OW) == ok, (h, w, OH, OW)
                seen.add(ok)
    assert seen == {True, False}
    for bad in ((0, 5, 4, 4), (5, 0, 4, 4), (5, 5, 0, 4), (5, 5, 4, 32768), (32768, 5, 4, 4)):
        assert not ops.img_resize_ragged_shape_ok(*bad)
    # the workload: every VOC size to 448 fits, with room for more than two workgroups per CU
    for h, w in ((375, 500), (500, 375), (333, 500), (500, 500), (112, 500)):
        assert lib.tt_img_resize_ragged_lds_bytes(h, w, 448, 448) <= ops.IMG_RAGGED_LDS_BUDGET // 2


# ---- VOCDataset -----------------------------------------------------------------------------------------------------------------------

def test_voc_dataset_layout_errors_and_order(tmp_path):
    root = str(tmp_path / "VOCSegmentation")
    names = R.make_voc_tree(root)
    with open(os.path.join(root, "sets", "train.txt"), "w") as f:
        f.write("\n".join(reversed(names[:3])) + "\n")
    for split, folder in (("trainaug", "SegmentationClassAug"), ("train", "SegmentationClassAug"), ("val", "SegmentationClass")):
        ds = L.VOCDataset(root, split)
        want = list(reversed(names[:3])) if split == "train" else names
        assert ds.images == [os.path.join(root, "images", n + ".jpg") for n in want]
        assert ds.masks == [os.path.join(root, folder, n + ".png") for n in want]
        assert len(ds) == len(want)
    with pytest.raises(ValueError, match="No support for image set test"):
        L.VOCDataset(root, "test")
    with pytest.raises(RuntimeError, match="Dataset not found or corrupted."):
        L.VOCDataset(str(tmp_path / "nowhere"), "val")
    os.rename(os.path.join(root, "SegmentationClass"), os.path.join(root, "moved"))
    with pytest.raises(RuntimeError, match="Dataset not found or corrupted."):
        L.VOCDataset(root, "val")
    L.VOCDataset(root, "trainaug")                      # the other folder is still there
    os.rename(os.path.join(root, "moved"), os.path.join(root, "SegmentationClass"))
    os.remove(os.path.join(root, "images", names[3] + ".jpg"))
    os.remove(os.path.join(root, "images", names[4] + ".jpg"))
    with pytest.raises(FileNotFoundError, match=names[3] + ".jpg"):
        L.VOCDataset(root, "val")
    os.remove(os.path.join(root, "SegmentationClass", names[1] + ".png"))
    with pytest.raises(FileNotFoundError, match=names[1] + ".png"):    # the masks are looked at first, as in the reference's assert
        L.VOCDataset(root, "val")


def test_pascal_loader_length(tmp_path):
    root = str(tmp_path / "VOCSegmentation")
    R.make_voc_tree(root)
    for b, want in ((1, 5), (2, 3), (4, 2), (5, 1), (60, 1)):
        loader = L.pascal_loader(b, root, "val", 9, train_size=16)
        assert len(loader) == want
        assert loader.train_size == 16 and loader.val_size == 9 and loader.transforms is None
    assert len(L.CLASS_IDX_TO_NAME) == 21 and L.CLASS_IDX_TO_NAME[0] == "background" and L.CLASS_IDX_TO_NAME[15] == "person"


# ---- the pair transforms --------------------------------------------------------------------------------------------------------------

def _torchvision_get_params(height, width, scale, ratio, rng):
    """torchvision.transforms.RandomResizedCrop.get_params, its torch draws replaced by the same draws from ``rng``."""
    area = height * width
    log_ratio = [math.log(r) for r in ratio]
    for _ in range(10):
        target_area = area * rng.uniform(scale[0], scale[1])
        aspect_ratio = math.exp(rng.uniform(log_ratio[0], log_ratio[1]))
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= width and 0 < h <= height:
            i = rng.randint(0, height - h)
            j = rng.randint(0, width - w)
            return i, j, h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w = width
        h = height
    return (height - h) // 2, (width - w) // 2, h, w


def test_random_resized_crop_box_follows_torchvision():
    dims = [(375, 500), (500, 375), (333, 500), (20, 300), (300, 20), (1, 1)]
    chain = L.train_transforms(448)
    plan = chain(dims, random.Random(1234))
    ref = random.Random(1234)
    boxes = []
    for H, W in dims:
        i, j, h, w = _torchvision_get_params(H, W, (0.8, 1.0), (3. / 4., 4. / 3.), ref)
        boxes.append((j, i, w, h))
    flips = [ref.random() < 0.5 for _ in dims]
    assert plan.boxes == boxes and plan.flips == flips
    assert plan.size == (448, 448) and plan.to_tensor and plan.mean_std == (L.MEAN, L.STD)
    assert True in flips and False in flips
    for (x0, y0, w, h), (H, W) in zip(plan.boxes, dims):
        assert 0 <= x0 and 0 <= y0 and x0 + w <= W and y0 + h <= H and w >= 1 and h >= 1
    # the fall-back of the rule (no try fits): the central crop at the nearest allowed ratio
    assert L.RandomResizedCrop.get_params(20, 300, (0.8, 1.0), (3. / 4., 4. / 3.), random.Random(0)) == (0, 136, 20, 27)
    with pytest.raises(ValueError):
        L.Compose([L.Normalize(L.MEAN, L.STD)])(dims, random.Random(0))


# ---- the command lines ----------------------------------------------------------------------------------------------------------------

def test_parsers_route_voc_and_keep_the_old_refusals(tmp_path):
    from timetuning_amd import cluster_based_foreground_extraction as CB, evaluation as EV, linear_finetune as LF, time_tuning as TT

    missing = str(tmp_path / "no_such_root")
    for main in (LF.main, CB.main, EV.main):
        with pytest.raises(RuntimeError, match="Dataset not found or corrupted."):
            main(["--dataset", "voc", "--dataset_path", missing])
    with pytest.raises(NotImplementedError, match="--dataset voc"):
        LF.main(["--dataset", "pascal"])
    with pytest.raises(NotImplementedError, match="--dataset voc"):
        EV.main(["--dataset", "davis_val"])
    with pytest.raises(NotImplementedError, match="--dataset voc"):
        CB.main(["--dataset", "davis"])
    assert LF.build_parser().parse_args([]).dataset == "pascal"
    assert EV.build_parser().parse_args([]).dataset == "davis_val"
    assert TT.build_parser().parse_args([]).eval_dataset_path == ""
    assert TT.build_parser().parse_args(["--eval_dataset_path", "/data/VOCSegmentation"]).eval_dataset_path == "/data/VOCSegmentation"
