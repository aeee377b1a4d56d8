"""N11 without a GPU: the host side of the annotation pipeline - index tables and their folding, the random draws of the new
classes in the reference's order, the errors the reference raises, the factories and ``read_batch``'s uint8 round trip."""
import os
import random
import sys

import numpy as np
import pytest
import torch

from timetuning_amd import mask_propagation as MP
from timetuning_amd import video_transformations as VT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nearest_ops as NO  # noqa: E402


def _lazy_pair(H=40, W=52, fs=2):
    return VT._Lazy(torch.zeros(fs, H, W, 3, dtype=torch.uint8)), VT._Lazy(torch.from_numpy(NO.label_clip(fs, H, W, 3)))


def test_nearest_table_follows_the_running_sum():
    for n_in, n_out in ((320, 224), (599, 500), (10, 4), (4, 10), (1, 7), (7, 1), (360, 224), (854, 448)):
        assert np.array_equal(VT.nearest_table(n_in, n_out), NO.nearest_index(n_in, n_out))
        assert np.array_equal(VT.nearest_table(n_in, n_out, 5, flip=True), NO.nearest_index(n_in, n_out)[::-1] + 5)
    mult = np.floor((320 / 224) * 0.5 + np.arange(224) * (320 / 224)).astype(np.int64)
    assert int((VT.nearest_table(320, 224) != mult).sum()) == 20               # the product form is a different map
    for bad in ((0, 4, 0), (4, 0, 0), (4, 4, -1)):
        with pytest.raises(ValueError):
            VT.nearest_table(*bad)


def test_annotation_steps_fold_into_one_pair_of_tables():
    """Resize -> RandomCrop -> flips -> CenterCrop on an annotation clip never launches: the tables compose on the host, and
    indexing once with them equals doing the steps one after the other."""
    d, a = _lazy_pair()
    labels = a.src.numpy()
    random.seed(4)
    steps = [VT.Resize((33, 47)), VT.RandomCrop((30, 40)), VT.RandomVerticalFlip(p=1.0), VT.RandomHorizontalFlip(p=1.0), VT.CenterCrop((21, 34))]
    for t in steps:
        d2, a = t._apply(VT._Lazy(torch.zeros(a.shape[0], a.shape[1], a.shape[2], 3, dtype=torch.uint8)), a)
    random.seed(4)
    want = np.stack([NO.resize_nearest(m, 33, 47) for m in labels])
    y1, x1 = VT.random_crop_origin(33, 47, 30, 40)
    random.random(), random.random()
    want = want[:, y1:y1 + 30, x1:x1 + 40][:, ::-1][:, :, ::-1]
    y1, x1 = VT.center_crop_origin(30, 40, 21, 34)
    want = want[:, y1:y1 + 21, x1:x1 + 34]
    assert a.shape == (2, 21, 34) and a.src.data_ptr() == torch.from_numpy(labels).data_ptr()
    assert np.array_equal(NO.gather(labels, a.yt, a.xt), want)
    # an identity step leaves the clip untouched
    d, a = _lazy_pair()
    VT.CenterCrop((40, 52))._apply(d, a)
    VT.Resize(40)._apply(d, a)           # the shorter side already has the size: the reference returns the clip as it is
    assert a.yt is None and d.yt is None and d.resize is None and a.materialize() is a.src


def test_draws_follow_the_reference_order():
    d, a = _lazy_pair()
    random.seed(11)
    VT.RandomCrop((10, 12))._apply(d, a)
    random.seed(11)
    x1 = random.randint(0, 52 - 12)
    y1 = random.randint(0, 40 - 10)
    assert a.yt[0] == y1 and a.xt[0] == x1 and a.shape == (2, 10, 12) and d.shape == (2, 10, 12, 3)
    # RandomHorizontalFlip: one random.random() with annotations, none without (and then never a flip)
    for cls in (VT.RandomHorizontalFlip, VT.RandomVerticalFlip):
        seen = []
        for seed in range(8):
            d, a = _lazy_pair()
            random.seed(seed)
            cls()._apply(d, a)
            after = random.getstate()
            random.seed(seed)
            chance = random.random()
            assert random.getstate() == after
            assert (a.yt is not None) == (chance < 0.5)
            seen.append(chance < 0.5)
        assert any(seen) and not all(seen)
    state = random.getstate()
    clip = torch.zeros(1, 4, 6, 3, dtype=torch.uint8)
    assert VT.RandomHorizontalFlip()(clip) is clip and random.getstate() == state
    with pytest.raises(TypeError):
        VT.RandomVerticalFlip()(clip)
    # RandomResizedCrop: one set of parameters for both clips
    d, a = _lazy_pair()
    random.seed(2)
    i, j, h, w = VT.RandomResizedCrop.get_params(d, (0.4, 1.0), (3. / 4., 4. / 3.))
    assert np.array_equal(VT._Lazy(a.src).resized_crop(i, j, h, w, (16, 16)).yt, VT.nearest_table(h, 16, i))


def test_constructor_and_size_checks_of_the_reference():
    with pytest.raises(ValueError):
        VT.RandomRotation(-3)
    with pytest.raises(ValueError):
        VT.RandomRotation((1, 2, 3))
    assert VT.RandomRotation(30).degrees == (-30, 30) and VT.RandomRotation((5, 9)).degrees == (5, 9)
    assert VT.RandomCrop(7).size == (7, 7) and VT.CenterCrop((3, 4)).size == (3, 4)
    d, a = _lazy_pair(8, 12)
    for t in (VT.RandomCrop((9, 4)), VT.RandomCrop((4, 13)), VT.CenterCrop((9, 4)), VT.CenterCrop((4, 13))):
        with pytest.raises(ValueError, match="Initial image size should be larger"):
            t._apply(d, a)
    assert VT.RandomResize().interpolation == "nearest" and VT.RandomResize().ratio == (3. / 4., 4. / 3.)
    with pytest.raises(NotImplementedError):
        VT.resize_clip(torch.zeros(1, 8, 8, dtype=torch.uint8), 4, "bilinear")
    with pytest.raises(NotImplementedError):
        VT.resize_clip(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 4, "bicubic")
    assert not hasattr(VT, "Normalize")


def test_factories_mirror_the_reference_entry_points():
    ev = VT.evaluation_transforms(448).transforms
    assert [type(t) for t in ev] == [VT.Resize, VT.CenterCrop, VT.ClipToTensor]
    assert ev[0].size == (448, 448) and ev[0].interpolation == "bilinear" and ev[1].size == (448, 448)
    pr = VT.propagation_transforms().transforms
    assert [type(t) for t in pr] == [VT.Resize, VT.RandomCrop, VT.ClipToTensor]
    assert pr[0].size == 224 and pr[0].interpolation == "bilinear" and pr[1].size == (224, 224)
    for chain in (ev, pr):
        assert chain[2].mean == [0.485, 0.456, 0.406] and chain[2].std == [0.228, 0.224, 0.225]


def test_annotations_to_uint8_is_lossless():
    v = torch.arange(256, dtype=torch.uint8)
    stacked = v.float().div(255).view(2, 4, 1, 4, 8)                 # [clips, fs, 1, H, W] as read_batch stacks them
    out = VT.annotations_to_uint8(stacked)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2, 4, 4, 8) and torch.equal(out.view(-1), v)
    assert tuple(VT.annotations_to_uint8(torch.zeros(2, 4, 3, 4, 8)).shape) == (2, 4, 3, 4, 8)   # only a size-1 axis 2 is squeezed


def test_rotate_coeffs_special_angles():
    assert VT.rotate_coeffs(8, 6, 0) == VT.rotate_coeffs(8, 6, 360) == (65536, 0, 32768, 0, 65536, 32768)
    a = np.arange(48, dtype=np.uint8).reshape(6, 8)
    assert np.array_equal(NO.affine_nearest(a, VT.rotate_coeffs(8, 6, 180)), a[::-1, ::-1])
    sq = np.arange(36, dtype=np.uint8).reshape(6, 6)
    assert np.array_equal(NO.affine_nearest(sq, VT.rotate_coeffs(6, 6, 90)), np.rot90(sq, 1))
    assert np.array_equal(NO.affine_nearest(sq, VT.rotate_coeffs(6, 6, -90)), np.rot90(sq, -1))


def test_raw_frame_clips_and_the_new_dataset_flag():
    args = MP.build_parser().parse_args([])
    assert tuple(args.raw_size) == (360, 480) and args.dataset == "davis_val"
    args = MP.build_parser().parse_args(["--dataset", "synthetic_frames", "--raw_size", "120", "160"])
    assert args.raw_size == [120, 160]
    frames, labels = MP.synthetic_frame_clip(3, 48, 64, seed=1)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (3, 48, 64, 3)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (3, 48, 64) and set(torch.unique(labels).tolist()) == {0, 1, 2}
    clip, masks = MP.synthetic_tracking_clip(3, 48, seed=1, width=64)
    assert torch.equal(labels.long(), masks) and 60 < float(frames.float().mean()) < 200
    with pytest.raises(ValueError):
        MP.synthetic_frame_clip(3, 50, 64, seed=1)
    with pytest.raises(NotImplementedError):
        MP.mask_propagation(MP.build_parser().parse_args(["--dataset", "davis_val"]))
