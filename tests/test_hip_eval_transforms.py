"""N11 on the GPU: the nearest-gather and nearest-affine kernels against the NumPy restatements of tests/_nearest_ops.py (which
tests/test_nearest_ops_pillow.py pins against Pillow), the pair transforms of video_transformations against the reference's own
classes (tests/golden/eval_transforms.npz, tools/gen_eval_transforms_golden.py), fused against step-by-step chains, the refusals
at the edge of the kernels' domain, and the two drivers that start from raw frames.  Everything is integer or exactly rounded
arithmetic: every comparison is equality.  Needs neither Pillow nor a reference checkout."""
import os
import random
import sys

import numpy as np
import pytest
import torch

from timetuning_amd import _lib
from timetuning_amd import hip_ops as ops
from timetuning_amd import video_transformations as VT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nearest_ops as NO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN, STD = [0.485, 0.456, 0.406], [0.228, 0.224, 0.225]
f32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def to_tensor_np(clip, mean=None, std=None):
    """ClipToTensor in NumPy fp32: [F, H, W] -> [F, 1, H, W] = v / 255; [F, H, W, 3] -> [F, 3, H, W] = (v / 255 - mean) / std."""
    if clip.ndim == 3:
        return (clip.astype(f32) / f32(255))[:, None]
    t = np.ascontiguousarray(clip.transpose(0, 3, 1, 2)).astype(f32) / f32(255)
    if mean is None:
        return t
    return ((t - np.asarray(mean, f32)[None, :, None, None]) / np.asarray(std, f32)[None, :, None, None]).astype(f32)


def _clip(rng, F, H, W, C):
    return rng.integers(0, 256, (F, H, W) if C == 1 else (F, H, W, 3), dtype=np.uint8)


# (F, Hin, Win, OH, OW, tables): output rows of 1, 16 k and 16 k + r bytes (C = 1) and of 3 OW bytes (C = 3), rows that start on
# and off a 16-byte boundary (F * OH > 1 with an odd row length), OH = 1, OW = 1, one work item, and more than one block of 256 items
GATHER_CASES = [(2, 37, 53, 29, 64, "random"), (3, 37, 53, 5, 17, "random"), (2, 9, 11, 7, 1, "random"), (2, 9, 11, 1, 13, "random"),
                (1, 1, 1, 1, 1, "identity"), (2, 19, 48, 19, 48, "identity"), (2, 19, 23, 19, 23, "identity"), (2, 19, 23, 19, 23, "flip_x"),
                (2, 19, 32, 19, 32, "flip_y"), (2, 21, 30, 21, 30, "flip_xy"), (2, 60, 80, 224, 224, "resize"), (1, 300, 5, 280, 3, "resize"),
                (3, 40, 50, 33, 47, "crop_resize_flip")]


def _tables(kind, rng, Hin, Win, OH, OW):
    if kind == "random":
        return rng.integers(0, Hin, OH).astype(np.int32), rng.integers(0, Win, OW).astype(np.int32)
    if kind == "resize":
        return VT.nearest_table(Hin, OH), VT.nearest_table(Win, OW)
    if kind == "crop_resize_flip":
        return VT.nearest_table(Hin - 9, OH, 4, flip=True), VT.nearest_table(Win - 11, OW, 6, flip=True)
    flips = kind[len("flip_"):] if kind.startswith("flip_") else ""
    return VT.nearest_table(Hin, Hin, flip="y" in flips), VT.nearest_table(Win, Win, flip="x" in flips)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("case", GATHER_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_gather_matches_numpy(case, C):
    F, Hin, Win, OH, OW, kind = case
    rng = np.random.default_rng(100 + Hin + OW + C)
    clip = _clip(rng, F, Hin, Win, C)
    ytab, xtab = _tables(kind, rng, Hin, Win, OH, OW)
    want = NO.gather(clip, ytab, xtab)
    if kind == "identity":
        assert np.array_equal(want, clip)
    got = ops.img_gather_nearest(dev(clip), ytab, xtab)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert np.array_equal(host(got), want)
    if C == 1:
        got_f = ops.img_gather_nearest(dev(clip), ytab, xtab, True)
        assert np.array_equal(host(got_f), to_tensor_np(want))
    else:
        got_f = ops.img_gather_nearest(dev(clip), ytab, xtab, (MEAN, STD))
        assert np.array_equal(host(got_f), to_tensor_np(want, MEAN, STD))
    assert got_f.dtype == torch.float32 and tuple(got_f.shape) == (F, C, OH, OW)


def test_float_label_plane_is_an_exact_division():
    """All 256 label values: v / 255 as torch's ``.float().div(255)`` gives it, and ``read_batch``'s ``(255 * a).type(uint8)`` undoes it."""
    v = torch.arange(256, dtype=torch.uint8).view(1, 1, 256)
    ident = np.arange(256, dtype=np.int32)
    got = ops.img_gather_nearest(v.to(DEV), np.zeros(1, np.int32), ident, True)
    # (the host division is the judge, as in the reference's ToTensor: torch's device kernel for a division by a scalar multiplies
    # by the reciprocal and differs from it in the last bit for some values)
    assert torch.equal(got.cpu(), v.float().div(255).view(1, 1, 1, 256))
    back = VT.annotations_to_uint8(got[None])
    assert back.dtype == torch.uint8 and tuple(back.shape) == (1, 1, 1, 256) and torch.equal(back.cpu().view(-1), v.view(-1))
    # through the class, at a width that is no multiple of the store width
    ann = torch.arange(256, dtype=torch.uint8).repeat(3)[:255 * 3].view(1, 15, 51).to(DEV)
    _, a = VT.ClipToTensor()(torch.zeros(1, 15, 51, 3, dtype=torch.uint8, device=DEV), ann)
    assert tuple(a.shape) == (1, 1, 15, 51) and torch.equal(a.cpu(), ann.cpu().float().div(255).unsqueeze(1))


@pytest.mark.parametrize("shape", [(2, 19, 23), (1, 16, 64), (3, 5, 1)])
def test_identity_gather_equals_clip_to_tensor(shape):
    F, H, W = shape
    clip = dev(_clip(np.random.default_rng(3), F, H, W, 3))
    ident = (np.arange(H, dtype=np.int32), np.arange(W, dtype=np.int32))
    for t in (VT.ClipToTensor(MEAN, STD), VT.ClipToTensor()):
        assert torch.equal(ops.img_gather_nearest(clip, *ident, t.mean_std()), t(clip))


AFFINE_SIZES = [(33, 47), (16, 64), (1, 1), (5, 1), (1, 7), (70, 70)]


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("size", AFFINE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_affine_matches_numpy(size, C):
    H, W = size
    rng = np.random.default_rng(200 + H + W + C)
    clip = _clip(rng, 2, H, W, C)
    coeff_sets = [NO.rotate_fixed_coeffs(W, H, a) for a in (0.0, 30.0, 90.0, 180.0, 270.0, -17.3, 123.456)]
    coeff_sets.append((65536, 0, 32768, 0, 65536, 32768))                          # identity
    coeff_sets.append((-40000, 90000, 3 << 16, 70000, 20000, -(5 << 16)))          # negative coordinates: arithmetic shifts, zero fill
    coeff_sets.append(tuple(int(v) for v in rng.integers(-200000, 200000, 6)))
    for coeffs in coeff_sets:
        want = np.stack([NO.affine_nearest(f, coeffs) for f in clip])
        got = ops.img_affine_nearest(dev(clip), coeffs)
        assert got.dtype == torch.uint8 and tuple(got.shape) == clip.shape
        assert np.array_equal(host(got), want), coeffs
    assert np.array_equal(host(ops.img_affine_nearest(dev(clip), coeff_sets[7])), clip)
    assert np.array_equal(host(VT.rotate_clip(dev(clip), 30.0)), np.stack([NO.rotate(f, 30.0) for f in clip]))
    assert VT.rotate_coeffs(W, H, -17.3) == NO.rotate_fixed_coeffs(W, H, -17.3)


def test_gather_reads_past_2_31_bytes():
    """A label clip of 2 200 frames of 1 000 x 1 000 is 2.2e9 bytes: frames behind byte 2^31 must come back (64-bit offsets)."""
    F, H, W = 2200, 1000, 1000
    rng = np.random.default_rng(8)
    clip = torch.zeros((F, H, W), dtype=torch.uint8, device=DEV)
    assert clip.numel() > 2 ** 31
    marked = {f: rng.integers(0, 256, (H, W), dtype=np.uint8) for f in (0, 2147, 2148, F - 1)}    # 2148 is the first frame past 2^31
    for f, a in marked.items():
        clip[f] = dev(a)
    ytab, xtab = rng.integers(0, H, 37).astype(np.int32), rng.integers(0, W, 41).astype(np.int32)
    got = ops.img_gather_nearest(clip, ytab, xtab)
    got_f = ops.img_gather_nearest(clip, ytab, xtab, True)
    for f, a in marked.items():
        assert np.array_equal(host(got[f]), a[ytab][:, xtab]), f
    assert int(got.sum(dtype=torch.int64)) == sum(int(a[ytab][:, xtab].sum()) for a in marked.values())   # every other frame is zero
    assert torch.equal(got_f.cpu(), got.cpu().float().div(255).unsqueeze(1))
    rot = ops.img_affine_nearest(clip, NO.rotate_fixed_coeffs(W, H, 90.0))
    assert np.array_equal(host(rot[F - 1]), NO.rotate(marked[F - 1], 90.0))
    assert np.array_equal(host(rot[2148]), NO.rotate(marked[2148], 90.0))


# ---- the reference's own classes (tests/golden/eval_transforms.npz) ----------------------------------------------------------------

def _seed(n):
    random.seed(n)
    torch.manual_seed(n)


def _finish(pair):
    data, ann = pair
    return host(data), host(VT.annotations_to_uint8(ann[None])[0])


def _fixture_chains(g, tag):
    """(key, seed, callable(data, ann) -> (data, ann))) for every chain recorded for one input, built as the generator built them."""
    R = int(g["cfg_R"])
    ccrop = tuple(int(v) for v in g["cfg_ccrop"])
    degrees = int(g["cfg_rot_degrees"])
    chains = [(f"eval_{tag}", 0, VT.evaluation_transforms(R)), (f"ccrop_{tag}", 0, VT.Compose([VT.CenterCrop(ccrop), VT.ClipToTensor()]))]

    def seeds(prefix):
        return sorted(int(k[len(prefix):-len("_data")]) for k in g.files if k.startswith(prefix) and k.endswith("_data"))

    for n in seeds(f"prop_{tag}_seed"):
        chains.append((f"prop_{tag}_seed{n}", n, VT.propagation_transforms(R)))
    train = VT.Compose([VT.Resize(R), VT.RandomResizedCrop((R, R)), VT.RandomHorizontalFlip(), VT.ClipToTensor(mean=MEAN, std=STD)])
    for n in seeds(f"train_{tag}_seed"):
        chains.append((f"train_{tag}_seed{n}", n, train))
    for n in seeds(f"vflip_{tag}_seed"):
        chains.append((f"vflip_{tag}_seed{n}", n, VT.Compose([VT.RandomVerticalFlip(), VT.ClipToTensor()])))

    def clip_only(t):
        def run(data, ann):
            state = random.getstate()
            d = t(data)
            random.setstate(state)        # the generator re-seeds in front of the annotation clip
            return VT.ClipToTensor()(d, t(ann))
        return run

    for n in seeds(f"rresize_{tag}_seed"):
        chains.append((f"rresize_{tag}_seed{n}", n, clip_only(VT.RandomResize())))
    for n in seeds(f"rrot_{tag}_seed"):
        chains.append((f"rrot_{tag}_seed{n}", n, clip_only(VT.RandomRotation(degrees))))
    return chains


@pytest.mark.parametrize("tag", ["a", "b"])
def test_chains_match_the_reference(golden, tag):
    g = golden("eval_transforms")
    frames, labels = g[f"{tag}_frames"], g[f"{tag}_labels"]
    fs, H, W = labels.shape
    assert np.array_equal(frames, NO.frame_clip(fs, H, W, 41 if tag == "a" else 42))
    assert np.array_equal(labels, NO.label_clip(fs, H, W, 41 if tag == "a" else 42)) and len(np.unique(labels)) >= 5
    chains = _fixture_chains(g, tag)
    assert len(chains) == len([k for k in g.files if k.endswith("_data") and f"_{tag}" in k])
    for key, seed, chain in chains:
        _seed(seed)
        data, ann = _finish(chain(dev(frames), dev(labels)))
        assert data.dtype == np.float32 and ann.dtype == np.uint8
        assert data.shape == g[key + "_data"].shape and ann.shape == g[key + "_ann"].shape, key
        assert np.array_equal(data, g[key + "_data"]), key
        assert np.array_equal(ann, g[key + "_ann"]), key
    for kind in ("train", "vflip"):   # both decisions occur among the recorded seeds
        flips = [bool(g[k]) for k in g.files if k.startswith(f"{kind}_{tag}_seed") and k.endswith("_flipped")]
        assert any(flips) and not all(flips), (kind, flips)


def test_random_resize_swaps_the_sides_as_the_reference_does(golden):
    g = golden("eval_transforms")
    labels = g["a_labels"]
    _seed(0)
    s = random.uniform(3. / 4., 4. / 3.)
    _seed(0)
    out = VT.RandomResize()(dev(labels))
    assert tuple(out.shape[1:]) == (int(labels.shape[2] * s), int(labels.shape[1] * s)) == g["rresize_a_seed0_ann"].shape[1:]


@pytest.mark.parametrize("name", ["evaluation", "propagation", "training", "flips"])
def test_fused_chain_equals_step_by_step(name):
    R = 48
    chain = {"evaluation": VT.evaluation_transforms(R), "propagation": VT.propagation_transforms(R),
             "training": VT.Compose([VT.Resize(R), VT.RandomResizedCrop((R, R)), VT.RandomHorizontalFlip(), VT.ClipToTensor(mean=MEAN, std=STD)]),
             "flips": VT.Compose([VT.RandomCrop((40, 61)), VT.RandomVerticalFlip(), VT.Resize((33, 50)), VT.RandomHorizontalFlip(),
                                  VT.CenterCrop((31, 47)), VT.ClipToTensor(mean=MEAN, std=STD)])}[name]
    frames, labels = dev(NO.frame_clip(2, 72, 104, 5)), dev(NO.label_clip(2, 72, 104, 5))
    for seed in range(4):
        _seed(seed)
        fd, fa = chain(frames, labels)
        state = random.getstate()
        _seed(seed)
        d, a = frames, labels
        for t in chain.transforms:          # tensors in, tensors out: every step launches on its own
            d, a = t(d, a)
            assert isinstance(d, torch.Tensor) and isinstance(a, torch.Tensor)
        assert random.getstate() == state   # the same draws
        assert torch.equal(fd, d) and torch.equal(fa, a), (name, seed)
    # a pair chain that does not end in ClipToTensor hands back uint8 clips of both kinds
    _seed(1)
    d, a = VT.Compose([VT.Resize(R), VT.RandomCrop(R)])(frames, labels)
    assert d.dtype == torch.uint8 and tuple(d.shape) == (2, R, R, 3) and a.dtype == torch.uint8 and tuple(a.shape) == (2, R, R)
    _seed(1)
    y1, x1 = VT.random_crop_origin(R, VT.get_resize_sizes(72, 104, R)[1], R, R)
    assert torch.equal(d, VT.resize_clip(frames, R)[:, y1:y1 + R, x1:x1 + R])
    assert torch.equal(a, VT.resize_clip(labels, R, "nearest")[:, y1:y1 + R, x1:x1 + R])
    assert np.array_equal(host(VT.resize_clip(labels, (30, 40), "nearest")), np.stack([NO.resize_nearest(m, 30, 40) for m in host(labels)]))
    assert np.array_equal(host(VT.resize_clip(frames, (30, 40), "nearest")), np.stack([NO.resize_nearest(m, 30, 40) for m in host(frames)]))


def test_refusals_at_the_edge_of_the_domain():
    """Outside the stated domain a call is an error raised on the host before any launch; the last size inside it runs."""
    one = np.zeros(1, np.int32)

    def u8(*shape):
        return torch.zeros(shape, dtype=torch.uint8, device=DEV)

    for C in (2, 4):
        with pytest.raises(_lib.HipLibraryError, match="C must be 1"):
            ops.img_gather_nearest(u8(1, 4, 4, C), one, one)
        with pytest.raises(_lib.HipLibraryError, match="C must be 1"):
            ops.img_affine_nearest(u8(1, 4, 4, C), (65536, 0, 32768, 0, 65536, 32768))
    # sides: 32 767 is the last one in
    assert tuple(ops.img_gather_nearest(u8(1, 1, 32767), one, np.array([32766], np.int32)).shape) == (1, 1, 1)
    with pytest.raises(_lib.HipLibraryError, match="sides up to 32767"):
        ops.img_gather_nearest(u8(1, 1, 32768), one, one)
    with pytest.raises(_lib.HipLibraryError, match="sides up to 32767"):
        ops.img_gather_nearest(u8(1, 2, 2), one, np.zeros(32768, np.int32))
    # frames (uint8 output) and frame planes (float output) against the grid limit
    assert tuple(ops.img_gather_nearest(u8(65535, 1, 1), one, one).shape) == (65535, 1, 1)
    with pytest.raises(_lib.HipLibraryError, match="grid limit"):
        ops.img_gather_nearest(u8(65536, 1, 1), one, one)
    assert tuple(ops.img_gather_nearest(u8(21846, 1, 1, 3), one, one).shape) == (21846, 1, 1, 3)
    assert tuple(ops.img_gather_nearest(u8(21845, 1, 1, 3), one, one, (MEAN, STD)).shape) == (21845, 3, 1, 1)
    with pytest.raises(_lib.HipLibraryError, match="grid limit"):
        ops.img_gather_nearest(u8(21846, 1, 1, 3), one, one, (MEAN, STD))
    # index tables are checked on the host
    for bad in (np.array([4], np.int32), np.array([-1], np.int32), np.zeros(0, np.int32), np.zeros((1, 1), np.int32)):
        with pytest.raises(ValueError):
            ops.img_gather_nearest(u8(1, 4, 4), bad, one)
        with pytest.raises(ValueError):
            ops.img_gather_nearest(u8(1, 4, 4), one, bad)
    with pytest.raises(TypeError):
        ops.img_gather_nearest(torch.zeros(1, 4, 4, device=DEV), one, one)
    with pytest.raises(ValueError):
        ops.img_gather_nearest(u8(4, 4), one, one)
    # the affine transform: sides up to 16 384, frames up to the grid limit, corners inside Pillow's fixed-point range
    ident = (65536, 0, 32768, 0, 65536, 32768)
    assert tuple(ops.img_affine_nearest(u8(1, 1, 16384), ident).shape) == (1, 1, 16384)
    with pytest.raises(_lib.HipLibraryError, match="sides up to 16384"):
        ops.img_affine_nearest(u8(1, 1, 16385), ident)
    with pytest.raises(_lib.HipLibraryError, match="grid limit"):
        ops.img_affine_nearest(u8(65536, 1, 1), ident)
    with pytest.raises(_lib.HipLibraryError, match="fixed-point range"):
        ops.img_affine_nearest(u8(1, 4, 4), (65536, 0, 32768 << 16, 0, 65536, 32768))
    with pytest.raises(_lib.HipLibraryError, match="fixed-point range"):
        ops.img_affine_nearest(u8(1, 4, 4), (65536, 0, 32768, 2 ** 31 - 1, 65536, 32768))
    with pytest.raises(ValueError):
        ops.img_affine_nearest(u8(1, 4, 4), ident[:5])
    # bilinear resizing of label maps is not built, and the class-level checks of the reference hold
    with pytest.raises(NotImplementedError):
        VT.resize_clip(u8(1, 8, 8), 4, "bilinear")
    with pytest.raises(ValueError):
        VT.RandomCrop(9)(u8(1, 8, 12, 3), u8(1, 8, 12))
    with pytest.raises(ValueError):
        VT.CenterCrop((4, 13))(u8(1, 8, 12, 3))
    with pytest.raises(TypeError):
        VT.RandomVerticalFlip()(u8(1, 8, 12, 3))
    torch.cuda.synchronize()
    assert torch.equal(ops.img_gather_nearest(torch.full((1, 2, 2), 7, dtype=torch.uint8, device=DEV), one, one).cpu(),
                       torch.full((1, 1, 1), 7, dtype=torch.uint8))


# ---- the drivers that start from raw frames ----------------------------------------------------------------------------------------

def test_evaluator_on_frame_clips():
    from timetuning_amd.evaluation import Evaluator
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import SyntheticEvalFrameClips, TimeT

    R = 224
    loader = SyntheticEvalFrameClips(3, 2, R, 2, torch.device(DEV), raw_size=(120, 160))
    assert len(loader) == 2
    for k, (data, ann) in enumerate(loader):
        bs = 2 - k
        assert data.dtype == torch.float32 and tuple(data.shape) == (bs, 1, 2, 3, R, R)
        assert ann.dtype == torch.uint8 and tuple(ann.shape) == (bs, 1, 2, R, R)
        assert set(torch.unique(ann).tolist()) == {0, 1, 2}
        assert abs(float(data.mean())) < 1.0 and 0.3 < float(data.std()) < 3.0     # normalised frames, not raw bytes
    model = TimeT(FeatureExtractor("dino-s16", "", [1024, 1024, 512, 256], init="stress", return_attention=False), 20).to(DEV)
    ev = Evaluator(model, loader, num_prototypes=3, clustering_algorithm="k-means", involve_bg=True)
    for protocol in ("frame-wise", "dataset-wise"):
        s = ev.evaluate(evaluation_protocol=protocol, eval_resolution=56, num_clusters=3)
        assert 0.0 <= s <= 1.0


def test_mask_propagation_from_raw_frames():
    from timetuning_amd import mask_propagation as MP

    args = MP.build_parser().parse_args(["--dataset", "synthetic_frames", "--raw_size", "120", "160", "--model_path", "", "--num_clips", "2",
                                         "--num_frames", "3", "--input_resolution", "112", "--uvos", "0"])
    for i in range(2):
        clip, masks = MP.synthetic_frames_clip(args, i, torch.device(DEV))
        assert clip.dtype == torch.float32 and tuple(clip.shape) == (3, 3, 112, 112)
        assert masks.dtype == torch.int64 and tuple(masks.shape) == (3, 112, 112)
        assert set(torch.unique(masks).tolist()) == {0, 1, 2}                          # the planted labels, unblended
        again, masks2 = MP.synthetic_frames_clip(args, i, torch.device(DEV))          # seeded per clip
        assert torch.equal(clip, again) and torch.equal(masks, masks2)
    score = MP.mask_propagation(args)
    assert np.isfinite(score) and 0.0 <= score <= 1.0
    args.frame_size = [112, 112]
    with pytest.raises(ValueError):
        MP.mask_propagation(args)
