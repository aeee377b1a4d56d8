"""N21 on the GPU: tt_jpeg_decode_batch against Pillow's decode of the fixture files (tests/golden/jpeg_frames.npz, written by
tools/gen_jpeg_golden.py) - every comparison is for equality in every bit -, the descriptor-table validation, and the clip loader and
the two drivers over a directory tree of those files."""
import os
import random

import numpy as np
import pytest
import torch

import _jpeg_ref as R
from timetuning_amd import _lib, hip_ops

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_frames.npz")


@pytest.fixture(scope="module")
def fx():
    return R.fixture(GOLDEN)


@pytest.fixture(scope="module")
def grid_names(fx):
    names = [n for n in fx[0] if n.startswith("grid_")]
    assert len(names) == 7 * 3 * 4 * 3
    return names


@pytest.fixture(scope="module")
def one_per_call(fx, grid_names):
    """Every grid case decoded in a call of its own (computed once, shared)."""
    return {n: hip_ops.decode_jpeg_batch([fx[0][n][0]], threads=1)[0].cpu().numpy() for n in grid_names}


def test_grid_cases_one_per_call_equal_pillow(fx, grid_names, one_per_call):
    """Sizes 1x1 ... 37x53 x 4:4:4 / 4:2:2 / 4:2:0 x quality 30 / 75 / 95 / 100 x default tables / optimize=True / restart interval 3."""
    wrong = [n for n in grid_names if not np.array_equal(one_per_call[n], fx[0][n][1])]
    assert not wrong, wrong[:10]


def test_all_grid_cases_in_one_call(fx, grid_names, one_per_call):
    """Mixed sizes and samplings in ONE descriptor table: the same bits as one case per call, and as Pillow."""
    frames = hip_ops.decode_jpeg_batch([fx[0][n][0] for n in grid_names], threads=4)
    assert len(frames) == len(grid_names)
    for n, f in zip(grid_names, frames):
        got = f.cpu().numpy()
        assert np.array_equal(got, one_per_call[n]), n
        assert np.array_equal(got, fx[0][n][1]), n


@pytest.mark.parametrize("name", ["checker_16x16_444_q100", "checker_16x16_422_q100", "checker_16x16_420_q100", "strip_64x8_420_q75",
                                  "strip_8x64_420_q75", "frame_360x480_420_q90"])
def test_extra_cases_equal_pillow(fx, name):
    """Both clamps (a 0 / 255 checkerboard at quality 100), one block row / column of chroma, and the workload's frame size once."""
    data, want = fx[0][name]
    if name.startswith("checker"):
        assert want.min() == 0 and want.max() == 255
    got = hip_ops.decode_jpeg_batch([data])[0]
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)


def test_equal_size_frames_come_back_as_one_tensor(fx):
    names = [f"clip_v0_f{k}" for k in range(5)]
    frames = hip_ops.decode_jpeg_batch([fx[0][n][0] for n in names], threads=5)
    clip = hip_ops.frames_as_clip(frames)
    assert tuple(clip.shape) == (5, 48, 64, 3) and clip.is_contiguous()
    assert clip.data_ptr() == frames[0].data_ptr() and clip[3].data_ptr() == frames[3].data_ptr()      # views, not copies
    assert np.array_equal(clip.cpu().numpy(), np.stack([fx[0][n][1] for n in names]))


def test_unsupported_and_broken_files_raise(fx):
    for name in ("prog_48x64_420_q90", "gray_16x16_q75", "cmyk_16x16_q75"):
        with pytest.raises(hip_ops.JpegUnsupported):
            hip_ops.decode_jpeg_batch([fx[0]["clip_v0_f0"][0], fx[0][name][0]])
    data = fx[0]["clip_v0_f0"][0]
    with pytest.raises(ValueError):
        hip_ops.decode_jpeg_batch([data, data[:len(data) // 2]])


def test_table_validation_refuses_without_launching(fx):
    """Every offset and extent of the table is checked against the buffers before anything is launched: a table that points outside
    is TT_EINVAL and the output keeps its bytes."""
    lib = _lib.load()
    names = ["clip_v0_f0", "grid_17x33_422_q75_std"]
    batch = hip_ops.jpeg_scan_batch([fx[0][n][0] for n in names], threads=2)
    n, row = 2, 16 * 8
    dev = torch.device("cuda", torch.cuda.current_device())
    coeffs, meta = batch.coeffs.to(dev), batch.meta.to(dev)
    good = batch.meta.numpy()[:n * row].view(np.int64).reshape(n, 16).copy()
    ws_bytes = lib.tt_jpeg_decode_batch_workspace_bytes(good.ctypes.data, n)
    assert ws_bytes >= int(good[1, 11]) + 64
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.full((batch.out_bytes,), 0xA5, dtype=torch.uint8, device=dev)

    def call(table, n_coeffs=batch.n_coeffs, n_q=3 * n, out_bytes=batch.out_bytes, ws_b=ws_bytes):
        table = np.ascontiguousarray(table)
        return lib.tt_jpeg_decode_batch(coeffs.data_ptr(), n_coeffs, meta.data_ptr() + n * row, n_q, table.ctypes.data, meta.data_ptr(), n,
                                        out.data_ptr(), out_bytes, ws.data_ptr(), ws_b, torch.cuda.current_stream().cuda_stream)

    def bad(col, value, frame=1):
        t = good.copy()
        t[frame, col] = value
        return t

    refused = [call(bad(3, batch.n_coeffs)), call(bad(4, -8)), call(bad(5, int(good[1, 5]) + 8)), call(bad(3, 4)),   # coefficients: past, negative, overrun, unaligned
               call(bad(6, 3 * n)), call(bad(7, -1)),                                                                # table slot
               call(bad(9, ws_bytes)), call(bad(11, ws_bytes - 8)), call(bad(10, 4)),                        # planes
               call(bad(12, batch.out_bytes - 10)), call(bad(12, -1)),                                                # output
               call(bad(0, 0)), call(bad(1, 70000)), call(bad(2, 3)), call(bad(0, 1 << 40, frame=0)),                 # not a frame
               call(good, n_coeffs=batch.n_coeffs - 1), call(good, n_q=3 * n - 1), call(good, out_bytes=int(good[1, 12]) + 17 * 33 * 3 - 1),
               call(good, ws_b=int(good[1, 11]))]
    torch.cuda.synchronize()
    assert refused == [-1] * len(refused)
    assert "jpeg_decode_batch" in lib.tt_last_error().decode()
    assert bool((out == 0xA5).all())
    assert lib.tt_jpeg_decode_batch_workspace_bytes(bad(2, 7).ctypes.data, n) == 0
    assert call(good) == 0
    torch.cuda.synchronize()
    want = fx[0][names[1]][1]
    at = int(good[1, 12])
    assert np.array_equal(out[at:at + want.size].cpu().numpy().reshape(want.shape), want)


# ---- the clip loader and the drivers over a directory tree of the fixture files
def _write_tree(root, fx, swap=None):
    """<root>/JPEGImages/video{0,1}/0000k.jpg and <root>/Annotations/video{0,1}/0000k.png: five 48 x 64 frames each.  ``swap`` maps
    (video, frame) to other bytes."""
    files, anns = fx
    for v in range(2):
        (root / "JPEGImages" / f"video{v}").mkdir(parents=True)
        (root / "Annotations" / f"video{v}").mkdir(parents=True)
        for f in range(5):
            data = (swap or {}).get((v, f), files[f"clip_v{v}_f{f}"][0])
            (root / "JPEGImages" / f"video{v}" / f"{f:05d}.jpg").write_bytes(data)
            (root / "Annotations" / f"video{v}" / f"{f:05d}.png").write_bytes(anns[f"clip_v{v}_f{f}"][0])
    return root


def _expected_batch(fx, indices, pixels_of):
    """The evaluation pair transform on Pillow's pixels and the fixture's label maps, as the loader stacks them."""
    from timetuning_amd import video_transformations as VT

    transform = VT.evaluation_transforms(32)
    data, ann = [], []
    for v, idx in enumerate(indices):
        frames = torch.from_numpy(np.stack([pixels_of(v, f) for f in idx])).cuda()
        labels = torch.from_numpy(np.stack([fx[1][f"clip_v{v}_f{f}"][1] for f in idx])).cuda()
        d, a = transform(frames, labels)
        data.append(d[None])
        ann.append(VT.annotations_to_uint8(a[None]))
    return torch.stack(data), torch.stack(ann)


@pytest.mark.parametrize("prefetch", [True, False])
def test_clip_loader_equals_the_transforms_on_pillow_pixels(fx, tmp_path, prefetch):
    pytest.importorskip("PIL.Image")
    from timetuning_amd import video_transformations as VT
    from timetuning_amd.data_loader import ClipLoader, SamplingMode, VideoDataset, generate_indices

    root = _write_tree(tmp_path / "set", fx)
    ds = VideoDataset(str(root / "JPEGImages"), str(root / "Annotations"), SamplingMode.UNIFORM, 1, 3, video_transform=VT.evaluation_transforms(32),
                      threads=4)
    loader = ClipLoader(ds, 2, shuffle=False, seed=7, prefetch=prefetch)
    twin = random.Random()
    twin.setstate(loader.rng.getstate())
    indices = [generate_indices(5, 3, SamplingMode.UNIFORM, rng=twin)[0] for _ in range(2)]
    random.seed(123)
    state = random.getstate()
    batches = list(loader)
    assert random.getstate() == state                    # the index draws left the transforms' generator alone
    assert len(batches) == 1 == len(loader)
    data, ann, label = batches[0]
    want_data, want_ann = _expected_batch(fx, indices, lambda v, f: fx[0][f"clip_v{v}_f{f}"][1])
    assert data.dtype == torch.float32 and tuple(data.shape) == (2, 1, 3, 3, 32, 32) and data.is_cuda
    assert ann.dtype == torch.uint8 and tuple(ann.shape) == (2, 1, 3, 32, 32)
    assert torch.equal(data, want_data) and torch.equal(ann, want_ann)
    assert label.tolist() == [[0.0], [1.0]]
    assert loader.fallback_frames == 0
    # __getitem__ is the same path for one video, drawing from the global generator as the reference does
    random.seed(9)
    idx = generate_indices(5, 3, SamplingMode.UNIFORM)[0]
    random.seed(9)
    d1, a1, l1 = ds[1]
    frames = torch.from_numpy(np.stack([fx[0][f"clip_v1_f{f}"][1] for f in idx])).cuda()
    labels = torch.from_numpy(np.stack([fx[1][f"clip_v1_f{f}"][1] for f in idx])).cuda()
    d, a = VT.evaluation_transforms(32)(frames, labels)
    assert torch.equal(d1, d[None]) and torch.equal(a1, VT.annotations_to_uint8(a[None])) and l1.tolist() == [1.0]


def test_unsupported_files_fall_back_and_are_counted_but_broken_ones_raise(fx, tmp_path):
    pytest.importorskip("PIL.Image")
    from timetuning_amd import video_transformations as VT
    from timetuning_amd.data_loader import ClipLoader, SamplingMode, VideoDataset

    prog, prog_pixels = fx[0]["prog_48x64_420_q90"]
    root = _write_tree(tmp_path / "mixed", fx, swap={(0, 2): prog})
    ds = VideoDataset(str(root / "JPEGImages"), str(root / "Annotations"), SamplingMode.Full, 1, 5, video_transform=VT.evaluation_transforms(32))
    loader = ClipLoader(ds, 2)
    data, ann, _ = next(iter(loader))
    pixels_of = lambda v, f: prog_pixels if (v, f) == (0, 2) else fx[0][f"clip_v{v}_f{f}"][1]
    want_data, want_ann = _expected_batch(fx, [range(5), range(5)], pixels_of)
    assert torch.equal(data, want_data) and torch.equal(ann, want_ann)
    assert loader.fallback_frames == 1
    # a SUPPORTED file that fails to decode is an error, not a fallback
    good = fx[0]["clip_v1_f3"][0]
    root = _write_tree(tmp_path / "broken", fx, swap={(1, 3): good[:len(good) * 2 // 3]})
    ds = VideoDataset(str(root / "JPEGImages"), str(root / "Annotations"), SamplingMode.Full, 1, 5, video_transform=VT.evaluation_transforms(32))
    with pytest.raises(ValueError, match="malformed JPEG"):
        next(iter(ClipLoader(ds, 2)))
    assert ds.fallback_frames == 0


def test_time_tuning_trains_an_epoch_on_a_directory_tree(fx, tmp_path, capsys):
    pytest.importorskip("PIL.Image")
    import re

    from timetuning_amd.time_tuning import build_parser, time_tuning

    root = _write_tree(tmp_path / "davis", fx)
    args = build_parser().parse_args(["--dataset", "davis", "--dataset_path", str(root), "--model_path", "", "--batch_size", "1", "--num_frames", "2",
                                      "--regular_step", "3", "--num_workers", "2", "--num_clusters", "20", "--num_epochs", "1", "--eval_every", "0",
                                      "--logging_directory", str(tmp_path / "logs")])
    before = hip_ops.get_gemm_precision()
    try:
        model = time_tuning(0, args)
    finally:
        hip_ops.set_gemm_precision(before)
    out = capsys.readouterr().out
    losses = [float(v) for v in re.findall(r"Iteration: \d+/2 loss ([-+0-9.einfa]+)", out)]
    assert len(losses) == 2 and all(np.isfinite(losses)) and all(v > 0 for v in losses)      # two videos, batch 1: two steps
    assert torch.isfinite(model.prototypes).all()
    assert "frames decoded with Pillow on the host so far (files the device decoder does not take): 0" in out


def test_mask_propagation_reads_a_directory_tree(fx, tmp_path, capsys):
    pytest.importorskip("PIL.Image")
    from timetuning_amd import mask_propagation as MP

    root = _write_tree(tmp_path / "davis", fx)
    score = MP.mask_propagation(MP.build_parser().parse_args(["--dataset", "davis_val", "--dataset_path", str(root), "--model_path", "",
                                                             "--num_frames", "3", "--num_workers", "2"]))
    out = capsys.readouterr().out
    assert 0.0 <= score <= 1.0 and "mean J over 2 clips" in out and "decoded with Pillow on the host" in out
