"""GPU checks of N10, the optical-flow baseline (mask_propagation.py:265-346, :803-815) on farneback.hip: the gray conversion bit for
bit, the level-0 image and expansion, and full flows against the fp64 restatement of OpenCV's Farneback (tests/_farneback.py; cv2
itself is unpinned) over pyramid depths 0-3, poly_n 5 / 7, several winsizes and iterations; a known translation; the label remap and
the propagate chain bit for bit; determinism and batching; the public functions and the command-line driver."""
import os
import sys

import numpy as np
import pytest
import torch

from timetuning_amd import _lib
from timetuning_amd import hip_ops as ops
from timetuning_amd import mask_propagation as MP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _farneback as FB  # noqa: E402
from test_optical_flow_host import smooth_texture  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
# fp32 kernel against the fp64 restatement (the same algorithm; the kernel's fp32 stages and fp64 sums round differently from fp64
# throughout).  Bounds per case on the whole field, borders included: (max |difference| in pixels, ||difference|| / ||flow||).
# Worst measured on one MI355X, in the order of CASES: 3.5e-6 / 3.0e-7, 1.09e-5 / 1.21e-6, 9.8e-6 / 8.3e-7, 5.8e-6 / 4.1e-7,
# 1.08e-5 / 1.49e-6, 1.5e-6 / 3.7e-7, 1.56e-4 / 4.9e-6, 3.8e-5 / 2.5e-6, 2.0e-6 / 2.6e-7: every bound at least 2x above.


def _gray_clip(fs, H, W, seed):
    clip, masks = MP.synthetic_tracking_clip(fs, H, seed=seed, width=W)
    return FB.gray_u8(clip.numpy()), masks.numpy()


def _kernel_flow(frames, pairs, **kw):
    return ops.farneback_flow(torch.from_numpy(np.ascontiguousarray(frames)).to(DEV), pairs, **kw).cpu().numpy()


def test_gray_bit_equal_to_torch_cast():
    rng = np.random.default_rng(7)
    clip = (rng.normal(size=(4, 3, 37, 53)) * 1.5).astype(np.float32)
    clip[0, 0, 0, :6] = [-1.7, 2.5, -0.5, 1.0, 0.999, -300.2]
    g = ops.flow_gray_u8(torch.from_numpy(clip).to(DEV)).cpu().numpy()
    v = (torch.from_numpy(clip) * 255).type(torch.uint8).numpy().astype(np.int64)
    assert np.array_equal(g, ((v[:, 0] * 4899 + v[:, 1] * 9617 + v[:, 2] * 1868 + 8192) >> 14).astype(np.uint8))
    assert np.array_equal(g, FB.gray_u8(clip))


@pytest.mark.parametrize("H,W,poly_n", [(64, 80, 5), (37, 53, 7)])
def test_level0_image_and_expansion(H, W, poly_n):
    # the last level the call computes is level 0: its images and expansions stay in the workspace (farneback.hip's layout)
    frames = np.stack([smooth_texture(H, W, seed=1), _gray_clip(2, 64, 80, 3)[0][1][:H, :W]])
    F, P = 2, 1
    nb = _lib.load().tt_farneback_workspace_bytes(F, P, H, W, 0.5, 3)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    ops.farneback_flow(torch.from_numpy(frames).to(DEV), [(0, 1)], poly_n=poly_n, workspace=ws)
    al = lambda b: (b + 255) // 256 * 256   # noqa: E731
    HW = H * W
    img = ws[al(4 * HW * F):al(4 * HW * F) + 4 * HW * F].view(torch.float32).view(F, H, W).cpu().numpy()
    off = 2 * al(4 * HW * F) + al(12 * HW * F)
    R = ws[off:off + 20 * HW * F].view(torch.float32).view(F, H, W, 5).cpu().numpy()
    for f in range(F):
        I = FB.level_image(frames[f], 0.5, 0, (H, W))
        assert np.abs(img[f] - I).max() <= 1e-4 * max(1.0, np.abs(I).max())
        Rr = FB.poly_exp(I, poly_n, 1.2)
        assert np.abs(R[f] - Rr).max() <= 2e-5 * np.abs(Rr).max()


CASES = [  # (name, H, W, kwargs, kind, (max_abs bound, rel_l2 bound))
    ("224sq", 224, 224, {}, "smooth", (1e-5, 1e-6)),                                        # 2 levels
    ("224sq_clip", 224, 224, {}, "clip", (3e-5, 3e-6)),
    ("480x854", 480, 854, {}, "smooth", (3e-5, 2e-6)),                                      # 3 levels, 213.5 -> 214, 106.75 -> 107
    ("97x131_n7_w9_i2", 97, 131, dict(poly_n=7, winsize=9, iterations=2, poly_sigma=1.5), "smooth", (2e-5, 1e-6)),
    ("97x131_clip_i1", 97, 131, dict(iterations=1), "clip", (3e-5, 4e-6)),
    ("20x50_nolevel", 20, 50, dict(iterations=3), "smooth", (1e-5, 1e-6)),                  # too small for any level
    ("64x80_w1", 64, 80, dict(winsize=1), "smooth", (5e-4, 2e-5)),                          # OpenCV's winsize-1 running-sum start
    ("128x96_w4_i1_n7", 128, 96, dict(winsize=4, iterations=1, poly_n=7), "clip", (1e-4, 1e-5)),
    ("72x200_s08", 72, 200, dict(pyr_scale=0.8, levels=5), "smooth", (1e-5, 1e-6)),
]


def _case_frames(H, W, kind):
    if kind == "smooth":
        return np.stack([smooth_texture(H, W, seed=2), smooth_texture(H, W, (0.8, -1.6), seed=2)])
    g, _ = _gray_clip(2, -(-H // 8) * 8, -(-W // 8) * 8, 5)
    return np.ascontiguousarray(g[:, :H, :W][::-1])   # (new, old) as the reference's call


@pytest.mark.parametrize("name,H,W,kw,kind,bounds", CASES, ids=[c[0] for c in CASES])
def test_flow_matches_restatement(name, H, W, kw, kind, bounds):
    frames = _case_frames(H, W, kind)
    got = _kernel_flow(frames, [(0, 1)], **kw)[0]
    ref = FB.farneback(frames[0], frames[1], **kw)
    d = got.astype(np.float64) - ref
    max_abs = np.abs(d).max()
    rel = np.linalg.norm(d) / max(np.linalg.norm(ref), 1e-30)
    print(f"FLOWERR {name} max_abs {max_abs:.3e} rel_l2 {rel:.3e} |ref| {np.abs(ref).max():.3f}")
    assert max_abs <= bounds[0] and rel <= bounds[1]


def test_known_translation_recovered():
    a, b = smooth_texture(160, 192), smooth_texture(160, 192, (1.3, -0.7))
    f = _kernel_flow(np.stack([a, b]), [(0, 1)])[0][32:-32, 32:-32]
    assert np.all(np.abs(f.reshape(-1, 2).mean(0) - [1.3, -0.7]) < 0.1)
    assert np.quantile(np.abs(f - [1.3, -0.7]).max(-1), 0.9) < 0.25
    c = np.full((2, 64, 80), 77, np.uint8)
    assert np.array_equal(_kernel_flow(c, [(0, 1)]), np.zeros((1, 64, 80, 2), np.float32))


def test_deterministic_and_batch_independent():
    g, _ = _gray_clip(6, 96, 128, 9)
    frames = torch.from_numpy(g).to(DEV)
    pairs = [(j + 1, j) for j in range(5)] + [(0, 5), (3, 3)]
    a = ops.farneback_flow(frames, pairs)
    b = ops.farneback_flow(frames, pairs)
    assert torch.equal(a, b)
    for i, p in enumerate(pairs):
        assert torch.equal(ops.farneback_flow(frames[list(p)].contiguous(), [(0, 1)])[0], a[i])


@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
def test_label_chain_bit_equal(dtype):
    fs, H, W = 25, 96, 128
    g, masks = _gray_clip(fs, H, W, 4)
    flows = ops.farneback_flow(torch.from_numpy(g).to(DEV), MP._clip_pairs(1, fs)).view(1, fs - 1, H, W, 2)
    first = masks[0].astype(dtype)
    got = ops.remap_nearest_labels(torch.from_numpy(first).to(DEV).view(1, H, W), flows).cpu().numpy()[0]
    ref = FB.propagate_chain(first, list(flows[0].cpu().numpy()))
    assert got.dtype == dtype and np.array_equal(got, ref)
    # ties at exactly .5 and reads outside the frame
    rng = np.random.default_rng(1)
    fl = (rng.integers(-8, 9, (2, 3, H, W, 2)) * 0.5).astype(np.float32)
    fl[0, 0, :4, :4] = np.nan
    lab = rng.integers(0, 7, (2, H, W)).astype(dtype)
    got = ops.remap_nearest_labels(torch.from_numpy(lab).to(DEV), torch.from_numpy(fl).to(DEV)).cpu().numpy()
    for n in range(2):
        assert np.array_equal(got[n], FB.propagate_chain(lab[n], list(fl[n])))


def test_interpolate_frames_and_propagate():
    bs, fs, H, W = 2, 4, 64, 96
    g = np.stack([_gray_clip(fs, H, W, 11 + i)[0] for i in range(bs)])
    masks = np.stack([_gray_clip(fs, H, W, 11 + i)[1] for i in range(bs)])
    fl_list = MP.dense_optical_flow(g)
    fl_gpu = MP.dense_optical_flow(torch.from_numpy(g).to(DEV))
    assert len(fl_list) == bs and len(fl_list[0]) == fs - 1 and fl_list[0][0].shape == (H, W, 2) and fl_list[0][0].dtype == np.float32
    assert fl_gpu.shape == (bs, fs - 1, H, W, 2) and fl_gpu.is_cuda
    assert np.array_equal(np.asarray(fl_list), fl_gpu.cpu().numpy())
    assert np.array_equal(fl_list[1][2], MP.calc_optical_flow_farneback(g[1, 3], g[1, 2]))
    batched = MP.calc_optical_flow_farneback(torch.from_numpy(g[:, 1:]).to(DEV), torch.from_numpy(g[:, :-1]).to(DEV))
    assert torch.equal(batched, fl_gpu)
    # interpolate_frames with n_frames > 1: the map coords + float32((f + 1) / n) * flow
    for n_frames in (1, 3, 7):
        outs = MP.interpolate_frames(masks[0, 0], fl_list[0][0], n_frames)
        assert len(outs) == n_frames
        for f, o in enumerate(outs):
            assert o.dtype == masks.dtype and np.array_equal(o, FB.remap_nearest(masks[0, 0], fl_list[0][0], (f + 1) / n_frames))
    ann = torch.from_numpy(masks)
    pred = MP.propagate(fl_list, ann)
    assert pred.dtype == torch.uint8 and pred.shape == (bs, fs - 1, H, W) and not pred.is_cuda
    for i in range(bs):
        assert np.array_equal(pred[i].numpy(), FB.propagate_chain(masks[i, 0], fl_list[i]).astype(np.uint8))
    assert torch.equal(MP.propagate(fl_gpu, ann).cpu(), pred)


def test_propagate_clip_optical_flow():
    clip, masks = MP.synthetic_tracking_clip(5, 64, seed=2, width=96)
    pred = MP.propagate_clip_optical_flow(clip.to(DEV), masks[0].to(DEV))
    assert pred.shape == (4, 64, 96) and pred.dtype == torch.int64 and pred.is_cuda
    g = FB.gray_u8(clip.numpy())
    flows = [FB.farneback(g[j + 1], g[j]) for j in range(4)]
    k_flows = ops.farneback_flow(torch.from_numpy(g).to(DEV), MP._clip_pairs(1, 5)).cpu().numpy()
    assert np.array_equal(pred.cpu().numpy(), FB.propagate_chain(masks[0].numpy(), list(k_flows)))
    agree = np.mean(pred.cpu().numpy() == FB.propagate_chain(masks[0].numpy(), flows))
    assert agree > 0.99   # the restatement's own flows move a few labels at most


@pytest.mark.parametrize("extra,size", [(["--input_resolution", "64"], (64, 64)), (["--frame_size", "48", "80"], (48, 80))])
def test_cli(extra, size, capsys):
    argv = ["--dataset", "synthetic", "--use_optical_flow", "True", "--num_clips", "2", "--num_frames", "5", "--davis_metrics"] + extra
    j = MP.mask_propagation(MP.build_parser().parse_args(argv))
    out = capsys.readouterr().out
    assert "J&F-Mean" in out and "mean J over 2 clips" in out
    assert 0.0 <= j <= 1.0
    H, W = size
    js = []
    for i in range(2):
        clip, masks = MP.synthetic_tracking_clip(5, H, seed=i + 1, width=W)
        masks = (masks > 0).long()
        pred = MP.propagate_clip_optical_flow(clip.to(DEV), masks[0].to(DEV))
        js.append(MP.jaccard(pred, masks[1:].to(DEV), int(masks.max()) + 1)[0])
    assert j == sum(js) / len(js)
