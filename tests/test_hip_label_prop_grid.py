"""GPU checks of N9, label propagation on rectangular token grids: tt_label_propagate_grid_maps against an fp64 restatement of the
reference's label_propagation / propagate_labels (mask_propagation.py:377-496) generalised to gh x gw grids, beyond the square entry's
4 096-candidate cap and with the unrestricted variant (radius 0); agreement with the square entry where that one runs;
tt_upsample_argmax_hw against torch; propagate_clip on a rectangular clip end to end; and the command-line driver."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from oracle import timet_oracle as O
from timetuning_amd import _lib, synth
from timetuning_amd import hip_ops as ops
from timetuning_amd import mask_propagation as MP

pytestmark = pytest.mark.gpu


def ref_maps(xn, seed, grid, n_last, radius, topk, temperature=0.1):
    """The reference's propagation in fp64 on a gh x gw grid: xn [fs, n, D] tokens (already normalised, as the kernel takes them), seed
    [n, K] -> [fs-1, n, K].  Context of frame t = frame 0 plus frames [max(1, t - n_last), t) (the reference's queue; n_last 0 leaves
    frame 0 alone); affinity exp(sim / T) times restrict_neighborhood(gh, gw, r) unless r == 0; keep aff >= the k-th largest of each
    column (ties kept, masked zeros count), normalise the column, fp64 weighted sum of the label rows."""
    gh, gw = grid
    n = gh * gw
    xn, seed = xn.double(), seed.double()
    mask = O.restrict_neighborhood(gh, gw, radius).double()
    maps = [seed]
    for t in range(1, xn.shape[0]):
        ctx = [0] + list(range(max(1, t - n_last), t))
        aff = torch.exp(torch.einsum("qd,csd->cqs", xn[t], xn[ctx]) / temperature)   # [c, n_tar, n_src]
        if radius > 0:
            aff = aff * mask
        aff = aff.transpose(2, 1).reshape(-1, n)                                       # [c * n_src, n_tar]
        kth = torch.topk(aff, dim=0, k=topk).values.min(0).values
        aff[aff < kth] = 0
        aff = aff / aff.sum(0, keepdim=True)
        maps.append(aff.t() @ torch.cat([maps[f] for f in ctx], 0))
    return torch.stack(maps[1:])


def quantised_tokens(fs, bs, n, D, seed, dup=False):
    """Tokens with entries in {-2..2} / 8 and D = 16: every similarity is a multiple of 1/64 in [-1, 1], exact in the kernel's fp32
    GEMM, so the top-k selects the same sources as the fp64 restatement and exact ties are frequent.  ``dup``: every third token of
    each frame repeats its first token (identical rows tie in every context)."""
    x = np.random.default_rng(seed).integers(-2, 3, (fs, bs, n, D)).astype(np.float32) / 8
    if dup:
        x[:, :, ::3] = x[:, :, :1]
    return torch.from_numpy(x)


def seeds(bs, n, K, seed):
    return torch.softmax(torch.from_numpy(np.random.default_rng(seed + 1).normal(size=(bs, n, K)) * 2), -1).float()


def check_against_ref(grid, n_last, radius, topk, K, bs, fs=9, seed=0, dup=False):
    n = grid[0] * grid[1]
    xn = quantised_tokens(fs, bs, n, 16, seed, dup)
    s0 = seeds(bs, n, K, seed)
    got = ops.label_propagate_grid_maps(xn.cuda(), s0.cuda(), grid, n_last, radius, topk, 0.1).cpu()
    assert got.shape == (fs - 1, bs, n, K) and got.dtype == torch.float64
    for b in range(bs):
        want = ref_maps(xn[:, b], s0[b], grid, n_last, radius, topk)
        assert rel_err(got[:, b], want) < 1e-6, (grid, n_last, radius, topk, K, bs, b)
        top2 = want.topk(2, dim=-1).values
        clear = (top2[..., 0] - top2[..., 1]) > 1e-6
        assert torch.equal(got[:, b].argmax(-1)[clear], want.argmax(-1)[clear])
    return got


# (n_last, topk, K, bs): every value of each appears against every (grid, radius)
_COMBOS = [(0, 1, 2, 1), (1, 5, 21, 3), (4, 5, 2, 3), (7, 1, 21, 1)]


@pytest.mark.parametrize("grid", [(5, 9), (9, 5), (7, 23), (14, 14)])
@pytest.mark.parametrize("radius", [0, 1, 3, 12])
def test_grid_maps_vs_fp64_restatement(grid, radius):
    for i, (n_last, topk, K, bs) in enumerate(_COMBOS):
        check_against_ref(grid, n_last, radius, topk, K, bs, seed=i)


def test_grid_maps_duplicated_tokens_tie():
    for grid, radius in (((7, 23), 3), ((9, 5), 0)):
        check_against_ref(grid, 4, radius, 5, 21, 2, seed=7, dup=True)


def test_grid_maps_beyond_candidate_cap():
    """r = 12 with n_last 7 on 30 x 30 (25 x 25 x 8 = 5 000 candidates, refused by the square entry) and r = 0 on 30 x 53."""
    xn = quantised_tokens(9, 1, 900, 16, 3)
    with pytest.raises(_lib.HipLibraryError):
        ops.label_propagate_maps(xn.cuda(), seeds(1, 900, 5, 3).cuda(), 7, 12, 5, 0.1)
    assert not MP.square_entry_accepts((30, 30), 9, 7, 12)
    check_against_ref((30, 30), 7, 12, 5, 5, 1, fs=9, seed=3)
    check_against_ref((30, 53), 4, 0, 5, 5, 1, fs=6, seed=4)


@pytest.mark.parametrize("g,n_last,radius,topk,K,bs,fs", [(14, 7, 6, 5, 21, 2, 9), (14, 4, 1, 1, 2, 1, 5), (14, 0, 3, 5, 7, 3, 4),
                                                         (28, 4, 12, 5, 5, 1, 7), (10, 1, 12, 5, 3, 2, 6)])
def test_grid_entry_equals_square_entry(g, n_last, radius, topk, K, bs, fs):
    """Where the square entry runs, the new one gives the same labels and maps within 1e-6 (same similarities; only the summation order
    of the column sum and of the fp64 gather differs)."""
    assert MP.square_entry_accepts((g, g), fs, n_last, radius)
    n = g * g
    x = torch.from_numpy(synth.normal(f"lpg.sq.{g}.{n_last}", (fs, bs, n, 64)))
    xn = ops.l2norm_fwd(x.reshape(-1, 64).cuda()).view(fs, bs, n, 64)
    s0 = seeds(bs, n, K, g).cuda()
    old = ops.label_propagate_maps(xn, s0, n_last, radius, topk, 0.1)
    new = ops.label_propagate_grid_maps(xn, s0, (g, g), n_last, radius, topk, 0.1)
    assert rel_err(new.cpu(), old.cpu()) < 1e-6
    assert torch.equal(new.argmax(-1), old.argmax(-1))


def test_grid_maps_errors():
    xn = quantised_tokens(3, 1, 45, 16, 0).cuda()
    s0 = seeds(1, 45, 3, 0).cuda()
    with pytest.raises(_lib.HipLibraryError):
        ops.label_propagate_grid_maps(xn, s0, (5, 9), 8, 3, 5, 0.1)      # n_last > 7
    with pytest.raises(ValueError):
        ops.label_propagate_grid_maps(xn, s0, (9, 6), 4, 3, 5, 0.1)      # grid does not hold the tokens
    with pytest.raises(_lib.HipLibraryError):
        ops.label_propagate_grid_maps(xn[:, :, :, :0].contiguous(), s0, (5, 9), 4, 3, 5, 0.1)   # D = 0
    lib = _lib.load()
    ws = torch.empty(16, dtype=torch.uint8, device="cuda")
    maps = torch.empty((2, 1, 45, 3), dtype=torch.float64, device="cuda")
    rc = lib.tt_label_propagate_grid_maps(xn.data_ptr(), s0.data_ptr(), maps.data_ptr(), 1, 3, 5, 9, 16, 3, 4, 3, 5, 0.1, 0, ws.data_ptr(),
                                          ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and "workspace too small" in lib.tt_last_error().decode()
    with pytest.raises(_lib.HipLibraryError):
        ops.upsample_argmax_hw(torch.zeros((1, 45, 0), dtype=torch.float64, device="cuda"), (5, 9), (7, 4))


@pytest.mark.parametrize("grid,size,K", [((30, 53), (480, 848), 5), ((5, 9), (7, 4), 2), ((9, 5), (20, 11), 21), ((7, 23), (7, 23), 3),
                                         ((14, 14), (224, 160), 4)])
def test_upsample_argmax_hw_vs_torch(grid, size, K):
    """Up- and down-sampling, non-integer factors, rows and columns scaled separately; the tie rule of test_upsample_argmax_vs_torch."""
    gh, gw = grid
    maps = torch.from_numpy(np.random.default_rng(gh * 100 + gw).random((3, gh * gw, K)))
    up = F.interpolate(maps.transpose(1, 2).reshape(3, K, gh, gw), size=size, mode="bilinear", align_corners=False)
    want = up.argmax(1)
    top2 = up.topk(2, dim=1).values
    got = ops.upsample_argmax_hw(maps.cuda(), grid, size).cpu()
    assert got.shape == (3, *size) and got.dtype == torch.int64
    mism = got != want
    assert not (mism & ((top2[:, 0] - top2[:, 1]) > 1e-12)).any()
    assert mism.float().mean() < 1e-3


def test_upsample_argmax_hw_square_equals_square_entry():
    maps = torch.from_numpy(np.random.default_rng(5).random((2, 196, 6))).cuda()
    assert torch.equal(ops.upsample_argmax_hw(maps, (14, 14), (100, 100)), ops.upsample_argmax(maps, 100))


def _tiny_extractor():
    from timetuning_amd.models import FeatureExtractor

    return FeatureExtractor("dino-s16", "", [64, 32], vit_cfg=synth.ARCHS["tiny-s16"], return_attention=False).cuda().eval()


def test_propagate_clip_rectangular_vs_oracle():
    """A 96 x 160 clip (6 x 10 tokens) through propagate_clip, against the oracle extractor's features put through the fp64 restatement,
    the nearest seed resize, the bilinear upsampling to 96 x 160 and the arg-max."""
    fe = _tiny_extractor()
    fs, H, W, C = 6, 96, 160, 3
    clip, masks = MP.synthetic_tracking_clip(fs, H, seed=2, width=W)
    pred = MP.propagate_clip(fe, clip.cuda(), masks[0].cuda(), 4, 12, 5, (H, W), C)
    assert pred.shape == (fs - 1, H, W) and pred.dtype == torch.int64
    oracle = O.FeatureExtractorOracle(synth.ARCHS["tiny-s16"], {k: v.detach().cpu() for k, v in fe.backbone.state_dict().items()})
    with torch.no_grad():
        feats, _ = oracle(clip, use_head=False, faithful=False)
    gh, gw = H // 16, W // 16
    seed = F.interpolate(O.to_one_hot(masks[0].unsqueeze(0), C).unsqueeze(0).double(), size=(gh, gw), mode="nearest")
    maps = ref_maps(F.normalize(feats.double(), dim=-1), seed[0].reshape(C, -1).t(), (gh, gw), 4, 12, 5)
    up = F.interpolate(maps.transpose(1, 2).reshape(fs - 1, C, gh, gw), size=(H, W), mode="bilinear", align_corners=False)
    want = up.argmax(1)
    mism = pred.cpu() != want
    assert mism.float().mean().item() <= 0.01
    j_gpu, _ = MP.jaccard(pred, masks[1:].cuda(), C)
    assert abs(j_gpu - O.jaccard(want, masks[1:], C)) < 0.02


def test_propagate_clip_square_routes_to_square_entries():
    """A 224 x 224 clip gives the tensor the square entries give (the code path of propagate_clip before N9)."""
    fe = _tiny_extractor()
    clip, masks = MP.synthetic_tracking_clip(5, 224, seed=1)
    pred = MP.propagate_clip(fe, clip.cuda(), masks[0].cuda(), 4, 12, 5, 224, 3)
    feats, _ = fe(clip.cuda(), use_head=False)
    seed = F.interpolate(MP.to_one_hot(masks[0].unsqueeze(0).cuda(), 3).unsqueeze(0).double(), size=(14, 14), mode="nearest")
    xn = ops.l2norm_fwd(feats.reshape(-1, feats.shape[-1]).contiguous().float()).view(5, 1, 196, -1)
    maps = ops.label_propagate_maps(xn, seed.reshape(3, 196).t().contiguous().float().view(1, 196, 3), 4, 12, 5, 0.1)
    assert torch.equal(pred, ops.upsample_argmax(maps.view(4, 196, 3), 224))
    rect = MP.propagate_labels(4, 12, 5, fe, feats, seed, features_exist=True, grid=(14, 14))
    assert all(torch.equal(m.reshape(3, -1).t(), maps[i, 0]) for i, m in enumerate(rect))


def test_cli_frame_size_and_unrestricted():
    base = ["--dataset", "synthetic", "--model_path", "", "--num_frames", "4", "--num_clips", "1"]
    args = MP.build_parser().parse_args(base + ["--frame_size", "96", "160", "--davis_metrics"])
    assert np.isfinite(MP.mask_propagation(args))
    args = MP.build_parser().parse_args(base + ["--size_mask_neighborhood", "0", "--input_resolution", "96"])
    assert np.isfinite(MP.mask_propagation(args))
    with pytest.raises(ValueError):
        MP.mask_propagation(MP.build_parser().parse_args(base + ["--frame_size", "96", "150"]))
