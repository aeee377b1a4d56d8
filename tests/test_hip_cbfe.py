"""Cluster-based foreground extraction on the GPU (N6): the statistics kernel against torch.bincount, the precision and cut kernels bit
for bit against the reference's outputs (tests/golden/cbfe.npz), k-means on virtual upsampled points against the materialised run,
the memory bound of get_foreground_masks, the masked Evaluator and an end-to-end run with a planted foreground."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_cbfe_host import golden_maps, unpack_mask
from timetuning_amd import cluster_based_foreground_extraction as CB, hip_ops as ops, synth
from timetuning_amd.clustering import Kmeans, nearest_index_table
from timetuning_amd.evaluation import Evaluator
from timetuning_amd.linear_finetune import synthetic_segmentation

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)


def _bincount_stats(cl, at, gt, k, ignore):
    M = cl.shape[0]
    cl, at, gt = cl.view(M, -1), at.view(M, -1), gt.view(M, -1)
    fg = (gt != 0) if ignore < 0 else ((gt != 0) & (gt != ignore))
    out = torch.zeros((M, k, 3), dtype=torch.int64)
    for m in range(M):
        out[m, :, 0] = torch.bincount(cl[m], minlength=k)
        out[m, :, 1] = torch.bincount(cl[m][at[m] == 1], minlength=k)
        out[m, :, 2] = torch.bincount(cl[m][fg[m]], minlength=k)
    return out, fg.sum(1)


@pytest.mark.parametrize("ignore", [-1, 255])
@pytest.mark.parametrize("M,R,k", [(6, 100, 300), (3, 37, 4096), (5, 61, 13), (40, 100, 60), (2, 1, 1)])
def test_cluster_stats_equal_bincount(M, R, k, ignore):
    rng = np.random.default_rng(M * 7919 + R * 31 + k)
    cl = torch.from_numpy(rng.integers(0, k, (M, R, R)))
    at = torch.from_numpy(rng.integers(0, 3, (M, R, R)))       # 2s are not attention
    gt = torch.from_numpy(rng.choice([0, 0, 3, 7, 255], (M, R, R)))
    stats, gt_fg = ops.cbfe_cluster_stats(cl.to(dev).view(M, -1), at.to(dev).view(M, -1), gt.to(dev).view(M, -1), k, ignore=ignore)
    ref, ref_fg = _bincount_stats(cl, at, gt, k, ignore)
    assert torch.equal(stats.cpu().long(), ref) and torch.equal(gt_fg.cpu().long(), ref_fg)


def test_cluster_stats_out_of_range_raises():
    cl = torch.zeros((2, 64), dtype=torch.int64, device=dev)
    gt = torch.zeros_like(cl)
    for bad in (5, -1):
        c = cl.clone()
        c[1, 17] = bad
        with pytest.raises(ops.ClusterRangeError):
            ops.cbfe_cluster_stats(c, None, gt, 5)
        with pytest.raises(ops.ClusterRangeError):
            ops.cbfe_apply_fg(c, torch.ones(5, dtype=torch.uint8, device=dev))
    with pytest.raises(AssertionError):   # get_cluster_precs: as the reference, an id that never occurs
        CB.get_cluster_precs(cl, gt, 2)


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("k", [60, 300])
def test_precs_and_cut_jaccards_bit_equal_the_reference(golden, k):
    g = golden("cbfe")
    p = f"k{k}_"
    cl, at, gt = golden_maps(g, k)
    precs = CB.get_cluster_precs(cl.to(dev), at.to(dev), k)
    assert _bits_equal(precs, g[p + "precs"])
    M = cl.shape[0]
    stats, gt_fg = ops.cbfe_cluster_stats(cl.to(dev).view(M, -1), None, gt.to(dev).view(M, -1), k)
    starts = g[p + "cut_start"].astype(np.int32)
    jac = ops.cbfe_cut_jaccard(stats, gt_fg, torch.from_numpy(g[p + "order"]).to(dev), torch.from_numpy(starts).to(dev))
    assert _bits_equal(jac.cpu().double().numpy(), g[p + "cut_jac"])
    res = CB.find_good_threshold(cl.to(dev), gt.to(dev), precs, k)
    assert [r[1] for r in res] == g[p + "cut_start"].tolist()
    assert _bits_equal([r[2] for r in res], g[p + "cut_jac"]) and _bits_equal([r[0] for r in res], g[p + "cut_prec"])


@pytest.mark.parametrize("k", [60, 300])
def test_threshold_soft_mask_and_eval_jac_bit_equal_the_reference(golden, k):
    g = golden("cbfe")
    p = f"k{k}_"
    cl, at, gt = golden_maps(g, k)
    vcl, vat, vgt = golden_maps(g, k, val=True)
    obj = CB.ClusterBasedForegroundExtraction.__new__(CB.ClusterBasedForegroundExtraction)
    torch.nn.Module.__init__(obj)
    obj.k_fg_extraction, obj.eval_resolution, obj.device = k, int(g["cfg"][1]), "cuda"
    th = obj.get_tuned_threshold(at[:, None].to(dev), gt[:, None].to(dev), cl[:, None].to(dev))
    assert th == g[p + "threshold"]
    obj.create_overclustering_maps = lambda features: vcl[:, None].to(dev)
    mask = obj.create_soft_masks(vat[:, None].to(dev), vgt[:, None].to(dev), None, th)
    assert mask.dtype == torch.int64 and torch.equal(mask.cpu(), unpack_mask(g, k))
    assert _bits_equal(CB.eval_jac(vgt.to(dev), mask, with_boundary=True), g[p + "eval_jac_boundary"])
    assert _bits_equal(CB.eval_jac(vgt.to(dev), mask, with_boundary=False), g[p + "eval_jac_no_boundary"])


def test_nan_case(golden):
    g = golden("cbfe")
    cl, at, gt = (torch.from_numpy(g[n].astype(np.int64)).to(dev) for n in ("nan_clusters", "nan_attn", "nan_gt"))
    precs = CB.get_cluster_precs(cl, at, 4)
    assert _bits_equal(precs, g["nan_precs"])
    res = CB.find_good_threshold(cl, gt, precs, 4)
    assert [r[1] for r in res] == g["nan_cut_start"].tolist()
    assert np.isnan(g["nan_cut_jac"]).all() and all(np.isnan(r[2]) for r in res)
    obj = CB.ClusterBasedForegroundExtraction.__new__(CB.ClusterBasedForegroundExtraction)
    fg = obj.make_post_matching_maps(cl, 0.5, precs)
    assert np.isnan(g["nan_eval_jac"]) and np.isnan(CB.eval_jac(gt, fg, with_boundary=True))


def _materialised(tokens, R):
    M, n, d = tokens.shape
    g = int(round(n ** 0.5))
    iy, ix = nearest_index_table(g, R)
    idx = torch.from_numpy((iy.astype(np.int64)[:, None] * g + ix.astype(np.int64)[None, :]).reshape(-1)).to(tokens.device)
    return tokens[:, idx, :].reshape(M * R * R, d).contiguous()


@pytest.mark.parametrize("M,g,R,k,d", [(2, 7, 20, 8, 8), (4, 14, 40, 10, 8), (3, 28, 100, 30, 8), (2, 28, 100, 300, 50)])
def test_kmeans_on_virtual_points_is_the_materialised_run(M, g, R, k, d):
    tokens = torch.from_numpy(synth.normal(f"vk.{M}.{g}.{R}", (M, g * g, d))).to(dev)
    # both regimes: all points trained on (n <= 256 k) and the subsample
    assert (M * R * R <= 256 * k) == (M == 2)   # (2, 28, 100, 300, 50): the CBFE over-clustering's k and d
    ref = Kmeans(d, k, niter=50, nredo=5, seed=1)
    pts = _materialised(tokens, R)
    ref.train(pts)
    ref_labels = ref.assign(pts)[1].view(M, R * R)
    km = Kmeans(d, k, niter=50, nredo=5, seed=1)
    km.train_upsampled(tokens, R)
    labels = km.assign_upsampled(tokens, R)
    assert np.array_equal(km.centroids.view(np.int32), ref.centroids.view(np.int32))
    assert torch.equal(labels, ref_labels)
    km2 = Kmeans(d, k, niter=50, nredo=5, seed=1)   # tokens on the host: only the subsample moves
    km2.train_upsampled(tokens.cpu(), R)
    assert np.array_equal(km2.centroids.view(np.int32), ref.centroids.view(np.int32))


def test_nearest_upsample_labels_kernel():
    for g, R in ((28, 100), (14, 37), (60, 100)):
        tok = torch.from_numpy(np.random.default_rng(g + R).integers(0, 1 << 30, (3, g * g)).astype(np.int32))
        iy, ix = nearest_index_table(g, R, device=dev)
        out = ops.nearest_upsample_labels(tok.to(dev), iy, ix)
        ref = F.interpolate(tok.double().view(3, 1, g, g), size=(R, R), mode="nearest").long().view(3, R * R)
        assert torch.equal(out.cpu(), ref)


def test_get_foreground_masks_memory():
    Mtr, Mva, g, R, D, k = 256, 64, 28, 100, 64, 300
    inputs = {}
    for name, M, seed in (("train", Mtr, 1), ("val", Mva, 2)):
        feats = torch.from_numpy(synth.normal(f"mem.f.{name}", (M, 1, g * g, D))).to(dev)
        attn = (torch.from_numpy(synth.normal(f"mem.a.{name}", (M, 1, g, g))) > 0).float().to(dev)
        _, y = synthetic_segmentation(M, R, 21, seed=seed)
        inputs[name] = (feats, attn, (y * 255).round().long().to(dev))
    obj = CB.ClusterBasedForegroundExtraction.__new__(CB.ClusterBasedForegroundExtraction)
    torch.nn.Module.__init__(obj)
    obj.k_fg_extraction, obj.eval_resolution, obj.eval_feature_dim, obj.device = k, R, 50, "cuda"
    obj.train_loader, obj.val_loader = "train", "val"
    obj.extract_dataset_features_attentions = lambda loader: inputs[loader]
    # per-process workspaces allocated at their first use are not CBFE's: the HIP GEMMs' K-split buffer and torch's own BLAS workspace
    # (about 128 MiB, taken by the small matrix-vector product in clustering.normalize_and_transform)
    ops.ksplit_workspace()
    torch.ones((2, 2), device=dev) @ torch.ones(2, device=dev)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    masks, ann, feats = obj.get_foreground_masks("val")
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    materialised_train = Mtr * 50 * R * R * 4
    assert materialised_train == 512 * 10 ** 6
    assert peak < materialised_train / 4, peak
    assert masks.shape == (Mva, R, R) and ann.shape == (Mva, 1, R, R) and feats.shape == (Mva, 1, 50, R, R) and not feats.is_cuda


class _PlantedModel:
    """Features and attention read off the image: a token is a fixed projection of its patch means, and the cls attention row puts
    70% of the mass on the patches whose channel 2 carries the planted foreground (+3), 30% on the others."""
    spatial_resolution = 14

    def __init__(self, D=64, heads=2, patch=8):
        self.w = torch.from_numpy(synth.normal("planted.w", (3, D), 1.0)).to(dev)
        self.heads, self.patch = heads, patch

    def __call__(self, x, use_head=False):
        Fr = x.shape[0]
        pm = F.avg_pool2d(x, self.patch)                           # [F, 3, g, g]
        g = pm.shape[-1]
        tok = pm.flatten(2).transpose(1, 2)                        # [F, g*g, 3]
        feats = torch.tanh(0.5 * tok @ self.w)
        fg = tok[..., 2] > 1.5
        n_fg = fg.sum(1, keepdim=True).clamp(min=1).float()
        n_bg = (~fg).sum(1, keepdim=True).clamp(min=1).float()
        row = torch.where(fg, 0.7 / n_fg, 0.3 / n_bg)
        probs = torch.zeros((Fr, self.heads, g * g + 1, g * g + 1), device=x.device)
        probs[:, :, 0, 1:] = row[:, None] * 0.99
        probs[:, :, 0, 0] = 0.01
        return feats.contiguous(), probs

    def eval(self):
        return self

    @property
    def feature_extractor(self):   # what the Evaluator looks for on a model that is not a FeatureExtractor
        return self


def _planted_data(n, S, seed):
    """One large disc per image (about half of it: Pascal-like object sizes), a 255 band at its border, channel 2 planted."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    xs, ys = [], []
    for _ in range(n):
        cy, cx = S * (0.5 + 0.1 * rng.uniform(-1, 1)), S * (0.5 + 0.1 * rng.uniform(-1, 1))
        r = S * (0.4 + 0.03 * rng.uniform(-1, 1))
        d = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
        lab = np.where(d < r, int(rng.integers(1, 21)), 0)
        lab[np.abs(d - r) < 1.5] = 255
        img = 0.5 * rng.standard_normal((3, S, S)).astype(np.float32)
        img[2] += 3.0 * (d < r)
        xs.append(img)
        ys.append(lab)
    x = torch.from_numpy(np.stack(xs).astype(np.float32))
    y01 = torch.from_numpy(np.stack(ys)[:, None].astype(np.uint8)).float() / 255
    return x, y01


def test_end_to_end_planted_foreground():
    S, R, k = 112, 56, 40
    model = _PlantedModel()
    x_tr, y_tr = _planted_data(24, S, seed=5)
    x_va, y_va = _planted_data(12, S, seed=6)
    train = [(x_tr[i:i + 8], y_tr[i:i + 8].clone()) for i in range(0, 24, 8)]
    val = [(x_va[i:i + 6], y_va[i:i + 6].clone()) for i in range(0, 12, 6)]
    cbfe = CB.ClusterBasedForegroundExtraction(model, k, R, 16, train, val)
    masks, ann, feats = cbfe.get_foreground_masks("val")
    jac = CB.eval_jac(ann.flatten(0, 1), masks, with_boundary=True)
    assert jac > 0.5, jac
    eval_loader = [(x[:, None], (y * 255).round().long()) for x, y in ((x_va[i:i + 6], y_va[i:i + 6]) for i in range(0, 12, 6))]
    ev = Evaluator(model, eval_loader, num_prototypes=21, fg_masks=masks)
    s1 = ev.evaluate(evaluation_protocol="dataset-wise", eval_resolution=R, num_clusters=21, use_mask=True)
    ev2 = Evaluator(model, eval_loader, num_prototypes=21)
    s2 = ev2.evaluate(evaluation_protocol="dataset-wise", eval_resolution=R, num_clusters=21, use_mask=True)
    assert 0.0 <= s1 <= 1.0 and 0.0 <= s2 <= 1.0
    # the masked features are exactly features * nearest(mask)
    f, gg = ev._features(x_va[:, None])
    out = ev._apply_fg_masks(f, gg)
    small = F.interpolate(masks.view(12, 1, R, R).float(), size=(gg, gg), mode="nearest").view(12, 1, gg * gg, 1)
    assert torch.equal(out, f * small)


def test_main_runs_on_synthetic_data(tmp_path):
    score = CB.main(["--dataset", "synthetic", "--model_path", "", "--input_resolution", "224", "--k_fg_extraction", "20",
                     "--num_train_images", "8", "--num_val_images", "4", "--batch_size", "4"])
    assert 0.0 <= score <= 1.0
