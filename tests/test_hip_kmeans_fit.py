"""N13 on the GPU: the fused, batched k-means fit (``tt_kmeans_fit_batched``), the batched assignment (``tt_kmeans_assign_batched``),
``clustering.KmeansBatch`` and the frame-wise / sample-wise routes of ``cluster_features`` - held bit for bit to the loop of
``clustering.Kmeans`` over ``tt_kmeans_assign`` / ``tt_kmeans_accumulate``, which stays in the tree unchanged."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import timet_oracle as O
from timetuning_amd import synth

pytestmark = pytest.mark.gpu

B, NITER, NREDO = 3, 7, 3
SPREAD = 2.0   # blob centres are N(0, SPREAD^2) per column, the points N(0, 1) about them: neighbours overlap, so points migrate
# (n, d, k): n either side of the accumulation's 128-point block edges, d either side of 16 and at 64, k from 1 to 64
SHAPES = [(1, 1, 1), (127, 3, 2), (128, 16, 5), (129, 17, 5), (257, 50, 10), (1000, 64, 21), (2560, 50, 10), (700, 50, 64)]


@pytest.fixture(scope="module")
def ops():
    from timetuning_amd import hip_ops

    return hip_ops


def dev(a):
    return torch.as_tensor(a).cuda().contiguous()


def blobs(n, d, k, tag=""):
    """B problems of n points in k Gaussian blobs (point p in blob p % k; SPREAD apart), and NREDO rows of k distinct initial points: each
    seed owns itself in the first assignment, and (checked with the fp64 oracle when these inputs were chosen) no cluster of any
    problem and redo is empty in any of the NITER iterations."""
    x = np.stack([np.stack([synth.normal(f"kf.c.{n}.{d}.{k}.{b}{tag}", (k, d))[p % k] * SPREAD for p in range(n)])
                  + synth.normal(f"kf.x.{n}.{d}.{k}.{b}{tag}", (n, d)) for b in range(B)]).astype(np.float32)
    init = [(r * k + np.arange(k)) % n for r in range(NREDO)]   # one seed in every blob
    return x, init


def count_splits(km):
    splits = []
    split = km._split_empty
    km._split_empty = lambda cent, counts, n: splits.append(split(cent, counts, n))
    return splits


_LOOP = {}


def loop_fit(n, d, k):
    """The loop path on every problem of a shape, run once per module: [(Kmeans, its _split_empty calls)] and the inputs."""
    from timetuning_amd.clustering import Kmeans

    if (n, d, k) not in _LOOP:
        x, init = blobs(n, d, k)
        xd = dev(x)
        fits = []
        for b in range(B):
            km = Kmeans(d, k, niter=NITER, nredo=NREDO, seed=1, max_points_per_centroid=10 ** 6)   # no subsampling: init indexes x itself
            splits = count_splits(km)
            km.train(xd[b], init_indices=init)
            fits.append((km, splits))
        _LOOP[(n, d, k)] = (x, init, xd, fits)
    return _LOOP[(n, d, k)]


# ---- 1. bit equality with the loop ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,d,k", SHAPES)
def test_fused_fit_equals_the_loop_bit_for_bit(ops, n, d, k):
    from timetuning_amd.clustering import KmeansBatch

    x, init, xd, fits = loop_fit(n, d, k)
    assert ops.kmeans_fit_shape_ok(n, d, k)
    kb = KmeansBatch(d, k, niter=NITER, nredo=NREDO, seed=1, max_points_per_centroid=10 ** 6)
    kb.train(xd, init_indices=init)
    assert (kb.status == 0).all(), kb.status
    assert kb.fallback == [False] * B           # (a test that passes because everything fell back shows nothing)
    dist2, labels = kb.assign(xd)
    for b, (km, splits) in enumerate(fits):
        assert splits == [], (b, splits)        # the loop itself met no empty cluster on these inputs
        print(b, "objectives", kb.obj[b], km.obj)
        assert len(kb.obj[b]) == NREDO
        for got, want in zip(kb.obj[b], km.obj):
            assert abs(got - want) <= 1e-12 * abs(want), (b, got, want)
        assert torch.equal(kb.centroids[b], km._centroids_dev), b
        ld2, ll = km.assign(xd[b])
        assert torch.equal(labels[b], ll) and torch.equal(dist2[b], ld2), b
    assert kb.centroids.shape == (B, k, d) and labels.dtype == torch.int64


# ---- 2. against fp64 --------------------------------------------------------------------------------------------------------------------

def test_fused_fit_against_the_fp64_oracle(ops):
    """The bounds of test_kmeans_driver_vs_oracle_lloyd (rtol 1e-4) on one shape of test 1."""
    from timetuning_amd.clustering import KmeansBatch

    n, d, k = 257, 50, 10
    x, init, xd, _ = loop_fit(n, d, k)
    kb = KmeansBatch(d, k, niter=NITER, nredo=NREDO, seed=1, max_points_per_centroid=10 ** 6)
    best = kb.train(xd, init_indices=init)
    for b in range(B):
        runs = [O.kmeans_lloyd(x[b], idx, NITER) for idx in init]
        objs = [obj for _, _, obj in runs]
        assert all(len(np.unique(lab)) == k for _, lab, _ in runs)
        assert np.allclose(kb.obj[b], objs, rtol=1e-4), (kb.obj[b], objs)
        assert abs(best[b] - min(objs)) < 1e-4 * min(objs)
        cent = runs[int(np.argmin(objs))][0]
        print(b, "centroids", rel_err(kb.centroids[b].cpu().numpy(), cent))
        assert rel_err(kb.centroids[b].cpu().numpy(), cent) < 1e-4


# ---- 3. empty clusters are flagged, isolated and repaired ------------------------------------------------------------------------------

def test_an_empty_cluster_is_flagged_and_that_problem_alone_falls_back(ops):
    """Problem 1 holds every point twice and redo 0 seeds clusters 0 and 1 on the two copies of one point: the strict < leaves cluster 1
    empty in the first assignment.  Problems 0 and 2 (the same seeds, distinct points) are clean."""
    from timetuning_amd.clustering import Kmeans, KmeansBatch

    n, d, k = 300, 17, 5
    x, init = blobs(n, d, k, tag=".e")
    x[1, n // 2:] = x[1, : n // 2]
    init = [np.array([0, n // 2, 60, 120, 180])] + init[1:]
    xd = dev(x)
    cent, obj, status = ops.kmeans_fit_batched(xd, torch.as_tensor(np.stack(init), dtype=torch.int32), NITER)
    status = status.cpu().numpy()
    assert status[1, 0] == 1 and (status[0] == 0).all() and (status[2] == 0).all(), status
    kb = KmeansBatch(d, k, niter=NITER, nredo=NREDO, seed=1, max_points_per_centroid=10 ** 6)
    kb.train(xd, init_indices=init)
    assert kb.fallback == [False, True, False]
    for b in range(B):
        km = Kmeans(d, k, niter=NITER, nredo=NREDO, seed=1, max_points_per_centroid=10 ** 6)
        splits = count_splits(km)
        km.train(xd[b], init_indices=init)
        assert (sum(splits) > 0) == (b == 1), (b, splits)
        assert torch.equal(kb.centroids[b], km._centroids_dev), b
        if b == 1:
            assert kb.obj[b] == km.obj           # the loop's own numbers
        else:
            assert all(abs(got - want) <= 1e-12 * abs(want) for got, want in zip(kb.obj[b], km.obj)), (b, kb.obj[b], km.obj)


# ---- 4. the batched assignment ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,k", [(16, 9), (50, 21), (128, 40)])   # the 16- and 64-register routes and rows read in place
def test_batched_assignment_equals_one_call_per_problem(ops, d, k):
    N = 700
    x = dev(synth.normal(f"kf.a.x.{d}", (B, N, d)))
    c = dev(synth.normal(f"kf.a.c.{d}.{k}", (B, k, d)) * 0.5)
    labels, dist2 = ops.kmeans_assign_batched(x, c, return_dist=True)
    assert labels.shape == (B, N) and labels.dtype == torch.int32
    for b in range(B):
        ll, ld2 = ops.kmeans_assign(x[b], c[b], return_dist=True)
        assert torch.equal(labels[b], ll) and torch.equal(dist2[b], ld2), b
    assert torch.equal(ops.kmeans_assign_batched(x, c), labels)


@pytest.mark.parametrize("dup", [False, True])
@pytest.mark.parametrize("d,k", [(16, 1024), (64, 252), (128, 128)])   # the largest k the resident rule takes on each of the three routes
def test_batched_assignment_equals_the_tiled_kernel(ops, d, k, dup):
    """``tt_kmeans_assign`` is the batched kernel at one problem, so the test above holds the offsets only; the arithmetic is held here
    against another kernel body, the tiled assignment with a tile of 7 centroids.  ``dup``: centroid 3 is point 0 itself and is
    repeated as centroid k - 1, in another tile - both kernels must keep the first of the two equal (zero) distances."""
    N = 700
    x = synth.normal(f"kf.t.x.{d}", (B, N, d))
    c = synth.normal(f"kf.t.c.{d}.{k}", (B, k, d)) * 0.5
    if dup:
        c[:, 3] = x[:, 0]
        c[:, k - 1] = c[:, 3]
    x, c = dev(x), dev(c)
    assert ops.kmeans_shape_ok(d, k) and not ops.kmeans_shape_ok(d, k + 1)
    labels, dist2 = ops.kmeans_assign_batched(x, c, return_dist=True)
    for b in range(B):
        tl, td2 = ops.kmeans_assign_tiled(x[b], c[b], return_dist=True, tile_k=7)
        assert torch.equal(labels[b], tl) and torch.equal(dist2[b], td2), b
        if dup:
            assert int(labels[b, 0]) == 3 and float(dist2[b, 0]) == 0.0, b


# ---- 5. cluster_features ------------------------------------------------------------------------------------------------------------------

def _planted():
    """The planted-quadrant features of test_cluster_features_over_clustering_many_to_one."""
    bs, fs, g_, dim, K, R = 2, 2, 14, 64, 4, 28
    protos = synth.normal("ev.cf.p", (K, dim)) * 3
    yy, xx = np.mgrid[0:g_, 0:g_]
    seg = ((yy >= 7).astype(int) * 2 + (xx >= 7).astype(int)).reshape(-1)              # 4 quadrants
    feats = np.stack([[protos[seg] + 0.3 * synth.normal(f"ev.cf.n{b}{f}", (g_ * g_, dim)) for f in range(fs)] for b in range(bs)])
    gt = torch.from_numpy(np.kron(seg.reshape(g_, g_), np.ones((R // g_, R // g_), int))).cuda()
    gts = gt[None, None].expand(bs, fs, R, R).contiguous() + 1                           # labels 1..4 (0 = background, unused)
    return dev(feats.astype(np.float32)), gts, (bs, fs, g_, K, R)


@pytest.mark.parametrize("protocol", ["frame-wise", "sample-wise"])
def test_cluster_features_takes_the_batched_route_and_returns_the_loops_maps(ops, monkeypatch, protocol):
    from timetuning_amd import clustering
    from timetuning_amd.evaluation import evaluate_localizations
    from timetuning_amd.metrics import PredsmIoU

    feats, gts, (bs, fs, g_, K, R) = _planted()
    k = 4
    calls = []
    iterate = clustering.Kmeans._iterate
    monkeypatch.setattr(clustering.Kmeans, "_iterate", lambda self, *a: (calls.append(1), iterate(self, *a))[1])
    maps = clustering.cluster_features(feats, k, g_, R, protocol)
    assert calls == []                       # every problem ran on the fused fit, none on the loop
    assert maps.shape == (bs, fs, R, R) and maps.dtype == torch.int16
    score = evaluate_localizations(PredsmIoU(k, K), gts, maps.long(), protocol)
    print(protocol, score)
    assert score > 0.9, (protocol, score)
    monkeypatch.setattr(ops, "kmeans_fit_shape_ok", lambda *a: False)   # the route off: the parent's code path
    want = clustering.cluster_features(feats, k, g_, R, protocol)
    assert len(calls) == (bs * fs if protocol == "frame-wise" else bs)
    assert torch.equal(maps, want)


@pytest.mark.parametrize("protocol", ["frame-wise", "sample-wise"])
def test_cluster_features_groups_the_problems_by_their_annotated_cluster_count(ops, monkeypatch, protocol):
    from timetuning_amd import clustering

    feats, _, (bs, fs, g_, K, R) = _planted()
    ann = torch.zeros((bs, fs, R, R), dtype=torch.int64, device="cuda")
    cols = torch.arange(R, device="cuda")
    ann[0] = (cols % 3)[None, None, :]       # clip 0: 3 distinct labels in every frame
    ann[1] = (cols % 5)[None, None, :]       # clip 1: 5
    fitted = []
    fit = ops.kmeans_fit_batched
    monkeypatch.setattr(ops, "kmeans_fit_batched", lambda x, init, niter: (fitted.append((x.shape[0], init.shape[1])), fit(x, init, niter))[1])
    maps = clustering.cluster_features(feats, 10, g_, R, protocol, annotations=ann)
    per = fs if protocol == "frame-wise" else 1
    assert fitted == [(per, 3), (per, 5)]    # two groups, one launch each
    assert 0 <= int(maps.min()) and int(maps[0].max()) < 3 and int(maps[1].max()) < 5
    monkeypatch.setattr(ops, "kmeans_fit_shape_ok", lambda *a: False)
    assert torch.equal(maps, clustering.cluster_features(feats, 10, g_, R, protocol, annotations=ann))


# ---- 6. the command line ------------------------------------------------------------------------------------------------------------------

def test_evaluation_cli_frame_wise_scores_what_the_loop_scores(ops, monkeypatch):
    from timetuning_amd.evaluation import main

    argv = ["--dataset", "synthetic", "--model_path", "", "--evaluation_protocol", "frame-wise", "--input_resolution", "64", "--batch_size", "2",
            "--num_frames", "2", "--eval_clips", "2"]
    fitted = []
    fit = ops.kmeans_fit_batched
    monkeypatch.setattr(ops, "kmeans_fit_batched", lambda *a: (fitted.append(1), fit(*a))[1])
    score = main(argv, vit_cfg=synth.ARCHS["tiny-s16"])
    assert fitted and 0.0 <= score <= 1.0
    monkeypatch.setattr(ops, "kmeans_fit_shape_ok", lambda *a: False)
    assert main(argv, vit_cfg=synth.ARCHS["tiny-s16"]) == score
