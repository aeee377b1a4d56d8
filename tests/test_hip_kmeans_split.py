"""N18 on the GPU: the batched k-means fit that splits empty clusters in the kernel (``tt_kmeans_fit_batched_split``),
``clustering.KmeansBatch(split="device")`` and the frame-wise / sample-wise routes of ``cluster_features`` on masked features - held bit
for bit to the loop of ``clustering.Kmeans`` with its host-side ``_split_empty``, which stays in the tree unchanged."""
import numpy as np
import pytest
import torch

from timetuning_amd import synth

pytestmark = pytest.mark.gpu

B, NITER, NREDO = 3, 6, 3
SPREAD = 2.0
# (n, d, k): both register routes (d <= 16, d <= 64), all three load widths (d % 4 == 0, d % 2 == 0, odd), one, two and three
# accumulation blocks of 128 points with a ragged last one
SHAPES = [(40, 3, 5), (130, 50, 10), (257, 64, 7), (300, 17, 5)]


@pytest.fixture(scope="module")
def ops():
    from timetuning_amd import hip_ops

    return hip_ops


def dev(a):
    return torch.as_tensor(a).cuda().contiguous()


def masked_blobs(n, d, k):
    """B problems of n points in k Gaussian blobs (point p in blob p % k, as tests/test_hip_kmeans_fit.py).  In problem 1 the last 60 %
    of the rows are ONE vector - what ``use_mask`` makes of the background tokens.  The seeds, shared by the problems: redo 0 holds
    three rows of that set (the strict < leaves two of the three clusters empty in the first assignment: two splits in one call), redo
    1 two of them, redo 2 none; all other seeds are rows 0 ... of the distinct points, one per blob."""
    x = np.stack([np.stack([synth.normal(f"ks.c.{n}.{d}.{k}.{b}", (k, d))[p % k] * SPREAD for p in range(n)])
                  + synth.normal(f"ks.x.{n}.{d}.{k}.{b}", (n, d)) for b in range(B)]).astype(np.float32)
    first = n - (6 * n) // 10
    assert first >= k
    x[1, first:] = x[1, first]
    init = [np.concatenate([np.arange(k - 3), [first, first + 1, n - 1]]), np.concatenate([np.arange(k - 2), [first + 2, n - 2]]), np.arange(k)]
    return x, init


def count_splits(km):
    splits = []
    split = km._split_empty
    km._split_empty = lambda cent, counts, n: splits.append(split(cent, counts, n))
    return splits


_LOOP = {}


def loop_fit(n, d, k):
    """The loop on every problem of a shape, run once per module: the inputs and [(Kmeans, the returns of its _split_empty calls)]."""
    from timetuning_amd.clustering import Kmeans

    if (n, d, k) not in _LOOP:
        x, init = masked_blobs(n, d, k)
        xd = dev(x)
        fits = []
        for b in range(B):
            km = Kmeans(d, k, niter=NITER, nredo=NREDO, seed=1, max_points_per_centroid=10 ** 6)   # no subsampling: init indexes x itself
            splits = count_splits(km)
            km.train(xd[b], init_indices=init)
            fits.append((km, splits))
        _LOOP[(n, d, k)] = (x, init, xd, fits)
    return _LOOP[(n, d, k)]


def assert_equals_the_loop(kb, xd, fits, problems=range(B)):
    dist2, labels = kb.assign(xd)
    for b in problems:
        km = fits[b][0]
        print(b, "objectives", kb.obj[b], km.obj)
        assert len(kb.obj[b]) == NREDO
        for got, want in zip(kb.obj[b], km.obj):
            assert abs(got - want) <= 1e-12 * abs(want), (b, got, want)
        assert torch.equal(kb.centroids[b], km._centroids_dev), b
        ld2, ll = km.assign(xd[b])
        assert torch.equal(labels[b], ll) and torch.equal(dist2[b], ld2), b


# ---- 1. bit equality with the loop, splits included -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,d,k", SHAPES)
def test_device_split_equals_the_loop_bit_for_bit(ops, n, d, k):
    from timetuning_amd.clustering import KmeansBatch

    x, init, xd, fits = loop_fit(n, d, k)
    print("splits of the loop", [s for _, s in fits])
    assert sum(fits[1][1]) > 0 and fits[1][1][0] == 2          # the loop did split on problem 1: two clusters in the first call of redo 0
    assert fits[0][1] == [] and fits[2][1] == []               # and never on the clean problems
    kb = KmeansBatch(d, k, niter=NITER, nredo=NREDO, seed=1, max_points_per_centroid=10 ** 6, split="device")
    kb.train(xd, init_indices=init)
    assert (kb.status == 0).all(), kb.status
    assert kb.fallback == [False] * B                           # (a test that passes because everything fell back shows nothing)
    assert_equals_the_loop(kb, xd, fits)
    assert kb.centroids.shape == (B, k, d)


# ---- 2. n == k: an empty cluster that nothing can fill ----------------------------------------------------------------------------------

def test_as_many_points_as_clusters_is_not_split_and_not_flagged(ops):
    """Six points of which two coincide, k = 6: the later of the two seeds on them stays empty in every iteration, ``_split_empty``
    stops at ``n <= k`` without a draw, and so does the kernel - status 0, the loop's centroids."""
    from timetuning_amd.clustering import Kmeans, KmeansBatch

    n = k = 6
    d = 4
    x = synth.normal("ks.nk", (B, n, d)).astype(np.float32)
    x[:, 4] = x[:, 1]
    init = [np.arange(6), np.array([4, 0, 5, 1, 2, 3]), np.array([5, 3, 2, 0, 4, 1])]
    xd = dev(x)
    kb = KmeansBatch(d, k, niter=NITER, nredo=NREDO, seed=1, max_points_per_centroid=10 ** 6, split="device")
    kb.train(xd, init_indices=init)
    assert (kb.status == 0).all() and kb.fallback == [False] * B, kb.status
    _, _, old = ops.kmeans_fit_batched(xd, torch.as_tensor(np.stack(init), dtype=torch.int32), NITER)
    assert (old.cpu().numpy() == 1).all()                       # every redo meets the empty cluster at once: all of it ran on the new kernel
    for b in range(B):
        km = Kmeans(d, k, niter=NITER, nredo=NREDO, seed=1, max_points_per_centroid=10 ** 6)
        splits = count_splits(km)
        km.train(xd[b], init_indices=init)
        assert splits == [0] * (NITER * NREDO), splits          # called at every iteration, never split
        assert torch.equal(kb.centroids[b], km._centroids_dev), b
        assert all(abs(got - want) <= 1e-12 * abs(want) for got, want in zip(kb.obj[b], km.obj)), (kb.obj[b], km.obj)


# ---- 3. a table that runs out ------------------------------------------------------------------------------------------------------------

def test_a_table_that_runs_out_is_flagged_and_that_problem_alone_falls_back(ops):
    from timetuning_amd.clustering import KmeansBatch, split_draws

    n, d, k = SHAPES[1]
    x, init, xd, fits = loop_fit(n, d, k)
    init32 = torch.as_tensor(np.stack(init), dtype=torch.int32)
    table = split_draws(device=xd.device)
    assert table.is_cuda and table.dtype == torch.float64 and table.numel() == 4096 and split_draws(device=xd.device) is table
    one = split_draws(1, device=xd.device)
    _, _, status = ops.kmeans_fit_batched(xd, init32, NITER, split_draws=table)
    assert (status == 0).all(), status
    cent1, _, status1 = ops.kmeans_fit_batched(xd, init32, NITER, split_draws=one)
    status1 = status1.cpu().numpy()
    print("status with one draw", status1)
    assert status1[1, 0] == 1                                   # two empty clusters need two draws at least
    assert (status1[0] == 0).all() and (status1[2] == 0).all()
    kb = KmeansBatch(d, k, niter=NITER, nredo=NREDO, seed=1, max_points_per_centroid=10 ** 6, split="device")
    kb.train(xd, init_indices=init, _draws=one)
    assert kb.fallback == [False, True, False] and kb.status[1, 0] == 1
    assert kb.obj[1] == fits[1][0].obj                          # the loop's own numbers
    assert_equals_the_loop(kb, xd, fits)


# ---- 4. the old entry ---------------------------------------------------------------------------------------------------------------------

def test_the_entry_without_a_table_still_flags_the_empty_cluster(ops):
    from timetuning_amd.clustering import KmeansBatch

    n, d, k = SHAPES[3]
    x, init, xd, fits = loop_fit(n, d, k)
    cent, obj, status = ops.kmeans_fit_batched(xd, torch.as_tensor(np.stack(init), dtype=torch.int32), NITER)
    status = status.cpu().numpy()
    assert status[1, 0] == 1 and status[1, 1] == 1 and (status[0] == 0).all() and (status[2] == 0).all(), status
    kb = KmeansBatch(d, k, niter=NITER, nredo=NREDO, seed=1, max_points_per_centroid=10 ** 6)   # split="host", the default
    kb.train(xd, init_indices=init)
    assert kb.fallback == [False, True, False] and kb.status[1, 0] == 1
    assert_equals_the_loop(kb, xd, fits)


# ---- 5. cluster_features on masked features -----------------------------------------------------------------------------------------------

def _masked_features():
    """1 clip of 3 frames, 6 x 6 tokens of 64 columns; the left half of every frame's tokens is multiplied by 0 (``use_mask``)."""
    bs, fs, g, dim = 1, 3, 6, 64
    protos = synth.normal("ks.cf.p", (4, dim)) * 3
    feats = np.stack([[protos[np.arange(g * g) % 4] + 0.5 * synth.normal(f"ks.cf.n{f}", (g * g, dim)) for f in range(fs)] for _ in range(bs)])
    keep = (np.arange(g * g) % g >= g // 2).astype(np.float32)
    return dev((feats * keep[None, None, :, None]).astype(np.float32)), (bs, fs, g, 24, 5)


@pytest.mark.parametrize("protocol", ["frame-wise", "sample-wise"])
def test_cluster_features_splits_on_the_device_and_returns_the_loops_maps(ops, monkeypatch, protocol):
    from timetuning_amd import clustering

    feats, (bs, fs, g, R, k) = _masked_features()
    calls = []
    iterate = clustering.Kmeans._iterate
    monkeypatch.setattr(clustering.Kmeans, "_iterate", lambda self, *a: (calls.append(1), iterate(self, *a))[1])
    assert clustering.DEVICE_SPLIT is True
    maps = clustering.cluster_features(feats, k, g, R, protocol)
    assert calls == []                       # no problem went to the loop
    assert maps.shape == (bs, fs, R, R) and maps.dtype == torch.int16
    monkeypatch.setattr(clustering, "DEVICE_SPLIT", False)
    want = clustering.cluster_features(feats, k, g, R, protocol)
    print(protocol, "problems the old route reran on the loop:", len(calls))
    assert len(calls) >= 1                   # the input does meet empty clusters: the old route fell back
    assert torch.equal(maps, want)
