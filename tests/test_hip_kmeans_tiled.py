"""GPU checks of N12, k-means beyond the LDS limit (kmeans.hip): the tiled assignment and accumulation are held BIT FOR BIT to the
LDS-resident pair of the same file wherever both run, and - beyond what the resident pair takes - to combinations of resident calls on
centroid chunks that fit (no tolerance either) and to fp64 NumPy at the bounds of tests/test_hip_evaluator.py::test_kmeans_kernels.
Then the router in ``clustering.Kmeans``, ``cluster_features`` / ``proto_clustering`` at cluster counts the resident kernels refuse, and
the evaluation command line."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import timet_oracle as O
from timetuning_amd import synth

pytestmark = pytest.mark.gpu

BOTH = [(7001, 50, 21), (3000, 16, 1024), (3000, 64, 252), (3000, 128, 128), (1, 50, 300), (257, 17, 9), (1_200_000, 8, 64)]   # (P, d, k)
BEYOND = [(7001, 50, 500), (3000, 64, 253), (3000, 16, 1025), (3000, 128, 129), (20000, 1, 16385)]


@pytest.fixture(scope="module")
def ops():
    from timetuning_amd import hip_ops

    return hip_ops


def dev(a):
    return torch.as_tensor(a).cuda().contiguous()


_DATA = {}


def data(P, d, k):
    """Points and centroids of one shape (host arrays and device tensors), made once per module and never written to."""
    if (P, d, k) not in _DATA:
        x = synth.normal(f"kt.x.{P}.{d}", (P, d))
        c = x[:k] * 0.5 if P >= k else synth.normal(f"kt.c.{k}.{d}", (k, d)) * 0.5
        _DATA[(P, d, k)] = (x, c, dev(x), dev(c))
    return _DATA[(P, d, k)]


def largest_resident_k(ops, d):
    m = 16384 // d
    while not ops.kmeans_shape_ok(d, m):
        m -= 1
    return m


def fp64_d2(x, c):
    """Squared distances [points, centroids] in fp64, a column at a time (no [P, k, d] temporary)."""
    x, c = x.astype(np.float64), c.astype(np.float64)
    d2 = np.zeros((len(x), len(c)))
    for t in range(x.shape[1]):
        d2 += (x[:, t, None] - c[None, :, t]) ** 2
    return d2


_FP64 = {}


def fp64_nearest(P, d, k):
    """(arg-min, smallest, second smallest) squared distance per point in fp64, 1000 points at a time."""
    if (P, d, k) not in _FP64:
        x, c = data(P, d, k)[:2]
        arg, lo, lo2 = np.empty(P, np.int64), np.empty(P), np.empty(P)
        for p0 in range(0, P, 1000):
            d2 = fp64_d2(x[p0:p0 + 1000], c)
            rows = np.arange(len(d2))
            a = d2.argmin(1)
            arg[p0:p0 + 1000], lo[p0:p0 + 1000] = a, d2[rows, a]
            d2[rows, a] = np.inf
            lo2[p0:p0 + 1000] = d2.min(1)
        _FP64[(P, d, k)] = (arg, lo, lo2)
    return _FP64[(P, d, k)]


# ---- 1. bit equality where both pairs run ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,d,k", BOTH)
def test_tiled_pair_equals_the_resident_pair_bit_for_bit(ops, P, d, k):
    _, _, x, c = data(P, d, k)
    assert ops.kmeans_shape_ok(d, k) and ops.kmeans_tiled_shape_ok(d, k)
    labels, dist2 = ops.kmeans_assign(x, c, return_dist=True)
    sums, counts = ops.kmeans_accumulate(x, labels, k)
    tiles = sorted({t for t in (0, 1, 7, k - 1, k) if t <= ops.kmeans_tile_centroids(d)})   # (0 = the default tile)
    for tile_k in tiles:
        l2, d2 = ops.kmeans_assign_tiled(x, c, return_dist=True, tile_k=tile_k)
        assert torch.equal(l2, labels) and torch.equal(d2, dist2), (tile_k, int((l2 != labels).sum()), int((d2 != dist2).sum()))
        assert torch.equal(ops.kmeans_assign_tiled(x, c, tile_k=tile_k), labels)          # without distances: the same labels
        s2, c2 = ops.kmeans_accumulate_tiled(x, labels, k, tile_k=tile_k)
        assert torch.equal(s2, sums) and torch.equal(c2, counts), (tile_k, int((s2 != sums).sum()), int((c2 != counts).sum()))


def test_a_tile_beyond_the_default_is_refused(ops):
    from timetuning_amd._lib import HipLibraryError

    _, _, x, c = data(257, 17, 9)
    most = ops.kmeans_tile_centroids(17)
    with pytest.raises(HipLibraryError, match=f"tile_k = {most + 1} .* {most}"):
        ops.kmeans_assign_tiled(x, c, tile_k=most + 1)
    with pytest.raises(HipLibraryError, match=f"tile_k = {most + 1} .* {most}"):
        ops.kmeans_accumulate_tiled(x, torch.zeros(257, dtype=torch.int32, device="cuda"), 9, tile_k=most + 1)


# ---- 2. the first minimum across a tile boundary, degenerate label sets ------------------------------------------------------------------

@pytest.mark.parametrize("P,d,k,tile_k", [(600, 6, 40, 7), (1500, 50, 400, 0)])
def test_first_minimum_survives_a_tile_boundary(ops, P, d, k, tile_k):
    tile = tile_k or ops.kmeans_tile_centroids(d)
    assert tile < k
    c = synth.normal(f"kt.fm.c.{k}", (k, d)).copy()
    j = 2
    c[j + tile] = c[j]                     # a duplicate one tile later, at the same place in its tile
    c[tile] = c[tile - 1]                  # a duplicate on the two sides of the first tile boundary
    x = (c[np.arange(P) % k] + 0.05 * synth.normal(f"kt.fm.x.{k}", (P, d))).astype(np.float32)   # every centroid has points at it
    labels, dist2 = ops.kmeans_assign_tiled(dev(x), dev(c), return_dist=True, tile_k=tile_k)
    lab = labels.cpu().numpy()
    assert (lab == j).any() and (lab == tile - 1).any()
    assert not (lab == j + tile).any() and not (lab == tile).any()          # no point takes the higher index of a duplicate
    d2 = fp64_d2(x, c)
    assert (lab == d2.argmin(1)).all() and rel_err(dist2.cpu(), d2.min(1)) < 1e-5   # (planted points: no near-ties; np.argmin is the first minimum too)
    for other in (1, tile - 1 if tile > 1 else 1):
        l2, e2 = ops.kmeans_assign_tiled(dev(x), dev(c), return_dist=True, tile_k=other)
        assert torch.equal(l2, labels) and torch.equal(e2, dist2), other


@pytest.mark.parametrize("d,k,tile_k", [(6, 40, 7), (50, 400, 0)])
def test_all_points_in_one_cluster_and_an_unused_label(ops, d, k, tile_k):
    P, only = 1000, k - 3
    c = synth.normal(f"kt.one.c.{k}", (k, d)) * 4
    x = (c[only] + 0.01 * synth.normal(f"kt.one.x.{k}", (P, d))).astype(np.float32)
    labels = ops.kmeans_assign_tiled(dev(x), dev(c), tile_k=tile_k)
    assert (labels == only).all()
    sums, counts = ops.kmeans_accumulate_tiled(dev(x), labels, k, tile_k=tile_k)
    want = torch.zeros(k, dtype=torch.int64)
    want[only] = P
    assert torch.equal(counts.cpu(), want)
    rest = torch.arange(k) != only
    assert (sums.cpu()[rest] == 0).all()                                     # labels no point carries: zero counts, zero sums
    assert rel_err(sums.cpu()[only], x.astype(np.float64).sum(0)) < 1e-5


@pytest.mark.parametrize("P,d", [(700, 50), (300, 128), (513, 3)])
def test_a_single_centroid(ops, P, d):
    x = synth.normal(f"kt.k1.x.{d}", (P, d))
    c = x[:1] * 0.5
    labels, dist2 = ops.kmeans_assign_tiled(dev(x), dev(c), return_dist=True)
    l1, d1 = ops.kmeans_assign(dev(x), dev(c), return_dist=True)
    assert (labels == 0).all() and torch.equal(labels, l1) and torch.equal(dist2, d1)
    assert rel_err(dist2.cpu(), ((x.astype(np.float64) - c.astype(np.float64)) ** 2).sum(1)) < 1e-5
    sums, counts = ops.kmeans_accumulate_tiled(dev(x), labels, 1)
    s1, c1 = ops.kmeans_accumulate(dev(x), labels, 1)
    assert torch.equal(sums, s1) and torch.equal(counts, c1) and int(counts[0]) == P


# ---- 3. beyond the resident limit, no tolerance: against resident calls on centroid chunks that fit -------------------------------------

@pytest.mark.parametrize("P,d,k", BEYOND)
def test_beyond_the_limit_assignment_equals_chunked_resident_calls(ops, P, d, k):
    _, _, x, c = data(P, d, k)
    assert not ops.kmeans_shape_ok(d, k) and ops.kmeans_tiled_shape_ok(d, k)
    m = largest_resident_k(ops, d)
    best = torch.full((P,), float("inf"), device="cuda")
    besti = torch.zeros(P, dtype=torch.int32, device="cuda")
    for a in range(0, k, m):                                                  # chunks in index order, strict <: the first minimum
        lab, dist = ops.kmeans_assign(x, c[a:a + m].contiguous(), return_dist=True)
        upd = dist < best
        best = torch.where(upd, dist, best)
        besti = torch.where(upd, lab + a, besti)
    for tile_k in (0, 1, 13):
        labels, dist2 = ops.kmeans_assign_tiled(x, c, return_dist=True, tile_k=tile_k)
        assert torch.equal(labels, besti) and torch.equal(dist2, best), (tile_k, int((labels != besti).sum()), int((dist2 != best).sum()))


@pytest.mark.parametrize("P,d,k", BEYOND)
def test_beyond_the_limit_accumulation_equals_chunked_resident_calls(ops, P, d, k):
    _, _, x, c = data(P, d, k)
    labels = ops.kmeans_assign_tiled(x, c)
    m = largest_resident_k(ops, d) - 1                                         # one more bin holds the points of every other chunk
    assert (m + 1) * d <= 16384 and ops.kmeans_shape_ok(d, m + 1)
    results = {tile_k: ops.kmeans_accumulate_tiled(x, labels, k, tile_k=tile_k) for tile_k in (0, 1, 13)}
    for a in range(0, k, m):
        b = min(a + m, k)
        inside = (labels >= a) & (labels < b)
        local = torch.where(inside, labels - a, torch.full_like(labels, b - a)).contiguous()
        s, n = ops.kmeans_accumulate(x, local, b - a + 1)
        for tile_k, (sums, counts) in results.items():
            assert torch.equal(sums[a:b], s[:b - a]) and torch.equal(counts[a:b], n[:b - a]), (tile_k, a, b)


# ---- 4. beyond the limit, against fp64 (bounds: tests/test_hip_evaluator.py:56-57) ---------------------------------------------------------

@pytest.mark.parametrize("P,d,k", BEYOND)
def test_beyond_the_limit_against_fp64(ops, P, d, k):
    x, c, xd, cd = data(P, d, k)
    want, lo, lo2 = fp64_nearest(P, d, k)
    labels, dist2 = ops.kmeans_assign_tiled(xd, cd, return_dist=True)
    lab = labels.cpu().numpy()
    near_tie = lo2 - lo < 1e-4 * lo
    mism = lab != want
    print(f"(P, d, k) = {(P, d, k)}: {int(near_tie.sum())} points within the 1e-4 margin, {int(mism.sum())} labels differ, "
          f"dist2 error {rel_err(dist2.cpu(), lo):.3g}")
    assert near_tie.sum() <= 0.005 * P                                         # the condition the check rests on
    assert near_tie[mism].all()                                                # only near-ties may differ
    assert rel_err(dist2.cpu(), lo) < 1e-5
    sums, counts = ops.kmeans_accumulate_tiled(xd, labels, k)
    assert (counts.cpu().numpy() == np.bincount(lab, minlength=k)).all()
    want_sums = np.zeros((k, d))
    np.add.at(want_sums, lab, x.astype(np.float64))
    print(f"   sums error {rel_err(sums.cpu(), want_sums):.3g}")
    assert rel_err(sums.cpu(), want_sums) < 1e-5


# ---- 5. the driver ----------------------------------------------------------------------------------------------------------------------

def _blobs():
    d, nb = 50, 8
    centres = synth.normal("kt.drv.c", (nb, d)) * 6
    return np.concatenate([centres[j] + synth.normal(f"kt.drv.{j}", (500, d)) for j in range(nb)]).astype(np.float32)


def test_kmeans_driver_beyond_the_limit_vs_oracle_lloyd():
    """k = 400 at d = 50 (k * d = 20000): ``train`` runs the tiled pair - on the parent commit it raises HipLibraryError.
    The initial rows are every tenth point from offsets 6 and 9: each seed owns itself, so no cluster is ever empty (the oracle's "empty
    keeps its centroid" rule never applies), and over the five fp64 iterations from them the two nearest centroids of a point are never
    closer than 8e-6 relative - well above the fp32 distances' error (1e-6), so fp32 and fp64 Lloyd make the same assignments."""
    from timetuning_amd.clustering import Kmeans

    k, d = 400, 50
    x = _blobs()
    assert len(np.unique(x, axis=0)) == 4000
    init = [np.arange(6, 4000, 10), np.arange(9, 4000, 10)]
    km = Kmeans(d, k, niter=5, nredo=2, seed=1, max_points_per_centroid=10 ** 6)   # no subsampling: the init rows index x itself
    best = km.train(dev(x), init_indices=init)
    runs = [O.kmeans_lloyd(x, idx, 5) for idx in init]
    objs = [obj for _, _, obj in runs]
    print("objectives", km.obj, objs)
    assert all(len(np.unique(lab)) == k for _, lab, _ in runs)
    assert np.allclose(km.obj, objs, rtol=1e-4)
    assert abs(best - min(objs)) < 1e-4 * min(objs)
    cent = runs[int(np.argmin(objs))][0]
    print("centroids", rel_err(km.centroids, cent))
    assert rel_err(km.centroids, cent) < 1e-4
    _, labels = km.assign(dev(x))
    assert (labels.cpu().numpy() == fp64_d2(x, km.centroids).argmin(1)).mean() > 0.999


def test_kmeans_driver_beyond_the_limit_default_seeding_splits_empty_clusters():
    from timetuning_amd.clustering import Kmeans

    x = _blobs()
    x[2000:] = x[:2000]                     # every point twice: two seeds on one point leave the second cluster empty
    km = Kmeans(50, 400)
    splits = []
    split = km._split_empty
    km._split_empty = lambda cent, counts, n: splits.append(split(cent, counts, n))
    km.train(dev(x))
    assert sum(splits) > 0 and km.centroids.shape == (400, 50) and np.isfinite(km.centroids).all()
    assert int(km.assign(dev(x))[1].max()) < 400


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------------

def test_cluster_features_over_clustering_many_to_one():
    """test_hip_evaluator.py::test_cluster_features_recovers_planted_segments with 400 clusters and many-to-one matching, its own bar."""
    from timetuning_amd.clustering import cluster_features
    from timetuning_amd.evaluation import evaluate_localizations
    from timetuning_amd.metrics import PredsmIoU

    bs, fs, g_, dim, K, R, k = 2, 2, 14, 64, 4, 28, 400
    protos = synth.normal("ev.cf.p", (K, dim)) * 3
    yy, xx = np.mgrid[0:g_, 0:g_]
    seg = ((yy >= 7).astype(int) * 2 + (xx >= 7).astype(int)).reshape(-1)              # 4 quadrants
    feats = np.stack([[protos[seg] + 0.3 * synth.normal(f"ev.cf.n{b}{f}", (g_ * g_, dim)) for f in range(fs)] for b in range(bs)])
    gt = torch.from_numpy(np.kron(seg.reshape(g_, g_), np.ones((R // g_, R // g_), int))).cuda()
    gts = gt[None, None].expand(bs, fs, R, R).contiguous() + 1                           # labels 1..4 (0 = background, unused)
    for protocol in ("frame-wise", "sample-wise", "dataset-wise"):
        maps = cluster_features(dev(feats.astype(np.float32)), k, g_, R, protocol)
        assert maps.shape == (bs, fs, R, R) and maps.dtype == torch.int16
        assert 0 <= int(maps.min()) and int(maps.max()) < k
        score = evaluate_localizations(PredsmIoU(k, K), gts, maps.long(), protocol, many_to_one=True)
        print(protocol, score, int(torch.unique(maps).numel()))
        assert score > 0.9, (protocol, score)
        if protocol == "dataset-wise":
            assert torch.unique(maps).numel() > 327


def test_proto_clustering_merges_wide_prototypes():
    from timetuning_amd.clustering import proto_clustering

    x = dev(synth.normal("kt.pc.x", (3, 196, 256)))
    protos = dev(synth.normal("kt.pc.p", (200, 256)))
    merged = proto_clustering(x, protos, input_size=14, output_size=56, num_classes=80)   # Kmeans(256, 80): k * d = 20480
    assert merged.shape == (3, 56, 56) and 0 <= int(merged.min()) and int(merged.max()) < 80


# ---- 7. the command line ------------------------------------------------------------------------------------------------------------------

def test_evaluation_cli_over_clustering(capsys):
    from timetuning_amd.evaluation import main

    argv = ["--dataset", "synthetic", "--model_path", "", "--architecture", "dino-s16", "--evaluation_protocol", "dataset-wise",
            "--num_clusters", "400", "--many_to_one", "1", "--batch_size", "2", "--num_frames", "2", "--eval_clips", "2",
            "--input_resolution", "64"]
    score = main(argv, vit_cfg=synth.ARCHS["tiny-s16"])
    assert 0.0 < score <= 1.0
    assert f"Dataset score is {score}" in capsys.readouterr().out
    argv[argv.index("--num_clusters") + 1] = "21"
    del argv[argv.index("--many_to_one"):argv.index("--many_to_one") + 2]
    assert 0.0 <= main(argv, vit_cfg=synth.ARCHS["tiny-s16"]) <= 1.0
