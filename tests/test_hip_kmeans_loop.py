"""N28 on the GPU: the device loop of the large k-means fits (``tt_kmeans_fit_loop``, ``clustering.Kmeans(loop="device")``) and its
callers, held bit for bit to the host loop ``clustering.Kmeans(loop="host")`` on the same points, seeds and ``init_indices`` - every
redo's centroids, the last iteration's labels and dist2 and the status words by ``torch.equal``, the per-redo objectives to 1e-12
relative (the two sum the same fp64 numbers in different orders: n * 2^-53).  Each comparison first asserts, on the host loop's
objectives alone, that the redos' objectives are more than 1e-9 apart, so that the choice of the redo cannot hide a difference."""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch

from timetuning_amd import synth

pytestmark = pytest.mark.gpu

OBJ_RTOL = 1e-12      # n * 2^-53 at the largest n here (530 000) is 6e-11 in the worst case and sqrt(n) * 2^-53 = 8e-14 typically
APART = 1e-9


@pytest.fixture(scope="module")
def ops():
    from timetuning_amd import hip_ops

    return hip_ops


def dev(a):
    return torch.as_tensor(a).cuda().contiguous()


def gaussian(n, d, k, nredo, tag=""):
    """n unstructured normal points (every redo ends in another local optimum: distinct objectives) and nredo seed sets of k distinct rows."""
    x = synth.normal(f"kl.x.{n}.{d}.{k}{tag}", (n, d))
    rng = np.random.RandomState(n + 7 * d + 13 * k)
    return x, [rng.permutation(n)[:k] for _ in range(nredo)]


def count_splits(km):
    splits = []
    split = km._split_empty
    km._split_empty = lambda cent, counts, n: splits.append(split(cent, counts, n))
    return splits


def host_redos(ops, xd, init, niter, k, tile_k=0):
    """``Kmeans(loop="host")`` redo by redo (its ``_iterate`` on one seed set at a time, on the kernel pair the device loop's rule names)
    -> per redo (centroids, last labels, last dist2, objective, the returns of its _split_empty calls)."""
    from timetuning_amd.clustering import Kmeans

    d = xd.shape[1]
    out = []
    for idx in init:
        km = Kmeans(d, k, niter=niter, nredo=1, seed=1, max_points_per_centroid=10 ** 6, loop="host")
        if tile_k:
            assign0, accumulate = partial(ops.kmeans_assign_tiled, tile_k=tile_k), partial(ops.kmeans_accumulate_tiled, tile_k=tile_k)
        else:
            assign0, accumulate = km._kernels(d)
        last = {}

        def assign(x_, cent, return_dist=True):
            last["labels"], last["dist2"] = assign0(x_, cent, return_dist=True)
            return last["labels"], last["dist2"]

        splits = count_splits(km)
        obj = km._iterate(xd, [idx], assign, accumulate)
        out.append((km._centroids_dev.clone(), last["labels"].clone(), last["dist2"].clone(), obj, splits))
    return out


def assert_apart(objs):
    for i in range(len(objs)):
        for j in range(i + 1, len(objs)):
            assert abs(objs[i] - objs[j]) > APART * max(abs(objs[i]), abs(objs[j])), ("the seeds give nearly equal objectives", objs)


def check_against_host(ops, x, init, niter, k, tile_k=0, draws="table", apart=True, **kw):
    """The op on every redo against the host loop; returns (host, (centroids, obj, status))."""
    from timetuning_amd.clustering import split_draws

    xd = dev(x)
    host = host_redos(ops, xd, init, niter, k, tile_k)
    objs = [h[3] for h in host]
    print("host objectives", objs, "splits per redo", [sum(1 for s in h[4] if s) for h in host])
    if apart:
        assert_apart(objs)
    table = split_draws(device=xd.device) if isinstance(draws, str) else draws
    cent, obj, status, labels, dist2 = ops.kmeans_fit_loop(xd, np.stack(init), niter, table, tile_k=tile_k, return_last=True, **kw)
    torch.cuda.synchronize()
    print("device objectives", obj.tolist(), "status", status.tolist())
    assert torch.equal(status, torch.zeros_like(status))                          # the host loop finishes every redo
    for r, (c, l, d2, o, _) in enumerate(host):
        assert torch.equal(cent[r], c), f"centroids of redo {r}"
        assert torch.equal(labels[r], l), f"labels of redo {r}"
        assert torch.equal(dist2[r], d2), f"dist2 of redo {r}"
        assert abs(float(obj[r]) - o) <= OBJ_RTOL * abs(o), (r, float(obj[r]), o)
    return host, (cent, obj, status)


# ---- 1. the shapes ------------------------------------------------------------------------------------------------------------------------

# (n, d, k, tile_k, nredo, niter)
SHAPES = [
    (300, 50, 7, 0, 3, 6),         # resident assignment, 3 accumulation blocks, ragged last block
    (1000, 50, 37, 8, 3, 6),       # 5 centroid tiles, ragged last tile
    (700, 1, 9, 0, 3, 6),          # d: the register routes 16 and 64 at and beside their edges, and rows read in place
    (700, 16, 9, 0, 3, 6),
    (700, 17, 9, 0, 3, 6),
    (700, 64, 9, 0, 3, 6),
    (700, 65, 9, 0, 3, 6),
    (700, 130, 9, 0, 3, 6),
    (2600, 50, 330, 0, 2, 4),      # just past the resident limit (k = 327): two default tiles
    (1024, 384, 50, 0, 3, 6),      # CBFE's column count: the default tile is 42 rows
    (530000, 2, 3, 0, 2, 2),       # past 524 288 points: a block takes ceil(P / 4096) = 130 points
    (12800, 50, 500, 0, 2, 3),     # the over-clustering's k
]


@pytest.mark.parametrize("n,d,k,tile_k,nredo,niter", SHAPES)
def test_device_loop_returns_the_host_loops_bits(ops, n, d, k, tile_k, nredo, niter):
    from timetuning_amd.clustering import Kmeans

    assert ops.kmeans_loop_shape_ok(n, d, k)
    x, init = gaussian(n, d, k, nredo)
    host, (cent, obj, status) = check_against_host(ops, x, init, niter, k, tile_k)
    # the class: the redo kept, its centroids and the objectives are the host loop's
    want = Kmeans(d, k, niter=niter, nredo=nredo, seed=1, max_points_per_centroid=10 ** 6, loop="host")
    got = Kmeans(d, k, niter=niter, nredo=nredo, seed=1, max_points_per_centroid=10 ** 6, loop="device")
    xd = dev(x)
    best_want, best_got = want.train(xd, init_indices=init), got.train(xd, init_indices=init)
    assert got.fallback is False and got.status.tolist() == [0] * nredo and want.status is None
    assert torch.equal(got._centroids_dev, want._centroids_dev) and np.array_equal(got.centroids, want.centroids)
    assert np.allclose(got.obj, want.obj, rtol=OBJ_RTOL, atol=0) and abs(best_got - best_want) <= OBJ_RTOL * best_want
    assert int(np.argmin(want.obj)) == int(np.argmin(got.obj))
    d2w, lw = want.assign(xd)
    d2g, lg = got.assign(xd)
    assert torch.equal(lw, lg) and torch.equal(d2w, d2g)


def test_k_equal_n_with_duplicate_points_takes_the_splits_stop_path(ops):
    """(33, 5, 33): every point seeds a cluster; of two equal points the first seed in cluster order takes both, the other cluster is
    empty, and the split stops at once (n <= k).  Every point then lies ON a centroid: the objective of every redo is exactly 0 on both loops, so this one case cannot
    assert objectives that are apart - it asserts the zeros, and compares every redo directly."""
    n = d_k = 33
    x = synth.normal("kl.dup", (n, 5))
    x[20:] = x[:13]                                                               # 13 rows twice
    rng = np.random.RandomState(33)
    init = [rng.permutation(n) for _ in range(3)]
    host, (_, obj, _) = check_against_host(ops, x, init, 6, d_k, apart=False)
    assert all(h[3] == 0.0 for h in host) and obj.tolist() == [0.0, 0.0, 0.0]
    assert all(len(h[4]) == 6 and not any(h[4]) for h in host)                    # _split_empty ran in every iteration and split nothing


# ---- 2. empty clusters ----------------------------------------------------------------------------------------------------------------------

def masked(n, d, k):
    """n points in k blobs; the last 60 % of the rows are ONE vector - what ``use_mask`` makes of the background tokens.  Redo 0 is seeded
    with three rows of that set (two of the three clusters are empty after the first assignment), redo 1 with two, redo 2 with none."""
    x = (np.stack([synth.normal(f"kl.m.c.{d}", (k, d))[p % k] * 2.0 for p in range(n)]) + synth.normal(f"kl.m.x.{d}", (n, d))).astype(np.float32)
    first = n - (6 * n) // 10
    x[first:] = x[first]
    init = [np.concatenate([np.arange(k - 3), [first, first + 1, n - 1]]), np.concatenate([np.arange(k - 2), [first + 2, n - 2]]), np.arange(k)]
    return x, init


@pytest.mark.parametrize("d", [50, 70])
def test_few_distinct_values_split_in_several_iterations(ops, d):
    x, init = masked(300, d, 6)
    host, _ = check_against_host(ops, x, init, 6, 6)
    iterations_that_split = [sum(1 for s in h[4] if s) for h in host]
    assert max(iterations_that_split) >= 2                                        # the split ran in several iterations of one redo
    assert host[0][4][0] >= 2 and iterations_that_split[1] >= 1 and iterations_that_split[2] == 0   # two empties at once in redo 0


def test_a_short_table_flags_the_redo_and_the_class_falls_back(ops):
    from timetuning_amd.clustering import Kmeans, split_draws

    d, k, niter = 50, 6, 6
    x, init = masked(300, d, k)
    xd = dev(x)
    host = host_redos(ops, xd, init, niter, k)
    assert_apart([h[3] for h in host])
    short = split_draws(device=xd.device)[:3].clone()
    cent, obj, status = ops.kmeans_fit_loop(xd, np.stack(init), niter, short)
    st = status.tolist()
    print("status with 3 draws", st)
    assert st[2] == 0 and 1 <= st[0] <= niter and any(st)                         # redo 0 needed more than three draws in one call
    for r in range(3):
        if st[r] == 0:
            assert torch.equal(cent[r], host[r][0]) and abs(float(obj[r]) - host[r][3]) <= OBJ_RTOL * host[r][3]
    want = Kmeans(d, k, niter=niter, nredo=3, seed=1, max_points_per_centroid=10 ** 6, loop="host")
    want._fit(xd, init)
    got = Kmeans(d, k, niter=niter, nredo=3, seed=1, max_points_per_centroid=10 ** 6, loop="device")
    best = got._fit(xd, init, _draws=short)
    assert got.fallback is True and got.status.tolist() == st
    assert torch.equal(got._centroids_dev, want._centroids_dev) and got.obj == want.obj and best == min(want.obj)
    # without a table the first empty cluster flags the redo: iteration 1 for the redos seeded inside the repeated row
    cent, obj, status = ops.kmeans_fit_loop(xd, np.stack(init), niter, None)
    assert status.tolist() == [1, 1, 0] and torch.equal(cent[2], host[2][0])


# ---- 3. redo_group, guards, capture -----------------------------------------------------------------------------------------------------------

def test_redo_group_does_not_show_in_the_result(ops):
    from timetuning_amd.clustering import split_draws

    n, d, k, nredo = 300, 50, 7, 5
    x, init = gaussian(n, d, k, nredo, ".g")
    xd, table = dev(x), split_draws(device="cuda")
    runs = [ops.kmeans_fit_loop(xd, np.stack(init), 6, table, redo_group=g) for g in (0, 1, 2)]
    assert_apart(runs[0][1].tolist())
    for cent, obj, status in runs[1:]:
        assert torch.equal(cent, runs[0][0]) and torch.equal(obj, runs[0][1]) and torch.equal(status, runs[0][2])
    assert ops.kmeans_loop_workspace_bytes(n, d, k, nredo, 1) < ops.kmeans_loop_workspace_bytes(n, d, k, nredo, 2) \
        < ops.kmeans_loop_workspace_bytes(n, d, k, nredo, 0)


def _entry_args(ops, n, d, k, nredo, niter, group, pad=64):
    """Buffers for a direct call of the entry, the outputs and the workspace of exactly the queried size between / before sentinel guards."""
    from timetuning_amd import _lib
    from timetuning_amd.clustering import split_draws

    lib = _lib.load()
    x, init = gaussian(n, d, k, nredo, ".e")
    xd = dev(x)
    init_h = torch.from_numpy(np.stack(init).astype(np.int32)).contiguous()
    init_d = init_h.cuda()
    table = split_draws(device="cuda")
    nb = lib.tt_kmeans_loop_workspace_bytes(n, d, k, nredo, group)
    bufs = {"cent": torch.full((pad + nredo * k * d + pad,), -7.0, device="cuda"),
            "obj": torch.full((pad + nredo + pad,), -7.0, dtype=torch.float64, device="cuda"),
            "status": torch.full((pad + nredo + pad,), -7, dtype=torch.int32, device="cuda"),
            "ws": torch.full((nb + pad,), 0xA5, dtype=torch.uint8, device="cuda")}

    def call(stream):
        return lib.tt_kmeans_fit_loop(xd.data_ptr(), init_d.data_ptr(), init_h.data_ptr(), bufs["cent"][pad:].data_ptr(), bufs["obj"][pad:].data_ptr(),
                                      bufs["status"][pad:].data_ptr(), n, d, k, nredo, niter, 0, group, table.data_ptr(), table.numel(),
                                      bufs["ws"].data_ptr(), nb, stream)

    return lib, call, bufs, nb, (xd, init, table)


@pytest.mark.parametrize("n,d,k,group", [(300, 50, 7, 0), (1000, 50, 330, 2)])
def test_outputs_and_workspace_stay_inside_their_guards(ops, n, d, k, group):
    nredo, niter, pad = 3, 3, 64
    lib, call, bufs, nb, (xd, init, table) = _entry_args(ops, n, d, k, nredo, niter, group, pad)
    assert call(torch.cuda.current_stream().cuda_stream) == 0, lib.tt_last_error()
    torch.cuda.synchronize()
    for name, size in (("cent", nredo * k * d), ("obj", nredo), ("status", nredo)):
        b = bufs[name]
        assert bool((b[:pad] == -7).all()) and bool((b[pad + size:] == -7).all()), name
        assert not bool((b[pad: pad + size] == -7).any()), name
    assert bool((bufs["ws"][nb:] == 0xA5).all())
    cent, obj, status = ops.kmeans_fit_loop(xd, np.stack(init), niter, table, redo_group=group)
    assert torch.equal(bufs["cent"][pad: pad + nredo * k * d].view(nredo, k, d), cent) and torch.equal(bufs["obj"][pad: pad + nredo], obj)
    assert bufs["status"][pad: pad + nredo].tolist() == [0] * nredo


def _loaded_hip_runtime():
    """The HIP runtime this process already runs on (the one the library and torch share), as a ctypes handle."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in path:
            return ctypes.CDLL(path)
    raise RuntimeError("no libamdhip64 in this process")


def test_entry_neither_allocates_nor_breaks_a_stream_capture(ops):
    """The whole fit is enqueued: under hipStreamBeginCapture the entry returns TT_OK, the capture ends with a graph of exactly the
    launches the loop needs, and the graph is destroyed without a replay.  A hidden synchronisation, read-back or allocation would
    invalidate the capture; the device's free memory is the same before and after."""
    n, d, k, nredo, niter, group = 1000, 50, 330, 3, 3, 2
    lib, call, bufs, nb, _ = _entry_args(ops, n, d, k, nredo, niter, group)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()                                                      # the buffers were filled on the current stream
    with torch.cuda.stream(side):
        assert call(side.cuda_stream) == 0, lib.tt_last_error()                   # the first call raises the kernels' LDS limits
        torch.cuda.synchronize()
        eager = {name: b.clone() for name, b in bufs.items() if name != "ws"}
        hip = _loaded_hip_runtime()
        hip.hipStreamBeginCapture.argtypes = [ctypes.c_void_p, ctypes.c_int]
        hip.hipStreamEndCapture.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
        hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
        hip.hipGraphDestroy.argtypes = [ctypes.c_void_p]
        free0 = torch.cuda.mem_get_info()[0]
        graph, nodes = ctypes.c_void_p(), ctypes.c_size_t()
        assert hip.hipStreamBeginCapture(side.cuda_stream, 1) == 0                # hipStreamCaptureModeThreadLocal: this thread's calls are policed
        rc = call(side.cuda_stream)
        end = hip.hipStreamEndCapture(side.cuda_stream, ctypes.byref(graph))
        assert rc == 0 and end == 0 and graph.value, (rc, end, lib.tt_last_error())
        assert hip.hipGraphGetNodes(graph, None, ctypes.byref(nodes)) == 0
        assert hip.hipGraphDestroy(graph) == 0
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0, "the entry changed the device's free memory"
        # seeds + 2 passes x (3 iterations x (assignment, one tile launch, fold, update, split) + objective)
        assert nodes.value == 1 + 2 * (niter * 5 + 1), nodes.value
        for name, b in eager.items():                                             # nothing ran: the eager call's outputs are untouched
            assert torch.equal(bufs[name], b), name


# ---- 4. the callers -----------------------------------------------------------------------------------------------------------------------------

def _count_entry(monkeypatch, ops):
    calls = []
    entry = ops.kmeans_fit_loop
    monkeypatch.setattr(ops, "kmeans_fit_loop", lambda *a, **kw: (calls.append(a[0].shape), entry(*a, **kw))[1])
    return calls


@pytest.mark.parametrize("annotated", [False, True])
def test_dataset_wise_cluster_features_takes_the_device_loop(ops, monkeypatch, annotated):
    from timetuning_amd import clustering

    bs, fs, g, dim, R, k = 2, 2, 4, 64, 16, 5
    protos = synth.normal("kl.cf.p", (4, dim)) * 3
    feats = dev(np.stack([[protos[np.arange(g * g) % 4] + 0.5 * synth.normal(f"kl.cf.{b}{f}", (g * g, dim)) for f in range(fs)]
                          for b in range(bs)]).astype(np.float32))
    ann = None
    if annotated:
        ann = (torch.arange(R, device="cuda") % 3)[None, None, None, :].expand(bs, fs, R, R).contiguous()   # 3 label values: k = 3
    calls = _count_entry(monkeypatch, ops)
    iterate_calls = []
    iterate = clustering.Kmeans._iterate
    monkeypatch.setattr(clustering.Kmeans, "_iterate", lambda self, *a: (iterate_calls.append(1), iterate(self, *a))[1])
    assert clustering.DEVICE_LOOP is True
    maps = clustering.cluster_features(feats, k, g, R, "dataset-wise", annotations=ann)
    k_fit = 3 if annotated else k
    assert calls == [(min(bs * fs * R * R, 256 * k_fit), 50)] and iterate_calls == []   # the subsample: 256 points per centroid
    assert maps.shape == (bs, fs, R, R) and maps.dtype == torch.int16 and int(maps.max()) < k_fit
    monkeypatch.setattr(clustering, "DEVICE_LOOP", False)
    want = clustering.cluster_features(feats, k, g, R, "dataset-wise", annotations=ann)
    assert len(calls) == 1 and iterate_calls == [1]
    assert torch.equal(maps, want)


def test_create_overclustering_maps_takes_the_device_loop(ops, monkeypatch):
    from timetuning_amd import cluster_based_foreground_extraction as CB
    from timetuning_amd import clustering

    bs, fs, g, dim, R, k = 2, 2, 4, 24, 16, 6
    tokens = dev(synth.normal("kl.cb.t", (bs, fs, g * g, dim)))
    iy, ix = clustering.nearest_index_table(g, R)
    idx = torch.from_numpy((iy.astype(np.int64)[:, None] * g + ix.astype(np.int64)[None, :]).reshape(-1)).cuda()
    materialised = tokens[:, :, idx, :].view(bs, fs, R, R, dim).permute(0, 1, 4, 2, 3).contiguous()          # [bs, fs, dim, R, R]
    obj = CB.ClusterBasedForegroundExtraction.__new__(CB.ClusterBasedForegroundExtraction)
    torch.nn.Module.__init__(obj)
    obj.k_fg_extraction = k
    calls = _count_entry(monkeypatch, ops)
    got = [obj.create_overclustering_maps(materialised), obj.create_overclustering_maps(CB.UpsampledFeatures(tokens, R))]
    assert calls == [(bs * fs * R * R, dim)] * 2
    assert torch.equal(got[0], got[1]) and got[0].shape == (bs, fs, R, R) and int(got[0].max()) < k
    monkeypatch.setattr(clustering, "DEVICE_LOOP", False)
    want = [obj.create_overclustering_maps(materialised), obj.create_overclustering_maps(CB.UpsampledFeatures(tokens, R))]
    assert len(calls) == 2
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
