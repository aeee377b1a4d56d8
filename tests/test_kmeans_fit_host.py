"""CPU-only checks of N13, the batched k-means fit: the new C entries and their host-side rules (shape rule, LDS budget, workspace size,
refusals), and ``clustering.KmeansBatch`` around a NumPy stand-in for the fused kernel (redo selection, the fallback to the loop)."""
import os
import re

import numpy as np
import pytest
import torch

from timetuning_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TT_EINVAL = -1   # include/timetuning_hip.h
NEW = ("tt_kmeans_fit_shape_ok", "tt_kmeans_fit_lds_bytes", "tt_kmeans_fit_workspace_bytes", "tt_kmeans_fit_batched", "tt_kmeans_assign_batched")


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_new_symbols_are_declared_bound_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "timetuning_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tt_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.tt_abi_version() == 8          # additive, as N12
    assert "kmeans_fit.hip" in open(os.path.join(REPO, "timetuning_amd", "csrc", "Makefile")).read()


def test_fit_shape_rule_covers_every_subsample_of_the_two_protocols(lib):
    """1 <= d, k <= 64 and k <= n <= 256 k: what a frame-wise or sample-wise fit can be handed at k <= 64 (the subsample is 256 k points)."""
    for d in (1, 2, 15, 16, 17, 49, 50, 63, 64):
        for k in (1, 2, 9, 10, 21, 63, 64):
            for n in (k, k + 1, 128 * k, 256 * k):
                assert lib.tt_kmeans_fit_shape_ok(n, d, k), (n, d, k)
                assert 0 < lib.tt_kmeans_fit_lds_bytes(n, d, k) <= 128 * 1024, (n, d, k)
    for n, d, k in ((1, 1, 1), (16384, 64, 64), (2560, 50, 10)):
        assert lib.tt_kmeans_fit_shape_ok(n, d, k), (n, d, k)
    for n, d, k in ((9, 50, 10), (0, 1, 1), (100, 0, 5), (100, 5, 0), (100, 65, 5), (2 ** 20 + 1, 5, 5)):
        assert not lib.tt_kmeans_fit_shape_ok(n, d, k), (n, d, k)
        assert lib.tt_kmeans_fit_lds_bytes(n, d, k) == 0 and lib.tt_kmeans_fit_workspace_bytes(1, 1, n, d, k) == 0
    # the LDS bound: fp64 sums, centroids, one block's fp32 sums (16 k d bytes) and the counts (4 k) within 128 KB
    assert lib.tt_kmeans_fit_shape_ok(40000, 64, 127) and not lib.tt_kmeans_fit_shape_ok(40000, 64, 128)
    assert lib.tt_kmeans_fit_shape_ok(50000, 50, 163) and not lib.tt_kmeans_fit_shape_ok(50000, 50, 164)


def test_fit_lds_holds_as_many_blocks_as_fit_the_preferred_budget(lib):
    per = lambda d, k, g: k * d * (8 + 4 * (1 + g)) + 4 * k   # noqa: E731
    assert lib.tt_kmeans_fit_lds_bytes(2560, 50, 10) == per(50, 10, 20)      # all 20 blocks of the default evaluator shape: 46 KB
    assert lib.tt_kmeans_fit_lds_bytes(100, 50, 10) == per(50, 10, 1)
    assert lib.tt_kmeans_fit_lds_bytes(16384, 64, 64) == per(64, 64, 1)      # 12 k d alone is 48 KB: one more block's 16 KB reaches 64 KB
    assert lib.tt_kmeans_fit_lds_bytes(40000, 64, 127) == per(64, 127, 1) <= 128 * 1024


def test_fit_workspace_is_monotone_in_the_batch_and_the_points(lib):
    for d, k in ((50, 10), (64, 64), (1, 1)):
        sizes = [lib.tt_kmeans_fit_workspace_bytes(B, 5, 2560, d, k) for B in (1, 2, 3, 64, 1000)]
        assert sizes == sorted(sizes) and sizes[0] >= 5 * 2560 * 4 and len(set(sizes)) == len(sizes), sizes
        sizes = [lib.tt_kmeans_fit_workspace_bytes(7, 5, n, d, k) for n in (64, 127, 128, 129, 2560, 16384)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), sizes


def _fit(lib, init_host, x=16, init=16, cent=16, obj=16, status=16, B=3, n=100, d=50, k=10, nredo=2, niter=5, ws=16, ws_bytes=1 << 40):
    # (every refusal comes before any pointer is read or any kernel launched: dummy non-null device pointers, no GPU)
    host = None if init_host is None else init_host.ctypes.data
    rc = lib.tt_kmeans_fit_batched(x, init, host, cent, obj, status, B, n, d, k, nredo, niter, ws, ws_bytes, None)
    return rc, lib.tt_last_error().decode()


def test_fit_refusals_name_their_numbers(lib):
    good = np.tile(np.arange(10, dtype=np.int32), (2, 1))
    for null in ("x", "init", "cent", "obj", "status", "ws"):
        rc, msg = _fit(lib, good, **{null: None})
        assert rc == TT_EINVAL and "null pointer" in msg, (null, msg)
    rc, msg = _fit(lib, None)
    assert rc == TT_EINVAL and "null pointer" in msg
    rc, msg = _fit(lib, good, n=9)
    assert rc == TT_EINVAL and "n = 9" in msg and "k = 10" in msg, msg
    rc, msg = _fit(lib, good, niter=0)
    assert rc == TT_EINVAL and "niter = 0" in msg, msg
    rc, msg = _fit(lib, good, nredo=0)
    assert rc == TT_EINVAL and "nredo = 0" in msg, msg
    rc, msg = _fit(lib, good, B=0)
    assert rc == TT_EINVAL and "B = 0" in msg, msg
    rc, msg = _fit(lib, good, d=65)
    assert rc == TT_EINVAL and "d = 65" in msg and "1 <= d <= 64" in msg, msg
    rc, msg = _fit(lib, np.tile(np.arange(128, dtype=np.int32), (2, 1)), n=40000, d=64, k=128)
    assert rc == TT_EINVAL and "k = 128" in msg and str(16 * 128 * 64 + 4 * 128) in msg and "131072" in msg, msg
    for bad, where in ((100, "init[1][3] = 100"), (-1, "init[1][3] = -1")):
        init = good.copy()
        init[1, 3] = bad
        rc, msg = _fit(lib, init)
        assert rc == TT_EINVAL and where in msg and "[0, 100)" in msg, msg
    need = lib.tt_kmeans_fit_workspace_bytes(3, 2, 100, 50, 10)
    assert need == 3 * 2 * 100 * 4
    rc, msg = _fit(lib, good, ws_bytes=need - 1)
    assert rc == TT_EINVAL and str(need - 1) in msg and str(need) in msg, msg


def test_assign_batched_refusals(lib):
    rc = lib.tt_kmeans_assign_batched(None, 16, 16, None, 3, 10, 50, 10, None)
    assert rc == TT_EINVAL and "null pointer" in lib.tt_last_error().decode()
    rc = lib.tt_kmeans_assign_batched(16, 16, 16, None, 0, 10, 50, 10, None)
    assert rc == TT_EINVAL and "B = 0" in lib.tt_last_error().decode()
    rc = lib.tt_kmeans_assign_batched(16, 16, 16, None, 3, 10, 64, 253, None)     # beyond tt_kmeans_shape_ok, like tt_kmeans_assign
    assert rc == TT_EINVAL and "k = 253, d = 64" in lib.tt_last_error().decode()
    for d, k in ((50, 327), (64, 252), (128, 128), (1, 16384), (64, 253), (50, 328), (0, 1), (1, 0)):
        refused = lib.tt_kmeans_assign_batched(16, 16, 16, None, 3, 0, d, k, None), lib.tt_last_error().decode()   # (N = 0: never launched)
        assert ("beyond what kmeans_assign takes" in refused[1]) == (not lib.tt_kmeans_shape_ok(d, k)), (d, k, refused)


def test_assign_batched_takes_exactly_the_resident_rule(lib):
    """One centroid beyond the largest k ``tt_kmeans_shape_ok`` accepts at d is refused by the batched entry, by argument (TT_EINVAL, not a
    failed launch) and naming k and d.  The refusing side only: an accepted shape would launch on the dummy pointers."""
    for d in list(range(1, 130)) + [256, 384, 1024]:
        kmax = max(k for k in range(1, 16384 // d + 2) if lib.tt_kmeans_shape_ok(d, k))
        assert lib.tt_kmeans_shape_ok(d, kmax) and not lib.tt_kmeans_shape_ok(d, kmax + 1), (d, kmax)
        rc = lib.tt_kmeans_assign_batched(16, 16, 16, None, 3, 10, d, kmax + 1, None)
        msg = lib.tt_last_error().decode()
        assert rc == TT_EINVAL and f"k = {kmax + 1}, d = {d}" in msg and "beyond what kmeans_assign takes" in msg, (d, kmax, rc, msg)


# ---- KmeansBatch, with a NumPy stand-in for the fused kernel ------------------------------------------------------------------------------

OBJ = np.array([[5.0, 3.0, 3.0], [4.0, 1.0, 2.0], [2.0, 2.0, 9.0]])


def test_kmeans_batch_selects_the_first_best_redo_and_reruns_only_the_flagged_problem(monkeypatch, lib):
    from timetuning_amd import hip_ops
    from timetuning_amd.clustering import Kmeans, KmeansBatch

    d, k, nredo, mppc, seed = 4, 3, 3, 4, 7
    points = torch.from_numpy(np.random.RandomState(0).randn(3, 40, d).astype(np.float32))
    seen, refits = {}, []

    def fit(x, init, niter):   # centroids that name their (problem, redo); problem 1 flagged at iteration 3 of redo 2
        seen.update(x=x.clone(), init=init.clone(), niter=niter)
        B = x.shape[0]
        cent = torch.zeros((B, nredo, k, d))
        for b in range(B):
            for r in range(nredo):
                cent[b, r] = 10 * b + r
        status = torch.zeros((B, nredo), dtype=torch.int32)
        status[1, 2] = 3
        return cent, torch.from_numpy(OBJ.copy()), status

    def loop_fit(self, x, init_indices=None):
        refits.append((self, x.clone(), torch.as_tensor(np.asarray(init_indices)).clone()))
        self._centroids_dev = torch.full((k, d), -1.0)
        self.obj = [7.0, 6.0, 8.0]
        return 6.0

    monkeypatch.setattr(hip_ops, "kmeans_fit_batched", fit)
    monkeypatch.setattr(Kmeans, "_fit", loop_fit)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **kw: self)
    kb = KmeansBatch(d, k, niter=9, nredo=nredo, seed=seed, max_points_per_centroid=mppc)
    best = kb.train(points)
    # the subsample and the seeds of Kmeans.train / Kmeans._iterate, shared by all problems
    sub = Kmeans._perm(40, seed)[: k * mppc]
    assert torch.equal(seen["x"], points[:, sub]) and seen["niter"] == 9
    want_init = torch.stack([Kmeans._perm(k * mppc, seed + 1 + r * 15486557)[:k] for r in range(nredo)])
    assert torch.equal(seen["init"].long(), want_init)
    # the loop ran once, for problem 1 alone, on that subsample and those seeds, configured as the batch
    assert len(refits) == 1
    km, x1, init1 = refits[0]
    assert torch.equal(x1, points[1, sub]) and torch.equal(init1.long(), want_init)
    assert (km.d, km.k, km.niter, km.nredo, km.seed, km.max_points_per_centroid) == (d, k, 9, nredo, seed, mppc)
    assert kb.fallback == [False, True, False]
    # redo selection: the FIRST of two equal objectives (the loop's strict <); the flagged problem carries the loop's result
    assert torch.equal(kb.centroids[0], torch.full((k, d), 1.0)) and torch.equal(kb.centroids[2], torch.full((k, d), 20.0))
    assert torch.equal(kb.centroids[1], torch.full((k, d), -1.0))
    assert kb.obj == [[5.0, 3.0, 3.0], [7.0, 6.0, 8.0], [2.0, 2.0, 9.0]] and best == [3.0, 6.0, 2.0]
    assert kb.centroids.shape == (3, k, d)


def test_kmeans_batch_explicit_seeds_and_too_few_points(monkeypatch, lib):
    from timetuning_amd import hip_ops
    from timetuning_amd.clustering import KmeansBatch

    seen = {}

    def fit(x, init, niter):
        seen["init"] = init.clone()
        B, (nredo, k) = x.shape[0], init.shape
        return torch.zeros((B, nredo, k, x.shape[2])), torch.ones((B, nredo), dtype=torch.float64), torch.zeros((B, nredo), dtype=torch.int32)

    monkeypatch.setattr(hip_ops, "kmeans_fit_batched", fit)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **kw: self)
    kb = KmeansBatch(4, 3, niter=2, nredo=2)
    kb.train(torch.zeros(2, 12, 4), init_indices=[np.array([0, 5, 7]), np.array([11, 2, 3])])
    assert seen["init"].tolist() == [[0, 5, 7], [11, 2, 3]] and kb.fallback == [False, False]
    with pytest.raises(RuntimeError, match=r"Number of training points \(2\) should be at least as large as number of clusters \(3\)"):
        kb.train(torch.zeros(5, 2, 4))
