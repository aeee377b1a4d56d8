"""CPU-only checks of N18, the device-side split of empty clusters in the batched k-means fit: the table of draws
(``clustering.split_draws``), the table-driven statement of faiss' split the kernel is written against
(``clustering.split_empty_from_table``) held to ``Kmeans._split_empty``, and the new C entry's declaration and refusals."""
import os
import re

import numpy as np
import pytest
import torch

from timetuning_amd import _lib, clustering
from timetuning_amd.clustering import Kmeans, split_draws, split_empty_from_table

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TT_EINVAL = -1   # include/timetuning_hip.h
RandomState = np.random.RandomState


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


# ---- the table ------------------------------------------------------------------------------------------------------------------------

def test_split_draws_is_the_generators_sequence_cached():
    for n in (1, 7, 4096):
        t = split_draws(n)
        assert t.dtype == torch.float64 and t.shape == (n,) and t.device.type == "cpu"
        assert np.array_equal(t.numpy(), RandomState(1234).random_sample(n))
        assert split_draws(n) is t
    assert split_draws() is split_draws(4096) and clustering.SPLIT_DRAWS == 4096
    assert np.array_equal(split_draws(7).numpy(), split_draws(4096).numpy()[:7])   # every call of the host reads a prefix of one sequence


# ---- the table walk against Kmeans._split_empty ---------------------------------------------------------------------------------------

class Counting:
    """``numpy.random.RandomState`` that counts the draws of the generator made last, or hands out ``fixed`` instead of drawing."""
    used, fixed = 0, None

    def __init__(self, seed):
        assert seed == 1234
        self.rs = RandomState(seed)
        Counting.used = 0

    def random_sample(self):
        Counting.used += 1
        return self.rs.random_sample() if Counting.fixed is None else Counting.fixed


def host_split(cent, counts, n):
    """``Kmeans._split_empty`` on copies -> (centroids, counts, splits, draws consumed)."""
    cent, counts = cent.clone(), counts.copy()
    nsplit = Kmeans(cent.shape[1], cent.shape[0])._split_empty(cent, counts, n)
    return cent, counts, nsplit, Counting.used


def drawn_cases():
    """(name, counts [k], d): a few hundred count vectors with zeros, k in 2 ... 21, d in {1, 3, 50, 64}, and the named edges."""
    rng = RandomState(18)
    cases = []
    for i in range(320):
        k, d = int(rng.randint(2, 22)), (1, 3, 50, 64)[i % 4]
        counts = rng.randint(1, 40, size=k)
        kind = i % 5
        if kind == 0:      # one empty cluster
            counts[rng.randint(k)] = 0
        elif kind == 1:    # several
            counts[rng.choice(k, size=max(1, k // 2), replace=False)] = 0
        elif kind == 2:    # donors of count 1 (never accepted) and empties in front of the walk, the mass behind
            counts[: max(1, k // 2)] = rng.randint(0, 2, size=max(1, k // 2))
            counts[0] = 0 if k > 2 else counts[0]
            counts[-1] += 50
            counts[rng.randint(k)] = 0
        elif kind == 3:    # nearly everything empty: clusters that were just filled have to donate
            counts[:] = 0
            counts[rng.randint(k)] = int(rng.randint(2 * k, 400))
        else:              # one large donor at the end of the walk, small ones before it
            counts[:] = rng.randint(0, 3, size=k)
            counts[-1] = 300
        cases.append((f"drawn{i}.{kind}", counts.astype(np.int64), d))
    cases.append(("one donor behind three empties", np.array([0, 0, 0, 64, 0], dtype=np.int64), 3))
    cases.append(("n == k", np.array([2, 0, 1, 1], dtype=np.int64), 3))                     # n = 4 = k: no split at all
    cases.append(("every count <= 1", np.array([1, 0, 1, 0, 1, 1], dtype=np.int64), 50))    # n = 4 < k = 6 - and below with n > k
    cases.append(("ones in front", np.array([1, 1, 1, 0, 1, 9, 0, 30], dtype=np.int64), 64))
    cases.append(("int32 counts", np.array([0, 7, 0, 11], dtype=np.int32), 1))
    return cases


def test_table_walk_equals_split_empty_over_drawn_cases(monkeypatch):
    table = split_draws().numpy()
    monkeypatch.setattr(np.random, "RandomState", Counting)
    rng = RandomState(19)
    seen = {"several": 0, "stopped": 0, "none": 0, "short": 0}
    most = 0
    for name, counts, d in drawn_cases():
        k = len(counts)
        cent = torch.from_numpy(rng.standard_normal((k, d)).astype(np.float32))
        for n in sorted({int(counts.sum()), k + 1} if name == "every count <= 1" else {int(counts.sum())}):
            want_c, want_n, want_s, used = host_split(cent, counts, n)
            got_c, got_n = cent.clone(), counts.copy()
            got_s = split_empty_from_table(got_c, got_n, n, table)
            assert got_s == want_s and torch.equal(got_c, want_c) and (got_n == want_n).all() and got_n.dtype == counts.dtype, (name, n)
            most = max(most, used)
            seen["several"] += want_s > 1
            seen["stopped"] += want_s < int((counts == 0).sum())
            seen["none"] += want_s == 0
            if used:   # one draw short of what the call needs: refused, not finished differently
                assert split_empty_from_table(cent.clone(), counts.copy(), n, table[: used - 1]) == -1, (name, used)
                assert split_empty_from_table(cent.clone(), counts.copy(), n, torch.from_numpy(table[:used])) == want_s, (name, used)
                seen["short"] += 1
    print("cases", seen, "most draws in one call", most)
    assert all(v > 0 for v in seen.values()), seen
    assert most < clustering.SPLIT_DRAWS


def test_a_cluster_filled_in_this_call_donates_and_the_edges_by_hand(monkeypatch):
    """The named edges once more, with what must come out written down."""
    # n == k and every count <= 1 (n > k): nothing is split and nothing is drawn - an empty table is enough
    for counts, n in ((np.array([2, 0, 1, 1]), 4), (np.array([1, 0, 1, 0, 1, 1]), 7)):
        cent = torch.arange(len(counts) * 2, dtype=torch.float32).view(-1, 2)
        keep, before = cent.clone(), counts.copy()
        assert split_empty_from_table(cent, counts, n, np.zeros(0)) == 0 and torch.equal(cent, keep) and (counts == before).all()
    # draws of 0 accept the first cluster of the walk that holds two points or more.  counts [0, 0, 8], n = 8: cluster 0 takes half of
    # cluster 2 after three draws (clusters 0 and 1 refuse: p < 0), then cluster 1 takes half of cluster 0, filled a moment ago, at once
    monkeypatch.setattr(np.random, "RandomState", Counting)
    monkeypatch.setattr(Counting, "fixed", 0.0)
    counts = np.array([0, 0, 8])
    cent = torch.from_numpy(RandomState(21).standard_normal((3, 5)).astype(np.float32))
    sign = torch.tensor([1 + 2.0 ** -10, 1 - 2.0 ** -10] * 3)[:5]
    c0 = cent[2] * sign
    want = torch.stack([c0 * (2.0 - sign), c0 * sign, cent[2] * (2.0 - sign)])
    host_c, host_n, host_s, used = host_split(cent, counts, 8)
    assert host_s == 2 and used == 4 and host_n.tolist() == [2, 2, 4] and torch.equal(host_c, want)
    got_c, got_n = cent.clone(), counts.copy()
    assert split_empty_from_table(got_c, got_n, 8, np.zeros(4)) == 2 and got_n.tolist() == [2, 2, 4] and torch.equal(got_c, want)
    assert split_empty_from_table(cent.clone(), counts.copy(), 8, np.zeros(3)) == -1


def test_vanishing_acceptance_takes_the_first_largest_cluster(monkeypatch):
    """A table whose draws are all >= 1 is never accepted: after 64 k + 1 of them the donor is the first arg-max of the counts, as in
    ``_split_empty`` with its generator handing out the same draws."""
    monkeypatch.setattr(np.random, "RandomState", Counting)
    monkeypatch.setattr(Counting, "fixed", 1.0)
    counts = np.array([3, 0, 9, 2, 9, 0], dtype=np.int64)
    k, d = len(counts), 3
    cent = torch.from_numpy(RandomState(20).standard_normal((k, d)).astype(np.float32))
    want_c, want_n, want_s, used = host_split(cent, counts, int(counts.sum()))
    assert want_s == 2 and used == 2 * (64 * k + 1)
    assert want_n.tolist() == [3, 4, 5, 2, 5, 4]        # 9 -> 5 + 4 from cluster 2, the first of the two 9s, then from cluster 4
    got_c, got_n = cent.clone(), counts.copy()
    assert split_empty_from_table(got_c, got_n, int(counts.sum()), np.ones(used)) == 2
    assert torch.equal(got_c, want_c) and (got_n == want_n).all()
    assert split_empty_from_table(cent.clone(), counts.copy(), int(counts.sum()), np.ones(used - 1)) == -1


# ---- the C entry ----------------------------------------------------------------------------------------------------------------------

def test_split_entry_is_declared_bound_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "timetuning_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tt_[a-z0-9_]+)\s*\(", text))
    name = "tt_kmeans_fit_batched_split"
    assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    old, new = _lib.SIGNATURES["tt_kmeans_fit_batched"][1], _lib.SIGNATURES[name][1]
    assert new[: len(old) - 1] == old[:-1] and len(new) == len(old) + 2      # the old arguments, then draws and n_draws before the stream
    assert lib.tt_abi_version() == 8                                          # additive
    assert f"{len(declared)} entry points" in open(os.path.join(REPO, "README.md")).read()


def _fit(lib, init_host, x=16, init=16, cent=16, obj=16, status=16, B=3, n=100, d=50, k=10, nredo=2, niter=5, ws=16, ws_bytes=1 << 40, draws=16,
         n_draws=4096):
    # (every refusal comes before any pointer is read or any kernel launched: dummy non-null device pointers, no GPU)
    host = None if init_host is None else init_host.ctypes.data
    rc = lib.tt_kmeans_fit_batched_split(x, init, host, cent, obj, status, B, n, d, k, nredo, niter, ws, ws_bytes, draws, n_draws, None)
    return rc, lib.tt_last_error().decode()


def test_split_entry_refusals_name_their_numbers(lib):
    good = np.tile(np.arange(10, dtype=np.int32), (2, 1))
    rc, msg = _fit(lib, good, draws=None)
    assert rc == TT_EINVAL and msg.startswith("kmeans_fit_batched_split: null pointer"), msg
    for n_draws in (0, -3):
        rc, msg = _fit(lib, good, n_draws=n_draws)
        assert rc == TT_EINVAL and f"n_draws = {n_draws}" in msg, msg
    # everything tt_kmeans_fit_batched refuses
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
    rc, msg = _fit(lib, good, ws_bytes=need - 1)
    assert rc == TT_EINVAL and str(need - 1) in msg and str(need) in msg, msg
    assert msg.startswith("kmeans_fit_batched_split: ")


def test_front_end_takes_the_table_and_kmeans_batch_its_switch():
    import inspect

    from timetuning_amd import hip_ops

    sig = inspect.signature(hip_ops.kmeans_fit_batched)
    assert list(sig.parameters) == ["x", "init", "niter", "split_draws"] and sig.parameters["split_draws"].default is None
    assert clustering.KmeansBatch(4, 3).split == "host" and clustering.KmeansBatch(4, 3, split="device").split == "device"
    assert clustering.DEVICE_SPLIT is True
    with pytest.raises(ValueError, match="split = 'loop'"):
        clustering.KmeansBatch(4, 3, split="loop")


OBJ = np.array([[5.0, 3.0, 3.0], [4.0, 1.0, 2.0], [2.0, 2.0, 9.0]])


@pytest.mark.parametrize("table_short", [False, True])
def test_kmeans_batch_refits_only_the_flagged_problem_with_the_table(monkeypatch, table_short):
    """``KmeansBatch(split="device")`` around a stand-in for the two entries: the first launch is the old entry on every problem, the
    second the splitting entry on the flagged problem alone; the loop runs only where that one is flagged again."""
    from timetuning_amd import hip_ops

    d, k, nredo = 4, 3, 3
    points = torch.from_numpy(RandomState(0).randn(3, 12, d).astype(np.float32))
    calls, refits = [], []

    def fit(x, init, niter, split_draws=None):
        calls.append((x.clone(), split_draws))
        B = x.shape[0]
        status = torch.zeros((B, nredo), dtype=torch.int32)
        if split_draws is None:
            cent = torch.stack([torch.full((nredo, k, d), 10.0 * b) + torch.arange(nredo).view(-1, 1, 1) for b in range(B)])
            status[1, 2] = 3
            return cent, torch.from_numpy(OBJ.copy()), status
        status[0, 0] = 2 if table_short else 0
        return torch.full((B, nredo, k, d), 77.0), torch.tensor([[9.0, 0.5, 8.0]], dtype=torch.float64), status

    def loop_fit(self, x, init_indices=None):
        refits.append(x.clone())
        self._centroids_dev = torch.full((k, d), -1.0)
        self.obj = [7.0, 6.0, 8.0]
        return 6.0

    monkeypatch.setattr(hip_ops, "kmeans_fit_batched", fit)
    monkeypatch.setattr(Kmeans, "_fit", loop_fit)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **kw: self)
    kb = clustering.KmeansBatch(d, k, niter=9, nredo=nredo, seed=7, split="device")
    best = kb.train(points)
    assert len(calls) == 2 and calls[0][1] is None and torch.equal(calls[0][0], points)
    assert torch.equal(calls[1][0], points[1:2]) and calls[1][1] is split_draws(device=points.device)
    assert torch.equal(kb.centroids[0], torch.full((k, d), 1.0)) and torch.equal(kb.centroids[2], torch.full((k, d), 20.0))
    if table_short:
        assert kb.fallback == [False, True, False] and kb.status.tolist() == [[0, 0, 0], [2, 0, 0], [0, 0, 0]]
        assert len(refits) == 1 and torch.equal(refits[0], points[1])
        assert torch.equal(kb.centroids[1], torch.full((k, d), -1.0)) and kb.obj[1] == [7.0, 6.0, 8.0] and best == [3.0, 6.0, 2.0]
    else:
        assert kb.fallback == [False] * 3 and (kb.status == 0).all() and refits == []
        assert torch.equal(kb.centroids[1], torch.full((k, d), 77.0)) and kb.obj[1] == [9.0, 0.5, 8.0] and best == [3.0, 0.5, 2.0]
    # a table handed in reaches the second launch as it is
    calls.clear()
    one = torch.zeros(1, dtype=torch.float64)
    kb.train(points, _draws=one)
    assert calls[1][1] is one
