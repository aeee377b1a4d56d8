"""CPU-only checks of N12, k-means beyond the LDS limit: the five new C entries and their host-side rules (shape rule, default tile,
workspace size), the routing of ``clustering.Kmeans`` between the resident and the tiled kernel pair (with NumPy stand-ins for the
four kernels), and the evaluation command line (``evaluation.py:490-566``)."""
import os
import re

import numpy as np
import pytest
import torch

from timetuning_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tt_kmeans_tiled_shape_ok", "tt_kmeans_tile_centroids", "tt_kmeans_assign_tiled", "tt_kmeans_accumulate_tiled_workspace_bytes",
       "tt_kmeans_accumulate_tiled")


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
    assert lib.tt_abi_version() == 8


def test_default_tile_fills_at_most_64_kb(lib):
    for d in list(range(1, 131)) + [256, 384, 1024]:
        tile = lib.tt_kmeans_tile_centroids(d)
        assert tile * d * 4 <= 65536 < (tile + 1) * d * 4, d
    assert lib.tt_kmeans_tile_centroids(50) == 327 and lib.tt_kmeans_tile_centroids(0) == 0 and lib.tt_kmeans_tile_centroids(1025) == 0


def test_tiled_shape_rule(lib):
    for d, k in ((50, 500), (64, 253), (1, 16385), (1024, 4096)):
        assert lib.tt_kmeans_tiled_shape_ok(d, k), (d, k)
    for d, k in ((0, 5), (5, 0), (1025, 5)):
        assert not lib.tt_kmeans_tiled_shape_ok(d, k), (d, k)
    assert lib.tt_kmeans_tiled_shape_ok(1024, 2 ** 21 - 1) and not lib.tt_kmeans_tiled_shape_ok(1024, 2 ** 21)   # k * d < 2^31


def test_workspace_query_is_monotone_and_holds_one_partial(lib):
    for d, k in ((50, 500), (64, 253), (1, 16385), (128, 129), (16, 1025)):
        for tile_k in (0, 1, 13):
            sizes = [lib.tt_kmeans_accumulate_tiled_workspace_bytes(P, d, k, tile_k) for P in (1, 127, 128, 129, 7001, 128000, 524288, 524289, 10 ** 7)]
            assert sizes == sorted(sizes) and sizes[0] >= k * d * 8 + k * 8, (d, k, tile_k, sizes)


def test_a_tile_beyond_the_default_is_refused_with_both_numbers(lib):
    # (the refusal comes before any pointer is read or any kernel launched: dummy non-null pointers, no GPU)
    rc = lib.tt_kmeans_assign_tiled(16, 16, 16, None, 10, 50, 500, 328, None)
    assert rc != 0
    msg = lib.tt_last_error().decode()
    assert "328" in msg and "327" in msg, msg
    rc = lib.tt_kmeans_accumulate_tiled(16, 16, 16, 16, 10, 50, 500, 328, 16, 1 << 40, None)
    assert rc != 0 and "328" in lib.tt_last_error().decode() and "327" in lib.tt_last_error().decode()
    rc = lib.tt_kmeans_assign_tiled(16, 16, 16, None, 10, 1025, 5, 0, None)
    assert rc != 0 and "1 <= d <= 1024" in lib.tt_last_error().decode()


# ---- driver routing, with NumPy stand-ins for the four kernels ----------------------------------------------------------------------

def _stub_ops(monkeypatch, calls):
    from timetuning_amd import hip_ops

    def assign(name):
        def f(x, c, return_dist=False, **kw):
            calls.append(name)
            d2 = ((x.numpy()[:, None, :].astype(np.float64) - c.numpy()[None].astype(np.float64)) ** 2).sum(-1)
            labels = torch.from_numpy(d2.argmin(1).astype(np.int32))
            return (labels, torch.from_numpy(d2.min(1).astype(np.float32))) if return_dist else labels
        return f

    def accumulate(name):
        def f(x, labels, k, **kw):
            calls.append(name)
            sums = np.zeros((k, x.shape[1]), np.float64)
            np.add.at(sums, labels.numpy(), x.numpy().astype(np.float64))
            return torch.from_numpy(sums), torch.from_numpy(np.bincount(labels.numpy(), minlength=k).astype(np.int64))
        return f

    monkeypatch.setattr(hip_ops, "kmeans_assign", assign("assign"))
    monkeypatch.setattr(hip_ops, "kmeans_accumulate", accumulate("accumulate"))
    monkeypatch.setattr(hip_ops, "kmeans_assign_tiled", assign("assign_tiled"))
    monkeypatch.setattr(hip_ops, "kmeans_accumulate_tiled", accumulate("accumulate_tiled"))
    monkeypatch.setattr(hip_ops, "kmeans_shape_ok", lambda d, k: bool(_lib.load().tt_kmeans_shape_ok(d, k)))   # (the library's own rule)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)


def test_driver_routes_by_the_resident_rule(monkeypatch, lib):
    from timetuning_amd import synth
    from timetuning_amd.clustering import Kmeans

    calls = []
    _stub_ops(monkeypatch, calls)
    x = torch.from_numpy(synth.normal("kt.host.x", (1200, 50)))
    small = Kmeans(50, 300, niter=2, nredo=1)
    small.train(x)
    assert set(calls) == {"assign", "accumulate"} and np.isfinite(small.centroids).all() and small.centroids.shape == (300, 50)
    small.assign(x)
    assert set(calls) == {"assign", "accumulate"}
    del calls[:]
    big = Kmeans(50, 500, niter=2, nredo=1)
    big.train(x)
    assert set(calls) == {"assign_tiled", "accumulate_tiled"} and np.isfinite(big.centroids).all() and big.centroids.shape == (500, 50)
    big.assign(x)
    big.train_upsampled(x.view(3, 400, 50), 20)
    assert set(calls) == {"assign_tiled", "accumulate_tiled"}
    # the resident driver keeps its refusal, and shapes beyond the tiled rule are refused before any kernel as well
    del calls[:]
    with pytest.raises(_lib.HipLibraryError, match="k = 253 centroids of d = 64"):
        Kmeans(64, 253)._lloyd(torch.zeros(300, 64))
    with pytest.raises(_lib.HipLibraryError, match="tiled k-means kernels"):
        Kmeans(1025, 20).train(torch.zeros(30, 1025))
    assert calls == []


# ---- the evaluation command line -----------------------------------------------------------------------------------------------------

def test_evaluation_cli_surface_and_bool_quirk():
    from timetuning_amd.evaluation import build_parser, main

    a = build_parser().parse_args([])
    want = dict(architecture="dino-s16", model_path="/home/ssalehi/video/vos_pretrained/cyclic_swav/src/leopart_vits16.ckpt", dataset="davis_val",
                dataset_path="../data", destination_path="ytvos", evaluation_protocol="frame-wise", logging_directory="visualizations",
                batch_size=16, num_workers=3, num_clusters=10, input_resolution=224, many_to_one=False, num_frames=4, precision_based=False,
                uvos=False, use_teacher=False, EMA_decay=0.999)
    for name, value in want.items():
        assert getattr(a, name) == value and type(getattr(a, name)) is type(value), name
    assert build_parser().parse_args(["--many_to_one", "False"]).many_to_one is True     # type=bool (evaluation.py:557)
    assert build_parser().parse_args(["--many_to_one", ""]).many_to_one is False
    b = build_parser().parse_args(["--num_clusters", "500", "--evaluation_protocol", "dataset-wise", "--eval_clips", "3"])
    assert (b.num_clusters, b.evaluation_protocol, b.eval_clips) == (500, "dataset-wise", 3)
    with pytest.raises(NotImplementedError, match="dataset readers"):
        main(["--dataset", "davis_val"])
