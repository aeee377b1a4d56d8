"""CPU checks of N9 (label propagation on rectangular token grids): the --frame_size / --size_mask_neighborhood 0 flags, the routing
rule between the square entry and tt_label_propagate_grid_maps, and the grid workspace query, a pure host function."""
import os
from types import SimpleNamespace

import pytest
import torch

from timetuning_amd import _lib
from timetuning_amd import mask_propagation as MP


def test_frame_size_flag():
    p = MP.build_parser()
    a = p.parse_args([])
    assert a.frame_size is None and MP.clip_size(a, 16) == (224, 224)
    a = p.parse_args(["--frame_size", "96", "160", "--size_mask_neighborhood", "0"])
    assert a.frame_size == [96, 160] and a.size_mask_neighborhood == 0
    assert MP.clip_size(a, 16) == (96, 160) and MP.clip_size(a, 8) == (96, 160)
    for bad in (["100", "160"], ["96", "150"], ["0", "160"]):
        with pytest.raises(ValueError):
            MP.clip_size(p.parse_args(["--frame_size"] + bad), 16)
    with pytest.raises(SystemExit):
        p.parse_args(["--frame_size", "96"])


def test_cli_rejects_frame_size_off_the_patch_grid_before_any_gpu_work():
    args = MP.build_parser().parse_args(["--dataset", "synthetic", "--model_path", "", "--frame_size", "96", "150"])
    with pytest.raises(ValueError):
        MP.mask_propagation(args)


def test_synthetic_clip_width():
    f, m = MP.synthetic_tracking_clip(3, 96, seed=1, width=160)
    assert f.shape == (3, 3, 96, 160) and m.shape == (3, 96, 160) and set(m.unique().tolist()) == {0, 1, 2}
    f2, m2 = MP.synthetic_tracking_clip(3, 96, seed=1, width=96)
    f3, m3 = MP.synthetic_tracking_clip(3, 96, seed=1)
    assert torch.equal(f2, f3) and torch.equal(m2, m3)


def test_routing_rule():
    acc = MP.square_entry_accepts
    assert acc((14, 14), 9, 7, 6)                # training protocol: 13 x 13 x 8 = 1 352
    assert acc((28, 28), 25, 4, 12)              # DAVIS protocol on 28 x 28: 25 x 25 x 5 = 3 125
    assert not acc((28, 28), 25, 7, 12)          # 5 000 > 4 096
    assert acc((28, 28), 3, 7, 12)               # a 3-frame clip has 2 context frames: 1 250
    assert acc((10, 10), 9, 7, 12)               # window clipped to the grid: 10 x 10 x 8
    assert not acc((30, 30), 9, 7, 12)
    assert not acc((14, 14), 9, 4, 0)            # unrestricted variant
    assert not acc((5, 9), 9, 4, 3) and not acc((9, 5), 9, 4, 3)


class _Stub:
    spatial_resolution = 14


def _route(monkeypatch, **kw):
    calls = []
    monkeypatch.setattr(MP.ops, "l2norm_fwd", lambda x: x)
    monkeypatch.setattr(MP.ops, "label_propagate_maps", lambda xn, s, *a: calls.append(("square", a)) or torch.zeros(
        xn.shape[0] - 1, 1, xn.shape[2], s.shape[-1], dtype=torch.float64))
    monkeypatch.setattr(MP.ops, "label_propagate_grid_maps", lambda xn, s, grid, *a: calls.append(("grid", tuple(grid), a)) or torch.zeros(
        xn.shape[0] - 1, 1, xn.shape[2], s.shape[-1], dtype=torch.float64))
    return calls


@pytest.mark.parametrize("grid,radius,n_last,entry", [(None, 12, 4, "square"), ((14, 14), 6, 7, "square"), ((14, 14), 0, 4, "grid"),
                                                      ((5, 9), 3, 4, "grid"), ((9, 5), 1, 0, "grid")])
def test_propagate_labels_routes(monkeypatch, grid, radius, n_last, entry):
    calls = _route(monkeypatch)
    gh, gw = grid or (14, 14)
    feats = torch.randn(5, gh * gw, 8)
    first = torch.rand(1, 3, 2 * gh, 2 * gw)
    kw = {} if grid is None else {"grid": grid}
    maps = MP.propagate_labels(n_last, radius, 5, _Stub(), feats, first, features_exist=True, **kw)
    assert len(maps) == 4 and maps[0].shape == (3, gh, gw)
    assert calls[0][0] == entry and len(calls) == 1
    if entry == "grid":
        assert calls[0][1] == (gh, gw) and calls[0][2][:3] == (n_last, radius, 5)


def test_propagate_labels_grid_must_hold_the_tokens(monkeypatch):
    _route(monkeypatch)
    with pytest.raises(ValueError):
        MP.propagate_labels(4, 12, 5, _Stub(), torch.randn(3, 45, 8), torch.rand(1, 2, 5, 9), features_exist=True)   # default 14 x 14


def test_grid_workspace_query_without_gpu():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    # a square grid needs what the square entry needs
    for bs, fs, g, K, nl in ((2, 9, 14, 5, 7), (1, 25, 28, 8, 4), (3, 4, 10, 21, 0)):
        assert lib.tt_label_propagate_grid_workspace_bytes(bs, fs, g, g, 64, K, nl, 12) == lib.tt_label_propagate_workspace_bytes(bs, fs, g, 64, K, nl)
    # 60 x 106 tokens (ViT-S/8 at 480 x 848), one clip of 50 frames, n_last 4: one target frame per chunk, 5 context slots of n^2 fp32
    n = 60 * 106
    sims = (5 * n * n * 4 + 255) // 256 * 256
    nb = lib.tt_label_propagate_grid_workspace_bytes(1, 50, 60, 106, 384, 5, 4, 12)
    assert nb == sims + 49 * n * 5 * 8
    assert lib.tt_label_propagate_grid_workspace_bytes(1, 50, 60, 106, 384, 5, 4, 0) == nb   # the window does not change it
    assert lib.tt_label_propagate_grid_workspace_bytes(1, 50, 106, 60, 384, 5, 4, 12) == nb
    for bad in ((0, 9, 5, 9, 16, 3, 4, 3), (1, 1, 5, 9, 16, 3, 4, 3), (1, 9, 0, 9, 16, 3, 4, 3), (1, 9, 5, 9, 16, 0, 4, 3)):
        assert lib.tt_label_propagate_grid_workspace_bytes(*bad) == 0
