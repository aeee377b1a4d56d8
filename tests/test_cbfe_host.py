"""CPU checks of the cluster-based foreground extraction surface (N6, ``timetuning_amd.cluster_based_foreground_extraction``).

The fixture tests/golden/cbfe.npz comes from the reference's own functions (tools/gen_cbfe_golden.py).  Here: its inputs regenerate,
the host-side pieces (label scaling, torch's nearest index tables, the threshold and foreground-set choices, the nearest upsampling of
features) reproduce it, and the driver's flags are the reference's.  The kernels are checked on the GPU (test_hip_cbfe.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from timetuning_amd import cluster_based_foreground_extraction as CB
from timetuning_amd.clustering import nearest_index_table

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_maps(g, k, val=False):
    """The fixture's train (or val) cluster maps, attention masks and labels, regenerated as tools/gen_cbfe_golden.py made them."""
    M, R, off = [int(v) for v in g["cfg"]]
    seed = int(g[f"k{k}_seed"]) + (off if val else 0)
    return CB.synthetic_cluster_maps(M, R, k, seed)


def unpack_mask(g, k):
    M, R, _ = [int(v) for v in g["cfg"]]
    return torch.from_numpy(np.unpackbits(g[f"k{k}_soft_mask_bits"])[: M * R * R].astype(np.int64).reshape(M, R, R))


@pytest.mark.parametrize("k", [60, 300])
def test_regenerated_inputs_are_the_references(golden, k):
    g = golden("cbfe")
    cl, at, gt = golden_maps(g, k)
    assert np.array_equal(cl[:, ::17, ::13].numpy(), g[f"k{k}_clusters_sample"])
    assert np.array_equal(at[:, ::17, ::13].numpy(), g[f"k{k}_attn_sample"])
    assert np.array_equal(gt[:, ::17, ::13].numpy(), g[f"k{k}_gt_sample"])
    vcl, _, _ = golden_maps(g, k, val=True)
    assert np.array_equal(vcl[:, ::17, ::13].numpy(), g[f"k{k}_val_clusters_sample"])
    assert (gt == 255).any() and set(np.unique(cl.numpy())) == set(range(k))
    precs = g[f"k{k}_precs"]
    starts = CB.cut_positions(k)
    # ties at exactly 1.0 straddle the cut positions, and exact 0.0 ties exist
    pos1 = np.where(np.sort(precs) == 1.0)[0]
    assert len(pos1) > 1 and starts[0] < pos1[0] <= starts[-1]
    assert (precs == 0.0).sum() > 1


def test_process_data_group_all_labels(golden):
    g = golden("cbfe")
    ann = torch.arange(256, dtype=torch.float32).div(255).view(1, 1, 16, 16)
    data = torch.zeros(1, 3, 2, 2)
    d, lab = CB.process_data_group((data, ann), CB.ScaleType.ZERO_TO_255)
    assert lab.dtype == torch.int64 and d.shape == (1, 1, 3, 2, 2)
    assert np.array_equal(lab.numpy(), g["labels256"].astype(np.int64))
    # video groups lose the clip axis, and ZERO_TO_ONE leaves the annotations alone
    v, a = CB.process_data_group((torch.zeros(2, 1, 3, 3, 4, 4), torch.ones(2, 1, 3, 4, 4), None))
    assert v.shape == (2, 3, 3, 4, 4) and a.shape == (2, 3, 4, 4) and a.dtype == torch.float32


@pytest.mark.parametrize("g,R", [(28, 100), (14, 100), (28, 448), (56, 100), (60, 100)])
def test_nearest_index_tables(g, R):
    iy, ix = nearest_index_table(g, R)
    assert iy.dtype == np.int32 and iy.shape == (R,) and ix.shape == (R,)
    lab = torch.from_numpy(np.random.default_rng(g * 1000 + R).integers(0, 1 << 20, (2, 1, g, g))).double()
    ref = F.interpolate(lab, size=(R, R), mode="nearest")[:, 0].long()
    mine = lab[:, 0].long()[:, iy][:, :, ix]
    assert torch.equal(mine, ref)


@pytest.mark.parametrize("g,r", [(28, 100), (14, 37)])
def test_interpolate_matches_the_reference(golden, g, r):
    gold = golden("cbfe")[f"interp_{g}_{r}"]
    dim = gold.shape[2]
    feats = torch.arange(2 * g * g * dim, dtype=torch.float32).view(2, 1, g * g, dim)
    obj = CB.ClusterBasedForegroundExtraction.__new__(CB.ClusterBasedForegroundExtraction)
    torch.nn.Module.__init__(obj)
    up = obj.interpolate(feats, r)
    assert up.shape == gold.shape and up.is_contiguous()
    assert np.array_equal(up.numpy().astype(np.int32), gold)


@pytest.mark.parametrize("k", [60, 300])
def test_host_threshold_and_foreground_sets(golden, k):
    g = golden("cbfe")
    p = f"k{k}_"
    assert np.array_equal(np.argsort(g[p + "precs"]).astype(np.int32), g[p + "order"])   # this numpy breaks the ties as the reference's did
    res = list(zip(g[p + "cut_prec"], g[p + "cut_start"].tolist(), g[p + "cut_jac"].tolist()))
    assert sorted(g[p + "cut_start"].tolist()) == CB.cut_positions(k)
    th = CB.threshold_from_cuts(res)
    assert th == g[p + "threshold"]
    fg = CB.foreground_ids(g[p + "val_precs"], th)
    assert np.array_equal(fg, g[p + "val_fg_ids"])
    # the stored mask is exactly those clusters of the val maps
    vcl, _, _ = golden_maps(g, k, val=True)
    table = np.zeros(k, np.int64)
    table[fg] = 1
    assert torch.equal(torch.from_numpy(table)[vcl], unpack_mask(g, k))


REFERENCE_FLAGS = {
    "architecture": "dino-s16", "model_path": "/home/ssalehi/video/dino/outputs/checkpoint0080.pth", "dataset": "davis",
    "dataset_path": "../data", "destination_path": "ytvos", "evaluation_protocol": "dataset-wise", "logging_directory": "visualizations",
    "batch_size": 16, "num_workers": 3, "k_fg_extraction": 300, "num_clusters": 21, "input_resolution": 448, "many_to_one": False,
    "num_frames": 4, "precision_based": False, "uvos": False, "use_teacher": False, "EMA_decay": 0.999,
}


def test_parser_has_the_reference_flags():
    args = vars(CB.build_parser().parse_args([]))
    for name, default in REFERENCE_FLAGS.items():
        assert name in args, name
        assert args[name] == default and type(args[name]) is type(default), (name, args[name])


def test_import_and_parser_need_no_gpu():
    code = ("import torch; from timetuning_amd import cluster_based_foreground_extraction as CB; CB.build_parser().parse_args([]); "
            "assert not torch.cuda.is_initialized(); print('ok')")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
