"""N31 without a GPU: the restatements of tests/_nn_ref.py against each other, the memory bank's seeded sampling, the command line's
surface, the new entries' shape queries and the search's tiling plan."""
import itertools

import numpy as np
import pytest
import torch

import _nn_ref as R
from timetuning_amd import _lib, hip_ops, nn_retrieval


def test_select_restatements_agree_on_ties_nan_and_short_banks():
    g = torch.Generator().manual_seed(3)
    for Q, n, k in [(3, 1, 1), (4, 7, 5), (5, 40, 5), (2, 40, 64), (6, 100, 30)]:
        sims = torch.randint(0, 8, (Q, n), generator=g).float()            # eight values: ties everywhere
        sims[0, :] = 2.0                                                   # an all-equal row
        if n > 3:
            sims[1, ::3] = float("nan")
            sims[1, 1] = float("-inf")
        if Q > 2:
            sims[2, :] = float("nan")                                      # nothing to select
        index = torch.randperm(n, generator=g) + 1000                      # columns in no particular index order
        a, b = R.select(sims, index, k), R.select_slow(sims, index, k)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (Q, n, k)
        assert (a[1][a[0] == R.NEG_INF] == -1).all() and (a[0][a[1] == -1] == R.NEG_INF).all()
        if Q > 2:
            assert (a[1][2] == -1).all()
        assert a[1][0].tolist()[: min(k, n)] == sorted(index.tolist())[: min(k, n)]      # equal values: ascending indices


def test_select_is_independent_of_the_cut_into_blocks():
    g = torch.Generator().manual_seed(4)
    sims, k = torch.randint(0, 8, (5, 300), generator=g).float(), 30
    whole = R.select(sims, torch.arange(300), k)
    for width in (1, 64, 100):
        vals, idx = torch.full((5, k), R.NEG_INF), torch.full((5, k), -1, dtype=torch.int64)
        for n0 in reversed(range(0, 300, width)):                          # blocks in reversed order, merged list by list
            cols = torch.arange(n0, min(n0 + width, 300))
            for q in range(5):
                have = idx[q] >= 0
                v, i = R.select(torch.cat([vals[q, have], sims[q, cols]])[None], torch.cat([idx[q, have], cols]), k)
                vals[q], idx[q] = v[0], i[0]
        assert torch.equal(vals, whole[0]) and torch.equal(idx, whole[1]), width


def test_counts_restatement_against_a_loop():
    g = torch.Generator().manual_seed(5)
    M, grid, Rr, C = 2, 3, 12, 4
    maps = torch.randint(0, C, (M, Rr, Rr), generator=g).to(torch.uint8)
    maps[0, :4, :4] = 255                                                  # a cell of ignored pixels only
    maps[1, 5, 5] = 255
    cnt, valid, bad = R.counts(maps, grid, C, 255)
    cell = Rr // grid
    for m, py, px, c in itertools.product(range(M), range(grid), range(grid), range(C)):
        want = int((maps[m, py * cell:(py + 1) * cell, px * cell:(px + 1) * cell] == c).sum())
        assert int(cnt[m, py * grid + px, c]) == want
    assert bad == -1 and int(valid[0, 0]) == 0 and int(valid.sum()) == M * Rr * Rr - 17
    maps[1, 0, 0] = C
    assert R.counts(maps, grid, C, 255)[2] == 1
    assert R.counts(maps, grid, C, None)[2] == 0                           # without an ignore value 255 itself is out of range


def test_aggregate_restatement_on_known_weights():
    labels = torch.eye(3)
    vals = torch.tensor([[0.5, 0.5, 0.1], [0.9, R.NEG_INF, R.NEG_INF], [R.NEG_INF] * 3])
    idx = torch.tensor([[0, 1, 2], [2, -1, -1], [-1, -1, -1]])
    out = R.aggregate(vals, idx, labels, 0.1)
    e = np.exp(-4.0)
    assert np.allclose(out[0].numpy(), np.array([1, 1, e]) / (2 + e), rtol=1e-12)
    assert out[1].tolist() == [0.0, 0.0, 1.0] and out[2].tolist() == [0.0, 0.0, 0.0]
    sims = torch.tensor([[0.1, 0.9, 0.3, 0.2]] * 4)                        # one token grid of 2 x 2, every query retrieves bank row 1
    assert (R.predict(sims, torch.eye(4)[:, :3].contiguous(), 1, 1, 0.02, 6) == 1).all()


def test_memory_bank_sampling_is_seeded():
    valid = torch.tensor([[3, 0, 1, 5, 0, 2, 2, 9, 1, 1, 4, 4]])

    def draw(seed, per_image):
        bank = nn_retrieval.MemoryBank(5, patches_per_image=per_image, seed=seed)
        return [bank.sample(valid[0]).tolist() for _ in range(3)]

    everything = [i for i, v in enumerate(valid[0].tolist()) if v > 0]
    assert draw(1, None) == [everything] * 3 and draw(1, 10) == [everything] * 3          # patches without a valid pixel never enter
    a, b, c = draw(1, 4), draw(1, 4), draw(2, 4)
    assert a == b and a != c
    assert all(len(s) == 4 and s == sorted(s) and set(s) <= set(everything) for s in a + c)
    assert a[0] != a[1] or a[1] != a[2]                                                   # one generator runs through the images
    with pytest.raises(ValueError):
        nn_retrieval.MemoryBank(5, patches_per_image=0)
    with pytest.raises(ValueError):
        nn_retrieval.MemoryBank(257)


def test_parser_surface_and_defaults():
    from timetuning_amd import linear_finetune

    args = nn_retrieval.build_parser().parse_args([])
    probe = linear_finetune.build_parser().parse_args([])
    for name in ("architecture", "model_path", "head_layers", "num_classes", "mask_size", "batch_size", "input_resolution", "dataset_path",
                 "num_train_images", "num_val_images", "png_decode"):
        assert getattr(args, name) == getattr(probe, name), name
    assert (args.k, args.beta, args.patches_per_image, args.bank_images, args.search_workspace_mb) == (30, 0.02, 0, 0, 64)
    assert args.select == nn_retrieval.DEFAULT_SELECT and args.select in ("hip", "torch") and args.dataset == "voc"
    args = nn_retrieval.build_parser().parse_args(["--dataset", "synthetic", "--k", "7", "--beta", "0.1", "--patches_per_image", "16", "--bank_images", "3",
                                                   "--search_workspace_mb", "16", "--select", "torch", "--png_decode", "device"])
    assert (args.dataset, args.k, args.beta, args.patches_per_image, args.bank_images, args.search_workspace_mb, args.select, args.png_decode) == \
        ("synthetic", 7, 0.1, 16, 3, 16, "torch", "device")
    for bad in (["--select", "eager"], ["--dataset", "davis"]):
        with pytest.raises(SystemExit):
            nn_retrieval.build_parser().parse_args(bad)


def test_shape_queries_without_a_gpu():
    if not _lib.os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert lib.tt_topk_merge_max_k() == 64 == hip_ops.NN_MAX_K
    ok = lib.tt_topk_merge_shape_ok
    assert ok(1, 1, 1, 1) and ok(130, 4097, 5000, 64) and ok(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 30)
    assert not ok(0, 5, 5, 5) and not ok(5, 0, 5, 5) and not ok(5, 5, 4, 5) and not ok(5, 5, 5, 0) and not ok(5, 5, 5, 65) and not ok(2 ** 31, 5, 5, 5)
    ok = lib.tt_patch_label_counts_shape_ok
    assert ok(1, 1, 1, 1) and ok(3, 448, 28, 256) and ok(60, 112, 28, 21)
    assert not ok(1, 30, 28, 21) and not ok(1, 28, 0, 21) and not ok(0, 28, 28, 21) and not ok(1, 28, 28, 257) and not ok(1, 28, 28, 0) and not ok(1, 14, 28, 21)
    ok = lib.tt_nn_label_aggregate_shape_ok
    assert ok(1, 1, 1, 1) and ok(10 ** 6, 30, 8 * 10 ** 6, 21) and ok(5, 64, 7, 256)
    assert not ok(0, 30, 7, 21) and not ok(5, 0, 7, 21) and not ok(5, 65, 7, 21) and not ok(5, 30, 0, 21) and not ok(5, 30, 7, 0)


@pytest.mark.parametrize("Q,N,ws,tile", [(130, 4000, 64 << 20, 4096), (130, 4000, 44 * 1334 * 4, 44), (130, 4000, 8 * 236 * 4, 8), (131, 4001, 4 * 997, 7),
                                         (5, 3, 4, 4096), (1, 1, 4, 1), (1000, 17, 4 * 100, 4096), (7, 100000, 4 * 12345, 3)])
def test_search_plan_covers_every_pair_once(Q, N, ws, tile):
    plan = hip_ops.nn_search_plan(Q, N, ws, tile)
    seen = np.zeros((Q, N), np.int32) if Q * N <= 1 << 22 else None
    area = 0
    for q0, q1, n0, n1 in plan:
        assert 0 <= q0 < q1 <= Q and 0 <= n0 < n1 <= N
        assert q1 - q0 <= tile and (q1 - q0) * (n1 - n0) * 4 <= ws
        area += (q1 - q0) * (n1 - n0)
        if seen is not None:
            seen[q0:q1, n0:n1] += 1
    assert area == Q * N and (seen is None or (seen == 1).all())
    firsts = {}
    for q0, q1, n0, n1 in plan:                                              # per query tile the bank runs front to back: block 0 first
        assert n0 == firsts.get(q0, 0)
        firsts[q0] = n1
    assert all(v == N for v in firsts.values())


def test_search_plan_block_counts_of_the_gpu_test():
    per_axis = lambda plan: (len({p[0] for p in plan}), len({p[2] for p in plan}))
    assert per_axis(hip_ops.nn_search_plan(130, 4000)) == (1, 1)
    assert per_axis(hip_ops.nn_search_plan(130, 4000, 44 * 1334 * 4, 44)) == (3, 3)
    assert per_axis(hip_ops.nn_search_plan(130, 4000, 8 * 236 * 4, 8)) == (17, 17)
    with pytest.raises(ValueError):
        hip_ops.nn_search_plan(130, 4000, 3)
    with pytest.raises(ValueError):
        hip_ops.nn_search_plan(0, 4000)
