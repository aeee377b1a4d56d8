"""N31 on the GPU: tt_topk_merge, tt_patch_label_counts and tt_nn_label_aggregate against the restatements of tests/_nn_ref.py, the tiled
search on both select routes and against fp64, self-retrieval, and DenseNNEvaluator end to end."""
import numpy as np
import pytest
import torch

import _nn_ref as R
from timetuning_amd import _lib, hip_ops, nn_retrieval, synth

pytestmark = pytest.mark.gpu
GUARD, VAL_SENTINEL, IDX_SENTINEL = 64, 777.0, 0x5A5A5A5A5A5A5A5A
BIG_BASE = 2 ** 31 - 1000          # the block's indices pass through 2^31
LINEAR_TOL = 2e-5                  # what tests/test_hip_ops.py holds linear_fwd to: max |y - ref| / max |ref|


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def stream():
    return torch.cuda.current_stream().cuda_stream


class Lists:
    """Running lists [Q, k] between guards of sentinels."""

    def __init__(self, Q, k):
        self.Q, self.k = Q, k
        self.vbuf = torch.full((Q * k + 2 * GUARD,), VAL_SENTINEL, dtype=torch.float32, device=dev())
        self.ibuf = torch.full((Q * k + 2 * GUARD,), IDX_SENTINEL, dtype=torch.int64, device=dev())
        self.vals = self.vbuf[GUARD:GUARD + Q * k].view(Q, k)
        self.idx = self.ibuf[GUARD:GUARD + Q * k].view(Q, k)

    def read(self):
        v, i = self.vbuf.cpu(), self.ibuf.cpu()
        for buf, s in ((v, VAL_SENTINEL), (i, IDX_SENTINEL)):
            assert (buf[:GUARD] == s).all() and (buf[-GUARD:] == s).all(), "a write outside the lists"
        return v[GUARD:-GUARD].view(self.Q, self.k).clone(), i[GUARD:-GUARD].view(self.Q, self.k).clone()

    def untouched(self):
        return bool((self.vbuf == VAL_SENTINEL).all()) and bool((self.ibuf == IDX_SENTINEL).all())


def place(sims: torch.Tensor, ld=None, offset=0):
    """sims (CPU) [Q, Nc] as a device view with rows ``ld`` floats apart, starting ``offset`` floats past a 16-byte boundary."""
    Q, Nc = sims.shape
    ld = Nc if ld is None else ld
    buf = torch.full((offset + Q * ld + 4,), float("nan"), dtype=torch.float32, device=dev())       # a NaN is never selected: the pitch must not be read as data
    view = buf[offset:offset + Q * ld].view(Q, ld)[:, :Nc]
    view.copy_(sims)
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view


def merge(lists: Lists, view, base, init):
    rc = _lib.load().tt_topk_merge(view.data_ptr(), view.shape[0], view.shape[1], view.stride(0), base, lists.vals.data_ptr(), lists.idx.data_ptr(),
                                   lists.k, 1 if init else 0, stream())
    assert rc == 0, _lib.load().tt_last_error()


def same(got, want, what=""):
    assert torch.equal(got[0], want[0]), what
    assert torch.equal(got[1], want[1]), what


@pytest.mark.parametrize("k", [1, 5, 30, 64])
def test_topk_merge_equals_the_restatement(k):
    g = torch.Generator().manual_seed(100 + k)
    case = 0
    for Q in (1, 3, 64, 65, 130):
        for Nc in (1, 63, 64, 65, 1000, 4097):
            sims = torch.randint(0, 8, (Q, Nc), generator=g).float()              # eight values: ties everywhere
            if case % 2:
                sims = sims + torch.rand((Q, Nc), generator=g)                     # ... and rows where they are rare
            ld, offset = (Nc, Nc + 3, Nc + 8)[case % 3], (0, 1, 3, 2)[case % 4]   # 4 and 12 bytes past a 16-byte boundary among them
            base = BIG_BASE if case % 2 == 0 or Nc == 4097 else 0
            if Nc == 4097:
                sims[0, 4000] = 100.0                                             # the best of query 0 lies beyond index 2^31
            lists = Lists(Q, k)
            merge(lists, place(sims, ld, offset), base, True)
            got = lists.read()
            same(got, R.select(sims, base + torch.arange(Nc), k), (Q, Nc, ld, offset))
            assert Nc != 4097 or int(got[1][0, 0]) == 2 ** 31 + 3000
            case += 1


def test_topk_merge_special_rows():
    k, Nc = 5, 200
    g = torch.Generator().manual_seed(7)
    sims = torch.randn((9, Nc), generator=g)
    sims[0, :] = 0.25                                                              # all equal: indices 0 .. k - 1
    sims[1, ::2] = float("nan")
    sims[1, 1::4] = float("-inf")
    sims[2, :] = float("nan")                                                      # only NaN: the list stays empty
    sims[3, :] = float("-inf")
    sims[3, 77] = float("nan")
    sims[4, :] = float("nan")
    sims[4, [5, 199, 64]] = torch.tensor([0.5, 0.5, -1.0])                         # three finite candidates for five places
    sims[5, :] = float("-inf")
    sims[5, 3] = float("inf")
    sims[6, 100:] = sims[6, :100]                                                  # every value twice
    sims[7, :] = -0.0
    sims[7, 150] = 0.0                                                             # -0 == +0: only the index orders them
    for offset in (0, 1, 3):
        lists = Lists(9, k)
        merge(lists, place(sims, Nc + 1, offset), BIG_BASE, True)
        got = lists.read()
        same(got, R.select(sims, BIG_BASE + torch.arange(Nc), k), offset)
        same(got, R.select_slow(sims, BIG_BASE + torch.arange(Nc), k), offset)
        assert got[1][0].tolist() == [BIG_BASE + j for j in range(k)]
        assert (got[1][2] == -1).all() and (got[0][2] == R.NEG_INF).all() and (got[1][3] == -1).all()
        assert got[1][4].tolist() == [BIG_BASE + 5, BIG_BASE + 199, BIG_BASE + 64, -1, -1]
        assert got[1][5].tolist() == [BIG_BASE + 3, -1, -1, -1, -1]
    # fewer than k columns in total, over two calls
    lists = Lists(2, 30)
    a, b = torch.randn((2, 7), generator=g), torch.randn((2, 9), generator=g)
    merge(lists, place(a), 0, True)
    merge(lists, place(b, 12, 1), 50, False)
    want = R.select(torch.cat([a, b], 1), torch.cat([torch.arange(7), 50 + torch.arange(9)]), 30)
    same(lists.read(), want)
    assert (want[1][:, 16:] == -1).all() and (want[1][:, :16] >= 0).all()


@pytest.mark.parametrize("k", [1, 30, 64])
def test_topk_merge_is_independent_of_the_cut_into_blocks(k):
    Q, N = 65, 300
    g = torch.Generator().manual_seed(11)
    sims = torch.randint(0, 8, (Q, N), generator=g).float()
    sims[:, 100:200] += torch.rand((Q, 100), generator=g)
    sims[5, 17] = float("nan")
    want = R.select(sims, BIG_BASE + torch.arange(N), k)
    whole = place(sims)
    results = []
    for width, backwards in ((N, False), (N, False), (64, False), (100, False), (1, False), (64, True), (100, True), (1, True)):
        lists = Lists(Q, k)
        starts = list(range(0, N, width))
        for j, n0 in enumerate(reversed(starts) if backwards else starts):
            merge(lists, whole[:, n0:n0 + width], BIG_BASE + n0, j == 0)           # column slices: pitched, misaligned wherever n0 % 4 != 0
        results.append(lists.read())
        same(results[-1], want, (width, backwards))
    same(results[0], results[1])                                                   # two calls on the same input


def test_topk_merge_refusals_write_nothing():
    lib = _lib.load()
    lists, view = Lists(3, 5), place(torch.zeros(3, 8))
    args = lambda **kw: [kw.get("sims", view.data_ptr()), kw.get("Q", 3), kw.get("Nc", 8), kw.get("ld", 8), kw.get("base", 0),
                         kw.get("vals", lists.vals.data_ptr()), kw.get("idx", lists.idx.data_ptr()), kw.get("k", 5), kw.get("init", 1), stream()]
    for bad in (dict(k=0), dict(k=65), dict(ld=7), dict(Q=0), dict(Nc=0), dict(base=-1), dict(init=2), dict(sims=None), dict(vals=None), dict(idx=None),
                dict(sims=view.data_ptr() + 2), dict(idx=lists.idx.data_ptr() + 4)):
        assert lib.tt_topk_merge(*args(**bad)) != 0, bad
        assert lib.tt_last_error()
    torch.cuda.synchronize()
    assert lists.untouched()
    with pytest.raises(ValueError):
        hip_ops.topk_merge(view, 0, k=65)
    with pytest.raises(ValueError):
        hip_ops.topk_merge(view.t(), 0, k=5)


# ---- tt_patch_label_counts ---------------------------------------------------------------------------------------------------------------

def raw_counts(maps: torch.Tensor, g, C, ignore, offset=0):
    M, Rr, _ = maps.shape
    buf = torch.full((offset + maps.numel() + 16,), 0xEE, dtype=torch.uint8, device=dev())
    buf[offset:offset + maps.numel()] = maps.flatten().to(dev())
    n = M * g * g
    out = torch.full((n * C + n + 2 * GUARD,), -77, dtype=torch.int32, device=dev())
    status = torch.full((3,), -77, dtype=torch.int32, device=dev())
    rc = _lib.load().tt_patch_label_counts(buf.data_ptr() + offset, M, Rr, g, C, -1 if ignore is None else ignore, out.data_ptr() + 4 * GUARD,
                                           out.data_ptr() + 4 * (GUARD + n * C), status.data_ptr() + 4, stream())
    host, st = out.cpu(), status.cpu()
    assert (host[:GUARD] == -77).all() and (host[-GUARD:] == -77).all() and st[0] == -77 and st[2] == -77
    return rc, host[GUARD:GUARD + n * C].view(M, g * g, C), host[GUARD + n * C:GUARD + n * C + n].view(M, g * g), int(st[1]), host


@pytest.mark.parametrize("g", [1, 2, 14, 28])
def test_patch_label_counts_equals_the_restatement(g):
    gen = torch.Generator().manual_seed(20 + g)
    case = 0
    for mult in (1, 2, 16):
        for C in (1, 21, 256):
            for M in (1, 3):
                Rr = g * mult
                maps = torch.randint(0, C, (M, Rr, Rr), generator=gen).to(torch.uint8)
                maps[torch.rand((M, Rr, Rr), generator=gen) < 0.1] = 255
                if mult > 1:
                    maps[0, :mult, :mult] = 255                                 # a cell without a valid pixel
                for ignore in (255, None):
                    if ignore is None and C < 256:
                        maps[maps == 255] = C - 1                               # without an ignore value 255 is a label like any other
                    rc, cnt, valid, status, _ = raw_counts(maps, g, C, ignore, offset=(0, 1, 3, 6)[case % 4])
                    want = R.counts(maps, g, C, ignore)
                    assert rc == 0 and status == -1 and want[2] == -1
                    assert (cnt == want[0]).all() and (valid == want[1]).all(), (g, Rr, C, M, ignore)
                    case += 1
                if mult > 1 and C == 21:
                    assert int(want[1].sum()) == M * Rr * Rr                    # (ignore None: every pixel is counted)


def test_patch_label_counts_reports_the_first_map_out_of_range():
    gen = torch.Generator().manual_seed(31)
    M, g, Rr, C = 4, 7, 28, 21
    maps = torch.randint(0, C, (M, Rr, Rr), generator=gen).to(torch.uint8)
    maps[3, 0, 0] = C
    maps[2, 27, 27] = 200
    maps[1, 5, 5] = 255
    rc, cnt, valid, status, _ = raw_counts(maps, g, C, 255, offset=1)
    want = R.counts(maps, g, C, 255)
    assert rc == 0 and status == 2 == want[2]
    assert (cnt == want[0]).all() and (valid == want[1]).all()                  # the labels out of range are counted nowhere
    with pytest.raises(ValueError, match="map 2 "):
        hip_ops.patch_label_counts(maps.to(dev()), g, C)
    with pytest.raises(ValueError, match="map 1 "):
        hip_ops.patch_label_counts(maps.to(dev()), g, C, ignore=None)
    c, v = hip_ops.patch_label_counts(maps[:2].to(dev()), g, C)
    assert (c.cpu() == want[0][:2]).all() and (v.cpu() == want[1][:2]).all()


def test_patch_label_counts_refusals_write_nothing():
    maps = torch.zeros((1, 30, 30), dtype=torch.uint8)
    for g, C, ignore in ((28, 21, 255), (0, 21, 255), (15, 0, 255), (15, 257, 255), (15, 21, 256), (15, 21, -2), (60, 21, 255)):
        rc, _, _, status, host = raw_counts(maps, g, C, ignore)                    # 30 % 28 != 0 first: refused before a launch
        assert rc != 0 and _lib.load().tt_last_error(), (g, C, ignore)
        assert status == -77 and (host == -77).all(), (g, C, ignore)
    with pytest.raises(ValueError):
        hip_ops.patch_label_counts(maps.to(dev()), 28, 21)


# ---- tt_nn_label_aggregate ---------------------------------------------------------------------------------------------------------------

AGG_ERRORS = {}


@pytest.mark.parametrize("beta", [0.02, 1.0])
@pytest.mark.parametrize("k", [1, 5, 30, 64])
def test_nn_label_aggregate_within_the_derived_bound(k, beta):
    """|out - fp64| <= (2 max_j |v_j - v_max| / beta + k + 4) 2^-24 per query: labels lie in [0, 1] and the weights sum to 1; the
    exponent's argument carries two roundings (the difference, the division), each of the k terms one more, the sum, the division by it
    and the expf a few.  The restatement divides by the fp32 value of beta, which is what the entry receives.  Measured on one MI355X:
    largest |error| 2.98e-7 (k = 64, beta = 1, C = 1), largest error / bound 0.23 (k = 5, beta = 1, C = 2)."""
    gen = torch.Generator().manual_seed(40 + k)
    Q, N = 70, 500
    beta32 = float(np.float32(beta))
    worst = 0.0
    for C in (1, 2, 21, 150, 256):
        labels = torch.rand((N, C), generator=gen) ** 4
        labels = (labels / labels.sum(1, keepdim=True)).float().clamp(0, 1)
        vals = torch.sort(torch.rand((Q, k), generator=gen) * 2 - 1, dim=1, descending=True).values.float()
        idx = torch.randint(0, N, (Q, k), generator=gen)
        for q in range(0, Q, 7):                                                   # lists with an empty tail
            idx[q, k - (q % k) - 1:] = -1
            vals[q, k - (q % k) - 1:] = R.NEG_INF
        idx[3, :], vals[3, :] = -1, R.NEG_INF                                      # no valid entry: a zero row
        out = torch.full((Q * C + 2 * GUARD,), VAL_SENTINEL, dtype=torch.float32, device=dev())
        got = hip_ops.nn_label_aggregate(vals.to(dev()), idx.to(dev()), labels.to(dev()), beta, out=out[GUARD:GUARD + Q * C].view(Q, C))
        host = out.cpu()
        assert (host[:GUARD] == VAL_SENTINEL).all() and (host[-GUARD:] == VAL_SENTINEL).all()
        want = R.aggregate(vals, idx, labels, beta32)
        ok = idx >= 0
        spread = torch.where(ok, vals[:, :1] - vals, torch.zeros_like(vals)).double().max(1).values
        bound = (2 * spread / beta32 + k + 4) * 2.0 ** -24
        err = (got.cpu().double() - want).abs().max(1).values
        worst = max(worst, float((err / bound).max()))
        AGG_ERRORS[(k, beta, C)] = float(err.max())
        print(f"nn_label_aggregate k={k} beta={beta} C={C}: max |error| {float(err.max()):.3e}, largest error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (k, beta, C, float((err / bound).max()))
        assert (got[3] == 0).all() and (want[3] == 0).all()
    assert worst <= 1.0


# ---- nn_search -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def search_data():
    out = {}
    for D in (64, 384):
        q = torch.from_numpy(synth.normal(f"nn.q{D}", (130, D), 1.0)).float()
        b = torch.from_numpy(synth.normal(f"nn.b{D}", (4000, D), 1.0)).float()
        q, b = torch.nn.functional.normalize(q, dim=1), torch.nn.functional.normalize(b, dim=1)
        out[D] = (q, b, q.double() @ b.double().t())
    return out


@pytest.mark.parametrize("D", [64, 384])
def test_nn_search_hip_equals_torch_and_agrees_with_fp64(search_data, D):
    q, b, S = search_data[D]
    Q, N, k = 130, 4000, 30
    qd, bd = q.to(dev()), b.to(dev())
    bound = LINEAR_TOL * float(S.abs().max())
    kth = torch.sort(S, dim=1, descending=True).values[:, k - 1]
    for ws, tile, blocks in ((64 << 20, 4096, 1), (44 * 1334 * 4, 44, 3), (8 * 236 * 4, 8, 17)):
        plan = hip_ops.nn_search_plan(Q, N, ws, tile)
        assert len({p[0] for p in plan}) == blocks and len({p[2] for p in plan}) == blocks
        hv, hi = hip_ops.nn_search(qd, bd, k, ws, select="hip", query_tile=tile)
        tv, ti = hip_ops.nn_search(qd, bd, k, ws, select="torch", query_tile=tile)
        assert torch.equal(hv, tv) and torch.equal(hi, ti), (D, blocks)
        hv, hi = hv.cpu(), hi.cpu()
        assert (hi >= 0).all() and (hi < N).all() and (hv[:, :-1] >= hv[:, 1:]).all()
        assert all(len(set(row)) == k for row in hi.tolist())
        at = torch.gather(S, 1, hi)
        print(f"nn_search D={D} blocks={blocks}: max |vals - fp64| {float((hv.double() - at).abs().max()):.3e} (bound {bound:.3e})")
        assert ((hv.double() - at).abs() <= bound).all()
        assert (hv[:, k - 1].double() >= kth - bound).all()
    # (the blocks of different sizes may run different GEMM tiles, so the lists of different plans are not compared bit for bit)


def test_self_retrieval():
    n, D, C = 500, 64, 6
    x = torch.nn.functional.normalize(torch.from_numpy(synth.normal("nn.self", (n, D), 1.0)).float(), dim=1)
    off = (x.double() @ x.double().t()).fill_diagonal_(-1).max()
    assert float(off) < 0.6                                                        # no second vector close to a query
    gen = torch.Generator().manual_seed(50)
    labels = torch.rand((n, C), generator=gen)
    labels = (labels / labels.sum(1, keepdim=True)).float()
    xd, ld = x.to(dev()), labels.to(dev())
    for ws, tile in ((64 << 20, 4096), (4 * 64 * 100, 64)):
        vals, idx = hip_ops.nn_search(xd, xd, 1, ws, query_tile=tile)
        assert torch.equal(idx.cpu().flatten(), torch.arange(n))
        assert torch.equal(hip_ops.nn_label_aggregate(vals, idx, ld, 0.02), ld)  # one neighbour: weight 1, the row itself


# ---- end to end --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny():
    from timetuning_amd.linear_finetune import synthetic_segmentation
    from timetuning_amd.models import FeatureExtractor

    fe = FeatureExtractor("dino-s16", "", [], vit_cfg=synth.ARCHS["tiny-s16"], return_attention=False).to(dev()).eval()
    C = 5
    x_tr, y_tr = synthetic_segmentation(8, 64, C, seed=1)
    x_va, y_va = synthetic_segmentation(4, 64, C, seed=2)
    return fe, C, (x_tr, y_tr), (x_va, y_va)


@pytest.mark.parametrize("k", [1, 7])
def test_evaluator_end_to_end(tiny, k):
    from timetuning_amd.metrics import PredsmIoU

    fe, C, (x_tr, y_tr), (x_va, y_va) = tiny
    ev = nn_retrieval.DenseNNEvaluator(fe, C, k=k, beta=0.02, mask_size=32)
    bank = ev.fit([(x_tr[:5], y_tr[:5]), (x_tr[5:], y_tr[5:])])
    feats_bank, labels_bank = bank.finalize()
    # the bank: every patch with a valid pixel, its distribution counts / valid of the 32 x 32 nearest-resized mask
    masks = nn_retrieval.prepare_masks(y_tr, 32)
    cnt, valid, _ = R.counts(masks, 4, C, 255)
    keep = valid.flatten() > 0
    assert feats_bank.shape == (int(keep.sum()), 128) and len(bank) == int(keep.sum())
    assert torch.equal(labels_bank.cpu(), (cnt.view(-1, C)[keep].float() / valid.view(-1, 1)[keep].float()))
    assert torch.allclose(feats_bank.norm(dim=1).cpu(), torch.ones(len(bank)), atol=1e-5)
    # predict against the restatement, fed the device's features and similarities
    xd = x_va.to(dev())
    got = ev.predict(xd)
    feats = ev.features(xd)
    queries = hip_ops.l2norm_fwd(feats.view(-1, feats.shape[-1]))
    sims = hip_ops.linear_fwd(queries, feats_bank)
    want = R.predict(sims.cpu(), labels_bank.cpu(), 4, k, float(np.float32(0.02)), 32)
    assert got.shape == (4, 32, 32) and got.dtype == torch.int64
    assert torch.equal(got.cpu(), want)
    assert len(torch.unique(want)) > 1
    # evaluate: the mIoU PredsmIoU gives for those maps
    gt = torch.nn.functional.interpolate((y_va * 255).float(), size=(32, 32), mode="nearest").squeeze(1)
    ok = gt != 255
    metric = PredsmIoU(C, C, involve_bg=True)
    metric.update(gt[ok].flatten().to(dev()), want.to(dev())[ok.to(dev())].flatten())
    value = ev.evaluate([(x_va[:3], y_va[:3]), (x_va[3:], y_va[3:])])
    assert value == metric.compute(True, linear_probe=True)[0]
    assert 0.0 <= value <= 1.0


def test_main_runs_on_synthetic_data():
    from timetuning_amd.linear_finetune import _batches, synthetic_segmentation
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    argv = ["--dataset", "synthetic", "--model_path", "", "--input_resolution", "64", "--mask_size", "32", "--batch_size", "3", "--num_classes", "5",
            "--num_train_images", "8", "--num_val_images", "4", "--num_prototypes", "10", "--head_layers", "64", "32", "--k", "7",
            "--patches_per_image", "12", "--bank_images", "7", "--search_workspace_mb", "1"]
    value = nn_retrieval.main(argv)
    assert np.isfinite(value) and 0.0 <= value <= 1.0
    # the same run by hand
    model = TimeT(FeatureExtractor("dino-s16", "", [64, 32], return_attention=False), 10).to(dev())
    ev = nn_retrieval.DenseNNEvaluator(model, 5, k=7, beta=0.02, mask_size=32, patches_per_image=12, seed=1, search_workspace_bytes=1 << 20)
    x_tr, y_tr = synthetic_segmentation(8, 64, 5, seed=1)
    x_va, y_va = synthetic_segmentation(4, 64, 5, seed=2)
    ev.fit(_batches(x_tr, y_tr, 3), max_images=7)
    assert len(ev.bank) == 7 * 12
    assert ev.evaluate(_batches(x_va, y_va, 3)) == value
    assert nn_retrieval.main(argv + ["--select", "torch"]) == value


# ---- launch hygiene ------------------------------------------------------------------------------------------------------------------------

def test_launch_neither_allocates_nor_breaks_capture():
    lib = _lib.load()
    gen = torch.Generator().manual_seed(60)
    Q, Nc, k, N, C, M, g, Rr = 70, 333, 30, 400, 21, 3, 14, 28
    sims = torch.rand((Q, Nc), generator=gen)
    labels = torch.rand((N, C), generator=gen)
    labels = (labels / labels.sum(1, keepdim=True)).float()
    maps = torch.randint(0, C, (M, Rr, Rr), generator=gen).to(torch.uint8)
    want_lists = R.select(sims, 10 + torch.arange(Nc), k)
    want_counts = R.counts(maps, g, C, 255)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        sd, ld, md = place(sims, Nc + 1, 1), labels.to(dev()), maps.to(dev())
        vals = torch.empty((Q, k), dtype=torch.float32, device=dev())
        idx = torch.empty((Q, k), dtype=torch.int64, device=dev())
        out = torch.empty((Q, C), dtype=torch.float32, device=dev())
        cnt = torch.empty((M, g * g, C), dtype=torch.int32, device=dev())
        valid = torch.empty((M, g * g), dtype=torch.int32, device=dev())
        status = torch.empty((1,), dtype=torch.int32, device=dev())
        outputs = (vals, idx, out, cnt, valid, status)

        def launch():
            s = torch.cuda.current_stream().cuda_stream
            assert lib.tt_topk_merge(sd.data_ptr(), Q, Nc, sd.stride(0), 10, vals.data_ptr(), idx.data_ptr(), k, 1, s) == 0
            assert lib.tt_nn_label_aggregate(vals.data_ptr(), idx.data_ptr(), ld.data_ptr(), Q, k, N, C, 0.02, out.data_ptr(), s) == 0
            assert lib.tt_patch_label_counts(md.data_ptr(), M, Rr, g, C, 255, cnt.data_ptr(), valid.data_ptr(), status.data_ptr(), s) == 0

        def check():
            torch.cuda.synchronize()
            assert torch.equal(vals.cpu(), want_lists[0]) and torch.equal(idx.cpu(), want_lists[1])
            assert (cnt.cpu() == want_counts[0]).all() and (valid.cpu() == want_counts[1]).all() and int(status.item()) == -1
            agg = R.aggregate(want_lists[0], want_lists[1], labels, float(np.float32(0.02)))
            assert float((out.cpu().double() - agg).abs().max()) < 1e-5

        launch()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(3):
            for t in outputs:
                t.fill_(7)
            launch()
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0, "a launch changed the device's free memory"
        check()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            launch()
        for _ in range(2):
            for t in outputs:
                t.fill_(7)
            graph.replay()
            check()
