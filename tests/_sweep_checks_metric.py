"""The checks of the sweep's fifth tier (tests/_sweep_cases.py, METRIC_OPS): the tiled k-means pair, the batched assignment and the fused
batched fit (kmeans.hip, kmeans_fit.hip), the segmented confusion counts (confusion.hip), the DAVIS J&F counts (davis.hip) and the
boundary-F counts (bfscore.hip).

One check per op, written once and run on two sides, as tests/_sweep_checks_eval.py: ``MetricTwin`` (tests/test_sweep_metric_host.py, no
GPU) and ``MetricHip`` (tests/test_hip_sweep.py).
  k-means   MetricTwin is the plain-C twins tt_cpu_kmeans_assign / tt_cpu_kmeans_accumulate (tile_k ignored, problems looped over, the fit
            a Python Lloyd loop over the two with c = float32(sum / count)).  Assignments are held to fp64 by the second tier's rules
            (TOL_KM on distances, a label may differ only under KM_GAP, capped by EXCUSE_SHARE / EXCUSE_MIN_POINTS), sums to TOL_KM, counts
            exactly; the fit to oracle.timet_oracle.kmeans_lloyd (objectives and centroids within 1e-4: the bounds of
            tests/test_hip_kmeans_fit.py) on inputs that ``fit_reference`` proves valid on BOTH sides - no empty cluster and no assignment
            within KM_GAP of a tie in any iteration of the fp64 run, so that an fp32 trajectory cannot legitimately leave the fp64 one.
            Inputs are valid by construction (``km_conditioned``, the redraw loop of ``check_kmeans_fit``): no draw of the generators
            fails for what it holds, whatever the kernels do (tests/test_sweep_metric_host.py runs hundreds of draws per op).
            On the HIP side, additionally, the bit equalities of include/timetuning_hip.h's k-means contract.
  counters  exact equality with the NumPy restatements of tests/_metric_refs.py.  They have no C twin: MetricTwin is instead a direct
            per-pixel (per-element) definition written out below with explicit loops over the structuring element and no helper shared with
            the restatement, run on every case of at most SMALL_PIXELS pixels - the host half thereby proves the restatement, and that no
            count column is zero over all of an op's cases (tests/test_sweep_metric_host.py)."""
from __future__ import annotations

import numpy as np
import torch

import _border_follow as bfl
import _metric_refs as R
from _sweep_cases import KM_MAX_GRID_Y, case_id, km_accumulate_blocks, km_tile
from _sweep_checks_eval import KM_GAP, TOL_KM, _excuse_cap, _normal, case_rng, f32, f64, km_inputs, km_reference, make_note, rel_err, twin_side

TOL_FIT = 1e-4             # objectives (relative) and centroids (max-normalised): tests/test_hip_kmeans_fit.py::test_fused_fit_against_the_fp64_oracle
FIT_LONG_RUN = 128         # points per accumulation block above which nobody had measured the fit's error: there the bound is 4 x the twin's
FIT_DRAWS = 8              # draws of a fit case's blobs until fit_reference proves them valid
SMALL_PIXELS = 64 * 64     # the direct definitions run on cases of at most this many pixels (elements) per map
COMPARED: dict = {}        # op -> {case id: whether the side returned counts that were compared (the host side: the definition ran)}
COLUMNS: dict = {}         # op -> {case id: per-column sums of the expected counts}: every column must be non-zero somewhere


# ---- the two sides ---------------------------------------------------------------------------------------------------------------------------

class MetricTwin:
    name = "twin"

    def __init__(self):
        self.t = twin_side()

    def kmeans_assign_tiled(self, x, c, tile_k):
        return self.t.kmeans_assign(x, c)

    def kmeans_accumulate_tiled(self, x, labels, k, tile_k):
        return self.t.kmeans_accumulate(x, labels, k)

    def kmeans_assign_batched(self, x, c):
        out = [self.t.kmeans_assign(x[b], c[b]) for b in range(x.shape[0])]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    def kmeans_fit(self, x, init, niter, offset=0):
        """clustering.Kmeans._iterate on the twins, stopped where the fused fit stops: at the first empty cluster."""
        B, n, d = x.shape
        nredo, k = init.shape
        cent, obj, status = np.zeros((B, nredo, k, d), f32), np.zeros((B, nredo), f64), np.zeros((B, nredo), np.int32)
        for b in range(B):
            xb = np.ascontiguousarray(x[b])
            for r in range(nredo):
                c = xb[init[r]].copy()
                for it in range(niter):
                    labels, dist2 = self.t.kmeans_assign(xb, c)
                    sums, counts = self.t.kmeans_accumulate(xb, labels, k)
                    if (counts == 0).any():
                        status[b, r] = it + 1
                        break
                    obj[b, r] = dist2.astype(f64).sum()
                    c = (sums / counts[:, None].astype(f64)).astype(f32)
                cent[b, r] = c
        return cent, obj, status

    def confusion_segments(self, pred, gt, Cg, Cp, ignore, offset):
        return confusion_direct(pred, gt, Cg, Cp, ignore) if pred.size <= SMALL_PIXELS else None

    def davis_counts(self, pred, gt, O, element, void):
        return davis_direct(pred, gt, O, element, void) if pred[0].size <= SMALL_PIXELS else None

    def bf_counts(self, gt, pr, t):
        return bf_direct(gt, pr, t) if gt[0].size <= SMALL_PIXELS else None


class MetricHip:
    """The HIP library through timetuning_amd.hip_ops on cuda:0 (NumPy in, NumPy out), with the contract's bit equalities asserted on the way."""
    name = "hip"

    def __init__(self):
        from timetuning_amd import _lib, hip_ops

        self.ops, self._lib = hip_ops, _lib

    @staticmethod
    def _d(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    @staticmethod
    def _off(a, offset):
        """``a`` on the device as a view that starts ``offset`` elements into its storage."""
        flat = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
        buf = torch.empty(flat.numel() + offset, dtype=flat.dtype, device="cuda")
        buf[offset:].copy_(flat)
        v = buf[offset:].view(a.shape)
        assert v.data_ptr() == buf.data_ptr() + offset * flat.element_size() and buf.data_ptr() % 256 == 0
        return v

    def _chunked_resident(self, xd, cd):
        """tests/test_hip_kmeans_tiled.py::test_beyond_the_limit_assignment...: resident calls on centroid chunks in index order, strict <."""
        d, k = xd.shape[1], cd.shape[0]
        m = largest_resident_k(self.ops, d)
        best = torch.full((xd.shape[0],), float("inf"), device="cuda")
        besti = torch.zeros(xd.shape[0], dtype=torch.int32, device="cuda")
        for a in range(0, k, m):
            lab, dist = self.ops.kmeans_assign(xd, cd[a:a + m].contiguous(), return_dist=True)
            upd = dist < best
            best, besti = torch.where(upd, dist, best), torch.where(upd, lab + a, besti)
        return besti, best

    def kmeans_assign_tiled(self, x, c, tile_k):
        P, d = x.shape
        k = c.shape[0]
        xd, cd = self._d(x), self._d(c)
        labels = torch.full((P,), -1, dtype=torch.int32, device="cuda")          # (a point the launch leaves unwritten is seen)
        dist2 = torch.full((P,), -1.0, dtype=torch.float32, device="cuda")
        self._lib.check(self._lib.load().tt_kmeans_assign_tiled(xd.data_ptr(), cd.data_ptr(), labels.data_ptr(), dist2.data_ptr(), P, d, k, int(tile_k),
                                                                torch.cuda.current_stream().cuda_stream), "tt_kmeans_assign_tiled")
        assert torch.equal(self.ops.kmeans_assign_tiled(xd, cd, tile_k=tile_k), labels)          # the wrapper, without distances
        if self.ops.kmeans_shape_ok(d, k):
            l2, d2 = self.ops.kmeans_assign(xd, cd, return_dist=True)
        else:
            l2, d2 = self._chunked_resident(xd, cd)
        assert torch.equal(labels, l2) and torch.equal(dist2, d2), ("tiled vs resident bits", int((labels != l2).sum()), int((dist2 != d2).sum()))
        return labels.cpu().numpy(), dist2.cpu().numpy()

    def kmeans_accumulate_tiled(self, x, labels, k, tile_k):
        xd, ld = self._d(x), self._d(labels)
        sums, counts = self.ops.kmeans_accumulate_tiled(xd, ld, k, tile_k=tile_k)
        s2, c2 = self.ops.kmeans_accumulate_tiled(xd, ld, k, tile_k=tile_k)
        assert torch.equal(s2, sums) and torch.equal(c2, counts)                  # deterministic: fixed summation order, no float atomics
        if self.ops.kmeans_shape_ok(x.shape[1], k):
            s1, c1 = self.ops.kmeans_accumulate(xd, ld, k)
            assert torch.equal(s1, sums) and torch.equal(c1, counts), ("tiled vs resident bits", int((s1 != sums).sum()))
        return sums.cpu().numpy(), counts.cpu().numpy()

    def kmeans_assign_batched(self, x, c):
        B = x.shape[0]
        xd, cd = self._d(x), self._d(c)
        labels, dist2 = self.ops.kmeans_assign_batched(xd, cd, return_dist=True)
        assert torch.equal(self.ops.kmeans_assign_batched(xd, cd), labels)
        for b in sample_problems(B):      # tt_kmeans_assign is the same kernel at one problem: this holds the problems' offsets
            l1, d1 = self.ops.kmeans_assign(xd[b], cd[b], return_dist=True)
            assert torch.equal(labels[b], l1) and torch.equal(dist2[b], d1), b
        return labels.cpu().numpy(), dist2.cpu().numpy()

    def _fit_raw(self, x, init, niter, offset):
        xd = self._off(x, offset)
        assert xd.data_ptr() % 16 == (4 * offset) % 16
        cent, obj, status = self.ops.kmeans_fit_batched(xd, torch.from_numpy(init.astype(np.int32)), niter)
        return cent, obj, status

    def kmeans_fit(self, x, init, niter, offset=0):
        cent, obj, status = self._fit_raw(x, init, niter, offset)
        if offset:      # the unaligned fallback (VEC 1) returns the bits of the aligned run
            c0, o0, s0 = self._fit_raw(x, init, niter, 0)
            assert torch.equal(cent, c0) and torch.equal(obj, o0) and torch.equal(status, s0), "offset = 1 differs from the aligned run"
        return cent.cpu().numpy(), obj.cpu().numpy(), status.cpu().numpy()

    def fit_loop(self, xb, idx, niter):
        """One redo of clustering.Kmeans' loop over tt_kmeans_assign / tt_kmeans_accumulate from the same seeds -> (centroids, objective, splits)."""
        from timetuning_amd.clustering import Kmeans

        km = Kmeans(xb.shape[1], len(idx), niter=niter, nredo=1, seed=1, max_points_per_centroid=10 ** 6)      # no subsampling: idx indexes xb itself
        splits = []
        split = km._split_empty
        km._split_empty = lambda cent, counts, n: splits.append(split(cent, counts, n))
        km.train(self._d(xb), init_indices=[idx])
        return km.centroids, km.obj[0], splits

    def confusion_segments(self, pred, gt, Cg, Cp, ignore, offset):
        pd, gd = self._off(pred, offset), self._off(gt, offset % 2)
        got = self.ops.confusion_counts_segments(pd, gd, Cg, Cp, ignore)
        assert got.dtype == torch.int64 and torch.equal(got, self.ops.confusion_counts_segments(pd, gd, Cg, Cp, ignore))
        return got.cpu().numpy()

    def davis_counts(self, pred, gt, O, element, void):
        got = self.ops.davis_jf_counts(self._d(pred), self._d(gt), O, element, None if void is None else self._d(void))
        assert got.dtype == torch.int64
        return got.cpu().numpy()

    def bf_counts(self, gt, pr, t):
        got = self.ops.bf_counts(self._d(gt), self._d(pr), t)
        assert got.dtype == torch.int64
        return got.cpu().numpy()


def largest_resident_k(ops, d):
    """The largest k the resident pair takes at d columns (hip_ops.kmeans_shape_ok)."""
    m = 16384 // d
    while not ops.kmeans_shape_ok(d, m):
        m -= 1
    return m


def sample_problems(B):
    """Every problem of a small batch; of a large one the first, the last and those either side of a launch boundary (65 535 per launch)."""
    if B <= 8:
        return list(range(B))
    return sorted({0, 1, B - 1} | {b for b in (KM_MAX_GRID_Y - 1, KM_MAX_GRID_Y, KM_MAX_GRID_Y + 1) if b < B})


# ---- the assignments ------------------------------------------------------------------------------------------------------------------------------

def km_conditioned(x, c, pair, keep):
    """The fp64 reference of tests/_sweep_checks_eval.py (arg-min, least and second-least squared distance) on inputs made valid by
    construction.  The excuse rule lets a label differ only within KM_GAP of a tie, on at most ``keep`` = EXCUSE_SHARE of a case's points
    and on none under EXCUSE_MIN_POINTS; points generated as the second tier generates them fall within fp32 rounding of a tie at a rate
    that grows with k and d (measured on the twin: about 1e-4 at d = 128, k = 160), so a draw can hold more of them than the rule allows
    whatever the code under test does.  The points within KM_GAP of a tie in fp64 are therefore found here and all but the first ``keep``
    of them are overwritten IN ``x`` by copies of points that are clear of one.  A duplicated centroid ``pair`` is an exact tie by
    definition, not a near one: the reference is taken without the higher row (moved far away), so it names the lower index and measures
    the gap to the nearest OTHER centroid.  -> want, best, second, points replaced"""
    cref = c
    if pair is not None:
        cref = c.copy()
        cref[pair[1]] += f32(1e3)
    want, best, second = km_reference(x, cref)
    near = np.flatnonzero(second - best < KM_GAP * best)[keep:]
    if near.size:
        ok = np.ones(len(x), bool)
        ok[near] = False
        ok &= second - best >= KM_GAP * best
        clear = np.flatnonzero(ok)
        assert clear.size, "invalid inputs: every point lies within KM_GAP of a tie"
        src = clear[np.arange(near.size) % clear.size]
        x[near], want[near], best[near], second[near] = x[src], want[src], best[src], second[src]
    return want, best, second, int(near.size)


def _check_assignment(side_name, labels, dist2, x, c, pair, ref, note):
    """tests/_sweep_checks_eval.py::check_kmeans_assign's rules on one problem's labels and distances against ``ref`` = (want, best, second)."""
    k = c.shape[0]
    assert labels.min() >= 0 and labels.max() < k, "a point was left unwritten or labelled outside [0, k)"
    want, best, second = ref
    mism = labels != want
    assert (second[mism] - best[mism] < KM_GAP * best[mism]).all(), "a label differs from the fp64 arg-min away from a near-tie"
    note("dist2 max", rel_err(dist2, best), TOL_KM)
    if side_name != "twin":      # the twin sums in the kernel's order: away from near-ties its labels are the kernel's
        clear = second - best >= KM_GAP * best
        assert np.array_equal(labels[clear], twin_side().kmeans_assign(x, c)[0][clear])
    if pair is not None:         # the deliberate tie, exactly: equal distances, the lower index wins
        assert not (labels == pair[1]).any(), "the higher index of a duplicated centroid was chosen"
        assert (labels[want == pair[0]] == pair[0]).all()
    return int(mism.sum())


def check_kmeans_assign_tiled(side, p, rng, note):
    P, d, k, dup = p["P"], p["d"], p["k"], p["dup"]
    x, c, pair = km_inputs(rng, P, d, k, 0)
    if k > P:         # (more centroids than points to take them from: rows repeat, and equal rows are exact ties - only the planted pair may be one)
        c = (c + f32(0.05) * _normal(rng, k, d)).astype(f32)
    if dup == 1 and k > 1:
        lo = int(rng.integers(0, k - 1))
        pair = (lo, int(rng.integers(lo + 1, k)))
    elif dup == 2:    # the same centroid as the last row of the first tile and the first row of the second
        tile = km_tile(d, p["tile_k"])
        assert tile < k, "dup = 2 needs more than one tile"
        pair = (tile - 1, tile)
    if pair is not None:
        c[pair[1]] = c[pair[0]]
    want, best, second, replaced = km_conditioned(x, c, pair, _excuse_cap(P))
    if pair is not None:      # point 0 sits ON the duplicated centroid: both rows are at distance exactly 0 from it, in fp32 as in fp64
        x[0] = c[pair[0]]
        others = np.delete(c.astype(f64), list(pair), axis=0)
        want[0], best[0] = pair[0], 0.0
        second[0] = ((others - c[pair[0]].astype(f64)) ** 2).sum(1).min() if len(others) else np.inf
        assert second[0] > 0
    labels, dist2 = side.kmeans_assign_tiled(x, c, p["tile_k"])
    if pair is not None:
        assert labels[0] == pair[0] and dist2[0] == 0, "the point on the duplicated centroid did not take the lower index at distance 0"
    note("near-tie points replaced / points", replaced / P, 0.5)
    note("labels excused / allowed", _check_assignment(side.name, labels, dist2, x, c, pair, (want, best, second), note), _excuse_cap(P), strict=True)


def check_kmeans_assign_batched(side, p, rng, note):
    B, N, d, k = p["B"], p["N"], p["d"], p["k"]
    x = _normal(rng, B, N, d)
    # (distinct rows where the problem has them: equal centroids are an exact tie, which the tiled cases plant deliberately)
    rows = np.argsort(rng.random((B, N)), axis=1)[:, :k] if k <= N else rng.integers(0, N, (B, k))
    c = (0.5 * x[np.arange(B)[:, None], rows] + (f32(0.05) * _normal(rng, B, k, d) if k > N else f32(0))).astype(f32)
    cap = _excuse_cap(B * N)
    if B * N * k * d <= 1 << 22:      # every problem at once: the differences themselves, in fp64
        d2 = ((x.astype(f64)[:, :, None, :] - c.astype(f64)[:, None, :, :]) ** 2).sum(-1)
        want = d2.argmin(-1)
        best = np.take_along_axis(d2, want[..., None], -1)[..., 0]
        second = np.partition(d2, 1, axis=-1)[..., 1] if k > 1 else np.full_like(best, np.inf)
        refs = None
        for b in np.unique(np.argwhere(second - best < KM_GAP * best)[cap:, 0]):      # (km_conditioned, on the problems that need it)
            want[b], best[b], second[b], _ = km_conditioned(x[b], c[b], None, 0)
    else:
        refs = [km_conditioned(x[b], c[b], None, cap // B) for b in range(B)]
    labels, dist2 = side.kmeans_assign_batched(x, c)
    assert labels.shape == (B, N) and dist2.shape == (B, N)
    if refs is None:
        assert labels.min() >= 0 and labels.max() < k
        mism = labels != want
        assert (second[mism] - best[mism] < KM_GAP * best[mism]).all(), "a label differs from the fp64 arg-min away from a near-tie"
        note("dist2 max", rel_err(dist2, best), TOL_KM)
        excused = int(mism.sum())
    else:
        excused = sum(_check_assignment(side.name, labels[b], dist2[b], x[b], c[b], None, refs[b][:3], note) for b in range(B))
    note("labels excused / allowed", excused, cap, strict=True)


# ---- the tiled accumulation -----------------------------------------------------------------------------------------------------------------------

def check_kmeans_accumulate_tiled(side, p, rng, note):
    P, d, k, mode = p["P"], p["d"], p["k"], p["mode"]
    x = (_normal(rng, P, d) + f32(0.5)).astype(f32)
    labels = rng.integers(0, k, P).astype(np.int32)
    if mode == "one":
        labels[:] = k // 2
    elif mode == "skip" and k > 1:
        skip = int(rng.integers(0, k))
        labels[labels == skip] = (skip + 1) % k
    if k > 1 and mode != "one":
        labels[-1] = k - 1           # the last cluster - the last tile, whatever its size - is never empty
    sums, counts = side.kmeans_accumulate_tiled(x, labels, k, p["tile_k"])
    want_counts = np.bincount(labels, minlength=k)
    assert np.array_equal(counts, want_counts)
    want = np.zeros((k, d), f64)
    for t in range(d):     # column by column: no P x d fp64 temporary
        want[:, t] = np.bincount(labels, weights=x[:, t].astype(f64), minlength=k)
    note("sums max", rel_err(sums, want), TOL_KM)
    assert (sums[want_counts == 0] == 0).all()          # an empty cluster has an exactly zero sum
    # ... and cluster by cluster, so that one dropped cluster (tile) cannot hide behind the largest sum of the case.  A block adds at most
    # ppb values to an fp32 sum whose magnitude never exceeds (its points of the cluster) x max|x|; each addition rounds by at most 2^-24
    # of that, so over the blocks |error| <= ppb x 2^-24 x count x max|x| (the fp64 fold adds nothing at this scale)
    live = want_counts > 0
    scale = float(np.abs(x).max()) * want_counts[live, None]
    note("sums per cluster / (count x max|x|)", float((np.abs(sums - want)[live] / scale).max()), km_accumulate_blocks(P)[1] * 2.0 ** -24)


# ---- the fused fit --------------------------------------------------------------------------------------------------------------------------------

def fit_inputs(rng, p):
    """B problems of n points in k Gaussian blobs (point q in blob q % k, centres N(0, sep^2) per column) and nredo rows of k seeds, one in
    every blob, as tests/test_hip_kmeans_fit.py; ``empty``: that file's flagged construction on problem 1, redo 0."""
    B, n, d, k, nredo = p["B"], p["n"], p["d"], p["k"], p["nredo"]
    centres = rng.standard_normal((B, k, d)) * p["sep"]
    x = (centres[:, np.arange(n) % k] + rng.standard_normal((B, n, d))).astype(f32)
    init = np.stack([(r * k + np.arange(k)) % n for r in range(nredo)]).astype(np.int64)
    flagged = set()
    if p["empty"]:
        x[1, n // 2:] = x[1, :n // 2]
        init[0, :2] = (0, n // 2)      # clusters 0 and 1 seeded on the two copies of one point: the strict < leaves cluster 1 empty
        flagged.add((1, 0))
    return x, init, flagged


class InvalidFitInputs(AssertionError):
    """fit_reference: the fp64 run meets an empty cluster or a near-tie on these inputs."""


def fit_reference(x, init, niter, flagged):
    """oracle.timet_oracle.kmeans_lloyd per (problem, redo) -> centroids [B, nredo, k, d], objectives [B, nredo], and the proof that the
    inputs are valid: the same fp64 iteration is traced here, and in EVERY iteration no cluster is empty and every point's best and
    second-best distance are more than KM_GAP (relative) apart.  The trace must end where the oracle ends."""
    from oracle import timet_oracle as O

    B, n, d = x.shape
    nredo, k = init.shape
    cents, objs = np.zeros((B, nredo, k, d)), np.zeros((B, nredo))
    min_gap = np.inf
    for b in range(B):
        x64 = x[b].astype(f64)
        for r in range(nredo):
            if (b, r) in flagged:
                continue
            cent = x64[init[r]].copy()
            for it in range(niter):
                d2 = ((x64[:, None, :] - cent[None, :, :]) ** 2).sum(-1)
                lab = d2.argmin(1)
                if len(np.unique(lab)) != k:
                    raise InvalidFitInputs(f"invalid inputs: an empty cluster in problem {b}, redo {r}, iteration {it}")
                if k > 1:
                    two = np.partition(d2, 1, axis=1)[:, :2]
                    gap = two[:, 1] - two[:, 0]
                    if not (gap > KM_GAP * two[:, 0]).all():
                        raise InvalidFitInputs(f"invalid inputs: a near-tie in problem {b}, redo {r}, iteration {it}")
                    with np.errstate(divide="ignore", invalid="ignore"):
                        min_gap = min(min_gap, float(np.where(two[:, 0] > 0, gap / two[:, 0], np.inf).min()))
                obj = d2[np.arange(n), lab].sum()
                for j in range(k):
                    cent[j] = x64[lab == j].mean(0)
            if b < 4 or b >= B - 2:      # (the trace restates the oracle: held to it on the first and the last problems of a batch)
                oc, ol, oo = O.kmeans_lloyd(x[b], init[r], niter)
                assert np.array_equal(oc, cent) and np.array_equal(ol, lab) and oo == obj
            cents[b, r], objs[b, r] = cent, obj
    return cents, objs, min_gap


def _fit_errors(cent, obj, cents64, objs64, ok):
    eo = max(abs(obj[b, r] - objs64[b, r]) / max(abs(objs64[b, r]), 1e-300) if objs64[b, r] else abs(obj[b, r]) for b, r in ok)
    ec = max(rel_err(cent[b, r], cents64[b, r]) for b, r in ok)
    return float(eo), float(ec)


def check_kmeans_fit(side, p, rng, note):
    B, n, d, k, nredo, niter = p["B"], p["n"], p["d"], p["k"], p["nredo"], p["niter"]
    # Inputs valid by construction: blobs are drawn from the case's generator until the fp64 run proves them valid (the pinned cases'
    # spreads were chosen so that the first draw is; of a fuzz draw's blobs two can nearly coincide).  Nothing of the code under test enters.
    for attempt in range(FIT_DRAWS):
        x, init, flagged = fit_inputs(rng, p)
        try:
            cents64, objs64, min_gap = fit_reference(x, init, niter, flagged)
            break
        except InvalidFitInputs:
            if attempt == FIT_DRAWS - 1:
                raise
    note("input draws until valid", attempt + 1, FIT_DRAWS, strict=True)
    cent, obj, status = side.kmeans_fit(x, init, niter, p["offset"])
    assert cent.shape == (B, nredo, k, d) and obj.shape == (B, nredo) and status.shape == (B, nredo)
    want_status = np.zeros((B, nredo), np.int32)
    for b, r in flagged:
        want_status[b, r] = 1          # the first assignment already leaves the cluster empty
    assert np.array_equal(status, want_status), ("status", np.argwhere(status != want_status)[:8])
    ok = [(b, r) for b in range(B) for r in range(nredo) if (b, r) not in flagged]
    tol = TOL_FIT
    long_run = km_accumulate_blocks(n)[1] > FIT_LONG_RUN
    if long_run:      # nobody has measured these runs: 4 x the twin's own error on this case, never below the existing bound
        tc, to, _ = (cent, obj, status) if side.name == "twin" else MetricTwin().kmeans_fit(x, init, niter)
        t_eo, t_ec = _fit_errors(tc, to, cents64, objs64, ok)
        note("twin objective (points per block > 128)", t_eo, TOL_FIT)
        note("twin centroids (points per block > 128)", t_ec, TOL_FIT)
        tol = max(TOL_FIT, 4.0 * max(t_eo, t_ec))
    eo, ec = _fit_errors(cent, obj, cents64, objs64, ok)
    tag = " (points per block > 128)" if long_run else ""
    note("objective" + tag, eo, tol)
    note("centroids" + tag, ec, tol)
    note("1 / smallest relative gap of the fp64 run x KM_GAP", KM_GAP / min_gap if np.isfinite(min_gap) else 0.0, 1.0)
    if side.name == "twin":
        return
    # ---- the contract's bit equalities (include/timetuning_hip.h): the loop of clustering.Kmeans from the same seeds
    for b in sample_problems(B):
        for r in range(nredo):
            if (b, r) in flagged:
                continue
            lc, lo, splits = side.fit_loop(x[b], init[r], niter)
            assert splits == [], (b, r, splits)
            assert np.array_equal(lc, cent[b, r]), ("centroids differ from the loop's", b, r)
            assert abs(obj[b, r] - lo) <= 1e-12 * abs(lo), ("objective differs from the loop's", b, r, obj[b, r], lo)
    if flagged:       # the others' bits are those of batches without the flagged (problem, redo)
        keep = [b for b in range(B) if all(fb != b for fb, _ in flagged)]
        c2, o2, s2 = side.kmeans_fit(x[keep], init, niter)
        assert (s2 == 0).all() and np.array_equal(c2, cent[keep]) and np.array_equal(o2, obj[keep])
        for fb, fr in flagged:
            rest = [r for r in range(nredo) if r != fr]
            c3, o3, s3 = side.kmeans_fit(x, init[rest], niter)
            assert (s3 == 0).all() and np.array_equal(c3[fb], cent[fb][rest]) and np.array_equal(o3[fb], obj[fb][rest])


# ---- the segmented confusion counts -----------------------------------------------------------------------------------------------------------------

def _seen(op, p, counts2d, got):
    COLUMNS.setdefault(op, {})[case_id(op, p)] = np.asarray(counts2d, np.int64).reshape(-1, counts2d.shape[-1]).sum(0)
    COMPARED.setdefault(op, {})[case_id(op, p)] = got is not None


def confusion_direct(pred, gt, Cg, Cp, ignore):
    """The definition, element by element (confusion.hip's header): counts[s][g][p] += 1 where 0 <= g < Cg, 0 <= p < Cp and g != ignore."""
    out = np.zeros((pred.shape[0], Cg, Cp), np.int64)
    for s in range(pred.shape[0]):
        for e in range(pred.shape[1]):
            g, q = int(gt[s, e]), int(pred[s, e])
            if 0 <= g < Cg and 0 <= q < Cp and (ignore is None or g != ignore):
                out[s, g, q] += 1
    return out


def check_confusion_segments(side, p, rng, note):
    S, n, Cg, Cp = p["S"], p["n"], p["Cg"], p["Cp"]
    ignore = None if p["ignore"] == "" else int(p["ignore"])
    total = S * n
    # labels in [-1, C + 1] (-1 and values >= C among them); the first half in runs of 16, as up-sampled token maps (the strips merge them)
    def labels(Cn):
        a = rng.integers(-1, Cn + 2, total)
        h = total // 2
        a[:h] = np.repeat(a[:(h + 15) // 16], 16)[:h]
        return a
    pred, gt = labels(Cp).astype(np.int16 if p["dtype"] == "i16" else np.int64).reshape(S, n), labels(Cg).astype(np.int64).reshape(S, n)
    gt.reshape(-1)[::37] = 255                              # the Pascal border value, inside or outside [0, Cg)
    want = R.confusion_segments_np(pred, gt, Cg, Cp, ignore)
    got = side.confusion_segments(pred, gt, Cg, Cp, ignore, p["offset"])
    if got is not None:
        assert got.shape == (S, Cg, Cp) and np.array_equal(got, want), np.argwhere(got != want)[:8]
    # (columns: counted elements, elements dropped for a label outside the matrix, elements dropped by the ignore value)
    inside = (gt >= 0) & (gt < Cg) & (pred >= 0) & (pred < Cp)
    _seen("confusion_segments", p, np.array([[int(want.sum()), int((~inside).sum()), int(inside.sum() - want.sum())]]), got)


# ---- the DAVIS J&F counts ------------------------------------------------------------------------------------------------------------------------------

def _blob_labels(rng, T, H, W, O, dtype):
    """Blobs of 1..O plus values outside 1..O (0, O + 1, and for int64 negatives and large ids): tests/test_hip_davis_metrics.py::_labels"""
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.zeros((T, H, W), np.int64)
    for t in range(T):
        for o in range(1, O + 3):
            cy, cx = rng.uniform(-0.2, 1.2) * H, rng.uniform(-0.2, 1.2) * W
            ry, rx = rng.uniform(0.1, 0.5) * H + 0.5, rng.uniform(0.1, 0.5) * W + 0.5
            lab[t][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = o
        noise = rng.random((H, W)) < 0.02
        lab[t][noise] = rng.integers(0, O + 2, int(noise.sum()))
    if dtype == np.int64:
        odd = rng.random(lab.shape) < 0.01
        lab[odd] = rng.choice([-1, -(O + 1), 1 << 40, 257], int(odd.sum()))
    return lab.astype(dtype)


def davis_direct(pred, gt, O, element, void):
    """The six counts from the definitions, pixel by pixel (mask_propagation.py: db_eval_iou, _seg2bmap, f_measure with cv2.dilate's rule
    dst(y, x) = max over the set (i, j) of src(y + i - ay, x + j - ax), anchor (rows // 2, cols // 2), nothing outside the image)."""
    T, H, W = pred.shape
    el = np.asarray(element)
    ay, ax = el.shape[0] // 2, el.shape[1] // 2
    offs = [(i - ay, j - ax) for i in range(el.shape[0]) for j in range(el.shape[1]) if el[i, j]]
    out = np.zeros((O, T, 6), np.int64)

    def boundary(s):
        b = [[False] * W for _ in range(H)]
        for y in range(H):
            for x in range(W):
                v = False
                if x < W - 1:
                    v = s[y][x] != s[y][x + 1]
                if y < H - 1:
                    v = v or s[y][x] != s[y + 1][x]
                if x < W - 1 and y < H - 1:
                    v = v or s[y][x] != s[y + 1][x + 1]
                b[y][x] = v
        return b

    def matched(mine, other):
        m = 0
        for y in range(H):
            for x in range(W):
                if mine[y][x]:
                    for dy, dx in offs:
                        yy, xx = y + dy, x + dx
                        if 0 <= yy < H and 0 <= xx < W and other[yy][xx]:
                            m += 1
                            break
        return m

    for o in range(1, O + 1):
        for t in range(T):
            keep = [[void is None or void[t, y, x] == 0 for x in range(W)] for y in range(H)]
            P = [[bool(pred[t, y, x] == o) and keep[y][x] for x in range(W)] for y in range(H)]
            G = [[bool(gt[t, y, x] == o) and keep[y][x] for x in range(W)] for y in range(H)]
            fb, gb = boundary(P), boundary(G)
            out[o - 1, t] = [sum(P[y][x] and G[y][x] for y in range(H) for x in range(W)), sum(P[y][x] or G[y][x] for y in range(H) for x in range(W)),
                             sum(map(sum, fb)), sum(map(sum, gb)), matched(fb, gb), matched(gb, fb)]
    return out


_NP_DT = {"u8": np.uint8, "i64": np.int64}


def check_davis_counts(side, p, rng, note):
    from timetuning_amd import mask_propagation as MP

    T, H, W, O = p["T"], p["H"], p["W"], p["O"]
    gt, pred = _blob_labels(rng, T, H, W, O, _NP_DT[p["gtt"]]), _blob_labels(rng, T, H, W, O, _NP_DT[p["pt"]])
    void = (rng.random((T, H, W)) < 0.05).astype(np.uint8) if p["void"] else None
    el = MP.disk(p["radius"])
    want = R.davis_np_counts(pred, gt, O, el, void)
    got = side.davis_counts(pred, gt, O, el, void)
    if got is not None:
        assert got.shape == (O, T, 6) and np.array_equal(got, want), np.argwhere(got != want)[:8]
    _seen("davis_counts", p, want, got)


# ---- the boundary-F counts ------------------------------------------------------------------------------------------------------------------------------

def _blob_maps(rng, P, H, W):
    """Two stacks of binary maps, three ellipses and 1 % flipped pixels each; the second with any non-zero value for "set"
    (tests/test_hip_bfscore.py::_maps, "blobs")."""
    out = []
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(2):
        m = np.zeros((P, H, W), np.uint8)
        for k in range(P):
            for _ in range(3):
                cy, cx = rng.uniform(0, H), rng.uniform(0, W)
                ry, rx = rng.uniform(0.1, 0.4) * H + 0.5, rng.uniform(0.1, 0.4) * W + 0.5
                m[k][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = 1
            m[k] ^= (rng.random((H, W)) < 0.01).astype(np.uint8)
        out.append(m)
    return out[0], out[1] * rng.integers(1, 256, (P, H, W)).astype(np.uint8)


def bf_direct(gt, pr, t):
    """The four counts from the definition (bfscore.py): the contour points of each map as the border follower visits them
    (tests/_border_follow.py: a pixel counts once per visit), and for each point of one list whether ANY point of the other lies at an
    integer squared distance d < t * t - calc_precision_recall's test, on the point lists themselves.  The distance side shares nothing
    with the restatement.  The multiplicity side is NOT a fully separate definition: the follower is the module the restatement's
    256-entry table is derived from (on isolated 3 x 3 contexts); what this adds is the follower run on the real map, every pixel in its
    real surroundings and at the image edge, against the table looked up per pixel."""
    tt = float(t) * float(t)
    out = np.zeros((gt.shape[0], 4), np.int64)
    for k in range(gt.shape[0]):
        pts = []
        for m in (pr[k], gt[k]):
            v = bfl.visit_counts((np.asarray(m) != 0).astype(np.uint8))
            pts.append([(y, x, int(v[y, x])) for y in range(v.shape[0]) for x in range(v.shape[1]) if v[y, x] > 0])
        for side_, (mine, other) in enumerate(((pts[0], pts[1]), (pts[1], pts[0]))):
            n = hit = 0
            for y, x, mult in mine:
                n += mult
                for oy, ox, _ in other:
                    if (oy - y) * (oy - y) + (ox - x) * (ox - x) < tt:
                        hit += mult
                        break
            out[k, 2 * side_], out[k, 2 * side_ + 1] = n, hit
    return out


def check_bf_counts(side, p, rng, note):
    P, H, W, t = p["P"], p["H"], p["W"], p["t"]
    gt, pr = _blob_maps(rng, P, H, W)
    want = R.bf_np_counts(gt, pr, t)
    got = side.bf_counts(gt, pr, t)
    if got is not None:
        assert got.shape == (P, 4) and np.array_equal(got, want), (got, want)
    _seen("bf_counts", p, want, got)


CHECK = {"kmeans_assign_tiled": check_kmeans_assign_tiled, "kmeans_accumulate_tiled": check_kmeans_accumulate_tiled,
         "kmeans_assign_batched": check_kmeans_assign_batched, "kmeans_fit": check_kmeans_fit, "confusion_segments": check_confusion_segments,
         "davis_counts": check_davis_counts, "bf_counts": check_bf_counts}


def run_metric_case(side, op: str, params: dict, worst: dict) -> None:
    CHECK[op](side, params, case_rng(op, params), make_note(worst, op))
