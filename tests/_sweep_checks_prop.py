"""The checks of the sweep's third tier (tests/_sweep_cases.py, PROP_OPS): temporal label propagation - the square entries with their six
per-query kernels, three similarity slot regimes and chunking, the rectangular-grid entry and its up-sampler - against a plain fp64
restatement.  One check per op, run on two sides as the second tier's are (tests/_sweep_checks_eval.py): the plain-C twins of
oracle/tt_cpu.c (tests/test_sweep_prop_host.py, no GPU) and the HIP library (tests/test_hip_sweep.py).

The reference works ONE FRAME AT A TIME: frame t's map is computed in fp64 from the seed and from the maps of the frames before t AS THE
SIDE UNDER TEST RETURNED THEM.  Every frame is judged on its own - an error cannot be blamed on, or hidden by, an earlier frame - and the
bound is a one-frame bound:

    |map - reference| <= (1e-6 + (m - 1) * 2^-24) * (largest entry of the frame's reference map)

m = the most sources any query of the frame keeps, counted by the reference.  1e-6 is the bound tests/test_hip_label_prop_grid.py holds:
it carries expf and the fp32 quotient sim / 0.1f.  (m - 1) * 2^-24 is the worst-case error of the operation's own fp32 column sum over m
positive terms in whatever order (hundreds of exact ties per query make it the larger term: 8.1e-7 measured on the twin at g 64, D 4, K 2).

Two input families per case.
  * EXACT SELECTION: tokens with entries j / 8, |j| small enough (and, beyond D = 64, few enough non-zeros) that |sim| <= 1 and every
    product and sum is exact in fp32, in fp16 pairs and in bf16.  All three precisions then select exactly the sources the reference
    selects, exact ties included; no query is excused.  With ``dup`` every third token repeats the first one, and a label column is
    repeated at a higher index: exactly equal channels, where the lower index must win (the first-maximum rule across lanes and slots).
  * REAL VALUED (f32 and f16x3 only): unit-normalised Gaussian tokens, x_t = 0.7 x_(t-1) + 0.3 noise.  A query may miss the bound only if
    the reference's topk-th and (topk+1)-th largest affinities are within DELTA = 10 * D * 2^-24 relative of each other - the worst-case
    error of one fp32 dot product of unit vectors, divided by the temperature 0.1 -, on at most 1 % of a case's queries; the reference
    alone may mark at most 0.5 % excusable, so the inputs cannot use up the cap.  Excused or not, every map row still sums to 1 within 1e-6.

Equalities, bit for bit: tt_label_propagate's map is the last of tt_label_propagate_maps and its labels that map's first-maximum arg-max;
the two-call form equals the one-call form and declines exactly when more than one chunk is needed; every chunking equals the whole run.
The grid entry agrees with the square entry within the one-frame bound wherever both take the shape."""
from __future__ import annotations

import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from _sweep_cases import LP_CAND_CAP, lp_caps, lp_chunk, lp_cmax
from _sweep_checks_eval import HipSide, TwinSide, _excuse_cap, _ptr, case_rng, make_note

f32, f64 = np.float32, np.float64
TEMP = 0.1
TOL_MAP = 1e-6                     # tests/test_hip_label_prop_grid.py: expf and the fp32 quotient sim / 0.1f
EPS32 = 2.0 ** -24
EXCUSE_CAP, EXCUSE_REF_CAP = 0.01, 0.005
TOL_ROWSUM = 1e-6
HW_GAP = 1e-9                      # relative gap of the two best interpolated channels under which an up-sampled label may differ
QBLOCK = 256                       # queries per block of the reference (a [c * n, block] fp64 affinity at a time)


def map_bound(m: int) -> float:
    return TOL_MAP + max(m - 1, 0) * EPS32


def sims_cap(side, mb):
    """The knob TT_LP_SIMS_CAP_MB for the HIP side's calls inside (the twins hold every frame's similarities at once: nothing to cap)."""
    return side.ops.tuning_knob("TT_LP_SIMS_CAP_MB", mb) if side.name == "hip" else contextlib.nullcontext()


# ---- the two sides ---------------------------------------------------------------------------------------------------------------------------

class PropTwin(TwinSide):
    def route(self, *a):
        return self._lib.load().tt_label_propagate_route(*a)

    def lp_maps(self, xn, seed, nl, r, topk, prec):
        fs, bs, n, D = xn.shape
        g, K = int(round(n ** 0.5)), seed.shape[-1]
        maps = np.full((fs - 1, bs, n, K), np.nan, f64)
        self._run("label_propagate_maps", xn, seed, maps, bs, fs, g, D, K, nl, r, topk, TEMP, 0, None, 0, None)
        return maps

    def lp_labels(self, xn, seed, nl, r, topk, prec, two_call=False):
        fs, bs, n, D = xn.shape
        g, K = int(round(n ** 0.5)), seed.shape[-1]
        labels, pmap = np.full((bs, n), -1, np.int64), np.full((bs, n, K), np.nan, f64)
        if two_call:
            self._run("label_propagate_sims", xn, bs, fs, g, D, K, nl, 0, None, 0, None)
            self._run("label_propagate_from_sims", xn, seed, labels, pmap, bs, fs, g, D, K, nl, r, topk, TEMP, None, 0, None)
        else:
            self._run("label_propagate", xn, seed, labels, pmap, bs, fs, g, D, K, nl, r, topk, TEMP, 0, None, 0, None)
        return labels, pmap

    def lp_grid_maps(self, xn, seed, grid, nl, r, topk, prec):
        fs, bs, n, D = xn.shape
        K = seed.shape[-1]
        maps = np.full((fs - 1, bs, n, K), np.nan, f64)
        self._run("label_propagate_grid_maps", xn, seed, maps, bs, fs, grid[0], grid[1], D, K, nl, r, topk, TEMP, 0, None, 0, None)
        return maps

    def upsample_argmax_hw(self, maps, grid, size):
        M, n, K = maps.shape
        out = np.full((M, size[0], size[1]), -1, np.int64)
        self._run("upsample_argmax_hw", maps, out, M, grid[0], grid[1], K, size[0], size[1], None)
        return out

    def refuses(self, fn, match):
        return None      # (the twins check nothing: the refusals are the launchers')


class PropHip(HipSide):
    def route(self, *a):
        return self._lib.load().tt_label_propagate_route(*a)

    @contextlib.contextmanager
    def _prec(self, prec):
        keep = self.ops.get_gemm_precision()
        self.ops.set_gemm_precision(prec)
        try:
            yield
        finally:
            self.ops.set_gemm_precision(keep)

    def lp_maps(self, xn, seed, nl, r, topk, prec):
        with self._prec(prec):
            return self._h(self.ops.label_propagate_maps(self._d(xn), self._d(seed), nl, r, topk, TEMP))

    def lp_labels(self, xn, seed, nl, r, topk, prec, two_call=False):
        """-> labels, pmap; with ``two_call`` None when the first half declines (more than one chunk)."""
        with self._prec(prec):
            xd, sd = self._d(xn), self._d(seed)
            sims = None
            if two_call:
                sims = self.ops.label_propagate_sims(xd, seed.shape[-1], nl)
                if sims is None:
                    return None
            labels, pmap = self.ops.label_propagate(xd, sd, nl, r, topk, TEMP, return_pmap=True, sims=sims)
            return self._h(labels), self._h(pmap)

    def lp_grid_maps(self, xn, seed, grid, nl, r, topk, prec):
        with self._prec(prec):
            return self._h(self.ops.label_propagate_grid_maps(self._d(xn), self._d(seed), grid, nl, r, topk, TEMP))

    def upsample_argmax_hw(self, maps, grid, size):
        return self._h(self.ops.upsample_argmax_hw(self._d(maps), grid, size))

    def refuses(self, fn, match):
        import pytest

        with pytest.raises(self._lib.HipLibraryError, match=match):
            fn()


_TWIN = None


def prop_twin():
    global _TWIN
    if _TWIN is None:
        _TWIN = PropTwin()
    return _TWIN


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------

def exact_tokens(rng, fs, bs, n, D, dup):
    """Entries j / 8 with |sim| <= 1 exactly: |j| <= L = floor(sqrt(64 / D)) up to D = 64; beyond, +-1/8 in 64 positions of each token."""
    if D <= 64:
        L = int(np.sqrt(64 / D))
        x = rng.integers(-L, L + 1, (fs, bs, n, D)).astype(f32) / f32(8)
    else:
        x = np.zeros((fs, bs, n, D), f32)
        pos = np.argsort(rng.random((fs, bs, n, D)), axis=-1)[..., :64]
        np.put_along_axis(x, pos, (rng.integers(0, 2, pos.shape) * 2 - 1).astype(f32) / f32(8), axis=-1)
    if dup:
        x[:, :, ::3] = x[:, :, :1]
    return x


def real_tokens(rng, fs, bs, n, D):
    x = rng.standard_normal((fs, bs, n, D))
    for t in range(1, fs):
        x[t] = 0.7 * x[t - 1] + 0.3 * x[t]
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(f32)


def seeds(rng, bs, n, K, dup):
    """softmax(2 * normal) rows (they sum to 1).  ``dup``: column ``hi`` repeats column ``lo`` < hi - in another lane, and another slot of
    a lane when K > 64 - and that column is the largest on about half the rows.  -> seed, (lo, hi) or None"""
    logits = 2.0 * rng.standard_normal((bs, n, K))
    pair = None
    if dup and K > 1:
        lo, hi = int(rng.integers(0, min(K - 1, 64))), K - 1
        logits[..., lo] += np.where(rng.random((bs, n)) < 0.5, 4.0, 0.0)
        pair = (lo, hi)
    s = torch.softmax(torch.from_numpy(logits), -1).numpy().astype(f32)
    if pair:
        s[..., pair[1]] = s[..., pair[0]]
    return s, pair


# ---- the reference, one frame -----------------------------------------------------------------------------------------------------------------

def ctx_frames(t, nl):
    return [0] + list(range(max(1, t - nl), t))


def ref_frame(xn, ctx_maps, t, grid, nl, radius, topk, D):
    """One clip, one target frame, in fp64: xn [fs, n, D] (the fp32 tokens the side was given), ctx_maps = the [n, K] maps of
    ctx_frames(t, nl) -> (map [n, K], m = the most sources a query keeps, excusable [n] bool).  Affinity exp(sim / T) inside the
    |dy|, |dx| <= radius window (radius 0: everywhere), 0 outside; kept: aff >= the topk-th largest of the column, the masked zeros
    counting (so fewer than topk candidates keep everything); weights aff / column sum.  ``excusable``: the relative gap between the
    topk-th and the (topk+1)-th largest affinity is below 10 * D * 2^-24."""
    gh, gw = grid
    n = gh * gw
    ctx = ctx_frames(t, nl)
    xt = torch.from_numpy(xn[t]).double()
    xc = torch.from_numpy(xn[ctx]).double()                                  # [c, n, D]
    cm = torch.from_numpy(np.concatenate(ctx_maps, 0)).double()              # [c * n, K]
    sy, sx = torch.arange(n) // gw, torch.arange(n) % gw
    out = torch.empty((n, cm.shape[1]), dtype=torch.float64)
    excusable = torch.zeros(n, dtype=torch.bool)
    m, delta = 0, 10.0 * D * EPS32
    for q0 in range(0, n, QBLOCK):
        q1 = min(n, q0 + QBLOCK)
        aff = torch.exp(torch.einsum("qd,csd->qcs", xt[q0:q1], xc) / TEMP)   # [q, c, n]
        if radius > 0:
            win = ((sy[q0:q1, None] - sy[None]).abs() <= radius) & ((sx[q0:q1, None] - sx[None]).abs() <= radius)
            aff = aff * win[:, None, :]
        aff = aff.reshape(q1 - q0, -1)
        top = torch.topk(aff, min(topk + 1, aff.shape[1]), dim=1).values     # descending
        kth = top[:, topk - 1] if aff.shape[1] >= topk else torch.zeros(q1 - q0, dtype=torch.float64)
        if aff.shape[1] > topk:
            excusable[q0:q1] = (top[:, topk] > 0) & ((top[:, topk - 1] - top[:, topk]) < delta * top[:, topk - 1])
        aff = torch.where(aff >= kth[:, None], aff, torch.zeros_like(aff))
        m = max(m, int((aff > 0).sum(1).max()))
        out[q0:q1] = (aff / aff.sum(1, keepdim=True)) @ cm
    return out.numpy(), m, excusable.numpy()


def judge_maps(maps, xn, seed, grid, nl, radius, topk, note, what, excuse, pair, rows_sum_to_one):
    """Every frame of ``maps`` [fs-1, bs, n, K] (as a side returned them) against ref_frame fed with the side's own earlier frames.
    ``excuse``: the real-valued family's rule (False: no query is excused).  -> the largest m of any frame"""
    fs1, bs, n, K = maps.shape
    D = xn.shape[-1]
    assert np.isfinite(maps).all(), "a map entry was left unwritten or is not finite"
    excused = ref_marked = m_max = 0
    for b in range(bs):
        for t in range(1, fs1 + 1):
            got = maps[t - 1, b]
            ctx_maps = [seed[b].astype(f64) if f == 0 else maps[f - 1, b] for f in ctx_frames(t, nl)]
            want, m, exc = ref_frame(xn[:, b], ctx_maps, t, grid, nl, radius, topk, D)
            bound, m_max = map_bound(m), max(m_max, m)
            scale = max(np.abs(want).max(), 1e-30)
            err = np.abs(got - want).max(-1) / scale                           # per query
            ref_marked += int(exc.sum())
            if excuse:
                off = err >= bound
                assert not (off & ~exc).any(), (what, "a query misses the bound away from a near-tie of the topk-th affinity", b, t,
                                                float(err[off & ~exc].max()), bound)
                excused += int(off.sum())
                note(f"{what} map / bound (queries not excused)", float((err[~off].max() if (~off).any() else 0.0) / bound), 1.0)
            else:
                note(f"{what} map / bound", float(err.max() / bound), 1.0)
                note(f"{what} map max", float(err.max()), bound)
                # labels: the first maximum of the frame's map, wherever the reference's two best channels are further apart than the bound
                if K > 1:
                    top2 = np.sort(np.partition(want, K - 2, axis=-1)[:, K - 2:], axis=-1)
                    clear = (top2[:, 1] - top2[:, 0]) > bound * scale
                    assert np.array_equal(got.argmax(-1)[clear], want.argmax(-1)[clear]), (what, "arg-max differs on a clear query", b, t)
            if pair is not None:    # exactly equal channels: bit-equal columns, and the lower index wins
                assert np.array_equal(got[:, pair[0]], got[:, pair[1]]), (what, "duplicated label columns differ", b, t)
                assert not (got.argmax(-1) == pair[1]).any()
            if rows_sum_to_one:
                note(f"{what} |row sum - 1|", float(np.abs(got.sum(-1) - 1.0).max()), TOL_ROWSUM)
    Q = fs1 * bs * n
    if excuse:
        note(f"{what} excused / allowed", excused, int(EXCUSE_CAP * Q), strict=True)
        note(f"{what} excusable by the reference / queries", ref_marked / Q, EXCUSE_REF_CAP, strict=True)
    return m_max


# ---- the square entries ------------------------------------------------------------------------------------------------------------------------

def lp_refusal(p):
    """The launcher's own message for a case outside the domain (None inside)."""
    win = min(2 * p["r"] + 1, p["g"])
    if win * win * lp_cmax(p["fs"], p["nl"]) > LP_CAND_CAP:
        return r"window %dx%d with %d context frames exceeds 4096 candidates per query" % (win, win, lp_cmax(p["fs"], p["nl"]))
    return None


def check_label_prop(side, p, rng, note):
    bs, fs, g, D, K, nl, r, topk, prec, dup = (p[k] for k in ("bs", "fs", "g", "D", "K", "nl", "r", "topk", "prec", "dup"))
    n = g * g
    routes = [side.route(fs, g, K, nl, r, t) for t in range(1, fs)]
    seed, pair = seeds(rng, bs, n, K, dup)
    xq = exact_tokens(rng, fs, bs, n, D, dup)
    msg = lp_refusal(p)
    if msg is not None:      # beyond the domain: the route query says so, and the launcher refuses ahead of any launch
        assert routes == [0] * (fs - 1)
        side.refuses(lambda: side.lp_maps(xq, seed, nl, r, topk, prec), msg)
        side.refuses(lambda: side.lp_labels(xq, seed, nl, r, topk, prec), msg)
        return
    assert all(1 <= rt <= 6 for rt in routes), routes
    families = [("exact", xq, False)]
    if prec != "bf16":
        families.append(("real", real_tokens(rng, fs, bs, n, D), True))
    for fam, xn, excuse in families:
        maps = side.lp_maps(xn, seed, nl, r, topk, prec)
        m_max = judge_maps(maps, xn, seed, (g, g), nl, r, topk, note, fam, excuse, pair, excuse and pair is None)
        # tt_label_propagate: the last map and its first-maximum arg-max, bit for bit
        labels, pmap = side.lp_labels(xn, seed, nl, r, topk, prec)
        assert np.array_equal(pmap, maps[-1]), (fam, "pmap_last is not the last map of tt_label_propagate_maps")
        assert np.array_equal(labels, pmap.argmax(-1)), (fam, "labels are not the first-maximum arg-max of pmap_last")
        # the two-call form: equal, or declined exactly when the similarities need more than one chunk
        two = side.lp_labels(xn, seed, nl, r, topk, prec, two_call=True)
        if side.name == "hip":
            assert (two is None) == (lp_chunk(bs, fs, n, nl) < fs - 1), (fam, "two-call form", lp_chunk(bs, fs, n, nl))
        if two is not None:
            assert np.array_equal(two[0], labels) and np.array_equal(two[1], pmap), (fam, "two-call form differs")
        # every chunking equals the whole run
        for cap in lp_caps(p):
            with sims_cap(side, cap):
                assert np.array_equal(side.lp_maps(xn, seed, nl, r, topk, prec), maps), (fam, "chunked run differs", cap, lp_chunk(bs, fs, n, nl, cap))
                if side.name == "hip" and lp_chunk(bs, fs, n, nl, cap) < fs - 1:
                    assert side.lp_labels(xn, seed, nl, r, topk, prec, two_call=True) is None
        # the grid entry on the same square grid: the same selection, another summation order
        if fam == "exact" and n <= 1024:
            gm = side.lp_grid_maps(xn, seed, (g, g), nl, r, topk, prec)
            scale = np.abs(maps).reshape(fs - 1, -1).max(1).reshape(-1, 1, 1, 1)
            note("grid entry vs square entry", float((np.abs(gm - maps) / scale).max()), map_bound(m_max))
            judge_maps(gm, xn, seed, (g, g), nl, r, topk, note, "grid entry on the square grid,", False, pair, False)


def check_label_prop_grid(side, p, rng, note):
    bs, fs, gh, gw, D, K, nl, r, topk, prec, dup = (p[k] for k in ("bs", "fs", "gh", "gw", "D", "K", "nl", "r", "topk", "prec", "dup"))
    n = gh * gw
    seed, pair = seeds(rng, bs, n, K, dup)
    families = [("exact", exact_tokens(rng, fs, bs, n, D, dup), False)]
    if prec != "bf16":
        families.append(("real", real_tokens(rng, fs, bs, n, D), True))
    for fam, xn, excuse in families:
        maps = side.lp_grid_maps(xn, seed, (gh, gw), nl, r, topk, prec)
        judge_maps(maps, xn, seed, (gh, gw), nl, r, topk, note, fam, excuse, pair, excuse and pair is None)


# ---- the up-sampler ------------------------------------------------------------------------------------------------------------------------------

def check_upsample_argmax_hw(side, p, rng, note):
    M, gh, gw, K, H, W, dup = (p[k] for k in ("M", "gh", "gw", "K", "H", "W", "dup"))
    maps = rng.random((M, gh * gw, K))
    pair = None
    if dup and K > 1:
        lo = int(rng.integers(0, K - 1))
        pair = (lo, K - 1)
        maps[..., lo] += np.where(rng.random((M, gh * gw)) < 0.5, 1.0, 0.0)
        maps[..., K - 1] = maps[..., lo]
    got = side.upsample_argmax_hw(maps, (gh, gw), (H, W)).reshape(M, H * W)
    assert got.min() >= 0 and got.max() < K, "a pixel was left unwritten or labelled outside [0, K)"
    up = F.interpolate(torch.from_numpy(maps).transpose(1, 2).reshape(M, K, gh, gw), size=(H, W), mode="bilinear", align_corners=False)
    up = up.reshape(M, K, H * W).transpose(1, 2)
    top = torch.topk(up, min(2, K), dim=-1)
    want, best = top.indices[..., 0].numpy(), top.values[..., 0].numpy()
    second = top.values[..., 1].numpy() if K > 1 else np.full_like(best, -np.inf)
    if pair is not None:      # the duplicated channel is the largest on some pixels: an exact tie there, and the lower index wins
        assert not (got == pair[1]).any(), "the higher index of a duplicated channel was chosen"
        tied = np.isin(want, pair)
        assert tied.any() and (got[tied] == pair[0]).all()
        want, second = np.where(tied, pair[0], want), np.where(tied, best, second)   # (elsewhere the two best are distinct channels)
        assert K == 2 or not tied.all()
    mism = got != want
    assert (best[mism] - second[mism] <= HW_GAP * np.abs(maps).max()).all(), "a label differs from the fp64 arg-max away from a near-tie"
    note("labels excused / allowed", int(mism.sum()), _excuse_cap(M * H * W), strict=True)


CHECK = {"label_prop": check_label_prop, "label_prop_grid": check_label_prop_grid, "upsample_argmax_hw": check_upsample_argmax_hw}


def run_prop_case(side, op: str, params: dict, worst: dict) -> None:
    CHECK[op](side, params, case_rng(op, params), make_note(worst, op))
