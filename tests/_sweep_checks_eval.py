"""The checks of the sweep's second tier (tests/_sweep_cases.py, EVAL_OPS): the evaluator, optimizer and mask kernels against fp64 references.

One check per op, written once and run on two "sides": ``TwinSide`` - the plain-C twins of oracle/tt_cpu.c on host buffers
(tests/test_sweep_eval_host.py, no GPU) - and ``HipSide`` - the HIP library through timetuning_amd.hip_ops on cuda:0
(tests/test_hip_sweep.py).  Both halves build the same inputs (seeded by the case id), the same fp64 reference and assert the same bounds;
the host half is where the references, the generators and the excuse rules are proved before a GPU is involved.

Bounds are the ones the single-shape tests hold (tests/test_hip_evaluator.py, tests/test_hip_ops.py, tests/test_cpu_twin.py).  Where a regime
cannot be expected to keep one - AdamW at step 100 000 - the bound is 4 x the error of the fp32 twin against fp64 ON THAT CASE, never below
the existing bound: summation and rounding order may cost a factor of a few, a dropped tail or block costs orders of magnitude.  The twins
of tt_col_moments, tt_kmeans_accumulate and tt_colsum already work in fp64: there the existing bound simply stays.

Excuse rules are capped: an arg-min / arg-max label may differ from the fp64 one only where best and second best are within the stated gap,
on at most 1e-4 of a case's points, and on none when the case has fewer than 10 000; a foreground-mask pixel only inside the two-ring
surroundings of a pixel within 2e-6 of the mass cut, a region that may cover at most 1 % of a case's pixels."""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from _sweep_cases import case_id

f32, f64 = np.float32, np.float64
TOL_MEAN, TOL_VAR = 1e-10, 1e-9     # tests/test_hip_evaluator.py::test_col_moments_and_affine
TOL_EVAL = 1e-6                     # affine, bilinear up-sampling (test_hip_evaluator.py); AdamW, EMA (test_hip_ops.py); colsum (test_cpu_twin.py)
TOL_KM = 1e-5                       # k-means distances and sums (test_hip_evaluator.py::test_kmeans_kernels)
TOL_BLUR = 2e-5                     # the blurred attention (test_hip_ops.py: TOL)
TOL_POS = 1e-5                      # bicubic position table (test_cpu_twin.py)
TOL_L2N = 2e-5                      # row normalisation: the sweep's TOL_F32
KM_GAP = 1e-4                       # relative gap of best and second-best distance under which a k-means label may differ
ARGMAX_GAP = 1e-12                  # absolute gap for the fp64 arg-max (test_hip_timet.py::test_upsample_argmax_vs_torch)
EXCUSE_SHARE, EXCUSE_MIN_POINTS = 1e-4, 10000
MASK_MARGIN, MASK_REGION_CAP = 2e-6, 0.01


def rel_err(a, b) -> float:
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def case_rng(op, p):
    return np.random.default_rng(zlib.crc32(case_id(op, p).encode()))


def _normal(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape, dtype=f32) * f32(scale)).astype(f32)


def mask_mismatch_excusable(mask, want, margin, tol=MASK_MARGIN):
    """A pixel may land on the other side of the mass cut only where its cumulative mass is within rounding of the
    cut; such a flip can also change which neighbours form a <= 2-pixel component, so the excuse covers 3x3
    surroundings of any near-cut pixel."""
    mism = mask != want
    if not mism.any():
        return True
    return bool((~mism | mask_excusable_region(margin, tol)).all())


def mask_excusable_region(margin, tol=MASK_MARGIN):
    Fr, n = margin.shape
    g = int(round(n ** 0.5))
    near = (margin < tol).reshape(Fr, 1, g, g).float()
    return F.max_pool2d(near, 5, 1, 2).reshape(Fr, n).bool()   # 2 rings: the flipped pixel's neighbours' neighbours


def _excuse_cap(points: int) -> int:
    return int(EXCUSE_SHARE * points) if points >= EXCUSE_MIN_POINTS else 0


# ---- the two sides ---------------------------------------------------------------------------------------------------------------------------

def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class TwinSide:
    """oracle/tt_cpu.c on host buffers: every method takes and returns NumPy arrays."""
    name = "twin"

    def __init__(self):
        from oracle import cpu_twin
        from timetuning_amd import _lib

        self.lib, self._lib = cpu_twin.load(), _lib

    def _run(self, name, *args):
        rc = getattr(self.lib, "tt_cpu_" + name)(*[_ptr(a) if isinstance(a, np.ndarray) else a for a in args])
        assert rc == 0, (name, rc)

    def kmeans_assign(self, x, c):
        P, d = x.shape
        labels, dist2 = np.full(P, -1, np.int32), np.empty(P, f32)
        self._run("kmeans_assign", x, c, labels, dist2, P, d, c.shape[0], None)
        return labels, dist2

    def kmeans_accumulate(self, x, labels, k):
        P, d = x.shape
        sums, counts = np.empty((k, d), f64), np.empty(k, np.int64)
        self._run("kmeans_accumulate", x, labels, sums, counts, P, d, k, None, 0, None)
        return sums, counts

    def col_moments(self, x):
        rows, cols = x.shape
        mean, var = np.empty(cols, f64), np.empty(cols, f64)
        self._run("col_moments", x, mean, var, rows, cols, None, 0, None)
        return mean, var

    def affine_cols(self, x, sc, sh):
        y = x.copy()
        self._run("affine_cols_inplace", y, sc, sh, x.shape[0], x.shape[1], None)
        return y

    def upsample_tokens(self, x, g, R):
        M, n, Cc = x.shape
        out = np.empty((M, R * R, Cc), f32)
        self._run("upsample_bilinear_tokens", x, out, M, g, Cc, R, None)
        return out

    def _argmax(self, name, maps, g, R):
        M, n, K = maps.shape
        out = np.full((M, R, R), -1, np.int64)
        self._run(name, maps, out, M, g, K, R, None)
        return out

    def upsample_argmax_f32(self, maps, g, R):
        return self._argmax("upsample_argmax_f32", maps, g, R)

    def upsample_argmax(self, maps, g, R):
        return self._argmax("upsample_argmax", maps, g, R)

    def confusion_counts(self, pred, gt, Cn):
        counts = np.empty((Cn, Cn), np.uint64)
        self._run("confusion_counts", pred, gt, pred.size, Cn, counts, None)
        return counts.astype(np.int64)

    def _table(self, ents):
        tab = (self._lib.AdamwTensor * len(ents))()
        for j, e in enumerate(ents):
            tab[j] = self._lib.AdamwTensor(*[None if e.get(k_) is None else e[k_].ctypes.data for k_ in "pgmv"], e["g"].size, float(e.get("lr", 0.0)),
                                           float(e.get("wd", 0.0)))
        return tab

    def scale_tensors(self, grads, scale):
        out = [g.copy() for g in grads]
        self._run("scale_tensors", self._table([dict(g=g) for g in out]), len(out), np.array([scale], f32), None)
        return out

    def adamw(self, ents, step, fused=None):
        """ents: dicts of p, g, m, v (arrays), lr, wd -> updated copies; ``fused``: dict(proto=index of the prototypes' entry, K, dim, teacher,
        student, teacher_proto, momentum) runs tt_adamw_ema_step and also returns the teacher buffers."""
        ents = [dict(e, p=e["p"].copy(), m=e["m"].copy(), v=e["v"].copy()) for e in ents]
        tab = self._table(ents)
        if fused is None:
            self._run("adamw_step", tab, len(ents), step, 0.9, 0.999, 1e-8, None)
            return ents, None
        t, tp = fused["teacher"].copy(), fused["teacher_proto"].copy()
        self._run("adamw_ema_step", tab, len(ents), step, 0.9, 0.999, 1e-8, ents[fused["proto"]]["p"], fused["K"], fused["dim"], t, fused["student"],
                  t.size, tp, fused["momentum"], None)
        return ents, (t, tp)

    def ema_update(self, t, s, m):
        t = t.copy()
        self._run("ema_update", t, s, t.size, m, None)
        return t

    def add(self, a, b):
        a = a.copy()
        self._run("add_inplace", a, b, a.size, None)
        return a

    def count_mismatch(self, a, b):
        out = np.zeros(1, np.int64)
        self._run("count_mismatch", a, b, a.size, out, None)
        return int(out[0])

    def colsum(self, a):
        out = np.empty(a.shape[1], f32)
        self._run("colsum", a, out, a.shape[0], a.shape[1], None, 0, None)
        return out

    def normalize_rows(self, w):
        w = w.copy()
        self._run("normalize_rows_inplace", w, w.shape[0], w.shape[1], None)
        return w

    def scale_rows(self, x, s):
        x = x.copy()
        self._run("scale_rows_inplace", x, s, x.shape[0], x.shape[1], None)
        return x

    def foreground_mask(self, qkv, H, g, th):
        Fr, N, D3 = qkv.shape
        hd = D3 // 3 // H
        mask, blur, margin = (np.empty((Fr, N - 1), f32) for _ in range(3))
        self._run("foreground_mask", qkv, mask, blur, margin, Fr, N, H, hd, g, float(hd) ** -0.5, th, 0.6, 7, None)
        return mask, blur, margin

    def foreground_mask_from_probs(self, probs, g, th):
        Fr, H, N = probs.shape
        mask, blur, margin = (np.empty((Fr, N - 1), f32) for _ in range(3))
        self._run("foreground_mask_from_probs", probs, mask, blur, margin, Fr, N, H, g, th, 0.6, 7, None)
        return mask, blur, margin

    def pos_embed(self, pos, g, gh, gw):
        D = pos.shape[1]
        out = np.empty((1 + gh * gw, D), f32)
        self._run("pos_embed_interpolate", pos, out, g, gh, gw, D, (gh + 0.1) / g, (gw + 0.1) / g, None)
        return out


class HipSide:
    """The HIP library through the timetuning_amd.hip_ops wrappers on cuda:0 (NumPy in, NumPy out)."""
    name = "hip"

    def __init__(self):
        from timetuning_amd import _lib, hip_ops

        self.ops, self._lib = hip_ops, _lib

    @staticmethod
    def _d(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    @staticmethod
    def _h(t):
        return t.cpu().numpy()

    def kmeans_assign(self, x, c):
        # (the raw entry, on labels pre-filled with -1: a point the launch leaves unwritten is seen)
        P, d = x.shape
        xd, cd = self._d(x), self._d(c)
        # (the three kernels compute the same bits, so only the route query can tell that the dispatch is the documented one)
        assert self._lib.load().tt_kmeans_assign_route(d) == (16 if d <= 16 else (64 if d <= 64 else 0))
        labels = torch.full((P,), -1, dtype=torch.int32, device="cuda")
        dist2 = torch.full((P,), -1.0, dtype=torch.float32, device="cuda")
        self._lib.check(self._lib.load().tt_kmeans_assign(xd.data_ptr(), cd.data_ptr(), labels.data_ptr(), dist2.data_ptr(), P, d, c.shape[0],
                                                         torch.cuda.current_stream().cuda_stream), "tt_kmeans_assign")
        l2 = self.ops.kmeans_assign(xd, cd)           # the wrapper, without distances: the same labels
        assert torch.equal(l2, labels)
        return self._h(labels), self._h(dist2)

    def kmeans_accumulate(self, x, labels, k):
        xd, ld = self._d(x), self._d(labels)
        sums, counts = self.ops.kmeans_accumulate(xd, ld, k)
        s2, c2 = self.ops.kmeans_accumulate(xd, ld, k)
        assert torch.equal(s2, sums) and torch.equal(c2, counts)               # deterministic: fixed summation order, no float atomics
        return self._h(sums), self._h(counts)

    def col_moments(self, x):
        return tuple(self._h(t) for t in self.ops.col_moments(self._d(x)))

    def affine_cols(self, x, sc, sh):
        return self._h(self.ops.affine_cols_(self._d(x), self._d(sc), self._d(sh)))

    def upsample_tokens(self, x, g, R):
        return self._h(self.ops.upsample_bilinear_tokens(self._d(x), R))

    def upsample_argmax_f32(self, maps, g, R):
        return self._h(self.ops.upsample_argmax_f32(self._d(maps), R))

    def upsample_argmax(self, maps, g, R):
        return self._h(self.ops.upsample_argmax(self._d(maps), R))

    def confusion_counts(self, pred, gt, Cn):
        return self._h(self.ops.confusion_counts(self._d(pred), self._d(gt), Cn))

    def scale_tensors(self, grads, scale):
        out = [self._d(g) for g in grads]
        self.ops.scale_tensors_(out, torch.tensor([scale], dtype=torch.float32, device="cuda"))
        return [self._h(g) for g in out]

    def adamw(self, ents, step, fused=None):
        dev = [dict(e, **{k_: self._d(e[k_]) for k_ in "pgmv"}) for e in ents]
        tup = [(e["p"], e["g"], e["m"], e["v"], e["lr"], e["wd"]) for e in dev]
        back = lambda: [dict(e, **{k_: self._h(e[k_]) for k_ in "pmv"}) for e in dev]
        if fused is None:
            self.ops.adamw_step_(tup, step)
            return back(), None
        t, s, tp = self._d(fused["teacher"]), self._d(fused["student"]), self._d(fused["teacher_proto"])
        self.ops.adamw_ema_step_(tup, step, prototypes=dev[fused["proto"]]["p"].view(fused["K"], fused["dim"]), teacher_flat=t, student_flat=s,
                                 teacher_prototypes=tp, momentum=fused["momentum"])
        return back(), (self._h(t), self._h(tp))

    def ema_update(self, t, s, m):
        return self._h(self.ops.ema_update_(self._d(t), self._d(s), m))

    def add(self, a, b):
        return self._h(self.ops.add_(self._d(a), self._d(b)))

    def count_mismatch(self, a, b):
        return self.ops.count_mismatch(self._d(a), self._d(b))

    def colsum(self, a):
        return self._h(self.ops.colsum(self._d(a)))

    def normalize_rows(self, w):
        return self._h(self.ops.normalize_rows_(self._d(w)))

    def scale_rows(self, x, s):
        return self._h(self.ops.scale_rows_(self._d(x), self._d(s)))

    def foreground_mask(self, qkv, H, g, th):
        return tuple(self._h(t) for t in self.ops.foreground_mask(self._d(qkv), H, g, threshold=th, return_aux=True))

    def foreground_mask_from_probs(self, probs, g, th):
        return tuple(self._h(t) for t in self.ops.foreground_mask_from_probs(self._d(probs), g, threshold=th, return_aux=True))

    def pos_embed(self, pos, g, gh, gw):
        return self._h(self.ops.pos_embed_interpolate(self._d(pos), gh, gw))


_TWIN = None
HOST_WORST: dict = {}      # the host halves' worst errors (tests/test_sweep_eval_host.py, tests/test_sweep_prop_host.py, tests/test_sweep_head_host.py, tests/test_sweep_metric_host.py): one TT_SWEEP_REPORT_HOST file


def twin_side():
    global _TWIN
    if _TWIN is None:
        _TWIN = TwinSide()
    return _TWIN


# ---- k-means ---------------------------------------------------------------------------------------------------------------------------------

def km_inputs(rng, P, d, k, dup=0):
    """Standard-normal points, centroids 0.5 * x[random rows]; ``dup``: one centroid repeated at a higher index. -> x, c, (lo, hi) or None"""
    x = _normal(rng, P, d)
    rows = rng.choice(P, k, replace=False) if k <= P else rng.integers(0, P, k)
    c = (0.5 * x[rows]).astype(f32)
    pair = None
    if dup and k > 1:
        lo = int(rng.integers(0, k - 1))
        hi = int(rng.integers(lo + 1, k))
        c[hi] = c[lo]
        pair = (lo, hi)
    return x, c, pair


def km_reference(x, c, block_elems=1 << 22):
    """fp64 arg-min (first minimum), the least and the second-least squared distance per point, in blocks of rows."""
    P, k = x.shape[0], c.shape[0]
    c64 = c.astype(f64)
    cn = (c64 * c64).sum(1)
    want, best, second = np.empty(P, np.int64), np.empty(P, f64), np.full(P, np.inf)
    direct = x.shape[1] * k <= 4096
    step = max(1, block_elems // (k * x.shape[1] if direct else k))
    for r0 in range(0, P, step):
        xb = x[r0:r0 + step].astype(f64)
        if direct:    # small: the differences themselves
            d2 = ((xb[:, None, :] - c64[None]) ** 2).sum(-1)
        else:
            d2 = np.maximum((xb * xb).sum(1)[:, None] - 2.0 * (xb @ c64.T) + cn[None], 0.0)
        w = d2.argmin(1)
        want[r0:r0 + step] = w
        best[r0:r0 + step] = d2[np.arange(len(w)), w]
        if k > 1:
            second[r0:r0 + step] = np.partition(d2, 1, axis=1)[:, 1]
    return want, best, second


def check_kmeans_assign(side, p, rng, note):
    P, d, k = p["P"], p["d"], p["k"]
    x, c, pair = km_inputs(rng, P, d, k, p["dup"])
    labels, dist2 = side.kmeans_assign(x, c)
    assert labels.min() >= 0 and labels.max() < k, "a point was left unwritten or labelled outside [0, k)"
    want, best, second = km_reference(x, c)
    mism = labels != want
    assert (second[mism] - best[mism] < KM_GAP * best[mism]).all(), "a label differs from the fp64 arg-min away from a near-tie"
    note("labels excused / allowed", int(mism.sum()), _excuse_cap(P), strict=True)
    note("dist2 max", rel_err(dist2, best), TOL_KM)
    if side.name != "twin":   # the twin sums in the kernel's order: away from near-ties its labels are the kernel's
        clear = second - best >= KM_GAP * best
        assert np.array_equal(labels[clear], twin_side().kmeans_assign(x, c)[0][clear])
    if pair is not None:      # the deliberate tie, exactly: equal distances, the lower index wins
        assert not (labels == pair[1]).any(), "the higher index of a duplicated centroid was chosen"
        assert (labels[want == pair[0]] == pair[0]).all()
    return labels


def check_kmeans_accumulate(side, p, rng, note):
    P, d, k, mode = p["P"], p["d"], p["k"], p["mode"]
    x = (_normal(rng, P, d) + f32(0.5)).astype(f32)
    labels = rng.integers(0, k, P).astype(np.int32)
    if mode == "one":
        labels[:] = k // 2
    elif mode == "skip" and k > 1:
        skip = int(rng.integers(0, k))
        labels[labels == skip] = (skip + 1) % k
    sums, counts = side.kmeans_accumulate(x, labels, k)
    want_counts = np.bincount(labels, minlength=k)
    assert np.array_equal(counts, want_counts)
    want = np.zeros((k, d), f64)
    for t in range(d):     # column by column: no P x d fp64 temporary
        want[:, t] = np.bincount(labels, weights=x[:, t].astype(f64), minlength=k)
    note("sums max", rel_err(sums, want), TOL_KM)
    assert (sums[want_counts == 0] == 0).all()          # an empty cluster has an exactly zero sum
    if side.name != "twin":     # integer output: equal to the twin's
        assert np.array_equal(counts, twin_side().kmeans_accumulate(x, labels, k)[1])


# ---- column moments and the scaler's affine map ------------------------------------------------------------------------------------------------

def check_col_moments(side, p, rng, note):
    rows, cols, kind = p["rows"], p["cols"], p["kind"]
    x = _normal(rng, rows, cols) * np.linspace(0.1, 3.0, cols, dtype=f32) + np.linspace(-2, 2, cols, dtype=f32)
    off = None
    if kind == "const_col":
        x[:, cols // 2] = f32(1.2345678)
    elif kind == "offset":     # mean 1e4, spread 1e-2, beside columns of unit scale
        off = 0
        x[:, off] = (1e4 + 1e-2 * rng.standard_normal(rows)).astype(f32)
    x = np.ascontiguousarray(x, f32)
    mean, var = side.col_moments(x)
    want_mean = np.array([x[:, c_].astype(f64).mean() for c_ in range(cols)])
    want_var = np.array([x[:, c_].astype(f64).var() for c_ in range(cols)])      # two passes in fp64
    note("mean max", rel_err(mean, want_mean), TOL_MEAN)
    note("var max", rel_err(var, want_var), TOL_VAR)
    assert (var >= 0).all()
    if rows == 1:
        assert (var == 0).all() and np.array_equal(mean, x[0].astype(f64))
    if off is not None and rows > 1:
        # ... and on that column ALONE, relative to its own variance (the max over columns above is scaled by the unit-scale ones): sums of
        # `rows` non-negative terms taken about a point within a few deviations of the mean carry at most rows * 2^-52 each, and the
        # subtraction of the squared shifted mean (up to 16 variances for a first row 4 deviations out) amplifies that by at most 16.  On the
        # raw values the same formula is (mean / deviation)^2 = 1e12 times worse in fp64, and useless in fp32.
        note("var of the mean-1e4 column, relative / (16 * rows * 2^-52)", abs(var[off] - want_var[off]) / want_var[off] / (16 * rows * 2.0 ** -52), 1.0)
    sc, sh = _normal(rng, cols), _normal(rng, cols)
    y = side.affine_cols(x, sc, sh)
    want_y = x.astype(f64) * sc.astype(f64) + sh.astype(f64)
    note("affine max", rel_err(y, want_y), TOL_EVAL)


# ---- bilinear resampling of token maps ------------------------------------------------------------------------------------------------------------

def _interp64(maps, g, R):
    """[M, g*g, C] -> fp64 [M, R*R, C]: F.interpolate(bilinear, align_corners=False) on the doubles"""
    M, n, Cc = maps.shape
    t = torch.from_numpy(maps).double().transpose(1, 2).reshape(M, Cc, g, g)
    return F.interpolate(t, size=(R, R), mode="bilinear", align_corners=False).reshape(M, Cc, R * R).transpose(1, 2)


def check_upsample_tokens(side, p, rng, note):
    M, g, R, Cc = p["M"], p["g"], p["R"], p["C"]
    x = _normal(rng, M, g * g, Cc)
    got = side.upsample_tokens(x, g, R)
    note("max", rel_err(got, _interp64(x, g, R).numpy()), TOL_EVAL)


def _check_argmax(side, p, rng, note, dtype):
    M, g, R, K = p["M"], p["g"], p["R"], p["K"]
    maps = rng.standard_normal((M, g * g, K)).astype(dtype)
    got = (side.upsample_argmax if dtype == f64 else side.upsample_argmax_f32)(maps, g, R).reshape(M, R * R)
    assert got.min() >= 0 and got.max() < K
    up = _interp64(maps, g, R)
    top = torch.topk(up, min(2, K), dim=-1)
    want, best = top.indices[..., 0].numpy(), top.values[..., 0].numpy()
    second = top.values[..., 1].numpy() if K > 1 else np.full_like(best, -np.inf)
    mism = got != want
    if dtype == f64:
        gap = np.full_like(best, ARGMAX_GAP)
    else:      # four products and three sums in fp32: 4 ulps of the larger value
        gap = 4.0 * np.spacing(np.abs(best).astype(f32)).astype(f64)
    assert (best[mism] - second[mism] <= gap[mism]).all(), "a label differs from the fp64 arg-max away from a near-tie"
    note("labels excused / allowed", int(mism.sum()), _excuse_cap(M * R * R), strict=True)


def check_upsample_argmax_f32(side, p, rng, note):
    _check_argmax(side, p, rng, note, f32)


def check_upsample_argmax(side, p, rng, note):
    _check_argmax(side, p, rng, note, f64)


# ---- confusion counts ---------------------------------------------------------------------------------------------------------------------------

def check_confusion_counts(side, p, rng, note):
    n, Cn = p["n"], p["C"]
    pred, gt = rng.integers(0, Cn, n).astype(np.int64), rng.integers(0, Cn, n).astype(np.int64)
    if p["stray"]:      # ignored pixels: -1 and 255 in either input (255 is a class of its own when C > 255)
        for a in (pred, gt):
            idx = rng.integers(0, n, max(1, n // 7))
            a[idx] = np.where(rng.random(idx.size) < 0.5, -1, 255)
    ok = (pred >= 0) & (pred < Cn) & (gt >= 0) & (gt < Cn)
    want = np.bincount(gt[ok] * Cn + pred[ok], minlength=Cn * Cn).reshape(Cn, Cn)
    got = side.confusion_counts(pred, gt, Cn)
    assert np.array_equal(got, want)
    if side.name != "twin":
        assert np.array_equal(got, twin_side().confusion_counts(pred, gt, Cn))


# ---- AdamW, the gradient scale, the fused step -------------------------------------------------------------------------------------------------------

ADAMW_LENGTHS = (1, 255, 257)
ADAMW_HYPER = ((1e-3, 0.04), (1e-4, 0.0), (5e-5, 0.4), (2e-3, 0.0))
PROTO_K, PROTO_DIM, N_FLAT, EMA_M = 7, 32, 1003, 0.9951234567


def adamw_lengths(T, big):
    """Lengths 1, 255, 257, big, 1, ... (one tensor: big): a length-1 tensor comes FIRST and shares the table - and the grid, which is sized
    by the longest entry - with `big`."""
    cyc = ADAMW_LENGTHS + (big,)
    return [cyc[i % 4] for i in range(T)] if T > 1 else [big]


def _adamw_ref(ents, step):
    # (the hyper-parameters cross the C ABI as floats: the reference takes the values the kernel is given)
    ps = [torch.nn.Parameter(torch.from_numpy(e["p"]).double()) for e in ents]
    opt = torch.optim.AdamW([dict(params=[q], lr=float(f32(e["lr"])), weight_decay=float(f32(e["wd"]))) for q, e in zip(ps, ents)], betas=(float(f32(0.9)), float(f32(0.999))),
                            eps=float(f32(1e-8)))
    for q, e in zip(ps, ents):
        q.grad = torch.from_numpy(e["g"]).double()
        opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(e["m"]).double(), exp_avg_sq=torch.from_numpy(e["v"]).double())
    opt.step()
    return [(q.detach().numpy(), opt.state[q]["exp_avg"].numpy(), opt.state[q]["exp_avg_sq"].numpy()) for q in ps]


def _adamw_errs(got, ref):
    return {k_: max(rel_err(e[k_], r[i]) for e, r in zip(got, ref)) for i, k_ in enumerate("pmv")}


def check_adamw(side, p, rng, note):
    T, step, fused = p["T"], p["step"], p["fused"]
    lengths = adamw_lengths(T, p["big"])
    if fused:      # the prototypes [PROTO_K, PROTO_DIM] ride as one more entry behind the T tensors
        lengths.append(PROTO_K * PROTO_DIM)
    ents = []
    for i, n in enumerate(lengths):
        lr, wd = ADAMW_HYPER[i % len(ADAMW_HYPER)]
        ents.append(dict(p=_normal(rng, n), g=_normal(rng, n), m=_normal(rng, n, scale=0.1), v=_normal(rng, n, scale=0.1) ** 2, lr=lr, wd=wd))
    # the incoming gradient of the loss first (loss.backward()'s chain rule on the gradients the fused step holds): one fp32 product each
    scaled = side.scale_tensors([e["g"] for e in ents], p["gscale"])
    for e, g in zip(ents, scaled):
        assert np.array_equal(g, e["g"] * f32(p["gscale"]))
        e["g"] = g
    fz = None
    if fused:
        fz = dict(proto=T, K=PROTO_K, dim=PROTO_DIM, teacher=_normal(rng, N_FLAT), student=_normal(rng, N_FLAT),
                  teacher_proto=_normal(rng, PROTO_K, PROTO_DIM), momentum=EMA_M)
    got, teach = side.adamw(ents, step, fz)
    ref = _adamw_ref(ents, step)
    tol = TOL_EVAL
    if step >= 1000:      # bias corrections at 1 - beta^step ~ 1: 4 x the fp32 twin's own error on this case, never below the bound
        tw, _ = twin_side().adamw(ents, step, None)
        tol = max(TOL_EVAL, 4.0 * max(_adamw_errs(tw, ref).values()))
    if fused:             # normalize_prototypes() after optimizer.step(); the EMA teacher (oracle/timet_oracle.py: update_momentum_teacher)
        pr = torch.from_numpy(ref[-1][0]).reshape(PROTO_K, PROTO_DIM)
        prn = F.normalize(pr, dim=1, p=2)
        note("prototypes max", rel_err(got[-1]["p"].reshape(PROTO_K, PROTO_DIM), prn.numpy()), max(tol, TOL_L2N))
        note("teacher max", rel_err(teach[0], fz["teacher"].astype(f64) * (1.0 - EMA_M) + fz["student"].astype(f64) * EMA_M), TOL_EVAL)
        tpr = F.normalize(torch.from_numpy(fz["teacher_proto"]).double() * (1.0 - EMA_M) + prn * EMA_M, dim=1, p=2)
        note("teacher prototypes max", rel_err(teach[1], tpr.numpy()), max(tol, TOL_L2N))
        got, ref = got[:-1], ref[:-1]
    if got:
        for k_, err in _adamw_errs(got, ref).items():
            note(f"{k_} max" + (" (step >= 1000)" if step >= 1000 else ""), err, tol)


# ---- element-wise and row ops ---------------------------------------------------------------------------------------------------------------------

def check_elementwise(side, p, rng, note):
    n, rows, cols = p["n"], p["rows"], p["cols"]
    t, s = _normal(rng, n), _normal(rng, n)
    note("ema max", rel_err(side.ema_update(t, s, EMA_M), t.astype(f64) * (1.0 - EMA_M) + s.astype(f64) * EMA_M), TOL_EVAL)
    assert np.array_equal(side.add(t, s), t + s)                      # one fp32 sum per element: the same bits
    # tt_count_mismatch compares BIT PATTERNS: +0 and -0 differ, NaNs of different payload differ, a NaN equals itself
    a = t.copy()
    a[rng.integers(0, n, max(1, n // 50))] = 0.0
    nan_pos = rng.integers(0, n, max(1, n // 50))
    a.view(np.uint32)[nan_pos] = 0x7FC00001
    b = a.copy()
    flip, zneg, npay = (rng.random(n) < 0.01), (a == 0) & (rng.random(n) < 0.5), np.zeros(n, bool)
    npay[nan_pos[::2]] = True
    b[flip] = b[flip] + f32(1.0)
    b[zneg] = f32(-0.0)
    b.view(np.uint32)[npay] = 0x7FC00002
    want = int((a.view(np.uint32) != b.view(np.uint32)).sum())
    assert want >= int(zneg.sum()) + int(npay.sum())
    assert side.count_mismatch(a, b) == want and side.count_mismatch(a, a) == 0
    x = _normal(rng, rows, cols)
    note("colsum max", rel_err(side.colsum(x), x.astype(f64).sum(0)), TOL_EVAL)
    xn = x.astype(f64)
    xn = xn / np.maximum(np.sqrt((xn * xn).sum(1, keepdims=True)), 1e-12)        # F.normalize
    note("normalize_rows max", rel_err(side.normalize_rows(x), xn), TOL_L2N)
    c4 = (cols + 3) // 4 * 4
    x4, w = _normal(rng, rows, c4), _normal(rng, rows)
    assert np.array_equal(side.scale_rows(x4, w), x4 * w[:, None])


# ---- the attention foreground mask ------------------------------------------------------------------------------------------------------------------

def check_foreground_mask(side, p, rng, note):
    from oracle import timet_oracle as O

    Fr, g, H, hd, th = p["F"], p["g"], p["H"], p["hd"], p["th"]
    N, D = g * g + 1, H * hd
    if p["entry"] == "qkv":      # q . k / sqrt(hd) of standard deviation 1.5, as the probabilities below
        qkv = _normal(rng, Fr, N, 3 * D, scale=1.5 ** 0.5)
        q0 = torch.from_numpy(qkv[:, 0, :D]).double().reshape(Fr, H, 1, hd)
        k = torch.from_numpy(qkv[:, :, D:2 * D]).double().reshape(Fr, N, H, hd).permute(0, 2, 3, 1)
        probs = torch.softmax((q0 @ k) * hd ** -0.5, -1).float()                  # [F, H, 1, N]
        mask, blur, margin = side.foreground_mask(qkv, H, g, th)
    else:
        probs = torch.softmax(1.5 * torch.from_numpy(_normal(rng, Fr, H, 1, N)).double(), -1).float()
        mask, blur, margin = side.foreground_mask_from_probs(np.ascontiguousarray(probs[:, :, 0].numpy()), g, th)
    want, want_blur, _ = O.process_attentions(probs, g, threshold=th, return_blurred=True)   # (reads row 0 of the attention only)
    want = want.reshape(Fr, -1)
    note("blurred max", rel_err(blur, want_blur.numpy()), TOL_BLUR)
    mask, margin = torch.from_numpy(mask), torch.from_numpy(margin)
    assert ((mask == 0) | (mask == 1)).all()
    note("excusable region / pixels", float(mask_excusable_region(margin).float().mean()), MASK_REGION_CAP, strict=True)
    assert mask_mismatch_excusable(mask, want, margin)
    note("mask mismatch share", float((mask != want).float().mean()), MASK_REGION_CAP, strict=True)


# ---- the bicubic position table ------------------------------------------------------------------------------------------------------------------------

def check_pos_embed(side, p, rng, note):
    from oracle import timet_oracle as O

    g, gh, gw, D = p["g"], p["gh"], p["gw"], p["D"]
    pos = _normal(rng, 1 + g * g, D)
    got = side.pos_embed(pos, g, gh, gw)
    ref = O.interpolate_pos_encoding(torch.from_numpy(pos).double()[None], gh * gw, gh * 16, gw * 16, 16)[0].numpy()
    assert got.shape == ref.shape and np.array_equal(got[0], pos[0])          # the class position is copied
    note("max", rel_err(got[1:], ref[1:]), TOL_POS)


CHECK = {"kmeans_assign": check_kmeans_assign, "kmeans_accumulate": check_kmeans_accumulate, "col_moments": check_col_moments,
         "upsample_tokens": check_upsample_tokens, "upsample_argmax_f32": check_upsample_argmax_f32, "upsample_argmax": check_upsample_argmax,
         "confusion_counts": check_confusion_counts, "adamw": check_adamw, "elementwise": check_elementwise,
         "foreground_mask": check_foreground_mask, "pos_embed": check_pos_embed}


def make_note(worst: dict, op: str):
    """note(what, err, tol): records the worst ``err`` under "op: what" with its bound and asserts err < tol (``strict``: err <= tol)."""
    def note(what, err, tol, strict=False):
        key = f"{op}: {what}"
        w = worst.setdefault(key, [0.0, tol])
        w[0], w[1] = max(w[0], err), max(w[1], tol)
        assert (err < tol) if not strict else (err <= tol), (key, err, tol)
    return note


def run_eval_case(side, op: str, params: dict, worst: dict) -> None:
    CHECK[op](side, params, case_rng(op, params), make_note(worst, op))
