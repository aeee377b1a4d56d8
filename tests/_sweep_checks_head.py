"""The checks of the sweep's fourth tier (tests/_sweep_cases.py, HEAD_OPS): the linear probe's kernels against fp64 references and the clip
input pipeline bit for bit against the Pillow-pinned oracle (oracle/image_ops.py).

One check per op, written once and run on two sides, as the second tier's (tests/_sweep_checks_eval.py): ``HeadTwin`` - the plain-C twins of
oracle/tt_cpu.c on host buffers (tests/test_sweep_head_host.py, no GPU) - and ``HeadHip`` - the HIP library through timetuning_amd.hip_ops
and timetuning_amd.video_transformations on cuda:0 (tests/test_hip_sweep.py).  Both build the same inputs (seeded by the case id) and the same
reference and assert the same bounds.

Bounds are the ones tests/test_hip_linear_probe.py holds: 1e-6 max-normalised for the logits, the adjoint, dW and db, 1e-5 for the CE loss
(relative) and its gradient, 1e-6 for SGD.  Three regimes cannot be expected to keep them and take the sweep's rule instead - 4 x the error of
the fp32 twin against fp64 ON THAT CASE, never below the existing bound:
  * tt_probe_wgrad where one workgroup sums WGRAD_LONG_RUN (512) rows or more in one fp32 accumulator.  The existing bound was set at
    runs of 288 rows (47 040 rows of D 384, C 21); the rounding error of a sequential fp32 sum grows with the square root of its length.
  * tt_bilinear_adjoint_tokens from R = 16 g on: a token gathers (2 R / g)^2 >= ADJOINT_LONG_RUN (1024) mask pixels in one fp32
    accumulator.  The existing bound was set at that ratio on 2 x 14 x 14 x 5 outputs; 64 x 64 tokens are four times as many draws
    of the same error distribution, and the fp32 twin's own worst is 1.08e-6 there.
  * tt_probe_upsample_ce on saturated logits (``kind = large``, sigma 30): a loss of tens of units carries an absolute error of fp32
    spacing at that size times the rounding of the four-tap interpolation of logits near 100.
With C = 1 the loss is exactly 0 in the reference and is compared absolutely: |loss| <= 4 * 2^-23 * max|logits| (the two evaluations of
the one logit may round differently); its gradient softmax - 1 = exp(0) / exp(0) - 1 is an exact zero in any IEEE arithmetic.
The image ops have no tolerance at all.  Nothing here has an arg-max, so there is no excuse rule."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from _sweep_cases import ADJOINT_LONG_RUN, IMG_MODES, WGRAD_LONG_RUN, adjoint_run, sgd_lengths, wgrad_split
from _sweep_checks_eval import _normal, case_rng, make_note, rel_err

f32, f64 = np.float32, np.float64
TOL_PROBE = 1e-6       # logits, adjoint, dW, db (tests/test_hip_linear_probe.py)
TOL_CE = 1e-5          # CE loss (relative) and gradient (max-normalised)
TOL_SGD = 1e-6
CE_PROOF_MAX = 1 << 22  # R * R * C up to which the host half proves the explicit reference against torch autograd
MEAN, STD = [0.485, 0.456, 0.406], [0.228, 0.224, 0.225]
SGD_LR = (0.01, 0.1, 0.003)
BAD_LABELS = (None, -1, 1 << 40)      # (None: the class count itself)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the two sides ---------------------------------------------------------------------------------------------------------------------------

class HeadTwin:
    """oracle/tt_cpu.c on host buffers (NumPy in, NumPy out); the resize taps are the oracle's (oracle/image_ops.py)."""
    name = "twin"

    def __init__(self):
        from oracle import cpu_twin, image_ops
        from timetuning_amd import _lib

        self.lib, self._lib, self.I = cpu_twin.load(), _lib, image_ops

    def call(self, name, *args):
        return getattr(self.lib, "tt_cpu_" + name)(*[_ptr(a) if isinstance(a, np.ndarray) else a for a in args])

    def _run(self, name, *args):
        rc = self.call(name, *args)
        assert rc == 0, (name, rc)

    def probe_logits(self, x, w, b):
        out = np.full((x.shape[0], w.shape[0]), np.nan, f32)
        self._run("probe_logits", x, w, b, out, x.shape[0], x.shape[1], w.shape[0], None)
        return out

    def probe_upsample_ce(self, low, labels):
        B, n, Cc = low.shape
        g, R = int(round(n ** 0.5)), labels.shape[1]
        dlow, loss, counts = np.full_like(low, np.nan), np.zeros(1, f32), np.full(2, -1, np.int64)
        self._run("probe_upsample_ce", low, labels, dlow, loss, counts, B, g, Cc, R, None, 0, None)
        return loss, dlow, counts

    def bilinear_adjoint(self, d_hi, g):
        B, m, Cc = d_hi.shape
        out = np.full((B, g * g, Cc), np.nan, f32)
        self._run("bilinear_adjoint_tokens", d_hi, out, B, g, Cc, int(round(m ** 0.5)), None)
        return out

    def upsample_tokens(self, x, g, R):
        M, n, Cc = x.shape
        out = np.empty((M, R * R, Cc), f32)
        self._run("upsample_bilinear_tokens", x, out, M, g, Cc, R, None)
        return out

    def probe_wgrad(self, dl, x, scale, need_bias):
        rows, Cc = dl.shape
        dw, db = np.full((Cc, x.shape[1]), np.nan, f32), (np.full(Cc, np.nan, f32) if need_bias else None)
        self._run("probe_wgrad", dl, x, scale, dw, db, rows, x.shape[1], Cc, None, 0, None)
        return dw, db

    def sgd(self, ents, grads, momentum):
        """ents: dicts of p, m (arrays), lr, wd; grads[step][tensor] -> (params, buffers) after len(grads) steps, the first with first_step."""
        ps, ms = [e["p"].copy() for e in ents], [e["m"].copy() for e in ents]
        for step, gs in enumerate(grads):
            for i in range(0, len(ents), 40):       # TT_MAX_TENSORS per call, as hip_ops.sgd_step_ chunks
                idx = range(i, min(i + 40, len(ents)))
                tab = (self._lib.AdamwTensor * len(idx))()
                for j, t in enumerate(idx):
                    tab[j] = self._lib.AdamwTensor(ps[t].ctypes.data, gs[t].ctypes.data, ms[t].ctypes.data, None, ps[t].size, float(ents[t]["lr"]),
                                                   float(ents[t]["wd"]))
                self._run("sgd_step", tab, len(idx), float(momentum), int(step == 0), None)
        return ps, ms

    def resized_crop(self, frames, i, j, h, w, size, to_tensor, flip):
        # both passes always: where a side keeps its size the taps are the identity (one tap of 2^22)
        Fr, H, W, _ = frames.shape
        OH, OW = size
        kh, bh = self.I.resample_coeffs(w, OW)
        kv, bv = self.I.resample_coeffs(h, OH)
        mid = np.empty((Fr, h, OW, 3), np.uint8)
        self._run("img_resample_h", frames, mid, kh, bh, Fr, H, W, i, j, h, OW, kh.shape[1], None)
        if not to_tensor:
            out = np.empty((Fr, OH, OW, 3), np.uint8)
            self._run("img_resample_v", mid, out, None, kv, bv, Fr, h, OW, 0, OH, kv.shape[1], 0, None, None, None)
            return out
        out = np.empty((Fr, 3, OH, OW), f32)
        m3, s3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
        self._run("img_resample_v", mid, None, out, kv, bv, Fr, h, OW, 0, OH, kv.shape[1], int(flip), m3, s3, None)
        return out

    def img_color(self, frames, mode, factor, hue_shift):
        out = frames.copy()
        self._run("img_color", out, out.shape[0], out.shape[1], out.shape[2], mode, float(factor), int(hue_shift), None, None)
        return out

    def gaussian_blur(self, frames, radius):
        r, ww, fw = self.I.box_weights(self.I.gaussian_box_radius(radius))
        cur = frames
        for direction in (0, 1):
            for _ in range(3):
                nxt = np.empty_like(cur)
                self._run("img_box_blur", cur, nxt, cur.shape[0], cur.shape[1], cur.shape[2], direction, r, ww, fw, None)
                cur = nxt
        return cur


class HeadHip:
    """The HIP library through the hip_ops wrappers and the transforms of video_transformations on cuda:0 (NumPy in, NumPy out)."""
    name = "hip"

    def __init__(self):
        from timetuning_amd import hip_ops, video_transformations

        self.ops, self.VT = hip_ops, video_transformations

    @staticmethod
    def _d(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    @staticmethod
    def _h(t):
        return None if t is None else t.cpu().numpy()

    def probe_logits(self, x, w, b):
        return self._h(self.ops.probe_logits(self._d(x), self._d(w), self._d(b)))

    def probe_upsample_ce(self, low, labels):
        return tuple(self._h(t) for t in self.ops.probe_upsample_ce(self._d(low), self._d(labels)))

    def bilinear_adjoint(self, d_hi, g):
        return self._h(self.ops.bilinear_adjoint_tokens(self._d(d_hi), g))

    def upsample_tokens(self, x, g, R):
        return self._h(self.ops.upsample_bilinear_tokens(self._d(x), R))

    def probe_wgrad(self, dl, x, scale, need_bias):
        dw, db = self.ops.probe_wgrad(self._d(dl), self._d(x), self._d(scale), need_bias=bool(need_bias))
        return self._h(dw), self._h(db)

    def sgd(self, ents, grads, momentum):
        ps, ms = [self._d(e["p"]) for e in ents], [self._d(e["m"]) for e in ents]
        for step, gs in enumerate(grads):
            self.ops.sgd_step_([(p, self._d(g), m, e["lr"], e["wd"]) for p, g, m, e in zip(ps, gs, ms, ents)], momentum, first_step=step == 0)
        return [self._h(p) for p in ps], [self._h(m) for m in ms]

    def resized_crop(self, frames, i, j, h, w, size, to_tensor, flip):
        return self._h(self.VT.resized_crop(self._d(frames), i, j, h, w, size, to_tensor=(MEAN, STD) if to_tensor else None, flip=bool(flip)))

    def img_color(self, frames, mode, factor, hue_shift):
        return self._h(self.ops.img_color_(self._d(frames), mode, factor, hue_shift))

    def gaussian_blur(self, frames, radius):
        return self._h(self.VT.gaussian_blur(self._d(frames), radius))


_TWIN = None


def head_twin():
    global _TWIN
    if _TWIN is None:
        _TWIN = HeadTwin()
    return _TWIN


def _regime_tol(base, twin_err):
    """The sweep's rule for a regime that cannot be expected to hold ``base``: 4 x the fp32 twin's own error on the case, never below it."""
    return max(base, 4.0 * twin_err)


# ---- tt_probe_logits -----------------------------------------------------------------------------------------------------------------------------

def check_probe_logits(side, p, rng, note):
    rows, D, Cc = p["rows"], p["D"], p["C"]
    x, w = _normal(rng, rows, D), _normal(rng, Cc, D, scale=0.05)
    b = _normal(rng, Cc, scale=0.1) if p["bias"] else None
    got = side.probe_logits(x, w, b)
    ref = x.astype(f64) @ w.astype(f64).T + (b.astype(f64) if b is not None else 0.0)
    assert got.shape == ref.shape and np.isfinite(got).all()
    note("logits max", rel_err(got, ref), TOL_PROBE)


# ---- the bilinear rule (ATen, align_corners = False) on one axis, in fp64 -------------------------------------------------------------------------

def src_taps(g, R):
    """-> i0, i1, l1 (fp64) for the R output positions of a g-long axis: s = max(g / R * (o + 0.5) - 0.5, 0)"""
    s = np.maximum((g / R) * (np.arange(R, dtype=f64) + 0.5) - 0.5, 0.0)
    i0 = s.astype(np.int64)
    return i0, i0 + (i0 < g - 1), s - i0


def _interp64(low, g, R):
    B, n, Cc = low.shape
    return F.interpolate(low.permute(0, 2, 1).reshape(B, Cc, g, g), size=(R, R), mode="bilinear", align_corners=False)


# ---- tt_probe_upsample_ce -------------------------------------------------------------------------------------------------------------------------

def ce_inputs(p, rng):
    B, g, R, Cc, ignored, kind = p["B"], p["g"], p["R"], p["C"], p["ignored"], p["kind"]
    if kind == "const":
        low = np.full((B, g * g, Cc), 1.5, f32)
    else:
        low = _normal(rng, B, g * g, Cc, scale=30.0 if kind == "large" else 2.0)
    y = rng.integers(0, Cc, (B, R, R)).astype(np.int64)      # (at C = 256 the draws include 255: ignored, not a class)
    if ignored == "rows":           # the upper half of every mask: the workgroups of the low-res rows under it own no valid pixel
        y[:, :R // 2] = 255
    elif ignored >= 1.0:
        y[:] = 255
    elif ignored > 0:
        y[rng.random((B, R, R)) < ignored] = 255
        if y.size >= 8:             # labels outside [0, C) that are not 255: counted, never used as an index
            flat = y.reshape(-1)
            for pos, bad in zip(rng.choice(y.size, len(BAD_LABELS), replace=False), BAD_LABELS):
                flat[pos] = Cc if bad is None else bad
    return low, y


def ce_reference(low, y, g):
    """The explicit restatement in fp64 over the VALID pixels only: four-tap gather, log-sum-exp, (softmax - one-hot) / count scattered
    back onto the taps.  -> loss (NaN without a valid pixel), gradient [B, g*g, C], valid, invalid"""
    B, n, Cc = low.shape
    R = y.shape[1]
    ok = (y >= 0) & (y < Cc) & (y != 255)
    invalid = int(((y != 255) & ~ok).sum())
    bb, oy, ox = np.nonzero(ok)
    nv = bb.size
    grad = np.zeros((B * n, Cc), f64)
    if nv == 0:
        return float("nan"), grad.reshape(B, n, Cc), 0, invalid
    i0, i1, l1 = src_taps(g, R)
    low2 = low.reshape(B * n, Cc).astype(f64)
    total = 0.0
    step = max(1, (1 << 22) // Cc)
    for a in range(0, nv, step):
        sl = slice(a, a + step)
        b_, y_, x_ = bb[sl], oy[sl], ox[sl]
        ly, lx = l1[y_], l1[x_]
        taps = [(b_ * n + i0[y_] * g + i0[x_], (1 - ly) * (1 - lx)), (b_ * n + i0[y_] * g + i1[x_], (1 - ly) * lx),
                (b_ * n + i1[y_] * g + i0[x_], ly * (1 - lx)), (b_ * n + i1[y_] * g + i1[x_], ly * lx)]
        z = sum(w[:, None] * low2[t] for t, w in taps)
        top = z.max(1, keepdims=True)
        e = np.exp(z - top)
        s = e.sum(1, keepdims=True)
        lab = y[b_, y_, x_]
        total += float((np.log(s[:, 0]) + top[:, 0] - z[np.arange(len(lab)), lab]).sum())
        d = e / s
        d[np.arange(len(lab)), lab] -= 1.0
        d /= nv
        for t, w in taps:
            np.add.at(grad, t, w[:, None] * d)
    return total / nv, grad.reshape(B, n, Cc), nv, invalid


def ce_autograd(low, y, g):
    """F.interpolate + F.cross_entropy(ignore_index=255) and autograd in fp64; labels outside [0, C) play no part: they are given as 255."""
    Cc = low.shape[2]
    yt = torch.from_numpy(np.where((y >= 0) & (y < Cc), y, 255))
    l64 = torch.from_numpy(low).double().requires_grad_(True)
    loss = F.cross_entropy(_interp64(l64, g, y.shape[1]), yt, ignore_index=255)
    loss.backward()
    return float(loss.detach()), l64.grad.numpy()


def check_probe_upsample_ce(side, p, rng, note):
    g, R, Cc, kind = p["g"], p["R"], p["C"], p["kind"]
    low, y = ce_inputs(p, rng)
    loss, dlow, counts = side.probe_upsample_ce(low, y)
    loss2, dlow2, counts2 = side.probe_upsample_ce(low, y)
    assert np.array_equal(loss.view(np.int32), loss2.view(np.int32)) and np.array_equal(dlow.view(np.int32), dlow2.view(np.int32))   # run to run, NaN too
    want, grad, nv, ninv = ce_reference(low, y, g)
    if side.name == "twin" and R * R * Cc <= CE_PROOF_MAX:       # the restatement itself, against torch
        tl, tg = ce_autograd(low, y, g)
        if nv == 0:
            assert np.isnan(tl) and not np.abs(tg).max()
        else:
            assert abs(tl - want) <= 1e-12 * max(abs(tl), 1.0) and np.abs(tg - grad).max() <= 1e-12 * max(np.abs(tg).max(), 1e-300), (tl, want)
    assert (int(counts[0]), int(counts[1])) == (nv, ninv) and np.array_equal(counts, counts2)
    if p["ignored"] not in ("rows", 0.0) and p["ignored"] < 1.0 and y.size >= 8:
        assert ninv == len(BAD_LABELS)
    if nv == 0:
        assert np.isnan(loss).all() and not np.abs(dlow).max(), "no valid pixel: the loss is NaN and the gradient zero"
        return
    assert np.isfinite(loss).all() and np.isfinite(dlow).all()
    if kind == "const":
        assert abs(want - np.log(Cc)) <= 1e-12
    if Cc == 1:
        note("C = 1 |loss| / (4 * 2^-23 * max|logits|)", abs(float(loss[0])) / (4 * 2.0 ** -23 * float(np.abs(low).max())), 1.0, strict=True)
        assert not np.abs(dlow).max(), "one class: softmax - 1 is an exact zero"
        return
    tol_l = tol_g = TOL_CE
    tag = ""
    if kind == "large":
        tag = " (saturated)"
        if side.name == "twin":
            tw_l, tw_g = loss, dlow
        else:
            tw_l, tw_g, _ = head_twin().probe_upsample_ce(low, y)
        tol_l = _regime_tol(TOL_CE, abs(float(tw_l[0]) - want) / abs(want))
        tol_g = _regime_tol(TOL_CE, rel_err(tw_g, grad))
    note("loss rel" + tag, abs(float(loss[0]) - want) / abs(want), tol_l)
    note("dlogits max" + tag, rel_err(dlow, grad), tol_g)


# ---- tt_bilinear_adjoint_tokens ---------------------------------------------------------------------------------------------------------------------

def check_bilinear_adjoint(side, p, rng, note):
    B, g, R, Cc = p["B"], p["g"], p["R"], p["C"]
    d_hi = _normal(rng, B, R * R, Cc)
    got = side.bilinear_adjoint(d_hi, g)
    l64 = torch.zeros(B, g * g, Cc, dtype=torch.float64, requires_grad=True)
    (_interp64(l64, g, R) * torch.from_numpy(d_hi).double().view(B, R, R, Cc).permute(0, 3, 1, 2)).sum().backward()
    ref = l64.grad.numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()
    tol, tag = TOL_PROBE, ""
    if adjoint_run(g, R) >= ADJOINT_LONG_RUN:
        tag = f" (>= {ADJOINT_LONG_RUN} pixels per token)"
        tol = _regime_tol(TOL_PROBE, rel_err(got if side.name == "twin" else head_twin().bilinear_adjoint(d_hi, g), ref))
    note("d_low max" + tag, rel_err(got, ref), tol)
    # <up(x), y> = <x, adj(y)> with `up` the library's own up-sampling entry.  Element-wise errors of 1e-6 max-normalised in up(x) and in
    # adj(y) move the two sides by at most 1e-6 * (max|up| * |y|_1 + max|adj| * |x|_1): the identity is held to that, in fp64
    x = _normal(rng, B, g * g, Cc)
    up = side.upsample_tokens(x, g, R).astype(f64)
    lhs, rhs = float((up * d_hi.astype(f64)).sum()), float((x.astype(f64) * got.astype(f64)).sum())
    room = np.abs(up).max() * np.abs(d_hi.astype(f64)).sum() + np.abs(ref).max() * np.abs(x.astype(f64)).sum()
    note("dot-product identity |<up x, y> - <x, adj y>| / room", abs(lhs - rhs) / room, TOL_PROBE)


# ---- tt_probe_wgrad -----------------------------------------------------------------------------------------------------------------------------------

def check_probe_wgrad(side, p, rng, note):
    rows, D, Cc = p["rows"], p["D"], p["C"]
    dl, x = _normal(rng, rows, Cc), _normal(rng, rows, D)
    scale = np.array([p["scale"]], f32) if p["scale"] else None
    dw, db = side.probe_wgrad(dl, x, scale, p["need_bias"])
    s = float(scale[0]) if scale is not None else 1.0
    ref_w, ref_b = s * (dl.astype(f64).T @ x.astype(f64)), s * dl.astype(f64).sum(0)
    assert dw.shape == ref_w.shape and np.isfinite(dw).all() and (db is None) == (not p["need_bias"])
    tol_w = tol_b = TOL_PROBE
    tag = ""
    if wgrad_split(rows, D, Cc)[1] >= WGRAD_LONG_RUN:
        tag = f" (runs >= {WGRAD_LONG_RUN} rows)"
        tw, tb = (dw, db) if side.name == "twin" else head_twin().probe_wgrad(dl, x, scale, p["need_bias"])
        tol_w = _regime_tol(TOL_PROBE, rel_err(tw, ref_w))
        tol_b = _regime_tol(TOL_PROBE, rel_err(tb, ref_b)) if tb is not None else TOL_PROBE
    note("dw max" + tag, rel_err(dw, ref_w), tol_w)
    if db is not None:
        assert np.isfinite(db).all()
        note("db max" + tag, rel_err(db, ref_b), tol_b)


# ---- tt_sgd_step ------------------------------------------------------------------------------------------------------------------------------------------

def check_sgd(side, p, rng, note):
    T, steps, momentum, wd = p["T"], p["steps"], p["momentum"], p["wd"]
    lengths = sgd_lengths(T, p["big"])
    # (momentum buffers start as noise: the first step must overwrite them, not read them)
    ents = [dict(p=_normal(rng, n), m=_normal(rng, n, scale=0.1), lr=SGD_LR[i % len(SGD_LR)], wd=wd) for i, n in enumerate(lengths)]
    grads = [[_normal(rng, n) for n in lengths] for _ in range(steps)]
    ps, ms = side.sgd(ents, grads, momentum)
    # (the hyper-parameters cross the C ABI as floats: the reference takes the values the kernel is given)
    qs = [torch.nn.Parameter(torch.from_numpy(e["p"]).double()) for e in ents]
    opt = torch.optim.SGD([dict(params=[q], lr=float(f32(e["lr"])), weight_decay=float(f32(wd))) for q, e in zip(qs, ents)], lr=0.1,
                          momentum=float(f32(momentum)))
    for gs in grads:
        for q, g_ in zip(qs, gs):
            q.grad = torch.from_numpy(g_).double()
        opt.step()
    # One scale for the whole table: every tensor holds unit-normal values, and a one-element tensor has no maximum of its own to be
    # normalised by - buf = momentum * buf + d can cancel to almost nothing there, while its rounding error stays that of its operands.
    # So the error of any element is taken against the largest reference value of the table, and never against less than the largest
    # operand (the parameters before the steps; the last gradients).
    def table_err(got, ref, floor):
        return max(float(np.abs(a.astype(f64) - r).max()) for a, r in zip(got, ref)) / max(max(float(np.abs(r).max()) for r in ref), floor)

    note("params max", table_err(ps, [q.detach().numpy() for q in qs], max(float(np.abs(e["p"]).max()) for e in ents)), TOL_SGD)
    if momentum:
        note("momentum buffers max", table_err(ms, [opt.state[q]["momentum_buffer"].numpy() for q in qs], max(float(np.abs(g_).max()) for g_ in grads[-1])),
             TOL_SGD)
    else:      # no momentum: the buffers are not touched
        assert all(np.array_equal(m, e["m"]) for m, e in zip(ms, ents))


# ---- the clip input pipeline: bit equality with oracle/image_ops.py ---------------------------------------------------------------------------------

def _frames(rng, Fr, H, W):
    return rng.integers(0, 256, (Fr, H, W, 3), dtype=np.uint8)


def check_img_resize(side, p, rng, note):
    from oracle import image_ops as I

    Fr, h, w, oh, ow = p["F"], p["h"], p["w"], p["oh"], p["ow"]
    i, j, ch, cw = [int(v) for v in p["crop"].split("/")] if p["crop"] else (0, 0, h, w)
    assert 0 <= i and i + ch <= h and 0 <= j and j + cw <= w and ch > 0 and cw > 0
    a = _frames(rng, Fr, h, w)
    got = side.resized_crop(a, i, j, ch, cw, (oh, ow), p["to_tensor"], p["flip"])
    if p["to_tensor"]:
        want = np.stack([I.resized_crop_to_tensor(a[f], (i, j, ch, cw), (oh, ow), bool(p["flip"]), MEAN, STD) for f in range(Fr)])
        assert got.dtype == f32 and got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))
    else:
        want = np.stack([I.resize_bilinear(a[f][i:i + ch, j:j + cw], (ow, oh)) for f in range(Fr)])
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)


def color_frames(rng, Fr, H, W):
    """Frame f is drawn below 256 (f + 1) / F - every frame its own mean gray - and the last frame of two or more is exact grays."""
    a = np.stack([rng.integers(0, max(1, 256 * (f + 1) // Fr), (H, W, 3), dtype=np.uint8) for f in range(Fr)])
    if Fr >= 2:
        a[-1] = a[-1][:, :, :1]
    return a


def check_img_color(side, p, rng, note):
    from oracle import image_ops as I

    Fr, H, W, mode, factor = p["F"], p["H"], p["W"], p["mode"], p["factor"]
    a = color_frames(rng, Fr, H, W)
    shift = I.hue_shift_u8(factor) if mode == "hue" else 0
    got = side.img_color(a, IMG_MODES.index(mode), 1.0 if mode == "hue" else factor, shift)
    fn = {"gray": lambda x: I.gray3(x), "brightness": lambda x: I.enhance_brightness(x, factor), "contrast": lambda x: I.enhance_contrast(x, factor),
          "saturation": lambda x: I.enhance_saturation(x, factor), "hue": lambda x: I.adjust_hue(x, factor)}[mode]
    want = np.stack([fn(a[f]) for f in range(Fr)])
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)


def check_img_blur(side, p, rng, note):
    from oracle import image_ops as I

    a = _frames(rng, p["F"], p["H"], p["W"])
    got = side.gaussian_blur(a, p["radius"])
    want = np.stack([I.gaussian_blur(a[f], p["radius"]) for f in range(p["F"])])
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)


CHECK = {"probe_logits": check_probe_logits, "probe_upsample_ce": check_probe_upsample_ce, "bilinear_adjoint": check_bilinear_adjoint,
         "probe_wgrad": check_probe_wgrad, "sgd": check_sgd, "img_resize": check_img_resize, "img_color": check_img_color,
         "img_blur": check_img_blur}


def run_head_case(side, op: str, params: dict, worst: dict) -> None:
    CHECK[op](side, params, case_rng(op, params), make_note(worst, op))
