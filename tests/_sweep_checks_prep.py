"""The checks of the sweep's sixth tier (tests/_sweep_cases.py, PREP_OPS): the operand-preparation kernels of gemm_planes.hip - the fp32 ->
fp16-pair / bf16-plane conversions, the dual split with its column sums and its gradient scale, its table form, the two transposes, the
im2col front ends of the three patch embeddings - and the maxima the backward producers publish for that scale (common.hpp amax_publish /
amax_publish_block: LayerNorm and row-normalisation backward in rowops.hip, attention_bwd.hip on fp32 and on pairs, the general pair
GEMM's epilogue and the persistent pair kernels' x gelu' epilogue).

One check per op, written once and run on two sides, as the other tiers': ``PrepTwin`` - the plain-C twins of oracle/tt_cpu.c on host
buffers (tests/test_sweep_prep_host.py, no GPU) - and ``PrepHip`` - the HIP library on cuda:0 (tests/test_hip_sweep.py).  Both sides are
driven through the C ABI itself (timetuning_amd._lib and oracle.cpu_twin carry the same prototypes; hip_ops gives the tuning knobs and the
K-split workspace): the hip_ops wrappers allocate their own outputs, and every output here has to lie inside a guarded buffer - 64
elements of a sentinel bit pattern before and after it, the output itself prefilled with a NaN pattern.  After every call the guards are
intact, no prefill is left inside the documented extent, and rows R .. Rpad - 1 of a transposed output are zero.

The reference of every conversion is the NumPy restatement below (``pair_bits``, ``pair_layout``, ``bf16_bits``, ``plane_bits``), not the
twin and not hip_ops.split_pairs: hi = fp16(v), lo = fp16((v - hi) * 2048) at pair_index(i) = ((i >> 5) << 6) + (i & 31) and 32 further;
bf16 planes are round-to-nearest-even residual splits.  Conversion, transpose and im2col outputs, the scale S, the range flag and the
published maxima are compared EXACTLY (a NaN's payload is not part of either format's contract: NaNs are compared as NaNs).  The
toleranced quantities are
  * column sums: 1e-6 max-normalised against fp64 (the bound tests/test_hip_pairs.py::test_transposed_pairs holds); from 4096 rows on
    the sweep's long-run rule - 4 x the error of the fp32 twin against fp64 on that case, never below 1e-6.  On the HIP side the folded
    sums also equal, bit for bit, the unfolded partials [ceil(Rpad / 64)][C] folded in launch_colsum_fold's order (``colsum_fold``):
    wave w of four adds blocks w, w + 4, w + 8, ... in that order, then (w0 + w1) + (w2 + w3);
  * patch-embedding tokens: TOL_F32 max-normalised and TOL_L2 against fp64 conv2d + cls + pos (for planes on the bf16-rounded image and
    weight), the class row within 1e-6; from C P P >= 96 on the pair entry's relative L2 is not above the f32 entry's (HIP side: the
    twin's f32 entry sums in fp64);
  * dx of the producers, at the first tier's bounds: TOL_BWD (LayerNorm, attention), TOL_F32 (row normalisation), TOL_F32 and TOL_L2 (the
    pair data gradient); y, mean and rstd of layernorm_long TOL_F32.
The twin takes its own maximum where the library takes a producer's slot and raises way 0 only, so what concerns the 16 ways and a slot
that is too small is asserted on the HIP side alone.  The twin's products are naive loops: cases beyond TWIN_MAX_MACS multiply-adds (the
general pair kernel's big grids, everything on the persistent kernels) run on the GPU only.

Worst values of the GPU run (profiles/sweep_prep_worst.json), each against its bound: every one of the 47 exact quantities 0 mismatches;
column sums 1.6e-7 (split_dual), 2.4e-7 (transpose_planes) and partials 1.2e-7 of 1e-6; tokens max 8.1e-7 / 2.6e-7 / 3.0e-7 (f32 / pairs /
planes) of 2e-5, L2 3.6e-7 / 1.4e-7 / 1.5e-7 of 2e-6, class row 8.5e-8 of 1e-6; LayerNorm dx 1.8e-7, attention dqkv 1.8e-6 (9.2e-7 on
pairs) of 5e-5; row-normalisation dx 7.9e-8 and the pair data gradient 4.2e-7 of 2e-5, its L2 2.2e-7 of 2e-6; layernorm_long y 1.5e-7
of 2e-5, dx / dgamma / dbeta 1.7e-7 / 2.8e-7 / 2.7e-7 of 5e-5.  ONE quantity comes within 2 x of its bound: the pair patch embedding's
L2 relative to the f32 entry's, 0.67 of 1.0 at its worst case (a ratio of two errors of the same class, not a distance to a reference)."""
from __future__ import annotations

import contextlib
import ctypes as C
import math

import numpy as np

from _sweep_cases import LN_MAX_D, ceil_to, multi_entries, sd_kernel, sd_rpad, tp_rpad
from _sweep_checks_eval import case_rng, make_note

f32, f64, u16, u32 = np.float32, np.float64, np.uint16, np.uint32
TOL_SUM = 1e-6          # column sums (tests/test_hip_pairs.py::test_transposed_pairs)
TOL_F32 = 2e-5          # the first tier's bounds (tests/test_hip_sweep.py)
TOL_BWD = 5e-5
TOL_L2 = 2e-6
LONG_RUN = 4096         # rows from which the column sums take the long-run rule
GUARD = 64
SENT16, FILL16 = 0x5A5A, 0x7FB1               # (0x7FB1: a NaN as fp16 and as bf16)
SENT32, FILL32 = 0x5A5A5A5A, 0x7FC12345       # (a NaN as fp32)
WAYS, WAY_STRIDE = 16, 64                     # common.hpp kAmaxWays, kAmaxStride


# ---- the restatements ------------------------------------------------------------------------------------------------------------------------

def pair_bits(v):
    """fp32 array -> (hi, lo) fp16 bit patterns: hi = fp16(v), lo = fp16((fp32(v) - fp32(hi)) * 2048)."""
    v = np.asarray(v, f32)
    with np.errstate(all="ignore"):
        hi = v.astype(np.float16)
        lo = ((v - hi.astype(f32)) * f32(2048)).astype(np.float16)
    return hi.view(u16), lo.view(u16)


def pair_layout(v):
    """fp32 [R, C] (C % 32 == 0) -> uint16 [R, 2 C]: groups of 32 as [hi x 32][lo x 32], i.e. hi of element i at pair_index(i), lo 32 further."""
    R, Cc = v.shape
    hi, lo = pair_bits(v)
    out = np.empty((R, Cc // 32, 2, 32), u16)
    out[:, :, 0], out[:, :, 1] = hi.reshape(R, Cc // 32, 32), lo.reshape(R, Cc // 32, 32)
    return out.reshape(R, 2 * Cc)


def pair_bad(v) -> int:
    """The range flag: (hi_bits & 0x7fff) >= 0x7c00 over every element that is split."""
    return int(((pair_bits(v)[0] & 0x7FFF) >= 0x7C00).any())


def pair_join(bits):
    """uint16 [R, 2 C] pairs -> the fp32 value fma(lo, 2^-11, hi) (exact in fp64, rounded once)."""
    R, C2 = bits.shape
    g = bits.reshape(R, C2 // 64, 2, 32)
    with np.errstate(all="ignore"):
        return (g[:, :, 0].copy().view(np.float16).astype(f64) + g[:, :, 1].copy().view(np.float16).astype(f64) / 2048.0).astype(f32).reshape(R, C2 // 2)


def bf16_bits(v):
    """fp32 -> bf16 bit patterns, round to nearest even."""
    u = np.ascontiguousarray(v, f32).view(u32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(u16)
    return np.where(np.isnan(v), u16(0x7FC0), r)


def bf16_value(bits):
    return (bits.astype(u32) << 16).view(f32)


def plane_bits(v, planes: int):
    """common.hpp split3: p0 = bf16(v), p1 = bf16(v - p0), p2 = bf16(v - p0 - p1) -> uint16 [planes, ...]"""
    out, r = [], np.asarray(v, f32)
    with np.errstate(all="ignore"):
        for _ in range(planes):
            b = bf16_bits(r)
            out.append(b)
            r = r - bf16_value(b)
    return np.stack(out)


def canon16(bits, bf=False):
    """NaNs -> one pattern (a NaN's payload is not part of the contract)."""
    lim, q = (0x7F80, 0x7FC0) if bf else (0x7C00, 0x7E00)
    return np.where((bits & 0x7FFF) > lim, u16(q), bits)


def canon32(v):
    b = np.ascontiguousarray(v, f32).view(u32)
    return np.where(np.isnan(v), u32(0x7FC00000), b)


def pair_scale(amax: float) -> float:
    """gemm_planes.hip pair_scale_of: S = 2^(13 - floor(log2(amax))) clamped to 2^+-100; 1 for 0, inf and NaN."""
    if not (amax > 0 and amax < math.inf):
        return 1.0
    e = 13 - (math.frexp(float(amax))[1] - 1)
    return math.ldexp(1.0, max(-100, min(100, e)))


def colsum_fold(parts):
    """rowops.hip launch_colsum_fold (common.hpp colsum_fold_block) on partials [chunks][C]: wave w of four adds chunks w, w + 4, ... in fp32,
    in that order; the result is (w0 + w1) + (w2 + w3)."""
    acc = np.zeros((4, parts.shape[1]), f32)
    for c in range(parts.shape[0]):
        acc[c % 4] = acc[c % 4] + parts[c]
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


def values(rng, shape, vals: str, mag: float = 1.0):
    """The kinds of values: N(0, 1) * mag; log-uniform magnitudes 1e-8 ... 6e4; N(0, 1) with one 7e4 / one inf / one NaN; zeros; fp16 subnormals."""
    n = int(np.prod(shape))
    if vals == "zero":
        return np.zeros(shape, f32)
    if vals == "loguniform":
        x = (10.0 ** rng.uniform(-8, math.log10(6e4), n) * rng.choice((-1.0, 1.0), n)).astype(f32)
    elif vals == "subnormal":
        x = (rng.uniform(6e-8, 6e-5, n) * rng.choice((-1.0, 1.0), n)).astype(f32)
    else:
        x = rng.standard_normal(n, dtype=f32) * f32(mag)
        if vals != "normal":
            x[int(rng.integers(0, n))] = {"big": 7e4, "inf": np.inf, "nan": np.nan}[vals]
    return x.reshape(shape)


def rel_max(a, b) -> float:
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---- the two sides ---------------------------------------------------------------------------------------------------------------------------

class Buf:
    """Storage of one side (a NumPy array / a cuda tensor of the same bytes), a byte offset into it and the element type it was made with."""
    def __init__(self, side, a, off=0):
        a = np.ascontiguousarray(a).reshape(-1)
        self.side, self.store, self.off, self.dt = side, side.upload(a), off * a.itemsize, a.dtype

    @property
    def ptr(self) -> int:
        return self.side.base(self.store) + self.off

    def host(self):
        return self.side.host(self.store).view(self.dt)

    def shift(self, nbytes):
        """The same storage, ``nbytes`` further."""
        b = Buf.__new__(Buf)
        b.side, b.store, b.off, b.dt = self.side, self.store, self.off + nbytes, self.dt
        return b


class Out(Buf):
    """An output of n 16-bit ("h") or 32-bit ("f") elements inside a guarded buffer: [64 x sentinel][n x NaN prefill][64 x sentinel];
    ``init``: what it holds instead of the prefill; ``skew``: elements it starts off the 16-byte boundary."""
    def __init__(self, side, n, kind, init=None, skew=0):
        dt, self.sent, self.fill = (u16, SENT16, FILL16) if kind == "h" else (u32, SENT32, FILL32)
        a = np.full(n + 2 * GUARD + skew, self.sent, dt)
        a[GUARD + skew:GUARD + skew + n] = self.fill if init is None else np.ascontiguousarray(init).reshape(-1).view(dt)
        super().__init__(side, a, GUARD + skew)
        self.n, self.lo = n, GUARD + skew

    def get(self, written=None):
        """The n elements; the guards are intact; ``written`` (a mask or None = all): no prefill is left there."""
        h = self.host()
        assert (h[:self.lo] == self.sent).all() and (h[self.lo + self.n:] == self.sent).all(), "a guard band was written"
        inner = h[self.lo:self.lo + self.n]
        left = inner == self.fill if written is None else (inner == self.fill) & written.reshape(-1)
        assert not left.any(), f"{int(left.sum())} elements of the documented extent were not written"
        return inner


class _Side:
    def src(self, a, off=0):
        """A read-only operand; ``off``: elements it starts off its storage's (16-byte aligned) base."""
        a = np.ascontiguousarray(a).reshape(-1)
        return Buf(self, np.concatenate([np.zeros(off, a.dtype), a]) if off else a, off)

    def call(self, name, *args):
        return self._fn(name)(*[a.ptr if isinstance(a, Buf) else a for a in args], self.stream())

    def run(self, name, *args):
        rc = self.call(name, *args)
        assert rc == 0, (name, rc, self.error())

    def size(self, name, *args) -> int:
        try:
            return int(self._fn(name)(*args))
        except AttributeError:      # (a twin without a workspace query takes none)
            return 0

    def ws(self, nbytes):
        return Buf(self, np.zeros(max(int(nbytes), 16), np.uint8))

    def flag(self):
        return Buf(self, np.zeros(4, np.int32))

    def ksplit(self):
        """(pointer, bytes) of the persistent GEMMs' K-split workspace (include/timetuning_hip.h: the caller's since ABI 7); none on the twin."""
        return None, 0


class PrepTwin(_Side):
    """oracle/tt_cpu.c on host buffers."""
    name = "twin"

    def __init__(self):
        from oracle import cpu_twin

        self.lib = cpu_twin.load()

    def _fn(self, name):
        return getattr(self.lib, "tt_cpu_" + name)

    def upload(self, a):
        return np.array(a, copy=True)

    def base(self, store):
        return store.ctypes.data

    def host(self, store):
        return store

    def stream(self):
        return None

    def error(self):
        return ""

    @contextlib.contextmanager
    def knob(self, name, value):
        yield


class PrepHip(_Side):
    """libtimetuning_hip.so on cuda:0, through the prototypes of timetuning_amd._lib (hip_ops for the tuning knob)."""
    name = "hip"

    def __init__(self):
        import torch
        from timetuning_amd import _lib, hip_ops

        self.torch, self.lib, self.ops = torch, _lib.load(), hip_ops

    def _fn(self, name):
        return getattr(self.lib, "tt_" + name)

    def upload(self, a):
        return self.torch.from_numpy(np.array(a, copy=True).view(np.uint8)).cuda()

    def base(self, store):
        return store.data_ptr()

    def host(self, store):
        return store.cpu().numpy()

    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def error(self):
        return self.lib.tt_last_error().decode(errors="replace")

    def knob(self, name, value):
        return self.ops.tuning_knob(name, value)

    def ksplit(self):
        ws = self.ops.ksplit_workspace()
        return ws.data_ptr(), ws.numel()


_TWIN = None


def prep_twin():
    global _TWIN
    if _TWIN is None:
        _TWIN = PrepTwin()
    return _TWIN


def _eq(note, what, got, want):
    """An exact comparison, reported as a count of mismatching elements with the bound 0."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    note(what + " (mismatches)", int((got != want).sum()), 0, strict=True)


# ---- convert ---------------------------------------------------------------------------------------------------------------------------------

def check_convert(side, p, rng, note):
    n = p["n"]
    x = values(rng, (n,), p["vals"])
    src = side.src(x)
    if p["what"] == "planes":
        P = p["P"]
        out = Out(side, P * n, "h")
        side.run("split_planes", src, out, n, P, n)
        _eq(note, f"planes P={P}", canon16(out.get().reshape(P, n), bf=True), canon16(plane_bits(x, P), bf=True))
        return
    out, flag = Out(side, 2 * n, "h"), side.flag()
    side.run("split_pairs", src, out, n, flag)
    bits = out.get().reshape(n // 32, 64)
    _eq(note, "pairs", canon16(bits), canon16(pair_layout(x.reshape(n // 32, 32))))
    _eq(note, "range flag", flag.host()[:1], [pair_bad(x)])
    back = Out(side, n, "f")
    side.run("join_pairs", out, back, n)
    _eq(note, "join", canon32(back.get().view(f32)), canon32(pair_join(bits).reshape(-1)))


# ---- split_dual ------------------------------------------------------------------------------------------------------------------------------

def run_split(side, x, rpad, t, row, sums, scale, slot=None, off=0):
    """One call of tt_split_pairs_dual (sums "" / "fold") or tt_split_pairs_dual_parts ("parts", or with a producer's slot) on x [R, C] ->
    dict of t [C, 2 Rpad], row [R, 2 C] (uint16), sums [C] or parts [ceil(Rpad / 64), C], S, flag."""
    R, Cc = x.shape
    parts = sums == "parts" or slot is not None
    nblk = (rpad + 63) // 64
    src = side.src(x, off)
    T = Out(side, Cc * 2 * rpad, "h") if t else None
    ROW = Out(side, R * 2 * Cc, "h") if row else None
    SUM = Out(side, nblk * Cc if parts else Cc, "f") if (sums or parts) else None
    SC = Out(side, 1, "f") if scale else None
    flag = side.flag()
    nb = side.size("split_pairs_dual_workspace_bytes", R, Cc, rpad)
    ws = side.ws(nb)
    if parts:
        side.run("split_pairs_dual_parts", src, T, ROW, SUM, SC, slot, R, Cc, rpad, ws, nb, flag)
    else:
        side.run("split_pairs_dual", src, T, ROW, SUM, SC, R, Cc, rpad, ws, nb, flag)
    res = dict(t=T.get().reshape(Cc, 2 * rpad) if t else None, row=ROW.get().reshape(R, 2 * Cc) if row else None,
               S=float(SC.get().view(f32)[0]) if scale else 1.0, flag=int(flag.host()[0]))
    if SUM is not None:
        res["parts" if parts else "sums"] = SUM.get().view(f32).reshape((nblk, Cc) if parts else (Cc,)).copy()
    return res


def expect_split(x, rpad, S):
    """The restatement of the split of x * S -> (t [C, 2 Rpad] with zero rows beyond R, row [R, 2 C] or None, flag)."""
    R, Cc = x.shape
    with np.errstate(all="ignore"):
        xs = x * f32(S)
    xp = np.zeros((rpad, Cc), f32)
    xp[:R] = xs
    return pair_layout(np.ascontiguousarray(xp.T)), (pair_layout(xs) if Cc % 32 == 0 else None), pair_bad(xs)


def slot_way(p: dict) -> int:
    """The way of a split_dual case's slot that carries the true maximum: from the case's own parameters, both halves of the 16 reached."""
    return (5 * p["R"] + p["C"] // 32 + int(p["mag"] < 1e-3) * 8) % WAYS


def slot_of(rng, amax, way, shrink=1.0):
    """A producer's slot [16 ways x 64 floats]: the maximum in ``way``, values at most a quarter of it in the other ways (a fold that
    misses the way is off by two binades or more) - and values far above it in the 63 floats behind each way, which nobody may read."""
    s = np.full(WAYS * WAY_STRIDE, 3e38, f32)
    with np.errstate(all="ignore"):
        s[::WAY_STRIDE] = (rng.uniform(0, 0.25, WAYS) * (amax if math.isfinite(amax) else 1.0) * shrink).astype(f32)
        s[(way % WAYS) * WAY_STRIDE] = f32(amax) * f32(shrink)
    return s


def sum_bound(twin_sums, ref, R):
    """1e-6; from LONG_RUN rows on 4 x the fp32 twin's error on this case, never below 1e-6."""
    return TOL_SUM if R < LONG_RUN else max(TOL_SUM, 4 * rel_max(twin_sums, ref))


def check_sums(note, what, got, ref, tol):
    fin = np.isfinite(ref)
    assert (np.isfinite(got) == fin).all(), what
    if fin.any():
        note(what, rel_max(got[fin], ref[fin]), tol)


def check_split_dual(side, p, rng, note):
    R, Cc, rpad, t, row = p["R"], p["C"], sd_rpad(p), p["t"], p["row"]
    x = values(rng, (R, Cc), p["vals"], p["mag"])
    amax = float(np.abs(x).max())
    S = pair_scale(amax) if p["scale"] else 1.0
    want_t, want_row, want_flag = expect_split(x, rpad, S)
    slot = side.src(slot_of(rng, amax, slot_way(p))) if p["scale"] == "slot" else None
    with side.knob("TT_SPLIT_ROWS", 1 if p["sr"] else 0):
        got = run_split(side, x, rpad, t, row, p["colsum"], bool(p["scale"]), slot, p["off"])
    kern = "/".join(str(k) for k in sd_kernel(p))

    def same(tag, res):
        if t:
            _eq(note, f"{tag} t pairs [{kern}]", canon16(res["t"]), canon16(want_t))      # (rows R .. Rpad - 1 are zero in want_t)
        if row:
            _eq(note, f"{tag} row pairs [{kern}]", canon16(res["row"]), canon16(want_row))
        _eq(note, f"{tag} range flag", [res["flag"]], [want_flag])
        if p["scale"]:
            _eq(note, f"{tag} S", [res["S"]], [S])

    same("split", got)
    if p["scale"] and 0 < amax < math.inf and 2.0 ** -100 < S < 2.0 ** 100:
        assert 2.0 ** 13 <= amax * S < 2.0 ** 14, (amax, S)
    if p["vals"] == "big" and p["scale"]:
        assert S == 0.125 and want_flag == 0 and pair_bad(x) == 1      # (7e4 is beyond fp16 unscaled, inside it at 2^-3)
    if p["vals"] in ("inf", "zero") and p["scale"]:
        assert S == 1.0 and want_flag == int(p["vals"] == "inf")
    # column sums: of the UNSCALED source, against fp64
    ref = x.astype(f64).sum(0)
    nblk = (rpad + 63) // 64
    xz = np.zeros((nblk * 64, Cc), f64)
    xz[:R] = x
    ref_parts = xz.reshape(nblk, 64, Cc).sum(1)
    if "sums" in got or "parts" in got:
        twin = got if side.name == "twin" or R < LONG_RUN else run_split(prep_twin(), x, rpad, t, row, "parts" if "parts" in got else "fold", False)
        if "sums" in got:
            check_sums(note, "column sums", got["sums"], ref, sum_bound(twin["sums"], ref, R))
        else:
            check_sums(note, "column partials", got["parts"], ref_parts, TOL_SUM)
            with np.errstate(all="ignore"):
                check_sums(note, "column sums", colsum_fold(got["parts"]), ref, sum_bound(colsum_fold(twin["parts"]), ref, R))
    if side.name != "hip":
        return
    if p["colsum"] == "fold" and not p["scale"]:      # the folded sums ARE the partials folded in launch_colsum_fold's order
        with side.knob("TT_SPLIT_ROWS", 1 if p["sr"] else 0):
            again = run_split(side, x, rpad, t, row, "parts", False, None, p["off"])
        with np.errstate(all="ignore"):
            _eq(note, "folded sums against the folded partials", canon32(got["sums"]), canon32(colsum_fold(again["parts"])))
    if sd_kernel(p)[0] == "rows":                      # the streaming kernel against the tile kernel on the same call
        with side.knob("TT_SPLIT_ROWS", 0):
            tile = run_split(side, x, rpad, t, row, p["colsum"], bool(p["scale"]), slot, p["off"])
        _eq(note, "streaming against tile kernel: row pairs", tile["row"], got["row"])
        assert (tile["S"], tile["flag"]) == (got["S"], got["flag"])
    if p["scale"] == "slot":                           # bit equal to the split that measures the maximum itself; a slot 64 x too small is loud
        own = run_split(side, x, rpad, t, row, p["colsum"], True, None, 0)
        same("own max", own)
        if 0 < amax < math.inf and 2.0 ** -100 < S * 64 <= 2.0 ** 100:
            low = run_split(side, x, rpad, t, row, p["colsum"], True, side.src(slot_of(rng, amax, slot_way(p), 1.0 / 64)), 0)
            assert low["S"] == S * 64 and low["flag"] == 1, (low["S"], S, low["flag"])


# ---- split_multi -----------------------------------------------------------------------------------------------------------------------------

def check_split_multi(side, p, rng, note):
    ents = multi_entries(p)
    n = len(ents)
    xs, ts, rows = [], [], []
    for R, Cc, outs in ents:
        x = values(rng, (R, Cc), "normal")
        xs.append(x)
        ts.append(Out(side, Cc * 2 * ceil_to(R, 32), "h") if outs in ("t", "both") else None)
        rows.append(Out(side, R * 2 * Cc, "h") if outs in ("row", "both") else None)
    srcs = [side.src(x) for x in xs]
    spare = Out(side, 4096, "h")                      # a buffer of no entry
    arr = lambda bufs: (C.c_void_p * n)(*[b.ptr if b is not None else None for b in bufs])
    ints = lambda v: (C.c_int * n)(*v)
    flag = side.flag()
    side.run("split_pairs_dual_multi", arr(srcs), arr(ts), arr(rows), ints([e[0] for e in ents]), ints([e[1] for e in ents]),
             ints([ceil_to(e[0], 32) for e in ents]), n, flag)
    bad_t = bad_row = bad_single = 0
    for i, ((R, Cc, outs), x) in enumerate(zip(ents, xs)):
        rpad = ceil_to(R, 32)
        want_t, want_row, _ = expect_split(x, rpad, 1.0)
        if ts[i] is not None:
            bad_t += int((ts[i].get().reshape(Cc, 2 * rpad) != want_t).sum())
        if rows[i] is not None:
            bad_row += int((rows[i].get().reshape(R, 2 * Cc) != want_row).sum())
        if i < len(set(ents)):                        # the single-call split of each distinct shape
            one = run_split(side, x, rpad, ts[i] is not None, rows[i] is not None, "", False)
            for k, o in (("t", ts[i]), ("row", rows[i])):
                if o is not None:
                    bad_single += int((o.get().reshape(one[k].shape) != one[k]).sum())
    note("t pairs (mismatches)", bad_t, 0, strict=True)
    note("row pairs (mismatches)", bad_row, 0, strict=True)
    note("against the single call (mismatches)", bad_single, 0, strict=True)
    assert (spare.host()[GUARD:GUARD + 4096] == FILL16).all() and int(flag.host()[0]) == 0


# ---- the transposes --------------------------------------------------------------------------------------------------------------------------

def check_transpose_pairs(side, p, rng, note):
    R, Cc, rpad = p["R"], p["C"], sd_rpad(p)
    # values of 22 significant bits, none under 2^-10: x - hi then has at most 11 bits, lo is exact, the pair joins to x itself and splits
    # again into the same pair (a full 24-bit value need not: its lo is rounded, and the joined value can round to another hi)
    x = (values(rng, (R, Cc), "normal").view(u32) & u32(0xFFFFFFFC)).view(f32)
    x[np.abs(x) < 2.0 ** -10] = 0
    pairs = pair_layout(x)
    out = Out(side, Cc * 2 * rpad, "h")
    side.run("transpose_pairs", side.src(pairs), out, R, Cc, rpad)
    got = out.get().reshape(Cc, 2 * rpad)
    joined = pair_join(pairs)
    assert (joined == x).all()
    _eq(note, "against the restatement", got, expect_split(x, rpad, 1.0)[0])
    _eq(note, "against split_dual of the joined source", got, run_split(side, joined, rpad, 1, 0, "", False)["t"])


def check_transpose_planes(side, p, rng, note):
    R, Cc, rpad = p["R"], p["C"], tp_rpad(p)
    x = values(rng, (R, Cc), "normal")
    want = np.zeros((Cc, rpad), u16)
    want[:, :R] = bf16_bits(np.ascontiguousarray(x.T))
    src = side.src(x)
    out = Out(side, Cc * rpad, "h")
    side.run("transpose_planes", src, out, R, Cc, rpad)
    plain = out.get().reshape(Cc, rpad)
    _eq(note, f"bf16 transpose [Rpad % 4 = {rpad % 4}, % 64 = {rpad % 64}]", plain, want)
    if not p["colsum"]:
        return
    out2, sums = Out(side, Cc * rpad, "h"), Out(side, Cc, "f")
    nb = side.size("transpose_planes_colsum_workspace_bytes", R, Cc, rpad)
    side.run("transpose_planes_colsum", src, out2, R, Cc, rpad, sums, side.ws(nb), nb)
    _eq(note, "bf16 transpose with the column sums", out2.get().reshape(Cc, rpad), plain)
    ref = x.astype(f64).sum(0)
    got = sums.get().view(f32)
    tol = TOL_SUM
    if R >= LONG_RUN:
        tsum = got
        if side.name != "twin":
            tw = prep_twin()
            o, s = Out(tw, Cc * rpad, "h"), Out(tw, Cc, "f")
            tw.run("transpose_planes_colsum", tw.src(x), o, R, Cc, rpad, s, tw.ws(16), 16)
            tsum = s.get().view(f32)
        tol = sum_bound(tsum, ref, R)
    note("column sums", rel_max(got, ref), tol)


# ---- the producers' maxima -------------------------------------------------------------------------------------------------------------------

def fresh_slot(fill=0.0):
    """A zeroed slot (or every way at ``fill``), with a pattern nobody may touch in the 63 floats behind each way."""
    s = np.full(WAYS * WAY_STRIDE, 1234.5, f32)
    s[::WAY_STRIDE] = fill
    return s


def slot_ways(slot_host):
    s = np.asarray(slot_host).view(f32)
    rest = np.delete(s, np.arange(0, WAYS * WAY_STRIDE, WAY_STRIDE))
    assert (rest == f32(1234.5)).all(), "floats between the ways were written"
    return s[::WAY_STRIDE].copy()


def ln_inputs(rng, groups, N, D):
    """x [groups, N, D] about 0.3 with deviation 2, gamma about 1, beta."""
    x = (rng.standard_normal((groups, N, D), dtype=f32) * f32(2.0) + f32(0.3)).astype(f32)
    gamma = (1 + 0.1 * rng.standard_normal(D, dtype=f32)).astype(f32)
    beta = (0.1 * rng.standard_normal(D, dtype=f32)).astype(f32)
    return x, gamma, beta


def ln_stats(x2):
    xd = x2.astype(f64)
    return xd.mean(1), 1.0 / np.sqrt(xd.var(1) + 1e-6)


def ln_reference(x2, gamma, dy):
    """x2 [rows, D] (the rows that have a dy) -> mean, rstd (fp64), xhat, dx, dgamma, dbeta of nn.LayerNorm's autograd in fp64."""
    xd, gd, dd = x2.astype(f64), gamma.astype(f64), dy.astype(f64)
    mean, rstd = ln_stats(x2)
    xh = (xd - mean[:, None]) * rstd[:, None]
    g = dd * gd
    dx = rstd[:, None] * (g - g.mean(1)[:, None] - xh * (g * xh).mean(1)[:, None])
    return mean, rstd, xh, dx, (dd * xh).sum(0), dd.sum(0)


def ln_bwd(side, dy, x, gamma, mean, rstd, dx_init, rows, D, add, skip, slot, wgrad, off):
    """tt_layernorm_bwd into a guarded dx (prefilled with ``dx_init`` or NaNs) -> (dx as fp32 bits' view, dgamma, dbeta)."""
    DX = Out(side, x.size, "f", init=dx_init, skew=off)
    dg, db = (Out(side, D, "f"), Out(side, D, "f")) if wgrad else (None, None)
    nb = side.size("layernorm_bwd_workspace_bytes", rows, D)
    side.run("layernorm_bwd", side.src(dy, off), side.src(x, off), side.src(gamma, off), side.src(mean), side.src(rstd), DX, dg, db, rows, D,
             int(add), int(skip), side.ws(nb), nb, slot)
    visited = None
    if skip:                                          # token 0's rows are not touched: they keep what they held
        visited = np.ones((x.size // D // skip, skip, D), bool)
        visited[:, 0] = False
    dx = DX.get(visited).view(f32).reshape(x.shape)
    return dx, (dg.get().view(f32) if wgrad else None), (db.get().view(f32) if wgrad else None)


def amax_rules(side, note, produce, make_dy):
    """The rules every producer keeps.  ``produce(dy, slot Buf)`` runs the kernel and returns the dx tensor that call wrote."""
    dy = make_dy(1.0)
    slot = side.src(fresh_slot())
    dx = produce(dy, slot)
    m1 = float(np.abs(dx).max())
    ways = slot_ways(slot.host())
    _eq(note, "published max against max |dx|", [float(ways.max())], [m1])
    # two calls into one slot leave the max of both; a slot already above the result is unchanged
    dx2 = produce(make_dy(0.37), slot)
    _eq(note, "max of two calls", [float(slot_ways(slot.host()).max())], [max(m1, float(np.abs(dx2).max()))])
    high = side.src(fresh_slot(f32(4.0) * f32(max(m1, 1e-30))))
    produce(dy, high)
    _eq(note, "a slot above the result", slot_ways(high.host()), fresh_slot(f32(4.0) * f32(max(m1, 1e-30)))[::WAY_STRIDE])
    return dy, dx, ways


def split_from_slot(side, note, dx2d, ways):
    """split_dual(dx, scale = "slot") on the producer's own slot equals scale = "own" bit for bit (transposed pairs; row pairs at D % 32 == 0)."""
    R, Cc = dx2d.shape
    rpad, row = ceil_to(R, 32), int(Cc % 32 == 0)
    b = run_split(side, dx2d, rpad, 1, row, "parts", True, None)
    for roll in (0, WAYS // 2):      # (a maximum is order-independent: the ways as the producer left them, and rotated by half the slot)
        s = fresh_slot()
        s[::WAY_STRIDE] = np.roll(ways, roll)
        a = run_split(side, dx2d, rpad, 1, row, "parts", True, side.src(s))
        _eq(note, "split from the slot against the split's own max: t", a["t"], b["t"])
        if row:
            _eq(note, "split from the slot against the split's own max: row", a["row"], b["row"])
        assert a["S"] == b["S"] == pair_scale(float(np.abs(dx2d).max())) and a["flag"] == b["flag"] == 0


def rel_l2(a, b) -> float:
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def attention_reference(qkv, do, H):
    """softmax(q k^T / 8) v per (frame, head) in fp64 -> out [F, N, 64 H], lse [F, H, N], dqkv [F, N, 192 H] for the upstream ``do``."""
    Fr, N, _ = qkv.shape
    q, k, v = (qkv.astype(f64).reshape(Fr, N, 3, H, 64)[:, :, i].transpose(0, 2, 1, 3) for i in range(3))      # [F, H, N, 64]
    dO = do.astype(f64).reshape(Fr, N, H, 64).transpose(0, 2, 1, 3)
    sc = q @ k.transpose(0, 1, 3, 2) * 0.125
    mx = sc.max(-1, keepdims=True)
    lse = mx[..., 0] + np.log(np.exp(sc - mx).sum(-1))
    P = np.exp(sc - lse[..., None])
    out = P @ v
    dV = P.transpose(0, 1, 3, 2) @ dO
    dS = P * (dO @ v.transpose(0, 1, 3, 2) - (dO * out).sum(-1, keepdims=True))
    dQ, dK = dS @ k * 0.125, dS.transpose(0, 1, 3, 2) @ q * 0.125
    dqkv = np.stack([dQ, dK, dV], 0).transpose(1, 3, 0, 2, 4).reshape(Fr, N, 3 * H * 64)
    return out.transpose(0, 2, 1, 3).reshape(Fr, N, H * 64), lse, dqkv


def check_attention_amax(side, p, rng, note):
    Fr, N, H, pairs = p["F"], p["N"], p["H"], p["producer"] == "attn_bwd_pairs"
    qkv = (rng.standard_normal((Fr, N, 3 * H * 64), dtype=f32) * f32(1.5)).astype(f32)
    draws = {s: (rng.standard_normal((Fr, N, H * 64), dtype=f32) * f32(p["gscale"] * s)).astype(f32) for s in (1.0, 0.37)}
    out, lse, _ = attention_reference(qkv, draws[1.0], H)
    out32, lse32 = out.astype(f32), lse.astype(f32)
    name = "attention_bwd_pairs" if pairs else "attention_bwd"
    nb = max(side.size(name + "_workspace_bytes", Fr, N, H, 64), 16)
    flags = []

    def produce(do, slot):
        DQ = Out(side, qkv.size, "f")
        args = [side.src(qkv), side.src(out32), side.src(do), side.src(lse32), DQ, Fr, N, H, 64, 0.125]
        if pairs:
            flag = side.flag()
            din = side.src(slot_of(rng, float(np.abs(do).max()), int(rng.integers(0, WAYS)))) if p["dslot"] else None
            side.run(name, *args, din, side.ws(nb), nb, flag, slot)
            flags.append(int(flag.host()[0]))
        else:
            side.run(name, *args, side.ws(nb), nb, slot)
        return DQ.get().view(f32).reshape(qkv.shape)

    do, dqkv, ways = amax_rules(side, note, produce, lambda s: draws[s])
    note(f"{p['producer']} dqkv max", rel_max(dqkv, attention_reference(qkv, do, H)[2]), TOL_BWD)
    assert not any(flags)
    split_from_slot(side, note, np.ascontiguousarray(dqkv.reshape(Fr * N, 3 * H * 64)), ways)


def gelu_grad64(x):
    import torch

    t = torch.from_numpy(np.asarray(x, f64))
    return (0.5 * (1 + torch.erf(t / math.sqrt(2.0))) + t * torch.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)).numpy()


def check_dgrad_amax(side, p, rng, note):
    """dx [M, K] = dy [M, N] @ w [N, K] (x gelu'(pre)) on pair operands the restatement made: dy scaled by its power of two, w transposed."""
    M, N, K, gelu = p["M"], p["N"], p["K"], p["producer"] == "dgrad_gelu"
    w = (rng.standard_normal((N, K), dtype=f32) * f32(0.05)).astype(f32)
    pre = rng.standard_normal((M, K), dtype=f32) if gelu else None
    draws = {s: (rng.standard_normal((M, N), dtype=f32) * f32(p["gscale"] * s)).astype(f32) for s in (1.0, 0.37)}
    wT, PRE = side.src(pair_layout(np.ascontiguousarray(w.T))), (side.src(pre) if gelu else None)
    kws, knb = side.ksplit()

    def produce(dy, slot):
        S = pair_scale(float(np.abs(dy).max()))
        DX = Out(side, M * K, "f")
        side.run("linear_bwd_data_pairs", side.src(pair_layout(dy * f32(S))), wT, PRE, DX, side.src(np.array([S], f32)), M, N, K, kws, knb, slot)
        return DX.get().view(f32).reshape(M, K)

    dy, dx, ways = amax_rules(side, note, produce, lambda s: draws[s])
    ref = dy.astype(f64) @ w.astype(f64)
    if gelu:
        ref = ref * gelu_grad64(pre)
    note(f"{p['producer']} dx max", rel_max(dx, ref), TOL_F32)
    note(f"{p['producer']} dx l2", rel_l2(dx, ref), TOL_L2)
    split_from_slot(side, note, dx, ways)


def check_grad_amax(side, p, rng, note):
    if p["producer"].startswith("attn"):
        return check_attention_amax(side, p, rng, note)
    if p["producer"].startswith("dgrad"):
        return check_dgrad_amax(side, p, rng, note)
    rows, D, N, off = p["rows"], p["D"], p["N"], p["off"]
    if p["producer"] == "l2_bwd":
        x = (rng.standard_normal((rows, D), dtype=f32) * f32(4.0)).astype(f32)
        nrm = np.sqrt((x.astype(f64) ** 2).sum(1))
        xn, inv = (x / np.maximum(nrm, 1e-12)[:, None]).astype(f32), (1.0 / np.maximum(nrm, 1e-12)).astype(f32)
        draws = {s: (rng.standard_normal((rows, D), dtype=f32) * f32(p["gscale"] * s)).astype(f32) for s in (1.0, 0.37)}

        def produce(dxn, slot):
            DX = Out(side, rows * D, "f")
            side.run("l2norm_bwd", side.src(dxn), side.src(xn), side.src(inv), DX, rows, D, slot)
            return DX.get().view(f32).reshape(rows, D)

        dxn, dx, ways = amax_rules(side, note, produce, lambda s: draws[s])
        xd = xn.astype(f64)
        ref = (dxn.astype(f64) - xd * (xd * dxn.astype(f64)).sum(1)[:, None]) * inv.astype(f64)[:, None]
        note("l2_bwd dx max", rel_max(dx, ref), TOL_F32)
        if side.name == "hip":
            assert (ways[min(WAYS, (rows + 3) // 4):] == 0).all()      # workgroup b raises way b % 16 only
        split_from_slot(side, note, dx, ways)
        return
    groups, tok = (rows // (N - 1), N) if N else (rows, 1)
    x, gamma, _ = ln_inputs(rng, groups, tok, D)
    x2 = x[:, 1:].reshape(rows, D) if N else x.reshape(rows, D)
    draws = {s: (rng.standard_normal((rows, D), dtype=f32) * f32(p["gscale"] * s)).astype(f32) for s in (1.0, 0.37)}
    acc = (rng.standard_normal(x.shape, dtype=f32) * f32(3 * p["gscale"])).astype(f32) if p["accum"] else None
    init = acc if p["accum"] else (np.zeros(x.shape, f32) if N else None)      # (dropping token 0: the caller zeroes dx, as hip_ops does)

    mean, rstd = ln_stats(x2)

    def produce(dy, slot):
        return ln_bwd(side, dy, x, gamma, mean.astype(f32), rstd.astype(f32), init, rows, D, p["accum"], N, slot, False, off)[0]

    dy, dx, ways = amax_rules(side, note, produce, lambda s: draws[s])
    ref = ln_reference(x2, gamma, dy)[3]
    full = np.zeros(x.shape, f64) if not p["accum"] else acc.astype(f64)
    if N:
        assert (dx[:, 0] == 0).all()
        full[:, 1:] += ref.reshape(groups, N - 1, D)
    else:
        full += ref.reshape(x.shape)
    note("ln_bwd dx max", rel_max(dx, full), TOL_BWD)
    if side.name == "hip":
        from _sweep_cases import ln_bwd_plan

        assert (ways[min(WAYS, ln_bwd_plan(rows, D, off)[1]):] == 0).all()
    split_from_slot(side, note, np.ascontiguousarray(dx.reshape(-1, D)), ways)


def check_layernorm_long(side, p, rng, note):
    Fr, Nt, D, drop = p["Fr"], p["Nt"], p["D"], p["drop"]
    x, gamma, beta = ln_inputs(rng, Fr, Nt, D)
    x2 = x[:, 1:].reshape(-1, D) if drop else x.reshape(-1, D)
    rows = x2.shape[0]
    dy = rng.standard_normal((rows, D), dtype=f32)
    mean, rstd, xh, dx_ref, dg_ref, db_ref = ln_reference(x2, gamma, dy)
    Y, M, RS = Out(side, rows * D, "f"), Out(side, rows, "f"), Out(side, rows, "f")
    side.run("layernorm_fwd", side.src(x), side.src(gamma), side.src(beta), Y, M, RS, rows, D, 1e-6, Nt if drop else 0)
    note("y max", rel_max(Y.get().view(f32).reshape(rows, D), xh * gamma.astype(f64) + beta.astype(f64)), TOL_F32)
    note("mean max", rel_max(M.get().view(f32), mean), TOL_F32)
    note("rstd max", rel_max(RS.get().view(f32), rstd), TOL_F32)
    init = np.zeros(x.shape, f32) if drop else None
    dx, dg, db = ln_bwd(side, dy, x, gamma, M.get().view(f32), RS.get().view(f32), init, rows, D, 0, Nt if drop else 0, None, True, 0)
    full = np.zeros(x.shape, f64)
    if drop:
        full[:, 1:] = dx_ref.reshape(Fr, Nt - 1, D)
    else:
        full = dx_ref.reshape(x.shape)
    note("dx max", rel_max(dx, full), TOL_BWD)
    note("dgamma max", rel_max(dg, dg_ref), TOL_BWD)
    note("dbeta max", rel_max(db, db_ref), TOL_BWD)


def ln_refuses_amax_with_drop_and_accum(side):
    """include/timetuning_hip.h: amax_out with add_to_dx and skip_group together is refused (token 0's rows of dx are not visited, so the
    published value would miss what was accumulated there) - before anything is written; each pair of the three is accepted."""
    rng = np.random.default_rng(5)
    x, gamma, _ = ln_inputs(rng, 3, 5, 64)
    dy = rng.standard_normal((12, 64), dtype=f32)
    mean, rstd = (a.astype(f32) for a in ln_stats(x[:, 1:].reshape(12, 64)))
    DX, slot = Out(side, x.size, "f"), side.src(fresh_slot())
    nb = side.size("layernorm_bwd_workspace_bytes", 12, 64)
    rc = side.call("layernorm_bwd", side.src(dy), side.src(x), side.src(gamma), side.src(mean), side.src(rstd), DX, None, None, 12, 64, 1, 5,
                   side.ws(nb), nb, slot)
    assert rc != 0 and (DX.host()[GUARD:GUARD + x.size] == FILL32).all() and (slot_ways(slot.host()) == 0).all()
    if side.name == "hip":
        assert "amax_out with add_to_dx and skip_group" in side.error()
    for add, skip, sl in ((1, 5, None), (0, 5, slot), (1, 0, slot)):
        xx = x if skip else x[:, 1:]
        init = np.zeros(xx.shape, f32)
        ln_bwd(side, dy, np.ascontiguousarray(xx), gamma, mean, rstd, init, 12, 64, add, skip, sl, False, 0)


# ---- patch embedding -------------------------------------------------------------------------------------------------------------------------

def im2col(img, fmap, P):
    """[F (n + 1), C P P]: row (f, t) is patch t - 1 of frame fmap[f] in the conv weight's own order k = (c P + y) P + x, gy = (t - 1) // gw; the
    class token's row is zero."""
    _, Cc, H, W = img.shape
    gh, gw = H // P, W // P
    pat = img[fmap].reshape(len(fmap), Cc, gh, P, gw, P).transpose(0, 2, 4, 1, 3, 5).reshape(len(fmap), gh * gw, Cc * P * P)
    return np.concatenate([np.zeros((len(fmap), 1, Cc * P * P), img.dtype), pat], 1).reshape(-1, Cc * P * P)


def check_patch_embed(side, p, rng, note):
    mode, Fr, Cc, P, gh, gw, D = p["mode"], p["F"], p["C"], p["P"], p["gh"], p["gw"], p["D"]
    H, W, n, K = gh * P, gw * P, gh * gw, Cc * P * P
    nsrc = Fr if p["fmap"] != "repeat" else min(Fr, 3) + 3
    fmap = (rng.integers(0, nsrc - 3, Fr) if p["fmap"] == "repeat" else (np.arange(Fr)[::-1] if p["fmap"] == "rev" else np.arange(Fr))).astype(np.int32)
    img = rng.standard_normal((nsrc, Cc, H, W), dtype=f32)
    w = (rng.standard_normal((D, K), dtype=f32) * f32(0.05)).astype(f32)
    bias, cls, pos = (rng.standard_normal(sh, dtype=f32) for sh in ((D,), (D,), (n + 1, D)))
    FM = None if p["fmap"] == "" else side.src(fmap)
    TOK = Out(side, Fr * (n + 1) * D, "f")
    common = [side.src(img), FM]
    tail = [side.src(bias), side.src(cls), side.src(pos), TOK, Fr, Cc, H, W, P, D]
    rows = im2col(img, fmap, P)
    img_r, w_r, WS = img, w, None
    if mode == "f32":
        with side.knob("TT_PATCH_LEAN", 1 if p["lean"] else 0):
            side.run("patch_embed_fwd", *common, side.src(w), *tail)
    else:
        nb = max(side.size(f"patch_embed_{mode}_workspace_bytes", Fr, Cc, H, W, P), 16)
        WS = Out(side, nb // 2, "h")
        if mode == "pairs":
            flag = side.flag()
            side.run("patch_embed_fwd_pairs", *common, side.src(pair_layout(w)), *tail, WS, nb, flag)
            assert int(flag.host()[0]) == 0
        else:      # the reference runs on the bf16-rounded image and weight, as the sweep's linear_planes does
            img_r, w_r = bf16_value(bf16_bits(img)), bf16_value(bf16_bits(w))
            side.run("patch_embed_fwd_planes", *common, side.src(bf16_bits(w)), *tail, WS, nb)
    tok = TOK.get().view(f32).reshape(Fr, n + 1, D)
    # fp64 conv2d + cls + pos
    ref = (im2col(img_r, fmap, P).astype(f64) @ w_r.astype(f64).T + bias.astype(f64)).reshape(Fr, n + 1, D) + pos.astype(f64)
    ref[:, 0] = cls.astype(f64) + pos[0].astype(f64)
    note(f"{mode} tokens max", rel_max(tok, ref), TOL_F32)
    note(f"{mode} tokens l2", rel_l2(tok, ref), TOL_L2)
    note(f"{mode} class row", rel_max(tok[:, 0], ref[:, 0]), 1e-6)
    # f32-class: no worse than the f32 entry's kernel on the same operands (HIP side: the twin's f32 entry sums in fp64)
    if mode == "pairs" and K >= 96 and side.name == "hip":
        T32 = Out(side, Fr * (n + 1) * D, "f")
        side.run("patch_embed_fwd", *common, side.src(w), side.src(bias), side.src(cls), side.src(pos), T32, Fr, Cc, H, W, P, D)
        note("pairs l2 / f32 entry's", rel_l2(tok, ref) / max(rel_l2(T32.get().view(f32).reshape(ref.shape), ref), 1e-30), 1.0, strict=True)
    if side.name == "hip" and WS is not None:      # the im2col rows the GEMM read, at the start of the workspace
        M = Fr * (n + 1)
        got = WS.host()[WS.lo:WS.lo + M * K * (2 if mode == "pairs" else 1)]
        _eq(note, f"{mode} im2col rows", got, (pair_layout(rows) if mode == "pairs" else bf16_bits(rows)).reshape(-1))


# ---- the accepted domains, at the edge ------------------------------------------------------------------------------------------------------

def domain_edges(side):
    """[(what, entry, args, outputs, the launcher's message)]: each call is the first value BEYOND what its entry accepts (the sweep's cases
    stand at the last accepted one: Rpad = ceil32(R), C = 32, n = 32 / 8, D = 1024, the exact workspace sizes).  Outputs are guarded buffers."""
    rng = np.random.default_rng(7)
    x = side.src(rng.standard_normal((33, 64), dtype=f32))
    x33 = side.src(rng.standard_normal((33, 33), dtype=f32))
    xp = side.src(pair_layout(rng.standard_normal((33, 64), dtype=f32)))
    h = lambda n: Out(side, n, "h")
    f = lambda n: Out(side, n, "f")
    out = []

    def add(what, name, args, msg):
        out.append((what, name, args, [a for a in args if isinstance(a, Out)], msg))

    add("transpose_pairs: Rpad % 32", "transpose_pairs", [xp, h(64 * 2 * 48), 33, 64, 48], "multiples of 32")
    add("transpose_pairs: Rpad < R", "transpose_pairs", [xp, h(64 * 2 * 64), 33, 64, 32], "bad arguments")
    add("transpose_pairs: C % 32", "transpose_pairs", [xp, h(64 * 2 * 64), 33, 48, 64], "multiples of 32")
    add("split_pairs_dual: Rpad % 32", "split_pairs_dual", [x, h(64 * 2 * 48), None, None, None, 33, 64, 48, None, 0, None], "Rpad a multiple of 32")
    add("split_pairs_dual: Rpad < R", "split_pairs_dual", [x, h(64 * 2 * 64), None, None, None, 33, 64, 32, None, 0, None], "Rpad a multiple of 32")
    add("split_pairs_dual: C % 32 with row pairs", "split_pairs_dual", [x33, h(33 * 2 * 64), h(33 * 2 * 64), None, None, 33, 33, 64, None, 0, None],
        "row-major pairs need C % 32")
    t = h(64 * 2 * 64 + 8)
    add("split_pairs_dual: dst_t 2 bytes off", "split_pairs_dual", [x, t.shift(2), None, None, None, 33, 64, 64, None, 0, None], "8-byte aligned")
    out[-1][3].append(t)
    nb = side.size("split_pairs_dual_workspace_bytes", 33, 64, 64)
    add("split_pairs_dual: scaled split of a source 4 bytes off", "split_pairs_dual",
        [side.src(rng.standard_normal(33 * 64, dtype=f32), 1), h(64 * 2 * 64), None, None, f(1), 33, 64, 64, side.ws(nb), nb, None], "16-byte aligned source")
    add("split_pairs_dual: workspace one byte short", "split_pairs_dual", [x, h(64 * 2 * 64), None, f(64), None, 33, 64, 64, side.ws(nb), nb - 1, None],
        "workspace too small")
    add("split_pairs_dual_parts: amax_in without scale_out", "split_pairs_dual_parts",
        [x, h(64 * 2 * 64), None, f(64), None, side.src(fresh_slot()), 33, 64, 64, None, 0, None], "scale_out required")
    nb = side.size("transpose_planes_colsum_workspace_bytes", 33, 64, 64)
    add("transpose_planes_colsum: workspace one byte short", "transpose_planes_colsum", [x, h(64 * 64), 33, 64, 64, f(64), side.ws(nb), nb - 1], "workspace too small")
    add("transpose_planes: Rpad < R", "transpose_planes", [x, h(64 * 32), 33, 64, 32], "bad arguments")
    add("split_pairs: n % 32", "split_pairs", [x, h(80), 40, None], "multiple of 32")
    add("join_pairs: n % 32", "join_pairs", [xp, f(40), 40], "multiple of 32")
    add("split_planes: n % 8", "split_planes", [x, h(12), 12, 1, 12], "multiples of 8")
    # the patch entries (tokens [F (n + 1)][D])
    img = side.src(rng.standard_normal((2, 4, 24, 24), dtype=f32))
    vec = side.src(rng.standard_normal(4096, dtype=f32))
    wbits = side.src(np.zeros(192 * 4 * 16 * 16 * 2, u16))
    for mode in ("pairs", "planes"):
        name = f"patch_embed_fwd_{mode}"
        tail = lambda: [] if mode == "planes" else [None]

        def patch(what, Cc, H, W, P, D, msg, short=0):
            nb = side.size(f"patch_embed_{mode}_workspace_bytes", 2, Cc, H, W, P)
            add(f"{name}: {what}", name, [img, None, wbits, vec, vec, vec, f(2 * ((H // max(P, 1)) * (W // max(P, 1)) + 1) * D), 2, Cc, H, W, P, D, side.ws(nb), nb - short,
                                          *tail()], msg)

        patch("P % 4", 4, 24, 24, 6, 64, "need P % 4 == 0")
        patch("C P P % 32 | 64", 1, 24, 24, 4, 64, "C P P %")
        patch("D % 64", 4, 24, 24, 8, 72, "D % 64 == 0")
        patch("H % P", 4, 20, 24, 8, 64, "multiples of the patch size")
        patch("workspace one byte short", 4, 24, 24, 8, 64, "workspace too small", 1)
    add("patch_embed_fwd: H % P", "patch_embed_fwd", [img, None, vec, vec, vec, vec, f(2 * 7 * 64), 2, 4, 20, 24, 8, 64], "multiples of the patch size")
    # D beyond 64 * kMaxPerLane
    D = LN_MAX_D + 1
    big = side.src(rng.standard_normal(3 * D, dtype=f32))
    nb = side.size("layernorm_bwd_workspace_bytes", 3, D)
    add("layernorm_bwd: D 1025", "layernorm_bwd", [big, big, big, big, big, f(3 * D), None, None, 3, D, 0, 0, side.ws(nb), nb, None], "need 0 < D <= 1024")
    return out


def assert_refused(side, what, name, args, outs, msg):
    rc = side.call(name, *args)
    assert rc != 0, f"{what}: accepted"
    assert msg in side.error(), (what, side.error())
    for o in outs:      # nothing was launched: every output still holds its prefill, the guards their sentinel
        hst = o.host()
        assert (hst[:o.lo] == o.sent).all() and (hst[o.lo + o.n:] == o.sent).all() and (hst[o.lo:o.lo + o.n] == o.fill).all(), what


CHECK = {"convert": check_convert, "patch_embed": check_patch_embed, "split_dual": check_split_dual, "split_multi": check_split_multi, "transpose_pairs": check_transpose_pairs,
         "transpose_planes": check_transpose_planes, "grad_amax": check_grad_amax, "layernorm_long": check_layernorm_long}
assert LN_MAX_D == 1024


def run_prep_case(side, op: str, params: dict, worst: dict) -> None:
    CHECK[op](side, params, case_rng(op, params), make_note(worst, op))
