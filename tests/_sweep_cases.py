"""The seeded case table of the ragged-shape kernel sweep (tests/test_hip_sweep.py) - and of tools/fuzz_ops.py, which draws more seeds of it.

A case is ``(op, params)``: ``params`` a flat dict of ints / floats / strings, so that a case prints as its own pytest id.  Each op has
PINNED cases - the route boundaries the launchers branch on, which tests/test_sweep_routes.py checks the table reaches - and ``COUNTS[op]``
random draws from ``SUITE_SEED``.  The draws are the kind a shape fuzz makes: ragged M, N and K, odd token counts, head counts, epilogue
combinations, window and context counts.  Nothing here touches a GPU."""
from __future__ import annotations

import numpy as np

SUITE_SEED = 20261015

# the fp16-pair GEMM's output combinations (hip_ops.linear_fwd_pairs arguments)
PAIR_EPILOGUES = {
    "y": dict(act=0, res=0, out_f32=1, out_pairs=0, save_pre=0),
    "y_res": dict(act=0, res=1, out_f32=1, out_pairs=0, save_pre=0),
    "y_pairs": dict(act=0, res=0, out_f32=1, out_pairs=1, save_pre=0),
    "y_pairs_gelu_pre": dict(act=1, res=0, out_f32=1, out_pairs=1, save_pre=1),
    "pairs_gelu": dict(act=1, res=0, out_f32=0, out_pairs=1, save_pre=0),
    "pairs_gelu_pre": dict(act=1, res=0, out_f32=0, out_pairs=1, save_pre=1),
}
CE_K = (1, 63, 64, 65, 200, 256, 257, 511, 512)


def _b(rng, p=0.5) -> int:
    return int(rng.random() < p)


def _ch(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _linear_f32(rng):
    return dict(M=int(rng.integers(1, 1200)), N=_ch(rng, (50, 64, 72, 128, 192, 200, 384)), K=_ch(rng, (16, 20, 48, 64, 100, 384)),
                act=_b(rng), res=_b(rng))


def _linear_pairs(rng):
    if rng.random() < 0.2:   # the persistent kernel's sizes: large ragged M, whole 128-wide column tiles
        M, N, K = int(rng.integers(9000, 30000)), 128 * int(rng.integers(1, 13)), 96 * int(rng.integers(1, 9))
        epi = _ch(rng, ("y", "y_res", "pairs_gelu"))
    else:
        M, N, K = int(rng.integers(1, 900)), 64 * int(rng.integers(1, 7)), 32 * int(rng.integers(1, 13))
        epi = _ch(rng, ("y_res", "y_pairs", "y_pairs_gelu_pre"))
    return dict(M=M, N=N, K=K, epi=epi)


def _linear_planes(rng):
    return dict(P=_ch(rng, (1, 3)), M=int(rng.integers(1, 600)), N=64 * int(rng.integers(1, 6)), K=64 * int(rng.integers(1, 5)), act=_b(rng),
                res=_b(rng))


def _bwd_pairs(rng):
    return dict(M=int(rng.integers(1, 7000)), N=64 * int(rng.integers(1, 13)), K=64 * int(rng.integers(1, 13)), gelu=_b(rng), tn=_b(rng, 0.7),
                mag=_ch(rng, (1e-3, 3e-8)))


def _layernorm(rng):
    D = _ch(rng, (64, 96, 128, 256, 384, 512, 768, 1000, 1024))
    return dict(Fr=int(rng.integers(1, 9)), Nt=int(rng.integers(2, 40)), D=D, drop=_b(rng), pairs=int(D % 32 == 0 and rng.random() < 0.5))


def _l2norm(rng):
    return dict(rows=int(rng.integers(1, 800)), D=_ch(rng, (3, 64, 96, 128, 256, 500, 1024)), zero_row=_b(rng))


def _attention(rng):
    N = int(rng.integers(1, 900))
    return dict(Fr=int(rng.integers(1, 4)), N=N, H=int(rng.integers(1, 4)), flash=int(N <= 256 and rng.random() < 0.3))


def _ce(rng):
    return dict(rows=int(rng.integers(1, 600)), K=_ch(rng, CE_K), weighted=_b(rng))


def _sinkhorn(rng):
    B, K = int(rng.integers(1, 9000)), int(rng.integers(1, 513))
    row0 = int(rng.integers(0, B)) if rng.random() < 0.4 else 0
    rows_out = int(rng.integers(1, B - row0 + 1)) if row0 or rng.random() < 0.3 else B - row0
    iters = _ch(rng, (0, 1, 3, 10))
    _b(rng)   # a draw nobody reads (it chose the retired one-launch solve): every later op draws from this generator, their cases stay
    return dict(B=B, K=K, iters=iters, row0=row0, rows_out=rows_out)


def _sinkhorn_from_q(rng):
    return dict(B=int(rng.integers(1, 5000)), K=int(rng.integers(1, 513)), iters=_ch(rng, (0, 1, 3, 10)), transposed=_b(rng))


def _sinkhorn_local(rng):
    return dict(B=int(rng.integers(1, 5000)), K=int(rng.integers(1, 513)), iters=_ch(rng, (0, 1, 3, 10)))


def _queue_push(rng):
    Q = int(rng.integers(1, 300))
    return dict(Q=Q, D=_ch(rng, (1, 32, 128, 256)), m=int(rng.integers(1, Q + 1)))


# ---- second tier: the evaluator, optimizer and mask kernels (checks: tests/_sweep_checks_eval.py, on the C twin and on the HIP library)
KM_MAXKD = 16384          # kmeans.hpp: k * d floats of centroids in LDS


def km_max_k(d: int) -> int:
    """kmeans.hpp, km_shape_ok: the largest k both k-means entries take at d (k * d <= KM_MAXKD; at d <= 64 the point tile shares the LDS)."""
    k = KM_MAXKD // d
    if d <= 64:
        k = min(k, (128 * 1024 // 4 - 256 * (d | 1)) // d)
    return k


def _kmeans_assign(rng):
    d = _ch(rng, (1, 2, 3, 8, 9, 16, 17, 31, 50, 64, 65, 100, 128, 384))
    k = int(rng.integers(1, min(km_max_k(d), 300) + 1))
    return dict(P=int(rng.integers(1, 20000)), d=d, k=k, dup=_b(rng, 0.3) if k > 1 else 0)


def _kmeans_accumulate(rng):
    d = _ch(rng, (1, 3, 8, 16, 50, 64, 100, 257, 384))
    k = int(rng.integers(1, min(km_max_k(d), 300) + 1))
    return dict(P=int(rng.integers(1, 30000)), d=d, k=k, mode=_ch(rng, ("rand", "rand", "skip", "one")))


def _col_moments(rng):
    cols = _ch(rng, (1, 2, 9, 50, 255, 256, 257, 384, 1024))      # (a constant column needs a second one to scale the error by)
    return dict(rows=int(rng.integers(1, 20000)), cols=cols, kind=_ch(rng, ("scaled", "const_col", "offset") if cols > 1 else ("scaled", "offset")))


def _upsample(name):
    def gen(rng):
        g = int(rng.integers(1, 29))
        R = int(rng.integers(1, 5 * g + 2))
        return {"M": int(rng.integers(1, 4)), "g": g, "R": R, name: _ch(rng, (1, 2, 7, 21, 64, 65, 200, 255, 256, 300))}
    return gen


def _confusion_counts(rng):
    return dict(n=int(rng.integers(1, 300000)), C=_ch(rng, (1, 2, 7, 21, 96, 97, 300, 1000)), stray=_b(rng))


def _adamw(rng):
    return dict(T=int(rng.integers(1, 100)), big=int(rng.integers(1, 400000)), step=_ch(rng, (1, 2, 37, 5000, 100000)), fused=_b(rng),
                gscale=_ch(rng, (1.0, 0.37, 1e-3)))


def _elementwise(rng):
    n = int(rng.integers(1, 3000000)) if rng.random() < 0.5 else int(rng.integers(1, 5000))
    return dict(n=n, rows=int(rng.integers(1, 40000)), cols=int(rng.integers(1, 65)) if rng.random() < 0.7 else _ch(rng, (255, 256, 1000, 1024)))


def _foreground_mask(rng):
    return dict(F=int(rng.integers(1, 9)), g=_ch(rng, (4, 5, 7, 13, 14, 28, 31, 32)), H=_ch(rng, (1, 3, 6, 12)), hd=_ch(rng, (4, 64, 128)),
                th=_ch(rng, (0.3, 0.65, 0.8)), entry=_ch(rng, ("probs", "qkv")))


def _pos_embed(rng):
    g = _ch(rng, (14, 28))
    while True:
        gh, gw = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        if (gh, gw) != (g, g):      # the stored grid itself is returned as it is, not interpolated
            return dict(g=g, gh=gh, gw=gw, D=_ch(rng, (4, 64, 384, 768)))



# ---- third tier: temporal label propagation (checks: tests/_sweep_checks_prop.py, on the C twin and on the HIP library)
LP_CAND_CAP = 4096        # label_prop.hip: 256 threads x LP_CAND_MAX candidates per query on the square entries
LP_PRECISIONS = ("f32", "f16x3", "bf16")


def lp_cmax(fs: int, nl: int) -> int:
    """label_prop.hip, lp_cmax: the most context frames any target frame of the clip has."""
    return max(1, 1 + min(fs - 2, nl))


def lp_chunk(bs: int, fs: int, n: int, nl: int, cap_mb: int = 0) -> int:
    """label_prop.hip, lp_chunk: target frames whose similarities are held at once (``cap_mb``: TT_LP_SIMS_CAP_MB, 0 = the 256 MB default)."""
    per_t = bs * lp_cmax(fs, nl) * n * n * 4
    T = ((cap_mb if cap_mb else 256) << 20) // per_t
    return max(1, min(T, 65535 // bs, max(fs - 1, 1)))


def lp_caps(p: dict) -> list:
    return [int(c) for c in p["cap"].split("/")] if p["cap"] else []


def LP(**kw) -> dict:
    """A label_prop case: the defaults are a small clip on the wave kernel for <= 3 contexts."""
    c = dict(bs=1, fs=3, g=14, D=16, K=5, nl=1, r=2, topk=5, prec="f32", dup=0, cap="")
    assert set(kw) <= set(c), kw
    c.update(kw)
    return c


def LPG(**kw) -> dict:
    c = dict(bs=1, fs=4, gh=5, gw=9, D=16, K=5, nl=2, r=2, topk=5, prec="f32", dup=0)
    assert set(kw) <= set(c), kw
    c.update(kw)
    return c


def _label_prop(rng):
    g = _ch(rng, (3, 5, 7, 10, 14))       # (win <= 14, <= 8 contexts: at most 1568 candidates, every draw is inside the domain)
    return LP(bs=int(rng.integers(1, 4)), fs=int(rng.integers(2, 8)), g=g, D=_ch(rng, (4, 16, 20, 64)), K=_ch(rng, (1, 2, 7, 21, 64, 65, 200, 300, 513)),
              nl=int(rng.integers(0, 8)), r=int(rng.integers(1, 9)), topk=_ch(rng, (1, 3, 5, 7)), prec=_ch(rng, LP_PRECISIONS), dup=_b(rng, 0.3))


def _label_prop_grid(rng):
    return LPG(bs=int(rng.integers(1, 3)), fs=int(rng.integers(2, 7)), gh=int(rng.integers(1, 13)), gw=int(rng.integers(1, 13)), D=_ch(rng, (4, 16, 64)),
               K=_ch(rng, (1, 2, 21, 257)), nl=int(rng.integers(0, 8)), r=int(rng.integers(0, 7)), topk=_ch(rng, (1, 5, 9)), prec=_ch(rng, LP_PRECISIONS),
               dup=_b(rng, 0.3))


def _upsample_argmax_hw(rng):
    gh, gw = int(rng.integers(1, 29)), int(rng.integers(1, 29))
    return dict(M=int(rng.integers(1, 4)), gh=gh, gw=gw, K=_ch(rng, (1, 2, 7, 21, 64, 65, 200)), H=int(rng.integers(1, 4 * gh + 2)),
                W=int(rng.integers(1, 4 * gw + 2)), dup=_b(rng, 0.3))


# ---- fourth tier: the linear probe and the clip input pipeline (checks: tests/_sweep_checks_head.py, on the C twin and on the HIP library)
PROBE_MAXD, PROBE_MAXC, PROBE_MAXG, PROBE_MAXR = 1024, 256, 64, 1024          # linear_probe.hip: LP_MAXD, LP_MAXC, LP_MAXG, LP_MAXR
WGRAD_LONG_RUN = 512      # rows one workgroup of tt_probe_wgrad sums in fp32 from which the regime rule sets the bound (tests/_sweep_checks_head.py)
ADJOINT_LONG_RUN = 1024   # mask pixels one token of tt_bilinear_adjoint_tokens gathers in fp32, (2 R / g)^2, from which the regime rule applies
GRAY_SUM_CAP = 256 * 2048  # image_ops.hip, tt_img_color: at most 256 workgroups of 256 threads x 8 pixels - beyond, gray_sum_kernel strides
IMG_MODES = ("gray", "brightness", "contrast", "saturation", "hue")


def gather_tp_log2(C: int) -> int:
    """linear_probe.hip, gather_tp_log2: lanes per pixel (log2) so that a lane owns at most 8 classes."""
    l = 0
    while (C + (1 << l) - 1) >> l > 8:
        l += 1
    return l


def probe_logits_kernel(C: int) -> tuple:
    """linear_probe.hip, tt_probe_logits: the (CT, RPT) instantiation for ct = ceil(C / 64) - and 16 * RPT rows per workgroup."""
    ct = (C + 63) // 64
    return (1, 4) if ct == 1 else ((2, 2) if ct == 2 else (4, 2))


def wgrad_split(rows: int, D: int, C: int) -> tuple:
    """linear_probe.hip, wgrad_split -> (splits, rows per split, what capped the split count: "one", "chunks" or "tiles")."""
    tiles = ((D + 63) // 64) * ((C + 63) // 64)
    chunks = (rows + 31) // 32
    cap = (1024 + tiles - 1) // tiles
    ns = max(1, min(cap, chunks))
    rps = ((rows + ns - 1) // ns + 31) // 32 * 32
    return (rows + rps - 1) // rps, rps, "one" if chunks == 1 else ("chunks" if chunks <= cap else "tiles")


def adjoint_run(g: int, R: int) -> float:
    """Mask pixels that read one low-res token: about 2 R / g along each axis (every token is the first or the second tap of R / g pixels)."""
    return (2.0 * R / g) ** 2


def sgd_lengths(T: int, big: int) -> list:
    """Lengths 1, 255, 257, big, 1, ... (one tensor: big), as the adamw cases: a length-1 tensor shares the grid of the longest."""
    cyc = (1, 255, 257, big)
    return [cyc[i % 4] for i in range(T)] if T > 1 else [big]


def PL(rows, D, C, bias) -> dict:
    return dict(rows=rows, D=D, C=C, bias=bias)


def CE(B, g, R, C, ignored=0.3, kind="normal") -> dict:
    return dict(B=B, g=g, R=R, C=C, ignored=ignored, kind=kind)


def ADJ(B, g, R, C) -> dict:
    return dict(B=B, g=g, R=R, C=C)


def WG(rows, D, C, scale, need_bias) -> dict:
    return dict(rows=rows, D=D, C=C, scale=scale, need_bias=need_bias)


def SGD(T, big, steps=3, momentum=0.9, wd=1e-4) -> dict:
    return dict(T=T, big=big, steps=steps, momentum=momentum, wd=wd)


def RS(F, h, w, oh, ow, crop="", flip=0, to_tensor=0) -> dict:
    """crop: "y0/x0/h/w" inside the h x w frame, "" = the whole frame; a flip needs the float output."""
    assert not flip or to_tensor
    return dict(F=F, h=h, w=w, crop=crop, oh=oh, ow=ow, flip=flip, to_tensor=to_tensor)


def COL(F, H, W, mode, factor) -> dict:
    return dict(F=F, H=H, W=W, mode=mode, factor=factor)


def BL(F, H, W, radius) -> dict:
    return dict(F=F, H=H, W=W, radius=radius)


def _probe_logits(rng):
    return PL(int(rng.integers(1, 1200)), _ch(rng, (4, 32, 36, 64, 100, 384, 768, 1024)), int(rng.integers(1, 257)), _b(rng))


def _probe_geometry(rng):
    g = int(rng.integers(1, 29))
    return int(rng.integers(1, 4)), g, int(rng.integers(1, 5 * g + 2)), _ch(rng, (1, 2, 5, 8, 9, 21, 33, 64, 65, 150, 256))


def _probe_upsample_ce(rng):
    B, g, R, C = _probe_geometry(rng)
    return CE(B, g, R, C, _ch(rng, (0.0, 0.3, 0.3, "rows")), _ch(rng, ("normal", "normal", "large", "const")))


def _bilinear_adjoint(rng):
    return ADJ(*_probe_geometry(rng))


def _probe_wgrad(rng):
    return WG(int(rng.integers(1, 3000)), _ch(rng, (4, 60, 64, 68, 384, 1024)), int(rng.integers(1, 257)), _ch(rng, (0, 0.5)), _b(rng))


def _sgd(rng):
    return SGD(int(rng.integers(1, 100)), int(rng.integers(1, 400000)), 3, _ch(rng, (0.0, 0.9)), _ch(rng, (0.0, 1e-4)))


def _img_resize(rng):
    h, w = int(rng.integers(1, 41)), int(rng.integers(1, 41))
    crop = ""
    if rng.random() < 0.5:
        ch, cw = int(rng.integers(1, h + 1)), int(rng.integers(1, w + 1))
        crop = f"{int(rng.integers(0, h - ch + 1))}/{int(rng.integers(0, w - cw + 1))}/{ch}/{cw}"
    tt = _b(rng)
    return RS(int(rng.integers(1, 5)), h, w, int(rng.integers(1, 41)), int(rng.integers(1, 41)), crop, _b(rng) if tt else 0, tt)


def _img_color(rng):
    mode = _ch(rng, IMG_MODES)
    factor = _ch(rng, (-0.5, -0.07, 0.13, 0.5)) if mode == "hue" else _ch(rng, (0.0, 0.2, 0.9999, 1.0, 1.3, 1.8))
    return COL(int(rng.integers(1, 5)), int(rng.integers(1, 70)), int(rng.integers(1, 70)), mode, factor)


def _img_blur(rng):
    return BL(int(rng.integers(1, 4)), int(rng.integers(1, 40)), int(rng.integers(1, 40)), _ch(rng, (0.1, 0.37, 0.9, 1.3, 2.0)))


# ---- fifth tier: the k-means family beyond the resident pair and the metric counters (checks: tests/_sweep_checks_metric.py)
KM_ASSIGN_STRIDE = 4096 * 256     # kmeans.hpp, km_assign_blocks: at most 4096 workgroups of 256 points - beyond, a workgroup strides
KM_MAX_GRID_Y = 65535             # kmeans.hpp: problems / tiles of one launch
KF_MAXD, KF_MAXN, KF_PREF_LDS, KM_MAX_LDS = 64, 1 << 20, 72 * 1024, 128 * 1024      # kmeans_fit.hip
CS_TILE, CS_MIN_PER_WG, CS_MAX_GRID_X, CS_LDS_CELLS, CS_MAX_C = 2048, 8192, 1024, 16384, 4096      # confusion.hip
DV_OC, DV_LDS_BUDGET, BF_LDS_BUDGET, BF_MAX_R = 4, 64 * 1024, 64 * 1024, 63      # davis.hip, bfscore.hip
DTYPES = ("u8", "i64")


def km_accumulate_blocks(P: int) -> tuple:
    """kmeans.hpp, km_accumulate_blocks -> (blocks, points per block): 128 points per block up to 4096 blocks, ceil(P / 4096) beyond."""
    b = min(4096, max(1, (P + 127) // 128))
    return b, (P + b - 1) // b


def km_tile_default(d: int) -> int:
    """kmeans.hpp, km_tile_default: the centroid rows of d columns that fill 64 KB - the default and the largest tile_k."""
    return KM_MAXKD // d if 1 <= d <= 1024 else 0


def km_tile(d: int, tile_k: int) -> int:
    """kmeans.hip, resolve_tile: 0 = the default."""
    return tile_k if tile_k else km_tile_default(d)


def kf_fit_lds(d: int, k: int, g: int) -> int:
    """kmeans_fit.hip, kf_fit_lds: fp64 sums and fp32 centroids [k][d], g blocks' fp32 sums, k counts."""
    return k * d * (8 + 4 * (1 + g)) + 4 * k


def kf_fit_ok(n: int, d: int, k: int) -> bool:
    """kmeans_fit.hip, kf_fit_shape_ok."""
    return 1 <= d <= KF_MAXD and 1 <= k <= n <= KF_MAXN and kf_fit_lds(d, k, 1) <= KM_MAX_LDS


def kf_fit_group(n: int, d: int, k: int) -> int:
    """kmeans_fit.hip, kf_fit_group: blocks whose fp32 sums one pass holds - what fits 72 KB, at least one, at most all of them."""
    fixed, per = kf_fit_lds(d, k, 0), 4 * k * d
    g = (KF_PREF_LDS - fixed) // per if fixed < KF_PREF_LDS else 0
    return min(max(g, 1), km_accumulate_blocks(n)[0])


def kf_fit_kernel(d: int, offset: int) -> tuple:
    """kmeans_fit.hip, tt_kmeans_fit_batched -> (DREG, VEC): x ``offset`` floats off a 16-byte boundary loads one float at a time."""
    return (16 if d <= 16 else 64), (1 if offset % 4 else (4 if d % 4 == 0 else (2 if d % 2 == 0 else 1)))


def cs_route(Cg: int, Cp: int) -> int:
    """confusion.hip, cs_route: 0 refused, 1 the LDS histogram (up to 16384 cells), 2 global atomics."""
    if not (1 <= Cg <= CS_MAX_C and 1 <= Cp <= CS_MAX_C):
        return 0
    return 1 if Cg * Cp <= CS_LDS_CELLS else 2


def cs_blocks(n: int, Cg: int, Cp: int) -> tuple:
    """confusion.hip, cs_blocks -> (workgroups of one segment, what set the elements per workgroup: "min", "cells" or "spread")."""
    cells = Cg * Cp if cs_route(Cg, Cp) == 1 else 0
    per, why = (CS_MIN_PER_WG, "min") if CS_MIN_PER_WG >= 4 * cells else (4 * cells, "cells")
    spread = (n + CS_MAX_GRID_X - 1) // CS_MAX_GRID_X
    if per < spread:
        per, why = spread, "spread"
    per = min(per, 1 << 31)
    return max(1, (n + per - 1) // per), why


def _shrink(H: int, W: int, lds_of, budget: int):
    """The loop davis_tiling and bf_tiling share: TH 32 -> 16 -> 8, then ow down to 1 -> (TH, ow, shrunk) or None."""
    words = (W + 63) // 64
    tx = (words + 7) // 8
    ow, TH, shrunk = (words + tx - 1) // tx, min(H, 32), False
    while lds_of(TH, ow) > budget:
        shrunk = True
        if TH > 8:
            TH //= 2
        elif ow > 1:
            ow -= 1
        else:
            return None
    return TH, ow, shrunk


def davis_tiling(H: int, W: int, rows: int, oc: int):
    """davis.hip, davis_tiling -> (TH, ow) of an element of ``rows`` rows at ``oc`` objects per pass (None: refused)."""
    t = _shrink(H, W, lambda TH, ow: 4 * oc * (TH + rows) * (ow + 2) * 8, DV_LDS_BUDGET)
    return None if t is None else t[:2]


def bf_tiling(H: int, W: int, R: int):
    """bfscore.hip, bf_tiling -> (TH, ow, whether the shrink loop ran at all)."""
    return _shrink(H, W, lambda TH, ow: 8 * (2 * (TH + 2 * R + 2) * (ow + 2) + 2 * (TH + 2 * R) * (ow + 2) + 6 * TH * ow), BF_LDS_BUDGET)


def tiles_of(H: int, W: int, TH: int, ow: int) -> tuple:
    """(tiles_y, tiles_x) of both counters' launchers."""
    return (H + TH - 1) // TH, ((W + 63) // 64 + ow - 1) // ow


def bf_radius(t) -> int:
    """hip_ops.bf_element_spans: the element radius of the test d < t * t on integer squared distances."""
    r = 0
    while (r + 1) * (r + 1) < float(t) * float(t):
        r += 1
    return r


def KT(P, d, k, tile_k, dup=0) -> dict:
    """dup: 0 none, 1 a random duplicated pair, 2 the pair (tile - 1, tile) either side of the first tile boundary"""
    return dict(P=P, d=d, k=k, tile_k=tile_k, dup=dup)


def KA(P, d, k, tile_k, mode="rand") -> dict:
    return dict(P=P, d=d, k=k, tile_k=tile_k, mode=mode)


def KB(B, N, d, k) -> dict:
    return dict(B=B, N=N, d=d, k=k)


def KF(B, n, d, k, nredo=2, niter=4, offset=0, sep=2.0, empty=0) -> dict:
    """sep: blob centres are N(0, sep^2) per column about which the points are N(0, 1); empty: problem 1 holds every point twice and redo 0
    seeds two clusters on the two copies of one point (tests/test_hip_kmeans_fit.py, test 3)"""
    return dict(B=B, n=n, d=d, k=k, nredo=nredo, niter=niter, offset=offset, sep=sep, empty=empty)


def CSG(S, n, Cg, Cp, dtype="i16", offset=0, ignore="") -> dict:
    """offset: elements pred's view starts into its storage (gt starts offset % 2 elements in); ignore: "" or the ignored gt value"""
    return dict(S=S, n=n, Cg=Cg, Cp=Cp, dtype=dtype, offset=offset, ignore=ignore)


def DV(T, H, W, O, radius, pt="u8", gtt="u8", void=0) -> dict:
    return dict(T=T, H=H, W=W, O=O, radius=radius, pt=pt, gtt=gtt, void=void)


def BFC(P, H, W, t) -> dict:
    return dict(P=P, H=H, W=W, t=t)


def _kmeans_assign_tiled(rng):
    d = _ch(rng, (1, 3, 8, 16, 17, 50, 64, 65, 128, 384))
    k = int(rng.integers(1, 400))
    tile_k = min(_ch(rng, (0, 1, 2, 5, 7, 13)), km_tile_default(d))
    return KT(int(rng.integers(1, 20000)), d, k, tile_k, int(rng.integers(0, 3)) if k > km_tile(d, tile_k) else _b(rng, 0.3) * int(k > 1))


def _kmeans_accumulate_tiled(rng):
    d = _ch(rng, (1, 3, 8, 16, 50, 64, 100, 257, 384))
    return KA(int(rng.integers(1, 30000)), d, int(rng.integers(1, 400)), min(_ch(rng, (0, 1, 3, 7, 64)), km_tile_default(d)), _ch(rng, ("rand", "rand", "skip", "one")))


def _kmeans_assign_batched(rng):
    d = _ch(rng, (1, 3, 16, 17, 50, 64, 65, 128))
    return KB(int(rng.integers(1, 9)), int(rng.integers(1, 3000)), d, int(rng.integers(1, min(km_max_k(d), 200) + 1)))


def _kmeans_fit(rng):
    # (blob centres N(0, 8^2) per column: most draws are valid input as they come - no empty cluster, no near-tie in any fp64 iteration -
    # and where two blobs nearly coincide the check draws the blobs again until its fp64 run proves them valid)
    d = _ch(rng, (1, 2, 3, 6, 12, 16, 17, 50, 64))
    k = int(rng.integers(1, 9))
    return KF(int(rng.integers(1, 4)), int(rng.integers(k, 3000)), d, k, int(rng.integers(1, 3)), int(rng.integers(1, 6)), _ch(rng, (0, 0, 1)), 8.0)


def _confusion_segments(rng):
    Cg, Cp = _ch(rng, ((1, 1), (3, 5), (5, 10), (21, 500), (128, 128), (127, 129), (130, 130)))
    dtype = _ch(rng, ("i16", "i64"))
    return CSG(int(rng.integers(1, 5)), int(rng.integers(1, 70000)), Cg, Cp, dtype, int(rng.integers(0, 8 if dtype == "i16" else 2)), _ch(rng, ("", 0, 255)))


def _davis_counts(rng):
    if rng.random() < 0.5:      # small: the per-pixel definition runs on these (tests/_sweep_checks_metric.py)
        return DV(int(rng.integers(1, 3)), int(rng.integers(1, 25)), int(rng.integers(1, 65)), int(rng.integers(1, 6)), _ch(rng, (0, 1, 2, 2.5, 3)),
                  _ch(rng, DTYPES), _ch(rng, DTYPES), _b(rng))
    return DV(int(rng.integers(1, 4)), int(rng.integers(1, 100)), int(rng.integers(1, 700)), int(rng.integers(1, 7)), _ch(rng, (1, 4, 8, 20)),
              _ch(rng, DTYPES), _ch(rng, DTYPES), _b(rng))


def _bf_counts(rng):
    if rng.random() < 0.5:
        return BFC(int(rng.integers(1, 4)), int(rng.integers(1, 25)), int(rng.integers(1, 65)), _ch(rng, (0, 0.5, 1, 2, 2.5, 5)))
    return BFC(int(rng.integers(1, 4)), int(rng.integers(1, 100)), int(rng.integers(1, 700)), _ch(rng, (1, 2, 5, 16)))


# ---- sixth tier: the operand-preparation kernels (gemm_planes.hip) and the gradient producers' published maxima (common.hpp amax_publish)
# (checks: tests/_sweep_checks_prep.py, on the C twin and on the HIP library)
CONVERT_CAP = 4096 * 256 * 8      # gemm_planes.hip, tt_split_pairs / tt_join_pairs / tt_split_planes: 4096 workgroups x 256 threads x 8 elements - beyond, the stride loop
AMAX_PART, AMAX_PARTS_CAP = 4096, 256      # gemm_planes.hip, split_pairs_dual_impl: n_part = min(ceil(R C / 4096), kAmaxParts)
MULTI_MAXN = 32                   # gemm_planes.hip, PairTable::MAXN: entries per launch of tt_split_pairs_dual_multi
LN_BWD_WG_CAP, LN_MAX_D = 1024, 1024      # rowops.hip, ln_bwd_wgs; 64 * kMaxPerLane
VALUE_KINDS = ("normal", "loguniform", "big", "inf", "nan", "zero", "subnormal")
MULTI_SHAPES = ((1, 1, "t"), (65, 96, "both"), (33, 32, "row"), (64, 64, "t"), (197, 160, "both"), (31, 65, "t"), (130, 128, "row"), (641, 449, "t"),
                (32, 96, "both"), (63, 33, "t"), (1, 32, "row"))      # (R, C, outputs) of entry (i + rot) % 11 of a split_multi table


def ceil_to(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def sd_rpad(p: dict) -> int:
    """Rpad of a split_dual / transpose_pairs case: the default ceil32(R) plus ``rpad`` (0, 32 or 64)."""
    return ceil_to(p["R"], 32) + p["rpad"]


def sd_kernel(p: dict) -> tuple:
    """gemm_planes.hip, split_pairs_dual_impl -> ("rows", SUM) for split_rows_kernel<SUM> (dr && !dt && C % 128 == 0 && 16-byte aligned source and
    row output && TT_SPLIT_ROWS != 0), else ("tile", ROW, SUM) for transpose_pairs_kernel<false, ROW, SUM>."""
    if p["row"] and not p["t"] and p["C"] % 128 == 0 and p["off"] == 0 and p["sr"]:
        return ("rows", bool(p["colsum"]))
    return ("tile", bool(p["row"]), bool(p["colsum"]))


def amax_n_part(n: int) -> tuple:
    """split_pairs_dual_impl -> (n_part, its class: "1", "2..255", "256" or "capped", whether amax_partial_kernel's scalar tail runs)."""
    want = (n + AMAX_PART - 1) // AMAX_PART
    cls = "1" if want == 1 else ("2..255" if want < AMAX_PARTS_CAP else ("256" if want == AMAX_PARTS_CAP else "capped"))
    return min(want, AMAX_PARTS_CAP), cls, n % 4 != 0


def tp_rpad(p: dict) -> int:
    """Rpad of a transpose_planes case: "R" = R itself, "c64" = ceil64(R) (the wrapper's default), "c64+64"."""
    return {"R": p["R"], "c64": ceil_to(p["R"], 64), "c64+64": ceil_to(p["R"], 64) + 64}[p["rpad"]]


def tp_store_branch(rpad: int) -> str:
    """gemm_planes.hip, transpose_planes_kernel: 8-byte stores of four bf16 when Rpad % 4 == 0 (aligned for every row), else one bf16 per lane."""
    return "scalar" if rpad % 4 else ("quad" if rpad % 64 else "quad64")


def multi_entries(p: dict) -> list:
    return [MULTI_SHAPES[(i + p["rot"]) % len(MULTI_SHAPES)] for i in range(p["n"])]


def ln_bwd_plan(rows: int, D: int, off: int = 0) -> tuple:
    """rowops.hip, tt_layernorm_bwd -> (kernel: "vec1" / "vec3" / "vec6" at D 128 / 384 / 768 with 8-byte aligned buffers, else "general";
    workgroups = min(ceil(rows / 8), 1024); rows per workgroup; workgroups that own no row)."""
    wgs = max(1, min((rows + 7) // 8, LN_BWD_WG_CAP))
    rpw = (rows + wgs - 1) // wgs
    kern = {128: "vec1", 384: "vec3", 768: "vec6"}.get(D, "general") if off % 2 == 0 else "general"
    return kern, wgs, rpw, wgs - (rows + rpw - 1) // rpw


def CV(what, n, vals="normal", P=0) -> dict:
    """what: "pairs" (tt_split_pairs and tt_join_pairs of its result) or "planes" (tt_split_planes at P planes)"""
    return dict(what=what, P=P, n=n, vals=vals)


def SD(R, C, t=1, row=0, colsum="", scale="", mag=1.0, vals="normal", rpad=0, off=0, sr=1) -> dict:
    """colsum: "", "fold" (tt_split_pairs_dual) or "parts" (tt_split_pairs_dual_parts); scale: "", "own" (the split's max pass) or "slot" (a
    producer's amax slot); off: floats the source starts off a 16-byte boundary; sr: 0 = TT_SPLIT_ROWS 0 for the call"""
    assert (t or row) and (not row or C % 32 == 0) and not (off and scale)
    return dict(R=R, C=C, rpad=rpad, t=t, row=row, colsum=colsum, scale=scale, mag=mag, vals=vals, off=off, sr=sr)


def SM(n, rot=0) -> dict:
    return dict(n=n, rot=rot)


def TPP(R, C, rpad=0) -> dict:
    return dict(R=R, C=C, rpad=rpad)


def TPL(R, C, rpad="c64", colsum=0) -> dict:
    return dict(R=R, C=C, rpad=rpad, colsum=colsum)


def GA(producer, rows, D, N=0, gscale=1.0, accum=0, off=0) -> dict:
    """producer: "ln_bwd" (N: tokens per frame of a call that drops token 0 - rows are then F (N - 1); 0 = none) or "l2_bwd"; off: floats
    every buffer starts off a 16-byte boundary (1: the 8-byte LayerNorm kernels fall back to the general one)"""
    assert not (N and accum), "refused by tt_layernorm_bwd with an amax slot (include/timetuning_hip.h)"
    return dict(producer=producer, rows=rows, D=D, N=N, gscale=gscale, accum=accum, off=off)


def GAT(producer, F, N, H, gscale=1.0, dslot=0) -> dict:
    """producer: "attn_bwd" or "attn_bwd_pairs" (dslot: max |dout| comes from a producer's slot, not from the call's own max pass)"""
    return dict(producer=producer, F=F, N=N, H=H, gscale=gscale, dslot=dslot)


def GD(M, N, K, gelu=0, gscale=1e-3) -> dict:
    """tt_linear_bwd_data_pairs with an amax slot, dx [M, K] = dy [M, N] @ w [N, K]: "dgrad_general" (no gelu_pre: pairs8_try declines, the
    general kernel runs) or "dgrad_gelu" (x gelu'(pre): the persistent kernels' epilogue where the shape is theirs)"""
    return dict(producer="dgrad_gelu" if gelu else "dgrad_general", M=M, N=N, K=K, gscale=gscale)


def pairs_general_tile(M: int, N: int, K: int, splits: int = 1, ncu: int = 256) -> str:
    """gemm_planes.hip, linear_pairs_impl: the general pair kernel's tile for an output [M, N] - "big" (128 x 128), "wide" (64 x 128), or
    64 x 64 with a ring of four slabs while the grid is under two workgroups per CU ("small4"), of three beyond ("small3")."""
    t128 = ((M + 127) // 128) * (N // 128)
    if N % 128 == 0 and t128 * splits >= 3 * 256:
        return "big"
    if N % 128 == 0 and ((M + 63) // 64) * (N // 128) * splits >= 2 * 256:
        return "wide"
    return "small4" if ((M + 63) // 64) * (N // 64) * splits <= 2 * ncu else "small3"


TWIN_MAX_MACS = 2e7      # the twin's products are naive loops over pair_dot: beyond this many multiply-adds a case runs on the GPU only


def prep_case_on_twin(op: str, p: dict) -> bool:
    if op == "grad_amax" and p["producer"].startswith("dgrad"):
        return p["M"] * p["N"] * p["K"] <= TWIN_MAX_MACS
    if op == "patch_embed":
        return p["F"] * (p["gh"] * p["gw"] + 1) * p["D"] * p["C"] * p["P"] * p["P"] <= TWIN_MAX_MACS
    return True


def PE(mode, F, C, P, gh, gw, D, fmap="", lean=1) -> dict:
    """mode: "f32", "pairs", "planes"; fmap: "" (frame f of F), "rev" (reversed), "repeat" (F draws from a source of three more frames than it
    uses); lean: 0 = TT_PATCH_LEAN 0 for the call (the f32 entry's general kernel on a lean shape)"""
    return dict(mode=mode, F=F, C=C, P=P, gh=gh, gw=gw, D=D, fmap=fmap, lean=lean)


def patch_f32_route(p: dict, tile: int) -> str:
    """gemm_nt_fast.hip, try_launch_patch_embed_fast: the lean kernel at P 16, D % 64 == 0, W % 4 == 0 (and TT_PATCH_LEAN != 0), 128 rows per
    tile where ``tile`` = tt_gemm_tile_choice(F n, D, 1) is 0 or 2, else 64; the general kernel otherwise."""
    if p["P"] != 16 or p["D"] % 64 or (p["gw"] * p["P"]) % 4 or not p["lean"]:
        return "general"
    return "lean128" if tile in (0, 2) else "lean64"


def LNL(Fr, Nt, D, drop=0) -> dict:
    return dict(Fr=Fr, Nt=Nt, D=D, drop=drop)


def _convert(rng):
    if rng.random() < 0.5:
        return CV("pairs", 32 * int(rng.integers(1, 40000)), _ch(rng, VALUE_KINDS))
    return CV("planes", 8 * int(rng.integers(1, 160000)), _ch(rng, VALUE_KINDS), int(rng.integers(1, 4)))


def _split_dual(rng):
    row = _b(rng)
    t = 1 if not row else _b(rng)
    C = 32 * int(rng.integers(1, 10)) if row else int(rng.integers(1, 300))
    scale = _ch(rng, ("", "own", "slot"))
    vals = _ch(rng, ("normal", "normal", "normal", "zero", "big", "inf"))
    return SD(int(rng.integers(1, 700)), C, t, row, _ch(rng, ("", "fold", "parts")), scale, _ch(rng, (1.0, 1e-3, 3e-8, 1e-30)) if vals == "normal" else 1.0,
              vals, _ch(rng, (0, 0, 32, 64)), 0 if scale else _b(rng, 0.2), _b(rng, 0.8))


def _split_multi(rng):
    return SM(int(rng.integers(1, 70)), int(rng.integers(0, len(MULTI_SHAPES))))


def _transpose_pairs(rng):
    return TPP(int(rng.integers(1, 700)), 32 * int(rng.integers(1, 10)), _ch(rng, (0, 32, 64)))


def _transpose_planes(rng):
    return TPL(int(rng.integers(1, 700)), int(rng.integers(1, 300)), _ch(rng, ("R", "c64", "c64+64")), _b(rng))


def _grad_amax(rng):
    if rng.random() < 0.3:
        return GA("l2_bwd", int(rng.integers(1, 300)), _ch(rng, (1, 3, 64, 65, 500, 1024)), gscale=_ch(rng, (1.0, 1e-7)))
    if rng.random() < 0.2:
        return GAT(_ch(rng, ("attn_bwd", "attn_bwd_pairs")), int(rng.integers(1, 3)), int(rng.integers(1, 300)), int(rng.integers(1, 4)), _ch(rng, (1.0, 1e-7)), _b(rng))
    if rng.random() < 0.2:
        return GD(int(rng.integers(1, 700)), 64 * int(rng.integers(1, 4)), 64 * int(rng.integers(1, 7)), _b(rng), _ch(rng, (1e-3, 3e-8)))
    N = _ch(rng, (0, 0, 2, 5, 17))
    F = int(rng.integers(1, 40))
    return GA("ln_bwd", F * (N - 1) if N else int(rng.integers(1, 600)), _ch(rng, (1, 63, 64, 65, 96, 128, 384, 768, 1000)), N, _ch(rng, (1.0, 1e-7)),
              0 if N else _b(rng), _b(rng, 0.3))


def _patch_embed(rng):
    mode = _ch(rng, ("f32", "pairs", "planes"))
    P = _ch(rng, (4, 8, 16))
    C = _ch(rng, [c for c in (1, 2, 3, 4) if (c * P * P) % (64 if mode == "planes" else (32 if mode == "pairs" else 1)) == 0])
    return PE(mode, int(rng.integers(1, 5)), C, P, int(rng.integers(1, 6)), int(rng.integers(1, 6)), _ch(rng, (64, 128, 192)), _ch(rng, ("", "rev", "repeat")))


def _layernorm_long(rng):
    return LNL(int(rng.integers(1, 9)), int(rng.integers(2, 40)), _ch(rng, (64, 96, 128, 384, 768, 1000)), _b(rng))


DRAW = {"linear_f32": _linear_f32, "linear_pairs": _linear_pairs, "linear_planes": _linear_planes, "bwd_pairs": _bwd_pairs,
        "layernorm": _layernorm, "l2norm": _l2norm, "attention": _attention, "ce": _ce, "sinkhorn": _sinkhorn,
        "sinkhorn_from_q": _sinkhorn_from_q, "sinkhorn_local": _sinkhorn_local, "queue_push": _queue_push}
STEP_OPS = tuple(DRAW)      # the first tier: the kernels of the training step
# (appended: the table draws op by op from one generator, so the first tier's cases - and their ids - stay what they were)
DRAW.update({"kmeans_assign": _kmeans_assign, "kmeans_accumulate": _kmeans_accumulate, "col_moments": _col_moments,
             "upsample_tokens": _upsample("C"), "upsample_argmax_f32": _upsample("K"), "upsample_argmax": _upsample("K"),
             "confusion_counts": _confusion_counts, "adamw": _adamw, "elementwise": _elementwise, "foreground_mask": _foreground_mask,
             "pos_embed": _pos_embed})
EVAL_OPS = tuple(DRAW)[len(STEP_OPS):]
# (appended again: the third tier draws after the first two)
DRAW.update({"label_prop": _label_prop, "label_prop_grid": _label_prop_grid, "upsample_argmax_hw": _upsample_argmax_hw})
PROP_OPS = tuple(DRAW)[len(STEP_OPS) + len(EVAL_OPS):]
# (and again: the fourth tier draws after the first three)
DRAW.update({"probe_logits": _probe_logits, "probe_upsample_ce": _probe_upsample_ce, "bilinear_adjoint": _bilinear_adjoint,
             "probe_wgrad": _probe_wgrad, "sgd": _sgd, "img_resize": _img_resize, "img_color": _img_color, "img_blur": _img_blur})
HEAD_OPS = tuple(DRAW)[len(STEP_OPS) + len(EVAL_OPS) + len(PROP_OPS):]
# (and once more: the fifth tier draws after the first four)
DRAW.update({"kmeans_assign_tiled": _kmeans_assign_tiled, "kmeans_accumulate_tiled": _kmeans_accumulate_tiled,
             "kmeans_assign_batched": _kmeans_assign_batched, "kmeans_fit": _kmeans_fit, "confusion_segments": _confusion_segments,
             "davis_counts": _davis_counts, "bf_counts": _bf_counts})
METRIC_OPS = tuple(DRAW)[len(STEP_OPS) + len(EVAL_OPS) + len(PROP_OPS) + len(HEAD_OPS):]
# (and the sixth tier after the first five)
DRAW.update({"convert": _convert, "split_dual": _split_dual, "split_multi": _split_multi, "transpose_pairs": _transpose_pairs,
             "transpose_planes": _transpose_planes, "patch_embed": _patch_embed, "grad_amax": _grad_amax, "layernorm_long": _layernorm_long})
OPS = tuple(DRAW)
PREP_OPS = OPS[len(STEP_OPS) + len(EVAL_OPS) + len(PROP_OPS) + len(HEAD_OPS) + len(METRIC_OPS):]

COUNTS = {"linear_f32": 6, "linear_pairs": 8, "linear_planes": 4, "bwd_pairs": 6, "layernorm": 5, "l2norm": 3, "attention": 6, "ce": 3,
          "sinkhorn": 6, "sinkhorn_from_q": 3, "sinkhorn_local": 3, "queue_push": 3,
          "kmeans_assign": 4, "kmeans_accumulate": 4, "col_moments": 3, "upsample_tokens": 3, "upsample_argmax_f32": 3, "upsample_argmax": 3,
          "confusion_counts": 3, "adamw": 3, "elementwise": 3, "foreground_mask": 4, "pos_embed": 3,
          "label_prop": 6, "label_prop_grid": 4, "upsample_argmax_hw": 4,
          "probe_logits": 4, "probe_upsample_ce": 4, "bilinear_adjoint": 3, "probe_wgrad": 4, "sgd": 3, "img_resize": 4, "img_color": 4,
          "img_blur": 3,
          "kmeans_assign_tiled": 4, "kmeans_accumulate_tiled": 4, "kmeans_assign_batched": 3, "kmeans_fit": 4, "confusion_segments": 4,
          "davis_counts": 4, "bf_counts": 4,
          "convert": 4, "split_dual": 4, "split_multi": 3, "transpose_pairs": 3, "transpose_planes": 4, "patch_embed": 4, "grad_amax": 4, "layernorm_long": 3}

# The route boundaries, pinned (tests/test_sweep_routes.py names the rule each one reaches)
PINNED = {
    "linear_f32": [
        # every tile of tt_linear_fwd_route, on the lean whole-tile kernel (K % 16 == 0) and the general one: 64x64, 128x64, 128x128, 64x128
        dict(M=1, N=64, K=20, act=0, res=0), dict(M=1, N=64, K=48, act=1, res=1), dict(M=16281, N=72, K=20, act=1, res=0),
        dict(M=8067, N=256, K=48, act=0, res=1), dict(M=16281, N=200, K=20, act=0, res=1), dict(M=16281, N=256, K=48, act=1, res=0),
        dict(M=5403, N=768, K=20, act=0, res=0), dict(M=5403, N=768, K=48, act=1, res=1),
        # ragged N beside whole 64-wide tiles; K < 16
        dict(M=130, N=72, K=20, act=1, res=1), dict(M=257, N=200, K=256, act=1, res=0), dict(M=70, N=700, K=1, act=0, res=1),
    ],
    "linear_pairs": [
        # the persistent kernel: half tiles (R = 1, rem 41), round-robin (R = 1, rem 200 > half the CUs), K-split (R = 1, rem 44, K 1536)
        dict(M=25216, N=384, K=384, epi="y"), dict(M=25216, N=384, K=384, epi="pairs_gelu"),
        dict(M=29000, N=512, K=96, epi="y_res"), dict(M=12800, N=768, K=1536, epi="y"),
        # every output combination on the general kernel; M < 256; too few tiles for the persistent kernel
        dict(M=1, N=64, K=32, epi="y"), dict(M=255, N=128, K=96, epi="y_pairs"), dict(M=591, N=256, K=128, epi="y_pairs_gelu_pre"),
        dict(M=300, N=128, K=96, epi="y_res"), dict(M=6272, N=256, K=512, epi="pairs_gelu_pre"), dict(M=777, N=320, K=416, epi="pairs_gelu"),
    ],
    "linear_planes": [
        dict(P=1, M=25216, N=768, K=768, act=0, res=1), dict(P=3, M=25216, N=384, K=384, act=0, res=0), dict(P=3, M=591, N=128, K=64, act=1, res=0),
        dict(P=1, M=1, N=64, K=64, act=0, res=0),
    ],
    "bwd_pairs": [
        # persistent data gradient (route 8 of dx [M, K] = dy [M, N] @ w) on both weight-gradient routes and both gradient magnitudes
        dict(M=6304, N=384, K=768, gelu=1, tn=1, mag=3e-8), dict(M=6299, N=1536, K=384, gelu=0, tn=0, mag=1e-3),
        dict(M=6304, N=384, K=1536, gelu=1, tn=0, mag=3e-8), dict(M=12600, N=128, K=384, gelu=0, tn=1, mag=1e-3),
        # general data gradient; the transposed-pair weight gradient because the shape is not the TN kernel's; M < 32
        dict(M=45, N=128, K=256, gelu=1, tn=1, mag=1e-3), dict(M=591, N=192, K=320, gelu=0, tn=1, mag=3e-8), dict(M=7, N=64, K=64, gelu=1, tn=0, mag=1e-3),
    ],
    "layernorm": [
        dict(Fr=1, Nt=2, D=64, drop=1, pairs=1), dict(Fr=3, Nt=197, D=384, drop=0, pairs=1), dict(Fr=2, Nt=17, D=1000, drop=1, pairs=0),
        dict(Fr=5, Nt=3, D=96, drop=0, pairs=1),
    ],
    "l2norm": [dict(rows=1, D=1, zero_row=1), dict(rows=700, D=256, zero_row=1), dict(rows=5, D=1024, zero_row=0)],
    "attention": [
        dict(Fr=1, N=1, H=1, flash=0), dict(Fr=2, N=256, H=2, flash=0), dict(Fr=1, N=257, H=1, flash=0), dict(Fr=2, N=256, H=1, flash=1),
        dict(Fr=1, N=65, H=3, flash=1), dict(Fr=1, N=897, H=2, flash=0), dict(Fr=43, N=197, H=6, flash=0),
    ],
    "ce": [dict(rows=37, K=K, weighted=int(i % 2)) for i, K in enumerate(CE_K)],
    "sinkhorn": [
        # KPL 4 / 8 either side of K = 256; workgroup counts below the cap, AT it (2048 rows: 64 of 64), beyond it (2049: 64 workgroups of
        # 33 rows - the last one gets none), 50176 rows (the cap of 256)
        dict(B=2048, K=256, iters=3, row0=0, rows_out=2048), dict(B=2049, K=257, iters=1, row0=100, rows_out=1500),
        dict(B=1, K=1, iters=0, row0=0, rows_out=1), dict(B=50176, K=200, iters=2, row0=6272, rows_out=6272),
        # odd B * K (777 x 333; 1001 x 255), KPL 4 and 8, iters 0 and 1, row windows that start past row 0 and end before B, one workgroup,
        # one column, and an output launch of more than 8192 rows
        dict(B=777, K=333, iters=5, row0=0, rows_out=777), dict(B=1001, K=255, iters=1, row0=3, rows_out=997),
        dict(B=6272, K=200, iters=0, row0=2000, rows_out=99), dict(B=33, K=511, iters=10, row0=0, rows_out=33),
        dict(B=1705, K=1, iters=3, row0=0, rows_out=1705), dict(B=50176, K=200, iters=2, row0=0, rows_out=50176),
    ],
    "sinkhorn_from_q": [dict(B=777, K=333, iters=5, transposed=0), dict(B=2049, K=256, iters=0, transposed=1), dict(B=65, K=511, iters=1, transposed=1)],
    "sinkhorn_local": [dict(B=777, K=333, iters=5), dict(B=2049, K=257, iters=0), dict(B=31, K=64, iters=1)],
    "queue_push": [dict(Q=40, D=32, m=1), dict(Q=40, D=32, m=40), dict(Q=1, D=128, m=1)],
    # ---- second tier (cluster.hip, upsample.hip, kmeans.hip, label_prop.hip, rowops.hip, attn_mask.hip)
    "kmeans_assign": [
        # tt_kmeans_assign's dispatch: d <= 16 (16 registers), d <= 64 (64 registers), wider rows read in place - either side of each edge
        dict(P=300, d=1, k=7, dup=0), dict(P=5000, d=16, k=100, dup=0), dict(P=5000, d=17, k=100, dup=0), dict(P=20000, d=64, k=200, dup=0),
        dict(P=20000, d=65, k=250, dup=0), dict(P=3000, d=128, k=100, dup=0), dict(P=257, d=384, k=42, dup=0), dict(P=7001, d=50, k=327, dup=0),
        # k = 1; one point; the last tile of 256 points full, one short, one over; a duplicated centroid (first minimum: the lower index)
        dict(P=1, d=1, k=1, dup=0), dict(P=1, d=9, k=4, dup=1), dict(P=255, d=16, k=1, dup=0), dict(P=256, d=50, k=21, dup=1),
        dict(P=257, d=65, k=21, dup=1), dict(P=12000, d=8, k=30, dup=1),
        # more than 4096 x 256 points: the grid-stride loop (with its __syncthreads) on each of the three kernels
        dict(P=1100000, d=8, k=5, dup=0), dict(P=1048577, d=17, k=3, dup=1), dict(P=1048700, d=65, k=2, dup=0),
        # the largest k * d each kernel takes (km_shape_ok): 16384 floats of centroids; at d = 64 the tile leaves room for 252
        dict(P=3000, d=16, k=1024, dup=0), dict(P=3000, d=64, k=252, dup=0), dict(P=3000, d=128, k=128, dup=0),
    ],
    "kmeans_accumulate": [
        # km_accumulate_blocks: ceil(P / 128) workgroups up to 4096 - beyond P = 524 288 a workgroup sums MORE than 128 points (129 here, and the
        # last 31 workgroups get none; 147 at 600 000); under the cap every workgroup has points
        dict(P=524289, d=8, k=5, mode="rand"), dict(P=600000, d=3, k=7, mode="skip"), dict(P=1100000, d=8, k=5, mode="rand"),
        dict(P=524288, d=2, k=3, mode="rand"), dict(P=7001, d=50, k=21, mode="rand"), dict(P=1, d=1, k=1, mode="rand"),
        dict(P=129, d=16, k=4, mode="rand"),
        # a label that no point carries; every point in one cluster; d > 256 (a thread owns two columns); k * d at the accepted maximum
        dict(P=5000, d=50, k=30, mode="skip"), dict(P=5000, d=64, k=9, mode="one"), dict(P=700000, d=4, k=3, mode="one"),
        dict(P=3000, d=384, k=42, mode="rand"), dict(P=900, d=257, k=2, mode="skip"), dict(P=3000, d=16, k=1024, mode="rand"),
        dict(P=3000, d=64, k=252, mode="rand"), dict(P=20000, d=1, k=16384, mode="rand"),
    ],
    "col_moments": [
        # moments_blocks: ceil(rows / 256) workgroups up to 1024 (262 144 rows); one row (variance exactly 0); one column; a constant
        # column; a column with mean 1e4 and spread 1e-2 (what a one-pass fp32 formula loses)
        dict(rows=1, cols=9, kind="scaled"), dict(rows=300000, cols=3, kind="scaled"), dict(rows=262144, cols=2, kind="offset"),
        dict(rows=262145, cols=1, kind="scaled"), dict(rows=5000, cols=1, kind="scaled"), dict(rows=5000, cols=384, kind="const_col"),
        dict(rows=2000, cols=4, kind="offset"), dict(rows=300, cols=1024, kind="scaled"), dict(rows=257, cols=257, kind="const_col"),
    ],
    "upsample_tokens": [
        # tt_upsample_bilinear_tokens: 64 threads up to C = 64, 128 below 256, 256 from there; g = 1; R = g; R < g; R = 1; ragged ratios
        dict(M=2, g=1, R=5, C=1), dict(M=1, g=14, R=14, C=64), dict(M=3, g=14, R=9, C=65), dict(M=2, g=28, R=1, C=255),
        dict(M=1, g=14, R=56, C=256), dict(M=2, g=3, R=8, C=300), dict(M=1, g=13, R=31, C=50), dict(M=1, g=28, R=60, C=7),
        dict(M=300, g=2, R=3, C=4),
    ],
    "upsample_argmax_f32": [
        dict(M=2, g=1, R=5, K=1), dict(M=1, g=14, R=14, K=64), dict(M=3, g=14, R=9, K=65), dict(M=2, g=28, R=1, K=255),
        dict(M=1, g=14, R=56, K=256), dict(M=2, g=3, R=8, K=300), dict(M=1, g=13, R=31, K=21), dict(M=2, g=14, R=100, K=12),
        dict(M=300, g=2, R=3, K=4),
    ],
    "upsample_argmax": [
        dict(M=2, g=1, R=5, K=1), dict(M=1, g=14, R=14, K=64), dict(M=3, g=14, R=9, K=65), dict(M=2, g=28, R=1, K=255),
        dict(M=1, g=14, R=56, K=256), dict(M=2, g=3, R=8, K=300), dict(M=1, g=13, R=31, K=21), dict(M=2, g=14, R=100, K=8),
        dict(M=300, g=2, R=3, K=4),
    ],
    "confusion_counts": [
        # tt_confusion_counts: the LDS histogram up to C = 96, global atomics beyond; ceil(n / 4096) workgroups up to 2048; labels outside
        # [0, C) - the -1 and 255 of ignored pixels - dropped
        dict(n=1, C=1, stray=0), dict(n=1, C=97, stray=1), dict(n=5000, C=1, stray=1), dict(n=100000, C=96, stray=1), dict(n=100000, C=97, stray=1),
        dict(n=70000, C=300, stray=1), dict(n=2048 * 4096, C=21, stray=0), dict(n=2048 * 4096 + 5, C=7, stray=1), dict(n=2048 * 4096 + 4097, C=300, stray=1),
    ],
    "adamw": [
        # tables of 1, 40 (TT_MAX_TENSORS) and more tensors - through the wrappers' chunks of 40 and through the fused entry's; lengths 1, 255,
        # 257 and `big` round-robin, so that a length-1 tensor shares the grid of one above 1024 x 256 elements; steps 1 and 100 000
        dict(T=1, big=1, step=1, fused=0, gscale=1.0), dict(T=1, big=300001, step=3, fused=1, gscale=0.37), dict(T=40, big=262145, step=1, fused=0, gscale=0.37),
        dict(T=41, big=300001, step=100000, fused=0, gscale=1e-3), dict(T=85, big=1000, step=2, fused=1, gscale=0.37),
        dict(T=81, big=70000, step=100000, fused=1, gscale=1.0), dict(T=4, big=262144, step=5000, fused=0, gscale=1.0),
    ],
    "elementwise": [
        # n & 3 in {0, 1, 2, 3} below 4 and above (tt_ema_update: float4 body, the tail on workgroup 0); n either side of the caps - ema
        # 2048 x 1024, add 4096 x 256, count_mismatch 2048 x 256; rows either side of colsum's 128 chunks of 256
        dict(n=1, rows=1, cols=1), dict(n=2, rows=2, cols=3), dict(n=3, rows=3, cols=64), dict(n=4, rows=5, cols=65), dict(n=5, rows=255, cols=4),
        dict(n=6, rows=256, cols=100), dict(n=7, rows=257, cols=1024), dict(n=100003, rows=32768, cols=7), dict(n=524288, rows=32769, cols=3),
        dict(n=524289, rows=40000, cols=66), dict(n=1048576, rows=100, cols=255), dict(n=1048578, rows=1000, cols=384),
        dict(n=2097152, rows=7, cols=2), dict(n=2097153 + 4096, rows=700, cols=1000), dict(n=3000003, rows=33, cols=33),
    ],
    "foreground_mask": [
        # one workgroup per frame, everything in LDS: g up to 32 (1024 patches); the 7-tap blur reflects over up to 3 pixels, so g >= 4
        dict(F=1, g=4, H=1, hd=4, th=0.65, entry="qkv"), dict(F=3, g=5, H=3, hd=64, th=0.3, entry="qkv"), dict(F=2, g=13, H=6, hd=128, th=0.8, entry="qkv"),
        dict(F=5, g=14, H=12, hd=64, th=0.65, entry="qkv"), dict(F=2, g=31, H=3, hd=4, th=0.3, entry="qkv"), dict(F=2, g=32, H=6, hd=64, th=0.65, entry="qkv"),
        dict(F=300, g=14, H=6, hd=64, th=0.65, entry="qkv"),
        dict(F=1, g=4, H=12, hd=64, th=0.3, entry="probs"), dict(F=4, g=5, H=1, hd=64, th=0.8, entry="probs"), dict(F=3, g=13, H=3, hd=64, th=0.65, entry="probs"),
        dict(F=2, g=14, H=6, hd=64, th=0.3, entry="probs"), dict(F=2, g=31, H=12, hd=64, th=0.65, entry="probs"), dict(F=1, g=32, H=1, hd=64, th=0.8, entry="probs"),
        dict(F=300, g=7, H=3, hd=64, th=0.65, entry="probs"),
    ],
    "pos_embed": [
        # bicubic, taps clamped at the border: gh != gw, one of them 1, down- and up-sampling, D = 4 (one float4 per token)
        dict(g=14, gh=1, gw=7, D=4), dict(g=14, gh=20, gw=1, D=384), dict(g=14, gh=20, gw=14, D=384), dict(g=28, gh=7, gw=9, D=768),
        dict(g=28, gh=30, gw=40, D=4), dict(g=14, gh=30, gw=40, D=768), dict(g=28, gh=14, gw=14, D=384), dict(g=14, gh=13, gw=15, D=64),
    ],
    # ---- third tier (label_prop.hip: lp_route, lp_sims_chunk, lp_chunk and the per-query kernels)
    "label_prop": [
        # lp_route, all six kernels either side of each deciding bound.  Contexts of frame t: 1 + min(t - 1, nl).  nl 2 at fs 5: at most 3
        # contexts (the <3,KT> wave kernels); nl 3 at fs 5: frame 4 has 4 (the clip changes to <8,KT> on its last frame)
        LP(fs=5, nl=2, r=6, K=64), LP(fs=5, nl=3, r=6, K=65, dup=1), LP(fs=5, nl=2, r=6, K=256, dup=1), LP(fs=5, nl=2, r=6, K=257, dup=1),
        LP(fs=5, nl=3, r=6, K=256), LP(fs=5, nl=3, r=6, K=257, dup=1), LP(fs=5, nl=3, K=1),
        # K 512 is the last the wave kernels take (lane + 64 * 7), 513 the first on the workgroup kernel - whatever the window
        LP(fs=5, nl=3, g=7, K=512, dup=1), LP(fs=5, nl=3, g=7, K=513, dup=1), LP(fs=5, nl=2, g=7, K=512), LP(g=1, K=513, bs=5, fs=4, nl=2),
        # window 16 (g = 16 under a large radius: min(2 r + 1, g)) on the wave kernel, 17 (radius 8 on g = 17 and g = 20) on the workgroup kernel
        LP(g=16, r=20, K=7), LP(g=16, r=8, K=7, nl=0), LP(g=17, r=8, K=7, dup=1), LP(g=20, r=8, K=3, fs=2),
        # every slot of the wave kernel full: 16 x 16 x 8 contexts = 2048 candidates
        LP(g=16, r=8, nl=7, fs=9, K=3),
        # n = 4096 is the last grid whose source patch fits 12 bits (wave kernel); g = 65 goes to the workgroup kernel.  At g = 64 three
        # contexts are 192 MB of similarities per target frame: the real 256 MB cap chunks this clip frame by frame, no variable set
        LP(g=64, fs=4, nl=2, K=2), LP(g=64, fs=2, nl=0, D=4, K=2, dup=1), LP(g=65, fs=3, K=2),
        # candidates at the caps.  2048 (32 x 32 x 2): every slot of label_prop_kernel<8> full; 2116 (23 x 23 x 4): the next count any
        # (window, contexts) reaches above 2048 - label_prop_kernel<16>; 4096 (32 x 32 x 4): every slot of <16> full; 5120: refused
        LP(g=32, r=16, fs=3, nl=1, K=3), LP(g=32, r=16, fs=4, nl=1, K=3, dup=1), LP(g=23, r=11, fs=5, nl=3, K=3), LP(g=32, r=16, fs=5, nl=3, K=3, dup=1),
        LP(g=32, r=16, fs=6, nl=4, K=3),
        # lp_sims_chunk's slot regimes, whole and chunked (cap in MB -> chunk length, lp_chunk): nl 0 (slot 0 only); the queue never fills
        # (fs < nl + 2), fills on the last frame (fs = nl + 2), is full for several frames (fs > nl + 2); fs = 2.  One target frame of these
        # shapes is 0.88 - 1.17 MB, so caps of 1 / 3 / 4 MB make chunks of 1 / 2 / 3 frames: starts inside the filling regime, ON
        # t = nl + 2 (nl 1: T 2 -> 1, 3; nl 3: T 2 -> 1, 3, 5, 7; nl 7: T 2 -> ..., 9, 11) and inside the full regime
        LP(bs=8, fs=2, nl=0), LP(bs=8, fs=4, nl=0, cap="1/3"), LP(bs=4, fs=2, nl=1), LP(bs=4, fs=3, nl=1, cap="1"), LP(bs=4, fs=5, nl=1, cap="1/3"),
        LP(bs=2, fs=4, nl=3, cap="1/2"), LP(bs=2, fs=5, nl=3, cap="1/3"), LP(bs=2, fs=8, nl=3, cap="1/3/4", K=21), LP(fs=8, nl=7, cap="3"),
        LP(fs=9, nl=7, cap="3/4"), LP(fs=12, nl=7, cap="3/4", dup=1), LP(bs=2, fs=8, nl=3, cap="3", K=513, prec="bf16"),
        # degenerate sizes: one patch (candidates = contexts < topk; bs * n = 3 is not a multiple of the 4 waves of a workgroup); g 2, g 3;
        # topk 1 and above every total; D 4 (K < 16 in the similarity product), 20 (the general kernel), 64, 384; a ragged batch of 37 clips
        LP(g=1, bs=3, fs=4, nl=2), LP(g=2, fs=4, nl=2, r=1), LP(g=3, bs=3, fs=4, nl=3, r=1, dup=1), LP(g=7, topk=1), LP(g=7, topk=1000, fs=4, nl=2),
        LP(g=7, topk=1000, K=513), LP(D=4), LP(D=20, K=21), LP(D=64, fs=4, nl=2), LP(D=384, K=21), LP(bs=37, g=5, fs=4, nl=2, D=20),
        # precision: the similarities as fp16 pairs' front end hands them over (f16x3) and on bf16 MFMA
        LP(fs=5, nl=3, r=6, K=21, prec="f16x3"), LP(fs=5, nl=3, r=6, K=21, prec="bf16", dup=1), LP(g=17, r=8, K=7, prec="bf16"),
        LP(g=23, r=11, fs=5, nl=3, K=3, prec="f16x3"), LP(D=384, K=21, prec="bf16"), LP(bs=37, g=5, fs=4, nl=2, D=20, prec="bf16"),
    ],
    "label_prop_grid": [
        # gh != gw, 1 x n and n x 1; radius 0 (no window) and beyond the grid; nl 0 and 7; topk above the candidates (the `total >= topk`
        # branch) and below; K 1 and above 256 (a thread owns two channels); 30 x 30 at radius 12 with 8 contexts: 5000 candidates
        LPG(), LPG(gh=9, gw=5, dup=1), LPG(gh=1, gw=9, r=3), LPG(gh=9, gw=1, r=3, nl=0), LPG(gh=1, gw=1, fs=3, nl=1), LPG(r=0), LPG(gh=7, gw=23, r=0, dup=1),
        LPG(r=30), LPG(fs=9, nl=7), LPG(fs=3, nl=0, bs=3), LPG(gh=2, gw=3, nl=0, topk=10), LPG(gh=2, gw=3, nl=0, topk=6), LPG(K=1), LPG(K=300, dup=1),
        LPG(gh=30, gw=30, r=12, fs=9, nl=7, K=3), LPG(gh=14, gw=14, r=6, fs=5, nl=3, K=21, prec="bf16"), LPG(D=4, prec="f16x3"),
    ],
    "upsample_argmax_hw": [
        # output smaller than the grid, equal to it, larger; H or W of 1; K 1, 64, 65; M 1 and above; a duplicated channel (first index wins)
        dict(M=1, gh=9, gw=5, K=21, H=4, W=3, dup=0), dict(M=3, gh=7, gw=23, K=3, H=7, W=23, dup=1), dict(M=2, gh=5, gw=9, K=64, H=40, W=77, dup=1),
        dict(M=1, gh=5, gw=9, K=65, H=1, W=30, dup=1), dict(M=2, gh=9, gw=5, K=7, H=30, W=1, dup=0), dict(M=1, gh=1, gw=1, K=1, H=3, W=2, dup=0),
        dict(M=3, gh=14, gw=1, K=2, H=9, W=9, dup=0), dict(M=1, gh=30, gw=53, K=5, H=480, W=848, dup=0), dict(M=2, gh=6, gw=10, K=200, H=96, W=31, dup=1),
    ],
    # ---- fourth tier (linear_probe.hip, image_ops.hip)
    "probe_logits": [
        # probe_logits_kernel<1,4> (C <= 64: 64 rows per workgroup), <2,2> (C <= 128: 32 rows) and <4,2> (ct = 3 and 4: 32 rows), the last
        # workgroup of each one short of whole, whole, one over and alone; D below, at and off the 32-column stage; bias present and NULL
        PL(1, 4, 1, 0), PL(63, 32, 63, 1), PL(64, 36, 64, 0), PL(65, 384, 64, 1), PL(1001, 1024, 1, 1),
        PL(31, 36, 65, 1), PL(32, 384, 128, 0), PL(33, 4, 128, 1), PL(1001, 32, 65, 0), PL(64, 1024, 128, 1),
        PL(31, 4, 129, 0), PL(32, 36, 192, 1), PL(33, 384, 192, 0), PL(1001, 32, 129, 1),
        PL(31, 384, 193, 1), PL(32, 1024, 256, 0), PL(33, 36, 256, 1), PL(65, 4, 193, 0), PL(1001, 384, 256, 1), PL(63, 32, 256, 0), PL(1, 1024, 256, 1),
    ],
    "probe_upsample_ce": [
        # geometry: down-sampling (R < g: low-res rows and columns that no pixel reads), R = g, R just above g, one token, one pixel,
        # the largest mask at 2 classes, the LDS maximum (64 x 64 x 256 accumulators, R 1024) with 1 % of the pixels valid
        CE(2, 28, 14, 5), CE(1, 28, 9, 21, 0.0), CE(2, 64, 1, 5, 0.0), CE(1, 5, 4, 9, 0.3, "large"), CE(2, 14, 14, 21), CE(1, 28, 29, 5, 0.0),
        CE(3, 1, 1, 5, 0.0), CE(2, 1, 7, 17), CE(1, 64, 1024, 2), CE(1, 64, 1024, 256, 0.99),
        # lanes per pixel 1, 2, 4, 8, 16, 32 either side of each edge (gather_tp_log2), every kind of logits and share of ignored pixels
        CE(2, 7, 20, 1, 0.3), CE(1, 7, 20, 1, 0.0, "const"), CE(2, 7, 20, 8, 0.0, "large"), CE(2, 7, 20, 9, "rows"), CE(3, 7, 20, 16, 0.3, "const"),
        CE(2, 7, 20, 17, 0.0, "const"), CE(2, 7, 20, 32, 0.3, "large"), CE(2, 7, 20, 33, "rows", "const"), CE(2, 7, 20, 64, 0.0, "const"), CE(2, 7, 20, 65, 0.3),
        CE(2, 7, 20, 128, "rows", "large"), CE(2, 7, 20, 129, 0.0, "const"), CE(2, 7, 20, 256, 0.3), CE(1, 7, 20, 256, 0.0, "large"),
        # nothing valid (NaN loss, zero gradient); whole mask rows ignored (workgroups that own no valid pixel); more than one pixel chunk
        # with a ragged last one (R 300 at 256 pixels per chunk, 100 at 64); three images
        CE(2, 7, 20, 5, 1.0), CE(1, 14, 14, 256, 1.0, "large"), CE(2, 14, 56, 21, "rows"), CE(1, 14, 300, 5), CE(3, 28, 100, 21),
        CE(1, 14, 150, 12, 0.0), CE(1, 7, 50, 40),          # ... R 150 at 128 pixels per chunk, 50 at 32
    ],
    "bilinear_adjoint": [
        # the same geometry and class counts; the big masks at small C only (d_hi is B * R * R * C floats); 64 x 64 x 256 accumulators
        ADJ(2, 28, 14, 5), ADJ(1, 28, 9, 21), ADJ(2, 64, 1, 5), ADJ(1, 5, 4, 9), ADJ(2, 14, 14, 21), ADJ(1, 28, 29, 5), ADJ(3, 1, 1, 5),
        ADJ(2, 1, 7, 17), ADJ(1, 64, 1024, 2), ADJ(1, 64, 64, 256), ADJ(1, 14, 300, 5), ADJ(3, 28, 100, 21), ADJ(1, 14, 150, 12), ADJ(1, 7, 50, 40),
        ADJ(2, 7, 20, 1), ADJ(2, 7, 20, 8), ADJ(2, 7, 20, 9), ADJ(2, 7, 20, 16), ADJ(2, 7, 20, 17), ADJ(2, 7, 20, 32), ADJ(2, 7, 20, 33),
        ADJ(2, 7, 20, 64), ADJ(2, 7, 20, 65), ADJ(2, 7, 20, 128), ADJ(2, 7, 20, 129), ADJ(2, 7, 20, 256),
    ],
    "probe_wgrad": [
        # wgrad_split: one split (rows <= 32); 33 rows (two splits, the last of one row); splits capped by the 32-row chunks; capped by
        # 1024 / tiles (47 040 rows of the probe's own shape: 164 splits of 288, the last of 96; 64 tiles: 10 splits of 64, the last of 24;
        # 16 splits of 512: the longest fp32 runs here); C and D off the 64-wide tiles; scale and db each present and NULL
        WG(1, 4, 1, 0.5, 1), WG(32, 60, 63, 0, 0), WG(17, 68, 65, 0.5, 1), WG(33, 4, 256, 0.5, 1), WG(1000, 60, 63, 0.5, 0),
        WG(100, 68, 65, 0, 1), WG(47040, 384, 21, 0.5, 1), WG(600, 1024, 256, 0, 1), WG(8192, 1024, 256, 0.5, 1), WG(2049, 1024, 1, 0, 0),
    ],
    "sgd": [
        # tables of 1, 40 (TT_MAX_TENSORS) and - through the wrapper's chunks - 41 and 85 tensors; lengths 1, 255, 257 and `big` round-robin
        # (a one-element tensor beside one above 1024 x 256 elements: the grid-stride loop); momentum and weight decay each on and off
        SGD(1, 300001), SGD(1, 1, 3, 0.0, 0.0), SGD(40, 262145, 3, 0.9, 0.0), SGD(41, 300001, 3, 0.0, 1e-4), SGD(85, 262145), SGD(4, 262144, 3, 0.0, 0.0),
        SGD(40, 1000, 1),
    ],
    "img_resize": [
        # one-pixel sides; 1 -> N and N -> 1 (a thousand taps per output pixel); an axis that keeps its size, each way and both; crops that
        # end on the right and bottom border, one-pixel crops; the flip at odd and even widths; 300 tiny frames; uint8 and float outputs
        RS(1, 1, 1, 5, 3), RS(2, 7, 1, 3, 4, to_tensor=1), RS(2, 1, 9, 4, 2, flip=1, to_tensor=1), RS(1, 1000, 3, 1, 3), RS(1, 3, 1000, 3, 1, to_tensor=1),
        RS(2, 9, 7, 9, 4), RS(2, 9, 7, 5, 7, flip=1, to_tensor=1), RS(1, 6, 5, 6, 5, flip=1, to_tensor=1), RS(1, 6, 5, 6, 5),
        RS(2, 20, 30, 8, 8, "5/11/15/19", to_tensor=1), RS(2, 20, 30, 4, 5, "19/29/1/1"), RS(1, 20, 30, 3, 3, "0/0/1/1", flip=1, to_tensor=1),
        RS(2, 20, 30, 5, 19, "3/11/10/19"), RS(1, 20, 30, 15, 19, "5/11/15/19"), RS(2, 20, 30, 15, 7, "5/0/15/30", to_tensor=1),
        RS(1, 12, 12, 8, 8, flip=1, to_tensor=1), RS(300, 3, 4, 2, 5, flip=1, to_tensor=1), RS(300, 2, 2, 3, 3, "1/1/1/1"), RS(1, 1000, 1, 1, 1),
    ],
    "img_color": [
        # every mode on one pixel; the contrast mean above gray_sum_kernel's cap of 524 288 pixels (its grid-stride loop) and exactly at it;
        # five frames of differing brightness (one mean each); factors 0, 0.9999, 1 and 1.8; hue shifts at both ends; the last frame of
        # every clip of two or more is exact grays
        COL(1, 1, 1, "gray", 1.0), COL(1, 1, 1, "brightness", 1.8), COL(1, 1, 1, "contrast", 0.0), COL(1, 1, 1, "saturation", 0.9999), COL(1, 1, 1, "hue", 0.5),
        COL(1, 600, 1024, "contrast", 1.8), COL(2, 512, 1024, "contrast", 0.9999), COL(5, 33, 47, "contrast", 0.0), COL(5, 33, 47, "contrast", 1.8),
        COL(3, 40, 31, "contrast", 1.0), COL(2, 40, 31, "brightness", 0.0), COL(2, 40, 31, "brightness", 0.9999), COL(2, 40, 31, "saturation", 1.8),
        COL(2, 40, 31, "saturation", 0.0), COL(2, 40, 31, "saturation", 1.0), COL(3, 40, 31, "hue", -0.5), COL(3, 40, 31, "hue", 0.5),
        COL(2, 17, 1, "hue", 0.13), COL(300, 3, 2, "gray", 1.0), COL(300, 2, 3, "contrast", 1.8),
    ],
    "img_blur": [
        # lines of 1, 2 and 3 pixels at radius 2.0 (box radius 1 and the far taps at +-2: at or beyond the line), each direction; 1 x 53
        # and 37 x 1; the smallest and the largest radius of the training transform
        BL(2, 5, 1, 2.0), BL(2, 1, 5, 2.0), BL(1, 2, 7, 2.0), BL(1, 7, 2, 2.0), BL(1, 3, 3, 2.0), BL(1, 1, 1, 2.0), BL(2, 1, 53, 2.0), BL(2, 37, 1, 2.0),
        BL(1, 1, 53, 0.1), BL(1, 37, 1, 0.1), BL(300, 3, 2, 2.0), BL(2, 37, 53, 0.1),
    ],
    # ---- fifth tier (kmeans.hip: the tiled pair and the batched assignment; kmeans_fit.hip; confusion.hip; davis.hip; bfscore.hip)
    "kmeans_assign_tiled": [
        # km_assign_blocks: beyond 4096 x 256 points the workgroups stride - on <16>, <0> and <64> with several tiles forced by a small tile
        # (the point tile is staged again, the centroid tiles are reloaded), and on <0> with ONE tile (`resident`: kept over the strides)
        KT(1048577, 17, 7, 3, 1), KT(1048700, 65, 5, 2), KT(1100000, 8, 9, 4, 2), KT(1048700, 65, 5, 0), KT(1100000, 8, 9, 0, 1), KT(1048577, 17, 7, 0),
        # a last tile of 1, 2, 3 and 5 centroids behind whole tiles of 8: the 4-wide block and its tail, on each kernel
        KT(3000, 16, 9, 8), KT(3000, 50, 10, 8, 2), KT(3000, 65, 11, 8), KT(3000, 16, 13, 8, 2), KT(700, 128, 13, 8, 2),
        # the first minimum across a tile boundary (dup 2) on each kernel; tile_k 1 (every centroid its own tile)
        KT(2000, 8, 40, 7, 2), KT(2000, 50, 40, 7, 2), KT(2000, 100, 40, 7, 2), KT(1000, 17, 9, 1, 2), KT(1000, 3, 5, 1, 1),
        # k one above the default tile (two tiles, the last of one centroid) at d 16, 64 and 128: beyond what the resident pair takes - at
        # d 64 also with enough points for the excuse rule to allow a label (one per 10 000)
        KT(3000, 16, 1025, 0, 2), KT(3000, 64, 257, 0, 2), KT(3000, 128, 129, 0, 2), KT(12000, 64, 257, 0, 2),
        # the last workgroup of 256 points one short, whole, one over; one point; one tile that holds every centroid; d 1024
        KT(255, 16, 9, 4), KT(256, 50, 9, 4, 1), KT(257, 65, 9, 4), KT(1, 9, 4, 3), KT(5000, 50, 21, 0, 1), KT(300, 1024, 17, 16, 2),
        KT(5000, 8, 30, 0, 1), KT(700, 100, 30, 0, 1),
    ],
    "kmeans_accumulate_tiled": [
        # more than 65 535 tiles: the launcher's t0 loop (65 541 tiles of one cluster: launches of 65 535 and of 6)
        KA(3000, 1, 65541, 1),
        # km_accumulate_blocks beyond P = 524 288: 129 points per block (31 blocks without a point) and 147; exactly at the cap
        KA(524289, 8, 5, 2), KA(600000, 3, 7, 3, "skip"), KA(524288, 2, 3, 1), KA(700000, 4, 3, 2, "one"),
        # d 257 (a thread owns two columns) with k above the tile; a last tile of one cluster; every mode; the default tile beyond the
        # resident limit; one point; tile_k above k
        KA(900, 257, 70, 63, "skip"), KA(5000, 50, 22, 7), KA(5000, 64, 9, 4, "one"), KA(5000, 50, 30, 7, "skip"), KA(3000, 16, 1025, 0),
        KA(3000, 128, 129, 0, "skip"), KA(1, 1, 1, 0), KA(129, 16, 4, 64), KA(7001, 50, 500, 0),
    ],
    "kmeans_assign_batched": [
        # launch_assign: the three kernels at B = 3 with a ragged last workgroup; more than 65 535 problems (the y0 loop); the largest
        # resident k of each kernel; one point per problem
        KB(3, 700, 16, 9), KB(3, 700, 50, 21), KB(3, 700, 128, 40), KB(65538, 2, 3, 2), KB(2, 300, 16, 1024), KB(2, 300, 64, 252),
        KB(2, 300, 128, 128), KB(5, 1, 17, 3),
    ],
    "kmeans_fit": [
        # kmeans_fit_kernel<16,2>: d even, no multiple of 4, at most 16; the other five instantiations; x 4 bytes off a 16-byte boundary
        # at d % 4 == 0 (VEC 1) beside the aligned run of the same case (VEC 4): equal bit for bit
        KF(3, 257, 2, 3), KF(2, 300, 6, 5), KF(2, 300, 10, 4), KF(2, 515, 14, 7), KF(2, 300, 12, 5), KF(2, 300, 12, 5, offset=1),
        KF(2, 700, 64, 9), KF(2, 700, 64, 9, offset=1), KF(2, 129, 3, 2), KF(2, 400, 17, 5), KF(2, 400, 50, 10), KF(2, 400, 16, 5),
        # kf_fit_group: 1 with whole and ragged block counts (6 and 11 blocks: every pass is one block); 3 with 8 blocks (a last pass of
        # two); all blocks in one pass.  The LDS maxima at d 64 and d 50; d 14 at k 300 (group 1 at a small d)
        KF(2, 700, 64, 127, niter=3), KF(1, 1300, 50, 80, niter=3), KF(2, 1000, 50, 60, niter=3), KF(1, 1100, 50, 60, nredo=1, niter=3),
        KF(1, 900, 50, 163, nredo=1, niter=3),
        KF(1, 1500, 14, 300, nredo=1, niter=3),
        # fewer points than threads; n = k; one point; more than 128 points per block (147 and 256: the fit's longest fp32 runs; blobs 16
        # deviations apart, so that none of a million points lies within KM_GAP of a bisector)
        KF(3, 100, 5, 4), KF(2, 37, 8, 37, nredo=1), KF(3, 1, 1, 1, nredo=1, niter=2), KF(1, 600000, 2, 3, 1, 3, sep=16.0),
        KF(1, 1048576, 1, 2, 1, 3, sep=16.0),
        # more problems than one launch carries (the wrapper's chunks of 65 535); an empty cluster on one (problem, redo) only
        KF(65538, 2, 1, 1, 1, 1), KF(3, 300, 17, 5, 2, 4, empty=1),
    ],
    "confusion_segments": [
        # cs_blocks: one workgroup up to 8192 elements, two from 8193; four elements per LDS cell (21 x 500: 42 000 / 42 001); beyond
        # 1024 x 8192 elements the workgroups take ceil(n / 1024) each - on the LDS route and on the global one
        CSG(2, 8192, 5, 10), CSG(2, 8193, 5, 10, "i64", 0, 0), CSG(2, 42000, 21, 500), CSG(2, 42001, 21, 500, "i16", 0, 255),
        CSG(1, 9000000, 3, 7), CSG(1, 8500000, 130, 130, "i16", 3, 0),
        # pred 1 ... 7 elements off a 16-byte boundary (int16), 1 (int64), with SEVERAL workgroups per segment: a head and a tail on
        # workgroup 0 beside the strip loop all of them share - LDS route, then global
        *[CSG(3, 50176, 5, 10, "i16", o, 0 if o % 2 else "") for o in range(1, 8)], CSG(3, 50176, 5, 10, "i64", 1, 255),
        *[CSG(3, 50176, 130, 130, "i16", o, 0 if o % 2 else "") for o in range(1, 8)], CSG(3, 50176, 130, 130, "i64", 1),
        # fewer than 8 elements (no strip); a head longer than the segment; odd n at S > 1 (int16 segments that start 2-byte aligned)
        CSG(3, 1, 3, 5), CSG(2, 7, 3, 5, "i64", 1), CSG(3, 3, 3, 5, "i16", 1), CSG(2, 5, 130, 130, "i16", 2), CSG(5, 4097, 127, 129, "i16", 0, 0),
        CSG(4, 777, 1, 1, "i64", 0, 0), CSG(2, 1000, 300, 7, "i16", 3, 255),
    ],
    "davis_counts": [
        # davis_tiling: the 127-row element at four objects per pass leaves TH 8, ow 1 (9 x 5 tiles); W 512 / 513 (one tile column of 8
        # words / two of 5); 81 rows at TH 8, ow 3 with a second pass of one object; H < 8; 3 x 3 tiles on three frames
        DV(2, 70, 300, 4, 63, "u8", "i64", 1), DV(2, 40, 513, 4, 8, "i64", "u8", 0), DV(2, 40, 512, 4, 8, "u8", "u8", 1),
        DV(2, 40, 600, 5, 40, "i64", "i64", 1), DV(2, 6, 200, 4, 63, "i64", "u8", 1), DV(3, 70, 1100, 3, 2, "u8", "i64", 0),
        # the remaining classes of davis_tiling: TH 32 -> 16 at all eight words; TH 32 -> 16 -> 8 at all eight words; H <= 8 with ow 8 -> 3;
        # H = 16 (one halving, then ow) with ow 8 -> 3 and with ow 5 -> 1
        DV(1, 40, 300, 4, 24, "u8", "u8", 0), DV(1, 40, 512, 4, 20, "i64", "u8", 1), DV(1, 6, 512, 4, 40, "u8", "i64", 0),
        DV(1, 16, 512, 4, 40, "i64", "i64", 0), DV(1, 16, 300, 4, 63, "u8", "u8", 1),
        # every dtype pair with and without void on small frames (the per-pixel definition runs on these); one pixel; an even element
        DV(2, 17, 23, 3, 1, "u8", "u8", 0), DV(2, 24, 64, 5, 2, "i64", "i64", 0), DV(1, 9, 33, 2, 3, "u8", "i64", 1), DV(2, 5, 7, 2, 10, "i64", "u8", 0),
        DV(1, 1, 1, 1, 0, "u8", "u8", 1), DV(1, 20, 40, 2, 2.5, "i64", "i64", 1),
    ],
    "bf_counts": [
        # 3 x 3 tiles on three pairs; R 63 at W 512 / 513; R 30 on two tile columns; H < 32 with W > 512
        BFC(3, 70, 1100, 2), BFC(2, 40, 513, 64), BFC(2, 40, 512, 64), BFC(2, 40, 600, 31), BFC(2, 20, 700, 5),
        # small maps (the per-pixel definition runs on these): one pixel, a row, a column, t 0 and 0.5 (no match but the pixel itself)
        BFC(3, 1, 1, 2), BFC(2, 1, 60, 2), BFC(2, 24, 1, 2.5), BFC(2, 13, 29, 0), BFC(2, 13, 29, 0.5), BFC(2, 24, 64, 5), BFC(1, 20, 33, 16),
    ],
    # ---- sixth tier (gemm_planes.hip: the conversions, the dual split and its table form, the two transposes; rowops.hip: the backward
    # producers' maxima)
    "convert": [
        # one pair group / one 8-element chunk with every kind of value; the grid cap of 8 388 608 elements exactly and one group / chunk
        # beyond it (the stride loop: workgroup 0's first thread comes round again), at 1, 2 and 3 planes
        *[CV("pairs", 32, v) for v in VALUE_KINDS], *[CV("planes", 8, v, P) for v, P in zip(VALUE_KINDS, (1, 2, 3, 1, 2, 3, 3))],
        CV("pairs", CONVERT_CAP), CV("pairs", CONVERT_CAP + 32, "loguniform"), CV("planes", CONVERT_CAP, "normal", 1),
        CV("planes", CONVERT_CAP + 8, "loguniform", 3), CV("planes", CONVERT_CAP + 8, "subnormal", 2), CV("pairs", 4128, "subnormal"),
        CV("pairs", 96000, "big"), CV("pairs", 96000, "inf"), CV("pairs", 96000, "nan"), CV("planes", 96008, "nan", 3), CV("planes", 96008, "inf", 2),
    ],
    "split_dual": [
        # transpose_pairs_kernel<false, ROW, SUM>, the four of them, at R 1 ... 197 (Rpad % 64 == 32 at R 1, 31, 32, 65, 197: the last tile's
        # second pair group lies beyond Rpad) - transposed pairs alone at C 1, 31, 33, 65; with row pairs at C 32, 96, 160
        SD(1, 1), SD(31, 31), SD(32, 33), SD(33, 65), SD(63, 1, colsum="fold"), SD(64, 31, colsum="parts"), SD(65, 33, colsum="fold"), SD(197, 65, colsum="parts"),
        SD(1, 32, row=1), SD(31, 96, row=1), SD(32, 160, row=1), SD(33, 32, row=1, colsum="fold"), SD(63, 96, row=1, colsum="parts"),
        SD(64, 160, row=1, colsum="fold"), SD(65, 32, row=1, colsum="parts"), SD(197, 96, row=1, colsum="fold"), SD(197, 160, row=1),
        # Rpad beyond the default: 32 and 64 more (whole tiles of zero rows)
        SD(33, 65, rpad=32), SD(65, 96, row=1, rpad=64, colsum="fold"), SD(197, 33, rpad=64, colsum="parts"), SD(32, 32, row=1, rpad=32),
        # no transposed output.  The streaming kernel either side of its gate: C 128 and 256 against 96 and 160; the same source one float
        # off a 16-byte boundary; TT_SPLIT_ROWS 0; R 1 ... 130 (a wave owns 16 rows of a 64-row block)
        *[SD(R, C, t=0, row=1, colsum=cs) for R, C, cs in ((1, 128, ""), (15, 256, "fold"), (16, 128, "parts"), (17, 256, ""), (63, 128, "fold"),
                                                          (65, 256, "parts"), (130, 128, "fold"), (130, 256, ""))],
        SD(65, 96, t=0, row=1, colsum="fold"), SD(130, 160, t=0, row=1, colsum="parts"), SD(17, 96, t=0, row=1),
        SD(65, 128, t=0, row=1, colsum="fold", off=1), SD(130, 256, t=0, row=1, off=1), SD(65, 128, t=0, row=1, colsum="fold", sr=0),
        SD(130, 256, t=0, row=1, colsum="parts", sr=0),
        # long columns: from 4096 rows on the sums take the long-run rule; 20 000 x 128 on the streaming kernel
        SD(4096, 128, t=0, row=1, colsum="fold"), SD(20000, 128, t=0, row=1, colsum="fold"), SD(4100, 33, colsum="fold"),
        # the split's own max pass: R C = 5, 4095, 4096, 4097 (one and two partials), 255 x 4096 + 1 and 256 x 4096 (256 partials), 4099 x 257
        # (odd, capped at 256 partials); a scalar tail wherever R C % 4 != 0
        SD(5, 1, scale="own"), SD(65, 63, scale="own"), SD(64, 64, row=1, scale="own"), SD(241, 17, scale="own", colsum="fold"),
        SD(1044481, 1, scale="own"), SD(8192, 128, t=0, row=1, scale="own", colsum="parts"), SD(4099, 257, scale="own", colsum="parts"),
        # gradient magnitudes, all zero, one 7e4 (S = 2^-3: no flag, where the unscaled split raises it), one inf (S = 1, flag) - on the tile
        # kernel and on the streaming one, from the own max pass and from a producer's slot
        *[SD(197, 96, row=1, scale="own", mag=m, colsum="parts") for m in (1e-3, 3e-8, 1e-30)],
        *[SD(130, 128, t=0, row=1, scale="slot", mag=m, colsum="parts") for m in (1.0, 1e-3, 3e-8, 1e-30)],
        *[SD(65, 96, row=1, scale=sc, vals=v) for sc in ("own", "slot") for v in ("zero", "big", "inf")], SD(65, 96, row=1, vals="big"),
        SD(130, 128, t=0, row=1, scale="own", vals="big"), SD(130, 128, t=0, row=1, scale="slot", vals="inf"), SD(33, 65, scale="slot", mag=3e-8),
        SD(130, 128, t=0, row=1, scale="slot", vals="zero"),
    ],
    "split_multi": [
        # 1, 2 and 32 entries (one launch), 33 (two), 65 (three); the 641 x 449 entry (88 tiles) takes tile0 across 64 wherever it stands
        SM(1), SM(1, 1), SM(2), SM(2, 6), SM(32), SM(33, 3), SM(65, 5),
    ],
    "transpose_pairs": [
        *[TPP(R, C) for R, C in zip((1, 31, 32, 33, 63, 64, 65, 197), (32, 96, 160, 32, 96, 160, 32, 96))],
        TPP(1, 160, 64), TPP(33, 96, 64), TPP(64, 32, 64), TPP(197, 160, 64), TPP(65, 96, 32),
    ],
    "transpose_planes": [
        # Rpad = R: odd (one bf16 per lane), % 4 == 0 but not % 64, % 64 == 0; the padded forms; with and without the column sums
        *[TPL(R, C, "R", cs) for R, C, cs in ((1, 1, 0), (3, 63, 1), (63, 64, 0), (65, 65, 1), (197, 200, 0), (197, 1, 1), (65, 200, 0))],
        *[TPL(R, C, "R", cs) for R, C, cs in ((4, 63, 1), (68, 65, 0), (196, 200, 1), (64, 64, 0), (64, 200, 1), (192, 65, 0))],
        *[TPL(R, C, "c64", cs) for R, C, cs in ((1, 63, 1), (3, 200, 0), (63, 65, 1), (64, 1, 0), (65, 64, 1), (197, 200, 1))],
        *[TPL(R, C, "c64+64", cs) for R, C, cs in ((1, 64, 0), (63, 200, 1), (64, 65, 0), (197, 63, 1))],
        TPL(4100, 65, "R", 1), TPL(4101, 33, "R", 1),
    ],
    "patch_embed": [
        # gh != gw both ways and a grid of one row / one column, at P 4, 8 and 16, C 1 ... 3, D 64 ... 192, token counts F (n + 1) that are no
        # multiple of 64, every frame map - in all three modes (pairs need C P P % 32 == 0, planes % 64)
        *[PE(m, 3, 3, 16, 2, 5, 64, "rev") for m in ("f32", "pairs", "planes")], *[PE(m, 2, 1, 8, 5, 2, 128, "repeat") for m in ("f32", "pairs", "planes")],
        *[PE(m, 5, 2, 8, 1, 7, 192) for m in ("f32", "pairs", "planes")], *[PE(m, 2, 3, 16, 6, 1, 128, "repeat") for m in ("f32", "pairs", "planes")],
        PE("f32", 3, 3, 4, 3, 5, 64, "rev"), PE("pairs", 3, 2, 4, 5, 3, 64, "repeat"), PE("planes", 2, 4, 4, 3, 4, 64), PE("f32", 2, 1, 4, 2, 3, 192),
        PE("pairs", 4, 1, 16, 3, 2, 192, "rev"), PE("planes", 3, 1, 16, 4, 3, 192, "rev"),
        # the f32 entry's general kernel: P 8 (above), D 72, TT_PATCH_LEAN 0 on a lean shape; its lean kernel at 64 rows per tile (above)
        # and at 128 (16 280 patch rows at D 128: 256 tiles of 128 x 64)
        PE("f32", 2, 3, 16, 2, 3, 72), PE("f32", 3, 3, 16, 2, 5, 64, "rev", lean=0), PE("f32", 407, 1, 16, 5, 8, 128, "repeat"),
        # rows enough for the persistent GEMMs (10 783 rows: K 64 into D 384 on pairs, K 128 into D 768 on planes)
        PE("pairs", 263, 1, 8, 5, 8, 384, "repeat"), PE("planes", 263, 2, 8, 5, 8, 768, "repeat"),
    ],
    "grad_amax": [
        # layernorm_bwd_kernel: D 1 ... 1000; 1, 3, 7, 9 rows (one workgroup, then two of five rows), 8192 (1024 workgroups of 8), 8193 and
        # 8200 (the cap: 9 rows each, trailing workgroups without a row); dropping token 0; accumulating
        GA("ln_bwd", 1, 1), GA("ln_bwd", 3, 63, accum=1), GA("ln_bwd", 7, 64, gscale=1e-7), GA("ln_bwd", 9, 65), GA("ln_bwd", 8192, 96, accum=1),
        GA("ln_bwd", 8193, 64, gscale=1e-7), GA("ln_bwd", 8200, 1000), GA("ln_bwd", 8, 96), GA("ln_bwd", 5, 1024, accum=1), GA("ln_bwd", 8200, 96, N=201),
        GA("ln_bwd", 12, 63, N=5), GA("ln_bwd", 1, 1000, N=2, gscale=1e-7), GA("ln_bwd", 196, 65, N=197),
        # layernorm_bwd_vec_kernel<1|3|6> at 1, 2, 3, 8 and 17 rows - and the same shapes one float off 8-byte alignment (the general kernel)
        *[GA("ln_bwd", r, D, accum=a) for r, D, a in ((1, 128, 0), (2, 384, 1), (3, 768, 0), (8, 128, 1), (17, 384, 0), (17, 768, 1), (8193, 384, 0))],
        GA("ln_bwd", 16, 384, N=17), GA("ln_bwd", 8471, 768, gscale=1e-7), GA("ln_bwd", 1, 384), GA("ln_bwd", 8, 384, gscale=1e-7),
        *[GA("ln_bwd", r, D, accum=a, off=1) for r, D, a in ((2, 384, 1), (3, 768, 0), (17, 128, 0))],
        # l2norm_bwd_kernel: a wave per row, four per workgroup - 1, 3, 4 and 5 rows
        GA("l2_bwd", 1, 1), GA("l2_bwd", 3, 64, gscale=1e-7), GA("l2_bwd", 4, 65), GA("l2_bwd", 5, 1024), GA("l2_bwd", 70, 1024, gscale=1e-7),
        # attention_bwd_dq / dkv_kernel, fp32 and on pairs (max |dout| from the call's own pass and from a slot): N 1 ... 257, H 1 and 3
        *[GAT("attn_bwd", F, N, H, g) for F, N, H, g in ((1, 1, 1, 1.0), (2, 63, 3, 1e-7), (1, 64, 1, 1.0), (2, 65, 1, 1.0), (1, 197, 3, 1.0), (1, 257, 1, 1e-7))],
        *[GAT("attn_bwd_pairs", F, N, H, g, d) for F, N, H, g, d in ((1, 1, 1, 1.0, 1), (2, 63, 3, 1e-7, 0), (1, 64, 1, 1.0, 1), (2, 65, 1, 1e-7, 1),
                                                                    (1, 197, 3, 1.0, 0), (1, 257, 1, 1e-7, 1), (2, 197, 3, 1e-7, 1))],
        # the general pair kernel's epilogue (no gelu'): its four tiles - 128 x 128, 64 x 128, 64 x 64 on four slabs and on three - on a
        # reduction of 64; M 1, 63, 65, 130 on the small grids
        GD(8200, 64, 1536), GD(8200, 64, 1024), GD(8200, 64, 320), GD(1, 64, 64), GD(63, 128, 192, gscale=3e-8), GD(65, 64, 128), GD(130, 192, 320, gscale=3e-8),
        # x gelu': the persistent kernels' regimes (half tiles, round robin, K-split) with a ragged last row tile, and the general kernel
        GD(4000, 64, 1024, 1), GD(6300, 64, 1024, 1, 3e-8), GD(8300, 768, 1024, 1), GD(65, 64, 128, 1), GD(591, 192, 320, 1, 3e-8),
    ],
    "layernorm_long": [
        # the first tier's layernorm check beyond 8192 rows: ln_bwd_wgs' cap of 1024 workgroups (9 rows each, trailing workgroups without a
        # row) on the general kernel (D 64) and on layernorm_bwd_vec_kernel<3>
        LNL(1, 8193, 64), LNL(1, 8193, 384), LNL(43, 197, 64), LNL(43, 197, 384), LNL(43, 197, 384, 1),
    ],
}


def draw(op: str, rng) -> dict:
    return DRAW[op](rng)


def table(seed: int = SUITE_SEED, counts: dict = COUNTS) -> list:
    """[(op, params)]: every pinned case, then ``counts[op]`` draws per op from one generator seeded with ``seed`` (op by op, in OPS order)."""
    rng = np.random.default_rng(seed)
    out = []
    for op in OPS:
        out += [(op, dict(c)) for c in PINNED[op]]
        out += [(op, draw(op, rng)) for _ in range(counts[op])]
    return out


def case_id(op: str, params: dict) -> str:
    return op + "[" + ",".join(f"{k}={v}" for k, v in params.items()) + "]"
