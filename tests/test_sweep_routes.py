"""The sweep's case table (tests/_sweep_cases.py) reaches every route of the kernels it checks - without a GPU.

The route queries are host logic: tt_linear_fwd_route, tt_linear_fwd_pairs_route, tt_linear_fwd_planes_route, tt_linear_bwd_weight_pairs_tn_ok
(hip_ops.linear_bwd_data_pairs_is_persistent, hip_ops.attention_pairs_ok).  With no device they assume 256 CUs, the MI355X's count.  Where a
launcher branches without a host query - the persistent pair GEMM's tile regimes, Sinkhorn's columns per lane and workgroup counts - its rule
is restated here with the line it comes from."""
import itertools

import pytest

from _sweep_cases import (AMAX_PARTS_CAP, CONVERT_CAP, LN_BWD_WG_CAP, MULTI_MAXN, PREP_OPS, VALUE_KINDS, amax_n_part, ceil_to, ln_bwd_plan, multi_entries,
                          pairs_general_tile, patch_f32_route, prep_case_on_twin, sd_kernel, sd_rpad, tp_rpad, tp_store_branch)
from _sweep_cases import (ADJOINT_LONG_RUN, BF_MAX_R, DTYPES, DV_OC, EVAL_OPS, GRAY_SUM_CAP, HEAD_OPS, IMG_MODES, KM_ASSIGN_STRIDE, KM_MAX_GRID_Y, KM_MAXKD,
                          LP_CAND_CAP, METRIC_OPS, OPS, PAIR_EPILOGUES, PROP_OPS, STEP_OPS, WGRAD_LONG_RUN, adjoint_run, bf_radius, bf_tiling, case_id,
                          cs_blocks, cs_route, davis_tiling, gather_tp_log2, kf_fit_group, kf_fit_kernel, kf_fit_lds, kf_fit_ok, km_accumulate_blocks,
                          km_max_k, km_tile, km_tile_default, lp_caps, lp_chunk, lp_cmax, probe_logits_kernel, sgd_lengths, table, tiles_of, wgrad_split)
from timetuning_amd import _lib, hip_ops

NCU = 256
CASES = table()


def _of(op):
    return [p for o, p in CASES if o == op]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_linear_f32_every_tile_on_both_kernels(lib):
    # every value tt_linear_fwd_route (gemm_f32.hip) returns over a wide grid of shapes: 4 tiles x {general, lean whole-tile kernel}
    grid = {lib.tt_linear_fwd_route(M, N, K) for M, N, K in itertools.product(list(range(1, 200, 13)) + list(range(200, 40000, 397)),
                                                                              (8, 50, 64, 72, 128, 192, 200, 256, 384, 700, 768, 1152, 2304),
                                                                              (1, 16, 20, 384))}
    assert grid == {0, 1, 2, 3, 256, 257, 258, 259}
    assert {lib.tt_linear_fwd_route(p["M"], p["N"], p["K"]) for p in _of("linear_f32")} == grid
    assert {(p["act"], p["res"]) for p in _of("linear_f32")} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def pairs8_regime(M, N, K):
    """gemm_pairs8.hip, pairs8_plan (the symmetric kernel, default knobs: TT_Q8_KSPLIT 1, TT_Q8_MIN_TILES 128, TT_P8_NO_HALF 0): None = the
    general kernel; otherwise how the left-over tiles of the last round are dealt - "ksplit" (Q8Args::ks_S, the K-split estimate),
    "half" (2 * rem <= CUs: half tiles), "round_robin" (whole tiles)."""
    if N % 128 or K % 32 or M < 256:
        return None
    ntiles = ((M + 255) // 256) * (N // 128)
    R, rem = divmod(ntiles, NCU)
    ks = 0
    if rem > 0 and R > 0:
        U = K // 32
        S = min(NCU // rem, U, 6)
        if S >= 2:
            t_tile = 1.3 * (K // 32) + 3.0
            t_slice = 1.3 * ((U + S - 1) // S) + 3.0 + 9.0 + 1.0 * S
            t_else = 0.86 * t_tile if 2 * rem <= NCU else t_tile
            if t_slice < 0.9 * t_else:
                ks = S
    if ntiles < 128 and ks == 0:
        return None
    if ks:
        return "ksplit"
    return "half" if (rem > 0 and 2 * rem <= NCU) else "round_robin"


def _pairs_route(lib, p):
    e = PAIR_EPILOGUES[p["epi"]]
    return lib.tt_linear_fwd_pairs_route(p["M"], p["N"], p["K"], e["act"], 1, e["res"], e["out_f32"], e["out_pairs"], e["save_pre"])


def test_linear_pairs_every_kernel_regime_and_epilogue(lib):
    cases = _of("linear_pairs")
    routes = {_pairs_route(lib, p) for p in cases}
    assert routes == {0, 8}
    # the restatement agrees with the library wherever the epilogue is one the persistent kernel compiles (plain fp32 output)
    for p in cases:
        assert (pairs8_regime(p["M"], p["N"], p["K"]) is not None) == (lib.tt_linear_fwd_pairs_route(p["M"], p["N"], p["K"], 0, 1, 0, 1, 0, 0) == 8), p
    assert {pairs8_regime(p["M"], p["N"], p["K"]) for p in cases if _pairs_route(lib, p) == 8} == {"ksplit", "half", "round_robin"}
    for r in (0, 8):
        assert {p["epi"] for p in cases if _pairs_route(lib, p) == r} >= ({"y", "y_res", "pairs_gelu"} if r == 8 else
                                                                         {"y", "y_res", "y_pairs", "y_pairs_gelu_pre", "pairs_gelu"})
    assert any(p["M"] < 256 for p in cases) and any(p["M"] >= 256 and pairs8_regime(p["M"], p["N"], p["K"]) is None for p in cases)
    assert any(p["N"] % 128 for p in cases) and any(p["K"] % 96 for p in cases)           # 64-wide column tiles; K not whole triples


def test_linear_planes_both_kernels(lib):
    cases = _of("linear_planes")
    got = {(p["P"], lib.tt_linear_fwd_planes_route(p["P"], p["M"], p["N"], p["K"], p["act"], 1, p["res"], 1, 0, 0)) for p in cases}
    assert got == {(1, 0), (1, 8), (3, 0), (3, 8)}


def test_backward_pairs_every_route(lib):
    cases = _of("bwd_pairs")
    seen = set()
    for p in cases:
        M, N, K = p["M"], p["N"], p["K"]
        assert hip_ops.bwd_pairs_ok(M, N, K)
        tn_ok = bool(lib.tt_linear_bwd_weight_pairs_tn_ok(N, K, M))
        seen.add((hip_ops.linear_bwd_data_pairs_is_persistent(M, N, K), bool(p["tn"]) and tn_ok, p["mag"], p["gelu"]))
    for persistent, tn in itertools.product((False, True), (False, True)):
        assert any(s[0] == persistent and s[1] == tn for s in seen), (persistent, tn)
    assert {s[2] for s in seen} == {1e-3, 3e-8} and {s[3] for s in seen} == {0, 1}
    # the transposed-pair weight gradient both because TN_WGRAD is off and because the shape is not the TN kernel's
    assert any(not p["tn"] and lib.tt_linear_bwd_weight_pairs_tn_ok(p["N"], p["K"], p["M"]) for p in cases)
    assert any(p["tn"] and not lib.tt_linear_bwd_weight_pairs_tn_ok(p["N"], p["K"], p["M"]) for p in cases)


def test_attention_resident_and_kv_tiled():
    cases = _of("attention")
    assert all(hip_ops.attention_pairs_ok(p["N"], 64) for p in cases)          # head_dim 64: the only one the attention kernels take
    # attention_pairs.hip: K / V resident in LDS up to 256 tokens, the KV-tiled kernel beyond - or forced (knob TT_ATTN_PAIRS_FLASH)
    kinds = {("kv_tiled" if (p["N"] > 256 or p["flash"]) else "resident", p["N"] > 256) for p in cases}
    assert kinds == {("resident", False), ("kv_tiled", False), ("kv_tiled", True)}
    Ns = {p["N"] for p in cases}
    assert {1, 256, 257} <= Ns and max(Ns) >= 850
    assert any(p["Fr"] * p["H"] > NCU for p in cases)      # more (frame, head) items than CUs: the resident kernel's persistent loop


def test_ce_every_width():
    cases = _of("ce")
    assert {p["K"] for p in cases} >= {1, 63, 64, 65, 200, 256, 257, 511, 512}
    assert {p["weighted"] for p in cases} == {0, 1}


# ---- Sinkhorn: sinkhorn.hip
def sk_default_cap(B):                      # sk_default_cap
    c = (B // 98 + 63) // 64 * 64
    if B >= 4096 and c < 128:
        c = 128
    return max(64, min(256, c))


def sk_wgs(B):                              # sk_wgs: >= 2 rows per wave, at most the cap
    w = (B + 31) // 32
    return max(1, min(w, sk_default_cap(B)))


def sk_kpl(K):                              # SK_LAUNCH_KPL: 4 columns per lane up to K = 256, 8 beyond
    return 4 if K <= 256 else 8


def _empty_wgs(B, G):
    rows = (B + G - 1) // G
    return G - (B + rows - 1) // rows


def test_sinkhorn_every_launch_regime():
    cases = _of("sinkhorn")
    # both KPLs; workgroup counts below, at and beyond the cap; a workgroup that gets no rows
    assert {sk_kpl(p["K"]) for p in cases} == {4, 8}
    w = lambda B: (B + 31) // 32
    assert any(w(p["B"]) < sk_default_cap(p["B"]) for p in cases)
    assert any(w(p["B"]) == sk_default_cap(p["B"]) for p in cases)
    assert any(w(p["B"]) > sk_default_cap(p["B"]) for p in cases)
    assert any(sk_wgs(p["B"]) == 256 for p in cases)
    assert any(_empty_wgs(p["B"], sk_wgs(p["B"])) > 0 for p in cases)
    # windows and iteration counts
    assert {p["iters"] for p in cases} >= {0, 1}
    assert any(p["row0"] > 0 for p in cases) and any(p["row0"] + p["rows_out"] < p["B"] for p in cases)
    assert any(p["rows_out"] > 8192 for p in cases)        # the output launch's own workgroup count (one per 32 rows up to 8192 rows)
    # what else the pinned shapes are in the table for (both KPLs and the iteration counts 0 and 1: above): an odd B * K - the partial
    # region then does not start where E ends - and ONE window that starts past row 0 and ends before B
    assert any(p["B"] * p["K"] % 2 for p in cases)
    assert any(p["row0"] > 0 and p["row0"] + p["rows_out"] < p["B"] for p in cases)


def test_sinkhorn_entries_and_queue():
    fq = _of("sinkhorn_from_q")
    assert {p["transposed"] for p in fq} == {0, 1} and {sk_kpl(p["K"]) for p in fq} == {4, 8}
    loc = _of("sinkhorn_local")
    assert {sk_kpl(p["K"]) for p in loc} == {4, 8} and 0 in {p["iters"] for p in loc}
    assert any(p["B"] % 32 for p in loc) and any(_empty_wgs(p["B"], sk_wgs(p["B"])) > 0 for p in loc)
    qp = _of("queue_push")
    assert any(p["m"] == 1 for p in qp) and any(p["m"] == p["Q"] for p in qp) and any(1 < p["m"] < p["Q"] for p in qp)


def test_rows_ops_edges():
    ln = _of("layernorm")
    assert {(p["drop"], p["pairs"]) for p in ln} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(p["D"] % 32 for p in ln)
    l2 = _of("l2norm")
    assert any(p["zero_row"] for p in l2) and any(not p["zero_row"] for p in l2) and max(p["D"] for p in l2) == 1024


# ---- the Sinkhorn workspace layout: E, padding to a 256-byte boundary, two partial buffers of SK_MAXWG = 256 rows
@pytest.mark.parametrize("B,K", [(777, 333), (6272, 200), (1, 1), (50176, 200), (3, 511), (1001, 255)])
def test_sinkhorn_workspace_is_e_padded_to_256_bytes_and_two_partial_buffers(lib, B, K):
    nb = lib.tt_sinkhorn_workspace_bytes(B, K)
    assert nb == (B * K * 4 + 255) // 256 * 256 + 2 * 256 * K * 4
    assert lib.tt_sinkhorn_local_workspace_bytes(B, K) == nb


# ---- the second tier: the evaluator, optimizer and mask kernels.  Their launchers branch without a host query, so each rule is restated
# here with the place it comes from.
def test_second_tier_is_appended_and_complete():
    assert STEP_OPS == ("linear_f32", "linear_pairs", "linear_planes", "bwd_pairs", "layernorm", "l2norm", "attention", "ce", "sinkhorn",
                        "sinkhorn_from_q", "sinkhorn_local", "queue_push")
    ops_in_order = list(dict.fromkeys(o for o, _ in CASES))
    assert tuple(ops_in_order) == STEP_OPS + EVAL_OPS + PROP_OPS + HEAD_OPS + METRIC_OPS + PREP_OPS == OPS   # appended: the first tier's draws - and case ids - are untouched
    ids = [case_id(o, p) for o, p in CASES]
    assert len(set(ids)) == len(ids)
    # (the first and the last case of the first tier, as they were before the second tier existed)
    first = [i for i, (o, _) in zip(ids, CASES) if o in STEP_OPS]
    assert len(first) == 130 and first[0] == "linear_f32[M=1,N=64,K=20,act=0,res=0]" and first[-4] == "queue_push[Q=1,D=128,m=1]"


def km_assign_kernel(d):                     # kmeans.hip, tt_kmeans_assign: kmeans_assign_kernel<16>, <64>, <0>
    return 16 if d <= 16 else (64 if d <= 64 else 0)


def km_assign_strides(P):                    # tt_kmeans_assign: ceil(P / 256) workgroups, at most 4096 - then the grid-stride loop
    return (P + 255) // 256 > 4096


def test_kmeans_shape_rule_is_one_rule(lib):
    # kmeans.hpp, km_shape_ok: k * d <= KM_MAXKD, and at d <= 64 the tile of 256 points shares the 128 KB of LDS
    for d in list(range(1, 130)) + [255, 256, 257, 384, 1024, 16384, 16385]:
        kmax = km_max_k(d)
        assert (kmax == 0 or lib.tt_kmeans_shape_ok(d, kmax)) and not lib.tt_kmeans_shape_ok(d, kmax + 1), d
    assert km_max_k(64) == 252 and km_max_k(63) == 16384 // 63 and km_max_k(65) == 252 and km_max_k(50) >= 300
    assert not lib.tt_kmeans_shape_ok(0, 1) and not lib.tt_kmeans_shape_ok(1, 0)


def test_kmeans_driver_refuses_before_its_first_assignment():
    import torch

    from timetuning_amd import clustering

    with pytest.raises(_lib.HipLibraryError, match="k = 253 centroids of d = 64"):
        clustering.Kmeans(64, 253)._lloyd(torch.zeros(300, 64))          # (host tensor: the refusal comes before any kernel)


def test_kmeans_assign_every_kernel_and_the_stride_loop(lib):
    cases = _of("kmeans_assign")
    assert all(lib.tt_kmeans_assign_route(d) == km_assign_kernel(d) for d in range(1, 200))
    assert all(p["k"] <= km_max_k(p["d"]) for p in cases)
    assert {(km_assign_kernel(p["d"]), km_assign_strides(p["P"])) for p in cases} == set(itertools.product((16, 64, 0), (False, True)))
    assert {p["d"] for p in cases} >= {1, 16, 17, 64, 65, 128, 384}
    assert {p["P"] for p in cases} >= {1, 255, 256, 257} and any(p["k"] == 1 for p in cases)
    assert any(p["P"] % 256 and not km_assign_strides(p["P"]) for p in cases) and any(p["P"] % 256 and km_assign_strides(p["P"]) for p in cases)
    # the largest k * d on each kernel; the duplicated centroid on each kernel
    for kern in (16, 64, 0):
        assert any(km_assign_kernel(p["d"]) == kern and p["k"] == km_max_k(p["d"]) for p in cases), kern
        assert any(km_assign_kernel(p["d"]) == kern and p["dup"] for p in cases), kern
    assert any(p["k"] * p["d"] == KM_MAXKD for p in cases)


def km_accumulate_grid(P):                   # kmeans.hpp, km_accumulate_blocks: (workgroups, points per workgroup, workgroups with no points)
    b = min(4096, max(1, (P + 127) // 128))
    ppb = (P + b - 1) // b
    return b, ppb, b - (P + ppb - 1) // ppb


def test_kmeans_accumulate_every_regime():
    cases = _of("kmeans_accumulate")
    grids = [km_accumulate_grid(p["P"]) for p in cases]
    assert any(b < 4096 for b, _, _ in grids) and any(b == 4096 and ppb == 128 for b, ppb, _ in grids)       # under and AT the cap
    assert any(ppb > 128 for _, ppb, _ in grids) and any(e > 0 for _, _, e in grids)                      # long fp32 sums; empty workgroups
    assert all(e == 0 for b, _, e in grids if b < 4096)             # (under the cap no workgroup is ever empty)
    assert {p["mode"] for p in cases} == {"rand", "skip", "one"}
    assert any(p["mode"] == "one" and km_accumulate_grid(p["P"])[1] > 128 for p in cases)                    # the longest sums of all
    assert any(p["d"] > 256 for p in cases) and any(p["d"] == 1 for p in cases)                              # a thread owns two columns / one
    assert any(p["k"] * p["d"] == KM_MAXKD for p in cases) and any(p["k"] == KM_MAXKD for p in cases)
    assert all(p["k"] <= km_max_k(p["d"]) for p in cases)


def test_col_moments_under_at_and_over_the_cap():
    cases = _of("col_moments")
    blocks = lambda rows: (rows + 255) // 256                        # cluster.hip, moments_blocks: at most 1024 workgroups
    assert any(blocks(p["rows"]) < 1024 for p in cases) and any(blocks(p["rows"]) == 1024 for p in cases)
    assert any(blocks(p["rows"]) > 1024 for p in cases)
    assert any(p["rows"] == 1 for p in cases) and any(p["cols"] == 1 for p in cases) and any(p["cols"] == 1024 for p in cases)
    assert any(p["cols"] > 256 for p in cases)                        # a thread owns more than one column
    assert {p["kind"] for p in cases} == {"scaled", "const_col", "offset"}
    assert any(p["kind"] == "offset" and blocks(p["rows"]) >= 1024 for p in cases)


def test_upsampling_every_ratio_and_workgroup_size():
    threads = lambda C: 256 if C >= 256 else (128 if C > 64 else 64)   # upsample.hip, tt_upsample_bilinear_tokens
    for op, key in (("upsample_tokens", "C"), ("upsample_argmax_f32", "K"), ("upsample_argmax", "K")):
        cases = _of(op)
        assert any(p["R"] < p["g"] for p in cases) and any(p["R"] == p["g"] for p in cases) and any(p["R"] > p["g"] for p in cases), op
        assert any(p["g"] == 1 for p in cases) and any(p["R"] == 1 for p in cases), op
        assert any(p["R"] > p["g"] and p["R"] % p["g"] for p in cases), op                  # a ragged ratio
        assert {p[key] for p in cases} >= {1, 64, 65, 255, 256, 300}, op
        assert any(p["M"] > NCU for p in cases) and any(p["R"] * p["R"] > 256 for p in cases), op   # gridDim.y; more than one workgroup of pixels
    assert {threads(p["C"]) for p in _of("upsample_tokens")} == {64, 128, 256}
    assert {p["C"] for p in _of("upsample_tokens")} >= {64, 65, 255, 256}                        # either side of both edges


def test_confusion_counts_both_kernels_and_the_cap():
    cases = _of("confusion_counts")
    blocks = lambda n: (n + 4095) // 4096                             # label_prop.hip, tt_confusion_counts: at most 2048 workgroups
    for lds in (True, False):                                         # ... the LDS histogram up to C = 96, global atomics beyond
        sel = [p for p in cases if (p["C"] <= 96) == lds]
        assert any(blocks(p["n"]) < 2048 for p in sel) and any(blocks(p["n"]) > 2048 for p in sel), lds
        assert any(p["stray"] for p in sel)
    assert any(blocks(p["n"]) == 2048 for p in cases)
    assert {p["C"] for p in cases} >= {1, 96, 97, 300} and any(p["n"] == 1 for p in cases)
    assert any(p["stray"] and p["C"] > 255 for p in cases) and any(p["stray"] and p["C"] <= 255 for p in cases)    # 255 a class / ignored


def test_adamw_tables_chunks_and_grids():
    from _sweep_checks_eval import adamw_lengths

    cases = _of("adamw")
    cap = 40                                                           # include/timetuning_hip.h: TT_MAX_TENSORS
    for fused in (0, 1):                                              # hip_ops.adamw_step_ / scale_tensors_ chunk; pipeline.cpp chunks the fused entry
        counts = {min(2, (p["T"] + fused - 1) // cap) for p in cases if p["fused"] == fused}
        assert counts == {0, 1, 2} or counts == {0, 2}, (fused, counts)
    assert {p["T"] for p in cases} >= {1, 40, 41}
    assert {p["step"] for p in cases} >= {1, 100000}
    # rowops.hip, tt_adamw_step: the grid is sized by the LONGEST tensor, at most 1024 workgroups of 256; a length-1 tensor rides along
    grid = lambda p: (max(adamw_lengths(p["T"], p["big"])) + 255) // 256
    assert any(grid(p) > 1024 and 1 in adamw_lengths(p["T"], p["big"]) and adamw_lengths(p["T"], p["big"])[0] == 1 for p in cases)
    assert any(grid(p) == 1024 for p in cases) and any(grid(p) < 1024 for p in cases) and any(grid(p) == 1 for p in cases)
    assert any({1, 255, 257} <= set(adamw_lengths(p["T"], p["big"])) for p in cases)
    assert len({p["gscale"] for p in cases}) >= 3


def test_elementwise_every_tail_and_cap():
    cases = _of("elementwise")
    ns = {p["n"] for p in cases}
    assert {1, 2, 3, 4, 5, 6, 7} <= ns and {n & 3 for n in ns if n > 100000} == {0, 1, 2, 3}
    # rowops.hip: tt_ema_update ceil(n / 4 / 256) workgroups up to 2048; tt_add_inplace ceil(n / 256) up to 4096; tt_count_mismatch up to 2048
    for per_wg, cap in ((1024, 2048), (256, 4096), (256, 2048)):
        wgs = lambda n: (n // 4 + 255) // 256 if per_wg == 1024 else (n + 255) // 256
        assert any(wgs(n) < cap for n in ns) and any(wgs(n) == cap for n in ns) and any(wgs(n) > cap for n in ns), (per_wg, cap)
    assert any(n > 2048 * 1024 and n & 3 for n in ns)                 # the tail behind a strided body
    chunks = lambda M: (M + 255) // 256                               # rowops.hip, colsum_chunks: at most 128
    assert any(chunks(p["rows"]) < 128 for p in cases) and any(chunks(p["rows"]) == 128 for p in cases) and any(chunks(p["rows"]) > 128 for p in cases)
    assert any(p["cols"] % 64 for p in cases) and any(p["cols"] == 1024 for p in cases) and any(p["rows"] % 4 for p in cases)


def test_foreground_mask_and_pos_embed_edges():
    fm = _of("foreground_mask")
    for entry in ("qkv", "probs"):
        sel = [p for p in fm if p["entry"] == entry]
        assert {p["g"] for p in sel} >= {4, 5, 13, 14, 31, 32} and {p["th"] for p in sel} == {0.3, 0.65, 0.8}, entry
        assert {p["H"] for p in sel} >= {1, 3, 6, 12} and any(p["F"] == 1 for p in sel) and any(p["F"] > NCU for p in sel), entry
    assert {p["hd"] for p in fm if p["entry"] == "qkv"} >= {4, 64, 128}
    assert all(p["g"] * p["g"] <= 1024 and 7 // 2 < p["g"] for p in fm)          # attn_mask.hip, launch_foreground_mask
    pe = _of("pos_embed")
    assert {p["g"] for p in pe} == {14, 28} and {p["D"] for p in pe} >= {4, 384, 768}
    assert any(p["gh"] == 1 for p in pe) and any(p["gw"] == 1 for p in pe) and all((p["gh"], p["gw"]) != (p["g"], p["g"]) for p in pe)
    assert any(p["gh"] < p["g"] and p["gw"] < p["g"] for p in pe) and any(p["gh"] > p["g"] and p["gw"] > p["g"] for p in pe)
    assert any((p["gh"] > p["g"]) != (p["gw"] > p["g"]) for p in pe) and any(p["gh"] != p["gw"] for p in pe)


# ---- the third tier: temporal label propagation (label_prop.hip).  tt_label_propagate_route is the function lp_run dispatches on; the
# rule is restated here independently and compared with it, then the table is held to every kernel, slot regime and chunk position.
def test_third_tier_is_appended_and_the_first_two_are_what_they_were():
    import zlib

    assert PROP_OPS == ("label_prop", "label_prop_grid", "upsample_argmax_hw")
    earlier = [case_id(o, p) for o, p in CASES if o in STEP_OPS + EVAL_OPS]
    assert len(earlier) == 290 and zlib.crc32("\n".join(earlier).encode()) == 3949057654      # the ids of the first two tiers, unchanged (but Sinkhorn's: no persist key since the one-launch solve left)
    assert earlier[-1].startswith("pos_embed[") and [o for o, _ in CASES][290] == "label_prop"


def lp_route_rule(fs, g, K, nl, r, t):
    """label_prop.hip, lp_run: 0 refused; 1..4 label_prop_wave_kernel<3,4>, <3,8>, <8,4>, <8,8>; 5 / 6 label_prop_kernel<8>, <16>."""
    if fs < 2 or g < 1 or K < 1 or not 0 <= nl <= 7 or r < 1 or not 1 <= t < fs:
        return 0
    win = min(2 * r + 1, g)
    cand_max = win * win * lp_cmax(fs, nl)                 # of the clip: the workgroup kernels are chosen per call
    if cand_max > LP_CAND_CAP:
        return 0
    if win <= 16 and g * g <= 4096 and K <= 512:           # a 16 x 16 window in 64 lanes x 4 rows; the source patch in 12 bits; lane + 64 * 7
        c = 1 + len(range(max(1, t - nl), t))              # the contexts of THIS frame: frame 0 and the queue
        return {(True, True): 1, (True, False): 2, (False, True): 3, (False, False): 4}[(c <= 3, K <= 256)]
    return 5 if cand_max <= 2048 else 6


def test_label_prop_route_export_is_the_restated_rule(lib):
    seen = set()
    for fs, g, K, nl, r in itertools.product((1, 2, 3, 4, 5, 6, 9, 10), (0, 1, 2, 7, 14, 16, 17, 23, 32, 33, 64, 65), (0, 1, 64, 256, 257, 512, 513),
                                             (-1, 0, 1, 2, 3, 4, 7, 8), (0, 1, 6, 7, 8, 11, 16, 40)):
        for t in range(0, fs + 1):
            got = lib.tt_label_propagate_route(fs, g, K, nl, r, t)
            assert got == lp_route_rule(fs, g, K, nl, r, t), (fs, g, K, nl, r, t, got)
            seen.add(got)
    assert seen == {0, 1, 2, 3, 4, 5, 6}


def _lp_routes(p):
    return [lp_route_rule(p["fs"], p["g"], p["K"], p["nl"], p["r"], t) for t in range(1, p["fs"])]


def _lp_cands(p):
    win = min(2 * p["r"] + 1, p["g"])
    return win * win * lp_cmax(p["fs"], p["nl"])


def test_label_prop_every_kernel_with_and_without_labels(lib):
    cases = _of("label_prop")
    for p in cases:
        assert _lp_routes(p) == [lib.tt_label_propagate_route(p["fs"], p["g"], p["K"], p["nl"], p["r"], t) for t in range(1, p["fs"])], p
    # every value of the route query: the refusal and the six kernels; each kernel on the LAST frame (tt_label_propagate requests the labels
    # there) and on some frame of tt_label_propagate_maps (which requests none) - every case runs both entries
    assert {rt for p in cases for rt in _lp_routes(p)} == {0, 1, 2, 3, 4, 5, 6}
    assert {_lp_routes(p)[-1] for p in cases} == {0, 1, 2, 3, 4, 5, 6}
    assert any(len(set(_lp_routes(p))) > 1 for p in cases)                       # a clip that changes kernel between its own frames
    refused = [p for p in cases if _lp_routes(p)[0] == 0]
    assert refused and all(_lp_cands(p) > LP_CAND_CAP and set(_lp_routes(p)) == {0} for p in refused)
    assert any(_lp_cands(p) == 5120 for p in refused)
    ok = [p for p in cases if p not in refused]
    # either side of each deciding bound: K, contexts, window, grid
    assert {p["K"] for p in ok} >= {1, 64, 65, 256, 257, 512, 513}
    for K in (512, 513):
        assert any(p["K"] == K and min(2 * p["r"] + 1, p["g"]) <= 16 and p["g"] <= 64 for p in ok)     # only K moves the call off the wave kernels
    wave = [p for p in ok if _lp_routes(p)[-1] <= 4]
    assert {1 + min(p["fs"] - 2, p["nl"]) for p in wave} >= {1, 2, 3, 4, 8}
    assert {min(2 * p["r"] + 1, p["g"]) for p in ok} >= {1, 2, 3, 16, 17} and any(p["g"] == 16 and p["r"] > 8 for p in ok)
    assert any(p["g"] == 64 and _lp_routes(p)[-1] <= 4 for p in ok) and any(p["g"] == 65 and _lp_routes(p)[-1] == 5 for p in ok)
    assert any(_lp_cands(p) == 2048 and _lp_routes(p)[-1] <= 4 and p["nl"] == 7 for p in ok)             # every slot of the wave kernel
    # candidate counts at the workgroup kernels' caps: 2048 on <8>, the next reachable count and 4096 on <16>
    reachable = sorted({w * w * c for w in range(1, 65) for c in range(1, 9)})
    nxt = min(v for v in reachable if v > 2048)
    assert nxt == 2116
    assert any(_lp_cands(p) == 2048 and _lp_routes(p)[-1] == 5 for p in ok)
    assert any(_lp_cands(p) == nxt and _lp_routes(p)[-1] == 6 for p in ok) and any(_lp_cands(p) == 4096 and _lp_routes(p)[-1] == 6 for p in ok)
    # the first-maximum rule with exactly equal channels on every kernel's label frame, across lanes (K > 1) and slots (K > 64, K > 256)
    for rt in range(1, 7):
        assert any(p["dup"] and _lp_routes(p)[-1] == rt for p in ok), rt
    assert any(p["dup"] and p["K"] > 256 and _lp_routes(p)[-1] in (2, 4) for p in ok) and any(p["dup"] and p["K"] > 256 and _lp_routes(p)[-1] == 5 for p in ok)
    # degenerate sizes, precisions
    assert {p["g"] for p in ok} >= {1, 2, 3} and any(p["bs"] * p["g"] ** 2 % 4 for p in wave)
    assert {p["topk"] for p in ok} >= {1, 5} and any(p["topk"] > _lp_cands(p) for p in wave) and any(p["topk"] > _lp_cands(p) for p in ok if p not in wave)
    assert any(p["g"] == 1 and lp_cmax(p["fs"], p["nl"]) < p["topk"] for p in ok)
    assert {p["D"] for p in ok} >= {4, 16, 20, 64, 384} and any(p["bs"] > 32 and p["bs"] % 4 for p in ok)
    for prec in ("f32", "f16x3", "bf16"):
        assert {min(_lp_routes(p)[-1], 5) for p in ok if p["prec"] == prec} >= {3, 5}, prec      # wave and workgroup kernels in each precision


def test_label_prop_every_slot_regime_and_chunk_position():
    cases = [p for p in _of("label_prop") if _lp_routes(p)[0] != 0]
    # lp_sims_chunk: slot 0 holds (t, 0); lag d sits in slot t - d while the queue fills (t <= nl + 1) and in 1 + nl - d afterwards
    regime = lambda nl, t: "slot0" if nl == 0 or t == 1 else ("filling" if t <= nl + 1 else "full")
    assert {p["nl"] for p in cases} >= {0, 1, 3, 7} and any(p["fs"] == 2 for p in cases)
    for nl in (1, 3, 7):      # a queue that never fills, one that fills on the last frame, one that is full for several frames
        fss = {p["fs"] for p in cases if p["nl"] == nl}
        assert any(fs < nl + 2 for fs in fss) and nl + 2 in fss and any(fs > nl + 3 for fs in fss), (nl, fss)
    assert any(p["nl"] == 0 and p["fs"] > 2 for p in cases)
    # chunk starts: t0 = 1, 1 + T, ... with T = lp_chunk under the case's cap
    hits = set()
    for p in cases:
        n = p["g"] ** 2
        for cap in lp_caps(p):
            T = lp_chunk(p["bs"], p["fs"], n, p["nl"], cap)
            assert T < p["fs"] - 1 or len(lp_caps(p)) > 1, (p, cap, T)             # a cap that cuts nothing is not a chunk case
            for t0 in range(1 + T, p["fs"], T):
                hits.add((p["nl"], regime(p["nl"], t0), t0 == p["nl"] + 2, T))
    for nl in (1, 3, 7):
        assert any(h[0] == nl and h[1] == "filling" for h in hits) or nl == 1, nl  # (nl 1: the filling regime is t = 2 alone)
        assert any(h[0] == nl and h[2] for h in hits), nl                          # a chunk that starts ON t = nl + 2
        assert any(h[0] == nl and h[1] == "full" and not h[2] for h in hits), nl   # ... and one inside the full regime
    assert any(h[0] == 1 and h[1] == "filling" for h in hits)
    assert any(h[0] == 0 for h in hits) and {h[3] for h in hits} >= {1, 2, 3}
    # the real 256 MB cap: a case that is chunked with no variable set
    real = [p for p in cases if not p["cap"] and lp_chunk(p["bs"], p["fs"], p["g"] ** 2, p["nl"]) < p["fs"] - 1]
    assert any(p["g"] == 64 and lp_cmax(p["fs"], p["nl"]) == 3 for p in real)
    assert sum(p["g"] >= 64 for p in cases) <= 3                                   # (the fp64 reference at n >= 4096 takes seconds)


def test_grid_entry_and_upsampler_edges():
    gr = _of("label_prop_grid")
    assert any(p["gh"] == 1 and p["gw"] > 1 for p in gr) and any(p["gw"] == 1 and p["gh"] > 1 for p in gr) and any(p["gh"] > p["gw"] > 1 for p in gr)
    assert any(1 < p["gh"] < p["gw"] for p in gr) and any(p["r"] == 0 for p in gr) and any(p["r"] > max(p["gh"], p["gw"]) for p in gr)
    assert {p["nl"] for p in gr} >= {0, 7} and {p["prec"] for p in gr} == {"f32", "f16x3", "bf16"}
    total = lambda p: (min(2 * p["r"] + 1, p["gh"]) * min(2 * p["r"] + 1, p["gw"]) if p["r"] else p["gh"] * p["gw"]) * lp_cmax(p["fs"], p["nl"])
    assert any(total(p) < p["topk"] for p in gr) and any(total(p) == p["topk"] for p in gr) and any(total(p) > LP_CAND_CAP for p in gr)
    assert any(p["K"] == 1 for p in gr) and any(p["K"] > 256 for p in gr) and any(p["dup"] and p["K"] > 256 for p in gr)
    hw = _of("upsample_argmax_hw")
    assert any(p["H"] < p["gh"] and p["W"] < p["gw"] for p in hw) and any((p["H"], p["W"]) == (p["gh"], p["gw"]) for p in hw)
    assert any(p["H"] > p["gh"] and p["W"] > p["gw"] for p in hw) and any(p["H"] == 1 for p in hw) and any(p["W"] == 1 for p in hw)
    assert {p["K"] for p in hw} >= {1, 64, 65} and any(p["M"] == 1 for p in hw) and any(p["M"] > 1 for p in hw)
    assert any(p["dup"] for p in hw) and any(p["H"] * p["W"] > 256 * 256 for p in hw)


# ---- the fourth tier: the linear probe (linear_probe.hip) and the clip input pipeline (image_ops.hip).  None of their launchers has a host
# query: each rule is restated in tests/_sweep_cases.py with the function it comes from, and the table is held to every branch here.
def test_fourth_tier_is_appended_and_the_first_three_are_what_they_were():
    import zlib

    assert HEAD_OPS == ("probe_logits", "probe_upsample_ce", "bilinear_adjoint", "probe_wgrad", "sgd", "img_resize", "img_color", "img_blur")
    earlier = [case_id(o, p) for o, p in CASES if o not in HEAD_OPS + METRIC_OPS + PREP_OPS]
    assert len(earlier) == 383 and zlib.crc32("\n".join(earlier).encode()) == 2502457127      # the ids of the first three tiers, unchanged (but Sinkhorn's: no persist key since the one-launch solve left)
    assert earlier[-1].startswith("upsample_argmax_hw[") and [o for o, _ in CASES][383] == "probe_logits"
    # every op of the table has a check on the side it runs on (tools/fuzz_ops.py draws from OPS and runs tests/test_hip_sweep.py::run_case)
    from _sweep_checks_eval import CHECK as EVAL_CHECK
    from _sweep_checks_head import CHECK as HEAD_CHECK
    from _sweep_checks_prop import CHECK as PROP_CHECK

    assert set(HEAD_CHECK) == set(HEAD_OPS) and set(EVAL_CHECK) == set(EVAL_OPS) and set(PROP_CHECK) == set(PROP_OPS)


def test_probe_logits_every_kernel_whole_and_ragged():
    cases = _of("probe_logits")
    assert [probe_logits_kernel(C) for C in (1, 64, 65, 128, 129, 192, 193, 256)] == [(1, 4)] * 2 + [(2, 2)] * 2 + [(4, 2)] * 4
    for ct in (1, 2, 3, 4):      # tt_probe_logits: ct = ceil(C / 64) picks the kernel, 16 * RPT rows per workgroup; <4,2> also serves ct = 3
        sel = [p for p in cases if (p["C"] + 63) // 64 == ct]
        rpb = 16 * probe_logits_kernel(64 * ct)[1]
        assert rpb == (64 if ct == 1 else 32)
        rows = {p["rows"] for p in sel}
        assert {rpb - 1, rpb, rpb + 1} <= rows and any(r > 8 * rpb and r % rpb for r in rows), ct      # the last workgroup short, whole, one row
        assert {p["bias"] for p in sel} == {0, 1} and any(p["D"] % 32 for p in sel) and any(p["D"] % 32 == 0 for p in sel), ct
    assert {p["rows"] for p in cases} >= {1, 31, 32, 33, 63, 64, 65, 1001}
    assert {p["C"] for p in cases} >= {1, 63, 64, 65, 128, 129, 192, 193, 256} and {p["D"] for p in cases} >= {4, 32, 36, 384, 1024}


def _gather_geometry(cases, op):
    gr = {(p["g"], p["R"]) for p in cases}
    assert gr >= {(28, 14), (28, 9), (64, 1), (5, 4), (14, 14), (28, 29), (1, 1), (1, 7), (64, 1024)}, op
    # lanes per pixel 1 .. 32, either side of each edge; pixel chunks P = 256 >> tp_log2: R below P, above it and no multiple of it
    assert [gather_tp_log2(C) for C in (1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256)] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]
    assert {p["C"] for p in cases if (p["g"], p["R"]) == (7, 20)} >= {1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256}, op
    for l in range(6):
        P = 256 >> l
        assert any(gather_tp_log2(p["C"]) == l and p["R"] > P and p["R"] % P for p in cases), (op, l)
    assert any(p["B"] == 3 for p in cases) and any(p["g"] * p["C"] == 64 * 256 for p in cases), op      # gridDim.y; the LDS accumulators' maximum


def test_probe_upsample_ce_every_geometry_lane_count_and_label_kind():
    cases = _of("probe_upsample_ce")
    _gather_geometry(cases, "probe_upsample_ce")
    assert any((p["g"], p["R"], p["C"], p["B"]) == (64, 1024, 256, 1) and p["ignored"] == 0.99 for p in cases)      # gather_lds_bytes at its maximum
    assert any((p["g"], p["R"], p["C"]) == (64, 1024, 2) for p in cases)
    assert {p["kind"] for p in cases} == {"normal", "large", "const"} and {p["ignored"] for p in cases} >= {0.0, 0.3, 1.0, "rows"}
    for kind in ("large", "const"):
        assert len({gather_tp_log2(p["C"]) for p in cases if p["kind"] == kind and p["C"] > 1}) >= 4, kind
    assert any(p["C"] == 1 and p["kind"] == k for p in cases for k in ("normal",)) and any(p["C"] == 1 and p["kind"] == "const" for p in cases)
    assert any(p["C"] == 256 and p["ignored"] == 0.3 for p in cases)      # 255 among the labels of a 256-class head: ignored, and counted labels
    assert any(p["ignored"] == "rows" and p["R"] >= 4 * p["g"] for p in cases)      # low-res rows whose every mask row is ignored


def test_bilinear_adjoint_every_geometry_and_lane_count():
    cases = _of("bilinear_adjoint")
    _gather_geometry(cases, "bilinear_adjoint")
    assert all(p["B"] * p["R"] ** 2 * p["C"] <= 1 << 22 for p in cases)      # d_hi stays small: the big masks at small C only
    assert any(adjoint_run(p["g"], p["R"]) >= ADJOINT_LONG_RUN for p in cases) and sum(adjoint_run(p["g"], p["R"]) >= ADJOINT_LONG_RUN for p in cases) <= 3


def test_probe_wgrad_every_split_regime():
    cases = _of("probe_wgrad")
    # linear_probe.hip, wgrad_split (restated in tests/_sweep_cases.py): ns = min(ceil(1024 / tiles), ceil(rows / 32)), at least 1;
    # rows per split = ceil(rows / ns) rounded up to 32; splits = ceil(rows / rows per split)
    assert wgrad_split(47040, 384, 21) == (164, 288, "tiles") and wgrad_split(33, 4, 256) == (2, 32, "chunks") and wgrad_split(32, 60, 63) == (1, 32, "one")
    assert wgrad_split(600, 1024, 256) == (10, 64, "tiles") and wgrad_split(8192, 1024, 256) == (16, 512, "tiles")
    seen = {}
    for p in cases:
        ns, rps, why = wgrad_split(p["rows"], p["D"], p["C"])
        assert ns >= 1 and (ns - 1) * rps < p["rows"] <= ns * rps and rps % 32 == 0, p      # every split has rows; none is left over
        seen.setdefault(why, []).append((p, ns, rps))
    assert set(seen) == {"one", "chunks", "tiles"}
    assert all(ns == 1 for _, ns, _ in seen["one"]) and any(p["rows"] == 32 for p, _, _ in seen["one"]) and any(p["rows"] == 1 for p, _, _ in seen["one"])
    for why in ("chunks", "tiles"):      # a short last split and a whole one... in each capped regime a last split shorter than the others
        assert any(p["rows"] % rps for p, _, rps in seen[why]), why
    assert any(p["rows"] % rps == 0 and ns > 1 for p, ns, rps in seen["tiles"])
    assert any(p["rows"] == 33 for p, _, _ in seen["chunks"]) and any((p["rows"], p["D"], p["C"]) == (47040, 384, 21) for p, _, _ in seen["tiles"])
    tiles = lambda p: ((p["D"] + 63) // 64) * ((p["C"] + 63) // 64)
    assert any(tiles(p) == 64 for p, _, _ in seen["tiles"]) and any(tiles(p) == 1 for p in cases)
    assert any(rps >= WGRAD_LONG_RUN for _, _, rps in seen["tiles"]) and sum(wgrad_split(p["rows"], p["D"], p["C"])[1] >= WGRAD_LONG_RUN for p in cases) <= 2
    assert {p["C"] for p in cases} >= {1, 63, 65, 256} and {p["D"] for p in cases} >= {4, 60, 68, 1024}
    assert {(bool(p["scale"]), p["need_bias"]) for p in cases} == {(False, 0), (False, 1), (True, 0), (True, 1)}


def test_sgd_tables_chunks_and_grids():
    cases = _of("sgd")
    assert {p["T"] for p in cases} >= {1, 40, 41, 85} and {min(2, (p["T"] - 1) // 40) for p in cases} == {0, 1, 2}      # hip_ops.sgd_step_: chunks of 40
    assert {(bool(p["momentum"]), bool(p["wd"])) for p in cases} == {(False, False), (False, True), (True, False), (True, True)}
    assert any(p["steps"] == 3 for p in cases) and all(p["steps"] >= 1 for p in cases)
    # linear_probe.hip, tt_sgd_step: the grid is sized by the LONGEST tensor, at most 1024 workgroups of 256; a length-1 tensor rides along
    grid = lambda p: (max(sgd_lengths(p["T"], p["big"])) + 255) // 256
    assert any(grid(p) > 1024 and sgd_lengths(p["T"], p["big"])[0] == 1 for p in cases) and any(grid(p) == 1024 for p in cases)
    assert any(grid(p) < 1024 for p in cases) and any(grid(p) == 1 for p in cases)
    assert {p["big"] for p in cases} >= {262145, 300001} and any({1, 255, 257} <= set(sgd_lengths(p["T"], p["big"])) for p in cases)


def test_clip_pipeline_edges():
    rs = _of("img_resize")
    dims = lambda p: tuple(int(v) for v in p["crop"].split("/")) if p["crop"] else (0, 0, p["h"], p["w"])
    shapes = {(dims(p)[2], dims(p)[3], p["oh"], p["ow"]) for p in rs}
    assert shapes >= {(1, 1, 5, 3), (7, 1, 3, 4), (1, 9, 4, 2), (1000, 3, 1, 3), (3, 1000, 3, 1)}
    # timetuning_amd.video_transformations.resized_crop: the horizontal pass is skipped at OW = w, the vertical one at OH = h on uint8 output
    for tt in (0, 1):
        sel = [p for p in rs if p["to_tensor"] == tt]
        assert any(dims(p)[3] == p["ow"] and dims(p)[2] != p["oh"] for p in sel) and any(dims(p)[2] == p["oh"] and dims(p)[3] != p["ow"] for p in sel), tt
        assert any(dims(p)[2:] == (p["oh"], p["ow"]) for p in sel) and any(p["crop"] for p in sel) and any(p["F"] == 300 for p in sel), tt
    crops = [p for p in rs if p["crop"]]
    assert any(dims(p)[0] + dims(p)[2] == p["h"] and dims(p)[1] + dims(p)[3] == p["w"] and dims(p)[0] and dims(p)[1] for p in crops)
    assert any(dims(p)[2:] == (1, 1) and dims(p)[:2] == (p["h"] - 1, p["w"] - 1) for p in crops) and any(dims(p) == (0, 0, 1, 1) for p in crops)
    assert any(p["crop"] and dims(p)[3] == p["ow"] and (dims(p)[1] or dims(p)[3] != p["w"]) for p in crops)      # the column slice instead of a pass
    assert {p["ow"] % 2 for p in rs if p["flip"]} == {0, 1} and all(p["to_tensor"] for p in rs if p["flip"])
    col = _of("img_color")
    assert {p["mode"] for p in col if p["H"] * p["W"] == 1} == set(IMG_MODES)
    # image_ops.hip, tt_img_color: gray_sum_kernel on min(256, ceil(npix / 2048)) workgroups - the grid-stride loop runs above 524 288 pixels
    con = [p for p in col if p["mode"] == "contrast"]
    assert GRAY_SUM_CAP == 524288 and any(p["H"] * p["W"] == GRAY_SUM_CAP for p in con) and any(p["H"] * p["W"] > GRAY_SUM_CAP for p in con)
    assert any(p["H"] * p["W"] == 600 * 1024 for p in con) and any(p["F"] == 5 for p in con) and any(p["F"] > 256 for p in con)
    for mode in ("brightness", "contrast", "saturation"):
        assert {p["factor"] for p in col if p["mode"] == mode} >= ({0.0, 0.9999, 1.0, 1.8} if mode != "brightness" else {0.0, 0.9999, 1.8}), mode
    assert {p["factor"] for p in col if p["mode"] == "hue"} >= {-0.5, 0.5} and any(p["mode"] == "hue" and p["F"] >= 2 for p in col)      # (a gray frame)
    bl = _of("img_blur")
    from timetuning_amd.video_transformations import gaussian_box_params

    assert gaussian_box_params(2.0)[0] == 1 and gaussian_box_params(0.1)[0] == 0      # box radius 1: the far taps sit at +-2
    for side in ("H", "W"):
        assert {p[side] for p in bl if p["radius"] == 2.0} >= {1, 2, 3}, side
    assert {(p["H"], p["W"]) for p in bl} >= {(1, 53), (37, 1)} and {p["radius"] for p in bl} >= {0.1, 2.0} and any(p["F"] > 256 for p in bl)


# ---- the fifth tier: the k-means family beyond the resident pair (kmeans.hip, kmeans_fit.hip) and the metric counters (confusion.hip,
# davis.hip, bfscore.hip).  tt_kmeans_fit_shape_ok / tt_kmeans_fit_lds_bytes / tt_kmeans_tile_centroids / tt_confusion_segments_route are host
# queries and are compared with the restated rules; the tilings of the two counters have none, so their rules stand in
# tests/_sweep_cases.py with the function they come from.
def test_fifth_tier_is_appended_and_the_first_four_are_what_they_were():
    import zlib

    assert METRIC_OPS == ("kmeans_assign_tiled", "kmeans_accumulate_tiled", "kmeans_assign_batched", "kmeans_fit", "confusion_segments", "davis_counts",
                          "bf_counts")
    earlier = [case_id(o, p) for o, p in CASES if o not in METRIC_OPS + PREP_OPS]
    assert len(earlier) == 558 and zlib.crc32("\n".join(earlier).encode()) == 4217683      # the ids of the first four tiers, unchanged (but Sinkhorn's: no persist key since the one-launch solve left)
    assert earlier[-1].startswith("img_blur[") and [o for o, _ in CASES][558] == "kmeans_assign_tiled"
    from _sweep_checks_metric import CHECK as METRIC_CHECK      # (tools/fuzz_ops.py draws from OPS and runs tests/test_hip_sweep.py::run_case)

    assert set(METRIC_CHECK) == set(METRIC_OPS)


def test_fit_rules_are_the_librarys(lib):
    for n, d, k in itertools.product((1, 2, 100, 700, 1300, 5000, 600000, 1 << 20, (1 << 20) + 1), (0, 1, 2, 14, 16, 17, 50, 64, 65),
                                     (0, 1, 2, 60, 80, 127, 128, 163, 164, 300, 2000)):
        assert bool(lib.tt_kmeans_fit_shape_ok(n, d, k)) == kf_fit_ok(n, d, k), (n, d, k)
        assert lib.tt_kmeans_fit_lds_bytes(n, d, k) == (kf_fit_lds(d, k, kf_fit_group(n, d, k)) if kf_fit_ok(n, d, k) else 0), (n, d, k)
    # the LDS maxima (16 k d + 4 k <= 128 KB): k = 127 at d = 64, 163 at d = 50
    assert kf_fit_ok(700, 64, 127) and not kf_fit_ok(700, 64, 128) and kf_fit_ok(900, 50, 163) and not kf_fit_ok(900, 50, 164)
    assert kf_fit_lds(64, 127, 1) == 130556 and kf_fit_lds(50, 163, 1) == 131052
    # kf_fit_group = 1 from 12 k d + 4 k >= 72 KB on (and just below, where not even one block's fp32 sums fit beside the fixed part)
    assert kf_fit_group(700, 64, 127) == 1 and kf_fit_group(1500, 14, 300) == 1 and kf_fit_group(1000, 50, 60) == 3 and kf_fit_group(257, 50, 10) == 3


def test_fit_every_instantiation_group_regime_and_block_length():
    cases = _of("kmeans_fit")
    assert all(kf_fit_ok(p["n"], p["d"], p["k"]) and 1 <= p["niter"] <= 5 and 1 <= p["nredo"] <= 2 for p in cases)
    # kmeans_fit.hip, tt_kmeans_fit_batched: DREG by km_assign_route, VEC by d % 4 / d % 2 - and 1 whenever x is off a 16-byte boundary
    assert {kf_fit_kernel(p["d"], p["offset"]) for p in cases} == set(itertools.product((16, 64), (1, 2, 4)))
    assert {p["d"] for p in cases if kf_fit_kernel(p["d"], p["offset"]) == (16, 2)} >= {2, 6, 10, 14}
    for dreg, d in ((16, 12), (64, 64)):      # the unaligned fallback at d % 4 == 0 on both register sizes, beside the aligned run of the same case
        off = [p for p in cases if p["offset"] % 4 and p["d"] == d]
        assert off and all(kf_fit_kernel(d, p["offset"]) == (dreg, 1) for p in off) and any(dict(p, offset=0) in cases for p in off), d
    assert any(p["offset"] == 0 and kf_fit_kernel(p["d"], 0)[1] == 1 for p in cases)      # VEC 1 because d is odd
    # kf_fit_group against the blocks of km_accumulate_blocks
    gb = [(kf_fit_group(p["n"], p["d"], p["k"]), *km_accumulate_blocks(p["n"]), p) for p in cases]
    assert any(g == 1 and b == 6 and (p["d"], p["k"]) == (64, 127) for g, b, _, p in gb) and any(g == 1 and b == 11 and (p["d"], p["k"]) == (50, 80) for g, b, _, p in gb)
    assert any(1 < g < b and b % g for g, b, _, p in gb) and any(1 < g < b and b % g == 0 for g, b, _, p in gb)      # a ragged last pass; whole passes
    assert any(g == b > 1 for g, b, _, p in gb) and any(g == b == 1 for g, b, _, p in gb)
    assert any(g == 1 and b > 1 and p["d"] <= 16 for g, b, _, p in gb)                      # group 1 on the 16-register kernel (d 14, k 300)
    # both LDS maxima are FITTED, not only queried
    assert any((p["d"], p["k"]) == (64, 127) for p in cases) and any((p["d"], p["k"]) == (50, 163) for p in cases)
    # points per block: up to 128 with several blocks, and beyond (n > 524 288: 147 and 256, the longest fp32 runs of the fit)
    assert any(ppb <= 128 and b > 1 for _, b, ppb, _ in gb) and {ppb for _, _, ppb, _ in gb if ppb > 128} == {147, 256}
    assert any(p["n"] == 1 << 20 for p in cases)                                             # KF_MAXN itself
    # threads without a point; every point a cluster; one point; more problems than one launch; the flagged problem
    assert any(p["n"] < 512 for p in cases) and any(p["n"] == p["k"] > 1 for p in cases) and any(p["n"] == 1 for p in cases)
    assert any(p["B"] > KM_MAX_GRID_Y for p in cases) and sum(p["empty"] for p in cases) == 1 and all(p["B"] >= 3 for p in cases if p["empty"])
    assert all(p["B"] * p["n"] * p["d"] * 4 <= 300 << 20 for p in cases)


def test_tiled_assignment_every_kernel_tile_count_and_stride(lib):
    cases = _of("kmeans_assign_tiled")
    assert all(lib.tt_kmeans_tile_centroids(d) == km_tile_default(d) for d in list(range(1, 200)) + [1023, 1024, 1025, 0])
    assert all(0 <= p["tile_k"] <= km_tile_default(p["d"]) and p["P"] * p["d"] * 4 <= 300 << 20 for p in cases)
    several = lambda p: km_tile(p["d"], p["tile_k"]) < p["k"]
    # kmeans_assign_tiled_kernel<16>, <64>, <0> x {one tile, several} x {at most 4096 x 256 points, the grid-stride loop}: <64> stages the
    # point tile again on every stride, <0> keeps ONE tile resident over the strides and reloads several
    seen = {(km_assign_kernel(p["d"]), several(p), p["P"] > KM_ASSIGN_STRIDE) for p in cases}
    assert seen == set(itertools.product((16, 64, 0), (False, True), (False, True)))         # ((0, False, True): `resident` kept past the first stride)
    # the last tile's size: 1, 2, 3 and 5 behind whole tiles (the 4-wide block and its tail); tile_k 1; the last workgroup's points
    last = {p["k"] - (p["k"] - 1) // km_tile(p["d"], p["tile_k"]) * km_tile(p["d"], p["tile_k"]) for p in cases if several(p)}
    assert last >= {1, 2, 3, 5} and any(p["tile_k"] == 1 and p["k"] > 1 for p in cases)
    assert {p["P"] for p in cases} >= {1, 255, 256, 257}
    # a duplicate either side of the first tile boundary on each kernel; k one above the default tile at d 16, 64, 128
    for kern in (16, 64, 0):
        assert any(p["dup"] == 2 and several(p) and km_assign_kernel(p["d"]) == kern for p in cases), kern
    assert all(several(p) for p in cases if p["dup"] == 2)
    for d in (16, 64, 128):
        assert any(p["d"] == d and p["tile_k"] == 0 and p["k"] == km_tile_default(d) + 1 and not lib.tt_kmeans_shape_ok(d, p["k"]) for p in cases), d
    assert any(p["d"] == 1024 for p in cases)


def test_tiled_accumulation_every_regime():
    cases = _of("kmeans_accumulate_tiled")
    tiles = lambda p: (p["k"] + km_tile(p["d"], p["tile_k"]) - 1) // km_tile(p["d"], p["tile_k"])
    assert all(0 <= p["tile_k"] <= km_tile_default(p["d"]) for p in cases)
    assert any(tiles(p) > KM_MAX_GRID_Y for p in cases) and any(tiles(p) == 1 for p in cases) and any(1 < tiles(p) <= KM_MAX_GRID_Y for p in cases)
    assert {p["mode"] for p in cases} == {"rand", "skip", "one"}
    grids = [km_accumulate_grid(p["P"]) for p in cases]
    assert {p["P"] for p in cases} >= {524288, 524289, 600000} and any(ppb > 128 for _, ppb, _ in grids) and any(e > 0 for _, _, e in grids)
    assert all(km_accumulate_blocks(p["P"]) == km_accumulate_grid(p["P"])[:2] for p in cases)
    assert any(p["mode"] == "one" and km_accumulate_grid(p["P"])[1] > 128 for p in cases)
    assert any(p["d"] == 257 and tiles(p) > 1 for p in cases)                                # a thread owns two columns, k above the tile
    assert any(tiles(p) > 1 and p["k"] % km_tile(p["d"], p["tile_k"]) == 1 for p in cases)   # a last tile of one cluster
    assert any(p["tile_k"] == 0 and p["k"] > km_max_k(p["d"]) for p in cases) and any(p["tile_k"] > p["k"] for p in cases)


def test_batched_assignment_every_kernel_and_the_problem_loop():
    cases = _of("kmeans_assign_batched")
    assert all(p["k"] <= km_max_k(p["d"]) for p in cases)
    for kern in (16, 64, 0):
        assert any(km_assign_kernel(p["d"]) == kern and p["B"] == 3 and p["N"] % 256 for p in cases), kern
        assert any(km_assign_kernel(p["d"]) == kern and p["k"] == km_max_k(p["d"]) and p["B"] > 1 for p in cases), kern
    assert any(p["B"] > KM_MAX_GRID_Y for p in cases) and any(p["N"] == 1 for p in cases)      # launch_assign's y0 loop


def test_confusion_segments_every_route_regime_and_misalignment(lib):
    cases = _of("confusion_segments")
    for Cg, Cp in itertools.product((0, 1, 3, 127, 128, 129, 4096, 4097), repeat=2):
        assert lib.tt_confusion_segments_route(Cg, Cp) == cs_route(Cg, Cp)
    assert all(cs_route(p["Cg"], p["Cp"]) for p in cases)
    # cs_blocks: elements per workgroup set by CS_MIN_PER_WG, by four per LDS cell, by the cap of 1024 workgroups.  The global route has no
    # cells to zero or flush, so only two of the three regimes exist there
    regimes = lambda route: {cs_blocks(p["n"], p["Cg"], p["Cp"])[1] for p in cases if cs_route(p["Cg"], p["Cp"]) == route}
    assert regimes(1) == {"min", "cells", "spread"} and regimes(2) == {"min", "spread"}
    assert cs_blocks(8192, 5, 10) == (1, "min") and cs_blocks(8193, 5, 10) == (2, "min")
    assert cs_blocks(42000, 21, 500) == (1, "cells") and cs_blocks(42001, 21, 500) == (2, "cells")
    assert cs_blocks(9000000, 3, 7) == (1024, "spread") and cs_blocks(1024 * 8192, 3, 7) == (1024, "min")
    have = {(p["n"], p["Cg"], p["Cp"]) for p in cases}
    assert have >= {(8192, 5, 10), (8193, 5, 10), (42000, 21, 500), (42001, 21, 500), (9000000, 3, 7)}
    # pred off a 16-byte boundary with MORE THAN ONE workgroup per segment: heads of 1 ... 7 elements (int16) and 1 (int64), on both routes
    for route in (1, 2):
        multi = [p for p in cases if cs_route(p["Cg"], p["Cp"]) == route and cs_blocks(p["n"], p["Cg"], p["Cp"])[0] > 1 and p["S"] > 1]
        assert {p["offset"] for p in multi if p["dtype"] == "i16"} >= set(range(1, 8)), route
        assert any(p["offset"] == 1 and p["dtype"] == "i64" for p in multi), route
        assert any(p["n"] % 8 for p in multi)                                                 # a tail behind the last strip
    head = lambda p: (8 - p["offset"]) % 8 if p["dtype"] == "i16" else p["offset"] % 2
    assert any(p["n"] < 8 for p in cases) and any(head(p) > p["n"] for p in cases) and any(p["n"] % 2 and p["S"] > 1 and p["dtype"] == "i16" for p in cases)
    assert {p["ignore"] for p in cases} >= {"", 0, 255} and {p["dtype"] for p in cases} == {"i16", "i64"}
    assert all(p["S"] * p["n"] * 10 <= 300 << 20 for p in cases)


def _davis_rows(radius):
    from timetuning_amd import mask_propagation as MP

    return MP.disk(radius).shape[0]


def davis_class(H, W, rows, oc):
    """How far davis_tiling shrank: (halvings of TH, whether ow stayed / shrank / shrank to one word)."""
    words = (W + 63) // 64
    ow0 = (words + (words + 7) // 8 - 1) // ((words + 7) // 8)
    TH, ow = davis_tiling(H, W, rows, oc)
    th0, halvings = min(H, 32), 0
    while th0 > TH:
        th0, halvings = th0 // 2, halvings + 1
    assert th0 == TH
    return halvings, ("full" if ow == ow0 else ("one" if ow == 1 else "shrunk"))


def test_davis_every_tiling_class_and_block_decomposition():
    cases = _of("davis_counts")
    # every class davis_tiling returns over a wide grid of (H, W, element rows, objects per pass) - and nothing is ever refused
    grid = {davis_class(H, W, rows, oc) for H, W, rows, oc in itertools.product((1, 6, 8, 9, 16, 20, 31, 32, 40, 70, 480), (1, 64, 65, 200, 300, 512, 513, 600, 854, 1100, 4000),
                                                                                (1, 3, 6, 17, 41, 81, 127), (1, 2, 3, 4))}
    mine = {davis_class(p["H"], p["W"], _davis_rows(p["radius"]), min(p["O"], DV_OC)) for p in cases}
    assert mine == grid, (sorted(grid - mine), sorted(mine - grid))
    tiling = lambda p: davis_tiling(p["H"], p["W"], _davis_rows(p["radius"]), min(p["O"], DV_OC))
    assert davis_tiling(70, 300, 127, 4) == (8, 1) and tiles_of(70, 300, 8, 1) == (9, 5)
    assert davis_tiling(40, 600, 81, 4) == (8, 3) and davis_tiling(40, 512, 17, 4)[1] == 8 and davis_tiling(40, 513, 17, 4)[1] == 5
    have = {(p["T"], p["H"], p["W"], p["O"], p["radius"]) for p in cases}
    assert have >= {(2, 70, 300, 4, 63), (2, 40, 513, 4, 8), (2, 40, 512, 4, 8), (2, 40, 600, 5, 40), (2, 6, 200, 4, 63), (3, 70, 1100, 3, 2)}
    # block index -> (frame, tile row, tile column) with all three above 1
    assert any(p["T"] > 1 and min(tiles_of(p["H"], p["W"], *tiling(p))) > 1 for p in cases)
    assert any(p["T"] > 2 and min(tiles_of(p["H"], p["W"], *tiling(p))) > 2 for p in cases)
    assert any(p["O"] > DV_OC and p["O"] % DV_OC == 1 for p in cases) and any(p["H"] < 8 and p["W"] > 64 for p in cases)
    assert {(p["pt"], p["gtt"], p["void"]) for p in cases} == set(itertools.product(DTYPES, DTYPES, (0, 1)))
    assert any(_davis_rows(p["radius"]) % 2 == 0 for p in cases) and any(_davis_rows(p["radius"]) == 127 for p in cases)


def test_bf_tiling_never_shrinks_and_block_decomposition():
    # bfscore.hip, bf_tiling: over the entry's whole domain (R <= 63, up to 8 words per tile, TH <= 32) the planes need at most 63 168 bytes
    # of the 64 KB budget: its shrink loop never runs.  A change of the budget or of the LDS layout that makes it live shows here
    worst = 0
    for H, W, R in itertools.product((1, 2, 8, 31, 32, 33, 100, 480), list(range(1, 1100, 61)) + [512, 513, 1024, 1025, 4096, 100000], range(0, BF_MAX_R + 1)):
        TH, ow, shrunk = bf_tiling(H, W, R)
        assert not shrunk and TH == min(H, 32) and ow <= 8, (H, W, R)
        worst = max(worst, 8 * (2 * (TH + 2 * R + 2) * (ow + 2) + 2 * (TH + 2 * R) * (ow + 2) + 6 * TH * ow))
    assert worst == 63168
    assert bf_radius(64) == 63 and bf_radius(63.9) == 63 and bf_radius(2) == 1 and bf_radius(0) == 0 and bf_radius(31) == 30
    cases = _of("bf_counts")
    tiling = lambda p: bf_tiling(p["H"], p["W"], bf_radius(p["t"]))[:2]
    assert any(p["P"] > 2 and min(tiles_of(p["H"], p["W"], *tiling(p))) > 2 for p in cases)      # pair, tile row, tile column all above 1
    for W, ow in ((512, 8), (513, 5)):      # one tile column of 8 words / two of 5, at the largest element
        assert any(p["W"] == W and bf_radius(p["t"]) == BF_MAX_R and tiling(p)[1] == ow and p["P"] > 1 for p in cases), W
    have = {(p["P"], p["H"], p["W"], p["t"]) for p in cases}
    assert have >= {(3, 70, 1100, 2), (2, 40, 513, 64), (2, 40, 512, 64), (2, 40, 600, 31)}
    assert any(p["H"] < 32 and p["W"] > 512 for p in cases) and any(p["t"] == 0 for p in cases) and any(p["H"] * p["W"] == 1 for p in cases)


# ---- the sixth tier: the operand-preparation kernels (gemm_planes.hip) and the producers' maxima (rowops.hip, attention_bwd.hip, the pair
# GEMMs' epilogues).  Only the patch embeddings' GEMMs have host queries; every other rule is restated in tests/_sweep_cases.py beside the
# function it comes from.
def test_sixth_tier_is_appended_and_the_first_five_are_what_they_were():
    import zlib

    assert PREP_OPS == ("convert", "split_dual", "split_multi", "transpose_pairs", "transpose_planes", "patch_embed", "grad_amax", "layernorm_long")
    earlier = [case_id(o, p) for o, p in CASES if o not in PREP_OPS]
    assert len(earlier) == 718 and zlib.crc32("\n".join(earlier).encode()) == 2505003073      # the ids of the first five tiers, unchanged (but Sinkhorn's: no persist key since the one-launch solve left)
    assert earlier[-1].startswith("bf_counts[") and [o for o, _ in CASES][718] == "convert"
    from _sweep_checks_prep import CHECK as PREP_CHECK      # (tools/fuzz_ops.py draws from OPS and runs tests/test_hip_sweep.py::run_case)

    assert set(PREP_CHECK) == set(PREP_OPS)
    # the layernorm cases the issue adds live under their own op, so that the first tier's draws keep their ids
    assert {(p["Fr"], p["Nt"], p["D"]) for p in _of("layernorm_long")} >= {(1, 8193, 64), (1, 8193, 384), (43, 197, 64), (43, 197, 384)}


def test_conversions_reach_the_grid_cap_and_every_kind_of_value():
    cases = _of("convert")
    # tt_split_pairs / tt_join_pairs / tt_split_planes: min(ceil(n / 8 / 256), 4096) workgroups of 256 threads x 8 elements - the stride loop
    # runs from n = 8 388 608 + 8 on
    assert CONVERT_CAP == 4096 * 256 * 8
    for what, step in (("pairs", 32), ("planes", 8)):
        ns = {p["n"] for p in cases if p["what"] == what}
        assert {step, CONVERT_CAP, CONVERT_CAP + step} <= ns, what
        assert {p["vals"] for p in cases if p["what"] == what} == set(VALUE_KINDS), what
    assert {p["P"] for p in cases if p["what"] == "planes"} == {1, 2, 3}
    assert {p["P"] for p in cases if p["what"] == "planes" and p["n"] > CONVERT_CAP} >= {2, 3}
    assert max(p["n"] for p in cases) == CONVERT_CAP + 32                                      # the largest tensors of the tier


def test_dual_split_every_instantiation_route_partial_count_and_scale():
    cases = _of("split_dual")
    kernels = {sd_kernel(p) for p in cases}
    # transpose_pairs_kernel<false, ROW, SUM> x 4, split_rows_kernel<SUM> x 2 (gemm_planes.hip, split_pairs_dual_impl)
    assert kernels == {("tile", r, s) for r in (False, True) for s in (False, True)} | {("rows", False), ("rows", True)}
    tile = [p for p in cases if sd_kernel(p)[0] == "tile"]
    assert {p["R"] for p in tile if p["t"]} >= {1, 31, 32, 33, 63, 64, 65, 197}
    assert {p["C"] for p in tile if p["t"] and not p["row"]} >= {1, 31, 33, 65} and {p["C"] for p in tile if p["t"] and p["row"]} >= {32, 96, 160}
    assert any(sd_rpad(p) % 64 == 32 and p["t"] for p in tile) and {p["rpad"] for p in cases} == {0, 32, 64}
    # the streaming kernel either side of each term of its gate: C % 128, the transposed output, alignment, the knob
    rows = [p for p in cases if sd_kernel(p)[0] == "rows"]
    assert {p["C"] for p in rows} >= {128, 256} and {p["R"] for p in rows} >= {1, 15, 16, 17, 63, 65, 130, 20000}
    off_gate = [p for p in cases if p["row"] and not p["t"] and sd_kernel(p)[0] == "tile"]
    assert {p["C"] for p in off_gate} >= {96, 160} and any(p["off"] and p["C"] % 128 == 0 for p in off_gate) and any(not p["sr"] and p["C"] % 128 == 0 for p in off_gate)
    # the max pass: n_part 1, 2 ... 255, 256 and capped; the scalar tail (R C % 4 != 0)
    own = [amax_n_part(p["R"] * p["C"]) for p in cases if p["scale"] == "own"]
    assert {c for _, c, _ in own} == {"1", "2..255", "256", "capped"} and {t for _, _, t in own} == {False, True}
    assert {p["R"] * p["C"] for p in cases if p["scale"] == "own"} >= {5, 4095, 4096, 4097, 255 * 4096 + 1, 256 * 4096, 4099 * 257}
    assert amax_n_part(4096) == (1, "1", False) and amax_n_part(4097) == (2, "2..255", True) and amax_n_part(256 * 4096)[:2] == (AMAX_PARTS_CAP, "256")
    assert amax_n_part(4099 * 257) == (AMAX_PARTS_CAP, "capped", True)
    for scale in ("own", "slot"):      # every magnitude and special value, from the own pass and from a slot, on both kernels
        mine = [p for p in cases if p["scale"] == scale]
        assert {p["mag"] for p in mine} >= {1.0, 1e-3, 3e-8, 1e-30} and {p["vals"] for p in mine} >= {"normal", "zero", "big", "inf"}, scale
        assert {sd_kernel(p)[0] for p in mine} == {"tile", "rows"}, scale
    from _sweep_checks_prep import slot_way      # the slot's way that carries the maximum: both halves of the 16 (a fold of 8 ways misses one)

    assert {slot_way(p) // 8 for p in cases if p["scale"] == "slot" and p["vals"] == "normal"} == {0, 1}
    assert {p["colsum"] for p in cases} == {"", "fold", "parts"} and any(p["R"] >= 4096 and p["colsum"] for p in rows) and any(p["R"] >= 4096 and p["colsum"] for p in tile)
    assert max(p["R"] * p["C"] for p in cases) == 20000 * 128


def test_table_split_every_launch_count():
    cases = _of("split_multi")
    assert {p["n"] for p in cases} >= {1, 2, MULTI_MAXN, MULTI_MAXN + 1, 2 * MULTI_MAXN + 1}      # PairTable::MAXN entries per launch
    assert {(p["n"] + MULTI_MAXN - 1) // MULTI_MAXN for p in cases} >= {1, 2, 3}
    for p in cases:
        ents = multi_entries(p)
        tile0 = list(itertools.accumulate([0] + [((ceil_to(R, 32) + 63) // 64) * ((C + 63) // 64) for R, C, _ in ents[:MULTI_MAXN]]))
        if p["n"] >= MULTI_MAXN:
            assert {o for _, _, o in ents} == {"t", "row", "both"} and (1, 1, "t") in ents and (65, 96, "both") in ents
            assert any(a // 64 != b // 64 for a, b in zip(tile0, tile0[1:]))                         # tile0 crosses a multiple of 64


def test_transposes_every_store_branch():
    cases = _of("transpose_planes")
    assert {tp_store_branch(tp_rpad(p)) for p in cases if p["rpad"] == "R"} == {"scalar", "quad", "quad64"}      # transpose_planes_kernel: Rpad % 4, % 64
    for cs in (0, 1):
        assert {tp_store_branch(tp_rpad(p)) for p in cases if p["colsum"] == cs} == {"scalar", "quad", "quad64"}, cs
    assert {p["rpad"] for p in cases} == {"R", "c64", "c64+64"}
    assert {p["R"] for p in cases} >= {1, 3, 63, 64, 65, 197} and {p["C"] for p in cases} >= {1, 63, 64, 65, 200}
    assert any(p["R"] >= 4096 and p["colsum"] for p in cases)
    tp = _of("transpose_pairs")
    assert {p["R"] for p in tp} >= {1, 31, 32, 33, 63, 64, 65, 197} and {p["C"] for p in tp} >= {32, 96, 160} and {p["rpad"] for p in tp} >= {0, 64}


def test_patch_embedding_every_route(lib):
    cases = _of("patch_embed")
    n_of = lambda p: p["gh"] * p["gw"]
    f32 = [p for p in cases if p["mode"] == "f32"]
    routes = {patch_f32_route(p, lib.tt_gemm_tile_choice(p["F"] * n_of(p), p["D"], 1)) for p in f32}
    assert routes == {"lean64", "lean128", "general"}
    general = [p for p in f32 if patch_f32_route(p, 3) == "general"]
    assert any(p["P"] == 8 for p in general) and any(p["D"] % 64 for p in general) and any(not p["lean"] and p["P"] == 16 and p["D"] % 64 == 0 for p in general)
    for mode, K_mod in (("f32", 1), ("pairs", 32), ("planes", 64)):
        mine = [p for p in cases if p["mode"] == mode]
        assert all((p["C"] * p["P"] * p["P"]) % K_mod == 0 for p in mine), mode
        assert any(p["gh"] > p["gw"] > 1 for p in mine) and any(1 < p["gh"] < p["gw"] for p in mine), mode      # a gh / gw mix-up changes the result
        assert any(p["gh"] == 1 for p in mine) and any(p["gw"] == 1 for p in mine) and {p["P"] for p in mine} == {4, 8, 16}, mode
        assert {p["D"] for p in mine} >= {64, 128, 192} and {p["fmap"] for p in mine} == {"", "rev", "repeat"}, mode
        assert all((p["F"] * (n_of(p) + 1)) % 64 for p in mine if p["F"] < 100), mode
    assert {p["C"] for p in cases} >= {1, 2, 3}
    M_K = lambda p: (p["F"] * (n_of(p) + 1), p["C"] * p["P"] * p["P"])
    # (the GEMM of the pair / plane entries: residual = y = tokens, bias, no activation)
    assert {lib.tt_linear_fwd_pairs_route(M_K(p)[0], p["D"], M_K(p)[1], 0, 1, 1, 1, 0, 0) for p in cases if p["mode"] == "pairs"} == {0, 8}
    assert {lib.tt_linear_fwd_planes_route(1, M_K(p)[0], p["D"], M_K(p)[1], 0, 1, 1, 1, 0, 0) != 0 for p in cases if p["mode"] == "planes"} == {False, True}
    persistent = [p for p in cases if p["mode"] != "f32" and p["F"] > 100]
    assert len(persistent) == 2 and not any(prep_case_on_twin("patch_embed", p) for p in persistent)


def test_gradient_maxima_every_producer_kernel_and_regime(lib):
    cases = _of("grad_amax")
    ln = [p for p in cases if p["producer"] == "ln_bwd"]
    plans = [ln_bwd_plan(p["rows"], p["D"], p["off"]) for p in ln]
    # rowops.hip, tt_layernorm_bwd: the general kernel and layernorm_bwd_vec_kernel<1|3|6>; ln_bwd_wgs: 1, 8 and more than 8 rows per
    # workgroup, and workgroups without a row behind the cap of 1024
    assert {k for k, *_ in plans} == {"general", "vec1", "vec3", "vec6"}
    for kern in ("general", "vec3"):
        assert {min(rpw, 9) for k, _, rpw, _ in plans if k == kern} >= {1, 8, 9}, kern
    assert any(w == LN_BWD_WG_CAP and idle > 0 for _, w, _, idle in plans) and ln_bwd_plan(8193, 64) == ("general", 1024, 9, 113)
    assert {p["D"] for p in ln if ln_bwd_plan(p["rows"], p["D"], p["off"])[0] == "general" and not p["off"]} >= {1, 63, 64, 65, 96, 1000}
    assert {p["rows"] for p in ln} >= {1, 2, 3, 7, 8, 9, 17, 8192, 8193, 8200}
    assert {p["D"] for p in ln if p["off"]} >= {128, 384, 768}                                    # the same D, one float off 8-byte alignment
    assert any(p["N"] for p in ln) and any(p["accum"] for p in ln) and not any(p["N"] and p["accum"] for p in ln)      # (together: refused)
    for kern in ("general", "vec1", "vec3", "vec6"):
        assert any(p["accum"] for p in ln if ln_bwd_plan(p["rows"], p["D"], p["off"])[0] == kern), kern
    l2 = [p for p in cases if p["producer"] == "l2_bwd"]
    assert {p["rows"] for p in l2} >= {1, 3, 4, 5} and {p["D"] for p in l2} >= {1, 64, 65, 1024}
    for prod in ("attn_bwd", "attn_bwd_pairs"):
        at = [p for p in cases if p["producer"] == prod]
        assert {p["N"] for p in at} >= {1, 63, 64, 65, 197, 257} and {p["H"] for p in at} >= {1, 3} and {p["F"] for p in at} >= {1, 2}, prod
    assert {p["dslot"] for p in cases if p["producer"] == "attn_bwd_pairs"} == {0, 1}
    assert {p["gscale"] for p in cases if "gscale" in p} >= {1.0, 1e-7}
    # the general pair kernel (dx [M, K]: the GEMM's N is K, its reduction N): linear_pairs_impl's four tiles; small M on the small grids
    gen = [p for p in cases if p["producer"] == "dgrad_general"]
    assert {pairs_general_tile(p["M"], p["K"], p["N"], 1, NCU) for p in gen} == {"big", "wide", "small4", "small3"}
    assert {p["M"] for p in gen if pairs_general_tile(p["M"], p["K"], p["N"]) == "small4"} >= {1, 63, 65, 130}
    # x gelu': each regime of the persistent kernel (pairs8_regime above) with a ragged last row tile, and the general kernel
    gg = [p for p in cases if p["producer"] == "dgrad_gelu"]
    assert {pairs8_regime(p["M"], p["K"], p["N"]) for p in gg} == {"half", "round_robin", "ksplit", None}
    for p in gg:
        persistent = pairs8_regime(p["M"], p["K"], p["N"]) is not None
        assert persistent == hip_ops.linear_bwd_data_pairs_is_persistent(p["M"], p["N"], p["K"]), p
        assert not persistent or (p["M"] % 256 and not prep_case_on_twin("grad_amax", p)), p
