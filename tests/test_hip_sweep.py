"""The ragged-shape kernel sweep: every case of the seeded table (tests/_sweep_cases.py) against fp64 torch or the oracle, at the suite's own
bounds - TOL_F32 (max-normalised) and TOL_L2 (relative L2) as in tests/test_hip_pairs.py, tighter where tools/fuzz_ops.py held a kernel to a
tighter one; the f32-class rule for the split modes (not worse than the exact-f32 kernel on the same operands); 5e-5 against O.sinkhorn;
run-to-run bit equality on the persistent kernels.  tests/test_sweep_routes.py checks, without a GPU, that the table reaches every route.

The second tier - the evaluator, optimizer and mask kernels (EVAL_OPS) - runs the checks of tests/_sweep_checks_eval.py on the HIP library:
the same inputs, fp64 references, bounds and capped excuse rules that tests/test_sweep_eval_host.py holds the plain-C twins to.  Behind it,
the accepted domain of each of those entries at its edge: the largest size computes correctly (a case of the table or a call below), the
first size beyond is refused by the launcher's own check, with its own message, before anything is launched.

The third tier - temporal label propagation (PROP_OPS: the square entries' six per-query kernels, slot regimes and chunkings, the grid
entry, its up-sampler) - runs the checks of tests/_sweep_checks_prop.py the same way: one-frame fp64 reference, exact-selection and
real-valued inputs, the bit-for-bit equalities between the entries; tests/test_sweep_prop_host.py is its host half.  Its domain edges
follow the second tier's.

The fourth tier - the linear probe's kernels and the clip input pipeline (HEAD_OPS) - runs the checks of tests/_sweep_checks_head.py: fp64
references at the existing linear-probe bounds, bit equality with the Pillow-pinned image oracle; tests/test_sweep_head_host.py is its host
half, and the probe's domain edges follow the second tier's.

The fifth tier - the tiled k-means pair, the batched assignment, the fused batched fit and the three metric counters (METRIC_OPS) - runs the
checks of tests/_sweep_checks_metric.py: fp64 references at the second tier's k-means rules, oracle.timet_oracle.kmeans_lloyd for the fit, the
k-means contract's bit equalities, exact equality with the NumPy restatements of the counters; tests/test_sweep_metric_host.py is its host
half.  Its refusals at the edge stand beside the second tier's below.

The sixth tier - the operand-preparation kernels of gemm_planes.hip (the pair / plane conversions, the dual split, its table form, the two
transposes, the patch embeddings' im2col front ends) and the maxima the backward producers publish for the split's scale (PREP_OPS) - runs
the checks of tests/_sweep_checks_prep.py through the C ABI into guarded buffers: bit equality with the NumPy restatements of the two
formats, exact maxima, fp64 references for the sums, the tokens and the producers' dx; tests/test_sweep_prep_host.py is its host half.  Its
refusals at the edge are at the end of this file.

``run_case`` is also what tools/fuzz_ops.py runs on more seeds of the same generator."""
import json
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _sweep_cases import EVAL_OPS, HEAD_OPS, METRIC_OPS, PAIR_EPILOGUES, PREP_OPS, PROP_OPS, case_id, table
from _sweep_checks_eval import HipSide, run_eval_case
from _sweep_checks_head import HeadHip, run_head_case
from _sweep_checks_metric import MetricHip, run_metric_case
from _sweep_checks_prep import PrepHip, assert_refused, domain_edges, ln_refuses_amax_with_drop_and_accum, run_prep_case
from _sweep_checks_prop import PropHip, run_prop_case

pytestmark = pytest.mark.gpu
TOL_F32 = 2e-5
TOL_L2 = 2e-6
TOL_PAIRS = 2e-6      # tools/fuzz_ops.py's bound for the pair GEMM's outputs (max-normalised)
TOL_BWD = 5e-5        # LayerNorm / attention backward (tests/test_hip_ops.py)
TOL_SK = 5e-5         # Sinkhorn against O.sinkhorn
# The f32-class comparison of a pair product with the exact-f32 kernel needs a reduction this long.  The split holds each operand to ~2^-22
# (2.4e-7) relative; an exact-f32 product over a few terms carries only a few fp32 roundings (6e-8 each), so on short reductions the split's
# own error is the larger by construction.  Measured pair / f32 relative L2: 1.06 at M 1 N 64 K 32, 1.004 at M 69 N 192 K 64; dw 1.60 at a
# reduction of M = 7.  (tests/test_hip_pairs.py holds the rule at K >= 96.)  TOL_L2 still holds everywhere.
F32_CLASS_MIN = 96
CASES = table()
WORST: dict = {}


def rel_err(a, b) -> float:
    a, b = a.detach().double(), b.detach().double().to(a.device)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rel_l2(a, b) -> float:
    a, b = a.detach().double(), b.detach().double().to(a.device)
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b).clamp_min(1e-30))


def _note(op):
    def note(what, err, tol, strict=False):
        key = f"{op}: {what}"
        w = WORST.setdefault(key, [0.0, tol])
        w[0] = max(w[0], err)
        assert (err < tol) if not strict else (err <= tol), (key, err, tol)
    return note


def _gen(op, p):
    g = torch.Generator().manual_seed(zlib.crc32(case_id(op, p).encode()))
    return lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).cuda()


def _linear_f32(ops, p, rnd, note):
    M, N, K = p["M"], p["N"], p["K"]
    x, w, b, r = rnd(M, K), rnd(N, K, scale=0.1), rnd(N), rnd(M, N)
    pre = x.double() @ w.double().t() + b.double()
    ref = (F.gelu(pre) if p["act"] else pre) + (r.double() if p["res"] else 0)
    y = ops.linear_fwd(x, w, b, residual=r if p["res"] else None, act=p["act"])
    note("y max", rel_err(y, ref), TOL_F32)
    note("y l2", rel_l2(y, ref), TOL_L2)
    dy = rnd(M, N)
    dx = ops.linear_bwd_data(dy, w)
    note("dx max", rel_err(dx, dy.double() @ w.double()), TOL_F32)
    dw, db = ops.linear_bwd_weight(dy, x)
    note("dw max", rel_err(dw, dy.double().t() @ x.double()), TOL_F32)
    note("db max", rel_err(db, dy.double().sum(0)), TOL_F32)


def _linear_pairs(ops, p, rnd, note):
    M, N, K = p["M"], p["N"], p["K"]
    e = PAIR_EPILOGUES[p["epi"]]
    x, w, b, r = rnd(M, K), rnd(N, K, scale=0.1), rnd(N), rnd(M, N)
    xp, wp = ops.split_pairs(x), ops.split_pairs(w)
    pre = x.double() @ w.double().t() + b.double()
    ref = (F.gelu(pre) if e["act"] else pre) + (r.double() if e["res"] else 0)
    run = lambda: ops.linear_fwd_pairs(xp, wp, b, residual=r if e["res"] else None, act=e["act"], out_f32=bool(e["out_f32"]),
                                       out_pairs=bool(e["out_pairs"]), save_pre=bool(e["save_pre"]))
    o = run()
    if e["out_pairs"]:
        note("pairs max", rel_err(ops.join_pairs(o["pairs"]), ref), TOL_PAIRS)
    if e["save_pre"]:
        note("pre max", rel_err(o["pre"], pre), TOL_PAIRS)
    if e["out_f32"]:
        note("y max", rel_err(o["y"], ref), TOL_PAIRS)
        note("y l2", rel_l2(o["y"], ref), TOL_L2)
        # f32-class: not worse than the exact-f32 kernel on the same operands (tests/test_hip_pairs.py::test_linear_pairs: 5 % slack on the
        # max, one element's luck; none on the L2 norm) - from a reduction of F32_CLASS_MIN terms on (see there)
        if K >= F32_CLASS_MIN:
            y32 = ops.linear_fwd(x, w, b, residual=r if e["res"] else None, act=e["act"])
            note("y l2 / f32 kernel's", rel_l2(o["y"], ref) / max(rel_l2(y32, ref), 1e-30), 1.0, strict=True)
            note("y max / f32 kernel's", rel_err(o["y"], ref) / max(rel_err(y32, ref), 1e-30), 1.05, strict=True)
    route = ops._lib.load().tt_linear_fwd_pairs_route(M, N, K, e["act"], 1, e["res"], e["out_f32"], e["out_pairs"], e["save_pre"])
    if route == 8:   # run-to-run bit equality of the persistent kernel (fixed K-split fold order)
        o2 = run()
        for k in ("y", "pairs", "pre"):
            assert (o[k] is None) or torch.equal(o[k], o2[k]), k


def _linear_planes(ops, p, rnd, note):
    P, M, N, K = p["P"], p["M"], p["N"], p["K"]
    x, w, b, r = rnd(M, K), rnd(N, K, scale=0.1), rnd(N), rnd(M, N)
    xp, wp = ops.split_planes(x, P), ops.split_planes(w, P)
    run = lambda: ops.linear_fwd_planes(xp, wp, b, residual=r if p["res"] else None, act=p["act"])["y"]
    y = run()
    pre = xp.double().sum(0) @ wp.double().sum(0).t() + b.double()    # the planes' own values: the GEMM's accuracy, not the split's
    ref = (F.gelu(pre) if p["act"] else pre) + (r.double() if p["res"] else 0)
    note(f"P={P} y max", rel_err(y, ref), TOL_F32)
    note(f"P={P} y l2", rel_l2(y, ref), TOL_L2)
    if ops._lib.load().tt_linear_fwd_planes_route(P, M, N, K, p["act"], 1, p["res"], 1, 0, 0) == 8:
        assert torch.equal(run(), y)


def _bwd_pairs(ops, p, rnd, note):
    from timetuning_amd import engine

    M, N, K, tn = p["M"], p["N"], p["K"], bool(p["tn"])
    dy, w, x, pre = rnd(M, N, scale=p["mag"]), rnd(N, K, scale=0.05), rnd(M, K), rnd(M, K)
    gp = pre if p["gelu"] else None
    xp = ops.split_pairs(x)
    keep = ops.TN_WGRAD
    ops.TN_WGRAD = tn
    try:
        assert ops.bwd_weight_pairs_tn_ok(M, N, K) == (tn and N % 128 == 0 and K % 128 == 0)
        dx, dw, db = engine._bwd_both_pairs(dy, w, xp, gp)
        if ops.bwd_weight_pairs_tn_ok(M, N, K) or ops.linear_bwd_data_pairs_is_persistent(M, N, K):   # fixed fold orders
            dx2, dw2, db2 = engine._bwd_both_pairs(dy, w, xp, gp)
            assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    finally:
        ops.TN_WGRAD = keep
    pd = pre.double().requires_grad_(True)
    F.gelu(pd).sum().backward()
    dx_ref = (dy.double() @ w.double()) * (pd.grad if p["gelu"] else 1.0)
    dw_ref = dy.double().t() @ x.double()
    note("dx max", rel_err(dx, dx_ref), TOL_F32)
    note("dx l2", rel_l2(dx, dx_ref), TOL_L2)
    note("dw max", rel_err(dw, dw_ref), TOL_F32)
    note("dw l2", rel_l2(dw, dw_ref), TOL_L2)
    note("db max", rel_err(db, dy.double().sum(0)), TOL_F32)
    # f32-class, as tests/test_hip_pairs.py::test_backward_products_on_pairs holds it (5 % on the data gradient's L2), where the product's
    # reduction (M for dw, N for dx) has F32_CLASS_MIN terms or more
    dx32, dw32, _ = ops.linear_bwd(dy, w, x, gelu_pre=gp)
    if M >= F32_CLASS_MIN:
        note("dw l2 / f32 kernel's", rel_l2(dw, dw_ref) / max(rel_l2(dw32, dw_ref), 1e-30), 1.0, strict=True)
    if N >= F32_CLASS_MIN:
        note("dx l2 / f32 kernel's", rel_l2(dx, dx_ref) / max(rel_l2(dx32, dx_ref), 1e-30), 1.05, strict=True)


def _layernorm(ops, p, rnd, note):
    Fr, Nt, D, drop = p["Fr"], p["Nt"], p["D"], bool(p["drop"])
    x, g, b = rnd(Fr, Nt, D, scale=2.0) + 0.3, 1 + rnd(D, scale=0.1), rnd(D, scale=0.1)
    xd, gd, bd = (t.double().requires_grad_(True) for t in (x, g, b))
    ref = F.layer_norm(xd, (D,), gd, bd, 1e-6)
    ref = ref[:, 1:] if drop else ref
    dy = rnd(*ref.shape)
    ref.backward(dy.double())
    y, mean, rstd = ops.layernorm_fwd(x, g, b, save_stats=True, drop_first_token=drop)
    note("y max", rel_err(y.reshape(ref.shape), ref), TOL_F32)
    if p["pairs"]:
        yp = ops.join_pairs(ops.layernorm_fwd_pairs(x, g, b, drop_first_token=drop)).reshape(ref.shape)
        note("pairs max", rel_err(yp, ref), TOL_F32)
        note("pairs l2", rel_l2(yp, ref), TOL_L2)
    dx, dg, dbt = ops.layernorm_bwd(dy.reshape(-1, D).contiguous(), x, g, mean, rstd, drop_first_token=drop)
    note("dx max", rel_err(dx.reshape(x.shape), xd.grad), TOL_BWD)
    note("dgamma max", rel_err(dg, gd.grad), TOL_BWD)
    note("dbeta max", rel_err(dbt, bd.grad), TOL_BWD)


def _l2norm(ops, p, rnd, note):
    rows, D = p["rows"], p["D"]
    x, dxn = rnd(rows, D, scale=4.0), rnd(rows, D)
    z = rows // 2
    if p["zero_row"]:
        x[z] = 0.0               # F.normalize's eps branch: x / max(|x|, 1e-12)
    xd = x.double().requires_grad_(True)
    ref = F.normalize(xd, dim=-1)
    ref.backward(dxn.double())
    xn, inv = ops.l2norm_fwd(x, save_inv=True)
    note("y max", rel_err(xn, ref), TOL_F32)
    dx = ops.l2norm_bwd(dxn, xn, inv)
    live = torch.ones(rows, dtype=torch.bool, device="cuda")
    if p["zero_row"]:
        live[z] = False
        assert torch.equal(xn[z], torch.zeros_like(xn[z]))
        note("dx max (zero row: dxn / eps)", rel_err(dx[z], xd.grad[z]), TOL_F32)
    if live.any():
        note("dx max", rel_err(dx[live], xd.grad[live]), TOL_F32)


def _attention(ops, p, rnd, note):
    Fr, N, H = p["Fr"], p["N"], p["H"]
    D = 64 * H
    qkv, do = rnd(Fr, N, 3 * D, scale=1.5), rnd(Fr, N, D)
    qd = qkv.double().requires_grad_(True)
    q, k, v = qd.view(Fr, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    sc = q @ k.transpose(-1, -2) * 0.125
    ref = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(Fr, N, D)
    lse_ref = torch.logsumexp(sc, -1).detach()
    ref.backward(do.double())
    ref = ref.detach()
    out, lse, _ = ops.attention_fwd(qkv, H, save_lse=True)
    note("f32 out max", rel_err(out, ref), TOL_F32)
    note("f32 lse max", rel_err(lse, lse_ref), TOL_F32)
    note("f32 dqkv max", rel_err(ops.attention_bwd(qkv, out, do, lse, H), qd.grad), TOL_BWD)
    # the pair backward at both gradient scales: TOL_L2, and within 2x the f32 kernels' relative L2.  NOT DESIGN section 3's f32-class rule
    # (not above the f32 kernels' own): the pair backward misses it at most shapes, 1.0 - 1.8x measured (tests/test_hip_ops.py::
    # test_attention_fwd_bwd lists the numbers).  At N = 1 the f32 kernels are exact (dq = dk = 0, dv = dout) and the pairs are not.
    for gs in (1.0, 1e-7):
        e32 = rel_l2(ops.attention_bwd(qkv, out, do * gs, lse, H), qd.grad * gs)
        dq_p = ops.attention_bwd(qkv, out, do * gs, lse, H, pair_products=True)
        note("pair dqkv max", rel_err(dq_p, qd.grad * gs), TOL_BWD)
        note("pair dqkv l2", rel_l2(dq_p, qd.grad * gs), TOL_L2)
        if N > 1:
            note("pair dqkv l2 / f32 kernel's", rel_l2(dq_p, qd.grad * gs) / max(e32, 1e-30), 2.0, strict=True)
    # the pair forward: resident (N <= 256) or KV-tiled (beyond, or forced)
    qkvp = ops.split_pairs(qkv.view(Fr * N, 3 * D)).view(Fr, N, 6 * D)
    with ops.tuning_knob("TT_ATTN_PAIRS_FLASH", p["flash"]):
        op_, of_, lsep = ops.attention_fwd_pairs(qkvp, H, out_pairs=True, out_f32=True, save_lse=True)
    note("pair out max", rel_err(of_, ref), 3e-6)                     # tools/fuzz_ops.py's bound
    note("pair out l2", rel_l2(of_, ref), TOL_L2)
    note("pair out (pairs) max", rel_err(ops.join_pairs(op_.view(Fr * N, -1)).view(Fr, N, D), ref), 3e-6)
    note("pair lse max", rel_err(lsep, lse_ref), 1e-5)
    if N > 1:   # (one token: the f32 kernel returns v exactly, the pair kernel v to ~2^-22 - measured 5.7e-8 relative L2)
        note("pair out l2 / f32 kernel's", rel_l2(of_, ref) / max(rel_l2(out, ref), 1e-30), 1.0, strict=True)
    ops.check_pair_range()


def _ce(ops, p, rnd, note):
    rows, K = p["rows"], p["K"]
    s = rnd(rows, K, scale=0.3)
    lab = torch.from_numpy(np.random.default_rng(rows * 1000 + K).integers(0, K, rows)).cuda()
    lab[0], lab[-1] = 0, K - 1
    wgt = (rnd(rows) > -0.3).float() if p["weighted"] else None
    sd = s.double().requires_grad_(True)
    ref = F.cross_entropy(sd / 0.1, lab, reduction="none")
    ref = (ref * (wgt.double() if wgt is not None else 1.0)).mean()
    ref.backward()
    loss, ds = ops.ce_loss_fwd_bwd(s, lab, 0.1, row_weight=wgt)
    note("loss abs", abs(loss.item() - ref.item()), 1e-5)
    note("dscores max", rel_err(ds, sd.grad), TOL_F32)


def _scores(rnd, B, K):
    x, pr = F.normalize(rnd(B, 48), dim=1), F.normalize(rnd(K, 48), dim=1)
    return (x @ pr.t()).contiguous()


def _sk_ref(scores, iters):
    from oracle import timet_oracle as O

    return O.sinkhorn(torch.exp(scores.double().cpu() / 0.05).t(), iters)


def _sinkhorn(ops, p, rnd, note):
    B, K, it, r0, n = p["B"], p["K"], p["iters"], p["row0"], p["rows_out"]
    scores = _scores(rnd, B, K)
    ref = _sk_ref(scores, it)[r0:r0 + n]
    note("q max", rel_err(ops.sinkhorn(scores, it, row0=r0, rows_out=n), ref), TOL_SK)


def _sinkhorn_from_q(ops, p, rnd, note):
    B, K, it = p["B"], p["K"], p["iters"]
    scores = _scores(rnd, B, K)
    Q = torch.exp(scores / 0.05)
    q = ops.sinkhorn_from_q(Q if p["transposed"] else Q.t().contiguous(), it, transposed=bool(p["transposed"]))
    note("q max", rel_err(q, _sk_ref(scores, it)), TOL_SK)


def _sinkhorn_local(ops, p, rnd, note):
    B, K, it = p["B"], p["K"], p["iters"]
    scores = _scores(rnd, B, K)
    sk = ops.SinkhornLocal(B, B, K, torch.device("cuda"))
    u = sk.begin(scores, 0.05)
    for i in range(it - 1):
        u = sk.step(u)
    q = sk.end(u if it > 0 else None)
    note("q max", rel_err(q, _sk_ref(scores, it)), TOL_SK)


def _queue_push(ops, p, rnd, note):
    Q, D, m = p["Q"], p["D"], p["m"]
    queue, feats = rnd(Q, D), rnd(m + 7, D)
    idx = torch.randperm(m + 7, generator=torch.Generator().manual_seed(Q * 7 + m))[:m].cuda()
    ref = queue.clone()
    ref[m:] = queue[:Q - m].clone()
    ref[:m] = feats[idx]
    assert torch.equal(ops.queue_push_(queue, feats, idx), ref)


CHECK = {"linear_f32": _linear_f32, "linear_pairs": _linear_pairs, "linear_planes": _linear_planes, "bwd_pairs": _bwd_pairs,
         "layernorm": _layernorm, "l2norm": _l2norm, "attention": _attention, "ce": _ce, "sinkhorn": _sinkhorn,
         "sinkhorn_from_q": _sinkhorn_from_q, "sinkhorn_local": _sinkhorn_local, "queue_push": _queue_push}


def run_case(op: str, params: dict, worst: dict = None) -> None:
    """Runs one case of the table on cuda:0; raises AssertionError on a bound it misses.  ``worst``: {"op: what": [max error, bound]}."""
    from timetuning_amd import hip_ops as ops

    global WORST
    keep = WORST
    if worst is not None:
        WORST = worst
    try:
        if op in EVAL_OPS:
            run_eval_case(HipSide(), op, params, WORST)
        elif op in PROP_OPS:
            run_prop_case(PropHip(), op, params, WORST)
        elif op in HEAD_OPS:
            run_head_case(HeadHip(), op, params, WORST)
        elif op in METRIC_OPS:
            run_metric_case(MetricHip(), op, params, WORST)
        elif op in PREP_OPS:
            run_prep_case(PrepHip(), op, params, WORST)
        else:
            CHECK[op](ops, params, _gen(op, params), _note(op))
    finally:
        WORST = keep


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("TT_SWEEP_REPORT")
    if path:   # the worst error per op and its bound (what a pull request touching these kernels reports)
        with open(path, "w") as f:
            json.dump(WORST, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("op,params", CASES, ids=[case_id(o, p) for o, p in CASES])
def test_sweep(op, params):
    run_case(op, params)


# ---- the accepted domains of the second tier's entries, at the edge (include/timetuning_hip.h states them).  Every refusal below is a
# host-side TT_REQUIRE: nothing is launched.
def _refused(match):
    from timetuning_amd import _lib

    return pytest.raises(_lib.HipLibraryError, match=match)


def _z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


@pytest.mark.parametrize("d,k,ok", [(64, 252, True), (64, 253, False), (16, 1024, True), (16, 1025, False), (128, 128, True), (128, 129, False),
                                    (1, 16384, True), (1, 16385, False)])
def test_kmeans_entries_share_one_domain(d, k, ok):
    """Largest accepted (d, k) - they compute correctly in the table above (kmeans_assign / kmeans_accumulate at k * d = 16384 and at
    d = 64, k = 252) - and the first one beyond: BOTH entries refuse it, so that no run gets through the assignment and fails in the update."""
    from timetuning_amd import hip_ops as ops

    assert ops.kmeans_shape_ok(d, k) == ok
    x, c, lab = _z(300, d), _z(k, d), _z(300, dtype=torch.int32)
    if ok:
        labels = ops.kmeans_assign(x, c)
        assert int(labels.max()) == 0                                            # equal distances everywhere: the first centroid
        sums, counts = ops.kmeans_accumulate(x, lab, k)
        assert int(counts[0]) == 300 and int(counts.sum()) == 300 and float(sums.abs().max()) == 0.0
    else:
        msg = r"k \* d = %d exceeds 16384" % (k * d) if k * d > 16384 else r"k = %d, d = %d" % (k, d)
        with _refused("kmeans_assign: " + msg):
            ops.kmeans_assign(x, c)
        with _refused("kmeans_accumulate: " + msg):
            ops.kmeans_accumulate(x, lab, k)


@pytest.mark.parametrize("entry", ["upsample_bilinear_tokens", "upsample_argmax_f32", "upsample_argmax"])
def test_upsampling_takes_65535_maps_and_refuses_more(entry):
    """M rides on gridDim.y: 65535 maps (1 x 1 each, to 2 x 2) are each resampled, 65536 are refused by the launcher."""
    from timetuning_amd import hip_ops as ops

    fn = getattr(ops, entry)
    dt = torch.float64 if entry == "upsample_argmax" else torch.float32
    M, K = 65535, 1 if entry == "upsample_bilinear_tokens" else 3
    x = torch.randn(M, 1, K, generator=torch.Generator().manual_seed(5)).to(dt).cuda()
    out = fn(x, 2)
    if entry == "upsample_bilinear_tokens":
        assert torch.equal(out, x.expand(M, 4, 1))                               # one source pixel: every output pixel is its value
    else:
        assert torch.equal(out, x.argmax(-1).view(M, 1, 1).expand(M, 2, 2))
    with _refused(f"{entry}: 65536 maps of 2x2 exceed one launch"):
        fn(_z(65536, 1, K, dtype=dt), 2)


def test_table_and_class_limits():
    from timetuning_amd import _lib, hip_ops as ops

    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    # TT_MAX_TENSORS = 40 per table (40 and, through the wrappers' chunks, more: the adamw cases above); 41 in one call is refused
    tab = (_lib.AdamwTensor * 41)()
    one = _z(4)
    for j in range(41):
        tab[j] = _lib.AdamwTensor(one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(), 4, 0.0, 0.0)
    with _refused(r"adamw: need 1\.\.40 tensors"):
        _lib.check(lib.tt_adamw_step(tab, 41, 1, 0.9, 0.999, 1e-8, st), "tt_adamw_step")
    with _refused(r"scale_tensors: need 1\.\.40 tensors"):
        _lib.check(lib.tt_scale_tensors(tab, 41, one.data_ptr(), st), "tt_scale_tensors")
    with _refused("adamw: need"):
        _lib.check(lib.tt_adamw_step(tab, 1, 0, 0.9, 0.999, 1e-8, st), "tt_adamw_step")          # step counts from 1
    # C <= 4096 classes: 4096 counts correctly (global atomics), 4097 is refused
    g = torch.Generator().manual_seed(6)
    pred, gt = torch.randint(0, 4096, (20000,), generator=g), torch.randint(0, 4096, (20000,), generator=g)
    want = torch.bincount(gt * 4096 + pred, minlength=4096 * 4096).view(4096, 4096)
    assert torch.equal(ops.confusion_counts(pred.cuda(), gt.cuda(), 4096).cpu(), want)
    with _refused(r"confusion_counts: need 0 < classes <= 4096 \(got 4097\)"):
        ops.confusion_counts(pred.cuda(), gt.cuda(), 4097)
    # 1024 feature columns for the moments (a case above); 1025 refused
    with _refused("col_moments: need 0 < cols <= 1024"):
        ops.col_moments(_z(3, 1025))


def test_mask_position_and_row_op_limits():
    from timetuning_amd import hip_ops as ops

    # 1024 patches (g = 32: cases above), 33 x 33 refused; the 7-tap blur reflects over 3 pixels: g = 3 refused; head_dim <= 128, % 4
    with _refused(r"foreground_mask_from_probs: need N = g\*g \+ 1 <= 1025 \(got N=1090 g=33\)"):
        ops.foreground_mask_from_probs(_z(1, 2, 33 * 33 + 1), 33)
    with _refused("foreground_mask_from_probs: blur kernel 7 needs odd size"):
        ops.foreground_mask_from_probs(_z(1, 2, 10), 3)
    with _refused("foreground_mask: blur kernel 7 needs odd size"):
        ops.foreground_mask(_z(1, 10, 3 * 8), 2, 3)
    with _refused("foreground_mask: head_dim 132 must be a multiple of 4, <= 128"):
        ops.foreground_mask(_z(1, 17, 3 * 132), 1, 4)
    with _refused("foreground_mask: head_dim 6 must be a multiple of 4"):
        ops.foreground_mask(_z(1, 17, 3 * 6), 1, 4)
    # D % 4 for the position table; 16-byte alignment for it and for the EMA; cols % 4 for the row scale; D <= 1024 for the row normalisation
    with _refused("pos_embed_interpolate: D must be a multiple of 4"):
        ops.pos_embed_interpolate(_z(1 + 4, 6), 3, 3)
    with _refused("pos_embed_interpolate: D must be a multiple of 4, buffers 16-byte aligned"):
        ops.pos_embed_interpolate(_z(1 + (1 + 4) * 4)[1:].view(1 + 4, 4), 3, 3)
    with _refused("ema: buffers must be 16-byte aligned"):
        ops.ema_update_(_z(9)[1:], _z(8), 0.5)
    with _refused("scale_rows: cols must be a multiple of 4"):
        ops.scale_rows_(_z(3, 6), _z(3))
    with _refused("l2norm_fwd: bad arguments"):
        ops.normalize_rows_(_z(2, 1025))
    assert rel_err(ops.normalize_rows_(torch.full((2, 1024), 2.0, device="cuda")), torch.full((2, 1024), 2.0 / 64.0)) < TOL_F32


# ---- the accepted domains of the fifth tier's entries, at the edge (kmeans_fit.hip: kf_fit_shape_ok; kmeans.hip: km_tiled_shape_ok,
# resolve_tile; confusion.hip: cs_route and the entry's own checks).  The largest accepted shapes compute correctly as cases of the table
# above (the fit at (64, 127) and (50, 163), d = 1024 tiled, n = 2^20); every refusal below is a host-side TT_REQUIRE: nothing is launched.
@pytest.mark.parametrize("n,d,k,msg", [(700, 64, 128, r"n = 700, d = 64, k = 128: need 1 <= d <= 64, 1 <= k <= n <= 1048576 and 16 k d \+ 4 k = 131584 bytes of LDS within 131072"),
                                       (900, 50, 164, r"n = 900, d = 50, k = 164: need .* 16 k d \+ 4 k = 131856 bytes of LDS within 131072"),
                                       (300, 65, 3, r"n = 300, d = 65, k = 3: need 1 <= d <= 64"),
                                       (3, 2, 5, r"n = 3 points are fewer than k = 5 clusters"),
                                       ((1 << 20) + 1, 1, 1, r"n = 1048577, d = 1, k = 1: need 1 <= d <= 64, 1 <= k <= n <= 1048576")])
def test_fused_fit_refuses_beyond_its_domain(n, d, k, msg):
    from timetuning_amd import _lib, hip_ops as ops

    assert not ops.kmeans_fit_shape_ok(n, d, k) and _lib.load().tt_kmeans_fit_lds_bytes(n, d, k) == 0
    assert _lib.load().tt_kmeans_fit_workspace_bytes(1, 1, n, d, k) == 0
    x, init = _z(1, n, d), torch.zeros((1, k), dtype=torch.int32)
    with _refused("kmeans_fit_batched: " + msg):
        ops.kmeans_fit_batched(x, init, 2)
    # ... and through the C entry on outputs filled beforehand: none of them is written
    lib = _lib.load()
    cent, obj, status = torch.full((1, 1, k, d), 7.0, device="cuda"), torch.full((1, 1), 7.0, dtype=torch.float64, device="cuda"), torch.full((1, 1), 7, dtype=torch.int32, device="cuda")
    ws = _z(4 * n + 16, dtype=torch.uint8)
    rc = lib.tt_kmeans_fit_batched(x.data_ptr(), init.cuda().data_ptr(), init.data_ptr(), cent.data_ptr(), obj.data_ptr(), status.data_ptr(), 1, n, d, k, 1, 2,
                                   ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and bool((cent == 7).all()) and float(obj) == 7.0 and int(status) == 7


def test_fused_fit_refuses_a_seed_outside_the_points():
    from timetuning_amd import hip_ops as ops

    x = torch.randn(2, 300, 5, generator=torch.Generator().manual_seed(3)).cuda()
    ok = torch.tensor([[0, 1, 299]], dtype=torch.int32)
    assert (ops.kmeans_fit_batched(x, ok, 1)[2] >= 0).all()                       # the last row is a seed like any other
    with _refused(r"kmeans_fit_batched: init\[1\]\[2\] = 300 is outside \[0, 300\)"):
        ops.kmeans_fit_batched(x, torch.tensor([[0, 1, 2], [3, 4, 300]], dtype=torch.int32), 1)
    with _refused(r"kmeans_fit_batched: init\[0\]\[0\] = -1 is outside \[0, 300\)"):
        ops.kmeans_fit_batched(x, torch.tensor([[-1, 1, 2]], dtype=torch.int32), 1)
    with _refused(r"kmeans_fit_batched: niter = 0, nredo = 1"):
        ops.kmeans_fit_batched(x, ok, 0)


def test_tiled_pair_refuses_beyond_its_domain():
    from timetuning_amd import hip_ops as ops

    lab = _z(40, dtype=torch.int32)
    for d in (1, 17, 64, 1024):      # the default tile is the largest: one row more is refused by both entries
        most = ops.kmeans_tile_centroids(d)
        assert most == 16384 // d
        for fn, args in ((ops.kmeans_assign_tiled, (_z(40, d), _z(3, d))), (ops.kmeans_accumulate_tiled, (_z(40, d), lab, 3))):
            with _refused(rf"{fn.__name__}: tile_k = {most + 1} is outside 1 \.\.\. {most}, the centroids of d = {d} columns"):
                fn(*args, tile_k=most + 1)
            with _refused(rf"{fn.__name__}: tile_k = -1 is outside"):
                fn(*args, tile_k=-1)
    assert ops.kmeans_tiled_shape_ok(1024, 3) and not ops.kmeans_tiled_shape_ok(1025, 3) and ops.kmeans_tile_centroids(1025) == 0
    with _refused(r"kmeans_assign_tiled: k = 3, d = 1025: need 1 <= d <= 1024"):
        ops.kmeans_assign_tiled(_z(40, 1025), _z(3, 1025))
    with _refused(r"kmeans_accumulate_tiled: k = 3, d = 1025: need 1 <= d <= 1024"):
        ops.kmeans_accumulate_tiled(_z(40, 1025), lab, 3)


def test_confusion_segments_refuses_beyond_its_domain():
    from timetuning_amd import _lib, hip_ops as ops

    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    z16, z64 = _z(2, 8, dtype=torch.int16), _z(2, 8, dtype=torch.int64)
    for Cg, Cp in ((4097, 3), (3, 4097)):
        with _refused(rf"confusion_counts_segments: Cg = {Cg}, Cp = {Cp}: need 1 <= Cg, Cp <= 4096"):
            ops.confusion_counts_segments(z16, z64, Cg, Cp)
    # S * Cg * Cp cells beyond 2^32 (257 matrices of 4096 x 4096), through the C entry: the counts are never touched, so a small buffer serves
    S = 257
    p1, g1, counts = _z(S, 1, dtype=torch.int64), _z(S, 1, dtype=torch.int64), torch.full((16,), 7, dtype=torch.int64, device="cuda")
    with _refused(r"confusion_counts_segments: S = 257 matrices of 4096 x 4096 are 4311744512 cells, more than the 4294967296"):
        _lib.check(lib.tt_confusion_counts_segments(p1.data_ptr(), 1, g1.data_ptr(), S, 1, 4096, 4096, 0, 0, counts.data_ptr(), st), "tt_confusion_counts_segments")
    # a pred pointer off its element size (one byte into int16 labels; four bytes into int64 labels) and a gt pointer off 8 bytes
    for pred, code, off, size in ((z16, 0, 1, 2), (z64, 1, 4, 8)):
        with _refused(rf"confusion_counts_segments: pred \(.*\) must be aligned to its {size}-byte elements"):
            _lib.check(lib.tt_confusion_counts_segments(pred.data_ptr() + off, code, z64.data_ptr(), 1, 4, 3, 3, 0, 0, counts.data_ptr(), st), "tt_confusion_counts_segments")
    with _refused(r"confusion_counts_segments: pred \(.*\) must be aligned to its 2-byte elements and gt \(.*\) to 8 bytes"):
        _lib.check(lib.tt_confusion_counts_segments(z16.data_ptr(), 0, z64.data_ptr() + 4, 1, 4, 3, 3, 0, 0, counts.data_ptr(), st), "tt_confusion_counts_segments")
    with _refused(r"confusion_counts_segments: Cg = 0, Cp = 3: need 1 <= Cg, Cp <= 4096"):
        _lib.check(lib.tt_confusion_counts_segments(z16.data_ptr(), 0, z64.data_ptr(), 1, 4, 0, 3, 0, 0, counts.data_ptr(), st), "tt_confusion_counts_segments")
    with _refused(r"confusion_counts_segments: S = 0 segments of n = 4 elements"):
        _lib.check(lib.tt_confusion_counts_segments(z16.data_ptr(), 0, z64.data_ptr(), 0, 4, 3, 3, 0, 0, counts.data_ptr(), st), "tt_confusion_counts_segments")
    torch.cuda.synchronize()
    assert bool((counts == 7).all())                                              # nothing was launched, nothing cleared


# ---- the accepted domain of the linear probe's entries, at the edge (include/timetuning_hip.h, N5; linear_probe.hip: probe_shape_error,
# probe_grid_error).  The largest accepted size computes correctly - here or as a case of the table above - and the first one beyond is
# refused by the launcher's own message: every refusal is a host-side TT_REQUIRE ahead of the first launch.
def _probe_ce_raw(B, g, Cc, R, ws_bytes=None):
    """tt_probe_upsample_ce on zero logits and labels 0, through the C entry: -> (rc, loss, dlow, counts)"""
    from timetuning_amd import _lib

    lib = _lib.load()
    low, y = _z(B, g * g, Cc), _z(B, R, R, dtype=torch.int64)
    dlow, loss, counts = torch.full_like(low, 7.0), _z(1), _z(2, dtype=torch.int64)
    nb = lib.tt_probe_upsample_ce_workspace_bytes(B, g) if ws_bytes is None else ws_bytes
    ws = _z(max(nb, 8), dtype=torch.uint8)
    rc = lib.tt_probe_upsample_ce(low.data_ptr(), y.data_ptr(), dlow.data_ptr(), loss.data_ptr(), counts.data_ptr(), B, g, Cc, R, ws.data_ptr(), nb,
                                  torch.cuda.current_stream().cuda_stream)
    return rc, loss, dlow, counts


@pytest.mark.parametrize("what,ok,bad,msg", [("g", 64, 65, r"need 1 <= g <= 64 \(got 65\)"), ("R", 1024, 1025, r"need 1 <= R <= 1024 \(got 1025\)"),
                                             ("C", 256, 257, r"need 1 <= classes <= 256 \(got 257\)"),
                                             ("B", 65535, 65536, r"need 1 <= B <= 65535 \(got 65536\)")])
def test_probe_grid_entries_at_the_edge(what, ok, bad, msg):
    """g, R, C and B of tt_probe_upsample_ce and tt_bilinear_adjoint_tokens.  Equal logits under labels 0 give loss = log C and, summed over
    the tokens, the gradient 1 / C - [c == 0] per class (the bilinear weights of every mask pixel sum to 1); a mask of ones gives the
    adjoint R * R per image and class - B = 65535 at g = R = C = 1 included."""
    from timetuning_amd import _lib, hip_ops as ops

    def dims(v):
        d = dict(g=dict(B=1, g=64, C=3, R=4), R=dict(B=1, g=64, C=2, R=1024), C=dict(B=1, g=2, C=256, R=4), B=dict(B=65535, g=1, C=1, R=1))[what]
        d[what] = v
        return d["B"], d["g"], d["C"], d["R"]

    B, g, Cc, R = dims(ok)
    rc, loss, dlow, counts = _probe_ce_raw(B, g, Cc, R)
    assert rc == 0 and counts.tolist() == [B * R * R, 0]
    assert abs(loss.item() - np.log(Cc)) <= 1e-5 * max(np.log(Cc), 1.0)
    want = torch.full((Cc,), 1.0 / Cc, dtype=torch.float64)
    want[0] -= 1.0
    assert float((dlow.double().sum((0, 1)).cpu() - want).abs().max()) <= 1e-5 * max(float(want.abs().max()), 1.0 / Cc)
    d_low = ops.bilinear_adjoint_tokens(torch.ones(B, R * R, Cc, device="cuda"), g)
    assert rel_err(d_low.double().sum(1), torch.full((B, Cc), float(R * R), dtype=torch.float64)) < 1e-6
    if R % g == 0:      # whole ratios: every token is read with a total weight of (R / g)^2, border tokens included
        assert rel_err(d_low, torch.full((B, g * g, Cc), (R / g) ** 2)) < 1e-6
    B, g, Cc, R = dims(bad)
    with _refused("linear probe: " + msg):
        _lib.check(_probe_ce_raw(B, g, Cc, R)[0], "tt_probe_upsample_ce")
    with _refused("linear probe: " + msg):
        ops.bilinear_adjoint_tokens(_z(B, R * R, Cc), g)


def test_probe_matrix_entries_at_the_edge():
    from timetuning_amd import _lib, hip_ops as ops

    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    # D = 1024 and C = 256 compute (cases above); D = 1028, D = 6 and C = 257 are refused by both matrix entries
    for D, Cc, msg in ((1028, 4, r"need D % 4 == 0 and 0 < D <= 1024 \(got 1028\)"), (6, 4, r"need D % 4 == 0 and 0 < D <= 1024 \(got 6\)"),
                       (8, 257, r"need 1 <= classes <= 256 \(got 257\)")):
        with _refused("linear probe: " + msg):
            ops.probe_logits(_z(3, D), _z(Cc, D))
        with _refused("linear probe: " + msg):
            ops.probe_wgrad(_z(3, Cc), _z(3, D))
    x = torch.ones(5, 1024, device="cuda")
    assert torch.equal(ops.probe_logits(x, torch.ones(256, 1024, device="cuda")), torch.full((5, 256), 1024.0, device="cuda"))
    dw, db = ops.probe_wgrad(torch.ones(5, 256, device="cuda"), x)
    assert torch.equal(dw, torch.full((256, 1024), 5.0, device="cuda")) and torch.equal(db, torch.full((256,), 5.0, device="cuda"))
    # feats one float off a 16-byte boundary
    off = _z(3 * 8 + 4)[1:25].view(3, 8)
    assert off.data_ptr() % 16 == 4
    with _refused("probe_logits: feats and weight must be 16-byte aligned"):
        ops.probe_logits(off, _z(2, 8))
    with _refused("probe_wgrad: feats and workspace must be 16-byte aligned"):
        ops.probe_wgrad(_z(3, 2), off)
    # a workspace one byte short
    dl, xs, dws = _z(100, 4), _z(100, 8), _z(4, 8)
    nb = lib.tt_probe_wgrad_workspace_bytes(100, 8, 4)
    ws = _z(nb, dtype=torch.uint8)
    assert nb > 0 and lib.tt_probe_wgrad(dl.data_ptr(), xs.data_ptr(), None, dws.data_ptr(), None, 100, 8, 4, ws.data_ptr(), nb, st) == 0
    with _refused("probe_wgrad: workspace too small"):
        _lib.check(lib.tt_probe_wgrad(dl.data_ptr(), xs.data_ptr(), None, dws.data_ptr(), None, 100, 8, 4, ws.data_ptr(), nb - 1, st), "tt_probe_wgrad")
    with _refused("probe_upsample_ce: workspace too small"):
        _lib.check(_probe_ce_raw(2, 3, 4, 5, ws_bytes=lib.tt_probe_upsample_ce_workspace_bytes(2, 3) - 1)[0], "tt_probe_upsample_ce")
    # TT_MAX_TENSORS = 40 per table: 40 update every tensor, 41 in one call are refused at the C entry
    ps = [torch.ones(4, device="cuda") for _ in range(41)]
    grad = torch.ones(4, device="cuda")
    tab = (_lib.AdamwTensor * 41)()
    for j, q in enumerate(ps):
        tab[j] = _lib.AdamwTensor(q.data_ptr(), grad.data_ptr(), None, None, 4, 0.5, 0.0)
    with _refused(r"sgd_step: need 1\.\.40 tensors"):
        _lib.check(lib.tt_sgd_step(tab, 41, 0.0, 1, st), "tt_sgd_step")
    assert all(torch.equal(q, torch.ones(4, device="cuda")) for q in ps)             # nothing was launched
    _lib.check(lib.tt_sgd_step(tab, 40, 0.0, 1, st), "tt_sgd_step")
    assert all(torch.equal(q, torch.full((4,), 0.5, device="cuda")) for q in ps[:40]) and torch.equal(ps[40], torch.ones(4, device="cuda"))
    with _refused("sgd_step: tensor 0 has no momentum buffer"):
        _lib.check(lib.tt_sgd_step(tab, 1, 0.9, 1, st), "tt_sgd_step")


# ---- the accepted domain of the propagation entries, at the edge (include/timetuning_hip.h, k14 and N9).  Every refusal below is a host-side
# TT_REQUIRE ahead of the first launch (label_prop.hip: lp_run, tt_label_propagate_grid_maps, tt_upsample_argmax_hw); no shape beyond the
# domain is ever launched.  4096 candidates (correct) against 5120 (refused) are cases of the table above.
def _one_patch(bs, fs, K, seed=11):
    """g = 1: every context is the one patch, so every map is the seed - exactly at fs 2 (one kept source of weight 1)."""
    gen = torch.Generator().manual_seed(seed)
    xn = F.normalize(torch.randn(fs, bs, 1, 16, generator=gen), dim=-1).cuda()
    s0 = torch.softmax(2 * torch.randn(bs, 1, K, generator=gen), -1).cuda()
    return xn, s0


def test_label_prop_square_entries_refuse_beyond_their_domain():
    from timetuning_amd import hip_ops as ops

    xn, s0 = _one_patch(2, 10, 3)
    x49 = F.normalize(torch.randn(10, 2, 49, 16, generator=torch.Generator().manual_seed(1)), dim=-1).cuda()
    s49 = torch.softmax(torch.randn(2, 49, 3, generator=torch.Generator().manual_seed(2)), -1).cuda()
    # n_last_frames 7 is the most (cases above run it); 8 is refused
    ops.label_propagate_maps(x49, s49, 7, 2, 5, 0.1)
    for fn in (ops.label_propagate_maps, ops.label_propagate):
        with _refused(r"n_last_frames must be <= 7"):
            fn(x49, s49, 8, 2, 5, 0.1)
        with _refused(r"size_mask_neighborhood must be > 0"):          # the unrestricted variant is the grid entry's
            fn(x49, s49, 4, 0, 5, 0.1)
        with _refused(r"feature dim must be a multiple of 4"):           # D = 4 runs in the table; 6 is refused
            fn(x49[..., :6].contiguous(), s49, 4, 2, 5, 0.1)
        with _refused(r"topk >= 1"):
            fn(x49, s49, 4, 2, 0, 0.1)
    with _refused(r"label_propagate_sims: n_last_frames must be <= 7"):
        ops.label_propagate_sims(x49, 3, 8)
    assert ops._lib.load().tt_label_propagate_route(10, 7, 3, 8, 2, 1) == 0 and ops._lib.load().tt_label_propagate_route(10, 7, 3, 4, 0, 1) == 0


@pytest.mark.parametrize("K,route,msg", [(513, 5, "65536 clips exceed the 65535 of one launch of the workgroup-per-query kernel"),
                                         (3, 1, "65536 clips exceed the 65535 problems of one similarity launch")])
def test_label_prop_takes_65535_clips_and_refuses_more(K, route, msg):
    """Clips ride on gridDim.y of the workgroup-per-query kernels (K = 513 puts g = 1 there) and, on every route, of the similarity
    product: 65535 one-patch clips propagate correctly, 65536 are refused by lp_run before anything is launched."""
    from timetuning_amd import hip_ops as ops

    assert ops._lib.load().tt_label_propagate_route(2, 1, K, 0, 1, 1) == route
    xn, s0 = _one_patch(65535, 2, K)
    maps = ops.label_propagate_maps(xn, s0, 0, 1, 5, 0.1)
    assert torch.equal(maps[0], s0.double())
    labels, pmap = ops.label_propagate(xn, s0, 0, 1, 5, 0.1, return_pmap=True)
    assert torch.equal(pmap, maps[0]) and torch.equal(labels, s0.argmax(-1))
    xn, s0 = _one_patch(65536, 2, K)
    with _refused(msg):
        ops.label_propagate_maps(xn, s0, 0, 1, 5, 0.1)
    with _refused(msg):
        ops.label_propagate(xn, s0, 0, 1, 5, 0.1)


def test_label_prop_shortens_the_chunk_to_the_similarity_launch():
    """40 000 clips x 2 target frames are 80 000 problems of the slot-0 similarity product, more than one launch carries on gridDim.y: the
    chunk is shortened to one frame (lp_chunk) and the call runs - the maps of one-patch clips are convex combinations of the seed with
    itself.  The two-call form, which needs one chunk, declines."""
    from _sweep_cases import lp_chunk
    from timetuning_amd import hip_ops as ops

    assert lp_chunk(40000, 3, 1, 1) == 1 and lp_chunk(30000, 3, 1, 1) == 2
    xn, s0 = _one_patch(40000, 3, 3)
    maps = ops.label_propagate_maps(xn, s0, 1, 1, 5, 0.1)
    assert torch.equal(maps[0], s0.double()) and rel_err(maps[1], s0.double()) < 1e-6
    assert ops.label_propagate_sims(xn, 3, 1) is None
    gm = ops.label_propagate_grid_maps(xn, s0, (1, 1), 1, 1, 5, 0.1)
    assert torch.equal(gm[0], s0.double()) and rel_err(gm[1], s0.double()) < 1e-6


def test_grid_entry_and_its_upsampler_at_the_edge():
    from timetuning_amd import hip_ops as ops

    xn, s0 = _one_patch(65535, 2, 3)
    assert torch.equal(ops.label_propagate_grid_maps(xn, s0, (1, 1), 0, 0, 5, 0.1)[0], s0.double())
    xn, s0 = _one_patch(65536, 2, 3)
    with _refused("label_propagate_grid_maps: need fs >= 2 and positive sizes"):
        ops.label_propagate_grid_maps(xn, s0, (1, 1), 0, 0, 5, 0.1)
    xn, s0 = _one_patch(2, 10, 3)
    ops.label_propagate_grid_maps(xn, s0, (1, 1), 7, 0, 5, 0.1)
    with _refused("label_propagate_grid_maps: n_last_frames must be <= 7"):
        ops.label_propagate_grid_maps(xn, s0, (1, 1), 8, 0, 5, 0.1)
    with _refused(r"label_propagate_grid_maps: size_mask_neighborhood must be >= 0"):
        ops.label_propagate_grid_maps(xn, s0, (1, 1), 4, -1, 5, 0.1)
    with _refused("label_propagate_grid_maps: feature dim must be a multiple of 4"):
        ops.label_propagate_grid_maps(xn[..., :6].contiguous(), s0, (1, 1), 4, 1, 5, 0.1)
    # M rides on gridDim.y: 65535 maps (1 x 1 each, to 2 x 2) are each resampled, 65536 are refused
    x = torch.randn(65535, 1, 3, generator=torch.Generator().manual_seed(5)).double().cuda()
    assert torch.equal(ops.upsample_argmax_hw(x, (1, 1), (2, 2)), x.argmax(-1).view(-1, 1, 1).expand(65535, 2, 2))
    with _refused("upsample_argmax_hw: 65536 maps of 2x2 exceed one launch"):
        ops.upsample_argmax_hw(_z(65536, 1, 3, dtype=torch.float64), (1, 1), (2, 2))


# ---- the sixth tier's entries at the edge of their domains (include/timetuning_hip.h).  The last accepted values are cases of the sweep
# (Rpad = ceil32(R) with Rpad % 64 == 32, C = 32, n = 32 and 8, D = 1024, workspaces of exactly the size the queries return); the first
# value beyond is refused with the launcher's own message before anything is launched: every output still holds its prefill.
_EDGES = []


def _edges():
    if not _EDGES:
        _EDGES.extend(domain_edges(PrepHip()))
    return _EDGES


@pytest.mark.parametrize("i", range(27))
def test_preparation_entries_refuse_the_first_value_beyond_their_domain(i):
    edges = _edges()
    assert len(edges) == 27
    assert_refused(PrepHip(), *edges[i])


def test_the_last_accepted_values_are_cases_of_the_sweep():
    have = {case_id(o, p) for o, p in CASES}
    for cid in ("split_dual[R=33,C=32,rpad=0,t=1,row=1,colsum=fold,scale=,mag=1.0,vals=normal,off=0,sr=1]", "transpose_pairs[R=33,C=32,rpad=0]",
                "convert[what=pairs,P=0,n=32,vals=normal]", "convert[what=planes,P=1,n=8,vals=normal]",
                "grad_amax[producer=ln_bwd,rows=5,D=1024,N=0,gscale=1.0,accum=1,off=0]", "transpose_planes[R=63,C=64,rpad=R,colsum=0]"):
        assert cid in have, cid


def test_layernorm_bwd_refuses_a_maximum_with_drop_and_accumulate():
    ln_refuses_amax_with_drop_and_accum(PrepHip())
