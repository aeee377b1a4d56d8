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
    return dict(B=B, K=K, iters=_ch(rng, (0, 1, 3, 10)), row0=row0, rows_out=rows_out, persist=_b(rng))


def _sinkhorn_from_q(rng):
    return dict(B=int(rng.integers(1, 5000)), K=int(rng.integers(1, 513)), iters=_ch(rng, (0, 1, 3, 10)), transposed=_b(rng))


def _sinkhorn_local(rng):
    return dict(B=int(rng.integers(1, 5000)), K=int(rng.integers(1, 513)), iters=_ch(rng, (0, 1, 3, 10)))


def _queue_push(rng):
    Q = int(rng.integers(1, 300))
    return dict(Q=Q, D=_ch(rng, (1, 32, 128, 256)), m=int(rng.integers(1, Q + 1)))


DRAW = {"linear_f32": _linear_f32, "linear_pairs": _linear_pairs, "linear_planes": _linear_planes, "bwd_pairs": _bwd_pairs,
        "layernorm": _layernorm, "l2norm": _l2norm, "attention": _attention, "ce": _ce, "sinkhorn": _sinkhorn,
        "sinkhorn_from_q": _sinkhorn_from_q, "sinkhorn_local": _sinkhorn_local, "queue_push": _queue_push}
OPS = tuple(DRAW)

COUNTS = {"linear_f32": 6, "linear_pairs": 8, "linear_planes": 4, "bwd_pairs": 6, "layernorm": 5, "l2norm": 3, "attention": 6, "ce": 3,
          "sinkhorn": 6, "sinkhorn_from_q": 3, "sinkhorn_local": 3, "queue_push": 3}

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
        # the launch-per-iteration kernels: KPL 4 / 8 either side of K = 256; workgroup counts below the cap, AT it (2048 rows: 64 of 64),
        # beyond it (2049: 64 workgroups of 33 rows - the last one gets none), 50176 rows (the cap of 256)
        dict(B=2048, K=256, iters=3, row0=0, rows_out=2048, persist=0), dict(B=2049, K=257, iters=1, row0=100, rows_out=1500, persist=0),
        dict(B=1, K=1, iters=0, row0=0, rows_out=1, persist=0), dict(B=50176, K=200, iters=2, row0=6272, rows_out=6272, persist=0),
        # the one-launch solve: odd B * K (777 x 333: 9 workgroups; 1001 x 255), KPL 4 and 8, iters 0 and 1, row windows, one workgroup,
        # and a problem too big for it (it falls back)
        dict(B=777, K=333, iters=5, row0=0, rows_out=777, persist=1), dict(B=1001, K=255, iters=1, row0=3, rows_out=997, persist=1),
        dict(B=6272, K=200, iters=0, row0=2000, rows_out=99, persist=1), dict(B=33, K=511, iters=10, row0=0, rows_out=33, persist=1),
        dict(B=1705, K=1, iters=3, row0=0, rows_out=1705, persist=1), dict(B=50176, K=200, iters=2, row0=0, rows_out=50176, persist=1),
    ],
    "sinkhorn_from_q": [dict(B=777, K=333, iters=5, transposed=0), dict(B=2049, K=256, iters=0, transposed=1), dict(B=65, K=511, iters=1, transposed=1)],
    "sinkhorn_local": [dict(B=777, K=333, iters=5), dict(B=2049, K=257, iters=0), dict(B=31, K=64, iters=1)],
    "queue_push": [dict(Q=40, D=32, m=1), dict(Q=40, D=32, m=40), dict(Q=1, D=128, m=1)],
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
