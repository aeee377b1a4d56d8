"""The sweep's sixth tier on the CPU: every case of the operand-preparation ops and the producers' maxima of the seeded table
(tests/_sweep_cases.py, PREP_OPS) runs on the host side of tests/_sweep_checks_prep.py - the plain-C twins of oracle/tt_cpu.c behind the
library's own prototypes - with the assertions the GPU half (tests/test_hip_sweep.py) makes on the HIP library.  This proves the NumPy
restatements of the pair and plane formats, the guard-band harness, the fp64 references and the generators, holds the twins to the same
bits as the kernels, and is the measurement the long-run bound of the column sums is taken from.  TT_SWEEP_REPORT_HOST=<path> writes the
worst error per quantity and its bound."""
import json
import os

import numpy as np
import pytest

from _sweep_cases import PREP_OPS, case_id, draw, prep_case_on_twin, table
from _sweep_checks_eval import HOST_WORST as WORST
from _sweep_checks_prep import (FILL16, GUARD, Out, bf16_bits, colsum_fold, ln_refuses_amax_with_drop_and_accum, pair_bits, pair_join, pair_layout,
                                pair_scale, prep_twin, run_prep_case)

CASES = [(o, p) for o, p in table() if o in PREP_OPS and prep_case_on_twin(o, p)]      # (the twin's products are naive loops)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("TT_SWEEP_REPORT_HOST")
    if path:
        with open(path, "w") as f:
            json.dump(WORST, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("op,params", CASES, ids=[case_id(o, p) for o, p in CASES])
def test_sweep_prep_on_the_host_side(op, params):
    run_prep_case(prep_twin(), op, params, WORST)


def test_the_restatements_on_values_worked_out_by_hand():
    """The restatements are the reference of every exact comparison, so they are held to values that follow from the formats' definitions."""
    v = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -10 + 2.0 ** -20, 65504.0, 65519.9, 65520.0, 2.0 ** -24, 2.0 ** -25, -0.0, 3e-8], np.float32)
    hi, lo = pair_bits(v)
    # 1 + 2^-11 is a tie: to even, hi = 1 and lo = 2^-11 * 2048 = 1; 65519.9 rounds to 65504 (lo: 15.9 * 2048, beyond fp16 - an infinity),
    # 65520 is the tie that rounds to infinity; 2^-25 is the tie that rounds to zero
    assert list(hi[:9]) == [0x3C00, 0x3C00, 0x3C01, 0x7BFF, 0x7BFF, 0x7C00, 0x0001, 0x0000, 0x8000]
    assert list(lo[:4]) == [0x0000, 0x3C00, np.float16(2.0 ** -9).view(np.uint16), 0x0000] and lo[7] == np.float16(2.0 ** -14).view(np.uint16)
    lay = pair_layout(np.arange(64, dtype=np.float32).reshape(1, 64))
    assert lay.shape == (1, 128) and (lay[0, :32].view(np.float16) == np.arange(32)).all() and (lay[0, 64:96].view(np.float16) == np.arange(32, 64)).all()
    assert (lay[0, 32:64] == 0).all()
    x = np.random.default_rng(1).standard_normal((3, 96)).astype(np.float32)
    assert np.abs(pair_join(pair_layout(x)).astype(np.float64) - x).max() <= 2.0 ** -22 * np.abs(x).max()
    # bf16: 1 + 2^-8 is a tie (to even: 1), 1 + 2^-8 + 2^-23 rounds up, the largest finite fp32 rounds to infinity
    b = bf16_bits(np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 3 * 2.0 ** -8, 3.4028235e38, -2.5], np.float32))
    assert list(b) == [0x3F80, 0x3F80, 0x3F81, 0x3F82, 0x7F80, 0xC020]
    assert [pair_scale(a) for a in (0.0, np.inf, np.nan, 1.0, 8192.0, 16383.9, 16384.0, 7e4, 1e-30, 1e38)] == \
           [1.0, 1.0, 1.0, 8192.0, 1.0, 1.0, 0.5, 0.125, 2.0 ** 100, 2.0 ** -100]      # (both ends clamped: 2^113 and 2^-113 unclamped)
    parts = np.arange(1, 11, dtype=np.float32).reshape(10, 1)      # waves: 1 + 5 + 9, 2 + 6 + 10, 3 + 7, 4 + 8
    assert colsum_fold(parts)[0] == (15 + 18) + (10 + 12)


def test_the_guard_bands_notice_an_overrun_and_an_unwritten_element():
    side = prep_twin()
    o = Out(side, 100, "h")
    with pytest.raises(AssertionError, match="not written"):
        o.get()
    o.host()[GUARD:GUARD + 100] = 7
    assert (o.get() == 7).all()
    o.host()[GUARD + 100] = 7
    with pytest.raises(AssertionError, match="guard band"):
        o.get()
    assert FILL16 & 0x7C00 == 0x7C00 and FILL16 & 0x3FF and FILL16 & 0x7F80 == 0x7F80 and FILL16 & 0x7F      # a NaN as fp16 and as bf16


def test_layernorm_bwd_refuses_a_maximum_with_drop_and_accumulate():
    ln_refuses_amax_with_drop_and_accum(prep_twin())


# ---- the draws: tools/fuzz_ops.py runs one draw per op and round through the same checks and stops at the first AssertionError; every draw
# must therefore give inputs its check accepts.
DRAWS = {"convert": 20, "split_dual": 60, "split_multi": 10, "transpose_pairs": 40, "transpose_planes": 40, "patch_embed": 30, "grad_amax": 40, "layernorm_long": 20}


@pytest.mark.parametrize("op", PREP_OPS)
def test_every_draw_is_a_case_its_check_accepts(op):
    rng = np.random.default_rng(20261020)
    worst = {}
    for i in range(DRAWS[op]):
        case = draw(op, rng)
        if not prep_case_on_twin(op, case):
            continue
        try:
            run_prep_case(prep_twin(), op, case, worst)
        except AssertionError as e:
            raise AssertionError(f"draw {i}, {case_id(op, case)}: {e}") from None
