"""The sweep's fifth tier on the CPU: every case of the k-means family and the metric counters of the seeded table (tests/_sweep_cases.py,
METRIC_OPS) runs on the host side of tests/_sweep_checks_metric.py with the assertions the GPU half (tests/test_hip_sweep.py) makes on the HIP
library.  For the k-means ops that side is the plain-C twins (oracle/tt_cpu.c): this proves the fp64 references, the generators, the capped
excuse rule and - for every fit case - that the inputs are valid (no empty cluster, no near-tie in any fp64 iteration), and it is the
measurement the bound of the long fp32 runs is taken from.  For the three counters it is a direct per-pixel definition, which proves the
NumPy restatements the GPU half compares with.  TT_SWEEP_REPORT_HOST=<path> writes the worst error per quantity and its bound."""
import json
import os

import numpy as np
import pytest

from _sweep_cases import METRIC_OPS, case_id, draw, table
from _sweep_checks_eval import HOST_WORST as WORST
from _sweep_checks_metric import COLUMNS, COMPARED, SMALL_PIXELS, MetricTwin, run_metric_case

CASES = [(o, p) for o, p in table() if o in METRIC_OPS]
_SIDE = []


def _side():
    if not _SIDE:
        _SIDE.append(MetricTwin())
    return _SIDE[0]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("TT_SWEEP_REPORT_HOST")
    if path:
        with open(path, "w") as f:
            json.dump(WORST, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("op,params", CASES, ids=[case_id(o, p) for o, p in CASES])
def test_sweep_metric_on_the_host_side(op, params):
    run_metric_case(_side(), op, params, WORST)


def test_no_count_column_is_zero_everywhere_and_the_definitions_ran():
    """A restatement that returned zeros would pass an equality with a kernel that does the same: over each counter's cases every column of
    the expected counts is non-zero somewhere (the cases above record them; one that has not run yet runs here).  And the per-pixel
    definitions ran on several cases of each counter."""
    for op, width in (("confusion_segments", 3), ("davis_counts", 6), ("bf_counts", 4)):
        for o, p in CASES:
            if o == op and case_id(o, p) not in COLUMNS.get(op, {}):
                run_metric_case(_side(), o, p, WORST)
        cols = np.sum([COLUMNS[op][case_id(o, p)] for o, p in CASES if o == op], axis=0)
        assert cols.shape == (width,) and (cols > 0).all(), (op, cols)
    # the per-pixel definition RAN and was compared on every case of at most SMALL_PIXELS pixels (elements), and on no other
    small = {"confusion_segments": lambda p: p["S"] * p["n"] <= SMALL_PIXELS, "davis_counts": lambda p: p["H"] * p["W"] <= SMALL_PIXELS,
             "bf_counts": lambda p: p["H"] * p["W"] <= SMALL_PIXELS}
    for op, rule in small.items():
        ran = [COMPARED[op][case_id(o, p)] for o, p in CASES if o == op]
        assert ran == [rule(p) for o, p in CASES if o == op] and sum(ran) >= 5, op


# ---- the draws: tools/fuzz_ops.py runs one draw per op and round through the same checks and stops at the first AssertionError, so a draw
# the checks cannot accept - an input that is invalid whatever the kernels do - ends a fuzz run on a false alarm.  Every new op's generator
# is therefore run here on the host side: every draw must give inputs its check accepts.
DRAWS = {"kmeans_assign_tiled": 200, "kmeans_accumulate_tiled": 200, "kmeans_assign_batched": 200, "kmeans_fit": 200, "confusion_segments": 200,
         "davis_counts": 100, "bf_counts": 100}


@pytest.mark.parametrize("op", METRIC_OPS)
def test_every_draw_is_a_case_its_check_accepts(op):
    rng = np.random.default_rng(20261019)
    worst = {}
    for i in range(DRAWS[op]):
        case = draw(op, rng)
        try:
            run_metric_case(_side(), op, case, worst)
        except AssertionError as e:
            raise AssertionError(f"draw {i}, {case_id(op, case)}: {e}") from None
