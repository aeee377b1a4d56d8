"""The sweep's second tier on the CPU: every case of the evaluator / optimizer / mask ops of the seeded table (tests/_sweep_cases.py, EVAL_OPS)
runs on the plain-C twins (oracle/tt_cpu.c) against the fp64 references, with the assertions the GPU half (tests/test_hip_sweep.py) makes on
the HIP library - tests/_sweep_checks_eval.py holds them once for both.  This proves the references, the generators and the capped excuse
rules without a GPU, and it is the measurement the regime-dependent bounds are taken from.  TT_SWEEP_REPORT_HOST=<path> writes the worst error
per quantity and its bound."""
import json
import os

import pytest

from _sweep_cases import EVAL_OPS, case_id, table
from _sweep_checks_eval import HOST_WORST as WORST, run_eval_case, twin_side

CASES = [(o, p) for o, p in table() if o in EVAL_OPS]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("TT_SWEEP_REPORT_HOST")
    if path:
        with open(path, "w") as f:
            json.dump(WORST, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("op,params", CASES, ids=[case_id(o, p) for o, p in CASES])
def test_sweep_eval_on_the_twin(op, params):
    run_eval_case(twin_side(), op, params, WORST)
