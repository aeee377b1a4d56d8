"""The sweep's third tier on the CPU: every label-propagation case of the seeded table (tests/_sweep_cases.py, PROP_OPS) runs on the plain-C
twins (oracle/tt_cpu.c) against the one-frame fp64 reference, with the assertions the GPU half (tests/test_hip_sweep.py) makes on the HIP
library - tests/_sweep_checks_prop.py holds them once for both.  This proves the reference, the two input families, the one-frame bound and
both excuse caps (at most 0.5 % of a case's queries marked excusable by the reference alone) before a GPU is involved.
TT_SWEEP_REPORT_HOST=<path> writes the worst error per quantity and its bound (one file with the second tier's, when both halves run)."""
import json
import os

import pytest

from _sweep_cases import PROP_OPS, case_id, table
from _sweep_checks_eval import HOST_WORST as WORST
from _sweep_checks_prop import prop_twin, run_prop_case

CASES = [(o, p) for o, p in table() if o in PROP_OPS]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("TT_SWEEP_REPORT_HOST")
    if path:
        with open(path, "w") as f:
            json.dump(WORST, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("op,params", CASES, ids=[case_id(o, p) for o, p in CASES])
def test_sweep_prop_on_the_twin(op, params):
    run_prop_case(prop_twin(), op, params, WORST)
