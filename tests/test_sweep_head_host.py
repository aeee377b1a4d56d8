"""The sweep's fourth tier on the CPU: every case of the linear-probe and clip-pipeline ops of the seeded table (tests/_sweep_cases.py,
HEAD_OPS) runs on the plain-C twins (oracle/tt_cpu.c) against the fp64 references and the Pillow-pinned image oracle, with the assertions
the GPU half (tests/test_hip_sweep.py) makes on the HIP library - tests/_sweep_checks_head.py holds them once for both.  Here the explicit
cross-entropy reference is also proved against torch autograd, and the twins' own refusals are held to the header's domain.
TT_SWEEP_REPORT_HOST=<path> writes the worst error per quantity and its bound."""
import json
import os

import numpy as np
import pytest

from _sweep_cases import HEAD_OPS, case_id, table
from _sweep_checks_eval import HOST_WORST as WORST
from _sweep_checks_head import head_twin, run_head_case

CASES = [(o, p) for o, p in table() if o in HEAD_OPS]
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("TT_SWEEP_REPORT_HOST")
    if path:
        with open(path, "w") as f:
            json.dump(WORST, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("op,params", CASES, ids=[case_id(o, p) for o, p in CASES])
def test_sweep_head_on_the_twin(op, params):
    run_head_case(head_twin(), op, params, WORST)


def test_twins_refuse_what_the_header_refuses():
    """include/timetuning_hip.h, N5: g <= 64, R <= 1024, 1 <= C <= 256, D % 4 == 0 and D <= 1024, B <= 65535, at most 40 tensors, feats on
    a 16-byte boundary - the largest accepted value runs (rc 0), the first one beyond is TT_EINVAL (-1)."""
    tw = head_twin()
    z = lambda *s, dt=f32: np.zeros(s, dt)

    def ce(B, g, Cc, R):
        return tw.call("probe_upsample_ce", z(B, g * g, Cc), np.full((B, R, R), 255, np.int64), z(B, g * g, Cc), z(1), z(2, dt=np.int64), B, g, Cc, R, None, 0, None)

    def adj(B, g, Cc, R):
        return tw.call("bilinear_adjoint_tokens", z(B, R * R, Cc), z(B, g * g, Cc), B, g, Cc, R, None)

    for fn in (ce, adj):
        assert fn(1, 64, 1, 2) == 0 and fn(1, 65, 1, 2) == -1
        assert fn(1, 2, 1, 1024) == 0 and fn(1, 2, 1, 1025) == -1
        assert fn(1, 2, 256, 2) == 0 and fn(1, 2, 257, 2) == -1 and fn(1, 2, 0, 2) == -1
        assert fn(65535, 1, 1, 1) == 0 and fn(65536, 1, 1, 1) == -1

    def logits(D, Cc, x=None):
        x = z(3, D) if x is None else x
        return tw.call("probe_logits", x, z(Cc, D), None, z(3, Cc), 3, D, Cc, None)

    def wgrad(D, Cc, x=None):
        x = z(3, D) if x is None else x
        return tw.call("probe_wgrad", z(3, Cc), x, None, z(Cc, D), None, 3, D, Cc, None, 0, None)

    for fn in (logits, wgrad):
        assert fn(1024, 256) == 0 and fn(1028, 256) == -1 and fn(6, 256) == -1 and fn(1024, 257) == -1
        off = np.zeros(3 * 8 + 4, f32)
        base = off[(-(off.ctypes.data // 4) % 4):]          # a 16-byte boundary inside the buffer, then one float past it
        assert base.ctypes.data % 16 == 0 and fn(8, 2, base[:24].reshape(3, 8)) == 0 and fn(8, 2, base[1:25].reshape(3, 8)) == -1
    one = z(4)
    tab = (tw._lib.AdamwTensor * 41)()
    for j in range(41):
        tab[j] = tw._lib.AdamwTensor(one.ctypes.data, one.ctypes.data, one.ctypes.data, None, 4, 0.0, 0.0)
    assert tw.call("sgd_step", tab, 40, 0.9, 1, None) == 0 and tw.call("sgd_step", tab, 41, 0.9, 1, None) == -1
    assert tw.call("sgd_step", tab, 0, 0.9, 1, None) == -1
    tab[0].m = None
    assert tw.call("sgd_step", tab, 1, 0.9, 1, None) == -1 and tw.call("sgd_step", tab, 1, 0.0, 1, None) == 0
