"""GPU check of N30: every kernel that takes its taps or weights from csrc/interp.hpp gives, bit for bit, what the library gave before
the rules were gathered there (tests/golden/interp_bits.npz, written by tools/gen_interp_golden.py from the parent commit's library).
The inputs are the tool's: seeded, not stored."""
import importlib.util
import os

import pytest
import torch

from timetuning_amd import hip_ops as ops

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def results():
    spec = importlib.util.spec_from_file_location("gen_interp_golden", os.path.join(REPO, "tools", "gen_interp_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool, tool.compute(ops)


def test_every_result_equals_the_recorded_bits(results, golden):
    _, got = results
    want = golden("interp_bits")
    assert sorted(got) == sorted(want.files)
    assert len(got) == 52
    for key in want.files:
        a, b = torch.from_numpy(got[key]), torch.from_numpy(want[key])
        assert a.dtype == b.dtype and torch.equal(a, b), key


def test_histogram_counts_the_label_kernels_labels(results):
    """The histogram kernel and the label kernel call one statement: the counts are the bincount of the labels, ties and all."""
    tool, got = results
    for M, g, R, K in tool.ARGMAX32:
        for kind in tool.KINDS:
            key = f"argmax32/{M}_{g}_{R}_{K}/{kind}"
            want = torch.bincount(torch.from_numpy(got[key]).long().flatten(), minlength=K)
            assert torch.equal(torch.from_numpy(got[key + "/hist"]), want), key
            start = torch.arange(1, K + 1) * 1000003
            assert torch.equal(torch.from_numpy(got[key + "/hist_added"]), want + start), key
        assert int(torch.from_numpy(got[f"argmax32/{M}_{g}_{R}_{K}/const"]).abs().sum()) == 0      # all channels equal: the first wins
