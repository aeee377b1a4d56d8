"""Writes tests/golden/fcn_head_bn.npz: an FCN head with norm layers (norm_cfg BN) on the N32 fixture's features, labels and dropout
multipliers: its state dict, loss, logits, every parameter gradient and the running statistics after the forward, from the fp64
restatement tests/_fcn_bn_ref.py, stored as fp32 (B = 2, g = 4, D = 16, channels = 8, C = 5, R = 9).

    python tools/gen_fcn_bn_golden.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import _fcn_bn_ref  # noqa: E402


def main():
    path = os.path.join(REPO, "tests", "golden", "fcn_head_bn.npz")
    np.savez_compressed(path, **_fcn_bn_ref.fixture_arrays())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
