#!/usr/bin/env python
"""Writes tests/golden/jpeg_entropy.npz: five JPEG files encoded by Pillow that stress the N24 entropy decode where the files of
jpeg_frames.npz do not (tests/test_jpeg_entropy_host.py, tests/test_hip_jpeg_entropy.py).  JPEG bytes only - the yardstick is the host scan
of the same bytes.  Needs Pillow; the tests that read the fixture do not.

  names        the cases, in order
  blob, offs   the files' bytes, concatenated: case i is blob[offs[i]:offs[i + 1]]

  noise_96x136_444_q100      more than 256 subsequences of 1024 bits (two tiles), long codes, dense FF 00 stuffing
  noise_96x136_420_q100_opt  the same content, 4:2:0, optimised tables
  flat_200x264_420_q30       hundreds of blocks inside one subsequence
  rst1_40x56_422_q90         a restart interval of one MCU: a segment per lane
  rst7_40x56_422_q90         an interval of 7 MCUs, which does not divide the MCU row of 4
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_jpeg_golden import REPO, encode, picture  # noqa: E402


def main():
    noise = np.random.default_rng(2401).integers(0, 256, (96, 136, 3), dtype=np.uint8)
    flat = np.full((200, 264, 3), (93, 141, 60), np.uint8)
    small = picture(40, 56, 2402, noise=3.0)
    cases = [("noise_96x136_444_q100", encode(noise, quality=100, subsampling=0)),
             ("noise_96x136_420_q100_opt", encode(noise, quality=100, subsampling=2, optimize=True)),
             ("flat_200x264_420_q30", encode(flat, quality=30, subsampling=2)),
             ("rst1_40x56_422_q90", encode(small, quality=90, subsampling=1, restart_marker_blocks=1)),
             ("rst7_40x56_422_q90", encode(small, quality=90, subsampling=1, restart_marker_blocks=7))]
    blob = np.frombuffer(b"".join(d for _, d in cases), np.uint8)
    offs = np.cumsum([0] + [len(d) for _, d in cases]).astype(np.int64)
    out = os.path.join(REPO, "tests", "golden", "jpeg_entropy.npz")
    np.savez_compressed(out, names=np.array([n for n, _ in cases]), blob=blob, offs=offs)
    size = os.path.getsize(out)
    print(f"{out}: {[(n, len(d)) for n, d in cases]}, {size} bytes")
    assert size < 100 * 1024, "the fixture must stay under 100 KB"
    return 0


if __name__ == "__main__":
    sys.exit(main())
