#!/bin/bash
# Builds tools/jpeg_entropy_check.cpp + timetuning_amd/csrc/jpeg_scan.cpp (with csrc/jpeg_huff.hpp, the header the device kernels share)
# with AddressSanitizer and UBSan - host code only: no GPU, nothing loaded into Python - and runs it over the files of
# tests/golden/jpeg_frames.npz and tests/golden/jpeg_entropy.npz, written out to a temporary directory.
#   tools/jpeg_entropy_check.sh          (CXX=g++ by default)
set -euo pipefail
cd "$(dirname "$0")/.."
out=$(mktemp -d)
trap 'rm -rf "$out"' EXIT
${CXX:-g++} -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined \
  tools/jpeg_entropy_check.cpp timetuning_amd/csrc/jpeg_scan.cpp -o "$out/jpeg_entropy_check"
python - "$out" <<'PY'
import sys
import numpy as np
for fixture in ("jpeg_frames", "jpeg_entropy"):
    g = np.load(f"tests/golden/{fixture}.npz")
    for i, name in enumerate(g["names"]):
        open(f"{sys.argv[1]}/{name}.jpg", "wb").write(g["blob"][g["offs"][i]:g["offs"][i + 1]].tobytes())
PY
"$out/jpeg_entropy_check" "$out"/*.jpg | tail -4
