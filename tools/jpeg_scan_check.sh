#!/bin/bash
# Builds tools/jpeg_scan_check.cpp + timetuning_amd/csrc/jpeg_scan.cpp with AddressSanitizer and UBSan (host code only: no GPU, nothing
# loaded into Python) and runs it over the files of tests/golden/jpeg_frames.npz, written out to a temporary directory.
#   tools/jpeg_scan_check.sh          (CXX=g++ by default)
set -euo pipefail
cd "$(dirname "$0")/.."
out=$(mktemp -d)
trap 'rm -rf "$out"' EXIT
${CXX:-g++} -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined \
  tools/jpeg_scan_check.cpp timetuning_amd/csrc/jpeg_scan.cpp -o "$out/jpeg_scan_check"
python - "$out" <<'PY'
import sys
import numpy as np
g = np.load("tests/golden/jpeg_frames.npz")
for i, name in enumerate(g["names"]):
    open(f"{sys.argv[1]}/{name}.jpg", "wb").write(g["blob"][g["offs"][i]:g["offs"][i + 1]].tobytes())
PY
"$out/jpeg_scan_check" "$out"/*.jpg | tail -4
