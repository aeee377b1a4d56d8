#!/bin/bash
# Builds tools/png_check.cpp + timetuning_amd/csrc/png_scan.cpp (with csrc/png_inflate.hpp, the header the device kernel shares) with
# AddressSanitizer and UBSan - host code only: no GPU, nothing loaded into Python - and runs it over the files of
# tests/golden/png_streams.npz, written out to a temporary directory.
#   tools/png_check.sh          (CXX=g++ by default)
set -euo pipefail
cd "$(dirname "$0")/.."
out=$(mktemp -d)
trap 'rm -rf "$out"' EXIT
${CXX:-g++} -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread \
  tools/png_check.cpp timetuning_amd/csrc/png_scan.cpp -o "$out/png_check"
python - "$out" <<'PY'
import sys
import numpy as np
g = np.load("tests/golden/png_streams.npz")
for key in g.files:
    open(f"{sys.argv[1]}/{key}.png", "wb").write(g[key].tobytes())
PY
"$out/png_check" "$out"/*.png | tail -4
