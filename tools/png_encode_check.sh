#!/bin/bash
# Builds tools/png_encode_check.cpp + timetuning_amd/csrc/png_scan.cpp (with csrc/png_deflate.hpp, the header the device kernels share,
# and csrc/png_inflate.hpp for the way back) with AddressSanitizer and UBSan - host code only: no GPU, nothing loaded into Python - and
# runs it: seeded maps encoded, wrapped into files, decoded back and compared.
#   tools/png_encode_check.sh          (CXX=g++ by default)
set -euo pipefail
cd "$(dirname "$0")/.."
out=$(mktemp -d)
trap 'rm -rf "$out"' EXIT
${CXX:-g++} -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread \
  tools/png_encode_check.cpp timetuning_amd/csrc/png_scan.cpp -o "$out/png_encode_check"
"$out/png_encode_check" | tail -4
