// Stand-alone sanitizer harness of the JPEG host parser (timetuning_amd/csrc/jpeg_scan.cpp, N21): built from that file alone with
// -fsanitize=address,undefined (tools/jpeg_scan_check.sh), no GPU, no Python.  For every file named on the command line it runs
// tt_jpeg_probe / tt_jpeg_scan on the file itself, on every prefix of it at 64 cut positions, with single bits flipped at 512 positions
// and with each restart marker removed - every input in a heap block of exactly its length and every output in a block of exactly the
// size the probe asked for, so a read or write one byte outside is reported.  Prints the status counts; exit 0 = no report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/timetuning_hip.h"

static long counts[3];   // ok, unsupported, malformed

static int run(const std::vector<uint8_t>& bytes) {
  uint8_t* data = static_cast<uint8_t*>(std::malloc(bytes.size() ? bytes.size() : 1));   // exactly the file: no slack behind it
  if (!bytes.empty()) std::memcpy(data, bytes.data(), bytes.size());
  int H, W, sampling;
  long long n;
  int rc = tt_jpeg_probe(data, bytes.size(), &H, &W, &sampling, &n);
  if (rc == 0) {
    int16_t* coeffs = static_cast<int16_t*>(std::malloc(sizeof(int16_t) * (size_t)n));
    uint16_t* q = static_cast<uint16_t*>(std::malloc(sizeof(uint16_t) * 192));
    rc = tt_jpeg_scan(data, bytes.size(), coeffs, n, q);
    if (rc == 0 && tt_jpeg_scan(data, bytes.size(), coeffs, n - 1, q) != TT_JPEG_EARGUMENT) {
      std::fprintf(stderr, "a coefficient buffer one element short was not refused\n");
      std::exit(2);
    }
    std::free(coeffs);
    std::free(q);
  }
  std::free(data);
  ++counts[rc == 0 ? 0 : (rc > 0 ? 1 : 2)];
  return rc;
}

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    std::FILE* f = std::fopen(argv[a], "rb");
    if (!f) {
      std::fprintf(stderr, "cannot open %s\n", argv[a]);
      return 2;
    }
    std::vector<uint8_t> bytes;
    uint8_t chunk[4096];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) bytes.insert(bytes.end(), chunk, chunk + got);
    std::fclose(f);
    const int whole = run(bytes);
    for (int k = 0; k < 64; ++k) run(std::vector<uint8_t>(bytes.begin(), bytes.begin() + (long)(bytes.size() * (size_t)k / 64)));
    uint32_t state = 12345u + (uint32_t)a;
    for (int k = 0; k < 512 && !bytes.empty(); ++k) {
      state = state * 1664525u + 1013904223u;
      std::vector<uint8_t> bad(bytes);
      bad[(state >> 8) % bad.size()] ^= (uint8_t)(1u << (state & 7u));
      run(bad);
    }
    for (size_t i = 0; i + 1 < bytes.size(); ++i) {
      if (bytes[i] == 0xFF && bytes[i + 1] >= 0xD0 && bytes[i + 1] <= 0xD7) {
        std::vector<uint8_t> bad(bytes);
        bad.erase(bad.begin() + (long)i, bad.begin() + (long)i + 2);
        run(bad);
      }
    }
    std::printf("%s: status %d\n", argv[a], whole);
  }
  std::printf("runs: %ld ok, %ld unsupported, %ld malformed\n", counts[0], counts[1], counts[2]);
  return 0;
}
