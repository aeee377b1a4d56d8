// Stand-alone sanitizer harness of the N26 route's host code (timetuning_amd/csrc/png_scan.cpp + csrc/png_inflate.hpp, the header the kernel
// of png_decode.hip compiles): built from these alone with -fsanitize=address,undefined (tools/png_check.sh), no HIP, no Python.  For every
// file named on the command line it runs tt_png_probe + tt_png_prepare + tt_png_decode_host on the file itself, on every prefix length of
// the small files (64 cut positions of the others), with single bits flipped at 256 positions of the file and at 512 positions of the
// prepared deflate stream (where no CRC stands in front of the inflate), with each chunk removed and each pair of neighbours swapped -
// every input, stream, workspace and output in a heap block of exactly its size.  Checks: a fixture file gives the status its name
// documents (ok__*: 0, uns__<r>__*: r, bad__m<s>__*: -s); prepare never takes what probe refuses; capacities one byte short are refused;
// a mutated file gives SOME status - never a crash, never a report; and the 64-lane emulation tt_png_decode_host_wave (the kernel's lanes as
// 64 threads behind a barrier: pending literals, lane-strided copies, the table fill, the Adler partial sums) gives the status and the
// pixels of the sequential one on every intact file and on 48 of the stream flips of each.  Prints the counts; exit 0 = all held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/timetuning_hip.h"

static long counts[3], waves;   // ok, unsupported, malformed; runs repeated on the 64-lane emulation

template <class T>
struct Block {   // exactly n elements: no slack behind them
  T* p;
  explicit Block(size_t n) : p(static_cast<T*>(std::malloc(n ? n * sizeof(T) : 1))) {}
  ~Block() { std::free(p); }
};

static void fail(const char* what, int a, int b) {
  std::fprintf(stderr, "FAILED: %s (%d, %d)\n", what, a, b);
  std::exit(2);
}

// The status of the whole route; flip >= 0: that bit of the prepared stream is flipped before the decode.
static int run(const std::vector<uint8_t>& bytes, long flip = -1, bool wave = false) {
  Block<uint8_t> data(bytes.size());
  if (!bytes.empty()) std::memcpy(data.p, bytes.data(), bytes.size());
  int H = 0, W = 0, depth = 0, color = 0;
  const int probed = tt_png_probe(data.p, bytes.size(), &H, &W, &depth, &color);
  size_t cap = 0;
  tt_png_prepare_bytes(bytes.size(), &cap);
  Block<uint8_t> big(cap);
  tt_png_stream row;
  int got = tt_png_prepare(data.p, bytes.size(), big.p, cap, &row);
  if (got == 0 && probed != 0) fail("prepare took what probe refuses", probed, got);
  if (probed > 0 && got != probed && got != TT_PNG_ECHECKSUM) fail("prepare neither gives probe's reason nor a CRC error", probed, got);
  if (probed < 0 && got >= 0) fail("prepare took a file probe calls malformed", probed, got);
  if (got == 0) {
    const size_t used = (size_t)(row.stream_len + 3) / 4 * 4;
    Block<uint32_t> stream(used / 4);   // exactly the padded stream, 4-byte aligned
    std::memcpy(stream.p, big.p, used);
    if (flip >= 0 && row.stream_len > 0) reinterpret_cast<uint8_t*>(stream.p)[(size_t)(flip / 8) % (size_t)row.stream_len] ^= (uint8_t)(1u << (flip & 7));
    const size_t ws_bytes = tt_png_decode_batch_workspace_bytes(&row, 1);
    if (ws_bytes == 0) fail("prepare wrote a row the decoder does not take", 0, 0);
    Block<uint32_t> ws((ws_bytes + 3) / 4);
    const long long out_bytes = (long long)row.H * row.W;
    Block<uint8_t> out((size_t)out_bytes);
    int32_t status = 1;
    const uint8_t* s = reinterpret_cast<const uint8_t*>(stream.p);
    if (tt_png_decode_host(s, (long long)used, &row, &row, 1, out.p, out_bytes - 1, ws.p, ws_bytes, &status, nullptr) != TT_EINVAL)
      fail("an output one byte short was not refused", 0, 0);
    if (tt_png_decode_host(s, (long long)used, &row, &row, 1, out.p, out_bytes, ws.p, ws_bytes - 1, &status, nullptr) != TT_EINVAL)
      fail("a workspace one byte short was not refused", 0, 0);
    if (used && tt_png_decode_host(s, (long long)used - 1, &row, &row, 1, out.p, out_bytes, ws.p, ws_bytes, &status, nullptr) != TT_EINVAL)
      fail("a stream buffer one byte short was not refused", 0, 0);
    if (tt_png_decode_host(s, (long long)used, &row, &row, 1, out.p, out_bytes, ws.p, ws_bytes, &status, nullptr) != 0) fail("decode_host refused prepare's row", 0, 0);
    got = status;
    if (got > 0) fail("a positive file status", got, 0);
    if (wave) {
      Block<uint32_t> ws2((ws_bytes + 3) / 4);
      Block<uint8_t> out2((size_t)out_bytes);
      int32_t status2 = 1;
      if (tt_png_decode_host_wave(s, (long long)used, &row, &row, 1, out2.p, out_bytes, ws2.p, ws_bytes, &status2, nullptr) != 0)
        fail("decode_host_wave refused prepare's row", 0, 0);
      if (status2 != status) fail("the 64-lane status differs from the sequential one", status, status2);
      if (status == 0 && std::memcmp(out.p, out2.p, (size_t)out_bytes) != 0) fail("the 64-lane pixels differ from the sequential ones", 0, 0);
      ++waves;
    }
  }
  ++counts[got == 0 ? 0 : (got > 0 ? 1 : 2)];
  return got;
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
    std::string name(argv[a]);
    name = name.substr(name.find_last_of('/') + 1);
    int want = 0;
    if (name.rfind("uns__", 0) == 0) want = std::atoi(name.c_str() + 5);
    if (name.rfind("bad__m", 0) == 0) want = -std::atoi(name.c_str() + 6);
    const int status = run(bytes, -1, bytes.size() <= 20000);
    if (status != want) fail(name.c_str(), want, status);
    const size_t cuts = bytes.size() <= 1200 ? bytes.size() : 64;
    for (size_t k = 0; k < cuts; ++k) run(std::vector<uint8_t>(bytes.begin(), bytes.begin() + (long)(bytes.size() * k / cuts)));
    uint32_t state = 26001u + (uint32_t)a;
    for (int k = 0; k < 256; ++k) {
      state = state * 1664525u + 1013904223u;
      std::vector<uint8_t> bad(bytes);
      bad[(state >> 8) % bad.size()] ^= (uint8_t)(1u << (state & 7u));
      run(bad);
    }
    if (bytes.size() <= 20000)
      for (int k = 0; k < 512; ++k) {
        state = state * 1664525u + 1013904223u;
        run(bytes, (long)(state >> 4), k < 48);
      }
    std::vector<size_t> at;   // chunk starts, and the end
    for (size_t p = 8; p + 12 <= bytes.size();) {
      at.push_back(p);
      const size_t n = ((size_t)bytes[p] << 24) | ((size_t)bytes[p + 1] << 16) | ((size_t)bytes[p + 2] << 8) | bytes[p + 3];
      if (n > bytes.size() - p - 12) break;
      p += 12 + n;
    }
    at.push_back(bytes.size());
    for (size_t c = 0; c + 1 < at.size() && at.size() <= 40; ++c) {
      std::vector<uint8_t> gone(bytes.begin(), bytes.begin() + (long)at[c]);
      gone.insert(gone.end(), bytes.begin() + (long)at[c + 1], bytes.end());
      run(gone);
      if (c + 2 < at.size()) {
        std::vector<uint8_t> swapped(bytes.begin(), bytes.begin() + (long)at[c]);
        swapped.insert(swapped.end(), bytes.begin() + (long)at[c + 1], bytes.begin() + (long)at[c + 2]);
        swapped.insert(swapped.end(), bytes.begin() + (long)at[c], bytes.begin() + (long)at[c + 1]);
        swapped.insert(swapped.end(), bytes.begin() + (long)at[c + 2], bytes.end());
        run(swapped);
      }
    }
  }
  std::printf("files: %d\nruns: %ld ok, %ld unsupported, %ld malformed\nrepeated on 64 lanes: %ld\n", argc - 1, counts[0], counts[1], counts[2], waves);
  return 0;
}
