// Stand-alone sanitizer harness of the N24 entropy route's host code (timetuning_amd/csrc/jpeg_scan.cpp + csrc/jpeg_huff.hpp, the header the
// kernels of jpeg_entropy.hip compile): built from these alone with -fsanitize=address,undefined (tools/jpeg_entropy_check.sh), no HIP, no
// Python.  For every file named on the command line it runs tt_jpeg_prepare + tt_jpeg_entropy_host at three subsequence sizes on the file
// itself, on every prefix length of the small files (64 cut positions of the others), with single bits flipped at 512 positions of the
// scan, with each restart marker removed and with each one renumbered - every input and every output in a heap block of exactly its
// size.  Two checks: wherever tt_jpeg_scan returns 0 the coefficients are equal, and wherever it does not the route's status has the same
// sign (never a crash, never a report) - the very code of tt_jpeg_scan where the stream reached the decode, the sign alone where
// tt_jpeg_prepare refused it (it judges markers without decoding).  Prints the counts; exit 0 = both held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/timetuning_hip.h"

static long counts[3], compared;   // ok, unsupported, malformed; coefficient buffers compared

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

static void run(const std::vector<uint8_t>& bytes, int subseq_bits) {
  Block<uint8_t> data(bytes.size());
  if (!bytes.empty()) std::memcpy(data.p, bytes.data(), bytes.size());
  int H, W, sampling;
  long long n = 0;
  int want = tt_jpeg_probe(data.p, bytes.size(), &H, &W, &sampling, &n);
  Block<int16_t> ref(want == 0 ? (size_t)n : 0);
  uint16_t qref[192], q[192];
  if (want == 0) want = tt_jpeg_scan(data.p, bytes.size(), ref.p, n, qref);
  size_t scan_cap, seg_cap;
  tt_jpeg_prepare_bytes(bytes.size(), &scan_cap, &seg_cap);
  Block<uint8_t> scan(scan_cap);
  Block<uint32_t> segs(2 * seg_cap);
  tt_jpeg_stream row;
  int got = tt_jpeg_prepare(data.p, bytes.size(), scan.p, scan_cap, segs.p, seg_cap, &row, q);
  if (got == 0) {
    // the tightest buffers: what prepare used
    const size_t used = (size_t)(row.scan_off + row.scan_len), nseg = (size_t)row.n_segments;
    Block<uint8_t> scan2(used);
    Block<uint32_t> segs2(2 * nseg);
    if (tt_jpeg_prepare(data.p, bytes.size(), scan2.p, used, segs2.p, nseg, &row, q) != 0) fail("prepare with exact capacities", 0, 0);
    {
      Block<uint8_t> scan3(used - 1);
      tt_jpeg_stream row3;
      uint16_t q3[192];
      if (tt_jpeg_prepare(data.p, bytes.size(), scan3.p, used - 1, segs.p, seg_cap, &row3, q3) != TT_JPEG_EARGUMENT)
        fail("a stream buffer one byte short was not refused", 0, 0);
      if (nseg > 1 && tt_jpeg_prepare(data.p, bytes.size(), scan.p, scan_cap, segs.p, nseg - 1, &row3, q3) != TT_JPEG_EARGUMENT)
        fail("a segment table one row short was not refused", 0, 0);
    }
    long long total = 0;
    if (tt_jpeg_probe(data.p, bytes.size(), &H, &W, &sampling, &total) != 0) fail("prepare took what probe refuses", 0, 0);
    Block<int16_t> coeffs((size_t)total);
    const size_t ws_bytes = tt_jpeg_entropy_batch_workspace_bytes(&row, 1, subseq_bits);
    Block<uint8_t> ws(ws_bytes);
    int32_t status = 1;
    const int rc = tt_jpeg_entropy_host(scan2.p, (long long)used, segs2.p, segs2.p, (long long)nseg, &row, &row, 1, subseq_bits, coeffs.p, total, &status,
                                        ws.p, ws_bytes, nullptr);
    if (rc != 0) fail("entropy_host refused prepare's tables", rc, 0);
    got = status;
    if (got != want) fail("the frame status is not tt_jpeg_scan's code", want, got);   // prepare let it through: the decode's code is the host's
    if (got > 0) fail("a positive frame status", got, 0);
    if (got == 0 && want == 0) {
      if (total != n || std::memcmp(coeffs.p, ref.p, sizeof(int16_t) * (size_t)n) != 0 || std::memcmp(q, qref, sizeof(q)) != 0)
        fail("coefficients differ from tt_jpeg_scan's", 0, 0);
      ++compared;
    }
  }
  if ((want == 0) != (got == 0) || (want > 0) != (got > 0) || (want > 0 && want != got)) fail("status differs from tt_jpeg_scan's", want, got);
  ++counts[want == 0 ? 0 : (want > 0 ? 1 : 2)];
}

int main(int argc, char** argv) {
  const int sizes[3] = {128, 1024, 4096};
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
    for (int s = 0; s < 3; ++s) run(bytes, sizes[s]);
    const size_t cuts = bytes.size() <= 1600 && a % 8 == 0 ? bytes.size() : 64;   // every prefix length of a handful
    for (size_t k = 0; k < cuts; ++k) run(std::vector<uint8_t>(bytes.begin(), bytes.begin() + (long)(bytes.size() * k / cuts)), sizes[k % 3]);
    size_t scan_at = 0;   // flips: in the scan, where the entropy layer reads
    for (size_t i = 0; i + 1 < bytes.size(); ++i)
      if (bytes[i] == 0xFF && bytes[i + 1] == 0xDA) scan_at = i;
    uint32_t state = 24001u + (uint32_t)a;
    for (int k = 0; k < 512 && scan_at + 16 < bytes.size(); ++k) {
      state = state * 1664525u + 1013904223u;
      std::vector<uint8_t> bad(bytes);
      bad[scan_at + (state >> 8) % (bad.size() - scan_at)] ^= (uint8_t)(1u << (state & 7u));
      run(bad, sizes[k % 3]);
    }
    for (size_t i = scan_at; i + 1 < bytes.size(); ++i) {
      if (bytes[i] == 0xFF && bytes[i + 1] >= 0xD0 && bytes[i + 1] <= 0xD7) {
        std::vector<uint8_t> gone(bytes), renumbered(bytes);
        gone.erase(gone.begin() + (long)i, gone.begin() + (long)i + 2);
        renumbered[i + 1] = (uint8_t)(0xD0 + ((bytes[i + 1] + 3) & 7));
        run(gone, sizes[i % 3]);
        run(renumbered, sizes[i % 3]);
      }
    }
  }
  std::printf("files: %d\nruns: %ld ok, %ld unsupported, %ld malformed\ncoefficient buffers equal to tt_jpeg_scan's: %ld\n", argc - 1, counts[0], counts[1],
              counts[2], compared);
  return 0;
}
