// Stand-alone sanitizer harness of the N29 route's host code (timetuning_amd/csrc/png_scan.cpp + csrc/png_deflate.hpp, the header the kernels
// of png_encode.hip compile): built from these alone with -fsanitize=address,undefined (tools/png_encode_check.sh), no HIP, no Python.
// It runs tt_png_encode_plan + tt_png_encode_host + tt_png_write_file over seeded maps - the shapes of the test list (tests/_png_enc_ref.py:
// the 1- and 2-pixel maps, the run lengths around 258, the 8/9-bit literal boundary, constant maps, wrapping rows, rows_per_chunk - 1, + 0,
// + 1 at W = 100, runs across chunk boundaries, 1 x 32767, 16384 x 1, noise at the capacity, the two workload sizes) and a few thousand
// random small ones, alone and in batches of mixed sizes, contiguous and pitched - every map, table, workspace, output and file in a heap
// block of exactly its size.  Every file goes back through tt_png_probe / tt_png_prepare / tt_png_decode_host and the pixels are compared;
// a stream is checked against the capacity rule, a batch against its maps encoded alone, and buffers one byte short must be refused.
// Prints the counts; exit 0 = all held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/timetuning_hip.h"

static long n_files, n_batches, n_bytes_in, n_bytes_out;
static uint32_t rng_state = 29001u;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u, rng_state >> 8; }

template <class T>
struct Block {   // exactly n elements: no slack behind them
  T* p;
  size_t n;
  explicit Block(size_t count) : p(nullptr), n(count) {   // 16-byte aligned (the workspace must be), the sanitizer's red zone right behind byte n
    if (posix_memalign(reinterpret_cast<void**>(&p), 16, count * sizeof(T) ? count * sizeof(T) : 1) != 0) std::abort();
  }
  ~Block() { std::free(p); }
  Block(const Block&) = delete;
};

static void fail(const char* what, long a, long b) {
  std::fprintf(stderr, "FAILED: %s (%ld, %ld)\n", what, a, b);
  std::exit(2);
}

struct Map {
  int H, W, pitch;
  std::vector<uint8_t> px;   // H x W, contiguous
};

// kind: 0 noise of a few values, 1 runs of random lengths up to 700, 2 noise of 9-bit codes after the filter, 3 constant, 4 blobs of rows
static Map make(int H, int W, int kind) {
  Map m{H, W, W, std::vector<uint8_t>((size_t)H * W)};
  if (kind == 3) {
    std::memset(m.px.data(), (int)(rnd() & 255u), m.px.size());
  } else if (kind == 1) {
    for (size_t i = 0; i < m.px.size();) {
      const size_t L = 1 + rnd() % 700;
      const uint8_t v = (uint8_t)(rnd() % 5 == 0 ? 2 : rnd());
      for (size_t k = 0; k < L && i < m.px.size(); ++k) m.px[i++] = v;
    }
  } else if (kind == 2) {
    for (int r = 0; r < H; ++r)
      for (int c = 0; c < W; ++c) m.px[(size_t)r * W + c] = (uint8_t)((r ? m.px[(size_t)(r - 1) * W + c] : 0) + 144 + rnd() % 112);
  } else if (kind == 4) {
    for (int r = 0; r < H; ++r) {
      const int a = (int)(rnd() % (unsigned)W), b = (int)(rnd() % (unsigned)W);
      for (int c = 0; c < W; ++c) m.px[(size_t)r * W + c] = (uint8_t)((c >= (a < b ? a : b) && c <= (a < b ? b : a)) ? 1 + r / 40 % 3 : 0);
    }
  } else {
    for (uint8_t& v : m.px) v = (uint8_t)(rnd() % 3 * 100);
  }
  return m;
}

struct Encoded {
  std::vector<std::vector<uint8_t>> streams;
  std::vector<uint32_t> adler;
};

// Encodes the maps in ONE call (pitched: every map inside rows `extra` bytes longer) and checks every file through the decoder.
static Encoded encode(const std::vector<Map>& maps, int extra) {
  const int n = (int)maps.size();
  std::vector<Block<uint8_t>*> data;
  Block<tt_png_map> table((size_t)n);
  for (int i = 0; i < n; ++i) {
    const Map& m = maps[(size_t)i];
    const int pitch = m.W + extra;
    Block<uint8_t>* d = new Block<uint8_t>((size_t)(m.H - 1) * pitch + m.W);   // the last row ends with its last pixel
    for (int r = 0; r < m.H; ++r) std::memcpy(d->p + (size_t)r * pitch, m.px.data() + (size_t)r * m.W, (size_t)m.W);
    data.push_back(d);
    std::memset(&table.p[i], 0, sizeof(tt_png_map));
    table.p[i].data = d->p;
    table.p[i].H = m.H;
    table.p[i].W = m.W;
    table.p[i].pitch = pitch;
    n_bytes_in += (long)m.px.size();
  }
  long long n_chunks = 0, cap = 0;
  if (tt_png_encode_plan(table.p, n, nullptr, 0, &n_chunks, &cap) != 0) fail("plan refused the maps", n, 0);
  Block<tt_png_chunk> chunks((size_t)n_chunks);
  if (n_chunks > 1 && tt_png_encode_plan(table.p, n, chunks.p, n_chunks - 1, &n_chunks, &cap) != TT_PNG_EARGUMENT) fail("a chunk table one row short was not refused", 0, 0);
  if (tt_png_encode_plan(table.p, n, chunks.p, n_chunks, &n_chunks, &cap) != 0) fail("plan refused its own count", 0, 0);
  const size_t ws_bytes = tt_png_encode_batch_workspace_bytes(table.p, n);
  if (ws_bytes == 0) fail("no workspace size for planned maps", 0, 0);
  Block<uint8_t> ws(ws_bytes), out((size_t)cap);
  Block<tt_png_result> res((size_t)n);
  if (tt_png_encode_host(table.p, nullptr, n, chunks.p, nullptr, n_chunks, out.p, cap - 1, res.p, ws.p, ws_bytes, nullptr) != TT_PNG_EARGUMENT)
    fail("an output one byte short was not refused", 0, 0);
  if (tt_png_encode_host(table.p, nullptr, n, chunks.p, nullptr, n_chunks, out.p, cap, res.p, ws.p, ws_bytes - 1, nullptr) != TT_PNG_EARGUMENT)
    fail("a workspace one byte short was not refused", 0, 0);
  std::memset(ws.p, 0xff, ws_bytes);   // a workspace that is not cleared
  if (tt_png_encode_host(table.p, nullptr, n, chunks.p, nullptr, n_chunks, out.p, cap, res.p, ws.p, ws_bytes, nullptr) != 0) fail("encode_host refused the plan", 0, 0);
  ++n_batches;
  Encoded e;
  long long at = 0;
  uint8_t palette[3 * 256];
  for (int k = 0; k < 3 * 256; ++k) palette[k] = (uint8_t)rnd();
  for (int i = 0; i < n; ++i) {
    const Map& m = maps[(size_t)i];
    if (res.p[i].offset != at) fail("the streams are not compact", i, (long)res.p[i].offset);
    at += res.p[i].length;
    long long rule = 0;   // (9 n + 7) / 8 + 7 per chunk of n filtered bytes
    for (long long c = table.p[i].first_chunk; c < table.p[i].first_chunk + table.p[i].n_chunks; ++c) rule += (9 * chunks.p[c].rows * (m.W + 1) + 7) / 8 + 7;
    if (res.p[i].length > rule) fail("a stream above the capacity rule", i, (long)res.p[i].length);
    e.streams.emplace_back(out.p + res.p[i].offset, out.p + res.p[i].offset + res.p[i].length);
    e.adler.push_back((uint32_t)res.p[i].adler);
    // the file, in a block of exactly its size, with and without a palette
    const int entries = i % 3 == 2 ? 0 : 1 + (int)(rnd() % 256);
    const size_t size = tt_png_file_bytes((size_t)res.p[i].length, entries);
    Block<uint8_t> stream((size_t)res.p[i].length), file(size);
    std::memcpy(stream.p, out.p + res.p[i].offset, (size_t)res.p[i].length);
    size_t got = 0;
    if (tt_png_write_file(stream.p, stream.n, e.adler.back(), m.H, m.W, entries ? palette : nullptr, entries, file.p, size - 1, &got) != TT_PNG_EARGUMENT)
      fail("a file buffer one byte short was not refused", i, 0);
    if (tt_png_write_file(stream.p, stream.n, e.adler.back(), m.H, m.W, entries ? palette : nullptr, entries, file.p, size, &got) != 0 || got != size)
      fail("write_file", i, (long)got);
    n_bytes_out += (long)size;
    ++n_files;
    // ... and back through the N26 route
    int H = 0, W = 0, depth = 0, color = 0;
    if (tt_png_probe(file.p, size, &H, &W, &depth, &color) != 0 || H != m.H || W != m.W || depth != 8 || color != (entries ? 3 : 0)) fail("probe", i, H);
    size_t pcap = 0;
    tt_png_prepare_bytes(size, &pcap);
    Block<uint32_t> prepared((pcap + 3) / 4);
    tt_png_stream row;
    if (tt_png_prepare(file.p, size, reinterpret_cast<uint8_t*>(prepared.p), pcap, &row) != 0) fail("prepare", i, 0);
    const size_t dws = tt_png_decode_batch_workspace_bytes(&row, 1);
    Block<uint32_t> dws_block((dws + 3) / 4);
    Block<uint8_t> pixels(m.px.size());
    int32_t status = 1;
    if (tt_png_decode_host(reinterpret_cast<uint8_t*>(prepared.p), (long long)((row.stream_len + 3) / 4 * 4), &row, &row, 1, pixels.p, (long long)m.px.size(), dws_block.p, dws,
                           &status, nullptr) != 0 || status != 0)
      fail("decode_host", i, status);
    if (std::memcmp(pixels.p, m.px.data(), m.px.size()) != 0) fail("the decoded pixels differ", i, 0);
  }
  for (Block<uint8_t>* d : data) delete d;
  return e;
}

static void same(const Encoded& a, size_t ia, const Encoded& b, size_t ib, const char* what) {
  if (a.streams[ia] != b.streams[ib] || a.adler[ia] != b.adler[ib]) fail(what, (long)ia, (long)ib);
}

int main() {
  // the shapes of the test list
  std::vector<Map> list;
  list.push_back(make(1, 1, 0));
  list.push_back(make(1, 2, 0));
  list.push_back(make(2, 1, 0));
  {
    const int runs[11] = {1, 2, 3, 4, 258, 259, 260, 261, 262, 517, 520};
    const uint8_t values[2][4] = {{5, 9, 77, 130}, {2, 143, 144, 255}};   // neighbours differ; the 8/9-bit boundary and the filter byte
    for (int v = 0; v < 2; ++v) {
      Map m{1, 0, 0, {}};
      for (int k = 0; k < 11; ++k) m.px.insert(m.px.end(), (size_t)runs[k], values[v][k % 4]);
      m.W = m.pitch = (int)m.px.size();
      list.push_back(m);
    }
  }
  list.push_back(make(40, 300, 3));
  list.push_back(make(50, 70, 0));
  for (int r = 0; r < 50; ++r) std::memset(list.back().px.data() + (size_t)r * 70, r % 2 ? 10 : 200, 70);
  for (int H = 161; H <= 163; ++H) list.push_back(make(H, 100, 4));
  list.push_back(make(400, 99, 1));
  list.push_back(make(1, 32767, 1));
  list.push_back(make(1, 32767, 2));
  list.push_back(make(16384, 1, 0));
  list.push_back(make(64, 100, 2));
  list.push_back(make(480, 854, 4));
  list.push_back(make(375, 500, 4));
  const Encoded all = encode(list, 0);
  const Encoded pitched = encode(list, 13);
  for (size_t i = 0; i < list.size(); ++i) {
    same(all, i, pitched, i, "a pitched map differs from its contiguous copy");
    const Encoded one = encode(std::vector<Map>(1, list[i]), 0);
    same(all, i, one, 0, "a map alone differs from the map inside the batch");
  }
  // random small maps, in batches of mixed sizes
  long random_maps = 0;
  for (int b = 0; b < 400; ++b) {
    std::vector<Map> maps;
    const int n = 1 + (int)(rnd() % 12);
    for (int i = 0; i < n; ++i) {
      const int shape = (int)(rnd() % 4);
      const int H = shape == 0 ? 1 + (int)(rnd() % 4) : 1 + (int)(rnd() % 200), W = shape == 1 ? 1 + (int)(rnd() % 4) : 1 + (int)(rnd() % 300);
      maps.push_back(make(H, W, (int)(rnd() % 5)));
    }
    const Encoded e = encode(maps, (int)(rnd() % 3) * 7);
    const size_t pick = rnd() % maps.size();
    same(e, pick, encode(std::vector<Map>(1, maps[pick]), 0), 0, "a random map alone differs from the map inside its batch");
    random_maps += n;
  }
  std::printf("list maps: %zu (each in the batch, pitched and alone)\nrandom maps: %ld in 400 batches\nfiles written and decoded back: %ld in %ld calls\n"
              "map bytes %ld -> file bytes %ld\n",
              list.size(), random_maps, n_files, n_batches, n_bytes_in, n_bytes_out);
  return 0;
}
