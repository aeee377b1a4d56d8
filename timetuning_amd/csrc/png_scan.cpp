// N26, host half: the chunk layer of an annotation PNG (tt_png_probe, tt_png_prepare) and the emulation of png_decode.hip
// (tt_png_decode_host: the sequential loop over the steps of png_inflate.hpp).  Plain C++: no HIP include, no state, no allocation,
// re-entrant; every read is checked against `len`, every write against the caller's capacity.  The one exception is the testing aid
// tt_png_decode_host_wave, which starts 64 threads.
// N29, host half, at the end: the file around a device-made stream (tt_png_file_bytes, tt_png_write_file), the tables of a batch
// (tt_png_encode_plan) and the emulation of png_encode.hip (tt_png_encode_host: the sequential loop over the steps of png_deflate.hpp).
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "png_deflate.hpp"
#include "png_inflate.hpp"

namespace {

using namespace tt;

struct Crc {
  uint32_t t[256];
  constexpr Crc() : t() {
    for (uint32_t n = 0; n < 256; ++n) {
      uint32_t c = n;
      for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
      t[n] = c;
    }
  }
};
constexpr Crc kCrc;

uint32_t crc32(const uint8_t* p, size_t n) {
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) c = kCrc.t[(c ^ p[i]) & 255u] ^ (c >> 8);
  return c ^ 0xffffffffu;
}

uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]; }
bool is(const uint8_t* type, const char* name) { return std::memcmp(type, name, 4) == 0; }

constexpr uint8_t kSignature[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};

struct Header {
  uint32_t H, W;
  int depth, color, interlace;
};

// Signature and IHDR: 0 or a negative code.  `at` is left at the first chunk behind IHDR.
int read_header(const uint8_t* data, size_t len, Header& h, size_t& at, bool check_crc) {
  if (!data) return TT_PNG_EARGUMENT;
  if (len < 8 || std::memcmp(data, kSignature, 8) != 0) return TT_PNG_EMALFORMED;
  if (len < 8 + 12) return TT_PNG_ETRUNCATED;
  if (be32(data + 8) != 13 || !is(data + 12, "IHDR")) return TT_PNG_EMALFORMED;
  if (len < 8 + 12 + 13) return TT_PNG_ETRUNCATED;
  const uint8_t* d = data + 16;
  if (check_crc && crc32(data + 12, 4 + 13) != be32(d + 13)) return TT_PNG_ECHECKSUM;
  h.W = be32(d);
  h.H = be32(d + 4);
  h.depth = d[8];
  h.color = d[9];
  h.interlace = d[12];
  if (h.W == 0 || h.H == 0 || h.W > 0x7fffffffu || h.H > 0x7fffffffu) return TT_PNG_EMALFORMED;
  if (d[10] != 0 || d[11] != 0 || h.interlace > 1) return TT_PNG_EMALFORMED;   // compression and filter method 0
  const int dp = h.depth;
  bool legal = false;
  if (h.color == 0) legal = dp == 1 || dp == 2 || dp == 4 || dp == 8 || dp == 16;
  if (h.color == 3) legal = dp == 1 || dp == 2 || dp == 4 || dp == 8;
  if (h.color == 2 || h.color == 4 || h.color == 6) legal = dp == 8 || dp == 16;
  if (!legal) return TT_PNG_EMALFORMED;
  at = 8 + 12 + 13;
  return 0;
}

int unsupported(const Header& h) {
  if (h.interlace) return TT_PNG_UNSUPPORTED_INTERLACE;
  if (h.color != 0 && h.color != 3) return TT_PNG_UNSUPPORTED_COLOUR;
  if (h.depth == 16) return TT_PNG_UNSUPPORTED_16BIT;
  if (h.color == 0 && h.depth < 8) return TT_PNG_UNSUPPORTED_GRAY_DEPTH;
  if (h.H > (uint32_t)pz::kMaxDim || h.W > (uint32_t)pz::kMaxDim) return TT_PNG_UNSUPPORTED_SIZE;
  return 0;
}

// Walks the chunks behind IHDR up to IEND.  With `stream`: checks the critical chunks' CRC-32 and appends the IDAT payloads.
int walk_chunks(const uint8_t* data, size_t len, size_t at, bool check_crc, uint8_t* stream, size_t capacity, size_t* idat_bytes) {
  size_t total = 0;
  bool seen_idat = false;
  for (;;) {
    if (len - at < 12) return TT_PNG_ETRUNCATED;
    const uint32_t n = be32(data + at);
    const uint8_t* type = data + at + 4;
    if (n > 0x7fffffffu) return TT_PNG_EMALFORMED;
    if (len - at - 12 < n) return TT_PNG_ETRUNCATED;
    const bool critical = (type[0] & 0x20u) == 0;
    if (check_crc && critical && crc32(type, 4 + (size_t)n) != be32(data + at + 8 + n)) return TT_PNG_ECHECKSUM;
    if (is(type, "IHDR")) return TT_PNG_EMALFORMED;
    if (is(type, "IDAT")) {
      seen_idat = true;
      if (stream) {
        if (capacity - total < n) return TT_PNG_EARGUMENT;
        std::memcpy(stream + total, data + at + 8, n);
      }
      total += n;
    } else if (is(type, "IEND")) {
      break;
    }
    at += 12 + (size_t)n;
  }
  if (!seen_idat) return TT_PNG_EMALFORMED;
  *idat_bytes = total;
  return 0;
}

struct HostCtx {
  static constexpr int NL = 1;
  int lane = 0;
  void sync() {}
};

// The 64-lane context on the host: one thread per lane, sync() a barrier of all of them.
struct Barrier {
  std::mutex m;
  std::condition_variable cv;
  int n, count = 0;
  unsigned generation = 0;
  explicit Barrier(int lanes) : n(lanes) {}
  void wait() {
    std::unique_lock<std::mutex> lock(m);
    const unsigned g = generation;
    if (++count == n) {
      count = 0;
      ++generation;
      cv.notify_all();
    } else {
      cv.wait(lock, [&] { return generation != g; });
    }
  }
};

struct WaveHostCtx {
  static constexpr int NL = pz::kLanes;
  int lane;
  Barrier* barrier;
  void sync() { barrier->wait(); }
};

}  // namespace

extern "C" int tt_png_probe(const uint8_t* data, size_t len, int* H, int* W, int* bit_depth, int* color_type) {
  if (!H || !W || !bit_depth || !color_type) return TT_PNG_EARGUMENT;
  Header h{};
  size_t at = 0, idat = 0;
  int rc = read_header(data, len, h, at, false);
  if (rc) return rc;
  rc = walk_chunks(data, len, at, false, nullptr, 0, &idat);
  if (rc) return rc;
  *H = (int)h.H;
  *W = (int)h.W;
  *bit_depth = h.depth;
  *color_type = h.color;
  return unsupported(h);
}

extern "C" int tt_png_prepare_bytes(size_t len, size_t* stream_bytes) {
  if (!stream_bytes) return TT_PNG_EARGUMENT;
  *stream_bytes = (len + 3) / 4 * 4 + 4;
  return 0;
}

extern "C" int tt_png_prepare(const uint8_t* data, size_t len, uint8_t* stream, size_t stream_capacity, tt_png_stream* row) {
  if (!stream || !row) return TT_PNG_EARGUMENT;
  Header h{};
  size_t at = 0, idat = 0;
  int rc = read_header(data, len, h, at, true);
  if (rc) return rc;
  const int reason = unsupported(h);   // a broken chunk list comes first, as in tt_png_probe
  // the payloads land two bytes early so that the stream, not its zlib header, starts at stream[0]: copy, check, then move down
  rc = walk_chunks(data, len, at, true, reason ? nullptr : stream, stream_capacity, &idat);
  if (rc) return rc;
  if (reason) return reason;
  if (idat < 2) return TT_PNG_ETRUNCATED;
  const unsigned cmf = stream[0], flg = stream[1];
  if ((cmf & 15u) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31u != 0 || (flg & 0x20u)) return TT_PNG_EMALFORMED;
  const size_t n = idat - 2, padded = (n + 3) / 4 * 4;
  if (padded > stream_capacity) return TT_PNG_EARGUMENT;
  std::memmove(stream, stream + 2, n);
  std::memset(stream + n, 0, padded - n);
  std::memset(row, 0, sizeof(*row));
  row->H = h.H;
  row->W = h.W;
  row->depth = h.depth;
  row->color_type = h.color;
  row->row_bytes = ((long long)h.W * h.depth + 7) / 8;
  row->stream_len = (int64_t)n;
  return 0;
}

extern "C" size_t tt_png_decode_batch_workspace_bytes(const tt_png_stream* table, int n_files) { return pz::workspace_bytes(table, n_files); }

extern "C" int tt_png_decode_host(const uint8_t* streams, long long stream_bytes, const tt_png_stream* table, const tt_png_stream*, int n_files,
                                  uint8_t* out, long long out_bytes, void* workspace, size_t workspace_bytes, int32_t* status, tt_stream_t) {
  if (!streams || !table || !out || !workspace || !status) return TT_EINVAL;
  if ((reinterpret_cast<uintptr_t>(streams) & 3u) || (reinterpret_cast<uintptr_t>(workspace) & 3u)) return TT_EINVAL;
  char msg[256];
  if (pz::validate(stream_bytes, table, n_files, out_bytes, workspace_bytes, msg, sizeof(msg)) != 0) return TT_EINVAL;
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  int32_t* stats = reinterpret_cast<int32_t*>(ws + pz::slices_end(table, n_files));
  pz::Work work;
  for (int i = 0; i < n_files; ++i) {
    const tt_png_stream& r = table[i];
    HostCtx c;
    pz::Stats st{};
    uint8_t* raw = ws + r.ws_off;
    int rc = pz::inflate(c, work, reinterpret_cast<const uint32_t*>(streams + r.stream_off), (uint64_t)r.stream_len, raw, (uint64_t)pz::slice_bytes(r), st);
    if (rc == 0) rc = pz::unfilter_rows(raw, r.H, r.W, r.row_bytes, (int)r.depth, out + r.out_off, st);
    status[i] = rc;
    std::memcpy(stats + (size_t)i * pz::kStatWords, &st, sizeof(st));
  }
  return TT_OK;
}

// The inflate of the kernel with its 64 lanes: 64 threads run pz::inflate of every file side by side behind a barrier, so the pending
// literals, the lane-strided copies, the table fill by all lanes and the Adler partial sums run on the CPU as they do on the device
// (the wavefront of the unfilter is the kernel's own; here lane 0 runs the sequential form).  A testing aid: it starts threads.
extern "C" int tt_png_decode_host_wave(const uint8_t* streams, long long stream_bytes, const tt_png_stream* table, const tt_png_stream*, int n_files,
                                       uint8_t* out, long long out_bytes, void* workspace, size_t workspace_bytes, int32_t* status, tt_stream_t) {
  if (!streams || !table || !out || !workspace || !status) return TT_EINVAL;
  if ((reinterpret_cast<uintptr_t>(streams) & 3u) || (reinterpret_cast<uintptr_t>(workspace) & 3u)) return TT_EINVAL;
  char msg[256];
  if (pz::validate(stream_bytes, table, n_files, out_bytes, workspace_bytes, msg, sizeof(msg)) != 0) return TT_EINVAL;
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  int32_t* stats = reinterpret_cast<int32_t*>(ws + pz::slices_end(table, n_files));
  pz::Work work;
  Barrier barrier(pz::kLanes);
  auto lane_main = [&](int lane) {
    WaveHostCtx c{lane, &barrier};
    for (int i = 0; i < n_files; ++i) {
      const tt_png_stream& r = table[i];
      pz::Stats st{};
      uint8_t* raw = ws + r.ws_off;
      int rc = pz::inflate(c, work, reinterpret_cast<const uint32_t*>(streams + r.stream_off), (uint64_t)r.stream_len, raw, (uint64_t)pz::slice_bytes(r), st);
      barrier.wait();   // every lane has stored its bytes
      if (lane == 0) {
        if (rc == 0) rc = pz::unfilter_rows(raw, r.H, r.W, r.row_bytes, (int)r.depth, out + r.out_off, st);
        status[i] = rc;
        std::memcpy(stats + (size_t)i * pz::kStatWords, &st, sizeof(st));
      }
      barrier.wait();   // the shared tables are free for the next file
    }
  };
  std::vector<std::thread> lanes;
  for (int lane = 1; lane < pz::kLanes; ++lane) lanes.emplace_back(lane_main, lane);
  lane_main(0);
  for (std::thread& t : lanes) t.join();
  return TT_OK;
}

// ---- N29: writing

namespace {

void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

// Closes the chunk whose type starts at out[type_at] and whose data end at out[end]: length in front, CRC-32 behind; the next free byte.
size_t close_chunk(uint8_t* out, size_t type_at, size_t end) {
  put_be32(out + type_at - 4, (uint32_t)(end - type_at - 4));
  put_be32(out + end, crc32(out + type_at, end - type_at));
  return end + 4;
}

}  // namespace

extern "C" size_t tt_png_file_bytes(size_t stream_len, int palette_entries) {
  return 8 + (12 + 13) + (palette_entries > 0 ? 12 + 3 * (size_t)palette_entries : 0) + (12 + 2 + stream_len + 4) + 12;
}

extern "C" int tt_png_write_file(const uint8_t* stream, size_t stream_len, uint32_t adler, int H, int W, const uint8_t* palette, int palette_entries,
                                 uint8_t* out, size_t out_capacity, size_t* out_len) {
  if (!stream || !out || !out_len || H < 1 || W < 1 || H > pe::kMaxDim || W > pe::kMaxDim) return TT_PNG_EARGUMENT;
  if (palette_entries < 0 || palette_entries > 256 || (palette_entries > 0) != (palette != nullptr)) return TT_PNG_EARGUMENT;
  if (stream_len > 0x7ffffff0u || out_capacity < tt_png_file_bytes(stream_len, palette_entries)) return TT_PNG_EARGUMENT;
  std::memcpy(out, kSignature, 8);
  size_t at = 8 + 4;
  std::memcpy(out + at, "IHDR", 4);
  put_be32(out + at + 4, (uint32_t)W);
  put_be32(out + at + 8, (uint32_t)H);
  out[at + 12] = 8;
  out[at + 13] = palette_entries > 0 ? 3 : 0;
  out[at + 14] = out[at + 15] = out[at + 16] = 0;
  at = close_chunk(out, at, at + 17) + 4;
  if (palette_entries > 0) {
    std::memcpy(out + at, "PLTE", 4);
    std::memcpy(out + at + 4, palette, 3 * (size_t)palette_entries);
    at = close_chunk(out, at, at + 4 + 3 * (size_t)palette_entries) + 4;
  }
  std::memcpy(out + at, "IDAT", 4);
  out[at + 4] = 0x78;
  out[at + 5] = 0x01;
  std::memcpy(out + at + 6, stream, stream_len);
  put_be32(out + at + 6 + stream_len, adler);
  at = close_chunk(out, at, at + 6 + stream_len + 4) + 4;
  std::memcpy(out + at, "IEND", 4);
  at = close_chunk(out, at, at + 4);
  *out_len = at;
  return 0;
}

extern "C" int tt_png_encode_plan(tt_png_map* maps, int n_maps, tt_png_chunk* chunks, long long chunk_capacity, long long* n_chunks,
                                  long long* out_capacity) {
  if (!n_chunks || !out_capacity) return TT_PNG_EARGUMENT;
  pe::Layout l;
  const int rc = pe::plan(maps, n_maps, chunks, chunk_capacity, &l);
  if (rc) return rc;
  *n_chunks = l.n_chunks;
  *out_capacity = l.slot_bytes;
  return 0;
}

extern "C" size_t tt_png_encode_batch_workspace_bytes(const tt_png_map* maps, int n_maps) {
  if (!maps || n_maps < 1 || n_maps > 65535) return 0;
  pe::Layout l{0, 0};
  for (int i = 0; i < n_maps; ++i) {
    if (!pe::map_ok(maps[i])) return 0;
    l.n_chunks += pe::chunk_count(maps[i].H, maps[i].W);
    l.slot_bytes += pe::file_capacity(maps[i].H, maps[i].W);
    if (l.slot_bytes > pe::kMaxBatchBytes) return 0;
  }
  return (size_t)pe::workspace_bytes(l);
}

extern "C" int tt_png_encode_host(const tt_png_map* maps, const tt_png_map*, int n_maps, const tt_png_chunk* chunks, const tt_png_chunk*,
                                  long long n_chunks, uint8_t* out, long long out_bytes, tt_png_result* results, void* workspace,
                                  size_t workspace_bytes, tt_stream_t) {
  if (!maps || !chunks || !out || !results || !workspace) return TT_PNG_EARGUMENT;
  if (reinterpret_cast<uintptr_t>(workspace) & 15u) return TT_PNG_EARGUMENT;
  pe::Layout l;
  const char* why = "";
  if (pe::validate(maps, n_maps, chunks, n_chunks, out_bytes, workspace_bytes, &l, &why) != 0) return TT_PNG_EARGUMENT;
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  int32_t* meta = reinterpret_cast<int32_t*>(ws + pe::meta_offset(l));
  uint32_t* chunk_off = reinterpret_cast<uint32_t*>(ws + pe::offsets_offset(l));
  // the chunks: what one workgroup does, with one thread that owns every position
  for (long long c = 0; c < l.n_chunks; ++c) {
    const tt_png_chunk& ck = chunks[c];
    const tt_png_map& m = maps[ck.map];
    const int W = (int)m.W, row0 = (int)ck.row0, n = (int)ck.rows * (W + 1);
    auto F = [&](int p) { return pe::filtered(m.data, m.pitch, W, row0, p); };
    uint32_t token_bits = 0;
    pe::walk(F, 0, n, 0, n, [&](pe::Code code) { token_bits += (uint32_t)code.count; });
    const int len = pe::chunk_bytes(token_bits), words = (len + 3) / 4;
    if (words * 4 > pe::slot_stride(n)) return TT_PNG_EARGUMENT;   // the capacity rule, checked where the kernel relies on it
    uint32_t* slot = reinterpret_cast<uint32_t*>(ws + ck.slot_off);
    for (int k = 0; k < words; ++k) slot[k] = 0u;
    auto or32 = [&](uint32_t word, uint32_t v) {
      if (v != 0u && word < (uint32_t)words) slot[word] |= v;
    };
    uint32_t at = pe::kHeadBits;
    pe::walk(F, 0, n, 0, n, [&](pe::Code code) {
      pe::put_bits(or32, at, code.bits, code.count);
      at += (uint32_t)code.count;
    });
    pe::put_frame(or32, token_bits, c == m.first_chunk + m.n_chunks - 1);
    uint64_t sa = 0, sb = 0;
    for (int p = 0; p < n; ++p) {
      const uint32_t d = F(p);
      sa += d;
      sb += (uint64_t)(n - p) * d;
    }
    int32_t* o = meta + c * pe::kMetaWords;
    o[0] = len;
    o[1] = (int32_t)(sa % pe::kAdlerMod);
    o[2] = (int32_t)(sb % pe::kAdlerMod);
    o[3] = n;
  }
  // the scan
  uint32_t total = 0;
  for (long long c = 0; c < l.n_chunks; ++c) {
    chunk_off[c] = total;
    total += (uint32_t)meta[c * pe::kMetaWords];
  }
  for (int f = 0; f < n_maps; ++f) {
    const tt_png_map& m = maps[f];
    uint32_t A = 1, B = 0;
    int64_t length = 0;
    for (long long c = m.first_chunk; c < m.first_chunk + m.n_chunks; ++c) {
      const int32_t* o = meta + c * pe::kMetaWords;
      length += o[0];
      pe::adler_append(A, B, (uint32_t)o[1], (uint32_t)o[2], (uint32_t)o[3]);
    }
    results[f].offset = chunk_off[m.first_chunk];
    results[f].length = length;
    results[f].adler = (int64_t)((B << 16) | A);
    results[f].reserved = 0;
  }
  // the gather
  for (long long c = 0; c < l.n_chunks; ++c) {
    const int len = meta[c * pe::kMetaWords];
    if ((long long)chunk_off[c] + len > out_bytes) return TT_PNG_EARGUMENT;
    std::memcpy(out + chunk_off[c], ws + chunks[c].slot_off, (size_t)len);
  }
  return TT_OK;
}
