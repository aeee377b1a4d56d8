// N29: the deflate side of the label maps - the byte format of a device-made PNG stream as steps shared by the kernels of png_encode.hip,
// by the host emulation tt_png_encode_host (png_scan.cpp) and, through it, by the sanitizer program tools/png_encode_check.cpp.  No HIP
// include: with the host compiler alone the qualifiers are empty.  The rules live here and nowhere else.
//
// The format.  An 8-bit map uint8 [H, W] (1 <= H, W <= 32767).  Every row gets filter 2 (Up): row r becomes the byte 2, then
// x[r][c] - x[r - 1][c] (mod 256) with x[-1] = 0: H (W + 1) filtered bytes.  The file is cut into CHUNKS of whole rows,
// rows_per_chunk = max(1, min(H, 16384 / (W + 1))), the last one takes the remainder: at most 16 384 filtered bytes, or one row of at
// most 32 768.  The first row of a chunk reads the row above it from the INPUT, so no chunk depends on another's output.
//   tokens   the maximal runs of equal bytes of the chunk's filtered bytes (a run may cross rows, never a chunk boundary); a run of byte
//            b and length L is the literal b, then with rem = L - 1: while rem >= 3 a match of min(rem, 258) at distance 1, then rem
//            (0, 1, 2) literals b.  token() says it per position.
//   bits     one fixed-Huffman block (BFINAL 0, BTYPE 01), the tokens in the fixed code of RFC 1951 3.2.6 (distance code 0: five bits),
//            the end-of-block code; then an EMPTY STORED block (BFINAL 1 on the file's last chunk, BTYPE 00, zero bits to the byte
//            boundary, 00 00 FF FF) - the sync-flush construction.  A chunk is a whole number of bytes, a file's stream the plain
//            concatenation of its chunks.
//   zlib     78 01, the chunks, the Adler-32 of the filtered image big-endian; the chunks' (a, b, n) combine by adler_append.
//   capacity a literal costs at most 9 bits, so a chunk of n filtered bytes is at most slot_bytes(n) = (9 n + 7) / 8 + 7 bytes; the slots
//            of the workspace are that, rounded up to 4 (the kernel stores whole words).
// The order of execution never shows in the bytes: every token ORs its bits into a zeroed buffer at a bit offset that is a sum.
// The host is little-endian, as the device is.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/timetuning_hip.h"

#if defined(__HIPCC__)
#define PE_HD __host__ __device__ inline
#else
#define PE_HD inline
#endif

namespace tt {
namespace pe {

constexpr long long kMaxDim = 32767;      // the decoder's limit (png_inflate.hpp), and what keeps a single-row chunk within 32 768 bytes
constexpr int kChunkBytes = 16384;        // filtered bytes of a chunk of more than one row
constexpr int kMaxChunkBytes = 32768;     // ... of the single-row chunk of the widest map
constexpr int kFilterUp = 2;
constexpr uint32_t kAdlerMod = 65521u;
constexpr int kMetaWords = 4;             // int32 per chunk behind the slots: stream bytes, Adler a, Adler b, filtered bytes
constexpr long long kMaxBatchBytes = 0x7fffffffll;   // the slots of one call: the offsets of the device scan are 32-bit

// ---- the chunk rule and the capacities
PE_HD long long rows_per_chunk(long long H, long long W) {
  long long r = kChunkBytes / (W + 1);
  if (r > H) r = H;
  return r < 1 ? 1 : r;
}
PE_HD long long chunk_count(long long H, long long W) {
  const long long r = rows_per_chunk(H, W);
  return (H + r - 1) / r;
}
PE_HD constexpr long long slot_bytes(long long n) { return (9 * n + 7) / 8 + 7; }
PE_HD constexpr long long slot_stride(long long n) { return (slot_bytes(n) + 3) / 4 * 4; }
// the slots of one file, which is also the most its stream can take
PE_HD long long file_capacity(long long H, long long W) {
  const long long r = rows_per_chunk(H, W), rest = H % r;
  return (H / r) * slot_stride(r * (W + 1)) + (rest ? slot_stride(rest * (W + 1)) : 0);
}

// ---- the filtered byte at position p of the chunk that starts at row `row0` (x: the map, rows `pitch` bytes apart)
PE_HD uint8_t filtered(const uint8_t* x, long long pitch, int W, int row0, int p) {
  const unsigned rowlen = (unsigned)W + 1u;
  const long long r = row0 + (long long)((unsigned)p / rowlen);
  const unsigned c = (unsigned)p % rowlen;
  if (c == 0) return (uint8_t)kFilterUp;
  const uint8_t cur = x[r * pitch + (c - 1)];
  return (uint8_t)(cur - (r ? x[(r - 1) * pitch + (c - 1)] : (uint8_t)0));
}

// ---- the token at offset k of a run of byte `b` and length L
struct Token {
  int kind;    // 0 nothing, 1 a literal (value: the byte), 2 a match at distance 1 (value: its length)
  int value;
};
PE_HD Token token(uint8_t b, int k, int L) {
  if (k == 0) return Token{1, b};
  const int j = (k - 1) % 258, left = L - 1 - (k - 1 - j);
  if (left < 3) return Token{1, b};
  if (j == 0) return Token{2, left < 258 ? left : 258};
  return Token{0, 0};
}

// ---- the fixed code: the bits as they go into the stream (first bit = bit 0; Huffman codes are packed from their MSB) and their count
struct Code {
  uint32_t bits;
  int count;
};
PE_HD uint32_t reversed(uint32_t v, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
  return r;
}
PE_HD Code literal_code(int b) { return b < 144 ? Code{reversed(0x30u + (uint32_t)b, 8), 8} : Code{reversed(0x190u + (uint32_t)(b - 144), 9), 9}; }
// a match of `len` (3..258) at distance 1: the length symbol, its extra bits, the distance code 0 (five zero bits, no extra bits)
PE_HD Code length_code(int len) {
  int idx, extra_bits = 0;
  uint32_t extra = 0;
  if (len == 258) {
    idx = 28;
  } else if (len < 11) {
    idx = len - 3;
  } else {
    const int l = len - 3;   // 8 .. 254: groups of four symbols per power of two
    int e = 1;
    while ((l >> (e + 3)) != 0) ++e;
    idx = 4 * e + 4 + ((l >> e) & 3);
    extra_bits = e;
    extra = (uint32_t)l & ((1u << e) - 1u);
  }
  const int sym = 257 + idx;
  const int nb = sym < 280 ? 7 : 8;
  const uint32_t code = sym < 280 ? (uint32_t)(sym - 256) : 0xc0u + (uint32_t)(sym - 280);
  return Code{reversed(code, nb) | (extra << nb), nb + extra_bits + 5};
}
PE_HD Code end_code() { return Code{0u, 7}; }
PE_HD Code token_code(Token t) { return t.kind == 1 ? literal_code(t.value) : length_code(t.value); }
constexpr int kHeadBits = 3;   // BFINAL 0, BTYPE 01, LSB first: the value 2

// bytes of a chunk whose tokens take `token_bits`: header, tokens, end of block, the stored block's header, the byte boundary, 00 00 FF FF
PE_HD int chunk_bytes(uint32_t token_bits) { return (int)((kHeadBits + token_bits + 7 + 3 + 7) / 8) + 4; }

// ORs `count` (<= 18) bits into 32-bit words through or32(word index, value)
template <class Or>
PE_HD void put_bits(Or&& or32, uint32_t bitpos, uint32_t bits, int count) {
  const uint32_t w = bitpos >> 5, s = bitpos & 31u;
  or32(w, bits << s);
  if (s + (uint32_t)count > 32u) or32(w + 1, bits >> (32u - s));
}
// everything of a chunk that is no token: the block header and the stored block behind the end-of-block code
template <class Or>
PE_HD void put_frame(Or&& or32, uint32_t token_bits, bool last_chunk) {
  put_bits(or32, 0, 2u, kHeadBits);
  if (last_chunk) put_bits(or32, kHeadBits + token_bits + 7, 1u, 1);
  put_bits(or32, 8u * (uint32_t)(chunk_bytes(token_bits) - 2), 0xffffu, 16);
}

// ---- the tokens of positions [p0, p1) of a chunk, in order, through emit(Code).  F(p): the filtered byte at p.  s_in: the last run
// start before p0 (looked at only when p0 continues a run), e_out: the first run start at or after p1 (the chunk's length when there is
// none).  The whole chunk is walk(F, 0, n, 0, n, emit).
template <class Fb, class Emit>
PE_HD void walk(Fb&& F, int p0, int p1, int s_in, int e_out, Emit&& emit) {
  int p = p0;
  while (p < p1) {
    const uint8_t b = F(p);
    const int s = (p == 0 || F(p - 1) != b) ? p : s_in;   // only p0 can lie inside a run
    int q = p + 1;
    while (q < p1 && F(q) == b) ++q;
    const int L = (q < p1 ? q : e_out) - s;
    for (int i = p; i < q; ++i) {
      const Token t = token(b, i - s, L);
      if (t.kind) emit(token_code(t));
    }
    p = q;
  }
}

// ---- Adler-32.  A piece of n bytes d_i is (a, b, n) with a = sum d_i, b = sum (n - i) d_i (mod 65521); the checksum (A, B) of a stream,
// (1, 0) when empty, takes a piece at its end by adler_append.
PE_HD void adler_append(uint32_t& A, uint32_t& B, uint32_t a, uint32_t b, uint32_t n) {
  B = (uint32_t)((B + (uint64_t)(n % kAdlerMod) * A + b) % kAdlerMod);
  A = (A + a) % kAdlerMod;
}

// ---- the tables of a batch (include/timetuning_hip.h): what tt_png_encode_plan writes is what every entry point demands
struct Layout {
  long long n_chunks, slot_bytes;   // slot_bytes: the slots of all files = the capacity of the output
};
PE_HD long long align16(long long v) { return (v + 15) / 16 * 16; }
PE_HD long long meta_offset(const Layout& l) { return align16(l.slot_bytes); }
PE_HD long long offsets_offset(const Layout& l) { return meta_offset(l) + l.n_chunks * kMetaWords * 4; }
PE_HD long long workspace_bytes(const Layout& l) { return offsets_offset(l) + align16(l.n_chunks * 4); }

inline bool map_ok(const tt_png_map& m) {
  return m.data && m.H >= 1 && m.W >= 1 && m.H <= kMaxDim && m.W <= kMaxDim && m.pitch >= m.W && m.pitch <= (1ll << 40);
}

// Fills first_chunk, n_chunks and out_off of every map, and the chunk rows when `chunks` is given (chunk_capacity rows).  0 or
// TT_PNG_EARGUMENT.
inline int plan(tt_png_map* maps, int n_maps, tt_png_chunk* chunks, long long chunk_capacity, Layout* out) {
  if (!maps || !out || n_maps < 1 || n_maps > 65535) return TT_PNG_EARGUMENT;
  Layout l{0, 0};
  for (int i = 0; i < n_maps; ++i) {
    tt_png_map& m = maps[i];
    if (!map_ok(m)) return TT_PNG_EARGUMENT;
    const long long rpc = rows_per_chunk(m.H, m.W), nc = chunk_count(m.H, m.W);
    m.first_chunk = l.n_chunks;
    m.n_chunks = nc;
    m.out_off = l.slot_bytes;
    if (chunks) {
      if (l.n_chunks + nc > chunk_capacity) return TT_PNG_EARGUMENT;
      long long at = l.slot_bytes;
      for (long long c = 0; c < nc; ++c) {
        tt_png_chunk& k = chunks[l.n_chunks + c];
        k.map = i;
        k.row0 = c * rpc;
        k.rows = m.H - k.row0 < rpc ? m.H - k.row0 : rpc;
        k.slot_off = at;
        at += slot_stride(k.rows * (m.W + 1));
      }
    }
    l.n_chunks += nc;
    l.slot_bytes += file_capacity(m.H, m.W);
    if (l.slot_bytes > kMaxBatchBytes) return TT_PNG_EARGUMENT;
  }
  *out = l;
  return 0;
}

// The HOST tables against the plan and every buffer size: 0, or TT_PNG_EARGUMENT with the reason in *why.
inline int validate(const tt_png_map* maps, int n_maps, const tt_png_chunk* chunks, long long n_chunks, long long out_bytes, size_t ws_bytes,
                    Layout* out, const char** why) {
  *why = "a null table, or n_maps outside 1..65535";
  if (!maps || !chunks || n_maps < 1 || n_maps > 65535) return TT_PNG_EARGUMENT;
  Layout l{0, 0};
  for (int i = 0; i < n_maps; ++i) {
    const tt_png_map& m = maps[i];
    *why = "a map with a null pointer, a side outside 1..32767 or a pitch below W";
    if (!map_ok(m)) return TT_PNG_EARGUMENT;
    const long long rpc = rows_per_chunk(m.H, m.W), nc = chunk_count(m.H, m.W);
    *why = "a map row that is not the plan's (first_chunk, n_chunks, out_off)";
    if (m.first_chunk != l.n_chunks || m.n_chunks != nc || m.out_off != l.slot_bytes || l.n_chunks + nc > n_chunks) return TT_PNG_EARGUMENT;
    long long at = l.slot_bytes;
    *why = "a chunk row that is not the plan's (map, row0, rows, slot_off)";
    for (long long c = 0; c < nc; ++c) {
      const tt_png_chunk& k = chunks[l.n_chunks + c];
      const long long rows = m.H - c * rpc < rpc ? m.H - c * rpc : rpc;
      if (k.map != i || k.row0 != c * rpc || k.rows != rows || k.slot_off != at) return TT_PNG_EARGUMENT;
      at += slot_stride(rows * (m.W + 1));
    }
    l.n_chunks += nc;
    l.slot_bytes += file_capacity(m.H, m.W);
    *why = "more than 2^31 - 1 bytes of slots in one call";
    if (l.slot_bytes > kMaxBatchBytes) return TT_PNG_EARGUMENT;
  }
  *why = "n_chunks is not the plan's";
  if (l.n_chunks != n_chunks) return TT_PNG_EARGUMENT;
  *why = "an output below the capacity";
  if (out_bytes < l.slot_bytes) return TT_PNG_EARGUMENT;
  *why = "a workspace below tt_png_encode_batch_workspace_bytes";
  if (ws_bytes < (size_t)workspace_bytes(l)) return TT_PNG_EARGUMENT;
  *why = "";
  *out = l;
  return 0;
}

}  // namespace pe
}  // namespace tt
