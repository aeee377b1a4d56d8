// N26: inflate (RFC 1951) and the PNG row filters as steps shared by the kernel of png_decode.hip and by the host emulation
// tt_png_decode_host (png_scan.cpp), which is what the CPU tests and the sanitizer program run.  No HIP include: with the host compiler
// alone the qualifiers are empty.
//
// The scheme.  One wave owns one file.  The symbol decode is serial: EVERY lane runs it on the same bits (uniform control flow, the table
// look-ups are LDS broadcasts), so no lane has to tell the others what it found.  The work around a symbol is split over the lanes of the
// context (Ctx::NL = 64 on the device and in tt_png_decode_host_wave, 64 host threads behind a barrier; 1 in tt_png_decode_host, which is
// therefore the plain sequential loop over the same code):
//   literals  lane (k mod NL) keeps the k-th pending literal in a register; NL of them, the next match or the end of the block store them
//             in one instruction, so that `pos` is the true position wherever a block begins.
//   matches   lane i copies bytes i, i + NL, ... from pos - dist + (i mod dist): right for dist < len down to dist = 1.
//   stored    lane i copies bytes i, i + NL, ... of the block out of the stream.
//   tables    counts, acceptance rules and the canonical symbol order on lane 0 (at most 320 symbols), the 512-entry look table of each
//             alphabet by all lanes (entry k: the canonical walk over the bits of k).
//   adler     lane i sums bytes i, i + NL, ... with their weights (n - index), the NL partial sums are combined in lane order.
// Bounds.  The loop tests the bits consumed against the stream's bit length before every symbol and a symbol consumes at least one bit, so
// the steps are bounded by the bit length; bits past the end read as zero.  Every write is checked against the file's expected byte
// count `expect` = H (1 + row_bytes), every back-reference against the bytes already written, every stored block against the stream's
// length.  The acceptance rules are zlib's (inflate_table): an over-subscribed set is refused, an incomplete one too unless it holds no
// code at all or a single code of one bit; a literal/length set without the end-of-block code is refused.
// The host is little-endian, as the device is: a 32-bit load of the stream yields its bytes LSB first.
#pragma once
#include <cstdint>
#include <cstdio>

#include "../../include/timetuning_hip.h"

#if defined(__HIPCC__)
#define PZ_HD __host__ __device__ inline
#else
#define PZ_HD inline
#endif

namespace tt {
namespace pz {

constexpr int kLanes = 64;           // lanes of the device context: one wave
constexpr int kLook = 9;             // bits of both look tables
constexpr int kStatWords = 8;        // int32 per file behind the workspace slices, see Stats
constexpr long long kMaxDim = 32767; // the limit of the ragged kernels that read the maps
constexpr uint32_t kAdlerMod = 65521u;

constexpr uint8_t kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
constexpr uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
constexpr uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
constexpr uint16_t kDistBase[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                    193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
constexpr uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

// What the decode of one file reports besides its status (the emulation and the kernel alike): the coverage counters of the tests.
struct Stats {
  int32_t kinds;      // bit t: a block of type t (0 stored, 1 fixed, 2 dynamic) was read
  int32_t lit_bits;   // the longest literal/length code used
  int32_t dist_bits;  // the longest distance code used
  int32_t min_dist, max_dist, max_len;
  int32_t filters;    // bit f: a row with filter f was unfiltered
  int32_t bytes;      // inflated bytes
};

// A canonical Huffman code: count[l] codes of l bits, their symbols in code order; look[k] = (symbol << 4) | length for the code that
// the low bits of k spell (first bit of the code = bit 0), 0 where the code is longer than kLook bits or k spells none.
struct Huff {
  uint16_t count[16];
  uint16_t offs[16];
  uint16_t symbol[288];
  uint16_t look[1 << kLook];
};

// What the lanes of one file share: LDS on the device.
struct Work {
  Huff lit, dist;
  uint8_t lens[320];   // 288 + 32: the fixed code's lengths are the longest list
  int32_t err;
  uint32_t sa[kLanes], sb[kLanes];
};

struct Bits {
  const uint32_t* words;
  uint32_t n_words, tail_mask;
  uint64_t nbits;
  uint64_t buf;
  int cnt;
  uint32_t next;
};

PZ_HD uint32_t word(const Bits& b, uint32_t i) {
  if (i >= b.n_words) return 0u;
  const uint32_t w = b.words[i];
  return i + 1 == b.n_words ? w & b.tail_mask : w;
}
PZ_HD void refill(Bits& b) {
  if (b.cnt <= 32) {
    b.buf |= (uint64_t)word(b, b.next) << b.cnt;
    b.cnt += 32;
    ++b.next;
  }
}
PZ_HD void drop(Bits& b, int n) {
  b.buf >>= n;
  b.cnt -= n;
}
PZ_HD uint32_t peek(Bits& b, int n) {   // n <= 16
  refill(b);
  return (uint32_t)b.buf & ((1u << n) - 1u);
}
PZ_HD uint32_t take(Bits& b, int n) {
  const uint32_t v = peek(b, n);
  drop(b, n);
  return v;
}
PZ_HD uint64_t used(const Bits& b) { return (uint64_t)b.next * 32u - (uint64_t)b.cnt; }
PZ_HD void seek(Bits& b, uint64_t bitpos) {
  b.next = (uint32_t)(bitpos >> 5);
  b.buf = 0;
  b.cnt = 0;
  refill(b);
  drop(b, (int)(bitpos & 31u));
}
PZ_HD void open(Bits& b, const uint32_t* words, uint64_t len_bytes) {
  b.words = words;
  b.n_words = (uint32_t)((len_bytes + 3) / 4);
  b.tail_mask = (len_bytes & 3u) ? (1u << (8 * (unsigned)(len_bytes & 3u))) - 1u : 0xffffffffu;
  b.nbits = 8 * len_bytes;
  seek(b, 0);
}

// The canonical walk over at most `maxlen` bits of `bits` (first bit of the code = bit 0): the symbol, or -1.
PZ_HD int walk(const Huff& h, uint32_t bits, int maxlen, int* len_out) {
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= maxlen; ++len) {
    code |= (int)(bits & 1u);
    bits >>= 1;
    const int count = h.count[len];
    if (code - count < first) {
      *len_out = len;
      return h.symbol[index + (code - first)];
    }
    index += count;
    first += count;
    first <<= 1;
    code <<= 1;
  }
  return -1;
}

PZ_HD int decode(const Huff& h, Bits& b, int* len_out) {
  const uint32_t v = peek(b, 15);
  const uint32_t e = h.look[v & ((1u << kLook) - 1u)];
  int len = (int)(e & 15u), sym = (int)(e >> 4);
  if (e == 0) {
    sym = walk(h, v, 15, &len);
    if (sym < 0) return -1;
  }
  drop(b, len);
  *len_out = len;
  return sym;
}

// kind: 0 the code-length code, 1 literal/length, 2 distance.  0 or TT_PNG_EHUFFMAN, the same in every lane.
template <class Ctx>
PZ_HD int build(Ctx& c, Work& w, Huff& h, const uint8_t* lens, int n, int kind) {
  if (c.lane == 0) {
    int err = 0, left = 1, maxl = 0;
    for (int l = 0; l < 16; ++l) h.count[l] = 0;
    for (int s = 0; s < n; ++s) ++h.count[lens[s] & 15];
    h.count[0] = 0;
    for (int l = 1; l < 16; ++l) {
      left <<= 1;
      left -= h.count[l];
      if (left < 0) {
        err = TT_PNG_EHUFFMAN;   // over-subscribed
        break;
      }
      if (h.count[l]) maxl = l;
    }
    if (!err && maxl == 0 && kind == 0) err = TT_PNG_EHUFFMAN;
    if (!err && maxl != 0 && left > 0 && (kind == 0 || maxl != 1)) err = TT_PNG_EHUFFMAN;   // incomplete
    if (err) {
      for (int l = 0; l < 16; ++l) h.count[l] = 0;
    } else {
      h.offs[1] = 0;
      for (int l = 1; l < 15; ++l) h.offs[l + 1] = (uint16_t)(h.offs[l] + h.count[l]);
      for (int s = 0; s < n; ++s)
        if (lens[s] & 15) h.symbol[h.offs[lens[s] & 15]++] = (uint16_t)s;
    }
    w.err = err;
  }
  c.sync();
  const int err = w.err;
  for (int k = c.lane; k < (1 << kLook); k += Ctx::NL) {
    int len = 0;
    const int sym = walk(h, (uint32_t)k, kLook, &len);
    h.look[k] = sym < 0 ? (uint16_t)0 : (uint16_t)((sym << 4) | len);
  }
  c.sync();
  return err;
}

// Inflates the stream of `len_bytes` bytes at `words` (4-byte aligned) into out[0 .. expect) and checks the Adler-32 behind the final
// block.  0 or the first error, the same in every lane.
template <class Ctx>
PZ_HD int inflate(Ctx& c, Work& w, const uint32_t* words, uint64_t len_bytes, uint8_t* out, uint64_t expect, Stats& st) {
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(words);
  Bits b;
  open(b, words, len_bytes);
  uint64_t pos = 0;
  int npend = 0;
  uint8_t mylit = 0;
  st.min_dist = 0x7fffffff;
  for (;;) {
    if (used(b) + 3 > b.nbits) return TT_PNG_ETRUNCATED;
    const uint32_t hdr = take(b, 3);
    const int type = (int)(hdr >> 1);
    if (type == 3) return TT_PNG_EMALFORMED;
    st.kinds |= 1 << type;
    if (type == 0) {
      drop(b, b.cnt & 7);   // the words are whole bytes, so the bits held and the bits used are congruent modulo 8
      if (used(b) + 32 > b.nbits) return TT_PNG_ETRUNCATED;
      const uint32_t len = take(b, 16), nlen = take(b, 16);
      if ((len ^ 0xffffu) != nlen) return TT_PNG_EMALFORMED;
      const uint64_t at = used(b) >> 3;
      if (at + len > len_bytes) return TT_PNG_ETRUNCATED;
      if (len > expect - pos) return TT_PNG_EOVERRUN;
      for (uint32_t i = (uint32_t)c.lane; i < len; i += Ctx::NL) out[pos + i] = bytes[at + i];
      pos += len;
      seek(b, (at + len) * 8);
    } else {
      int nlit = 288, ndist = 32;
      if (type == 1) {
        for (int s = c.lane; s < 320; s += Ctx::NL) w.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
        c.sync();
      } else {
        if (used(b) + 14 > b.nbits) return TT_PNG_ETRUNCATED;
        nlit = (int)take(b, 5) + 257;
        ndist = (int)take(b, 5) + 1;
        const int ncode = (int)take(b, 4) + 4;
        if (nlit > 286 || ndist > 30) return TT_PNG_EHUFFMAN;
        for (int i = 0; i < 19; ++i) {
          const uint32_t v = i < ncode ? take(b, 3) : 0u;
          if (c.lane == 0) w.lens[kOrder[i]] = (uint8_t)v;
        }
        if (used(b) > b.nbits) return TT_PNG_ETRUNCATED;
        c.sync();
        if (build(c, w, w.lit, w.lens, 19, 0)) return TT_PNG_EHUFFMAN;
        const int total = nlit + ndist;
        int idx = 0, prev = 0;
        while (idx < total) {
          if (used(b) > b.nbits) return TT_PNG_ETRUNCATED;
          int l;
          const int sym = decode(w.lit, b, &l);
          if (sym < 0) return TT_PNG_EHUFFMAN;
          if (sym < 16) {
            if (c.lane == 0) w.lens[idx] = (uint8_t)sym;
            ++idx;
            prev = sym;
          } else {
            int rep, val = 0;
            if (sym == 16) {
              if (idx == 0) return TT_PNG_EHUFFMAN;
              val = prev;
              rep = 3 + (int)take(b, 2);
            } else if (sym == 17) {
              rep = 3 + (int)take(b, 3);
            } else {
              rep = 11 + (int)take(b, 7);
            }
            if (idx + rep > total) return TT_PNG_EHUFFMAN;
            if (c.lane == 0)
              for (int k = 0; k < rep; ++k) w.lens[idx + k] = (uint8_t)val;
            idx += rep;
            prev = val;
          }
        }
        if (used(b) > b.nbits) return TT_PNG_ETRUNCATED;
        c.sync();
        if (w.lens[256] == 0) return TT_PNG_EHUFFMAN;   // no end-of-block code
      }
      if (build(c, w, w.lit, w.lens, nlit, 1)) return TT_PNG_EHUFFMAN;
      if (build(c, w, w.dist, w.lens + nlit, ndist, 2)) return TT_PNG_EHUFFMAN;
      for (;;) {
        if (used(b) > b.nbits) return TT_PNG_ETRUNCATED;
        int l;
        int sym = decode(w.lit, b, &l);
        if (sym < 0) return TT_PNG_EHUFFMAN;
        if (l > st.lit_bits) st.lit_bits = l;
        if (sym < 256) {
          if (pos + (uint64_t)npend >= expect) return TT_PNG_EOVERRUN;
          if (npend % Ctx::NL == c.lane) mylit = (uint8_t)sym;
          if (++npend == Ctx::NL) {
            out[pos + (uint64_t)c.lane] = mylit;
            pos += (uint64_t)npend;
            npend = 0;
          }
          continue;
        }
        if (sym == 256) {   // the pending literals do not outlive their block: the next one may be stored, and copies at pos
          if (c.lane < npend) out[pos + (uint64_t)c.lane] = mylit;
          pos += (uint64_t)npend;
          npend = 0;
          break;
        }
        if (sym >= 286) return TT_PNG_EHUFFMAN;
        sym -= 257;
        const uint32_t length = kLenBase[sym] + take(b, kLenExtra[sym]);
        const int ds = decode(w.dist, b, &l);
        if (ds < 0 || ds >= 30) return TT_PNG_EHUFFMAN;
        if (l > st.dist_bits) st.dist_bits = l;
        const uint32_t dist = kDistBase[ds] + take(b, kDistExtra[ds]);
        if (used(b) > b.nbits) return TT_PNG_ETRUNCATED;
        if (c.lane < npend) out[pos + (uint64_t)c.lane] = mylit;
        pos += (uint64_t)npend;
        npend = 0;
        if (dist > pos) return TT_PNG_EDISTANCE;
        if (length > expect - pos) return TT_PNG_EOVERRUN;
        c.sync();   // the bytes the match reads were written by other lanes
        for (uint32_t i = (uint32_t)c.lane; i < length; i += Ctx::NL) out[pos + i] = out[pos - dist + (dist >= length ? i : i % dist)];
        pos += length;
        if ((int32_t)dist < st.min_dist) st.min_dist = (int32_t)dist;
        if ((int32_t)dist > st.max_dist) st.max_dist = (int32_t)dist;
        if ((int32_t)length > st.max_len) st.max_len = (int32_t)length;
      }
    }
    if (hdr & 1u) break;
  }
  st.bytes = (int32_t)pos;   // (npend is 0: every Huffman block stored its literals at its end)
  if (used(b) > b.nbits) return TT_PNG_ETRUNCATED;
  if (pos != expect) return TT_PNG_ETRUNCATED;
  drop(b, b.cnt & 7);
  if (used(b) + 32 > b.nbits) return TT_PNG_ETRUNCATED;
  uint32_t want = 0;
  for (int k = 0; k < 4; ++k) want = (want << 8) | take(b, 8);
  c.sync();
  // Adler-32: A = 1 + sum d_i, B = n + sum (n - i) d_i (mod 65521); lane-wise partial sums, combined in lane order
  uint64_t sa = 0, sb = 0;
  for (uint64_t i = (uint64_t)c.lane; i < pos; i += Ctx::NL) {
    const uint32_t d = out[i];
    sa += d;
    sb += (uint64_t)((uint32_t)(pos - i) % kAdlerMod) * d;
  }
  w.sa[c.lane] = (uint32_t)(sa % kAdlerMod);
  w.sb[c.lane] = (uint32_t)(sb % kAdlerMod);
  c.sync();
  uint32_t A = 1, B = (uint32_t)(pos % kAdlerMod);
  for (int k = 0; k < Ctx::NL; ++k) {
    A = (A + w.sa[k]) % kAdlerMod;
    B = (B + w.sb[k]) % kAdlerMod;
  }
  c.sync();
  return ((B << 16) | A) == want ? 0 : TT_PNG_ECHECKSUM;
}

// ---- the row filters at one byte per pixel group (bpp = 1: every supported format)
PZ_HD uint8_t unfilter(int ft, uint8_t x, uint8_t a, uint8_t b, uint8_t cc) {
  int add = 0;
  if (ft == 1) {
    add = a;
  } else if (ft == 2) {
    add = b;
  } else if (ft == 3) {
    add = ((int)a + (int)b) >> 1;
  } else if (ft == 4) {
    const int p = (int)a + (int)b - (int)cc;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > cc ? p - cc : cc - p;
    add = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : cc);
  }
  return (uint8_t)(x + add);
}

// The pixels of byte `col` of a row at `depth` bits (1, 2, 4, 8), MSB first, into row_out[0 .. W).
PZ_HD void unpack(uint8_t byte, int depth, long long col, long long W, uint8_t* row_out) {
  if (depth == 8) {
    row_out[col] = byte;
    return;
  }
  const int ppb = 8 / depth, mask = (1 << depth) - 1;
  for (int k = 0; k < ppb; ++k) {
    const long long x = col * ppb + k;
    if (x < W) row_out[x] = (uint8_t)((byte >> (8 - depth * (k + 1))) & mask);
  }
}

// The sequential form of the unfilter (the emulation): raw = H rows of 1 + rb bytes, unfiltered in place; out = H x W pixels.
inline int unfilter_rows(uint8_t* raw, long long H, long long W, long long rb, int depth, uint8_t* out, Stats& st) {
  for (long long r = 0; r < H; ++r)
    if (raw[r * (1 + rb)] > 4) return TT_PNG_EFILTER;
  for (long long r = 0; r < H; ++r) {
    uint8_t* row = raw + r * (1 + rb) + 1;
    const uint8_t* up = r ? row - (1 + rb) : nullptr;
    const int ft = row[-1];
    st.filters |= 1 << ft;
    for (long long x = 0; x < rb; ++x) {
      row[x] = unfilter(ft, row[x], x ? row[x - 1] : (uint8_t)0, up ? up[x] : (uint8_t)0, (up && x) ? up[x - 1] : (uint8_t)0);
      unpack(row[x], depth, x, W, out + r * W);
    }
  }
  return 0;
}

PZ_HD long long slice_bytes(const tt_png_stream& r) { return r.H * (1 + r.row_bytes); }
PZ_HD long long align16(long long v) { return (v + 15) / 16 * 16; }

// Is the row a file this build decodes, with consistent numbers?
inline bool row_ok(const tt_png_stream& r) {
  if (r.H < 1 || r.W < 1 || r.H > kMaxDim || r.W > kMaxDim) return false;
  if (r.color_type == 3 ? !(r.depth == 1 || r.depth == 2 || r.depth == 4 || r.depth == 8) : !(r.color_type == 0 && r.depth == 8)) return false;
  return r.row_bytes == (r.W * r.depth + 7) / 8;
}

// Bytes of the workspace slices (rounded to 16), 0 for a bad table; the statistics lie behind them.
inline long long slices_end(const tt_png_stream* table, int n) {
  if (!table || n < 1) return 0;
  long long end = 0;
  for (int i = 0; i < n; ++i) {
    if (!row_ok(table[i]) || table[i].ws_off < 0 || table[i].ws_off > (1ll << 40)) return 0;
    const long long e = table[i].ws_off + slice_bytes(table[i]);
    if (e > end) end = e;
  }
  return align16(end);
}
inline size_t workspace_bytes(const tt_png_stream* table, int n) {
  const long long end = slices_end(table, n);
  return end ? (size_t)end + (size_t)n * kStatWords * 4 : 0;
}

// The HOST table against every buffer size: 0, or -1 with the reason in msg.
inline int validate(long long stream_bytes, const tt_png_stream* t, int n, long long out_bytes, size_t ws_bytes, char* msg, size_t msg_len) {
  if (n < 1 || n > 65535 || stream_bytes < 0 || out_bytes < 0) {
    std::snprintf(msg, msg_len, "png_decode_batch: n_files %d, stream_bytes %lld, out_bytes %lld", n, stream_bytes, out_bytes);
    return -1;
  }
  for (int i = 0; i < n; ++i) {
    const tt_png_stream& r = t[i];
    if (!row_ok(r)) {
      std::snprintf(msg, msg_len, "png_decode_batch: file %d is not a supported map (%lld x %lld, depth %lld, colour type %lld, row bytes %lld)", i,
                    (long long)r.H, (long long)r.W, (long long)r.depth, (long long)r.color_type, (long long)r.row_bytes);
      return -1;
    }
    if (r.stream_off < 0 || (r.stream_off & 3) || r.stream_len < 0 || r.stream_len > 0x7ffffff0ll || r.stream_off > stream_bytes ||
        (r.stream_len + 3) / 4 * 4 > stream_bytes - r.stream_off) {
      std::snprintf(msg, msg_len, "png_decode_batch: file %d: stream at %lld of %lld bytes (4-byte aligned, inside %lld bytes)", i,
                    (long long)r.stream_off, (long long)r.stream_len, stream_bytes);
      return -1;
    }
    if (r.out_off < 0 || r.out_off > out_bytes || r.H * r.W > out_bytes - r.out_off) {
      std::snprintf(msg, msg_len, "png_decode_batch: file %d: output at %lld of %lld bytes outside %lld bytes", i, (long long)r.out_off,
                    (long long)(r.H * r.W), out_bytes);
      return -1;
    }
    if (r.ws_off < 0 || r.ws_off > (1ll << 40)) {
      std::snprintf(msg, msg_len, "png_decode_batch: file %d: workspace offset %lld", i, (long long)r.ws_off);
      return -1;
    }
  }
  const size_t need = workspace_bytes(t, n);
  if (need == 0 || ws_bytes < need) {
    std::snprintf(msg, msg_len, "png_decode_batch: a workspace of %zu bytes, %zu needed", ws_bytes, need);
    return -1;
  }
  // overlaps of the outputs and of the workspace slices: a batch is small, the quadratic check is a few thousand comparisons
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      if (t[i].out_off < t[j].out_off + t[j].H * t[j].W && t[j].out_off < t[i].out_off + t[i].H * t[i].W) {
        std::snprintf(msg, msg_len, "png_decode_batch: the outputs of files %d and %d overlap", i, j);
        return -1;
      }
      if (t[i].ws_off < t[j].ws_off + slice_bytes(t[j]) && t[j].ws_off < t[i].ws_off + slice_bytes(t[i])) {
        std::snprintf(msg, msg_len, "png_decode_batch: the workspace slices of files %d and %d overlap", i, j);
        return -1;
      }
    }
  return 0;
}

}  // namespace pz
}  // namespace tt
