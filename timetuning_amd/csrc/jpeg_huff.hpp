// N24: the Huffman layer of a baseline JPEG scan as a state step - shared by the kernels of jpeg_entropy.hip and by the host emulation
// tt_jpeg_entropy_host (jpeg_scan.cpp), which is what the CPU tests and the sanitizer program run.  No HIP include: with the host compiler
// alone the qualifiers are empty.  It is also the one home of what every JPEG source states alike: the code table (Table), kLook, kZigzag,
// extend and the block grid (grid) - the sequential parser of jpeg_scan.cpp and the kernels of jpeg.hip read them from here.
//
// The scheme (self-synchronising subsequence decode).  tt_jpeg_prepare has cut the scan into restart segments of clean bytes (no
// stuffing, no markers), each starting on a 4-byte boundary.  A segment is cut into subsequences of S bits; one lane owns one.  A decoder's
// state is (p, b, z, c): p the bit position of the next symbol inside the segment, b the block index inside the MCU (it selects the
// component and so the tables), z the zigzag index (0: a DC category is next), c the bits the SEQUENTIAL host reader (Bits in
// jpeg_scan.cpp) would hold in its accumulator at this point - it refills to 57 ... 64 bits whenever a symbol finds fewer than 16, and
// whether it has reached the restart marker when an interval's last block is done decides TT_JPEG_ERESTART, so c is part of the state.
//   round 0: lane i decodes from (i S, 0, 0, 0) - for the first subsequence of a segment that IS the true state - to p >= (i + 1) S.
//   rounds:  lane i takes lane i - 1's exit state as its entry state and decodes again if that changed; after round r the first r + 1
//            exit states are the sequential decoder's, so the fixed point is the true decode whatever the data, after at most as many
//            rounds as the tile has lanes.
//   count:   every pass counts the blocks it completes; a prefix sum gives each lane the index of its first block in the segment.
//   write:   one more pass from the true state writes the coefficients (the DC DIFFERENCE into blk[0]) and reports errors.
//   dc:      per component and restart segment an inclusive sum of the differences in scan order.
// Bounds.  step() consumes at least one bit (a code that no table holds skips one bit while speculating), so a pass runs at most
// S + 31 iterations; S >= 32 keeps one symbol (<= 31 bits) from jumping a subsequence.  Every read of the stream is checked against the
// segment's bit length (bits past it read as zero), every write against the segment's and the frame's block count.  Errors are reported
// by the write pass only, where the state is the true one.
#pragma once
#include <cstdint>
#include <cstdio>

#include "../../include/timetuning_hip.h"

#if defined(__HIPCC__)
#define JH_HD __host__ __device__ inline
#else
#define JH_HD inline
#endif

namespace tt {
namespace jh {

constexpr int kTile = 256;           // lanes of a workgroup = subsequences of a tile
constexpr int kLook = 9;             // bits of the Huffman look-ahead table
constexpr int kDht = 272;            // bytes of one shipped table: 16 counts, 256 values
constexpr int kHuffBytes = 6 * kDht; // DC, AC of component 0, 1, 2
constexpr int kMinSubseq = 128, kMaxSubseq = 4096;
constexpr long long kMaxDim = 65535;
constexpr uint32_t kMaxSegBits = 0x7fffffe0u;

constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
JH_HD int zigzag(int k) { return kZigzag[k & 63]; }

// The block grid of component `comp` (0 luma, else chroma, which is 1 x 1) of an H x W frame: ceil(H / (8 vmax)) v rows of
// ceil(W / (8 hmax)) h blocks.  THE statement of where tt_jpeg_scan places blocks; the chroma grid is the grid of MCUs.
struct Grid { long long rows, cols; };   // blocks
JH_HD Grid grid(long long H, long long W, int sampling, int comp) {
  const int hmax = sampling == TT_JPEG_444 ? 1 : 2, vmax = sampling == TT_JPEG_420 ? 2 : 1;
  const long long mx = (W + 8 * hmax - 1) / (8 * hmax), my = (H + 8 * vmax - 1) / (8 * vmax);
  return comp == 0 ? Grid{my * vmax, mx * hmax} : Grid{my, mx};
}

// A 9-bit look table, mincode / maxcode / valptr for longer codes.  1556 bytes.  The sequential parser (Huff in jpeg_scan.cpp) holds one
// per DHT table, the kernel six in LDS.
struct Table {
  uint16_t look[1 << kLook];   // (length << 8) | value, 0 = a longer code
  int32_t maxcode[18];         // -1 = no code of this length
  int32_t mincode[17];
  int32_t valptr[17];
  uint32_t limit[17];          // (maxcode + 1) left-aligned in 16 bits, carried over lengths without codes: non-decreasing
  uint8_t vals[256];
};

// From the DHT counts.  Takes ANY 16 bytes: nothing here indexes with them.
JH_HD void build_codes(Table& t, const uint8_t* counts) {
  int code = 0, k = 0;
  t.maxcode[0] = -1;
  t.mincode[0] = t.valptr[0] = 0;
  t.limit[0] = 0;
  for (int len = 1; len <= 16; ++len) {
    const int cnt = counts[len - 1];
    t.valptr[len] = k;
    t.mincode[len] = code;
    code += cnt;
    k += cnt;
    t.maxcode[len] = cnt ? code - 1 : -1;
    const uint32_t lim = (uint32_t)code << (16 - len);
    t.limit[len] = lim > t.limit[len - 1] ? lim : t.limit[len - 1];
    code <<= 1;
  }
  t.maxcode[17] = 0x7fffffff;
}
// entry v of the look table: what build_huff scatters, gathered (for a prefix code at most one length matches)
JH_HD uint16_t look_entry(const Table& t, int v) {
  for (int len = 1; len <= kLook; ++len) {
    const int code = v >> (kLook - len);
    if (t.maxcode[len] >= 0 && code <= t.maxcode[len] && code >= t.mincode[len])
      return (uint16_t)((len << 8) | t.vals[(t.valptr[len] + code - t.mincode[len]) & 255]);
  }
  return 0;
}
// one symbol from the 32 bits at the read position: its value and length, -1 = no table entry
JH_HD int symbol(const Table& t, uint32_t peek, int* len) {
  const uint16_t e = t.look[peek >> (32 - kLook)];
  if (e) {
    *len = e >> 8;
    return e & 0xff;
  }
  // The rare path for a lane, but not for a wave of 64: no loop, no branch.  A canonical code's left-aligned value grows with its
  // length, so the length is kLook + 1 + the number of limits at or below the 16 bits read; what the host's search over
  // mincode / maxcode finds for every table tt_jpeg_prepare lets through (build_huff has checked the counts).
  const uint32_t code16 = peek >> 16;
  int l = kLook + 1;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = kLook + 1; k < 16; ++k) l += code16 >= t.limit[k] ? 1 : 0;
  if (code16 >= t.limit[16]) return -1;
  *len = l;
  return t.vals[(t.valptr[l] + (int)(code16 >> (16 - l)) - t.mincode[l]) & 255];
}

JH_HD int extend(int v, int s) { return s && v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// What the passes need of a frame; all counts fit 32 bits (sides <= 65535).
struct Frame {
  uint32_t bpm, h0, v0;   // blocks per MCU, the luma factors
  uint32_t mx, mcus;
  uint32_t restart;       // MCUs per segment (all of them without DRI)
  uint32_t n_segments;
  long long coeff0, coeff1, coeff2;   // the components' first elements (no array: a lane keeps them in registers)
};
JH_HD Frame make_frame(const tt_jpeg_stream& s) {
  Frame f;
  f.h0 = s.sampling == TT_JPEG_444 ? 1 : 2;
  f.v0 = s.sampling == TT_JPEG_420 ? 2 : 1;
  f.bpm = f.h0 * f.v0 + 2;
  const Grid mcu = grid(s.H, s.W, (int)s.sampling, 1);
  f.mx = (uint32_t)mcu.cols;
  f.mcus = f.mx * (uint32_t)mcu.rows;
  f.restart = s.restart > 0 && s.restart < (long long)f.mcus ? (uint32_t)s.restart : f.mcus;
  f.n_segments = (f.mcus + f.restart - 1) / f.restart;
  f.coeff0 = s.coeff_off[0];
  f.coeff1 = s.coeff_off[1];
  f.coeff2 = s.coeff_off[2];
  return f;
}
JH_HD int comp_of_block(const Frame& f, uint32_t b) { return b < f.h0 * f.v0 ? 0 : (int)(b - f.h0 * f.v0 + 1); }
JH_HD uint32_t segment_blocks(const Frame& f, uint32_t seg) {
  const uint32_t first = seg * f.restart, left = f.mcus - first;
  return (left < f.restart ? left : f.restart) * f.bpm;
}
// element offset of block `w` (of component c) of MCU `mcu`, as tt_jpeg_scan places it; -1 past the frame
JH_HD long long block_at(const Frame& f, uint32_t mcu, int c, uint32_t w) {
  if (mcu >= f.mcus) return -1;
  const uint32_t hc = c ? 1 : f.h0, vc = c ? 1 : f.v0;
  const uint32_t y = w / hc, x = w % hc, my_i = mcu / f.mx, mx_i = mcu % f.mx;
  const long long base = c == 0 ? f.coeff0 : (c == 1 ? f.coeff1 : f.coeff2);
  return base + (((long long)my_i * vc + y) * ((long long)f.mx * hc) + ((long long)mx_i * hc + x)) * 64;
}
// ... of block n of segment seg in scan order
JH_HD long long block_offset(const Frame& f, uint32_t seg, uint32_t n) {
  const uint32_t mcu = seg * f.restart + n / f.bpm, b = n % f.bpm;
  const int c = comp_of_block(f, b);
  return block_at(f, mcu, c, c ? 0 : b);
}

struct State {
  uint32_t p;
  int b, z, c;
};
JH_HD uint32_t pack(const State& s) { return (uint32_t)s.b | ((uint32_t)s.z << 3) | ((uint32_t)s.c << 9); }
JH_HD State unpack(uint32_t p, uint32_t q) { return State{p, (int)(q & 7u), (int)((q >> 3) & 63u), (int)(q >> 9)}; }

// The bits of one segment: big-endian words of the clean stream, 64 bits ahead in a register.
struct Reader {
  const uint32_t* w;
  uint32_t nbits;
  uint64_t acc;   // left-aligned
  int avail;
  uint32_t next;
  JH_HD uint32_t word(uint32_t i) const {
    if (i >= ((nbits + 31u) >> 5)) return 0;
    uint32_t v = __builtin_bswap32(w[i]);
    const uint32_t keep = nbits - i * 32u;
    if (keep < 32u) v &= ~0u << (32u - keep);
    return v;
  }
  JH_HD void init(const uint32_t* words, uint32_t bits, uint32_t p) {
    w = words;
    nbits = bits;
    const uint32_t i = p >> 5, sh = p & 31u;
    acc = (((uint64_t)word(i) << 32) | word(i + 1)) << sh;
    avail = 64 - (int)sh;
    next = i + 2;
  }
  JH_HD uint32_t peek() {
    if (avail < 32) {
      acc |= (uint64_t)word(next) << (32 - avail);
      avail += 32;
      ++next;
    }
    return (uint32_t)(acc >> 32);
  }
  JH_HD void skip(int n) {
    acc <<= n;
    avail -= n;
  }
};

// the host reader's refill at consumed position p: whole bytes until it holds more than 56 bits, or the segment ends
JH_HD int host_fill(uint32_t p, uint32_t nbits) {
  const uint32_t upto = ((p + 57u + 7u) >> 3) << 3;
  return (int)((upto < nbits ? upto : nbits) - p);
}

// One symbol (and its value bits) from state s; s.p < rd.nbits.  Returns 1 when it completed a block.  *err gets the TT_JPEG_E* code
// of what the sequential decoder would report here; the state then moves on by the speculative rules (it must, to stay a function of
// the state alone).  blk: the block to write into, or null.  track: the segment is followed by a restart marker, so c matters; in a frame's
// last (or only) segment c stays 0 and costs no round.
template <bool WRITE>
JH_HD int step(const Table* tabs, const Frame& f, Reader& rd, State& s, int16_t* blk, int* err, bool track) {
  const bool dc = s.z == 0;
  const Table& t = tabs[2 * comp_of_block(f, (uint32_t)s.b) + (dc ? 0 : 1)];
  const uint32_t peek = rd.peek();
  uint32_t rem = rd.nbits - s.p;
  if (track && s.c < 16) s.c = host_fill(s.p, rd.nbits);
  int l = 0, sz = 0, run = 0;
  const int v = symbol(t, peek, &l);
  if (v < 0) {   // no such code: one bit on
    *err = rem < 16 ? TT_JPEG_ETRUNCATED : TT_JPEG_EHUFFMAN;
    rd.skip(1);
    s.p += 1;
    if (track) s.c -= 1;
    return 0;
  }
  if ((uint32_t)l > rem) {
    *err = TT_JPEG_ETRUNCATED;
    s.p = rd.nbits;
    s.c = 0;
    return 0;
  }
  rd.skip(l);
  s.p += (uint32_t)l;
  if (track) s.c -= l;
  rem -= (uint32_t)l;
  bool done = false;
  if (dc) {
    sz = v;
    if (sz > 11) {   // a DC category an 8-bit file cannot hold
      *err = TT_JPEG_EHUFFMAN;
      sz = 0;
    }
  } else {
    run = v >> 4;
    sz = v & 15;
    if (sz == 0) {
      if (run != 15) {
        done = true;   // EOB
      } else {         // ZRL
        const int k = s.z + 16;
        if (k > 64) *err = TT_JPEG_ERUN;
        if (k >= 64) {
          done = true;
        } else {
          s.z = k;
          return 0;
        }
      }
    } else if (s.z + run > 63) {
      *err = TT_JPEG_ERUN;
      done = true;
    }
  }
  if (!done) {
    int bits = 0;
    if (sz) {
      if (track && s.c < sz) s.c = host_fill(s.p, rd.nbits);
      if ((uint32_t)sz > rem) {
        *err = TT_JPEG_ETRUNCATED;
        s.p = rd.nbits;
        s.c = 0;
        return 0;
      }
      bits = (int)((peek << l) >> (32 - sz));   // l + sz <= 31
      rd.skip(sz);
      s.p += (uint32_t)sz;
      if (track) s.c -= sz;
    }
    const int val = extend(bits, sz);
    if (dc) {
      if (WRITE && blk) blk[0] = (int16_t)val;
      s.z = 1;
      return 0;
    }
    const int k = s.z + run;
    if (WRITE && blk) blk[zigzag(k)] = (int16_t)val;
    s.z = k + 1;
    if (s.z < 64) return 0;
  }
  s.z = 0;
  s.b = s.b + 1 == (int)f.bpm ? 0 : s.b + 1;
  return 1;
}

// Decodes from s to p >= end, leaves the exit state in s and returns the blocks completed.  At most end - s.p iterations.
JH_HD uint32_t run_count(const Table* tabs, const Frame& f, const uint32_t* words, uint32_t nbits, State& s, uint32_t end, uint32_t seg) {
  Reader rd;
  rd.init(words, nbits, s.p);
  uint32_t blocks = 0;
  int err = 0;
  const bool track = seg + 1 < f.n_segments;
  while (s.p < end) blocks += (uint32_t)step<false>(tabs, f, rd, s, nullptr, &err, track);
  return blocks;
}

// The write pass of one subsequence from its TRUE entry state; n: the index in the segment of the block it starts in.  Writes blocks
// n ... below the segment's count only.  Returns 0 or the error the sequential decoder reports.
JH_HD int run_write(const Table* tabs, const Frame& f, const uint32_t* words, uint32_t nbits, State s, uint32_t end, uint32_t seg, uint32_t n,
                    int16_t* coeffs) {
  const uint32_t nb_seg = segment_blocks(f, seg);
  if (n >= nb_seg) return 0;   // the segment's blocks are done: padding, or what follows an early end that its lane has reported
  Reader rd;
  rd.init(words, nbits, s.p);
  long long off = block_offset(f, seg, n);
  int16_t* blk = off >= 0 ? coeffs + off : nullptr;
  int err = 0;
  const bool track = seg + 1 < f.n_segments;
  while (s.p < end) {
    const int done = step<true>(tabs, f, rd, s, blk, &err, track);
    if (err) return err;
    if (done) {
      if (++n == nb_seg) {
        // the interval is over: the host reader takes the marker only if its refills have reached the segment's end
        if (track && s.p + (uint32_t)s.c != nbits) return TT_JPEG_ERESTART;
        return 0;
      }
      off = block_offset(f, seg, n);
      blk = off >= 0 ? coeffs + off : nullptr;
    }
  }
  return end == nbits ? TT_JPEG_ETRUNCATED : 0;   // the segment ended before its MCUs were done
}

JH_HD uint32_t subsequences(uint32_t bits, uint32_t S) { return bits ? (bits + S - 1) / S : 1u; }

// DC prediction of component c over the differences j0 ... j1 - 1 of its scan order.  dc_sum: the sum since the last restart in the
// range (*reset: there was one); dc_apply: the running prediction written back, entering with `carry`.  uint32 sums, truncated to int16
// where the host truncates.
JH_HD uint32_t dc_blocks(const Frame& f, int c) { return f.mcus * (c ? 1u : f.h0 * f.v0); }
JH_HD uint32_t dc_sum(const Frame& f, const int16_t* coeffs, int c, uint32_t j0, uint32_t j1, int* reset) {
  const uint32_t bpc = c ? 1u : f.h0 * f.v0, period = f.restart * bpc;
  uint32_t acc = 0;
  *reset = 0;
  for (uint32_t j = j0; j < j1; ++j) {
    if (j % period == 0) {
      acc = 0;
      *reset = 1;
    }
    const long long off = block_at(f, j / bpc, c, j % bpc);
    if (off >= 0) acc += (uint32_t)(int)coeffs[off];
  }
  return acc;
}
JH_HD void dc_apply(const Frame& f, int16_t* coeffs, int c, uint32_t j0, uint32_t j1, uint32_t carry) {
  const uint32_t bpc = c ? 1u : f.h0 * f.v0, period = f.restart * bpc;
  for (uint32_t j = j0; j < j1; ++j) {
    if (j % period == 0) carry = 0;
    const long long off = block_at(f, j / bpc, c, j % bpc);
    if (off < 0) continue;
    carry += (uint32_t)(int)coeffs[off];
    coeffs[off] = (int16_t)(int)carry;
  }
}

// The whole check of a call's HOST tables against its buffer sizes.  0, or -1 with the reason in msg.
inline int validate(long long scan_bytes, const uint32_t* segs, long long n_segs, const tt_jpeg_stream* table, int n_frames, int subseq_bits,
                    long long n_coeffs, char* msg, size_t msg_len) {
#define JH_FAIL(...)                        \
  do {                                      \
    std::snprintf(msg, msg_len, __VA_ARGS__); \
    return -1;                              \
  } while (0)
  if (!segs || !table || n_frames < 1 || n_frames > 65535 || scan_bytes < 0 || n_segs < 0 || n_coeffs < 0)
    JH_FAIL("jpeg_entropy: null table or bad count (%d frames)", n_frames);
  if (subseq_bits < kMinSubseq || subseq_bits > kMaxSubseq || subseq_bits % 32)
    JH_FAIL("jpeg_entropy: subseq_bits %d is not a multiple of 32 in [%d, %d]", subseq_bits, kMinSubseq, kMaxSubseq);
  for (int i = 0; i < n_frames; ++i) {
    const tt_jpeg_stream& s = table[i];
    if (s.H < 1 || s.W < 1 || s.H > kMaxDim || s.W > kMaxDim || s.sampling < TT_JPEG_444 || s.sampling > TT_JPEG_420 || s.restart < 0 ||
        s.restart > 65535)
      JH_FAIL("jpeg_entropy: frame %d is %lld x %lld, sampling %lld, restart %lld", i, (long long)s.H, (long long)s.W, (long long)s.sampling,
              (long long)s.restart);
    const Frame f = make_frame(s);
    if (s.n_segments != (long long)f.n_segments || s.seg_off < 0 || s.seg_off > n_segs || s.n_segments > n_segs - s.seg_off)
      JH_FAIL("jpeg_entropy: frame %d: %lld segments at row %lld of %lld, its shape has %u", i, (long long)s.n_segments, (long long)s.seg_off,
              n_segs, f.n_segments);
    if (s.scan_off < 0 || s.scan_off % 4 || s.scan_len < 0 || s.scan_off > scan_bytes || s.scan_len > scan_bytes - s.scan_off)
      JH_FAIL("jpeg_entropy: frame %d: %lld stream bytes at offset %lld do not lie 4-byte aligned inside the %lld given", i, (long long)s.scan_len,
              (long long)s.scan_off, scan_bytes);
    if (s.huff_off < 0 || s.huff_off % 4 || s.huff_off > scan_bytes || kHuffBytes > scan_bytes - s.huff_off)
      JH_FAIL("jpeg_entropy: frame %d: the Huffman tables at offset %lld do not lie inside the %lld bytes given", i, (long long)s.huff_off,
              scan_bytes);
    for (long long k = 0; k < s.n_segments; ++k) {
      const uint32_t start = segs[2 * (s.seg_off + k)], bits = segs[2 * (s.seg_off + k) + 1];
      if (start % 4 || bits > kMaxSegBits || (long long)start > s.scan_len || (long long)((bits + 31u) / 32u) * 4 > s.scan_len - (long long)start)
        JH_FAIL("jpeg_entropy: frame %d segment %lld: %u bits at byte %u do not lie inside the frame's %lld stream bytes", i, k, bits, start,
                (long long)s.scan_len);
    }
    for (int c = 0; c < 3; ++c) {
      const long long blocks = (long long)dc_blocks(f, c);
      if (s.coeff_off[c] < 0 || s.coeff_off[c] % 8 || s.coeff_off[c] > n_coeffs || blocks * 64 > n_coeffs - s.coeff_off[c])
        JH_FAIL("jpeg_entropy: frame %d component %d: %lld coefficients at offset %lld do not lie inside the %lld given", i, c, blocks * 64,
                (long long)s.coeff_off[c], n_coeffs);
    }
  }
#undef JH_FAIL
  return 0;
}

constexpr int kStatWords = 4;   // per frame in the workspace: rounds, tiles, subsequences, the first failing subsequence (or -1)
inline size_t workspace_bytes(int n_frames) { return n_frames < 1 ? 0 : ((size_t)n_frames * kStatWords * 4 + 255) / 256 * 256; }

}  // namespace jh
}  // namespace tt
