// N21, host half: marker parsing and Huffman decoding of baseline JPEG files - what is serial by nature.  tt_jpeg_probe classifies a
// file, tt_jpeg_scan writes its quantised DCT coefficients (de-zigzagged, int16, 64 per block, per component in block-grid raster order)
// and the quantisation table of each component; dequantisation, IDCT, up-sampling and colour run on the device (jpeg.hip).
//
// Plain C++17 with no HIP include: the file also compiles with the host compiler alone (tools/jpeg_scan_check.cpp builds it under
// AddressSanitizer).  Both entries are pure functions: no state, no allocation (the tables live on the stack, about 13 KB), no GPU call, so
// a thread pool may run them side by side.  EVERY read is checked against the buffer's length and every write against the caller's
// capacity; a file is data from outside.
//
// Supported: SOF0 and 8-bit SOF1 (Huffman), three components, luma 1x1 / 2x1 / 2x2 over chroma 1x1, DRI / RSTn, any number of DQT / DHT
// segments, one interleaved scan, YCbCr colour.  Everything else that is a well-formed JPEG file is "unsupported" (a positive status: the
// caller falls back), never an error; a broken file is a negative status.
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/timetuning_hip.h"
#include "jpeg_huff.hpp"

namespace {

namespace jh = tt::jh;
using jh::kLook;
using jh::kZigzag;

// What the parser keeps of a DHT table beyond the code table the device decode shares
struct Huff {
  bool present = false;
  uint8_t counts[16];           // the DHT segment's own bytes, for tt_jpeg_prepare
  int nvals = 0;
  jh::Table t;
};

struct Header {
  int H = 0, W = 0, sampling = -1;
  int h[3], v[3], tq[3], td[3], ta[3];
  uint8_t id[3];
  bool has_q[4] = {false, false, false, false};
  uint16_t q[4][64];            // natural order
  Huff dc[4], ac[4];
  int restart = 0;
  size_t scan_pos = 0;          // first entropy-coded byte
};

inline int rd16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// false: the counts do not describe a prefix code
bool build_huff(Huff& h, const uint8_t* bits, const uint8_t* vals, int n) {
  for (int len = 1, code = 0; len <= 16; ++len, code <<= 1)
    if ((code += bits[len - 1]) > (1 << len)) return false;
  std::memcpy(h.counts, bits, 16);
  h.nvals = n;
  jh::Table& t = h.t;
  std::memcpy(t.vals, vals, (size_t)n);
  jh::build_codes(t, bits);
  // the look table by scatter (jh::look_entry gathers the same entries, at several compares per entry, and every file is parsed
  // twice): a code of len bits owns the 2^(kLook - len) entries it is a prefix of, which the check above keeps inside the table
  std::memset(t.look, 0, sizeof(t.look));
  for (int len = 1; len <= kLook; ++len)
    for (int code = t.mincode[len]; code <= t.maxcode[len]; ++code) {
      const uint16_t e = (uint16_t)((len << 8) | t.vals[t.valptr[len] + code - t.mincode[len]]);
      for (int j = 0; j < (1 << (kLook - len)); ++j) t.look[(code << (kLook - len)) + j] = e;
    }
  h.present = true;
  return true;
}

// Walks the segments up to and including SOS.  0 supported, > 0 unsupported, < 0 malformed.
int parse_header(const uint8_t* d, size_t len, Header& hd) {
  if (!d || len < 4 || d[0] != 0xFF || d[1] != 0xD8) return TT_JPEG_EMALFORMED;
  size_t pos = 2;
  bool have_sof = false, jfif = false, adobe = false;
  int adobe_transform = -1, unsupported = 0;
  for (;;) {
    if (pos + 2 > len || d[pos] != 0xFF) return TT_JPEG_EMALFORMED;
    while (pos + 1 < len && d[pos + 1] == 0xFF) ++pos;   // fill bytes
    if (pos + 2 > len) return TT_JPEG_EMALFORMED;
    const int m = d[pos + 1];
    pos += 2;
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // TEM / a stray RSTn: no payload
    if (m == 0xD8 || m == 0xD9 || m == 0x00) return TT_JPEG_EMALFORMED;   // SOI again, EOI before a scan, a stuffed byte
    if (pos + 2 > len) return TT_JPEG_EMALFORMED;
    const int seglen = rd16(d + pos);
    if (seglen < 2 || pos + (size_t)seglen > len) return TT_JPEG_EMALFORMED;
    const uint8_t* s = d + pos + 2;
    const int n = seglen - 2;
    pos += (size_t)seglen;
    if (m == 0xDB) {   // DQT
      int i = 0;
      while (i < n) {
        const int pq = s[i] >> 4, tq = s[i] & 15;
        if (tq > 3 || pq > 1) return TT_JPEG_EMALFORMED;
        if (pq == 1) {   // 16-bit entries: well-formed, not taken
          if (i + 129 > n) return TT_JPEG_EMALFORMED;
          if (!unsupported) unsupported = TT_JPEG_UNSUPPORTED_QTABLE;
          i += 129;
          continue;
        }
        if (i + 65 > n) return TT_JPEG_EMALFORMED;
        for (int k = 0; k < 64; ++k) hd.q[tq][kZigzag[k]] = s[i + 1 + k];
        hd.has_q[tq] = true;
        i += 65;
      }
    } else if (m == 0xC4) {   // DHT
      int i = 0;
      while (i < n) {
        if (i + 17 > n) return TT_JPEG_EMALFORMED;
        const int tc = s[i] >> 4, th = s[i] & 15;
        if (tc > 1 || th > 3) return TT_JPEG_EMALFORMED;
        int total = 0;
        for (int k = 0; k < 16; ++k) total += s[i + 1 + k];
        if (total > 256 || i + 17 + total > n) return TT_JPEG_EMALFORMED;
        if (!build_huff(tc ? hd.ac[th] : hd.dc[th], s + i + 1, s + i + 17, total)) return TT_JPEG_EMALFORMED;
        i += 17 + total;
      }
    } else if (m == 0xC0 || m == 0xC1) {   // SOF0 / SOF1
      if (have_sof || n < 6) return TT_JPEG_EMALFORMED;
      have_sof = true;
      const int prec = s[0], nc = s[5];
      hd.H = rd16(s + 1);
      hd.W = rd16(s + 3);
      if (n != 6 + 3 * nc || hd.W == 0) return TT_JPEG_EMALFORMED;
      if (prec != 8) {
        if (prec != 12 || m != 0xC1) return TT_JPEG_EMALFORMED;
        if (!unsupported) unsupported = TT_JPEG_UNSUPPORTED_PRECISION;
      }
      if (hd.H == 0 && !unsupported) unsupported = TT_JPEG_UNSUPPORTED_FRAME;   // the height comes in a DNL segment
      if (nc != 3) {
        if (nc < 1 || nc > 4) return TT_JPEG_EMALFORMED;
        if (!unsupported) unsupported = TT_JPEG_UNSUPPORTED_COMPONENTS;
      } else {
        for (int c = 0; c < 3; ++c) {
          hd.id[c] = s[6 + 3 * c];
          hd.h[c] = s[7 + 3 * c] >> 4;
          hd.v[c] = s[7 + 3 * c] & 15;
          hd.tq[c] = s[8 + 3 * c];
          if (hd.h[c] < 1 || hd.h[c] > 4 || hd.v[c] < 1 || hd.v[c] > 4 || hd.tq[c] > 3) return TT_JPEG_EMALFORMED;
        }
        const bool chroma11 = hd.h[1] == 1 && hd.v[1] == 1 && hd.h[2] == 1 && hd.v[2] == 1;
        if (chroma11 && hd.h[0] == 1 && hd.v[0] == 1)
          hd.sampling = TT_JPEG_444;
        else if (chroma11 && hd.h[0] == 2 && hd.v[0] == 1)
          hd.sampling = TT_JPEG_422;
        else if (chroma11 && hd.h[0] == 2 && hd.v[0] == 2)
          hd.sampling = TT_JPEG_420;
        else if (!unsupported)
          unsupported = TT_JPEG_UNSUPPORTED_SAMPLING;
      }
    } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8) {   // the other frame types (0xC4 was taken above); 0xCC = DAC
      if (m == 0xCC || m >= 0xC9) {
        if (!unsupported) unsupported = TT_JPEG_UNSUPPORTED_ARITHMETIC;
      } else if (!unsupported) {
        unsupported = TT_JPEG_UNSUPPORTED_FRAME;   // progressive, lossless, hierarchical
      }
      if (m != 0xCC) {
        if (have_sof) return TT_JPEG_EMALFORMED;
        have_sof = true;
      }
    } else if (m == 0xDD) {   // DRI
      if (n != 2) return TT_JPEG_EMALFORMED;
      hd.restart = rd16(s);
    } else if (m == 0xE0) {
      if (n >= 5 && std::memcmp(s, "JFIF", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (n >= 12 && std::memcmp(s, "Adobe", 5) == 0) {
        adobe = true;
        adobe_transform = s[11];
      }
    } else if (m == 0xDA) {   // SOS
      if (!have_sof) return TT_JPEG_EMALFORMED;
      if (unsupported) return unsupported;
      if (n < 1) return TT_JPEG_EMALFORMED;
      const int ns = s[0];
      if (ns < 1 || ns > 4 || n != 4 + 2 * ns) return TT_JPEG_EMALFORMED;
      if (ns != 3) return TT_JPEG_UNSUPPORTED_SCANS;   // one component per scan
      for (int c = 0; c < 3; ++c) {
        if (s[1 + 2 * c] != hd.id[c]) return TT_JPEG_UNSUPPORTED_SCANS;
        hd.td[c] = s[2 + 2 * c] >> 4;
        hd.ta[c] = s[2 + 2 * c] & 15;
        if (hd.td[c] > 3 || hd.ta[c] > 3) return TT_JPEG_EMALFORMED;
        if (!hd.dc[hd.td[c]].present || !hd.ac[hd.ta[c]].present || !hd.has_q[hd.tq[c]]) return TT_JPEG_EMALFORMED;
      }
      if (s[7] != 0 || s[8] != 63 || s[9] != 0) return TT_JPEG_EMALFORMED;   // spectral selection / approximation of a sequential scan
      // colour: libjpeg's rule.  JFIF says YCbCr; an Adobe segment says what its transform byte says; otherwise the component ids decide
      if (jfif) {
      } else if (adobe) {
        if (adobe_transform != 1) return TT_JPEG_UNSUPPORTED_COLOUR;
      } else if (hd.id[0] == 'R' && hd.id[1] == 'G' && hd.id[2] == 'B') {
        return TT_JPEG_UNSUPPORTED_COLOUR;
      }
      hd.scan_pos = pos;
      return TT_JPEG_OK;
    }
    // APPn, COM and anything else with a length: skipped
  }
}

// of a supported header: its sampling code says what h[] and v[] say
inline jh::Grid grid(const Header& hd, int c) { return jh::grid(hd.H, hd.W, hd.sampling, c); }

// int16 elements of the frame's coefficients; base[c]: where component c's begin
inline long long coeff_layout(const Header& hd, long long* base) {
  long long total = 0;
  for (int c = 0; c < 3; ++c) {
    const jh::Grid g = grid(hd, c);
    if (base) base[c] = total;
    total += g.rows * g.cols * 64;
  }
  return total;
}

struct Bits {
  const uint8_t* d;
  size_t pos, len;
  uint64_t acc = 0;   // left-aligned
  int cnt = 0;
  bool stop = false;  // a marker or the end of the buffer is next

  void fill() {
    while (cnt <= 56 && !stop) {
      if (pos >= len) {
        stop = true;
        break;
      }
      uint8_t b = d[pos];
      if (b == 0xFF) {
        if (pos + 1 >= len) {
          stop = true;
          break;
        }
        const uint8_t b2 = d[pos + 1];
        if (b2 == 0x00) {
          pos += 2;
        } else if (b2 == 0xFF) {   // a fill byte in front of a marker
          pos += 1;
          continue;
        } else {
          stop = true;
          break;
        }
      } else {
        pos += 1;
      }
      acc |= (uint64_t)b << (56 - cnt);
      cnt += 8;
    }
  }
  // n <= 16.  false: the data ended
  bool get(int n, int* out) {
    if (n == 0) {
      *out = 0;
      return true;
    }
    if (cnt < n) {
      fill();
      if (cnt < n) return false;
    }
    *out = (int)(acc >> (64 - n));
    acc <<= n;
    cnt -= n;
    return true;
  }
  // one Huffman symbol.  0 ok, TT_JPEG_ETRUNCATED, TT_JPEG_EHUFFMAN
  int symbol(const jh::Table& t, int* out) {
    if (cnt < 16) fill();
    const unsigned peek = (unsigned)(acc >> (64 - kLook));
    const uint16_t e = t.look[peek];
    if (e) {
      const int l = e >> 8;
      if (l > cnt) return TT_JPEG_ETRUNCATED;
      acc <<= l;
      cnt -= l;
      *out = e & 0xff;
      return 0;
    }
    const int code16 = (int)(acc >> 48);
    for (int l = kLook + 1; l <= 16; ++l) {
      const int code = code16 >> (16 - l);
      if (t.maxcode[l] >= 0 && code <= t.maxcode[l] && code >= t.mincode[l]) {
        if (l > cnt) return TT_JPEG_ETRUNCATED;
        acc <<= l;
        cnt -= l;
        *out = t.vals[t.valptr[l] + code - t.mincode[l]];
        return 0;
      }
    }
    return cnt < 16 && stop ? TT_JPEG_ETRUNCATED : TT_JPEG_EHUFFMAN;
  }
};

}  // namespace

extern "C" int tt_jpeg_probe(const uint8_t* data, size_t len, int* H, int* W, int* sampling, long long* n_coeffs) {
  Header hd;
  const int rc = parse_header(data, len, hd);
  if (H) *H = rc == 0 ? hd.H : 0;
  if (W) *W = rc == 0 ? hd.W : 0;
  if (sampling) *sampling = rc == 0 ? hd.sampling : -1;
  if (n_coeffs) *n_coeffs = rc == 0 ? coeff_layout(hd, nullptr) : 0;
  return rc;
}

extern "C" int tt_jpeg_scan(const uint8_t* data, size_t len, int16_t* coeffs, long long coeffs_capacity, uint16_t* qtables) {
  Header hd;
  const int rc = parse_header(data, len, hd);
  if (rc != 0) return rc;
  if (!coeffs || !qtables) return TT_JPEG_EARGUMENT;
  long long base[3];
  const long long total = coeff_layout(hd, base);
  if (coeffs_capacity < total) return TT_JPEG_EARGUMENT;
  std::memset(coeffs, 0, sizeof(int16_t) * (size_t)total);
  for (int c = 0; c < 3; ++c) std::memcpy(qtables + 64 * c, hd.q[hd.tq[c]], sizeof(uint16_t) * 64);

  const long long cols[3] = {grid(hd, 0).cols, grid(hd, 1).cols, grid(hd, 2).cols};
  const long long mx = cols[1], mcus = mx * grid(hd, 1).rows;   // the chroma grid is the grid of MCUs
  Bits br{data, hd.scan_pos, len};
  int pred[3] = {0, 0, 0};
  long long until_restart = hd.restart ? hd.restart : mcus;
  int next_rst = 0;
  for (long long mcu = 0; mcu < mcus; ++mcu) {
    if (until_restart == 0) {   // the interval is over: drop the padding bits and take the marker
      br.acc = 0;
      br.cnt = 0;
      size_t p = br.pos;
      if (p >= len || data[p] != 0xFF) return TT_JPEG_ERESTART;
      while (p < len && data[p] == 0xFF) ++p;
      if (p >= len || data[p] != 0xD0 + next_rst) return TT_JPEG_ERESTART;
      br.pos = p + 1;
      br.stop = false;
      next_rst = (next_rst + 1) & 7;
      pred[0] = pred[1] = pred[2] = 0;
      until_restart = hd.restart;
    }
    --until_restart;
    const long long my_i = mcu / mx, mx_i = mcu % mx;
    for (int c = 0; c < 3; ++c) {
      const jh::Table& dc = hd.dc[hd.td[c]].t;
      const jh::Table& ac = hd.ac[hd.ta[c]].t;
      for (int y = 0; y < hd.v[c]; ++y) {
        for (int x = 0; x < hd.h[c]; ++x) {
          int16_t* blk = coeffs + base[c] + ((my_i * hd.v[c] + y) * cols[c] + (mx_i * hd.h[c] + x)) * 64;
          int s, bits, e;
          if ((e = br.symbol(dc, &s)) != 0) return e;
          if (s > 11) return TT_JPEG_EHUFFMAN;   // a DC category an 8-bit file cannot hold
          if (!br.get(s, &bits)) return TT_JPEG_ETRUNCATED;
          pred[c] += jh::extend(bits, s);
          blk[0] = (int16_t)pred[c];
          int k = 1;
          while (k < 64) {
            int rs;
            if ((e = br.symbol(ac, &rs)) != 0) return e;
            const int r = rs >> 4;
            s = rs & 15;
            if (s == 0) {
              if (r != 15) break;   // EOB
              k += 16;              // ZRL
              if (k > 64) return TT_JPEG_ERUN;
              continue;
            }
            k += r;
            if (k > 63) return TT_JPEG_ERUN;
            if (!br.get(s, &bits)) return TT_JPEG_ETRUNCATED;
            blk[kZigzag[k]] = (int16_t)jh::extend(bits, s);
            ++k;
          }
        }
      }
    }
  }
  return TT_JPEG_OK;
}

// ---- N24: the host half of the device entropy decode.  tt_jpeg_prepare copies the scan ONCE without decoding a bit (the runs between FF bytes whole: memchr, then memcpy):
// stuffing and fill bytes dropped, cut at the RSTn markers (whose numbering it checks), every segment on a 4-byte boundary.  In front of
// the stream it puts the DHT bytes of the six tables in use (jh::kHuffBytes).  tt_jpeg_entropy_host is the emulation of jpeg_entropy.hip:
// the same phases through the same header (jpeg_huff.hpp), with loops over the lanes.
extern "C" int tt_jpeg_prepare_bytes(size_t len, size_t* scan_bytes, size_t* n_segments) {
  // every boundary drops a 2-byte marker and pads at most 3 bytes: at most len / 2 boundaries, one byte more each
  if (scan_bytes) *scan_bytes = ((size_t)tt::jh::kHuffBytes + len + len / 2 + 8 + 3) / 4 * 4;
  if (n_segments) *n_segments = len / 2 + 1;
  return TT_JPEG_OK;
}

extern "C" int tt_jpeg_prepare(const uint8_t* data, size_t len, uint8_t* scan, size_t scan_capacity, uint32_t* segs, size_t seg_capacity,
                               tt_jpeg_stream* row, uint16_t* qtables) {
  Header hd;
  const int rc = parse_header(data, len, hd);
  if (rc != 0) return rc;
  if (!scan || !segs || !row || !qtables || scan_capacity < (size_t)jh::kHuffBytes) return TT_JPEG_EARGUMENT;
  std::memset(row, 0, sizeof(*row));
  row->H = hd.H;
  row->W = hd.W;
  row->sampling = hd.sampling;
  row->restart = hd.restart;
  long long base[3];
  coeff_layout(hd, base);
  for (int c = 0; c < 3; ++c) {
    row->coeff_off[c] = base[c];
    std::memcpy(qtables + 64 * c, hd.q[hd.tq[c]], sizeof(uint16_t) * 64);
    const Huff* two[2] = {&hd.dc[hd.td[c]], &hd.ac[hd.ta[c]]};
    for (int k = 0; k < 2; ++k) {
      uint8_t* dst = scan + (2 * c + k) * jh::kDht;
      std::memset(dst, 0, (size_t)jh::kDht);
      std::memcpy(dst, two[k]->counts, 16);
      std::memcpy(dst + 16, two[k]->t.vals, (size_t)two[k]->nvals);
    }
  }
  const jh::Frame f = jh::make_frame(*row);
  if ((size_t)f.n_segments > seg_capacity) return TT_JPEG_EARGUMENT;
  row->huff_off = 0;
  row->scan_off = jh::kHuffBytes;
  row->seg_off = 0;
  row->n_segments = f.n_segments;
  uint8_t* out = scan + jh::kHuffBytes;
  const size_t cap = scan_capacity - (size_t)jh::kHuffBytes;
  size_t w = 0, seg_start = 0, pos = hd.scan_pos;
  uint32_t seg = 0;
  bool closed = false;
  while (!closed) {
    int marker = -1;   // -1 none, 0 the data ended
    if (pos >= len) {
      marker = 0;
    } else {
      const uint8_t b = data[pos];
      if (b != 0xFF) {   // the run up to the next FF in one copy
        const void* ff = std::memchr(data + pos, 0xFF, len - pos);
        const size_t run = ff ? (size_t)(static_cast<const uint8_t*>(ff) - (data + pos)) : len - pos;
        if (run > cap - w) return TT_JPEG_EARGUMENT;
        std::memcpy(out + w, data + pos, run);
        w += run;
        pos += run;
      } else if (pos + 1 >= len) {
        marker = 0;
      } else if (data[pos + 1] == 0x00) {   // a stuffed FF
        if (w >= cap) return TT_JPEG_EARGUMENT;
        out[w++] = 0xFF;
        pos += 2;
      } else if (data[pos + 1] == 0xFF) {   // a fill byte
        ++pos;
      } else {
        marker = data[pos + 1];
      }
    }
    if (marker < 0) continue;
    if ((w - seg_start) * 8 > (size_t)jh::kMaxSegBits) return TT_JPEG_EARGUMENT;
    segs[2 * seg] = (uint32_t)seg_start;
    segs[2 * seg + 1] = (uint32_t)((w - seg_start) * 8);
    while (w % 4) {
      if (w >= cap) return TT_JPEG_EARGUMENT;
      out[w++] = 0;
    }
    if (seg + 1 == f.n_segments) {
      closed = true;   // whatever follows the last interval is not looked at, as in tt_jpeg_scan
    } else {
      if (marker == 0) return TT_JPEG_ETRUNCATED;
      if (marker != 0xD0 + (int)(seg & 7u)) return TT_JPEG_ERESTART;
      pos += 2;
      ++seg;
      seg_start = w;
      if (seg_start > 0xfffffff0u) return TT_JPEG_EARGUMENT;
    }
  }
  row->scan_len = (int64_t)w;
  return TT_JPEG_OK;
}

namespace {

// One frame, as one workgroup of jh::kTile lanes runs it (jpeg_entropy.hip: the same steps, the loops over i are its lanes).
int entropy_frame(const uint8_t* scan, const uint32_t* segs, const tt_jpeg_stream& row, uint32_t S, int16_t* coeffs, int32_t* stats) {
  constexpr int T = jh::kTile;
  const jh::Frame f = jh::make_frame(row);
  static_assert(sizeof(jh::Table) * 6 < 16384, "the tables fit the stack");
  jh::Table tabs[6];
  const uint8_t* dht = scan + row.huff_off;
  for (int t = 0; t < 6; ++t) {
    std::memcpy(tabs[t].vals, dht + t * jh::kDht + 16, 256);
    jh::build_codes(tabs[t], dht + t * jh::kDht);
    for (int v = 0; v < (1 << jh::kLook); ++v) tabs[t].look[v] = jh::look_entry(tabs[t], v);
  }
  const uint32_t* stream = reinterpret_cast<const uint32_t*>(scan + row.scan_off);
  const uint32_t* sg = segs + 2 * row.seg_off;
  uint32_t cur_seg = 0, cur_sub = 0, carry_p = 0, carry_q = 0, carry_blocks = 0;
  int status = 0, rounds = 0, tiles = 0, first_bad = -1;
  long long subs = 0;
  uint32_t l_seg[T], l_sub[T], ex_p[T], ex_q[T], l_cnt[T], l_n0[T];
  jh::State entry[T];
  bool dirty[T];
  while (cur_seg < f.n_segments && status == 0) {
    int n = 0;
    while (n < T && cur_seg < f.n_segments) {
      l_seg[n] = cur_seg;
      l_sub[n] = cur_sub;
      ++n;
      if (++cur_sub >= jh::subsequences(sg[2 * cur_seg + 1], S)) {
        ++cur_seg;
        cur_sub = 0;
      }
    }
    for (int i = 0; i < n; ++i) {
      entry[i] = l_sub[i] == 0 ? jh::State{0, 0, 0, 0} : (i == 0 ? jh::unpack(carry_p, carry_q) : jh::State{l_sub[i] * S, 0, 0, 0});
      dirty[i] = true;
    }
    for (int round = 0; round <= T; ++round) {
      for (int i = 0; i < n; ++i) {
        if (!dirty[i]) continue;
        const uint32_t bits = sg[2 * l_seg[i] + 1], end = (l_sub[i] + 1) * S < bits ? (l_sub[i] + 1) * S : bits;
        jh::State s = entry[i];
        l_cnt[i] = jh::run_count(tabs, f, stream + sg[2 * l_seg[i]] / 4, bits, s, end, l_seg[i]);
        ex_p[i] = s.p;
        ex_q[i] = jh::pack(s);
      }
      bool any = false;
      for (int i = 0; i < n; ++i) {
        dirty[i] = false;
        if (i == 0 || l_sub[i] == 0) continue;
        if (ex_p[i - 1] != entry[i].p || ex_q[i - 1] != jh::pack(entry[i])) {
          entry[i] = jh::unpack(ex_p[i - 1], ex_q[i - 1]);
          dirty[i] = any = true;
        }
      }
      if (!any) break;
      ++rounds;
    }
    for (int i = 0; i < n; ++i) {
      uint32_t n0 = 0;
      int u = i - 1;
      for (; u >= 0 && l_seg[u] == l_seg[i]; --u) n0 += l_cnt[u];
      if (u < 0 && l_sub[i] > (uint32_t)i) n0 += carry_blocks;
      l_n0[i] = n0;
    }
    for (int i = 0; i < n; ++i) {
      const uint32_t bits = sg[2 * l_seg[i] + 1], end = (l_sub[i] + 1) * S < bits ? (l_sub[i] + 1) * S : bits;
      const int e = jh::run_write(tabs, f, stream + sg[2 * l_seg[i]] / 4, bits, entry[i], end, l_seg[i], l_n0[i], coeffs);
      if (e && status == 0) {
        status = e;
        first_bad = (int)(subs + i);
      }
    }
    carry_p = ex_p[n - 1];
    carry_q = ex_q[n - 1];
    carry_blocks = l_n0[n - 1] + l_cnt[n - 1];
    subs += n;
    ++tiles;
  }
  if (status == 0)
    for (int c = 0; c < 3; ++c) jh::dc_apply(f, coeffs, c, 0, jh::dc_blocks(f, c), 0);
  if (stats) {
    stats[0] = rounds;
    stats[1] = tiles;
    stats[2] = (int32_t)subs;
    stats[3] = first_bad;
  }
  return status;
}

}  // namespace

// (a pure host function, so it lives here: the sanitizer program links this file alone)
extern "C" size_t tt_jpeg_entropy_batch_workspace_bytes(const tt_jpeg_stream* stream_table, int n_frames, int subseq_bits) {
  if (!stream_table || n_frames < 1 || n_frames > 65535 || subseq_bits < jh::kMinSubseq || subseq_bits > jh::kMaxSubseq || subseq_bits % 32) return 0;
  return jh::workspace_bytes(n_frames);
}

extern "C" int tt_jpeg_entropy_host(const uint8_t* scan, long long scan_bytes, const uint32_t* segs, const uint32_t* segs_again, long long n_segs,
                                    const tt_jpeg_stream* stream_table, const tt_jpeg_stream* stream_table_again, int n_frames, int subseq_bits,
                                    int16_t* coeffs, long long n_coeffs, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  (void)segs_again;
  (void)stream_table_again;
  (void)stream;
  char msg[256];
  if (!scan || !coeffs || !status || !workspace || (reinterpret_cast<uintptr_t>(scan) & 3u) || (reinterpret_cast<uintptr_t>(workspace) & 3u))
    return TT_EINVAL;
  if (tt::jh::validate(scan_bytes, segs, n_segs, stream_table, n_frames, subseq_bits, n_coeffs, msg, sizeof(msg)) != 0) return TT_EINVAL;
  if (workspace_bytes < tt::jh::workspace_bytes(n_frames)) return TT_EINVAL;
  std::memset(coeffs, 0, sizeof(int16_t) * (size_t)n_coeffs);
  int32_t* stats = static_cast<int32_t*>(workspace);
  for (int i = 0; i < n_frames; ++i)
    status[i] = entropy_frame(scan, segs, stream_table[i], (uint32_t)subseq_bits, coeffs, stats + i * tt::jh::kStatWords);
  return TT_OK;
}
