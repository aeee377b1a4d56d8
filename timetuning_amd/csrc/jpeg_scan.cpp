// N21, host half: marker parsing and Huffman decoding of baseline JPEG files - what is serial by nature.  tt_jpeg_probe classifies a
// file, tt_jpeg_scan writes its quantised DCT coefficients (de-zigzagged, int16, 64 per block, per component in block-grid raster order)
// and the quantisation table of each component; dequantisation, IDCT, up-sampling and colour run on the device (jpeg.hip).
//
// Plain C++17 with no HIP include: the file also compiles with the host compiler alone (tools/jpeg_scan_check.cpp builds it under
// AddressSanitizer).  Both entries are pure functions: no state, no allocation (the tables live on the stack, about 5 KB), no GPU call, so
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

namespace {

constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kLook = 9;   // bits of the Huffman look-ahead table

struct Huff {
  bool present = false;
  uint8_t vals[256];
  int32_t maxcode[18];          // largest code of each length, -1 = none
  int32_t valptr[17];           // vals index of the first code of each length
  int32_t mincode[17];
  uint16_t look[1 << kLook];    // (length << 8) | value for codes of up to kLook bits, 0 = longer
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
bool build_huff(Huff& t, const uint8_t* bits, const uint8_t* vals, int n) {
  std::memcpy(t.vals, vals, (size_t)n);
  std::memset(t.look, 0, sizeof(t.look));
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    t.valptr[len] = k;
    t.mincode[len] = code;
    const int cnt = bits[len - 1];
    if (code + cnt > (1 << len)) return false;
    for (int i = 0; i < cnt; ++i, ++k, ++code) {
      if (len <= kLook) {
        const int first = code << (kLook - len);
        for (int j = 0; j < (1 << (kLook - len)); ++j) t.look[first + j] = (uint16_t)((len << 8) | t.vals[k]);
      }
    }
    t.maxcode[len] = cnt ? code - 1 : -1;
    code <<= 1;
  }
  t.maxcode[17] = 0x7fffffff;
  t.present = true;
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

inline void grid(const Header& hd, int c, long long* rows, long long* cols) {
  const long long mx = (hd.W + 8 * hd.h[0] - 1) / (8 * hd.h[0]), my = (hd.H + 8 * hd.v[0] - 1) / (8 * hd.v[0]);
  *rows = my * hd.v[c];
  *cols = mx * hd.h[c];
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
  int symbol(const Huff& t, int* out) {
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

inline int extend(int v, int s) { return s && v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

}  // namespace

extern "C" int tt_jpeg_probe(const uint8_t* data, size_t len, int* H, int* W, int* sampling, long long* n_coeffs) {
  Header hd;
  const int rc = parse_header(data, len, hd);
  if (H) *H = rc == 0 ? hd.H : 0;
  if (W) *W = rc == 0 ? hd.W : 0;
  if (sampling) *sampling = rc == 0 ? hd.sampling : -1;
  long long total = 0;
  if (rc == 0) {
    for (int c = 0; c < 3; ++c) {
      long long r, q;
      grid(hd, c, &r, &q);
      total += r * q * 64;
    }
  }
  if (n_coeffs) *n_coeffs = total;
  return rc;
}

extern "C" int tt_jpeg_scan(const uint8_t* data, size_t len, int16_t* coeffs, long long coeffs_capacity, uint16_t* qtables) {
  Header hd;
  const int rc = parse_header(data, len, hd);
  if (rc != 0) return rc;
  if (!coeffs || !qtables) return TT_JPEG_EARGUMENT;
  long long rows[3], cols[3], base[3], total = 0;
  for (int c = 0; c < 3; ++c) {
    grid(hd, c, &rows[c], &cols[c]);
    base[c] = total;
    total += rows[c] * cols[c] * 64;
  }
  if (coeffs_capacity < total) return TT_JPEG_EARGUMENT;
  std::memset(coeffs, 0, sizeof(int16_t) * (size_t)total);
  for (int c = 0; c < 3; ++c) std::memcpy(qtables + 64 * c, hd.q[hd.tq[c]], sizeof(uint16_t) * 64);

  const long long mx = cols[0] / hd.h[0], my = rows[0] / hd.v[0], mcus = mx * my;
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
      const Huff& dc = hd.dc[hd.td[c]];
      const Huff& ac = hd.ac[hd.ta[c]];
      for (int y = 0; y < hd.v[c]; ++y) {
        for (int x = 0; x < hd.h[c]; ++x) {
          int16_t* blk = coeffs + base[c] + ((my_i * hd.v[c] + y) * cols[c] + (mx_i * hd.h[c] + x)) * 64;
          int s, bits, e;
          if ((e = br.symbol(dc, &s)) != 0) return e;
          if (s > 11) return TT_JPEG_EHUFFMAN;   // a DC category an 8-bit file cannot hold
          if (!br.get(s, &bits)) return TT_JPEG_ETRUNCATED;
          pred[c] += extend(bits, s);
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
            blk[kZigzag[k]] = (int16_t)extend(bits, s);
            ++k;
          }
        }
      }
    }
  }
  return TT_JPEG_OK;
}
