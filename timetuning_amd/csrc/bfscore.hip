// Boundary F1 score: the contour matching score of bfscore.py:21-165 as integer counts.
//
// The reference takes the contours of gt == c and pr == c with cv2.findContours(RETR_LIST, CHAIN_APPROX_NONE), concatenates their
// points WITH multiplicity (a pixel the border follower passes twice is listed twice) and counts, for each point of one list, whether
// the other list has a point at squared distance d < t^2.  The follower's passes through a pixel depend on its 3 x 3 neighbourhood
// only, so the multiplicity m(p) is BF_MULT[the 8 neighbour bits] (derived from the border-following restatement of the tests and
// checked there for all 256 entries).  Per (map pair) the score needs four integers:
//   tt_bf_counts   [P, 4] = {n_pr, hit_pr, n_gt, hit_gt}: n = sum of m over the map, hit = the same sum over the pixels that have a
//                  contour pixel (m > 0) of the OTHER map within the element {(dy, dx): dy^2 + dx^2 < t^2} (the host's spans).
//
// One workgroup per (pair, tile of TH rows x ow 64-bit words):
//   A  every (row, word) of the tile plus its halo (r + 1 rows above and below, one word either side) is loaded once, one pixel per lane,
//      BF_BATCH words per wave in flight, and balloted into wave64 "set" words in LDS (both maps).
//   B  one wave per (row, word) of the tile and the r-row halo: lane k reads the 3 x 3 neighbourhood of bit k from the set words, looks
//      m up in the table (LDS), and ballots m >= 1 (the contour words, all rows) and m >= 2, 3, 4 (the tile's own words only).
//      Bit 0 of the left halo word and bit 63 of the right one miss a neighbour; the dilation never reads them.
//   C  per own word and map: n += sum_k popc(m >= k); where the contour word is non-zero, the other map's contour is dilated at that
//      word only (bit_dilate.hpp: per element row a run-OR of its span, stopping once every contour pixel of the word is matched) and
//      hit += sum_k popc((m >= k) & dilation).
// Counts are int32 per thread, reduced over the workgroup and added with ONE 64-bit integer atomic per counter per tile: exact and
// independent of the order of the adds.  No floating point anywhere.
#include "common.hpp"
#include "bit_dilate.hpp"

namespace tt {

constexpr int BF_THREADS = 256;
constexpr int BF_WAVES = BF_THREADS / 64;
constexpr int BF_MAX_R = 63;          // element radius: a one-word halo either side covers offsets -63..63
constexpr int BF_BATCH = 8;           // cells a wave loads before it ballots them
constexpr size_t BF_LDS_BUDGET = 64 * 1024;

// m of a set pixel by its neighbour bits, bit k = E, SE, S, SW, W, NW, N, NE (rows grow downwards); 0 = interior, 1 = isolated pixel
__constant__ uint8_t BF_MULT[256] = {
    1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1,
    1, 2, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3, 2, 2, 2, 2, 1, 2, 2, 2, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1,
    1, 1, 2, 1, 2, 1, 2, 1, 2, 2, 3, 2, 2, 1, 2, 1, 1, 1, 2, 1, 1, 0, 1, 0, 1, 1, 2, 1, 1, 0, 1, 0,
    1, 1, 2, 1, 2, 1, 2, 1, 2, 2, 3, 2, 2, 1, 2, 1, 1, 1, 2, 1, 1, 0, 1, 0, 1, 1, 2, 1, 1, 0, 1, 0,
    1, 1, 2, 1, 2, 1, 2, 1, 2, 2, 3, 2, 2, 1, 2, 1, 2, 2, 3, 2, 2, 1, 2, 1, 2, 2, 3, 2, 2, 1, 2, 1,
    2, 2, 3, 2, 3, 2, 3, 2, 3, 3, 4, 3, 3, 2, 3, 2, 2, 2, 3, 2, 2, 1, 2, 1, 2, 2, 3, 2, 2, 1, 2, 1,
    1, 1, 2, 1, 2, 1, 2, 1, 2, 2, 3, 2, 2, 1, 2, 1, 1, 1, 2, 1, 1, 0, 1, 0, 1, 1, 2, 1, 1, 0, 1, 0,
    1, 1, 2, 1, 2, 1, 2, 1, 2, 2, 3, 2, 2, 1, 2, 1, 1, 1, 2, 1, 1, 0, 1, 0, 1, 1, 2, 1, 1, 0, 1, 0};

struct BfElement {
  int r;                                                 // rows -r..r, columns -r..r around the anchor (r, r)
  signed char lo[2 * BF_MAX_R + 1], hi[2 * BF_MAX_R + 1];   // set columns of each row; lo > hi: an empty row
};

// bit k of the word Cw with its neighbours in the words either side: dx = -1 (left), +1 (right)
__device__ __forceinline__ unsigned bit_left(u64 Lw, u64 Cw, int k) { return k == 0 ? (unsigned)(Lw >> 63) : (unsigned)(Cw >> (k - 1)) & 1u; }
__device__ __forceinline__ unsigned bit_right(u64 Cw, u64 Rw, int k) { return k == 63 ? (unsigned)(Rw & 1ull) : (unsigned)(Cw >> (k + 1)) & 1u; }

__global__ __launch_bounds__(BF_THREADS) void bf_counts_kernel(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ pr,
                                                               long long* __restrict__ out, int H, int W, int TH, int ow, int tiles_x,
                                                               int tiles_y, BfElement el) {
  extern __shared__ u64 lds[];
  __shared__ uint8_t tab[256];
  __shared__ int red[BF_WAVES][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per_pair = tiles_x * tiles_y;
  const int pair = blockIdx.x / per_pair;
  const int rem = blockIdx.x - pair * per_pair;
  const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
  const int R = el.r;
  const int y0 = ty * TH;
  const int wx0 = tx * ow;                 // first own word
  const int lw = ow + 2;                   // loaded words: one halo word either side
  const int rows_l = TH + 2 * R + 2;       // set rows: y0 - R - 1 .. y0 + TH + R
  const int rows_m = TH + 2 * R;           // contour rows: y0 - R .. y0 + TH + R - 1
  const int own_rows = min(TH, H - y0);
  const int own_words = min(ow, (W + 63) / 64 - wx0);
  const size_t plane_l = (size_t)rows_l * lw, plane_m = (size_t)rows_m * lw, plane_o = (size_t)TH * ow;
  u64* setw = lds;                         // [2][rows_l][lw], map 0 = pr, 1 = gt
  u64* cont = setw + 2 * plane_l;          // [2][rows_m][lw]: m >= 1
  u64* thr = cont + 2 * plane_m;           // [2][3][TH][ow]: m >= 2, 3, 4 of the own words
  const long long HW = (long long)H * W;
  const uint8_t* maps[2] = {pr + pair * HW, gt + pair * HW};

  if (tid < 256) tab[tid] = BF_MULT[tid];

  // ---- A: set words of the tile and its halo
  const int ncells = rows_l * lw;
  for (int base = wave; base < ncells; base += BF_WAVES * BF_BATCH) {
    uint8_t v[2][BF_BATCH];
#pragma unroll
    for (int k = 0; k < BF_BATCH; ++k) {
      const int cell = base + k * BF_WAVES;
      const int r = cell / lw, w = cell - r * lw;
      const int y = y0 - R - 1 + r;
      const long long x = (long long)(wx0 + w - 1) * 64 + lane;
      v[0][k] = 0;
      v[1][k] = 0;
      if (cell < ncells && y >= 0 && y < H && x >= 0 && x < W) {
        const long long i = (long long)y * W + x;
        v[0][k] = maps[0][i];
        v[1][k] = maps[1][i];
      }
    }
#pragma unroll
    for (int k = 0; k < BF_BATCH; ++k) {
      const int cell = base + k * BF_WAVES;
      if (cell >= ncells) break;   // uniform over the wave
      const u64 b0 = __ballot(v[0][k] != 0);
      const u64 b1 = __ballot(v[1][k] != 0);
      if (lane == 0) {
        setw[cell] = b0;
        setw[plane_l + cell] = b1;
      }
    }
  }
  __syncthreads();

  // ---- B: multiplicity threshold words, one wave per (row, word), lane = bit
  for (int cell = wave; cell < rows_m * lw; cell += BF_WAVES) {
    const int mr = cell / lw, w = cell - mr * lw;
    const bool own = mr >= R && mr < R + own_rows && w >= 1 && w <= own_words;   // uniform over the wave
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const u64* s = setw + m * plane_l;
      u64 nb[3][3];   // rows mr .. mr + 2 of the set words (y - 1, y, y + 1), words w - 1 .. w + 1
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int wj = w + j - 1;
          nb[i][j] = (wj >= 0 && wj < lw) ? s[(size_t)(mr + i) * lw + wj] : 0ull;
        }
      const unsigned centre = (unsigned)(nb[1][1] >> lane) & 1u;
      const unsigned idx = bit_right(nb[1][1], nb[1][2], lane) | bit_right(nb[2][1], nb[2][2], lane) << 1 |
                           ((unsigned)(nb[2][1] >> lane) & 1u) << 2 | bit_left(nb[2][0], nb[2][1], lane) << 3 |
                           bit_left(nb[1][0], nb[1][1], lane) << 4 | bit_left(nb[0][0], nb[0][1], lane) << 5 |
                           ((unsigned)(nb[0][1] >> lane) & 1u) << 6 | bit_right(nb[0][1], nb[0][2], lane) << 7;
      const int mult = centre ? tab[idx] : 0;
      const u64 c1 = __ballot(mult >= 1);
      if (lane == 0) cont[m * plane_m + cell] = c1;
      if (own) {
        const u64 c2 = __ballot(mult >= 2), c3 = __ballot(mult >= 3), c4 = __ballot(mult >= 4);
        if (lane == 0) {
          const size_t o = (size_t)(mr - R) * ow + (w - 1);
          thr[(m * 3 + 0) * plane_o + o] = c2;
          thr[(m * 3 + 1) * plane_o + o] = c3;
          thr[(m * 3 + 2) * plane_o + o] = c4;
        }
      }
    }
  }
  __syncthreads();

  // ---- C: weighted counts and matches of the own words
  int cnt[4] = {0, 0, 0, 0};
  for (int cell = tid; cell < own_rows * own_words; cell += BF_THREADS) {
    const int ro = cell / own_words, wo = cell - ro * own_words;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const u64 t1 = cont[m * plane_m + (size_t)(ro + R) * lw + wo + 1];
      if (!t1) continue;
      const size_t o = (size_t)ro * ow + wo;
      const u64 t2 = thr[(m * 3 + 0) * plane_o + o], t3 = thr[(m * 3 + 1) * plane_o + o], t4 = thr[(m * 3 + 2) * plane_o + o];
      cnt[2 * m] += __popcll(t1) + __popcll(t2) + __popcll(t3) + __popcll(t4);
      const u64* other = cont + (1 - m) * plane_m;
      u64 dil = 0;
      for (int i = 0; i <= 2 * R; ++i) {
        const int lo = el.lo[i], hi = el.hi[i];
        if (lo > hi) continue;
        const size_t q = (size_t)(ro + i) * lw + wo;   // contour row y + i - R, words wo - 1 .. wo + 1
        const u64 L = other[q], C = other[q + 1], Rw = other[q + 2];
        if (!(L | C | Rw)) continue;
        dil |= row_dilate(L, C, Rw, lo, hi, R);
        if (!(t1 & ~dil)) break;   // every contour pixel of this word is matched already
      }
      cnt[2 * m + 1] += __popcll(t1 & dil) + __popcll(t2 & dil) + __popcll(t3 & dil) + __popcll(t4 & dil);
    }
  }

  // ---- one integer atomic per counter per tile
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    int v = cnt[c];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) red[wave][c] = v;
  }
  __syncthreads();
  if (tid < 4) {
    int s = 0;
    for (int w = 0; w < BF_WAVES; ++w) s += red[w][tid];
    if (s) atomicAdd(reinterpret_cast<u64*>(out) + (size_t)pair * 4 + tid, (u64)s);
  }
}

// TH rows x ow words per tile: TH = 32 and up to 8 words, smaller where the LDS planes of a large element would not fit the budget
static bool bf_tiling(int H, int W, int R, int& TH, int& ow, size_t& lds) {
  const int words = (W + 63) / 64;
  const int tx = (words + 7) / 8;
  ow = (words + tx - 1) / tx;
  TH = H < 32 ? H : 32;
  for (;;) {
    const size_t lw = ow + 2;
    lds = sizeof(u64) * (2 * (TH + 2 * R + 2) * lw + 2 * (TH + 2 * R) * lw + 6 * (size_t)TH * ow);
    if (lds <= BF_LDS_BUDGET) return true;
    if (TH > 8) TH /= 2;
    else if (ow > 1) --ow;
    else return false;
  }
}

}  // namespace tt

using namespace tt;

extern "C" int tt_bf_counts(const uint8_t* gt, const uint8_t* pr, long long* counts, int P, int H, int W, const int* spans, int el_rows,
                            tt_stream_t stream) {
  TT_REQUIRE(gt && pr && counts && spans, "bf_counts: gt, pr, counts and spans are required");
  TT_REQUIRE(P >= 1 && H >= 1 && W >= 1 && (long long)H * W <= (1LL << 31),
             "bf_counts: need P, H, W >= 1 and H * W <= 2^31 (got %d, %d, %d)", P, H, W);
  TT_REQUIRE(el_rows >= 1 && el_rows % 2 == 1 && el_rows <= 2 * BF_MAX_R + 1,
             "bf_counts: the element has %d rows; an odd count up to %d (t <= %d) is supported", el_rows, 2 * BF_MAX_R + 1, BF_MAX_R + 1);
  BfElement el;
  el.r = el_rows / 2;
  for (int i = 0; i <= 2 * BF_MAX_R; ++i) {
    el.lo[i] = 1;
    el.hi[i] = 0;
  }
  for (int i = 0; i < el_rows; ++i) {
    const int lo = spans[2 * i], hi = spans[2 * i + 1];
    TT_REQUIRE(lo > hi || (lo >= 0 && hi < el_rows), "bf_counts: span %d..%d of row %d outside the %d columns", lo, hi, i, el_rows);
    el.lo[i] = (signed char)(lo > hi ? 1 : lo);
    el.hi[i] = (signed char)(lo > hi ? 0 : hi);
  }
  int TH, ow;
  size_t lds;
  TT_REQUIRE(bf_tiling(H, W, el.r, TH, ow, lds), "bf_counts: no tiling fits the LDS budget");
  const int tiles_y = (H + TH - 1) / TH;
  const int tiles_x = ((W + 63) / 64 + ow - 1) / ow;
  const long long blocks = (long long)P * tiles_y * tiles_x;
  TT_REQUIRE(blocks <= 0x7fffffffLL, "bf_counts: %lld workgroups", blocks);
  hipStream_t s = as_stream(stream);
  if (hipMemsetAsync(counts, 0, sizeof(long long) * 4 * (size_t)P, s) != hipSuccess) {
    set_error("bf_counts: clearing the counts failed");
    return TT_ELAUNCH;
  }
  hipLaunchKernelGGL(bf_counts_kernel, dim3((unsigned)blocks), dim3(BF_THREADS), lds, s, gt, pr, counts, H, W, TH, ow, tiles_x, tiles_y,
                     el);
  TT_CHECK_LAUNCH("bf_counts");
  return TT_OK;
}
