// DAVIS J&F: the region and boundary metrics of semi-supervised VOS, mask_propagation.py:501-715.
//
// The reference scores every (object, frame) with numpy and cv2: J = |P & G| / |P | G| over the non-void pixels (db_eval_iou), and
// F from two 1-pixel boundary maps (_seg2bmap of the masks times "not void"), each dilated by a disk (cv2.dilate), matched against the
// other map's boundary (f_measure).  Every one of those numbers is an integer count, which is what this file computes:
//   tt_davis_jf_counts   [O, T, 6] = {J intersection, J union, n_fg, n_gt, fg_match, gt_match} for objects 1..O of label maps
//   tt_davis_seg2bmap    the boundary map of a binary map, per pixel (the _seg2bmap surface and the tests)
//
// tt_davis_jf_counts runs one workgroup per (frame, tile of TH rows x ow 64-bit words).  Per pass over a chunk of up to DV_OC objects:
//   A  every (row, word) of the tile plus its halo (ay rows above, rows - ay below, one word either side) is loaded once, one pixel per
//      lane, DV_BATCH words per wave in flight; each object's P = (pred == o) & !void and G = (gt == o) & !void come out as wave64
//      __ballot words into LDS.  The J counts of the tile's own words are taken here.
//   B  the boundary words of every halo row but the last, from the rule of _seg2bmap at the IMAGE edge: interior s^e | s^s | s^se,
//      last row s^e, last column s^s, the bottom-right pixel 0, nothing outside the image.
//   C  per own word: popcount of the two boundaries; where a word of one boundary is non-zero, the other boundary is dilated at that
//      word only - per element row, a horizontal run-OR of its span (shift doubling on a 128-bit window) - and ANDed with it.
// Counts are int32 per thread, reduced over the wave and the workgroup and added with ONE 64-bit integer atomic per counter per tile:
// the sums are exact and the result does not depend on the order of the adds.  No floating point anywhere.
#include "common.hpp"
#include "bit_dilate.hpp"

namespace tt {

constexpr int DV_THREADS = 256;
constexpr int DV_WAVES = DV_THREADS / 64;
constexpr int DV_OC = 4;               // objects per pass over the labels
constexpr int DV_MAX_EL = 127;         // element rows / columns: a one-word halo either side covers offsets -63..63
constexpr int DV_NCNT = 6;
constexpr int DV_BATCH = 8;          // cells whose labels a wave loads before it ballots them
constexpr size_t DV_LDS_BUDGET = 64 * 1024;

typedef unsigned long long u64;

struct DavisElement {
  int rows, cols, ay, ax;
  signed char lo[DV_MAX_EL + 1], hi[DV_MAX_EL + 1];   // columns of the set pixels of each row; lo > hi: an empty row
};

// bits k of the word whose first column is xw that lie in [0, n)
__device__ __forceinline__ u64 cols_below(long long xw, long long n) {
  if (xw < 0) return 0ull;
  const long long m = n - xw;
  return m <= 0 ? 0ull : (m >= 64 ? ~0ull : ((1ull << m) - 1ull));
}

template <typename TP, typename TG>
__global__ __launch_bounds__(DV_THREADS) void davis_counts_kernel(const TP* __restrict__ pred, const TG* __restrict__ gt,
                                                                  const uint8_t* __restrict__ voidm, long long* __restrict__ out, int T,
                                                                  int H, int W, int O, int TH, int ow, int tiles_x, int tiles_y,
                                                                  DavisElement el) {
  extern __shared__ u64 lds[];
  __shared__ int red[DV_WAVES][DV_OC * DV_NCNT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per_frame = tiles_x * tiles_y;
  const int t = blockIdx.x / per_frame;
  const int rem = blockIdx.x - t * per_frame;
  const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
  const int y0 = ty * TH;
  const int wx0 = tx * ow;                 // first own word
  const int lw = ow + 2;                   // loaded words: one halo word either side
  const int rows_l = TH + el.rows;         // loaded rows: y0 - ay .. y0 + TH + rows - ay - 1
  const int own_rows = min(TH, H - y0);
  const int own_words = min(ow, (W + 63) / 64 - wx0);
  const int oc_max = min(O, DV_OC);
  const size_t plane = (size_t)rows_l * lw;
  u64* segP = lds;                         // [oc][rows_l][lw]
  u64* segG = segP + oc_max * plane;
  u64* bndP = segG + oc_max * plane;
  u64* bndG = bndP + oc_max * plane;
  const long long HW = (long long)H * W;
  const TP* pf = pred + t * HW;
  const TG* gf = gt + t * HW;
  const uint8_t* vf = voidm ? voidm + t * HW : nullptr;

  for (int obj0 = 0; obj0 < O; obj0 += DV_OC) {
    const int oc = min(DV_OC, O - obj0);
    int cnt[DV_OC][DV_NCNT];
#pragma unroll
    for (int o = 0; o < DV_OC; ++o)
#pragma unroll
      for (int c = 0; c < DV_NCNT; ++c) cnt[o][c] = 0;

    // ---- A: object bits of the tile and its halo, J counts of the own words.  DV_BATCH cells' loads are issued before their
    // ballots, so a wave waits for one memory latency per batch, not per cell.
    const int ncells = rows_l * lw;
    for (int base = wave; base < ncells; base += DV_WAVES * DV_BATCH) {
      long long lp[DV_BATCH], lg[DV_BATCH];   // 0 is never an object
#pragma unroll
      for (int k = 0; k < DV_BATCH; ++k) {
        const int cell = base + k * DV_WAVES;
        const int r = cell / lw, w = cell - r * lw;
        const int y = y0 - el.ay + r;
        const long long x = (long long)(wx0 + w - 1) * 64 + lane;
        lp[k] = 0;
        lg[k] = 0;
        if (cell < ncells && y >= 0 && y < H && x >= 0 && x < W) {
          const long long i = (long long)y * W + x;
          if (!(vf && vf[i])) {
            lp[k] = (long long)pf[i];
            lg[k] = (long long)gf[i];
          }
        }
      }
#pragma unroll
      for (int k = 0; k < DV_BATCH; ++k) {
        const int cell = base + k * DV_WAVES;
        if (cell >= ncells) break;   // uniform over the wave
        const int r = cell / lw, w = cell - r * lw;
        const bool own = r >= el.ay && r < el.ay + own_rows && w >= 1 && w <= own_words;
#pragma unroll
        for (int o = 0; o < DV_OC; ++o) {
          if (o < oc) {
            const u64 bp = __ballot(lp[k] == obj0 + o + 1);
            const u64 bg = __ballot(lg[k] == obj0 + o + 1);
            if (lane == 0) {
              segP[o * plane + cell] = bp;
              segG[o * plane + cell] = bg;
              if (own) {
                cnt[o][0] += __popcll(bp & bg);
                cnt[o][1] += __popcll(bp | bg);
              }
            }
          }
        }
      }
    }
    __syncthreads();

    // ---- B: boundary words of rows 0 .. rows_l - 2 (row rows_l - 1 only feeds the row above it)
    for (int cell = tid; cell < oc * (rows_l - 1) * lw; cell += DV_THREADS) {
      const int o = cell / ((rows_l - 1) * lw);
      const int rc = cell - o * (rows_l - 1) * lw;
      const int r = rc / lw, w = rc - r * lw;
      const int y = y0 - el.ay + r;
      u64 bp = 0, bg = 0;
      if (y >= 0 && y < H) {
        const long long xw = (long long)(wx0 + w - 1) * 64;
        const u64 in = cols_below(xw, W);
        const u64 xe = cols_below(xw, (long long)W - 1);   // columns with a right neighbour
        const bool down = y < H - 1;
        const size_t i0 = o * plane + (size_t)r * lw + w;
        const bool has_next = w + 1 < lw;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          const u64* sg = m == 0 ? segP : segG;
          const u64 s = sg[i0];
          const u64 e = (s >> 1) | (has_next ? sg[i0 + 1] << 63 : 0ull);
          const u64 ss = sg[i0 + lw];
          const u64 se = (ss >> 1) | (has_next ? sg[i0 + lw + 1] << 63 : 0ull);
          u64 b = (s ^ e) & xe;
          if (down) b |= (s ^ ss) | ((s ^ se) & xe);
          b &= in;
          if (m == 0) bp = b; else bg = b;
        }
      }
      bndP[o * plane + (size_t)r * lw + w] = bp;
      bndG[o * plane + (size_t)r * lw + w] = bg;
    }
    __syncthreads();

    // ---- C: boundary counts and matches of the own words
    for (int cell = tid; cell < own_rows * own_words; cell += DV_THREADS) {
      const int ro = cell / own_words, wo = cell - ro * own_words;
#pragma unroll
      for (int o = 0; o < DV_OC; ++o) {
        if (o < oc) {
          const size_t base = o * plane;
          const size_t at = base + (size_t)(ro + el.ay) * lw + wo + 1;
          const u64 fb = bndP[at], gb = bndG[at];
          cnt[o][2] += __popcll(fb);
          cnt[o][3] += __popcll(gb);
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            const u64 mine = m == 0 ? fb : gb;
            if (!mine) continue;
            const u64* other = m == 0 ? bndG : bndP;
            u64 dil = 0;
            for (int i = 0; i < el.rows; ++i) {
              const int lo = el.lo[i], hi = el.hi[i];
              if (lo > hi) continue;
              const size_t q = base + (size_t)(ro + i) * lw + wo;   // row y + i - ay of the boundary, words wo - 1 .. wo + 1
              const u64 L = other[q], C = other[q + 1], R = other[q + 2];
              if (!(L | C | R)) continue;
              dil |= row_dilate(L, C, R, lo, hi, el.ax);
              if (!(mine & ~dil)) break;   // every boundary pixel of this word is matched already
            }
            cnt[o][4 + m] += __popcll(mine & dil);
          }
        }
      }
    }

    // ---- one integer atomic per counter per tile
#pragma unroll
    for (int o = 0; o < DV_OC; ++o)
#pragma unroll
      for (int c = 0; c < DV_NCNT; ++c) {
        int v = cnt[o][c];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) red[wave][o * DV_NCNT + c] = v;
      }
    __syncthreads();
    if (tid < oc * DV_NCNT) {
      int s = 0;
      for (int w = 0; w < DV_WAVES; ++w) s += red[w][tid];
      const int o = tid / DV_NCNT, c = tid - o * DV_NCNT;
      if (s) atomicAdd(reinterpret_cast<u64*>(out) + ((size_t)(obj0 + o) * T + t) * DV_NCNT + c, (u64)s);
    }
    __syncthreads();   // the next pass rewrites the LDS planes and red
  }
}

__global__ void davis_seg2bmap_kernel(const uint8_t* __restrict__ seg, uint8_t* __restrict__ bmap, long long total, int H, int W) {
  const long long HW = (long long)H * W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long f = i / HW;
    const long long p = i - f * HW;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const uint8_t* s = seg + f * HW;
    const bool c = s[p] != 0;
    const bool right = x < W - 1, down = y < H - 1;
    bool b = false;
    if (right) b = c != (s[p + 1] != 0);
    if (down) b = b || c != (s[p + W] != 0);
    if (right && down) b = b || c != (s[p + W + 1] != 0);
    bmap[i] = b ? 1 : 0;
  }
}

// TH rows x ow words per tile: TH = 32 and up to 8 words, smaller where the LDS planes of a large element would not fit the budget
static bool davis_tiling(int H, int W, int rows, int oc, int& TH, int& ow, size_t& lds) {
  const int words = (W + 63) / 64;
  int tx = (words + 7) / 8;
  ow = (words + tx - 1) / tx;
  TH = H < 32 ? H : 32;
  for (;;) {
    lds = (size_t)4 * oc * (TH + rows) * (ow + 2) * sizeof(u64);
    if (lds <= DV_LDS_BUDGET) return true;
    if (TH > 8) TH /= 2;
    else if (ow > 1) --ow;
    else return false;
  }
}

static unsigned grid_for_bytes(long long total) {
  long long b = (total + DV_THREADS - 1) / DV_THREADS;
  return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

}  // namespace tt

using namespace tt;

extern "C" int tt_davis_jf_counts(const void* pred, int pred_dtype, const void* gt, int gt_dtype, const uint8_t* void_mask, long long* counts,
                                  int T, int H, int W, int O, const int* spans, int el_rows, int el_cols, int anchor_y, int anchor_x,
                                  tt_stream_t stream) {
  TT_REQUIRE(pred && gt && counts && spans, "davis_jf_counts: pred, gt, counts and spans are required");
  TT_REQUIRE((pred_dtype == 0 || pred_dtype == 1) && (gt_dtype == 0 || gt_dtype == 1),
             "davis_jf_counts: label dtypes are 0 (uint8) or 1 (int64) (got %d, %d)", pred_dtype, gt_dtype);
  TT_REQUIRE(T >= 1 && H >= 1 && W >= 1 && O >= 1 && (long long)H * W <= (1LL << 31),
             "davis_jf_counts: need T, H, W, O >= 1 and H * W <= 2^31 (got %d, %d, %d, %d)", T, H, W, O);
  TT_REQUIRE(el_rows >= 1 && el_rows <= DV_MAX_EL && el_cols >= 1 && el_cols <= DV_MAX_EL,
             "davis_jf_counts: the structuring element is %d x %d; at most %d x %d is supported", el_rows, el_cols, DV_MAX_EL, DV_MAX_EL);
  TT_REQUIRE(anchor_y >= 0 && anchor_y < el_rows && anchor_x >= 0 && anchor_x < el_cols && anchor_x <= 63 && el_cols - 1 - anchor_x <= 63,
             "davis_jf_counts: anchor (%d, %d) outside the element or more than 63 columns from either side", anchor_y, anchor_x);
  DavisElement el;
  el.rows = el_rows;
  el.cols = el_cols;
  el.ay = anchor_y;
  el.ax = anchor_x;
  for (int i = 0; i <= DV_MAX_EL; ++i) {
    el.lo[i] = 1;
    el.hi[i] = 0;
  }
  for (int i = 0; i < el_rows; ++i) {
    const int lo = spans[2 * i], hi = spans[2 * i + 1];
    TT_REQUIRE(lo > hi || (lo >= 0 && hi < el_cols), "davis_jf_counts: span %d of row %d outside the %d columns", lo, i, el_cols);
    el.lo[i] = (signed char)(lo > hi ? 1 : lo);
    el.hi[i] = (signed char)(lo > hi ? 0 : hi);
  }
  const int oc = O < DV_OC ? O : DV_OC;
  int TH, ow;
  size_t lds;
  TT_REQUIRE(davis_tiling(H, W, el_rows, oc, TH, ow, lds), "davis_jf_counts: no tiling fits the LDS budget");
  const int tiles_y = (H + TH - 1) / TH;
  const int tiles_x = ((W + 63) / 64 + ow - 1) / ow;
  const long long blocks = (long long)T * tiles_y * tiles_x;
  TT_REQUIRE(blocks <= 0x7fffffffLL, "davis_jf_counts: %lld workgroups", blocks);
  hipStream_t s = as_stream(stream);
  if (hipMemsetAsync(counts, 0, sizeof(long long) * DV_NCNT * (size_t)O * T, s) != hipSuccess) {
    set_error("davis_jf_counts: clearing the counts failed");
    return TT_ELAUNCH;
  }
  const dim3 grid((unsigned)blocks), block(DV_THREADS);
  const uint8_t* p8 = static_cast<const uint8_t*>(pred);
  const int64_t* p64 = static_cast<const int64_t*>(pred);
  const uint8_t* g8 = static_cast<const uint8_t*>(gt);
  const int64_t* g64 = static_cast<const int64_t*>(gt);
  if (pred_dtype == 0 && gt_dtype == 0)
    hipLaunchKernelGGL((davis_counts_kernel<uint8_t, uint8_t>), grid, block, lds, s, p8, g8, void_mask, counts, T, H, W, O, TH, ow, tiles_x,
                       tiles_y, el);
  else if (pred_dtype == 0)
    hipLaunchKernelGGL((davis_counts_kernel<uint8_t, int64_t>), grid, block, lds, s, p8, g64, void_mask, counts, T, H, W, O, TH, ow, tiles_x,
                       tiles_y, el);
  else if (gt_dtype == 0)
    hipLaunchKernelGGL((davis_counts_kernel<int64_t, uint8_t>), grid, block, lds, s, p64, g8, void_mask, counts, T, H, W, O, TH, ow, tiles_x,
                       tiles_y, el);
  else
    hipLaunchKernelGGL((davis_counts_kernel<int64_t, int64_t>), grid, block, lds, s, p64, g64, void_mask, counts, T, H, W, O, TH, ow, tiles_x,
                       tiles_y, el);
  TT_CHECK_LAUNCH("davis_jf_counts");
  return TT_OK;
}

extern "C" int tt_davis_seg2bmap(const uint8_t* seg, uint8_t* bmap, int T, int H, int W, tt_stream_t stream) {
  TT_REQUIRE(seg && bmap, "davis_seg2bmap: bad arguments");
  TT_REQUIRE(T >= 1 && H >= 1 && W >= 1 && (long long)H * W <= (1LL << 31), "davis_seg2bmap: need T, H, W >= 1 (got %d, %d, %d)", T, H, W);
  const long long total = (long long)T * H * W;
  hipLaunchKernelGGL(davis_seg2bmap_kernel, dim3(grid_for_bytes(total)), dim3(DV_THREADS), 0, as_stream(stream), seg, bmap, total, H, W);
  TT_CHECK_LAUNCH("davis_seg2bmap");
  return TT_OK;
}
