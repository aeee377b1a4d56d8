// Ragged image kernels (N22): what the Pascal VOC reader (leoloader.pascal_loader) does to a batch of images of DIFFERENT sizes -
// Resize((S, S)) + ToTensor + Normalize for the JPEGs, Resize((R, R), NEAREST) + ToTensor for the palette PNGs - as ONE launch per
// batch for the images and one for the masks.  image_ops.hip's kernels take one [F, H, W] shape per call; here a descriptor row per
// item (tt_img_ragged_item) carries the item's place in a byte buffer, its size, a crop box, a flip and its offsets into one int32
// pool of taps / bounds / index tables, and blockIdx.y is the item.
//   resize_ragged_kernel   crop(box).resize((OW, OH), BILINEAR) with Resample.c's arithmetic (22-bit taps, uint8 rounding after the
//                          horizontal pass and again after the vertical pass; a pass whose lengths are equal is the identity).  A
//                          workgroup owns one item and a band of RG_BAND output rows: it runs the horizontal pass for the source rows
//                          the band's vertical taps reach into LDS (uint8), then the vertical pass from LDS - the intermediate never
//                          sees HBM.  Output uint8 [B, OH, OW, 3] or the finished float32 [B, 3, OH, OW].
//   gather_ragged_kernel   out[i, y, x] = in_i[ytab_i[y], xtab_i[x]] on label maps, uint8 or (float)v / 255.
// Source offsets are arbitrary bytes (a decoder's out_off, a packed mask buffer): every source read is a byte load.
#include "common.hpp"

#include <climits>

// As in image_ops.hip: Pillow's C code multiplies and adds separately, and the host restatement of precompute_coeffs' bounds below must
// round like the Python one - contraction is off for this whole file.
#pragma clang fp contract(off)

namespace tt {

constexpr int RG_THREADS = 256;
constexpr int RG_BAND = TT_IMG_RAGGED_BAND;         // output rows per workgroup
constexpr int RG_PB = 22;                           // PRECISION_BITS of Resample.c
constexpr long long RG_LDS_BUDGET = TT_IMG_RAGGED_LDS_BUDGET;   // 64 KiB: two workgroups per CU leave 32 of the 160 KiB free
constexpr int RG_MAX_SIDE = 32767;                  // the domain of tt_img_gather_nearest
constexpr int RG_MAX_ITEMS = 65535;                 // the grid's y extent

__device__ __forceinline__ unsigned char rg_clip8(int v) { return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ __launch_bounds__(RG_THREADS) void resize_ragged_kernel(const unsigned char* __restrict__ in, const tt_img_ragged_item* __restrict__ items,
                                                                   const int* __restrict__ pool, unsigned char* __restrict__ out_u8,
                                                                   float* __restrict__ out_f32, int OH, int OW, float m0, float m1, float m2,
                                                                   float s0, float s1, float s2) {
  extern __shared__ unsigned char rg_rows[];   // [rows the band reaches][OW][3], after the horizontal pass
  const tt_img_ragged_item it = items[blockIdx.y];
  const int yb0 = blockIdx.x * RG_BAND, yb1 = min(yb0 + RG_BAND, OH);
  const int W = (int)it.W, x0 = (int)it.x0, y0 = (int)it.y0;
  const bool hpass = (int)it.w != OW, vpass = (int)it.h != OH;
  const int* hk = pool + it.hk_off;
  const int* hb = pool + it.hb_off;
  const int* vk = pool + it.vk_off;
  const int* vb = pool + it.vb_off;
  const int hks = (int)it.hksize, vks = (int)it.vksize;
  // the source rows (of the box) this band reads: bounds[first].ymin .. bounds[last].ymin + cnt for Pillow's tables; min / max over
  // the band's rows for any table the launcher let through
  int lo = yb0, hi = yb1;
  if (vpass) {
    lo = INT_MAX;
    hi = 0;
    for (int yy = yb0; yy < yb1; ++yy) {
      const int ymin = vb[2 * yy], cnt = vb[2 * yy + 1];
      lo = min(lo, ymin);
      hi = max(hi, ymin + cnt);
    }
  }
  const int nrows = hi - lo, stride = OW * 3;
  const unsigned char* src = in + it.src_off;
  for (int idx = threadIdx.x; idx < nrows * OW; idx += RG_THREADS) {
    const int r = idx / OW, xx = idx - r * OW;
    const unsigned char* row = src + ((size_t)(y0 + lo + r) * W + x0) * 3;
    unsigned char* d = rg_rows + r * stride + xx * 3;
    if (hpass) {
      const int xmin = hb[2 * xx], cnt = hb[2 * xx + 1];
      const int* k = hk + (size_t)xx * hks;
      const unsigned char* p = row + (size_t)xmin * 3;
      int a0 = 1 << (RG_PB - 1), a1 = a0, a2 = a0;
      for (int x = 0; x < cnt; ++x) {
        const int wgt = k[x];
        a0 += p[3 * x] * wgt;
        a1 += p[3 * x + 1] * wgt;
        a2 += p[3 * x + 2] * wgt;
      }
      d[0] = rg_clip8(a0 >> RG_PB);
      d[1] = rg_clip8(a1 >> RG_PB);
      d[2] = rg_clip8(a2 >> RG_PB);
    } else {
      const unsigned char* p = row + (size_t)xx * 3;
      d[0] = p[0];
      d[1] = p[1];
      d[2] = p[2];
    }
  }
  __syncthreads();
  const int flip = (int)it.flip;
  const size_t plane = (size_t)OH * OW;
  for (int idx = threadIdx.x; idx < (yb1 - yb0) * OW; idx += RG_THREADS) {
    const int ry = idx / OW, x = idx - ry * OW, yy = yb0 + ry;
    unsigned char r, g, b;
    if (vpass) {
      const int ymin = vb[2 * yy], cnt = vb[2 * yy + 1];
      const int* k = vk + (size_t)yy * vks;
      const unsigned char* p = rg_rows + (ymin - lo) * stride + x * 3;
      int a0 = 1 << (RG_PB - 1), a1 = a0, a2 = a0;
      for (int y = 0; y < cnt; ++y) {
        const int wgt = k[y];
        a0 += p[0] * wgt;
        a1 += p[1] * wgt;
        a2 += p[2] * wgt;
        p += stride;
      }
      r = rg_clip8(a0 >> RG_PB);
      g = rg_clip8(a1 >> RG_PB);
      b = rg_clip8(a2 >> RG_PB);
    } else {
      const unsigned char* p = rg_rows + ry * stride + x * 3;
      r = p[0];
      g = p[1];
      b = p[2];
    }
    const int ox = flip ? OW - 1 - x : x;
    if (out_f32) {   // the expression of resample_v_kernel
      const size_t base = (size_t)blockIdx.y * 3 * plane + (size_t)yy * OW + ox;
      out_f32[base] = ((float)r / 255.0f - m0) / s0;
      out_f32[base + plane] = ((float)g / 255.0f - m1) / s1;
      out_f32[base + 2 * plane] = ((float)b / 255.0f - m2) / s2;
    } else {
      unsigned char* o = out_u8 + ((size_t)blockIdx.y * plane + (size_t)yy * OW + ox) * 3;
      o[0] = r;
      o[1] = g;
      o[2] = b;
    }
  }
}

// one thread per output pixel of one item's label map; (float)v / 255 is one IEEE division (gather_nearest_f32_kernel<1>'s rule)
__global__ __launch_bounds__(RG_THREADS) void gather_ragged_kernel(const unsigned char* __restrict__ in, const tt_img_ragged_item* __restrict__ items,
                                                                   const int* __restrict__ pool, unsigned char* __restrict__ out_u8,
                                                                   float* __restrict__ out_f32, int OH, int OW) {
  const int idx = blockIdx.x * RG_THREADS + threadIdx.x;
  if (idx >= OH * OW) return;
  const tt_img_ragged_item* it = items + blockIdx.y;
  const int y = idx / OW, x = idx - y * OW;
  const int sy = pool[it->ytab_off + y], sx = pool[it->xtab_off + x];
  const unsigned char v = in[it->src_off + (long long)sy * it->W + sx];
  const size_t o = (size_t)blockIdx.y * OH * OW + idx;
  if (out_f32) out_f32[o] = (float)v / 255.0f;
  else out_u8[o] = v;
}

// Resample.c precompute_coeffs' bounds for the bilinear filter, in the double arithmetic of video_transformations.resample_coeffs
static void rg_bounds(int in_size, int out_size, int pos, int* first, int* end) {
  const double scale = (double)in_size / (double)out_size;
  const double support = scale < 1.0 ? 1.0 : scale;
  const double center = ((double)pos + 0.5) * scale;
  long long lo = (long long)(center - support + 0.5), hi = (long long)(center + support + 0.5);
  *first = (int)(lo < 0 ? 0 : lo);
  *end = (int)(hi > in_size ? in_size : hi);
}

static bool rg_sizes_ok(long long h, long long w, long long OH, long long OW) {
  return h >= 1 && w >= 1 && OH >= 1 && OW >= 1 && h <= RG_MAX_SIDE && w <= RG_MAX_SIDE && OH <= RG_MAX_SIDE && OW <= RG_MAX_SIDE;
}

}  // namespace tt

using namespace tt;

extern "C" size_t tt_img_resize_ragged_lds_bytes(int h, int w, int OH, int OW) {
  if (!rg_sizes_ok(h, w, OH, OW)) return 0;
  long long rows = 0;
  for (int yb0 = 0; yb0 < OH; yb0 += RG_BAND) {
    const int yb1 = yb0 + RG_BAND < OH ? yb0 + RG_BAND : OH;
    long long n = yb1 - yb0;
    if (h != OH) {
      int lo, hi, e;
      rg_bounds(h, OH, yb0, &lo, &e);
      rg_bounds(h, OH, yb1 - 1, &e, &hi);
      n = hi - lo;
    }
    rows = n > rows ? n : rows;
  }
  return (size_t)(rows * OW * 3);
}

extern "C" int tt_img_resize_ragged_shape_ok(int h, int w, int OH, int OW) {
  return rg_sizes_ok(h, w, OH, OW) && (long long)tt_img_resize_ragged_lds_bytes(h, w, OH, OW) <= RG_LDS_BUDGET ? 1 : 0;
}

// the checks both entry points share: the item's image inside the buffer, its box inside the image
static int rg_check_item(const char* who, const tt_img_ragged_item* it, int i, long long in_bytes, int channels) {
  TT_REQUIRE(it->H >= 1 && it->W >= 1 && it->H <= RG_MAX_SIDE && it->W <= RG_MAX_SIDE, "%s: item %d: image %lld x %lld outside 1 .. %d", who, i,
             (long long)it->H, (long long)it->W, RG_MAX_SIDE);
  TT_REQUIRE(it->src_off >= 0 && it->src_off <= in_bytes && it->H * it->W * channels <= in_bytes - it->src_off,
             "%s: item %d: offset %lld + %lld x %lld x %d bytes leave the buffer of %lld", who, i, (long long)it->src_off, (long long)it->H,
             (long long)it->W, channels, in_bytes);
  TT_REQUIRE(it->w >= 1 && it->h >= 1 && it->x0 >= 0 && it->y0 >= 0 && it->x0 <= it->W - it->w && it->y0 <= it->H - it->h,
             "%s: item %d: box (%lld, %lld, %lld, %lld) outside the image %lld x %lld", who, i, (long long)it->x0, (long long)it->y0,
             (long long)it->w, (long long)it->h, (long long)it->H, (long long)it->W);
  TT_REQUIRE(it->flip == 0 || it->flip == 1, "%s: item %d: flip must be 0 or 1", who, i);
  return TT_OK;
}

// one pass's taps and bounds: inside the pool, every bounds[...] + cnt inside the box's line of `in_len`
static int rg_check_pass(const tt_img_ragged_item* it, int i, const char* pass, const int32_t* pool, long long pool_len, long long k_off,
                         long long b_off, long long ksize, long long in_len, int out_len) {
  TT_REQUIRE(ksize >= 1 && ksize <= RG_MAX_SIDE * 2 + 3, "img_resize_ragged: item %d: %s ksize %lld", i, pass, ksize);
  TT_REQUIRE(k_off >= 0 && k_off <= pool_len && ksize * out_len <= pool_len - k_off && b_off >= 0 && b_off <= pool_len &&
                 2LL * out_len <= pool_len - b_off,
             "img_resize_ragged: item %d: %s taps at %lld (%d x %lld) / bounds at %lld leave the pool of %lld", i, pass, k_off, out_len, ksize,
             b_off, pool_len);
  const int32_t* b = pool + b_off;
  for (int o = 0; o < out_len; ++o)
    TT_REQUIRE(b[2 * o] >= 0 && b[2 * o + 1] >= 0 && b[2 * o + 1] <= ksize && (long long)b[2 * o] + b[2 * o + 1] <= in_len,
               "img_resize_ragged: item %d: %s bound %d = (%d, %d) reaches outside its box line of %lld (ksize %lld)", i, pass, o, b[2 * o],
               b[2 * o + 1], in_len, ksize);
  return TT_OK;
}

extern "C" int tt_img_resize_ragged(const uint8_t* in, long long in_bytes, const tt_img_ragged_item* items, const tt_img_ragged_item* items_dev,
                                    int n_items, const int32_t* pool, const int32_t* pool_dev, long long pool_len, uint8_t* out_u8,
                                    float* out_f32, int OH, int OW, const float* mean3, const float* std3, tt_stream_t stream) {
  TT_REQUIRE(in && items && items_dev && pool && pool_dev && (out_u8 != nullptr) != (out_f32 != nullptr),
             "img_resize_ragged: null pointer, or not exactly one output buffer");
  TT_REQUIRE(!out_f32 || (mean3 && std3), "img_resize_ragged: the float output needs mean and std (host pointers to 3 floats)");
  TT_REQUIRE(!out_f32 || (reinterpret_cast<uintptr_t>(out_f32) & 3u) == 0, "img_resize_ragged: the float output must be 4-byte aligned");
  TT_REQUIRE(n_items >= 1 && n_items <= RG_MAX_ITEMS && in_bytes >= 1 && pool_len >= 0, "img_resize_ragged: %d items (1 .. %d), %lld bytes",
             n_items, RG_MAX_ITEMS, in_bytes);
  TT_REQUIRE(OH >= 1 && OW >= 1 && OH <= RG_MAX_SIDE && OW <= RG_MAX_SIDE, "img_resize_ragged: output %d x %d outside 1 .. %d", OH, OW, RG_MAX_SIDE);
  long long lds = 16;
  for (int i = 0; i < n_items; ++i) {
    const tt_img_ragged_item* it = items + i;
    if (int rc = rg_check_item("img_resize_ragged", it, i, in_bytes, 3)) return rc;
    if (it->w != OW)
      if (int rc = rg_check_pass(it, i, "horizontal", pool, pool_len, it->hk_off, it->hb_off, it->hksize, it->w, OW)) return rc;
    long long rows = RG_BAND < OH ? RG_BAND : OH;
    if (it->h != OH) {
      if (int rc = rg_check_pass(it, i, "vertical", pool, pool_len, it->vk_off, it->vb_off, it->vksize, it->h, OH)) return rc;
      const int32_t* vb = pool + it->vb_off;
      rows = 0;
      for (int yb0 = 0; yb0 < OH; yb0 += RG_BAND) {
        int lo = INT_MAX, hi = 0;
        for (int yy = yb0; yy < OH && yy < yb0 + RG_BAND; ++yy) {
          lo = vb[2 * yy] < lo ? vb[2 * yy] : lo;
          hi = vb[2 * yy] + vb[2 * yy + 1] > hi ? vb[2 * yy] + vb[2 * yy + 1] : hi;
        }
        rows = hi - lo > rows ? hi - lo : rows;
      }
    }
    const long long need = rows * OW * 3;
    TT_REQUIRE(need <= RG_LDS_BUDGET, "img_resize_ragged: item %d (%lld x %lld -> %d x %d): a band of %d rows reaches %lld source rows = %lld bytes of LDS, "
               "the budget is %lld (tt_img_resize_ragged_shape_ok)", i, (long long)it->h, (long long)it->w, OH, OW, RG_BAND, rows, need, RG_LDS_BUDGET);
    lds = need > lds ? need : lds;
  }
  const float m0 = mean3 ? mean3[0] : 0.f, m1 = mean3 ? mean3[1] : 0.f, m2 = mean3 ? mean3[2] : 0.f;
  const float s0 = std3 ? std3[0] : 1.f, s1 = std3 ? std3[1] : 1.f, s2 = std3 ? std3[2] : 1.f;
  const dim3 grid((unsigned)((OH + RG_BAND - 1) / RG_BAND), (unsigned)n_items);
  hipLaunchKernelGGL(resize_ragged_kernel, grid, dim3(RG_THREADS), (size_t)((lds + 15) / 16 * 16), as_stream(stream), in, items_dev, pool_dev, out_u8,
                     out_f32, OH, OW, m0, m1, m2, s0, s1, s2);
  TT_CHECK_LAUNCH("img_resize_ragged");
  return TT_OK;
}

extern "C" int tt_img_gather_nearest_ragged(const uint8_t* in, long long in_bytes, const tt_img_ragged_item* items,
                                            const tt_img_ragged_item* items_dev, int n_items, const int32_t* pool, const int32_t* pool_dev,
                                            long long pool_len, uint8_t* out_u8, float* out_f32, int OH, int OW, tt_stream_t stream) {
  TT_REQUIRE(in && items && items_dev && pool && pool_dev && (out_u8 != nullptr) != (out_f32 != nullptr),
             "img_gather_nearest_ragged: null pointer, or not exactly one output buffer");
  TT_REQUIRE(!out_f32 || (reinterpret_cast<uintptr_t>(out_f32) & 3u) == 0, "img_gather_nearest_ragged: the float output must be 4-byte aligned");
  TT_REQUIRE(n_items >= 1 && n_items <= RG_MAX_ITEMS && in_bytes >= 1 && pool_len >= 0, "img_gather_nearest_ragged: %d items (1 .. %d), %lld bytes",
             n_items, RG_MAX_ITEMS, in_bytes);
  TT_REQUIRE(OH >= 1 && OW >= 1 && OH <= RG_MAX_SIDE && OW <= RG_MAX_SIDE, "img_gather_nearest_ragged: output %d x %d outside 1 .. %d", OH, OW,
             RG_MAX_SIDE);
  for (int i = 0; i < n_items; ++i) {
    const tt_img_ragged_item* it = items + i;
    if (int rc = rg_check_item("img_gather_nearest_ragged", it, i, in_bytes, 1)) return rc;
    TT_REQUIRE(it->ytab_off >= 0 && it->ytab_off <= pool_len && OH <= pool_len - it->ytab_off && it->xtab_off >= 0 && it->xtab_off <= pool_len &&
                   OW <= pool_len - it->xtab_off,
               "img_gather_nearest_ragged: item %d: tables at %lld / %lld leave the pool of %lld", i, (long long)it->ytab_off,
               (long long)it->xtab_off, pool_len);
    const int32_t *yt = pool + it->ytab_off, *xt = pool + it->xtab_off;
    for (int y = 0; y < OH; ++y)
      TT_REQUIRE(yt[y] >= 0 && yt[y] < it->H, "img_gather_nearest_ragged: item %d: ytab[%d] = %d outside [0, %lld)", i, y, yt[y], (long long)it->H);
    for (int x = 0; x < OW; ++x)
      TT_REQUIRE(xt[x] >= 0 && xt[x] < it->W, "img_gather_nearest_ragged: item %d: xtab[%d] = %d outside [0, %lld)", i, x, xt[x], (long long)it->W);
  }
  const dim3 grid((unsigned)(((long long)OH * OW + RG_THREADS - 1) / RG_THREADS), (unsigned)n_items);
  hipLaunchKernelGGL(gather_ragged_kernel, grid, dim3(RG_THREADS), 0, as_stream(stream), in, items_dev, pool_dev, out_u8, out_f32, OH, OW);
  TT_CHECK_LAUNCH("img_gather_nearest_ragged");
  return TT_OK;
}
