// Overlay rendering (N17): the qualitative side of the reference - time_tuning.make_overlayed_grid / localize_objects
// (time_tuning.py:305-341: frame beside frame blended with its coloured cluster map) and the ground-truth / prediction panels of
// evaluation.evaluate_localizations' GIFs (evaluation.py:271-272,288,293 through my_utils.localize_objects, my_utils.py:41-65) - for
// ALL frames of a batch in one launch, as finished uint8 grids.
//
// The reference renders on the host, frame by frame: a .cpu() of the float frame and of the int64 map, torchvision's
// draw_segmentation_masks on a full one-hot mask, make_grid, then a matplotlib figure saved to PNG and decoded again.  Here the frames,
// the cluster maps and the matching tables are on the device already, and what leaves it is the grid.
//
//   out uint8 [F, 3, H + 2 pad, n W + (n + 1) pad]: torchvision.utils.make_grid's layout for n tiles in one row - pad value 0, tile t
//   at column t (W + pad) + pad, row pad.
//     TT_OVERLAY_PHOTO   n = 2   [base | blend(base, colour(A))]
//     TT_OVERLAY_LABELS  n = 3   [colour(B) | colour(A) | blend(colour(B), colour(A))]      (B the ground truth, A the prediction)
//   base_c  = (uint8) clamp(trunc((x_c * std_c + mean_c) * 255), 0, 255), NaN -> 0: my_utils.denormalize followed by
//             (img * 255).type(torch.uint8) wherever torch's cast is defined; three rounded fp32 operations.
//   colour  = palette[idx mod P] (a true modulo: negative indices wrap), idx = lut[f * lut_stride + v] for the labels A where a LUT is
//             given (a v outside [0, lut_len) gives idx 0), else idx = v.  The LUT is the matching pred value -> gt value: B, the ground
//             truth, is never mapped.
//   blend   = (uint8) trunc(fl(fl(a (1 - alpha)) + fl(b alpha))): draw_segmentation_masks' img * (1 - alpha) + colour * alpha and its
//             .to(uint8) with every pixel masked; three rounded fp32 operations, contraction switched off (ov_blend).
//   Label maps [F, Hl, Wl] of uint8, int16 or int64; where (Hl, Wl) != (H, W) they are read through ytab[H] / xtab[W] (nearest gather).
//
// Kernel: the idiom of gather_nearest_u8_kernel (image_ops.hip).  A thread owns one 16-byte-ALIGNED piece of an output row, found from
// the row's own address, so rows of any width and any start get one global_store_dwordx4 in their interior and byte stores at their two
// ends only.  The padding is written by the same threads.  Offsets are 64-bit.  No LDS, no atomics, no workspace.
#include "common.hpp"

namespace tt {

constexpr int OV_THREADS = 256;
constexpr long long OV_MAX_BLOCKS = 1 << 20;   // the grid strides beyond (2^28 pieces = 4 GB of output per pass)

struct OverlayArgs {
  const float* frames;           // [F, 3, H, W] or null (LABELS)
  const void* a;                 // [F, Hl, Wl]
  const void* b;                 // [F, Hl, Wl] or null (PHOTO)
  const int* ytab;               // [H] or null: rows of the label maps
  const int* xtab;               // [W] or null
  const int* lut;                // [lut_len] (lut_stride 0) or [F, lut_stride] or null
  const unsigned char* palette;  // [P, 3]
  float mean[3], std[3];
  float alpha, one_minus_alpha;
  int lut_len, lut_stride, P;
  int H, W, Hl, Wl, pad, n;
  long long rows;                // F * 3 * OH
  int OH, OW, nseg;
};

template <typename T>
__device__ __forceinline__ long long ov_label(const void* map, long long off) {
  return (long long)static_cast<const T*>(map)[off];
}

template <typename LabelT, bool MAPPED>   // MAPPED: through the LUT where one is given (labels A; the ground truth B never is)
__device__ __forceinline__ unsigned ov_colour(const OverlayArgs& p, const void* map, long long f, long long off, int c) {
  long long idx = ov_label<LabelT>(map, off);
  if (MAPPED && p.lut) idx = (idx >= 0 && idx < p.lut_len) ? (long long)p.lut[f * p.lut_stride + idx] : 0;
  long long m;
  if ((unsigned long long)idx <= 0x7fffffffull) {   // what labels are: a 32-bit remainder instead of the 64-bit division sequence
    m = (int)idx % p.P;
  } else {
    m = idx % p.P;
    if (m < 0) m += p.P;
  }
  return p.palette[m * 3 + c];
}

// The two arithmetic statements are torch's: one rounding per operation.  hipcc contracts a * b + c into a fused multiply-add by default,
// and this toolchain's __fmul_rn / __fadd_rn are plain x * y / x + y that contract like any other once inlined (a labels-mode pixel at
// alpha 0.3 came out one off through them); `#pragma clang fp contract(off)` takes the contraction flag off the operations written
// inside the block, wherever they are inlined.
__device__ __forceinline__ unsigned ov_base(const OverlayArgs& p, long long f, int c, int y, int x) {
#pragma clang fp contract(off)
  const float v = p.frames[((f * 3 + c) * p.H + y) * (long long)p.W + x];
  const float scaled = v * p.std[c];
  const float shifted = scaled + p.mean[c];
  const float t = truncf(shifted * 255.0f);
  return t >= 255.0f ? 255u : (t > 0.0f ? (unsigned)t : 0u);   // NaN fails both comparisons: 0
}

__device__ __forceinline__ unsigned ov_blend(const OverlayArgs& p, unsigned a, unsigned b) {
#pragma clang fp contract(off)
  const float wa = (float)a * p.one_minus_alpha;
  const float wb = (float)b * p.alpha;
  return (unsigned)(wa + wb);   // <= 255: alpha in [0, 1]
}

template <typename LabelT, bool PHOTO>
__global__ __launch_bounds__(OV_THREADS) void overlay_grid_kernel(unsigned char* __restrict__ out, const OverlayArgs p, long long items) {
  const int tile_w = p.W + p.pad;
  for (long long item = (long long)blockIdx.x * OV_THREADS + threadIdx.x; item < items; item += (long long)gridDim.x * OV_THREADS) {
    const long long r = item / p.nseg;
    const int k = (int)(item - r * p.nseg);
    const long long fc = r / p.OH, f = fc / 3;
    const int oy = (int)(r - fc * p.OH), c = (int)(fc - f * 3);
    unsigned char* orow = out + r * p.OW;
    const int mis = (int)(reinterpret_cast<uintptr_t>(orow) & 15u);
    const long long s = (long long)k * 16 - mis;   // 64 bits: the last piece of a row of nearly 2^31 bytes ends beyond INT_MAX
    if (s >= p.OW) continue;   // the spare piece of a row that starts on a boundary
    const int b0 = s < 0 ? 0 : (int)s;
    const int b1 = s + 16 < p.OW ? (int)(s + 16) : p.OW;
    const int y = oy - p.pad;
    const bool row_in = y >= 0 && y < p.H;
    const int ly = row_in ? (p.ytab ? p.ytab[y] : y) : 0;
    const long long lrow = (f * p.Hl + ly) * (long long)p.Wl;
    int t = b0 / tile_w, within = b0 - t * tile_w;   // tile and column inside [pad | W columns]
    auto next = [&]() -> unsigned {
      unsigned v = 0;
      if (row_in && t < p.n && within >= p.pad) {
        const int x = within - p.pad;
        const long long off = lrow + (p.xtab ? p.xtab[x] : x);
        if (PHOTO) {
          v = ov_base(p, f, c, y, x);
          if (t == 1) v = ov_blend(p, v, ov_colour<LabelT, true>(p, p.a, f, off, c));
        } else if (t == 0) {
          v = ov_colour<LabelT, false>(p, p.b, f, off, c);
        } else if (t == 1) {
          v = ov_colour<LabelT, true>(p, p.a, f, off, c);
        } else {
          v = ov_blend(p, ov_colour<LabelT, false>(p, p.b, f, off, c), ov_colour<LabelT, true>(p, p.a, f, off, c));
        }
      }
      if (++within == tile_w) {
        within = 0;
        ++t;
      }
      return v;
    };
    if (b1 - b0 == 16) {
      unsigned w[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        unsigned v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) v |= next() << (8 * j);
        w[q] = v;
      }
      *reinterpret_cast<uint4*>(orow + b0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      for (int b = b0; b < b1; ++b) orow[b] = (unsigned char)next();
    }
  }
}

template <typename LabelT>
static void ov_launch(bool photo, dim3 grid, hipStream_t s, unsigned char* out, const OverlayArgs& p, long long items) {
  if (photo)
    hipLaunchKernelGGL((overlay_grid_kernel<LabelT, true>), grid, dim3(OV_THREADS), 0, s, out, p, items);
  else
    hipLaunchKernelGGL((overlay_grid_kernel<LabelT, false>), grid, dim3(OV_THREADS), 0, s, out, p, items);
}

}  // namespace tt

using namespace tt;

extern "C" int tt_overlay_grid(unsigned char* out, int mode, const float* frames, const float* mean3, const float* std3, const void* labels_a,
                               const void* labels_b, int label_dtype, int Hl, int Wl, const int* ytab, const int* xtab, const int* lut,
                               int lut_len, int lut_stride, const unsigned char* palette, int P, double alpha, int F, int H, int W, int pad,
                               tt_stream_t stream) {
  TT_REQUIRE(mode == TT_OVERLAY_PHOTO || mode == TT_OVERLAY_LABELS, "overlay_grid: mode %d is neither %d (photo) nor %d (labels)", mode,
             TT_OVERLAY_PHOTO, TT_OVERLAY_LABELS);
  const bool photo = mode == TT_OVERLAY_PHOTO;
  TT_REQUIRE(out && labels_a && palette, "overlay_grid: null pointer (out, labels_a, palette)");
  TT_REQUIRE(!photo || frames, "overlay_grid: the photo mode needs the frames");
  TT_REQUIRE(photo || labels_b, "overlay_grid: the labels mode needs labels_b (the ground truth)");
  TT_REQUIRE(label_dtype == TT_LABELS_I16 || label_dtype == TT_LABELS_I64 || label_dtype == TT_LABELS_U8,
             "overlay_grid: label dtype code %d is none of %d (int16), %d (int64), %d (uint8)", label_dtype, TT_LABELS_I16, TT_LABELS_I64,
             TT_LABELS_U8);
  TT_REQUIRE(F > 0 && H > 0 && W > 0, "overlay_grid: F = %d frames of %d x %d: need all > 0", F, H, W);
  TT_REQUIRE(P > 0, "overlay_grid: a palette of P = %d colours", P);
  TT_REQUIRE(pad >= 0, "overlay_grid: pad = %d", pad);
  TT_REQUIRE(Hl > 0 && Wl > 0, "overlay_grid: label maps of %d x %d", Hl, Wl);
  TT_REQUIRE((ytab && xtab) || (!ytab && !xtab && Hl == H && Wl == W),
             "overlay_grid: label maps of %d x %d under frames of %d x %d need both index tables (and a map of the frames' size none or both)", Hl,
             Wl, H, W);
  TT_REQUIRE(!lut || (lut_len > 0 && (lut_stride == 0 || lut_stride >= lut_len)), "overlay_grid: lut_len = %d, lut_stride = %d", lut_len,
             lut_stride);
  TT_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "overlay_grid: alpha = %g outside [0, 1]", alpha);
  const int n = photo ? 2 : 3;
  const long long OW = (long long)n * W + (long long)(n + 1) * pad, OH = (long long)H + 2ll * pad;
  TT_REQUIRE(OW <= 2147483647ll && OH <= 2147483647ll, "overlay_grid: an output row of %lld bytes (%lld rows): at most 2^31 - 1", OW, OH);
  const size_t lsize = label_dtype == TT_LABELS_I16 ? 2 : (label_dtype == TT_LABELS_I64 ? 8 : 1);
  TT_REQUIRE(reinterpret_cast<uintptr_t>(labels_a) % lsize == 0 && (!labels_b || reinterpret_cast<uintptr_t>(labels_b) % lsize == 0) &&
                 (!frames || reinterpret_cast<uintptr_t>(frames) % 4 == 0),
             "overlay_grid: label maps must be aligned to their %zu-byte elements and the frames to 4 bytes", lsize);
  OverlayArgs p;
  p.frames = frames;
  p.a = labels_a;
  p.b = labels_b;
  p.ytab = ytab;
  p.xtab = xtab;
  p.lut = lut;
  p.palette = palette;
  for (int c = 0; c < 3; ++c) {
    p.mean[c] = mean3 ? mean3[c] : 0.f;
    p.std[c] = std3 ? std3[c] : 1.f;
  }
  p.alpha = (float)alpha;
  p.one_minus_alpha = (float)(1.0 - alpha);   // the double difference rounded once, as torch rounds a Python scalar
  p.lut_len = lut ? lut_len : 0;
  p.lut_stride = lut ? lut_stride : 0;
  p.P = P;
  p.H = H;
  p.W = W;
  p.Hl = Hl;
  p.Wl = Wl;
  p.pad = pad;
  p.n = n;
  p.OH = (int)OH;
  p.OW = (int)OW;
  p.rows = (long long)F * 3 * OH;
  p.nseg = (int)((OW + 30) / 16);   // 16-byte pieces of a row whose start may sit anywhere in a piece
  const long long items = p.rows * p.nseg;
  long long blocks = (items + OV_THREADS - 1) / OV_THREADS;
  blocks = blocks > OV_MAX_BLOCKS ? OV_MAX_BLOCKS : blocks;
  const dim3 grid((unsigned)blocks);
  hipStream_t s = as_stream(stream);
  if (label_dtype == TT_LABELS_I16)
    ov_launch<int16_t>(photo, grid, s, out, p, items);
  else if (label_dtype == TT_LABELS_I64)
    ov_launch<int64_t>(photo, grid, s, out, p, items);
  else
    ov_launch<unsigned char>(photo, grid, s, out, p, items);
  TT_CHECK_LAUNCH("overlay_grid");
  return TT_OK;
}
