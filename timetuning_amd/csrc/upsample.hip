// Bilinear up-sampling of token-major maps (align_corners = False), every form of it the evaluators use:
//
//   tt_upsample_bilinear_tokens   [M, g*g, C] -> [M, R*R, C]: fp64 arithmetic on fp32 data like the reference's DoubleTensor pass
//                                 (clustering.cluster_features, clustering.py:20-117)
//   tt_upsample_argmax (_hw)      fp64 maps -> arg-max labels, the evaluation tail of mask_propagation.py:826-829 - fused, so the
//                                 [M, K, R, R] fp64 tensor (77 MB per 25-frame clip at K = 8) is never written; _hw takes a gh x gw
//                                 grid and an H x W output (N9: rows and columns scale separately)
//   tt_upsample_argmax_f32        fp32 scores -> labels, interpolation in fp32 like F.interpolate on a float tensor
//                                 (proto_clustering, clustering.py:101-103)
//   tt_upsample_argmax_hist_f32   the histogram of those labels without the labels (N17)
//
// One rule: the taps and weights are interp.hpp's lin_tap, the per-pixel blend and first maximum its bilinear_argmax.  The three
// arg-max entries are ONE kernel template over the arithmetic type, and the histogram kernel calls the same statement, so its labels
// are the label kernel's by construction.
#include "common.hpp"
#include "interp.hpp"

namespace tt {

constexpr int UP_THREADS = 256;
constexpr int UP_MAXM = 65535;    // maps of one up-sampling launch (they ride on gridDim.y)

// The label of output pixel (oy, ox) of one gh x gw x K map.  area_pixel_compute_scale, align_corners = False: input / output size per
// axis; a square map on a square output divides once (the branch is uniform over the launch, the quotient the same number).
template <typename T>
__device__ __forceinline__ int upsample_label(const T* __restrict__ map, int gh, int gw, int K, int H, int W, int oy, int ox) {
  const T scale_y = (T)gh / (T)H;
  const T scale_x = (gh == gw && H == W) ? scale_y : (T)gw / (T)W;
  const LinTap<T> y = lin_tap<T>(oy, scale_y, gh), x = lin_tap<T>(ox, scale_x, gw);
  // (cell and K are non-negative 32-bit numbers: said with unsigned casts, a tap's offset is one 32 x 32 -> 64 bit multiply-add)
  const auto tap = [&](int iy, int ix) { return map + (size_t)(unsigned)(iy * gw + ix) * (unsigned)K; };
  const T *p00 = tap(y.i0, x.i0), *p01 = tap(y.i0, x.i1), *p10 = tap(y.i1, x.i0), *p11 = tap(y.i1, x.i1);
  return bilinear_argmax<T>(p00, p01, p10, p11, T(1) - y.l, y.l, T(1) - x.l, x.l, K);
}

// fp32 in / out, fp64 arithmetic: one workgroup per output pixel, the threads over the channels
__global__ __launch_bounds__(UP_THREADS) void upsample_tokens_kernel(const float* __restrict__ x, float* __restrict__ out, int g, int C,
                                                                     int R) {
  const int pix = blockIdx.x, m = blockIdx.y;
  const int oy = pix / R, ox = pix - oy * R;
  const double scale = (double)g / (double)R;
  const LinTap<double> ty = lin_tap<double>(oy, scale, g), tx = lin_tap<double>(ox, scale, g);
  const double ly = ty.l, lx = tx.l, hy = 1.0 - ly, hx = 1.0 - lx;
  const float* base = x + (size_t)m * g * g * C;
  const float* p00 = base + (size_t)(ty.i0 * g + tx.i0) * C;
  const float* p01 = base + (size_t)(ty.i0 * g + tx.i1) * C;
  const float* p10 = base + (size_t)(ty.i1 * g + tx.i0) * C;
  const float* p11 = base + (size_t)(ty.i1 * g + tx.i1) * C;
  float* o = out + ((size_t)m * R * R + pix) * C;
  for (int c = threadIdx.x; c < C; c += blockDim.x)
    o[c] = (float)(hy * (hx * (double)p00[c] + lx * (double)p01[c]) + ly * (hx * (double)p10[c] + lx * (double)p11[c]));
}

// maps [M, gh*gw, K] -> labels [M, H, W] int64: one thread per output pixel, the maps on gridDim.y.  H * W fits 31 bits (the entries
// check), so the pixel index and its division stay 32-bit.
template <typename T>
__global__ __launch_bounds__(UP_THREADS) void upsample_argmax_kernel(const T* __restrict__ maps, int64_t* __restrict__ out, int gh, int gw,
                                                                     int K, int H, int W) {
  const unsigned pixels = (unsigned)(H * W), pix = blockIdx.x * (unsigned)UP_THREADS + threadIdx.x;
  if (pix >= pixels) return;
  const int m = blockIdx.y, oy = (int)(pix / (unsigned)W), ox = (int)(pix - (unsigned)oy * (unsigned)W);
  out[(size_t)m * pixels + pix] = upsample_label<T>(maps + (size_t)m * gh * gw * K, gh, gw, K, H, W, oy, ox);
}

// ---- N17: the histogram of upsample_argmax_kernel<float>'s labels without the labels (time_tuning.get_similarity_histogram,
// time_tuning.py:354-375: the reference builds every [224, 224] map on the host and calls torch.histc on it).  counts[k] += the number of
// output pixels whose bilinear arg-max is k.  The per-pixel statement IS the label kernel's (upsample_label), so a pixel gets the label
// that kernel gives it.  Counting follows confusion.hip: a u32 histogram of K bins per workgroup in LDS, a grid-stride walk
// over the M * R * R pixels, equal consecutive labels merged into one LDS add per run (arg-max maps are piecewise constant, and equal
// keys serialise on one LDS address), and one 64-bit global integer atomic per non-zero bin at the end.  Integer atomics only: the
// result depends neither on the order nor on the grid.
// Runs are merged ACROSS THE LANES of a wave, not along a strip of one thread: a lane takes one pixel, consecutive lanes consecutive
// pixels - the load pattern of the label kernel, four or five token rows per wave and instruction - and the first lane of every run
// (one ballot of "my label differs from the lane before me") adds the run's length, the distance to the next such lane.  The form
// confusion.hip uses, a strip of 8 consecutive pixels per thread merged in registers, was built first and measured: lanes 8 pixels
// apart touch some 32 token rows per load instruction, and the launch took 3.15 ms at (64, 14, 200, 224) where the label kernel and
// torch.bincount together take 0.50 ms.  confusion.hip streams labels it reads once; here a pixel costs 4 K loads.
constexpr int UH_MAX_K = 16384;                    // u32 bins of the LDS histogram: 64 KB, confusion.hip's limit
#ifndef TT_UH_MAX_GRID       // (the three constants of the grid rule can be set from the command line for A/B builds: tools/build_variant.sh)
#define TT_UH_MAX_GRID 65536
#endif
#ifndef TT_UH_MIN_ROUNDS
#define TT_UH_MIN_ROUNDS 1
#endif
#ifndef TT_UH_BIN_FACTOR
#define TT_UH_BIN_FACTOR 0
#endif
constexpr long long UH_MAX_GRID = TT_UH_MAX_GRID;  // workgroups, unless the 2^31 bound below asks for more
constexpr long long UH_MAX_PER_WG = 1ll << 31;     // pixels a workgroup walks at most: a 32-bit bin cannot wrap

// Workgroups for `pixels` pixels and K bins: cs_blocks' rule (confusion.hip) with other constants.  There a workgroup walks at least four
// rounds and four elements per bin, because zeroing and flushing the bins is its fixed cost beside elements that cost one load each.
// Here a pixel costs 4 K loads, the bins K / 256 stores and loads per thread: the fixed cost is nothing at any K, and the launch is
// faster the finer it is cut (measured, profiles/n17_overlay.txt: one round of UP_THREADS pixels per workgroup 0.43 ms, four rounds and
// four pixels per bin under a cap of 2048 workgroups 0.46 ms, the rounds dealt evenly over 1792 workgroups 0.48 ms - the workgroups
// do not take equally long, and a finer grid lets the dispatcher even that out).  So: one round each up to UH_MAX_GRID workgroups, more
// rounds beyond, and never more than UH_MAX_PER_WG pixels - then the grid grows instead.  A workgroup walks whole rounds: at most
// per + UP_THREADS < 2^32 pixels.
static unsigned uh_blocks(long long pixels, int K) {
  const long long rounds = (long long)TT_UH_MIN_ROUNDS * UP_THREADS, bins = (long long)TT_UH_BIN_FACTOR * K;
  long long per = rounds > bins ? rounds : bins;
  const long long spread = (pixels + UH_MAX_GRID - 1) / UH_MAX_GRID;
  if (per < spread) per = spread;
  if (per > UH_MAX_PER_WG) per = UH_MAX_PER_WG;
  const long long blocks = (pixels + per - 1) / per;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

__global__ __launch_bounds__(UP_THREADS) void upsample_argmax_hist_f32_kernel(const float* __restrict__ maps,
                                                                              unsigned long long* __restrict__ counts, int g, int K, int R,
                                                                              long long pixels) {
  extern __shared__ unsigned int uh_hist[];
  for (int i = threadIdx.x; i < K; i += UP_THREADS) uh_hist[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  // every thread of the workgroup makes the same number of rounds (the ballot below needs whole waves); a lane past the end holds -1
  for (long long round = (long long)blockIdx.x * UP_THREADS; round < pixels; round += (long long)gridDim.x * UP_THREADS) {
    const long long i = round + threadIdx.x;
    int label = -1;
    if (i < pixels) {
      const long long m = i / ((long long)R * R);
      const int pix = (int)(i - m * R * R);
      const int oy = pix / R, ox = pix - oy * R;
      label = upsample_label<float>(maps + (size_t)m * g * g * K, g, g, K, R, R, oy, ox);
    }
    const int before = __shfl_up(label, 1, kWave);
    const bool first = lane == 0 || label != before;          // the first lane of a run of equal labels
    const unsigned long long firsts = __ballot(first);
    if (first && label >= 0) {
      const unsigned long long above = (firsts >> lane) >> 1;   // the run ends where the next one starts, or with the wave
      const unsigned int c = above ? (unsigned int)__ffsll((long long)above) : (unsigned int)(kWave - lane);
      atomicAdd(&uh_hist[label], c);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K; i += UP_THREADS) {
    const unsigned int c = uh_hist[i];
    if (c) atomicAdd(&counts[i], (unsigned long long)c);
  }
}

template <typename T>
static void launch_upsample_argmax(const T* maps, int64_t* labels_out, int M, int gh, int gw, int K, int H, int W, tt_stream_t stream) {
  const unsigned blocks = (unsigned)(((long long)H * W + UP_THREADS - 1) / UP_THREADS);
  hipLaunchKernelGGL(upsample_argmax_kernel<T>, dim3(blocks, M), dim3(UP_THREADS), 0, as_stream(stream), maps, labels_out, gh, gw, K, H, W);
}

}  // namespace tt

using namespace tt;

extern "C" int tt_upsample_bilinear_tokens(const float* x, float* out, int M, int g, int C, int R, tt_stream_t stream) {
  TT_REQUIRE(x && out && M > 0 && g > 0 && C > 0 && R > 0, "upsample_bilinear_tokens: bad arguments");
  TT_REQUIRE(M <= UP_MAXM && R <= 32768, "upsample_bilinear_tokens: %d maps of %dx%d exceed one launch (at most %d maps)", M, R, R, UP_MAXM);
  const int threads = C >= 256 ? 256 : (C > 64 ? 128 : 64);
  hipLaunchKernelGGL(upsample_tokens_kernel, dim3(R * R, M), dim3(threads), 0, as_stream(stream), x, out, g, C, R);
  TT_CHECK_LAUNCH("upsample_bilinear_tokens");
  return TT_OK;
}

extern "C" int tt_upsample_argmax(const double* maps, int64_t* labels_out, int M, int g, int K, int R, tt_stream_t stream) {
  TT_REQUIRE(maps && labels_out && M > 0 && g > 0 && K > 0 && R > 0, "upsample_argmax: bad arguments");
  TT_REQUIRE(M <= 65535 && R <= 32768, "upsample_argmax: %d maps of %dx%d exceed one launch (at most 65535 maps)", M, R, R);
  launch_upsample_argmax<double>(maps, labels_out, M, g, g, K, R, R, stream);
  TT_CHECK_LAUNCH("upsample_argmax");
  return TT_OK;
}

extern "C" int tt_upsample_argmax_hw(const double* maps, int64_t* labels_out, int M, int gh, int gw, int K, int H, int W, tt_stream_t stream) {
  TT_REQUIRE(maps && labels_out && M > 0 && gh > 0 && gw > 0 && K > 0 && H > 0 && W > 0, "upsample_argmax_hw: bad arguments");
  TT_REQUIRE(M <= 65535 && (long long)H * W <= 0x7fffffffLL, "upsample_argmax_hw: %d maps of %dx%d exceed one launch", M, H, W);
  launch_upsample_argmax<double>(maps, labels_out, M, gh, gw, K, H, W, stream);
  TT_CHECK_LAUNCH("upsample_argmax_hw");
  return TT_OK;
}

extern "C" int tt_upsample_argmax_f32(const float* maps, int64_t* labels_out, int M, int g, int K, int R, tt_stream_t stream) {
  TT_REQUIRE(maps && labels_out && M > 0 && g > 0 && K > 0 && R > 0, "upsample_argmax_f32: bad arguments");
  TT_REQUIRE(M <= UP_MAXM && R <= 32768, "upsample_argmax_f32: %d maps of %dx%d exceed one launch (at most %d maps)", M, R, R, UP_MAXM);
  launch_upsample_argmax<float>(maps, labels_out, M, g, g, K, R, R, stream);
  TT_CHECK_LAUNCH("upsample_argmax_f32");
  return TT_OK;
}

extern "C" int tt_upsample_argmax_hist_f32(const float* maps, unsigned long long* counts, int M, int g, int K, int R, tt_stream_t stream) {
  TT_REQUIRE(maps && counts, "upsample_argmax_hist_f32: null pointer");
  TT_REQUIRE(M > 0 && g > 0 && K > 0 && R > 0, "upsample_argmax_hist_f32: M = %d maps of %d x %d x %d to %d x %d: need all > 0", M, g, g, K, R, R);
  TT_REQUIRE(K <= UH_MAX_K, "upsample_argmax_hist_f32: K = %d bins exceed the %d a workgroup holds in LDS", K, UH_MAX_K);
  TT_REQUIRE(M <= UP_MAXM && R <= 32768 && g <= 32768, "upsample_argmax_hist_f32: %d maps of %dx%d to %dx%d: at most %d maps, sides up to 32768", M, g,
             g, R, R, UP_MAXM);
  TT_REQUIRE(reinterpret_cast<uintptr_t>(counts) % 8 == 0, "upsample_argmax_hist_f32: counts must be 8-byte aligned");
  const long long pixels = (long long)M * R * R;
  hipLaunchKernelGGL(upsample_argmax_hist_f32_kernel, dim3(uh_blocks(pixels, K)), dim3(UP_THREADS), sizeof(unsigned int) * (size_t)K,
                     as_stream(stream), maps, counts, g, K, R, pixels);
  TT_CHECK_LAUNCH("upsample_argmax_hist_f32");
  return TT_OK;
}
