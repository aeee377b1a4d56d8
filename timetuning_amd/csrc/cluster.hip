// Evaluator clustering: the GPU side of clustering.cluster_features / proto_clustering
// (clustering.py:20-117) and my_utils.normalize_and_transform (my_utils.py:19-37) around the k-means, which has its own file (kmeans.hip).
//
// The reference moves every feature map to the host, upsamples it in fp64 with ATen, and runs faiss' CPU Lloyd iterations
// while the other ranks wait at a barrier (time_tuning.py:634-648).  Here the dense passes stay on the device (with kmeans.hip's):
//   column moments (StandardScaler)         one two-stage fp64 reduction over the rows
//   bilinear upsampling of token maps       [M, g*g, C] -> [M, R*R, C], fp64 arithmetic like the reference's DoubleTensor pass
// The tiny dense algebra between them (50 x 384 PCA basis from a 384 x 384 eigen-problem, k x d centroid bookkeeping, the
// Hungarian matching of a k x k score matrix) stays on the host.
#include "common.hpp"

namespace tt {

constexpr int CL_THREADS = 256;
constexpr int CL_MAXD = 1024;     // feature columns for the moments
constexpr int UP_MAXM = 65535;    // maps of one up-sampling launch (they ride on gridDim.y)

// ---- column moments: partial[b][0][c] = sum_r v, partial[b][1][c] = sum_r v^2 over the block's rows (fp64), v = x[r][c] - x[0][c].
// The sums are taken about the column's first row: E[v^2] - E[v]^2 on the raw values subtracts two numbers of size mean^2 and loses a
// small variance beside a large mean even in fp64 (mean 1e4, spread 1e-2 over 262 144 rows: the variance came out 10 % off).  The
// difference of two floats is exact in fp64, so the shift costs nothing.
__global__ __launch_bounds__(CL_THREADS) void col_moments_stage1(const float* __restrict__ x, double* __restrict__ partial, long long rows,
                                                                 int cols, long long rows_per_block) {
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const long long r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
  for (int c = threadIdx.x; c < cols; c += CL_THREADS) {
    const double shift = (double)x[c];
    double s = 0.0, s2 = 0.0;
    for (long long r = r0; r < r1; ++r) {
      const double v = (double)x[r * cols + c] - shift;
      s += v;
      s2 += v * v;
    }
    partial[((long long)blockIdx.x * 2 + 0) * cols + c] = s;
    partial[((long long)blockIdx.x * 2 + 1) * cols + c] = s2;
  }
}

__global__ __launch_bounds__(CL_THREADS) void col_moments_stage2(const float* __restrict__ x, const double* __restrict__ partial,
                                                                 double* __restrict__ mean, double* __restrict__ var, long long rows, int cols,
                                                                 int blocks) {
  const int c = blockIdx.x * CL_THREADS + threadIdx.x;
  if (c >= cols) return;
  double s = 0.0, s2 = 0.0;
  for (int b = 0; b < blocks; ++b) {  // fixed order
    s += partial[((long long)b * 2 + 0) * cols + c];
    s2 += partial[((long long)b * 2 + 1) * cols + c];
  }
  const double m = s / (double)rows;   // the mean of the shifted values
  mean[c] = (double)x[c] + m;
  const double v = s2 / (double)rows - m * m;   // population variance, as StandardScaler (ddof = 0)
  var[c] = v > 0.0 ? v : 0.0;
}

// ---- bilinear upsampling of token-major maps (align_corners = False), fp64 arithmetic, fp32 in / out
__global__ __launch_bounds__(CL_THREADS) void upsample_tokens_kernel(const float* __restrict__ x, float* __restrict__ out, int g, int C,
                                                                     int R) {
  const int pix = blockIdx.x, m = blockIdx.y;
  const int oy = pix / R, ox = pix - oy * R;
  const double scale = (double)g / (double)R;
  double sy = scale * (oy + 0.5) - 0.5, sx = scale * (ox + 0.5) - 0.5;
  sy = sy < 0.0 ? 0.0 : sy;
  sx = sx < 0.0 ? 0.0 : sx;
  const int y0 = (int)sy, x0 = (int)sx;
  const int y1 = y0 + (y0 < g - 1 ? 1 : 0), x1 = x0 + (x0 < g - 1 ? 1 : 0);
  const double ly = sy - y0, lx = sx - x0, hy = 1.0 - ly, hx = 1.0 - lx;
  const float* base = x + (size_t)m * g * g * C;
  const float* p00 = base + (size_t)(y0 * g + x0) * C;
  const float* p01 = base + (size_t)(y0 * g + x1) * C;
  const float* p10 = base + (size_t)(y1 * g + x0) * C;
  const float* p11 = base + (size_t)(y1 * g + x1) * C;
  float* o = out + ((size_t)m * R * R + pix) * C;
  for (int c = threadIdx.x; c < C; c += blockDim.x)
    o[c] = (float)(hy * (hx * (double)p00[c] + lx * (double)p01[c]) + ly * (hx * (double)p10[c] + lx * (double)p11[c]));
}

// fp32 twin of upsample_argmax (label_prop.hip) for proto_clustering: scores [M, n, K] fp32 -> labels [M, R, R] int64,
// interpolation in fp32 like F.interpolate on a float tensor (clustering.py:101-103)
__global__ __launch_bounds__(CL_THREADS) void upsample_argmax_f32_kernel(const float* __restrict__ maps, int64_t* __restrict__ out, int g,
                                                                         int K, int R) {
  const int pix = blockIdx.x * CL_THREADS + threadIdx.x;
  if (pix >= R * R) return;
  const int m = blockIdx.y, oy = pix / R, ox = pix - oy * R;
  const float scale = (float)g / (float)R;
  float sy = scale * (oy + 0.5f) - 0.5f, sx = scale * (ox + 0.5f) - 0.5f;
  sy = sy < 0.f ? 0.f : sy;
  sx = sx < 0.f ? 0.f : sx;
  const int y0 = (int)sy, x0 = (int)sx;
  const int y1 = y0 + (y0 < g - 1 ? 1 : 0), x1 = x0 + (x0 < g - 1 ? 1 : 0);
  const float ly = sy - y0, lx = sx - x0, hy = 1.f - ly, hx = 1.f - lx;
  const float* base = maps + (size_t)m * g * g * K;
  const float* p00 = base + (size_t)(y0 * g + x0) * K;
  const float* p01 = base + (size_t)(y0 * g + x1) * K;
  const float* p10 = base + (size_t)(y1 * g + x0) * K;
  const float* p11 = base + (size_t)(y1 * g + x1) * K;
  float best = -INFINITY;
  int besti = 0;
  for (int k = 0; k < K; ++k) {
    const float v = hy * (hx * p00[k] + lx * p01[k]) + ly * (hx * p10[k] + lx * p11[k]);
    if (v > best) {
      best = v;
      besti = k;
    }
  }
  out[(size_t)m * R * R + pix] = besti;
}

// ---- N17: the histogram of upsample_argmax_f32_kernel's labels without the labels (time_tuning.get_similarity_histogram,
// time_tuning.py:354-375: the reference builds every [224, 224] map on the host and calls torch.histc on it).  counts[k] += the number of
// output pixels whose bilinear arg-max is k.  The per-pixel statement REPEATS the kernel above - the same fp32 expressions in the same
// form, first maximum first, compiled in this translation unit under the same flags - so a pixel gets the label that kernel gives it;
// that kernel itself is untouched.  Counting follows confusion.hip: a u32 histogram of K bins per workgroup in LDS, a grid-stride walk
// over the M * R * R pixels, equal consecutive labels merged into one LDS add per run (arg-max maps are piecewise constant, and equal
// keys serialise on one LDS address), and one 64-bit global integer atomic per non-zero bin at the end.  Integer atomics only: the
// result depends neither on the order nor on the grid.
// Runs are merged ACROSS THE LANES of a wave, not along a strip of one thread: a lane takes one pixel, consecutive lanes consecutive
// pixels - the load pattern of the kernel above, four or five token rows per wave and instruction - and the first lane of every run
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
// faster the finer it is cut (measured, profiles/n17_overlay.txt: one round of CL_THREADS pixels per workgroup 0.43 ms, four rounds and
// four pixels per bin under a cap of 2048 workgroups 0.46 ms, the rounds dealt evenly over 1792 workgroups 0.48 ms - the workgroups
// do not take equally long, and a finer grid lets the dispatcher even that out).  So: one round each up to UH_MAX_GRID workgroups, more
// rounds beyond, and never more than UH_MAX_PER_WG pixels - then the grid grows instead.  A workgroup walks whole rounds: at most
// per + CL_THREADS < 2^32 pixels.
static unsigned uh_blocks(long long pixels, int K) {
  const long long rounds = (long long)TT_UH_MIN_ROUNDS * CL_THREADS, bins = (long long)TT_UH_BIN_FACTOR * K;
  long long per = rounds > bins ? rounds : bins;
  const long long spread = (pixels + UH_MAX_GRID - 1) / UH_MAX_GRID;
  if (per < spread) per = spread;
  if (per > UH_MAX_PER_WG) per = UH_MAX_PER_WG;
  const long long blocks = (pixels + per - 1) / per;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

__global__ __launch_bounds__(CL_THREADS) void upsample_argmax_hist_f32_kernel(const float* __restrict__ maps,
                                                                              unsigned long long* __restrict__ counts, int g, int K, int R,
                                                                              long long pixels) {
  extern __shared__ unsigned int uh_hist[];
  for (int i = threadIdx.x; i < K; i += CL_THREADS) uh_hist[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  // every thread of the workgroup makes the same number of rounds (the ballot below needs whole waves); a lane past the end holds -1
  for (long long round = (long long)blockIdx.x * CL_THREADS; round < pixels; round += (long long)gridDim.x * CL_THREADS) {
    const long long i = round + threadIdx.x;
    int label = -1;
    if (i < pixels) {
      const long long m = i / ((long long)R * R);
      const int pix = (int)(i - m * R * R);
      // ---- upsample_argmax_f32_kernel's statement
      const int oy = pix / R, ox = pix - oy * R;
      const float scale = (float)g / (float)R;
      float sy = scale * (oy + 0.5f) - 0.5f, sx = scale * (ox + 0.5f) - 0.5f;
      sy = sy < 0.f ? 0.f : sy;
      sx = sx < 0.f ? 0.f : sx;
      const int y0 = (int)sy, x0 = (int)sx;
      const int y1 = y0 + (y0 < g - 1 ? 1 : 0), x1 = x0 + (x0 < g - 1 ? 1 : 0);
      const float ly = sy - y0, lx = sx - x0, hy = 1.f - ly, hx = 1.f - lx;
      const float* base = maps + (size_t)m * g * g * K;
      const float* p00 = base + (size_t)(y0 * g + x0) * K;
      const float* p01 = base + (size_t)(y0 * g + x1) * K;
      const float* p10 = base + (size_t)(y1 * g + x0) * K;
      const float* p11 = base + (size_t)(y1 * g + x1) * K;
      float best = -INFINITY;
      int besti = 0;
      for (int k = 0; k < K; ++k) {
        const float v = hy * (hx * p00[k] + lx * p01[k]) + ly * (hx * p10[k] + lx * p11[k]);
        if (v > best) {
          best = v;
          besti = k;
        }
      }
      // ----
      label = besti;
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
  for (int i = threadIdx.x; i < K; i += CL_THREADS) {
    const unsigned int c = uh_hist[i];
    if (c) atomicAdd(&counts[i], (unsigned long long)c);
  }
}

// x[r][c] = x[r][c] * scale[c] + shift[c]  (StandardScaler.transform, my_utils.py:29-30)
__global__ __launch_bounds__(CL_THREADS) void affine_cols_kernel(float* __restrict__ x, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, long long total, int cols) {
  const long long stride = (long long)gridDim.x * CL_THREADS;
  for (long long i = (long long)blockIdx.x * CL_THREADS + threadIdx.x; i < total; i += stride) {
    const int c = (int)(i % cols);
    x[i] = x[i] * scale[c] + shift[c];
  }
}

static int moments_blocks(long long rows) {
  long long b = (rows + 255) / 256;
  return (int)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}

}  // namespace tt

using namespace tt;

extern "C" size_t tt_col_moments_workspace_bytes(long long rows, int cols) {
  return (size_t)moments_blocks(rows) * 2 * cols * sizeof(double);
}

extern "C" int tt_col_moments(const float* x, double* mean, double* var, long long rows, int cols, void* workspace, size_t workspace_bytes,
                              tt_stream_t stream) {
  TT_REQUIRE(x && mean && var && workspace && rows > 0 && cols > 0 && cols <= CL_MAXD, "col_moments: need 0 < cols <= %d", CL_MAXD);
  TT_REQUIRE(workspace_bytes >= tt_col_moments_workspace_bytes(rows, cols), "col_moments: workspace too small");
  hipStream_t s = as_stream(stream);
  const int blocks = moments_blocks(rows);
  const long long rpb = (rows + blocks - 1) / blocks;
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(col_moments_stage1, dim3(blocks), dim3(CL_THREADS), 0, s, x, partial, rows, cols, rpb);
  hipLaunchKernelGGL(col_moments_stage2, dim3((cols + CL_THREADS - 1) / CL_THREADS), dim3(CL_THREADS), 0, s, x, partial, mean, var, rows,
                     cols, blocks);
  TT_CHECK_LAUNCH("col_moments");
  return TT_OK;
}

extern "C" int tt_upsample_bilinear_tokens(const float* x, float* out, int M, int g, int C, int R, tt_stream_t stream) {
  TT_REQUIRE(x && out && M > 0 && g > 0 && C > 0 && R > 0, "upsample_bilinear_tokens: bad arguments");
  TT_REQUIRE(M <= UP_MAXM && R <= 32768, "upsample_bilinear_tokens: %d maps of %dx%d exceed one launch (at most %d maps)", M, R, R, UP_MAXM);
  const int threads = C >= 256 ? 256 : (C > 64 ? 128 : 64);
  hipLaunchKernelGGL(upsample_tokens_kernel, dim3(R * R, M), dim3(threads), 0, as_stream(stream), x, out, g, C, R);
  TT_CHECK_LAUNCH("upsample_bilinear_tokens");
  return TT_OK;
}

extern "C" int tt_upsample_argmax_f32(const float* maps, int64_t* labels_out, int M, int g, int K, int R, tt_stream_t stream) {
  TT_REQUIRE(maps && labels_out && M > 0 && g > 0 && K > 0 && R > 0, "upsample_argmax_f32: bad arguments");
  TT_REQUIRE(M <= UP_MAXM && R <= 32768, "upsample_argmax_f32: %d maps of %dx%d exceed one launch (at most %d maps)", M, R, R, UP_MAXM);
  hipLaunchKernelGGL(upsample_argmax_f32_kernel, dim3((R * R + CL_THREADS - 1) / CL_THREADS, M), dim3(CL_THREADS), 0, as_stream(stream), maps,
                     labels_out, g, K, R);
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
  hipLaunchKernelGGL(upsample_argmax_hist_f32_kernel, dim3(uh_blocks(pixels, K)), dim3(CL_THREADS), sizeof(unsigned int) * (size_t)K,
                     as_stream(stream), maps, counts, g, K, R, pixels);
  TT_CHECK_LAUNCH("upsample_argmax_hist_f32");
  return TT_OK;
}

extern "C" int tt_affine_cols_inplace(float* x, const float* scale, const float* shift, long long rows, int cols, tt_stream_t stream) {
  TT_REQUIRE(x && scale && shift && rows > 0 && cols > 0, "affine_cols: bad arguments");
  const long long total = rows * cols;
  long long blocks = (total + CL_THREADS * 8 - 1) / (CL_THREADS * 8);
  blocks = blocks > 8192 ? 8192 : (blocks < 1 ? 1 : blocks);
  hipLaunchKernelGGL(affine_cols_kernel, dim3((unsigned)blocks), dim3(CL_THREADS), 0, as_stream(stream), x, scale, shift, total, cols);
  TT_CHECK_LAUNCH("affine_cols");
  return TT_OK;
}
