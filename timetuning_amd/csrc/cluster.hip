// Evaluator clustering: the GPU side of clustering.cluster_features / proto_clustering
// (clustering.py:20-117) and my_utils.normalize_and_transform (my_utils.py:19-37) around the k-means, which has its own file (kmeans.hip).
//
// The reference moves every feature map to the host, upsamples it in fp64 with ATen, and runs faiss' CPU Lloyd iterations
// while the other ranks wait at a barrier (time_tuning.py:634-648).  Here the dense passes stay on the device (with kmeans.hip's and
// the bilinear up-samplings of upsample.hip):
//   column moments (StandardScaler)         one two-stage fp64 reduction over the rows
//   affine_cols (StandardScaler.transform)  x * scale + shift per column, in place
// The tiny dense algebra between them (50 x 384 PCA basis from a 384 x 384 eigen-problem, k x d centroid bookkeeping, the
// Hungarian matching of a k x k score matrix) stays on the host.
#include "common.hpp"

namespace tt {

constexpr int CL_THREADS = 256;
constexpr int CL_MAXD = 1024;     // feature columns for the moments

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

extern "C" int tt_affine_cols_inplace(float* x, const float* scale, const float* shift, long long rows, int cols, tt_stream_t stream) {
  TT_REQUIRE(x && scale && shift && rows > 0 && cols > 0, "affine_cols: bad arguments");
  const long long total = rows * cols;
  long long blocks = (total + CL_THREADS * 8 - 1) / (CL_THREADS * 8);
  blocks = blocks > 8192 ? 8192 : (blocks < 1 ? 1 : blocks);
  hipLaunchKernelGGL(affine_cols_kernel, dim3((unsigned)blocks), dim3(CL_THREADS), 0, as_stream(stream), x, scale, shift, total, cols);
  TT_CHECK_LAUNCH("affine_cols");
  return TT_OK;
}
