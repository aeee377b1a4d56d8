// Batch normalisation over token-major tensors (N33): nn.BatchNorm2d of the FCN head's ConvModules (timetuning_amd/leopart.py norm_cfg) on
// [rows = B gh gw, C] fp32, channel-contiguous - the layout conv_tokens.hip reads and writes - forward (training and eval) and backward, fused
// with the ReLU and the Dropout2d multiplier that follow it.  include/timetuning_hip.h "N33" has the formulas and the contract.
//
// Both directions are two streaming launches over one decomposition: the rows are cut into `nslice` slices, the channels into groups of
// 64, and workgroup (slice, group) owns that tile in both launches.  Its 256 threads are 16 row lanes x 16 channel quads: a thread reads
// and writes 16 bytes, a row of the tile is 256 contiguous bytes.
//   launch 1  per tile, per column: two fp64 sums over the tile's rows (forward: sum v and sum v^2 of v = z - z[0][c]; backward: sum g and
//             sum g xhat).  A thread adds its rows in ascending order, the 16 row lanes are added in lane order through LDS, and the result is
//             partial[slice][2][C] in the caller's workspace.
//   launch 2  the workgroup folds the partials of ITS 64 columns over all slices (in slice order, as two halves on two threads whose
//             results are added: one fixed order, so two calls give the same bits), derives the per-column constants in LDS and streams
//             its tile.  The workgroups of slice 0 also write the per-column outputs (save_mean / save_rstd and the running statistics;
//             dgamma / dbeta).  No atomics, no counters, nothing handed between workgroups inside a launch.
// Every workgroup of launch 2 reads nslice KB of partials out of L2 beside the 64 KB or more it streams; bn_slices() keeps nslice <= 192.
#include "common.hpp"

namespace tt {

constexpr int BN_MAXC = 1024;
constexpr int BN_COLS = 64;            // channels of a workgroup: 16 quads
constexpr int BN_QUADS = BN_COLS / 4;
constexpr int BN_LANES = 256 / BN_QUADS;   // 16 row lanes
constexpr int BN_UNROLL = 4;           // rows a thread has in flight

struct BnSplit {
  int nslice;
  long long chunk;   // rows of a slice (the last may be shorter; every slice has at least one row)
};
// Slices of the rows: none shorter than 64 rows, and about 768 workgroups (three per CU) over all channel groups; between 32 and 192.
static BnSplit bn_slices(long long rows, int C) {
  const int groups = (C + BN_COLS - 1) / BN_COLS;
  long long cap = 768 / groups;
  if (cap < 32) cap = 32;
  if (cap > 192) cap = 192;
  long long ns = (rows + 63) / 64;
  if (ns > cap) ns = cap;
  if (ns < 1) ns = 1;
  const long long chunk = (rows + ns - 1) / ns;
  return BnSplit{(int)((rows + chunk - 1) / chunk), chunk};
}

__device__ __forceinline__ float4 bn_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// The thread's place in its tile: quad < 0 means "no columns" (the last group of a C that is no multiple of 64).
struct BnPlace {
  int lane, c;           // row lane, first of the 4 global columns (or -1)
  long long r0, r1;      // the slice's rows
};
__device__ __forceinline__ BnPlace bn_place(long long rows, long long chunk, int C) {
  BnPlace p;
  p.lane = threadIdx.x / BN_QUADS;
  const int c = blockIdx.y * BN_COLS + (threadIdx.x % BN_QUADS) * 4;
  p.c = c < C ? c : -1;
  p.r0 = (long long)blockIdx.x * chunk;
  p.r1 = p.r0 + chunk < rows ? p.r0 + chunk : rows;
  return p;
}

// The 16 row lanes' sums of the tile's 64 columns x 2 statistics, added in lane order; thread t < 128 owns (stat = t / 64, column = t % 64).
__device__ __forceinline__ void bn_store_partial(const double (&a)[4], const double (&b)[4], double* __restrict__ partial, int C) {
  __shared__ double red[BN_LANES][2 * BN_COLS];
  const int lane = threadIdx.x / BN_QUADS, q = (threadIdx.x % BN_QUADS) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    red[lane][q + i] = a[i];
    red[lane][BN_COLS + q + i] = b[i];
  }
  __syncthreads();
  if (threadIdx.x < 2 * BN_COLS) {
    const int stat = threadIdx.x / BN_COLS, col = blockIdx.y * BN_COLS + threadIdx.x % BN_COLS;
    if (col < C) {
      double s = 0.0;
#pragma unroll
      for (int l = 0; l < BN_LANES; ++l) s += red[l][threadIdx.x];
      partial[((size_t)blockIdx.x * 2 + stat) * C + col] = s;
    }
  }
}

// fold[stat][col] of the workgroup's 64 columns over all slices: thread t takes (stat, col) = t % 128 and half t / 128 of the slices.
// Returns after a barrier; valid for col < C only.
__device__ __forceinline__ void bn_fold(const double* __restrict__ partial, int nslice, int C, double (*fold)[2 * BN_COLS]) {
  const int pair = threadIdx.x % (2 * BN_COLS), half = threadIdx.x / (2 * BN_COLS);
  const int stat = pair / BN_COLS, col = blockIdx.y * BN_COLS + pair % BN_COLS;
  const int hn = (nslice + 1) / 2, s0 = half * hn, s1 = s0 + hn < nslice ? s0 + hn : nslice;
  double s = 0.0;
  if (col < C) {
#pragma unroll 8
    for (int k = s0; k < s1; ++k) s += partial[((size_t)k * 2 + stat) * C + col];
  }
  fold[half][pair] = s;
  __syncthreads();
}

// ---- forward, launch 1: sums of v and v^2, v = z - z[0][c]
__global__ __launch_bounds__(256) void bn_fwd_partial_kernel(const float* __restrict__ z, double* __restrict__ partial, long long rows,
                                                             long long chunk, int C) {
  const BnPlace p = bn_place(rows, chunk, C);
  double s[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
  if (p.c >= 0) {
    const float4 sh = bn_ld4(z + p.c);
    const double shift[4] = {(double)sh.x, (double)sh.y, (double)sh.z, (double)sh.w};
    for (long long r = p.r0 + p.lane; r < p.r1; r += BN_LANES * BN_UNROLL) {
      float4 v[BN_UNROLL];
#pragma unroll
      for (int u = 0; u < BN_UNROLL; ++u) {
        const long long ru = r + u * BN_LANES;
        v[u] = ru < p.r1 ? bn_ld4(z + ru * C + p.c) : sh;   // the shift itself adds zero
      }
#pragma unroll
      for (int u = 0; u < BN_UNROLL; ++u) {
        const double d[4] = {(double)v[u].x - shift[0], (double)v[u].y - shift[1], (double)v[u].z - shift[2], (double)v[u].w - shift[3]};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          s[i] += d[i];
          s2[i] += d[i] * d[i];
        }
      }
    }
  }
  bn_store_partial(s, s2, partial, C);
}

struct BnFwdArgs {
  const float* z;
  const float* gamma;
  const float* beta;
  const float* out_scale;
  float* running_mean;
  float* running_var;
  float* y;
  float* save_mean;
  float* save_rstd;
  const double* partial;
  long long rows, chunk;
  int npix, C, nslice, training, act;
  double momentum, eps;
};

// ---- forward, launch 2 (the only one in eval mode): statistics of the workgroup's columns, then y
__global__ __launch_bounds__(256) void bn_fwd_apply_kernel(BnFwdArgs a) {
  __shared__ double fold[2][2 * BN_COLS];
  __shared__ float col_mean[BN_COLS], col_scale[BN_COLS], col_beta[BN_COLS];
  const int C = a.C;
  if (a.training) bn_fold(a.partial, a.nslice, C, fold);
  if (threadIdx.x < BN_COLS) {
    const int col = blockIdx.y * BN_COLS + threadIdx.x;
    if (col < C) {
      double mean, var;
      if (a.training) {
        const double n = (double)a.rows;
        const double m = (fold[0][threadIdx.x] + fold[1][threadIdx.x]) / n;   // the mean of the shifted values
        mean = (double)a.z[col] + m;
        var = (fold[0][BN_COLS + threadIdx.x] + fold[1][BN_COLS + threadIdx.x]) / n - m * m;
        var = var > 0.0 ? var : 0.0;
      } else {
        mean = (double)a.running_mean[col];
        var = (double)a.running_var[col];
      }
      const double rstd = 1.0 / sqrt(var + a.eps);
      const float mean_f = (float)mean, rstd_f = (float)rstd;
      col_mean[threadIdx.x] = mean_f;
      col_scale[threadIdx.x] = rstd_f * a.gamma[col];
      col_beta[threadIdx.x] = a.beta[col];
      if (a.training && blockIdx.x == 0) {
        a.save_mean[col] = mean_f;
        a.save_rstd[col] = rstd_f;
        if (a.running_mean) {
          const double n = (double)a.rows;
          a.running_mean[col] = (float)((1.0 - a.momentum) * (double)a.running_mean[col] + a.momentum * mean);
          a.running_var[col] = (float)((1.0 - a.momentum) * (double)a.running_var[col] + a.momentum * (var * (n / (n - 1.0))));
        }
      }
    }
  }
  __syncthreads();
  const BnPlace p = bn_place(a.rows, a.chunk, C);
  if (p.c < 0) return;
  const int q = (threadIdx.x % BN_QUADS) * 4;
  const float mean[4] = {col_mean[q], col_mean[q + 1], col_mean[q + 2], col_mean[q + 3]};
  const float scale[4] = {col_scale[q], col_scale[q + 1], col_scale[q + 2], col_scale[q + 3]};
  const float beta[4] = {col_beta[q], col_beta[q + 1], col_beta[q + 2], col_beta[q + 3]};
  const bool relu = a.act != 0;
  for (long long r = p.r0 + p.lane; r < p.r1; r += BN_LANES * BN_UNROLL) {
    float4 v[BN_UNROLL];
#pragma unroll
    for (int u = 0; u < BN_UNROLL; ++u) {
      const long long ru = r + u * BN_LANES;
      if (ru < p.r1) v[u] = bn_ld4(a.z + ru * C + p.c);
    }
#pragma unroll
    for (int u = 0; u < BN_UNROLL; ++u) {
      const long long ru = r + u * BN_LANES;
      if (ru >= p.r1) break;
      float o[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o[i] = fmaf(o[i] - mean[i], scale[i], beta[i]);
        if (relu) o[i] = o[i] > 0.f ? o[i] : 0.f;
      }
      if (a.out_scale) {
        const float4 s = bn_ld4(a.out_scale + (size_t)((unsigned)ru / (unsigned)a.npix) * C + p.c);   // rows < 2^31
        o[0] *= s.x; o[1] *= s.y; o[2] *= s.z; o[3] *= s.w;
      }
      *reinterpret_cast<float4*>(a.y + ru * C + p.c) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

// ---- backward, launch 1: sums of g and g xhat
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const float* __restrict__ g, const float* __restrict__ z,
                                                             const float* __restrict__ save_mean, const float* __restrict__ save_rstd,
                                                             double* __restrict__ partial, long long rows, long long chunk, int C) {
  const BnPlace p = bn_place(rows, chunk, C);
  double sb[4] = {0.0, 0.0, 0.0, 0.0}, sg[4] = {0.0, 0.0, 0.0, 0.0};
  if (p.c >= 0) {
    float mean[4], rstd[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      mean[i] = save_mean[p.c + i];
      rstd[i] = save_rstd[p.c + i];
    }
    for (long long r = p.r0 + p.lane; r < p.r1; r += BN_LANES * BN_UNROLL) {
      float4 vg[BN_UNROLL], vz[BN_UNROLL];
#pragma unroll
      for (int u = 0; u < BN_UNROLL; ++u) {
        const long long ru = r + u * BN_LANES;
        if (ru < p.r1) {
          vg[u] = bn_ld4(g + ru * C + p.c);
          vz[u] = bn_ld4(z + ru * C + p.c);
        } else {
          vg[u] = make_float4(0.f, 0.f, 0.f, 0.f);   // adds zero to both sums
          vz[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
#pragma unroll
      for (int u = 0; u < BN_UNROLL; ++u) {
        const float gg[4] = {vg[u].x, vg[u].y, vg[u].z, vg[u].w}, zz[4] = {vz[u].x, vz[u].y, vz[u].z, vz[u].w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float xhat = (zz[i] - mean[i]) * rstd[i];
          sb[i] += (double)gg[i];
          sg[i] += (double)gg[i] * (double)xhat;
        }
      }
    }
  }
  bn_store_partial(sb, sg, partial, C);
}

// ---- backward, launch 2: dbeta, dgamma of the workgroup's columns, then dz
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ g, const float* __restrict__ z,
                                                           const float* __restrict__ save_mean, const float* __restrict__ save_rstd,
                                                           const float* __restrict__ gamma, const double* __restrict__ partial,
                                                           float* __restrict__ dz, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           long long rows, long long chunk, int C, int nslice) {
  __shared__ double fold[2][2 * BN_COLS];
  __shared__ float col_mean[BN_COLS], col_rstd[BN_COLS], col_a[BN_COLS], col_mb[BN_COLS], col_mg[BN_COLS];
  bn_fold(partial, nslice, C, fold);
  if (threadIdx.x < BN_COLS) {
    const int col = blockIdx.y * BN_COLS + threadIdx.x;
    if (col < C) {
      const double db = fold[0][threadIdx.x] + fold[1][threadIdx.x];
      const double dg = fold[0][BN_COLS + threadIdx.x] + fold[1][BN_COLS + threadIdx.x];
      const float rstd = save_rstd[col];
      col_mean[threadIdx.x] = save_mean[col];
      col_rstd[threadIdx.x] = rstd;
      col_a[threadIdx.x] = gamma[col] * rstd;
      col_mb[threadIdx.x] = (float)(db / (double)rows);
      col_mg[threadIdx.x] = (float)(dg / (double)rows);
      if (blockIdx.x == 0) {
        dbeta[col] = (float)db;
        dgamma[col] = (float)dg;
      }
    }
  }
  __syncthreads();
  const BnPlace p = bn_place(rows, chunk, C);
  if (p.c < 0) return;
  const int q = (threadIdx.x % BN_QUADS) * 4;
  float mean[4], rstd[4], ca[4], mb[4], mg[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    mean[i] = col_mean[q + i];
    rstd[i] = col_rstd[q + i];
    ca[i] = col_a[q + i];
    mb[i] = col_mb[q + i];
    mg[i] = col_mg[q + i];
  }
  for (long long r = p.r0 + p.lane; r < p.r1; r += BN_LANES * BN_UNROLL) {
    float4 vg[BN_UNROLL], vz[BN_UNROLL];
#pragma unroll
    for (int u = 0; u < BN_UNROLL; ++u) {
      const long long ru = r + u * BN_LANES;
      if (ru < p.r1) {
        vg[u] = bn_ld4(g + ru * C + p.c);
        vz[u] = bn_ld4(z + ru * C + p.c);
      }
    }
#pragma unroll
    for (int u = 0; u < BN_UNROLL; ++u) {
      const long long ru = r + u * BN_LANES;
      if (ru >= p.r1) break;
      const float gg[4] = {vg[u].x, vg[u].y, vg[u].z, vg[u].w}, zz[4] = {vz[u].x, vz[u].y, vz[u].z, vz[u].w};
      float o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float xhat = (zz[i] - mean[i]) * rstd[i];
        o[i] = ca[i] * ((gg[i] - mb[i]) - xhat * mg[i]);
      }
      *reinterpret_cast<float4*>(dz + ru * C + p.c) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

// ---- host side
static int bn_shape_error(const char* who, long long rows, int C, int training) {
  TT_REQUIRE(C > 0 && C % 4 == 0 && C <= BN_MAXC, "%s: need C %% 4 == 0 and 0 < C <= %d (got %d)", who, BN_MAXC, C);
  TT_REQUIRE(rows > 0 && rows < (1LL << 31), "%s: need 0 < rows < 2^31 (got %lld)", who, rows);
  TT_REQUIRE(!training || rows >= 2, "%s: batch statistics need at least 2 rows (got %lld)", who, rows);
  return TT_OK;
}

static size_t bn_workspace_bytes(long long rows, int C) {
  if (rows <= 0 || rows >= (1LL << 31) || C <= 0 || C > BN_MAXC) return 0;
  return (size_t)bn_slices(rows, C).nslice * 2 * C * sizeof(double);
}

}  // namespace tt

using namespace tt;

extern "C" int tt_bn_tokens_shape_ok(long long rows, int C, int training) {
  return C > 0 && C % 4 == 0 && C <= BN_MAXC && rows > 0 && rows < (1LL << 31) && (!training || rows >= 2);
}

extern "C" size_t tt_bn_tokens_fwd_workspace_bytes(long long rows, int C) { return bn_workspace_bytes(rows, C); }
extern "C" size_t tt_bn_tokens_bwd_workspace_bytes(long long rows, int C) { return bn_workspace_bytes(rows, C); }

extern "C" int tt_bn_tokens_fwd(const float* z, const float* gamma, const float* beta, const float* out_scale, float* running_mean,
                                float* running_var, float* y, float* save_mean, float* save_rstd, long long rows, long long rows_per_image,
                                int C, int training, int act, double momentum, double eps, void* workspace, size_t workspace_bytes,
                                tt_stream_t stream) {
  const char* who = "bn_tokens_fwd";
  TT_REQUIRE(training == 0 || training == 1, "%s: training must be 0 or 1 (got %d)", who, training);
  TT_REQUIRE(z && gamma && beta && y, "%s: null pointer", who);
  if (int rc = bn_shape_error(who, rows, C, training)) return rc;
  TT_REQUIRE(act == 0 || act == 1, "%s: act must be 0 or 1 (ReLU) (got %d)", who, act);
  TT_REQUIRE(eps > 0.0, "%s: need eps > 0 (got %g)", who, eps);   // also refuses a NaN
  TT_REQUIRE(momentum >= 0.0 && momentum <= 1.0, "%s: need 0 <= momentum <= 1 (got %g)", who, momentum);
  if (training) {
    TT_REQUIRE(save_mean && save_rstd, "%s: training needs save_mean and save_rstd", who);
    TT_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "%s: running_mean and running_var go together", who);
    TT_REQUIRE(workspace, "%s: training needs a workspace", who);
    TT_REQUIRE(workspace_bytes >= bn_workspace_bytes(rows, C), "%s: workspace too small", who);
  } else {
    TT_REQUIRE(running_mean && running_var, "%s: eval mode needs running_mean and running_var", who);
  }
  if (out_scale)
    TT_REQUIRE(rows_per_image >= 1 && rows % rows_per_image == 0, "%s: out_scale needs rows (%lld) to be whole images of %lld rows", who, rows,
               rows_per_image);
  TT_REQUIRE(aligned16(z) && aligned16(y) && aligned16(out_scale) && (!training || aligned16(workspace)),
             "%s: z, y, out_scale and the workspace must be 16-byte aligned", who);
  const BnSplit sp = bn_slices(rows, C);
  const dim3 grid((unsigned)sp.nslice, (unsigned)((C + BN_COLS - 1) / BN_COLS));
  hipStream_t s = as_stream(stream);
  double* partial = static_cast<double*>(workspace);
  if (training) {
    hipLaunchKernelGGL(bn_fwd_partial_kernel, grid, dim3(256), 0, s, z, partial, rows, sp.chunk, C);
    TT_CHECK_LAUNCH("bn_tokens_fwd.partial");
  }
  BnFwdArgs a{z, gamma, beta, out_scale, running_mean, running_var, y, save_mean, save_rstd, partial, rows, sp.chunk,
              (int)(out_scale ? rows_per_image : 1), C, sp.nslice, training, act, momentum, eps};
  hipLaunchKernelGGL(bn_fwd_apply_kernel, grid, dim3(256), 0, s, a);
  TT_CHECK_LAUNCH("bn_tokens_fwd");
  return TT_OK;
}

extern "C" int tt_bn_tokens_bwd(const float* g, const float* z, const float* save_mean, const float* save_rstd, const float* gamma, float* dz,
                                float* dgamma, float* dbeta, long long rows, int C, void* workspace, size_t workspace_bytes,
                                tt_stream_t stream) {
  const char* who = "bn_tokens_bwd";
  TT_REQUIRE(g && z && save_mean && save_rstd && gamma && dz && dgamma && dbeta && workspace, "%s: null pointer", who);
  if (int rc = bn_shape_error(who, rows, C, 1)) return rc;
  TT_REQUIRE(aligned16(g) && aligned16(z) && aligned16(dz) && aligned16(workspace), "%s: g, z, dz and the workspace must be 16-byte aligned", who);
  TT_REQUIRE(workspace_bytes >= bn_workspace_bytes(rows, C), "%s: workspace too small", who);
  const BnSplit sp = bn_slices(rows, C);
  const dim3 grid((unsigned)sp.nslice, (unsigned)((C + BN_COLS - 1) / BN_COLS));
  hipStream_t s = as_stream(stream);
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(bn_bwd_partial_kernel, grid, dim3(256), 0, s, g, z, save_mean, save_rstd, partial, rows, sp.chunk, C);
  TT_CHECK_LAUNCH("bn_tokens_bwd.partial");
  hipLaunchKernelGGL(bn_bwd_apply_kernel, grid, dim3(256), 0, s, g, z, save_mean, save_rstd, gamma, partial, dz, dgamma, dbeta, rows, sp.chunk, C,
                     sp.nslice);
  TT_CHECK_LAUNCH("bn_tokens_bwd");
  return TT_OK;
}
