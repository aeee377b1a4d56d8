// Linear-probe fine-tuning: the device side of linear_finetune.py - a 1x1-conv head on frozen features, trained
// with CrossEntropyLoss(ignore_index=255) at mask resolution and torch.optim.SGD.
//
// The reference upsamples the features to the mask size and then applies the conv (linear_finetune.py:23-31).  Both operators are
// linear and the bilinear weights (align_corners = False) sum to 1 at every output pixel, clamped edges included, so
// conv(upsample(f)) = upsample(conv(f)), bias included.  Everything here therefore runs at token resolution with C class channels:
//   tt_probe_logits              logits = feats W^T + b, one pass over feats, fp32 FMA
//   tt_probe_upsample_ce         upsample -> softmax CE -> gradient -> adjoint of the upsample, fused: one workgroup per (image, low-res
//                                row i) recomputes the mask rows that feed row i and gathers their gradient into it (one writer per
//                                low-res row, fixed summation order: deterministic), then a second launch folds the per-workgroup
//                                loss / count partials in a fixed order and applies the 1/count of the mean
//   tt_bilinear_adjoint_tokens   the same gather on a given mask-resolution gradient (backward of tt_upsample_bilinear_tokens)
//   tt_probe_wgrad               dW = dlogits^T feats, db = colsum(dlogits): split rows, per-split partials, fixed-order fold
//   tt_sgd_step                  torch.optim.SGD (dampening 0, no Nesterov) over a table of tensors
#include <math.h>

#include "common.hpp"
#include "interp.hpp"

namespace tt {

constexpr int LP_THREADS = 256;
constexpr int LP_MAXD = 1024, LP_MAXC = 256, LP_MAXG = 64, LP_MAXR = 1024;

static int probe_shape_error(int D, int C) {
  TT_REQUIRE(D > 0 && D % 4 == 0 && D <= LP_MAXD, "linear probe: need D %% 4 == 0 and 0 < D <= %d (got %d)", LP_MAXD, D);
  TT_REQUIRE(C >= 1 && C <= LP_MAXC, "linear probe: need 1 <= classes <= %d (got %d)", LP_MAXC, C);
  return TT_OK;
}

static int probe_grid_error(int B, int g, int C, int R) {
  TT_REQUIRE(B >= 1 && B <= 65535, "linear probe: need 1 <= B <= 65535 (got %d)", B);
  TT_REQUIRE(g >= 1 && g <= LP_MAXG, "linear probe: need 1 <= g <= %d (got %d)", LP_MAXG, g);
  TT_REQUIRE(C >= 1 && C <= LP_MAXC, "linear probe: need 1 <= classes <= %d (got %d)", LP_MAXC, C);
  TT_REQUIRE(R >= 1 && R <= LP_MAXR, "linear probe: need 1 <= R <= %d (got %d)", LP_MAXR, R);
  return TT_OK;
}

// ---- logits[rows, C] = feats[rows, D] W[C, D]^T + b.  A workgroup owns 16 RPT rows and ALL classes (CT tiles of 64), so feats is read
// once; D is staged 32 columns at a time, both operands transposed into LDS.  Thread t: rows RPT (t / 16) .. + RPT - 1, classes
// t % 16 + 16 j.  Each 32-column stage is summed on its own and then added to the total (two-level sum: fp32 error grows with
// 32 + D / 32 terms instead of D).
constexpr int PL_DK = 32;

template <int CT, int RPT>
__global__ __launch_bounds__(LP_THREADS) void probe_logits_kernel(const float* __restrict__ feats, const float* __restrict__ w,
                                                                  const float* __restrict__ bias, float* __restrict__ out, long long rows, int D,
                                                                  int C) {
  constexpr int ROWS = 16 * RPT;
  __shared__ float xs[PL_DK][ROWS + 4];
  __shared__ float ws[PL_DK][CT * 64 + 4];
  const int t = threadIdx.x, rg = t >> 4, cl = t & 15;
  const long long r0 = (long long)blockIdx.x * ROWS;
  float acc[RPT][4 * CT];
#pragma unroll
  for (int i = 0; i < RPT; ++i)
#pragma unroll
    for (int j = 0; j < 4 * CT; ++j) acc[i][j] = 0.f;
  for (int k0 = 0; k0 < D; k0 += PL_DK) {
    for (int q = t; q < ROWS * PL_DK / 4; q += LP_THREADS) {
      const int r = q >> 3, c4 = (q & 7) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r0 + r < rows && k0 + c4 < D) v = *reinterpret_cast<const float4*>(feats + (r0 + r) * D + k0 + c4);
      xs[c4][r] = v.x;
      xs[c4 + 1][r] = v.y;
      xs[c4 + 2][r] = v.z;
      xs[c4 + 3][r] = v.w;
    }
    for (int q = t; q < CT * 64 * PL_DK / 4; q += LP_THREADS) {
      const int c = q >> 3, c4 = (q & 7) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < C && k0 + c4 < D) v = *reinterpret_cast<const float4*>(w + (long long)c * D + k0 + c4);
      ws[c4][c] = v.x;
      ws[c4 + 1][c] = v.y;
      ws[c4 + 2][c] = v.z;
      ws[c4 + 3][c] = v.w;
    }
    __syncthreads();
    float part[RPT][4 * CT];
#pragma unroll
    for (int i = 0; i < RPT; ++i)
#pragma unroll
      for (int j = 0; j < 4 * CT; ++j) part[i][j] = 0.f;
#pragma unroll 4
    for (int k = 0; k < PL_DK; ++k) {
      float xv[RPT];
#pragma unroll
      for (int i = 0; i < RPT; ++i) xv[i] = xs[k][rg * RPT + i];
#pragma unroll
      for (int j = 0; j < 4 * CT; ++j) {
        const float wv = ws[k][cl + 16 * j];
#pragma unroll
        for (int i = 0; i < RPT; ++i) part[i][j] = fmaf(xv[i], wv, part[i][j]);
      }
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i)
#pragma unroll
      for (int j = 0; j < 4 * CT; ++j) acc[i][j] += part[i][j];
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const long long r = r0 + rg * RPT + i;
    if (r >= rows) continue;
#pragma unroll
    for (int j = 0; j < 4 * CT; ++j) {
      const int c = cl + 16 * j;
      if (c < C) out[r * C + c] = acc[i][j] + (bias ? bias[c] : 0.f);
    }
  }
}

// ---- bilinear source index, align_corners = False: interp.hpp's lin_tap in fp64, the very function tt_upsample_bilinear_tokens takes
// its taps from (upsample.hip), whose adjoint this must be; the weight is then rounded to fp32
// (l1: the weight of the second tap, i0 gets 1 - l1)

// ---- the gather shared by tt_probe_upsample_ce (CE = true) and tt_bilinear_adjoint_tokens (CE = false).
// Workgroup (i, b) owns low-res row i of image b: it walks the mask rows oy whose source rows include i, produces the mask-resolution
// gradient dz of row oy (CE: softmax - one-hot of the recomputed upsampled logits; adjoint: read from d_hi), pre-multiplied by the row
// weight, P pixels at a time into LDS, and adds sum_ox wx(ox, j) dz(ox, c) into its accumulator acc[j][c].  Pixels are handled by TP
// lanes each (classes lane, lane + TP, ...; at most 8 per lane).  The CE loss and the label counts of row oy are taken by the workgroup
// of its FIRST source row (y0 == i), so every pixel is counted once.
constexpr int PG_MAXK = 8;                          // classes per lane
constexpr int PG_DZ = LP_THREADS * PG_MAXK;         // LDS floats of one pixel chunk: (256 / TP) pixels x C <= 256 * 8

__host__ __device__ inline int gather_tp_log2(int C) {
  int l = 0;
  while ((C + (1 << l) - 1) >> l > PG_MAXK) ++l;
  return l;
}

inline size_t gather_lds_bytes(int g, int C, int R) { return sizeof(float) * ((size_t)g * C + PG_DZ) + (size_t)R * (2 * sizeof(int) + sizeof(float)); }

template <bool CE>
__global__ __launch_bounds__(LP_THREADS) void probe_gather_kernel(const float* __restrict__ src, const int64_t* __restrict__ labels,
                                                                  float* __restrict__ dlow, double* __restrict__ part_loss,
                                                                  double* __restrict__ part_cnt, int g, int C, int R, int tp_log2) {
  extern __shared__ float sm[];
  float* acc = sm;                                        // [g][C]
  float* dz = acc + g * C;                                // [P][C]
  int* x0s = reinterpret_cast<int*>(dz + PG_DZ);          // [R] per output column: source columns and weight
  int* x1s = x0s + R;
  float* l1s = reinterpret_cast<float*>(x1s + R);
  __shared__ double red[3][LP_THREADS / 64];
  const int t = threadIdx.x, i = blockIdx.x, b = blockIdx.y;
  const double scale = (double)g / (double)R;
  for (int o = t; o < R; o += LP_THREADS) {
    const LinTap<double> s = lin_tap<double>(o, scale, g);
    x0s[o] = s.i0;
    x1s[o] = s.i1;
    l1s[o] = (float)s.l;
  }
  for (int e = t; e < g * C; e += LP_THREADS) acc[e] = 0.f;
  __syncthreads();
  const int TP = 1 << tp_log2, P = LP_THREADS >> tp_log2;
  const int slot = t >> tp_log2, lane = t & (TP - 1);
  const float* img = src + (size_t)b * (CE ? (size_t)g * g : (size_t)R * R) * C;
  double loss = 0.0, nvalid = 0.0, ninvalid = 0.0;
  for (int oy = 0; oy < R; ++oy) {
    const LinTap<double> sy = lin_tap<double>(oy, scale, g);
    if (sy.i0 != i && sy.i1 != i) continue;  // uniform over the workgroup
    const float ly = (float)sy.l;
    const float wy = (sy.i0 == i ? 1.f - ly : 0.f) + (sy.i1 == i ? ly : 0.f);
    const bool owner = sy.i0 == i;
    for (int xa = 0; xa < R; xa += P) {
      const int ox = xa + slot;
      if (ox < R) {
        float* dzp = dz + slot * C;
        if (CE) {
          const int x0 = x0s[ox], x1 = x1s[ox];
          const float lx = l1s[ox], hx = 1.f - lx, hy = 1.f - ly;
          const float* p00 = img + (size_t)(sy.i0 * g + x0) * C;
          const float* p01 = img + (size_t)(sy.i0 * g + x1) * C;
          const float* p10 = img + (size_t)(sy.i1 * g + x0) * C;
          const float* p11 = img + (size_t)(sy.i1 * g + x1) * C;
          const long long y = labels[((size_t)b * R + oy) * R + ox];
          const bool ignored = y == 255;
          const bool valid = !ignored && y >= 0 && y < C;
          float z[PG_MAXK];
          float m = -INFINITY;
#pragma unroll
          for (int k = 0; k < PG_MAXK; ++k) {
            const int c = lane + k * TP;
            z[k] = -INFINITY;
            if (c < C) {
              z[k] = hy * (hx * p00[c] + lx * p01[c]) + ly * (hx * p10[c] + lx * p11[c]);
              m = fmaxf(m, z[k]);
            }
          }
          for (int o = TP >> 1; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
          float s = 0.f;
#pragma unroll
          for (int k = 0; k < PG_MAXK; ++k) {
            z[k] = expf(z[k] - m);  // exp(-inf) = 0 for the padding classes
            s += z[k];
          }
          for (int o = TP >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
          const float inv = wy / s;
#pragma unroll
          for (int k = 0; k < PG_MAXK; ++k) {
            const int c = lane + k * TP;
            if (c < C) dzp[c] = valid ? z[k] * inv - (c == y ? wy : 0.f) : 0.f;
          }
          if (owner && lane == 0) {
            if (valid) {
              const int c = (int)y;
              const float zy = hy * (hx * p00[c] + lx * p01[c]) + ly * (hx * p10[c] + lx * p11[c]);
              loss += (double)(logf(s) + m - zy);
              nvalid += 1.0;
            } else if (!ignored) {
              ninvalid += 1.0;
            }
          }
        } else {
          const float* row = img + ((size_t)oy * R + ox) * C;
          for (int c = lane; c < C; c += TP) dzp[c] = wy * row[c];
        }
      }
      __syncthreads();
      const int xe = (xa + P < R ? xa + P : R) - 1;
      const int jlo = x0s[xa], jhi = x1s[xe];
      for (int e = jlo * C + t; e < (jhi + 1) * C; e += LP_THREADS) {
        const int j = e / C, c = e - j * C;
        float a = acc[e];
        for (int o = xa; o <= xe; ++o) {
          const int a0 = x0s[o], a1 = x1s[o];
          if (a0 > j) break;  // source columns are non-decreasing in o
          if (a1 < j) continue;
          const float lx = l1s[o];
          const float wx = (a0 == j ? 1.f - lx : 0.f) + (a1 == j ? lx : 0.f);
          a = fmaf(wx, dz[(o - xa) * C + c], a);
        }
        acc[e] = a;
      }
      __syncthreads();
    }
  }
  float* out = dlow + ((size_t)b * g + i) * g * C;
  for (int e = t; e < g * C; e += LP_THREADS) out[e] = acc[e];
  if (CE) {
    loss = wave_sum_d(loss);
    nvalid = wave_sum_d(nvalid);
    ninvalid = wave_sum_d(ninvalid);
    if ((t & 63) == 0) {
      red[0][t >> 6] = loss;
      red[1][t >> 6] = nvalid;
      red[2][t >> 6] = ninvalid;
    }
    __syncthreads();
    if (t == 0) {
      double l = 0.0, v = 0.0, n = 0.0;
      for (int w = 0; w < LP_THREADS / 64; ++w) {
        l += red[0][w];
        v += red[1][w];
        n += red[2][w];
      }
      const size_t p = (size_t)b * g + i;
      part_loss[p] = l;
      part_cnt[2 * p] = v;
      part_cnt[2 * p + 1] = n;
    }
  }
}

// Folds the per-workgroup partials (every workgroup the same fixed order, so all agree bit for bit), writes the mean loss and the
// counts (workgroup 0) and scales this workgroup's share of dlogits_low by 1 / count (0 when every pixel is ignored, as torch).
__global__ __launch_bounds__(LP_THREADS) void probe_ce_finalize_kernel(const double* __restrict__ part_loss, const double* __restrict__ part_cnt,
                                                                       int nparts, float* __restrict__ dlow, long long n,
                                                                       float* __restrict__ loss_out, long long* __restrict__ counts_out) {
  __shared__ double red[3][LP_THREADS / 64];
  __shared__ float sc;
  const int t = threadIdx.x;
  double l = 0.0, v = 0.0, inv = 0.0;
  for (int p = t; p < nparts; p += LP_THREADS) {
    l += part_loss[p];
    v += part_cnt[2 * p];
    inv += part_cnt[2 * p + 1];
  }
  l = wave_sum_d(l);
  v = wave_sum_d(v);
  inv = wave_sum_d(inv);
  if ((t & 63) == 0) {
    red[0][t >> 6] = l;
    red[1][t >> 6] = v;
    red[2][t >> 6] = inv;
  }
  __syncthreads();
  if (t == 0) {
    double L = 0.0, V = 0.0, I = 0.0;
    for (int w = 0; w < LP_THREADS / 64; ++w) {
      L += red[0][w];
      V += red[1][w];
      I += red[2][w];
    }
    sc = V > 0.0 ? (float)(1.0 / V) : 0.f;
    if (blockIdx.x == 0) {
      loss_out[0] = (float)(L / V);  // 0 / 0 = NaN with every pixel ignored, as torch
      counts_out[0] = (long long)V;
      counts_out[1] = (long long)I;
    }
  }
  __syncthreads();
  const float s = sc;
  for (long long e = (long long)blockIdx.x * LP_THREADS + t; e < n; e += (long long)gridDim.x * LP_THREADS) dlow[e] *= s;
}

// ---- weight gradient.  Stage 1: workgroup (d tile, c tile, split) accumulates a 64 x 64 tile of dlogits^T feats over the split's rows
// (thread t: classes 4 (t / 16) .., columns 4 (t % 16) ..), the workgroups of d tile 0 also the column sums of dlogits; the partials go to
// the workspace [split][C * D + C].  Stage 2 folds the splits in order and applies the optional device-scalar multiplier.
constexpr int PW_R = 32;

struct WgradSplit {
  int nsplit;
  long long rows_per_split;
};
// floats per split in the workspace: C * D + C rounded up to 4, so that every split starts 16-byte aligned
__host__ __device__ inline long long wgrad_split_stride(int D, int C) { return ((long long)C * D + C + 3) / 4 * 4; }
static WgradSplit wgrad_split(long long rows, int D, int C) {
  const long long tiles = (long long)((D + 63) / 64) * ((C + 63) / 64);
  const long long chunks = (rows + PW_R - 1) / PW_R;
  long long ns = (1024 + tiles - 1) / tiles;
  if (ns > chunks) ns = chunks;
  if (ns < 1) ns = 1;
  const long long rps = ((rows + ns - 1) / ns + PW_R - 1) / PW_R * PW_R;
  return WgradSplit{(int)((rows + rps - 1) / rps), rps};
}

__global__ __launch_bounds__(LP_THREADS) void probe_wgrad_partial_kernel(const float* __restrict__ dl, const float* __restrict__ x,
                                                                         float* __restrict__ part, long long rows, int D, int C,
                                                                         long long rps) {
  __shared__ float as[PW_R][64 + 4];
  __shared__ float bs[PW_R][64 + 4];
  const int t = threadIdx.x, ci = t >> 4, di = t & 15;
  const int d0 = blockIdx.x * 64, c0 = blockIdx.y * 64, s = blockIdx.z;
  const long long ra = (long long)s * rps, rb = ra + rps < rows ? ra + rps : rows;
  const bool colsum = blockIdx.x == 0 && t < 64;
  float acc[4][4] = {};
  float cs = 0.f;
  for (long long r0 = ra; r0 < rb; r0 += PW_R) {
    for (int q = t; q < PW_R * 64; q += LP_THREADS) {
      const int r = q >> 6, c = q & 63;
      as[r][c] = (r0 + r < rb && c0 + c < C) ? dl[(r0 + r) * C + c0 + c] : 0.f;
    }
    for (int q = t; q < PW_R * 16; q += LP_THREADS) {
      const int r = q >> 4, d4 = (q & 15) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r0 + r < rb && d0 + d4 < D) v = *reinterpret_cast<const float4*>(x + (r0 + r) * D + d0 + d4);
      *reinterpret_cast<float4*>(&bs[r][d4]) = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < PW_R; ++r) {
      const float4 a = *reinterpret_cast<const float4*>(&as[r][ci * 4]);
      const float4 bv = *reinterpret_cast<const float4*>(&bs[r][di * 4]);
      const float av[4] = {a.x, a.y, a.z, a.w}, bw[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = fmaf(av[u], bw[v], acc[u][v]);
    }
    if (colsum)
      for (int r = 0; r < PW_R; ++r) cs += as[r][t];
    __syncthreads();
  }
  float* ps = part + (size_t)s * wgrad_split_stride(D, C);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = c0 + ci * 4 + u;
    if (c >= C) continue;
    const int d = d0 + di * 4;
    if (d < D) *reinterpret_cast<float4*>(ps + (size_t)c * D + d) = make_float4(acc[u][0], acc[u][1], acc[u][2], acc[u][3]);
  }
  if (colsum && c0 + t < C) ps[(size_t)C * D + c0 + t] = cs;
}

__global__ __launch_bounds__(LP_THREADS) void probe_wgrad_fold_kernel(const float* __restrict__ part, int nsplit, long long stride,
                                                                      long long CD, int C, const float* __restrict__ mult,
                                                                      float* __restrict__ dw, float* __restrict__ db) {
  const long long n = CD + C;
  const float m = mult ? *mult : 1.f;
  for (long long e = (long long)blockIdx.x * LP_THREADS + threadIdx.x; e < n; e += (long long)gridDim.x * LP_THREADS) {
    float s = 0.f;
    for (int k = 0; k < nsplit; ++k) s += part[(size_t)k * stride + e];
    if (e < CD)
      dw[e] = s * m;
    else if (db)
      db[e - CD] = s * m;
  }
}

// ---- SGD (torch.optim.SGD, dampening 0, no Nesterov, maximize False): d = g + wd p; buf = d (first step) or momentum buf + d; p -= lr buf.
struct SgdTable {
  tt_adamw_tensor t[TT_MAX_TENSORS];
};
__global__ __launch_bounds__(LP_THREADS) void sgd_kernel(SgdTable tab, float momentum, int first_step) {
  const tt_adamw_tensor t = tab.t[blockIdx.y];
  for (long long i = (long long)blockIdx.x * LP_THREADS + threadIdx.x; i < t.n; i += (long long)gridDim.x * LP_THREADS) {
    const float p = t.p[i];
    float d = t.weight_decay != 0.f ? t.g[i] + t.weight_decay * p : t.g[i];
    if (t.m) {
      d = first_step ? d : t.m[i] * momentum + d;
      t.m[i] = d;
    }
    t.p[i] = p + (-t.lr) * d;
  }
}

static bool raise_gather_lds() {
  static const bool ok = [] {
    const int bytes = 96 * 1024;  // g * C <= 64 * 256 floats of accumulator + the pixel chunk + the column tables
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&probe_gather_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) ==
               hipSuccess &&
           hipFuncSetAttribute(reinterpret_cast<const void*>(&probe_gather_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) ==
               hipSuccess;
  }();
  return ok;
}

}  // namespace tt

using namespace tt;

extern "C" int tt_probe_logits(const float* feats, const float* weight, const float* bias, float* logits, long long rows, int D, int C,
                               tt_stream_t stream) {
  TT_REQUIRE(feats && weight && logits && rows > 0, "probe_logits: bad arguments");
  if (int rc = probe_shape_error(D, C)) return rc;
  TT_REQUIRE(aligned16(feats) && aligned16(weight), "probe_logits: feats and weight must be 16-byte aligned");
  hipStream_t s = as_stream(stream);
  const int ct = (C + 63) / 64;
  const int rows_per_block = ct == 1 ? 64 : 32;   // accumulators + stage sums per thread: 2 RPT 4 CT floats
  const long long blocks = (rows + rows_per_block - 1) / rows_per_block;
  TT_REQUIRE(blocks <= 0x7fffffffLL, "probe_logits: too many rows");
  const dim3 grid((unsigned)blocks), block(LP_THREADS);
  if (ct == 1)
    hipLaunchKernelGGL((probe_logits_kernel<1, 4>), grid, block, 0, s, feats, weight, bias, logits, rows, D, C);
  else if (ct == 2)
    hipLaunchKernelGGL((probe_logits_kernel<2, 2>), grid, block, 0, s, feats, weight, bias, logits, rows, D, C);
  else
    hipLaunchKernelGGL((probe_logits_kernel<4, 2>), grid, block, 0, s, feats, weight, bias, logits, rows, D, C);
  TT_CHECK_LAUNCH("probe_logits");
  return TT_OK;
}

extern "C" size_t tt_probe_upsample_ce_workspace_bytes(int B, int g) { return (size_t)(B > 0 ? B : 0) * (g > 0 ? g : 0) * 3 * sizeof(double); }

extern "C" int tt_probe_upsample_ce(const float* logits_low, const int64_t* labels, float* dlogits_low, float* loss_out, long long* counts_out,
                                    int B, int g, int C, int R, void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  TT_REQUIRE(logits_low && labels && dlogits_low && loss_out && counts_out && workspace, "probe_upsample_ce: null pointer");
  if (int rc = probe_grid_error(B, g, C, R)) return rc;
  TT_REQUIRE(workspace_bytes >= tt_probe_upsample_ce_workspace_bytes(B, g), "probe_upsample_ce: workspace too small");
  TT_REQUIRE(raise_gather_lds(), "probe_upsample_ce: could not raise the dynamic LDS limit");
  hipStream_t s = as_stream(stream);
  double* part_loss = static_cast<double*>(workspace);
  double* part_cnt = part_loss + (size_t)B * g;
  hipLaunchKernelGGL(probe_gather_kernel<true>, dim3(g, B), dim3(LP_THREADS), gather_lds_bytes(g, C, R), s, logits_low, labels, dlogits_low,
                     part_loss, part_cnt, g, C, R, gather_tp_log2(C));
  TT_CHECK_LAUNCH("probe_upsample_ce");
  const long long n = (long long)B * g * g * C;
  long long blocks = (n + LP_THREADS * 4 - 1) / (LP_THREADS * 4);
  blocks = blocks > 128 ? 128 : blocks;
  hipLaunchKernelGGL(probe_ce_finalize_kernel, dim3((unsigned)blocks), dim3(LP_THREADS), 0, s, part_loss, part_cnt, B * g, dlogits_low, n,
                     loss_out, counts_out);
  TT_CHECK_LAUNCH("probe_upsample_ce.finalize");
  return TT_OK;
}

extern "C" int tt_bilinear_adjoint_tokens(const float* d_hi, float* d_low, int B, int g, int C, int R, tt_stream_t stream) {
  TT_REQUIRE(d_hi && d_low, "bilinear_adjoint_tokens: null pointer");
  if (int rc = probe_grid_error(B, g, C, R)) return rc;
  TT_REQUIRE(raise_gather_lds(), "bilinear_adjoint_tokens: could not raise the dynamic LDS limit");
  hipLaunchKernelGGL(probe_gather_kernel<false>, dim3(g, B), dim3(LP_THREADS), gather_lds_bytes(g, C, R), as_stream(stream), d_hi,
                     (const int64_t*)nullptr, d_low, (double*)nullptr, (double*)nullptr, g, C, R, gather_tp_log2(C));
  TT_CHECK_LAUNCH("bilinear_adjoint_tokens");
  return TT_OK;
}

extern "C" size_t tt_probe_wgrad_workspace_bytes(long long rows, int D, int C) {
  if (rows <= 0 || D <= 0 || C <= 0) return 0;
  return (size_t)wgrad_split(rows, D, C).nsplit * wgrad_split_stride(D, C) * sizeof(float);
}

extern "C" int tt_probe_wgrad(const float* dlogits, const float* feats, const float* scale_device, float* dw, float* db, long long rows, int D,
                              int C, void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  TT_REQUIRE(dlogits && feats && dw && workspace && rows > 0, "probe_wgrad: bad arguments");
  if (int rc = probe_shape_error(D, C)) return rc;
  TT_REQUIRE(aligned16(feats) && aligned16(workspace), "probe_wgrad: feats and workspace must be 16-byte aligned");
  TT_REQUIRE(workspace_bytes >= tt_probe_wgrad_workspace_bytes(rows, D, C), "probe_wgrad: workspace too small");
  const WgradSplit sp = wgrad_split(rows, D, C);
  hipStream_t s = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(probe_wgrad_partial_kernel, dim3((D + 63) / 64, (C + 63) / 64, sp.nsplit), dim3(LP_THREADS), 0, s, dlogits, feats, part,
                     rows, D, C, sp.rows_per_split);
  TT_CHECK_LAUNCH("probe_wgrad");
  const long long n = (long long)C * D + C;
  long long blocks = (n + LP_THREADS - 1) / LP_THREADS;
  blocks = blocks > 2048 ? 2048 : blocks;
  hipLaunchKernelGGL(probe_wgrad_fold_kernel, dim3((unsigned)blocks), dim3(LP_THREADS), 0, s, part, sp.nsplit, wgrad_split_stride(D, C),
                     (long long)C * D, C, scale_device, dw, db);
  TT_CHECK_LAUNCH("probe_wgrad.fold");
  return TT_OK;
}

extern "C" int tt_sgd_step(const tt_adamw_tensor* tensors, int count, float momentum, int first_step, tt_stream_t stream) {
  TT_REQUIRE(tensors && count > 0 && count <= TT_MAX_TENSORS, "sgd_step: need 1..%d tensors", TT_MAX_TENSORS);
  SgdTable tab{};
  long long maxn = 0;
  for (int i = 0; i < count; ++i) {
    TT_REQUIRE(tensors[i].p && tensors[i].g && tensors[i].n > 0, "sgd_step: tensor %d has a null pointer", i);
    TT_REQUIRE(momentum == 0.f || tensors[i].m, "sgd_step: tensor %d has no momentum buffer", i);
    tab.t[i] = tensors[i];
    if (momentum == 0.f) tab.t[i].m = nullptr;
    if (tensors[i].n > maxn) maxn = tensors[i].n;
  }
  long long bx = (maxn + LP_THREADS - 1) / LP_THREADS;
  if (bx > 1024) bx = 1024;
  hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)bx, count), dim3(LP_THREADS), 0, as_stream(stream), tab, momentum, first_step);
  TT_CHECK_LAUNCH("sgd_step");
  return TT_OK;
}
