// FCN-head fine-tuning (N32): the device side of leopart.py:83-147 (FCNHead) - 3x3 convolutions over the token grid, forward and backward,
// in fp32 on v_mfma_f32_32x32x2_f32.
//
// Tokens are stored [B, gh*gw, C], which is NHWC, so a 3x3 convolution with zero padding is an implicit GEMM whose reduction runs over
// (tap, channel): the A operand of output row (b, i, j) at tap (di, dj) is the token row (b, i + di, j + dj), or zeros when that leaves
// the grid.  The test is made on the grid coordinates (i, j), never on the row index, so a tap cannot read the next row's first token or
// the next image's first row.  A second source xb continues the channel axis (concat_input): the concatenation is never stored.
//   tt_conv3x3_tokens_fwd          y = act(bias + conv(x, w)) * out_scale            repack + one GEMM launch
//   tt_conv3x3_tokens_bwd_data     dx[:, slice] = conv^T(dpre, w), zeroed by gate     repack + the same GEMM kernel
//   tt_conv3x3_tokens_bwd_weight   dw, db from dpre and the sources                   split-row TN product + fold
//   tt_fcn_head_grad               dpre = (dlogits wseg) * out_scale * [y > 0]        the gradient entering the last convolution
// The GEMM kernels read the weight TAP-MAJOR, wt[tap][k][n] with n contiguous: a slab of 16 reduction indices is then 16 rows of one tap,
// each a run of 16-byte loads, where nn.Conv2d's [Cout, Cin, 3, 3] has the nine taps innermost (a 36-byte stride between the channels of
// one tap).  The repack is one launch per call into the caller's workspace; backward-data repacks the FLIPPED taps of the channel slice,
// so that one kernel serves both directions.  Tiles are 128 x 128, 16 reduction indices per slab, two LDS buffers, the next slab's
// global loads issued before the current slab's MFMAs (the scheme of gemm_bwd_fast.hip).  Every sum has a fixed order and nothing is
// accumulated with atomics: two calls give the same bits.
#include "common.hpp"

namespace tt {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CT_MAXC = 1024, CT_MAXG = 64;
constexpr int CT_BK = 16, CT_LD = 128 + 4, CT_SZ = CT_BK * CT_LD;   // one operand slab: [16][128] floats, padded rows

__device__ __forceinline__ float4 ct_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 ct_zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// 16 reduction indices of a 128 x 128 tile: wave (wm, wn) owns 64 x 64 as 2 x 2 MFMA tiles.  Both slabs are [reduction][extent].
__device__ __forceinline__ void ct_mfma_slab(const float* a_slab, const float* b_slab, int wm, int wn, int r, int h, f32x16 (&acc)[2][2]) {
  const float* fa = a_slab + (4 * h) * CT_LD + wm * 64 + r;
  const float* fb = b_slab + (4 * h) * CT_LD + wn * 64 + r;
#pragma unroll
  for (int j = 0; j < CT_BK / 8; ++j) {
    float a[2][4], b[2][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i][q] = fa[(8 * j + q) * CT_LD + i * 32];
        b[i][q] = fb[(8 * j + q) * CT_LD + i * 32];
      }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][q], b[n][q], acc[i][n], 0, 0, 0);
  }
}

// The tile leaves through LDS, 64 rows at a time: put(row in tile, column in tile, four adjacent values) once per float4.
template <class Put>
__device__ __forceinline__ void ct_tile_out(float* lds, const f32x16 (&acc)[2][2], int wm, int wn, int r, int h, Put&& put) {
  const int tid = threadIdx.x, c4 = (tid & 31) * 4;
#pragma unroll
  for (int wmi = 0; wmi < 2; ++wmi) {
    if (wm == wmi) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) lds[(i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h) * CT_LD + wn * 64 + j * 32 + r] = acc[i][j][e];
    }
    __syncthreads();
    for (int rr = tid >> 5; rr < 64; rr += 8) put(wmi * 64 + rr, c4, ct_ld4(lds + rr * CT_LD + c4));
    __syncthreads();
  }
}

// ---- weight repack: out[tap][k][n], n contiguous.
//   forward        k = input channel, n = output channel: out = w[n][k][tap]
//   backward data  k = output channel, n = channel c_begin + n of the input, taps flipped: out = w[k][c_begin + n][8 - tap]
__global__ __launch_bounds__(256) void conv_repack_kernel(const float* __restrict__ w, float* __restrict__ out, int K, int N, int Cin, int c_begin,
                                                          int backward) {
  const long long total = 9LL * K * N;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int n = (int)(e % N);
    const long long q = e / N;
    const int k = (int)(q % K), tap = (int)(q / K);
    out[e] = backward ? w[((long long)k * Cin + c_begin + n) * 9 + (8 - tap)] : w[((long long)n * Cin + k) * 9 + tap];
  }
}

// ---- out[m][n] = epilogue(sum over tap, k of src(m shifted by tap)[k] * wt[tap][k][n]): forward and backward data.
struct ConvArgs {
  const float* xa;          // [rows][Ca]
  const float* xb;          // [rows][Cb] or null (Cb == 0): channels Ca .. Ca + Cb - 1 of the reduction
  const float* wt;          // [9][K][N], K = Ca + Cb
  float* out;               // [rows][N]
  const float* bias;        // [N] or null
  const float* out_scale;   // [B][N] or null
  const float* gate;        // [rows][N] or null: the result is zero where gate <= 0
  long long rows;
  int gh, gw, Ca, Cb, K, N, act;
};

__global__ __launch_bounds__(256) void conv_gemm_kernel(ConvArgs g) {
  __shared__ __attribute__((aligned(16))) float lds[4 * CT_SZ];   // A0 A1 B0 B1; 4 * CT_SZ = 64 * CT_LD: the epilogue's image fits
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const int ntn = (g.N + 127) / 128, ntm = (int)((g.rows + 127) / 128);
  const int tile = xcd_remap(blockIdx.x, ntm * ntn);
  const long long m0 = (long long)(tile / ntn) * 128;
  const int n0 = (tile % ntn) * 128;
  const int npix = g.gh * g.gw, nkc = (g.K + CT_BK - 1) / CT_BK;

  // A staging: thread owns output rows tid / 4 and tid / 4 + 64 and the four channels at (tid % 4) * 4 of a slab
  const int kc = (tid & 3) * 4;
  long long am[2];   // the output row, or -1 past the end
  int ai[2], aj[2];  // its grid coordinates
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long long m = m0 + (tid >> 2) + 64 * i;
    const int p = (int)(m % npix);
    am[i] = m < g.rows ? m : -1;
    ai[i] = p / g.gw;
    aj[i] = p - ai[i] * g.gw;
  }
  // B staging: slab rows tid / 32 and tid / 32 + 8, the four columns at (tid % 32) * 4
  const int bk = tid >> 5, bn = n0 + (tid & 31) * 4;
  const bool b_in = bn < g.N;
  float4 ra[2], rb[2];
  auto gload = [&](int kt) {
    const int tap = kt / nkc, k0 = (kt - tap * nkc) * CT_BK;
    const int di = tap / 3 - 1, dj = tap - (tap / 3) * 3 - 1;
    const int c = k0 + kc;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      ra[i] = ct_zero4();
      if (am[i] >= 0 && c < g.K && (unsigned)(ai[i] + di) < (unsigned)g.gh && (unsigned)(aj[i] + dj) < (unsigned)g.gw) {
        const long long s = am[i] + di * g.gw + dj;   // same image: the grid test above keeps it inside
        ra[i] = c < g.Ca ? ct_ld4(g.xa + s * g.Ca + c) : ct_ld4(g.xb + s * g.Cb + (c - g.Ca));
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int k = k0 + bk + 8 * i;
      rb[i] = b_in && k < g.K ? ct_ld4(g.wt + ((size_t)tap * g.K + k) * g.N + bn) : ct_zero4();
    }
  };
  auto sstore = [&](int buf) {
    float* da = lds + buf * CT_SZ;
    float* db = lds + (2 + buf) * CT_SZ;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (tid >> 2) + 64 * i;
      da[(kc + 0) * CT_LD + row] = ra[i].x;
      da[(kc + 1) * CT_LD + row] = ra[i].y;
      da[(kc + 2) * CT_LD + row] = ra[i].z;
      da[(kc + 3) * CT_LD + row] = ra[i].w;
      *reinterpret_cast<float4*>(db + (bk + 8 * i) * CT_LD + (tid & 31) * 4) = rb[i];
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  const int nk = 9 * nkc;
  gload(0);
  sstore(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) gload(kt + 1);
    ct_mfma_slab(lds + buf * CT_SZ, lds + (2 + buf) * CT_SZ, wm, wn, r, h, acc);
    if (kt + 1 < nk) sstore(buf ^ 1);
    __syncthreads();
  }
  ct_tile_out(lds, acc, wm, wn, r, h, [&](int rr, int c4, float4 v) {
    const long long m = m0 + rr;
    const int n = n0 + c4;
    if (m >= g.rows || n >= g.N) return;
    if (g.bias) {
      const float4 b = ct_ld4(g.bias + n);
      v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
    }
    if (g.act) {
      v.x = v.x < 0.f ? 0.f : v.x; v.y = v.y < 0.f ? 0.f : v.y; v.z = v.z < 0.f ? 0.f : v.z; v.w = v.w < 0.f ? 0.f : v.w;
    }
    if (g.out_scale) {
      const float4 s = ct_ld4(g.out_scale + (m / npix) * g.N + n);
      v.x *= s.x; v.y *= s.y; v.z *= s.z; v.w *= s.w;
    }
    if (g.gate) {
      const float4 t = ct_ld4(g.gate + m * g.N + n);
      v.x = t.x <= 0.f ? 0.f : v.x; v.y = t.y <= 0.f ? 0.f : v.y; v.z = t.z <= 0.f ? 0.f : v.z; v.w = t.w <= 0.f ? 0.f : v.w;
    }
    *reinterpret_cast<float4*>(g.out + m * g.N + n) = v;
  });
}

// ---- weight gradient, stage 1: part[z][tap][co][ci] = sum over the rows of slice z of dpre[row][co] * src(row shifted by tap)[ci], a TN
// product whose B operand is gathered.  The workgroups of tap 0 and input tile 0 also sum the dpre rows they stage: colpart[z][co].
struct ConvWgradArgs {
  const float* dpre;   // [rows][Cout]
  const float* xa;     // [rows][Ca]
  const float* xb;     // [rows][Cb] or null
  float* part;         // [nsplit][9][Cout][Cin]
  float* colpart;      // [nsplit][Cout] or null
  long long rows, chunk;   // chunk: rows per slice, a multiple of 16
  int gh, gw, Ca, Cb, Cin, Cout;
};

__global__ __launch_bounds__(256) void conv_wgrad_kernel(ConvWgradArgs g) {
  __shared__ __attribute__((aligned(16))) float lds[4 * CT_SZ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const int ntn = (g.Cin + 127) / 128, ntm = (g.Cout + 127) / 128, per_tap = ntm * ntn;
  const int id = xcd_remap(blockIdx.x, 9 * per_tap);
  const int tap = id / per_tap, t = id - tap * per_tap;
  const int m0 = (t / ntn) * 128, n0 = (t % ntn) * 128;
  const int di = tap / 3 - 1, dj = tap - (tap / 3) * 3 - 1;
  const int z = blockIdx.z;
  const long long rbeg = (long long)z * g.chunk, rend = rbeg + g.chunk < g.rows ? rbeg + g.chunk : g.rows;
  const int npix = g.gh * g.gw;
  const float inv_gw = 1.0f / (float)g.gw;

  // staging: thread owns slab rows tid / 32 and tid / 32 + 8 and the four columns at (tid % 32) * 4 of both operand tiles
  const int kr = tid >> 5, c4 = (tid & 31) * 4;
  const bool a_in = m0 + c4 < g.Cout;
  const int cb = n0 + c4;
  const bool b_in = cb < g.Cin;
  const bool from_a = cb < g.Ca || !b_in;
  const float* bsrc = from_a ? g.xa + (b_in ? cb : 0) : g.xb + (cb - g.Ca);   // only dereferenced when b_in
  const int ldb = from_a ? g.Ca : g.Cb;
  const bool colsum = g.colpart && tap == 0 && n0 == 0;   // uniform over the workgroup
  int p[2];   // position inside its image of this thread's row of the NEXT slab to load (kept from slab to slab)
#pragma unroll
  for (int i = 0; i < 2; ++i) p[i] = (int)((rbeg + kr + 8 * i) % npix);
  float4 ra[2], rb[2];
  float4 csum = ct_zero4();
  auto gload = [&](long long row0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long long row = row0 + kr + 8 * i;
      ra[i] = ct_zero4();
      rb[i] = ct_zero4();
      if (row < rend) {
        if (a_in) ra[i] = ct_ld4(g.dpre + row * g.Cout + m0 + c4);
        if (b_in) {
          // the grid row by a float reciprocal: exact for p < 2^20 (p < 64 * 64 here)
          const int gi = (int)(((float)p[i] + 0.5f) * inv_gw), gj = p[i] - gi * g.gw;
          if ((unsigned)(gi + di) < (unsigned)g.gh && (unsigned)(gj + dj) < (unsigned)g.gw) rb[i] = ct_ld4(bsrc + (row + di * g.gw + dj) * ldb);
        }
      }
      if (colsum) {
        csum.x += ra[i].x; csum.y += ra[i].y; csum.z += ra[i].z; csum.w += ra[i].w;
      }
      p[i] += CT_BK;
      if (p[i] >= npix) p[i] -= (p[i] / npix) * npix;
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<float4*>(lds + buf * CT_SZ + (kr + 8 * i) * CT_LD + c4) = ra[i];
      *reinterpret_cast<float4*>(lds + (2 + buf) * CT_SZ + (kr + 8 * i) * CT_LD + c4) = rb[i];
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  const int nk = (int)((rend - rbeg + CT_BK - 1) / CT_BK);   // >= 1: every slice has rows (conv_wgrad_split)
  gload(rbeg);
  sstore(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) gload(rbeg + (long long)(kt + 1) * CT_BK);
    ct_mfma_slab(lds + buf * CT_SZ, lds + (2 + buf) * CT_SZ, wm, wn, r, h, acc);
    if (kt + 1 < nk) sstore(buf ^ 1);
    __syncthreads();
  }
  float* out = g.part + ((size_t)z * 9 + tap) * g.Cout * g.Cin;
  ct_tile_out(lds, acc, wm, wn, r, h, [&](int rr, int cc, float4 v) {
    const int m = m0 + rr, n = n0 + cc;
    if (m < g.Cout && n < g.Cin) *reinterpret_cast<float4*>(out + (size_t)m * g.Cin + n) = v;
  });
  if (colsum) {   // the 8 threads that share a column quad, in order (ct_tile_out ended on a barrier: the LDS is free)
    *reinterpret_cast<float4*>(lds + kr * CT_LD + c4) = csum;
    __syncthreads();
    if (tid < 128 && m0 + tid < g.Cout) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) s += lds[k * CT_LD + tid];
      g.colpart[(size_t)z * g.Cout + m0 + tid] = s;
    }
  }
}

// Stage 2: dw[co][ci][tap] = mult * sum over the slices (in order) of part[z][tap][co][ci] for workgroups [0, blocks_main); the rest take
// 64 columns each of db (common.hpp colsum_fold_block: the order of every bias gradient here).
__global__ __launch_bounds__(256) void conv_wgrad_fold_kernel(const float* __restrict__ part, const float* __restrict__ colpart, int nsplit,
                                                              int Cout, int Cin, const float* __restrict__ mult, float* __restrict__ dw,
                                                              float* __restrict__ db, int blocks_main) {
  __shared__ float red[4][64];
  const float m = mult ? *mult : 1.f;
  if ((int)blockIdx.x >= blocks_main) {
    const int blk = (int)blockIdx.x - blocks_main, n = blk * 64 + (threadIdx.x & 63);
    colsum_fold_block(colpart, db, nsplit, Cout, Cout, 0, blk, red);
    if (mult && threadIdx.x < 64 && n < Cout) db[n] *= m;   // the thread that wrote it
    return;
  }
  const size_t plane = (size_t)Cout * Cin;
  const long long total = 9LL * Cout * Cin;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)blocks_main * 256) {
    const int tap = (int)(e % 9);
    const size_t q = (size_t)(e / 9);
    float s = 0.f;
    for (int zz = 0; zz < nsplit; ++zz) s += part[((size_t)zz * 9 + tap) * plane + q];
    dw[e] = s * m;
  }
}

// ---- dpre[m][c] = (sum over k of dlogits[m][k] * wseg[k][c]) * out_scale[b][c] * [y[m][c] > 0]: the gradient entering the last
// convolution, from the gradient of the token-resolution logits.  Thread: 4 rows x 4 channels, k ascending.
__global__ __launch_bounds__(256) void fcn_head_grad_kernel(const float* __restrict__ dl, const float* __restrict__ wseg,
                                                            const float* __restrict__ out_scale, const float* __restrict__ y,
                                                            float* __restrict__ dpre, long long rows, int npix, int C, int N) {
  const int nq = N / 4;
  const long long total = (rows + 3) / 4 * nq;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int c = (int)(e % nq) * 4;
    const long long m0 = e / nq * 4;
    float4 acc[4] = {ct_zero4(), ct_zero4(), ct_zero4(), ct_zero4()};
    for (int k = 0; k < C; ++k) {
      const float4 w = ct_ld4(wseg + (size_t)k * N + c);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float d = m0 + i < rows ? dl[(m0 + i) * C + k] : 0.f;
        acc[i].x = fmaf(d, w.x, acc[i].x); acc[i].y = fmaf(d, w.y, acc[i].y); acc[i].z = fmaf(d, w.z, acc[i].z); acc[i].w = fmaf(d, w.w, acc[i].w);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long m = m0 + i;
      if (m >= rows) break;
      float4 v = acc[i];
      if (out_scale) {
        const float4 s = ct_ld4(out_scale + (m / npix) * N + c);
        v.x *= s.x; v.y *= s.y; v.z *= s.z; v.w *= s.w;
      }
      if (y) {
        const float4 t = ct_ld4(y + m * N + c);
        v.x = t.x > 0.f ? v.x : 0.f; v.y = t.y > 0.f ? v.y : 0.f; v.z = t.z > 0.f ? v.z : 0.f; v.w = t.w > 0.f ? v.w : 0.f;
      }
      *reinterpret_cast<float4*>(dpre + m * N + c) = v;
    }
  }
}

// ---- host side
static int conv_grid_error(const char* who, int B, int gh, int gw, long long* rows) {
  TT_REQUIRE(B >= 1, "%s: need B >= 1 (got %d)", who, B);
  TT_REQUIRE(gh >= 1 && gh <= CT_MAXG && gw >= 1 && gw <= CT_MAXG, "%s: need 1 <= gh, gw <= %d (got %d x %d)", who, CT_MAXG, gh, gw);
  *rows = (long long)B * gh * gw;
  TT_REQUIRE(*rows < (1LL << 31), "%s: need B * gh * gw < 2^31 (got %lld)", who, *rows);
  return TT_OK;
}

static int conv_channel_error(const char* who, int Ca, int Cb, int Cout) {
  TT_REQUIRE(Ca >= 4 && Ca % 4 == 0 && Ca <= CT_MAXC, "%s: need Ca %% 4 == 0 and 4 <= Ca <= %d (got %d)", who, CT_MAXC, Ca);
  TT_REQUIRE(Cb >= 0 && Cb % 4 == 0 && Cb <= CT_MAXC, "%s: need Cb %% 4 == 0 and 0 <= Cb <= %d (got %d)", who, CT_MAXC, Cb);
  TT_REQUIRE(Cout >= 4 && Cout % 4 == 0 && Cout <= CT_MAXC, "%s: need Cout %% 4 == 0 and 4 <= Cout <= %d (got %d)", who, CT_MAXC, Cout);
  return TT_OK;
}

static void conv_repack(const float* w, float* out, int K, int N, int Cin, int c_begin, int backward, hipStream_t s) {
  long long blocks = (9LL * K * N + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(conv_repack_kernel, dim3((unsigned)blocks), dim3(256), 0, s, w, out, K, N, Cin, c_begin, backward);
}

static unsigned conv_gemm_tiles(long long rows, int N) { return (unsigned)(((rows + 127) / 128) * ((N + 127) / 128)); }

struct ConvWgradSplit {
  int nsplit;
  long long chunk;
};
// Slices of the rows: enough for about two workgroups per CU, none shorter than 64 rows, at most 64 of them; every slice has rows.
static ConvWgradSplit conv_wgrad_split(long long rows, int Cin, int Cout) {
  const long long tiles = 9LL * ((Cin + 127) / 128) * ((Cout + 127) / 128);
  long long ns = (512 + tiles - 1) / tiles;
  const long long most = (rows + 63) / 64;
  if (ns > most) ns = most;
  if (ns > 64) ns = 64;
  if (ns < 1) ns = 1;
  const long long chunk = ((rows + ns - 1) / ns + CT_BK - 1) / CT_BK * CT_BK;
  return ConvWgradSplit{(int)((rows + chunk - 1) / chunk), chunk};
}
static size_t conv_wgrad_part_floats(int nsplit, int Cin, int Cout) { return (size_t)nsplit * 9 * Cout * Cin; }

}  // namespace tt

using namespace tt;

extern "C" size_t tt_conv3x3_tokens_fwd_workspace_bytes(int Ca, int Cb, int Cout) {
  if (Ca <= 0 || Cb < 0 || Cout <= 0) return 0;
  return (size_t)9 * (Ca + Cb) * Cout * sizeof(float);
}

extern "C" int tt_conv3x3_tokens_fwd(const float* xa, const float* xb, const float* weight, const float* bias, const float* out_scale, float* y,
                                     int B, int gh, int gw, int Ca, int Cb, int Cout, int act, void* workspace, size_t workspace_bytes,
                                     tt_stream_t stream) {
  const char* who = "conv3x3_tokens_fwd";
  TT_REQUIRE(xa && weight && y && workspace, "%s: null pointer", who);
  long long rows;
  if (int rc = conv_grid_error(who, B, gh, gw, &rows)) return rc;
  if (int rc = conv_channel_error(who, Ca, Cb, Cout)) return rc;
  TT_REQUIRE(Cb == 0 || xb, "%s: Cb = %d without a second source", who, Cb);
  TT_REQUIRE(act == 0 || act == 1, "%s: act must be 0 or 1 (ReLU) (got %d)", who, act);
  TT_REQUIRE(aligned16(xa) && aligned16(xb) && aligned16(bias) && aligned16(out_scale) && aligned16(y) && aligned16(workspace),
             "%s: every pointer must be 16-byte aligned", who);
  TT_REQUIRE(workspace_bytes >= tt_conv3x3_tokens_fwd_workspace_bytes(Ca, Cb, Cout), "%s: workspace too small", who);
  hipStream_t s = as_stream(stream);
  float* wt = static_cast<float*>(workspace);
  conv_repack(weight, wt, Ca + Cb, Cout, Ca + Cb, 0, 0, s);
  TT_CHECK_LAUNCH("conv3x3_tokens_fwd.repack");
  ConvArgs g{xa, Cb ? xb : nullptr, wt, y, bias, out_scale, nullptr, rows, gh, gw, Ca, Cb, Ca + Cb, Cout, act};
  hipLaunchKernelGGL(conv_gemm_kernel, dim3(conv_gemm_tiles(rows, Cout)), dim3(256), 0, s, g);
  TT_CHECK_LAUNCH("conv3x3_tokens_fwd");
  return TT_OK;
}

extern "C" size_t tt_conv3x3_tokens_bwd_data_workspace_bytes(int Cout, int c_count) {
  if (Cout <= 0 || c_count <= 0) return 0;
  return (size_t)9 * Cout * c_count * sizeof(float);
}

extern "C" int tt_conv3x3_tokens_bwd_data(const float* dpre, const float* weight, const float* gate, float* dx, int B, int gh, int gw, int Cin,
                                          int Cout, int c_begin, int c_count, void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  const char* who = "conv3x3_tokens_bwd_data";
  TT_REQUIRE(dpre && weight && dx && workspace, "%s: null pointer", who);
  long long rows;
  if (int rc = conv_grid_error(who, B, gh, gw, &rows)) return rc;
  TT_REQUIRE(Cin >= 4 && Cin % 4 == 0 && Cin <= 2 * CT_MAXC, "%s: need Cin %% 4 == 0 and 4 <= Cin <= %d (got %d)", who, 2 * CT_MAXC, Cin);
  TT_REQUIRE(Cout >= 4 && Cout % 4 == 0 && Cout <= CT_MAXC, "%s: need Cout %% 4 == 0 and 4 <= Cout <= %d (got %d)", who, CT_MAXC, Cout);
  TT_REQUIRE(c_begin >= 0 && c_count >= 4 && c_count % 4 == 0 && c_count <= CT_MAXC && c_begin <= Cin - c_count,
             "%s: need a channel slice inside [0, %d) with c_count %% 4 == 0 and 4 <= c_count <= %d (got begin %d, count %d)", who, Cin, CT_MAXC,
             c_begin, c_count);
  TT_REQUIRE(aligned16(dpre) && aligned16(gate) && aligned16(dx) && aligned16(workspace), "%s: every pointer must be 16-byte aligned", who);
  TT_REQUIRE(workspace_bytes >= tt_conv3x3_tokens_bwd_data_workspace_bytes(Cout, c_count), "%s: workspace too small", who);
  hipStream_t s = as_stream(stream);
  float* wt = static_cast<float*>(workspace);
  conv_repack(weight, wt, Cout, c_count, Cin, c_begin, 1, s);
  TT_CHECK_LAUNCH("conv3x3_tokens_bwd_data.repack");
  ConvArgs g{dpre, nullptr, wt, dx, nullptr, nullptr, gate, rows, gh, gw, Cout, 0, Cout, c_count, 0};
  hipLaunchKernelGGL(conv_gemm_kernel, dim3(conv_gemm_tiles(rows, c_count)), dim3(256), 0, s, g);
  TT_CHECK_LAUNCH("conv3x3_tokens_bwd_data");
  return TT_OK;
}

extern "C" size_t tt_conv3x3_tokens_bwd_weight_workspace_bytes(long long rows, int Cin, int Cout) {
  if (rows <= 0 || Cin <= 0 || Cout <= 0) return 0;
  const ConvWgradSplit sp = conv_wgrad_split(rows, Cin, Cout);
  return (conv_wgrad_part_floats(sp.nsplit, Cin, Cout) + (size_t)sp.nsplit * Cout) * sizeof(float);
}

extern "C" int tt_conv3x3_tokens_bwd_weight(const float* dpre, const float* xa, const float* xb, const float* scale_device, float* dw, float* db,
                                            int B, int gh, int gw, int Ca, int Cb, int Cout, void* workspace, size_t workspace_bytes,
                                            tt_stream_t stream) {
  const char* who = "conv3x3_tokens_bwd_weight";
  TT_REQUIRE(dpre && xa && dw && workspace, "%s: null pointer", who);
  long long rows;
  if (int rc = conv_grid_error(who, B, gh, gw, &rows)) return rc;
  if (int rc = conv_channel_error(who, Ca, Cb, Cout)) return rc;
  TT_REQUIRE(Cb == 0 || xb, "%s: Cb = %d without a second source", who, Cb);
  TT_REQUIRE(aligned16(dpre) && aligned16(xa) && aligned16(xb) && aligned16(workspace), "%s: dpre, the sources and the workspace must be 16-byte aligned",
             who);
  const int Cin = Ca + Cb;
  TT_REQUIRE(workspace_bytes >= tt_conv3x3_tokens_bwd_weight_workspace_bytes(rows, Cin, Cout), "%s: workspace too small", who);
  const ConvWgradSplit sp = conv_wgrad_split(rows, Cin, Cout);
  hipStream_t s = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  float* colpart = part + conv_wgrad_part_floats(sp.nsplit, Cin, Cout);
  ConvWgradArgs g{dpre, xa, Cb ? xb : nullptr, part, db ? colpart : nullptr, rows, sp.chunk, gh, gw, Ca, Cb, Cin, Cout};
  const unsigned tiles = 9u * ((Cin + 127) / 128) * ((Cout + 127) / 128);
  hipLaunchKernelGGL(conv_wgrad_kernel, dim3(tiles, 1, sp.nsplit), dim3(256), 0, s, g);
  TT_CHECK_LAUNCH("conv3x3_tokens_bwd_weight");
  long long blocks = (9LL * Cout * Cin + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  const int bias_blocks = db ? (Cout + 63) / 64 : 0;
  hipLaunchKernelGGL(conv_wgrad_fold_kernel, dim3((unsigned)blocks + bias_blocks), dim3(256), 0, s, part, colpart, sp.nsplit, Cout, Cin,
                     scale_device, dw, db, (int)blocks);
  TT_CHECK_LAUNCH("conv3x3_tokens_bwd_weight.fold");
  return TT_OK;
}

extern "C" int tt_fcn_head_grad(const float* dlogits, const float* wseg, const float* out_scale, const float* y, float* dpre, int B, int gh,
                                int gw, int C, int channels, tt_stream_t stream) {
  const char* who = "fcn_head_grad";
  TT_REQUIRE(dlogits && wseg && dpre, "%s: null pointer", who);
  long long rows;
  if (int rc = conv_grid_error(who, B, gh, gw, &rows)) return rc;
  TT_REQUIRE(C >= 1 && C <= 256, "%s: need 1 <= classes <= 256 (got %d)", who, C);
  TT_REQUIRE(channels >= 4 && channels % 4 == 0 && channels <= CT_MAXC, "%s: need channels %% 4 == 0 and 4 <= channels <= %d (got %d)", who,
             CT_MAXC, channels);
  TT_REQUIRE(aligned16(wseg) && aligned16(out_scale) && aligned16(y) && aligned16(dpre), "%s: wseg, out_scale, y and dpre must be 16-byte aligned", who);
  long long blocks = ((rows + 3) / 4 * (channels / 4) + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(fcn_head_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), dlogits, wseg, out_scale, y, dpre, rows,
                     gh * gw, C, channels);
  TT_CHECK_LAUNCH("fcn_head_grad");
  return TT_OK;
}
