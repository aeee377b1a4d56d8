// Backward of the stem (prepare_tokens, dino_vision_transformer.py:166-171, 236-247): the gradients of everything below block 0.
//   x[f, 0]     = cls + pos[0]
//   x[f, 1 + p] = w @ patch(img[frame_map[f]], p) + bias + pos[1 + p]
// so with dtok [F, n+1, D] the gradient entering block 0:
//   dw[D, C P P]   = sum over (f, p) of dtok[f, 1 + p, :] (x) patch(img[frame_map[f]], p)     stem_wgrad_kernel + stem_fold_kernel
//   dtable[n+1, D] = sum over f of dtok[f]                                                    stem_table_kernel
//   dcls[D]        = dtable[0],   dbias[D] = sum over p >= 1 of dtable[p]                     stem_table_kernel / stem_fold_kernel
// and, where the token grid is not the stored square one, dpos = the adjoint of the bicubic resampling of the position table
// (pos_embed_bicubic_bwd_kernel; forward: attn_mask.hip pos_embed_bicubic_kernel).
// Every sum has a fixed order and no float atomics: two calls give the same bits.
#include "common.hpp"
#include "interp.hpp"

namespace tt {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct StemArgs {
  const float* dtok;      // [F][n + 1][D]
  const float* img;       // [F_src][C][H][W]
  const int* frame_map;   // [F] or null (identity)
  float* out;             // [splits][D][K]: the partial tiles (the workspace), or dw itself when splits == 1
  int F, C, H, W, P, D;
  int K, gw, n, R;        // K = C P P, n = patches per frame, R = F n rows of the product
  int chunk;              // rows per slice (a multiple of 16)
};

// dw = dtok_patch_rows^T @ patches as a TN product on v_mfma_f32_32x32x2_f32 (the scheme of gemm_bwd_fast.hip's weight gradient: both
// operands [reduction][extent], 64 x 64 output tile, 16 reduction rows per slab, two LDS buffers, the next slab's global loads issued
// before the current slab's MFMAs).  The A operand is dtok read with row stride D, skipping each frame's class row; the B operand is
// never materialised: slab row (f, p) and columns k .. k+3 = (c, py, px .. px+3) are four contiguous pixels of the image (P % 4 == 0 and
// W % 4 == 0: one 16-byte load).  blockIdx.z = the slice of rows; rows past the slice's end and columns past D / K load zeros, so any
// F n, D % 4 == 0 and K % 4 == 0 are taken; an empty slice writes a zero tile.
__global__ __launch_bounds__(256) void stem_wgrad_kernel(StemArgs g) {
  constexpr int BK = 16, LD = 64 + 4, SZ = BK * LD;
  __shared__ __attribute__((aligned(16))) float lds[4 * SZ];   // A0 A1 B0 B1; 4 * SZ = 64 * LD: the epilogue's tile image fits
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const int ntn = (g.K + 63) / 64, ntm = (g.D + 63) / 64;
  const int tile = xcd_remap(blockIdx.x, ntm * ntn);
  const int m0 = (tile / ntn) * 64, n0 = (tile % ntn) * 64;
  const int z = blockIdx.z;
  const int rbeg = z * g.chunk, rend = min(g.R, rbeg + g.chunk);

  // staging: thread owns slab row tid / 16 and the four columns at (tid % 16) * 4 of both operand tiles
  const int kr = tid >> 4, c4 = (tid & 15) * 4;
  const bool a_in = m0 + c4 < g.D, b_in = n0 + c4 < g.K;
  size_t b_off = 0;   // offset of (c, py, px) inside a frame, from the patch's top-left pixel
  if (b_in) {
    const int k = n0 + c4, pp = g.P * g.P;
    const int c = k / pp, rem = k - c * pp, py = rem / g.P, px = rem - py * g.P;
    b_off = ((size_t)c * g.H + py) * g.W + px;
  }
  const size_t frame_elems = (size_t)g.C * g.H * g.W;
  // (frame, patch) of this thread's row of the NEXT slab to load, kept from slab to slab: a slab step is + 16 patches and the two integer
  // divisions of a fresh row index only where that crosses a frame - they sat on the address path of every slab's loads.  The grid row of
  // a patch by a float reciprocal: exact while n < 2^20 (stem_shape_rule), the quotient's error is far below the 0.5 / gw it may have
  int f = (rbeg + kr) / g.n, p = (rbeg + kr) - f * g.n;
  const float inv_gw = 1.0f / (float)g.gw;
  float4 ra, rb;
  auto gload = [&](int row0) {
    const int row = row0 + kr;
    ra = make_float4(0.f, 0.f, 0.f, 0.f);
    rb = ra;
    if (row < rend) {
      if (a_in) ra = *reinterpret_cast<const float4*>(g.dtok + ((size_t)f * (g.n + 1) + 1 + p) * g.D + m0 + c4);
      if (b_in) {
        const int fs = g.frame_map ? g.frame_map[f] : f;
        const int pr = (int)(((float)p + 0.5f) * inv_gw), pc = p - pr * g.gw;
        rb = *reinterpret_cast<const float4*>(g.img + (size_t)fs * frame_elems + ((size_t)pr * g.P) * g.W + pc * g.P + b_off);
      }
    }
    p += BK;
    if (p >= g.n) {
      const int q = p / g.n;
      f += q;
      p -= q * g.n;
    }
  };
  auto sstore = [&](int buf) {
    *reinterpret_cast<float4*>(lds + buf * SZ + kr * LD + c4) = ra;
    *reinterpret_cast<float4*>(lds + (2 + buf) * SZ + kr * LD + c4) = rb;
  };
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  const int nk = rend > rbeg ? (rend - rbeg + BK - 1) / BK : 0;   // uniform across the workgroup
  if (nk > 0) {
    gload(rbeg);
    sstore(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int buf = kt & 1;
      if (kt + 1 < nk) gload(rbeg + (kt + 1) * BK);
      const float* fa = lds + buf * SZ + (4 * h) * LD + wm * 32 + r;
      const float* fb = lds + (2 + buf) * SZ + (4 * h) * LD + wn * 32 + r;
#pragma unroll
      for (int j = 0; j < BK / 8; ++j) {
        float a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          a[q] = fa[(8 * j + q) * LD];
          b[q] = fb[(8 * j + q) * LD];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], b[q], acc, 0, 0, 0);
      }
      if (kt + 1 < nk) sstore(buf ^ 1);
      __syncthreads();
    }
  }
  // the tile leaves through LDS as 16-byte row-major stores (rows past D and columns past K are not stored)
#pragma unroll
  for (int e = 0; e < 16; ++e) lds[(wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * h) * LD + wn * 32 + r] = acc[e];
  __syncthreads();
  float* C = g.out + (size_t)z * g.D * g.K;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rr = kr + 16 * i;
    if (m0 + rr < g.D && b_in)
      *reinterpret_cast<float4*>(C + (size_t)(m0 + rr) * g.K + n0 + c4) = *reinterpret_cast<const float4*>(lds + rr * LD + c4);
  }
}

// dtable[t][d] = sum over f (ascending) of dtok[f][t][d]; dcls = row 0.  One thread per (t, four d's) of the first count4 float4s of a
// frame (stride4 apart: the class row alone when only dcls is asked for).
__global__ __launch_bounds__(256) void stem_table_kernel(const float* __restrict__ dtok, float* __restrict__ dtable, float* __restrict__ dcls,
                                                         int F, long long count4, long long stride4, int d4) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= count4) return;
  const float4* p = reinterpret_cast<const float4*>(dtok) + i;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
  for (int f = 0; f < F; ++f) {
    const float4 v = p[(long long)f * stride4];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  if (dtable) reinterpret_cast<float4*>(dtable)[i] = s;
  if (dcls && i < d4) reinterpret_cast<float4*>(dcls)[i] = s;
}

// One launch for the two folds: workgroups [0, blocks_main) fold the partial tiles into dw (slice order 0, 1, ...), the rest take 64
// columns each of dbias = sum over the patch rows of dtable (common.hpp colsum_fold_block: the order of every bias gradient here).
__global__ __launch_bounds__(256) void stem_fold_kernel(const float* __restrict__ partial, float* __restrict__ dw, long long n4, int splits,
                                                        int blocks_main, const float* __restrict__ table_rows, float* __restrict__ dbias,
                                                        int n_patch, int D) {
  __shared__ float red[4][64];
  if ((int)blockIdx.x >= blocks_main) {
    colsum_fold_block(table_rows, dbias, n_patch, D, D, 0, (int)blockIdx.x - blocks_main, red);
    return;
  }
  const float4* p = reinterpret_cast<const float4*>(partial);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)blocks_main * 256) {
    float4 s = p[i];
    for (int zz = 1; zz < splits; ++zz) {
      const float4 v = p[i + zz * n4];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    reinterpret_cast<float4*>(dw)[i] = s;
  }
}

// Weight with which output coordinate o taps source cell s along one axis: the forward's four taps at clamp(floor(r) - 1 + i, 0, g - 1)
// (several taps of a border output fall on the same cell: their weights add up, in tap order).
__device__ __forceinline__ float stem_axis_weight(int o, int s, int g, float rscale) {
  const float rr = rscale * (o + 0.5f) - 0.5f;
  const float fl = floorf(rr);
  float w[4];
  cubic_coeffs(rr - fl, w);   // interp.hpp: the forward's weight function itself
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (min(max((int)fl - 1 + i, 0), g - 1) == s) sum += w[i];
  return sum;
}
// Outputs that can tap source cell s: their source coordinate lies within 2 of s (3 here: a unit of margin against rounding - the exact
// test is stem_axis_weight's); the border cells also collect every clamped tap beyond them.
__device__ __forceinline__ void stem_axis_range(int s, int g, int go, float rscale, int& lo, int& hi) {
  const float inv = 1.f / rscale;
  lo = (int)floorf((s - 3 + 0.5f) * inv - 0.5f) - 1;
  hi = (int)ceilf((s + 3 + 0.5f) * inv - 0.5f) + 1;
  if (s == 0) lo = 0;
  if (s == g - 1) hi = go - 1;
  lo = max(lo, 0);
  hi = min(hi, go - 1);
}

// s + lo += c * v, compensated (the product's rounding error by fma, the sum's by the branch-free two-sum): an upscaled grid puts
// (4 scale)^2 taps on a source cell - 64 at 14 -> 28 - and a plain fp32 chain over them measured up to 2^-22 of sum |terms|, the whole
// budget of the adjoint's check; with the compensation the sum is good to the last bit or two whatever the number of taps.  Still fp32,
// still one fixed order.  (Contraction is off here: fusing c * v into the sum would break the two-sum's identity.)
__device__ __forceinline__ void comp_fma(float& s, float& lo, float c, float v) {
#pragma clang fp contract(off)
  const float p = c * v;
  const float pe = fmaf(c, v, -p);
  const float t = s + p;
  const float bp = t - s;
  const float e = (s - (t - bp)) + (p - bp);
  s = t;
  lo += e + pe;
}

// Adjoint of pos_embed_bicubic_kernel in gather form: one thread per (source token, four d's) sums, rows then columns ascending, the
// output rows that tap its cell.  dtable [1 + gh*gw, D] -> dpos [1 + g*g, D]; the class row is copied.
__global__ __launch_bounds__(256) void pos_embed_bicubic_bwd_kernel(const float* __restrict__ dtable, float* __restrict__ dpos, int g, int gh,
                                                                    int gw, int D, float rscale_h, float rscale_w) {
  const int d4 = D / 4;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)(1 + g * g) * d4;
  if (idx >= total) return;
  const int tok = (int)(idx / d4), d = (int)(idx - (long long)tok * d4) * 4;
  if (tok == 0) {
    *reinterpret_cast<float4*>(dpos + d) = *reinterpret_cast<const float4*>(dtable + d);
    return;
  }
  const int sy = (tok - 1) / g, sx = (tok - 1) - sy * g;
  int y0, y1, x0, x1;
  stem_axis_range(sy, g, gh, rscale_h, y0, y1);
  stem_axis_range(sx, g, gw, rscale_w, x0, x1);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), lo = acc;
  for (int oy = y0; oy <= y1; ++oy) {
    const float wy = stem_axis_weight(oy, sy, g, rscale_h);
    if (wy == 0.f) continue;
    for (int ox = x0; ox <= x1; ++ox) {
      const float wx = stem_axis_weight(ox, sx, g, rscale_w);
      if (wx == 0.f) continue;
      const float c = wy * wx;
      const float4 v = *reinterpret_cast<const float4*>(dtable + (size_t)(1 + oy * gw + ox) * D + d);
      comp_fma(acc.x, lo.x, c, v.x); comp_fma(acc.y, lo.y, c, v.y); comp_fma(acc.z, lo.z, c, v.z); comp_fma(acc.w, lo.w, c, v.w);
    }
  }
  acc.x += lo.x; acc.y += lo.y; acc.z += lo.z; acc.w += lo.w;
  *reinterpret_cast<float4*>(dpos + (size_t)tok * D + d) = acc;
}

// The row split of the weight gradient: about 1024 workgroups (one resident wave of 64 x 64 tiles, the plan of the other weight
// gradients: gemm_f32.hip gemm_splitk_choice), slices of whole 16-row slabs, at most 64 of them and none empty.
struct StemPlan { int splits, chunk; };
static StemPlan stem_plan(long long R, int D, int K) {
  const long long tiles = (long long)((D + 63) / 64) * ((K + 63) / 64);
  long long s = (1024 + tiles - 1) / tiles;
  const long long slabs = (R + 15) / 16;
  if (s > slabs) s = slabs;
  if (s > 64) s = 64;
  if (s < 1) s = 1;
  const long long chunk = ((R + s - 1) / s + 15) / 16 * 16;
  return StemPlan{(int)((R + chunk - 1) / chunk), (int)chunk};
}
static size_t stem_table_floats(int n, int D) { return ((size_t)(n + 1) * D + 3) / 4 * 4; }

// nullptr when the shape is taken, else the rule it breaks
static const char* stem_shape_rule(int F, int C, int H, int W, int P, int D) {
  if (F <= 0 || C <= 0 || H <= 0 || W <= 0 || P <= 0 || D <= 0) return "F, C, H, W, P, D must be positive";
  if (P % 4 != 0 || W % 4 != 0) return "need P % 4 == 0 and W % 4 == 0 (a patch row is read as 16-byte pieces)";
  if (H % P != 0 || W % P != 0) return "H, W must be multiples of the patch size";
  if (D % 4 != 0) return "need D % 4 == 0";
  const long long n = (long long)(H / P) * (W / P), K = (long long)C * P * P;
  if (n >= (1ll << 20)) return "at most 2^20 - 1 patches per frame";
  if ((long long)F * (n + 1) * D >= (1ll << 31) || K * D >= (1ll << 31) || (long long)F * n >= (1ll << 31)) return "F (n + 1) D, F n and C P P D must stay below 2^31";
  return nullptr;
}

}  // namespace tt

using namespace tt;

extern "C" int tt_patch_embed_bwd_shape_ok(int F, int C, int H, int W, int P, int D) { return stem_shape_rule(F, C, H, W, P, D) == nullptr; }

extern "C" size_t tt_patch_embed_bwd_workspace_bytes(int F, int C, int H, int W, int P, int D) {
  if (stem_shape_rule(F, C, H, W, P, D)) return 0;
  const int n = (H / P) * (W / P), K = C * P * P;
  const StemPlan pl = stem_plan((long long)F * n, D, K);
  // the position-table gradient (dbias is folded from it also when the caller does not ask for dtable), then the partial tiles
  return (stem_table_floats(n, D) + (pl.splits > 1 ? (size_t)pl.splits * D * K : 0)) * sizeof(float);
}

extern "C" int tt_patch_embed_bwd(const float* dtok, const float* img, const int32_t* frame_map, float* dw, float* dbias, float* dcls,
                                  float* dtable, int F, int C, int H, int W, int P, int D, void* workspace, size_t workspace_bytes,
                                  tt_stream_t stream) {
  const char* rule = stem_shape_rule(F, C, H, W, P, D);
  TT_REQUIRE(rule == nullptr, "patch_embed_bwd: %s (got F=%d C=%d H=%d W=%d P=%d D=%d)", rule ? rule : "", F, C, H, W, P, D);
  TT_REQUIRE(dtok && aligned16(dtok), "patch_embed_bwd: dtok must be a 16-byte aligned device pointer");
  TT_REQUIRE(!dw || (img && aligned16(img) && aligned16(dw)), "patch_embed_bwd: the weight gradient needs img, and img / dw 16-byte aligned");
  TT_REQUIRE(aligned16(dbias) && aligned16(dcls) && aligned16(dtable), "patch_embed_bwd: dbias, dcls and dtable must be 16-byte aligned");
  const int gw = W / P, n = gw * (H / P), K = C * P * P;
  const StemPlan pl = stem_plan((long long)F * n, D, K);
  const bool need_ws = (dbias && !dtable) || (dw && pl.splits > 1);
  TT_REQUIRE(!need_ws || (workspace && aligned16(workspace) && workspace_bytes >= tt_patch_embed_bwd_workspace_bytes(F, C, H, W, P, D)),
             "patch_embed_bwd: workspace too small (need tt_patch_embed_bwd_workspace_bytes = %zu bytes, 16-byte aligned; got %zu)",
             tt_patch_embed_bwd_workspace_bytes(F, C, H, W, P, D), workspace_bytes);
  hipStream_t s = as_stream(stream);
  float* table = dtable ? dtable : (dbias ? static_cast<float*>(workspace) : nullptr);
  float* partial = (dw && pl.splits > 1) ? static_cast<float*>(workspace) + stem_table_floats(n, D) : nullptr;
  if (table || dcls) {
    const long long total4 = (long long)(n + 1) * (D / 4);
    // dcls alone: only the class row's threads are launched
    const long long count4 = table ? total4 : D / 4;
    hipLaunchKernelGGL(stem_table_kernel, dim3((unsigned)((count4 + 255) / 256)), dim3(256), 0, s, dtok, table, dcls, F, count4, total4, D / 4);
    TT_CHECK_LAUNCH("patch_embed_bwd.table");
  }
  if (dw) {
    StemArgs g{dtok, img, frame_map, partial ? partial : dw, F, C, H, W, P, D, K, gw, n, F * n, pl.chunk};
    hipLaunchKernelGGL(stem_wgrad_kernel, dim3(((D + 63) / 64) * ((K + 63) / 64), 1, pl.splits), dim3(256), 0, s, g);
    TT_CHECK_LAUNCH("patch_embed_bwd.wgrad");
  }
  if (partial || dbias) {
    const long long n4 = (long long)D * K / 4;
    long long blocks = partial ? (n4 + 255) / 256 : 0;
    if (blocks > 1024) blocks = 1024;
    const int bias_blocks = dbias ? (D + 63) / 64 : 0;
    hipLaunchKernelGGL(stem_fold_kernel, dim3((unsigned)blocks + bias_blocks), dim3(256), 0, s, partial, dw, n4, pl.splits, (int)blocks,
                       table ? table + D : nullptr, dbias, n, D);
    TT_CHECK_LAUNCH("patch_embed_bwd.fold");
  }
  return TT_OK;
}

extern "C" int tt_pos_embed_interpolate_bwd(const float* dtable, float* dpos, int g, int gh, int gw, int D, float scale_h, float scale_w,
                                            tt_stream_t stream) {
  TT_REQUIRE(dtable && dpos && g > 0 && gh > 0 && gw > 0, "pos_embed_interpolate_bwd: bad arguments");
  TT_REQUIRE(D > 0 && D % 4 == 0 && aligned16(dtable) && aligned16(dpos), "pos_embed_interpolate_bwd: D must be a multiple of 4, buffers 16-byte aligned");
  TT_REQUIRE(scale_h > 0.f && scale_w > 0.f, "pos_embed_interpolate_bwd: scale factors must be positive");
  const long long total = (long long)(1 + g * g) * (D / 4);
  hipLaunchKernelGGL(pos_embed_bicubic_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), dtable, dpos, g, gh, gw,
                     D, 1.0f / scale_h, 1.0f / scale_w);
  TT_CHECK_LAUNCH("pos_embed_interpolate_bwd");
  return TT_OK;
}
