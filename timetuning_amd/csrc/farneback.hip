// Dense Farneback optical flow and the nearest-neighbour label remap: the optical-flow baseline of the reference's
// label-propagation evaluation (mask_propagation.py:265-346, :803-815), i.e. cv2.calcOpticalFlowFarneback(prev, next, None, pyr_scale,
// levels, winsize, iterations, poly_n, poly_sigma, 0) for every (prev, next) pair of a batch, then cv2.remap(INTER_NEAREST).
//
// Stages, each ONE launch over the whole batch (frames F or pairs P), level by level from the coarsest:
//   fb_vblur         gray u8 [F, H, W] -> fp32 [F, H, W]: the vertical pass of level k's GaussianBlur (BORDER_REFLECT_101)
//   fb_hblur_resize  -> level image [F, h_k, w_k]: the horizontal pass, fused with the INTER_LINEAR resize (each output reads the 2 x 2
//                    blurred source pixels it interpolates; level 0 is the same size, so a plain copy of the blurred pixel)
//   fb_poly_v/_h     -> R [F, h_k, w_k, 5] (FarnebackPolyExp: vertical pass fp32, horizontal fp64, borders replicated).  R of a frame is
//                    computed once per level and read by both pairs that contain it.
//   fb_init_level    per pair and pixel: the flow of the coarser level resized in (x 1 / pyr_scale; zero at the coarsest level), then
//                    the matrices M [P, h_k, w_k, 5] of FarnebackUpdateMatrices
//   fb_box_v         M -> vertical box sums (winsize rows, replicated borders, fp64 sums stored fp32)
//   fb_box_h_solve   horizontal box sums (fp64), the 2 x 2 solve -> flow, and - except after the last iteration - the new M of the
//                    pixel (it reads the pixel's own flow only, so the update fuses into the solve: the Jacobi form, which is what
//                    OpenCV's row-lagged update inside its running sum amounts to)
// The separable passes read global memory directly (each row of a stencil is reused from L2 / the L1 of the CU); no float atomics
// anywhere, so two calls give the same bits, and a pair's flow does not depend on which other pairs share the launch.
//
// tt_remap_nearest_labels: one launch per chain step over N maps; the map is coords + scale * flow in fp32 with separate roundings
// (numpy's float32 arithmetic), rounded half to even and saturated to int16 (saturate_cast<short>), constant-0 border.
#include <cmath>
#include <algorithm>
#include <cstring>

#include "common.hpp"

namespace tt {

constexpr int FB_THREADS = 256;
constexpr int FB_MAX_BLUR_R = 127;    // GaussianBlur half-width (ksize <= 255): sigma up to ~25, i.e. frames up to ~3 400 px at scale 0.5
constexpr int FB_MAX_POLY_N = 7;      // poly_n 5 or 7: taps x = -poly_n..poly_n, as FarnebackPolyExp(src, dst, n = poly_n, sigma)
constexpr int FB_MAX_WIN = 127;       // winsize
constexpr int FB_MAX_LEVELS = 64;
constexpr int FB_MIN_SIZE = 32;

struct FbBlurTaps { int r; float k[FB_MAX_BLUR_R + 1]; };                      // k[|i|], i = -r..r
struct FbPolyTaps { int n; float g[FB_MAX_POLY_N + 1], xg[FB_MAX_POLY_N + 1], xxg[FB_MAX_POLY_N + 1]; double ig11, ig03, ig33, ig55; };

__device__ __forceinline__ int refl101(int p, int n) {
  if (n == 1) return 0;
  while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * n - 2 - p;
  return p;
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// INTER_LINEAR source index pair and weight along one axis (half-pixel centres, clamped)
__device__ __forceinline__ void lin_axis(int d, float scale, int n_src, int& s0, int& s1, float& w) {
  float f = (float)(((double)d + 0.5) * (double)scale - 0.5);
  int s = (int)floorf(f);
  w = f - (float)s;
  if (s < 0) { s = 0; w = 0.f; }
  if (s >= n_src - 1) { s = n_src - 1; w = 0.f; }
  s0 = s;
  s1 = s + 1 < n_src ? s + 1 : n_src - 1;
}

__global__ __launch_bounds__(FB_THREADS) void fb_gray_u8(const float* __restrict__ clip, uint8_t* __restrict__ gray, long long n_pix, long long HW) {
  const long long i = (long long)blockIdx.x * FB_THREADS + threadIdx.x;
  if (i >= n_pix) return;
  const long long f = i / HW, p = i - f * HW;
  const float* c = clip + f * 3 * HW + p;
  int v[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) v[ch] = (int)((long long)truncf(__fmul_rn(c[ch * HW], 255.f)) & 255);   // torch's CPU uint8 cast
  gray[i] = (uint8_t)((v[0] * 4899 + v[1] * 9617 + v[2] * 1868 + 8192) >> 14);                          // BGR2GRAY of RGB2BGR
}

__global__ __launch_bounds__(FB_THREADS) void fb_vblur(const uint8_t* __restrict__ gray, float* __restrict__ out, int F, int H, int W,
                                                       FbBlurTaps t) {
  const long long i = (long long)blockIdx.x * FB_THREADS + threadIdx.x;
  const long long HW = (long long)H * W;
  if (i >= HW * F) return;
  const long long f = i / HW;
  const int p = (int)(i - f * HW), y = p / W, x = p - y * W;
  const uint8_t* g = gray + f * HW + x;
  float s = 0.f;
  for (int d = -t.r; d <= t.r; ++d) s = fmaf(t.k[d < 0 ? -d : d], (float)g[(long long)refl101(y + d, H) * W], s);
  out[i] = s;
}

__device__ __forceinline__ float hconv(const float* row, int x, int W, const FbBlurTaps& t) {
  float s = 0.f;
  for (int d = -t.r; d <= t.r; ++d) s = fmaf(t.k[d < 0 ? -d : d], row[refl101(x + d, W)], s);
  return s;
}

__global__ __launch_bounds__(FB_THREADS) void fb_hblur_resize(const float* __restrict__ vb, float* __restrict__ img, int F, int H, int W,
                                                              int h, int w, float sy, float sx, FbBlurTaps t) {
  const long long i = (long long)blockIdx.x * FB_THREADS + threadIdx.x;
  const long long hw = (long long)h * w;
  if (i >= hw * F) return;
  const long long f = i / hw;
  const int p = (int)(i - f * hw), y = p / w, x = p - y * w;
  const float* src = vb + f * H * (long long)W;
  if (h == H && w == W) {                                   // resize to the same size is a copy
    img[i] = hconv(src + (long long)y * W, x, W, t);
    return;
  }
  int y0, y1, x0, x1;
  float wy, wx;
  lin_axis(y, sy, H, y0, y1, wy);
  lin_axis(x, sx, W, x0, x1, wx);
  const float* r0 = src + (long long)y0 * W;
  const float* r1 = src + (long long)y1 * W;
  const float top = hconv(r0, x0, W, t) * (1.f - wx) + hconv(r0, x1, W, t) * wx;
  const float bot = hconv(r1, x0, W, t) * (1.f - wx) + hconv(r1, x1, W, t) * wx;
  img[i] = top * (1.f - wy) + bot * wy;
}

__global__ __launch_bounds__(FB_THREADS) void fb_poly_v(const float* __restrict__ img, float* __restrict__ v3, int F, int h, int w,
                                                        FbPolyTaps t) {
  const long long i = (long long)blockIdx.x * FB_THREADS + threadIdx.x;
  const long long hw = (long long)h * w;
  if (i >= hw * F) return;
  const long long f = i / hw;
  const int p = (int)(i - f * hw), y = p / w, x = p - y * w;
  const float* s = img + f * hw + x;
  float r0 = s[(long long)y * w] * t.g[0], r1 = 0.f, r2 = 0.f;
  for (int k = 1; k <= t.n; ++k) {
    const float a = s[(long long)max(y - k, 0) * w], b = s[(long long)min(y + k, h - 1) * w];
    const float sum = a + b;
    r0 += t.g[k] * sum;
    r1 += t.xg[k] * (b - a);
    r2 += t.xxg[k] * sum;
  }
  float* o = v3 + i * 3;
  o[0] = r0; o[1] = r1; o[2] = r2;
}

__global__ __launch_bounds__(FB_THREADS) void fb_poly_h(const float* __restrict__ v3, float* __restrict__ R, int F, int h, int w,
                                                        FbPolyTaps t) {
  const long long i = (long long)blockIdx.x * FB_THREADS + threadIdx.x;
  const long long hw = (long long)h * w;
  if (i >= hw * F) return;
  const long long f = i / hw;
  const int p = (int)(i - f * hw), y = p / w, x = p - y * w;
  const float* row = v3 + (f * hw + (long long)y * w) * 3;
  const double g0 = t.g[0];
  double b1 = row[x * 3] * g0, b2 = 0, b3 = row[x * 3 + 1] * g0, b4 = 0, b5 = row[x * 3 + 2] * g0, b6 = 0;
  for (int k = 1; k <= t.n; ++k) {
    const float* L = row + max(x - k, 0) * 3;
    const float* Rr = row + min(x + k, w - 1) * 3;
    const double tg = (double)Rr[0] + (double)L[0];
    const double gk = t.g[k], xgk = t.xg[k], xxgk = t.xxg[k];
    b1 += tg * gk;
    b4 += tg * xxgk;
    b2 += ((double)Rr[0] - (double)L[0]) * xgk;
    b3 += ((double)Rr[1] + (double)L[1]) * gk;
    b6 += ((double)Rr[1] - (double)L[1]) * xgk;
    b5 += ((double)Rr[2] + (double)L[2]) * gk;
  }
  float* o = R + i * 5;
  o[0] = (float)(b3 * t.ig11);
  o[1] = (float)(b2 * t.ig11);
  o[2] = (float)(b1 * t.ig03 + b5 * t.ig33);
  o[3] = (float)(b1 * t.ig03 + b4 * t.ig33);
  o[4] = (float)(b6 * t.ig55);
}

__device__ __forceinline__ float border_w(int i) {
  return i == 0 || i == 1 ? 0.14f : 0.4472f;
}

// FarnebackUpdateMatrices at one pixel: R0 / R1 the pair's expansions [h, w, 5], (dx, dy) the pixel's flow
__device__ __forceinline__ void update_matrices(const float* __restrict__ R0, const float* __restrict__ R1, int h, int w, int y, int x,
                                                float dx, float dy, float* __restrict__ M) {
  float fx = (float)x + dx, fy = (float)y + dy;
  const float fx1 = floorf(fx), fy1 = floorf(fy);
  const float* r0 = R0 + ((long long)y * w + x) * 5;
  float r2, r3, r4, r5, r6;
  // the float -> int conversion is taken only where the floor is in range (a NaN or a huge flow counts as outside, as OpenCV's
  // unsigned compare of cvFloor does)
  if (fx1 >= 0.f && fx1 < (float)(w - 1) && fy1 >= 0.f && fy1 < (float)(h - 1)) {
    const int x1 = (int)fx1, y1 = (int)fy1;
    fx -= fx1; fy -= fy1;
    const float a00 = (1.f - fx) * (1.f - fy), a01 = fx * (1.f - fy), a10 = (1.f - fx) * fy, a11 = fx * fy;
    const float* p = R1 + ((long long)y1 * w + x1) * 5;
    const float* q = p + (long long)w * 5;
    float r[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) r[c] = a00 * p[c] + a01 * p[5 + c] + a10 * q[c] + a11 * q[5 + c];
    r2 = r[0]; r3 = r[1];
    r4 = (r0[2] + r[2]) * 0.5f;
    r5 = (r0[3] + r[3]) * 0.5f;
    r6 = (r0[4] + r[4]) * 0.25f;
  } else {
    r2 = r3 = 0.f;
    r4 = r0[2];
    r5 = r0[3];
    r6 = r0[4] * 0.5f;
  }
  r2 = (r0[0] - r2) * 0.5f;
  r3 = (r0[1] - r3) * 0.5f;
  r2 += r4 * dy + r6 * dx;
  r3 += r6 * dy + r5 * dx;
  if (x < 5 || x >= w - 5 || y < 5 || y >= h - 5) {
    const float s = (x < 5 ? border_w(x) : 1.f) * (x >= w - 5 ? border_w(w - x - 1) : 1.f) * (y < 5 ? border_w(y) : 1.f) *
                    (y >= h - 5 ? border_w(h - y - 1) : 1.f);
    r2 *= s; r3 *= s; r4 *= s; r5 *= s; r6 *= s;
  }
  M[0] = r4 * r4 + r6 * r6;
  M[1] = (r4 + r5) * r6;
  M[2] = r5 * r5 + r6 * r6;
  M[3] = r4 * r2 + r6 * r3;
  M[4] = r6 * r2 + r5 * r3;
}

// the pair's two frames, or false (an index outside [0, F): the pair's flow is NaN, nothing is read)
__device__ __forceinline__ bool pair_frames(const int32_t* __restrict__ pairs, int pair, int F, int& a, int& b) {
  a = pairs[2 * pair];
  b = pairs[2 * pair + 1];
  return (unsigned)a < (unsigned)F && (unsigned)b < (unsigned)F;
}

__global__ __launch_bounds__(FB_THREADS) void fb_init_level(const float* __restrict__ R, const int32_t* __restrict__ pairs,
                                                            const float* __restrict__ coarse, float* __restrict__ flow, float* __restrict__ M,
                                                            int F, int P, int h, int w, int hc, int wc, float sy, float sx, float up) {
  const long long i = (long long)blockIdx.x * FB_THREADS + threadIdx.x;
  const long long hw = (long long)h * w;
  if (i >= hw * P) return;
  const int pair = (int)(i / hw);
  const int p = (int)(i - pair * hw), y = p / w, x = p - y * w;
  int a, b;
  if (!pair_frames(pairs, pair, F, a, b)) {
    flow[i * 2] = flow[i * 2 + 1] = __builtin_nanf("");
#pragma unroll
    for (int c = 0; c < 5; ++c) M[i * 5 + c] = 0.f;
    return;
  }
  float dx = 0.f, dy = 0.f;
  if (coarse) {
    const float* cf = coarse + (long long)pair * hc * wc * 2;
    float vx, vy;
    if (hc == h && wc == w) {
      vx = cf[(long long)p * 2]; vy = cf[(long long)p * 2 + 1];
    } else {
      int y0, y1, x0, x1;
      float wy, wx;
      lin_axis(y, sy, hc, y0, y1, wy);
      lin_axis(x, sx, wc, x0, x1, wx);
      const float* q00 = cf + ((long long)y0 * wc + x0) * 2;
      const float* q01 = cf + ((long long)y0 * wc + x1) * 2;
      const float* q10 = cf + ((long long)y1 * wc + x0) * 2;
      const float* q11 = cf + ((long long)y1 * wc + x1) * 2;
      vx = (q00[0] * (1.f - wx) + q01[0] * wx) * (1.f - wy) + (q10[0] * (1.f - wx) + q11[0] * wx) * wy;
      vy = (q00[1] * (1.f - wx) + q01[1] * wx) * (1.f - wy) + (q10[1] * (1.f - wx) + q11[1] * wx) * wy;
    }
    dx = vx * up; dy = vy * up;
  }
  flow[i * 2] = dx;
  flow[i * 2 + 1] = dy;
  update_matrices(R + (long long)a * hw * 5, R + (long long)b * hw * 5, h, w, y, x, dx, dy, M + i * 5);
}

__global__ __launch_bounds__(FB_THREADS) void fb_box_v(const float* __restrict__ M, float* __restrict__ Mv, int P, int h, int w, int m) {
  const long long i = (long long)blockIdx.x * FB_THREADS + threadIdx.x;
  const long long hw = (long long)h * w;
  if (i >= hw * P) return;
  const long long pair = i / hw;
  const int p = (int)(i - pair * hw), y = p / w, x = p - y * w;
  const float* col = M + (pair * hw + x) * 5;
  double s[5] = {0, 0, 0, 0, 0};
  if (m == 0) {                                             // OpenCV's running-sum start for winsize 1: row 0 plus row y
#pragma unroll
    for (int c = 0; c < 5; ++c) s[c] = (double)col[c] + (double)col[(long long)y * w * 5 + c];
  } else {
    for (int d = -m; d <= m; ++d) {
      const float* q = col + (long long)clampi(y + d, 0, h - 1) * w * 5;
#pragma unroll
      for (int c = 0; c < 5; ++c) s[c] += q[c];
    }
  }
#pragma unroll
  for (int c = 0; c < 5; ++c) Mv[i * 5 + c] = (float)s[c];
}

__global__ __launch_bounds__(FB_THREADS) void fb_box_h_solve(const float* __restrict__ Mv, const float* __restrict__ R,
                                                             const int32_t* __restrict__ pairs, float* __restrict__ flow, float* __restrict__ M,
                                                             int F, int P, int h, int w, int m, double scale) {
  const long long i = (long long)blockIdx.x * FB_THREADS + threadIdx.x;
  const long long hw = (long long)h * w;
  if (i >= hw * P) return;
  const int pair = (int)(i / hw);
  const int p = (int)(i - pair * hw), y = p / w, x = p - y * w;
  int a, b;
  if (!pair_frames(pairs, pair, F, a, b)) return;           // fb_init_level wrote NaN
  const float* row = Mv + ((long long)pair * hw + (long long)y * w) * 5;
  double s[5] = {0, 0, 0, 0, 0};
  if (m == 0) {
#pragma unroll
    for (int c = 0; c < 5; ++c) s[c] = (double)row[c] + (double)row[x * 5 + c];
  } else {
    for (int d = -m; d <= m; ++d) {
      const float* q = row + clampi(x + d, 0, w - 1) * 5;
#pragma unroll
      for (int c = 0; c < 5; ++c) s[c] += q[c];
    }
  }
  const double g11 = s[0] * scale, g12 = s[1] * scale, g22 = s[2] * scale, h1 = s[3] * scale, h2 = s[4] * scale;
  const double idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3);
  const float dx = (float)((g11 * h2 - g12 * h1) * idet), dy = (float)((g22 * h1 - g12 * h2) * idet);
  flow[i * 2] = dx;
  flow[i * 2 + 1] = dy;
  if (M) update_matrices(R + (long long)a * hw * 5, R + (long long)b * hw * 5, h, w, y, x, dx, dy, M + i * 5);
}

template <typename T>
__global__ __launch_bounds__(FB_THREADS) void fb_remap_nearest(const T* __restrict__ src, long long src_stride, const float* __restrict__ flow,
                                                               long long flow_stride, T* __restrict__ dst, long long dst_stride, int N, int H,
                                                               int W, float scale) {
  const long long i = (long long)blockIdx.x * FB_THREADS + threadIdx.x;
  const long long HW = (long long)H * W;
  if (i >= HW * N) return;
  const long long n = i / HW;
  const int p = (int)(i - n * HW), y = p / W, x = p - y * W;
  const float* fl = flow + n * flow_stride + (long long)p * 2;
  const float mx = __fadd_rn((float)x, __fmul_rn(scale, fl[0]));
  const float my = __fadd_rn((float)y, __fmul_rn(scale, fl[1]));
  // saturate_cast<short>(cvRound(v)): half to even, clamped to int16; a NaN becomes INT_MIN -> -32768 (outside)
  const float rx = rintf(mx), ry = rintf(my);
  const int sx = rx != rx ? -32768 : (int)fminf(fmaxf(rx, -32768.f), 32767.f);
  const int sy = ry != ry ? -32768 : (int)fminf(fmaxf(ry, -32768.f), 32767.f);
  T v = 0;
  if ((unsigned)sx < (unsigned)W && (unsigned)sy < (unsigned)H) v = src[n * src_stride + (long long)sy * W + sx];
  dst[n * dst_stride + p] = v;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------

static inline unsigned fb_blocks(long long n) { return (unsigned)((n + FB_THREADS - 1) / FB_THREADS); }

static int fb_plan(int H, int W, double pyr_scale, int levels, int* sizes /* 2 (levels + 1) */) {
  double scale = 1.0;
  int k = 0;
  for (; k < levels; ++k) {
    scale *= pyr_scale;
    if (W * scale < FB_MIN_SIZE || H * scale < FB_MIN_SIZE) break;
  }
  if (sizes) {
    double s = 1.0;
    for (int i = 0; i <= k; ++i) {
      sizes[2 * i] = (int)std::nearbyint(H * s);
      sizes[2 * i + 1] = (int)std::nearbyint(W * s);
      s *= pyr_scale;
    }
  }
  return k;
}

static bool fb_params_ok(int H, int W, double pyr_scale, int levels) {
  return H > 0 && W > 0 && pyr_scale > 0.0 && pyr_scale < 1.0 && levels >= 1 && levels <= FB_MAX_LEVELS;
}

static size_t fb_al(size_t b) { return (b + 255) & ~(size_t)255; }

struct FbLayout { size_t vb, img, v3, R, M, Mv, fa, fb, total; };

static FbLayout fb_layout(int F, int P, int H, int W, int L, const int* sizes) {
  const size_t HW = (size_t)H * W;
  const size_t h1w1 = L >= 1 ? (size_t)sizes[2] * sizes[3] : 0;
  FbLayout l;
  size_t o = 0;
  l.vb = o;  o += fb_al(4 * HW * F);
  l.img = o; o += fb_al(4 * HW * F);
  l.v3 = o;  o += fb_al(12 * HW * F);
  l.R = o;   o += fb_al(20 * HW * F);
  l.M = o;   o += fb_al(20 * HW * P);
  l.Mv = o;  o += fb_al(20 * HW * P);
  l.fa = o;  o += fb_al(8 * h1w1 * P);
  l.fb = o;  o += fb_al(8 * h1w1 * P);
  l.total = o;
  return l;
}

static FbBlurTaps fb_blur_taps(double pyr_scale, int k) {
  double s = 1.0;
  for (int i = 0; i < k; ++i) s *= pyr_scale;
  const double sigma = (1.0 / s - 1.0) * 0.5;
  const int ksize = std::max((int)std::nearbyint(sigma * 5) | 1, 3);
  FbBlurTaps t;
  std::memset(&t, 0, sizeof(t));
  t.r = ksize / 2;
  if (t.r > FB_MAX_BLUR_R) { t.r = -1; return t; }
  if (sigma <= 0 && ksize == 3) {                      // getGaussianKernel's fixed 3-tap table
    t.k[0] = 0.5f; t.k[1] = 0.25f;
    return t;
  }
  double sum = 0, e[FB_MAX_BLUR_R + 1];
  for (int i = 0; i <= t.r; ++i) { e[i] = std::exp(-(double)i * i / (2 * sigma * sigma)); sum += i ? 2 * e[i] : e[i]; }
  for (int i = 0; i <= t.r; ++i) t.k[i] = (float)(e[i] / sum);
  return t;
}

static FbPolyTaps fb_poly_taps(int n, double sigma) {
  FbPolyTaps t;
  std::memset(&t, 0, sizeof(t));
  t.n = n;
  float g[2 * FB_MAX_POLY_N + 1];
  double s = 0;
  for (int x = -n; x <= n; ++x) { g[x + n] = (float)std::exp(-x * x / (2 * sigma * sigma)); s += g[x + n]; }
  s = 1.0 / s;
  for (int x = -n; x <= n; ++x) g[x + n] = (float)(g[x + n] * s);
  for (int x = 0; x <= n; ++x) { t.g[x] = g[x + n]; t.xg[x] = (float)(x * g[x + n]); t.xxg[x] = (float)(x * x * g[x + n]); }
  double G00 = 0, G11 = 0, G33 = 0, G55 = 0;
  for (int y = -n; y <= n; ++y)
    for (int x = -n; x <= n; ++x) {
      const double gg = (double)g[y + n] * g[x + n];
      G00 += gg; G11 += gg * x * x; G33 += gg * x * x * x * x; G55 += gg * x * x * y * y;
    }
  // the inverse of the 6 x 6 moment matrix: rows 1, 2 and 5 are diagonal, rows {0, 3, 4} form [[a, b, b], [b, c, d], [b, d, c]]
  const double D = G00 * (G33 + G55) - 2 * G11 * G11;
  t.ig11 = 1.0 / G11;
  t.ig03 = -G11 / D;
  t.ig33 = (G00 * G33 - G11 * G11) / ((G33 - G55) * D);
  t.ig55 = 1.0 / G55;
  return t;
}

}  // namespace tt

using namespace tt;

extern "C" {

int tt_farneback_plan(int H, int W, double pyr_scale, int levels, int* levels_out, int* sizes_out) {
  TT_REQUIRE(fb_params_ok(H, W, pyr_scale, levels), "tt_farneback_plan: H %d, W %d, pyr_scale %g, levels %d (0 < pyr_scale < 1, 1 <= levels "
             "<= %d)", H, W, pyr_scale, levels, FB_MAX_LEVELS);
  int sizes[2 * (FB_MAX_LEVELS + 1)];
  const int L = fb_plan(H, W, pyr_scale, levels, sizes);
  if (levels_out) *levels_out = L;
  if (sizes_out) std::memcpy(sizes_out, sizes, sizeof(int) * 2 * (L + 1));
  return TT_OK;
}

size_t tt_farneback_workspace_bytes(int F, int P, int H, int W, double pyr_scale, int levels) {
  if (F < 1 || P < 0 || !fb_params_ok(H, W, pyr_scale, levels)) return 0;
  int sizes[2 * (FB_MAX_LEVELS + 1)];
  const int L = fb_plan(H, W, pyr_scale, levels, sizes);
  return fb_layout(F, P, H, W, L, sizes).total;
}

int tt_flow_gray_u8(const float* clip, uint8_t* gray, int F, int H, int W, tt_stream_t stream) {
  TT_REQUIRE(F >= 0 && H > 0 && W > 0, "tt_flow_gray_u8: F %d, H %d, W %d", F, H, W);
  TT_REQUIRE(F == 0 || (clip && gray), "tt_flow_gray_u8: null pointer");
  const long long n = (long long)F * H * W;
  if (n == 0) return TT_OK;
  fb_gray_u8<<<fb_blocks(n), FB_THREADS, 0, as_stream(stream)>>>(clip, gray, n, (long long)H * W);
  TT_CHECK_LAUNCH("tt_flow_gray_u8");
  return TT_OK;
}

int tt_farneback_flow(const uint8_t* frames, int F, int H, int W, const int32_t* pairs, int P, double pyr_scale, int levels, int winsize,
                      int iterations, int poly_n, double poly_sigma, int flags, float* flow, void* workspace, size_t workspace_bytes,
                      tt_stream_t stream) {
  TT_REQUIRE(flags == 0, "tt_farneback_flow: flags %d (OPTFLOW_USE_INITIAL_FLOW and OPTFLOW_FARNEBACK_GAUSSIAN are not supported)", flags);
  TT_REQUIRE(F >= 1 && P >= 0 && fb_params_ok(H, W, pyr_scale, levels), "tt_farneback_flow: F %d, P %d, H %d, W %d, pyr_scale %g, levels %d",
             F, P, H, W, pyr_scale, levels);
  TT_REQUIRE(winsize >= 1 && winsize <= FB_MAX_WIN && iterations >= 1 && (poly_n == 5 || poly_n == 7) && poly_sigma > 0 &&
             std::isfinite(poly_sigma), "tt_farneback_flow: winsize %d (1..%d), iterations %d, poly_n %d (5 or 7), poly_sigma %g", winsize,
             FB_MAX_WIN, iterations, poly_n, poly_sigma);
  if (P == 0) return TT_OK;
  TT_REQUIRE(frames && pairs && flow && workspace, "tt_farneback_flow: null pointer");
  int sizes[2 * (FB_MAX_LEVELS + 1)];
  const int L = fb_plan(H, W, pyr_scale, levels, sizes);
  const FbLayout lay = fb_layout(F, P, H, W, L, sizes);
  TT_REQUIRE(workspace_bytes >= lay.total, "tt_farneback_flow: workspace %zu bytes < %zu", workspace_bytes, lay.total);
  FbBlurTaps taps[FB_MAX_LEVELS + 1];
  for (int k = 0; k <= L; ++k) {
    taps[k] = fb_blur_taps(pyr_scale, k);
    TT_REQUIRE(taps[k].r >= 0, "tt_farneback_flow: level %d's Gaussian exceeds %d taps (frame %d x %d too large for pyr_scale %g)", k,
               2 * FB_MAX_BLUR_R + 1, H, W, pyr_scale);
  }
  const FbPolyTaps pt = fb_poly_taps(poly_n, poly_sigma);
  char* ws = static_cast<char*>(workspace);
  float* vb = reinterpret_cast<float*>(ws + lay.vb);
  float* img = reinterpret_cast<float*>(ws + lay.img);
  float* v3 = reinterpret_cast<float*>(ws + lay.v3);
  float* R = reinterpret_cast<float*>(ws + lay.R);
  float* M = reinterpret_cast<float*>(ws + lay.M);
  float* Mv = reinterpret_cast<float*>(ws + lay.Mv);
  float* fbuf[2] = {reinterpret_cast<float*>(ws + lay.fa), reinterpret_cast<float*>(ws + lay.fb)};
  hipStream_t s = as_stream(stream);
  const int m = winsize / 2;
  const double box_scale = 1.0 / ((double)winsize * winsize);
  const float up = (float)(1.0 / pyr_scale);
  for (int k = L; k >= 0; --k) {
    const int h = sizes[2 * k], w = sizes[2 * k + 1];
    const long long nf = (long long)F * h * w, np = (long long)P * h * w;
    fb_vblur<<<fb_blocks((long long)F * H * W), FB_THREADS, 0, s>>>(frames, vb, F, H, W, taps[k]);
    fb_hblur_resize<<<fb_blocks(nf), FB_THREADS, 0, s>>>(vb, img, F, H, W, h, w, (float)((double)H / h), (float)((double)W / w), taps[k]);
    fb_poly_v<<<fb_blocks(nf), FB_THREADS, 0, s>>>(img, v3, F, h, w, pt);
    fb_poly_h<<<fb_blocks(nf), FB_THREADS, 0, s>>>(v3, R, F, h, w, pt);
    float* out = k == 0 ? flow : fbuf[k & 1];
    const float* coarse = k == L ? nullptr : fbuf[(k + 1) & 1];
    const int hc = k == L ? h : sizes[2 * (k + 1)], wc = k == L ? w : sizes[2 * (k + 1) + 1];
    fb_init_level<<<fb_blocks(np), FB_THREADS, 0, s>>>(R, pairs, coarse, out, M, F, P, h, w, hc, wc, (float)((double)hc / h),
                                                       (float)((double)wc / w), up);
    for (int it = 0; it < iterations; ++it) {
      fb_box_v<<<fb_blocks(np), FB_THREADS, 0, s>>>(M, Mv, P, h, w, m);
      fb_box_h_solve<<<fb_blocks(np), FB_THREADS, 0, s>>>(Mv, R, pairs, out, it < iterations - 1 ? M : nullptr, F, P, h, w, m, box_scale);
    }
  }
  TT_CHECK_LAUNCH("tt_farneback_flow");
  return TT_OK;
}

int tt_remap_nearest_labels(const void* first, const float* flows, void* out, int N, int steps, int H, int W, float scale, int label_bytes,
                            tt_stream_t stream) {
  TT_REQUIRE(N >= 0 && steps >= 0 && H > 0 && W > 0 && (label_bytes == 1 || label_bytes == 8),
             "tt_remap_nearest_labels: N %d, steps %d, H %d, W %d, label_bytes %d (1 = uint8, 8 = int64)", N, steps, H, W, label_bytes);
  if (N == 0 || steps == 0) return TT_OK;
  TT_REQUIRE(first && flows && out, "tt_remap_nearest_labels: null pointer");
  const long long HW = (long long)H * W;
  hipStream_t s = as_stream(stream);
  for (int st = 0; st < steps; ++st) {
    const long long src_off = st == 0 ? 0 : (st - 1) * HW, src_stride = st == 0 ? HW : steps * HW;
    const float* fl = flows + st * HW * 2;
    if (label_bytes == 1) {
      const uint8_t* src = st == 0 ? static_cast<const uint8_t*>(first) : static_cast<const uint8_t*>(out) + src_off;
      fb_remap_nearest<uint8_t><<<fb_blocks(N * HW), FB_THREADS, 0, s>>>(src, src_stride, fl, steps * HW * 2,
                                                                        static_cast<uint8_t*>(out) + st * HW, steps * HW, N, H, W, scale);
    } else {
      const int64_t* src = st == 0 ? static_cast<const int64_t*>(first) : static_cast<const int64_t*>(out) + src_off;
      fb_remap_nearest<int64_t><<<fb_blocks(N * HW), FB_THREADS, 0, s>>>(src, src_stride, fl, steps * HW * 2,
                                                                        static_cast<int64_t*>(out) + st * HW, steps * HW, N, H, W, scale);
    }
  }
  TT_CHECK_LAUNCH("tt_remap_nearest_labels");
  return TT_OK;
}

}  // extern "C"
