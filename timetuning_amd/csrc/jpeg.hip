// N21, device half: dequantisation, inverse DCT, chroma up-sampling and YCbCr -> RGB of a whole batch of baseline JPEG frames in two
// launches, bit-equal to libjpeg-turbo's defaults (the accurate integer IDCT "islow", "fancy" triangle-filter up-sampling, the 16-bit
// fixed-point colour tables) - what Pillow's Image.open decodes with.  The host half (jpeg_scan.cpp) has parsed the markers and undone
// the Huffman coding; the arithmetic rules are those of DESIGN.md N21, and tests/_jpeg_ref.py restates them in NumPy.
//
// The frames of one call may differ in size and sampling: a descriptor table (tt_jpeg_frame, one row per frame) says where each
// frame's coefficients, quantisation tables, reconstructed planes and RGB output lie.  The frames ride on gridDim.y as the segments of
// confusion.hip do - (frame, component) in the first launch, frame in the second - and gridDim.x covers the largest one; a workgroup
// past its own frame's work returns at once.  tt_jpeg_decode_batch checks every offset and extent of the HOST copy of the table against
// the buffer sizes it is given before it launches anything; the kernels trust the device copy.
//
// (a) jpeg_idct_kernel: 256 lanes = 32 blocks x 8 lanes.  Lane j of a block loads coefficient row j and table row j as one 16-byte vector
//     each, multiplies, and writes the products into the block's LDS tile.  The tile is int32 [8][9] (row stride 9 words, block stride
//     72): a wave's row writes (word b * 72 + j * 9 + k, lanes (b, j)) and its transposed column reads (b * 72 + r * 9 + c, lanes
//     (b, c)) both fall into 32 distinct banks per half-wave.  Lane c runs the column pass in registers and writes its column back; lane r
//     runs the row pass, adds 128, clamps and stores its 8 samples as one 8-byte vector into the component's plane, which is laid out at
//     the block-grid size (so its stride is a multiple of 8 and no store needs a bound).
// (b) jpeg_colour_kernel: a lane owns 4 pixels of TWO rows (2r, 2r + 1): with 2x2 sampling both rows come from chroma row r and its
//     neighbours r - 1 / r + 1, which are read once.  Chroma neighbours past the TRUE chroma size (ceil(W h / hmax), ceil(H v / vmax))
//     replicate the edge sample - never the block grid's padding - by clamping the index, which also yields libjpeg's first / last column
//     special cases.  Luma comes as one 4-byte load per row, RGB leaves as three 4-byte stores (12 contiguous bytes) where the address
//     allows, byte by byte at ragged edges and unaligned rows.
// Plain C++, vector loads and stores only; 32-bit integer arithmetic suffices for 8-bit baseline data.
#include "common.hpp"
#include "jpeg_huff.hpp"   // jh::grid: the block grid, stated once for the scan, the entropy kernels and these

namespace tt {

constexpr int JP_THREADS = 256;
constexpr int JP_BLOCKS_PER_WG = JP_THREADS / 8;
constexpr int JP_TILE_ROW = 9, JP_TILE = 8 * JP_TILE_ROW;   // words
constexpr int JP_MAX_FRAMES = 65535 / 3;                    // (frame, component) rides on gridDim.y
constexpr long long JP_MAX_DIM = 65535;                     // a JPEG frame's largest side
constexpr size_t JP_ALIGN = 256;

// One 1-D pass (Loeffler-Ligtenberg-Moschytz, CONST_BITS = 13), descaled by `shift` bits.
template <int SHIFT>
__device__ __forceinline__ void jp_pass(int (&x)[8]) {
  int z1 = (x[2] + x[6]) * 4433;
  const int t2 = z1 - x[6] * 15137;
  const int t3 = z1 + x[2] * 6270;
  const int t0 = (x[0] + x[4]) * 8192;
  const int t1 = (x[0] - x[4]) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int a0 = x[7], a1 = x[5], a2 = x[3], a3 = x[1];
  z1 = a0 + a3;
  int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const int z5 = (z3 + z4) * 9633;
  a0 *= 2446;
  a1 *= 16819;
  a2 *= 25172;
  a3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  a0 += z1 + z3;
  a1 += z2 + z4;
  a2 += z2 + z3;
  a3 += z1 + z4;
  constexpr int R = 1 << (SHIFT - 1);
  x[0] = (t10 + a3 + R) >> SHIFT;
  x[7] = (t10 - a3 + R) >> SHIFT;
  x[1] = (t11 + a2 + R) >> SHIFT;
  x[6] = (t11 - a2 + R) >> SHIFT;
  x[2] = (t12 + a1 + R) >> SHIFT;
  x[5] = (t12 - a1 + R) >> SHIFT;
  x[3] = (t13 + a0 + R) >> SHIFT;
  x[4] = (t13 - a0 + R) >> SHIFT;
}

__device__ __forceinline__ int jp_clamp(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ __launch_bounds__(JP_THREADS) void jpeg_idct_kernel(const int16_t* __restrict__ coeffs, const uint16_t* __restrict__ qtables,
                                                              const tt_jpeg_frame* __restrict__ table, uint8_t* __restrict__ planes) {
  __shared__ int tile[JP_BLOCKS_PER_WG * JP_TILE];
  const int frame = blockIdx.y / 3, comp = blockIdx.y % 3;
  const tt_jpeg_frame& f = table[frame];
  const jh::Grid g = jh::grid(f.H, f.W, (int)f.sampling, comp);
  const long long nblocks = g.rows * g.cols;
  if ((long long)blockIdx.x * JP_BLOCKS_PER_WG >= nblocks) return;   // uniform over the workgroup
  const int b = threadIdx.x >> 3, j = threadIdx.x & 7;
  const long long blk = (long long)blockIdx.x * JP_BLOCKS_PER_WG + b;
  const bool live = blk < nblocks;
  int* t = tile + b * JP_TILE;
  int x[8];
  if (live) {
    const uint4 cv = *reinterpret_cast<const uint4*>(coeffs + f.coeff_off[comp] + blk * 64 + j * 8);
    const uint4 qv = *reinterpret_cast<const uint4*>(qtables + f.qslot[comp] * 64 + j * 8);
    const unsigned cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      t[j * JP_TILE_ROW + 2 * k] = (int)(short)(cw[k] & 0xffffu) * (int)(qw[k] & 0xffffu);
      t[j * JP_TILE_ROW + 2 * k + 1] = (int)(short)(cw[k] >> 16) * (int)(qw[k] >> 16);
    }
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int r = 0; r < 8; ++r) x[r] = t[r * JP_TILE_ROW + j];
    jp_pass<11>(x);
#pragma unroll
    for (int r = 0; r < 8; ++r) t[r * JP_TILE_ROW + j] = x[r];
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = t[j * JP_TILE_ROW + k];
    jp_pass<18>(x);
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lo |= (unsigned)jp_clamp(x[k] + 128) << (8 * k);
      hi |= (unsigned)jp_clamp(x[k + 4] + 128) << (8 * k);
    }
    const long long by = blk / g.cols, bx = blk % g.cols;
    uint8_t* dst = planes + f.plane_off[comp] + (by * 8 + j) * (g.cols * 8) + bx * 8;
    *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
  }
}

constexpr int JP_FIX_R_CR = 91881;    // F(1.402), F(x) = int(x * 65536 + 0.5)
constexpr int JP_FIX_B_CB = 116130;   // F(1.772)
constexpr int JP_FIX_G_CB = 22554;    // F(0.34414)
constexpr int JP_FIX_G_CR = 46802;    // F(0.71414)

__device__ __forceinline__ long long jp_clampi(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the four up-sampled chroma samples of output columns x0 ... x0 + 3 of one output row.  p: the chroma plane, stride its row stride,
// dw x dh its TRUE size; r the chroma row, nbr the neighbour row of this output row (2x2 only)
__device__ __forceinline__ void jp_chroma4(const uint8_t* __restrict__ p, long long stride, long long dw, int sampling, long long r,
                                           long long nbr, long long x0, int (&out)[4]) {
  if (sampling == TT_JPEG_444) {
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = p[r * stride + jp_clampi(x0 + i, dw - 1)];
    return;
  }
  const long long c0 = x0 >> 1;   // x0 is a multiple of 4: chroma columns c0, c0 + 1 and their neighbours c0 - 1, c0 + 2
  int s[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long c = jp_clampi(c0 - 1 + i, dw - 1);
    const int v = p[r * stride + c];
    s[i] = sampling == TT_JPEG_420 ? 3 * v + (int)p[nbr * stride + c] : v;
  }
  if (sampling == TT_JPEG_420) {
    out[0] = (3 * s[1] + s[0] + 8) >> 4;
    out[1] = (3 * s[1] + s[2] + 7) >> 4;
    out[2] = (3 * s[2] + s[1] + 8) >> 4;
    out[3] = (3 * s[2] + s[3] + 7) >> 4;
  } else {
    out[0] = (3 * s[1] + s[0] + 1) >> 2;
    out[1] = (3 * s[1] + s[2] + 2) >> 2;
    out[2] = (3 * s[2] + s[1] + 1) >> 2;
    out[3] = (3 * s[2] + s[3] + 2) >> 2;
  }
}

__global__ __launch_bounds__(JP_THREADS) void jpeg_colour_kernel(const tt_jpeg_frame* __restrict__ table, const uint8_t* __restrict__ planes,
                                                                uint8_t* __restrict__ out) {
  const tt_jpeg_frame& f = table[blockIdx.y];
  const long long H = f.H, W = f.W;
  const int sampling = (int)f.sampling;
  const long long groups = (W + 3) >> 2, pairs = (H + 1) >> 1;
  const long long item = (long long)blockIdx.x * JP_THREADS + threadIdx.x;
  if (item >= groups * pairs) return;
  const long long r = item / groups, x0 = (item % groups) * 4;
  const jh::Grid gy = jh::grid(H, W, sampling, 0), gc = jh::grid(H, W, sampling, 1);
  const long long ystride = gy.cols * 8, cstride = gc.cols * 8;
  const int hmax = sampling == TT_JPEG_444 ? 1 : 2, vmax = sampling == TT_JPEG_420 ? 2 : 1;
  const long long dw = (W + hmax - 1) / hmax, dh = (H + vmax - 1) / vmax;
  const uint8_t* __restrict__ py = planes + f.plane_off[0];
  const uint8_t* __restrict__ pcb = planes + f.plane_off[1];
  const uint8_t* __restrict__ pcr = planes + f.plane_off[2];
  uint8_t* __restrict__ dst = out + f.out_off;
  const int valid = W - x0 >= 4 ? 4 : (int)(W - x0);
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const long long y = 2 * r + half;
    if (y >= H) break;
    const long long cr_row = vmax == 2 ? r : y;
    const long long nbr = jp_clampi(half ? cr_row + 1 : cr_row - 1, dh - 1);
    int cb[4], cr[4];
    jp_chroma4(pcb, cstride, dw, sampling, cr_row, nbr, x0, cb);
    jp_chroma4(pcr, cstride, dw, sampling, cr_row, nbr, x0, cr);
    const unsigned yv = *reinterpret_cast<const unsigned*>(py + y * ystride + x0);   // the plane is as wide as the block grid: x0 + 3 is inside
    uint8_t rgb[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int Y = (int)((yv >> (8 * i)) & 0xffu), b = cb[i] - 128, c = cr[i] - 128;
      rgb[3 * i] = (uint8_t)jp_clamp(Y + ((JP_FIX_R_CR * c + 32768) >> 16));
      rgb[3 * i + 1] = (uint8_t)jp_clamp(Y + ((-JP_FIX_G_CB * b - JP_FIX_G_CR * c + 32768) >> 16));
      rgb[3 * i + 2] = (uint8_t)jp_clamp(Y + ((JP_FIX_B_CB * b + 32768) >> 16));
    }
    uint8_t* o = dst + (y * W + x0) * 3;
    if (valid == 4 && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
      unsigned* o4 = reinterpret_cast<unsigned*>(o);
#pragma unroll
      for (int k = 0; k < 3; ++k)
        o4[k] = (unsigned)rgb[4 * k] | ((unsigned)rgb[4 * k + 1] << 8) | ((unsigned)rgb[4 * k + 2] << 16) | ((unsigned)rgb[4 * k + 3] << 24);
    } else {
      for (int k = 0; k < 3 * valid; ++k) o[k] = rgb[k];
    }
  }
}

// The bytes of the frames' planes: what the table's plane offsets must stay inside.  -1: a row of the table is not a frame.
static long long jp_plane_extent(const tt_jpeg_frame* table, int n_frames) {
  long long extent = 0;
  for (int i = 0; i < n_frames; ++i) {
    const tt_jpeg_frame& f = table[i];
    if (f.H < 1 || f.W < 1 || f.H > JP_MAX_DIM || f.W > JP_MAX_DIM || f.sampling < TT_JPEG_444 || f.sampling > TT_JPEG_420) return -1;
    for (int c = 0; c < 3; ++c) {
      const jh::Grid g = jh::grid(f.H, f.W, (int)f.sampling, c);
      if (f.plane_off[c] < 0 || f.plane_off[c] > (1ll << 46)) return -1;
      const long long end = f.plane_off[c] + g.rows * g.cols * 64;
      if (end > extent) extent = end;
    }
  }
  return extent;
}

}  // namespace tt

using namespace tt;

extern "C" size_t tt_jpeg_decode_batch_workspace_bytes(const tt_jpeg_frame* frame_table, int n_frames) {
  if (!frame_table || n_frames < 1) return 0;
  const long long extent = jp_plane_extent(frame_table, n_frames);
  return extent < 0 ? 0 : (size_t)((extent + (long long)JP_ALIGN - 1) / (long long)JP_ALIGN * (long long)JP_ALIGN);
}

extern "C" int tt_jpeg_decode_batch(const int16_t* coeffs, long long n_coeffs, const uint16_t* qtables, int n_qtables,
                                    const tt_jpeg_frame* frame_table, const tt_jpeg_frame* frame_table_dev, int n_frames, uint8_t* out,
                                    long long out_bytes, void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  TT_REQUIRE(coeffs && qtables && frame_table && frame_table_dev && out && workspace, "jpeg_decode_batch: null pointer");
  TT_REQUIRE(n_frames >= 1 && n_frames <= JP_MAX_FRAMES, "jpeg_decode_batch: %d frames: one call takes 1 ... %d", n_frames, JP_MAX_FRAMES);
  TT_REQUIRE(n_coeffs >= 0 && n_qtables >= 1 && out_bytes >= 0, "jpeg_decode_batch: negative buffer size");
  TT_REQUIRE(aligned16(coeffs) && aligned16(qtables) && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 &&
                 (reinterpret_cast<uintptr_t>(frame_table_dev) & 7u) == 0,
             "jpeg_decode_batch: coeffs and qtables must be 16-byte aligned, the workspace and the table 8-byte aligned");
  long long max_blocks = 0, max_items = 0;
  for (int i = 0; i < n_frames; ++i) {
    const tt_jpeg_frame& f = frame_table[i];
    TT_REQUIRE(f.H >= 1 && f.W >= 1 && f.H <= JP_MAX_DIM && f.W <= JP_MAX_DIM, "jpeg_decode_batch: frame %d is %lld x %lld", i, (long long)f.H,
               (long long)f.W);
    TT_REQUIRE(f.sampling >= TT_JPEG_444 && f.sampling <= TT_JPEG_420, "jpeg_decode_batch: frame %d has sampling code %lld", i, (long long)f.sampling);
    for (int c = 0; c < 3; ++c) {
      const jh::Grid g = jh::grid(f.H, f.W, (int)f.sampling, c);
      const long long nblocks = g.rows * g.cols;
      TT_REQUIRE(f.coeff_off[c] >= 0 && f.coeff_off[c] % 8 == 0 && f.coeff_off[c] <= n_coeffs && nblocks * 64 <= n_coeffs - f.coeff_off[c],
                 "jpeg_decode_batch: frame %d component %d: %lld coefficients at offset %lld do not lie 16-byte aligned inside the %lld given", i, c,
                 nblocks * 64, (long long)f.coeff_off[c], n_coeffs);
      TT_REQUIRE(f.qslot[c] >= 0 && f.qslot[c] < n_qtables, "jpeg_decode_batch: frame %d component %d: table slot %lld of %d", i, c,
                 (long long)f.qslot[c], n_qtables);
      TT_REQUIRE(f.plane_off[c] >= 0 && f.plane_off[c] % 8 == 0 && (unsigned long long)f.plane_off[c] <= workspace_bytes &&
                     (unsigned long long)(nblocks * 64) <= workspace_bytes - (unsigned long long)f.plane_off[c],
                 "jpeg_decode_batch: frame %d component %d: a plane of %lld bytes at offset %lld does not lie 8-byte aligned inside the workspace of %zu", i,
                 c, nblocks * 64, (long long)f.plane_off[c], workspace_bytes);
      if (nblocks > max_blocks) max_blocks = nblocks;
    }
    const long long rgb = f.H * f.W * 3;
    TT_REQUIRE(f.out_off >= 0 && f.out_off <= out_bytes && rgb <= out_bytes - f.out_off,
               "jpeg_decode_batch: frame %d: %lld output bytes at offset %lld do not lie inside the %lld given", i, rgb, (long long)f.out_off, out_bytes);
    const long long items = ((f.W + 3) / 4) * ((f.H + 1) / 2);
    if (items > max_items) max_items = items;
  }
  hipStream_t s = as_stream(stream);
  const dim3 grid_a((unsigned)((max_blocks + JP_BLOCKS_PER_WG - 1) / JP_BLOCKS_PER_WG), (unsigned)(3 * n_frames));
  hipLaunchKernelGGL(jpeg_idct_kernel, grid_a, dim3(JP_THREADS), 0, s, coeffs, qtables, frame_table_dev, static_cast<uint8_t*>(workspace));
  const dim3 grid_b((unsigned)((max_items + JP_THREADS - 1) / JP_THREADS), (unsigned)n_frames);
  hipLaunchKernelGGL(jpeg_colour_kernel, grid_b, dim3(JP_THREADS), 0, s, frame_table_dev, static_cast<const uint8_t*>(workspace), out);
  TT_CHECK_LAUNCH("jpeg_decode_batch");
  return TT_OK;
}
