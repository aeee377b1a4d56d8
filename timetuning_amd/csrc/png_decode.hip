// N26: the annotation PNGs of a batch decoded on the device - inflate, Adler-32, row filters and unpacking in ONE launch; the steps, the
// scheme of the inflate and its bounds are in png_inflate.hpp (which tt_png_decode_host in png_scan.cpp runs sequentially on the host).
//
// One workgroup of ONE wave (64 lanes) owns one file from its first bit to its last pixel: no workgroup waits on another, no flag, no
// spin, and a barrier of a one-wave workgroup costs a wait on the wave's own memory counters.  Phases:
//   inflate   pz::inflate with the 64-lane context into the file's slice of the workspace, H rows of 1 + row_bytes bytes; back-references
//             read the slice from global memory behind a barrier (the bytes were stored by other lanes).  The symbol loop is uniform: all
//             lanes decode the same symbol, so the wave never diverges in it and nothing is broadcast.
//   filters   the filter bytes of all rows are checked first (a byte above 4: TT_PNG_EFILTER, no pixel written).
//   unfilter  a skewed wavefront over tiles of 64 rows x kTile row bytes staged in LDS: lane j owns row r0 + j and is one column behind
//             lane j - 1, so its `up` is what lane j - 1 left in the tile one step earlier, its `left` and `up-left` are registers.  All
//             five filters and any mix of them per row run through the one branch-free step pz::unfilter.  Row 0 of the tile is the
//             unfiltered row above the block: the last row of every block is stored back IN PLACE for it.  The tile rows are
//             kTile + 5 bytes apart, so the 64 lanes of a step fall into 64 different LDS banks.  A tile costs kTile + 63 steps.
//   unpack    the unfiltered tile is unpacked (1-, 2-, 4-bit: MSB first) and stored to the output with the lanes along the row.
// LDS: two code tables (3.3 KB), the code lengths, the Adler partial sums and the tile (65 x 261): under 21 KB.
#include "common.hpp"
#include "png_inflate.hpp"

namespace tt {

namespace {

constexpr int PD_T = pz::kLanes;
constexpr int kTile = 256, kTileStride = kTile + 5;   // (stride - 1) / 4 is odd: lane j of a step is in bank (j + const) mod 64

struct WaveCtx {
  static constexpr int NL = PD_T;
  int lane;
  __device__ void sync() { __syncthreads(); }
};

__global__ __launch_bounds__(PD_T) void png_decode_kernel(const uint8_t* __restrict__ streams, const tt_png_stream* __restrict__ table,
                                                         uint8_t* __restrict__ out, uint8_t* __restrict__ ws, int32_t* __restrict__ stats,
                                                         int32_t* __restrict__ status) {
  __shared__ pz::Work work;
  __shared__ uint8_t tile[65 * kTileStride];
  __shared__ int s_bad, s_filters;

  const int lane = (int)threadIdx.x;
  const tt_png_stream row = table[blockIdx.x];
  const long long H = row.H, W = row.W, rb = row.row_bytes, pitch = 1 + rb;
  const int depth = (int)row.depth;
  uint8_t* raw = ws + row.ws_off;
  uint8_t* pix = out + row.out_off;
  WaveCtx c{lane};
  pz::Stats st{};
  if (lane == 0) s_bad = s_filters = 0;
  int rc = pz::inflate(c, work, reinterpret_cast<const uint32_t*>(streams + row.stream_off), (uint64_t)row.stream_len, raw, (uint64_t)(H * pitch), st);
  __syncthreads();
  if (rc == 0) {
    int bad = 0, seen = 0;
    for (long long r = lane; r < H; r += PD_T) {
      const int ft = raw[r * pitch];
      if (ft > 4) bad = 1; else seen |= 1 << ft;
    }
    if (bad) atomicOr(&s_bad, 1);
    if (seen) atomicOr(&s_filters, seen);
    __syncthreads();
    if (s_bad) rc = TT_PNG_EFILTER;
    else st.filters = s_filters;   // (a refused file reports no filters, as the emulation)
  }
  if (rc == 0) {
    for (long long r0 = 0; r0 < H; r0 += PD_T) {
      const int rows = (int)(H - r0 < PD_T ? H - r0 : PD_T);
      const int ft = lane < rows ? raw[(r0 + lane) * pitch] : 0;
      uint8_t left = 0;
      for (long long c0 = 0; c0 < rb; c0 += kTile) {
        const int tw = (int)(rb - c0 < kTile ? rb - c0 : kTile);
        // row 0 of the tile: the unfiltered row above the block (zeros above the image); rows 1 .. rows: the filtered bytes
        for (int rr = 0; rr <= rows; ++rr)
          for (int x = lane; x < tw; x += PD_T)
            tile[rr * kTileStride + x] = (rr == 0 && r0 == 0) ? (uint8_t)0 : raw[(r0 + rr - 1) * pitch + 1 + c0 + x];
        // up-left of the tile's first column: what the lane above left last (lane 0: the stored row above), zero in column 0
        uint8_t upleft = (uint8_t)__shfl_up((int)left, 1);
        if (lane == 0) upleft = (c0 > 0 && r0 > 0) ? raw[(r0 - 1) * pitch + c0] : (uint8_t)0;
        if (c0 == 0) upleft = 0;
        __syncthreads();
        const int steps = tw + rows - 1;
        for (int t = 0; t < steps; ++t) {
          const int col = t - lane;
          if (lane < rows && col >= 0 && col < tw) {
            const uint8_t x = tile[(lane + 1) * kTileStride + col], up = tile[lane * kTileStride + col];
            const uint8_t v = pz::unfilter(ft, x, left, up, upleft);
            tile[(lane + 1) * kTileStride + col] = v;
            left = v;
            upleft = up;
          }
          __syncthreads();
        }
        for (int x = lane; x < tw; x += PD_T) raw[(r0 + rows - 1) * pitch + 1 + c0 + x] = tile[rows * kTileStride + x];
        for (int rr = 0; rr < rows; ++rr)
          for (int x = lane; x < tw; x += PD_T) pz::unpack(tile[(rr + 1) * kTileStride + x], depth, c0 + x, W, pix + (r0 + rr) * W);
        __syncthreads();   // the tile is loaded again, and the next block reads the row just stored
      }
    }
  }
  if (lane == 0) {
    status[blockIdx.x] = rc;
    int32_t* o = stats + (size_t)blockIdx.x * pz::kStatWords;
    o[0] = st.kinds;
    o[1] = st.lit_bits;
    o[2] = st.dist_bits;
    o[3] = st.min_dist;
    o[4] = st.max_dist;
    o[5] = st.max_len;
    o[6] = st.filters;
    o[7] = st.bytes;
  }
}

}  // namespace

}  // namespace tt

using namespace tt;

extern "C" int tt_png_decode_batch(const uint8_t* streams, long long stream_bytes, const tt_png_stream* table_host, const tt_png_stream* table_dev,
                                   int n_files, uint8_t* out, long long out_bytes, void* workspace, size_t workspace_bytes, int32_t* status_dev,
                                   tt_stream_t stream) {
  TT_REQUIRE(streams && table_host && table_dev && out && workspace && status_dev, "png_decode_batch: null pointer");
  TT_REQUIRE((reinterpret_cast<uintptr_t>(streams) & 3u) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 3u) == 0 &&
                 (reinterpret_cast<uintptr_t>(table_dev) & 7u) == 0 && (reinterpret_cast<uintptr_t>(status_dev) & 3u) == 0,
             "png_decode_batch: streams, workspace and status must be 4-byte, the table 8-byte aligned");
  char msg[256];
  if (pz::validate(stream_bytes, table_host, n_files, out_bytes, workspace_bytes, msg, sizeof(msg)) != 0) {
    set_error("%s", msg);
    return TT_EINVAL;
  }
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  hipLaunchKernelGGL(png_decode_kernel, dim3((unsigned)n_files), dim3(PD_T), 0, as_stream(stream), streams, table_dev, out, ws,
                     reinterpret_cast<int32_t*>(ws + pz::slices_end(table_host, n_files)), status_dev);
  TT_CHECK_LAUNCH("png_decode_batch");
  return TT_OK;
}
