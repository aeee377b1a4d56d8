// N24: the Huffman streams of a batch of baseline JPEG frames decoded on the device - self-synchronising subsequence decode, the
// scheme, its state step and its bounds in jpeg_huff.hpp (which tt_jpeg_entropy_host in jpeg_scan.cpp runs lane by lane on the host).
//
// One workgroup of jh::kTile = 256 lanes owns one frame and walks its subsequences in tiles of 256: no workgroup waits on another, no
// flag, no spin.  Per tile:
//   assign  the lanes load the subsequence counts of the next 256 segments; lane 0 deals subsequences to lanes in scan order (a frame
//           without DRI is one segment; one with an interval of one MCU has a segment per lane).
//   rounds  every lane decodes its subsequence from its entry state and leaves the exit state and the blocks it completed in LDS; then it
//           takes its left neighbour's exit state as entry and decodes again if that changed.  The loop ends when a round changes nothing
//           (__syncthreads_or) and is bounded by the tile size: after round r the first r + 1 states are the true ones.  The first lane
//           of a tile enters with the state the last lane of the tile before left (the true one).
//   count   a lane's first block = the blocks of the lanes to its left in the same segment (+ the segment's blocks in earlier tiles).
//   write   one more pass from the true state writes coefficients and DC differences and reports errors; the lowest failing lane sets
//           the frame's status and the workgroup stops.
// After the last tile the DC differences become predictions: per component the lanes sum contiguous chunks of the scan order, a
// segmented scan over the 256 chunk sums in LDS gives every chunk its carry, and the chunk is rewritten.
// LDS: six tables (9.1 KB) + seven words per lane: under 17 KB.  The table look-ups are data-dependent gathers (bank conflicts are the
// cost of the scheme); the stream is read through a 64-bit register window, one 4-byte load per 32 bits consumed.  The lanes of a wave
// diverge in the symbol loop by nature: step() keeps the common path (look table hit, value bits) straight-line.
#include "common.hpp"
#include "jpeg_huff.hpp"

namespace tt {

namespace {

constexpr int JE_T = jh::kTile;

__global__ __launch_bounds__(JE_T) void jpeg_entropy_kernel(const uint8_t* __restrict__ scan, const uint32_t* __restrict__ segs,
                                                           const tt_jpeg_stream* __restrict__ table, uint32_t S, int16_t* __restrict__ coeffs,
                                                           int32_t* __restrict__ status, int32_t* __restrict__ stats) {
  __shared__ jh::Table tabs[6];
  __shared__ uint32_t s_nsub[JE_T], s_seg[JE_T], s_sub[JE_T], s_p[JE_T], s_q[JE_T], s_cnt[JE_T];
  __shared__ int s_reset[JE_T];
  __shared__ uint32_t s_cur_seg, s_cur_sub, s_n, s_carry_p, s_carry_q, s_carry_blocks;
  __shared__ int s_first_bad, s_status;

  const int i = (int)threadIdx.x;
  const tt_jpeg_stream row = table[blockIdx.x];
  const jh::Frame f = jh::make_frame(row);
  const uint8_t* __restrict__ dht = scan + row.huff_off;
  const uint32_t* __restrict__ stream = reinterpret_cast<const uint32_t*>(scan + row.scan_off);
  const uint32_t* __restrict__ sg = segs + 2 * row.seg_off;

  for (int k = i; k < 6 * 256; k += JE_T) tabs[k >> 8].vals[k & 255] = dht[(k >> 8) * jh::kDht + 16 + (k & 255)];
  if (i < 6) jh::build_codes(tabs[i], dht + i * jh::kDht);
  if (i == 0) {
    s_cur_seg = s_cur_sub = 0;
    s_carry_p = s_carry_q = s_carry_blocks = 0;
    s_status = 0;
  }
  __syncthreads();
  for (int k = i; k < 6 << jh::kLook; k += JE_T) tabs[k >> jh::kLook].look[k & ((1 << jh::kLook) - 1)] = jh::look_entry(tabs[k >> jh::kLook], k & ((1 << jh::kLook) - 1));
  __syncthreads();

  int rounds = 0, tiles = 0, first_bad = -1;
  uint32_t subs = 0;
  // every tile takes at least one subsequence, so the tiles are at most the frame's subsequences
  while (true) {
    const uint32_t seg0 = s_cur_seg, sub0 = s_cur_sub;
    if (seg0 >= f.n_segments || s_status != 0) break;   // uniform: read behind a barrier
    s_nsub[i] = seg0 + (uint32_t)i < f.n_segments ? jh::subsequences(sg[2 * (seg0 + (uint32_t)i) + 1], S) : 0u;
    __syncthreads();
    if (i == 0) {
      uint32_t n = 0, seg = seg0, sub = sub0;
      while (n < (uint32_t)JE_T && seg < f.n_segments) {   // seg - seg0 <= n: every segment takes a lane
        s_seg[n] = seg;
        s_sub[n] = sub;
        ++n;
        if (++sub >= s_nsub[seg - seg0]) {
          ++seg;
          sub = 0;
        }
      }
      s_n = n;
      s_cur_seg = seg;
      s_cur_sub = sub;
      s_first_bad = JE_T;
    }
    __syncthreads();
    const int n = (int)s_n;
    const bool active = i < n;
    uint32_t seg = 0, sub = 0, bits = 0, end = 0;
    const uint32_t* words = stream;
    jh::State entry{0, 0, 0, 0};
    if (active) {
      seg = s_seg[i];
      sub = s_sub[i];
      bits = sg[2 * seg + 1];
      words = stream + sg[2 * seg] / 4;
      end = (sub + 1) * S < bits ? (sub + 1) * S : bits;
      if (sub != 0) entry = i == 0 ? jh::unpack(s_carry_p, s_carry_q) : jh::State{sub * S, 0, 0, 0};
    }
    bool dirty = active;
    for (int round = 0; round <= JE_T; ++round) {
      if (dirty) {
        jh::State s = entry;
        s_cnt[i] = jh::run_count(tabs, f, words, bits, s, end, seg);
        s_p[i] = s.p;
        s_q[i] = jh::pack(s);
      }
      __syncthreads();
      dirty = false;
      if (active && i > 0 && sub != 0) {
        const uint32_t p = s_p[i - 1], q = s_q[i - 1];
        if (p != entry.p || q != jh::pack(entry)) {
          entry = jh::unpack(p, q);
          dirty = true;
        }
      }
      if (!__syncthreads_or(dirty ? 1 : 0)) break;
      ++rounds;
    }
    uint32_t n0 = 0;
    int err = 0;
    if (active) {
      int u = i - 1;
      for (; u >= 0 && s_seg[u] == seg; --u) n0 += s_cnt[u];
      if (u < 0 && sub > (uint32_t)i) n0 += s_carry_blocks;
      err = jh::run_write(tabs, f, words, bits, entry, end, seg, n0, coeffs);
      if (err) atomicMin(&s_first_bad, i);
    }
    __syncthreads();
    if (active && s_first_bad == i) {
      s_status = err;
      first_bad = (int)subs + i;
    }
    if (i == n - 1) {
      s_carry_p = s_p[i];
      s_carry_q = s_q[i];
      s_carry_blocks = n0 + s_cnt[i];
    }
    subs += (uint32_t)n;
    ++tiles;
    __syncthreads();
  }
  const int st = s_status;
  if (st == 0) {
    for (int c = 0; c < 3; ++c) {
      const uint32_t total = jh::dc_blocks(f, c), per = (total + JE_T - 1) / JE_T;
      const uint32_t j0 = (uint32_t)i * per < total ? (uint32_t)i * per : total, j1 = j0 + per < total ? j0 + per : total;
      int reset = 0;
      __syncthreads();   // the write pass of every lane, and the component before, are behind us
      s_p[i] = jh::dc_sum(f, coeffs, c, j0, j1, &reset);
      s_reset[i] = reset;
      __syncthreads();
      uint32_t carry = 0;
      for (int u = i - 1; u >= 0; --u) {
        carry += s_p[u];
        if (s_reset[u]) break;
      }
      jh::dc_apply(f, coeffs, c, j0, j1, carry);
    }
  }
  // one lane per tile may have recorded the failing subsequence; the counts are uniform
  if (first_bad >= 0) stats[blockIdx.x * jh::kStatWords + 3] = first_bad;
  if (i == 0) {
    status[blockIdx.x] = st;
    int32_t* o = stats + blockIdx.x * jh::kStatWords;
    o[0] = rounds;
    o[1] = tiles;
    o[2] = (int32_t)subs;
    if (st == 0) o[3] = -1;
  }
}

}  // namespace

}  // namespace tt

using namespace tt;

extern "C" int tt_jpeg_entropy_batch(const uint8_t* scan, long long scan_bytes, const uint32_t* segs_host, const uint32_t* segs_dev, long long n_segs,
                                     const tt_jpeg_stream* stream_table_host, const tt_jpeg_stream* stream_table_dev, int n_frames, int subseq_bits,
                                     int16_t* coeffs, long long n_coeffs, int32_t* status, void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  TT_REQUIRE(scan && segs_host && segs_dev && stream_table_host && stream_table_dev && coeffs && status && workspace, "jpeg_entropy_batch: null pointer");
  TT_REQUIRE((reinterpret_cast<uintptr_t>(scan) & 3u) == 0 && (reinterpret_cast<uintptr_t>(segs_dev) & 3u) == 0 && aligned16(coeffs) &&
                 (reinterpret_cast<uintptr_t>(stream_table_dev) & 7u) == 0 && (reinterpret_cast<uintptr_t>(status) & 3u) == 0 &&
                 (reinterpret_cast<uintptr_t>(workspace) & 3u) == 0,
             "jpeg_entropy_batch: scan, segments, status and workspace must be 4-byte, the table 8-byte, coeffs 16-byte aligned");
  char msg[256];
  if (jh::validate(scan_bytes, segs_host, n_segs, stream_table_host, n_frames, subseq_bits, n_coeffs, msg, sizeof(msg)) != 0) {
    set_error("%s", msg);
    return TT_EINVAL;
  }
  TT_REQUIRE(workspace_bytes >= jh::workspace_bytes(n_frames), "jpeg_entropy_batch: a workspace of %zu bytes, %zu needed", workspace_bytes,
             jh::workspace_bytes(n_frames));
  hipStream_t s = as_stream(stream);
  if (n_coeffs > 0 && hipMemsetAsync(coeffs, 0, sizeof(int16_t) * (size_t)n_coeffs, s) != hipSuccess) {
    set_error("jpeg_entropy_batch: clearing the coefficients failed: %s", hipGetErrorString(hipGetLastError()));
    return TT_ELAUNCH;
  }
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)n_frames), dim3(JE_T), 0, s, scan, segs_dev, stream_table_dev, (uint32_t)subseq_bits, coeffs,
                     status, static_cast<int32_t*>(workspace));
  TT_CHECK_LAUNCH("jpeg_entropy_batch");
  return TT_OK;
}
