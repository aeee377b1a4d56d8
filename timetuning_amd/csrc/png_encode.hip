// N29: the label maps of a batch deflated on the device into PNG streams; the byte format, its steps and the table rules are in
// png_deflate.hpp (which tt_png_encode_host in png_scan.cpp runs sequentially on the host).
//
// Three launches, ordered by the stream and by nothing else: no workgroup waits for another, no look-back, no spin, no counter.
//   chunks   one workgroup of 256 threads per (file, chunk).  Thread t owns the `ipt` consecutive positions from t * ipt (ipt: the power
//            of two from 8 up with 256 ipt >= n).  The filtered bytes are staged in LDS with the lanes along the rows, each thread's
//            segment ipt + 4 bytes from the next (an odd number of words: the lanes of a wave read 64 different banks) - up to the
//            16 384 bytes of a chunk of several rows; the single-row chunk of a map wider than that reads the filtered bytes through
//            the cache instead, so that the bit buffer alone (36 872 bytes for 32 768 positions) stays within the static 64 KB.
//            pass 0   run starts: the first and the last one of the segment, and the segment's Adler sums;
//            scans    the last run start before the segment (prefix max) and the first one behind it (suffix min) over the threads;
//            pass 1   pe::walk counts the bits of the segment's tokens; their exclusive sum over the threads is the bit offset;
//            pass 2   pe::walk again ORs every token's bits into the zeroed bit buffer (LDS atomics: the OR commutes, the bytes do not
//                     depend on the order); thread 0 adds the block header and the stored block.
//            The buffer goes to the chunk's slot as whole words (so a slot never keeps bits of an earlier call), the length and the
//            Adler (a, b, n) behind the slots.
//   scan     ONE workgroup: the exclusive sum of all chunk lengths in table order IS every chunk's place in the compact output (files
//            follow each other); then one thread per file combines its chunks' Adler triples and writes (offset, length, adler).
//   gather   one workgroup per chunk copies slot -> output.
// Wave64 scans: __shfl_up / __shfl_down inside a wave, one LDS pass across the waves.
#include "common.hpp"
#include "png_deflate.hpp"

namespace tt {

namespace {

constexpr int PE_T = 256, PE_WAVES = PE_T / kWave;
constexpr int kStagePad = 4;
constexpr int kStageBytes = PE_T * (pe::kChunkBytes / PE_T + kStagePad);
constexpr int kBitWords = (int)(pe::slot_stride(pe::kMaxChunkBytes) / 4);
constexpr int SCAN_T = 1024, SCAN_WAVES = SCAN_T / kWave;

struct OpMax {
  static constexpr int ident = -1;
  __device__ static int of(int a, int b) { return a > b ? a : b; }
};
struct OpMin {
  static constexpr int ident = 0x7fffffff;
  __device__ static int of(int a, int b) { return a < b ? a : b; }
};
struct OpSum {
  static constexpr int ident = 0;
  __device__ static int of(int a, int b) { return a + b; }
};

// The EXCLUSIVE scan of v over the threads of the workgroup (Reverse: over the threads behind this one) and, in *total, the whole.
// Every thread must call it; s_w: NW ints of LDS, free again when it returns.
template <class Op, bool Reverse, int NW>
__device__ int block_scan(int v, int* s_w, int* total) {
  const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = Reverse ? __shfl_down(x, o, 64) : __shfl_up(x, o, 64);
    if (Reverse ? lane + o < 64 : lane >= o) x = Op::of(x, y);
  }
  if (lane == (Reverse ? 0 : 63)) s_w[w] = x;
  int before = Reverse ? __shfl_down(x, 1, 64) : __shfl_up(x, 1, 64);
  if (lane == (Reverse ? 63 : 0)) before = Op::ident;
  __syncthreads();
  int all = Op::ident;
  for (int k = 0; k < NW; ++k) {
    const int t = s_w[k];
    all = Op::of(all, t);
    if (Reverse ? k > w : k < w) before = Op::of(before, t);
  }
  __syncthreads();
  if (total) *total = all;
  return before;
}

__global__ __launch_bounds__(PE_T) void png_encode_chunk_kernel(const tt_png_map* __restrict__ maps, const tt_png_chunk* __restrict__ chunks,
                                                               uint8_t* __restrict__ slots, int32_t* __restrict__ meta) {
  __shared__ uint8_t s_f[kStageBytes];
  __shared__ uint32_t s_bits[kBitWords];
  __shared__ int s_w[PE_WAVES];

  const int tid = (int)threadIdx.x;
  const tt_png_chunk ck = chunks[blockIdx.x];
  const tt_png_map m = maps[ck.map];
  const uint8_t* x = m.data;
  const long long pitch = m.pitch;
  const int W = (int)m.W, row0 = (int)ck.row0;
  const int n = (int)ck.rows * (W + 1);   // <= pe::kMaxChunkBytes by the chunk rule (the host checked the tables)
  int shift = 3;
  while ((PE_T << shift) < n) ++shift;
  const int ipt = 1 << shift, seg = ipt + kStagePad;
  const bool staged = n <= pe::kChunkBytes;   // ipt <= 64
  if (staged)
    for (int p = tid; p < n; p += PE_T) s_f[(p >> shift) * seg + (p & (ipt - 1))] = pe::filtered(x, pitch, W, row0, p);
  __syncthreads();
  auto F = [&](int p) -> uint8_t { return staged ? s_f[(p >> shift) * seg + (p & (ipt - 1))] : pe::filtered(x, pitch, W, row0, p); };

  // pass 0: the run starts of the segment, and its Adler sums (at most 128 x 255 x 32 768: inside 32 bits)
  const int p0 = (tid << shift) < n ? (tid << shift) : n, p1 = p0 + ipt < n ? p0 + ipt : n;
  int first = n, last = -1;
  uint32_t sa = 0, sb = 0;
  {
    uint8_t prev = p0 > 0 && p0 < n ? F(p0 - 1) : (uint8_t)0;
    for (int p = p0; p < p1; ++p) {
      const uint8_t b = F(p);
      if (p == 0 || b != prev) {
        if (first == n) first = p;
        last = p;
      }
      sa += b;
      sb += (uint32_t)(n - p) * b;
      prev = b;
    }
  }
  const int s_in = block_scan<OpMax, false, PE_WAVES>(last, s_w, nullptr);
  int e_out = block_scan<OpMin, true, PE_WAVES>(first, s_w, nullptr);
  if (e_out > n) e_out = n;

  // pass 1: the bits of the segment's tokens
  int my_bits = 0;
  pe::walk(F, p0, p1, s_in, e_out, [&](pe::Code c) { my_bits += c.count; });
  int token_bits = 0;
  const int bit_off = block_scan<OpSum, false, PE_WAVES>(my_bits, s_w, &token_bits);
  int adler_a = 0, adler_b = 0;
  block_scan<OpSum, false, PE_WAVES>((int)(sa % pe::kAdlerMod), s_w, &adler_a);
  block_scan<OpSum, false, PE_WAVES>((int)(sb % pe::kAdlerMod), s_w, &adler_b);

  const int len = pe::chunk_bytes((uint32_t)token_bits), words = (len + 3) / 4;   // <= kBitWords: slot_bytes is the bound of chunk_bytes
  for (int k = tid; k < words; k += PE_T) s_bits[k] = 0u;
  __syncthreads();

  // pass 2: the tokens' bits, then the frame
  auto or32 = [&](uint32_t word, uint32_t v) {
    if (v != 0u && word < (uint32_t)words) atomicOr(&s_bits[word], v);
  };
  uint32_t at = (uint32_t)(pe::kHeadBits + bit_off);
  pe::walk(F, p0, p1, s_in, e_out, [&](pe::Code c) {
    pe::put_bits(or32, at, c.bits, c.count);
    at += (uint32_t)c.count;
  });
  const bool last_chunk = (long long)blockIdx.x == m.first_chunk + m.n_chunks - 1;
  if (tid == 0) pe::put_frame(or32, (uint32_t)token_bits, last_chunk);
  __syncthreads();

  uint32_t* dst = reinterpret_cast<uint32_t*>(slots + ck.slot_off);
  for (int k = tid; k < words; k += PE_T) dst[k] = s_bits[k];
  if (tid == 0) {
    int32_t* o = meta + (size_t)blockIdx.x * pe::kMetaWords;
    o[0] = len;
    o[1] = (int32_t)((uint32_t)adler_a % pe::kAdlerMod);
    o[2] = (int32_t)((uint32_t)adler_b % pe::kAdlerMod);
    o[3] = n;
  }
}

__global__ __launch_bounds__(SCAN_T) void png_encode_scan_kernel(const tt_png_map* __restrict__ maps, int n_maps,
                                                               const tt_png_chunk* __restrict__ chunks, long long n_chunks,
                                                               const int32_t* __restrict__ meta, uint32_t* __restrict__ chunk_off,
                                                               tt_png_result* __restrict__ results) {
  __shared__ int s_w[SCAN_WAVES];
  const int tid = (int)threadIdx.x;
  uint32_t carry = 0;   // the same in every thread
  for (long long base = 0; base < n_chunks; base += SCAN_T) {
    const long long i = base + tid;
    const int v = i < n_chunks ? meta[i * pe::kMetaWords] : 0;
    int tile = 0;
    const int before = block_scan<OpSum, false, SCAN_WAVES>(v, s_w, &tile);   // the slots of a call are below 2^31 bytes
    if (i < n_chunks) {
      const uint32_t off = carry + (uint32_t)before;
      chunk_off[i] = off;
      if (chunks[i].row0 == 0) results[chunks[i].map].offset = (int64_t)off;
    }
    carry += (uint32_t)tile;
  }
  for (int f = tid; f < n_maps; f += SCAN_T) {
    const tt_png_map m = maps[f];
    uint32_t A = 1, B = 0;
    int64_t length = 0;
    for (long long c = m.first_chunk; c < m.first_chunk + m.n_chunks; ++c) {
      const int32_t* o = meta + c * pe::kMetaWords;
      length += o[0];
      pe::adler_append(A, B, (uint32_t)o[1], (uint32_t)o[2], (uint32_t)o[3]);
    }
    results[f].length = length;
    results[f].adler = (int64_t)((B << 16) | A);
    results[f].reserved = 0;
  }
}

__global__ __launch_bounds__(PE_T) void png_encode_gather_kernel(const tt_png_chunk* __restrict__ chunks, const uint8_t* __restrict__ slots,
                                                                const int32_t* __restrict__ meta, const uint32_t* __restrict__ chunk_off,
                                                                uint8_t* __restrict__ out, long long out_bytes) {
  const long long off = chunk_off[blockIdx.x];
  const int len = meta[(size_t)blockIdx.x * pe::kMetaWords];
  if (len < 0 || off + len > out_bytes) return;   // cannot happen after the host's checks: the lengths sum to at most the slots
  const uint8_t* src = slots + chunks[blockIdx.x].slot_off;
  for (int k = (int)threadIdx.x; k < len; k += PE_T) out[off + k] = src[k];
}

}  // namespace

}  // namespace tt

using namespace tt;

extern "C" int tt_png_encode_batch(const tt_png_map* maps_host, const tt_png_map* maps_dev, int n_maps, const tt_png_chunk* chunks_host,
                                   const tt_png_chunk* chunks_dev, long long n_chunks, uint8_t* out, long long out_bytes,
                                   tt_png_result* results_dev, void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  if (!maps_host || !maps_dev || !chunks_host || !chunks_dev || !out || !results_dev || !workspace) {
    set_error("png_encode_batch: null pointer");
    return TT_PNG_EARGUMENT;
  }
  if ((reinterpret_cast<uintptr_t>(workspace) & 15u) || (reinterpret_cast<uintptr_t>(maps_dev) & 7u) || (reinterpret_cast<uintptr_t>(chunks_dev) & 7u) ||
      (reinterpret_cast<uintptr_t>(results_dev) & 7u)) {
    set_error("png_encode_batch: the workspace must be 16-byte, the tables and the results 8-byte aligned");
    return TT_PNG_EARGUMENT;
  }
  pe::Layout l;
  const char* why = "";
  if (pe::validate(maps_host, n_maps, chunks_host, n_chunks, out_bytes, workspace_bytes, &l, &why) != 0) {
    set_error("png_encode_batch: %s", why);
    return TT_PNG_EARGUMENT;
  }
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  int32_t* meta = reinterpret_cast<int32_t*>(ws + pe::meta_offset(l));
  uint32_t* chunk_off = reinterpret_cast<uint32_t*>(ws + pe::offsets_offset(l));
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(png_encode_chunk_kernel, dim3((unsigned)l.n_chunks), dim3(PE_T), 0, s, maps_dev, chunks_dev, ws, meta);
  TT_CHECK_LAUNCH("png_encode_batch (chunks)");
  hipLaunchKernelGGL(png_encode_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, maps_dev, n_maps, chunks_dev, l.n_chunks, meta, chunk_off, results_dev);
  TT_CHECK_LAUNCH("png_encode_batch (scan)");
  hipLaunchKernelGGL(png_encode_gather_kernel, dim3((unsigned)l.n_chunks), dim3(PE_T), 0, s, chunks_dev, ws, meta, chunk_off, out, out_bytes);
  TT_CHECK_LAUNCH("png_encode_batch (gather)");
  return TT_OK;
}
