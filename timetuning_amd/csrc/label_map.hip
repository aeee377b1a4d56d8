// Label maps as byte streams (N23): which values occur in a segment, and the YouTube-VOS instance -> category remap built on it
// (data_loader.py:453-464 make_categories_dict, :497-506 map_instances, :774-796 YVOSDataset).
//
//   tt_label_presence_segments   words[s][v >> 5] bit (v & 31) is set iff value v (0 .. 255) occurs among the P labels of segment s
//                                (elements s P ... s P + P - 1; uint8, or int64 for the evaluator's .long() maps).  An int64 value
//                                outside 0 .. 255 sets status[s] = 1 and no bit.  What torch.unique(segment) answers for label maps,
//                                for ALL segments in one launch and 32 bytes per segment to read back.
//   tt_map_instances             out[e] = lut_s[in[e]] on uint8: the presence pass, then an apply pass whose workgroups each compose
//                                the 256-entry table of their segment in LDS from the presence bits and cat[s][256] before gathering.
//
// The table (ml_compose; data_loader.compose_instance_lut is the host statement the tests hold it to):
//   sequential  the reference's in-place loop `frame[frame == obj] = category` over the ascending torch.unique of the ORIGINAL clip:
//               start from the identity; for obj = 1 .. 255 in order, if obj is present, every entry whose CURRENT value equals obj
//               becomes cat[obj].  A pixel remapped onto a value that is itself a later, present object id is remapped again: the
//               reference's chaining, reproduced.  Each thread owns one entry in a register and walks the 255 steps: no barrier inside.
//   plain       v -> cat[v] for present v >= 1.
//   Value 0 is never remapped.  A present object whose cat is outside 0 .. 255 (-1 = "not in the meta file") makes status[s] the smallest
//   such id and the table the identity: the segment is copied unmapped.
//
// No workgroup waits on another: the presence bits are OR-ed with ordinary global atomics into words the entry zeroed on the stream, the
// apply pass is a later launch on the same stream.  Every workgroup of a segment composes the same table from the same finished words.
//
// Loads: a segment starts at byte s P elem_bytes of the tensor, whatever that is modulo 16.  A workgroup's share of the segment is
// whole 16-byte chunks of the part between the first and the last 16-byte boundary inside it (uint4 loads; the apply pass stores uint4 where
// the output is 16-byte aligned at the same element, bytes otherwise), the fewer than 16 bytes before and after are taken one per thread
// by the segment's first workgroup.  Label maps come in runs: a chunk whose 16 bytes all equal the value this thread marked last is
// skipped by one compare, and the LDS bitmap is READ before it is OR-ed, so atomics stop once a value's bit is set.
#include "common.hpp"

namespace tt {

constexpr int ML_THREADS = 256;
constexpr int ML_WORDS = 8;                          // 256 presence bits
constexpr long long ML_CHUNKS_PER_WG = 4 * ML_THREADS;   // 16-byte chunks a workgroup walks at least (where the segment has them): 16 KB
constexpr int ML_MAX_GRID_X = 1024;
constexpr int ML_MAX_GRID_Y = 65535;

inline unsigned ml_blocks(long long bytes) {
  const long long chunks = bytes / 16 + 1;
  long long b = (chunks + ML_CHUNKS_PER_WG - 1) / ML_CHUNKS_PER_WG;
  if (b > ML_MAX_GRID_X) b = ML_MAX_GRID_X;
  return (unsigned)(b < 1 ? 1 : b);
}

// the part of [p, p + bytes) between 16-byte boundaries: head bytes in front of it, `chunks` whole chunks, then the tail
struct MlSpan {
  long long head, chunks, tail0;
};
__device__ __forceinline__ MlSpan ml_span(const uint8_t* p, long long bytes) {
  MlSpan sp;
  sp.head = (long long)((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u);
  if (sp.head > bytes) sp.head = bytes;
  sp.chunks = (bytes - sp.head) / 16;
  sp.tail0 = sp.head + sp.chunks * 16;
  return sp;
}

__device__ __forceinline__ void ml_mark(unsigned int* bits, unsigned v) {   // v in 0 .. 255
  const unsigned bit = 1u << (v & 31u);
  if (!(bits[v >> 5] & bit)) atomicOr(&bits[v >> 5], bit);
}

template <int EB>   // element bytes: 1 (uint8) or 8 (int64)
__global__ __launch_bounds__(ML_THREADS) void label_presence_kernel(const uint8_t* __restrict__ labels, long long P, unsigned int* __restrict__ words,
                                                                    int* __restrict__ status, int s0) {
  __shared__ unsigned int bits[ML_WORDS];
  __shared__ int bad_any;
  const long long s = (long long)s0 + blockIdx.y;
  const long long bytes = P * EB;
  const uint8_t* __restrict__ p = labels + s * bytes;
  if (threadIdx.x < ML_WORDS) bits[threadIdx.x] = 0;
  if (threadIdx.x == 0) bad_any = 0;
  __syncthreads();
  const MlSpan sp = ml_span(p, bytes);   // (EB == 8: p is 8-byte aligned, the entry checks, so head is 0 or 8 bytes: whole elements)
  bool bad = false;
  if (blockIdx.x == 0) {   // head and tail: fewer than 16 bytes each, one ELEMENT per thread
    const long long t = threadIdx.x;
    long long off = -1;
    if (t * EB < sp.head)
      off = t * EB;
    else if (t >= 16 && sp.tail0 + (t - 16) * EB < bytes)
      off = sp.tail0 + (t - 16) * EB;
    if (off >= 0) {
      if (EB == 1) {
        ml_mark(bits, p[off]);
      } else {
        const long long v = *reinterpret_cast<const long long*>(p + off);
        if ((unsigned long long)v < 256ull) ml_mark(bits, (unsigned)v); else bad = true;
      }
    }
  }
  const uint8_t* __restrict__ body = p + sp.head;
  unsigned last = 0xffffffffu;   // the value this thread marked last (none yet)
  for (long long i = (long long)blockIdx.x * ML_THREADS + threadIdx.x; i < sp.chunks; i += (long long)gridDim.x * ML_THREADS) {
    const uint4 q = *reinterpret_cast<const uint4*>(body + i * 16);
    if (EB == 1) {
      const unsigned splat = last * 0x01010101u;   // (used only once a value has been marked: last <= 255)
      if (last <= 255u && q.x == splat && q.y == splat && q.z == splat && q.w == splat) continue;
      const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const unsigned v = (w[j] >> (8 * b)) & 0xffu;
          if (v != last) {
            ml_mark(bits, v);
            last = v;
          }
        }
      }
    } else {
      const long long v0 = (long long)(((unsigned long long)q.y << 32) | q.x), v1 = (long long)(((unsigned long long)q.w << 32) | q.z);
      if ((unsigned long long)v0 < 256ull) {
        if ((unsigned)v0 != last) {
          ml_mark(bits, (unsigned)v0);
          last = (unsigned)v0;
        }
      } else {
        bad = true;
      }
      if ((unsigned long long)v1 < 256ull) {
        if ((unsigned)v1 != last) {
          ml_mark(bits, (unsigned)v1);
          last = (unsigned)v1;
        }
      } else {
        bad = true;
      }
    }
  }
  if (bad) bad_any = 1;   // (every writer stores the same value)
  __syncthreads();
  if (threadIdx.x < ML_WORDS) {
    const unsigned int w = bits[threadIdx.x];
    if (w) atomicOr(&words[s * ML_WORDS + threadIdx.x], w);
  }
  if (threadIdx.x == ML_WORDS && bad_any) atomicOr(&status[s], 1);
}

// The table of one segment, entry threadIdx.x in the calling thread's register; *bad_id (LDS): the smallest present id >= 1 whose cat is
// outside 0 .. 255, or 256.  present / cats: LDS, ML_THREADS entries each.  Two barriers, every thread of the workgroup must call it.
__device__ __forceinline__ unsigned ml_compose(const unsigned int* __restrict__ words_s, const int* __restrict__ cat_s, int sequential,
                                               unsigned char* present, int* cats, int* bad_id) {
  const unsigned t = threadIdx.x;
  const bool here = (words_s[t >> 5] >> (t & 31u)) & 1u;
  const int c = cat_s[t];
  present[t] = here ? 1 : 0;
  cats[t] = c;
  if (t == 0) *bad_id = 256;
  __syncthreads();
  if (t >= 1 && here && (c < 0 || c > 255)) atomicMin(bad_id, (int)t);
  __syncthreads();
  unsigned v = t;
  if (*bad_id == 256) {
    if (sequential) {
      for (unsigned obj = 1; obj < 256; ++obj)   // uniform trip count; present[obj] and cats[obj] are broadcast reads
        if (present[obj] && v == obj) v = (unsigned)cats[obj];
    } else if (t >= 1 && here) {
      v = (unsigned)c;
    }
  }
  return v;
}

__global__ __launch_bounds__(ML_THREADS) void map_instances_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, long long P,
                                                                   const unsigned int* __restrict__ words, const int* __restrict__ cat,
                                                                   int sequential, uint8_t* __restrict__ lut_out, int* __restrict__ status,
                                                                   int s0) {
  __shared__ unsigned char present[ML_THREADS];
  __shared__ int cats[ML_THREADS];
  __shared__ int bad_id;
  __shared__ __attribute__((aligned(16))) unsigned char lut[ML_THREADS];
  const long long s = (long long)s0 + blockIdx.y;
  const unsigned v = ml_compose(words + s * ML_WORDS, cat + s * 256, sequential, present, cats, &bad_id);
  lut[threadIdx.x] = (unsigned char)v;
  if (blockIdx.x == 0) {
    lut_out[s * 256 + threadIdx.x] = (unsigned char)v;
    if (threadIdx.x == 0) status[s] = bad_id == 256 ? 0 : bad_id;
  }
  __syncthreads();
  const uint8_t* __restrict__ p = in + s * P;
  uint8_t* __restrict__ o = out + s * P;
  const MlSpan sp = ml_span(p, P);
  if (blockIdx.x == 0) {
    const long long t = threadIdx.x;
    long long off = -1;
    if (t < sp.head)
      off = t;
    else if (t >= 16 && sp.tail0 + (t - 16) < P)
      off = sp.tail0 + (t - 16);
    if (off >= 0) o[off] = lut[p[off]];
  }
  const uint8_t* __restrict__ body = p + sp.head;
  uint8_t* __restrict__ obody = o + sp.head;
  const bool out16 = (reinterpret_cast<uintptr_t>(obody) & 15u) == 0;   // uniform over the workgroup
  for (long long i = (long long)blockIdx.x * ML_THREADS + threadIdx.x; i < sp.chunks; i += (long long)gridDim.x * ML_THREADS) {
    const uint4 q = *reinterpret_cast<const uint4*>(body + i * 16);
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
    unsigned r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      r[j] = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) r[j] |= (unsigned)lut[(w[j] >> (8 * b)) & 0xffu] << (8 * b);
    }
    if (out16) {
      *reinterpret_cast<uint4*>(obody + i * 16) = make_uint4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int b = 0; b < 4; ++b) obody[i * 16 + 4 * j + b] = (uint8_t)(r[j] >> (8 * b));
    }
  }
}

static int ml_presence(const char* who, const void* labels, int elem_bytes, int S, long long P, unsigned int* words, int* status, hipStream_t s) {
  if (hipMemsetAsync(words, 0, sizeof(unsigned int) * ML_WORDS * (size_t)S, s) != hipSuccess ||
      hipMemsetAsync(status, 0, sizeof(int) * (size_t)S, s) != hipSuccess) {
    set_error("%s: memset failed", who);
    return TT_ELAUNCH;
  }
  const unsigned bx = ml_blocks(P * elem_bytes);
  const uint8_t* p = static_cast<const uint8_t*>(labels);
  for (int s0 = 0; s0 < S; s0 += ML_MAX_GRID_Y) {   // the segments ride on gridDim.y, at most 65535 per launch
    const dim3 grid(bx, (unsigned)(S - s0 < ML_MAX_GRID_Y ? S - s0 : ML_MAX_GRID_Y));
    if (elem_bytes == 1)
      hipLaunchKernelGGL((label_presence_kernel<1>), grid, dim3(ML_THREADS), 0, s, p, P, words, status, s0);
    else
      hipLaunchKernelGGL((label_presence_kernel<8>), grid, dim3(ML_THREADS), 0, s, p, P, words, status, s0);
  }
  return TT_OK;
}

}  // namespace tt

using namespace tt;

extern "C" int tt_label_presence_segments(const void* labels, int elem_bytes, int S, long long P, uint32_t* words, int32_t* status,
                                          tt_stream_t stream) {
  TT_REQUIRE(labels && words && status, "label_presence_segments: null pointer (labels %p, words %p, status %p)", labels, (void*)words, (void*)status);
  TT_REQUIRE(elem_bytes == 1 || elem_bytes == 8, "label_presence_segments: elem_bytes = %d is neither 1 (uint8) nor 8 (int64)", elem_bytes);
  TT_REQUIRE(S >= 1 && P >= 1, "label_presence_segments: S = %d segments of P = %lld labels: need both >= 1", S, P);
  TT_REQUIRE(P <= (1ll << 59) / S, "label_presence_segments: S = %d segments of P = %lld labels exceed 2^59 labels", S, P);
  TT_REQUIRE(reinterpret_cast<uintptr_t>(labels) % (size_t)elem_bytes == 0 && reinterpret_cast<uintptr_t>(words) % 4 == 0 &&
                 reinterpret_cast<uintptr_t>(status) % 4 == 0,
             "label_presence_segments: labels (%p) must be aligned to its %d-byte elements, words (%p) and status (%p) to 4 bytes", labels,
             elem_bytes, (void*)words, (void*)status);
  hipStream_t s = as_stream(stream);
  const int rc = ml_presence("label_presence_segments", labels, elem_bytes, S, P, words, status, s);
  if (rc != TT_OK) return rc;
  TT_CHECK_LAUNCH("label_presence_segments");
  return TT_OK;
}

extern "C" size_t tt_map_instances_workspace_bytes(int S) { return S < 1 ? 0 : sizeof(unsigned int) * ML_WORDS * (size_t)S; }

extern "C" int tt_map_instances(const uint8_t* labels_in, uint8_t* labels_out, const int32_t* cat, int S, long long P, int sequential,
                                uint8_t* lut_out, int32_t* status, void* words_ws, size_t words_ws_bytes, tt_stream_t stream) {
  TT_REQUIRE(labels_in && labels_out && cat && lut_out && status && words_ws,
             "map_instances: null pointer (labels_in %p, labels_out %p, cat %p, lut_out %p, status %p, words_ws %p)", (const void*)labels_in,
             (void*)labels_out, (const void*)cat, (void*)lut_out, (void*)status, words_ws);
  TT_REQUIRE(S >= 1 && P >= 1, "map_instances: S = %d segments of P = %lld labels: need both >= 1", S, P);
  TT_REQUIRE(P <= (1ll << 59) / S, "map_instances: S = %d segments of P = %lld labels exceed 2^59 labels", S, P);
  TT_REQUIRE(sequential == 0 || sequential == 1, "map_instances: sequential = %d is neither 0 (plain) nor 1 (the reference's chained loop)", sequential);
  const unsigned long long a = reinterpret_cast<uintptr_t>(labels_in), b = reinterpret_cast<uintptr_t>(labels_out), n = (unsigned long long)S * P;
  TT_REQUIRE(a + n <= b || b + n <= a, "map_instances: labels_in (%p) and labels_out (%p) overlap within their %llu bytes: the remap is not in place",
             (const void*)labels_in, (void*)labels_out, n);
  TT_REQUIRE(words_ws_bytes >= tt_map_instances_workspace_bytes(S), "map_instances: workspace of %zu bytes, S = %d segments need %zu", words_ws_bytes, S,
             tt_map_instances_workspace_bytes(S));
  TT_REQUIRE(reinterpret_cast<uintptr_t>(cat) % 4 == 0 && reinterpret_cast<uintptr_t>(status) % 4 == 0 && reinterpret_cast<uintptr_t>(words_ws) % 4 == 0,
             "map_instances: cat (%p), status (%p) and words_ws (%p) must be aligned to 4 bytes", (const void*)cat, (void*)status, words_ws);
  hipStream_t s = as_stream(stream);
  unsigned int* words = static_cast<unsigned int*>(words_ws);
  const int rc = ml_presence("map_instances", labels_in, 1, S, P, words, status, s);
  if (rc != TT_OK) return rc;
  TT_CHECK_LAUNCH("map_instances (presence pass)");
  const unsigned bx = ml_blocks(P);
  for (int s0 = 0; s0 < S; s0 += ML_MAX_GRID_Y) {
    const dim3 grid(bx, (unsigned)(S - s0 < ML_MAX_GRID_Y ? S - s0 : ML_MAX_GRID_Y));
    hipLaunchKernelGGL(map_instances_kernel, grid, dim3(ML_THREADS), 0, s, labels_in, labels_out, P, words, cat, sequential, lut_out, status, s0);
  }
  TT_CHECK_LAUNCH("map_instances");
  return TT_OK;
}
