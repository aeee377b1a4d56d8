// Segmented confusion counts (N15): the integer matrices behind every score of evaluation.evaluate_localizations (evaluation.py:250-310:
// one PredsmIoU.compute per frame, per clip or per dataset) and of PredsmIoU.compute_propagation_score (metrics.py:271-346), for ALL
// segments of a batch in one launch.
//
//   counts[s][g][p] += 1 for every element e of segment s (elements s n ... s n + n - 1 of pred and gt) with 0 <= g = gt[e] < Cg,
//   0 <= p = pred[e] < Cp and g != ignore_gt; everything else is skipped.  tt_confusion_counts (label_prop.hip) made rectangular, given
//   an ignore value and a segment axis; that entry and its two kernels are untouched.
//
// Grid: the workgroups along x share ONE segment, the segments ride on gridDim.y (65535 per launch, the entry chunks them), so no
// workgroup straddles two segments.  Two routes (cs_route):
//   LDS     Cg * Cp <= 16384 cells: a u32 histogram per workgroup in LDS (at most 64 KB: two workgroups share a CU's 160 KB), its
//           non-zero cells flushed with one 64-bit global atomic each into counts[s];
//   global  beyond, up to Cg, Cp <= 4096: 64-bit global atomics directly, as confusion_global_kernel.
// Only integer atomics: the result depends neither on the order nor on the grid.
//
// Loads: a thread owns strips of CS_STRIP = 8 consecutive elements.  The strips start where pred's address is 16-byte aligned (a segment
// of odd n starts 2-byte aligned only with int16 labels), so pred comes in 16-byte loads (one per strip at int16, four at int64) and gt in
// four 16-byte loads where its address at that element is 16-byte aligned too - it is whenever both tensors start on 16 bytes - and in
// 8-byte loads otherwise.  The elements before the first strip and after the last one (fewer than 8 each) are read one per thread by the
// segment's first workgroup.  Element offsets are 64-bit throughout.
//
// Runs: evaluation maps are up-sampled token maps, so equal (gt, pred) keys come in runs and the 64 lanes of a wave would add to a
// handful of LDS addresses, which serialises.  A thread merges the equal consecutive keys of its strip in registers into one atomic per
// run.  A build with -DTT_CONFSEG_NO_MERGE (tools/build_variant.sh) is the one-atomic-per-element form it was measured against.
#include "common.hpp"

namespace tt {

constexpr int CS_THREADS = 256;
constexpr int CS_STRIP = 8;                          // consecutive elements of one thread: 16 bytes of int16 labels
constexpr long long CS_TILE = (long long)CS_THREADS * CS_STRIP;   // elements a workgroup takes per step
constexpr int CS_MAX_C = 4096;                       // Cg, Cp: a key gt * Cp + pred stays below 2^24
constexpr int CS_LDS_CELLS = 16384;                  // u32 cells of the LDS histogram: 64 KB
constexpr int CS_MAX_GRID_Y = 65535;                 // segments of one launch
constexpr int CS_MAX_GRID_X = 1024;                  // workgroups of one segment, unless the 2^31 bound below asks for more
constexpr long long CS_MIN_PER_WG = 4 * CS_TILE;     // elements a workgroup walks at least (where the segment has them)
constexpr long long CS_MAX_PER_WG = 1ll << 31;       // ... and at most: an LDS cell is 32 bits (cs_blocks)
constexpr long long CS_MAX_COUNT_CELLS = 1ll << 32;  // S * Cg * Cp the entry takes: 32 GB of counts
#ifdef TT_CONFSEG_NO_MERGE
constexpr bool CS_MERGE = false;
#else
constexpr bool CS_MERGE = true;
#endif

inline int cs_route(int Cg, int Cp) {   // 0 = refused, 1 = LDS, 2 = global
  if (Cg < 1 || Cp < 1 || Cg > CS_MAX_C || Cp > CS_MAX_C) return 0;
  return Cg * Cp <= CS_LDS_CELLS ? 1 : 2;
}

// Workgroups of one segment.  A workgroup takes whole tiles (CS_TILE elements) in a grid-stride loop, so it walks at most
// ceil(ceil(n / CS_TILE) / blocks) tiles.  `per` elements per workgroup: at least CS_MIN_PER_WG and four elements per histogram cell (zeroing
// and flushing the cells is the workgroup's fixed cost), more where the segment would otherwise need over CS_MAX_GRID_X workgroups, and
// NEVER more than CS_MAX_PER_WG = 2^31 - then the grid grows instead.  blocks = ceil(n / per) workgroups therefore walk at most
// per + CS_TILE < 2^32 elements each (the first one a few head and tail elements more): a 32-bit LDS cell cannot wrap.
inline unsigned cs_blocks(long long n, long long cells) {
  long long per = CS_MIN_PER_WG > 4 * cells ? CS_MIN_PER_WG : 4 * cells;
  const long long spread = (n + CS_MAX_GRID_X - 1) / CS_MAX_GRID_X;
  if (per < spread) per = spread;
  if (per > CS_MAX_PER_WG) per = CS_MAX_PER_WG;
  const long long blocks = (n + per - 1) / per;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

typedef long long cs_ll2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void cs_load8(const int16_t* __restrict__ p, long long (&v)[CS_STRIP]) {   // p is 16-byte aligned
  const uint4 q = *reinterpret_cast<const uint4*>(p);
  const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[2 * j] = (short)(w[j] & 0xffffu);
    v[2 * j + 1] = (short)(w[j] >> 16);
  }
}
__device__ __forceinline__ void cs_load8(const int64_t* __restrict__ p, long long (&v)[CS_STRIP]) {   // p is 16-byte aligned
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const cs_ll2 q = *reinterpret_cast<const cs_ll2*>(p + 2 * j);
    v[2 * j] = q.x;
    v[2 * j + 1] = q.y;
  }
}

// the cell of one element, -1 = skipped.  `ignore` is -1 where the caller gave no ignore value: no counted gt equals it.
__device__ __forceinline__ int cs_key(long long t, long long p, int Cg, int Cp, long long ignore) {
  const bool ok = (unsigned long long)t < (unsigned long long)Cg && (unsigned long long)p < (unsigned long long)Cp && t != ignore;
  return ok ? (int)t * Cp + (int)p : -1;
}

template <bool LDS>
__device__ __forceinline__ void cs_add(unsigned int* hist, unsigned long long* __restrict__ out, int key, unsigned int c) {
  if (key < 0) return;
  if (LDS)
    atomicAdd(&hist[key], c);
  else
    atomicAdd(&out[key], (unsigned long long)c);
}

template <typename PredT, bool LDS>
__global__ __launch_bounds__(CS_THREADS) void confusion_segments_kernel(const PredT* __restrict__ pred, const int64_t* __restrict__ gt, long long n,
                                                                        int Cg, int Cp, long long ignore, unsigned long long* __restrict__ counts,
                                                                        int s0) {
  extern __shared__ unsigned int hist[];
  const int cells = Cg * Cp;
  const long long s = (long long)s0 + blockIdx.y;
  const PredT* __restrict__ p = pred + s * n;
  const int64_t* __restrict__ g = gt + s * n;
  unsigned long long* __restrict__ out = counts + s * cells;
  if (LDS) {
    for (int i = threadIdx.x; i < cells; i += CS_THREADS) hist[i] = 0;
    __syncthreads();
  }
  // elements before pred's first 16-byte boundary (p is aligned to its element size: the entry checks)
  constexpr int PER16 = 16 / (int)sizeof(PredT);
  long long head = (long long)((PER16 - (int)((reinterpret_cast<uintptr_t>(p) / sizeof(PredT)) % PER16)) % PER16);
  if (head > n) head = n;
  const long long strips = (n - head) / CS_STRIP;
  const long long tail0 = head + strips * CS_STRIP;   // the first of the n - tail0 < 8 elements after the last strip
  if (blockIdx.x == 0) {
    const int t = (int)threadIdx.x;   // threads 0 ... 7 take the head, threads 8 ... 15 the tail
    long long e = -1;
    if (t < head)
      e = t;
    else if (t >= CS_STRIP && tail0 + (t - CS_STRIP) < n)
      e = tail0 + (t - CS_STRIP);
    if (e >= 0) cs_add<LDS>(hist, out, cs_key(g[e], (long long)p[e], Cg, Cp, ignore), 1u);
  }
  const bool gt16 = (reinterpret_cast<uintptr_t>(g + head) & 15u) == 0;   // uniform over the workgroup
  for (long long i = (long long)blockIdx.x * CS_THREADS + threadIdx.x; i < strips; i += (long long)gridDim.x * CS_THREADS) {
    const long long e0 = head + i * CS_STRIP;
    long long pv[CS_STRIP], tv[CS_STRIP];
    cs_load8(p + e0, pv);
    if (gt16) {
      cs_load8(g + e0, tv);
    } else {
#pragma unroll
      for (int j = 0; j < CS_STRIP; ++j) tv[j] = g[e0 + j];
    }
    int key[CS_STRIP];
#pragma unroll
    for (int j = 0; j < CS_STRIP; ++j) key[j] = cs_key(tv[j], pv[j], Cg, Cp, ignore);
    if (CS_MERGE) {
      int run = key[0];
      unsigned int c = 1;
#pragma unroll
      for (int j = 1; j < CS_STRIP; ++j) {
        if (key[j] == run) {
          ++c;
        } else {
          cs_add<LDS>(hist, out, run, c);
          run = key[j];
          c = 1;
        }
      }
      cs_add<LDS>(hist, out, run, c);
    } else {
#pragma unroll
      for (int j = 0; j < CS_STRIP; ++j) cs_add<LDS>(hist, out, key[j], 1u);
    }
  }
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += CS_THREADS) {
      const unsigned int c = hist[i];
      if (c) atomicAdd(&out[i], (unsigned long long)c);
    }
  }
}

template <typename PredT>
static void cs_launch(int route, dim3 grid, size_t lds, hipStream_t s, const void* pred, const int64_t* gt, long long n, int Cg, int Cp,
                      long long ignore, unsigned long long* counts, int s0) {
  const PredT* p = static_cast<const PredT*>(pred);
  if (route == 1)
    hipLaunchKernelGGL((confusion_segments_kernel<PredT, true>), grid, dim3(CS_THREADS), lds, s, p, gt, n, Cg, Cp, ignore, counts, s0);
  else
    hipLaunchKernelGGL((confusion_segments_kernel<PredT, false>), grid, dim3(CS_THREADS), 0, s, p, gt, n, Cg, Cp, ignore, counts, s0);
}

}  // namespace tt

using namespace tt;

extern "C" int tt_confusion_segments_route(int Cg, int Cp) { return cs_route(Cg, Cp); }

extern "C" int tt_confusion_counts_segments(const void* pred, int pred_dtype, const int64_t* gt, int S, long long n, int Cg, int Cp,
                                            long long ignore_gt, int has_ignore, unsigned long long* counts, tt_stream_t stream) {
  TT_REQUIRE(pred && gt && counts, "confusion_counts_segments: null pointer");
  TT_REQUIRE(pred_dtype == TT_LABELS_I16 || pred_dtype == TT_LABELS_I64, "confusion_counts_segments: pred dtype code %d is neither %d (int16) nor %d (int64)",
             pred_dtype, TT_LABELS_I16, TT_LABELS_I64);
  TT_REQUIRE(S >= 1 && n >= 1, "confusion_counts_segments: S = %d segments of n = %lld elements: need both >= 1", S, n);
  const int route = cs_route(Cg, Cp);
  TT_REQUIRE(route != 0, "confusion_counts_segments: Cg = %d, Cp = %d: need 1 <= Cg, Cp <= %d", Cg, Cp, CS_MAX_C);
  const long long cells = (long long)Cg * Cp;
  TT_REQUIRE((long long)S * cells <= CS_MAX_COUNT_CELLS, "confusion_counts_segments: S = %d matrices of %d x %d are %lld cells, more than the %lld this entry addresses",
             S, Cg, Cp, (long long)S * cells, CS_MAX_COUNT_CELLS);
  TT_REQUIRE(n <= (1ll << 59) / S, "confusion_counts_segments: S = %d segments of n = %lld elements exceed 2^59 elements", S, n);
  const size_t psize = pred_dtype == TT_LABELS_I16 ? 2 : 8;
  TT_REQUIRE(reinterpret_cast<uintptr_t>(pred) % psize == 0 && reinterpret_cast<uintptr_t>(gt) % 8 == 0,
             "confusion_counts_segments: pred (%p) must be aligned to its %zu-byte elements and gt (%p) to 8 bytes", pred, psize, (const void*)gt);
  hipStream_t s = as_stream(stream);
  if (hipMemsetAsync(counts, 0, sizeof(unsigned long long) * (size_t)S * (size_t)cells, s) != hipSuccess) {
    set_error("confusion_counts_segments: memset failed");
    return TT_ELAUNCH;
  }
  const long long ignore = has_ignore ? ignore_gt : -1;   // -1 is never a counted gt
  const size_t lds = route == 1 ? sizeof(unsigned int) * (size_t)cells : 0;
  const unsigned bx = cs_blocks(n, route == 1 ? cells : 0);
  for (int s0 = 0; s0 < S; s0 += CS_MAX_GRID_Y) {   // the segments ride on gridDim.y, at most 65535 per launch
    const dim3 grid(bx, (unsigned)(S - s0 < CS_MAX_GRID_Y ? S - s0 : CS_MAX_GRID_Y));
    if (pred_dtype == TT_LABELS_I16)
      cs_launch<int16_t>(route, grid, lds, s, pred, gt, n, Cg, Cp, ignore, counts, s0);
    else
      cs_launch<int64_t>(route, grid, lds, s, pred, gt, n, Cg, Cp, ignore, counts, s0);
  }
  TT_CHECK_LAUNCH("confusion_counts_segments");
  return TT_OK;
}
