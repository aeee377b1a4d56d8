// Dense nearest-neighbour retrieval (N31): the exact top-k search step, the per-patch label histograms of the memory bank and the
// softmax-weighted label gather - the device side of timetuning_amd/nn_retrieval.py (the "in-context scene understanding" protocol of
// Balazevic et al., 2023).  The similarities themselves are tt_linear_fwd's: queries x bank-block^T, one block at a time.
//
//   tt_topk_merge           per query the k best of (its running list U one block of similarities), under ONE total order:
//                             the larger similarity first, among equal similarities the smaller bank index first.
//                           The empty list is k times (-inf, -1).  A candidate enters only if it precedes the list's last entry in that
//                           order, so a NaN (every comparison false) and a -inf (it ties with the sentinel and -1 is the smaller index)
//                           never enter: the tail of a list that has seen fewer than k finite candidates stays (-inf, -1).  Bank indices
//                           are distinct, so the order is strict and the k best of a multiset are ONE list: the result does not depend on
//                           how the bank was cut into blocks, on the order of the blocks or on the launch geometry.
//                           One wave per query, NN_WAVES queries per workgroup.  The list lives in registers, entry j in lane j, always
//                           sorted; the threshold (entry k - 1) is wave-uniform.  The lanes stream the row in 16-byte loads, NN_UNROLL of
//                           them in flight per lane, and ONE ballot per 1024 similarities asks whether any value reaches the threshold
//                           value - after the first blocks almost none does.  A survivor is inserted at the position a ballot counts
//                           (the entries that precede it are a prefix of the lanes), the entries behind move up one lane.
//                           A row may start at any 4-byte address: the fewer than four similarities in front of the first 16-byte
//                           boundary and behind the last are taken one per lane.
//   tt_patch_label_counts   counts[m][p][c] = pixels of class c in cell p of the g x g grid over map m, valid[m][p] their sum.  One workgroup
//                           per (map, row of cells): a histogram of up to PLC_LDS_INTS / C cells in LDS, integer atomics (exact, order-free),
//                           then plain stores - every output word has one owner.  The pixels are read byte by byte, consecutive threads
//                           consecutive columns: a map may start at any address and this pass runs once per bank image.
//   tt_nn_label_aggregate   out[q] = sum_j w_j labels[idx_j], w = softmax(vals / beta) over the entries with idx >= 0.  One wave per query:
//                           lane j owns entry j (its weight), the lanes then own the classes and walk j = 0 .. k - 1 in order.
//
// No workgroup waits for another, nothing allocates or synchronises; the one status word of tt_patch_label_counts is set on the stream
// in front of its launch.
#include <climits>

#include "common.hpp"

namespace tt {

constexpr int NN_WAVES = 4;                 // queries per workgroup
constexpr int NN_THREADS = kWave * NN_WAVES;
constexpr int NN_UNROLL = 4;                // 16-byte loads in flight per lane
constexpr int NN_MAX_K = 64;

// a precedes b in the total order
__device__ __forceinline__ bool nn_precedes(float av, long long ai, float bv, long long bi) { return av > bv || (av == bv && ai < bi); }

struct NnList {
  float ev;           // this lane's entry
  long long ei;
  float tv;           // entry k - 1: wave-uniform
  long long ti;
  int k, lane;
  unsigned long long kmask;   // lanes 0 .. k - 1

  __device__ __forceinline__ void refresh() {
    tv = __shfl(ev, k - 1, kWave);
    ti = __shfl(ei, k - 1, kWave);
  }
  // Every lane offers one candidate (a NaN is no candidate).  All lanes of the wave must call it.
  __device__ __forceinline__ void offer(float v, long long gi) {
    unsigned long long m = __ballot(nn_precedes(v, gi, tv, ti));
    while (m) {                                       // wave-uniform
      const int s = __ffsll((long long)m) - 1;
      m &= m - 1;
      const float cv = __shfl(v, s, kWave);
      const long long ci = __shfl(gi, s, kWave);
      if (!nn_precedes(cv, ci, tv, ti)) continue;     // the threshold has moved since the ballot
      const int p = __popcll(__ballot(nn_precedes(ev, ei, cv, ci)) & kmask);   // the list is sorted: those are lanes 0 .. p - 1
      const float uv = __shfl_up(ev, 1, kWave);
      const long long ui = __shfl_up(ei, 1, kWave);
      if (lane == p) {
        ev = cv;
        ei = ci;
      } else if (lane > p) {
        ev = uv;
        ei = ui;
      }
      refresh();
    }
  }
};

__global__ __launch_bounds__(NN_THREADS) void topk_merge_kernel(const float* __restrict__ sims, int Q, int Nc, long long ld, long long base,
                                                                float* __restrict__ vals, long long* __restrict__ idx, int k, int init) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long q = (long long)blockIdx.x * NN_WAVES + (threadIdx.x >> 6);
  if (q >= Q) return;   // whole waves leave: no barrier below
  NnList L;
  L.k = k;
  L.lane = lane;
  L.kmask = k == 64 ? ~0ull : (1ull << k) - 1ull;
  L.ev = -INFINITY;
  L.ei = -1;
  if (!init && lane < k) {
    L.ev = vals[q * k + lane];
    L.ei = idx[q * k + lane];
  }
  L.refresh();

  const float* __restrict__ row = sims + q * ld;
  int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) >> 2);
  if (head > Nc) head = Nc;
  const int chunks = (Nc - head) >> 2;
  const int tail0 = head + 4 * chunks;
  {   // fewer than 4 similarities in front of the first 16-byte boundary (lanes 0 .. 2) and behind the last (lanes 8 .. 10)
    int col = -1;
    if (lane < head)
      col = lane;
    else if (lane >= 8 && lane < 12 && tail0 + (lane - 8) < Nc)
      col = tail0 + (lane - 8);
    float v = __builtin_nanf("");
    if (col >= 0) v = row[col];
    L.offer(v, base + (col >= 0 ? col : 0));
  }
  const float4* __restrict__ body = reinterpret_cast<const float4*>(row + head);
  const long long body0 = base + head;
  for (int c0 = 0; c0 < chunks; c0 += kWave * NN_UNROLL) {   // wave-uniform trip count
    float4 x[NN_UNROLL];
#pragma unroll
    for (int u = 0; u < NN_UNROLL; ++u) {
      const int c = c0 + u * kWave + lane;
      const float nan = __builtin_nanf("");
      x[u] = c < chunks ? body[c] : make_float4(nan, nan, nan, nan);
    }
    bool any = false;   // ">=": a value equal to the threshold's may still precede it by its index
#pragma unroll
    for (int u = 0; u < NN_UNROLL; ++u) any = any || x[u].x >= L.tv || x[u].y >= L.tv || x[u].z >= L.tv || x[u].w >= L.tv;
    if (__ballot(any) == 0ull) continue;
#pragma unroll
    for (int u = 0; u < NN_UNROLL; ++u) {
      const long long gi = body0 + 4ll * (c0 + u * kWave + lane);
      L.offer(x[u].x, gi);
      L.offer(x[u].y, gi + 1);
      L.offer(x[u].z, gi + 2);
      L.offer(x[u].w, gi + 3);
    }
  }
  if (lane < k) {
    vals[q * k + lane] = L.ev;
    idx[q * k + lane] = L.ei;
  }
}

// ---- per-patch label histograms ---------------------------------------------------------------------------------------------------------
constexpr int PLC_THREADS = 256;
constexpr int PLC_LDS_INTS = 8192;   // 32 KB: at C = 256 a pass holds 32 cells
constexpr int PLC_MAX_R = 16384;

__global__ __launch_bounds__(PLC_THREADS) void patch_label_counts_kernel(const uint8_t* __restrict__ maps, int R, int g, int C, int ignore,
                                                                         int* __restrict__ counts, int* __restrict__ valid,
                                                                         unsigned int* __restrict__ status) {
  __shared__ int hist[PLC_LDS_INTS];
  const int m = blockIdx.x / g, py = blockIdx.x - m * g;
  const int cell = R / g;
  int per_pass = PLC_LDS_INTS / C;
  if (per_pass > g) per_pass = g;
  const uint8_t* __restrict__ band = maps + ((long long)m * R + (long long)py * cell) * R;
  const long long cell0 = (long long)m * g * g + (long long)py * g;
  bool bad = false;
  for (int px0 = 0; px0 < g; px0 += per_pass) {
    const int np = g - px0 < per_pass ? g - px0 : per_pass;
    const int w = np * cell;
    for (int i = threadIdx.x; i < np * C; i += PLC_THREADS) hist[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < cell * w; i += PLC_THREADS) {   // cell * w <= R * R / g <= 2^28
      const int y = i / w, x = i - y * w;
      const int v = band[(long long)y * R + (long long)px0 * cell + x];
      if (v == ignore) continue;
      if (v >= C) {
        bad = true;
        continue;
      }
      atomicAdd(&hist[(x / cell) * C + v], 1);
    }
    __syncthreads();
    int* __restrict__ o = counts + (cell0 + px0) * C;
    for (int i = threadIdx.x; i < np * C; i += PLC_THREADS) o[i] = hist[i];
    for (int p = threadIdx.x; p < np; p += PLC_THREADS) {
      int s = 0;
      for (int c = 0; c < C; ++c) s += hist[p * C + c];
      valid[cell0 + px0 + p] = s;
    }
    __syncthreads();
  }
  if (bad) atomicMin(status, (unsigned int)m);
}

// ---- the weighted gather ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NN_THREADS) void nn_label_aggregate_kernel(const float* __restrict__ vals, const long long* __restrict__ idx,
                                                                        const float* __restrict__ labels, long long Q, int k, long long N, int C,
                                                                        float beta, float* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long q = (long long)blockIdx.x * NN_WAVES + (threadIdx.x >> 6);
  if (q >= Q) return;
  long long i = -1;
  float v = -INFINITY;
  if (lane < k) {
    i = idx[q * k + lane];
    if (i >= N) i = -1;   // no row of the bank: left out like an empty entry, never read
    if (i >= 0) v = vals[q * k + lane];
  }
  const float vmax = wave_max(v);
  const float e = i >= 0 ? expf((v - vmax) / beta) : 0.f;
  const float sum = wave_sum(e);
  const float wgt = sum > 0.f ? e / sum : 0.f;   // no valid entry: a zero row
  for (int c0 = 0; c0 < C; c0 += kWave) {   // wave-uniform
    const int c = c0 + lane;
    float acc = 0.f;
    for (int j = 0; j < k; ++j) {
      const long long ij = __shfl(i, j, kWave);
      const float wj = __shfl(wgt, j, kWave);
      if (ij >= 0 && c < C) acc = fmaf(wj, labels[ij * C + c], acc);
    }
    if (c < C) out[q * C + c] = acc;
  }
}

}  // namespace tt

using namespace tt;

extern "C" int tt_topk_merge_max_k(void) { return NN_MAX_K; }

extern "C" int tt_topk_merge_shape_ok(long long Q, long long Nc, long long ld, int k) {
  return Q >= 1 && Q <= (long long)INT_MAX && Nc >= 1 && Nc <= (long long)INT_MAX && ld >= Nc && ld <= (1ll << 40) && k >= 1 && k <= NN_MAX_K;
}

extern "C" int tt_topk_merge(const float* sims, long long Q, long long Nc, long long ld, long long base, float* vals, int64_t* idx, int k, int init,
                             tt_stream_t stream) {
  TT_REQUIRE(sims && vals && idx, "topk_merge: null pointer (sims %p, vals %p, idx %p)", (const void*)sims, (void*)vals, (void*)idx);
  TT_REQUIRE(tt_topk_merge_shape_ok(Q, Nc, ld, k),
             "topk_merge: Q = %lld queries, a block of Nc = %lld columns, ld = %lld, k = %d: need 1 <= Q, Nc <= 2^31 - 1, Nc <= ld <= 2^40 and 1 <= k <= %d",
             Q, Nc, ld, k, NN_MAX_K);
  TT_REQUIRE(base >= 0 && base <= (1ll << 62) - Nc, "topk_merge: base = %lld: the block's bank indices must lie in 0 .. 2^62", base);
  TT_REQUIRE(init == 0 || init == 1, "topk_merge: init = %d is neither 0 (merge into the lists) nor 1 (start from empty lists)", init);
  TT_REQUIRE(reinterpret_cast<uintptr_t>(sims) % 4 == 0 && reinterpret_cast<uintptr_t>(vals) % 4 == 0 && reinterpret_cast<uintptr_t>(idx) % 8 == 0,
             "topk_merge: sims (%p) and vals (%p) must be aligned to 4 bytes, idx (%p) to 8", (const void*)sims, (void*)vals, (void*)idx);
  const unsigned blocks = (unsigned)((Q + NN_WAVES - 1) / NN_WAVES);
  hipLaunchKernelGGL(topk_merge_kernel, dim3(blocks), dim3(NN_THREADS), 0, as_stream(stream), sims, (int)Q, (int)Nc, ld, base, vals,
                     reinterpret_cast<long long*>(idx), k, init);
  TT_CHECK_LAUNCH("topk_merge");
  return TT_OK;
}

extern "C" int tt_patch_label_counts_shape_ok(int M, int R, int g, int C) {
  return M >= 1 && g >= 1 && R >= g && R <= PLC_MAX_R && R % g == 0 && C >= 1 && C <= 256 && (long long)M * g <= (long long)INT_MAX &&
         (long long)M * g * g <= (long long)INT_MAX / 256;
}

extern "C" int tt_patch_label_counts(const uint8_t* maps, int M, int R, int g, int C, int ignore, int32_t* counts, int32_t* valid, uint32_t* status,
                                     tt_stream_t stream) {
  TT_REQUIRE(maps && counts && valid && status, "patch_label_counts: null pointer (maps %p, counts %p, valid %p, status %p)", (const void*)maps,
             (void*)counts, (void*)valid, (void*)status);
  TT_REQUIRE(tt_patch_label_counts_shape_ok(M, R, g, C),
             "patch_label_counts: M = %d maps of %d x %d, a grid of g = %d, C = %d classes: need M, g >= 1, g <= R <= %d, R %% g == 0, 1 <= C <= 256 "
             "and M g g <= 2^23",
             M, R, R, g, C, PLC_MAX_R);
  TT_REQUIRE(ignore >= -1 && ignore <= 255, "patch_label_counts: ignore = %d is neither a label value 0 .. 255 nor -1 (none)", ignore);
  TT_REQUIRE(reinterpret_cast<uintptr_t>(counts) % 4 == 0 && reinterpret_cast<uintptr_t>(valid) % 4 == 0 && reinterpret_cast<uintptr_t>(status) % 4 == 0,
             "patch_label_counts: counts (%p), valid (%p) and status (%p) must be aligned to 4 bytes", (void*)counts, (void*)valid, (void*)status);
  hipStream_t s = as_stream(stream);
  if (hipMemsetAsync(status, 0xff, sizeof(uint32_t), s) != hipSuccess) {
    set_error("patch_label_counts: memset failed");
    return TT_ELAUNCH;
  }
  hipLaunchKernelGGL(patch_label_counts_kernel, dim3((unsigned)(M * g)), dim3(PLC_THREADS), 0, s, maps, R, g, C, ignore, counts, valid, status);
  TT_CHECK_LAUNCH("patch_label_counts");
  return TT_OK;
}

extern "C" int tt_nn_label_aggregate_shape_ok(long long Q, int k, long long N, int C) {
  return Q >= 1 && Q <= (long long)INT_MAX * NN_WAVES && k >= 1 && k <= NN_MAX_K && N >= 1 && C >= 1 && C <= (1 << 20) && N <= (1ll << 60) / C &&
         Q <= (1ll << 60) / C;
}

extern "C" int tt_nn_label_aggregate(const float* vals, const int64_t* idx, const float* labels, long long Q, int k, long long N, int C, float beta,
                                     float* out, tt_stream_t stream) {
  TT_REQUIRE(vals && idx && labels && out, "nn_label_aggregate: null pointer (vals %p, idx %p, labels %p, out %p)", (const void*)vals, (const void*)idx,
             (const void*)labels, (void*)out);
  TT_REQUIRE(tt_nn_label_aggregate_shape_ok(Q, k, N, C),
             "nn_label_aggregate: Q = %lld queries, k = %d, a bank of N = %lld rows of C = %d classes: need Q, N >= 1, 1 <= k <= %d, 1 <= C <= 2^20", Q, k,
             N, C, NN_MAX_K);
  TT_REQUIRE(beta > 0.f && beta <= 3.0e38f, "nn_label_aggregate: beta = %g must be a positive finite temperature", (double)beta);
  TT_REQUIRE(reinterpret_cast<uintptr_t>(vals) % 4 == 0 && reinterpret_cast<uintptr_t>(labels) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0 &&
                 reinterpret_cast<uintptr_t>(idx) % 8 == 0,
             "nn_label_aggregate: vals (%p), labels (%p) and out (%p) must be aligned to 4 bytes, idx (%p) to 8", (const void*)vals, (const void*)labels,
             (void*)out, (const void*)idx);
  const unsigned blocks = (unsigned)((Q + NN_WAVES - 1) / NN_WAVES);
  hipLaunchKernelGGL(nn_label_aggregate_kernel, dim3(blocks), dim3(NN_THREADS), 0, as_stream(stream), vals, reinterpret_cast<const long long*>(idx), labels,
                     Q, k, N, C, beta, out);
  TT_CHECK_LAUNCH("nn_label_aggregate");
  return TT_OK;
}
