// The rules every k-means kernel shares (kmeans.hip: the resident and the tiled pair; kmeans_fit.hip: the fused fit), stated ONCE.
// The three must agree bit for bit wherever more than one of them takes a shape (include/timetuning_hip.h, "the k-means contract"):
// they do because the shape rules and the partition of the points below are the only statement of each, and the distance chain is
// km_dist2 everywhere but in kmeans_assign_tiled_kernel, which writes the same chain out (its 4-wide block and its tail).
#pragma once
#include <initializer_list>

#include "common.hpp"

namespace tt {

constexpr int KM_THREADS = 256;                // threads of an assignment / accumulation workgroup: one point each in the assignment
constexpr int KM_MAXD = 1024;                  // feature columns the tiled pair takes
constexpr int KM_MAXKD = 16384;                // k * d floats of centroids the resident pair holds in LDS (64 KB; k = 300 at d = 50 fits)
constexpr int KM_TILE_FLOATS = KM_MAXKD;       // floats of centroids (of sums) one tile of the tiled pair holds: what the resident pair holds
constexpr size_t KM_MAX_LDS = 128 * 1024;      // dynamic LDS a k-means workgroup may ask for (km_raise_lds)
constexpr int KM_MAX_GRID_Y = 65535;           // problems / tiles of one launch (they ride on gridDim.y)

// ---- the resident pair.  The (d, k) BOTH entries take - clustering.Kmeans calls one after the other, so they share the rule:
//   k * d <= KM_MAXKD floats of centroids (the assignment's LDS copy; the accumulation's sums, plus k counts: at most 128 KB at d = 1);
//   d <= 64: the assignment's tile of 256 points (row stride d | 1) shares the LDS - k * d + 256 (d | 1) floats <= 128 KB.  That binds
//   at d = 64 only: the tile takes 65 KB, which leaves 63 KB of centroids, k <= 252.
// The assignment kernel by d (both pairs): 16 / 64 = the point's row in that many registers (tile in LDS), 0 = wider rows read in place
inline int km_assign_route(int d) { return d <= 16 ? 16 : (d <= 64 ? 64 : 0); }
inline size_t km_point_tile_floats(int d) { return km_assign_route(d) ? (size_t)KM_THREADS * (d | 1) : 0; }
inline size_t km_assign_lds(int d, int k) { return sizeof(float) * ((size_t)k * d + km_point_tile_floats(d)); }
inline bool km_shape_ok(int d, int k) { return d > 0 && k > 0 && (long long)k * d <= KM_MAXKD && km_assign_lds(d, k) <= KM_MAX_LDS; }

// workgroups of an assignment (both pairs): one per 256 points, at most 4096 - beyond 4096 x 256 points a workgroup strides
inline unsigned km_assign_blocks(long long P) {
  const long long b = (P + KM_THREADS - 1) / KM_THREADS;
  return (unsigned)(b > 4096 ? 4096 : b);
}

// ---- the partition of the points of EVERY accumulation (resident, tiled, fused): a different one changes the sums' bits.
// 128 points per block keep the fp32 LDS sums short - up to 4096 blocks: beyond P = 524 288 a block takes ceil(P / 4096) points
// (269 at the 1.1 M points of the CBFE over-clustering; the sums stay within the fp32 class there: the sweep holds them to 1e-5)
inline int km_accumulate_blocks(long long P) {
  long long b = (P + 127) / 128;
  return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}
// one fp64 partial per (block, cluster, column) and one count per (block, cluster): the workspace of both accumulations
inline size_t km_accumulate_workspace_bytes(long long P, int d, int k) {
  return (size_t)km_accumulate_blocks(P) * ((size_t)k * d * sizeof(double) + (size_t)k * sizeof(long long));
}

// ---- the tiled pair: any k, the centroids (the sums) pass through LDS tile_k rows at a time
inline bool km_tiled_shape_ok(int d, int k) { return d >= 1 && d <= KM_MAXD && k >= 1 && (long long)k * d < (1LL << 31); }
inline int km_tile_default(int d) { return d >= 1 && d <= KM_MAXD ? KM_TILE_FLOATS / d : 0; }
// The tile of 256 points (d <= 64) and the centroid tile SHARE the LDS: the points are in registers before the first centroid tile
// overwrites them.  At most 256 * 65 floats = 65 KB (d = 64), so two workgroups fit a CU's 160 KB.
inline size_t km_assign_tiled_lds(int d, int tile_k) {
  const size_t cent = (size_t)tile_k * d, pts = km_point_tile_floats(d);
  return sizeof(float) * (cent > pts ? cent : pts);
}
// sums [tile_k][d] and as many counts: at most 128 KB (d = 1: KM_TILE_FLOATS sums and as many counts)
inline size_t km_accumulate_tiled_lds(int d, int tile_k) { return sizeof(float) * ((size_t)tile_k * d + tile_k); }

// ---- launching.  KM_ROUTES(kernel): the three instantiations of an assignment kernel template, for km_raise_lds;
// KM_LAUNCH_ROUTE: the one of them that km_assign_route(d) names.
inline bool km_raise_lds(std::initializer_list<const void*> kernels) {   // beyond the 64 KB a kernel gets unasked
  bool ok = true;
  for (const void* f : kernels) ok = ok && hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)KM_MAX_LDS) == hipSuccess;
  return ok;
}
#define KM_KERNEL(...) reinterpret_cast<const void*>(&__VA_ARGS__)
#define KM_ROUTES(kernel) {KM_KERNEL(kernel<16>), KM_KERNEL(kernel<64>), KM_KERNEL(kernel<0>)}
#define KM_LAUNCH_ROUTE(kernel, d, grid, lds, stream, ...)                                                 \
  do {                                                                                                     \
    const int route__ = ::tt::km_assign_route(d);                                                          \
    if (route__ == 16)                                                                                     \
      hipLaunchKernelGGL((kernel<16>), grid, dim3(::tt::KM_THREADS), lds, stream, __VA_ARGS__);            \
    else if (route__ == 64)                                                                                \
      hipLaunchKernelGGL((kernel<64>), grid, dim3(::tt::KM_THREADS), lds, stream, __VA_ARGS__);            \
    else                                                                                                   \
      hipLaunchKernelGGL((kernel<0>), grid, dim3(::tt::KM_THREADS), lds, stream, __VA_ARGS__);             \
  } while (0)

// ---- the distance chain: one fp32 accumulator per (point, centroid), the columns in increasing order (s += df * df contracts to one
// fma; every kernel is built with the same flags).  DREG > 0: the row is in the registers xr (d <= DREG); DREG == 0: read in place from xp.
template <int DREG>
__device__ __forceinline__ float km_dist2(const float* xr, const float* xp, const float* c, int d) {
  float s = 0.f;
  if (DREG > 0) {
#pragma unroll
    for (int t = 0; t < DREG; ++t)
      if (t < d) {
        const float df = xr[t] - c[t];
        s += df * df;
      }
  } else {
    for (int t = 0; t < d; ++t) {
      const float df = xp[t] - c[t];
      s += df * df;
    }
  }
  return s;
}

// The nearest of the k centroids cs [k][d] to one point: the FIRST minimum, by a strict < in increasing j from best = INFINITY, besti = 0
template <int DREG>
__device__ __forceinline__ void km_nearest(const float* xr, const float* __restrict__ xp, const float* cs, int d, int k, float& best_out,
                                           int& besti_out) {
  float best = INFINITY;
  int besti = 0;
  for (int j = 0; j < k; ++j) {
    const float* c = cs + j * d;
    float s = km_dist2<DREG>(xr, xp, c, d);
    if (s < best) {
      best = s;
      besti = j;
    }
  }
  best_out = best;
  besti_out = besti;
}

// ---- faiss' split of the empty clusters, clustering.Kmeans._split_empty statement for statement, run by ONE wave on a fit's centroids
// cs [k][d] and counts cnt [k] after the update - a workgroup's LDS copies (the fused fit, kmeans_fit.hip) or its rows of global memory
// (the device loop, kmeans.hip); the host restatement is clustering.split_empty_from_table.  draws holds the first n_draws values of
// numpy.random.RandomState(1234).random_sample(): the host re-creates that generator at every call, so every call reads a prefix of
// one sequence and the index starts at 0 here.  Lane 0 decides - it alone reads and writes the counts and the table - and hands each
// decision to the wave by a shuffle; lane j owns columns j, j + 64, ... (d <= KM_MAXD) of every row, so no lane reads what another
// wrote, and a column's sign goes by the lane's parity.  Trip counts: k clusters, at most 64 k + 1 tries each and at most n_draws draws
// in all.  False: a draw beyond the table was needed (cs and cnt are then part-way through the call and must not be used).
__device__ __forceinline__ bool kf_split_empty(float* cs, int* cnt, int n, int d, int k, const double* __restrict__ draws, int n_draws,
                                               int lane) {
  constexpr int SKIP = -1, STOP = -2, SHORT = -3;
  const float s = (lane & 1) ? 1.0f - 1.0f / 1024.0f : 1.0f + 1.0f / 1024.0f;   // both, and 2 - s, are exact in fp32
  int next = 0;   // lane 0's index of the next draw
  for (int ci = 0; ci < k; ++ci) {
    int dec = SKIP;   // the donor cj >= 0, or one of the three above
    if (lane == 0 && cnt[ci] == 0) {
      int most = cnt[0], arg = 0;   // the first arg-max (numpy.argmax)
      for (int j = 1; j < k; ++j)
        if (cnt[j] > most) most = cnt[j], arg = j;
      if (n <= k || most <= 1) {
        dec = STOP;
      } else {
        const double span = (double)(n - k);
        int cj = 0;
        long long tries = 0;   // (64 k + 1 of them: beyond an int at the largest k the device loop takes)
        for (;;) {
          if (next >= n_draws) {
            dec = SHORT;
            break;
          }
          if (draws[next++] < (double)(cnt[cj] - 1) / span) {
            dec = cj;
            break;
          }
          cj = cj + 1 == k ? 0 : cj + 1;
          if (++tries > 64LL * k) {   // vanishing acceptance: the largest cluster
            dec = arg;
            break;
          }
        }
      }
    }
    dec = __shfl(dec, 0, 64);
    if (dec == STOP) break;
    if (dec == SHORT) return false;
    if (dec == SKIP) continue;
    for (int t = lane; t < d; t += 64) {   // single fp32 products, the new row from the OLD donor row
      const float old = cs[(size_t)dec * d + t];
      cs[(size_t)ci * d + t] = old * s;
      cs[(size_t)dec * d + t] = old * (2.0f - s);
    }
    if (lane == 0) {
      cnt[ci] = cnt[dec] / 2;
      cnt[dec] -= cnt[ci];
    }
  }
  return true;
}

}  // namespace tt
