// k-means for the evaluator (N2, N12, N13): the assignment and the accumulation of a Lloyd iteration, which the reference
// delegates to faiss (faiss.Kmeans(d, k, niter=50, nredo=5, seed=1), clustering.py:39-41,55-57,69-71,108-110; evaluation.py:431-441).
// Two kernel pairs, one contract (kmeans.hpp has the rules, include/timetuning_hip.h the words):
//   resident   every centroid (every sum) in LDS: k * d <= KM_MAXKD floats (tt_kmeans_shape_ok; k = 327 at d = 50).  The assignment is an
//              HBM-bound scan (200 B / point at d = 50) with the problem on gridDim.y: tt_kmeans_assign is one problem of it,
//              tt_kmeans_assign_batched the final index.search(x, 1) of every problem of a batched fit (kmeans_fit.hip).
//   tiled      any k (the over-clustering's faiss.Kmeans(50, 500)): the centroids (the sums) pass through LDS in TILES of tile_k rows,
//              at most 64 KB of them.
// Both compute, per output number, the very same sequence of operations:
//   assignment     km_dist2's chain per (point, centroid) - the tiled kernel writes it out, four side by side and singly - and the
//                  running (best, besti) updated with a strict < in increasing j, across tiles too: the FIRST minimum survives a tile
//                  boundary.
//   accumulation   the partition km_accumulate_blocks, points walked in order, fp32 sums in LDS (tiled: for one tile of clusters; a point
//                  whose label lies outside the tile is skipped), fp64 partials folded in block order.  Deterministic, no atomics.
// Where both pairs take a shape their outputs are equal bit for bit (tests/test_hip_kmeans_tiled.py), so which of them
// clustering.Kmeans runs does not show in its result.
#include "kmeans.hpp"

namespace tt {

// ---- resident assignment: label = argmin_j |x - c_j|^2 (first minimum), optional squared distance, of problem y0 + blockIdx.y.
// A workgroup owns 256 consecutive points: their rows are fetched as one contiguous, fully coalesced block into LDS (row
// stride d | 1, odd, so that the per-thread row reads below are bank-conflict-free), each thread then keeps ITS point in
// registers (d <= 64) and walks the centroids, which every lane reads from LDS at the same address (broadcast).
template <int DREG>
__global__ __launch_bounds__(KM_THREADS) void kmeans_assign_kernel(const float* __restrict__ x, const float* __restrict__ cent,
                                                                   int32_t* __restrict__ labels, float* __restrict__ dist2, long long P, int d,
                                                                   int k, int y0) {
  extern __shared__ float sm[];
  float* cs = sm;                 // [k][d]
  float* xs = sm + k * d;         // [256][ds]
  const int ds = d | 1;
  const size_t b = (size_t)y0 + blockIdx.y;
  x += b * (size_t)P * d;
  cent += b * (size_t)k * d;
  labels += b * (size_t)P;
  if (dist2) dist2 += b * (size_t)P;
  for (int i = threadIdx.x; i < k * d; i += KM_THREADS) cs[i] = cent[i];
  for (long long p0 = (long long)blockIdx.x * KM_THREADS; p0 < P; p0 += (long long)gridDim.x * KM_THREADS) {
    __syncthreads();
    if (DREG > 0) {
      const long long cnt = (P - p0 < KM_THREADS ? P - p0 : KM_THREADS) * d;
      for (long long i = threadIdx.x; i < cnt; i += KM_THREADS) xs[(i / d) * ds + (i % d)] = x[p0 * d + i];
      __syncthreads();
    }
    const long long p = p0 + threadIdx.x;
    if (p >= P) continue;
    const float* xp = DREG > 0 ? xs + threadIdx.x * ds : x + p * d;   // wide rows (d > 64) are read in place
    float xr[DREG > 0 ? DREG : 1];
    if (DREG > 0) {
#pragma unroll
      for (int t = 0; t < DREG; ++t) xr[t] = t < d ? xp[t] : 0.f;
    }
    float best;
    int besti;
    km_nearest<DREG>(xr, xp, cs, d, k, best, besti);
    labels[p] = besti;
    if (dist2) dist2[p] = best;
  }
}

// ---- tiled assignment.  A workgroup owns 256 consecutive points (grid-stride), as kmeans_assign_kernel; DREG as there.
template <int DREG>
__global__ __launch_bounds__(KM_THREADS) void kmeans_assign_tiled_kernel(const float* __restrict__ x, const float* __restrict__ cent,
                                                                         int32_t* __restrict__ labels, float* __restrict__ dist2,
                                                                         long long P, int d, int k, int tile_k) {
  extern __shared__ __attribute__((aligned(16))) float sm[];   // the point tile [256][d | 1], THEN the centroid tile [tile_k][d]
  const int ds = d | 1;
  const bool one_tile = tile_k >= k;
  bool resident = false;   // (wide rows, one tile: the centroids stay in LDS over the stride loop)
  for (long long p0 = (long long)blockIdx.x * KM_THREADS; p0 < P; p0 += (long long)gridDim.x * KM_THREADS) {
    const long long p = p0 + threadIdx.x;
    const bool live = p < P;
    float xr[DREG > 0 ? DREG : 1];
    if (DREG > 0) {
      __syncthreads();   // the previous points' last centroid tile has been read
      const long long cnt = (P - p0 < KM_THREADS ? P - p0 : KM_THREADS) * d;
      for (long long i = threadIdx.x; i < cnt; i += KM_THREADS) sm[(i / d) * ds + (i % d)] = x[p0 * d + i];
      __syncthreads();
      const float* xs = sm + threadIdx.x * ds;
#pragma unroll
      for (int t = 0; t < DREG; ++t) xr[t] = (live && t < d) ? xs[t] : 0.f;
    }
    const float* xp = x + (live ? p : 0) * d;   // wide rows (d > 64) are read in place
    float best = INFINITY;
    int besti = 0;
    for (int j0 = 0; j0 < k; j0 += tile_k) {
      const int tk = k - j0 < tile_k ? k - j0 : tile_k;
      if (!resident) {
        __syncthreads();   // the points are in registers / the previous tile has been read
        const float* src = cent + (size_t)j0 * d;
        for (int i = threadIdx.x; i < tk * d; i += KM_THREADS) sm[i] = src[i];
        __syncthreads();
        resident = DREG == 0 && one_tile;
      }
      if (!live) continue;
      int j = 0;
      for (; j + 4 <= tk; j += 4) {   // four centroids at a time: four independent accumulators, each km_dist2's chain
        const float *c0 = sm + j * d, *c1 = c0 + d, *c2 = c1 + d, *c3 = c2 + d;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        if (DREG > 0) {
#pragma unroll
          for (int t = 0; t < DREG; ++t)
            if (t < d) {
              const float f0 = xr[t] - c0[t], f1 = xr[t] - c1[t], f2 = xr[t] - c2[t], f3 = xr[t] - c3[t];
              s0 += f0 * f0;
              s1 += f1 * f1;
              s2 += f2 * f2;
              s3 += f3 * f3;
            }
        } else {
          for (int t = 0; t < d; ++t) {
            const float xv = xp[t];
            const float f0 = xv - c0[t], f1 = xv - c1[t], f2 = xv - c2[t], f3 = xv - c3[t];
            s0 += f0 * f0;
            s1 += f1 * f1;
            s2 += f2 * f2;
            s3 += f3 * f3;
          }
        }
        if (s0 < best) { best = s0; besti = j0 + j; }
        if (s1 < best) { best = s1; besti = j0 + j + 1; }
        if (s2 < best) { best = s2; besti = j0 + j + 2; }
        if (s3 < best) { best = s3; besti = j0 + j + 3; }
      }
      for (; j < tk; ++j) {   // km_dist2's chain, written out: through the call the <64> kernel came out longer and measured slower
        const float* c = sm + j * d;
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
        if (s < best) { best = s; besti = j0 + j; }
      }
    }
    if (live) {
      labels[p] = besti;
      if (dist2) dist2[p] = best;
    }
  }
}

// ---- resident accumulation: per-block sums[k][d] (fp32 in LDS over the block's pts_per_block points, then fp64 partials)
__global__ __launch_bounds__(KM_THREADS) void kmeans_accumulate_stage1(const float* __restrict__ x, const int32_t* __restrict__ labels,
                                                                       double* __restrict__ part_sums, long long* __restrict__ part_cnt,
                                                                       long long P, int d, int k, long long pts_per_block) {
  extern __shared__ float acc[];  // [k][d] sums, then [k] counts
  float* cnt = acc + k * d;
  for (int i = threadIdx.x; i < k * d + k; i += KM_THREADS) acc[i] = 0.f;
  __syncthreads();
  const long long p0 = (long long)blockIdx.x * pts_per_block;
  const long long p1 = p0 + pts_per_block < P ? p0 + pts_per_block : P;
  // thread t owns feature columns t, t + 256, ... and walks the block's points in order: no atomics, fixed summation order
  for (int t = threadIdx.x; t < d; t += KM_THREADS)
    for (long long p = p0; p < p1; ++p) acc[labels[p] * d + t] += x[p * d + t];
  if (threadIdx.x == 0)
    for (long long p = p0; p < p1; ++p) cnt[labels[p]] += 1.f;
  __syncthreads();
  for (int i = threadIdx.x; i < k * d; i += KM_THREADS) part_sums[(long long)blockIdx.x * k * d + i] = (double)acc[i];
  for (int i = threadIdx.x; i < k; i += KM_THREADS) part_cnt[(long long)blockIdx.x * k + i] = (long long)cnt[i];
}

// ---- tiled accumulation: workgroup (b, y) sums the points of block b whose label lies in tile tile0 + y.  Per (cluster, column) the
// additions are kmeans_accumulate_stage1's: the block's points in order, fp32.
__global__ __launch_bounds__(KM_THREADS) void kmeans_accumulate_tiled_stage1(const float* __restrict__ x, const int32_t* __restrict__ labels,
                                                                             double* __restrict__ part_sums, long long* __restrict__ part_cnt,
                                                                             long long P, int d, int k, int tile_k, int tile0,
                                                                             long long pts_per_block) {
  extern __shared__ __attribute__((aligned(16))) float acc[];   // [tile_k][d] sums, then [tile_k] counts
  int* cnt = reinterpret_cast<int*>(acc + tile_k * d);
  const int a = (tile0 + (int)blockIdx.y) * tile_k;              // the tile's first cluster (a < k: the host launches ceil(k / tile_k) tiles)
  const int tk = k - a < tile_k ? k - a : tile_k;
  for (int i = threadIdx.x; i < tk * d; i += KM_THREADS) acc[i] = 0.f;
  for (int i = threadIdx.x; i < tk; i += KM_THREADS) cnt[i] = 0;
  __syncthreads();
  const long long p0 = (long long)blockIdx.x * pts_per_block;
  const long long p1 = p0 + pts_per_block < P ? p0 + pts_per_block : P;
  // thread t owns feature columns t, t + 256, ... and walks the block's points in order: no atomics, fixed summation order
  for (int t = threadIdx.x; t < d; t += KM_THREADS)
    for (long long p = p0; p < p1; ++p) {
      const unsigned l = (unsigned)labels[p] - (unsigned)a;
      if (l < (unsigned)tk) acc[l * d + t] += x[p * d + t];
    }
  if (threadIdx.x == 0)
    for (long long p = p0; p < p1; ++p) {
      const unsigned l = (unsigned)labels[p] - (unsigned)a;
      if (l < (unsigned)tk) cnt[l] += 1;
    }
  __syncthreads();
  double* ps = part_sums + ((long long)blockIdx.x * k + a) * d;
  long long* pc = part_cnt + (long long)blockIdx.x * k + a;
  for (int i = threadIdx.x; i < tk * d; i += KM_THREADS) ps[i] = (double)acc[i];
  for (int i = threadIdx.x; i < tk; i += KM_THREADS) pc[i] = (long long)cnt[i];
}

// ---- the fold of both accumulations: block order, fp64
__global__ __launch_bounds__(KM_THREADS) void kmeans_accumulate_stage2(const double* __restrict__ part_sums, const long long* __restrict__ part_cnt,
                                                                       double* __restrict__ sums, long long* __restrict__ counts, long long kd,
                                                                       int k, int blocks) {
  const long long i = (long long)blockIdx.x * KM_THREADS + threadIdx.x;
  if (i < kd) {
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += part_sums[(long long)b * kd + i];
    sums[i] = s;
  }
  if (i < k) {
    long long c = 0;
    for (int b = 0; b < blocks; ++b) c += part_cnt[(long long)b * k + i];
    counts[i] = c;
  }
}

// Both resident assignment entries, after their own refusals: B problems of P points, problem b at x + b P d with its centroids at
// centroids + b k d and its outputs at labels + b P (dist2 + b P).
static int launch_assign(const char* who, const float* x, const float* centroids, int32_t* labels, float* dist2, int B, long long P, int d,
                         int k, tt_stream_t stream) {
  static const bool lds_attr_set = km_raise_lds(KM_ROUTES(kmeans_assign_kernel));   // the centroids and the d <= 64 tile's points, 128 KB together
  TT_REQUIRE(lds_attr_set, "%s: could not raise the dynamic LDS limit", who);
  const size_t lds = km_assign_lds(d, k);
  hipStream_t s = as_stream(stream);
  for (int y0 = 0; y0 < B; y0 += KM_MAX_GRID_Y) {   // the problems ride on gridDim.y, at most 65535 per launch
    const dim3 grid(km_assign_blocks(P), (unsigned)(B - y0 < KM_MAX_GRID_Y ? B - y0 : KM_MAX_GRID_Y));
    KM_LAUNCH_ROUTE(kmeans_assign_kernel, d, grid, lds, s, x, centroids, labels, dist2, P, d, k, y0);
  }
  TT_CHECK_LAUNCH(who);
  return TT_OK;
}

// the workspace of an accumulation as its two stages see it: fp64 partial sums [blocks][k][d], then the counts [blocks][k]
struct Partials {
  double* sums;
  long long* cnt;
};
static Partials carve_partials(void* workspace, int blocks, long long kd) {
  double* sums = static_cast<double*>(workspace);
  return {sums, reinterpret_cast<long long*>(sums + (size_t)blocks * kd)};
}
static void launch_fold(Partials part, double* sums, long long* counts, long long kd, int k, int blocks, hipStream_t s) {
  hipLaunchKernelGGL(kmeans_accumulate_stage2, dim3((unsigned)((kd + KM_THREADS - 1) / KM_THREADS)), dim3(KM_THREADS), 0, s, part.sums, part.cnt, sums,
                     counts, kd, k, blocks);
}

// tile_k as the caller gave it -> the tile the kernels run (0 = the default); -1 = refused (the message is set)
static int resolve_tile(const char* who, int d, int k, int tile_k) {
  const int most = km_tile_default(d);
  if (tile_k < 0 || tile_k > most) {
    set_error("%s: tile_k = %d is outside 1 ... %d, the centroids of d = %d columns that fill 64 KB (0 = that default)", who, tile_k, most, d);
    return -1;
  }
  return tile_k == 0 ? most : tile_k;
}

}  // namespace tt

using namespace tt;

// ---- the resident pair

extern "C" int tt_kmeans_shape_ok(int d, int k) { return km_shape_ok(d, k) ? 1 : 0; }
extern "C" int tt_kmeans_assign_route(int d) { return km_assign_route(d); }

extern "C" int tt_kmeans_assign(const float* x, const float* centroids, int32_t* labels, float* dist2, long long P, int d, int k,
                                tt_stream_t stream) {
  TT_REQUIRE(x && centroids && labels && P > 0 && d > 0 && k > 0, "kmeans_assign: bad arguments");
  TT_REQUIRE((long long)k * d <= KM_MAXKD, "kmeans_assign: k * d = %lld exceeds %d", (long long)k * d, KM_MAXKD);
  TT_REQUIRE(km_shape_ok(d, k), "kmeans_assign: k = %d, d = %d need %zu bytes of LDS (at most %zu)", k, d, km_assign_lds(d, k), KM_MAX_LDS);
  return launch_assign("kmeans_assign", x, centroids, labels, dist2, 1, P, d, k, stream);
}

extern "C" int tt_kmeans_assign_batched(const float* x, const float* centroids, int32_t* labels, float* dist2, int B, long long N, int d, int k,
                                        tt_stream_t stream) {
  TT_REQUIRE(x && centroids && labels, "kmeans_assign_batched: null pointer");
  TT_REQUIRE(km_shape_ok(d, k), "kmeans_assign_batched: k = %d, d = %d is beyond what kmeans_assign takes (k * d <= %d, %zu bytes of LDS within %zu)",
             k, d, KM_MAXKD, d > 0 && k > 0 ? km_assign_lds(d, k) : (size_t)0, KM_MAX_LDS);
  TT_REQUIRE(B >= 1 && N >= 1, "kmeans_assign_batched: B = %d problems of N = %lld points: need both >= 1", B, N);
  return launch_assign("kmeans_assign_batched", x, centroids, labels, dist2, B, N, d, k, stream);
}

extern "C" size_t tt_kmeans_accumulate_workspace_bytes(long long P, int d, int k) { return km_accumulate_workspace_bytes(P, d, k); }

extern "C" int tt_kmeans_accumulate(const float* x, const int32_t* labels, double* sums, long long* counts, long long P, int d, int k,
                                    void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  TT_REQUIRE(x && labels && sums && counts && workspace && P > 0 && d > 0 && k > 0, "kmeans_accumulate: bad arguments");
  TT_REQUIRE((long long)k * d <= KM_MAXKD, "kmeans_accumulate: k * d = %lld exceeds %d", (long long)k * d, KM_MAXKD);
  TT_REQUIRE(km_shape_ok(d, k), "kmeans_accumulate: k = %d, d = %d is beyond what kmeans_assign takes (%zu bytes of LDS, at most %zu)", k, d,
             km_assign_lds(d, k), KM_MAX_LDS);
  TT_REQUIRE(workspace_bytes >= km_accumulate_workspace_bytes(P, d, k), "kmeans_accumulate: workspace too small");
  static const bool lds_attr_set = km_raise_lds({KM_KERNEL(kmeans_accumulate_stage1)});
  TT_REQUIRE(lds_attr_set, "kmeans_accumulate: could not raise the dynamic LDS limit");
  hipStream_t s = as_stream(stream);
  const int blocks = km_accumulate_blocks(P);
  const long long ppb = (P + blocks - 1) / blocks;
  const Partials part = carve_partials(workspace, blocks, (long long)k * d);
  hipLaunchKernelGGL(kmeans_accumulate_stage1, dim3(blocks), dim3(KM_THREADS), sizeof(float) * (k * d + k), s, x, labels, part.sums, part.cnt, P, d,
                     k, ppb);
  launch_fold(part, sums, counts, (long long)k * d, k, blocks, s);
  TT_CHECK_LAUNCH("kmeans_accumulate");
  return TT_OK;
}

// ---- the tiled pair

extern "C" int tt_kmeans_tiled_shape_ok(int d, int k) { return km_tiled_shape_ok(d, k) ? 1 : 0; }
extern "C" int tt_kmeans_tile_centroids(int d) { return km_tile_default(d); }

extern "C" int tt_kmeans_assign_tiled(const float* x, const float* centroids, int32_t* labels, float* dist2, long long P, int d, int k,
                                      int tile_k, tt_stream_t stream) {
  TT_REQUIRE(x && centroids && labels && P > 0, "kmeans_assign_tiled: bad arguments");
  TT_REQUIRE(km_tiled_shape_ok(d, k), "kmeans_assign_tiled: k = %d, d = %d: need 1 <= d <= %d, k >= 1, k * d < 2^31", k, d, KM_MAXD);
  const int tile = resolve_tile("kmeans_assign_tiled", d, k, tile_k);
  if (tile < 0) return TT_EINVAL;
  const size_t lds = km_assign_tiled_lds(d, tile);
  TT_REQUIRE(lds <= KM_MAX_LDS, "kmeans_assign_tiled: %zu bytes of LDS (at most %zu)", lds, KM_MAX_LDS);
  static const bool lds_attr_set = km_raise_lds(KM_ROUTES(kmeans_assign_tiled_kernel));   // up to 65 KB (d = 64: the point tile)
  TT_REQUIRE(lds_attr_set, "kmeans_assign_tiled: could not raise the dynamic LDS limit");
  KM_LAUNCH_ROUTE(kmeans_assign_tiled_kernel, d, dim3(km_assign_blocks(P)), lds, as_stream(stream), x, centroids, labels, dist2, P, d, k, tile);
  TT_CHECK_LAUNCH("kmeans_assign_tiled");
  return TT_OK;
}

// The workspace of tt_kmeans_accumulate: the tiles of one call write disjoint rows of it, so the size does not depend on tile_k (the
// argument is part of the query for symmetry with the launch).
extern "C" size_t tt_kmeans_accumulate_tiled_workspace_bytes(long long P, int d, int k, int tile_k) {
  (void)tile_k;
  return km_tiled_shape_ok(d, k) ? km_accumulate_workspace_bytes(P, d, k) : 0;
}

extern "C" int tt_kmeans_accumulate_tiled(const float* x, const int32_t* labels, double* sums, long long* counts, long long P, int d, int k,
                                          int tile_k, void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  TT_REQUIRE(x && labels && sums && counts && workspace && P > 0, "kmeans_accumulate_tiled: bad arguments");
  TT_REQUIRE(km_tiled_shape_ok(d, k), "kmeans_accumulate_tiled: k = %d, d = %d: need 1 <= d <= %d, k >= 1, k * d < 2^31", k, d, KM_MAXD);
  const int tile = resolve_tile("kmeans_accumulate_tiled", d, k, tile_k);
  if (tile < 0) return TT_EINVAL;
  TT_REQUIRE(workspace_bytes >= km_accumulate_workspace_bytes(P, d, k), "kmeans_accumulate_tiled: workspace too small");
  const size_t lds = km_accumulate_tiled_lds(d, tile);
  TT_REQUIRE(lds <= KM_MAX_LDS, "kmeans_accumulate_tiled: %zu bytes of LDS (at most %zu)", lds, KM_MAX_LDS);
  static const bool lds_attr_set = km_raise_lds({KM_KERNEL(kmeans_accumulate_tiled_stage1)});
  TT_REQUIRE(lds_attr_set, "kmeans_accumulate_tiled: could not raise the dynamic LDS limit");
  hipStream_t s = as_stream(stream);
  const int blocks = km_accumulate_blocks(P);
  const long long ppb = (P + blocks - 1) / blocks;
  const long long kd = (long long)k * d;
  const Partials part = carve_partials(workspace, blocks, kd);
  const int tiles = (k + tile - 1) / tile;   // they ride on gridDim.y, at most 65535 per launch
  for (int t0 = 0; t0 < tiles; t0 += KM_MAX_GRID_Y) {
    const int ny = tiles - t0 < KM_MAX_GRID_Y ? tiles - t0 : KM_MAX_GRID_Y;
    hipLaunchKernelGGL(kmeans_accumulate_tiled_stage1, dim3(blocks, ny), dim3(KM_THREADS), lds, s, x, labels, part.sums, part.cnt, P, d, k, tile, t0,
                       ppb);
  }
  launch_fold(part, sums, counts, kd, k, blocks, s);
  TT_CHECK_LAUNCH("kmeans_accumulate_tiled");
  return TT_OK;
}
