// k-means beyond the LDS limit (N12): the assignment and the accumulation of cluster.hip for centroid sets that do
// not fit in LDS - the reference's over-clustering runs faiss.Kmeans(50, 500) (clustering.py:39-41,55-57,69-71,108-110; evaluation.py:431-441),
// and cluster.hip's resident pair stops at k * d = 16384 floats (k = 327 at d = 50).
//
// Both kernels walk the centroids in TILES of tile_k rows (at most 64 KB of them) staged through LDS, and both compute, per output
// number, the very sequence of operations of their resident counterpart:
//   assignment     one fp32 accumulator per (point, centroid), columns in increasing order, df = x - c; s += df * df (contracted to
//                  an fma exactly as in cluster.hip: same compiler flags); the running (best, besti) is updated with a strict <
//                  in increasing j, across tiles too, so the FIRST minimum survives a tile boundary.
//   accumulation   the point partition of cluster.hip (accumulate_blocks), points walked in order, fp32 sums in LDS for one tile of
//                  clusters (a point whose label lies outside the tile is skipped), fp64 partials folded in block order.
// Where both pairs take a shape their outputs are equal bit for bit (tests/test_hip_kmeans_tiled.py), so which of them
// clustering.Kmeans runs does not show in its result.
#include "common.hpp"

namespace tt {

constexpr int KT_THREADS = 256;
constexpr int KT_MAXD = 1024;                // feature columns (cluster.hip's CL_MAXD)
constexpr int KT_TILE_FLOATS = 16384;        // floats of centroids (of sums) one tile holds: 64 KB
constexpr size_t KT_MAX_LDS = 128 * 1024;    // the dynamic LDS cluster.hip's kernels ask for; the kernels here stay below it
constexpr int KT_MAX_GRID_Y = 65535;

static bool kt_shape_ok(int d, int k) { return d >= 1 && d <= KT_MAXD && k >= 1 && (long long)k * d < (1LL << 31); }
static int kt_tile_default(int d) { return d >= 1 && d <= KT_MAXD ? KT_TILE_FLOATS / d : 0; }
static int kt_assign_route(int d) { return d <= 16 ? 16 : (d <= 64 ? 64 : 0); }   // cluster.hip's km_assign_route
// The tile of 256 points (d <= 64, row stride d | 1) and the centroid tile SHARE the LDS: the points are in registers before the
// first centroid tile overwrites them.  At most 256 * 65 floats = 65 KB (d = 64), so two workgroups fit a CU's 160 KB.
static size_t kt_assign_lds(int d, int tile_k) {
  const size_t cent = (size_t)tile_k * d, pts = kt_assign_route(d) ? (size_t)KT_THREADS * (d | 1) : 0;
  return sizeof(float) * (cent > pts ? cent : pts);
}
static int kt_accumulate_blocks(long long P) {   // cluster.hip's accumulate_blocks: the SAME partition, or the sums' bits differ
  long long b = (P + 127) / 128;
  return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

// ---- tiled assignment.  A workgroup owns 256 consecutive points (grid-stride), as kmeans_assign_kernel; DREG as there.
template <int DREG>
__global__ __launch_bounds__(KT_THREADS) void kmeans_assign_tiled_kernel(const float* __restrict__ x, const float* __restrict__ cent,
                                                                         int32_t* __restrict__ labels, float* __restrict__ dist2,
                                                                         long long P, int d, int k, int tile_k) {
  extern __shared__ __attribute__((aligned(16))) float sm[];   // the point tile [256][d | 1], THEN the centroid tile [tile_k][d]
  const int ds = d | 1;
  const bool one_tile = tile_k >= k;
  bool resident = false;   // (wide rows, one tile: the centroids stay in LDS over the stride loop)
  for (long long p0 = (long long)blockIdx.x * KT_THREADS; p0 < P; p0 += (long long)gridDim.x * KT_THREADS) {
    const long long p = p0 + threadIdx.x;
    const bool live = p < P;
    float xr[DREG > 0 ? DREG : 1];
    if (DREG > 0) {
      __syncthreads();   // the previous points' last centroid tile has been read
      const long long cnt = (P - p0 < KT_THREADS ? P - p0 : KT_THREADS) * d;
      for (long long i = threadIdx.x; i < cnt; i += KT_THREADS) sm[(i / d) * ds + (i % d)] = x[p0 * d + i];
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
        for (int i = threadIdx.x; i < tk * d; i += KT_THREADS) sm[i] = src[i];
        __syncthreads();
        resident = DREG == 0 && one_tile;
      }
      if (!live) continue;
      int j = 0;
      for (; j + 4 <= tk; j += 4) {   // four centroids at a time: four independent accumulators, each summed in column order
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
      for (; j < tk; ++j) {
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

// ---- tiled accumulation: workgroup (b, y) sums the points of block b whose label lies in tile tile0 + y.  Per (cluster, column) the
// additions are kmeans_accumulate_stage1's: the block's points in order, fp32.
__global__ __launch_bounds__(KT_THREADS) void kmeans_accumulate_tiled_stage1(const float* __restrict__ x, const int32_t* __restrict__ labels,
                                                                             double* __restrict__ part_sums, long long* __restrict__ part_cnt,
                                                                             long long P, int d, int k, int tile_k, int tile0,
                                                                             long long pts_per_block) {
  extern __shared__ __attribute__((aligned(16))) float acc[];   // [tile_k][d] sums, then [tile_k] counts
  int* cnt = reinterpret_cast<int*>(acc + tile_k * d);
  const int a = (tile0 + (int)blockIdx.y) * tile_k;              // the tile's first cluster (a < k: the host launches ceil(k / tile_k) tiles)
  const int tk = k - a < tile_k ? k - a : tile_k;
  for (int i = threadIdx.x; i < tk * d; i += KT_THREADS) acc[i] = 0.f;
  for (int i = threadIdx.x; i < tk; i += KT_THREADS) cnt[i] = 0;
  __syncthreads();
  const long long p0 = (long long)blockIdx.x * pts_per_block;
  const long long p1 = p0 + pts_per_block < P ? p0 + pts_per_block : P;
  // thread t owns feature columns t, t + 256, ... and walks the block's points in order: no atomics, fixed summation order
  for (int t = threadIdx.x; t < d; t += KT_THREADS)
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
  for (int i = threadIdx.x; i < tk * d; i += KT_THREADS) ps[i] = (double)acc[i];
  for (int i = threadIdx.x; i < tk; i += KT_THREADS) pc[i] = (long long)cnt[i];
}

// the fold of kmeans_accumulate_stage2: block order, fp64
__global__ __launch_bounds__(KT_THREADS) void kmeans_accumulate_tiled_stage2(const double* __restrict__ part_sums,
                                                                             const long long* __restrict__ part_cnt, double* __restrict__ sums,
                                                                             long long* __restrict__ counts, long long kd, int k, int blocks) {
  const long long i = (long long)blockIdx.x * KT_THREADS + threadIdx.x;
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

// tile_k as the caller gave it -> the tile the kernels run (0 = the default); -1 = refused (the message is set)
static int kt_resolve_tile(const char* who, int d, int k, int tile_k) {
  const int most = kt_tile_default(d);
  if (tile_k < 0 || tile_k > most) {
    set_error("%s: tile_k = %d is outside 1 ... %d, the centroids of d = %d columns that fill 64 KB (0 = that default)", who, tile_k, most, d);
    return -1;
  }
  return tile_k == 0 ? most : tile_k;
}

}  // namespace tt

using namespace tt;

extern "C" int tt_kmeans_tiled_shape_ok(int d, int k) { return kt_shape_ok(d, k) ? 1 : 0; }
extern "C" int tt_kmeans_tile_centroids(int d) { return kt_tile_default(d); }

extern "C" int tt_kmeans_assign_tiled(const float* x, const float* centroids, int32_t* labels, float* dist2, long long P, int d, int k,
                                      int tile_k, tt_stream_t stream) {
  TT_REQUIRE(x && centroids && labels && P > 0, "kmeans_assign_tiled: bad arguments");
  TT_REQUIRE(kt_shape_ok(d, k), "kmeans_assign_tiled: k = %d, d = %d: need 1 <= d <= %d, k >= 1, k * d < 2^31", k, d, KT_MAXD);
  const int tile = kt_resolve_tile("kmeans_assign_tiled", d, k, tile_k);
  if (tile < 0) return TT_EINVAL;
  const size_t lds = kt_assign_lds(d, tile);
  TT_REQUIRE(lds <= KT_MAX_LDS, "kmeans_assign_tiled: %zu bytes of LDS (at most %zu)", lds, KT_MAX_LDS);
  static const bool lds_attr_set = [] {  // up to 65 KB (d = 64: the point tile), beyond the 64 KB a kernel gets unasked
    bool ok = true;
    for (const void* f : {reinterpret_cast<const void*>(&kmeans_assign_tiled_kernel<16>), reinterpret_cast<const void*>(&kmeans_assign_tiled_kernel<64>),
                          reinterpret_cast<const void*>(&kmeans_assign_tiled_kernel<0>)})
      ok = ok && hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)KT_MAX_LDS) == hipSuccess;
    return ok;
  }();
  TT_REQUIRE(lds_attr_set, "kmeans_assign_tiled: could not raise the dynamic LDS limit");
  long long blocks = (P + KT_THREADS - 1) / KT_THREADS;
  blocks = blocks > 4096 ? 4096 : blocks;
  hipStream_t s = as_stream(stream);
  const int route = kt_assign_route(d);
  if (route == 16)
    hipLaunchKernelGGL((kmeans_assign_tiled_kernel<16>), dim3((unsigned)blocks), dim3(KT_THREADS), lds, s, x, centroids, labels, dist2, P, d, k, tile);
  else if (route == 64)
    hipLaunchKernelGGL((kmeans_assign_tiled_kernel<64>), dim3((unsigned)blocks), dim3(KT_THREADS), lds, s, x, centroids, labels, dist2, P, d, k, tile);
  else
    hipLaunchKernelGGL((kmeans_assign_tiled_kernel<0>), dim3((unsigned)blocks), dim3(KT_THREADS), lds, s, x, centroids, labels, dist2, P, d, k, tile);
  TT_CHECK_LAUNCH("kmeans_assign_tiled");
  return TT_OK;
}

// One fp64 partial per (block, cluster, column) and one count per (block, cluster), as tt_kmeans_accumulate: the tiles of one call
// write disjoint rows of it, so the size does not depend on tile_k (the argument is part of the query for symmetry with the launch).
extern "C" size_t tt_kmeans_accumulate_tiled_workspace_bytes(long long P, int d, int k, int tile_k) {
  (void)tile_k;
  if (!kt_shape_ok(d, k)) return 0;
  return (size_t)kt_accumulate_blocks(P) * ((size_t)k * d * sizeof(double) + (size_t)k * sizeof(long long));
}

extern "C" int tt_kmeans_accumulate_tiled(const float* x, const int32_t* labels, double* sums, long long* counts, long long P, int d, int k,
                                          int tile_k, void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  TT_REQUIRE(x && labels && sums && counts && workspace && P > 0, "kmeans_accumulate_tiled: bad arguments");
  TT_REQUIRE(kt_shape_ok(d, k), "kmeans_accumulate_tiled: k = %d, d = %d: need 1 <= d <= %d, k >= 1, k * d < 2^31", k, d, KT_MAXD);
  const int tile = kt_resolve_tile("kmeans_accumulate_tiled", d, k, tile_k);
  if (tile < 0) return TT_EINVAL;
  TT_REQUIRE(workspace_bytes >= tt_kmeans_accumulate_tiled_workspace_bytes(P, d, k, tile), "kmeans_accumulate_tiled: workspace too small");
  const size_t lds = sizeof(float) * ((size_t)tile * d + tile);   // at most 128 KB (d = 1: 16384 sums and as many counts)
  TT_REQUIRE(lds <= KT_MAX_LDS, "kmeans_accumulate_tiled: %zu bytes of LDS (at most %zu)", lds, KT_MAX_LDS);
  static const bool lds_attr_set = hipFuncSetAttribute(reinterpret_cast<const void*>(&kmeans_accumulate_tiled_stage1),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)KT_MAX_LDS) == hipSuccess;
  TT_REQUIRE(lds_attr_set, "kmeans_accumulate_tiled: could not raise the dynamic LDS limit");
  hipStream_t s = as_stream(stream);
  const int blocks = kt_accumulate_blocks(P);
  const long long ppb = (P + blocks - 1) / blocks;
  const long long kd = (long long)k * d;
  double* part_sums = static_cast<double*>(workspace);
  long long* part_cnt = reinterpret_cast<long long*>(part_sums + (size_t)blocks * kd);
  const int tiles = (k + tile - 1) / tile;   // they ride on gridDim.y, at most 65535 per launch
  for (int t0 = 0; t0 < tiles; t0 += KT_MAX_GRID_Y) {
    const int ny = tiles - t0 < KT_MAX_GRID_Y ? tiles - t0 : KT_MAX_GRID_Y;
    hipLaunchKernelGGL(kmeans_accumulate_tiled_stage1, dim3(blocks, ny), dim3(KT_THREADS), lds, s, x, labels, part_sums, part_cnt, P, d, k, tile, t0,
                       ppb);
  }
  hipLaunchKernelGGL(kmeans_accumulate_tiled_stage2, dim3((unsigned)((kd + KT_THREADS - 1) / KT_THREADS)), dim3(KT_THREADS), 0, s, part_sums, part_cnt,
                     sums, counts, kd, k, blocks);
  TT_CHECK_LAUNCH("kmeans_accumulate_tiled");
  return TT_OK;
}
