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
// The device loop (N28, tt_kmeans_fit_loop) is the same kernels with the redo of a fit on a grid axis - every redo reads ONE point set and
// its own centroids, labels and partials - plus four small kernels of its own (seeds, update, split, objective): all redos and
// iterations of clustering.Kmeans._iterate enqueued on one stream, the loop's bits, one read-back of objectives and status words.
#include "kmeans.hpp"

namespace tt {

// ---- resident assignment: label = argmin_j |x - c_j|^2 (first minimum), optional squared distance, of problem y0 + blockIdx.y.
// Problem b reads the points at x + b x_stride - P d for a batch of point sets, 0 where every problem reads ONE set against its own
// centroids (the redos of the device loop) - and is left alone where status[b] != 0 (the loop's flagged redos; null = none).
// A workgroup owns 256 consecutive points: their rows are fetched as one contiguous, fully coalesced block into LDS (row
// stride d | 1, odd, so that the per-thread row reads below are bank-conflict-free), each thread then keeps ITS point in
// registers (d <= 64) and walks the centroids, which every lane reads from LDS at the same address (broadcast).
template <int DREG>
__global__ __launch_bounds__(KM_THREADS) void kmeans_assign_kernel(const float* __restrict__ x, const float* __restrict__ cent,
                                                                   int32_t* __restrict__ labels, float* __restrict__ dist2, long long P, int d,
                                                                   int k, int y0, long long x_stride, const int32_t* __restrict__ status) {
  extern __shared__ float sm[];
  float* cs = sm;                 // [k][d]
  float* xs = sm + k * d;         // [256][ds]
  const int ds = d | 1;
  const size_t b = (size_t)y0 + blockIdx.y;
  if (status && status[b] != 0) return;   // (uniform over the workgroup)
  x += b * (size_t)x_stride;
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

// ---- tiled assignment.  A workgroup owns 256 consecutive points (grid-stride), as kmeans_assign_kernel; DREG as there.  blockIdx.y is
// the centroid set (one for the tiled entry, the redo for the device loop): set r at cent + r cent_stride against the ONE point set x,
// its outputs at labels + r P (dist2 + r P), left alone where status[r] != 0 (null = none).
template <int DREG>
__global__ __launch_bounds__(KM_THREADS) void kmeans_assign_tiled_kernel(const float* __restrict__ x, const float* __restrict__ cent,
                                                                         int32_t* __restrict__ labels, float* __restrict__ dist2,
                                                                         long long P, int d, int k, int tile_k, long long cent_stride,
                                                                         const int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) float sm[];   // the point tile [256][d | 1], THEN the centroid tile [tile_k][d]
  const int ds = d | 1;
  const size_t r = blockIdx.y;
  if (status && status[r] != 0) return;   // (uniform over the workgroup)
  cent += r * (size_t)cent_stride;
  labels += r * (size_t)P;
  if (dist2) dist2 += r * (size_t)P;
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

// ---- resident accumulation: per-block sums[k][d] (fp32 in LDS over the block's pts_per_block points, then fp64 partials).
// blockIdx.y is the label set (one for the entry, the redo for the device loop): set r reads labels + r P of the ONE point set x and
// writes its own gridDim.x blocks of partials; left alone where status[r] != 0 (null = none).
__global__ __launch_bounds__(KM_THREADS) void kmeans_accumulate_stage1(const float* __restrict__ x, const int32_t* __restrict__ labels,
                                                                       double* __restrict__ part_sums, long long* __restrict__ part_cnt,
                                                                       long long P, int d, int k, long long pts_per_block,
                                                                       const int32_t* __restrict__ status) {
  extern __shared__ float acc[];  // [k][d] sums, then [k] counts
  float* cnt = acc + k * d;
  const size_t r = blockIdx.y;
  if (status && status[r] != 0) return;   // (uniform over the workgroup)
  labels += r * (size_t)P;
  part_sums += r * (size_t)gridDim.x * k * d;
  part_cnt += r * (size_t)gridDim.x * k;
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
// additions are kmeans_accumulate_stage1's: the block's points in order, fp32.  The label set rides on blockIdx.z, as on
// kmeans_accumulate_stage1's blockIdx.y.
__global__ __launch_bounds__(KM_THREADS) void kmeans_accumulate_tiled_stage1(const float* __restrict__ x, const int32_t* __restrict__ labels,
                                                                             double* __restrict__ part_sums, long long* __restrict__ part_cnt,
                                                                             long long P, int d, int k, int tile_k, int tile0,
                                                                             long long pts_per_block, const int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) float acc[];   // [tile_k][d] sums, then [tile_k] counts
  const size_t r = blockIdx.z;
  if (status && status[r] != 0) return;   // (uniform over the workgroup)
  labels += r * (size_t)P;
  part_sums += r * (size_t)gridDim.x * k * d;
  part_cnt += r * (size_t)gridDim.x * k;
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

// ---- the fold of both accumulations: block order, fp64.  blockIdx.y is the set of partials (one for the entries, the redo for the
// device loop), its sums at sums + y kd and counts at counts + y k.
__global__ __launch_bounds__(KM_THREADS) void kmeans_accumulate_stage2(const double* __restrict__ part_sums, const long long* __restrict__ part_cnt,
                                                                       double* __restrict__ sums, long long* __restrict__ counts, long long kd,
                                                                       int k, int blocks, const int32_t* __restrict__ status) {
  const size_t r = blockIdx.y;
  if (status && status[r] != 0) return;   // (uniform over the workgroup)
  part_sums += r * (size_t)blocks * kd;
  part_cnt += r * (size_t)blocks * k;
  sums += r * (size_t)kd;
  counts += r * (size_t)k;
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

// ---- the device loop's own kernels (N28): what clustering.Kmeans._iterate does between the kernels above.  Redo r is left alone by
// each of them where status[r] != 0.

// the seeds: centroid j of redo r is row init[r][j] of x; status[r] = 0.  grid (ceil(k d / 256), nredo)
__global__ __launch_bounds__(KM_THREADS) void kmeans_loop_init_kernel(const float* __restrict__ x, const int32_t* __restrict__ init,
                                                                      float* __restrict__ cent, int32_t* __restrict__ status, int d, int k) {
  const size_t r = blockIdx.y;
  const long long kd = (long long)k * d, i = (long long)blockIdx.x * KM_THREADS + threadIdx.x;
  if (i < kd) cent[r * (size_t)kd + i] = x[(size_t)init[r * (size_t)k + i / d] * d + (i % d)];
  if (i == 0) status[r] = 0;
}

// the update: c = (float)(sum / (double)count) where count > 0, the old row otherwise (the host's torch.where; the fused fit's
// update), and cnt, an int copy of this iteration's counts for the split that nothing carries to the next iteration - as the host's
// counts_h.  grid (ceil(k d / 256), redos): one thread per centroid entry, the first k of a redo also copy a count.
__global__ __launch_bounds__(KM_THREADS) void kmeans_loop_update_kernel(const double* __restrict__ sums, const long long* __restrict__ counts,
                                                                        float* __restrict__ cent, int* __restrict__ cnt,
                                                                        const int32_t* __restrict__ status, int d, int k) {
  const size_t r = blockIdx.y;
  if (status[r] != 0) return;   // (uniform over the workgroup)
  const long long kd = (long long)k * d, i = (long long)blockIdx.x * KM_THREADS + threadIdx.x;
  counts += r * (size_t)k;
  if (i < kd) {
    const long long c = counts[i / d];
    if (c > 0) cent[r * (size_t)kd + i] = (float)(sums[r * (size_t)kd + i] / (double)c);
  }
  if (i < k) cnt[r * (size_t)k + i] = (int)counts[i];
}

// the split of iteration `it` (0-based), after the update: one workgroup per redo looks for a zero among the counts and, where there is
// one, its first wave runs kf_split_empty on the redo's centroids and on cnt.  draws == null: no split, the first empty cluster flags
// the redo; a split that would read past the table flags it too: status = it + 1.  The split works on global memory: lane 0's arg-max
// scan reads the k counts once per empty cluster, O(k * empties) loads from L2 - nothing at the k = 500 of the over-clustering and
// paid only in an iteration that has an empty cluster.
__global__ __launch_bounds__(KM_THREADS) void kmeans_loop_split_kernel(float* cent, int* cnt, int32_t* status, int n, int d, int k, int it,
                                                                       const double* __restrict__ draws, int n_draws) {
  const size_t r = blockIdx.x;
  if (status[r] != 0) return;   // (uniform over the workgroup)
  cent += r * (size_t)k * d;
  cnt += r * (size_t)k;
  int mine = 0;
  for (int i = threadIdx.x; i < k; i += KM_THREADS) mine |= cnt[i] == 0;
  if (!__syncthreads_or(mine)) return;
  if (!draws) {
    if (threadIdx.x == 0) status[r] = it + 1;
    return;
  }
  if (threadIdx.x < 64) {
    const bool ok = kf_split_empty(cent, cnt, n, d, k, draws, n_draws, threadIdx.x);
    if (threadIdx.x == 0 && !ok) status[r] = it + 1;
  }
}

// the objective: the last iteration's dist2 of redo r, summed in fp64 - per thread over its points in order, across a wave by a fixed
// shuffle tree, across the waves in order: a function of (n, KM_THREADS) alone.  One workgroup per redo.
__global__ __launch_bounds__(KM_THREADS) void kmeans_loop_objective_kernel(const float* __restrict__ dist2, double* __restrict__ obj,
                                                                           const int32_t* __restrict__ status, long long n) {
  __shared__ double wave_obj[KM_THREADS / 64];
  const size_t r = blockIdx.x;
  if (status[r] != 0) return;   // (uniform over the workgroup)
  dist2 += r * (size_t)n;
  double o = 0.0;
  for (long long p = threadIdx.x; p < n; p += KM_THREADS) o += (double)dist2[p];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) o += __shfl_down(o, off, 64);
  if ((threadIdx.x & 63) == 0) wave_obj[threadIdx.x >> 6] = o;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < KM_THREADS / 64; ++w) t += wave_obj[w];
    obj[r] = t;
  }
}

// ---- launching: ONE statement of each launch for the entries and the device loop.  `sets` centroid / label sets ride on a grid axis
// (the entries: the problems of a batch, or one; the loop: the redos in flight), status as in the kernels.

static bool raise_assign_lds() {
  static const bool ok = km_raise_lds(KM_ROUTES(kmeans_assign_kernel));   // the centroids and the d <= 64 tile's points, 128 KB together
  return ok;
}
static bool raise_assign_tiled_lds() {
  static const bool ok = km_raise_lds(KM_ROUTES(kmeans_assign_tiled_kernel));   // up to 65 KB (d = 64: the point tile)
  return ok;
}
static bool raise_accumulate_lds() {
  static const bool ok = km_raise_lds({KM_KERNEL(kmeans_accumulate_stage1)});
  return ok;
}
static bool raise_accumulate_tiled_lds() {
  static const bool ok = km_raise_lds({KM_KERNEL(kmeans_accumulate_tiled_stage1)});
  return ok;
}

// resident assignment of B problems of P points: problem b at x + b x_stride with its centroids at centroids + b k d and its outputs at
// labels + b P (dist2 + b P)
static void launch_assign(const float* x, long long x_stride, const float* centroids, int32_t* labels, float* dist2, int B, long long P, int d,
                          int k, const int32_t* status, hipStream_t s) {
  const size_t lds = km_assign_lds(d, k);
  for (int y0 = 0; y0 < B; y0 += KM_MAX_GRID_Y) {   // the problems ride on gridDim.y, at most 65535 per launch
    const dim3 grid(km_assign_blocks(P), (unsigned)(B - y0 < KM_MAX_GRID_Y ? B - y0 : KM_MAX_GRID_Y));
    KM_LAUNCH_ROUTE(kmeans_assign_kernel, d, grid, lds, s, x, centroids, labels, dist2, P, d, k, y0, x_stride, status);
  }
}

// tiled assignment of the ONE point set x against `sets` <= 65535 centroid sets [k][d], one after the other in memory
static void launch_assign_tiled(const float* x, const float* centroids, int32_t* labels, float* dist2, int sets, long long P, int d, int k,
                                int tile, const int32_t* status, hipStream_t s) {
  KM_LAUNCH_ROUTE(kmeans_assign_tiled_kernel, d, dim3(km_assign_blocks(P), (unsigned)sets), km_assign_tiled_lds(d, tile), s, x, centroids, labels,
                  dist2, P, d, k, tile, (long long)k * d, status);
}

// the workspace of an accumulation as its two stages see it: fp64 partial sums [sets][blocks][k][d], then the counts [sets][blocks][k]
struct Partials {
  double* sums;
  long long* cnt;
};
static Partials carve_partials(void* workspace, int sets, int blocks, long long kd) {
  double* sums = static_cast<double*>(workspace);
  return {sums, reinterpret_cast<long long*>(sums + (size_t)sets * blocks * kd)};
}

// both accumulations of `sets` <= 65535 label sets [P] of the ONE point set x, and their fold: tile == 0 = the resident stage 1
static void launch_accumulate(const float* x, const int32_t* labels, Partials part, double* sums, long long* counts, int sets, long long P,
                              int d, int k, int tile, const int32_t* status, hipStream_t s) {
  const int blocks = km_accumulate_blocks(P);
  const long long ppb = (P + blocks - 1) / blocks;
  const long long kd = (long long)k * d;
  if (tile == 0) {
    hipLaunchKernelGGL(kmeans_accumulate_stage1, dim3(blocks, sets), dim3(KM_THREADS), sizeof(float) * (k * d + k), s, x, labels, part.sums, part.cnt,
                       P, d, k, ppb, status);
  } else {
    const size_t lds = km_accumulate_tiled_lds(d, tile);
    const int tiles = (k + tile - 1) / tile;   // they ride on gridDim.y, at most 65535 per launch
    for (int t0 = 0; t0 < tiles; t0 += KM_MAX_GRID_Y) {
      const int ny = tiles - t0 < KM_MAX_GRID_Y ? tiles - t0 : KM_MAX_GRID_Y;
      hipLaunchKernelGGL(kmeans_accumulate_tiled_stage1, dim3(blocks, ny, sets), dim3(KM_THREADS), lds, s, x, labels, part.sums, part.cnt, P, d, k,
                         tile, t0, ppb, status);
    }
  }
  hipLaunchKernelGGL(kmeans_accumulate_stage2, dim3((unsigned)((kd + KM_THREADS - 1) / KM_THREADS), sets), dim3(KM_THREADS), 0, s, part.sums,
                     part.cnt, sums, counts, kd, k, blocks, status);
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

// ---- the device loop's rules.  The shape: the tiled pair's, k <= n, and n within an int (kf_split_empty's n - k).
constexpr long long KL_MAXN = (1LL << 31) - 1;
static bool kl_shape_ok(long long n, int d, int k) { return km_tiled_shape_ok(d, k) && (long long)k <= n && n <= KL_MAXN; }
// redos of one pass: redo_group of them, 0 (or more than there are) = all
static int kl_group(int nredo, int redo_group) { return redo_group <= 0 || redo_group > nredo ? nredo : redo_group; }
// The workspace of g redos in flight, widest type first: the accumulation's partials, the folded sums [g][k][d] and counts [g][k], the
// labels and the last dist2 [g][n], the split's int counts [g][k].
struct LoopWorkspace {
  Partials part;
  double* sums;
  long long* counts;
  int32_t* labels;
  float* dist2;
  int* cnt;
  size_t bytes;
};
static LoopWorkspace kl_carve(void* workspace, int g, long long n, int d, int k) {
  const int blocks = km_accumulate_blocks(n);
  const long long kd = (long long)k * d;
  LoopWorkspace w;
  w.part = carve_partials(workspace, g, blocks, kd);
  w.sums = reinterpret_cast<double*>(w.part.cnt + (size_t)g * blocks * k);
  w.counts = reinterpret_cast<long long*>(w.sums + (size_t)g * kd);
  w.labels = reinterpret_cast<int32_t*>(w.counts + (size_t)g * k);
  w.dist2 = reinterpret_cast<float*>(w.labels + (size_t)g * n);
  w.cnt = reinterpret_cast<int*>(w.dist2 + (size_t)g * n);
  w.bytes = (size_t)(reinterpret_cast<char*>(w.cnt + (size_t)g * k) - static_cast<char*>(workspace));
  return w;
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
  TT_REQUIRE(raise_assign_lds(), "kmeans_assign: could not raise the dynamic LDS limit");
  launch_assign(x, P * d, centroids, labels, dist2, 1, P, d, k, nullptr, as_stream(stream));
  TT_CHECK_LAUNCH("kmeans_assign");
  return TT_OK;
}

extern "C" int tt_kmeans_assign_batched(const float* x, const float* centroids, int32_t* labels, float* dist2, int B, long long N, int d, int k,
                                        tt_stream_t stream) {
  TT_REQUIRE(x && centroids && labels, "kmeans_assign_batched: null pointer");
  TT_REQUIRE(km_shape_ok(d, k), "kmeans_assign_batched: k = %d, d = %d is beyond what kmeans_assign takes (k * d <= %d, %zu bytes of LDS within %zu)",
             k, d, KM_MAXKD, d > 0 && k > 0 ? km_assign_lds(d, k) : (size_t)0, KM_MAX_LDS);
  TT_REQUIRE(B >= 1 && N >= 1, "kmeans_assign_batched: B = %d problems of N = %lld points: need both >= 1", B, N);
  TT_REQUIRE(raise_assign_lds(), "kmeans_assign_batched: could not raise the dynamic LDS limit");
  launch_assign(x, N * d, centroids, labels, dist2, B, N, d, k, nullptr, as_stream(stream));
  TT_CHECK_LAUNCH("kmeans_assign_batched");
  return TT_OK;
}

extern "C" size_t tt_kmeans_accumulate_workspace_bytes(long long P, int d, int k) { return km_accumulate_workspace_bytes(P, d, k); }

extern "C" int tt_kmeans_accumulate(const float* x, const int32_t* labels, double* sums, long long* counts, long long P, int d, int k,
                                    void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  TT_REQUIRE(x && labels && sums && counts && workspace && P > 0 && d > 0 && k > 0, "kmeans_accumulate: bad arguments");
  TT_REQUIRE((long long)k * d <= KM_MAXKD, "kmeans_accumulate: k * d = %lld exceeds %d", (long long)k * d, KM_MAXKD);
  TT_REQUIRE(km_shape_ok(d, k), "kmeans_accumulate: k = %d, d = %d is beyond what kmeans_assign takes (%zu bytes of LDS, at most %zu)", k, d,
             km_assign_lds(d, k), KM_MAX_LDS);
  TT_REQUIRE(workspace_bytes >= km_accumulate_workspace_bytes(P, d, k), "kmeans_accumulate: workspace too small");
  TT_REQUIRE(raise_accumulate_lds(), "kmeans_accumulate: could not raise the dynamic LDS limit");
  launch_accumulate(x, labels, carve_partials(workspace, 1, km_accumulate_blocks(P), (long long)k * d), sums, counts, 1, P, d, k, 0, nullptr,
                    as_stream(stream));
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
  TT_REQUIRE(raise_assign_tiled_lds(), "kmeans_assign_tiled: could not raise the dynamic LDS limit");
  launch_assign_tiled(x, centroids, labels, dist2, 1, P, d, k, tile, nullptr, as_stream(stream));
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
  TT_REQUIRE(raise_accumulate_tiled_lds(), "kmeans_accumulate_tiled: could not raise the dynamic LDS limit");
  launch_accumulate(x, labels, carve_partials(workspace, 1, km_accumulate_blocks(P), (long long)k * d), sums, counts, 1, P, d, k, tile, nullptr,
                    as_stream(stream));
  TT_CHECK_LAUNCH("kmeans_accumulate_tiled");
  return TT_OK;
}

// ---- N28: the device loop - every redo and iteration of clustering.Kmeans._iterate enqueued on one stream, the kernels above per
// iteration.  Nothing here synchronises, reads back or allocates; kernel boundaries are the only ordering between workgroups.

extern "C" int tt_kmeans_loop_shape_ok(long long n, int d, int k) { return kl_shape_ok(n, d, k) ? 1 : 0; }

extern "C" size_t tt_kmeans_loop_workspace_bytes(long long n, int d, int k, int nredo, int redo_group) {
  if (nredo < 1 || nredo > KM_MAX_GRID_Y || redo_group < 0 || !kl_shape_ok(n, d, k)) return 0;
  return kl_carve(nullptr, kl_group(nredo, redo_group), n, d, k).bytes;
}

// where, in a workspace of that query, the redos in flight of the LAST pass leave their last iteration's labels int32 [g][n] and dist2
// fp32 [g][n] (g = redo_group, 0 = nredo): byte offsets, for tests and tools that look at them; 0 = refused like the query
extern "C" int tt_kmeans_loop_last_offsets(long long n, int d, int k, int nredo, int redo_group, size_t* labels_offset, size_t* dist2_offset) {
  if (!labels_offset || !dist2_offset || tt_kmeans_loop_workspace_bytes(n, d, k, nredo, redo_group) == 0) return 0;
  const LoopWorkspace w = kl_carve(nullptr, kl_group(nredo, redo_group), n, d, k);
  *labels_offset = (size_t)(reinterpret_cast<char*>(w.labels) - static_cast<char*>(nullptr));
  *dist2_offset = (size_t)(reinterpret_cast<char*>(w.dist2) - static_cast<char*>(nullptr));
  return 1;
}

extern "C" int tt_kmeans_fit_loop(const float* x, const int32_t* init, const int32_t* init_host, float* centroids, double* obj,
                                  int32_t* status, long long n, int d, int k, int nredo, int niter, int tile_k, int redo_group,
                                  const double* draws, int n_draws, void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  TT_REQUIRE(x && init && init_host && centroids && obj && status && workspace, "kmeans_fit_loop: null pointer");
  TT_REQUIRE(niter >= 1 && nredo >= 1 && nredo <= KM_MAX_GRID_Y, "kmeans_fit_loop: niter = %d, nredo = %d: need niter >= 1, 1 <= nredo <= %d", niter,
             nredo, KM_MAX_GRID_Y);
  TT_REQUIRE(redo_group >= 0, "kmeans_fit_loop: redo_group = %d: need >= 0 (0 = all %d redos in one pass)", redo_group, nredo);
  TT_REQUIRE(n_draws >= 0 && (draws || n_draws == 0), "kmeans_fit_loop: n_draws = %d values at a %s table of draws: need n_draws >= 0, and 0 without a table",
             n_draws, draws ? "given" : "null");
  TT_REQUIRE(kl_shape_ok(n, d, k), "kmeans_fit_loop: n = %lld, d = %d, k = %d: need 1 <= d <= %d, 1 <= k <= n <= %lld, k * d < 2^31", n, d, k, KM_MAXD,
             KL_MAXN);
  int tile = resolve_tile("kmeans_fit_loop", d, k, tile_k);
  if (tile < 0) return TT_EINVAL;
  if (tile_k == 0 && km_shape_ok(d, k)) tile = 0;   // the resident pair where it takes the shape; a tile_k given asks for the tiled one
  if (tile > 0) {
    TT_REQUIRE(km_assign_tiled_lds(d, tile) <= KM_MAX_LDS && km_accumulate_tiled_lds(d, tile) <= KM_MAX_LDS,
               "kmeans_fit_loop: tile_k = %d at d = %d: %zu and %zu bytes of LDS (at most %zu)", tile, d, km_assign_tiled_lds(d, tile),
               km_accumulate_tiled_lds(d, tile), KM_MAX_LDS);
  }
  for (long long i = 0; i < (long long)nredo * k; ++i)
    TT_REQUIRE(init_host[i] >= 0 && init_host[i] < n, "kmeans_fit_loop: init[%lld][%lld] = %d is outside [0, %lld)", i / k, i % k, init_host[i], n);
  const int group = kl_group(nredo, redo_group);
  const LoopWorkspace w = kl_carve(workspace, group, n, d, k);
  TT_REQUIRE(workspace_bytes >= w.bytes, "kmeans_fit_loop: workspace of %zu bytes is too small (%zu needed)", workspace_bytes, w.bytes);
  TT_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "kmeans_fit_loop: the workspace is not aligned to 8 bytes");
  TT_REQUIRE(tile > 0 ? raise_assign_tiled_lds() && raise_accumulate_tiled_lds() : raise_assign_lds() && raise_accumulate_lds(),
             "kmeans_fit_loop: could not raise the dynamic LDS limit");
  hipStream_t s = as_stream(stream);
  const long long kd = (long long)k * d;
  hipLaunchKernelGGL(kmeans_loop_init_kernel, dim3((unsigned)((kd + KM_THREADS - 1) / KM_THREADS), nredo), dim3(KM_THREADS), 0, s, x, init, centroids,
                     status, d, k);
  for (int r0 = 0; r0 < nredo; r0 += group) {   // one pass: `g` redos in flight on a grid axis, their centroids updated in place
    const int g = nredo - r0 < group ? nredo - r0 : group;
    float* cent = centroids + (size_t)r0 * kd;
    int32_t* st = status + r0;
    for (int it = 0; it < niter; ++it) {
      float* dist2 = it == niter - 1 ? w.dist2 : nullptr;   // the objective is the last iteration's
      if (tile > 0)
        launch_assign_tiled(x, cent, w.labels, dist2, g, n, d, k, tile, st, s);
      else
        launch_assign(x, 0, cent, w.labels, dist2, g, n, d, k, st, s);
      launch_accumulate(x, w.labels, w.part, w.sums, w.counts, g, n, d, k, tile, st, s);
      hipLaunchKernelGGL(kmeans_loop_update_kernel, dim3((unsigned)((kd + KM_THREADS - 1) / KM_THREADS), g), dim3(KM_THREADS), 0, s, w.sums,
                         w.counts, cent, w.cnt, st, d, k);
      hipLaunchKernelGGL(kmeans_loop_split_kernel, dim3(g), dim3(KM_THREADS), 0, s, cent, w.cnt, st, (int)n, d, k, it,
                         n_draws > 0 ? draws : nullptr, n_draws);
    }
    hipLaunchKernelGGL(kmeans_loop_objective_kernel, dim3(g), dim3(KM_THREADS), 0, s, w.dist2, obj + r0, st, n);
  }
  TT_CHECK_LAUNCH("kmeans_fit_loop");
  return TT_OK;
}

