// Batched, fused k-means fit (N13): the frame-wise and sample-wise protocols of clustering.cluster_features
// (clustering.py:39-41,55-57) train one faiss.Kmeans(50, k, niter=50, nredo=5) per frame / per clip on a subsample of at most 256 k
// points.  Driven from the host, one such fit is 250 Lloyd iterations of a dozen launches and two synchronisations each, on half a
// megabyte of points.  Here the whole loop of clustering.Kmeans._iterate runs inside ONE launch for B problems of equal shape:
//   kmeans_fit_kernel            workgroup (redo, problem) keeps its centroids, the fp32 block sums, the fp64 sums and the counts in
//                                LDS and walks niter iterations of assignment / accumulation / update.  No workgroup waits on
//                                another: there is no flag, counter or barrier between workgroups.
// The final index.search(x, 1) of every problem is tt_kmeans_assign_batched (kmeans.hip).
// The arithmetic per output number is that of kmeans.hip's resident pair - km_nearest and km_accumulate_blocks are kmeans.hpp's, the
// contract is spelled out in the header - so a fit that meets no empty cluster returns the bits of the loop.  One that does is
//   tt_kmeans_fit_batched         flagged (status = the iteration) and left to the loop;
//   tt_kmeans_fit_batched_split   (N18) carried on: the SPLIT instantiations run faiss' split - Kmeans._split_empty, statement for
//                                 statement - on the workgroup's LDS centroids and counts after the update (kf_split_empty, one wave), from
//                                 the caller's table of the draws numpy.random.RandomState(1234) hands the host, and return the loop's bits
//                                 there too.  A split call that would read past the table ends its (problem, redo) with the same flag.
#include "kmeans.hpp"

namespace tt {

constexpr int KF_THREADS = 512;              // one workgroup per (problem, redo); two of them fit a CU
constexpr int KF_WAVES = KF_THREADS / 64;
constexpr int KF_MAXD = 64;                  // the point's row lives in registers (km_assign_route's 16 and 64)
constexpr long long KF_MAXN = 1 << 20;       // points of one problem (the subsample of a fit: at most 256 k)
constexpr size_t KF_PREF_LDS = 72 * 1024;    // what it asks for when more blocks per pass are on offer: two workgroups per 160 KB CU

// LDS of a fit workgroup that holds g blocks' fp32 sums at once: fp64 sums [k][d], centroids [k][d], g x fp32 sums [k][d], counts [k].
// The rule (tt_kmeans_fit_shape_ok): 1 <= d <= 64, 1 <= k <= n <= 2^20, and that budget at g = 1 within 128 KB - 16 k d + 4 k bytes,
// k * d <= 8160 or so: k <= 127 at d = 64, k <= 163 at d = 50.  Everything inside 1 <= d, k <= 64 fits with g >= 5.
static size_t kf_fit_lds(int d, int k, int g) { return (size_t)k * d * (sizeof(double) + sizeof(float) * (1 + (size_t)g)) + sizeof(int) * (size_t)k; }
static bool kf_fit_shape_ok(long long n, int d, int k) {
  return d >= 1 && d <= KF_MAXD && k >= 1 && n >= k && n <= KF_MAXN && kf_fit_lds(d, k, 1) <= KM_MAX_LDS;
}
// blocks whose fp32 sums a pass holds side by side: as many as fit the preferred budget, at least one, at most all of them
static int kf_fit_group(long long n, int d, int k) {
  const int blocks = km_accumulate_blocks(n);
  const size_t fixed = kf_fit_lds(d, k, 0), per = sizeof(float) * (size_t)k * d;
  long long g = fixed < KF_PREF_LDS ? (long long)((KF_PREF_LDS - fixed) / per) : 0;
  g = g < 1 ? 1 : g;
  return (int)(g > blocks ? blocks : g);
}

// (faiss' split of the empty clusters, kf_split_empty, is kmeans.hpp's: the device loop of kmeans.hip runs the same statement.)

// ---- the fused fit.  grid (nredo, B), KF_THREADS threads.  Per iteration:
//   assignment    one thread per point (stride KF_THREADS); the row goes from global memory (L2 at these sizes) into registers, the
//                 centroids are read from LDS at one address per wave (broadcast).  The label goes to the workspace, the count to an
//                 integer LDS atomic (integers: the order does not show).
//   accumulation  the points are cut into tt_kmeans_accumulate's blocks; a pass holds `group` of them side by side in LDS, thread
//                 (block, column) walks its block's points in order (fp32), then thread (cluster, column) adds the pass's partials to
//                 the fp64 sums in block order.
//   update        c = (float)(sum / (double)count) where count > 0.
// The objective is taken in the last iteration only: per thread over its points in order, across a wave by a fixed shuffle tree,
// across the waves in order - fp64, a function of (n, KF_THREADS) alone.
template <int DREG, int VEC, bool SPLIT = false>
__global__ __launch_bounds__(KF_THREADS) void kmeans_fit_kernel(const float* __restrict__ x, const int32_t* __restrict__ init,
                                                                float* __restrict__ cent_out, double* __restrict__ obj_out,
                                                                int32_t* __restrict__ status_out, int32_t* __restrict__ labels_ws,
                                                                int n, int d, int k, int niter, int blocks, int ppb, int group,
                                                                const double* __restrict__ draws, int n_draws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kf_smem[];
  const int kd = k * d;
  double* sums = reinterpret_cast<double*>(kf_smem);   // [k][d]
  float* cs = reinterpret_cast<float*>(sums + kd);     // [k][d]
  float* part = cs + kd;                               // [group][k][d]
  int* cnt = reinterpret_cast<int*>(part + (size_t)group * kd);   // [k]
  __shared__ double wave_obj[KF_WAVES];
  __shared__ int empty;
  __shared__ int split_short;   // SPLIT: the draw table ended inside a split call

  const int redo = blockIdx.x, nredo = gridDim.x, b = blockIdx.y, tid = threadIdx.x;
  const float* xb = x + (size_t)b * n * d;
  int32_t* labels = labels_ws + ((size_t)b * nredo + redo) * n;
  const int32_t* seeds = init + (size_t)redo * k;

  for (int i = tid; i < kd; i += KF_THREADS) cs[i] = xb[(size_t)seeds[i / d] * d + (i % d)];
  if (tid == 0) empty = 0, split_short = 0;

  for (int it = 0; it < niter; ++it) {
    for (int i = tid; i < kd; i += KF_THREADS) sums[i] = 0.0;
    for (int i = tid; i < k; i += KF_THREADS) cnt[i] = 0;
    __syncthreads();   // centroids, zeroed sums and counts

    // -- assignment
    const bool last = it == niter - 1;
    double o = 0.0;
    for (int p = tid; p < n; p += KF_THREADS) {
      const float* xp = xb + (size_t)p * d;
      float xr[DREG];
      if (VEC == 4) {
#pragma unroll
        for (int t = 0; t < DREG; t += 4) {
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (t < d) v = *reinterpret_cast<const float4*>(xp + t);
          xr[t] = v.x, xr[t + 1] = v.y, xr[t + 2] = v.z, xr[t + 3] = v.w;
        }
      } else if (VEC == 2) {
#pragma unroll
        for (int t = 0; t < DREG; t += 2) {
          float2 v = make_float2(0.f, 0.f);
          if (t < d) v = *reinterpret_cast<const float2*>(xp + t);
          xr[t] = v.x, xr[t + 1] = v.y;
        }
      } else {
#pragma unroll
        for (int t = 0; t < DREG; ++t) xr[t] = t < d ? xp[t] : 0.f;
      }
      float best;
      int besti;
      km_nearest<DREG>(xr, xp, cs, d, k, best, besti);
      labels[p] = besti;
      atomicAdd(&cnt[besti], 1);
      if (last) o += (double)best;
    }
    __syncthreads();   // labels (this workgroup's own, read back below) and counts

    for (int i = tid; i < k; i += KF_THREADS)
      if (cnt[i] == 0) empty = 1;
    __syncthreads();
    if (!SPLIT && empty) {   // the split is the loop's business (clustering.KmeansBatch reruns this problem there)
      if (tid == 0) status_out[(size_t)b * nredo + redo] = it + 1;
      return;
    }

    if (last) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) o += __shfl_down(o, off, 64);
      if ((tid & 63) == 0) wave_obj[tid >> 6] = o;
    }

    // -- accumulation
    for (int b0 = 0; b0 < blocks; b0 += group) {
      const int g_here = blocks - b0 < group ? blocks - b0 : group;
      for (int i = tid; i < g_here * kd; i += KF_THREADS) part[i] = 0.f;
      __syncthreads();
      for (int i = tid; i < g_here * d; i += KF_THREADS) {
        const int g = i / d, t = i - g * d;
        float* acc = part + (size_t)g * kd + t;
        const int p0 = (b0 + g) * ppb;
        const int p1 = p0 + ppb < n ? p0 + ppb : n;
        int p = p0;
        for (; p + 8 <= p1; p += 8) {   // eight loads in flight, then the additions in point order
          int l[8];
          float v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            l[u] = labels[p + u];
            v[u] = xb[(size_t)(p + u) * d + t];
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) acc[l[u] * d] += v[u];
        }
        for (; p < p1; ++p) acc[labels[p] * d] += xb[(size_t)p * d + t];
      }
      __syncthreads();
      for (int i = tid; i < kd; i += KF_THREADS) {
        double s = sums[i];
        for (int g = 0; g < g_here; ++g) s += (double)part[(size_t)g * kd + i];
        sums[i] = s;
      }
      __syncthreads();
    }

    // -- update
    for (int i = tid; i < kd; i += KF_THREADS) {
      const int c = cnt[i / d];
      if (c > 0) cs[i] = (float)(sums[i] / (double)c);
    }
    __syncthreads();

    // -- split (SPLIT only): Kmeans._split_empty on the updated centroids and this iteration's counts, by the first wave
    if (SPLIT && empty) {
      if (tid < 64) {
        const bool ok = kf_split_empty(cs, cnt, n, d, k, draws, n_draws, tid);
        if (tid == 0 && !ok) split_short = 1;
      }
      __syncthreads();   // the split centroids; every thread has read `empty`
      if (split_short) {   // nothing diverges silently: this (problem, redo) ends as an empty cluster does without SPLIT
        if (tid == 0) status_out[(size_t)b * nredo + redo] = it + 1;
        return;
      }
      if (tid == 0) empty = 0;   // (next written two barriers into the next iteration)
    }
  }

  float* co = cent_out + ((size_t)b * nredo + redo) * kd;
  for (int i = tid; i < kd; i += KF_THREADS) co[i] = cs[i];
  if (tid == 0) {
    double o = 0.0;
    for (int w = 0; w < KF_WAVES; ++w) o += wave_obj[w];
    obj_out[(size_t)b * nredo + redo] = o;
    status_out[(size_t)b * nredo + redo] = 0;
  }
}

}  // namespace tt

using namespace tt;

extern "C" int tt_kmeans_fit_shape_ok(long long n, int d, int k) { return kf_fit_shape_ok(n, d, k) ? 1 : 0; }

// the dynamic LDS a fit workgroup asks for at this shape (0 for a refused one): for the budget's documentation and its test
extern "C" size_t tt_kmeans_fit_lds_bytes(long long n, int d, int k) {
  return kf_fit_shape_ok(n, d, k) ? kf_fit_lds(d, k, kf_fit_group(n, d, k)) : 0;
}

// the labels of every (problem, redo): int32 [B][nredo][n]
extern "C" size_t tt_kmeans_fit_workspace_bytes(int B, int nredo, long long n, int d, int k) {
  if (B < 1 || nredo < 1 || !kf_fit_shape_ok(n, d, k)) return 0;
  return (size_t)B * nredo * (size_t)n * sizeof(int32_t);
}

// Both entries: `who` names the entry in every message; split = the SPLIT instantiations with the draw table.
static int kf_fit_launch(const char* who, bool split, const float* x, const int32_t* init, const int32_t* init_host, float* centroids,
                         double* obj, int32_t* status, int B, long long n, int d, int k, int nredo, int niter, void* workspace,
                         size_t workspace_bytes, const double* draws, int n_draws, tt_stream_t stream) {
  TT_REQUIRE(x && init && init_host && centroids && obj && status && workspace && (!split || draws), "%s: null pointer", who);
  TT_REQUIRE(!split || n_draws >= 1, "%s: n_draws = %d: the table of draws needs at least one", who, n_draws);
  TT_REQUIRE(B >= 1 && B <= KM_MAX_GRID_Y, "%s: B = %d problems: need 1 ... %d per call", who, B, KM_MAX_GRID_Y);
  TT_REQUIRE(niter >= 1 && nredo >= 1 && nredo <= KM_MAX_GRID_Y, "%s: niter = %d, nredo = %d: need niter >= 1, 1 <= nredo <= %d", who, niter, nredo,
             KM_MAX_GRID_Y);
  TT_REQUIRE(n >= k, "%s: n = %lld points are fewer than k = %d clusters", who, n, k);
  TT_REQUIRE(kf_fit_shape_ok(n, d, k),
             "%s: n = %lld, d = %d, k = %d: need 1 <= d <= %d, 1 <= k <= n <= %lld and 16 k d + 4 k = %zu bytes of LDS within %zu", who, n, d, k,
             KF_MAXD, KF_MAXN, kf_fit_lds(d > 0 ? d : 0, k > 0 ? k : 0, 1), KM_MAX_LDS);
  for (long long i = 0; i < (long long)nredo * k; ++i)
    TT_REQUIRE(init_host[i] >= 0 && init_host[i] < n, "%s: init[%lld][%lld] = %d is outside [0, %lld)", who, i / k, i % k, init_host[i], n);
  const size_t need = tt_kmeans_fit_workspace_bytes(B, nredo, n, d, k);
  TT_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes is too small (%zu needed)", who, workspace_bytes, need);
  static const bool lds_attr_set = km_raise_lds(
      {KM_KERNEL(kmeans_fit_kernel<16, 1>), KM_KERNEL(kmeans_fit_kernel<16, 2>), KM_KERNEL(kmeans_fit_kernel<16, 4>),
       KM_KERNEL(kmeans_fit_kernel<64, 1>), KM_KERNEL(kmeans_fit_kernel<64, 2>), KM_KERNEL(kmeans_fit_kernel<64, 4>),
       KM_KERNEL(kmeans_fit_kernel<16, 1, true>), KM_KERNEL(kmeans_fit_kernel<16, 2, true>), KM_KERNEL(kmeans_fit_kernel<16, 4, true>),
       KM_KERNEL(kmeans_fit_kernel<64, 1, true>), KM_KERNEL(kmeans_fit_kernel<64, 2, true>), KM_KERNEL(kmeans_fit_kernel<64, 4, true>)});
  TT_REQUIRE(lds_attr_set, "%s: could not raise the dynamic LDS limit", who);
  const int blocks = km_accumulate_blocks(n);
  const int ppb = (int)((n + blocks - 1) / blocks);
  const int group = kf_fit_group(n, d, k);
  const size_t lds = kf_fit_lds(d, k, group);
  const int vec = !aligned16(x) ? 1 : (d % 4 == 0 ? 4 : (d % 2 == 0 ? 2 : 1));   // the widest load every row of every problem is aligned for
  int32_t* labels = static_cast<int32_t*>(workspace);
  hipStream_t s = as_stream(stream);
  const dim3 grid(nredo, B), block(KF_THREADS);
#define KF_LAUNCH(DREG, VEC)                                                                                                                     \
  do {                                                                                                                                           \
    if (split)                                                                                                                                   \
      hipLaunchKernelGGL((kmeans_fit_kernel<DREG, VEC, true>), grid, block, lds, s, x, init, centroids, obj, status, labels, (int)n, d, k, niter, \
                         blocks, ppb, group, draws, n_draws);                                                                                    \
    else                                                                                                                                         \
      hipLaunchKernelGGL((kmeans_fit_kernel<DREG, VEC>), grid, block, lds, s, x, init, centroids, obj, status, labels, (int)n, d, k, niter,      \
                         blocks, ppb, group, static_cast<const double*>(nullptr), 0);                                                            \
  } while (0)
  if (km_assign_route(d) == 16) {
    if (vec == 4) KF_LAUNCH(16, 4); else if (vec == 2) KF_LAUNCH(16, 2); else KF_LAUNCH(16, 1);
  } else {
    if (vec == 4) KF_LAUNCH(64, 4); else if (vec == 2) KF_LAUNCH(64, 2); else KF_LAUNCH(64, 1);
  }
#undef KF_LAUNCH
  TT_CHECK_LAUNCH(who);
  return TT_OK;
}

extern "C" int tt_kmeans_fit_batched(const float* x, const int32_t* init, const int32_t* init_host, float* centroids, double* obj,
                                     int32_t* status, int B, long long n, int d, int k, int nredo, int niter, void* workspace,
                                     size_t workspace_bytes, tt_stream_t stream) {
  return kf_fit_launch("kmeans_fit_batched", false, x, init, init_host, centroids, obj, status, B, n, d, k, nredo, niter, workspace, workspace_bytes,
                       nullptr, 0, stream);
}

// The same fit with faiss' split of empty clusters done in the kernel (kf_split_empty) from the caller's table of draws.
extern "C" int tt_kmeans_fit_batched_split(const float* x, const int32_t* init, const int32_t* init_host, float* centroids, double* obj,
                                           int32_t* status, int B, long long n, int d, int k, int nredo, int niter, void* workspace,
                                           size_t workspace_bytes, const double* draws, int n_draws, tt_stream_t stream) {
  return kf_fit_launch("kmeans_fit_batched_split", true, x, init, init_host, centroids, obj, status, B, n, d, k, nredo, niter, workspace,
                       workspace_bytes, draws, n_draws, stream);
}

