// Cluster-based foreground extraction: the statistics path of cluster_based_foreground_extraction.py.
//
// The reference scores every over-cluster by how much of it lies inside the ViT-attention foreground (get_cluster_precs, :85-108),
// searches the precision cut that maximises the Jaccard index against the ground truth (find_good_threshold, :140-153, through
// eval_jac, :111-129) and turns the clusters above the cut into foreground masks (make_post_matching_maps, :221-227).  It loops in
// Python over images and clusters and rebuilds full-dataset masks for every candidate cut.  All of it reduces to per-(image,
// cluster) integer counts, which is what this file computes:
//   tt_cbfe_cluster_stats       one workgroup per image: n, tp_attn, tp_gt per cluster with integer LDS atomics (order-free), and the
//                               image's ground-truth foreground count
//   tt_cbfe_cluster_precs       per cluster, the fp64 sum of tp_attn / n over the images where it occurs, in increasing image order
//                               (the reference's Python float adds), divided by the occurrence count: bit for bit get_cluster_precs
//   tt_cbfe_cut_jaccard         per image, suffix sums of n and tp_gt in the caller's cluster order give intersection and union of
//                               every candidate cut at once; per candidate, the fp32 IoUs are added in image order and divided by M
//                               (eval_jac's `jacs += intersection / union`)
//   tt_cbfe_apply_fg            cluster map -> 0/1 mask through a k-entry table
//   tt_nearest_upsample_labels  token labels -> pixel labels through the row / column tables of torch's nearest rule
// Divisions are IEEE, correctly rounded (__fdiv_rn / __ddiv_rn); nothing here depends on fast-math.
#include "common.hpp"

namespace tt {

constexpr int CB_THREADS = 256;
constexpr int CB_MAXK = 4096;
constexpr int CB_PRECS_CHUNK = 64;   // images staged through LDS per step of tt_cbfe_cluster_precs

__device__ __forceinline__ int block_sum_int(int v, int* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
  return s;
}

// ---- stats[m][j] = {n, tp_attn, tp_gt}, gt_fg[m].  One workgroup per image; counters in LDS (3 k ints).
__global__ __launch_bounds__(CB_THREADS) void cbfe_stats_kernel(const int64_t* __restrict__ clusters, const int64_t* __restrict__ attn,
                                                                const int64_t* __restrict__ gt, int32_t* __restrict__ stats,
                                                                int32_t* __restrict__ gt_fg, long long P, int k, long long ignore,
                                                                int* range_flag) {
  extern __shared__ int cnt[];   // [k][3]
  __shared__ int red[CB_THREADS / 64];
  const long long m = blockIdx.x;
  for (int i = threadIdx.x; i < 3 * k; i += CB_THREADS) cnt[i] = 0;
  __syncthreads();
  const int64_t* cl = clusters + m * P;
  const int64_t* at = attn ? attn + m * P : nullptr;
  const int64_t* gg = gt ? gt + m * P : nullptr;
  int fg_count = 0;
  bool bad = false;
  for (long long p = threadIdx.x; p < P; p += CB_THREADS) {
    const int64_t c = cl[p];
    const int64_t gv = gg ? gg[p] : 0;
    const bool fg = gv != 0 && (ignore < 0 || gv != ignore);
    fg_count += fg ? 1 : 0;
    if (c < 0 || c >= k) {
      bad = true;
      continue;
    }
    atomicAdd(&cnt[3 * c], 1);
    if (at && at[p] == 1) atomicAdd(&cnt[3 * c + 1], 1);
    if (fg) atomicAdd(&cnt[3 * c + 2], 1);
  }
  range_flag_raise(range_flag, bad);
  const int total = block_sum_int(fg_count, red);   // (its barrier also orders the LDS atomics before the write-out)
  int32_t* out = stats + m * 3 * (long long)k;
  for (int i = threadIdx.x; i < 3 * k; i += CB_THREADS) out[i] = cnt[i];
  if (threadIdx.x == 0) gt_fg[m] = total;
}

// ---- precs[j] = (sum over images m with n > 0, in increasing m, of tp_attn / n) / occurrences.  A wave owns 64 clusters; the n and
// tp_attn columns of CB_PRECS_CHUNK images are staged through LDS by all four waves, then each lane runs its serial fp64 chain.
__global__ __launch_bounds__(CB_THREADS) void cbfe_precs_kernel(const int32_t* __restrict__ stats, double* __restrict__ precs,
                                                                int32_t* __restrict__ occ, int M, int k) {
  __shared__ int sn[CB_PRECS_CHUNK][64];
  __shared__ int sa[CB_PRECS_CHUNK][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int j0 = blockIdx.x * 64;
  const int j = j0 + lane;
  double sum = 0.0;
  int count = 0;
  for (int m0 = 0; m0 < M; m0 += CB_PRECS_CHUNK) {
    const int rows = M - m0 < CB_PRECS_CHUNK ? M - m0 : CB_PRECS_CHUNK;
    __syncthreads();
    for (int r = w; r < rows; r += CB_THREADS / 64) {
      const int32_t* row = stats + ((long long)(m0 + r) * k + j) * 3;
      sn[r][lane] = j < k ? row[0] : 0;
      sa[r][lane] = j < k ? row[1] : 0;
    }
    __syncthreads();
    if (w == 0) {
      for (int r = 0; r < rows; ++r) {
        const int n = sn[r][lane];
        if (n > 0) {
          sum += __ddiv_rn((double)sa[r][lane], (double)n);
          ++count;
        }
      }
    }
  }
  if (w == 0 && j < k) {
    precs[j] = __ddiv_rn(sum, (double)count);   // count 0: NaN (the host reports the cluster that never occurs)
    occ[j] = count;
  }
}

// ---- per image m: suffix sums of n and tp_gt over the clusters in `order`, then iou[m][c] for every candidate start.
__global__ __launch_bounds__(CB_THREADS) void cbfe_cut_iou_kernel(const int32_t* __restrict__ stats, const int32_t* __restrict__ gt_fg,
                                                                  const int32_t* __restrict__ order, const int32_t* __restrict__ starts,
                                                                  float* __restrict__ iou_mc, float* __restrict__ iou_cm, int M, int k,
                                                                  int C) {
  __shared__ int suf_n[CB_MAXK + 1];
  __shared__ int suf_t[CB_MAXK + 1];
  __shared__ int part_n[CB_THREADS];
  __shared__ int part_t[CB_THREADS];
  const int m = blockIdx.x, t = threadIdx.x;
  const int32_t* st = stats + (long long)m * k * 3;
  for (int p = t; p < k; p += CB_THREADS) {
    const int j = order[p];
    const bool ok = j >= 0 && j < k;
    suf_n[p] = ok ? st[3 * j] : 0;
    suf_t[p] = ok ? st[3 * j + 2] : 0;
  }
  if (t == 0) {
    suf_n[k] = 0;
    suf_t[k] = 0;
  }
  __syncthreads();
  // suffix sums: thread t owns positions [t seg, (t + 1) seg); integer adds, so any order gives the same counts
  const int seg = (k + CB_THREADS - 1) / CB_THREADS;
  const int lo = t * seg, hi = min(lo + seg, k);
  int sn = 0, stp = 0;
  for (int p = lo; p < hi; ++p) {
    sn += suf_n[p];
    stp += suf_t[p];
  }
  part_n[t] = sn;
  part_t[t] = stp;
  __syncthreads();
  if (t == 0) {
    int an = 0, at = 0;
    for (int q = CB_THREADS - 1; q >= 0; --q) {   // exclusive suffix over the segments
      const int vn = part_n[q], vt = part_t[q];
      part_n[q] = an;
      part_t[q] = at;
      an += vn;
      at += vt;
    }
  }
  __syncthreads();
  int an = part_n[t], at = part_t[t];
  for (int p = hi - 1; p >= lo; --p) {
    an += suf_n[p];
    at += suf_t[p];
    suf_n[p] = an;
    suf_t[p] = at;
  }
  __syncthreads();
  const int g = gt_fg[m];
  for (int c = t; c < C; c += CB_THREADS) {
    int s = starts[c];
    s = s < 0 ? 0 : (s > k ? k : s);
    const int inter = suf_t[s];
    const int uni = g + suf_n[s] - inter;
    const float v = __fdiv_rn((float)inter, (float)uni);   // 0 / 0 = NaN, as the reference's
    iou_mc[(long long)m * C + c] = v;
    if (iou_cm) iou_cm[(long long)c * M + m] = v;
  }
}

// ---- jac[c] = (sequential fp32 sum over m of iou[m][c]) / M: one lane per candidate, lanes read consecutive candidates.
__global__ __launch_bounds__(64) void cbfe_cut_sum_kernel(const float* __restrict__ iou_mc, float* __restrict__ jac, int M, int C) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
#pragma unroll 16
  for (int m = 0; m < M; ++m) s += iou_mc[(long long)m * C + c];
  jac[c] = __fdiv_rn(s, (float)M);
}

__global__ void cbfe_apply_fg_kernel(const int64_t* __restrict__ clusters, const uint8_t* __restrict__ fg, int64_t* __restrict__ mask,
                                     long long total, int k, int* range_flag) {
  bool bad = false;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int64_t c = clusters[i];
    const bool ok = c >= 0 && c < k;
    bad |= !ok;
    mask[i] = (ok && fg[c]) ? 1 : 0;
  }
  range_flag_raise(range_flag, bad);
}

__global__ void nearest_upsample_labels_kernel(const int32_t* __restrict__ tok, const int32_t* __restrict__ iy,
                                               const int32_t* __restrict__ ix, int64_t* __restrict__ out, long long total, int g, int R) {
  const long long RR = (long long)R * R;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long m = i / RR;
    const int pix = (int)(i - m * RR);
    const int y = iy[pix / R], x = ix[pix % R];
    out[i] = (y >= 0 && y < g && x >= 0 && x < g) ? (int64_t)tok[m * g * g + y * g + x] : (int64_t)-1;
  }
}

static unsigned grid_for(long long total) {
  long long b = (total + CB_THREADS - 1) / CB_THREADS;
  return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

}  // namespace tt

using namespace tt;

extern "C" int tt_cbfe_cluster_stats(const int64_t* clusters, const int64_t* attn, const int64_t* gt, int32_t* stats, int32_t* gt_fg, int M,
                                     long long P, int k, long long ignore, int* range_flag, tt_stream_t stream) {
  TT_REQUIRE(clusters && stats && gt_fg && range_flag, "cbfe_cluster_stats: clusters, stats, gt_fg and range_flag are required");
  TT_REQUIRE(M >= 1 && P >= 1 && P <= (1LL << 24), "cbfe_cluster_stats: need M >= 1 and 1 <= P <= 2^24 (got %d, %lld)", M, P);
  TT_REQUIRE(k >= 1 && k <= CB_MAXK, "cbfe_cluster_stats: need 1 <= k <= %d (got %d)", CB_MAXK, k);
  hipLaunchKernelGGL(cbfe_stats_kernel, dim3((unsigned)M), dim3(CB_THREADS), sizeof(int) * 3 * (size_t)k, as_stream(stream), clusters, attn, gt,
                     stats, gt_fg, P, k, ignore, range_flag);
  TT_CHECK_LAUNCH("cbfe_cluster_stats");
  return TT_OK;
}

extern "C" int tt_cbfe_cluster_precs(const int32_t* stats, double* precs, int32_t* occurrences, int M, int k, tt_stream_t stream) {
  TT_REQUIRE(stats && precs && occurrences, "cbfe_cluster_precs: bad arguments");
  TT_REQUIRE(M >= 1 && k >= 1 && k <= CB_MAXK, "cbfe_cluster_precs: need M >= 1 and 1 <= k <= %d (got %d, %d)", CB_MAXK, M, k);
  hipLaunchKernelGGL(cbfe_precs_kernel, dim3((unsigned)((k + 63) / 64)), dim3(CB_THREADS), 0, as_stream(stream), stats, precs, occurrences, M, k);
  TT_CHECK_LAUNCH("cbfe_cluster_precs");
  return TT_OK;
}

extern "C" size_t tt_cbfe_cut_jaccard_workspace_bytes(int M, int C) { return (size_t)M * (size_t)C * sizeof(float); }

extern "C" int tt_cbfe_cut_jaccard(const int32_t* stats, const int32_t* gt_fg, const int32_t* order, const int32_t* starts, float* jac,
                                   float* iou, int M, int k, int C, void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  TT_REQUIRE(stats && gt_fg && order && starts && jac && workspace, "cbfe_cut_jaccard: bad arguments");
  TT_REQUIRE(M >= 1 && k >= 1 && k <= CB_MAXK && C >= 1, "cbfe_cut_jaccard: need M >= 1, 1 <= k <= %d, C >= 1 (got %d, %d, %d)", CB_MAXK, M, k,
             C);
  TT_REQUIRE(workspace_bytes >= tt_cbfe_cut_jaccard_workspace_bytes(M, C), "cbfe_cut_jaccard: workspace too small");
  hipStream_t s = as_stream(stream);
  float* iou_mc = static_cast<float*>(workspace);
  hipLaunchKernelGGL(cbfe_cut_iou_kernel, dim3((unsigned)M), dim3(CB_THREADS), 0, s, stats, gt_fg, order, starts, iou_mc, iou, M, k, C);
  hipLaunchKernelGGL(cbfe_cut_sum_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, s, iou_mc, jac, M, C);
  TT_CHECK_LAUNCH("cbfe_cut_jaccard");
  return TT_OK;
}

extern "C" int tt_cbfe_apply_fg(const int64_t* clusters, const uint8_t* fg_table, int64_t* mask, long long total, int k, int* range_flag,
                                tt_stream_t stream) {
  TT_REQUIRE(clusters && fg_table && mask && range_flag && total >= 1 && k >= 1, "cbfe_apply_fg: bad arguments");
  hipLaunchKernelGGL(cbfe_apply_fg_kernel, dim3(grid_for(total)), dim3(CB_THREADS), 0, as_stream(stream), clusters, fg_table, mask, total, k,
                     range_flag);
  TT_CHECK_LAUNCH("cbfe_apply_fg");
  return TT_OK;
}

extern "C" int tt_nearest_upsample_labels(const int32_t* tok, const int32_t* iy, const int32_t* ix, int64_t* out, int M, int g, int R,
                                          tt_stream_t stream) {
  TT_REQUIRE(tok && iy && ix && out, "nearest_upsample_labels: bad arguments");
  TT_REQUIRE(M >= 1 && g >= 1 && R >= 1 && (long long)g * g <= (1LL << 30), "nearest_upsample_labels: need M, g, R >= 1 (got %d, %d, %d)", M,
             g, R);
  const long long total = (long long)M * R * R;
  hipLaunchKernelGGL(nearest_upsample_labels_kernel, dim3(grid_for(total)), dim3(CB_THREADS), 0, as_stream(stream), tok, iy, ix, out, total,
                     g, R);
  TT_CHECK_LAUNCH("nearest_upsample_labels");
  return TT_OK;
}
