// Matching and scoring of evaluated segments on the device (N20): everything PredsmIoU.compute_miou_from_confusion (metrics.py) derives
// from one confusion matrix - the class sets, the score matrix, the Hungarian or the greedy many-to-one matching, tp / fp / fn after
// remapping, the mean Jaccard index and the table pred value -> matched gt value - for ALL segments of an evaluate_localizations call in
// one launch straight behind tt_confusion_counts_segments (confusion.hip), whose counts [S, Cg, Cp] it reads.
//
// The statement is the host path's, bit for bit: every score is an fp64 quotient of exact integers (the segment total stays below 2^53,
// else status 3), the divisions are correctly rounded (__ddiv_rn), nothing is contracted (the pragma below) and nothing depends on
// fast-math.  The Hungarian matching is scipy's rectangular linear_sum_assignment (Crouse's shortest augmenting paths) with ITS scan
// order, because zero-overlap cells all cost exactly 1.0 and the ties decide the false positives:
//   the transpose is solved where there are fewer preds than gts; per row the list of open columns starts DESCENDING; a search step
//   relaxes spc[j] over the list, then takes the LAST minimal position whose column is unassigned, else the FIRST minimal position
//   (the order-free form of scipy's sequential `<, or == and unassigned` scan) and swap-removes it from the list.
// The mean is numpy's pairwise sum at n <= 128 (one block): sequential below 8 values, eight strided accumulators from 8 up.
//
// Layout: ONE wave64 per segment (a workgroup of 64 threads), the segments on gridDim.x.  The searches are data-dependent loops; every
// value that steers one (the minimum, the chosen position, the sink) is reduced to the same bits in all 64 lanes, so the wave never
// diverges around a loop, and the __syncthreads() between the LDS phases of this one-wave workgroup order its LDS traffic only.  Every
// loop is bounded by construction (n_rows augmentations of at most n_cols steps, walks back of at most n_rows edges) and ALSO carries that
// bound as a counter: an overrun or a non-finite minimum sets status 2 and the wave leaves as a whole.
//
// Storage: the row and column sums, the duals and the search state live in LDS (ms_lds_bytes: at most 54 KB at 128 x 1024, under the
// 64 KB a kernel gets unasked); a cost is recomputed from its count (8 bytes, L2-resident: the confusion kernel wrote it a moment ago).
#include "common.hpp"

#pragma clang fp contract(off)

namespace tt {

constexpr int MS_MAX_GT = 128;      // n in numpy's mean stays inside ONE pairwise block (128 values), whose order ms_mean restates
constexpr int MS_MAX_PRED = 1024;   // bounds the per-segment vectors in LDS
constexpr int MS_MAX_GRID = 1 << 20;   // segments of one launch
enum { MS_OK = 0, MS_EMPTY = 1, MS_SEARCH = 2, MS_INEXACT = 3 };
constexpr unsigned long long MS_EXACT = 1ull << 53;

// THE shape rule (tt_match_segments_shape_ok)
inline bool ms_shape_ok(int Cg, int Cp) { return Cg >= 1 && Cg <= MS_MAX_GT && Cp >= 1 && Cp <= MS_MAX_PRED; }

// LDS of one segment, carved in ms_carve's order: 8-byte arrays first
struct MsLds {
  unsigned long long *rows, *cols, *tp_acc, *col_acc;   // [Cg], [Cp], [Cg], [Cg]
  double *u, *v, *spc, *jac;                            // [NR], [NC], [NC], [Cg]
  int *gts, *preds, *target;                            // [Cg], [Cp], [Cp]: present values ascending; pred value -> gt value, -1 unmapped
  int *col4row, *row4col, *path, *remaining;            // [NR], [NC], [NC], [NC]
  int *in_row, *in_col;                                 // [NR], [NC]
};
__host__ __device__ inline int ms_nr(int Cg, int Cp) { return Cg < Cp ? Cg : Cp; }   // rows of the assignment: the smaller class set
__host__ __device__ inline int ms_nc(int Cg, int Cp) { return Cg < Cp ? Cp : Cg; }
__host__ __device__ inline size_t ms_lds_bytes(int Cg, int Cp) {
  const size_t nr = (size_t)ms_nr(Cg, Cp), nc = (size_t)ms_nc(Cg, Cp), g = (size_t)Cg, p = (size_t)Cp;
  return 8 * (g + p + g + g) + 8 * (nr + nc + nc + g) + 4 * (g + p + p) + 4 * (nr + nc + nc + nc) + 4 * (nr + nc);
}
__device__ __forceinline__ MsLds ms_carve(unsigned char* base, int Cg, int Cp) {
  const int nr = ms_nr(Cg, Cp), nc = ms_nc(Cg, Cp);
  MsLds m;
  unsigned long long* q = reinterpret_cast<unsigned long long*>(base);
  m.rows = q; q += Cg;
  m.cols = q; q += Cp;
  m.tp_acc = q; q += Cg;
  m.col_acc = q; q += Cg;
  double* d = reinterpret_cast<double*>(q);
  m.u = d; d += nr;
  m.v = d; d += nc;
  m.spc = d; d += nc;
  m.jac = d; d += Cg;
  int* i = reinterpret_cast<int*>(d);
  m.gts = i; i += Cg;
  m.preds = i; i += Cp;
  m.target = i; i += Cp;
  m.col4row = i; i += nr;
  m.row4col = i; i += nc;
  m.path = i; i += nc;
  m.remaining = i; i += nc;
  m.in_row = i; i += nr;
  m.in_col = i;
  return m;
}

__device__ __forceinline__ unsigned long long ms_wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int ms_wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// IoU / precision if gt class g (row sum `row`) were matched to pred class p (column sum `col`), tp their cell: score_matrix's order
__device__ __forceinline__ double ms_score(unsigned long long cell, unsigned long long col, unsigned long long row, bool precision) {
  const double tp = (double)cell;
  const double fp = (double)col - tp;
  if (precision) return __ddiv_rn(tp, fmax(tp + fp, 1e-8));
  const double fn = (double)row - tp;
  return __ddiv_rn(tp, fmax(tp + fp + fn, 1e-8));
}

// a candidate of the search step: the value and a key that orders equal values - an unassigned column beats an assigned one, among the
// unassigned the LAST list position wins, among the assigned the FIRST.  A total order: the butterfly leaves the same pair in every lane.
struct MsPick { double val; int key; };
__device__ __forceinline__ int ms_key(bool unassigned, int pos) { return unassigned ? 2 * MS_MAX_PRED + pos : MS_MAX_PRED - 1 - pos; }
__device__ __forceinline__ int ms_key_pos(int key) { return key >= 2 * MS_MAX_PRED ? key - 2 * MS_MAX_PRED : MS_MAX_PRED - 1 - key; }
__device__ __forceinline__ MsPick ms_better(MsPick a, MsPick b) { return (b.val < a.val || (b.val == a.val && b.key > a.key)) ? b : a; }
__device__ __forceinline__ MsPick ms_wave_pick(MsPick a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    MsPick b;
    b.val = __shfl_xor(a.val, o, 64);
    b.key = __shfl_xor(a.key, o, 64);
    a = ms_better(a, b);
  }
  a.val = __shfl(a.val, 0, 64);   // lane 0's pair for everyone: the same bits in all lanes even if a NaN broke the order
  a.key = __shfl(a.key, 0, 64);
  return a;
}

// numpy's mean of a[0 .. n - 1], 1 <= n <= 128 (pairwise_sum's single block).  Every lane computes it: the reads are LDS broadcasts.
__device__ __forceinline__ double ms_mean(const double* a, int n) {
  double s;
  if (n < 8) {
    s = a[0];
    for (int i = 1; i < n; ++i) s = s + a[i];
  } else {
    double r[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) r[t] = a[t];
    const int whole = n - n % 8;
    for (int k = 8; k < whole; k += 8) {
#pragma unroll
      for (int t = 0; t < 8; ++t) r[t] = r[t] + a[k + t];
    }
    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (int i = whole; i < n; ++i) s = s + a[i];
  }
  return __ddiv_rn(s, (double)n);
}

// linear_sum_assignment(1 - IoU) on the compacted n_gt x n_pred matrix; writes m.target.  Returns MS_OK or MS_SEARCH, uniformly.
__device__ int ms_hungarian(const MsLds& m, const unsigned long long* __restrict__ counts, int Cp, int n_gt, int n_pred, int lane) {
  const bool transposed = n_pred < n_gt;           // rows are the preds then
  const int nr = transposed ? n_pred : n_gt, nc = transposed ? n_gt : n_pred;
  for (int i = lane; i < nr; i += kWave) {
    m.u[i] = 0.0;
    m.col4row[i] = -1;
  }
  for (int j = lane; j < nc; j += kWave) {
    m.v[j] = 0.0;
    m.row4col[j] = -1;
  }
  for (int cur = 0; cur < nr; ++cur) {
    for (int j = lane; j < nc; j += kWave) {
      m.spc[j] = INFINITY;
      m.path[j] = -1;
      m.in_col[j] = 0;
      m.remaining[j] = nc - 1 - j;
    }
    for (int i = lane; i < nr; i += kWave) m.in_row[i] = 0;
    __syncthreads();
    int n_rem = nc, i = cur, sink = -1;
    double min_val = 0.0;
    for (int steps = 0; sink < 0; ++steps) {
      if (steps >= nc || n_rem < 1) return MS_SEARCH;        // the bound, carried: a row's search takes at most nc steps
      m.in_row[i] = 1;                                      // (every lane, one value)
      const double ui = m.u[i];
      const int row_value = transposed ? m.preds[i] : m.gts[i];
      MsPick best;
      best.val = INFINITY;
      best.key = -1;
      for (int t = lane; t < n_rem; t += kWave) {
        const int j = m.remaining[t];
        const int g = transposed ? m.gts[j] : row_value, p = transposed ? row_value : m.preds[j];
        const double cost = 1.0 - ms_score(counts[(size_t)g * Cp + p], m.cols[p], m.rows[g], false);
        const double r = min_val + cost - ui - m.v[j];
        double s = m.spc[j];
        if (r < s) {
          s = r;
          m.spc[j] = r;
          m.path[j] = i;
        }
        MsPick c;
        c.val = s;
        c.key = ms_key(m.row4col[j] < 0, t);
        best = ms_better(best, c);
      }
      best = ms_wave_pick(best);
      if (best.key < 0 || !(best.val < INFINITY)) return MS_SEARCH;   // nothing reachable, or a NaN: no finite minimum
      const int pos = ms_key_pos(best.key);
      min_val = best.val;
      const int j = m.remaining[pos], last = m.remaining[n_rem - 1];
      const int r4 = m.row4col[j];
      if (r4 < 0)
        sink = j;
      else
        i = r4;
      __syncthreads();                                      // every lane has read the list before it changes
      m.in_col[j] = 1;                                      // (every lane, one value)
      m.remaining[pos] = last;
      --n_rem;
      __syncthreads();                                      // ... and sees the new list, and this step's spc / path, in the next step
    }
    // dual update
    for (int r = lane; r < nr; r += kWave) {
      if (m.in_row[r]) {
        if (r == cur)
          m.u[r] = m.u[r] + min_val;
        else
          m.u[r] = m.u[r] + (min_val - m.spc[m.col4row[r]]);
      }
    }
    for (int j = lane; j < nc; j += kWave) {
      if (m.in_col[j]) m.v[j] = m.v[j] - (min_val - m.spc[j]);
    }
    __syncthreads();
    // augment: walk back from the sink.  Every lane does the same reads and writes the same values.
    int j = sink;
    for (int edges = 0;; ++edges) {
      if (edges >= nr) return MS_SEARCH;                     // an alternating path has at most nr edges into rows
      const int i2 = m.path[j];
      if (i2 < 0 || i2 >= nr) return MS_SEARCH;
      const int prev = m.col4row[i2];
      __syncthreads();
      m.row4col[j] = i2;
      m.col4row[i2] = j;
      __syncthreads();
      j = prev;
      if (i2 == cur) break;
      if (j < 0 || j >= nc) return MS_SEARCH;
    }
  }
  for (int i = lane; i < nr; i += kWave) {
    const int j = m.col4row[i];
    const int g = transposed ? m.gts[j] : m.gts[i], p = transposed ? m.preds[i] : m.preds[j];
    m.target[p] = g;
  }
  return MS_OK;
}

__global__ __launch_bounds__(kWave) void match_segments_kernel(const unsigned long long* __restrict__ counts_all, int s0, int Cg, int Cp, int mode,
                                                               int precision_based, int involve_bg, double* __restrict__ score,
                                                               double* __restrict__ matched_bg, long long* __restrict__ tp,
                                                               long long* __restrict__ fp, long long* __restrict__ fn,
                                                               long long* __restrict__ lut, int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ms_smem[];
  const MsLds m = ms_carve(ms_smem, Cg, Cp);
  const int lane = (int)threadIdx.x;
  const size_t s = (size_t)s0 + blockIdx.x;
  const unsigned long long* __restrict__ counts = counts_all + s * (size_t)Cg * Cp;

  // 1. row and column sums, the class sets
  for (int p = lane; p < Cp; p += kWave) {
    m.cols[p] = 0;
    m.target[p] = -1;
  }
  for (int g = lane; g < Cg; g += kWave) m.tp_acc[g] = m.col_acc[g] = 0;
  unsigned long long total = 0;
  for (int g = 0; g < Cg; ++g) {
    unsigned long long row = 0;
    for (int p = lane; p < Cp; p += kWave) {                // lane p owns cols[p], cols[p + 64], ...
      const unsigned long long c = counts[(size_t)g * Cp + p];
      row += c;
      m.cols[p] += c;
    }
    row = ms_wave_sum_u64(row);
    m.rows[g] = row;                                        // (every lane, one value)
    total += row;
  }
  __syncthreads();
  int n_gt = 0, n_pred = 0;
  for (int base = 0; base < Cg; base += kWave) {
    const bool present = base + lane < Cg && m.rows[base + lane] > 0;
    const unsigned long long mask = __ballot(present);
    if (present) m.gts[n_gt + __popcll(mask & ((1ull << lane) - 1ull))] = base + lane;
    n_gt += __popcll(mask);
  }
  for (int base = 0; base < Cp; base += kWave) {
    const bool present = base + lane < Cp && m.cols[base + lane] > 0;
    const unsigned long long mask = __ballot(present);
    if (present) m.preds[n_pred + __popcll(mask & ((1ull << lane) - 1ull))] = base + lane;
    n_pred += __popcll(mask);
  }
  __syncthreads();
  int status = MS_OK;
  if (n_gt == 0)
    status = MS_EMPTY;
  else if (total >= MS_EXACT)
    status = MS_INEXACT;
  double bg = 0.0, mean = 0.0;

  // 3. the matching (status, n_gt, n_pred, mode are the same in every lane)
  if (status == MS_OK && mode == TT_MATCH_MANY_TO_ONE) {
    const int first = m.gts[0];
    int to_first = 0;
    for (int t = lane; t < n_pred; t += kWave) {
      const int p = m.preds[t];
      double best = -1.0;
      int best_g = first;
      for (int k = 0; k < n_gt; ++k) {                     // ascending gt: the first maximum wins
        const int g = m.gts[k];
        const double sc = ms_score(counts[(size_t)g * Cp + p], m.cols[p], m.rows[g], precision_based != 0);
        if (sc > best) {
          best = sc;
          best_g = g;
        }
      }
      m.target[p] = best_g;
      to_first += best_g == first;
    }
    bg = __ddiv_rn((double)ms_wave_sum_i(to_first), (double)n_pred);
  } else if (status == MS_OK) {
    status = ms_hungarian(m, counts, Cp, n_gt, n_pred, lane);
    bg = __ddiv_rn(1.0, (double)n_gt);
  }
  __syncthreads();

  // 4. counts after remapping (unmapped preds count towards gt VALUE 0), Jaccard indices, numpy's mean
  if (status == MS_OK) {
    for (int t = lane; t < n_pred; t += kWave) {
      const int p = m.preds[t];
      const int g = m.target[p] < 0 ? 0 : m.target[p];
      atomicAdd(&m.tp_acc[g], counts[(size_t)g * Cp + p]);   // integer adds: the order does not show
      atomicAdd(&m.col_acc[g], m.cols[p]);
    }
    __syncthreads();
    const int skip = (!involve_bg && m.gts[0] == 0) ? 1 : 0;   // gt value 0, if present, is the first of the ascending list
    for (int k = lane; k < n_gt; k += kWave) {
      const int g = m.gts[k];
      const long long t = (long long)m.tp_acc[g], f = (long long)(m.col_acc[g] - m.tp_acc[g]), n = (long long)(m.rows[g] - m.tp_acc[g]);
      if (k >= skip) m.jac[k - skip] = __ddiv_rn((double)t, fmax((double)(t + f + n), 1e-8));
    }
    __syncthreads();
    mean = n_gt - skip > 0 ? ms_mean(m.jac, n_gt - skip) : 0.0;
  } else {
    bg = 0.0;
  }

  // 5. write-out: every element of the segment's outputs, once
  const bool ok = status == MS_OK;
  for (int g = lane; g < Cg; g += kWave) {
    const bool present = ok && m.rows[g] > 0;
    const unsigned long long t = present ? m.tp_acc[g] : 0ull;
    tp[s * Cg + g] = (long long)t;
    fp[s * Cg + g] = present ? (long long)(m.col_acc[g] - t) : 0ll;
    fn[s * Cg + g] = present ? (long long)(m.rows[g] - t) : 0ll;
  }
  for (int p = lane; p < Cp; p += kWave) lut[s * Cp + p] = (ok && m.target[p] > 0) ? (long long)m.target[p] : 0ll;
  if (lane == 0) {
    score[s] = mean;
    matched_bg[s] = bg;
    info[s * 4 + 0] = status;
    info[s * 4 + 1] = n_gt;
    info[s * 4 + 2] = n_pred;
    info[s * 4 + 3] = n_pred > 0 ? m.preds[n_pred - 1] : 0;
  }
}

}  // namespace tt

using namespace tt;

extern "C" int tt_match_segments_shape_ok(int Cg, int Cp) { return ms_shape_ok(Cg, Cp) ? 1 : 0; }

extern "C" int tt_match_segments(const unsigned long long* counts, int S, int Cg, int Cp, int mode, int precision_based, int involve_bg,
                                 double* score, double* matched_bg, long long* tp, long long* fp, long long* fn, long long* lut, int* info,
                                 tt_stream_t stream) {
  TT_REQUIRE(counts && score && matched_bg && tp && fp && fn && lut && info, "match_segments: null pointer");
  TT_REQUIRE(S >= 1, "match_segments: S = %d segments: need S >= 1", S);
  TT_REQUIRE(ms_shape_ok(Cg, Cp), "match_segments: Cg = %d, Cp = %d: need 1 <= Cg <= %d and 1 <= Cp <= %d", Cg, Cp, MS_MAX_GT, MS_MAX_PRED);
  TT_REQUIRE(mode == TT_MATCH_HUNGARIAN || mode == TT_MATCH_MANY_TO_ONE, "match_segments: mode code %d is neither %d (Hungarian) nor %d (many-to-one)",
             mode, TT_MATCH_HUNGARIAN, TT_MATCH_MANY_TO_ONE);
  const void* wide[] = {counts, score, matched_bg, tp, fp, fn, lut};
  for (const void* p : wide) TT_REQUIRE(reinterpret_cast<uintptr_t>(p) % 8 == 0, "match_segments: pointer %p must be aligned to 8 bytes", p);
  TT_REQUIRE(reinterpret_cast<uintptr_t>(info) % 4 == 0, "match_segments: info (%p) must be aligned to 4 bytes", (const void*)info);
  hipStream_t st = as_stream(stream);
  const size_t lds = ms_lds_bytes(Cg, Cp);   // at most 54 KB: no limit to raise
  for (int s0 = 0; s0 < S; s0 += MS_MAX_GRID) {
    const int chunk = S - s0 < MS_MAX_GRID ? S - s0 : MS_MAX_GRID;
    hipLaunchKernelGGL(match_segments_kernel, dim3((unsigned)chunk), dim3(kWave), lds, st, counts, s0, Cg, Cp, mode, precision_based, involve_bg,
                       score, matched_bg, tp, fp, fn, lut, info);
  }
  TT_CHECK_LAUNCH("match_segments");
  return TT_OK;
}
