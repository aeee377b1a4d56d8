// Run-OR dilation of 64-pixel ballot words, shared by davis.hip (N7) and bfscore.hip (N8).
#pragma once
#include "common.hpp"

namespace tt {

typedef unsigned long long u64;

// out bit k = OR over d in [a, a + n) of W(64 + k + d), W = L | C << 64 | R << 128; a in [-63, 63], 1 <= n <= 64 and a + n - 1 <= 63.
__device__ __forceinline__ u64 run_or(u64 L, u64 C, u64 R, int a, int n) {
  const int s = 64 + a;   // 1..127
  u64 lo, hi;
  if (s < 64) {
    lo = (L >> s) | (C << (64 - s));
    hi = (C >> s) | (R << (64 - s));
  } else if (s == 64) {
    lo = C;
    hi = R;
  } else {
    const int q = s - 64;
    lo = (C >> q) | (R << (64 - q));
    hi = R >> q;
  }
  int cov = 1;   // lo bit k holds the OR of u(k .. k + cov - 1)
  while (2 * cov <= n) {
    lo |= (lo >> cov) | (hi << (64 - cov));
    hi |= hi >> cov;
    cov *= 2;
  }
  if (cov < n) {
    const int k = n - cov;
    lo |= (lo >> k) | (hi << (64 - k));
  }
  return lo;
}

// the dilation of one 64-pixel word by element row i: columns lo..hi of the element, anchor column ax
__device__ __forceinline__ u64 row_dilate(u64 L, u64 C, u64 R, int lo, int hi, int ax) {
  int a = lo - ax;
  int n = hi - lo + 1;
  u64 r = 0;
  if (n > 64) {
    r = run_or(L, C, R, a, 64);
    a += 64;
    n -= 64;
  }
  return r | run_or(L, C, R, a, n);
}

}  // namespace tt
