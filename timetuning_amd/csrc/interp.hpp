// The interpolation rules every kernel of this library shares, stated once (device functions only).
//
//   lin_tap          ATen's bilinear source index with align_corners = False (area_pixel_compute_source_index): the two taps of one
//                    output coordinate along one axis and the weight of the second.  upsample.hip's kernels (fp64 and fp32) and
//                    linear_probe.hip's gather, the adjoint of the fp64 up-sampling, all take their taps from here.
//   bilinear_argmax  the four-tap blend of K channels and the first strict maximum over them (torch.max / torch.argmax: the first index
//                    of the maximum), the per-pixel statement of every arg-max up-sampling.
//   cubic_coeffs     the cubic-convolution weights (A = -0.75) of bicubic interpolation: the position-embedding forward (attn_mask.hip)
//                    and its backward (stem_bwd.hip), which must use the forward's weights exactly.
//
// The functions are __forceinline__ and keep one expression form: the compiler contracts a * b + c into fma after inlining, so two
// kernels that call the same function round alike - equal labels from the label kernel and the histogram kernel, an exact adjoint -
// by construction and not by two pasted blocks staying identical.
#pragma once
#include <hip/hip_runtime.h>

namespace tt {

template <typename T>
struct LinTap {
  int i0, i1;   // source cells; i1 == i0 at the far border
  T l;          // weight of i1; i0 gets 1 - l
};

// src = max(scale (dst + 0.5) - 0.5, 0) with scale = (T)n_in / (T)n_out, computed by the caller once per axis
template <typename T>
__device__ __forceinline__ LinTap<T> lin_tap(int dst, T scale, int n_in) {
  T s = scale * (T(dst) + T(0.5)) - T(0.5);
  s = s < T(0) ? T(0) : s;
  LinTap<T> r;
  r.i0 = (int)s;
  r.i1 = r.i0 + (r.i0 < n_in - 1 ? 1 : 0);
  r.l = s - T(r.i0);
  return r;
}

// arg max_k of hy (hx p00[k] + lx p01[k]) + ly (hx p10[k] + lx p11[k]), k < K: the first index of the maximum
template <typename T>
__device__ __forceinline__ int bilinear_argmax(const T* p00, const T* p01, const T* p10, const T* p11, T hy, T ly, T hx, T lx, int K) {
  T best = -INFINITY;
  int besti = 0;
  for (int k = 0; k < K; ++k) {
    const T v = hy * (hx * p00[k] + lx * p01[k]) + ly * (hx * p10[k] + lx * p11[k]);
    if (v > best) {
      best = v;
      besti = k;
    }
  }
  return besti;
}

// cubic convolution, A = -0.75: the weights of the taps at floor(r) - 1 ... floor(r) + 2 for the fraction t = r - floor(r)
__device__ __forceinline__ void cubic_coeffs(float t, float (&w)[4]) {
  const float A = -0.75f;
  const float x0 = t + 1.f, x3 = 2.f - t, u = 1.f - t;
  w[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
  w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  w[2] = ((A + 2.f) * u - (A + 3.f)) * u * u + 1.f;
  w[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

}  // namespace tt
