"""NumPy restatement of the optical-flow baseline of the reference's evaluation (mask_propagation.py:265-346, :803-815): the 8-bit gray
conversion, OpenCV's dense Farneback flow as ``cv2.calcOpticalFlowFarneback(prev, next, None, pyr_scale, levels, winsize, iterations,
poly_n, poly_sigma, 0)`` computes it on the CPU, the nearest-neighbour label remap and the ``propagate`` chain.

cv2 is not a dependency of this project, so this file stands in for it (as tests/_border_follow.py does for the contour follower): it is
written from OpenCV's algorithm (optflowgf.cpp FarnebackPrepareGaussian / FarnebackPolyExp / FarnebackUpdateMatrices /
FarnebackUpdateFlow_Blur, GaussianBlur with BORDER_REFLECT_101, resize INTER_LINEAR, remap INTER_NEAREST) and parity with cv2 itself is
unpinned.  Arithmetic is fp64 unless ``dtype=np.float32`` is passed (used to size the tests' bounds: the fp32 kernel against fp64).
The box filter is the Jacobi form (every matrix recomputed from the whole new field), which is what OpenCV's row-lagged update amounts
to: a row's matrices are refreshed only after the running sum has passed every row that reads them.  winsize 1 keeps OpenCV's quirk:
its running-sum start counts row / column 0 twice, so the "box" at (y, x) is M(0,0) + M(0,x) + M(y,0) + M(y,x)."""
from __future__ import annotations

import numpy as np

OPTFLOW_USE_INITIAL_FLOW = 4
OPTFLOW_FARNEBACK_GAUSSIAN = 256
MIN_SIZE = 32
BORDER_W = (0.14, 0.14, 0.4472, 0.4472, 0.4472)


def cv_round(x: float) -> int:
    """cvRound: round half to even (the FPU's default mode)."""
    return int(np.rint(x))


def u8_cast(x: np.ndarray) -> np.ndarray:
    """torch's CPU fp32 -> uint8 cast: truncation toward zero, then modulo 256."""
    return (np.trunc(x.astype(np.float32)).astype(np.int64) & 255).astype(np.uint8)


def gray_u8(clip: np.ndarray) -> np.ndarray:
    """clip [F, 3, H, W] fp32 RGB -> uint8 [F, H, W]: ``datum *= 255`` in fp32, the uint8 cast, RGB2BGR then BGR2GRAY's fixed point
    Y = (R 4899 + G 9617 + B 1868 + 8192) >> 14."""
    v = u8_cast(clip.astype(np.float32) * np.float32(255)).astype(np.int64)
    return ((v[:, 0] * 4899 + v[:, 1] * 9617 + v[:, 2] * 1868 + 8192) >> 14).astype(np.uint8)


def plan(H: int, W: int, pyr_scale: float = 0.5, levels: int = 3):
    """(effective levels L, [(h_k, w_k) for k = 0..L]): levels cut where a side would drop below 32, sizes cvRound(side * scale^k)."""
    scale, k = 1.0, 0
    while k < levels:
        scale *= pyr_scale
        if W * scale < MIN_SIZE or H * scale < MIN_SIZE:
            break
        k += 1
    sizes, s = [], 1.0
    for i in range(k + 1):
        sizes.append((cv_round(H * s), cv_round(W * s)))
        s *= pyr_scale
    return k, sizes


def check_params(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags):
    """The parameter rules of the HIP entry point (hip_ops.farneback_flow raises the same)."""
    if flags & (OPTFLOW_USE_INITIAL_FLOW | OPTFLOW_FARNEBACK_GAUSSIAN):
        raise NotImplementedError("OPTFLOW_USE_INITIAL_FLOW / OPTFLOW_FARNEBACK_GAUSSIAN are not part of this build")
    if flags != 0:
        raise ValueError(f"flags {flags}: only 0 is supported")
    for name, v, hi in (("levels", levels, 64), ("winsize", winsize, 127), ("iterations", iterations, 1 << 16)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= hi:
            raise ValueError(f"{name} {v!r}: expected an int in [1, {hi}]")
    if poly_n not in (5, 7) or isinstance(poly_n, bool):
        raise ValueError(f"poly_n {poly_n!r}: expected 5 or 7")
    if not 0.0 < float(pyr_scale) < 1.0:
        raise ValueError(f"pyr_scale {pyr_scale!r}: expected 0 < pyr_scale < 1")
    if not float(poly_sigma) > 0.0 or not np.isfinite(poly_sigma):
        raise ValueError(f"poly_sigma {poly_sigma!r}: expected a positive number")


def gaussian_kernel(ksize: int, sigma: float) -> np.ndarray:
    """getGaussianKernel: the fixed [1/4, 1/2, 1/4] for ksize 3 and sigma <= 0, else exp(-x^2 / 2 sigma^2) normalised."""
    if sigma <= 0 and ksize == 3:
        return np.array([0.25, 0.5, 0.25])
    if sigma <= 0:
        sigma = ((ksize - 1) * 0.5 - 1) * 0.3 + 0.8
    x = np.arange(ksize) - (ksize - 1) * 0.5
    g = np.exp(-x * x / (2 * sigma * sigma))
    return g / g.sum()


def level_blur(pyr_scale: float, k: int):
    """(ksize, sigma) of level k's GaussianBlur."""
    s = pyr_scale ** k
    sigma = (1.0 / s - 1.0) * 0.5
    return max(cv_round(sigma * 5) | 1, 3), sigma


def reflect101(idx: np.ndarray, n: int) -> np.ndarray:
    if n == 1:
        return np.zeros_like(idx)
    idx = np.abs(idx)
    period = 2 * n - 2
    idx = idx % period
    return np.where(idx >= n, period - idx, idx)


def gaussian_blur(img: np.ndarray, ksize: int, sigma: float, dt=np.float64) -> np.ndarray:
    k = gaussian_kernel(ksize, sigma).astype(dt)
    r = ksize // 2
    H, W = img.shape
    off = np.arange(-r, r + 1)
    rows = reflect101(np.arange(H)[:, None] + off[None], H)     # [H, ksize]
    v = np.einsum("hk,hkw->hw", np.broadcast_to(k, (H, ksize)), img.astype(dt)[rows])
    cols = reflect101(np.arange(W)[:, None] + off[None], W)
    return np.einsum("wk,hwk->hw", np.broadcast_to(k, (W, ksize)), v[:, cols])


def _lin_axis(n_src: int, n_dst: int):
    """INTER_LINEAR source indices and weights along one axis (half-pixel centres, clamped at the edges)."""
    scale = n_src / n_dst
    f = (np.arange(n_dst) + 0.5) * scale - 0.5
    s0 = np.floor(f).astype(np.int64)
    w = f - s0
    w = np.where(s0 < 0, 0.0, w)
    s0 = np.maximum(s0, 0)
    w = np.where(s0 >= n_src - 1, 0.0, w)
    s0 = np.minimum(s0, n_src - 1)
    return s0, np.minimum(s0 + 1, n_src - 1), w


def resize_linear(src: np.ndarray, size, dt=np.float64) -> np.ndarray:
    """cv2.resize(src, (w, h), interpolation=INTER_LINEAR) of [h0, w0] or [h0, w0, c]; the same size is a copy."""
    h, w = size
    if src.shape[:2] == (h, w):
        return src.astype(dt).copy()
    y0, y1, wy = _lin_axis(src.shape[0], h)
    x0, x1, wx = _lin_axis(src.shape[1], w)
    s = src.astype(dt)
    if s.ndim == 2:
        s = s[..., None]
    wy, wx = wy.astype(dt)[:, None, None], wx.astype(dt)[None, :, None]
    top = s[y0][:, x0] * (1 - wx) + s[y0][:, x1] * wx
    bot = s[y1][:, x0] * (1 - wx) + s[y1][:, x1] * wx
    out = top * (1 - wy) + bot * wy
    return out if src.ndim == 3 else out[..., 0]


def level_image(gray: np.ndarray, pyr_scale: float, k: int, size, dt=np.float64) -> np.ndarray:
    """Level k's image: the full-resolution frame blurred with level k's Gaussian, resized to ``size``."""
    ksize, sigma = level_blur(pyr_scale, k)
    return resize_linear(gaussian_blur(gray.astype(dt), ksize, sigma if k > 0 else 0.0, dt), size, dt)


def poly_taps(n: int, sigma: float):
    """FarnebackPrepareGaussian: float taps g, xg, xxg over x = -n..n and ig11, ig03, ig33, ig55 of the inverse moment matrix."""
    x = np.arange(-n, n + 1)
    g = np.exp(-(x * x) / (2.0 * sigma * sigma)).astype(np.float32).astype(np.float64)
    g = (g * (1.0 / g.sum())).astype(np.float32).astype(np.float64)
    xg = (x * g).astype(np.float32).astype(np.float64)
    xxg = (x * x * g).astype(np.float32).astype(np.float64)
    gy, gx = np.meshgrid(g, g, indexing="ij")
    Y, X = np.meshgrid(x, x, indexing="ij")
    G = np.zeros((6, 6))
    G[0, 0] = (gy * gx).sum()
    G[1, 1] = (gy * gx * X * X).sum()
    G[3, 3] = (gy * gx * X ** 4).sum()
    G[5, 5] = (gy * gx * X * X * Y * Y).sum()
    G[2, 2] = G[0, 3] = G[0, 4] = G[3, 0] = G[4, 0] = G[1, 1]
    G[4, 4] = G[3, 3]
    G[3, 4] = G[4, 3] = G[5, 5]
    iG = np.linalg.inv(G)
    return g, xg, xxg, (iG[1, 1], iG[0, 3], iG[3, 3], iG[5, 5])


def poly_exp(img: np.ndarray, n: int, sigma: float, dt=np.float64) -> np.ndarray:
    """FarnebackPolyExp: [h, w] -> R [h, w, 5] = (y, x, yy, xx, xy) coefficients, borders replicated."""
    g, xg, xxg, (ig11, ig03, ig33, ig55) = poly_taps(n, sigma)
    g, xg, xxg = g.astype(dt), xg.astype(dt), xxg.astype(dt)
    h, w = img.shape
    s = img.astype(dt)
    ys = np.arange(h)
    r0 = s * g[n]
    r1 = np.zeros_like(s)
    r2 = np.zeros_like(s)
    for k in range(1, n + 1):
        a, b = s[np.maximum(ys - k, 0)], s[np.minimum(ys + k, h - 1)]
        r0 = r0 + g[n + k] * (a + b)
        r1 = r1 + xg[n + k] * (b - a)
        r2 = r2 + xxg[n + k] * (a + b)
    xs = np.arange(w)
    b1, b3, b5 = r0 * g[n], r1 * g[n], r2 * g[n]
    b2 = np.zeros_like(s)
    b4 = np.zeros_like(s)
    b6 = np.zeros_like(s)
    for k in range(1, n + 1):
        L, R = np.maximum(xs - k, 0), np.minimum(xs + k, w - 1)
        b1 = b1 + (r0[:, R] + r0[:, L]) * g[n + k]
        b4 = b4 + (r0[:, R] + r0[:, L]) * xxg[n + k]
        b2 = b2 + (r0[:, R] - r0[:, L]) * xg[n + k]
        b3 = b3 + (r1[:, R] + r1[:, L]) * g[n + k]
        b6 = b6 + (r1[:, R] - r1[:, L]) * xg[n + k]
        b5 = b5 + (r2[:, R] + r2[:, L]) * g[n + k]
    return np.stack([b3 * ig11, b2 * ig11, b1 * ig03 + b5 * ig33, b1 * ig03 + b4 * ig33, b6 * ig55], -1).astype(dt)


def _border_scale(h: int, w: int, dt) -> np.ndarray:
    bw = np.array(BORDER_W, np.float32).astype(dt)

    def axis(n):
        i = np.arange(n)
        s = np.ones(n, dt)
        lo, hi = i < 5, i >= n - 5
        s = np.where(lo, s * bw[np.minimum(i, 4)], s)
        s = np.where(hi, s * bw[np.minimum(n - 1 - i, 4)], s)
        return s

    return axis(h)[:, None] * axis(w)[None, :]


def update_matrices(R0: np.ndarray, R1: np.ndarray, flow: np.ndarray, dt=np.float64) -> np.ndarray:
    """FarnebackUpdateMatrices: M [h, w, 5] = (G11, G12, G22, h1, h2) from R0, R1 sampled at x + flow, and the flow."""
    h, w, _ = R0.shape
    dx, dy = flow[..., 0].astype(dt), flow[..., 1].astype(dt)
    yy, xx = np.mgrid[0:h, 0:w]
    fx, fy = xx + dx, yy + dy
    x1, y1 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    fx, fy = fx - x1, fy - y1
    inside = (x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1)
    xa, ya = np.clip(x1, 0, max(w - 2, 0)), np.clip(y1, 0, max(h - 2, 0))
    xb, yb = np.minimum(xa + 1, w - 1), np.minimum(ya + 1, h - 1)
    a00, a01 = ((1 - fx) * (1 - fy))[..., None], (fx * (1 - fy))[..., None]
    a10, a11 = ((1 - fx) * fy)[..., None], (fx * fy)[..., None]
    R1 = R1.astype(dt)
    R0 = R0.astype(dt)
    r = a00 * R1[ya, xa] + a01 * R1[ya, xb] + a10 * R1[yb, xa] + a11 * R1[yb, xb]
    ins = inside[..., None]
    r4 = np.where(inside, (R0[..., 2] + r[..., 2]) * 0.5, R0[..., 2])
    r5 = np.where(inside, (R0[..., 3] + r[..., 3]) * 0.5, R0[..., 3])
    r6 = np.where(inside, (R0[..., 4] + r[..., 4]) * 0.25, R0[..., 4] * 0.5)
    r01 = np.where(ins, r[..., :2], 0.0)
    r2 = (R0[..., 0] - r01[..., 0]) * 0.5
    r3 = (R0[..., 1] - r01[..., 1]) * 0.5
    r2 = r2 + r4 * dy + r6 * dx
    r3 = r3 + r6 * dy + r5 * dx
    sc = _border_scale(h, w, dt)
    r2, r3, r4, r5, r6 = (v * sc for v in (r2, r3, r4, r5, r6))
    return np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3], -1).astype(dt)


def box(M: np.ndarray, winsize: int, dt=np.float64) -> np.ndarray:
    """The box sum of FarnebackUpdateFlow_Blur over rows / columns [-m, m], m = winsize // 2, borders replicated (not yet scaled);
    m = 0 keeps OpenCV's running-sum start: row / column 0 plus row / column y (x)."""
    m = winsize // 2
    h, w, _ = M.shape
    M = M.astype(dt)
    if m == 0:
        v = M[0:1] + M
        return v[:, 0:1] + v
    ys = np.arange(h)
    v = sum(M[np.clip(ys + i, 0, h - 1)] for i in range(-m, m + 1))
    xs = np.arange(w)
    return sum(v[:, np.clip(xs + i, 0, w - 1)] for i in range(-m, m + 1))


def solve(Mb: np.ndarray, winsize: int, dt=np.float64) -> np.ndarray:
    scale = dt(1.0 / (winsize * winsize))
    g11, g12, g22, h1, h2 = (Mb[..., i] * scale for i in range(5))
    idet = 1.0 / (g11 * g22 - g12 * g12 + dt(1e-3))
    return np.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet], -1).astype(dt)


def farneback(prev: np.ndarray, nxt: np.ndarray, pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2, flags=0,
              dt=np.float64, trace=None) -> np.ndarray:
    """calcOpticalFlowFarneback(prev, next, None, ...) of two uint8 [H, W] frames -> flow [H, W, 2] (dx, dy) with
    prev(x) ~ next(x + flow(x)).  ``trace`` (a dict) receives the level images and expansions of both frames."""
    check_params(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
    H, W = prev.shape
    L, sizes = plan(H, W, pyr_scale, levels)
    flow = None
    for k in range(L, -1, -1):
        h, w = sizes[k]
        if flow is None:
            flow = np.zeros((h, w, 2), dt)
        else:
            flow = resize_linear(flow, (h, w), dt) * dt(1.0 / pyr_scale)
        R = []
        for img in (prev, nxt):
            I = level_image(img, pyr_scale, k, (h, w), dt)
            R.append(poly_exp(I, poly_n, poly_sigma, dt))
            if trace is not None:
                trace.setdefault(k, []).append((I, R[-1]))
        M = update_matrices(R[0], R[1], flow, dt)
        for it in range(iterations):
            flow = solve(box(M, winsize, dt), winsize, dt)
            if it < iterations - 1:
                M = update_matrices(R[0], R[1], flow, dt)
    return flow


def remap_nearest(labels: np.ndarray, flow: np.ndarray, scale: float = 1.0) -> np.ndarray:
    """cv2.remap(labels, coords + scale * flow, None, INTER_NEAREST): the map in float32 as numpy computes it (the scale rounded to
    float32, one multiply, one add), each coordinate rounded half to even and saturated to int16; reads outside the frame give 0."""
    h, w = labels.shape
    yy, xx = np.mgrid[0:h, 0:w]
    coords = np.float32(np.dstack([xx, yy]))
    fl = np.asarray(flow, np.float32)
    pm = coords + np.float32(scale) * fl
    with np.errstate(invalid="ignore"):
        pc = np.clip(np.rint(pm), -32768, 32767)
    pc = np.where(np.isnan(pc), -32768, pc).astype(np.int64)     # cvRound(NaN) is INT_MIN: saturated to -32768, outside
    sx, sy = pc[..., 0], pc[..., 1]
    ok = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    out = np.zeros_like(labels)
    out[ok] = labels[sy[ok], sx[ok]]
    return out


def propagate_chain(first: np.ndarray, flows) -> np.ndarray:
    """The reference's ``propagate`` for one clip: label_{j+1} = remap(label_j, flow_j), each step from the previous result."""
    out, cur = [], first
    for f in flows:
        cur = remap_nearest(cur, f)
        out.append(cur)
    return np.stack(out)
