"""Border following (Suzuki & Abe, "Topological structural analysis of digitized binary images by border following", CVGIP 30,
1985, Algorithm 1) as ``cv2.findContours(img, RETR_LIST, CHAIN_APPROX_NONE)`` applies it, restated from the published algorithm for
the BF-score tests (N8) and tools/gen_bfscore_golden.py.  It stands in for cv2, which is not installed: "parity unpinned".

  - Any non-zero pixel is 1; the image is zero-padded by one pixel, so pixels on the image edge are border pixels.
  - 1-pixels are 8-connected, 0-pixels 4-connected.  Every border is followed once, outer borders and hole borders alike
    (RETR_LIST), and every pixel the follower passes is a point (CHAIN_APPROX_NONE): a pixel passed twice appears twice.
  - Raster scan; at a 1-pixel whose left neighbour is 0 an outer border starts (1a), and at a pixel >= 1 whose right neighbour is 0
    a hole border starts (1b).  Both are tested at the same pixel, (1a) first: a one-pixel wall between the background and a hole
    starts both borders (the two transitions of the row are two events of the scan).
  - Points are (x, y) int32, contours [n, 1, 2] as cv2 returns them.

``contour_area`` restates ``cv2.contourArea`` (the absolute shoelace area of the point sequence); it only lets the reference's
``bfscore`` run, nothing reads the areas.
"""
from __future__ import annotations

import numpy as np

# the 8 neighbours (row step, column step) in clockwise order on the screen (rows grow downwards): E, SE, S, SW, W, NW, N, NE.
# Bit k of a neighbourhood index is neighbour k; the HIP kernel uses the same order.
DIRS = ((0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1))
_DIR_OF = {d: k for k, d in enumerate(DIRS)}


def _follow(f, i, j, i2, j2, nbd):
    """Step 3: follow the border through (i, j) starting from its 0-neighbour (i2, j2); marks f in place; -> [(row, col)]."""
    d0 = _DIR_OF[(i2 - i, j2 - j)]
    first = None
    for k in range(8):   # 3.1: clockwise from (i2, j2)
        di, dj = DIRS[(d0 + k) % 8]
        if f[i + di, j + dj] != 0:
            first = (i + di, j + dj)
            break
    if first is None:    # an isolated pixel
        f[i, j] = -nbd
        return [(i, j)]
    pts = []
    prev, cur = first, (i, j)   # 3.2
    while True:
        pts.append(cur)
        dp = _DIR_OF[(prev[0] - cur[0], prev[1] - cur[1])]
        east_zero_examined = False
        for k in range(1, 9):   # 3.3: counterclockwise from the element after prev
            d = (dp - k) % 8
            q = (cur[0] + DIRS[d][0], cur[1] + DIRS[d][1])
            if f[q] != 0:
                nxt = q
                break
            if d == 0:
                east_zero_examined = True
        if east_zero_examined:   # 3.4
            f[cur] = -nbd
        elif f[cur] == 1:
            f[cur] = nbd
        if nxt == (i, j) and cur == first:   # 3.5: back at the start
            return pts
        prev, cur = cur, nxt


def find_contours(img, mode=None, method=None):
    """``cv2.findContours(img, RETR_LIST, CHAIN_APPROX_NONE)`` -> (contours, None); ``mode`` / ``method`` are accepted and ignored."""
    a = np.asarray(img) != 0
    if a.ndim != 2:
        raise ValueError(f"find_contours: a 2-D image is required, got shape {a.shape}")
    H, W = a.shape
    f = np.zeros((H + 2, W + 2), np.int64)
    f[1:-1, 1:-1] = a
    nbd = 1
    contours = []
    for i in range(1, H + 1):
        for j in range(1, W + 1):
            if f[i, j] == 0:
                continue
            if f[i, j] == 1 and f[i, j - 1] == 0:
                nbd += 1
                contours.append(_follow(f, i, j, i, j - 1, nbd))
            if f[i, j] >= 1 and f[i, j + 1] == 0:
                nbd += 1
                contours.append(_follow(f, i, j, i, j + 1, nbd))
    out = [np.array([[[c - 1, r - 1]] for r, c in pts], np.int32).reshape(-1, 1, 2) for pts in contours]
    return out, None


def contour_points(img):
    """All contour points of ``img`` concatenated in cv2's order, as the reference builds them: [(x, y)]."""
    contours, _ = find_contours(img)
    return [tuple(int(v) for v in p[0]) for c in contours for p in c]


def visit_counts(img):
    """int64 [H, W]: how many times the border follower passes each pixel."""
    a = np.asarray(img)
    m = np.zeros(a.shape, np.int64)
    for x, y in contour_points(a):
        m[y, x] += 1
    return m


def contour_area(points, oriented=False):
    p = np.asarray(points, np.float64).reshape(-1, 2)
    if len(p) < 3:
        return 0.0
    x, y = p[:, 0], p[:, 1]
    a = 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))
    return a if oriented else abs(a)


def draw_contours(img, contours, idx, color, thickness=1, *a, **k):
    """The reference draws the contours into an image nobody reads: a no-op."""
    return img


def multiplicity_table():
    """uint8 [256]: the visit count of the centre of a 3 x 3 patch whose centre is set and whose neighbours are the bits of the
    index (bit k = DIRS[k]), from the border follower."""
    tab = np.zeros(256, np.uint8)
    for idx in range(256):
        patch = np.zeros((3, 3), np.uint8)
        patch[1, 1] = 1
        for k, (di, dj) in enumerate(DIRS):
            if idx >> k & 1:
                patch[1 + di, 1 + dj] = 1
        tab[idx] = visit_counts(patch)[1, 1]
    return tab


def neighbourhood_index(a):
    """int64 [H, W]: the 8-bit neighbourhood index of every pixel of the binary map ``a`` (zero-padded)."""
    s = np.asarray(a) != 0
    H, W = s.shape
    p = np.zeros((H + 2, W + 2), bool)
    p[1:-1, 1:-1] = s
    idx = np.zeros((H, W), np.int64)
    for k, (di, dj) in enumerate(DIRS):
        idx |= p[1 + di:1 + di + H, 1 + dj:1 + dj + W].astype(np.int64) << k
    return idx
