"""Plain-Python restatement of what ``tt_match_segments`` (csrc/match.hip, N20) computes for ONE segment: the class sets, the score
matrix, the matching (greedy many-to-one, or scipy's rectangular ``linear_sum_assignment`` with its scan order), the remapped counts and
numpy's mean.  Python floats are IEEE doubles and nothing here is contracted, so every value has the bits of the kernel's.  The tests pin
it against ``scipy.optimize.linear_sum_assignment`` and ``PredsmIoU.compute_miou_from_confusion``; it is never the yardstick itself."""
import math

HUNGARIAN, MANY_TO_ONE = 0, 1                                # TT_MATCH_HUNGARIAN, TT_MATCH_MANY_TO_ONE
OK, EMPTY, SEARCH, INEXACT = 0, 1, 2, 3                      # status codes
MAX_GT, MAX_PRED = 128, 1024                                 # the shape rule


def shape_ok(Cg, Cp):
    return 1 <= Cg <= MAX_GT and 1 <= Cp <= MAX_PRED


def lsap(cost):
    """``linear_sum_assignment`` on a list of rows (finite costs), as scipy 1.15 computes it -> (row indices, column indices) sorted by
    row.  The search step is written in the order-free form the kernel uses: the last minimal unassigned position of the list, else
    the first minimal one."""
    n_rows, n_cols = len(cost), len(cost[0])
    transposed = n_cols < n_rows
    if transposed:
        cost = [[cost[i][j] for i in range(n_rows)] for j in range(n_cols)]
    nr, nc = len(cost), len(cost[0])
    u, v = [0.0] * nr, [0.0] * nc
    col4row, row4col = [-1] * nr, [-1] * nc
    for cur in range(nr):
        spc, path = [math.inf] * nc, [-1] * nc
        in_row, in_col = [False] * nr, [False] * nc
        remaining = [nc - 1 - t for t in range(nc)]
        min_val, i, sink, steps = 0.0, cur, -1, 0
        while sink < 0:
            steps += 1
            assert steps <= nc, "search overran its bound"
            in_row[i] = True
            for j in remaining:
                r = min_val + cost[i][j] - u[i] - v[j]
                if r < spc[j]:
                    spc[j], path[j] = r, i
            lowest = min(spc[j] for j in remaining)
            assert math.isfinite(lowest)
            minimal = [t for t, j in enumerate(remaining) if spc[j] == lowest]
            free = [t for t in minimal if row4col[remaining[t]] < 0]
            pos = free[-1] if free else minimal[0]
            min_val, j = lowest, remaining[pos]
            if row4col[j] < 0:
                sink = j
            else:
                i = row4col[j]
            in_col[j] = True
            remaining[pos] = remaining[-1]
            remaining.pop()
        u[cur] += min_val
        for i in range(nr):
            if in_row[i] and i != cur:
                u[i] += min_val - spc[col4row[i]]
        for j in range(nc):
            if in_col[j]:
                v[j] -= min_val - spc[j]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    if transposed:
        pairs = sorted((col4row[i], i) for i in range(nr))
    else:
        pairs = [(i, col4row[i]) for i in range(nr)]
    return [a for a, _ in pairs], [b for _, b in pairs]


def numpy_mean(a):
    """``np.mean`` of at most 128 doubles: numpy's pairwise sum is one block there - eight strided accumulators from 8 values up."""
    n = len(a)
    assert 1 <= n <= 128
    if n < 8:
        s = a[0]                                              # numpy starts from -0.0: -0.0 + a[0] has a[0]'s bits (a[0] >= +0.0)
        for x in a[1:]:
            s = s + x
    else:
        r = list(a[:8])
        whole = n - n % 8
        for k in range(8, whole, 8):
            for t in range(8):
                r[t] = r[t] + a[k + t]
        s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for x in a[whole:]:
            s = s + x
    return s / n


def match_segment(counts, mode, precision_based, involve_bg):
    """counts: Cg rows of Cp non-negative ints -> dict(status, score, matched_bg, tp, fp, fn (lists of Cg ints), lut (list of Cp ints),
    n_gt, n_pred, pred_max), the outputs of ``tt_match_segments`` for this segment."""
    Cg, Cp = len(counts), len(counts[0])
    rows = [sum(r) for r in counts]
    cols = [sum(counts[g][p] for g in range(Cg)) for p in range(Cp)]
    gts = [g for g in range(Cg) if rows[g] > 0]
    preds = [p for p in range(Cp) if cols[p] > 0]
    out = dict(status=OK, score=0.0, matched_bg=0.0, tp=[0] * Cg, fp=[0] * Cg, fn=[0] * Cg, lut=[0] * Cp, n_gt=len(gts), n_pred=len(preds),
               pred_max=preds[-1] if preds else 0)
    if not gts:
        out["status"] = EMPTY
        return out
    if sum(rows) >= 2 ** 53:
        out["status"] = INEXACT
        return out

    def score(g, p, precision):
        tp = float(counts[g][p])
        fp = float(cols[p]) - tp
        if precision:
            return tp / max(tp + fp, 1e-8)
        fn = float(rows[g]) - tp
        return tp / max(tp + fp + fn, 1e-8)

    target = {}                                               # pred value -> gt value
    if mode == MANY_TO_ONE:
        to_first = 0
        for p in preds:
            best, best_g = -1.0, gts[0]
            for g in gts:
                s = score(g, p, precision_based)
                if s > best:
                    best, best_g = s, g
            target[p] = best_g
            to_first += best_g == gts[0]
        out["matched_bg"] = to_first / len(preds)
    else:
        ri, ci = lsap([[1.0 - score(g, p, False) for p in preds] for g in gts])
        for a, b in zip(ri, ci):
            target[preds[b]] = gts[a]
        out["matched_bg"] = 1 / len(gts)
    jac = []
    for g in gts:
        mapped = [p for p in preds if target.get(p, 0) == g]
        tp = sum(counts[g][p] for p in mapped)
        fp = sum(cols[p] for p in mapped) - tp
        fn = rows[g] - tp
        out["tp"][g], out["fp"][g], out["fn"][g] = tp, fp, fn
        if involve_bg or g != 0:
            jac.append(float(tp) / max(float(tp + fp + fn), 1e-8))
    out["score"] = numpy_mean(jac) if jac else 0.0
    for p, g in target.items():
        out["lut"][p] = g
    return out


KINDS = ("small", "one_cell", "equal", "sparse", "dense", "diagonal", "no_bg", "only_bg")


def draw_counts(rng, Cg, Cp, kind):
    """One [Cg, Cp] int64 count matrix (numpy) of a named kind, never all zero:
    small     counts in {0, 1, 2}: ties everywhere;         one_cell  a single non-zero cell;
    equal     every cell the same;                          sparse    one cell in five non-zero, some rows and columns absent;
    dense     every cell up to 1000;                        diagonal  a noisy many-to-one structure, as real predictions have;
    no_bg     dense with gt value 0 absent;                 only_bg   gt value 0 alone present."""
    import numpy as np

    if kind == "small":
        c = rng.integers(0, 3, (Cg, Cp))
    elif kind == "one_cell":
        c = np.zeros((Cg, Cp), np.int64)
        c[rng.integers(Cg), rng.integers(Cp)] = rng.integers(1, 50)
    elif kind == "equal":
        c = np.full((Cg, Cp), int(rng.integers(1, 9)))
    elif kind == "sparse":
        c = rng.integers(1, 200, (Cg, Cp)) * (rng.random((Cg, Cp)) < 0.2)
        c[rng.random(Cg) < 0.3] = 0
        c[:, rng.random(Cp) < 0.3] = 0
    elif kind == "dense":
        c = rng.integers(0, 1000, (Cg, Cp))
    elif kind == "diagonal":
        c = rng.integers(0, 3, (Cg, Cp)) * (rng.random((Cg, Cp)) < 0.3)
        c[rng.integers(0, Cg, Cp), np.arange(Cp)] += rng.integers(0, 400, Cp)
    elif kind == "no_bg":
        c = rng.integers(0, 1000, (Cg, Cp))
        c[0] = 0
    elif kind == "only_bg":
        c = np.zeros((Cg, Cp), np.int64)
        c[0] = rng.integers(0, 30, Cp)
    else:
        raise ValueError(kind)
    c = np.asarray(c, np.int64)
    if not c.any():
        c[Cg - 1 if kind == "no_bg" and Cg > 1 else 0, rng.integers(Cp)] = 3
    return c


def as_compute_tuple(counts, out, with_mapping):
    """The tuple ``compute_miou_from_confusion`` returns, rebuilt from the flat outputs (what ``PredsmIoU.compute_segments`` does)."""
    import torch

    gts = [g for g in range(len(counts)) if sum(counts[g]) > 0]
    tp, fp, fn = ({g: out[k][g] for g in gts} for k in ("tp", "fp", "fn"))
    table = torch.tensor(out["lut"][: out["pred_max"] + 1], dtype=torch.int64) if with_mapping else None
    return out["score"], tp, fp, fn, table, out["matched_bg"]
