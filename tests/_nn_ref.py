"""Plain restatements of the N31 kernels (csrc/nn_retrieval.hip) and of DenseNNEvaluator.predict, on the CPU.

select      the k best of a set of (similarity, bank index) under the kernel's total order: NaN -> -inf, the columns put into index
            order, ``torch.sort(stable=True, descending=True)`` - among equal values a stable descending sort keeps the ascending
            indices, which is the tie rule - the first k, and every entry whose value is -inf is the empty entry (-inf, -1): a -inf
            similarity ties with the empty entry and loses to its index -1, so it is never selected.
counts      one-hot and a sum over each cell.
aggregate   fp64 softmax over the valid entries and a gather.
predict     select -> aggregate -> bilinear upsampling (align_corners=False) -> first arg-max, from given similarities.
"""
import numpy as np
import torch
import torch.nn.functional as F

NEG_INF = float("-inf")


def select(sims: torch.Tensor, index: torch.Tensor, k: int):
    """sims fp32 [Q, n] (CPU), index int64 [n]: the bank index of each column, all distinct -> (vals fp32 [Q, k], idx int64 [Q, k])."""
    sims, index = sims.detach().cpu().float(), index.detach().cpu().long()
    Q, n = sims.shape
    by_index = torch.argsort(index, stable=True)
    v = sims[:, by_index].clone()
    v[torch.isnan(v)] = NEG_INF
    sv, pos = torch.sort(v, dim=1, descending=True, stable=True)
    vals = torch.full((Q, k), NEG_INF, dtype=torch.float32)
    idx = torch.full((Q, k), -1, dtype=torch.int64)
    m = min(k, n)
    vals[:, :m] = sv[:, :m]
    idx[:, :m] = index[by_index][pos[:, :m]]
    idx[vals == NEG_INF] = -1
    return vals, idx


def select_slow(sims: torch.Tensor, index: torch.Tensor, k: int):
    """The same order written as a comparison sort in plain Python: the partner ``select`` is checked against on small cases."""
    sims, index = sims.detach().cpu().float(), index.detach().cpu().long()
    vals = torch.full((sims.shape[0], k), NEG_INF, dtype=torch.float32)
    idx = torch.full((sims.shape[0], k), -1, dtype=torch.int64)
    for q in range(sims.shape[0]):
        cand = [(float(s), int(i)) for s, i in zip(sims[q].tolist(), index.tolist()) if s == s and s != NEG_INF]
        cand.sort(key=lambda e: (-e[0], e[1]))
        for j, (s, i) in enumerate(cand[:k]):
            vals[q, j], idx[q, j] = s, i
    return vals, idx


def counts(maps: torch.Tensor, g: int, C: int, ignore):
    """maps uint8 [M, R, R] -> (counts int32 [M, g*g, C], valid int32 [M, g*g], first map holding a label >= C that is not ignore, or -1)."""
    maps = maps.detach().cpu().long()
    M, R, _ = maps.shape
    cell = R // g
    keep = torch.ones_like(maps, dtype=torch.bool) if ignore is None else maps != ignore
    bad = keep & (maps >= C)
    first_bad = int(torch.nonzero(bad.flatten(1).any(1)).flatten()[0]) if bad.any() else -1
    keep = keep & ~bad
    onehot = (maps[..., None] == torch.arange(C)) & keep[..., None]                                # [M, R, R, C], as booleans
    cnt = onehot.view(M, g, cell, g, cell, C).sum(dim=(2, 4)).reshape(M, g * g, C)
    return cnt.int(), cnt.sum(-1).int(), first_bad


def aggregate(vals: torch.Tensor, idx: torch.Tensor, labels: torch.Tensor, beta: float) -> torch.Tensor:
    """fp64 [Q, C]: sum_j softmax(vals / beta)_j labels[idx_j] over the entries with 0 <= idx; a zero row where there is none."""
    vals, idx, labels = vals.detach().cpu().double(), idx.detach().cpu().long(), labels.detach().cpu().double()
    ok = idx >= 0
    x = torch.where(ok, vals, torch.full_like(vals, NEG_INF))
    vmax = x.max(dim=1, keepdim=True).values
    e = torch.where(ok, torch.exp((torch.where(ok, vals, vmax) - vmax) / beta), torch.zeros_like(vals))
    s = e.sum(1, keepdim=True)
    w = torch.where(s > 0, e / s.clamp_min(1e-300), torch.zeros_like(e))
    return (w[..., None] * labels[idx.clamp_min(0)]).sum(1)


def upsample_argmax(scores: torch.Tensor, R: int) -> torch.Tensor:
    """scores [B, g*g, C] -> int64 [B, R, R]: bilinear (align_corners=False) in fp64, the FIRST maximum."""
    B, n, C = scores.shape
    g = int(round(n ** 0.5))
    up = F.interpolate(scores.double().view(B, g, g, C).permute(0, 3, 1, 2), size=(R, R), mode="bilinear", align_corners=False)
    best = up.max(dim=1, keepdim=True).values
    return torch.from_numpy(np.argmax((up == best).numpy(), axis=1)).long()   # numpy's argmax: the first of equal maxima


def predict(sims: torch.Tensor, labels: torch.Tensor, B: int, k: int, beta: float, R: int) -> torch.Tensor:
    """sims fp32 [B * n, N]: every query patch against every bank row -> the predicted maps int64 [B, R, R]."""
    N = sims.shape[1]
    vals, idx = select(sims, torch.arange(N), k)
    scores = aggregate(vals, idx, labels, beta).float()
    return upsample_argmax(scores.view(B, -1, labels.shape[1]), R)
