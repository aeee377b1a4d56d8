"""Evaluator clustering with the reference's surface (``clustering.py:20-117``, ``my_utils.py:19-37``) on the HIP kernels.

``cluster_features`` / ``proto_clustering`` / ``normalize_and_transform`` keep the reference's names, arguments and output
layouts.  The reference leans on two third-party CPU libraries here: scikit-learn's ``StandardScaler`` and faiss
(``PCAMatrix``, ``Kmeans``).  Their published algorithms are restated on the GPU:

* StandardScaler        per-column mean / population variance (``tt_col_moments``), scale = sqrt(var) with zeros -> 1
                        (pinned: tests/golden/scaler.npz is the reference's run with the real scikit-learn)
* faiss.PCAMatrix(d, p) eigenvectors of the covariance of the (standardised) data, largest eigenvalues first; the p x d basis
                        comes from a d x d eigen-problem solved on the host in fp64, the Gram matrix and the projection are
                        device GEMMs.  Component SIGNS are LAPACK's choice in faiss; here each row is oriented so that its
                        largest-magnitude entry is positive.  k-means is invariant to that.
* faiss.Kmeans          Clustering::train of faiss 1.7.2 with the reference's parameters (niter 50, nredo 5, seed 1,
                        max_points_per_centroid 256, min 39): random subsample of k * 256 points, k random points as initial
                        centroids per redo, Lloyd iterations (assignment + mean), empty clusters re-seeded by splitting a
                        large one (perturbation 1/1024), best objective over the redos kept.  faiss' own RNG stream is not
                        reproduced (``torch.Generator`` / ``numpy.RandomState`` with the same seed formulas), so cluster ids
                        and, on hard data, the local optimum can differ from a faiss run: parity here is "unpinned" and the
                        tests check the algorithm against a NumPy restatement fed with the same random draws.

The frame-wise and sample-wise protocols fit all their problems of one k in one launch (``KmeansBatch``, N13).  The split of empty
clusters draws from ``numpy.RandomState(1234)``, re-created at every call; ``split_draws`` holds that one sequence as a table, with which
the fused kernel splits on the device (N18: ``KmeansBatch(split="device")``, ``split_empty_from_table`` is its host statement), so a
masked evaluation batch, whose every fit meets empty clusters, stays off the host-driven loop.

The large fits - the dataset-wise protocol, the over-clustering at k = 500, the over-clustering of cluster-based foreground extraction on
384 raw columns - do not fit the fused kernel's LDS.  ``Kmeans(loop="device")`` (N28) enqueues their whole Lloyd loop, split included, on
the stream (``ops.kmeans_fit_loop``: the loop's own kernels with the redo on a grid axis) and reads the objectives and status words
back once; ``DEVICE_LOOP`` routes the callers.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import hip_ops as ops


# ------------------------------------------------------------------------------------------------
# StandardScaler + PCA  (my_utils.py:19-37)
# ------------------------------------------------------------------------------------------------

def fit_scaler_pca(feats: torch.Tensor, pca_dim: int):
    """feats [n, dim] on the GPU -> (scale_mul [dim], scale_shift [dim], z_mean [dim], basis [pca_dim, dim], z [n, dim]) with
    ``z = feats * scale_mul + scale_shift`` (the standardised features) such that ``(z - z_mean) @ basis.T`` is
    ``normalize_and_transform(feats, pca_dim)``."""
    n, dim = feats.shape
    mean, var = ops.col_moments(feats)
    scale = var.sqrt()
    scale = torch.where(scale < 10 * torch.finfo(torch.float64).eps, torch.ones_like(scale), scale)  # sklearn _handle_zeros_in_scale
    mul = (1.0 / scale).float()
    shift = (-mean / scale).float()
    z = ops.affine_cols_(feats.clone(), mul, shift)
    gram, _ = ops.linear_bwd_weight(z, z, need_bias=False)                    # Z^T Z  [dim, dim]
    zmean, _ = ops.col_moments(z)
    cov = gram.double() / n - torch.outer(zmean, zmean)
    evals, evecs = torch.linalg.eigh(cov.cpu())                               # ascending
    basis = evecs[:, torch.argsort(evals, descending=True)[:pca_dim]].t().contiguous()  # [pca_dim, dim]
    lead = basis.abs().argmax(dim=1)
    basis = basis * torch.sign(basis[torch.arange(basis.shape[0]), lead]).unsqueeze(1)
    return mul, shift, zmean.float(), basis.float().to(feats.device), z


def normalize_and_transform(feats: torch.Tensor, pca_dim: int) -> torch.Tensor:
    """``my_utils.normalize_and_transform``: StandardScaler then PCA to ``pca_dim`` dims; stays on the device."""
    _, _, zmean, basis, z = fit_scaler_pca(feats.contiguous().float(), pca_dim)
    return ops.linear_fwd(z, basis, -(basis @ zmean))                         # A (z - mean_z)


# ------------------------------------------------------------------------------------------------
# k-means  (faiss.Kmeans as the reference configures it)
# ------------------------------------------------------------------------------------------------

def _check_n(n: int, k: int) -> None:
    if n < k:
        raise RuntimeError(f"Number of training points ({n}) should be at least as large as number of clusters ({k})")


def _subsample_rows(n: int, k: int, seed: int, max_points_per_centroid: int) -> Optional[torch.Tensor]:
    """faiss subsample_training_set: the rows kept of n training points (host int64), or None where all of them are.  The draw depends
    on (n, seed) alone."""
    return Kmeans._perm(n, seed)[: k * max_points_per_centroid] if n > k * max_points_per_centroid else None


def _redo_seeds(n: int, k: int, seed: int, nredo: int, init_indices=None) -> torch.Tensor:
    """int64 [nredo, k]: the rows of the n (subsampled) points that seed each redo - faiss' draw, or the first nredo rows of
    ``init_indices`` where given (all of one length: they are stacked before the first redo)."""
    if init_indices is not None:
        return torch.stack([torch.as_tensor(init_indices[r], dtype=torch.int64) for r in range(nredo)])
    return torch.stack([Kmeans._perm(n, seed + 1 + r * 15486557)[:k] for r in range(nredo)])


class Kmeans:
    """``faiss.Kmeans(d, k, niter=50, nredo=5, seed=1, verbose=False, gpu=False, spherical=False)`` surface: ``train(x)``,
    ``centroids`` ([k, d] numpy, as faiss exposes them), ``assign(x) -> (dist2, labels)`` in place of ``index.search(x, 1)``.

    ``loop`` says who drives the Lloyd iterations.  ``"host"``: ``_iterate``, a dozen launches and two synchronisations per iteration.
    ``"device"`` (N28): where ``ops.kmeans_loop_shape_ok`` takes the (subsampled) shape, every redo and iteration is enqueued at once
    (``ops.kmeans_fit_loop``, empty clusters split from the table of ``split_draws``) and the objectives and status words are read
    back once.  Per redo the arithmetic is ``_iterate``'s, so the centroids are the same bits - with one reservation: the per-redo
    objective is the kernel's own fixed-order fp64 sum, not torch's reduction (they agree to about n * 2^-53 relative), so the redo
    kept can differ where two DISTINCT objectives lie that close.  A fit in which any redo ended with a non-zero status (one split call
    needed more draws than the table holds), or whose shape the rule refuses, runs the unchanged host loop on the same subsample and
    seeds.  ``loop_workspace_bytes`` bounds the device loop's workspace: as many redos ride one launch as fit it, at least one (the
    result does not depend on it; ``redo_group`` says how many did).  ``status`` [nredo] is the device loop's (None where it did not run), ``fallback`` whether the host loop fitted after it."""

    def __init__(self, d: int, k: int, niter: int = 50, nredo: int = 5, seed: int = 1, verbose: bool = False, gpu: bool = False,
                 spherical: bool = False, max_points_per_centroid: int = 256, loop: str = "host", loop_workspace_bytes: Optional[int] = None):
        if spherical:
            raise NotImplementedError("spherical k-means is not used by the reference")
        if loop not in ("host", "device"):
            raise ValueError(f"Kmeans: loop = {loop!r}: expected 'host' or 'device'")
        self.loop = loop
        self.loop_workspace_bytes = loop_workspace_bytes   # None = LOOP_WORKSPACE_BYTES
        self.status: Optional[np.ndarray] = None
        self.fallback = False
        self.redo_group: Optional[int] = None   # redos per launch of the last device loop
        self.d, self.k, self.niter, self.nredo, self.seed = d, k, niter, nredo, seed
        self.max_points_per_centroid = max_points_per_centroid
        self.centroids: Optional[np.ndarray] = None
        self._centroids_dev: Optional[torch.Tensor] = None
        self.obj: list = []

    @staticmethod
    def _perm(n: int, seed: int) -> torch.Tensor:
        return torch.randperm(n, generator=torch.Generator().manual_seed(seed % (2 ** 63)))

    def _split_empty(self, cent: torch.Tensor, counts: np.ndarray, n: int) -> int:
        """faiss split_clusters: every empty cluster takes over half of a donor picked with probability proportional to its
        size; the two copies are perturbed in opposite directions by 1/1024."""
        k, d = cent.shape
        rng = np.random.RandomState(1234)
        eps = 1.0 / 1024.0
        sign = torch.tensor([1.0 + eps if j % 2 == 0 else 1.0 - eps for j in range(d)], device=cent.device)
        nsplit = 0
        for ci in range(k):
            if counts[ci] != 0:
                continue
            if n <= k or counts.max() <= 1:
                break   # nothing left to split (n == k, or every cluster holds at most one point): faiss' loop would never accept
            cj, tries = 0, 0
            while True:  # (counts[cj] - 1) / (n - k) acceptance, as faiss
                p = (counts[cj] - 1.0) / float(n - k)
                if rng.random_sample() < p:
                    break
                cj = (cj + 1) % k
                tries += 1
                if tries > 64 * k:   # vanishing acceptance (duplicates everywhere): take the largest cluster instead of spinning
                    cj = int(np.argmax(counts))
                    break
            cent[ci] = cent[cj] * sign
            cent[cj] = cent[cj] * (2.0 - sign)
            counts[ci] = counts[cj] // 2
            counts[cj] -= counts[ci]
            nsplit += 1
        return nsplit

    def train(self, x, init_indices=None) -> float:
        """x [n, d] (GPU tensor, or numpy like faiss).  ``init_indices`` [nredo, k] optionally fixes the initial centroids
        (testing aid).  Returns the best objective."""
        x = torch.as_tensor(x, dtype=torch.float32)
        if not x.is_cuda:
            x = x.cuda()
        x = x.contiguous()
        n = x.shape[0]
        _check_n(n, self.k)
        rows = _subsample_rows(n, self.k, self.seed, self.max_points_per_centroid)
        if rows is not None:
            x = x[rows.to(x.device)].contiguous()
        return self._fit(x, init_indices)

    # -- the two kernel pairs ----------------------------------------------------------------------------------------------------------
    # ``kmeans_assign`` / ``kmeans_accumulate`` hold all centroids in LDS and take what ``kmeans_shape_ok`` says (k * d <= 16384: k <= 327
    # at the 50 PCA columns of cluster_features); ``kmeans_assign_tiled`` / ``kmeans_accumulate_tiled`` pass them through LDS in tiles and
    # take any k.  Where both run they return the same bits, so the route does not show in a result; a shape the resident pair takes
    # stays on it.

    def _kernels(self, d: int):
        """(assign, accumulate) for self.k centroids of d columns; a shape neither pair takes is refused here, before any launch."""
        if ops.kmeans_shape_ok(d, self.k):
            return ops.kmeans_assign, ops.kmeans_accumulate
        if not ops.kmeans_tiled_shape_ok(d, self.k):
            raise ops._lib.HipLibraryError(f"Kmeans: k = {self.k} centroids of d = {d} columns are beyond what the tiled k-means kernels "
                                           "take (1 <= d <= 1024, k >= 1, k * d < 2^31)")
        return ops.kmeans_assign_tiled, ops.kmeans_accumulate_tiled

    def _fit(self, x: torch.Tensor, init_indices=None, *, _draws: Optional[torch.Tensor] = None) -> float:
        """The fit of the (subsampled) training points x [n, d].  ``_draws``: another table than ``split_draws()`` for ``loop="device"``
        (testing aid: a table that is too short)."""
        n, d = x.shape
        self.status, self.fallback = None, False
        if self.loop == "device" and ops.kmeans_loop_shape_ok(n, d, self.k):
            if self._fit_device(x, init_indices, _draws):
                return min(self.obj)
            self.fallback = True
        return self._iterate(x, init_indices, *self._kernels(d))

    def _fit_device(self, x: torch.Tensor, init_indices, draws) -> bool:
        """The device loop: fills ``centroids``, ``_centroids_dev``, ``obj`` and ``status``; False where a redo's status is non-zero."""
        n, d = x.shape
        init = _redo_seeds(n, self.k, self.seed, self.nredo, init_indices).to(torch.int32)
        table = split_draws(device=x.device) if draws is None else draws
        budget = LOOP_WORKSPACE_BYTES if self.loop_workspace_bytes is None else self.loop_workspace_bytes
        group = self.nredo   # all redos in one pass where their workspace fits the budget, else as many as do, at least one
        while group > 1 and ops.kmeans_loop_workspace_bytes(n, d, self.k, self.nredo, group) > budget:
            group -= 1
        self.redo_group = group
        cent, obj, status = ops.kmeans_fit_loop(x, init, self.niter, table, redo_group=group)
        host = torch.cat([obj, status.to(torch.float64)]).cpu().numpy()   # the one read-back
        obj_h, status_h = host[: self.nredo], host[self.nredo:]
        self.status = status_h.astype(np.int32)
        if (status_h != 0).any():
            return False
        best, best_r = float("inf"), 0
        for r in range(self.nredo):   # the loop's ``obj < best_obj``: the first redo with the strictly smallest objective
            if float(obj_h[r]) < best:
                best, best_r = float(obj_h[r]), r
        self.obj = [float(o) for o in obj_h]
        self._centroids_dev = cent[best_r].clone()
        self.centroids = self._centroids_dev.cpu().numpy()
        return True

    def _lloyd(self, x: torch.Tensor, init_indices=None) -> float:
        """The redos of Lloyd iterations on the (subsampled) training points x [n, d], on the resident pair only."""
        d, k = x.shape[1], self.k
        if not ops.kmeans_shape_ok(d, k):   # refused here, not after the first assignment: both kernels share this rule
            raise ops._lib.HipLibraryError(f"Kmeans: k = {k} centroids of d = {d} columns are beyond what the k-means kernels hold in LDS "
                                       "(k * d <= 16384; at d = 64, k <= 252)")
        return self._iterate(x, init_indices, ops.kmeans_assign, ops.kmeans_accumulate)

    def _iterate(self, x: torch.Tensor, init_indices, assign, accumulate) -> float:
        """The Lloyd loop both drivers share; ``assign`` / ``accumulate`` are the kernel pair."""
        n, d = x.shape
        k = self.k
        best_obj, best = float("inf"), None
        self.obj = []
        for idx in _redo_seeds(n, k, self.seed, self.nredo, init_indices):
            cent = x[idx.to(x.device)].clone()
            obj = float("inf")
            for _ in range(self.niter):
                labels, dist2 = assign(x, cent, return_dist=True)
                obj = float(dist2.double().sum())
                sums, counts = accumulate(x, labels, k)
                counts_h = counts.cpu().numpy().copy()
                nonempty = counts > 0
                cent = torch.where(nonempty.unsqueeze(1), (sums / counts.clamp(min=1).unsqueeze(1)).float(), cent)
                if (counts_h == 0).any():
                    self._split_empty(cent, counts_h, n)
            self.obj.append(obj)
            if obj < best_obj:
                best_obj, best = obj, cent.clone()
        self._centroids_dev = best
        self.centroids = best.cpu().numpy()
        return best_obj

    def assign(self, x):
        x = torch.as_tensor(x, dtype=torch.float32)
        if not x.is_cuda:
            x = x.cuda()
        labels, dist2 = self._kernels(x.shape[1])[0](x.contiguous(), self._centroids_dev, return_dist=True)
        return dist2, labels.long()

    # -- points that are the nearest upsampling of token grids ---------------------------------------------------------------------
    # Nearest upsampling from a g x g token grid to R x R only repeats token vectors: point (m, y, x) of the upsampled set is token
    # (m, iy[y], ix[x]).  The two methods below take the tokens [M, g*g, d] and never build the [M * R * R, d] points; the training
    # subsample gathers the same rows ``train`` would pick from the materialised tensor (flattened as (m, y, x), the reference's
    # create_overclustering_maps layout, cluster_based_foreground_extraction.py:268-279), and the assignment runs once per token.
    # Labels and centroids are bit-identical to ``train`` / ``assign`` on the materialised tensor; faiss parity stays unpinned.

    def _virtual_rows(self, p: torch.Tensor, M: int, g: int, R: int) -> torch.Tensor:
        iy, ix = nearest_index_table(g, R)
        iy, ix = torch.from_numpy(iy.astype(np.int64)), torch.from_numpy(ix.astype(np.int64))
        m, rem = p // (R * R), p % (R * R)
        return m * (g * g) + iy[rem // R] * g + ix[rem % R]

    def train_upsampled(self, tokens: torch.Tensor, resolution: int, init_indices=None) -> float:
        """``train`` on the nearest upsampling of tokens [M, g*g, d] to resolution x resolution, without materialising it."""
        tokens = torch.as_tensor(tokens, dtype=torch.float32)   # (tokens on the host stay there: only the subsample moves)
        M, n_tok, d = tokens.shape
        g = int(round(n_tok ** 0.5))
        if g * g != n_tok:
            raise ValueError(f"train_upsampled: {n_tok} tokens are not a square grid")
        R = int(resolution)
        n = M * R * R
        _check_n(n, self.k)
        p = _subsample_rows(n, self.k, self.seed, self.max_points_per_centroid)
        rows = self._virtual_rows(torch.arange(n) if p is None else p, M, g, R).to(tokens.device)
        x = tokens.reshape(M * n_tok, d)[rows].cuda().contiguous()
        return self._fit(x, init_indices)

    def assign_upsampled(self, tokens: torch.Tensor, resolution: int) -> torch.Tensor:
        """Labels int64 [M, R*R] of the nearest upsampling of tokens [M, g*g, d]: one assignment per token, then the labels are
        upsampled (tt_nearest_upsample_labels)."""
        tokens = torch.as_tensor(tokens, dtype=torch.float32)
        if not tokens.is_cuda:
            tokens = tokens.cuda()
        M, n_tok, d = tokens.shape
        g = int(round(n_tok ** 0.5))
        labels = self._kernels(d)[0](tokens.reshape(M * n_tok, d).contiguous(), self._centroids_dev)
        iy, ix = nearest_index_table(g, resolution, device=tokens.device)
        return ops.nearest_upsample_labels(labels.view(M, n_tok), iy, ix)


# -- the split of empty clusters as a table walk (N18) -------------------------------------------------------------------------------
# ``Kmeans._split_empty`` re-creates ``numpy.random.RandomState(1234)`` at every call, so every call consumes a prefix of ONE fixed
# sequence.  With that sequence in a table the split needs no generator: ``split_empty_from_table`` is ``_split_empty`` stated that way
# on the host (the tests hold the two to each other), and kf_split_empty of csrc/kmeans_fit.hip is the same statement in the kernel.

DEVICE_SPLIT = True          # _kmeans_maps_grouped builds KmeansBatch(split="device"); False forces the fall-back to the loop
DEVICE_LOOP = True           # the dataset-wise fit and create_overclustering_maps build Kmeans(loop="device"); False = the host loop
LOOP_WORKSPACE_BYTES = 1 << 30   # what the redos in flight of a device loop may take (200 MB each at n = 128 000, d = 50, k = 500)
SPLIT_DRAWS = 4096           # ten times the most one _split_empty call was seen to draw at the evaluator's shapes (393, at k = 21)
_split_tables: dict = {}


def split_draws(n_draws: int = SPLIT_DRAWS, device=None) -> torch.Tensor:
    """float64 [n_draws]: the first values of ``numpy.random.RandomState(1234).random_sample()`` - what ``_split_empty`` draws, in its
    order.  On ``device`` (default: the host); one tensor per (device, n_draws), built once."""
    key = (str(torch.device("cpu" if device is None else device)), int(n_draws))
    if key not in _split_tables:
        _split_tables[key] = torch.from_numpy(np.random.RandomState(1234).random_sample(int(n_draws))).to(key[0])
    return _split_tables[key]


def split_empty_from_table(cent: torch.Tensor, counts: np.ndarray, n: int, draws) -> int:
    """``Kmeans._split_empty(cent, counts, n)`` with the generator's draws read from ``draws`` (float64, ``split_draws``), from index 0:
    ``cent`` [k, d] and ``counts`` [k] are changed the same way.  Returns the number of splits, or -1 where a draw beyond the table was
    needed (``cent`` and ``counts`` are then part-way through the call).  The kernel's split is written against this function."""
    k, d = cent.shape
    draws = np.asarray(draws.cpu() if isinstance(draws, torch.Tensor) else draws, dtype=np.float64)
    eps = 1.0 / 1024.0
    sign = torch.tensor([1.0 + eps if j % 2 == 0 else 1.0 - eps for j in range(d)], device=cent.device)
    nsplit, nxt = 0, 0
    for ci in range(k):
        if counts[ci] != 0:
            continue
        if n <= k or counts.max() <= 1:
            break
        cj, tries = 0, 0
        while True:
            if nxt >= len(draws):
                return -1
            p = (counts[cj] - 1.0) / float(n - k)
            nxt += 1
            if draws[nxt - 1] < p:
                break
            cj = (cj + 1) % k
            tries += 1
            if tries > 64 * k:
                cj = int(np.argmax(counts))
                break
        cent[ci] = cent[cj] * sign
        cent[cj] = cent[cj] * (2.0 - sign)
        counts[ci] = counts[cj] // 2
        counts[cj] -= counts[ci]
        nsplit += 1
    return nsplit


class KmeansBatch:
    """``Kmeans(d, k, ...)`` for B problems of equal shape at once: ``train(points [B, n, d])`` runs every problem's redos and Lloyd
    iterations in ONE launch (``ops.kmeans_fit_batched``) and reads the objectives and the empty-cluster flags back once.  Per problem
    the subsample, the seeds and the arithmetic are those of ``Kmeans.train``, so the centroids are the same bits - with one
    reservation: the per-redo objective is the kernel's own fixed-order fp64 sum, not torch's reduction (they agree to about
    n * 2^-53 relative), so the redo kept can differ where two DISTINCT objectives lie that close.

    ``split`` says who splits an empty cluster.  ``"host"``: a problem in which any redo met one is rerun whole on the loop
    (``Kmeans._fit``), which knows faiss' split.  ``"device"`` (N18): the flagged problems - those alone, so a batch without empty
    clusters is the one launch it was - are fitted again by the kernel that splits from the table of ``split_draws``, and only a
    problem whose status is still non-zero, because one split call needed more draws than the table holds, goes to the loop.
    ``fallback`` says which problems the loop fitted; ``status`` is that of the last launch that fitted the problem."""

    def __init__(self, d: int, k: int, niter: int = 50, nredo: int = 5, seed: int = 1, max_points_per_centroid: int = 256, split: str = "host"):
        if split not in ("host", "device"):
            raise ValueError(f"KmeansBatch: split = {split!r}: expected 'host' or 'device'")
        self.d, self.k, self.niter, self.nredo, self.seed = d, k, niter, nredo, seed
        self.max_points_per_centroid = max_points_per_centroid
        self.split = split
        self.centroids: Optional[torch.Tensor] = None   # [B, k, d] on the device
        self.obj: list = []                             # per problem, the per-redo objectives (as Kmeans.obj)
        self.fallback: list = []                        # per problem, whether the loop replaced the kernel's result
        self.status: Optional[np.ndarray] = None        # [B, nredo]: 0, or the iteration at which the kernel ended that redo

    def _read_back(self, obj: torch.Tensor, status: torch.Tensor):
        host = torch.cat([obj, status.to(torch.float64)], dim=1).cpu().numpy()   # one read-back per launch
        return host[:, : self.nredo], host[:, self.nredo:]

    def train(self, points, init_indices=None, *, _draws: Optional[torch.Tensor] = None) -> list:
        """points [B, n, d].  ``init_indices`` [nredo, k] optionally fixes the initial centroids of every problem (testing aid).
        ``_draws``: another table than ``split_draws()`` for ``split="device"`` (testing aid: a table that is too short).
        Returns the best objective of each problem."""
        x = torch.as_tensor(points, dtype=torch.float32)
        if not x.is_cuda:
            x = x.cuda()
        B, n, d = x.shape
        k = self.k
        _check_n(n, k)
        rows = _subsample_rows(n, k, self.seed, self.max_points_per_centroid)   # shared by all problems
        if rows is not None:
            x = x[:, rows.to(x.device)]
        x = x.contiguous()
        init = _redo_seeds(x.shape[1], k, self.seed, self.nredo, init_indices)
        cent, obj, status = ops.kmeans_fit_batched(x, init.to(torch.int32), self.niter)
        obj_h, status_h = self._read_back(obj, status)
        flagged = [b for b in range(B) if (status_h[b] != 0).any()]
        if flagged and self.split == "device":   # those problems again, whole, on the kernel that splits
            table = split_draws(device=x.device) if _draws is None else _draws
            sel = torch.as_tensor(flagged, device=x.device)
            c2, o2, s2 = ops.kmeans_fit_batched(x if len(flagged) == B else x[sel].contiguous(), init.to(torch.int32), self.niter, table)
            cent[sel] = c2
            obj_h[flagged], status_h[flagged] = self._read_back(o2, s2)
        self.status = status_h.astype(np.int32)
        self.obj, self.fallback, best_obj, pick = [], [], [], []
        for b in range(B):
            self.fallback.append(bool((status_h[b] != 0).any()))
            best, best_r = float("inf"), 0
            for r in range(self.nredo):   # the loop's ``obj < best_obj``: the first redo with the strictly smallest objective
                if float(obj_h[b, r]) < best:
                    best, best_r = float(obj_h[b, r]), r
            self.obj.append([float(o) for o in obj_h[b]])
            best_obj.append(best)
            pick.append(best_r)
        self.centroids = cent[torch.arange(B, device=cent.device), torch.as_tensor(pick, device=cent.device)].contiguous()
        for b in range(B):
            if self.fallback[b]:   # the unchanged loop on the very subsample and seeds
                km = Kmeans(d, k, niter=self.niter, nredo=self.nredo, seed=self.seed, max_points_per_centroid=self.max_points_per_centroid)
                best_obj[b] = km._fit(x[b], init)
                self.centroids[b] = km._centroids_dev
                self.obj[b] = list(km.obj)
        return best_obj

    def assign(self, points):
        """points [B, N, d] -> (dist2 [B, N], labels int64 [B, N]) against each problem's own centroids."""
        x = torch.as_tensor(points, dtype=torch.float32)
        if not x.is_cuda:
            x = x.cuda()
        labels, dist2 = ops.kmeans_assign_batched(x.contiguous(), self.centroids, return_dist=True)
        return dist2, labels.long()


def nearest_index_table(g: int, R: int, device=None):
    """Row / column source indices of ``F.interpolate(mode="nearest")`` from g x g to R x R, read off torch itself (an index grid
    interpolated on the host): int32 numpy arrays (iy, ix), or int32 tensors on ``device``."""
    import torch.nn.functional as F

    grid = torch.arange(g * g, dtype=torch.float64).view(1, 1, g, g)
    up = F.interpolate(grid, size=(R, R), mode="nearest")[0, 0].long()
    iy, ix = (up[:, 0] // g).numpy().astype(np.int32), (up[0, :] % g).numpy().astype(np.int32)
    if device is None:
        return iy, ix
    return torch.from_numpy(iy).to(device), torch.from_numpy(ix).to(device)


# ------------------------------------------------------------------------------------------------
# cluster_features / proto_clustering  (clustering.py:20-117)
# ------------------------------------------------------------------------------------------------

def _kmeans_maps(points: torch.Tensor, num_clusters: int, loop: str = "host") -> torch.Tensor:
    km = Kmeans(points.shape[1], num_clusters, niter=50, nredo=5, seed=1, loop=loop)
    km.train(points)
    return km.assign(points)[1]


def _kmeans_maps_grouped(points: torch.Tensor, ks) -> torch.Tensor:
    """``_kmeans_maps`` of every problem of points [B, N, d], problem b with ks[b] clusters -> labels int64 [B, N].  The problems of one
    k run as one ``KmeansBatch`` where the fused fit takes their (subsampled) shape, and one after the other on the loop otherwise;
    both return the same bits (the reservation on nearly equal objectives: ``KmeansBatch``).  Empty clusters - the normal case under
    ``use_mask``, where the background tokens are one point - are split on the device unless ``DEVICE_SPLIT`` is off."""
    B, N, d = points.shape
    out = torch.empty((B, N), dtype=torch.int64, device=points.device)
    for k in sorted(set(ks)):
        idx = [b for b in range(B) if ks[b] == k]
        if ops.kmeans_fit_shape_ok(min(N, 256 * k), d, k):
            group = points if len(idx) == B else points[torch.as_tensor(idx, device=points.device)]
            kb = KmeansBatch(d, k, niter=50, nredo=5, seed=1, split="device" if DEVICE_SPLIT else "host")
            kb.train(group)
            labels = kb.assign(group)[1]
            if len(idx) == B:
                return labels
            out[torch.as_tensor(idx, device=points.device)] = labels
        else:
            for b in idx:   # (on the host loop: the route the N13 / N18 tests count; the large dataset-wise fit is the device loop's)
                out[b] = _kmeans_maps(points[b], k)
    return out


def _annotation_counts(annotations: torch.Tensor, segments: int, device) -> list:
    """``torch.unique(segment).shape[0]`` of each of ``segments`` equal parts of the annotations (the reference: one ``torch.unique`` and so
    one host sync per frame, ``clustering.py:95-103``) from ONE presence launch and one read-back (``hip_ops.label_value_counts``; a part
    holding a value outside 0 .. 255 is counted by ``torch.unique`` there)."""
    a = annotations.to(device)
    if a.dtype not in (torch.uint8, torch.int64):
        a = a.long()
    return ops.label_value_counts(a.reshape(segments, -1).contiguous())


def cluster_features(features, num_clusters, feature_resolution, input_resolution, evaluation_protocol, annotations=None):
    """``clustering.cluster_features``: features [bs, fs, num_patches, dim] -> cluster maps [bs, fs, R, R] int16.  With ``annotations``
    ([bs, fs, ...] label maps) every k-means takes as many clusters as its frame / clip / dataset has label values."""
    bs, fs, num_patches, dim = features.shape
    feats = normalize_and_transform(features.reshape(bs * fs * num_patches, dim), 50)
    dim = feats.shape[1]
    feats = feats.view(bs * fs, num_patches, dim)
    R = input_resolution
    up = ops.upsample_bilinear_tokens(feats, R).view(bs, fs, R * R, dim)      # what the reference builds frame by frame
    if evaluation_protocol == "frame-wise":   # one k-means per frame
        ks = _annotation_counts(annotations, bs * fs, features.device) if annotations is not None else [num_clusters] * (bs * fs)
        out = _kmeans_maps_grouped(up.view(bs * fs, R * R, dim), ks).view(bs, fs, R, R)
    elif evaluation_protocol == "sample-wise":   # one per clip
        ks = _annotation_counts(annotations, bs, features.device) if annotations is not None else [num_clusters] * bs
        out = _kmeans_maps_grouped(up.view(bs, fs * R * R, dim), ks).view(bs, fs, R, R)
    elif evaluation_protocol == "dataset-wise":
        k = _annotation_counts(annotations, 1, features.device)[0] if annotations is not None else num_clusters
        out = _kmeans_maps(up.reshape(bs * fs * R * R, dim), k, "device" if DEVICE_LOOP else "host").view(bs, fs, R, R)
    else:
        raise ValueError(f"unknown evaluation protocol {evaluation_protocol!r}")
    return out.to(torch.int16)


@torch.no_grad()
def proto_scores(x, prototypes):
    """The cosine scores ``proto_clustering`` up-samples: x [samples, num_patch, dim], prototypes [k, dim] -> fp32 [samples, num_patch, k]."""
    sample_num, num_patches, dim = x.shape
    xn = ops.l2norm_fwd(x.reshape(sample_num * num_patches, dim).contiguous().float())
    pn = ops.l2norm_fwd(prototypes.detach().contiguous().float())
    return ops.linear_fwd(xn, pn).view(sample_num, num_patches, -1)


@torch.no_grad()
def proto_clustering(x, prototypes, input_size=14, output_size=224, num_classes=None):
    """``clustering.proto_clustering``: x [samples, num_patch, dim], prototypes [k, dim] -> assignments [samples, R, R]
    (upsampled cosine scores, arg-max; with ``num_classes`` the prototypes are first merged by k-means)."""
    sample_num, num_patches, dim = x.shape
    assign = ops.upsample_argmax_f32(proto_scores(x, prototypes), output_size)
    if num_classes is not None:
        km = Kmeans(prototypes.shape[1], num_classes, niter=50, nredo=5, seed=1)
        km.train(prototypes.detach().float())
        proto_maps = km.assign(prototypes.detach().float())[1]
        assign = proto_maps[assign.reshape(-1)].view(sample_num, output_size, output_size)
    return assign
