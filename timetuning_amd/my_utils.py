"""``sinkhorn`` and ``cosine_scheduler`` with the reference's signatures (``my_utils.py:246-283``), and ``imwrite_indexed``
(``my_utils.py:72-79``) with ``write_indexed_clip``, its batched form: label maps written as palette PNGs that are deflated on the device
(``hip_ops.encode_png_batch``)."""
from __future__ import annotations

import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import engine
from . import hip_ops as ops


@torch.no_grad()
def sinkhorn(Q: torch.Tensor, nmb_iters: int, world_size=1) -> torch.Tensor:
    """``my_utils.py:246-274``: Q is ``exp(scores / eps).T`` of shape [K, B_local]; returns the [B_local, K] assignment.
    The positive matrix goes to the kernel as it is (``tt_sinkhorn_from_q``).  For ``world_size > 1`` the local columns are
    all-gathered once and the global problem is solved on every rank (identical to the reference's 1 + 1 + nmb_iters
    all-reduces)."""
    Q = Q.detach().float().contiguous()
    dist = engine.exchange_group() if world_size > 1 else None
    if dist is None:
        return ops.sinkhorn_from_q(Q, int(nmb_iters))
    W, (K, B) = dist.get_world_size(), Q.shape
    cols = Q.t().contiguous()                                    # [B_local, K]: rank-major rows after the gather
    gathered = torch.empty((W * B, K), dtype=Q.dtype, device=Q.device)
    try:
        dist.all_gather_into_tensor(gathered, cols)
    except RuntimeError:  # backends without the flat all-gather
        dist.all_gather(list(gathered.chunk(W, dim=0)), cols)
    return ops.sinkhorn_from_q(gathered, int(nmb_iters), row0=dist.get_rank() * B, rows_out=B, transposed=True)


def cosine_scheduler(base_value: float, final_value: float, epochs: int, niter_per_ep: int):
    """``my_utils.py:278-283``."""
    iters = np.arange(epochs * niter_per_ep)
    schedule = final_value + 0.5 * (base_value - final_value) * (1 + np.cos(np.pi * iters / len(iters)))
    assert len(schedule) == epochs * niter_per_ep
    return schedule


def _on_gpu(array) -> torch.Tensor:
    if isinstance(array, torch.Tensor):
        return array if array.is_cuda else array.cuda()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(array))).cuda()


def _write_files(paths: Sequence[str], files: Sequence[bytes], threads: int = 8) -> None:
    def write(i):
        with open(paths[i], "wb") as f:
            f.write(files[i])
        return 0

    ops._each_file(write, len(paths), threads)


def imwrite_indexed(filename, array, color_palette):
    """Save indexed png for DAVIS (``my_utils.py:72-79``): ``array`` [H, W] integer labels - a GPU tensor, or a NumPy array, which is
    uploaded - written as a mode-P file with ``color_palette`` uint8 [n, 3].  Anything not 2-D raises, as the reference does.  The file
    holds the reference's pixels and palette; its bytes are the device encoder's, not Pillow's."""
    if (array.dim() if isinstance(array, torch.Tensor) else np.ndim(array)) != 2:
        raise Exception("Saving indexed PNGs requires 2D array.")
    _write_files([str(filename)], ops.encode_png_batch([_on_gpu(array)], palette=color_palette, threads=1), 1)


def write_indexed_clip(directory, maps, color_palette=None, names: Optional[Sequence[str]] = None) -> list:
    """The label maps ``maps`` [T, H, W] of one clip as ``directory/00000.png`` ... (or ``names``): ONE ``encode_png_batch`` call for the
    clip, the files written in the thread pool.  The palette defaults to ``visualization.voc_palette()``, which is the DAVIS palette.
    Returns the paths."""
    from . import visualization

    maps = _on_gpu(maps)
    if maps.dim() != 3:
        raise ValueError(f"write_indexed_clip: expected [T, H, W] label maps, got {tuple(maps.shape)}")
    T = maps.shape[0]
    names = [f"{t:05d}.png" for t in range(T)] if names is None else [str(n) for n in names]
    if len(names) != T:
        raise ValueError(f"write_indexed_clip: {len(names)} names for {T} maps")
    os.makedirs(directory, exist_ok=True)
    paths = [os.path.join(str(directory), n) for n in names]
    _write_files(paths, ops.encode_png_batch(maps, palette=visualization.voc_palette() if color_palette is None else color_palette))
    return paths
