"""Torch-tensor front end of the C ABI (include/timetuning_hip.h).

PyTorch supplies device memory and the HIP stream only; all arithmetic happens in
libtimetuning_hip.so.  Every function validates device / dtype / contiguity and raises if
the library is unavailable - there is no eager fallback.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

f32 = torch.float32


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, name: str, dtype=f32) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.HipLibraryError(f"{name}: expected a tensor in GPU memory (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")
    return t


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# ---- ABI 7: the K-split workspace of the persistent GEMMs is the CALLER's (tt_linear_ksplit_workspace_bytes / _init).  This front end keeps
# one per (device, stream) - launches on one stream are ordered, so they can share the partials and the self-resetting counters - allocated
# and initialised at its first use, OUTSIDE any launch path of the library (under a hipGraph capture of a step the buffer already exists:
# ``ksplit_workspace()`` is called once before capturing).
_KSPLIT_WS: dict = {}


def ksplit_workspace(device=None) -> torch.Tensor:
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), _stream())
    ws = _KSPLIT_WS.get(key)
    if ws is None:
        lib = _lib.load()
        with torch.cuda.device(key[0]):
            nb = int(lib.tt_linear_ksplit_workspace_bytes())
            ws = torch.empty(nb, dtype=torch.uint8, device=torch.device("cuda", key[0]))
            _lib.check(lib.tt_linear_ksplit_workspace_init(_p(ws), nb, _stream()), "tt_linear_ksplit_workspace_init")
        _KSPLIT_WS[key] = ws
    return ws


class PairRangeError(_lib.HipLibraryError):
    """An operand of the "f16x3" mode left fp16's range (|x| > 65504) or was not finite: the one way the mode differs from fp32."""


# The pair producers' range flag (include/timetuning_hip.h, "RANGE FLAG"): one device int per device, passed to every entry point that
# splits fp32 values into pairs.  ``check_pair_range`` reads it (a synchronisation: call it where the host synchronises anyway - the
# training driver does when it prints the loss, TimeT.train_update does every RANGE_CHECK_EVERY steps) and raises PairRangeError.
_RANGE_FLAG: dict = {}
RANGE_CHECK = True


def range_flag(device=None) -> Optional[torch.Tensor]:
    if not RANGE_CHECK:
        return None
    idx = torch.cuda.current_device() if device is None else (torch.device(device).index if torch.device(device).index is not None
                                                              else torch.cuda.current_device())
    f = _RANGE_FLAG.get(idx)
    if f is None:
        f = _RANGE_FLAG[idx] = torch.zeros(4, dtype=torch.int32, device=torch.device("cuda", idx))
    return f


def check_pair_range(device=None, reset: bool = True) -> None:
    """Raises PairRangeError if any pair producer since the last check saw a value beyond fp16's range.  Synchronises."""
    f = range_flag(device)
    if f is None:
        return
    bad = int(f[0].item())
    if bad:
        if reset:
            f.zero_()
        raise PairRangeError('an operand of the "f16x3" arithmetic is beyond fp16\'s range (|x| > 65504) or not finite; its products are '
                             "inf / NaN where fp32 arithmetic would not be.  Use --precision f32 (hip_ops.set_gemm_precision('f32')) "
                             "for this model / input.")


# name -> (mode of the C-side switch for tt_linear_fwd, bf16 planes used by the launch sequences for blocks that keep nothing)
# (2 "planes" = fp16 PAIRS: hi / lo halves of an fp32 value, the "f16x3" mode)
_PRECISIONS = {"f32": (0, 0), "bf16x3": (1, 0), "bf16": (2, 1), "bf16x6": (0, 3), "f16x3": (0, 2)}
_precision = "f32"


def set_gemm_precision(mode: str) -> None:
    """Arithmetic of the forward nn.Linear products: a setting of THIS front end (which launch sequences it strings together, and the
    ``precision`` argument it hands to the entry points that take one - ABI 8: the library itself keeps no such state).
    "f32"     (default) exact fp32 MFMA - every headline / parity number.
    "f16x3"   fp32-ACCURATE split mode (round 4): operands pre-split by their producers into fp16 PAIRS (hi = fp16(x), lo = fp16((x - hi)
              2^11): 23 significant bits), three fp16 MFMAs per product term into two fp32 accumulators (gemm_pairs8.hip).  Same blocks
              as "bf16x6" below; per-op error at or under the f32-MFMA kernels' own.
    "bf16x6"  fp32-ACCURATE split mode: operands pre-split by their producers into three bf16 planes (24 significant bits), six
              bf16 MFMAs per product term (gemm_planes.hip).  Applies to the blocks that keep no activations (frozen blocks,
              teacher, the non-target frames of the trainable blocks); everything with a backward stays exact fp32.
    "bf16"    BASELINE C4's MFMA bf16 path: the same blocks run on bf16 activations and weights in HBM (one plane, bf16
              attention); the blocks that keep activations convert fp32 operands while staging (gemm_nt_bf16.hip).
    "bf16x3"  two-plane split (~2^-16 per product) converted while staging; fp32 in HBM."""
    global _precision
    if mode not in _PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}")
    _lib.load()            # (a missing library fails here, loudly, as it always has)
    _precision = mode


def set_tuning_knob(name: str, value: int) -> None:
    """A dispatcher tuning knob (``TT_<NAME>``; the library reads them once from the environment): A/B tools and tests only."""
    _lib.check(_lib.load().tt_set_tuning_knob(name.encode(), int(value)), "tt_set_tuning_knob")


def tuning_knobs() -> dict:
    """``{name: (default, value)}`` of every tuning knob, in the order of the library's list (tt_tuning_knob_info; the index past its end
    is refused without touching the last-error string)."""
    lib, table = _lib.load(), {}
    name, default, value = C.c_char_p(), C.c_int(), C.c_int()
    while lib.tt_tuning_knob_info(len(table), C.byref(name), C.byref(default), C.byref(value)) == 0:
        table[name.value.decode()] = (default.value, value.value)
    return table


@contextlib.contextmanager
def tuning_knob(name: str, value: int):
    """Sets a tuning knob for the ``with`` block and restores the value it FOUND (not the default: nested blocks unwind correctly)."""
    found = tuning_knobs().get(name)
    set_tuning_knob(name, value)          # (an unknown name raises here)
    try:
        yield
    finally:
        set_tuning_knob(name, found[1])


def get_gemm_precision() -> str:
    return _precision


def precision_code() -> int:
    """The ``precision`` argument (TT_PRECISION_F32 / _BF16X3 / _BF16) of tt_linear_fwd, tt_label_propagate[_maps], tt_mlp_head_forward,
    tt_scores_sinkhorn and tt_vit_params.precision in the current mode."""
    return _PRECISIONS[_precision][0]


def plane_count() -> int:
    """bf16 planes the launch sequences use for blocks that keep no activations (0 = fp32 operands; 2 = fp16 PAIRS, see ``pairs()``)."""
    return _PRECISIONS[_precision][1]


def pairs() -> bool:
    """True in the "f16x3" mode: the blocks that keep nothing run on fp16-pair operands (``linear_fwd_pairs``)."""
    return _PRECISIONS[_precision][1] == 2


# The "f16x3" mode is a DISPATCH decision between two fp32-class arithmetics: below this many token rows per launch the pair kernels'
# extra passes (operand splits, the gradient's max pass) cost more than three-MFMA products save, so small launches keep the exact-f32
# kernels.  Measured on BASELINE C1 (4 frames: 788-row block launches, 394 / 392-row kept-frame and head launches), ms per step by
# threshold.  Round 4 (launch by launch): 1536 -> 3.10 (everything on f32), 700 -> 2.68, 512 -> 2.79, 393 -> 3.47, 300 -> 2.89, 200 -> 3.23:
# 640.  Round 5 (the step replayed as a HIP graph - launch counts no longer cost host time - and the general pair kernel on a ring of
# three / four K-tiles): 640 -> 2.07-2.11, 400 -> 2.08, 393 -> 2.18 (the kept frames' 394 rows on pairs, the head's 392 not: conversions),
# 300 -> 1.98-2.02, 200 -> 1.97-2.02, 0 -> 1.99-2.07: 256.  Tests set it to 0 to drive the pair kernels with tiny models.
PAIRS_MIN_ROWS = int(os.environ.get("TT_PAIRS_MIN_ROWS", "256"))   # (the environment variable: sweeps only)
GRAD_SCALE = os.environ.get("TT_NO_GRAD_SCALE") != "1"   # gradients are scaled by a power of two before their pair split (A/B aid: off)
AMAX_FROM_PRODUCERS = os.environ.get("TT_NO_AMAX_POOL") != "1"   # the gradient scale's maximum from the kernel that produced the dy (A/B aid: off = a max pass per dy)
TN_WGRAD = True   # weight gradients of the "f16x3" mode from row pairs (gemm_pairs_tn.hip); False: the transposed-operand route (A/B, tests)


def plane_count_for(rows: int) -> int:
    """``plane_count()`` for a launch sequence over ``rows`` token rows: the pair mode applies from PAIRS_MIN_ROWS rows on."""
    n = _PRECISIONS[_precision][1]
    return 0 if (n == 2 and rows < PAIRS_MIN_ROWS) else n


# Bumped by every op that rewrites parameters through raw pointers (AdamW, EMA, prototype renormalisation): tensors touched that way do not
# advance torch's version counter, so caches of derived operands (engine.weight_planes: the per-step pair split of a TRAINABLE weight)
# key on this as well.
PARAM_EPOCH = 0


def _bump_param_epoch() -> None:
    global PARAM_EPOCH
    PARAM_EPOCH += 1


# bench.py sets PROFILE to a list to get (layout, tile_choice, flops, start_event, end_event) per GEMM launch,
# recorded with HIP events on the stream the kernel is launched on.
PROFILE = None


def _prof_begin():
    if PROFILE is None:
        return None
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _prof_end(e0, name: str, M: int, N: int, K: int, batch: int = 1):
    """name "NT" = a forward Linear: booked as "NT" only when the lean whole-tile kernel really ran it (tt_linear_fwd_route),
    as "NTgen" when the general kernel did, as "NTbf16" in the on-the-fly bf16 modes."""
    if e0 is None:
        return
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record()
    lib = _lib.load()
    tile = lib.tt_gemm_tile_choice(M, N, batch)
    if name == "NT":
        if _PRECISIONS[_precision][0] != 0:
            name = "NTbf16"
        else:
            route = lib.tt_linear_fwd_route(M, N, K)
            tile, name = route & 3, ("NT" if route & 256 else "NTgen")
    PROFILE.append((name, tile, 2.0 * M * N * K * batch, e0, e1))


# ---- Linear ------------------------------------------------------------------------------------

def linear_fwd(x, w, bias=None, residual=None, act: int = 0, save_pre: bool = False, out=None):
    """y = act(x @ w.T + bias) (+ residual).  x [M,K], w [N,K].  Returns y or (y, pre_act)."""
    lib = _lib.load()
    _chk(x, "x"); _chk(w, "w")
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K
    y = out if out is not None else torch.empty((M, N), dtype=f32, device=x.device)
    pre = torch.empty((M, N), dtype=f32, device=x.device) if save_pre else None
    if bias is not None: _chk(bias, "bias")
    if residual is not None: _chk(residual, "residual")
    e0 = _prof_begin()
    _lib.check(lib.tt_linear_fwd(_p(x), _p(w), _p(bias), _p(residual), _p(y), _p(pre), M, N, K, act, precision_code(), _stream()), "tt_linear_fwd")
    _prof_end(e0, "NT", M, N, K)
    return (y, pre) if save_pre else y


def linear_bwd_data(dy, w, gelu_pre=None, out=None):
    """dx = dy @ w (* gelu'(gelu_pre))."""
    lib = _lib.load()
    _chk(dy, "dy"); _chk(w, "w")
    M, N = dy.shape
    K = w.shape[1]
    dx = out if out is not None else torch.empty((M, K), dtype=f32, device=dy.device)
    e0 = _prof_begin()
    _lib.check(lib.tt_linear_bwd_data(_p(dy), _p(w), _p(gelu_pre), _p(dx), M, N, K, _stream()), "tt_linear_bwd_data")
    _prof_end(e0, "NN", M, K, N)
    return dx


def linear_bwd_weight(dy, x, need_bias=True, dw_out=None, db_out=None):
    """dw = dy.T @ x, db = dy.sum(0)."""
    lib = _lib.load()
    _chk(dy, "dy"); _chk(x, "x")
    M, N = dy.shape
    K = x.shape[1]
    dw = dw_out if dw_out is not None else torch.empty((N, K), dtype=f32, device=dy.device)
    db = (db_out if db_out is not None else torch.empty((N,), dtype=f32, device=dy.device)) if need_bias else None
    nb = lib.tt_linear_bwd_weight_workspace_bytes(M, N, K)
    ws = _ws(nb, dy.device)
    if PROFILE is not None:  # time the GEMM alone: issue the bias column-sum as its own call
        e0 = _prof_begin()
        _lib.check(lib.tt_linear_bwd_weight(_p(dy), _p(x), _p(dw), None, M, N, K, _p(ws), nb, _stream()), "tt_linear_bwd_weight")
        _prof_end(e0, "TN", N, K, M)
        if db is not None:
            _lib.check(lib.tt_colsum(_p(dy), _p(db), M, N, _p(ws), nb, _stream()), "tt_colsum")
        return dw, db
    _lib.check(lib.tt_linear_bwd_weight(_p(dy), _p(x), _p(dw), _p(db), M, N, K, _p(ws), nb, _stream()), "tt_linear_bwd_weight")
    return dw, db


def linear_bwd(dy, w, x, gelu_pre=None, need_bias=True, dw_out=None, db_out=None):
    """Both backward products of an nn.Linear: dx = dy @ w (* gelu'(gelu_pre)), dw = dy.T @ x, db = dy.sum(0) - ONE launch for the
    two GEMMs where the lean kernels apply (tt_linear_bwd), bit-identical to linear_bwd_data + linear_bwd_weight.  ``dw_out`` / ``db_out``:
    caller-owned destinations (the data-parallel exchange's flat gradient buckets)."""
    lib = _lib.load()
    _chk(dy, "dy"); _chk(w, "w"); _chk(x, "x")
    M, N = dy.shape
    K = w.shape[1]
    assert w.shape[0] == N and tuple(x.shape) == (M, K), (dy.shape, w.shape, x.shape)
    if gelu_pre is not None: _chk(gelu_pre, "gelu_pre")
    dx = torch.empty((M, K), dtype=f32, device=dy.device)
    dw = _chk(dw_out, "dw_out") if dw_out is not None else torch.empty((N, K), dtype=f32, device=dy.device)
    db = (_chk(db_out, "db_out") if db_out is not None else torch.empty((N,), dtype=f32, device=dy.device)) if need_bias else None
    nb = lib.tt_linear_bwd_weight_workspace_bytes(M, N, K)
    ws = _ws(nb, dy.device)
    e0 = _prof_begin()   # booked as ONE entry: both products (4 M N K flops) and the split-K fold they end in
    _lib.check(lib.tt_linear_bwd(_p(dy), _p(w), _p(x), _p(gelu_pre), _p(dx), _p(dw), _p(db), M, N, K, _p(ws), nb, _stream()), "tt_linear_bwd")
    if e0 is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        PROFILE.append(("BWD", 3, 4.0 * M * N * K, e0, e1))
    return dx, dw, db


def colsum(a):
    lib = _lib.load()
    _chk(a, "a")
    M, N = a.shape
    out = torch.empty((N,), dtype=f32, device=a.device)
    nb = lib.tt_colsum_workspace_bytes(M, N)
    ws = _ws(nb, a.device)
    _lib.check(lib.tt_colsum(_p(a), _p(out), M, N, _p(ws), nb, _stream()), "tt_colsum")
    return out


def gemm(A, B, a_mmajor=False, b_nmajor=False, alpha=1.0, out=None):
    """C = alpha * op(A) @ op(B) (see tt_gemm_f32).  2-D operands, or 3-D for a batch."""
    lib = _lib.load()
    _chk(A, "A"); _chk(B, "B")
    batch = 1
    sA = sB = sC = 0
    if A.dim() == 3:
        batch = A.shape[0]
        A2, B2 = A[0], B[0]
        sA, sB = A.stride(0), B.stride(0)
    else:
        A2, B2 = A, B
    if a_mmajor:
        K, M = A2.shape
    else:
        M, K = A2.shape
    if b_nmajor:
        Kb, N = B2.shape
    else:
        N, Kb = B2.shape
    assert K == Kb, (A.shape, B.shape)
    shape = (batch, M, N) if A.dim() == 3 else (M, N)
    Cm = out if out is not None else torch.empty(shape, dtype=f32, device=A.device)
    sC = M * N if batch > 1 else 0
    _lib.check(lib.tt_gemm_f32(_p(A), _p(B), _p(Cm), M, N, K, A2.stride(0), B2.stride(0), N, int(a_mmajor), int(b_nmajor),
                               float(alpha), batch, sA, sB, sC, _stream()), "tt_gemm_f32")
    return Cm


# ---- ViT pieces ----------------------------------------------------------------------------------

def patch_embed_fwd(img, w, bias, cls, pos, patch: int, frame_map=None):
    """img [F_src,C,H,W] -> tokens [F, n+1, D] (conv k=s=patch, cls token, pos-embed)."""
    lib = _lib.load()
    _chk(img, "img"); _chk(w, "w"); _chk(bias, "bias"); _chk(cls, "cls"); _chk(pos, "pos")
    Fs, Cc, H, W = img.shape
    D = w.shape[0]
    F = Fs if frame_map is None else frame_map.numel()
    if frame_map is not None: _chk(frame_map, "frame_map", torch.int32)
    n = (H // patch) * (W // patch)
    if pos.numel() != (n + 1) * D:
        raise ValueError("pos_embed does not match the token grid: pass VisionTransformer.pos_table(H, W)")
    tokens = torch.empty((F, n + 1, D), dtype=f32, device=img.device)
    e0 = _prof_begin()
    _lib.check(lib.tt_patch_embed_fwd(_p(img), _p(frame_map), _p(w), _p(bias), _p(cls), _p(pos), _p(tokens), F, Cc, H, W, patch, D,
                                      _stream()), "tt_patch_embed_fwd")
    _prof_end(e0, "patch", F * n, D, Cc * patch * patch)
    return tokens


def patch_embed_planes_ok(patch: int, W: int, K: int, D: int) -> bool:
    """Shapes ``patch_embed_fwd_planes`` takes (tt_patch_embed_fwd_planes)."""
    return patch % 4 == 0 and W % 4 == 0 and K % 64 == 0 and D % 64 == 0


def patch_embed_pairs_ok(patch: int, W: int, K: int, D: int) -> bool:
    """Shapes ``patch_embed_fwd_pairs`` takes (tt_patch_embed_fwd_pairs)."""
    return patch % 4 == 0 and W % 4 == 0 and K % 32 == 0 and D % 64 == 0


def patch_embed_fwd_pairs(img, w_pairs, bias, cls, pos, patch: int, frame_map=None):
    """``patch_embed_fwd`` on fp16-pair operands (the "f16x3" mode): w_pairs [D, 2 C P P] = ``split_pairs`` of the conv weight viewed
    [D, C P P]; the patches are split into pairs on their way into an im2col buffer, ONE pair GEMM over all token rows."""
    lib = _lib.load()
    _chk(img, "img"); _chk(w_pairs, "w_pairs", f16); _chk(bias, "bias"); _chk(cls, "cls"); _chk(pos, "pos")
    Fs, Cc, H, W = img.shape
    D = w_pairs.shape[0]
    F = Fs if frame_map is None else frame_map.numel()
    if frame_map is not None: _chk(frame_map, "frame_map", torch.int32)
    n = (H // patch) * (W // patch)
    K = Cc * patch * patch
    assert w_pairs.shape == (D, 2 * K), (w_pairs.shape, D, K)
    if pos.numel() != (n + 1) * D:
        raise ValueError("pos_embed does not match the token grid: pass VisionTransformer.pos_table(H, W)")
    tokens = torch.empty((F, n + 1, D), dtype=f32, device=img.device)
    nb = lib.tt_patch_embed_pairs_workspace_bytes(F, Cc, H, W, patch)
    ws = _ws(nb, img.device)
    M = F * (n + 1)
    p8 = PROFILE is not None and lib.tt_linear_fwd_pairs_route(M, D, K, 0, 1, 1, 1, 0, 0) == 8
    e0 = _prof_begin()
    _lib.check(lib.tt_patch_embed_fwd_pairs(_p(img), _p(frame_map), _p(w_pairs), _p(bias), _p(cls), _p(pos), _p(tokens), F, Cc, H, W, patch, D,
                                            _p(ws), nb, _p(range_flag(img.device)), _stream()), "tt_patch_embed_fwd_pairs")
    _prof_end(e0, "PAIRS8" if p8 else "PAIRS", M, D, K)
    return tokens


def patch_embed_fwd_planes(img, w_planes, bias, cls, pos, patch: int, frame_map=None):
    """``patch_embed_fwd`` on bf16 operands (the "bf16" precision mode, BASELINE C4's path): w_planes [1, D, C*P*P] bf16 =
    ``split_planes(w, 1)``; the patches are rounded to bf16 on their way into an im2col buffer, fp32 accumulation, fp32 tokens."""
    lib = _lib.load()
    _chk(img, "img"); _chk(w_planes, "w_planes", bf16); _chk(bias, "bias"); _chk(cls, "cls"); _chk(pos, "pos")
    Fs, Cc, H, W = img.shape
    D = w_planes.shape[1]
    F = Fs if frame_map is None else frame_map.numel()
    if frame_map is not None: _chk(frame_map, "frame_map", torch.int32)
    n = (H // patch) * (W // patch)
    K = Cc * patch * patch
    if pos.numel() != (n + 1) * D:
        raise ValueError("pos_embed does not match the token grid: pass VisionTransformer.pos_table(H, W)")
    tokens = torch.empty((F, n + 1, D), dtype=f32, device=img.device)
    nb = lib.tt_patch_embed_planes_workspace_bytes(F, Cc, H, W, patch)
    ws = _ws(nb, img.device)
    M = F * (n + 1)
    p8 = bool(lib.tt_linear_fwd_planes_route(1, M, D, K, 0, 1, 1, 1, 0, 0))
    e0 = _prof_begin()
    _lib.check(lib.tt_patch_embed_fwd_planes(_p(img), _p(frame_map), _p(w_planes), _p(bias), _p(cls), _p(pos), _p(tokens), F, Cc, H, W, patch, D,
                                             _p(ws), nb, _stream()), "tt_patch_embed_fwd_planes")
    _prof_end(e0, "PLANES8_1" if p8 else "PLANES1", M, D, K)
    return tokens


def pos_embed_interpolate(pos, grid_h: int, grid_w: int):
    """interpolate_pos_encoding's bicubic branch (dino_vision_transformer.py:219-234): pos [1+g*g, D] -> [1+grid_h*grid_w, D]."""
    lib = _lib.load()
    _chk(pos, "pos")
    D = pos.shape[-1]
    g = int(round((pos.shape[0] - 1) ** 0.5))
    out = torch.empty((1 + grid_h * grid_w, D), dtype=f32, device=pos.device)
    # the reference adds 0.1 to the target grid before dividing ("to avoid floating point error in the interpolation")
    _lib.check(lib.tt_pos_embed_interpolate(_p(pos), _p(out), g, grid_h, grid_w, D, (grid_h + 0.1) / g, (grid_w + 0.1) / g, _stream()),
               "tt_pos_embed_interpolate")
    return out


def pos_embed_interpolate_bwd(dtable, g: int, grid_h: int, grid_w: int, out=None):
    """The adjoint of ``pos_embed_interpolate``: dtable [1+grid_h*grid_w, D] (the gradient of the resampled table) -> the gradient of the
    stored table [1+g*g, D] (``out``: a caller-owned destination)."""
    lib = _lib.load()
    _chk(dtable, "dtable")
    D = dtable.shape[-1]
    if dtable.numel() != (1 + grid_h * grid_w) * D:
        raise ValueError(f"dtable {tuple(dtable.shape)} is not a [1 + {grid_h} * {grid_w}, D] table")
    dpos = _chk(out, "out") if out is not None else torch.empty((1 + g * g, D), dtype=f32, device=dtable.device)
    if dpos.numel() != (1 + g * g) * D:
        raise ValueError(f"out {tuple(dpos.shape)} is not a [1 + {g} * {g}, {D}] table")
    _lib.check(lib.tt_pos_embed_interpolate_bwd(_p(dtable), _p(dpos), g, grid_h, grid_w, D, (grid_h + 0.1) / g, (grid_w + 0.1) / g, _stream()),
               "tt_pos_embed_interpolate_bwd")
    return dpos


def patch_embed_bwd_ok(F: int, C_: int, H: int, W: int, patch: int, D: int) -> bool:
    """Shapes ``patch_embed_bwd`` takes (tt_patch_embed_bwd_shape_ok)."""
    return bool(_lib.load().tt_patch_embed_bwd_shape_ok(F, C_, H, W, patch, D))


def patch_embed_bwd(dtok, img, patch: int, frame_map=None, need=("dw", "dbias", "dcls", "dtable"), dw_out=None, dbias_out=None,
                    dcls_out=None, dtable_out=None, workspace=None):
    """The adjoint of ``patch_embed_fwd`` (tt_patch_embed_bwd): dtok [F, n+1, D] = the gradient of the tokens, img [F_src, C, H, W] and
    ``frame_map`` as in the forward.  Returns a dict with the entries named in ``need``: ``dw`` [D, C*P*P], ``dbias`` [D], ``dcls`` [D],
    ``dtable`` [n+1, D] (the gradient of the position table the forward added).  ``*_out``: caller-owned destinations (the gradient
    exchange's flat buckets), implied needed.  ``workspace``: a uint8 buffer of at least ``tt_patch_embed_bwd_workspace_bytes`` (default: one
    is allocated)."""
    lib = _lib.load()
    _chk(dtok, "dtok"); _chk(img, "img")
    Fs, Cc, H, W = img.shape
    if dtok.dim() != 3:
        raise ValueError(f"dtok must be [F, n + 1, D], got {tuple(dtok.shape)}")
    F, N, D = dtok.shape
    if frame_map is not None:
        _chk(frame_map, "frame_map", torch.int32)
        if frame_map.numel() != F:
            raise ValueError(f"frame_map has {frame_map.numel()} entries for {F} frames of dtok")
    elif Fs != F:
        raise ValueError(f"dtok has {F} frames, img {Fs} (and no frame_map)")
    if patch > 0 and H % patch == 0 and W % patch == 0 and N != (H // patch) * (W // patch) + 1:
        raise ValueError(f"dtok has {N} token rows per frame; a {H} x {W} input at patch size {patch} has {(H // patch) * (W // patch) + 1}")
    K = Cc * patch * patch
    outs = dict(dw=dw_out, dbias=dbias_out, dcls=dcls_out, dtable=dtable_out)
    shapes = dict(dw=(D, K), dbias=(D,), dcls=(D,), dtable=(N, D))
    unknown = set(need) - set(shapes)
    if unknown:
        raise ValueError(f"need: unknown outputs {sorted(unknown)}")
    for name, shape in shapes.items():
        if outs[name] is not None:
            _chk(outs[name], name + "_out")
            if outs[name].numel() != int(np.prod(shape)):
                raise ValueError(f"{name}_out has {outs[name].numel()} elements, expected {shape}")
        elif name in need:
            outs[name] = torch.empty(shape, dtype=f32, device=dtok.device)
    nb = lib.tt_patch_embed_bwd_workspace_bytes(F, Cc, H, W, patch, D)
    ws = workspace if workspace is not None else _ws(nb, dtok.device)
    _lib.check(lib.tt_patch_embed_bwd(_p(dtok), _p(img), _p(frame_map), _p(outs["dw"]), _p(outs["dbias"]), _p(outs["dcls"]), _p(outs["dtable"]),
                                      F, Cc, H, W, patch, D, _p(ws), ws.numel() * ws.element_size(), _stream()), "tt_patch_embed_bwd")
    return {k: v for k, v in outs.items() if v is not None}


def _layernorm_fwd_into(entry, alloc, x, gamma, beta, eps, save_stats, drop_first_token, *tail):
    """The bookkeeping the three ``layernorm_fwd*`` wrappers share: rows and the ``skip_group`` of ``drop_first_token``, the statistics, the call.
    ``alloc(rows, D)`` returns the output and the arguments that stand between ``beta`` and ``mean`` in the entry's signature (y first);
    ``tail``: what stands between ``skip_group`` and the stream."""
    lib = _lib.load()
    _chk(x, "x"); _chk(gamma, "gamma"); _chk(beta, "beta")
    D = x.shape[-1]
    rows = x.numel() // D
    skip = 0
    if drop_first_token:
        skip = x.shape[-2]
        rows = rows // skip * (skip - 1)
    y, *y_args = alloc(rows, D)
    mean = torch.empty((rows,), dtype=f32, device=x.device) if save_stats else None
    rstd = torch.empty((rows,), dtype=f32, device=x.device) if save_stats else None
    _lib.check(getattr(lib, entry)(_p(x), _p(gamma), _p(beta), _p(y), *y_args, _p(mean), _p(rstd), rows, D, float(eps), skip, *tail, _stream()), entry)
    return (y, mean, rstd) if save_stats else y


def layernorm_fwd(x, gamma, beta, eps=1e-6, save_stats=False, out=None, drop_first_token=False):
    """LayerNorm over the last dim.  drop_first_token: x is [F,N,D] and the result is [F*(N-1), D] (cls row removed)."""
    def alloc(rows, D):
        if out is not None:
            return (out,)
        return (torch.empty((rows, D), dtype=f32, device=x.device) if drop_first_token else torch.empty_like(x),)
    return _layernorm_fwd_into("tt_layernorm_fwd", alloc, x, gamma, beta, eps, save_stats, drop_first_token)


def layernorm_bwd(dy, x, gamma, mean, rstd, need_wgrad=True, dx_accum=None, drop_first_token=False, dg_out=None, db_out=None, amax_out=None):
    """Returns (dx, dgamma, dbeta).  dx_accum: tensor to accumulate dx into (residual branch).
    drop_first_token: dy is [F*(N-1), D] against x [F,N,D]; dx is [F,N,D] with zero cls rows.
    ``amax_out``: a zeroed 1-float device tensor (``AmaxPool.take``) the kernel raises to max |dx| - dx is the next Linear's dy, whose pair
    split then needs no max pass (``linear_bwd_pairs(dy_amax=)``)."""
    lib = _lib.load()
    _chk(dy, "dy"); _chk(x, "x")
    D = x.shape[-1]
    rows = dy.numel() // D
    skip = x.shape[-2] if drop_first_token else 0
    if dx_accum is not None:
        dx = dx_accum
    elif drop_first_token:
        dx = torch.zeros_like(x)
    else:
        dx = torch.empty_like(x)
    dg = (_chk(dg_out, "dg_out") if dg_out is not None else torch.empty((D,), dtype=f32, device=x.device)) if need_wgrad else None
    db = (_chk(db_out, "db_out") if db_out is not None else torch.empty((D,), dtype=f32, device=x.device)) if need_wgrad else None
    nb = lib.tt_layernorm_bwd_workspace_bytes(rows, D)
    ws = _ws(nb, x.device)
    _lib.check(lib.tt_layernorm_bwd(_p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dg), _p(db), rows, D,
                                    1 if dx_accum is not None else 0, skip, _p(ws), nb, _p(amax_out), _stream()), "tt_layernorm_bwd")
    return dx, dg, db


def attention_fwd(qkv, num_heads: int, save_lse=False, return_probs=False):
    """qkv [F,N,3*D] -> out [F,N,D] (+ lse [F,H,N], probs [F,H,N,N])."""
    lib = _lib.load()
    _chk(qkv, "qkv")
    F, N, D3 = qkv.shape
    D = D3 // 3
    hd = D // num_heads
    out = torch.empty((F, N, D), dtype=f32, device=qkv.device)
    lse = torch.empty((F, num_heads, N), dtype=f32, device=qkv.device) if save_lse else None
    probs = torch.empty((F, num_heads, N, N), dtype=f32, device=qkv.device) if return_probs else None
    _lib.check(lib.tt_attention_fwd(_p(qkv), _p(out), _p(lse), _p(probs), F, N, num_heads, hd, float(hd ** -0.5), _stream()),
               "tt_attention_fwd")
    return out, lse, probs


# the "f16x3" mode's attention backward with its row-wise products on fp16 pairs (tt_attention_bwd_pairs); "0": the fp32-MFMA kernels (A/B)
ATTN_BWD_PAIRS = os.environ.get("TT_ATTN_BWD_PAIRS", "1") != "0"


def attention_bwd(qkv, out, dout, lse, num_heads: int, bf16_products: bool = False, amax_out=None, pair_products: bool = False, dout_amax=None):
    """dqkv of the fused attention core from the forward's out / lse.  ``bf16_products``: the matrix products on bf16 MFMA
    (tt_attention_bwd_bf16 - the "bf16" precision mode's backward; statistics, P and dS stay fp32); ``pair_products``: S and dP on fp16
    pairs (tt_attention_bwd_pairs - the "f16x3" mode's: fp32-class; the range flag is the pair entry points'; ``dout_amax``: the amax
    slot the kernel that wrote dout raised - without one the call measures max |dout| itself)."""
    lib = _lib.load()
    _chk(qkv, "qkv"); _chk(out, "out"); _chk(dout, "dout"); _chk(lse, "lse")
    F, N, D3 = qkv.shape
    hd = D3 // 3 // num_heads
    dqkv = torch.empty_like(qkv)
    if pair_products and not bf16_products:
        nb = lib.tt_attention_bwd_pairs_workspace_bytes(F, N, num_heads, hd)
        ws = _ws(nb, qkv.device)
        _lib.check(lib.tt_attention_bwd_pairs(_p(qkv), _p(out), _p(dout), _p(lse), _p(dqkv), F, N, num_heads, hd, float(hd ** -0.5), _p(dout_amax), _p(ws), nb,
                                              _p(range_flag(qkv.device)), _p(amax_out), _stream()), "tt_attention_bwd_pairs")
        return dqkv
    nb = lib.tt_attention_bwd_workspace_bytes(F, N, num_heads, hd)
    ws = _ws(nb, qkv.device)
    if bf16_products:
        _lib.check(lib.tt_attention_bwd_bf16(_p(qkv), _p(out), _p(dout), _p(lse), _p(dqkv), F, N, num_heads, hd, float(hd ** -0.5), _p(ws), nb, _stream()),
                   "tt_attention_bwd_bf16")
    else:   # (amax_out: max |dqkv| for the pair split of the qkv Linear's dy, as layernorm_bwd)
        _lib.check(lib.tt_attention_bwd(_p(qkv), _p(out), _p(dout), _p(lse), _p(dqkv), F, N, num_heads, hd, float(hd ** -0.5), _p(ws), nb, _p(amax_out),
                                        _stream()), "tt_attention_bwd")
    return dqkv


# ---- prototypes / assignment ---------------------------------------------------------------------

def l2norm_fwd(x, save_inv=False, out=None):
    """F.normalize(x, dim=-1).  x may be a row-strided 2-D view (stride(1) == 1)."""
    lib = _lib.load()
    if x.dim() != 2 or x.stride(1) != 1 or not x.is_cuda or x.dtype != f32:
        raise ValueError("l2norm_fwd: expected a 2-D fp32 GPU tensor with unit inner stride")
    rows, D = x.shape
    xn = out if out is not None else torch.empty((rows, D), dtype=f32, device=x.device)
    inv = torch.empty((rows,), dtype=f32, device=x.device) if save_inv else None
    _lib.check(lib.tt_l2norm_fwd(_p(x), x.stride(0), _p(xn), _p(inv), rows, D, _stream()), "tt_l2norm_fwd")
    return (xn, inv) if save_inv else xn


def l2norm_bwd(dxn, xn, inv, amax_out=None):
    lib = _lib.load()
    _chk(dxn, "dxn"); _chk(xn, "xn"); _chk(inv, "inv")
    rows, D = xn.shape
    dx = torch.empty_like(xn)
    _lib.check(lib.tt_l2norm_bwd(_p(dxn), _p(xn), _p(inv), _p(dx), rows, D, _p(amax_out), _stream()), "tt_l2norm_bwd")
    return dx


class AmaxPool:
    """Zeroed 1-float device slots for the maxima the gradient PRODUCERS publish (``amax_out`` of layernorm_bwd / attention_bwd /
    l2norm_bwd / the gelu' data gradient) and the pair split of that gradient consumes (``linear_bwd_pairs(dy_amax=)``): one ``reset()`` (a
    64-float fill) at the top of a backward instead of a max pass over every dy (12 per C2 step, 0.11 ms)."""
    _pools: dict = {}

    def __init__(self, device):
        self.SLOT = _lib.load().tt_amax_slot_bytes() // 4   # floats per slot: 16 ways, 64 floats apart (the producers spread their atomics)
        self.buf = torch.zeros(24 * self.SLOT, dtype=f32, device=device)
        self.n = 0

    @classmethod
    def get(cls, device) -> "AmaxPool":
        dev = torch.device(device)
        key = (dev.index if dev.index is not None else torch.cuda.current_device(), _stream())
        p = cls._pools.get(key)
        if p is None:
            p = cls._pools[key] = cls(dev)
        return p

    def reset(self) -> None:
        self.buf.zero_()
        self.n = 0

    def take(self):
        if (self.n + 1) * self.SLOT > self.buf.numel():
            return None            # (more gradients than slots: those splits make their own max pass)
        self.n += 1
        return self.buf[(self.n - 1) * self.SLOT:self.n * self.SLOT]


def normalize_rows_(w):
    _bump_param_epoch()
    lib = _lib.load()
    _chk(w, "w")
    _lib.check(lib.tt_normalize_rows_inplace(_p(w), w.shape[0], w.shape[1], _stream()), "tt_normalize_rows_inplace")
    return w


def _sinkhorn_solve(what: str, src, B: int, K: int, row0: int, rows_out: Optional[int], launch):
    """Allocates q [rows_out, K] and the workspace of a [B, K] solve, runs ``launch(lib, q, rows_out, ws, nb)`` and checks its return code."""
    lib = _lib.load()
    rows_out = B - row0 if rows_out is None else rows_out
    q = torch.empty((rows_out, K), dtype=f32, device=src.device)
    nb = lib.tt_sinkhorn_workspace_bytes(B, K)
    _lib.check(launch(lib, q, rows_out, _ws(nb, src.device), nb), what)
    return q


def sinkhorn(scores, iters: int, eps: float = 0.05, row0: int = 0, rows_out: Optional[int] = None):
    """scores [B_total, K] -> q [rows_out, K] for rows [row0, row0+rows_out)."""
    _chk(scores, "scores")
    B, K = scores.shape
    return _sinkhorn_solve("tt_sinkhorn", scores, B, K, row0, rows_out, lambda lib, q, rows, ws, nb: lib.tt_sinkhorn(
        _p(scores), _p(q), B, K, row0, rows, float(eps), int(iters), _p(ws), nb, _stream()))


class SinkhornLocal:
    """One rank's share of a DISTRIBUTED solve in the reference's own form (my_utils.py:250-272): the columns stay on their rank, the K
    row sums are all-reduced once per iteration by the caller - ``u = begin(scores)``; ``iters - 1`` times ``u = step(all_reduce(u))``;
    ``q = end(all_reduce(u))`` (``end(None)`` for zero iterations).  ``lib``: the HIP library (default) or the CPU twin (tests)."""

    def __init__(self, B_loc: int, B_total: int, K: int, device, lib=None):
        self.lib = _lib.load() if lib is None else lib
        self.pre = "tt_" if lib is None else "tt_cpu_"
        self.B_loc, self.B_total, self.K = int(B_loc), int(B_total), int(K)
        self.nb = getattr(self.lib, self.pre + "sinkhorn_local_workspace_bytes")(self.B_loc, self.K)
        self.ws = torch.empty((self.nb + 3) // 4, dtype=f32, device=device)   # owned: it holds E between the calls
        self.device = device

    def _stream(self):
        return _stream() if torch.device(self.device).type == "cuda" else None

    def _ck(self, rc: int, what: str) -> None:
        if rc != 0:
            if self.pre == "tt_":
                _lib.check(rc, "tt_" + what)
            raise RuntimeError(f"{self.pre}{what} failed (code {rc})")

    def begin(self, scores, eps: float):
        assert scores.shape == (self.B_loc, self.K) and scores.dtype == f32 and scores.is_contiguous()
        u = torch.empty((self.K,), dtype=f32, device=scores.device)
        self._ck(getattr(self.lib, self.pre + "sinkhorn_local_begin")(_p(scores), _p(u), self.B_loc, self.K, float(eps), _p(self.ws), self.nb, self._stream()),
                 "sinkhorn_local_begin")
        return u

    def step(self, u_global):
        u = torch.empty_like(u_global)
        self._ck(getattr(self.lib, self.pre + "sinkhorn_local_step")(_p(u_global), _p(u), self.B_loc, self.B_total, self.K, _p(self.ws), self.nb, self._stream()),
                 "sinkhorn_local_step")
        return u

    def end(self, u_global, rows_out: Optional[int] = None):
        rows_out = self.B_loc if rows_out is None else int(rows_out)
        q = torch.empty((rows_out, self.K), dtype=f32, device=self.ws.device)
        self._ck(getattr(self.lib, self.pre + "sinkhorn_local_end")(_p(u_global), _p(q), self.B_loc, rows_out, self.K, _p(self.ws), self.nb, self._stream()),
                 "sinkhorn_local_end")
        return q


def sinkhorn_from_q(Q, iters: int, row0: int = 0, rows_out: Optional[int] = None, transposed: bool = False):
    """Q positive = exp(scores / eps): [K, B_total] as my_utils.sinkhorn receives it, or [B_total, K] with ``transposed``
    -> q [rows_out, K]."""
    _chk(Q, "Q")
    B, K = Q.shape if transposed else Q.shape[::-1]
    return _sinkhorn_solve("tt_sinkhorn_from_q", Q, B, K, row0, rows_out, lambda lib, q, rows, ws, nb: lib.tt_sinkhorn_from_q(
        _p(Q), int(transposed), _p(q), B, K, row0, rows, int(iters), _p(ws), nb, _stream()))


def label_propagate_sims(xn, K: int, n_last_frames=7):
    """The first half of ``label_propagate`` - the cosine similarities of all target frames, which do not depend on the assignment - for a
    caller that computes them beside other work (``label_propagate(..., sims=)`` takes the result).  None when they do not fit one chunk."""
    lib = _lib.load()
    _chk(xn, "xn")
    fs, bs, n, D = xn.shape
    g = int(round(n ** 0.5))
    assert g * g == n
    nb = lib.tt_label_propagate_workspace_bytes(bs, fs, g, D, K, n_last_frames)
    ws = _ws(nb, xn.device)
    rc = lib.tt_label_propagate_sims(_p(xn), bs, fs, g, D, K, n_last_frames, precision_code(), _p(ws), nb, _stream())
    if rc == 1:
        return None
    _lib.check(rc, "tt_label_propagate_sims")
    return ws


def label_propagate(xn, seg0, n_last_frames=7, radius=6, topk=5, temperature=0.1, return_pmap=False, sims=None):
    """xn [fs,bs,n,D] normalised tokens (time-major), seg0 [bs,n,K] -> labels [bs,n] int64 (+ pmap [bs,n,K] fp64).  ``sims``: the workspace
    ``label_propagate_sims`` prepared for the same xn / K / n_last_frames."""
    lib = _lib.load()
    _chk(xn, "xn"); _chk(seg0, "seg0")
    fs, bs, n, D = xn.shape
    K = seg0.shape[-1]
    g = int(round(n ** 0.5))
    assert g * g == n
    labels = torch.empty((bs, n), dtype=torch.int64, device=xn.device)
    pmap = torch.empty((bs, n, K), dtype=torch.float64, device=xn.device) if return_pmap else None
    nb = lib.tt_label_propagate_workspace_bytes(bs, fs, g, D, K, n_last_frames)
    if sims is not None:
        assert sims.numel() >= nb, (sims.numel(), nb)
        _lib.check(lib.tt_label_propagate_from_sims(_p(xn), _p(seg0), _p(labels), _p(pmap), bs, fs, g, D, K, n_last_frames, radius, topk,
                                                    float(temperature), _p(sims), sims.numel(), _stream()), "tt_label_propagate_from_sims")
        return (labels, pmap) if return_pmap else labels
    ws = _ws(nb, xn.device)
    _lib.check(lib.tt_label_propagate(_p(xn), _p(seg0), _p(labels), _p(pmap), bs, fs, g, D, K, n_last_frames, radius, topk,
                                      float(temperature), precision_code(), _p(ws), nb, _stream()), "tt_label_propagate")
    return (labels, pmap) if return_pmap else labels


def label_propagate_maps(xn, seg0, n_last_frames=7, radius=6, topk=5, temperature=0.1):
    """As ``label_propagate`` but returns ALL propagated maps [fs-1, bs, n, K] fp64 (mask_propagation.py:448-496)."""
    lib = _lib.load()
    _chk(xn, "xn"); _chk(seg0, "seg0")
    fs, bs, n, D = xn.shape
    K = seg0.shape[-1]
    g = int(round(n ** 0.5))
    assert g * g == n
    maps = torch.empty((fs - 1, bs, n, K), dtype=torch.float64, device=xn.device)
    nb = lib.tt_label_propagate_workspace_bytes(bs, fs, g, D, K, n_last_frames)
    ws = _ws(nb, xn.device)
    _lib.check(lib.tt_label_propagate_maps(_p(xn), _p(seg0), _p(maps), bs, fs, g, D, K, n_last_frames, radius, topk, float(temperature),
                                           precision_code(), _p(ws), nb, _stream()), "tt_label_propagate_maps")
    return maps


def _grid(grid, n: int, who: str):
    gh, gw = (int(v) for v in grid)
    if gh <= 0 or gw <= 0 or gh * gw != n:
        raise ValueError(f"{who}: grid {gh}x{gw} does not hold the {n} tokens")
    return gh, gw


def label_propagate_grid_maps(xn, seg0, grid, n_last_frames=7, radius=6, topk=5, temperature=0.1):
    """``label_propagate_maps`` on a gh x gw token grid: xn [fs,bs,n,D] normalised tokens (time-major, n = gh*gw row-major), seg0 [bs,n,K]
    -> all propagated maps [fs-1, bs, n, K] fp64.  ``radius`` 0 is the unrestricted variant (no mask); no cap on candidates per query."""
    lib = _lib.load()
    _chk(xn, "xn"); _chk(seg0, "seg0")
    fs, bs, n, D = xn.shape
    K = seg0.shape[-1]
    gh, gw = _grid(grid, n, "label_propagate_grid_maps")
    if tuple(seg0.shape) != (bs, n, K):
        raise ValueError(f"label_propagate_grid_maps: seg0 {tuple(seg0.shape)} does not match xn {tuple(xn.shape)}")
    maps = torch.empty((max(fs - 1, 0), bs, n, K), dtype=torch.float64, device=xn.device)
    nb = lib.tt_label_propagate_grid_workspace_bytes(bs, fs, gh, gw, D, K, n_last_frames, radius)
    ws = _ws(nb, xn.device)
    _lib.check(lib.tt_label_propagate_grid_maps(_p(xn), _p(seg0), _p(maps), bs, fs, gh, gw, D, K, n_last_frames, radius, topk,
                                                float(temperature), precision_code(), _p(ws), ws.numel(), _stream()),
               "tt_label_propagate_grid_maps")
    return maps


def upsample_argmax_hw(maps, grid, size):
    """maps [M, n, K] fp64 on a gh x gw grid -> labels [M, H, W] int64 = argmax_K of the bilinear (align_corners=False) upsampling to
    ``size`` = (H, W)."""
    lib = _lib.load()
    _chk(maps, "maps", torch.float64)
    M, n, K = maps.shape
    gh, gw = _grid(grid, n, "upsample_argmax_hw")
    H, W = (int(v) for v in size)
    out = torch.empty((M, max(H, 0), max(W, 0)), dtype=torch.int64, device=maps.device)
    _lib.check(lib.tt_upsample_argmax_hw(_p(maps), _p(out), M, gh, gw, K, H, W, _stream()), "tt_upsample_argmax_hw")
    return out


def upsample_argmax(maps, resolution: int):
    """maps [M, n, K] fp64 -> labels [M, R, R] int64 = argmax_K of the bilinear (align_corners=False) upsampling."""
    lib = _lib.load()
    _chk(maps, "maps", torch.float64)
    M, n, K = maps.shape
    g = int(round(n ** 0.5))
    assert g * g == n
    out = torch.empty((M, resolution, resolution), dtype=torch.int64, device=maps.device)
    _lib.check(lib.tt_upsample_argmax(_p(maps), _p(out), M, g, K, int(resolution), _stream()), "tt_upsample_argmax")
    return out


def confusion_counts(pred, gt, num_classes: int):
    """counts[gt, pred] over all elements, int64 [C, C] (labels outside [0, C) are ignored)."""
    lib = _lib.load()
    _chk(pred, "pred", torch.int64); _chk(gt, "gt", torch.int64)
    if pred.numel() != gt.numel():
        raise ValueError("pred and gt need the same number of elements")
    counts = torch.empty((num_classes, num_classes), dtype=torch.int64, device=pred.device)
    _lib.check(lib.tt_confusion_counts(_p(pred), _p(gt), pred.numel(), int(num_classes), _p(counts), _stream()), "tt_confusion_counts")
    return counts


_LABEL_CODES = {torch.int16: 0, torch.int64: 1}   # TT_LABELS_I16 / TT_LABELS_I64


def confusion_counts_segments(pred, gt, num_gt: int, num_pred: int, ignore_gt: Optional[int] = None):
    """pred [S, n] int16 or int64, gt [S, n] int64 -> counts[s, gt, pred] int64 [S, num_gt, num_pred], one launch for all S segments:
    every element of segment s with 0 <= gt < num_gt, 0 <= pred < num_pred and gt != ignore_gt counts once, all others are skipped."""
    lib = _lib.load()
    if pred.dtype not in _LABEL_CODES:
        raise TypeError(f"pred: expected torch.int16 or torch.int64, got {pred.dtype}")
    _chk(pred, "pred", pred.dtype); _chk(gt, "gt", torch.int64)
    if pred.dim() != 2 or pred.shape != gt.shape:
        raise ValueError(f"pred and gt: expected two [S, n] tensors of one shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    S, n = pred.shape
    counts = torch.empty((S, int(num_gt), int(num_pred)), dtype=torch.int64, device=pred.device)
    _lib.check(lib.tt_confusion_counts_segments(_p(pred), _LABEL_CODES[pred.dtype], _p(gt), S, n, int(num_gt), int(num_pred),
                                                0 if ignore_gt is None else int(ignore_gt), 0 if ignore_gt is None else 1, _p(counts),
                                                _stream()), "tt_confusion_counts_segments")
    return counts


MATCH_MODES = {"hungarian": 0, "many_to_one": 1}   # TT_MATCH_HUNGARIAN / TT_MATCH_MANY_TO_ONE


def match_segments_shape_ok(num_gt: int, num_pred: int) -> bool:
    """The shape rule of ``match_segments``: 1 <= num_gt <= 128 and 1 <= num_pred <= 1024 (``tt_match_segments_shape_ok``)."""
    return bool(_lib.load().tt_match_segments_shape_ok(int(num_gt), int(num_pred)))


class MatchedSegments:
    """The outputs of ``match_segments``, views of ONE int64 allocation ``packed``: score, matched_bg float64 [S]; tp, fp, fn int64
    [S, Cg] by gt value; lut int64 [S, Cp]; info int32 [S, 4] = (status, n_gt, n_pred, largest present pred value).  ``cpu()`` brings
    all of them to the host in one copy."""

    def __init__(self, packed: torch.Tensor, S: int, Cg: int, Cp: int):
        self.packed, self.shape = packed, (S, Cg, Cp)
        at = 0

        def take(words, *view):
            nonlocal at
            part = packed[at:at + words]
            at += words
            return part.view(*view) if view else part

        self.score = take(S).view(torch.float64)
        self.matched_bg = take(S).view(torch.float64)
        self.tp, self.fp, self.fn = take(S * Cg, S, Cg), take(S * Cg, S, Cg), take(S * Cg, S, Cg)
        self.lut = take(S * Cp, S, Cp)
        self.info = take(2 * S).view(torch.int32).view(S, 4)

    @staticmethod
    def words(S: int, Cg: int, Cp: int) -> int:
        return 2 * S + 3 * S * Cg + S * Cp + 2 * S

    def cpu(self) -> "MatchedSegments":
        return MatchedSegments(self.packed.cpu(), *self.shape)


def match_segments(counts, mode: str = "hungarian", precision_based: bool = False, involve_bg: bool = False) -> MatchedSegments:
    """counts int64 [S, Cg, Cp] (``confusion_counts_segments``) -> the matched scores of all S segments from one launch: what
    ``PredsmIoU.compute_miou_from_confusion`` returns for each matrix, with its bits.  ``mode``: "hungarian" or "many_to_one"
    (``precision_based`` is read in the latter only)."""
    lib = _lib.load()
    _chk(counts, "counts", torch.int64)
    if counts.dim() != 3:
        raise ValueError(f"counts: expected [S, Cg, Cp], got {tuple(counts.shape)}")
    if mode not in MATCH_MODES:
        raise ValueError(f"mode: expected one of {sorted(MATCH_MODES)}, got {mode!r}")
    S, Cg, Cp = counts.shape
    out = MatchedSegments(torch.empty(MatchedSegments.words(S, Cg, Cp), dtype=torch.int64, device=counts.device), S, Cg, Cp)
    _lib.check(lib.tt_match_segments(_p(counts), S, Cg, Cp, MATCH_MODES[mode], int(bool(precision_based)), int(bool(involve_bg)), _p(out.score),
                                     _p(out.matched_bg), _p(out.tp), _p(out.fp), _p(out.fn), _p(out.lut), _p(out.info), _stream()),
               "tt_match_segments")
    return out


# ---- clip input pipeline (uint8 frames [F, H, W, 3]) ------------------------------------------------------------------

def img_resample_h(frames, coeffs, bounds, y0: int, x0: int, h: int):
    """Horizontal pass of Pillow's bilinear resize over rows y0..y0+h, columns from x0: -> uint8 [F, h, OW, 3]."""
    lib = _lib.load()
    _chk(frames, "frames", torch.uint8); _chk(coeffs, "coeffs", torch.int32); _chk(bounds, "bounds", torch.int32)
    Fr, H, W, _ = frames.shape
    OW, ksize = coeffs.shape
    out = torch.empty((Fr, h, OW, 3), dtype=torch.uint8, device=frames.device)
    _lib.check(lib.tt_img_resample_h(_p(frames), _p(out), _p(coeffs), _p(bounds), Fr, H, W, y0, x0, h, OW, ksize, _stream()), "tt_img_resample_h")
    return out


def img_resample_v(frames, coeffs, bounds, y0: int = 0, to_tensor=None, flip: bool = False):
    """Vertical pass: -> uint8 [F, OH, W, 3], or with ``to_tensor=(mean, std)`` the finished float32 [F, 3, OH, W]."""
    import ctypes as C

    lib = _lib.load()
    _chk(frames, "frames", torch.uint8); _chk(coeffs, "coeffs", torch.int32); _chk(bounds, "bounds", torch.int32)
    Fr, Hin, W, _ = frames.shape
    OH, ksize = coeffs.shape
    if to_tensor is None:
        out = torch.empty((Fr, OH, W, 3), dtype=torch.uint8, device=frames.device)
        _lib.check(lib.tt_img_resample_v(_p(frames), _p(out), None, _p(coeffs), _p(bounds), Fr, Hin, W, y0, OH, ksize, 0, None, None, _stream()),
                   "tt_img_resample_v")
        return out
    mean, std = to_tensor
    out = torch.empty((Fr, 3, OH, W), dtype=f32, device=frames.device)
    m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    _lib.check(lib.tt_img_resample_v(_p(frames), None, _p(out), _p(coeffs), _p(bounds), Fr, Hin, W, y0, OH, ksize, int(bool(flip)), m3, s3,
                                     _stream()), "tt_img_resample_v")
    return out


IMG_GRAYSCALE, IMG_BRIGHTNESS, IMG_CONTRAST, IMG_SATURATION, IMG_HUE = range(5)


def img_color_(frames, mode: int, factor: float = 1.0, hue_shift: int = 0):
    """In-place colour operation on uint8 [F, H, W, 3] (modes above)."""
    lib = _lib.load()
    _chk(frames, "frames", torch.uint8)
    Fr, H, W, _ = frames.shape
    ws = torch.empty(Fr, dtype=torch.int64, device=frames.device) if mode == IMG_CONTRAST else None
    _lib.check(lib.tt_img_color(_p(frames), Fr, H, W, int(mode), float(factor), int(hue_shift), _p(ws), _stream()), "tt_img_color")
    return frames


def img_box_blur(frames, direction: int, radius: int, ww: int, fw: int):
    lib = _lib.load()
    _chk(frames, "frames", torch.uint8)
    Fr, H, W, _ = frames.shape
    out = torch.empty_like(frames)
    _lib.check(lib.tt_img_box_blur(_p(frames), _p(out), Fr, H, W, int(direction), int(radius), int(ww), int(fw), _stream()), "tt_img_box_blur")
    return out


_DEVICE_TABLES: dict = {}


def _index_table_on(tab, limit: int, device, what: str):
    """A host int32 index table -> its device copy (cached by content), after checking every entry against [0, limit): the gather
    kernel does not look."""
    t = np.ascontiguousarray(np.asarray(tab), dtype=np.int32)
    if t.ndim != 1 or t.size == 0:
        raise ValueError(f"{what}: a non-empty 1-D index table is needed")
    if int(t.min()) < 0 or int(t.max()) >= limit:
        raise ValueError(f"{what}: entries must lie in [0, {limit}), got [{int(t.min())}, {int(t.max())}]")
    key = (str(device), t.tobytes())
    hit = _DEVICE_TABLES.get(key)
    if hit is None:
        if len(_DEVICE_TABLES) > 4096:
            _DEVICE_TABLES.clear()
        hit = _DEVICE_TABLES[key] = torch.from_numpy(t).to(device)
    return hit


def _clip_dims(clip, what: str):
    _chk(clip, what, torch.uint8)
    if clip.dim() == 3:
        return (*clip.shape, 1)
    if clip.dim() == 4:
        return tuple(clip.shape)
    raise ValueError(f"{what}: a uint8 clip [F, H, W] (label maps) or [F, H, W, C] is needed, got {tuple(clip.shape)}")


def img_gather_nearest(clip, ytab, xtab, to_tensor=None):
    """``out[f, y, x] = clip[f, ytab[y], xtab[x]]`` for a uint8 clip [F, H, W] (label maps) or [F, H, W, 3] (frames); ``ytab`` /
    ``xtab`` are HOST integer tables (checked here).  Returns a uint8 clip of the input's kind, or with ``to_tensor`` the finished
    ``ClipToTensor``: ``(mean, std)`` for frames -> float32 [F, 3, OH, OW], ``True`` for label maps -> float32 [F, 1, OH, OW] = v / 255."""
    import ctypes as C

    lib = _lib.load()
    Fr, H, W, Cn = _clip_dims(clip, "clip")
    yt, xt = _index_table_on(ytab, H, clip.device, "ytab"), _index_table_on(xtab, W, clip.device, "xtab")
    OH, OW = yt.numel(), xt.numel()
    if to_tensor is None:
        out = torch.empty((Fr, OH, OW) if clip.dim() == 3 else (Fr, OH, OW, Cn), dtype=torch.uint8, device=clip.device)
        _lib.check(lib.tt_img_gather_nearest(_p(clip), _p(out), None, _p(yt), _p(xt), Fr, H, W, Cn, OH, OW, None, None, _stream()),
                   "tt_img_gather_nearest")
        return out
    out = torch.empty((Fr, Cn, OH, OW), dtype=f32, device=clip.device)
    m3 = s3 = None
    if to_tensor is not True:
        mean, std = to_tensor
        m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    _lib.check(lib.tt_img_gather_nearest(_p(clip), None, _p(out), _p(yt), _p(xt), Fr, H, W, Cn, OH, OW, m3, s3, _stream()),
               "tt_img_gather_nearest")
    return out


def img_affine_nearest(clip, coeffs):
    """Pillow's nearest affine transform with zero fill on a uint8 clip [F, H, W] or [F, H, W, 3]; ``coeffs`` are the six 16.16
    fixed-point integers (a0 .. a5) of ``video_transformations.rotate_coeffs``."""
    import ctypes as C

    lib = _lib.load()
    Fr, H, W, Cn = _clip_dims(clip, "clip")
    if len(coeffs) != 6:
        raise ValueError("six fixed-point coefficients are needed")
    a6 = (C.c_int * 6)(*[int(v) for v in coeffs])
    out = torch.empty_like(clip)
    _lib.check(lib.tt_img_affine_nearest(_p(clip), _p(out), Fr, H, W, Cn, a6, _stream()), "tt_img_affine_nearest")
    return out


def col_moments(x):
    """Per-column mean and population variance of x [rows, cols] (fp64 tensors)."""
    lib = _lib.load()
    _chk(x, "x")
    rows, cols = x.shape
    mean = torch.empty(cols, dtype=torch.float64, device=x.device)
    var = torch.empty_like(mean)
    nb = lib.tt_col_moments_workspace_bytes(rows, cols)
    ws = _ws(nb, x.device)
    _lib.check(lib.tt_col_moments(_p(x), _p(mean), _p(var), rows, cols, _p(ws), nb, _stream()), "tt_col_moments")
    return mean, var


def affine_cols_(x, scale, shift):
    """x[r, c] = x[r, c] * scale[c] + shift[c] in place."""
    lib = _lib.load()
    _chk(x, "x"); _chk(scale, "scale"); _chk(shift, "shift")
    rows, cols = x.shape
    _lib.check(lib.tt_affine_cols_inplace(_p(x), _p(scale), _p(shift), rows, cols, _stream()), "tt_affine_cols_inplace")
    return x


def upsample_bilinear_tokens(x, resolution: int):
    """x [M, g*g, C] fp32 -> [M, R*R, C] fp32 (bilinear, align_corners=False, fp64 arithmetic)."""
    lib = _lib.load()
    _chk(x, "x")
    M, n, Cc = x.shape
    g = int(round(n ** 0.5))
    assert g * g == n
    out = torch.empty((M, resolution * resolution, Cc), dtype=f32, device=x.device)
    _lib.check(lib.tt_upsample_bilinear_tokens(_p(x), _p(out), M, g, Cc, int(resolution), _stream()), "tt_upsample_bilinear_tokens")
    return out


def upsample_argmax_f32(maps, resolution: int):
    """maps [M, n, K] fp32 -> labels [M, R, R] int64 (fp32 bilinear interpolation, first maximum)."""
    lib = _lib.load()
    _chk(maps, "maps")
    M, n, K = maps.shape
    g = int(round(n ** 0.5))
    assert g * g == n
    out = torch.empty((M, resolution, resolution), dtype=torch.int64, device=maps.device)
    _lib.check(lib.tt_upsample_argmax_f32(_p(maps), _p(out), M, g, K, int(resolution), _stream()), "tt_upsample_argmax_f32")
    return out


def upsample_argmax_hist(maps, resolution: int, counts=None):
    """maps [M, n, K] fp32 -> int64 [K]: how many of the M * R * R pixels ``upsample_argmax_f32(maps, R)`` labels k, without the
    labels (one launch, integer atomics: exact).  ``counts`` (int64 [K] on the device) is ADDED to and returned; None starts from zero."""
    lib = _lib.load()
    _chk(maps, "maps")
    M, n, K = maps.shape
    g = int(round(n ** 0.5))
    if g * g != n:
        raise ValueError(f"maps: {n} tokens are not a square grid")
    if counts is None:
        counts = torch.zeros(K, dtype=torch.int64, device=maps.device)
    _chk(counts, "counts", torch.int64)
    if tuple(counts.shape) != (K,):
        raise ValueError(f"counts: expected int64 [{K}], got {tuple(counts.shape)}")
    _lib.check(lib.tt_upsample_argmax_hist_f32(_p(maps), _p(counts), M, g, K, int(resolution), _stream()), "tt_upsample_argmax_hist_f32")
    return counts


# ---- overlay rendering (N17) ---------------------------------------------------------------------------------------------

OVERLAY_PHOTO, OVERLAY_LABELS = 0, 1                                       # TT_OVERLAY_PHOTO / TT_OVERLAY_LABELS
_OVERLAY_LABEL_CODES = {torch.int16: 0, torch.int64: 1, torch.uint8: 2}    # TT_LABELS_I16 / _I64 / _U8


def overlay_grid(mode: int, labels_a, palette, frames=None, labels_b=None, size=None, ytab=None, xtab=None, lut=None, alpha: float = 0.5,
                 pad: int = 2, mean=None, std=None):
    """One launch renders every frame of a batch as uint8 [F, 3, H + 2 pad, n W + (n + 1) pad] (``make_grid``'s layout, pad value 0).

    ``OVERLAY_PHOTO``  (n = 2): ``[base | blend(base, colour(labels_a))]`` with ``frames`` float32 [F, 3, H, W] and
    ``base = uint8(clamp(trunc((x * std + mean) * 255), 0, 255))`` (``mean`` / ``std``: 3 numbers each, None = 0 / 1).
    ``OVERLAY_LABELS`` (n = 3): ``[colour(labels_b) | colour(labels_a) | blend(colour(labels_b), colour(labels_a))]``, (H, W) = ``size``
    or the maps' own.

    ``labels_*`` [F, Hl, Wl] uint8 / int16 / int64 (one dtype); where (Hl, Wl) != (H, W) the HOST index tables ``ytab`` [H] / ``xtab`` [W]
    say which map row / column a pixel reads (checked here).  ``palette`` uint8 [P, 3]; ``colour(v) = palette[idx mod P]`` with
    ``idx = lut[v]`` (``lut`` [L]) or ``lut[f, v]`` ([F, L]) for ``labels_a`` where a LUT is given (a v outside [0, L) gives 0), else
    ``idx = v``; ``labels_b``, the ground truth, is never mapped.
    ``blend = uint8(a * (1 - alpha) + b * alpha)`` in three rounded fp32 operations."""
    import ctypes as C

    lib = _lib.load()
    if labels_a.dtype not in _OVERLAY_LABEL_CODES:
        raise TypeError(f"labels_a: expected torch.uint8, torch.int16 or torch.int64, got {labels_a.dtype}")
    _chk(labels_a, "labels_a", labels_a.dtype)
    if labels_a.dim() != 3:
        raise ValueError(f"labels_a: expected [F, Hl, Wl], got {tuple(labels_a.shape)}")
    Fr, Hl, Wl = labels_a.shape
    dev = labels_a.device
    if labels_b is not None:
        _chk(labels_b, "labels_b", labels_a.dtype)
        if labels_b.shape != labels_a.shape:
            raise ValueError(f"labels_b {tuple(labels_b.shape)} and labels_a {tuple(labels_a.shape)} need one shape")
    if mode == OVERLAY_PHOTO:
        if frames is None:
            raise ValueError("overlay_grid: the photo mode needs the frames")
        _chk(frames, "frames")
        if frames.dim() != 4 or frames.shape[0] != Fr or frames.shape[1] != 3:
            raise ValueError(f"frames: expected [{Fr}, 3, H, W], got {tuple(frames.shape)}")
        H, W = frames.shape[2:]
    elif mode == OVERLAY_LABELS:
        if labels_b is None:
            raise ValueError("overlay_grid: the labels mode needs labels_b (the ground truth)")
        H, W = (Hl, Wl) if size is None else (int(size[0]), int(size[1]))
        frames = None
    else:
        raise ValueError(f"overlay_grid: unknown mode {mode!r}")
    if H <= 0 or W <= 0 or Fr <= 0:
        raise ValueError(f"overlay_grid: {Fr} frames of {H} x {W}")
    yt = xt = None
    if (ytab is None) != (xtab is None):
        raise ValueError("overlay_grid: ytab and xtab come together")
    if ytab is not None:
        yt, xt = _index_table_on(ytab, Hl, dev, "ytab"), _index_table_on(xtab, Wl, dev, "xtab")
        if yt.numel() != H or xt.numel() != W:
            raise ValueError(f"overlay_grid: tables of {yt.numel()} rows and {xt.numel()} columns for frames of {H} x {W}")
    elif (Hl, Wl) != (H, W):
        raise ValueError(f"overlay_grid: label maps of {Hl} x {Wl} under frames of {H} x {W} need ytab and xtab")
    pal = torch.as_tensor(palette)
    if pal.dtype != torch.uint8 or pal.dim() != 2 or pal.shape[1] != 3 or pal.shape[0] < 1:
        raise ValueError(f"palette: expected uint8 [P, 3], got {pal.dtype} {tuple(pal.shape)}")
    pal = pal.to(dev).contiguous()
    lut_t, lut_len, lut_stride = None, 0, 0
    if lut is not None:
        lut_t = torch.as_tensor(lut)
        if lut_t.dim() not in (1, 2) or lut_t.shape[-1] < 1 or (lut_t.dim() == 2 and lut_t.shape[0] != Fr) or lut_t.is_floating_point():
            raise ValueError(f"lut: expected integers [L] or [{Fr}, L], got {lut_t.dtype} {tuple(lut_t.shape)}")
        lut_t = lut_t.to(device=dev, dtype=torch.int32).contiguous()
        lut_len = int(lut_t.shape[-1])
        lut_stride = lut_len if lut_t.dim() == 2 else 0
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"overlay_grid: alpha = {alpha} outside [0, 1]")
    if pad < 0:
        raise ValueError(f"overlay_grid: pad = {pad}")
    n = 2 if mode == OVERLAY_PHOTO else 3
    out = torch.empty((Fr, 3, H + 2 * pad, n * W + (n + 1) * pad), dtype=torch.uint8, device=dev)
    m3 = None if mean is None else (C.c_float * 3)(*[float(v) for v in mean])
    s3 = None if std is None else (C.c_float * 3)(*[float(v) for v in std])
    _lib.check(lib.tt_overlay_grid(_p(out), int(mode), _p(frames), m3, s3, _p(labels_a), _p(labels_b), _OVERLAY_LABEL_CODES[labels_a.dtype],
                                   Hl, Wl, _p(yt), _p(xt), _p(lut_t), lut_len, lut_stride, _p(pal), int(pal.shape[0]), float(alpha), Fr, H, W,
                                   int(pad), _stream()), "tt_overlay_grid")
    return out


def kmeans_shape_ok(d: int, k: int) -> bool:
    """Whether ``kmeans_assign`` and ``kmeans_accumulate`` take k centroids of d columns (one rule for both: tt_kmeans_shape_ok)."""
    return bool(_lib.load().tt_kmeans_shape_ok(int(d), int(k)))


def _kmeans_assign(entry: str, x, centroids, return_dist, *tile):
    """labels / dist2 of ``x`` and the call of the assignment entry ``entry`` (``tile``: the tiled entry's tile_k)."""
    lib = _lib.load()
    _chk(x, "x"); _chk(centroids, "centroids")
    P, d = x.shape
    k = centroids.shape[0]
    labels = torch.empty(P, dtype=torch.int32, device=x.device)
    dist2 = torch.empty(P, dtype=f32, device=x.device) if return_dist else None
    _lib.check(getattr(lib, entry)(_p(x), _p(centroids), _p(labels), _p(dist2), P, d, k, *tile, _stream()), entry)
    return (labels, dist2) if return_dist else labels


def _kmeans_accumulate(entry: str, x, labels, k: int, *tile):
    """sums / counts, the workspace and the call of the accumulation entry ``entry`` (``tile``: the tiled entry's tile_k)."""
    lib = _lib.load()
    _chk(x, "x"); _chk(labels, "labels", torch.int32)
    P, d = x.shape
    sums = torch.empty((k, d), dtype=torch.float64, device=x.device)
    counts = torch.empty(k, dtype=torch.int64, device=x.device)
    nb = getattr(lib, entry + "_workspace_bytes")(P, d, k, *tile)
    ws = _ws(nb, x.device)
    _lib.check(getattr(lib, entry)(_p(x), _p(labels), _p(sums), _p(counts), P, d, k, *tile, _p(ws), nb, _stream()), entry)
    return sums, counts


def kmeans_assign(x, centroids, return_dist=False):
    """x [P, d], centroids [k, d] -> labels int32 [P] (+ squared distances)."""
    return _kmeans_assign("tt_kmeans_assign", x, centroids, return_dist)


def kmeans_accumulate(x, labels, k: int):
    """Sums [k, d] (fp64) and counts [k] (int64) of the points of each label."""
    return _kmeans_accumulate("tt_kmeans_accumulate", x, labels, k)


def kmeans_tiled_shape_ok(d: int, k: int) -> bool:
    """Whether ``kmeans_assign_tiled`` and ``kmeans_accumulate_tiled`` take k centroids of d columns (tt_kmeans_tiled_shape_ok)."""
    return bool(_lib.load().tt_kmeans_tiled_shape_ok(int(d), int(k)))


def kmeans_tile_centroids(d: int) -> int:
    """The default (and largest) ``tile_k`` at d columns: the centroid rows that fill at most 64 KB of LDS."""
    return int(_lib.load().tt_kmeans_tile_centroids(int(d)))


def kmeans_assign_tiled(x, centroids, return_dist=False, tile_k: int = 0):
    """``kmeans_assign`` for centroids that do not fit in LDS: they pass through it ``tile_k`` rows at a time (0 = the default tile).
    Same layouts and dtypes, and the same bits wherever ``kmeans_assign`` runs."""
    return _kmeans_assign("tt_kmeans_assign_tiled", x, centroids, return_dist, int(tile_k))


def kmeans_accumulate_tiled(x, labels, k: int, tile_k: int = 0):
    """``kmeans_accumulate`` for k * d beyond the LDS: sums [k, d] (fp64) and counts [k] (int64), one tile of ``tile_k`` clusters at a
    time (0 = the default tile).  The same bits wherever ``kmeans_accumulate`` runs."""
    return _kmeans_accumulate("tt_kmeans_accumulate_tiled", x, labels, k, int(tile_k))


def kmeans_fit_shape_ok(n: int, d: int, k: int) -> bool:
    """Whether ``kmeans_fit_batched`` takes problems of n points, d columns and k clusters (tt_kmeans_fit_shape_ok)."""
    return bool(_lib.load().tt_kmeans_fit_shape_ok(int(n), int(d), int(k)))


def kmeans_fit_batched(x, init, niter: int, split_draws=None):
    """The Lloyd loops of B problems in one launch: x [B, n, d], init int32 [nredo, k] on the HOST (rows of each problem's points that
    seed redo r) -> centroids [B, nredo, k, d], obj fp64 [B, nredo], status int32 [B, nredo] (0, or the 1-based iteration at which an
    empty cluster ended that redo: its centroids and objective are then unspecified).  Everything stays on the device.
    ``split_draws``: None = tt_kmeans_fit_batched (an empty cluster ends the redo); a float64 tensor on x's device - the first values of
    ``numpy.random.RandomState(1234).random_sample()``, ``clustering.split_draws`` - = tt_kmeans_fit_batched_split: empty clusters are
    split in the kernel as ``Kmeans._split_empty`` does, and a redo ends with a non-zero status only where one split call would read
    past the table."""
    lib = _lib.load()
    _chk(x, "x")
    if split_draws is not None:
        _chk(split_draws, "split_draws", torch.float64)
        if split_draws.dim() != 1 or split_draws.device != x.device:
            raise ValueError(f"split_draws: expected a 1-d table on {x.device}, got {tuple(split_draws.shape)} on {split_draws.device}")
    B, n, d = x.shape
    init_h = torch.as_tensor(init, dtype=torch.int32).cpu().contiguous()
    if init_h.dim() != 2:
        raise ValueError(f"init: expected [nredo, k], got {tuple(init_h.shape)}")
    nredo, k = init_h.shape
    init_d = init_h.to(x.device)
    cent = torch.empty((B, nredo, k, d), dtype=f32, device=x.device)
    obj = torch.empty((B, nredo), dtype=torch.float64, device=x.device)
    status = torch.empty((B, nredo), dtype=torch.int32, device=x.device)
    step = max(1, min(B, 65535))   # problems of one launch (they ride on gridDim.y)
    nb = lib.tt_kmeans_fit_workspace_bytes(step, nredo, n, d, k)
    ws = _ws(nb, x.device)
    for b0 in range(0, B, step):
        b1 = min(b0 + step, B)
        args = (_p(x[b0:b1]), _p(init_d), _p(init_h), _p(cent[b0:b1]), _p(obj[b0:b1]), _p(status[b0:b1]), b1 - b0, n, d, k, nredo, int(niter),
                _p(ws), nb)
        if split_draws is None:
            _lib.check(lib.tt_kmeans_fit_batched(*args, _stream()), "tt_kmeans_fit_batched")
        else:
            _lib.check(lib.tt_kmeans_fit_batched_split(*args, _p(split_draws), split_draws.numel(), _stream()), "tt_kmeans_fit_batched_split")
    return cent, obj, status


def kmeans_loop_shape_ok(n: int, d: int, k: int) -> bool:
    """Whether ``kmeans_fit_loop`` takes a fit of n points, d columns and k clusters (tt_kmeans_loop_shape_ok)."""
    return bool(_lib.load().tt_kmeans_loop_shape_ok(int(n), int(d), int(k)))


def kmeans_loop_workspace_bytes(n: int, d: int, k: int, nredo: int, redo_group: int = 0) -> int:
    """The workspace of ``kmeans_fit_loop`` with ``redo_group`` redos in flight (0 = all ``nredo``); 0 for a refused shape."""
    return int(_lib.load().tt_kmeans_loop_workspace_bytes(int(n), int(d), int(k), int(nredo), int(redo_group)))


def kmeans_fit_loop(x, init, niter: int, draws=None, tile_k: int = 0, redo_group: int = 0, return_last: bool = False):
    """Every redo and Lloyd iteration of ONE fit enqueued on the current stream: x [n, d], init int32 [nredo, k] on the HOST (rows of x
    that seed redo r) -> centroids [nredo, k, d], obj fp64 [nredo], status int32 [nredo] (0, or the 1-based iteration at which the redo
    ended: its centroids and objective are then unspecified).  Nothing is read back here.  ``draws``: a float64 table on x's device
    (``clustering.split_draws``) from which empty clusters are split as ``Kmeans._split_empty`` does; None = no split, the first empty
    cluster ends the redo.  ``tile_k``: 0 = the resident kernels where they take (d, k), the tiled ones at their default tile otherwise;
    a value asks for the tiled ones.  ``redo_group``: redos of one launch (0 = all; fewer = a smaller workspace, the same result).
    ``return_last`` (testing aid, all redos in one pass only): also the last iteration's labels int32 [nredo, n] and dist2 [nredo, n]."""
    lib = _lib.load()
    _chk(x, "x")
    if draws is not None:
        _chk(draws, "draws", torch.float64)
        if draws.dim() != 1 or draws.device != x.device:
            raise ValueError(f"draws: expected a 1-d table on {x.device}, got {tuple(draws.shape)} on {draws.device}")
    n, d = x.shape
    init_h = torch.as_tensor(init, dtype=torch.int32).cpu().contiguous()
    if init_h.dim() != 2:
        raise ValueError(f"init: expected [nredo, k], got {tuple(init_h.shape)}")
    nredo, k = init_h.shape
    if return_last and 0 < int(redo_group) < nredo:
        raise ValueError(f"return_last: the workspace holds the last pass only (redo_group = {redo_group} of {nredo} redos)")
    init_d = init_h.to(x.device)
    cent = torch.empty((nredo, k, d), dtype=f32, device=x.device)
    obj = torch.empty(nredo, dtype=torch.float64, device=x.device)
    status = torch.empty(nredo, dtype=torch.int32, device=x.device)
    nb = lib.tt_kmeans_loop_workspace_bytes(n, d, k, nredo, int(redo_group))
    ws = _ws(nb, x.device)
    _lib.check(lib.tt_kmeans_fit_loop(_p(x), _p(init_d), _p(init_h), _p(cent), _p(obj), _p(status), n, d, k, nredo, int(niter), int(tile_k),
                                      int(redo_group), _p(draws), 0 if draws is None else draws.numel(), _p(ws), nb, _stream()),
               "tt_kmeans_fit_loop")
    if not return_last:
        return cent, obj, status
    lab_off, d2_off = C.c_size_t(), C.c_size_t()   # where the library keeps them in its workspace
    if not lib.tt_kmeans_loop_last_offsets(n, d, k, nredo, int(redo_group), C.addressof(lab_off), C.addressof(d2_off)):
        raise _lib.HipLibraryError("tt_kmeans_loop_last_offsets refused the shape tt_kmeans_fit_loop took")
    size = 4 * nredo * n
    return (cent, obj, status, ws[lab_off.value: lab_off.value + size].view(torch.int32).view(nredo, n).clone(),
            ws[d2_off.value: d2_off.value + size].view(f32).view(nredo, n).clone())


def kmeans_assign_batched(x, centroids, return_dist=False):
    """x [B, N, d], centroids [B, k, d] -> labels int32 [B, N] (+ squared distances): ``kmeans_assign`` per problem, in one launch."""
    lib = _lib.load()
    _chk(x, "x"); _chk(centroids, "centroids")
    B, N, d = x.shape
    if centroids.shape[0] != B or centroids.shape[2] != d:
        raise ValueError(f"centroids: expected [{B}, k, {d}], got {tuple(centroids.shape)}")
    k = centroids.shape[1]
    labels = torch.empty((B, N), dtype=torch.int32, device=x.device)
    dist2 = torch.empty((B, N), dtype=f32, device=x.device) if return_dist else None
    _lib.check(lib.tt_kmeans_assign_batched(_p(x), _p(centroids), _p(labels), _p(dist2), B, N, d, k, _stream()), "tt_kmeans_assign_batched")
    return (labels, dist2) if return_dist else labels


def ce_loss_fwd_bwd(scores, labels, temperature=0.1, need_grad=True, row_weight=None):
    """mean CE of scores/temperature vs labels (per-row weights = the --use_mask loss mask); returns (loss[1], dscores or None)."""
    lib = _lib.load()
    _chk(scores, "scores"); _chk(labels, "labels", torch.int64)
    if row_weight is not None:
        _chk(row_weight, "row_weight")
        if row_weight.numel() != scores.shape[0]:
            raise ValueError("row_weight needs one entry per score row")
    rows, K = scores.shape
    loss = torch.empty((1,), dtype=f32, device=scores.device)
    ds = torch.empty_like(scores) if need_grad else None
    nb = lib.tt_ce_workspace_bytes(rows)
    ws = _ws(nb, scores.device)
    _lib.check(lib.tt_ce_loss_fwd_bwd(_p(scores), _p(labels), _p(row_weight), _p(loss), _p(ds), rows, K, float(temperature), _p(ws), nb,
                                      _stream()), "tt_ce_loss_fwd_bwd")
    return loss, ds


def foreground_mask(qkv, num_heads: int, spatial_res: int, threshold: float = 0.65, blur_sigma: float = 0.6, kernel_size: int = 7,
                    return_aux: bool = False):
    """process_attentions (models.py:93-131) from the last block's qkv activations [F, N, 3*D] -> mask [F, g*g] in {0,1}
    (and, with ``return_aux``, the blurred head-mean attention and each pixel's distance to the mass cut)."""
    lib = _lib.load()
    _chk(qkv, "qkv")
    Fr, N, D3 = qkv.shape
    hd = D3 // 3 // num_heads
    n = N - 1
    mask = torch.empty((Fr, n), dtype=f32, device=qkv.device)
    blurred = torch.empty_like(mask) if return_aux else None
    margin = torch.empty_like(mask) if return_aux else None
    _lib.check(lib.tt_foreground_mask(_p(qkv), _p(mask), _p(blurred), _p(margin), Fr, N, num_heads, hd, spatial_res, float(hd) ** -0.5,
                                      float(threshold), float(blur_sigma), int(kernel_size), _stream()), "tt_foreground_mask")
    return (mask, blurred, margin) if return_aux else mask


def foreground_mask_from_probs(cls_probs, spatial_res: int, threshold: float = 0.65, blur_sigma: float = 0.6, kernel_size: int = 7,
                               return_aux: bool = False):
    """Same from row 0 of the attention probabilities, cls_probs [F, H, N]."""
    lib = _lib.load()
    _chk(cls_probs, "cls_probs")
    Fr, H, N = cls_probs.shape
    mask = torch.empty((Fr, N - 1), dtype=f32, device=cls_probs.device)
    blurred = torch.empty_like(mask) if return_aux else None
    margin = torch.empty_like(mask) if return_aux else None
    _lib.check(lib.tt_foreground_mask_from_probs(_p(cls_probs), _p(mask), _p(blurred), _p(margin), Fr, N, H, spatial_res, float(threshold),
                                                 float(blur_sigma), int(kernel_size), _stream()), "tt_foreground_mask_from_probs")
    return (mask, blurred, margin) if return_aux else mask


def scale_rows_(x, row_scale):
    """x[r, :] *= row_scale[r] in place (features * mask, models.py:142)."""
    lib = _lib.load()
    _chk(x, "x"); _chk(row_scale, "row_scale")
    rows, cols = x.shape
    if row_scale.numel() != rows:
        raise ValueError("row_scale needs one entry per row")
    _lib.check(lib.tt_scale_rows_inplace(_p(x), _p(row_scale), rows, cols, _stream()), "tt_scale_rows_inplace")
    return x


def queue_push_(queue, feats, idx):
    lib = _lib.load()
    _chk(queue, "queue"); _chk(feats, "feats"); _chk(idx, "idx", torch.int64)
    Q, D = queue.shape
    m = idx.numel()
    scratch = torch.empty_like(queue)
    _lib.check(lib.tt_queue_push(_p(queue), _p(scratch), _p(feats), _p(idx), Q, D, m, _stream()), "tt_queue_push")
    return queue


# ---- optimiser -------------------------------------------------------------------------------------

def adamw_step_(entries: Sequence[tuple], step: int, beta1=0.9, beta2=0.999, eps=1e-8):
    """entries: (param, grad, exp_avg, exp_avg_sq, lr, weight_decay) tuples, all fp32 GPU contiguous."""
    _bump_param_epoch()
    lib = _lib.load()
    cap = 40
    for i in range(0, len(entries), cap):
        chunk = entries[i:i + cap]
        arr = (_lib.AdamwTensor * len(chunk))()
        for j, (p, g, m, v, lr, wd) in enumerate(chunk):
            for t, nm in ((p, "param"), (g, "grad"), (m, "exp_avg"), (v, "exp_avg_sq")):
                _chk(t, nm)
            arr[j] = _lib.AdamwTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr), float(wd))
        _lib.check(lib.tt_adamw_step(arr, len(chunk), int(step), float(beta1), float(beta2), float(eps), _stream()), "tt_adamw_step")


def scale_tensors_(tensors: Sequence[torch.Tensor], scale: torch.Tensor):
    """t *= scale for every tensor (scale: a one-element fp32 GPU tensor), one launch per 40 tensors."""
    lib = _lib.load()
    _chk(scale, "scale")
    cap = 40
    for i in range(0, len(tensors), cap):
        chunk = tensors[i:i + cap]
        arr = (_lib.AdamwTensor * len(chunk))()
        for j, t in enumerate(chunk):
            _chk(t, "tensor")
            arr[j] = _lib.AdamwTensor(None, t.data_ptr(), None, None, t.numel(), 0.0, 0.0)
        _lib.check(lib.tt_scale_tensors(arr, len(chunk), _p(scale), _stream()), "tt_scale_tensors")


def ema_update_(teacher, student, momentum: float):
    """teacher <- teacher * (1 - m) + student * m  (time_tuning.py:113-115)."""
    _bump_param_epoch()
    lib = _lib.load()
    _chk(teacher, "teacher"); _chk(student, "student")
    assert teacher.numel() == student.numel()
    _lib.check(lib.tt_ema_update(_p(teacher), _p(student), teacher.numel(), float(momentum), _stream()), "tt_ema_update")
    return teacher


def add_(dst, src):
    lib = _lib.load()
    _chk(dst, "dst"); _chk(src, "src")
    _lib.check(lib.tt_add_inplace(_p(dst), _p(src), dst.numel(), _stream()), "tt_add_inplace")
    return dst


def count_mismatch(a, b) -> int:
    """Number of positions where two fp32 buffers differ bitwise; synchronises (a one-off check, not a step op)."""
    lib = _lib.load()
    _chk(a, "a"); _chk(b, "b")
    assert a.numel() == b.numel()
    out = torch.empty((1,), dtype=torch.int64, device=a.device)
    _lib.check(lib.tt_count_mismatch(_p(a), _p(b), a.numel(), _p(out), _stream()), "tt_count_mismatch")
    return int(out.item())


# ---- bf16-plane operands (include/timetuning_hip.h: "bf16-plane operands") ------------------------------------------------
bf16 = torch.bfloat16


def split_planes(x, planes: int, out=None):
    """fp32 tensor -> [planes, *x.shape] bf16 with x = sum of the planes (exactly, for planes = 3)."""
    lib = _lib.load()
    _chk(x, "x")
    n = x.numel()
    if n % 8:
        raise ValueError("split_planes: the element count must be a multiple of 8")
    y = out if out is not None else torch.empty((planes, *x.shape), dtype=bf16, device=x.device)
    _lib.check(lib.tt_split_planes(_p(x), _p(y), n, int(planes), n, _stream()), "tt_split_planes")
    return y


def layernorm_fwd_planes(x, gamma, beta, planes: int, eps=1e-6, save_stats=False, drop_first_token=False):
    """LayerNorm whose result is written as bf16 planes [planes, rows, D] (see ``layernorm_fwd`` for the arguments)."""
    def alloc(rows, D):
        return torch.empty((planes, rows, D), dtype=bf16, device=x.device), rows * D, int(planes)
    return _layernorm_fwd_into("tt_layernorm_fwd_planes", alloc, x, gamma, beta, eps, save_stats, drop_first_token)


def linear_fwd_planes(xp, wp, bias=None, residual=None, act: int = 0, out_f32: bool = True, out_planes: int = 0, save_pre: bool = False,
                      out=None):
    """y = act(x @ w.T + bias) (+ residual) on bf16-plane operands xp [P, M, K], wp [P, N, K].  Returns a dict with the
    requested outputs: ``y`` (fp32 [M,N]), ``planes`` (bf16 [out_planes, M, N]), ``pre`` (fp32 pre-activation)."""
    lib = _lib.load()
    _chk(xp, "xp", bf16); _chk(wp, "wp", bf16)
    P, M, K = xp.shape
    N = wp.shape[1]
    assert wp.shape[0] == P and wp.shape[2] == K, (xp.shape, wp.shape)
    if bias is not None: _chk(bias, "bias")
    if residual is not None: _chk(residual, "residual")
    y = (out if out is not None else torch.empty((M, N), dtype=f32, device=xp.device)) if out_f32 else None
    yp = torch.empty((out_planes, M, N), dtype=bf16, device=xp.device) if out_planes else None
    pre = torch.empty((M, N), dtype=f32, device=xp.device) if save_pre else None
    # (profiled runs book the launch under the kernel that really runs it)
    p8 = PROFILE is not None and lib.tt_linear_fwd_planes_route(P, M, N, K, int(act), int(bias is not None), int(residual is not None),
                                                                int(y is not None), int(out_planes), int(pre is not None)) == 8
    e0 = _prof_begin()
    kws = ksplit_workspace(xp.device)
    _lib.check(lib.tt_linear_fwd_planes(_p(xp), M * K, _p(wp), N * K, P, _p(bias), _p(residual), _p(y), _p(pre), _p(yp), M * N, int(out_planes),
                                        M, N, K, int(act), _p(kws), kws.numel(), _stream()), "tt_linear_fwd_planes")
    _prof_end(e0, f"PLANES8_{P}" if p8 else f"PLANES{P}", M, N, K)
    return dict(y=y, planes=yp, pre=pre)


_RANGE_PENDING: dict = {}


def poll_pair_range(device=None) -> None:
    """``check_pair_range`` without a synchronisation, for the per-step path: the flag travels to a pinned host word asynchronously, and the
    call raises PairRangeError when a PREVIOUS poll's copy has landed with the flag set (detection lags by one step)."""
    f = range_flag(device)
    if f is None:
        return
    idx = f.device.index
    pend = _RANGE_PENDING.get(idx)
    if pend is None:
        pend = _RANGE_PENDING[idx] = dict(host=torch.zeros(4, dtype=torch.int32).pin_memory(), event=None)
    if pend["event"] is not None and pend["event"].query():
        pend["event"] = None
        if int(pend["host"][0]) != 0:
            check_pair_range(device)   # (synchronises, resets, raises)
    if pend["event"] is None:
        pend["host"].copy_(f, non_blocking=True)
        pend["event"] = torch.cuda.Event()
        pend["event"].record()


# ---- fp16-pair operands (include/timetuning_hip.h: "fp16-PAIR operands") ------------------------------------------------------
f16 = torch.float16


def split_pairs(x, out=None):
    """fp32 tensor [..., C] (C % 32 == 0) -> fp16 pairs [..., 2 C]: groups of 32 elements as [hi x 32][lo x 32]."""
    lib = _lib.load()
    _chk(x, "x")
    if x.shape[-1] % 32:
        raise ValueError("split_pairs: the last dimension must be a multiple of 32")
    y = out if out is not None else torch.empty((*x.shape[:-1], 2 * x.shape[-1]), dtype=f16, device=x.device)
    _lib.check(lib.tt_split_pairs(_p(x), _p(y), x.numel(), _p(range_flag(x.device)), _stream()), "tt_split_pairs")
    return y


def join_pairs(xp):
    """fp16 pairs [..., 2 C] -> fp32 [..., C] (hi + lo 2^-11)."""
    lib = _lib.load()
    _chk(xp, "xp", f16)
    y = torch.empty((*xp.shape[:-1], xp.shape[-1] // 2), dtype=f32, device=xp.device)
    _lib.check(lib.tt_join_pairs(_p(xp), _p(y), y.numel(), _stream()), "tt_join_pairs")
    return y


def layernorm_fwd_pairs(x, gamma, beta, eps=1e-6, save_stats=False, drop_first_token=False):
    """LayerNorm whose result is written as fp16 pairs [rows, 2 D] (see ``layernorm_fwd`` for the arguments)."""
    def alloc(rows, D):
        return (torch.empty((rows, 2 * D), dtype=f16, device=x.device),)
    return _layernorm_fwd_into("tt_layernorm_fwd_pairs", alloc, x, gamma, beta, eps, save_stats, drop_first_token, _p(range_flag(x.device)))


def linear_fwd_pairs(xp, wp, bias=None, residual=None, act: int = 0, out_f32: bool = True, out_pairs: bool = False, save_pre: bool = False,
                     out=None):
    """y = act(x @ w.T + bias) (+ residual) on fp16-pair operands xp [M, 2 K], wp [N, 2 K].  Returns a dict with the requested
    outputs: ``y`` (fp32 [M,N]), ``pairs`` (fp16 [M, 2 N]), ``pre`` (fp32 pre-activation)."""
    lib = _lib.load()
    _chk(xp, "xp", f16); _chk(wp, "wp", f16)
    M, K2 = xp.shape
    N = wp.shape[0]
    K = K2 // 2
    assert wp.shape[1] == K2, (xp.shape, wp.shape)
    if bias is not None: _chk(bias, "bias")
    if residual is not None: _chk(residual, "residual")
    y = (out if out is not None else torch.empty((M, N), dtype=f32, device=xp.device)) if out_f32 else None
    yp = torch.empty((M, 2 * N), dtype=f16, device=xp.device) if out_pairs else None
    pre = torch.empty((M, N), dtype=f32, device=xp.device) if save_pre else None
    p8 = PROFILE is not None and lib.tt_linear_fwd_pairs_route(M, N, K, int(act), int(bias is not None), int(residual is not None),
                                                               int(y is not None), int(yp is not None), int(pre is not None)) == 8
    e0 = _prof_begin()
    kws = ksplit_workspace(xp.device)
    _lib.check(lib.tt_linear_fwd_pairs(_p(xp), _p(wp), _p(bias), _p(residual), _p(y), _p(pre), _p(yp), M, N, K, int(act), _p(kws), kws.numel(),
                                       _p(range_flag(xp.device)) if yp is not None else None, _stream()), "tt_linear_fwd_pairs")
    _prof_end(e0, "PAIRS8" if p8 else "PAIRS", M, N, K)
    return dict(y=y, pairs=yp, pre=pre)


def attention_pairs_ok(N: int, head_dim: int) -> bool:
    """Shapes ``attention_fwd_pairs`` takes (any N: K / V resident in LDS up to 256 tokens, the KV-tiled kernel beyond)."""
    return head_dim == 64


def attention_fwd_pairs(qkv_pairs, num_heads: int, out_pairs: bool = True, out_f32: bool = False, save_lse: bool = False):
    """qkv [F, N, 2 * 3D] fp16 pairs -> (out pairs [F, N, 2 D] or None, out fp32 [F, N, D] or None, lse [F, H, N] or None)."""
    lib = _lib.load()
    _chk(qkv_pairs, "qkv_pairs", f16)
    F, N, D6 = qkv_pairs.shape
    D = D6 // 6
    hd = D // num_heads
    op = torch.empty((F, N, 2 * D), dtype=f16, device=qkv_pairs.device) if out_pairs else None
    of = torch.empty((F, N, D), dtype=f32, device=qkv_pairs.device) if out_f32 else None
    lse = torch.empty((F, num_heads, N), dtype=f32, device=qkv_pairs.device) if save_lse else None
    _lib.check(lib.tt_attention_fwd_pairs(_p(qkv_pairs), _p(op), _p(of), _p(lse), F, N, num_heads, hd, float(hd ** -0.5), _stream()),
               "tt_attention_fwd_pairs")
    return op, of, lse


def split_pairs_dual(x, want_row: bool = False, want_colsum: bool = False, rpad: Optional[int] = None, colsum_out=None, want_t: bool = True,
                     scaled: bool = False, colsum_parts: bool = False, amax_in=None):
    """fp32 [R, C] -> (transposed pairs [C, 2 Rpad] or None, row-major pairs [R, 2 C] or None, column sums [C] or None) in ONE pass
    (tt_split_pairs_dual): what the backward of an nn.Linear needs of its dy.  ``scaled`` (a GRADIENT, whose whole magnitude may sit
    below fp16's normal range): the pairs hold x * S with S the power of two that brings max |x| into [2^13, 2^14); a fourth value is
    returned, the DEVICE scalar S, which the products take as ``dy_scale`` and divide by (no host round trip).
    ``colsum_parts`` (tt_split_pairs_dual_parts): the column sums come back UNFOLDED, as the partials of 64-row blocks [ceil(Rpad / 64), C],
    for ``linear_bwd_weight_pairs_tn(..., colsum_parts=, db_out=)`` to fold in the launch that folds the weight gradient."""
    lib = _lib.load()
    _chk(x, "x")
    R, Cc = x.shape
    rpad = (R + 31) // 32 * 32 if rpad is None else rpad
    assert want_t or want_row
    if colsum_parts:
        assert want_colsum and colsum_out is None
        t = torch.empty((Cc, 2 * rpad), dtype=f16, device=x.device) if want_t else None
        row = torch.empty((R, 2 * Cc), dtype=f16, device=x.device) if want_row else None
        parts = torch.empty(((rpad + 63) // 64, Cc), dtype=f32, device=x.device)
        own_max = scaled and amax_in is None
        nb = lib.tt_split_pairs_dual_workspace_bytes(R, Cc, rpad) if own_max else 0
        ws = _ws(nb, x.device) if own_max else None
        scale = torch.empty((1,), dtype=f32, device=x.device) if scaled else None
        _lib.check(lib.tt_split_pairs_dual_parts(_p(x), _p(t), _p(row), _p(parts), _p(scale), _p(amax_in) if scaled else None, R, Cc, rpad, _p(ws), nb,
                                                 _p(range_flag(x.device)), _stream()), "tt_split_pairs_dual_parts")
        return (t, row, parts, scale) if scaled else (t, row, parts)
    t = torch.empty((Cc, 2 * rpad), dtype=f16, device=x.device) if want_t else None
    row = torch.empty((R, 2 * Cc), dtype=f16, device=x.device) if want_row else None
    sums = (_chk(colsum_out, "colsum_out") if colsum_out is not None else torch.empty((Cc,), dtype=f32, device=x.device)) if want_colsum else None
    need_ws = want_colsum or scaled
    nb = lib.tt_split_pairs_dual_workspace_bytes(R, Cc, rpad) if need_ws else 0
    ws = _ws(nb, x.device) if need_ws else None
    scale = torch.empty((1,), dtype=f32, device=x.device) if scaled else None
    _lib.check(lib.tt_split_pairs_dual(_p(x), _p(t), _p(row), _p(sums), _p(scale), R, Cc, rpad, _p(ws), nb, _p(range_flag(x.device)), _stream()),
               "tt_split_pairs_dual")
    return (t, row, sums, scale) if scaled else (t, row, sums)


def split_pairs_dual_multi(items) -> None:
    """``items``: (x fp32 [R, C], row pairs out [R, 2 C] or None, transposed pairs out [C, 2 Rpad] or None) - every matrix converted in ONE
    launch per 32 of them (tt_split_pairs_dual_multi): the pair operands of all the weights an optimizer / EMA update rewrote."""
    import ctypes as C
    lib = _lib.load()
    n = len(items)
    if n == 0:
        return
    src, dt, dr = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
    Rs, Cs, Rp = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
    for i, (x, row, t) in enumerate(items):
        _chk(x, "x")
        R, Cc = x.shape
        rpad = (R + 31) // 32 * 32
        if row is not None:
            _chk(row, "row", f16); assert row.shape == (R, 2 * Cc), (row.shape, x.shape)
        if t is not None:
            _chk(t, "t", f16); assert t.shape == (Cc, 2 * rpad), (t.shape, x.shape)
        src[i], dr[i], dt[i] = _p(x), _p(row), _p(t)
        Rs[i], Cs[i], Rp[i] = R, Cc, rpad
    _lib.check(lib.tt_split_pairs_dual_multi(src, dt, dr, Rs, Cs, Rp, n, _p(range_flag()), _stream()), "tt_split_pairs_dual_multi")


def transpose_pairs(xp, rpad: Optional[int] = None):
    """pairs [R, 2 C] -> transposed pairs [C, 2 Rpad] (zero beyond R)."""
    lib = _lib.load()
    _chk(xp, "xp", f16)
    R, C2 = xp.shape
    rpad = (R + 31) // 32 * 32 if rpad is None else rpad
    t = torch.empty((C2 // 2, 2 * rpad), dtype=f16, device=xp.device)
    _lib.check(lib.tt_transpose_pairs(_p(xp), _p(t), R, C2 // 2, rpad, _stream()), "tt_transpose_pairs")
    return t


def bwd_pairs_ok(M: int, N: int, K: int) -> bool:
    """Shapes the pair backward products take (dy [M,N], w [N,K])."""
    return N % 64 == 0 and K % 64 == 0


def bwd_weight_pairs_tn_ok(M: int, N: int, K: int) -> bool:
    """Shapes the transpose-free weight-gradient kernel takes (dy [M,N], x [M,K] in row pairs)."""
    return bool(TN_WGRAD) and bool(_lib.load().tt_linear_bwd_weight_pairs_tn_ok(N, K, M))


def linear_bwd_weight_pairs_tn(dy_pairs, x_pairs, dw_out=None, dy_scale=None, colsum_parts=None, db_out=None):
    """dw [N,K] = dy^T @ x from ROW pairs dy [M, 2 N], x [M, 2 K] (gemm_pairs_tn.hip: no transposed copies); ``dy_scale``: the device
    scalar a scaled split of dy returned.  ``colsum_parts`` (``split_pairs_dual(..., colsum_parts=True)``): the bias gradient is folded
    from them in the same launch as dw's split partials and returned too: (dw, db)."""
    lib = _lib.load()
    _chk(dy_pairs, "dy_pairs", f16); _chk(x_pairs, "x_pairs", f16)
    M, N, K = dy_pairs.shape[0], dy_pairs.shape[1] // 2, x_pairs.shape[1] // 2
    assert x_pairs.shape[0] == M, (dy_pairs.shape, x_pairs.shape)
    dw = _chk(dw_out, "dw_out") if dw_out is not None else torch.empty((N, K), dtype=f32, device=dy_pairs.device)
    nb = lib.tt_linear_bwd_weight_pairs_tn_workspace_bytes(N, K, M)
    ws = _ws(nb, dy_pairs.device)
    e0 = _prof_begin()
    if colsum_parts is not None:
        _chk(colsum_parts, "colsum_parts")
        assert colsum_parts.shape[1] == N, (colsum_parts.shape, N)
        db = _chk(db_out, "db_out") if db_out is not None else torch.empty((N,), dtype=f32, device=dy_pairs.device)
        _lib.check(lib.tt_linear_bwd_weight_pairs_tn_bias(_p(dy_pairs), _p(x_pairs), _p(dw), _p(dy_scale), N, K, M, _p(ws), nb, _p(colsum_parts),
                                                          colsum_parts.shape[0], _p(db), _stream()), "tt_linear_bwd_weight_pairs_tn_bias")
        _prof_end(e0, "PAIRS_TN", N, K, M)
        return dw, db
    _lib.check(lib.tt_linear_bwd_weight_pairs_tn(_p(dy_pairs), _p(x_pairs), _p(dw), _p(dy_scale), N, K, M, _p(ws), nb, _stream()), "tt_linear_bwd_weight_pairs_tn")
    _prof_end(e0, "PAIRS_TN", N, K, M)
    return dw


# Weight gradients on a side stream (round 6): ``wgrad_fork(stream)`` at the top of a backward, ``wgrad_join()`` before anything reads a
# gradient (the optimizer, a gradient bucket's all-reduce).  Between them ``linear_bwd_pairs`` launches its transpose-free weight-gradient
# product on ``stream`` behind the dy's split and carries on with the data gradient on the current stream.
_WGRAD = {"side": None, "keep": []}


def wgrad_fork(stream) -> None:
    _WGRAD["side"] = stream


def wgrad_side():
    """The armed weight-gradient side stream, or None."""
    return _WGRAD["side"] if PROFILE is None else None


def wgrad_join(final: bool = True) -> None:
    side = _WGRAD["side"]
    if side is not None:
        torch.cuda.current_stream().wait_stream(side)
        _WGRAD["keep"].clear()
        if final:
            _WGRAD["side"] = None


def wgrad_call(fn, keep=()):
    """``fn()`` on the weight-gradient side stream when one is armed (``wgrad_fork``), behind everything queued on the current stream so far;
    ``keep``: the tensors ``fn`` reads that the caller is about to drop (held until the join)."""
    side = _WGRAD["side"] if PROFILE is None else None
    if side is None:
        return fn()
    side.wait_stream(torch.cuda.current_stream())
    _WGRAD["keep"].append(keep)
    with torch.cuda.stream(side):
        return fn()


def linear_bwd_data_pairs_is_persistent(M: int, N: int, K: int) -> bool:
    """Would the data gradient dx [M, K] = dy [M, N] @ w of an nn.Linear(K -> N) run on the persistent pair kernel (plain fp32 epilogue)?"""
    return _lib.load().tt_linear_fwd_pairs_route(M, K, N, 0, 0, 0, 1, 0, 0) == 8


def linear_bwd_pairs(dy, wT_pairs, xT_pairs=None, gelu_pre=None, need_bias: bool = True, need_dx: bool = True, dw_out=None, db_out=None, x_pairs=None,
                     dy_amax=None, dx_amax_out=None):
    """(dx, dw, db) of an nn.Linear on pair operands: dy fp32 [M,N] is split here in ONE pass (row pairs for both gradient products, column
    sums = the bias gradient); wT_pairs [K, 2 N] = the weight transposed in pairs.  The layer's input comes as ``x_pairs`` [M, 2 K] (row
    pairs as the forward kept them: the transpose-free weight-gradient kernel) or, for the shapes that kernel does not take, as
    ``xT_pairs`` [K, 2 Mpad] (``transpose_pairs``; dy's transposed pairs are then made in the same pass).
    ``dy_amax``: max |dy| as the kernel that produced dy published it (``AmaxPool``; the scaled split then skips its max pass);
    ``dx_amax_out``: a zeroed slot the data-gradient kernel raises to max |dx| (dx = the next Linear's dy: the gelu' route)."""
    lib = _lib.load()
    _chk(dy, "dy"); _chk(wT_pairs, "wT_pairs", f16)
    M, N = dy.shape
    K = wT_pairs.shape[0]
    if x_pairs is not None and bwd_weight_pairs_tn_ok(M, N, K):
        _chk(x_pairs, "x_pairs", f16)
        assert wT_pairs.shape == (K, 2 * N) and x_pairs.shape == (M, 2 * K), (dy.shape, wT_pairs.shape, x_pairs.shape)
        # the bias gradient's fold rides on the weight gradient's (one launch less per Linear): the column partials stay unfolded here
        r4 = split_pairs_dual(dy, want_row=True, want_colsum=need_bias, want_t=False, scaled=GRAD_SCALE, colsum_parts=need_bias,
                              amax_in=dy_amax if (need_bias and GRAD_SCALE) else None)
        dy_row, parts, dy_scale = r4[1], r4[2], (r4[3] if GRAD_SCALE else None)
        # the weight gradient is a LEAF of the backward (nothing downstream reads it before the optimizer): with a side stream set
        # (``wgrad_fork``: engine.TWO_STREAMS) it runs there, beside the data-gradient chain that continues on this stream
        # (kept alive until the join: freed earlier, their blocks could be reused on THIS stream under the side stream's reads)
        if need_bias:
            dw, db = wgrad_call(lambda: linear_bwd_weight_pairs_tn(dy_row, x_pairs, dw_out, dy_scale, colsum_parts=parts, db_out=db_out),
                                keep=(dy_row, parts, dy_scale, x_pairs))
        else:
            dw, db = wgrad_call(lambda: linear_bwd_weight_pairs_tn(dy_row, x_pairs, dw_out, dy_scale), keep=(dy_row, dy_scale, x_pairs)), None
    else:
        if xT_pairs is None:
            xT_pairs = transpose_pairs(x_pairs)
        _chk(xT_pairs, "xT_pairs", f16)
        Mpad = xT_pairs.shape[1] // 2
        assert wT_pairs.shape == (K, 2 * N) and xT_pairs.shape[0] == K and Mpad >= M, (dy.shape, wT_pairs.shape, xT_pairs.shape)
        r4 = split_pairs_dual(dy, want_row=need_dx, want_colsum=need_bias, rpad=Mpad, colsum_out=db_out, scaled=GRAD_SCALE)
        dyT, dy_row, db, dy_scale = r4[0], r4[1], r4[2], (r4[3] if GRAD_SCALE else None)
        dw = _chk(dw_out, "dw_out") if dw_out is not None else torch.empty((N, K), dtype=f32, device=dy.device)
        nb = lib.tt_linear_bwd_weight_pairs_workspace_bytes(N, K, Mpad)
        ws = _ws(nb, dy.device)
        e0 = _prof_begin()
        _lib.check(lib.tt_linear_bwd_weight_pairs(_p(dyT), _p(xT_pairs), _p(dw), _p(dy_scale), N, K, Mpad, _p(ws), nb, _stream()), "tt_linear_bwd_weight_pairs")
        _prof_end(e0, "PAIRS", N, K, M)
    dx = None
    if need_dx:
        if gelu_pre is not None: _chk(gelu_pre, "gelu_pre")
        dx = torch.empty((M, K), dtype=f32, device=dy.device)
        # (label: the persistent kernel takes a data-gradient product under the shape rules of its fp32 (+ operand) epilogues)
        p8 = PROFILE is not None and lib.tt_linear_fwd_pairs_route(M, K, N, 0, 0, int(gelu_pre is not None), 1, 0, 0) == 8
        e0 = _prof_begin()
        kws = ksplit_workspace(dx.device)
        _lib.check(lib.tt_linear_bwd_data_pairs(_p(dy_row), _p(wT_pairs), _p(gelu_pre), _p(dx), _p(dy_scale), M, N, K, _p(kws), kws.numel(),
                                                _p(dx_amax_out), _stream()), "tt_linear_bwd_data_pairs")
        _prof_end(e0, "PAIRS8" if p8 else "PAIRS", M, K, N)
    return dx, dw, db


def attention_fwd_bf16(qkv, num_heads: int):
    """qkv [F,N,3*D] bf16 -> out [F,N,D] bf16 (N <= 256, head_dim 64)."""
    lib = _lib.load()
    _chk(qkv, "qkv", bf16)
    F, N, D3 = qkv.shape
    D = D3 // 3
    hd = D // num_heads
    out = torch.empty((F, N, D), dtype=bf16, device=qkv.device)
    _lib.check(lib.tt_attention_fwd_bf16(_p(qkv), _p(out), F, N, num_heads, hd, float(hd ** -0.5), _stream()), "tt_attention_fwd_bf16")
    return out


def transpose_planes(x, rpad: Optional[int] = None, colsum: bool = False):
    """fp32 [R, C] -> bf16 [1, C, Rpad] (transposed, zero-padded along R to a multiple of 64 by default).  ``colsum``: the same pass also
    returns x.sum(0) in fp32 (tt_transpose_planes_colsum) -> (planes, sums)."""
    lib = _lib.load()
    _chk(x, "x")
    R, Cc = x.shape
    rpad = (R + 63) // 64 * 64 if rpad is None else rpad
    y = torch.empty((1, Cc, rpad), dtype=bf16, device=x.device)
    if colsum:
        sums = torch.empty((Cc,), dtype=f32, device=x.device)
        nb = lib.tt_transpose_planes_colsum_workspace_bytes(R, Cc, rpad)
        ws = _ws(nb, x.device)
        _lib.check(lib.tt_transpose_planes_colsum(_p(x), _p(y), R, Cc, rpad, _p(sums), _p(ws), nb, _stream()), "tt_transpose_planes_colsum")
        return y, sums
    _lib.check(lib.tt_transpose_planes(_p(x), _p(y), R, Cc, rpad, _stream()), "tt_transpose_planes")
    return y


def bwd_planes_ok(M: int, N: int, K: int) -> bool:
    """Shapes the bf16 backward products take (dy [M,N], w [N,K]): whole 64-wide tiles along N and K."""
    return N % 64 == 0 and K % 64 == 0


def linear_bwd_data_planes(dy, w, gelu_pre=None):
    """dx = dy @ w (* gelu'(gelu_pre)) on bf16 operands: dy [M,N] and w [N,K] fp32 are converted here (dy rounded, w
    transposed), fp32 accumulate and output."""
    lib = _lib.load()
    _chk(dy, "dy"); _chk(w, "w")
    M, N = dy.shape
    K = w.shape[1]
    dyp = split_planes(dy, 1)
    wT = transpose_planes(w, N)                      # [1, K, N]
    dx = torch.empty((M, K), dtype=f32, device=dy.device)
    if gelu_pre is not None: _chk(gelu_pre, "gelu_pre")
    e0 = _prof_begin()
    kws = ksplit_workspace(dx.device)
    _lib.check(lib.tt_linear_bwd_data_planes(_p(dyp), M * N, _p(wT), K * N, 1, _p(gelu_pre), _p(dx), M, N, K, _p(kws), kws.numel(), _stream()),
               "tt_linear_bwd_data_planes")
    _prof_end(e0, "PLANES1", M, K, N)
    return dx


def linear_bwd_weight_planes(dy, x, need_bias=True):
    """dw = dy.T @ x on bf16 operands (both transposed + rounded here), db = dy.sum(0) in fp32."""
    lib = _lib.load()
    _chk(dy, "dy"); _chk(x, "x")
    M, N = dy.shape
    K = x.shape[1]
    # [1, N, Mpad], [1, K, Mpad]; the bias gradient dy.sum(0) comes out of dy's transposing pass
    dyT, db = transpose_planes(dy, colsum=True) if need_bias else (transpose_planes(dy), None)
    xT = transpose_planes(x)
    Mpad = dyT.shape[2]
    dw = torch.empty((N, K), dtype=f32, device=dy.device)
    nb = lib.tt_linear_bwd_weight_planes_workspace_bytes(N, K, Mpad)
    ws = _ws(nb, dy.device)
    e0 = _prof_begin()
    _lib.check(lib.tt_linear_bwd_weight_planes(_p(dyT), N * Mpad, _p(xT), K * Mpad, 1, _p(dw), N, K, Mpad, _p(ws), nb, _stream()),
               "tt_linear_bwd_weight_planes")
    _prof_end(e0, "PLANES1", N, K, Mpad)
    return dw, db


# ---- coarse entry points: one C call per reference function ------------------------------------------------

def fine_grained() -> bool:
    """True while a per-launch GEMM profile is being collected (bench.py's roofline leg): the launch sequences then go through
    the op-level entry points one ctypes call at a time - the same kernels in the same order as the coarse entry points
    enqueue - so that every GEMM launch can be bracketed by events."""
    return PROFILE is not None


def vit_forward(params, n_blocks: int, tokens, img=None, frame_map=None, normed_out=None, drop_cls: bool = False, last_qkv: bool = False,
                last_probs: bool = False):
    """``tt_vit_forward``: [prepare_tokens of ``img``] + ``n_blocks`` blocks in place on ``tokens`` [F,N,D] [+ final norm].
    ``params`` = (VitParams struct, keep-alive list) as ``engine.vit_params`` builds it.  Returns (normed or None, qkv of the
    last block or None, its attention probabilities or None)."""
    lib = _lib.load()
    vp, _keep = params
    _chk(tokens, "tokens")
    F, N, D = tokens.shape
    vp.n_blocks = int(n_blocks)
    planes_given = vp.planes   # (the caller's struct is restored below - a cached (vp, keep) must not stay in f32 for later launches)
    if vp.planes == 2 and F * N < PAIRS_MIN_ROWS:
        vp.planes = 0   # a small launch sequence keeps the exact-f32 kernels (PAIRS_MIN_ROWS); the fp32 weights are in the table anyway
    dev = tokens.device
    rf = range_flag(dev) if vp.planes == 2 else None
    vp.range_flag = _p(rf)
    vp.precision = precision_code()
    if img is not None:
        _chk(img, "img")
        C_, H, W = img.shape[1], img.shape[2], img.shape[3]
    else:
        # the token grid only matters through N: hand the entry point an H x W that yields it
        C_, H, W = 3, vp.patch, (N - 1) * vp.patch
    normed = None
    if normed_out is not None:
        normed = normed_out if isinstance(normed_out, torch.Tensor) else torch.empty((F * (N - 1), D) if drop_cls else (F, N, D), dtype=f32, device=dev)
        _chk(normed, "normed_out")
    qkv = torch.empty((F, N, 3 * D), dtype=f32, device=dev) if last_qkv else None
    probs = torch.empty((F, vp.heads, N, N), dtype=f32, device=dev) if last_probs else None
    nb = lib.tt_vit_forward_workspace_bytes(F, N, D, vp.hidden, vp.planes) if n_blocks else 0
    ws = _ws(nb, dev)
    try:
        _lib.check(lib.tt_vit_forward(vp, _p(img), _p(frame_map), F, C_, H, W, _p(tokens), _p(normed), int(bool(drop_cls)), _p(qkv), _p(probs),
                                      _p(ws), nb, _stream()), "tt_vit_forward")
    finally:
        vp.planes = planes_given
    return normed, qkv, probs


def mlp_head_forward(x, layers: Sequence[tuple]):
    """``tt_mlp_head_forward``: layers = [(weight [out,in], bias or None), ...], GELU between them."""
    lib = _lib.load()
    _chk(x, "x")
    M = x.shape[0]
    arr = (_lib.LinearParams * len(layers))()
    for i, (w, b) in enumerate(layers):
        _chk(w, "weight")
        if b is not None: _chk(b, "bias")
        arr[i] = _lib.LinearParams(w.data_ptr(), b.data_ptr() if b is not None else None, w.shape[0], w.shape[1])
    out = torch.empty((M, layers[-1][0].shape[0]), dtype=f32, device=x.device)
    nb = lib.tt_mlp_head_forward_workspace_bytes(M, arr, len(layers))
    ws = _ws(nb, x.device)
    _lib.check(lib.tt_mlp_head_forward(_p(x), M, arr, len(layers), _p(out), precision_code(), _p(ws), nb, _stream()), "tt_mlp_head_forward")
    return out


def scores_sinkhorn(z, prototypes, queue=None, iters: int = 10, eps: float = 0.05, rows_out: Optional[int] = None):
    """``tt_scores_sinkhorn``: (q [rows_out, K], scores [B + queue rows, K]) of TimeT.get_scores on one rank."""
    lib = _lib.load()
    _chk(z, "z"); _chk(prototypes, "prototypes")
    B, dim = z.shape
    K = prototypes.shape[0]
    Qr = 0
    if queue is not None:
        _chk(queue, "queue")
        Qr = queue.shape[0]
    rows_out = B if rows_out is None else rows_out
    scores = torch.empty((B + Qr, K), dtype=f32, device=z.device)
    q = torch.empty((rows_out, K), dtype=f32, device=z.device)
    nb = lib.tt_scores_sinkhorn_workspace_bytes(B, Qr, K, dim)
    ws = _ws(nb, z.device)
    _lib.check(lib.tt_scores_sinkhorn(_p(z), B, _p(queue), Qr, _p(prototypes), K, dim, _p(scores), _p(q), rows_out, float(eps), int(iters),
                                      precision_code(), _p(ws), nb, _stream()), "tt_scores_sinkhorn")
    return q, scores


def adamw_ema_step_(entries: Sequence[tuple], step: int, beta1=0.9, beta2=0.999, eps=1e-8, prototypes=None, teacher_flat=None,
                    student_flat=None, teacher_prototypes=None, momentum: float = 0.0):
    """``tt_adamw_ema_step``: AdamW over ``entries`` (as ``adamw_step_``), prototypes renormalised, then the EMA teacher update of
    the flat parameter buffers and the teacher prototypes (each part skipped when its tensors are None)."""
    _bump_param_epoch()
    lib = _lib.load()
    arr = (_lib.AdamwTensor * max(len(entries), 1))()
    for j, (p, g, m, v, lr, wd) in enumerate(entries):
        for t, nm in ((p, "param"), (g, "grad"), (m, "exp_avg"), (v, "exp_avg_sq")):
            _chk(t, nm)
        arr[j] = _lib.AdamwTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr), float(wd))
    K = dim = 0
    if prototypes is not None:
        _chk(prototypes, "prototypes")
        K, dim = prototypes.shape
    n_flat = 0
    if teacher_flat is not None:
        _chk(teacher_flat, "teacher_flat"); _chk(student_flat, "student_flat")
        assert teacher_flat.numel() == student_flat.numel()
        n_flat = teacher_flat.numel()
    if teacher_prototypes is not None:
        _chk(teacher_prototypes, "teacher_prototypes")
    _lib.check(lib.tt_adamw_ema_step(arr, len(entries), int(step), float(beta1), float(beta2), float(eps), _p(prototypes), K, dim,
                                     _p(teacher_flat) if n_flat else None, _p(student_flat) if n_flat else None, n_flat, _p(teacher_prototypes),
                                     float(momentum), _stream()), "tt_adamw_ema_step")


# ---- N5: linear-probe fine-tuning (linear_finetune.py; include/timetuning_hip.h "N5") ---------------------------------------------------

def probe_logits(feats, weight, bias=None):
    """feats [rows, D], weight [C, D] (the 1x1 conv weight viewed as a matrix), bias [C] -> logits [rows, C]."""
    lib = _lib.load()
    _chk(feats, "feats"); _chk(weight, "weight")
    if bias is not None:
        _chk(bias, "bias")
    rows, D = feats.shape
    Cc = weight.shape[0]
    if weight.shape[1] != D:
        raise ValueError(f"probe_logits: weight has {weight.shape[1]} input channels, feats has {D}")
    out = torch.empty((rows, Cc), dtype=f32, device=feats.device)
    _lib.check(lib.tt_probe_logits(_p(feats), _p(weight), _p(bias), _p(out), rows, D, Cc, _stream()), "tt_probe_logits")
    return out


def probe_upsample_ce(logits_low, labels):
    """logits_low [B, g*g, C], labels int64 [B, R, R] -> (loss [1] = mean CE(ignore_index=255) of the bilinear upsampling to R x R,
    dlogits_low [B, g*g, C], counts int64 [2] = (valid pixels, invalid labels)).  Nothing is synchronised: read counts[1] to find
    out whether a label was outside [0, C) and not 255 (such labels are only counted)."""
    lib = _lib.load()
    _chk(logits_low, "logits_low"); _chk(labels, "labels", torch.int64)
    B, n, Cc = logits_low.shape
    g = int(round(n ** 0.5))
    if g * g != n:
        raise ValueError(f"probe_upsample_ce: {n} tokens are not a square grid")
    if labels.dim() != 3 or labels.shape[0] != B or labels.shape[1] != labels.shape[2]:
        raise ValueError(f"probe_upsample_ce: labels must be [B, R, R], got {tuple(labels.shape)}")
    R = labels.shape[1]
    dev = logits_low.device
    loss = torch.empty((1,), dtype=f32, device=dev)
    counts = torch.empty((2,), dtype=torch.int64, device=dev)
    dlow = torch.empty_like(logits_low)
    nb = lib.tt_probe_upsample_ce_workspace_bytes(B, g)
    ws = _ws(nb, dev)
    _lib.check(lib.tt_probe_upsample_ce(_p(logits_low), _p(labels), _p(dlow), _p(loss), _p(counts), B, g, Cc, R, _p(ws), nb, _stream()),
               "tt_probe_upsample_ce")
    return loss, dlow, counts


def bilinear_adjoint_tokens(d_hi, g: int):
    """d_hi [B, R*R, C] -> d_low [B, g*g, C]: the adjoint (backward) of ``upsample_bilinear_tokens``."""
    lib = _lib.load()
    _chk(d_hi, "d_hi")
    B, m, Cc = d_hi.shape
    R = int(round(m ** 0.5))
    if R * R != m:
        raise ValueError(f"bilinear_adjoint_tokens: {m} pixels are not a square mask")
    out = torch.empty((B, g * g, Cc), dtype=f32, device=d_hi.device)
    _lib.check(lib.tt_bilinear_adjoint_tokens(_p(d_hi), _p(out), B, int(g), Cc, R, _stream()), "tt_bilinear_adjoint_tokens")
    return out


def probe_wgrad(dlogits, feats, scale=None, need_bias=True):
    """dlogits [rows, C], feats [rows, D] -> (dW [C, D] = dlogits^T feats, db [C] = colsum(dlogits) or None), both times the
    one-element device tensor ``scale`` if given."""
    lib = _lib.load()
    _chk(dlogits, "dlogits"); _chk(feats, "feats")
    if scale is not None:
        _chk(scale, "scale")
    rows, Cc = dlogits.shape
    if feats.shape[0] != rows:
        raise ValueError("probe_wgrad: dlogits and feats need the same number of rows")
    D = feats.shape[1]
    dev = feats.device
    dw = torch.empty((Cc, D), dtype=f32, device=dev)
    db = torch.empty((Cc,), dtype=f32, device=dev) if need_bias else None
    nb = lib.tt_probe_wgrad_workspace_bytes(rows, D, Cc)
    ws = _ws(nb, dev)
    _lib.check(lib.tt_probe_wgrad(_p(dlogits), _p(feats), _p(scale), _p(dw), _p(db), rows, D, Cc, _p(ws), nb, _stream()), "tt_probe_wgrad")
    return dw, db


def sgd_step_(entries: Sequence[tuple], momentum: float = 0.0, first_step: bool = False):
    """torch.optim.SGD (dampening 0, no Nesterov) over (param, grad, momentum_buffer or None, lr, weight_decay) tuples, fp32 GPU
    contiguous; ``first_step``: the buffers are (re)initialised to the step direction, as SGD does for a tensor's first step."""
    _bump_param_epoch()
    lib = _lib.load()
    cap = 40
    for i in range(0, len(entries), cap):
        chunk = entries[i:i + cap]
        arr = (_lib.AdamwTensor * len(chunk))()
        for j, (p, g, buf, lr, wd) in enumerate(chunk):
            _chk(p, "param"); _chk(g, "grad")
            if buf is not None:
                _chk(buf, "momentum_buffer")
            if g.numel() != p.numel() or (buf is not None and buf.numel() != p.numel()):
                raise ValueError("sgd_step_: param, grad and momentum buffer need the same size")
            arr[j] = _lib.AdamwTensor(p.data_ptr(), g.data_ptr(), _p(buf), None, p.numel(), float(lr), float(wd))
        _lib.check(lib.tt_sgd_step(arr, len(chunk), float(momentum), int(bool(first_step)), _stream()), "tt_sgd_step")


# ---- N32: FCN-head fine-tuning (leopart.py:83-147; include/timetuning_hip.h "N32") -------------------------------------------------------

def _conv_sources(who: str, xa, xb, grid):
    _chk(xa, "xa")
    if xa.dim() != 3:
        raise ValueError(f"{who}: xa must be [B, gh*gw, Ca], got {tuple(xa.shape)}")
    B, n, Ca = xa.shape
    gh, gw = _grid(grid, n, who)
    Cb = 0
    if xb is not None:
        _chk(xb, "xb")
        if xb.dim() != 3 or xb.shape[:2] != xa.shape[:2]:
            raise ValueError(f"{who}: xb must be [B, gh*gw, Cb] on xa's tokens, got {tuple(xb.shape)}")
        Cb = xb.shape[2]
    return B, gh, gw, Ca, Cb


def _conv_weight(who: str, weight, Cin=None):
    _chk(weight, "weight")
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or (Cin is not None and weight.shape[1] != Cin):
        raise ValueError(f"{who}: weight must be [Cout, {'Cin' if Cin is None else Cin}, 3, 3], got {tuple(weight.shape)}")
    return weight.shape[0], weight.shape[1]


def conv3x3_tokens(xa, weight, bias=None, xb=None, grid=None, act: int = 0, out_scale=None):
    """3x3 convolution, zero padding, over token-major features: xa [B, gh*gw, Ca] (and xb [B, gh*gw, Cb], the further input channels of
    a concatenation that is never stored), weight [Cout, Ca + Cb, 3, 3] (nn.Conv2d's), bias [Cout] -> y [B, gh*gw, Cout] =
    act(bias + conv) * out_scale[b, co]; act 0 / 1 (ReLU), out_scale [B, Cout] (Dropout2d as a multiplier)."""
    lib = _lib.load()
    who = "conv3x3_tokens"
    B, gh, gw, Ca, Cb = _conv_sources(who, xa, xb, grid)
    Cout, _ = _conv_weight(who, weight, Ca + Cb)
    if bias is not None:
        _chk(bias, "bias")
        if bias.shape != (Cout,):
            raise ValueError(f"{who}: bias must be [{Cout}], got {tuple(bias.shape)}")
    if out_scale is not None:
        _chk(out_scale, "out_scale")
        if out_scale.shape != (B, Cout):
            raise ValueError(f"{who}: out_scale must be [{B}, {Cout}], got {tuple(out_scale.shape)}")
    y = torch.empty((B, gh * gw, Cout), dtype=f32, device=xa.device)
    nb = lib.tt_conv3x3_tokens_fwd_workspace_bytes(Ca, Cb, Cout)
    ws = _ws(nb, xa.device)
    _lib.check(lib.tt_conv3x3_tokens_fwd(_p(xa), _p(xb), _p(weight), _p(bias), _p(out_scale), _p(y), B, gh, gw, Ca, Cb, Cout, int(act), _p(ws), nb,
                                         _stream()), "tt_conv3x3_tokens_fwd")
    return y


def conv3x3_tokens_bwd_data(dpre, weight, grid, c_begin: int = 0, c_count: Optional[int] = None, gate=None):
    """dpre [B, gh*gw, Cout] (the gradient of the pre-activation), weight [Cout, Cin, 3, 3] -> dx [B, gh*gw, c_count]: the gradient with
    respect to input channels c_begin .. c_begin + c_count - 1 (default: all), zeroed where gate [B, gh*gw, c_count] <= 0."""
    lib = _lib.load()
    who = "conv3x3_tokens_bwd_data"
    B, gh, gw, Cout, _ = _conv_sources(who, dpre, None, grid)
    wo, Cin = _conv_weight(who, weight)
    if wo != Cout:
        raise ValueError(f"{who}: weight has {wo} output channels, dpre has {Cout}")
    c_count = Cin - int(c_begin) if c_count is None else int(c_count)
    if gate is not None:
        _chk(gate, "gate")
        if gate.numel() != B * gh * gw * c_count:
            raise ValueError(f"{who}: gate must be [{B}, {gh * gw}, {c_count}], got {tuple(gate.shape)}")
    dx = torch.empty((B, gh * gw, max(c_count, 0)), dtype=f32, device=dpre.device)
    nb = lib.tt_conv3x3_tokens_bwd_data_workspace_bytes(Cout, c_count)
    ws = _ws(nb, dpre.device)
    _lib.check(lib.tt_conv3x3_tokens_bwd_data(_p(dpre), _p(weight), _p(gate), _p(dx), B, gh, gw, Cin, Cout, int(c_begin), c_count, _p(ws), nb,
                                              _stream()), "tt_conv3x3_tokens_bwd_data")
    return dx


def conv3x3_tokens_bwd_weight(dpre, xa, xb=None, grid=None, scale=None, need_bias: bool = True):
    """dpre [B, gh*gw, Cout], the sources of ``conv3x3_tokens`` -> (dw [Cout, Ca + Cb, 3, 3], db [Cout] or None), both times the
    one-element device tensor ``scale`` if given."""
    lib = _lib.load()
    who = "conv3x3_tokens_bwd_weight"
    B, gh, gw, Ca, Cb = _conv_sources(who, xa, xb, grid)
    _chk(dpre, "dpre")
    if dpre.dim() != 3 or dpre.shape[:2] != xa.shape[:2]:
        raise ValueError(f"{who}: dpre must be [B, gh*gw, Cout] on xa's tokens, got {tuple(dpre.shape)}")
    if scale is not None:
        _chk(scale, "scale")
    Cout = dpre.shape[2]
    dev = xa.device
    dw = torch.empty((Cout, Ca + Cb, 3, 3), dtype=f32, device=dev)
    db = torch.empty((Cout,), dtype=f32, device=dev) if need_bias else None
    nb = lib.tt_conv3x3_tokens_bwd_weight_workspace_bytes(B * gh * gw, Ca + Cb, Cout)
    ws = _ws(nb, dev)
    _lib.check(lib.tt_conv3x3_tokens_bwd_weight(_p(dpre), _p(xa), _p(xb), _p(scale), _p(dw), _p(db), B, gh, gw, Ca, Cb, Cout, _p(ws), nb, _stream()),
               "tt_conv3x3_tokens_bwd_weight")
    return dw, db


def fcn_head_grad(dlogits, wseg, grid, out_scale=None, y=None):
    """dlogits [B, gh*gw, C], wseg [C, channels] (conv_seg's weight as a matrix) -> dpre [B, gh*gw, channels] =
    (dlogits wseg) * out_scale[b, c] * [y > 0]: the gradient entering the convolution whose output is y."""
    lib = _lib.load()
    who = "fcn_head_grad"
    B, gh, gw, Cc, _ = _conv_sources(who, dlogits, None, grid)
    _chk(wseg, "wseg")
    if wseg.dim() != 2 or wseg.shape[0] != Cc:
        raise ValueError(f"{who}: wseg must be [{Cc}, channels], got {tuple(wseg.shape)}")
    ch = wseg.shape[1]
    if out_scale is not None:
        _chk(out_scale, "out_scale")
        if out_scale.shape != (B, ch):
            raise ValueError(f"{who}: out_scale must be [{B}, {ch}], got {tuple(out_scale.shape)}")
    if y is not None:
        _chk(y, "y")
        if y.numel() != B * gh * gw * ch:
            raise ValueError(f"{who}: y must be [{B}, {gh * gw}, {ch}], got {tuple(y.shape)}")
    dpre = torch.empty((B, gh * gw, ch), dtype=f32, device=dlogits.device)
    _lib.check(lib.tt_fcn_head_grad(_p(dlogits), _p(wseg), _p(out_scale), _p(y), _p(dpre), B, gh, gw, Cc, ch, _stream()), "tt_fcn_head_grad")
    return dpre


# ---- N33: batch normalisation of the FCN head's ConvModules (leopart.py norm_cfg; include/timetuning_hip.h "N33") ---------------------------

def _bn_rows(who: str, z):
    _chk(z, "z")
    if z.dim() not in (2, 3):
        raise ValueError(f"{who}: z must be [B, gh*gw, C] or [rows, C], got {tuple(z.shape)}")
    C = z.shape[-1]
    rows = z.numel() // max(C, 1)
    npix = z.shape[1] if z.dim() == 3 else rows
    return rows, npix, C


def _bn_vector(who: str, t, name: str, C: int):
    _chk(t, name)
    if t.shape != (C,):
        raise ValueError(f"{who}: {name} must be [{C}], got {tuple(t.shape)}")
    return t


def bn_tokens(z, gamma, beta, running_mean, running_var, *, training: bool, momentum: float = 0.1, eps: float = 1e-5, act: int = 1,
              out_scale=None):
    """nn.BatchNorm2d over token-major z [B, gh*gw, C] (or [rows, C]), then ReLU (``act`` 1) and the Dropout2d multipliers out_scale
    [B, C] -> (y, save_mean [C], save_rstd [C]).  ``training``: batch statistics, and running_mean / running_var (None: none kept) are
    updated in place as nn.BatchNorm2d does; otherwise the running statistics normalise, nothing else is written and the two saved
    vectors are None."""
    lib = _lib.load()
    who = "bn_tokens"
    rows, npix, C = _bn_rows(who, z)
    training = bool(training)
    _bn_vector(who, gamma, "gamma", C)
    _bn_vector(who, beta, "beta", C)
    if (running_mean is None) != (running_var is None) or (running_mean is None and not training):
        raise ValueError(f"{who}: running_mean and running_var go together, and eval mode needs them")
    if running_mean is not None:
        _bn_vector(who, running_mean, "running_mean", C)
        _bn_vector(who, running_var, "running_var", C)
    if not lib.tt_bn_tokens_shape_ok(rows, C, int(training)):
        raise ValueError(f"{who}: {rows} rows of {C} channels are not supported (need C % 4 == 0, 0 < C <= 1024, 0 < rows < 2^31 and, "
                         f"in training, rows >= 2)")
    if out_scale is not None:
        _chk(out_scale, "out_scale")
        if z.dim() != 3 or out_scale.shape != (z.shape[0], C):
            raise ValueError(f"{who}: out_scale must be [B, {C}] beside z [B, gh*gw, {C}], got {tuple(out_scale.shape)}")
    if not float(eps) > 0.0 or not 0.0 <= float(momentum) <= 1.0 or act not in (0, 1):
        raise ValueError(f"{who}: need eps > 0, 0 <= momentum <= 1 and act 0 or 1 (got {eps}, {momentum}, {act})")
    y = torch.empty_like(z)
    mean = torch.empty((C,), dtype=f32, device=z.device) if training else None
    rstd = torch.empty((C,), dtype=f32, device=z.device) if training else None
    nb = lib.tt_bn_tokens_fwd_workspace_bytes(rows, C) if training else 0
    ws = _ws(nb, z.device) if training else None
    _lib.check(lib.tt_bn_tokens_fwd(_p(z), _p(gamma), _p(beta), _p(out_scale), _p(running_mean), _p(running_var), _p(y), _p(mean), _p(rstd),
                                    rows, npix, C, int(training), int(act), float(momentum), float(eps), _p(ws), nb, _stream()),
               "tt_bn_tokens_fwd")
    return y, mean, rstd


def bn_tokens_bwd(g, z, save_mean, save_rstd, gamma):
    """g (the gradient with respect to ``bn_tokens``' output before ReLU and out_scale: already gated and scaled by its producer), z and
    the saved statistics -> (dz, dgamma [C], dbeta [C]); dz is the ``dpre`` of the convolution that produced z."""
    lib = _lib.load()
    who = "bn_tokens_bwd"
    rows, _, C = _bn_rows(who, z)
    _chk(g, "g")
    if g.shape != z.shape:
        raise ValueError(f"{who}: g must have z's shape {tuple(z.shape)}, got {tuple(g.shape)}")
    _bn_vector(who, save_mean, "save_mean", C)
    _bn_vector(who, save_rstd, "save_rstd", C)
    _bn_vector(who, gamma, "gamma", C)
    if not lib.tt_bn_tokens_shape_ok(rows, C, 1):
        raise ValueError(f"{who}: {rows} rows of {C} channels are not supported (need C % 4 == 0, 0 < C <= 1024, 2 <= rows < 2^31)")
    dz = torch.empty_like(z)
    dgamma = torch.empty((C,), dtype=f32, device=z.device)
    dbeta = torch.empty((C,), dtype=f32, device=z.device)
    nb = lib.tt_bn_tokens_bwd_workspace_bytes(rows, C)
    ws = _ws(nb, z.device)
    _lib.check(lib.tt_bn_tokens_bwd(_p(g), _p(z), _p(save_mean), _p(save_rstd), _p(gamma), _p(dz), _p(dgamma), _p(dbeta), rows, C, _p(ws), nb,
                                    _stream()), "tt_bn_tokens_bwd")
    return dz, dgamma, dbeta


# ---- N6: cluster-based foreground extraction (cluster_based_foreground_extraction.py; include/timetuning_hip.h "N6") ------------------

class ClusterRangeError(_lib.HipLibraryError):
    """A cluster id outside [0, k) reached one of the N6 kernels."""


def _raise_cluster_range(flag, what: str, k: int) -> None:
    if int(flag.item()):
        raise ClusterRangeError(f"{what}: a cluster id lies outside [0, {k})")


def cbfe_cluster_stats(clusters, attn, gt, k: int, ignore: int = -1, check: bool = True, range_flag=None):
    """clusters, attn (or None), gt (or None): int64 [M, P] -> (stats int32 [M, k, 3] = {n, tp_attn, tp_gt}, gt_fg int32 [M]).  GT foreground is
    ``gt != 0`` (``ignore < 0``) or ``gt != 0 and gt != ignore``.  An id outside [0, k) raises ClusterRangeError when ``check`` (a
    synchronisation); with ``check=False`` the caller's ``range_flag`` (device int32, zeroed) receives it instead."""
    lib = _lib.load()
    _chk(clusters, "clusters", torch.int64)
    for name, t in (("gt", gt), ("attn", attn)):
        if t is not None:
            _chk(t, name, torch.int64)
    M = clusters.shape[0]
    P = clusters.numel() // max(M, 1)
    for name, t in (("gt", gt), ("attn", attn)):
        if t is not None and (t.shape[0] != M or t.numel() != clusters.numel()):
            raise ValueError(f"cbfe_cluster_stats: {name} must have the shape of clusters")
    dev = clusters.device
    stats = torch.empty((M, k, 3), dtype=torch.int32, device=dev)
    gt_fg = torch.empty((M,), dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev) if range_flag is None else _chk(range_flag, "range_flag", torch.int32)
    _lib.check(lib.tt_cbfe_cluster_stats(_p(clusters), _p(attn), _p(gt), _p(stats), _p(gt_fg), int(M), int(P), int(k), int(ignore), _p(flag),
                                         _stream()), "tt_cbfe_cluster_stats")
    if check:
        _raise_cluster_range(flag, "tt_cbfe_cluster_stats", k)
    return stats, gt_fg


def cbfe_cluster_precs(stats):
    """stats int32 [M, k, 3] -> (precs fp64 [k], occurrences int32 [k]): get_cluster_precs' averages, bit for bit."""
    lib = _lib.load()
    _chk(stats, "stats", torch.int32)
    M, k, _ = stats.shape
    precs = torch.empty((k,), dtype=torch.float64, device=stats.device)
    occ = torch.empty((k,), dtype=torch.int32, device=stats.device)
    _lib.check(lib.tt_cbfe_cluster_precs(_p(stats), _p(precs), _p(occ), int(M), int(k), _stream()), "tt_cbfe_cluster_precs")
    return precs, occ


def cbfe_cut_jaccard(stats, gt_fg, order, starts, return_iou: bool = False):
    """stats [M, k, 3], gt_fg [M], order int32 [k] (cluster ids, ascending precision), starts int32 [C] -> jac fp32 [C] (and the per-image
    IoU fp32 [C, M]): candidate c marks order[starts[c]:] as foreground; eval_jac's fp32 mean over the images, in image order."""
    lib = _lib.load()
    _chk(stats, "stats", torch.int32); _chk(gt_fg, "gt_fg", torch.int32); _chk(order, "order", torch.int32); _chk(starts, "starts", torch.int32)
    M, k, _ = stats.shape
    if order.numel() != k or gt_fg.numel() != M:
        raise ValueError("cbfe_cut_jaccard: order needs k entries and gt_fg M entries")
    Cn = starts.numel()
    dev = stats.device
    jac = torch.empty((Cn,), dtype=f32, device=dev)
    iou = torch.empty((Cn, M), dtype=f32, device=dev) if return_iou else None
    nb = lib.tt_cbfe_cut_jaccard_workspace_bytes(M, Cn)
    ws = _ws(nb, dev)
    _lib.check(lib.tt_cbfe_cut_jaccard(_p(stats), _p(gt_fg), _p(order), _p(starts), _p(jac), _p(iou), int(M), int(k), int(Cn), _p(ws), nb,
                                       _stream()), "tt_cbfe_cut_jaccard")
    return (jac, iou) if return_iou else jac


def cbfe_apply_fg(clusters, fg_table, check: bool = True):
    """clusters int64 (any shape), fg_table uint8 [k] -> mask int64 of the same shape (1 where the cluster is foreground)."""
    lib = _lib.load()
    _chk(clusters, "clusters", torch.int64); _chk(fg_table, "fg_table", torch.uint8)
    k = fg_table.numel()
    out = torch.empty_like(clusters)
    flag = torch.zeros(1, dtype=torch.int32, device=clusters.device)
    _lib.check(lib.tt_cbfe_apply_fg(_p(clusters), _p(fg_table), _p(out), clusters.numel(), int(k), _p(flag), _stream()), "tt_cbfe_apply_fg")
    if check:
        _raise_cluster_range(flag, "tt_cbfe_apply_fg", k)
    return out


def nearest_upsample_labels(tok, iy, ix):
    """tok int32 [M, g*g], iy / ix int32 [R] (entries in [0, g): the tables of ``nearest_index_table``) -> int64 [M, R*R]."""
    lib = _lib.load()
    _chk(tok, "tok", torch.int32); _chk(iy, "iy", torch.int32); _chk(ix, "ix", torch.int32)
    M, n = tok.shape
    g = int(round(n ** 0.5))
    if g * g != n:
        raise ValueError(f"nearest_upsample_labels: {n} tokens are not a square grid")
    R = iy.numel()
    if ix.numel() != R:
        raise ValueError("nearest_upsample_labels: iy and ix need the same length")
    out = torch.empty((M, R * R), dtype=torch.int64, device=tok.device)
    _lib.check(lib.tt_nearest_upsample_labels(_p(tok), _p(iy), _p(ix), _p(out), int(M), g, int(R), _stream()), "tt_nearest_upsample_labels")
    return out


# ---- N7: DAVIS J&F counts ----------------------------------------------------------------------------------------------

DAVIS_MAX_ELEMENT = 127   # rows and columns of the structuring element tt_davis_jf_counts accepts
_DAVIS_DTYPES = {torch.uint8: 0, torch.int64: 1}


def davis_element_spans(element):
    """A 2-D 0 / 1 structuring element -> (spans [(first, last set column)] per row ((1, 0) for an empty row), its (rows, cols),
    the anchor (rows // 2, cols // 2): cv2's default).  The set pixels of each row must be contiguous, as a disk's are."""
    el = torch.as_tensor(element).cpu().numpy() != 0
    if el.ndim != 2 or el.shape[0] < 1 or el.shape[1] < 1:
        raise ValueError(f"davis: the structuring element must be a non-empty 2-D array, got shape {el.shape}")
    spans = []
    for row in el:
        idx = row.nonzero()[0]
        if idx.size and idx[-1] - idx[0] + 1 != idx.size:
            raise ValueError("davis: every row of the structuring element must be one contiguous run")
        spans.append((int(idx[0]), int(idx[-1])) if idx.size else (1, 0))
    return spans, el.shape, (el.shape[0] // 2, el.shape[1] // 2)


def davis_jf_counts(pred, gt, num_objects: int, element, void=None):
    """pred, gt: label maps [T, H, W] (uint8 or int64, independently), void: uint8 [T, H, W] (non-zero = void) or None; objects
    1..num_objects; element: the 2-D 0 / 1 structuring element of the dilation (at most DAVIS_MAX_ELEMENT rows and columns) ->
    int64 [O, T, 6] = {J intersection, J union, n_fg, n_gt, fg_match, gt_match}."""
    lib = _lib.load()
    for name, t in (("pred", pred), ("gt", gt)):
        if t.dtype not in _DAVIS_DTYPES:
            raise TypeError(f"{name}: expected torch.uint8 or torch.int64, got {t.dtype}")
        _chk(t, name, t.dtype)
        if t.dim() != 3:
            raise ValueError(f"davis_jf_counts: {name} must be [T, H, W], got {tuple(t.shape)}")
    if gt.shape != pred.shape:
        raise ValueError(f"davis_jf_counts: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ")
    if void is not None:
        _chk(void, "void", torch.uint8)
        if void.shape != pred.shape:
            raise ValueError(f"davis_jf_counts: void {tuple(void.shape)} and pred {tuple(pred.shape)} differ")
    if int(num_objects) < 1:
        raise ValueError(f"davis_jf_counts: num_objects must be >= 1, got {num_objects}")
    T, H, W = pred.shape
    O = int(num_objects)
    spans, (rows, cols), (ay, ax) = davis_element_spans(element)
    flat = [v for sp in spans for v in sp]
    counts = torch.empty((O, T, 6), dtype=torch.int64, device=pred.device)
    _lib.check(lib.tt_davis_jf_counts(_p(pred), _DAVIS_DTYPES[pred.dtype], _p(gt), _DAVIS_DTYPES[gt.dtype], _p(void), _p(counts), T, H, W, O,
                                      (C.c_int * len(flat))(*flat), rows, cols, ay, ax, _stream()),
               "tt_davis_jf_counts")
    return counts


def davis_seg2bmap(seg):
    """seg uint8 [T, H, W] (non-zero = set) -> uint8 [T, H, W] boundary map (``_seg2bmap`` per frame)."""
    lib = _lib.load()
    _chk(seg, "seg", torch.uint8)
    if seg.dim() != 3:
        raise ValueError(f"davis_seg2bmap: seg must be [T, H, W], got {tuple(seg.shape)}")
    T, H, W = seg.shape
    out = torch.empty_like(seg)
    _lib.check(lib.tt_davis_seg2bmap(_p(seg), _p(out), T, H, W, _stream()), "tt_davis_seg2bmap")
    return out


# ---- N8: boundary F1 (bfscore) counts ----------------------------------------------------------------------------------

BF_MAX_RADIUS = 63   # element radius tt_bf_counts accepts: t <= 64


def bf_element_spans(threshold):
    """The element of calc_precision_recall's test ``d < threshold * threshold`` (d an integer squared distance, the bound a Python
    float, as the reference evaluates it) -> (spans [(first, last set column)] per row, (1, 0) for an empty row; radius r), columns
    0..2r with the centre at r.  Raises ValueError beyond BF_MAX_RADIUS."""
    tt = float(threshold) * float(threshold)
    r = 0
    while (r + 1) * (r + 1) < tt:
        r += 1
        if r > BF_MAX_RADIUS:
            raise ValueError(f"bf_counts: threshold {threshold} needs an element of radius > {BF_MAX_RADIUS} (t <= 64 is supported)")
    spans = []
    for dy in range(-r, r + 1):
        w = -1
        while (w + 1) * (w + 1) + dy * dy < tt:
            w += 1
        spans.append((r - w, r + w) if w >= 0 else (1, 0))
    return spans, r


def bf_counts(gt, pr, threshold):
    """gt, pr: binary maps uint8 [P, H, W] (non-zero = set) on the GPU; threshold: calc_precision_recall's t (|t| <= 64) ->
    int64 [P, 4] = {n_pr, hit_pr, n_gt, hit_gt}: contour points with multiplicity and those within the threshold of the other map's
    contour (include/timetuning_hip.h, N8)."""
    lib = _lib.load()
    _chk(gt, "gt", torch.uint8)
    _chk(pr, "pr", torch.uint8)
    if gt.dim() != 3 or gt.shape != pr.shape:
        raise ValueError(f"bf_counts: gt {tuple(gt.shape)} and pr {tuple(pr.shape)} must be the same [P, H, W]")
    P, H, W = gt.shape
    spans, r = bf_element_spans(threshold)
    flat = [v for sp in spans for v in sp]
    counts = torch.empty((P, 4), dtype=torch.int64, device=gt.device)
    if P == 0:
        return counts
    _lib.check(lib.tt_bf_counts(_p(gt), _p(pr), _p(counts), int(P), int(H), int(W), (C.c_int * len(flat))(*flat), 2 * r + 1, _stream()),
               "tt_bf_counts")
    return counts


# ---- N10: the optical-flow baseline of the evaluation (dense Farneback flow, nearest label remap; farneback.hip) -----------------------

OPTFLOW_USE_INITIAL_FLOW = 4
OPTFLOW_FARNEBACK_GAUSSIAN = 256
FARNEBACK_MAX_WINSIZE = 127
FARNEBACK_MAX_LEVELS = 64


def check_farneback_params(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags) -> None:
    """The parameters tt_farneback_flow takes: flags 0, poly_n 5 or 7, 0 < pyr_scale < 1, ints levels in [1, 64], winsize in [1, 127],
    iterations >= 1, poly_sigma > 0.  The two flag bits raise NotImplementedError, anything else ValueError."""
    import math

    if not isinstance(flags, int) or isinstance(flags, bool):
        raise ValueError(f"flags {flags!r}: expected an int")
    if flags & (OPTFLOW_USE_INITIAL_FLOW | OPTFLOW_FARNEBACK_GAUSSIAN):
        raise NotImplementedError("OPTFLOW_USE_INITIAL_FLOW and OPTFLOW_FARNEBACK_GAUSSIAN are not part of this build (flags 0 only)")
    if flags != 0:
        raise ValueError(f"flags {flags}: only 0 is supported")
    for name, v, hi in (("levels", levels, FARNEBACK_MAX_LEVELS), ("winsize", winsize, FARNEBACK_MAX_WINSIZE), ("iterations", iterations, 1 << 16)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= hi:
            raise ValueError(f"{name} {v!r}: expected an int in [1, {hi}]")
    if isinstance(poly_n, bool) or poly_n not in (5, 7):
        raise ValueError(f"poly_n {poly_n!r}: expected 5 or 7")
    if isinstance(pyr_scale, bool) or not isinstance(pyr_scale, (int, float)) or not 0.0 < float(pyr_scale) < 1.0:
        raise ValueError(f"pyr_scale {pyr_scale!r}: expected 0 < pyr_scale < 1")
    if isinstance(poly_sigma, bool) or not isinstance(poly_sigma, (int, float)) or not (math.isfinite(poly_sigma) and poly_sigma > 0):
        raise ValueError(f"poly_sigma {poly_sigma!r}: expected a positive number")


def farneback_plan(H: int, W: int, pyr_scale: float = 0.5, levels: int = 3):
    """(effective levels L, [(h_k, w_k) for k = 0..L]) of calcOpticalFlowFarneback's pyramid (host only, no GPU)."""
    lib = _lib.load()
    L = C.c_int(0)
    sizes = (C.c_int * (2 * (int(levels) + 1)))()
    _lib.check(lib.tt_farneback_plan(int(H), int(W), float(pyr_scale), int(levels), C.byref(L), sizes), "tt_farneback_plan")
    return L.value, [(sizes[2 * k], sizes[2 * k + 1]) for k in range(L.value + 1)]


def flow_gray_u8(clip):
    """clip [F, 3, H, W] fp32 RGB on the GPU -> uint8 [F, H, W]: the reference's ``datum *= 255``, uint8 cast and RGB2BGR + BGR2GRAY."""
    lib = _lib.load()
    _chk(clip, "clip")
    if clip.dim() != 4 or clip.shape[1] != 3:
        raise ValueError(f"flow_gray_u8: clip {tuple(clip.shape)} is not [F, 3, H, W]")
    F, _, H, W = clip.shape
    out = torch.empty((F, H, W), dtype=torch.uint8, device=clip.device)
    _lib.check(lib.tt_flow_gray_u8(_p(clip), _p(out), F, H, W, _stream()), "tt_flow_gray_u8")
    return out


def farneback_flow(frames, pairs, pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2, flags=0, workspace=None):
    """frames uint8 [F, H, W] on the GPU, pairs [(prev, next), ...] (host) -> flow [P, H, W, 2] fp32 of
    cv2.calcOpticalFlowFarneback(frames[prev], frames[next], None, ...) for every pair, one launch per stage and level; each frame's
    pyramid and expansion is computed once.  ``workspace``: an optional uint8 GPU buffer of at least tt_farneback_workspace_bytes
    (allocated per call otherwise)."""
    check_farneback_params(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
    lib = _lib.load()
    _chk(frames, "frames", torch.uint8)
    if frames.dim() != 3 or frames.shape[0] < 1:
        raise ValueError(f"farneback_flow: frames {tuple(frames.shape)} is not [F >= 1, H, W]")
    F, H, W = frames.shape
    pr = [(int(a), int(b)) for a, b in pairs]
    for a, b in pr:
        if not (0 <= a < F and 0 <= b < F):
            raise ValueError(f"farneback_flow: pair ({a}, {b}) outside the {F} frames")
    P = len(pr)
    flow = torch.empty((P, H, W, 2), dtype=f32, device=frames.device)
    if P == 0:
        return flow
    pt = torch.tensor(pr, dtype=torch.int32).to(frames.device, non_blocking=False)
    nb = lib.tt_farneback_workspace_bytes(F, P, H, W, float(pyr_scale), int(levels))
    if nb == 0:
        raise ValueError(f"farneback_flow: no workspace for F {F}, P {P}, {H} x {W}")
    ws = _ws(nb, frames.device) if workspace is None else _chk(workspace, "workspace", torch.uint8)
    if ws.numel() < nb:
        raise ValueError(f"farneback_flow: workspace of {ws.numel()} bytes < {nb}")
    _lib.check(lib.tt_farneback_flow(_p(frames), F, H, W, _p(pt), P, float(pyr_scale), int(levels), int(winsize), int(iterations), int(poly_n),
                                     float(poly_sigma), int(flags), _p(flow), _p(ws), ws.numel(), _stream()), "tt_farneback_flow")
    return flow


def remap_nearest_labels(first, flows, scale: float = 1.0):
    """first [N, H, W] labels (uint8 or int64), flows [N, steps, H, W, 2] fp32, both on the GPU -> [N, steps, H, W] of the same dtype:
    step s remaps step s - 1 (step 0 remaps ``first``) through coords + scale * flows[:, s] with cv2.remap(INTER_NEAREST), constant-0
    border.  ``scale`` is rounded to fp32 as numpy rounds a Python float multiplying a float32 array."""
    lib = _lib.load()
    if first.dtype not in (torch.uint8, torch.int64):
        raise TypeError(f"remap_nearest_labels: labels must be uint8 or int64, got {first.dtype}")
    _chk(first, "first", first.dtype)
    _chk(flows, "flows")
    if first.dim() != 3 or flows.dim() != 5 or flows.shape[0] != first.shape[0] or tuple(flows.shape[2:]) != (*first.shape[1:], 2):
        raise ValueError(f"remap_nearest_labels: first {tuple(first.shape)} and flows {tuple(flows.shape)} are not [N, H, W] and "
                         "[N, steps, H, W, 2]")
    N, H, W = first.shape
    steps = flows.shape[1]
    out = torch.empty((N, steps, H, W), dtype=first.dtype, device=first.device)
    if H == 0 or W == 0:
        return out
    _lib.check(lib.tt_remap_nearest_labels(_p(first), _p(flows), _p(out), N, steps, H, W, float(scale), first.element_size(), _stream()),
               "tt_remap_nearest_labels")
    return out


# ---- N27: what a batch of compressed files is, whatever the codec (JPEG frames and annotation PNGs below): the thread pool of the host
# half, the status vocabulary, the one pinned buffer with its parts, the device-side preamble and the read-back of the files' status.
FILE_MAX_THREADS = 16
_FILE_POOLS: dict = {}


def _file_pool(workers: int):
    """One thread pool per size, kept: starting 16 threads per batch costs as much as scanning a dozen frames."""
    pool = _FILE_POOLS.get(workers)
    if pool is None:
        from concurrent.futures import ThreadPoolExecutor

        pool = _FILE_POOLS[workers] = ThreadPoolExecutor(workers, thread_name_prefix="tt_files")
    return pool


def _file_list(files: Sequence[bytes], who: str) -> list:
    files = [bytes(f) for f in files]
    if not files:
        raise ValueError(f"{who}: no files")
    return files


def _each_file(fn, n: int, threads: int, error=None, status=int) -> list:
    """[fn(i) for i in range(n)] in min(threads, 16, n) threads - one task per thread, not per file; serial at one.  With ``error``: then
    the first file in order whose ``status(result)`` is not 0 raises ``error(status, i)``."""
    workers = max(1, min(int(threads), FILE_MAX_THREADS, n))
    chunks = [range(k * n // workers, (k + 1) * n // workers) for k in range(workers)]
    work = lambda chunk: [fn(i) for i in chunk]
    results = [r for part in ([work(chunks[0])] if workers == 1 else _file_pool(workers).map(work, chunks)) for r in part]
    if error is not None:
        for i, r in enumerate(results):
            if status(r):
                raise error(status(r), i)
    return results


class _Codec:
    """The status vocabulary of one codec: its word, the reasons of its positive (unsupported) and negative (malformed) statuses, the
    fields ``probe`` fills, and - set where that class is declared - the exception of a file the device decoder does not take."""

    def __init__(self, word, unsupported, malformed, fields):
        self.word, self.unsupported, self.malformed, self.fields = word, unsupported, malformed, fields

    def error(self, status: int, index: Optional[int] = None) -> Exception:
        """The exception of a non-zero status: ValueError for a broken file (< 0), the codec's ``*Unsupported`` for one the device decoder
        does not take."""
        if status > 0:
            return self.unsupported_class(status, index)
        where = "" if index is None else f"file {index}: "
        return ValueError(f"{where}malformed {self.word} (status {status}: {self.malformed.get(int(status), 'unknown')})")

    def probed(self, info):
        """``info`` as ``*_probe`` returns it: a broken file raises"""
        if info.status < 0:
            raise self.error(info.status)
        return info


class _FileUnsupported(Exception):
    def __init_subclass__(cls, codec):
        cls.codec, codec.unsupported_class = codec, cls

    def __init__(self, status: int, index: Optional[int] = None):
        self.status, self.index = int(status), index
        where = "" if index is None else f"file {index}: "
        super().__init__(f"{where}unsupported {self.codec.word} ({self.codec.unsupported.get(int(status), status)})")


class _FileInfo:
    def __init_subclass__(cls, codec):
        cls.codec = codec

    @property
    def supported(self) -> bool:
        return self.status == 0

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={getattr(self, k)}' for k in ('status',) + self.codec.fields)})"


def _layout(parts):
    """[(name, bytes), ...] -> ({name: (offset, bytes)}, the bytes of the whole): every part on a 16-byte boundary"""
    layout, at = {}, 0
    for name, size in parts:
        layout[name] = (at, size)
        at += -(-size // 16) * 16
    return layout, at


class _FileBatch:
    def part(self, name):
        """A uint8 NumPy view of one part of ``meta``, by its name in ``layout``."""
        at, size = self.layout[name]
        return self.meta.numpy()[at:at + size]


def _need_gpu(who: str, device) -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.HipLibraryError(f"{who}: needs a GPU (the HIP path has no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def _file_status(status: torch.Tensor, codec: _Codec, bad=None) -> np.ndarray:
    """ONE read-back of the files' status (int32 [n] on the device); the first file in order whose status ``bad`` holds for raises."""
    host = status.cpu().numpy()
    if bad is not None:
        for i, rc in enumerate(host):
            if bad(rc):
                raise codec.error(int(rc), i)
    return host


# ---- N21, N24: JPEG frames.  The host half (tt_jpeg_probe, then tt_jpeg_scan: markers and Huffman codes - or, on the "device" route,
# tt_jpeg_prepare: markers only; pure host functions that ctypes runs without the GIL) in a thread pool, the arithmetic half
# (tt_jpeg_decode_batch) in two launches for the whole batch, behind tt_jpeg_entropy_batch on the "device" route.
JPEG_UNSUPPORTED = {1: "progressive, lossless or hierarchical frame", 2: "arithmetic coding", 3: "not three components", 4: "12-bit samples",
                    5: "sampling factors other than 4:4:4 / 4:2:2 / 4:2:0", 6: "more than one scan", 7: "16-bit quantisation tables",
                    8: "RGB stored without a colour transform"}
JPEG_MALFORMED = {-1: "broken markers, segment lengths or tables", -2: "the scan data ends early", -3: "a Huffman code no table holds",
                  -4: "a run past coefficient 63", -5: "a missing or misnumbered restart marker", -6: "bad argument"}
# the rows of the two descriptor tables (include/timetuning_hip.h), 128 bytes each: their fields are named here and nowhere else
_JPEG_FRAME = np.dtype([("H", "<i8"), ("W", "<i8"), ("sampling", "<i8"), ("coeff_off", "<i8", 3), ("qslot", "<i8", 3), ("plane_off", "<i8", 3),
                        ("out_off", "<i8"), ("reserved", "<i8", 3)])                                                  # tt_jpeg_frame
_JPEG_STREAM = np.dtype([("H", "<i8"), ("W", "<i8"), ("sampling", "<i8"), ("restart", "<i8"), ("scan_off", "<i8"), ("scan_len", "<i8"),
                         ("huff_off", "<i8"), ("seg_off", "<i8"), ("n_segments", "<i8"), ("coeff_off", "<i8", 3), ("reserved", "<i8", 4)])   # tt_jpeg_stream
_JPEG_QTABLES = 3 * 64 * 2     # bytes of one file's quantisation tables: uint16 [3, 64]
_JPEG = _Codec("JPEG", JPEG_UNSUPPORTED, JPEG_MALFORMED, ("H", "W", "sampling", "n_coeffs"))


class JpegUnsupported(_FileUnsupported, codec=_JPEG):
    """A well-formed JPEG file the device decoder does not take (``status`` > 0: TT_JPEG_UNSUPPORTED_*).  hip_ops has no CPU fallback;
    data_loader decodes such a file with Pillow and counts it."""


class JpegInfo(_FileInfo, codec=_JPEG):
    """What ``jpeg_probe`` found: ``status`` 0 = the device decoder takes the file (then H, W, ``sampling`` 0 / 1 / 2 = 4:4:4 / 4:2:2 /
    4:2:0 and the number of int16 coefficients are set), > 0 = unsupported."""

    def __init__(self, status, H, W, sampling, n_coeffs):
        self.status, self.H, self.W, self.sampling, self.n_coeffs = status, H, W, sampling, n_coeffs


def _jpeg_probe_raw(lib, data: bytes) -> JpegInfo:
    H, W, samp, n = C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
    rc = lib.tt_jpeg_probe(data, len(data), C.byref(H), C.byref(W), C.byref(samp), C.byref(n))
    return JpegInfo(rc, H.value, W.value, samp.value, n.value)


def jpeg_probe(data: bytes) -> JpegInfo:
    """Classifies a JPEG file without decoding it.  A broken file raises ValueError; an unsupported one is a JpegInfo with status > 0."""
    return _JPEG.probed(_jpeg_probe_raw(_lib.load(), bytes(data)))


def jpeg_scan(data: bytes):
    """Host only: (JpegInfo, coefficients int16 [n_coeffs], quantisation tables uint16 [3, 64]) of one supported file - the entropy layer
    alone, for tests and tools.  Raises ValueError (broken file) or JpegUnsupported."""
    lib = _lib.load()
    data = bytes(data)
    info = jpeg_probe(data)
    if not info.supported:
        raise _JPEG.error(info.status)
    coeffs, q = np.empty(info.n_coeffs, np.int16), np.empty((3, 64), np.uint16)
    rc = lib.tt_jpeg_scan(data, len(data), coeffs.ctypes.data, coeffs.size, q.ctypes.data)
    if rc:
        raise _JPEG.error(rc)
    return info, coeffs, q


def _jpeg_grid(H: int, W: int, sampling: int, comp: int):
    hmax, vmax = (1 if sampling == 0 else 2), (2 if sampling == 2 else 1)
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    return (my * vmax, mx * hmax) if comp == 0 else (my, mx)


class JpegBatch(_FileBatch):
    """The host half of a batch, ready for the device.  ``route`` "host" (N21): ``coeffs`` holds the int16 coefficients and ``meta`` the
    frame table, then the quantisation tables.  ``route`` "device" (N24: the host copies each scan once, what crosses PCIe is the
    compressed stream, and tt_jpeg_entropy_batch leaves the coefficients where tt_jpeg_decode_batch reads them): ``coeffs`` is None and
    ``meta`` holds the stream table, the frame table, the quantisation tables, the segment table, then every file's Huffman tables and
    clean stream.  Either way ONE pinned buffer per copy; ``layout``: name -> (offset, bytes) of ``meta``'s parts, each on a 16-byte
    boundary - 'frames' and 'qtables', on the device route also 'streams', 'segs' and 'scan'; ``groups`` (size -> offset in the output,
    count), ``where`` (file -> size, place in its group) and ``out_bytes``: the output."""

    def __init__(self, route, infos, meta, layout, coeffs, n_coeffs, n_segs, out_bytes, groups, where):
        self.route, self.infos, self.meta, self.layout, self.coeffs, self.n_coeffs, self.n_segs = route, infos, meta, layout, coeffs, n_coeffs, n_segs
        self.out_bytes, self.groups, self.where = out_bytes, groups, where


def _jpeg_batch(files: Sequence[bytes], threads: int, pin: bool, route: str) -> JpegBatch:
    """What ``jpeg_scan_batch`` (route "host") and ``jpeg_prepare_batch`` ("device") share - the pool, the probes, the output layout and the
    frame table - around what they do not: the buffers each fills and the host entry that fills them."""
    lib = _lib.load()
    files = _file_list(files, f"jpeg_{'scan' if route == 'host' else 'prepare'}_batch")
    n = len(files)
    each = lambda fn, status=int: _each_file(fn, n, threads, _JPEG.error, status)
    infos = each(lambda i: _jpeg_probe_raw(lib, files[i]), lambda info: info.status)
    # a component's int16 coefficients and the bytes of its plane are one number, so one running sum places both
    sizes = np.array([[rows * cols * 64 for rows, cols in (_jpeg_grid(f.H, f.W, f.sampling, c) for c in range(3))] for f in infos], np.int64)
    offs, total = (np.cumsum(sizes) - sizes.reshape(-1)).reshape(n, 3), int(sizes.sum())
    # output layout: the frames of one size lie one after the other, so that they are views of one [k, H, W, 3] tensor
    groups, where = {}, []
    for i, info in enumerate(infos):
        members = groups.setdefault((info.H, info.W), [])
        where.append(((info.H, info.W), len(members)))
        members.append(i)
    out_bytes, group_base = 0, {}
    for key, members in groups.items():
        group_base[key] = out_bytes
        out_bytes += -(-len(members) * key[0] * key[1] * 3 // 16) * 16
    parts, coeffs = [("frames", n * _JPEG_FRAME.itemsize), ("qtables", n * _JPEG_QTABLES)], None
    if route == "host":
        coeffs = torch.empty(total, dtype=torch.int16, pin_memory=pin)
    else:
        scan_cap, seg_cap = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        a, b = C.c_size_t(), C.c_size_t()
        for i, (f, info) in enumerate(zip(files, infos)):
            lib.tt_jpeg_prepare_bytes(len(f), C.byref(a), C.byref(b))
            rows, cols = _jpeg_grid(info.H, info.W, info.sampling, 1)
            mcus = rows * cols     # (the chroma grid is the grid of MCUs)
            # a frame has at most one segment per MCU, and a boundary costs the stream at most one byte: tighter than the bound from len alone
            scan_cap[i + 1], seg_cap[i + 1] = min(a.value, -(-(1632 + len(f) + mcus + 8) // 4) * 4), min(b.value, mcus)
        np.cumsum(scan_cap, out=scan_cap)
        np.cumsum(seg_cap, out=seg_cap)
        parts = [("streams", n * _JPEG_STREAM.itemsize)] + parts + [("segs", int(seg_cap[-1]) * 8), ("scan", int(scan_cap[-1]))]
    layout, meta_bytes = _layout(parts)
    meta = torch.zeros(meta_bytes, dtype=torch.uint8, pin_memory=pin)    # every table and stream of the batch: one copy
    batch = JpegBatch(route, infos, meta, layout, coeffs, total, 0 if route == "host" else int(seg_cap[-1]), out_bytes,
                      {k: (group_base[k], len(m)) for k, m in groups.items()}, where)
    q_at = meta.data_ptr() + layout["qtables"][0]
    if route == "host":
        c_base, first = coeffs.data_ptr(), offs[:, 0].tolist()      # plain ints: the calls below run once per file
        each(lambda i: lib.tt_jpeg_scan(files[i], len(files[i]), c_base + 2 * first[i], infos[i].n_coeffs, q_at + i * _JPEG_QTABLES))
    else:
        scan_at, segs_at, rows_at = (meta.data_ptr() + layout[name][0] for name in ("scan", "segs", "streams"))
        sc, sg = scan_cap.tolist(), seg_cap.tolist()
        each(lambda i: lib.tt_jpeg_prepare(files[i], len(files[i]), scan_at + sc[i], sc[i + 1] - sc[i], segs_at + 8 * sg[i], sg[i + 1] - sg[i],
                                           rows_at + i * _JPEG_STREAM.itemsize, q_at + i * _JPEG_QTABLES))
        streams = batch.part("streams").view(_JPEG_STREAM)     # tt_jpeg_prepare counts from the file's own slots: now from the buffers
        streams["scan_off"] += scan_cap[:-1]
        streams["huff_off"] += scan_cap[:-1]
        streams["seg_off"] += seg_cap[:-1]
        streams["coeff_off"] += offs[:, :1]
    frames = batch.part("frames").view(_JPEG_FRAME)
    for name in ("H", "W", "sampling"):
        frames[name] = [getattr(info, name) for info in infos]
    frames["coeff_off"] = frames["plane_off"] = offs
    frames["qslot"] = np.arange(3 * n).reshape(n, 3)
    frames["out_off"] = [group_base[key] + k * key[0] * key[1] * 3 for key, k in where]
    return batch


def jpeg_scan_batch(files: Sequence[bytes], threads: int = 8, pin: bool = True) -> JpegBatch:
    """The host route.  Probes and entropy-decodes every file in a pool of min(threads, 16) threads into ONE (pinned) coefficient buffer and
    builds the descriptor table.  Raises JpegUnsupported for the first unsupported file and ValueError for the first broken one.  The
    pinned buffers come from torch's caching host allocator: a steady stream of batches allocates nothing after the first."""
    return _jpeg_batch(files, threads, pin, "host")


def jpeg_prepare_batch(files: Sequence[bytes], threads: int = 8, pin: bool = True) -> JpegBatch:
    """The device route.  Probes every file and copies its scan, cleaned and cut at the restart markers, into ONE (pinned) buffer in the
    same pool; nothing is decoded.  Raises JpegUnsupported for the first unsupported file and ValueError for the first broken one
    (markers and restart numbering; the codes themselves are the device's to judge)."""
    return _jpeg_batch(files, threads, pin, "device")


# ---- N24: the Huffman streams of a device-route batch decoded on the device (tt_jpeg_entropy_batch) or, for tests, by its host emulation.
JPEG_SUBSEQ_BITS = 2048   # bits of stream per lane: the default ``subseq_bits`` (profiles/n24_jpeg_entropy.txt); an argument, not a state


def _jpeg_subseq_bits(subseq_bits) -> int:
    bits = JPEG_SUBSEQ_BITS if subseq_bits is None else int(subseq_bits)
    if bits % 32 or not 128 <= bits <= 4096:
        raise ValueError(f"jpeg entropy decode: subseq_bits {bits} is not a multiple of 32 in [128, 4096]")
    return bits


def jpeg_entropy_host(batch: JpegBatch, subseq_bits=None):
    """The host emulation of the device entropy decode (tt_jpeg_entropy_host: the kernel's phases lane by lane through the same header),
    for tests and tools: (coefficients int16 [n_coeffs], status int32 [n], statistics int32 [n, 4] = rounds, tiles, subsequences, the
    first failing subsequence).  Raises nothing for a broken stream: the status says it."""
    lib, n, bits = _lib.load(), len(batch.infos), _jpeg_subseq_bits(subseq_bits)
    coeffs, status = np.empty(max(batch.n_coeffs, 1), np.int16), np.zeros(n, np.int32)
    streams, segs, scan = batch.part("streams"), batch.part("segs"), batch.part("scan")
    ws = np.zeros(int(lib.tt_jpeg_entropy_batch_workspace_bytes(streams.ctypes.data, n, bits)) // 4, np.int32)
    _lib.check(lib.tt_jpeg_entropy_host(scan.ctypes.data, scan.size, segs.ctypes.data, segs.ctypes.data, batch.n_segs, streams.ctypes.data,
                                        streams.ctypes.data, n, bits, coeffs.ctypes.data, batch.n_coeffs, status.ctypes.data, ws.ctypes.data,
                                        ws.nbytes, None), "tt_jpeg_entropy_host")
    return coeffs[:batch.n_coeffs], status, ws[:4 * n].reshape(n, 4)


def jpeg_entropy_decode(batch: JpegBatch, device=None, subseq_bits=None, stats: bool = False):
    """The device entropy decode: one host-to-device copy of the batch's buffer (the compressed streams and their tables), a memset and
    one launch on the current stream, then ONE read-back of 4 n bytes - the frames' status.  Returns (coefficients int16 [n_coeffs] on the
    device, in the layout of the batch's frame table; status int32 [n] on the host; the batch's buffer on the device).  A negative status
    raises ValueError naming the file.  ``stats``: the per-frame statistics (rounds, tiles, subsequences, -1) as a fourth item."""
    lib, dev = _lib.load(), _need_gpu("jpeg_entropy_decode", device)
    n, bits = len(batch.infos), _jpeg_subseq_bits(subseq_bits)
    streams, segs = batch.part("streams"), batch.part("segs")
    ws_bytes = int(lib.tt_jpeg_entropy_batch_workspace_bytes(streams.ctypes.data, n, bits))
    with torch.cuda.device(dev):
        meta = batch.meta.to(dev, non_blocking=True)
        coeffs = torch.empty(max(batch.n_coeffs, 8), dtype=torch.int16, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if stats else _ws(ws_bytes, dev)
        at = lambda name: meta.data_ptr() + batch.layout[name][0]
        _lib.check(lib.tt_jpeg_entropy_batch(at("scan"), batch.layout["scan"][1], segs.ctypes.data, at("segs"), batch.n_segs, streams.ctypes.data,
                                             at("streams"), n, bits, _p(coeffs), batch.n_coeffs, _p(status), _p(ws), ws.numel(), _stream()),
                   "tt_jpeg_entropy_batch")
        host_status = _file_status(status, _JPEG, lambda rc: rc < 0)
    if stats:
        return coeffs, host_status, meta, ws[:16 * n].view(torch.int32).view(n, 4).cpu().numpy()
    return coeffs, host_status, meta


def jpeg_decode(batch: JpegBatch, device=None, subseq_bits=None):
    """The device half.  Host route: one host-to-device copy of the coefficients, one of the tables, two launches on the current stream.
    Device route: ``jpeg_entropy_decode`` (``subseq_bits`` is its), then the same two launches on the device-resident coefficients.
    Returns the frames as uint8 [H, W, 3] tensors in the order of the files; frames of one size are consecutive views of one
    [k, H, W, 3] tensor (``frames_as_clip`` returns it without a copy)."""
    lib, dev = _lib.load(), _need_gpu("decode_jpeg_batch", device)
    n = len(batch.infos)
    table = batch.part("frames")
    ws_bytes = int(lib.tt_jpeg_decode_batch_workspace_bytes(table.ctypes.data, n))
    if ws_bytes == 0:
        raise ValueError("decode_jpeg_batch: the descriptor table holds a row that is not a frame")
    with torch.cuda.device(dev):
        if batch.route == "device":
            coeffs, _, meta = jpeg_entropy_decode(batch, dev, subseq_bits)
        else:
            coeffs, meta = batch.coeffs.to(dev, non_blocking=True), batch.meta.to(dev, non_blocking=True)
        out = torch.empty(max(batch.out_bytes, 16), dtype=torch.uint8, device=dev)
        ws = _ws(ws_bytes, dev)
        _lib.check(lib.tt_jpeg_decode_batch(_p(coeffs), batch.n_coeffs, meta.data_ptr() + batch.layout["qtables"][0], 3 * n, table.ctypes.data,
                                            meta.data_ptr() + batch.layout["frames"][0], n, _p(out), out.numel(), _p(ws), ws.numel(), _stream()),
                   "tt_jpeg_decode_batch")
    stacks = {key: out[base:base + k * key[0] * key[1] * 3].view(k, key[0], key[1], 3) for key, (base, k) in batch.groups.items()}
    return [stacks[key][k] for key, k in batch.where]


def decode_jpeg_batch(files: Sequence[bytes], device=None, threads: int = 8, entropy: str = "host", subseq_bits=None):
    """JPEG files -> uint8 [H, W, 3] GPU tensors, bit-equal to Pillow's decode.  The frames may differ in size and sampling; those of one
    size come back as views of one [k, H, W, 3] tensor.  Unsupported files raise JpegUnsupported (no CPU fallback here), broken ones
    ValueError.  ``entropy``: "host" undoes the Huffman coding in the thread pool and copies coefficients; "device" copies the compressed
    scans and undoes it in one launch (``subseq_bits``: bits of stream per lane, None = JPEG_SUBSEQ_BITS)."""
    if entropy not in ("host", "device"):
        raise ValueError(f"decode_jpeg_batch: entropy must be 'host' or 'device', not {entropy!r}")
    return jpeg_decode(_jpeg_batch(files, threads, True, entropy), device, subseq_bits)


def frames_as_clip(frames: Sequence[torch.Tensor]) -> torch.Tensor:
    """Frames [H, W, 3] - or label maps [H, W], or views of any one shape - -> [k, ...]: the tensor they are consecutive views of where
    they are (``jpeg_decode``, ``png_decode``), a stacked copy otherwise."""
    f0 = frames[0]
    step = f0.numel()
    same = all(f.shape == f0.shape and f.dtype == f0.dtype and f.is_contiguous() and f.device == f0.device and
               f.untyped_storage().data_ptr() == f0.untyped_storage().data_ptr() and
               f.storage_offset() == f0.storage_offset() + i * step for i, f in enumerate(frames))
    if not same:
        return torch.stack(list(frames))
    return f0.as_strided((len(frames) * step,), (1,), f0.storage_offset()).view(len(frames), *f0.shape)


# ---- N22: ragged image kernels.  A batch of images (or label maps) of different sizes through ONE launch: a descriptor row per item and one
# int32 pool of taps / bounds / index tables, each uploaded with one copy.
_RAGGED_ROW = 16     # int64 words of one tt_img_ragged_item
(_RG_SRC, _RG_H, _RG_W, _RG_X0, _RG_Y0, _RG_BW, _RG_BH, _RG_FLIP, _RG_HK, _RG_HB, _RG_HKS, _RG_VK, _RG_VB, _RG_VKS, _RG_YT, _RG_XT) = range(16)
IMG_RAGGED_BAND, IMG_RAGGED_LDS_BUDGET = 16, 65536


def img_resize_ragged_shape_ok(h: int, w: int, OH: int, OW: int) -> bool:
    """Whether ``tt_img_resize_ragged`` takes an ``h x w`` box resized to ``OH x OW``: the source rows the widest band of 16 output rows
    reaches, as uint8 [rows, OW, 3], fit 64 KiB of LDS (pure host function)."""
    return bool(_lib.load().tt_img_resize_ragged_shape_ok(int(h), int(w), int(OH), int(OW)))


def _ragged_size(size):
    OH, OW = (size, size) if isinstance(size, int) else size
    return int(OH), int(OW)


def _ragged_source(items: Sequence[torch.Tensor], what: str, ndim: int):
    """The items' common buffer without a copy where they are views of one storage (``decode_jpeg_batch``'s frames, slices of a packed mask
    buffer), else ONE ``torch.cat`` of their flattened views: (keep-alive tensor, base pointer, bytes, byte offset of every item)."""
    if len(items) == 0:
        raise ValueError(f"{what}: no items")
    for t in items:
        _chk(t, what, torch.uint8)
        if t.dim() != ndim or (ndim == 3 and t.shape[2] != 3) or t.numel() == 0:
            raise ValueError(f"{what}: uint8 {'[H, W, 3]' if ndim == 3 else '[H, W]'} tensors are needed, got {tuple(t.shape)}")
        if t.device != items[0].device:
            raise ValueError(f"{what}: the items lie on different devices")
    s0 = items[0].untyped_storage()
    if all(t.untyped_storage().data_ptr() == s0.data_ptr() for t in items):
        base = min(t.data_ptr() for t in items)
        return list(items), base, max(t.data_ptr() + t.numel() for t in items) - base, [t.data_ptr() - base for t in items]
    packed = torch.cat([t.reshape(-1) for t in items])
    offs = np.zeros(len(items) + 1, np.int64)
    np.cumsum([t.numel() for t in items], out=offs[1:])
    return packed, packed.data_ptr(), packed.numel(), [int(o) for o in offs[:-1]]


class _RaggedPool:
    """The int32 pool of one call, deduplicated by key (``array``: the whole pool as one host array)."""

    def __init__(self):
        self.parts, self.where, self.length = [], {}, 0

    def array(self) -> np.ndarray:
        return np.concatenate(self.parts) if self.parts else np.zeros(0, np.int32)

    def add(self, key, make):
        hit = self.where.get(key)
        if hit is None:
            arrays = make()
            hit = []
            for a in arrays:
                a = np.ascontiguousarray(a, np.int32).reshape(-1)
                hit.append(self.length)
                self.parts.append(a)
                self.length += a.size
            self.where[key] = hit
        return hit


def _ragged_upload(table: np.ndarray, pool: np.ndarray, device):
    """The descriptor table and the pool, each written into one pinned buffer and uploaded with one copy: (host table, device table, host
    pool, device pool).  The host copies are what the entry points validate."""
    table_host = torch.empty(table.size, dtype=torch.int64, pin_memory=True)
    table_host.numpy()[:] = table.reshape(-1)
    pool_host = torch.zeros(max(pool.size, 1), dtype=torch.int32, pin_memory=True)
    pool_host.numpy()[:pool.size] = pool
    return table_host, table_host.to(device, non_blocking=True), pool_host, pool_host.to(device, non_blocking=True)


def _ragged_boxes(dims, boxes, flips, what: str):
    n = len(dims)
    boxes = [None] * n if boxes is None else list(boxes)
    flips = [False] * n if flips is None else list(flips)
    if len(boxes) != n or len(flips) != n:
        raise ValueError(f"{what}: {n} items but {len(boxes)} boxes / {len(flips)} flips")
    out = []
    for (H, W), box in zip(dims, boxes):
        x0, y0, w, h = (0, 0, W, H) if box is None else (int(v) for v in box)
        if w < 1 or h < 1 or x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
            raise ValueError(f"{what}: box (x0 {x0}, y0 {y0}, w {w}, h {h}) outside its image {H} x {W}")
        out.append((x0, y0, w, h))
    return out, [bool(f) for f in flips]


def _ragged_rows(dims, offsets, boxes, flips) -> np.ndarray:
    table = np.zeros((len(dims), _RAGGED_ROW), np.int64)
    for row, (H, W), off, (x0, y0, w, h), flip in zip(table, dims, offsets, boxes, flips):
        row[_RG_SRC], row[_RG_H], row[_RG_W] = off, H, W
        row[_RG_X0], row[_RG_Y0], row[_RG_BW], row[_RG_BH], row[_RG_FLIP] = x0, y0, w, h, int(flip)
    return table


def img_resize_ragged_plan(dims, offsets, size, boxes=None, flips=None):
    """Host only: the descriptor table (int64 [n, 16], the words of ``tt_img_ragged_item``) and the int32 pool ``tt_img_resize_ragged``
    takes for images of ``dims[i] = (H, W)`` at byte ``offsets[i]``.  The taps are ``video_transformations.resample_coeffs`` (pinned
    against Pillow), one copy per (in, out) length; a pass of equal lengths gets none."""
    from . import video_transformations as VT

    OH, OW = _ragged_size(size)
    boxes, flips = _ragged_boxes(dims, boxes, flips, "img_resize_ragged")
    table, pool = _ragged_rows(dims, offsets, boxes, flips), _RaggedPool()

    def taps(n_in, n_out):
        kk, bounds = VT.resample_coeffs(n_in, n_out)
        return pool.add(("taps", n_in, n_out), lambda: (kk.numpy(), bounds.numpy())) + [kk.shape[1]]

    for row, (x0, y0, w, h) in zip(table, boxes):
        if w != OW:
            row[_RG_HK], row[_RG_HB], row[_RG_HKS] = taps(w, OW)
        if h != OH:
            row[_RG_VK], row[_RG_VB], row[_RG_VKS] = taps(h, OH)
    return table, pool.array()


def img_gather_nearest_ragged_plan(dims, offsets, size, boxes=None, flips=None):
    """Host only: table and pool for ``tt_img_gather_nearest_ragged``; the tables are ``video_transformations.nearest_table`` with the crop
    offset and the flip folded in, one copy per distinct table."""
    from . import video_transformations as VT

    OH, OW = _ragged_size(size)
    boxes, flips = _ragged_boxes(dims, boxes, flips, "img_gather_nearest_ragged")
    table, pool = _ragged_rows(dims, offsets, boxes, flips), _RaggedPool()
    for row, (x0, y0, w, h), flip in zip(table, boxes, flips):
        row[_RG_YT], = pool.add(("near", h, OH, y0, False), lambda: (VT.nearest_table(h, OH, y0),))
        row[_RG_XT], = pool.add(("near", w, OW, x0, flip), lambda: (VT.nearest_table(w, OW, x0, flip),))
    return table, pool.array()


def img_resize_ragged(frames: Sequence[torch.Tensor], size, boxes=None, flips=None, to_tensor=None, out=None):
    """``Image.crop(box).resize((OW, OH), BILINEAR)`` of every frame of a mixed-size batch in ONE launch.  ``frames``: uint8 [H, W, 3] GPU
    tensors (the views ``decode_jpeg_batch`` returns are used where they lie, by byte offset); ``size``: S or (OH, OW); ``boxes``: per item
    ``(x0, y0, w, h)`` or None = the whole image; ``flips``: per item, mirror the output row.  Returns uint8 [n, OH, OW, 3], or with
    ``to_tensor=(mean, std)`` the finished float32 [n, 3, OH, OW].  An item ``img_resize_ragged_shape_ok`` refuses goes through
    ``video_transformations.resized_crop`` into its row of the same output: the result does not depend on the route.  ``out``: an output
    tensor of that shape and dtype to write into (tests)."""
    from . import video_transformations as VT

    lib = _lib.load()
    OH, OW = _ragged_size(size)
    keep, base, in_bytes, offs = _ragged_source(frames, "frames", 3)
    dev = frames[0].device
    n = len(frames)
    dims = [(t.shape[0], t.shape[1]) for t in frames]
    boxes, flips = _ragged_boxes(dims, boxes, flips, "img_resize_ragged")
    shape = (n, OH, OW, 3) if to_tensor is None else (n, 3, OH, OW)
    dtype = torch.uint8 if to_tensor is None else f32
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=dev)
    elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"img_resize_ragged: out must be a contiguous {dtype} tensor {shape} on {dev}")
    fast = [i for i in range(n) if lib.tt_img_resize_ragged_shape_ok(boxes[i][3], boxes[i][2], OH, OW)]
    m3 = s3 = None
    if to_tensor is not None:
        mean, std = to_tensor
        m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    with torch.cuda.device(dev):
        if fast:
            table, pool = img_resize_ragged_plan([dims[i] for i in fast], [offs[i] for i in fast], (OH, OW), [boxes[i] for i in fast],
                                                 [flips[i] for i in fast])
            table_host, table_dev, pool_host, pool_dev = _ragged_upload(table, pool, dev)
            whole = len(fast) == n
            dst = out if whole else torch.empty((len(fast),) + shape[1:], dtype=dtype, device=dev)
            _lib.check(lib.tt_img_resize_ragged(base, in_bytes, table_host.data_ptr(), _p(table_dev), len(fast), pool_host.data_ptr(), _p(pool_dev),
                                                pool.size, _p(dst) if to_tensor is None else None, None if to_tensor is None else _p(dst),
                                                OH, OW, m3, s3, _stream()), "tt_img_resize_ragged")
            if not whole:
                out[torch.as_tensor(fast, device=dev)] = dst
        taken = set(fast)
        for i in range(n):
            if i in taken:
                continue
            x0, y0, w, h = boxes[i]
            one = VT.resized_crop(frames[i][None], y0, x0, h, w, (OH, OW), to_tensor, flips[i])
            if to_tensor is None and flips[i]:
                one = one.flip(2)
            out[i] = one[0]
    del keep
    return out


def img_gather_nearest_ragged(maps: Sequence[torch.Tensor], size, boxes=None, flips=None, to_tensor: bool = False, out=None):
    """``Image.crop(box).resize((OW, OH), NEAREST)`` of every label map of a mixed-size batch in ONE launch.  ``maps``: uint8 [H, W] GPU
    tensors (slices of one packed buffer are used where they lie).  Returns uint8 [n, OH, OW], or with ``to_tensor`` float32
    [n, 1, OH, OW] = v / 255.  The tables are ``video_transformations.nearest_table`` with the crop offset and the flip folded in."""
    lib = _lib.load()
    OH, OW = _ragged_size(size)
    keep, base, in_bytes, offs = _ragged_source(maps, "maps", 2)
    dev = maps[0].device
    n = len(maps)
    table, pool = img_gather_nearest_ragged_plan([(t.shape[0], t.shape[1]) for t in maps], offs, (OH, OW), boxes, flips)
    shape = (n, 1, OH, OW) if to_tensor else (n, OH, OW)
    dtype = f32 if to_tensor else torch.uint8
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=dev)
    elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"img_gather_nearest_ragged: out must be a contiguous {dtype} tensor {shape} on {dev}")
    with torch.cuda.device(dev):
        table_host, table_dev, pool_host, pool_dev = _ragged_upload(table, pool, dev)
        _lib.check(lib.tt_img_gather_nearest_ragged(base, in_bytes, table_host.data_ptr(), _p(table_dev), n, pool_host.data_ptr(), _p(pool_dev),
                                                    pool.size, None if to_tensor else _p(out), _p(out) if to_tensor else None, OH, OW,
                                                    _stream()), "tt_img_gather_nearest_ragged")
    del keep
    return out


# ------------------------------------------------------------------------------------------------
# N23: label maps as byte streams (csrc/label_map.hip)
# ------------------------------------------------------------------------------------------------

_LABEL_MAP_BYTES = {torch.uint8: 1, torch.int64: 8}


def _chk_label_segments(labels: torch.Tensor, name: str, dtypes) -> torch.Tensor:
    if labels.dtype not in dtypes:
        raise TypeError(f"{name}: expected {' or '.join(str(d) for d in dtypes)}, got {labels.dtype}")
    _chk(labels, name, labels.dtype)
    if labels.dim() != 2 or labels.shape[0] < 1 or labels.shape[1] < 1:
        raise ValueError(f"{name}: expected [S, P] with S, P >= 1, got {tuple(labels.shape)}")
    return labels


def _label_presence_into(labels: torch.Tensor, words: torch.Tensor, status: torch.Tensor) -> None:
    S, P = labels.shape
    with torch.cuda.device(labels.device):
        _lib.check(_lib.load().tt_label_presence_segments(_p(labels), _LABEL_MAP_BYTES[labels.dtype], S, P, _p(words), _p(status), _stream()),
                   "tt_label_presence_segments")


def label_presence(labels: torch.Tensor):
    """labels uint8 or int64 [S, P] -> (words int32 [S, 8], status int32 [S]), one launch: bit ``v & 31`` of ``words[s, v >> 5]`` (read as
    unsigned) is set iff value v in 0 .. 255 occurs in row s; ``status[s]`` is 1 where an int64 value lies outside 0 .. 255."""
    _chk_label_segments(labels, "labels", _LABEL_MAP_BYTES)
    S = labels.shape[0]
    words = torch.empty((S, 8), dtype=torch.int32, device=labels.device)
    status = torch.empty((S,), dtype=torch.int32, device=labels.device)
    _label_presence_into(labels, words, status)
    return words, status


def presence_values(words_row) -> list:
    """Host only: the ascending values whose bit is set in one row of ``label_presence``'s words (8 integers, signed or unsigned)."""
    return [32 * k + b for k, w in enumerate(words_row) for b in range(32) if (int(w) >> b) & 1]


def label_value_counts(labels: torch.Tensor) -> list:
    """``[torch.unique(row).shape[0] for row in labels]`` for label maps uint8 or int64 [S, P]: one presence launch and ONE read-back (the 32
    bytes of presence bits and the status word of every row), popcount on the host.  A row whose status is set - an int64 value outside
    0 .. 255 - is counted by ``torch.unique`` instead."""
    _chk_label_segments(labels, "labels", _LABEL_MAP_BYTES)
    S = labels.shape[0]
    packed = torch.empty((S * 9,), dtype=torch.int32, device=labels.device)   # words [S, 8], then status [S]: one copy brings both
    _label_presence_into(labels, packed[: S * 8], packed[S * 8:])
    host = packed.cpu().numpy()
    words, status = host[: S * 8].view(np.uint8).reshape(S, 32), host[S * 8:]
    counts = np.unpackbits(words, axis=1).sum(axis=1)
    return [int(counts[s]) if status[s] == 0 else int(torch.unique(labels[s]).shape[0]) for s in range(S)]


def map_instances(labels: torch.Tensor, cat: torch.Tensor, sequential: bool = True, out: Optional[torch.Tensor] = None):
    """The YouTube-VOS instance -> category remap (``data_loader.map_instances``, reference ``:497-506``) of S clips in two launches.
    labels uint8 [S, P]; cat int32 [S, 256], the category of each object id of row s's video, -1 = not in the meta file.  Returns
    ``(mapped uint8 [S, P], lut uint8 [S, 256], status int32 [S])``; the table is ``data_loader.compose_instance_lut``'s: ``sequential``
    reproduces the reference's chained in-place loop, otherwise ``v -> cat[v]``.  ``status[s]`` != 0: the smallest present object id without
    a category; that row is copied unmapped.  ``out``: a uint8 tensor of labels' shape to write into, not overlapping labels (tests)."""
    lib = _lib.load()
    _chk_label_segments(labels, "labels", (torch.uint8,))
    _chk(cat, "cat", torch.int32)
    S, P = labels.shape
    if tuple(cat.shape) != (S, 256):
        raise ValueError(f"cat: expected [{S}, 256], got {tuple(cat.shape)}")
    if out is None:
        out = torch.empty_like(labels)
    elif out.shape != labels.shape or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != labels.device:
        raise ValueError(f"map_instances: out must be a contiguous uint8 tensor {tuple(labels.shape)} on {labels.device}")
    lut = torch.empty((S, 256), dtype=torch.uint8, device=labels.device)
    status = torch.empty((S,), dtype=torch.int32, device=labels.device)
    ws_bytes = int(lib.tt_map_instances_workspace_bytes(S))
    ws = _ws(ws_bytes, labels.device)
    with torch.cuda.device(labels.device):
        _lib.check(lib.tt_map_instances(_p(labels), _p(out), _p(cat), S, P, 1 if sequential else 0, _p(lut), _p(status), _p(ws), ws_bytes,
                                        _stream()), "tt_map_instances")
    return out, lut, status


# ---- N26: annotation PNGs.  The host half (tt_png_probe, tt_png_prepare: chunks and CRC-32 only, pure host functions that ctypes runs
# without the GIL) in the thread pool the JPEG batches use, the device half (tt_png_decode_batch: inflate, Adler-32, row filters, unpacking)
# in one launch for the whole batch.
PNG_UNSUPPORTED = {1: "Adam7 interlace", 2: "a colour type other than palette or gray", 3: "gray below 8 bits", 4: "16-bit samples",
                   5: "a side above 32767"}
PNG_MALFORMED = {-1: "broken signature, IHDR, zlib header or block header", -2: "the file, the stream or the output ends early",
                 -3: "a refused code-length set or a code no table holds", -4: "a back-reference before the first byte",
                 -5: "more inflated bytes than the header's rows hold", -6: "a wrong CRC-32 or Adler-32", -7: "a filter byte above 4",
                 -8: "bad argument"}
_PNG_STREAM = np.dtype([("H", "<i8"), ("W", "<i8"), ("depth", "<i8"), ("color_type", "<i8"), ("row_bytes", "<i8"), ("stream_off", "<i8"),
                        ("stream_len", "<i8"), ("out_off", "<i8"), ("ws_off", "<i8"), ("reserved", "<i8", 7)])                # tt_png_stream
PNG_STATS = ("kinds", "lit_bits", "dist_bits", "min_dist", "max_dist", "max_len", "filters", "bytes")   # the eight int32 per file
_PNG = _Codec("PNG", PNG_UNSUPPORTED, PNG_MALFORMED, ("H", "W", "depth", "color_type"))


class PngUnsupported(_FileUnsupported, codec=_PNG):
    """A well-formed PNG file the device decoder does not take (``status`` > 0: TT_PNG_UNSUPPORTED_*).  hip_ops has no CPU fallback;
    the loaders decode such a file with Pillow and count it."""


class PngInfo(_FileInfo, codec=_PNG):
    """What ``png_probe`` found: ``status`` 0 = the device decoder takes the file, > 0 = unsupported; H, W, bit depth, colour type."""

    def __init__(self, status, H, W, depth, color_type):
        self.status, self.H, self.W, self.depth, self.color_type = status, H, W, depth, color_type


def png_probe(data: bytes) -> PngInfo:
    """Classifies a PNG file without decoding it.  A broken file raises ValueError; an unsupported one is a PngInfo with status > 0."""
    data = bytes(data)
    H, W, depth, color = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rc = _lib.load().tt_png_probe(data, len(data), C.byref(H), C.byref(W), C.byref(depth), C.byref(color))
    return _PNG.probed(PngInfo(rc, H.value, W.value, depth.value, color.value))


class PngBatch(_FileBatch):
    """The host half of a batch of annotation files, ready for the device: ONE (pinned) buffer ``meta`` holding the stream table, then
    every file's deflate stream; ``layout``: name -> (offset, bytes) of its two parts 'table' and 'streams', each on a 16-byte boundary.
    The maps lie one after the other in the output (``out_bytes`` in all), so consecutive files of one size are one [k, H, W] tensor."""

    def __init__(self, infos, meta, layout, out_bytes, ws_bytes):
        self.infos, self.meta, self.layout, self.out_bytes, self.ws_bytes = infos, meta, layout, out_bytes, ws_bytes

    @property
    def table(self):
        return self.part("table").view(_PNG_STREAM)


def png_prepare_batch(files: Sequence[bytes], threads: int = 8, pin: bool = True) -> PngBatch:
    """Probes every file and copies its IDAT payloads, CRC-checked, into ONE (pinned) buffer in the thread pool; nothing is inflated.
    Raises PngUnsupported for the first unsupported file and ValueError for the first broken one (chunks, CRC-32, zlib header: the
    deflate stream itself is the device's to judge)."""
    lib = _lib.load()
    files = _file_list(files, "png_prepare_batch")
    n = len(files)
    cap = np.zeros(n + 1, np.int64)
    a = C.c_size_t()
    for i, f in enumerate(files):
        lib.tt_png_prepare_bytes(len(f), C.byref(a))
        cap[i + 1] = a.value
    np.cumsum(cap, out=cap)
    layout, _ = _layout([("table", n * _PNG_STREAM.itemsize), ("streams", int(cap[-1]))])
    meta = torch.zeros(sum(layout["streams"]), dtype=torch.uint8, pin_memory=pin)      # (ends with the last stream, not on a boundary)
    rows_at, streams_at, at = meta.data_ptr(), meta.data_ptr() + layout["streams"][0], cap.tolist()
    _each_file(lambda i: lib.tt_png_prepare(files[i], len(files[i]), streams_at + at[i], at[i + 1] - at[i], rows_at + i * _PNG_STREAM.itemsize),
               n, threads, _PNG.error)
    table = meta.numpy()[:layout["table"][1]].view(_PNG_STREAM)
    table["stream_off"] = cap[:-1]
    pixels = table["H"] * table["W"]
    slices = (table["H"] * (1 + table["row_bytes"]) + 15) // 16 * 16
    table["out_off"] = np.cumsum(pixels) - pixels
    table["ws_off"] = np.cumsum(slices) - slices
    infos = [PngInfo(0, int(r["H"]), int(r["W"]), int(r["depth"]), int(r["color_type"])) for r in table]
    return PngBatch(infos, meta, layout, int(pixels.sum()), int(lib.tt_png_decode_batch_workspace_bytes(table.ctypes.data, n)))


def _png_views(flat, table):
    return [flat[int(r["out_off"]):int(r["out_off"]) + int(r["H"]) * int(r["W"])].reshape(int(r["H"]), int(r["W"])) for r in table]


def png_decode_host(batch: PngBatch, lanes: int = 1):
    """The host emulation of the device decode (tt_png_decode_host: the sequential loop over the kernel's steps), for tests and tools:
    (the maps as uint8 [H, W] NumPy views of one flat buffer, status int32 [n], statistics int32 [n, 8] in the order of PNG_STATS, the
    inflated - and, where the status is 0, unfiltered - bytes of every file).  Raises nothing for a broken stream: the status says it.
    ``lanes`` = 64: tt_png_decode_host_wave, the inflate with the kernel's 64 lanes as 64 threads behind a barrier (slow on large files)."""
    if lanes not in (1, 64):
        raise ValueError(f"png_decode_host: lanes must be 1 or 64, not {lanes}")
    lib, n = _lib.load(), len(batch.infos)
    table, streams = batch.table, batch.part("streams")
    out, status = np.zeros(max(batch.out_bytes, 1), np.uint8), np.zeros(n, np.int32)
    ws = np.zeros(batch.ws_bytes // 4 + 1, np.int32)
    entry = "tt_png_decode_host" if lanes == 1 else "tt_png_decode_host_wave"
    _lib.check(getattr(lib, entry)(streams.ctypes.data, streams.size, table.ctypes.data, table.ctypes.data, n, out.ctypes.data, batch.out_bytes,
                                   ws.ctypes.data, batch.ws_bytes, status.ctypes.data, None), entry)
    raw = ws.view(np.uint8)
    slices = [raw[int(r["ws_off"]):int(r["ws_off"]) + int(r["H"]) * (1 + int(r["row_bytes"]))] for r in table]
    return _png_views(out, table), status, ws[(batch.ws_bytes - 32 * n) // 4:batch.ws_bytes // 4].reshape(n, 8), slices


def png_decode(batch: PngBatch, device=None, out: Optional[torch.Tensor] = None, check: bool = True):
    """The device half: one host-to-device copy of the batch's buffer, ONE launch on the current stream, one read-back of 4 n bytes - the
    files' status.  Returns (the maps as uint8 [H, W] views of ONE flat device buffer in file order - ``out``, a contiguous uint8 tensor
    of at least ``batch.out_bytes`` elements, when given -, status int32 [n] on the host).  A non-zero status raises ValueError naming
    the file and the reason unless ``check`` is False."""
    lib, dev = _lib.load(), _need_gpu("png_decode", device)
    n, table = len(batch.infos), batch.table
    with torch.cuda.device(dev):
        meta = batch.meta.to(dev, non_blocking=True)
        if out is None:
            out = torch.empty(max(batch.out_bytes, 16), dtype=torch.uint8, device=dev)
        elif out.dtype != torch.uint8 or not out.is_contiguous() or out.dim() != 1 or out.numel() < batch.out_bytes or out.device != dev:
            raise ValueError(f"png_decode: out must be a flat contiguous uint8 tensor of at least {batch.out_bytes} elements on {dev}")
        status = torch.empty(n, dtype=torch.int32, device=dev)
        ws = _ws(batch.ws_bytes, dev)
        _lib.check(lib.tt_png_decode_batch(meta.data_ptr() + batch.layout["streams"][0], batch.layout["streams"][1], table.ctypes.data,
                                           meta.data_ptr(), n, _p(out), out.numel(), _p(ws), ws.numel(), _p(status), _stream()),
                   "tt_png_decode_batch")
        host_status = _file_status(status, _PNG, (lambda rc: rc != 0) if check else None)
    return _png_views(out, table), host_status


def decode_png_batch(files: Sequence[bytes], device=None, threads: int = 8):
    """Annotation PNG files -> uint8 [H, W] GPU label maps, bit-equal to ``np.asarray(Image.open(...))``; views of one flat buffer in file
    order.  Unsupported files raise PngUnsupported (no CPU fallback here), broken ones ValueError."""
    return png_decode(png_prepare_batch(files, threads, True), device)[0]


# ---- N29: label maps written as palette PNGs.  The device half (tt_png_encode_batch: Up filter, run tokens, fixed-Huffman bits, one
# workgroup per band of rows, then a scan and a gather) leaves ONE compact buffer of streams; the host half (tt_png_write_file: signature,
# IHDR, PLTE, one IDAT, IEND - a pure host function that ctypes runs without the GIL) wraps them into files in the thread pool the decode
# batches use.  The byte format: csrc/png_deflate.hpp.
_PNG_MAP = np.dtype([("data", "<u8"), ("H", "<i8"), ("W", "<i8"), ("pitch", "<i8"), ("first_chunk", "<i8"), ("n_chunks", "<i8"),
                     ("out_off", "<i8"), ("reserved", "<i8")])                                                          # tt_png_map
_PNG_CHUNK = np.dtype([("map", "<i8"), ("row0", "<i8"), ("rows", "<i8"), ("slot_off", "<i8")])                        # tt_png_chunk
_PNG_RESULT = np.dtype([("offset", "<i8"), ("length", "<i8"), ("adler", "<i8"), ("reserved", "<i8")])                 # tt_png_result


class PngEncodePlan(_FileBatch):
    """The tables of a batch of maps to encode: ONE (pinned) buffer ``meta`` with its parts 'maps' (tt_png_map rows) and 'chunks'
    (tt_png_chunk rows); ``out_bytes``: the capacity the output needs, ``ws_bytes``: the workspace.  ``maps`` keeps the tensors or arrays
    the rows point into."""

    def __init__(self, maps, meta, layout, n_chunks, out_bytes, ws_bytes):
        self.maps, self.meta, self.layout, self.n_chunks, self.out_bytes, self.ws_bytes = maps, meta, layout, n_chunks, out_bytes, ws_bytes

    @property
    def table(self):
        return self.part("maps").view(_PNG_MAP)

    @property
    def chunks(self):
        return self.part("chunks").view(_PNG_CHUNK)


def _png_map_list(maps, who: str) -> list:
    """One [k, H, W] / [H, W] tensor or array, or a sequence of [H, W] ones -> a list of 2-D maps (views)."""
    if isinstance(maps, (torch.Tensor, np.ndarray)):
        if maps.ndim == 2:
            return [maps]
        if maps.ndim != 3:
            raise ValueError(f"{who}: expected [H, W] maps or one [k, H, W] stack, got {tuple(maps.shape)}")
        maps = [maps[i] for i in range(maps.shape[0])]
    maps = list(maps)
    if not maps:
        raise ValueError(f"{who}: no maps")
    for i, m in enumerate(maps):
        if not isinstance(m, (torch.Tensor, np.ndarray)) or m.ndim != 2:
            raise ValueError(f"{who}: map {i} is not a 2-D tensor or array")
        if m.shape[0] < 1 or m.shape[1] < 1 or m.shape[0] > 32767 or m.shape[1] > 32767:
            raise ValueError(f"{who}: map {i} is {m.shape[0]} x {m.shape[1]}: both sides must be in 1..32767")
    return maps


def _png_rows(m):
    """A uint8 [H, W] map whose rows are contiguous and at least W bytes apart (a view where it is one already), and that pitch."""
    if isinstance(m, torch.Tensor):
        s0, s1 = m.stride()
        if (s1 != 1 and m.shape[1] > 1) or (s0 < m.shape[1] and m.shape[0] > 1):
            m = m.contiguous()
        return m, (int(m.stride(0)) if m.shape[0] > 1 else int(m.shape[1]))
    s0, s1 = m.strides
    if (s1 != 1 and m.shape[1] > 1) or (s0 < m.shape[1] and m.shape[0] > 1):
        m = np.ascontiguousarray(m)
    return m, (int(m.strides[0]) if m.shape[0] > 1 else int(m.shape[1]))


def _png_uint8_maps(maps: list, who: str) -> list:
    """Integer maps as uint8, by a CHECKED conversion: a value outside 0..255 raises ValueError naming the map (one read-back of the
    extrema of the maps that are not uint8 already)."""
    maps = list(maps)
    wide = []            # the maps whose values have to be looked at: integer, not uint8, not bool
    for i, m in enumerate(maps):
        dt, tensor = m.dtype, isinstance(m, torch.Tensor)
        if dt in (torch.uint8, np.dtype(np.uint8)):
            continue
        if (dt.is_floating_point or dt.is_complex) if tensor else dt.kind not in "iub":
            raise TypeError(f"{who}: map {i} is {dt}: label maps must be integer")
        if dt not in (torch.bool, np.dtype(bool)):
            wide.append(i)
    on_gpu = [i for i in wide if isinstance(maps[i], torch.Tensor)]
    extrema = {i: (int(maps[i].min()), int(maps[i].max())) for i in wide if i not in on_gpu}
    if on_gpu:
        host = torch.stack([torch.stack([maps[i].min(), maps[i].max()]).long() for i in on_gpu]).cpu().tolist()
        extrema.update(zip(on_gpu, host))
    for i in wide:
        lo, hi = extrema[i]
        if lo < 0 or hi > 255:
            raise ValueError(f"{who}: map {i} holds values in {lo}..{hi}: an 8-bit PNG takes 0..255")
    return [m if m.dtype in (torch.uint8, np.dtype(np.uint8)) else (m.to(torch.uint8) if isinstance(m, torch.Tensor) else m.astype(np.uint8)) for m in maps]


def png_encode_plan(maps, pin: bool = True) -> PngEncodePlan:
    """The tables of tt_png_encode_plan for uint8 [H, W] maps (GPU tensors for ``png_encode``, NumPy arrays for ``png_encode_host``; a
    pitched view - rows of a wider tensor - is taken as it is), in one (pinned) buffer."""
    lib = _lib.load()
    maps = _png_map_list(maps, "png_encode_plan")
    rows = [_png_rows(m) for m in maps]
    n = len(rows)
    table = np.zeros(n, _PNG_MAP)
    for i, (m, pitch) in enumerate(rows):
        if m.dtype not in (torch.uint8, np.dtype(np.uint8)):
            raise TypeError(f"png_encode_plan: map {i} is {m.dtype}, expected uint8")
        table[i]["data"] = m.data_ptr() if isinstance(m, torch.Tensor) else m.ctypes.data
        table[i]["H"], table[i]["W"], table[i]["pitch"] = m.shape[0], m.shape[1], pitch
    n_chunks, cap = C.c_longlong(), C.c_longlong()
    rc = lib.tt_png_encode_plan(table.ctypes.data, n, None, 0, C.byref(n_chunks), C.byref(cap))
    if rc != 0:
        raise ValueError(f"png_encode_plan: the maps were refused (status {rc}: {PNG_MALFORMED.get(rc, 'unknown')})")
    layout, size = _layout([("maps", n * _PNG_MAP.itemsize), ("chunks", n_chunks.value * _PNG_CHUNK.itemsize)])
    meta = torch.zeros(size, dtype=torch.uint8, pin_memory=pin)
    host = meta.numpy()
    host[:layout["maps"][1]] = table.view(np.uint8)
    rc = lib.tt_png_encode_plan(meta.data_ptr(), n, meta.data_ptr() + layout["chunks"][0], n_chunks.value, C.byref(n_chunks), C.byref(cap))
    assert rc == 0
    ws_bytes = int(lib.tt_png_encode_batch_workspace_bytes(meta.data_ptr(), n))
    return PngEncodePlan([m for m, _ in rows], meta, layout, int(n_chunks.value), int(cap.value), ws_bytes)


def _png_streams(flat: np.ndarray, results: np.ndarray):
    return [flat[int(r["offset"]):int(r["offset"]) + int(r["length"])] for r in results], results["adler"].astype(np.uint32)


def png_encode_host(maps):
    """The host emulation of the device encoder (tt_png_encode_host: the sequential loop over the kernels' steps) on NumPy maps, for tests
    and tools: (the streams as uint8 views of one flat array in map order, their Adler-32 uint32 [n])."""
    lib = _lib.load()
    maps = _png_uint8_maps([np.asarray(m) for m in _png_map_list(maps, "png_encode_host")], "png_encode_host")
    plan = png_encode_plan(maps, pin=False)
    n = len(plan.maps)
    table, chunks = plan.table, plan.chunks
    out, results = np.zeros(max(plan.out_bytes, 1), np.uint8), np.zeros(n, _PNG_RESULT)
    ws = np.zeros(plan.ws_bytes // 16 + 2, np.dtype("<u8, <u8"))
    at = ws.ctypes.data + (-ws.ctypes.data) % 16
    rc = lib.tt_png_encode_host(table.ctypes.data, None, n, chunks.ctypes.data, None, plan.n_chunks, out.ctypes.data, plan.out_bytes,
                                results.ctypes.data, at, plan.ws_bytes, None)
    if rc != 0:
        raise ValueError(f"png_encode_host: refused (status {rc})")
    return _png_streams(out, results)


def png_encode(maps, device=None):
    """The device half: uint8 [H, W] GPU maps (or one [k, H, W] stack; mixed sizes and pitched views in one call) -> (the deflate streams
    as uint8 NumPy views of one flat array in map order, their Adler-32 uint32 [n]).  One host-to-device copy of the tables, the three
    launches of tt_png_encode_batch on the current stream, and exactly TWO read-backs: the result table (32 bytes per map), then exactly
    the streams' bytes - the maps themselves never cross the bus."""
    lib = _lib.load()
    maps = _png_map_list(maps, "png_encode")
    for i, m in enumerate(maps):
        if not isinstance(m, torch.Tensor) or not m.is_cuda:
            raise _lib.HipLibraryError(f"png_encode: map {i}: expected a tensor in GPU memory (the HIP path has no CPU fallback)")
    dev = _need_gpu("png_encode", maps[0].device if device is None else device)
    if any(m.device != dev for m in maps):
        raise ValueError(f"png_encode: every map must be on {dev}")
    plan = png_encode_plan(_png_uint8_maps(maps, "png_encode"))
    n = len(plan.maps)
    with torch.cuda.device(dev):
        meta = plan.meta.to(dev, non_blocking=True)
        out = torch.empty(max(plan.out_bytes, 16), dtype=torch.uint8, device=dev)
        results = torch.empty(n * _PNG_RESULT.itemsize, dtype=torch.uint8, device=dev)
        ws = _ws(plan.ws_bytes, dev)
        rc = lib.tt_png_encode_batch(plan.table.ctypes.data, meta.data_ptr() + plan.layout["maps"][0], n, plan.chunks.ctypes.data,
                                     meta.data_ptr() + plan.layout["chunks"][0], plan.n_chunks, _p(out), out.numel(), _p(results), _p(ws),
                                     ws.numel(), _stream())
        _lib.check(rc, "tt_png_encode_batch")
        table = results.cpu().numpy().view(_PNG_RESULT)                                   # read-back 1
        total = int(table["offset"][-1] + table["length"][-1])
        flat = out[:total].cpu().numpy()                                                  # read-back 2
    return _png_streams(flat, table)


def _png_palette(palette, who: str):
    if palette is None:
        return None
    pal = np.ascontiguousarray(palette.cpu().numpy() if isinstance(palette, torch.Tensor) else np.asarray(palette))
    if pal.ndim != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= 256 or pal.dtype != np.uint8:
        raise ValueError(f"{who}: the palette must be uint8 [n, 3] with 1 <= n <= 256, got {pal.dtype} {tuple(pal.shape)}")
    return pal


def png_wrap_files(streams, adlers, shapes, palette=None, threads: int = 8) -> list:
    """The finished files around device-made streams (tt_png_write_file), in the thread pool: ``shapes`` [(H, W)] per stream; ``palette``
    uint8 [n, 3] (mode P) or None (mode L)."""
    lib = _lib.load()
    pal = _png_palette(palette, "png_wrap_files")
    entries = 0 if pal is None else pal.shape[0]
    streams = [np.ascontiguousarray(s) for s in streams]

    def wrap(i):
        cap = int(lib.tt_png_file_bytes(streams[i].size, entries))
        buf, n = np.empty(cap, np.uint8), C.c_size_t()
        rc = lib.tt_png_write_file(streams[i].ctypes.data, streams[i].size, int(adlers[i]), int(shapes[i][0]), int(shapes[i][1]),
                                   None if pal is None else pal.ctypes.data, entries, buf.ctypes.data, cap, C.byref(n))
        return rc, buf[:n.value].tobytes()

    done = _each_file(wrap, len(streams), threads, lambda rc, i: ValueError(f"png_wrap_files: file {i} was refused (status {rc})"), lambda r: r[0])
    return [data for _, data in done]


def encode_png_batch(maps, palette=None, device=None, threads: int = 8) -> list:
    """Label maps on the GPU -> finished PNG files (``bytes``), one per map: palette files (mode P) with ``palette`` uint8 [n, 3], gray
    files (mode L) without.  Maps: contiguous-row uint8 [H, W] GPU tensors of any mix of sizes, or one [k, H, W] tensor; other integer
    dtypes convert (a value outside 0..255: ValueError naming the map).  Pixel-equal to what Pillow would write, not byte-equal.  CPU
    tensors are refused."""
    maps = _png_map_list(maps, "encode_png_batch")
    _png_palette(palette, "encode_png_batch")
    streams, adlers = png_encode(maps, device)
    return png_wrap_files(streams, adlers, [tuple(m.shape) for m in maps], palette, threads)


# ------------------------------------------------------------------------------------------------
# N31: dense nearest-neighbour retrieval (csrc/nn_retrieval.hip)
# ------------------------------------------------------------------------------------------------

NN_MAX_K = 64
NN_SEARCH_WORKSPACE_BYTES = 64 << 20     # one block of similarities; DESIGN.md N31 has the measurement behind the default
NN_SEARCH_QUERY_TILE = 4096              # queries per block: one wave each, enough of them to fill the device


def _chk_topk_lists(vals, idx, Q: int, k: int, device, who: str) -> None:
    _chk(vals, "vals"); _chk(idx, "idx", torch.int64)
    if tuple(vals.shape) != (Q, k) or tuple(idx.shape) != (Q, k) or vals.device != device or idx.device != device:
        raise ValueError(f"{who}: vals and idx must be [{Q}, {k}] on {device}, got {tuple(vals.shape)} and {tuple(idx.shape)}")


def topk_merge(sims, base: int, vals=None, idx=None, k: Optional[int] = None, init: Optional[bool] = None):
    """One step of the exact top-k search.  sims fp32 [Q, Nc] (rows may be pitched: ``stride(1) == 1``, any ``stride(0) >= Nc``, any
    4-byte-aligned start): the similarities of Q queries to bank rows ``base .. base + Nc - 1``.  ``vals`` fp32 [Q, k] / ``idx`` int64
    [Q, k]: the running lists, replaced IN PLACE by the k best of (list U block); without them (pass ``k``) the search starts from
    empty lists, and so it does with ``init=True`` (the lists' contents are then not read).  Order: larger similarity first, then smaller bank index; NaN and -inf are never selected; a list that has seen fewer
    than k finite candidates ends in (-inf, -1).  Returns ``(vals, idx)``."""
    lib = _lib.load()
    if sims.dim() != 2 or not sims.is_cuda or sims.dtype != f32 or sims.shape[0] < 1 or sims.shape[1] < 1:
        raise ValueError("topk_merge: sims must be a non-empty 2-D fp32 GPU tensor")
    Q, Nc = sims.shape
    ld = sims.stride(0) if Q > 1 else max(sims.stride(0), Nc)
    if sims.stride(1) != 1 or ld < Nc:
        raise ValueError(f"topk_merge: sims must have unit inner stride and rows at least Nc = {Nc} apart, got strides {sims.stride()}")
    fresh = vals is None and idx is None
    init = fresh if init is None else bool(init)
    if fresh:
        if not init:
            raise ValueError("topk_merge: init=False needs the running lists")
        if k is None:
            raise ValueError("topk_merge: pass the running lists (vals, idx), or k to start from empty ones")
        k = int(k)
        if not 1 <= k <= NN_MAX_K:
            raise ValueError(f"topk_merge: k = {k} is outside 1 .. {NN_MAX_K}")
        vals = torch.empty((Q, k), dtype=f32, device=sims.device)
        idx = torch.empty((Q, k), dtype=torch.int64, device=sims.device)
    elif vals is None or idx is None:
        raise ValueError("topk_merge: vals and idx come together")
    else:
        if k is not None and int(k) != vals.shape[1]:
            raise ValueError(f"topk_merge: k = {k}, the lists hold {vals.shape[1]} entries")
        k = int(vals.shape[1])
    _chk_topk_lists(vals, idx, Q, k, sims.device, "topk_merge")
    with torch.cuda.device(sims.device):
        _lib.check(lib.tt_topk_merge(_p(sims), Q, Nc, ld, int(base), _p(vals), _p(idx), k, 1 if init else 0, _stream()), "tt_topk_merge")
    return vals, idx


def patch_label_counts(maps, grid: int, num_classes: int, ignore: Optional[int] = 255, check: bool = True):
    """maps uint8 [M, R, R] -> ``(counts int32 [M, g*g, C], valid int32 [M, g*g])``: the pixels of every class in every cell of the g x g grid,
    and their sum.  Pixels equal to ``ignore`` (None: no such value) count nowhere.  A label >= C that is not ``ignore`` raises ValueError
    naming the first such map (``check=True`` reads the status word: one device-to-host copy; ``check=False`` returns
    ``(counts, valid, status)`` with the device word, 0xffffffff = -1 when every label was in range)."""
    lib = _lib.load()
    _chk(maps, "maps", torch.uint8)
    if maps.dim() != 3 or maps.shape[1] != maps.shape[2]:
        raise ValueError(f"patch_label_counts: expected uint8 [M, R, R], got {tuple(maps.shape)}")
    M, R = int(maps.shape[0]), int(maps.shape[1])
    g, Cn, ign = int(grid), int(num_classes), (-1 if ignore is None else int(ignore))
    if not lib.tt_patch_label_counts_shape_ok(M, R, g, Cn):
        raise ValueError(f"patch_label_counts: {M} maps of {R} x {R} on a grid of {g} with {Cn} classes are not supported "
                         f"(need R % g == 0, R <= 16384, 1 <= C <= 256)")
    counts = torch.empty((M, g * g, Cn), dtype=torch.int32, device=maps.device)
    valid = torch.empty((M, g * g), dtype=torch.int32, device=maps.device)
    status = torch.empty((1,), dtype=torch.int32, device=maps.device)
    with torch.cuda.device(maps.device):
        _lib.check(lib.tt_patch_label_counts(_p(maps), M, R, g, Cn, ign, _p(counts), _p(valid), _p(status), _stream()), "tt_patch_label_counts")
    if not check:
        return counts, valid, status
    bad = int(status.item())
    if bad >= 0:
        raise ValueError(f"patch_label_counts: map {bad} holds a label outside [0, {Cn}) that is not the ignore value {ignore}")
    return counts, valid


def nn_label_aggregate(vals, idx, labels, beta: float, out=None):
    """``out[q] = sum_j softmax(vals[q] / beta)_j * labels[idx[q, j]]`` over the entries with ``idx >= 0``: vals fp32 [Q, k], idx int64 [Q, k],
    labels fp32 [N, C] -> fp32 [Q, C]; a query with no valid entry gets a zero row."""
    lib = _lib.load()
    _chk(labels, "labels")
    if vals.dim() != 2 or labels.dim() != 2:
        raise ValueError(f"nn_label_aggregate: expected vals [Q, k] and labels [N, C], got {tuple(vals.shape)} and {tuple(labels.shape)}")
    Q, k = vals.shape
    N, Cn = labels.shape
    _chk_topk_lists(vals, idx, Q, k, labels.device, "nn_label_aggregate")
    if not lib.tt_nn_label_aggregate_shape_ok(Q, k, N, Cn) or not float(beta) > 0:
        raise ValueError(f"nn_label_aggregate: Q = {Q}, k = {k}, N = {N}, C = {Cn}, beta = {beta} are not supported (1 <= k <= {NN_MAX_K}, beta > 0)")
    if out is None:
        out = torch.empty((Q, Cn), dtype=f32, device=labels.device)
    else:
        _chk(out, "out")
        if tuple(out.shape) != (Q, Cn):
            raise ValueError(f"nn_label_aggregate: out must be [{Q}, {Cn}]")
    with torch.cuda.device(labels.device):
        _lib.check(lib.tt_nn_label_aggregate(_p(vals), _p(idx), _p(labels), Q, k, N, Cn, float(beta), _p(out), _stream()), "tt_nn_label_aggregate")
    return out


def nn_search_plan(Q: int, N: int, workspace_bytes: int = NN_SEARCH_WORKSPACE_BYTES, query_tile: int = NN_SEARCH_QUERY_TILE) -> list:
    """Host only: the blocks ``(q0, q1, n0, n1)`` of ``nn_search``, in the order it runs them.  A block is at most ``query_tile`` queries by as
    many bank rows as ``workspace_bytes`` of fp32 similarities hold beside them; every (query, bank row) pair lies in exactly one block."""
    Q, N, floats = int(Q), int(N), int(workspace_bytes) // 4
    if Q < 1 or N < 1 or floats < 1 or int(query_tile) < 1:
        raise ValueError(f"nn_search_plan: Q = {Q}, N = {N}, workspace_bytes = {workspace_bytes}, query_tile = {query_tile}: need each >= 1 "
                         "(the workspace at least one fp32)")
    rows = min(Q, int(query_tile), floats)
    cols = min(N, floats // rows, 2 ** 31 - 1)
    return [(q0, min(q0 + rows, Q), n0, min(n0 + cols, N)) for q0 in range(0, Q, rows) for n0 in range(0, N, cols)]


def _nn_select_torch(block, base: int, vals, idx, k: int):
    """``select="torch"``: what a user of torch alone writes - top-k of the block, concatenated with the running list, top-k again."""
    bv, bi = torch.topk(block, min(k, block.shape[1]), dim=1)
    bi = bi + base
    if vals is not None:
        bv, bi = torch.cat([vals, bv], dim=1), torch.cat([idx, bi], dim=1)
    if bv.shape[1] > k:
        bv, at = torch.topk(bv, k, dim=1)
        bi = torch.gather(bi, 1, at)
    return bv, bi


def _nn_canonical_torch(vals, idx, k: int):
    """The torch route's lists in the order tt_topk_merge keeps: similarity descending, then index ascending; padded with (-inf, -1)."""
    idx, order = torch.sort(idx, dim=1, stable=True)
    vals = torch.gather(vals, 1, order)
    vals, order = torch.sort(vals, dim=1, descending=True, stable=True)
    idx = torch.gather(idx, 1, order)
    if vals.shape[1] < k:
        pad = k - vals.shape[1]
        vals = torch.cat([vals, vals.new_full((vals.shape[0], pad), float("-inf"))], dim=1)
        idx = torch.cat([idx, idx.new_full((idx.shape[0], pad), -1)], dim=1)
    return vals.contiguous(), idx.contiguous()


def nn_search(queries, bank, k: int, workspace_bytes: int = NN_SEARCH_WORKSPACE_BYTES, select: str = "hip", query_tile: int = NN_SEARCH_QUERY_TILE,
              workspace=None):
    """Exact k nearest bank rows of every query by inner product (cosine similarity on L2-normalised rows): queries fp32 [Q, D], bank fp32
    [N, D] -> ``(vals fp32 [Q, k], idx int64 [Q, k])``, best first, ties by the smaller bank index.  The [Q, N] similarities are never held
    whole: block by block (``nn_search_plan``) ``linear_fwd`` writes queries x bank-block^T into the workspace and the select merges it into
    the running lists.  ``select="hip"``: tt_topk_merge.  ``select="torch"``: the same tiling with torch.topk on the block and
    cat + topk for the merge - the A/B partner on finite similarities, not a fallback.  ``workspace``: a uint8 GPU tensor of at least
    ``workspace_bytes`` to reuse between calls."""
    _chk(queries, "queries"); _chk(bank, "bank")
    if queries.dim() != 2 or bank.dim() != 2 or queries.shape[1] != bank.shape[1] or queries.device != bank.device:
        raise ValueError(f"nn_search: expected queries [Q, D] and bank [N, D] on one device, got {tuple(queries.shape)} and {tuple(bank.shape)}")
    if select not in ("hip", "torch"):
        raise ValueError(f"nn_search: select = {select!r} is neither 'hip' nor 'torch'")
    k = int(k)
    if not 1 <= k <= NN_MAX_K:
        raise ValueError(f"nn_search: k = {k} is outside 1 .. {NN_MAX_K}")
    Q, N = int(queries.shape[0]), int(bank.shape[0])
    plan = nn_search_plan(Q, N, workspace_bytes, query_tile)
    need = 4 * max((q1 - q0) * (n1 - n0) for q0, q1, n0, n1 in plan)
    if workspace is None:
        workspace = _ws(need, queries.device)
    elif workspace.dtype != torch.uint8 or not workspace.is_cuda or not workspace.is_contiguous() or workspace.numel() < need \
            or workspace.data_ptr() % 16:
        raise ValueError(f"nn_search: workspace must be a contiguous, 16-byte-aligned uint8 GPU tensor of at least {need} bytes")
    floats = workspace[: need].view(f32)
    vals = torch.empty((Q, k), dtype=f32, device=queries.device)
    idx = torch.empty((Q, k), dtype=torch.int64, device=queries.device)
    done = None
    for q0, q1, n0, n1 in plan:
        block = linear_fwd(queries[q0:q1], bank[n0:n1], out=floats[: (q1 - q0) * (n1 - n0)].view(q1 - q0, n1 - n0))
        first = n0 == 0
        if select == "hip":
            topk_merge(block, n0, vals[q0:q1], idx[q0:q1], init=first)
        else:
            done = _nn_select_torch(block, n0, None if first else done[0], None if first else done[1], k)
            if n1 == N:
                v, i = _nn_canonical_torch(done[0], done[1], k)
                vals[q0:q1], idx[q0:q1] = v, i
    return vals, idx
