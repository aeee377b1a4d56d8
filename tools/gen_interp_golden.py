#!/usr/bin/env python3
"""Writes tests/golden/interp_bits.npz: the BITS of every kernel that takes its taps or weights from csrc/interp.hpp (N30), recorded
from the library built at the commit BEFORE the rules were gathered there:

    TT_LIB_PATH=<the parent commit's libtimetuning_hip.so> python tools/gen_interp_golden.py        # on the GPU

The tool calls only entries both trees have, through timetuning_amd.hip_ops.  tests/test_hip_interp_bits.py loads this file, runs
``compute`` on the tree under test and asserts torch.equal against the stored arrays: a refactor of the rule that changes one
rounding - a hoisted scale, a literal of the other type, a reordered product - changes a stored bit.

The inputs are not stored: ``synth.normal`` makes them from (name, seed, shape).  Every arg-max case runs on three maps: normal
values; the same values rounded to multiples of 1/4 (exact ties: the first index must win); a constant map.

The file is written only if
  * every entry, run twice, gave identical results;
  * the rounded maps produced, for every arg-max kernel, at least one pixel whose two largest interpolated values are equal (fp64
    F.interpolate of the rounded map, where every product and sum of the cases' weights is exact enough to tie);
  * the labels of the normal maps differ from the arg-max of the fp64 F.interpolate at no pixel whose two largest values are more than
    4 ulp of the kernel's arithmetic type apart (stock torch's fp32 interpolation meets the same condition: ``--self-check``, CPU).
"""
from __future__ import annotations

import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "interp_bits.npz")
SEED = 30

TOKENS = ((2, 3, 8, 65), (1, 5, 3, 7), (1, 1, 4, 1), (1, 2, 5, 256))    # (M, g, R, C): workgroups of 128, 64, 64, 256; down-sampling; g = 1
ARGMAX64 = ((2, 3, 17, 5), (1, 6, 4, 2), (1, 1, 3, 1))                  # (M, g, R, K): 289 pixels are two workgroups
ARGMAX_HW = (((3, 5), (17, 9)), ((5, 3), (2, 20)), ((1, 4), (1, 1)))    # (gh, gw) -> (H, W), K = 5, M = 2
ARGMAX32 = ((2, 3, 17, 5), (1, 6, 4, 65))                               # (M, g, R, K), the histogram on the same maps
ADJOINT = ((2, 3, 8, 5), (1, 4, 3, 9))                                  # (B, g, R, C)
POS_EMBED = ((14, 9, 20, 8), (14, 14, 15, 8))                           # (g, gh, gw, D)
KINDS = ("normal", "ties", "const")


def _maps(name, shape, kind, dtype):
    """[M, n, K] maps of one arg-max case."""
    from timetuning_amd import synth

    x = synth.normal(name, shape, seed=SEED).astype(dtype)
    if dtype == np.float64:   # mantissa bits below fp32's
        x = x + synth.normal(name + ".lo", shape, seed=SEED).astype(np.float64) * 2.0 ** -26
    if kind == "ties":
        return (np.round(synth.normal(name, shape, seed=SEED) * 4) / 4).astype(dtype)
    if kind == "const":
        return np.full(shape, 0.5, dtype)
    return x


def argmax_cases():
    """(key, entry, maps, (gh, gw), (H, W)) of every arg-max run."""
    for M, g, R, K in ARGMAX64:
        for kind in KINDS:
            yield f"argmax64/{M}_{g}_{R}_{K}/{kind}", "f64", _maps(f"interp.a64.{g}.{R}", (M, g * g, K), kind, np.float64), (g, g), (R, R)
    for (gh, gw), (H, W) in ARGMAX_HW:
        for kind in KINDS:
            yield (f"argmax_hw/{gh}x{gw}_{H}x{W}/{kind}", "hw", _maps(f"interp.hw.{gh}.{gw}", (2, gh * gw, 5), kind, np.float64), (gh, gw),
                   (H, W))
    for M, g, R, K in ARGMAX32:
        for kind in KINDS:
            yield f"argmax32/{M}_{g}_{R}_{K}/{kind}", "f32", _maps(f"interp.a32.{g}.{R}", (M, g * g, K), kind, np.float32), (g, g), (R, R)


def compute(ops, device="cuda"):
    """name -> array: every recorded result, from the library ``ops`` has loaded."""
    import torch

    from timetuning_amd import synth

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)

    def host(t):
        return t.detach().cpu().numpy()

    out = {}
    for M, g, R, C in TOKENS:
        x = synth.normal(f"interp.tok.{g}.{R}", (M, g * g, C), seed=SEED)
        out[f"tokens/{M}_{g}_{R}_{C}"] = host(ops.upsample_bilinear_tokens(dev(x), R))
    for key, entry, maps, (gh, gw), (H, W) in argmax_cases():
        m = dev(maps)
        if entry == "f64":
            out[key] = host(ops.upsample_argmax(m, H)).astype(np.int16)
        elif entry == "hw":
            out[key] = host(ops.upsample_argmax_hw(m, (gh, gw), (H, W))).astype(np.int16)
        else:
            out[key] = host(ops.upsample_argmax_f32(m, H)).astype(np.int16)
            K = maps.shape[2]
            out[key + "/hist"] = host(ops.upsample_argmax_hist(m, H))
            start = dev(np.arange(1, K + 1, dtype=np.int64) * 1000003)      # added onto non-zero counts
            out[key + "/hist_added"] = host(ops.upsample_argmax_hist(m, H, start))
    for B, g, R, C in ADJOINT:
        d_hi = synth.normal(f"interp.adj.{g}.{R}", (B, R * R, C), seed=SEED)
        out[f"adjoint/{B}_{g}_{R}_{C}"] = host(ops.bilinear_adjoint_tokens(dev(d_hi), g))
        logits = synth.normal(f"interp.ce.{g}.{R}", (B, g * g, C), seed=SEED)
        labels = (np.abs(synth.normal(f"interp.ce.y.{g}.{R}", (B, R, R), seed=SEED)) * 3).astype(np.int64) % C
        labels[:, ::3, 1::2] = 255
        loss, dlow, counts = ops.probe_upsample_ce(dev(logits), dev(labels))
        out[f"probe_ce/{B}_{g}_{R}_{C}/loss"], out[f"probe_ce/{B}_{g}_{R}_{C}/dlow"] = host(loss), host(dlow)
        out[f"probe_ce/{B}_{g}_{R}_{C}/counts"] = host(counts)
    for g, gh, gw, D in POS_EMBED:
        pos = synth.normal(f"interp.pos.{g}", (1 + g * g, D), seed=SEED)
        dtable = synth.normal(f"interp.dtable.{gh}.{gw}", (1 + gh * gw, D), seed=SEED)
        out[f"pos_embed/{g}_{gh}_{gw}_{D}"] = host(ops.pos_embed_interpolate(dev(pos), gh, gw))
        out[f"pos_embed_bwd/{g}_{gh}_{gw}_{D}"] = host(ops.pos_embed_interpolate_bwd(dev(dtable), g, gh, gw))
    return out


def reference_top2(maps, grid, size):
    """The two largest fp64 F.interpolate values per pixel and the first arg-max: (top [M, 2, H, W] or None at K = 1, labels)."""
    import torch
    import torch.nn.functional as F

    M, n, K = maps.shape
    x = torch.from_numpy(maps.astype(np.float64)).view(M, grid[0], grid[1], K).permute(0, 3, 1, 2)
    up = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
    return (up.topk(2, dim=1).values if K > 1 else None), up.argmax(1)


def check_against_fp64(results, label_of=None):
    """The two conditions on the arg-max results (``label_of``: what stands in for the recorded labels - the self-check's torch)."""
    import torch

    ties = {"f64": 0, "hw": 0, "f32": 0}
    for key, entry, maps, grid, size in argmax_cases():
        top, ref = reference_top2(maps, grid, size)
        kind = key.rsplit("/", 1)[1]
        if kind == "ties" and top is not None:
            ties[entry] += int((top[:, 0] == top[:, 1]).sum())
        if kind == "normal":
            got = torch.from_numpy((label_of(maps, grid, size) if label_of else results[key]).astype(np.int64))
            differ = got != ref
            if top is not None and bool(differ.any()):
                eps = np.finfo(np.float32 if entry == "f32" else np.float64).eps
                gap = (top[:, 0] - top[:, 1]) / (eps * top[:, 0].abs().clamp_min(np.finfo(np.float64).tiny))
                assert bool((gap[differ] <= 4).all()), f"{key}: a label differs from the fp64 arg-max across a gap of {float(gap[differ].max()):.1f} ulp"
            else:
                assert not bool(differ.any()), key
    assert all(v > 0 for v in ties.values()), f"the rounded maps tie at {ties} pixels: every arg-max kernel needs at least one"
    return ties


def self_check():
    """CPU: stock torch's own interpolation (fp32 for the fp32 entry) in place of the kernels meets the two conditions."""
    import torch
    import torch.nn.functional as F

    def torch_labels(maps, grid, size):
        M, n, K = maps.shape
        x = torch.from_numpy(maps).view(M, grid[0], grid[1], K).permute(0, 3, 1, 2)
        return F.interpolate(x, size=size, mode="bilinear", align_corners=False).argmax(1).numpy()

    print("self-check ok, tie pixels per kernel:", check_against_fp64(None, torch_labels))


def main():
    if "--self-check" in sys.argv:
        return self_check()
    from timetuning_amd import _lib
    from timetuning_amd import hip_ops as ops

    first, second = compute(ops), compute(ops)
    assert first.keys() == second.keys()
    for k in first:
        assert first[k].dtype == second[k].dtype and np.array_equal(first[k], second[k]), f"{k}: two runs differ"
    ties = check_against_fp64(first)
    np.savez_compressed(OUT, **first)
    print(f"{OUT} written from {_lib.LIB_PATH}: {len(first)} arrays, {os.path.getsize(OUT)} bytes, tie pixels {ties}")


if __name__ == "__main__":
    main()
