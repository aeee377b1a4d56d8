#!/usr/bin/env python
"""N31: the dense nearest-neighbour search, ``select="hip"`` (tt_topk_merge) against ``select="torch"`` (torch.topk on the block, cat +
topk for the merge) on the same blocks, alternating inside each repetition, HIP events after a warm-up, medians.  The GEMM blocks and the
select are timed apart; the select's achieved bytes per second (4 bytes per similarity read) are reported per workspace size, which is
what measures whether a block written by the GEMM is still cache-resident when the select reads it.

The VOC-sized problem is Q = 1 449 x 784 queries against a bank of 10 582 x 784 rows at D = 384, k = 30: 9.4e12 similarities, minutes
per route.  The default runs a FRACTION of it - the patches of ``--val_images`` validation images against those of ``--bank_images``
training images - and scales the times by the ratio of similarities; the cost per similarity does not depend on the fraction once the
bank is many blocks long (every block is a full one but the last).

    python tools/bench_nn_retrieval.py [--val_images 16] [--bank_images 1323] [--workspace_mb 16 64 256] [--reps 5] [--warmup 2]
                                       [--out profiles/n31_nn_retrieval.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from timetuning_amd import hip_ops as ops  # noqa: E402

PATCHES, D, K = 784, 384, 30
FULL_Q, FULL_N = 1449 * PATCHES, 10582 * PATCHES


def unit_rows(n, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    out = torch.empty((n, D), dtype=torch.float32, device=dev)
    for r0 in range(0, n, 1 << 18):
        x = torch.randn((min(1 << 18, n - r0), D), generator=g, device=dev)
        out[r0:r0 + x.shape[0]] = torch.nn.functional.normalize(x, dim=1)
    return out


def run(queries, bank, select, plan, floats, timed):
    """One search on the given plan; returns (vals, idx, gemm ms, select ms) with the two parts from HIP events around every block."""
    Q = queries.shape[0]
    vals = torch.empty((Q, K), dtype=torch.float32, device=queries.device)
    idx = torch.empty((Q, K), dtype=torch.int64, device=queries.device)
    events, done = [], None
    for q0, q1, n0, n1 in plan:
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timed else None
        if timed:
            e[0].record()
        block = ops.linear_fwd(queries[q0:q1], bank[n0:n1], out=floats[: (q1 - q0) * (n1 - n0)].view(q1 - q0, n1 - n0))
        if timed:
            e[1].record()
        if select == "hip":
            ops.topk_merge(block, n0, vals[q0:q1], idx[q0:q1], init=n0 == 0)
        else:
            done = ops._nn_select_torch(block, n0, None if n0 == 0 else done[0], None if n0 == 0 else done[1], K)
            if n1 == bank.shape[0]:
                vals[q0:q1], idx[q0:q1] = ops._nn_canonical_torch(done[0], done[1], K)
        if timed:
            e[2].record()
            events.append(e)
    torch.cuda.synchronize()
    gemm = sum(e[0].elapsed_time(e[1]) for e in events)
    sel = sum(e[1].elapsed_time(e[2]) for e in events)
    return vals, idx, gemm, sel


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--val_images", type=int, default=16)
    p.add_argument("--bank_images", type=int, default=1323)
    p.add_argument("--workspace_mb", type=int, nargs="+", default=[16, 64, 256])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", type=str, default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "n31_nn_retrieval.txt"))
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    Q, N = args.val_images * PATCHES, args.bank_images * PATCHES
    sims = Q * N
    scale = (FULL_Q * FULL_N) / sims
    lines = [torch.cuda.get_device_name(0),
             f"dense NN search, D = {D}, k = {K}: Q = {args.val_images} x {PATCHES} = {Q} queries, bank N = {args.bank_images} x {PATCHES} = {N} rows, "
             f"{sims:.3e} similarities",
             f"  = 1 / {scale:.1f} of the VOC-sized problem (Q = {FULL_Q}, N = {FULL_N}, {FULL_Q * FULL_N:.3e} similarities); 'full' below is the time x {scale:.1f}",
             f"routes alternate inside each repetition; {args.warmup} warm-up + {args.reps} timed repetitions, medians; HIP events around every block"]
    queries, bank = unit_rows(Q, 1, dev), unit_rows(N, 2, dev)
    for mb in args.workspace_mb:
        ws_bytes = mb << 20
        plan = ops.nn_search_plan(Q, N, ws_bytes)
        floats = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)
        t = {r: {"gemm": [], "select": [], "wall": []} for r in ("hip", "torch")}
        for rep in range(args.warmup + args.reps):
            results = {}
            for route in ("hip", "torch"):
                torch.cuda.synchronize()
                w0, w1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                w0.record()
                results[route] = run(queries, bank, route, plan, floats, True)
                w1.record()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    t[route]["gemm"].append(results[route][2])
                    t[route]["select"].append(results[route][3])
                    t[route]["wall"].append(w0.elapsed_time(w1))
            if rep == 0:
                same = torch.equal(results["hip"][0], results["torch"][0]) and torch.equal(results["hip"][1], results["torch"][1])
                lines.append(f"workspace {mb} MiB: {len(plan)} blocks of up to {plan[0][1] - plan[0][0]} queries x {plan[0][3] - plan[0][2]} bank rows; "
                             f"lists of the two routes equal: {same}")
        med = {r: {k: statistics.median(v) for k, v in t[r].items()} for r in t}
        for r in ("hip", "torch"):
            m = med[r]
            lines.append(f"  select={r:5s}  GEMM blocks {m['gemm']:9.2f} ms   select {m['select']:9.2f} ms = {4e-6 * sims / m['select']:8.1f} GB/s of similarities read   "
                         f"search {m['wall']:9.2f} ms   full: GEMM {m['gemm'] * scale / 1e3:7.1f} s + select {m['select'] * scale / 1e3:7.1f} s")
        lines.append(f"  select hip / torch = {med['hip']['select'] / med['torch']['select']:.3f}   search hip / torch = {med['hip']['wall'] / med['torch']['wall']:.3f}   "
                     f"select share of the hip search = {100 * med['hip']['select'] / (med['hip']['select'] + med['hip']['gemm']):.1f} %")
        del floats
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
