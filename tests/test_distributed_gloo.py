"""world_size-2 `gloo` tests (CPU) of the N>1 path: the global Sinkhorn all-gather, the flat gradient all-reduce and the
data-parallel wrapper.  The collective logic is the product's (timetuning_amd.engine / models); where a HIP kernel would
run, the CPU oracle is injected as the solver - exactly what the `solver=` hook is for."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _oracle_solver(scores, iters, eps, row0=0, rows_out=None):
    from oracle import timet_oracle as O

    q = O.sinkhorn(torch.exp(scores / eps).t(), iters)
    rows_out = scores.shape[0] - row0 if rows_out is None else rows_out
    return q[row0:row0 + rows_out]


def _worker(rank, W, port, ret):
    import sys

    sys.path.insert(0, REPO)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=W)
    from oracle import timet_oracle as O
    from timetuning_amd import engine, synth
    from timetuning_amd.models import DistributedDataParallelModel, FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    out = {}
    # (1) global Sinkhorn: all-gather + redundant global solve == reference W=2 run == its all-reduce formulation
    g = np.load(os.path.join(GOLDEN, "sinkhorn_w2.npz"))
    scores = torch.from_numpy(g["scores"])
    B = scores.shape[0] // W
    local = scores[rank * B:(rank + 1) * B].contiguous()
    q = engine.global_sinkhorn(local, B, 0.05, int(g["iters"]), solver=_oracle_solver)
    out["q_err_vs_reference"] = float((q - torch.from_numpy(g["q"][rank * B:(rank + 1) * B])).abs().max())

    def allreduce(t):
        t = t.clone()
        dist.all_reduce(t)
        return t

    q_r = O.sinkhorn(torch.exp(local / 0.05).t(), int(g["iters"]), world_size=W, all_reduce=allreduce)
    out["q_err_vs_allreduce_form"] = float((q - q_r).abs().max())
    # (1b) the product's OWN all-reduce variant (engine.global_sinkhorn_allreduce, --sinkhorn_exchange allreduce): the reference's
    # pattern - columns stay on their rank, the K row sums are all-reduced per iteration; the CPU twin stands in for the HIP kernels
    from oracle import cpu_twin

    n_coll = [0]
    real_all_reduce = dist.all_reduce

    def counting_all_reduce(t, *a, **k):
        n_coll[0] += 1
        return real_all_reduce(t, *a, **k)

    dist.all_reduce = counting_all_reduce
    try:
        q_own = engine.global_sinkhorn_allreduce(local, B, 0.05, int(g["iters"]), lib=cpu_twin.load())
        engine.SINKHORN_EXCHANGE = "allreduce"          # ... and through the begin / end pair the training step uses
        ctx = engine.global_sinkhorn_begin(local)
        out["allreduce_ctx_is_local"] = ctx[1] is None and ctx[2] == "allreduce"
    finally:
        dist.all_reduce = real_all_reduce
        engine.SINKHORN_EXCHANGE = "allgather"
    out["allreduce_variant_collectives"] = n_coll[0] - int(g["iters"])   # 0: exactly one K-vector all-reduce per iteration
    out["q_own_allreduce_err_vs_reference"] = float((q_own - torch.from_numpy(g["q"][rank * B:(rank + 1) * B])).abs().max())
    q0 = engine.global_sinkhorn_allreduce(local, B, 0.05, 0, lib=cpu_twin.load())   # zero iterations: the column-normalised exp(scores / eps)
    e0 = torch.exp(local / 0.05)
    out["q_own_allreduce_iters0_err"] = float((q0 - e0 / e0.sum(1, keepdim=True)).abs().max())

    # (2) flat gradient all-reduce == mean of the per-rank gradients
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.zeros(7, 5)), torch.nn.Parameter(torch.zeros(11)), torch.nn.Parameter(torch.zeros(3, 2, 2))]
    grads = {p: torch.from_numpy(synth.normal(f"ddp.g{i}.r{rank}", tuple(p.shape))) for i, p in enumerate(params)}
    expect = [sum(torch.from_numpy(synth.normal(f"ddp.g{i}.r{r}", tuple(p.shape))) for r in range(W)) / W for i, p in enumerate(params)]
    red = engine.GradExchange().finish(dict(grads))   # everything in one bucket
    out["grad_err"] = max(float((red[p] - e).abs().max()) for p, e in zip(params, expect))
    # (2b) the bucketed, asynchronous form the fused step uses: gradients are pushed as backward produces them
    ex = engine.GradExchange()
    staged = {params[0]: grads[params[0]].clone()}
    ex.push(staged)
    staged[params[1]] = grads[params[1]].clone()
    ex.push(staged)
    ex.push(staged)                       # nothing new: no bucket
    staged[params[2]] = grads[params[2]].clone()
    fin = ex.finish(staged)
    out["bucket_err"] = max(float((fin[p] - e).abs().max()) for p, e in zip(params, expect))
    out["bucket_count_ok"] = bool(len(ex.sent) == 3)

    # (2c) round 5: the exchange decides ITSELF on the first multi-rank run (engine.autotune_exchange): both Sinkhorn exchanges and the
    # 4- / 1-bucket gradient exchange are timed on the step, MAX over ranks, and a variant replaces the default only when it is faster by
    # more than 3 %.  The step here is the product's collective logic on CPU tensors (oracle / CPU twin as the solvers) plus a sleep that
    # makes one configuration slow ON ONE RANK ONLY - every rank must still take the same decision.
    import time

    twin_lib = cpu_twin.load()
    n_red = [0]

    def make_step(slow):
        def step():
            if engine.SINKHORN_EXCHANGE == "allreduce":
                engine.global_sinkhorn_allreduce(local, B, 0.05, 3, lib=twin_lib)
            else:
                engine.global_sinkhorn(local, B, 0.05, 3, solver=_oracle_solver)
            ex_ = engine.GradExchange()
            st_ = {}
            for p_ in params:
                st_[p_] = grads[p_].clone()
                ex_.push(st_)
            fin_ = ex_.finish(st_)
            out["last_step_bucket_err"] = max(float((fin_[p_] - e_).abs().max()) for p_, e_ in zip(params, expect))
            if rank == 1:   # 30 ms for each slow property of the configuration: a penalty no host's compute time can outweigh
                time.sleep(0.03 * slow(engine.SINKHORN_EXCHANGE, engine.GRAD_BUCKETS))
        return step

    def counting2(t, *a, **k):
        n_red[0] += 1
        return real_all_reduce(t, *a, **k)

    # (i) the default is slow on rank 1 -> both variants win, on BOTH ranks
    c1 = engine.autotune_exchange(make_step(lambda sk, nb: (sk == "allgather") + (nb == 0)), "cpu", reps=2)
    out["auto_1"] = (c1["sinkhorn_exchange"], c1["grad_buckets"], engine.SINKHORN_EXCHANGE, engine.GRAD_BUCKETS, sorted(c1["ms_per_step"]))
    # with one bucket the whole exchange is ONE all-reduce, issued by finish()
    dist.all_reduce = counting2
    try:
        n0 = n_red[0]
        ex1 = engine.GradExchange()
        st1 = {}
        for p_ in params:
            st1[p_] = grads[p_].clone()
            ex1.push(st1)
        pushed = n_red[0] - n0
        f1 = ex1.finish(st1)
        out["one_bucket"] = (pushed, n_red[0] - n0, max(float((f1[p_] - e_).abs().max()) for p_, e_ in zip(params, expect)))
    finally:
        dist.all_reduce = real_all_reduce
    # (ii) the variants are the slow ones -> the default stays
    engine.SINKHORN_EXCHANGE, engine.GRAD_BUCKETS, engine.EXCHANGE_CHOICE = "allgather", 0, None
    # (round 6, ADVICE r5: the probe is side-effect free) a step that consumes the host generator and pushes "queue rows": with
    # ``state = (snapshot, restore)`` every timed variant starts from the same state and the state after the probe is the state before it
    probe = {"pushed": 0, "seen": []}

    def snap():
        return (probe["pushed"], torch.get_rng_state())

    def restore(st):
        probe["pushed"] = st[0]
        torch.set_rng_state(st[1])

    inner = make_step(lambda sk, nb: (sk == "allreduce") + (nb == 1))

    def stateful_step():
        probe["seen"].append((engine.SINKHORN_EXCHANGE, engine.GRAD_BUCKETS, probe["pushed"]))
        torch.randperm(64)          # (the queue permutation: torch's CPU generator)
        probe["pushed"] += 1
        inner()

    torch.manual_seed(77)
    before = torch.get_rng_state().clone()
    c2 = engine.autotune_exchange(stateful_step, "cpu", reps=2, state=(snap, restore))
    out["auto_2"] = (c2["sinkhorn_exchange"], c2["grad_buckets"], engine.SINKHORN_EXCHANGE, engine.GRAD_BUCKETS)
    # every variant saw the queue as it was (its warm-up step starts at 0 pushes), and nothing of the probe is left behind
    firsts = {}
    for sk_, nb_, pushed_ in probe["seen"]:
        firsts.setdefault((sk_, nb_), pushed_)
    out["auto_state_ok"] = bool(all(v == 0 for v in firsts.values()) and len(firsts) == 3 and probe["pushed"] == 0
                                and torch.equal(torch.get_rng_state(), before))
    out["auto_err"] = out["last_step_bucket_err"]
    engine.SINKHORN_EXCHANGE, engine.GRAD_BUCKETS, engine.EXCHANGE_CHOICE = "allgather", 0, None

    # (3) the wrapper broadcasts rank 0's parameters and passes attribute access through
    cfg = synth.ARCHS["tiny-s16"]
    fe = FeatureExtractor("dino-s16", "", [128, 128, 64, 32], unfreeze_layers=["blocks.11", "blocks.10"], vit_cfg=cfg, init="stress", seed=1 + rank)
    model = TimeT(fe, 20, prototype_init=torch.from_numpy(synth.make_prototypes(20, 32, seed=1 + rank)))
    ddp = DistributedDataParallelModel(model, 0)
    ref = synth.make_prototypes(20, 32, seed=1)
    out["bcast_err"] = float((ddp.prototypes.detach() - torch.from_numpy(ref)).abs().max())
    w0 = synth.make_vit_weights(mode="stress", seed=1, **cfg)["blocks.11.mlp.fc2.weight"]
    out["bcast_err_w"] = float((model.feature_extractor.backbone.blocks[11].mlp.fc2.weight.detach() - torch.from_numpy(w0)).abs().max())
    ddp.init_queue(40)
    out["passthrough"] = bool(ddp.queue.shape == (40, 32) and ddp.get_non_ddp_model() is model and ddp.data_parallel)
    ret[rank] = out
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_world_size_2_gloo():
    W = 2
    ctx = mp.get_context("spawn")
    mgr = ctx.Manager()
    ret = mgr.dict()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, W, port, ret)) for r in range(W)]
    [p.start() for p in procs]
    [p.join(240) for p in procs]
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    for r in range(W):
        o = ret[r]
        assert o["bucket_err"] < 1e-6 and o["bucket_count_ok"], o
        assert o["q_err_vs_reference"] < 2e-6, o
        assert o["q_err_vs_allreduce_form"] < 2e-6, o
        # the product's own all-reduce variant: the reference's numbers, exactly `iters` K-vector all-reduces, the begin / end pair routes to it
        assert o["q_own_allreduce_err_vs_reference"] < 2e-6 and o["q_own_allreduce_iters0_err"] < 1e-6, o
        assert o["allreduce_variant_collectives"] == 0 and o["allreduce_ctx_is_local"], o
        assert o["grad_err"] < 1e-6, o
        # the self-deciding exchange: same decision on every rank, recorded with its measurements; one bucket = one all-reduce at the end
        assert o["auto_1"] == ("allreduce", 1, "allreduce", 1, ["allgather/4", "allreduce/1", "allreduce/4"]), o["auto_1"]
        assert o["auto_2"] == ("allgather", 4, "allgather", 0), o["auto_2"]
        assert o["auto_state_ok"], "the exchange probe left state behind (queue rows / host generator)"
        assert o["one_bucket"][0] == 0 and o["one_bucket"][1] == 1 and o["one_bucket"][2] < 1e-6, o["one_bucket"]
        assert o["auto_err"] < 1e-6, o
        assert o["bcast_err"] == 0.0 and o["bcast_err_w"] == 0.0, o
        assert o["passthrough"], o
