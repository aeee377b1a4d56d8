"""`python bench.py --gpus N` must start N ranks by itself (the reference's mp.spawn, time_tuning.py:714-717), before any
GPU call.  Dry mode (TT_BENCH_DRY=1, gloo): no GPU, no kernels - the ranks only join the process group and report."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(n, extra_env=None, timeout=240):
    env = dict(os.environ, TT_BENCH_DRY="1", TT_BENCH_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", str(n), "--steps", "2", "--warmup", "1"],
                          env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.timeout(300)
def test_gpus_n_spawns_n_distinct_ranks():
    r = _run(3)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout                      # ONE JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == 3 and out["ranks"] == [0, 1, 2]
    assert len(set(out["pids"])) == 3 and os.getpid() not in out["pids"]
    assert out["rccl"] == {"world_size": 3, "backend": "gloo"}
    assert out["config"]["global_batch"] == 96 and out["config"]["parallelism"] == "dp3"


@pytest.mark.timeout(300)
def test_a_failing_rank_fails_the_run_without_hanging():
    r = _run(2, {"TT_BENCH_DRY_FAIL_RANK": "1"}, timeout=200)
    assert r.returncode != 0
    assert "rank process 1 exited with 3" in r.stderr


def test_the_launcher_parent_never_touches_the_gpu():
    """Static check: what the parent executes (main() up to the launch_ranks call, launch_ranks, _free_port) contains no
    torch.cuda attribute access and no import of the HIP front end."""
    import ast

    src = open(os.path.join(REPO, "bench.py")).read()
    tree = ast.parse(src)
    fn = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}

    def gpu_touching(nodes):
        for top in nodes:
            for n in ast.walk(top):
                if isinstance(n, ast.Attribute) and n.attr == "cuda":
                    return True
                if isinstance(n, (ast.Import, ast.ImportFrom)) and "timetuning_amd" in ast.dump(n):
                    return True
        return False

    assert not gpu_touching([fn["launch_ranks"], fn["_free_port"]])
    head = []
    for stmt in fn["main"].body:
        head.append(stmt)
        if "launch_ranks" in ast.dump(stmt):
            break
    else:
        raise AssertionError("main() no longer calls launch_ranks")
    assert not gpu_touching(head)


def test_dump_outputs_writes_the_last_step_within_budget(tmp_path, monkeypatch):
    """``--dump-outputs``: loss, assignment, every trainable tensor and its gradient as float32 .npy; over the byte budget the large arrays
    keep a fixed sample of their elements - the same one in every run."""
    import importlib.util

    import numpy as np
    import torch

    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    g = torch.Generator().manual_seed(0)
    model = torch.nn.Linear(300, 100)
    model.bias.requires_grad_(False)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=g)
    model.last_aux = {"q": torch.rand(2, 50, 20, generator=g, dtype=torch.float64)}
    loss = torch.tensor(1.25)

    bench.dump_outputs(str(tmp_path / "full"), model, loss)
    full = {f[:-4]: np.load(tmp_path / "full" / f) for f in os.listdir(tmp_path / "full")}
    assert sorted(full) == ["grad.weight", "loss", "param.weight", "q"]
    assert all(v.dtype == np.float32 for v in full.values())
    assert full["loss"] == np.float32(1.25) and np.array_equal(full["q"], model.last_aux["q"].float().numpy())
    assert np.array_equal(full["param.weight"], model.weight.detach().numpy()) and np.array_equal(full["grad.weight"], model.weight.grad.numpy())

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 15000)   # 62 001 floats in all: the weight and its gradient are sampled
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), model, loss)
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f[:-4]: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert sum(v.size for v in a.values()) <= 15000 + 4096 and a["q"].shape == (2, 50, 20)
    assert a["param.weight"].size < 30000 and all(np.array_equal(a[k], b[k]) for k in a)
    assert np.isin(a["param.weight"], full["param.weight"]).all()


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_line_is_the_headline_and_full_adds_the_rest():
    """A plain one-GPU run prints the headline line and nothing measured outside the timed steps; ``--full`` adds the replay check, the
    eager step time, the roofline pass, the other precision modes and the Sinkhorn rate (C1-sized: the timed steps are graph replays)."""
    args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch_size", "2", "--num_frames", "2", "--num_clusters", "50"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full", "--no_cpu_baseline", "--no_exchange_probe"])):
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args, *extra], env=env, capture_output=True, text=True, timeout=400)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, r.stdout
        lines[name] = json.loads(out[0])
    plain, full = lines["plain"], lines["full"]
    extras = {"ms_per_step_eager", "graph_check", "roofline", "alt_precision", "sinkhorn", "cpu_baseline", "rccl_single_rank_probe"}
    assert not extras & set(plain)
    assert plain["metric"] == "clip-frames/sec" and plain["unit"] == "clip-frames/sec" and plain["higher_is_better"] is True
    assert plain["dtype"] == "f32-split(f16x3)" and plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["rccl"] is None
    assert set(plain) < set(full) and extras - {"rccl_single_rank_probe"} <= set(full)
    if full["step_graph"]:
        assert full["graph_check"]["replay_equals_eager"] and full["ms_per_step_eager"] > 0
    assert full["roofline"]["achieved"] > 0 and sorted(full["alt_precision"]) == ["bf16", "bf16x6", "f32"]
    assert full["sinkhorn"]["iters_per_sec"] > 0 and full["cpu_baseline"] is None
