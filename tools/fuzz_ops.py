#!/usr/bin/env python3
"""Randomised shape fuzz of the HIP ops against torch fp64 / the oracle (development aid; run on the GPU box).
Each round draws one case per op from the generator of the suite's sweep (tests/_sweep_cases.py) and checks it with the sweep's own
checks and bounds (tests/test_hip_sweep.py::run_case): more seeds of that sweep, all six tiers - the kernels of the training step, the
evaluator / optimizer / mask kernels (tests/_sweep_checks_eval.py), label propagation on square and rectangular grids with its
up-sampler (tests/_sweep_checks_prop.py: one-frame fp64 reference), the linear probe with the clip input pipeline
(tests/_sweep_checks_head.py) and the tiled / batched / fused k-means kernels with the metric counters (tests/_sweep_checks_metric.py: the
checks make their inputs valid by construction - fit blobs are drawn again until the fp64 run proves them valid, points within the
excuse gap of a tie beyond the allowed share are replaced - and tests/test_sweep_metric_host.py runs hundreds of draws per op to hold that)
and the operand-preparation kernels with the producers' gradient maxima (tests/_sweep_checks_prep.py: bit equality with NumPy restatements
of the pair and plane formats inside guarded buffers).  Then the ops the sweep does not cover.
usage: fuzz_ops.py [rounds=40] [seed=0]"""
import os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np, torch, torch.nn.functional as F
from timetuning_amd import hip_ops as ops
from oracle import timet_oracle as O
from _sweep_cases import OPS, case_id, draw
from test_hip_sweep import run_case

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 40
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
dev = lambda a: torch.as_tensor(a).cuda()
rel = lambda a, b: float((a.double().cpu() - b.double().cpu()).abs().max() / (b.double().abs().max() + 1e-30))
worst = {}
sweep_worst = {}
def note(name, err, tol, info):
    worst[name] = max(worst.get(name, 0.0), err)
    assert err < tol, (name, err, info)

for it in range(rounds):
    # the sweep's ops: one draw each from the shared generator
    for op in OPS:
        case = draw(op, rng)
        try:
            run_case(op, case, sweep_worst)
        except AssertionError as e:
            raise AssertionError(f"{case_id(op, case)}: {e}") from None
    # label propagation: random grid, window, contexts, prototypes
    gl, Dl, Kl = int(rng.choice([5, 7, 14])), int(rng.choice([16, 32])), int(rng.choice([3, 20, 200, 300]))
    fs, bs, nlast, rad, topk = int(rng.integers(2, 7)), int(rng.integers(1, 4)), int(rng.integers(1, 5)), int(rng.integers(1, 8)), int(rng.integers(1, 7))   # (n_last_frames = 0 crashes the reference itself, mask_propagation.py:489)
    nl = gl * gl
    feats = torch.randn(fs, bs, nl, Dl)
    for t in range(1, fs): feats[t] = 0.7 * feats[t - 1] + 0.3 * feats[t]
    xn = F.normalize(feats, dim=-1)
    seg0 = torch.softmax(torch.randn(bs, nl, Kl) * 2, -1)
    maps = ops.label_propagate_maps(dev(xn), dev(seg0), nlast, rad, topk, 0.1).cpu().numpy()
    bad = tot = 0
    for b_ in range(bs):
        seed = seg0[b_].view(gl, gl, Kl).permute(2, 0, 1).unsqueeze(0)
        refm = torch.stack(O.propagate_labels(nlast, rad, topk, gl, xn[:, b_], seed)).reshape(fs - 1, Kl, nl).transpose(1, 2).numpy()
        d = np.abs(maps[:, b_] - refm).max(-1) > 1e-5 * np.abs(refm).max()
        bad += d.sum(); tot += d.size
    note("label_propagate_maps (fraction of queries off)", bad / tot, 0.03, (gl, Dl, Kl, fs, bs, nlast, rad, topk))
    # patch embedding (lean gather instance for 16-pixel patches)
    Dp, Hh, Ww = int(rng.choice([64, 128, 384])), 16 * int(rng.integers(1, 5)), 16 * int(rng.integers(1, 5))
    nsrc = int(rng.integers(1, 5)); fmap = rng.integers(0, nsrc, int(rng.integers(1, 6))).astype(np.int32)
    img, wp, bp, cls = torch.randn(nsrc, 3, Hh, Ww), torch.randn(Dp, 768) * 0.05, torch.randn(Dp), torch.randn(Dp)
    npat = (Hh // 16) * (Ww // 16)
    pos = torch.randn(1 + npat, Dp)
    conv = F.conv2d(img[torch.as_tensor(fmap).long()].double(), wp.double().view(Dp, 3, 16, 16), bp.double(), stride=16)
    ref = torch.cat([cls.double().expand(len(fmap), 1, Dp), conv.flatten(2).transpose(1, 2)], 1) + pos.double()
    tok = ops.patch_embed_fwd(dev(img), dev(wp), dev(bp), dev(cls), dev(pos), 16, dev(fmap))
    note("patch_embed_fwd", rel(tok, ref), 3e-5, (Dp, Hh, Ww, nsrc, len(fmap)))
    # patch embedding on bf16 operands (round 3): against the fp64 conv of the SAME rounded operands
    Dq = int(rng.choice([64, 128, 256, 384, 768]))
    wq = torch.randn(Dq, 768) * 0.05; bq, clsq, posq = torch.randn(Dq), torch.randn(Dq), torch.randn(1 + npat, Dq)
    convq = F.conv2d(img[torch.as_tensor(fmap).long()].to(torch.bfloat16).double(), wq.to(torch.bfloat16).double().view(Dq, 3, 16, 16), bq.double(), stride=16)
    refq = torch.cat([clsq.double().expand(len(fmap), 1, Dq), convq.flatten(2).transpose(1, 2)], 1) + posq.double()
    tokq = ops.patch_embed_fwd_planes(dev(img), ops.split_planes(dev(wq), 1), dev(bq), dev(clsq), dev(posq), 16, dev(fmap))
    note("patch_embed_fwd_planes", rel(tokq, refq), 3e-5, (Dq, Hh, Ww, nsrc, len(fmap)))
    # bf16 attention forward: any token count up to 256, any head count
    Fa, Na, Ha = int(rng.integers(1, 4)), int(rng.integers(1, 257)), int(rng.integers(1, 5))
    qb = (torch.randn(Fa, Na, 3 * Ha * 64) * 0.7).to(torch.bfloat16)
    q_, k_, v_ = qb.double().view(Fa, Na, 3, Ha, 64).permute(2, 0, 3, 1, 4)
    refa = (torch.softmax(q_ @ k_.transpose(-1, -2) * 0.125, -1) @ v_).permute(0, 2, 1, 3).reshape(Fa, Na, Ha * 64)
    note("attention_fwd_bf16", rel(ops.attention_fwd_bf16(dev(qb), Ha).float(), refa), 2e-2, (Fa, Na, Ha))
    # the persistent 8-phase plane GEMM (large ragged M, whole 256 / 128-wide column tiles, every tile-count regime by chance)
    if it % 4 == 0:
        P8 = int(rng.choice([1, 3])); BN = 256 if P8 == 1 else 128; BKq = 128 if P8 == 1 else 64
        M8, N8, K8 = int(rng.integers(9000, 40000)), BN * int(rng.integers(1, 7)), BKq * int(rng.integers(1, 5))
        x8, w8, b8 = torch.randn(M8, K8), torch.randn(N8, K8) * 0.1, torch.randn(N8)
        xp8, wp8 = ops.split_planes(dev(x8), P8), ops.split_planes(dev(w8), P8)
        res8 = torch.randn(M8, N8) if rng.random() < 0.5 else None
        out8 = ops.linear_fwd_planes(xp8, wp8, dev(b8), residual=dev(res8) if res8 is not None else None)["y"]
        ref8 = F.linear(xp8.double().sum(0).cpu(), wp8.double().sum(0).cpu(), b8.double())
        if res8 is not None: ref8 = ref8 + res8.double()
        note(f"linear_fwd_planes (large M) P={P8}", rel(out8, ref8), 3e-5, (P8, M8, N8, K8, res8 is not None))
    # weight gradient from row pairs (transposing LDS reads): any M, N and K multiples of 128
    Mt, Nt_, Kt = int(rng.integers(1, 9000)), 128 * int(rng.integers(1, 5)), 128 * int(rng.integers(1, 5))
    dyt, xt = torch.randn(Mt, Nt_) * 0.05, torch.randn(Mt, Kt)
    dwt = ops.linear_bwd_weight_pairs_tn(ops.split_pairs(dev(dyt)), ops.split_pairs(dev(xt)))
    note("linear_bwd_weight_pairs_tn", rel(dwt, dyt.double().t() @ xt.double()), 2e-6, (Mt, Nt_, Kt))
print("fuzz ok:", {k: f"{v:.2e}" for k, v in worst.items()})
print("sweep ops (worst / bound):", {k: f"{v[0]:.2e} / {v[1]:.0e}" for k, v in sorted(sweep_worst.items())})
