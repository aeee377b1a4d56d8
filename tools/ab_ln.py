#!/usr/bin/env python3
"""A/B of the row-wise operand producers between library builds: usage ab_ln.py libA.so libB.so ...

Entries: tt_layernorm_fwd / _planes (3 planes) / _pairs, tt_split_planes (3 planes), tt_split_pairs - timed in interleaved rounds (median and
min..max of the rounds per build; the four large shapes) and every output buffer compared bit for bit against the FIRST build's: y, mean, rstd, the range flag (also
with one out-of-range input, which must raise it in every build), LayerNorm planes at 1 / 2 / 3 planes.  Then tt_patch_embed_fwd_planes /
_pairs at ViT-S/16 on 4 frames of 224 x 224: tokens and the im2col rows of the workspace, bits only."""
import ctypes as C, os, statistics, sys, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from timetuning_amd._lib import SIGNATURES

ENTRIES = ("tt_layernorm_fwd", "tt_layernorm_fwd_planes", "tt_layernorm_fwd_pairs", "tt_split_planes", "tt_split_pairs",
           "tt_patch_embed_fwd_planes", "tt_patch_embed_fwd_pairs", "tt_patch_embed_planes_workspace_bytes", "tt_patch_embed_pairs_workspace_bytes")
def load(p):
    lib = C.CDLL(os.path.abspath(p))
    for name in ENTRIES: getattr(lib, name).restype, getattr(lib, name).argtypes = SIGNATURES[name]
    return lib
libs = [(os.path.basename(p)[3:-3], load(p)) for p in sys.argv[1:]]
st = torch.cuda.current_stream().cuda_stream
dev = dict(device="cuda")
ptr = lambda t: None if t is None else t.data_ptr()
bits = lambda t: t.view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.uint8)
differing = 0

def compare(what, outs):
    """outs: {build: [tensors]} - counts the elements whose bits differ from the first build's"""
    global differing
    first = outs[libs[0][0]]
    for name, _ in libs[1:]:
        n = sum(int((bits(a) != bits(b)).sum().item()) for a, b in zip(first, outs[name]))
        differing += n
        print(f"  bits {what}: {name} vs {libs[0][0]}: {n} differing elements in {len(first)} buffers", flush=True)

def timed(what, call):
    ts = {name: [] for name, _ in libs}
    for rd in range(12):
        for name, lib in libs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20): assert call(lib) == 0
            e1.record(); torch.cuda.synchronize()
            if rd >= 3: ts[name].append(e0.elapsed_time(e1) * 1e3 / 20)
    print(f"  time {what}: " + " | ".join(f"{n} {statistics.median(t):6.2f} us ({min(t):.2f}..{max(t):.2f})" for n, t in ts.items()), flush=True)

# the four timed shapes, then every other instantiation at a few ragged rows, bits only: D = 128 NV, and the general kernel (96, 640)
SHAPES = [(25216, 384, 0, True), (25088, 384, 197, True), (25216, 768, 0, True), (6304, 384, 0, True)] + \
         [(1003, D, 0, False) for D in (128, 256, 512, 1024, 96, 640)] + [(1000, 1024, 6, False)]
for rows, D, skip, is_timed in SHAPES:
    print(f"rows={rows} D={D} skip={skip}", flush=True)
    Fr = rows // (skip - 1) if skip else 0
    x = torch.randn(Fr * skip if skip else rows, D, **dev) * 2 + 0.3; g = 1 + 0.1 * torch.randn(D, **dev); b = 0.1 * torch.randn(D, **dev)
    n = x.numel()
    mean, rstd, flag = torch.empty(rows, **dev), torch.empty(rows, **dev), torch.zeros(4, dtype=torch.int32, **dev)
    yf, yp, yq = torch.empty(rows, D, **dev), torch.empty(3, rows, D, dtype=torch.bfloat16, **dev), torch.empty(rows, 2 * D, dtype=torch.float16, **dev)
    sp, sq = torch.empty(3, n, dtype=torch.bfloat16, **dev), torch.empty(2 * n, dtype=torch.float16, **dev)
    calls = {
        "layernorm_fwd": (lambda lib, P=3: lib.tt_layernorm_fwd(ptr(x), ptr(g), ptr(b), ptr(yf), ptr(mean), ptr(rstd), rows, D, 1e-6, skip, st), yf),
        "layernorm_fwd_planes": (lambda lib, P=3: lib.tt_layernorm_fwd_planes(ptr(x), ptr(g), ptr(b), ptr(yp), rows * D, P, ptr(mean), ptr(rstd), rows, D, 1e-6, skip, st), yp),
        "layernorm_fwd_pairs": (lambda lib, P=3: lib.tt_layernorm_fwd_pairs(ptr(x), ptr(g), ptr(b), ptr(yq), ptr(mean), ptr(rstd), rows, D, 1e-6, skip, ptr(flag), st), yq),
        "split_planes": (lambda lib, P=3: lib.tt_split_planes(ptr(x), ptr(sp), n, P, n, st), sp),
        "split_pairs": (lambda lib, P=3: lib.tt_split_pairs(ptr(x), ptr(sq), n, ptr(flag), st), sq),
    }
    for what, (call, out) in calls.items():
        if is_timed: timed(what, call)
        for planes in ((1, 2, 3) if "planes" in what else (3,)):
            # in range; then one result beyond fp16's range - a value of x for a split, a gamma for a LayerNorm (the pair producers must raise
            # the flag, in every build)
            tgt, at = (g, (3,)) if "layernorm" in what else (x, (5, 7))
            for poke in (None, 1e6):
                keep = tgt[at].item()
                if poke: tgt[at] = poke
                outs = {}
                for name, lib in libs:
                    for t in (out, mean, rstd): bits(t).fill_(-1)
                    flag.zero_()
                    assert call(lib, planes) == 0
                    outs[name] = [t.clone() for t in (out, mean, rstd, flag)]
                    if "pairs" in what: assert int(flag[0].item()) == (1 if poke else 0), (what, name, poke, flag)
                tgt[at] = keep
                compare(f"{what} planes={planes} poke={poke}", outs)

Fr, Cc, H, W, P, D = 4, 3, 224, 224, 16, 384
K, M = Cc * P * P, Fr * (1 + (H // P) * (W // P))
print(f"patch embed F={Fr} {H}x{W} P={P} D={D}", flush=True)
img, w, bias, cls, pos = torch.randn(Fr, Cc, H, W, **dev), 0.05 * torch.randn(D, K, **dev), torch.randn(D, **dev), torch.randn(D, **dev), torch.randn(M // Fr, D, **dev)
flag = torch.zeros(4, dtype=torch.int32, **dev)
for kind, elem in (("planes", 2), ("pairs", 4)):
    outs = {}
    for name, lib in libs:
        wq = torch.empty(D, K * elem // 2, dtype=torch.bfloat16 if kind == "planes" else torch.float16, **dev)
        assert (lib.tt_split_planes(ptr(w), ptr(wq), w.numel(), 1, w.numel(), st) if kind == "planes" else lib.tt_split_pairs(ptr(w), ptr(wq), w.numel(), ptr(flag), st)) == 0
        nb = getattr(lib, f"tt_patch_embed_{kind}_workspace_bytes")(Fr, Cc, H, W, P)
        ws, tokens = torch.zeros(nb, dtype=torch.uint8, **dev), torch.full((M, D), float("nan"), **dev)
        args = [ptr(img), None, ptr(wq), ptr(bias), ptr(cls), ptr(pos), ptr(tokens), Fr, Cc, H, W, P, D, ptr(ws), nb] + ([ptr(flag)] if kind == "pairs" else []) + [st]
        assert getattr(lib, f"tt_patch_embed_fwd_{kind}")(*args) == 0
        torch.cuda.synchronize()
        outs[name] = [tokens, ws[:M * K * elem].clone(), wq, flag.clone()]   # (the rest of the workspace is the GEMM's K-split block)
    compare(f"patch_embed_fwd_{kind}", outs)
print(f"TOTAL differing elements: {differing}", flush=True)
sys.exit(1 if differing else 0)
