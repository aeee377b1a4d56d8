"""GPU parity of the stem gradients (scope row N19): tt_patch_embed_bwd and tt_pos_embed_interpolate_bwd at the op level against torch on
the CPU in fp64, and the trainable stem end to end - module surface, training step, optimizer steps, EMA teacher, cached operands, the
captured step graph - against the CPU oracle.  Every reference is computed once and shared."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err, rel_l2
from timetuning_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-3
FULL = ["blocks", "patch_embed", "pos_embed", "cls_token"]        # the reference's full fine-tuning (models.py:929-935)
STEM11 = ["patch_embed", "pos_embed", "cls_token", "blocks.11"]
STEM = ("feature_extractor.backbone.patch_embed.proj.weight", "feature_extractor.backbone.patch_embed.proj.bias",
        "feature_extractor.backbone.cls_token", "feature_extractor.backbone.pos_embed")
HEAD = (128, 128, 64, 32)

# (F, C, H, W, P, D, frame_map): one row; 18 rows, rectangular; 980 rows through a frame map with a repeated source frame (F_src = 4);
# P = 8 (15 patches, K = 192); K = 256; fewer rows than a row slab
CASES = [(1, 3, 16, 16, 16, 64, None), (3, 3, 32, 48, 16, 128, None), (5, 3, 224, 224, 16, 384, (2, 0, 3, 1, 2)), (2, 3, 40, 24, 8, 192, None),
         (3, 1, 32, 32, 16, 64, None), (7, 3, 16, 32, 16, 64, None)]
_CACHE: dict = {}


def _case(i):
    """Inputs of case i and the fp64 reference: autograd of F.conv2d(stride = P) + class token + position table."""
    if ("case", i) not in _CACHE:
        Fr, C, H, W, P, D, fm = CASES[i]
        n = (H // P) * (W // P)
        gen = torch.Generator().manual_seed(100 + i)
        Fs = Fr if fm is None else max(fm) + 1
        img = torch.randn((Fs, C, H, W), generator=gen)
        dtok = torch.randn((Fr, n + 1, D), generator=gen)
        idx = torch.arange(Fr) if fm is None else torch.tensor(fm)
        w = torch.randn((D, C, P, P), generator=gen, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(D, dtype=torch.float64, requires_grad=True)
        cls = torch.zeros((1, 1, D), dtype=torch.float64, requires_grad=True)
        table = torch.zeros((1, n + 1, D), dtype=torch.float64, requires_grad=True)
        t = F.conv2d(img[idx].double(), w, b, stride=P).flatten(2).transpose(1, 2)
        tok = torch.cat((cls.expand(Fr, -1, -1), t), dim=1) + table
        (tok * dtok.double()).sum().backward()
        a = dtok.double().abs()
        _CACHE["case", i] = dict(img=img, dtok=dtok, fm=None if fm is None else torch.tensor(fm, dtype=torch.int32), n=n, K=C * P * P,
                                 dw=w.grad.reshape(D, -1), dbias=b.grad, dcls=cls.grad.reshape(D), dtable=table.grad.reshape(n + 1, D),
                                 abs_table=a.sum(0), abs_bias=a[:, 1:].sum((0, 1)),
                                 rows=F.unfold(img[idx], P, stride=P).transpose(1, 2).reshape(Fr * n, C * P * P).contiguous())
    return _CACHE["case", i]


def _run(i, **kw):
    from timetuning_amd import hip_ops as ops

    c = _case(i)
    return ops.patch_embed_bwd(c["dtok"].cuda(), c["img"].cuda(), CASES[i][4], None if c["fm"] is None else c["fm"].cuda(), **kw)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_patch_weight_gradient_vs_fp64_and_the_materialised_route(i):
    """dw against fp64, held to the error of the existing weight-gradient kernel on the materialised rows (patches unfolded by torch,
    dtok rows gathered) at the same shape: max(2 x that error, 2e-6) - the two kernels partition the same fp32 row sum differently."""
    from timetuning_amd import _lib
    from timetuning_amd import hip_ops as ops

    c = _case(i)
    Fr, _, _, _, _, D, _ = CASES[i]
    got = _run(i, need=("dw",))["dw"]
    assert got.shape == (D, c["K"])
    dy = c["dtok"][:, 1:].reshape(Fr * c["n"], D).contiguous().cuda()
    try:
        yard, _ = ops.linear_bwd_weight(dy, c["rows"].cuda(), need_bias=False)
    except _lib.HipLibraryError:
        yard = ops.gemm(dy, c["rows"].cuda(), a_mmajor=True, b_nmajor=True)
    e, ey = rel_err(got, c["dw"]), rel_err(yard, c["dw"])
    print(f"[stem dw] case {CASES[i]}: fused {e:.3e}  materialised {ey:.3e}  ratio {e / max(ey, 1e-30):.2f}")
    assert e <= max(2 * ey, 2e-6), (CASES[i], e, ey)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_stem_reductions_within_the_fixed_order_sum_bound(i):
    """dtable / dcls / dbias elementwise within m 2^-24 sum|terms| (m terms: F for dtable and dcls, F n for dbias) - the worst case of a
    fixed-order fp32 sum.  Asked for together and one at a time (dbias without dtable folds from the workspace)."""
    c = _case(i)
    Fr, n = CASES[i][0], c["n"]
    u = 2.0 ** -24
    r = _run(i, need=("dbias", "dcls", "dtable"))
    solo = {k: _run(i, need=(k,))[k] for k in ("dbias", "dcls", "dtable")}
    for k in solo:
        assert torch.equal(solo[k], r[k]), k
    for k, m, mag in (("dtable", Fr, c["abs_table"]), ("dcls", Fr, c["abs_table"][0]), ("dbias", Fr * n, c["abs_bias"])):
        d = (r[k].cpu().double() - c[k]).abs()
        assert bool((d <= m * u * mag).all()), (CASES[i], k, float((d / (m * u * mag).clamp_min(1e-300)).max()))


def test_two_calls_give_the_same_bits_and_refusals_launch_nothing():
    from timetuning_amd import _lib
    from timetuning_amd import hip_ops as ops

    i = 2   # 980 rows: the row split and the workspace are live
    c = _case(i)
    Fr, C, H, W, P, D, _ = CASES[i]
    nb = _lib.load().tt_patch_embed_bwd_workspace_bytes(Fr, C, H, W, P, D)
    assert nb > (c["n"] + 1) * D * 4 + D * c["K"] * 4           # more than one slice of partial tiles behind the table scratch
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    a = _run(i, workspace=ws)
    ws.view(torch.float32).fill_(float("nan"))
    b = _run(i, workspace=ws)
    assert set(a) == {"dw", "dbias", "dcls", "dtable"}
    for k in a:
        assert torch.equal(a[k], b[k]) and bool(torch.isfinite(a[k]).all()), k
    # a too-small workspace and an out-of-domain shape: an error that names the rule, and the destinations untouched
    keep = torch.full((D, c["K"]), 7.0, device="cuda")
    with pytest.raises(_lib.HipLibraryError, match="workspace too small"):
        _run(i, need=("dw",), dw_out=keep, workspace=ws[: nb - 16])
    img6, dtok6 = torch.zeros((2, 3, 24, 24), device="cuda"), torch.zeros((2, 17, 64), device="cuda")
    keep6 = torch.full((64, 108), 7.0, device="cuda")
    with pytest.raises(_lib.HipLibraryError, match="P % 4 == 0"):
        ops.patch_embed_bwd(dtok6, img6, 6, need=("dw",), dw_out=keep6)
    assert not ops.patch_embed_bwd_ok(2, 3, 24, 24, 6, 64) and ops.patch_embed_bwd_ok(Fr, C, H, W, P, D)
    torch.cuda.synchronize()
    assert bool((keep == 7.0).all()) and bool((keep6 == 7.0).all())


@pytest.mark.parametrize("g,gh,gw", [(14, 10, 14), (14, 28, 28), (14, 1, 3), (4, 7, 5)])
def test_pos_embed_interpolate_adjoint(g, gh, gw):
    """The adjoint against the forward's own matrix M (one-hot tables through ops.pos_embed_interpolate): elementwise
    |got - M^T dy| <= 2^-22 |M|^T |dy| (the fixed-order sum bound with headroom for the weight's own rounding), and against torch's fp64
    autograd of the reference's F.interpolate(..., mode="bicubic") call within TOL."""
    from timetuning_amd import hip_ops as ops

    S, Dd = g * g, 8
    onehot = torch.zeros((1 + S, S))
    onehot[1:] = torch.eye(S)
    M = ops.pos_embed_interpolate(onehot.cuda(), gh, gw)[1:].cpu().double()      # [gh * gw, g * g]
    dy = torch.randn((1 + gh * gw, Dd), generator=torch.Generator().manual_seed(7 + g + gh))
    got = ops.pos_embed_interpolate_bwd(dy.cuda(), g, gh, gw).cpu().double()
    assert got.shape == (1 + S, Dd) and torch.equal(got[0], dy[0].double())      # the class row is copied
    want, mag = M.t() @ dy[1:].double(), M.abs().t() @ dy[1:].double().abs()
    d = (got[1:] - want).abs()
    assert bool((d <= 2.0 ** -22 * mag).all()), float((d / mag.clamp_min(1e-300)).max() * 2.0 ** 22)
    pos = torch.zeros((1, 1 + S, Dd), dtype=torch.float64, requires_grad=True)
    patch = F.interpolate(pos[:, 1:].reshape(1, g, g, Dd).permute(0, 3, 1, 2), scale_factor=((gh + 0.1) / g, (gw + 0.1) / g), mode="bicubic")
    assert patch.shape[-2:] == (gh, gw)
    table = torch.cat((pos[:, 0].unsqueeze(0), patch.permute(0, 2, 3, 1).reshape(1, -1, Dd)), dim=1)
    (table[0] * dy.double()).sum().backward()
    assert rel_err(got, pos.grad[0]) < TOL
    out = torch.full((1 + S, Dd), 3.0, device="cuda")                             # a caller-owned destination
    assert ops.pos_embed_interpolate_bwd(dy.cuda(), g, gh, gw, out=out) is out and torch.equal(out.cpu().double(), got)


def assert_all_grads(mine, og, what, tol_l2=1e-4, tol_max=TOL):
    """The rule of tests/test_hip_timet.py::assert_all_grads: EVERY trainable tensor's gradient against the oracle's, relative L2 < 1e-4 and
    max-normalised < 1e-3."""
    names = [n for n, p_ in mine.items() if p_.requires_grad]
    assert len(names) >= 10 and set(names) <= set(og), (len(names), sorted(set(names) - set(og))[:3])
    for n in names:
        assert mine[n].grad is not None, (what, n, "no gradient")
        l2, e = rel_l2(mine[n].grad.cpu(), og[n]), rel_err(mine[n].grad.cpu(), og[n])
        assert l2 < tol_l2 and e < tol_max, (what, n, l2, e)
    return names


def _surface_oracle(hw, use_head, layers):
    key = ("surface", hw, use_head, tuple(layers))
    if key not in _CACHE:
        from oracle import timet_oracle as O

        om = O.build_oracle("dino-s16", 8, HEAD, mode="stress", vit_cfg=synth.ARCHS["tiny-s16"], unfreeze_layers=tuple(layers))
        x = torch.from_numpy(synth.make_clips(1, 3, 224, seed=41)).view(3, 3, 224, 224)[:, :, : hw[0], : hw[1]].contiguous()
        of, _ = om.feature_extractor(x, use_head=use_head, faithful=False)
        w = torch.from_numpy(synth.normal("stem.surface.w", tuple(of.shape)))
        (of * w).sum().backward()
        _CACHE[key] = dict(x=x, w=w, f=of.detach(), grads={"feature_extractor." + k: v.grad.detach().clone()
                                                           for k, v in om.feature_extractor.named_parameters() if v.grad is not None})
    return _CACHE[key]


@pytest.mark.parametrize("layers", [FULL, STEM11], ids=["all", "stem+blocks.11"])
@pytest.mark.parametrize("use_head", [True, False])
@pytest.mark.parametrize("hw", [(224, 224), (160, 224)], ids=["224x224", "160x224"])
def test_stem_gradients_at_the_module_surface(accurate_precision, hw, use_head, layers):
    """``FeatureExtractor(..., train_stem=True)``: the gradient of a random linear functional of the features against the oracle's
    autograd, every trainable tensor, on the stored grid and on a 10 x 14 one (the position gradient through the bicubic adjoint)."""
    from timetuning_amd.models import FeatureExtractor

    o = _surface_oracle(hw, use_head, layers)
    fe = FeatureExtractor("dino-s16", "", list(HEAD), unfreeze_layers=layers, vit_cfg=synth.ARCHS["tiny-s16"], init="stress",
                          return_attention=False, train_stem=True).cuda()
    f, _ = fe(o["x"].cuda(), use_head=use_head)
    assert f.requires_grad and rel_err(f, o["f"]) < 1e-4
    (f * o["w"].cuda()).sum().backward()
    mine = {"feature_extractor." + k: v for k, v in fe.named_parameters() if use_head or not k.startswith("head.")}
    names = assert_all_grads(mine, o["grads"], (accurate_precision, hw, use_head))
    assert set(STEM) <= set(names)
    for n in STEM:   # by name: the four stem tensors
        assert rel_err(mine[n].grad.cpu(), o["grads"][n]) < TOL and tuple(mine[n].grad.shape) == tuple(mine[n].shape), n
    if layers is STEM11:
        assert mine["feature_extractor.backbone.blocks.3.mlp.fc1.weight"].grad is None   # on the path, computed, dropped


def _build_timet(layers, K=20, teacher=False, arch="tiny-s16"):
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    fe = FeatureExtractor("dino-s16", "", list(HEAD), unfreeze_layers=layers, vit_cfg=synth.ARCHS[arch], init="stress",
                          return_attention=False, train_stem=True)
    model = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, fe.feature_dim))).cuda()
    if teacher:
        model.init_momentum_teacher()
        model.set_momentum_teacher_schedular_params(0.9, 1.0, 1, 4)
    return model


def _step_oracle(use_mask, masks):
    # (the oracle does not depend on the GPU's arithmetic mode: one run is shared - per distinct pair of foreground masks with --use_mask)
    key = ("step", use_mask, None if masks is None else tuple(m.numpy().tobytes() for m in masks))
    if key not in _CACHE:
        from oracle import timet_oracle as O

        bs, fs, K = 2, 3, 20
        om = O.build_oracle("dino-s16", K, HEAD, mode="stress", vit_cfg=synth.ARCHS["tiny-s16"], unfreeze_layers=tuple(FULL))
        x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=5))
        kw = dict(mask_features=True, masks_override=masks) if use_mask else dict(faithful=False)
        oloss, aux = om.get_loss(x, return_aux=True, **kw)
        oloss.backward()
        _CACHE[key] = dict(x=x, loss=oloss.item(), labels=aux["labels"].reshape(bs, -1).clone(),
                           grads={n: p_.grad.detach().clone() for n, p_ in om.named_parameters() if p_.grad is not None})
    return _CACHE[key]


@pytest.mark.parametrize("use_mask", [False, True], ids=["plain", "use_mask"])
def test_training_step_with_everything_trainable(accurate_precision, use_mask):
    """``get_loss().backward()`` with the oracle's labels, everything trainable: every gradient by the ``assert_all_grads`` rule, the four
    stem tensors among them.  With --use_mask the oracle is given the GPU's foreground masks (a discontinuous decision, as in
    test_hip_timet.py)."""
    bs, fs = 2, 3
    model = _build_timet(FULL)
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=5))
    masks = None
    if use_mask:
        with torch.no_grad():
            model.get_loss(x.cuda(), mask_features=True)
        masks = (model.last_aux["source_mask"].cpu(), model.last_aux["target_mask"].cpu())
    o = _step_oracle(use_mask, masks)
    loss = model.get_loss(x.cuda(), mask_features=use_mask, target_labels=o["labels"])
    loss.backward()
    assert abs(loss.item() - o["loss"]) < 2e-4, (loss.item(), o["loss"])
    names = assert_all_grads(dict(model.named_parameters()), o["grads"], (accurate_precision, use_mask))
    assert set(STEM) <= set(names) and len(names) == len(o["grads"])


def test_three_optimizer_steps_track_the_oracle():
    """Three iterations with SwavOptimizer against SwavOptimizerOracle, everything trainable: the losses stay together (rtol 5e-3, as
    test_ten_training_steps_track_the_oracle) and the updated stem agrees."""
    from oracle import timet_oracle as O
    from timetuning_amd.my_utils import cosine_scheduler
    from timetuning_amd.time_tuning import SwavOptimizer

    bs, fs, K, E, I = 2, 3, 20, 1, 4
    model = _build_timet(FULL)
    opt = SwavOptimizer(model, "AdamW", True, 1e-5, 1e-4, "CosineAnnealingLR", cosine_scheduler(0.04, 0.4, E, I), I, E)
    om = O.build_oracle("dino-s16", K, HEAD, mode="stress", vit_cfg=synth.ARCHS["tiny-s16"], unfreeze_layers=tuple(FULL))
    oopt = O.SwavOptimizerOracle(om, 1e-5, 1e-4, O.cosine_scheduler(0.04, 0.4, E, I), I, E)
    gpu, cpu = [], []
    for s in range(3):
        x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=80 + s))
        loss = model.get_loss(x.cuda())
        opt.step(loss)
        model.normalize_prototypes()
        oloss = om.get_loss(x, faithful=False)
        oopt.zero_grad()
        oloss.backward()
        oopt.step()
        om.normalize_prototypes()
        gpu.append(loss.item())
        cpu.append(oloss.item())
    np.testing.assert_allclose(gpu, cpu, rtol=5e-3)
    mine = dict(model.named_parameters())
    for n in STEM:
        assert rel_err(mine[n], om.feature_extractor.backbone[n.split("backbone.", 1)[1]]) < 1e-4, n


def test_teacher_embeds_its_own_frames_when_the_stem_trains():
    """Stem + blocks.11 trainable: the frozen blocks 0 - 10 are shared with the EMA teacher, the stem is not - a teacher whose patch
    projection differs must not continue from the student's activations.  Fails if the tap is taken above block 0."""
    from oracle import timet_oracle as O

    cfg, K, bs, fs = synth.ARCHS["tiny-s16"], 20, 2, 3
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=31))
    delta = torch.from_numpy(synth.normal("teacher.stem.delta", (cfg["embed_dim"], 3, 16, 16), 0.05))
    model = _build_timet(STEM11, K, teacher=True)
    om = O.build_oracle("dino-s16", K, HEAD, mode="stress", vit_cfg=cfg, unfreeze_layers=tuple(STEM11))
    om.init_momentum_teacher()
    om.set_momentum_teacher_schedular_params(0.9, 1.0, 1, 4)
    with torch.no_grad():
        model.teacher.backbone.patch_embed.proj.weight.add_(delta.cuda())
        om.teacher.backbone["patch_embed.proj.weight"].add_(delta)
    model.invalidate_teacher_cache()
    assert model.teacher_shares_frozen_blocks()          # the FROZEN tensors still match: only the stem tells the two apart
    oloss, aux = om.get_loss(x, faithful=False, return_aux=True)
    loss = model.get_loss(x.cuda(), target_labels=aux["labels"].reshape(bs, -1))
    assert rel_err(model.last_aux["q"].cpu(), aux["batch_q"]) < TOL
    assert abs(loss.item() - oloss.item()) < 2e-4, (loss.item(), oloss.item())


def test_cached_operands_follow_the_optimizer_update():
    """"f16x3" with the stem trainable: after an optimizer update (raw-pointer writes: torch's version counters do not move) the cached pair
    form of the patch weight and the cached resampled position table must be rebuilt - the features equal, bit for bit, those of a fresh
    FeatureExtractor loaded with the updated state dict."""
    from timetuning_amd import engine
    from timetuning_amd import hip_ops as ops
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.my_utils import cosine_scheduler
    from timetuning_amd.time_tuning import FusedAdamW, SwavOptimizer

    def fresh(state):
        fe2 = FeatureExtractor("dino-s16", "", list(HEAD), unfreeze_layers=FULL, init="stress", return_attention=False, train_stem=True).cuda()
        fe2.load_state_dict(state)
        return fe2

    keep, ops.PAIRS_MIN_ROWS = ops.PAIRS_MIN_ROWS, 0
    ops.set_gemm_precision("f16x3")
    try:
        # (a) the training step at 224 x 224: the pair form of the patch weight (ViT-S/16: C P P <= 3 D, the pair patch embedding runs)
        model = _build_timet(FULL, arch="dino-s16")
        assert engine.patch_pairs_ok(model.feature_extractor.backbone, torch.empty(1, 3, 224, 224))
        opt = SwavOptimizer(model, "AdamW", True, 1e-3, 1e-3, "CosineAnnealingLR", cosine_scheduler(0.04, 0.4, 1, 4), 4, 1)
        x = torch.from_numpy(synth.make_clips(2, 3, 224, seed=5)).cuda()
        frames = x.view(6, 3, 224, 224)
        with torch.no_grad():
            before, _ = model.feature_extractor(frames, use_head=False)
        opt.step(model.get_loss(x))
        with torch.no_grad():
            after, _ = model.feature_extractor(frames, use_head=False)
            want, _ = fresh(model.feature_extractor.state_dict())(frames, use_head=False)
        assert not torch.equal(before, after) and torch.equal(after, want)
        # (b) the module surface at 160 x 224: the resampled position table
        fe = model.feature_extractor
        small = frames[:3, :, :160].contiguous()
        adam = FusedAdamW([p for p in fe.parameters() if p.requires_grad], lr=1e-3)
        f, _ = fe(small, use_head=False)
        before = f.detach().clone()
        f.square().sum().backward()
        adam.step()
        with torch.no_grad():
            after, _ = fe(small, use_head=False)
            want, _ = fresh(fe.state_dict())(small, use_head=False)
        assert not torch.equal(before, after) and torch.equal(after, want)
    finally:
        ops.PAIRS_MIN_ROWS = keep
        ops.set_gemm_precision("f32")


def test_step_graph_replays_the_eager_step_with_the_stem_trainable(accurate_precision):
    """The captured step takes the stem's launches: two models from the same weights train three steps on the same clips - one eagerly, one
    through the graph (step 1 eager, step 2 captured and replayed, step 3 replayed) - and stay bit for bit equal."""
    from timetuning_amd.my_utils import cosine_scheduler
    from timetuning_amd.time_tuning import SwavOptimizer

    bs, fs = 2, 2
    clips = [torch.from_numpy(synth.make_clips(bs, fs, 224, seed=40 + i)).cuda() for i in range(3)]
    runs = []
    for graph in (False, True):
        m = _build_timet(FULL)
        o = SwavOptimizer(m, "AdamW", True, 1e-5, 1e-4, "CosineAnnealingLR", cosine_scheduler(0.04, 0.4, 1, 8), 8, 1)
        if graph:
            m.enable_step_graph()
        rec = []
        for i, x in enumerate(clips):
            loss = m.get_loss(x)
            m.train_update(o, loss, i + 1)
            rec.append((loss.item(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
        torch.cuda.synchronize()
        runs.append((m, rec))
    (me, re_), (mg, rg) = runs
    assert len(mg._step_graphs) >= 1, "no step was captured"
    for i, ((le, ge), (lg, gg)) in enumerate(zip(re_, rg)):
        assert le == lg, (i, le, lg)
        assert set(STEM) <= set(ge) and ge.keys() == gg.keys() and all(torch.equal(ge[n], gg[n]) for n in ge), i
    pe, pg = dict(me.named_parameters()), dict(mg.named_parameters())
    assert all(torch.equal(pe[n], pg[n]) for n in pe)


def test_stem_gradients_through_the_exchange_path():
    """The data-parallel exchange with everything trainable, as an N-GPU rank runs it (a one-rank RCCL communicator): the stem's
    gradients enter the exchange after block 0's, in a bucket of their own, written by the kernels straight into the flat buffer - and
    train exactly what the plain step trains (W = 1: the mean is the identity).  In a child process: the communicator is process-global."""
    import json
    import os
    import subprocess
    import sys

    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_stem_exchange_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    o = json.loads(lines[-1][7:])
    assert all(o.values()), o
