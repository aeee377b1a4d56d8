"""End-to-end GPU parity of the reference-named modules (FeatureExtractor / TimeT / SwavOptimizer) against the
golden vectors generated from the reference, and against the CPU oracle at BASELINE sizes through
size-independent properties."""
import numpy as np
import pytest
import torch

from conftest import rel_err, rel_l2, tail_err
from timetuning_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-3  # north-star bound: 1e-3 relative fp32 on patch embeddings and assignment logits


def assert_close(a, b, tol, what="", guard=3e-5):
    """The north-star quantities (patch embeddings, assignment logits) in three measures: max-normalised (``rel_err``), relative L2
    (a single large reference element cannot flatter it) and relative L2 over the 10 % smallest-magnitude reference elements (what a
    max-normalised bound hides; their own scale is ~1/20 of the tensor's, hence the factor).  ``tol`` is the contract (north-star: 1e-3);
    ``guard`` is a regression tripwire on the relative L2 error: the fp32-class modes measure 3e-7 ... 1e-5 here (round 4, printed with
    TT_TEST_PRINT_ERRORS=1), so an arithmetic regression of 3x - 100x fails the test long before the contract is in danger."""
    e, l2, tl = rel_err(a, b), rel_l2(a, b), tail_err(a, b)
    assert l2 < guard, (what, "regression guard", l2, guard)
    import os
    if os.environ.get("TT_TEST_PRINT_ERRORS"):
        print(f"[errors] {what}: max-norm {e:.2e}  rel-L2 {l2:.2e}  tail-L2 {tl:.2e}  (bound {tol:.0e})")
    assert e < tol and l2 < tol and tl < 20 * tol, (what, e, l2, tl)



def assert_all_grads(mg, og, what, tol_l2=1e-4, tol_max=TOL):
    """EVERY trainable tensor's gradient against the oracle's (the full-size tests used to look at three of the 33): relative
    L2 < 1e-4 - the fp32-class modes measure 1e-6 ... 2e-5 here; 2.5e-5 was what the unscaled fp16 split of the dy tensors cost in round
    4 - and the max-normalised contract bound beside it.  ``og``: name -> gradient (tensor) of the oracle."""
    import os
    names = [n for n, p_ in mg.items() if p_.requires_grad]
    assert len(names) >= 10 and set(names) <= set(og), (len(names), sorted(set(names) - set(og))[:3])
    worst = ("", 0.0)
    for n in names:
        assert mg[n].grad is not None, (what, n, "no gradient")
        l2, e = rel_l2(mg[n].grad.cpu(), og[n]), rel_err(mg[n].grad.cpu(), og[n])
        if l2 > worst[1]:
            worst = (n, l2)
        assert l2 < tol_l2 and e < tol_max, (what, n, l2, e)
    if os.environ.get("TT_TEST_PRINT_ERRORS"):
        print(f"[errors] {what}: {len(names)} gradients, worst rel-L2 {worst[1]:.2e} ({worst[0]})")
    return len(names)


# The CPU oracle's full-size steps take minutes on the host and do not depend on the GPU's arithmetic mode: computed ONCE per session and
# shared by the three fp32-class modes (C3's 32-clip batch had been skipped in the headline mode for the oracle's cost).
_ORACLE_CACHE: dict = {}


def _c2_oracle_step():
    if "c2" not in _ORACLE_CACHE:
        from oracle import timet_oracle as O

        bs, fs, K = 32, 4, 200
        torch.set_num_threads(min(32, torch.get_num_threads()))
        om = O.build_oracle("dino-s16", K, (1024, 1024, 512, 256), mode="stress")
        x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=3))
        oloss, aux = om.get_loss(x, faithful=False, return_aux=True)
        oloss.backward()
        _ORACLE_CACHE["c2"] = dict(x=x, loss=oloss.item(), batch_q=aux["batch_q"].detach().clone(), target_scores=aux["target_scores"].detach().clone(),
                                   labels=aux["labels"].reshape(bs, -1).clone(),
                                   grads={n: p_.grad.detach().clone() for n, p_ in om.named_parameters() if p_.grad is not None})
    return _ORACLE_CACHE["c2"]


C3_WATCH = ("prototypes", "feature_extractor.head.6.weight", "feature_extractor.backbone.blocks.10.attn.qkv.weight",
            "feature_extractor.backbone.blocks.11.mlp.fc2.weight")


def _c3_oracle_steps(bs, steps):
    """C3's per-rank work on the oracle: per step the inputs' seeds, the loss, the assignment, the labels, EVERY gradient, and the state
    after the optimizer / prototype / teacher update (watched parameters, queue, teacher prototypes, a teacher weight)."""
    key = ("c3", bs, steps)
    if key not in _ORACLE_CACHE:
        from oracle import timet_oracle as O

        fs, K, Q, E, I = 4, 200, 2048, 1, 4
        torch.set_num_threads(min(32, torch.get_num_threads()))
        om = O.build_oracle("dino-s16", K, (1024, 1024, 512, 256), mode="stress")
        oopt = O.SwavOptimizerOracle(om, 1e-5, 1e-4, O.cosine_scheduler(0.04, 0.4, E, I), I, E)
        om.init_momentum_teacher()
        om.set_momentum_teacher_schedular_params(0.995, 1.0, E, I)
        om.init_queue(Q)
        om.queue.copy_(_c3_queue_fill(Q))
        recs = []
        for s_ in range(steps):
            x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=70 + s_))
            perm = torch.randperm(bs * 196, generator=torch.Generator().manual_seed(s_)).numpy()
            oloss, aux = om.get_loss(x, faithful=False, return_aux=True, queue_perm=perm)
            oopt.zero_grad()
            oloss.backward()
            rec = dict(perm=perm, loss=oloss.item(), batch_q=aux["batch_q"].detach().clone(), labels=aux["labels"].reshape(bs, -1).clone(),
                       grads={n: p_.grad.detach().clone() for n, p_ in om.named_parameters() if p_.grad is not None})
            oopt.step()
            om.normalize_prototypes()
            om.update_momentum_teacher(oopt.global_step)
            og = dict(om.named_parameters())
            rec.update(params={n: og[n].detach().clone() for n in C3_WATCH}, queue=om.queue.clone(), teacher_prototypes=om.teacher_prototypes.clone(),
                       teacher_fc2=om.teacher.backbone["blocks.11.mlp.fc2.weight"].clone())
            recs.append(rec)
        _ORACLE_CACHE[key] = recs
    return _ORACLE_CACHE[key]


def _c3_queue_fill(Q):
    return torch.nn.functional.normalize(torch.from_numpy(synth.normal("c3.queue", (Q, 256))), dim=1) * 3.0


def _build(g, teacher=False, queue=0):
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.my_utils import cosine_scheduler
    from timetuning_amd.time_tuning import SwavOptimizer, TimeT

    D, depth, heads, patch = [int(v) for v in g["vit_cfg"]]
    cfg = dict(embed_dim=D, depth=depth, num_heads=heads, patch_size=patch)
    bs, fs, K, _, _, steps, E, I = [int(v) for v in g["cfg"]]
    arch = str(g["arch"]) if "arch" in g.files else "dino-s16"
    fe = FeatureExtractor(arch, "", [int(v) for v in g["head_list"]], unfreeze_layers=["blocks.11", "blocks.10"],
                          vit_cfg=cfg, init=str(g["mode"]))
    model = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, fe.feature_dim))).cuda()
    opt = SwavOptimizer(model, "AdamW", True, 1e-5, 1e-4, "CosineAnnealingLR", cosine_scheduler(0.04, 0.4, E, I), I, E)
    if teacher:
        model.init_momentum_teacher()
        model.set_momentum_teacher_schedular_params(0.995, 1.0, E, I)
    if queue:
        model.init_queue(queue)
    return model, opt


def test_state_dict_keys_match_reference(golden):
    g = golden("timet_tiny_tq")
    model, _ = _build(g, True, 40)
    assert set(model.state_dict().keys()) == {str(k) for k in g["state_dict_keys"]}


def test_extractor_tiny(golden, accurate_precision):
    g = golden("timet_tiny")
    model, _ = _build(g)
    bs, fs = int(g["cfg"][0]), int(g["cfg"][1])
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=1)).view(bs * fs, 3, 224, 224).cuda()
    f, attn = model.feature_extractor(x)
    bf, _ = model.feature_extractor(x, use_head=False)
    assert_close(f.cpu(), g["features"], 1e-4, "tiny patch embeddings")
    assert_close(bf.cpu(), g["backbone_features"], 1e-4, "tiny backbone features")
    assert rel_err(attn[:, :, 0, :].cpu(), g["attn_cls_row"]) < 1e-4
    f2, _ = model(x)  # TimeT.forward(train=False): the extractor under no_grad
    with torch.no_grad():
        f3, _ = model.feature_extractor(x)
    assert torch.equal(f2, f3) and rel_err(f2, f) < 1e-5   # (with grad the trainable blocks take the activation-keeping path)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_extractor_other_input_sizes(golden, tag):
    """Inputs that are not 224x224: bicubic pos-embed resampling (tt_pos_embed_interpolate), non-square token grids,
    token counts 121 / 257 / 25 through the attention kernels; against the reference's outputs."""
    from timetuning_amd import hip_ops as ops
    from timetuning_amd.models import FeatureExtractor

    g = golden("extractor_sizes")
    D, depth, heads, patch = [int(v) for v in g["vit_cfg"]]
    fe = FeatureExtractor("dino-s16", "", [int(v) for v in g["head_list"]], vit_cfg=dict(embed_dim=D, depth=depth, num_heads=heads, patch_size=patch),
                          init="stress").cuda()
    H, W = [int(v) for v in g[f"{tag}_hw"]]
    x = torch.from_numpy(synth.normal(f"sizes.x.{tag}", (2, 3, H, W))).cuda()
    pos = fe.backbone.pos_table(H, W)
    assert rel_err(pos.cpu(), g[f"{tag}_pos"]) < 1e-5
    assert fe.backbone.pos_table(H, W) is pos            # cached per input size
    f, attn = fe(x)
    bf, _ = fe(x, use_head=False)
    assert rel_err(f.cpu(), g[f"{tag}_features"]) < 1e-4
    assert rel_err(bf.cpu(), g[f"{tag}_backbone_features"]) < 1e-4
    assert rel_err(attn[:, :, 0, :].cpu(), g[f"{tag}_attn_cls_row"]) < 1e-4
    with pytest.raises(ValueError):
        fe(torch.zeros(1, 3, 100, 224, device="cuda"))    # not a multiple of the patch size


def test_loss_internals_tiny(golden, accurate_precision):
    g, t = golden("aux_tiny"), golden("timet_tiny")
    model, _ = _build(t)
    bs, fs, K = [int(v) for v in g["cfg"]]
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=1)).cuda()
    with torch.no_grad():
        # the reference's own hard labels feed the cross entropy, so the loss is compared whether or not a top-k near-tie
        # flipped one of ours; the propagation's labels are compared separately
        loss = model.get_loss(x, target_labels=g["labels"].reshape(bs, -1))
    aux = model.last_aux
    assert rel_err(aux["q"].cpu(), g["q"]) < TOL and rel_l2(aux["q"].cpu(), g["q"]) < TOL
    assert_close(aux["target_scores"].cpu(), g["target_scores"], TOL, "tiny assignment logits")
    mism = aux["labels"].cpu().numpy() != g["labels"].reshape(bs, -1)
    assert mism.mean() <= 0.01
    assert abs(loss.item() - float(t["loss0"])) < 1e-4


def _run_steps(g, teacher, queue):
    bs, fs, K, _, _, steps, E, I = [int(v) for v in g["cfg"]]
    model, opt = _build(g, teacher, queue)
    params = dict(model.named_parameters())
    assert [len(gr["params"]) for gr in opt.optimizer.param_groups] == list(g["group_sizes"])
    use_mask = bool(int(g["use_mask"])) if "use_mask" in g.files else False
    for s in range(steps):
        if use_mask:
            x = torch.from_numpy(synth.make_smooth_clips(bs, fs, 224, seed=int(g["clip_seed0"]) + 1 + s)).cuda()
        else:
            x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=1 + s)).cuda()
        loss = model.get_loss(x, queue_perm=g[f"perm{s}"], mask_features=use_mask)
        if use_mask and s == 0:
            # the reference's masks of the step-0 student frames [bs*fs,1,g,g] (clip-major); ours are kept for the target frames
            # and, without a teacher, the source frames
            ref = g["student_mask0"].reshape(bs, fs, -1)
            assert (model.last_aux["target_mask"].cpu().numpy() == ref[:, -1]).all()
            if not teacher:
                assert (model.last_aux["source_mask"].cpu().numpy() == ref[:, 0]).all()
            assert 0.2 < ref.mean() < 0.9
        opt.step(loss)
        model.normalize_prototypes()
        if teacher:
            model.update_momentum_teacher(opt.global_step)
        assert abs(loss.item() - float(g[f"loss{s}"])) < 2e-4, (s, loss.item(), float(g[f"loss{s}"]))
        names = [str(n) for n in g[f"gradnorm_names{s}"]]
        mine = np.array([params[n].grad.double().norm().item() for n in names])
        np.testing.assert_allclose(mine, g[f"gradnorm{s}"], rtol=TOL, atol=1e-9)
        for key in g.files:
            if key.startswith(f"grad{s}:"):
                assert rel_err(params[key.split(":", 1)[1]].grad.cpu(), g[key]) < TOL, key
            if key.startswith(f"param{s}:"):
                # the mask fixtures use the small-weight "dino" init: |w| ~ 0.02, so Adam's first steps (lr * g / (|g| + eps),
                # sensitive where g ~ 0) weigh 2.5x more in the relative error of the updated parameter
                assert rel_err(params[key.split(":", 1)[1]].detach().cpu(), g[key]) < (3e-5 if use_mask else 1e-5), key
        np.testing.assert_allclose([gr["lr"] for gr in opt.optimizer.param_groups], g[f"lr{s}"], rtol=1e-9)
        np.testing.assert_allclose([gr["weight_decay"] for gr in opt.optimizer.param_groups], g[f"wd{s}"], rtol=1e-9)
        if teacher:
            sd = model.state_dict()
            assert rel_err(sd["teacher_prototypes"].cpu(), g[f"teacher_prototypes{s}"]) < 1e-5
            # (the EMA copies 99.5 % of the student's updated tensor: same tolerance as the parameter itself)
            assert rel_err(sd["teacher.backbone.blocks.11.mlp.fc2.weight"].cpu(), g[f"teacher_fc2_{s}"]) < (3e-5 if use_mask else 1e-5)
            assert rel_err(sd["teacher.backbone.blocks.3.attn.qkv.weight"].cpu().reshape(-1)[::97], g[f"teacher_b3qkv_{s}"]) < 1e-5
        if queue:
            assert rel_err(model.queue[:64].cpu(), g[f"queue_head{s}"]) < 1e-4
            assert abs(model.queue.double().sum().item() - float(g[f"queue_sum{s}"])) < 1e-2


def test_training_steps_tiny(golden, accurate_precision):
    _run_steps(golden("timet_tiny"), False, 0)


def test_training_steps_tiny_300_prototypes(golden, accurate_precision):
    """K = 300 prototypes against the reference's own run: the K > 256 instances of the label-propagation, Sinkhorn and
    cross-entropy kernels (BASELINE C4 has 400) and a score GEMM whose width is not a multiple of 64."""
    _run_steps(golden("timet_tiny_k300"), False, 0)


def test_training_steps_tiny_six_frames(golden, accurate_precision):
    """Six-frame clips against the reference's own run: up to five context frames per target in the label propagation (the
    similarities of all 15 (target, context) pairs in 6 batched launches, the 8-context instance of the wave-per-query kernel)."""
    _run_steps(golden("timet_tiny_f6"), False, 0)


def test_training_steps_tiny_patch8(golden, accurate_precision):
    """Patch size 8 (BASELINE C5's shape: 785 tokens - the KV-tiled attention, the general patch-embedding kernel, the 28 x 28
    propagation grid) against the REFERENCE's own run on a narrow ViT (head dim 64): extractor outputs, then loss, gradients
    and parameters over two optimizer steps."""
    g = golden("timet_tiny_s8")
    model, _ = _build(g)
    bs, fs = int(g["cfg"][0]), int(g["cfg"][1])
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=1)).view(bs * fs, 3, 224, 224).cuda()
    f, attn = model.feature_extractor(x)
    assert f.shape[1] == 784 and rel_err(f.cpu(), g["features"]) < 1e-4 and rel_err(attn[:, :, 0, :].cpu(), g["attn_cls_row"]) < 1e-4
    _run_steps(g, False, 0)


def test_training_steps_tiny_teacher_queue(golden, accurate_precision):
    _run_steps(golden("timet_tiny_tq"), True, 40)


def test_training_steps_tiny_use_mask(golden, accurate_precision):
    """--use_mask: attention foreground masks on features and loss against the reference's numbers."""
    _run_steps(golden("timet_tiny_mask"), False, 0)


def test_training_steps_tiny_use_mask_teacher_queue(golden, accurate_precision):
    _run_steps(golden("timet_tiny_mask_tq"), True, 40)


def test_full_size_c1(golden, accurate_precision):
    """ViT-S/16, bs 2 x 2 frames, K=50 (BASELINE C1) against the reference's own numbers."""
    g = golden("timet_c1")
    model, opt = _build(g)
    bs, fs = int(g["cfg"][0]), int(g["cfg"][1])
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=1)).cuda()
    f, _ = model.feature_extractor(x.view(bs * fs, 3, 224, 224))
    bf, _ = model.feature_extractor(x.view(bs * fs, 3, 224, 224), use_head=False)
    assert_close(f[:, ::49, ::16].cpu(), g["features_slice"], TOL, "C1 patch embeddings (slice)")
    assert_close(bf[:, ::49, ::16].cpu(), g["backbone_features_slice"], TOL, "C1 backbone features (slice)")
    assert abs(f.double().norm().item() / float(g["features_norm"]) - 1) < 1e-4
    loss = model.get_loss(x)
    assert abs(loss.item() - float(g["loss0"])) < 2e-4
    loss.backward()
    params = dict(model.named_parameters())
    for key in g.files:
        if key.startswith("grad0:"):
            mine = params[key.split(":", 1)[1]].grad.cpu().numpy()
            mine = mine if mine.size < 70000 else mine.reshape(-1)[::97]
            assert rel_err(mine, g[key]) < TOL, key


@pytest.mark.parametrize("teacher_queue", [False, True])
def test_step_graph_replays_the_eager_step(accurate_precision, teacher_queue):
    """``TimeT.enable_step_graph()`` (round 5, BASELINE C1's launch-bound regime): from the second step of a shape on, the step's whole
    launch sequence is ONE captured hipGraph.  Two models from the same weights train four steps on the same clips (C1's shape: 2 clips x 2
    frames at ViT-S/16 size) - one eagerly, one through the graph (step 1 eager, step 2 captured + replayed, steps 3 - 4 replayed) - and
    must stay bit for bit equal: losses, every gradient, every parameter, the queue and the teacher (the same kernels on the same bytes;
    the queue's permutations come from the same host generator state)."""
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.my_utils import cosine_scheduler
    from timetuning_amd.time_tuning import SwavOptimizer, TimeT

    bs, fs, K = 2, 2, 50

    def make():
        fe = FeatureExtractor("dino-s16", "", [1024, 1024, 512, 256], unfreeze_layers=["blocks.11", "blocks.10"], init="stress", return_attention=False)
        m = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, 256))).cuda()
        o = SwavOptimizer(m, "AdamW", True, 1e-5, 1e-4, "CosineAnnealingLR", cosine_scheduler(0.04, 0.4, 1, 8), 8, 1)
        if teacher_queue:
            m.init_momentum_teacher()
            m.set_momentum_teacher_schedular_params(0.995, 1.0, 1, 8)
            m.init_queue(bs * 10 * 4)    # bs * 10 rows are pushed per step (time_tuning.py:250-261): steps 1 - 3 see a filling queue (eager,
                                         # captured, replayed), step 4's push fills it (a new state: eager), 5 is captured, 6 replayed
        return m, o

    clips = [torch.from_numpy(synth.make_clips(bs, fs, 224, seed=40 + i)).cuda() for i in range(6)]
    runs = []
    for graph in (False, True):
        m, o = make()
        if graph:
            m.enable_step_graph()
        torch.manual_seed(123)   # (the queue's permutations: torch's CPU generator, as the reference)
        rec = []
        for i, x in enumerate(clips):
            loss = m.get_loss(x)
            m.train_update(o, loss, min(i + 1, 7))
            rec.append((loss.item(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
        torch.cuda.synchronize()
        runs.append((m, rec))
    (me, re_), (mg, rg) = runs
    assert len(mg._step_graphs) >= 1, "no step was captured"
    for i, ((le, ge), (lg, gg)) in enumerate(zip(re_, rg)):
        assert le == lg, (i, le, lg)
        assert ge.keys() == gg.keys() and all(torch.equal(ge[n], gg[n]) for n in ge), i
    pe, pg = dict(me.named_parameters()), dict(mg.named_parameters())
    assert all(torch.equal(pe[n], pg[n]) for n in pe)
    if teacher_queue:
        assert torch.equal(me.queue, mg.queue) and torch.equal(me.teacher_prototypes, mg.teacher_prototypes)
        assert len(mg._step_graphs) == 2   # filling, then full


def test_step_graph_sees_rewritten_frozen_weights(accurate_precision):
    """A captured step refreshes the pair operands of the tensors that were stale at capture time - the trainable ones.  A FROZEN weight
    rewritten in place afterwards (``load_state_dict``, a hand edit) must not be served from the graph's stale operands: the frozen
    tensors' version counters are part of the graph's signature, the step falls back to the eager path (which refreshes) and captures anew."""
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.my_utils import cosine_scheduler
    from timetuning_amd.time_tuning import SwavOptimizer, TimeT

    bs, fs, K = 2, 2, 50
    clips = [torch.from_numpy(synth.make_clips(bs, fs, 224, seed=60 + i)).cuda() for i in range(6)]
    runs = []
    for graph in (False, True):
        fe = FeatureExtractor("dino-s16", "", [1024, 1024, 512, 256], unfreeze_layers=["blocks.11", "blocks.10"], init="stress", return_attention=False)
        m = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, 256))).cuda()
        o = SwavOptimizer(m, "AdamW", True, 1e-5, 1e-4, "CosineAnnealingLR", cosine_scheduler(0.04, 0.4, 1, 8), 8, 1)
        if graph:
            m.enable_step_graph()
        losses = []
        for i, x in enumerate(clips):
            if i == 3:   # steps 0 - 2: eager, captured, replayed; now a frozen block's weight changes under the graph
                with torch.no_grad():
                    m.feature_extractor.backbone.blocks[3].mlp.fc1.weight.mul_(1.25)
            loss = m.get_loss(x)
            m.train_update(o, loss, min(i + 1, 7))
            losses.append(loss.item())
        torch.cuda.synchronize()
        runs.append((m, losses))
    (me, le), (mg, lg) = runs
    assert le == lg, (le, lg)
    pe, pg = dict(me.named_parameters()), dict(mg.named_parameters())
    assert all(torch.equal(pe[n], pg[n]) for n in pe)
    assert len(mg._step_graphs) == 2   # before and after the rewrite


GRAPH_CASES = [("c2", "f16x3", 12), ("c3", "f16x3", 10), ("c5", "f16x3", 6), ("c4", "bf16", 6), ("c4", "f16x3", 5)]


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("cfg,mode,steps", GRAPH_CASES)
def test_step_graph_equals_eager_at_baseline_shapes(cfg, mode, steps):
    """the captured step IS the eager step at every BASELINE shape - C2 (32 x 4, K 200), C3 (EMA teacher + full 2048-row
    queue, 32 clips), C5 (16 x 4, ViT-S/8), C4 (16 x 8, ViT-B/16, K 400) in the "bf16" mode and in the default one - with the bench's own
    dispatch thresholds (PAIRS_MIN_ROWS as shipped: the persistent pair GEMM, its K-split workspace, the row-pair weight gradients, the
    amax slots, the persistent / KV-tiled attention) and in the bench's REGIME: no host synchronisation between steps, so the host runs
    ahead of the device by as many replays as the runtime lets it.  Two models from the same weights, the same clip every step (as
    bench.py), one eager, one through the graph: every step's loss, the last step's 33 gradients, every parameter (and C3's queue and
    teacher) bit for bit.  (Round 5's headline was timed on replays that failed exactly this: an unbounded run-ahead of graph launches
    corrupts them on ROCm 7.2 - time_tuning.STEP_GRAPHS_IN_FLIGHT.)"""
    from timetuning_amd import hip_ops
    from tools.graph_vs_eager import CONFIGS, make

    arch, bs, fs, K, queue = CONFIGS[cfg]
    hip_ops.set_gemm_precision(mode)
    try:
        x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=11)).cuda()
        runs = []
        from timetuning_amd import engine

        for graph in (False, True):
            m, o = make(cfg, steps + 203)
            if graph:
                m.enable_step_graph()
            # (a captured step runs on ONE stream - engine.two_streams: the eager reference too; what the side streams change, the K-split
            # rounding of some launches' left-over tiles, is test_two_streams_equal_one_stream's subject)
            keep_streams, engine.TWO_STREAMS = engine.TWO_STREAMS, False
            torch.manual_seed(321)   # the queue's permutations
            losses = []
            for i in range(steps):
                loss = m.get_loss(x)
                m.train_update(o, loss, i + 1 if queue else 0)
                losses.append(loss.detach().clone())          # (no .item(): nothing here waits for the device)
            grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
            torch.cuda.synchronize()
            engine.TWO_STREAMS = keep_streams
            runs.append((m, [l.item() for l in losses], grads))
            del o
        (me, le, ge), (mg, lg, gg) = runs
        assert len(mg._step_graphs) == 1 and not mg._step_graph_failed, (len(mg._step_graphs), mg._step_graph_failed)
        assert le == lg, (cfg, mode, le, lg)
        assert len(ge) == 33 and ge.keys() == gg.keys() and all(torch.equal(ge[n], gg[n]) for n in ge)
        pe, pg = dict(me.named_parameters()), dict(mg.named_parameters())
        assert all(torch.equal(pe[n], pg[n]) for n in pe)
        if queue:
            assert torch.equal(me.queue, mg.queue) and torch.equal(me.teacher_prototypes, mg.teacher_prototypes)
            te, tg = dict(me.teacher.named_parameters()), dict(mg.teacher.named_parameters())
            assert all(torch.equal(te[n], tg[n]) for n in te)
    finally:
        hip_ops.set_gemm_precision("f32")


@pytest.mark.timeout(900)
def test_step_graph_replay_vs_oracle_c2():
    """A REPLAYED step against the oracle at C2's full size: ``target_labels`` ride into the captured step through a device buffer (they no
    longer bypass it), so the very assertions of ``test_c2_full_step_vs_oracle`` apply to the graph - the first call runs eagerly, the
    second is captured and replayed, the third replayed; all three are the same step (no update in between: the capture converts the pair
    operands although nothing made them stale)."""
    from timetuning_amd import hip_ops
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    hip_ops.set_gemm_precision("f16x3")
    try:
        bs, fs, K = 32, 4, 200
        fe = FeatureExtractor("dino-s16", "", [1024, 1024, 512, 256], unfreeze_layers=["blocks.11", "blocks.10"], init="stress", return_attention=False)
        model = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, 256))).cuda()
        model.enable_step_graph()
        o = _c2_oracle_step()
        x = o["x"].cuda()
        for call in range(3):
            model.zero_grad(set_to_none=True)
            loss = model.get_loss(x, target_labels=o["labels"])
            assert len(model._step_graphs) == (1 if call else 0)
            assert rel_err(model.last_aux["q"].cpu(), o["batch_q"]) < TOL and rel_l2(model.last_aux["q"].cpu(), o["batch_q"]) < TOL, call
            assert_close(model.last_aux["target_scores"].cpu(), o["target_scores"], TOL, f"C2 assignment logits, call {call}")
            assert (model.last_aux["labels"].cpu() != o["labels"]).float().mean().item() <= 0.01
            assert abs(loss.item() - o["loss"]) < 2e-4, (call, loss.item(), o["loss"])
            loss.backward()
            assert assert_all_grads(dict(model.named_parameters()), o["grads"], f"C2 replayed step, call {call}") == 33
    finally:
        hip_ops.set_gemm_precision("f32")


def _small_graph_pair(make_queue=None, teacher=False, K=50):
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.my_utils import cosine_scheduler
    from timetuning_amd.time_tuning import SwavOptimizer, TimeT

    out = []
    for graph in (False, True):
        fe = FeatureExtractor("dino-s16", "", [1024, 1024, 512, 256], unfreeze_layers=["blocks.11", "blocks.10"], init="stress", return_attention=False)
        m = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, 256))).cuda()
        o = SwavOptimizer(m, "AdamW", True, 1e-5, 1e-4, "CosineAnnealingLR", cosine_scheduler(0.04, 0.4, 1, 12), 12, 1)
        if teacher:
            m.init_momentum_teacher()
            m.set_momentum_teacher_schedular_params(0.995, 1.0, 1, 12)
        if make_queue is not None:
            make_queue(m)
        if graph:
            m.enable_step_graph()
        out.append((m, o))
    return out


def test_step_graph_with_a_restored_half_filled_queue(accurate_precision):
    """after ``set_queue`` with a NOT yet full queue (a restored checkpoint) the queue's fullness is unknown to the host; the
    step must ask the device - a synchronisation no capture can hold - so those steps stay eager until the FIFO is full, and the run equals
    the eager one bit for bit (it used to die in the capture at its second step)."""
    bs, fs = 2, 2
    Q = bs * 10 * 5
    half = torch.zeros(Q, 256)
    half[: Q // 2] = torch.nn.functional.normalize(torch.randn(Q // 2, 256, generator=torch.Generator().manual_seed(3)), dim=1)

    def mq(m):
        m.init_queue(Q)
        m.set_queue(half.cuda())

    clips = [torch.from_numpy(synth.make_clips(bs, fs, 224, seed=80 + i)).cuda() for i in range(7)]
    res = []
    for m, o in _small_graph_pair(mq, teacher=True):
        torch.manual_seed(7)
        losses = []
        for i, x in enumerate(clips):
            loss = m.get_loss(x)
            m.train_update(o, loss, i + 1)
            losses.append(loss.item())
        res.append((m, losses))
    (me, le), (mg, lg) = res
    assert le == lg, (le, lg)
    assert torch.equal(me.queue, mg.queue)
    assert len(mg._step_graphs) == 1 and not mg._step_graph_failed   # the full-queue signature, captured once the device said "full"


def test_step_graph_two_losses_per_update(accurate_precision):
    """the capture must not freeze the host's staleness decision.  Two ``get_loss`` calls per update (a probe forward, gradient
    statistics): the second call is the one that gets captured, at a moment when no weight is stale - the captured step converts the
    trainable weights' pair operands all the same, so the replays after the following updates see the updated weights."""
    bs, fs = 2, 2
    clips = [torch.from_numpy(synth.make_clips(bs, fs, 224, seed=90 + i)).cuda() for i in range(5)]
    res = []
    for m, o in _small_graph_pair():
        losses = []
        for i, x in enumerate(clips):
            probe = m.get_loss(x).item()          # no backward, no update
            loss = m.get_loss(x)
            m.train_update(o, loss, 0)
            losses.append((probe, loss.item()))
        res.append((m, losses))
    (me, le), (mg, lg) = res
    assert le == lg, (le, lg)
    assert all(a == b for a, b in le), le       # (the probe IS the step's loss: same weights, same clip)
    pe, pg = dict(me.named_parameters()), dict(mg.named_parameters())
    assert all(torch.equal(pe[n], pg[n]) for n in pe)
    assert len(mg._step_graphs) == 1


def test_step_graph_refuses_silent_gradient_accumulation():
    """a captured step's gradients are the graph's static buffers.  Accumulating over two steps without ``zero_grad`` would add
    the second gradient to a buffer the second replay has already overwritten (2 x g2 instead of g1 + g2): the backward raises instead."""
    from timetuning_amd import hip_ops

    hip_ops.set_gemm_precision("f16x3")
    try:
        (_, _), (m, o) = _small_graph_pair()
        x = torch.from_numpy(synth.make_clips(2, 2, 224, seed=5)).cuda()
        for i in range(3):                         # eager, captured, replayed - with zero_grad in between: fine
            m.zero_grad(set_to_none=True)
            m.get_loss(x).backward()
        with pytest.raises(RuntimeError, match="accumulation"):
            m.get_loss(x).backward()
    finally:
        hip_ops.set_gemm_precision("f32")


@pytest.mark.timeout(900)
@pytest.mark.parametrize("cfg", ["c2", "c3"])
def test_two_streams_equal_one_stream(cfg):
    """Round 6: the frozen blocks as two half batches on two HIP streams and the trainable blocks' kept / non-kept chains
    concurrently (engine.TWO_STREAMS) compute what one stream computes.  Frames are independent, so with the one decomposition-dependent
    accumulation order taken out (the K-split of the left-over tiles of the persistent pair GEMM, knob TT_Q8_KSPLIT = 0) three training
    steps at BASELINE C2 / C3 size are BIT FOR BIT equal (losses, all gradients, all parameters); with the K-split as shipped the two runs
    differ by fp32 rounding on the rows of those tiles only: relative L2 of every gradient < 2e-6.  (In that second part the two-stream run
    takes the one-stream run's HARD LABELS: one of the 6 272 arg-maxes over the propagated maps is a near-tie inside fp32 rounding at step 3
    of this seed, and one flipped label moves a gradient by 1.5e-2 - tools/probes/two_stream_labels.py; its own labels may differ from
    them in at most 0.1 % of the patches.)"""
    from timetuning_amd import engine, hip_ops
    from tools.graph_vs_eager import CONFIGS, make

    arch, bs, fs, K, queue = CONFIGS[cfg]
    hip_ops.set_gemm_precision("f16x3")
    keep = engine.TWO_STREAMS
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=12)).cuda()
    try:
        for ksplit, exact in ((0, True), (1, False)):
            with hip_ops.tuning_knob("TT_Q8_KSPLIT", ksplit):
                runs = []
                labels = []
                for two in (False, True):
                    engine.TWO_STREAMS = two
                    m, o = make(cfg, 8)
                    torch.manual_seed(5)
                    losses = []
                    for i in range(3):
                        pin = labels[i] if (two and not exact) else None
                        loss = m.get_loss(x, target_labels=pin)
                        if not two:
                            labels.append(m.last_aux["labels"].clone())
                        elif pin is not None:
                            assert (m.last_aux["labels"] != pin).float().mean().item() <= 1e-3
                        m.train_update(o, loss, i + 1 if queue else 0)
                        losses.append(loss.item())
                    runs.append((m, losses, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
                (m1, l1, g1), (m2, l2, g2) = runs
                if exact:
                    assert l1 == l2, (cfg, l1, l2)
                    assert all(torch.equal(g1[n], g2[n]) for n in g1)
                    p1, p2 = dict(m1.named_parameters()), dict(m2.named_parameters())
                    assert all(torch.equal(p1[n], p2[n]) for n in p1)
                else:
                    assert max(abs(a - b) for a, b in zip(l1, l2)) < 2e-5, (l1, l2)
                    worst = max(rel_l2(g2[n], g1[n]) for n in g1)
                    assert worst < 2e-6, worst
    finally:
        engine.TWO_STREAMS = keep
        hip_ops.set_gemm_precision("f32")


def test_c2_size_properties():
    """BASELINE C2 (bs 32 x 4 frames, K=200): too big for golden tensors; checked through invariants and against
    the CPU oracle on a sub-batch (per-clip computations are independent except for the Sinkhorn coupling)."""
    from oracle import timet_oracle as O
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    bs, fs, K = 32, 4, 200
    fe = FeatureExtractor("dino-s16", "", [1024, 1024, 512, 256], unfreeze_layers=["blocks.11", "blocks.10"], init="stress",
                          return_attention=False)
    model = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, 256))).cuda()
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=3))
    loss = model.get_loss(x.cuda())
    loss.backward()
    aux = model.last_aux
    q = aux["q"].reshape(bs * 196, K)
    assert rel_err(q.sum(1).cpu(), torch.ones(bs * 196)) < 1e-5
    col = q.double().sum(0)
    assert (col.max() / col.min()).item() < 1.05                     # equipartition over prototypes
    assert np.isfinite(loss.item()) and abs(loss.item() - np.log(K)) < 1.5
    # oracle on the same inputs: features of two clips, and the full loss given the GPU's q (bypasses the coupling)
    om = O.build_oracle("dino-s16", K, (1024, 1024, 512, 256), mode="stress")
    sub = x[:2].reshape(2 * fs, 3, 224, 224)
    with torch.no_grad():
        of, _ = om.feature_extractor(sub, faithful=False)
    mf, _ = model.feature_extractor(sub.cuda())
    assert_close(mf.cpu(), of, TOL, "C2 patch embeddings (2-clip sub-batch)")
    g = torch.cat([p.grad.reshape(-1) for p in model.parameters() if p.grad is not None])
    assert torch.isfinite(g).all() and g.abs().max() > 0


@pytest.mark.timeout(900)
def test_c2_full_step_vs_oracle(accurate_precision):
    """BASELINE C2 at FULL size (ViT-S/16, 32 clips x 4 frames, 200 prototypes): the whole training step against the CPU oracle
    (one pass per frame, ``faithful=False``: same arithmetic as the reference's four) - Sinkhorn assignment of all 6272 source
    patches, hard labels, loss, and the gradient of EVERY trainable tensor (prototypes, head, blocks 10 / 11, final norm) in
    relative L2.  The oracle's step is computed once per session and shared by the three modes."""
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    bs, fs, K = 32, 4, 200
    fe = FeatureExtractor("dino-s16", "", [1024, 1024, 512, 256], unfreeze_layers=["blocks.11", "blocks.10"], init="stress",
                          return_attention=False)
    model = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, 256))).cuda()
    o = _c2_oracle_step()
    loss = model.get_loss(o["x"].cuda(), target_labels=o["labels"])
    loss.backward()
    assert rel_err(model.last_aux["q"].cpu(), o["batch_q"]) < TOL and rel_l2(model.last_aux["q"].cpu(), o["batch_q"]) < TOL
    assert_close(model.last_aux["target_scores"].cpu(), o["target_scores"], TOL, "C2 assignment logits")
    mism = (model.last_aux["labels"].cpu() != o["labels"]).float().mean().item()
    assert mism <= 0.01, mism
    assert abs(loss.item() - o["loss"]) < 2e-4, (loss.item(), o["loss"])
    n = assert_all_grads(dict(model.named_parameters()), o["grads"], f"C2 full step [{accurate_precision}]")
    assert n == 33, n   # prototypes + 8 head tensors + 2 x 12 block tensors (the final norm is frozen with the rest of the backbone)


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("bs,steps", [(4, 2), (32, 1)])
def test_c3_per_rank_workload_vs_oracle(accurate_precision, bs, steps):
    """BASELINE C3's per-rank work at ViT-S/16 size: EMA teacher + a pre-filled 2048-row queue (16384 // 8 ranks,
    time_tuning.py:618) + 200 prototypes against the oracle: assignment, labels, loss, gradients, updated parameters, teacher
    and queue.  4 clips x TWO optimizer steps (the teacher used by step 2 is an EMA product and the queue has been shifted once), and
    C3's FULL per-rank batch - 32 clips, the 6272 + 2048-row Sinkhorn problem - for one step, in EVERY fp32-class mode (round 5: the
    oracle's steps are computed once per session); every trainable gradient in relative L2."""
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.my_utils import cosine_scheduler
    from timetuning_amd.time_tuning import SwavOptimizer, TimeT

    fs, K, Q, E, I = 4, 200, 2048, 1, 4
    fe = FeatureExtractor("dino-s16", "", [1024, 1024, 512, 256], unfreeze_layers=["blocks.11", "blocks.10"], init="stress",
                          return_attention=False)
    model = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, 256))).cuda()
    opt = SwavOptimizer(model, "AdamW", True, 1e-5, 1e-4, "CosineAnnealingLR", cosine_scheduler(0.04, 0.4, E, I), I, E)
    model.init_momentum_teacher()
    model.set_momentum_teacher_schedular_params(0.995, 1.0, E, I)
    model.init_queue(Q)
    model.queue.copy_(_c3_queue_fill(Q))
    assert model.queue_is_full()
    recs = _c3_oracle_steps(bs, steps)   # (once per session: shared by the three modes)
    for s_, o in enumerate(recs):
        x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=70 + s_))
        loss = model.get_loss(x.cuda(), queue_perm=o["perm"], target_labels=o["labels"])
        assert rel_err(model.last_aux["q"].cpu(), o["batch_q"]) < TOL, s_
        mism = (model.last_aux["labels"].cpu() != o["labels"]).float().mean().item()
        assert mism <= 0.01, (s_, mism)
        opt.step(loss)
        assert abs(loss.item() - o["loss"]) < 2e-4, (s_, loss.item(), o["loss"])
        mg = dict(model.named_parameters())
        assert_all_grads(mg, o["grads"], f"C3 bs={bs} step {s_} [{accurate_precision}]")
        model.normalize_prototypes()
        model.update_momentum_teacher(opt.global_step)
        for name in C3_WATCH:
            assert rel_err(mg[name].detach().cpu(), o["params"][name]) < 1e-4, (s_, name)
        assert rel_err(model.queue.cpu(), o["queue"]) < 1e-4
        assert rel_err(model.teacher_prototypes.detach().cpu(), o["teacher_prototypes"]) < 1e-4
        tw = dict(model.teacher.named_parameters())["backbone.blocks.11.mlp.fc2.weight"].detach().cpu()
        assert rel_err(tw, o["teacher_fc2"]) < 1e-4


def test_use_mask_full_size_vs_oracle():
    """--use_mask at ViT-S/16 size with the "stress" weights and white-noise clips: speckled attention, so the masks DO
    contain 1- and 2-pixel components (the case the reference cannot process, models.py:127-130) and their removal is
    exercised end to end against the oracle's intended behaviour."""
    from oracle import timet_oracle as O
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    K, bs, fs = 50, 2, 2
    fe = FeatureExtractor("dino-s16", "", [1024, 1024, 512, 256], unfreeze_layers=["blocks.11", "blocks.10"], init="stress",
                          return_attention=False)
    model = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, 256))).cuda()
    om = O.build_oracle("dino-s16", K, (1024, 1024, 512, 256), mode="stress")
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=11))
    loss = model.get_loss(x.cuda(), mask_features=True)
    loss.backward()
    with torch.no_grad():
        _, aux = om.get_loss(x, return_aux=True, mask_features=True)
    om_masks = aux["masks"].reshape(bs, fs, -1)
    # the oracle's thresholded maps before component removal would differ from these where small components existed
    with torch.no_grad():
        _, attn = om.feature_extractor(x.view(bs * fs, 3, 224, 224))
    att = attn[:, :, 0, 1:].mean(1).reshape(bs * fs, 1, 14, 14)
    bl = O.gaussian_blur(att).reshape(bs * fs, -1)
    val, idx = torch.sort(bl)
    cum = torch.cumsum(val / val.sum(-1, keepdim=True), -1)
    raw = torch.gather((cum > 0.35).float(), 1, torch.argsort(idx)).reshape(bs, fs, -1)
    assert (raw != om_masks).any(), "the inputs were chosen so that small components exist"
    tm, sm = model.last_aux["target_mask"].cpu(), model.last_aux["source_mask"].cpu()
    mism = ((tm != om_masks[:, -1]).float().mean() + (sm != om_masks[:, 0]).float().mean()).item() / 2
    assert mism <= 0.005
    lab_mism = (model.last_aux["labels"].cpu() != aux["labels"].reshape(bs, -1)).float().mean().item()
    assert lab_mism <= 0.01 or mism > 0
    # loss and gradients, unconditionally: the oracle is re-run with the two discontinuous decisions (foreground masks, hard
    # labels) pinned to the GPU's, so a flipped mask pixel or label cannot switch the comparison off
    oloss = om.get_loss(x, mask_features=True, masks_override=(sm, tm), labels_override=model.last_aux["labels"].cpu())
    oloss.backward()
    assert abs(loss.item() - oloss.item()) < 2e-4
    op = dict(om.named_parameters())
    for name, p in model.named_parameters():
        if p.grad is not None and name in ("prototypes", "feature_extractor.head.6.weight",
                                           "feature_extractor.backbone.blocks.10.attn.qkv.weight"):
            assert rel_err(p.grad.cpu(), op[name].grad) < TOL, name


def test_reference_named_methods_vs_oracle(golden):
    """The delegating methods a caller of the reference would use directly - get_feature_prototype_similarity, get_scores (with
    and without a full queue, student and teacher prototypes), find_optimal_assignment, make_seg_maps, the
    PatchPrototypeSimilarity module, reshape_to_spatial_resolution - against the oracle's restatements."""
    from oracle import timet_oracle as O

    g = golden("timet_tiny_tq")
    model, _ = _build(g, True, 40)
    D, depth, heads, patch = [int(v) for v in g["vit_cfg"]]
    om = O.build_oracle("dino-s16", int(g["cfg"][2]), tuple(int(v) for v in g["head_list"]), mode=str(g["mode"]),
                        vit_cfg=dict(embed_dim=D, depth=depth, num_heads=heads, patch_size=patch))
    om.init_momentum_teacher()
    om.init_queue(40)
    bs, fs = int(g["cfg"][0]), int(g["cfg"][1])
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=1)).view(bs * fs, 3, 224, 224)
    with torch.no_grad():
        of, _ = om.feature_extractor(x, faithful=False)
        obf, _ = om.feature_extractor(x, use_head=False, faithful=False)
    f, _ = model.feature_extractor(x.cuda())
    with torch.no_grad():
        n, dim = f.shape[1], f.shape[2]
        feats, ofeats = f.view(bs, fs, n, dim)[:, 0].contiguous(), of.view(bs, fs, n, dim)[:, 0].contiguous()
        # similarity (student / teacher prototypes)
        for use_teacher in (False, True):
            sc = model.get_feature_prototype_similarity(feats.reshape(-1, dim), use_teacher)
            assert rel_err(sc.cpu(), om.get_feature_prototype_similarity(ofeats.reshape(-1, dim), use_teacher)) < TOL
        # get_scores without a full queue, then with one (the queue rows join the Sinkhorn problem, :207-211)
        q, sc = model.get_scores(feats, 0.05, 10)
        oq, osc = om.get_scores(ofeats, 0.05, 10)
        assert q.shape == (bs, n, om.prototypes.shape[0]) and rel_err(q.cpu(), oq) < TOL and rel_err(sc.cpu(), osc) < TOL
        fill = torch.from_numpy(synth.normal("rnm.queue", (40, dim)))
        model.queue.copy_(fill)
        om.queue.copy_(fill)
        q2, _ = model.get_scores(feats, 0.05, 10, use_teacher=True)
        oq2, _ = om.get_scores(ofeats, 0.05, 10, use_teacher=True)
        assert rel_err(q2.cpu(), oq2) < TOL and rel_err(q2.cpu(), oq) > 1e-3       # the queue changed the assignment
        q3, sc3 = model.similarity(feats, use_teacher=True)                          # the PatchPrototypeSimilarity module itself
        assert torch.equal(q3, q2)
        # find_optimal_assignment and make_seg_maps
        qa = model.find_optimal_assignment(sc.reshape(-1, sc.shape[-1]), 0.05, 3)
        assert rel_err(qa.cpu(), om.find_optimal_assignment(osc.reshape(-1, osc.shape[-1]), 0.05, 3)) < TOL
        bf, _ = model.feature_extractor(x.cuda(), use_head=False)
        maps = model.make_seg_maps(q[0], bf.view(bs, fs, n, -1)[0], 7, 6, 5, features_exist=True)
        omaps = om.make_seg_maps(oq[0], obf.view(bs, fs, n, -1)[0], 7, 6, 5)
        got, want = maps[-1].cpu().numpy(), omaps[-1].numpy()
        bad = np.abs(got - want).reshape(got.shape[0], -1).max(0) > 1e-4 * np.abs(want).max()
        assert bad.mean() <= 0.01
        r = model.reshape_to_spatial_resolution(q[0], 14)
        assert r.shape == (q.shape[-1], 14, 14) and torch.equal(r[:, 3, 5], q[0][3 * 14 + 5])


def test_propagate_labels_from_frames(golden):
    """mask_propagation.propagate_labels with features_exist=False: the frames go through the extractor first (:462-466), and
    the result equals the features_exist=True call on those features."""
    from timetuning_amd import mask_propagation as MP

    g = golden("timet_tiny")
    model, _ = _build(g)
    frames = torch.from_numpy(synth.make_clips(1, 3, 224, seed=9))[0].cuda()
    seed = torch.softmax(torch.from_numpy(synth.normal("plf.seed", (1, 6, 14, 14))) * 2, dim=1).cuda()
    a = MP.propagate_labels(7, 6, 5, model, frames, seed, features_exist=False)
    feats, _ = model.feature_extractor(frames, use_head=False)
    b = MP.propagate_labels(7, 6, 5, model, feats, seed, features_exist=True)
    assert len(a) == len(b) == 2 and all(torch.equal(u, v) for u, v in zip(a, b)) and a[0].shape == (6, 14, 14)


def test_ten_training_steps_track_the_oracle():
    """Ten consecutive iterations (teacher + queue, which fills after two steps so the queue branch of the Sinkhorn is live from
    step 3) on the tiny ViT, GPU vs CPU oracle fed the same clips and queue permutations: the loss trajectories stay together
    and the final parameters agree - no drift from accumulated rounding, stale buffers or state that only shows after step 3."""
    from oracle import timet_oracle as O
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.my_utils import cosine_scheduler
    from timetuning_amd.time_tuning import SwavOptimizer, TimeT

    cfg = synth.ARCHS["tiny-s16"]
    K, head, bs, fs, steps, E, I = 20, (128, 128, 64, 32), 2, 3, 10, 1, 12
    fe = FeatureExtractor("dino-s16", "", list(head), unfreeze_layers=["blocks.11", "blocks.10"], vit_cfg=cfg, init="stress", return_attention=False)
    model = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, fe.feature_dim))).cuda()
    opt = SwavOptimizer(model, "AdamW", True, 1e-5, 1e-4, "CosineAnnealingLR", cosine_scheduler(0.04, 0.4, E, I), I, E)
    model.init_momentum_teacher()
    model.set_momentum_teacher_schedular_params(0.995, 1.0, E, I)
    model.init_queue(40)
    om = O.build_oracle("dino-s16", K, head, mode="stress", vit_cfg=cfg)
    oopt = O.SwavOptimizerOracle(om, 1e-5, 1e-4, O.cosine_scheduler(0.04, 0.4, E, I), I, E)
    om.init_momentum_teacher()
    om.set_momentum_teacher_schedular_params(0.995, 1.0, E, I)
    om.init_queue(40)
    gpu_losses, cpu_losses = [], []
    for s in range(steps):
        x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=50 + s))
        perm = torch.randperm(bs * 196, generator=torch.Generator().manual_seed(s)).numpy()
        loss = model.get_loss(x.cuda(), queue_perm=perm)
        opt.step(loss)
        model.normalize_prototypes()
        model.update_momentum_teacher(opt.global_step)
        oloss = om.get_loss(x, queue_perm=perm, faithful=False)
        oopt.zero_grad()
        oloss.backward()
        oopt.step()
        om.normalize_prototypes()
        om.update_momentum_teacher(oopt.global_step)
        gpu_losses.append(loss.item())
        cpu_losses.append(oloss.item())
    assert model.queue_is_full()
    np.testing.assert_allclose(gpu_losses, cpu_losses, rtol=5e-3)
    assert rel_err(model.prototypes.detach().cpu(), om.prototypes.detach()) < 1e-3
    assert rel_err(model.teacher_prototypes.detach().cpu(), om.teacher_prototypes) < 1e-3
    assert rel_err(model.queue.cpu(), om.queue) < 1e-3
    w = dict(model.named_parameters())["feature_extractor.backbone.blocks.11.mlp.fc2.weight"].detach().cpu()
    assert rel_err(w, om.feature_extractor.backbone["blocks.11.mlp.fc2.weight"].detach()) < 1e-4


def test_teacher_reuses_student_frozen_blocks_only_when_they_are_equal():
    """The EMA teacher pass continues from the student's activations at the first trainable block when - and only when - the
    teacher's frozen tensors equal the student's bit for bit (the reference's deepcopy teacher, time_tuning.py:96); a teacher
    whose frozen weights differ takes the full pass and the full EMA.  Both against the oracle."""
    from oracle import timet_oracle as O
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    cfg, head, K, bs, fs = synth.ARCHS["tiny-s16"], (128, 128, 64, 32), 20, 2, 3
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=31))
    delta = torch.from_numpy(synth.normal("teacher.delta", (4 * cfg["embed_dim"], cfg["embed_dim"]), 0.05))
    for perturbed in (False, True):
        fe = FeatureExtractor("dino-s16", "", list(head), unfreeze_layers=["blocks.11", "blocks.10"], vit_cfg=cfg, init="stress", return_attention=False)
        model = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, fe.feature_dim))).cuda()
        om = O.build_oracle("dino-s16", K, head, mode="stress", vit_cfg=cfg)
        for m_ in (model, om):
            m_.init_momentum_teacher()
            m_.set_momentum_teacher_schedular_params(0.9, 1.0, 1, 4)
        if perturbed:
            with torch.no_grad():
                model.teacher.backbone.blocks[3].mlp.fc1.weight.add_(delta.cuda())
                om.teacher.backbone["blocks.3.mlp.fc1.weight"].add_(delta)
            model.invalidate_teacher_cache()
        assert model.teacher_shares_frozen_blocks() == (not perturbed)
        oloss, aux = om.get_loss(x, faithful=False, return_aux=True)
        oloss.backward()
        loss = model.get_loss(x.cuda(), target_labels=aux["labels"].reshape(bs, -1))
        loss.backward()
        assert rel_err(model.last_aux["q"].cpu(), aux["batch_q"]) < TOL, perturbed
        assert abs(loss.item() - oloss.item()) < 2e-4, perturbed
        model.update_momentum_teacher(1)
        om.update_momentum_teacher(1)
        tw = model.teacher.backbone.blocks[3].mlp.fc1.weight.detach().cpu()
        sw = model.feature_extractor.backbone.blocks[3].mlp.fc1.weight.detach().cpu()
        assert rel_err(tw, om.teacher.backbone["blocks.3.mlp.fc1.weight"]) < 1e-6
        assert torch.equal(tw, sw) == (not perturbed)      # shared: untouched and identical; else blended towards the student
        t11 = model.teacher.backbone.blocks[11].mlp.fc2.weight.detach().cpu()
        assert rel_err(t11, om.teacher.backbone["blocks.11.mlp.fc2.weight"]) < 1e-6


@pytest.mark.parametrize("use_head", [True, False])
def test_features_carry_grad_at_the_module_surface(use_head):
    """models.py:1070-1078: ``FeatureExtractor.forward`` returns features WITH grad (a caller such as linear_finetune.py:59-63
    trains through ``model(x)``); attentions never carry grad (:969).  Gradient of a random linear functional of the features
    against the oracle's autograd, for head, unfrozen-block and frozen parameters."""
    from oracle import timet_oracle as O
    from timetuning_amd.models import FeatureExtractor

    cfg, head = synth.ARCHS["tiny-s16"], (128, 128, 64, 32)
    fe = FeatureExtractor("dino-s16", "", list(head), unfreeze_layers=["blocks.11", "blocks.10"], vit_cfg=cfg, init="stress").cuda()
    om = O.build_oracle("dino-s16", 8, head, mode="stress", vit_cfg=cfg)
    x = torch.from_numpy(synth.make_clips(1, 3, 224, seed=41)).view(3, 3, 224, 224)
    f, attn = fe(x.cuda(), use_head=use_head)
    assert f.requires_grad and attn is not None and not attn.requires_grad
    of, oattn = om.feature_extractor(x, use_head=use_head, faithful=True)
    assert rel_err(f.detach().cpu(), of.detach()) < 1e-4 and rel_err(attn.cpu(), oattn) < 1e-4
    w = torch.from_numpy(synth.normal("surface.w", tuple(f.shape)))
    (f * w.cuda()).sum().backward()
    (of * w).sum().backward()
    og = {"feature_extractor." + k: v for k, v in om.feature_extractor.named_parameters()}
    mine = {"feature_extractor." + k: v for k, v in fe.named_parameters()}
    names = ["feature_extractor.backbone.blocks.10.attn.qkv.weight", "feature_extractor.backbone.blocks.11.norm2.weight",
             "feature_extractor.backbone.blocks.11.mlp.fc2.bias"]
    if use_head:
        names += ["feature_extractor.head.0.weight", "feature_extractor.head.6.bias"]
    for name in names:
        assert mine[name].grad is not None, name
        assert rel_err(mine[name].grad.cpu(), og[name].grad) < TOL, name
    assert mine["feature_extractor.backbone.blocks.3.mlp.fc1.weight"].grad is None          # frozen
    if not use_head:
        assert mine["feature_extractor.head.0.weight"].grad is None
    with torch.no_grad():                                                                    # and nothing is kept without grad
        f2, _ = fe(x.cuda(), use_head=use_head)
    assert not f2.requires_grad and torch.equal(f2, f.detach())


def test_similarity_scores_carry_grad():
    """time_tuning.py:130-141: ``get_feature_prototype_similarity`` is differentiable in the features and the prototypes."""
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    fe = FeatureExtractor("dino-s16", "", [64, 32], vit_cfg=synth.ARCHS["tiny-s16"], init="stress", return_attention=False)
    model = TimeT(fe, 24, prototype_init=torch.from_numpy(synth.make_prototypes(24, 32))).cuda()
    z = torch.from_numpy(synth.normal("sim.z", (200, 32)))
    w = torch.from_numpy(synth.normal("sim.w", (200, 24)))
    zg = z.clone().cuda().requires_grad_(True)
    sc = model.get_feature_prototype_similarity(zg)
    assert sc.requires_grad
    (sc * w.cuda()).sum().backward()
    zc, pc = z.clone().requires_grad_(True), model.prototypes.detach().cpu().clone().requires_grad_(True)
    ref = torch.nn.functional.normalize(zc, dim=-1) @ pc.t()
    (ref * w).sum().backward()
    assert rel_err(sc.detach().cpu(), ref.detach()) < 1e-5
    assert rel_err(zg.grad.cpu(), zc.grad) < 1e-4 and rel_err(model.prototypes.grad.cpu(), pc.grad) < 1e-4
    sct = model.get_feature_prototype_similarity(zg.detach(), use_teacher=False)            # prototypes alone still require grad
    assert sct.requires_grad


def test_mask_propagation_evaluation_vs_oracle():
    """N4: the evaluation loop body (extractor without head -> propagate_labels(4, 12, 5) -> upsample -> arg-max -> J) on a
    synthetic tracking clip, against the oracle fed with the same features; and the command-line driver."""
    from oracle import timet_oracle as O
    from timetuning_amd import mask_propagation as MP
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    fe = FeatureExtractor("dino-s16", "", [1024, 1024, 512, 256], init="stress", return_attention=False)
    model = TimeT(fe, 10).cuda().eval()
    fs, R, C = 7, 224, 3
    clip, masks = MP.synthetic_tracking_clip(fs, R, seed=1)
    pred = MP.propagate_clip(model, clip.cuda(), masks[0].cuda(), 4, 12, 5, R, C)
    assert pred.shape == (fs - 1, R, R) and pred.dtype == torch.int64
    feats, _ = model(clip.cuda(), use_head=False)
    want, margin, _ = O.propagate_clip_predictions(4, 12, 5, 14, feats.cpu(), masks[0], R, C, return_margin=True)
    mism = pred.cpu() != want
    assert mism.float().mean().item() <= 0.005
    assert (margin[mism] < 1e-3).all()       # flips only where the top-2 upsampled scores are close (a top-k near-tie upstream)
    j_gpu, _ = MP.jaccard(pred, masks[1:].cuda(), C)
    j_cpu = O.jaccard(want, masks[1:], C)
    assert abs(j_gpu - j_cpu) < 0.01 and j_gpu > 0.3
    args = MP.build_parser().parse_args(["--dataset", "synthetic", "--model_path", "", "--num_frames", "5", "--num_clips", "2"])
    assert args.n_last_frames == 4 and args.size_mask_neighborhood == 12 and args.topk == 5   # the reference's defaults
    assert np.isfinite(MP.mask_propagation(args))


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("arch,K,bs,fs", [("dino-b16", 40, 1, 2), ("dino-s8", 40, 1, 2), ("dino-b16", 400, 1, 8), ("dino-s8", 200, 1, 4),
                                          ("dino-b16", 400, 4, 8), ("dino-s8", 200, 4, 4)])
def test_other_architectures_vs_oracle(arch, K, bs, fs):
    """ViT-B/16 (D=768, 12 heads) and ViT-S/8 (785 tokens: KV-tiled attention, 28x28 propagation grid) against the oracle:
    extractor outputs and one full loss + gradient - at a small shape and at the clip length / prototype count of BASELINE's
    configs C4 (ViT-B/16, 8 frames, 400 prototypes) and C5 (ViT-S/8, 4 frames, 200 prototypes), one clip each, and (round 6: VERDICT r5
    weak 9) FOUR clips each: 6 304 / 12 560 token rows, where the persistent pair GEMMs, the transpose-free weight gradients and - on
    ViT-S/8 - the KV-tiled attention run at multi-round grids; all 33 gradients against the oracle's in both modes."""
    from oracle import timet_oracle as O
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    fe = FeatureExtractor(arch, "", [1024, 1024, 512, 256], unfreeze_layers=["blocks.11", "blocks.10"], init="stress", return_attention=False)
    assert fe.spatial_resolution == (28 if arch == "dino-s8" else 14)
    model = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, 256))).cuda()
    om = O.build_oracle(arch, K, (1024, 1024, 512, 256), mode="stress")
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=5))
    with torch.no_grad():
        of, _ = om.feature_extractor(x.view(bs * fs, 3, 224, 224), faithful=False)
        obf, _ = om.feature_extractor(x.view(bs * fs, 3, 224, 224), use_head=False, faithful=False)
    f, _ = model.feature_extractor(x.view(bs * fs, 3, 224, 224).cuda())
    bf, _ = model.feature_extractor(x.view(bs * fs, 3, 224, 224).cuda(), use_head=False)
    assert rel_err(f.cpu(), of) < TOL
    assert rel_err(bf.cpu(), obf) < TOL
    oloss, aux = om.get_loss(x, faithful=False, return_aux=True)
    oloss.backward()
    og = {n_: p_.grad for n_, p_ in om.named_parameters() if p_.grad is not None}
    from timetuning_amd import hip_ops
    for mode in ("f32", "f16x3"):   # the exact-f32 kernels and the headline arithmetic (launches of >= PAIRS_MIN_ROWS rows on pairs), one oracle step
        try:
            hip_ops.set_gemm_precision(mode)
            model.zero_grad(set_to_none=True)
            loss = model.get_loss(x.cuda(), target_labels=aux["labels"].reshape(bs, -1))   # the oracle's hard labels feed the CE
            loss.backward()
        finally:
            hip_ops.set_gemm_precision("f32")
        mism = (model.last_aux["labels"].cpu() != aux["labels"].reshape(bs, -1)).float().mean().item()
        assert mism <= 0.01
        assert rel_err(model.last_aux["q"].cpu(), aux["batch_q"]) < TOL
        assert abs(loss.item() - oloss.item()) < 2e-4
        assert_all_grads(dict(model.named_parameters()), og, f"{arch} K={K} fs={fs} [{mode}]")   # all 33 trainable tensors, relative L2


@pytest.mark.timeout(900)
@pytest.mark.parametrize("arch,K,bs,fs,mode,ftol", [("dino-b16", 400, 16, 8, "f16x3", TOL), ("dino-b16", 400, 16, 8, "bf16", 1.5e-2),
                                                    ("dino-s8", 200, 16, 4, "f16x3", TOL), ("dino-s8", 200, 16, 4, "f32", TOL)])
def test_c4_c5_full_per_gpu_batch(arch, K, bs, fs, mode, ftol):
    """BASELINE C4 (ViT-B/16, 8-frame clips, 400 prototypes) and C5 (ViT-S/8, 785 tokens) at the FULL per-GPU batch the bench times
    (16 clips): too big for the CPU oracle as a whole, so - as ``test_c2_size_properties`` does for C2 - the training step is checked
    through size-independent properties (assignment rows sum to one, prototypes equally loaded, finite non-zero gradients, a loss
    near ln K) and the extractor against the oracle on a 2-clip sub-batch (per-clip computations are independent), in the precision
    mode the bench line of that config runs in."""
    from oracle import timet_oracle as O
    from timetuning_amd import hip_ops
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    fe = FeatureExtractor(arch, "", [1024, 1024, 512, 256], unfreeze_layers=["blocks.11", "blocks.10"], init="stress", return_attention=False)
    model = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, 256))).cuda()
    n = fe.spatial_resolution ** 2
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=7))
    try:
        hip_ops.set_gemm_precision(mode)
        loss = model.get_loss(x.cuda())
        loss.backward()
        q = model.last_aux["q"].reshape(bs * n, K)
        assert rel_err(q.sum(1).cpu(), torch.ones(bs * n)) < 1e-5
        col = q.double().sum(0)
        assert (col.max() / col.min()).item() < 1.05
        assert np.isfinite(loss.item()) and abs(loss.item() - np.log(K)) < 1.5
        g = torch.cat([p.grad.reshape(-1) for p in model.parameters() if p.grad is not None])
        assert torch.isfinite(g).all() and g.abs().max() > 0
        om = O.build_oracle(arch, K, (1024, 1024, 512, 256), mode="stress")
        sub = x[:2].reshape(2 * fs, 3, 224, 224)
        with torch.no_grad():
            of, _ = om.feature_extractor(sub, faithful=False)
            mf, _ = model.feature_extractor(sub.cuda())
        if mode == "bf16":
            assert rel_err(mf.cpu(), of) < ftol and rel_l2(mf.cpu(), of) < ftol
        else:
            assert_close(mf.cpu(), of, ftol, f"{arch} patch embeddings (2-clip sub-batch, {mode})")
    finally:
        hip_ops.set_gemm_precision("f32")


def test_c4_shape_in_bf16_mode():
    """BASELINE config C4 names the "MFMA bf16 path": ViT-B/16, 8-frame clips, 400 prototypes.  One clip of that shape in the
    opt-in "bf16" mode of the forward Linears against the fp32 oracle, held to a bf16-sized bound (the mode cannot meet the
    1e-3 fp32 contract and is never the default); "bf16x3" on the same shape stays inside the fp32 contract."""
    from oracle import timet_oracle as O
    from timetuning_amd import hip_ops
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    K, bs, fs = 400, 1, 8
    fe = FeatureExtractor("dino-b16", "", [1024, 1024, 512, 256], unfreeze_layers=["blocks.11", "blocks.10"], init="stress", return_attention=False)
    model = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, 256))).cuda()
    om = O.build_oracle("dino-b16", K, (1024, 1024, 512, 256), mode="stress")
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=5))
    with torch.no_grad():
        of, _ = om.feature_extractor(x.view(bs * fs, 3, 224, 224), faithful=False)
        oloss, aux = om.get_loss(x, faithful=False, return_aux=True)
    olabels = aux["labels"].reshape(bs, -1)
    try:
        # (bf16: 3 x the error the bench line measures on this shape, 4.5e-3)
        for mode, ftol, ltol, flips in (("f16x3", 1e-4, 2e-4, 0.01), ("bf16x6", 1e-4, 2e-4, 0.01), ("bf16x3", 1e-3, 2e-3, 0.03), ("bf16", 1.5e-2, 0.15, 0.5)):
            hip_ops.set_gemm_precision(mode)
            with torch.no_grad():
                f, _ = model.feature_extractor(x.view(bs * fs, 3, 224, 224).cuda())
                loss = model.get_loss(x.cuda(), target_labels=olabels)      # hard labels pinned: the loss is then continuous
            assert rel_err(f.cpu(), of) < ftol, mode
            assert abs(loss.item() - oloss.item()) < ltol * abs(oloss.item()), (mode, loss.item(), oloss.item())
            assert (model.last_aux["labels"].cpu() != olabels).float().mean().item() <= flips, mode
    finally:
        hip_ops.set_gemm_precision("f32")


@pytest.mark.timeout(900)
def test_c4_bf16_step_gradients_vs_fp32_oracle():
    """BASELINE C4's "MFMA bf16 path" with its bf16 backward products, at C4's shape (ViT-B/16, one clip of 8 frames, 400
    prototypes), against the fp32 ORACLE - not against another run of the HIP path: loss, and the gradients of the prototypes, a
    head weight, a blocks.10 attention weight and a blocks.11 MLP weight.  bf16 carries 8 significant bits, so the bounds are
    bf16-sized and stated here: loss within 1 %, every gradient within 2 % of the oracle (relative L2 error) and at cosine > 0.9995 with it
    (measured on MI355X, round 3: loss 5.97655 vs 5.97659, gradient errors 0.3-0.7 %, cosines >= 0.99997; the test prints them).  The hard labels are the oracle's, so the loss and its
    gradients are continuous functions of the features."""
    from oracle import timet_oracle as O
    from timetuning_amd import hip_ops
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    K, bs, fs = 400, 1, 8
    fe = FeatureExtractor("dino-b16", "", [1024, 1024, 512, 256], unfreeze_layers=["blocks.11", "blocks.10"], init="dino", return_attention=False)
    model = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, 256))).cuda()
    om = O.build_oracle("dino-b16", K, (1024, 1024, 512, 256), mode="dino")
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=5))
    oloss, aux = om.get_loss(x, faithful=False, return_aux=True)
    oloss.backward()
    og = dict(om.named_parameters())
    names = ("prototypes", "feature_extractor.head.0.weight", "feature_extractor.backbone.blocks.10.attn.qkv.weight",
             "feature_extractor.backbone.blocks.11.mlp.fc2.weight")
    try:
        hip_ops.set_gemm_precision("bf16")
        loss = model.get_loss(x.cuda(), target_labels=aux["labels"].reshape(bs, -1))
        loss.backward()
    finally:
        hip_ops.set_gemm_precision("f32")
    mg = dict(model.named_parameters())
    print(f"\nC4 bf16 vs fp32 oracle: loss {loss.item():.5f} / {oloss.item():.5f}")
    assert abs(loss.item() - oloss.item()) < 0.01 * abs(oloss.item()), (loss.item(), oloss.item())
    for n in names:
        a_, b_ = mg[n].grad.double().cpu().flatten(), og[n].grad.double().flatten()
        cos = float(torch.dot(a_, b_) / (a_.norm() * b_.norm()))
        ratio = float(a_.norm() / b_.norm())
        print(f"  {n}: cosine {cos:.5f}  norm ratio {ratio:.4f}  rel err {float((a_ - b_).norm() / b_.norm()):.4f}")
        assert cos > 0.9995 and float((a_ - b_).norm() / b_.norm()) < 0.02, (n, cos, ratio)


@pytest.mark.parametrize("mode,feat_tol", [("bf16x3", 1e-3), ("bf16", 6e-2)])
def test_precision_modes_end_to_end(golden, mode, feat_tol):
    """The opt-in bf16 MFMA modes of the forward Linears against the reference's numbers (tiny ViT golden fixture):
    "bf16x3" (split precision) must stay inside the north-star 1e-3 bound on embeddings, logits and loss; plain "bf16"
    (BASELINE C4's path) is held to a bf16-sized bound.  f32 is restored afterwards."""
    from timetuning_amd import hip_ops

    g, a = golden("timet_tiny"), golden("aux_tiny")
    model, _ = _build(g)
    bs, fs = int(g["cfg"][0]), int(g["cfg"][1])
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=1)).cuda()
    try:
        hip_ops.set_gemm_precision(mode)
        f, _ = model.feature_extractor(x.view(bs * fs, 3, 224, 224))
        bf, _ = model.feature_extractor(x.view(bs * fs, 3, 224, 224), use_head=False)
        loss = model.get_loss(x)
        scores = model.last_aux["target_scores"].cpu()
    finally:
        hip_ops.set_gemm_precision("f32")
    assert rel_err(f.cpu(), g["features"]) < feat_tol
    assert rel_err(bf.cpu(), g["backbone_features"]) < feat_tol
    assert rel_err(scores, a["target_scores"]) < feat_tol
    if mode == "bf16x3":
        assert abs(loss.item() - float(g["loss0"])) < 1e-3 * float(g["loss0"])
    else:
        assert abs(loss.item() - float(g["loss0"])) < 0.1


@pytest.mark.parametrize("bs,fs,K,teacher,queue", [(1, 2, 8, False, 0), (3, 5, 30, False, 0), (5, 3, 21, True, 0), (2, 9, 12, False, 30),
                                                   (4, 2, 200, True, 64)])
def test_ragged_configurations_vs_oracle(bs, fs, K, teacher, queue):
    """Odd batch sizes, clip lengths (fs = 9 exercises the 7-frame context ring of propagate_labels), prototype counts that
    are not multiples of 4 (element-load GEMM path), teacher and queue: loss, labels and gradients against the oracle."""
    from oracle import timet_oracle as O
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    cfg, head = synth.ARCHS["tiny-s16"], (128, 128, 64, 32)
    fe = FeatureExtractor("dino-s16", "", list(head), unfreeze_layers=["blocks.11", "blocks.10"], vit_cfg=cfg, init="stress", return_attention=False)
    model = TimeT(fe, K, prototype_init=torch.from_numpy(synth.make_prototypes(K, fe.feature_dim))).cuda()
    om = O.build_oracle("dino-s16", K, head, mode="stress", vit_cfg=cfg)
    if teacher:
        model.init_momentum_teacher()
        om.init_momentum_teacher()
    if queue:
        model.init_queue(queue)
        om.init_queue(queue)
        fill = torch.from_numpy(synth.normal("ragged.queue", (queue, 32)))
        model.queue.copy_(fill)
        om.queue.copy_(fill)
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=7))
    perm = torch.randperm(bs * 196)
    oloss, aux = om.get_loss(x, faithful=False, return_aux=True, queue_perm=perm)
    oloss.backward()
    loss = model.get_loss(x.cuda(), queue_perm=perm, target_labels=aux["labels"].reshape(bs, -1))
    loss.backward()
    assert rel_err(model.last_aux["q"].cpu(), aux["batch_q"]) < TOL
    mism = (model.last_aux["labels"].cpu() != aux["labels"].reshape(bs, -1)).float().mean().item()
    assert mism <= 0.01
    assert abs(loss.item() - oloss.item()) < 2e-4
    og, mg = dict(om.named_parameters()), dict(model.named_parameters())
    for name in ("prototypes", "feature_extractor.head.0.weight", "feature_extractor.backbone.blocks.11.mlp.fc2.weight",
                 "feature_extractor.backbone.blocks.10.norm1.weight"):
        assert rel_err(mg[name].grad.cpu(), og[name].grad) < TOL, name
    if queue:
        assert rel_err(model.queue.cpu(), om.queue) < 1e-4


def test_bf16x3_full_size_c1(golden):
    """Split-bf16 forward Linears on the full-size ViT-S/16 C1 fixture: patch embeddings, head features and loss stay inside
    the north-star 1e-3 bound against the reference's own numbers."""
    from timetuning_amd import hip_ops

    g = golden("timet_c1")
    model, _ = _build(g)
    bs, fs = int(g["cfg"][0]), int(g["cfg"][1])
    x = torch.from_numpy(synth.make_clips(bs, fs, 224, seed=1)).cuda()
    try:
        hip_ops.set_gemm_precision("bf16x3")
        f, _ = model.feature_extractor(x.view(bs * fs, 3, 224, 224))
        bf, _ = model.feature_extractor(x.view(bs * fs, 3, 224, 224), use_head=False)
        loss = model.get_loss(x)
    finally:
        hip_ops.set_gemm_precision("f32")
    assert_close(f[:, ::49, ::16].cpu(), g["features_slice"], TOL, "C1 patch embeddings (slice)")
    assert_close(bf[:, ::49, ::16].cpu(), g["backbone_features_slice"], TOL, "C1 backbone features (slice)")
    assert abs(loss.item() - float(g["loss0"])) < 1e-3 * float(g["loss0"])


def test_graft_entry_smoke():
    """The driver's smoke(): one tiny training iteration on cuda:0 checked against the oracle (__graft_entry__.py)."""
    import importlib.util, os

    spec = importlib.util.spec_from_file_location("graft_entry", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.smoke()
