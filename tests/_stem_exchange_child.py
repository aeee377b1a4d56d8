"""Child process of tests/test_hip_stem_grad.py::test_stem_gradients_through_the_exchange_path: the training step with everything
trainable on the exchange path (one-rank RCCL communicator, TT_EXCHANGE_SINGLE_RANK=1: the very calls of an N-GPU rank - from the second
step on the stem's kernels write the exchange's flat buckets directly) against the plain one-process step.  Prints one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import timetuning_amd  # noqa: E402,F401
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from timetuning_amd import synth  # noqa: E402
from timetuning_amd.models import FeatureExtractor  # noqa: E402
from timetuning_amd.my_utils import cosine_scheduler  # noqa: E402
from timetuning_amd.time_tuning import SwavOptimizer, TimeT  # noqa: E402

STEM = ("patch_embed.proj.weight", "patch_embed.proj.bias", "cls_token", "pos_embed")


def make():
    fe = FeatureExtractor("dino-s16", "", [128, 128, 64, 32], unfreeze_layers=["blocks", "patch_embed", "pos_embed", "cls_token"],
                          vit_cfg=synth.ARCHS["tiny-s16"], init="stress", return_attention=False, train_stem=True)
    m = TimeT(fe, 20, prototype_init=torch.from_numpy(synth.make_prototypes(20, 32))).cuda()
    o = SwavOptimizer(m, "AdamW", True, 1e-5, 1e-4, "CosineAnnealingLR", cosine_scheduler(0.04, 0.4, 1, 8), 8, 1)
    return m, o


def run(clips):
    m, o = make()
    losses = []
    for x in clips:
        loss = m.get_loss(x)
        m.train_update(o, loss, 0)
        losses.append(loss.item())
    return m, losses


def main():
    torch.cuda.set_device(0)
    clips = [torch.from_numpy(synth.make_clips(2, 3, 224, seed=90 + i)).cuda() for i in range(3)]
    m, plain = run(clips)
    p_plain = {n: p.detach().clone() for n, p in m.named_parameters()}
    g_plain = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    os.environ["TT_EXCHANGE_SINGLE_RANK"] = "1"
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29543")
    dist.init_process_group(backend="nccl", init_method="env://", world_size=1, rank=0, device_id=torch.device("cuda", 0))
    m, ex = run(clips)
    arena = m._grad_arena
    lo, hi = arena.flat.data_ptr(), arena.flat.data_ptr() + 4 * arena.flat.numel()
    named = dict(m.feature_extractor.backbone.named_parameters())
    out = dict(losses_equal=plain == ex,
               params_equal=all(torch.equal(p_plain[n], p.detach()) for n, p in m.named_parameters()),
               grads_equal=all(torch.equal(g_plain[n], p.grad) for n, p in m.named_parameters() if p.grad is not None),
               stem_grads_in_arena=all(lo <= named[n].grad.data_ptr() < hi for n in STEM),
               stem_in_last_bucket=all(any(named[n] is p for p in arena.buckets[-1][2]) for n in STEM))
    torch.cuda.synchronize()
    print("RESULT " + json.dumps(out), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
