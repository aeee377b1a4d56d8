#!/usr/bin/env python3
"""Writes tests/golden/eval_transforms.npz from the reference's own ``video_transformations.py`` classes run on
``(data_clip, annotation_clip)`` pairs of PIL images (N11).

Runs on the CPU of the build container, next to a reference checkout, with Pillow installed:

    python tools/gen_eval_transforms_golden.py

torchvision is not installed; as in ``oracle.gen_golden.gen_transforms`` a stand-in for ``torchvision.transforms.ToTensor`` (its
published PIL path: bytes -> ``[C, H, W]`` float32 ``/ 255``, for modes RGB and L / P) is all the chains below reach.

Inputs (stored whole; tests/_nearest_ops.py makes them): ``{tag}_frames`` uint8 [fs, H, W, 3] and ``{tag}_labels`` uint8
[fs, H, W] - integer label maps with several objects and a 255 rim - for tag ``a`` (60 x 80, annotation images of mode L) and ``b``
(75 x 50, mode P).  Every chain is seeded with ``random.seed(seed); torch.manual_seed(seed)`` right before it runs and ends in
``read_batch``'s ``(255 * annotations).type(torch.uint8)`` + squeeze (data_loader.py:673-675); ``*_data`` is float32 [fs, 3, h, w],
``*_ann`` uint8 [fs, h, w]:
  eval_{tag}                 Resize((R, R), 'bilinear') -> CenterCrop(R) -> ClipToTensor(mean, std)        (evaluation.py:533), R = 32
  prop_{tag}_seed{n}         Resize(R, 'bilinear') -> RandomCrop(R) -> ClipToTensor(mean, std)             (mask_propagation.py:779)
  train_{tag}_seed{n}        Resize(R) -> RandomResizedCrop((R, R)) -> RandomHorizontalFlip() -> ClipToTensor(mean, std) on a pair;
                             ``_flipped`` records whether ``random.random()`` fell below p
  vflip_{tag}_seed{n}        RandomVerticalFlip() -> ClipToTensor(); ``_flipped`` as above
  rresize_{tag}_seed{n}      RandomResize() on the data clip and (re-seeded) on the annotation clip, then ClipToTensor() on the pair
  rrot_{tag}_seed{n}         RandomRotation(40) likewise
  ccrop_{tag}                CenterCrop((21, 34)) -> ClipToTensor()
"""
from __future__ import annotations

import os
import random
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

R = 32
MEAN, STD = [0.485, 0.456, 0.406], [0.228, 0.224, 0.225]
INPUTS = dict(a=(2, 60, 80, 41, "L"), b=(2, 75, 50, 42, "P"))   # fs, H, W, seed, annotation image mode
PROP_SEEDS, TRAIN_SEEDS, VFLIP_SEEDS, RRESIZE_SEEDS, RROT_SEEDS = (0, 1), tuple(range(6)), (0, 1, 2, 3), (0, 1), (0, 1, 2)
CCROP = (21, 34)
ROT_DEGREES = 40


def main():
    import importlib

    import torch
    from PIL import Image

    import _nearest_ops as NO
    from oracle.gen_golden import OUT, import_reference

    import_reference()
    vt = importlib.import_module("video_transformations")

    def to_tensor(pic):
        a = np.array(pic, np.uint8, copy=True)
        return torch.from_numpy(a).view(pic.size[1], pic.size[0], len(pic.getbands())).permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    vt.torchvision = types.SimpleNamespace(transforms=types.SimpleNamespace(ToTensor=lambda: to_tensor))

    draws = []
    real_random = random.random

    def spy_random():
        v = real_random()
        draws.append(v)
        return v

    def seed(n):
        random.seed(n)
        torch.manual_seed(n)
        draws.clear()

    def read_batch_tail(data, ann):
        """data_loader.py:669-675 for one clip: stack, ``(255 * a).type(uint8)``, squeeze the channel."""
        ann = torch.stack([ann])
        ann = (255 * ann).type(torch.uint8)
        if ann.shape[2] == 1:
            ann = ann.squeeze(2)
        return data.numpy().copy(), ann[0].numpy().copy()

    out = {"cfg_R": np.array(R, np.int64), "cfg_ccrop": np.array(CCROP, np.int64), "cfg_rot_degrees": np.array(ROT_DEGREES, np.int64)}
    random.random = spy_random   # the module attribute: what ``random.random()`` in the reference's flips resolves to
    try:
        for tag, (fs, H, W, sd, mode) in INPUTS.items():
            frames, labels = NO.frame_clip(fs, H, W, sd), NO.label_clip(fs, H, W, sd)
            out[f"{tag}_frames"], out[f"{tag}_labels"] = frames, labels

            def clips():
                return [Image.fromarray(f) for f in frames], [Image.fromarray(m, mode) for m in labels]

            def put(key, pair):
                out[key + "_data"], out[key + "_ann"] = read_batch_tail(*pair)

            seed(0)
            chain = vt.Compose([vt.Resize((R, R), "bilinear"), vt.CenterCrop(R), vt.ClipToTensor(mean=MEAN, std=STD)])
            put(f"eval_{tag}", chain(*clips()))
            chain = vt.Compose([vt.Resize(R, "bilinear"), vt.RandomCrop(R), vt.ClipToTensor(mean=MEAN, std=STD)])
            for n in PROP_SEEDS:
                seed(n)
                put(f"prop_{tag}_seed{n}", chain(*clips()))
            chain = vt.Compose([vt.Resize(R), vt.RandomResizedCrop((R, R)), vt.RandomHorizontalFlip(), vt.ClipToTensor(mean=MEAN, std=STD)])
            for n in TRAIN_SEEDS:
                seed(n)
                put(f"train_{tag}_seed{n}", chain(*clips()))
                out[f"train_{tag}_seed{n}_flipped"] = np.array(draws[-1] < 0.5)
            chain = vt.Compose([vt.RandomVerticalFlip(), vt.ClipToTensor()])
            for n in VFLIP_SEEDS:
                seed(n)
                put(f"vflip_{tag}_seed{n}", chain(*clips()))
                out[f"vflip_{tag}_seed{n}_flipped"] = np.array(draws[-1] < 0.5)
            for name, t, seeds in (("rresize", vt.RandomResize(), RRESIZE_SEEDS), ("rrot", vt.RandomRotation(ROT_DEGREES), RROT_SEEDS)):
                for n in seeds:
                    d, a = clips()
                    seed(n)
                    d = t(d)
                    seed(n)
                    a = t(a)
                    put(f"{name}_{tag}_seed{n}", vt.ClipToTensor()(d, a))
            seed(0)
            put(f"ccrop_{tag}", vt.Compose([vt.CenterCrop(CCROP), vt.ClipToTensor()])(*clips()))
    finally:
        random.random = real_random

    for kind in ("train", "vflip"):
        flips = [bool(v) for k, v in out.items() if k.startswith(kind) and k.endswith("_flipped")]
        assert any(flips) and not all(flips), (kind, flips)
    path = os.path.join(OUT, "eval_transforms.npz")
    np.savez_compressed(path, **out)
    print(f"{path} written: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
