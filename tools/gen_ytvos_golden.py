#!/usr/bin/env python3
"""Writes tests/golden/ytvos_meta.npz from the reference's own ``make_categories_dict`` and ``map_instances``
(``data_loader.py:453-464, 497-506``) run on a small generated meta dict and uint8 clips (N23).

Runs on the CPU of the build container, next to a reference checkout:

    python tools/gen_ytvos_golden.py

The reference is imported with the stub recipe of ``oracle.gen_golden.import_reference``.  Stored (data only):
  meta_json              the meta dict, as JSON text
  category_names / category_ids     ``make_categories_dict(meta, "ytvos")``, in the dict's order
  videos                 the video name of each clip
  clip_{i}               uint8 [1, fs, h, w], the input of ``map_instances``
  mapped_{i}             what ``map_instances(clip, meta["videos"][video]["objects"], category_dict)`` left, uint8 [1, fs, h, w]
The clips: ``chain`` (object 1 -> category 2 with object 2 present: mapped again), ``cycle`` (1 -> 2 -> 3 -> 1: everything ends as 1),
``absent`` (a category equal to an object id that is not in the clip, and 5 -> 1 after 1 was handled: no chaining backwards),
``bg`` (background only), ``max`` (ids 4 and 255) and ``mixed`` (random ids 0 .. 6).
"""
from __future__ import annotations

import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

FS, H, W = 2, 5, 7


def _obj(category):
    return {"category": category, "frames": ["00000"]}


META = {"videos": {
    "chain": {"objects": {"1": _obj("bear"), "2": _obj("dog")}},                                  # 1 -> 2, and 2 -> 4
    "cycle": {"objects": {"1": _obj("bear"), "2": _obj("cat"), "3": _obj("ape")}},                # 1 -> 2 -> 3 -> 1
    "absent": {"objects": {"1": _obj("cat"), "3": _obj("zebra"), "5": _obj("ape")}},              # 1 -> 3 (3 not in the clip), 5 -> 1
    "bg": {"objects": {"1": _obj("eel")}},
    "max": {"objects": {"4": _obj("eel"), "255": _obj("fox")}},
    "mixed": {"objects": {str(k): _obj(c) for k, c in zip(range(1, 7), ("dog", "ape", "fox", "bear", "cat", "eel"))}},
}}


def clips():
    rng = np.random.default_rng(23)

    def draw(values):
        v = np.asarray(values, np.uint8)
        c = v[rng.integers(0, len(v), size=(1, FS, H, W))]
        c.reshape(-1)[: len(v)] = v   # every value occurs
        return c

    return [("chain", draw([0, 1, 2])), ("cycle", draw([0, 1, 2, 3])), ("absent", draw([0, 1, 5])), ("bg", np.zeros((1, FS, H, W), np.uint8)),
            ("max", draw([0, 4, 255])), ("mixed", draw([0, 1, 2, 3, 4, 5, 6]))]


def main():
    import importlib

    import torch

    from oracle.gen_golden import OUT, import_reference

    import_reference()
    ref = importlib.import_module("data_loader")
    category_dict = ref.make_categories_dict(META, "ytvos")
    out = {"meta_json": np.array(json.dumps(META)), "category_names": np.array(list(category_dict.keys())),
           "category_ids": np.array(list(category_dict.values()), np.int64)}
    videos = []
    for i, (video, clip) in enumerate(clips()):
        videos.append(video)
        out[f"clip_{i}"] = clip
        mapped = ref.map_instances(torch.from_numpy(clip.copy()), META["videos"][video]["objects"], category_dict)
        out[f"mapped_{i}"] = mapped.numpy().astype(np.uint8)
    out["videos"] = np.array(videos)
    path = os.path.join(OUT, "ytvos_meta.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", category_dict)


if __name__ == "__main__":
    main()
