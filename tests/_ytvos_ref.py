"""The reference's YouTube-VOS category mapping (``data_loader.py:453-464, 497-506``) transcribed for the tests, and the generated cases
they share.  NumPy only; nothing here touches the library under test."""
from __future__ import annotations

import numpy as np


def map_instances_loop(clip: np.ndarray, cat) -> np.ndarray:
    """``map_instances`` for one clip: the objects are the ascending unique values of the clip BEFORE the loop, and every
    ``frame[frame == obj] = category`` acts in place on what the earlier ones left.  ``cat``: int [256], -1 = not in the meta file
    (``KeyError(obj)``, as the reference's dict lookup)."""
    frame = clip.copy()
    objects = np.unique(frame)
    for obj in objects:
        if int(obj) == 0:
            continue
        if not 0 <= int(cat[int(obj)]) <= 255:
            raise KeyError(int(obj))
        frame[frame == obj] = cat[int(obj)]
    return frame


def map_instances_plain(clip: np.ndarray, cat) -> np.ndarray:
    """What a user who wants correct classes asks for: every present object id straight to its category, read from the ORIGINAL clip."""
    out = clip.copy()
    for obj in np.unique(clip):
        if int(obj) == 0:
            continue
        if not 0 <= int(cat[int(obj)]) <= 255:
            raise KeyError(int(obj))
        out[clip == obj] = cat[int(obj)]
    return out


def map_instances_ref(clip: np.ndarray, cat, sequential: bool = True) -> np.ndarray:
    return map_instances_loop(clip, cat) if sequential else map_instances_plain(clip, cat)


def make_categories_loop(meta_dict) -> dict:
    """``make_categories_dict(meta_dict, "ytvos")``: first-seen list, sorted, numbered from 1."""
    category_list = []
    for name in meta_dict["videos"].keys():
        for obj in meta_dict["videos"][name]["objects"].keys():
            c = meta_dict["videos"][name]["objects"][obj]["category"]
            if c not in category_list:
                category_list.append(c)
    return {k: v + 1 for v, k in enumerate(sorted(category_list))}


def drawn_case(rng: np.random.Generator, top: int = 11, pixels: int = 48):
    """One random clip (uint8 [pixels]) with ids drawn from 0 .. top, and a table with categories 1 .. top for ids 1 .. top."""
    n_ids = int(rng.integers(1, 6))
    ids = rng.integers(0, top + 1, size=n_ids)
    clip = ids[rng.integers(0, n_ids, size=pixels)].astype(np.uint8)
    cat = np.full(256, -1, np.int32)
    cat[1:top + 1] = rng.integers(1, top + 1, size=top)
    return clip, cat


def segment_tables(S: int, seed: int) -> np.ndarray:
    """int32 [S, 256] tables that differ between segments: ids 1 .. 40 and 255 have categories (some chain onto other ids)."""
    rng = np.random.default_rng(seed)
    cat = np.full((S, 256), -1, np.int32)
    for s in range(S):
        cat[s, 1:41] = rng.integers(1, 60, size=40)
        cat[s, 255] = 7 + s
    return cat


def segment_labels(S: int, P: int, seed: int) -> np.ndarray:
    """uint8 [S, P] label maps in runs, values among 0, 1 .. 40 and 255."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([np.arange(0, 41), [255]]).astype(np.uint8)
    out = np.empty((S, P), np.uint8)
    for s in range(S):
        picks = pool[rng.integers(0, len(pool), size=max(1, P // 3 + 1))]
        out[s] = np.repeat(picks, rng.integers(3, 7, size=len(picks)))[:P]   # (at least 3 (P // 3 + 1) > P labels)
    return out
