"""CPU-only checks of the stem gradients' host surface (scope row N19): the four new entry points are exported, declared and bound; the
``train_stem`` keyword of ``FeatureExtractor`` opens the reference's full substring match (models.py:929-935) and nothing else; the training
CLI's ``--unfreeze_layers`` defaults to the reference's hard-coded list (time_tuning.py:574)."""
import os
import re

import pytest

from timetuning_amd import _lib, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("tt_patch_embed_bwd", "tt_patch_embed_bwd_workspace_bytes", "tt_patch_embed_bwd_shape_ok", "tt_pos_embed_interpolate_bwd")
STEM = ("patch_embed.proj.weight", "patch_embed.proj.bias", "cls_token", "pos_embed")


def test_the_four_entries_are_exported_declared_and_bound():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "timetuning_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in include/timetuning_hip.h"
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), f"{name} is not exported"
    assert lib.tt_abi_version() == 8   # additive: the ABI version stays
    # every entry cites its reference site
    for name in ("tt_patch_embed_bwd", "tt_pos_embed_interpolate_bwd"):
        comment = header[: header.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "dino_vision_transformer.py:" in comment, name


def test_shape_rule_and_workspace_size_are_host_functions():
    lib = _lib.load()
    # (F, C, H, W, P, D): what tt_patch_embed_fwd takes at P % 4 == 0, W % 4 == 0, D % 4 == 0 - tile remainders of D and C P P included
    for ok in ((32, 3, 224, 224, 16, 384), (1, 3, 16, 16, 16, 64), (2, 3, 40, 24, 8, 192), (3, 1, 32, 32, 16, 64), (2, 3, 32, 32, 4, 100)):
        assert lib.tt_patch_embed_bwd_shape_ok(*ok) == 1, ok
        n, K = (ok[2] // ok[4]) * (ok[3] // ok[4]), ok[1] * ok[4] * ok[4]
        nb = lib.tt_patch_embed_bwd_workspace_bytes(*ok)
        assert nb >= (n + 1) * ok[5] * 4, ok                      # at least the position-table scratch
        assert nb <= ((n + 1) * ok[5] + 3 + 64 * ok[5] * K) * 4   # ... and at most 64 slices of partial tiles behind it
    for bad in ((2, 3, 24, 24, 6, 64), (2, 3, 32, 30, 2, 64), (2, 3, 32, 32, 16, 66), (2, 3, 40, 32, 16, 64), (0, 3, 32, 32, 16, 64)):
        assert lib.tt_patch_embed_bwd_shape_ok(*bad) == 0, bad
        assert lib.tt_patch_embed_bwd_workspace_bytes(*bad) == 0


def test_train_stem_opens_the_reference_substring_match():
    from timetuning_amd.models import FeatureExtractor

    cfg = synth.ARCHS["tiny-s16"]
    layers = ["patch_embed", "pos_embed", "cls_token", "blocks.11"]
    fe = FeatureExtractor("dino-s16", "", [128, 128, 64, 32], unfreeze_layers=layers, vit_cfg=cfg, train_stem=True)
    want = {n for n, _ in fe.backbone.named_parameters() if n in STEM or n.startswith("blocks.11.")}
    assert {n for n, p in fe.backbone.named_parameters() if p.requires_grad} == want and set(STEM) <= want
    assert fe.trainable_block_ids() == [11]                                     # unchanged in meaning: blocks that HOLD a trainable tensor
    assert fe.stem_trainable() and fe.backward_block_ids() == list(range(cfg["depth"]))   # the backward path: every block
    for p in fe.backbone.parameters():
        assert p._tt_static == (not p.requires_grad)
    with pytest.raises(NotImplementedError, match="train_stem"):               # without the keyword: refused as before, the message names it
        FeatureExtractor("dino-s16", "", [128, 128, 64, 32], unfreeze_layers=layers, vit_cfg=cfg)
    # the keyword alone changes nothing: the default list trains what it trained, the backward stops at the first trainable block
    fe2 = FeatureExtractor("dino-s16", "", [128, 128, 64, 32], unfreeze_layers=["blocks.11", "blocks.9.mlp"], vit_cfg=cfg, train_stem=True)
    assert not fe2.stem_trainable() and fe2.trainable_block_ids() == [9, 11] and fe2.backward_block_ids() == [9, 10, 11]
    # a single stem tensor is enough to put every block on the path
    fe3 = FeatureExtractor("dino-s16", "", [], unfreeze_layers=["pos_embed"], vit_cfg=cfg, train_stem=True)
    assert [n for n, p in fe3.backbone.named_parameters() if p.requires_grad] == ["pos_embed"]
    assert fe3.trainable_block_ids() == [] and fe3.backward_block_ids() == list(range(cfg["depth"]))


def test_input_gradients_stay_refused():
    import torch

    from timetuning_amd.models import FeatureExtractor

    fe = FeatureExtractor("dino-s16", "", [], unfreeze_layers=["patch_embed"], vit_cfg=synth.ARCHS["tiny-s16"], train_stem=True)
    with pytest.raises(NotImplementedError, match="input frames"):
        fe(torch.zeros(1, 3, 224, 224, requires_grad=True))


def test_cli_default_is_the_two_blocks():
    from timetuning_amd.time_tuning import build_parser

    assert build_parser().parse_args([]).unfreeze_layers == ["blocks.11", "blocks.10"]
    a = build_parser().parse_args(["--unfreeze_layers", "blocks", "patch_embed", "pos_embed", "cls_token"])
    assert a.unfreeze_layers == ["blocks", "patch_embed", "pos_embed", "cls_token"]
