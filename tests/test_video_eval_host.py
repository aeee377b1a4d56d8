"""Host-side checks of the video-dataset evaluation (N23): the category dict and the instance -> category table against outputs recorded
from the reference's own ``make_categories_dict`` / ``map_instances`` (tests/golden/ytvos_meta.npz) and against a transcription of its
in-place loop (tests/_ytvos_ref.py), the entries' refusals through the C ABI (they return before any launch, so no GPU is needed), the
reader's errors and the command line."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import _ytvos_ref as R
from timetuning_amd import _lib, data_loader as DL, evaluation as EV, hip_ops as ops

TT_EINVAL = -1
FAKE = 4096    # a non-null "device pointer": every call below is refused before anything could read it


@pytest.fixture(scope="module")
def gold(golden):
    g = golden("ytvos_meta")
    return g, json.loads(str(g["meta_json"]))


def test_categories_dict_equals_the_reference(gold):
    g, meta = gold
    cd = DL.make_categories_dict(meta, "ytvos")
    assert list(cd.keys()) == [str(k) for k in g["category_names"]] and list(cd.values()) == [int(v) for v in g["category_ids"]]
    assert cd == R.make_categories_loop(meta)
    assert min(cd.values()) == 1                                # 0 stays the background
    with pytest.raises(ValueError, match="ytvos"):
        DL.make_categories_dict(meta, "davis")                 # (the reference: UnboundLocalError)


def test_composed_table_equals_the_reference_on_the_golden_clips(gold):
    g, meta = gold
    cd = DL.make_categories_dict(meta, "ytvos")
    chained = 0
    for i, video in enumerate(g["videos"]):
        clip, want = torch.from_numpy(g[f"clip_{i}"]), torch.from_numpy(g[f"mapped_{i}"])
        cat = DL.video_category_table(meta, cd, str(video))
        lut = torch.from_numpy(DL.compose_instance_lut(np.unique(clip.numpy()), cat, sequential=True))
        assert torch.equal(lut[clip.long()], want), video
        plain = torch.from_numpy(DL.compose_instance_lut(np.unique(clip.numpy()), cat, sequential=False))[clip.long()]
        assert torch.equal(plain, torch.from_numpy(R.map_instances_plain(clip.numpy(), cat))), video
        chained += int(not torch.equal(plain, want))
    names = [str(v) for v in g["videos"]]
    assert chained >= 2 and {"chain", "cycle", "absent", "bg", "max"} <= set(names)
    assert int(g[f"clip_{names.index('bg')}"].max()) == 0 and int(g[f"clip_{names.index('max')}"].max()) == 255
    k = names.index("chain")                                    # object 1 -> category 2 with object 2 present: mapped again, onto 4
    assert set(np.unique(g[f"clip_{k}"])) == {0, 1, 2} and set(np.unique(g[f"mapped_{k}"])) == {0, 4}


def test_composed_table_equals_the_in_place_loop_on_drawn_cases():
    rng = np.random.default_rng(2023)
    same = differ = 0
    for _ in range(3000):
        clip, cat = R.drawn_case(rng)
        present = np.unique(clip)
        seq = DL.compose_instance_lut(present, cat, True)
        plain = DL.compose_instance_lut(present, cat, False)
        assert seq.dtype == np.uint8 and seq.shape == (256,)
        assert np.array_equal(seq[clip], R.map_instances_loop(clip, cat))
        assert np.array_equal(plain[clip], R.map_instances_plain(clip, cat))
        absent = np.setdiff1d(np.arange(256), present)
        assert np.array_equal(seq[absent], absent) and np.array_equal(plain[absent], absent) and seq[0] == 0 and plain[0] == 0
        flags = np.zeros(256, bool)
        flags[present] = True
        assert np.array_equal(DL.compose_instance_lut(flags, cat, True), seq)      # both forms of `present`
        if np.array_equal(seq[clip], plain[clip]):
            same += 1
        else:
            differ += 1
    assert same > 100 and differ > 100, (same, differ)          # the chaining is real, and so is its absence


def test_missing_category_raises_the_smallest_id():
    cat = np.full(256, -1, np.int32)
    cat[[2, 9]] = 3
    for sequential in (True, False):
        with pytest.raises(KeyError) as e:
            DL.compose_instance_lut([0, 2, 7, 5, 9], cat, sequential)
        assert e.value.args[0] == 5
        assert DL.compose_instance_lut([0, 2, 9], cat, sequential)[[0, 2, 9, 5]].tolist() == [0, 3, 3, 5]
    with pytest.raises(KeyError):
        R.map_instances_loop(np.array([0, 5], np.uint8), cat)


def test_exports_and_abi():
    lib = _lib.load()
    for name in ("tt_label_presence_segments", "tt_map_instances", "tt_map_instances_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.tt_abi_version() == 8
    assert lib.tt_map_instances_workspace_bytes(5) == 5 * 32 and lib.tt_map_instances_workspace_bytes(0) == 0
    for name in ("label_presence", "label_value_counts", "map_instances"):
        assert callable(getattr(ops, name))
    for name in ("make_categories_dict", "compose_instance_lut", "YVOSDataset", "VideoDataset", "make_loader"):
        assert hasattr(DL, name)
    assert issubclass(DL.YVOSDataset, DL.VideoDataset)
    with pytest.raises(_lib.HipLibraryError):                   # no CPU fallback
        ops.label_value_counts(torch.zeros((2, 8), dtype=torch.uint8))
    with pytest.raises(_lib.HipLibraryError):
        ops.map_instances(torch.zeros((2, 8), dtype=torch.uint8), torch.zeros((2, 256), dtype=torch.int32))


def _refused(rc, *needles):
    assert rc == TT_EINVAL
    msg = _lib.load().tt_last_error().decode()
    for n in needles:
        assert str(n) in msg, msg


def test_entries_refuse_before_launching():
    lib = _lib.load()
    pres = lambda labels=FAKE, eb=1, S=3, P=17, words=FAKE, status=FAKE: lib.tt_label_presence_segments(labels, eb, S, P, words, status, None)  # noqa: E731
    _refused(pres(labels=None), "null")
    _refused(pres(words=None), "null")
    _refused(pres(status=None), "null")
    _refused(pres(eb=2), "elem_bytes = 2")
    _refused(pres(S=0), "S = 0")
    _refused(pres(P=0), "P = 0")
    _refused(pres(labels=FAKE + 4, eb=8), "8-byte")

    def remap(src=FAKE, dst=FAKE + 4096, cat=FAKE, S=3, P=17, sequential=1, lut=FAKE, status=FAKE, ws=FAKE, ws_bytes=96):
        return lib.tt_map_instances(src, dst, cat, S, P, sequential, lut, status, ws, ws_bytes, None)

    for arg in ("src", "dst", "cat", "lut", "status", "ws"):
        _refused(remap(**{arg: None}), "null")
    _refused(remap(S=0), "S = 0")
    _refused(remap(P=-1), "P = -1")
    _refused(remap(sequential=2), "sequential = 2")
    _refused(remap(dst=FAKE), "overlap", 51)                    # in place
    _refused(remap(dst=FAKE + 50), "overlap", 51)               # the last byte of the input
    _refused(remap(dst=FAKE - 50), "overlap", 51)
    _refused(remap(ws_bytes=95), "95", "96")                   # a short workspace
    _refused(remap(cat=FAKE + 2), "4 bytes")
    assert remap(dst=FAKE + 51, S=0) == TT_EINVAL               # (adjacent ranges do not overlap: refused for S alone)
    assert "overlap" not in lib.tt_last_error().decode()


def _touch_tree(root, videos, frames=3):
    for v in videos:
        for sub, ext in (("JPEGImages", "jpg"), ("Annotations", "png")):
            os.makedirs(root / sub / v, exist_ok=True)
            for k in range(frames):
                (root / sub / v / f"{k:05d}.{ext}").write_bytes(b"")
    return root


def test_reader_builds_tables_and_raises(tmp_path, gold):
    g, meta = gold
    root = _touch_tree(tmp_path / "yv", ["chain", "max", "unlisted"])
    meta_path = root / "meta.json"
    meta_path.write_text(json.dumps(meta))
    args = (str(root / "JPEGImages"), str(root / "Annotations"), DL.SamplingMode.UNIFORM)
    ds = DL.YVOSDataset(*args, 1, 2, 1, meta_file_directory=str(meta_path), device="cpu")
    assert ds.category_dict == DL.make_categories_dict(meta, "ytvos") and ds.sequential_category_map is True
    assert ds.category_tables.shape == (3, 256) and ds.category_tables.dtype == np.int32
    chain, mx, unlisted = ds.category_tables                    # the sorted directories
    assert chain[1] == 2 and chain[2] == 4 and (np.delete(chain, [1, 2]) == -1).all()
    assert mx[4] == 5 and mx[255] == 6 and (unlisted == -1).all()
    plain = DL.VideoDataset(*args, 1, 2, meta_file_directory=str(meta_path), device="cpu", sequential_category_map=False)
    assert plain.sequential_category_map is False and plain.category_tables is not None     # VideoDataset takes a meta file too
    with pytest.raises(NotImplementedError, match="num_clips"):
        DL.VideoDataset(*args, 2, 2, meta_file_directory=str(meta_path), device="cpu")
    with pytest.raises(FileNotFoundError):
        DL.YVOSDataset(*args, 1, 2, 1, device="cpu")
    absent = DL.VideoDataset(*args, 1, 2, meta_file_directory=str(root / "none.json"), device="cpu")   # the reference: "There is no meta file."
    assert absent.meta_dict is None and absent.category_tables is None
    same = torch.arange(6, dtype=torch.uint8).view(1, 6)
    assert absent.map_categories(same, [0]) is same
    bad = dict(meta, videos=dict(meta["videos"], chain={"objects": {"300": {"category": "dog"}}}))
    (root / "bad.json").write_text(json.dumps(bad))
    with pytest.raises(ValueError, match="300"):
        DL.VideoDataset(*args, 1, 2, meta_file_directory=str(root / "bad.json"), device="cpu")


def test_parser_defaults_and_the_old_refusal(tmp_path):
    a = EV.build_parser().parse_args([])
    assert (a.dataset, a.dataset_path, a.batch_size, a.num_workers, a.num_frames, a.input_resolution) == ("davis_val", "../data", 16, 3, 4, 224)
    assert (a.evaluation_protocol, a.num_clusters, a.many_to_one, a.log_videos) == ("frame-wise", 10, False, False)
    assert a.plain_category_map is False
    assert EV.build_parser().parse_args(["--plain_category_map"]).plain_category_map is True
    for argv in (["--dataset", "davis_val"], ["--dataset", "ytvos_val", "--dataset_path", str(tmp_path)]):   # no JPEGImages there
        with pytest.raises(NotImplementedError, match="--dataset voc") as e:
            EV.main(argv)
        assert "dataset readers" in str(e.value)
    import inspect

    sig = inspect.signature(DL.make_loader).parameters
    assert sig["meta_file_directory"].default is None and sig["sequential_category_map"].default is True
