"""The evaluation command on video trees (N23): a generated YouTube-VOS-like tree (3 videos of 5 baseline JPEG frames with palette-PNG
annotations and a ``meta.json`` holding a chained case) read through ``make_loader`` / ``YVOSDataset`` and ``evaluation.main``, against the
same loader without the meta file remapped on the host by the transcription of the reference's loop (tests/_ytvos_ref.py)."""
import json
import os
import random

import numpy as np
import pytest
import torch

import _ytvos_ref as R
from timetuning_amd import data_loader as DL, evaluation as EV, hip_ops as ops, synth, video_transformations as VT

pytestmark = pytest.mark.gpu

H, W, FRAMES, RES = 40, 56, 5, 32
# per video: object id -> category.  Sorted categories: ape 1, bear 2, cat 3.
OBJECTS = {"va": {1: "bear", 2: "cat"},      # chained: 1 -> 2, and 2 is present -> 3
           "vb": {1: "ape", 3: "bear"},      # 3 -> 2: 2 is absent from the clip and smaller, no chain
           "vc": {1: "cat", 2: "ape"}}       # 1 -> 3 (absent), 2 -> 1 (already handled)


def _write_tree(root):
    from PIL import Image

    palette = [c for k in range(256) for c in ((37 * k) % 256, (91 * k) % 256, (53 * k) % 256)]
    yy, xx = np.mgrid[0:H, 0:W]
    for v, (video, objects) in enumerate(sorted(OBJECTS.items())):
        os.makedirs(root / "JPEGImages" / video)
        os.makedirs(root / "Annotations" / video)
        ids = sorted(objects)
        for f in range(FRAMES):
            labels = np.zeros((H, W), np.uint8)
            labels[4 + f:22 + f, 3 + 2 * v:25 + 2 * v] = ids[0]
            labels[14:36, 30 - f:52 - f] = ids[1]
            rgb = np.stack([(labels * 60 + xx * 2 + 5 * f) % 256, (yy * 5 + 40 * v) % 256, (xx + yy + 17 * labels) % 256], axis=-1).astype(np.uint8)
            Image.fromarray(rgb).save(root / "JPEGImages" / video / f"{f:05d}.jpg", quality=90)
            im = Image.frombytes("P", (W, H), labels.tobytes())
            im.putpalette(palette)
            im.save(root / "Annotations" / video / f"{f:05d}.png")
    meta = {"videos": {video: {"objects": {str(k): {"category": c, "frames": []} for k, c in objects.items()}} for video, objects in OBJECTS.items()}}
    (root / "meta.json").write_text(json.dumps(meta))
    return str(root), meta


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return _write_tree(tmp_path_factory.mktemp("ytvos") / "val1")


def _loader(root, batch_size=2, **kw):
    return DL.make_loader(root, 4, batch_size, sampling_mode=DL.SamplingMode.UNIFORM, video_transform=VT.evaluation_transforms(RES), shuffle=False,
                          num_workers=3, device=torch.device("cuda", 0), **kw)


def _tables(meta):
    cd = DL.make_categories_dict(meta, "ytvos")
    assert cd == {"ape": 1, "bear": 2, "cat": 3}
    return np.stack([DL.video_category_table(meta, cd, v) for v in sorted(OBJECTS)])


def _remapped_on_host(batches, tables, sequential):
    """The batches of a loader without meta file, every clip remapped by the transcription of the reference's loop."""
    out, k = [], 0
    for data, ann, label in batches:
        a = ann.cpu().numpy()
        for i in range(a.shape[0]):
            a[i] = R.map_instances_ref(a[i], tables[k], sequential)
            k += 1
        out.append((data, torch.from_numpy(a).to(ann.device), label))
    return out


@pytest.fixture(scope="module")
def plain_batches(tree):
    """The tree read WITHOUT the meta file: made once, left unchanged."""
    return list(_loader(tree[0]))


@pytest.mark.parametrize("sequential", [True, False])
def test_loader_with_meta_equals_the_host_remap(tree, plain_batches, sequential):
    root, meta = tree
    loader = _loader(root, meta_file_directory=os.path.join(root, "meta.json"), sequential_category_map=sequential)
    assert isinstance(loader.dataset, DL.YVOSDataset) and loader.fallback_frames == 0
    want = _remapped_on_host(plain_batches, _tables(meta), sequential)
    got = list(loader)
    assert [b[1].shape for b in got] == [(2, 1, 4, RES, RES), (1, 1, 4, RES, RES)]
    for (d, a, l), (wd, wa, wl) in zip(got, want):
        assert torch.equal(d, wd) and torch.equal(l, wl) and a.dtype == torch.uint8
        assert torch.equal(a, wa)
    first = torch.cat([b[1] for b in got])[0]
    assert sorted(first.unique().tolist()) == ([0, 3] if sequential else [0, 2, 3])        # va: 1 -> 2 -> 3 chained, or 1 -> 2 and 2 -> 3
    # __getitem__ maps its one clip the same way
    random_state = random.getstate()                       # (a dataset without an rng of its own draws from the random module)
    item = loader.dataset[2]
    random.setstate(random_state)
    assert item[1].dtype == torch.uint8 and set(item[1].unique().tolist()) <= {0, 1, 3}     # vc: 1 -> 3, 2 -> 1


def test_loader_without_meta_is_unchanged(tree, plain_batches):
    root, _ = tree
    dataset = DL.VideoDataset(os.path.join(root, "JPEGImages"), os.path.join(root, "Annotations"), DL.SamplingMode.UNIFORM, 1, 4, 1, None, None,
                              VT.evaluation_transforms(RES), regular_step=1, device=torch.device("cuda", 0), threads=3)
    assert dataset.category_tables is None
    old = list(DL.ClipLoader(dataset, 2, shuffle=False, seed=0))
    assert not isinstance(_loader(root).dataset, DL.YVOSDataset)                             # the meta.json of the tree is never looked for
    for (d, a, l), (wd, wa, wl) in zip(plain_batches, old):
        assert torch.equal(d, wd) and torch.equal(a, wa) and torch.equal(l, wl)
    ids = [sorted(a[i].unique().tolist()) for _, a, _ in plain_batches for i in range(a.shape[0])]
    assert ids == [[0, 1, 2], [0, 1, 3], [0, 1, 2]]                                          # instance ids, as drawn


def test_unlisted_object_raises_key_error(tree, tmp_path):
    root, meta = tree
    short = {"videos": dict(meta["videos"], vb={"objects": {"1": {"category": "ape", "frames": []}}})}
    path = tmp_path / "short.json"
    path.write_text(json.dumps(short))
    with pytest.raises(KeyError, match="vb.*object id 3"):
        list(_loader(root, meta_file_directory=str(path)))
    with pytest.raises(KeyError, match="vb.*object id 3"):
        _loader(root, meta_file_directory=str(path)).dataset[1]


@pytest.fixture(scope="module")
def model():
    from timetuning_amd.models import FeatureExtractor
    from timetuning_amd.time_tuning import TimeT

    fe = FeatureExtractor("dino-s16", "", [1024, 1024, 512, 256], vit_cfg=synth.ARCHS["tiny-s16"], return_attention=False)
    return TimeT(fe, 200).to(torch.device("cuda", 0))


def _main(root, dataset, protocol, many_to_one, *extra):
    argv = ["--dataset", dataset, "--dataset_path", root, "--model_path", "", "--batch_size", "2", "--num_workers", "3", "--input_resolution", str(RES),
            "--num_clusters", "4", "--evaluation_protocol", protocol] + (["--many_to_one", "True"] if many_to_one else []) + list(extra)
    return EV.main(argv, vit_cfg=synth.ARCHS["tiny-s16"])


def _evaluate(model, batches, protocol, many_to_one):
    ev = EV.Evaluator(model, batches, 10, torch.device("cuda", 0), clustering_algorithm="k-means", uvos_flag=False, involve_bg=True)
    return float(ev.evaluate(many_to_one=many_to_one, evaluation_protocol=protocol, eval_resolution=112 if protocol == "dataset-wise" else RES,
                             num_clusters=4, use_annotations=False, use_mask=False, precision_based=False))


@pytest.mark.parametrize("many_to_one", [False, True])
@pytest.mark.parametrize("protocol", ["frame-wise", "sample-wise", "dataset-wise"])
def test_evaluation_main_scores_the_remapped_batches(tree, plain_batches, model, capsys, protocol, many_to_one):
    root, meta = tree
    score = _main(root, "ytvos_val", protocol, many_to_one)
    assert "Frames decoded on the host (fallback): 0" in capsys.readouterr().out
    assert score == _evaluate(model, _remapped_on_host(plain_batches, _tables(meta), True), protocol, many_to_one)
    assert 0.0 <= score <= 1.0


def test_plain_map_and_davis_on_the_same_tree(tree, plain_batches, model):
    root, meta = tree
    plain = _main(root, "ytvos_val", "sample-wise", False, "--plain_category_map")
    assert plain == _evaluate(model, _remapped_on_host(plain_batches, _tables(meta), False), "sample-wise", False)
    davis = _main(root, "davis_val", "sample-wise", False)                                   # no "ytvos" in the name: instance ids stay
    assert davis == _evaluate(model, plain_batches, "sample-wise", False)


@pytest.mark.parametrize("protocol", ["frame-wise", "sample-wise", "dataset-wise"])
def test_cluster_features_counts_equal_the_unique_loop(monkeypatch, protocol):
    from timetuning_amd import clustering

    bs, fs, g, dim, R = 2, 2, 8, 64, 16
    feats = torch.from_numpy(synth.normal("n23.cf", (bs, fs, g * g, dim)).astype(np.float32)).cuda()
    ann = torch.zeros((bs, fs, R, R), dtype=torch.int64, device="cuda")
    cols = torch.arange(R, device="cuda")
    ann[0] = (cols % 3)[None, None, :]
    ann[1, 0] = (cols % 5)[None, :]
    ann[1, 1] = 255 * (cols % 2)[None, :]
    asked = []
    counts = ops.label_value_counts
    monkeypatch.setattr(ops, "label_value_counts", lambda t: (asked.append(tuple(t.shape)), counts(t))[1])
    maps = clustering.cluster_features(feats, 10, g, R, protocol, annotations=ann)
    segments = {"frame-wise": bs * fs, "sample-wise": bs, "dataset-wise": 1}[protocol]
    assert asked == [(segments, bs * fs * R * R // segments)]                                # ONE call for all segments
    monkeypatch.setattr(ops, "label_value_counts", lambda t: [int(torch.unique(row).shape[0]) for row in t])
    assert torch.equal(maps, clustering.cluster_features(feats, 10, g, R, protocol, annotations=ann))
    wide = ann.clone()
    wide[0, 0, 0, 0] = 1000                                                                   # outside a byte: counted by torch.unique
    monkeypatch.setattr(ops, "label_value_counts", counts)
    got = clustering.cluster_features(feats, 10, g, R, protocol, annotations=wide)
    monkeypatch.setattr(ops, "label_value_counts", lambda t: [int(torch.unique(row).shape[0]) for row in t])
    assert torch.equal(got, clustering.cluster_features(feats, 10, g, R, protocol, annotations=wide))
