"""N21 without a GPU: the NumPy restatement of the decode (tests/_jpeg_ref.py) against Pillow's pixels, the host parser / entropy
decoder (tt_jpeg_probe, tt_jpeg_scan) against the restatement and on unsupported and broken files, ``generate_indices`` against a
transcription of the reference's rule, and the loader's directory pairing and file order."""
import ctypes as C
import io
import os
import random

import numpy as np
import pytest

import _jpeg_ref as R
from timetuning_amd import _lib, hip_ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_frames.npz")
UNSUPPORTED = {"prog_48x64_420_q90": 1, "gray_16x16_q75": 3, "cmyk_16x16_q75": 3}


@pytest.fixture(scope="module")
def fx():
    return R.fixture(GOLDEN)


@pytest.fixture(scope="module")
def supported(fx):
    names = [n for n in fx[0] if n not in UNSUPPORTED]
    assert len(names) == 252 + 3 + 2 + 1 + 10 and all(fx[0][n][1] is not None for n in names)
    return names


@pytest.fixture(scope="module")
def parsed(fx, supported):
    """The restatement's parse of every supported file (computed once, shared)."""
    return {n: R.parse(fx[0][n][0]) for n in supported}


def test_fixture_holds_the_grid(fx):
    for h, w in [(1, 1), (8, 8), (9, 15), (16, 16), (17, 33), (40, 24), (37, 53)]:
        for s in ("444", "422", "420"):
            for q in (30, 75, 95, 100):
                for v in ("std", "opt", "rst"):
                    data, pixels = fx[0][f"grid_{h}x{w}_{s}_q{q}_{v}"]
                    assert pixels.shape == (h, w, 3) and pixels.dtype == np.uint8
                    assert (b"\xff\xdd" in data) == (v == "rst")
    assert os.path.getsize(GOLDEN) < 300 * 1024


def test_restatement_equals_the_fixture_pixels(fx, supported, parsed):
    wrong = [n for n in supported if not np.array_equal(R.reconstruct(parsed[n]), fx[0][n][1])]
    assert not wrong, wrong[:10]


def test_restatement_and_fixture_equal_a_live_pillow_decode(fx, supported, parsed):
    Image = pytest.importorskip("PIL.Image")
    for n in supported:
        live = np.asarray(Image.open(io.BytesIO(fx[0][n][0])).convert("RGB"))
        assert np.array_equal(live, fx[0][n][1]), n
    for n in supported[::7]:
        assert np.array_equal(R.reconstruct(parsed[n]), np.asarray(Image.open(io.BytesIO(fx[0][n][0])).convert("RGB"))), n


def test_scan_equals_the_restatement(fx, supported, parsed):
    """tt_jpeg_probe's geometry and tt_jpeg_scan's coefficients and tables, on every case."""
    for n in supported:
        p = parsed[n]
        info, coeffs, q = hip_ops.jpeg_scan(fx[0][n][0])
        assert (info.status, info.H, info.W, info.sampling) == (0, p.H, p.W, p.sampling), n
        assert info.n_coeffs == sum(r * c * 64 for r, c in p.grids), n
        assert np.array_equal(coeffs, np.concatenate([c.reshape(-1) for c in p.coeffs])), n
        assert q.dtype == np.uint16 and np.array_equal(q, p.qtables), n


def _raw_scan(data: bytes):
    """(probe status, scan status) straight from the C entries, with a guarded buffer: 64 sentinel words on either side must survive."""
    lib = _lib.load()
    H, W, s, n = C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
    rc = lib.tt_jpeg_probe(data, len(data), C.byref(H), C.byref(W), C.byref(s), C.byref(n))
    if rc != 0:
        return rc, None
    buf = np.full(n.value + 128, 0x5A5A, np.int16)
    q = np.full(3 * 64 + 128, 0x5A5A, np.uint16)
    rc2 = lib.tt_jpeg_scan(data, len(data), buf.ctypes.data + 128, n.value, q.ctypes.data + 128)
    assert (buf[:64] == 0x5A5A).all() and (buf[-64:] == 0x5A5A).all() and (q[:64] == 0x5A5A).all() and (q[-64:] == 0x5A5A).all()
    return rc, rc2


def test_unsupported_files_are_classified_not_errors(fx):
    for name, status in UNSUPPORTED.items():
        data = fx[0][name][0]
        info = hip_ops.jpeg_probe(data)
        assert info.status == status and not info.supported, name
        assert _raw_scan(data) == (status, None)
        with pytest.raises(hip_ops.JpegUnsupported):
            hip_ops.jpeg_scan(data)
        with pytest.raises(hip_ops.JpegUnsupported):
            hip_ops.jpeg_scan_batch([fx[0]["clip_v0_f0"][0], data], threads=2, pin=False)
    assert not issubclass(hip_ops.JpegUnsupported, ValueError)


@pytest.mark.parametrize("name", ["grid_37x53_420_q75_std", "grid_37x53_422_q95_rst", "clip_v0_f0"])
def test_a_file_cut_short_is_malformed(fx, name):
    """20 cut positions spread over header and scan: every one a negative status (ValueError from the wrapper), none a crash."""
    data = fx[0][name][0]
    for cut in np.linspace(0, len(data) - 4, 20).astype(int):
        part = data[:cut]
        probe, scan = _raw_scan(part)
        assert probe < 0 or (probe == 0 and scan < 0), (name, cut, probe, scan)
        with pytest.raises(ValueError):
            hip_ops.jpeg_scan(part)
        with pytest.raises(ValueError):
            hip_ops.jpeg_scan_batch([data, part], threads=2, pin=False)


@pytest.mark.parametrize("name", ["grid_37x53_420_q75_std", "grid_40x24_444_q30_opt", "grid_17x33_422_q95_rst"])
def test_one_flipped_bit_in_the_scan_never_crashes(fx, name):
    """A flipped bit gives other coefficients or a negative status - never "unsupported", never a write outside the buffers."""
    data = fx[0][name][0]
    start = data.index(b"\xff\xda") + 14
    rng = np.random.default_rng(3)
    outcomes = set()
    for pos in rng.integers(start, len(data) - 2, 96):
        bad = bytearray(data)
        bad[pos] ^= 1 << int(rng.integers(0, 8))
        probe, scan = _raw_scan(bytes(bad))
        assert probe == 0 and scan <= 0, (name, pos, probe, scan)
        outcomes.add(scan)
        if scan < 0:
            with pytest.raises(ValueError):
                hip_ops.jpeg_scan(bytes(bad))
    assert min(outcomes) < 0          # some flips break the stream


def test_a_missing_restart_marker_is_malformed(fx):
    for name in ("grid_37x53_420_q75_rst", "grid_40x24_444_q100_rst", "grid_17x33_422_q30_rst"):
        data = fx[0][name][0]
        start = data.index(b"\xff\xda")
        for marker in (b"\xff\xd0", b"\xff\xd1"):
            at = data.index(marker, start)
            probe, scan = _raw_scan(data[:at] + data[at + 2:])
            assert probe == 0 and scan < 0, (name, marker, scan)
        renumbered = bytearray(data)
        renumbered[data.index(b"\xff\xd1", start) + 1] = 0xD3
        assert _raw_scan(bytes(renumbered)) == (0, -5)
        with pytest.raises(ValueError, match="restart"):
            hip_ops.jpeg_scan(bytes(renumbered))


def test_segment_lengths_fill_bytes_and_skipped_segments(fx):
    data = fx[0]["grid_17x33_420_q75_std"][0]
    _, want, _ = hip_ops.jpeg_scan(data)
    comment = b"\xff\xfe\x00\x06abcd" + b"\xff\xe5\x00\x04xy"
    padded = data[:2] + b"\xff\xff" + comment[:2] + comment[2:] + data[2:]      # fill bytes before a marker, a COM and an APP5 segment
    assert np.array_equal(hip_ops.jpeg_scan(padded)[1], want)
    overrun = bytearray(data)
    overrun[4:6] = b"\xff\xf0"                                                  # the first segment now claims 65520 bytes
    assert _raw_scan(bytes(overrun))[0] < 0
    for junk in (b"", b"\xff", b"\xff\xd8", b"\x00" * 64, b"\xff\xd8\xff\xd9", data[2:]):
        assert _raw_scan(junk)[0] < 0
        with pytest.raises(ValueError):
            hip_ops.jpeg_probe(junk)


# ---- the loader's host logic
def _reference_indices(mode, size, sampling_num, num_clips, regular_step):
    """Transcription of the reference's rule (VideoDataset.generate_indices) on the global ``random`` module, modes by number."""
    indices = []
    for _ in range(num_clips):
        if mode == 0:
            if size < sampling_num:
                idx = random.choices(range(0, size), k=sampling_num)
            else:
                idx = random.sample(range(0, size), sampling_num)
            idx.sort()
            indices.append(idx)
        elif mode == 1:
            base = random.randint(0, size - sampling_num)
            indices.append(range(base, base + sampling_num))
        elif mode == 2:
            indices.append(range(0, size))
        elif mode == 3:
            step = size // sampling_num if size < sampling_num * regular_step else regular_step
            base = random.randint(0, size - (sampling_num * step))
            indices.append(range(base, base + (sampling_num * step), step))
    return indices


@pytest.mark.parametrize("size,num_frames,step", [(50, 4, 3), (11, 4, 3), (3, 4, 3), (4, 4, 1), (80, 8, 10), (9, 4, 2)])
def test_generate_indices_follows_the_reference(size, num_frames, step):
    """All four modes under one seed, also with size < num_frames (UNIFORM samples with repetition) and size < num_frames * step (Regular
    shrinks its step); the generator ends in the same state, so later draws agree too."""
    from timetuning_amd.data_loader import SamplingMode, generate_indices

    assert [m.value for m in (SamplingMode.UNIFORM, SamplingMode.DENSE, SamplingMode.Full, SamplingMode.Regular)] == [0, 1, 2, 3]
    for mode in SamplingMode:
        if size < num_frames and mode in (SamplingMode.DENSE,):
            continue                      # randint(0, negative) raises in the reference as well
        if mode == SamplingMode.Regular and size < num_frames:
            continue                      # step 0: range() raises in the reference as well
        for clips in (1, 3):
            random.seed(11)
            want = [list(r) for r in _reference_indices(mode.value, size, num_frames, clips, step)]
            tail = random.random()
            random.seed(11)
            got = [list(r) for r in generate_indices(size, num_frames, mode, clips, step)]
            assert got == want and random.random() == tail, (mode, clips)
            own = random.Random(11)
            assert [list(r) for r in generate_indices(size, num_frames, mode, clips, step, rng=own)] == want
    if size < num_frames:
        random.seed(5)
        idx = generate_indices(size, num_frames, SamplingMode.UNIFORM)[0]
        assert len(idx) == num_frames and idx == sorted(idx) and max(idx) < size


@pytest.mark.parametrize("entropy", ["host", "device"])
def test_scan_frames_sorts_files_between_the_device_and_pillow(fx, entropy):
    """The loaders' host half: supported frames into one batch of the route asked for, an unsupported JPEG and a PNG to Pillow, the
    (H, W) of every slot without a decode of the supported ones; a supported file cut short raises."""
    Image = pytest.importorskip("PIL.Image")
    from timetuning_amd.data_loader import decode_frame_on_host, scan_frames

    png = io.BytesIO()
    Image.fromarray(np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)).save(png, "PNG")
    first, last = fx[0]["clip_v0_f0"][0], fx[0]["grid_9x15_420_q75_std"][0]
    files = [first, fx[0]["prog_48x64_420_q90"][0], png.getvalue(), last]
    assert hip_ops.jpeg_probe(files[1]).status > 0
    host = scan_frames(files, 2, entropy, pin=False)
    assert host.device_slots == [0, 3] and set(host.host_items) == {1, 2}
    for k in (1, 2):
        assert np.array_equal(host.host_items[k], decode_frame_on_host(files[k]))
    assert host.host_items[2].tolist() == np.arange(5 * 7 * 3).reshape(5, 7, 3).tolist()
    assert [tuple(d) for d in host.dims] == [fx[0]["clip_v0_f0"][1].shape[:2], (48, 64), (5, 7), (9, 15)]
    assert host.batch.route == entropy and [(i.H, i.W) for i in host.batch.infos] == [host.dims[0], host.dims[3]]
    with pytest.raises(ValueError):
        scan_frames(files[:3] + [last[:len(last) // 2]], 2, entropy, pin=False)


def test_loader_pairs_directories_by_position_and_orders_files(fx, tmp_path):
    pytest.importorskip("PIL.Image")
    from timetuning_amd.data_loader import ClipLoader, SamplingMode, VideoDataset, list_frames, make_loader

    files, anns = fx
    root = tmp_path / "set"
    # video names whose sorted order differs from creation order; annotation directories under OTHER names: paired by position
    for v, (vid, ann) in enumerate([("zebra", "a_first"), ("apple", "b_second")]):
        (root / "JPEGImages" / vid).mkdir(parents=True)
        (root / "Annotations" / ann).mkdir(parents=True)
        src = 1 - v                                                     # "apple" sorts first and holds clip_v0
        for f in (3, 0, 4, 1, 2):                                       # written out of order
            (root / "JPEGImages" / vid / f"{f:05d}.jpg").write_bytes(files[f"clip_v{src}_f{f}"][0])
    for v, ann in enumerate(["a_first", "b_second"]):
        for f in range(5):
            (root / "Annotations" / ann / f"{f:05d}.png").write_bytes(anns[f"clip_v{v}_f{f}"][0])
    (root / "JPEGImages" / "apple" / "notes.txt").write_text("not a frame")
    (root / "JPEGImages" / "stray.jpg").write_bytes(b"not a directory")
    ds = VideoDataset(str(root / "JPEGImages"), str(root / "Annotations"), SamplingMode.Full, 1, 5, device="cpu")
    assert [os.path.basename(k) for k in ds.keys] == ["apple", "zebra"] and len(ds) == 2
    assert [os.path.basename(k) for k in ds.annotation_keys] == ["a_first", "b_second"] and ds.use_annotations
    assert [ds.train_dict_lenghts[k] for k in ds.keys] == [5, 5]         # frame files only
    for v in range(2):
        s = ds.read_host(v)
        assert s.frames == [[files[f"clip_v{v}_f{f}"][0] for f in range(5)]]
        assert np.array_equal(s.annotations[0], np.stack([anns[f"clip_v{v}_f{f}"][1] for f in range(5)]))
        assert s.label.tolist() == [v]
    # sampled frames follow the drawn indices; the loader's own generator leaves the global one alone
    reg = VideoDataset(str(root / "JPEGImages"), "", SamplingMode.Regular, 2, 2, regular_step=2, device="cpu")
    assert not reg.use_annotations
    random.seed(3)
    want = _reference_indices(3, 5, 2, 2, 2)
    random.seed(3)
    s = reg.read_host(1)
    assert s.annotations is None and s.frames == [[files[f"clip_v1_f{f}"][0] for f in clip] for clip in want]
    random.seed(3)
    before = random.getstate()
    reg.read_host(0, rng=random.Random(1))
    assert random.getstate() == before
    # png frames are read when a directory holds no jpg
    (root / "JPEGImages" / "apple" / "x.png").write_bytes(b"")
    assert [os.path.basename(p) for p in list_frames(str(root / "JPEGImages" / "apple"))] == [f"{f:05d}.jpg" for f in range(5)]
    assert [os.path.basename(p) for p in list_frames(str(root / "Annotations" / "a_first"))] == [f"{f:05d}.png" for f in range(5)]
    # the sampler: every rank the same number of videos, a permutation per epoch
    loader = ClipLoader(ds, 1, shuffle=True, world_size=2, rank=1, seed=4)
    assert len(loader) == 1 and len(loader._order()) == 1
    whole = ClipLoader(ds, 2, shuffle=False)
    assert whole._order() == [0, 1] and len(whole) == 1
    assert sorted(ClipLoader(ds, 1, shuffle=True, seed=4)._order()) == [0, 1]
    assert make_loader(str(root), 2, 2, 2, SamplingMode.Regular, device="cpu").dataset.use_annotations
    with pytest.raises(NotImplementedError, match="JPEGImages"):
        make_loader(str(tmp_path / "nowhere"), 2, 2)


# ---- N27: what the JPEG and PNG batches share (the PNG half of the vocabulary and of the layout: tests/test_png_host.py)
def test_status_vocabulary_jpeg():
    for index, where in ((None, ""), (3, "file 3: ")):
        e = hip_ops._JPEG.error(1, index)
        assert type(e) is hip_ops.JpegUnsupported and (e.status, e.index) == (1, index)
        assert str(e) == where + "unsupported JPEG (progressive, lossless or hierarchical frame)"
        e = hip_ops._JPEG.error(-2, index)
        assert type(e) is ValueError and str(e) == where + "malformed JPEG (status -2: the scan data ends early)"
    assert str(hip_ops.JpegUnsupported(99)) == "unsupported JPEG (99)" and str(hip_ops._JPEG.error(-99)) == "malformed JPEG (status -99: unknown)"
    info = hip_ops.JpegInfo(0, 37, 53, 2, 5376)
    assert repr(info) == "JpegInfo(status=0, H=37, W=53, sampling=2, n_coeffs=5376)" and info.supported
    assert not hip_ops.JpegInfo(1, 0, 0, 0, 0).supported
    assert not issubclass(hip_ops.JpegUnsupported, hip_ops.PngUnsupported) and not issubclass(hip_ops.PngUnsupported, hip_ops.JpegUnsupported)
    with pytest.raises(ValueError, match=r"^malformed JPEG \(status -1: broken markers, segment lengths or tables\)$"):
        hip_ops.jpeg_probe(b"\xff\xd8\xff\xd9")


@pytest.mark.parametrize("threads", [1, 3, 16, 100])
def test_the_per_file_runner(threads):
    import threading

    calls, lock = [], threading.Lock()

    def fn(i):
        with lock:
            calls.append((i, threading.get_ident()))
        return 10 * i

    assert hip_ops._each_file(fn, 7, threads) == [0, 10, 20, 30, 40, 50, 60]
    assert sorted(i for i, _ in calls) == list(range(7))                       # every item once
    by_thread = {}
    for i, t in calls:
        by_thread.setdefault(t, []).append(i)
    assert len(by_thread) <= min(threads, 16, 7)                               # a chunk runs on one thread: no more chunks than that
    assert all(items == list(range(items[0], items[0] + len(items))) or len(by_thread) < min(threads, 16, 7)
               for items in by_thread.values())                                # (a thread that took two chunks holds two runs)
    if threads == 1:
        assert set(by_thread) == {threading.get_ident()}                       # serial: no pool
    statuses = [0, 0, -2, 5, 0]
    with pytest.raises(ValueError, match=r"^file 2: malformed JPEG \(status -2"):
        hip_ops._each_file(lambda i: statuses[i], 5, threads, hip_ops._JPEG.error)
    with pytest.raises(hip_ops.PngUnsupported, match="^file 3: unsupported PNG"):
        hip_ops._each_file(lambda i: {"rc": statuses[i]}, 5, threads, hip_ops._PNG.error, lambda r: max(r["rc"], 0))
    assert hip_ops._each_file(fn, 0, threads) == []
    assert hip_ops.FILE_MAX_THREADS == 16 and all(t.name.startswith("tt_files") for t in threading.enumerate() if t.ident in by_thread
                                                  and t is not threading.current_thread())


def test_the_layout_of_a_pinned_buffer(fx):
    import torch

    layout, total = hip_ops._layout([("a", 1), ("b", 16), ("c", 17), ("d", 0)])
    assert layout == {"a": (0, 1), "b": (16, 16), "c": (32, 17), "d": (64, 0)} and total == 64
    for batch in (hip_ops.jpeg_scan_batch([fx[0]["clip_v0_f0"][0]], 1, pin=False), hip_ops.jpeg_prepare_batch([fx[0]["clip_v0_f0"][0]], 1, pin=False)):
        assert all(at % 16 == 0 for at, _ in batch.layout.values())
        for name, (at, size) in batch.layout.items():
            part = batch.part(name)
            assert part.dtype == np.uint8 and part.size == size
            if size:
                assert part.ctypes.data == batch.meta.data_ptr() + at          # a view, not a copy
                part[0] ^= 0xFF
                assert int(batch.meta[at]) == int(part[0])
                part[0] ^= 0xFF
    assert isinstance(batch.meta, torch.Tensor)


def _consecutive(shape, dtype=None):
    import torch

    step = int(np.prod(shape))
    flat = torch.arange(7 * step, dtype=torch.int64).to(torch.uint8 if dtype is None else dtype)
    return flat, [flat[(1 + i) * step:(2 + i) * step].view(*shape) for i in range(5)]


@pytest.mark.parametrize("shape", [(2, 5), (2, 5, 3)])
def test_consecutive_views_are_one_tensor(shape):
    import torch
    from timetuning_amd.data_loader import maps_as_clip

    step = int(np.prod(shape))
    flat, views = _consecutive(shape)
    other, _ = _consecutive(shape)
    for fn in (hip_ops.frames_as_clip, maps_as_clip):
        one = fn(views)
        assert one.shape == (5,) + shape and one.is_contiguous() and torch.equal(one, torch.stack(views))
        assert one.data_ptr() == flat.data_ptr() + step and one.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
        lists = {"gap": views[:2] + views[3:], "order": [views[1], views[0]] + views[2:],
                 "storages": views[:4] + [other[5 * step:6 * step].view(*shape)], "dtype": views[:4] + [views[4].to(torch.int16)]}
        for name, items in lists.items():
            got = fn(items)
            assert got.shape == (len(items),) + shape and got.untyped_storage().data_ptr() != flat.untyped_storage().data_ptr(), name
            assert all(torch.equal(g.to(torch.int64), v.to(torch.int64)) for g, v in zip(got, items)), name
    assert torch.equal(hip_ops.frames_as_clip(lists["gap"]), maps_as_clip(lists["gap"]))


def test_the_route_check_at_all_six_sites(tmp_path):
    from types import SimpleNamespace

    from timetuning_amd import data_loader as DL, leoloader as LL

    ds = SimpleNamespace(jpeg_entropy="host", png="device")
    sites = {"VideoDataset": lambda **k: DL.VideoDataset(str(tmp_path), None, DL.SamplingMode.Full, 1, 4, **k),
             "ClipLoader": lambda **k: DL.ClipLoader(ds, 2, **k), "VOCDataset": lambda **k: LL.VOCDataset(str(tmp_path), **k)}
    for site, make in sites.items():
        for name in ("jpeg_entropy", "png"):
            with pytest.raises(ValueError, match=f"^{name} must be 'host' or 'device', not 'gpu'$"):
                make(**{name: "gpu"})
            if site != "ClipLoader":
                with pytest.raises(ValueError, match=f"^{name} must be 'host' or 'device', not None$"):
                    make(**{name: None})
    loader = DL.ClipLoader(ds, 2, jpeg_entropy=None, png=None)
    assert (loader.jpeg_entropy, loader.png) == ("host", "device")
    loader = DL.ClipLoader(ds, 2, jpeg_entropy="device", png="host")
    assert (loader.jpeg_entropy, loader.png) == ("device", "host") and (ds.jpeg_entropy, ds.png) == ("host", "device")


def _prefetch_threads():
    import threading

    return [t for t in threading.enumerate() if t.name.startswith("tt_prefetch")]


def test_the_prefetch_loop():
    import threading

    from timetuning_amd.data_loader import prefetched

    batches = [[0, 1], [2, 3], [4, 5], [6]]
    for prefetch in (True, False):
        log, seen, logged = [], [], {b[0]: threading.Event() for b in batches}
        host = lambda indices: (log.append(indices), logged[indices[0]].set(), tuple(indices))[2]
        gen = prefetched(batches, host, None, prefetch)
        for k, item in enumerate(gen):
            if prefetch and k + 1 < len(batches):
                assert logged[batches[k + 1][0]].wait(10)       # submitted before batch k was handed out: it runs without our asking for it
                assert log == batches[:k + 2]
            else:
                assert log == batches[:k + 1]
            seen.append(item)
        assert seen == [tuple(b) for b in batches] and log == batches and not _prefetch_threads()
    assert list(prefetched([], host, None, True)) == [] and list(prefetched([], host, None, False)) == []
    gen = prefetched(batches, host, None, True)
    assert next(gen) == (0, 1) and len(_prefetch_threads()) == 1
    gen.close()
    assert not _prefetch_threads()

    def failing(indices):
        if indices == [2, 3]:
            raise KeyError("batch 1")
        return indices

    for prefetch in (True, False):
        gen = prefetched(batches, failing, "cpu", prefetch)
        assert next(gen) == [0, 1]
        with pytest.raises(KeyError, match="batch 1"):
            next(gen)
        assert not _prefetch_threads()


def test_the_drivers_decode_flags():
    import importlib

    for name, jpeg in (("time_tuning", True), ("evaluation", True), ("mask_propagation", True), ("linear_finetune", False),
                       ("cluster_based_foreground_extraction", False)):
        parser = importlib.import_module("timetuning_amd." + name).build_parser()
        flags = ["--jpeg_entropy", "--png_decode"] if jpeg else ["--png_decode"]
        assert ("--jpeg_entropy" in parser._option_string_actions) == jpeg and "--png_decode" in parser._option_string_actions, name
        args = parser.parse_args([])
        assert all(getattr(args, f[2:]) == "host" for f in flags), name
        for f in flags:
            assert getattr(parser.parse_args([f, "device"]), f[2:]) == "device", name
            with pytest.raises(SystemExit):
                parser.parse_args([f, "gpu"])
