"""N26 without a GPU: tt_png_probe, tt_png_prepare and the emulation tt_png_decode_host (the sequential loop over the kernel's steps in
csrc/png_inflate.hpp) over every file of tests/golden/png_streams.npz - pixels against Pillow's with ``==``, inflated bytes against
``zlib.decompress``, the documented reason of every unsupported file and status of every broken one, capacities, seeded bit flips against
zlib, the coverage the fixture must reach, and the loaders' host logic."""
import ctypes as C
import random

import numpy as np
import pytest

import _png_ref as P
from timetuning_amd import _lib, hip_ops

FLIPS = 100            # per small file
SMALL = 600            # bytes of stream below which a file takes part in the bit flips


@pytest.fixture(scope="module")
def fx():
    return P.fixture()


@pytest.fixture(scope="module")
def decoded(fx):
    """Every supported file through prepare and the emulation, once: (names, batch, maps, status, statistics, unfiltered slices)."""
    names = list(fx[0])
    batch = hip_ops.png_prepare_batch([fx[0][n] for n in names], threads=4, pin=False)
    return (names, batch) + hip_ops.png_decode_host(batch)


def test_the_64_lane_emulation_equals_the_sequential_one(fx, decoded):
    """tt_png_decode_host_wave runs the shared inflate as the kernel does - 64 lanes, here threads behind a barrier -, which is where the
    pending literals, the lane-strided copies, the table fill by all lanes and the Adler partial sums run at all on the CPU: every
    supported and every broken file gives the maps, status and statistics of the one-lane loop."""
    names, batch, maps, status, stats, slices = decoded
    wave = hip_ops.png_decode_host(batch, lanes=64)
    assert np.array_equal(wave[1], status) and np.array_equal(wave[2], stats)
    assert all(np.array_equal(a, b) for a, b in zip(wave[0], maps)) and all(np.array_equal(a, b) for a, b in zip(wave[3], slices))
    bad = [d for n, (s, d) in fx[1].items() if n != "wrong_idat_crc"]
    broken = hip_ops.png_prepare_batch(bad, threads=1, pin=False)
    one, many = hip_ops.png_decode_host(broken), hip_ops.png_decode_host(broken, lanes=64)
    assert np.array_equal(one[1], many[1]) and np.array_equal(one[2], many[2]) and (one[1] != 0).all()
    with pytest.raises(ValueError, match="lanes"):
        hip_ops.png_decode_host(batch, lanes=32)


def test_every_supported_file_equals_pillow_and_zlib(fx, decoded):
    """The inflated bytes are compared behind the unfilter - the emulation unfilters its slice in place, the test unfilters zlib's bytes
    with its own NumPy code; the filter bytes stay where they are, so equal slices are equal inflated bytes."""
    names, batch, maps, status, stats, slices = decoded
    assert len(names) == 48 and status.tolist() == [0] * len(names)
    for i, n in enumerate(names):
        info = hip_ops.png_probe(fx[0][n])
        want = P.pillow(fx[0][n])
        assert info.supported and (info.H, info.W) == want.shape == maps[i].shape, n
        assert (maps[i] == want).all(), n
        raw = P.zlib_accepts(batch.part("streams")[int(batch.table[i]["stream_off"]):][:int(batch.table[i]["stream_len"])].tobytes())
        assert raw is not None and len(raw) == stats[i, 7] == slices[i].size, n
        rows, pix = P.unfilter(raw, info.H, info.W, info.depth)
        assert (rows.reshape(-1) == slices[i]).all() and (pix == want).all(), n


def test_unsupported_files_give_their_reason(fx):
    assert {n: r for n, (r, _) in fx[2].items()} == {"interlaced": 1, "rgb": 2, "gray_depth4": 3, "gray_16bit": 4}
    for name, (reason, data) in fx[2].items():
        info = hip_ops.png_probe(data)
        assert info.status == reason and not info.supported and (info.H, info.W) == (16, 16), name
        with pytest.raises(hip_ops.PngUnsupported, match="file 1: unsupported PNG") as e:
            hip_ops.png_prepare_batch([fx[0]["z0_3x7_d4"], data], threads=1, pin=False)
        assert e.value.status == reason and hip_ops.PNG_UNSUPPORTED[reason] in str(e.value)


def test_broken_files_give_their_status_and_pillow_raises(fx):
    assert sorted(fx[1]) == sorted(["wrong_adler", "wrong_idat_crc", "filter_byte_5", "truncated_idat", "distance_before_start",
                                    "oversubscribed_table", "missing_end_of_block", "one_row_too_long", "one_row_too_short", "nlen_mismatch",
                                    "stored_after_literals_too_long"])
    want = {"wrong_adler": -6, "wrong_idat_crc": -6, "filter_byte_5": -7, "truncated_idat": -2, "distance_before_start": -4,
            "oversubscribed_table": -3, "missing_end_of_block": -3, "one_row_too_long": -5, "one_row_too_short": -2, "nlen_mismatch": -1,
            "stored_after_literals_too_long": -5}
    good = fx[0]["z0_3x7_d4"]
    for name, (status, data) in fx[1].items():
        assert status == want[name], name
        assert P.pillow_raises(data) == (name not in P.PILLOW_ACCEPTS), name       # both sides: _png_ref.PILLOW_ACCEPTS says which and why
        assert hip_ops.png_probe(data).supported, name                             # the chunk layout is sound: the probe takes it
        if name == "wrong_idat_crc":                                               # the host half's to find
            with pytest.raises(ValueError, match=r"file 1: malformed PNG \(status -6"):
                hip_ops.png_prepare_batch([good, data], threads=1, pin=False)
            continue
        batch = hip_ops.png_prepare_batch([good, data, good], threads=1, pin=False)
        for lanes in (1, 64):
            maps, st, _, _ = hip_ops.png_decode_host(batch, lanes)
            assert st.tolist() == [0, status, 0], (name, lanes, st)
            assert (maps[0] == P.pillow(good)).all() and (maps[2] == P.pillow(good)).all(), name
    # files that are not PNG files at all, or end inside a chunk
    for data, status in [(b"", -1), (good[:7], -1), (b"\x89PNG\r\n\x1a\n", -2), (good[:40], -2), (good[:-5], -2), (b"x" + good[1:], -1),
                         (good[:12] + b"IDAT" + good[16:], -1), (good[:16] + bytes(4) + good[20:], -1), (good[:24] + b"\x03\x00" + good[26:], -1)]:
        with pytest.raises(ValueError, match=f"status {status}"):
            hip_ops.png_probe(data)


def test_capacities_one_byte_short_are_refused(fx):
    lib = _lib.load()
    data = fx[0]["z2_65x33_d8_flush7"]
    need = C.c_size_t()
    assert lib.tt_png_prepare_bytes(len(data), C.byref(need)) == 0
    stream, row = np.zeros(need.value, np.uint8), np.zeros(16, np.int64)
    assert lib.tt_png_prepare(data, len(data), stream.ctypes.data, stream.size, row.ctypes.data) == 0
    idat = len(P.idat(data))
    assert row[6] == idat - 2 and idat <= need.value
    assert lib.tt_png_prepare(data, len(data), stream.ctypes.data, idat - 1, row.ctypes.data) == -8      # the payloads do not fit
    assert lib.tt_png_prepare(data, len(data), stream.ctypes.data, idat, row.ctypes.data) == 0
    batch = hip_ops.png_prepare_batch([data, fx[0]["z0_1x1_d1_flush7"]], threads=1, pin=False)
    table, streams = batch.table, batch.part("streams")
    out, ws, status = np.full(batch.out_bytes, 0x5A, np.uint8), np.zeros(batch.ws_bytes // 4 + 1, np.int32), np.full(2, 77, np.int32)

    def call(out_bytes=batch.out_bytes, ws_bytes=batch.ws_bytes, stream_bytes=streams.size, t=table):
        t = np.ascontiguousarray(t)
        return lib.tt_png_decode_host(streams.ctypes.data, stream_bytes, t.ctypes.data, t.ctypes.data, 2, out.ctypes.data, out_bytes,
                                      ws.ctypes.data, ws_bytes, status.ctypes.data, None)

    last = int(table[1]["stream_off"] + (table[1]["stream_len"] + 3) // 4 * 4)
    for kw in (dict(out_bytes=batch.out_bytes - 1), dict(ws_bytes=batch.ws_bytes - 1), dict(stream_bytes=last - 1)):
        assert call(**kw) == -1, kw
        assert (out == 0x5A).all() and (status == 77).all(), kw
    assert lib.tt_png_decode_batch_workspace_bytes(table.ctypes.data, 2) == batch.ws_bytes
    assert call(stream_bytes=last) == 0 and status.tolist() == [0, 0]


def test_seeded_bit_flips_agree_with_zlib(fx, decoded):
    """FLIPS single-bit flips in the deflate stream (the Adler-32 trailer included) of EVERY small file.  Status 0 exactly when zlib
    accepts the stream, its length is H (1 + row_bytes) and every filter byte is <= 4; then the pixels are those the test's own unfilter
    makes of zlib's bytes.  The one-lane loop takes every flip, the 64-lane emulation those of eight files, the ones with a stored block behind a Huffman block among them."""
    names, batch = decoded[0], decoded[1]
    small = [i for i in range(len(names)) if batch.table[i]["stream_len"] <= SMALL]
    assert len(small) >= 30
    zeros = 0
    for i in small:
        rng = random.Random(1000 + i)
        n_bytes = int(batch.table[i]["stream_len"])
        flips = [(rng.randrange(n_bytes), rng.randrange(8)) for _ in range(FLIPS)]
        many = hip_ops.png_prepare_batch([fx[0][names[i]]] * FLIPS, threads=1, pin=False)
        streams, table = many.part("streams"), many.table
        for k, (at, bit) in enumerate(flips):
            streams[int(table[k]["stream_off"]) + at] ^= 1 << bit
        maps, status, _, _ = hip_ops.png_decode_host(many)
        wave = "stored_after" in names[i] or "three_block" in names[i] or small.index(i) % 8 == 0      # (64 threads a file: a subset)
        wave_maps, wave_status, _, _ = hip_ops.png_decode_host(many, lanes=64) if wave else (maps, status, None, None)
        assert np.array_equal(wave_status, status), names[i]
        H, W, depth = (int(table[0][f]) for f in ("H", "W", "depth"))
        for k in range(FLIPS):
            raw = P.zlib_accepts(streams[int(table[k]["stream_off"]):][:n_bytes].tobytes())
            want = None if raw is None else P.unfilter(raw, H, W, depth)
            assert (status[k] == 0) == (want is not None), (names[i], flips[k], status[k])
            if want is not None:
                zeros += 1
                assert (maps[k] == want[1]).all() and (wave_maps[k] == want[1]).all(), (names[i], flips[k])
    assert zeros > 0        # some flips fall into bits no decoder reads: the accepting side is exercised too


def test_the_fixture_reaches_every_case(decoded):
    """From the statistics the emulation returns: a regenerated fixture cannot silently lose a case."""
    names, batch, _, _, stats, _ = decoded
    col = {n: stats[:, k] for k, n in enumerate(hip_ops.PNG_STATS)}
    assert np.bitwise_or.reduce(col["kinds"]) == 7                             # stored, fixed and dynamic blocks
    assert any(k == 7 for k in col["kinds"])                                   # ... all three in one stream
    assert col["lit_bits"].max() == 15 and col["dist_bits"].max() == 15
    assert col["min_dist"].min() == 1 and col["max_dist"].max() == 32768 and (col["max_dist"] >= 16385).any()
    assert col["max_len"].max() == 258
    # a non-empty stored block BEHIND a Huffman block, where the lanes' pending literals have to be stored first: by hand and from zlib
    for n, kinds in (("craft_stored_after_7_literals", 3), ("craft_stored_after_100_literals", 7), ("gray_runs_then_noise_120x400", 5)):
        assert col["kinds"][names.index(n)] == kinds, n
    assert np.bitwise_or.reduce(col["filters"]) == 31
    assert {int(d) for d in batch.table["depth"]} == {1, 2, 4, 8} and {int(c) for c in batch.table["color_type"]} == {0, 3}
    assert {(1, 1), (1, 9), (3, 7), (7, 1), (63, 33), (64, 33), (65, 33), (130, 33), (375, 500), (480, 854)} <= {(i.H, i.W) for i in batch.infos}


def test_host_loader_logic(fx, tmp_path):
    """The pooled host route is the serial list; the device route's host half sorts files and counts the fall-backs without a GPU."""
    from timetuning_amd import data_loader as DL

    files = [fx[0][n] for n in list(fx[0])[:12]] + [fx[2]["interlaced"][1]]
    serial = [DL.decode_annotation(f) for f in files]
    for threads in (1, 4, 16):
        pooled = DL.decode_annotations(files, threads)
        assert len(pooled) == len(serial) and all(a.dtype == np.uint8 and np.array_equal(a, b) for a, b in zip(pooled, serial))
    host = DL.scan_annotations(files, 4, pin=False)
    assert host.device_slots == list(range(12)) and list(host.host_items) == [12] and len(host.batch.infos) == 12
    assert np.array_equal(host.host_items[12], serial[12])
    with pytest.raises(ValueError, match="malformed PNG"):
        DL.scan_annotations([files[0], files[0][:50]], 1, pin=False)
    maps = P.write_video_tree(str(tmp_path / "set"))
    ds = DL.VideoDataset(str(tmp_path / "set" / "JPEGImages"), str(tmp_path / "set" / "Annotations"), DL.SamplingMode.Full, 1, 4, device=None, threads=4)
    assert ds.png == "host" and ds.fallback_annotations == 0
    for v in range(3):
        s = ds.read_host(v)
        assert s.annotation_files is None and np.array_equal(s.annotations[0], np.stack([maps[(v, f)] for f in range(4)]))
        raw = ds.read_host(v, png="device")
        assert raw.annotations is None and [len(c) for c in raw.annotation_files] == [4]
    with pytest.raises(ValueError, match="png"):
        DL.VideoDataset(str(tmp_path / "set" / "JPEGImages"), None, DL.SamplingMode.Full, 1, 4, png="gpu")
    # a loader pools over the BATCH: one decode_annotations call for the 2 x 4 files of a batch of two videos, not one per video
    # (the frames' half pins memory, which needs a device: left out here)
    calls, pooled, frames = [], DL.decode_annotations, DL.scan_frames
    try:
        DL.decode_annotations = lambda files, threads=1: (calls.append(len(list(files))), pooled(files, threads))[1]
        DL.scan_frames = lambda *a, **k: None
        loader = DL.ClipLoader(ds, 2, prefetch=False)
        host = loader._host([0, 1])
    finally:
        DL.decode_annotations, DL.scan_frames = pooled, frames
    assert calls == [8] and host.annotations is None
    for v, s in enumerate(host.samples):
        assert s.annotation_files is None and np.array_equal(s.annotations[0], np.stack([maps[(v, f)] for f in range(4)]))


# ---- N27: the PNG half of what the two codecs share (the rest: tests/test_jpeg_host.py)
def test_status_vocabulary_png(fx):
    for index, where in ((None, ""), (3, "file 3: ")):
        e = hip_ops._PNG.error(1, index)
        assert type(e) is hip_ops.PngUnsupported and (e.status, e.index) == (1, index)
        assert str(e) == where + "unsupported PNG (Adam7 interlace)"
        e = hip_ops._PNG.error(-6, index)
        assert type(e) is ValueError and str(e) == where + "malformed PNG (status -6: a wrong CRC-32 or Adler-32)"
    assert str(hip_ops.PngUnsupported(99)) == "unsupported PNG (99)" and str(hip_ops._PNG.error(-99)) == "malformed PNG (status -99: unknown)"
    info = hip_ops.PngInfo(0, 480, 854, 8, 3)
    assert repr(info) == "PngInfo(status=0, H=480, W=854, depth=8, color_type=3)" and info.supported
    assert not hip_ops.PngInfo(2, 0, 0, 0, 0).supported
    assert not isinstance(hip_ops._PNG.error(1), hip_ops.JpegUnsupported) and not isinstance(hip_ops._JPEG.error(1), hip_ops.PngUnsupported)
    good = fx[0][list(fx[0])[0]]
    with pytest.raises(hip_ops.PngUnsupported, match=r"^file 3: unsupported PNG \(Adam7 interlace\)$") as e:
        hip_ops.png_prepare_batch([good] * 3 + [fx[2]["interlaced"][1], good[:50]], threads=2, pin=False)
    assert (e.value.status, e.value.index) == (1, 3)
    with pytest.raises(ValueError, match=r"^file 1: malformed PNG \(status -"):
        hip_ops.png_prepare_batch([good, good[:50]], threads=2, pin=False)
    with pytest.raises(ValueError, match=r"^malformed PNG \(status -"):
        hip_ops.png_probe(good[:50])
    with pytest.raises(ValueError, match="^png_prepare_batch: no files$"):
        hip_ops.png_prepare_batch([], pin=False)


def test_the_layout_of_a_png_batch(fx):
    files = [fx[0][n] for n in list(fx[0])[:3]]
    batch = hip_ops.png_prepare_batch(files, threads=2, pin=False)
    assert batch.layout["table"] == (0, 3 * 128) and batch.layout["streams"][0] == 3 * 128
    assert batch.meta.numel() == 3 * 128 + batch.layout["streams"][1] == 3 * 128 + sum((len(f) + 3) // 4 * 4 + 4 for f in files)
    for name, (at, size) in batch.layout.items():
        assert batch.part(name).ctypes.data == batch.meta.data_ptr() + at and batch.part(name).size == size      # views, not copies
    assert batch.table.ctypes.data == batch.meta.data_ptr()
