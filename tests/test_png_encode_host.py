"""N29 without a GPU: the host half of the PNG writer - tt_png_encode_host (the sequential loop over the kernels' steps of
csrc/png_deflate.hpp), tt_png_write_file and the table rules - against the plain-Python restatement of the format (tests/_png_enc_ref.py),
zlib, Pillow and the project's own N26 decoder."""
import ctypes as C
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import _png_enc_ref as R
from timetuning_amd import _lib, hip_ops

EARGUMENT = -8


@pytest.fixture(scope="module")
def maps():
    return R.map_list()


@pytest.fixture(scope="module")
def encoded(maps):
    """Every map of the list in ONE call of the emulation, wrapped into palette files: computed once."""
    streams, adlers = hip_ops.png_encode_host(list(maps.values()))
    files = hip_ops.png_wrap_files(streams, adlers, [m.shape for m in maps.values()], R.palette(), threads=4)
    return {n: (s.tobytes(), int(a), f) for n, s, a, f in zip(maps, streams, adlers, files)}


def test_streams_and_files_equal_the_restatement_byte_for_byte(maps, encoded):
    pal = R.palette()
    for n, m in maps.items():
        stream, adler, _ = R.stream(m)
        assert encoded[n][0] == stream, n
        assert encoded[n][1] == adler, n
        assert encoded[n][2] == R.png_file(m, pal), n
    one, ad = hip_ops.png_encode_host([maps["straddle"]])                         # alone in a call: the same bytes as inside the batch
    assert one[0].tobytes() == encoded["straddle"][0] and int(ad[0]) == encoded["straddle"][1]
    gray = hip_ops.png_wrap_files(one, ad, [maps["straddle"].shape])
    assert gray[0] == R.png_file(maps["straddle"])


def test_zlib_pillow_and_the_decoder_read_the_files_back(maps, encoded):
    pal = R.palette()
    names = list(maps)
    for n in names:
        f = encoded[n][2]
        assert zlib.decompress(R.idat_payload(f)) == R.filtered_image(maps[n]).tobytes(), n
        im = Image.open(io.BytesIO(f))
        assert im.mode == "P" and np.array_equal(np.asarray(im), maps[n]), n
        assert np.array_equal(np.asarray(im.getpalette(), np.uint8).reshape(-1, 3), pal), n
        info = hip_ops.png_probe(f)
        assert info.status == 0 and (info.H, info.W, info.depth, info.color_type) == (*maps[n].shape, 8, 3), n
    gray = hip_ops.png_wrap_files(*hip_ops.png_encode_host([maps["blob_375x500"]]), [maps["blob_375x500"].shape])[0]
    im = Image.open(io.BytesIO(gray))
    assert im.mode == "L" and np.array_equal(np.asarray(im), maps["blob_375x500"]) and hip_ops.png_probe(gray).color_type == 0
    short = hip_ops.png_wrap_files(*hip_ops.png_encode_host([maps["blob_375x500"]]), [maps["blob_375x500"].shape], R.palette(3))[0]
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(short)).getpalette(), np.uint8).reshape(-1, 3)[:3], R.palette(3))
    batch = hip_ops.png_prepare_batch([encoded[n][2] for n in names], threads=4, pin=False)
    back, status, stats, _ = hip_ops.png_decode_host(batch)
    assert status.tolist() == [0] * len(names)
    kinds, filters = hip_ops.PNG_STATS.index("kinds"), hip_ops.PNG_STATS.index("filters")
    for n, b, st in zip(names, back, stats):
        assert np.array_equal(b, maps[n]), n
        assert st[filters] == 1 << 2, n                                           # the filter set {2}
        assert st[kinds] == (1 << 0) | (1 << 1), n                               # stored + fixed blocks, no dynamic one


def test_streams_stay_within_the_capacity_and_noise_reaches_it(maps, encoded):
    for n, m in maps.items():
        cap = R.stream(m)[2]
        assert len(encoded[n][0]) <= cap, n
    for n in ("noise9_64x100", "noise9_1x32767"):
        cap = R.stream(maps[n])[2]
        assert len(encoded[n][0]) >= 0.99 * cap, n


def _tables(arrays):
    plan = hip_ops.png_encode_plan(arrays, pin=False)
    n = len(arrays)
    out, results = np.zeros(plan.out_bytes + 16, np.uint8), np.zeros(n, hip_ops._PNG_RESULT)
    ws = np.zeros(plan.ws_bytes // 16 + 2, np.dtype("<u8, <u8"))
    return plan, n, out, results, ws, ws.ctypes.data + (-ws.ctypes.data) % 16


def test_argument_validation(maps):
    lib = _lib.load()
    arrays = [maps["rows_163x100"], maps["1x2"], maps["blob_375x500"]]
    plan, n, out, results, ws, ws_at = _tables(arrays)

    def call(**kw):
        a = dict(maps=plan.table.ctypes.data, n=n, chunks=plan.chunks.ctypes.data, n_chunks=plan.n_chunks, out=out.ctypes.data, out_bytes=plan.out_bytes,
                 results=results.ctypes.data, ws=ws_at, ws_bytes=plan.ws_bytes)
        a.update(kw)
        return lib.tt_png_encode_host(a["maps"], None, a["n"], a["chunks"], None, a["n_chunks"], a["out"], a["out_bytes"], a["results"], a["ws"],
                                      a["ws_bytes"], None)

    assert call() == 0

    def doctored(part, field, value, row=1):
        t = (plan.table if part == "maps" else plan.chunks).copy()
        t[field][row] = value
        return t

    for part, field, value, row in [("maps", "data", 0, 1), ("maps", "H", 0, 1), ("maps", "H", 32768, 1), ("maps", "W", 0, 1), ("maps", "W", 32768, 1),
                                    ("maps", "pitch", 1, 1), ("maps", "first_chunk", 0, 1), ("maps", "n_chunks", 2, 1), ("maps", "out_off", 0, 1),
                                    ("chunks", "map", 0, 2), ("chunks", "row0", 1, 1), ("chunks", "rows", 500, 0), ("chunks", "slot_off", 4, 0)]:
        t = doctored(part, field, value, row)
        assert call(**{part: t.ctypes.data}) == EARGUMENT, (part, field, value)
    for kw in ({"maps": None}, {"chunks": None}, {"out": None}, {"results": None}, {"ws": None}, {"ws": ws_at + 4}, {"n": 0}, {"n": 70000},
               {"n_chunks": plan.n_chunks - 1}, {"out_bytes": plan.out_bytes - 1}, {"ws_bytes": plan.ws_bytes - 1}):
        assert call(**kw) == EARGUMENT, kw
    # the plan and the size queries refuse the same rows
    nc, cap = C.c_longlong(), C.c_longlong()
    for field, value in (("data", 0), ("H", 0), ("W", 40000), ("pitch", 1)):
        t = doctored("maps", field, value)
        assert lib.tt_png_encode_plan(t.ctypes.data, n, None, 0, C.byref(nc), C.byref(cap)) == EARGUMENT
        assert lib.tt_png_encode_batch_workspace_bytes(t.ctypes.data, n) == 0
    t = plan.table.copy()
    short = np.zeros(plan.n_chunks - 1, hip_ops._PNG_CHUNK)
    assert lib.tt_png_encode_plan(t.ctypes.data, n, short.ctypes.data, short.size, C.byref(nc), C.byref(cap)) == EARGUMENT
    assert lib.tt_png_encode_plan(t.ctypes.data, n, None, 0, None, C.byref(cap)) == EARGUMENT
    # the file writer
    stream, adler = (x[0] for x in hip_ops.png_encode_host([maps["1x2"]]))
    size = lib.tt_png_file_bytes(stream.size, 2)
    buf, got, pal = np.zeros(size, np.uint8), C.c_size_t(), R.palette(2)
    args = [stream.ctypes.data, stream.size, int(adler), 1, 2, pal.ctypes.data, 2, buf.ctypes.data, size, C.byref(got)]
    assert lib.tt_png_write_file(*args) == 0 and got.value == size and buf.tobytes() == R.png_file(maps["1x2"], pal)
    for at, value in ((0, None), (3, 0), (3, 32768), (4, 0), (4, 40000), (5, None), (6, 257), (6, 0), (7, None), (8, size - 1), (9, None)):
        bad = list(args)
        bad[at] = value
        assert lib.tt_png_write_file(*bad) == EARGUMENT, (at, value)


def test_input_forms_of_the_emulation(maps):
    m = maps["blob_375x500"]
    want = hip_ops.png_encode_host([m])[0][0].tobytes()
    wide = np.zeros((375, 700), np.uint8)
    wide[:, 100:600] = m
    view = wide[:, 100:600]
    assert hip_ops.png_encode_plan([view], pin=False).table["pitch"][0] == 700
    assert hip_ops.png_encode_host([view])[0][0].tobytes() == want                # a pitched view, taken as it is
    stack = np.stack([m, m[::-1]])
    both = hip_ops.png_encode_host(stack)[0]
    assert both[0].tobytes() == want and both[1].tobytes() == hip_ops.png_encode_host([np.ascontiguousarray(m[::-1])])[0][0].tobytes()
    assert hip_ops.png_encode_host([m.astype(np.int64)])[0][0].tobytes() == want
    bad = m.astype(np.int64)
    bad[3, 3] = 256
    with pytest.raises(ValueError, match="map 1 .*256"):
        hip_ops.png_encode_host([m, bad])
    with pytest.raises(TypeError):
        hip_ops.png_encode_host([m.astype(np.float32)])
    with pytest.raises(ValueError):
        hip_ops.png_encode_host(m[None, None])
    with pytest.raises(ValueError):
        hip_ops.png_encode_host([])
