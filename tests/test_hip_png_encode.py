"""N29 on the GPU: tt_png_encode_batch against the host emulation - equality of every stream byte and Adler-32 - for the maps of
tests/_png_enc_ref.py, all in one call, each alone and on a workspace that is not cleared; the finished files through the project's own
device decoder and through Pillow; the input forms; launch hygiene; ``my_utils.imwrite_indexed`` / ``write_indexed_clip`` and
``mask_propagation --save_masks``."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import _png_enc_ref as R
from timetuning_amd import _lib, hip_ops

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 256, 0x5A


@pytest.fixture(scope="module")
def maps():
    return R.map_list()


@pytest.fixture(scope="module")
def host(maps):
    """The emulation's streams and Adler-32 of every map, computed once (tests/test_png_encode_host.py holds it to the restatement)."""
    streams, adlers = hip_ops.png_encode_host(list(maps.values()))
    return {n: (s.tobytes(), int(a)) for n, s, a in zip(maps, streams, adlers)}


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class RawCall:
    """tt_png_encode_batch on buffers of its own: the output between guards of sentinels, the workspace kept from call to call."""

    def __init__(self, tensors, ws_fill=None):
        self.lib = _lib.load()
        self.plan = hip_ops.png_encode_plan(tensors)
        self.n = len(tensors)
        self.dev = tensors[0].device
        self.meta = self.plan.meta.to(self.dev)
        self.ws = torch.zeros(self.plan.ws_bytes, dtype=torch.uint8, device=self.dev)
        if ws_fill is not None:
            self.ws.fill_(ws_fill)
        self.buf = torch.empty(self.plan.out_bytes + 2 * GUARD, dtype=torch.uint8, device=self.dev)
        self.results = torch.empty(self.n * 32, dtype=torch.uint8, device=self.dev)

    def launch(self, **kw):
        p = self.plan
        a = dict(maps_host=p.table.ctypes.data, maps_dev=self.meta.data_ptr() + p.layout["maps"][0], n=self.n, chunks_host=p.chunks.ctypes.data,
                 chunks_dev=self.meta.data_ptr() + p.layout["chunks"][0], n_chunks=p.n_chunks, out=self.buf.data_ptr() + GUARD, out_bytes=p.out_bytes,
                 results=self.results.data_ptr(), ws=self.ws.data_ptr(), ws_bytes=p.ws_bytes)
        a.update(kw)
        return self.lib.tt_png_encode_batch(a["maps_host"], a["maps_dev"], a["n"], a["chunks_host"], a["chunks_dev"], a["n_chunks"], a["out"],
                                            a["out_bytes"], a["results"], a["ws"], a["ws_bytes"], torch.cuda.current_stream().cuda_stream)

    def run(self):
        self.buf.fill_(SENTINEL)
        self.results.fill_(SENTINEL)
        assert self.launch() == 0
        torch.cuda.synchronize()
        return self.read()

    def read(self):
        res = self.results.cpu().numpy().view(hip_ops._PNG_RESULT)
        buf = self.buf.cpu().numpy()
        total = int(res["offset"][-1] + res["length"][-1])
        assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + total:] == SENTINEL).all(), "a byte outside the streams was written"
        assert res["offset"][0] == 0 and (res["offset"][1:] == np.cumsum(res["length"])[:-1]).all(), "the streams are not compact"
        return [(buf[GUARD + int(r["offset"]):GUARD + int(r["offset"] + r["length"])].tobytes(), int(r["adler"])) for r in res]


def test_all_maps_in_one_call_twice_on_a_stale_workspace(maps, host):
    """Mixed sizes, every chunk shape and both staging routes in ONE call; the second call runs on the first one's workspace, the third
    on a workspace of ones, so a bit a slot kept would show."""
    names = list(maps)
    call = RawCall([gpu(maps[n]) for n in names])
    for fill in (None, None, 0xFF):
        if fill is not None:
            call.ws.fill_(fill)
        got = call.run()
        for n, g in zip(names, got):
            assert g == host[n], n


def test_each_map_alone_in_a_call(maps, host):
    for n, m in maps.items():
        assert RawCall([gpu(m)], ws_fill=0xA5).run() == [host[n]], n
    streams, adlers = hip_ops.png_encode([gpu(maps["blob_375x500"]), gpu(maps["1x1"])])          # the public call
    assert [(s.tobytes(), int(a)) for s, a in zip(streams, adlers)] == [host["blob_375x500"], host["1x1"]]


def test_files_round_trip_through_the_device_decoder_and_pillow(maps):
    names = list(maps)
    pal = R.palette()
    files = hip_ops.encode_png_batch([gpu(maps[n]) for n in names], palette=pal)
    assert all(isinstance(f, bytes) for f in files)
    back = hip_ops.decode_png_batch(files)
    for n, f, b in zip(names, files, back):
        assert b.is_cuda and np.array_equal(b.cpu().numpy(), maps[n]), n
        im = Image.open(io.BytesIO(f))
        assert im.mode == "P" and np.array_equal(np.asarray(im), maps[n]), n
        assert np.array_equal(np.asarray(im.getpalette(), np.uint8).reshape(-1, 3), pal), n
        assert f == R.png_file(maps[n], pal), n
    gray = hip_ops.encode_png_batch([gpu(maps["blob_375x500"])])
    im = Image.open(io.BytesIO(gray[0]))
    assert im.mode == "L" and np.array_equal(np.asarray(im), maps["blob_375x500"])


def test_stacks_pitched_views_and_mixed_lists_equal_their_contiguous_copies(maps):
    rng = np.random.default_rng(3)
    stack = gpu(np.stack([R.blob_map(70, 90, s) for s in range(3)]))
    each = hip_ops.encode_png_batch([stack[i].clone() for i in range(3)])
    assert hip_ops.encode_png_batch(stack) == each
    wide = gpu(rng.integers(0, 4, (70, 300)).astype(np.uint8))
    view = wide[:, 17:107]
    assert view.stride() == (300, 1) and not view.is_contiguous()
    assert hip_ops.encode_png_batch([view]) == hip_ops.encode_png_batch([view.contiguous()])
    assert hip_ops.png_encode_plan([view]).table["pitch"][0] == 300                                  # taken as it is, not copied
    mixed = [stack[1], view, gpu(maps["1x2"]), stack[0].t()]                                         # the last one: columns as rows, copied
    assert hip_ops.encode_png_batch(mixed) == [f for m in mixed for f in hip_ops.encode_png_batch([m.contiguous()])]
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(hip_ops.encode_png_batch(mixed)[3]))), stack[0].t().cpu().numpy())


def test_integer_predictions_convert_and_values_past_255_raise(maps):
    m = maps["blob_375x500"]
    pred = gpu(m.astype(np.int64))
    assert hip_ops.encode_png_batch([pred]) == hip_ops.encode_png_batch([gpu(m)])
    assert hip_ops.encode_png_batch([gpu(m.astype(np.int32)), gpu(m)])[0] == hip_ops.encode_png_batch([gpu(m)])[0]
    bad = pred.clone()
    bad[5, 5] = 256
    with pytest.raises(ValueError, match="map 1 .*256"):
        hip_ops.encode_png_batch([pred, bad])
    bad[5, 5] = -1
    with pytest.raises(ValueError, match="map 0"):
        hip_ops.encode_png_batch([bad])
    with pytest.raises(TypeError):
        hip_ops.encode_png_batch([pred.float()])
    with pytest.raises(_lib.HipLibraryError, match="GPU"):
        hip_ops.encode_png_batch([torch.from_numpy(m)])
    with pytest.raises(ValueError, match="palette"):
        hip_ops.encode_png_batch([gpu(m)], palette=np.zeros((257, 3), np.uint8))
    with pytest.raises(ValueError):
        hip_ops.encode_png_batch(gpu(m)[None, None])


def test_table_validation_refuses_without_launching(maps):
    names = ["rows_163x100", "1x2", "blob_375x500"]
    call = RawCall([gpu(maps[n]) for n in names])
    want = call.run()
    p = call.plan

    def doctored(part, field, value, row=1):
        t = (p.table if part == "maps" else p.chunks).copy()
        t[field][row] = value
        return {("maps_host" if part == "maps" else "chunks_host"): t.ctypes.data, "keep": t}

    cases = [doctored("maps", "data", 0), doctored("maps", "H", 0), doctored("maps", "W", 32768), doctored("maps", "H", 40000),
             doctored("maps", "pitch", 1), doctored("maps", "first_chunk", 0), doctored("maps", "n_chunks", 2), doctored("maps", "out_off", 0),
             doctored("chunks", "map", 0, row=2), doctored("chunks", "row0", 1), doctored("chunks", "rows", 500, row=0),
             doctored("chunks", "slot_off", 4, row=0),
             {"out_bytes": p.out_bytes - 1}, {"ws_bytes": p.ws_bytes - 1}, {"n_chunks": p.n_chunks - 1}, {"n": 0},
             {"maps_host": None}, {"maps_dev": None}, {"chunks_host": None}, {"chunks_dev": None}, {"out": None}, {"results": None}, {"ws": None},
             {"ws": call.ws.data_ptr() + 4}]
    for kw in cases:
        call.buf.fill_(SENTINEL)
        call.results.fill_(SENTINEL)
        kw = dict(kw)
        kw.pop("keep", None)
        assert call.launch(**kw) == -8, kw                                                         # TT_PNG_EARGUMENT
        assert "png_encode_batch" in call.lib.tt_last_error().decode()
        torch.cuda.synchronize()
        assert (call.buf == SENTINEL).all() and (call.results == SENTINEL).all(), kw
    assert call.run() == want


def test_launch_neither_allocates_nor_breaks_capture(maps, host):
    names = ["blob_375x500", "straddle", "1x32767"]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call = RawCall([gpu(maps[n]) for n in names])
        want = [host[n] for n in names]

        def launch():
            assert call.launch() == 0

        launch()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(3):
            call.buf.fill_(SENTINEL)
            launch()
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0, "a launch changed the device's free memory"
        assert call.read() == want
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch()
        for _ in range(2):
            call.buf.fill_(SENTINEL)
            call.results.fill_(SENTINEL)
            g.replay()
            torch.cuda.synchronize()
            assert call.read() == want


def test_imwrite_indexed_and_write_indexed_clip(tmp_path, maps):
    from timetuning_amd import my_utils, visualization

    pal = R.palette(21)
    m = maps["blob_375x500"]
    for k, array in enumerate((gpu(m), m, gpu(m.astype(np.int64)))):                                 # a GPU tensor, a NumPy array (uploaded), int64
        path = str(tmp_path / f"one{k}.png")
        my_utils.imwrite_indexed(path, array, pal)
        im = Image.open(path)
        assert im.mode == "P" and np.array_equal(np.asarray(im), m)
        assert np.array_equal(np.asarray(im.getpalette(), np.uint8).reshape(-1, 3)[:21], pal)
    with pytest.raises(Exception, match="2D|2-D|2 dim"):
        my_utils.imwrite_indexed(str(tmp_path / "no.png"), gpu(m)[None], pal)
    clip = gpu(np.stack([R.blob_map(48, 64, s) for s in range(5)]))
    paths = my_utils.write_indexed_clip(str(tmp_path / "clip"), clip)
    assert [os.path.basename(p) for p in paths] == [f"{t:05d}.png" for t in range(5)]
    for t, path in enumerate(paths):
        im = Image.open(path)
        assert im.mode == "P" and np.array_equal(np.asarray(im), clip[t].cpu().numpy())
        assert np.array_equal(np.asarray(im.getpalette(), np.uint8).reshape(-1, 3), visualization.voc_palette())
    named = my_utils.write_indexed_clip(str(tmp_path / "named"), clip[:2], pal, names=["a.png", "b.png"])
    assert [os.path.basename(p) for p in named] == ["a.png", "b.png"] and np.array_equal(np.asarray(Image.open(named[1])), clip[1].cpu().numpy())
    with pytest.raises(ValueError):
        my_utils.write_indexed_clip(str(tmp_path / "bad"), clip[:2], names=["only_one.png"])


def test_mask_propagation_save_masks_writes_what_it_scores(tmp_path):
    from timetuning_amd import mask_propagation as MP
    from timetuning_amd import synth, visualization

    tiny = synth.ARCHS["tiny-s16"]
    out = {}
    for flow in (False, True):
        root = tmp_path / ("flow" if flow else "feat")
        argv = ["--dataset", "synthetic", "--model_path", "", "--input_resolution", "64", "--num_clips", "2",
                "--num_frames", "4", "--save_masks", str(root)] + (["--use_optical_flow", "True"] if flow else [])
        args = MP.build_parser().parse_args(argv)
        mean = MP.mask_propagation(args, vit_cfg=tiny)
        js = []
        for i in range(2):
            _, masks = MP.synthetic_tracking_clip(4, 64, seed=i + 1)
            masks = (masks > 0).long()                                                             # --uvos is on by default
            frames = []
            for t in range(4):
                im = Image.open(root / f"clip_{i:04d}" / f"{t:05d}.png")
                assert im.mode == "P" and im.size == (64, 64)
                assert np.array_equal(np.asarray(im.getpalette(), np.uint8).reshape(-1, 3), visualization.voc_palette())
                frames.append(np.asarray(im))
            assert not (root / f"clip_{i:04d}" / "00004.png").exists()
            assert np.array_equal(frames[0], masks[0].numpy())                                     # frame 0: the seed as propagated from
            pred = torch.from_numpy(np.stack(frames[1:]).astype(np.int64)).cuda()
            js.append(MP.jaccard(pred, masks[1:].cuda(), int(masks.max()) + 1)[0])
        assert sum(js) / len(js) == mean                                                          # the files ARE the predictions scored
        out[flow] = mean
    args = MP.build_parser().parse_args(["--dataset", "synthetic", "--model_path", "", "--input_resolution", "64", "--num_clips", "2",
                                         "--num_frames", "4"])
    assert args.save_masks is None and MP.mask_propagation(args, vit_cfg=tiny) == out[False]                    # default off, same score


def test_save_masks_names_the_clips_of_a_tree_on_disk_after_their_videos(tmp_path):
    import _png_ref as P
    from timetuning_amd import mask_propagation as MP
    from timetuning_amd import synth

    P.write_video_tree(str(tmp_path / "set"), videos=2, frames=3, H=64, W=64)
    argv = ["--dataset", "davis_val", "--dataset_path", str(tmp_path / "set"), "--model_path", "", "--input_resolution", "64", "--num_frames", "3",
            "--num_workers", "2"]
    plain = MP.mask_propagation(MP.build_parser().parse_args(argv), vit_cfg=synth.ARCHS["tiny-s16"])
    saved = MP.mask_propagation(MP.build_parser().parse_args(argv + ["--save_masks", str(tmp_path / "out")]), vit_cfg=synth.ARCHS["tiny-s16"])
    assert saved == plain
    assert sorted(os.listdir(tmp_path / "out")) == ["video0", "video1"]
    for v in range(2):
        assert sorted(os.listdir(tmp_path / "out" / f"video{v}")) == ["00000.png", "00001.png", "00002.png"]
        im = Image.open(tmp_path / "out" / f"video{v}" / "00000.png")
        assert im.mode == "P" and im.size == (64, 64) and set(np.unique(np.asarray(im)).tolist()) <= {0, 1}      # --uvos: one foreground class
