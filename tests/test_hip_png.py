"""N26 on the GPU: tt_png_decode_batch against Pillow's decode and against the emulation - equality of every byte - for all supported
files of tests/golden/png_streams.npz, the status of the fixture's broken files between good ones, the table validation, launch hygiene,
and the loaders and the evaluation command line with png="device"."""
import numpy as np
import pytest
import torch

import _png_ref as P
from timetuning_amd import _lib, hip_ops

pytestmark = pytest.mark.gpu
GUARD, GAP, SENTINEL = 256, 24, 0x5A


@pytest.fixture(scope="module")
def fx():
    return P.fixture()


@pytest.fixture(scope="module")
def pillow(fx):
    """The yardstick, computed once."""
    return {n: P.pillow(d) for n, d in fx[0].items()}


def raw_call(batch, table=None, out_bytes=None, ws_bytes=None, stream_bytes=None, misalign=0):
    """tt_png_decode_batch with the output inside a buffer of sentinels; ``table``: a doctored table (host AND device copy)."""
    lib, n = _lib.load(), len(batch.infos)
    dev = torch.device("cuda", torch.cuda.current_device())
    table = np.ascontiguousarray(batch.table if table is None else table)
    size = batch.out_bytes + GAP * n if out_bytes is None else out_bytes          # room for spread(), not for a doctored offset
    meta = batch.meta.to(dev)
    table_dev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(dev)
    buf = torch.full((size + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    status = torch.full((n,), 77, dtype=torch.int32, device=dev)
    need = max(int(lib.tt_png_decode_batch_workspace_bytes(table.ctypes.data, n)), batch.ws_bytes)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
    rc = lib.tt_png_decode_batch(meta.data_ptr() + batch.layout["streams"][0] + misalign, batch.layout["streams"][1] if stream_bytes is None else stream_bytes,
                                 table.ctypes.data, table_dev.data_ptr(), n, buf.data_ptr() + GUARD, size, ws.data_ptr(),
                                 need if ws_bytes is None else ws_bytes, status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    stats = ws[need - 32 * n:need].view(torch.int32).view(n, 8).cpu().numpy()
    return rc, buf.cpu().numpy(), status.cpu().numpy(), stats, table


def spread(batch):
    """The batch's table with GAP bytes between the outputs: what lies in the gaps must stay."""
    t = batch.table.copy()
    t["out_off"] += GAP * np.arange(len(t))
    return t


def check_maps(buf, table, names, want, status):
    covered = np.zeros(buf.size, bool)
    covered[:GUARD] = covered[-GUARD:] = False
    for i, n in enumerate(names):
        if status[i] != 0:
            continue
        at, (H, W) = GUARD + int(table[i]["out_off"]), want[n].shape
        assert (buf[at:at + H * W].reshape(H, W) == want[n]).all(), n
    for i in range(len(table)):
        at = GUARD + int(table[i]["out_off"])
        covered[at:at + int(table[i]["H"] * table[i]["W"])] = True
    assert (buf[~covered] == SENTINEL).all(), "a byte outside the files' maps was written"


def test_all_supported_files_in_one_call(fx, pillow):
    """48 files of every depth, size and deflate shape in ONE launch, one wave per file; maps equal Pillow's and the emulation's."""
    names = list(fx[0])
    batch = hip_ops.png_prepare_batch([fx[0][n] for n in names], threads=4)
    rc, buf, status, stats, table = raw_call(batch, spread(batch))
    assert rc == 0 and status.tolist() == [0] * len(names)
    check_maps(buf, table, names, pillow, status)
    host_maps, host_status, host_stats, _ = hip_ops.png_decode_host(batch)
    assert np.array_equal(host_status, status) and np.array_equal(host_stats, stats)      # the emulation: the same counters, file by file
    assert all(np.array_equal(m, pillow[n]) for m, n in zip(host_maps, names))
    maps, st = hip_ops.png_decode(batch)                                                     # the public call: views of ONE flat buffer
    assert st.tolist() == [0] * len(names) and all(np.array_equal(m.cpu().numpy(), pillow[n]) for m, n in zip(maps, names))
    assert len({m.untyped_storage().data_ptr() for m in maps}) == 1
    got = hip_ops.decode_png_batch([fx[0][n] for n in names[:5]], threads=2)
    assert all(np.array_equal(m.cpu().numpy(), pillow[n]) for m, n in zip(got, names))


def test_each_file_alone_in_a_call(fx, pillow):
    for n, data in fx[0].items():
        batch = hip_ops.png_prepare_batch([data], threads=1)
        rc, buf, status, _, table = raw_call(batch)
        assert rc == 0 and status.tolist() == [0], n
        check_maps(buf, table, [n], pillow, status)


def test_broken_files_between_good_ones(fx, pillow):
    """Only the fixture's broken list: each of them the emulation (tests/test_png_host.py) and the sanitizer program have handled on the
    CPU, and every access of the kernel is bounds-checked by construction."""
    good = ["z4_63x33_d8", "craft_three_block_kinds", "z1_65x33_d4"]
    bad = [(n, s, d) for n, (s, d) in fx[1].items() if n != "wrong_idat_crc"]         # (that one never leaves the host half)
    order, k = [], 0
    for n, s, d in bad:
        order += [(good[k % 3], 0, fx[0][good[k % 3]]), (n, s, d)]
        k += 1
    order.append((good[0], 0, fx[0][good[0]]))
    batch = hip_ops.png_prepare_batch([d for _, _, d in order], threads=2)
    rc, buf, status, stats, table = raw_call(batch, spread(batch))
    assert rc == 0 and status.tolist() == [s for _, s, _ in order]
    for lanes in (1, 64):                                   # the emulations: the same status AND counters, failed files included
        host = hip_ops.png_decode_host(batch, lanes)
        assert np.array_equal(host[1], status) and np.array_equal(host[2], stats), lanes
    # a failed file's pixels are unspecified INSIDE its slice: the good maps, the gaps and the guards are what they must be
    check_maps(buf, table, [n for n, _, _ in order], pillow, status)
    with pytest.raises(ValueError, match=r"file 1: malformed PNG \(status -6"):
        hip_ops.png_decode(hip_ops.png_prepare_batch([fx[0][good[0]], fx[1]["wrong_adler"][1]], threads=1))
    with pytest.raises(ValueError, match=r"file 1: malformed PNG \(status -6"):
        hip_ops.decode_png_batch([fx[0][good[0]], fx[1]["wrong_idat_crc"][1]])


def test_table_validation_refuses_without_launching(fx, pillow):
    lib = _lib.load()
    names = ["z4_63x33_d8", "z1_65x33_d4", "z3_3x7_d1"]
    batch = hip_ops.png_prepare_batch([fx[0][n] for n in names], threads=1)
    good = batch.table.copy()

    def table(field, value, row=1):
        t = good.copy()
        t[field][row] = value
        return {"table": t}

    streams = batch.layout["streams"][1]
    cases = [table("out_off", batch.out_bytes), table("out_off", -1), table("out_off", int(good["out_off"][0]) + 5),           # past the buffer, overlap
             table("stream_off", streams), table("stream_off", int(good["stream_off"][1]) + 2), table("stream_off", -4),
             table("stream_len", streams), table("stream_len", -1),
             table("ws_off", int(good["ws_off"][0]) + 16), table("ws_off", -16), table("ws_off", 1 << 50),
             table("H", 0), table("W", 40000), table("depth", 3), table("color_type", 2), table("row_bytes", int(good["row_bytes"][1]) + 1),
             table("depth", 4, row=0),
             {"out_bytes": batch.out_bytes - 1}, {"ws_bytes": batch.ws_bytes - 1}, {"stream_bytes": int(good["stream_off"][2]) + 3}, {"misalign": 2}]
    for kw in cases:
        rc, buf, status, _, _ = raw_call(batch, **kw)
        assert rc == -1, kw
        assert "png_decode_batch" in lib.tt_last_error().decode()
        assert (buf == SENTINEL).all() and (status == 77).all(), kw
    rc, buf, status, _, t = raw_call(batch)
    assert rc == 0 and status.tolist() == [0, 0, 0]
    check_maps(buf, t, names, pillow, status)


def test_launch_neither_allocates_nor_breaks_capture(fx, pillow):
    lib = _lib.load()
    names = ["pillow_375x500", "craft_dist32768_len3", "z4_130x33_d2"]
    batch = hip_ops.png_prepare_batch([fx[0][n] for n in names], threads=1)
    dev = torch.device("cuda", torch.cuda.current_device())
    n, table = len(names), batch.table
    want = np.concatenate([pillow[k].reshape(-1) for k in names])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        meta = batch.meta.to(dev)
        out = torch.full((batch.out_bytes,), 7, dtype=torch.uint8, device=dev)
        status = torch.full((n,), 7, dtype=torch.int32, device=dev)
        ws = torch.zeros(batch.ws_bytes, dtype=torch.uint8, device=dev)

        def launch():
            rc = lib.tt_png_decode_batch(meta.data_ptr() + batch.layout["streams"][0], batch.layout["streams"][1], table.ctypes.data, meta.data_ptr(), n,
                                         out.data_ptr(), out.numel(), ws.data_ptr(), ws.numel(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0

        launch()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(3):
            out.fill_(7)
            launch()
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0, "a launch changed the device's free memory"
        assert np.array_equal(out.cpu().numpy(), want) and status.tolist() == [0] * n
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch()
        for _ in range(2):
            out.fill_(7)
            status.fill_(7)
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want) and status.tolist() == [0] * n


def test_clip_loader_with_device_png_equals_the_host_route(tmp_path):
    from timetuning_amd import video_transformations as VT
    from timetuning_amd.data_loader import ClipLoader, SamplingMode, VideoDataset, make_loader, maps_as_clip

    P.write_video_tree(str(tmp_path / "set"))
    root, out = tmp_path / "set", {}
    for png in ("host", "device"):
        ds = VideoDataset(str(root / "JPEGImages"), str(root / "Annotations"), SamplingMode.Full, 1, 4, video_transform=VT.evaluation_transforms(32))
        loader = ClipLoader(ds, 2, shuffle=False, seed=7, png=png)
        assert loader.png == png and ds.png == "host"                # the loader's choice: a dataset two loaders share keeps its own
        out[png] = (list(loader), loader.fallback_annotations)
    assert out["host"][1] == 0 and out["device"][1] == 1            # the interlaced map: Pillow, counted
    assert len(out["host"][0]) == len(out["device"][0]) == 2
    for a, b in zip(out["host"][0], out["device"][0]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert out["host"][0][0][1].dtype == torch.uint8 and out["host"][0][0][1].any()
    made = make_loader(str(root), 4, 2, sampling_mode=SamplingMode.Full, video_transform=VT.evaluation_transforms(32), png="device")
    assert made.dataset.png == "device" and made.png == "device" and torch.equal(next(iter(made))[1], out["host"][0][0][1])
    with pytest.raises(ValueError, match="png"):
        ClipLoader(ds, 2, png="gpu")
    # a clip of equal-sized maps is a view of the decode's buffer, not a copy
    files = [(root / "Annotations" / "video0" / f"{f:05d}.png").read_bytes() for f in range(4)]
    maps = hip_ops.decode_png_batch(files)
    clip = maps_as_clip(maps)
    assert clip.shape == (4, 24, 32) and clip.data_ptr() == maps[0].data_ptr()
    # a supported file with a broken stream is an error on the device route, not a fallback
    bad = P.fixture()[1]["wrong_adler"][1]
    (root / "Annotations" / "video2" / "00001.png").write_bytes(bad)
    ds = VideoDataset(str(root / "JPEGImages"), str(root / "Annotations"), SamplingMode.Full, 1, 4, video_transform=VT.evaluation_transforms(32), png="device")
    with pytest.raises(ValueError, match="malformed PNG"):
        list(ClipLoader(ds, 3))
    assert ds.fallback_annotations == 0


def test_pascal_loader_with_device_png_equals_the_host_route(tmp_path):
    import _voc_ref as V
    from timetuning_amd.leoloader import pascal_loader

    root = str(tmp_path / "voc")
    names = V.make_voc_tree(root)
    from PIL import Image
    for k, name in enumerate(names[:3]):           # hand-built files in place of Pillow's: depth 8 with cycling filters, and one interlaced
        for d in ("SegmentationClass", "SegmentationClassAug"):
            path = f"{root}/{d}/{name}.png"
            idx = np.asarray(Image.open(path))
            with open(path, "wb") as f:
                f.write(P.label_png(idx, 8, interlaced=(k == 1)))
    out = {}
    for png in ("host", "device"):
        loader = pascal_loader(3, root, "val", 24, train_size=32, png=png)
        out[png] = (list(loader), loader.fallback_annotations)
    assert out["host"][1] == 0 and out["device"][1] == 1
    assert len(out["host"][0]) == len(out["device"][0]) == 2
    for (xa, ya), (xb, yb) in zip(out["host"][0], out["device"][0]):
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
    with pytest.raises(ValueError, match="png"):
        pascal_loader(3, root, "val", 24, png="gpu")


def test_evaluation_command_line_scores_the_same_on_both_routes(tmp_path):
    from timetuning_amd import evaluation as E
    from timetuning_amd import synth

    P.write_video_tree(str(tmp_path / "set"), H=64, W=64)
    argv = ["--dataset", "davis_val", "--dataset_path", str(tmp_path / "set"), "--model_path", "", "--input_resolution", "64", "--batch_size", "2",
            "--num_frames", "2", "--num_clusters", "4", "--num_workers", "2"]
    host = E.main(argv + ["--png_decode", "host"], vit_cfg=synth.ARCHS["tiny-s16"])
    assert E.main(argv + ["--png_decode", "device"], vit_cfg=synth.ARCHS["tiny-s16"]) == host
    assert E.main(argv, vit_cfg=synth.ARCHS["tiny-s16"]) == host and 0.0 <= host <= 1.0
    assert E.build_parser().parse_args([]).png_decode == "host"
