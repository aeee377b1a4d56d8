"""N24 on the GPU: tt_jpeg_entropy_batch against tt_jpeg_scan of the same bytes - equality of every int16 coefficient, no tolerance - for
all supported files of tests/golden/jpeg_frames.npz and tests/golden/jpeg_entropy.npz, the pixels of the whole route against Pillow's, the
status of broken streams, the table validation, launch hygiene, and the clip loader with jpeg_entropy="device"."""
import os

import numpy as np
import pytest
import torch

import _jpeg_ref as R
import test_hip_jpeg as J
import test_jpeg_entropy_host as H
from timetuning_amd import _lib, hip_ops

pytestmark = pytest.mark.gpu
NEW = ["noise_96x136_444_q100", "noise_96x136_420_q100_opt", "flat_200x264_420_q30", "rst1_40x56_422_q90", "rst7_40x56_422_q90"]
# three fixed single-bit flips in the scan that tt_jpeg_scan rejects (a code no table holds, a restart marker not reached, a run past 63)
FLIPS = [("noise_96x136_420_q100_opt", 6674, 7, -3), ("rst7_40x56_422_q90", 914, 7, -5), ("clip_v0_f0", 930, 6, -4)]


@pytest.fixture(scope="module")
def files():
    return H.supported_files()


@pytest.fixture(scope="module")
def scans(files):
    """The yardstick, computed once: hip_ops.jpeg_scan of every file."""
    return {n: hip_ops.jpeg_scan(d) for n, d in files.items()}


@pytest.fixture(scope="module")
def fx():
    return R.fixture(J.GOLDEN)


def flipped(files, name, at, bit):
    d = files[name]
    return d[:at] + bytes([d[at] ^ (1 << bit)]) + d[at + 1:]


def check_batch(names, files, scans, subseq_bits):
    batch = hip_ops.jpeg_prepare_batch([files[n] for n in names], threads=4)
    coeffs, status, _, stats = hip_ops.jpeg_entropy_decode(batch, subseq_bits=subseq_bits, stats=True)
    got, rows = coeffs.cpu().numpy(), H.stream_rows(batch)
    assert status.tolist() == [0] * len(names)
    wrong = [n for i, n in enumerate(names) if not np.array_equal(got[rows[i, 9]:rows[i, 9] + scans[n][0].n_coeffs], scans[n][1])]
    assert not wrong, wrong[:10]
    # the emulation is the kernel lane by lane: the same rounds, tiles and subsequences
    assert np.array_equal(stats, hip_ops.jpeg_entropy_host(batch, subseq_bits)[2])
    return stats


@pytest.mark.parametrize("subseq_bits", [128, 1024])
def test_all_supported_files_in_one_call_equal_the_host_scan(files, scans, subseq_bits):
    """Mixed sizes, samplings and restart intervals in ONE launch, one workgroup per file."""
    names = list(files)
    assert len(names) == 268 + 5
    stats = check_batch(names, files, scans, subseq_bits)
    tiles = dict(zip(names, stats[:, 1]))
    assert tiles["noise_96x136_444_q100"] >= 2 and (subseq_bits != 128 or tiles["frame_360x480_420_q90"] > 1)


@pytest.mark.parametrize("name", NEW)
def test_new_cases_alone_in_a_call(files, scans, name):
    """One frame, one workgroup, several tiles where the stream is long."""
    for subseq_bits in (128, 1024, 4096):
        check_batch([name], files, scans, subseq_bits)


def test_device_route_pixels_equal_pillow_and_the_host_route(files, fx):
    names = list(files)
    dev = hip_ops.decode_jpeg_batch([files[n] for n in names], threads=4, entropy="device")
    host = hip_ops.decode_jpeg_batch([files[n] for n in names], threads=4, entropy="host")
    seen = 0
    for n, a, b in zip(names, dev, host):
        assert torch.equal(a, b), n
        if n in fx[0]:
            assert np.array_equal(a.cpu().numpy(), fx[0][n][1]), n
            seen += 1
    assert seen == 268
    frames = hip_ops.decode_jpeg_batch([files[f"clip_v0_f{k}"] for k in range(5)], entropy="device", subseq_bits=256)
    clip = hip_ops.frames_as_clip(frames)
    assert clip.data_ptr() == frames[0].data_ptr() and np.array_equal(clip.cpu().numpy(), np.stack([fx[0][f"clip_v0_f{k}"][1] for k in range(5)]))
    with pytest.raises(ValueError, match="entropy"):
        hip_ops.decode_jpeg_batch([files["clip_v0_f0"]], entropy="gpu")


def raw_call(batch, subseq_bits=1024, streams=None, segs=None, guard=64, n_coeffs=None, ws_bytes=None, scan_bytes=None, n_segs=None):
    """tt_jpeg_entropy_batch with the coefficients inside a buffer of sentinels and (optionally) doctored HOST tables."""
    lib, n = _lib.load(), len(batch.infos)
    dev = torch.device("cuda", torch.cuda.current_device())
    meta = batch.meta.to(dev)
    buf = torch.full((batch.n_coeffs + 2 * guard,), 0x5A5A, dtype=torch.int16, device=dev)
    status = torch.full((n,), 77, dtype=torch.int32, device=dev)
    streams = np.ascontiguousarray(batch.part("streams") if streams is None else streams)
    segs = np.ascontiguousarray(batch.part("segs") if segs is None else segs)
    need = lib.tt_jpeg_entropy_batch_workspace_bytes(batch.part("streams").ctypes.data, n, 1024)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    at = lambda name: meta.data_ptr() + batch.layout[name][0]
    rc = lib.tt_jpeg_entropy_batch(at("scan"), batch.layout["scan"][1] if scan_bytes is None else scan_bytes, segs.ctypes.data, at("segs"),
                                   batch.n_segs if n_segs is None else n_segs, streams.ctypes.data, at("streams"), n, subseq_bits,
                                   buf.data_ptr() + 2 * guard, batch.n_coeffs if n_coeffs is None else n_coeffs, status.data_ptr(), ws.data_ptr(),
                                   need if ws_bytes is None else ws_bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, buf.cpu().numpy(), status.cpu().numpy(), guard


def test_broken_streams_set_their_frames_status_and_touch_nothing_else(files, scans, fx):
    good = ["grid_37x53_420_q75_std", "rst1_40x56_422_q90", "frame_360x480_420_q90"]
    data = fx[0]["clip_v0_f0"][0]
    with pytest.raises(ValueError, match="file 1: malformed JPEG"):   # test_hip_jpeg's truncated file: cut inside its tables, the host half says so
        hip_ops.decode_jpeg_batch([data, data[:len(data) // 2]], entropy="device")
    start = H.scan_start(data)
    broken = [(data[:start + (len(data) - start) * 3 // 5], -2)] + [(flipped(files, n, at, bit), rc) for n, at, bit, rc in FLIPS]
    for bad, want in broken:
        with pytest.raises(ValueError):                               # what the host route says to the same bytes
            hip_ops.decode_jpeg_batch([files[good[0]], bad], entropy="host")
        with pytest.raises(ValueError, match="file 1: malformed JPEG"):
            hip_ops.decode_jpeg_batch([files[good[0]], bad, files[good[1]]], entropy="device")
    # all of them in one batch between good frames: every status by itself, the good frames' coefficients as the host's
    order = [good[0], 0, 1, good[1], 2, 3, good[2]]
    batch = hip_ops.jpeg_prepare_batch([files[k] if isinstance(k, str) else broken[k][0] for k in order], threads=2)
    for subseq_bits in (128, 1024):
        rc, buf, status, guard = raw_call(batch, subseq_bits)
        assert rc == 0
        assert (buf[:guard] == 0x5A5A).all() and (buf[-guard:] == 0x5A5A).all()
        rows = H.stream_rows(batch)
        for i, k in enumerate(order):
            if isinstance(k, str):
                assert status[i] == 0, k
                assert np.array_equal(buf[guard + rows[i, 9]:guard + rows[i, 9] + scans[k][0].n_coeffs], scans[k][1]), k
            else:
                assert status[i] == broken[k][1], (k, status[i])
        host = hip_ops.jpeg_entropy_host(batch, subseq_bits)
        assert np.array_equal(host[1], status)                        # the emulation: the same status, frame by frame
        for i, k in enumerate(order):                                 # ... and the same bits in the good frames (a failed frame's are unspecified)
            if isinstance(k, str):
                assert np.array_equal(host[0][rows[i, 9]:rows[i, 9] + scans[k][0].n_coeffs], scans[k][1]), k


def test_table_validation_refuses_without_launching(files):
    """The host copies of the stream table and the segment table are checked against every buffer size before the memset and the launch:
    TT_EINVAL, and coefficients and status keep their bytes."""
    lib = _lib.load()
    names = ["clip_v0_f0", "rst7_40x56_422_q90"]
    batch = hip_ops.jpeg_prepare_batch([files[n] for n in names], threads=1)
    good = batch.part("streams").view(np.int64).reshape(2, 16).copy()
    good_segs = batch.part("segs").view(np.uint32).reshape(-1, 2).copy()
    scan_bytes = batch.layout["scan"][1]

    def table(col, value, frame=1):
        t = good.copy()
        t[frame, col] = value
        return {"streams": t.view(np.uint8).reshape(-1)}

    def segment(row, col, value):
        s = good_segs.copy()
        s[row, col] = value
        return {"segs": s.view(np.uint8).reshape(-1)}

    last = int(good[1, 7] + good[1, 8] - 1)
    cases = [table(4, scan_bytes), table(4, int(good[1, 4]) + 2), table(4, -4), table(5, scan_bytes), table(5, int(good[1, 5]) - 4),   # the stream
             table(6, scan_bytes - 1000), table(6, 2), table(6, -4),                                                                   # the tables
             table(7, batch.n_segs), table(8, int(good[1, 8]) + 1), table(8, int(good[1, 8]) - 1), table(7, -1, frame=0),              # segment rows
             segment(last, 0, int(good[1, 5])), segment(last, 0, 2), segment(last, 1, 8 * int(good[1, 5])), segment(0, 1, 0x80000000),
             table(9, batch.n_coeffs), table(10, -8), table(11, int(good[1, 11]) + 64), table(9, 4),                                   # coefficients
             table(0, 0), table(1, 70000), table(2, 3), table(3, -1), table(3, 1 << 20),                                               # not a frame
             {"n_coeffs": batch.n_coeffs - 8}, {"ws_bytes": 16}, {"scan_bytes": int(good[1, 4] + good[1, 5]) - 4}, {"n_segs": last},
             {"subseq_bits": 100}, {"subseq_bits": 8192}, {"subseq_bits": 1000}]
    for kw in cases:
        rc, buf, status, _ = raw_call(batch, **kw)
        assert rc == -1, kw
        assert "jpeg_entropy" in lib.tt_last_error().decode()
        assert (buf == 0x5A5A).all() and (status == 77).all(), kw
    rc, buf, status, guard = raw_call(batch)
    assert rc == 0 and status.tolist() == [0, 0]
    assert np.array_equal(buf[guard:-guard], np.concatenate([hip_ops.jpeg_scan(files[n])[1] for n in names]))


def test_entropy_launch_neither_allocates_nor_breaks_capture(files, scans):
    lib = _lib.load()
    names = ["frame_360x480_420_q90", "rst7_40x56_422_q90", "noise_96x136_420_q100_opt"]
    batch = hip_ops.jpeg_prepare_batch([files[n] for n in names], threads=1)
    want = np.concatenate([scans[n][1] for n in names])
    dev = torch.device("cuda", torch.cuda.current_device())
    n = len(names)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        meta = batch.meta.to(dev)
        coeffs = torch.full((batch.n_coeffs,), 7, dtype=torch.int16, device=dev)
        status = torch.full((n,), 7, dtype=torch.int32, device=dev)
        streams, segs = batch.part("streams"), batch.part("segs")
        ws = torch.zeros(lib.tt_jpeg_entropy_batch_workspace_bytes(streams.ctypes.data, n, 1024), dtype=torch.uint8, device=dev)
        at = lambda name: meta.data_ptr() + batch.layout[name][0]

        def launch():
            rc = lib.tt_jpeg_entropy_batch(at("scan"), batch.layout["scan"][1], segs.ctypes.data, at("segs"), batch.n_segs, streams.ctypes.data,
                                           at("streams"), n, 1024, coeffs.data_ptr(), batch.n_coeffs, status.data_ptr(), ws.data_ptr(), ws.numel(),
                                           torch.cuda.current_stream().cuda_stream)
            assert rc == 0

        launch()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(3):
            coeffs.fill_(7)
            launch()
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0, "a launch changed the device's free memory"
        assert np.array_equal(coeffs.cpu().numpy(), want) and status.tolist() == [0] * n
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch()
        for _ in range(2):
            coeffs.fill_(7)
            status.fill_(7)
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(coeffs.cpu().numpy(), want) and status.tolist() == [0] * n


def test_clip_loader_with_device_entropy_equals_the_host_route(fx, tmp_path):
    pytest.importorskip("PIL.Image")
    from timetuning_amd import video_transformations as VT
    from timetuning_amd.data_loader import ClipLoader, SamplingMode, VideoDataset, make_loader

    prog = fx[0]["prog_48x64_420_q90"][0]
    root = J._write_tree(tmp_path / "set", fx, swap={(0, 2): prog})
    out = {}
    for entropy in ("host", "device"):
        ds = VideoDataset(str(root / "JPEGImages"), str(root / "Annotations"), SamplingMode.Full, 1, 5, video_transform=VT.evaluation_transforms(32))
        loader = ClipLoader(ds, 2, shuffle=False, seed=7, jpeg_entropy=entropy)
        assert loader.jpeg_entropy == entropy and ds.jpeg_entropy == "host"      # the loader's choice: a dataset two loaders share keeps its own
        out[entropy] = (list(loader), loader.fallback_frames)
    assert out["host"][1] == out["device"][1] == 1                   # the progressive file: Pillow, counted, on either route
    assert len(out["host"][0]) == len(out["device"][0]) == 1
    for a, b in zip(out["host"][0], out["device"][0]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    made = make_loader(str(root), 5, 2, sampling_mode=SamplingMode.Full, video_transform=VT.evaluation_transforms(32), jpeg_entropy="device")
    assert made.dataset.jpeg_entropy == "device" and made.jpeg_entropy == "device" and torch.equal(next(iter(made))[0], out["host"][0][0][0])
    with pytest.raises(ValueError, match="jpeg_entropy"):
        ClipLoader(ds, 2, jpeg_entropy="gpu")
    # a supported file with a broken stream is an error on the device route too, not a fallback
    good = fx[0]["clip_v1_f3"][0]
    root = J._write_tree(tmp_path / "broken", fx, swap={(1, 3): good[:len(good) * 2 // 3]})
    ds = VideoDataset(str(root / "JPEGImages"), str(root / "Annotations"), SamplingMode.Full, 1, 5, video_transform=VT.evaluation_transforms(32),
                      jpeg_entropy="device")
    with pytest.raises(ValueError, match="malformed JPEG"):
        next(iter(ClipLoader(ds, 2)))
    assert ds.fallback_frames == 0
