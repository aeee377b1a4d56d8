"""N24 without a GPU: tt_jpeg_prepare and tt_jpeg_entropy_host - the emulation of the device entropy decode, lane by lane through the header
the kernel compiles (csrc/jpeg_huff.hpp) - against tt_jpeg_scan of the same bytes.  Every comparison is for equality of int16
coefficients; the files are those of tests/golden/jpeg_frames.npz and tests/golden/jpeg_entropy.npz (tools/gen_jpeg_entropy_golden.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from timetuning_amd import _lib, hip_ops

HERE = os.path.dirname(os.path.abspath(__file__))
FRAMES, ENTROPY = os.path.join(HERE, "golden", "jpeg_frames.npz"), os.path.join(HERE, "golden", "jpeg_entropy.npz")
EARGUMENT, ERESTART = -6, -5


def load_files(path):
    g = np.load(path)
    return {str(n): g["blob"][g["offs"][i]:g["offs"][i + 1]].tobytes() for i, n in enumerate(g["names"])}


def supported_files():
    """{name: bytes} of every file of both fixtures the decoder takes: 268 of jpeg_frames.npz and the five of jpeg_entropy.npz."""
    frames = {n: d for n, d in load_files(FRAMES).items() if hip_ops.jpeg_probe(d).supported}
    extra = load_files(ENTROPY)
    assert len(frames) == 268 and len(extra) == 5 and all(hip_ops.jpeg_probe(d).supported for d in extra.values())
    return {**frames, **extra}


@pytest.fixture(scope="module")
def files():
    return supported_files()


@pytest.fixture(scope="module")
def scans(files):
    """The yardstick, computed once: {name: (info, coefficients, quantisation tables)} of hip_ops.jpeg_scan."""
    return {n: hip_ops.jpeg_scan(d) for n, d in files.items()}


def stream_rows(batch):
    return batch.part("streams").view(np.int64).reshape(-1, 16)


@pytest.mark.parametrize("subseq_bits", [128, 1024, 4096])
def test_every_supported_file_equals_the_host_scan(files, scans, subseq_bits):
    names = list(files)
    batch = hip_ops.jpeg_prepare_batch([files[n] for n in names], threads=2, pin=False)
    coeffs, status, stats = hip_ops.jpeg_entropy_host(batch, subseq_bits)
    rows, q = stream_rows(batch), batch.part("qtables").view(np.uint16).reshape(-1, 3, 64)
    covered = 0
    for i, n in enumerate(names):
        info, want, want_q = scans[n]
        assert status[i] == 0 and stats[i, 3] == -1, n
        assert np.array_equal(coeffs[rows[i, 9]:rows[i, 9] + info.n_coeffs], want), n
        assert np.array_equal(q[i], want_q), n
        covered += 1
    assert covered == 268 + 5
    tiles, subs = dict(zip(names, stats[:, 1])), dict(zip(names, stats[:, 2]))
    if subseq_bits == 128:
        assert tiles["frame_360x480_420_q90"] > 1
    if subseq_bits == 1024:
        assert subs["noise_96x136_444_q100"] > 256 and tiles["noise_96x136_444_q100"] == 2
        assert 13 * 17 * 6 / subs["flat_200x264_420_q30"] > 150      # hundreds of blocks in one subsequence: 13 x 17 MCUs of 6
        assert subs["rst1_40x56_422_q90"] == 4 * 5                   # a segment per MCU
    if subseq_bits == 4096:
        grid = [n for n in names if n.startswith("grid_") and not n.endswith("_rst")]
        assert sum(subs[n] == 1 for n in grid) > len(grid) // 2


def test_both_builders_produce_the_same_tables(files):
    """jpeg_scan_batch and jpeg_prepare_batch describe one batch alike: the frame table and the quantisation tables byte for byte, the
    output layout, and the stream rows' coefficient offsets - what tt_jpeg_prepare wrote, moved to the file's place - equal to the frame
    rows'.  Every sampling at a ragged size, a 1 x 1 file, restart intervals, and a group of two frames."""
    names = list(load_files(ENTROPY)) + ["clip_v0_f0", "clip_v0_f1"] + [f"grid_9x15_{s}_q75_std" for s in ("444", "422", "420")] + ["grid_1x1_420_q75_std"]
    data, n = [files[k] for k in names], len(names)
    host, dev = hip_ops.jpeg_scan_batch(data, threads=2, pin=False), hip_ops.jpeg_prepare_batch(data, threads=2, pin=False)
    assert (host.route, dev.route) == ("host", "device") and host.n_segs == 0 and dev.coeffs is None and host.coeffs.numel() == host.n_coeffs
    assert host.part("frames").size == n * 128 and host.part("qtables").size == n * 3 * 64 * 2 and host.meta.numel() == n * (128 + 384)
    for part in ("frames", "qtables"):
        assert np.array_equal(host.part(part), dev.part(part)), part
    assert host.groups == dev.groups and host.where == dev.where
    assert host.out_bytes == dev.out_bytes and host.n_coeffs == dev.n_coeffs == sum(hip_ops.jpeg_probe(d).n_coeffs for d in data)
    clip = hip_ops.jpeg_probe(files["clip_v0_f0"])
    assert host.groups[(clip.H, clip.W)][1] >= 2 and host.where[6][1] == host.where[5][1] + 1
    frames = host.part("frames").view(np.int64).reshape(n, 16)
    assert np.array_equal(stream_rows(dev)[:, 9:12], frames[:, 3:6])
    assert frames[:, 3].tolist() == np.cumsum([0] + [hip_ops.jpeg_probe(d).n_coeffs for d in data])[:-1].tolist()


# ---- tt_jpeg_prepare
def scan_start(data):
    """Offset of the first entropy-coded byte: behind the SOS segment."""
    pos = 2
    while True:
        assert data[pos] == 0xFF
        marker, length = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        pos += 2 + length
        if marker == 0xDA:
            return pos


def clean_segments(data, n_segments):
    """The restatement: the scan's bytes with FF 00 -> FF, fill bytes dropped, cut at the restart markers; the last segment ends at the
    first marker."""
    d = np.frombuffer(data, np.uint8)
    pos, segs, cur = scan_start(data), [], []
    while pos < len(d):
        if d[pos] != 0xFF:
            cur.append(d[pos])
            pos += 1
        elif d[pos + 1] == 0x00:
            cur.append(0xFF)
            pos += 2
        elif d[pos + 1] == 0xFF:
            pos += 1
        else:
            segs.append(bytes(cur))
            cur = []
            if len(segs) == n_segments:
                break
            assert 0xD0 <= d[pos + 1] <= 0xD7
            pos += 2
    return segs


def prepare_raw(data, scan_cap=None, seg_cap=None):
    lib = _lib.load()
    a, b = C.c_size_t(), C.c_size_t()
    assert lib.tt_jpeg_prepare_bytes(len(data), C.byref(a), C.byref(b)) == 0
    scan_cap, seg_cap = a.value if scan_cap is None else scan_cap, b.value if seg_cap is None else seg_cap
    scan, segs = np.full(scan_cap + 8, 0xA5, np.uint8), np.full((seg_cap + 1, 2), 0xA5A5A5A5, np.uint32)
    row, q = np.zeros(16, np.int64), np.zeros((3, 64), np.uint16)
    rc = lib.tt_jpeg_prepare(data, len(data), scan.ctypes.data, scan_cap, segs.ctypes.data, seg_cap, row.ctypes.data, q.ctypes.data)
    assert (scan[scan_cap:] == 0xA5).all() and (segs[seg_cap:] == 0xA5A5A5A5).all()      # nothing behind the capacities
    return rc, scan, segs, row


def with_fill_bytes(data):
    """Two fill bytes in front of every restart marker of the scan."""
    out, start = bytearray(data[:scan_start(data)]), scan_start(data)
    for i in range(start, len(data)):
        if data[i] == 0xFF and i + 1 < len(data) and 0xD0 <= data[i + 1] <= 0xD7:
            out += b"\xff\xff"
        out.append(data[i])
    return bytes(out)


@pytest.mark.parametrize("name", ["noise_96x136_444_q100", "rst7_40x56_422_q90", "rst1_40x56_422_q90", "grid_37x53_420_q100_rst"])
def test_prepare_writes_the_clean_stream_in_aligned_segments(files, scans, name):
    plain = files[name]
    data = with_fill_bytes(plain)
    assert (len(data) > len(plain)) == ("rst" in name)
    if name.startswith("noise"):
        assert data[scan_start(data):].count(b"\xff\x00") > 100
    rc, scan, segs, row = prepare_raw(data)
    assert rc == 0
    n = int(row[8])
    want = clean_segments(data, n)
    assert len(want) == n and (n > 1) == ("rst" in name)
    assert row[6] == 0 and row[4] == 6 * 272 and row[7] == 0
    stream = scan[row[4]:row[4] + row[5]]
    at = 0
    for k, seg in enumerate(want):
        start, bits = int(segs[k, 0]), int(segs[k, 1])
        assert start % 4 == 0 and start == at and bits == 8 * len(seg)
        assert stream[start:start + len(seg)].tobytes() == seg
        at = -(-(start + len(seg)) // 4) * 4
        assert not stream[start + len(seg):at].any()
    assert at == row[5]
    # the fill bytes change nothing downstream
    batch = hip_ops.jpeg_prepare_batch([data], threads=1, pin=False)
    coeffs, status, _ = hip_ops.jpeg_entropy_host(batch, 256)
    assert status[0] == 0 and np.array_equal(coeffs, scans[name][1])


def test_prepare_refuses_a_capacity_too_small_and_keeps_unsupported_codes(files):
    data = files["rst7_40x56_422_q90"]
    rc, scan, segs, row = prepare_raw(data)
    assert rc == 0
    used, n = int(row[4] + row[5]), int(row[8])
    assert prepare_raw(data, scan_cap=used)[0] == 0 and prepare_raw(data, seg_cap=n)[0] == 0
    assert prepare_raw(data, scan_cap=used - 1)[0] == EARGUMENT
    assert prepare_raw(data, scan_cap=6 * 272 - 1)[0] == EARGUMENT
    assert prepare_raw(data, seg_cap=n - 1)[0] == EARGUMENT
    other = load_files(FRAMES)
    for name in ("prog_48x64_420_q90", "gray_16x16_q75", "cmyk_16x16_q75"):
        want = hip_ops.jpeg_probe(other[name]).status
        assert want > 0 and prepare_raw(other[name])[0] == want
        with pytest.raises(hip_ops.JpegUnsupported):
            hip_ops.jpeg_prepare_batch([data, other[name]], pin=False)


@pytest.mark.parametrize("name", ["rst7_40x56_422_q90", "rst1_40x56_422_q90", "grid_17x33_444_q75_rst"])
def test_prepare_checks_the_restart_numbering(files, name):
    data = files[name]
    start = scan_start(data)
    markers = [i for i in range(start, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    assert len(markers) >= 2
    for i in (markers[0], markers[len(markers) // 2], markers[-1]):
        assert prepare_raw(data[:i] + data[i + 2:])[0] == ERESTART                                        # missing
        assert prepare_raw(data[:i + 1] + bytes([0xD0 + (data[i + 1] + 2) % 8]) + data[i + 2:])[0] == ERESTART   # misnumbered
        with pytest.raises(ValueError, match="file 1: malformed JPEG"):
            hip_ops.jpeg_prepare_batch([data, data[:i] + data[i + 2:]], pin=False)


# ---- broken streams: the emulation is as strict as the sequential decoder, and equal to it wherever that succeeds
def host_outcome(data):
    """(tt_jpeg_scan's status, its coefficients where that is 0)."""
    lib, info = _lib.load(), hip_ops._jpeg_probe_raw(_lib.load(), data)
    if info.status != 0:
        return info.status, None
    coeffs, q = np.empty(info.n_coeffs, np.int16), np.empty((3, 64), np.uint16)
    rc = lib.tt_jpeg_scan(data, len(data), coeffs.ctypes.data, coeffs.size, q.ctypes.data)
    return rc, coeffs if rc == 0 else None


def route_outcome(data, subseq_bits):
    """(status, coefficients, who said it): tt_jpeg_prepare's status where it refuses, else the frame status of the emulation."""
    rc = prepare_raw(data)[0]
    if rc != 0:
        return rc, None, "prepare"
    coeffs, status, _ = hip_ops.jpeg_entropy_host(hip_ops.jpeg_prepare_batch([data], threads=1, pin=False), subseq_bits)
    return int(status[0]), coeffs, "decode"


BROKEN = ["noise_96x136_420_q100_opt", "rst1_40x56_422_q90", "rst7_40x56_422_q90", "grid_37x53_420_q95_rst", "clip_v0_f0", "flat_200x264_420_q30",
          "grid_17x33_422_q75_opt"]


@pytest.mark.parametrize("name", BROKEN)
def test_truncated_and_bit_flipped_scans_agree_with_the_host_scan(files, name):
    data = files[name]
    start = scan_start(data)
    rng = np.random.default_rng(2400 + BROKEN.index(name))
    variants = [data[:start + (len(data) - start) * k // 24] for k in range(24)] + [data[:len(data) - k] for k in (1, 2, 3)]
    for _ in range(160):
        at, bit = int(rng.integers(start, len(data) - 2)), int(rng.integers(0, 8))
        variants.append(data[:at] + bytes([data[at] ^ (1 << bit)]) + data[at + 1:])
    seen = {0: 0, -1: 0, 1: 0}
    for k, bad in enumerate(variants):
        rc, want = host_outcome(bad)
        got_rc, got, who = route_outcome(bad, (256, 1024, 128)[k % 3])
        seen[(rc > 0) - (rc < 0)] += 1
        assert (got_rc > 0) - (got_rc < 0) == (rc > 0) - (rc < 0), (name, k, rc, got_rc)
        if who == "decode":            # the decode reports the sequential decoder's own code; prepare's refusals (markers) only share its sign
            assert got_rc == rc, (name, k, rc, got_rc)
        if rc == 0:
            assert np.array_equal(got, want), (name, k)
    assert seen[0] > 0 and seen[-1] > 20 and seen[1] == 0, seen


def test_subseq_bits_outside_the_range_are_refused(files):
    lib = _lib.load()
    batch = hip_ops.jpeg_prepare_batch([files["clip_v0_f0"]], threads=1, pin=False)
    streams, segs, scan = batch.part("streams"), batch.part("segs"), batch.part("scan")
    coeffs, status, ws = np.full(batch.n_coeffs, 77, np.int16), np.full(1, 77, np.int32), np.zeros(64, np.int32)

    def call(bits, n_coeffs=batch.n_coeffs, ws_bytes=ws.nbytes):
        return lib.tt_jpeg_entropy_host(scan.ctypes.data, scan.size, segs.ctypes.data, segs.ctypes.data, batch.n_segs, streams.ctypes.data,
                                        streams.ctypes.data, 1, bits, coeffs.ctypes.data, n_coeffs, status.ctypes.data, ws.ctypes.data, ws_bytes, None)

    for bits in (100, 8192, 96, 4128, 1000, 0, -1024):
        assert call(bits) == -1 and lib.tt_jpeg_entropy_batch_workspace_bytes(streams.ctypes.data, 1, bits) == 0
        with pytest.raises(ValueError, match="subseq_bits"):
            hip_ops.jpeg_entropy_host(batch, bits)
    assert call(1024, n_coeffs=batch.n_coeffs - 8) == -1 and call(1024, ws_bytes=8) == -1
    assert (coeffs == 77).all() and status[0] == 77                  # a refused call writes nothing
    assert lib.tt_jpeg_entropy_batch_workspace_bytes(streams.ctypes.data, 1, 128) >= 16
    assert call(128) == 0 and status[0] == 0 and np.array_equal(coeffs, hip_ops.jpeg_scan(files["clip_v0_f0"])[1])
