"""The label-map kernels (N23, csrc/label_map.hip) on the GPU: presence bits against ``torch.unique``, the instance -> category remap
against the transcription of the reference's in-place loop (tests/_ytvos_ref.py), ``data_loader.compose_instance_lut`` and the clips
recorded from the reference itself (tests/golden/ytvos_meta.npz)."""
import json

import numpy as np
import pytest
import torch

import _ytvos_ref as R
from timetuning_amd import _lib, data_loader as DL, hip_ops as ops

pytestmark = pytest.mark.gpu

SEGMENTS = (1, 3, 5)
LENGTHS = (1, 15, 16, 17, 63, 64, 65, 4099)
LONG = 33001            # more than one workgroup per segment at uint8 (a workgroup walks 16 KB), odd
TT_EINVAL = -1


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def values_of(words_row):
    return ops.presence_values(words_row.cpu().numpy().view(np.uint32))


def at_offset(a: np.ndarray, offset: int, guard: int = 0, fill: int = 0xA5):
    """A GPU copy of ``a`` (uint8 [S, P]) whose first byte lies ``offset`` bytes past a 16-byte boundary, inside a ``fill``-ed buffer with at
    least ``guard`` bytes either side -> (view, buffer, first byte's index)."""
    lead = 16 * ((guard + 15) // 16) + offset
    buf = torch.full((lead + a.size + guard + 16,), fill, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[lead:lead + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == offset and view.is_contiguous()
    return view, buf, lead


@pytest.fixture(scope="module")
def labels():
    """uint8 [S, P] maps in runs for every (S, P) of the grid, made once and left unchanged."""
    return {(S, P): R.segment_labels(S, P, seed=100 * S + P) for S in SEGMENTS for P in LENGTHS + (LONG,)}


# ---- presence ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
@pytest.mark.parametrize("P", LENGTHS + (LONG,))
@pytest.mark.parametrize("S", SEGMENTS)
def test_presence_equals_unique(labels, S, P, dtype):
    t = dev(labels[S, P]).to(dtype)
    words, status = ops.label_presence(t)
    assert words.dtype == torch.int32 and tuple(words.shape) == (S, 8) and status.tolist() == [0] * S
    for s in range(S):
        assert values_of(words[s]) == torch.unique(t[s]).tolist(), (S, P, s)
    assert ops.label_value_counts(t) == [torch.unique(t[s]).shape[0] for s in range(S)]


@pytest.mark.parametrize("offset", [1, 7, 15])
@pytest.mark.parametrize("P", [17, 65, 4099, LONG])
def test_presence_of_an_unaligned_tensor(labels, P, offset):
    a = labels[3, P]
    view, _, _ = at_offset(a, offset)
    words, _ = ops.label_presence(view)
    for s in range(3):
        assert values_of(words[s]) == np.unique(a[s]).tolist(), (P, offset, s)
    wide = torch.empty((3 * P + 1,), dtype=torch.int64, device="cuda")[1:].view(3, P)    # int64 starting 8 bytes past a 16-byte boundary
    wide.copy_(torch.from_numpy(a.astype(np.int64)))
    assert wide.data_ptr() % 16 == 8
    for s in range(3):
        assert values_of(ops.label_presence(wide)[0][s]) == np.unique(a[s]).tolist(), (P, "int64", s)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
def test_presence_of_constant_and_extreme_maps(dtype):
    P = 4099
    t = torch.zeros((4, P), dtype=dtype, device="cuda")
    t[0] = 7                                    # all equal
    t[1] = 255
    t[2, ::2] = 255                             # 0 and 255
    t[3, P - 1] = 255                           # one label in the tail
    words, status = ops.label_presence(t)
    assert [values_of(words[s]) for s in range(4)] == [[7], [255], [0, 255], [0, 255]] and status.tolist() == [0] * 4
    assert ops.label_value_counts(t) == [1, 1, 2, 2]


def test_presence_flags_int64_values_outside_a_byte():
    P = 4099
    t = torch.zeros((4, P), dtype=torch.int64, device="cuda")
    t[:, 5:9] = 3
    t[1, 2000] = 300
    t[2, P - 1] = -1                            # in the tail
    t[3, 0] = 256
    words, status = ops.label_presence(t)
    assert status.tolist() == [0, 1, 1, 1]
    assert all(values_of(words[s]) == [0, 3] for s in range(4))          # a value outside 0 .. 255 sets no bit
    assert ops.label_value_counts(t) == [2, 3, 3, 3]                     # ... and that row is counted by torch.unique


# ---- map_instances ----------------------------------------------------------------------------------------------------------------------

def check_remap(a, cat, sequential, in_offset=0, out_offset=0):
    S, P = a.shape
    src, _, _ = at_offset(a, in_offset)
    out, buf, lead = at_offset(np.zeros_like(a), out_offset, guard=32)
    out.fill_(0x5A)                              # sentinel: no label, no category
    mapped, lut, status = ops.map_instances(src, dev(cat), sequential, out=out)
    assert mapped.data_ptr() == out.data_ptr() and status.tolist() == [0] * S
    host = buf.cpu().numpy()
    assert (host[:lead] == 0xA5).all() and (host[lead + S * P:] == 0xA5).all()             # the guards either side
    got, lut = host[lead:lead + S * P].reshape(S, P), lut.cpu().numpy()
    assert np.array_equal(src.cpu().numpy(), a)                                               # the input is read only
    for s in range(S):
        assert np.array_equal(got[s], R.map_instances_ref(a[s], cat[s], sequential)), (S, P, s, sequential)
        assert np.array_equal(lut[s], DL.compose_instance_lut(np.unique(a[s]), cat[s], sequential)), (S, P, s, sequential)
    return got


@pytest.mark.parametrize("sequential", [True, False])
@pytest.mark.parametrize("P", LENGTHS + (LONG,))
@pytest.mark.parametrize("S", SEGMENTS)
def test_remap_equals_the_in_place_loop(labels, S, P, sequential):
    cat = R.segment_tables(S, seed=7)
    assert S == 1 or not np.array_equal(cat[0], cat[1])                  # each segment has a table of its own
    check_remap(labels[S, P], cat, sequential)


@pytest.mark.parametrize("in_offset,out_offset", [(1, 0), (0, 3), (5, 5), (15, 8)])
@pytest.mark.parametrize("P", [17, 4099, LONG])
def test_remap_of_unaligned_tensors(labels, P, in_offset, out_offset):
    check_remap(labels[3, P], R.segment_tables(3, seed=8), True, in_offset, out_offset)


def test_sequential_and_plain_differ_where_the_reference_chains(labels):
    a, cat = labels[5, 4099], R.segment_tables(5, seed=7)
    assert not np.array_equal(check_remap(a, cat, True), check_remap(a, cat, False))


def test_remap_equals_the_reference_on_the_golden_clips(golden):
    g = golden("ytvos_meta")
    meta = json.loads(str(g["meta_json"]))
    cd = DL.make_categories_dict(meta, "ytvos")
    videos = [str(v) for v in g["videos"]]
    clips = np.stack([g[f"clip_{i}"].reshape(-1) for i in range(len(videos))])
    want = np.stack([g[f"mapped_{i}"].reshape(-1) for i in range(len(videos))])
    cat = np.stack([DL.video_category_table(meta, cd, v) for v in videos])
    mapped, _, status = ops.map_instances(dev(clips), dev(cat), True)
    assert torch.equal(mapped.cpu(), torch.from_numpy(want)) and status.tolist() == [0] * len(videos)
    plain = ops.map_instances(dev(clips), dev(cat), False)[0].cpu().numpy()
    assert np.array_equal(plain, np.stack([R.map_instances_plain(c, t) for c, t in zip(clips, cat)])) and not np.array_equal(plain, want)


@pytest.mark.parametrize("sequential", [True, False])
def test_object_without_a_category_is_reported_and_copied(labels, sequential):
    a, cat = labels[3, 4099].copy(), R.segment_tables(3, seed=9)
    a[1, 100:104] = 77                          # ids 41 .. 254 have no category
    a[1, 4098] = 50
    a[2, 7] = 255
    cat[2, 255] = 256                           # a category that does not fit a byte counts as none
    mapped, lut, status = ops.map_instances(dev(a), dev(cat), sequential)
    assert status.tolist() == [0, 50, 255]      # the smallest such id
    got, lut = mapped.cpu().numpy(), lut.cpu().numpy()
    assert np.array_equal(got[0], R.map_instances_ref(a[0], cat[0], sequential))
    for s in (1, 2):
        assert np.array_equal(got[s], a[s]) and np.array_equal(lut[s], np.arange(256))
        with pytest.raises(KeyError) as e:
            DL.compose_instance_lut(np.unique(a[s]), cat[s], sequential)
        assert e.value.args[0] == status[s].item()


def test_two_calls_are_bit_equal(labels):
    a, cat = dev(labels[5, LONG]), dev(R.segment_tables(5, seed=7))
    first, second = ops.map_instances(a, cat, True), ops.map_instances(a, cat, True)
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    assert torch.equal(ops.label_presence(a)[0], ops.label_presence(a)[0])


def test_refusals_launch_nothing(labels):
    lib = _lib.load()
    S, P = 3, 65
    a, cat = dev(labels[S, P]), dev(R.segment_tables(S, seed=7))
    buf = torch.full((2 * S * P,), 0x5A, dtype=torch.uint8, device="cuda")
    lut = torch.full((S, 256), 0x5A, dtype=torch.uint8, device="cuda")
    status = torch.full((S,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ws = torch.full((S * 32,), 0x5A, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def remap(src=a.data_ptr(), dst=buf.data_ptr(), table=cat.data_ptr(), S=S, P=P, sequential=1, lut_p=lut.data_ptr(), st=status.data_ptr(),
              ws_p=ws.data_ptr(), ws_bytes=S * 32):
        return lib.tt_map_instances(src, dst, table, S, P, sequential, lut_p, st, ws_p, ws_bytes, stream)

    inside = buf.data_ptr() + S * P             # src = buf: every dst below overlaps it
    calls = [remap(src=None), remap(dst=None), remap(table=None), remap(lut_p=None), remap(st=None), remap(ws_p=None), remap(S=0), remap(P=0),
             remap(sequential=3), remap(ws_bytes=S * 32 - 1), remap(src=buf.data_ptr(), dst=buf.data_ptr()),
             remap(src=buf.data_ptr(), dst=inside - 1), remap(src=inside - 1, dst=buf.data_ptr()), remap(table=cat.data_ptr() + 1)]
    assert calls == [TT_EINVAL] * len(calls)
    words = torch.full((S, 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    pres = [lib.tt_label_presence_segments(None, 1, S, P, words.data_ptr(), status.data_ptr(), stream),
            lib.tt_label_presence_segments(a.data_ptr(), 1, S, P, None, status.data_ptr(), stream),
            lib.tt_label_presence_segments(a.data_ptr(), 1, S, P, words.data_ptr(), None, stream),
            lib.tt_label_presence_segments(a.data_ptr(), 4, S, P, words.data_ptr(), status.data_ptr(), stream),
            lib.tt_label_presence_segments(a.data_ptr(), 1, 0, P, words.data_ptr(), status.data_ptr(), stream),
            lib.tt_label_presence_segments(a.data_ptr(), 1, S, 0, words.data_ptr(), status.data_ptr(), stream),
            lib.tt_label_presence_segments(a.data_ptr() + 4, 8, 1, 8, words.data_ptr(), status.data_ptr(), stream)]
    assert pres == [TT_EINVAL] * len(pres)
    torch.cuda.synchronize()
    for t in (buf, lut, ws):
        assert (t == 0x5A).all()                # nothing was written
    assert (status == 0x5A5A5A5A).all() and (words == 0x5A5A5A5A).all()
    with pytest.raises(TypeError):
        ops.map_instances(a.long(), cat)
    with pytest.raises(ValueError):
        ops.map_instances(a, cat[:2])
    with pytest.raises(TypeError):
        ops.label_presence(a.to(torch.int16))
    assert remap(dst=buf.data_ptr()) == 0       # the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert status.tolist() == [0] * S
