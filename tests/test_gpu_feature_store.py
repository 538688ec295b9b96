"""-m gpu: utterances' features kept on the device as Kaldi's CompressedMatrix codes and decoded where they are read (tdnnf_feature_store_*,
tdnnf_chunk_input_gather_stored; include/tdnnf_hip.h, "FEATURE STORES").  The specification is numpy: tests/feature_store_ref.py gives the
value of every code (the bits of the library's own reader: tests/test_feature_store_ref.py), tests/chunk_input_ref.py the gather.  Every
output is byte for byte that statement, at the shapes of tests/test_gpu_chunk_input.py -- fsf 3, chunks of 4 output frames, a window of 21
frames from -5, utterances of 13, 30 and 12 frames so that windows overhang both edges -- in formats 1, 2 and 3, with feat_dim 8 (form 4: a
lane decodes 4 columns), feat_dim 5 (form 1) and feat_dim 8 into an output view 4 bytes off a 16-byte boundary (form 1).  The codes and
headers are drawn directly, every format's edge codes planted in every utterance; the store is filled by two appends.  Then the expand,
the float appends, stream order, no allocation, device_bytes against the header's closed form, and the refusals."""
import functools

import numpy as np
import pytest
import torch

from tests import chunk_input_ref as chunks
from tests import feature_store_ref as ref
from tests.gpu_util import dev, host

pytestmark = pytest.mark.gpu

FSF, T, FIRST_T, NUM_T = 3, 4, -5, 21
SHAPE = (FIRST_T, NUM_T, FSF)
FRAMES, IV_ROWS, IV_DIM = (13, 30, 12), (1, 2, 3), 4  # O = 5, 10, 4
BATCHES = {3: ([0, 1, 2], [0, 6, 0]), 1: ([1], [3])}
LAYOUTS = [(8, "plain", 4), (5, "plain", 1), (8, "view", 1)]


@pytest.fixture(scope="module")
def abi(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pkg.hipabi


@functools.lru_cache(maxsize=None)
def fixture(fmt, feat_dim, iv_dim=IV_DIM):
    """(items, utts): the store's payloads and the same utterances decoded by the statement, with float i-vectors; computed once"""
    items = ref.random_items(100 * fmt + feat_dim, fmt, feat_dim, FRAMES)
    rng = np.random.default_rng(7)
    utts = [(ref.decode(it), rng.standard_normal((r, iv_dim)).astype(np.float32) if iv_dim else None) for it, r in zip(items, IV_ROWS)]
    for f, _ in utts:
        f.setflags(write=False)
    return items, utts


def filled(abi, fmt, feat_dim):
    """a store of the fixture's utterances: two appends, utterances 0-1 then 2"""
    items, _ = fixture(fmt, feat_dim)
    store = abi.FeatureStore(fmt, feat_dim, 3, sum(FRAMES))
    store.append(items[:2])
    store.append(items[2:])
    assert store.frames == list(FRAMES)
    return store


def output(rows, cols, layout):
    """a zeroed output on the device: contiguous, or a view of a wider buffer whose base is 4 bytes off a 16-byte boundary"""
    if layout != "view":
        return torch.zeros(rows, cols, dtype=torch.float32, device="cuda")
    view = torch.zeros(rows, cols + 4, dtype=torch.float32, device="cuda")[:, 1:1 + cols]
    assert view.data_ptr() % 16 == 4 and view.stride(0) % 4 == 0
    return view


def same_bytes(got, want, what):
    got = host(got)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.int32), np.ascontiguousarray(want).view(np.int32)), what


@pytest.mark.parametrize("feat_dim,layout,form", LAYOUTS)
@pytest.mark.parametrize("fmt", [1, 2, 3])
@pytest.mark.parametrize("B", [3, 1])
def test_gather_stored_is_the_gather_of_the_decoded_utterances(abi, fmt, feat_dim, layout, form, B):
    _, utts = fixture(fmt, feat_dim)
    store = filled(abi, fmt, feat_dim)
    seq_utt, begins = BATCHES[B]
    h = abi.ChunkInput(3)
    expanded = store.expand([0, 1, 2])
    calls = 0
    for period in (10, 0):
        _, iv, frames, rows = chunks.stacked(utts, period)
        iv_dev = dev(iv)
        for shift in range(-2, 3):
            want_f, want_iv = chunks.gather(FIRST_T, NUM_T, FSF, T, seq_utt, begins, utts, period, shift)
            out = (output(NUM_T * B, feat_dim, layout), torch.zeros(B, IV_DIM, device="cuda"))
            got_f, got_iv = h.gather_stored(SHAPE, T, seq_utt, begins, store, rows if period > 0 else None, iv_dev, period, frame_shift=shift, out=out)
            calls += 1
            info = store.info()
            assert (info["gathers"], info["last_form"], info["allocations"], info["expands"]) == (calls, form, 0, 1), info
            same_bytes(got_f, want_f, (period, shift))
            same_bytes(got_iv, want_iv, (period, shift))
            # ... and it is the float gather on the expand's output
            flt_f, flt_iv = h.gather(SHAPE, T, seq_utt, begins, frames, expanded, rows if period > 0 else None, iv_dev, period, frame_shift=shift)
            same_bytes(flt_f, want_f, ("float", period, shift))
            same_bytes(flt_iv, want_iv, ("float", period, shift))
    assert h.info()["gathers"] == calls  # the handle counts its float gathers alone


@pytest.mark.parametrize("feat_dim,form", [(8, 4), (5, 1)])
@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_without_ivectors_nothing_of_them_is_read_or_written(abi, fmt, feat_dim, form):
    _, utts = fixture(fmt, feat_dim)
    bare = [(f, None) for f, _ in utts]
    store = filled(abi, fmt, feat_dim)
    seq_utt, begins = BATCHES[3]
    h = abi.ChunkInput(3)
    want_f, want_iv = chunks.gather(FIRST_T, NUM_T, FSF, T, seq_utt, begins, bare, 10, 1)
    got_f, got_iv = h.gather_stored(SHAPE, T, seq_utt, begins, store, None, None, 10, frame_shift=1)
    assert got_iv is None and want_iv is None and store.info()["last_form"] == form
    same_bytes(got_f, want_f, feat_dim)
    # i-vectors that do not allow 16 bytes take the features to form 1 with them
    _, odd = fixture(fmt, feat_dim, 3)
    _, iv, frames, rows = chunks.stacked(odd, 10)
    want_f, want_iv = chunks.gather(FIRST_T, NUM_T, FSF, T, seq_utt, begins, odd, 10, 0)
    got_f, got_iv = h.gather_stored(SHAPE, T, seq_utt, begins, store, rows, dev(iv), 10)
    assert store.info()["last_form"] == 1
    same_bytes(got_f, want_f, "odd")
    same_bytes(got_iv, want_iv, "odd")


@pytest.mark.parametrize("feat_dim,layout,form", LAYOUTS)
@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_expand_is_the_stacked_decodes(abi, fmt, feat_dim, layout, form):
    _, utts = fixture(fmt, feat_dim)
    store = filled(abi, fmt, feat_dim)
    # repeats and any order; a list of one; a list longer than the store
    for k, utt in enumerate(([2, 0, 2], [1], [2, 0, 2, 1, 1])):
        want = np.concatenate([utts[u][0] for u in utt])
        out = output(len(want), feat_dim, layout)
        assert store.expand(utt, out=out) is out
        same_bytes(out, want, utt)
        info = store.info()
        assert (info["expands"], info["last_form"], info["allocations"], info["gathers"]) == (k + 1, form, 0, 0), info
    same_bytes(store.expand([0, 1, 2]), np.concatenate([f for f, _ in utts]), "new tensor")
    # the views AcousticModel.compute takes: one expand
    pairs = store.utterances([2, 0], [utts[2][1], utts[0][1]])
    assert store.info()["expands"] == 5 and [tuple(f.shape) for f, _ in pairs] == [(12, feat_dim), (13, feat_dim)]
    same_bytes(pairs[0][0], utts[2][0], "view 2")
    same_bytes(pairs[1][0], utts[0][0], "view 0")
    assert pairs[0][1] is utts[2][1] and pairs[0][0].data_ptr() + 4 * 12 * feat_dim == pairs[1][0].data_ptr()


@pytest.mark.parametrize("fmt,feat_dim,form", [(1, 8, 4), (2, 5, 1)])
def test_expand_of_a_long_list_takes_pieces(abi, fmt, feat_dim, form):
    """a list is staged 1024 entries a turn of the store's ring (8 KB pinned a buffer, whatever max_utterances): 2500 entries take three
    pieces, the third in the first's buffer; utterances of 1 and 2 frames, so a piece's rows begin anywhere"""
    rng = np.random.default_rng(fmt)
    items = [ref.random_item(rng, fmt, rows, feat_dim) for rows in (1, 2)]
    decoded = [ref.decode(it) for it in items]
    store = abi.FeatureStore(fmt, feat_dim, 2, 3)
    store.append(items)
    utt = rng.integers(0, 2, size=2500)
    assert len(set(utt[1020:1030])) == 2
    same_bytes(store.expand(utt), np.concatenate([decoded[u] for u in utt]), "pieces")
    info = store.info()
    assert (info["expands"], info["last_form"], info["allocations"]) == (1, form, 0)


@pytest.mark.parametrize("feat_dim", [8, 5])
@pytest.mark.parametrize("fmt", [2, 3])
def test_append_float_then_expand_is_the_compression_decoded(abi, fmt, feat_dim):
    rng = np.random.default_rng(fmt)
    ms = [rng.standard_normal((f, feat_dim)).astype(np.float32) * 3 for f in FRAMES]
    ms[1][:] = 0.25  # a constant matrix: max = min + 1
    store = abi.FeatureStore(fmt, feat_dim, 3, sum(FRAMES))
    store.append_float(ms[:1])
    store.append_float([torch.from_numpy(m) for m in ms[1:]])
    assert store.frames == list(FRAMES)
    want = np.concatenate([ref.decode(ref.compress(m, fmt)) for m in ms])
    same_bytes(store.expand([0, 1, 2]), want, fmt)
    # and it is a compression of the matrices: a code is the truncation of (x - min) / step + 0.499, so at most 0.501 steps off, and float32
    # rounding of values below 16 adds a few 1e-6
    step = max(float(m.max() - m.min()) for m in ms) / (65535 if fmt == 2 else 255)
    assert np.abs(want - np.concatenate(ms)).max() <= 0.501 * step + 1e-5
    one = abi.FeatureStore(1, feat_dim, 3, sum(FRAMES))
    with pytest.raises(abi.HipAbiError, match="feature_store_append_float: format 1 .CM. from float matrices is not built: Kaldi's percentile selection"):
        one.append_float(ms[:1])
    assert one.info()["utterances"] == 0 and one.frames == []


def test_stream_order(abi):
    """two gathers with different tables into different outputs, a third into the first's output, a copy of the first's output and an expand
    enqueued in between; nothing waits until the end.  Three turns: the third takes the first's staging buffer."""
    _, utts = fixture(1, 8)
    store = filled(abi, 1, 8)
    _, iv, frames, rows = chunks.stacked(utts, 10)
    iv_dev = dev(iv)
    h = abi.ChunkInput(3)
    tables = [([0, 1, 2], [0, 6, 0], 0), ([1, 1, 0], [2, 5, 1], 2), ([2, 0, 1], [0, 1, 0], -1)]
    new = lambda: (torch.zeros(NUM_T * 3, 8, device="cuda"), torch.zeros(3, IV_DIM, device="cuda"))
    out_a, out_b = new(), new()
    torch.cuda.synchronize()
    gather = lambda k, out: h.gather_stored(SHAPE, T, tables[k][0], tables[k][1], store, rows, iv_dev, 10, frame_shift=tables[k][2], out=out)
    gather(0, out_a)
    kept = (out_a[0].clone(), out_a[1].clone())  # (a copy on the same stream: no wait)
    gather(1, out_b)
    expanded = store.expand([1, 0])
    gather(2, out_a)
    torch.cuda.synchronize()
    for k, got in ((0, kept), (1, out_b), (2, out_a)):
        want = chunks.gather(FIRST_T, NUM_T, FSF, T, tables[k][0], tables[k][1], utts, 10, tables[k][2])
        same_bytes(got[0], want[0], k)
        same_bytes(got[1], want[1], k)
    same_bytes(expanded, np.concatenate([utts[1][0], utts[0][0]]), "expand")
    assert store.info()["gathers"] == 3 and h.info()["gathers"] == 0


@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_no_call_allocates_and_device_bytes_is_the_closed_form(abi, fmt):
    items, utts = fixture(fmt, 8)
    store = abi.FeatureStore(fmt, 8, 3, sum(FRAMES))
    closed = lambda n: ref.layout(fmt, 8, FRAMES[:n])[1]
    assert store.info()["device_bytes"] == 0 == closed(0)
    store.append(items[:2])
    assert store.info()["device_bytes"] == closed(2) == abi.FeatureStore.layout(fmt, 8, FRAMES[:2])[1]
    store.append(items[2:])
    width = 2 if fmt == 2 else 1
    by_hand = sum((f * 8 * width + 15) // 16 * 16 for f in FRAMES) + 3 * (32 + (16 * 8 if fmt == 1 else 0))
    info = store.info()
    assert info["device_bytes"] == closed(3) == by_hand and info["reserved_bytes"] >= by_hand
    assert (info["format"], info["feat_dim"], info["utterances"], info["frames"]) == (fmt, 8, 3, sum(FRAMES))
    assert by_hand - 3 * (32 + (16 * 8 if fmt == 1 else 0)) <= sum(FRAMES) * 8 * width + 3 * 15  # the codes: a quarter or a half of float32, and padding
    _, iv, frames, rows = chunks.stacked(utts, 10)
    iv_dev = dev(iv)
    h = abi.ChunkInput(3)
    out = (torch.zeros(NUM_T * 3, 8, device="cuda"), torch.zeros(3, IV_DIM, device="cuda"))
    whole = torch.zeros(sum(FRAMES), 8, device="cuda")
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    for i in range(20):
        h.gather_stored(SHAPE, T, *BATCHES[3], store, rows, iv_dev, 10, frame_shift=i % 3, out=out)
        store.expand(np.roll([0, 1, 2], i % 3), out=whole)
    info = store.info()
    assert (info["allocations"], info["gathers"], info["expands"], info["last_form"], info["device_bytes"]) == (0, 20, 20, 4, by_hand)
    assert torch.cuda.mem_get_info()[0] == free  # the device agrees: nothing was allocated or freed
    same_bytes(out[0], chunks.gather(FIRST_T, NUM_T, FSF, T, *BATCHES[3], utts, 10, 19 % 3)[0], "last gather")
    same_bytes(whole, np.concatenate([utts[u][0] for u in (2, 0, 1)]), "last expand")


@pytest.mark.parametrize("fmt", [1, 2])
def test_refusals_leave_the_store_and_its_utterances_readable(abi, fmt):
    items, utts = fixture(fmt, 8)
    store = abi.FeatureStore(fmt, 8, 3, sum(FRAMES))
    store.append(items[:2])
    info = store.info()
    both = np.concatenate([utts[0][0], utts[1][0]])
    other = ref.random_item(np.random.default_rng(0), 3 if fmt == 1 else 1, 12, 8)

    def refused(words, call, *args, **kw):
        with pytest.raises(abi.HipAbiError) as e:
            call(*args, **kw)
        assert "tdnnf error 1:" in str(e.value) and words in str(e.value), str(e.value)  # TDNNF_EINVAL
        assert store.info() == info and store.frames == list(FRAMES[:2])
        same_bytes(store.expand([0, 1]), both, words)
        info.update(expands=info["expands"] + 1, last_form=4)

    last = items[2]
    refused("feature_store_append: 4 utterances exceed the capacity max_utterances = 3 by 1", store.append, [last, last])
    refused("feature_store_append: 56 frames exceed the capacity max_frames = 55 by 1", store.append, [ref.random_item(np.random.default_rng(1), fmt, 13, 8)])
    refused("feature_store_append: item 0 has 5 columns, feat_dim is 8", store.append, [ref.random_item(np.random.default_rng(1), fmt, 12, 5)])
    refused("feature_store_append: item 1 has 0 rows", store.append, [last, dict(last, rows=0, codes=np.zeros((0, 8), last["codes"].dtype))])
    refused("feature_store_append: item 0: its min or range is not finite", store.append, [dict(last, range=np.float32("nan"))])
    refused("feature_store_append: item 0: its min or range is not finite", store.append, [dict(last, min=np.float32("-inf"))])
    refused("feature_store_append: item 0 is a payload of format %d, the store holds format %d" % (other["format"], fmt), store.append, [other])
    if fmt == 2:
        refused("feature_store_append_float: 56 frames exceed the capacity max_frames = 55 by 1", store.append_float, [np.zeros((13, 8), np.float32)])
        refused("feature_store_append_float: item 0 has 0 rows", store.append_float, [np.zeros((0, 8), np.float32)])
        refused("feature_store_append_float: item 0: its min or range is not finite", store.append_float, [np.full((2, 8), np.inf, np.float32)])
    # the expand and the gather: a refusal leaves outputs and counters
    refused("feature_store_expand: entry 1: utterance 2 outside [0, 2)", store.expand, [0, 2])
    refused("feature_store_expand: out must be 43 x 8 (the listed utterances stacked), not 42 x 8", store.expand, [0, 1], out=torch.zeros(42, 8, device="cuda"))
    h = abi.ChunkInput(2)
    _, iv, frames, rows = chunks.stacked(utts[:2], 10)
    iv_dev = dev(iv)
    out = h.gather_stored(SHAPE, T, [0, 1], [0, 6], store, rows, iv_dev, 10)
    info = store.info()
    want = chunks.gather(FIRST_T, NUM_T, FSF, T, [0, 1], [0, 6], utts, 10, 0)

    def no_gather(words, seq_utt=(0, 1), begins=(0, 6), rows=rows, shift=0, into=out):
        refused("chunk_input_gather_stored: " + words, h.gather_stored, SHAPE, T, list(seq_utt), list(begins), store, rows, iv_dev, 10, frame_shift=shift, out=into)
        same_bytes(out[0], want[0], words)
        same_bytes(out[1], want[1], words)

    no_gather("sequence 1: the chunk begins at frame -1", begins=(0, -1))
    no_gather("sequence 1: the chunk of 4 frames from frame 7 ends behind the 10 output frames of the utterance", begins=(0, 7))
    no_gather("sequence 1: utterance 2 outside [0, 2)", seq_utt=(0, 2))
    no_gather("frame_shift 3: its magnitude must be below frame_subsampling 3", shift=3)
    no_gather("utterance 1 has no i-vector rows (0)", rows=[1, 0])
    no_gather("ivectors must be 4 x 4", rows=[2, 2])
    no_gather("3 sequences exceed the capacity max_sequences = 2 by 1", seq_utt=(0, 1, 0), begins=(0, 6, 0))
    no_gather("feats_out must be 42 x 8 (num_t x sequences rows), not 43 x 8", into=(torch.zeros(43, 8, device="cuda"), out[1]))
    # ... and the store goes on: the third utterance, then a gather from it
    store.append(items[2:])
    same_bytes(store.expand([2, 0, 1]), np.concatenate([utts[2][0], both]), "after")
    _, iv, frames, rows = chunks.stacked(utts, 10)
    got = abi.ChunkInput(3).gather_stored(SHAPE, T, *BATCHES[3], store, rows, dev(iv), 10, frame_shift=2)
    same_bytes(got[0], chunks.gather(FIRST_T, NUM_T, FSF, T, *BATCHES[3], utts, 10, 2)[0], "after")
