"""-m gpu: the net's input for minibatches of chunks, gathered on the device from whole utterances (tdnnf_chunk_input_*; include/tdnnf_hip.h,
"CHUNK INPUTS").  The specification is tests/chunk_input_ref.py, the definition in numpy: feats_out and ivectors_out are byte for byte its
arrays at the smallest shapes that can go wrong -- fsf 3, chunks of 4 output frames, a net window of 21 frames from -5, utterances of 13, 30
and 12 frames so that windows overhang both edges and one utterance is exactly one chunk long -- in the 16-byte and in the scalar form,
at every frame shift, in both period modes and without i-vectors.  Then stream order, no allocation, the refusals, and the archive route:
the chunks write_chunk_egs writes, read back by egs.minibatches at three frame shifts, are the gathered bytes."""
import numpy as np
import pytest
import torch

from tests import alignment_supervision_ref as ali
from tests import chunk_input_ref as ref
from tests.gpu_util import dev, host

pytestmark = pytest.mark.gpu

FSF, T, FIRST_T, NUM_T = 3, 4, -5, 21
FRAMES, IV_ROWS, IV_DIM = (13, 30, 12), (1, 2, 3), 4  # O = 5, 10, 4
# B = 3: the start of the short utterance (the window overhangs both its edges), the end of the long one, the utterance of exactly one chunk
BATCHES = {3: ([0, 1, 2], [0, 6, 0]), 1: ([1], [3])}


@pytest.fixture(scope="module")
def abi(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pkg.hipabi


def utterances(feat_dim, iv_dim=IV_DIM, seed=0):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((f, feat_dim)).astype(np.float32), rng.standard_normal((r, iv_dim)).astype(np.float32) if iv_dim else None)
            for f, r in zip(FRAMES, IV_ROWS)]


def placed(a, layout):
    """the stacked features on the device: contiguous, or a view of a wider buffer whose base is 4 bytes off a 16-byte boundary"""
    if layout != "view":
        return dev(a)
    buf = torch.full((a.shape[0], a.shape[1] + 4), 7.0, dtype=torch.float32, device="cuda")
    buf[:, 1:1 + a.shape[1]] = dev(a)
    view = buf[:, 1:1 + a.shape[1]]
    assert view.data_ptr() % 16 == 4 and view.stride(0) % 4 == 0
    return view


def same_bytes(got, want, what):
    got = host(got)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32)), what


@pytest.mark.parametrize("feat_dim,layout,form", [(8, "plain", 4), (5, "plain", 1), (8, "view", 1)])
@pytest.mark.parametrize("B", [3, 1])
def test_outputs_are_the_numpy_statements_bytes(abi, feat_dim, layout, form, B):
    utts = utterances(feat_dim)
    seq_utt, begins = BATCHES[B]
    h = abi.ChunkInput(3)
    calls = 0
    for period in (10, 0):
        f, iv, frames, rows = ref.stacked(utts, period)
        f_dev, iv_dev = placed(f, layout), dev(iv)
        for shift in range(-2, 3):
            want_f, want_iv = ref.gather(FIRST_T, NUM_T, FSF, T, seq_utt, begins, utts, period, shift)
            got_f, got_iv = h.gather((FIRST_T, NUM_T, FSF), T, seq_utt, begins, frames, f_dev, rows if period > 0 else None, iv_dev, period, frame_shift=shift)
            calls += 1
            assert h.info() == dict(max_sequences=3, allocations=0, gathers=calls, last_form=form)
            same_bytes(got_f, want_f, (period, shift))
            same_bytes(got_iv, want_iv, (period, shift))
        if B == 3:  # the statement's own edges: both overhangs are there, and the two modes pick different rows
            want_f = ref.gather(FIRST_T, NUM_T, FSF, T, seq_utt, begins, utts, period, 0)[0]
            assert np.array_equal(want_f[0], utts[0][0][0]) and np.array_equal(want_f[(NUM_T - 1) * 3], utts[0][0][-1])
            assert np.array_equal(want_f[(NUM_T - 1) * 3 + 1], utts[1][0][-1]) and np.array_equal(want_f[2], utts[2][0][0])
    if B == 3:  # (the long utterance's chunk takes its second i-vector row with a period, its first without)
        by_period = [ref.gather(FIRST_T, NUM_T, FSF, T, seq_utt, begins, utts, period, 0)[1] for period in (10, 0)]
        assert np.array_equal(by_period[0][1], utts[1][1][1]) and np.array_equal(by_period[1][1], utts[1][1][0])


@pytest.mark.parametrize("feat_dim,form", [(8, 4), (5, 1)])
def test_without_ivectors_nothing_of_them_is_read_or_written(abi, feat_dim, form):
    utts = utterances(feat_dim, iv_dim=0)
    seq_utt, begins = BATCHES[3]
    f, iv, frames, rows = ref.stacked(utts, 10)
    assert iv is None and rows is None
    h = abi.ChunkInput(3)
    want_f, want_iv = ref.gather(FIRST_T, NUM_T, FSF, T, seq_utt, begins, utts, 10, 1)
    got_f, got_iv = h.gather((FIRST_T, NUM_T, FSF), T, seq_utt, begins, frames, dev(f), None, None, 10, frame_shift=1)
    assert got_iv is None and want_iv is None and h.info()["last_form"] == form
    same_bytes(got_f, want_f, feat_dim)
    # a matrix of no columns is no i-vector either; i-vectors that do not allow 16 bytes take the features to the scalar form with them
    empty = torch.zeros(3, 0, dtype=torch.float32, device="cuda")
    got_f, got_iv = h.gather((FIRST_T, NUM_T, FSF), T, seq_utt, begins, frames, dev(f), None, empty, 10, frame_shift=1)
    assert got_iv is None
    same_bytes(got_f, want_f, feat_dim)
    odd = utterances(feat_dim, iv_dim=3)
    f, iv, frames, rows = ref.stacked(odd, 10)
    want_f, want_iv = ref.gather(FIRST_T, NUM_T, FSF, T, seq_utt, begins, odd, 10, 0)
    got_f, got_iv = h.gather((FIRST_T, NUM_T, FSF), T, seq_utt, begins, frames, dev(f), rows, dev(iv), 10)
    assert h.info()["last_form"] == 1
    same_bytes(got_f, want_f, "odd")
    same_bytes(got_iv, want_iv, "odd")


def test_stream_order(abi):
    """two gathers with different tables into different outputs, a third into the first's output, a copy of the first's output enqueued in
    between; nothing waits until the end.  Three turns: the third takes the first's staging buffer."""
    utts = utterances(8)
    f, iv, frames, rows = ref.stacked(utts, 10)
    f_dev, iv_dev = dev(f), dev(iv)
    h = abi.ChunkInput(3)
    tables = [([0, 1, 2], [0, 6, 0], 0), ([1, 1, 0], [2, 5, 1], 2), ([2, 0, 1], [0, 1, 0], -1)]
    new = lambda: (torch.zeros(NUM_T * 3, 8, device="cuda"), torch.zeros(3, IV_DIM, device="cuda"))
    out_a, out_b = new(), new()
    torch.cuda.synchronize()
    gather = lambda k, out: h.gather((FIRST_T, NUM_T, FSF), T, tables[k][0], tables[k][1], frames, f_dev, rows, iv_dev, 10, frame_shift=tables[k][2], out=out)
    gather(0, out_a)
    kept = (out_a[0].clone(), out_a[1].clone())  # (a copy on the same stream: no wait)
    gather(1, out_b)
    gather(2, out_a)
    torch.cuda.synchronize()
    for k, got in ((0, kept), (1, out_b), (2, out_a)):
        want = ref.gather(FIRST_T, NUM_T, FSF, T, tables[k][0], tables[k][1], utts, 10, tables[k][2])
        same_bytes(got[0], want[0], k)
        same_bytes(got[1], want[1], k)
    assert h.info()["gathers"] == 3


def test_no_gather_allocates(abi):
    utts = utterances(8)
    f, iv, frames, rows = ref.stacked(utts, 10)
    f_dev, iv_dev = dev(f), dev(iv)
    h = abi.ChunkInput(3)
    out = (torch.zeros(NUM_T * 3, 8, device="cuda"), torch.zeros(3, IV_DIM, device="cuda"))
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    for i in range(20):
        h.gather((FIRST_T, NUM_T, FSF), T, *BATCHES[3], frames, f_dev, rows, iv_dev, 10, frame_shift=i % 3, out=out)
    assert h.info() == dict(max_sequences=3, allocations=0, gathers=20, last_form=4)
    assert torch.cuda.mem_get_info()[0] == free  # the device agrees: nothing was allocated or freed
    want = ref.gather(FIRST_T, NUM_T, FSF, T, *BATCHES[3], utts, 10, 19 % 3)
    same_bytes(out[0], want[0], "last")


def test_a_refused_gather_leaves_outputs_and_counters(abi):
    utts = utterances(8)
    f, iv, frames, rows = ref.stacked(utts, 10)
    f_dev, iv_dev = dev(f), dev(iv)
    seq_utt, begins = BATCHES[3]
    h = abi.ChunkInput(3)
    out = h.gather((FIRST_T, NUM_T, FSF), T, seq_utt, begins, frames, f_dev, rows, iv_dev, 10)
    want = ref.gather(FIRST_T, NUM_T, FSF, T, seq_utt, begins, utts, 10, 0)
    info = h.info()
    at = lambda a, i, v: list(a[:i]) + [v] + list(a[i + 1:])

    def refused(words, seq_utt=seq_utt, begins=begins, frames=frames, feats=f_dev, rows=rows, ivectors=iv_dev, shift=0, out=out):
        with pytest.raises(abi.HipAbiError) as e:
            h.gather((FIRST_T, NUM_T, FSF), T, seq_utt, begins, frames, feats, rows, ivectors, 10, frame_shift=shift, out=out)
        assert "tdnnf error 1:" in str(e.value) and "chunk_input_gather: " + words in str(e.value), str(e.value)  # TDNNF_EINVAL
        assert h.info() == info
        same_bytes(out[0], want[0], words)
        same_bytes(out[1], want[1], words)

    refused("sequence 1: the chunk begins at frame -1", begins=at(begins, 1, -1))
    refused("sequence 1: the chunk of 4 frames from frame 7 ends behind the 10 output frames of the utterance", begins=at(begins, 1, 7))
    refused("sequence 2: utterance 3 outside [0, 3)", seq_utt=at(seq_utt, 2, 3))
    refused("sequence 0: utterance -1 outside [0, 3)", seq_utt=at(seq_utt, 0, -1))
    refused("utterance 1 has 0 frames", frames=at(frames, 1, 0))
    refused("frame_shift 3: its magnitude must be below frame_subsampling 3", shift=3)
    refused("frame_shift -3: its magnitude must be below frame_subsampling 3", shift=-3)
    refused("utterance 2 has no i-vector rows (0)", rows=at(rows, 2, 0))
    refused("feats must be 56 x 8 (the utterances stacked), not 55 x 8", frames=at(frames, 1, 31))
    refused("ivectors must be 7 x 4", rows=at(rows, 0, 2))
    refused("4 sequences exceed the capacity max_sequences = 3 by 1", seq_utt=seq_utt + [0], begins=begins + [0])
    # outputs of another shape: the real ones stay as they are
    for wrong, words in (((torch.zeros(NUM_T * 3 + 1, 8, device="cuda"), out[1]), "feats_out must be 63 x 8"),
                         ((torch.zeros(NUM_T * 3, 4, device="cuda"), out[1]), "feats_out must be 63 x 8"),
                         ((out[0], torch.zeros(2, IV_DIM, device="cuda")), "ivectors_out must be 3 x 4")):
        with pytest.raises(abi.HipAbiError) as e:
            h.gather((FIRST_T, NUM_T, FSF), T, seq_utt, begins, frames, f_dev, rows, iv_dev, 10, out=wrong)
        assert "tdnnf error 1:" in str(e.value) and "chunk_input_gather: " + words in str(e.value), str(e.value)
        assert h.info() == info and not any(host(t).any() for t in wrong if t is not out[0] and t is not out[1])
    same_bytes(out[0], want[0], "shapes")
    same_bytes(out[1], want[1], "shapes")
    # ... and the handle goes on
    h.gather((FIRST_T, NUM_T, FSF), T, seq_utt, begins, frames, f_dev, rows, iv_dev, 10, frame_shift=2, out=out)
    same_bytes(out[0], ref.gather(FIRST_T, NUM_T, FSF, T, seq_utt, begins, utts, 10, 2)[0], "after")
    assert h.info()["gathers"] == info["gathers"] + 1


def tiny_net(pkg):
    """the net of tests/test_gpu_egs.py: chunks of 24 input frames (8 output frames), 4 sequences"""
    cfg = pkg.trainer.make_config(frames_per_chunk=24, num_sequences=4, strides=[1, 0, 3], bottleneck=16, feat_dim=40, ivector_dim=100, num_pdfs=60,
                                  hidden_dim=64, small_dim=32)
    return pkg.trainer.ChainNet(cfg)


def aligned_utterances(seed=0):
    """four utterances of 3 + 1 + 2 + 2 = 8 chunks of 8 output frames, an i-vector every 10 frames, and random alignments"""
    rng = np.random.default_rng(seed)
    frames = (70, 24, 41, 48)
    utts = [(rng.standard_normal((f, 40)).astype(np.float32), rng.standard_normal(((f + 9) // 10, 100)).astype(np.float32)) for f in frames]
    return utts, [ali.random_alignment(rng, (f + 2) // 3) for f in frames]


def test_the_archive_route_reads_back_the_gathered_bytes(pkg, abi, tmp_path):
    E = pkg.egs
    net = tiny_net(pkg)
    utts, als = aligned_utterances()
    us = ali.unit_set(pkg.synth, 1)
    out_frames = [(len(f) + 2) // 3 for f, _ in utts]
    batches = E.chunk_minibatches(E.utterance_chunks(out_frames, 8), 4, seed=2)
    chunks = [c for m in batches for c in m]
    assert len(chunks) == 8 and (net.cfg.frame_subsampling, net.cfg.frames_per_chunk) == (3, 24)
    path = tmp_path / "chunks.ark"
    assert E.write_chunk_egs(path, utts, als, net, us, 2, chunks) == 8
    f, iv, frames, rows = ref.stacked(utts, 10)
    f_dev, iv_dev = dev(f), dev(iv)
    h = abi.ChunkInput(4)
    for shift in (0, 1, 2):
        got = list(E.minibatches(path, net, frame_shift=shift))
        assert len(got) == 2
        for m, (f_arch, iv_arch, _) in zip(batches, got):
            utt, begins = [u for u, _ in m], [o for _, o in m]
            f_gath, iv_gath = h.gather(net, 8, utt, begins, frames, f_dev, rows, iv_dev, 10, frame_shift=shift)
            same_bytes(f_gath, host(f_arch), shift)
            same_bytes(iv_gath, host(iv_arch), shift)
            same_bytes(f_gath, ref.gather(net.first_t, net.num_t_in, 3, 8, utt, begins, utts, 10, shift)[0], shift)
    assert h.info()["last_form"] == 4
    # the supervisions of the archive are the host lattice's arrays, by value
    egs = list(E.Reader(path))
    for k, m in enumerate(batches):
        _, _, sup = E.merge(egs[4 * k:4 * k + 4], net.first_t, net.num_t_in, 0)
        want = pkg.synth.supervision_lattice_from_alignment_chunks(us, [als[u] for u, _ in m], [out_frames[u] for u, _ in m], [o for _, o in m], 8, 2)
        assert (sup["B"], sup["T"], sup["weight"]) == (4, 8, 1.0)
        for key in ("seq_state_begin", "seq_arc_begin", "state_time", "final_logprob", "arc_src", "arc_dst", "arc_pdf", "arc_logprob"):
            assert np.array_equal(sup[key], want[key]), key
    net.close()
