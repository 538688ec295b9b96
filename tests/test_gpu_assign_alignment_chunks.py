"""-m gpu: supervisions of chunks compiled on the device from whole-utterance alignments and a frame tolerance
(tdnnf_supervision_assign_alignment_chunks, tdnnf_alignment_chunk_supervision_sizes; include/tdnnf_hip.h "ALIGNMENT CHUNKS").  The
specification is tests/alignment_chunk_ref.py, the utterance's lattice cut by the definition (tests/test_alignment_chunk_ref.py holds it to
its properties): a reserved supervision assigned chunks has BYTE FOR BYTE the 17 device tables of a second reserved supervision given
assign(the statement's dict), the same info(), and tdnnf_chain_objf_and_deriv / tdnnf_chain_objf give the same BITS from the two -- the
same build kernels run on equal raw arrays.  The chunk of a whole utterance has the bytes of assign_alignments.  Then the closed loop
(assign_transcripts, best_path_labels, infer.alignment_from_path, infer.chunk_begins, assign_alignment_chunks with tolerance 0: every
chunk is the best path's frames), the refusals (each leaves the previous minibatch byte for byte), the three assigns alternating on one
handle with no allocation, and stream order."""
import numpy as np
import pytest
import torch

from tests import alignment_chunk_ref as chk
from tests import alignment_supervision_ref as ali
from tests.gpu_util import Hip, dev, host
from tests.test_gpu_assign_alignments import same_tables
from tests.test_gpu_supervision_assign import P as DEN_P
from tests.test_gpu_supervision_assign import capacity, enqueue, inputs, run, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abi(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pkg.hipabi


@pytest.fixture(scope="module")
def hip(pkg):
    return Hip(pkg)


@pytest.fixture(scope="module")
def den(pkg):
    return pkg.hipabi.DenGraph(pkg.synth.make_den_graph(30, DEN_P, mean_out_degree=4.0, seed=5))


@pytest.fixture(scope="module")
def sets(pkg, abi):
    """per context: the unit set dict and its device form"""
    out = []
    for context in (0, 1):
        us = ali.unit_set(pkg.synth, context)
        out.append((us, abi.UnitSet(us["entry_pdf"], us["loop_pdf"], us["loop_logprob"], us["leave_logprob"], us["P"], us["take_logprob"], us["skip_logprob"])))
    return out


def args(chunks):
    """(alignments, utt_frames, chunk_begins) as the Python methods take them"""
    return [c[0] for c in chunks], [c[1] for c in chunks], [c[2] for c in chunks]


def roomy(cap, states_per_sequence=8):
    """The capacity with some states more.  Short chunks stage more than the reserve makes room for at exactly their states and arcs -- 12
    bytes a staged unit and 16 a sequence against 8 a state and 16 an arc -- so the handles of the small minibatches get 8 states a
    sequence (64 bytes of staging) on top; the arcs stay exact."""
    return (cap[0], cap[1], cap[2] + states_per_sequence * cap[0], cap[3])


@pytest.mark.parametrize("context", [0, 1])
@pytest.mark.parametrize("utt_frames", chk.UTT_FRAMES)
def test_tables_and_info_are_those_of_an_assign_of_the_cut_lattice(abi, sets, context, utt_frames):
    us, units = sets[context]
    frames = [T for T in chk.CHUNK_FRAMES if T <= utt_frames]
    assert frames == ([1, 2] if utt_frames == 2 else [1, 2, 7])
    cases = [(chk.small_batch(utt_frames, T), T, tol) for T in frames for tol in chk.tolerances(utt_frames)]
    sups = [chk.lattice(us, chunks, T, tol) for chunks, T, tol in cases]
    cap = roomy(capacity(sups))
    compiled, assigned = abi.Supervision.reserve(*cap), abi.Supervision.reserve(*cap)
    for (chunks, T, tol), s in zip(cases, sups):
        assert {c[2] for c in chunks} == {0, 1, (utt_frames - T) // 2, utt_frames - T} & set(range(utt_frames - T + 1))
        assert [len(c[0][0]) for c in chunks[::len(chunks) // 3]][:2] == [1, utt_frames]  # a one-unit utterance, one of one-frame units
        states, arcs = units.alignment_chunk_sizes(*args(chunks), T, tol)
        assert states.tolist() == np.diff(s["seq_state_begin"]).tolist() and arcs.tolist() == np.diff(s["seq_arc_begin"]).tolist()
        compiled.assign_alignment_chunks(units, *args(chunks), T, tol)
        assigned.assign(s)
        assert compiled.info() == assigned.info() and (compiled.B, compiled.T) == (len(chunks), T), (T, tol)
        assert compiled.info()["num_states"] == len(s["state_time"]) and compiled.info()["num_arcs"] == len(s["arc_src"])
        same_tables(compiled.tables(), assigned.tables(), (context, utt_frames, T, tol))
    assert compiled.capacity()["allocations"] == 0 and compiled.capacity()["assigns"] == len(cases)


@pytest.fixture(scope="module")
def large(pkg):
    """name -> (chunks, T, tolerance, wide)"""
    return {"narrow": chk.narrow_batch() + (False,), "wide": chk.wide_batch() + (True,)}


@pytest.mark.parametrize("context", [0, 1])
@pytest.mark.parametrize("name", ["narrow", "wide"])
def test_tables_of_the_narrow_and_the_wide_minibatch(abi, sets, large, context, name):
    us, units = sets[context]
    chunks, T, tol, wide = large[name]
    s = chk.lattice(us, chunks, T, tol)
    assert ali.is_wide(s) == wide and (len(chunks), T, tol, chunks[0][1]) == ((4, 150, 5, 400) if name == "narrow" else (2, 60, 40, 150))
    cap = capacity([s])  # exactly the largest: nothing may be written beyond it
    compiled, assigned = abi.Supervision.reserve(*cap), abi.Supervision.reserve(*cap)
    compiled.assign_alignment_chunks(units, *args(chunks), T, tol)
    assigned.assign(s)
    assert compiled.info() == assigned.info() and compiled.info()["wide"] == int(wide)
    same_tables(compiled.tables(), assigned.tables(), name)


@pytest.mark.parametrize("context", [0, 1])
def test_the_chunk_of_a_whole_utterance_has_the_bytes_of_assign_alignments(abi, sets, context):
    us, units = sets[context]
    for T in ali.FRAMES:
        alignments = ali.small_batch(T)
        cap = roomy(capacity([ali.lattice(us, alignments, T, tol) for tol in ali.tolerances(T)]))
        ds = abi.Supervision.reserve(*cap)
        for tol in ali.tolerances(T):
            ds.assign_alignments(units, alignments, T, tol)
            want, info = ds.tables(), ds.info()
            ds.assign_alignment_chunks(units, alignments, [T] * 3, [0] * 3, T, tol)
            assert ds.info() == info
            same_tables(ds.tables(), want, (context, T, tol))


@pytest.mark.parametrize("name", ["narrow", "wide"])
def test_objective_and_derivatives_are_the_assigned_lattices_bits(abi, hip, den, sets, large, name):
    us, units = sets[1]
    chunks, T, tol, wide = large[name]
    s = chk.lattice(us, chunks, T, tol, weight=0.75)
    cap = capacity([s])
    compiled, assigned = abi.Supervision.reserve(*cap), abi.Supervision.reserve(*cap)
    compiled.assign_alignment_chunks(units, *args(chunks), T, tol, weight=0.75)
    assigned.assign(s)
    y, xo = inputs(s, 3)
    want, got = run(hip, den, assigned, y, xo), run(hip, den, compiled, y, xo)
    assert want[0][5] == 1.0 and np.isfinite(want[0][:7]).all() and np.abs(want[1]).sum() > 0 and np.abs(want[2]).sum() > 0
    same_bits(want, got)


@pytest.mark.parametrize("context", [0, 1])
def test_the_loop_closes_on_the_best_paths_chunks(pkg, abi, sets, context):
    """align one 40-frame utterance against its transcript, segment, cut into chunks of 8, supervise with tolerance 0: each chunk's single
    path carries the best path's pdfs of its frames"""
    us, units = sets[context]
    Tu, T = 40, 8
    transcripts = pkg.synth.make_transcripts(1, ali.U, slots=(5, 9), optional_rate=0.4, seed=21 + context)
    states, arcs = units.sizes(transcripts)
    graphs = abi.AlignGraphs.reserve(1, ali.P, int(states.sum()), int(arcs.sum()), num_labels=10)
    graphs.assign_transcripts(units, transcripts)
    rng = np.random.default_rng(6)
    y = dev((2.0 * rng.standard_normal((Tu, ali.P))).astype(np.float32))
    pdfs, _, results, labels, _ = graphs.best_path_labels(y, [Tu], [0])
    pdfs, labels, results = host(pdfs), host(labels), host(results)
    assert (results[:, 1] == 1.0).all()
    alignment = pkg.infer.alignment_from_path(labels, transcripts[0])
    assert len(alignment[0]) >= 3  # chunks begin and end inside units
    begins = pkg.infer.chunk_begins(Tu, T) + [13]
    assert begins == [0, 8, 16, 24, 32, 13]
    B = len(begins)
    sup = abi.Supervision.reserve(B, T, B * (T + 1) + 8 * B, B * T)
    sup.assign_alignment_chunks(units, [alignment] * B, [Tu] * B, begins, T, 0)
    t = sup.tables()
    assert np.diff(t["seq_state_begin"]).tolist() == [T + 1] * B and sup.info()["num_arcs"] == B * T
    assert t["state_time"].tolist() == list(range(T + 1)) * B
    # state order is time order: the arc out of the state of time t is frame t's
    assert np.array_equal(t["out_pdf"], np.concatenate([pdfs[o:o + T] for o in begins]))


def test_refusals_leave_the_previous_minibatch(abi, hip, den, sets):
    us, units = sets[1]
    Tu, T = 7, 2
    chunks = chk.small_batch(Tu, T)
    al, frames, first = args(chunks)
    small, big = chk.lattice(us, chunks, T, 1), chk.lattice(us, chunks, T, 2)
    B, _, NS, NA = capacity([big])
    assert len(small["state_time"]) < NS - 1 and len(small["arc_src"]) < NA - 1 and B == 12
    who = "supervision_assign_alignment_chunks: "

    def holds(ds, want):
        def refused(call, *words):
            with pytest.raises(abi.HipAbiError) as e:
                call()
            assert "tdnnf error 1:" in str(e.value)  # TDNNF_EINVAL
            for word in words:
                assert word in str(e.value), (word, str(e.value))
            assert ds.capacity()["assigns"] == 1 and (ds.B, ds.T) == (B, T)
            same_tables(ds.tables(), want, words)
        return refused

    # one state, one arc over the capacity (the other capacity roomy enough for the staging)
    for cap, words in (((B, T, NS - 1, NA + 4 * B), "%d states exceed the capacity max_states = %d by 1" % (NS, NS - 1)),
                       ((B, T, NS + 8 * B, NA - 1), "%d arcs exceed the capacity max_arcs = %d by 1" % (NA, NA - 1))):
        tight = abi.Supervision.reserve(*cap)
        tight.assign_alignment_chunks(units, al, frames, first, T, 1)
        holds(tight, tight.tables())(lambda: tight.assign_alignment_chunks(units, al, frames, first, T, 2), who, words)
    ds = abi.Supervision.reserve(*roomy((B, T, NS, NA)))
    ds.assign_alignment_chunks(units, al, frames, first, T, 2)
    want = ds.tables()
    refused = holds(ds, want)
    at = lambda a, i, v: list(a[:i]) + [v] + list(a[i + 1:])
    u2, b2 = al[-1]  # the random segmentation
    assert len(u2) >= 2
    # the alignment's refusals, against the utterance's frames
    refused(lambda: ds.assign_alignment_chunks(units, at(al, 0, (al[0][0], np.ones(1, np.int32))), frames, first, T, 2), who, "sequence 0 unit 0", "starts at frame 1")
    refused(lambda: ds.assign_alignment_chunks(units, at(al, B - 1, (u2, np.concatenate([b2[:-1], [Tu]]))), frames, first, T, 2), who,
            "sequence %d unit %d" % (B - 1, len(b2) - 1), "starts at frame %d, outside the %d frames" % (Tu, Tu))
    refused(lambda: ds.assign_alignment_chunks(units, at(al, B - 1, (np.concatenate([u2[:-1], [ali.U]]), b2)), frames, first, T, 2), who,
            "sequence %d unit %d" % (B - 1, len(b2) - 1), "unit %d outside [0, %d)" % (ali.U, ali.U))
    refused(lambda: ds.assign_alignment_chunks(units, al, frames, first, T, -1), who, "tolerance -1 is negative")
    # the chunks' own
    refused(lambda: ds.assign_alignment_chunks(units, al, at(frames, 3, 0), first, T, 2), who, "sequence 3: an utterance of 0 frames")
    refused(lambda: ds.assign_alignment_chunks(units, al, frames, at(first, 4, -1), T, 2), who, "sequence 4: the chunk begins at frame -1")
    refused(lambda: ds.assign_alignment_chunks(units, al, frames, at(first, 5, Tu - T + 1), T, 2), who,
            "sequence 5: the chunk of %d frames from frame %d ends behind the %d frames of the utterance" % (T, Tu - T + 1, Tu))
    refused(lambda: ds.assign_alignment_chunks(units, al + al[:1], frames + frames[:1], first + first[:1], T, 2), who, "max_sequences = %d by 1" % B)
    with pytest.raises(abi.HipAbiError, match="alignment_chunk_supervision_sizes: sequence 5: the chunk of"):
        units.alignment_chunk_sizes(al, frames, at(first, 5, Tu - T + 1), T, 2)
    # a reserve of exactly the states and arcs of one-frame chunks has too little staging: refused by name, the minibatch kept
    ones = chk.small_batch(Tu, 1)
    one = chk.lattice(us, ones, 1, 0)
    exact = abi.Supervision.reserve(*capacity([one]))
    exact.assign(one)
    kept = exact.tables()
    with pytest.raises(abi.HipAbiError) as e:
        exact.assign_alignment_chunks(units, *args(ones), 1, 0)
    assert "tdnnf error 1:" in str(e.value) and who in str(e.value) and "bytes of staging" in str(e.value) and "short by" in str(e.value)
    assert exact.capacity()["assigns"] == 1
    same_tables(exact.tables(), kept, "staging")
    # the objective still has the previous minibatch's bits
    y, xo = inputs(big, 9)
    assigned = abi.Supervision.reserve(B, T, NS, NA)
    assigned.assign(big)
    same_bits(run(hip, den, assigned, y, xo), run(hip, den, ds, y, xo))
    # an end-to-end handle, a created handle
    e2e = abi.Supervision.reserve_e2e(B, T, ali.P, 64, 256)
    with pytest.raises(abi.HipAbiError) as e:
        e2e.assign_alignment_chunks(units, al, frames, first, T, 2)
    assert who + "an end-to-end supervision" in str(e.value) and e2e.kind == 1
    made = abi.Supervision(big)
    before = made.tables()
    with pytest.raises(abi.HipAbiError) as e:
        made.assign_alignment_chunks(units, al, frames, first, T, 1)
    assert who in str(e.value) and "tdnnf_supervision_create" in str(e.value) and "tdnnf_supervision_reserve" in str(e.value)
    for name, v in made.tables().items():
        assert np.array_equal(v.view(np.int32), before[name].view(np.int32)), name


def test_the_three_assigns_alternate_on_one_handle_and_allocate_nothing(abi, sets, large):
    us, units = sets[0]
    chunks, T, tol, _ = large["wide"]
    whole = ali.small_batch(7)
    a, b = chk.lattice(us, chunks, T, tol), ali.lattice(us, whole, 7, 5)
    cap = roomy(capacity([a, b]))
    ref = abi.Supervision.reserve(*cap)
    ref.assign(a)
    want_a = ref.tables()
    ref.assign(b)
    want_b = ref.tables()
    ds = abi.Supervision.reserve(*cap)
    free = torch.cuda.mem_get_info()[0]
    for i in range(12):
        kind, which = i % 3, (i // 3) % 2  # chunks / alignments / arrays; a, b, a, b within each kind
        if kind == 0:
            if which == 0:
                ds.assign_alignment_chunks(units, *args(chunks), T, tol)
            else:
                ds.assign_alignment_chunks(units, whole, [7] * 3, [0] * 3, 7, 5)
        elif kind == 1:
            ds.assign_alignments(units, whole, 7, 5)
            which = 1
        else:
            ds.assign(a if which == 0 else b)
        same_tables(ds.tables(), want_a if which == 0 else want_b, i)
    c = ds.capacity()
    assert c["allocations"] == 0 and c["assigns"] == 12
    assert torch.cuda.mem_get_info()[0] == free  # the device agrees: nothing was allocated or freed


def test_stream_order(abi, hip, den, sets, large):
    """objective on A, assign_alignment_chunks B, objective on B, and only then a look at either; three times over, so that both staging
    buffers come round: a call enqueued before an assign sees the previous minibatch"""
    us, units = sets[1]
    ch_a, Ta, tol_a, _ = large["wide"]
    ch_b, Tb, tol_b = chk.small_batch(40, 7), 7, 5
    a, b = chk.lattice(us, ch_a, Ta, tol_a), chk.lattice(us, ch_b, Tb, tol_b)
    ya, xa = inputs(a, 1)
    yb, xb = inputs(b, 2)
    cap = roomy(capacity([a, b]))
    ref = abi.Supervision.reserve(*cap)
    ref.assign(a)
    want_a = run(hip, den, ref, ya, xa)
    ref.assign(b)
    want_b = run(hip, den, ref, yb, xb)
    ds = abi.Supervision.reserve(*cap)
    ds.assign_alignment_chunks(units, *args(ch_a), Ta, tol_a)
    for _ in range(3):
        out_a, keep_a = enqueue(hip, den, ds, ya, xa)
        ds.assign_alignment_chunks(units, *args(ch_b), Tb, tol_b)
        out_b, keep_b = enqueue(hip, den, ds, yb, xb)
        ds.assign_alignment_chunks(units, *args(ch_a), Ta, tol_a)
        same_bits(want_a, [host(t).copy() for t in out_a])
        same_bits(want_b, [host(t).copy() for t in out_b])
    assert ds.capacity()["assigns"] == 7 and ds.capacity()["allocations"] == 0
