"""-m gpu: supervisions compiled on the device from alignments and a frame tolerance (tdnnf_supervision_assign_alignments,
tdnnf_alignment_supervision_sizes; include/tdnnf_hip.h "ALIGNMENT SUPERVISIONS").  The specification is tests/alignment_supervision_ref.py,
the lattice in numpy from its definition (tests/test_alignment_supervision_ref.py holds it to its properties): a reserved supervision
assigned alignments has BYTE FOR BYTE the 17 device tables of a second reserved supervision given assign(the statement's dict), the same
info(), and tdnnf_chain_objf_and_deriv / tdnnf_chain_objf give the same BITS from the two -- the same build kernels run on equal raw arrays.
Then the closed loop (assign_transcripts, best_path_labels, infer.alignment_from_path, assign_alignments with tolerance 0: the lattice is
the best path), the refusals (each leaves the previous minibatch byte for byte), both assigns alternating on one handle with no
allocation, and stream order."""
import numpy as np
import pytest
import torch

from tests import alignment_supervision_ref as ali
from tests.gpu_util import Hip, dev, host
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


def same_tables(got, want, what):
    assert set(got) == set(want) and len(got) == 17
    for name in want:
        a, b = got[name], want[name]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)), (what, name)


def both(abi, units, us, alignments, T, tol, compiled, assigned, weight=1.0):
    """the minibatch on both handles; the statement's dict"""
    s = ali.lattice(us, alignments, T, tol, weight=weight)
    compiled.assign_alignments(units, alignments, T, tol, weight=weight)
    assigned.assign(s)
    return s


@pytest.mark.parametrize("context", [0, 1])
@pytest.mark.parametrize("T", ali.FRAMES)
def test_tables_and_info_are_those_of_an_assign_of_the_lattice(abi, sets, context, T):
    us, units = sets[context]
    alignments = ali.small_batch(T)
    assert [len(u) for u, _ in alignments][:2] == [1, T]
    sups = [ali.lattice(us, alignments, T, tol) for tol in ali.tolerances(T)]
    cap = capacity(sups)  # exactly the largest: nothing may be written beyond it
    compiled, assigned = abi.Supervision.reserve(*cap), abi.Supervision.reserve(*cap)
    for tol, s in zip(ali.tolerances(T), sups):
        states, arcs = units.alignment_sizes(alignments, T, tol)
        assert states.tolist() == np.diff(s["seq_state_begin"]).tolist() and arcs.tolist() == np.diff(s["seq_arc_begin"]).tolist()
        assert states[1] == T + 1 and arcs[1] == T  # every unit one frame: a single path for any tolerance
        compiled.assign_alignments(units, alignments, T, tol)
        assigned.assign(s)
        assert compiled.info() == assigned.info() and (compiled.B, compiled.T) == (3, T), tol
        assert compiled.info()["num_states"] == len(s["state_time"]) and compiled.info()["num_arcs"] == len(s["arc_src"])
        same_tables(compiled.tables(), assigned.tables(), (context, T, tol))
    assert compiled.capacity()["allocations"] == 0 and compiled.capacity()["assigns"] == 5


@pytest.fixture(scope="module")
def large(pkg):
    """name -> (alignments, T, tolerance, wide)"""
    return {"narrow": ali.narrow_batch() + (False,), "wide": ali.wide_batch() + (True,)}


@pytest.mark.parametrize("context", [0, 1])
@pytest.mark.parametrize("name", ["narrow", "wide"])
def test_tables_of_the_narrow_and_the_wide_minibatch(abi, sets, large, context, name):
    us, units = sets[context]
    alignments, T, tol, wide = large[name]
    s = ali.lattice(us, alignments, T, tol)
    assert ali.is_wide(s) == wide and (len(alignments), T, tol) == ((4, 150, 5) if name == "narrow" else (2, 60, 40))
    cap = capacity([s])
    compiled, assigned = abi.Supervision.reserve(*cap), abi.Supervision.reserve(*cap)
    compiled.assign_alignments(units, alignments, T, tol)
    assigned.assign(s)
    assert compiled.info() == assigned.info() and compiled.info()["wide"] == int(wide)
    same_tables(compiled.tables(), assigned.tables(), name)


@pytest.mark.parametrize("name", ["narrow", "wide"])
def test_objective_and_derivatives_are_the_assigned_lattices_bits(abi, hip, den, sets, large, name):
    us, units = sets[1]
    alignments, T, tol, wide = large[name]
    cap = capacity([ali.lattice(us, alignments, T, tol)])
    compiled, assigned = abi.Supervision.reserve(*cap), abi.Supervision.reserve(*cap)
    s = both(abi, units, us, alignments, T, tol, compiled, assigned, weight=0.75)
    y, xo = inputs(s, 3)
    want, got = run(hip, den, assigned, y, xo), run(hip, den, compiled, y, xo)
    assert want[0][5] == 1.0 and np.isfinite(want[0][:7]).all() and np.abs(want[1]).sum() > 0 and np.abs(want[2]).sum() > 0
    same_bits(want, got)


@pytest.mark.parametrize("context", [0, 1])
def test_the_loop_closes_on_the_best_path(pkg, abi, sets, context):
    """align against the transcript, segment, supervise with tolerance 0: the supervision is the best path"""
    us, units = sets[context]
    B, T = 3, 20
    transcripts = pkg.synth.make_transcripts(B, ali.U, slots=(2, 7), optional_rate=0.4, seed=11 + context)
    states, arcs = units.sizes(transcripts)
    graphs = abi.AlignGraphs.reserve(B, ali.P, int(states.sum()), int(arcs.sum()), num_labels=7)
    graphs.assign_transcripts(units, transcripts)
    rng = np.random.default_rng(5)
    y = dev((2.0 * rng.standard_normal((B * T, ali.P))).astype(np.float32))
    pdfs, _, results, labels, _ = graphs.best_path_labels(y, [T] * B, np.arange(B) * T)
    pdfs, labels, results = host(pdfs), host(labels), host(results)
    assert (results[:, 1] == 1.0).all()
    alignments = [pkg.infer.alignment_from_path(labels[u * T:(u + 1) * T], transcripts[u]) for u in range(B)]
    sup = abi.Supervision.reserve(B, T, B * (T + 1), B * T)
    sup.assign_alignments(units, alignments, T, 0)
    t = sup.tables()
    assert np.diff(t["seq_state_begin"]).tolist() == [T + 1] * B and sup.info()["num_arcs"] == B * T
    assert np.array_equal(t["out_pdf"], pdfs)  # state order is time order: the arc out of the state of time t is frame t's
    assert t["state_time"].tolist() == list(range(T + 1)) * B


def test_refusals_leave_the_previous_minibatch(abi, hip, den, sets, pkg):
    us, units = sets[1]
    T = 7
    alignments = ali.small_batch(T)
    small, big = ali.lattice(us, alignments, T, 1), ali.lattice(us, alignments, T, 2)
    B, _, NS, NA = capacity([big])
    assert len(small["state_time"]) < NS - 1 and len(small["arc_src"]) < NA - 1
    who = "supervision_assign_alignments: "

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

    # one state, one arc over the capacity
    for cap, words in (((B, T, NS - 1, NA), "%d states exceed the capacity max_states = %d by 1" % (NS, NS - 1)),
                       ((B, T, NS, NA - 1), "%d arcs exceed the capacity max_arcs = %d by 1" % (NA, NA - 1))):
        tight = abi.Supervision.reserve(*cap)
        tight.assign_alignments(units, alignments, T, 1)
        holds(tight, tight.tables())(lambda: tight.assign_alignments(units, alignments, T, 2), who, words)
    ds = abi.Supervision.reserve(B, T, NS, NA)
    ds.assign_alignments(units, alignments, T, 2)
    want = ds.tables()
    refused = holds(ds, want)
    (u0, b0), (u1, b1), (u2, b2) = alignments
    at = lambda a, i, v: np.concatenate([a[:i], [v], a[i + 1:]]).astype(np.int32)
    assert len(u2) >= 2
    refused(lambda: ds.assign_alignments(units, [(u0, at(b0, 0, 1)), (u1, b1), (u2, b2)], T, 2), who, "sequence 0 unit 0", "starts at frame 1")
    refused(lambda: ds.assign_alignments(units, [(u0, b0), (u1, at(b1, 3, 2)), (u2, b2)], T, 2), who, "sequence 1 unit 3", "not behind")
    refused(lambda: ds.assign_alignments(units, [(u0, b0), (u1, b1), (u2, at(b2, len(b2) - 1, T))], T, 2), who,
            "sequence 2 unit %d" % (len(b2) - 1), "starts at frame %d, outside the %d frames" % (T, T))
    refused(lambda: ds.assign_alignments(units, [(u0, b0), (at(u1, 4, ali.U), b1), (u2, b2)], T, 2), who, "sequence 1 unit 4", "unit %d outside [0, %d)" % (ali.U, ali.U))
    refused(lambda: ds.assign_alignments(units, alignments, T, -1), who, "tolerance -1 is negative")
    refused(lambda: ds.assign_alignments(units, alignments + alignments[:1], T, 2), who, "max_sequences = 3 by 1")
    for bad in ([(u0, at(b0, 0, 1)), (u1, b1), (u2, b2)], [(u0, b0), (u1, b1), (at(u2, 1, -1), b2)]):  # the sizes entry: the same words under its name
        with pytest.raises(abi.HipAbiError, match="alignment_supervision_sizes: sequence"):
            units.alignment_sizes(bad, T, 2)
    # the objective still has the previous minibatch's bits
    y, xo = inputs(big, 9)
    assigned = abi.Supervision.reserve(B, T, NS, NA)
    assigned.assign(big)
    same_bits(run(hip, den, assigned, y, xo), run(hip, den, ds, y, xo))
    # an end-to-end handle, a created handle
    e2e = abi.Supervision.reserve_e2e(B, T, ali.P, 64, 256)
    with pytest.raises(abi.HipAbiError) as e:
        e2e.assign_alignments(units, alignments, T, 2)
    assert who + "an end-to-end supervision" in str(e.value) and e2e.kind == 1
    made = abi.Supervision(big)
    before = made.tables()
    with pytest.raises(abi.HipAbiError) as e:
        made.assign_alignments(units, alignments, T, 1)
    assert who in str(e.value) and "tdnnf_supervision_create" in str(e.value) and "tdnnf_supervision_reserve" in str(e.value)
    for name, v in made.tables().items():
        assert np.array_equal(v.view(np.int32), before[name].view(np.int32)), name


def test_both_assigns_alternate_on_one_handle_and_allocate_nothing(abi, sets, large):
    us, units = sets[0]
    alignments, T, tol, _ = large["wide"]
    other = ali.small_batch(7)
    a, b = ali.lattice(us, alignments, T, tol), ali.lattice(us, other, 7, 5)
    cap = capacity([a, b])
    ref = abi.Supervision.reserve(*cap)
    ref.assign(a)
    want_a = ref.tables()
    ref.assign(b)
    want_b = ref.tables()
    ds = abi.Supervision.reserve(*cap)
    free = torch.cuda.mem_get_info()[0]
    for i in range(10):
        if i % 2 == 0:
            ds.assign_alignments(units, alignments, T, tol) if i % 4 == 0 else ds.assign_alignments(units, other, 7, 5)
        else:
            ds.assign(b if i % 4 == 1 else a)
        same_tables(ds.tables(), want_a if i % 4 in (0, 3) else want_b, i)
    c = ds.capacity()
    assert c["allocations"] == 0 and c["assigns"] == 10
    assert torch.cuda.mem_get_info()[0] == free  # the device agrees: nothing was allocated or freed


def test_stream_order(abi, hip, den, sets, large):
    """objective on A, assign_alignments B, objective on B, and only then a look at either; three times over, so that both staging buffers come round"""
    us, units = sets[1]
    al_a, Ta, tol_a, _ = large["wide"]
    al_b, Tb, tol_b = ali.small_batch(40), 40, 5
    a, b = ali.lattice(us, al_a, Ta, tol_a), ali.lattice(us, al_b, Tb, tol_b)
    ya, xa = inputs(a, 1)
    yb, xb = inputs(b, 2)
    ref = abi.Supervision.reserve(*capacity([a, b]))
    ref.assign(a)
    want_a = run(hip, den, ref, ya, xa)
    ref.assign(b)
    want_b = run(hip, den, ref, yb, xb)
    ds = abi.Supervision.reserve(*capacity([a, b]))
    ds.assign_alignments(units, al_a, Ta, tol_a)
    for _ in range(3):
        out_a, keep_a = enqueue(hip, den, ds, ya, xa)
        ds.assign_alignments(units, al_b, Tb, tol_b)
        out_b, keep_b = enqueue(hip, den, ds, yb, xb)
        ds.assign_alignments(units, al_a, Ta, tol_a)
        same_bits(want_a, [host(t).copy() for t in out_a])
        same_bits(want_b, [host(t).copy() for t in out_b])
    assert ds.capacity()["assigns"] == 7 and ds.capacity()["allocations"] == 0
