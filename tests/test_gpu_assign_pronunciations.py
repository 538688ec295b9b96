"""-m gpu: transcript graphs with pronunciation alternatives compiled on the device (tdnnf_pronunciation_graph_sizes,
tdnnf_align_graphs_assign_pronunciations, tdnnf_supervision_assign_e2e_pronunciations; include/tdnnf_hip.h "PRONUNCIATION GRAPHS").  The
specification is tests/pronunciation_graphs_ref.py, the definition in numpy (tests/test_pronunciation_graphs_ref.py pins it): a handle
assigned from pronunciation transcripts has BYTE FOR BYTE the device arrays (AlignGraphs.tables) of a handle assigned the statement's arc
arrays, and since the kernels that read them are the same, every entry gives the same bits.  No tolerance anywhere.

Shapes (tests/pronunciation_graphs_ref.py): 7 transcripts of 1 to 6 positions with 1 to 3 alternatives of 1 to 3 units -- an optional
position first, last and between two multi-alternative positions, one-unit alternatives on both sides of an optional position -- and one of
them alone (batches of 7 and 1); a transcript of more than 256 entries (the chunk carries); two positions of 65 one-unit alternatives one
behind the other (66 arcs into a state: a heavy row of the build).  Both contexts, labelled and unlabelled handles.

An end-to-end supervision has no tables of its own to dump (tdnnf_supervision_dump refuses it: its tables are its graph set's, which the
first test compares): the supervision test compares info, the launch form and the bits of the objective and both derivatives."""
import gc

import numpy as np
import pytest
import torch

from tests import pronunciation_graphs_ref as ref
from tests import transcript_graphs_ref as slots_ref
from tests.gpu_util import Hip, dev
from tests.test_gpu_align_assign import outputs, refused, same_outputs, same_tables, totals
from tests.test_gpu_chain_e2e_assign import run, same_bits

pytestmark = pytest.mark.gpu
F = np.float32
NAMES = ["edge-7", "one", "long", "heavy"]


@pytest.fixture(scope="module")
def abi(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pkg.hipabi


def batches():
    """{name: transcripts}"""
    return {"edge-7": ref.edge_batch(), "one": [ref.edge_batch()[4]], "long": [ref.long_transcript()], "heavy": [ref.heavy_transcript()]}


@pytest.fixture(scope="module")
def sets(pkg):
    """per context the unit set dict (pdfs that collide: the column lists are shorter than the states' pdfs) and, computed once, the
    statement's graphs of every batch"""
    out = {}
    for context in (0, 1):
        us = ref.unit_set(pkg.synth, context, distinct=False)
        b = batches()
        out[context] = dict(us=us, transcripts=b, graphs={k: [ref.pronunciation_graph(us, t) for t in v] for k, v in b.items()})
    return out


def unit_set(abi, us):
    return abi.UnitSet(us["entry_pdf"], us["loop_pdf"], us["loop_logprob"], us["leave_logprob"], us["P"], us["take_logprob"], us["skip_logprob"])


ARRAYS = ("S", "P", "src", "dst", "pdf", "logprob", "init", "final")


def plain(graphs, labelled):
    """the statement's graphs as AlignGraphs takes them"""
    return [{k: g[k] for k in ARRAYS + (("label", "L") if labelled else ())} for g in graphs]


def num_labels(graphs, labelled):
    return max(g["L"] for g in graphs) if labelled else None


# ------------------------------------------------------------------------------------------------ 1. bytes
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("labelled", [False, True], ids=["plain", "labelled"])
@pytest.mark.parametrize("context", [0, 1])
def test_compiled_tables_are_the_statements_tables(abi, sets, context, labelled, name):
    s = sets[context]
    P = s["us"]["P"]
    transcripts, graphs = s["transcripts"][name], plain(s["graphs"][name], labelled)
    units = unit_set(abi, s["us"])
    G, S, A = totals(graphs)
    L = num_labels(graphs, labelled)
    states, arcs = units.pronunciation_sizes(transcripts)  # tdnnf_pronunciation_graph_sizes: what the reserve is sized from
    assert states.tolist() == [g["S"] for g in graphs] and arcs.tolist() == [len(g["src"]) for g in graphs]
    compiled = abi.AlignGraphs.reserve(G, P, S, A, num_labels=L)  # exactly the batch: nothing may be written beyond it
    compiled.assign_pronunciations(units, transcripts)
    assigned = abi.AlignGraphs.reserve(G, P, S, A, num_labels=L)
    assigned.assign(graphs)
    same_tables(assigned, compiled)
    assert compiled.G == assigned.G and compiled.num_states == assigned.num_states and np.array_equal(compiled.arc_begin, assigned.arc_begin)
    for k in range(G):
        assert compiled.info(k) == assigned.info(k) and np.array_equal(compiled.pdfs(k), assigned.pdfs(k))
        assert not labelled or np.array_equal(compiled.labels(k), assigned.labels(k))
    if name == "heavy":
        assert compiled.info(0)["max_in_degree"] == 66 and len(compiled.tables()["by_dst"]["heavy"]) > 0
    if name == "long":
        assert ref.flat_arrays(transcripts)[4][-1] > 256


def test_a_larger_capacity_gives_the_same_tables(abi, sets):
    s = sets[1]
    graphs = plain(s["graphs"]["edge-7"], True)
    compiled = abi.AlignGraphs.reserve(9, s["us"]["P"], 400, 1500, num_labels=30)
    compiled.assign_pronunciations(unit_set(abi, s["us"]), s["transcripts"]["edge-7"])
    same_tables(abi.AlignGraphs(graphs, num_pdfs=s["us"]["P"], num_labels=30), compiled)


# ------------------------------------------------------------------------------------------------ 2. reduction
@pytest.mark.parametrize("labelled", [False, True], ids=["plain", "labelled"])
@pytest.mark.parametrize("context", [0, 1])
def test_single_alternative_single_unit_transcripts_compile_to_slot_transcripts(pkg, abi, sets, context, labelled):
    us = sets[context]["us"]
    units = unit_set(abi, us)
    slots = pkg.synth.make_transcripts(7, ref.U, slots=(1, 12), optional_rate=0.4, seed=8) + pkg.synth.make_transcripts(1, ref.U, slots=(300, 300), optional_rate=0.4, seed=9)
    states, arcs = units.sizes(slots)
    L = max(len(u) for u, _ in slots) if labelled else None
    by_slots = abi.AlignGraphs.reserve(len(slots), us["P"], int(states.sum()), int(arcs.sum()), num_labels=L)
    by_slots.assign_transcripts(units, slots)
    by_positions = abi.AlignGraphs.reserve(len(slots), us["P"], int(states.sum()), int(arcs.sum()), num_labels=L)
    by_positions.assign_pronunciations(units, [ref.as_slots(u, o) for u, o in slots])
    same_tables(by_slots, by_positions)
    assert by_slots.num_states == by_positions.num_states and np.array_equal(by_slots.arc_begin, by_positions.arc_begin)
    assert all(by_slots.info(k) == by_positions.info(k) for k in range(len(slots)))


# ------------------------------------------------------------------------------------------------ 3. planted pronunciations
def planted():
    """[(transcript, the alternative planted at every position or -1 for a skipped one)] over 10 units; neighbouring positions draw from
    disjoint units and no alternative of a position begins another, so a sequence of units names its pronunciations"""
    eighths = lambda *x: [F(-v / 8.0) for v in x]
    return [(([[[0, 1], [2]], [[3]], [[7], [8, 9], [9]], [[0], [1, 0]]], [0, 1, 0, 0], [eighths(2, 1), eighths(0), eighths(1, 5, 0), eighths(3, 3)]), [1, -1, 1, 1]),
            (([[[1]], [[4, 5], [5, 4], [6]], [[7, 7], [8]]], [1, 0, 0], [eighths(0), eighths(0, 2, 9), eighths(4, 1)]), [0, 2, 0]),
            (([[[2], [0]], [[3, 4, 5]], [[9]]], [0, 0, 1], [eighths(6, 2), eighths(0), eighths(1)]), [1, 0, -1])]


@pytest.mark.parametrize("context", [0, 1])
def test_planted_pronunciations_are_the_best_path(pkg, abi, context):
    us = pkg.synth.make_unit_set(10, context=context, seed=21, distinct=True)  # every (left, unit) entry and loop pdf a pdf of its own
    P = us["P"]
    entry, loop = np.asarray(us["entry_pdf"]), np.asarray(us["loop_pdf"])
    pdf_of = lambda table, left, u: int(table[left + 1, u] if context else table[u])
    units = unit_set(abi, us)
    transcripts = [t for t, _ in planted()]
    rng = np.random.default_rng(3)
    rows_of, want = [], []  # per utterance its frames' planted pdfs; (entries per frame, units, starts, chosen)
    for t, chosen in planted():
        number = ref.entry_numbers(t[0])
        pdfs, entries, us_, starts, left = [], [], [], [], -1
        for p, a in enumerate(chosen):
            for j, u in enumerate(t[0][p][a] if a >= 0 else []):
                d = int(rng.integers(1, 4))
                starts.append(len(pdfs))
                us_.append(u)
                pdfs += [pdf_of(entry, left, u)] + [pdf_of(loop, left, u)] * (d - 1)
                entries += [number[(p, a, j)]] * d
                left = u
        rows_of.append(pdfs)
        want.append((entries, us_, starts, chosen))
    frames = [len(r) for r in rows_of]
    rows = np.concatenate([[0], np.cumsum(frames)[:-1]])
    y = np.zeros((sum(frames), P), F)
    y[np.arange(sum(frames)), np.concatenate(rows_of)] = 1000.0  # (a path that leaves the planted pdfs for one frame loses 1000; all weights together are above -200)
    y = dev(y)
    graphs = [ref.pronunciation_graph(us, t) for t in transcripts]
    G, S, A = totals(graphs)
    L = num_labels(graphs, True)
    compiled = abi.AlignGraphs.reserve(G, P, S, A, num_labels=L)
    compiled.assign_pronunciations(units, transcripts)
    assigned = abi.AlignGraphs.reserve(G, P, S, A, num_labels=L)
    assigned.assign(plain(graphs, True))
    got = outputs(compiled, y, frames, rows, True)  # best_path, logprob, posteriors, posteriors_compact, the sparse and the labelled ones
    same_outputs(outputs(assigned, y, frames, rows, True), got)
    pdf_out, _, results, label_out, _ = compiled.best_path_labels(y, frames, rows, states=True)
    torch.cuda.synchronize()
    assert (results[:, 1] == 1).all()
    assert pdf_out.cpu().numpy().tolist() == np.concatenate(rows_of).tolist()
    labels = label_out.cpu().numpy()
    for k, (t, (entries, us_, starts, chosen)) in enumerate(zip(transcripts, want)):
        mine = labels[rows[k]:rows[k] + frames[k]]
        assert mine.tolist() == entries, k
        u, b, c = pkg.infer.alignment_from_pronunciation_path(mine, t)
        assert u.tolist() == us_ and b.tolist() == starts and c.tolist() == chosen, k
        assert u.dtype == b.dtype == np.int32
    # a path that is none
    with pytest.raises(ValueError):
        pkg.infer.alignment_from_pronunciation_path(labels[rows[0]:rows[0] + frames[0]][::-1].copy(), transcripts[0])
    with pytest.raises(ValueError):
        pkg.infer.alignment_from_pronunciation_path(np.full(4, -1), transcripts[0])


# ------------------------------------------------------------------------------------------------ 4. the end-to-end supervision
@pytest.mark.parametrize("context", [0, 1])
def test_e2e_supervision_from_pronunciations(pkg, abi, context):
    """one reserved supervision, two minibatches that differ in sequences, frames and graphs: the chain objective and its derivatives from
    pronunciation transcripts have the bits of the same calls after assign with the statement's graphs"""
    hip = Hip(pkg)
    synth = pkg.synth
    Pd = 41
    us = synth.make_unit_set(ref.U, context=context, seed=3, distinct=False, P=Pd)
    units = unit_set(abi, us)
    den = abi.DenGraph(synth.make_den_graph(30, Pd, mean_out_degree=4.0, seed=5))
    minibatches = [(3, 16, 1.0, synth.make_pronunciation_transcripts(3, ref.U, positions=(2, 5), seed=40)),
                   (5, 14, 0.75, synth.make_pronunciation_transcripts(5, ref.U, positions=(1, 4), seed=41))]
    graphs = [[ref.pronunciation_graph(us, t) for t in m[3]] for m in minibatches]
    cap = (5, 16, max(totals(g)[1] for g in graphs), max(totals(g)[2] for g in graphs))
    compiled = abi.Supervision.reserve_e2e(cap[0], cap[1], Pd, cap[2], cap[3])
    assigned = abi.Supervision.reserve_e2e(cap[0], cap[1], Pd, cap[2], cap[3])
    for i, ((B, T, w, transcripts), gs) in enumerate(zip(minibatches, graphs)):
        rng = np.random.default_rng(50 + i)
        y = dev((1.5 * rng.standard_normal((B * T, Pd))).astype(F))
        xo = rng.standard_normal((B * T, Pd))
        xo = dev((xo - np.log(np.exp(xo).sum(1, keepdims=True))).astype(F))
        compiled.assign_pronunciations(units, transcripts, T, weight=w)
        assigned.assign(plain(gs, False), T, weight=w)
        assert compiled.e2e_form() == assigned.e2e_form() and compiled.info() == assigned.info() and (compiled.B, compiled.T) == (B, T)
        want, got = run(hip, den, assigned, y, xo), run(hip, den, compiled, y, xo)
        same_bits(want, got)
        assert want[0][5] == 1.0 and np.isfinite(want[0][:7]).all() and np.abs(want[1]).sum() > 0
    # refusals leave the minibatch: too many sequences, too many frames, a bad position, too many states, a created supervision
    who = "supervision_assign_e2e_pronunciations: "
    last = minibatches[1][3]
    refused(abi, lambda: compiled.assign_pronunciations(units, last + [([[[1]]], [0])], 14), who, "max_sequences", "by 1")
    refused(abi, lambda: compiled.assign_pronunciations(units, last, 17), who, "max_frames", "by 1")
    refused(abi, lambda: compiled.assign_pronunciations(units, [([[[1]], [[2]]], [1, 1])] + last[1:], 14), who, "transcript 0 position 1", "adjacent optional")
    refused(abi, lambda: compiled.assign_pronunciations(units, [([[[u % ref.U] for u in range(12)]] * 12, [0] * 12)] * 5, 14), "max_states")
    assert (compiled.B, compiled.T) == (5, 14) and compiled.info() == assigned.info()
    same_bits(want, run(hip, den, compiled, y, xo))
    made = abi.Supervision.from_graphs(plain(graphs[0], False), 16, num_pdfs=Pd)
    refused(abi, lambda: made.assign_pronunciations(units, minibatches[0][3], 16), who, "tdnnf_supervision_reserve_e2e")


# ------------------------------------------------------------------------------------------------ 5. refusals, capacities, allocation
@pytest.mark.parametrize("context", [0, 1])
def test_refusals_keep_the_previous_batch(abi, sets, context):
    s = sets[context]
    P = s["us"]["P"]
    units = unit_set(abi, s["us"])
    transcripts, graphs = s["transcripts"]["edge-7"][:4], plain(s["graphs"]["edge-7"][:4], True)
    G, S, A = totals(graphs)
    L = num_labels(graphs, True)
    made = abi.AlignGraphs(graphs, num_pdfs=P, num_labels=L)
    frames = [12] * G
    rows = (np.arange(G) * 12).tolist()
    y = dev(np.random.default_rng(31).standard_normal((G * 12, P)).astype(F))
    want = outputs(made, y, frames, rows, True)
    who = "align_graphs_assign_pronunciations: "

    def holds(res, labelled=True):
        assert res.G == G and res.capacity()["assigns"] == 1
        same_tables(made if labelled else abi.AlignGraphs(plain(s["graphs"]["edge-7"][:4], False), num_pdfs=P), res)
        if labelled:
            same_outputs(want, outputs(res, y, frames, rows, True))

    res = abi.AlignGraphs.reserve(G + 1, P, S + 60, A + 300, num_labels=L)
    res.assign_pronunciations(units, transcripts)
    good = transcripts[1]
    U = ref.U
    for bad, words in ((([[[1]], []], [0, 0]), ("transcript 1 position 1 has 0 alternatives",)),
                       (([[[1]], [[2], []]], [0, 0]), ("transcript 1 position 1 alternative 1 has 0 units",)),
                       (([[[1]], [[2], [0, U]]], [0, 0]), ("transcript 1 position 1 alternative 1", "unit %d (its number 1) outside [0, %d)" % (U, U))),
                       (([[[1, -1]]], [0]), ("transcript 1 position 0 alternative 0", "unit -1 (its number 1) outside")),
                       (([[[1]], [[2], [3]]], [0, 0], [[0.0], [0.0, float("nan")]]), ("transcript 1 position 1 alternative 1", "alt_logprob is NaN or infinite")),
                       (([[[1], [4]]], [0], [[float("-inf"), 0.0]]), ("transcript 1 position 0 alternative 0", "alt_logprob is NaN or infinite")),
                       (([[[1]], [[2]], [[3]], [[4]]], [0, 1, 1, 0]), ("transcript 1 position 2", "adjacent optional positions")),
                       (([[[5], [2]]], [1]), ("transcript 1 position 0", "no mandatory position"))):
        refused(abi, lambda: res.assign_pronunciations(units, [good, bad]), who, *words)
        refused(abi, lambda: units.pronunciation_sizes([good, bad]), "pronunciation_graph_sizes: ", *words)  # the same refusal under its own name
        holds(res)
    refused(abi, lambda: res.assign_pronunciations(units, []), who, "bad arguments")
    holds(res)
    # num_labels smaller than the entries by one
    refused(abi, lambda: res.assign_pronunciations(units, [([[[u % U for u in range(L + 1)]]], [0])]), who, "num_labels = %d" % L, "short by 1")
    holds(res)
    # each of the three capacities exceeded by exactly 1: a handle that holds the batch, sized for one more transcript but for one kind
    over = transcripts + [([[[1]]], [0])]
    states, arcs = units.pronunciation_sizes(over)
    for short, word in enumerate(("max_graphs", "max_states", "max_arcs")):
        cap = [len(over), int(states.sum()), int(arcs.sum())]
        cap[short] -= 1
        tight = abi.AlignGraphs.reserve(cap[0], P, cap[1], cap[2], num_labels=L)
        tight.assign_pronunciations(units, transcripts)
        refused(abi, lambda: tight.assign_pronunciations(units, over), who, word, "by 1")
        holds(tight)
    # the unit set's num_pdfs against the handle's
    us = dict(s["us"], P=P + 1)
    refused(abi, lambda: res.assign_pronunciations(unit_set(abi, us), transcripts), who, "%d pdfs" % (P + 1), "num_pdfs %d" % P)
    holds(res)
    unlabelled = abi.AlignGraphs.reserve(G, P, S, A)
    unlabelled.assign_pronunciations(units, transcripts)
    refused(abi, lambda: unlabelled.assign(graphs), "align_graphs_assign", "without labels")
    holds(unlabelled, labelled=False)
    # a created handle
    refused(abi, lambda: made.assign_pronunciations(units, transcripts), who, "tdnnf_align_graphs_create")
    same_outputs(want, outputs(made, y, frames, rows, True))


def test_twenty_alternating_assigns_allocate_nothing(pkg, abi, sets):
    s = sets[1]
    P = s["us"]["P"]
    units = unit_set(abi, s["us"])
    slots = pkg.synth.make_transcripts(5, ref.U, slots=(1, 9), optional_rate=0.4, seed=6)
    slot_graphs = [{k: v for k, v in slots_ref.transcript_graph(s["us"], u, o).items() if k in ARRAYS} for u, o in slots]
    names = ["edge-7", "long", "one", "heavy"]
    cap = [max(v) for v in zip(*[totals(s["graphs"][n]) for n in names], totals(slot_graphs))]
    res = abi.AlignGraphs.reserve(cap[0], P, cap[1], cap[2])
    before = res.capacity()
    assert before["assigns"] == 0 and before["device_allocs"] == 1
    gc.collect()  # (the handles of earlier tests that only the collector frees go now, not between the two readings)
    free = torch.cuda.mem_get_info()[0]
    for i in range(20):
        if i % 3 == 0:
            res.assign(plain(s["graphs"][names[i % 4]], False))
        elif i % 3 == 1:
            res.assign_transcripts(units, slots)
        else:
            res.assign_pronunciations(units, s["transcripts"][names[i % 4]])
    after = res.capacity()
    assert after["assigns"] == 20 and {k: v for k, v in after.items() if k != "assigns"} == {k: v for k, v in before.items() if k != "assigns"}
    assert torch.cuda.mem_get_info()[0] == free  # the device agrees: nothing was allocated or freed
    same_tables(abi.AlignGraphs(slot_graphs, num_pdfs=P), res)  # the last, i = 19: assign_transcripts
    res.assign_pronunciations(units, s["transcripts"]["edge-7"])
    same_tables(abi.AlignGraphs(plain(s["graphs"]["edge-7"], False), num_pdfs=P), res)
