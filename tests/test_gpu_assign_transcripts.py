"""-m gpu: transcript graphs compiled on the device (tdnnf_unit_set_create, tdnnf_align_graphs_assign_transcripts,
tdnnf_supervision_assign_e2e_transcripts; include/tdnnf_hip.h "TRANSCRIPT GRAPHS").  The specification is tests/transcript_graphs_ref.py,
the definition in numpy (tests/test_transcript_graphs_ref.py holds it against synth.make_alignment_graph and a direct enumeration): a handle
assigned from transcripts has BYTE FOR BYTE the device arrays (AlignGraphs.tables) of a handle assigned, and of one created, from the
reference's graphs, and since the kernels that read them are the same, every entry gives the same bits.  No tolerance anywhere.

Shapes: what the compile kernel can get wrong -- the start's one or two arcs (first slot optional), the final weights behind an optional
last slot, B states and the skip's destination in context 1, optional slots back to back with mandatory ones, a unit beside itself, a
transcript of one slot, transcripts of 256 and 257 slots (the chunk of 256 threads, and one slot into the next) and of 700 (the scan's carry
over two chunk boundaries, with B states in between), one transcript and 70.  23 pdfs, 40 frames at most."""
import numpy as np
import pytest
import torch

from tests import transcript_graphs_ref as ref
from tests.gpu_util import Hip, dev
from tests.test_gpu_align_assign import refused, same_outputs, same_tables, totals
from tests.test_gpu_chain_e2e_assign import LEAKY, L2, XENT, run, same_bits

pytestmark = pytest.mark.gpu
F = np.float32
P, U = 23, 7


@pytest.fixture(scope="module")
def abi(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pkg.hipabi


def tr(units, optional):
    return np.asarray(units, np.int32), np.asarray(optional, np.int32)


def batches(synth):
    """{name: transcripts}"""
    rng = np.random.default_rng(0)
    alternating = np.arange(9) % 2
    return {
        "one-slot": [tr([3], [0])],
        "first-optional": [tr([1, 2, 3], [1, 0, 0]), tr([4, 5], [1, 0])],
        "last-optional": [tr([1, 2, 3], [0, 0, 1]), tr([4, 5], [0, 1])],
        "middle-optional": [tr([1, 2, 3, 4, 5], [0, 0, 1, 0, 0]), tr([6, 0, 6], [0, 1, 0])],
        "alternating": [tr(rng.integers(0, U, 9), alternating), tr(rng.integers(0, U, 9), 1 - alternating), tr(rng.integers(0, U, 8), np.arange(8) % 2)],
        "repeated-units": [tr([2, 2, 2, 5, 5], [0, 1, 0, 0, 1]), tr([4, 4], [1, 0]), tr([1, 1, 1], [0, 0, 0])],
        "700-slots": synth.make_transcripts(1, U, slots=(700, 700), optional_rate=0.4, seed=1),
        "256-and-257": synth.make_transcripts(1, U, slots=(256, 256), optional_rate=0.4, seed=2) + synth.make_transcripts(1, U, slots=(257, 257), optional_rate=0.4, seed=3),
        "70-graphs": synth.make_transcripts(70, U, slots=(1, 12), optional_rate=0.35, seed=4),
    }


@pytest.fixture(scope="module")
def sets(pkg):
    """per context the unit set dict (pdfs that collide: the column lists are shorter than the states' pdfs) and, computed once, the
    reference's graphs of every batch"""
    out = {}
    for context in (0, 1):
        us = pkg.synth.make_unit_set(U, context=context, seed=11 + context, distinct=False, P=P)
        b = batches(pkg.synth)
        out[context] = dict(us=us, transcripts=b, graphs={k: [ref.transcript_graph(us, u, o) for u, o in v] for k, v in b.items()})
    return out


def unit_set(abi, us):
    return abi.UnitSet(us["entry_pdf"], us["loop_pdf"], us["loop_logprob"], us["leave_logprob"], us["P"], us["take_logprob"], us["skip_logprob"])


def plain(graphs, labelled):
    return graphs if labelled else [{k: v for k, v in g.items() if k not in ("label", "L")} for g in graphs]


def num_labels(graphs, labelled):
    return max(g["L"] for g in graphs) if labelled else None


def outputs(ag, y, frames, rows, labelled):
    """the entries the issue names, as a flat list of CUDA tensors (nothing synchronised)"""
    out = list(ag.best_path(y, frames, rows, states=True))
    v, begin, res = ag.posteriors_compact(y, frames, rows)
    out += [v, torch.from_numpy(begin), res]
    if labelled:
        out += list(ag.best_path_labels(y, frames, rows, states=True))
        v, begin, res = ag.label_posteriors_compact(y, frames, rows)
        out += [v, torch.from_numpy(begin), res]
    return out


def nnet_output(n, T, seed):
    return dev(np.random.default_rng(seed).standard_normal((n * T, P)).astype(F)), [T] * n, (np.arange(n) * T).tolist()


NAMES = ["one-slot", "first-optional", "last-optional", "middle-optional", "alternating", "repeated-units", "700-slots", "256-and-257", "70-graphs"]


# ------------------------------------------------------------------------------------------------ bytes and outputs
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("labelled", [False, True], ids=["plain", "labelled"])
@pytest.mark.parametrize("context", [0, 1])
def test_compiled_tables_are_the_references_tables(abi, sets, context, labelled, name):
    s = sets[context]
    transcripts, graphs = s["transcripts"][name], plain(s["graphs"][name], labelled)
    units = unit_set(abi, s["us"])
    G, S, A = totals(graphs)
    L = num_labels(graphs, labelled)
    states, arcs = units.sizes(transcripts)  # tdnnf_transcript_graph_sizes: what the reserve is sized from
    assert states.tolist() == [g["S"] for g in graphs] and arcs.tolist() == [len(g["src"]) for g in graphs]
    assert context == 0 or name in ("one-slot", "last-optional") or S > G + sum(len(u) for u, _ in transcripts)  # B states
    compiled = abi.AlignGraphs.reserve(G, P, S, A, num_labels=L)  # exactly the batch: nothing may be written beyond it
    compiled.assign_transcripts(units, transcripts)
    assigned = abi.AlignGraphs.reserve(G, P, S, A, num_labels=L)
    assigned.assign(graphs)
    made = abi.AlignGraphs(graphs, num_pdfs=P, num_labels=L)
    same_tables(assigned, compiled)
    same_tables(made, compiled)
    assert compiled.G == made.G and compiled.num_states == made.num_states and np.array_equal(compiled.arc_begin, made.arc_begin)
    for k in range(0, G, 7):
        assert compiled.info(k) == made.info(k) and np.array_equal(compiled.pdfs(k), made.pdfs(k))
        assert not labelled or np.array_equal(compiled.labels(k), made.labels(k))


def test_a_larger_capacity_gives_the_same_tables(abi, sets):
    s = sets[1]
    graphs = s["graphs"]["70-graphs"]
    compiled = abi.AlignGraphs.reserve(90, P, 3000, 9000, num_labels=20)
    compiled.assign_transcripts(unit_set(abi, s["us"]), s["transcripts"]["70-graphs"])
    same_tables(abi.AlignGraphs(graphs, num_pdfs=P, num_labels=20), compiled)


@pytest.mark.parametrize("align_form", [0, 2])
@pytest.mark.parametrize("context", [0, 1])
def test_outputs_are_the_references_outputs(abi, sets, context, align_form):
    s = sets[context]
    transcripts = s["transcripts"]["70-graphs"][:12] + s["transcripts"]["first-optional"] + s["transcripts"]["last-optional"]
    graphs = s["graphs"]["70-graphs"][:12] + s["graphs"]["first-optional"] + s["graphs"]["last-optional"]
    G, S, A = totals(graphs)
    L = num_labels(graphs, True)
    y, frames, rows = nnet_output(G, 40, 5 + context)
    with abi.option("align_form", align_form):
        compiled = abi.AlignGraphs.reserve(G, P, S, A, num_labels=L)
        compiled.assign_transcripts(unit_set(abi, s["us"]), transcripts)
        assigned = abi.AlignGraphs.reserve(G, P, S, A, num_labels=L)
        assigned.assign(graphs)
        want, got = outputs(assigned, y, frames, rows, True), outputs(compiled, y, frames, rows, True)
        same_outputs(want, got)
    # every transcript has at most 12 mandatory slots: every utterance has a path, and its labels are its slots in order
    assert (got[2][:, 1] == 1).all() and (got[0] >= 0).all() and got[3].abs().sum() > 0
    labels = got[9].cpu().numpy().reshape(G, 40)
    assert (np.diff(labels, axis=1) >= 0).all() and all(labels[k, -1] >= len(transcripts[k][0]) - 2 for k in range(G))


# ------------------------------------------------------------------------------------------------ reuse, stream order, allocation
def test_reuse_stream_order_and_mixing(abi, sets):
    """one handle: a large batch, a small one, another large one, the first again -- compiled, and in between assigned from arrays; every
    call is enqueued without a synchronise, so a call in front of an assign must have read the batch before it"""
    s = sets[1]
    units = unit_set(abi, s["us"])
    order = ["70-graphs", "middle-optional", "256-and-257", "70-graphs"]
    cap = [max(v) for v in zip(*[totals(s["graphs"][n]) for n in order])]
    L = max(num_labels(s["graphs"][n], True) for n in order)
    res = abi.AlignGraphs.reserve(cap[0], P, cap[1], cap[2], num_labels=L)
    inputs = {n: nnet_output(len(s["graphs"][n]), 30 if n != "256-and-257" else 300, 20 + i) for i, n in enumerate(order)}
    want = {}
    for n in set(order):
        made = abi.AlignGraphs(s["graphs"][n], num_pdfs=P, num_labels=L)
        want[n] = outputs(made, *inputs[n], True)
    torch.cuda.synchronize()
    got = []
    for i, n in enumerate(order):
        if i == 2:  # from arrays in between: both kinds of assign on one handle
            res.assign(s["graphs"]["one-slot"])
        res.assign_transcripts(units, s["transcripts"][n])
        got.append(outputs(res, *inputs[n], True))
    for n, g in zip(order, got):
        same_outputs(want[n], g)
    same_tables(abi.AlignGraphs(s["graphs"][order[-1]], num_pdfs=P, num_labels=L), res)
    assert res.capacity()["assigns"] == 5
    res.assign(s["graphs"]["alternating"])
    same_tables(abi.AlignGraphs(s["graphs"]["alternating"], num_pdfs=P, num_labels=L), res)


def test_assign_transcripts_allocates_nothing(abi, sets):
    s = sets[0]
    units = unit_set(abi, s["us"])
    names = ["70-graphs", "alternating", "700-slots", "one-slot"]
    cap = [max(v) for v in zip(*[totals(s["graphs"][n]) for n in names])]
    res = abi.AlignGraphs.reserve(cap[0], P, cap[1], cap[2])
    before = res.capacity()
    assert before["assigns"] == 0 and before["device_allocs"] == 1
    free = torch.cuda.mem_get_info()[0]
    for i in range(20):
        res.assign_transcripts(units, s["transcripts"][names[i % 4]])
    after = res.capacity()
    assert after["assigns"] == 20 and {k: v for k, v in after.items() if k != "assigns"} == {k: v for k, v in before.items() if k != "assigns"}
    assert torch.cuda.mem_get_info()[0] == free  # the device agrees: nothing was allocated or freed
    same_tables(abi.AlignGraphs(plain(s["graphs"]["one-slot"], False), num_pdfs=P), res)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("context", [0, 1])
def test_refusals_keep_the_previous_batch(abi, sets, context):
    s = sets[context]
    units = unit_set(abi, s["us"])
    transcripts, graphs = s["transcripts"]["middle-optional"], s["graphs"]["middle-optional"]
    G, S, A = totals(graphs)
    L = num_labels(graphs, True)
    made = abi.AlignGraphs(graphs, num_pdfs=P, num_labels=L)
    y, frames, rows = nnet_output(G, 12, 31)
    want = outputs(made, y, frames, rows, True)
    who = "align_graphs_assign_transcripts: "

    def holds(res, labelled=True):
        assert res.G == G and res.capacity()["assigns"] == 1
        same_tables(made if labelled else abi.AlignGraphs(plain(graphs, False), num_pdfs=P), res)
        if labelled:
            same_outputs(want, outputs(res, y, frames, rows, True))

    res = abi.AlignGraphs.reserve(G + 1, P, S + 30, A + 90, num_labels=L)
    res.assign_transcripts(units, transcripts)
    good = transcripts[0]
    for bad, words in ((tr([1, U, 2], [0, 0, 0]), ("transcript 1 slot 1", "unit %d outside [0, %d)" % (U, U))),
                       (tr([1, 2, -1], [0, 0, 0]), ("transcript 1 slot 2", "unit -1 outside")),
                       (tr([1, 2, 3, 4], [0, 1, 1, 0]), ("transcript 1 slot 2", "adjacent optional")),
                       (tr([5], [1]), ("transcript 1 slot 0", "no mandatory slot"))):
        refused(abi, lambda: res.assign_transcripts(units, [good, bad]), who, *words)
        refused(abi, lambda: units.sizes([good, bad]), "transcript_graph_sizes: ", *words)  # the same message under its own name
        holds(res)
    # num_labels smaller than the slot count
    refused(abi, lambda: res.assign_transcripts(units, [tr(np.arange(L + 1) % U, np.zeros(L + 1))]), who, "num_labels = %d" % L, "short by 1")
    holds(res)
    # each of the three capacities exceeded by exactly 1: a handle that holds the batch, sized for one more transcript but for one kind
    over = transcripts + [tr([1], [0])]
    states, arcs = units.sizes(over)
    for short, word in enumerate(("max_graphs", "max_states", "max_arcs")):
        cap = [len(over), int(states.sum()), int(arcs.sum())]
        cap[short] -= 1
        tight = abi.AlignGraphs.reserve(cap[0], P, cap[1], cap[2], num_labels=L)
        tight.assign_transcripts(units, transcripts)
        refused(abi, lambda: tight.assign_transcripts(units, over), who, word, "by 1")
        holds(tight)
    # the unit set's num_pdfs against the handle's
    us = dict(s["us"], P=P + 1)
    refused(abi, lambda: res.assign_transcripts(unit_set(abi, us), transcripts), who, "%d pdfs" % (P + 1), "num_pdfs %d" % P)
    holds(res)
    # labels against the reservation: a transcript batch always fits (the labels are the slots), an assign from arrays must still match
    refused(abi, lambda: res.assign(plain(graphs, False)), "align_graphs_assign", "arc_label is null")
    holds(res)
    unlabelled = abi.AlignGraphs.reserve(G, P, S, A)
    unlabelled.assign_transcripts(units, transcripts)
    refused(abi, lambda: unlabelled.assign(graphs), "align_graphs_assign", "without labels")
    holds(unlabelled, labelled=False)
    # a created handle
    refused(abi, lambda: made.assign_transcripts(units, transcripts), who, "tdnnf_align_graphs_create")
    same_outputs(want, outputs(made, y, frames, rows, True))


def test_unit_set_refusals(abi, sets):
    us = sets[1]["us"]
    bad = dict(us, entry_pdf=np.where(np.arange(us["entry_pdf"].size).reshape(us["entry_pdf"].shape) == 9, P, us["entry_pdf"]))
    refused(abi, lambda: unit_set(abi, bad), "unit_set_create: ", "entry_pdf[9] is %d, outside [0, %d)" % (P, P))
    bad = dict(us, loop_pdf=np.where(np.arange(us["loop_pdf"].size).reshape(us["loop_pdf"].shape) == 3, -1, us["loop_pdf"]))
    refused(abi, lambda: unit_set(abi, bad), "unit_set_create: ", "loop_pdf[3] is -1")
    with pytest.raises(abi.HipAbiError, match=r"\(U,\) or \(U \+ 1, U\)"):
        abi.UnitSet(np.zeros((3, 3), np.int32), np.zeros((3, 3), np.int32), np.zeros(3, F), np.zeros(3, F), 4)


# ------------------------------------------------------------------------------------------------ the end-to-end supervision
@pytest.mark.parametrize("context", [0, 1])
def test_e2e_supervision_from_transcripts(pkg, abi, context):
    """one reserved supervision, two minibatches that differ in sequences, frames and graphs: the chain objective and its derivatives from
    transcripts have the bits of the same calls after assign with the reference's graphs"""
    hip = Hip(pkg)
    synth = pkg.synth
    Pd = 41
    us = synth.make_unit_set(5, context=context, seed=3, distinct=False, P=Pd)
    units = unit_set(abi, us)
    den = abi.DenGraph(synth.make_den_graph(30, Pd, mean_out_degree=4.0, seed=5))
    minibatches = [(3, 12, 1.0, synth.make_transcripts(3, 5, slots=(2, 7), optional_rate=0.4, seed=40)),
                   (5, 9, 0.75, synth.make_transcripts(5, 5, slots=(1, 6), optional_rate=0.4, seed=41))]
    hopeless = [tr(np.arange(11) % 5, np.zeros(11))] + minibatches[1][3][1:]  # 11 mandatory slots, 9 frames: no path of that length
    minibatches.append((5, 9, 0.75, hopeless))
    graphs = [[ref.transcript_graph(us, u, o) for u, o in m[3]] for m in minibatches]
    cap = (5, 12, max(totals(g)[1] for g in graphs), max(totals(g)[2] for g in graphs))
    compiled = abi.Supervision.reserve_e2e(cap[0], cap[1], Pd, cap[2], cap[3])
    assigned = abi.Supervision.reserve_e2e(cap[0], cap[1], Pd, cap[2], cap[3])
    for i, ((B, T, w, transcripts), gs) in enumerate(zip(minibatches, graphs)):
        rng = np.random.default_rng(50 + i)
        y = dev((1.5 * rng.standard_normal((B * T, Pd))).astype(F))
        xo = rng.standard_normal((B * T, Pd))
        xo = dev((xo - np.log(np.exp(xo).sum(1, keepdims=True))).astype(F))
        compiled.assign_transcripts(units, transcripts, T, weight=w)
        assigned.assign(plain(gs, False), T, weight=w)
        assert compiled.e2e_form() == assigned.e2e_form() and compiled.info() == assigned.info() and (compiled.B, compiled.T) == (B, T)
        want, got = run(hip, den, assigned, y, xo), run(hip, den, compiled, y, xo)
        same_bits(want, got)
        if i < 2:
            assert want[0][5] == 1.0 and np.isfinite(want[0][:7]).all() and np.abs(want[1]).sum() > 0
        else:  # the objective's failure path
            assert want[0][5] == 0.0
    # refusals leave the minibatch: too many sequences, too many frames, a bad slot, a created supervision
    who = "supervision_assign_e2e_transcripts: "
    last = minibatches[2][3]
    refused(abi, lambda: compiled.assign_transcripts(units, last + [tr([1], [0])], 9), who, "max_sequences", "by 1")
    refused(abi, lambda: compiled.assign_transcripts(units, last, 13), who, "max_frames", "by 1")
    refused(abi, lambda: compiled.assign_transcripts(units, [tr([1, 2], [1, 1])] + last[1:], 9), who, "transcript 0 slot 1", "adjacent optional")
    refused(abi, lambda: compiled.assign_transcripts(units, [tr(np.arange(60) % 5, np.zeros(60))] * 5, 9), "max_states")
    assert (compiled.B, compiled.T) == (5, 9) and compiled.info() == assigned.info()
    same_bits(want, run(hip, den, compiled, y, xo))
    made = abi.Supervision.from_graphs(plain(graphs[0], False), 12, num_pdfs=Pd)
    refused(abi, lambda: made.assign_transcripts(units, minibatches[0][3], 12), who, "tdnnf_supervision_reserve_e2e")
