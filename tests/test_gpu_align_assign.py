"""-m gpu: reusable graph sets (tdnnf_align_graphs_reserve / _assign; include/tdnnf_hip.h "A REUSABLE graph set").  A reserved handle is
assigned batches whose tables the device builds (csrc/align_build_kernels.h); the specification is the host build of
tdnnf_align_graphs_create: every device array of the assigned handle equals the created handle's BYTE FOR BYTE (AlignGraphs.tables), and
since the kernels that read them are the same, every entry gives the same bits (torch.equal).  No tolerance anywhere.

Shapes: the edges of the tables -- rows of 0 / 1 / 63 / 64 / 65 arcs (65: a heavy row), 1 / 63 / 64 / 65 / 129 rows (one slice, a full
one, one row into the next, three), the staircase 64 .. 0 (the arc padding at its bound), rows of equal length (ties of the stable order),
many one-state graphs, one pdf on 300 arcs, 6034 pdfs of which three occur, labels per unit and per arc and a labelling that splits and
merges pdfs, one graph and as many as the capacity, and a 2 000-state denominator-like graph (more than one chunk of 256 rows and arcs
per workgroup, many fill parts).  At most 23 frames and a few hundred pdfs, but for the stated exceptions."""
import numpy as np
import pytest
import torch

from tests.gpu_util import dev

pytestmark = pytest.mark.gpu
F = np.float32
NINF = -np.inf


@pytest.fixture(scope="module")
def abi(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pkg.hipabi


# ------------------------------------------------------------------------------------------------ graphs
def graph(S, src, dst, pdf, P, seed, label=None):
    """a graph dict on the given arcs, in a shuffled order (the caller's order is no sorted order); state 0 initial, the last state final"""
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(src))
    init, final = np.full(S, NINF, F), np.full(S, NINF, F)
    init[0], final[S - 1] = 0.0, 0.0
    g = dict(S=S, P=P, src=np.asarray(src, np.int32)[order], dst=np.asarray(dst, np.int32)[order], pdf=np.asarray(pdf, np.int32)[order],
             logprob=(-rng.random(len(src))).astype(F), init=init, final=final)
    if label is not None:
        g["label"] = np.asarray(label, np.int32)[order]
        g["L"] = int(max(label) + 1) if len(label) else 1
    return g


def in_degrees(lengths, P, seed):
    """state i has lengths[i] incoming arcs, from sources that go round the states"""
    S = len(lengths)
    dst = np.repeat(np.arange(S), lengths)
    src = np.arange(len(dst)) * 7 % S
    return graph(S, src, dst, np.random.default_rng(seed).integers(0, P, len(dst)), P, seed)


def chain(S, P, seed, pdf=None):
    """S states, each with its loop and an arc to the next: rows of equal length by destination and by source"""
    st = np.arange(S)
    src, dst = np.concatenate([st, st[:-1]]), np.concatenate([st, st[1:]])
    return graph(S, src, dst, np.random.default_rng(seed).integers(0, P, len(src)) if pdf is None else pdf(len(src)), P, seed)


def relabelled(g, label):
    g = dict(g)
    g["label"] = np.asarray(label(g), np.int32)
    g["L"] = int(g["label"].max()) + 1
    return g


def transcript(synth, n, P, seed, labels=None):
    rng = np.random.default_rng(seed)
    return synth.make_alignment_graph(rng.integers(0, P, n), optional=(1,) if n > 2 else (), alternatives={0: [int(rng.integers(0, P))]}, seed=seed,
                                      num_pdfs=P, labels=labels)


def cases(synth):
    """{name: (graphs, num_pdfs)}"""
    P = 40
    den = synth.alignment_graph_from_den(synth.make_den_graph(2000, 300, seed=3))
    c = {
        "row-lengths": ([in_degrees([0, 1, 63, 64, 65, 2], P, 1)], P),
        "row-counts": ([chain(S, P, 10 + S) for S in (1, 63, 64, 65, 129)], P),
        "staircase": ([in_degrees(list(range(64, -1, -1)), P, 2)], P),
        "one-state-graphs": ([in_degrees([k % 3], P, 20 + k) for k in range(70)], P),
        "equal-rows": ([chain(200, P, 4)], P),
        "heavy-pdf": ([chain(151, P, 5, pdf=lambda n: np.where(np.arange(n) < 300, 7, 1 + np.arange(n) % 5))], P),
        "in-degree-65": ([in_degrees([65, 3, 0, 64], P, 6), chain(5, P, 7)], P),
        "6034-pdfs": ([chain(90, 6034, 8, pdf=lambda n: np.asarray([5, 3001, 6033])[np.arange(n) % 3])], 6034),
        "labels-unit": ([transcript(synth, n, P, 30 + n, "unit") for n in (3, 9, 1)], P),
        "labels-arc": ([transcript(synth, n, P, 40 + n, "arc") for n in (4, 7)], P),
        # pdf p's arcs alternate between labels 2 (p // 3) and 2 (p // 3) + 1: every pdf is split over two labels, three pdfs share each
        "labels-split-merge": ([relabelled(chain(70, P, 9), lambda g: 2 * (g["pdf"] // 3) + np.arange(len(g["pdf"])) % 2),
                                relabelled(in_degrees([66, 1, 0, 5], P, 11), lambda g: g["pdf"] % 2)], P),
        "one-graph": ([transcript(synth, 6, P, 50)], P),
        "den-2000": ([den], 300),
    }
    assert len(den["src"]) > 20000 and max(np.bincount(den["pdf"])) > 64
    return c


@pytest.fixture(scope="module")
def sets(pkg):
    return cases(pkg.synth)


def totals(graphs):
    return len(graphs), sum(g["S"] for g in graphs), sum(len(g["src"]) for g in graphs)


def num_labels(graphs):
    return max(g["L"] for g in graphs) if "label" in graphs[0] else None


def pair(abi, graphs, P, capacity=None):
    """(created, reserved at `capacity` -- default exactly the batch -- and assigned)"""
    L = num_labels(graphs)
    made = abi.AlignGraphs(graphs, num_pdfs=P, num_labels=L)
    G, S, A = capacity or totals(graphs)
    res = abi.AlignGraphs.reserve(G, P, S, A, num_labels=L)
    res.assign(graphs)
    return made, res


def same_tables(a, b):
    ta, tb = a.tables(), b.tables()
    assert sorted(ta) == sorted(tb)
    for k in ta:
        if isinstance(ta[k], dict):
            for w in ta[k]:
                assert ta[k][w].shape == tb[k][w].shape and np.array_equal(ta[k][w], tb[k][w]), (k, w)
        else:
            assert ta[k].shape == tb[k].shape and np.array_equal(ta[k], tb[k]), k


def frames_for(graphs, seed):
    """a few frames per graph, long enough for an accepting path where the graph is a chain"""
    rng = np.random.default_rng(seed)
    return [int(min(23, max(g["S"] - 1, 1) + rng.integers(0, 4))) if g["S"] <= 20 else int(rng.integers(5, 24)) for g in graphs]


def outputs(ag, y, frames, rows, labelled, checkpoint=None, path_checkpoint=None):
    """every entry's outputs on the handle, as a flat list of CUDA tensors (nothing synchronised)"""
    out = list(t for t in ag.best_path(y, frames, rows, states=True, checkpoint=path_checkpoint))
    out += [ag.logprob(y, frames, rows)]
    out += list(ag.posteriors(y, frames, rows, weight=0.5, checkpoint=checkpoint))
    v, begin, res = ag.posteriors_compact(y, frames, rows, checkpoint=checkpoint)
    out += [v, torch.from_numpy(begin), res]
    out += list(ag.posteriors_sparse(y, frames, rows, min_post=0.05, max_per_frame=4, checkpoint=checkpoint))
    if labelled:
        out += list(ag.best_path_labels(y, frames, rows, states=True, checkpoint=path_checkpoint))
        v, begin, res = ag.label_posteriors_compact(y, frames, rows, checkpoint=checkpoint)
        out += [v, torch.from_numpy(begin), res]
        out += list(ag.label_posteriors_sparse(y, frames, rows, min_post=0.05, max_per_frame=4, checkpoint=checkpoint))
    return out


def same_outputs(a, b):
    assert len(a) == len(b)
    torch.cuda.synchronize()
    for i, (x, z) in enumerate(zip(a, b)):
        if x.dtype.is_floating_point:  # the bit patterns: a NaN equals itself, -0 is not 0
            x, z = x.contiguous().view(torch.int64 if x.dtype == torch.float64 else torch.int32), z.contiguous().view(torch.int64 if z.dtype == torch.float64 else torch.int32)
        assert x.shape == z.shape and torch.equal(x.cpu(), z.cpu()), i


def nnet_output(graphs, P, frames, seed):
    rows = np.concatenate([[0], np.cumsum(frames)[:-1]])
    return dev(np.random.default_rng(seed).standard_normal((sum(frames), P)).astype(F)), rows


NAMES = ["row-lengths", "row-counts", "staircase", "one-state-graphs", "equal-rows", "heavy-pdf", "in-degree-65", "6034-pdfs", "labels-unit",
         "labels-arc", "labels-split-merge", "one-graph", "den-2000"]


# ------------------------------------------------------------------------------------------------ bytes and outputs
@pytest.mark.parametrize("name", NAMES)
def test_assigned_tables_are_the_created_tables(abi, sets, name):
    graphs, P = sets[name]
    made, res = pair(abi, graphs, P)  # G = capacity, and for "one-graph" and "den-2000" G = 1
    same_tables(made, res)
    assert res.G == made.G and res.num_states == made.num_states and res.L == made.L and np.array_equal(res.arc_begin, made.arc_begin)
    for k in range(made.G):
        assert res.info(k) == made.info(k) and np.array_equal(res.pdfs(k), made.pdfs(k))
        assert not made.L or np.array_equal(res.labels(k), made.labels(k))


def test_a_larger_capacity_gives_the_same_tables(abi, sets):
    graphs, P = sets["in-degree-65"]
    made, res = pair(abi, graphs, P, capacity=(9, 500, 4000))
    same_tables(made, res)


@pytest.mark.parametrize("name", [n for n in NAMES if n != "den-2000"])
def test_assigned_outputs_are_the_created_outputs(abi, sets, name):
    graphs, P = sets[name]
    made, res = pair(abi, graphs, P)
    frames = frames_for(graphs, 1)
    y, rows = nnet_output(graphs, P, frames, 2)
    want, got = outputs(made, y, frames, rows, bool(made.L)), outputs(res, y, frames, rows, bool(made.L))
    same_outputs(want, got)
    if name in ("labels-unit", "labels-arc", "one-graph"):  # transcripts: every utterance has a path, so the equal outputs are not all "no path"
        assert (got[2][:, 1] == 1).all() and (got[0] >= 0).all() and got[4].abs().sum() > 0


def test_outputs_on_the_large_graph(abi, sets):
    graphs, P = sets["den-2000"]
    made, res = pair(abi, graphs, P)
    frames = [9]
    y, rows = nnet_output(graphs, P, frames, 3)
    same_outputs(outputs(made, y, frames, rows, False), outputs(res, y, frames, rows, False))


@pytest.mark.parametrize("how", ["path-checkpoint", "checkpoint", "align_form-2"])
def test_outputs_under_the_options(abi, sets, how):
    graphs, P = sets["labels-split-merge"]
    made, res = pair(abi, graphs, P)
    frames = [23, 17]
    y, rows = nnet_output(graphs, P, frames, 4)
    kw = {"path-checkpoint": dict(path_checkpoint=3), "checkpoint": dict(checkpoint=3), "align_form-2": {}}[how]
    if how == "align_form-2":
        with abi.option("align_form", 2):
            a, b = outputs(made, y, frames, rows, True), outputs(res, y, frames, rows, True)
    else:
        a, b = outputs(made, y, frames, rows, True, **kw), outputs(res, y, frames, rows, True, **kw)
    same_outputs(a, b)


# ------------------------------------------------------------------------------------------------ reuse, stream order, allocation
def test_reuse_large_small_large_and_back(abi, sets):
    """one handle: a large batch, a smaller one (fewer graphs, states and arcs), a differently shaped large one, the first again"""
    P = 40
    large, small, other = sets["row-counts"][0], sets["in-degree-65"][0], sets["one-state-graphs"][0] + sets["staircase"][0]
    cap = [max(v) for v in zip(totals(large), totals(small), totals(other))]
    assert totals(small) < totals(large)
    res = abi.AlignGraphs.reserve(cap[0], P, cap[1], cap[2])
    for graphs in (large, small, other, large):
        res.assign(graphs)
        made = abi.AlignGraphs(graphs, num_pdfs=P)
        same_tables(made, res)  # (the dump has the new batch's counts: nothing of the batch before shows)
        frames = frames_for(graphs, 5)
        y, rows = nnet_output(graphs, P, frames, 6)
        same_outputs(outputs(made, y, frames, rows, False), outputs(res, y, frames, rows, False))
    assert res.capacity()["assigns"] == 4


def test_stream_order(abi, sets):
    """calls on batch A, then assign B and calls, nothing synchronised in between: A's outputs are A's, B's are B's"""
    P = 40
    A, B = sets["row-counts"][0], sets["in-degree-65"][0]
    fa, fb = frames_for(A, 7), frames_for(B, 8)
    (ya, ra), (yb, rb) = nnet_output(A, P, fa, 9), nnet_output(B, P, fb, 10)
    want_a = outputs(abi.AlignGraphs(A, num_pdfs=P), ya, fa, ra, False)
    want_b = outputs(abi.AlignGraphs(B, num_pdfs=P), yb, fb, rb, False)
    cap = [max(v) for v in zip(totals(A), totals(B))]
    res = abi.AlignGraphs.reserve(cap[0], P, cap[1], cap[2])
    torch.cuda.synchronize()
    res.assign(A)
    got_a = outputs(res, ya, fa, ra, False)
    res.assign(B)
    got_b = outputs(res, yb, fb, rb, False)
    res.assign(A)
    got_a2 = outputs(res, ya, fa, ra, False)
    same_outputs(want_a, got_a)
    same_outputs(want_b, got_b)
    same_outputs(want_a, got_a2)


def test_assign_allocates_nothing(abi, sets):
    P = 40
    batches = [sets[n][0] for n in ("row-counts", "in-degree-65", "staircase", "equal-rows")]
    cap = [max(v) for v in zip(*[totals(b) for b in batches])]
    res = abi.AlignGraphs.reserve(cap[0], P, cap[1], cap[2])
    before = res.capacity()
    assert before["assigns"] == 0 and before["device_allocs"] >= 1 and before["device_bytes"] > 48 * cap[2]
    assert (before["max_graphs"], before["max_states"], before["max_arcs"]) == tuple(cap)
    free = torch.cuda.mem_get_info()[0]
    for i in range(20):
        res.assign(batches[i % 4])
    after = res.capacity()
    assert after["assigns"] == 20 and {k: v for k, v in after.items() if k != "assigns"} == {k: v for k, v in before.items() if k != "assigns"}
    assert torch.cuda.mem_get_info()[0] == free  # the device agrees: nothing was allocated or freed
    same_tables(abi.AlignGraphs(batches[3], num_pdfs=P), res)


# ------------------------------------------------------------------------------------------------ refusals
def refused(abi, call, *words):
    with pytest.raises(abi.HipAbiError) as e:
        call()
    msg = str(e.value)
    assert "tdnnf error 1:" in msg, msg  # TDNNF_EINVAL
    for w in words:
        assert w in msg, (w, msg)


def test_capacity_refusals_keep_the_previous_batch(abi, sets):
    P = 40
    graphs = sets["in-degree-65"][0]
    G, S, A = totals(graphs)
    made = abi.AlignGraphs(graphs, num_pdfs=P)
    frames = frames_for(graphs, 11)
    y, rows = nnet_output(graphs, P, frames, 12)
    want = outputs(made, y, frames, rows, False)
    for short, word in enumerate(("max_graphs", "max_states", "max_arcs")):
        cap = [G + 1, S + 1, A + 1]
        res = abi.AlignGraphs.reserve(cap[0], P, cap[1], cap[2])
        res.assign(graphs)
        # one more than the capacity of exactly one kind
        n = [cap[0], 1, 1]
        if short == 0:
            over = [chain(1, P, k) for k in range(cap[0] + 1)]
        elif short == 1:
            over = [in_degrees([0] * (cap[1] + 1), P, 1)]
        else:
            over = [in_degrees([cap[2] + 1 - 64, 64], P, 1)]
        t = totals(over)
        assert [t[i] > cap[i] for i in range(3)] == [i == short for i in range(3)] and t[short] == cap[short] + 1
        refused(abi, lambda: res.assign(over), "align_graphs_assign", word, "by 1")
        assert res.G == G and res.capacity()["assigns"] == 1
        same_tables(made, res)
        same_outputs(want, outputs(res, y, frames, rows, False))


def test_other_refusals(abi, sets):
    P = 40
    graphs = sets["in-degree-65"][0]
    G, S, A = totals(graphs)
    made = abi.AlignGraphs(graphs, num_pdfs=P)
    lib = abi.load()
    k = made._keep
    assert lib.tdnnf_align_graphs_assign(made.h, made.G, *[x[1] for x in k[:8]], None, None) == 1  # TDNNF_EINVAL
    assert b"align_graphs_assign" in lib.tdnnf_last_error() and b"tdnnf_align_graphs_create" in lib.tdnnf_last_error()
    refused(abi, made.capacity, "align_graphs_capacity")

    # a reserved handle that was never assigned: every entry says so
    res = abi.AlignGraphs.reserve(G, P, S, A)
    lres = abi.AlignGraphs.reserve(G, P, S, A, num_labels=3)
    y = dev(np.zeros((8, P), F))
    empty = "holds no graphs yet"
    for call in (lambda: res.info(0), lambda: res.pdfs(0), lambda: lres.labels(0), res.tables, lambda: res.best_path(y, [4], [0], utt_graph=[0]),
                 lambda: res.logprob(y, [4], [0], utt_graph=[0]), lambda: res.posteriors(y, [4], [0], utt_graph=[0]),
                 lambda: res.posteriors_compact(y, [4], [0], utt_graph=[0]), lambda: res.posteriors_sparse(y, [4], [0], utt_graph=[0]),
                 lambda: res.posteriors_compact_layout([4], utt_graph=[0]), lambda: lres.best_path_labels(y, [4], [0], utt_graph=[0]),
                 lambda: lres.label_posteriors_compact(y, [4], [0], utt_graph=[0]), lambda: lres.label_posteriors_sparse(y, [4], [0], utt_graph=[0])):
        with pytest.raises(abi.HipAbiError, match=empty):
            call()
    assert res.workspace_bytes([0], [4]) == 0 and empty.encode() in lib.tdnnf_last_error()

    # labels against the reservation
    labelled = [relabelled(g, lambda g: g["pdf"] % 3) for g in graphs]
    refused(abi, lambda: res.assign(labelled), "align_graphs_assign", "arc_label", "without labels")
    refused(abi, lambda: lres.assign(graphs), "align_graphs_assign", "arc_label is null")
    refused(abi, lambda: lres.assign([relabelled(g, lambda g: g["pdf"] % 3 + 1) for g in graphs]), "align_graphs_assign", "label 3 outside [0, 3)")
    lres.assign(labelled)
    same_tables(abi.AlignGraphs(labelled, num_pdfs=P, num_labels=3), lres)

    # create's refusals under the new call's name; the handle keeps its batch
    res.assign(graphs)

    def broken(**change):
        g = dict(graphs[1])
        for key, fn in change.items():
            g[key] = fn(np.array(g[key]))
        return [graphs[0], g]

    def put(i, v):
        def f(a):
            a[i] = v
            return a
        return f

    refused(abi, lambda: res.assign(broken(pdf=put(2, P))), "align_graphs_assign: arc", "carries pdf %d outside [0, %d) (epsilon arcs are not supported)" % (P, P))
    refused(abi, lambda: res.assign(broken(pdf=put(0, -1))), "align_graphs_assign: arc", "epsilon arcs are not supported")
    refused(abi, lambda: res.assign(broken(dst=put(1, 5))), "align_graphs_assign: arc", "leaves graph 1's states")
    refused(abi, lambda: res.assign(broken(init=lambda a: np.full_like(a, NINF))), "align_graphs_assign: graph 1 has no initial state")
    refused(abi, lambda: res.assign(broken(final=lambda a: np.full_like(a, NINF))), "align_graphs_assign: graph 1 has no final state")
    assert res.capacity()["assigns"] == 1 and res.G == G
    same_tables(made, res)


def test_refusals_take_no_turn_of_the_staging_and_both_assigns_share_it(pkg, abi, sets):
    """one labelled handle, three rounds of: assign A and a best path, a refused assign, assign_transcripts B and a best path, a refused
    assign_transcripts, assign A and a best path -- nothing synchronised, nothing read until the end.  Three assigns a round: the two pinned
    staging buffers change hands with every assign that succeeds, of either kind, and with none that is refused, or a buffer would be
    written again while its copies are still to run and some output below would be another batch's"""
    from tests import transcript_graphs_ref as ref
    P, U = 40, 6
    A = sets["labels-unit"][0]
    us = pkg.synth.make_unit_set(U, context=1, seed=5, distinct=False, P=P)
    units = abi.UnitSet(us["entry_pdf"], us["loop_pdf"], us["loop_logprob"], us["leave_logprob"], us["P"], us["take_logprob"], us["skip_logprob"])
    transcripts = [(np.asarray([1, 2, 3], np.int32), np.asarray([0, 1, 0], np.int32)), (np.asarray([4, 5], np.int32), np.asarray([1, 0], np.int32))]
    B = [ref.transcript_graph(us, u, o) for u, o in transcripts]
    L = max(num_labels(A), num_labels(B))
    cap = [max(v) for v in zip(totals(A), totals(B))]
    one_arc_over = [relabelled(in_degrees([cap[2] + 1, 0], P, 1), lambda g: g["pdf"] % L)]
    assert totals(one_arc_over) == (1, 2, cap[2] + 1) and cap[1] >= 2
    one_slot_over = [(np.arange(L + 1, dtype=np.int32) % U, np.zeros(L + 1, np.int32))]
    fa, fb = frames_for(A, 13), [12, 12]
    (ya, ra), (yb, rb) = nnet_output(A, P, fa, 14), nnet_output(B, P, fb, 15)

    def paths(ag, y, frames, rows):
        return list(ag.best_path(y, frames, rows, states=True)) + list(ag.best_path_labels(y, frames, rows, states=True))

    want_a = paths(abi.AlignGraphs(A, num_pdfs=P, num_labels=L), ya, fa, ra)
    want_b = paths(abi.AlignGraphs(B, num_pdfs=P, num_labels=L), yb, fb, rb)
    res = abi.AlignGraphs.reserve(cap[0], P, cap[1], cap[2], num_labels=L)
    torch.cuda.synchronize()
    got = []
    for _ in range(3):
        res.assign(A)
        got.append((want_a, paths(res, ya, fa, ra)))
        refused(abi, lambda: res.assign(one_arc_over), "align_graphs_assign: ", "max_arcs", "by 1")
        res.assign_transcripts(units, transcripts)
        got.append((want_b, paths(res, yb, fb, rb)))
        refused(abi, lambda: res.assign_transcripts(units, one_slot_over), "align_graphs_assign_transcripts: ", "num_labels = %d" % L, "short by 1")
        res.assign(A)
        got.append((want_a, paths(res, ya, fa, ra)))
    for want, have in got:
        same_outputs(want, have)
    assert (want_a[2][:, 1] == 1).all() and (want_b[2][:, 1] == 1).all()  # every utterance has a path: the equal outputs are not all "no path"
    assert res.capacity()["assigns"] == 9 and res.capacity()["device_allocs"] == 1
