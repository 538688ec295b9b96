"""-m gpu: labelled alignment graphs (tdnnf_align_graphs_create_labelled; include/tdnnf_hip.h "best-path alignment" and "label posteriors"):
the labelled best path, the compact posteriors per label and their sparse form, on the shapes of tests/test_gpu_posteriors_compact.py --
the same boundaries decide the launch form -- and on labellings that make the by-label rows what the by-pdf rows never are.

Bars.  The label compact call runs the pdf compact call's row walk on a fourth arc table, so with label = pdf (the identity labelling) its
block equals tdnnf_align_posteriors_compact's BIT FOR BIT, and so do logprob and ok.  Every other labelling is held to the float64
reference tests/label_posteriors_ref64.py at the bars of tests/test_gpu_posteriors.py (its _close): logprob 1e-9 relative, values one
float32 ulp at `weight`, rows summing to weight.  The best path's arcs and labels equal tests/viterbi_ref64.py's exactly; the sparse form
equals tests/posteriors_sparse_ref.sparsify of the label compact block exactly.  Between two calls, between layouts and between a labelled
and an unlabelled handle of the same graphs results are compared bit for bit.
Every output lies between canaries and is pre-filled with a sentinel no result can be: the canaries must survive and no sentinel may."""
import struct

import numpy as np
import pytest
import torch

from tests import label_posteriors_ref64 as LR
from tests import viterbi_ref64 as V
from tests.gpu_util import Hip, dev, host
from tests.posteriors_sparse_ref import sparsify
from tests.test_gpu_posteriors import _close, _same_bits
from tests.test_gpu_posteriors_compact import _compact_raw, _labelled

pytestmark = pytest.mark.gpu
F = np.float32
NINF = -np.inf
ULP = 2.0 ** -23
GUARD, CANARY, SENTINEL = 16, 123, -7


@pytest.fixture(scope="module")
def hip(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return Hip(pkg)


def _guarded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
    buf[:GUARD] = CANARY
    buf[GUARD + n:] = CANARY
    return buf


def _inner(buf, n, what, written=True):
    b = host(buf)
    assert (b[:GUARD] == CANARY).all() and (b[GUARD + n:] == CANARY).all(), "the call wrote outside its " + what
    assert not written or not (b[GUARD:GUARD + n] == SENTINEL).any(), "an element of the " + what + " was not written"
    return b[GUARD:GUARD + n]


def _args(pkg, frames, rows, utt_graph):
    abi = pkg.hipabi
    return len(frames), abi.iarr(frames), abi.iarr(rows), abi.iarr(utt_graph) if utt_graph is not None else (None, None)


def _graph_of(ag, utt_graph, u):
    return utt_graph[u] if utt_graph is not None else (0 if ag.G == 1 else u)


def _stack(ys, P):
    frames = [len(y) for y in ys]
    rows = np.concatenate([[0], np.cumsum(frames)[:-1]])
    return dev(np.concatenate(ys) if sum(frames) else np.zeros((1, P), F)), frames, rows


def _label_raw(pkg, ag, y, frames, rows, stride, utt_graph, scale=1.0, weight=1.0):
    """tdnnf_align_label_posteriors_compact on a guarded buffer: (values [elems], utt_begin, results [U, 2]), downloaded"""
    abi, lib = pkg.hipabi, pkg.hipabi.load()
    n, fr, rb, ug = _args(pkg, frames, rows, utt_graph)
    begin = ag.label_posteriors_compact_layout(frames, utt_graph)
    elems = int(begin[-1])
    buf = _guarded(elems, torch.float32)
    nbytes = ag.posteriors_workspace_bytes(utt_graph, frames)  # the pdf call's workspace, unchanged
    assert nbytes > 0
    ws = abi.workspace(nbytes)
    res = torch.full((n, 2), -5.0, dtype=torch.float64, device="cuda")
    abi.check(lib.tdnnf_align_label_posteriors_compact(ag.h, n, ug[1], fr[1], rb[1], int(stride), abi.pmat(y), float(scale), float(weight),
                                                       abi.ptr(buf[GUARD:]), elems, abi.ptr(res), abi.ptr(ws), nbytes, abi.stream()))
    return _inner(buf, elems, "blocks"), begin, host(res)


def _per_utt(ag, vals, begin, res, frames, utt_graph):
    return [(res[u, 0], res[u, 1], vals[begin[u]:begin[u + 1]].reshape(T, len(ag.labels(_graph_of(ag, utt_graph, u))))) for u, T in enumerate(frames)]


def _check_ref(pkg, graphs, ys, utt_graph=None, scale=1.0, weight=1.0, ag=None):
    """the label compact call on stacked rows against the float64 reference; returns (per utterance (logprob, ok, block), references)"""
    graphs = [graphs] if isinstance(graphs, dict) else graphs
    ag = ag or pkg.hipabi.AlignGraphs(graphs, num_labels=max(g["L"] for g in graphs))
    y, frames, rows = _stack(ys, ag.P)
    vals, begin, res = _label_raw(pkg, ag, y, frames, rows, 1, utt_graph, scale, weight)
    got, refs = _per_utt(ag, vals, begin, res, frames, utt_graph), []
    for u, T in enumerate(frames):
        g = graphs[_graph_of(ag, utt_graph, u)]
        refs.append(LR.label_posteriors(g, g["label"], ys[u], scale))
        assert ag.labels(_graph_of(ag, utt_graph, u)).tolist() == refs[u]["labels"].tolist() and begin[u + 1] - begin[u] == T * len(refs[u]["labels"])
        _close(got[u], refs[u], weight, "utterance %d" % u)
    return got, refs


# ------------------------------------------------------------------------------------------------------------------------- shapes
def _cyclic(pkg, S, P=50):
    return pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(S, P, mean_out_degree=4.0, seed=S))


def _heavy(pkg):
    """one pdf on 300 arcs (a heavy by-pdf row), one on exactly 64, light ones beside them"""
    return _labelled(50, np.concatenate([np.full(300, 9), np.full(64, 4), np.full(3, 2), np.full(20, 11), np.full(1, 30)]), 300)


# name: (graph, align_form, frames of the two utterances); the thread counts change at 64 / 65 and 1024 / 1025 states
SHAPES = {"S64": (lambda pkg: _cyclic(pkg, 64), 0), "S65": (lambda pkg: _cyclic(pkg, 65), 0), "S1024": (lambda pkg: _cyclic(pkg, 1024), 0),
          "S1025": (lambda pkg: _cyclic(pkg, 1025), 0), "S65-workspace": (lambda pkg: _cyclic(pkg, 65), 2),
          "S40-P600-rows-not-staged": (lambda pkg: _cyclic(pkg, 40, 600), 0), "heavy-row": (_heavy, 0)}


def _shape(pkg, name):
    g = SHAPES[name][0](pkg)
    rng = np.random.default_rng(len(name))
    return g, SHAPES[name][1], [rng.standard_normal((T, g["P"])).astype(F) for T in (9, 4)]


def _with(g, label, L):
    return dict(g, label=np.asarray(label, np.int32), L=int(L))


def _coarse(g):
    """the graph with its pdfs mapped onto the 5 labels 3, 10, 17, 24, 31 (of 40): the pdfs on most arcs go to label 3 until it is on
    more than 64 arcs -- a heavy row -- and every other pdf to a random one of the five"""
    count = np.bincount(g["pdf"], minlength=g["P"])
    to_label = 3 + 7 * np.random.default_rng(7).integers(0, 5, size=g["P"])
    on_first = 0
    for p in np.argsort(-count, kind="stable"):
        if on_first > 64:
            break
        to_label[p] = 3
        on_first += count[p]
    return _with(g, to_label[g["pdf"]], 40)


# ------------------------------------------------------------------------------------------------------------------------- identity labelling
@pytest.mark.parametrize("name", list(SHAPES))
def test_identity_labelling_gives_the_pdf_call_s_bits(pkg, hip, name):
    """label = pdf, num_labels = P: the same lists, the same order, the same owners -- the compact pdf block bit for bit"""
    g, form, ys = _shape(pkg, name)
    ag = pkg.hipabi.AlignGraphs(_with(g, g["pdf"], g["P"]), num_labels=g["P"])
    assert ag.labels().dtype == np.int32 and ag.labels().tolist() == ag.pdfs().tolist()
    y, frames, rows = _stack(ys, ag.P)
    with pkg.hipabi.option("align_form", form):
        lv, lb, lr = _label_raw(pkg, ag, y, frames, rows, 1, [0, 0], F(0.3), F(0.25))
        pv, pb, pr = _compact_raw(pkg, ag, y, frames, rows, 1, [0, 0], F(0.3), F(0.25))
    assert lb.tolist() == pb.tolist() == ag.posteriors_compact_layout(frames, [0, 0]).tolist()
    assert np.array_equal(lv.view(np.int32), pv.view(np.int32)) and np.array_equal(lr.view(np.int64), pr.view(np.int64))
    assert (lr[:, 1] == 1.0).all() and lv.max() > 0


# ------------------------------------------------------------------------------------------------------------------------- coarse labelling
@pytest.mark.parametrize("scale,weight", [(1.0, 1.0), (0.3, 0.25)])
@pytest.mark.parametrize("name", list(SHAPES))
def test_coarse_labelling_against_the_reference(pkg, hip, name, scale, weight):
    """a map of the pdfs onto 5 labels (_coarse): rows mix pdfs, so y is read per arc, and one label is on more than 64 arcs -- a heavy
    row; twice: the same bits"""
    g, form, ys = _shape(pkg, name)
    gl = _coarse(g)
    counts = np.bincount(gl["label"], minlength=40)
    assert counts[3] > 64 and sum(len(set(g["pdf"][gl["label"] == l].tolist())) > 1 for l in np.nonzero(counts)[0]) >= 1
    ag = pkg.hipabi.AlignGraphs(gl, num_labels=40)
    with pkg.hipabi.option("align_form", form):
        got, refs = _check_ref(pkg, gl, ys, utt_graph=[0, 0], scale=F(scale), weight=F(weight), ag=ag)
        again, _ = _check_ref(pkg, gl, ys, utt_graph=[0, 0], scale=F(scale), weight=F(weight), ag=ag)
    assert all(r["ok"] for r in refs)
    _same_bits(got, again)


# ------------------------------------------------------------------------------------------------------------------------- arc labelling
@pytest.mark.parametrize("name", ["S65", "S1025", "heavy-row", "transcript"])
def test_arc_labelling(pkg, hip, name):
    """label = the arc's index: one column per arc, every row of the table has one arc; against the reference, and summed by pdf on the
    host in double within the same bar of the compact pdf call (each of a pdf's arcs is rounded to float at half an ulp of its own size,
    together at most half an ulp of their sum, which is at most weight; the pdf call rounds once more)"""
    if name == "transcript":
        g = pkg.synth.make_alignment_graph(np.random.default_rng(3).integers(0, 40, size=17).tolist(), optional=[0, 9], alternatives={3: [1], 16: [2, 3, 4]},
                                           num_pdfs=40, seed=3)
        ys = [(np.random.default_rng(5).standard_normal((T, 40)) * 3).astype(F) for T in (23, 30)]
    else:
        g, _, ys = _shape(pkg, name)
    A = len(g["src"])
    gl = _with(g, np.arange(A), A)
    ag = pkg.hipabi.AlignGraphs(gl, num_labels=A)
    assert ag.labels().tolist() == list(range(A))
    w = F(0.5)
    got, refs = _check_ref(pkg, gl, ys, utt_graph=[0, 0], weight=w, ag=ag)
    y, frames, rows = _stack(ys, ag.P)
    pv, pb, pr = _compact_raw(pkg, ag, y, frames, rows, 1, [0, 0], 1.0, w)
    pdfs = ag.pdfs()
    for u, T in enumerate(frames):
        by_pdf = LR.sum_by(got[u][2].astype(np.float64), g["pdf"], pdfs)
        assert np.abs(by_pdf - pv[pb[u]:pb[u + 1]].reshape(T, len(pdfs))).max() <= ULP * float(w)
        assert got[u][0] == pr[u, 0] and got[u][1] == pr[u, 1] == 1.0  # the same forward pass: the same logprob bits


# ------------------------------------------------------------------------------------------------------------------------- mixed call
def _transcripts(pkg, labels, P=40):
    """the three transcript graphs of tests/test_gpu_posteriors.py, labelled"""
    rng = np.random.default_rng(11)
    seqs = [rng.integers(0, P, size=n).tolist() for n in (1, 5, 17)]
    return [pkg.synth.make_alignment_graph(seqs[0], num_pdfs=P, seed=1, labels=labels),
            pkg.synth.make_alignment_graph(seqs[1], optional=[1, 4], alternatives={2: [7, 8]}, num_pdfs=P, seed=2, labels=labels),
            pkg.synth.make_alignment_graph(seqs[2], optional=[0, 9], alternatives={3: [1], 16: [2, 3, 4]}, num_pdfs=P, seed=3, labels=labels)]


@pytest.mark.parametrize("labels", ["unit", "arc"])
def test_mixed_call_in_both_layouts(pkg, hip, labels):
    """three transcript graphs of different sizes, utterances of 0, 1, 7, 23 and 12 frames, two pairs sharing a graph; the 12 frames are too
    few for the 17-unit transcript: ok = 0, a block of zeros, the others unaffected.  Once on stacked rows (row_stride 1), once t-major
    (row_stride B) on a sub-matrix view of a wider matrix whose surroundings hold NaN: the same bits"""
    graphs = _transcripts(pkg, labels)
    assert len({g["S"] for g in graphs}) == 3
    ag = pkg.hipabi.AlignGraphs(graphs, num_labels=max(g["L"] for g in graphs))
    rng = np.random.default_rng(5)
    frames, utt_graph, B, P = [0, 1, 7, 23, 12], [1, 0, 1, 2, 2], 5, 40
    tmajor = (rng.standard_normal((max(frames) * B, P)) * 3).astype(F)
    ys = [tmajor[u::B][:frames[u]] for u in range(B)]
    got, refs = _check_ref(pkg, graphs, ys, utt_graph=utt_graph, scale=F(0.3), weight=F(0.25), ag=ag)
    assert [r["ok"] for r in refs] == [False, True, True, True, False]
    assert got[4][2].shape == (12, graphs[2]["L"]) and (got[4][2] == 0).all() and got[4][0] == NINF
    alone, _ = _check_ref(pkg, graphs, [ys[1], ys[2], ys[3]], utt_graph=[0, 1, 2], scale=F(0.3), weight=F(0.25), ag=ag)
    _same_bits(alone, got[1:4])
    buf = torch.full((max(frames) * B + 4, P + 9), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[2:2 + max(frames) * B, 3:3 + P]
    view.copy_(dev(tmajor))
    assert view.stride(0) > view.shape[1]
    vals, begin, res = _label_raw(pkg, ag, view, frames, np.arange(B), B, utt_graph, F(0.3), F(0.25))
    _same_bits(_per_utt(ag, vals, begin, res, frames, utt_graph), got)
    # the wrapper: the same values
    v, b, r = ag.label_posteriors_compact(view, frames, np.arange(B), row_stride=B, utt_graph=utt_graph, acoustic_scale=F(0.3), weight=F(0.25))
    assert b.tolist() == begin.tolist() and np.array_equal(host(v).view(np.int32), vals.view(np.int32)) and np.array_equal(host(r).view(np.int64), res.view(np.int64))


# ------------------------------------------------------------------------------------------------------------------------- best path
def _best_raw(pkg, ag, y, frames, rows, utt_graph, scale, arcs=True):
    """tdnnf_align_best_path_labels on guarded outputs: (pdf, state, label, arc or None, results [U, 2])"""
    abi, lib = pkg.hipabi, pkg.hipabi.load()
    n, fr, rb, ug = _args(pkg, frames, rows, utt_graph)
    total = int(np.sum(frames))
    nbytes = ag.workspace_bytes(utt_graph, frames)
    assert nbytes > 0
    ws = abi.workspace(nbytes)
    pdf, state, label, arc = (_guarded(m, torch.int32) for m in (total, total + n, total, total))
    res = torch.full((n, 2), -5.0, dtype=torch.float64, device="cuda")
    abi.check(lib.tdnnf_align_best_path_labels(ag.h, n, ug[1], fr[1], rb[1], 1, abi.pmat(y), float(scale), abi.ptr(pdf[GUARD:]), abi.ptr(state[GUARD:]),
                                               abi.ptr(label[GUARD:]), abi.ptr(arc[GUARD:]) if arcs else None, abi.ptr(res), abi.ptr(ws), nbytes, abi.stream()))
    return (_inner(pdf, total, "pdfs"), _inner(state, total + n, "states"), _inner(label, total, "labels"),
            _inner(arc, total, "arcs", written=arcs), host(res))


def _check_best(pkg, graphs, ys, utt_graph=None, scale=1.0):
    graphs = [graphs] if isinstance(graphs, dict) else graphs
    ag = pkg.hipabi.AlignGraphs(graphs, num_labels=max(g["L"] for g in graphs))
    y, frames, rows = _stack(ys, ag.P)
    pdf, state, label, arc, res = _best_raw(pkg, ag, y, frames, rows, utt_graph, scale)
    p0, s0, r0 = ag.best_path(y, frames, rows, 1, utt_graph, scale, states=True)  # the unlabelled entry on the same handle
    assert np.array_equal(pdf, host(p0)) and np.array_equal(state, host(s0)) and np.array_equal(res.view(np.int64), host(r0).view(np.int64))
    wp, ws_, wr, wl, wa = ag.best_path_labels(y, frames, rows, 1, utt_graph, scale, states=True)  # the wrapper: arcs local to the graph dict
    assert np.array_equal(host(wl), label) and np.array_equal(host(wp), pdf)
    refs, at = [], 0
    for u, T in enumerate(frames):
        gi = _graph_of(ag, utt_graph, u)
        r = V.best_path(graphs[gi], ys[u], scale)
        refs.append(r)
        first = int(ag.arc_begin[gi])
        assert res[u, 1] == (1.0 if r["ok"] else 0.0)
        if r["ok"]:
            assert res[u, 0] == r["score"]
            assert np.array_equal(arc[at:at + T], r["arcs"] + first), "utterance %d: the arcs, in the call's numbering" % u
            assert np.array_equal(host(wa)[at:at + T], r["arcs"])
            assert np.array_equal(label[at:at + T], np.asarray(graphs[gi]["label"])[r["arcs"]])
        else:
            assert (arc[at:at + T] == -1).all() and (label[at:at + T] == -1).all() and (host(wa)[at:at + T] == -1).all()
        at += T
    return refs


@pytest.mark.parametrize("S", [64, 65, 1025])
def test_best_path_labels_cyclic(pkg, hip, S):
    g = _cyclic(pkg, S)
    rng = np.random.default_rng(S)
    gl = _with(g, rng.integers(0, 1000, size=len(g["src"])), 1000)
    refs = _check_best(pkg, gl, [rng.standard_normal((T, 50)).astype(F) * 2 for T in (9, 4, 300)], utt_graph=[0, 0, 0], scale=F(0.7))
    assert all(r["ok"] for r in refs)


@pytest.mark.parametrize("labels", ["unit", "arc"])
def test_best_path_labels_transcripts(pkg, hip, labels):
    """graphs with alternatives and optional units, the second and third graph's arcs behind the first's in the call's numbering; an
    utterance of no frames and one too short for its transcript: -1 for every label and arc"""
    graphs = _transcripts(pkg, labels)
    rng = np.random.default_rng(6)
    ys = [rng.standard_normal((T, 40)).astype(F) * 3 for T in (0, 1, 7, 23, 12, 40)]
    refs = _check_best(pkg, graphs, ys, utt_graph=[1, 0, 1, 2, 2, 2])
    assert [r["ok"] for r in refs] == [False, True, True, True, False, True]


def test_best_path_parallel_arcs_give_the_first_label(pkg, hip):
    """two arcs of equal (source, destination, pdf, logprob) and different labels: the first in the caller's list is reported, whichever
    its label; without arc_out the call writes the labels alone"""
    g = {"S": 3, "P": 4, "src": np.asarray([0, 0, 1, 1, 1, 2], np.int32), "dst": np.asarray([1, 1, 1, 2, 2, 2], np.int32),
         "pdf": np.asarray([1, 1, 2, 3, 3, 0], np.int32), "logprob": np.asarray([-0.5, -0.5, -0.25, -1.0, -1.0, -0.125], F),
         "init": np.asarray([0, NINF, NINF], F), "final": np.asarray([NINF, NINF, 0], F)}
    y = np.random.default_rng(2).standard_normal((6, 4)).astype(F)
    for label in ([9, 2, 5, 1, 8, 5], [2, 9, 5, 8, 1, 5]):
        gl = _with(g, label, 10)
        r = _check_best(pkg, gl, [y])[0]
        assert r["ok"] and r["arcs"][0] == 0 and 3 in r["arcs"] and 4 not in r["arcs"] and 1 not in r["arcs"]
        ag = pkg.hipabi.AlignGraphs(gl, num_labels=10)
        yd, frames, rows = _stack([y], 4)
        _, _, lab, untouched, _ = _best_raw(pkg, ag, yd, frames, rows, None, 1.0, arcs=False)
        assert (untouched == SENTINEL).all()
        assert lab.tolist() == np.asarray(label)[r["arcs"]].tolist() and lab[0] == label[0] and label[3] in lab.tolist()


# ------------------------------------------------------------------------------------------------------------------------- sparse
def _sparse_raw(pkg, ag, y, frames, rows, utt_graph, scale, weight, min_post, K):
    abi, lib = pkg.hipabi, pkg.hipabi.load()
    n, fr, rb, ug = _args(pkg, frames, rows, utt_graph)
    total = int(np.sum(frames))
    nbytes = int(lib.tdnnf_align_label_posteriors_sparse_workspace_bytes(ag.h, n, ug[1], fr[1], K))
    assert nbytes > 0, lib.tdnnf_last_error()
    ws = abi.workspace(nbytes)
    lab, post, count, res = _guarded(total * K, torch.int32), _guarded(total * K, torch.float32), _guarded(total, torch.int32), _guarded(4 * n, torch.float64)
    abi.check(lib.tdnnf_align_label_posteriors_sparse(ag.h, n, ug[1], fr[1], rb[1], 1, abi.pmat(y), float(scale), float(weight), float(min_post), K,
                                                      abi.ptr(lab[GUARD:]), abi.ptr(post[GUARD:]), abi.ptr(count[GUARD:]), abi.ptr(res[GUARD:]), abi.ptr(ws),
                                                      nbytes, abi.stream()))
    return (_inner(lab, total * K, "labels").reshape(total, K), _inner(post, total * K, "values").reshape(total, K), _inner(count, total, "counts"),
            _inner(res, 4 * n, "results").reshape(n, 4))


@pytest.mark.parametrize("min_post", [0.0, 0.01])
@pytest.mark.parametrize("K", [1, 4, 64])
def test_sparse_equals_sparsify_of_the_label_block(pkg, hip, K, min_post):
    graphs = _transcripts(pkg, "arc")
    ag = pkg.hipabi.AlignGraphs(graphs, num_labels=max(g["L"] for g in graphs))
    rng = np.random.default_rng(8)
    ys = [rng.standard_normal((T, 40)).astype(F) for T in (0, 1, 7, 23, 12)]
    utt_graph, w = [1, 0, 1, 2, 2], F(0.75)
    y, frames, rows = _stack(ys, 40)
    vals, begin, cres = _label_raw(pkg, ag, y, frames, rows, 1, utt_graph, 1.0, w)
    lab, post, count, res = _sparse_raw(pkg, ag, y, frames, rows, utt_graph, 1.0, w, min_post, K)
    at, truncated = 0, 0
    for u, T in enumerate(frames):
        labels = ag.labels(utt_graph[u])
        wl, wp, wc, n = sparsify(vals[begin[u]:begin[u + 1]].reshape(T, len(labels)), labels, min_post, K)
        assert np.array_equal(lab[at:at + T], wl) and np.array_equal(post[at:at + T].view(np.int32), wp.view(np.int32)) and np.array_equal(count[at:at + T], wc)
        assert res[u].view(np.int64).tolist()[:2] == cres[u].view(np.int64).tolist() and res[u, 2] == (n > K).sum() and res[u, 3] == n.max(initial=0)
        truncated += int((n > K).sum())
        at += T
    assert (K >= 4) or truncated > 0  # with one slot a frame some frame has more candidates than slots
    assert cres[:, 1].tolist() == [0.0, 1.0, 1.0, 1.0, 0.0] and (count[-12:] == 0).all() and (lab[-12:] == -1).all()
    # the wrapper
    wl_, wp_, wc_, wr_ = ag.label_posteriors_sparse(y, frames, rows, 1, utt_graph, 1.0, w, min_post, K)
    assert np.array_equal(host(wl_), lab) and np.array_equal(host(wp_).view(np.int32), post.view(np.int32)) and np.array_equal(host(wc_), count)
    assert np.array_equal(host(wr_).view(np.int64), res.view(np.int64))


# ------------------------------------------------------------------------------------------------------------------------- unchanged behaviour
def test_a_labelled_handle_serves_the_old_entries_with_the_same_bits(pkg, hip):
    graphs = _transcripts(pkg, "unit") + [_with(_cyclic(pkg, 300), np.arange(len(_cyclic(pkg, 300)["src"])) % 11, 11)]
    plain = [{k: v for k, v in g.items() if k not in ("label", "L")} for g in graphs]
    P = 50
    a, b = pkg.hipabi.AlignGraphs(graphs, num_pdfs=P, num_labels=max(g["L"] for g in graphs)), pkg.hipabi.AlignGraphs(plain, num_pdfs=P)
    assert a.labelled and not b.labelled
    rng = np.random.default_rng(9)
    ys = [rng.standard_normal((T, P)).astype(F) * 2 for T in (5, 9, 30, 12, 8)]
    y, frames, rows = _stack(ys, P)
    ug = [0, 1, 2, 3, 2]
    same = lambda x, z: all(np.array_equal(host(p).view(np.uint8), host(q).view(np.uint8)) for p, q in zip(x, z))
    assert same(a.best_path(y, frames, rows, 1, ug, 0.5, states=True), b.best_path(y, frames, rows, 1, ug, 0.5, states=True))
    assert same(a.posteriors(y, frames, rows, 1, ug, 0.5, 0.25), b.posteriors(y, frames, rows, 1, ug, 0.5, 0.25))
    ca, cb = a.posteriors_compact(y, frames, rows, 1, ug, 0.5, 0.25), b.posteriors_compact(y, frames, rows, 1, ug, 0.5, 0.25)
    assert same((ca[0], ca[2]), (cb[0], cb[2])) and ca[1].tolist() == cb[1].tolist()
    assert same(a.posteriors_sparse(y, frames, rows, 1, ug, 0.5, 0.25, 0.01, 4), b.posteriors_sparse(y, frames, rows, 1, ug, 0.5, 0.25, 0.01, 4))
    assert same([a.logprob(y, frames, rows, 1, ug, 0.5)], [b.logprob(y, frames, rows, 1, ug, 0.5)])
    assert all(a.pdfs(k).tolist() == b.pdfs(k).tolist() and a.info(k) == b.info(k) for k in range(4))


def test_label_entries_refuse_an_unlabelled_handle_and_a_bad_count(pkg, hip):
    abi, lib = pkg.hipabi, pkg.hipabi.load()
    g = pkg.synth.make_alignment_graph([1, 2, 3], num_pdfs=5, labels="unit")
    plain = {k: v for k, v in g.items() if k not in ("label", "L")}
    ag = abi.AlignGraphs(plain, num_pdfs=5)
    y = dev(np.zeros((10, 5), F))
    for call, who in ((lambda: ag.labels(), "align_graphs_labels"), (lambda: ag.label_posteriors_compact_layout([4, 6], [0, 0]), "align_label_posteriors_compact_layout"),
                      (lambda: ag.label_posteriors_compact(y, [4, 6], [0, 4], utt_graph=[0, 0]), "align_label_posteriors_compact_layout"),
                      (lambda: ag.best_path_labels(y, [4, 6], [0, 4], utt_graph=[0, 0]), "align_best_path_labels"),
                      (lambda: ag.label_posteriors_sparse(y, [4, 6], [0, 4], utt_graph=[0, 0]), "align_label_posteriors_sparse")):
        with pytest.raises(abi.HipAbiError, match=who + ": the graphs carry no labels"):
            call()
    fr, rb, ug = abi.iarr([4, 6]), abi.iarr([0, 4]), abi.iarr([0, 0])
    out, res, ws = torch.full((64,), float(SENTINEL), device="cuda"), torch.full((4,), -5.0, dtype=torch.float64, device="cuda"), abi.workspace(1 << 16)
    assert lib.tdnnf_align_label_posteriors_compact(ag.h, 2, ug[1], fr[1], rb[1], 1, abi.pmat(y), 1.0, 1.0, abi.ptr(out), 64, abi.ptr(res), abi.ptr(ws), 1 << 16,
                                                    abi.stream()) == 1
    assert lib.tdnnf_last_error().startswith(b"align_label_posteriors_compact: the graphs carry no labels")
    assert (host(out) == SENTINEL).all() and (host(res) == -5.0).all()  # nothing was launched
    lag = abi.AlignGraphs(g, num_pdfs=5, num_labels=3)
    for K in (0, 65):
        with pytest.raises(abi.HipAbiError, match="align_label_posteriors_sparse: max_per_frame"):
            lag.label_posteriors_sparse(y, [4, 6], [0, 4], utt_graph=[0, 0], max_per_frame=K)
    v, b, r = lag.label_posteriors_compact(y, [4, 6], [0, 4], utt_graph=[0, 0])
    assert b.tolist() == [0, 12, 30] and (host(r)[:, 1] == 1.0).all() and np.abs(host(v).reshape(10, 3).sum(1, dtype=np.float64) - 1.0).max() <= 1e-6


# ------------------------------------------------------------------------------------------------------------------------- the model, archives
def test_infer_entries_and_archives(pkg, hip, tmp_path):
    """infer.align_labels / label_posteriors_compact / label_posteriors_sparse on a model's output; write_int_vector_archive of the labels
    and write_posterior_archive of a sparse label item give the bytes of the same data written by hand"""
    graphs = _transcripts(pkg, "arc")
    ag = pkg.hipabi.AlignGraphs(graphs, num_labels=max(g["L"] for g in graphs))
    rng = np.random.default_rng(12)
    outs = [dev(rng.standard_normal((T, 40)).astype(F) * 3) for T in (4, 9, 25)]
    ali = pkg.infer.align_labels(outs, ag)
    comp = pkg.infer.label_posteriors_compact(outs, ag, weight=0.5)
    sp = pkg.infer.label_posteriors_sparse(outs, ag, weight=0.5, min_post=0.01, max_per_frame=4)
    plain = pkg.infer.align(outs, ag)
    for u, g in enumerate(graphs):
        pdfs, labels, arcs, score, ok = ali[u]
        r = V.best_path(g, host(outs[u]))
        assert ok and score == r["score"] == plain[u][1] and np.array_equal(host(pdfs), host(plain[u][0]))
        assert np.array_equal(host(arcs), r["arcs"]) and np.array_equal(host(labels), g["label"][r["arcs"]]) and labels.dtype == torch.int32
        ids, post, lp, ok2 = comp[u]
        assert ok2 and np.array_equal(ids, ag.labels(u)) and tuple(post.shape) == (len(r["arcs"]), g["L"])
        wl, wp, wc, _ = sparsify(host(post), ids, 0.01, 4)
        assert np.array_equal(host(sp[u][0]), wl) and np.array_equal(host(sp[u][1]), wp) and np.array_equal(host(sp[u][2]), wc) and sp[u][3] == lp
    a = tmp_path / "ali.ark"
    pkg.infer.write_int_vector_archive(a, [("utt%d" % u, x[1]) for u, x in enumerate(ali)])
    by_hand = b"".join(b"utt%d \0B" % u + struct.pack("<bi", 4, len(x[1])) + host(x[1]).astype("<i4").tobytes() for u, x in enumerate(ali))
    assert a.read_bytes() == by_hand and len(by_hand) > 100
    b = tmp_path / "post.ark"
    pkg.infer.write_posterior_archive(b, [("utt%d" % u, x[0], x[1], x[2]) for u, x in enumerate(sp)], min_post=0.01)
    by_hand = b""
    for u, x in enumerate(sp):
        lab, post, count = host(x[0]), host(x[1]), host(x[2])
        by_hand += b"utt%d \0B" % u + struct.pack("<bi", 4, len(lab))
        for t in range(len(lab)):
            by_hand += struct.pack("<bi", 4, int(count[t])) + b"".join(struct.pack("<bibf", 4, int(lab[t, k]), 4, float(post[t, k])) for k in range(count[t]))
    assert b.read_bytes() == by_hand and len(by_hand) > 300
    back = pkg.infer.read_posterior_archive(b)
    assert all(all(l in graphs[u]["label"] for l, _ in frame) for u in range(3) for frame in back["utt%d" % u])
