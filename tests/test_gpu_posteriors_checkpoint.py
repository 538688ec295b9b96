"""-m gpu: alpha checkpointing of the forward-backward pass (option align_checkpoint; csrc/align_fb_kernels.h fb_backward_ckpt, the plan in
csrc/align_tables.h; include/tdnnf_hip.h "forward-backward").

The bar is BITS: the backward pass recomputes a segment's alphas from its checkpoint by the forward pass's own step in its own order, so
under align_checkpoint = C every output, logprob and ok flag of the dense, the compact and the label call equals what option 0 gives, bit
for bit -- on every launch form (thread counts, alpha_t staged or not, vectors in LDS or in the workspace, rows staged or not) and for the
intervals that reach every branch of the schedule: C = 1, C dividing T, C = T - 1, T, T + 1, beyond, one-frame last segments.  So that the
code is not only compared with itself, the option-0 result of every case is also held to tests/posteriors_ref64.py (labels:
tests/label_posteriors_ref64.py) at the bars of tests/test_gpu_posteriors.py (its _close).

Every call runs in a workspace allocated at the size option 0 needs, filled with a byte pattern, and is told the checkpointed size: the
pattern beyond that size must survive, so a kernel that still indexed alpha by frame shows as a failed assertion inside the allocation.
Outputs lie between canaries over a sentinel, as in tests/test_gpu_posteriors_compact.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import label_posteriors_ref64 as LR
from tests import posteriors_ref64 as PR
from tests.gpu_util import Hip, dev, host, padded
from tests.test_gpu_posteriors import _close, _same_bits, _transcripts
from tests.test_gpu_posteriors_compact import _labelled as _graph_with_pdfs

pytestmark = pytest.mark.gpu
F = np.float32
NINF = -np.inf
GUARD, CANARY, SENTINEL, FILL, PATTERN = 16, 123.0, -7.25, -81.0, 0xA5
OPT = "align_checkpoint"


@pytest.fixture(scope="module")
def hip(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return Hip(pkg)


def _with_labels(g):
    """a labelling that is neither the pdfs nor the arcs: the pdfs 2k and 2k + 1 share the labels 2k and 2k + 1, which an arc takes by the
    parity of its index -- a label's arcs name two pdfs and a pdf's arcs carry two labels"""
    pdf = np.asarray(g["pdf"])
    return dict(g, label=((pdf // 2) * 2 + np.arange(len(pdf)) % 2).astype(np.int32), L=(int(g["P"]) + 1) // 2 * 2)


def _handle(pkg, graphs):
    graphs = [_with_labels(g) for g in ([graphs] if isinstance(graphs, dict) else graphs)]
    return graphs, pkg.hipabi.AlignGraphs(graphs, num_labels=max(g["L"] for g in graphs))


def _interval(c, frames):
    return max(1, math.isqrt(max(max(frames), 1) - 1) + 1 if max(frames) > 1 else 1) if c == -1 else c


def _vectors(T, c):
    """V(T, C) of include/tdnnf_hip.h"""
    return T + 1 if c == 0 else 1 if T == 0 else -(-T // c) + min(c, T) - 1


def _graph_of(ag, utt_graph, u):
    return utt_graph[u] if utt_graph is not None else (0 if ag.G == 1 else u)


def _formula(ag, frames, utt_graph, c, workspace_form):
    """bytes of tdnnf_align_posteriors_workspace_bytes with want_posteriors, from the header"""
    S = [ag.num_states[_graph_of(ag, utt_graph, u)] for u in range(len(frames))]
    c = _interval(c, frames)
    return (16 + -(-32 * len(frames) // 256) * 256 + 8 * sum(_vectors(T, c) * s for T, s in zip(frames, S))
            + (16 * sum(S) if workspace_form else 0))


def _workspace(nbytes0):
    ws = torch.full((GUARD + nbytes0 + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    return ws


def _pattern_kept(ws, nbytes, what):
    b = host(ws)
    assert (b[:GUARD] == PATTERN).all() and (b[GUARD + nbytes:] == PATTERN).all(), what + " wrote beyond the workspace it was given"


def _guarded(n):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    buf[:GUARD] = CANARY
    buf[GUARD + n:] = CANARY
    return buf


def _inner(buf, n, what):
    b = host(buf)
    assert (b[:GUARD] == CANARY).all() and (b[GUARD + n:] == CANARY).all(), what + " wrote outside its blocks"
    assert not (b[GUARD:GUARD + n] == SENTINEL).any(), "an element of a block of " + what + " was not written"
    return b[GUARD:GUARD + n]


def _calls(pkg, ag, y, frames, rows, stride, utt_graph, c, workspace_form, scale=1.0, weight=1.0):
    """The dense, the compact and the label call under align_checkpoint = c, each in a patterned workspace of option 0's size that it is
    told to be of the checkpointed size, on guarded outputs.  Returns {"dense" | "compact" | "label": per utterance (logprob, ok, its rows
    or block)}."""
    abi, lib = pkg.hipabi, pkg.hipabi.load()
    n = len(frames)
    fr, rb = abi.iarr(frames), abi.iarr(rows)
    ug = abi.iarr(utt_graph) if utt_graph is not None else (None, None)
    with abi.option(OPT, 0):
        nbytes0 = ag.posteriors_workspace_bytes(utt_graph, frames)
        assert nbytes0 == _formula(ag, frames, utt_graph, 0, workspace_form)
    out = {}
    with abi.option(OPT, c):
        nbytes = ag.posteriors_workspace_bytes(utt_graph, frames)
        assert nbytes == _formula(ag, frames, utt_graph, c, workspace_form), (nbytes, c)
        assert nbytes <= nbytes0
        ce = _interval(c, frames)
        if any(_vectors(T, ce) < T + 1 for T in frames) and c != 0:
            assert nbytes < nbytes0
        assert ag.posteriors_workspace_bytes(utt_graph, frames, False) == nbytes0 - 8 * sum(
            (T + 1) * ag.num_states[_graph_of(ag, utt_graph, u)] for u, T in enumerate(frames))  # (no alpha, no option)
        # dense: post_out is a view, two columns and a row wider than the call, inside a buffer wider and longer still
        nrows = y.shape[0]
        post_buf = torch.full((nrows + 2, ag.P + 7), FILL, dtype=torch.float32, device="cuda")
        post_view = post_buf[:nrows + 1, :ag.P + 3]
        res, ws = torch.full((n, 2), -5.0, dtype=torch.float64, device="cuda"), _workspace(nbytes0)
        abi.check(lib.tdnnf_align_posteriors(ag.h, n, ug[1], fr[1], rb[1], int(stride), abi.pmat(y), float(scale), float(weight), abi.pmat(post_view),
                                             abi.ptr(res), abi.ptr(ws[GUARD:]), nbytes, abi.stream()))
        _pattern_kept(ws, nbytes, "the dense call")
        post, r = host(post_buf), host(res)
        assert (post[:, ag.P:] == FILL).all() and (post[nrows:] == FILL).all(), "the dense call wrote outside its columns or rows"
        touched = np.zeros(nrows + 2, bool)
        out["dense"] = []
        for u, T in enumerate(frames):
            at = rows[u] + stride * np.arange(T)
            touched[at] = True
            out["dense"].append((r[u, 0], r[u, 1], post[at, :ag.P].copy()))
        assert (post[~touched] == FILL).all(), "the dense call wrote a row that is no frame of the call"
        for name, entry, layout in (("compact", lib.tdnnf_align_posteriors_compact, ag.posteriors_compact_layout),
                                    ("label", lib.tdnnf_align_label_posteriors_compact, ag.label_posteriors_compact_layout)):
            begin = layout(frames, utt_graph)
            elems = int(begin[-1])
            buf, res, ws = _guarded(elems), torch.full((n, 2), -5.0, dtype=torch.float64, device="cuda"), _workspace(nbytes0)
            abi.check(entry(ag.h, n, ug[1], fr[1], rb[1], int(stride), abi.pmat(y), float(scale), float(weight), abi.ptr(buf[GUARD:]), elems,
                            abi.ptr(res), abi.ptr(ws[GUARD:]), nbytes, abi.stream()))
            _pattern_kept(ws, nbytes, "the %s call" % name)
            vals, r = _inner(buf, elems, "the %s call" % name), host(res)
            out[name] = [(r[u, 0], r[u, 1], vals[begin[u]:begin[u + 1]].reshape(T, -1) if T else np.zeros((0, 1), F)) for u, T in enumerate(frames)]
    return out


def _all_same_bits(a, b):
    for name in ("dense", "compact", "label"):
        _same_bits(a[name], b[name])


def _reference_bars(ag, graphs, ys, utt_graph, base, scale=1.0, weight=1.0):
    """the option-0 result within the bars of the float64 references; the compact block is the dense rows' columns, bit for bit"""
    for u, yu in enumerate(ys):
        gi = _graph_of(ag, utt_graph, u)
        g = graphs[gi]
        _close(base["dense"][u], PR.forward_backward(g, yu, scale), weight, "dense, utterance %d" % u)
        pdfs = ag.pdfs(gi)
        lp, ok, block = base["compact"][u]
        if len(yu):
            _same_bits([(lp, ok, block)], [(base["dense"][u][0], base["dense"][u][1], base["dense"][u][2][:, pdfs])])
        ref = LR.label_posteriors(g, g["label"], yu, scale)
        assert ag.labels(gi).tolist() == ref["labels"].tolist()
        if len(yu):
            _close(base["label"][u], ref, weight, "label, utterance %d" % u)


def _stacked(ys, P):
    frames = [len(y) for y in ys]
    rows = np.concatenate([[0], np.cumsum(frames)[:-1]])
    return dev(np.concatenate(ys) if sum(frames) else np.zeros((1, P), F)), frames, rows


def _case(pkg, graphs, ys, intervals, utt_graph=None, workspace_form=False, scale=1.0, weight=1.0):
    """option 0 once, held to the references; then every interval against its bits"""
    graphs, ag = _handle(pkg, graphs)
    y, frames, rows = _stacked(ys, ag.P)
    base = _calls(pkg, ag, y, frames, rows, 1, utt_graph, 0, workspace_form, scale, weight)
    _reference_bars(ag, graphs, ys, utt_graph, base, scale, weight)
    for c in intervals:
        _all_same_bits(_calls(pkg, ag, y, frames, rows, 1, utt_graph, c, workspace_form, scale, weight), base)
    return graphs, ag, base


# ------------------------------------------------------------------------------------------------------------------------- the schedule
MIXED_FRAMES, MIXED_GRAPH = (0, 1, 7, 23, 12), [2, 0, 1, 2, 1]


@pytest.fixture(scope="module")
def mixed(pkg, hip):
    """transcript graphs, five utterances with two pairs sharing a graph: the option-0 call, held to the references once"""
    graphs, ag = _handle(pkg, _transcripts(pkg))
    rng = np.random.default_rng(5)
    ys = [rng.standard_normal((T, 40)).astype(F) * 3 for T in MIXED_FRAMES]
    y, frames, rows = _stacked(ys, ag.P)
    base = _calls(pkg, ag, y, frames, rows, 1, MIXED_GRAPH, 0, False, F(0.3), F(0.25))
    _reference_bars(ag, graphs, ys, MIXED_GRAPH, base, F(0.3), F(0.25))
    assert [x[1] for x in base["dense"]] == [0.0, 1.0, 1.0, 1.0, 1.0]
    return ag, y, frames, rows, base


@pytest.mark.parametrize("c", [1, 2, 3, 7, 22, 23, 24, 100, -1])
def test_mixed_call_every_interval(pkg, hip, mixed, c):
    """frames (0, 1, 7, 23, 12): C = 1 (no recomputation, the rows staged on from segment to segment), 2 and 3 (a one-frame last segment
    at 7 and 23 / at 7), 7 (C = T and C dividing nothing else), 22 = T - 1, 23 = T, 24 = T + 1, 100 beyond every utterance, -1 (5)"""
    ag, y, frames, rows, base = mixed
    got = _calls(pkg, ag, y, frames, rows, 1, MIXED_GRAPH, c, False, F(0.3), F(0.25))
    _all_same_bits(got, base)
    if c == 3:
        _all_same_bits(_calls(pkg, ag, y, frames, rows, 1, MIXED_GRAPH, c, False, F(0.3), F(0.25)), got)  # two identical calls


@pytest.mark.parametrize("S", [64, 65, 1024, 1025])
def test_block_size_boundaries_cyclic(pkg, hip, S):
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(S, 50, mean_out_degree=4.0, seed=S))
    rng = np.random.default_rng(S)
    _case(pkg, g, [rng.standard_normal((T, 50)).astype(F) for T in (9, 4)], [4])


@pytest.mark.parametrize("S", [6400, 6401, 9600, 9601])
def test_state_vector_thresholds(pkg, hip, S):
    """alpha_t staged in a third LDS vector up to 6 400 states (the recomputation runs on LDS vectors), two LDS vectors up to 9 600 and
    the workspace form above (it gathers from the segment buffer); three segments, the last of one frame"""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(S, 50, mean_out_degree=3.0, seed=S))
    rng = np.random.default_rng(S)
    _case(pkg, g, [rng.standard_normal((T, 50)).astype(F) for T in (7, 7)], [3], workspace_form=S > 9600)


@pytest.mark.parametrize("S,P", [(30, 512), (30, 513), (100, 2048), (100, 2049)])
def test_row_staging_threshold(pkg, hip, S, P):
    """rows staged in LDS (primed again at every change of direction) and gathered from global memory"""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(S, P, mean_out_degree=6.0, seed=P))
    rng = np.random.default_rng(P)
    _case(pkg, g, [rng.standard_normal((T, P)).astype(F) for T in (7, 1, 2)], [3])


@pytest.mark.parametrize("form", [1, 2])
def test_both_forms(pkg, hip, form):
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(H=300, P=50))
    rng = np.random.default_rng(9)
    with pkg.hipabi.option("align_form", form):
        _case(pkg, g, [rng.standard_normal((T, 50)).astype(F) * 4 for T in (10, 4)], [3], workspace_form=form == 2)


def test_heavy_pdf_row(pkg, hip):
    """one pdf on 300 arcs: a wave walks its row in step 2; C = 2"""
    g = _graph_with_pdfs(50, np.concatenate([np.full(300, 9), np.full(64, 4), np.full(3, 2), np.full(20, 11), np.full(1, 30)]), 300)
    rng = np.random.default_rng(300)
    _case(pkg, g, [rng.standard_normal((T, g["P"])).astype(F) * 2 for T in (8, 3)], [2])


# ------------------------------------------------------------------------------------------------------------------------- ok = 0
def test_failed_utterances_leave_neighbours_alone(pkg, hip):
    """an utterance too short for its graph and one with +inf in its rows: ok = 0 and zeros, under the option as without it; the other
    utterances have the bits they have in a call of their own"""
    rng = np.random.default_rng(8)
    ys = [rng.standard_normal((T, 40)).astype(F) for T in (12, 2, 30, 9)]  # graph 1 needs at least 3 frames; the last is on graph 0, as the first
    ys[3][5, :] = np.inf
    graphs, ag, base = _case(pkg, _transcripts(pkg), ys, [3], utt_graph=[0, 1, 2, 0])
    y, frames, rows = _stacked(ys, ag.P)
    got = _calls(pkg, ag, y, frames, rows, 1, [0, 1, 2, 0], 3, False)
    for name in ("dense", "compact", "label"):
        assert [x[1] for x in got[name]] == [1.0, 0.0, 1.0, 0.0]
        assert got[name][1][0] == NINF and got[name][3][0] == np.inf
        assert (got[name][1][2] == 0).all() and (got[name][3][2] == 0).all()
    y2, frames2, rows2 = _stacked([ys[0], ys[2]], ag.P)
    alone = _calls(pkg, ag, y2, frames2, rows2, 1, [0, 2], 3, False)
    for name in ("dense", "compact", "label"):
        _same_bits(alone[name], [got[name][0], got[name][2]])


# ------------------------------------------------------------------------------------------------------------------------- layouts
def test_strided_call_on_views(pkg, hip):
    """t-major rows (row_stride = B) in a sub-matrix view of nnet_output; post_out is a view in every call of this file"""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(H=90, P=20, mean_out_degree=5.0, seed=2))
    graphs, ag = _handle(pkg, g)
    rng = np.random.default_rng(4)
    B, frames = 3, [11, 5, 8]
    tmajor = rng.standard_normal((max(frames) * B, 20)).astype(F)
    ys = [tmajor[u::B][:frames[u]] for u in range(B)]
    view, _ = padded(tmajor)
    assert view.stride(0) > view.shape[1]
    base = _calls(pkg, ag, view, frames, np.arange(B), B, None, 0, False)
    _reference_bars(ag, graphs, ys, None, base)
    for c in (3, -1):
        _all_same_bits(_calls(pkg, ag, view, frames, np.arange(B), B, None, c, False), base)
    y, _, rows = _stacked(ys, ag.P)
    _all_same_bits(_calls(pkg, ag, y, frames, rows, 1, None, 3, False), base)  # the same data concatenated


# ------------------------------------------------------------------------------------------------------------------------- sparse
@pytest.mark.parametrize("labels", [False, True])
def test_sparse_forms(pkg, hip, mixed, labels):
    """the sparse calls run the compact call inside: their workspace question follows the option and their outputs keep their bits"""
    ag, y, frames, rows, _ = mixed
    call = ag.label_posteriors_sparse if labels else ag.posteriors_sparse
    nbytes = ag.label_posteriors_sparse_workspace_bytes if labels else ag.posteriors_sparse_workspace_bytes
    base = [host(t) for t in call(y, frames, rows, 1, MIXED_GRAPH, 0.3, 0.25, 0.01, 4, checkpoint=0)]
    got = [host(t) for t in call(y, frames, rows, 1, MIXED_GRAPH, 0.3, 0.25, 0.01, 4, checkpoint=3)]
    assert (base[2] > 0).any()
    for a, b in zip(got, base):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int64 if a.dtype == np.float64 else np.int32),
                                                     b.view(np.int64 if b.dtype == np.float64 else np.int32))
    with pkg.hipabi.option(OPT, 0):
        fb0, sp0 = ag.posteriors_workspace_bytes(MIXED_GRAPH, frames), nbytes(MIXED_GRAPH, frames, 4)
    with pkg.hipabi.option(OPT, 3):
        fb3, sp3 = ag.posteriors_workspace_bytes(MIXED_GRAPH, frames), nbytes(MIXED_GRAPH, frames, 4)
    assert fb3 < fb0 and fb0 % 16 == 0 and fb3 % 16 == 0 and sp0 - sp3 == fb0 - fb3
    assert nbytes(MIXED_GRAPH, frames, 4, checkpoint=3) == sp3 and nbytes(MIXED_GRAPH, frames, 4, checkpoint=0) == sp0


# ------------------------------------------------------------------------------------------------------------------------- refusals
def _option(pkg):
    v = C.c_int()
    pkg.hipabi.check(pkg.hipabi.load().tdnnf_get_option(OPT.encode(), C.byref(v)))
    return v.value


def test_refusals(pkg, hip, mixed):
    abi, lib = pkg.hipabi, hip.lib
    ag, y, frames, rows, base = mixed
    n = len(frames)
    fr, rb, ug = abi.iarr(frames), abi.iarr(rows), abi.iarr(MIXED_GRAPH)
    post = torch.full((y.shape[0], ag.P), FILL, dtype=torch.float32, device="cuda")
    res = torch.full((n, 4), -5.0, dtype=torch.float64, device="cuda")
    elems = max(int(ag.posteriors_compact_layout(frames, MIXED_GRAPH)[-1]), int(ag.label_posteriors_compact_layout(frames, MIXED_GRAPH)[-1]))
    vals = torch.full((elems,), SENTINEL, dtype=torch.float32, device="cuda")
    F4 = sum(frames) * 4
    ids, sel, cnt = (torch.full((F4,), -9, dtype=torch.int32, device="cuda"), torch.full((F4,), SENTINEL, dtype=torch.float32, device="cuda"),
                     torch.full((sum(frames),), -9, dtype=torch.int32, device="cuda"))
    with abi.option(OPT, 0):
        big = ag.posteriors_sparse_workspace_bytes(MIXED_GRAPH, frames, 4) + ag.label_posteriors_sparse_workspace_bytes(MIXED_GRAPH, frames, 4)
        nb0 = ag.posteriors_workspace_bytes(MIXED_GRAPH, frames, False)
    ws = hip.ws(big)
    common = (ag.h, n, ug[1], fr[1], rb[1], 1, abi.pmat(y), 1.0, 1.0)
    calls = {b"align_posteriors: ": lambda nb: lib.tdnnf_align_posteriors(*common, abi.pmat(post), abi.ptr(res), abi.ptr(ws), nb, abi.stream()),
             b"align_posteriors_compact: ": lambda nb: lib.tdnnf_align_posteriors_compact(*common, abi.ptr(vals), elems, abi.ptr(res), abi.ptr(ws), nb,
                                                                                          abi.stream()),
             b"align_label_posteriors_compact: ": lambda nb: lib.tdnnf_align_label_posteriors_compact(*common, abi.ptr(vals), elems, abi.ptr(res),
                                                                                                      abi.ptr(ws), nb, abi.stream()),
             b"align_posteriors_sparse: ": lambda nb: lib.tdnnf_align_posteriors_sparse(*common, 0.01, 4, abi.ptr(ids), abi.ptr(sel), abi.ptr(cnt),
                                                                                        abi.ptr(res), abi.ptr(ws), nb, abi.stream()),
             b"align_label_posteriors_sparse: ": lambda nb: lib.tdnnf_align_label_posteriors_sparse(*common, 0.01, 4, abi.ptr(ids), abi.ptr(sel),
                                                                                                    abi.ptr(cnt), abi.ptr(res), abi.ptr(ws), nb,
                                                                                                    abi.stream())}
    for bad in (-2, -7):
        with abi.option(OPT, bad):
            assert ag.posteriors_workspace_bytes(MIXED_GRAPH, frames) == 0 and OPT.encode() in lib.tdnnf_last_error()
            assert ag.posteriors_sparse_workspace_bytes(MIXED_GRAPH, frames, 4) == 0 and OPT.encode() in lib.tdnnf_last_error()
            assert ag.label_posteriors_sparse_workspace_bytes(MIXED_GRAPH, frames, 4) == 0 and OPT.encode() in lib.tdnnf_last_error()
            for who, call in calls.items():
                assert call(big) == 1, who
                assert lib.tdnnf_last_error().startswith(who) and OPT.encode() in lib.tdnnf_last_error(), (who, lib.tdnnf_last_error())
            # where no alpha is kept the option is not read: the workspace question and the call without a posterior matrix
            assert ag.posteriors_workspace_bytes(MIXED_GRAPH, frames, False) == nb0
            lp = host(ag.logprob(y, frames, rows, 1, MIXED_GRAPH, 0.3))
            assert np.array_equal(lp[:, 0].view(np.int64), np.asarray([x[0] for x in base["dense"]]).view(np.int64))
    torch.cuda.synchronize()
    assert (host(post) == FILL).all() and (host(vals) == SENTINEL).all() and (host(res) == -5.0).all() and (host(cnt) == -9).all()  # nothing was launched
    # a workspace one byte short of the checkpointed size
    with abi.option(OPT, 3):
        need = ag.posteriors_workspace_bytes(MIXED_GRAPH, frames)
        for who in (b"align_posteriors: ", b"align_posteriors_compact: ", b"align_label_posteriors_compact: "):
            assert calls[who](need - 1) == 1
            assert lib.tdnnf_last_error().startswith(who) and b"workspace" in lib.tdnnf_last_error() and str(need).encode() in lib.tdnnf_last_error()
            assert calls[who](need) == 0


# ------------------------------------------------------------------------------------------------------------------------- the keyword
def test_python_keyword(pkg, hip, mixed):
    abi = pkg.hipabi
    ag, y, frames, rows, base = mixed
    same = lambda a, b: np.array_equal(host(a).view(np.int32), host(b).view(np.int32))
    with abi.option(OPT, 3):
        want = ag.posteriors_compact(y, frames, rows, 1, MIXED_GRAPH, 0.3, 0.25)
        want_bytes = ag.posteriors_workspace_bytes(MIXED_GRAPH, frames)
    assert _option(pkg) == 0
    got = ag.posteriors_compact(y, frames, rows, 1, MIXED_GRAPH, 0.3, 0.25, checkpoint=3)
    assert _option(pkg) == 0
    assert same(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(host(got[2]).view(np.int64), host(want[2]).view(np.int64))
    assert np.array_equal(host(got[0]).view(np.int32), np.concatenate([x[2].reshape(-1) for x in base["compact"]]).view(np.int32))
    assert ag.posteriors_workspace_bytes(MIXED_GRAPH, frames, checkpoint=3) == want_bytes < ag.posteriors_workspace_bytes(MIXED_GRAPH, frames)
    with abi.option(OPT, 5):  # the keyword restores what it found, also when the call raises; None leaves the option alone
        assert ag.posteriors_workspace_bytes(MIXED_GRAPH, frames, checkpoint=None) == _formula(ag, frames, MIXED_GRAPH, 5, False)
        for call in (lambda: ag.posteriors_compact(y, frames, rows, 1, MIXED_GRAPH, checkpoint=-2),
                     lambda: ag.posteriors(y, frames, rows, 1, MIXED_GRAPH, checkpoint=-2),
                     lambda: ag.label_posteriors_compact(y, frames, rows, 1, MIXED_GRAPH, checkpoint=-2),
                     lambda: ag.posteriors_sparse(y, frames, rows, 1, MIXED_GRAPH, checkpoint=-2),
                     lambda: ag.label_posteriors_sparse(y, frames, rows, 1, MIXED_GRAPH, checkpoint=-2)):
            with pytest.raises(abi.HipAbiError, match=OPT):
                call()
            assert _option(pkg) == 5
        for c in (0, 3):
            dense = ag.posteriors(y, frames, rows, 1, MIXED_GRAPH, 0.3, 0.25, checkpoint=c)
            label = ag.label_posteriors_compact(y, frames, rows, 1, MIXED_GRAPH, 0.3, 0.25, checkpoint=c)
            assert _option(pkg) == 5
            for u, T in enumerate(frames):
                assert np.array_equal(host(dense[0])[rows[u]:rows[u] + T].view(np.int32), base["dense"][u][2].view(np.int32))
            assert np.array_equal(host(label[0]).view(np.int32), np.concatenate([x[2].reshape(-1) for x in base["label"]]).view(np.int32))
    assert _option(pkg) == 0
    # the same keyword through infer
    outs = [y[rows[u]:rows[u] + T] for u, T in enumerate(frames) if T]
    sub = [g for g, T in zip(MIXED_GRAPH, frames) if T]
    a = pkg.infer.posteriors_compact(outs, ag, utt_graph=sub, acoustic_scale=0.3, weight=0.25, checkpoint=-1)
    b = pkg.infer.posteriors_compact(outs, ag, utt_graph=sub, acoustic_scale=0.3, weight=0.25)
    for x, z in zip(a, b):
        assert same(x[1], z[1]) and x[2] == z[2] and x[3] == z[3]
    assert _option(pkg) == 0
