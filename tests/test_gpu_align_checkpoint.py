"""-m gpu: back-pointer checkpointing of the best path (option align_path_checkpoint; csrc/align_kernels.h align_best_path_ckpt_kernel and
align_path_labels_ckpt_kernel, the plan in csrc/align_tables.h; include/tdnnf_hip.h "best-path alignment").

The bar is EQUALITY: the trace-back recomputes a segment's back-pointers from its checkpoint by the forward pass's own step -- max and + in
double on the same operands in the same order -- so under align_path_checkpoint = C every pdf, state, label, arc, score and ok flag equals
what option 0 gives (torch.equal; the results as int64 bit patterns) -- on every launch form (thread counts, vectors in LDS or in the
workspace, rows staged or not) and for the intervals that reach every branch of the schedule.  So that the code is not only compared
with itself, the option-0 result of every case is also held to tests/viterbi_ref64.py, bit for bit, as tests/test_gpu_align.py holds it.

Every call runs in a workspace allocated at the size option 0 needs (or the checkpointed size, where that is the larger) plus a tail,
filled with a byte pattern, and is told the size of the option it runs under: the pattern beyond that size must survive, so a kernel that
still indexed back-pointers by frame shows as a failed assertion inside the allocation.  Both sizes are held to the byte to the formulas of
include/tdnnf_hip.h restated in _formula.  Outputs lie between canaries over a sentinel."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import viterbi_ref64 as V
from tests.gpu_util import Hip, dev, host, padded

pytestmark = pytest.mark.gpu
F = np.float32
NINF = -np.inf
GUARD, CANARY, SENTINEL, PATTERN = 16, 123, -7, 0xA5
OPT = "align_path_checkpoint"


@pytest.fixture(scope="module")
def hip(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return Hip(pkg)


def _with_labels(g):
    """a labelling that is neither the pdfs nor the arcs: the pdfs 2k and 2k + 1 share the labels 2k and 2k + 1, which an arc takes by the
    parity of its index, shifted by 3 so that no label is its arc's pdf throughout"""
    pdf = np.asarray(g["pdf"])
    return dict(g, label=((pdf // 2) * 2 + np.arange(len(pdf)) % 2 + 3).astype(np.int32), L=(int(g["P"]) + 1) // 2 * 2 + 3)


def _handle(pkg, graphs):
    graphs = [_with_labels(g) for g in ([graphs] if isinstance(graphs, dict) else graphs)]
    return graphs, pkg.hipabi.AlignGraphs(graphs, num_labels=max(g["L"] for g in graphs))


def _graph_of(ag, utt_graph, u):
    return utt_graph[u] if utt_graph is not None else (0 if ag.G == 1 else u)


def _interval(c, frames):
    """the interval of the call: -1 the least C with C * C >= the longest utterance; at most that utterance, at least 1"""
    longest = max(max(frames), 1)
    return min(math.isqrt(longest - 1) + 1 if longest > 1 else 1, longest) if c == -1 else min(c, longest)


def _up(n, m):
    return -(-n // m) * m


def _formula(ag, frames, utt_graph, c, workspace_form):
    """bytes of tdnnf_align_workspace_bytes, from the header: option 0, and option align_path_checkpoint = c"""
    S = [ag.num_states[_graph_of(ag, utt_graph, u)] for u in range(len(frames))]
    head = 16 + _up(32 * len(frames), 256) + (16 * sum(S) if workspace_form else 0)
    if c == 0:
        return head + 4 * sum(_up(T * s, 2) for T, s in zip(frames, S))
    c = _interval(c, frames)
    return head + sum(8 * -(-T // c) * s + 4 * _up(min(c, T) * s, 2) + 4 * _up(T, 2) for T, s in zip(frames, S))


def _guarded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
    buf[:GUARD] = CANARY
    buf[GUARD + n:] = CANARY
    return buf


def _inner(buf, n, what):
    b = host(buf)
    assert (b[:GUARD] == CANARY).all() and (b[GUARD + n:] == CANARY).all(), "the call wrote outside its " + what
    assert not (b[GUARD:GUARD + n] == SENTINEL).any(), "an element of " + what + " was not written"
    return torch.from_numpy(b[GUARD:GUARD + n].copy())


def _calls(pkg, ag, y, frames, rows, stride, utt_graph, c, workspace_form, scale=1.0):
    """tdnnf_align_best_path and tdnnf_align_best_path_labels under align_path_checkpoint = c, each in a patterned workspace that it is
    told to be of the size the option asks for, on guarded outputs.  Returns {"pdf", "state", "label", "arc", "results" (int64 bits)} as
    CPU tensors; the two calls' shared outputs must agree."""
    abi, lib = pkg.hipabi, pkg.hipabi.load()
    n, total = len(frames), int(sum(frames))
    fr, rb = abi.iarr(frames), abi.iarr(rows)
    ug = abi.iarr(utt_graph) if utt_graph is not None else (None, None)
    with abi.option(OPT, 0):
        nbytes0 = ag.workspace_bytes(utt_graph, frames)
        assert nbytes0 == _formula(ag, frames, utt_graph, 0, workspace_form), (nbytes0, _formula(ag, frames, utt_graph, 0, workspace_form))
    out = {}
    with abi.option(OPT, c):
        nbytes = ag.workspace_bytes(utt_graph, frames)
        assert nbytes == _formula(ag, frames, utt_graph, c, workspace_form), (nbytes, c, _formula(ag, frames, utt_graph, c, workspace_form))
        assert nbytes % 8 == 0
        for labels in (False, True):
            ws = torch.full((GUARD + max(nbytes0, nbytes) + 4 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
            assert ws.data_ptr() % 16 == 0
            pdf, state, res = _guarded(total, torch.int32), _guarded(total + n, torch.int32), _guarded(2 * n, torch.float64)
            if labels:
                label, arc = _guarded(total, torch.int32), _guarded(total, torch.int32)
                abi.check(lib.tdnnf_align_best_path_labels(ag.h, n, ug[1], fr[1], rb[1], int(stride), abi.pmat(y), float(scale), abi.ptr(pdf[GUARD:]),
                                                           abi.ptr(state[GUARD:]), abi.ptr(label[GUARD:]), abi.ptr(arc[GUARD:]), abi.ptr(res[GUARD:]),
                                                           abi.ptr(ws[GUARD:]), nbytes, abi.stream()))
            else:
                abi.check(lib.tdnnf_align_best_path(ag.h, n, ug[1], fr[1], rb[1], int(stride), abi.pmat(y), float(scale), abi.ptr(pdf[GUARD:]),
                                                    abi.ptr(state[GUARD:]), abi.ptr(res[GUARD:]), abi.ptr(ws[GUARD:]), nbytes, abi.stream()))
            b = host(ws)
            assert (b[:GUARD] == PATTERN).all() and (b[GUARD + nbytes:] == PATTERN).all(), "the call wrote beyond the workspace it was given"
            got = dict(pdf=_inner(pdf, total, "pdf_out"), state=_inner(state, total + n, "state_out"),
                       results=_inner(res, 2 * n, "results").view(torch.int64))
            if labels:
                got.update(label=_inner(label, total, "label_out"), arc=_inner(arc, total, "arc_out"))
                for k in ("pdf", "state", "results"):
                    assert torch.equal(got[k], out[k]), "the labelled call's %s differs from the plain call's" % k
            out.update(got)
    return out


def _equal(got, base, what=""):
    for k in ("pdf", "state", "label", "arc", "results"):
        assert got[k].dtype == base[k].dtype and torch.equal(got[k], base[k]), (what, k, got[k], base[k])


def _reference(ag, graphs, ys, utt_graph, base, scale=1.0):
    """the option-0 result against tests/viterbi_ref64.py, bit for bit; returns the references"""
    res = base["results"].view(torch.float64).numpy().reshape(-1, 2)
    refs, p0 = [], 0
    for u, yu in enumerate(ys):
        gi = _graph_of(ag, utt_graph, u)
        g, T = graphs[gi], len(yu)
        ref = V.best_path(g, yu, scale)
        what = "utterance %d" % u
        assert res[u, 1] == (1.0 if ref["ok"] else 0.0), what
        assert np.array_equal(res[u, :1].view(np.int64), np.asarray([ref["score"]], np.float64).view(np.int64)), (what, res[u, 0], ref["score"])
        assert np.array_equal(base["pdf"][p0:p0 + T].numpy(), ref["pdfs"]), what
        assert np.array_equal(base["state"][p0 + u:p0 + u + T + 1].numpy(), ref["states"]), what
        arcs = base["arc"][p0:p0 + T].numpy()
        assert np.array_equal(np.where(arcs >= 0, arcs - int(ag.arc_begin[gi]), -1), ref["arcs"]), what
        assert np.array_equal(base["label"][p0:p0 + T].numpy(), np.where(ref["arcs"] >= 0, g["label"][np.maximum(ref["arcs"], 0)], -1)), what
        refs.append(ref)
        p0 += T
    return refs


def _stacked(ys, P):
    frames = [len(y) for y in ys]
    rows = np.concatenate([[0], np.cumsum(frames)[:-1]])
    return dev(np.concatenate(ys) if sum(frames) else np.zeros((1, P), F)), frames, rows


def _case(pkg, graphs, ys, intervals, utt_graph=None, workspace_form=False, scale=1.0):
    """option 0 once, held to the reference; then every interval against it"""
    graphs, ag = _handle(pkg, graphs)
    y, frames, rows = _stacked(ys, ag.P)
    base = _calls(pkg, ag, y, frames, rows, 1, utt_graph, 0, workspace_form, scale)
    refs = _reference(ag, graphs, ys, utt_graph, base, scale)
    for c in intervals:
        _equal(_calls(pkg, ag, y, frames, rows, 1, utt_graph, c, workspace_form, scale), base, "C = %d" % c)
    return graphs, ag, base, refs


def _transcripts(pkg, P=40):
    rng = np.random.default_rng(11)
    seqs = [rng.integers(0, P, size=n).tolist() for n in (1, 5, 17)]
    return [pkg.synth.make_alignment_graph(seqs[0], num_pdfs=P, seed=1),
            pkg.synth.make_alignment_graph(seqs[1], optional=[1, 4], alternatives={2: [7, 8]}, num_pdfs=P, seed=2),
            pkg.synth.make_alignment_graph(seqs[2], optional=[0, 9], alternatives={3: [1], 16: [2, 3, 4]}, num_pdfs=P, seed=3)]


def _option(pkg, name=OPT):
    v = C.c_int()
    pkg.hipabi.check(pkg.hipabi.load().tdnnf_get_option(name.encode(), C.byref(v)))
    return v.value


# ------------------------------------------------------------------------------------------------------------------------- the schedule
MIXED_FRAMES, MIXED_GRAPH = (0, 1, 7, 23, 12), [2, 0, 1, 0, 1]


@pytest.fixture(scope="module")
def mixed(pkg, hip):
    """transcript graphs, five utterances with two pairs sharing a graph: the option-0 call, held to the reference once.  (The 23 frames
    go through the one-unit graph and the 12 through the five-unit one: both have a path; the 0 frames on the 17-unit graph have none.)"""
    graphs, ag = _handle(pkg, _transcripts(pkg))
    rng = np.random.default_rng(5)
    ys = [rng.standard_normal((T, 40)).astype(F) * 3 for T in MIXED_FRAMES]
    y, frames, rows = _stacked(ys, ag.P)
    base = _calls(pkg, ag, y, frames, rows, 1, MIXED_GRAPH, 0, False, F(0.3))
    refs = _reference(ag, graphs, ys, MIXED_GRAPH, base, F(0.3))
    assert [r["ok"] for r in refs] == [False, True, True, True, True]
    return ag, y, frames, rows, base


@pytest.mark.parametrize("c", [1, 2, 3, 7, 22, 23, 24, 100, -1])
def test_mixed_call_every_interval(pkg, hip, mixed, c):
    """frames (0, 1, 7, 23, 12): C = 1 (one-frame segments), 2 and 3 (a one-frame last segment at 7 and 23 / at 7), 7 (C = T and C
    dividing nothing else), 22 = T - 1, 23 = T, 24 = T + 1, 100 beyond every utterance (one segment, nothing recomputed), -1 (5).  The
    labelled call runs beside the plain one in every case (_calls)."""
    ag, y, frames, rows, base = mixed
    got = _calls(pkg, ag, y, frames, rows, 1, MIXED_GRAPH, c, False, F(0.3))
    _equal(got, base)
    if c == 3:
        _equal(_calls(pkg, ag, y, frames, rows, 1, MIXED_GRAPH, c, False, F(0.3)), got)  # two identical calls


@pytest.mark.parametrize("S", [64, 65, 1024, 1025])
def test_block_size_boundaries_cyclic(pkg, hip, S):
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(S, 50, mean_out_degree=4.0, seed=S))
    rng = np.random.default_rng(S)
    _, _, _, refs = _case(pkg, g, [rng.standard_normal((T, 50)).astype(F) for T in (9, 4)], [4])
    assert all(r["ok"] for r in refs)


@pytest.mark.parametrize("S", [9600, 9601])
def test_state_vector_threshold(pkg, hip, S):
    """two LDS vectors up to 9 600 states, the workspace form above (the checkpoints are copied from the workspace vectors); three
    segments, the last of one frame"""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(S, 50, mean_out_degree=3.0, seed=S))
    rng = np.random.default_rng(S)
    _, _, _, refs = _case(pkg, g, [rng.standard_normal((T, 50)).astype(F) for T in (5, 3)], [2], workspace_form=S > 9600)
    assert all(r["ok"] for r in refs)


@pytest.mark.parametrize("form", [1, 2])
def test_both_forms(pkg, hip, form):
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(H=300, P=50))
    rng = np.random.default_rng(9)
    with pkg.hipabi.option("align_form", form):
        _case(pkg, g, [rng.standard_normal((T, 50)).astype(F) * 4 for T in (10, 4)], [3], workspace_form=form == 2)


@pytest.mark.parametrize("S,P", [(30, 512), (30, 513), (100, 2048), (100, 2049)])
def test_row_staging_threshold(pkg, hip, S, P):
    """rows staged in LDS (primed again at every segment the trace-back reruns) and gathered from global memory: T = 7, C = 3"""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(S, P, mean_out_degree=6.0, seed=P))
    assert g["pdf"].max() > P - 40  # (pdfs near the end of the row are on arcs)
    rng = np.random.default_rng(P)
    _case(pkg, g, [rng.standard_normal((T, P)).astype(F) for T in (7, 1, 2)], [3])


def test_heavy_row(pkg, hip):
    """one state with 300 incoming arcs: a wave takes the row; integer scores, so many of its arcs tie.  C = 2"""
    rng = np.random.default_rng(300)
    S, deg = 100, 300
    heavy = S // 2
    src = np.concatenate([rng.integers(0, S, size=deg), np.arange(S), rng.integers(0, S, size=2 * S)]).astype(np.int32)
    dst = np.concatenate([np.full(deg, heavy), (np.arange(S) + 1) % S, rng.integers(0, S, size=2 * S)]).astype(np.int32)
    perm = rng.permutation(len(src))
    g = {"S": S, "P": 6, "src": src[perm], "dst": dst[perm], "pdf": rng.integers(0, 6, size=len(src)).astype(np.int32),
         "logprob": rng.integers(-2, 1, size=len(src)).astype(F), "init": np.zeros(S, F), "final": np.where(np.arange(S) == heavy, 0, NINF).astype(F)}
    assert pkg.hipabi.AlignGraphs(g).info()["max_in_degree"] >= deg
    _, _, _, refs = _case(pkg, g, [rng.integers(-1, 2, size=(T, 6)).astype(F) for T in (7, 3)], [2])
    assert refs[0]["ok"] and refs[0]["states"][-1] == heavy


def test_ties(pkg, hip):
    """parallel arcs of equal score, two equal final states, rows of constant y: every choice is a tie"""
    rng = np.random.default_rng(21)
    S, A, P = 7, 60, 4
    g = {"S": S, "P": P, "src": rng.integers(0, S, size=A).astype(np.int32), "dst": rng.integers(0, S, size=A).astype(np.int32),
         "pdf": rng.integers(0, P, size=A).astype(np.int32), "logprob": np.zeros(A, F), "init": np.zeros(S, F),
         "final": np.where(np.arange(S) >= S - 2, 0, NINF).astype(F)}
    two = {"S": 2, "P": 3, "src": np.asarray([0, 0, 1], np.int32), "dst": np.asarray([1, 1, 1], np.int32), "pdf": np.asarray([0, 1, 2], np.int32),
           "logprob": np.asarray([-1, -1, 0], F), "init": np.asarray([0, NINF], F), "final": np.asarray([NINF, 0], F)}
    ys = [np.full((12, P), 0.5, F), np.full((5, P), 0.5, F)]
    _, _, base, refs = _case(pkg, [g, two], ys, [1, 2, 5, -1])
    assert all(r["ok"] for r in refs) and refs[0]["states"][-1] == S - 2 and list(refs[1]["pdfs"]) == [0, 2, 2, 2, 2]


# ------------------------------------------------------------------------------------------------------------------------- ok = 0
def test_failed_utterances_leave_neighbours_alone(pkg, hip):
    """an utterance too short for its graph, one with +inf in a row and one with a row of NaN: ok = 0 and -1s, under the option as without
    it; the other utterances have the bits they have in a call of their own"""
    rng = np.random.default_rng(8)
    ys = [rng.standard_normal((T, 40)).astype(F) for T in (12, 2, 30, 9, 10)]  # graph 1 needs at least 3 frames
    ys[3][5, :] = np.inf
    ys[4][6, :] = np.nan
    ug = [0, 1, 2, 0, 1]
    graphs, ag, base, refs = _case(pkg, _transcripts(pkg), ys, [3, -1], utt_graph=ug)
    assert [r["ok"] for r in refs] == [True, False, True, False, False]
    assert refs[1]["score"] == NINF and refs[3]["score"] == np.inf and refs[4]["score"] == NINF
    y, frames, rows = _stacked(ys, ag.P)
    got = _calls(pkg, ag, y, frames, rows, 1, ug, 3, False)
    res = got["results"].view(torch.float64).numpy().reshape(-1, 2)
    assert res[:, 1].tolist() == [1.0, 0.0, 1.0, 0.0, 0.0]
    begin = np.concatenate([[0], np.cumsum(frames)])
    for u in (1, 3, 4):
        for k in ("pdf", "label", "arc"):
            assert (got[k][begin[u]:begin[u + 1]] == -1).all()
        assert (got["state"][begin[u] + u:begin[u + 1] + u + 1] == -1).all()
    y2, frames2, rows2 = _stacked([ys[0], ys[2]], ag.P)
    alone = _calls(pkg, ag, y2, frames2, rows2, 1, [0, 2], 3, False)
    for k in ("pdf", "label", "arc"):
        assert torch.equal(alone[k], torch.cat([got[k][begin[0]:begin[1]], got[k][begin[2]:begin[3]]]))
    assert torch.equal(alone["state"], torch.cat([got["state"][begin[0]:begin[1] + 1], got["state"][begin[2] + 2:begin[3] + 3]]))
    assert torch.equal(alone["results"], torch.cat([got["results"][0:2], got["results"][4:6]]))


# ------------------------------------------------------------------------------------------------------------------------- layouts
def test_strided_call_on_views(pkg, hip):
    """t-major rows (row_stride = B) in a sub-matrix view of nnet_output"""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(H=90, P=20, mean_out_degree=5.0, seed=2))
    graphs, ag = _handle(pkg, g)
    rng = np.random.default_rng(4)
    B, frames = 3, [11, 5, 8]
    tmajor = rng.standard_normal((max(frames) * B, 20)).astype(F)
    ys = [tmajor[u::B][:frames[u]] for u in range(B)]
    view, _ = padded(tmajor)
    assert view.stride(0) > view.shape[1]
    base = _calls(pkg, ag, view, frames, np.arange(B), B, None, 0, False)
    _reference(ag, graphs, ys, None, base)
    for c in (3, -1):
        _equal(_calls(pkg, ag, view, frames, np.arange(B), B, None, c, False), base)
    y, _, rows = _stacked(ys, ag.P)
    _equal(_calls(pkg, ag, y, frames, rows, 1, None, 3, False), base)  # the same data concatenated


# ------------------------------------------------------------------------------------------------------------------------- a long utterance
def test_long_utterance(pkg, hip):
    """4 000 frames on a 301-state transcript graph at -1 (C = 64, 63 segments): the workspace is the formula's, below a tenth of option 0's
    (about 0.25 MB against 4.8 MB by the formula: a condition it meets with room, not a measurement)"""
    rng = np.random.default_rng(40)
    g = pkg.synth.make_alignment_graph(rng.integers(0, 50, size=300).tolist(), num_pdfs=50, seed=5)
    assert g["S"] == 301
    T = 4000
    graphs, ag, base, refs = _case(pkg, g, [rng.standard_normal((T, 50)).astype(F)], [-1])
    assert refs[0]["ok"] and _interval(-1, [T]) == 64
    want = _formula(ag, [T], None, -1, False)
    assert want == 16 + 256 + 8 * 63 * 301 + 4 * 64 * 301 + 4 * T
    assert ag.workspace_bytes(None, [T], checkpoint=-1) == want and ag.workspace_bytes(None, [T], checkpoint=0) == 16 + 256 + 4 * T * 301
    assert 10 * want < ag.workspace_bytes(None, [T], checkpoint=0)


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(pkg, hip, mixed):
    abi, lib = pkg.hipabi, hip.lib
    ag, y, frames, rows, base = mixed
    n, total = len(frames), sum(frames)
    fr, rb, ug = abi.iarr(frames), abi.iarr(rows), abi.iarr(MIXED_GRAPH)
    pdf, lab = torch.full((total,), -9, dtype=torch.int32, device="cuda"), torch.full((total,), -9, dtype=torch.int32, device="cuda")
    res = torch.full((n, 2), -5.0, dtype=torch.float64, device="cuda")
    with abi.option(OPT, 0):
        big = 2 * ag.workspace_bytes(MIXED_GRAPH, frames)
    ws = hip.ws(big)
    common = (ag.h, n, ug[1], fr[1], rb[1], 1, abi.pmat(y), 1.0, abi.ptr(pdf), None)
    calls = {b"align_best_path: ": lambda nb: lib.tdnnf_align_best_path(*common, abi.ptr(res), abi.ptr(ws), nb, abi.stream()),
             b"align_best_path_labels: ": lambda nb: lib.tdnnf_align_best_path_labels(*common, abi.ptr(lab), None, abi.ptr(res), abi.ptr(ws), nb,
                                                                                      abi.stream())}
    for bad in (-2, -7):
        with abi.option(OPT, bad):
            assert ag.workspace_bytes(MIXED_GRAPH, frames) == 0
            assert OPT.encode() in lib.tdnnf_last_error() and str(bad).encode() in lib.tdnnf_last_error()
            for who, call in calls.items():
                assert call(big) == 1, who
                e = lib.tdnnf_last_error()
                assert e.startswith(who) and OPT.encode() in e and str(bad).encode() in e, (who, e)
            for m in (lambda: ag.best_path(y, frames, rows, 1, MIXED_GRAPH), lambda: ag.best_path_labels(y, frames, rows, 1, MIXED_GRAPH)):
                with pytest.raises(abi.HipAbiError, match=OPT):
                    m()
    torch.cuda.synchronize()
    assert (host(pdf) == -9).all() and (host(lab) == -9).all() and (host(res) == -5.0).all()  # nothing was launched
    # a workspace one byte short of the checkpointed size
    with abi.option(OPT, 3):
        need = ag.workspace_bytes(MIXED_GRAPH, frames)
        assert 0 < need < big
        for who, call in calls.items():
            assert call(need - 1) == 1
            e = lib.tdnnf_last_error()
            assert e.startswith(who) and b"workspace" in e and str(need).encode() in e, e
            assert call(need) == 0
    torch.cuda.synchronize()
    assert torch.equal(pdf.cpu(), base["pdf"]) and torch.equal(lab.cpu(), base["label"])


# ------------------------------------------------------------------------------------------------------------------------- the two options
def test_option_isolation(pkg, hip, mixed):
    """align_checkpoint (the posteriors' option) reaches neither the best path's workspace nor its result; align_path_checkpoint reaches
    no posterior workspace"""
    abi = pkg.hipabi
    ag, y, frames, rows, base = mixed
    n0 = ag.workspace_bytes(MIXED_GRAPH, frames)
    post = [ag.posteriors_workspace_bytes(MIXED_GRAPH, frames), ag.posteriors_workspace_bytes(MIXED_GRAPH, frames, False),
            ag.posteriors_sparse_workspace_bytes(MIXED_GRAPH, frames, 4), ag.label_posteriors_sparse_workspace_bytes(MIXED_GRAPH, frames, 4)]
    assert n0 == _formula(ag, frames, MIXED_GRAPH, 0, False) and all(v > 0 for v in post)
    for v in (3, -1, -2):  # (-2: a value its own calls refuse)
        with abi.option("align_checkpoint", v):
            assert ag.workspace_bytes(MIXED_GRAPH, frames) == n0
            _equal(_calls(pkg, ag, y, frames, rows, 1, MIXED_GRAPH, 0, False, F(0.3)), base)
            _equal(_calls(pkg, ag, y, frames, rows, 1, MIXED_GRAPH, 3, False, F(0.3)), base)
        with abi.option(OPT, v):
            assert [ag.posteriors_workspace_bytes(MIXED_GRAPH, frames), ag.posteriors_workspace_bytes(MIXED_GRAPH, frames, False),
                    ag.posteriors_sparse_workspace_bytes(MIXED_GRAPH, frames, 4),
                    ag.label_posteriors_sparse_workspace_bytes(MIXED_GRAPH, frames, 4)] == post
    assert _option(pkg) == 0 and _option(pkg, "align_checkpoint") == 0


# ------------------------------------------------------------------------------------------------------------------------- the keyword
def test_python_keyword(pkg, hip, mixed):
    abi = pkg.hipabi
    ag, y, frames, rows, base = mixed
    assert _option(pkg) == 0
    for c in (0, 3, -1):
        pdfs, states, res = ag.best_path(y, frames, rows, 1, MIXED_GRAPH, 0.3, states=True, checkpoint=c)
        assert _option(pkg) == 0
        assert torch.equal(pdfs.cpu(), base["pdf"]) and torch.equal(states.cpu(), base["state"])
        assert torch.equal(res.cpu().reshape(-1).view(torch.int64), base["results"])
        pdfs, states, res, lab, arcs = ag.best_path_labels(y, frames, rows, 1, MIXED_GRAPH, 0.3, states=True, checkpoint=c)
        assert _option(pkg) == 0
        assert torch.equal(pdfs.cpu(), base["pdf"]) and torch.equal(states.cpu(), base["state"]) and torch.equal(lab.cpu(), base["label"])
        first = np.repeat(ag.arc_begin[np.asarray(MIXED_GRAPH)], frames)
        assert np.array_equal(host(arcs), np.where(base["arc"].numpy() >= 0, base["arc"].numpy() - first, -1))
    assert ag.workspace_bytes(MIXED_GRAPH, frames, checkpoint=3) == _formula(ag, frames, MIXED_GRAPH, 3, False)
    assert ag.workspace_bytes(MIXED_GRAPH, frames) == _formula(ag, frames, MIXED_GRAPH, 0, False)
    with abi.option(OPT, 5):  # the keyword restores what it found, also when the call raises; None reads the standing value
        assert ag.workspace_bytes(MIXED_GRAPH, frames, checkpoint=None) == _formula(ag, frames, MIXED_GRAPH, 5, False)
        assert ag.workspace_bytes(MIXED_GRAPH, frames, checkpoint=0) == _formula(ag, frames, MIXED_GRAPH, 0, False)
        assert ag.workspace_bytes(MIXED_GRAPH, frames, checkpoint=-2) == 0
        for call in (lambda: ag.best_path(y, frames, rows, 1, MIXED_GRAPH, checkpoint=-2),
                     lambda: ag.best_path_labels(y, frames, rows, 1, MIXED_GRAPH, checkpoint=-2)):
            with pytest.raises(abi.HipAbiError, match=OPT):
                call()
            assert _option(pkg) == 5
        pdfs, _, _ = ag.best_path(y, frames, rows, 1, MIXED_GRAPH, 0.3)
        assert torch.equal(pdfs.cpu(), base["pdf"]) and _option(pkg) == 5
    assert _option(pkg) == 0
    # the same keyword through infer
    outs = [y[rows[u]:rows[u] + T] for u, T in enumerate(frames) if T]
    sub = [g for g, T in zip(MIXED_GRAPH, frames) if T]
    a = pkg.infer.align(outs, ag, utt_graph=sub, acoustic_scale=0.3, checkpoint=-1)
    b = pkg.infer.align(outs, ag, utt_graph=sub, acoustic_scale=0.3)
    for x, z in zip(a, b):
        assert torch.equal(x[0], z[0]) and x[1] == z[1] and x[2] == z[2]
    a = pkg.infer.align_labels(outs, ag, utt_graph=sub, acoustic_scale=0.3, checkpoint=2)
    b = pkg.infer.align_labels(outs, ag, utt_graph=sub, acoustic_scale=0.3)
    for x, z in zip(a, b):
        assert all(torch.equal(p, q) for p, q in zip(x[:3], z[:3])) and x[3:] == z[3:]
    assert _option(pkg) == 0


def test_acoustic_model_keyword(pkg, hip):
    """AcousticModel.align / align_labels with the tiny model: checkpoint= gives the path option 0 gives and restores the option"""
    from tests.test_gpu_infer import SMALL, make_model, utterances
    cfg, net = make_model(pkg, SMALL)
    model = pkg.infer.AcousticModel(net, frames_per_chunk=24)
    rng = np.random.default_rng(17)
    utts = utterances(rng, [50, 7, 95])
    P = cfg.num_pdfs
    graphs, ag = _handle(pkg, [pkg.synth.make_alignment_graph(rng.integers(0, P, size=k).tolist(), optional=[1], num_pdfs=P, seed=k) for k in (6, 2, 40)])
    a0, l0 = model.align(utts, ag), model.align_labels(utts, ag)
    assert [x[2] for x in a0] == [True, True, False]
    for c in (0, 4, -1):
        a, l = model.align(utts, ag, checkpoint=c), model.align_labels(utts, ag, checkpoint=c)
        assert _option(pkg) == 0
        for x, z in zip(a, a0):
            assert torch.equal(x[0], z[0]) and x[1] == z[1] and x[2] == z[2]
        for x, z in zip(l, l0):
            assert all(torch.equal(p, q) for p, q in zip(x[:3], z[:3])) and x[3:] == z[3:]
    with pkg.hipabi.option(OPT, 4):
        a = model.align(utts, ag, checkpoint=None)
    assert all(torch.equal(x[0], z[0]) for x, z in zip(a, a0))
