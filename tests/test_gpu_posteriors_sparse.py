"""-m gpu: the sparse posteriors (tdnnf_align_posteriors_sparse, csrc/align_sparse.hip; include/tdnnf_hip.h "sparse posteriors").

The bar is EQUALITY with tests/posteriors_sparse_ref.py applied to what tdnnf_align_posteriors_compact writes on the same inputs: the
sparse call is defined as a function of those floats, so pdf, post (as bits), count and results[:, 2:4] equal the reference's, and
results[:, 0:2] have the compact call's bits.  So that the code is not only compared with the library's own compact pass, one case holds
the kept pairs and the dropped ones to tests/posteriors_ref64.py at the dense call's bar (one float32 ulp at `weight`).
Every output lies between canaries and is pre-filled with a sentinel no result can be: the canaries must survive, and equality with the
reference shows that every slot and count was written though nothing is zeroed first."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import posteriors_ref64 as PR
from tests.gpu_util import Hip, dev, host
from tests.posteriors_sparse_ref import sparsify
from tests.test_gpu_posteriors import _transcripts
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


def _inner(buf, n, what):
    b = host(buf)
    assert (b[:GUARD] == CANARY).all() and (b[GUARD + n:] == CANARY).all(), "the call wrote outside its " + what
    return b[GUARD:GUARD + n]


def _sparse_raw(pkg, ag, y, frames, rows, stride, utt_graph, scale, weight, min_post, K):
    """the C call on guarded outputs: (pdf [F, K], post [F, K], count [F], results [U, 4]) downloaded, the canaries checked"""
    abi = pkg.hipabi
    lib = abi.load()
    n, total = len(frames), int(np.sum(frames))
    fr, rb = abi.iarr(frames), abi.iarr(rows)
    ug = abi.iarr(utt_graph) if utt_graph is not None else (None, None)
    nbytes = int(lib.tdnnf_align_posteriors_sparse_workspace_bytes(ag.h, n, ug[1], fr[1], K))
    assert nbytes > 0, lib.tdnnf_last_error()
    ws = abi.workspace(nbytes)
    pdf, post, count = _guarded(total * K, torch.int32), _guarded(total * K, torch.float32), _guarded(total, torch.int32)
    res = _guarded(4 * n, torch.float64)
    abi.check(lib.tdnnf_align_posteriors_sparse(ag.h, n, ug[1], fr[1], rb[1], int(stride), abi.pmat(y), float(scale), float(weight), float(min_post), K,
                                                abi.ptr(pdf[GUARD:]), abi.ptr(post[GUARD:]), abi.ptr(count[GUARD:]), abi.ptr(res[GUARD:]), abi.ptr(ws), nbytes,
                                                abi.stream()))
    return (_inner(pdf, total * K, "pdfs").reshape(total, K), _inner(post, total * K, "values").reshape(total, K), _inner(count, total, "counts"),
            _inner(res, 4 * n, "results").reshape(n, 4))


def _expected(ag, vals, begin, cres, frames, utt_graph, min_post, K):
    """sparsify of the compact call's output, utterance after utterance: (pdf, post, count, results [U, 4], n [F])"""
    parts, res = [], np.zeros((len(frames), 4))
    for u, T in enumerate(frames):
        gi = utt_graph[u] if utt_graph is not None else (0 if ag.G == 1 else u)
        pdfs = ag.pdfs(gi)
        parts.append(sparsify(vals[begin[u]:begin[u + 1]].reshape(T, len(pdfs)), pdfs, min_post, K))
        n = parts[-1][3]
        res[u] = cres[u, 0], cres[u, 1], (n > K).sum(), n.max(initial=0)
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3)) + (res, np.concatenate([p[3] for p in parts]))


def _equal(got, want):
    pdf, post, count, res = got
    assert pdf.dtype == np.int32 and post.dtype == F and count.dtype == np.int32 and res.dtype == np.float64
    assert np.array_equal(count, want[2]), (count, want[2])
    assert np.array_equal(pdf, want[0])
    assert np.array_equal(post.view(np.int32), want[1].view(np.int32))
    assert np.array_equal(res.view(np.int64), want[3].view(np.int64)), (res, want[3])


def _check(pkg, ag, y, frames, rows, stride, utt_graph, scale=1.0, weight=1.0, min_post=0.0, K=16):
    """compact and sparse on the same inputs: the sparse call equals sparsify of the compact one.  Returns (the sparse call's four
    arrays, (values, utt_begin, results) of the compact call, n [F] the candidates of every frame)"""
    y = y if isinstance(y, torch.Tensor) else dev(y)
    comp = _compact_raw(pkg, ag, y, frames, rows, stride, utt_graph, scale, weight)
    got = _sparse_raw(pkg, ag, y, frames, rows, stride, utt_graph, scale, weight, min_post, K)
    want = _expected(ag, comp[0], comp[1], comp[2], frames, utt_graph, F(min_post), K)
    _equal(got, want[:4])
    return got, comp, want[4]


def _stacked(ys, P):
    frames = [len(y) for y in ys]
    rows = np.concatenate([[0], np.cumsum(frames)[:-1]])
    return (np.concatenate(ys) if sum(frames) else np.zeros((1, P), F)), frames, rows  # (a call of zero-frame utterances reads no row)


# ------------------------------------------------------------------------------------------------------------------------- transcript graphs
MIXED_T, MIXED_GRAPH = (37, 0, 1, 5, 37, 1), [2, 0, 1, 1, 0, 0]


@pytest.mark.parametrize("K", [1, 3, 64])
@pytest.mark.parametrize("min_post", [0.0, 0.01])
@pytest.mark.parametrize("scale,weight", [(1.0, 1.0), (0.3, 0.25)])
def test_mixed_call(pkg, hip, scale, weight, min_post, K):
    """three transcript graphs with different column counts, six utterances of 0, 1, 5 and 37 frames -- 37 = 2 groups of 16 and 5, so
    the last workgroup of an utterance has idle waves and a wave idle turns; graphs shared through utt_graph"""
    graphs = _transcripts(pkg)
    ag = pkg.hipabi.AlignGraphs(graphs)
    assert len({len(ag.pdfs(k)) for k in range(3)}) == 3
    rng = np.random.default_rng(5)
    y, frames, rows = _stacked([rng.standard_normal((T, 40)).astype(F) * 3 for T in MIXED_T], 40)
    got, comp, n = _check(pkg, ag, y, frames, rows, 1, MIXED_GRAPH, F(scale), F(weight), min_post, K)
    assert comp[2][:, 1].tolist() == [1.0, 0.0, 0.0, 1.0, 1.0, 1.0]  # (no path of 0 frames; graph 1 needs 3 at least)
    if K == 3:
        assert (n > K).any() and ((n <= K) & (n > 0)).any(), "the inputs must give truncated and untruncated frames"
    if K == 64:
        assert got[3][:, 2].sum() == 0 and got[3][:, 3].max() == n.max() > 3
    # one graph per utterance without utt_graph
    y, frames, rows = _stacked([rng.standard_normal((T, 40)).astype(F) * 3 for T in (5, 37, 20)], 40)
    _check(pkg, ag, y, frames, rows, 1, None, F(scale), F(weight), min_post, K)


@pytest.mark.parametrize("D", [1, 63, 64, 65, 129, 257])
def test_lane_stride_boundaries(pkg, hip, D):
    """column counts at and around the wave's 64 lanes: one stride with idle lanes, exactly one, one column into the second, the third and
    the fifth.  With min_post 0 and K = 64 every frame above 64 columns goes through the cutoff search across several strides; K = 7 and a
    floor run the same graphs with a truncation inside the first stride"""
    ids = 3 + 2 * np.arange(D)  # odd pdfs only
    S = min(D, 40)
    g = _labelled(S, np.concatenate([ids, ids[:D // 2], ids[:7]]), D)
    ag = pkg.hipabi.AlignGraphs(g)
    assert ag.pdfs().tolist() == ids.tolist()
    rng = np.random.default_rng(D)
    y, frames, rows = _stacked([rng.standard_normal((T, g["P"])).astype(F) for T in (18, 3)], g["P"])
    got, _, n = _check(pkg, ag, y, frames, rows, 1, None, weight=F(0.5), min_post=0.0, K=64)
    assert n.max() <= D and (D <= 64) == (got[3][:, 2].sum() == 0)
    if D > 64:
        assert (n > 64).all() and (got[2] == 64).all() and got[3][:, 2].tolist() == [18.0, 3.0]
    _check(pkg, ag, y, frames, rows, 1, None, weight=F(0.5), min_post=1e-3, K=7)


def _tied(seed=0):
    """a ring of 6 states, every state initial and final; from each state to the next five parallel arcs: pdf 2 (the likeliest), pdfs 4, 9
    and 20 with one log-prob, pdf 10 (the least)"""
    S, pdfs, lps = 6, [2, 4, 9, 10, 20], [-0.25, -1.0, -1.0, -3.0, -1.0]
    src = np.repeat(np.arange(S), len(pdfs)).astype(np.int32)
    return {"S": S, "P": 24, "src": src, "dst": ((src + 1) % S).astype(np.int32), "pdf": np.tile(pdfs, S).astype(np.int32),
            "logprob": np.tile(lps, S).astype(F), "init": np.zeros(S, F), "final": np.zeros(S, F)}


def test_ties_at_the_cutoff(pkg, hip):
    """pdfs 4, 9 and 20 sit on parallel arcs of equal log-prob and their output columns are equal, so their posteriors are the same sums
    in the same order: bit-equal values.  pdf 2 lies above them and pdf 10 below in every frame, so K = 2 and 3 cut through the tie"""
    g = _tied()
    ag = pkg.hipabi.AlignGraphs(g)
    assert ag.pdfs().tolist() == [2, 4, 9, 10, 20]
    rng = np.random.default_rng(1)
    T = 9
    y = rng.standard_normal((T, g["P"])).astype(F)
    y[:, 9] = y[:, 20] = y[:, 4]
    y[:, 2], y[:, 10] = y[:, 4] + F(1), y[:, 4] - F(1)
    for K, kept in ((1, [2]), (2, [2, 4]), (3, [2, 4, 9]), (4, [2, 4, 9, 20]), (5, [2, 4, 9, 10, 20])):
        got, comp, n = _check(pkg, ag, y, [T], [0], 1, None, min_post=0.0, K=K)
        block = comp[0].reshape(T, 5)
        tie = block[:, [1, 2, 4]].view(np.int32)
        assert (tie[:, 0] == tie[:, 1]).all() and (tie[:, 0] == tie[:, 2]).all(), "the compact output must hold bit-equal values"
        assert (block[:, 0] > block[:, 1]).all() and (block[:, 1] > block[:, 3]).all() and (block[:, 3] > 0).all() and (n == 5).all()
        assert (got[0] == np.asarray(kept, np.int32)).all() and (got[2] == K).all()
        assert got[3][0, 2:].tolist() == [float(T if K < 5 else 0), 5.0]


def test_no_floor_and_room_for_every_column_gives_every_non_zero(pkg, hip):
    """min_post 0 and K >= D_g: scattering the pairs back reproduces the compact block, zeros where it has zeros"""
    graphs = _transcripts(pkg)
    ag = pkg.hipabi.AlignGraphs(graphs)
    K = 64
    assert max(len(ag.pdfs(k)) for k in range(3)) <= K
    rng = np.random.default_rng(12)
    y, frames, rows = _stacked([rng.standard_normal((T, 40)).astype(F) * 3 for T in (21, 4, 30)], 40)
    (pdf, post, count, res), (vals, begin, _), n = _check(pkg, ag, y, frames, rows, 1, None, min_post=0.0, K=K)
    f = 0
    for u, T in enumerate(frames):
        pdfs = ag.pdfs(u)
        block = vals[begin[u]:begin[u + 1]].reshape(T, len(pdfs))
        back = np.zeros((T, 40), F)
        for t in range(T):
            back[t, pdf[f + t, :count[f + t]]] = post[f + t, :count[f + t]]
        assert np.array_equal(back[:, pdfs].view(np.int32), block.view(np.int32)) and (block >= 0).all()
        f += T
    assert (res[:, 2] == 0).all() and (vals == 0).any() and (count > 0).all()


def test_no_accepting_path_leaves_neighbours_alone(pkg, hip):
    graphs = _transcripts(pkg)
    ag = pkg.hipabi.AlignGraphs(graphs)
    rng = np.random.default_rng(8)
    ys = [rng.standard_normal((T, 40)).astype(F) for T in (12, 2, 30)]  # graph 1 needs at least 3 frames
    y, frames, rows = _stacked(ys, 40)
    (pdf, post, count, res), _, _ = _check(pkg, ag, y, frames, rows, 1, None, min_post=0.01, K=3)
    assert res[1].tolist() == [NINF, 0.0, 0.0, 0.0]
    assert (count[12:14] == 0).all() and (pdf[12:14] == -1).all() and (post[12:14].view(np.int32) == 0).all()
    assert (res[[0, 2], 1] == 1.0).all() and (count[:12] > 0).all() and (count[14:] > 0).all()
    for u, sl in ((0, slice(0, 12)), (2, slice(14, 44))):
        (p1, v1, c1, r1), _, _ = _check(pkg, ag, ys[u], [len(ys[u])], [0], 1, [u], min_post=0.01, K=3)
        assert np.array_equal(p1, pdf[sl]) and np.array_equal(v1.view(np.int32), post[sl].view(np.int32)) and np.array_equal(c1, count[sl])
        assert np.array_equal(r1[0].view(np.int64), res[u].view(np.int64))


def test_call_of_zero_frame_utterances(pkg, hip):
    """no frame: null outputs are accepted and only the results are written"""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(H=70, P=20, mean_out_degree=4.0, seed=6))
    t = pkg.synth.make_alignment_graph([1, 2], num_pdfs=20)
    ag = pkg.hipabi.AlignGraphs([t, g])
    abi, lib = pkg.hipabi, pkg.hipabi.load()
    y = dev(np.zeros((1, 20), F))
    got, comp, _ = _check(pkg, ag, y, [0, 0, 0], [0, 0, 0], 1, [0, 1, 0])
    assert got[3][:, 1:].tolist() == [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    fr, ug = abi.iarr([0, 0, 0]), abi.iarr([0, 1, 0])
    nbytes = int(lib.tdnnf_align_posteriors_sparse_workspace_bytes(ag.h, 3, ug[1], fr[1], 16))
    ws, res = hip.ws(nbytes), torch.full((3, 4), -5.0, dtype=torch.float64, device="cuda")
    abi.check(lib.tdnnf_align_posteriors_sparse(ag.h, 3, ug[1], fr[1], fr[1], 1, abi.pmat(y), 1.0, 1.0, 0.01, 16, None, None, None, hip.vec(res), hip.vec(ws),
                                                nbytes, hip.stream()))
    assert np.array_equal(host(res).view(np.int64), got[3].view(np.int64))
    pdf, post, count, res2 = ag.posteriors_sparse(y, [0, 0, 0], [0, 0, 0], utt_graph=[0, 1, 0])  # the wrapper passes the null outputs itself
    assert tuple(pdf.shape) == tuple(post.shape) == (0, 16) and tuple(count.shape) == (0,) and np.array_equal(host(res2), got[3])


# ------------------------------------------------------------------------------------------------------------------------- layouts, forms
def test_t_major_rows_in_a_guarded_view(pkg, hip):
    """row_stride = B on a t-major minibatch, read through a sub-matrix view whose surrounding columns and rows hold NaN: frame numbering
    follows utt_frames alone, so the outputs are those of the rows concatenated, bit for bit; the outputs' canaries stay (_sparse_raw)"""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(H=90, P=20, mean_out_degree=5.0, seed=2))
    ag = pkg.hipabi.AlignGraphs(g)
    rng = np.random.default_rng(4)
    B, frames, P = 3, [11, 5, 8], 20
    tmajor = rng.standard_normal((max(frames) * B, P)).astype(F)
    y, fr, rows = _stacked([tmajor[u::B][:frames[u]] for u in range(B)], P)
    cat, _, n = _check(pkg, ag, y, fr, rows, 1, [0, 0, 0], min_post=0.05, K=6)
    assert (n > 6).any() and (n <= 6).any()
    buf = torch.full((max(frames) * B + 4, P + 9), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[2:2 + max(frames) * B, 3:3 + P]
    view.copy_(dev(tmajor))
    assert view.stride(0) > view.shape[1] and not torch.isnan(view).any()
    got, _, _ = _check(pkg, ag, view, frames, np.arange(B), B, [0, 0, 0], min_post=0.05, K=6)
    _equal(got, cat)
    # the wrapper: the same values in tensors of the documented shapes
    pdf, post, count, res = ag.posteriors_sparse(view, frames, np.arange(B), row_stride=B, utt_graph=[0, 0, 0], min_post=0.05, max_per_frame=6)
    assert pdf.dtype == torch.int32 and post.dtype == torch.float32 and count.dtype == torch.int32 and res.dtype == torch.float64 and pdf.is_cuda
    assert tuple(pdf.shape) == tuple(post.shape) == (24, 6) and tuple(count.shape) == (24,) and tuple(res.shape) == (B, 4)
    _equal((host(pdf), host(post), host(count), host(res)), cat)


def test_workspace_form_of_the_recursion(pkg, hip):
    """option align_form 2 (the state vectors in the workspace) is read by the recursion inside the call and by the workspace question: the
    selection sees the same block either way"""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(H=300, P=50))
    ag = pkg.hipabi.AlignGraphs(g)
    rng = np.random.default_rng(9)
    y, frames, rows = _stacked([rng.standard_normal((12, 50)).astype(F) * 4 for _ in range(3)], 50)
    res, nbytes = {}, {}
    for form in (1, 2):
        with pkg.hipabi.option("align_form", form):
            res[form], _, _ = _check(pkg, ag, y, frames, rows, 1, [0, 0, 0], min_post=0.01, K=5)
            nbytes[form] = int(hip.lib.tdnnf_align_posteriors_sparse_workspace_bytes(ag.h, 3, None, pkg.hipabi.iarr(frames)[1], 5))
    _equal(res[2], res[1])
    assert nbytes[2] == nbytes[1] + 3 * 2 * 300 * 8


def test_two_calls_give_the_same_bits(pkg, hip):
    graphs = _transcripts(pkg)
    ag = pkg.hipabi.AlignGraphs(graphs)
    rng = np.random.default_rng(21)
    y, frames, rows = _stacked([rng.standard_normal((T, 40)).astype(F) * 3 for T in (33, 17, 40)], 40)
    y = dev(y)
    a = _sparse_raw(pkg, ag, y, frames, rows, 1, None, 1.0, 1.0, 0.0, 2)
    b = _sparse_raw(pkg, ag, y, frames, rows, 1, None, 1.0, 1.0, 0.0, 2)
    _equal(a, b)
    assert a[3][:, 2].sum() > 0


# ------------------------------------------------------------------------------------------------------------------------- the float64 reference
@pytest.mark.parametrize("scale,weight,min_post,K", [(1.0, 1.0, 0.01, 3), (0.3, 0.25, 0.002, 5), (1.0, 1.0, 0.0, 64)])
def test_against_the_float64_reference(pkg, hip, scale, weight, min_post, K):
    """every kept pair lies within one float32 ulp at `weight` of weight x the float64 posterior, and in a frame that was not truncated
    every pdf that was not kept has weight x its float64 posterior <= min_post + that bar; every frame, every pdf"""
    graphs = _transcripts(pkg)
    ag = pkg.hipabi.AlignGraphs(graphs)
    rng = np.random.default_rng(31)
    ys = [rng.standard_normal((T, 40)).astype(F) * 3 for T in (19, 6, 37)]
    y, frames, rows = _stacked(ys, 40)
    (pdf, post, count, res), _, n = _check(pkg, ag, y, frames, rows, 1, None, F(scale), F(weight), min_post, K)
    w = float(F(weight))
    f = truncated = 0
    for u, T in enumerate(frames):
        ref = PR.forward_backward(graphs[u], ys[u], F(scale))
        assert ref["ok"] and res[u, 1] == 1.0 and abs(res[u, 0] - ref["logprob"]) <= 1e-9 * abs(ref["logprob"])
        want = np.zeros((T, 40))
        want[:, :ref["post"].shape[1]] = w * ref["post"]
        for t in range(T):
            c = count[f + t]
            ids = pdf[f + t, :c]
            assert c == min(n[f + t], K) and (np.diff(ids) > 0).all() and (ids >= 0).all()
            assert np.abs(post[f + t, :c].astype(np.float64) - want[t, ids].astype(F)).max(initial=0.0) <= ULP * w
            assert (post[f + t, :c] > F(min_post)).all()
            if n[f + t] <= K:
                rest = np.setdiff1d(np.arange(40), ids)
                assert (want[t, rest] <= float(F(min_post)) + ULP * w).all()
            else:
                truncated += 1
        f += T
    assert (truncated > 0) == (K < 64)


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(pkg, hip):
    lib, abi = hip.lib, pkg.hipabi
    g = pkg.synth.make_alignment_graph([1, 2, 3], num_pdfs=5)
    ag = abi.AlignGraphs(g, num_pdfs=5)
    K = 2
    frames, rows = abi.iarr([4, 6]), abi.iarr([0, 4])
    y = dev(np.zeros((10, 5), F))
    nbytes = int(lib.tdnnf_align_posteriors_sparse_workspace_bytes(ag.h, 2, None, frames[1], K))
    W = ag.posteriors_workspace_bytes(None, [4, 6])
    assert nbytes == 16 + (W + 15) // 16 * 16 + 48 * 2 + 8 * 2 + 4 * 10 * 3  # the formula of include/tdnnf_hip.h
    ws = hip.ws(nbytes)
    pdf, post, count = _guarded(10 * K, torch.int32), _guarded(10 * K, torch.float32), _guarded(10, torch.int32)
    res = _guarded(8, torch.float64)
    outs = dict(pdf=pdf, post=post, count=count)

    def call(k=K, min_post=0.01, nb=nbytes, y_=y, rows_=rows, stride=1, frames_=frames, ug=None, null=None):
        o = {name: (None if name == null else hip.vec(t[GUARD:])) for name, t in outs.items()}
        return lib.tdnnf_align_posteriors_sparse(ag.h, 2, ug, frames_[1], rows_[1], stride, C.byref(y_) if isinstance(y_, abi.Mat) else abi.pmat(y_), 1.0, 1.0, min_post, k,
                                                 o["pdf"], o["post"], o["count"], hip.vec(res[GUARD:]), hip.vec(ws), nb, hip.stream())

    def refused(rc, *words):
        e = lib.tdnnf_last_error()
        assert rc == 1 and e.startswith(b"align_posteriors_sparse: ") and all(w in e for w in words), (rc, e)

    refused(call(k=0), b"max_per_frame")
    refused(call(k=65), b"max_per_frame")
    refused(call(min_post=-1e-6), b"min_post")
    refused(call(min_post=float("nan")), b"min_post")
    refused(call(min_post=float("inf")), b"min_post")
    for name in outs:
        refused(call(null=name), b"null")
    refused(call(nb=nbytes - 1), b"workspace")
    # what the compact call refuses
    refused(call(rows_=abi.iarr([0, 5])), b"rows")  # rows 5 .. 10 of 10
    refused(call(y_=dev(np.zeros((10, 4), F))), b"columns")
    refused(call(stride=0), b"row_stride")
    refused(call(ug=abi.iarr([0, 1])[1]), b"graph")  # graph 1 of 1
    refused(call(frames_=abi.iarr([4, -1])))
    # an utterance whose block starts beyond float 2^31 - 1 of the compact block: 3 columns a frame.  (The matrix is only described, at the
    # size such a call would need: a refused call reads nothing, and the workspace at hand is far too small for it in any case.)
    big = abi.iarr([(1 << 31) // 3 + 1, 1])
    huge = abi.Mat(y.data_ptr(), (1 << 31) // 3 + 2, 5, 5)
    refused(call(frames_=big, rows_=abi.iarr([0, (1 << 31) // 3 + 1]), y_=huge), b"split the call")
    assert lib.tdnnf_align_posteriors_sparse_workspace_bytes(ag.h, 2, None, big[1], K) == 0 and b"split the call" in lib.tdnnf_last_error()
    assert lib.tdnnf_align_posteriors_sparse_workspace_bytes(ag.h, 2, None, frames[1], 0) == 0
    for t, n in ((pdf, 10 * K), (post, 10 * K), (count, 10), (res, 8)):
        assert (_inner(t, n, "buffer") == SENTINEL).all()  # nothing was launched
    assert call() == 0
    r = _inner(res, 8, "results").reshape(2, 4)
    assert (r[:, 1] == 1.0).all() and (_inner(count, 10, "counts") >= 1).all() and (_inner(pdf, 10 * K, "pdfs") != SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------------------- the model
def test_acoustic_model_posteriors_sparse_and_archive(pkg, hip, tmp_path):
    from tests.test_gpu_infer import SMALL, make_model, utterances
    cfg, net = make_model(pkg, SMALL)
    model = pkg.infer.AcousticModel(net, frames_per_chunk=24)
    rng = np.random.default_rng(17)
    utts = utterances(rng, [50, 7, 95])
    P = cfg.num_pdfs
    graphs = [pkg.synth.make_alignment_graph(rng.integers(0, P, size=n).tolist(), optional=[1], num_pdfs=P, seed=n) for n in (6, 2, 40)]
    ag = pkg.hipabi.AlignGraphs(graphs)
    K, floor = 16, 1e-4
    comp = model.posteriors_compact(utts, ag, acoustic_scale=1.0)
    sparse = model.posteriors_sparse(utts, ag, acoustic_scale=1.0, min_post=floor, max_per_frame=K)
    again = pkg.infer.posteriors_sparse(model.compute(utts), ag, acoustic_scale=1.0, min_post=floor, max_per_frame=K)
    assert [s[4] for s in sparse] == [True, True, False] and sparse[2][5] == 0
    for u, (c, s, a) in enumerate(zip(comp, sparse, again)):
        ids, block, lp, ok = c
        pdf, post, count, slp, sok, trunc = s
        assert pdf.dtype == torch.int32 and post.dtype == torch.float32 and count.dtype == torch.int32 and pdf.is_cuda and post.is_cuda and count.is_cuda
        assert tuple(pdf.shape) == tuple(post.shape) == (block.shape[0], K) and tuple(count.shape) == (block.shape[0],)
        want = sparsify(host(block), ids, F(floor), K)
        assert np.array_equal(host(pdf), want[0]) and np.array_equal(host(post).view(np.int32), want[1].view(np.int32)) and np.array_equal(host(count), want[2])
        assert slp == lp and sok == ok and trunc == int((want[3] > K).sum()) and isinstance(trunc, int)
        assert all(np.array_equal(host(x), host(z)) for x, z in zip(s[:3], a[:3])) and s[3:] == a[3:]
    assert sum(s[5] for s in sparse) == 0, "no frame may be truncated for the archives to agree"
    for min_post in (floor, 1e-2):  # the writer's floor is at least the call's
        a, b = tmp_path / "compact.ark", tmp_path / "sparse.ark"
        pkg.infer.write_posterior_archive(a, [("utt%d" % u, c[0], c[1]) for u, c in enumerate(comp)], min_post=min_post)
        pkg.infer.write_posterior_archive(b, [("utt%d" % u, s[0], s[1], s[2]) for u, s in enumerate(sparse)], min_post=min_post)
        assert a.read_bytes() == b.read_bytes() and len(a.read_bytes()) > 300
        assert pkg.infer.read_posterior_archive(b) == pkg.infer.read_posterior_archive(a)
