"""-m gpu: the compact posteriors (tdnnf_align_posteriors_compact, csrc/align_fb.hip; include/tdnnf_hip.h "compact posteriors") on the shapes
of tests/test_gpu_posteriors.py -- the same boundaries decide the launch form -- and on graphs that stride the owner loop.

The bar is the dense call's BITS: the compact kernel runs the dense kernel's arithmetic in its order with the same owner per element, so
compact[t, k] scattered to [t, pdfs[k]] of a zero matrix equals the post_out of tdnnf_align_posteriors bit for bit, and so do logprob and ok.
So that the code is not only compared with itself, every case is also held to tests/posteriors_ref64.py at the bars of
tests/test_gpu_posteriors.py (its _close): logprob 1e-9 relative, posteriors one float32 ulp at `weight`, rows summing to weight.
The compact buffer lies between canaries and is pre-filled with a sentinel no posterior can be (they are >= 0): the canaries must survive
and no sentinel may -- every element of every block is written, though nothing is zeroed first."""
import numpy as np
import pytest
import torch

from tests import posteriors_ref64 as PR
from tests.gpu_util import Hip, dev, host
from tests.test_gpu_posteriors import _close, _same_bits, _transcripts

pytestmark = pytest.mark.gpu
F = np.float32
NINF = -np.inf
GUARD, CANARY, SENTINEL = 16, 123.0, -7.25


@pytest.fixture(scope="module")
def hip(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return Hip(pkg)


def _graph_of(graphs, utt_graph, u):
    return utt_graph[u] if utt_graph is not None else (0 if len(graphs) == 1 else u)


def _compact_raw(pkg, ag, y, frames, rows, stride, utt_graph, scale=1.0, weight=1.0):
    """the C call on a guarded buffer: (values [elems] with the canaries checked and no sentinel left, utt_begin, results [U, 2]), downloaded"""
    abi = pkg.hipabi
    lib = abi.load()
    n = len(frames)
    fr, rb = abi.iarr(frames), abi.iarr(rows)
    ug = abi.iarr(utt_graph) if utt_graph is not None else (None, None)
    begin = ag.posteriors_compact_layout(frames, utt_graph)
    elems = int(begin[-1])
    buf = torch.full((elems + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    buf[:GUARD] = CANARY
    buf[GUARD + elems:] = CANARY
    nbytes = ag.posteriors_workspace_bytes(utt_graph, frames)
    assert nbytes > 0
    ws = abi.workspace(nbytes)
    res = torch.full((n, 2), -5.0, dtype=torch.float64, device="cuda")
    abi.check(lib.tdnnf_align_posteriors_compact(ag.h, n, ug[1], fr[1], rb[1], int(stride), abi.pmat(y), float(scale), float(weight), abi.ptr(buf[GUARD:]),
                                                 elems, abi.ptr(res), abi.ptr(ws), nbytes, abi.stream()))
    b = host(buf)
    assert (b[:GUARD] == CANARY).all() and (b[GUARD + elems:] == CANARY).all(), "the call wrote outside its blocks"
    vals = b[GUARD:GUARD + elems]
    assert not (vals == SENTINEL).any(), "an element of a block was not written"
    return vals, begin, host(res)


def _scatter(vals, begin, u, T, pdfs, P):
    m = np.zeros((T, P), F)
    m[:, pdfs] = vals[begin[u]:begin[u + 1]].reshape(T, len(pdfs))
    return m


def _check(pkg, graphs, ys, utt_graph=None, scale=1.0, weight=1.0, ag=None, lp_floor=0.0):
    """dense and compact on the utterances' rows stacked: the bits agree, and both are within the bars of the float64 reference.
    Returns (the compact call as per-utterance (logprob, ok, scattered post), the references)."""
    graphs = [graphs] if isinstance(graphs, dict) else graphs
    ag = ag or pkg.hipabi.AlignGraphs(graphs)
    frames = [len(y) for y in ys]
    rows = np.concatenate([[0], np.cumsum(frames)[:-1]])
    y = dev(np.concatenate(ys) if sum(frames) else np.zeros((1, ag.P), F))  # (a call of zero-frame utterances reads no row)
    post, dres = ag.posteriors(y, frames, rows, 1, utt_graph, scale, weight, out=torch.full((y.shape[0], ag.P), SENTINEL, dtype=torch.float32, device="cuda"))
    post, dres = host(post), host(dres)
    dense = [(dres[u, 0], dres[u, 1], post[rows[u]:rows[u] + T]) for u, T in enumerate(frames)]
    vals, begin, res = _compact_raw(pkg, ag, y, frames, rows, 1, utt_graph, scale, weight)
    got, refs = [], []
    for u, T in enumerate(frames):
        gi = _graph_of(graphs, utt_graph, u)
        pdfs = ag.pdfs(gi)
        assert pdfs.dtype == np.int32 and pdfs.tolist() == sorted(set(np.asarray(graphs[gi]["pdf"]).tolist()))
        assert begin[u + 1] - begin[u] == T * len(pdfs)
        got.append((res[u, 0], res[u, 1], _scatter(vals, begin, u, T, pdfs, ag.P)))
        refs.append(PR.forward_backward(graphs[gi], ys[u], scale))
        _close(got[u], refs[u], weight, "utterance %d" % u, lp_floor if T == 0 else 0.0)
    _same_bits(got, dense)
    return got, refs


# ------------------------------------------------------------------------------------------------------------------------- transcript graphs
@pytest.mark.parametrize("scale,weight", [(1.0, 1.0), (0.3, 0.25)])
def test_mixed_call(pkg, hip, scale, weight):
    """three transcript graphs of different sizes, five utterances of 0, 1, 7, 23 and 12 frames, two pairs sharing a graph; then one graph
    per utterance without utt_graph; twice: the same bits"""
    graphs = _transcripts(pkg)
    assert len({g["S"] for g in graphs}) == 3
    rng = np.random.default_rng(5)
    ys = [rng.standard_normal((T, 40)).astype(F) * 3 for T in (0, 1, 7, 23, 12)]
    ag = pkg.hipabi.AlignGraphs(graphs)
    got, refs = _check(pkg, graphs, ys, utt_graph=[2, 0, 1, 2, 1], scale=F(scale), weight=F(weight), ag=ag)
    assert [r["ok"] for r in refs] == [False, True, True, True, True]
    again, _ = _check(pkg, graphs, ys, utt_graph=[2, 0, 1, 2, 1], scale=F(scale), weight=F(weight), ag=ag)
    _same_bits(got, again)
    _, refs = _check(pkg, graphs, [ys[1], ys[2], ys[3]], scale=F(scale), weight=F(weight), ag=ag)
    assert all(r["ok"] for r in refs)


@pytest.mark.parametrize("S", [64, 65, 1024, 1025])
def test_block_size_boundaries_cyclic(pkg, hip, S):
    """64 threads up to 64 states, 256 up to 1024, 1024 above: the last graph of each size and the first of the next"""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(S, 50, mean_out_degree=4.0, seed=S))
    rng = np.random.default_rng(S)
    _, refs = _check(pkg, g, [rng.standard_normal((T, 50)).astype(F) for T in (9, 4)])
    assert all(r["ok"] for r in refs)


def _labelled(S, pdf, seed):
    """a cyclic graph of S states, every state initial and final, with one arc per entry of pdf (shuffled): a ring first, so every length
    has a path, the rest between random states"""
    rng = np.random.default_rng(seed)
    n = len(pdf)
    assert n >= S
    src = np.concatenate([np.arange(S), rng.integers(0, S, size=n - S)]).astype(np.int32)
    dst = np.concatenate([(np.arange(S) + 1) % S, rng.integers(0, S, size=n - S)]).astype(np.int32)
    return {"S": S, "P": int(max(pdf)) + 14, "src": src, "dst": dst, "pdf": rng.permutation(np.asarray(pdf)).astype(np.int32),
            "logprob": (-rng.random(n) * 2).astype(F), "init": (-rng.random(S)).astype(F), "final": (-rng.random(S)).astype(F)}


@pytest.mark.parametrize("S,D", [(40, 65), (40, 129), (100, 257)])
def test_owner_loop_strides(pkg, hip, S, D):
    """more distinct pdfs than the workgroup has threads -- over 64 and over 128 at 64 threads, 257 at 256 -- so the loop over the by-pdf
    slots takes a second and a third turn; some pdfs below, between and above the named ones are on no arc"""
    ids = 3 + 2 * np.arange(D)  # odd pdfs only
    g = _labelled(S, np.concatenate([ids, ids[:D // 2], ids[:7]]), D)
    ag = pkg.hipabi.AlignGraphs(g)
    assert ag.pdfs().tolist() == ids.tolist() and g["P"] > ids[-1] + 1
    rng = np.random.default_rng(D)
    _, refs = _check(pkg, g, [rng.standard_normal((T, g["P"])).astype(F) for T in (5, 2)], ag=ag, weight=F(0.5))
    assert all(r["ok"] for r in refs)


@pytest.mark.parametrize("heavy", [65, 300])
def test_heavy_pdf_rows(pkg, hip, heavy):
    """one pdf on more than 64 arcs (a wave walks its row, and at 300 its lanes take several arcs each) between light ones: its column,
    neither the first nor the last, comes from the heavy-row descriptor; the pdf on exactly 64 arcs is the longest light row"""
    pdf = np.concatenate([np.full(heavy, 9), np.full(64, 4), np.full(3, 2), np.full(20, 11), np.full(1, 30)])
    g = _labelled(50, pdf, heavy)
    ag = pkg.hipabi.AlignGraphs(g)
    assert ag.pdfs().tolist() == [2, 4, 9, 11, 30]
    rng = np.random.default_rng(heavy)
    _, refs = _check(pkg, g, [rng.standard_normal((T, g["P"])).astype(F) * 2 for T in (8, 3)], ag=ag)
    assert all(r["ok"] for r in refs)


# ------------------------------------------------------------------------------------------------------------------------- staging thresholds
@pytest.mark.parametrize("S,P", [(30, 512), (30, 513), (100, 2048), (100, 2049)])
def test_row_staging_threshold(pkg, hip, S, P):
    """output rows staged in LDS up to 8 floats a thread -- 512 pdfs at 64 threads, 2048 at 256 -- and gathered from global memory above"""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(S, P, mean_out_degree=6.0, seed=P))
    rng = np.random.default_rng(P)
    _check(pkg, g, [rng.standard_normal((T, P)).astype(F) for T in (7, 1, 2)])


@pytest.mark.parametrize("S", [6400, 6401, 9600, 9601])
def test_state_vector_thresholds(pkg, hip, S):
    """three vectors of doubles fit the LDS up to 6 400 states (alpha_t staged), two up to 9 600, none above (the workspace form)"""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(S, 50, mean_out_degree=3.0, seed=S))
    rng = np.random.default_rng(S)
    _, refs = _check(pkg, g, [rng.standard_normal((T, 50)).astype(F) for T in (3, 3)])
    assert all(r["ok"] for r in refs)


def test_both_forms(pkg, hip):
    """option align_form 1 (LDS) and 2 (workspace) is read as by the dense call: each form equals its dense call, and the forms each other"""
    den = pkg.synth.make_den_graph(H=300, P=50)
    g = pkg.synth.alignment_graph_from_den(den)
    ag = pkg.hipabi.AlignGraphs(g)
    rng = np.random.default_rng(9)
    ys = [rng.standard_normal((12, 50)).astype(F) * 4 for _ in range(3)]
    res = {}
    for form in (1, 2):
        with pkg.hipabi.option("align_form", form):
            res[form], _ = _check(pkg, g, ys, utt_graph=[0, 0, 0], ag=ag)
    _same_bits(res[1], res[2])
    with pkg.hipabi.option("align_form", 3):
        lib = pkg.hipabi.load()
        y = dev(np.concatenate(ys))
        fr, rb = pkg.hipabi.iarr([12] * 3), pkg.hipabi.iarr([0, 12, 24])
        out = torch.zeros(36 * 50, dtype=torch.float32, device="cuda")
        ws = hip.ws(1 << 20)
        r = torch.zeros(6, dtype=torch.float64, device="cuda")
        assert lib.tdnnf_align_posteriors_compact(ag.h, 3, None, fr[1], rb[1], 1, pkg.hipabi.pmat(y), 1.0, 1.0, hip.vec(out), 36 * 50, hip.vec(r), hip.vec(ws),
                                                  1 << 20, hip.stream()) == 1
        assert lib.tdnnf_last_error().startswith(b"align_posteriors_compact: ") and b"align_form" in lib.tdnnf_last_error()


# ------------------------------------------------------------------------------------------------------------------------- failing and empty utterances
def test_no_accepting_path_leaves_neighbours_alone(pkg, hip):
    graphs = _transcripts(pkg)
    rng = np.random.default_rng(8)
    ys = [rng.standard_normal((T, 40)).astype(F) for T in (12, 2, 30)]  # graph 1 needs at least 3 frames
    got, refs = _check(pkg, graphs, ys)
    assert [r["ok"] for r in refs] == [True, False, True]
    assert got[1][0] == NINF and got[1][1] == 0.0 and got[1][2].shape == (2, 40) and (got[1][2] == 0).all()  # (and no sentinel: _compact_raw)
    alone, _ = _check(pkg, [graphs[0], graphs[2]], [ys[0], ys[2]])
    _same_bits(alone, [got[0], got[2]])


def test_call_of_zero_frame_utterances(pkg, hip):
    """elems = 0: a null buffer is accepted, logprob = LSE(init + final) as in the dense call"""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(H=70, P=20, mean_out_degree=4.0, seed=6))
    t = pkg.synth.make_alignment_graph([1, 2], num_pdfs=20)
    ag = pkg.hipabi.AlignGraphs([t, g])
    ys = [np.zeros((0, 20), F)] * 3
    got, refs = _check(pkg, [t, g], ys, utt_graph=[0, 1, 0], ag=ag, lp_floor=2.6e-15)  # (the floor of tests/test_gpu_posteriors.py for this graph)
    assert [r["ok"] for r in refs] == [False, True, False]
    assert ag.posteriors_compact_layout([0, 0, 0], [0, 1, 0]).tolist() == [0, 0, 0, 0]
    lib, abi = pkg.hipabi.load(), pkg.hipabi
    fr, rb, ug = abi.iarr([0, 0, 0]), abi.iarr([0, 0, 0]), abi.iarr([0, 1, 0])
    nbytes = ag.posteriors_workspace_bytes([0, 1, 0], [0, 0, 0])
    ws, res = hip.ws(nbytes), torch.full((3, 2), -5.0, dtype=torch.float64, device="cuda")
    y = dev(np.zeros((1, 20), F))
    abi.check(lib.tdnnf_align_posteriors_compact(ag.h, 3, ug[1], fr[1], rb[1], 1, abi.pmat(y), 1.0, 1.0, None, 0, hip.vec(res), hip.vec(ws), nbytes, hip.stream()))
    r = host(res)
    assert np.array_equal(r[:, 0].view(np.int64), np.asarray([x[0] for x in got]).view(np.int64)) and r[:, 1].tolist() == [0.0, 1.0, 0.0]
    v, begin, res2 = ag.posteriors_compact(y, [0, 0, 0], [0, 0, 0], utt_graph=[0, 1, 0])  # the wrapper passes the null buffer itself
    assert v.numel() == 0 and begin.dtype == np.int64 and np.array_equal(host(res2), r)


# ------------------------------------------------------------------------------------------------------------------------- layouts, guards
def test_t_major_rows_in_a_guarded_view(pkg, hip):
    """row_stride = B on a t-major minibatch, read through a sub-matrix view (stride above its columns) whose surrounding columns and rows
    hold NaN: the same bits as the rows concatenated"""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(H=90, P=20, mean_out_degree=5.0, seed=2))
    ag = pkg.hipabi.AlignGraphs(g)
    rng = np.random.default_rng(4)
    B, frames, P = 3, [11, 5, 8], 20
    tmajor = rng.standard_normal((max(frames) * B, P)).astype(F)
    ys = [tmajor[u::B][:frames[u]] for u in range(B)]
    cat, refs = _check(pkg, g, ys, utt_graph=[0, 0, 0], ag=ag)
    buf = torch.full((max(frames) * B + 4, P + 9), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[2:2 + max(frames) * B, 3:3 + P]
    view.copy_(dev(tmajor))
    assert view.stride(0) > view.shape[1] and not torch.isnan(view).any()
    vals, begin, res = _compact_raw(pkg, ag, view, frames, np.arange(B), B, [0, 0, 0])
    pdfs = ag.pdfs()
    got = [(res[u, 0], res[u, 1], _scatter(vals, begin, u, T, pdfs, P)) for u, T in enumerate(frames)]
    _same_bits(got, cat)
    assert np.isfinite(vals).all() and all(r["ok"] for r in refs)
    # the wrapper: the same values, views of one tensor
    v, b, r = ag.posteriors_compact(view, frames, np.arange(B), row_stride=B, utt_graph=[0, 0, 0])
    assert v.dtype == torch.float32 and v.is_cuda and b.dtype == np.int64 and b.tolist() == begin.tolist() and r.dtype == torch.float64 and tuple(r.shape) == (B, 2)
    assert np.array_equal(host(v).view(np.int32), vals.view(np.int32)) and np.array_equal(host(r).view(np.int64), res.view(np.int64))


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(pkg, hip):
    lib, abi = hip.lib, pkg.hipabi
    g = pkg.synth.make_alignment_graph([1, 2, 3], num_pdfs=5)
    ag = abi.AlignGraphs(g, num_pdfs=5)
    D = len(ag.pdfs())
    assert D == 3 and ag.posteriors_compact_layout([4, 6]).tolist() == [0, 4 * D, 10 * D]
    frames, rows = abi.iarr([4, 6]), abi.iarr([0, 4])
    y = dev(np.zeros((10, 5), F))
    nbytes = ag.posteriors_workspace_bytes(None, [4, 6])
    ws = hip.ws(nbytes)
    out = torch.full((10 * D,), SENTINEL, dtype=torch.float32, device="cuda")
    res = torch.full((4,), -5.0, dtype=torch.float64, device="cuda")
    call = lambda elems, nb, out_=out, y_=y, rows_=rows, stride=1: lib.tdnnf_align_posteriors_compact(
        ag.h, 2, None, frames[1], rows_[1], stride, abi.pmat(y_), 1.0, 1.0, hip.vec(out_) if out_ is not None else None, elems, hip.vec(res), hip.vec(ws), nb,
        hip.stream())
    named = lambda: lib.tdnnf_last_error().startswith(b"align_posteriors_compact: ")
    assert call(10 * D - 1, nbytes) == 1 and named() and b"post_compact_elems" in lib.tdnnf_last_error()
    assert call(10 * D, nbytes - 1) == 1 and named() and b"workspace" in lib.tdnnf_last_error()
    assert call(10 * D, nbytes, out_=None) == 1 and named() and b"post_compact_dev" in lib.tdnnf_last_error()
    assert call(10 * D, nbytes, rows_=abi.iarr([0, 5])) == 1 and named() and b"rows" in lib.tdnnf_last_error()  # rows 5 .. 10 of 10
    assert call(10 * D, nbytes, y_=dev(np.zeros((10, 4), F))) == 1 and named() and b"columns" in lib.tdnnf_last_error()
    assert call(10 * D, nbytes, stride=0) == 1 and named()
    e = abi.iarr([0])
    assert lib.tdnnf_align_posteriors_compact_layout(ag.h, 2, abi.iarr([0, 1])[1], frames[1], None, None) == 1  # graph 1 of 1
    assert lib.tdnnf_last_error().startswith(b"align_posteriors_compact_layout: ")
    assert lib.tdnnf_align_posteriors_compact_layout(ag.h, 2, None, abi.iarr([4, -1])[1], None, None) == 1
    assert lib.tdnnf_align_graphs_pdfs(ag.h, 1, e[1], None) == 1 and lib.tdnnf_last_error().startswith(b"align_graphs_pdfs: ")
    assert (host(out) == SENTINEL).all() and (host(res) == -5.0).all()  # nothing was launched
    assert call(10 * D, nbytes) == 0
    assert (host(res)[[1, 3]] == 1.0).all() and np.abs(host(out).reshape(10, D).sum(1, dtype=np.float64) - 1.0).max() <= 1e-6


# ------------------------------------------------------------------------------------------------------------------------- the model
def test_acoustic_model_posteriors_compact_and_archive(pkg, hip, tmp_path):
    from tests.test_gpu_infer import SMALL, make_model, utterances
    cfg, net = make_model(pkg, SMALL)
    model = pkg.infer.AcousticModel(net, frames_per_chunk=24)
    rng = np.random.default_rng(17)
    utts = utterances(rng, [50, 7, 95])
    P = cfg.num_pdfs
    graphs = [pkg.synth.make_alignment_graph(rng.integers(0, P, size=n).tolist(), optional=[1], num_pdfs=P, seed=n) for n in (6, 2, 40)]
    ag = pkg.hipabi.AlignGraphs(graphs)
    dense = model.posteriors(utts, ag, acoustic_scale=1.0)
    comp = model.posteriors_compact(utts, ag, acoustic_scale=1.0)
    again = pkg.infer.posteriors_compact(model.compute(utts), ag, acoustic_scale=1.0)
    assert [c[3] for c in comp] == [True, True, False]  # (32 output frames for a transcript of at least 39 units)
    for u, (d, c, a) in enumerate(zip(dense, comp, again)):
        ids, post, lp, ok = c
        assert ids.dtype == np.int32 and np.array_equal(ids, ag.pdfs(u)) and post.dtype == torch.float32 and post.is_cuda
        assert tuple(post.shape) == (d[0].shape[0], len(ids)) and lp == d[1] == a[2] and ok == d[2] == a[3]
        m = np.zeros(tuple(d[0].shape), F)
        m[:, ids] = host(post)
        assert np.array_equal(m.view(np.int32), host(d[0]).view(np.int32)) and np.array_equal(host(a[1]), host(post))
    # shared graphs through utt_graph and a weight: views of one tensor, per utterance its graph's list
    c2 = pkg.infer.posteriors_compact(model.compute(utts), ag, utt_graph=[0, 1, 0], weight=0.5)
    assert np.array_equal(c2[2][0], ag.pdfs(0)) and c2[2][3] and abs(float(host(c2[2][1]).sum(1, dtype=np.float64).mean()) - 0.5) < 1e-6
    for min_post in (0.0, 1e-4):
        a, b = tmp_path / "dense.ark", tmp_path / "compact.ark"
        pkg.infer.write_posterior_archive(a, [("utt%d" % u, d[0]) for u, d in enumerate(dense)], min_post=min_post)
        pkg.infer.write_posterior_archive(b, [("utt%d" % u, c[0], c[1]) for u, c in enumerate(comp)], min_post=min_post)
        assert a.read_bytes() == b.read_bytes() and len(a.read_bytes()) > 300
